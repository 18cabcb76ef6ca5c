// tde_vector_obs.hip — the vector observation of tde_vector_obs (include/tde_hip.h: the K nearest agents in the ego frame, ray
// distances to the road edge, to other cars and to red stop lines) and its launcher.  One wavefront per env, kVoWaves envs per
// workgroup (a one-env workgroup costs ~8 us per launch at 8192 envs even with nothing to do, profiles/near_field_kernel_stats.txt).
//   * the env's other present agents are staged in LDS as boxes; neighbours are ranked by their (d2 bits, slot) keys - the rank of a
//     key is the number of smaller keys, so the k nearest write themselves to their entries without a sort
//   * one lane per ray: the car and red-line channels are slab tests against the boxes in LDS (the red lines of the env's map in
//     chunks of 64); the road channel marches the ray's samples in batches of kVoBatch whose class-map look-ups are issued together,
//     skips the samples that a FULL coarse tile's clearance proves on the road, and resolves a sample in a MIXED cell against the
//     cell's candidate triangles as offroad_resolve does
// The specification is restated in numpy by tests/vector_obs_ref.py.
#include "tde_kernels.h"
#include "tde_host.h"

namespace tde {

constexpr int kVoWaves = 4;         // envs per workgroup
#ifndef TDE_VO_BATCH
#define TDE_VO_BATCH 8
#endif
constexpr int kVoBatch = TDE_VO_BATCH;  // road samples whose look-ups are in flight together
constexpr float kVoSkipMargin = 0.05f;  // metres taken off a coarse tile's clearance: the fp32 error of the sample positions

struct VoWave {
    float4 box[TDE_MAX_AGENTS];                 // the other present agents: x, y, c, s
    float2 ext[TDE_MAX_AGENTS];                 // half length, half width
    unsigned long long key[TDE_MAX_AGENTS];     // (d2 bits << 32) | slot of the neighbour candidates, ~0 otherwise (by slot)
    float4 lbox[kWave];                         // a chunk of red stop lines: x, y, c, s
    float2 lext[kWave];                         //                            hl, hw
};

// per axis of a box: the ray's parameter interval inside the slab |o + t d| <= h
TDE_DEV void vo_slab(float o, float d, float h, float &lo, float &hi)
{
    if (d == 0.0f) {
        const bool in = -h <= o && o <= h;
        lo = in ? -INFINITY : INFINITY;
        hi = in ? INFINITY : -INFINITY;
    } else {
        const float ta = (-h - o) / d, tb = (h - o) / d;
        lo = fminf(ta, tb);
        hi = fmaxf(ta, tb);
    }
}

// entry distance of the ray (x0, y0) + t (ux, uy) into the box (b.x, b.y, c = b.z, s = b.w, half extents h); +inf on a miss
TDE_DEV float vo_ray_box(float x0, float y0, float ux, float uy, float4 b, float2 h)
{
    const float rx = x0 - b.x, ry = y0 - b.y;
    const float o0 = rx * b.z + ry * b.w, o1 = ry * b.z - rx * b.w;
    const float d0 = ux * b.z + uy * b.w, d1 = uy * b.z - ux * b.w;
    float lo0, hi0, lo1, hi1;
    vo_slab(o0, d0, h.x, lo0, hi0);
    vo_slab(o1, d1, h.y, lo1, hi1);
    const float tn = fmaxf(lo0, lo1), tf = fminf(hi0, hi1);
    return (tn <= tf && tf >= 0.0f) ? fmaxf(tn, 0.0f) : INFINITY;
}

// class | clearance << 2 of the coarse tile that holds the cell of (px, py) (the clamp of cell_class_lookup; tde_abi.h: cell_coarse)
TDE_DEV uint32_t vo_coarse(const tde_world &w, const tde_map &m, float px, float py)
{
    const float fx = __builtin_amdgcn_fmed3f((px - m.ox) * m.inv_cell, 0.0f, (float)(m.nx - 1));
    const float fy = __builtin_amdgcn_fmed3f((py - m.oy) * m.inv_cell, 0.0f, (float)(m.ny - 1));
    static_assert(TDE_COARSE_CELLS == 4, "coarse tiles of 4 x 4 cells");
    const uint32_t cx = (uint32_t)(int)fx >> 2, cy = (uint32_t)(int)fy >> 2;
    const uint32_t line = (uint32_t)m.coarse_base + ((cy >> 3) << (m.row_shift - 6)) + (cx >> 4);
    return w.cell_coarse[(line << 7) | (((cy & 7u) << 4) | (cx & 15u))];
}

// class of the sub-cell of (px, py) in its cell (meaningful for a MIXED cell; tde_abi.h: cell_sub, the rasteriser's subcell_class)
TDE_DEV uint32_t vo_subcell(const tde_world &w, const tde_map &m, float px, float py)
{
    const float fx = __builtin_amdgcn_fmed3f((px - m.ox) * m.inv_cell, 0.0f, (float)(m.nx - 1));
    const float fy = __builtin_amdgcn_fmed3f((py - m.oy) * m.inv_cell, 0.0f, (float)(m.ny - 1));
    const uint32_t ix = (uint32_t)(int)fx, iy = (uint32_t)(int)fy;
    const uint32_t tile = ((iy >> 2) << (m.row_shift - 3)) + (ix >> 3);
    const uint32_t bm = w.cell_sub[(uint32_t)m.cell_base + ((tile << 5) | (((iy & 3u) << 3) | (ix & 7u)))];
    const int sx = min((int)(__builtin_amdgcn_fractf(fx) * (float)TDE_CELL_SUB), TDE_CELL_SUB - 1);
    const int sy = min((int)(__builtin_amdgcn_fractf(fy) * (float)TDE_CELL_SUB), TDE_CELL_SUB - 1);
    return (bm >> (2 * (sy * TDE_CELL_SUB + sx))) & 3u;
}

// a point of a MIXED sub-cell: on the road when one of the cell's candidate triangles is within the threshold
TDE_DEV bool vo_mixed_off(const tde_world &w, const tde_map &m, float px, float py, float thr2)
{
    const uint32_t wd = cell_lookup(w, m, px, py);
    const float4 *recs = reinterpret_cast<const float4 *>(w.cell_tri);
    uint32_t cur = (wd >> 10) + (uint32_t)m.rec_base;
    const uint32_t end = cur + ((wd >> 2) & 255u);
    for (; cur < end; cur += 2) {                             // two records per trip (offroad_resolve's PAIR form)
        const float4 *r0 = recs + 3 * (size_t)cur, *r1 = recs + 3 * (size_t)(cur + 1 < end ? cur + 1 : cur);
        const float4 a0 = r0[0], a1 = r0[1], a2 = r0[2], b0 = r1[0], b1 = r1[1], b2 = r1[2];
        if (point_tri_d2_words(px, py, a0, a1, a2) <= thr2) return false;
        if (cur + 1 < end && point_tri_d2_words(px, py, b0, b1, b2) <= thr2) return false;
    }
    return true;
}

// the road channel of one ray over its samples j0..j1: the first j off the road, INT_MAX without one
TDE_DEV int vo_road(const tde_world &w, const tde_map &m, float x0, float y0, float ux, float uy, float step, int j0, int j1, float thr2)
{
    const int M = j1;
    for (int j = j0; j <= M;) {
        uint32_t cls[kVoBatch];
#pragma unroll
        for (int i = 0; i < kVoBatch; ++i) {                  // (independent look-ups, all in flight before the first is used)
            const float t = (float)min(j + i, M) * step;
            cls[i] = cell_class_lookup(w, m, x0 + t * ux, y0 + t * uy) & 3u;
        }
        const float t0 = (float)j * step;
        const uint32_t co = vo_coarse(w, m, x0 + t0 * ux, y0 + t0 * uy);
        // a FULL tile under sample j with clearance R: every sample closer than R to it lies in a FULL cell
        // (sample j itself lies in the tile: covered >= 0 exempts it; -1 = nothing proved)
        int covered = -1;
        if ((co & 3u) == TDE_CELL_FULL) covered = max(0, (int)(((float)(co >> 2) * TDE_COARSE_UNIT - kVoSkipMargin) / step));
        uint32_t empty = 0u, mixed = 0u;
#pragma unroll
        for (int i = 0; i < kVoBatch; ++i) {
            const bool in = j + i <= M && i > covered;
            empty |= (in && cls[i] == TDE_CELL_EMPTY) ? 1u << i : 0u;
            mixed |= (in && cls[i] == TDE_CELL_MIXED) ? 1u << i : 0u;
        }
        // the samples in MIXED cells: their sub-cell classes, fetched together; only a MIXED sub-cell walks the candidate triangles
        uint32_t sub_e = 0u, sub_m = 0u;
        if (mixed) {
            uint32_t sc[kVoBatch];
#pragma unroll
            for (int i = 0; i < kVoBatch; ++i) {
                const float t = (float)min(j + i, M) * step;
                sc[i] = vo_subcell(w, m, x0 + t * ux, y0 + t * uy);
            }
#pragma unroll
            for (int i = 0; i < kVoBatch; ++i) {
                const bool mi = ((mixed >> i) & 1u) != 0u;
                sub_e |= (mi && sc[i] == TDE_CELL_EMPTY) ? 1u << i : 0u;
                sub_m |= (mi && sc[i] == TDE_CELL_MIXED) ? 1u << i : 0u;
            }
        }
        const uint32_t off_now = empty | sub_e;
        for (uint32_t pend = off_now | sub_m; pend; pend &= pend - 1u) {    // in sample order
            const int i = __ffs((int)pend) - 1;
            const float t = (float)(j + i) * step;
            if ((off_now >> i) & 1u) return j + i;
            if (vo_mixed_off(w, m, x0 + t * ux, y0 + t * uy, thr2)) return j + i;
        }
        j += max(kVoBatch, covered + 1);
    }
    return INT_MAX;
}

__global__ __launch_bounds__(kWave * kVoWaves) void vector_obs_kernel(tde_config cfg, tde_world w, tde_state st, struct tde_vector_obs vo,
                                                                    const uint8_t *only, float *out)
{
    __shared__ VoWave shw[kVoWaves];
    const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int e = (int)blockIdx.x * kVoWaves + wv;
    if (e >= st.B || (only && !only[e])) return;             // (wave-uniform; no workgroup barrier below)
    VoWave &sh = shw[wv];
    const int A = st.A;
    const int64_t base = (int64_t)e * A;
    const int kn = vo.k_nbr, nr = vo.n_rays;
    float *row = out + (int64_t)e * (TDE_VO_EGO + TDE_VO_NBR * kn + TDE_VO_RAY * nr);
    const float x0 = st.x[base], y0 = st.y[base], v0 = st.v[base];
    float s0, c0;
    sincos_f32(st.psi[base], s0, c0);
    const int s = st.scn[e];
    const tde_scenario sc = w.scn[s];
    const tde_map m = w.maps[sc.map];
    const int steps = st.steps[e], ti = st.target_idx[e];

    // ---- ego block
    if (lane < 2) {
        const int j = ti + lane;
        float fwd = 0.0f, lat = 0.0f;
        if (j < sc.wp_n) {
            const double2 t = reinterpret_cast<const double2 *>(w.wp_xy)[(int64_t)s * w.NW + j];
            const float dx = (float)t.x - x0, dy = (float)t.y - y0;
            fwd = dx * c0 + dy * s0;
            lat = dy * c0 - dx * s0;
        }
        row[3 + 2 * lane] = fwd;
        row[4 + 2 * lane] = lat;
    } else if (lane == 2) {
        row[0] = v0;
        row[1] = st.len[base];
        row[2] = st.wid[base];
        row[7] = (float)min(max(sc.wp_n - ti, 0), 2);
        row[8] = (float)steps / (float)cfg.max_steps;
        row[9] = (m.n_stop > 0 && m.cycle_steps > 0) ? 1.0f : 0.0f;
    }

    // ---- the other present agents: boxes in LDS (compacted), neighbour keys by slot
    const float r2 = vo.nbr_radius * vo.nbr_radius;
    float fx[2], fy[2], cr[2], sr[2], va[2], la[2], wa[2];
    unsigned long long mykey[2];
    int nb = 0, ncand = 0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int a = p * kWave + lane;
        mykey[p] = ~0ull;
        if (p * kWave >= A) break;                            // (wave-uniform)
        const bool live = a > 0 && a < A && st.present[base + a] != 0;
        float4 b = make_float4(0.0f, 0.0f, 1.0f, 0.0f);
        float2 h = make_float2(0.0f, 0.0f);
        bool cand = false;
        if (live) {
            const int64_t g = base + a;
            const float x = st.x[g], y = st.y[g];
            float sa, ca;
            sincos_f32(st.psi[g], sa, ca);
            la[p] = st.len[g];
            wa[p] = st.wid[g];
            va[p] = st.v[g];
            b = make_float4(x, y, ca, sa);
            h = make_float2(0.5f * la[p], 0.5f * wa[p]);
            const float dx = x - x0, dy = y - y0;
            const float d2 = dx * dx + dy * dy;
            cand = d2 < r2;
            fx[p] = dx * c0 + dy * s0;
            fy[p] = dy * c0 - dx * s0;
            cr[p] = ca * c0 + sa * s0;
            sr[p] = sa * c0 - ca * s0;
            if (cand) mykey[p] = ((unsigned long long)__float_as_uint(d2) << 32) | (uint32_t)a;
        }
        const unsigned long long bl = __ballot(live);
        if (live) {
            const int q = nb + lane_prefix(bl);
            sh.box[q] = b;
            sh.ext[q] = h;
        }
        nb += __popcll(bl);
        ncand += __popcll(__ballot(cand));
        if (a < A) sh.key[a] = mykey[p];
    }
    wave_lds_fence();

    // ---- neighbour block: the entry of a candidate is its rank among the candidates' keys
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (p * kWave >= A) break;
        const unsigned long long k = mykey[p];
        if (k != ~0ull) {
            int rank = 0;
            for (int b = 0; b < A; ++b) rank += sh.key[b] < k ? 1 : 0;
            if (rank < kn) {
                float *en = row + TDE_VO_EGO + TDE_VO_NBR * rank;
                en[0] = 1.0f;
                en[1] = fx[p];
                en[2] = fy[p];
                en[3] = cr[p];
                en[4] = sr[p];
                en[5] = va[p] * cr[p] - v0;
                en[6] = va[p] * sr[p];
                en[7] = la[p];
                en[8] = wa[p];
            }
        }
    }
    for (int i = ncand + lane; i < kn; i += kWave) {
        float *en = row + TDE_VO_EGO + TDE_VO_NBR * i;
#pragma unroll
        for (int q = 0; q < TDE_VO_NBR; ++q) en[q] = 0.0f;
    }

    // ---- ray block: one lane per ray
    const bool ray = lane < nr;
    const float L = vo.ray_range;
    float ux = 0.0f, uy = 0.0f;
    if (ray) {
        const float2 rd = reinterpret_cast<const float2 *>(vo.ray_dir)[lane];
        ux = rd.x * c0 - rd.y * s0;
        uy = rd.x * s0 + rd.y * c0;
    }
    float car = L, redl = L;
    if (ray)
        for (int i = 0; i < nb; ++i) car = fminf(car, vo_ray_box(x0, y0, ux, uy, sh.box[i], sh.ext[i]));
    const uint32_t red = ((cfg.flags & TDE_F_TRAFFIC_LIGHTS) && m.n_stop > 0) ? red_mask(w, m, steps) : 0u;
    if (red) {
        for (int q0 = 0; q0 < m.n_stop; q0 += kWave) {
            const int q = q0 + lane;
            bool on = false;
            tde_stopline ln;
            if (q < m.n_stop) {
                ln = w.stoplines[m.stop_base + q];
                on = ((red >> ((uint32_t)ln.light & 31u)) & 1u) != 0u;
            }
            const unsigned long long bl = __ballot(on);
            if (on) {
                const int r = lane_prefix(bl);
                sh.lbox[r] = make_float4(ln.x, ln.y, ln.c, ln.s);
                sh.lext[r] = make_float2(ln.hl, ln.hw);
            }
            wave_lds_fence();
            const int nl = __popcll(bl);
            if (ray)
                for (int i = 0; i < nl; ++i) redl = fminf(redl, vo_ray_box(x0, y0, ux, uy, sh.lbox[i], sh.lext[i]));
            wave_lds_fence();                                 // (the next chunk overwrites the boxes)
        }
    }
    // road channel: the 64 / P lanes of ray k = lane % P (P = n_rays rounded up to a power of two) march consecutive segments of its
    // samples side by side; the earliest hit over the segments is the ray's
    if (nr > 0) {
        int P = 1;
        while (P < nr) P <<= 1;
        const int k = lane & (P - 1), G = kWave / P, seg = lane / P;
        const int M = (int)(L / vo.ray_step);
        const int S = (M + G - 1) / G;
        int hit = INT_MAX;
        const int j0 = seg * S + 1, j1 = min(seg * S + S, M);
        if (k < nr && j0 <= j1) {
            const float2 rd = reinterpret_cast<const float2 *>(vo.ray_dir)[k];
            const float vx = rd.x * c0 - rd.y * s0, vy = rd.x * s0 + rd.y * c0;
            hit = vo_road(w, m, x0, y0, vx, vy, vo.ray_step, j0, j1, thr2_of(cfg));
        }
        for (int o = P; o < kWave; o <<= 1) hit = min(hit, __shfl_xor(hit, o));
        if (ray) {
            float *rr = row + TDE_VO_EGO + TDE_VO_NBR * kn + TDE_VO_RAY * lane;
            rr[0] = hit == INT_MAX ? L : (float)hit * vo.ray_step;
            rr[1] = car;
            rr[2] = redl;
        }
    }
}

}  // namespace tde

namespace tde_host {

int launch_vector_obs(const tde_config *cfg, const tde_world *world, const tde_state *st, const struct tde_vector_obs *vo,
                      const uint8_t *only, float *out, void *stream)
{
    const unsigned nb = (unsigned)((st->B + tde::kVoWaves - 1) / tde::kVoWaves);
    tde::vector_obs_kernel<<<nb, tde::kWave * tde::kVoWaves, 0, (hipStream_t)stream>>>(*cfg, *world, *st, *vo, only, out);
    return launch_status("tde_vector_obs");
}

}  // namespace tde_host
