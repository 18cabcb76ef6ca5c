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
#include "tde_vector_obs_dev.h"

namespace tde {

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
