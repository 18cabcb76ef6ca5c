// tde_agents.hip — the entry points of include/tde_agents.h and their kernels: the vector observation taken from any (env, slot) pair
// (agent_obs_kernel) and each pair's reward and flags after the step(s) that followed (agent_outcomes_kernel).
//   * agent_obs_kernel is vector_obs_kernel (tde_vector_obs.hip) with the pair's slot as the observer: one wavefront per pair, kVoWaves
//     pairs per workgroup, one lane per ray, no workgroup barrier; the boxes in LDS are those of the present slots other than the
//     observer (the ego among them), the waypoint entries of a slot >= 1 come from its route.  The LDS block, the slab test and the road
//     march are the shared helpers of tde_vector_obs_dev.h, so a pair with slot 0 gives tde_vector_obs's row bit for bit.
//   * agent_outcomes_kernel: one lane per pair; the reward is reward_core's pieces (tde_device.h) on the pose the track holds and the
//     pose the state holds now.
// The specification is restated in numpy by tests/agent_obs_ref.py.
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_vector_obs_dev.h"
#include "../../include/tde_agents.h"

namespace tde {

__global__ __launch_bounds__(kWave * kVoWaves) void agent_obs_kernel(tde_config cfg, tde_world w, tde_state st, struct tde_vector_obs vo,
                                                                   const int32_t *pairs, int n, float *out, tde_agent_track *track)
{
    __shared__ VoWave shw[kVoWaves];
    const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    // the pair's index is the same in every lane of the wavefront: taken through readfirstlane, so that the pair, its indices and the
    // observer's own words are scalar loads (and scalar registers: 5 wavefronts per SIMD, as vector_obs_kernel)
    const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kVoWaves + wv);
    if (i >= n) return;                                       // (wave-uniform; no workgroup barrier below)
    VoWave &sh = shw[wv];
    const int A = st.A;
    const int e = pairs[2 * (int64_t)i], ao = pairs[2 * (int64_t)i + 1];
    const int kn = vo.k_nbr, nr = vo.n_rays;
    const int D = TDE_VO_EGO + TDE_VO_NBR * kn + TDE_VO_RAY * nr;
    float *row = out + (int64_t)i * D;
    const bool in_range = e >= 0 && e < st.B && ao >= 0 && ao < A;
    const int es = in_range ? e : 0;                          // (a row that exists: the loads below go out beside the presence byte)
    const int64_t base = (int64_t)es * A;
    const int64_t g0 = base + (in_range ? ao : 0);
    const uint8_t here = st.present[g0];
    const float x0 = st.x[g0], y0 = st.y[g0], v0 = st.v[g0], psi0 = st.psi[g0];
    const int s = st.scn[es], steps = st.steps[es];
    if (!in_range || here == 0) {                             // (wave-uniform) nothing to observe: zeros, and a track that says so
        for (int q = lane; q < D; q += kWave) row[q] = 0.0f;
        if (track && lane < 8) reinterpret_cast<uint32_t *>(track + i)[lane] = 0u;
        return;
    }
    float s0, c0;
    sincos_f32(psi0, s0, c0);
    const tde_scenario sc = w.scn[s];
    const tde_map m = w.maps[sc.map];

    // ---- the observer's block: entries [3, 8) from the scenario's waypoints (slot 0) or from the slot's route
    int wp_i, wp_n;                                           // the index of the first of the two waypoints, and how many there are
    int route = -1;
    if (ao == 0) {
        wp_i = st.target_idx[e];
        wp_n = sc.wp_n;
    } else {
        const uint32_t word = st.slot_route ? st.slot_route[g0] : 0u;
        if (word) {
            route = (int)(word & ((1u << TDE_CACHE_ID_BITS) - 1u)) - 1;
            wp_n = (int)(word >> TDE_CACHE_ID_BITS);
        } else {
            const tde_spawn *rec = w.spawn + ((int64_t)s * A + ao);
            route = rec->route;
            wp_n = rec->route_n;
        }
        wp_i = st.route_wp[g0];
        if (route < 0 || route >= w.n_routes) wp_n = 0, wp_i = 0;      // no route: all five entries are 0
    }
    if (lane < 2) {
        const int j = wp_i + lane;
        float fwd = 0.0f, lat = 0.0f;
        if (ao == 0) {
            if (j < wp_n) {
                const double2 t = reinterpret_cast<const double2 *>(w.wp_xy)[(int64_t)s * w.NW + j];
                const float dx = (float)t.x - x0, dy = (float)t.y - y0;
                fwd = dx * c0 + dy * s0;
                lat = dy * c0 - dx * s0;
            }
        } else if (j >= 0 && j < wp_n) {
            const float2 t = reinterpret_cast<const float2 *>(w.route_xy)[(int64_t)route * w.RW + j];
            const float dx = t.x - x0, dy = t.y - y0;
            fwd = dx * c0 + dy * s0;
            lat = dy * c0 - dx * s0;
        }
        row[3 + 2 * lane] = fwd;
        row[4 + 2 * lane] = lat;
    } else if (lane == 2) {
        row[0] = v0;
        row[1] = st.len[g0];
        row[2] = st.wid[g0];
        row[7] = (float)min(max(wp_n - wp_i, 0), 2);
        row[8] = (float)steps / (float)cfg.max_steps;
        row[9] = (m.n_stop > 0 && m.cycle_steps > 0) ? 1.0f : 0.0f;
    } else if (lane == 3 && track) {
        tde_agent_track t;
        t.x = x0; t.y = y0; t.psi = psi0; t.v = v0;
        t.route_wp = st.route_wp[g0]; t.episode = st.episode[e];
        t.steps = steps; t.present = 1u;
        track[i] = t;
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
        const bool live = a != ao && a < A && st.present[base + a] != 0;
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
    for (int q = ncand + lane; q < kn; q += kWave) {
        float *en = row + TDE_VO_EGO + TDE_VO_NBR * q;
#pragma unroll
        for (int c = 0; c < TDE_VO_NBR; ++c) en[c] = 0.0f;
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
        for (int q = 0; q < nb; ++q) car = fminf(car, vo_ray_box(x0, y0, ux, uy, sh.box[q], sh.ext[q]));
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
                for (int c = 0; c < nl; ++c) redl = fminf(redl, vo_ray_box(x0, y0, ux, uy, sh.lbox[c], sh.lext[c]));
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

__global__ __launch_bounds__(kBlock) void agent_outcomes_kernel(tde_config cfg, tde_state st, const int32_t *pairs, int n,
                                                               const tde_agent_track *track, float *reward, uint8_t *flags)
{
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= n) return;
    const int e = pairs[2 * (int64_t)i], a = pairs[2 * (int64_t)i + 1];
    const tde_agent_track tr = track[i];
    float r = 0.0f;
    uint32_t f = 0u;
    if (tr.present != 0u && e >= 0 && e < st.B && a >= 1 && a < st.A) {
        const int64_t g = (int64_t)e * st.A + a;
        f = TDE_AG_VALID;
        if (st.episode[e] != tr.episode || st.present[g] == 0) {
            f |= TDE_AG_ENDED;                                // the agent that was observed is gone
        } else {
            const bool reach = st.route_wp[g] > tr.route_wp;
            f |= (st.collided[g] ? TDE_AG_COLLIDED : 0u) | (st.offroad[g] ? TDE_AG_OFFROAD : 0u) | (reach ? TDE_AG_REACHED : 0u);
            double dist_r, psi_r;
            reward_motion_terms(cfg, reward_bounds(cfg), tr.x, tr.y, tr.psi, st.x[g], st.y[g], st.psi[g], dist_r, psi_r);
            r = reward_sum(cfg, reach, dist_r, psi_r);
        }
    }
    reward[i] = r;
    flags[i] = (uint8_t)f;
}

}  // namespace tde

int tde_agents_version(void) { return TDE_AGENTS_VERSION; }

int tde_agent_obs(const tde_config *cfg, const tde_world *world, const tde_state *st, const struct tde_vector_obs *vo, const int32_t *pairs,
                  int32_t n, float *out, tde_agent_track *track, void *stream)
{
    using tde_host::bad;
    if (const int rc = tde_host::check_vector_obs_args("tde_agent_obs", cfg, world, st, vo, true)) return rc;
    if (!world->spawn) return bad("tde_agent_obs: world.spawn is NULL");
    if (!st->route_wp || !st->episode) return bad("tde_agent_obs: state.route_wp or state.episode is NULL");
    if (!world->route_xy && world->n_routes > 0) return bad("tde_agent_obs: world.route_xy is NULL with n_routes > 0");
    if (n < 0) return bad("tde_agent_obs: n must be >= 0");
    if (n == 0) return 0;
    if (!pairs || !out) return bad("tde_agent_obs: pairs or out is NULL with n > 0");
    if (st->B <= 0) {                                         // no env: every pair is out of range (and the kernel has no row to read)
        const int64_t D = TDE_VO_EGO + TDE_VO_NBR * vo->k_nbr + TDE_VO_RAY * vo->n_rays;
        hipError_t err = hipMemsetAsync(out, 0, sizeof(float) * D * n, (hipStream_t)stream);
        if (err == hipSuccess && track) err = hipMemsetAsync(track, 0, sizeof(tde_agent_track) * (size_t)n, (hipStream_t)stream);
        return err == hipSuccess ? 0 : tde_host::fail("tde_agent_obs", err);
    }
    const unsigned nb = (unsigned)((n + tde::kVoWaves - 1) / tde::kVoWaves);
    tde::agent_obs_kernel<<<nb, tde::kWave * tde::kVoWaves, 0, (hipStream_t)stream>>>(*cfg, *world, *st, *vo, pairs, n, out, track);
    return tde_host::launch_status("tde_agent_obs");
}

int tde_agent_outcomes(const tde_config *cfg, const tde_world *world, const tde_state *st, const int32_t *pairs, int32_t n,
                       const tde_agent_track *track, float *reward, uint8_t *flags, void *stream)
{
    using tde_host::bad;
    if (!cfg || !world || !st) return bad("tde_agent_outcomes: NULL argument");
    if (n < 0) return bad("tde_agent_outcomes: n must be >= 0");
    if (n == 0) return 0;
    if (!pairs || !track || !reward || !flags) return bad("tde_agent_outcomes: pairs, track, reward or flags is NULL with n > 0");
    if (!st->x || !st->y || !st->psi || !st->route_wp || !st->present || !st->collided || !st->offroad || !st->episode)
        return bad("tde_agent_outcomes: a required state pointer is NULL");
    const unsigned nb = (unsigned)((n + tde::kBlock - 1) / tde::kBlock);
    tde::agent_outcomes_kernel<<<nb, tde::kBlock, 0, (hipStream_t)stream>>>(*cfg, *st, pairs, n, track, reward, flags);
    return tde_host::launch_status("tde_agent_outcomes");
}
