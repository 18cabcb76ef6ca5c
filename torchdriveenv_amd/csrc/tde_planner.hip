// tde_planner.hip — the sampling planner of tde_plan_action (include/tde_hip.h: a lattice of constant (acceleration, steering)
// candidates rolled forward through the step's bicycle and judged by the step's offroad, collision and red-line predicates) and its
// launcher.  One wavefront per env, kPlWaves envs per workgroup, one lane per candidate.
//   * the env's other present agents are staged once in LDS as (x, y, c, s | vx dt, vy dt, hl, hw | reject radius^2) rows
//   * lane h resolves the light phase of horizon step h once; a step reads its mask with one v_readlane, and the stop lines are
//     walked with wave-uniform (scalar) loads, only those whose light is red at that step reaching the overlap test
//   * per horizon step a lane advances its state; a FULL coarse tile whose clearance covers the box's circum-radius proves all four
//     corners on the road, the others go through the class map and offroad_resolve; the LDS rows are swept with a centre-distance
//     reject ahead of the separating-axis test; a lane drops out at its first failure and the wavefront leaves the loop when no
//     lane is alive
//   * the winner is a butterfly minimum of the (ordered cost bits, candidate) key
// The specification is restated in numpy by tests/planner_ref.py.
#include "tde_kernels.h"
#include "tde_host.h"

namespace tde {

constexpr int kPlWaves = 4;             // envs per workgroup
constexpr float kPlSkipMargin = 0.05f;  // metres taken off a coarse tile's clearance (the fp32 error of the corner positions)

struct PlWave {
    float4 box[TDE_MAX_AGENTS];         // the other present agents: x, y, c, s
    float4 mot[TDE_MAX_AGENTS];         //                           (v c) dt, (v s) dt, hl + margin, hw + margin
    float rej2[TDE_MAX_AGENTS];         // a centre distance^2 beyond which the boxes cannot overlap
};

// class | clearance << 2 of the coarse tile that holds the cell of (px, py) (tde_abi.h: cell_coarse; the clamp of cell_class_lookup)
TDE_DEV uint32_t pl_coarse(const tde_world &w, const tde_map &m, float px, float py)
{
    const float fx = __builtin_amdgcn_fmed3f((px - m.ox) * m.inv_cell, 0.0f, (float)(m.nx - 1));
    const float fy = __builtin_amdgcn_fmed3f((py - m.oy) * m.inv_cell, 0.0f, (float)(m.ny - 1));
    static_assert(TDE_COARSE_CELLS == 4, "coarse tiles of 4 x 4 cells");
    const uint32_t cx = (uint32_t)(int)fx >> 2, cy = (uint32_t)(int)fy >> 2;
    const uint32_t line = (uint32_t)m.coarse_base + ((cy >> 3) << (m.row_shift - 6)) + (cx >> 4);
    return w.cell_coarse[(line << 7) | (((cy & 7u) << 4) | (cx & 15u))];
}

TDE_DEV float pl_dist(float wx, float wy, float x, float y)
{
    const float dx = wx - x, dy = wy - y;
    return __builtin_sqrtf(dx * dx + dy * dy);
}

__global__ __launch_bounds__(kWave * kPlWaves) void plan_action_kernel(tde_config cfg, tde_world w, tde_state st, tde_planner pl,
                                                                     const uint8_t *only, float *action, tde_plan_diag *diag)
{
    __shared__ PlWave shw[kPlWaves];
    const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int e = (int)blockIdx.x * kPlWaves + wv;
    if (e >= st.B || (only && !only[e])) return;             // (wave-uniform; no workgroup barrier below)
    PlWave &sh = shw[wv];
    const int A = st.A, H = pl.horizon;
    const int64_t base = (int64_t)e * A;
    const float dt = cfg.dt, thr2 = thr2_of(cfg);
    const int s = st.scn[e];
    const tde_scenario sc = w.scn[s];
    const tde_map m = w.maps[sc.map];
    const int steps = st.steps[e];
    const float hl0 = 0.5f * st.len[base], hw0 = 0.5f * st.wid[base];
    const float inv_lr = 1.0f / st.lr[base];
    const float r0 = __builtin_sqrtf(hl0 * hl0 + hw0 * hw0);

    // ---- the other present agents: rows in LDS (compacted)
    int nb = 0;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (p * kWave >= A) break;                            // (wave-uniform)
        const int a = p * kWave + lane;
        const bool live = a > 0 && a < A && st.present[base + a] != 0;
        float4 b = make_float4(0.0f, 0.0f, 1.0f, 0.0f), mo = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        float rj = 0.0f;
        if (live) {
            const int64_t g = base + a;
            float sa, ca;
            sincos_f32(st.psi[g], sa, ca);
            const float va = st.v[g];
            const float hl = 0.5f * st.len[g] + pl.margin, hw = 0.5f * st.wid[g] + pl.margin;
            b = make_float4(st.x[g], st.y[g], ca, sa);
            mo = make_float4((va * ca) * dt, (va * sa) * dt, hl, hw);
            const float rr = (r0 + __builtin_sqrtf(hl * hl + hw * hw)) * 1.001f + 0.01f;   // (conservative: only a shortcut)
            rj = rr * rr;
        }
        const unsigned long long bl = __ballot(live);
        if (live) {
            const int q = nb + lane_prefix(bl);
            sh.box[q] = b;
            sh.mot[q] = mo;
            sh.rej2[q] = rj;
        }
        nb += __popcll(bl);
    }
    wave_lds_fence();

    // ---- the light phases of the horizon: lane h holds the red mask of step steps + h
    const bool lights = (cfg.flags & TDE_F_TRAFFIC_LIGHTS) && m.n_stop > 0 && m.cycle_steps > 0;
    uint32_t redv = 0u;
    if (lights && lane >= 1 && lane <= H) redv = red_mask(w, m, steps + lane);

    // ---- one lane per candidate
    const int nc = pl.n_a * pl.n_s;
    const bool active = lane < nc;
    const int ci = active ? lane : 0;
    const float a = pl.accel[ci / pl.n_s], d = pl.steer[ci % pl.n_s];
    float x = st.x[base], y = st.y[base], psi = st.psi[base], v = st.v[base];
    int ti = st.target_idx[e];
    float wx = 0.0f, wy = 0.0f, dp = 0.0f, gain = 0.0f, sv = 0.0f;
    const double2 *wps = reinterpret_cast<const double2 *>(w.wp_xy) + (int64_t)s * w.NW;
    if (ti < sc.wp_n) {
        const double2 t = wps[ti];
        wx = (float)t.x;
        wy = (float)t.y;
        dp = pl_dist(wx, wy, x, y);
    }
    const float rr = (float)cfg.reach_radius;
    float a1 = (v + a * dt < 0.0f) ? 0.0f : a;
    bool alive = active;
    int f = H + 1;
    for (int h = 1; h <= H; ++h) {
        if (!__ballot(alive)) break;
        float sn = 0.0f, cs = 1.0f;
        bool need = false;
        if (alive) {
            const float ah = (v + a * dt < 0.0f) ? 0.0f : a;
            bicycle(x, y, psi, v, inv_lr, ah, d, dt);
            sincos_f32(psi, sn, cs);
            // (i) a FULL coarse tile under the centre whose clearance covers the circum-radius proves the four corners on the road
            const uint32_t co = pl_coarse(w, m, x, y);
            need = !((co & 3u) == TDE_CELL_FULL && (float)(co >> 2) * TDE_COARSE_UNIT - kPlSkipMargin >= r0);
        }
        bool fail = box_offroad<true, true>(w, m, need, x, y, cs, sn, hl0, hw0, thr2);   // (by all lanes: offroad_resolve ballots)
        if (alive && !fail) {
            // (ii) the predicted boxes
            const float fh = (float)h;
            for (int j = 0; j < nb; ++j) {
                const float4 b = sh.box[j], mo = sh.mot[j];
                const float bx = b.x + fh * mo.x, by = b.y + fh * mo.y;
                const float ex = bx - x, ey = by - y;
                if (ex * ex + ey * ey > sh.rej2[j]) continue;
                if (obb_overlap(x, y, cs, sn, hl0, hw0, bx, by, b.z, b.w, mo.z, mo.w)) { fail = true; break; }
            }
        }
        if (lights) {
            // (iii) the stop lines that are red at this step (wave-uniform walk)
            const uint32_t red = (uint32_t)__builtin_amdgcn_readlane((int)redv, h);
            if (red) {
                for (int q = 0; q < m.n_stop; ++q) {
                    const tde_stopline ln = w.stoplines[m.stop_base + q];
                    if (!((red >> ((uint32_t)ln.light & 31u)) & 1u)) continue;
                    if (alive && !fail && obb_overlap(x, y, cs, sn, hl0, hw0, ln.x, ln.y, ln.c, ln.s, ln.hl, ln.hw)) fail = true;
                }
            }
        }
        if (alive && fail) {
            f = h;
            alive = false;
        }
        if (alive) {
            if (ti < sc.wp_n) {
                const float dn = pl_dist(wx, wy, x, y);
                gain = gain + (dp - dn);
                dp = dn;
                if (dn < rr) {
                    ti += 1;
                    if (ti < sc.wp_n) {
                        const double2 t = wps[ti];
                        wx = (float)t.x;
                        wy = (float)t.y;
                        dp = pl_dist(wx, wy, x, y);
                    }
                }
            }
            const float ev = v - (ti < sc.wp_n ? pl.v_target : 0.0f);
            sv = sv + ev * ev;
        }
    }
    const float run = (pl.w_speed * sv + pl.w_steer * (d * d)) - pl.w_progress * gain;
    const float cost = (float)(H + 1 - f) * TDE_PLAN_FAIL_UNIT + fminf(fmaxf(run + TDE_PLAN_RUN_BIAS, 0.0f), TDE_PLAN_RUN_MAX);
    const uint32_t cb = __float_as_uint(cost);
    uint32_t kc = active ? ((cb >> 31) ? ~cb : (cb ^ 0x80000000u)) : 0xFFFFFFFFu;
    int ki = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t oc = (uint32_t)__shfl_xor((int)kc, o);
        const int oi = __shfl_xor(ki, o);
        if (oc < kc || (oc == kc && oi < ki)) {
            kc = oc;
            ki = oi;
        }
    }
    const int n_safe = __popcll(__ballot(active && f == H + 1));
    const float wa = __shfl(a1, ki), wd = __shfl(d, ki), wc = __shfl(cost, ki);
    const int wf = __shfl(f, ki);
    if (lane == 0) {
        reinterpret_cast<float2 *>(action)[e] = make_float2(wa, wd);
        if (diag) {
            tde_plan_diag o;
            o.winner = ki;
            o.fail_step = wf;
            o.cost = wc;
            o.n_safe = n_safe;
            diag[e] = o;
        }
    }
}

}  // namespace tde

namespace tde_host {

int launch_plan_action(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_planner *pl, const uint8_t *only,
                       float *action, tde_plan_diag *diag, void *stream)
{
    const unsigned nb = (unsigned)((st->B + tde::kPlWaves - 1) / tde::kPlWaves);
    tde::plan_action_kernel<<<nb, tde::kWave * tde::kPlWaves, 0, (hipStream_t)stream>>>(*cfg, *world, *st, *pl, only, action, diag);
    return launch_status("tde_plan_action");
}

}  // namespace tde_host
