// tde_plan_scene.hip — tde_score_plans_scene (include/tde_hip.h): tde_score_plans with a scene of its own for every (env, sequence)
// pair - a VIRTUAL ENV v = (e, n) in which the ego follows sequence n, the other slots run the controller with its leader sweep over
// THAT scene (forecast_scene_kernel's loop, tde_forecast_scene.hip) and the ego's box is judged against it at every step by the plan
// judge's three predicates.  No forecast is materialised.
//   * one lane per (e, n, slot), v-major, 256-thread workgroups; every lane of (e, ., j) loads the same state of env e
//   * the rows of v live in the step's LDS tile (Tiles<kBlock>), two tile syncs per step as in forecast_scene_kernel; the ego's
//     judged pose (x, y, c, s) travels beside the tile (ego_box: one entry per virtual env of the workgroup), so an absent ego is
//     parked in the tile - the others do not see it - and judged all the same, as tde_score_plans_forecast does
//   * the judge of step h is spread over v's lanes: lane j >= 1 tests its own box, inflated by the margin, against the ego's
//     (obb_overlap); lanes 0..3 take one corner of the ego's box each (corner_offroad; fewer than four lanes: corners in turn); the
//     stop lines go to lane 4 (lane 0 below eight slots).  The verdict is joined by ballot (A <= 64) or through LDS (A = 128)
//   * the slot-0 lane forms the knot's action, walks the cost and stores cost and fail_step
//   * the loop ends early when no virtual env of the WAVEFRONT is still judged (A <= 64: the syncs are wave barriers); at A = 128
//     the sync is a workgroup barrier and every lane runs every step
// plan_scene_winner_kernel reduces the N virtual envs of an env (they span workgroups) to action / diag: one wavefront per env.
// The device functions are the step's own; tests/plan_scene_ref.py restates the rule by composition in numpy.
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"

namespace tde {

template <int A, bool LIGHTS>
__global__ __launch_bounds__(kBlock) void score_plans_scene_kernel(tde_config cfg, tde_world w, tde_state st, tde_planner pl, tde_plan_set ps,
                                                                   const uint8_t *__restrict__ only, float *__restrict__ cost_out,
                                                                   int32_t *__restrict__ fail_out)
{
    constexpr int kVirt = kBlock / A;               // virtual envs per workgroup
    __shared__ Tiles<kBlock> t;
    __shared__ Cold cold;
    __shared__ float4 ego_box[kVirt];               // the judged ego of each virtual env after the step: x, y, c, s
    __shared__ int ego_on[kVirt];                   // 1: still judged; 2 (A = 128): some lane found a failure at this step
    if (threadIdx.x == 0) fill_cold(cold, cfg, w);
    __syncthreads();
    const uint32_t F = cfg.flags;
    const int tid = threadIdx.x;
    const int N = ps.N, K = ps.K, H = pl.horizon, HT = pl.horizon + ps.tail;
    const int64_t g = (int64_t)blockIdx.x * kBlock + tid;
    const int64_t vg = g / A;                       // the virtual env: e * N + n
    const int a = (int)(g % A);
    const int vi = tid / A, base = tid - a;         // its index and first lane inside the workgroup
    const bool valid = vg < (int64_t)st.B * N;
    const int64_t vs = valid ? vg : 0;
    const int es = (int)(vs / N);
    const bool on = valid && (!only || only[es]);
    const int64_t gs = (int64_t)es * A + a;
    Agent ag;
    load_agent(st, gs, ag);
    // (the ego is judged present or not, as tde_score_plans does; an absent one is parked in the tile)
    const bool live = on && ag.present;
    const bool npc = (F & TDE_F_NPC) && a > 0 && live;
    const int steps = st.steps[es];
    const int scn = st.scn[es];
    // (no ego reward context: a target index past every route keeps load_ctx from fetching the ego's waypoint)
    const EnvRegs er{scn, steps, 0x7fffffff, 0, 0};
    Ctx cx;
    load_ctx<A>(cfg, cold, a, ag, er, cx);
    const tde_map m = w.maps[cx.map_id];            // (the judge reads the map whatever the flags)
    const float dt = cfg.dt, thr2 = thr2_of(cfg);
    const float hl0 = 0.5f * st.len[gs - a], hw0 = 0.5f * st.wid[gs - a];
    const float mhl = 0.5f * ag.len + pl.margin, mhw = 0.5f * ag.wid + pl.margin;
    float c0, s0;
    sincos_f32(ag.psi, s0, c0);
    write_tile_slot(t.a[tid], t.b[tid], live, ag, c0, s0, cfg.npc_lane_half);
    tile_sync<A>();

    // ---- the slot-0 lane: tde_score_plans' sequence state, expression for expression (tde_plan_set.hip) -------------------------
    const bool ego = a == 0;
    const float2 *knots = reinterpret_cast<const float2 *>(ps.seq) + vs * K;
    float ka = 0.0f, kd = 0.0f, dmax2 = 0.0f;
    bool alive = ego && on;
    if (alive) {
        const float2 k0 = knots[0];
        ka = fminf(fmaxf(k0.x, -TDE_PLAN_BOX_ACCEL), TDE_PLAN_BOX_ACCEL);
        kd = fminf(fmaxf(k0.y, -TDE_PLAN_BOX_STEER), TDE_PLAN_BOX_STEER);
    }
    int kidx = 0, kleft = ps.knot_len;
    int ti = st.target_idx[es];
    const int wp_n = w.scn[scn].wp_n;
    float wx = 0.0f, wy = 0.0f, dp = 0.0f, gain = 0.0f, sv = 0.0f;
    const double2 *wps = reinterpret_cast<const double2 *>(w.wp_xy) + (int64_t)scn * w.NW;
    const auto dist = [](float px, float py, float x, float y) {
        const float dx = px - x, dy = py - y;
        return __builtin_sqrtf(dx * dx + dy * dy);
    };
    if (ego && ti < wp_n) {
        const double2 tg = wps[ti];
        wx = (float)tg.x;
        wy = (float)tg.y;
        dp = dist(wx, wy, ag.x, ag.y);
    }
    const float rr = (float)cfg.reach_radius;
    int f = HT + 1;

    for (int h = 1; h <= HT; ++h) {
        if constexpr (A <= kWave) {
            if (!__ballot(alive)) break;            // (wave-uniform: nobody in this wavefront is judged any more)
        }
        const int k = steps + h;
        const bool tail = h > H;
        // replayed agents take their recorded state at time k; the read is issued ahead of the sweep
        const bool replayed = (F & TDE_F_REPLAY) && a > 0 && live && k < cx.replay_len;
        float4 rep = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (replayed) rep = reinterpret_cast<const float4 *>(w.replay_states)[(int64_t)ag.replay * w.RT + k];
        // ---- actions: the ego's from its knot (the tail: full braking), the others' from the controller over the pre-step tile ------
        const bool has_target = npc && ag.route >= 0 && ag.route_wp < cx.route_n;
        float acc = 0.0f, beta = 0.0f;
        if (ego) {
            if (tail) {
                ka = -TDE_PLAN_BOX_ACCEL;
                if (alive && ag.v + ka * dt < 0.0f) alive = false;     // at rest as far as the action box can brake: safe
            } else {
                if (kleft == 0) {
                    if (kidx < K - 1) {
                        ++kidx;
                        if (alive) {
                            const float2 kn = knots[kidx];
                            ka = fminf(fmaxf(kn.x, -TDE_PLAN_BOX_ACCEL), TDE_PLAN_BOX_ACCEL);
                            kd = fminf(fmaxf(kn.y, -TDE_PLAN_BOX_STEER), TDE_PLAN_BOX_STEER);
                        }
                    }
                    kleft = ps.knot_len;
                }
                --kleft;
                if (alive) dmax2 = fmaxf(dmax2, kd * kd);
            }
            acc = (ag.v + ka * dt < 0.0f) ? 0.0f : ka;
            beta = kd;
        }
        const uint32_t red = (LIGHTS && (F & TDE_F_TRAFFIC_LIGHTS)) ? red_mask(w, m, k) : 0u;
        if (F & TDE_F_NPC) {
            float na, nb;
            const float red_gap = (LIGHTS && red && has_target) ? red_line_gap(cfg, w, m, red, ag, c0, s0) : 1e30f;
            if constexpr (A > 64) npc_action_wide<A>(cfg, &t.a[base], &t.b[base], a, ag, c0, s0, has_target, cx.tgx, cx.tgy, cx.g_far, red_gap, na, nb);
            else npc_action<A>(cfg, &t.a[base], &t.b[base], a, ag, c0, s0, has_target, cx.tgx, cx.tgy, cx.g_far, red_gap, na, nb);
            if (npc && (k > 1 || (F & TDE_F_NPC_FIRST_STEP))) { acc = na; beta = nb; }
        }
        if (ego ? alive : live) {
            bicycle(ag.x, ag.y, ag.psi, ag.v, ag.inv_lr, acc, beta, dt);
            if (replayed) { ag.x = rep.x; ag.y = rep.y; ag.psi = rep.z; ag.v = rep.w; }
        }
        bool switched = false;
        if (has_target) {
            const float dx = cx.tgx - ag.x, dy = cx.tgy - ag.y;
            if (dx * dx + dy * dy < cfg.npc_reach * cfg.npc_reach) { ag.route_wp += 1; switched = true; }
        }
        // ---- the post-step tile: this step's judged scene, the next step's pre-step scene --------------------------------------------
        sincos_f32(ag.psi, s0, c0);
        tile_sync<A>();                                 // every lane is done reading the pre-step tile (and the last step's verdict)
        write_tile_slot(t.a[tid], t.b[tid], live, ag, c0, s0, cfg.npc_lane_half);
        if (ego) {
            ego_box[vi] = make_float4(ag.x, ag.y, c0, s0);
            ego_on[vi] = alive ? 1 : 0;
        }
        tile_sync<A>();
        if (switched) load_route_target(cold, ag, cx);
        // ---- the judge of step h, spread over the lanes of the virtual env ------------------------------------------------------------
        bool bad = false;
        if (ego_on[vi]) {
            const float4 eb = ego_box[vi];
            // (ii) this lane's own box, inflated by the margin
            if (a > 0 && live) bad = obb_overlap(eb.x, eb.y, eb.z, eb.w, hl0, hw0, ag.x, ag.y, c0, s0, mhl, mhw);
            // (i) one corner of the ego's box per lane
            if (a < 4) {
                for (int ci = a; ci < 4; ci += A) bad = bad || corner_offroad<true>(w, m, ci, eb.x, eb.y, eb.z, eb.w, hl0, hw0, thr2);
            }
            // (iii) the stop lines that are red at this step
            if constexpr (LIGHTS) {
                if (a == (A > 4 ? 4 : 0) && red) bad = bad || tl_violation(w, m, red, eb.x, eb.y, eb.z, eb.w, hl0, hw0);
            }
        }
        bool fail;
        if constexpr (A > kWave) {
            if (bad) ego_on[vi] = 2;
            lds_barrier();
            fail = ego_on[vi] == 2;
        } else if constexpr (A == kWave) {
            fail = __ballot(bad) != 0ull;
        } else {
            // (an env's lanes: a power of two <= 32, aligned - they lie in one half of the mask)
            constexpr uint32_t kMine = A >= 32 ? 0xFFFFFFFFu : ((1u << (A & 31)) - 1u);
            fail = (mask_field(__ballot(bad), (tid & 63) - a) & kMine) != 0u;
        }
        if (alive && fail) {
            f = h;
            alive = false;
        }
        // ---- the Cost walk (tde_score_plans') -----------------------------------------------------------------------------------------
        if (alive && !tail) {
            if (ti < wp_n) {
                const float dn = dist(wx, wy, ag.x, ag.y);
                gain = gain + (dp - dn);
                dp = dn;
                if (dn < rr) {
                    ti += 1;
                    if (ti < wp_n) {
                        const double2 tg = wps[ti];
                        wx = (float)tg.x;
                        wy = (float)tg.y;
                        dp = dist(wx, wy, ag.x, ag.y);
                    }
                }
            }
            const float ev = ag.v - (ti < wp_n ? pl.v_target : 0.0f);
            sv = sv + ev * ev;
        }
    }
    if (ego && on) {
        const float run = (pl.w_speed * sv + pl.w_steer * dmax2) - pl.w_progress * gain;
        cost_out[vs] = (float)(HT + 1 - f) * TDE_PLAN_FAIL_UNIT + fminf(fmaxf(run + TDE_PLAN_RUN_BIAS, 0.0f), TDE_PLAN_RUN_MAX);
        fail_out[vs] = f;
    }
}

constexpr int kPvWaves = 4;             // envs per workgroup of the winner kernel

// tde_score_plans' Winner over cost[e][.] and fail_step[e][.] as score_plans_scene_kernel left them: one wavefront per env
__global__ __launch_bounds__(kWave * kPvWaves) void plan_scene_winner_kernel(float dt, tde_state st, tde_plan_set ps, int HT, const uint8_t *__restrict__ only,
                                                                            const float *__restrict__ cost, const int32_t *__restrict__ fail,
                                                                            float *action, tde_plan_diag *diag)
{
    const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int e = (int)blockIdx.x * kPvWaves + wv;
    if (e >= st.B || (only && !only[e])) return;            // (wave-uniform, no barrier below)
    const int N = ps.N;
    const int64_t row = (int64_t)e * N;
    uint32_t kc = 0xFFFFFFFFu;
    int ki = 0x7FFFFFFF, ns = 0;
    for (int n = lane; n < N; n += kWave) {
        const uint32_t cb = __float_as_uint(cost[row + n]);
        const uint32_t key = (cb >> 31) ? ~cb : (cb ^ 0x80000000u);
        if (key < kc || (key == kc && n < ki)) { kc = key; ki = n; }
        ns += fail[row + n] == HT + 1 ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t oc = (uint32_t)__shfl_xor((int)kc, o);
        const int oi = __shfl_xor(ki, o);
        if (oc < kc || (oc == kc && oi < ki)) { kc = oc; ki = oi; }
        ns += __shfl_xor(ns, o);
    }
    if (lane != 0) return;
    if (action) {
        const float2 k0 = reinterpret_cast<const float2 *>(ps.seq)[(row + ki) * ps.K];
        const float a = fminf(fmaxf(k0.x, -TDE_PLAN_BOX_ACCEL), TDE_PLAN_BOX_ACCEL);
        const float d = fminf(fmaxf(k0.y, -TDE_PLAN_BOX_STEER), TDE_PLAN_BOX_STEER);
        const float v = st.v[(int64_t)e * st.A];
        reinterpret_cast<float2 *>(action)[e] = make_float2((v + a * dt < 0.0f) ? 0.0f : a, d);
    }
    if (diag) {
        tde_plan_diag o;
        o.winner = ki;
        o.fail_step = fail[row + ki];
        o.cost = cost[row + ki];
        o.n_safe = ns;
        diag[e] = o;
    }
}

}  // namespace tde

namespace tde_host {

int launch_score_plans_scene(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_planner *pl, const tde_plan_set *ps,
                             const uint8_t *only, float *cost, int32_t *fail_step, float *action, tde_plan_diag *diag, void *stream)
{
    const bool lights = (cfg->flags & TDE_F_TRAFFIC_LIGHTS) != 0;
    const unsigned nb = (unsigned)(((int64_t)st->B * ps->N * st->A + tde::kBlock - 1) / tde::kBlock);
    TDE_DISPATCH_A128(st->A, with_flags({lights}, [&](auto l) {
        tde::score_plans_scene_kernel<kA, l.value><<<nb, tde::kBlock, 0, (hipStream_t)stream>>>(*cfg, *world, *st, *pl, *ps, only, cost, fail_step);
    }));
    int rc = launch_status("tde_score_plans_scene");
    if (rc || (!action && !diag)) return rc;
    const unsigned nw = (unsigned)((st->B + tde::kPvWaves - 1) / tde::kPvWaves);
    tde::plan_scene_winner_kernel<<<nw, tde::kWave * tde::kPvWaves, 0, (hipStream_t)stream>>>(cfg->dt, *st, *ps, pl->horizon + ps->tail, only, cost,
                                                                                             fail_step, action, diag);
    return launch_status("tde_score_plans_scene");
}

}  // namespace tde_host
