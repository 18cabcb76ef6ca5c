// tde_forecast_scene.hip — tde_forecast_scene (include/tde_hip.h): where EVERY slot of an env, the ego included, will be at each of the
// next T steps when the ego takes caller-given actions - the motion half of step_lane (tde_kernels.h) with the leader sweep kept: the
// ego's action from outside, every other slot's from the controller over the A pre-step rows, the bicycle, the replay record, the route
// advance, the new row.  No judging, no reward, no re-spawn: nothing of that half feeds back into motion while an episode lasts.
//   * one lane per (env, slot), env-major as in env_step_kernel, the T steps a loop in registers
//   * the env's rows live in the step's LDS tile (Tiles<kBlock>): written once ahead of the loop, then once per step, between two
//     tile syncs (after the pre-step reads, after the writes).  Up to 64 slots an env sits inside one wavefront and a sync is a
//     wave barrier; at 128 slots it spans two and they meet at the LDS-only workgroup barrier
//   * every lane of the workgroup runs every step (the sweeps ballot, the 128-slot sync is a barrier): the lanes of envs outside
//     `only` or past the batch hold absent slots - rows parked at kFar, no controller, no store
//   * at every step the lanes of an env store A consecutive 16-byte rows of out[e][h - 1]
// The device functions are the step's own; tests/forecast_scene_ref.py restates the rule in numpy.
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"

namespace tde {

template <int A, bool LIGHTS>
__global__ __launch_bounds__(kBlock) void forecast_scene_kernel(tde_config cfg, tde_world w, tde_state st, int T, const float *__restrict__ ego_action,
                                                                const uint8_t *__restrict__ only, float4 *__restrict__ out)
{
    __shared__ Tiles<kBlock> t;
    __shared__ Cold cold;
    if (threadIdx.x == 0) fill_cold(cold, cfg, w);
    __syncthreads();
    const uint32_t F = cfg.flags;
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)blockIdx.x * kBlock + tid;
    const int e = (int)(g / A), a = (int)(g % A);
    const int base = tid - a;                       // first lane of this env inside the workgroup
    const bool valid = e < st.B;
    const int64_t gs = valid ? g : 0;
    const int es = valid ? e : 0;
    const bool on = valid && (!only || only[es]);
    Agent ag;
    load_agent(st, gs, ag);
    const bool live = on && ag.present;
    const bool npc = (F & TDE_F_NPC) && a > 0 && live;
    const int steps = st.steps[es];
    // (no ego reward context: a target index past every route keeps load_ctx from fetching the ego's waypoint)
    const EnvRegs er{st.scn[es], steps, 0x7fffffff, 0, 0};
    Ctx cx;
    load_ctx<A>(cfg, cold, a, ag, er, cx);
    float c0, s0;
    sincos_f32(ag.psi, s0, c0);
    write_tile_slot(t.a[tid], t.b[tid], live, ag, c0, s0, cfg.npc_lane_half);
    tile_sync<A>();
    const float2 *act = ego_action ? reinterpret_cast<const float2 *>(ego_action) + (int64_t)es * T : nullptr;
    float4 *row = out + ((int64_t)es * T * A + a);
    for (int h = 1; h <= T; ++h) {
        const int k = steps + h;
        // replayed agents take their recorded state at time k; the read is issued ahead of the sweep
        const bool replayed = (F & TDE_F_REPLAY) && a > 0 && live && k < cx.replay_len;
        float4 rep = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (replayed) rep = reinterpret_cast<const float4 *>(w.replay_states)[(int64_t)ag.replay * w.RT + k];
        // ---- actions: the ego's from the caller (none: it coasts), the others' from the controller over the pre-step tile ----------
        const bool has_target = npc && ag.route >= 0 && ag.route_wp < cx.route_n;
        float acc = 0.0f, beta = 0.0f;
        if (a == 0 && act) { const float2 u = act[h - 1]; acc = u.x; beta = u.y; }
        const uint32_t red = (LIGHTS && (F & TDE_F_TRAFFIC_LIGHTS)) ? red_mask(w, cx.m, k) : 0u;
        if (F & TDE_F_NPC) {
            float na, nb;
            const float red_gap = (LIGHTS && red && has_target) ? red_line_gap(cfg, w, cx.m, red, ag, c0, s0) : 1e30f;
            if constexpr (A > 64) npc_action_wide<A>(cfg, &t.a[base], &t.b[base], a, ag, c0, s0, has_target, cx.tgx, cx.tgy, cx.g_far, red_gap, na, nb);
            else npc_action<A>(cfg, &t.a[base], &t.b[base], a, ag, c0, s0, has_target, cx.tgx, cx.tgy, cx.g_far, red_gap, na, nb);
            if (npc && (k > 1 || (F & TDE_F_NPC_FIRST_STEP))) { acc = na; beta = nb; }
        }
        if (live) {
            bicycle(ag.x, ag.y, ag.psi, ag.v, ag.inv_lr, acc, beta, cfg.dt);
            if (replayed) { ag.x = rep.x; ag.y = rep.y; ag.psi = rep.z; ag.v = rep.w; }
        }
        bool switched = false;
        if (has_target) {
            const float dx = cx.tgx - ag.x, dy = cx.tgy - ag.y;
            if (dx * dx + dy * dy < cfg.npc_reach * cfg.npc_reach) { ag.route_wp += 1; switched = true; }
        }
        // ---- the post-step tile: the next step's pre-step scene ---------------------------------------------------------------------
        sincos_f32(ag.psi, s0, c0);
        tile_sync<A>();                                 // every lane is done reading the pre-step tile
        write_tile_slot(t.a[tid], t.b[tid], live, ag, c0, s0, cfg.npc_lane_half);
        tile_sync<A>();
        if (switched) load_route_target(cold, ag, cx);
        if (on) *row = live ? make_float4(ag.x, ag.y, ag.psi, ag.v) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        row += A;
    }
}

}  // namespace tde

namespace tde_host {

int launch_forecast_scene(const tde_config *cfg, const tde_world *world, const tde_state *st, int32_t T, const float *ego_action,
                          const uint8_t *only, float *out, void *stream)
{
    const bool lights = (cfg->flags & TDE_F_TRAFFIC_LIGHTS) != 0;
    const unsigned nb = (unsigned)(((int64_t)st->B * st->A + tde::kBlock - 1) / tde::kBlock);
    TDE_DISPATCH_A128(st->A, with_flags({lights}, [&](auto l) {
        tde::forecast_scene_kernel<kA, l.value><<<nb, tde::kBlock, 0, (hipStream_t)stream>>>(*cfg, *world, *st, T, ego_action, only, reinterpret_cast<float4 *>(out));
    }));
    return launch_status("tde_forecast_scene");
}

}  // namespace tde_host
