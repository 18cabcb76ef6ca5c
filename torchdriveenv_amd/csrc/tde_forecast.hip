// tde_forecast.hip — tde_forecast_agents (include/tde_hip.h): where every non-ego slot will be at each of the next T steps when
// nobody is in its cone - step_lane's treatment of a present slot j >= 1 (tde_kernels.h) with the leader sweep replaced by "no
// leader": the controller's action from npc_act_of_gap, the bicycle, the replay record, the route advance; and its launcher.
//   * one lane per (env, slot), the T steps a loop in registers: agents do not interact in a free-flow forecast, so there is no
//     LDS and no barrier
//   * at every step the lanes of an env store consecutive 16-byte rows of out[e][h - 1]: A * 16 contiguous bytes per env and step
//   * the ego's lane and the lanes of absent slots run the same loop and store zeros, so that the stores stay whole lines
// The device functions are the step's own; tests/forecast_ref.py restates the rule in numpy.
#include "tde_kernels.h"
#include "tde_host.h"

namespace tde {

constexpr int kFcBlock = 256;

__global__ __launch_bounds__(kFcBlock) void forecast_agents_kernel(tde_config cfg, tde_world w, tde_state st, int T, const uint8_t *only,
                                                                   float4 *out)
{
    const int A = st.A;
    const int64_t g = (int64_t)blockIdx.x * kFcBlock + threadIdx.x;
    const int e = (int)(g / A), a = (int)(g - (int64_t)e * A);
    if (e >= st.B || (only && !only[e])) return;
    const uint32_t F = cfg.flags;
    Agent ag;
    load_agent(st, g, ag);
    const bool live = a > 0 && ag.present;
    const bool npc = (F & TDE_F_NPC) && live;
    const int scn = st.scn[e], steps = st.steps[e];
    Cold cold{};                                              // (load_route_target reads these two members)
    cold.route_xy = w.route_xy;
    cold.RW = w.RW;
    Ctx cx{};
    bool lights = false;
    if (live) {
        const tde_spawn *rec = w.spawn + ((int64_t)scn * A + a);
        if (F & TDE_F_NPC) {
            ag.route = rec->route;
            cx.route_n = rec->route_n;
            load_route_target(cold, ag, cx);
        }
        if (F & TDE_F_REPLAY) {
            ag.replay = rec->replay;
            cx.replay_len = rec->replay_len;
        }
        if (npc && (F & TDE_F_TRAFFIC_LIGHTS)) {
            cx.m = w.maps[w.scn[scn].map];
            lights = cx.m.n_stop > 0 && cx.m.cycle_steps > 0;
        }
    }
    float s0 = 0.0f, c0 = 1.0f;
    if (live) sincos_f32(ag.psi, s0, c0);
    float4 *row = out + ((int64_t)e * T * A + a);
    for (int h = 1; h <= T; ++h) {
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (live) {
            const int k = steps + h;
            const bool has_target = npc && ag.route >= 0 && ag.route_wp < cx.route_n;
            float acc = 0.0f, beta = 0.0f;
            if (npc && (k > 1 || (F & TDE_F_NPC_FIRST_STEP))) {
                const uint32_t red = lights ? red_mask(w, cx.m, k) : 0u;
                const float red_gap = (red && has_target) ? red_line_gap(cfg, w, cx.m, red, ag, c0, s0) : 1e30f;
                npc_act_of_gap(cfg, ag, c0, s0, has_target, cx.tgx, cx.tgy, 1e30f, red_gap, acc, beta);
            }
            bicycle(ag.x, ag.y, ag.psi, ag.v, ag.inv_lr, acc, beta, cfg.dt);
            if ((F & TDE_F_REPLAY) && ag.replay >= 0 && k < cx.replay_len) {
                const float4 rep = reinterpret_cast<const float4 *>(w.replay_states)[(int64_t)ag.replay * w.RT + k];
                ag.x = rep.x; ag.y = rep.y; ag.psi = rep.z; ag.v = rep.w;
            }
            if (has_target) {
                const float dx = cx.tgx - ag.x, dy = cx.tgy - ag.y;
                if (dx * dx + dy * dy < cfg.npc_reach * cfg.npc_reach) {
                    ag.route_wp += 1;
                    load_route_target(cold, ag, cx);
                }
            }
            sincos_f32(ag.psi, s0, c0);
            r = make_float4(ag.x, ag.y, ag.psi, ag.v);
        }
        *row = r;
        row += A;
    }
}

}  // namespace tde

namespace tde_host {

int launch_forecast_agents(const tde_config *cfg, const tde_world *world, const tde_state *st, int32_t T, const uint8_t *only, float *out,
                           void *stream)
{
    const int64_t n = (int64_t)st->B * st->A;
    const unsigned nb = (unsigned)((n + tde::kFcBlock - 1) / tde::kFcBlock);
    tde::forecast_agents_kernel<<<nb, tde::kFcBlock, 0, (hipStream_t)stream>>>(*cfg, *world, *st, T, only, reinterpret_cast<float4 *>(out));
    return launch_status("tde_forecast_agents");
}

}  // namespace tde_host
