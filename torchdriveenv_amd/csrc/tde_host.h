// tde_host.h — what the translation units of libtde_hip.so share on the HOST side: the error slot of tde_last_error, the
// dispatch-by-slot-count macros (the step and rollout units use tde_launch.h instead) and the launchers each kernel family's unit exports to the C-ABI entry points in tde_api.hip.
// Everything here has hidden visibility (the library is built with -fvisibility=hidden; only TDE_API symbols are exported).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/tde_hip.h"

namespace tde { struct StepArgs; }
struct tde_replay;
struct tde_terminal;

namespace tde_host {

// the calling thread's error slot (256 bytes), defined in tde_api.hip
char *err_buf();
constexpr int kErrLen = 256;

inline int fail(const char *what, hipError_t e)
{
    snprintf(err_buf(), kErrLen, "%s: %s", what, hipGetErrorString(e));
    return (int)e;
}

inline int bad(const char *msg)
{
    snprintf(err_buf(), kErrLen, "%s", msg);
    return (int)hipErrorInvalidValue;
}

// the same for a rule that several entry points share: the message names the one that was called
inline int bad_in(const char *fn, const char *msg)
{
    snprintf(err_buf(), kErrLen, "%s: %s", fn, msg);
    return (int)hipErrorInvalidValue;
}

inline int launch_status(const char *what)
{
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail(what, e);
}

// number of CUs of the current device (cached per device and thread)
inline int cu_count()
{
    static thread_local int cached_dev = -1, cached = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (dev != cached_dev) {
        int n = 0;
        cached = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
        cached_dev = dev;
    }
    return cached;
}

// hash of what the NPC controller depends on besides the state (tde_act_cache; act_key_steps)
inline uint32_t act_cfg_hash(const tde_config &cfg, const tde_world &w)
{
#ifdef TDE_ACT_KEY_PLAIN          // (A/B builds: the round-3 key, the step counter alone)
    return 0u;
#endif
    uint32_t h = cfg.flags & (TDE_F_NPC | TDE_F_REPLAY | TDE_F_TRAFFIC_LIGHTS);
    // the identity of the tables the controller reads (routes, spawn records, stop lines, light phases, maps, scenarios): a caller
    // that swaps or rebuilds the world under an unchanged state gets the actions recomputed, not replayed
    const void *tabs[7] = {w.route_xy, w.spawn, w.stoplines, w.phases, w.maps, w.scn, w.replay_states};
    for (int i = 0; i < 7; ++i) {
        const uint64_t a = (uint64_t)(uintptr_t)tabs[i];
        h = (h ^ (uint32_t)a) * 0x9E3779B1u;
        h = (h ^ (uint32_t)(a >> 32)) * 0x9E3779B1u;
    }
    const int32_t dims[6] = {w.n_routes, w.RW, w.n_replay, w.RT, w.n_scn, w.n_maps};
    for (int i = 0; i < 6; ++i) h = (h ^ (uint32_t)dims[i]) * 0x9E3779B1u;
    const float c[10] = {cfg.npc_k_steer, cfg.npc_k_speed, cfg.npc_gap_s0, cfg.npc_cone_k, cfg.npc_lane_half, cfg.npc_reach,
                         cfg.npc_max_accel, cfg.npc_max_steer, cfg.npc_cone_range, cfg.dt};
    for (int i = 0; i < 10; ++i) {
        uint32_t b;
        memcpy(&b, &c[i], 4);
        h = (h ^ b) * 0x9E3779B1u;
    }
    return h;
}

// ---- one launcher per kernel family; each is defined by the unit that instantiates the family (build.py compiles them side by
// side).  All return 0 or a hipError_t value with the message in the error slot. -------------------------------------------------
// tde_step_trio.hip: env_step_trio_kernel<A in {8, 16, 32}, LIGHTS, OBS, MAG>
int launch_step_trio(const tde_config *cfg, const tde_world *world, const tde_state *st, uint32_t act_hash, void *stream);
// tde_step_wide.hip: env_step_wide_kernel<LIGHTS, OBS, MAG, NW = 4> (128 agent slots per env, two roles)
// (`args` = the launch's argument block in device memory, tde_api.hip: step_args; `st` = the caller's struct - shape, optional outputs, action)
int launch_step_wide(const tde::StepArgs *args, const tde_config *cfg, const tde_state *st, int waves, void *stream);
// tde_step_wide8.hip: the same kernel's eight-wavefront instantiations (launch_step_wide hands waves == 8 over)
int launch_step_wide8(const tde::StepArgs *args, const tde_config *cfg, const tde_state *st, void *stream);
// The one-role step families.  Each is two translation units, without / with tde_state.magnitudes (MAG = false / true; the split is for
// compile time), and every unit's launcher is launch_step_one_role (tde_launch.h: the choice of form is stated there).  Callers go
// through step_solo / step_routed / step_driven below, which pick the unit.
// tde_step_solo.hip / tde_step_solo_mag.hip: env_step_kernel<A, LIGHTS, OBS, BIG, WAVES, MAG>
int launch_step_solo(const tde_config *cfg, const tde_world *world, const tde_state *st, void *stream);
int launch_step_solo_mag(const tde_config *cfg, const tde_world *world, const tde_state *st, void *stream);
// tde_step_routed.hip / tde_step_routed_mag.hip: env_step_routed_kernel<A >= 4, LIGHTS, OBS, BIG, WAVES, MAG> (state.slot_route != NULL)
int launch_step_routed(const tde_config *cfg, const tde_world *world, const tde_state *st, void *stream);
int launch_step_routed_mag(const tde_config *cfg, const tde_world *world, const tde_state *st, void *stream);
// tde_step_driven.hip / tde_step_driven_mag.hip: env_step_driven_kernel<A, LIGHTS, OBS, BIG, WAVES, MAG> (tde_env_step_driven)
int launch_step_driven(const tde_config *cfg, const tde_world *world, const tde_state *st, const float *agent_action, const uint8_t *driven, void *stream);
int launch_step_driven_mag(const tde_config *cfg, const tde_world *world, const tde_state *st, const float *agent_action, const uint8_t *driven, void *stream);
inline int step_solo(const tde_config *cfg, const tde_world *world, const tde_state *st, void *stream)
{
    return st->magnitudes ? launch_step_solo_mag(cfg, world, st, stream) : launch_step_solo(cfg, world, st, stream);
}
inline int step_routed(const tde_config *cfg, const tde_world *world, const tde_state *st, void *stream)
{
    return st->magnitudes ? launch_step_routed_mag(cfg, world, st, stream) : launch_step_routed(cfg, world, st, stream);
}
inline int step_driven(const tde_config *cfg, const tde_world *world, const tde_state *st, const float *agent_action, const uint8_t *driven, void *stream)
{
    return st->magnitudes ? launch_step_driven_mag(cfg, world, st, agent_action, driven, stream) : launch_step_driven(cfg, world, st, agent_action, driven, stream);
}
// tde_api.hip: what every entry point that takes (config, world, state) checks first; the message names `fn`
int check_env_args(const char *fn, const tde_config *cfg, const tde_world *w, const tde_state *st);
// tde_api.hip: what tde_env_step and tde_env_step_driven ask of the batch after that.  *run = false with 0 returned: no envs, nothing to do
int check_step_batch(const char *fn, const tde_config *cfg, const tde_world *world, const tde_state *st, bool *run);
// tde_rollout_trio.hip: env_rollout_trio_kernel<A in {8, 16, 32}, LIGHTS, BIG>; env_rollout_wide_kernel<LIGHTS> (128 slots)
int launch_rollout_trio(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_rollout *ro, void *stream);
int launch_rollout_wide(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_rollout *ro, int waves, void *stream);
// tde_rollout_duo.hip: env_rollout_duo_kernel<A <= 64, LIGHTS, BIG>
int launch_rollout_duo(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_rollout *ro, void *stream);
// tde_rollout_solo.hip: env_rollout_kernel<A <= 128, LIGHTS>
int launch_rollout_solo(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_rollout *ro, void *stream);
// tde_render_scene.hip: render_scene_kernel (tde_render_scene; arguments checked by the caller)
int launch_render_scene(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_scene_view *views,
                        int32_t n_views, int32_t H, int32_t W, float fov, int32_t flags, uint8_t *out, void *stream);
// tde_near_field.hip: near_field_kernel (tde_near_field_spawn; arguments checked by the caller)
int launch_near_field(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_near_field *nf,
                      const uint8_t *mask, void *stream);
// tde_vector_obs.hip: vector_obs_kernel (tde_vector_obs; arguments checked by the caller)
int launch_vector_obs(const tde_config *cfg, const tde_world *world, const tde_state *st, const struct tde_vector_obs *vo,
                      const uint8_t *only, float *out, void *stream);
// tde_api.hip: every argument rule of tde_vector_obs, for the entry points that take the same observation (tde_agents.hip); have_out:
// the output pointer is set or not needed; the message names `fn`
int check_vector_obs_args(const char *fn, const tde_config *cfg, const tde_world *world, const tde_state *st, const struct tde_vector_obs *vo,
                          bool have_out);
// tde_planner.hip: plan_action_kernel (tde_plan_action; arguments checked by the caller)
int launch_plan_action(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_planner *pl, const uint8_t *only,
                       float *action, tde_plan_diag *diag, void *stream);
// tde_plan_set.hip: score_plans_kernel (tde_score_plans; forecast != NULL: tde_score_plans_forecast; arguments checked by the caller)
int launch_score_plans(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_planner *pl, const tde_plan_set *ps,
                       const uint8_t *only, float *cost, int32_t *fail_step, float *action, tde_plan_diag *diag, void *stream,
                       const float *forecast = nullptr, int32_t forecast_T = 0);
// tde_forecast.hip: forecast_agents_kernel (tde_forecast_agents; arguments checked by the caller)
int launch_forecast_agents(const tde_config *cfg, const tde_world *world, const tde_state *st, int32_t T, const uint8_t *only, float *out,
                           void *stream);
// tde_forecast_scene.hip: forecast_scene_kernel<A, LIGHTS> (tde_forecast_scene; arguments checked by the caller)
int launch_forecast_scene(const tde_config *cfg, const tde_world *world, const tde_state *st, int32_t T, const float *ego_action,
                          const uint8_t *only, float *out, void *stream);
// tde_plan_scene.hip: score_plans_scene_kernel<A, LIGHTS> and plan_scene_winner_kernel (tde_score_plans_scene; arguments checked by the caller)
int launch_score_plans_scene(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_planner *pl, const tde_plan_set *ps,
                             const uint8_t *only, float *cost, int32_t *fail_step, float *action, tde_plan_diag *diag, void *stream);
// tde_replay.hip: the check of a tde_replay struct that every replay entry point starts with, for the units that read the ring
// (tde_onpolicy.hip); the message names `fn`
int check_replay_struct(const char *fn, const tde_replay *rp);
// tde_terminal.hip: the ring (check_replay_struct) and the terminal pool beside it - M in [1, B], pool and ref present and aligned -
// that every entry point of tde_terminal.h that takes a pool starts with; the message names `fn`
int check_terminal_struct(const char *fn, const tde_replay *rp, const tde_terminal *tm);

}  // namespace tde_host

#define TDE_DISPATCH_A(A, ...)                                  \
    switch (A) {                                                \
        case 1: { constexpr int kA = 1; __VA_ARGS__; } break;   \
        case 2: { constexpr int kA = 2; __VA_ARGS__; } break;   \
        case 4: { constexpr int kA = 4; __VA_ARGS__; } break;   \
        case 8: { constexpr int kA = 8; __VA_ARGS__; } break;   \
        case 16: { constexpr int kA = 16; __VA_ARGS__; } break; \
        case 32: { constexpr int kA = 32; __VA_ARGS__; } break; \
        case 64: { constexpr int kA = 64; __VA_ARGS__; } break; \
    }
#define TDE_DISPATCH_A128(A, ...)                               \
    if ((A) == 128) { constexpr int kA = 128; __VA_ARGS__; } else TDE_DISPATCH_A(A, __VA_ARGS__)
