/* tde_onpolicy.h — the on-policy side of the replay ring (PPO, A2C: the other two algorithms of the reference trainer, ref
 * examples/rl_training.py with env_configs/<name>/{ppo,a2c}_training.yml): an ADDITIVE header over tde_replay.h with a version of its own.
 * TDE_ABI_VERSION, TDE_REPLAY_VERSION and every struct and entry point of tde_abi.h / tde_hip.h / tde_replay.h are untouched; a
 * library that exports these symbols implements TDE_ONPOLICY_VERSION.
 *
 * The store is a tde_replay ring, filled by tde_replay_begin / tde_replay_push as it is.  What this header adds is the time-ordered
 * view of its newest steps, generalised advantage estimation over them, and a minibatch gather that writes observations only.
 * The caller owns all memory; the entry points allocate nothing, work on the stream they are given, return 0 or a hipError_t value
 * and leave their message in tde_last_error().
 */
#ifndef TDE_ONPOLICY_H
#define TDE_ONPOLICY_H

#include "tde_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDE_ONPOLICY_VERSION 1

/* The rollout is the newest T valid slots of the ring (first, count: as tde_replay_sample takes them): its step t, 0 <= t < T, is
 * slot s(t) = (first + count - T + t) % C.  T >= 1 and count >= T (and count <= C - 1, first in [0, C)) are required.  The per-step
 * side data of the learner - values, log-probabilities, advantages, returns - are float32 [T][B] arrays of the caller's, indexed by
 * the step t, not by the slot.  Every argument rule is checked on the host before anything is launched. */

/* Generalised advantage estimation (SB3's RolloutBuffer.compute_returns_and_advantage) over the rollout.  Per env e, for
 * t = T - 1 ... 0, in float32 with one IEEE rounding per written operation, in exactly this order:
 *     nnt   = (done[s(t)][e] & (3 | TDE_REPLAY_CUT)) == 0
 *     nv    = t == T - 1 ? last_values[e] : values[t + 1][e]
 *     delta = (reward[s(t)][e] + (nnt ? gamma * nv : 0.0f)) - values[t][e]
 *     last  = delta + (nnt ? gl * last : 0.0f)          (gl = gamma * lam, rounded once to float32; last starts at 0)
 *     advantages[t][e] = last;   returns[t][e] = last + values[t][e]
 * "The next step starts an episode" is read from the done bits of the step itself: a terminated, truncated or caller-cut step does
 * not bootstrap.  (A finished env is re-spawned inside the step, the terminal frame is never rendered, so there is no terminal value
 * to bootstrap a truncated episode from: SB3's timeout bootstrap is not offered, as in tde_replay_sample.)
 * values [T][B], last_values [B]: the critic's value of the observation each step was taken from / of the observation after the last
 * step.  advantages and returns [T][B] are written whole; they may not overlap the inputs.  All float arrays are 4-byte aligned. */
TDE_API int tde_gae(const tde_replay *rp, int32_t first, int32_t count, int32_t T, const float *values, const float *last_values,
                    float gamma, float lam, float *advantages, float *returns, void *stream);

/* Gather N samples of the rollout.  idx [N] holds t * B + e (T * B <= INT32_MAX is required).
 * obs[i] is what tde_replay_sample writes as obs for the pair (s(t), e): planes mode uint8 [3 * n_stack][plane] through the palette,
 * frame j (oldest first) being slot s(t) - d, d = n_stack - 1 - j, or zeros when d > age[s(t)][e] or when that slot lies before
 * `first`; rows mode the float32 row [D].  No next observation is written.
 * action[i] = action[s(t)][e]; old_values, old_log_prob, adv_out, ret_out [i] = values, log_prob, advantages, returns [t][e].
 * An idx[i] outside [0, T * B) gathers zeros everywhere.  Every output byte is written exactly once.
 * Alignment: obs as tde_replay_sample's (16 bytes in planes mode, 4 in rows mode), action 8, everything else 4. */
TDE_API int tde_onpolicy_gather(const tde_replay *rp, int32_t first, int32_t count, int32_t T, int32_t N, const int32_t *idx,
                                const float *values, const float *log_prob, const float *advantages, const float *returns,
                                uint8_t *obs, float *action, float *old_values, float *old_log_prob, float *adv_out, float *ret_out,
                                void *stream);

TDE_API int tde_onpolicy_version(void);

#ifdef __cplusplus
}
#endif
#endif
