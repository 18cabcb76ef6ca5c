/* tde_nstep.h — n-step returns from the replay ring, for the off-policy learners (the n_steps option of SAC, TD3 and DQN): the target
 *     r_t + gamma r_{t+1} + ... + gamma^(m-1) r_{t+m-1} + gamma^m Q(s_{t+m})
 * of a drawn step, with m cut short where the ring says the episode stopped.  An ADDITIVE header over tde_terminal.h with a version of
 * its own: TDE_ABI_VERSION, TDE_REPLAY_VERSION, TDE_ONPOLICY_VERSION, TDE_TERMINAL_VERSION and every struct and entry point of the older
 * headers are untouched; a library that exports these symbols implements TDE_NSTEP_VERSION.
 *
 * The ring is a tde_replay as it is, with or without a tde_terminal pool beside it.  The caller owns all memory; the entry point
 * allocates nothing, works on the stream it is given, returns 0 or a hipError_t value and leaves its message in tde_last_error().
 * Every argument rule is checked on the host before anything is launched.
 */
#ifndef TDE_NSTEP_H
#define TDE_NSTEP_H

#include "tde_terminal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDE_NSTEP_VERSION 1
#define TDE_NSTEP_MAX 64     /* n_steps <= 64: one lane of a wavefront per looked-at step */

/* tde_replay_sample (tm == NULL) / tde_terminal_sample (tm != NULL) with a look-ahead of up to n_steps stored steps: the same
 * arguments, the same pick of sample i - the draw philox(seed, i, draw, TDE_REPLAY_TAG) with the same skip, or the pair given through
 * idx_in under the same validity rule - and two more outputs, discount float32 [N] and steps uint8 [N].  1 <= n_steps <= TDE_NSTEP_MAX;
 * gamma is finite and in [0, 1].  With slot(t) = t mod C, for a valid pair (s, e) that lies `off` slots after `first`:
 *
 *     a  = min(n_steps, count - off)                          the look-ahead never leaves the stored slots
 *     m  = the smallest k in 1 .. a with done[slot(s + k - 1)][e] & (3 | TDE_REPLAY_CUT), else a
 *     L  = slot(s + m - 1)                                    the last step of the look-ahead
 *     R  = reward[s][e];  g = gamma
 *     for k = 1 .. m - 1:   R = R + g * reward[slot(s + k)][e]      the product rounded to float32, then the sum: no fused
 *                           g = g * gamma                           multiply-add, in this order
 *     reward[i] = R;  discount[i] = g  (gamma multiplied m times: gamma^m);  steps[i] = m
 *     action[i] = action[s][e];  idx[i] = (s, e)
 *     obs[i]      = what tde_replay_sample writes as obs for (s, e)
 *     next_obs[i] = what tde_replay_sample (tm == NULL) / tde_terminal_sample (tm != NULL) writes as next_obs for the pair (L, e),
 *                   which lies off + m - 1 slots after `first`
 *     done[i]     = the done byte they return for (L, e)  (TDE_TERMINAL_HAS included)
 *
 * so that the learner's target is reward + discount * bootstrap(done) * Q(next_obs).  next_obs is therefore zeros after an ending
 * without a kept frame, the terminal stack where the pool has the frame, and the stack of slot L + 1 otherwise, under age[L + 1] and
 * the `first` blanking rule - slot L + 1 is the open slot when the look-ahead stops at the end of the stored range, and the open slot
 * holds its frame by construction.  A given pair that is not a stored transition gathers zeros everywhere (discount 0, steps 0) and
 * echoes its indices.  With n_steps == 1 every output tde_replay_sample / tde_terminal_sample has equals theirs bit for bit.
 * discount is 4-byte aligned.  Every output byte is written exactly once. */
TDE_API int tde_nstep_sample(const tde_replay *rp, const tde_terminal *tm, int32_t first, int32_t count, int32_t N,
                             const int32_t *idx_in, uint64_t seed, uint64_t draw, int32_t n_steps, float gamma, int32_t *idx,
                             uint8_t *obs, uint8_t *next_obs, float *action, float *reward, uint8_t *done, float *discount,
                             uint8_t *steps, void *stream);

TDE_API int tde_nstep_version(void);

#ifdef __cplusplus
}
#endif
#endif
