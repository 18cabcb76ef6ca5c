/* tde_sequence.h — windows of consecutive steps of one env from the replay ring, for the recurrent off-policy learners (DRQN, R2D2,
 * recurrent SAC / TD3): N windows of up to T steps, each cut short where the ring says the episode stopped, with the T + 1 stacked
 * observations a window needs.  An ADDITIVE header over tde_terminal.h with a version of its own: TDE_ABI_VERSION, TDE_REPLAY_VERSION,
 * TDE_ONPOLICY_VERSION, TDE_TERMINAL_VERSION, TDE_NSTEP_VERSION, TDE_PRIORITY_VERSION and every struct and entry point of the older
 * headers are untouched; a library that exports these symbols implements TDE_SEQUENCE_VERSION.
 *
 * The ring is a tde_replay as it is, with or without a tde_terminal pool beside it.  The caller owns all memory; the entry point
 * allocates nothing, works on the stream it is given, returns 0 or a hipError_t value and leaves its message in tde_last_error().
 * Every argument rule is checked on the host before anything is launched.
 */
#ifndef TDE_SEQUENCE_H
#define TDE_SEQUENCE_H

#include "tde_terminal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDE_SEQUENCE_VERSION 1
#define TDE_SEQUENCE_MAX 256     /* T <= 256 steps per window */

/* N windows of up to T stored steps (1 <= T <= TDE_SEQUENCE_MAX), through the terminal pool when tm != NULL.  Outputs:
 *     obs     T + 1 observations per window: uint8 [N][T + 1][3 * n_stack][plane] (planes mode) / float32 [N][T + 1][D] (rows mode)
 *     action  float32 [N][T][2];  reward float32 [N][T];  done uint8 [N][T];  length int32 [N];  idx int32 [N][2]
 * obs is 16-byte aligned (rows mode: 4), action 8-byte, reward / idx / length 4-byte.
 *
 * The window.  With slot(t) = t mod C and ENDED = 3 | TDE_REPLAY_CUT, for a pair (s, e) that is a stored transition `off` slots after
 * `first` (a given pair under tde_nstep_sample's validity rule: in range, and off < count):
 *
 *     a  = min(T, count - off)                                the window never leaves the stored slots
 *     m  = the smallest k in 1 .. a with done[slot(s + k - 1)][e] & ENDED, else a          (tde_nstep.h's rule)
 *     L  = slot(s + m - 1)
 *     for k = 0 .. m - 1:
 *         obs[i][k]    = what tde_replay_sample writes as obs for the pair (slot(s + k), e), which lies off + k slots after `first`
 *                        (the frame rule and the `first` blanking rule included)
 *         action[i][k], reward[i][k] = the stored values
 *         done[i][k]   = the done byte that sampler returns for that pair (with a pool: TDE_TERMINAL_HAS where the step ended and its
 *                        frame was kept - only ever at k = m - 1)
 *     obs[i][m] = what tde_replay_sample (tm == NULL) / tde_terminal_sample (tm != NULL) writes as next_obs for (L, e): zeros after
 *                 an ending without a kept frame, the terminal stack where the pool has the frame, the stack of slot L + 1 otherwise
 *                 (the open slot when the window stops at the end of the stored range)
 *     obs[i][k] = zeros for k = m + 1 .. T;  action, reward, done = zeros for k = m .. T - 1
 *     length[i] = m;  idx[i] = (s, e)
 *
 * A given pair that is not a stored transition writes zeros everywhere, length 0, and echoes its indices.  Every output byte is written
 * exactly once.
 *
 * The draw (idx_in == NULL): window i starts at
 *
 *     wd   = philox(seed, i, draw, TDE_REPLAY_TAG)            tde_replay_sample's words
 *     skip = n_stack - 1;  span = max(1, count - skip - (T - 1))
 *     off  = skip + mulhi32(wd.x, span);  env = mulhi32(wd.y, B)
 *
 * so that a drawn window fits into the stored range whenever the range can hold one (count - skip >= T) and only an episode's end or a
 * cut shortens it.  count <= skip is refused, as tde_replay_sample refuses it.  With T == 1 the draw is tde_replay_sample's own, and
 * obs[:, 0], obs[:, 1], action[:, 0], reward[:, 0], done[:, 0] and idx equal tde_replay_sample's / tde_terminal_sample's outputs bit
 * for bit, for drawn and given pairs.  For T <= TDE_NSTEP_MAX, length equals `steps` of tde_nstep_sample(n_steps = T). */
TDE_API int tde_sequence_sample(const tde_replay *rp, const tde_terminal *tm, int32_t first, int32_t count, int32_t N,
                                const int32_t *idx_in, uint64_t seed, uint64_t draw, int32_t T, int32_t *idx, uint8_t *obs,
                                float *action, float *reward, uint8_t *done, int32_t *length, void *stream);

TDE_API int tde_sequence_version(void);

#ifdef __cplusplus
}
#endif
#endif
