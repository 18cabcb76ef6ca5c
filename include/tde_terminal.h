/* tde_terminal.h — terminal observations beside the replay ring: the frame a finished env showed before it was re-spawned, so that a
 * truncated episode (in this environment the SUCCESS case: max_environment_steps reached, ref gym_env.py:135, 145) can bootstrap from it
 * as SB3 does from info["terminal_observation"].  An ADDITIVE header over tde_replay.h with a version of its own: TDE_ABI_VERSION,
 * TDE_REPLAY_VERSION, TDE_ONPOLICY_VERSION and every struct and entry point of the older headers are untouched; a library that exports
 * these symbols implements TDE_TERMINAL_VERSION.
 *
 * The ring is a tde_replay as it is, filled by tde_replay_begin / tde_replay_push.  What this header adds is a pool of terminal frames
 * beside it - dense per slot, sparse per env: M rows per ring slot, not B, because ~1 % of the steps end an episode - and a sample
 * that returns a pooled frame as the newest frame of next_obs.  The caller owns all memory; the entry points allocate nothing, work on
 * the stream they are given, return 0 or a hipError_t value and leave their message in tde_last_error().  Every argument rule is
 * checked on the host before anything is launched.
 */
#ifndef TDE_TERMINAL_H
#define TDE_TERMINAL_H

#include "tde_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDE_TERMINAL_VERSION 1

typedef struct tde_terminal {
    int32_t  M;        /* pool rows per ring slot, 1 .. B */
    uint8_t *pool;     /* planes: uint8 [C][M][plane] layer bytes; rows: float32 [C][M][D] */
    int32_t *ref;      /* [C][B]: row of pool[slot] holding this transition's terminal frame, or -1 */
} tde_terminal;
#define TDE_TERMINAL_HAS 0x40   /* ORed into the done byte tde_terminal_sample RETURNS, never into the ring (tde_state.done_bits uses
                                   bits 0-4, TDE_REPLAY_CUT bit 7): next_obs holds the terminal observation */

/* Alignment: planes mode moves 16 bytes per lane, so pool, src / term_src, dst and the strides are multiples of 16 there; rows mode
 * needs 4.  ref is 4-byte aligned. */

/* The masked copy an env makes between observing and re-spawning: dst + e * row_bytes = src + e * src_stride (row_bytes bytes) for the
 * envs with done_bits[e] & 3; the other envs' entries of dst are untouched.  row_bytes is a plane or a float32 row: a multiple of 4.
 * When it is a multiple of 16 (every plane is), src, dst and src_stride must be multiples of 16 too and the copy moves 16 bytes per
 * lane; otherwise they are multiples of 4.  One lane per env finds the finished envs, one wavefront per finished env copies. */
TDE_API int tde_terminal_stash(int32_t B, int32_t row_bytes, const uint8_t *done_bits, const uint8_t *src, int64_t src_stride,
                               uint8_t *dst, void *stream);

/* Beside tde_replay_push for slot w, before the host advances w: with r(e) = the number of envs e' < e with done_bits[e'] & 3,
 *     ref[w][e]     = r(e)  if done_bits[e] & 3 and r(e) < M,  else -1          (every ref[w][*] is written on every push: a slot
 *                                                                                the ring overwrites is thereby freed)
 *     pool[w][r(e)] = term_src + e * term_stride  (one plane / row)              for those envs
 * The rank is a scan over the done mask in env order - the same call gives the same rows, whatever the schedule - and overflow is
 * defined: the first M finished envs in env order are kept, the others behave as without this header.  Pool rows at or above the
 * number kept are not written. */
TDE_API int tde_terminal_push(const tde_replay *rp, const tde_terminal *tm, int32_t w, const uint8_t *done_bits, const uint8_t *term_src,
                              int64_t term_stride, void *stream);

/* tde_replay_sample with the pool beside it: the same arguments, the same index draw (TDE_REPLAY_TAG, skip), the same outputs, every
 * output byte written exactly once - with one difference.  Where done[s][e] & 3 and ref[s][e] >= 0 (whether or not TDE_REPLAY_CUT is
 * set as well):
 *     planes mode: next_obs[i] is a stack whose newest frame is pool[s][ref[s][e]] through the palette and whose older frames
 *                  j < n_stack - 1 are frames j + 1 of obs[i] (the same slots under the same age[s][e] / `first` blanking rule);
 *     rows mode:   next_obs[i] is the pool row;
 *     done[i] has TDE_TERMINAL_HAS set.
 * A transition that is only cut, or that ended and overflowed the pool, still gets zeros and no TDE_TERMINAL_HAS. */
TDE_API int tde_terminal_sample(const tde_replay *rp, const tde_terminal *tm, int32_t first, int32_t count, int32_t N,
                                const int32_t *idx_in, uint64_t seed, uint64_t draw, int32_t *idx, uint8_t *obs, uint8_t *next_obs,
                                float *action, float *reward, uint8_t *done, void *stream);

TDE_API int tde_terminal_version(void);

#ifdef __cplusplus
}
#endif
#endif
