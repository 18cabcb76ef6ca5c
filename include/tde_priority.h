/* tde_priority.h — prioritized experience replay (Schaul et al.) over the replay ring: an integer priority per stored transition, a
 * draw proportional to it, an update from the learner's TD errors, and the bookkeeping that keeps a priority from outliving its
 * transition as the ring turns.  An ADDITIVE header over tde_replay.h with a version of its own: TDE_ABI_VERSION, TDE_REPLAY_VERSION,
 * TDE_ONPOLICY_VERSION, TDE_TERMINAL_VERSION, TDE_NSTEP_VERSION and every struct and entry point of the older headers are untouched; a
 * library that exports these symbols implements TDE_PRIORITY_VERSION.
 *
 * Priorities are INTEGERS (16.16 fixed point), so every sum is exact and independent of the order it was made in: the draw is a pure
 * function of the leaves, the seed and the draw counter, and can be held bit for bit.  The pick is a kernel of its own; the batch is
 * then gathered by tde_replay_sample / tde_terminal_sample / tde_nstep_sample with the picked pairs as idx_in.
 *
 * The ring is a tde_replay as it is.  The caller owns all memory; the entry points allocate nothing, work on the stream they are
 * given, return 0 or a hipError_t value and leave their message in tde_last_error().  Every argument rule is checked on the host
 * before anything is launched.
 */
#ifndef TDE_PRIORITY_H
#define TDE_PRIORITY_H

#include "tde_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDE_PRIORITY_VERSION 1

typedef struct tde_priority {
    uint32_t *leaf;   /* [C][B], (slot, env) order as the ring's own arrays: the integer priority q of the pair, 0 = not drawable;
                         16-byte aligned */
    uint64_t *sums;   /* tde_priority_words(C, B) words, caller-owned scratch; sums[0] == total == sum of all leaves after every
                         entry point (in stream order); the rest is the implementation's */
    uint32_t *qmax;   /* [1]: the largest q any update has written, at least TDE_PRIORITY_ONE; new transitions enter with it */
} tde_priority;
#define TDE_PRIORITY_ONE  (1u << 16)   /* q of priority 1.0 */
#define TDE_PRIORITY_QMAX (1u << 28)
#define TDE_PRIORITY_TAG  0x5052u      /* fourth Philox counter word of the draws */

/* THE INVARIANT.  After every entry point, leaf[s][e] != 0 exactly for the pairs that are stored transitions with their whole frame
 * stack in the ring under the (first, count) the call was given:
 *     off = (s - first) mod C < count   and   min(age[s][e], n_stack - 1) <= off
 * (what tde_replay_sample's idx_in may be given without gathering zeros or blank older frames).  C * B leaves; a leaf is < 2^28 + 1,
 * so the total of any ring the ABI can describe fits 64 bits. */

/* Words of `sums` a ring of C slots and B envs needs (host only): the inner nodes of a 64-ary sum tree over the C * B leaves.
 * -1 (and a message) when C < 2 or B < 1. */
TDE_API int64_t tde_priority_words(int32_t C, int32_t B);

/* Every leaf and every word of sums = 0, *qmax = TDE_PRIORITY_ONE: the buffer's first begin(). */
TDE_API int tde_priority_reset(const tde_priority *pr, const tde_replay *rp, void *stream);

/* After tde_replay_push filled slot w; first and count are the host's values AFTER it advanced (so w is the newest stored slot:
 * (first + count - 1) mod C, and count >= 1).  For every env e, in this order:
 *     leaf[w][e] = *qmax                                   the new transition enters with the largest priority seen
 *     leaf[(w + 1) mod C][e] = 0                           the open slot
 *     for d = 0 .. min(n_stack - 1, count) - 1:            the stacks whose older frames the ring just overwrote
 *         s = (first + d) mod C;  if min(age[s][e], n_stack - 1) > d:  leaf[s][e] = 0
 * then total is made current. */
TDE_API int tde_priority_push(const tde_priority *pr, const tde_replay *rp, int32_t w, int32_t first, int32_t count, void *stream);

/* New priorities p float32 [N] for the pairs idx int32 [N][2] (slot, env) - the idx a sample returned.  Entry i is quantised as
 *     q_i = clamp(rint(p_i * 65536.0f), 1, TDE_PRIORITY_QMAX)     rint to nearest, ties to even; the scaling is exact in float32
 * so NaN and p_i <= 0 give 1 and +inf gives TDE_PRIORITY_QMAX.  A pair that is out of range or not valid under the invariant's rule is
 * IGNORED: an index sampled before the ring overwrote its slot does not resurrect a dead leaf.  Every valid pair named gets
 * leaf = max of the q_i of the entries that name it (duplicates in a minibatch are order-independent), *qmax = max(*qmax, q_i of the
 * valid entries), then total is made current.  count may be 0 (every pair is then ignored). */
TDE_API int tde_priority_update(const tde_priority *pr, const tde_replay *rp, int32_t first, int32_t count, int32_t N,
                                const int32_t *idx, const float *p, void *stream);

/* Draw N pairs in proportion to their leaves, stratified.  With T = total, base = T / N, rem = T % N:
 *     lo_i   = i * base + min(i, rem),  span_i = base + (i < rem)        an exact partition of [0, T) into N strata
 *     wd     = philox(seed, i, (uint32_t)draw, (uint32_t)(draw >> 32), TDE_PRIORITY_TAG),   r = (uint64_t)wd.x << 32 | wd.y
 *     u_i    = lo_i + mulhi64(r, span_i)          (mulhi64: the high 64 bits of the 64 x 64 bit product)
 *     u_i    = mulhi64(r, T)                      for every i when base == 0 (fewer priority units than samples)
 * the pick is the leaf l, in flat slot * B + env order, with cum(l - 1) <= u_i < cum(l), cum the inclusive prefix sum of the leaves:
 *     idx[i] = (l / B, l % B),  q[i] = leaf[l]
 * T == 0 writes idx[i] = (-1, -1) and q[i] = 0 for every i (the gathers turn such a pair into zeros).  first and count are checked
 * as every sampler checks them; the pick itself reads leaf and sums only.  Every output word is written exactly once. */
TDE_API int tde_priority_sample(const tde_priority *pr, const tde_replay *rp, int32_t first, int32_t count, int32_t N, uint64_t seed,
                                uint64_t draw, int32_t *idx, uint32_t *q, void *stream);

TDE_API int tde_priority_version(void);

#ifdef __cplusplus
}
#endif
#endif
