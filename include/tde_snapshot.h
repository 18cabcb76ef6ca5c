/* tde_snapshot.h — copy chosen env rows of one tde_state into chosen env rows of another (or of the same one): what a per-env
 * snapshot, a restore, a fork of one env into many and a recorder of episodes are made of.  An ADDITIVE header over tde_hip.h with a
 * version of its own: TDE_ABI_VERSION and every struct and entry point of the older headers are untouched; a library that exports
 * these symbols implements TDE_SNAPSHOT_VERSION.
 *
 * The caller owns all memory; the entry point allocates nothing on the device, works on the stream it is given, returns 0 or a
 * hipError_t value and leaves its message in tde_last_error().  Every argument rule is checked on the host before anything is launched.
 */
#ifndef TDE_SNAPSHOT_H
#define TDE_SNAPSHOT_H

#include "tde_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDE_SNAPSHOT_VERSION 1
#define TDE_SNAPSHOT_OUTPUTS (1u << 0)   /* also copy the step's outputs (the OUTPUTS group below) */
#define TDE_SNAPSHOT_CHECK (1u << 1)     /* read src_env / dst_env back and check them on the host first (synchronises the stream) */
#define TDE_SNAPSHOT_MAX_STACK 8         /* n_stack <= 8, as TDE_REPLAY_MAX_STACK */

/* The frame-stack ring of the same rows (ops.FrameStack: a ring of n_stack one-byte-per-pixel layer planes per env, and the stacked
 * colour observation made of them, oldest frame first).  Device addresses.  `layers` and `obs` are each optional as a PAIR: both
 * members NULL = not copied, one NULL and one not = refused.  Present planes are 16-byte aligned and plane % 16 == 0. */
typedef struct tde_snapshot_frames {
    const uint8_t *src_layers;  /* [src.B][n_stack][plane] */
    uint8_t *dst_layers;        /* [dst.B][n_stack][plane] */
    const uint8_t *src_obs;     /* [src.B][3 * n_stack][plane] */
    uint8_t *dst_obs;           /* [dst.B][3 * n_stack][plane] */
    int32_t n_stack, plane;     /* 1 <= n_stack <= TDE_SNAPSHOT_MAX_STACK; plane = H * W > 0 */
    int32_t src_phase, dst_phase; /* the ring slot the NEXT frame goes to, in [0, n_stack), of the source / the destination ring */
} tde_snapshot_frames;

/* For each pair k in [0, n): env row src_env[k] of `src` is written to env row dst_env[k] of `dst`.  src_env / dst_env are int32 device
 * arrays [n]; n == 0 does nothing.  src and dst may have different B and must have the same A.
 *
 * Every member of tde_state belongs to exactly one group (tests hold this list to the struct):
 *
 *   COPIED        per agent, A entries per row:  x y psi v len wid lr vdes route_wp present collided offroad slot_route
 *                 per env:                       scn steps target_idx reached episode action obs ep_return
 *   OUTPUTS       per env, only with TDE_SNAPSHOT_OUTPUTS:
 *                                                reward terminated truncated tl_violation done_bits info info_reached ep_final
 *                                                ep_final_len magnitudes
 *   INVALIDATED   never copied; the DESTINATION row is reset so that the next step rebuilds it:
 *                                                slot_cache env_cache act_cache
 *   (B and A are sizes, not arrays.)
 *
 * An array whose pointer is NULL in either state is skipped, with one exception: slot_route present in src and absent in dst is
 * refused (the routes of near-field agents would be lost silently; absent in src and present in dst is skipped like any other).
 * The copy is exact: bytes move, NaN payloads and the contents of unused slots included.
 *
 * Invalidation, in the same launch, of the destination row e of every cache dst carries: slot_cache[e * A .. e * A + A) and env_cache[e]
 * become zero bytes (TDE_CACHE_VALID clear); act_cache[e * (A + 1) .. e * (A + 1) + A) become zero bytes and the env's key entry
 * act_cache[e * (A + 1) + A] becomes the two int32 (-1, 0): episode -1, invalid.  This is what a caller who edits a state by hand must
 * do for the whole state; here it is done for the rows written and for no other.  dst's slot_cache and env_cache are 16-byte aligned,
 * its act_cache 8-byte.
 *
 * Frames (frames != NULL): layer plane j of source row s goes to plane (j - src_phase + dst_phase) mod n_stack of destination row d -
 * the ring slot of the same age - and the stacked obs row, which is oldest-first and so free of the phase, is copied as it is.
 *
 * Aliasing.  src and dst may be the same state (the same struct, or structs whose x arrays are the same): a fork.  dst_env must then
 * be disjoint from src_env, and the frames' source and destination then alias in the same way.  dst_env must always be free of
 * duplicates.  With TDE_SNAPSHOT_CHECK the two index arrays are read back (the stream is synchronised) and these rules and the ranges
 * 0 <= src_env[k] < src.B, 0 <= dst_env[k] < dst.B are checked before anything is launched; a violation is refused.  (In a process
 * without a HIP device the two arrays are read as host memory: there is nothing to launch on, and the rules can be exercised.)
 * Without the flag a pair with an index out of range is skipped by the kernel - neither row is touched - and overlapping or duplicate
 * rows are the caller's error: the result of such rows is undefined, other rows are unaffected.
 *
 * Refused on the host: NULL src / dst, A different or not a power of two in [1, TDE_MAX_AGENTS], B < 1, n < 0, NULL or misaligned index
 * arrays with n > 0, unknown flag bits, the slot_route exception, misaligned caches, and for frames: n_stack or plane out of range,
 * plane % 16 != 0, half a pair, a plane address that is not 16-byte aligned, a phase outside [0, n_stack). */
TDE_API int tde_state_copy(const tde_state *src, tde_state *dst, int32_t n, const int32_t *src_env, const int32_t *dst_env,
                           const tde_snapshot_frames *frames /* may be NULL */, uint32_t flags, void *stream);

TDE_API int tde_snapshot_version(void);

#ifdef __cplusplus
}
#endif
#endif
