/* tde_replay.h — a device-resident replay buffer for the off-policy algorithms (SAC, TD3: the reference trainer's defaults, ref
 * examples/rl_training.py:166-183): an ADDITIVE header over tde_abi.h with a version of its own.  TDE_ABI_VERSION and every struct
 * of tde_abi.h / entry point of tde_hip.h are untouched; a library that exports these symbols implements TDE_REPLAY_VERSION.
 *
 * The buffer is a ring over time of C slots, one entry per env and slot.  The caller owns all memory; the entry points allocate
 * nothing, work on the stream they are given, return 0 or a hipError_t value and leave their message in tde_last_error().
 *
 * Birdview observations are kept as ONE layer plane (one byte per pixel, tde_render.layers) per env and step - 4096 bytes per
 * transition at 64 x 64 against the 2 * 3 * n_stack * 4096 of a store of stacked obs + next_obs - and both stacks are rebuilt at
 * sample time through the palette (TDE_RGB_*).  Vector / state observations are kept as float32 rows.
 */
#ifndef TDE_REPLAY_H
#define TDE_REPLAY_H

#include "tde_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TDE_REPLAY_VERSION 1

#ifndef TDE_API
#define TDE_API __attribute__((visibility("default")))
#endif

typedef struct tde_replay {
    int32_t C, B;            /* slots (>= 2 and >= n_stack + 1), envs */
    int32_t n_stack;         /* 1 .. 8: frames per stacked observation (planes mode); 1 in rows mode */
    int32_t plane;           /* planes mode: H*W bytes per frame, a multiple of 16, <= 4096; rows mode: 0 */
    int32_t D;               /* rows mode: float32 values per observation row (> 0); planes mode: 0 */
    uint8_t *frames;         /* planes: uint8 [C][B][plane] layer bytes; rows: float32 [C][B][D] */
    float   *action;         /* [C][B][2] */
    float   *reward;         /* [C][B] */
    uint8_t *done;           /* [C][B]: tde_state.done_bits of the step taken from this slot (bit0 terminated, bit1 truncated,
                                bit2 offroad, bit3 collided, bit4 red light) | TDE_REPLAY_CUT */
    uint8_t *age;            /* [C][B]: steps since the episode of this slot's frame began, saturating at 255 */
} tde_replay;
#define TDE_REPLAY_CUT 0x80  /* set by the buffer, never by the step: the env was reset by the caller after this slot, so its
                                successor is not this transition's next observation */
#define TDE_REPLAY_TAG 0x5250u /* fourth Philox counter word of the index draws */
#define TDE_REPLAY_MAX_STACK 8
#define TDE_REPLAY_MAX_PLANE 4096

/* Slot s holds, per env e: frame[s][e], the newest frame of the observation the env showed at time s; the action, reward and
 * done bits of the step taken from that observation; age[s][e].  The frame that follows a transition is frame[(s + 1) % C][e]:
 * it always exists, because the slot being filled (the "open" slot w) already holds its frame.  The valid transitions are the
 * `count` slots first, first + 1, ... (mod C) up to, not including, w; the host tracks first, w and count (count <= C - 1).
 *
 * Alignment: planes mode moves 16 bytes per lane, so frames, src and src_stride are multiples of 16 there; rows mode needs 4. */

/* Write the open slot's frame: frames[w][e] = src + e * src_stride (one plane / row per env; in planes mode the newest ring slot
 * of a tde_render.layers ring with src_stride = n_stack * plane) and age[w][e] = 0, for the envs of `mask` (uint8 [B], nonzero =
 * taken; NULL = every env: the buffer's first call after a reset of all envs).  With a mask it also ORs TDE_REPLAY_CUT into
 * done[(w - 1) % C][e] of the masked envs: the caller's mid-run reset(mask).  (When w == first, slot w - 1 holds no transition:
 * the bit lands in a slot that the push which fills it overwrites.) */
TDE_API int tde_replay_begin(const tde_replay *rp, int32_t w, const uint8_t *src, int64_t src_stride, const uint8_t *mask,
                             void *stream);

/* After a step: action [B][2], reward [B] and done_bits [B] go to slot w, the new frame to slot w1 = (w + 1) % C, and
 * age[w1][e] = (done_bits[e] & 3) ? 0 : min(age[w][e] + 1, 255).  One launch, one wavefront per env.  The host then advances w,
 * and `first` too when w1 was `first` (the ring is full). */
TDE_API int tde_replay_push(const tde_replay *rp, int32_t w, const float *action, const float *reward, const uint8_t *done_bits,
                            const uint8_t *src, int64_t src_stride, void *stream);

/* Gather N transitions.  idx_in == NULL: transition i is drawn as
 *     wd   = philox(seed, i, (uint32_t)draw, (uint32_t)(draw >> 32), TDE_REPLAY_TAG)
 *     slot = (first + skip + mulhi32(wd.x, count - skip)) % C,   env = mulhi32(wd.y, B),   skip = n_stack - 1
 * (mulhi32: the high word of the 32 x 32 bit product, as the reset draws its scenario).  A drawn slot lies at least n_stack - 1
 * slots behind `first`, so the n_stack - 1 older frames of its stack are slots of the valid range themselves: every frame a drawn
 * transition needs is still in the ring, whatever its age.  count <= n_stack - 1 is refused.
 * idx_in != NULL: int32 [N][2] (slot, env) pairs of the caller's (tests, prioritised replay, a host-side sampler).  A pair whose
 * slot is outside the valid range or whose env is outside [0, B) gathers zeros (done = 0).
 * idx [N][2] always receives the pairs used.
 *
 * Planes mode: obs[i] is uint8 [3 * n_stack][plane]; frame j (oldest first) is slot s - d, d = n_stack - 1 - j, of env e expanded
 * through the palette, or zeros when d > age[s][e] (the frame belongs to the previous episode or to nothing; TDE_LAYER_BLANK
 * expands to (0, 0, 0)) or when slot s - d lies before `first` (overwritten: only pairs given through idx_in can ask for it).
 * next_obs[i] is the same construction from slot s + 1 with age[s + 1], or zeros when done[s][e] & (3 | TDE_REPLAY_CUT): a finished
 * env is re-spawned inside the step, so the terminal frame is never rendered and such a transition has no next observation - the
 * learner masks its bootstrap with the returned done.
 * Rows mode: obs[i] = row of slot s, next_obs[i] = row of slot s + 1 or zeros when the transition ended or was cut.
 * action [N][2], reward [N], done [N] are copied from the slot.  Every output byte is written exactly once. */
TDE_API int tde_replay_sample(const tde_replay *rp, int32_t first, int32_t count, int32_t N, const int32_t *idx_in, uint64_t seed,
                              uint64_t draw, int32_t *idx, uint8_t *obs, uint8_t *next_obs, float *action, float *reward,
                              uint8_t *done, void *stream);

/* Planes mode without a layer ring (n_stack == 1: the rasteriser then writes colours only): colour observations rgb + e *
 * rgb_stride, uint8 [3][plane] per env, back to layer planes planes + e * planes_stride - the inverse of the palette (its eight
 * colours are distinct; any other colour becomes TDE_LAYER_BLANK).  Both strides and pointers are multiples of 16. */
TDE_API int tde_replay_pack(const tde_replay *rp, const uint8_t *rgb, int64_t rgb_stride, uint8_t *planes, int64_t planes_stride,
                            void *stream);

TDE_API int tde_replay_version(void);

#ifdef __cplusplus
}
#endif
#endif
