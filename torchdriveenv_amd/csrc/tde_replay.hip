// tde_replay.hip — the device-resident replay buffer of include/tde_replay.h: its kernels, its host-side checks and its four entry
// points (a translation unit of its own: no existing kernel includes it).
//   * tde_replay_begin / tde_replay_push: one wavefront per env copies the env's newest layer plane (or float32 row) into its slot of
//     the ring with 16-byte loads and stores; lane 0 writes the slot's scalars.  kRingWaves envs per workgroup (a one-env workgroup
//     costs ~8 us per launch at 8192 envs with nothing to do, profiles/near_field_kernel_stats.txt).
//   * tde_replay_sample: tde_ring.h's gather (ring_gather_planes_kernel / ring_gather_rows_kernel) without a terminal pool.  Planes mode:
//     one workgroup per drawn transition, one wavefront per source slot s - n_stack + 1 .. s + 1.  A wavefront reads its plane once
//     (four 16-byte loads per lane at 64 x 64, in flight together: the last stage of the rasteriser) and expands it through
//     raster_expand into the frame of `obs` and / or of `next_obs` it belongs to - or writes zeros there.  Every wavefront repeats the
//     draw (ten Philox rounds on wave-uniform values) instead of waiting for one that did.  Rows mode: one wavefront per transition
//     copies its two rows.
//   * tde_replay_pack: colour observations back to layer planes, for buffers over an env without a layer ring.
// All offsets into frames / obs / next_obs are int64_t: C * B * plane passes 2^31 at the sizes the buffer is for.
// The specification is restated in numpy by tests/replay_ref.py.
#include "tde_ring.h"

namespace tde {

struct ReplayArgs {
    tde_replay rp;
    int64_t row;                        // bytes per frame / row of `frames`
    bool vec;                           // rows move as 16-byte words (planes mode always)
};

__global__ __launch_bounds__(64 * kRingWaves) void replay_begin_kernel(ReplayArgs a, int w, const uint8_t *src, int64_t src_stride,
                                                                         const uint8_t *mask)
{
    const int lane = (int)(threadIdx.x & 63u), e = (int)blockIdx.x * kRingWaves + (int)(threadIdx.x >> 6);
    if (e >= a.rp.B) return;
    if (mask && !mask[e]) return;
    const int64_t at = (int64_t)w * a.rp.B + e;
    ring_copy_row(a.rp.frames + at * a.row, src + (int64_t)e * src_stride, (int)a.row, a.vec, lane);
    if (lane == 0) {
        a.rp.age[at] = 0;
        if (mask) {
            const int64_t prev = (int64_t)ring_slot(w, -1, a.rp.C) * a.rp.B + e;
            a.rp.done[prev] = (uint8_t)(a.rp.done[prev] | TDE_REPLAY_CUT);
        }
    }
}

__global__ __launch_bounds__(64 * kRingWaves) void replay_push_kernel(ReplayArgs a, int w, const float *action, const float *reward,
                                                                        const uint8_t *done_bits, const uint8_t *src, int64_t src_stride)
{
    const int lane = (int)(threadIdx.x & 63u), e = (int)blockIdx.x * kRingWaves + (int)(threadIdx.x >> 6);
    if (e >= a.rp.B) return;
    const int64_t at = (int64_t)w * a.rp.B + e, at1 = (int64_t)ring_slot(w, 1, a.rp.C) * a.rp.B + e;
    ring_copy_row(a.rp.frames + at1 * a.row, src + (int64_t)e * src_stride, (int)a.row, a.vec, lane);
    if (lane == 0) {
        const uint8_t db = done_bits[e];
        reinterpret_cast<float2 *>(a.rp.action)[at] = reinterpret_cast<const float2 *>(action)[e];
        a.rp.reward[at] = reward[e];
        a.rp.done[at] = db;
        const int age = a.rp.age[at];
        a.rp.age[at1] = (uint8_t)((db & 3) ? 0 : (age < 255 ? age + 1 : 255));
    }
}

// 16 colour bytes of each channel -> 16 layer bytes: the palette's inverse, byte by byte
TDE_DEV uint32_t replay_layer_of(uint32_t r, uint32_t g, uint32_t b)
{
    const uint32_t BG[3] = {TDE_RGB_BACKGROUND}, ROAD[3] = {TDE_RGB_ROAD}, WP[3] = {TDE_RGB_WAYPOINT}, NPC[3] = {TDE_RGB_NPC},
                   EGO[3] = {TDE_RGB_EGO}, SRED[3] = {TDE_RGB_STOP_RED}, SGO[3] = {TDE_RGB_STOP_GO};
    const uint32_t c = r | (g << 8) | (b << 16);
    auto key = [](const uint32_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16); };
    uint32_t lay = TDE_LAYER_BLANK;
    lay = c == key(BG) ? (uint32_t)TDE_LAYER_BACKGROUND : lay;
    lay = c == key(ROAD) ? (uint32_t)TDE_LAYER_ROAD : lay;
    lay = c == key(WP) ? (uint32_t)TDE_LAYER_WAYPOINT : lay;
    lay = c == key(NPC) ? (uint32_t)TDE_LAYER_NPC : lay;
    lay = c == key(EGO) ? (uint32_t)TDE_LAYER_EGO : lay;
    lay = c == key(SRED) ? (uint32_t)TDE_LAYER_STOP_RED : lay;
    lay = c == key(SGO) ? (uint32_t)TDE_LAYER_STOP_GO : lay;
    return lay;
}

TDE_DEV uint32_t replay_layers4(uint32_t r, uint32_t g, uint32_t b)
{
    uint32_t o = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) o |= replay_layer_of((r >> (8 * k)) & 255u, (g >> (8 * k)) & 255u, (b >> (8 * k)) & 255u) << (8 * k);
    return o;
}

__global__ __launch_bounds__(64 * kRingWaves) void replay_pack_kernel(int B, int plane, const uint8_t *rgb, int64_t rgb_stride,
                                                                        uint8_t *planes, int64_t planes_stride)
{
    const int lane = (int)(threadIdx.x & 63u), e = (int)blockIdx.x * kRingWaves + (int)(threadIdx.x >> 6);
    if (e >= B) return;
    const uint8_t *s = rgb + (int64_t)e * rgb_stride;
    uint4 *d = reinterpret_cast<uint4 *>(planes + (int64_t)e * planes_stride);
    for (int i = lane; i < plane / 16; i += 64) {
        const uint4 r = reinterpret_cast<const uint4 *>(s)[i], g = reinterpret_cast<const uint4 *>(s + plane)[i],
                    b = reinterpret_cast<const uint4 *>(s + 2 * plane)[i];
        d[i] = make_uint4(replay_layers4(r.x, g.x, b.x), replay_layers4(r.y, g.y, b.y), replay_layers4(r.z, g.z, b.z),
                          replay_layers4(r.w, g.w, b.w));
    }
}

}  // namespace tde

using namespace tde_host;

namespace {

// the struct alone (every entry point); fills the launch's argument block
int check_replay(const char *fn, const tde_replay *rp, tde::ReplayArgs &a)
{
    if (!rp) return bad_in(fn, "NULL argument");
    if (rp->B < 1) return bad_in(fn, "B must be >= 1");
    const bool planes = rp->plane > 0 && rp->D == 0, rows = rp->plane == 0 && rp->D > 0;
    if (!planes && !rows) return bad_in(fn, "exactly one of plane (planes mode) and D (rows mode) must be > 0");
    if (planes && (rp->n_stack < 1 || rp->n_stack > TDE_REPLAY_MAX_STACK)) return bad_in(fn, "n_stack must be in [1, 8]");
    if (rows && rp->n_stack != 1) return bad_in(fn, "n_stack must be 1 in rows mode");
    if (planes && (rp->plane % 16 != 0 || rp->plane > TDE_REPLAY_MAX_PLANE)) return bad_in(fn, "plane must be a multiple of 16, at most 4096");
    if (rp->C < 2 || rp->C < rp->n_stack + 1) return bad_in(fn, "C must be >= 2 and >= n_stack + 1");
    if (!rp->frames || !rp->action || !rp->reward || !rp->done || !rp->age) return bad_in(fn, "a NULL array in the buffer");
    if (!aligned(rp->frames, planes ? 16 : 4) || !aligned(rp->action, 8) || !aligned(rp->reward, 4))
        return bad_in(fn, "frames must be 16-byte aligned (rows mode: 4), action 8-byte, reward 4-byte");
    a.rp = *rp;
    a.row = planes ? (int64_t)rp->plane : (int64_t)rp->D * 4;
    a.vec = planes;
    return 0;
}

unsigned env_blocks(int B) { return ring_blocks(B, tde::kRingWaves); }

}  // namespace

int tde_host::check_replay_struct(const char *fn, const tde_replay *rp)
{
    tde::ReplayArgs a;
    return check_replay(fn, rp, a);
}

int tde_replay_version(void) { return TDE_REPLAY_VERSION; }

int tde_replay_begin(const tde_replay *rp, int32_t w, const uint8_t *src, int64_t src_stride, const uint8_t *mask, void *stream)
{
    const char *fn = "tde_replay_begin";
    tde::ReplayArgs a;
    int rc = check_replay(fn, rp, a);
    if (rc) return rc;
    if ((rc = check_slot(fn, rp, w)) != 0 || (rc = check_src(fn, a.row, a.vec, src, src_stride, "src", "src_stride")) != 0) return rc;
    tde::replay_begin_kernel<<<env_blocks(rp->B), 64 * tde::kRingWaves, 0, (hipStream_t)stream>>>(a, w, src, src_stride, mask);
    return tde_host::launch_status(fn);
}

int tde_replay_push(const tde_replay *rp, int32_t w, const float *action, const float *reward, const uint8_t *done_bits,
                    const uint8_t *src, int64_t src_stride, void *stream)
{
    const char *fn = "tde_replay_push";
    tde::ReplayArgs a;
    int rc = check_replay(fn, rp, a);
    if (rc) return rc;
    if (!action || !reward || !done_bits) return bad_in(fn, "NULL argument");
    if (!aligned(action, 8) || !aligned(reward, 4)) return bad_in(fn, "action must be 8-byte aligned, reward 4-byte");
    if ((rc = check_slot(fn, rp, w)) != 0 || (rc = check_src(fn, a.row, a.vec, src, src_stride, "src", "src_stride")) != 0) return rc;
    tde::replay_push_kernel<<<env_blocks(rp->B), 64 * tde::kRingWaves, 0, (hipStream_t)stream>>>(a, w, action, reward, done_bits, src,
                                                                                                   src_stride);
    return tde_host::launch_status(fn);
}

int tde_replay_sample(const tde_replay *rp, int32_t first, int32_t count, int32_t N, const int32_t *idx_in, uint64_t seed, uint64_t draw,
                      int32_t *idx, uint8_t *obs, uint8_t *next_obs, float *action, float *reward, uint8_t *done, void *stream)
{
    const char *fn = "tde_replay_sample";
    tde::SampleArgs s;
    int rc = check_replay_struct(fn, rp);
    if (rc || (rc = check_sample(fn, rp, first, count, N, idx_in, seed, draw, idx, obs, next_obs, action, reward, done, s)) != 0) return rc;
    return launch_sample(fn, s, N, stream);
}

int tde_replay_pack(const tde_replay *rp, const uint8_t *rgb, int64_t rgb_stride, uint8_t *planes, int64_t planes_stride, void *stream)
{
    const char *fn = "tde_replay_pack";
    tde::ReplayArgs a;
    int rc = check_replay(fn, rp, a);
    if (rc) return rc;
    // (the kernel takes B and plane of the struct and nothing else: ops.replay_pack_struct builds a struct for this call alone)
    if (rp->plane <= 0) return bad_in(fn, "planes mode only");
    if (!rgb || !planes) return bad_in(fn, "NULL argument");
    if (rgb_stride < 3 * (int64_t)rp->plane || planes_stride < rp->plane) return bad_in(fn, "a stride is smaller than what it strides over");
    if (rgb_stride % 16 != 0 || planes_stride % 16 != 0 || !aligned(rgb, 16) || !aligned(planes, 16))
        return bad_in(fn, "rgb, planes and their strides must be multiples of 16");
    tde::replay_pack_kernel<<<env_blocks(rp->B), 64 * tde::kRingWaves, 0, (hipStream_t)stream>>>(rp->B, rp->plane, rgb, rgb_stride, planes,
                                                                                                  planes_stride);
    return tde_host::launch_status(fn);
}
