// tde_replay.hip — the device-resident replay buffer of include/tde_replay.h: its kernels, its host-side checks and its four entry
// points (a translation unit of its own: no existing kernel includes it).
//   * tde_replay_begin / tde_replay_push: one wavefront per env copies the env's newest layer plane (or float32 row) into its slot of
//     the ring with 16-byte loads and stores; lane 0 writes the slot's scalars.  kReplayWaves envs per workgroup (a one-env workgroup
//     costs ~8 us per launch at 8192 envs with nothing to do, profiles/near_field_kernel_stats.txt).
//   * tde_replay_sample, planes mode: one workgroup per drawn transition, one wavefront per source slot s - n_stack + 1 .. s + 1.  A
//     wavefront reads its plane once (four 16-byte loads per lane at 64 x 64, in flight together: the last stage of the rasteriser)
//     and expands it through raster_expand into the frame of `obs` and / or of `next_obs` it belongs to - or writes zeros there.  Every
//     wavefront repeats the draw (ten Philox rounds on wave-uniform values) instead of waiting for one that did.
//   * tde_replay_sample, rows mode: one wavefront per transition copies its two rows.
//   * tde_replay_pack: colour observations back to layer planes, for buffers over an env without a layer ring.
// All offsets into frames / obs / next_obs are int64_t: C * B * plane passes 2^31 at the sizes the buffer is for.
// The specification is restated in numpy by tests/replay_ref.py.
#include "tde_raster.h"
#include "tde_host.h"
#include "../../include/tde_replay.h"

namespace tde {

constexpr int kReplayWaves = 4;         // envs (begin / push / pack) or transitions (rows gather) per workgroup
constexpr int kReplayEnded = 3 | TDE_REPLAY_CUT;

struct ReplayArgs {
    tde_replay rp;
    int64_t row;                        // bytes per frame / row of `frames`
    bool vec;                           // rows move as 16-byte words (planes mode always)
};

// `n` bytes from `src` to `dst` by one wavefront: 16-byte words when both are 16-byte aligned and n is a multiple of 16 (vec),
// 4-byte words otherwise (n is a multiple of 4)
TDE_DEV void replay_copy_row(uint8_t *dst, const uint8_t *src, int n, bool vec, int lane)
{
    if (vec) {
        for (int i = lane; i < n / 16; i += 64) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
    } else {
        for (int i = lane; i < n / 4; i += 64) reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(src)[i];
    }
}

__global__ __launch_bounds__(64 * kReplayWaves) void replay_begin_kernel(ReplayArgs a, int w, const uint8_t *src, int64_t src_stride,
                                                                         const uint8_t *mask)
{
    const int lane = (int)(threadIdx.x & 63u), e = (int)blockIdx.x * kReplayWaves + (int)(threadIdx.x >> 6);
    if (e >= a.rp.B) return;
    if (mask && !mask[e]) return;
    const int64_t at = (int64_t)w * a.rp.B + e;
    replay_copy_row(a.rp.frames + at * a.row, src + (int64_t)e * src_stride, (int)a.row, a.vec, lane);
    if (lane == 0) {
        a.rp.age[at] = 0;
        if (mask) {
            const int64_t prev = (int64_t)(w == 0 ? a.rp.C - 1 : w - 1) * a.rp.B + e;
            a.rp.done[prev] = (uint8_t)(a.rp.done[prev] | TDE_REPLAY_CUT);
        }
    }
}

__global__ __launch_bounds__(64 * kReplayWaves) void replay_push_kernel(ReplayArgs a, int w, const float *action, const float *reward,
                                                                        const uint8_t *done_bits, const uint8_t *src, int64_t src_stride)
{
    const int lane = (int)(threadIdx.x & 63u), e = (int)blockIdx.x * kReplayWaves + (int)(threadIdx.x >> 6);
    if (e >= a.rp.B) return;
    const int w1 = w + 1 == a.rp.C ? 0 : w + 1;
    const int64_t at = (int64_t)w * a.rp.B + e, at1 = (int64_t)w1 * a.rp.B + e;
    replay_copy_row(a.rp.frames + at1 * a.row, src + (int64_t)e * src_stride, (int)a.row, a.vec, lane);
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

__global__ __launch_bounds__(64 * kReplayWaves) void replay_pack_kernel(int B, int plane, const uint8_t *rgb, int64_t rgb_stride,
                                                                        uint8_t *planes, int64_t planes_stride)
{
    const int lane = (int)(threadIdx.x & 63u), e = (int)blockIdx.x * kReplayWaves + (int)(threadIdx.x >> 6);
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

// transition i of a sample (wave-uniform): the pair drawn or given, and whether it is a stored transition
// (tde_terminal.hip restates replay_pick, replay_scalars and the planes gather - terminal_pick, terminal_scalars,
//  terminal_gather_planes_kernel - because tde_terminal_sample must draw the pairs tde_replay_sample draws: a change to the draw, the
//  validity rule or the blanking rule here is made there too; tests/test_gpu_terminal.py holds the two draws to each other)
struct ReplayPick {
    int slot, env, off;                 // off: slots between `first` and `slot`
    bool ok;
};

struct SampleArgs {
    ReplayArgs a;
    int first, count;
    const int32_t *idx_in;
    uint64_t seed;
    uint32_t draw_lo, draw_hi;
    int32_t *idx;
    uint8_t *obs, *next_obs;
    float *action, *reward;
    uint8_t *done;
};

TDE_DEV ReplayPick replay_pick(const SampleArgs &s, int i)
{
    const int C = s.a.rp.C, B = s.a.rp.B;
    ReplayPick p;
    if (s.idx_in) {
        p.slot = s.idx_in[2 * (int64_t)i];
        p.env = s.idx_in[2 * (int64_t)i + 1];
        p.ok = p.slot >= 0 && p.slot < C && p.env >= 0 && p.env < B;
        p.off = p.ok ? (p.slot - s.first + C) % C : 0;
        p.ok = p.ok && p.off < s.count;
    } else {
        const int skip = s.a.rp.n_stack - 1;
        const uint4 wd = philox(s.seed, (uint32_t)i, s.draw_lo, s.draw_hi, TDE_REPLAY_TAG);
        p.off = skip + (int)__umulhi(wd.x, (uint32_t)(s.count - skip));
        p.slot = (s.first + p.off) % C;
        p.env = (int)__umulhi(wd.y, (uint32_t)B);
        p.ok = true;
    }
    return p;
}

// the scalars of transition i, by one lane
TDE_DEV void replay_scalars(const SampleArgs &s, int i, const ReplayPick &p)
{
    const int64_t at = (int64_t)p.slot * s.a.rp.B + p.env;
    s.idx[2 * (int64_t)i] = p.slot;
    s.idx[2 * (int64_t)i + 1] = p.env;
    reinterpret_cast<float2 *>(s.action)[i] = p.ok ? reinterpret_cast<const float2 *>(s.a.rp.action)[at] : make_float2(0.0f, 0.0f);
    s.reward[i] = p.ok ? s.a.rp.reward[at] : 0.0f;
    s.done[i] = p.ok ? s.a.rp.done[at] : (uint8_t)0;
}

// SIZE64: plane == 4096 (the reference's 64 x 64 observation: the four chunks of a lane in flight together)
template <bool SIZE64>
__global__ __launch_bounds__(64 * (TDE_REPLAY_MAX_STACK + 1)) void replay_gather_planes_kernel(SampleArgs s)
{
    const int lane = (int)(threadIdx.x & 63u), k = (int)(threadIdx.x >> 6), i = (int)blockIdx.x;
    const int C = s.a.rp.C, B = s.a.rp.B, ns = s.a.rp.n_stack, plane = SIZE64 ? 4096 : s.a.rp.plane;
    const ReplayPick p = replay_pick(s, i);
    if (k == 0 && lane == 0) replay_scalars(s, i, p);
    // this wavefront's source: slot s - (ns - 1) + k, i.e. frame k of obs (k < ns) and frame k - 1 of next_obs (k > 0)
    const int d_obs = ns - 1 - k, d_next = ns - k;       // its distance from slot s / from slot s + 1
    bool to_obs = false, to_next = false;
    int64_t src = 0;
    if (p.ok) {
        const int64_t at = (int64_t)p.slot * B + p.env;
        const int s1 = p.slot + 1 == C ? 0 : p.slot + 1;
        const int age = s.a.rp.age[at], age1 = s.a.rp.age[(int64_t)s1 * B + p.env];
        const bool ended = (s.a.rp.done[at] & kReplayEnded) != 0;
        // a frame is shown when it belongs to the episode (age) and has not been overwritten (it lies at or behind `first`)
        to_obs = k < ns && d_obs <= age && d_obs <= p.off;
        to_next = k > 0 && !ended && d_next <= age1 && d_next <= p.off + 1;
        const int ss = (p.slot - d_obs + C) % C;         // (d_obs >= -1 and C >= ns + 1 > d_obs)
        src = ((int64_t)ss * B + p.env) * plane;
    }
    const uint4 *from = reinterpret_cast<const uint4 *>(s.a.rp.frames + src);
    uint8_t *o = s.obs + ((int64_t)i * ns + k) * 3 * plane, *n = s.next_obs + ((int64_t)i * ns + (k > 0 ? k - 1 : 0)) * 3 * plane;
    const uint32_t bl = TDE_LAYER_BLANK * 0x01010101u;
    const uint4 blank = make_uint4(bl, bl, bl, bl);
    const bool rd = to_obs || to_next;
    if (SIZE64) {
        uint4 ch[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) ch[c] = rd ? from[lane + 64 * c] : blank;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (k < ns) raster_expand(to_obs ? ch[c] : blank, o, plane, lane + 64 * c);
            if (k > 0) raster_expand(to_next ? ch[c] : blank, n, plane, lane + 64 * c);
        }
    } else {
        for (int c = lane; c < plane / 16; c += 64) {
            const uint4 v = rd ? from[c] : blank;
            if (k < ns) raster_expand(to_obs ? v : blank, o, plane, c);
            if (k > 0) raster_expand(to_next ? v : blank, n, plane, c);
        }
    }
}

__global__ __launch_bounds__(64 * kReplayWaves) void replay_gather_rows_kernel(SampleArgs s, int N)
{
    const int lane = (int)(threadIdx.x & 63u), i = (int)blockIdx.x * kReplayWaves + (int)(threadIdx.x >> 6);
    if (i >= N) return;
    const int C = s.a.rp.C, B = s.a.rp.B, D = s.a.rp.D;
    const ReplayPick p = replay_pick(s, i);
    if (lane == 0) replay_scalars(s, i, p);
    bool next = false;
    int64_t at = 0, at1 = 0;
    if (p.ok) {
        at = (int64_t)p.slot * B + p.env;
        at1 = (int64_t)(p.slot + 1 == C ? 0 : p.slot + 1) * B + p.env;
        next = (s.a.rp.done[at] & kReplayEnded) == 0;
    }
    const float *rows = reinterpret_cast<const float *>(s.a.rp.frames);
    float *o = reinterpret_cast<float *>(s.obs) + (int64_t)i * D, *n = reinterpret_cast<float *>(s.next_obs) + (int64_t)i * D;
    for (int c = lane; c < D; c += 64) {
        o[c] = p.ok ? rows[at * D + c] : 0.0f;
        n[c] = next ? rows[at1 * D + c] : 0.0f;
    }
}

}  // namespace tde

namespace {

int bad_in(const char *fn, const char *msg)
{
    snprintf(tde_host::err_buf(), tde_host::kErrLen, "%s: %s", fn, msg);
    return (int)hipErrorInvalidValue;
}

bool aligned(const void *p, int64_t n) { return ((uintptr_t)p % (uintptr_t)n) == 0; }

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

// the source of a frame: one plane / row per env, src_stride bytes apart
int check_src(const char *fn, const tde::ReplayArgs &a, int32_t w, const uint8_t *src, int64_t src_stride)
{
    if (w < 0 || w >= a.rp.C) return bad_in(fn, "w must be in [0, C)");
    if (!src) return bad_in(fn, "src is NULL");
    if (src_stride < a.row) return bad_in(fn, "src_stride is smaller than a frame / row");
    const int64_t al = a.vec ? 16 : 4;
    if (src_stride % al != 0 || !aligned(src, al)) return bad_in(fn, "src and src_stride must be multiples of 16 (rows mode: 4)");
    return 0;
}

unsigned env_blocks(int B) { return (unsigned)((B + tde::kReplayWaves - 1) / tde::kReplayWaves); }

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
    if ((rc = check_src(fn, a, w, src, src_stride)) != 0) return rc;
    tde::replay_begin_kernel<<<env_blocks(rp->B), 64 * tde::kReplayWaves, 0, (hipStream_t)stream>>>(a, w, src, src_stride, mask);
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
    if ((rc = check_src(fn, a, w, src, src_stride)) != 0) return rc;
    tde::replay_push_kernel<<<env_blocks(rp->B), 64 * tde::kReplayWaves, 0, (hipStream_t)stream>>>(a, w, action, reward, done_bits, src,
                                                                                                   src_stride);
    return tde_host::launch_status(fn);
}

int tde_replay_sample(const tde_replay *rp, int32_t first, int32_t count, int32_t N, const int32_t *idx_in, uint64_t seed, uint64_t draw,
                      int32_t *idx, uint8_t *obs, uint8_t *next_obs, float *action, float *reward, uint8_t *done, void *stream)
{
    const char *fn = "tde_replay_sample";
    tde::SampleArgs s;
    int rc = check_replay(fn, rp, s.a);
    if (rc) return rc;
    if (N < 1) return bad_in(fn, "N must be >= 1");
    if (count < 1) return bad_in(fn, "count must be >= 1 (the buffer holds no transition)");
    if (count > rp->C - 1) return bad_in(fn, "count must be <= C - 1 (one slot is open)");
    if (first < 0 || first >= rp->C) return bad_in(fn, "first must be in [0, C)");
    if (!idx || !obs || !next_obs || !action || !reward || !done) return bad_in(fn, "a NULL output");
    if (!idx_in && count <= rp->n_stack - 1) return bad_in(fn, "count must be > n_stack - 1 to draw: no stored transition has its whole stack in the ring yet");
    const bool planes = rp->plane > 0;
    if (!aligned(obs, planes ? 16 : 4) || !aligned(next_obs, planes ? 16 : 4) || !aligned(action, 8) || !aligned(reward, 4) ||
        !aligned(idx, 4) || !aligned(idx_in, 4))
        return bad_in(fn, "obs / next_obs must be 16-byte aligned (rows mode: 4), action 8-byte, reward / idx 4-byte");
    s.first = first; s.count = count; s.idx_in = idx_in; s.seed = seed;
    s.draw_lo = (uint32_t)draw; s.draw_hi = (uint32_t)(draw >> 32);
    s.idx = idx; s.obs = obs; s.next_obs = next_obs; s.action = action; s.reward = reward; s.done = done;
    hipStream_t st = (hipStream_t)stream;
    if (planes) {
        const unsigned threads = 64u * (unsigned)(rp->n_stack + 1);
        if (rp->plane == 4096) tde::replay_gather_planes_kernel<true><<<(unsigned)N, threads, 0, st>>>(s);
        else tde::replay_gather_planes_kernel<false><<<(unsigned)N, threads, 0, st>>>(s);
    } else {
        tde::replay_gather_rows_kernel<<<env_blocks(N), 64 * tde::kReplayWaves, 0, st>>>(s, N);
    }
    return tde_host::launch_status(fn);
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
    tde::replay_pack_kernel<<<env_blocks(rp->B), 64 * tde::kReplayWaves, 0, (hipStream_t)stream>>>(rp->B, rp->plane, rgb, rgb_stride, planes,
                                                                                                  planes_stride);
    return tde_host::launch_status(fn);
}
