// tde_ring.h — what the six units over the replay ring share: what a learner sees of a stored transition, stated once.
//   * device side: the "ended" mask, the ring's wrap, the row copy, the pick of a sample (the draw, and the validity rule of a given
//     pair), the frame rule, the expansion of a layer plane into frames of obs / next_obs, the scalars of a sampled transition, the
//     look-ahead from a pick to the first ending (ring_ahead) and the last step of a look-ahead with what follows it (ring_last);
//   * kernels: ring_gather_planes_kernel / ring_gather_rows_kernel<Args> - tde_replay_sample (Args = SampleArgs) and
//     tde_terminal_sample (Args = TerminalSampleArgs: the same with the terminal pool, which the first instantiation does not contain);
//   * host side: the argument checks that more than one entry point makes, and the choice of the argument block of an entry point
//     that takes the pool or not (with_ring_args).  Each message names its entry point (`fn`).
// What each unit takes:
//   tde_replay.hip     the wrap, the row copy, check_slot / check_src, check_sample, the two gather kernels (launch_sample), kRingWaves
//   tde_terminal.hip   the row copy, the same checks, and the gather kernels over TerminalSampleArgs
//   tde_onpolicy.hip   the wrap, the "ended" mask, the frame rule, the expansion of a plane (ring_expand), check_stored, kRingWaves
//   tde_priority.hip   the wrap, the stack rule (ring_whole), check_slot / check_stored, kRingWaves
//   tde_nstep.hip      the pick, ring_ahead<1>, ring_last, the frame rule, ring_expand, the pool row, check_sample, with_ring_args
//   tde_sequence.hip   the pick of a given pair, ring_ahead<4>, ring_last, the frame rule, the pool row, the row copy, check_sample
//                      without a next_obs, with_ring_args
#pragma once
#include "tde_raster.h"
#include "tde_host.h"
#include "../../include/tde_terminal.h"

namespace tde {

constexpr int kRingWaves = 4;           // envs (begin / push / pack) or samples (rows gathers) per workgroup
constexpr int kRingEnded = 3 | TDE_REPLAY_CUT;          // done bits after which the next slot starts another episode

// slot `s` moved by `d` in a ring of C slots (s in [0, C), |d| < C)
TDE_DEV int ring_slot(int s, int d, int C)
{
    const int t = s + d;
    return t < 0 ? t + C : (t >= C ? t - C : t);
}

// `n` bytes from `src` to `dst` by one wavefront: 16-byte words when both are 16-byte aligned and n is a multiple of 16 (vec),
// 4-byte words otherwise (n is a multiple of 4)
TDE_DEV void ring_copy_row(uint8_t *dst, const uint8_t *src, int n, bool vec, int lane)
{
    if (vec) {
        for (int i = lane; i < n / 16; i += 64) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
    } else {
        for (int i = lane; i < n / 4; i += 64) reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(src)[i];
    }
}

// sample i (wave-uniform): the pair drawn or given, and whether it is a stored transition
struct RingPick {
    int slot, env, off;                 // off: slots between `first` and `slot`
    bool ok;
};

struct SampleArgs {
    static constexpr bool kPool = false;
    tde_replay rp;
    int first, count;
    const int32_t *idx_in;
    uint64_t seed;
    uint32_t draw_lo, draw_hi;
    int32_t *idx;
    uint8_t *obs, *next_obs;
    float *action, *reward;
    uint8_t *done;
};

struct TerminalSampleArgs : SampleArgs {
    static constexpr bool kPool = true;
    tde_terminal tm;
};

TDE_DEV RingPick ring_pick(const SampleArgs &s, int i)
{
    const int C = s.rp.C, B = s.rp.B;
    RingPick p;
    if (s.idx_in) {
        p.slot = s.idx_in[2 * (int64_t)i];
        p.env = s.idx_in[2 * (int64_t)i + 1];
        p.ok = p.slot >= 0 && p.slot < C && p.env >= 0 && p.env < B;
        p.off = p.ok ? ring_slot(p.slot, -s.first, C) : 0;
        p.ok = p.ok && p.off < s.count;
    } else {
        const int skip = s.rp.n_stack - 1;
        const uint4 wd = philox(s.seed, (uint32_t)i, s.draw_lo, s.draw_hi, TDE_REPLAY_TAG);
        p.off = skip + (int)__umulhi(wd.x, (uint32_t)(s.count - skip));
        p.slot = ring_slot(s.first, p.off, C);
        p.env = (int)__umulhi(wd.y, (uint32_t)B);
        p.ok = true;
    }
    return p;
}

// the frame rule: the frame `d` slots behind a slot (of that age, `off` slots after `first`) is shown iff it belongs to the episode
// and has not been overwritten (it lies at or behind `first`)
TDE_DEV bool ring_shown(int d, int age, int off) { return d <= age && d <= off; }

// the stack rule: a stored slot of that age, `off` slots after `first`, still has every frame of its stack in the ring (ring_shown for
// each d < n_stack at once) - what makes a stored pair one of valid_pairs()
TDE_DEV bool ring_whole(int age, int n_stack, int off) { return min(age, n_stack - 1) <= off; }

// a frame of obs / next_obs as one wavefront sees it: whether it writes the frame at all, and the plane or zeros (show implies write)
struct RingFrame {
    uint8_t *at;
    bool write, show;
};

// one wavefront expands the layer plane at `from` into its frame of obs and / or of next_obs
// SIZE64: plane == 4096 (the reference's 64 x 64 observation: the four chunks of a lane in flight together)
template <bool SIZE64>
TDE_DEV void ring_expand(const uint4 *from, int plane, int lane, const RingFrame &o, const RingFrame &n)
{
    const uint32_t bl = TDE_LAYER_BLANK * 0x01010101u;
    const uint4 blank = make_uint4(bl, bl, bl, bl);
    // the plane is read if either frame shows it (if neither does, what stands for it is blank already); a frame is blanked on its own
    // only beside one that is shown
    const bool rd = o.show || n.show, o_blank = n.show && !o.show, n_blank = o.show && !n.show;
    if (SIZE64) {
        uint4 ch[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) ch[c] = rd ? from[lane + 64 * c] : blank;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (o.write) raster_expand(o_blank ? blank : ch[c], o.at, plane, lane + 64 * c);
            if (n.write) raster_expand(n_blank ? blank : ch[c], n.at, plane, lane + 64 * c);
        }
    } else {
        for (int c = lane; c < plane / 16; c += 64) {
            const uint4 v = rd ? from[c] : blank;
            if (o.write) raster_expand(o_blank ? blank : v, o.at, plane, c);
            if (n.write) raster_expand(n_blank ? blank : v, n.at, plane, c);
        }
    }
}

// the pool row of the stored transition at `at`, or -1: it ended its episode and its terminal frame was kept (never without a pool)
template <class Args>
TDE_DEV int ring_pool_row(const Args &s, int64_t at, uint32_t done)
{
    if constexpr (Args::kPool) {
        const int r = s.tm.ref[at];
        return (done & 3u) != 0 && r >= 0 && r < s.tm.M ? r : -1;
    } else {
        return -1;
    }
}

// m, the steps a look-ahead of up to `limit` stored steps takes from the pick `p` (wave-uniform, by all 64 lanes; 0 for a pair that is
// no stored transition): it stops at the first step that ended its episode or was cut, and at the newest stored step.  Lane j reads
// the done byte of step base + j, the ballot of the ended lanes lists the endings, its first set bit is m (a scalar find-first-one: no
// vector shift).  ROUNDS rounds of 64 steps cover `limit` (limit <= 64 * ROUNDS); with ROUNDS == 1 there is no loop.
template <int ROUNDS, class Args>
TDE_DEV int ring_ahead(const Args &s, const RingPick &p, int limit, int lane)
{
    if (!p.ok) return 0;
    const int a = min(limit, s.count - p.off);          // (1 <= a <= C - 1: slot s + k is a stored slot for k < a)
    // (a <= 64 * ROUNDS bounds the rounds at run time; with one round the bound is the constant 1, so that no loop is compiled)
    for (int base = 0; base < (ROUNDS == 1 ? 1 : a); base += 64) {
        const int k = base + lane;
        bool ended = false;
        if (k < a) ended = (s.rp.done[(int64_t)ring_slot(p.slot, k, s.rp.C) * s.rp.B + p.env] & kRingEnded) != 0;
        const unsigned long long ends = __ballot(ended);
        if (ends) return base + __ffsll((long long)ends);
    }
    return a;
}

// the last step L = slot + m - 1 of a look-ahead of m >= 1 steps, and what follows it: the next observation is the pool plane / row
// over L's stack moved one frame down (row >= 0), or the stack of slot L + 1 (live), or zeros after an ending.  (The one-step
// gathers below are this with m = 1; they keep their own lines - see ring_gather_planes_kernel.)
struct RingLast {
    int64_t at_last;                    // the stored transition at slot L
    uint32_t done_last;
    int row;                            // its pool row, or -1
    bool live;                          // L neither ended its episode nor was cut
};

template <class Args>
TDE_DEV RingLast ring_last(const Args &s, int slot, int env, int m)
{
    RingLast z;
    z.at_last = (int64_t)ring_slot(slot, m - 1, s.rp.C) * s.rp.B + env;
    z.done_last = s.rp.done[z.at_last];
    z.row = ring_pool_row(s, z.at_last, z.done_last);
    z.live = (z.done_last & kRingEnded) == 0;
    return z;
}

// the scalars of transition i, by one lane
template <class Args>
TDE_DEV void ring_scalars(const Args &s, int i, const RingPick &p)
{
    const int64_t at = (int64_t)p.slot * s.rp.B + p.env;
    s.idx[2 * (int64_t)i] = p.slot;
    s.idx[2 * (int64_t)i + 1] = p.env;
    reinterpret_cast<float2 *>(s.action)[i] = p.ok ? reinterpret_cast<const float2 *>(s.rp.action)[at] : make_float2(0.0f, 0.0f);
    s.reward[i] = p.ok ? s.rp.reward[at] : 0.0f;
    uint32_t d = 0;
    if (p.ok) {
        d = s.rp.done[at];
        if (ring_pool_row(s, at, d) >= 0) d |= TDE_TERMINAL_HAS;
    }
    s.done[i] = (uint8_t)d;
}

// planes mode: one workgroup per transition, one wavefront per source slot s - n_stack + 1 .. s + 1.  With a pool, where the transition
// ended its episode and its terminal frame was kept, the wavefront of slot s + 1 reads the pool plane and the older slots go to next_obs
// one frame down as well.
template <bool SIZE64, class Args>
__global__ __launch_bounds__(64 * (TDE_REPLAY_MAX_STACK + 1)) void ring_gather_planes_kernel(Args s)
{
    const int lane = (int)(threadIdx.x & 63u), k = (int)(threadIdx.x >> 6), i = (int)blockIdx.x;
    const int C = s.rp.C, B = s.rp.B, ns = s.rp.n_stack, plane = SIZE64 ? 4096 : s.rp.plane;
    const RingPick p = ring_pick(s, i);
    if (k == 0 && lane == 0) ring_scalars(s, i, p);
    // this wavefront's source: slot s - (ns - 1) + k, i.e. frame k of obs (k < ns) and frame k - 1 of next_obs (k > 0)
    const int d_obs = ns - 1 - k, d_next = ns - k;       // its distance from slot s / from slot s + 1
    bool to_obs = false, to_next = false;
    const uint8_t *from = s.rp.frames;
    if (p.ok) {
        const int64_t at = (int64_t)p.slot * B + p.env;
        // (ring_last's rule at m = 1 in this kernel's own lines: through ring_last the general form takes 34 VGPRs, not 32)
        const int age = s.rp.age[at], age1 = s.rp.age[(int64_t)ring_slot(p.slot, 1, C) * B + p.env];
        const uint32_t done = s.rp.done[at];
        const bool ended = (done & kRingEnded) != 0;     // (its own statement: folded into to_next the 64 x 64 form takes 34 VGPRs, not 32)
        const int row = ring_pool_row(s, at, done);
        to_obs = k < ns && ring_shown(d_obs, age, p.off);
        // the terminal stack: obs moved one frame down, the pool plane on top; otherwise the stack of slot s + 1, zeros after an end
        to_next = row >= 0 ? k == ns || (k > 0 && to_obs) : k > 0 && !ended && ring_shown(d_next, age1, p.off + 1);
        from += ((int64_t)ring_slot(p.slot, -d_obs, C) * B + p.env) * plane;      // (d_obs >= -1 and C >= ns + 1 > d_obs)
        if constexpr (Args::kPool) {
            if (row >= 0 && k == ns) from = s.tm.pool + ((int64_t)p.slot * s.tm.M + row) * plane;
        }
    }
    const RingFrame o = {s.obs + ((int64_t)i * ns + k) * 3 * plane, k < ns, to_obs};
    const RingFrame n = {s.next_obs + ((int64_t)i * ns + (k > 0 ? k - 1 : 0)) * 3 * plane, k > 0, to_next};
    ring_expand<SIZE64>(reinterpret_cast<const uint4 *>(from), plane, lane, o, n);
}

// rows mode: one wavefront per transition copies its two rows
template <class Args>
__global__ __launch_bounds__(64 * kRingWaves) void ring_gather_rows_kernel(Args s, int N)
{
    const int lane = (int)(threadIdx.x & 63u), i = (int)blockIdx.x * kRingWaves + (int)(threadIdx.x >> 6);
    if (i >= N) return;
    const int C = s.rp.C, B = s.rp.B, D = s.rp.D;
    const RingPick p = ring_pick(s, i);
    if (lane == 0) ring_scalars(s, i, p);
    // the two rows: offsets into `frames`, or the successor in the pool
    const float *rows = reinterpret_cast<const float *>(s.rp.frames), *from = rows;
    bool next = false;
    int64_t at = 0, at1 = 0;
    if (p.ok) {
        at = (int64_t)p.slot * B + p.env;
        at1 = (int64_t)ring_slot(p.slot, 1, C) * B + p.env;
        const uint32_t done = s.rp.done[at];            // (ring_last's rule at m = 1 in its own lines: through ring_last, 9 more instructions)
        const int r = ring_pool_row(s, at, done);
        next = r >= 0 || (done & kRingEnded) == 0;
        if constexpr (Args::kPool) {
            if (r >= 0) from = reinterpret_cast<const float *>(s.tm.pool), at1 = (int64_t)p.slot * s.tm.M + r;
        }
    }
    float *o = reinterpret_cast<float *>(s.obs) + (int64_t)i * D, *n = reinterpret_cast<float *>(s.next_obs) + (int64_t)i * D;
    for (int c = lane; c < D; c += 64) {
        o[c] = p.ok ? rows[at * D + c] : 0.0f;
        n[c] = next ? from[at1 * D + c] : 0.0f;
    }
}

}  // namespace tde

namespace tde_host {

inline bool aligned(const void *p, int64_t n) { return ((uintptr_t)p % (uintptr_t)n) == 0; }

inline unsigned ring_blocks(int n, int per) { return (unsigned)((n + per - 1) / per); }

// the slot an entry point writes
inline int check_slot(const char *fn, const tde_replay *rp, int32_t w) { return w < 0 || w >= rp->C ? bad_in(fn, "w must be in [0, C)") : 0; }

// the source of a frame: one plane / row of `row` bytes per env, `stride` bytes apart; the message speaks of `src` and `stride` by the
// entry point's own names
inline int check_src(const char *fn, int64_t row, bool vec, const uint8_t *src, int64_t stride, const char *src_name, const char *stride_name)
{
    char msg[96];
    const int64_t al = vec ? 16 : 4;
    if (!src) snprintf(msg, sizeof(msg), "%s is NULL", src_name);
    else if (stride < row) snprintf(msg, sizeof(msg), "%s is smaller than a frame / row", stride_name);
    else if (stride % al != 0 || !aligned(src, al)) snprintf(msg, sizeof(msg), "%s and %s must be multiples of 16 (rows mode: 4)", src_name, stride_name);
    else return 0;
    return bad_in(fn, msg);
}

// the stored slots: `count` of them from `first`
inline int check_stored(const char *fn, const tde_replay *rp, int32_t first, int32_t count)
{
    if (count > rp->C - 1) return bad_in(fn, "count must be <= C - 1 (one slot is open)");
    if (first < 0 || first >= rp->C) return bad_in(fn, "first must be in [0, C)");
    return 0;
}

// what the samplers take after their structs (checked by the caller); fills the launch's argument block.  want_next: the sampler has a
// next_obs (tde_sequence_sample has none and passes NULL)
inline int check_sample(const char *fn, const tde_replay *rp, int32_t first, int32_t count, int32_t N, const int32_t *idx_in, uint64_t seed,
                        uint64_t draw, int32_t *idx, uint8_t *obs, uint8_t *next_obs, float *action, float *reward, uint8_t *done,
                        tde::SampleArgs &s, bool want_next = true)
{
    if (N < 1) return bad_in(fn, "N must be >= 1");
    if (count < 1) return bad_in(fn, "count must be >= 1 (the buffer holds no transition)");
    const int rc = check_stored(fn, rp, first, count);
    if (rc) return rc;
    if (!idx || !obs || (want_next && !next_obs) || !action || !reward || !done) return bad_in(fn, "a NULL output");
    if (!idx_in && count <= rp->n_stack - 1) return bad_in(fn, "count must be > n_stack - 1 to draw: no stored transition has its whole stack in the ring yet");
    const int64_t al = rp->plane > 0 ? 16 : 4;
    if (!aligned(obs, al) || !aligned(next_obs, al) || !aligned(action, 8) || !aligned(reward, 4) || !aligned(idx, 4) || !aligned(idx_in, 4))
        return bad_in(fn, "obs / next_obs must be 16-byte aligned (rows mode: 4), action 8-byte, reward / idx 4-byte");
    s.rp = *rp;
    s.first = first; s.count = count; s.idx_in = idx_in; s.seed = seed;
    s.draw_lo = (uint32_t)draw; s.draw_hi = (uint32_t)(draw >> 32);
    s.idx = idx; s.obs = obs; s.next_obs = next_obs; s.action = action; s.reward = reward; s.done = done;
    return 0;
}

// an entry point that takes the ring and, or not (tm NULL), the terminal pool beside it: checks the struct(s), makes the argument block
// Block<SampleArgs> or Block<TerminalSampleArgs> with *tm in it, and runs `body` - the entry point's own checks and its launch - on it
template <template <class> class Block, class Body>
int with_ring_args(const char *fn, const tde_replay *rp, const tde_terminal *tm, Body body)
{
    if (tm) {
        Block<tde::TerminalSampleArgs> s;
        const int rc = check_terminal_struct(fn, rp, tm);
        if (rc) return rc;
        s.tm = *tm;
        return body(s);
    }
    Block<tde::SampleArgs> s;
    const int rc = check_replay_struct(fn, rp);
    return rc ? rc : body(s);
}

// the launch of either sampler's gather
template <class Args>
int launch_sample(const char *fn, const Args &s, int32_t N, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (s.rp.plane > 0) {
        const unsigned threads = 64u * (unsigned)(s.rp.n_stack + 1);
        if (s.rp.plane == 4096) tde::ring_gather_planes_kernel<true><<<(unsigned)N, threads, 0, st>>>(s);
        else tde::ring_gather_planes_kernel<false><<<(unsigned)N, threads, 0, st>>>(s);
    } else {
        tde::ring_gather_rows_kernel<<<ring_blocks(N, tde::kRingWaves), 64 * tde::kRingWaves, 0, st>>>(s, N);
    }
    return launch_status(fn);
}

}  // namespace tde_host
