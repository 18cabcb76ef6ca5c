// tde_sequence.hip — windows of consecutive steps from the replay ring, include/tde_sequence.h: its kernels, its host-side checks and
// its entry point (a translation unit of its own: no existing kernel includes it, and it changes none - the ring is filled by
// tde_replay.hip, the pool by tde_terminal.hip).
//   * the ring's wrap, the pick of a given pair, the look-ahead, its last step and what follows it, the frame rule, the pool row and
//     the palette are tde_ring.h's (ring_slot, ring_pick, ring_ahead, ring_last, ring_shown, ring_pool_row, raster_expand): nothing of
//     them is restated here.  The draw takes ring_pick's Philox words over a span that keeps a whole window inside the stored range.
//   * two launches on the caller's stream.  sequence_scalars_kernel, one wavefront per window, finds the window's length m (ring_ahead,
//     64 steps per round) and writes idx, length and the T actions, rewards and done bytes.  The
//     gather that follows reads (idx, length) back: a window has up to T + n_stack = 264 gathering wavefronts, and one 12-byte load
//     each replaces a Philox draw and up to four rounds of the length search per wavefront.
//   * planes mode: output entry k, frame f (oldest first) shows source slot s + q, q = k - (n_stack - 1 - f) - entry m under a pool
//     row included: the terminal stack is entry m - 1 moved one frame down, which is the same q.  So every output frame has exactly
//     one of the T + n_stack source planes q = -(n_stack - 1) .. T, and one wavefront owns a source plane: it reads the plane once
//     (four 16-byte loads per lane at 64 x 64, in flight together) and expands it through the palette into each of its up to n_stack
//     destinations; a destination that does not show it (another episode, before `first`, k > m, after an ending) gets zeros.  Every
//     destination byte is written exactly once with raster_expand's streaming stores; nothing is pre-zeroed; no LDS, no barrier.
//   * rows mode: one wavefront per window and range of kSeqRowsPerWave entries copies their rows, or writes zeros.
// All offsets into frames / pool / obs are int64_t.  The specification is restated in numpy by tests/sequence_ref.py.
#include "tde_ring.h"
#include "../../include/tde_sequence.h"

namespace tde {

constexpr int kSeqRowsPerWave = 8;      // rows mode: entries of a window per wavefront

template <class Base>
struct SequenceArgs : Base {            // SampleArgs / TerminalSampleArgs (kPool is theirs; next_obs is unused) and what a window adds
    int T;
    int32_t *length;
    bool vec;                           // rows mode: rows move as 16-byte words
};

// window i (wave-uniform): ring_pick's pair for a given one; for a drawn one ring_pick's words over the offsets that leave room for T steps
template <class Args>
TDE_DEV RingPick sequence_pick(const Args &s, int i)
{
    if (s.idx_in) return ring_pick(s, i);
    const int skip = s.rp.n_stack - 1;
    const uint4 wd = philox(s.seed, (uint32_t)i, s.draw_lo, s.draw_hi, TDE_REPLAY_TAG);
    RingPick p;
    p.off = skip + (int)__umulhi(wd.x, (uint32_t)max(1, s.count - skip - (s.T - 1)));
    p.slot = ring_slot(s.first, p.off, s.rp.C);
    p.env = (int)__umulhi(wd.y, (uint32_t)s.rp.B);
    p.ok = true;
    return p;
}

// one wavefront per window: its length, its indices and its T actions, rewards and done bytes
template <class Args>
__global__ __launch_bounds__(64 * kRingWaves) void sequence_scalars_kernel(Args s, int N)
{
    const int lane = (int)(threadIdx.x & 63u), i = (int)blockIdx.x * kRingWaves + (int)(threadIdx.x >> 6);
    if (i >= N) return;
    const int C = s.rp.C, B = s.rp.B, T = s.T;
    const RingPick p = sequence_pick(s, i);
    const int m = ring_ahead<TDE_SEQUENCE_MAX / 64>(s, p, s.T, lane);
    if (lane == 0) {
        s.idx[2 * (int64_t)i] = p.slot;
        s.idx[2 * (int64_t)i + 1] = p.env;
        s.length[i] = m;
    }
    for (int k = lane; k < T; k += 64) {
        float2 act = make_float2(0.0f, 0.0f);
        float r = 0.0f;
        uint32_t d = 0;
        if (k < m) {
            const int64_t at = (int64_t)ring_slot(p.slot, k, C) * B + p.env;
            act = reinterpret_cast<const float2 *>(s.rp.action)[at];
            r = s.rp.reward[at];
            d = s.rp.done[at];
            if (ring_pool_row(s, at, d) >= 0) d |= TDE_TERMINAL_HAS;
        }
        const int64_t to = (int64_t)i * T + k;
        reinterpret_cast<float2 *>(s.action)[to] = act;
        s.reward[to] = r;
        s.done[to] = (uint8_t)d;
    }
}

// what the gathers know of window i (wave-uniform): the pair and length the scalars kernel wrote, and the window's last step
struct SequenceWindow : RingLast {
    int slot, env, off, m;              // m == 0: the pair is no stored transition (slot and env are then only echoes)
};

template <class Args>
TDE_DEV SequenceWindow sequence_window(const Args &s, int i)
{
    SequenceWindow w;
    w.m = s.length[i];
    w.slot = s.idx[2 * (int64_t)i];
    w.env = s.idx[2 * (int64_t)i + 1];
    w.off = 0, w.at_last = 0, w.done_last = 0, w.row = -1, w.live = false;
    if (w.m > 0) {
        w.off = ring_slot(w.slot, -s.first, s.rp.C);
        static_cast<RingLast &>(w) = ring_last(s, w.slot, w.env, w.m);
    }
    return w;
}

// planes mode: blockIdx.x = the window, wavefront j = blockIdx.y * kRingWaves + (its index in the workgroup) owns source plane
// q = j - (n_stack - 1), the layer plane of slot s + q (the pool plane for q == m under a pool row).  Its destination l < n_stack is
// frame n_stack - 1 - l of entry q + l: the frame l slots behind that entry's newest one.
template <bool SIZE64, class Args>
__global__ __launch_bounds__(64 * kRingWaves) void sequence_planes_kernel(Args s)
{
    const int lane = (int)(threadIdx.x & 63u), i = (int)blockIdx.x;
    const int C = s.rp.C, B = s.rp.B, ns = s.rp.n_stack, T = s.T, plane = SIZE64 ? 4096 : s.rp.plane;
    const int j = (int)blockIdx.y * kRingWaves + (int)(threadIdx.x >> 6);
    if (j >= T + ns) return;
    const int q = j - (ns - 1);
    const SequenceWindow w = sequence_window(s, i);
    // lane l decides whether destination l shows the plane
    bool show = false;
    const int k = q + lane;
    if (lane < ns && k >= 0 && k <= w.m && w.m > 0) {
        if (k < w.m) {
            // obs of the pair (s + k, e)
            show = ring_shown(lane, s.rp.age[(int64_t)ring_slot(w.slot, k, C) * B + w.env], w.off + k);
        } else if (w.row >= 0) {
            // the terminal stack of L: the pool plane on top, the stack of L one frame down
            show = lane == 0 || ring_shown(lane - 1, s.rp.age[w.at_last], w.off + w.m - 1);
        } else {
            // the stack of slot L + 1, zeros after an end (w.live in its own words: read from the window it takes 4 more SGPRs without a pool)
            show = (w.done_last & kRingEnded) == 0 && ring_shown(lane, s.rp.age[(int64_t)ring_slot(w.slot, w.m, C) * B + w.env], w.off + w.m);
        }
    }
    const uint32_t shown = mask_lo(__ballot(show));                    // (n_stack <= 8 bits)
    const uint8_t *from = s.rp.frames;
    if (shown) {                                                        // (then -(n_stack - 1) <= q <= m <= C - 1)
        from += ((int64_t)ring_slot(w.slot, q, C) * B + w.env) * plane;
        if constexpr (Args::kPool) {
            if (w.row >= 0 && q == w.m) from = s.tm.pool + ((w.at_last / B) * s.tm.M + w.row) * plane;
        }
    }
    const uint4 *src = reinterpret_cast<const uint4 *>(from);
    const uint32_t bl = TDE_LAYER_BLANK * 0x01010101u;
    const uint4 blank = make_uint4(bl, bl, bl, bl);
    const int l0 = max(0, -q), l1 = min(ns - 1, T - q);                // destinations with 0 <= q + l <= T
    uint8_t *to = s.obs + (((int64_t)i * (T + 1) + q + l0) * ns + (ns - 1 - l0)) * 3 * plane;
    const int64_t step = (int64_t)(ns - 1) * 3 * plane;                // entry + 1, frame - 1
    if (SIZE64) {
        uint4 ch[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) ch[c] = shown ? src[lane + 64 * c] : blank;
        for (int l = l0; l <= l1; ++l, to += step) {
            const bool on = mask_bit(shown, l) != 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) raster_expand(on ? ch[c] : blank, to, plane, lane + 64 * c);
        }
    } else {
        for (int c = lane; c < plane / 16; c += 64) {
            const uint4 v = shown ? src[c] : blank;
            uint8_t *t = to;
            for (int l = l0; l <= l1; ++l, t += step) raster_expand(mask_bit(shown, l) ? v : blank, t, plane, c);
        }
    }
}

// rows mode: blockIdx.x = the window; a wavefront copies the rows of kSeqRowsPerWave consecutive entries
template <class Args>
__global__ __launch_bounds__(64 * kRingWaves) void sequence_rows_kernel(Args s)
{
    const int lane = (int)(threadIdx.x & 63u), i = (int)blockIdx.x;
    const int C = s.rp.C, B = s.rp.B, D = s.rp.D, T = s.T;
    const int k0 = ((int)blockIdx.y * kRingWaves + (int)(threadIdx.x >> 6)) * kSeqRowsPerWave;
    if (k0 > T) return;
    const SequenceWindow w = sequence_window(s, i);
    for (int k = k0; k < min(k0 + kSeqRowsPerWave, T + 1); ++k) {
        const uint8_t *from = nullptr;
        if (k < w.m) {
            from = s.rp.frames + ((int64_t)ring_slot(w.slot, k, C) * B + w.env) * D * 4;
        } else if (k == w.m && w.m > 0) {
            if (w.row >= 0) {
                if constexpr (Args::kPool) from = s.tm.pool + ((w.at_last / B) * s.tm.M + w.row) * D * 4;
            } else if (w.live) {
                from = s.rp.frames + ((int64_t)ring_slot(w.slot, k, C) * B + w.env) * D * 4;
            }
        }
        uint8_t *to = s.obs + ((int64_t)i * (T + 1) + k) * D * 4;
        if (from) {
            ring_copy_row(to, from, 4 * D, s.vec, lane);
        } else if (s.vec) {
            for (int c = lane; c < D / 4; c += 64) reinterpret_cast<uint4 *>(to)[c] = make_uint4(0u, 0u, 0u, 0u);
        } else {
            for (int c = lane; c < D; c += 64) reinterpret_cast<uint32_t *>(to)[c] = 0u;
        }
    }
}

}  // namespace tde

using namespace tde_host;

namespace {

template <class Args>
int launch_sequence(const char *fn, const Args &s, int32_t N, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    tde::sequence_scalars_kernel<<<ring_blocks(N, tde::kRingWaves), 64 * tde::kRingWaves, 0, st>>>(s, N);
    const int rc = launch_status(fn);
    if (rc) return rc;
    if (s.rp.plane > 0) {
        const dim3 grid((unsigned)N, ring_blocks(s.T + s.rp.n_stack, tde::kRingWaves));
        if (s.rp.plane == 4096) tde::sequence_planes_kernel<true><<<grid, 64 * tde::kRingWaves, 0, st>>>(s);
        else tde::sequence_planes_kernel<false><<<grid, 64 * tde::kRingWaves, 0, st>>>(s);
    } else {
        const dim3 grid((unsigned)N, ring_blocks(s.T + 1, tde::kRingWaves * tde::kSeqRowsPerWave));
        tde::sequence_rows_kernel<<<grid, 64 * tde::kRingWaves, 0, st>>>(s);
    }
    return launch_status(fn);
}

// what tde_sequence_sample takes after its structs (checked by the caller); fills the launch's argument block
template <class Args>
int check_sequence(const char *fn, const tde_replay *rp, int32_t first, int32_t count, int32_t N, const int32_t *idx_in, uint64_t seed,
                   uint64_t draw, int32_t T, int32_t *idx, uint8_t *obs, float *action, float *reward, uint8_t *done, int32_t *length,
                   Args &s)
{
    if (T < 1 || T > TDE_SEQUENCE_MAX) return bad_in(fn, "T must be in [1, 256]");
    const int rc = check_sample(fn, rp, first, count, N, idx_in, seed, draw, idx, obs, nullptr, action, reward, done, s, false);
    if (rc) return rc;
    if (!length) return bad_in(fn, "a NULL output");
    if (!aligned(length, 4)) return bad_in(fn, "length must be 4-byte aligned");
    s.T = T; s.length = length;
    s.vec = rp->plane == 0 && rp->D % 4 == 0 && aligned(obs, 16) && aligned(rp->frames, 16);
    if constexpr (Args::kPool) s.vec = s.vec && aligned(s.tm.pool, 16);      // (s.tm is set already: with_ring_args copies *tm in before it runs the body)
    return 0;
}

}  // namespace

int tde_sequence_version(void) { return TDE_SEQUENCE_VERSION; }

int tde_sequence_sample(const tde_replay *rp, const tde_terminal *tm, int32_t first, int32_t count, int32_t N, const int32_t *idx_in,
                        uint64_t seed, uint64_t draw, int32_t T, int32_t *idx, uint8_t *obs, float *action, float *reward, uint8_t *done,
                        int32_t *length, void *stream)
{
    const char *fn = "tde_sequence_sample";
    return with_ring_args<tde::SequenceArgs>(fn, rp, tm, [&](auto &s) {
        const int rc = check_sequence(fn, rp, first, count, N, idx_in, seed, draw, T, idx, obs, action, reward, done, length, s);
        return rc ? rc : launch_sequence(fn, s, N, stream);
    });
}
