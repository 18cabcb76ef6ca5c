// tde_nstep.hip — n-step returns from the replay ring, include/tde_nstep.h: its kernels, its host-side checks and its entry point (a
// translation unit of its own: no existing kernel includes it, and it changes none - the ring is filled by tde_replay.hip, the pool by
// tde_terminal.hip).
//   * the pick of a sample, the look-ahead, its last step and what follows it, the frame rule, the expansion of a layer plane and the
//     pool row are tde_ring.h's (ring_pick, ring_ahead, ring_last, ring_shown, ring_expand, ring_pool_row): nothing of them is restated.
//   * the look-ahead is wave-uniform and every wavefront repeats it instead of waiting for one that made it.  Only the wavefront that writes the scalars reads the rewards - lane j that of slot s + j - and sums them in the
//     header's order with __fmul_rn / __fadd_rn, which the compiler may not fuse.
//   * planes mode: one workgroup per sample, one wavefront per WRITTEN frame - frames 0 .. n_stack - 1 of obs from the stack of slot s,
//     frames 0 .. n_stack - 1 of next_obs from the stack that follows slot L (or the terminal stack of L, or zeros).  A wavefront
//     reads its plane once (four 16-byte loads per lane at 64 x 64, in flight together) and expands it through ring_expand, or writes
//     zeros.  Every destination byte is written exactly once with raster_expand's streaming stores; nothing is pre-zeroed; no LDS.
//     Where the two stacks overlap (m < n_stack) a plane is read by two wavefronts of the workgroup, the second time from L2.
//   * rows mode: one wavefront per sample copies its two rows.
// All offsets into frames / pool / obs / next_obs are int64_t.  The specification is restated in numpy by tests/nstep_ref.py.
#include "tde_ring.h"
#include "../../include/tde_nstep.h"

namespace tde {

template <class Base>
struct NStepArgs : Base {               // SampleArgs / TerminalSampleArgs (kPool is theirs) and what the look-ahead adds
    int n_steps;
    float gamma;
    float *discount;
    uint8_t *steps;
};

// the scalars of sample i, by one whole wavefront: the reward sum in the header's order, then lane 0 writes
template <class Args>
TDE_DEV void nstep_scalars(const Args &s, int i, const RingPick &p, int m, int lane)
{
    const int C = s.rp.C, B = s.rp.B;
    float r = 0.0f;
    if (lane < m) r = s.rp.reward[(int64_t)ring_slot(p.slot, lane, C) * B + p.env];
    float R = __shfl(r, 0), g = p.ok ? s.gamma : 0.0f;
    for (int k = 1; k < m; ++k) {
        R = __fadd_rn(R, __fmul_rn(g, __shfl(r, k)));
        g = __fmul_rn(g, s.gamma);
    }
    if (lane != 0) return;
    s.idx[2 * (int64_t)i] = p.slot;
    s.idx[2 * (int64_t)i + 1] = p.env;
    uint32_t d = 0;
    float2 act = make_float2(0.0f, 0.0f);
    if (p.ok) {
        act = reinterpret_cast<const float2 *>(s.rp.action)[(int64_t)p.slot * B + p.env];
        const RingLast z = ring_last(s, p.slot, p.env, m);
        d = z.row >= 0 ? z.done_last | TDE_TERMINAL_HAS : z.done_last;
    }
    reinterpret_cast<float2 *>(s.action)[i] = act;
    s.reward[i] = R;
    s.discount[i] = g;
    s.steps[i] = (uint8_t)m;
    s.done[i] = (uint8_t)d;
}

// planes mode: one workgroup per sample; wavefront k < n_stack writes frame k of obs, wavefront n_stack + j frame j of next_obs
template <bool SIZE64, class Args>
__global__ __launch_bounds__(64 * 2 * TDE_REPLAY_MAX_STACK) void nstep_planes_kernel(Args s)
{
    const int lane = (int)(threadIdx.x & 63u), k = (int)(threadIdx.x >> 6), i = (int)blockIdx.x;
    const int C = s.rp.C, B = s.rp.B, ns = s.rp.n_stack, plane = SIZE64 ? 4096 : s.rp.plane;
    const RingPick p = ring_pick(s, i);
    const int m = ring_ahead<TDE_NSTEP_MAX / 64>(s, p, s.n_steps, lane);
    if (k == 0) nstep_scalars(s, i, p, m, lane);
    const bool to_next = k >= ns;
    const int j = to_next ? k - ns : k;
    bool show = false;
    const uint8_t *from = s.rp.frames;
    if (p.ok) {
        // the stack this frame belongs to: its newest slot and that slot's distance from `first`; the frame lies d slots behind it
        int newest = p.slot, off = p.off, d = ns - 1 - j, row = -1;
        bool live = true;
        if (to_next) {
            const int last = ring_slot(p.slot, m - 1, C);
            const RingLast z = ring_last(s, p.slot, p.env, m);
            row = z.row;
            if (row >= 0) {
                // the terminal stack: the stack of slot L one frame down (d = -1: the pool plane on top)
                newest = last, off = p.off + m - 1, d -= 1;
            } else {
                // the stack of slot L + 1, zeros after an end
                newest = ring_slot(last, 1, C), off = p.off + m, live = z.live;
            }
        }
        show = live && ring_shown(d, s.rp.age[(int64_t)newest * B + p.env], off);
        from += ((int64_t)ring_slot(newest, -d, C) * B + p.env) * plane;           // (-1 <= d <= ns - 1 < C)
        if constexpr (Args::kPool) {
            if (row >= 0 && d < 0) from = s.tm.pool + ((int64_t)newest * s.tm.M + row) * plane;
        }
    }
    const RingFrame mine = {(to_next ? s.next_obs : s.obs) + ((int64_t)i * ns + j) * 3 * plane, true, show}, none = {nullptr, false, false};
    ring_expand<SIZE64>(reinterpret_cast<const uint4 *>(from), plane, lane, mine, none);
}

// rows mode: one wavefront per sample copies the row of slot s and the row that follows slot L
template <class Args>
__global__ __launch_bounds__(64 * kRingWaves) void nstep_rows_kernel(Args s, int N)
{
    const int lane = (int)(threadIdx.x & 63u), i = (int)blockIdx.x * kRingWaves + (int)(threadIdx.x >> 6);
    if (i >= N) return;
    const int C = s.rp.C, B = s.rp.B, D = s.rp.D;
    const RingPick p = ring_pick(s, i);
    const int m = ring_ahead<TDE_NSTEP_MAX / 64>(s, p, s.n_steps, lane);
    nstep_scalars(s, i, p, m, lane);
    const float *rows = reinterpret_cast<const float *>(s.rp.frames), *from = rows;
    bool next = false;
    int64_t at = 0, at1 = 0;
    if (p.ok) {
        const int last = ring_slot(p.slot, m - 1, C);
        const RingLast z = ring_last(s, p.slot, p.env, m);
        at = (int64_t)p.slot * B + p.env;
        at1 = (int64_t)ring_slot(last, 1, C) * B + p.env;
        next = z.row >= 0 || z.live;
        if constexpr (Args::kPool) {
            if (z.row >= 0) from = reinterpret_cast<const float *>(s.tm.pool), at1 = (int64_t)last * s.tm.M + z.row;
        }
    }
    float *o = reinterpret_cast<float *>(s.obs) + (int64_t)i * D, *n = reinterpret_cast<float *>(s.next_obs) + (int64_t)i * D;
    for (int c = lane; c < D; c += 64) {
        o[c] = p.ok ? rows[at * D + c] : 0.0f;
        n[c] = next ? from[at1 * D + c] : 0.0f;
    }
}

}  // namespace tde

using namespace tde_host;

namespace {

template <class Args>
int launch_nstep(const char *fn, const Args &s, int32_t N, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (s.rp.plane > 0) {
        const unsigned threads = 64u * 2u * (unsigned)s.rp.n_stack;
        if (s.rp.plane == 4096) tde::nstep_planes_kernel<true><<<(unsigned)N, threads, 0, st>>>(s);
        else tde::nstep_planes_kernel<false><<<(unsigned)N, threads, 0, st>>>(s);
    } else {
        tde::nstep_rows_kernel<<<ring_blocks(N, tde::kRingWaves), 64 * tde::kRingWaves, 0, st>>>(s, N);
    }
    return launch_status(fn);
}

// what tde_nstep_sample takes beyond a sample's arguments; fills the look-ahead's part of the argument block
template <class Args>
int check_nstep(const char *fn, int32_t n_steps, float gamma, float *discount, uint8_t *steps, Args &s)
{
    if (n_steps < 1 || n_steps > TDE_NSTEP_MAX) return bad_in(fn, "n_steps must be in [1, 64]");
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return bad_in(fn, "gamma must be finite and in [0, 1]");
    if (!discount || !steps) return bad_in(fn, "a NULL output");
    if (!aligned(discount, 4)) return bad_in(fn, "discount must be 4-byte aligned");
    s.n_steps = n_steps; s.gamma = gamma; s.discount = discount; s.steps = steps;
    return 0;
}

}  // namespace

int tde_nstep_version(void) { return TDE_NSTEP_VERSION; }

int tde_nstep_sample(const tde_replay *rp, const tde_terminal *tm, int32_t first, int32_t count, int32_t N, const int32_t *idx_in,
                     uint64_t seed, uint64_t draw, int32_t n_steps, float gamma, int32_t *idx, uint8_t *obs, uint8_t *next_obs,
                     float *action, float *reward, uint8_t *done, float *discount, uint8_t *steps, void *stream)
{
    const char *fn = "tde_nstep_sample";
    return with_ring_args<tde::NStepArgs>(fn, rp, tm, [&](auto &s) {
        int rc = check_sample(fn, rp, first, count, N, idx_in, seed, draw, idx, obs, next_obs, action, reward, done, s);
        if (rc || (rc = check_nstep(fn, n_steps, gamma, discount, steps, s)) != 0) return rc;
        return launch_nstep(fn, s, N, stream);
    });
}
