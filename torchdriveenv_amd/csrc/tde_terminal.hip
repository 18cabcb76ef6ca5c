// tde_terminal.hip — terminal observations beside the replay ring, include/tde_terminal.h: its kernels, its host-side checks and its
// entry points (a translation unit of its own: no existing kernel includes it, and it changes none - the ring is filled by
// tde_replay.hip).
//   * tde_terminal_stash / tde_terminal_push: ~1 % of the envs finish at a step, so the launch is sized for FINDING them: one lane per
//     env reads its done byte, the wavefront's ballot is the list of its finished envs, and the wavefront then copies each of them with
//     all 64 lanes, 16 bytes per lane (kTermEnvs envs per workgroup: 32 workgroups at 8192 envs instead of the 2048 of a wavefront
//     per env that mostly returns at once).
//   * the rank of tde_terminal_push is a scan in env order, without an atomic counter: a workgroup counts the finished envs before its
//     first (ballot + popcount over the done bytes in front of it, a quarter per wavefront: at most B bytes, read from L2), the
//     wavefronts exchange their counts through LDS, and a lane's rank is that base plus the set bits below its own (v_mbcnt).
//   * tde_terminal_sample, planes mode: replay_gather_planes_kernel's shape - one workgroup per transition, one wavefront per source
//     slot s - n_stack + 1 .. s + 1 - where the wavefront of slot s + 1, which writes zeros for an ended transition, reads the pool
//     plane instead, and the wavefronts of the older slots write their plane to next_obs one frame down as well.  The same bytes are
//     written; at most one more plane is read per ended sample.
//   * tde_terminal_sample, rows mode: one wavefront per transition copies its two rows.
// All offsets into frames / pool / obs / next_obs are int64_t.  The specification is restated in numpy by tests/terminal_ref.py.
#include "tde_raster.h"
#include "tde_host.h"
#include "../../include/tde_terminal.h"

namespace tde {

constexpr int kTermEnvs = 256;          // envs per workgroup of stash / push: one lane each, four wavefronts
constexpr int kTermWaves = 4;           // transitions per workgroup of the rows gather
constexpr int kTermEnded = 3 | TDE_REPLAY_CUT;

// `n` bytes from `src` to `dst` by one wavefront: 16-byte words (vec: both 16-byte aligned, n a multiple of 16) or 4-byte words
TDE_DEV void terminal_copy_row(uint8_t *dst, const uint8_t *src, int n, bool vec, int lane)
{
    if (vec) {
        for (int i = lane; i < n / 16; i += 64) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(src)[i];
    } else {
        for (int i = lane; i < n / 4; i += 64) reinterpret_cast<uint32_t *>(dst)[i] = reinterpret_cast<const uint32_t *>(src)[i];
    }
}

__global__ __launch_bounds__(kTermEnvs) void terminal_stash_kernel(int B, int row, bool vec, const uint8_t *__restrict__ done_bits,
                                                                   const uint8_t *__restrict__ src, int64_t src_stride,
                                                                   uint8_t *__restrict__ dst)
{
    const int lane = (int)(threadIdx.x & 63u), e = (int)blockIdx.x * kTermEnvs + (int)threadIdx.x;
    const bool fin = e < B && (done_bits[e] & 3) != 0;
    unsigned long long m = __ballot(fin);               // (wave-uniform: the loop below is scalar)
    const int e0 = e - lane;
    while (m) {
        const int ee = e0 + __ffsll((long long)m) - 1;
        m &= m - 1;
        terminal_copy_row(dst + (int64_t)ee * row, src + (int64_t)ee * src_stride, row, vec, lane);
    }
}

struct TerminalArgs {
    tde_replay rp;
    tde_terminal tm;
    int64_t row;                        // bytes per frame / row of `frames` and of `pool`
    bool vec;                           // rows move as 16-byte words (planes mode always)
};

__global__ __launch_bounds__(kTermEnvs) void terminal_push_kernel(TerminalArgs a, int w, const uint8_t *__restrict__ done_bits,
                                                                  const uint8_t *__restrict__ src, int64_t src_stride)
{
    __shared__ int before[kTermEnvs / 64], own[kTermEnvs / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int B = a.rp.B, M = a.tm.M, e0 = (int)blockIdx.x * kTermEnvs, e = e0 + tid;
    // finished envs in front of this workgroup (e0 is a multiple of kTermEnvs: every chunk is whole and inside [0, B))
    int cnt = 0;
    for (int j0 = 0; j0 < e0; j0 += kTermEnvs) cnt += __popcll(__ballot((done_bits[j0 + tid] & 3) != 0));
    const bool fin = e < B && (done_bits[e] & 3) != 0;
    unsigned long long m = __ballot(fin);
    if (lane == 0) {
        before[wv] = cnt;
        own[wv] = __popcll(m);
    }
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int k = 0; k < kTermEnvs / 64; ++k) base += before[k] + (k < wv ? own[k] : 0);
    const int rank = base + lane_prefix(m);
    if (e < B) a.tm.ref[(int64_t)w * B + e] = fin && rank < M ? rank : -1;
    // the wavefront's finished envs in env order, rows base, base + 1, ...: the first M of the batch are kept
    int r = base;
    while (m && r < M) {
        const int ee = e0 + 64 * wv + __ffsll((long long)m) - 1;
        m &= m - 1;
        terminal_copy_row(a.tm.pool + ((int64_t)w * M + r) * a.row, src + (int64_t)ee * src_stride, (int)a.row, a.vec, lane);
        ++r;
    }
}

// transition i of a sample (wave-uniform): tde_replay_sample's pick, restated - the same draw, the same validity rule
struct TerminalPick {
    int slot, env, off;                 // off: slots between `first` and `slot`
    bool ok;
};

struct TerminalSampleArgs {
    TerminalArgs a;
    int first, count;
    const int32_t *idx_in;
    uint64_t seed;
    uint32_t draw_lo, draw_hi;
    int32_t *idx;
    uint8_t *obs, *next_obs;
    float *action, *reward;
    uint8_t *done;
};

TDE_DEV TerminalPick terminal_pick(const TerminalSampleArgs &s, int i)
{
    const int C = s.a.rp.C, B = s.a.rp.B;
    TerminalPick p;
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

// the pool row of a stored transition, or -1: it ended its episode and its terminal frame was kept
TDE_DEV int terminal_row(const TerminalSampleArgs &s, int64_t at, uint32_t done)
{
    const int r = s.a.tm.ref[at];
    return (done & 3u) != 0 && r >= 0 && r < s.a.tm.M ? r : -1;
}

// the scalars of transition i, by one lane
TDE_DEV void terminal_scalars(const TerminalSampleArgs &s, int i, const TerminalPick &p)
{
    const int64_t at = (int64_t)p.slot * s.a.rp.B + p.env;
    s.idx[2 * (int64_t)i] = p.slot;
    s.idx[2 * (int64_t)i + 1] = p.env;
    reinterpret_cast<float2 *>(s.action)[i] = p.ok ? reinterpret_cast<const float2 *>(s.a.rp.action)[at] : make_float2(0.0f, 0.0f);
    s.reward[i] = p.ok ? s.a.rp.reward[at] : 0.0f;
    uint32_t d = 0;
    if (p.ok) {
        d = s.a.rp.done[at];
        if (terminal_row(s, at, d) >= 0) d |= TDE_TERMINAL_HAS;
    }
    s.done[i] = (uint8_t)d;
}

// SIZE64: plane == 4096 (the reference's 64 x 64 observation: the four chunks of a lane in flight together)
template <bool SIZE64>
__global__ __launch_bounds__(64 * (TDE_REPLAY_MAX_STACK + 1)) void terminal_gather_planes_kernel(TerminalSampleArgs s)
{
    const int lane = (int)(threadIdx.x & 63u), k = (int)(threadIdx.x >> 6), i = (int)blockIdx.x;
    const int C = s.a.rp.C, B = s.a.rp.B, ns = s.a.rp.n_stack, plane = SIZE64 ? 4096 : s.a.rp.plane;
    const TerminalPick p = terminal_pick(s, i);
    if (k == 0 && lane == 0) terminal_scalars(s, i, p);
    // this wavefront's source: slot s - (ns - 1) + k, i.e. frame k of obs (k < ns) and frame k - 1 of next_obs (k > 0)
    const int d_obs = ns - 1 - k, d_next = ns - k;       // its distance from slot s / from slot s + 1
    bool to_obs = false, to_next = false;
    const uint8_t *from8 = s.a.rp.frames;
    if (p.ok) {
        const int64_t at = (int64_t)p.slot * B + p.env;
        const int s1 = p.slot + 1 == C ? 0 : p.slot + 1;
        const int age = s.a.rp.age[at], age1 = s.a.rp.age[(int64_t)s1 * B + p.env];
        const uint32_t done = s.a.rp.done[at];
        const bool ended = (done & kTermEnded) != 0;
        const int row = terminal_row(s, at, done);
        // a frame is shown when it belongs to the episode (age) and has not been overwritten (it lies at or behind `first`)
        to_obs = k < ns && d_obs <= age && d_obs <= p.off;
        if (row >= 0) {
            // the terminal stack: obs moved one frame down, the pool plane on top (the wavefront of slot s + 1 reads it)
            to_next = k == ns || (k > 0 && to_obs);
        } else {
            to_next = k > 0 && !ended && d_next <= age1 && d_next <= p.off + 1;
        }
        if (row >= 0 && k == ns) {
            from8 = s.a.tm.pool + ((int64_t)p.slot * s.a.tm.M + row) * plane;
        } else {
            const int ss = (p.slot - d_obs + C) % C;     // (d_obs >= -1 and C >= ns + 1 > d_obs)
            from8 = s.a.rp.frames + ((int64_t)ss * B + p.env) * plane;
        }
    }
    const uint4 *from = reinterpret_cast<const uint4 *>(from8);
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

__global__ __launch_bounds__(64 * kTermWaves) void terminal_gather_rows_kernel(TerminalSampleArgs s, int N)
{
    const int lane = (int)(threadIdx.x & 63u), i = (int)blockIdx.x * kTermWaves + (int)(threadIdx.x >> 6);
    if (i >= N) return;
    const int C = s.a.rp.C, B = s.a.rp.B, D = s.a.rp.D;
    const TerminalPick p = terminal_pick(s, i);
    if (lane == 0) terminal_scalars(s, i, p);
    const float *rows = reinterpret_cast<const float *>(s.a.rp.frames);
    const float *row = rows, *next = nullptr;
    if (p.ok) {
        const int64_t at = (int64_t)p.slot * B + p.env;
        const uint32_t done = s.a.rp.done[at];
        const int r = terminal_row(s, at, done);
        row = rows + at * D;
        if (r >= 0) next = reinterpret_cast<const float *>(s.a.tm.pool) + ((int64_t)p.slot * s.a.tm.M + r) * D;
        else if ((done & kTermEnded) == 0) next = rows + ((int64_t)(p.slot + 1 == C ? 0 : p.slot + 1) * B + p.env) * D;
    }
    float *o = reinterpret_cast<float *>(s.obs) + (int64_t)i * D, *n = reinterpret_cast<float *>(s.next_obs) + (int64_t)i * D;
    for (int c = lane; c < D; c += 64) {
        o[c] = p.ok ? row[c] : 0.0f;
        n[c] = next ? next[c] : 0.0f;
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

unsigned env_blocks(int B) { return (unsigned)((B + tde::kTermEnvs - 1) / tde::kTermEnvs); }

// the ring and the pool beside it; fills the launch's argument block
int check_terminal(const char *fn, const tde_replay *rp, const tde_terminal *tm, tde::TerminalArgs &a)
{
    const int rc = tde_host::check_terminal_struct(fn, rp, tm);
    if (rc) return rc;
    a.rp = *rp;
    a.tm = *tm;
    a.vec = rp->plane > 0;
    a.row = a.vec ? (int64_t)rp->plane : (int64_t)rp->D * 4;
    return 0;
}

}  // namespace

int tde_host::check_terminal_struct(const char *fn, const tde_replay *rp, const tde_terminal *tm)
{
    const int rc = tde_host::check_replay_struct(fn, rp);
    if (rc) return rc;
    if (!tm) return bad_in(fn, "NULL argument");
    if (tm->M < 1 || tm->M > rp->B) return bad_in(fn, "M must be in [1, B]");
    if (!tm->pool || !tm->ref) return bad_in(fn, "a NULL array in the terminal pool");
    if (!aligned(tm->pool, rp->plane > 0 ? 16 : 4) || !aligned(tm->ref, 4))
        return bad_in(fn, "pool must be 16-byte aligned (rows mode: 4), ref 4-byte");
    return 0;
}

int tde_terminal_version(void) { return TDE_TERMINAL_VERSION; }

int tde_terminal_stash(int32_t B, int32_t row_bytes, const uint8_t *done_bits, const uint8_t *src, int64_t src_stride, uint8_t *dst,
                       void *stream)
{
    const char *fn = "tde_terminal_stash";
    if (B < 1) return bad_in(fn, "B must be >= 1");
    if (row_bytes < 4 || row_bytes % 4 != 0) return bad_in(fn, "row_bytes must be a positive multiple of 4");
    if (!done_bits || !src || !dst) return bad_in(fn, "NULL argument");
    if (src_stride < row_bytes) return bad_in(fn, "src_stride is smaller than a frame / row");
    const bool vec = row_bytes % 16 == 0;
    const int64_t al = vec ? 16 : 4;
    if (src_stride % al != 0 || !aligned(src, al) || !aligned(dst, al))
        return bad_in(fn, "src, src_stride and dst must be multiples of 16 (row_bytes not a multiple of 16: 4)");
    tde::terminal_stash_kernel<<<env_blocks(B), tde::kTermEnvs, 0, (hipStream_t)stream>>>(B, row_bytes, vec, done_bits, src, src_stride, dst);
    return tde_host::launch_status(fn);
}

int tde_terminal_push(const tde_replay *rp, const tde_terminal *tm, int32_t w, const uint8_t *done_bits, const uint8_t *term_src,
                      int64_t term_stride, void *stream)
{
    const char *fn = "tde_terminal_push";
    tde::TerminalArgs a;
    const int rc = check_terminal(fn, rp, tm, a);
    if (rc) return rc;
    if (w < 0 || w >= rp->C) return bad_in(fn, "w must be in [0, C)");
    if (!done_bits) return bad_in(fn, "NULL argument");
    if (!term_src) return bad_in(fn, "term_src is NULL");
    if (term_stride < a.row) return bad_in(fn, "term_stride is smaller than a frame / row");
    const int64_t al = a.vec ? 16 : 4;
    if (term_stride % al != 0 || !aligned(term_src, al)) return bad_in(fn, "term_src and term_stride must be multiples of 16 (rows mode: 4)");
    tde::terminal_push_kernel<<<env_blocks(rp->B), tde::kTermEnvs, 0, (hipStream_t)stream>>>(a, w, done_bits, term_src, term_stride);
    return tde_host::launch_status(fn);
}

int tde_terminal_sample(const tde_replay *rp, const tde_terminal *tm, int32_t first, int32_t count, int32_t N, const int32_t *idx_in,
                        uint64_t seed, uint64_t draw, int32_t *idx, uint8_t *obs, uint8_t *next_obs, float *action, float *reward,
                        uint8_t *done, void *stream)
{
    const char *fn = "tde_terminal_sample";
    tde::TerminalSampleArgs s;
    const int rc = check_terminal(fn, rp, tm, s.a);
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
        if (rp->plane == 4096) tde::terminal_gather_planes_kernel<true><<<(unsigned)N, threads, 0, st>>>(s);
        else tde::terminal_gather_planes_kernel<false><<<(unsigned)N, threads, 0, st>>>(s);
    } else {
        tde::terminal_gather_rows_kernel<<<(unsigned)((N + tde::kTermWaves - 1) / tde::kTermWaves), 64 * tde::kTermWaves, 0, st>>>(s, N);
    }
    return tde_host::launch_status(fn);
}
