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
//   * tde_terminal_sample: tde_ring.h's gather (ring_gather_planes_kernel / ring_gather_rows_kernel), the template tde_replay_sample
//     instantiates, with the pool - the same draw, validity rule and blanking rule by construction.  In planes mode the wavefront of
//     slot s + 1, which writes zeros for an ended transition, reads the pool plane instead, and the wavefronts of the older slots write
//     their plane to next_obs one frame down as well.  The same bytes are written; at most one more plane is read per ended sample.
// All offsets into frames / pool / obs / next_obs are int64_t.  The specification is restated in numpy by tests/terminal_ref.py.
#include "tde_ring.h"

namespace tde {

constexpr int kTermEnvs = 256;          // envs per workgroup of stash / push: one lane each, four wavefronts

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
        ring_copy_row(dst + (int64_t)ee * row, src + (int64_t)ee * src_stride, row, vec, lane);
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
        ring_copy_row(a.tm.pool + ((int64_t)w * M + r) * a.row, src + (int64_t)ee * src_stride, (int)a.row, a.vec, lane);
        ++r;
    }
}

}  // namespace tde

using namespace tde_host;

namespace {

unsigned term_blocks(int B) { return ring_blocks(B, tde::kTermEnvs); }

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
    tde::terminal_stash_kernel<<<term_blocks(B), tde::kTermEnvs, 0, (hipStream_t)stream>>>(B, row_bytes, vec, done_bits, src, src_stride, dst);
    return tde_host::launch_status(fn);
}

int tde_terminal_push(const tde_replay *rp, const tde_terminal *tm, int32_t w, const uint8_t *done_bits, const uint8_t *term_src,
                      int64_t term_stride, void *stream)
{
    const char *fn = "tde_terminal_push";
    tde::TerminalArgs a;
    int rc = check_terminal(fn, rp, tm, a);
    if (rc || (rc = check_slot(fn, rp, w)) != 0) return rc;
    if (!done_bits) return bad_in(fn, "NULL argument");
    if ((rc = check_src(fn, a.row, a.vec, term_src, term_stride, "term_src", "term_stride")) != 0) return rc;
    tde::terminal_push_kernel<<<term_blocks(rp->B), tde::kTermEnvs, 0, (hipStream_t)stream>>>(a, w, done_bits, term_src, term_stride);
    return tde_host::launch_status(fn);
}

int tde_terminal_sample(const tde_replay *rp, const tde_terminal *tm, int32_t first, int32_t count, int32_t N, const int32_t *idx_in,
                        uint64_t seed, uint64_t draw, int32_t *idx, uint8_t *obs, uint8_t *next_obs, float *action, float *reward,
                        uint8_t *done, void *stream)
{
    const char *fn = "tde_terminal_sample";
    tde::TerminalSampleArgs s;
    int rc = check_terminal_struct(fn, rp, tm);
    if (rc || (rc = check_sample(fn, rp, first, count, N, idx_in, seed, draw, idx, obs, next_obs, action, reward, done, s)) != 0) return rc;
    s.tm = *tm;
    return launch_sample(fn, s, N, stream);
}
