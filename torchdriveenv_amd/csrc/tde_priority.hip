// tde_priority.hip — prioritized replay over the ring, include/tde_priority.h: its kernels, its host-side checks and its entry points (a
// translation unit of its own: no existing kernel includes it, and it changes none - the ring is filled by tde_replay.hip and the
// picked pairs are gathered by the samplers that exist, through idx_in).
//   * the tree: a 64-ary sum tree over the n = C * B leaves.  Level 0 is `leaf` (uint32); level k has n_k = ceil(n_(k-1) / 64) uint64
//     nodes, the last level K has one: the total.  `sums` holds the levels top down - the root at word 0, level K - 1 behind it, level 1
//     last - so sums[0] is the total whatever the shape.  A child beyond its level's end reads as zero and is never written.
//   * the rebuild: priorities are integers, so the inner nodes are rebuilt WHOLE after every push and update instead of being patched -
//     the same bits in any order.  One launch: lane j of a wavefront adds the 64 leaves of one level-1 node (sixteen 16-byte loads) and
//     stores it, the wavefront adds its 64 lanes into its level-2 node and stores it, and lane 0 adds that into the wavefront's
//     ancestors of level 3 and up with a 64-bit atomicAdd.  Those top levels are the first words of `sums`; the kernel that wrote the
//     leaves - the launch before, in stream order - zeroed them.  2 MB of reads at 64 x 8192 leaves.
//   * the descent: one wavefront per sample, four samples per workgroup.  At each level lane j loads child j of the node, the
//     wavefront makes an inclusive scan over its 64 lanes, the ballot of `inclusive > u` gives the child (its first set bit, a scalar
//     find-first-one: no vector shift), and u loses that child's exclusive prefix.  Four dependent loads per sample at 64 x 8192; the
//     chain is hidden by the other wavefronts of the CU (the kernel needs few registers, so every SIMD holds its eight).
//   * the validity rule of a pair is tde_ring.h's (ring_slot, ring_whole): nothing of it is restated here.
// All 64-bit arithmetic is adds, compares, multiplies and one division per wavefront: no 64-bit shift by a per-lane amount.
// The specification is restated in Python integers by tests/priority_ref.py, which picks by a prefix sum and knows no tree.
#include "tde_ring.h"
#include "../../include/tde_priority.h"

namespace tde {

constexpr int kPriorityLevels = 11;      // 64^11 > 2^62 >= C * B
constexpr int kPriorityThreads = 256;

struct PriorityArgs {
    tde_replay rp;
    tde_priority pr;
    int64_t n;                           // leaves: C * B
    int K;                               // inner levels 1 .. K; level K is the root
    int64_t len[kPriorityLevels + 1];    // nodes of level k (len[0] = n)
    int64_t at[kPriorityLevels + 1];     // first word of level k in `sums` (k >= 1)
    int64_t top;                         // words of the levels >= 3: sums[0 .. top)
};

// is (slot, env) a stored transition with its whole frame stack in the ring?  (the invariant's rule, for pairs a caller names)
TDE_DEV bool priority_valid(const PriorityArgs &a, int first, int count, int slot, int env)
{
    if (slot < 0 || slot >= a.rp.C || env < 0 || env >= a.rp.B) return false;
    const int off = ring_slot(slot, -first, a.rp.C);
    return off < count && ring_whole(a.rp.age[(int64_t)slot * a.rp.B + env], a.rp.n_stack, off);
}

// the levels the rebuild adds into with atomics start from zero: by the first workgroup of the launch that writes the leaves
TDE_DEV void priority_clear_top(const PriorityArgs &a)
{
    if (blockIdx.x != 0) return;
    for (int64_t i = threadIdx.x; i < a.top; i += blockDim.x) a.pr.sums[i] = 0;
}

__global__ __launch_bounds__(kPriorityThreads) void priority_reset_kernel(PriorityArgs a, int64_t words)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t i = t; i < a.n; i += stride) a.pr.leaf[i] = 0;
    for (int64_t i = t; i < words; i += stride) a.pr.sums[i] = 0;
    if (t == 0) *a.pr.qmax = TDE_PRIORITY_ONE;
}

// one thread per env: the header's three rules in the header's order
__global__ __launch_bounds__(kPriorityThreads) void priority_push_kernel(PriorityArgs a, int w, int first, int count)
{
    priority_clear_top(a);
    const int e = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int C = a.rp.C, B = a.rp.B, ns = a.rp.n_stack;
    if (e >= B) return;
    a.pr.leaf[(int64_t)w * B + e] = *a.pr.qmax;
    a.pr.leaf[(int64_t)ring_slot(w, 1, C) * B + e] = 0;
    const int reach = min(ns - 1, count);
    for (int d = 0; d < reach; ++d) {
        const int64_t at = (int64_t)ring_slot(first, d, C) * B + e;
        if (!ring_whole(a.rp.age[at], ns, d)) a.pr.leaf[at] = 0;
    }
}

TDE_DEV uint32_t priority_quantise(float p)
{
    const float r = __builtin_rintf(p * 65536.0f);
    if (!(r >= 1.0f)) return 1u;                            // NaN, zero, negative, and what rounds to zero
    return r >= (float)TDE_PRIORITY_QMAX ? TDE_PRIORITY_QMAX : (uint32_t)r;
}

// one thread per entry.  RAISE false: the valid named leaves go to zero; true: each takes the largest q that names it
template <bool RAISE>
__global__ __launch_bounds__(kPriorityThreads) void priority_update_kernel(PriorityArgs a, int first, int count, int N, const int32_t *idx,
                                                                           const float *p)
{
    if (!RAISE) priority_clear_top(a);
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= N) return;
    const int slot = idx[2 * (int64_t)i], env = idx[2 * (int64_t)i + 1];
    if (!priority_valid(a, first, count, slot, env)) return;
    uint32_t *leaf = a.pr.leaf + ((int64_t)slot * a.rp.B + env);
    if (RAISE) {
        const uint32_t q = priority_quantise(p[i]);
        atomicMax(leaf, q);
        atomicMax(a.pr.qmax, q);
    } else {
        *leaf = 0;
    }
}

// the sum of a wavefront's 64 values, in every lane
TDE_DEV uint64_t priority_wave_sum(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// levels 1 and 2 by stores, the levels above by atomics: wavefront g owns level-2 node g, lane j of it level-1 node 64 g + j
__global__ __launch_bounds__(kPriorityThreads) void priority_rebuild_kernel(PriorityArgs a)
{
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t g = (int64_t)blockIdx.x * (kPriorityThreads / 64) + (threadIdx.x >> 6);
    if (g >= a.len[2]) return;                              // (len[2] >= 1 for every tree: see priority_shape)
    const int64_t node = g * 64 + lane, at = node * 64;     // my level-1 node and its first leaf
    uint64_t s = 0;
    if (at + 64 <= a.n) {
        const uint4 *src = reinterpret_cast<const uint4 *>(a.pr.leaf + at);
        uint4 v[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) v[c] = src[c];
#pragma unroll
        for (int c = 0; c < 16; ++c) s += (uint64_t)v[c].x + v[c].y + v[c].z + v[c].w;
    } else {
        for (int64_t l = at; l < a.n; ++l) s += a.pr.leaf[l];
    }
    if (node < a.len[1]) a.pr.sums[a.at[1] + node] = s;
    if (a.K < 2) return;
    const uint64_t all = priority_wave_sum(s);
    if (lane != 0) return;
    a.pr.sums[a.at[2] + g] = all;
    int64_t up = g;
    for (int k = 3; k <= a.K; ++k) {
        up >>= 6;
        atomicAdd(reinterpret_cast<unsigned long long *>(a.pr.sums + a.at[k] + up), (unsigned long long)all);
    }
}

// one wavefront per sample
__global__ __launch_bounds__(64 * kRingWaves) void priority_sample_kernel(PriorityArgs a, int N, uint64_t seed, uint32_t draw_lo,
                                                                          uint32_t draw_hi, int32_t *idx, uint32_t *q)
{
    const int lane = (int)(threadIdx.x & 63u), i = (int)blockIdx.x * kRingWaves + (int)(threadIdx.x >> 6);
    if (i >= N) return;
    const uint64_t T = a.pr.sums[0];
    int64_t node = 0;
    uint32_t picked = 0;
    bool found = T != 0;
    if (found) {
        const uint4 wd = philox(seed, (uint32_t)i, draw_lo, draw_hi, TDE_PRIORITY_TAG);
        const uint64_t r = ((uint64_t)wd.x << 32) | wd.y;
        const uint64_t base = T / (uint64_t)N, rem = T - base * (uint64_t)N;
        uint64_t u;
        if (base == 0) {
            u = __umul64hi(r, T);
        } else {
            const uint64_t lo = (uint64_t)i * base + ((uint64_t)i < rem ? (uint64_t)i : rem);
            u = lo + __umul64hi(r, base + ((uint64_t)i < rem ? 1u : 0u));
        }
        for (int k = a.K - 1; k >= 0; --k) {
            const int64_t child = node * 64 + lane;
            uint64_t v = 0;
            if (child < a.len[k]) v = k == 0 ? (uint64_t)a.pr.leaf[child] : a.pr.sums[a.at[k] + child];
            uint64_t inc = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t below = __shfl_up(inc, d);
                if (lane >= d) inc += below;
            }
            const unsigned long long over = __ballot(inc > u);
            // (a tree whose inner nodes are current always has such a child: u < the node's sum; one that is not picks nothing)
            if (!over) {
                found = false;
                break;
            }
            const int c = __ffsll((long long)over) - 1;
            u -= __shfl(inc - v, c);
            picked = (uint32_t)__shfl(v, c);
            node = node * 64 + c;
        }
    }
    if (lane != 0) return;
    found = found && node < a.n;
    idx[2 * (int64_t)i] = found ? (int32_t)(node / a.rp.B) : -1;
    idx[2 * (int64_t)i + 1] = found ? (int32_t)(node % a.rp.B) : -1;
    q[i] = found ? picked : 0u;
}

}  // namespace tde

using namespace tde_host;

namespace {

// levels, lengths and offsets of the tree over n leaves; returns the words of `sums`
int64_t priority_shape(int64_t n, tde::PriorityArgs *a)
{
    int64_t len[tde::kPriorityLevels + 1];
    int K = 0;
    len[0] = n;
    do {
        len[K + 1] = (len[K] + 63) / 64;
        ++K;
    } while (len[K] > 1);
    int64_t words = 0;
    for (int k = 1; k <= K; ++k) words += len[k];
    if (a) {
        a->n = n;
        a->K = K;
        for (int k = 0; k <= tde::kPriorityLevels; ++k) a->len[k] = k <= K ? len[k] : 0, a->at[k] = 0;
        int64_t at = 0;
        for (int k = K; k >= 1; --k) a->at[k] = at, at += len[k];
        a->top = K >= 3 ? a->at[2] : 0;
        if (K < 2) a->len[2] = 1;                           // one wavefront rebuilds a one-level tree; it stores no level-2 node
    }
    return words;
}

// the two structs every entry point takes; fills the launch's argument block
int check_priority(const char *fn, const tde_priority *pr, const tde_replay *rp, tde::PriorityArgs &a)
{
    if (!pr) return bad_in(fn, "NULL argument");
    const int rc = check_replay_struct(fn, rp);
    if (rc) return rc;
    if (!pr->leaf || !pr->sums || !pr->qmax) return bad_in(fn, "a NULL array in the priorities");
    if (!aligned(pr->leaf, 16) || !aligned(pr->sums, 8) || !aligned(pr->qmax, 4))
        return bad_in(fn, "leaf must be 16-byte aligned, sums 8-byte, qmax 4-byte");
    a.rp = *rp;
    a.pr = *pr;
    priority_shape((int64_t)rp->C * rp->B, &a);
    return 0;
}

int launch_rebuild(const char *fn, const tde::PriorityArgs &a, hipStream_t st)
{
    const int per = tde::kPriorityThreads / 64;
    tde::priority_rebuild_kernel<<<(unsigned)((a.len[2] + per - 1) / per), tde::kPriorityThreads, 0, st>>>(a);
    return launch_status(fn);
}

}  // namespace

int tde_priority_version(void) { return TDE_PRIORITY_VERSION; }

int64_t tde_priority_words(int32_t C, int32_t B)
{
    if (C < 2 || B < 1) {
        bad_in("tde_priority_words", "C must be >= 2 and B >= 1");
        return -1;
    }
    return priority_shape((int64_t)C * B, nullptr);
}

int tde_priority_reset(const tde_priority *pr, const tde_replay *rp, void *stream)
{
    const char *fn = "tde_priority_reset";
    tde::PriorityArgs a;
    const int rc = check_priority(fn, pr, rp, a);
    if (rc) return rc;
    const int64_t blocks = (a.n + tde::kPriorityThreads - 1) / tde::kPriorityThreads;
    tde::priority_reset_kernel<<<(unsigned)(blocks < 1024 ? blocks : 1024), tde::kPriorityThreads, 0, (hipStream_t)stream>>>(
        a, tde_priority_words(rp->C, rp->B));
    return launch_status(fn);
}

int tde_priority_push(const tde_priority *pr, const tde_replay *rp, int32_t w, int32_t first, int32_t count, void *stream)
{
    const char *fn = "tde_priority_push";
    tde::PriorityArgs a;
    int rc = check_priority(fn, pr, rp, a);
    if (rc || (rc = check_slot(fn, rp, w)) != 0) return rc;
    if (count < 1) return bad_in(fn, "count must be >= 1 (after the push the buffer holds a transition)");
    if ((rc = check_stored(fn, rp, first, count)) != 0) return rc;
    if (((int64_t)first + count - 1) % rp->C != w) return bad_in(fn, "w must be the newest stored slot: (first + count - 1) mod C");
    hipStream_t st = (hipStream_t)stream;
    tde::priority_push_kernel<<<ring_blocks(rp->B, tde::kPriorityThreads), tde::kPriorityThreads, 0, st>>>(a, w, first, count);
    if ((rc = launch_status(fn)) != 0) return rc;
    return launch_rebuild(fn, a, st);
}

int tde_priority_update(const tde_priority *pr, const tde_replay *rp, int32_t first, int32_t count, int32_t N, const int32_t *idx,
                        const float *p, void *stream)
{
    const char *fn = "tde_priority_update";
    tde::PriorityArgs a;
    int rc = check_priority(fn, pr, rp, a);
    if (rc) return rc;
    if (N < 1) return bad_in(fn, "N must be >= 1");
    if (count < 0) return bad_in(fn, "count must be >= 0");
    if ((rc = check_stored(fn, rp, first, count)) != 0) return rc;
    if (!idx || !p) return bad_in(fn, "NULL argument");
    if (!aligned(idx, 4) || !aligned(p, 4)) return bad_in(fn, "idx and p must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = ring_blocks(N, tde::kPriorityThreads);
    tde::priority_update_kernel<false><<<blocks, tde::kPriorityThreads, 0, st>>>(a, first, count, N, idx, p);
    if ((rc = launch_status(fn)) != 0) return rc;
    tde::priority_update_kernel<true><<<blocks, tde::kPriorityThreads, 0, st>>>(a, first, count, N, idx, p);
    if ((rc = launch_status(fn)) != 0) return rc;
    return launch_rebuild(fn, a, st);
}

int tde_priority_sample(const tde_priority *pr, const tde_replay *rp, int32_t first, int32_t count, int32_t N, uint64_t seed,
                        uint64_t draw, int32_t *idx, uint32_t *q, void *stream)
{
    const char *fn = "tde_priority_sample";
    tde::PriorityArgs a;
    int rc = check_priority(fn, pr, rp, a);
    if (rc) return rc;
    if (N < 1) return bad_in(fn, "N must be >= 1");
    if (count < 0) return bad_in(fn, "count must be >= 0");
    if ((rc = check_stored(fn, rp, first, count)) != 0) return rc;
    if (!idx || !q) return bad_in(fn, "a NULL output");
    if (!aligned(idx, 4) || !aligned(q, 4)) return bad_in(fn, "idx and q must be 4-byte aligned");
    tde::priority_sample_kernel<<<ring_blocks(N, tde::kRingWaves), 64 * tde::kRingWaves, 0, (hipStream_t)stream>>>(
        a, N, seed, (uint32_t)draw, (uint32_t)(draw >> 32), idx, q);
    return launch_status(fn);
}
