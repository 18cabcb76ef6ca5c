// tde_snapshot.hip — copies of chosen env rows between two tde_state (or within one), include/tde_snapshot.h: the kernel, the host-side
// checks and the entry point (a translation unit of its own: no existing kernel includes it, and it changes none).
//   * ONE launch on the caller's stream.  blockIdx.x = the pair k.  Workgroup y == 0 is one wavefront: it copies the state row - lanes
//     run over the A slots of each per-agent array (two trips at A = 128, a partial wavefront below 64), then every per-env field moves
//     as 32-bit words and bytes with one field per lane group (one load and one store per lane), then the destination row of each cache
//     is invalidated (zero words; the act cache's key entry (-1, 0)).  Workgroups y >= 1, four wavefronts each, copy the pair's frame
//     planes 16 bytes per lane: the layer planes to the ring slot of the same age, the stacked observation as it is.
//   * the kernel never holds the two states' ~70 addresses in registers (that form spilled 46 SGPRs): the host lays the arrays out as
//     tables in the argument block and a wavefront reads an entry when it needs it - by the loop counter (a scalar load) for the
//     per-agent arrays, by the lane index (a vector load) for the per-env words and bytes.
//   * a pair with an index out of range is skipped by every workgroup of the pair before any address is formed.
//   * no LDS, no barrier, no atomics; vector stores only; no 64-bit lane mask is formed (nothing for tde_device.h's helpers to do).
// All row offsets are int64_t.  The specification is restated in numpy by tests/snapshot_ref.py.
#include <stdlib.h>

#include <vector>

#include "tde_device.h"
#include "tde_host.h"
#include "../../include/tde_snapshot.h"

namespace tde {

constexpr int kSnapFrameThreads = 256;      // a frame workgroup
constexpr int kSnapWordsPerThread = 4;      // 16-byte words a frame thread moves when the grid is not capped
constexpr int kSnapMaxFrameGroups = 1024;   // workgroups per pair at most (a thread then loops)
constexpr int kSnapAgentFields = 13;        // the per-agent arrays, in the header's order
constexpr int kSnapWordLanes = 34;          // 32-bit words of the per-env fields: one lane each
constexpr int kSnapByteLanes = 4;           // the per-env flag bytes: one lane each, behind the word lanes

// one array of the row: where it starts on either side (to == NULL: not copied - absent on a side, or an output without the flag)
struct SnapField {
    const uint8_t *from;
    uint8_t *to;
};

struct SnapshotArgs {
    SnapField agent[kSnapAgentFields];
    uint8_t agent_size[kSnapAgentFields + 3];      // bytes per element (padded to 16)
    SnapField word[kSnapWordLanes];                // the lane's word of env 0 of its field on either side
    SnapField byte[kSnapByteLanes];
    uint8_t word_stride[kSnapWordLanes + 6];       // 32-bit words per env of the lane's field (padded to 40)
    uint8_t *slot_cache, *env_cache, *act_cache;   // dst's, NULL = absent
    tde_snapshot_frames fr;                        // zeros without frames
    const int32_t *src_env, *dst_env;
    int sB, dB, A;
    int frame_groups;                              // workgroups y >= 1 per pair
};

__global__ __launch_bounds__(kSnapFrameThreads) void state_copy_kernel(SnapshotArgs s)
{
    const int k = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int se32 = s.src_env[k], de32 = s.dst_env[k];
    if (se32 < 0 || se32 >= s.sB || de32 < 0 || de32 >= s.dB) return;           // (uniform over the pair's workgroups)
    const int64_t se = se32, de = de32;
    if (blockIdx.y != 0) {
        // ---- frame planes: word w of the pair's layer planes, then of its stacked observation ----
        const int ns = s.fr.n_stack, pw = s.fr.plane / 16;
        const int lw = s.fr.src_layers ? ns * pw : 0, ow = s.fr.src_obs ? 3 * ns * pw : 0;
        const int shift = (s.fr.dst_phase - s.fr.src_phase + ns) % ns;
        const uint4 *sl = reinterpret_cast<const uint4 *>(s.fr.src_layers) + se * ns * pw;
        uint4 *dl = reinterpret_cast<uint4 *>(s.fr.dst_layers) + de * ns * pw;
        const uint4 *so = reinterpret_cast<const uint4 *>(s.fr.src_obs) + se * 3 * ns * pw;
        uint4 *dob = reinterpret_cast<uint4 *>(s.fr.dst_obs) + de * 3 * ns * pw;
        const int stride = s.frame_groups * kSnapFrameThreads;
        for (int w = ((int)blockIdx.y - 1) * kSnapFrameThreads + tid; w < lw + ow; w += stride) {
            if (w < lw) {
                const int j = w / pw, c = w - j * pw;
                int to = j + shift;
                if (to >= ns) to -= ns;
                dl[to * pw + c] = sl[w];
            } else {
                dob[w - lw] = so[w - lw];
            }
        }
        return;
    }
    if (tid >= 64) return;
    const int lane = tid, A = s.A;
    const int64_t sb = se * A, db = de * A;
    // ---- per-agent arrays ----
    for (int f = 0; f < kSnapAgentFields; ++f) {
        const SnapField fd = s.agent[f];
        if (!fd.to) continue;
        if (s.agent_size[f] == 4) {
            const uint32_t *from = reinterpret_cast<const uint32_t *>(fd.from) + sb;
            uint32_t *to = reinterpret_cast<uint32_t *>(fd.to) + db;
            for (int a = lane; a < A; a += 64) to[a] = from[a];
        } else {
            for (int a = lane; a < A; a += 64) fd.to[db + a] = fd.from[sb + a];
        }
    }
    // ---- per-env fields: one 32-bit word per lane, then one byte per lane ----
    if (lane < kSnapWordLanes) {
        const SnapField fd = s.word[lane];
        const int64_t w = s.word_stride[lane];
        if (fd.to) reinterpret_cast<uint32_t *>(fd.to)[de * w] = reinterpret_cast<const uint32_t *>(fd.from)[se * w];
    } else if (lane < kSnapWordLanes + kSnapByteLanes) {
        const SnapField fd = s.byte[lane - kSnapWordLanes];
        if (fd.to) fd.to[de] = fd.from[se];
    }
    // ---- the destination row of every cache dst carries: invalid ----
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    if (s.slot_cache) {
        uint4 *c = reinterpret_cast<uint4 *>(s.slot_cache) + 2 * db;            // 32-byte records
        for (int a = lane; a < 2 * A; a += 64) c[a] = zero;
    }
    if (s.env_cache && lane < 2) reinterpret_cast<uint4 *>(s.env_cache)[2 * de + lane] = zero;
    if (s.act_cache) {
        uint2 *c = reinterpret_cast<uint2 *>(s.act_cache) + de * (A + 1);
        for (int a = lane; a <= A; a += 64) c[a] = a == A ? make_uint2(0xFFFFFFFFu, 0u) : make_uint2(0u, 0u);
    }
}

}  // namespace tde

using namespace tde_host;

namespace {

inline bool snap_aligned(const void *p, uintptr_t n) { return ((uintptr_t)p % n) == 0; }

// the tables of the argument block: the header's groups, array by array; an array absent on either side is left out
void fill_tables(tde::SnapshotArgs &s, const tde_state &a, const tde_state &b, bool outputs)
{
    static_assert(sizeof(tde_slot_cache) == 32 && sizeof(tde_env_cache) == 32 && sizeof(tde_act_cache) == 8, "cache records");
    int f = 0;
    auto agent = [&](const void *from, const void *to, int size) {
        s.agent_size[f] = (uint8_t)size;
        if (from && to) s.agent[f] = tde::SnapField{(const uint8_t *)from, (uint8_t *)const_cast<void *>(to)};
        ++f;
    };
    agent(a.x, b.x, 4); agent(a.y, b.y, 4); agent(a.psi, b.psi, 4); agent(a.v, b.v, 4); agent(a.len, b.len, 4); agent(a.wid, b.wid, 4);
    agent(a.lr, b.lr, 4); agent(a.vdes, b.vdes, 4); agent(a.route_wp, b.route_wp, 4); agent(a.present, b.present, 1);
    agent(a.collided, b.collided, 1); agent(a.offroad, b.offroad, 1); agent(a.slot_route, b.slot_route, 4);
    int lane = 0;
    auto words = [&](const void *from, const void *to, int width, bool on) {           // `width` lanes: word i of the field on lane + i
        for (int i = 0; i < width; ++i, ++lane) {
            s.word_stride[lane] = (uint8_t)width;
            if (on && from && to) s.word[lane] = tde::SnapField{(const uint8_t *)from + 4 * i, (uint8_t *)const_cast<void *>(to) + 4 * i};
        }
    };
    words(a.scn, b.scn, 1, true); words(a.steps, b.steps, 1, true); words(a.target_idx, b.target_idx, 1, true);
    words(a.reached, b.reached, 1, true); words(a.episode, b.episode, 1, true); words(a.action, b.action, 2, true);
    words(a.obs, b.obs, 8, true); words(a.ep_return, b.ep_return, 2, true);
    words(a.reward, b.reward, 1, outputs); words(a.info, b.info, 8, outputs); words(a.info_reached, b.info_reached, 1, outputs);
    words(a.ep_final, b.ep_final, 2, outputs); words(a.ep_final_len, b.ep_final_len, 1, outputs); words(a.magnitudes, b.magnitudes, 4, outputs);
    if (lane != tde::kSnapWordLanes || f != tde::kSnapAgentFields) abort();       // (the tables above and their sizes are one statement)
    int q = 0;
    auto byte = [&](const uint8_t *from, uint8_t *to) {
        if (outputs && from && to) s.byte[q] = tde::SnapField{from, to};
        ++q;
    };
    byte(a.terminated, b.terminated); byte(a.truncated, b.truncated); byte(a.tl_violation, b.tl_violation); byte(a.done_bits, b.done_bits);
    s.slot_cache = (uint8_t *)b.slot_cache; s.env_cache = (uint8_t *)b.env_cache; s.act_cache = (uint8_t *)b.act_cache;
}

// TDE_SNAPSHOT_CHECK: the index arrays on the host (read back through the stream; as host memory in a process without a device)
int read_indices(const char *fn, const int32_t *src_env, const int32_t *dst_env, int32_t n, void *stream, std::vector<int32_t> &se,
                 std::vector<int32_t> &de)
{
    se.resize((size_t)n);
    de.resize((size_t)n);
    int devices = 0;
    if (hipGetDeviceCount(&devices) != hipSuccess || devices < 1) {
        (void)hipGetLastError();
        memcpy(se.data(), src_env, sizeof(int32_t) * (size_t)n);
        memcpy(de.data(), dst_env, sizeof(int32_t) * (size_t)n);
        return 0;
    }
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemcpyAsync(se.data(), src_env, sizeof(int32_t) * (size_t)n, hipMemcpyDefault, st);
    if (e == hipSuccess) e = hipMemcpyAsync(de.data(), dst_env, sizeof(int32_t) * (size_t)n, hipMemcpyDefault, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? 0 : fail(fn, e);
}

int check_indices(const char *fn, const std::vector<int32_t> &se, const std::vector<int32_t> &de, int32_t sB, int32_t dB, bool same)
{
    std::vector<uint8_t> written((size_t)dB, 0), read(same ? (size_t)sB : 0, 0);
    const size_t n = se.size();
    for (size_t k = 0; k < n; ++k) {
        if (se[k] < 0 || se[k] >= sB) return bad_in(fn, "TDE_SNAPSHOT_CHECK: a src_env index is outside [0, src.B)");
        if (de[k] < 0 || de[k] >= dB) return bad_in(fn, "TDE_SNAPSHOT_CHECK: a dst_env index is outside [0, dst.B)");
        if (written[(size_t)de[k]]) return bad_in(fn, "TDE_SNAPSHOT_CHECK: dst_env names a row twice");
        written[(size_t)de[k]] = 1;
        if (same) read[(size_t)se[k]] = 1;
    }
    if (same)
        for (size_t k = 0; k < n; ++k)
            if (read[(size_t)de[k]]) return bad_in(fn, "TDE_SNAPSHOT_CHECK: src and dst are the same state and dst_env overlaps src_env");
    return 0;
}

}  // namespace

int tde_snapshot_version(void) { return TDE_SNAPSHOT_VERSION; }

int tde_state_copy(const tde_state *src, tde_state *dst, int32_t n, const int32_t *src_env, const int32_t *dst_env,
                   const tde_snapshot_frames *frames, uint32_t flags, void *stream)
{
    const char *fn = "tde_state_copy";
    if (!src || !dst) return bad_in(fn, "NULL argument");
    const int A = src->A;
    if (A < 1 || A > TDE_MAX_AGENTS || (A & (A - 1)) != 0) return bad_in(fn, "A must be a power of two in [1, 128]");
    if (dst->A != A) return bad_in(fn, "src and dst must have the same A");
    if (src->B < 1 || dst->B < 1) return bad_in(fn, "B must be >= 1");
    if (n < 0) return bad_in(fn, "n must be >= 0");
    if (flags & ~(uint32_t)(TDE_SNAPSHOT_OUTPUTS | TDE_SNAPSHOT_CHECK)) return bad_in(fn, "unknown flag bits");
    if (n > 0 && (!src_env || !dst_env)) return bad_in(fn, "src_env and dst_env must not be NULL");
    if (!snap_aligned(src_env, 4) || !snap_aligned(dst_env, 4)) return bad_in(fn, "src_env and dst_env must be 4-byte aligned");
    if (src->slot_route && !dst->slot_route) return bad_in(fn, "src carries slot_route and dst does not: the routes would be lost");
    if (!snap_aligned(dst->slot_cache, 16) || !snap_aligned(dst->env_cache, 16) || !snap_aligned(dst->act_cache, 8))
        return bad_in(fn, "dst.slot_cache and dst.env_cache must be 16-byte aligned, dst.act_cache 8-byte");
    tde::SnapshotArgs s;
    memset(&s, 0, sizeof(s));
    fill_tables(s, *src, *dst, (flags & TDE_SNAPSHOT_OUTPUTS) != 0);
    s.src_env = src_env; s.dst_env = dst_env; s.sB = src->B; s.dB = dst->B; s.A = A;
    if (frames) {
        const tde_snapshot_frames &f = *frames;
        if (f.n_stack < 1 || f.n_stack > TDE_SNAPSHOT_MAX_STACK) return bad_in(fn, "frames.n_stack must be in [1, 8]");
        if (f.plane < 1 || f.plane % 16 != 0) return bad_in(fn, "frames.plane must be positive and a multiple of 16");
        if (f.plane > (1 << 24)) return bad_in(fn, "frames.plane must be <= 2^24");
        if (!f.src_layers != !f.dst_layers || !f.src_obs != !f.dst_obs)
            return bad_in(fn, "frames: layers and obs are each given for both sides or for neither");
        if (!snap_aligned(f.src_layers, 16) || !snap_aligned(f.dst_layers, 16) || !snap_aligned(f.src_obs, 16) || !snap_aligned(f.dst_obs, 16))
            return bad_in(fn, "frames: the planes must be 16-byte aligned");
        if (f.src_phase < 0 || f.src_phase >= f.n_stack || f.dst_phase < 0 || f.dst_phase >= f.n_stack)
            return bad_in(fn, "frames: src_phase and dst_phase must be in [0, n_stack)");
        s.fr = f;
        const int64_t words = ((f.src_layers ? 1 : 0) + (f.src_obs ? 3 : 0)) * (int64_t)f.n_stack * (f.plane / 16);
        const int64_t per = (int64_t)tde::kSnapFrameThreads * tde::kSnapWordsPerThread;
        const int64_t groups = (words + per - 1) / per;
        s.frame_groups = (int)(groups < tde::kSnapMaxFrameGroups ? groups : tde::kSnapMaxFrameGroups);
    }
    if (n == 0) return 0;
    if (flags & TDE_SNAPSHOT_CHECK) {
        std::vector<int32_t> se, de;
        int rc = read_indices(fn, src_env, dst_env, n, stream, se, de);
        if (rc) return rc;
        rc = check_indices(fn, se, de, src->B, dst->B, src == dst || (src->x != nullptr && src->x == dst->x));
        if (rc) return rc;
    }
    const dim3 grid((unsigned)n, (unsigned)(1 + s.frame_groups));
    tde::state_copy_kernel<<<grid, tde::kSnapFrameThreads, 0, (hipStream_t)stream>>>(s);
    return launch_status(fn);
}
