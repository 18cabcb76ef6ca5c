// tde_onpolicy.hip — the on-policy view of the replay ring, include/tde_onpolicy.h: its kernels, its host-side checks and its entry
// points (a translation unit of its own: no existing kernel includes it, and it changes none - the ring is filled by tde_replay.hip).
//   * tde_gae: one lane per env, rows read coalesced along B.  The recurrence is a serial chain of T steps per lane, but nothing it
//     loads depends on it, so the loads of the NEXT kGaeBlock steps (reward, done bits, value: three per step) are issued before the
//     arithmetic of the current block and land while it runs.  At 8192 envs the grid is 128 wavefronts on 256 CUs: no second
//     wavefront hides anything, the block in flight is all the latency hiding there is, and its registers (2 x 3 x kGaeBlock) cost
//     no occupancy that anyone would use.  T / kGaeBlock memory round trips per lane instead of T.
//   * tde_onpolicy_gather, planes mode: one workgroup per sample, one wavefront per frame of the stack; each reads its layer plane
//     once (four 16-byte loads per lane at 64 x 64, in flight together) and expands it into its frame of `obs`, or writes zeros there:
//     tde_replay_sample's construction of `obs` - tde_ring.h's frame rule and expansion - without the wavefront and the bytes of
//     `next_obs`.
//   * tde_onpolicy_gather, rows mode: one wavefront per sample copies its row.
// All offsets into frames / obs and into the [T][B] arrays are int64_t.  The specification is restated in numpy by
// tests/onpolicy_ref.py.
#include "tde_ring.h"
#include "../../include/tde_onpolicy.h"

namespace tde {

constexpr int kGaeBlock = 16;           // steps whose loads are in flight together

struct GaeArgs {
    const float *reward;                // [C][B] of the ring
    const uint8_t *done;
    int C, B, T, base;                  // base: the slot of step 0
    const float *values, *last_values;
    float gamma, gl;
    float *adv, *ret;
};

struct GaeSteps {
    float r[kGaeBlock], v[kGaeBlock];
    uint32_t d[kGaeBlock];
};

// steps hi, hi - 1, ... of env e (a step before the rollout's first reads step 0 again: no lane branches around a load)
TDE_DEV void gae_load(const GaeArgs &g, int e, int hi, GaeSteps &b)
{
#pragma unroll
    for (int j = 0; j < kGaeBlock; ++j) {
        const int t = hi - j < 0 ? 0 : hi - j;
        const int64_t at = (int64_t)ring_slot(g.base, t, g.C) * g.B + e;
        b.r[j] = g.reward[at];
        b.d[j] = g.done[at];
        b.v[j] = g.values[(int64_t)t * g.B + e];
    }
}

__global__ __launch_bounds__(64) void gae_kernel(GaeArgs g)
{
    const int e = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (e >= g.B) return;
    float nv = g.last_values[e], last = 0.0f;
    GaeSteps cur, nxt;
    gae_load(g, e, g.T - 1, cur);
    for (int hi = g.T - 1; hi >= 0; hi -= kGaeBlock) {
        gae_load(g, e, hi - kGaeBlock, nxt);
#pragma unroll
        for (int j = 0; j < kGaeBlock; ++j) {
            const int t = hi - j;
            if (t >= 0) {               // (wave-uniform; no break: the loop must unroll for cur to stay in registers)
                const bool nnt = (cur.d[j] & kRingEnded) == 0;
                const float delta = (cur.r[j] + (nnt ? g.gamma * nv : 0.0f)) - cur.v[j];
                last = delta + (nnt ? g.gl * last : 0.0f);
                g.adv[(int64_t)t * g.B + e] = last;
                g.ret[(int64_t)t * g.B + e] = last + cur.v[j];
                nv = cur.v[j];
            }
        }
        cur = nxt;
    }
}

struct OnpolicyArgs {
    tde_replay rp;
    int base, lead, T;                  // base: the slot of step 0; lead = count - T: stored slots before it
    const int32_t *idx;
    const float *values, *log_prob, *adv, *ret;
    uint8_t *obs;
    float *action, *old_values, *old_log_prob, *adv_out, *ret_out;
};

// sample i (wave-uniform): the pair of index t * B + e - step t is slot base + t, lead + t slots after `first`
TDE_DEV RingPick onpolicy_pick(const OnpolicyArgs &g, int i)
{
    const int B = g.rp.B, v = g.idx[i];
    RingPick p;
    p.ok = v >= 0 && v < g.T * B;       // (T * B <= INT32_MAX: checked by the host)
    const int t = p.ok ? v / B : 0;
    p.env = p.ok ? v - t * B : 0;
    p.slot = ring_slot(g.base, t, g.rp.C);
    p.off = g.lead + t;
    return p;
}

// the scalars of sample i, by one lane
TDE_DEV void onpolicy_scalars(const OnpolicyArgs &g, int i, const RingPick &p)
{
    const int64_t at = (int64_t)p.slot * g.rp.B + p.env, row = (int64_t)(p.off - g.lead) * g.rp.B + p.env;
    reinterpret_cast<float2 *>(g.action)[i] = p.ok ? reinterpret_cast<const float2 *>(g.rp.action)[at] : make_float2(0.0f, 0.0f);
    g.old_values[i] = p.ok ? g.values[row] : 0.0f;
    g.old_log_prob[i] = p.ok ? g.log_prob[row] : 0.0f;
    g.adv_out[i] = p.ok ? g.adv[row] : 0.0f;
    g.ret_out[i] = p.ok ? g.ret[row] : 0.0f;
}

// SIZE64: plane == 4096 (the reference's 64 x 64 observation: the four chunks of a lane in flight together)
template <bool SIZE64>
__global__ __launch_bounds__(64 * TDE_REPLAY_MAX_STACK) void onpolicy_gather_planes_kernel(OnpolicyArgs g)
{
    const int lane = (int)(threadIdx.x & 63u), k = (int)(threadIdx.x >> 6), i = (int)blockIdx.x;
    const int C = g.rp.C, B = g.rp.B, ns = g.rp.n_stack, plane = SIZE64 ? 4096 : g.rp.plane;
    const RingPick p = onpolicy_pick(g, i);
    if (k == 0 && lane == 0) onpolicy_scalars(g, i, p);
    // this wavefront's frame: k of obs (oldest first), slot s - d
    const int d = ns - 1 - k;
    bool show = false;
    int64_t src = 0;
    if (p.ok) {
        show = ring_shown(d, g.rp.age[(int64_t)p.slot * B + p.env], p.off);
        src = ((int64_t)ring_slot(p.slot, -d, C) * B + p.env) * plane;       // (C >= ns + 1 > d)
    }
    const RingFrame o = {g.obs + ((int64_t)i * ns + k) * 3 * plane, true, show}, none = {nullptr, false, false};
    ring_expand<SIZE64>(reinterpret_cast<const uint4 *>(g.rp.frames + src), plane, lane, o, none);
}

__global__ __launch_bounds__(64 * kRingWaves) void onpolicy_gather_rows_kernel(OnpolicyArgs g, int N)
{
    const int lane = (int)(threadIdx.x & 63u), i = (int)blockIdx.x * kRingWaves + (int)(threadIdx.x >> 6);
    if (i >= N) return;
    const int D = g.rp.D;
    const RingPick p = onpolicy_pick(g, i);
    if (lane == 0) onpolicy_scalars(g, i, p);
    const float *row = reinterpret_cast<const float *>(g.rp.frames) + ((int64_t)p.slot * g.rp.B + p.env) * D;
    float *o = reinterpret_cast<float *>(g.obs) + (int64_t)i * D;
    for (int c = lane; c < D; c += 64) o[c] = p.ok ? row[c] : 0.0f;
}

}  // namespace tde

using namespace tde_host;

namespace {

// the ring (tde_replay.hip's own check of the struct) and the rollout inside it
int check_rollout(const char *fn, const tde_replay *rp, int32_t first, int32_t count, int32_t T)
{
    const int rc = tde_host::check_replay_struct(fn, rp);
    if (rc) return rc;
    if (T < 1) return bad_in(fn, "T must be >= 1");
    if (count < T) return bad_in(fn, "count must be >= T (the rollout is the newest T stored steps)");
    return check_stored(fn, rp, first, count);
}

}  // namespace

int tde_onpolicy_version(void) { return TDE_ONPOLICY_VERSION; }

int tde_gae(const tde_replay *rp, int32_t first, int32_t count, int32_t T, const float *values, const float *last_values, float gamma,
            float lam, float *advantages, float *returns, void *stream)
{
    const char *fn = "tde_gae";
    const int rc = check_rollout(fn, rp, first, count, T);
    if (rc) return rc;
    if (!values || !last_values || !advantages || !returns) return bad_in(fn, "NULL argument");
    if (!aligned(values, 4) || !aligned(last_values, 4) || !aligned(advantages, 4) || !aligned(returns, 4))
        return bad_in(fn, "values, last_values, advantages and returns must be 4-byte aligned");
    tde::GaeArgs g;
    g.reward = rp->reward; g.done = rp->done; g.C = rp->C; g.B = rp->B; g.T = T;
    g.base = (first + count - T) % rp->C;
    g.values = values; g.last_values = last_values;
    g.gamma = gamma; g.gl = gamma * lam;
    g.adv = advantages; g.ret = returns;
    tde::gae_kernel<<<(unsigned)((rp->B + 63) / 64), 64, 0, (hipStream_t)stream>>>(g);
    return tde_host::launch_status(fn);
}

int tde_onpolicy_gather(const tde_replay *rp, int32_t first, int32_t count, int32_t T, int32_t N, const int32_t *idx, const float *values,
                        const float *log_prob, const float *advantages, const float *returns, uint8_t *obs, float *action,
                        float *old_values, float *old_log_prob, float *adv_out, float *ret_out, void *stream)
{
    const char *fn = "tde_onpolicy_gather";
    const int rc = check_rollout(fn, rp, first, count, T);
    if (rc) return rc;
    if (N < 1) return bad_in(fn, "N must be >= 1");
    if ((int64_t)T * rp->B > INT32_MAX) return bad_in(fn, "T * B must be <= INT32_MAX (idx is int32)");
    if (!idx || !values || !log_prob || !advantages || !returns) return bad_in(fn, "NULL argument");
    if (!obs || !action || !old_values || !old_log_prob || !adv_out || !ret_out) return bad_in(fn, "a NULL output");
    const bool planes = rp->plane > 0;
    if (!aligned(obs, planes ? 16 : 4) || !aligned(action, 8) || !aligned(idx, 4) || !aligned(values, 4) || !aligned(log_prob, 4) ||
        !aligned(advantages, 4) || !aligned(returns, 4) || !aligned(old_values, 4) || !aligned(old_log_prob, 4) || !aligned(adv_out, 4) ||
        !aligned(ret_out, 4))
        return bad_in(fn, "obs must be 16-byte aligned (rows mode: 4), action 8-byte, idx and the float arrays 4-byte");
    tde::OnpolicyArgs g;
    g.rp = *rp;
    g.base = (first + count - T) % rp->C; g.lead = count - T; g.T = T;
    g.idx = idx; g.values = values; g.log_prob = log_prob; g.adv = advantages; g.ret = returns;
    g.obs = obs; g.action = action; g.old_values = old_values; g.old_log_prob = old_log_prob; g.adv_out = adv_out; g.ret_out = ret_out;
    hipStream_t st = (hipStream_t)stream;
    if (planes) {
        const unsigned threads = 64u * (unsigned)rp->n_stack;
        if (rp->plane == 4096) tde::onpolicy_gather_planes_kernel<true><<<(unsigned)N, threads, 0, st>>>(g);
        else tde::onpolicy_gather_planes_kernel<false><<<(unsigned)N, threads, 0, st>>>(g);
    } else {
        tde::onpolicy_gather_rows_kernel<<<ring_blocks(N, tde::kRingWaves), 64 * tde::kRingWaves, 0, st>>>(g, N);
    }
    return tde_host::launch_status(fn);
}
