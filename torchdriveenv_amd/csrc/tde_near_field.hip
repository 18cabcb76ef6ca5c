// tde_near_field.hip — the near-field spawner of tde_near_field_spawn (the stand-in for the reference's iai_conditional_initialize,
// gym_env.py:232-238, iai.py:6-60) and its launcher.  One wavefront per env: the candidates of the env's scenario that are eligible
// by distance and fixed conflicts are compacted into LDS as (priority, index) keys, sorted (bitonic), and visited in batches of 64
// in that order; the accepted set is a bitmap in LDS.  Inside a batch the sequential rule - a candidate is taken unless a neighbour
// of it was taken before it - is resolved from ballots: lanes without an earlier neighbour in the batch decide at once, the others
// in lane order on the scalar unit; a prefix count (v_mbcnt) caps the batch at the target.  The specification (include/tde_hip.h)
// is restated in numpy by tests/near_field_ref.py.
#include "tde_kernels.h"
#include "tde_host.h"

namespace tde {

constexpr int kNfCand = TDE_NF_MAX_CAND;

struct NfShared {
    unsigned long long key[kNfCand];   // (priority << 32) | candidate, the eligible ones first, padded with ~0
    uint32_t taken[kNfCand / 32];      // accepted candidates
    uint8_t lane_of[kNfCand];          // lane of a candidate in the current batch, 0xFF: not in it
    uint8_t free_slot[TDE_MAX_AGENTS];
};

TDE_DEV uint32_t word_of(uint4 r, uint32_t k) { return k == 0u ? r.x : k == 1u ? r.y : k == 2u ? r.z : r.w; }

TDE_DEV double nf_d2(float ax, float ay, float bx, float by)
{
    const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by;
    return dx * dx + dy * dy;
}

__global__ __launch_bounds__(kWave) void near_field_kernel(tde_config cfg, tde_world w, tde_state st, tde_near_field nf,
                                                         const uint8_t *mask)
{
    __shared__ NfShared sh;
    const int e = blockIdx.x;
    const int lane = threadIdx.x;
    if (e >= st.B || (mask && !mask[e])) return;
    const int A = st.A;
    const int64_t base = (int64_t)e * A;
    // the per-slot routes of the env's last episode end here, whatever this call spawns (the accepted lanes write theirs below,
    // behind at least one barrier)
    if (st.slot_route)
        for (int a = 1 + lane; a < A; a += kWave) st.slot_route[base + a] = 0u;
    const int s = st.scn[e];
    if (s < 0 || s >= nf.S) return;
    const uint32_t c = (uint32_t)st.episode[e];
    const uint32_t g = cfg.env_base + (uint32_t)e;
    const float ex = st.x[base], ey = st.y[base];
    const double r2 = (double)nf.radius * (double)nf.radius;
    const double ce2 = (double)nf.clear_ego * (double)nf.clear_ego;

    // present / in-range counts and the free slots (spawn record absent), ascending
    int n_present = 0, n_in = 0, n_free = 0;
    for (int a0 = 0; a0 < A; a0 += kWave) {
        const int a = a0 + lane;
        const bool live = a < A && st.present[base + a] != 0;
        const bool in = live && nf_d2(st.x[base + a], st.y[base + a], ex, ey) < r2;
        const bool fr = a < A && a > 0 && w.spawn[(int64_t)s * A + a].present == 0;
        const unsigned long long bf = __ballot(fr);
        if (fr) sh.free_slot[n_free + lane_prefix(bf)] = (uint8_t)a;
        n_present += __popcll(__ballot(live));
        n_in += __popcll(__ballot(in));
        n_free += __popcll(bf);
    }
    int T = nf.count - n_present;
    if (nf.density > T) T = nf.density;
    T -= n_in;
    if (n_free < T) T = n_free;
    if (T <= 0) return;

    // eligible candidates -> keys
    const int n = min(nf.n_cand[s], nf.NC);
    const tde_nf_cand *cand = nf.cand + (int64_t)s * nf.NC;
    const uint8_t *fixed = nf.fixed + (int64_t)s * nf.NC;
    int ne = 0;
    for (int i0 = 0; i0 < n; i0 += kWave) {
        const int i = i0 + lane;
        bool ok = false;
        uint32_t prio = 0u;
        if (i < n && !fixed[i]) {
            const double d2 = nf_d2(cand[i].x, cand[i].y, ex, ey);
            ok = ce2 <= d2 && d2 <= r2;
            if (ok) prio = word_of(philox(cfg.seed, g, c, (uint32_t)i >> 2, TDE_NF_TAG), (uint32_t)i & 3u);
        }
        const unsigned long long b = __ballot(ok);
        if (ok) sh.key[ne + lane_prefix(b)] = ((unsigned long long)prio << 32) | (uint32_t)i;
        ne += __popcll(b);
    }
    if (ne == 0) return;
    int P = 1;
    while (P < ne) P <<= 1;
    for (int i = ne + lane; i < P; i += kWave) sh.key[i] = ~0ull;
    for (int i = lane; i < kNfCand / 32; i += kWave) sh.taken[i] = 0u;
    for (int i = lane; i < kNfCand; i += kWave) sh.lane_of[i] = 0xFF;
    __syncthreads();

    // bitonic sort of the P keys, ascending
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += kWave) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const unsigned long long ki = sh.key[i], kl = sh.key[l];
                if ((ki > kl) == ((i & k) == 0)) { sh.key[i] = kl; sh.key[l] = ki; }
            }
            __syncthreads();
        }

    // visit in batches of 64
    const uint16_t *nbr = nf.nbr + (int64_t)s * nf.NC * nf.K;
    const uint8_t *nbr_n = nf.nbr_n + (int64_t)s * nf.NC;
    int n_acc = 0;
    for (int b0 = 0; b0 < ne && n_acc < T; b0 += kWave) {
        const bool has = b0 + lane < ne;
        const int i = has ? (int)(uint32_t)sh.key[b0 + lane] : 0;
        if (has) sh.lane_of[i] = (uint8_t)lane;
        __syncthreads();
        bool elig = has;
        uint32_t conf_lo = 0u, conf_hi = 0u;                 // earlier lanes of this batch that are neighbours
        if (has) {
            const int nn = min((int)nbr_n[i], nf.K);
            for (int q = 0; q < nn; ++q) {
                const int j = nbr[(int64_t)i * nf.K + q];
                if (j >= n) continue;
                if ((sh.taken[j >> 5] >> (j & 31)) & 1u) elig = false;
                const int m = sh.lane_of[j];
                if (m < lane) {                              // (0xFF: not in the batch)
                    if (m < 32) conf_lo |= 1u << m;
                    else conf_hi |= 1u << (m - 32);
                }
            }
        }
        __syncthreads();
        if (has) sh.lane_of[i] = 0xFF;
        const unsigned long long E = __ballot(elig);
        const unsigned long long C = __ballot(elig && (conf_lo | conf_hi) != 0u);
        unsigned long long acc = E & ~C;
        for (unsigned long long rem = C; rem; rem &= rem - 1) {   // (wave-uniform: scalar)
            const int m = __builtin_ctzll(rem);
            const unsigned long long cm = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)conf_hi, m) << 32) |
                                          (uint32_t)__builtin_amdgcn_readlane((int)conf_lo, m);
            if (!(cm & acc)) acc |= 1ull << m;
        }
        const int room = T - n_acc;
        const int rank = lane_prefix(acc);
        if (mask_bit(acc, lane) && rank < room) {
            const int a = sh.free_slot[n_acc + rank];
            const int64_t gi = base + a;
            const tde_nf_cand cd = cand[i];
            const uint32_t wv = word_of(philox(cfg.seed, g, c, 512u + ((uint32_t)i >> 2), TDE_NF_TAG), (uint32_t)i & 3u);
            st.x[gi] = cd.x; st.y[gi] = cd.y; st.psi[gi] = cd.psi;
            st.v[gi] = (float)(u01(wv) * (double)cd.vdes);
            st.len[gi] = cd.len; st.wid[gi] = cd.wid; st.lr[gi] = cd.lr; st.vdes[gi] = cd.vdes;
            st.route_wp[gi] = st.slot_route ? (int)cd.route_wp : 0;
            if (st.slot_route && cd.route) st.slot_route[gi] = cd.route | (cd.route_n << TDE_CACHE_ID_BITS);
            st.present[gi] = 1; st.collided[gi] = 0; st.offroad[gi] = 0;
            if (st.slot_cache) st.slot_cache[gi].key = 0;        // (TDE_CACHE_VALID clear)
            atomicOr(&sh.taken[i >> 5], 1u << (i & 31));
        }
        const int got = __popcll(acc);
        n_acc += got < room ? got : room;
        __syncthreads();
    }
    // the NPC actions stored for this env were formed without the new agents: the next step recomputes them
    if (n_acc > 0 && st.act_cache && lane == 0)
        *reinterpret_cast<int2 *>(st.act_cache + (int64_t)e * (A + 1) + A) = make_int2(-1, 0);
}

}  // namespace tde

namespace tde_host {

int launch_near_field(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_near_field *nf,
                      const uint8_t *mask, void *stream)
{
    tde::near_field_kernel<<<(unsigned)st->B, tde::kWave, 0, (hipStream_t)stream>>>(*cfg, *world, *st, *nf, mask);
    return launch_status("tde_near_field_spawn");
}

}  // namespace tde_host
