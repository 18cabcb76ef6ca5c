// tde_eval_kernels.h — evaluation over chosen scenarios (tde_env_reset_to, tde_eval_advance: include/tde_hip.h): the reset with the
// scenario given instead of drawn, and the per-step fold of whole-episode records with the re-spawn to the next planned scenario.
// Included by tde_kernels.h after the step path's own definitions (Agent, reset_lane, kBlock); both kernels are templates,
// instantiated by the unit that launches them (tde_api.hip).  Every store is an ordinary vector store from plain C++.
#pragma once

namespace tde {

// env_reset_kernel with the scenario of env e taken from scn[e] when that is >= 0 (one lane per (env, slot), the lanes of an env
// enter reset_lane together: its Philox blocks travel by wavefront shuffles).  An id >= n_scn leaves its env unwritten.
template <int A>
__global__ __launch_bounds__(kBlock) void env_reset_to_kernel(tde_config cfg, tde_world w, tde_state st,
                                                              const uint8_t *__restrict__ mask, const int32_t *__restrict__ scn)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int e = (int)(g / A), a = (int)(g % A);
    if (e >= st.B) return;
    if (mask && !mask[e]) return;
    const int forced = scn ? scn[e] : -1;
    if (forced >= w.n_scn) return;                                   // (per env: the lanes of an env leave together)
    Agent ag;
    EnvRegs er{0, 0, 0, 0, st.episode[e]};
    Cold cold;
    fill_cold(cold, cfg, w);
    reset_lane<A>(cfg, cold, e, a, ag, er, make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), nullptr, forced);
    store_agent_dynamic(st, g, ag);
    store_agent_static(st, g, ag);
    st.collided[g] = 0;
    st.offroad[g] = 0;
    if (a == 0) {
        st.scn[e] = er.scn; st.steps[e] = 0; st.target_idx[e] = 1; st.reached[e] = 0; st.episode[e] = er.episode;
        if (st.ep_return) st.ep_return[e] = 0.0;
    }
}

// a tde_episode_record as the three 16-byte words it is stored with
struct RecordWords {
    double2 w0;                 // ret, psi_sum
    double speed_sum;           // w1: speed_sum | length, reached
    int length, reached;
    int4 w2;                    // scn, bits (byte 0; the padding bytes zero), 0, 0
};

TDE_DEV void store_record(tde_episode_record *dst, const RecordWords &r)
{
    static_assert(sizeof(tde_episode_record) == 48, "a record is three 16-byte words");
    double2 *d = reinterpret_cast<double2 *>(dst);
    d[0] = r.w0;
    d[1] = make_double2(r.speed_sum, __hiloint2double(r.reached, r.length));
    reinterpret_cast<int4 *>(dst)[2] = r.w2;
}

// tde_eval_advance: one wavefront per env, after a step launched WITHOUT TDE_F_AUTORESET.  The fold and the record are lane 0's;
// the re-spawn is env_post_step_kernel's (a lane per slot, two trips at 128 slots, no shuffles) with the planned scenario forced.
// Every value the record and the re-spawn need is read before the first store to the state: a wavefront runs its loads and
// stores in program order, so the counters lane 0 rewrites are the step's for every lane that read them.
template <int A>
__global__ __launch_bounds__(kBlock) void env_eval_advance_kernel(tde_config cfg, tde_world w, tde_state st, tde_eval ev)
{
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    const int e = (int)(blockIdx.x * (kBlock / kWave) + wv);
    if (e >= st.B) return;                                           // (wave-uniform, like every branch below but the slot guards)
    if (!ev.active[e]) return;
    const int B = st.B;
    tde_episode_record *acc = ev.acc + e;
    RecordWords r;
    r.w0 = reinterpret_cast<const double2 *>(acc)[0];
    r.speed_sum = reinterpret_cast<const double *>(acc)[2];
    const double2 inf = reinterpret_cast<const double2 *>(st.info)[2 * (int64_t)e];     // psi_smoothness, speed_smoothness
    r.w0.x = r.w0.x + (double)st.reward[e];
    r.w0.y = r.w0.y + inf.x;
    r.speed_sum = r.speed_sum + inf.y;
    r.length = 0; r.reached = 0;
    r.w2 = make_int4(0, 0, 0, 0);
    if (!(st.terminated[e] | st.truncated[e])) {
        if (lane == 0) store_record(acc, r);
        return;
    }
    r.length = st.steps[e];
    r.reached = st.info_reached[e];
    r.w2.x = st.scn[e];
    r.w2.y = (int)st.done_bits[e];
    const int round = ev.round[e];
    const int episode = st.episode[e];
    // (a round outside [0, R) is a caller's error the host cannot see: nothing is recorded, the env stops evaluating)
    const bool in_range = round >= 0 && round < ev.R;
    int forced = -1;
    if (in_range && round + 1 < ev.R) forced = ev.plan[(int64_t)(round + 1) * B + e];
    const bool next = forced >= 0 && forced < w.n_scn;
    if (lane == 0) {
        if (in_range) {
            store_record(ev.results + ((int64_t)round * B + e), r);
            RecordWords z;
            z.w0 = make_double2(0.0, 0.0); z.speed_sum = 0.0; z.length = 0; z.reached = 0; z.w2 = make_int4(0, 0, 0, 0);
            store_record(acc, z);
            ev.round[e] = round + 1;
        }
        if (!next) ev.active[e] = 0;
    }
    if (!next) return;
    Cold cold;
    fill_cold(cold, cfg, w);
    const int64_t g0 = (int64_t)e * A;
    for (int a0 = 0; a0 < A; a0 += 64) {
        const int a = a0 + lane;
        if (a >= A) continue;
        Agent ag;
        EnvRegs er{0, 0, 0, 0, episode};
        reset_lane<A, false>(cfg, cold, e, a, ag, er, make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0), nullptr, forced);
        const int64_t g = g0 + a;
        store_agent_dynamic(st, g, ag);
        store_agent_static(st, g, ag);
        st.collided[g] = 0;
        st.offroad[g] = 0;
        if (a == 0) {
            st.scn[e] = er.scn; st.steps[e] = 0; st.target_idx[e] = 1; st.reached[e] = 0; st.episode[e] = er.episode;
            if (st.ep_return) st.ep_return[e] = 0.0;
            if (st.obs) {                                            // (env_post_step_kernel's: state_obs_kernel's expression)
                const bool has = 1 < reinterpret_cast<const int4 *>(w.scn)[er.scn].y;
                float fwd = 0.0f, lat = 0.0f;
                if (has) {
                    const double2 t = reinterpret_cast<const double2 *>(w.wp_xy)[(int64_t)er.scn * w.NW + 1];
                    float s, c;
                    sincos_f32(ag.psi, s, c);
                    const float dx = (float)t.x - ag.x, dy = (float)t.y - ag.y;
                    fwd = dx * c + dy * s;
                    lat = dy * c - dx * s;
                }
                float4 *ob = reinterpret_cast<float4 *>(st.obs) + 2 * (int64_t)e;
                ob[0] = make_float4(ag.x, ag.y, ag.psi, ag.v);
                ob[1] = make_float4(fwd, lat, has ? 1.0f : 0.0f, 0.0f);
            }
        }
    }
}

}  // namespace tde
