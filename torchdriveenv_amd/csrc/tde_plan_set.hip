// tde_plan_set.hip — tde_score_plans (include/tde_hip.h): N caller-given knot sequences of (acceleration, steering) per env rolled
// through the step's bicycle and judged by the three predicates of tde_plan_action (tde_planner.hip), then braked to rest through
// a tail that is judged the same way; and its launcher.  One lane per sequence, ceil(N / 64) wavefronts per env.
//   * TEAM = false (N <= 64): one wavefront per env, kPsWaves envs per workgroup, no workgroup barrier - the shape of
//     plan_action_kernel, whose arithmetic this repeats expression for expression (K = 1, tail = 0 and the lattice as sequences
//     give its bits)
//   * TEAM = true (N > 64): one env per workgroup of up to 16 wavefronts; wavefront 0 stages the other agents' rows in LDS once
//     for all, and the winner of each wavefront's butterfly is reduced through LDS by wavefront 0
//   * a lane reads its knot (8 bytes) when the step loop reaches it: one (a, d) pair in registers whatever K is
//   * the red masks of steps 1 .. H + tail <= 96: lane l holds the mask of step l in one register and of step 64 + l in a second
//   * FC = true (tde_score_plans_forecast): the others' boxes of step h come from a caller-given forecast [B][forecast_T][A][4]
//     instead of the constant-velocity line.  What does not change with the step (slot, half extents, reject radius) is staged once
//     as before; the rows of step h are staged PER WAVEFRONT at the top of the step - lane q takes compacted row q (and 64 + q),
//     forms (s, c) = sincos_f32(psi) once for all lanes and writes (x, y, c, s) to its wavefront's own LDS rows - by code every lane
//     of the wavefront still executes (lanes drop out of the judge at their first failure, not out of the staging), so the team
//     form has no workgroup barrier in the step loop either.  The rows of step h + 1 are fetched into registers while step h is judged.
// The specification is restated in numpy by tests/plan_set_ref.py (FC: tests/forecast_ref.py).
#include "tde_kernels.h"
#include "tde_host.h"

namespace tde {

constexpr int kPsWaves = 4;             // envs per workgroup without a team
constexpr int kPsTeamMax = TDE_PLAN_MAX_SET / kWave;
constexpr float kPsSkipMargin = 0.05f;  // metres taken off a coarse tile's clearance (plan_action_kernel's)

struct PsRows {
    float4 box[TDE_MAX_AGENTS];         // the other present agents: x, y, c, s
    float4 mot[TDE_MAX_AGENTS];         //                           (v c) dt, (v s) dt, hl + margin, hw + margin
    float rej2[TDE_MAX_AGENTS];         // a centre distance^2 beyond which the boxes cannot overlap
};

struct PsBest {                         // a wavefront's winner, for the team's second reduction
    uint32_t key;
    int idx, f, n_safe;
    float a1, d1, cost;
};

// class | clearance << 2 of the coarse tile that holds the cell of (px, py) (tde_planner.hip: pl_coarse)
TDE_DEV uint32_t ps_coarse(const tde_world &w, const tde_map &m, float px, float py)
{
    const float fx = __builtin_amdgcn_fmed3f((px - m.ox) * m.inv_cell, 0.0f, (float)(m.nx - 1));
    const float fy = __builtin_amdgcn_fmed3f((py - m.oy) * m.inv_cell, 0.0f, (float)(m.ny - 1));
    static_assert(TDE_COARSE_CELLS == 4, "coarse tiles of 4 x 4 cells");
    const uint32_t cx = (uint32_t)(int)fx >> 2, cy = (uint32_t)(int)fy >> 2;
    const uint32_t line = (uint32_t)m.coarse_base + ((cy >> 3) << (m.row_shift - 6)) + (cx >> 4);
    return w.cell_coarse[(line << 7) | (((cy & 7u) << 4) | (cx & 15u))];
}

TDE_DEV float ps_dist(float wx, float wy, float x, float y)
{
    const float dx = wx - x, dy = wy - y;
    return __builtin_sqrtf(dx * dx + dy * dy);
}

// the least (key, idx) of the wavefront on every lane
TDE_DEV void ps_wave_min(uint32_t &kc, int &ki)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t oc = (uint32_t)__shfl_xor((int)kc, o);
        const int oi = __shfl_xor(ki, o);
        if (oc < kc || (oc == kc && oi < ki)) {
            kc = oc;
            ki = oi;
        }
    }
}

// the one more argument of the FC form (a pack that is empty without it: the other instantiations keep their argument list)
struct PsForecast {
    const float4 *rows;                 // [B][T][A] rows of (x, y, psi, v)
    int T;
};
TDE_DEV PsForecast ps_forecast(const PsForecast &f) { return f; }

template <bool TEAM, typename... Fc>
__global__ __launch_bounds__(TEAM ? kWave * kPsTeamMax : kWave * kPsWaves) void score_plans_kernel(
    tde_config cfg, tde_world w, tde_state st, tde_planner pl, tde_plan_set ps, const uint8_t *only, float *cost_out, int32_t *fail_out,
    float *action, tde_plan_diag *diag, Fc... fc)
{
    static_assert(sizeof...(Fc) <= 1, "at most one PsForecast");
    constexpr bool FC = sizeof...(Fc) == 1;

    __shared__ PsRows shw[TEAM ? 1 : kPsWaves];
    __shared__ PsBest best[TEAM ? kPsTeamMax : 1];
    __shared__ int sh_nb;
    const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int e = TEAM ? (int)blockIdx.x : (int)blockIdx.x * kPsWaves + wv;
    if (e >= st.B || (only && !only[e])) return;             // (TEAM: uniform over the workgroup; else wave-uniform and no barrier below)
    PsRows &sh = shw[TEAM ? 0 : wv];
    const int A = st.A, H = pl.horizon, N = ps.N, K = ps.K, T = ps.tail;
    const int64_t base = (int64_t)e * A;
    const float dt = cfg.dt, thr2 = thr2_of(cfg);
    const int s = st.scn[e];
    const tde_scenario sc = w.scn[s];
    const tde_map m = w.maps[sc.map];
    const int steps = st.steps[e];
    const float hl0 = 0.5f * st.len[base], hw0 = 0.5f * st.wid[base];
    const float inv_lr = 1.0f / st.lr[base];
    const float r0 = __builtin_sqrtf(hl0 * hl0 + hw0 * hw0);

    // ---- the other present agents: rows in LDS (compacted), by the env's first wavefront
    int nb = 0;
    if (!TEAM || wv == 0) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (p * kWave >= A) break;                        // (wave-uniform)
            const int a = p * kWave + lane;
            const bool live = a > 0 && a < A && st.present[base + a] != 0;
            float4 b = make_float4(0.0f, 0.0f, 1.0f, 0.0f), mo = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float rj = 0.0f;
            if (live) {
                const int64_t g = base + a;
                float sa, ca;
                sincos_f32(st.psi[g], sa, ca);
                const float va = st.v[g];
                const float hl = 0.5f * st.len[g] + pl.margin, hw = 0.5f * st.wid[g] + pl.margin;
                b = make_float4(st.x[g], st.y[g], ca, sa);
                mo = make_float4((va * ca) * dt, (va * sa) * dt, hl, hw);
                if constexpr (FC) mo.x = __int_as_float(a);       // (the slot whose forecast rows these are; box and (v c) dt are not read)
                const float rr = (r0 + __builtin_sqrtf(hl * hl + hw * hw)) * 1.001f + 0.01f;   // (conservative: only a shortcut)
                rj = rr * rr;
            }
            const unsigned long long bl = __ballot(live);
            if (live) {
                const int q = nb + lane_prefix(bl);
                sh.box[q] = b;
                sh.mot[q] = mo;
                sh.rej2[q] = rj;
            }
            nb += __popcll(bl);
        }
    }
    if constexpr (TEAM) {
        if (threadIdx.x == 0) sh_nb = nb;
        __syncthreads();
        nb = sh_nb;
    } else {
        wave_lds_fence();
    }

    // ---- the light phases: lane l holds the red mask of step steps + l (red0) and of step steps + 64 + l (red1)
    const bool lights = (cfg.flags & TDE_F_TRAFFIC_LIGHTS) && m.n_stop > 0 && m.cycle_steps > 0;
    const int HT = H + T;
    uint32_t red0 = 0u, red1 = 0u;
    if (lights && lane >= 1 && lane <= HT) red0 = red_mask(w, m, steps + lane);
    if (lights && kWave + lane <= HT) red1 = red_mask(w, m, steps + kWave + lane);

    // ---- one lane per sequence
    const int n = (TEAM ? wv * kWave : 0) + lane;
    const bool active = n < N;
    const float2 *knots = reinterpret_cast<const float2 *>(ps.seq) + ((int64_t)e * N + (active ? n : 0)) * K;
    float a = 0.0f, d = 0.0f, dmax2 = 0.0f;
    if (active) {
        const float2 k0 = knots[0];
        a = fminf(fmaxf(k0.x, -TDE_PLAN_BOX_ACCEL), TDE_PLAN_BOX_ACCEL);
        d = fminf(fmaxf(k0.y, -TDE_PLAN_BOX_STEER), TDE_PLAN_BOX_STEER);
    }
    int kidx = 0, kleft = ps.knot_len;
    float x = st.x[base], y = st.y[base], psi = st.psi[base], v = st.v[base];
    int ti = st.target_idx[e];
    float wx = 0.0f, wy = 0.0f, dp = 0.0f, gain = 0.0f, sv = 0.0f;
    const double2 *wps = reinterpret_cast<const double2 *>(w.wp_xy) + (int64_t)s * w.NW;
    if (ti < sc.wp_n) {
        const double2 t = wps[ti];
        wx = (float)t.x;
        wy = (float)t.y;
        dp = ps_dist(wx, wy, x, y);
    }
    const float rr = (float)cfg.reach_radius;
    const float a1 = (v + a * dt < 0.0f) ? 0.0f : a, d1 = d;
    bool alive = active;
    int f = HT + 1;
    // FC: this wavefront's rows of the step and the forecast rows of the next one (compacted rows lane and 64 + lane)
    float4 *fbox = nullptr;
    float4 fnext[2] = {make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
    int fslot[2] = {0, 0};
    const float4 *frow = nullptr;
    if constexpr (FC) {
        __shared__ float4 fc_box[TEAM ? kPsTeamMax : kPsWaves][TDE_MAX_AGENTS];
        fbox = fc_box[wv];
        const PsForecast fo = ps_forecast(fc...);
        frow = fo.rows + (int64_t)e * fo.T * A;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int q = p * kWave + lane;
            if (q < nb) {
                fslot[p] = __float_as_int(sh.mot[q].x);
                fnext[p] = frow[fslot[p]];
            }
        }
    }
    // steps 1 .. H under the knots, steps H + 1 .. H + T under full braking with the steering of step H
    for (int h = 1; h <= HT; ++h) {
        if (!__ballot(alive)) break;
        if constexpr (FC) {
            // every lane of the wavefront is here, alive or not: stage the others' rows of step h, fetch those of step h + 1
            wave_lds_fence();                                 // (the judge of step h - 1 has read its rows)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const int q = p * kWave + lane;
                if (q < nb) {
                    float sj, cj;
                    sincos_f32(fnext[p].z, sj, cj);
                    fbox[q] = make_float4(fnext[p].x, fnext[p].y, cj, sj);
                    if (h < HT) fnext[p] = frow[(int64_t)h * A + fslot[p]];
                }
            }
            wave_lds_fence();
        }
        const bool tail = h > H;                              // (wave-uniform)
        if (tail) {
            a = -TDE_PLAN_BOX_ACCEL;
            if (alive && v + a * dt < 0.0f) alive = false;   // at rest as far as the action box can brake: safe, f stays H + T + 1
        } else {
            if (kleft == 0) {
                if (kidx < K - 1) {
                    ++kidx;
                    if (alive) {
                        const float2 kn = knots[kidx];
                        a = fminf(fmaxf(kn.x, -TDE_PLAN_BOX_ACCEL), TDE_PLAN_BOX_ACCEL);
                        d = fminf(fmaxf(kn.y, -TDE_PLAN_BOX_STEER), TDE_PLAN_BOX_STEER);
                    }
                }
                kleft = ps.knot_len;
            }
            --kleft;
            if (alive) dmax2 = fmaxf(dmax2, d * d);
        }
        float sn = 0.0f, cs = 1.0f;
        bool need = false;
        if (alive) {
            const float ah = (v + a * dt < 0.0f) ? 0.0f : a;
            bicycle(x, y, psi, v, inv_lr, ah, d, dt);
            sincos_f32(psi, sn, cs);
            // (i) a FULL coarse tile under the centre whose clearance covers the circum-radius proves the four corners on the road
            const uint32_t co = ps_coarse(w, m, x, y);
            need = !((co & 3u) == TDE_CELL_FULL && (float)(co >> 2) * TDE_COARSE_UNIT - kPsSkipMargin >= r0);
        }
        bool fail = box_offroad<true, true>(w, m, need, x, y, cs, sn, hl0, hw0, thr2);   // (by all lanes: offroad_resolve ballots)
        if (alive && !fail) {
            // (ii) the predicted boxes
            const float fh = (float)h;
            for (int j = 0; j < nb; ++j) {
                const float4 b = FC ? fbox[j] : sh.box[j], mo = sh.mot[j];
                const float bx = FC ? b.x : b.x + fh * mo.x, by = FC ? b.y : b.y + fh * mo.y;
                const float ex = bx - x, ey = by - y;
                if (ex * ex + ey * ey > sh.rej2[j]) continue;
                if (obb_overlap(x, y, cs, sn, hl0, hw0, bx, by, b.z, b.w, mo.z, mo.w)) { fail = true; break; }
            }
        }
        if (lights) {
            // (iii) the stop lines that are red at this step (wave-uniform walk)
            const uint32_t red = (uint32_t)__builtin_amdgcn_readlane((int)(h < kWave ? red0 : red1), h & (kWave - 1));
            if (red) {
                for (int q = 0; q < m.n_stop; ++q) {
                    const tde_stopline ln = w.stoplines[m.stop_base + q];
                    if (!((red >> ((uint32_t)ln.light & 31u)) & 1u)) continue;
                    if (alive && !fail && obb_overlap(x, y, cs, sn, hl0, hw0, ln.x, ln.y, ln.c, ln.s, ln.hl, ln.hw)) fail = true;
                }
            }
        }
        if (alive && fail) {
            f = h;
            alive = false;
        }
        if (alive && !tail) {
            if (ti < sc.wp_n) {
                const float dn = ps_dist(wx, wy, x, y);
                gain = gain + (dp - dn);
                dp = dn;
                if (dn < rr) {
                    ti += 1;
                    if (ti < sc.wp_n) {
                        const double2 t = wps[ti];
                        wx = (float)t.x;
                        wy = (float)t.y;
                        dp = ps_dist(wx, wy, x, y);
                    }
                }
            }
            const float ev = v - (ti < sc.wp_n ? pl.v_target : 0.0f);
            sv = sv + ev * ev;
        }
    }
    const float run = (pl.w_speed * sv + pl.w_steer * dmax2) - pl.w_progress * gain;
    const float cost = (float)(HT + 1 - f) * TDE_PLAN_FAIL_UNIT + fminf(fmaxf(run + TDE_PLAN_RUN_BIAS, 0.0f), TDE_PLAN_RUN_MAX);
    if (active) {
        cost_out[(int64_t)e * N + n] = cost;
        fail_out[(int64_t)e * N + n] = f;
    }
    if (!action && !diag) return;                            // (uniform over the launch)

    // ---- the winner: least (ordered cost bits, index)
    const uint32_t cb = __float_as_uint(cost);
    uint32_t kc = active ? ((cb >> 31) ? ~cb : (cb ^ 0x80000000u)) : 0xFFFFFFFFu;
    int ki = active ? n : 0x7FFFFFFF;
    ps_wave_min(kc, ki);
    int n_safe = __popcll(__ballot(active && f == HT + 1));
    const int src = ki & (kWave - 1);                        // (the winner's lane; lane 0's own values when no lane is active)
    float wa = __shfl(a1, src), wd = __shfl(d1, src), wc = __shfl(cost, src);
    int wf = __shfl(f, src);
    if constexpr (TEAM) {
        if (lane == 0) {
            PsBest b;
            b.key = kc; b.idx = ki; b.f = wf; b.n_safe = n_safe; b.a1 = wa; b.d1 = wd; b.cost = wc;
            best[wv] = b;
        }
        __syncthreads();
        if (wv != 0) return;
        const int nw = (int)(blockDim.x >> 6);
        const bool has = lane < nw;
        const PsBest b = best[has ? lane : 0];
        kc = has ? b.key : 0xFFFFFFFFu;
        ki = has ? b.idx : 0x7FFFFFFF;
        int from = lane;
        // (key, idx) decide; `from` rides along: idx is unique over the wavefronts that hold a sequence
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t oc = (uint32_t)__shfl_xor((int)kc, o);
            const int oi = __shfl_xor(ki, o), of = __shfl_xor(from, o);
            if (oc < kc || (oc == kc && oi < ki)) {
                kc = oc;
                ki = oi;
                from = of;
            }
        }
        int ns = has ? b.n_safe : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ns += __shfl_xor(ns, o);
        n_safe = ns;
        wa = __shfl(b.a1, from);
        wd = __shfl(b.d1, from);
        wc = __shfl(b.cost, from);
        wf = __shfl(b.f, from);
    }
    if (lane == 0) {
        if (action) reinterpret_cast<float2 *>(action)[e] = make_float2(wa, wd);
        if (diag) {
            tde_plan_diag o;
            o.winner = ki;
            o.fail_step = wf;
            o.cost = wc;
            o.n_safe = n_safe;
            diag[e] = o;
        }
    }
}

}  // namespace tde

namespace tde_host {

int launch_score_plans(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_planner *pl, const tde_plan_set *ps,
                       const uint8_t *only, float *cost, int32_t *fail_step, float *action, tde_plan_diag *diag, void *stream,
                       const float *forecast, int32_t forecast_T)
{
    if (forecast) {
        const tde::PsForecast fc{reinterpret_cast<const float4 *>(forecast), forecast_T};
        if (ps->N <= tde::kWave) {
            const unsigned nb = (unsigned)((st->B + tde::kPsWaves - 1) / tde::kPsWaves);
            tde::score_plans_kernel<false, tde::PsForecast><<<nb, tde::kWave * tde::kPsWaves, 0, (hipStream_t)stream>>>(
                *cfg, *world, *st, *pl, *ps, only, cost, fail_step, action, diag, fc);
        } else {
            const unsigned nw = (unsigned)((ps->N + tde::kWave - 1) / tde::kWave);
            tde::score_plans_kernel<true, tde::PsForecast><<<(unsigned)st->B, tde::kWave * nw, 0, (hipStream_t)stream>>>(
                *cfg, *world, *st, *pl, *ps, only, cost, fail_step, action, diag, fc);
        }
        return launch_status("tde_score_plans_forecast");
    }
    if (ps->N <= tde::kWave) {
        const unsigned nb = (unsigned)((st->B + tde::kPsWaves - 1) / tde::kPsWaves);
        tde::score_plans_kernel<false><<<nb, tde::kWave * tde::kPsWaves, 0, (hipStream_t)stream>>>(*cfg, *world, *st, *pl, *ps, only, cost,
                                                                                                 fail_step, action, diag);
    } else {
        const unsigned nw = (unsigned)((ps->N + tde::kWave - 1) / tde::kWave);
        tde::score_plans_kernel<true><<<(unsigned)st->B, tde::kWave * nw, 0, (hipStream_t)stream>>>(*cfg, *world, *st, *pl, *ps, only, cost,
                                                                                                  fail_step, action, diag);
    }
    return launch_status("tde_score_plans");
}

}  // namespace tde_host
