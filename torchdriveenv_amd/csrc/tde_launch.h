// tde_launch.h — HOST only: how a unit's launcher turns what a call brings at run time (flags, the slot count) into a kernel
// instantiation, and the step launchers that several units share (tde_step_*.hip).  Include it after tde_kernels.h and tde_host.h.  Nothing
// here is instantiated until a unit calls it: a unit emits exactly the kernels its own calls name.
#pragma once
#include <type_traits>

namespace tde_host {

// run-time flags as template arguments: with_flags({p, q}, f) calls f(std::bool_constant<p>{}, std::bool_constant<q>{}) - one branch
// per flag; inside f, `flag.value` is a constant
template <int N, class F, class... T>
inline void with_flags(const bool (&flags)[N], F &&f, T... t)
{
    if constexpr (sizeof...(T) == N) f(t...);
    else if (flags[sizeof...(T)]) with_flags(flags, f, t..., std::true_type{});
    else with_flags(flags, f, t..., std::false_type{});
}

// a run-time slot count as a template argument: f(std::integral_constant<int, A>{}) for A among the powers of two LO .. HI - the
// bounds say which instantiations the caller's unit holds.  false, and nothing called, for any other A.
template <int LO, int HI, class F>
inline bool with_slots(int A, F &&f)
{
    if (A == LO) { f(std::integral_constant<int, LO>{}); return true; }
    if constexpr (LO < HI) return with_slots<2 * LO, HI>(A, f);
    else return false;
}

// ---- the one-role step kernels: env_step_kernel, env_step_routed_kernel, env_step_driven_kernel (tde_kernels.h) ----------------
// A family = the kernel template, the smallest slot count it is instantiated for and the entry point launch_status names.
struct StepSolo {
    template <int A, bool L, bool O, bool G, int W, bool M> static constexpr auto kernel = &tde::env_step_kernel<A, L, O, G, W, M>;
    static constexpr int kMinSlots = 1;
    static constexpr const char *kEntry = "tde_env_step";
};
struct StepRouted {                                     // (tde_env_step has refused fewer than 4 slots per env)
    template <int A, bool L, bool O, bool G, int W, bool M> static constexpr auto kernel = &tde::env_step_routed_kernel<A, L, O, G, W, M>;
    static constexpr int kMinSlots = 4;
    static constexpr const char *kEntry = "tde_env_step";
};
struct StepDriven {
    template <int A, bool L, bool O, bool G, int W, bool M> static constexpr auto kernel = &tde::env_step_driven_kernel<A, L, O, G, W, M>;
    static constexpr int kMinSlots = 1;
    static constexpr const char *kEntry = "tde_env_step_driven";
};

// The choice of form and the (lights, obs) fan-out of every one-role step launch.  `extra` = what the family's kernel takes after
// done_bits: nothing, or (agent_action, driven).  A unit instantiates one MAG half of one family (the split is for compile time).
template <class Family, bool MAG, class... Extra>
int launch_step_one_role(const tde_config *cfg, const tde_world *world, const tde_state *st, void *stream, Extra... extra)
{
    const bool lights = (cfg->flags & TDE_F_TRAFFIC_LIGHTS) != 0;
    const unsigned nb = (unsigned)(((int64_t)st->B * st->A + tde::kBlock - 1) / tde::kBlock);
    const auto launch = [&](auto a, auto big, auto waves) {
        with_flags({st->obs != nullptr, lights}, [&](auto obs, auto l) {
            Family::template kernel<a.value, l.value, obs.value, big.value, waves.value, MAG><<<nb, tde::kBlock, 0, (hipStream_t)stream>>>(
                *cfg, *world, *st, st->action, (float *)nullptr, st->done_bits, extra...);
        });
    };
    constexpr std::integral_constant<int, TDE_WIDE_WAVES> usual_waves{};
    if ((world->hints & TDE_WORLD_LARGE_GRID) && (st->A == 32 || st->A == 64)) {      // (up to 16 slots per env the class map is read anyway)
        with_slots<32, 64>(st->A, [&](auto a) { launch(a, std::true_type{}, usual_waves); });
    } else if (st->A == 128 && st->B > 6 * cu_count()) {   // (128 slots, more than a residency round of the 3-per-SIMD form: 4 per SIMD)
        launch(std::integral_constant<int, 128>{}, std::false_type{}, std::integral_constant<int, 4>{});
    } else {
        with_slots<Family::kMinSlots, 128>(st->A, [&](auto a) { launch(a, std::false_type{}, usual_waves); });
    }
    return launch_status(Family::kEntry);
}

// ---- the two-role step kernel for 128 slots per env (env_step_wide_kernel) in its NW-wavefront form: NW = 4 and NW = 8 are two units
template <int NW>
int launch_step_wide_form(const tde::StepArgs *args, const tde_config *cfg, const tde_state *st, void *stream)
{
    const bool lights = (cfg->flags & TDE_F_TRAFFIC_LIGHTS) != 0;
    with_flags({st->obs != nullptr, lights, st->magnitudes != nullptr}, [&](auto obs, auto l, auto mag) {
        tde::env_step_wide_kernel<l.value, obs.value, mag.value, NW><<<(unsigned)st->B, NW * tde::kWave, 0, (hipStream_t)stream>>>(args, st->action);
    });
    return launch_status("tde_env_step");
}

}  // namespace tde_host
