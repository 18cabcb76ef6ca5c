// tde_step_driven.hip — the one-role step kernel with outside actions for chosen NPC slots (env_step_driven_kernel: tde_kernels.h) without the infraction magnitudes (MAG = false), its launcher - the forms and the choice among them are launch_step_solo's - and the entry point of include/tde_driven.h.
#include "tde_kernels.h"
#include "tde_host.h"
#include "../../include/tde_driven.h"

namespace tde_host {

int launch_step_driven(const tde_config *cfg, const tde_world *world, const tde_state *st, const float *agent_action,
                       const uint8_t *driven, void *stream)
{
    constexpr bool kMag = false;
    const bool lights = (cfg->flags & TDE_F_TRAFFIC_LIGHTS) != 0;
    const unsigned nb = (unsigned)(((int64_t)st->B * st->A + tde::kBlock - 1) / tde::kBlock);
#define TDE_LAUNCH_FORM(AA, L, O, G, W) \
    tde::env_step_driven_kernel<AA, L, O, G, W, kMag><<<nb, tde::kBlock, 0, (hipStream_t)stream>>>(*cfg, *world, *st, st->action, (float *)nullptr, st->done_bits, agent_action, driven)
#define TDE_LAUNCH_LO(AA, G, W)                                                                                            \
    if (st->obs) { if (lights) TDE_LAUNCH_FORM(AA, true, true, G, W); else TDE_LAUNCH_FORM(AA, false, true, G, W); }       \
    else { if (lights) TDE_LAUNCH_FORM(AA, true, false, G, W); else TDE_LAUNCH_FORM(AA, false, false, G, W); }
    if ((world->hints & TDE_WORLD_LARGE_GRID) && (st->A == 32 || st->A == 64)) {      // (up to 16 slots per env the class map is read anyway)
        if (st->A == 32) { TDE_LAUNCH_LO(32, true, TDE_WIDE_WAVES) } else { TDE_LAUNCH_LO(64, true, TDE_WIDE_WAVES) }
    } else if (st->A == 128 && st->B > 6 * cu_count()) {   // (128 slots, more than a residency round of the 3-per-SIMD form: 4 per SIMD)
        TDE_LAUNCH_LO(128, false, 4)
    } else {
        TDE_DISPATCH_A128(st->A, TDE_LAUNCH_LO(kA, false, TDE_WIDE_WAVES));
    }
#undef TDE_LAUNCH_LO
#undef TDE_LAUNCH_FORM
    return launch_status("tde_env_step_driven");
}

}  // namespace tde_host

int tde_driven_version(void) { return TDE_DRIVEN_VERSION; }

// Always the driven one-role kernel, by value: no tde_kernel_override, no lookup caches read or written (the kernel invalidates the
// act cache's key), no argument-block pool at 128 slots - nothing is allocated or uploaded, so the call can be captured in a graph.
int tde_env_step_driven(const tde_config *cfg, const tde_world *world, const tde_state *st, const float *agent_action,
                        const uint8_t *driven, void *stream)
{
    using tde_host::bad;
    if (const int rc = tde_host::check_env_args("tde_env_step_driven", cfg, world, st)) return rc;
    if (driven && !agent_action) return bad("tde_env_step_driven: driven is set and agent_action is NULL");
    if (st->slot_route)
        return bad("tde_env_step_driven: state.slot_route is set: routes of near-field agents and outside actions do not combine yet (step such a state with tde_env_step)");
    if (st->B <= 0) return 0;
    if (!st->action) return bad("tde_env_step_driven: state.action is NULL");
    if ((cfg->flags & TDE_F_OFFROAD) && !world->cell_cls2) return bad("tde_env_step_driven: world.cell_cls2 is NULL (ABI 7 class map)");
    return st->magnitudes ? tde_host::launch_step_driven_mag(cfg, world, st, agent_action, driven, stream)
                          : tde_host::launch_step_driven(cfg, world, st, agent_action, driven, stream);
}
