// tde_step_driven.hip — the one-role step kernel with outside actions for chosen NPC slots (env_step_driven_kernel: tde_kernels.h) without the infraction magnitudes (MAG = false): this unit instantiates that half of the family (launch_step_one_role: tde_launch.h) and holds the entry point of include/tde_driven.h.
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"
#include "../../include/tde_driven.h"

namespace tde_host {

int launch_step_driven(const tde_config *cfg, const tde_world *world, const tde_state *st, const float *agent_action, const uint8_t *driven, void *stream)
{
    return launch_step_one_role<StepDriven, false>(cfg, world, st, stream, agent_action, driven);
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
    bool run = false;
    if (const int rc = tde_host::check_step_batch("tde_env_step_driven", cfg, world, st, &run)) return rc;
    return run ? tde_host::step_driven(cfg, world, st, agent_action, driven, stream) : 0;
}
