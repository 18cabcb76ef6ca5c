// tde_step_routed.hip — the one-role step kernel with per-slot routes (env_step_routed_kernel: tde_kernels.h; tde_state.slot_route != NULL) without the infraction magnitudes (MAG = false): this unit instantiates that half of the family, from 4 slots per env up (launch_step_one_role: tde_launch.h).
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"

namespace tde_host {

int launch_step_routed(const tde_config *cfg, const tde_world *world, const tde_state *st, void *stream)
{
    return launch_step_one_role<StepRouted, false>(cfg, world, st, stream);
}

}  // namespace tde_host
