// tde_step_driven_mag.hip — the one-role step kernel with outside actions for chosen NPC slots (env_step_driven_kernel: tde_kernels.h; tde_env_step_driven) with the infraction magnitudes (MAG = true: tde_state.magnitudes): this unit instantiates that half of the family (launch_step_one_role: tde_launch.h).
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"

namespace tde_host {

int launch_step_driven_mag(const tde_config *cfg, const tde_world *world, const tde_state *st, const float *agent_action, const uint8_t *driven, void *stream)
{
    return launch_step_one_role<StepDriven, true>(cfg, world, st, stream, agent_action, driven);
}

}  // namespace tde_host
