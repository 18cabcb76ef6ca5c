// tde_step_solo_mag.hip — the one-role step kernel (env_step_kernel: tde_kernels.h) with the infraction magnitudes (MAG = true: tde_state.magnitudes): this unit instantiates that half of the family (launch_step_one_role: tde_launch.h).
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"

namespace tde_host {

int launch_step_solo_mag(const tde_config *cfg, const tde_world *world, const tde_state *st, void *stream)
{
    return launch_step_one_role<StepSolo, true>(cfg, world, st, stream);
}

}  // namespace tde_host
