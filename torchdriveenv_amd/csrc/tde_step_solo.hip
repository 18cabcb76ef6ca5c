// tde_step_solo.hip — the one-role step kernel (env_step_kernel: tde_kernels.h) without the infraction magnitudes (MAG = false): this unit instantiates that half of the family through the launcher all one-role families share (launch_step_one_role: tde_launch.h).
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"

namespace tde_host {

int launch_step_solo(const tde_config *cfg, const tde_world *world, const tde_state *st, void *stream)
{
    return launch_step_one_role<StepSolo, false>(cfg, world, st, stream);
}

}  // namespace tde_host
