// tde_step_wide8.hip — the closed-loop step's two-role kernel for 128 agent slots per env (env_step_wide_kernel: tde_kernels.h) in its
// eight-wavefront form (drive / drive / judge / judge + two sweep helpers and two offroad helpers per env).  The two forms are two translation units: sixteen
// instantiations of this kernel in one unit were the library's longest compile (49 s of a 60-s build).
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"

namespace tde_host {

int launch_step_wide8(const tde::StepArgs *args, const tde_config *cfg, const tde_state *st, void *stream)
{
    return launch_step_wide_form<8>(args, cfg, st, stream);
}

}  // namespace tde_host
