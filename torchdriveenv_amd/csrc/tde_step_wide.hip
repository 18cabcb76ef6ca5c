// tde_step_wide.hip — the closed-loop step's two-role kernel for 128 agent slots per env (env_step_wide_kernel: tde_kernels.h) in its
// four-wavefront form (drive / drive / judge / judge), and the launcher of both forms.  The two forms are two translation units: sixteen
// instantiations of this kernel in one unit were the library's longest compile (49 s of a 60-s build).
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"

namespace tde_host {

int launch_step_wide(const tde::StepArgs *args, const tde_config *cfg, const tde_state *st, int waves, void *stream)
{
    if (st->A != 128) return bad("tde_env_step: the two-role wide kernel serves 128 agent slots per env");
    if (waves == 8) return launch_step_wide8(args, cfg, st, stream);
    return launch_step_wide_form<4>(args, cfg, st, stream);
}

}  // namespace tde_host
