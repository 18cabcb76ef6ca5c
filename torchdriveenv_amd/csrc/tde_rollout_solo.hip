// tde_rollout_solo.hip — the persistent rollout's one-role kernel (env_rollout_kernel: any slot count; at 128 slots the workgroup
// is the env's two wavefronts) and its launcher.
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"

namespace tde_host {

int launch_rollout_solo(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_rollout *ro, void *stream)
{
    const bool lights = (cfg->flags & TDE_F_TRAFFIC_LIGHTS) != 0;
    with_slots<1, 128>(st->A, [&](auto a) {
        // up to 64 slots: a wavefront per 64 slots of the batch; 128: an env per workgroup
        constexpr int kGroup = a.value > tde::kWave ? a.value : tde::kWave;
        const unsigned nb = (unsigned)(((int64_t)st->B * st->A + kGroup - 1) / kGroup);
        with_flags({lights}, [&](auto l) {
            tde::env_rollout_kernel<a.value, l.value><<<nb, kGroup, 0, (hipStream_t)stream>>>(*cfg, *world, *st, *ro);
        });
    });
    return launch_status("tde_env_rollout");
}

}  // namespace tde_host
