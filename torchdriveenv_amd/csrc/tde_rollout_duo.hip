// tde_rollout_duo.hip — the persistent rollout's two-role kernel (env_rollout_duo_kernel: up to 64 agent slots per env) and its launcher.
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"

namespace tde_host {

int launch_rollout_duo(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_rollout *ro, void *stream)
{
    const unsigned nb = (unsigned)(((int64_t)st->B * st->A + tde::kWave - 1) / tde::kWave);
    const bool lights = (cfg->flags & TDE_F_TRAFFIC_LIGHTS) != 0;
    const bool big = (world->hints & TDE_WORLD_LARGE_GRID) != 0;      // corner classes from the 2-bit class map (tde_abi.h)
    const uint32_t act_hash = act_cfg_hash(*cfg, *world);             // keys the world's first-step gap cache (tde_first_gap)
    with_flags({lights, big}, [&](auto l, auto g) {
        with_slots<1, 64>(st->A, [&](auto a) {
            tde::env_rollout_duo_kernel<a.value, l.value, g.value><<<nb, 2 * tde::kWave, 0, (hipStream_t)stream>>>(*cfg, *world, *st, *ro, act_hash);
        });
    });
    return launch_status("tde_env_rollout");
}

}  // namespace tde_host
