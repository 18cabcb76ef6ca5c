// tde_rollout_trio.hip — the persistent rollout's three-role kernel (env_rollout_trio_kernel: 8 / 16 / 32 agent slots per env)
// and the two-role kernel for 128 slots (env_rollout_wide_kernel), with their launchers.
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"

namespace tde_host {

int launch_rollout_trio(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_rollout *ro, void *stream)
{
    const unsigned nb = (unsigned)(((int64_t)st->B * st->A + tde::kWave - 1) / tde::kWave);
    const bool lights = (cfg->flags & TDE_F_TRAFFIC_LIGHTS) != 0;
    const bool big = (world->hints & TDE_WORLD_LARGE_GRID) != 0;      // corner classes from the 2-bit class map (tde_abi.h)
    const uint32_t act_hash = act_cfg_hash(*cfg, *world);             // keys the world's first-step gap cache (tde_first_gap)
    const bool served = with_slots<8, 32>(st->A, [&](auto a) {
        with_flags({lights, big}, [&](auto l, auto g) {
            tde::env_rollout_trio_kernel<a.value, l.value, g.value><<<nb, 3 * tde::kWave, 0, (hipStream_t)stream>>>(*cfg, *world, *st, *ro, act_hash);
        });
    });
    if (!served) return bad("tde_env_rollout: the three-role kernel serves 8, 16 or 32 agent slots per env");
    return launch_status("tde_env_rollout");
}

int launch_rollout_wide(const tde_config *cfg, const tde_world *world, const tde_state *st, const tde_rollout *ro, int waves, void *stream)
{
    // two roles, four wavefronts per env of 128 slots (waves = 8: + two sweep helpers and two offroad helpers): one env per workgroup
    const bool lights = (cfg->flags & TDE_F_TRAFFIC_LIGHTS) != 0;
    with_flags({waves == 8, lights}, [&](auto eight, auto l) {
        constexpr int NW = eight.value ? 8 : 4;
        tde::env_rollout_wide_kernel<l.value, NW><<<(unsigned)st->B, NW * tde::kWave, 0, (hipStream_t)stream>>>(*cfg, *world, *st, *ro);
    });
    return launch_status("tde_env_rollout");
}

}  // namespace tde_host
