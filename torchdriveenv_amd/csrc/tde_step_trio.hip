// tde_step_trio.hip — the closed-loop step's three-role kernel (env_step_trio_kernel: tde_kernels.h) and its launcher.
#include "tde_kernels.h"
#include "tde_host.h"
#include "tde_launch.h"

namespace tde_host {

int launch_step_trio(const tde_config *cfg, const tde_world *world, const tde_state *st, uint32_t act_hash, void *stream)
{
    const bool lights = (cfg->flags & TDE_F_TRAFFIC_LIGHTS) != 0;
    const unsigned ng = (unsigned)(((int64_t)st->B * st->A + tde::kWave - 1) / tde::kWave);
    const bool served = with_slots<8, 32>(st->A, [&](auto a) {
        with_flags({st->obs != nullptr, lights, st->magnitudes != nullptr}, [&](auto obs, auto l, auto mag) {
            tde::env_step_trio_kernel<a.value, l.value, obs.value, mag.value><<<ng, 3 * tde::kWave, 0, (hipStream_t)stream>>>(*cfg, *world, *st, act_hash);
        });
    });
    if (!served) return bad("tde_env_step: the three-role kernel serves 8, 16 or 32 agent slots per env");
    return launch_status("tde_env_step");
}

}  // namespace tde_host
