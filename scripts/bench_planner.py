"""Planner timings: tde_plan_action alone with the default Planner at 8192 x 16 on the junction maps, 8192 x 16 on the 1 km town and
1024 x 128 on the junction maps, next to tde_vector_obs (default VectorObs) and tde_render_ego (64 x 64 birdview) on the same states -
fresh resets and the states 150 steps under the planner's own actions reach; BatchedWaypointEnv.step() alone (zero actions) and
step(plan_actions()) at 8192 x 16 (obs_mode "state", auto-reset).  Prints one JSON line.  Run it under `rocprofv3 --kernel-trace
--stats` for the kernels' own durations (profiles/README.md)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from torchdriveenv_amd import ops  # noqa: E402
from torchdriveenv_amd.config import EnvConfig, Planner, VectorObs  # noqa: E402
from torchdriveenv_amd.env import BatchedWaypointEnv  # noqa: E402
from torchdriveenv_amd.synth import synthetic_town, synthetic_world  # noqa: E402

dev = torch.device("cuda:0")


def time_us(fn, n=50, warm=5):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for _ in range(2):                      # the faster of two timed regions (a host hiccup is not device time)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / n
        best = us if best is None else min(best, us)
    return best


out = {}
pl, vo = Planner(), VectorObs()
junctions16 = synthetic_world(n_scn=64, A=16, seed=0)
junctions128 = synthetic_world(n_scn=16, A=128, seed=1)
town16 = synthetic_town(n_scn=256, A=16, seed=0)
cfg = EnvConfig(seed=3, distance_cutoff=0.25, max_environment_steps=200)

for name, world, B in (("junctions", junctions16, 8192), ("town", town16, 8192), ("junctions", junctions128, 1024)):
    A = world.A
    env = BatchedWaypointEnv(cfg, world, num_envs=B, agents_per_env=A, device=dev, obs_mode="state", planner=pl)
    env.reset()
    rd = torch.from_numpy(vo.ray_directions()).to(dev)
    buf = torch.empty((B, vo.dim), dtype=torch.float32, device=dev)
    img = torch.empty((B, 3, 64, 64), dtype=torch.uint8, device=dev)
    for when in ("reset", "driven"):
        if when == "driven":
            for _ in range(150):
                env.step(env.plan_actions())
        key = f"{name}_{B}x{A}_{when}"
        out[f"plan_action_{key}"] = dict(us=time_us(lambda: env.plan_actions()))
        out[f"vector_obs_{key}"] = dict(us=time_us(lambda: ops.vector_obs(env.tde_cfg, env.dworld, env.state, vo, rd, buf)))
        out[f"render_ego64_{key}"] = dict(us=time_us(lambda: ops.render_ego(env.tde_cfg, env.dworld, env.state, 64, 64, 35.0, 1, img)))
    del env

B = 8192
zero = torch.zeros(B, 2, device=dev)
env = BatchedWaypointEnv(cfg, junctions16, num_envs=B, device=dev, obs_mode="state", planner=pl)
env.reset()
out[f"step_zero_{B}x16"] = dict(us=time_us(lambda: env.step(zero), n=200, warm=20))
env.reset()
out[f"step_plan_actions_{B}x16"] = dict(us=time_us(lambda: env.step(env.plan_actions()), n=200, warm=20))
print(json.dumps(out))
