"""Vector-observation timings: tde_vector_obs alone with the default VectorObs at 8192 x 16 on the junction maps, 8192 x 16 on the
1 km town and 1024 x 128 on the junction maps, next to tde_render_ego (64 x 64 birdview) on the same states; BatchedWaypointEnv.step()
for each obs mode at 8192 x 16 (auto-reset, 40-step episodes); the WaypointVecEnv numpy step for "state" and "vector".  Prints one
JSON line.  Run it under `rocprofv3 --kernel-trace --stats` for the kernels' own durations (profiles/README.md)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torchdriveenv_amd import _abi, ops  # noqa: E402
from torchdriveenv_amd.config import EnvConfig, VectorObs  # noqa: E402
from torchdriveenv_amd.env import BatchedWaypointEnv  # noqa: E402
from torchdriveenv_amd.state import EnvState  # noqa: E402
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
vo = VectorObs()
junctions16 = synthetic_world(n_scn=64, A=16, seed=0)
junctions128 = synthetic_world(n_scn=16, A=128, seed=1)
town16 = synthetic_town(n_scn=256, A=16, seed=0)

# the kernel alone, on the states a reset leaves, next to the birdview rasteriser
for name, world, B in (("junctions", junctions16, 8192), ("town", town16, 8192), ("junctions", junctions128, 1024)):
    A = world.A
    cfg = _abi.default_config(seed=5)
    if world.has_lights:
        cfg.flags |= _abi.F_TRAFFIC_LIGHTS
    dw = world.to_device(dev)
    st = EnvState(B, A, device=dev, with_info=False)
    ops.env_reset(cfg, dw, st)
    rd = torch.from_numpy(vo.ray_directions()).to(dev)
    buf = torch.empty((B, vo.dim), dtype=torch.float32, device=dev)
    img = torch.empty((B, 3, 64, 64), dtype=torch.uint8, device=dev)
    out[f"vector_obs_{name}_{B}x{A}"] = dict(us=time_us(lambda: ops.vector_obs(cfg, dw, st, vo, rd, buf)), dim=vo.dim)
    out[f"render_ego64_{name}_{B}x{A}"] = dict(us=time_us(lambda: ops.render_ego(cfg, dw, st, 64, 64, 35.0, 1, img)))
    del dw, st

# BatchedWaypointEnv.step() per obs mode, and the VecEnv's numpy step
B = 8192
cfg = EnvConfig(seed=3, distance_cutoff=0.25, max_environment_steps=40)
g = torch.Generator().manual_seed(0)
acts = torch.stack([torch.rand(64, B, generator=g) * 1.2 - 0.2, torch.rand(64, B, generator=g) * 0.2 - 0.1], -1).to(dev)
for mode in ("birdview", "state", "vector"):
    env = BatchedWaypointEnv(cfg, junctions16, num_envs=B, device=dev, obs_mode=mode)
    env.reset()
    k = [0]

    def step():
        env.step(acts[k[0] % 64])
        k[0] += 1
    out[f"step_{mode}_{B}x16"] = dict(us=time_us(step, n=200, warm=20))
    if mode != "birdview":
        venv = env.as_vec_env(copy_obs=False)
        venv.reset()
        a_np = acts.cpu().numpy()

        def vstep():
            venv.step(a_np[k[0] % 64])
            k[0] += 1
        out[f"vecenv_step_{mode}_{B}x16"] = dict(us=time_us(vstep, n=100, warm=10))
    del env
print(json.dumps(out))
