"""tde_score_plans timings next to tde_plan_action on the same states: 8192 x 16 on the junction maps and on the 1 km town, 1024 x 128
on the junction maps, for (N = 63, K = 1, tail = 0) - the lattice as sequences, the planner's own work -, (N = 63, K = 2, tail = 40)
and (N = 126, K = 2, tail = 40); and BatchedWaypointEnv.step(plan_actions()) at 8192 x 16 without and with the default PlanRefine
(obs_mode "state", auto-reset).  HIP events around 50 launches per case; prints one JSON line.  Run it under `rocprofv3
--kernel-trace --stats` for the kernels' own durations (profiles/README.md).  `--behaviour` prints instead the episode statistics of
the plain planner, the tail only and the default PlanRefine (512 envs x 400 steps, the rows of profiles/plan_refine_behaviour.txt)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torchdriveenv_amd.config import EnvConfig, Planner, PlanRefine  # noqa: E402
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


def behaviour():
    world = synthetic_world(n_scn=8, A=16, seed=0, n_maps=2)
    print(f"{'policy':>8} {'episodes':>9} {'infraction_ends':>16} {'offroad':>8} {'collision':>10} {'red_light':>10} {'waypoints/episode':>18}")
    for name, pr in (("planner", None), ("tail", PlanRefine(rounds=0)), ("refined", PlanRefine())):
        env = BatchedWaypointEnv(EnvConfig(seed=7, distance_cutoff=0.25, max_environment_steps=200), world, num_envs=512, device=dev,
                                 obs_mode="state", planner=Planner(), plan_refine=pr)
        env.reset()
        acc = torch.zeros(6, dtype=torch.float64, device=dev)
        for _ in range(400):
            env.step(env.plan_actions())
            bits = env.state["done_bits"].to(torch.int64)
            done = ((bits & 3) != 0).double()
            acc += torch.stack([done.sum(), (done * (bits & 1)).sum(), (done * ((bits >> 2) & 1)).sum(), (done * ((bits >> 3) & 1)).sum(),
                                (done * ((bits >> 4) & 1)).sum(), (done * env.state["info_reached"].double()).sum()])
        n, inf, off, col, red, wps = acc.tolist()
        print(f"{name:>8} {int(n):>9d} {int(inf):>16d} {int(off):>8d} {int(col):>10d} {int(red):>10d} {wps / max(n, 1.0):>18.3f}")


if "--behaviour" in sys.argv:
    behaviour()
    sys.exit(0)

out = {}
pl = Planner()
lat = np.stack([np.repeat(pl.tables()[0], 7), np.tile(pl.tables()[1], 9)], -1).astype(np.float32)
cfg = EnvConfig(seed=3, distance_cutoff=0.25, max_environment_steps=200)
for name, world, B in (("junctions", synthetic_world(n_scn=64, A=16, seed=0), 8192), ("town", synthetic_town(n_scn=256, A=16, seed=0), 8192),
                       ("junctions", synthetic_world(n_scn=16, A=128, seed=1), 1024)):
    A = world.A
    env = BatchedWaypointEnv(cfg, world, num_envs=B, agents_per_env=A, device=dev, obs_mode="state", planner=pl)
    env.reset()
    for _ in range(150):                    # the states 150 steps under the planner's own actions reach
        env.step(env.plan_actions())
    key = f"{name}_{B}x{A}"
    out[f"plan_action_{key}"] = dict(us=time_us(lambda: env.plan_actions()))
    for N, K, tail in ((63, 1, 0), (63, 2, 40), (126, 2, 40)):
        seq = torch.from_numpy(np.tile(lat, (N // 63, 1))).to(dev)[None, :, None, :].expand(B, N, K, 2).contiguous()
        cost = torch.zeros((B, N), dtype=torch.float32, device=dev)
        fail = torch.zeros((B, N), dtype=torch.int32, device=dev)
        act = torch.zeros((B, 2), dtype=torch.float32, device=dev)
        dg = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        knot_len = -(-pl.horizon // K)
        out[f"score_plans_N{N}_K{K}_tail{tail}_{key}"] = dict(us=time_us(lambda: env._score_plans(seq, knot_len, tail, None, cost, fail, act, dg)))
    del env

B = 8192
world = synthetic_world(n_scn=64, A=16, seed=0)
for name, pr in (("plain", None), ("refined", PlanRefine())):
    env = BatchedWaypointEnv(cfg, world, num_envs=B, device=dev, obs_mode="state", planner=pl, plan_refine=pr)
    env.reset()
    out[f"step_plan_actions_{name}_{B}x16"] = dict(us=time_us(lambda: env.step(env.plan_actions()), n=100, warm=20))
print(json.dumps(out))
