"""tde_forecast_agents and tde_score_plans_forecast timings: the forecast at 8192 x 16 (T = 32 and 72) on the junction maps and the 1 km
town and at 1024 x 128 (the crowded town); tde_score_plans_forecast next to tde_score_plans at the same (N, K, tail) on the same states (150 steps under
the planner), as a ratio; and BatchedWaypointEnv.step(plan_actions()) at 8192 x 16 under each Planner.predict, without and with the
brake tail.  HIP events around 50 launches per case; prints one JSON line (profiles/forecast_kernel_stats.txt).  `--behaviour`
prints instead the episode statistics of constant / route, each without and with a 40-step tail (512 envs x 400 steps, the rows of
profiles/forecast_behaviour.txt); `--behaviour B STEPS` on a cut-down run."""
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


def behaviour_rows(world, B=512, steps=400, seed=7):
    """(name, episodes, infraction ends, offroad, collision, red light, waypoints per episode) per policy"""
    rows = []
    for name, predict, pr in (("constant", "constant", None), ("route", "route", None), ("constant+tail40", "constant", PlanRefine(rounds=0)),
                              ("route+tail40", "route", PlanRefine(rounds=0))):
        env = BatchedWaypointEnv(EnvConfig(seed=seed, distance_cutoff=0.25, max_environment_steps=200), world, num_envs=B, device=dev,
                                 obs_mode="state", planner=Planner(predict=predict), plan_refine=pr)
        env.reset()
        acc = torch.zeros(6, dtype=torch.float64, device=dev)
        for _ in range(steps):
            env.step(env.plan_actions())
            bits = env.state["done_bits"].to(torch.int64)
            done = ((bits & 3) != 0).double()
            acc += torch.stack([done.sum(), (done * (bits & 1)).sum(), (done * ((bits >> 2) & 1)).sum(), (done * ((bits >> 3) & 1)).sum(),
                                (done * ((bits >> 4) & 1)).sum(), (done * env.state["info_reached"].double()).sum()])
        n, inf, off, col, red, wps = acc.tolist()
        rows.append((name, int(n), int(inf), int(off), int(col), int(red), wps / max(n, 1.0)))
    return rows


if "--behaviour" in sys.argv:
    rest = [a for a in sys.argv[1:] if a != "--behaviour"]
    B, steps = (int(rest[0]), int(rest[1])) if len(rest) >= 2 else (512, 400)
    print(f"{'policy':>16} {'episodes':>9} {'infraction_ends':>16} {'offroad':>8} {'collision':>10} {'red_light':>10} {'waypoints/episode':>18}")
    for name, n, inf, off, col, red, wps in behaviour_rows(synthetic_world(n_scn=8, A=16, seed=0, n_maps=2), B, steps):
        print(f"{name:>16} {n:>9d} {inf:>16d} {off:>8d} {col:>10d} {red:>10d} {wps:>18.3f}", flush=True)
    sys.exit(0)

out = {}
pl = Planner()
lat = np.stack([np.repeat(pl.tables()[0], 7), np.tile(pl.tables()[1], 9)], -1).astype(np.float32)
cfg = EnvConfig(seed=3, distance_cutoff=0.25, max_environment_steps=200)
for name, world, B in (("junctions", synthetic_world(n_scn=64, A=16, seed=0), 8192), ("town", synthetic_town(n_scn=256, A=16, seed=0), 8192),
                       # (128 slots: the crowded town, ~122 slots present per env - a junction map has spawn room for some 20 cars)
                       ("crowded_town", synthetic_town(n_scn=16, A=128, seed=5, n_streets=4, spacing=100.0, ext=160.0, min_gap=3.4), 1024)):
    A = world.A
    env = BatchedWaypointEnv(cfg, world, num_envs=B, agents_per_env=A, device=dev, obs_mode="state", planner=pl)
    env.reset()
    for _ in range(150):                    # the states 150 steps under the planner's own actions reach
        env.step(env.plan_actions())
    key = f"{name}_{B}x{A}"
    fcs = {}
    for T in (32, 72):
        fcs[T] = torch.zeros((B, T, A, 4), dtype=torch.float32, device=dev)
        out[f"forecast_T{T}_{key}"] = dict(us=time_us(lambda: env.forecast_agents(T, out=fcs[T])), bytes=fcs[T].numel() * 4)
    for N, K, tail in ((63, 1, 0), (63, 2, 40), (126, 2, 40)):
        seq = torch.from_numpy(np.tile(lat, (N // 63, 1))).to(dev)[None, :, None, :].expand(B, N, K, 2).contiguous()
        cost = torch.zeros((B, N), dtype=torch.float32, device=dev)
        fail = torch.zeros((B, N), dtype=torch.int32, device=dev)
        act = torch.zeros((B, 2), dtype=torch.float32, device=dev)
        dg = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        knot_len = -(-pl.horizon // K)
        fc = fcs[72 if tail else 32]
        a = time_us(lambda: env._score_plans(seq, knot_len, tail, None, cost, fail, act, dg))
        b = time_us(lambda: env._score_plans(seq, knot_len, tail, None, cost, fail, act, dg, fc))
        out[f"score_plans_N{N}_K{K}_tail{tail}_{key}"] = dict(constant_us=a, forecast_us=b, ratio=b / a)
    del env, fcs

B = 8192
world = synthetic_world(n_scn=64, A=16, seed=0)
for name, predict, pr in (("constant", "constant", None), ("route", "route", None), ("constant_tail40", "constant", PlanRefine(rounds=0)),
                          ("route_tail40", "route", PlanRefine(rounds=0))):
    env = BatchedWaypointEnv(cfg, world, num_envs=B, device=dev, obs_mode="state", planner=Planner(predict=predict), plan_refine=pr)
    env.reset()
    out[f"step_plan_actions_{name}_{B}x16"] = dict(us=time_us(lambda: env.step(env.plan_actions()), n=100, warm=20))
    del env
print(json.dumps(out))
