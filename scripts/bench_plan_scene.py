"""tde_score_plans_scene timings against the existing code doing the same job - the state replicated N times with torch, then
tde_forecast_scene under every sequence's effective actions, then tde_score_plans_forecast with one sequence per replicated env - on
the same states (150 steps under the planner after a reset): 512 x 16 and 64 x 128 (the crowded town) with N = 63, (H, tail) = (32, 40),
the two ALTERNATED (composition, scene, composition, scene, ...: five samples each, the median of each); the new call alone at
8192 x 16 x 63 (the composition's forecast would be 9.5 GB there); and BatchedWaypointEnv.step(plan_actions()) at 8192 x 16 under
PlanReact against Planner(predict="queue"), each without and with the 40-step brake tail.  HIP events around 10 launches per sample;
prints one JSON line (profiles/plan_scene_kernel_stats.txt).  `--behaviour` prints instead the episode statistics of queue and react,
each without and with a 40-step tail (512 envs x 400 steps, seed 7: the rows of profiles/plan_scene_behaviour.txt); `--behaviour B
STEPS` on a cut-down run."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from torchdriveenv_amd import _abi, ops  # noqa: E402
from torchdriveenv_amd.config import EnvConfig, Planner, PlanReact, PlanRefine  # noqa: E402
from torchdriveenv_amd.env import BatchedWaypointEnv  # noqa: E402
from torchdriveenv_amd.state import EnvState  # noqa: E402
from torchdriveenv_amd.synth import synthetic_town, synthetic_world  # noqa: E402

dev = torch.device("cuda:0")
H, TAIL, N = 32, 40, 63
POLICIES = (("queue", dict(planner=Planner(predict="queue"))), ("react", dict(planner=Planner(), plan_react=PlanReact(tail=0))),
            ("queue+tail40", dict(planner=Planner(predict="queue"), plan_refine=PlanRefine(rounds=0))),
            ("react+tail40", dict(planner=Planner(), plan_react=PlanReact(tail=40))))


def sample_us(fn, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def alternated(fns, rounds, n=10, warm=3):
    """{name: fn} -> {name: (median us, [samples])}: warm-up of each, then `rounds` passes over the functions in order"""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            got[k].append(sample_us(fn, n))
    return {k: (statistics.median(v), v) for k, v in got.items()}


def behaviour_rows(world, B=512, steps=400, seed=7):
    """(name, episodes, infraction ends, offroad, collision, red light, waypoints per episode) per policy"""
    rows = []
    for name, kw in POLICIES:
        env = BatchedWaypointEnv(EnvConfig(seed=seed, distance_cutoff=0.25, max_environment_steps=200), world, num_envs=B, device=dev,
                                 obs_mode="state", **kw)
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


def effective_actions(env, seq, tail):
    """[B * N, H + tail, 2] on the device: every sequence's clamped knot actions after the no-reverse rule, then (-1, d_H) until it
    stands - the ego alone, stepped with torch (timing input: the composition's forecast kernel takes any actions)"""
    B, n, K = seq.shape[:3]
    v = env.state["v"].view(B, env.A)[:, 0].repeat_interleave(n).clone()
    dt = float(env.tde_cfg.dt)
    L = -(-H // K)
    ea = torch.zeros((B * n, H + tail, 2), dtype=torch.float32, device=dev)
    s = seq.view(B * n, K, 2)
    for h in range(1, H + tail + 1):
        k = min((h - 1) // L, K - 1)
        a = s[:, k, 0].clamp(-1.0, 1.0) if h <= H else torch.full_like(v, -1.0)
        a = torch.where(v + a * dt < 0, torch.zeros_like(a), a)
        ea[:, h - 1, 0], ea[:, h - 1, 1] = a, s[:, min(k, K - 1), 1].clamp(-0.3, 0.3)
        v = v + a * dt
    return ea


out = {}
pl = Planner()
cfg = EnvConfig(seed=3, distance_cutoff=0.25, max_environment_steps=200)
for name, world, B, compose in (("junctions", synthetic_world(n_scn=64, A=16, seed=0), 512, True),
                                ("crowded_town", synthetic_town(n_scn=16, A=128, seed=5, n_streets=4, spacing=100.0, ext=160.0, min_gap=3.4), 64, True),
                                ("junctions", synthetic_world(n_scn=64, A=16, seed=0), 8192, False)):
    A = world.A
    env = BatchedWaypointEnv(cfg, world, num_envs=B, agents_per_env=A, device=dev, obs_mode="state", planner=pl)
    env.reset()
    for _ in range(150):                    # the states 150 steps under the planner's own actions reach
        env.step(env.plan_actions())
    seq = torch.stack([torch.empty((B, N, 2), device=dev).uniform_(-1.0, 1.0), torch.empty((B, N, 2), device=dev).uniform_(-0.3, 0.3)], -1).contiguous()
    cost, fail = torch.zeros((B, N), dtype=torch.float32, device=dev), torch.zeros((B, N), dtype=torch.int32, device=dev)
    fns = {"scene": lambda: ops.score_plans_scene(env.tde_cfg, env.dworld, env.state, pl, seq, None, TAIL, None, cost, fail)}
    key = f"{name}_{B}x{A}x{N}"
    if compose:
        big = EnvState(B * N, A, device=dev)
        ea = effective_actions(env, seq, TAIL)
        fc = torch.zeros((B * N, H + TAIL, A, 4), dtype=torch.float32, device=dev)
        c1, f1 = torch.zeros((B * N, 1), dtype=torch.float32, device=dev), torch.zeros((B * N, 1), dtype=torch.int32, device=dev)
        seq1 = seq.view(B * N, 1, 2, 2)

        def composition():
            for k in _abi.STATE_AGENT_F32 + _abi.STATE_AGENT_I32 + _abi.STATE_AGENT_U8 + _abi.STATE_ENV_I32:       # what the kernels read
                a = env.state.arrays[k]
                big.arrays[k].copy_(a.reshape(B, -1).repeat_interleave(N, dim=0).reshape(big.arrays[k].shape))
            ops.forecast_scene(env.tde_cfg, env.dworld, big, H + TAIL, ea, None, fc)
            ops.score_plans(env.tde_cfg, env.dworld, big, pl, seq1, None, TAIL, None, c1, f1, forecast=fc)

        fns = {"composition": composition, **fns}
    r = alternated(fns, rounds=5)
    out[key] = {f"{k}_us": v[0] for k, v in r.items()}
    out[key].update({f"{k}_samples": v[1] for k, v in r.items()})
    if compose:
        out[key]["ratio_scene_over_composition"] = r["scene"][0] / r["composition"][0]
        out[key]["forecast_bytes"] = fc.numel() * 4
        out[key]["same_fail_steps"] = bool(torch.equal(fail.view(-1), f1.view(-1)))
        del big, fc, ea
    print(f"# {key}", out[key], file=sys.stderr, flush=True)
    del env

B = 8192
world = synthetic_world(n_scn=64, A=16, seed=0)
envs = {}
for name, kw in POLICIES:
    envs[name] = BatchedWaypointEnv(cfg, world, num_envs=B, device=dev, obs_mode="state", **kw)
    envs[name].reset()
r = alternated({k: (lambda e=e: e.step(e.plan_actions())) for k, e in envs.items()}, rounds=3, n=50, warm=10)
for k, (med, samples) in r.items():
    out[f"step_plan_actions_{k}_{B}x16"] = dict(us=med, samples=samples)
print(json.dumps(out))
