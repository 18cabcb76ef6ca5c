"""Near-field spawner timings: BatchedWaypointEnv.step() (obs_mode "state", auto-reset, 40-step episodes) with and without
near_field at 8192 x 16 and 1024 x 128 envs on the first validation case, and tde_near_field_spawn alone on the same worlds and on a
town (lattice candidates) with 0 %, 2 % and 100 % of the envs masked.  Prints one JSON line.  --routes: only the closed-loop step, the
unrouted near field (role-split step forms) against NearField(routes=True) (routed one-role form), alternated in one process, five
timed regions each (median and spread).  Run it under
`rocprofv3 --kernel-trace --stats` for the kernels' own durations (profiles/README.md)."""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import near_field_ref as R  # noqa: E402
from torchdriveenv_amd import _abi, ops  # noqa: E402
from torchdriveenv_amd.config import EnvConfig, NearField  # noqa: E402
from torchdriveenv_amd.env import BatchedWaypointEnv, world_from_waypoint_suite  # noqa: E402
from torchdriveenv_amd.state import EnvState  # noqa: E402

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
d = tempfile.mkdtemp()
if "--routes" in sys.argv[1:]:
    for B, A in ((8192, 16), (1024, 128)):
        cfg = EnvConfig(seed=3, distance_cutoff=0.25, max_environment_steps=40, use_background_traffic=False)
        g = torch.Generator().manual_seed(0)
        acts = torch.stack([torch.rand(64, B, generator=g) * 1.2 - 0.2, torch.rand(64, B, generator=g) * 0.2 - 0.1], -1).to(dev)
        envs = {}
        for name, nf in (("unrouted", NearField()), ("routed", NearField(routes=True))):
            world, tab = R.validation_world(0, A, d, nf=nf)
            envs[name] = BatchedWaypointEnv(cfg, world, num_envs=B, device=dev, obs_mode="state", near_field=tab)
            envs[name].reset()
        times = {name: [] for name in envs}
        k = [0]
        for rep in range(5):                                  # alternated: both forms see the same clocks and neighbours
            for name, env in envs.items():
                def step():
                    env.step(acts[k[0] % 64])
                    k[0] += 1
                times[name].append(time_us(step, n=200, warm=20))
        for name, t in times.items():
            out[f"step_{B}x{A}_{name}"] = dict(us_median=float(np.median(t)), us_min=min(t), us_max=max(t))
    print(json.dumps(out))
    sys.exit(0)
worlds = {A: R.validation_world(0, A, d) for A in (16, 128)}
data, meshes, field = R.town_suite(n_scn=2, n_streets=4)
worlds["town128"] = world_from_waypoint_suite(data, agents_per_env=128, road_meshes=meshes, start_headings=field, near_field=NearField(),
                                              near_field_seed=3)

# closed-loop step with and without the near field
for B, A in ((8192, 16), (1024, 128)):
    world, tab = worlds[A]
    cfg = EnvConfig(seed=3, distance_cutoff=0.25, max_environment_steps=40, use_background_traffic=False)
    g = torch.Generator().manual_seed(0)
    acts = torch.stack([torch.rand(64, B, generator=g) * 1.2 - 0.2, torch.rand(64, B, generator=g) * 0.2 - 0.1], -1).to(dev)
    for nf in (None, tab):
        env = BatchedWaypointEnv(cfg, world, num_envs=B, device=dev, obs_mode="state", near_field=nf)
        env.reset()
        k = [0]

        def step():
            env.step(acts[k[0] % 64])
            k[0] += 1
        out[f"step_{B}x{A}_" + ("near_field" if nf is not None else "plain")] = dict(us=time_us(step, n=200, warm=20))
        del env

# the spawner alone (after a reset), by share of envs masked
for name, B, key in (("val16", 8192, 16), ("val128", 1024, 128), ("town128", 1024, "town128")):
    world, tab = worlds[key]
    A = world.A
    cfg = _abi.default_config(seed=5)
    dw, dnf = world.to_device(dev, first_gap=False), tab.to_device(dev)
    st = EnvState(B, A, device=dev, with_info=False)
    ops.env_reset(cfg, dw, st)
    base = {k: v.clone() for k, v in st.arrays.items() if v is not None}
    rng = np.random.default_rng(0)
    for share in (0.0, 0.02, 1.0):
        mask = torch.from_numpy((rng.random(B) < share).astype(np.uint8)).to(dev)

        def spawn():
            ops.near_field_spawn(cfg, dw, st, dnf, mask)
        us = time_us(spawn)                 # (re-spawning on a filled state: T = 0 after the first call)
        for k_, v in base.items():
            st.arrays[k_].copy_(v)
        torch.cuda.synchronize()

        def fresh():
            st["present"].copy_(base["present"])
            ops.near_field_spawn(cfg, dw, st, dnf, mask)
        us_fill = time_us(fresh)
        out[f"spawn_{name}_{B}x{A}_mask{int(share * 100)}pct"] = dict(us_refill=us_fill, us_filled_state=us,
                                                                       n_cand=int(tab.n_cand.max()))
print(json.dumps(out))
