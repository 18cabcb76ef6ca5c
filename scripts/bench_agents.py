"""tde_agent_obs timings: 8192 pairs - slot 1 of every env - at 8192 envs x 16 slots on the junction maps with the default VectorObs,
next to (a) tde_vector_obs on the same state (the same work per row: one box and one index load less) and (b) the torch composition
the call replaces: rows 0 and 1 of a copy of the state swapped with torch ops, then tde_vector_obs on the copy; and, to tell the kernel
from the scene, tde_agent_obs for slot 0 of every env, whose rows are tde_vector_obs's (the same observers), with and without the track.  Device-event time per
call over `--calls` calls, the variants alternating inside each of `--rounds` rounds; per variant the median, the minimum and the
maximum over the rounds (the spread).  Also checks that (b)'s neighbour and ray blocks are agent_obs's.  Prints one JSON line;
profiles/agent_obs.txt keeps a run."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torchdriveenv_amd import _abi, ops  # noqa: E402
from torchdriveenv_amd.config import VectorObs  # noqa: E402
from torchdriveenv_amd.state import EnvState  # noqa: E402
from torchdriveenv_amd.synth import synthetic_world  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=8192)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--rounds", type=int, default=7)
args = ap.parse_args()

dev = torch.device("cuda:0")
B, A = args.envs, 16
vo = VectorObs()
world = synthetic_world(n_scn=64, A=A, seed=0)
cfg = _abi.default_config(seed=5)
if world.has_lights:
    cfg.flags |= _abi.F_TRAFFIC_LIGHTS
dw = world.to_device(dev)
st = EnvState(B, A, device=dev, with_info=False)
ops.env_reset(cfg, dw, st)
for _ in range(10):                                   # a state in motion, not the spawn poses
    ops.env_step(cfg, dw, st, action=torch.zeros(B, 2, device=dev))
copy = EnvState(B, A, device=dev, with_info=False)
rd = torch.from_numpy(vo.ray_directions()).to(dev)
pairs = torch.stack([torch.arange(B, dtype=torch.int32), torch.ones(B, dtype=torch.int32)], -1).contiguous().to(dev)
pairs0 = torch.stack([torch.arange(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)], -1).contiguous().to(dev)
rows_0 = torch.empty((B, vo.dim), dtype=torch.float32, device=dev)
rows_a = torch.empty((B, vo.dim), dtype=torch.float32, device=dev)
rows_v = torch.empty_like(rows_a)
rows_s = torch.empty_like(rows_a)
track = torch.empty((B, 32), dtype=torch.uint8, device=dev)
SWAPPED = ("x", "y", "psi", "v", "len", "wid", "present")
COPIED = SWAPPED + ("scn", "steps", "target_idx")


def agent_obs():
    ops.agent_obs(cfg, dw, st, vo, pairs, rd, rows_a, track)


def agent_obs_slot0():
    ops.agent_obs(cfg, dw, st, vo, pairs0, rd, rows_0, track)


def agent_obs_slot0_no_track():
    ops.agent_obs(cfg, dw, st, vo, pairs0, rd, rows_0)


def vector_obs():
    ops.vector_obs(cfg, dw, st, vo, rd, rows_v)


def swap_then_vector_obs():
    for k in COPIED:
        copy[k].copy_(st[k])
    for k in SWAPPED:
        c, s = copy[k].view(B, A), st[k].view(B, A)
        c[:, 0] = s[:, 1]
        c[:, 1] = s[:, 0]
    ops.vector_obs(cfg, dw, copy, vo, rd, rows_s)


def time_us(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


variants = (("agent_obs", agent_obs), ("vector_obs", vector_obs), ("swap_then_vector_obs", swap_then_vector_obs),
            ("agent_obs_slot0", agent_obs_slot0), ("agent_obs_slot0_no_track", agent_obs_slot0_no_track))
for _, fn in variants:
    for _ in range(20):
        fn()
times = {name: [] for name, _ in variants}
for _ in range(args.rounds):
    for name, fn in variants:
        times[name].append(time_us(fn, args.calls))
torch.cuda.synchronize()
present = (st["present"].view(B, A)[:, 1] != 0) & (st["present"].view(B, A)[:, 0] != 0)
same = bool(torch.equal(rows_a[present][:, 10:].view(torch.int32), rows_s[present][:, 10:].view(torch.int32)))
same0 = bool(torch.equal(rows_0.view(torch.int32), rows_v.view(torch.int32)))
out = dict(envs=B, slots=A, pairs=B, dim=vo.dim, calls=args.calls, rounds=args.rounds, swapped_rows_equal_agent_obs_from_entry_10=same,
           rows_compared=int(present.sum()), slot0_rows_equal_vector_obs=same0)
for name, ts in times.items():
    out[name] = dict(median_us=round(float(np.median(ts)), 2), min_us=round(min(ts), 2), max_us=round(max(ts), 2))
print(json.dumps(out))
