"""What a copy of n env rows costs on the GPU (include/tde_snapshot.h: tde_state_copy, one launch) against the composition a user writes
in torch without it, alternated in one process: one index_select / index_copy_ per state array plus the invalidation of the destination
rows' caches, and with frames two more pairs for the layer planes and the stacked observation.  The results are compared bit for bit
before anything is timed.  HIP events, medians over --reps repetitions after warm-up.  Writes a text report (default
profiles/state_copy.txt).

    python scripts/bench_snapshot.py [--envs 8192] [--reps 100] [--out profiles/state_copy.txt] [--note "..."]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_replay import CEILING, alternated

from torchdriveenv_amd import _abi, ops
from torchdriveenv_amd.config import EnvConfig
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.synth import synthetic_world

POINTS = (16, 1024)
MOVED = _abi.SNAPSHOT_COPIED + _abi.SNAPSHOT_OUTPUT_ARRAYS


def composition(src, dst, se, de, frames):
    """tde_state_copy(outputs=True) in torch: se / de int64 [n]; frames = (src_layers, dst_layers, src_obs, dst_obs, shift) or None"""
    sB, dB, A = src.B, dst.B, src.A
    launches = 0
    for k in MOVED:
        a, b = src[k], dst[k]
        if a is None or b is None:
            continue
        b.view(dB, -1).index_copy_(0, de, a.view(sB, -1).index_select(0, se))
        launches += 2
    dst["slot_cache"].view(dB, -1).index_fill_(0, de, 0)
    dst["env_cache"].index_fill_(0, de, 0)
    act = dst["act_cache"].view(dB, A + 1, 2)
    act.index_fill_(0, de, 0)
    act[:, A, 0].index_fill_(0, de, -1)
    launches += 4
    if frames is not None:
        sl, dl, so, do, shift = frames
        dl.index_copy_(0, de, sl.index_select(0, se).roll(shift, 1))
        do.index_copy_(0, de, so.index_select(0, se))
        launches += 5
    return launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join("profiles", "state_copy.txt"))
    ap.add_argument("--note", action="append", default=[], help="a line appended to the report (e.g. the flagship bench figures)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_snapshot.py needs a GPU: there is no CPU path"
    B, ns, plane = a.envs, 3, 64 * 64
    cfg = EnvConfig(seed=0, distance_cutoff=0.25, frame_stack=ns)
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    env = BatchedWaypointEnv(cfg, world, num_envs=B, frame_stack=ns)
    dev = env.torch_device
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    low, high = (torch.tensor(v, device=dev) for v in (env.action_space.low, env.action_space.high))
    for t in range(8):
        env.step(low + (high - low) * torch.rand(B, 2, device=dev, generator=gen))
    src, stack = env.state, env.observer.stack
    from torchdriveenv_amd.snapshot import _handle_for
    from torchdriveenv_amd.state import EnvState

    lines = [f"tde_state_copy: {B} envs x {env.A} agents, frame_stack {ns}, 64 x 64; outputs copied; {a.reps} repetitions after 20 warm-up "
             f"calls, HIP events, median [min, max] in us; device {torch.cuda.get_device_name(dev)}"]
    same = lambda x, y: torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8))   # noqa: E731
    row_bytes = sum(v.numel() * v.element_size() for k, v in src.arrays.items() if v is not None and k in MOVED) // B
    for n in POINTS:
        perm = torch.randperm(B, device=dev, generator=gen)
        se, de = perm[:n].contiguous(), torch.randperm(n, device=dev, generator=gen)
        se32, de32 = se.to(torch.int32), de.to(torch.int32)
        for with_frames in (False, True):
            dsts = []
            for _ in range(2):                              # one destination for the entry point, one for the composition
                st_c = EnvState(n, src.A, device=dev)        # the env state's optional arrays, and caches to invalidate
                lay = torch.zeros((n, ns, plane), dtype=torch.uint8, device=dev)
                obs = torch.zeros((n, 3 * ns, plane), dtype=torch.uint8, device=dev)
                dsts.append((st_c, lay, obs))
            (k_st, k_lay, k_obs), (c_st, c_lay, c_obs) = dsts
            h = (env._h, _handle_for(env, k_st))
            dphase = 1
            fr = ops.snapshot_frames(stack.layers, k_lay, stack.obs.view(B, 3 * ns, plane), k_obs, ns, plane, stack.phase, dphase) if with_frames else None
            frc = (stack.layers, c_lay, stack.obs.view(B, 3 * ns, plane), c_obs, (dphase - stack.phase) % ns) if with_frames else None
            kernel = lambda: ops.state_copy(src, k_st, se32, de32, frames=fr, outputs=True, check=False, handles=h)      # noqa: E731
            torch_way = lambda: composition(src, c_st, se, de, frc)                                                    # noqa: E731
            kernel()
            launches = torch_way()
            torch.cuda.synchronize()
            for k in k_st.arrays:
                if k_st[k] is not None:
                    assert same(k_st[k], c_st[k]), k
            assert same(k_lay, c_lay) and same(k_obs, c_obs)
            (k, c) = alternated([kernel, torch_way], a.reps)
            moved = n * (row_bytes + (4 * ns * plane if with_frames else 0))
            line = (f"n = {n:5d} pairs, {'with' if with_frames else 'without'} frames: tde_state_copy (1 launch) {k[0]:.1f} [{k[1]:.1f}, {k[2]:.1f}] us; "
                    f"the torch composition ({launches} launches) {c[0]:.1f} [{c[1]:.1f}, {c[2]:.1f}] us (ratio {c[0] / k[0]:.2f}x); results equal "
                    f"bit for bit; {moved / 1e6:.3f} MB copied")
            if with_frames:
                line += (f", read and written once: {2 * moved / k[0] / 1e6:.3f} TB/s of traffic = {100 * 2 * moved / (k[0] * 1e-6) / CEILING:.1f} % of the "
                         f"{CEILING / 1e12:.0f} TB/s copy ceiling")
            lines.append(line)
    lines += a.note
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
