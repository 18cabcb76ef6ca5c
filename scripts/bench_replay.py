"""Replay buffer timings on the GPU: push per step, and sample(256) / sample(4096) against the torch composition a user would otherwise
write (a buffer of stacked uint8 observations [C * B, 9, 64, 64] at a C that fits, index_select once for obs and once for next_obs,
where() for the finished rows), alternated with the kernel in the same process.  HIP events, medians over --reps repetitions after
warm-up.  Writes a text report (default profiles/replay_sample.txt).

    python scripts/bench_replay.py [--envs 8192] [--capacity 64] [--reps 200] [--out profiles/replay_sample.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchdriveenv_amd.config import EnvConfig
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.synth import synthetic_world

CEILING = 6.0e12          # bytes/s: the practical write ceiling DESIGN section 5 uses for large views


def timed(fn, reps, warmup=20):
    """median, min, max of `reps` event-timed calls, in microseconds"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in ev]
    return statistics.median(us), min(us), max(us)


def alternated(fns, reps, warmup=20):
    """the same for several callables, one call of each per round"""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(reps)]
    for row in ev:
        for f, (a, b) in zip(fns, row):
            a.record()
            f()
            b.record()
    torch.cuda.synchronize()
    out = []
    for k in range(len(fns)):
        us = [row[k][0].elapsed_time(row[k][1]) * 1e3 for row in ev]
        out.append((statistics.median(us), min(us), max(us)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--torch-capacity", type=int, default=8, help="slots of the stacked-observation baseline (8 x 8192 x 36864 B = 2.4 GB)")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join("profiles", "replay_sample.txt"))
    ap.add_argument("--note", action="append", default=[], help="a line appended to the report (e.g. the flagship bench figures)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_replay.py needs a GPU: there is no CPU path"
    B, ns, plane = a.envs, 3, 64 * 64
    cfg = EnvConfig(seed=0, distance_cutoff=0.25, frame_stack=ns)
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    env = BatchedWaypointEnv(cfg, world, num_envs=B, frame_stack=ns)
    buf = env.replay_buffer(a.capacity, seed=1)
    dev = env.torch_device
    env.reset()
    buf.begin()
    # the baseline's store: stacked observations of the last `torch-capacity` steps, filled beside the buffer
    Ct = a.torch_capacity
    store = torch.zeros((Ct * B, 3 * ns, 64, 64), dtype=torch.uint8, device=dev)
    store_done = torch.zeros(Ct * B, dtype=torch.uint8, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    low, high = (torch.tensor(v, device=dev) for v in (env.action_space.low, env.action_space.high))
    steps = a.capacity + 8
    for t in range(steps):
        act = low + (high - low) * torch.rand(B, 2, device=dev, generator=gen)
        store[(t % Ct) * B:(t % Ct + 1) * B].copy_(env.observer.obs)
        obs, *_ = env.step(act)
        store_done[(t % Ct) * B:(t % Ct + 1) * B].copy_(env.state["done_bits"])
        buf.push(act)
    lines = [f"replay buffer: {B} envs, frame_stack {ns}, capacity_steps {a.capacity}, {buf.count} steps stored; {a.reps} repetitions after 20 warm-up "
             f"calls, HIP events, median [min, max] in us; device {torch.cuda.get_device_name(dev)}"]
    act = low + (high - low) * torch.rand(B, 2, device=dev, generator=gen)
    w0, first0, count0 = buf.w, buf.first, buf.count

    def push_only():
        buf.push(act)                    # (the same frame again: the kernel's work does not depend on the pixels)

    m = timed(push_only, a.reps)
    moved = B * (2 * plane + 8 + 4 + 1 + 1 + 1 + 1)
    lines.append(f"push: {m[0]:.1f} [{m[1]:.1f}, {m[2]:.1f}] us per step of {B} envs; {moved / 1e6:.1f} MB read + written = {moved / m[0] / 1e6:.2f} TB/s")
    for n in (256, 4096):
        sel = torch.empty(n, dtype=torch.int64, device=dev)
        out_o, out_n = (torch.empty((n, 3 * ns, 64, 64), dtype=torch.uint8, device=dev) for _ in range(2))
        zero = torch.zeros((), dtype=torch.uint8, device=dev)

        def kernel():
            buf.sample(n)

        def composition():
            # draws in [0, (Ct - 1) * B): the row B further on is the next step's observation of the same env
            torch.randint(0, (Ct - 1) * B, (n,), device=dev, generator=gen, out=sel)
            torch.index_select(store, 0, sel, out=out_o)
            torch.index_select(store, 0, sel + B, out=out_n)
            ended = (store_done[sel] & 3) != 0
            torch.where(ended[:, None, None, None], zero, out_n, out=out_n)

        (k, c) = alternated([kernel, composition], a.reps)
        rd, wr = n * (ns + 1) * plane, n * 2 * 3 * ns * plane
        lines.append(f"sample({n}): kernel {k[0]:.1f} [{k[1]:.1f}, {k[2]:.1f}] us, torch composition {c[0]:.1f} [{c[1]:.1f}, {c[2]:.1f}] us "
                     f"(ratio {c[0] / k[0]:.2f}x)")
        lines.append(f"    kernel, per sample: {(ns + 1) * plane} B read, {2 * 3 * ns * plane} B written; in all {rd / 1e6:.1f} MB read, {wr / 1e6:.1f} MB written; "
                     f"write bandwidth {wr / k[0] / 1e6:.2f} TB/s = {100 * wr / (k[0] * 1e-6) / CEILING:.0f} % of the {CEILING / 1e12:.0f} TB/s ceiling")
        lines.append(f"    composition, per sample: {2 * 3 * ns * plane} B read, {2 * 3 * ns * plane} B written (+ the where pass: {3 * ns * plane} B read and written)")
    held = buf.bytes_per_transition
    lines.append(f"bytes held per transition: buffer {held} ({plane} layer bytes + action 8 + reward 4 + done 1 + age 1), "
                 f"stacked obs + next_obs store {2 * 3 * ns * plane + 13} (SB3's layout); the baseline above keeps obs only and reads next_obs from the next row: "
                 f"{3 * ns * plane + 1}")
    lines.append(f"at {B} envs: buffer {held * B / 1e6:.1f} MB per step, {held * B * a.capacity / 1e9:.2f} GB for {a.capacity} steps; "
                 f"stacked store {(2 * 3 * ns * plane + 13) * B / 1e6:.1f} MB per step")
    lines += a.note
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
