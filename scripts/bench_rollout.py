"""Rollout buffer timings on the GPU, each against what a user would otherwise write, alternated with it in the same process:
(a) finish() - one tde_gae launch - against the same recurrence as a torch loop over time-ordered [T][B] tensors (SB3's
    compute_returns_and_advantage, its inputs gathered out of the ring beforehand, outside the timing);
(b) one get(4096) minibatch (tde_onpolicy_gather) against ReplayBuffer.sample(idx=...) of the same (slot, env) pairs, the only other
    way to rebuild those stacks, which also writes next_observations; and a whole epoch of get(4096), permutation included.
The two gathers are compared byte for byte, and the two advantage computations to 1e-5 (the torch loop multiplies by the float
non-terminal mask where the kernel selects), before anything is timed.  HIP events, medians over --reps repetitions after warm-up.
Writes a text report (default profiles/onpolicy_buffer.txt).

    python scripts/bench_rollout.py [--envs 8192] [--steps 128] [--batch 4096] [--reps 200] [--out profiles/onpolicy_buffer.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchdriveenv_amd import _abi
from torchdriveenv_amd.config import EnvConfig
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.synth import synthetic_world


def alternated(fns, reps, warmup=20):
    """(median, min, max) in microseconds of `reps` event-timed calls of each callable, one call of each per round"""
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
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join("profiles", "onpolicy_buffer.txt"))
    ap.add_argument("--note", action="append", default=[], help="a line appended to the report (e.g. the flagship bench figures)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rollout.py needs a GPU: there is no CPU path"
    B, T, n, ns, plane = a.envs, a.steps, a.batch, 3, 64 * 64
    cfg = EnvConfig(seed=0, distance_cutoff=0.25, frame_stack=ns)
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    env = BatchedWaypointEnv(cfg, world, num_envs=B, frame_stack=ns)
    buf = env.rollout_buffer(T, gamma=0.99, gae_lambda=0.95, seed=1)
    dev = env.torch_device
    gen = torch.Generator(device=dev).manual_seed(0)
    low, high = (torch.tensor(v, device=dev) for v in (env.action_space.low, env.action_space.high))
    env.reset()
    buf.begin()
    for t in range(T + T // 2):                      # one rollout and a half: the timed one has wrapped the ring
        if buf.full:
            buf.finish(torch.randn(B, device=dev, generator=gen))
        act = low + (high - low) * torch.rand(B, 2, device=dev, generator=gen)
        env.step(act)
        buf.push(act, torch.randn(B, device=dev, generator=gen), -torch.rand(B, device=dev, generator=gen))
    while not buf.full:
        act = low + (high - low) * torch.rand(B, 2, device=dev, generator=gen)
        env.step(act)
        buf.push(act, torch.randn(B, device=dev, generator=gen), -torch.rand(B, device=dev, generator=gen))
    last_values = torch.randn(B, device=dev, generator=gen)
    ring = buf.ring
    lines = [f"rollout buffer: {B} envs, frame_stack {ns}, n_steps {T} (ring of {ring.C} slots, {ring.count} steps stored, first slot {ring.first}); "
             f"{a.reps} repetitions after 20 warm-up calls, HIP events, median [min, max] in us; device {torch.cuda.get_device_name(dev)}"]

    # ---- (a) advantages ----------------------------------------------------------------------------------------------------
    slots = (ring.first + ring.count - T + torch.arange(T, device=dev)) % ring.C
    reward = ring.reward[slots].contiguous()
    nnt = ((ring.done[slots] & (3 | _abi.REPLAY_CUT)) == 0).to(torch.float32).contiguous()
    values, gamma, lam = buf.values, buf.gamma, buf.gae_lambda
    adv_t, ret_t = torch.empty_like(values), torch.empty_like(values)

    def torch_gae():
        last = torch.zeros(B, device=dev)
        for t in range(T - 1, -1, -1):
            nv = last_values if t == T - 1 else values[t + 1]
            delta = reward[t] + gamma * nv * nnt[t] - values[t]
            last = delta + gamma * lam * nnt[t] * last
            adv_t[t] = last
        torch.add(adv_t, values, out=ret_t)

    def kernel_gae():
        buf.finish(last_values)

    kernel_gae()
    torch_gae()
    torch.cuda.synchronize()
    err = float((buf.advantages - adv_t).abs().max() / adv_t.abs().max())
    assert err < 1e-5, f"the torch loop and tde_gae disagree: {err}"
    k, c = alternated([kernel_gae, torch_gae], max(10, a.reps // 4))
    moved = T * B * (4 + 1 + 4 + 4 + 4) + 4 * B
    lines.append(f"(a) finish(): tde_gae {k[0]:.1f} [{k[1]:.1f}, {k[2]:.1f}] us, torch loop over [T][B] tensors {c[0]:.1f} [{c[1]:.1f}, {c[2]:.1f}] us "
                 f"(ratio {c[0] / k[0]:.0f}x); largest relative difference of the two results {err:.1e}")
    lines.append(f"    tde_gae: 1 launch, {(B + 63) // 64} wavefronts, {moved / 1e6:.1f} MB read + written = {moved / k[0] / 1e6:.2f} TB/s "
                 f"(latency-bound: a serial chain of {T} steps per lane); torch loop: {T} x 8 + 2 launches")

    # ---- (b) minibatches ----------------------------------------------------------------------------------------------------
    idx = torch.randperm(T * B, device=dev, generator=gen)[:n].to(torch.int32)
    pairs = torch.stack([slots[(idx // B).long()].to(torch.int32), idx % B], 1).contiguous()

    def kernel_gather():
        return buf.gather(idx)

    def replay_sample():
        return ring.sample(n, idx=pairs, check=False)

    g, s = kernel_gather(), replay_sample()
    assert torch.equal(g.observations, s.observations) and torch.equal(g.actions, s.actions), "the two gathers disagree"
    k, c = alternated([kernel_gather, replay_sample], a.reps)
    rd, wr = n * ns * plane, n * 3 * ns * plane
    lines.append(f"(b) one minibatch of {n}: get() / tde_onpolicy_gather {k[0]:.1f} [{k[1]:.1f}, {k[2]:.1f}] us, ReplayBuffer.sample(idx=) of the same "
                 f"pairs {c[0]:.1f} [{c[1]:.1f}, {c[2]:.1f}] us (ratio {c[0] / k[0]:.2f}x); observations and actions of the two identical")
    lines.append(f"    tde_onpolicy_gather, per sample: {ns * plane} B read, {3 * ns * plane} B written; in all {rd / 1e6:.1f} MB read, {wr / 1e6:.1f} MB "
                 f"written; write bandwidth {wr / k[0] / 1e6:.2f} TB/s.  tde_replay_sample: {(ns + 1) * plane} B read, {2 * 3 * ns * plane} B written per sample")
    torch.cuda.synchronize()
    epochs = []
    for _ in range(5):
        t0 = time.perf_counter()
        batches = sum(1 for _ in buf.get(n))
        torch.cuda.synchronize()
        epochs.append((time.perf_counter() - t0) * 1e3)
    lines.append(f"    a whole epoch of get({n}): {batches} batches of {T * B} samples, permutation included, host clock around a device synchronise: "
                 f"{statistics.median(epochs):.2f} [{min(epochs):.2f}, {max(epochs):.2f}] ms over {len(epochs)} epochs = "
                 f"{statistics.median(epochs) * 1e3 / batches:.1f} us per batch")
    held = ring.bytes_per_transition + 16
    lines.append(f"bytes held per sample: {held} ({plane} layer bytes + action 8 + reward 4 + done 1 + age 1 + value, log-probability, advantage, return "
                 f"16); a store of stacked observations: {3 * ns * plane + 32} (SB3's layout)")
    lines.append(f"at {B} envs x {T} steps: {held * B * T / 1e9:.2f} GB held ({ring.C} ring slots: {ring.bytes_per_transition * B * ring.C / 1e9:.2f} GB); "
                 f"stacked store {(3 * ns * plane + 32) * B * T / 1e9:.1f} GB")
    lines += a.note
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
