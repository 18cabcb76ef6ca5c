"""What prioritized replay costs on the GPU (include/tde_priority.h), each against its counterpart, alternated in one process: (a)
sample_prioritized(n, 3) against the composition a user writes in torch without it - the validity mask over the ring, an int64 cumsum
of the masked priorities, a searchsorted of the same positions, then sample_nstep(idx=) - at n = 256 and 4096, the picks compared
before anything is timed, and beside them the uniform sample_nstep(n, 3) of the same process: the difference is the pick's cost; (b)
push() with and without priorities; (c) update_priorities(4096).  HIP events, medians over --reps repetitions after warm-up.  Writes a
text report (default profiles/priority_sample.txt).

    python scripts/bench_priority.py [--envs 8192] [--capacity 64] [--reps 200] [--out profiles/priority_sample.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_replay import alternated

from tests.priority_ref import strata
from torchdriveenv_amd.config import EnvConfig, Prioritized
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.synth import synthetic_world


def composition(buf, u, n_steps, gamma):
    """the prioritized batch at the positions u (int64 [n]) with torch ops: mask, cumsum, searchsorted, then the gather"""
    off = (torch.arange(buf.C, device=buf.dev) - buf.first) % buf.C
    ok = (off[:, None] < buf.count) & (torch.clamp(buf.age.to(torch.int64), max=buf.n_stack - 1) <= off[:, None])
    cum = torch.cumsum(torch.where(ok, buf.leaf, torch.zeros_like(buf.leaf)).reshape(-1).to(torch.int64), 0)
    l = torch.searchsorted(cum, u, right=True)
    idx = torch.stack([l // buf.B, l % buf.B], 1).to(torch.int32)
    return buf.sample_nstep(None, n_steps, gamma, idx=idx, check=False), buf.leaf.reshape(-1)[l]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--n-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "priority_sample.txt"))
    ap.add_argument("--note", action="append", default=[], help="a line appended to the report (e.g. the flagship bench figures)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_priority.py needs a GPU: there is no CPU path"
    B, ns, nst, gamma = a.envs, 3, a.n_steps, 0.99
    cfg = EnvConfig(seed=0, distance_cutoff=0.25, frame_stack=ns)
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    env = BatchedWaypointEnv(cfg, world, num_envs=B, frame_stack=ns)
    buf, plain = env.replay_buffer(a.capacity, seed=1, prioritized=Prioritized()), env.replay_buffer(a.capacity, seed=1)
    dev = env.torch_device
    env.reset()
    buf.begin()
    plain.begin()
    gen = torch.Generator(device=dev).manual_seed(0)
    low, high = (torch.tensor(v, device=dev) for v in (env.action_space.low, env.action_space.high))
    for t in range(a.capacity + 8):
        act = low + (high - low) * torch.rand(B, 2, device=dev, generator=gen)
        env.step(act)
        buf.push(act)
        plain.push(act)
    every = buf.valid_pairs()
    buf.update_priorities(every, 3 * torch.randn(len(every), device=dev, generator=gen))      # priorities that differ
    T = int(buf.sums[0])
    assert T == int(buf.leaf.to(torch.int64).sum()) and int((buf.leaf != 0).sum()) == len(every)
    lines = [f"prioritized replay: {B} envs, frame_stack {ns}, capacity_steps {a.capacity}, {buf.count} steps stored, {len(every)} drawable pairs of "
             f"{buf.C * B} leaves, total {T}; n_steps {nst}, gamma {gamma}; {a.reps} repetitions after 20 warm-up calls, HIP events, "
             f"median [min, max] in us; device {torch.cuda.get_device_name(dev)}"]
    for n in (256, 4096):
        draws = buf.draws
        got = buf.sample_prioritized(n, nst, gamma)
        u = torch.tensor(strata(T, n, buf.seed, draws), dtype=torch.int64, device=dev)
        want, wq = composition(buf, u, nst, gamma)
        same = lambda x, y: torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8))
        assert same(got.indices, want.indices) and same(got.priorities, wq) and same(got.observations, want.observations)
        assert same(got.next_observations, want.next_observations) and same(got.rewards, want.rewards)
        k, c, s = alternated([lambda: buf.sample_prioritized(n, nst, gamma), lambda: composition(buf, u, nst, gamma),
                              lambda: buf.sample_nstep(n, nst, gamma)], a.reps)
        lines.append(f"(a) sample_prioritized({n}, {nst}) {k[0]:.1f} [{k[1]:.1f}, {k[2]:.1f}] us (the pick, the gather and the weights); the torch "
                     f"composition at the same positions (mask + int64 cumsum + searchsorted + sample_nstep(idx=)) {c[0]:.1f} [{c[1]:.1f}, {c[2]:.1f}] us "
                     f"(ratio {c[0] / k[0]:.2f}x); picks and batches equal bit for bit; the uniform sample_nstep({n}, {nst}) {s[0]:.1f} "
                     f"[{s[1]:.1f}, {s[2]:.1f}] us: the pick and the weights cost {k[0] - s[0]:.1f} us")
    batch = buf.sample_prioritized(4096, nst, gamma)
    idx, td = batch.indices.clone(), torch.randn(4096, device=dev, generator=gen)
    (up,) = alternated([lambda: buf.update_priorities(idx, td)], a.reps)
    lines.append(f"(c) update_priorities(4096) {up[0]:.1f} [{up[1]:.1f}, {up[2]:.1f}] us (the torch power, the zeroing and raising passes, and the "
                 f"rebuild of the sums from all {buf.C * B} leaves: {4 * buf.C * B / 1e6:.1f} MB read)")
    act = low + (high - low) * torch.rand(B, 2, device=dev, generator=gen)
    pp, pn = alternated([lambda: buf.push(act), lambda: plain.push(act)], a.reps)
    assert int(buf.sums[0]) == int(buf.leaf.to(torch.int64).sum())
    lines.append(f"(b) push() with priorities {pp[0]:.1f} [{pp[1]:.1f}, {pp[2]:.1f}] us, without {pn[0]:.1f} [{pn[1]:.1f}, {pn[2]:.1f}] us "
                 f"({pp[0] - pn[0]:+.1f} us: tde_priority_push's two launches, the second the same rebuild)")
    lines += a.note
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
