"""What the n-step sample costs on the GPU (include/tde_nstep.h), each against its counterpart, alternated in one process: (a)
sample_nstep(n, 3) against the composition a user writes without it - tde_replay_sample at (s, e), a torch loop over the ring's reward
and done arrays that finds the last step L and sums the rewards, tde_replay_sample again at (L, e) - at n = 4096 and 256, the results
compared bit for bit before anything is timed; (b) sample_nstep(4096, 1) against tde_replay_sample(4096) on the same ring.  HIP events,
medians over --reps repetitions after warm-up.  Writes a text report (default profiles/nstep_sample.txt).

    python scripts/bench_nstep.py [--envs 8192] [--capacity 64] [--reps 200] [--out profiles/nstep_sample.txt]
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

ENDED = 3 | _abi.REPLAY_CUT


def composition(buf, idx, n_steps, gamma, first_out, last_out):
    """the n-step batch of the pairs idx (int32 [n, 2], valid) from two one-step samples and a torch loop -> (rewards, discounts, steps)"""
    n, dev = idx.shape[0], buf.dev
    ops.replay_sample(buf.struct, dev, buf.first, buf.count, n, first_out, idx)
    s, e = idx[:, 0].long(), idx[:, 1].long()
    off = (s - buf.first) % buf.C
    R, g = buf.reward[s, e].clone(), torch.full((n,), gamma, dtype=torch.float32, device=dev)
    m, last = torch.ones(n, dtype=torch.int64, device=dev), s.clone()
    alive = ((buf.done[s, e] & ENDED) == 0) & (off + 1 < buf.count)
    for k in range(1, n_steps):
        t = (s + k) % buf.C
        R = torch.where(alive, R + g * buf.reward[t, e], R)
        g = torch.where(alive, g * gamma, g)
        last = torch.where(alive, t, last)
        m = m + alive
        alive = alive & ((buf.done[t, e] & ENDED) == 0) & (off + k + 1 < buf.count)
    ops.replay_sample(buf.struct, dev, buf.first, buf.count, n, last_out, torch.stack([last, e], 1).to(torch.int32))
    return R, g, m.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--n-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "nstep_sample.txt"))
    ap.add_argument("--note", action="append", default=[], help="a line appended to the report (e.g. the flagship bench figures)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_nstep.py needs a GPU: there is no CPU path"
    B, ns, plane, nst, gamma = a.envs, 3, 64 * 64, a.n_steps, 0.99
    cfg = EnvConfig(seed=0, distance_cutoff=0.25, frame_stack=ns)
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    env = BatchedWaypointEnv(cfg, world, num_envs=B, frame_stack=ns)
    buf = env.replay_buffer(a.capacity, seed=1)
    dev = env.torch_device
    env.reset()
    buf.begin()
    gen = torch.Generator(device=dev).manual_seed(0)
    low, high = (torch.tensor(v, device=dev) for v in (env.action_space.low, env.action_space.high))
    for t in range(a.capacity + 8):
        act = low + (high - low) * torch.rand(B, 2, device=dev, generator=gen)
        env.step(act)
        buf.push(act)
    stored = (buf.first + torch.arange(buf.count, device=dev)) % buf.C
    lines = [f"n-step sample: {B} envs, frame_stack {ns}, capacity_steps {a.capacity}, {buf.count} steps stored, "
             f"{100 * float(((buf.done[stored] & ENDED) != 0).float().mean()):.2f} % of them ended an episode; n_steps {nst}, gamma {gamma}; "
             f"{a.reps} repetitions after 20 warm-up calls, HIP events, median [min, max] in us; device {torch.cuda.get_device_name(dev)}"]
    for n in (4096, 256):
        first_out, last_out = ({k: torch.empty_like(v) for k, v in buf._alloc(n).items()} for _ in range(2))
        got = buf.sample_nstep(n, nst, gamma)
        idx = got.indices.clone()
        R, g, m = composition(buf, idx, nst, gamma, first_out, last_out)
        same = lambda x, y: torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8))
        assert same(got.observations, first_out["observations"]) and same(got.actions, first_out["actions"])
        assert same(got.next_observations, last_out["next_observations"]) and same(got.dones, last_out["dones"])
        assert same(got.rewards, R) and same(got.discounts, g) and same(got.steps, m)
        hist = torch.bincount(got.steps.long(), minlength=nst + 1).tolist()[1:]
        k, kd, c = alternated([lambda: buf.sample_nstep(n, nst, gamma, idx=idx, check=False), lambda: buf.sample_nstep(n, nst, gamma),
                               lambda: composition(buf, idx, nst, gamma, first_out, last_out)], a.reps)
        wr = n * 2 * 3 * ns * plane
        lines.append(f"(a) sample_nstep({n}, {nst}): given pairs {k[0]:.1f} [{k[1]:.1f}, {k[2]:.1f}] us, drawn {kd[0]:.1f} [{kd[1]:.1f}, {kd[2]:.1f}] us; "
                     f"the composition on the same pairs (two tde_replay_sample calls + the torch loop) {c[0]:.1f} [{c[1]:.1f}, {c[2]:.1f}] us "
                     f"(ratio {c[0] / k[0]:.2f}x); results equal bit for bit; steps taken 1..{nst}: {hist}")
        lines.append(f"    kernel: {wr / 1e6:.1f} MB written, once; write bandwidth {wr / kd[0] / 1e6:.2f} TB/s = "
                     f"{100 * wr / (kd[0] * 1e-6) / CEILING:.0f} % of the {CEILING / 1e12:.0f} TB/s ceiling; the composition writes {2 * wr / 1e6:.1f} MB and keeps half")
    n = 4096
    out = {k: torch.empty_like(v) for k, v in buf._alloc(n).items()}
    draw = [0]

    def replay_sample():
        draw[0] += 1
        ops.replay_sample(buf.struct, dev, buf.first, buf.count, n, out, None, 1, draw[0])

    r0, r1, r3 = alternated([replay_sample, lambda: buf.sample_nstep(n, 1, gamma), lambda: buf.sample_nstep(n, nst, gamma)], a.reps)
    rd0, rd1 = (ns + 1) * plane, 2 * ns * plane
    lines.append(f"(b) on the same ring at n = {n}: tde_replay_sample {r0[0]:.1f} [{r0[1]:.1f}, {r0[2]:.1f}] us, sample_nstep(n, 1) "
                 f"{r1[0]:.1f} [{r1[1]:.1f}, {r1[2]:.1f}] us ({100 * (r1[0] / r0[0] - 1):+.1f} %), sample_nstep(n, {nst}) {r3[0]:.1f} [{r3[1]:.1f}, {r3[2]:.1f}] us")
    lines.append(f"    per sample the one-step gather reads {rd0} B and writes {2 * 3 * ns * plane} B; the n-step gather (a wavefront per written frame) "
                 f"reads {rd1} B, {rd1 - rd0} of them a second read of a plane its workgroup has just read: "
                 f"{100 * (rd1 - rd0) / (rd0 + 2 * 3 * ns * plane):.1f} % more traffic")
    lines += a.note
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
