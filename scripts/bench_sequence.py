"""What the sequence sample costs on the GPU (include/tde_sequence.h) against the composition a user writes without it, alternated in one
process: sample_sequence(N, T) against tde_replay_sample over the N * T expanded pairs (slot(s + k), e) plus the torch stop rule that
finds each window's length and mask from the ring's done array.  The results are compared bit for bit before anything is timed.  HIP
events, medians over --reps repetitions after warm-up.  Writes a text report (default profiles/sequence_sample.txt).

    python scripts/bench_sequence.py [--envs 8192] [--capacity 128] [--reps 100] [--out profiles/sequence_sample.txt]
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
POINTS = ((64, 80), (256, 16), (1024, 8))


def composition(buf, idx, T, out):
    """the windows of the start pairs idx (int32 [n, 2], valid) from one one-step sample of the n * T expanded pairs and the stop rule
    in torch -> (lengths [n], mask [n, T]); observations / next_observations land in `out` in [n * T] order"""
    n, dev = idx.shape[0], buf.dev
    s, e = idx[:, 0].long(), idx[:, 1].long()
    k = torch.arange(T, device=dev)
    slots = (s[:, None] + k[None, :]) % buf.C
    pairs = torch.stack([slots, e[:, None].expand(n, T)], 2).reshape(n * T, 2).to(torch.int32)
    ops.replay_sample(buf.struct, dev, buf.first, buf.count, n * T, out, pairs)
    off = (s - buf.first) % buf.C
    a = torch.clamp(buf.count - off, max=T)
    ended = ((buf.done[slots, e[:, None]] & ENDED) != 0) & (k[None, :] < a[:, None])
    first_end = torch.where(ended.any(1), ended.to(torch.uint8).argmax(1) + 1, a)
    return first_end.to(torch.int32), k[None, :] < first_end[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--capacity", type=int, default=128)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join("profiles", "sequence_sample.txt"))
    ap.add_argument("--note", action="append", default=[], help="a line appended to the report (e.g. the flagship bench figures)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sequence.py needs a GPU: there is no CPU path"
    B, ns, plane = a.envs, 3, 64 * 64
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
    lines = [f"sequence sample: {B} envs, frame_stack {ns}, capacity_steps {a.capacity}, {buf.count} steps stored, "
             f"{100 * float(((buf.done[stored] & ENDED) != 0).float().mean()):.2f} % of them ended an episode; "
             f"{a.reps} repetitions after 20 warm-up calls, HIP events, median [min, max] in us; device {torch.cuda.get_device_name(dev)}"]
    same = lambda x, y: torch.equal(x.contiguous().reshape(-1).view(torch.uint8), y.contiguous().reshape(-1).view(torch.uint8))
    for n, T in POINTS:
        if T > buf.count - (ns - 1):
            lines.append(f"sample_sequence({n}, {T}): skipped, the buffer holds {buf.count} steps")
            continue
        out = {k: torch.empty_like(v) for k, v in buf._alloc(n * T).items()}
        got = buf.sample_sequence(n, T)
        idx = got.indices.clone()
        lengths, mask = composition(buf, idx, T, out)
        m = got.lengths.long()
        rows = torch.arange(n, device=dev)
        obs_c = out["observations"].view(n, T, *out["observations"].shape[1:])
        nxt_c = out["next_observations"].view(n, T, *out["next_observations"].shape[1:])
        assert same(got.lengths, lengths) and torch.equal(got.mask, mask)
        assert same(got.observations[:, :T][mask], obs_c[mask]) and same(got.observations[rows, m], nxt_c[rows, m - 1])
        assert same(got.actions[mask], out["actions"].view(n, T, 2)[mask]) and same(got.dones[mask], out["dones"].view(n, T)[mask])
        assert same(got.rewards[mask], out["rewards"].view(n, T)[mask])
        pad = torch.arange(T + 1, device=dev)[None, :] > m[:, None]
        assert not got.observations[pad].any()
        del obs_c, nxt_c
        k, kd, c = alternated([lambda: buf.sample_sequence(n, T, idx=idx, check=False), lambda: buf.sample_sequence(n, T),
                               lambda: composition(buf, idx, T, out)], a.reps)
        wr, wr_c = n * (T + 1) * 3 * ns * plane, n * T * 2 * 3 * ns * plane
        rd, rd_c = n * (T + ns) * plane, n * T * (ns + 1) * plane
        hist = f"mean length {float(got.lengths.float().mean()):.1f}, {100 * float((got.lengths == T).float().mean()):.0f} % of the windows full"
        lines.append(f"sample_sequence({n}, {T}): given starts {k[0]:.1f} [{k[1]:.1f}, {k[2]:.1f}] us, drawn {kd[0]:.1f} [{kd[1]:.1f}, {kd[2]:.1f}] us; "
                     f"the composition on the same starts (tde_replay_sample over {n * T} pairs + the torch stop rule) {c[0]:.1f} [{c[1]:.1f}, {c[2]:.1f}] us "
                     f"(ratio {c[0] / k[0]:.2f}x); results equal bit for bit; {hist}")
        lines.append(f"    entry point (two launches): {wr / 1e6:.1f} MB written once, at most {rd / 1e6:.1f} MB of planes read once; write bandwidth "
                     f"{wr / k[0] / 1e6:.2f} TB/s = {100 * wr / (k[0] * 1e-6) / CEILING:.0f} % of the {CEILING / 1e12:.0f} TB/s ceiling; "
                     f"the composition writes {wr_c / 1e6:.1f} MB ({wr_c / wr:.2f}x) and reads {rd_c / 1e6:.1f} MB, at "
                     f"{wr_c / c[0] / 1e6:.2f} TB/s written over its whole time")
        del out
    lines += a.note
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
