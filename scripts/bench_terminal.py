"""What terminal observations cost on the GPU (include/tde_terminal.h), each against its counterpart without them, alternated in one
process: (a) step() of a terminal_obs env against the same env without the option, (b) tde_terminal_sample(n) against tde_replay_sample(n)
on the same ring, (c) push() with tde_terminal_push against push() alone.  HIP events, medians over --reps repetitions after warm-up.
Writes a text report (default profiles/terminal_obs.txt).

    python scripts/bench_terminal.py [--envs 8192] [--capacity 64] [--reps 200] [--max-steps 100] [--out profiles/terminal_obs.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_replay import alternated

from torchdriveenv_amd import _abi, ops
from torchdriveenv_amd.config import EnvConfig
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.synth import synthetic_world


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--capacity", type=int, default=64)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--max-steps", type=int, default=100, help="max_environment_steps: every env is truncated, all at once, each time it runs out")
    ap.add_argument("--out", default=os.path.join("profiles", "terminal_obs.txt"))
    ap.add_argument("--note", action="append", default=[], help="a line appended to the report (e.g. the flagship bench figures)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_terminal.py needs a GPU: there is no CPU path"
    B, ns, n = a.envs, 3, 4096
    cfg = EnvConfig(seed=0, distance_cutoff=0.25, frame_stack=ns, max_environment_steps=a.max_steps)
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    plain = BatchedWaypointEnv(cfg, world, num_envs=B, frame_stack=ns)
    term = BatchedWaypointEnv(cfg, world, num_envs=B, frame_stack=ns, terminal_obs=True)
    pbuf, tbuf = plain.replay_buffer(a.capacity, seed=1), term.replay_buffer(a.capacity, seed=1)
    dev = term.torch_device
    plain.reset(), term.reset()
    pbuf.begin(), tbuf.begin()
    gen = torch.Generator(device=dev).manual_seed(0)
    low, high = (torch.tensor(v, device=dev) for v in (term.action_space.low, term.action_space.high))
    acts = [low + (high - low) * torch.rand(B, 2, device=dev, generator=gen) for _ in range(16)]
    for t in range(a.max_steps + a.capacity // 2):       # the ring ends up holding the step at which every env ran out
        plain.step(acts[t % 16]), term.step(acts[t % 16])
        pbuf.push(acts[t % 16]), tbuf.push(acts[t % 16])
    assert torch.equal(plain.observer.obs, term.observer.obs) and torch.equal(pbuf.done, tbuf.done)
    stored = (tbuf.first + torch.arange(tbuf.count, device=dev)) % tbuf.C      # (the open slot holds no step)
    fin, pooled = (tbuf.done[stored] & 3) != 0, int((tbuf.ref[stored] >= 0).sum())
    lines = [f"terminal observations: {B} envs x 16 agents, frame_stack {ns}, capacity_steps {a.capacity}, pool rows per step {tbuf.M}; "
             f"{a.reps} repetitions after 20 warm-up calls, HIP events, median [min, max] in us; device {torch.cuda.get_device_name(dev)}",
             f"ring: {tbuf.count} steps stored, {100 * float(fin.float().mean()):.2f} % of the stored steps ended an episode, "
             f"{pooled} terminal frames pooled ({int(fin.sum()) - pooled} overflowed)"]
    k = [0]

    def act():
        k[0] += 1
        return acts[k[0] % 16]

    s0, s1 = alternated([lambda: plain.step(act()), lambda: term.step(act())], a.reps)
    lines.append(f"(a) step(): without the option {s0[0]:.1f} [{s0[1]:.1f}, {s0[2]:.1f}] us, terminal_obs=True {s1[0]:.1f} [{s1[1]:.1f}, {s1[2]:.1f}] us "
                 f"(+{s1[0] - s0[0]:.1f} us)")
    # what the option adds to a step, each part called alone on the state the last step left (its mask: the envs that step finished)
    st = term.state
    src, off, stride = term.observer.newest_frame()

    def mask():
        torch.bitwise_or(st["terminated"], st["truncated"], out=term._term_mask)

    parts = alternated([mask, lambda: ops.terminal_stash(dev, st["done_bits"], src, off, stride, term.terminal_frames),
                        lambda: term.reset(mask=term._term_mask)], a.reps)
    lines.append("    its parts, each alone: the mask (one torch kernel) {:.1f} us, tde_terminal_stash {:.1f} us, reset(mask): the masked re-spawn + "
                 "re-render {:.1f} us; sum {:.1f} us".format(parts[0][0], parts[1][0], parts[2][0], sum(p[0] for p in parts)))
    out = {key: torch.empty_like(v) for key, v in tbuf._buffers(n).items()}
    draw = [0]

    def replay_sample():
        draw[0] += 1
        ops.replay_sample(tbuf.struct, dev, tbuf.first, tbuf.count, n, out, None, 1, draw[0])

    r0, r1 = alternated([replay_sample, lambda: tbuf.sample(n)], a.reps)
    s = tbuf.sample(n)
    has = int(((s.dones & _abi.TERMINAL_HAS) != 0).sum())
    lines.append(f"(b) sample({n}) on the same ring: tde_replay_sample {r0[0]:.1f} [{r0[1]:.1f}, {r0[2]:.1f}] us, tde_terminal_sample "
                 f"{r1[0]:.1f} [{r1[1]:.1f}, {r1[2]:.1f}] us ({has} of the {n} samples carried a terminal observation)")
    p0, p1 = alternated([lambda: pbuf.push(acts[0]), lambda: tbuf.push(acts[0])], a.reps)
    lines.append(f"(c) push(): tde_replay_push alone {p0[0]:.1f} [{p0[1]:.1f}, {p0[2]:.1f}] us, with tde_terminal_push {p1[0]:.1f} [{p1[1]:.1f}, {p1[2]:.1f}] us "
                 f"(+{p1[0] - p0[0]:.1f} us)")
    pool = tbuf.pool.numel() * tbuf.pool.element_size() + tbuf.ref.numel() * 4
    ring = tbuf.frames.numel()
    lines.append(f"memory: ring frames {ring / 1e9:.2f} GB, pool + references {pool / 1e9:.3f} GB (+{100 * pool / ring:.1f} %); a second ring of "
                 f"terminal frames would be +100 %")
    lines += a.note
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
