"""What tde_env_step_driven costs against the one-role step it is made of (include/tde_driven.h), at 8192 envs x 16 slots and 1024 envs x
128 slots.  Four launches alternated in one process, one call of each per round, on four states reset alike:

    solo      tde_env_step forced to its one-role kernel (tde_kernel_override): the yardstick
    none      tde_env_step_driven, driven = NULL
    all       tde_env_step_driven, every slot's mask byte set
    one       tde_env_step_driven, slot 1 of every env driven

HIP events around each call, median [min, max] in us over --reps rounds after 20 warm-up rounds.  Each shape is measured by a child
process of its own under `timeout`; the children run one after the other and the first that fails ends the run (the && of a shell
chain).  Writes a text report (default profiles/driven_step.txt).

    python scripts/measure_driven.py [--reps 300] [--out profiles/driven_step.txt]
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

POINTS = ((8192, 16), (1024, 128))
LIMIT = 240          # seconds per shape: world build + 4 x (20 + reps) launches of tens of microseconds


def point(B, A, reps):
    import torch

    from bench_replay import alternated
    from torchdriveenv_amd import _abi, _lib, ops
    from torchdriveenv_amd.state import EnvState
    from torchdriveenv_amd.synth import synthetic_town, synthetic_world

    assert torch.cuda.is_available(), "measure_driven.py needs a GPU: there is no CPU path"
    dev = "cuda:0"
    if A == 128:
        world = synthetic_town(n_scn=4, A=A, n_streets=4, spacing=100.0, ext=160.0, min_gap=3.4, n_signals=4)
    else:
        world = synthetic_world(n_scn=64, A=A, seed=0, n_maps=4)
    dw = world.to_device(dev)
    cfg = _abi.default_config(seed=1, distance_cutoff=0.25, flags=_abi.F_ALL)
    states = [EnvState(B, A, device=dev) for _ in range(4)]
    gen = torch.Generator(device=dev).manual_seed(0)
    act = torch.stack([torch.rand(B, generator=gen, device=dev) * 2 - 1, torch.rand(B, generator=gen, device=dev) * 0.6 - 0.3], -1).contiguous()
    for s in states:
        ops.env_reset(cfg, dw, s)
        s["action"].copy_(act)
    aa = torch.stack([torch.rand(B, A, generator=gen, device=dev) * 2 - 1, torch.rand(B, A, generator=gen, device=dev) * 0.2 - 0.1], -1).contiguous()
    every = torch.ones(B, A, dtype=torch.uint8, device=dev)
    one = torch.zeros(B, A, dtype=torch.uint8, device=dev)
    one[:, 1] = 1
    _lib.kernel_override(step="solo")
    fns = [lambda: ops.env_step(cfg, dw, states[0]), lambda: ops.env_step_driven(cfg, dw, states[1]),
           lambda: ops.env_step_driven(cfg, dw, states[2], aa, every), lambda: ops.env_step_driven(cfg, dw, states[3], aa, one)]
    res = alternated(fns, reps)
    _lib.kernel_override()
    names = ("solo", "none", "all", "one")
    print(f"{B} envs x {A} slots ({torch.cuda.get_device_name(0)}), {reps} rounds: " +
          "; ".join(f"{n} {m:.2f} [{lo:.2f}, {hi:.2f}] us" for n, (m, lo, hi) in zip(names, res)) +
          f"; all - solo {res[2][0] - res[0][0]:+.2f} us, none - solo {res[1][0] - res[0][0]:+.2f} us", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--out", default=os.path.join("profiles", "driven_step.txt"))
    ap.add_argument("--point", type=int, nargs=2, metavar=("B", "A"), help="(a child) measure this shape and print its line")
    a = ap.parse_args()
    if a.point:
        return point(a.point[0], a.point[1], a.reps)
    lines = ["tde_env_step_driven against the one-role step (scripts/measure_driven.py): HIP events around each call, four launches alternated "
             "in one process, median [min, max] in us.  solo = tde_env_step forced to its one-role kernel; none / all / one = "
             "tde_env_step_driven with driven NULL / every mask byte set / slot 1 of every env."]
    for B, A in POINTS:                                     # each under its own time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--point", str(B), str(A)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:
            sys.exit(f"measure_driven.py: the {B} x {A} shape ended with status {r.returncode}: nothing more is started")
        lines.append(r.stdout.strip().splitlines()[-1])
    with open(os.path.join(ROOT, a.out) if not os.path.isabs(a.out) else a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
