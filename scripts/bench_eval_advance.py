"""What an evaluation step costs next to a training step of the two-launch form, at 8192 envs x 16 agents on the junction maps:
tde_env_step without TDE_F_AUTORESET followed by tde_eval_advance (fold the step into the running episode records, record finished
episodes, re-spawn their envs to the next planned scenario) against the same step followed by tde_env_post_step with magnitudes =
NULL (the re-spawn alone).  Two envs with the same seed and the same resident actions, the two pairs ALTERNATED (post, eval, post,
eval, ...: seven passes, the median of each), HIP events around 100 pairs per sample, launches through the C++ extension.  Also the
two second launches alone on a state a step has just left.  Prints one JSON line (profiles/eval_advance.txt)."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torchdriveenv_amd import _abi, ops  # noqa: E402
from torchdriveenv_amd.config import EnvConfig  # noqa: E402
from torchdriveenv_amd.env import BatchedWaypointEnv  # noqa: E402
from torchdriveenv_amd.synth import synthetic_world  # noqa: E402

dev = torch.device("cuda:0")
B, A, R = (int(sys.argv[1]), int(sys.argv[2])) + (256,) if len(sys.argv) > 2 else (8192, 16, 256)


def sample_us(fn, n=100):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def alternated(fns, rounds, n=100, warm=20):
    for fn in fns.values():
        for _ in range(warm):
            fn()
    got = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            got[k].append(sample_us(fn, n))
    return {k: dict(us=statistics.median(v), samples=[round(x, 3) for x in v]) for k, v in got.items()}


world = synthetic_world(n_scn=64, A=A, seed=0)
cfg = EnvConfig(seed=3, distance_cutoff=0.25, max_environment_steps=200)
envs = {k: BatchedWaypointEnv(cfg, world, num_envs=B, agents_per_env=A, device=dev, obs_mode="state", auto_reset=False, info_magnitudes=False)
        for k in ("post", "eval")}
rng = np.random.default_rng(0)
act = torch.from_numpy(np.stack([rng.uniform(-0.2, 1, B), rng.uniform(-0.1, 0.1, B)], -1).astype(np.float32)).to(dev)
plan = rng.integers(0, world.n_scn, (R, B)).astype(np.int32)
ev = ops.EvalBuffers(plan, dev)
ev.active.fill_(1)
for e in envs.values():
    e.reset(options={"scenario": torch.from_numpy(plan[0])})
flags = int(envs["post"].tde_cfg.flags)
assert not flags & _abi.F_AUTORESET
hp, he = envs["post"]._h, envs["eval"]._h


def pair_post():
    hp.step(act, flags)
    hp.post_step(None, flags | _abi.F_AUTORESET)


def pair_eval():
    he.step(act, flags)
    he.eval_advance(ev.plan, ev.round, ev.active, ev.acc, ev.results, flags)


out = {"shape": f"{B}x{A}", "R": R}
out.update({f"step+{k}": v for k, v in alternated({"post_step": pair_post, "eval_advance": pair_eval}, rounds=7).items()})
out.update({f"{k}_alone": v for k, v in alternated({"post_step": lambda: hp.post_step(None, flags | _abi.F_AUTORESET),
                                                     "eval_advance": lambda: he.eval_advance(ev.plan, ev.round, ev.active, ev.acc, ev.results, flags),
                                                     "step": lambda: hp.step(act, flags)}, rounds=5).items()})
torch.cuda.synchronize()
rnd = ev.round.cpu().numpy()
out["episodes_recorded"] = int(rnd.sum())
out["envs_still_active"] = int(ev.active.sum())
out["max_round"] = int(rnd.max())
out["record_bytes_per_step"] = B * 48 * 2           # acc read + written per active env; a finished episode adds one 48-byte row
print(json.dumps(out))
