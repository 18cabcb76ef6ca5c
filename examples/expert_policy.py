"""A scripted expert in closed loop: the sampling planner (BatchedWaypointEnv.plan_actions, tde_plan_action) drives every ego of a
batch; the rates the reference trainer's evaluation callback logs (ref examples/rl_training.py:23-119: success, offroad, collision,
red light) are printed and, with a file name, the (observation, action) pairs are saved for behaviour cloning.

    python examples/expert_policy.py [--refine] [--predict constant|route] [num_envs] [steps] [pairs.npz]
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchdriveenv_amd.config import EnvConfig, Planner, PlanRefine
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.synth import synthetic_world


def main():
    args = [a for a in sys.argv[1:] if a != "--refine"]
    predict = "constant"                                            # --predict route: the others by tde_forecast_agents (Planner.predict)
    if "--predict" in args:
        i = args.index("--predict")
        predict = args[i + 1]
        del args[i:i + 2]
    refine = PlanRefine() if "--refine" in sys.argv[1:] else None   # --refine: brake tail + knot refinement (tde_score_plans)
    num_envs = int(args[0]) if len(args) > 0 else 1024
    steps = int(args[1]) if len(args) > 1 else 400
    save = args[2] if len(args) > 2 else None
    cfg = EnvConfig(seed=0, distance_cutoff=0.25)
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)               # or a WaypointSuite from the loaders
    env = BatchedWaypointEnv(cfg, world, num_envs=num_envs, obs_mode="vector", planner=Planner(predict=predict), plan_refine=refine)
    obs = env.reset()
    stats = torch.zeros(6, dtype=torch.float64, device=obs.device)   # episodes, infraction ends, offroad, collision, red light, waypoints
    pairs = []
    for _ in range(steps):
        action = env.plan_actions()                                  # float32 [B, 2] on the device
        if save:
            pairs.append((obs.cpu().numpy().copy(), action.cpu().numpy().copy()))
        obs, reward, terminated, truncated, info = env.step(action)
        bits = env.state["done_bits"].to(torch.int64)                # the ego's flags of this step, before any re-spawn
        done = ((bits & 3) != 0).double()
        stats += torch.stack([done.sum(), (done * (bits & 1)).sum(), (done * ((bits >> 2) & 1)).sum(), (done * ((bits >> 3) & 1)).sum(),
                              (done * ((bits >> 4) & 1)).sum(), (done * env.state["info_reached"].double()).sum()])
    n, inf, off, col, red, wps = stats.tolist()
    print(f"{num_envs} envs x {steps} steps under the {'refined ' if refine else ''}planner: {int(n)} episodes")
    if n:
        print(f"success {1 - inf / n:.1%}, offroad {off / n:.1%}, collision {col / n:.1%}, red light {red / n:.1%}, "
              f"{wps / n:.2f} waypoints per episode")
    if save:
        np.savez_compressed(save, obs=np.concatenate([p[0] for p in pairs]), action=np.concatenate([p[1] for p in pairs]))
        print(f"saved {len(pairs) * num_envs} (observation, action) pairs to {save}")


if __name__ == "__main__":
    main()
