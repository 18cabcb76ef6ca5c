"""A scripted adversary: whichever NPC drives in the ego's lane within 30 m ahead of it is taken over and brakes hard
(BatchedWaypointEnv.step(action, agent_actions, driven), tde_env_step_driven); every other slot, and the same slot once the ego is past
it, stays with the built-in controller.  The ego is driven by the sampling planner (plan_actions), which predicts the others at
constant velocity and so does not expect the brake.  The ego's collision rate per episode is printed with and without the adversary.

    python examples/driven_agents.py [num_envs] [steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchdriveenv_amd.config import EnvConfig
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.synth import synthetic_world


def brake_ahead_of_ego(env, agent_actions, driven, reach=30.0, lane=2.0, brake=-8.0):
    """fill the mask and the actions in place from the state on the device: the present NPCs inside the box ahead of their env's ego"""
    st, B, A = env.state, env.num_envs, env.A
    x, y, psi = (st[k].view(B, A) for k in ("x", "y", "psi"))
    dx, dy = x - x[:, :1], y - y[:, :1]
    c, s = torch.cos(psi[:, :1]), torch.sin(psi[:, :1])
    fwd, lat = dx * c + dy * s, dy * c - dx * s
    torch.logical_and((fwd > 0) & (fwd < reach) & (lat.abs() < lane), st["present"].view(B, A) != 0, out=driven)
    driven[:, 0] = False                                            # (row 0 is never read: the ego's action is `action`)
    agent_actions[..., 0] = brake                                   # only the rows of driven slots are read
    agent_actions[..., 1] = 0.0


def run(env, steps, adversary):
    env.reset()
    dev = env.torch_device
    agent_actions = torch.zeros(env.num_envs, env.A, 2, device=dev)
    driven = torch.zeros(env.num_envs, env.A, dtype=torch.bool, device=dev)
    stats = torch.zeros(3, dtype=torch.float64, device=dev)          # episodes, ended by a collision, steps with a driven slot
    for _ in range(steps):
        action = env.plan_actions()
        if adversary:
            brake_ahead_of_ego(env, agent_actions, driven)
            env.step(action, agent_actions, driven)
        else:
            env.step(action)
        bits = env.state["done_bits"].to(torch.int64)                # the ego's flags of this step, before any re-spawn
        done = ((bits & 3) != 0).double()
        stats += torch.stack([done.sum(), (done * ((bits >> 3) & 1)).sum(), driven.any(1).double().sum()])
    return stats.tolist()


def main():
    num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 400
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    for adversary in (False, True):
        env = BatchedWaypointEnv(EnvConfig(seed=0, distance_cutoff=0.25), world, num_envs=num_envs, obs_mode="state")
        n, col, taken = run(env, steps, adversary)
        print(f"{'with' if adversary else 'without'} the braking adversary: {int(n)} episodes of {num_envs} envs x {steps} steps, "
              f"{col / max(n, 1):.1%} ended by a collision of the ego" + (f"; a slot was driven in {taken / (num_envs * steps):.1%} of the env steps" if adversary else ""))


if __name__ == "__main__":
    main()
