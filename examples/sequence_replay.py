"""Sequence replay for a recurrent learner (DRQN, R2D2, recurrent SAC / TD3): the policy must remember what it saw - a car that drove
behind an occluder - so it learns from windows of consecutive steps of one env, not from single transitions.  The scripted expert
drives, every step is pushed, and each learner step draws windows of up to T steps; a window stops where its episode stopped.  Inside a
window the learner forms n-step targets from the per-step rewards with `mask`, and bootstraps behind the last step where `bootstrap`
says so.

    python examples/sequence_replay.py [num_envs] [steps] [capacity_steps] [T]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchdriveenv_amd.config import EnvConfig
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.synth import synthetic_world


def nstep_targets(batch, q, n, gamma):
    """float32 [N, T]: the n-step target of every step of every window from the values q [N, T + 1] of its observations - the rewards of
    up to n steps that the window holds, then gamma^j * q of the observation behind them; behind the window's last step only where
    batch.bootstrap (an ended episode has nothing to bootstrap from, a truncated one has its terminal observation)"""
    N, T = batch.rewards.shape
    L = batch.lengths.long()[:, None]
    k = torch.arange(T, device=q.device)[None, :]
    r = batch.rewards * batch.mask                          # (zeros behind the length already; the mask says so)
    target, disc = torch.zeros_like(r), torch.ones_like(r)
    for j in range(n):
        inside = k + j < L
        target = target + disc * torch.where(inside, r.gather(1, (k + j).clamp(max=T - 1)), torch.zeros_like(r))
        disc = torch.where(inside, disc * gamma, disc)
    end = torch.minimum(k + n, L.expand(N, T))              # the observation the target bootstraps from
    boot = (end < L) | batch.bootstrap[:, None]
    return (target + disc * boot * q.gather(1, end)) * batch.mask


def main():
    num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    capacity = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    T = int(sys.argv[4]) if len(sys.argv) > 4 else 20
    cfg = EnvConfig(seed=0, distance_cutoff=0.25, frame_stack=3)
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    env = BatchedWaypointEnv(cfg, world, num_envs=num_envs, frame_stack=3, terminal_obs=True)
    buf = env.replay_buffer(capacity_steps=capacity)
    env.reset()
    buf.begin()
    for t in range(steps):
        actions = env.plan_actions()                        # policy(obs, hidden) goes here
        env.step(actions)
        buf.push(actions)
        if t < T + 2:
            continue
        batch = buf.sample_sequence(32, T)                  # a burn-in of b steps: draw b + T and slice
        # the recurrent critic unrolled over batch.observations [32, T + 1, 9, 64, 64] goes here; a stand-in:
        q = batch.observations.float().mean(dim=(2, 3, 4)) / 255.0
        target = nstep_targets(batch, q, n=3, gamma=0.99)
        td = (target - q[:, :T]) * batch.mask
        loss = (td ** 2).sum() / batch.mask.sum()           # loss.backward() goes here
    torch.cuda.synchronize()
    for name in ("observations", "actions", "rewards", "dones", "lengths", "indices"):
        v = getattr(batch, name)
        print(f"{name:14s} {str(v.dtype):14s} {tuple(v.shape)}")
    print(f"mask {tuple(batch.mask.shape)}: {int(batch.mask.sum())} of {batch.mask.numel()} steps; lengths {batch.lengths.tolist()}")
    print(f"bootstrap behind the last step: {int(batch.bootstrap.sum())} of 32 windows ({int(batch.terminal.sum())} ended, "
          f"{int((batch.terminal & batch.bootstrap).sum())} of them truncated with their terminal observation kept); last loss {float(loss):.5f}")


if __name__ == "__main__":
    main()
