"""Prioritized experience replay on the GPU (Schaul et al.; what Rainbow, Ape-X and R2D2 add to the replay buffer): here the reward is
a sparse waypoint bonus and an episode ends on the first infraction, so most stored transitions carry no signal - the learner draws
the ones its critic is wrong about.  A SAC-shaped loop: the scripted expert drives, every step is pushed, and each learner step draws a
batch in proportion to the priorities, computes a TD error (a stand-in here) and hands it back.

    python examples/prioritized_replay.py [num_envs] [steps] [capacity_steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchdriveenv_amd.config import EnvConfig, Prioritized
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.synth import synthetic_world


def main():
    num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    capacity = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    cfg = EnvConfig(seed=0, distance_cutoff=0.25, frame_stack=3)
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    env = BatchedWaypointEnv(cfg, world, num_envs=num_envs, frame_stack=3, terminal_obs=True)
    buf = env.replay_buffer(capacity_steps=capacity, prioritized=Prioritized(alpha=0.6, beta=0.4))
    env.reset()
    buf.begin()
    rewarded = 0
    for t in range(steps):
        actions = env.plan_actions()                   # policy(obs) goes here
        env.step(actions)
        buf.push(actions)                              # the new transitions enter with the largest priority seen
        if t < 8:
            continue
        beta = 0.4 + 0.6 * t / steps                   # annealed to 1, as the paper does
        batch = buf.sample_prioritized(256, n_steps=3, gamma=0.99, beta=beta)
        q_next = torch.zeros(256, device=batch.rewards.device)          # Q(batch.next_observations, policy(...)) goes here
        q_now = torch.zeros(256, device=batch.rewards.device)           # Q(batch.observations, batch.actions)
        td = batch.rewards + batch.discounts * batch.bootstrap * q_next - q_now
        loss = (batch.weights * td ** 2).mean()        # the importance weights undo the bias of the draw; loss.backward() goes here
        buf.update_priorities(batch.indices, td)       # p = (|td| + eps) ** alpha
        rewarded += int((batch.rewards != 0).sum())
    torch.cuda.synchronize()
    for name in batch._fields:
        v = getattr(batch, name)
        print(f"{name:18s} {str(v.dtype):14s} {tuple(v.shape)}")
    uniform = buf.sample_nstep(4096, 3)
    print(f"{len(buf)} transitions held; priorities from {int(buf.leaf[buf.leaf > 0].min())} to {int(buf.qmax)} (65536 = 1.0); last loss {float(loss):.4f}")
    print(f"drawn transitions with a nonzero reward: {rewarded / (256 * max(1, steps - 8)):.1%} of the prioritized batches, "
          f"{float((uniform.rewards != 0).float().mean()):.1%} of a uniform one")


if __name__ == "__main__":
    main()
