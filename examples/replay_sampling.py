"""Off-policy data flow on the GPU (the reference trainer's default algorithms, SAC and TD3, draw random batches of transitions
from a replay buffer: ref examples/rl_training.py:166-183): the scripted expert drives, every step is pushed into a device-resident
ReplayBuffer, and a batch is sampled - observations and next observations rebuilt from one stored layer plane per step.

    python examples/replay_sampling.py [num_envs] [steps] [capacity_steps]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchdriveenv_amd.config import EnvConfig
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.synth import synthetic_world


def main():
    num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    capacity = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    cfg = EnvConfig(seed=0, distance_cutoff=0.25, frame_stack=3)
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    # terminal_obs=True: the env observes a finished episode before it re-spawns it, and the buffer pools that frame
    env = BatchedWaypointEnv(cfg, world, num_envs=num_envs, frame_stack=3, terminal_obs=True)
    buf = env.replay_buffer(capacity_steps=capacity)   # terminal_per_step=: pool rows per step (default num_envs // 8)
    env.reset()
    buf.begin()
    for _ in range(steps):
        actions = env.plan_actions()                   # policy(obs) goes here
        env.step(actions)
        buf.push(actions)
    batch = buf.sample(256)                            # SB3's ReplayBufferSamples fields, on the device
    torch.cuda.synchronize()
    for name in batch._fields:
        t = getattr(batch, name)
        print(f"{name:18s} {str(t.dtype):14s} {tuple(t.shape)}")
    print(f"{len(buf)} transitions held ({buf.count} steps x {num_envs} envs), {int(batch.terminal.sum())} of the 256 drawn ended their episode")
    # where .bootstrap is set, next_observations is what the learner bootstraps from - for a truncated episode, its terminal observation
    print(f"{int(batch.bootstrap.sum())} of them bootstrap from next_observations ({int((batch.bootstrap & batch.terminal).sum())} truncated, from the terminal observation)")
    # the n-step target of the same learner: rewards summed over up to three steps, cut short where the episode stopped
    nb = buf.sample_nstep(256, n_steps=3, gamma=0.99)
    q_next = torch.zeros(256, device=nb.rewards.device)  # Q(nb.next_observations, policy(nb.next_observations)) goes here
    target = nb.rewards + nb.discounts * nb.bootstrap * q_next
    print(f"n-step: target {tuple(target.shape)}, steps taken {torch.bincount(nb.steps.long(), minlength=4).tolist()[1:]} (1, 2, 3)")
    stacked = 2 * batch.observations[0].numel() * batch.observations.element_size()
    print(f"bytes held per transition: {buf.bytes_per_transition} (a store of stacked obs + next_obs: {stacked})")


if __name__ == "__main__":
    main()
