"""On-policy data flow on the GPU (PPO and A2C, the reference trainer's other two algorithms: ref examples/rl_training.py with
env_configs/<name>/{ppo,a2c}_training.yml): a random "policy" returns actions, values and log-probabilities, every step is pushed into
a device-resident RolloutBuffer, one launch computes advantages and returns, and two epochs of minibatches are gathered -
observations rebuilt from one stored layer plane per step.

    python examples/ppo_rollout.py [num_envs] [n_steps]
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
    n_steps = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    cfg = EnvConfig(seed=0, distance_cutoff=0.25, frame_stack=3)
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    # terminal_obs=True: a truncated episode (the success case: max_environment_steps reached) can bootstrap from its terminal observation
    env = BatchedWaypointEnv(cfg, world, num_envs=num_envs, frame_stack=3, terminal_obs=True)
    dev = env.torch_device
    gen = torch.Generator(device=dev).manual_seed(0)
    low, high = (torch.tensor(v, device=dev) for v in (env.action_space.low, env.action_space.high))

    def policy(obs):
        """actor and critic go here: actions [B, 2], values [B], log-probabilities [B]"""
        actions = low + (high - low) * torch.rand(num_envs, 2, device=dev, generator=gen)
        return actions, torch.randn(num_envs, device=dev, generator=gen), -torch.rand(num_envs, device=dev, generator=gen)

    buf = env.rollout_buffer(n_steps, gamma=0.99, gae_lambda=0.95)
    obs = env.reset()
    buf.begin()
    for _ in range(n_steps):
        actions, values, log_probs = policy(obs)
        obs, *_ = env.step(actions)
        buf.push(actions, values, log_probs)
        envs, term_obs = buf.terminal_observations()   # the envs this step truncated, and what they showed before the re-spawn
        if len(envs):
            buf.bootstrap(envs, policy(term_obs)[1][:len(envs)])       # reward += gamma * V(terminal observation), as SB3 does
    buf.finish(policy(obs)[1])                         # the critic's value of the observation after the last step
    for epoch in range(2):
        n = batches = 0
        for batch in buf.get(256):                     # a fresh permutation of all n_steps * num_envs samples per epoch
            n, batches = n + batch.indices.numel(), batches + 1
        print(f"epoch {epoch}: {batches} batches, {n} samples")
    torch.cuda.synchronize()
    for name in batch._fields:
        t = getattr(batch, name)
        print(f"{name:14s} {str(t.dtype):14s} {tuple(t.shape)}")
    stacked = batch.observations[0].numel() * batch.observations.element_size()
    print(f"{len(buf)} samples held ({n_steps} steps x {num_envs} envs); bytes held per sample: {buf.ring.bytes_per_transition + 16} "
          f"(a store of stacked observations: {stacked + 32}); mean advantage {float(buf.advantages.mean()):+.4f}")


if __name__ == "__main__":
    main()
