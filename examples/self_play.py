"""Self-play on the vector observation: one NPC slot of every env is driven by a policy that sees the scene from ITS seat
(BatchedWaypointEnv.agents -> AgentGroup.observe, tde_agent_obs), acts through step(action, agent_actions, driven)
(tde_env_step_driven) and is scored by AgentGroup.outcomes (tde_agent_outcomes): the reference's reward applied to the slot, plus
what became of it.  The policy is a stand-in for a network: steer toward the observed offset of the slot's next route waypoint, hold a
speed, brake when the ray straight ahead meets a car.  The ego is driven by the sampling planner.  Prints the mean reward per agent
step and the ended / collided / offroad / reached rates.

    python examples/self_play.py [num_envs] [steps] [slot]

The slot defaults to 2: in the synthetic world slot 1 replays a recorded trajectory and has no route, so its waypoint entries are zeros.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchdriveenv_amd.config import EnvConfig, VectorObs
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.synth import synthetic_world


def policy(obs, sl, v_target=6.0):
    """(acceleration, steering) float32 [n, 2] from the rows of AgentGroup.observe(); sl = VectorObs.slices()"""
    v = obs[:, sl["v"]].squeeze(1)
    fwd, left = obs[:, sl["target"]].unbind(1)
    steer = torch.atan2(left, fwd.clamp(min=1.0)).clamp(-0.3, 0.3)
    ahead = obs[:, sl["rays"]].reshape(obs.shape[0], -1, 3)[:, 0, 1]          # ray 0 points straight ahead; channel 1: the nearest car
    acc = torch.where(ahead < 8.0, torch.full_like(v, -4.0), (v_target - v).clamp(-2.0, 2.0))
    return torch.stack([acc, steer], -1)


def main():
    num_envs = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 400
    slot = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    env = BatchedWaypointEnv(EnvConfig(seed=0, distance_cutoff=0.25), world, num_envs=num_envs, obs_mode="state")
    env.reset()
    dev, B, A = env.torch_device, env.num_envs, env.A
    vo = VectorObs(k_neighbours=4, n_rays=8, ray_range=20.0, ray_step=0.5)
    group = env.agents(torch.arange(B), torch.full((B,), slot), vector_obs=vo)
    sl = vo.slices()
    agent_actions = torch.zeros(B, A, 2, device=dev)
    driven = torch.zeros(B, A, dtype=torch.bool, device=dev)
    driven[:, slot] = True
    stats = torch.zeros(6, dtype=torch.float64, device=dev)       # agent steps, reward, ended, collided, offroad, reached
    for _ in range(steps):
        agent_actions[:, slot] = policy(group.observe(), sl)         # (the row of an absent slot is zeros; its action is never read)
        env.step(env.plan_actions(), agent_actions, driven)
        out = group.outcomes()
        live = out.valid & ~out.ended
        stats += torch.stack([live.sum(), out.reward.double().sum(), out.ended.sum(), out.collided.sum(), out.offroad.sum(),
                              out.reached.sum()]).double()
    n, reward, ended, collided, offroad, reached = stats.tolist()
    print(f"slot {slot} of {B} envs driven from its own vector observation for {steps} steps: {int(n)} agent steps, mean reward "
          f"{reward / max(n, 1):+.4f}; per agent step: ended {ended / max(n + ended, 1):.2%}, collided {collided / max(n, 1):.2%}, "
          f"offroad {offroad / max(n, 1):.2%}, waypoint reached {reached / max(n, 1):.2%}")


if __name__ == "__main__":
    main()
