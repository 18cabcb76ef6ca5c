"""Evaluate a policy on chosen suite cases: the planner (BatchedWaypointEnv.plan_actions) runs every case of the validation suite
once per repeat and the nine values the reference trainer's EvalNTimestepsCallback logs (ref examples/rl_training.py:96-108) are
printed.  Every case is run - not a random draw of cases - and whole-episode results are collected on the GPU (tde_env_reset_to,
tde_eval_advance).

    python examples/evaluate_policy.py [validation_cases.yml] [num_envs] [repeats]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from torchdriveenv_amd.config import EnvConfig, Planner
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.loaders import load_waypoint_suite_data


def main():
    args = sys.argv[1:]
    path = args[0] if len(args) > 0 else os.path.join(ROOT, "tests", "golden", "reference_data", "validation_cases.yml")
    num_envs = int(args[1]) if len(args) > 1 else 16
    repeats = int(args[2]) if len(args) > 2 else 1
    data = load_waypoint_suite_data(path)
    cfg = EnvConfig(seed=0, distance_cutoff=0.25, use_background_traffic=False)
    # a second env next to the training env, as the reference builds its eval_val_env; a policy network goes where "planner" is:
    # any callable observation -> float32 [num_envs, 2] actions on the device
    env = BatchedWaypointEnv(cfg, data, num_envs=num_envs, agents_per_env=16, obs_mode="vector", planner=Planner())
    result = env.evaluate("planner", repeats=repeats)
    print(f"{len(result)} episodes: {env.world.n_scn} cases of {os.path.basename(path)} x {repeats} on {num_envs} envs")
    for name, value in result.metrics().items():
        print(f"{name:>30} {value:.6g}")
    worst = result.episode_return.argmin().item()
    print(f"lowest return: case {int(result.scenario[worst])}, {float(result.episode_return[worst]):.2f} in {int(result.length[worst])} steps, "
          f"done bits {int(result.bits[worst]):#04x}")


if __name__ == "__main__":
    main()
