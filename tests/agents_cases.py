"""What the agents tests share (tests/test_agents_cpu.py, tests/test_gpu_agents.py): the closed loop observe -> step(driven=) -> outcomes
of a small batch, stated once so that the CPU file can show on the references alone (tests/driven_ref.py through test_gpu_driven's
ref_step, tests/agent_obs_ref.py) that the run holds every outcome flag, and the GPU file then runs the same scene.  A plain helper
module: nothing in the package imports it."""
import numpy as np

from tests import config_zoo
from torchdriveenv_amd import _abi

B, A, T, MAX_STEPS = 8, 16, 12, 5
FLAGS = config_zoo.FLAGS & ~_abi.F_TRAFFIC_LIGHTS          # (auto-reset on; without lights ref_step restates the whole step)


def loop_world():
    return config_zoo.world(None, A)


def loop_config():
    return config_zoo.config(None, A, flags=FLAGS, max_steps=MAX_STEPS)


def loop_stage(h):
    """edits the reset state (host dict) in place: in env 0 slot 1 stands half a car behind slot 2 at its heading, so the two collide at
    once and the ego, which they do not touch, keeps its episode"""
    x, y, psi, pres = (h[k].reshape(-1, A) for k in ("x", "y", "psi", "present"))
    assert pres[0, 1] and pres[0, 2]
    x[0, 1], y[0, 1], psi[0, 1] = x[0, 2] - np.float32(2.5) * np.cos(psi[0, 2]), y[0, 2] - np.float32(2.5) * np.sin(psi[0, 2]), psi[0, 2]


def loop_pairs():
    """every (env, slot), slot 0 included (reported invalid), then two pairs out of range and one duplicate"""
    e, a = np.divmod(np.arange(B * A), A)
    return np.concatenate([np.stack([e, a], -1), [[B, 1], [0, A], [3, 5]]]).astype(np.int32)


def loop_actions():
    """the fixed table: (agent_action float32 [B, A, 2], driven uint8 [B, A]).  In the even envs every NPC slot is driven - slots 1 mod 3
    straight ahead at full throttle (they run into what is in front of them), slots 2 mod 3 at full lock (they leave the road), the
    others coast; in the odd envs nobody is driven and the controller follows the routes (waypoints are reached)."""
    aa = np.zeros((B, A, 2), np.float32)
    aa[:, 1::3] = (6.0, 0.0)
    aa[:, 2::3] = (3.0, 0.6)
    drv = np.zeros((B, A), np.uint8)
    drv[0::2, 1:] = 1
    aa[drv == 0] = np.nan
    return aa, drv
