"""Record a few envs of a training batch without rendering inside the loop, and branch one env into several: per step the recorder copies
the chosen envs' state rows into a trace on the device (one small launch, a few hundred bytes per env); the frames are rendered after
the loop by the scene renderer and written through video.save_video.  Then a snapshot is taken, the batch is driven on, the snapshot is
put back and the same steps give the same rewards bit for bit; and one env is forked into three that are given different actions.

    python examples/record_video.py [num_envs] [steps] [out.mp4]
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
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    out = sys.argv[3] if len(sys.argv) > 3 else "recorded.mp4"
    cfg = EnvConfig(seed=0, distance_cutoff=0.25, frame_stack=3)
    world = synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)
    env = BatchedWaypointEnv(cfg, world, num_envs=num_envs, frame_stack=3)
    env.reset()
    rec = env.recorder([0, 1, 2, 3], video_length=steps + 1)
    rec.capture()                                           # the frame after reset()
    for t in range(steps):
        env.step(env.plan_actions())                        # policy(obs) goes here
        rec.capture()                                       # a finished env was re-spawned in the step: its new episode's first frame
    path = rec.save(out, tile=True, H=256, W=256, fov=120.0, camera="ego")
    print(f"{len(rec)} frames of envs {rec.envs} -> {path}")

    # snapshot, drive on, restore, drive again: the same rewards, bit for bit
    keep = [5, 9]
    snap = env.snapshot(keep)
    actions = [env.plan_actions().clone() for _ in range(1)] * 10
    first = [env.step(a)[1][keep].clone() for a in actions]
    env.restore(snap)
    again = [env.step(a)[1][keep].clone() for a in actions]
    print("restored envs repeat their rewards:", all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(first, again)))

    # fork env 5 into envs 6, 7, 8 and steer the copies apart
    env.fork(5, [6, 7, 8])
    a = env.plan_actions().clone()
    a[6:9, 1] = torch.tensor([-0.3, 0.0, 0.3], device=a.device)
    _, reward, *_ = env.step(a)
    print("rewards of env 5 and its three branches after one step:", reward[5:9].tolist())


if __name__ == "__main__":
    main()
