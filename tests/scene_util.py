"""Helpers of the tde_render_scene tests: the oracle renders only ego-centred views (oracle.render_ego), so a view from any camera
pose is the oracle's ego view of a copy of the env in which a PHANTOM ego - absent, so never painted - stands at the camera pose and
the real ego has moved to a free agent slot.  With TDE_RENDER_PLAIN_EGO every agent has one colour, so the move does not show."""
import numpy as np

from oracle import oracle
from torchdriveenv_amd import _abi
from torchdriveenv_amd.state import EnvState

EGO_RGB = np.array(_abi.PALETTE[4], np.uint8)
NPC_RGB = np.array(_abi.PALETTE[3], np.uint8)


def env_slice(h, e, B, A):
    """the arrays of env e of a state's host dict (agent arrays [B * A], env arrays [B]) as a one-env dict"""
    out = {}
    for k, a in h.items():
        if a.shape[0] == B * A and A > 1:
            out[k] = a[e * A:(e + 1) * A].copy()
        elif a.shape[0] == B:
            out[k] = a[e:e + 1].copy()
    return out


def one_env_state(h, e, B, A):
    st = EnvState(1, A)
    st.load(env_slice(h, e, B, A))
    return st


def oracle_ego_views(cfg, world, h, B, A, envs, H, W, fov, flags):
    """oracle.render_ego of env envs[i] -> uint8 [n, 3, H, W]"""
    return np.stack([oracle.render_ego(cfg, world, one_env_state(h, e, B, A), H, W, fov, flags=flags)[0] for e in envs])


def phantom_state(h, e, B, A, pose):
    """one-env state of env e with slot 0 = an absent phantom at `pose` (x, y, psi) and the real ego moved into a free slot"""
    d = env_slice(h, e, B, A)
    free = np.flatnonzero(d["present"][1:] == 0)
    assert len(free), "no free agent slot for the real ego"
    j = 1 + int(free[0])
    for k, a in d.items():
        if a.shape[0] == A:
            a[j] = a[0]
    d["x"][0], d["y"][0], d["psi"][0] = np.float32(pose[0]), np.float32(pose[1]), np.float32(pose[2])
    d["present"][0] = 0
    st = EnvState(1, A)
    st.load(d)
    return st


def free_last_slot(h, B, A):
    """host dict with agent slot A - 1 of every env absent (load it into the device state too: both then hold a free slot)"""
    h = {k: v.copy() for k, v in h.items()}
    h["present"].reshape(B, A)[:, A - 1] = 0
    return h


def oracle_scene_views(cfg, world, h, B, A, envs, poses, H, W, fov, flags):
    """the oracle's view of env envs[i] from camera poses[i], painted with TDE_RENDER_PLAIN_EGO -> uint8 [n, 3, H, W]"""
    return np.stack([oracle.render_ego(cfg, world, phantom_state(h, e, B, A, p), H, W, fov,
                                       flags=flags | _abi.RENDER_PLAIN_EGO)[0] for e, p in zip(envs, poses)])


def ego_as_npc(img):
    """uint8 [..., 3, H, W]: pixels of the ego's colour recoloured as an NPC's"""
    img = np.array(img, copy=True)
    hw = np.moveaxis(img, -3, -1)
    hw[(hw == EGO_RGB).all(-1)] = NPC_RGB
    return img
