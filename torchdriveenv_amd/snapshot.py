"""Snapshots, restores, forks and recordings of chosen envs of a BatchedWaypointEnv, all made of one entry point, tde_state_copy
(include/tde_snapshot.h): env rows of one tde_state into env rows of another, or of the same one, in one launch, with the destination
rows' caches invalidated in that launch.

What a row is.  Everything a BatchedWaypointEnv keeps per env and that outlives a step: the state arrays (agents, counters, the step's
outputs, the routes of near-field agents in slot_route), the frame-stack ring and the stacked observation, the single-frame birdview of
an env without a stack, the vector observation's row, and the terminal frame of a terminal_obs env.  Nothing else is per env: the
planner's, the near-field spawner's and the terminal stash's buffers are scratch rewritten by every call, evaluate() keeps its schedule
in buffers of its own for the length of the call, and replay / rollout buffers are not part of a snapshot.

The RNG rule.  The only random draws of the env - the re-spawn's (scenario, start point, speed, heading noise) and the near-field
spawner's - are Philox streams keyed by (seed, GLOBAL env index = tde_config.env_base + row, episode counter); nothing else in the
kernels is keyed by the env index.  The episode counter is part of the row, the index is not.  So a row restored into the index it came
from continues bit for bit, for ever; a row put into another index (fork(), restore(envs=other)) continues bit for bit until that env
next re-spawns, and then draws from ITS index's stream with the copied episode counter."""
import os

import numpy as np
import torch

from . import _abi, ops
from .state import EnvState


def _as_rows(envs, B, what="envs"):
    """the env indices as a list of ints, checked against [0, B) and for duplicates (host values: they name the snapshot)"""
    if torch.is_tensor(envs):
        envs = envs.detach().cpu().tolist()
    rows = [int(e) for e in (envs if np.ndim(envs) else [envs])]
    if not rows:
        raise ValueError(f"{what} is empty")
    if any(e < 0 or e >= B for e in rows):
        raise ValueError(f"{what} must be in [0, {B})")
    if len(set(rows)) != len(rows):
        raise ValueError(f"{what} names an env twice")
    return rows


def _like(state):
    """EnvState's keywords for a state with the optional arrays `state` carries, and no caches"""
    a = state.arrays
    return dict(with_info=a["info"] is not None, with_obs=a["obs"] is not None, with_episode=a["ep_return"] is not None, with_cache=False,
                with_magnitudes=a["magnitudes"] is not None, with_slot_route=a["slot_route"] is not None)


def _handle_for(venv, state):
    """a launch handle of `state` in the binding `venv` launches through"""
    if venv.binding == "ext":
        from . import _ext

        return _ext.env_handle(venv.tde_cfg, venv.dworld, state)
    return ops.CtypesHandle(venv.tde_cfg, venv.dworld, state)


class EnvSnapshot(EnvState):
    """`len(envs)` env rows of a BatchedWaypointEnv, taken by venv.snapshot(envs): an EnvState of that many rows without caches (row i =
    env envs[i] at the time of the call, the step's outputs included), plus

        envs             the indices the rows were taken from (list of int), envs_t the same as an int32 device tensor
        layers, obs      the rows of the frame-stack ring, turned so that the snapshot's ring phase is 0, and of the stacked observation
                         (birdview envs that have been observed; layers is None without a frame stack)
        vector           the rows of the vector observation (obs_mode "vector")
        terminal_frames  the rows of the env's terminal frames (terminal_obs=True)

    The compact observation of obs_mode "state" is the state's own `obs` array.  torch.save of `arrays` and these tensors serialises it."""

    def __init__(self, venv, envs):
        rows = _as_rows(envs, venv.num_envs)
        src = venv.state
        dev = venv.torch_device
        EnvState.__init__(self, len(rows), src.A, device=dev, **_like(src))
        self.envs = rows
        self.envs_t = torch.tensor(rows, dtype=torch.int32, device=dev)
        self._own = torch.arange(len(rows), dtype=torch.int32, device=dev)
        self._handle = _handle_for(venv, self)
        self.layers = self.obs = self.vector = self.terminal_frames = None
        self.n_stack = self.plane = 0
        layers, obs, ns, plane, phase = venv.observer.frames()
        frames = None
        if obs is not None:
            self.n_stack, self.plane = ns, plane
            if layers is not None:
                self.layers = torch.empty((len(rows), ns, plane), dtype=torch.uint8, device=dev)
            self.obs = torch.empty((len(rows),) + tuple(obs.shape[1:]), dtype=torch.uint8, device=dev)
            frames = ops.snapshot_frames(layers, self.layers, obs, self.obs, ns, plane, phase, 0)
        ops.state_copy(src, self, self.envs_t, self._own, frames=frames, outputs=True, check=False, handles=(venv._h, self._handle))
        self.vector, self.terminal_frames = (None if t is None else t.index_select(0, self.envs_t.long())
                                             for t in (venv.observer.rows, venv.terminal_frames))


def restore(venv, snap, envs=None):
    """venv.restore(snap, envs=None)"""
    if not isinstance(snap, EnvSnapshot):
        raise ValueError("restore() takes an EnvSnapshot made by snapshot()")
    if snap.A != venv.A:
        raise ValueError(f"the snapshot has {snap.A} agent slots per env, this env {venv.A}")
    rows = snap.envs if envs is None else _as_rows(envs, venv.num_envs)
    if len(rows) != snap.B:
        raise ValueError(f"the snapshot holds {snap.B} rows, envs names {len(rows)}")
    if max(rows) >= venv.num_envs:
        raise ValueError(f"envs must be in [0, {venv.num_envs})")
    dst = venv.state
    for n, arr in snap.arrays.items():
        if n not in _abi.SNAPSHOT_INVALIDATED and (arr is None) != (dst.arrays[n] is None):
            raise ValueError(f"the snapshot {'lacks' if arr is None else 'carries'} the state array {n!r} and this env does not: it was "
                             "taken from an env built with other options")
    if (snap.vector is None) != (venv.observer.rows is None) or (snap.terminal_frames is None) != (venv.terminal_frames is None):
        raise ValueError("the snapshot was taken from an env with another obs_mode or terminal_obs setting")
    layers, obs, ns, plane, phase = venv.observer.frames()
    frames = None
    if snap.obs is not None:
        if obs is None and venv.observer.plane:
            venv.get_obs()                                       # the env has not been observed yet: its buffers come into being
            layers, obs, ns, plane, phase = venv.observer.frames()
        if obs is None or (ns, plane) != (snap.n_stack, snap.plane) or (layers is None) != (snap.layers is None):
            raise ValueError("the snapshot's frames (frame_stack, resolution) do not fit this env's")
        frames = ops.snapshot_frames(snap.layers, layers, snap.obs, obs, ns, plane, 0, phase)
    elif obs is not None:
        raise ValueError("the snapshot was taken before the env's first observation and holds no frames, this env has been observed: "
                         "its frame buffers (the observer's frame / frame stack) would keep the overwritten envs' frames")
    rows_t = snap.envs_t if envs is None else torch.tensor(rows, dtype=torch.int32, device=venv.torch_device)
    ops.state_copy(snap, dst, snap._own, rows_t, frames=frames, outputs=True, check=False, handles=(snap._handle, venv._h))
    for live, saved in ((venv.observer.rows, snap.vector), (venv.terminal_frames, snap.terminal_frames)):
        if saved is not None:
            live.index_copy_(0, rows_t.long(), saved)
    return venv.observer.current()


def fork(venv, src_env, dst_envs):
    """venv.fork(src_env, dst_envs)"""
    s = _as_rows(src_env, venv.num_envs, "src_env")
    if len(s) != 1:
        raise ValueError("fork() copies ONE env: src_env is a single index")
    d = _as_rows(dst_envs, venv.num_envs, "dst_envs")
    if s[0] in d:
        raise ValueError(f"dst_envs holds src_env ({s[0]}): a fork writes other envs")
    dev = venv.torch_device
    se, de = torch.full((len(d),), s[0], dtype=torch.int32, device=dev), torch.tensor(d, dtype=torch.int32, device=dev)
    layers, obs, ns, plane, phase = venv.observer.frames()
    frames = ops.snapshot_frames(layers, layers, obs, obs, ns, plane, phase, phase) if obs is not None else None
    ops.state_copy(venv.state, venv.state, se, de, frames=frames, outputs=True, check=False, handles=(venv._h, venv._h))
    for live in (venv.observer.rows, venv.terminal_frames):
        if live is not None:
            live[de.long()] = live[s[0]]
    return venv.observer.current()


class EpisodeRecorder:
    """venv.recorder(envs, video_length=200): records the state rows of `envs` step by step and renders them afterwards.

    capture() - call it after each reset() or step() - writes the rows into time slot t of a trace, a plain EnvState of
    len(envs) * video_length rows (slot t, recorded env i -> row t * len(envs) + i), with ONE tde_state_copy launch and nothing else: a few
    hundred bytes per env and step, no rendering inside the loop.  frames() renders the trace with the scene renderer as it is
    (tde_render_scene on the trace state), save() writes a file.  Once video_length slots are full capture() returns False and records
    nothing.

    A finished env is re-spawned inside the step, so the frame captured after a done step is the NEW episode's first one - as with SB3's
    VecVideoRecorder, whose frame after a done step shows the reset env.  The traffic-light colours of a frame follow from the recorded
    step counter; the trace does not hold the frame stack or any observation."""

    def __init__(self, venv, envs, video_length=200):
        self.venv = venv
        self.envs = _as_rows(envs, venv.num_envs)
        self.video_length = int(video_length)
        if self.video_length < 1:
            raise ValueError("video_length must be >= 1")
        n, dev = len(self.envs), venv.torch_device
        self.trace = EnvState(n * self.video_length, venv.state.A, device=dev, **_like(venv.state))
        self._handle = _handle_for(venv, self.trace)
        self._src = torch.tensor(self.envs, dtype=torch.int32, device=dev)
        self._slots = torch.arange(n * self.video_length, dtype=torch.int32, device=dev).reshape(self.video_length, n)
        self.t = 0

    def __len__(self):
        return self.t

    def capture(self):
        """record the envs as they are now into the next time slot; False (and nothing recorded) once the trace is full"""
        if self.t >= self.video_length:
            return False
        ops.state_copy(self.venv.state, self.trace, self._src, self._slots[self.t], outputs=False, check=False,
                       handles=(self.venv._h, self._handle))
        self.t += 1
        return True

    def clear(self):
        """start over at slot 0 (the trace's memory is reused)"""
        self.t = 0

    def frames(self, H=1024, W=1024, fov=500.0, camera="map", chunk=16, env=None):
        """uint8 [t, n, 3, H, W] on the device: the recorded steps of the recorded envs (env=i: of recorded env i alone, [t, 1, 3, H, W]),
        rendered `chunk` time slots per tde_render_scene launch exactly as venv.render_scene(envs, H, W, fov, camera) would have rendered
        them live.  camera: "map", "ego" or a float32 tensor [n, 3] used for every slot."""
        v = self.venv
        n = len(self.envs)
        cols = list(range(n)) if env is None else [_as_rows(env, n, "env")[0]]
        out = torch.empty((self.t, len(cols), 3, int(H), int(W)), dtype=torch.uint8, device=v.torch_device)
        chunk = max(1, int(chunk))
        for t0 in range(0, self.t, chunk):
            t1 = min(self.t, t0 + chunk)
            rows = self._slots[t0:t1][:, cols].reshape(-1)
            cam = camera[cols].repeat(t1 - t0, 1).contiguous() if torch.is_tensor(camera) else camera
            ops.render_scene(v.tde_cfg, v.dworld, self.trace, rows, H, W, fov, cam, out[t0:t1].view(-1, 3, int(H), int(W)),
                             flags=v._rflags, check_envs=False)
        return out

    def save(self, path, env=0, tile=False, fps=10, **render):
        """write the recording of recorded env `env` (an index into `envs`) to `path` through video.save_video (cv2's mp4, an animated GIF
        beside it with only PIL, ImportError with neither) and return the path written; tile=True: a mosaic of all recorded envs, laid
        out like SB3's VecEnv.render tiles its images (tile_frames).  `render`: the arguments of frames()."""
        from .video import save_video

        if self.t < 1:
            raise ValueError("nothing recorded: call capture() after reset() / step()")
        fr = self.frames(env=None if tile else env, **render)
        fr = tile_frames(fr) if tile else fr[:, 0]
        return save_video([f[None] for f in fr], path, fps=fps)


def tile_frames(fr):
    """[t, n, 3, H, W] -> [t, 3, rows * H, cols * W]: the n views of each time slot as one image, rows = ceil(sqrt(n)), cols =
    ceil(n / rows), filled row by row, empty tiles black - the layout of stable_baselines3's tile_images"""
    t, n, c, H, W = fr.shape
    rows = int(np.ceil(np.sqrt(n)))
    cols = int(np.ceil(n / rows))
    out = torch.zeros((t, c, rows * H, cols * W), dtype=fr.dtype, device=fr.device)
    for i in range(n):
        r, q = divmod(i, cols)
        out[:, :, r * H:(r + 1) * H, q * W:(q + 1) * W] = fr[:, i]
    return out


class VecRecording:
    """What WaypointVecEnv does with record_video_trigger / video_length / video_folder: stable_baselines3's VecVideoRecorder (ref
    examples/rl_training.py:163-164) over an EpisodeRecorder.  after(step_id) runs after reset() (step_id 0) and after every step: when
    record_video_trigger(step_id) holds and nothing is being recorded, a recording of video_length frames starts with the current one;
    when it is full the file `{name_prefix}-step-{start}-to-step-{start + video_length}.mp4` is written into video_folder (tiled over
    all envs, as VecEnv.render tiles them)."""

    def __init__(self, venv, trigger, video_length, video_folder, name_prefix="rl-video", render=None):
        if not callable(trigger):
            raise ValueError("record_video_trigger must be a callable step -> bool")
        self.trigger, self.folder, self.prefix = trigger, os.path.abspath(video_folder or "videos"), name_prefix
        self.render = dict(H=256, W=256, fov=200.0, camera="ego") if render is None else dict(render)
        self.rec = EpisodeRecorder(venv, list(range(venv.num_envs)), video_length)
        self.start = None
        self.files = []

    def after(self, step_id):
        if self.start is None and self.trigger(step_id):
            self.start = step_id
            self.rec.clear()
        if self.start is not None:
            self.rec.capture()
            if len(self.rec) >= self.rec.video_length:
                self.close()

    def close(self):
        """write what has been recorded (if anything) and stop recording"""
        if self.start is not None and len(self.rec):
            os.makedirs(self.folder, exist_ok=True)
            name = f"{self.prefix}-step-{self.start}-to-step-{self.start + self.rec.video_length}.mp4"
            self.files.append(self.rec.save(os.path.join(self.folder, name), tile=True, **self.render))
        self.start = None
        self.rec.clear()
