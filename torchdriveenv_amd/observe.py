"""The observation of a BatchedWaypointEnv, stated once per obs_mode: which buffers hold it, which launch refreshes it and where its
newest frame lies.  make_observer(env) picks the class; the env, the replay and on-policy buffers and the snapshots ask `env.observer`
and compare no obs_mode.  Every launch goes through the env's handle (env._h)."""
import weakref

import torch

from . import ops
from .config import VectorObs, check_vector_obs, observation_layout


class Observer:
    """the interface, with what holds for float rows; a class states at least reobserve()"""
    plane, n_stack, res = 0, 1, 0      # bytes of a layer plane (0: float rows), frames per observation, side of the birdview
    state_obs = False                  # the observation is the state's own `obs` array, which the step and re-spawn kernels write
    vector_obs = rows = obs = None     # the checked config.VectorObs; the per-env float rows outside tde_state; what current() returns

    def __init__(self, env, vector_obs=None):       # (no reference cycle: the env's device buffers go when its last reference goes)
        self.env, self.layout = weakref.proxy(env), observation_layout(env.config, env.obs_mode, env.frame_stack, vector_obs)

    def after_step(self):
        """the observation the step just taken produced"""
        return self.observe()

    def observe(self, fresh=None):
        """take the observation of the state as it is (env.get_obs); fresh: uint8 [B], the envs whose frame stack restarts blank"""
        return self.reobserve(None)

    def reobserve(self, mask):
        """after a re-spawn of the envs in `mask` (uint8 [B] of 0 / 1; None: all): their part of the observation anew, the others' kept"""
        raise NotImplementedError

    def reset_reobserve(self, mask):
        """the masked re-spawn and reobserve(mask) as ONE C-ABI call (tde_env_reset_render); None where there is no such call"""

    def clear(self):
        """a full reset: VecFrameStack clears the stack"""

    def current(self):
        """the buffer the last step / reset returned (None before the first birdview observation)"""
        return self.obs

    def newest_frame(self):
        """(tensor, byte offset, byte stride) of the newest frame of every env's current observation"""
        obs = self.current()
        return obs, 0, 4 * obs.shape[1]

    def frames(self):
        """(layers, obs, n_stack, plane, phase) of the birdview buffers for tde_state_copy; None / 0 where there are none"""
        return None, None, 0, 0, 0

    def state_dict(self):
        """the `_frame_stack` entry of the env's state dict; None without a frame stack"""

    def load_state_dict(self, sd):
        raise ValueError("the state holds a frame stack, this env has no birdview observation")


class StateObserver(Observer):
    """obs_mode "state": x, y, psi, v, target offset (forward, left) in the ego frame, target-exists flag, environment_steps - the
    state's `obs` array.  tde_env_step writes it itself: no second launch per step."""
    state_obs = True

    def after_step(self):
        return self.env.state["obs"]

    current = after_step

    def reobserve(self, mask):
        self.env._h.state_obs(self.env.state["obs"])         # (every row: the launch takes no mask)
        return self.env.state["obs"]


class VectorObserver(Observer):
    """obs_mode "vector": tde_vector_obs into the float32 [B, D] rows"""

    def __init__(self, env, vector_obs=None):
        super().__init__(env, vector_obs)
        vo = self.vector_obs = check_vector_obs(vector_obs if vector_obs is not None else VectorObs())
        self.obs = self.rows = torch.zeros((env.num_envs,) + self.layout[0], dtype=self.layout[1], device=env.torch_device)
        self._args = (torch.from_numpy(vo.ray_directions()).to(env.torch_device), int(vo.k_neighbours), int(vo.n_rays),
                      float(vo.neighbour_radius), float(vo.ray_range), float(vo.ray_step))

    def reobserve(self, mask):
        self.env._h.vector_obs(self.rows, *self._args, mask, int(self.env.tde_cfg.flags))
        return self.rows


class BirdviewObserver(Observer):
    """obs_mode "birdview": the single uint8 [B, 3, res, res] frame `obs`, or with frame_stack > 1 the ops.FrameStack ring `stack` (obs is
    then its stacked observation).  The buffers come into being with the first observation."""

    def __init__(self, env, vector_obs=None):
        super().__init__(env, vector_obs)
        (c, self.res, _), _ = self.layout
        self.n_stack, self.plane = c // 3, self.res * self.res
        self.obs = self.stack = self._packed = self._pack_struct = None      # (_packed: the colour-to-plane scratch of an env without a stack)

    def _ring(self):
        e = self.env
        if self.stack is None:
            self.stack = ops.FrameStack(e.num_envs, self.n_stack, self.res, self.res, e.torch_device, flags=e._rflags, handle=e._h)
            self.obs = self.stack.obs                # (what every launch of the ring writes and returns)
        return self.stack

    def after_step(self):
        fresh, st = None, self.env.state
        if self.n_stack > 1 and self.env.auto_reset:
            # envs that finished were re-spawned inside the kernel: their frame stack restarts blank.  The render
            # kernel reads bits 0-1 of the mask, which is exactly the done part of done_bits
            fresh = st["done_bits"] if st["done_bits"] is not None else (st["terminated"] | st["truncated"])
        return self.observe(fresh)

    def observe(self, fresh=None):
        e = self.env
        if self.n_stack > 1:
            return self._ring().render(e.tde_cfg, e.dworld, e.state, e._fov, fresh=fresh)
        if self.obs is None:
            self.obs = torch.zeros((e.num_envs,) + self.layout[0], dtype=self.layout[1], device=e.torch_device)
        return self.reobserve(None)

    def reobserve(self, mask):
        e = self.env                                 # (the masked envs' newest frame re-rendered in place, their older frames blank)
        if self.obs is None:
            return self.observe()
        if self.stack is not None:
            return self.stack.rerender(e.tde_cfg, e.dworld, e.state, mask, e._fov)
        e._h.render(self.obs, self.res, self.res, e._fov, 1, None, 0, e._rflags, None, mask)     # the single frame of the masked (None: every) view
        return self.obs

    def reset_reobserve(self, mask):
        e = self.env
        if self.obs is None or e.dnf is not None:
            return None                              # (first observation: the buffers are not there; near field: reset -> spawn -> render)
        if self.stack is not None:
            return self.stack.reset_rerender(e.tde_cfg, e.dworld, e.state, mask, e._fov)
        e._h.reset_render(mask, int(e.tde_cfg.flags), self.obs, self.res, self.res, e._fov, 1, None, 0, e._rflags)
        return self.obs

    def clear(self):
        if self.stack is not None:
            self.stack.clear()

    def newest_frame(self):
        # (the pack runs on EVERY request: the observation changes between a terminal_obs step's two, the stash's and the replay push's)
        if self.obs is None:
            raise ValueError("the env has no observation yet: call env.reset() first")
        if self.stack is not None:
            return self.stack.layers, ((self.stack.phase - 1) % self.n_stack) * self.plane, self.n_stack * self.plane
        if self._packed is None:
            self._packed = torch.empty((self.env.num_envs, self.plane), dtype=torch.uint8, device=self.env.torch_device)
            self._pack_struct = ops.replay_pack_struct(self.env.num_envs, self.plane, self._packed)
        return ops.replay_pack(self._pack_struct, self.env.torch_device, self.obs, self._packed), 0, self.plane

    def frames(self):
        if self.obs is None:
            return None, None, 0, 0, 0
        if self.stack is None:
            return None, self.obs, 1, self.plane, 0
        return self.stack.layers, self.stack.obs, self.n_stack, self.plane, self.stack.phase

    def state_dict(self):
        return self.stack.state_dict() if self.stack is not None else None

    def load_state_dict(self, sd):
        self._ring().load_state_dict(sd)


def make_observer(env, vector_obs=None):
    """the observer of env.obs_mode / env.frame_stack (config.observation_layout refuses the combinations that do not exist)"""
    return {"birdview": BirdviewObserver, "state": StateObserver, "vector": VectorObserver}[env.obs_mode](env, vector_obs)
