"""Python mirror of the operator-level interface the reference env calls on its simulator
(`SimulatorInterface` methods used at ref gym_env.py:117,127,142-144) plus the fused env-level entry points, over
libtde_hip.so.  Inputs are torch tensors on a HIP device (PyTorch is only the allocator / stream owner); every call
is asynchronous on torch's current stream.  Argument errors raise ValueError (the reference does no validation, ref
gym_env.py:115-120; we check dtype/shape/device/contiguity because a bad pointer is fatal on a GPU).
"""
import ctypes as C

import numpy as np
import torch

from . import _abi, _lib


def _call(dev, fn, *args):
    """invoke a C-ABI entry point with `dev` as the current HIP device (a stream is only valid on its own device);
    the guard costs nothing in the usual single-device-per-process layout"""
    dev = torch.device(dev)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if torch.cuda.current_device() != idx:
        with torch.cuda.device(idx):
            return fn(*args)
    return fn(*args)


def _chk(t, dtype, n, name, device=None, optional=False):
    if t is None:
        if optional:
            return None
        raise ValueError(f"{name} is required")
    if not torch.is_tensor(t):
        raise ValueError(f"{name} must be a torch tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_cuda:
        raise ValueError(f"{name} must live on a HIP device (there is no CPU path)")
    if device is not None and t.device != device:
        raise ValueError(f"{name} is on {t.device}, expected {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if n is not None and t.numel() != n:
        raise ValueError(f"{name} must have {n} elements, got {t.numel()}")
    return t.data_ptr()


def kinematics_step(x, y, psi, v, lr, action, present=None, dt=0.1):
    """KinematicBicycle.step for every agent, in place (ref gym_env.py:117; model :245-247). action [...,2]."""
    L = _lib.load()
    n, dev = x.numel(), x.device
    args = [_chk(t, torch.float32, n, nm, dev) for t, nm in ((x, "x"), (y, "y"), (psi, "psi"), (v, "v"), (lr, "lr"))]
    pp = _chk(present, torch.uint8, n, "present", dev, optional=True)
    pa = _chk(action, torch.float32, 2 * n, "action", dev)
    _lib.check(_call(dev, L.tde_kinematics_step, n, *args, pp, pa, dt, _lib.current_stream(dev)), "tde_kinematics_step")


def compute_collision(B, A, x, y, psi, length, width, present, out=None):
    """compute_collision() > 0 per agent (ref gym_env.py:143) -> uint8 [B*A]"""
    L = _lib.load()
    n, dev = B * A, x.device
    ptrs = [_chk(t, torch.float32, n, nm, dev) for t, nm in ((x, "x"), (y, "y"), (psi, "psi"), (length, "length"),
                                                            (width, "width"))]
    pp = _chk(present, torch.uint8, n, "present", dev)
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=dev)
    po = _chk(out, torch.uint8, n, "out", dev)
    _lib.check(_call(dev, L.tde_compute_collision, B, A, *ptrs, pp, po, _lib.current_stream(dev)), "tde_compute_collision")
    return out


def compute_offroad(B, A, x, y, psi, length, width, present, dworld, map_of_env, threshold=0.5, out=None):
    """compute_offroad() > 0 per agent (ref gym_env.py:142) -> uint8 [B*A]"""
    L = _lib.load()
    n, dev = B * A, x.device
    ptrs = [_chk(t, torch.float32, n, nm, dev) for t, nm in ((x, "x"), (y, "y"), (psi, "psi"), (length, "length"),
                                                            (width, "width"))]
    pp = _chk(present, torch.uint8, n, "present", dev)
    pm = _chk(map_of_env, torch.int32, B, "map_of_env", dev)
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=dev)
    po = _chk(out, torch.uint8, n, "out", dev)
    _lib.check(_call(dev, L.tde_compute_offroad, B, A, *ptrs, pp, C.byref(dworld.struct), pm, threshold, po,
                                     _lib.current_stream(dev)), "tde_compute_offroad")
    return out


def kin_collide_step(B, A, x, y, psi, v, lr, length, width, present, action, dt=0.1, out=None):
    """fused kinematics + collision for all agents (BASELINE configs[1]); action [B*A,2]"""
    L = _lib.load()
    n, dev = B * A, x.device
    ptrs = [_chk(t, torch.float32, n, nm, dev) for t, nm in ((x, "x"), (y, "y"), (psi, "psi"), (v, "v"), (lr, "lr"),
                                                            (length, "length"), (width, "width"))]
    pp = _chk(present, torch.uint8, n, "present", dev)
    pa = _chk(action, torch.float32, 2 * n, "action", dev)
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=dev)
    po = _chk(out, torch.uint8, n, "out", dev)
    _lib.check(_call(dev, L.tde_kin_collide_step, B, A, *ptrs, pp, pa, dt, po, _lib.current_stream(dev)), "tde_kin_collide_step")
    return out


def waypoint_reward(cfg, pre, post, offroad, collided, tl, wp_xy, wp_n, scn, steps, target_idx, reached,
                    with_info=True):
    """Reference-owned reward/termination logic (ref gym_env.py:391-437) for n envs.
    pre/post: tuples of 4 float32 tensors [n] (x,y,psi,v).  steps/target_idx/reached int32 [n], updated in place."""
    L = _lib.load()
    n, dev = pre[0].numel(), pre[0].device
    p_pre = [_chk(t, torch.float32, n, f"pre[{i}]", dev) for i, t in enumerate(pre)]
    p_post = [_chk(t, torch.float32, n, f"post[{i}]", dev) for i, t in enumerate(post)]
    po = _chk(offroad, torch.uint8, n, "offroad", dev)
    pc = _chk(collided, torch.uint8, n, "collided", dev)
    pt = _chk(tl, torch.uint8, n, "tl", dev, optional=True)
    S, NW = wp_xy.shape[0], wp_xy.shape[1]
    pw = _chk(wp_xy, torch.float64, S * NW * 2, "wp_xy", dev)
    pn = _chk(wp_n, torch.int32, S, "wp_n", dev)
    ps = _chk(scn, torch.int32, n, "scn", dev)
    pst, pti, prc = (_chk(t, torch.int32, n, nm, dev) for t, nm in ((steps, "steps"), (target_idx, "target_idx"),
                                                                    (reached, "reached")))
    out = dict(reward=torch.empty(n, dtype=torch.float32, device=dev),
               terminated=torch.empty(n, dtype=torch.uint8, device=dev),
               truncated=torch.empty(n, dtype=torch.uint8, device=dev),
               info=torch.empty((n, 4), dtype=torch.float64, device=dev) if with_info else None,
               info_reached=torch.empty(n, dtype=torch.int32, device=dev) if with_info else None)
    _lib.check(_call(dev, L.tde_waypoint_reward, C.byref(cfg), n, *p_pre, *p_post, po, pc, pt, pw, pn, NW, ps, pst, pti, prc,
                                     out["reward"].data_ptr(), out["terminated"].data_ptr(),
                                     out["truncated"].data_ptr(),
                                     None if out["info"] is None else out["info"].data_ptr(),
                                     None if out["info_reached"] is None else out["info_reached"].data_ptr(),
                                     _lib.current_stream(dev)), "tde_waypoint_reward")
    return out


def env_reset(cfg, dworld, state, mask=None):
    L = _lib.load()
    pm = _chk(mask, torch.uint8, state.B, "mask", optional=True)
    _lib.check(_call(state.device, L.tde_env_reset, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), pm,
                               _lib.current_stream(state.device)), "tde_env_reset")


def check_scenario_ids(ids, B, n_scn):
    """the checks of reset(options={"scenario": ids}) that need no GPU: an int, a sequence of B ints or an integer tensor [B], every
    id in [-1, n_scn) (-1: draw the scenario) -> int32 [B] host tensor"""
    if isinstance(ids, bool) or (isinstance(ids, float) and int(ids) != ids):
        raise ValueError("scenario ids must be integers")
    if torch.is_tensor(ids):
        if ids.dtype.is_floating_point or ids.dtype == torch.bool:
            raise ValueError(f"scenario ids must be an integer tensor, got {ids.dtype}")
        t = ids.detach().cpu().to(torch.int64).reshape(-1)
    else:
        try:
            a = np.asarray(ids)
        except Exception as ex:
            raise ValueError(f"scenario ids must be an int, a sequence of ints or an integer tensor: {ex}") from ex
        if a.dtype.kind not in "iu":
            raise ValueError(f"scenario ids must be integers, got dtype {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a, np.int64).reshape(-1))
    if (ids.dim() if torch.is_tensor(ids) else np.ndim(ids)) == 0:
        t = t.expand(int(B)).contiguous()                           # one id: every env
    if t.numel() != int(B):
        raise ValueError(f"scenario ids must be one int or {int(B)} of them, got {t.numel()}")
    if t.numel() and (int(t.min()) < -1 or int(t.max()) >= int(n_scn)):
        raise ValueError(f"scenario ids must be in [-1, {int(n_scn)}) (-1: draw), got {int(t.min())} .. {int(t.max())}")
    return t.to(torch.int32)


def env_reset_to(cfg, dworld, state, scn=None, mask=None):
    """tde_env_reset_to: tde_env_reset with the scenario of env e given by scn[e] >= 0 (int32 [B] on the device; < 0, or scn None:
    drawn as env_reset draws it).  An id >= n_scn leaves its env unwritten (the kernel cannot raise).  Asynchronous."""
    L = _lib.load()
    dev = torch.device(state.device)
    pm = _chk(mask, torch.uint8, state.B, "mask", dev, optional=True)
    ps = _chk(scn, torch.int32, state.B, "scn", dev, optional=True)
    _lib.check(_call(dev, L.tde_env_reset_to, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), pm, ps,
                     _lib.current_stream(dev)), "tde_env_reset_to")


class EvalBuffers:
    """the device arrays of a tde_eval for B envs x R episodes: plan int32 [R, B], round int32 [B], active uint8 [B], acc / results as
    raw bytes (uint8 [B, 48] / [R, B, 48]: tde_episode_record rows, _abi.EPISODE_RECORD_DTYPE on the host)"""

    def __init__(self, plan, device):
        plan = torch.as_tensor(plan, dtype=torch.int32)
        if plan.dim() != 2 or plan.shape[0] < 1:
            raise ValueError(f"plan must be int32 [R >= 1, B], got {tuple(plan.shape)}")
        R, B = int(plan.shape[0]), int(plan.shape[1])
        self._bind(plan.to(device).contiguous(), torch.zeros(B, dtype=torch.int32, device=device),
                   torch.zeros(B, dtype=torch.uint8, device=device), torch.zeros((B, 48), dtype=torch.uint8, device=device),
                   torch.zeros((R, B, 48), dtype=torch.uint8, device=device))

    @classmethod
    def over(cls, plan, round, active, acc, results):
        """the EvalBuffers of five device arrays the caller already holds, laid out as __init__ makes them"""
        if not torch.is_tensor(plan) or plan.dim() != 2 or plan.shape[0] < 1:
            raise ValueError("plan must be int32 [R >= 1, B]")
        ev = cls.__new__(cls)
        ev._bind(plan, round, active, acc, results)
        return ev

    def _bind(self, plan, round, active, acc, results):
        self.R, self.B = R, B = int(plan.shape[0]), int(plan.shape[1])
        self.plan, self.round, self.active, self.acc, self.results = plan, round, active, acc, results
        self.struct = _abi.TdeEval(_chk(plan, torch.int32, R * B, "plan"), _chk(round, torch.int32, B, "round"),
                                   _chk(active, torch.uint8, B, "active"), _chk(acc, torch.uint8, B * 48, "acc"),
                                   _chk(results, torch.uint8, R * B * 48, "results"), R, 0)

    def records(self):
        """the results on the host: a numpy record array [R, B] of _abi.EPISODE_RECORD_DTYPE (synchronises)"""
        return self.results.cpu().numpy().view(_abi.EPISODE_RECORD_DTYPE).reshape(self.R, self.B)


def eval_advance(cfg, dworld, state, ev):
    """tde_eval_advance after an env_step made WITHOUT TDE_F_AUTORESET: fold the step into the running episode records of `ev`
    (EvalBuffers), record the episodes it finished and re-spawn their envs to the next planned scenario.  One launch, asynchronous."""
    L = _lib.load()
    dev = torch.device(state.device)
    if ev.B != state.B:
        raise ValueError(f"the evaluation buffers are for {ev.B} envs, the state has {state.B}")
    for n in ("plan", "round", "active", "acc", "results"):
        if getattr(ev, n).device != dev:
            raise ValueError(f"eval.{n} is on {getattr(ev, n).device}, expected {dev}")
    _lib.check(_call(dev, L.tde_eval_advance, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), C.byref(ev.struct),
                     _lib.current_stream(dev)), "tde_eval_advance")


def _no_near_field(dworld, what):
    if getattr(dworld, "near_field", None) is not None:
        raise NotImplementedError(f"{what} re-spawns finished envs inside one launch, where the near-field spawner cannot run: "
                                  "step the envs of a near-field world with env_step + near_field_spawn")


def near_field_spawn(cfg, dworld, state, nf, mask=None):
    """tde_near_field_spawn: fill the free slots of the envs in `mask` (uint8 [B] on the device; None: all) with near-field traffic
    from the candidate table `nf` (world.DeviceNearField), on the state the preceding reset / re-spawn left.  Asynchronous."""
    L = _lib.load()
    dev = state.device
    pm = _chk(mask, torch.uint8, state.B, "mask", torch.device(dev), optional=True)
    _lib.check(_call(dev, L.tde_near_field_spawn, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), C.byref(nf.struct),
                     pm, _lib.current_stream(dev)), "tde_near_field_spawn")


def first_gaps(cfg, dworld):
    """tde_first_gaps: fill the device world's first-step gap cache for `cfg` now (tde_env_step / tde_env_rollout do it themselves
    on first use: only needed to choose when the launch happens)"""
    L = _lib.load()
    dev = next(iter(dworld.tensors.values())).device
    _lib.check(_call(dev, L.tde_first_gaps, C.byref(cfg), C.byref(dworld.struct), _lib.current_stream(dev)), "tde_first_gaps")


def env_step(cfg, dworld, state, action=None):
    """one timestep of every env.  `action` (float32 [B,2] on the device) is read in place if given, else
    state["action"] is used."""
    L = _lib.load()
    st = state.struct
    if action is not None:
        st = _abi.TdeState.from_buffer_copy(state.struct)
        st.action = _chk(action, torch.float32, 2 * state.B, "action", torch.device(state.device))
    _lib.check(_call(state.device, L.tde_env_step, C.byref(cfg), C.byref(dworld.struct), C.byref(st),
                              _lib.current_stream(state.device)), "tde_env_step")


def check_driven(agent_action, driven, B, A, dev):
    """the two tensors of env_step_driven -> their device addresses (None, None when nobody is driven): agent_action float32 [B, A, 2],
    driven bool or uint8 [B, A], both contiguous on `dev`"""
    if driven is None:
        return _chk(agent_action, torch.float32, B * A * 2, "agent_action", torch.device(dev), optional=True), None
    if torch.is_tensor(driven) and driven.dtype == torch.bool:
        driven = driven.view(torch.uint8)               # (the same bytes: True is 1)
    pd = _chk(driven, torch.uint8, B * A, "driven", torch.device(dev))
    if tuple(driven.shape) != (B, A):
        raise ValueError(f"driven must have shape [{B}, {A}], got {list(driven.shape)}")
    if agent_action is None:
        raise ValueError("agent_action is required when driven is given")
    pa = _chk(agent_action, torch.float32, B * A * 2, "agent_action", torch.device(dev))
    if tuple(agent_action.shape) != (B, A, 2):
        raise ValueError(f"agent_action must have shape [{B}, {A}, 2], got {list(agent_action.shape)}")
    return pa, pd


def env_step_driven(cfg, dworld, state, agent_action=None, driven=None, stream=None):
    """tde_env_step_driven (include/tde_driven.h): one timestep of every env in which the present slots a >= 1 with driven[e, a] set take
    agent_action[e, a] = (acceleration, steering) as slot 0 takes state["action"]; everything else is env_step's.  agent_action float32
    [B, A, 2], driven bool / uint8 [B, A], on the state's device; driven=None: nobody is driven.  `stream`: a torch.cuda.Stream
    (default: the current one).  Through ctypes under either binding."""
    L = _lib.load()
    dev = state.device
    pa, pd = check_driven(agent_action, driven, state.B, state.A, dev)
    s = _lib.current_stream(dev) if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(_call(dev, L.tde_env_step_driven, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), pa, pd, s),
               "tde_env_step_driven")


def env_rollout(cfg, dworld, state, actions, reward=None, done=None):
    """actions float32 [K,B,2] on device -> (reward [K,B] f32, done [K,B] u8)"""
    _no_near_field(dworld, "env_rollout")
    L = _lib.load()
    K, B = actions.shape[0], actions.shape[1]
    dev = actions.device
    if B != state.B:
        raise ValueError(f"actions are for {B} envs, state has {state.B}")
    pa = _chk(actions, torch.float32, K * B * 2, "actions", dev)
    if reward is None:
        reward = torch.empty((K, B), dtype=torch.float32, device=dev)
    if done is None:
        done = torch.empty((K, B), dtype=torch.uint8, device=dev)
    ro = _abi.TdeRollout(pa, _chk(reward, torch.float32, K * B, "reward", dev), _chk(done, torch.uint8, K * B, "done", dev),
                         K, 0)
    _lib.check(_call(dev, L.tde_env_rollout, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), C.byref(ro),
                                 _lib.current_stream(dev)), "tde_env_rollout")
    return reward, done


def ego_infractions(cfg, dworld, state, out=None):
    """tde_ego_infractions: float32 [B, 4] = the ego's (offroad, collision = sum of IoUs, number of overlapping agents, 0)
    MAGNITUDES of the current state - what the reference's info dict holds (ref gym_env.py:427-428) where the step path only
    needs `> 0`.  Call it after a step made
    WITHOUT TDE_F_AUTORESET and before the finished envs are re-spawned."""
    L = _lib.load()
    dev = state.device
    if out is None:
        out = torch.empty((state.B, 4), dtype=torch.float32, device=dev)
    _lib.check(_call(dev, L.tde_ego_infractions, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct),
                     _chk(out, torch.float32, 4 * state.B, "out", torch.device(dev)), _lib.current_stream(dev)), "tde_ego_infractions")
    return out


def env_post_step(cfg, dworld, state, magnitudes=None):
    """tde_env_post_step, after a step made WITHOUT TDE_F_AUTORESET: `magnitudes` (float32 [B, 4], optional) = ego_infractions of the
    state that step left, computed only for the envs it flagged; with TDE_F_AUTORESET in cfg.flags the envs it finished are
    re-spawned (their compact observation refreshed when the state carries one).  One launch.  Returns `magnitudes`."""
    L = _lib.load()
    dev = state.device
    p = None if magnitudes is None else _chk(magnitudes, torch.float32, 4 * state.B, "magnitudes", torch.device(dev))
    _lib.check(_call(dev, L.tde_env_post_step, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), p, _lib.current_stream(dev)),
               "tde_env_post_step")
    return magnitudes


def state_obs(dworld, state, out=None):
    """compact kinematic observation of every ego -> float32 [B, 8] on device: x, y, psi, v, target waypoint offset in
    the ego frame (forward, left), target-exists flag, environment_steps"""
    L = _lib.load()
    dev = state.device
    if out is None:
        out = torch.empty((state.B, 8), dtype=torch.float32, device=dev)
    po = _chk(out, torch.float32, state.B * 8, "out", torch.device(dev))
    _lib.check(_call(dev, L.tde_state_obs, C.byref(dworld.struct), C.byref(state.struct), po, _lib.current_stream(dev)),
               "tde_state_obs")
    return out


def vector_obs(cfg, dworld, state, vo, ray_dir=None, out=None, only=None):
    """tde_vector_obs: the vector observation of every env (or of those in `only`, uint8 [B] on the device; the other rows of `out`
    are left as they are) -> float32 [B, D] on the device, D = vo.dim.  vo: config.VectorObs (or the tde_vector_obs made of one:
    `ray_dir` is then required and its address goes into the struct); ray_dir: its ray_directions() as a float32 [n_rays, 2] device
    tensor (formed from vo when None).  Asynchronous."""
    from .config import check_vector_obs

    L = _lib.load()
    dev = torch.device(state.device)
    if isinstance(vo, _abi.TdeVectorObs):
        s, n_rays, dim = vo, vo.n_rays, _abi.VO_EGO + _abi.VO_NBR * vo.k_nbr + _abi.VO_RAY * vo.n_rays
    else:
        vo = check_vector_obs(vo)
        n_rays, dim = vo.n_rays, vo.dim
        s = _abi.TdeVectorObs(None, vo.k_neighbours, vo.n_rays, vo.neighbour_radius, vo.ray_range, vo.ray_step, 0)
        if ray_dir is None:
            ray_dir = torch.from_numpy(vo.ray_directions()).to(dev)
    if out is None:
        out = torch.empty((state.B, dim), dtype=torch.float32, device=dev)
    s.ray_dir = _chk(ray_dir, torch.float32, 2 * n_rays, "ray_dir", dev)
    po = _chk(out, torch.float32, state.B * dim, "out", dev)
    pm = _chk(only, torch.uint8, state.B, "only", dev, optional=True)
    _lib.check(_call(dev, L.tde_vector_obs, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), C.byref(s), pm, po,
                     _lib.current_stream(dev)), "tde_vector_obs")
    return out


def check_agent_pairs(pairs, dev, n=None):
    """the pair list of agent_obs / agent_outcomes -> (its device address, n): int32 [n, 2] = (env, slot), contiguous on `dev`"""
    _chk(pairs, torch.int32, None if n is None else 2 * n, "pairs", torch.device(dev))
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError(f"pairs must have shape [n, 2], got {list(pairs.shape)}")
    return pairs.data_ptr(), int(pairs.shape[0])


def agent_obs(cfg, dworld, state, vo, pairs, ray_dir=None, out=None, track=None, stream=None):
    """tde_agent_obs (include/tde_agents.h): the vector observation of tde_vector_obs taken from the (env, slot) pairs of `pairs` (int32
    [n, 2] on the state's device) -> float32 [n, D], D = vo.dim; the row of a pair that is out of range or absent is zeros.  vo:
    config.VectorObs; ray_dir: its ray_directions() as a float32 [n_rays, 2] device tensor (formed from vo when None).  track: uint8
    [n, 32] on the device (one tde_agent_track per pair, for agent_outcomes), written when given.  Returns `out`.  `stream`: a
    torch.cuda.Stream (default: the current one).  Through ctypes under either binding."""
    from .config import check_vector_obs

    L = _lib.load()
    dev = torch.device(state.device)
    vo = check_vector_obs(vo)
    pp, n = check_agent_pairs(pairs, dev)
    if ray_dir is None:
        ray_dir = torch.from_numpy(vo.ray_directions()).to(dev)
    s = _abi.TdeVectorObs(_chk(ray_dir, torch.float32, 2 * vo.n_rays, "ray_dir", dev), vo.k_neighbours, vo.n_rays, vo.neighbour_radius,
                          vo.ray_range, vo.ray_step, 0)
    if out is None:
        out = torch.empty((n, vo.dim), dtype=torch.float32, device=dev)
    po = _chk(out, torch.float32, n * vo.dim, "out", dev)
    pt = _chk(track, torch.uint8, n * C.sizeof(_abi.TdeAgentTrack), "track", dev, optional=True)
    st = _lib.current_stream(dev) if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(_call(dev, L.tde_agent_obs, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), C.byref(s), pp, n, po, pt, st),
               "tde_agent_obs")
    return out


def agent_outcomes(cfg, dworld, state, pairs, track, reward=None, flags=None, stream=None):
    """tde_agent_outcomes (include/tde_agents.h): what became of the pairs since agent_obs wrote `track` (uint8 [n, 32]), on the state as
    it is now -> (reward float32 [n], flags uint8 [n] of _abi.AG_*).  Through ctypes under either binding."""
    L = _lib.load()
    dev = torch.device(state.device)
    pp, n = check_agent_pairs(pairs, dev)
    pt = _chk(track, torch.uint8, n * C.sizeof(_abi.TdeAgentTrack), "track", dev)
    if reward is None:
        reward = torch.empty(n, dtype=torch.float32, device=dev)
    if flags is None:
        flags = torch.empty(n, dtype=torch.uint8, device=dev)
    pr, pf = _chk(reward, torch.float32, n, "reward", dev), _chk(flags, torch.uint8, n, "flags", dev)
    st = _lib.current_stream(dev) if stream is None else C.c_void_p(stream.cuda_stream)
    _lib.check(_call(dev, L.tde_agent_outcomes, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), pp, n, pt, pr, pf, st),
               "tde_agent_outcomes")
    return reward, flags


def planner_struct(pl):
    """the tde_planner (host struct, lattice inline) of a config.Planner"""
    from .config import check_planner

    pl = check_planner(pl)
    a, s = pl.tables()
    t = _abi.TdePlanner()
    for i, v in enumerate(a):
        t.accel[i] = float(v)
    for i, v in enumerate(s):
        t.steer[i] = float(v)
    t.n_a, t.n_s, t.horizon = len(a), len(s), int(pl.horizon)
    t.v_target, t.margin = float(pl.v_target), float(pl.margin)
    t.w_progress, t.w_speed, t.w_steer = float(pl.w_progress), float(pl.w_speed), float(pl.w_steer)
    return t


def plan_action(cfg, dworld, state, planner, out=None, only=None, diag=None):
    """tde_plan_action: the sampling planner's ego action of every env (or of those in `only`, uint8 [B] on the device; the other
    rows of `out` / `diag` are left as they are) -> float32 [B, 2] on the device.  planner: config.Planner (or the tde_planner
    planner_struct made of one); diag: optional int32 [B, 4] device tensor receiving tde_plan_diag rows (winner, fail_step, the
    cost's float32 bits, n_safe).  Asynchronous."""
    L = _lib.load()
    dev = torch.device(state.device)
    ps = planner if isinstance(planner, _abi.TdePlanner) else planner_struct(planner)
    if out is None:
        out = torch.empty((state.B, 2), dtype=torch.float32, device=dev)
    po = _chk(out, torch.float32, state.B * 2, "out", dev)
    pm = _chk(only, torch.uint8, state.B, "only", dev, optional=True)
    pd = _chk(diag, torch.int32, state.B * 4, "diag", dev, optional=True)
    _lib.check(_call(dev, L.tde_plan_action, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), C.byref(ps), pm, po, pd,
                     _lib.current_stream(dev)), "tde_plan_action")
    return out


def check_plan_set(seq, B, H, knot_len=None, tail=0):
    """the shape / range checks of score_plans that need no GPU: seq float32 [B, N, K, 2], contiguous (no silent copy) -> (N, K,
    knot_len, tail) with knot_len=None resolved to ceil(H / K)"""
    if not torch.is_tensor(seq) or seq.dtype != torch.float32:
        raise ValueError("seq must be a float32 torch tensor")
    if seq.dim() != 4 or seq.shape[0] != B or seq.shape[3] != 2:
        raise ValueError(f"seq must be [B={B}, N, K, 2], got {tuple(seq.shape)}")
    if not seq.is_contiguous():
        raise ValueError("seq must be contiguous (score_plans makes no copy of it)")
    N, K = int(seq.shape[1]), int(seq.shape[2])
    if not 1 <= N <= _abi.PLAN_MAX_SET:
        raise ValueError(f"seq: N must be in [1, {_abi.PLAN_MAX_SET}], got {N}")
    if not 1 <= K <= _abi.PLAN_MAX_H:
        raise ValueError(f"seq: K must be in [1, {_abi.PLAN_MAX_H}], got {K}")
    if knot_len is None:
        knot_len = -(-int(H) // K)
    if int(knot_len) != knot_len or int(knot_len) < 1:
        raise ValueError("knot_len must be an integer >= 1")
    if int(tail) != tail or not 0 <= int(tail) <= _abi.PLAN_MAX_TAIL:
        raise ValueError(f"tail must be an integer in [0, {_abi.PLAN_MAX_TAIL}]")
    return N, K, int(knot_len), int(tail)


def check_forecast(forecast, B, A, need):
    """the shape checks of a forecast that need no GPU: float32 [B, T, A, 4], contiguous (no silent copy), need <= T <=
    FORECAST_MAX_T -> T"""
    if not torch.is_tensor(forecast) or forecast.dtype != torch.float32:
        raise ValueError("forecast must be a float32 torch tensor")
    if forecast.dim() != 4 or forecast.shape[0] != B or forecast.shape[2] != A or forecast.shape[3] != 4:
        raise ValueError(f"forecast must be [B={B}, T, A={A}, 4], got {tuple(forecast.shape)}")
    if not forecast.is_contiguous():
        raise ValueError("forecast must be contiguous (no copy of it is made)")
    T = int(forecast.shape[1])
    if not int(need) <= T <= _abi.FORECAST_MAX_T:
        raise ValueError(f"forecast: T must be in [{int(need)}, {_abi.FORECAST_MAX_T}] (horizon + tail steps are read), got {T}")
    return T


def _forecast_out(state, T, only, out, dev):
    """the forecast family's T (an integer in range) and `out`, float32 [B, T, A, 4]: checked, or allocated - zeroed when `only`
    leaves rows unwritten -> (T, out, out's address)"""
    if int(T) != T or not 1 <= int(T) <= _abi.FORECAST_MAX_T:
        raise ValueError(f"T must be an integer in [1, {_abi.FORECAST_MAX_T}]")
    T = int(T)
    if out is None:
        out = (torch.empty if only is None else torch.zeros)((state.B, T, state.A, 4), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (state.B, T, state.A, 4):
        raise ValueError(f"out must be [B={state.B}, T={T}, A={state.A}, 4], got {tuple(out.shape)}")
    return T, out, _chk(out, torch.float32, state.B * T * state.A * 4, "out", dev)


def forecast_agents(cfg, dworld, state, T, only=None, out=None):
    """tde_forecast_agents: (x, y, psi, v) of every slot at each of the next T steps when nobody is in its cone -> float32 [B, T, A,
    4] on the device (zeros for the ego and absent slots).  only: uint8 [B], the other envs' rows of `out` are left as they are;
    out: a float32 [B, T, A, 4] device tensor to write into.  Asynchronous."""
    L = _lib.load()
    dev = torch.device(state.device)
    T, out, po = _forecast_out(state, T, only, out, dev)
    pm = _chk(only, torch.uint8, state.B, "only", dev, optional=True)
    _lib.check(_call(dev, L.tde_forecast_agents, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), T, pm, po,
                     _lib.current_stream(dev)), "tde_forecast_agents")
    return out


def check_ego_actions(ego_actions, B, T):
    """the shape checks of forecast_scene's ego actions that need no GPU: float32 [B, T, 2], contiguous (no silent copy)"""
    if not torch.is_tensor(ego_actions) or ego_actions.dtype != torch.float32:
        raise ValueError("ego_actions must be a float32 torch tensor")
    if tuple(ego_actions.shape) != (int(B), int(T), 2):
        raise ValueError(f"ego_actions must be [B={int(B)}, T={int(T)}, 2], got {tuple(ego_actions.shape)}")
    if not ego_actions.is_contiguous():
        raise ValueError("ego_actions must be contiguous (no copy of it is made)")


def forecast_scene(cfg, dworld, state, T, ego_actions=None, only=None, out=None):
    """tde_forecast_scene: (x, y, psi, v) of every slot, the ego (row 0) included, at each of the next T steps with the controller's
    leader sweep kept -> float32 [B, T, A, 4] on the device (zeros for absent slots): what T calls of tde_env_step with these ego
    actions leave in the state while no env re-spawns.  ego_actions: float32 [B, T, 2] device tensor of (acceleration, steering),
    contiguous, taken as given; None: the ego coasts.  only: uint8 [B], the other envs' rows of `out` are left as they are; out: a
    float32 [B, T, A, 4] device tensor to write into.  Asynchronous."""
    L = _lib.load()
    dev = torch.device(state.device)
    T, out, po = _forecast_out(state, T, only, out, dev)
    if ego_actions is not None:
        check_ego_actions(ego_actions, state.B, T)
    pa = _chk(ego_actions, torch.float32, state.B * T * 2, "ego_actions", dev, optional=True)
    pm = _chk(only, torch.uint8, state.B, "only", dev, optional=True)
    _lib.check(_call(dev, L.tde_forecast_scene, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), T, pa, pm, po,
                     _lib.current_stream(dev)), "tde_forecast_scene")
    return out


def score_plans(cfg, dworld, state, planner, seq, knot_len=None, tail=0, only=None, cost=None, fail_step=None, action=None, diag=None,
                forecast=None):
    """tde_score_plans: how each of N action sequences per env fares on the state as it is -> (cost float32 [B, N], fail_step int32
    [B, N]) on the device.  seq: float32 [B, N, K, 2] device tensor of (acceleration, steering) knots, contiguous; knot k holds for
    knot_len steps (None: ceil(horizon / K)), then `tail` steps of full braking; planner: config.Planner (or its tde_planner) for
    the horizon, margin, v_target and the weights.  fail_step == horizon + tail + 1: the sequence is safe.  only: uint8 [B], the
    other rows of every output are left as they are; action float32 [B, 2] / diag int32 [B, 4]: optional, receive the winner's first
    action and its tde_plan_diag row.  forecast: float32 [B, T >= horizon + tail, A, 4] device tensor, contiguous - the other agents'
    (x, y, psi, v) per step (tde_score_plans_forecast; tde_forecast_agents' layout); None: tde_score_plans' constant velocity.
    Asynchronous."""
    return _score_plans(cfg, dworld, state, planner, seq, knot_len, tail, only, cost, fail_step, action, diag, forecast)


def score_plans_scene(cfg, dworld, state, planner, seq, knot_len=None, tail=0, only=None, cost=None, fail_step=None, action=None, diag=None):
    """tde_score_plans_scene: score_plans with every sequence judged in a scene of its own, in which the other agents run the
    controller - leader sweep included - against the ego that follows THAT sequence (no forecast is materialised) -> (cost float32
    [B, N], fail_step int32 [B, N]) on the device.  Arguments and outputs are score_plans' (there is no forecast=).  With
    planner.margin == 0 fail_step is the step at which env_step would end the episode by an infraction under those actions.
    B * N * A is bounded by PLAN_SCENE_MAX_LANES.  Asynchronous."""
    return _score_plans(cfg, dworld, state, planner, seq, knot_len, tail, only, cost, fail_step, action, diag, scene=True)


def _score_plans(cfg, dworld, state, planner, seq, knot_len, tail, only, cost, fail_step, action, diag, forecast=None, scene=False):
    """score_plans (forecast: tde_score_plans_forecast) and score_plans_scene (scene=True): one set of checks and buffers, the entry
    point chosen last"""
    L = _lib.load()
    ps = planner if isinstance(planner, _abi.TdePlanner) else planner_struct(planner)
    N, K, knot_len, tail = check_plan_set(seq, state.B, ps.horizon, knot_len, tail)
    if scene and state.B * N * state.A > _abi.PLAN_SCENE_MAX_LANES:
        raise ValueError(f"B * N * A = {state.B * N * state.A} exceeds {_abi.PLAN_SCENE_MAX_LANES} (the launch grid of tde_score_plans_scene)")
    fT = check_forecast(forecast, state.B, state.A, ps.horizon + tail) if forecast is not None else 0
    dev = torch.device(state.device)
    if cost is None:
        cost = torch.empty((state.B, N), dtype=torch.float32, device=dev)
    if fail_step is None:
        fail_step = torch.empty((state.B, N), dtype=torch.int32, device=dev)
    st = _abi.TdePlanSet(_chk(seq, torch.float32, state.B * N * K * 2, "seq", dev), N, K, knot_len, tail)
    pc = _chk(cost, torch.float32, state.B * N, "cost", dev)
    pf = _chk(fail_step, torch.int32, state.B * N, "fail_step", dev)
    pm = _chk(only, torch.uint8, state.B, "only", dev, optional=True)
    pa = _chk(action, torch.float32, state.B * 2, "action", dev, optional=True)
    pd = _chk(diag, torch.int32, state.B * 4, "diag", dev, optional=True)
    name, more = "tde_score_plans_scene" if scene else "tde_score_plans", ()
    if forecast is not None:
        name, more = "tde_score_plans_forecast", (_chk(forecast, torch.float32, state.B * fT * state.A * 4, "forecast", dev), fT)
    _lib.check(_call(dev, getattr(L, name), C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), C.byref(ps), C.byref(st), pm, pc,
                     pf, pa, pd, *more, _lib.current_stream(dev)), name)
    return cost, fail_step


def render_ego(cfg, dworld, state, H=64, W=64, fov=35.0, n_stack=1, out=None, layers=None, phase=0, flags=0,
               fresh=None, only=None):
    """render_egocentric() of every env's ego -> uint8 [B, 3*n_stack, H, W] on device (ref gym_env.py:122-124).
    Frame stack (n_stack > 1): `out` is the stack of the previous call.  With `layers` (uint8 [B, n_stack, H*W], see
    FrameStack) nothing is shifted: the ring of layer planes is expanded into all frames of `out`; without it the older
    frames are shifted in place by a launch of their own.
    flags: _abi.RENDER_LEFT_HANDED | _abi.RENDER_PLAIN_EGO; fresh / only: optional uint8 [B] device masks
    (tde_render.fresh: views whose episode just started get blank older frames; tde_render.only: render these views
    only, re-rendering their newest frame in place)."""
    L = _lib.load()
    ns = max(1, n_stack)
    dev = state.device
    if out is None:
        out = torch.zeros((state.B, 3 * ns, H, W), dtype=torch.uint8, device=dev)
    pl = _chk(layers, torch.uint8, state.B * ns * H * W, "layers", optional=True) if ns > 1 else None
    pf = _chk(fresh, torch.uint8, state.B, "fresh", optional=True)
    po = _chk(only, torch.uint8, state.B, "only", optional=True)
    rd = _abi.TdeRender(_chk(out, torch.uint8, state.B * 3 * ns * H * W, "out"), H, W, fov, n_stack, pl, int(phase),
                        int(flags), pf, po)
    _lib.check(_call(dev, L.tde_render_ego, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), C.byref(rd),
                     _lib.current_stream(dev)), "tde_render_ego")
    return out


def scene_views(dworld, state, envs, camera="map"):
    """int32 [n, 4] device tensor of tde_scene_view records (env, x, y, psi; the pose as float32 bits) of the views of envs `envs`
    (int64 / int32 device tensor [n]) - see render_scene for `camera`.  No host synchronisation."""
    dev = state.device
    n = envs.numel()
    v = torch.empty((n, 4), dtype=torch.int32, device=dev)
    v[:, 0] = envs
    pose = v[:, 1:].view(torch.float32)
    if isinstance(camera, str) and camera == "map":
        if dworld.scene_camera is None:
            raise ValueError("camera='map' needs a DeviceWorld made by World.to_device (its scene_camera table)")
        pose.copy_(dworld.scene_camera[state["scn"][envs.long()].long()])
    elif isinstance(camera, str) and camera == "ego":
        g0 = envs.long() * state.A                     # slot 0 of each env: the state's own bits
        pose[:, 0] = state["x"][g0]
        pose[:, 1] = state["y"][g0]
        pose[:, 2] = state["psi"][g0]
    elif torch.is_tensor(camera):
        if camera.dtype != torch.float32 or tuple(camera.shape) != (n, 3):
            raise ValueError(f"camera must be 'map', 'ego' or a float32 tensor [{n}, 3] of (x, y, psi)")
        pose.copy_(camera.to(dev))
    else:
        raise ValueError(f"camera must be 'map', 'ego' or a float32 tensor [{n}, 3] of (x, y, psi)")
    return v


def render_scene(cfg, dworld, state, envs=None, H=1024, W=1024, fov=500.0, camera="map", out=None, flags=0, check_envs=True):
    """BirdviewRecordingWrapper-style frames (render_mode="video", ref gym_env.py:295-297): uint8 [n, 3, H, W] on device, view i of
    env envs[i] (default: every env, in order) seen from `camera`, any H, W in [1, 4096] (tde_render_scene), on the current stream.
    camera: "map" - the centre of the bounding box of the env's map mesh, heading pi/2 (our reading of torchdrivesim, whose
    camera_xy defaults to the world centre and camera_psi to pi/2: UNPINNED, that package is not available here); "ego" - slot 0's
    pose, gathered on the device; or a float32 tensor [n, 3] of (x, y, psi).  The pixels are render_ego's specification with the
    camera pose in place of the ego's; slot 0 is painted as the ego whatever the camera.  flags: _abi.RENDER_*.
    `envs` out of [0, B) raise (check_envs=False skips that check - it reads `envs` on the host - for indices known to be valid;
    the kernel then writes such a view as zeros)."""
    dev = state.device
    if envs is None:
        envs = torch.arange(state.B, dtype=torch.int32, device=dev)
    envs = torch.as_tensor(envs, dtype=torch.int32).reshape(-1)
    if check_envs and envs.numel() and not bool(((envs >= 0) & (envs < state.B)).all()):
        raise ValueError(f"envs must be in [0, {state.B})")
    envs = envs.to(dev)
    n = envs.numel()
    if not (1 <= int(H) <= 4096 and 1 <= int(W) <= 4096):
        raise ValueError("H and W must be in [1, 4096]")
    if not (np.isfinite(fov) and fov > 0):
        raise ValueError("fov must be finite and positive")
    if out is None:
        out = torch.empty((n, 3, int(H), int(W)), dtype=torch.uint8, device=dev)
    _chk(out, torch.uint8, n * 3 * int(H) * int(W), "out")
    if n == 0:
        return out
    return render_scene_views(cfg, dworld, state, scene_views(dworld, state, envs, camera), H, W, fov, out, flags)


def render_scene_views(cfg, dworld, state, views, H, W, fov, out, flags=0):
    """tde_render_scene of prepared views (scene_views: int32 [n, 4] device tensor) into `out` (uint8 [n, 3, H, W]): the launch
    alone, for callers that keep their views across calls (WaypointSuiteEnv's video frames)"""
    n = views.shape[0]
    po = _chk(out, torch.uint8, n * 3 * int(H) * int(W), "out")
    pv = _chk(views, torch.int32, n * 4, "views")
    dev = state.device
    _lib.check(_call(dev, _lib.load().tde_render_scene, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct), pv, n,
                     int(H), int(W), float(fov), int(flags), po, _lib.current_stream(dev)), "tde_render_scene")
    return out


def fork_streams(streams, device=None):
    """order `streams` (torch.cuda.Stream) after the work already queued on the current stream (before the first
    env_step_render call / after the action tensor was produced)"""
    cur = torch.cuda.current_stream(device)
    for s in streams:
        s.wait_stream(cur)


def join_streams(streams, device=None):
    """order the current stream after the work queued on `streams` (before the outputs are consumed)"""
    cur = torch.cuda.current_stream(device)
    for s in streams:
        cur.wait_stream(s)


def env_reset_render(cfg, dworld, state, mask, out, H=64, W=64, fov=35.0, n_stack=1, layers=None, phase=0, flags=0):
    """tde_env_reset_render: masked reset + the re-spawned views' first observation in ONE call (their newest frame rendered in
    place, their older stack frames blanked); `phase` = the phase of the last full render.  Returns `out`."""
    L = _lib.load()
    dev = state.device
    ns = max(1, n_stack)
    pl = _chk(layers, torch.uint8, state.B * ns * H * W, "layers", optional=True) if ns > 1 else None
    rd = _abi.TdeRender(_chk(out, torch.uint8, state.B * 3 * ns * H * W, "out"), H, W, fov, n_stack, pl, int(phase), int(flags), None, None)
    _lib.check(_call(dev, L.tde_env_reset_render, C.byref(cfg), C.byref(dworld.struct), C.byref(state.struct),
                     _chk(mask, torch.uint8, state.B, "mask", torch.device(dev)), C.byref(rd), _lib.current_stream(dev)),
               "tde_env_reset_render")
    return out


def env_step_render(cfg, dworld, state, streams, action=None, out=None, H=64, W=64, fov=35.0, n_stack=1, layers=None, phase=0,
                    flags=0, fresh=None, render=True):
    """tde_env_step_render: one timestep + (render) the birdview of every env as len(streams) contiguous sub-batches, each on
    its own HIP stream, so that the step of one sub-batch overlaps the rasteriser of another.  Same results as env_step +
    render_ego.  `streams`: torch.cuda.Stream objects; the caller orders them against the current stream (fork_streams /
    join_streams) - open-loop drivers join once, at the end.  Returns `out` (None without render)."""
    _no_near_field(dworld, "env_step_render")
    L = _lib.load()
    dev = state.device
    st = state.struct
    if action is not None:
        st = _abi.TdeState.from_buffer_copy(state.struct)
        st.action = _chk(action, torch.float32, 2 * state.B, "action", torch.device(dev))
    rdp = None
    if render:
        ns = max(1, n_stack)
        if out is None:
            # allocated (and zero-filled) on the CURRENT stream: the side streams must see the fill before they write, and
            # the caching allocator must not hand the block out again while their kernels are pending.  Callers that pass
            # `out` / `layers` / `action` own that ordering (fork_streams before, join_streams or record_stream after).
            out = torch.zeros((state.B, 3 * ns, H, W), dtype=torch.uint8, device=dev)
            cur = torch.cuda.current_stream(torch.device(dev))
            for s_ in streams:
                s_.wait_stream(cur)
                out.record_stream(s_)
        pl = _chk(layers, torch.uint8, state.B * ns * H * W, "layers", optional=True) if ns > 1 else None
        pf = _chk(fresh, torch.uint8, state.B, "fresh", optional=True)
        rd = _abi.TdeRender(_chk(out, torch.uint8, state.B * 3 * ns * H * W, "out"), H, W, fov, n_stack, pl, int(phase),
                            int(flags), pf, None)
        rdp = C.byref(rd)
    arr = (C.c_void_p * len(streams))(*[s.cuda_stream for s in streams])
    _lib.check(_call(dev, L.tde_env_step_render, C.byref(cfg), C.byref(dworld.struct), C.byref(st), rdp, arr,
                     len(streams)), "tde_env_step_render")
    return out


class CtypesHandle:
    """The ctypes binding in the shape of the C++ extension's EnvHandle (csrc/tde_torch_ext.cpp): one object per (cfg, dworld, state)
    with EnvHandle's methods - same names, same positional arguments in the same order (tests/test_binding_parity_cpu.py) - so that a
    caller holds either and launches the same way.  Every method that takes the config's `flags` stores it into `cfg` first (the
    caller's own TdeConfig, not a copy; EnvHandle's `cfg_.flags = flags`) and then calls the function of this module that states the
    launch.  `flags` of render() and `rflags` are the RENDER flags, as in EnvHandle.  step_render has no counterpart: it takes raw
    stream handles, and env_step_render above is its ctypes form."""

    def __init__(self, cfg, dworld, state):
        self.cfg, self.dworld, self.state = cfg, dworld, state
        self._planners = {}                       # the scalars of plan_action / score_plans* -> their _abi.TdePlanner

    def _planner(self, *key):
        """the tde_planner of (horizon, v_target, margin, w_progress, w_speed, w_steer, accel, steer), made once per value (the
        plan-set judges do not read the lattice: theirs is empty, as EnvHandle's planner_of leaves it)"""
        t = self._planners.get(key)
        if t is None:
            t = self._planners[key] = _abi.TdePlanner()
            t.horizon, t.v_target, t.margin, t.w_progress, t.w_speed, t.w_steer, accel, steer = key
            t.accel[:len(accel)], t.steer[:len(steer)] = accel, steer
            t.n_a, t.n_s = len(accel), len(steer)
        return t

    def step(self, action, flags):
        self.cfg.flags = flags
        env_step(self.cfg, self.dworld, self.state, action)

    def reset(self, mask, flags):
        self.cfg.flags = flags
        env_reset(self.cfg, self.dworld, self.state, mask)

    def reset_to(self, scn, mask, flags):
        self.cfg.flags = flags
        env_reset_to(self.cfg, self.dworld, self.state, scn, mask)

    def rollout(self, actions, reward, done, flags):
        self.cfg.flags = flags
        env_rollout(self.cfg, self.dworld, self.state, actions, reward, done)

    def render(self, out, H, W, fov, n_stack, layers, phase, flags, fresh, only):
        render_ego(self.cfg, self.dworld, self.state, H, W, fov, n_stack, out, layers, phase, flags, fresh, only)

    def reset_render(self, mask, flags, out, H, W, fov, n_stack, layers, phase, rflags):
        self.cfg.flags = flags
        env_reset_render(self.cfg, self.dworld, self.state, mask, out, H, W, fov, n_stack, layers, phase, rflags)

    def state_obs(self, out):
        state_obs(self.dworld, self.state, out)

    def vector_obs(self, out, ray_dir, k_nbr, n_rays, nbr_radius, ray_range, ray_step, only, flags):
        self.cfg.flags = flags
        vector_obs(self.cfg, self.dworld, self.state, _abi.TdeVectorObs(None, k_nbr, n_rays, nbr_radius, ray_range, ray_step, 0), ray_dir,
                   out, only)

    def plan_action(self, out, accel, steer, horizon, v_target, margin, w_progress, w_speed, w_steer, only, diag, flags):
        self.cfg.flags = flags
        pl = self._planner(horizon, v_target, margin, w_progress, w_speed, w_steer, tuple(accel), tuple(steer))
        plan_action(self.cfg, self.dworld, self.state, pl, out, only, diag)

    def score_plans(self, seq, knot_len, tail, cost, fail_step, horizon, v_target, margin, w_progress, w_speed, w_steer, only, action, diag,
                    flags, forecast=None):
        self.cfg.flags = flags
        pl = self._planner(horizon, v_target, margin, w_progress, w_speed, w_steer, (), ())
        score_plans(self.cfg, self.dworld, self.state, pl, seq, knot_len, tail, only, cost, fail_step, action, diag, forecast)

    def score_plans_scene(self, seq, knot_len, tail, cost, fail_step, horizon, v_target, margin, w_progress, w_speed, w_steer, only, action,
                          diag, flags):
        self.cfg.flags = flags
        pl = self._planner(horizon, v_target, margin, w_progress, w_speed, w_steer, (), ())
        score_plans_scene(self.cfg, self.dworld, self.state, pl, seq, knot_len, tail, only, cost, fail_step, action, diag)

    def forecast_agents(self, out, only, flags):
        self.cfg.flags = flags
        forecast_agents(self.cfg, self.dworld, self.state, out.shape[1], only, out)

    def forecast_scene(self, out, ego_actions, only, flags):
        self.cfg.flags = flags
        forecast_scene(self.cfg, self.dworld, self.state, out.shape[1], ego_actions, only, out)

    def ego_infractions(self, out, flags):
        self.cfg.flags = flags
        ego_infractions(self.cfg, self.dworld, self.state, out)

    def post_step(self, magnitudes, flags):
        self.cfg.flags = flags
        env_post_step(self.cfg, self.dworld, self.state, magnitudes)

    def eval_advance(self, plan, round, active, acc, results, flags):
        self.cfg.flags = flags
        eval_advance(self.cfg, self.dworld, self.state, EvalBuffers.over(plan, round, active, acc, results))

    def near_field_spawn(self, nf, mask, flags):
        self.cfg.flags = flags
        near_field_spawn(self.cfg, self.dworld, self.state, nf, mask)


class FrameStack:
    """Device-side VecFrameStack(n_stack, channels_order="first") (ref examples/rl_training.py:160) kept as a ring of
    one-byte-per-pixel layer planes: every call writes all n_stack frames of `obs` (oldest first) from the ring, so no
    pixels are moved between calls.  `phase` (the ring slot of the next frame) stays reduced modulo n_stack."""

    def __init__(self, B, n_stack, H=64, W=64, device="cuda", flags=0, handle=None):
        self.n_stack, self.H, self.W, self.flags = int(n_stack), H, W, int(flags)
        self.handle = handle                      # optional EnvHandle / CtypesHandle of (cfg, dworld, state): the launches go through it
        self.obs = torch.zeros((B, 3 * self.n_stack, H, W), dtype=torch.uint8, device=device)
        self.layers = torch.full((B, self.n_stack, H * W), _abi.LAYER_BLANK, dtype=torch.uint8, device=device)
        self.phase = 0

    def _launcher(self, cfg, dworld, state):
        """the handle the launches go through: the one given, else the ctypes binding of these arguments"""
        return self.handle if self.handle is not None else CtypesHandle(cfg, dworld, state)

    def render(self, cfg, dworld, state, fov=35.0, fresh=None):
        """append the current frame of every view; `fresh` (uint8 [B]): views whose episode just (re)started - their
        older frames become blank, as VecFrameStack shows them after a reset"""
        self._launcher(cfg, dworld, state).render(self.obs, self.H, self.W, fov, self.n_stack, self.layers, self.phase, self.flags, fresh, None)
        self.phase = (self.phase + 1) % self.n_stack
        return self.obs

    def reset_rerender(self, cfg, dworld, state, mask, fov=35.0):
        """masked reset + rerender() of the same views as one C-ABI call (tde_env_reset_render)"""
        last = (self.phase - 1) % self.n_stack
        self._launcher(cfg, dworld, state).reset_render(mask, int(cfg.flags), self.obs, self.H, self.W, fov, self.n_stack, self.layers, last,
                                                        self.flags)
        return self.obs

    def rerender(self, cfg, dworld, state, mask, fov=35.0):
        """re-render the NEWEST frame of the masked views in place (they were re-spawned after the last `render`) and
        blank their older frames; the other views and the ring position are untouched"""
        last = (self.phase - 1) % self.n_stack
        self._launcher(cfg, dworld, state).render(self.obs, self.H, self.W, fov, self.n_stack, self.layers, last, self.flags, mask, mask)
        return self.obs

    def clear(self, mask=None):
        """blank the stack of the masked views (all views without a mask), as VecFrameStack does on reset"""
        if mask is None:
            self.layers.fill_(_abi.LAYER_BLANK)
        else:
            self.layers[mask] = _abi.LAYER_BLANK

    def state_dict(self):
        return {"layers": self.layers.clone(), "obs": self.obs.clone(), "phase": self.phase}

    def load_state_dict(self, sd):
        self.layers.copy_(sd["layers"])
        self.obs.copy_(sd["obs"])
        self.phase = int(sd["phase"]) % self.n_stack


# ---- replay buffer (include/tde_replay.h) ---------------------------------------------------------------------------------------
def _ring_frame(rp, stacked=False):
    """dtype and elements of a frame of the ring `rp` - a layer plane (planes mode) or a row (rows mode) - or, stacked, of the
    observation a gather builds from it"""
    if rp.plane > 0:
        return torch.uint8, (3 * rp.n_stack if stacked else 1) * rp.plane
    return torch.float32, rp.D


def _src_bounds(src, B, row, src_offset, src_stride):
    """`src` must hold B rows of `row` bytes, `src_stride` bytes apart, the first at byte `src_offset`"""
    if src_offset < 0 or src_stride < row or src_offset + (B - 1) * src_stride + row > src.numel() * src.element_size():
        raise ValueError(f"src holds {src.numel() * src.element_size()} bytes: too few for {B} rows of {row} bytes, {src_stride} apart, from byte {src_offset}")


def _replay_src(rp, src, src_offset, src_stride, dev):
    """address and stride of the frame source of replay_begin / replay_push: a uint8 (planes mode) or float32 (rows mode) device
    tensor holding one plane / row per env `src_stride` bytes apart, the first at byte `src_offset`"""
    dt, per = _ring_frame(rp)
    p = _chk(src, dt, None, "src", dev)
    row = per * src.element_size()
    src_stride = row if src_stride is None else int(src_stride)
    src_offset = int(src_offset)
    _src_bounds(src, rp.B, row, src_offset, src_stride)
    return p + src_offset, src_stride


def _ring_call(dev, name, *args):
    """the entry point `name` of the library with `args` and, behind them, the current stream of `dev`; a refusal raises"""
    _lib.check(_call(dev, getattr(_lib.load(), name), *args, _lib.current_stream(dev)), name)


def _u64(seed, draw):
    """a seed and a draw counter as the two uint64 the entry points take"""
    return int(seed) & (2**64 - 1), int(draw) & (2**64 - 1)


# the scalar rules of a sample, each stated once: the wrappers below and ReplayBuffer's methods call these
def _check_n(n):
    if n is None or (n := int(n)) < 1:
        raise ValueError("n must be >= 1")
    return n


def _check_n_steps(n_steps):
    if not 1 <= (n_steps := int(n_steps)) <= _abi.NSTEP_MAX:
        raise ValueError(f"n_steps must be in [1, {_abi.NSTEP_MAX}], got {n_steps}")
    return n_steps


def _check_gamma(gamma):
    if not 0.0 <= (gamma := float(gamma)) <= 1.0:
        raise ValueError(f"gamma must be in [0, 1], got {gamma}")
    return gamma


def _sample_args(rp, dev, n, out, idx_in, seed, draw, T=None):
    """what the samplers pass after (first, count): n, idx_in, seed and draw, and behind them the outputs - the six of a transition or, with
    T (sequence_sample), a window's: T + 1 observations and no next_observations, T actions, rewards and dones, and its length"""
    n = _check_n(n)
    dt, per = _ring_frame(rp, stacked=True)
    k, ko = (1, 1) if T is None else (T, T + 1)
    po = _chk(out["observations"], dt, n * ko * per, "observations", dev)
    pn = _chk(out["next_observations"], dt, n * per, "next_observations", dev) if T is None else None
    pi = _chk(out["indices"], torch.int32, 2 * n, "indices", dev)
    pa, pr = _chk(out["actions"], torch.float32, 2 * n * k, "actions", dev), _chk(out["rewards"], torch.float32, n * k, "rewards", dev)
    pd = _chk(out["dones"], torch.uint8, n * k, "dones", dev)
    pl = _chk(out["lengths"], torch.int32, n, "lengths", dev) if T is not None else None
    head = (n, _chk(idx_in, torch.int32, 2 * n, "idx", dev, optional=True), *_u64(seed, draw))
    return head, ((pi, po, pn, pa, pr, pd) if T is None else (pi, po, pa, pr, pd, pl))


def replay_struct(C_, B, n_stack, plane, D, frames, action, reward, done, age):
    """_abi.TdeReplay over the caller's ring tensors: frames uint8 [C, B, plane] (planes mode, D = 0) or float32 [C, B, D] (rows mode,
    plane = 0), action float32 [C, B, 2], reward float32 [C, B], done / age uint8 [C, B], all on one HIP device"""
    C_, B, n_stack, plane, D = int(C_), int(B), int(n_stack), int(plane), int(D)
    if (plane > 0) == (D > 0):
        raise ValueError("exactly one of plane (planes mode) and D (rows mode) must be > 0")
    dev = frames.device if torch.is_tensor(frames) else None
    n = C_ * B
    pf = _chk(frames, torch.uint8 if plane > 0 else torch.float32, n * (plane if plane > 0 else D), "frames", dev)
    return _abi.TdeReplay(C_, B, n_stack, plane, D, pf, _chk(action, torch.float32, 2 * n, "action", dev),
                          _chk(reward, torch.float32, n, "reward", dev), _chk(done, torch.uint8, n, "done", dev),
                          _chk(age, torch.uint8, n, "age", dev))


def replay_begin(rp, dev, w, src, src_offset=0, src_stride=None, mask=None):
    """tde_replay_begin on the current stream: the open slot `w` takes its frame (and age 0) for the envs of `mask` (uint8 [B]; None:
    all) from `src` (_replay_src); with a mask the slot before `w` is cut for those envs"""
    dev = torch.device(dev)
    ps, stride = _replay_src(rp, src, src_offset, src_stride, dev)
    pm = _chk(mask, torch.uint8, rp.B, "mask", dev, optional=True)
    _ring_call(dev, "tde_replay_begin", C.byref(rp), int(w), ps, stride, pm)


def replay_push(rp, dev, w, action, reward, done_bits, src, src_offset=0, src_stride=None):
    """tde_replay_push on the current stream: action float32 [B, 2], reward float32 [B] and done_bits uint8 [B] of the step just taken
    go to slot `w`, the new frame (from `src`, _replay_src) and its age to slot (w + 1) % C"""
    dev = torch.device(dev)
    ps, stride = _replay_src(rp, src, src_offset, src_stride, dev)
    pa, pr = _chk(action, torch.float32, 2 * rp.B, "action", dev), _chk(reward, torch.float32, rp.B, "reward", dev)
    pd = _chk(done_bits, torch.uint8, rp.B, "done_bits", dev)
    _ring_call(dev, "tde_replay_push", C.byref(rp), int(w), pa, pr, pd, ps, stride)


def replay_sample(rp, dev, first, count, n, out, idx_in=None, seed=0, draw=0):
    """tde_replay_sample on the current stream: `n` transitions into the tensors of `out` - "indices" int32 [n, 2], "observations" /
    "next_observations" uint8 [n, 3 * n_stack, plane] (planes mode) or float32 [n, D] (rows mode), "actions" float32 [n, 2],
    "rewards" float32 [n], "dones" uint8 [n] - drawn from (seed, draw) or, with idx_in (int32 [n, 2] (slot, env) pairs), as given"""
    dev = torch.device(dev)
    head, outs = _sample_args(rp, dev, n, out, idx_in, seed, draw)
    _ring_call(dev, "tde_replay_sample", C.byref(rp), int(first), int(count), *head, *outs)
    return out


def replay_pack_struct(B, plane, scratch):
    """an _abi.TdeReplay for replay_pack alone, for a caller that has no ring (an env that keeps terminal frames at frame_stack=1).
    tde_replay_pack reads B and plane of the struct and nothing else (csrc/tde_replay.hip: replay_pack_kernel takes those two), but it
    starts, like every replay entry point, with the check of the whole struct: C = 2, n_stack = 1 and arrays that are present and
    aligned satisfy it, so all five point at `scratch` (a uint8 device tensor of at least 16 bytes, 16-byte aligned), which nothing
    reads or writes through them.  tests/test_gpu_terminal.py holds the frames packed this way to an env without auto-reset."""
    p = _chk(scratch, torch.uint8, None, "scratch", scratch.device if torch.is_tensor(scratch) else None)
    if scratch.numel() < 16 or p % 16 != 0:
        raise ValueError("scratch must hold at least 16 bytes and be 16-byte aligned")
    return _abi.TdeReplay(2, int(B), 1, int(plane), 0, p, p, p, p, p)


def replay_pack(rp, dev, rgb, planes):
    """tde_replay_pack on the current stream: colour observations uint8 [B, 3, plane] back to layer planes uint8 [B, plane]"""
    dev = torch.device(dev)
    _ring_call(dev, "tde_replay_pack", C.byref(rp), _chk(rgb, torch.uint8, rp.B * 3 * rp.plane, "rgb", dev), 3 * rp.plane,
               _chk(planes, torch.uint8, rp.B * rp.plane, "planes", dev), rp.plane)
    return planes


# ---- on-policy view of the ring (include/tde_onpolicy.h) ------------------------------------------------------------------------------
def gae(rp, dev, first, count, T, values, last_values, gamma, lam, advantages, returns):
    """tde_gae on the current stream: generalised advantage estimation over the newest `T` stored steps of the ring `rp` - values /
    advantages / returns float32 [T, B] (the last two written), last_values float32 [B]"""
    dev = torch.device(dev)
    T = int(T)
    if T < 1:
        raise ValueError("T must be >= 1")
    n = T * rp.B
    pv, pl = _chk(values, torch.float32, n, "values", dev), _chk(last_values, torch.float32, rp.B, "last_values", dev)
    pa, pr = _chk(advantages, torch.float32, n, "advantages", dev), _chk(returns, torch.float32, n, "returns", dev)
    _ring_call(dev, "tde_gae", C.byref(rp), int(first), int(count), T, pv, pl, float(gamma), float(lam), pa, pr)
    return advantages, returns


def onpolicy_gather(rp, dev, first, count, T, idx, values, log_probs, advantages, returns, out):
    """tde_onpolicy_gather on the current stream: the samples idx (int32 [n], t * B + e over the newest `T` stored steps of the ring
    `rp`) into the tensors of `out` - "observations" uint8 [n, 3 * n_stack, plane] (planes mode) or float32 [n, D] (rows mode),
    "actions" float32 [n, 2], "old_values" / "old_log_prob" / "advantages" / "returns" float32 [n], read from the float32 [T, B]
    values / log_probs / advantages / returns; an index outside [0, T * B) gathers zeros"""
    dev = torch.device(dev)
    T = int(T)
    if T < 1:
        raise ValueError("T must be >= 1")
    pi = _chk(idx, torch.int32, None, "idx", dev)
    n = idx.numel()
    if n < 1:
        raise ValueError("idx must hold at least one index")
    src = [_chk(t, torch.float32, T * rp.B, nm, dev) for t, nm in ((values, "values"), (log_probs, "log_probs"), (advantages, "advantages"),
                                                                  (returns, "returns"))]
    dt, per = _ring_frame(rp, stacked=True)
    po, pa = _chk(out["observations"], dt, n * per, "observations", dev), _chk(out["actions"], torch.float32, 2 * n, "actions", dev)
    dst = [_chk(out[k], torch.float32, n, k, dev) for k in ("old_values", "old_log_prob", "advantages", "returns")]
    _ring_call(dev, "tde_onpolicy_gather", C.byref(rp), int(first), int(count), T, n, pi, *src, po, pa, *dst)
    return out


# ---- terminal observations beside the ring (include/tde_terminal.h) ----------------------------------------------------------------------
def terminal_struct(rp, M, pool, ref):
    """_abi.TdeTerminal over the caller's pool tensors beside the ring `rp`: pool uint8 [C, M, plane] (planes mode) or float32 [C, M, D]
    (rows mode), ref int32 [C, B], on the ring's HIP device"""
    M = int(M)
    if M < 1 or M > rp.B:
        raise ValueError(f"M must be in [1, B = {rp.B}], got {M}")
    dev = pool.device if torch.is_tensor(pool) else None
    dt, per = _ring_frame(rp)
    return _abi.TdeTerminal(M, _chk(pool, dt, rp.C * M * per, "pool", dev), _chk(ref, torch.int32, rp.C * rp.B, "ref", dev))


def terminal_stash(dev, done_bits, src, src_offset, src_stride, dst):
    """tde_terminal_stash on the current stream: dst[e] = the plane / row of env e in `src` (uint8 or float32 device tensor; rows
    `src_stride` bytes apart, the first at byte `src_offset`) for the envs with done_bits[e] & 3; dst is [B, plane] uint8 or [B, D]
    float32 and keeps the other envs' entries"""
    dev = torch.device(dev)
    B = int(dst.shape[0])
    row = dst[0].numel() * dst.element_size()
    pd = _chk(done_bits, torch.uint8, B, "done_bits", dev)
    ps = _chk(src, dst.dtype, None, "src", dev)
    pt = _chk(dst, dst.dtype, None, "dst", dev)
    src_offset, src_stride = int(src_offset), int(src_stride)
    _src_bounds(src, B, row, src_offset, src_stride)
    _ring_call(dev, "tde_terminal_stash", B, row, pd, ps + src_offset, src_stride, pt)
    return dst


def terminal_push(rp, tm, dev, w, done_bits, term_src):
    """tde_terminal_push on the current stream, beside replay_push for slot `w`: the terminal frames term_src ([B, plane] uint8 or
    [B, D] float32) of the envs with done_bits[e] & 3 go to pool[w] in env order (the first M of them), ref[w] is written whole"""
    dev = torch.device(dev)
    dt, per = _ring_frame(rp)
    pd = _chk(done_bits, torch.uint8, rp.B, "done_bits", dev)
    ps = _chk(term_src, dt, rp.B * per, "term_src", dev)
    _ring_call(dev, "tde_terminal_push", C.byref(rp), C.byref(tm), int(w), pd, ps, per * term_src.element_size())


def terminal_sample(rp, tm, dev, first, count, n, out, idx_in=None, seed=0, draw=0):
    """tde_terminal_sample on the current stream: replay_sample's arguments and outputs; where a transition ended its episode and its
    terminal frame is in the pool, "next_observations" is the terminal observation and "dones" carries _abi.TERMINAL_HAS"""
    dev = torch.device(dev)
    head, outs = _sample_args(rp, dev, n, out, idx_in, seed, draw)
    _ring_call(dev, "tde_terminal_sample", C.byref(rp), C.byref(tm), int(first), int(count), *head, *outs)
    return out


# ---- n-step returns from the ring (include/tde_nstep.h) ---------------------------------------------------------------------------------
def nstep_sample(rp, tm, dev, first, count, n, n_steps, gamma, out, idx_in=None, seed=0, draw=0):
    """tde_nstep_sample on the current stream: replay_sample's (tm None) / terminal_sample's arguments and outputs with a look-ahead of
    up to `n_steps` stored steps - "rewards" is the discounted sum over the m steps taken, "next_observations" and "dones" are those of
    the last of them - and two more tensors of `out`: "discounts" float32 [n] (gamma ** m) and "steps" uint8 [n] (m)"""
    return _nstep_sample(rp, tm, dev, first, count, n, _check_n_steps(n_steps), _check_gamma(gamma), out, idx_in, seed, draw)


def _nstep_sample(rp, tm, dev, first, count, n, n_steps, gamma, out, idx_in=None, seed=0, draw=0):
    """nstep_sample with an n_steps and a gamma that have passed their rules (ReplayBuffer checks them first, in its methods' own order)"""
    dev = torch.device(dev)
    head, outs = _sample_args(rp, dev, n, out, idx_in, seed, draw)
    pg, ps = _chk(out["discounts"], torch.float32, head[0], "discounts", dev), _chk(out["steps"], torch.uint8, head[0], "steps", dev)
    _ring_call(dev, "tde_nstep_sample", C.byref(rp), None if tm is None else C.byref(tm), int(first), int(count), *head,
               n_steps, gamma, *outs, pg, ps)
    return out


# ---- prioritized replay over the ring (include/tde_priority.h) ---------------------------------------------------------------------------
def priority_words(C_, B):
    """tde_priority_words: int64 words of `sums` a ring of C_ slots and B envs needs (host only)"""
    n = _lib.load().tde_priority_words(int(C_), int(B))
    if n < 0:
        raise ValueError(_lib.load().tde_last_error().decode())
    return int(n)


def priority_struct(rp, leaf, sums, qmax):
    """_abi.TdePriority over the caller's tensors beside the ring `rp`: leaf int32 [C, B] (q < 2^28: the bits of the header's uint32),
    sums int64 [priority_words(C, B)], qmax int32 [1], on the ring's HIP device"""
    dev = leaf.device if torch.is_tensor(leaf) else None
    return _abi.TdePriority(_chk(leaf, torch.int32, rp.C * rp.B, "leaf", dev), _chk(sums, torch.int64, priority_words(rp.C, rp.B), "sums", dev),
                            _chk(qmax, torch.int32, 1, "qmax", dev))


def priority_reset(pr, rp, dev):
    """tde_priority_reset on the current stream: every leaf and sum zero, qmax = PRIORITY_ONE"""
    dev = torch.device(dev)
    _ring_call(dev, "tde_priority_reset", C.byref(pr), C.byref(rp))


def priority_push(pr, rp, dev, w, first, count):
    """tde_priority_push on the current stream, after replay_push filled slot `w`: first and count are the host's values after it
    advanced.  The pushed pairs enter with qmax, the open slot and the stacks the ring just overwrote leave"""
    dev = torch.device(dev)
    _ring_call(dev, "tde_priority_push", C.byref(pr), C.byref(rp), int(w), int(first), int(count))


def priority_update(pr, rp, dev, first, count, idx, p):
    """tde_priority_update on the current stream: the pairs idx int32 [n, 2] (slot, env) take the priorities p float32 [n] (quantised to
    16.16 fixed point, the largest where a pair is named twice); pairs that are no longer valid_pairs() are ignored"""
    dev = torch.device(dev)
    pp = _chk(p, torch.float32, None, "p", dev)
    n = p.numel()
    if n < 1:
        raise ValueError("p must hold at least one priority")
    pi = _chk(idx, torch.int32, 2 * n, "idx", dev)
    _ring_call(dev, "tde_priority_update", C.byref(pr), C.byref(rp), int(first), int(count), n, pi, pp)


def priority_sample(pr, rp, dev, first, count, n, idx, q, seed=0, draw=0):
    """tde_priority_sample on the current stream: `n` pairs drawn in proportion to their priorities from (seed, draw) into idx int32
    [n, 2] (slot, env) and their priorities into q int32 [n]; (-1, -1) and 0 when nothing is drawable"""
    dev = torch.device(dev)
    n = _check_n(n)
    pi, pq = _chk(idx, torch.int32, 2 * n, "idx", dev), _chk(q, torch.int32, n, "q", dev)
    _ring_call(dev, "tde_priority_sample", C.byref(pr), C.byref(rp), int(first), int(count), n, *_u64(seed, draw), pi, pq)
    return idx, q


# ---- windows of consecutive steps from the ring (include/tde_sequence.h) -----------------------------------------------------------------
def sequence_sample(rp, tm, dev, first, count, n, T, out, idx_in=None, seed=0, draw=0):
    """tde_sequence_sample on the current stream, through the terminal pool when tm is not None: `n` windows of up to `T` stored steps
    into the tensors of `out` - "observations" uint8 [n, T + 1, 3 * n_stack, plane] (planes mode) or float32 [n, T + 1, D] (rows mode),
    "actions" float32 [n, T, 2], "rewards" float32 [n, T], "dones" uint8 [n, T], "lengths" int32 [n], "indices" int32 [n, 2] - whose
    starts are drawn from (seed, draw) or, with idx_in (int32 [n, 2] (slot, env) pairs), as given"""
    dev = torch.device(dev)
    T = int(T)
    if not 1 <= T <= _abi.SEQUENCE_MAX:
        raise ValueError(f"T must be in [1, {_abi.SEQUENCE_MAX}], got {T}")
    head, outs = _sample_args(rp, dev, n, out, idx_in, seed, draw, T)
    _ring_call(dev, "tde_sequence_sample", C.byref(rp), None if tm is None else C.byref(tm), int(first), int(count), *head, T, *outs)
    return out


# ---- copies of env rows between states (include/tde_snapshot.h) ---------------------------------------------------------------------------
def snapshot_frames(src_layers, dst_layers, src_obs, dst_obs, n_stack, plane, src_phase=0, dst_phase=0):
    """the `frames` argument of state_copy: the frame-stack ring of the same rows - layers uint8 [B, n_stack, plane] and the stacked
    observation uint8 [B, 3 * n_stack, plane] of the source and of the destination (each pair optional: None, None), and the ring slot the
    next frame goes to on either side (FrameStack.phase)"""
    return dict(src_layers=src_layers, dst_layers=dst_layers, src_obs=src_obs, dst_obs=dst_obs, n_stack=int(n_stack), plane=int(plane),
                src_phase=int(src_phase), dst_phase=int(dst_phase))


def _row_indices(envs, name, dev):
    """int32 device tensor [n] of env indices from a sequence or tensor"""
    t = torch.as_tensor(envs)
    if t.dtype in (torch.float16, torch.float32, torch.float64, torch.bool, torch.bfloat16):
        raise ValueError(f"{name} must hold integers")
    return t.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()


def state_copy(src_state, dst_state, src_env, dst_env, frames=None, outputs=False, check=True, handles=None):
    """tde_state_copy on the current stream: env row src_env[k] of `src_state` into env row dst_env[k] of `dst_state` (device EnvStates
    of the same A; the same state for a fork, with dst_env disjoint from src_env) - every per-agent and per-env array both states carry,
    with outputs=True the step's outputs too; the destination rows of dst_state's caches are invalidated in the same launch and no cache
    is ever copied (include/tde_snapshot.h lists the groups).  frames: snapshot_frames(...) - the rows' frame-stack ring moves with them.
    check=True (default) reads the indices back first (one synchronisation) and raises on indices out of range, rows named twice in
    dst_env, or dst_env overlapping src_env within one state; check=False skips that: a pair out of range is then skipped by the kernel.
    handles: (src, dst) launch handles of the two states - the extension's EnvHandles (the call then goes through the extension) or
    ops.CtypesHandles / None (through ctypes): both reach the same entry point."""
    if src_state.device is None or dst_state.device is None:
        raise ValueError("state_copy needs device states (there is no CPU path)")
    dev = torch.device(dst_state.device)
    if torch.device(src_state.device) != dev:
        raise ValueError(f"src_state is on {src_state.device}, dst_state on {dst_state.device}")
    if src_state.A != dst_state.A:
        raise ValueError(f"src_state has A = {src_state.A}, dst_state A = {dst_state.A}: they must be equal")
    if src_state["slot_route"] is not None and dst_state["slot_route"] is None:
        raise ValueError("src_state carries slot_route and dst_state does not: the routes of near-field agents would be lost")
    se, de = _row_indices(src_env, "src_env", dev), _row_indices(dst_env, "dst_env", dev)
    if se.numel() != de.numel():
        raise ValueError(f"src_env holds {se.numel()} indices, dst_env {de.numel()}")
    n = se.numel()
    flags = (_abi.SNAPSHOT_OUTPUTS if outputs else 0) | (_abi.SNAPSHOT_CHECK if check else 0)
    f = None
    if frames is not None:
        f = dict(frames)
        ns, plane = f["n_stack"], f["plane"]
        if not 1 <= ns <= _abi.SNAPSHOT_MAX_STACK:
            raise ValueError(f"frames: n_stack must be in [1, {_abi.SNAPSHOT_MAX_STACK}], got {ns}")
        if plane < 1 or plane % 16:
            raise ValueError(f"frames: plane must be a positive multiple of 16, got {plane}")
        for k in ("src_phase", "dst_phase"):
            if not 0 <= f[k] < ns:
                raise ValueError(f"frames: {k} must be in [0, {ns}), got {f[k]}")
        for a, b in (("src_layers", "dst_layers"), ("src_obs", "dst_obs")):
            if (f[a] is None) != (f[b] is None):
                raise ValueError(f"frames: {a} and {b} are given together or not at all")
        sizes = {"src_layers": src_state.B * ns * plane, "dst_layers": dst_state.B * ns * plane,
                 "src_obs": src_state.B * 3 * ns * plane, "dst_obs": dst_state.B * 3 * ns * plane}
        ptrs = {k: _chk(f[k], torch.uint8, sizes[k], k, dev, optional=True) for k in sizes}
    ext = handles is not None and not isinstance(handles[1], CtypesHandle)
    if ext:
        from . import _ext

        g = f or dict(src_layers=None, dst_layers=None, src_obs=None, dst_obs=None, n_stack=0, plane=0, src_phase=0, dst_phase=0)
        _ext.load().state_copy(handles[0], handles[1], se, de, g["src_layers"], g["dst_layers"], g["src_obs"], g["dst_obs"], g["n_stack"],
                               g["plane"], g["src_phase"], g["dst_phase"], flags)
        return dst_state
    fr = None
    if f is not None:
        fr = C.byref(_abi.TdeSnapshotFrames(ptrs["src_layers"], ptrs["dst_layers"], ptrs["src_obs"], ptrs["dst_obs"], ns, plane,
                                            f["src_phase"], f["dst_phase"]))
    _ring_call(dev, "tde_state_copy", C.byref(src_state.struct), C.byref(dst_state.struct), n, se.data_ptr() if n else None,
               de.data_ptr() if n else None, fr, flags)
    return dst_state
