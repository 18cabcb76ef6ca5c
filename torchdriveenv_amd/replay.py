"""A device-resident replay buffer for the off-policy algorithms the reference trains by default (SAC, TD3: ref
examples/rl_training.py:166-183) over BatchedWaypointEnv (include/tde_replay.h, csrc/tde_replay.hip).

Birdview observations are kept as ONE layer plane (a byte per pixel) per env and step - 4096 bytes per transition at 64 x 64, against
the 2 * 3 * frame_stack * 4096 of a store of stacked obs + next_obs - and both stacks are rebuilt through the palette when a batch is
sampled.  Vector and state observations are kept as float32 rows.

    buf = env.replay_buffer(capacity_steps=128)
    obs = env.reset();            buf.begin()
    obs, *_ = env.step(actions);  buf.push(actions)            # every step
    env.reset(mask=m);            buf.begin(mask=m)            # a reset of the caller's own
    batch = buf.sample(256)                                    # observations, actions, next_observations, dones, rewards
    batch = buf.sample_nstep(256, n_steps=3, gamma=0.99)       # the same with n-step rewards, and discounts, steps
    batch = buf.sample_sequence(64, length=80)                 # windows of consecutive steps for a recurrent learner (tde_sequence.h)

sample_nstep() (include/tde_nstep.h, csrc/tde_nstep.hip) looks up to n_steps stored steps ahead of the drawn one and stops where the
episode stopped: `rewards` is the discounted sum over the steps taken, `next_observations` and `dones` are those of the last of them,
and the learner's target is rewards + discounts * bootstrap * Q(next_observations).

On an env built with terminal_obs=True the buffer also keeps the terminal frames (include/tde_terminal.h, csrc/tde_terminal.hip): a
transition that ended its episode then returns the observation the env showed before it was re-spawned as `next_observations`, and
`batch.bootstrap` says where the learner should use it.

With prioritized=Prioritized(...) the buffer keeps an integer priority per stored transition on the device (include/tde_priority.h,
csrc/tde_priority.hip):

    buf = env.replay_buffer(capacity_steps=128, prioritized=Prioritized(alpha=0.6, beta=0.4))
    batch = buf.sample_prioritized(256, n_steps=3)             # NStepSamples' fields, and priorities, weights
    buf.update_priorities(batch.indices, td_errors)            # p = (|td| + eps) ** alpha
"""
from collections import namedtuple

import torch

from . import _abi, ops
from .config import check_prioritized
from .ops import _check_gamma, _check_n, _check_n_steps


def _ended(d):
    """the done byte(s) `d` of a stored step: it ended its episode or was cut - the next slot is not its next observation"""
    return (d & (3 | _abi.REPLAY_CUT)) != 0


def _bootstraps(d):
    """the done byte(s) `d` of a sample's last step: it did not end, or it was truncated and its terminal observation is there"""
    return ~_ended(d) | (((d & 3) == 2) & ((d & _abi.TERMINAL_HAS) != 0))


class ReplaySamples(namedtuple("ReplaySamples", ["observations", "actions", "next_observations", "dones", "rewards", "indices"])):
    """SB3's ReplayBufferSamples fields, all device tensors: observations / next_observations as the env returns them (uint8
    [n, 3 * frame_stack, H, W] or float32 [n, D]), actions float32 [n, 2], rewards float32 [n], dones uint8 [n] (tde_state.done_bits of
    the step | REPLAY_CUT), indices int32 [n, 2] (slot, env)."""
    __slots__ = ()

    @property
    def terminal(self):
        """bool [n]: the transition has no next observation (terminated, truncated, or cut by a reset of the caller's)"""
        return _ended(self.dones)

    @property
    def bootstrap(self):
        """bool [n]: the learner should bootstrap from next_observations - the transition did not end (not terminal), or it was
        truncated, not terminated, and its terminal observation is there (dones & TERMINAL_HAS: a terminal_obs env; SB3's
        handle_timeout_termination)"""
        return _bootstraps(self.dones)


class NStepSamples(namedtuple("NStepSamples", ReplaySamples._fields + ("discounts", "steps"))):
    """ReplaySamples over a look-ahead of m <= n_steps stored steps from the drawn one (observations, actions, indices are the drawn
    step's): rewards float32 [n] is r_0 + gamma r_1 + ... + gamma^(m-1) r_(m-1), next_observations and dones are those of the last step
    taken, discounts float32 [n] is gamma^m and steps uint8 [n] is m (0 for a pair that gathered zeros).  The n-step target is
    rewards + discounts * bootstrap * Q(next_observations)."""
    __slots__ = ()
    terminal = ReplaySamples.terminal
    bootstrap = ReplaySamples.bootstrap


class PrioritizedSamples(namedtuple("PrioritizedSamples", NStepSamples._fields + ("priorities", "weights"))):
    """NStepSamples of pairs drawn in proportion to their priorities: priorities int32 [n] is the integer priority q of each pick
    (16.16 fixed point; 0 for a row that picked nothing) and weights float32 [n] the importance weight (min_j q_j / q_i) ** beta -
    (N * P(i)) ** -beta normalised by the batch's largest; a row with q = 0 has weight 0."""
    __slots__ = ()
    terminal = ReplaySamples.terminal
    bootstrap = ReplaySamples.bootstrap


class SequenceSamples(namedtuple("SequenceSamples", ["observations", "actions", "rewards", "dones", "lengths", "indices", "priorities",
                                                    "weights"])):
    """n windows of up to T consecutive steps of one env each, all device tensors: observations uint8 [n, T + 1, 3 * frame_stack, H, W] or
    float32 [n, T + 1, D] - observations[i, k] is what the env showed at step k of window i, observations[i, lengths[i]] the next
    observation of its last step (zeros, the terminal observation, or the following step's, as ReplaySamples.next_observations) -
    actions float32 [n, T, 2], rewards float32 [n, T], dones uint8 [n, T], lengths int32 [n] (the steps the window holds: it stops at
    the first step that ended its episode or was cut, and at the newest stored step; 0 for a pair that gathered zeros), indices int32
    [n, 2] the (slot, env) of step 0.  Everything behind a window's length is zeros.  priorities int32 [n] and weights float32 [n] are
    those of PrioritizedSamples for a prioritized draw, None otherwise."""
    __slots__ = ()

    @property
    def mask(self):
        """bool [n, T]: step k of window i is one of its lengths[i] steps"""
        T = self.dones.shape[1]
        return torch.arange(T, device=self.lengths.device)[None, :] < self.lengths[:, None]

    @property
    def _last_done(self):
        return self.dones.gather(1, (self.lengths.long() - 1).clamp(min=0)[:, None])[:, 0]

    @property
    def terminal(self):
        """bool [n]: ReplaySamples.terminal of the window's last step (step lengths - 1)"""
        return _ended(self._last_done)

    @property
    def bootstrap(self):
        """bool [n]: ReplaySamples.bootstrap of the window's last step: the learner should bootstrap from observations[i, lengths[i]]"""
        return _bootstraps(self._last_done)


def priority_weights(q, beta):
    """float32 [n] importance weights of the integer priorities q [n]: (min of the nonzero q / q) ** beta, 0 where q is 0.  In float64
    (a q of 2^28 is not a float32), rounded once."""
    live = q > 0
    qd = q.to(torch.float64)
    smallest = torch.where(live, qd, torch.full_like(qd, float("inf"))).min()
    return torch.where(live, (smallest / qd.clamp(min=1.0)) ** float(beta), torch.zeros_like(qd)).to(torch.float32)


def _cached(cache, key, alloc, *args):
    """cache[key], made by alloc(*args) the first time: an output set is kept per size and reused by the next sample of that size"""
    out = cache.get(key)
    if out is None:
        out = cache[key] = alloc(*args)
    return out


class ReplayBuffer:
    """A ring of `capacity_steps` time slots, one entry per env and slot, bound to a BatchedWaypointEnv (auto_reset=True, with_info=True).

    Call order: begin() after env.reset(), push(actions) after every env.step(actions), begin(mask=m) after env.reset(mask=m).  The
    buffer reads the observation the env RETURNED (for a near_field env that is the one taken after its spawner ran), so it must be
    called after the env call it records and before the next one.

    What a sample is: `observations` is the observation the env showed at the drawn step, byte for byte; `next_observations` is the
    one it showed at the next step - or ZEROS where the transition ended its episode (dones & 3) or was cut by the caller's reset
    (dones & REPLAY_CUT): a finished env is re-spawned inside the step kernel, the terminal frame is never rendered, so such a
    transition has no next observation and the learner masks its bootstrap with `dones` / `.terminal`.  (SB3's
    handle_timeout_termination, which bootstraps from the terminal observation of a truncated episode, is therefore not offered.)

    One of the capacity_steps slots is always open (it holds the newest frame, whose step has not been taken), so the buffer holds at
    most capacity_steps - 1 transitions per env; sample() draws from those whose whole frame stack is still in the ring (it needs
    more than frame_stack - 1 stored steps).  The tensors a sample returns are reused by the next sample of the same size.

    On an env with terminal_obs=True: push() also files the frames of the envs the step finished (env.terminal_frames) in a pool of
    `terminal_per_step` rows per slot (tde_terminal_push: in env order; when more envs finish at one step than the pool has rows, the
    first terminal_per_step keep theirs and the others behave as above), and sample() (tde_terminal_sample) returns, for an ended
    transition whose frame was kept, the terminal observation as next_observations - its newest frame from the pool, its older frames
    those of `observations` moved down by one - with TERMINAL_HAS set in dones, also when the transition was cut as well.
    `.terminal` keeps its meaning; `.bootstrap` is where the learner should use next_observations.  The pool costs capacity_steps *
    terminal_per_step * (H * W or 4 * D) bytes (default terminal_per_step = max(1, num_envs // 8): an eighth of the ring) plus
    4 * capacity_steps * num_envs bytes of references.

    With prioritized=Prioritized(alpha, beta, eps): push() also gives the new transitions the largest priority seen and retires the
    priorities of the transitions the ring overwrote (tde_priority_push), sample_prioritized() draws in proportion to the priorities
    and update_priorities() takes the learner's TD errors.  sample() and sample_nstep() stay the uniform draws they are.  It costs 4
    bytes per transition and an eighth of a byte of sums."""

    def __init__(self, env, capacity_steps, seed=0, terminal_per_step=None, prioritized=None):
        C_ = int(capacity_steps)
        self.prioritized = check_prioritized(prioritized) if prioritized is not None else None
        self.terminal_obs = bool(getattr(env, "terminal_obs", False))
        if terminal_per_step is not None and not self.terminal_obs:
            raise ValueError("terminal_per_step needs an env built with terminal_obs=True")
        if terminal_per_step is not None and not 1 <= int(terminal_per_step) <= env.num_envs:
            raise ValueError(f"terminal_per_step must be in [1, num_envs = {env.num_envs}], got {terminal_per_step}")
        if not env.auto_reset:
            raise ValueError("ReplayBuffer needs an env with auto_reset=True: it records the frame of the re-spawned episode as the successor of a finished one")
        if env.state["done_bits"] is None:
            raise ValueError("ReplayBuffer needs an env with with_info=True: it reads the step's done_bits")
        self.env, self.B, self.C, self.seed = env, env.num_envs, C_, int(seed)
        self.dev = env.torch_device
        ob = env.observer
        self.n_stack, self.plane, (self.obs_shape, self.obs_dtype) = ob.n_stack, ob.plane, ob.layout
        self.planes, self.D = self.plane > 0, 0 if ob.plane else int(ob.layout[0][0])
        if C_ < self.n_stack + 1 or C_ < 2:
            raise ValueError(f"capacity_steps must be >= frame_stack + 1 = {max(2, self.n_stack + 1)} (a stack and its successor), got {C_}")
        if self.planes:
            if self.plane % 16 != 0:
                raise ValueError(f"H * W = {self.plane} must be a multiple of 16 (the planes move as 16-byte words)")
            if self.plane > _abi.REPLAY_MAX_PLANE:
                raise ValueError(f"H * W = {self.plane} exceeds {_abi.REPLAY_MAX_PLANE}")
            self.frames = torch.full((C_, self.B, self.plane), _abi.LAYER_BLANK, dtype=torch.uint8, device=self.dev)
        else:
            self.frames = torch.zeros((C_, self.B, self.D), dtype=torch.float32, device=self.dev)
        self.action = torch.zeros((C_, self.B, 2), dtype=torch.float32, device=self.dev)
        self.reward = torch.zeros((C_, self.B), dtype=torch.float32, device=self.dev)
        self.done = torch.zeros((C_, self.B), dtype=torch.uint8, device=self.dev)
        self.age = torch.zeros((C_, self.B), dtype=torch.uint8, device=self.dev)
        self.struct = ops.replay_struct(C_, self.B, self.n_stack, self.plane, self.D, self.frames, self.action, self.reward, self.done, self.age)
        self.M, self.pool, self.ref, self.tstruct = 0, None, None, None
        if self.terminal_obs:
            self.M = int(terminal_per_step) if terminal_per_step is not None else max(1, self.B // 8)
            self.pool = (torch.full((C_, self.M, self.plane), _abi.LAYER_BLANK, dtype=torch.uint8, device=self.dev) if self.planes else
                         torch.zeros((C_, self.M, self.D), dtype=torch.float32, device=self.dev))
            self.ref = torch.full((C_, self.B), -1, dtype=torch.int32, device=self.dev)
            self.tstruct = ops.terminal_struct(self.struct, self.M, self.pool, self.ref)
        self.leaf, self.sums, self.qmax, self.pstruct = None, None, None, None
        if self.prioritized is not None:
            self.leaf = torch.zeros((C_, self.B), dtype=torch.int32, device=self.dev)
            self.sums = torch.zeros(ops.priority_words(C_, self.B), dtype=torch.int64, device=self.dev)
            self.qmax = torch.full((1,), _abi.PRIORITY_ONE, dtype=torch.int32, device=self.dev)
            self.pstruct = ops.priority_struct(self.struct, self.leaf, self.sums, self.qmax)
        self.first = self.w = self.count = self.draws = 0
        self._begun = False
        self._out = {}                  # sample()'s output sets by n; _sets: the other samplers' by (kind, n[, T])
        self._sets = {}

    # ---- bookkeeping --------------------------------------------------------------------------------------------------------
    def __len__(self):
        """stored transitions: valid slots x envs"""
        return self.count * self.B

    @property
    def bytes_per_transition(self):
        """bytes the ring holds per stored transition"""
        return (self.plane if self.planes else 4 * self.D) + 8 + 4 + 1 + 1

    def begin(self, mask=None):
        """after env.reset() (mask None) or env.reset(mask=m): the open slot takes the re-spawned envs' first frame with age 0; on a
        buffer that already runs, the envs' last stored step is cut (REPLAY_CUT: its successor is not its next observation)"""
        if mask is not None:
            mask = (torch.as_tensor(mask, device=self.dev) != 0).to(torch.uint8).contiguous()
            if mask.numel() != self.B:
                raise ValueError(f"mask must have {self.B} elements")
        elif self._begun:
            mask = torch.ones(self.B, dtype=torch.uint8, device=self.dev)
        ops.replay_begin(self.struct, self.dev, self.w, *self.env.observer.newest_frame(), mask)
        if self.pstruct is not None and not self._begun:
            ops.priority_reset(self.pstruct, self.struct, self.dev)
        self._begun = True

    def push(self, actions):
        """after env.step(actions): the step's action, reward and done bits complete the open slot; the observation it returned opens
        the next one"""
        if not self._begun:
            raise ValueError("push() before begin(): call begin() after env.reset()")
        a = actions
        if not (torch.is_tensor(a) and a.dtype is torch.float32 and a.device == self.dev and a.dim() == 2 and a.shape[0] == self.B
                and a.shape[1] == 2 and a.is_contiguous()):
            a = torch.as_tensor(actions, dtype=torch.float32, device=self.dev).reshape(self.B, 2).contiguous()
        st = self.env.state
        ops.replay_push(self.struct, self.dev, self.w, a, st["reward"], st["done_bits"], *self.env.observer.newest_frame())
        if self.tstruct is not None:
            ops.terminal_push(self.struct, self.tstruct, self.dev, self.w, st["done_bits"], self.env.terminal_frames)
        self.w = (self.w + 1) % self.C
        if self.w == self.first:
            self.first = (self.first + 1) % self.C           # the ring is full: the oldest step's frame was just overwritten
        else:
            self.count += 1
        if self.pstruct is not None:
            ops.priority_push(self.pstruct, self.struct, self.dev, (self.w - 1) % self.C, self.first, self.count)

    def valid_pairs(self):
        """int32 [m, 2] device tensor of every stored (slot, env) whose whole frame stack is still in the ring (what sample(idx=) may be
        given): slot s, `off` slots behind `first`, of env e is one when min(age[s][e], n_stack - 1) <= off"""
        off = torch.arange(self.count, device=self.dev)
        slots = (self.first + off) % self.C
        ok = torch.clamp(self.age[slots].to(torch.int64), max=self.n_stack - 1) <= off[:, None]
        s, e = torch.nonzero(ok, as_tuple=True)
        return torch.stack([slots[s], e], 1).to(torch.int32).contiguous()

    def _alloc(self, n):
        """a fresh set of the output tensors of a sample of `n` transitions"""
        shape, dt = (n,) + self.obs_shape, self.obs_dtype
        return {"observations": torch.empty(shape, dtype=dt, device=self.dev),
                "next_observations": torch.empty(shape, dtype=dt, device=self.dev),
                "actions": torch.empty((n, 2), dtype=torch.float32, device=self.dev),
                "rewards": torch.empty(n, dtype=torch.float32, device=self.dev),
                "dones": torch.empty(n, dtype=torch.uint8, device=self.dev),
                "indices": torch.empty((n, 2), dtype=torch.int32, device=self.dev)}

    def _buffers(self, n):
        """the output set of sample(n), kept per size (a learner draws a handful of fixed minibatch sizes)"""
        return _cached(self._out, n, self._alloc, n)

    def _alloc_nstep(self, n):
        return {**self._alloc(n), "discounts": torch.empty(n, dtype=torch.float32, device=self.dev),
                "steps": torch.empty(n, dtype=torch.uint8, device=self.dev)}

    def _alloc_sequence(self, n, T):
        return {"observations": torch.empty((n, T + 1) + self.obs_shape, dtype=self.obs_dtype, device=self.dev),
                "actions": torch.empty((n, T, 2), dtype=torch.float32, device=self.dev),
                "rewards": torch.empty((n, T), dtype=torch.float32, device=self.dev),
                "dones": torch.empty((n, T), dtype=torch.uint8, device=self.dev),
                "lengths": torch.empty(n, dtype=torch.int32, device=self.dev),
                "indices": torch.empty((n, 2), dtype=torch.int32, device=self.dev)}

    def sample(self, n, idx=None, check=True):
        """`n` transitions -> ReplaySamples, drawn on the device from (seed, the buffer's draw counter) - or, with idx (int [n, 2]
        (slot, env) pairs; n may be None), those.  check (idx only): refuse pairs that are not valid_pairs() - one host
        synchronisation; without it such a pair gathers zeros or blank older frames."""
        n, idx = self._request(n, idx, check, "sample()")
        out = _cached(self._out, n, self._alloc, n)
        if self.tstruct is not None:
            ops.terminal_sample(self.struct, self.tstruct, self.dev, self.first, self.count, n, out, idx, self.seed, self.draws)
        else:
            ops.replay_sample(self.struct, self.dev, self.first, self.count, n, out, idx, self.seed, self.draws)
        if idx is None:
            self.draws += 1
        return ReplaySamples(out["observations"], out["actions"], out["next_observations"], out["dones"], out["rewards"], out["indices"])

    def sample_nstep(self, n, n_steps, gamma=0.99, idx=None, check=True):
        """`n` n-step transitions -> NStepSamples: sample()'s pick (the same draw from the same counter, or idx under the same `check`)
        with a look-ahead of up to `n_steps` (1 .. NSTEP_MAX) stored steps from each picked step, which stops at the first step that
        ended its episode or was cut, and at the newest stored step.  One launch (tde_nstep_sample), through the terminal pool when
        the buffer has one.  The tensors it returns are its own, reused by the next sample_nstep of the same size."""
        n_steps, gamma = _check_n_steps(n_steps), _check_gamma(gamma)
        n, idx = self._request(n, idx, check)
        out = _cached(self._sets, ("nstep", n), self._alloc_nstep, n)
        ops._nstep_sample(self.struct, self.tstruct, self.dev, self.first, self.count, n, n_steps, gamma, out, idx, self.seed, self.draws)
        if idx is None:
            self.draws += 1
        return NStepSamples(out["observations"], out["actions"], out["next_observations"], out["dones"], out["rewards"], out["indices"],
                            out["discounts"], out["steps"])

    def _need_priorities(self, what):
        if getattr(self, "pstruct", None) is None:
            raise ValueError(f"{what} needs a buffer built with prioritized=Prioritized(...)")

    def _beta(self, beta):
        """the exponent of the importance weights: the caller's, or the Prioritized's"""
        beta = float(self.prioritized.beta if beta is None else beta)
        if not 0.0 <= beta <= 1.0:
            raise ValueError(f"beta must be in [0, 1], got {beta}")
        return beta

    def _prioritized_pick(self, n, beta, key, alloc, gather, *scalars):
        """the prioritized pick of `n` checked pairs, for sample_prioritized() and sample_sequence(prioritized=True): the output set
        `key` = (kind, *what `alloc` takes) with "picked" and "priorities" beside what `alloc` makes, tde_priority_sample from (seed, the
        draw counter), the gather (ops._nstep_sample or ops.sequence_sample, `scalars` between n and the outputs) of the picked pairs, and
        the counter's advance -> (out, weights under `beta`)"""
        if self.count < 1:
            raise ValueError("the buffer holds no transition yet")
        out = _cached(self._sets, key, alloc, *key[1:])
        if "picked" not in out:
            out["picked"] = torch.empty((n, 2), dtype=torch.int32, device=self.dev)
            out["priorities"] = torch.empty(n, dtype=torch.int32, device=self.dev)
        ops.priority_sample(self.pstruct, self.struct, self.dev, self.first, self.count, n, out["picked"], out["priorities"], self.seed,
                            self.draws)
        gather(self.struct, self.tstruct, self.dev, self.first, self.count, n, *scalars, out, out["picked"])
        self.draws += 1
        return out, priority_weights(out["priorities"], beta)

    def sample_prioritized(self, n, n_steps=1, gamma=0.99, beta=None):
        """`n` transitions drawn in proportion to their priorities -> PrioritizedSamples: sample_nstep()'s batch (n_steps = 1: sample()'s)
        of the picked pairs, their integer priorities, and the importance weights under `beta` (None: the Prioritized's).  Two launches:
        the pick (tde_priority_sample: a stratified draw from (seed, the buffer's draw counter), which then advances as sample()'s does)
        and tde_nstep_sample with the picked pairs, through the terminal pool when the buffer has one.  The tensors it returns are its
        own, reused by the next sample_prioritized of the same size."""
        self._need_priorities("sample_prioritized()")
        n, n_steps, gamma, beta = _check_n(n), _check_n_steps(n_steps), _check_gamma(gamma), self._beta(beta)
        out, weights = self._prioritized_pick(n, beta, ("prioritized", n), self._alloc_nstep, ops._nstep_sample, n_steps, gamma)
        return PrioritizedSamples(out["observations"], out["actions"], out["next_observations"], out["dones"], out["rewards"],
                                  out["indices"], out["discounts"], out["steps"], out["priorities"], weights)

    def update_priorities(self, indices, td_errors):
        """the learner's TD errors of a batch: the pairs `indices` (int [n, 2]: batch.indices) take the priority (|td| + eps) ** alpha
        (tde_priority_update: the largest where a pair is named twice); pairs the ring has overwritten since are ignored"""
        self._need_priorities("update_priorities()")
        idx = torch.as_tensor(indices, device=self.dev).to(torch.int32).reshape(-1, 2).contiguous()
        td = torch.as_tensor(td_errors, device=self.dev).to(torch.float32).reshape(-1)
        if idx.shape[0] < 1:
            raise ValueError("indices must hold at least one (slot, env) pair")
        if td.shape[0] != idx.shape[0]:
            raise ValueError(f"td_errors must hold {idx.shape[0]} values, one per pair of indices, got {td.shape[0]}")
        p = ((td.abs() + float(self.prioritized.eps)) ** float(self.prioritized.alpha)).contiguous()
        ops.priority_update(self.pstruct, self.struct, self.dev, self.first, self.count, idx, p)

    def sample_sequence(self, n, length, idx=None, check=True, prioritized=False, beta=None):
        """`n` windows of up to `length` (T in 1 .. SEQUENCE_MAX) consecutive steps of one env each -> SequenceSamples, for recurrent
        learners (DRQN, R2D2, recurrent SAC / TD3).  A window starts at a step picked as sample_nstep() picks one - idx (int [n, 2]
        (slot, env) pairs; n may be None) under the same `check`, or a draw from (seed, the buffer's draw counter), which advances by one -
        and stops where sample_nstep's look-ahead stops: at the first step that ended its episode or was cut, and at the newest stored
        step.  A drawn start leaves room for `length` steps whenever the buffer holds that many, so that only an episode's end shortens
        a drawn window; with length == 1 the draw is sample()'s.  One entry point (tde_sequence_sample) rebuilds all T + 1 stacked
        observations from the layer planes, through the terminal pool when the buffer has one.

        prioritized=True (a buffer built with prioritized=Prioritized(...)): the starts are picked in proportion to their priorities
        by tde_priority_sample, the pick sample_prioritized() makes from the same counter, and `priorities` and `weights` (under
        `beta`; None: the Prioritized's) are filled as there.  Priorities stay per transition: the learner writes a window's back with
        update_priorities(batch.indices, seq_priority), and R2D2's mix of the max and the mean TD error over the window is the caller's
        one line of torch, e.g. 0.9 * td.abs().amax(1) + 0.1 * (td.abs() * batch.mask).sum(1) / batch.lengths.clamp(min=1).  A
        prioritized start is any stored step, so one near the newest step gives a short window.

        The tensors it returns are its own, kept per (n, length) and reused by the next sample_sequence of the same size."""
        T = int(length)
        if not 1 <= T <= _abi.SEQUENCE_MAX:
            raise ValueError(f"length must be in [1, {_abi.SEQUENCE_MAX}], got {T}")
        priorities = weights = None
        if prioritized:
            self._need_priorities("sample_sequence(prioritized=True)")
            if idx is not None:
                raise ValueError("sample_sequence() takes idx or prioritized=True, not both")
            beta, n = self._beta(beta), _check_n(n)
            out, weights = self._prioritized_pick(n, beta, ("sequence", n, T), self._alloc_sequence, ops.sequence_sample, T)
            priorities = out["priorities"]
        else:
            if beta is not None:
                raise ValueError("beta needs prioritized=True")
            n, idx = self._request(n, idx, check, "sample_sequence()")
            out = _cached(self._sets, ("sequence", n, T), self._alloc_sequence, n, T)
            ops.sequence_sample(self.struct, self.tstruct, self.dev, self.first, self.count, n, T, out, idx, self.seed, self.draws)
            if idx is None:
                self.draws += 1
        return SequenceSamples(out["observations"], out["actions"], out["rewards"], out["dones"], out["lengths"], out["indices"],
                               priorities, weights)

    def _request(self, n, idx, check, what="sample_nstep()"):
        """(n, idx) of a sample / sample_nstep / sample_sequence call as the launch takes them: idx as int32 [n, 2] on the device, n from
        it when None; refuses an empty request, an empty buffer, a draw before a whole frame stack is stored and, under `check` (one
        host synchronisation), pairs that are not valid_pairs()"""
        if idx is not None:
            idx = torch.as_tensor(idx, device=self.dev).to(torch.int32).reshape(-1, 2).contiguous()
            if n is None:
                n = idx.shape[0]
            if idx.shape[0] != int(n):
                raise ValueError(f"idx must hold {n} (slot, env) pairs")
        n = _check_n(n)
        if self.count < 1:
            raise ValueError("the buffer holds no transition yet")
        if idx is None and self.count <= self.n_stack - 1:
            raise ValueError(f"{what} draws steps whose whole frame stack is in the ring: it needs more than {self.n_stack - 1} stored steps, the buffer holds {self.count}")
        if idx is not None and check:
            s, e = idx[:, 0].long(), idx[:, 1].long()
            ok = (s >= 0) & (s < self.C) & (e >= 0) & (e < self.B)
            s, e = s.clamp(0, self.C - 1), e.clamp(0, self.B - 1)
            off = (s - self.first) % self.C
            ok &= (off < self.count) & (torch.clamp(self.age[s, e].long(), max=self.n_stack - 1) <= off)
            if not bool(ok.all()):
                raise ValueError("idx holds pairs that are not stored transitions with their whole frame stack in the ring (valid_pairs())")
        return n, idx

    @property
    def _tensors(self):
        return (("frames", "action", "reward", "done", "age") + (("pool", "ref") if self.tstruct is not None else ())
                + (("leaf", "qmax") if getattr(self, "pstruct", None) is not None else ()))

    def state_dict(self):
        return {**{k: getattr(self, k).clone() for k in self._tensors}, "first": self.first, "w": self.w, "count": self.count,
                "draws": self.draws, "seed": self.seed, "begun": self._begun}

    def load_state_dict(self, sd):
        if ("pool" in sd) != (self.tstruct is not None):
            raise ValueError("the state is of a buffer " + ("with" if "pool" in sd else "without") + " terminal frames, this buffer is "
                             + ("with" if self.tstruct is not None else "without") + " (terminal_obs=True of the env)")
        if ("leaf" in sd) != (self.pstruct is not None):
            raise ValueError("the state is of a buffer " + ("with" if "leaf" in sd else "without") + " priorities, this buffer is "
                             + ("with" if self.pstruct is not None else "without") + " (prioritized=Prioritized(...))")
        for k in self._tensors:
            if tuple(sd[k].shape) != tuple(getattr(self, k).shape):
                raise ValueError(f"{k} has shape {tuple(sd[k].shape)}, this buffer's is {tuple(getattr(self, k).shape)}")
        for k in self._tensors:
            getattr(self, k).copy_(sd[k])
        self.first, self.w, self.count, self.draws = int(sd["first"]), int(sd["w"]), int(sd["count"]), int(sd["draws"])
        self.seed, self._begun = int(sd.get("seed", self.seed)), bool(sd.get("begun", True))
        if self.pstruct is not None:
            # the sums are not part of the state: an update that names no stored pair changes no leaf and makes them current
            none = torch.full((1, 2), -1, dtype=torch.int32, device=self.dev)
            ops.priority_update(self.pstruct, self.struct, self.dev, self.first, self.count, none, torch.zeros(1, device=self.dev))
