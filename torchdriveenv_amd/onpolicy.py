"""A device-resident rollout buffer for the on-policy algorithms of the reference trainer (PPO, A2C: ref examples/rl_training.py with
env_configs/<name>/{ppo,a2c}_training.yml) over BatchedWaypointEnv (include/tde_onpolicy.h, csrc/tde_onpolicy.hip).

The store is a replay.ReplayBuffer, unchanged: one layer plane (a byte per pixel) per env and step - 4096 bytes at 64 x 64, against the
3 * frame_stack * 4096 of a store of stacked observations - with the stacks rebuilt through the palette when a minibatch is gathered.
Beside it the buffer keeps the critic's values and the policy's log-probabilities of every step, and computes advantages and returns
(generalised advantage estimation) in one launch.

    buf = env.rollout_buffer(n_steps=128, gamma=0.99, gae_lambda=0.95)
    obs = env.reset();                 buf.begin()
    for _ in range(128):
        actions, values, log_probs = policy(obs)
        obs, *_ = env.step(actions);   buf.push(actions, values, log_probs)
    buf.finish(critic(obs))                                  # advantages and returns
    for epoch in range(10):
        for batch in buf.get(4096):                          # observations, actions, old_values, old_log_prob, advantages, returns
            ...
    # the next push starts the next rollout

On an env built with terminal_obs=True, after a push:
    envs, term_obs = buf.terminal_observations()             # the envs the step truncated, and what they showed before the re-spawn
    if len(envs): buf.bootstrap(envs, critic(term_obs))      # reward += gamma * V(terminal observation), as SB3 does
"""
from collections import namedtuple

import torch

from . import ops
from .replay import ReplayBuffer

RolloutSamples = namedtuple("RolloutSamples", ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns", "indices"])
RolloutSamples.__doc__ = """SB3's RolloutBufferSamples fields, all device tensors: observations as the env returned them (uint8
[n, 3 * frame_stack, H, W] or float32 [n, D]), actions float32 [n, 2], old_values / old_log_prob / advantages / returns float32 [n],
indices int32 [n] (step * num_envs + env)."""


class RolloutBuffer:
    """`n_steps` steps of every env of a BatchedWaypointEnv (auto_reset=True, with_info=True), in time order.

    Call order: begin() after env.reset(), push(actions, values, log_probs) after every env.step(actions), begin(mask=m) after
    env.reset(mask=m); finish(last_values) once n_steps steps are held; then get() any number of times.  The first push after finish()
    starts the next rollout.  The buffer reads the observation the env RETURNED, so it must be called after the env call it records
    and before the next one.

    The ring behind it (`.ring`, a ReplayBuffer of n_steps + frame_stack slots) always holds the newest n_steps steps and the
    frame_stack - 1 frames before them: the first observations of a rollout stack over the last frames of the one before, as the
    env itself showed them.

    Advantages: SB3's RolloutBuffer.compute_returns_and_advantage, with "the next step starts an episode" read from the done bits of
    the step itself.  A terminated, truncated or caller-reset (REPLAY_CUT) step does not bootstrap: a finished env is re-spawned inside
    the step kernel, the terminal frame is never rendered, so there is no terminal observation whose value a truncated episode could
    bootstrap from (SB3's timeout bootstrap is therefore not offered, as in ReplayBuffer).  On an env with terminal_obs=True there is
    one: terminal_observations() returns it for the envs the last pushed step truncated, and bootstrap() adds gamma * V of it to that
    step's stored reward, as SB3's on_policy_algorithm.py does.  tde_gae is unchanged: the step still cuts the recurrence, and now
    carries its bootstrap in the reward.

    The tensors a batch of get() holds are reused by the next batch of the same size: consume a batch before taking the next."""

    def __init__(self, env, n_steps, gamma=0.99, gae_lambda=0.95, seed=None, terminal_per_step=None):
        T = int(n_steps)
        if T < 1:
            raise ValueError(f"n_steps must be >= 1, got {n_steps}")
        self.seed = int(getattr(env, "seed_value", 0) if seed is None else seed)
        self.ring = ReplayBuffer(env, capacity_steps=T + env.observer.n_stack, seed=self.seed, terminal_per_step=terminal_per_step)
        self.env, self.B, self.n_steps, self.dev = env, env.num_envs, T, torch.device(env.torch_device)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.values, self.log_probs, self.advantages, self.returns = (torch.zeros((T, self.B), dtype=torch.float32, device=self.dev)
                                                                      for _ in range(4))
        self.pos, self.finished, self.calls = 0, False, 0
        self._out = {}
        self._term_out = None                              # terminal_observations(): one output set of terminal_per_step rows

    # ---- filling ------------------------------------------------------------------------------------------------------------
    def __len__(self):
        """samples held: steps of the current rollout x envs"""
        return self.pos * self.B

    @property
    def full(self):
        """n_steps steps are held: finish() may be called, push() may not until it has been"""
        return self.pos == self.n_steps

    def begin(self, mask=None):
        """after env.reset() (mask None) or env.reset(mask=m): ReplayBuffer.begin of the ring"""
        self.ring.begin(mask)

    def _rows(self, **rows):
        """the float32 [B] device tensors of a call, checked: shapes first, then devices"""
        for name, t in rows.items():
            if not (torch.is_tensor(t) and t.dtype is torch.float32 and t.numel() == self.B):
                raise ValueError(f"{name} must be a float32 tensor of {self.B} elements (one per env)")
        for name, t in rows.items():
            if t.device != self.dev:
                raise ValueError(f"{name} is on {t.device}, expected {self.dev}")
        return [t.reshape(self.B) for t in rows.values()]

    def push(self, actions, values, log_probs):
        """after env.step(actions): the step joins the rollout; values / log_probs float32 [B]: the critic's value of, and the policy's
        log-probability of `actions` under, the observation the step was taken from"""
        if self.full and not self.finished:
            raise ValueError(f"the rollout already holds n_steps = {self.n_steps} steps: call finish() before the next push()")
        values, log_probs = self._rows(values=values, log_probs=log_probs)
        pos = 0 if self.finished else self.pos             # the first push after finish() starts the next rollout
        self.ring.push(actions)
        self.values[pos].copy_(values)
        self.log_probs[pos].copy_(log_probs)
        self.pos, self.finished = pos + 1, False

    def terminal_observations(self):
        """(envs int64 [k], observations [k, ...]): the envs whose last pushed step was truncated and not terminated (and whose frame
        the ring's pool kept: the first terminal_per_step finished envs of a step), and the stacked terminal observation of each, as
        tde_terminal_sample returns it for the pairs (last slot, env).  One host synchronisation (the nonzero that counts such envs).
        The observations are the first k rows of one set of terminal_per_step rows the buffer owns: valid until the next call."""
        r = self.ring
        if r.tstruct is None:
            raise ValueError("terminal_observations() needs an env built with terminal_obs=True")
        if self.pos < 1 or self.finished:
            raise ValueError("terminal_observations() follows a push(): the rollout holds no step")
        slot = (r.w - 1) % r.C
        envs = torch.nonzero(((r.done[slot] & 3) == 2) & (r.ref[slot] >= 0)).reshape(-1)
        k = int(envs.numel())                              # (<= terminal_per_step: a slot's refs name distinct pool rows)
        if self._term_out is None:
            # one output set for every call, whatever k is: ReplayBuffer._buffers keeps a set per size, and k changes from step to step
            self._term_out = r._alloc(r.M)
        out = {key: v[:k] for key, v in self._term_out.items()}
        if k == 0:
            return envs, out["next_observations"]
        idx = torch.stack([torch.full_like(envs, slot), envs], 1).to(torch.int32).contiguous()
        ops.terminal_sample(r.struct, r.tstruct, self.dev, r.first, r.count, k, out, idx)
        return envs, out["next_observations"]

    def bootstrap(self, envs, values):
        """reward[last pushed step, envs] += gamma * values (float32 [k]: the critic's value of terminal_observations()'s
        observations), once per step.  An env named twice is added to twice."""
        r = self.ring
        if self.pos < 1 or self.finished:
            raise ValueError("bootstrap() follows a push(): the rollout holds no step")
        envs = torch.as_tensor(envs, device=self.dev).to(torch.int64).reshape(-1)
        if not (torch.is_tensor(values) and values.dtype is torch.float32 and values.numel() == envs.numel()):
            raise ValueError(f"values must be a float32 tensor of {envs.numel()} elements (one per env of `envs`)")
        if values.device != self.dev:
            raise ValueError(f"values is on {values.device}, expected {self.dev}")
        r.reward[(r.w - 1) % r.C].index_add_(0, envs, values.reshape(-1) * self.gamma)

    def finish(self, last_values):
        """advantages and returns of the rollout (tde_gae); last_values float32 [B]: the critic's value of the observation the last
        step returned"""
        if not self.full:
            raise ValueError(f"finish() needs a full rollout: {self.pos} of n_steps = {self.n_steps} steps are held")
        last = self._rows(last_values=last_values)[0].contiguous()
        r = self.ring
        ops.gae(r.struct, self.dev, r.first, r.count, self.n_steps, self.values, last, self.gamma, self.gae_lambda, self.advantages,
                self.returns)
        self.finished = True

    # ---- reading ------------------------------------------------------------------------------------------------------------
    def _buffers(self, n):
        out = self._out.get(n)
        if out is None:
            r = self.ring
            out = self._out[n] = {"observations": torch.empty((n,) + r.obs_shape, dtype=r.obs_dtype, device=self.dev),
                                  "actions": torch.empty((n, 2), dtype=torch.float32, device=self.dev),
                                  **{k: torch.empty(n, dtype=torch.float32, device=self.dev)
                                     for k in ("old_values", "old_log_prob", "advantages", "returns")}}
        return out

    def gather(self, indices):
        """the samples `indices` (int32 [n] device tensor of step * num_envs + env) -> RolloutSamples (tde_onpolicy_gather)"""
        if not self.finished:
            raise ValueError("get() / gather() need finish(): the advantages of this rollout have not been computed")
        r = self.ring
        out = ops.onpolicy_gather(r.struct, self.dev, r.first, r.count, self.n_steps, indices, self.values, self.log_probs, self.advantages,
                                  self.returns, self._buffers(indices.numel()))
        return RolloutSamples(out["observations"], out["actions"], out["old_values"], out["old_log_prob"], out["advantages"], out["returns"],
                              indices)

    def get(self, batch_size=None):
        """a generator of RolloutSamples over all n_steps * num_envs samples: in batches of `batch_size` (the last may be short) along a
        fresh device permutation - torch.randperm from a generator seeded by (seed, the number of earlier permuted calls) - or, with
        None, one batch of everything in time order"""
        if not self.finished:
            raise ValueError("get() / gather() need finish(): the advantages of this rollout have not been computed")
        n = self.n_steps * self.B
        if batch_size is None:
            order, bs = torch.arange(n, dtype=torch.int32, device=self.dev), n
        else:
            bs = int(batch_size)
            if bs < 1:
                raise ValueError(f"batch_size must be >= 1 or None, got {batch_size}")
            gen = torch.Generator(device=self.dev)
            gen.manual_seed((self.seed * 1000003 + self.calls) % (1 << 63))
            self.calls += 1
            order = torch.randperm(n, generator=gen, device=self.dev).to(torch.int32)
        return (self.gather(order[i:i + bs]) for i in range(0, n, bs))

    # ---- checkpoint ---------------------------------------------------------------------------------------------------------
    def state_dict(self):
        return {"ring": self.ring.state_dict(), "values": self.values.clone(), "log_probs": self.log_probs.clone(),
                "advantages": self.advantages.clone(), "returns": self.returns.clone(), "pos": self.pos, "finished": self.finished,
                "calls": self.calls, "seed": self.seed}

    def load_state_dict(self, sd):
        for k in ("values", "log_probs", "advantages", "returns"):
            if tuple(sd[k].shape) != tuple(getattr(self, k).shape):
                raise ValueError(f"{k} has shape {tuple(sd[k].shape)}, this buffer's is {tuple(getattr(self, k).shape)}")
        self.ring.load_state_dict(sd["ring"])
        for k in ("values", "log_probs", "advantages", "returns"):
            getattr(self, k).copy_(sd[k])
        self.pos, self.finished, self.calls = int(sd["pos"]), bool(sd["finished"]), int(sd["calls"])
        self.seed = int(sd.get("seed", self.seed))
