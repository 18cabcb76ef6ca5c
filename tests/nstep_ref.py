"""numpy float32 statement of the n-step sample (include/tde_nstep.h) over tests/replay_ref.Ring / tests/terminal_ref.TerminalRing: the
look-ahead that stops where the ring says the episode stopped, the reward sum with every rounding written out, and the two stacks - obs
of the picked step, next_obs and done of the last step taken - from the restatements of the one-step samplers, which are not restated."""
import numpy as np

from tests.replay_ref import ENDED, Ring
from tests.terminal_ref import TerminalRing

F = np.float32
NSTEP_MAX = 64


def one_step(ring, idx, terminal):
    """the one-step sample of `idx`: tde_terminal_sample's (terminal) or tde_replay_sample's, whatever the ring holds beside it"""
    return ring.gather(idx) if terminal else Ring.gather(ring, idx)


def stored(ring, s, e):
    """the validity rule of a given pair"""
    return 0 <= s < ring.C and 0 <= e < ring.B and int(ring.offset(s)) < ring.count


def look_ahead(ring, s, e, n_steps):
    """m of the stored pair (s, e): the steps taken"""
    a = min(n_steps, ring.count - int(ring.offset(s)))
    for k in range(1, a + 1):
        if ring.done[(s + k - 1) % ring.C, e] & ENDED:
            return k
    return a


def reward_sum(rewards, gamma):
    """(R, g) over the float32 rewards of the steps taken, in the header's order: the product rounded to float32, then the sum"""
    gamma = F(gamma)
    R, g = F(rewards[0]), gamma
    for r in rewards[1:]:
        prod = F(g * F(r))
        R = F(R + prod)
        g = F(g * gamma)
    return R, g


def gather(ring, idx, n_steps, gamma, terminal=None):
    """tde_nstep_sample of the given pairs; terminal: with the ring's pool (default: when it has one)"""
    assert 1 <= n_steps <= NSTEP_MAX and 0.0 <= gamma <= 1.0
    terminal = isinstance(ring, TerminalRing) if terminal is None else terminal
    idx = np.asarray(idx, np.int64).reshape(-1, 2)
    out = one_step(ring, idx, terminal)                    # observations, actions and indices are the picked step's
    n = len(idx)
    out["discounts"], out["steps"] = np.zeros(n, F), np.zeros(n, np.uint8)
    for i, (s, e) in enumerate(idx):
        if not stored(ring, s, e):
            continue
        m = look_ahead(ring, int(s), int(e), n_steps)
        last = one_step(ring, [((s + m - 1) % ring.C, e)], terminal)
        out["rewards"][i], out["discounts"][i] = reward_sum([ring.reward[(s + k) % ring.C, e] for k in range(m)], gamma)
        out["steps"][i] = m
        out["next_observations"][i], out["dones"][i] = last["next_observations"][0], last["dones"][0]
    return out
