"""numpy statement of the sequence sample (include/tde_sequence.h) over tests/replay_ref.Ring / tests/terminal_ref.TerminalRing: a window
is put together one step at a time from the restatements of the one-step samplers (nstep_ref.one_step: obs, action, reward and done of
every step, next_obs of the last) and the look-ahead of the n-step restatement (nstep_ref.look_ahead); none of them is restated.  The
draw is replay_ref's with the span that leaves room for a whole window."""
import numpy as np

from tests import nstep_ref as N
from tests.near_field_ref import philox_np
from tests.terminal_ref import TerminalRing
from torchdriveenv_amd import _abi

SEQUENCE_MAX = 256
FIELDS = ("observations", "actions", "rewards", "dones", "lengths", "indices")


def draw(ring, seed, draw, n, T):
    """int32 [n, 2]: the starts of n drawn windows of T steps"""
    skip = ring.n_stack - 1
    assert ring.count > skip and 1 <= T <= SEQUENCE_MAX
    span = max(1, ring.count - skip - (T - 1))
    wd = philox_np(seed, np.arange(n, dtype=np.uint64), int(draw) & 0xFFFFFFFF, (int(draw) >> 32) & 0xFFFFFFFF, _abi.REPLAY_TAG).astype(np.uint64)
    off = skip + ((wd[0] * np.uint64(span)) >> np.uint64(32)).astype(np.int64)
    env = ((wd[1] * np.uint64(ring.B)) >> np.uint64(32)).astype(np.int64)
    return np.stack([(ring.first + off) % ring.C, env], 1).astype(np.int32)


def gather(ring, idx, T, terminal=None):
    """tde_sequence_sample of the given pairs; terminal: with the ring's pool (default: when it has one)"""
    assert 1 <= T <= SEQUENCE_MAX
    terminal = isinstance(ring, TerminalRing) if terminal is None else terminal
    idx = np.asarray(idx, np.int64).reshape(-1, 2)
    n = len(idx)
    per = (3 * ring.n_stack, ring.plane) if ring.plane else (ring.D,)
    out = {"observations": np.zeros((n, T + 1) + per, ring.frames.dtype), "actions": np.zeros((n, T, 2), np.float32),
           "rewards": np.zeros((n, T), np.float32), "dones": np.zeros((n, T), np.uint8), "lengths": np.zeros(n, np.int32),
           "indices": idx.astype(np.int32)}
    for i, (s, e) in enumerate(idx):
        if not N.stored(ring, s, e):
            continue
        m = N.look_ahead(ring, int(s), int(e), T)
        steps = N.one_step(ring, [((s + k) % ring.C, e) for k in range(m)], terminal)
        out["observations"][i, :m] = steps["observations"]
        out["observations"][i, m] = steps["next_observations"][m - 1]
        out["actions"][i, :m], out["rewards"][i, :m], out["dones"][i, :m] = steps["actions"], steps["rewards"], steps["dones"]
        out["lengths"][i] = m
    return out
