"""Python-integer statement of prioritized replay (include/tde_priority.h) over a tests/replay_ref.Ring: the quantisation, the push and
update rules, the stratified draw (Python ints for the 64 x 64 bit products, the Philox of tests/replay_ref.py) and the pick - by
np.cumsum and np.searchsorted over the flat leaves.  It knows no tree: an inner node of the library's that is stale shows up as a
wrong pick."""
import numpy as np

from tests.replay_ref import philox_np
from torchdriveenv_amd import _abi

ONE, QMAX, TAG = _abi.PRIORITY_ONE, _abi.PRIORITY_QMAX, _abi.PRIORITY_TAG
M64 = (1 << 64) - 1


def quantise(p):
    """float32 priorities -> uint32 q: clamp(rint(p * 65536), 1, QMAX), ties to even; NaN and p <= 0 give 1, +inf gives QMAX"""
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(np.asarray(p, np.float32) * np.float32(65536.0)).astype(np.float64)
    q = np.ones(r.shape, np.uint32)
    ok = r >= 1.0                                           # (False for NaN)
    q[ok] = np.minimum(r[ok], float(QMAX)).astype(np.uint32)
    return q


def valid_mask(ring):
    """bool [C, B]: the pairs of the invariant - off = (s - first) mod C < count and min(age, n_stack - 1) <= off"""
    off = ((np.arange(ring.C) - ring.first) % ring.C)[:, None]
    return (off < ring.count) & (np.minimum(ring.age.astype(np.int64), ring.n_stack - 1) <= off)


def strata(T, n, seed, draw):
    """the n positions u_i in [0, T) as Python ints"""
    wd = philox_np(seed, np.arange(n, dtype=np.uint64), int(draw) & 0xFFFFFFFF, (int(draw) >> 32) & 0xFFFFFFFF, TAG)
    base, rem = divmod(T, n)
    out = []
    for i in range(n):
        r = (int(wd[0, i]) << 32) | int(wd[1, i])
        if base == 0:
            out.append((r * T) >> 64)
        else:
            out.append(i * base + min(i, rem) + ((r * (base + (1 if i < rem else 0))) >> 64))
    return out


def pick(leaves, us):
    """the flat leaf l with cum(l - 1) <= u < cum(l) for every u"""
    cum = np.cumsum(np.asarray(leaves, np.uint32).reshape(-1).astype(np.int64))
    return np.searchsorted(cum, np.asarray(us, np.int64), side="right")


def weights(q, beta):
    """float64 importance weights (min of the nonzero q / q) ** beta, 0 where q is 0"""
    q = np.asarray(q).astype(np.float64)
    live = q > 0
    out = np.zeros(q.shape, np.float64)
    if live.any():
        out[live] = (q[live].min() / q[live]) ** float(beta)
    return out


class Priorities:
    """leaf uint32 [C, B] and qmax beside a Ring; every method is called after the ring's own (push after Ring.push)"""

    def __init__(self, ring):
        self.ring = ring
        self.leaf = np.zeros((ring.C, ring.B), np.uint32)
        self.qmax = ONE

    @property
    def total(self):
        return int(self.leaf.astype(np.int64).sum())

    def reset(self):
        self.leaf[:] = 0
        self.qmax = ONE

    def push(self):
        g = self.ring
        w = (g.w - 1) % g.C                                 # the slot the ring's push just filled
        self.leaf[w] = self.qmax
        self.leaf[g.w] = 0
        for d in range(min(g.n_stack - 1, g.count)):
            s = (g.first + d) % g.C
            self.leaf[s, np.minimum(g.age[s].astype(np.int64), g.n_stack - 1) > d] = 0

    def update(self, idx, p):
        g = self.ring
        idx, q = np.asarray(idx, np.int64).reshape(-1, 2), quantise(p)
        ok = valid_mask(g)
        named = [(int(s), int(e), int(qi)) for (s, e), qi in zip(idx, q) if 0 <= s < g.C and 0 <= e < g.B and ok[s, e]]
        for s, e, _ in named:
            self.leaf[s, e] = 0
        for s, e, qi in named:
            self.leaf[s, e] = max(int(self.leaf[s, e]), qi)
            self.qmax = max(self.qmax, qi)
        return len(named)

    def draw(self, seed, draw, n):
        """(idx int32 [n, 2], q uint32 [n], the positions u)"""
        T, B = self.total, self.ring.B
        if T == 0:
            return np.full((n, 2), -1, np.int32), np.zeros(n, np.uint32), []
        us = strata(T, n, seed, draw)
        l = pick(self.leaf, us)
        return np.stack([l // B, l % B], 1).astype(np.int32), self.leaf.reshape(-1)[l].copy(), us
