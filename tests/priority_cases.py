"""The cases of prioritized replay that tests/test_gpu_priority.py runs through the C-ABI (include/tde_priority.h) and that
tests/test_priority_cpu.py holds to the conditions that make each of them mean something.  HandPriorities puts the priorities beside a
tests/ring_util.HandRing: the device tensors of a tde_priority - each between canaries - and the Python statement
(tests/priority_ref.Priorities), fed the same calls; without a device (dev=None) only the statement is driven."""
import numpy as np
import torch

from tests import priority_ref as P
from tests import ring_util as U

FILL = {**U.FILL, torch.int64: -0x5A5A5A5A5A5A5A}
ONE, QMAX = P.ONE, P.QMAX


def guarded(shape, dtype, dev, init=None):
    """tests/ring_util.guarded with a canary for int64 as well"""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    g = -(-max(U.GUARD, int(np.prod(shape[1:]))) // 16) * 16
    whole = torch.full((n + 2 * g,), FILL[dtype], dtype=dtype, device=dev)
    middle = whole[g:g + n].view(shape)
    if init is not None:
        middle.fill_(init)
    return whole, middle


def guards_ok(whole, middle):
    g = (whole.numel() - middle.numel()) // 2
    return bool((whole[:g] == FILL[whole.dtype]).all()) and bool((whole[g + middle.numel():] == FILL[whole.dtype]).all())


def tree_words(n):
    """inner nodes of a 64-ary tree over n leaves: what tde_priority_words returns"""
    words = 0
    while True:
        n = -(-n // 64)
        words += n
        if n == 1:
            return words


class HandPriorities:
    def __init__(self, ring):
        self.ring, self.dev = ring, ring.dev
        self.ref = P.Priorities(ring.ref)
        if self.dev is None:
            return
        from torchdriveenv_amd import ops

        C, B = ring.C, ring.B
        self.whole, self.t = {}, {}
        # what reset must overwrite: every leaf and sum starts as rubbish
        for k, shape, dt, init in (("leaf", (C, B), torch.int32, 0x01234567), ("sums", (tree_words(C * B),), torch.int64, 0x0123456789),
                                   ("qmax", (1,), torch.int32, 7)):
            self.whole[k], self.t[k] = guarded(shape, dt, self.dev, init)
        self.pr = ops.priority_struct(ring.rp, self.t["leaf"], self.t["sums"], self.t["qmax"])

    # ---- the entry points, on the device and in the statement ---------------------------------------------------------------------------
    def reset(self):
        if self.dev is not None:
            from torchdriveenv_amd import ops

            ops.priority_reset(self.pr, self.ring.rp, self.dev)
        self.ref.reset()
        self.check(invariant=self.ring.count == 0)          # (a reset beside stored transitions makes them undrawable: not the invariant)

    def begin(self, mask=None):
        self.ring.begin(self.ring.rows(), mask)
        self.check()                                        # a masked begin changes no priority and breaks no invariant

    def step(self, done_bits=None):
        """a push of the ring, then of the priorities"""
        g = self.ring
        g.step(None if done_bits is None else np.asarray(done_bits, np.uint8))
        if self.dev is not None:
            from torchdriveenv_amd import ops

            ops.priority_push(self.pr, g.rp, self.dev, (g.w - 1) % g.C, g.first, g.count)
        self.ref.push()
        self.check()

    def update(self, idx, p):
        idx, p = np.asarray(idx, np.int32).reshape(-1, 2), np.asarray(p, np.float32)
        g = self.ring
        if self.dev is not None:
            from torchdriveenv_amd import ops

            ops.priority_update(self.pr, g.rp, self.dev, g.first, g.count, torch.from_numpy(idx).to(self.dev), torch.from_numpy(p).to(self.dev))
        named = self.ref.update(idx, p)
        self.check()
        return named

    def set_all(self, q):
        """every drawable pair takes the integer priority q (a scalar or one per pair, in valid_pairs() order)"""
        pairs = self.ring.ref.valid_pairs()
        q = np.broadcast_to(np.asarray(q, np.int64), (len(pairs),))
        assert (q >= 1).all() and (q <= QMAX).all() and np.array_equal(P.quantise(q.astype(np.float32) / np.float32(65536)), q)
        self.update(pairs, q.astype(np.float32) / np.float32(65536))
        return pairs

    def check(self, invariant=True):
        """the invariant in the statement; on the device leaf, sums[0], qmax and every canary bit for bit"""
        assert not invariant or np.array_equal(self.ref.leaf != 0, P.valid_mask(self.ring.ref))
        assert ONE <= self.ref.qmax <= QMAX
        if self.dev is None:
            return
        assert np.array_equal(self.t["leaf"].cpu().numpy().view(np.uint32), self.ref.leaf), "leaf"
        assert int(self.t["sums"][0]) == self.ref.total, "sums[0]"
        assert int(self.t["qmax"][0]) == self.ref.qmax, "qmax"
        for k in self.t:
            assert guards_ok(self.whole[k], self.t[k]), k

    def draw(self, n, seed, draw):
        """the statement's draw; on the device tde_priority_sample into guarded outputs, held to it bit for bit"""
        idx, q, us = self.ref.draw(seed, draw, n)
        if self.dev is not None:
            from torchdriveenv_amd import ops

            g = self.ring
            wi, ti = guarded((n, 2), torch.int32, self.dev)
            wq, tq = guarded((n,), torch.int32, self.dev)
            ops.priority_sample(self.pr, g.rp, self.dev, g.first, g.count, n, ti, tq, seed, draw)
            assert np.array_equal(ti.cpu().numpy(), idx), ("idx", n, seed, draw)
            assert np.array_equal(tq.cpu().numpy().view(np.uint32), q), ("q", n, seed, draw)
            assert guards_ok(wi, ti) and guards_ok(wq, tq)
            self.check()                                    # the draw writes nothing else
        return idx, q, us


# ---- the draws ----------------------------------------------------------------------------------------------------------------------------
SEED = 0x0123456789ABCDEF
BIG_DRAW = 2**32 + 5                                        # a draw counter whose high word counts
SHAPES = {"one_level": dict(C=4, B=5), "partial_block": dict(C=12, B=5), "three_levels": dict(C=40, B=130)}
PUSHES = {"one_level": 6, "partial_block": 17, "three_levels": 57}     # each ring wraps: the open slot lies inside the live range


def filled(shape, n_stack, dev=None, ends=True):
    """a wrapped ring of that shape with priorities pushed beside it; with `ends`, episodes end at random so that ages differ"""
    c = SHAPES[shape]
    ring = U.HandRing(c["C"], c["B"], n_stack, plane=16, dev=dev, seed=7 + n_stack)
    hp = HandPriorities(ring)
    ring.begin(ring.rows())
    hp.reset()
    for _ in range(PUSHES[shape]):
        hp.step(((ring.rng.uniform(size=ring.B) < 0.15) * ring.rng.integers(1, 4, ring.B)) if ends else None)
    return hp


def priorities_of(kind, hp):
    """integer priorities for every drawable pair"""
    m = len(hp.ring.ref.valid_pairs())
    rng = np.random.default_rng(m)
    if kind == "ones":
        return np.ones(m, np.int64)
    if kind == "equal":
        return np.full(m, ONE, np.int64)
    if kind == "qmax_among_ones":
        q = np.ones(m, np.int64)
        q[(2 * m) // 3] = QMAX
        return q
    assert kind == "mixed"
    return rng.integers(1, 1 << 22, m) * rng.choice([1, 1, 16], m)


KINDS = ("mixed", "ones", "equal", "qmax_among_ones")


def draw_settings(kind, m):
    """(N, seed, draw) for a case with m drawable pairs"""
    ns = [(1, SEED, 0), (7, SEED, 1), (256, SEED, BIG_DRAW), (256, SEED + 1, 2**63 + 1)]
    if kind == "ones":
        # T = m: N = m puts every position on a leaf edge (span 1), a divisor of m strides whole leaves, N > T has base == 0
        ns += [(m, SEED, 2), (m + 13, SEED, 3)] + [(d, SEED, 4) for d in (5, 13) if m % d == 0]
    if kind == "equal":
        ns += [(m, SEED, 5), (2 * m, SEED, 6)]              # N divides T = m * ONE: strata edges fall on leaf edges
    return ns


def past_zero_block(leaf, picks, B):
    """does a pick lie behind a 64-leaf block that is wholly zero, with a live leaf before that block?"""
    flat = leaf.reshape(-1)
    n = len(flat)
    blocks = [b for b in range(n // 64) if not flat[64 * b:64 * b + 64].any() and flat[:64 * b].any()]
    l = picks[:, 0].astype(np.int64) * B + picks[:, 1]
    return any((l >= 64 * (b + 1)).any() for b in blocks)


# ---- the updates ----------------------------------------------------------------------------------------------------------------------------
F = np.float32
QUANT_EDGES = [(F(0.0), 1), (F(-1.0), 1), (F("nan"), 1), (F("inf"), QMAX), (F(2.0**-17), 1), (F(1.5 / 65536), 2), (F(2.5 / 65536), 2),
               (F(3.5 / 65536), 4), (F(2.0**13), QMAX), (F(4095.99), 268434800), (F(1.0), ONE), (F(-0.0), 1), (F("-inf"), 1),
               (F(1e-30), 1), (F(3.0e38), QMAX)]
