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
        self.installed = False                              # leaves put in by install() do not follow the ring: no invariant to hold
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
            assert not self.t["sums"].any(), "sums"         # "every leaf and every word of sums = 0": not the total alone
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

    def install(self, leaf):
        """a whole [C][B] leaf array of the caller's (leaf is caller-owned memory; the pick "reads leaf and sums only") into the device
        tensor and into the statement; the sums are then made current as ReplayBuffer.load_state_dict makes them: an update whose one
        pair (-1, -1) is ignored changes no leaf, "then total is made current".  From here on the leaves do not follow the ring."""
        leaf = np.ascontiguousarray(leaf, np.uint32).reshape(self.ring.C, self.ring.B)
        assert int(leaf.max()) <= QMAX
        self.installed = True
        if self.dev is not None:
            self.t["leaf"].copy_(torch.from_numpy(leaf.view(np.int32)).to(self.dev))
        self.ref.leaf[:] = leaf
        assert self.update([(-1, -1)], [0.0]) == 0

    def check(self, invariant=True):
        """the invariant in the statement; on the device leaf, sums[0], qmax and every canary bit for bit"""
        invariant = invariant and not self.installed
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


# ---- every depth of the tree, leaf counts that fill their blocks exactly, and installed leaves ------------------------------------------------
def tree_lens(n):
    """[n, n_1, .., n_K = 1]: the nodes of every level of the 64-ary tree over n leaves"""
    lens = [int(n)]
    while True:
        lens.append(-(-lens[-1] // 64))
        if lens[-1] == 1:
            return lens


# n = C * B leaves, K inner levels, `words` of sums.  full_k: every level exactly full; tail_k: one leaf more, every level ends in a node
# of one child.  tail_4 also has B > 256 (the push runs in 205 workgroups) and n > 1024 * 256 (the second trip of the reset's loop).
DEPTH_SHAPES = {"full_1": dict(C=2, B=32, n=64, K=1, words=1), "tail_2": dict(C=5, B=13, n=65, K=2, words=2 + 1),
                "mid_2": dict(C=7, B=100, n=700, K=2, words=11 + 1), "full_2": dict(C=64, B=64, n=4096, K=2, words=64 + 1),
                "tail_3": dict(C=17, B=241, n=4097, K=3, words=65 + 2 + 1), "full_3": dict(C=64, B=4096, n=262144, K=3, words=4096 + 64 + 1),
                "tail_4": dict(C=5, B=52429, n=262145, K=4, words=4097 + 65 + 2 + 1)}
DEPTH_STACKED = ("tail_2", "mid_2", "full_2", "tail_3", "tail_4")      # run with n_stack = 3 as well: the push's loop over young stacks
ONES_MAX = 4097                                             # `ones` draws N = n and n + 13: the statement's strata loop in Python
UPDATED = 300                                               # pairs of the first update of depth_run, where the shape has as many


def depth_ring(shape, n_stack=1, dev=None):
    """a begun ring of a DEPTH_SHAPES row - frames do not matter here: 16 bytes each - with priorities that are still rubbish"""
    c = DEPTH_SHAPES[shape]
    ring = U.HandRing(c["C"], c["B"], n_stack, plane=16, dev=dev, seed=11 + n_stack)
    hp = HandPriorities(ring)
    ring.begin(ring.rows())
    return hp


def spread(m, k):
    """up to k of the indices 0 .. m - 1, evenly spread, 0 and m - 1 among them"""
    return np.unique(np.linspace(0, m - 1, min(k, m)).round().astype(np.int64))


def depth_run(shape, n_stack=1, dev=None):
    """reset over rubbish, C + 2 pushes (the ring wraps), an update of UPDATED valid pairs spread over the flat range with the first and
    the last valid pair among them, an update of other pairs, one more push - and 256 draws after each of the three: rebuild after
    rebuild, so that a top level that is not cleared between them shows.  Every call checks itself (HandPriorities).  Returns hp and
    the (named pairs, flat picks, their q) of the three rounds."""
    hp = depth_ring(shape, n_stack, dev)
    ring = hp.ring
    hp.reset()
    for _ in range(ring.C + 2):
        hp.step(((ring.rng.uniform(size=ring.B) < 0.15) * ring.rng.integers(1, 4, ring.B)) if n_stack > 1 else None)
    rounds = []
    for r in range(3):
        valid = np.argwhere(P.valid_mask(ring.ref)).astype(np.int32)       # flat order
        which = spread(len(valid), UPDATED)
        if r == 1:                                          # other pairs than the first update's, where the shape has any
            rest = np.setdiff1d(np.arange(len(valid)), which)
            which = rest[spread(len(rest), 257)] if len(rest) else which[::2]
        if r < 2:
            p = np.exp(ring.rng.uniform(np.log(2.0**-10), np.log(100.0), len(which))).astype(np.float32)
            # the first and the last pair named weigh as much as thousands of the others: they are drawn, wherever in the tree they lie
            p[0], p[-1] = 2048.0 / (r + 1), 4096.0 / (r + 1)
            assert hp.update(valid[which], p) == len(which)
        else:
            hp.step()
        idx, q, _ = hp.draw(256, SEED, 40 + r)
        rounds.append((valid[which], idx[:, 0].astype(np.int64) * ring.B + idx[:, 1], q))
    return hp, rounds


def _last_only(n):
    leaf = np.zeros(n, np.uint32)
    leaf[n - 1] = 1
    return leaf


def _first_only(n):
    leaf = np.zeros(n, np.uint32)
    leaf[0] = 1
    return leaf


def _lane_edges(n):
    """nonzero at the first and the last lane of every level-1 node alone: 1 or 2 at lane 0, 3 at lane 63"""
    l = np.arange(n)
    return np.where(l % 64 == 0, 1 + (l // 64) % 2, np.where(l % 64 == 63, 3, 0)).astype(np.uint32)


def _far_apart(n):
    """live leaves in the first and in the last level-1 block, and at the first leaf of the last level-2 and of the last level-3
    subtree where the shape has more than one: whole subtrees of 4096 and of 262144 leaves in between are zero"""
    lens = tree_lens(n)
    live = np.zeros(n, bool)
    live[:64] = live[64 * (lens[1] - 1):] = True
    for k in (2, 3):
        if len(lens) - 1 > k:
            live[64**k * (lens[k] - 1)] = True
    return (live * np.random.default_rng(n).integers(1, 1000, n)).astype(np.uint32)


def _far_apart_late(n):
    """far_apart with the root's whole first child zero: the first 64^(K - 1) leaves.  In the tail shapes the only subtrees that lie
    wholly before a live leaf are the root's first child and what it holds, so that it takes this variant to pick behind a zero one."""
    leaf = _far_apart(n)
    leaf[:64 ** (len(tree_lens(n)) - 2)] = 0
    return leaf


def _mixed_dense(n):
    """priorities_of("mixed"), over all n leaves"""
    rng = np.random.default_rng(n)
    return (rng.integers(1, 1 << 22, n) * rng.choice([1, 1, 16], n)).astype(np.uint32)


PATTERNS = {"last_only": _last_only, "first_only": _first_only, "lane_edges": _lane_edges, "far_apart": _far_apart,
            "far_apart_late": _far_apart_late, "all_qmax": lambda n: np.full(n, QMAX, np.uint32), "ones": lambda n: np.ones(n, np.uint32),
            "mixed_dense": _mixed_dense}
# the pattern installed over each, without a reset in between: far from the first, so that a sum left over from it is a wrong pick
OVER = {"last_only": "mixed_dense", "first_only": "all_qmax", "lane_edges": "far_apart", "far_apart": "lane_edges",
        "far_apart_late": "first_only", "all_qmax": "last_only", "ones": "far_apart", "mixed_dense": "last_only"}


def patterns_of(shape):
    c = DEPTH_SHAPES[shape]
    return [k for k in PATTERNS if (k != "ones" or c["n"] <= ONES_MAX) and (k != "far_apart_late" or c["K"] >= 2)]


INSTALLED_CASES = [(shape, pattern) for shape in DEPTH_SHAPES for pattern in patterns_of(shape)]


def depth_draw_settings(pattern, leaf):
    """(N, seed, draw) for installed leaves: one sample, a few, a full sampler workgroup count with a wide draw counter, a last sampler
    workgroup that is not full; never more than 4096 samples (the statement's strata loop in Python)"""
    n, T = len(leaf), int(leaf.astype(np.int64).sum())
    ns = [(1, SEED, 0), (7, SEED, 1), (256, SEED, BIG_DRAW), (4093, SEED + 1, 2**63 + 1)]
    if pattern == "ones":
        assert n <= ONES_MAX
        ns += [(n, SEED, 2), (n + 13, SEED, 3)]             # span 1: every position on a leaf edge; N > T: base == 0
    if pattern == "lane_edges":
        ns += [(min(T, 4096), SEED, 4)]                     # span 1 or little more over leaves of 1 .. 3: many positions on leaf edges
    return ns


def installed_run(shape, pattern, dev=None):
    """three pushes, then: the pattern installed and every draw setting made; OVER[pattern] installed over it without a reset and drawn
    from; one real push and one real update of a few valid pairs on top of the installed leaves (the statement's push and update are
    defined on any leaf array), and drawn from once more.  Returns hp and one record per draw: the stage, the name of the leaves, N,
    the flat picks l, q, the positions us and the flat leaves they were drawn from."""
    hp = depth_ring(shape, 1, dev)
    ring, n = hp.ring, DEPTH_SHAPES[shape]["n"]
    hp.reset()
    for _ in range(3):
        hp.step()
    out = []

    def draws(stage, name):
        leaf = hp.ref.leaf.reshape(-1).copy()
        for N, seed, draw in depth_draw_settings(name, leaf):
            idx, q, us = hp.draw(N, seed, draw + 8 * stage)
            out.append(dict(stage=stage, pattern=name, N=N, draw=draw + 8 * stage, l=idx[:, 0].astype(np.int64) * ring.B + idx[:, 1], q=q,
                            us=us, leaf=leaf))

    hp.install(PATTERNS[pattern](n))
    draws(0, pattern)
    hp.install(PATTERNS[OVER[pattern]](n))
    draws(1, OVER[pattern])
    hp.step()
    valid = np.argwhere(P.valid_mask(ring.ref)).astype(np.int32)
    named = valid[[0, len(valid) - 1, len(valid) // 2, len(valid) - 1]]
    assert hp.update(named, np.array([0.5, 3.0, 100.0, 7.0], np.float32)) == 4
    draws(2, "stepped")
    return hp, out


def behind_zero_subtree(leaf, l, size):
    """does a pick lie behind an aligned run of `size` leaves that is wholly zero?"""
    whole = len(leaf) // size
    zero = np.flatnonzero(~leaf[:whole * size].reshape(whole, size).any(1))
    return bool(len(zero)) and bool((np.asarray(l) >= size * (zero[0] + 1)).any())
