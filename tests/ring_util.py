"""A replay ring filled by hand through the C-ABI (include/tde_replay.h, tde_onpolicy.h, tde_terminal.h), without an env: HandRing owns
the device tensors of a tde_replay - each with canaries on either side - and, when asked, of a tde_terminal, together with the numpy
restatement (tests/replay_ref.Ring / tests/terminal_ref.TerminalRing) that is fed the same arrays.  first, w and count are the
restatement's: the host-side bookkeeping is stated there and nowhere else.  Without a device (dev=None) only the restatement is driven,
so that tests/test_ring_edges_cpu.py can hold the case tables below - which tests/test_gpu_ring_edges.py runs on the GPU - to the
conditions that make each case mean something."""
import numpy as np
import torch

from tests import replay_ref as R
from tests import terminal_ref as TR
from torchdriveenv_amd import _abi

CUT, HAS, BLANK = _abi.REPLAY_CUT, _abi.TERMINAL_HAS, _abi.LAYER_BLANK
FIELDS = ("observations", "next_observations", "actions", "rewards", "dones", "indices")
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
GUARD = 64                                                  # canary elements on either side of a tensor, at least
FILL = {torch.uint8: 0xA5, torch.float32: -12345.5, torch.int32: -77}      # what a canary, and an output before the call, holds


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint8) if a.dtype in (np.float32, np.uint8) else a


def guarded(shape, dtype, dev, init=None):
    """(whole, middle): `middle` has `shape` and lies between two runs of canaries, each GUARD elements or one row (shape[1:]) long,
    whichever is more, rounded to 16 elements so that `middle` keeps the allocation's 16-byte alignment"""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    g = -(-max(GUARD, int(np.prod(shape[1:]))) // 16) * 16
    whole = torch.full((n + 2 * g,), FILL[dtype], dtype=dtype, device=dev)
    middle = whole[g:g + n].view(shape)
    if init is not None:
        middle.fill_(init)
    return whole, middle


def guards_ok(whole, middle):
    g = (whole.numel() - middle.numel()) // 2
    f = FILL[whole.dtype]
    return bool((whole[:g] == f).all()) and bool((whole[g + middle.numel():] == f).all())


class HandRing:
    """C slots x B envs in planes mode (plane > 0) or rows mode (D > 0), with M > 0 pool rows per slot when the terminal pool is wanted.
    dev=None: the restatement alone."""

    def __init__(self, C, B, n_stack=1, plane=0, D=0, M=0, dev=None, seed=0):
        self.C, self.B, self.n_stack, self.plane, self.D, self.M, self.dev = C, B, n_stack, plane, D, M, dev
        self.ref = TR.TerminalRing(C, B, M, n_stack, plane, D) if M else R.Ring(C, B, n_stack, plane, D)
        self.per, self.np_dt = (plane, np.uint8) if plane else (D, np.float32)
        self.rng = np.random.default_rng(seed)
        self.names = ("frames", "action", "reward", "done", "age") + (("pool", "ref") if M else ())
        if dev is None:
            return
        from torchdriveenv_amd import ops

        dt = torch.uint8 if plane else torch.float32
        spec = {"frames": ((C, B, self.per), dt, BLANK if plane else 0), "action": ((C, B, 2), torch.float32, 0),
                "reward": ((C, B), torch.float32, 0), "done": ((C, B), torch.uint8, 0), "age": ((C, B), torch.uint8, 0),
                "pool": ((C, M, self.per), dt, BLANK if plane else 0), "ref": ((C, B), torch.int32, -1)}
        self.whole, self.t = {}, {}
        for k in self.names:
            self.whole[k], self.t[k] = guarded(spec[k][0], spec[k][1], dev, spec[k][2])
        self.rp = ops.replay_struct(C, B, n_stack, plane, D, *[self.t[k] for k in self.names[:5]])
        self.tm = ops.terminal_struct(self.rp, M, self.t["pool"], self.t["ref"]) if M else None

    first = property(lambda self: self.ref.first)
    w = property(lambda self: self.ref.w)
    count = property(lambda self: self.ref.count)

    # ---- filling -----------------------------------------------------------------------------------------------------------------
    def rows(self):
        """random frames [B, per]: layer codes 0 .. 7, or float32 rows"""
        if self.plane:
            return self.rng.integers(0, 8, (self.B, self.per)).astype(np.uint8)
        return self.rng.standard_normal((self.B, self.per)).astype(np.float32)

    def _src(self, rows, layout):
        """the device source of a begin / push: (tensor, src_offset, src_stride).  layout = (offset, stride) in bytes puts row e at
        byte offset + e * stride of a larger tensor whose other bytes hold a canary"""
        if layout is None:
            return torch.from_numpy(rows).to(self.dev), 0, None
        off, stride = layout
        row = rows[0].nbytes
        assert stride >= row and off % 4 == 0 and stride % 4 == 0
        big = np.full(off + self.B * stride, 0x5A, np.uint8)
        for e in range(self.B):
            big[off + e * stride:off + e * stride + row] = rows[e].view(np.uint8)
        return torch.from_numpy(big.view(self.np_dt)).to(self.dev), off, stride

    def begin(self, frame, mask=None, layout=None):
        frame = np.ascontiguousarray(frame, self.np_dt)
        mask = None if mask is None else np.asarray(mask, np.uint8)
        if self.dev is not None:
            from torchdriveenv_amd import ops

            src, off, stride = self._src(frame, layout)
            ops.replay_begin(self.rp, self.dev, self.w, src, off, stride, None if mask is None else torch.from_numpy(mask).to(self.dev))
        self.ref.begin(frame, mask)

    def push(self, action, reward, done_bits, frame, term=None, layout=None):
        action, reward = np.ascontiguousarray(action, np.float32), np.ascontiguousarray(reward, np.float32)
        done_bits, frame = np.ascontiguousarray(done_bits, np.uint8), np.ascontiguousarray(frame, self.np_dt)
        assert (term is not None) == bool(self.M)
        if self.dev is not None:
            from torchdriveenv_amd import ops

            src, off, stride = self._src(frame, layout)
            td = torch.from_numpy(done_bits).to(self.dev)
            ops.replay_push(self.rp, self.dev, self.w, torch.from_numpy(action).to(self.dev), torch.from_numpy(reward).to(self.dev), td,
                            src, off, stride)
            if self.M:
                ops.terminal_push(self.rp, self.tm, self.dev, self.w, td, torch.from_numpy(np.ascontiguousarray(term, self.np_dt)).to(self.dev))
        if self.M:
            self.ref.push(action, reward, done_bits, frame, np.ascontiguousarray(term, self.np_dt))
        else:
            self.ref.push(action, reward, done_bits, frame)

    def step(self, done_bits=None, layout=None):
        """a push of random actions, rewards, frames (and terminal frames)"""
        db = np.zeros(self.B, np.uint8) if done_bits is None else done_bits
        a, r = self.rng.standard_normal((self.B, 2)).astype(np.float32), self.rng.standard_normal(self.B).astype(np.float32)
        self.push(a, r, db, self.rows(), self.rows() if self.M else None, layout)

    def drop_oldest(self, k):
        """the host forgets the k oldest transitions: tde_replay_sample takes first and count from the host, and nothing but a push
        that wraps moves `first` otherwise"""
        assert 0 <= k < self.ref.count
        self.ref.first, self.ref.count = (self.ref.first + k) % self.C, self.ref.count - k

    # ---- checking ----------------------------------------------------------------------------------------------------------------
    def check_state(self):
        """every ring array and every canary bit for bit; returns (first, w, count)"""
        f, w, c = self.ref.first, self.ref.w, self.ref.count
        assert 0 <= f < self.C and 0 <= c <= self.C - 1 and w == (f + c) % self.C
        if self.dev is not None:
            for k in self.names:
                assert np.array_equal(bits(self.t[k].cpu().numpy()), bits(getattr(self.ref, k))), k
                assert guards_ok(self.whole[k], self.t[k]), k
        return f, w, c

    def stored_pairs(self):
        """every (slot, env) of the valid range, whether or not the older frames of its stack are still in the ring"""
        return np.array([((self.first + off) % self.C, e) for off in range(self.count) for e in range(self.B)], np.int32).reshape(-1, 2)

    def want_sample(self, idx, terminal):
        return self.ref.gather(idx) if terminal else R.Ring.gather(self.ref, idx)

    def check_sample(self, pairs=None, terminal=False, n=None, seed=0, draw=0):
        """tde_replay_sample (terminal: tde_terminal_sample) of the given pairs, or of n drawn ones, into guarded outputs, against the
        restatement byte for byte; returns (got, want)"""
        from torchdriveenv_amd import ops

        idx = self.ref.draw(seed, draw, n) if pairs is None else np.asarray(pairs, np.int32).reshape(-1, 2)
        n = len(idx)
        obs = ((n, 3 * self.n_stack, self.plane), torch.uint8) if self.plane else ((n, self.D), torch.float32)
        spec = {"observations": obs, "next_observations": obs, "actions": ((n, 2), torch.float32), "rewards": ((n,), torch.float32),
                "dones": ((n,), torch.uint8), "indices": ((n, 2), torch.int32)}
        whole, out = {}, {}
        for k, (shape, dt) in spec.items():
            whole[k], out[k] = guarded(shape, dt, self.dev)
        tin = None if pairs is None else torch.from_numpy(idx).to(self.dev)
        if terminal:
            ops.terminal_sample(self.rp, self.tm, self.dev, self.first, self.count, n, out, tin, seed, draw)
        else:
            ops.replay_sample(self.rp, self.dev, self.first, self.count, n, out, tin, seed, draw)
        want = self.want_sample(idx, terminal)
        got = {k: out[k].cpu().numpy() for k in FIELDS}
        for k in FIELDS:
            assert got[k].shape == want[k].shape and np.array_equal(bits(got[k]), bits(want[k])), (k, "terminal" if terminal else "replay")
            assert guards_ok(whole[k], out[k]), k
        return got, want


# ---- 1. tde_gae ----------------------------------------------------------------------------------------------------------------------
GAE_BLOCK = 16                                              # kGaeBlock of csrc/tde_onpolicy.hip
GAE_T = (1, 15, 16, 17, 31, 32, 33, 130)
GAE_B = (1, 63, 64, 65, 130)
GAE_SHAPES = [(T, 65) for T in GAE_T] + [(33, B) for B in GAE_B if B != 65] + [(130, 130)]
GAE_SETTINGS = ((0.99, 0.95), (1.0, 1.0), (0.99, 0.0), (0.0, 0.95), (0.5, 1.0))
GAE_BYTES = (1, 2, 3, CUT, CUT | 2)
GAE_EDGE_DISTANCES = (15, 16, 17, 31, 32)                   # T - 1 - t on either side of the first two block edges, counted from the top


def gae_marks(T):
    return sorted({0, T - 1} | {T - 1 - k for k in GAE_EDGE_DISTANCES if T - 1 - k >= 0})


def gae_done_pattern(T, B):
    """the endings of a rollout as (t, env, byte): env 0 ends at every mark, env 1 never, env 2 at every step, every later env at one
    mark - the marks in turn, the bytes in turn"""
    marks, out = gae_marks(T), []
    for e in range(B):
        if e == 0:
            out += [(t, e, GAE_BYTES[i % 5]) for i, t in enumerate(marks)]
        elif e == 2:
            out += [(t, e, GAE_BYTES[t % 5]) for t in range(T)]
        elif e >= 3:
            j = e - 3
            out.append((marks[j % len(marks)], e, GAE_BYTES[(j // len(marks) + j) % 5]))
    return out


GAE_DONE = {(T, B): gae_done_pattern(T, B) for T, B in GAE_SHAPES}


def gae_positions(T):
    """where the rollout lies in the ring, as (name, C, pushes, t_wrap): the ring has C slots and takes `pushes` steps, of which the
    last T are the rollout; t_wrap is the step whose slot is 0 after slot C - 1 (None: the rollout does not wrap)"""
    pos = [("base0", T + 2, T, None), ("lead", T + 4, T + 2, None)]
    C = T + 3
    if T == 1:
        return pos + [("last_slot", C, C, None)]            # (one step cannot wrap: it lies in slot C - 1)
    wraps = [("wrap_top", T - 1), ("wrap_mid", T - 1 - 8 if T >= 10 else T - 2)]
    if T - 1 - GAE_BLOCK >= 1:
        wraps.append(("wrap_edge", T - 1 - GAE_BLOCK))
    return pos + [(name, C, C + T - t, t) for name, t in wraps]


GAE_POSITIONS = {T: gae_positions(T) for T in GAE_T}


def gae_fill(ring, T, pushes, pattern):
    """`pushes` steps into a ring after its begin(): the last T carry `pattern`, the ones before them endings of their own, and every
    step of every env random infraction bits.  Returns the critic's values [T, B] and last_values [B]."""
    B, rng, lead = ring.B, ring.rng, pushes - T
    done = np.zeros((pushes, B), np.uint8)
    done[:lead] = np.where(rng.uniform(size=(lead, B)) < 0.3, rng.integers(1, 4, (lead, B)), 0)
    for t, e, byte in pattern:
        done[lead + t, e] = byte
    done |= (rng.integers(0, 8, (pushes, B)) << 2).astype(np.uint8)
    ring.begin(ring.rows())
    for p in range(pushes):
        ring.step(done[p])
    return (3 * rng.standard_normal((T, B))).astype(np.float32), (3 * rng.standard_normal(B)).astype(np.float32)


def gae_ring(T, B, C, dev=None):
    return HandRing(C, B, 1, plane=16, dev=dev, seed=1000 * T + B)


# ---- 2. the gathers ------------------------------------------------------------------------------------------------------------------
GATHER_SHAPES = ((8, 16), (8, 4096), (2, 2304), (1, 16), (3, 4080))        # (n_stack, plane); C = n_stack + 3
GATHER_B, GATHER_M = 3, 2
AGE_RING = dict(n_stack=8, plane=16, C=10, B=2)
AGE_STEPS = {254: 254, 255: 255, 256: 255, 260: 255}       # pushes without an ending -> the age of the open slot


def gather_history(ns):
    """("begin", mask or None) and ("push", done bits) in turn, for a ring of C = ns + 3 slots and three envs"""
    free = ("push", (0, 0, 0))
    return ([("begin", None)] + [free] * (ns + 1)           # age == off grows past every d
            + [("push", (1, 0, 0))]                         # env 0 terminates, its frame is kept
            + [free] * 2                                    # the ring wraps; env 0's new episode is young far behind `first`
            + [("push", (2, 0, 0)), ("begin", (1, 0, 0))]   # env 0 is truncated and kept, then reset by the caller: cut and kept
            + [free] * (ns + 2)                             # envs 1 and 2 grow older than the ring is long
            + [("begin", (0, 0, 1))]                        # env 2 is cut mid-episode
            + [free] * 2 + [("push", (1, 2, 3))]            # all three end: the pool of two overflows at env 2
            + [free] * 2)


GATHER_HISTORIES = {ns: gather_history(ns) for ns in sorted({s for s, _ in GATHER_SHAPES})}


def play(ring, history):
    """run a history, yielding after every call that leaves a stored transition"""
    for op, arg in history:
        if op == "begin":
            ring.begin(ring.rows(), arg)
        else:
            db = np.array(arg, np.uint8) | (ring.rng.integers(0, 8, ring.B) << 2).astype(np.uint8)
            ring.step(db)
        if ring.count:
            yield op


def blanking(ring, pairs):
    """what the blanking rule of the gathers meets in these stored pairs: the set of (k, d <= age, d <= off), d = n_stack - 1 - k"""
    seen = set()
    for s, e in pairs:
        age, off = int(ring.ref.age[s, e]), int(ring.ref.offset(s))
        seen |= {(k, ring.n_stack - 1 - k <= age, ring.n_stack - 1 - k <= off) for k in range(ring.n_stack)}
    return seen


# ---- 3. pairs that gather zeros ---------------------------------------------------------------------------------------------------------
# a ring of C = 8 slots and B = 4 envs after 11 pushes: first = 4, w = 3, count = 7; with the three oldest dropped first = 7, count = 4
INVALID_C, INVALID_B, INVALID_PUSHES = 8, 4, 11
INVALID_RINGS = {
    "full": dict(drop=0, state=(4, 3, 7),
                 invalid=[(-1, 0), (8, 0), (0, -1), (0, 4), (INT32_MIN, 0), (0, INT32_MAX), (3, 1)],
                 valid=[(4, 0), (7, 3), (0, 1), (2, 2), (5, 3), (1, 0), (6, 2)]),
    "short": dict(drop=3, state=(7, 3, 4),
                  invalid=[(-1, 0), (8, 0), (0, -1), (0, 4), (INT32_MIN, 0), (0, INT32_MAX), (3, 1), (5, 2), (4, 0), (6, 3)],
                  valid=[(7, 0), (0, 3), (1, 1), (2, 2), (7, 3), (0, 0), (2, 1), (1, 2), (7, 1), (2, 0)]),
}
INVALID_MODES = {"planes": dict(n_stack=3, plane=64), "rows": dict(D=5)}
INVALID_N = (1, 5, 9)                                       # the rows gather takes four transitions per workgroup


def interleaved(case):
    """invalid, valid, invalid, ...: a wrong `ok` in one row cannot hide behind its neighbours"""
    return [p for pair in zip(case["invalid"], case["valid"]) for p in pair]


def invalid_ring(mode, name, dev=None):
    ring = HandRing(INVALID_C, INVALID_B, M=2, dev=dev, seed=31, **INVALID_MODES[mode])
    ring.begin(ring.rows())
    for p in range(INVALID_PUSHES):
        # no stored transition may look like the zeros an invalid pair gathers: every done byte is nonzero
        db = np.where(ring.rng.uniform(size=ring.B) < 0.4, ring.rng.integers(1, 4, ring.B), 0) | (ring.rng.integers(1, 8, ring.B) << 2)
        ring.step(db.astype(np.uint8))
    ring.drop_oldest(INVALID_RINGS[name]["drop"])
    return ring


# ---- 4. the draw ------------------------------------------------------------------------------------------------------------------------
DRAW_CASES = {"one_slot": dict(C=6, B=4, n_stack=3, pushes=3), "one_env": dict(C=5, B=1, n_stack=1, pushes=7),
              "first_last": dict(C=5, B=4, n_stack=2, pushes=8)}
DRAWS = (0, 1, 2**32, 2**32 + 1)
DRAW_N, DRAW_SEED = 257, 0x123456789ABCDEF0


def draw_ring(name, dev=None):
    c = DRAW_CASES[name]
    ring = HandRing(c["C"], c["B"], c["n_stack"], plane=16, M=1, dev=dev, seed=41)
    ring.begin(ring.rows())
    for p in range(c["pushes"]):
        ring.step(((ring.rng.uniform(size=ring.B) < 0.3) * ring.rng.integers(1, 4, ring.B)).astype(np.uint8))
    return ring


# ---- 5. the seam ------------------------------------------------------------------------------------------------------------------------
SEAM_C = 4
# layout: (byte offset of env 0's row, bytes between rows) of the source tensor; the first is a layer ring's newest slot
SEAM_CASES = ([dict(n_stack=3, plane=64, D=0, B=5, layout=(2 * 64, 3 * 64)), dict(n_stack=1, plane=16, D=0, B=1, layout=(32, 48)),
               dict(n_stack=2, plane=2304, D=0, B=5, layout=(16, 2304 + 16))]
              + [dict(n_stack=1, plane=0, D=D, B=B, layout=(8, 4 * D + 12)) for D in (1, 5, 64, 65) for B in (1, 5)])


def seam_script(B):
    """two wraps of a four-slot ring: ("begin", mask) / ("push",); the masked begins come at w == 0 (twice, once with no env masked)
    and at w == 2"""
    even, third, none = [int(e % 2 == 0) for e in range(B)], [int(e % 3 == 0) for e in range(B)], [0] * B
    return ([("begin", None)] + [("push",)] * 4 + [("begin", even), ("begin", none)] + [("push",)] * 4 + [("begin", none), ("begin", third)]
            + [("push",)] * 2 + [("begin", even)] + [("push",)] * 3)


# ---- 6. tde_replay_pack -----------------------------------------------------------------------------------------------------------------
PACK_CASES = [(B, plane) for B in (1, 5) for plane in (16, 2304, 4096)]


def pack_colours():
    """uint8 [K, 3]: the palette, every colour that differs from one of its colours by 1 in exactly one channel, black and white"""
    out = [tuple(c) for c in _abi.PALETTE] + [(0, 0, 0), (255, 255, 255)]
    for c in _abi.PALETTE:
        for ch in range(3):
            for step in (-1, 1):
                if 0 <= c[ch] + step <= 255:
                    out.append(tuple(c[i] + (step if i == ch else 0) for i in range(3)))
    return np.array(sorted(set(out)), np.uint8)


PACK_COLOURS = pack_colours()
