"""CPU checks of the sequence sample (include/tde_sequence.h, torchdriveenv_amd/replay.py): the header's constant (the header beside the others,
its symbols and the loader's refusals: tests/test_abi_families_cpu.py), every host-side rejection of the entry point, of the ops wrapper and of sample_sequence's arguments (all before any
launch: no GPU needed), the numpy restatement (tests/sequence_ref.py) against a brute force written here, the draw, and the case tables
(tests/sequence_cases.py) that tests/test_gpu_sequence.py runs on the GPU, held to the conditions that make them mean something."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import nstep_ref as N
from tests import sequence_cases as K
from tests import sequence_ref as S
from tests.replay_ref import ENDED, PAL
from tests.ring_util import HAS
from tests.test_abi_families_cpu import c_status
from tests.test_replay_cpu import BAD_STRUCTS, _Host
from torchdriveenv_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- header, symbols, constants -----------------------------------------------------------------------------------------------------
def test_constants_match_header(tmp_path):
    assert c_status(tmp_path, ["tde_sequence.h", "tde_nstep.h"], "(TDE_SEQUENCE_MAX - 256) | (TDE_NSTEP_MAX - 64)") == 0
    text = open(os.path.join(ROOT, "include", "tde_sequence.h")).read()
    assert int(re.search(r"#define TDE_SEQUENCE_MAX (\d+)", text).group(1)) == _abi.SEQUENCE_MAX == S.SEQUENCE_MAX == 256


# ---- every host-side refusal, before any launch -------------------------------------------------------------------------------------
def test_entry_point_rejects_bad_arguments_without_a_launch():
    from torchdriveenv_amd import _lib

    L = _lib.load()
    h = _Host()                                             # C = 6, B = 3, n_stack = 3, plane = 64
    M, T = 2, 3
    pool, ref = np.zeros((6, M, 64), np.uint8), np.zeros((6, 3), np.int32)
    idx, obs = np.zeros((4, 2), np.int32), np.zeros((4, T + 1, 9, 64), np.uint8)
    oa, orw, od, ol = np.zeros((4, T, 2), np.float32), np.zeros((4, T), np.float32), np.zeros((4, T), np.uint8), np.zeros(5, np.int32)
    given = np.zeros((4, 2), np.int32)
    ptr = lambda a: a.ctypes.data

    def tm(**over):
        a = {**dict(M=M, pool=ptr(pool), ref=ptr(ref)), **over}
        return _abi.TdeTerminal(a["M"], a["pool"], a["ref"])

    def sample(rp=None, t=None, pooled=True, first=0, count=4, N_=4, idx_in=None, T_=T, out=None, null_rp=False):
        o = {**dict(idx=ptr(idx), obs=ptr(obs), action=ptr(oa), reward=ptr(orw), done=ptr(od), length=ptr(ol)), **(out or {})}
        return L.tde_sequence_sample(None if null_rp else C.byref(rp or h.rp()), C.byref(t or tm()) if pooled else None, first, count, N_,
                                     idx_in, 1, 0, T_, o["idx"], o["obs"], o["action"], o["reward"], o["done"], o["length"], None)

    def refused(fragment, **kw):
        rc, err = sample(**kw), L.tde_last_error()
        assert rc != 0 and fragment in err and err.startswith(b"tde_sequence_sample: "), (fragment, sorted(kw), rc, err)

    for pooled in (False, True):
        refused(b"NULL argument", null_rp=True, pooled=pooled)
        for over, fragment in BAD_STRUCTS:                  # the ring's own rules, as every replay entry point states them
            refused(fragment, rp=h.rp(**over), pooled=pooled)
        refused(b"16-byte aligned", rp=h.rp(frames=h.frames.ctypes.data + 4), pooled=pooled)
        for T_ in (0, -1, 257, 2**31 - 1):
            refused(b"T must be in [1, 256]", T_=T_, pooled=pooled)
            refused(b"T must be in [1, 256]", T_=T_, idx_in=ptr(given), pooled=pooled)
        for n in (0, -2):
            refused(b"N must be >= 1", N_=n, pooled=pooled)
        for count in (0, -1):
            refused(b"count must be >= 1", count=count, pooled=pooled)
        refused(b"count must be <= C - 1", count=6, pooled=pooled)
        for first in (-1, 6):
            refused(b"first must be in [0, C)", first=first, pooled=pooled)
        for name in ("idx", "obs", "action", "reward", "done", "length"):
            refused(b"a NULL output", out={name: None}, pooled=pooled)
        for count in (1, 2):
            refused(b"count must be > n_stack - 1", count=count, pooled=pooled)
        refused(b"16-byte aligned", out={"obs": ptr(obs) + 8}, pooled=pooled)
        refused(b"action 8-byte", out={"action": ptr(oa) + 4}, pooled=pooled)
        refused(b"reward / idx 4-byte", out={"reward": ptr(orw) + 2}, pooled=pooled)
        refused(b"reward / idx 4-byte", out={"idx": ptr(idx) + 2}, pooled=pooled)
        refused(b"reward / idx 4-byte", idx_in=ptr(given) + 2, pooled=pooled)
        refused(b"length must be 4-byte aligned", out={"length": ptr(ol) + 2}, pooled=pooled)
    for bad_m in (0, -1, 4):
        refused(b"M must be in [1, B]", t=tm(M=bad_m))
    refused(b"a NULL array in the terminal pool", t=tm(pool=None))
    refused(b"a NULL array in the terminal pool", t=tm(ref=None))
    refused(b"pool must be 16-byte aligned", t=tm(pool=ptr(pool) + 8))
    refused(b"ref 4-byte", t=tm(ref=ptr(ref) + 2))
    # nothing was written by any of the calls above
    for a in (h.frames, h.action, h.reward, h.done, h.age, pool, ref, idx, obs, oa, orw, od, ol):
        assert not a.view(np.uint8).any()


def test_ops_wrapper_rejects_host_tensors_and_bad_arguments():
    import torch

    from torchdriveenv_amd import ops

    z = torch.zeros
    rp, tm = _abi.TdeReplay(6, 4, 3, 64, 0, None, None, None, None, None), _abi.TdeTerminal(2, None, None)
    for t in (None, tm):
        for T in (0, -3, 257):
            with pytest.raises(ValueError, match=r"T must be in \[1, 256\]"):
                ops.sequence_sample(rp, t, "cuda:0", 0, 4, 2, T, {})
        with pytest.raises(ValueError, match="n must be >= 1"):
            ops.sequence_sample(rp, t, "cuda:0", 0, 4, 0, 3, {})
        with pytest.raises(ValueError, match="observations must live on a HIP device"):
            ops.sequence_sample(rp, t, "cuda:0", 0, 4, 2, 3, {"observations": z((2, 4, 9, 64), dtype=torch.uint8)})
        with pytest.raises(ValueError, match="observations must be torch.uint8"):
            ops.sequence_sample(rp, t, "cuda:0", 0, 4, 2, 3, {"observations": z((2, 4, 9, 64))})


def test_sample_sequence_arguments_are_refused_without_a_gpu():
    import inspect

    import torch

    from torchdriveenv_amd.config import Prioritized
    from torchdriveenv_amd.replay import ReplayBuffer, ReplaySamples, SequenceSamples

    sig = inspect.signature(ReplayBuffer.sample_sequence).parameters
    assert list(sig) == ["self", "n", "length", "idx", "check", "prioritized", "beta"]
    assert (sig["idx"].default, sig["check"].default, sig["prioritized"].default, sig["beta"].default) == (None, True, False, None)
    assert SequenceSamples._fields == ("observations", "actions", "rewards", "dones", "lengths", "indices", "priorities", "weights")
    buf = ReplayBuffer.__new__(ReplayBuffer)                # a buffer in host memory: every refusal comes before the first device call
    buf.dev, buf.C, buf.B, buf.n_stack, buf.first, buf.count, buf.draws = torch.device("cpu"), 6, 3, 3, 1, 4, 5
    buf.age = torch.tensor([[0] * 3, [0, 1, 2], [1, 2, 3], [2, 0, 4], [3, 1, 5], [4, 2, 6]], dtype=torch.uint8)
    for length in (0, -1, 257):
        with pytest.raises(ValueError, match=r"length must be in \[1, 256\]"):
            buf.sample_sequence(4, length)
    for n in (0, -1, None):
        with pytest.raises(ValueError, match="n must be >= 1"):
            buf.sample_sequence(n, 3)
    with pytest.raises(ValueError, match=r"idx must hold 3 \(slot, env\) pairs"):
        buf.sample_sequence(3, 3, idx=[(1, 0), (2, 0)])
    for bad in ((0, 0), (1, 2), (2, 2), (5, 0), (2, 3), (6, 0), (-1, 0), (2, -1)):
        with pytest.raises(ValueError, match=r"not stored transitions with their whole frame stack in the ring \(valid_pairs\(\)\)"):
            buf.sample_sequence(None, 3, idx=[(1, 0), bad, (3, 1)])
    with pytest.raises(ValueError, match=r"sample_sequence\(prioritized=True\) needs a buffer built with prioritized=Prioritized"):
        buf.sample_sequence(4, 3, prioritized=True)
    with pytest.raises(ValueError, match="beta needs prioritized=True"):
        buf.sample_sequence(4, 3, beta=0.5)
    buf.pstruct, buf.prioritized = object(), Prioritized()
    with pytest.raises(ValueError, match="idx or prioritized=True, not both"):
        buf.sample_sequence(None, 3, idx=[(1, 0)], prioritized=True)
    for beta in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"beta must be in \[0, 1\]"):
            buf.sample_sequence(4, 3, prioritized=True, beta=beta)
    for n in (0, -1, None):
        with pytest.raises(ValueError, match="n must be >= 1"):
            buf.sample_sequence(n, 3, prioritized=True)
    buf.count = 2
    with pytest.raises(ValueError, match=r"sample_sequence\(\) draws steps .* needs more than 2 stored steps, the buffer holds 2"):
        buf.sample_sequence(4, 3)
    buf.count = 0
    with pytest.raises(ValueError, match="holds no transition yet"):
        buf.sample_sequence(4, 3)
    with pytest.raises(ValueError, match="holds no transition yet"):
        buf.sample_sequence(4, 3, prioritized=True)
    assert buf.draws == 5                                   # a refused call draws nothing
    # .mask, .terminal and .bootstrap: ReplaySamples' rules on the done byte of step lengths - 1
    d = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    dones = torch.zeros((256, 4), dtype=torch.uint8)
    lengths = (torch.arange(256) % 4 + 1).to(torch.int32)
    dones[torch.arange(256), lengths.long() - 1] = d
    a, b = SequenceSamples(None, None, None, dones, lengths, None, None, None), ReplaySamples(None, None, None, d, None, None)
    assert torch.equal(a.bootstrap, b.bootstrap) and torch.equal(a.terminal, b.terminal)
    assert a.mask.dtype is torch.bool and torch.equal(a.mask.sum(1).to(torch.int32), lengths) and bool(a.mask[:, 0].all())
    zero = SequenceSamples(None, None, None, torch.zeros((2, 3), dtype=torch.uint8), torch.tensor([0, 3], dtype=torch.int32), None, None, None)
    assert zero.mask.tolist() == [[False] * 3, [True] * 3]


# ---- the restatement against a brute force -----------------------------------------------------------------------------------------------
def stack_of(ring, t, e, off):
    """the observation whose newest frame is slot t, off slots after `first`: written out frame by frame"""
    if not ring.plane:
        return ring.frames[t % ring.C, e].copy()
    ns = ring.n_stack
    out = np.zeros((ns, 3, ring.plane), np.uint8)
    for f in range(ns):
        d = ns - 1 - f
        if d <= int(ring.age[t % ring.C, e]) and d <= off:
            out[f] = PAL[ring.frames[(t - d) % ring.C, e]].T
    return out.reshape(3 * ns, ring.plane)


def brute(ring, s, e, T, pool):
    """walk the window one step at a time from the stored pair (s, e): (obs [T + 1], action, reward, done [T], m)"""
    per = (3 * ring.n_stack, ring.plane) if ring.plane else (ring.D,)
    obs = np.zeros((T + 1,) + per, ring.frames.dtype)
    act, rew, done = np.zeros((T, 2), np.float32), np.zeros(T, np.float32), np.zeros(T, np.uint8)
    off, k = int(ring.offset(s)), 0
    while True:
        t = (s + k) % ring.C
        obs[k] = stack_of(ring, t, e, off + k)
        act[k], rew[k], done[k] = ring.action[t, e], ring.reward[t, e], ring.done[t, e]
        kept = pool and done[k] & 3 and ring.ref[t, e] >= 0
        if kept:
            done[k] |= HAS
        k += 1
        if done[k - 1] & ENDED or k == T or off + k == ring.count:
            break
    if kept:
        if ring.plane:
            ns = ring.n_stack
            nxt = obs[k].reshape(ns, 3, ring.plane)
            nxt[:ns - 1] = obs[k - 1].reshape(ns, 3, ring.plane)[1:]
            nxt[ns - 1] = PAL[ring.pool[t, ring.ref[t, e]]].T
        else:
            obs[k] = ring.pool[t, ring.ref[t, e]]
    elif not done[k - 1] & ENDED:
        obs[k] = stack_of(ring, (s + k) % ring.C, e, off + k)
    return obs, act, rew, done, k


RINGS = [dict(n_stack=3, plane=16), dict(n_stack=1, plane=16), dict(n_stack=8, plane=16), dict(D=5)]


@pytest.mark.parametrize("shape", RINGS, ids=str)
@pytest.mark.parametrize("pool", (False, True))
def test_restatement_equals_the_brute_force(shape, pool):
    ring = K.history_ring(pool=pool, **shape)
    assert (ring.first, ring.w, ring.count) == (6, 5, 11)
    pairs = ring.stored_pairs()
    for T in K.T_STEPS:
        got = S.gather(ring.ref, pairs, T)
        nst = N.gather(ring.ref, pairs, T, 0.99)
        assert np.array_equal(got["lengths"], nst["steps"]) and np.array_equal(got["indices"], pairs)
        for i, (s, e) in enumerate(pairs):
            obs, act, rew, done, m = brute(ring.ref, int(s), int(e), T, pool)
            assert got["lengths"][i] == m
            for k, w in (("observations", obs), ("actions", act), ("rewards", rew), ("dones", done)):
                assert np.array_equal(got[k][i].view(np.uint8), w.view(np.uint8)), (k, T, s, e)
        if T == 1:                                          # the one-step samplers' outputs
            one = N.one_step(ring.ref, pairs, pool)
            assert np.array_equal(got["observations"][:, 0], one["observations"]) and np.array_equal(got["observations"][:, 1], one["next_observations"])
            assert np.array_equal(got["dones"][:, 0], one["dones"]) and np.array_equal(got["rewards"][:, 0], one["rewards"])
    got = S.gather(ring.ref, K.INVALID, 5)
    assert np.array_equal(got["indices"], np.array(K.INVALID, np.int32))
    assert not any(got[k].any() for k in got if k != "indices")


# ---- the case tables mean something -----------------------------------------------------------------------------------------------------
def test_case_table_contains_every_reason():
    for pool in (False, True):
        ring = K.history_ring(plane=16, n_stack=3, pool=pool)
        seen, ms = set(), {T: set() for T in K.T_STEPS}
        for T in K.T_STEPS:
            for s, e in ring.stored_pairs():
                r, m = K.reasons(ring.ref, int(s), int(e), T)
                seen |= r
                ms[T].add(m)
        assert seen == set(K.REASONS) - (set() if pool else K.POOLED), sorted(set(K.REASONS) ^ seen)
        assert ms[1] == {1} and ms[2] == {1, 2} and ms[5] == {1, 2, 3, 4, 5} and max(ms[11]) == max(ms[17]) == ring.count == 11
    # a window shorter and longer than the stack at every depth above 1; the shapes the issue names
    for ns, _ in K.PLANES:
        if ns > 1:
            assert any(m < ns for T in K.T_STEPS for m in ms[T]) and any(m >= ns for T in K.T_STEPS for m in ms[T])
    assert K.PLANES == ((1, 16), (3, 2304), (8, 4096), (3, 4096), (8, 16)) and K.ROWS == (5, 65) and K.T_STEPS == (1, 2, 5, 11, 17)
    assert (K.C, K.B, K.M) == (12, 5, 2)
    for p in K.INVALID:
        assert not N.stored(ring.ref, *p)


def test_long_ring_places_endings_around_the_rounds_of_the_length_search():
    ring = K.long_ring()
    assert (ring.C, ring.B, ring.n_stack, ring.plane) == (300, 2, 2, 16) and (ring.first, ring.count) == (0, 280)
    assert K.LONG_T == (64, 65, 130, 256)
    for start, m in K.LONG_LENGTHS.items():
        assert N.stored(ring.ref, start, 0)
        for T in K.LONG_T:
            got = S.gather(ring.ref, [(start, 0), (start, 1)], T)["lengths"]
            assert got[0] == min(m, T) and got[1] == min(T, ring.count - start)
    assert sorted(K.LONG_LENGTHS.values()) == [64, 65, 129]
    lengths = S.gather(ring.ref, K.long_pairs(), 256)["lengths"]
    assert lengths.max() == 256 and lengths.min() == 1 and {63, 64, 65, 128, 129, 255} <= set(lengths.tolist())


def test_age_ring_is_saturated_along_a_window():
    ring = K.age_ring(D=5)
    slots = [(ring.first + off) % ring.C for off in range(ring.count)]
    assert ring.count == ring.C - 1 and all(ring.ref.age[s, 0] == 255 for s in slots + [ring.w])
    assert S.gather(ring.ref, [(slots[0], 0), (slots[0], 1)], 17)["lengths"].tolist() == [ring.count, ring.count - 2]


# ---- the draw ---------------------------------------------------------------------------------------------------------------------------------
def test_a_drawn_window_fits_and_the_draw_of_one_step_is_the_replay_draw():
    ring = K.history_ring(plane=16, n_stack=3).ref
    assert ring.count == 11 and ring.skip == 2
    for T in (1, 2, 5, 9, 10, 11, 17, 256):
        idx = S.draw(ring, 7, 3, 4096, T)
        off = ring.offset(idx[:, 0])
        assert off.min() >= ring.skip and off.max() < ring.count and idx[:, 1].min() == 0 and idx[:, 1].max() == ring.B - 1
        if ring.count - ring.skip >= T:
            assert (off + T <= ring.count).all() and off.max() == ring.count - T and off.min() == ring.skip
            lengths = S.gather(ring, idx, T)["lengths"]
            short = lengths < T                             # only an ending shortens a window that was drawn
            last = (idx[:, 0] + lengths - 1) % ring.C
            assert (ring.done[last[short], idx[short, 1]] & ENDED).all()
        else:
            assert (off == ring.skip).all()                 # no window fits: the oldest drawable start, as long as the range allows
    for draw in (0, 1, 2**32, 2**32 + 1):
        assert np.array_equal(S.draw(ring, 0x123456789ABCDEF0, draw, 257, 1), ring.draw(0x123456789ABCDEF0, draw, 257))
    assert not np.array_equal(S.draw(ring, 7, 3, 257, 5), ring.draw(7, 3, 257))
