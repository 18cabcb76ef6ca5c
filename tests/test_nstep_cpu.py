"""CPU checks of the n-step sample (include/tde_nstep.h, torchdriveenv_amd/replay.py): the header's constant (the header beside the others, its
symbols and the loader's refusals: tests/test_abi_families_cpu.py), every host-side rejection of the entry point, of the ops wrapper and of sample_nstep's arguments (all before any launch:
no GPU needed), the numpy restatement (tests/nstep_ref.py) against a brute-force composition written here, and the case table
(tests/nstep_cases.py) that tests/test_gpu_nstep.py runs on the GPU, held to the conditions that make it mean something."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import nstep_cases as K
from tests import nstep_ref as N
from tests.replay_ref import ENDED
from tests.test_abi_families_cpu import c_status
from tests.test_replay_cpu import BAD_STRUCTS, _Host
from torchdriveenv_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- header, symbols, constants -----------------------------------------------------------------------------------------------------
def test_constants_match_header(tmp_path):
    assert c_status(tmp_path, ["tde_nstep.h"], "TDE_NSTEP_MAX - 64") == 0
    text = open(os.path.join(ROOT, "include", "tde_nstep.h")).read()
    assert int(re.search(r"#define TDE_NSTEP_MAX (\d+)", text).group(1)) == _abi.NSTEP_MAX == N.NSTEP_MAX == 64


# ---- every host-side refusal, before any launch -------------------------------------------------------------------------------------
def test_entry_point_rejects_bad_arguments_without_a_launch():
    from torchdriveenv_amd import _lib

    L = _lib.load()
    h = _Host()                                             # C = 6, B = 3, n_stack = 3, plane = 64
    M = 2
    pool, ref = np.zeros((6, M, 64), np.uint8), np.zeros((6, 3), np.int32)
    idx, obs, nxt = np.zeros((4, 2), np.int32), np.zeros((4, 9, 64), np.uint8), np.zeros((4, 9, 64), np.uint8)
    oa, orw, od = np.zeros((4, 2), np.float32), np.zeros(4, np.float32), np.zeros(4, np.uint8)
    og, os_ = np.zeros(5, np.float32), np.zeros(4, np.uint8)
    ptr = lambda a: a.ctypes.data

    def tm(**over):
        a = {**dict(M=M, pool=ptr(pool), ref=ptr(ref)), **over}
        return _abi.TdeTerminal(a["M"], a["pool"], a["ref"])

    def sample(rp=None, t=None, pooled=True, first=0, count=4, N_=4, idx_in=None, n_steps=3, gamma=0.99, out=None, null_rp=False):
        o = {**dict(idx=ptr(idx), obs=ptr(obs), next_obs=ptr(nxt), action=ptr(oa), reward=ptr(orw), done=ptr(od), discount=ptr(og),
                    steps=ptr(os_)), **(out or {})}
        return L.tde_nstep_sample(None if null_rp else C.byref(rp or h.rp()), C.byref(t or tm()) if pooled else None, first, count, N_, idx_in,
                                  1, 0, n_steps, gamma, o["idx"], o["obs"], o["next_obs"], o["action"], o["reward"], o["done"], o["discount"],
                                  o["steps"], None)

    def refused(fragment, **kw):
        rc, err = sample(**kw), L.tde_last_error()
        assert rc != 0 and fragment in err and err.startswith(b"tde_nstep_sample: "), (fragment, sorted(kw), rc, err)

    for pooled in (False, True):
        refused(b"NULL argument", null_rp=True, pooled=pooled)
        for over, fragment in BAD_STRUCTS:                  # the ring's own rules, as every replay entry point states them
            refused(fragment, rp=h.rp(**over), pooled=pooled)
        refused(b"16-byte aligned", rp=h.rp(frames=h.frames.ctypes.data + 4), pooled=pooled)
        for n_steps in (0, -1, 65, 2**31 - 1):
            refused(b"n_steps must be in [1, 64]", n_steps=n_steps, pooled=pooled)
        for gamma in (-0.5, 1.5, float("nan"), float("inf"), float("-inf"), np.nextafter(F(1), F(2)).item(), -1e-30):
            refused(b"gamma must be finite and in [0, 1]", gamma=gamma, pooled=pooled)
        for n in (0, -2):
            refused(b"N must be >= 1", N_=n, pooled=pooled)
        for count in (0, -1):
            refused(b"count must be >= 1", count=count, pooled=pooled)
        refused(b"count must be <= C - 1", count=6, pooled=pooled)
        for first in (-1, 6):
            refused(b"first must be in [0, C)", first=first, pooled=pooled)
        for name in ("idx", "obs", "next_obs", "action", "reward", "done", "discount", "steps"):
            refused(b"a NULL output", out={name: None}, pooled=pooled)
        for count in (1, 2):
            refused(b"count must be > n_stack - 1", count=count, pooled=pooled)
        refused(b"16-byte aligned", out={"obs": ptr(obs) + 8}, pooled=pooled)
        refused(b"16-byte aligned", out={"next_obs": ptr(nxt) + 8}, pooled=pooled)
        refused(b"action 8-byte", out={"action": ptr(oa) + 4}, pooled=pooled)
        refused(b"discount must be 4-byte aligned", out={"discount": ptr(og) + 2}, pooled=pooled)
    for bad_m in (0, -1, 4):
        refused(b"M must be in [1, B]", t=tm(M=bad_m))
    refused(b"a NULL array in the terminal pool", t=tm(pool=None))
    refused(b"a NULL array in the terminal pool", t=tm(ref=None))
    refused(b"pool must be 16-byte aligned", t=tm(pool=ptr(pool) + 8))
    refused(b"ref 4-byte", t=tm(ref=ptr(ref) + 2))
    # nothing was written by any of the calls above
    for a in (h.frames, h.action, h.reward, h.done, h.age, pool, ref, idx, obs, nxt, oa, orw, od, og, os_):
        assert not a.view(np.uint8).any()


def test_ops_wrapper_rejects_host_tensors_and_bad_arguments():
    import torch

    from torchdriveenv_amd import ops

    z = torch.zeros
    rp, tm = _abi.TdeReplay(6, 4, 3, 64, 0, None, None, None, None, None), _abi.TdeTerminal(2, None, None)
    for t in (None, tm):
        for n_steps in (0, -3, 65):
            with pytest.raises(ValueError, match=r"n_steps must be in \[1, 64\]"):
                ops.nstep_sample(rp, t, "cuda:0", 0, 4, 2, n_steps, 0.99, {})
        for gamma in (-0.1, 1.01, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=r"gamma must be in \[0, 1\]"):
                ops.nstep_sample(rp, t, "cuda:0", 0, 4, 2, 3, gamma, {})
        with pytest.raises(ValueError, match="n must be >= 1"):
            ops.nstep_sample(rp, t, "cuda:0", 0, 4, 0, 3, 0.99, {})
        with pytest.raises(ValueError, match="observations must live on a HIP device"):
            ops.nstep_sample(rp, t, "cuda:0", 0, 4, 2, 3, 0.99, {"observations": z((2, 9, 64), dtype=torch.uint8)})


def test_sample_nstep_arguments_are_refused_without_a_gpu():
    import inspect

    import torch

    from torchdriveenv_amd.replay import NStepSamples, ReplayBuffer, ReplaySamples

    sig = inspect.signature(ReplayBuffer.sample_nstep).parameters
    assert list(sig) == ["self", "n", "n_steps", "gamma", "idx", "check"]
    assert sig["gamma"].default == 0.99 and sig["idx"].default is None and sig["check"].default is True
    assert NStepSamples._fields == ReplaySamples._fields + ("discounts", "steps")
    buf = ReplayBuffer.__new__(ReplayBuffer)                # a buffer in host memory: every refusal comes before the first device call
    buf.dev, buf.C, buf.B, buf.n_stack, buf.first, buf.count, buf.draws = torch.device("cpu"), 6, 3, 3, 1, 4, 5
    buf.age = torch.tensor([[0] * 3, [0, 1, 2], [1, 2, 3], [2, 0, 4], [3, 1, 5], [4, 2, 6]], dtype=torch.uint8)
    for n_steps in (0, -1, 65):
        with pytest.raises(ValueError, match=r"n_steps must be in \[1, 64\]"):
            buf.sample_nstep(4, n_steps)
    for gamma in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match=r"gamma must be in \[0, 1\]"):
            buf.sample_nstep(4, 3, gamma)
    for n in (0, -1, None):
        with pytest.raises(ValueError, match="n must be >= 1"):
            buf.sample_nstep(n, 3)
    with pytest.raises(ValueError, match=r"idx must hold 3 \(slot, env\) pairs"):
        buf.sample_nstep(3, 3, idx=[(1, 0), (2, 0)])
    # slot 0 is the open slot's successor, (1, 2) lacks its older frames (age 2 at off 0), env 3 and slot 6 do not exist
    for bad in ((0, 0), (1, 2), (2, 2), (5, 0), (2, 3), (6, 0), (-1, 0), (2, -1)):
        with pytest.raises(ValueError, match=r"not stored transitions with their whole frame stack in the ring \(valid_pairs\(\)\)"):
            buf.sample_nstep(None, 3, idx=[(1, 0), bad, (3, 1)])
    buf.count = 2
    with pytest.raises(ValueError, match="needs more than 2 stored steps, the buffer holds 2"):
        buf.sample_nstep(4, 3)
    buf.count = 0
    with pytest.raises(ValueError, match="holds no transition yet"):
        buf.sample_nstep(4, 3)
    assert buf.draws == 5                                   # a refused call draws nothing
    # .bootstrap and .terminal read the returned done byte as ReplaySamples does
    d = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    a, b = NStepSamples(None, None, None, d, None, None, None, None), ReplaySamples(None, None, None, d, None, None)
    assert torch.equal(a.bootstrap, b.bootstrap) and torch.equal(a.terminal, b.terminal)


# ---- the restatement against a brute-force composition ---------------------------------------------------------------------------------
def brute(ring, s, e, n_steps, gamma, terminal):
    """walk the done bits one step at a time from the stored pair (s, e); next_obs and done from the one-step restatements at (L, e)"""
    gamma = F(gamma)
    t, taken, R, g = s, 1, F(ring.reward[s, e]), gamma
    while not ring.done[t, e] & ENDED and taken < n_steps and int(ring.offset(t)) + 1 < ring.count:
        t = (t + 1) % ring.C
        R = F(R + F(g * ring.reward[t, e]))
        g = F(g * gamma)
        taken += 1
    last = N.one_step(ring, [(t, e)], terminal)
    return R, g, taken, last["next_observations"][0], last["dones"][0]


RINGS = [dict(n_stack=3, plane=16), dict(n_stack=1, plane=16), dict(n_stack=8, plane=16), dict(D=5)]


@pytest.mark.parametrize("shape", RINGS, ids=str)
@pytest.mark.parametrize("pool", (False, True))
def test_restatement_equals_the_brute_force_composition(shape, pool):
    ring = K.history_ring(pool=pool, **shape)
    assert (ring.first, ring.w, ring.count) == (6, 5, 11)
    pairs = ring.stored_pairs()
    one = N.one_step(ring.ref, pairs, pool)
    for n in K.N_STEPS:
        for gamma in K.GAMMAS:
            got = N.gather(ring.ref, pairs, n, gamma)
            for k in ("observations", "actions", "indices"):
                assert np.array_equal(got[k], one[k])
            for i, (s, e) in enumerate(pairs):
                R, g, m, nxt, d = brute(ring.ref, int(s), int(e), n, gamma, pool)
                assert got["rewards"][i].view(np.uint32) == R.view(np.uint32) and got["discounts"][i].view(np.uint32) == g.view(np.uint32)
                assert got["steps"][i] == m and got["dones"][i] == d and np.array_equal(got["next_observations"][i], nxt)
                assert g == F(gamma) ** m or gamma not in (0.0, 0.5, 1.0)       # exact where the powers are
        if n == 1:
            for k in one:
                assert np.array_equal(got[k], one[k]), k
    # pairs that are no stored transition: zeros everywhere, indices echoed
    bad = [(5, 0), (-1, 0), (12, 1), (6, 5), (6, -1)]
    got = N.gather(ring.ref, bad, 5, 0.99)
    assert np.array_equal(got["indices"], np.array(bad, np.int32))
    assert not any(got[k].any() for k in got if k != "indices")


# ---- the case table means something ---------------------------------------------------------------------------------------------------------
def test_case_table_contains_every_stop_reason():
    for pool in (False, True):
        ring = K.history_ring(plane=16, n_stack=3, pool=pool)
        seen, ms = set(), {n: set() for n in K.N_STEPS}
        for n in K.N_STEPS:
            for s, e in ring.stored_pairs():
                r, m = K.reasons(ring.ref, int(s), int(e), n)
                seen |= r
                ms[n].add(m)
        pooled = {"terminated_with_row", "overflowed", "truncated_cut_with_row"}
        assert seen == set(K.REASONS) - (set() if pool else pooled), sorted(set(K.REASONS) - seen)
        assert ms[1] == {1} and ms[2] == {1, 2} and ms[5] == {1, 2, 3, 4, 5} and max(ms[64]) == ring.count
    # an obs stack and a next stack that overlap (m < n_stack) and that do not, at every stack depth above 1
    for ns, _ in K.PLANES:
        if ns > 1:
            assert any(m < ns for n in K.N_STEPS for m in ms[n]) and any(m >= ns for n in K.N_STEPS for m in ms[n])
    assert sorted({p // 16 for _, p in K.PLANES}) == [1, 144, 256] and sorted({ns for ns, _ in K.PLANES}) == [1, 3, 8]
    assert K.ROWS == (5, 65) and 3 <= K.B <= 5 and K.C == 12


def test_case_table_age_saturates_along_the_look_ahead():
    ring = K.age_ring(D=5)
    slots = [(ring.first + off) % ring.C for off in range(ring.count)]
    assert ring.count == ring.C - 1 and all(ring.ref.age[s, 0] == 255 for s in slots + [ring.w])
    assert ring.ref.age[ring.w, 1] == 2 and N.look_ahead(ring.ref, slots[0], 1, 64) == ring.count - 2


def test_long_ring_reaches_the_full_width_of_the_look_ahead():
    """what tests/test_gpu_nstep.py::test_the_look_ahead_at_its_full_width runs: n_steps = 64 over the long ring of tests/sequence_cases.py"""
    from tests import sequence_cases as S

    for pool in (False, True):
        ring = S.long_ring(pool=pool)
        assert (ring.C, ring.B, ring.n_stack, ring.plane) == (300, 2, 2, 16) and (ring.first, ring.count) == (0, 280)
        pairs, ref = S.long_pairs(), ring.ref
        got = N.gather(ref, pairs, 64, 0.99, terminal=pool)
        assert got["steps"].tolist() == [64, 64, 64, 64, 64, 64, 63, 64, 1, 64, 64, 64, 64, 64, 1, 64, 64, 64, 64, 64, 50, 64, 49, 64, 52, 64, 1, 1]
        m = {tuple(p): int(k) for p, k in zip(pairs.tolist(), got["steps"])}
        last = lambda s: int(ref.done[(s + m[(s, 0)] - 1) % ref.C, 0])
        assert m[(10, 0)] == 64 and last(10) & 3 == 1                              # terminated at the last step: the ending is in lane 63
        assert m[(75, 0)] == 64 and last(75) & 3 == 2                              # truncated at the last step
        assert m[(9, 0)] == 64 and not last(9) & ENDED and ref.done[9 + 64, 0] & ENDED         # no ending, and one a step beyond
        assert m[(11, 0)] == 63 and last(11) & ENDED
        assert m[(216, 1)] == 64 == ref.count - int(ref.offset(216))              # the stored range ends with the look-ahead
        assert m[(279, 0)] == m[(279, 1)] == 1 and int(ref.offset(279)) == ref.count - 1       # the newest stored step


def test_case_table_tells_the_stated_order_from_a_fused_multiply_add():
    ring = K.history_ring(D=5)
    differ = 0
    for s, e in ring.stored_pairs():
        m = N.look_ahead(ring.ref, int(s), int(e), 5)
        rewards = [ring.ref.reward[(s + k) % ring.C, e] for k in range(m)]
        (R, g), (Rf, gf) = N.reward_sum(rewards, 0.99), K.fused_sum(rewards, 0.99)
        assert g == gf
        differ += int(R.view(np.uint32) != Rf.view(np.uint32))
    assert differ >= 1
