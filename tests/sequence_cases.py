"""The case table of the sequence sample (include/tde_sequence.h): the scripted history of tests/nstep_cases.py - its endings, cuts and
wrap, C = 12, B = 5, M = 2 - played into hand-filled rings (tests/ring_util.HandRing) of every shape, the name of the reason each window
stops for and of what it contains, and a second, long ring for the length search's rounds of 64 steps.  tests/test_gpu_sequence.py runs
them on the GPU; tests/test_sequence_cpu.py plays the same histories into the restatement alone and holds them to the conditions that
make them mean something: every reason is there."""
import numpy as np

from tests import nstep_cases as K
from tests import nstep_ref as N
from tests.replay_ref import ENDED
from tests.ring_util import CUT, HandRing

C, B, M = K.C, K.B, K.M
T_STEPS = (1, 2, 5, 11, 17)                                 # 17 exceeds count = 11
PLANES = ((1, 16), (3, 2304), (8, 4096), (3, 4096), (8, 16))
ROWS = (5, 65)
REASONS = ("ends_at_first_step", "ends_inside", "ends_at_last_step", "no_ending", "ends_just_beyond", "stored_range_ends", "wraps",
           "only_cut", "terminated_with_row", "overflowed", "truncated_cut_with_row", "starts_young", "before_first")
POOLED = {"terminated_with_row", "overflowed", "truncated_cut_with_row"}
# pairs that are no stored transition of the history ring (first = 6, w = 5: slot 5 is the open one)
INVALID = ((5, 0), (-1, 0), (12, 1), (6, 5), (6, -1), (-2**31, 0), (0, 2**31 - 1))

history_ring = K.history_ring
age_ring = K.age_ring


def reasons(ref, s, e, T):
    """(names, m): what the window of T steps from the stored pair (s, e) of the restatement `ref` meets"""
    off, done, ns = int(ref.offset(s)), ref.done, ref.n_stack
    m = N.look_ahead(ref, s, e, T)
    last = (s + m - 1) % ref.C
    d = int(done[last, e])
    out = set()
    if d & ENDED:
        out |= {"ends_at_first_step"} if m == 1 else set()
        out |= {"ends_inside"} if 1 < m < T else set()
        out |= {"ends_at_last_step"} if m == T else set()
    elif m == T:
        out.add("no_ending")
        if off + T < ref.count and done[(s + T) % ref.C, e] & ENDED:
            out.add("ends_just_beyond")
    else:
        assert m == ref.count - off < T
        out.add("stored_range_ends")
    if s + m - 1 >= ref.C:
        out.add("wraps")
    if d & ENDED == CUT:
        out.add("only_cut")
    has_row = hasattr(ref, "ref") and ref.ref[last, e] >= 0
    if d & 3 == 1 and has_row:
        out.add("terminated_with_row")
    if d & 3 and hasattr(ref, "ref") and ref.ref[last, e] < 0:
        out.add("overflowed")
    if d & 3 == 2 and d & CUT and has_row:
        out.add("truncated_cut_with_row")
    if int(ref.age[s, e]) < ns - 1:
        out.add("starts_young")
    if off < ns - 1:
        out.add("before_first")
    return out, m


# ---- the length search beyond one round of 64 steps ---------------------------------------------------------------------------------------
LONG_C, LONG_B, LONG_PUSHES = 300, 2, 280                   # first = 0, count = 280: step t lies in slot t
LONG_T = (64, 65, 130, 256)
# env 0 ends at t = 73, 138 and 267: from the starts 10, 74 and 139 these are steps 64, 65 and 129 of a window; env 1 never ends
LONG_ENDINGS = {73: 1, 138: 2, 267: 1}
LONG_LENGTHS = {10: 64, 74: 65, 139: 129}
LONG_STARTS = (1, 9, 10, 11, 73, 74, 75, 138, 139, 140, 24, 25, 216, 279)


def long_ring(pool=True, dev=None):
    ring = HandRing(LONG_C, LONG_B, 2, plane=16, M=1 if pool else 0, dev=dev, seed=300)
    ring.begin(ring.rows())
    for t in range(LONG_PUSHES):
        ring.step(np.array([LONG_ENDINGS.get(t, 0), 0], np.uint8))
    return ring


def long_pairs():
    return np.array([(s, e) for s in LONG_STARTS for e in range(LONG_B)], np.int32)
