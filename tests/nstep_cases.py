"""The case table of the n-step sample (include/tde_nstep.h): one scripted history of endings, cuts and wraps that
tests/test_gpu_nstep.py plays into hand-filled rings (tests/ring_util.HandRing) of every shape, and the name of the reason each look-ahead
stops for.  tests/test_nstep_cpu.py plays the same history into the restatement alone and holds it to the conditions that make it mean
something: every reason is there."""
import numpy as np

from tests import nstep_ref as N
from tests.replay_ref import ENDED
from tests.ring_util import CUT, HandRing

C, B, M = 12, 5, 2
N_STEPS = (1, 2, 5, 64)
GAMMAS = (0.0, 0.5, 0.99, 1.0)
# (n_stack, plane bytes): planes of 1, 144 and 256 sixteen-byte chunks; rows of 5 and 65 floats
PLANES = ((1, 16), (3, 2304), (8, 4096), (3, 4096), (8, 16))
ROWS = (5, 65)
PUSHES = 17                                                 # first = 6, w = 5, count = 11: the stored steps are t = 6 .. 16, slot t % 12
# done bits of push t, env e (everything else 0); bits 2-4 are random infraction bits on top
ENDINGS = {(2, 0): 1,                                       # env 0 ends before the stored range and never again
           (9, 1): 1, (9, 3): 1, (9, 4): 2,                 # three envs end at t = 9: rows 0 and 1, env 4 overflows a pool of two
           (13, 1): 2,                                      # env 1 is truncated and then reset by the caller: cut with a row
           (14, 2): 1, (15, 4): 2}
CUTS = {10: (0, 0, 1, 0, 0), 13: (0, 1, 0, 0, 0)}           # begin(mask) after push t: env 2 is only cut at t = 10
REASONS = ("ends_at_s", "ends_at_s+1", "ends_at_last_looked", "ends_just_beyond", "no_ending", "stored_range_ends", "wraps", "only_cut",
           "terminated_with_row", "overflowed", "truncated_cut_with_row")


def history_ring(n_stack=1, plane=0, D=0, pool=True, dev=None):
    ring = HandRing(C, B, n_stack, plane=plane, D=D, M=M if pool else 0, dev=dev, seed=1000 * n_stack + plane + D)
    ring.begin(ring.rows())
    for t in range(PUSHES):
        db = (ring.rng.integers(0, 8, B) << 2).astype(np.uint8)
        for e in range(B):
            db[e] |= ENDINGS.get((t, e), 0)
        ring.step(db)
        if t in CUTS:
            ring.begin(ring.rows(), np.array(CUTS[t], np.uint8))
    return ring


def reasons(ref, s, e, n):
    """the names of what the look-ahead of n steps from the stored pair (s, e) of the restatement `ref` meets"""
    off, done = int(ref.offset(s)), ref.done
    m = N.look_ahead(ref, s, e, n)
    last = (s + m - 1) % ref.C
    d = int(done[last, e])
    out = set()
    if d & ENDED:
        out |= {"ends_at_s"} if m == 1 else set()
        out |= {"ends_at_s+1"} if m == 2 else set()
        out |= {"ends_at_last_looked"} if m == n else set()
    elif m == n:
        out.add("no_ending")
        if off + n < ref.count and done[(s + n) % ref.C, e] & ENDED:
            out.add("ends_just_beyond")
    else:
        assert m == ref.count - off < n
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
    return out, m


# ---- a saturated age along the look-ahead -----------------------------------------------------------------------------------------------
AGE_PUSHES = 270                                            # env 0 never ends: its age is 255 in every stored slot; env 1 ends at the end


def age_ring(n_stack=1, plane=0, D=0, pool=True, dev=None):
    ring = HandRing(C, 3, n_stack, plane=plane, D=D, M=1 if pool else 0, dev=dev, seed=77)
    ring.begin(ring.rows())
    for t in range(AGE_PUSHES):
        ring.step(np.array([0, 1 if t == AGE_PUSHES - 3 else 0, 0], np.uint8))
    return ring


# ---- rewards whose sum tells a fused multiply-add from the stated order -----------------------------------------------------------------
def fused_sum(rewards, gamma):
    """reward_sum with R + g * r as ONE rounding (through float64: the product of two float32 is exact there)"""
    gamma = np.float32(gamma)
    R, g = np.float32(rewards[0]), gamma
    for r in rewards[1:]:
        R = np.float32(np.float64(R) + np.float64(g) * np.float64(np.float32(r)))
        g = np.float32(g * gamma)
    return R, g
