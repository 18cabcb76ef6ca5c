"""The case tables of tests/ring_util.py are not vacuous: conditions on the INPUTS of tests/test_gpu_ring_edges.py, checked on the numpy
restatements alone (HandRing without a device), so that a later edit to a table cannot quietly turn a GPU case into a no-op."""
import itertools

import numpy as np
import pytest

from tests import onpolicy_ref as O
from tests import replay_ref as R
from tests import ring_util as U
from tests.ring_util import HandRing

ENDED = R.ENDED


# ---- 1. tde_gae --------------------------------------------------------------------------------------------------------------------------
def test_the_gae_shapes_are_the_required_ones():
    shapes = set(U.GAE_SHAPES)
    assert {(T, 65) for T in (1, 15, 16, 17, 31, 32, 33, 130)} <= shapes and {(33, B) for B in (1, 63, 64, 65, 130)} <= shapes
    assert (130, 130) in shapes and len(shapes) == len(U.GAE_SHAPES)
    assert U.GAE_SETTINGS == ((0.99, 0.95), (1.0, 1.0), (0.99, 0.0), (0.0, 0.95), (0.5, 1.0))


@pytest.mark.parametrize("T,B", U.GAE_SHAPES)
def test_gae_done_patterns_end_on_both_sides_of_every_block_edge(T, B):
    pattern = U.GAE_DONE[T, B]
    done = np.zeros((T, B), np.uint8)
    for t, e, byte in pattern:
        assert 0 <= t < T and 0 <= e < B and byte in U.GAE_BYTES and done[t, e] == 0
        done[t, e] = byte
    ends = (done & ENDED) != 0
    assert ends[0].any() and ends[T - 1].any()
    # block k of the kernel holds the steps with T - 1 - t in [16 k, 16 k + 15]: an ending in the last step of one block and in the
    # first step of the next, for the edges the distances name
    edges = [k for k in (U.GAE_BLOCK, 2 * U.GAE_BLOCK) if T - 1 - k >= 0]
    assert len(edges) == min(2, (T - 1) // U.GAE_BLOCK)
    for k in edges:
        assert {k - 1, k} <= set(U.GAE_EDGE_DISTANCES)
        assert ends[T - 1 - (k - 1)].any() and ends[T - 1 - k].any(), k
        # ... and an env that carries `last` and the next value across that edge, with endings elsewhere or nowhere
        assert (~ends[T - 1 - k] & ~ends[T - 1 - (k - 1)]).any() or B < 2
    for d in U.GAE_EDGE_DISTANCES:
        assert T - 1 - d < 0 or ends[T - 1 - d].any(), d
    if B >= 3:
        assert (~ends).all(0).any() and ends.all(0).any()   # an env without an ending, an env that ends at every step
        assert {int(b) for b in done[ends]} == set(U.GAE_BYTES) or T == 1


@pytest.mark.parametrize("T,B", U.GAE_SHAPES)
def test_gae_positions_are_where_they_claim_and_the_settings_differ(T, B):
    names = [p[0] for p in U.GAE_POSITIONS[T]]
    assert len(names) >= 3 and names[:2] == ["base0", "lead"] and (T == 1 or {"wrap_top", "wrap_mid"} <= set(names))
    assert ("wrap_edge" in names) == (T - 1 - U.GAE_BLOCK >= 1)
    for name, C, pushes, t_wrap in U.GAE_POSITIONS[T]:
        ring = U.gae_ring(T, B, C)
        values, last = U.gae_fill(ring, T, pushes, U.GAE_DONE[T, B])
        first, w, count = ring.check_state()
        s = O.slots(first, count, T, C)
        if name == "base0":
            assert first == 0 and count == T and s[0] == 0
        elif name == "lead":
            assert count > T and s[0] > 0 and (np.diff(s) == 1).all()
        elif name == "last_slot":
            assert T == 1 and s[0] == C - 1 and first != 0
        else:
            assert 1 <= t_wrap <= T - 1 and s[t_wrap] == 0 and s[t_wrap - 1] == C - 1 and count > T and first != 0
            at_edge = (T - 1 - t_wrap) % U.GAE_BLOCK == 0
            assert at_edge == (name in ("wrap_top", "wrap_edge")) and (name != "wrap_edge" or T - 1 - t_wrap == U.GAE_BLOCK)
        # the rollout's done bytes are the pattern, under random infraction bits
        done = ring.ref.done[s]
        want = np.zeros((T, B), np.uint8)
        for t, e, byte in U.GAE_DONE[T, B]:
            want[t, e] = byte
        assert np.array_equal(done & ENDED, want) and ((done >> 2) & 7).any() and ((done >> 2) & 7 == 0).any()
        assert (done[(done & ENDED) == 0] != 0).any()        # infraction bits alone, which end nothing
        advs = []
        for gamma, lam in U.GAE_SETTINGS:
            adv, ret = O.ring_gae(ring.ref, T, values, last, gamma, lam)
            assert np.isfinite(adv).all() and np.isfinite(ret).all()
            advs.append(adv)
        for a, b in itertools.combinations(range(len(advs)), 2):
            # (one step has no `last` to carry: lambda cannot show, gamma must)
            same_gamma = U.GAE_SETTINGS[a][0] == U.GAE_SETTINGS[b][0]
            assert np.array_equal(advs[a], advs[b]) == (T == 1 and same_gamma), (U.GAE_SETTINGS[a], U.GAE_SETTINGS[b])


# ---- 2. the gathers ------------------------------------------------------------------------------------------------------------------------
def test_the_gather_shapes_are_the_required_ones():
    assert set(U.GATHER_SHAPES) == {(8, 16), (8, 4096), (2, 2304), (1, 16), (3, 4080)} and U.GATHER_B == 3 and U.GATHER_M == 2
    assert [p // 16 for _, p in U.GATHER_SHAPES] == [1, 256, 144, 1, 255]
    assert U.AGE_RING == dict(n_stack=8, plane=16, C=10, B=2) and U.AGE_STEPS == {254: 254, 255: 255, 256: 255, 260: 255}


@pytest.mark.parametrize("ns", sorted(U.GATHER_HISTORIES))
def test_gather_histories_meet_every_blanking_combination(ns):
    ring = HandRing(ns + 3, U.GATHER_B, ns, plane=16, M=U.GATHER_M, seed=ns)
    seen, frames = set(), {True: 0, False: 0}
    kinds = dict(kept=0, overflowed=0, cut_kept=0, cut_only=0, open=0)
    for _ in U.play(ring, U.GATHER_HISTORIES[ns]):
        pairs = ring.stored_pairs()
        assert len(pairs) == ring.count * ring.B
        seen |= U.blanking(ring, pairs)
        g = ring.ref.gather(pairs)
        for k in ("observations", "next_observations"):
            blank = ~g[k].reshape(len(pairs), ns, -1).any(2)
            frames[True] += int(blank.sum())
            frames[False] += int((~blank).sum())
        d = g["dones"]
        fin, has, cut = (d & 3) != 0, (d & U.HAS) != 0, (d & U.CUT) != 0
        kinds["kept"] += int((has & ~cut).sum())
        kinds["overflowed"] += int((fin & ~has).sum())
        kinds["cut_kept"] += int((has & cut).sum())
        kinds["cut_only"] += int((cut & ~fin).sum())
        kinds["open"] += int(((d & ENDED) == 0).sum())
    # wavefront k shows the frame d = ns - 1 - k slots back.  d = 0 is the transition's own slot: 0 <= age and 0 <= off always hold.
    # Every older frame meets all four combinations of (d <= age, d <= off)
    want = {(ns - 1, True, True)} | {(k, a, o) for k in range(ns - 1) for a in (False, True) for o in (False, True)}
    assert seen == want, sorted(want - seen)
    assert frames[True] and frames[False] and all(kinds.values()), (frames, kinds)
    assert ring.first != 0 and ring.count == ring.C - 1


def test_the_age_saturates_in_the_restatement():
    ring = HandRing(U.AGE_RING["C"], U.AGE_RING["B"], U.AGE_RING["n_stack"], plane=U.AGE_RING["plane"], M=1, seed=5)
    ring.begin(ring.rows())
    for p in range(1, max(U.AGE_STEPS) + 1):
        ring.step()
        if p in U.AGE_STEPS:
            assert (ring.ref.age[ring.w] == U.AGE_STEPS[p]).all()
    assert len(U.blanking(ring, ring.stored_pairs())) == 2 * U.AGE_RING["n_stack"] - 1      # (d <= 255 everywhere; d <= off or not)


# ---- 3. pairs that gather zeros ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.INVALID_RINGS))
@pytest.mark.parametrize("mode", list(U.INVALID_MODES))
def test_invalid_pairs_are_invalid_and_the_others_valid(mode, name):
    case = U.INVALID_RINGS[name]
    ring = U.invalid_ring(mode, name)
    first, w, count = ring.check_state()
    C, B = ring.C, ring.B
    assert (first, w, count) == case["state"] and first != 0 and (count == C - 1) == (name == "full")
    must = [(-1, 0), (C, 0), (0, -1), (0, B), (U.INT32_MIN, 0), (0, U.INT32_MAX), (w, 1)]
    assert all(p in case["invalid"] for p in must) and len(case["invalid"]) == len(case["valid"])
    if name == "short":
        assert any(0 <= s < C and 0 <= e < B and s != w and int(ring.ref.offset(s)) >= count for s, e in case["invalid"])
    stored = {tuple(p) for p in ring.stored_pairs().tolist()}
    assert all(p not in stored for p in case["invalid"]) and all(p in stored for p in case["valid"])
    pairs = U.interleaved(case)
    assert len(pairs) == 2 * len(case["invalid"]) >= max(U.INVALID_N) and U.INVALID_N == (1, 5, 9)
    for terminal in (False, True):
        g = ring.want_sample(pairs, terminal)
        assert np.array_equal(g["indices"], np.array(pairs, np.int32))
        for i, p in enumerate(pairs):
            zero = not any(U.bits(g[k][i]).any() for k in U.FIELDS[:5])
            assert zero == (i % 2 == 0), p
            # a stored transition is told from the zeros by every output on its own
            assert i % 2 == 0 or (g["dones"][i] != 0 and g["rewards"][i] != 0 and g["observations"][i].any() and g["actions"][i].all())
    d = ring.want_sample(pairs, True)["dones"]
    assert ((d & U.HAS) != 0).any() and ((ring.ref.done[:, :] & ENDED) == 0).any()


# ---- 4. the draw ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.DRAW_CASES))
def test_draw_cases_are_the_corners_they_claim(name):
    ring = U.draw_ring(name)
    first, w, count = ring.check_state()
    assert U.DRAWS == (0, 1, 2**32, 2**32 + 1) and U.DRAW_N == 257
    lists = [ring.ref.draw(U.DRAW_SEED, d, U.DRAW_N) for d in U.DRAWS]
    assert len({a.tobytes() for a in lists}) == 4
    for idx in lists:
        assert {tuple(p) for p in idx.tolist()} <= {tuple(p) for p in ring.stored_pairs().tolist()}
    slots = {int(s) for idx in lists for s in idx[:, 0]}
    if name == "one_slot":
        assert count - ring.ref.skip == 1 and slots == {(first + ring.ref.skip) % ring.C}
        assert {int(e) for e in lists[0][:, 1]} == set(range(ring.B))
    elif name == "one_env":
        assert ring.B == 1 and len(slots) == count
    else:
        assert first == ring.C - 1 and count == ring.C - 1 and len(slots) == count - ring.ref.skip and 0 in slots
    assert U.DRAW_SEED >> 32


# ---- 5, 6. the seam and the pack ---------------------------------------------------------------------------------------------------------
def test_seam_cases_cover_the_copy_loops_and_the_workgroup_tail():
    rows = {(c["D"], c["B"]) for c in U.SEAM_CASES if c["D"]}
    assert rows == {(D, B) for D in (1, 5, 64, 65) for B in (1, 5)} and U.SEAM_C == 4
    planes = [c for c in U.SEAM_CASES if c["plane"]]
    assert any(c["layout"] == ((c["n_stack"] - 1) * c["plane"], c["n_stack"] * c["plane"]) and c["n_stack"] > 1 for c in planes)
    assert {c["B"] for c in planes} == {1, 5}
    for c in U.SEAM_CASES:
        row = c["plane"] or 4 * c["D"]
        off, stride = c["layout"]
        assert off > 0 and stride > row and off % (16 if c["plane"] else 4) == 0 and stride % (16 if c["plane"] else 4) == 0
        ring = HandRing(U.SEAM_C, c["B"], c["n_stack"], plane=c["plane"], D=c["D"])
        at_seam, empty, wraps = 0, 0, 0
        for op, *arg in U.seam_script(c["B"]):
            if op == "begin":
                before = ring.ref.done.copy()
                ring.begin(ring.rows(), arg[0])
                changed = np.argwhere(ring.ref.done != before)
                if arg[0] is not None:
                    assert {(int(s), int(e)) for s, e in changed} <= {((ring.w - 1) % ring.C, e) for e in range(c["B"]) if arg[0][e]}
                    at_seam += int(ring.w == 0 and len(changed) > 0 and (changed[:, 0] == ring.C - 1).all())
                    empty += int(not any(arg[0]))
            else:
                ring.step()
                wraps += int(ring.w == 0)
        assert at_seam >= 1 and empty >= 1 and wraps >= 3


def test_pack_colours_hold_the_palette_its_neighbours_and_the_extremes():
    cols = {tuple(int(v) for v in c) for c in U.PACK_COLOURS}
    pal = [tuple(c) for c in R.PAL.tolist()]
    assert set(pal) <= cols and (0, 0, 0) in cols and (255, 255, 255) in cols and len(cols) == len(U.PACK_COLOURS)
    for c in pal:
        for ch in range(3):
            for step in (-1, 1):
                if 0 <= c[ch] + step <= 255:
                    assert tuple(c[i] + (step if i == ch else 0) for i in range(3)) in cols
    lay = R.layers_of_rgb(U.PACK_COLOURS.T[None])[0]        # [1, 3, K] -> [K]
    assert set(lay.tolist()) == set(range(8))
    others = np.array([tuple(c) not in pal for c in U.PACK_COLOURS.tolist()])
    assert others.sum() >= 2 * 8 and (lay[others] == U.BLANK).all() and (lay[~others] == [pal.index(tuple(c)) for c in U.PACK_COLOURS[~others].tolist()]).all()
    assert set(U.PACK_CASES) == {(B, p) for B in (1, 5) for p in (16, 2304, 4096)}
