"""The ring kernels at their edges, through the C-ABI alone (include/tde_replay.h, tde_onpolicy.h, tde_terminal.h): rings filled by hand
(tests/ring_util.HandRing) at the shapes no env produces - tde_gae past one 16-step block, the gathers at the stack limit, at planes whose
chunk count is no multiple of a wavefront and at a saturated age, the pairs that must gather zeros, the draw at its corners, begin and
push at the ring's seam, and tde_replay_pack's blank branch and strides.  Nothing here has a tolerance: every byte is held to the numpy
restatements (tests/replay_ref.py, onpolicy_ref.py, terminal_ref.py).  tests/test_ring_edges_cpu.py holds the case tables to the
conditions that make these cases mean something."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import onpolicy_ref as O
from tests import replay_ref as R
from tests import ring_util as U
from tests.ring_util import FILL, HandRing, bits, guarded, guards_ok
from torchdriveenv_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- 1. tde_gae across its blocks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B", U.GAE_SHAPES)
def test_gae_across_blocks_and_ring_positions(T, B):
    extra = 2                                               # rows of advantages / returns beyond T, which the call may not touch
    for name, C, pushes, _ in U.GAE_POSITIONS[T]:
        ring = U.gae_ring(T, B, C, DEV)
        values, last = U.gae_fill(ring, T, pushes, U.GAE_DONE[T, B])
        first, w, count = ring.check_state()
        tv, tl = up(values), up(last)
        for gamma, lam in U.GAE_SETTINGS:
            want_adv, want_ret = O.ring_gae(ring.ref, T, values, last, gamma, lam)
            got = []
            for rep in range(2):
                (wa, adv), (wr, ret) = guarded((T + extra, B), F32, DEV), guarded((T + extra, B), F32, DEV)
                ops.gae(ring.rp, DEV, first, count, T, tv, tl, gamma, lam, adv[:T], ret[:T])
                for whole, t, want in ((wa, adv, want_adv), (wr, ret, want_ret)):
                    assert np.array_equal(bits(t[:T].cpu().numpy()), bits(want)), (name, gamma, lam)
                    assert bool((t[T:] == FILL[F32]).all()) and guards_ok(whole, t), (name, gamma, lam)
                got.append((adv[:T].clone(), ret[:T].clone()))
            assert torch.equal(got[0][0].view(torch.int32), got[1][0].view(torch.int32))
            assert torch.equal(got[0][1].view(torch.int32), got[1][1].view(torch.int32))
        # the call reads: values, last_values and the ring are what they were
        assert np.array_equal(bits(tv.cpu().numpy()), bits(values)) and np.array_equal(bits(tl.cpu().numpy()), bits(last)), name
        ring.check_state()


# ---- 2. the gathers at the stack limit, at odd plane sizes, at a saturated age ---------------------------------------------------------
def check_onpolicy_gather(ring, T):
    """tde_onpolicy_gather of every sample of the newest T steps, and of indices outside them, against onpolicy_ref.gather"""
    B, rng = ring.B, np.random.default_rng(T)
    idx = np.concatenate([[-1], rng.permutation(T * B), [T * B, U.INT32_MAX, U.INT32_MIN]]).astype(np.int32)
    side = [rng.standard_normal((T, B)).astype(np.float32) for _ in range(4)]
    n = len(idx)
    spec = {"observations": ((n, 3 * ring.n_stack, ring.plane), torch.uint8), "actions": ((n, 2), F32)}
    spec.update({k: ((n,), F32) for k in ("old_values", "old_log_prob", "advantages", "returns")})
    whole, out = {}, {}
    for k, (shape, dt) in spec.items():
        whole[k], out[k] = guarded(shape, dt, DEV)
    ops.onpolicy_gather(ring.rp, DEV, ring.first, ring.count, T, up(idx), *[up(a) for a in side], out)
    want = O.gather(ring.ref, T, idx, *side)
    for k in spec:
        g = out[k].cpu().numpy()
        assert g.shape == want[k].shape and np.array_equal(bits(g), bits(want[k])), k
        assert guards_ok(whole[k], out[k]), k


@pytest.mark.parametrize("ns,plane", U.GATHER_SHAPES)
def test_gathers_at_the_stack_limit_and_odd_planes(ns, plane):
    ring = HandRing(ns + 3, U.GATHER_B, ns, plane=plane, M=U.GATHER_M, dev=DEV, seed=ns * 10000 + plane)
    n_has = n_cut_has = n_over = 0
    for _ in U.play(ring, U.GATHER_HISTORIES[ns]):
        ring.check_state()
        pairs = ring.stored_pairs()
        ring.check_sample(pairs)
        got, _ = ring.check_sample(pairs, terminal=True)
        d = got["dones"]
        n_has += int(((d & U.HAS) != 0).sum())
        n_cut_has += int(((d & (U.HAS | U.CUT)) == (U.HAS | U.CUT)).sum())
        n_over += int((((d & 3) != 0) & ((d & U.HAS) == 0)).sum())
        for T in sorted({1, ring.count}):
            check_onpolicy_gather(ring, T)
    assert n_has and n_cut_has and n_over


def test_gathers_at_a_saturated_age():
    ring = HandRing(U.AGE_RING["C"], U.AGE_RING["B"], U.AGE_RING["n_stack"], plane=U.AGE_RING["plane"], M=1, dev=DEV, seed=5)
    ring.begin(ring.rows())
    for p in range(1, max(U.AGE_STEPS) + 1):
        ring.step()
        if p in U.AGE_STEPS:
            ring.check_state()
            assert (ring.t["age"][ring.w].cpu().numpy() == U.AGE_STEPS[p]).all(), p
    for k in range(9):                                      # one ending, then eight steps of the new episodes beside the old ones
        ring.step(np.array([1, 0] if k == 0 else [0, 0], np.uint8))
        ring.check_state()
        pairs = ring.stored_pairs()
        ring.check_sample(pairs)
        ring.check_sample(pairs, terminal=True)
        check_onpolicy_gather(ring, ring.count)
    assert ring.ref.age[ring.w].tolist() == [8, 255]


# ---- 3. pairs the kernel must answer with zeros ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.INVALID_RINGS))
@pytest.mark.parametrize("mode", list(U.INVALID_MODES))
def test_invalid_pairs_gather_zeros(mode, name):
    case = U.INVALID_RINGS[name]
    ring = U.invalid_ring(mode, name, DEV)
    assert ring.check_state() == case["state"]
    pairs = U.interleaved(case)
    bad = np.arange(len(pairs)) % 2 == 0
    for n in sorted({len(pairs), *U.INVALID_N}):
        for terminal in (False, True):
            got, want = ring.check_sample(pairs[:n], terminal=terminal)
            # what the restatement says of these rows, said once more of the kernel's own output
            b = bad[:n]
            assert np.array_equal(got["indices"], np.array(pairs[:n], np.int32))
            for k in U.FIELDS[:5]:
                assert not bits(got[k][b]).any(), k
            for i in np.flatnonzero(~b):
                assert got["dones"][i] != 0 and got["rewards"][i] != 0 and got["observations"][i].any(), i


# ---- 4. the draw at its corners --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(U.DRAW_CASES))
def test_the_draw_at_its_corners(name):
    ring = U.draw_ring(name, DEV)
    ring.check_state()
    lists = []
    for draw in U.DRAWS:
        got, _ = ring.check_sample(n=U.DRAW_N, seed=U.DRAW_SEED, draw=draw)
        tgot, _ = ring.check_sample(n=U.DRAW_N, seed=U.DRAW_SEED, draw=draw, terminal=True)
        assert np.array_equal(got["indices"], tgot["indices"])
        off = (got["indices"][:, 0] - ring.first) % ring.C
        assert (off >= ring.ref.skip).all() and (off < ring.count).all() and (got["indices"][:, 1] < ring.B).all()
        if ring.count - ring.ref.skip == 1:
            assert (off == ring.ref.skip).all()
        lists.append(got["indices"].tobytes())
    assert len(set(lists)) == len(U.DRAWS)
    got, _ = ring.check_sample(n=1, seed=U.DRAW_SEED, draw=3)
    assert got["indices"].shape == (1, 2)


# ---- 5. begin and push at the ring's seam ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", U.SEAM_CASES, ids=lambda c: f"ns{c['n_stack']}-p{c['plane']}-D{c['D']}-B{c['B']}")
def test_begin_and_push_at_the_seam(case):
    B, layout = case["B"], case["layout"]
    ring = HandRing(U.SEAM_C, B, case["n_stack"], plane=case["plane"], D=case["D"], dev=DEV, seed=case["plane"] + case["D"] + B)
    cuts_at_seam = pushes = 0
    for op, *arg in U.seam_script(B):
        if op == "begin":
            mask = arg[0]
            before = ring.ref.done.copy()
            ring.begin(ring.rows(), mask, layout)
            if mask is not None:
                prev = (ring.w - 1) % ring.C
                want = before.copy()
                want[prev] |= np.where(np.array(mask) != 0, U.CUT, 0).astype(np.uint8)
                assert np.array_equal(ring.ref.done, want)              # the masked envs of the slot before w, and nothing else
                cuts_at_seam += int(ring.w == 0 and prev == ring.C - 1 and any(mask))
        else:
            db = ((ring.rng.uniform(size=B) < 0.3) * ring.rng.integers(1, 4, B)).astype(np.uint8) | (ring.rng.integers(0, 8, B) << 2).astype(np.uint8)
            ring.step(db, layout)
            pushes += 1
        ring.check_state()
    assert cuts_at_seam == 2 and pushes >= 3 * U.SEAM_C


# ---- 6. tde_replay_pack ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,plane", U.PACK_CASES)
def test_pack_blanks_what_is_no_palette_colour(B, plane):
    rng = np.random.default_rng(B * 10000 + plane)
    rgb = U.PACK_COLOURS[rng.integers(0, len(U.PACK_COLOURS), (B, plane))].transpose(0, 2, 1)       # [B, 3, plane]
    rgb_stride, planes_stride, off = 3 * plane + 32, plane + 48, 16
    src = np.full(off + B * rgb_stride, 0xEE, np.uint8)
    for e in range(B):
        src[off + e * rgb_stride:off + e * rgb_stride + 3 * plane] = rgb[e].reshape(-1)
    tsrc = up(src)
    whole, dst = guarded((B * planes_stride,), torch.uint8, DEV)
    scratch = torch.zeros(64, dtype=torch.uint8, device=DEV)
    rp = ops.replay_pack_struct(B, plane, scratch)
    _lib.check(_lib.load().tde_replay_pack(C.byref(rp), tsrc.data_ptr() + off, rgb_stride, dst.data_ptr(), planes_stride,
                                           _lib.current_stream(torch.device(DEV))), "tde_replay_pack")
    got = dst.cpu().numpy().reshape(B, planes_stride)
    want = R.layers_of_rgb(rgb)
    assert np.array_equal(got[:, :plane], want)
    assert (got[:, plane:] == FILL[torch.uint8]).all() and guards_ok(whole, dst)
    assert np.array_equal(tsrc.cpu().numpy(), src)
    # round trip at the strides of ops.replay_pack: palette-only planes -> colours -> the same planes
    codes = rng.integers(0, 8, (B, plane)).astype(np.uint8)
    whole, out = guarded((B, plane), torch.uint8, DEV)
    ops.replay_pack(rp, DEV, up(R.PAL[codes].transpose(0, 2, 1)), out)
    assert np.array_equal(out.cpu().numpy(), codes) and guards_ok(whole, out)
