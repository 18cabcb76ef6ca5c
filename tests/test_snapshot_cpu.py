"""CPU checks of tde_state_copy (include/tde_snapshot.h, torchdriveenv_amd/snapshot.py): the header's constants and struct (the header beside
the others, its symbols and the loader's refusals: tests/test_abi_families_cpu.py), every host-side refusal of the entry point (all before any launch: no GPU needed - the index rules of
TDE_SNAPSHOT_CHECK included, which a process without a device reads from host memory), the classification of every tde_state member, and
the numpy restatement (tests/snapshot_ref.py) against a brute force written here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import snapshot_ref as S
from tests.test_abi_families_cpu import COMPILERS, c_status
from torchdriveenv_amd import _abi
from torchdriveenv_amd.state import EnvState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tde_snapshot.h")


# ---- header, symbols, constants -----------------------------------------------------------------------------------------------------
def test_constants_and_struct_match_header(tmp_path):
    for cc, ext in COMPILERS:
        assert c_status(tmp_path, ["tde_snapshot.h"], "(f.n_stack - 1) | (TDE_SNAPSHOT_OUTPUTS - 1) | (TDE_SNAPSHOT_CHECK - 2) |"
                        " (TDE_SNAPSHOT_MAX_STACK - 8) | (sizeof(f) != 48) | (s.B - 1)", cc, ext,
                        decls="tde_snapshot_frames f; tde_state s; f.n_stack = TDE_SNAPSHOT_VERSION; s.B = TDE_SNAPSHOT_VERSION;") == 0
    assert (_abi.SNAPSHOT_OUTPUTS, _abi.SNAPSHOT_CHECK, _abi.SNAPSHOT_MAX_STACK) == (S.SNAPSHOT_OUTPUTS, S.SNAPSHOT_CHECK, 8) == (1, 2, 8)
    assert C.sizeof(_abi.TdeSnapshotFrames) == 48


# ---- every member of tde_state is classified ----------------------------------------------------------------------------------------
def test_every_state_member_is_in_exactly_one_group():
    """a member added to tde_state fails here until the header, the restatement and _abi say what tde_state_copy does with it"""
    for n in _abi.STATE_PTRS:
        assert S.group(n) in ("copied", "outputs", "invalidated")
    everything = S.COPIED_AGENT + S.COPIED_ENV + S.OUTPUTS + S.INVALIDATED
    assert sorted(everything) == sorted(_abi.STATE_PTRS) and len(set(everything)) == len(everything)
    assert sorted(_abi.SNAPSHOT_COPIED) == sorted(S.COPIED_AGENT + S.COPIED_ENV)
    assert sorted(_abi.SNAPSHOT_OUTPUT_ARRAYS) == sorted(S.OUTPUTS) and sorted(_abi.SNAPSHOT_INVALIDATED) == sorted(S.INVALIDATED)
    with pytest.raises(KeyError):
        S.group("a_member_of_tomorrow")
    # the header's own list, word for word
    text = open(HEADER).read()
    block = text[text.index("COPIED        per agent"):text.index("(B and A are sizes")]
    words = lambda a, b: re.findall(r"[a-z_0-9]+", re.sub(r"/?\*", " ", block[block.index(a) + len(a):block.index(b)]))     # noqa: E731
    assert words("per row:", "per env:") == S.COPIED_AGENT
    assert words("per env:", "OUTPUTS") == S.COPIED_ENV
    assert words("TDE_SNAPSHOT_OUTPUTS:", "INVALIDATED") == S.OUTPUTS
    assert re.findall(r"[a-z_0-9]+", block[block.index("rebuilds it:") + len("rebuilds it:"):]) == S.INVALIDATED
    # the struct itself: every pointer member of tde_state in tde_abi.h is a name of STATE_PTRS
    abi = open(os.path.join(ROOT, "include", "tde_abi.h")).read()
    struct = abi[abi.index("typedef struct tde_state {"):abi.index("} tde_state;")]
    struct = re.sub(r"/\*.*?\*/", "", struct, flags=re.S)
    members = [m for decl in re.findall(r"[\w ]+?\*([^;]+);", struct) for m in re.findall(r"\w+", decl)]
    assert sorted(members) == sorted(_abi.STATE_PTRS)
    # the EnvState options the Python surface mirrors
    assert set(_abi.state_shapes(2, 4)) == set(_abi.STATE_PTRS)


# ---- every host-side refusal, before any launch -------------------------------------------------------------------------------------
def _host_state(B, A, **kw):
    st = EnvState(B, A, with_cache=True, **kw)
    for a in st.arrays.values():
        if a is not None:
            a.reshape(-1).view(np.uint8)[...] = 0x5A
    return st


def test_entry_point_rejects_bad_arguments_without_a_launch():
    from torchdriveenv_amd import _lib

    L = _lib.load()
    A = 4
    src, dst = _host_state(5, A, with_slot_route=True), _host_state(7, A, with_slot_route=True)
    before = {n: a.copy() for n, a in dst.arrays.items() if a is not None}
    se, de = np.array([0, 1, 2], np.int32), np.array([3, 4, 5], np.int32)
    lay_s, lay_d = np.zeros((5, 3, 64), np.uint8), np.zeros((7, 3, 64), np.uint8)
    obs_s, obs_d = np.zeros((5, 9, 64), np.uint8), np.zeros((7, 9, 64), np.uint8)
    ptr = lambda a: a.ctypes.data                                         # noqa: E731

    def frames(**over):
        a = {**dict(src_layers=ptr(lay_s), dst_layers=ptr(lay_d), src_obs=ptr(obs_s), dst_obs=ptr(obs_d), n_stack=3, plane=64, src_phase=1,
                    dst_phase=2), **over}
        return _abi.TdeSnapshotFrames(*[a[k] for k, _ in _abi.TdeSnapshotFrames._fields_])

    def struct(st, **over):
        s = _abi.TdeState.from_buffer_copy(st.struct)
        for k, v in over.items():
            setattr(s, k, v)
        return s

    def refused(fragment, s=None, d=None, n=3, sp=ptr(se), dp=ptr(de), fr=None, flags=0, null=None):
        s, d = s or src.struct, d or dst.struct
        rc = L.tde_state_copy(None if null == "src" else C.byref(s), None if null == "dst" else C.byref(d), n, sp, dp,
                              None if fr is None else C.byref(fr), flags, None)
        err = L.tde_last_error()
        assert rc != 0 and fragment in err and err.startswith(b"tde_state_copy: "), (fragment, rc, err)

    refused(b"NULL argument", null="src")
    refused(b"NULL argument", null="dst")
    refused(b"same A", d=_host_state(7, 8).struct)
    for bad_a in (0, 3, 256, -4):
        refused(b"A must be a power of two", s=struct(src, A=bad_a), d=struct(dst, A=bad_a))
    refused(b"B must be >= 1", s=struct(src, B=0))
    refused(b"B must be >= 1", d=struct(dst, B=-1))
    for n in (-1, -(2**31)):
        refused(b"n must be >= 0", n=n)
    refused(b"unknown flag bits", flags=4)
    refused(b"unknown flag bits", flags=0x80000001)
    refused(b"must not be NULL", sp=None)
    refused(b"must not be NULL", dp=None)
    refused(b"4-byte aligned", sp=ptr(se) + 2)
    refused(b"4-byte aligned", dp=ptr(de) + 1)
    refused(b"src carries slot_route and dst does not", d=struct(dst, slot_route=None))
    refused(b"16-byte aligned, dst.act_cache 8-byte", d=struct(dst, slot_cache=ptr(dst["slot_cache"]) + 8))
    refused(b"16-byte aligned, dst.act_cache 8-byte", d=struct(dst, env_cache=ptr(dst["env_cache"]) + 4))
    refused(b"16-byte aligned, dst.act_cache 8-byte", d=struct(dst, act_cache=ptr(dst["act_cache"]) + 4))
    # frames
    for ns in (0, -1, 9):
        refused(b"n_stack must be in [1, 8]", fr=frames(n_stack=ns))
    for plane in (0, -16, 24, 65):
        refused(b"plane must be positive and a multiple of 16", fr=frames(plane=plane))
    refused(b"plane must be <= 2^24", fr=frames(plane=(1 << 24) + 16))
    for k in ("src_layers", "dst_layers", "src_obs", "dst_obs"):
        refused(b"for both sides or for neither", fr=frames(**{k: None}))
        refused(b"planes must be 16-byte aligned", fr=frames(**{k: ptr(obs_d) + 8}))
    for k in ("src_phase", "dst_phase"):
        for ph in (-1, 3, 100):
            refused(b"must be in [0, n_stack)", fr=frames(**{k: ph}))
    # TDE_SNAPSHOT_CHECK: ranges, duplicates, overlap within one state (no device here: the arrays are read as host memory)
    chk = _abi.SNAPSHOT_CHECK
    i32 = lambda *v: np.array(v, np.int32)                                # noqa: E731
    cases = [(i32(0, 5, 1), i32(0, 1, 2), False), (i32(0, -1, 1), i32(0, 1, 2), False), (i32(0, 1, 2), i32(0, 7, 2), False),
             (i32(0, 1, 2), i32(0, -1, 2), False), (i32(0, 1, 2), i32(6, 1, 6), False), (i32(0, 1, 2), i32(3, 4, 2), True),
             (i32(0, 0, 0), i32(1, 2, 0), True), (i32(0, 0, 0), i32(1, 2, 1), True), (i32(4, 4), i32(4, 3), True)]
    for a, b, same in cases:
        want = S.check_indices(a.tolist(), b.tolist(), 5, 5 if same else 7, same)
        assert want is not None
        refused(want.encode(), s=src.struct, d=src.struct if same else dst.struct, n=len(a), sp=ptr(a), dp=ptr(b), flags=chk)
        if same:                                             # a second struct over the same arrays is the same state
            refused(want.encode(), s=src.struct, d=struct(src), n=len(a), sp=ptr(a), dp=ptr(b), flags=chk | _abi.SNAPSHOT_OUTPUTS)
    assert S.check_indices([0, 0, 0], [1, 2, 3], 5, 5, True) is None and S.check_indices([0, 1, 2], [0, 1, 2], 5, 7, False) is None
    # n == 0 passes every check and launches nothing
    assert L.tde_state_copy(C.byref(src.struct), C.byref(dst.struct), 0, None, None, None, chk, None) == 0
    assert L.tde_state_copy(C.byref(src.struct), C.byref(dst.struct), 0, None, None, C.byref(frames()), 0, None) == 0
    # nothing was written by any of the calls above
    for n, a in dst.arrays.items():
        if a is not None:
            assert np.array_equal(a, before[n]), n
    assert not lay_d.any() and not obs_d.any()


def test_ops_wrapper_rejects_bad_arguments_without_a_gpu():
    from torchdriveenv_amd import ops

    a, b = EnvState(3, 4), EnvState(3, 4)
    with pytest.raises(ValueError, match="needs device states"):
        ops.state_copy(a, b, [0], [1])


def test_row_arguments_of_the_python_surface():
    from torchdriveenv_amd import snapshot as P

    assert P._as_rows([2, 0], 3) == [2, 0] and P._as_rows(1, 3) == [1] and P._as_rows(np.array([1, 2]), 3) == [1, 2]
    for bad, msg in (([], "is empty"), ([3], r"must be in \[0, 3\)"), ([-1], r"must be in \[0, 3\)"), ([1, 1], "names an env twice")):
        with pytest.raises(ValueError, match=msg):
            P._as_rows(bad, 3)
    import torch

    fr = torch.arange(2 * 5 * 3 * 2 * 4, dtype=torch.uint8).reshape(2, 5, 3, 2, 4)
    t = P.tile_frames(fr)                                   # 5 views: 3 rows x 2 columns, the last tile black
    assert tuple(t.shape) == (2, 3, 6, 8)
    for i in range(5):
        r, q = divmod(i, 2)
        assert torch.equal(t[:, :, 2 * r:2 * r + 2, 4 * q:4 * q + 4], fr[:, i])
    assert not t[:, :, 4:, 4:].any()


# ---- the restatement against a brute force ------------------------------------------------------------------------------------------
def _random_state(rng, B, A, **kw):
    st = EnvState(B, A, with_cache=True, **kw)
    for a in st.arrays.values():
        if a is not None:
            a.reshape(-1).view(np.uint8)[...] = rng.integers(0, 256, a.nbytes, dtype=np.uint8)
    return st


def brute(src, dst, sB, dB, A, src_env, dst_env, outputs):
    """element by element, array by array, from the header's words"""
    per_agent = ["x", "y", "psi", "v", "len", "wid", "lr", "vdes", "route_wp", "present", "collided", "offroad", "slot_route"]
    per_env = {"scn": 1, "steps": 1, "target_idx": 1, "reached": 1, "episode": 1, "action": 2, "obs": 8, "ep_return": 1}
    outs = {"reward": 1, "terminated": 1, "truncated": 1, "tl_violation": 1, "done_bits": 1, "info": 4, "info_reached": 1, "ep_final": 1,
            "ep_final_len": 1, "magnitudes": 4}
    for s, d in zip(src_env, dst_env):
        if s < 0 or s >= sB or d < 0 or d >= dB:
            continue
        for n in per_agent:
            if src.get(n) is not None and dst.get(n) is not None:
                for a in range(A):
                    dst[n].reshape(-1)[d * A + a] = src[n].reshape(-1)[s * A + a]
        for n, w in {**per_env, **(outs if outputs else {})}.items():
            if src.get(n) is not None and dst.get(n) is not None:
                for i in range(w):
                    dst[n].reshape(-1)[d * w + i] = src[n].reshape(-1)[s * w + i]
        if dst.get("slot_cache") is not None:
            for a in range(A):
                for i in range(8):
                    dst["slot_cache"].reshape(-1)[(d * A + a) * 8 + i] = 0
        if dst.get("env_cache") is not None:
            for i in range(8):
                dst["env_cache"].reshape(-1)[d * 8 + i] = 0
        if dst.get("act_cache") is not None:
            for a in range(A + 1):
                dst["act_cache"].reshape(-1)[(d * (A + 1) + a) * 2] = -1 if a == A else 0
                dst["act_cache"].reshape(-1)[(d * (A + 1) + a) * 2 + 1] = 0
    return dst


@pytest.mark.parametrize("A", (1, 4, 16))
@pytest.mark.parametrize("outputs", (False, True))
def test_restatement_equals_the_brute_force(A, outputs):
    rng = np.random.default_rng(A + outputs)
    for src_kw, dst_kw in (({}, {}), (dict(with_info=False), {}), ({}, dict(with_info=False, with_magnitudes=False)),
                           (dict(with_slot_route=True, with_obs=True), dict(with_slot_route=True, with_obs=True)),
                           ({}, dict(with_slot_route=True))):
        src, dst = _random_state(rng, 5, A, **src_kw), _random_state(rng, 7, A, **dst_kw)
        for se, de in (([3], [6]), ([4, 0, 2], [1, 5, 0]), ([0, 1, 2, 3, 4], [6, 2, 4, 0, 1]), ([0, 5, -1, 2, 1], [1, 2, 3, 7, -2]), ([4, 1], [0, 9])):
            base = {n: (None if a is None else a.copy()) for n, a in dst.arrays.items()}
            got = S.state_copy(src.arrays, {n: (None if a is None else a.copy()) for n, a in base.items()}, 5, 7, A, se, de, outputs)
            want = brute(src.arrays, {n: (None if a is None else a.copy()) for n, a in base.items()}, 5, 7, A, se, de, outputs)
            touched = {d for s, d in S.valid_pairs(se, de, 5, 7)}
            for n in _abi.STATE_PTRS:
                if base[n] is None:
                    assert got[n] is None
                    continue
                assert np.array_equal(S.rows(got[n], 7), S.rows(want[n], 7)), (n, se, de)
                rest = [r for r in range(7) if r not in touched]
                assert np.array_equal(S.rows(got[n], 7)[rest], S.rows(base[n], 7)[rest]), n
                moved = S.group(n) == "copied" or (outputs and S.group(n) == "outputs")
                if touched and moved and src.arrays[n] is not None and S.rows(base[n], 7).shape[1] >= 8:      # (random rows of 8 bytes differ)
                    assert not np.array_equal(S.rows(got[n], 7), S.rows(base[n], 7)), n
            if touched:
                d = min(touched)
                assert not got["slot_cache"].reshape(7, -1)[d].any() and not got["env_cache"][d].any()
                assert got["act_cache"].reshape(7, A + 1, 2)[d].tolist() == [[0, 0]] * A + [[-1, 0]]


def test_frames_restatement_turns_the_ring():
    rng = np.random.default_rng(3)
    for ns in (1, 3, 4):
        sl, so = rng.integers(0, 256, (5, ns, 16), dtype=np.uint8), rng.integers(0, 256, (5, 3 * ns, 16), dtype=np.uint8)
        for sp in range(ns):
            for dp in range(ns):
                dl, do = np.full((7, ns, 16), 0xEE, np.uint8), np.full((7, 3 * ns, 16), 0xEE, np.uint8)
                S.frames_copy(sl, dl, so, do, ns, sp, dp, [4, 1, 9], [0, 6, 2])
                for s, d in ((4, 0), (1, 6)):
                    # age by age: the frame written `age` pushes ago sits `age` slots behind the phase on either side
                    for age in range(1, ns + 1):
                        assert np.array_equal(dl[d, (dp - age) % ns], sl[s, (sp - age) % ns])
                    assert np.array_equal(do[d], so[s])
                assert (dl[[1, 2, 3, 4, 5]] == 0xEE).all() and (do[[1, 2, 3, 4, 5]] == 0xEE).all()
