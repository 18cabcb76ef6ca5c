"""CPU checks of the "driven" family (include/tde_driven.h, _lib.ADDED_FAMILIES): the record held to the rules
tests/test_abi_families_cpu.py states for a family (that file pins _lib.FAMILIES to its eight names and is not edited: its helpers are
imported), the host-side refusals of tde_env_step_driven by message, and tests/driven_ref.py - the numpy statement of the step's motion
half with the override - against the oracle's step with nothing driven and with every NPC echoing the controller's own action."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import config_zoo, driven_ref
from tests.test_abi_families_cpu import COMPILERS, CSRC, INCLUDE, PINS, c_status, includes, reach
from torchdriveenv_amd import _abi, _lib, build, ops
from torchdriveenv_amd.state import EnvState

FAM = _lib.ADDED_FAMILIES[0]
PIN = (1, {"tde_driven_version": 0, "tde_env_step_driven": 6})
each_compiler = pytest.mark.parametrize("cc,ext", COMPILERS, ids=["c", "cxx"])


def test_families_is_untouched_and_the_added_list_holds_the_driven_record():
    assert [f.name for f in _lib.FAMILIES] == list(PINS) and len(_lib.FAMILIES) == 8 and len(_lib.symbols("core")) == 31
    assert [f.name for f in _lib.ADDED_FAMILIES] == ["driven"]
    assert (FAM.header, FAM.unit, FAM.version) == ("tde_driven.h", "tde_step_driven.hip", "TDE_DRIVEN_VERSION")
    assert _lib.symbols("driven") == list(PIN[1])
    every = [s[0] for f in _lib.FAMILIES + _lib.ADDED_FAMILIES for s in f.symbols]
    assert len(set(every)) == len(every)


@each_compiler
def test_header_compiles_alone_ahead_of_and_behind_all_the_others(tmp_path, cc, ext):
    syms = _lib.symbols("driven")
    functions = " + ".join(f"sizeof(&{s})" for s in syms) + f" != {len(syms)} * sizeof(void (*)(void))"
    assert c_status(tmp_path, [FAM.header], f"(TDE_DRIVEN_VERSION - 1) | (TDE_ABI_VERSION - {PINS['core'][0]}) | ({functions})", cc, ext) == 0
    others = [f.header for f in _lib.FAMILIES]
    for order in ([FAM.header] + others, others + [FAM.header], others[::-1] + [FAM.header]):
        assert c_status(tmp_path, order, "TDE_DRIVEN_VERSION - 1", cc, ext) == 0


def test_header_builds_on_tde_hip_and_declares_the_records_symbols():
    assert includes(FAM.header) == ["tde_hip.h"] and reach(FAM.header) == {"tde_driven.h", "tde_hip.h", "tde_abi.h"}
    text = open(os.path.join(INCLUDE, FAM.header)).read()
    declared = re.findall(r"TDE_API\s+[\w\s\*]+?\b(tde_\w+)\s*\(", text)
    table = _lib.symbols("driven")
    assert table[0].endswith("_version") and [s for s in declared if s.endswith("_version")] == table[:1]
    assert [s for s in declared if s != table[0]] == table[1:]
    assert len(re.findall(r"^TDE_API\s", text, re.M)) == len(table)
    assert "slot index" in text.lower()                       # the mask of a re-spawned env: said in the header


def test_version_macro_abi_and_library_agree_and_the_argtypes_count_is_six():
    defines = [int(v) for h in sorted(reach(FAM.header))
               for v in re.findall(r"^#define TDE_DRIVEN_VERSION (\d+)\b", open(os.path.join(INCLUDE, h)).read(), re.M)]
    L = _lib.load()
    assert defines == [1] and _abi.TDE_DRIVEN_VERSION == 1 == L.tde_driven_version()
    assert [len(getattr(L, s).argtypes) for s in PIN[1]] == list(PIN[1].values()) == [0, 6]
    assert all(getattr(L, s).restype is C.c_int for s in PIN[1])


def test_units_and_header_are_what_the_build_depends_on():
    deps = [os.path.normpath(d) for d in build.DEPS]
    assert all(os.path.exists(d) for d in build.DEPS)
    assert os.path.join(INCLUDE, FAM.header) in deps and os.path.join(CSRC, FAM.unit) in deps
    assert build.UNITS.count(FAM.unit) == 1 and build.UNITS.count("tde_step_driven_mag.hip") == 1
    assert FAM.unit not in [f.unit for f in _lib.FAMILIES]


def test_a_library_without_a_symbol_of_the_family_is_a_stale_build(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "ADDED_FAMILIES", [FAM._replace(symbols=FAM.symbols + [("tde_driven_not_there", [])])])
    with pytest.raises(_lib.TdeError) as err:
        _lib.load()
    assert str(err.value) == f"{_lib.LIB_PATH} lacks symbols ['tde_driven_not_there']: stale build?"
    monkeypatch.undo()
    _lib.load()


def test_a_library_of_another_version_is_refused_by_the_family(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_abi, "TDE_DRIVEN_VERSION", 2)
    with pytest.raises(_lib.TdeError) as err:
        _lib.load()
    assert str(err.value) == "driven version mismatch: library 1 vs python 2"
    monkeypatch.undo()
    _lib.load()


def test_an_older_family_at_fault_is_reported_ahead_of_the_added_one(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_abi, "TDE_DRIVEN_VERSION", 2)
    monkeypatch.setattr(_abi, "TDE_SNAPSHOT_VERSION", 2)
    with pytest.raises(_lib.TdeError, match=r"^snapshot version mismatch: library 1 vs python 2$"):
        _lib.load()
    monkeypatch.undo()
    _lib.load()


# ---- refusals of the entry point: all on the host, ahead of any launch (host structs: nothing is dereferenced) ---------------------
def _host_args(A=4, B=2, **state_kw):
    world = config_zoo.world(None, A)
    cfg = config_zoo.config(None, A)
    hs = EnvState(B, A, **state_kw)
    return cfg, world, hs


def _refused(cfg, world, st, agent_action, driven):
    L = _lib.load()
    rc = L.tde_env_step_driven(None if cfg is None else C.byref(cfg), None if world is None else C.byref(world.host_struct()),
                               None if st is None else C.byref(st.struct if hasattr(st, "struct") else st), agent_action, driven, None)
    assert rc != 0
    return L.tde_last_error().decode()


def test_refusals_through_the_c_abi_by_message():
    cfg, world, hs = _host_args()
    one = C.c_void_p(16)                                   # (an address that is never read: the refusals precede every launch)
    assert _refused(None, world, hs, None, None) == "tde_env_step_driven: NULL argument"
    assert _refused(cfg, None, hs, None, None) == "tde_env_step_driven: NULL argument"
    assert _refused(cfg, world, None, None, None) == "tde_env_step_driven: NULL argument"
    st = _abi.TdeState.from_buffer_copy(hs.struct)
    st.A = 3
    assert _refused(cfg, world, st, None, None) == "tde_env_step_driven: A must be a power of two in [1,128]"
    st.A = 8
    assert _refused(cfg, world, st, None, None) == "tde_env_step_driven: world.A (4) != state.A (8)"
    bad = config_zoo.config(None, 4, npc_max_steer=-1.0)
    assert _refused(bad, world, hs, None, None) == "tde_env_step_driven: config.npc_max_steer must be >= 0 (got -1)"
    bad = config_zoo.config(None, 4, npc_max_accel=0.0)
    assert _refused(bad, world, hs, None, None) == "tde_env_step_driven: config.npc_max_accel must be in [1e-3, 1e3] m/s^2 (got 0)"
    assert _refused(cfg, world, hs, None, one) == "tde_env_step_driven: driven is set and agent_action is NULL"
    routed = _host_args(with_slot_route=True)[2]
    assert routed.struct.slot_route
    assert _refused(cfg, world, routed, one, one).startswith("tde_env_step_driven: state.slot_route is set: ")
    assert _refused(cfg, world, routed, None, None).startswith("tde_env_step_driven: state.slot_route is set: ")
    st = _abi.TdeState.from_buffer_copy(hs.struct)
    st.action = None
    assert _refused(cfg, world, st, None, None) == "tde_env_step_driven: state.action is NULL"
    st = _abi.TdeState.from_buffer_copy(hs.struct)
    st.B = 0                                               # an empty batch is no error and launches nothing
    assert _lib.load().tde_env_step_driven(C.byref(cfg), C.byref(world.host_struct()), C.byref(st), None, None, None) == 0


def test_refusals_of_the_tensor_checks_by_message():
    B, A = 2, 4
    with pytest.raises(ValueError, match="^driven must be a torch tensor$"):
        ops.check_driven(torch.zeros(B, A, 2), np.zeros((B, A), np.uint8), B, A, "cuda:0")
    with pytest.raises(ValueError, match="^driven must be torch.uint8, got torch.int32$"):
        ops.check_driven(torch.zeros(B, A, 2), torch.zeros(B, A, dtype=torch.int32), B, A, "cuda:0")
    with pytest.raises(ValueError, match="^agent_action must be torch.float32, got torch.float64$"):
        ops.check_driven(torch.zeros(B, A, 2, dtype=torch.float64), None, B, A, "cuda:0")
    with pytest.raises(ValueError, match=r"^driven must live on a HIP device \(there is no CPU path\)$"):
        ops.check_driven(torch.zeros(B, A, 2), torch.zeros(B, A, dtype=torch.bool), B, A, "cuda:0")
    assert ops.check_driven(None, None, B, A, "cuda:0") == (None, None)


# ---- driven_ref against the oracle ---------------------------------------------------------------------------------------------------
MOTION = ("x", "y", "psi", "v", "route_wp")


@pytest.mark.parametrize("lights", [False, True], ids=["nolights", "lights"])
@pytest.mark.parametrize("A", [4, 16])
def test_driven_ref_equals_the_oracle_with_nothing_driven_and_with_every_npc_echoed(A, lights):
    """4 steps without the re-spawn (the oracle's step leaves the poses the motion half made); the echo drives every present NPC slot
    without a live replay record with the controller's own action (driven_ref.npc_actions), and the other rows hold NaN"""
    B = 6
    world = config_zoo.world(None, A)
    flags = (config_zoo.FLAGS if lights else config_zoo.FLAGS & ~_abi.F_TRAFFIC_LIGHTS) & ~_abi.F_AUTORESET
    cfg = config_zoo.config(None, A, flags=flags)
    hs = EnvState(B, A)
    oracle.env_reset(cfg, world, hs)
    acts = config_zoo.actions(None, B, A, T=4)
    n_echo = 0
    for t in range(4):
        hs["action"][...] = acts[t]
        pre = hs.host()
        s = driven_ref._scene(cfg, world, pre)
        live_record = (s["replay"] >= 0) & (s["k"] < s["replay_len"])
        mask = (s["other"] & ~live_record).reshape(B, A)
        echo = driven_ref.npc_actions(cfg, world, pre)
        echo[~mask] = np.nan
        plain = driven_ref.step_motion(cfg, world, pre)
        echoed = driven_ref.step_motion(cfg, world, pre, echo, mask.astype(np.uint8))
        oracle.env_step(cfg, world, hs)
        for k in MOTION:
            want = np.ascontiguousarray(hs[k]).view(np.uint32)
            assert np.array_equal(plain[k].view(np.uint32), want), (t, k)
            assert np.array_equal(echoed[k].view(np.uint32), want), (t, k)
        n_echo += int(mask.sum())
        moved = np.asarray(hs["v"]).reshape(B, A)[:, 1:]
    assert n_echo > 0 and np.any(moved != 0)
