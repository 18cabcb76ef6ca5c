"""CPU checks of the "agents" family (include/tde_agents.h, _lib.LATER_FAMILIES): the record held to the rules
tests/test_abi_families_cpu.py states for a family (its helpers are imported, as tests/test_driven_cpu.py does); every host-side refusal
of tde_agent_obs and tde_agent_outcomes by message, on host structs; tests/agent_obs_ref.py - the numpy statement of both entry points -
against tests/vector_obs_ref.py and the oracle's reward; and the closed loop of tests/agents_cases.py on the references alone: it
must hold every outcome flag before tests/test_gpu_agents.py runs it on the GPU.  The list _lib.LATER_FAMILIES is not pinned here: the
next family appends to it."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import agent_obs_ref as ref
from tests import agents_cases as ac
from tests import config_zoo, vector_obs_ref
from tests.test_abi_families_cpu import COMPILERS, CSRC, INCLUDE, PINS, c_status, includes, reach
from torchdriveenv_amd import _abi, _lib, build, ops
from torchdriveenv_amd.config import VectorObs
from torchdriveenv_amd.state import EnvState

FAM = next(f for f in _lib.LATER_FAMILIES if f.name == "agents")
PIN = (1, {"tde_agents_version": 0, "tde_agent_obs": 9, "tde_agent_outcomes": 9})
each_compiler = pytest.mark.parametrize("cc,ext", COMPILERS, ids=["c", "cxx"])


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


# ---- the family rules -----------------------------------------------------------------------------------------------------------------
def test_the_record_is_in_the_later_list_and_no_symbol_occurs_twice_over_the_three_lists():
    assert [f.name for f in _lib.LATER_FAMILIES].count("agents") == 1
    assert (FAM.header, FAM.unit, FAM.version) == ("tde_agents.h", "tde_agents.hip", "TDE_AGENTS_VERSION")
    assert _lib.symbols("agents") == list(PIN[1])
    every = [s[0] for f in _lib.FAMILIES + _lib.ADDED_FAMILIES + _lib.LATER_FAMILIES for s in f.symbols]
    assert len(set(every)) == len(every)
    names = [f.name for f in _lib.FAMILIES + _lib.ADDED_FAMILIES + _lib.LATER_FAMILIES]
    assert len(set(names)) == len(names)


@each_compiler
def test_header_compiles_alone_ahead_of_and_behind_all_the_others(tmp_path, cc, ext):
    syms = _lib.symbols("agents")
    functions = " + ".join(f"sizeof(&{s})" for s in syms) + f" != {len(syms)} * sizeof(void (*)(void))"
    layout = "sizeof(tde_agent_track) != 32 || (TDE_AG_VALID | TDE_AG_COLLIDED | TDE_AG_OFFROAD | TDE_AG_REACHED | TDE_AG_ENDED) != 31"
    assert c_status(tmp_path, [FAM.header], f"(TDE_AGENTS_VERSION - 1) | (TDE_ABI_VERSION - {PINS['core'][0]}) | ({functions}) | ({layout})", cc, ext) == 0
    others = [f.header for f in _lib.FAMILIES + _lib.ADDED_FAMILIES]
    for order in ([FAM.header] + others, others + [FAM.header], others[::-1] + [FAM.header]):
        assert c_status(tmp_path, order, "TDE_AGENTS_VERSION - 1", cc, ext) == 0


def test_header_builds_on_tde_hip_alone_and_declares_the_records_symbols():
    assert includes(FAM.header) == ["tde_hip.h"] and reach(FAM.header) == {"tde_agents.h", "tde_hip.h", "tde_abi.h"}
    text = open(os.path.join(INCLUDE, FAM.header)).read()
    declared = re.findall(r"TDE_API\s+[\w\s\*]+?\b(tde_\w+)\s*\(", text)
    table = _lib.symbols("agents")
    assert table[0].endswith("_version") and [s for s in declared if s.endswith("_version")] == table[:1]
    assert [s for s in declared if s != table[0]] == table[1:]
    assert len(re.findall(r"^TDE_API\s", text, re.M)) == len(table)


def test_version_macro_abi_library_struct_and_flags_agree():
    text = "".join(open(os.path.join(INCLUDE, h)).read() for h in sorted(reach(FAM.header)))
    assert [int(v) for v in re.findall(r"^#define TDE_AGENTS_VERSION (\d+)\b", text, re.M)] == [1]
    L = _lib.load()
    assert _abi.TDE_AGENTS_VERSION == 1 == L.tde_agents_version()
    assert [len(getattr(L, s).argtypes) for s in PIN[1]] == list(PIN[1].values())
    assert all(getattr(L, s).restype is C.c_int for s in PIN[1])
    flags = {n: int(v) for n, v in re.findall(r"^#define TDE_AG_(\w+)\s+(\d+)\b", text, re.M)}
    assert flags == dict(VALID=_abi.AG_VALID, COLLIDED=_abi.AG_COLLIDED, OFFROAD=_abi.AG_OFFROAD, REACHED=_abi.AG_REACHED, ENDED=_abi.AG_ENDED)
    assert flags == dict(VALID=1, COLLIDED=2, OFFROAD=4, REACHED=8, ENDED=16)
    assert C.sizeof(_abi.TdeAgentTrack) == 32 == ref.TRACK.itemsize
    assert [(n, getattr(_abi.TdeAgentTrack, n).offset) for n, _ in _abi.TdeAgentTrack._fields_] == [(n, ref.TRACK.fields[n][1]) for n in ref.TRACK.names]


def test_unit_headers_and_the_single_unit_form_are_what_the_build_depends_on():
    deps = [os.path.normpath(d) for d in build.DEPS]
    assert all(os.path.exists(d) for d in build.DEPS)
    assert os.path.join(INCLUDE, FAM.header) in deps and os.path.join(CSRC, FAM.unit) in deps
    assert os.path.join(CSRC, "tde_vector_obs_dev.h") in deps                   # the helpers both observation units include
    assert build.UNITS.count(FAM.unit) == 1
    assert FAM.unit not in [f.unit for f in _lib.FAMILIES + _lib.ADDED_FAMILIES]
    single = open(os.path.join(CSRC, "tde_kernels.hip")).read()
    assert single.count(f'#include "{FAM.unit}"') == 1
    for unit in ("tde_vector_obs.hip", FAM.unit):
        assert '#include "tde_vector_obs_dev.h"' in open(os.path.join(CSRC, unit)).read()


def test_a_library_without_a_symbol_of_the_family_is_a_stale_build(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LATER_FAMILIES", [f._replace(symbols=f.symbols + [("tde_agents_not_there", [])]) if f is FAM else f
                                                 for f in _lib.LATER_FAMILIES])
    with pytest.raises(_lib.TdeError) as err:
        _lib.load()
    assert str(err.value) == f"{_lib.LIB_PATH} lacks symbols ['tde_agents_not_there']: stale build?"
    monkeypatch.undo()
    _lib.load()


def test_a_library_of_another_version_is_refused_by_the_family(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_abi, "TDE_AGENTS_VERSION", 2)
    with pytest.raises(_lib.TdeError) as err:
        _lib.load()
    assert str(err.value) == "agents version mismatch: library 1 vs python 2"
    monkeypatch.undo()
    _lib.load()


def test_symbols_are_checked_before_the_version_and_an_older_family_at_fault_is_reported_first(monkeypatch):
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_abi, "TDE_AGENTS_VERSION", 2)
    monkeypatch.setattr(_lib, "LATER_FAMILIES", [FAM._replace(symbols=FAM.symbols + [("tde_agents_not_there", [])])])
    with pytest.raises(_lib.TdeError, match=r"lacks symbols \['tde_agents_not_there'\]: stale build\?$"):
        _lib.load()
    monkeypatch.setattr(_abi, "TDE_DRIVEN_VERSION", 2)
    with pytest.raises(_lib.TdeError, match=r"^driven version mismatch: library 1 vs python 2$"):
        _lib.load()
    monkeypatch.setattr(_abi, "TDE_SNAPSHOT_VERSION", 2)
    with pytest.raises(_lib.TdeError, match=r"^snapshot version mismatch: library 1 vs python 2$"):
        _lib.load()
    monkeypatch.undo()
    _lib.load()


# ---- refusals of the entry points: all on the host, ahead of any launch (host structs: nothing is dereferenced) ---------------------
ONE = C.c_void_p(16)                                       # (an address that is never read: the refusals precede every launch)


def _host_args(A=4, B=2, flags=None, **state_kw):
    world = config_zoo.world(None, A)
    cfg = config_zoo.config(None, A) if flags is None else config_zoo.config(None, A, flags=flags)
    return cfg, world, EnvState(B, A, **state_kw)


def _vo(**kw):
    v = dict(ray_dir=16, k_nbr=2, n_rays=4, nbr_radius=30.0, ray_range=10.0, ray_step=0.5)
    v.update(kw)
    return _abi.TdeVectorObs(v["ray_dir"], v["k_nbr"], v["n_rays"], v["nbr_radius"], v["ray_range"], v["ray_step"], 0)


def _ref(x):
    return None if x is None else C.byref(x.host_struct() if hasattr(x, "host_struct") else x.struct if hasattr(x, "struct") else x)


def _obs_refused(cfg, world, st, vo, pairs=ONE, n=1, out=ONE, track=None):
    L = _lib.load()
    rc = L.tde_agent_obs(_ref(cfg), _ref(world), _ref(st), _ref(vo), pairs, n, out, track, None)
    assert rc != 0
    return L.tde_last_error().decode()


def _out_refused(cfg, world, st, pairs=ONE, n=1, track=ONE, reward=ONE, flags=ONE):
    L = _lib.load()
    rc = L.tde_agent_outcomes(_ref(cfg), _ref(world), _ref(st), pairs, n, track, reward, flags, None)
    assert rc != 0
    return L.tde_last_error().decode()


def test_refusals_of_tde_agent_obs_by_message():
    cfg, world, hs = _host_args()
    vo = _vo()
    fn = "tde_agent_obs: "
    assert _obs_refused(None, world, hs, vo) == fn + "NULL argument"
    assert _obs_refused(cfg, None, hs, vo) == fn + "NULL argument"
    assert _obs_refused(cfg, world, None, vo) == fn + "NULL argument"
    assert _obs_refused(cfg, world, hs, None) == fn + "NULL argument"
    st = _abi.TdeState.from_buffer_copy(hs.struct)
    st.A = 3
    assert _obs_refused(cfg, world, st, vo) == fn + "A must be a power of two in [1,128]"
    st.A = 8
    assert _obs_refused(cfg, world, st, vo) == fn + "world.A (4) != state.A (8)"
    # everything tde_vector_obs refuses, in its words
    assert _obs_refused(cfg, world, hs, _vo(k_nbr=17)) == fn + "k_nbr must be in [0, TDE_VO_MAX_NBR]"
    assert _obs_refused(cfg, world, hs, _vo(k_nbr=-1)) == fn + "k_nbr must be in [0, TDE_VO_MAX_NBR]"
    assert _obs_refused(cfg, world, hs, _vo(n_rays=65)) == fn + "n_rays must be in [0, TDE_VO_MAX_RAYS]"
    assert _obs_refused(cfg, world, hs, _vo(ray_dir=None)) == fn + "ray_dir is NULL"
    for bad in (dict(nbr_radius=0.0), dict(ray_range=float("inf")), dict(ray_step=float("nan")), dict(ray_step=-1.0)):
        assert _obs_refused(cfg, world, hs, _vo(**bad)) == fn + "nbr_radius, ray_range and ray_step must be finite and > 0"
    for bad in (dict(ray_step=0.3), dict(ray_range=1.0, ray_step=2.0), dict(ray_range=2000.0, ray_step=1.0)):
        assert _obs_refused(cfg, world, hs, _vo(**bad)) == fn + "ray_range / ray_step must be an integer in [1, TDE_VO_MAX_SAMPLES]"
    assert _obs_refused(config_zoo.config(None, 4, max_steps=0), world, hs, vo) == fn + "config.max_steps must be >= 1"
    for name in ("x", "wid", "present", "steps", "target_idx"):
        st = _abi.TdeState.from_buffer_copy(hs.struct)
        setattr(st, name, None)
        assert _obs_refused(cfg, world, st, vo) == fn + "a required state / world pointer is NULL"
    ws = _abi.TdeWorld.from_buffer_copy(world.host_struct())
    ws.cell_coarse = None
    assert _obs_refused(cfg, ws, hs, vo) == fn + "a required state / world pointer is NULL"
    ws = _abi.TdeWorld.from_buffer_copy(world.host_struct())
    ws.stoplines = None
    assert cfg.flags & _abi.F_TRAFFIC_LIGHTS
    assert _obs_refused(cfg, ws, hs, vo) == fn + "TDE_F_TRAFFIC_LIGHTS without stop lines / phases"
    # its own
    ws = _abi.TdeWorld.from_buffer_copy(world.host_struct())
    ws.spawn = None
    assert _obs_refused(cfg, ws, hs, vo) == fn + "world.spawn is NULL"
    for name in ("route_wp", "episode"):
        st = _abi.TdeState.from_buffer_copy(hs.struct)
        setattr(st, name, None)
        assert _obs_refused(cfg, world, st, vo) == fn + "state.route_wp or state.episode is NULL"
    ws = _abi.TdeWorld.from_buffer_copy(world.host_struct())
    assert ws.n_routes > 0
    ws.route_xy = None
    assert _obs_refused(cfg, ws, hs, vo) == fn + "world.route_xy is NULL with n_routes > 0"
    assert _obs_refused(cfg, world, hs, vo, n=-1) == fn + "n must be >= 0"
    assert _obs_refused(cfg, world, hs, vo, pairs=None) == fn + "pairs or out is NULL with n > 0"
    assert _obs_refused(cfg, world, hs, vo, out=None) == fn + "pairs or out is NULL with n > 0"
    # n == 0 is no error, launches nothing and needs neither pointer; a state with per-slot routes is taken as any other
    L = _lib.load()
    assert L.tde_agent_obs(_ref(cfg), _ref(world), _ref(hs), _ref(vo), None, 0, None, None, None) == 0
    routed = _host_args(with_slot_route=True)[2]
    assert routed.struct.slot_route and L.tde_agent_obs(_ref(cfg), _ref(world), _ref(routed), _ref(vo), None, 0, None, None, None) == 0
    assert _obs_refused(cfg, world, routed, vo, n=-1) == fn + "n must be >= 0"


def test_refusals_of_tde_agent_outcomes_by_message():
    cfg, world, hs = _host_args()
    fn = "tde_agent_outcomes: "
    assert _out_refused(None, world, hs) == fn + "NULL argument"
    assert _out_refused(cfg, None, hs) == fn + "NULL argument"
    assert _out_refused(cfg, world, None) == fn + "NULL argument"
    assert _out_refused(cfg, world, hs, n=-3) == fn + "n must be >= 0"
    for kw in (dict(pairs=None), dict(track=None), dict(reward=None), dict(flags=None)):
        assert _out_refused(cfg, world, hs, **kw) == fn + "pairs, track, reward or flags is NULL with n > 0"
    for name in ("x", "y", "psi", "route_wp", "present", "collided", "offroad", "episode"):
        st = _abi.TdeState.from_buffer_copy(hs.struct)
        setattr(st, name, None)
        assert _out_refused(cfg, world, st) == fn + "a required state pointer is NULL"
    assert _lib.load().tde_agent_outcomes(_ref(cfg), _ref(world), _ref(hs), None, 0, None, None, None, None) == 0


def test_refusals_of_the_tensor_checks_by_message():
    with pytest.raises(ValueError, match="^pairs is required$"):
        ops.check_agent_pairs(None, "cuda:0")
    with pytest.raises(ValueError, match="^pairs must be a torch tensor$"):
        ops.check_agent_pairs(np.zeros((1, 2), np.int32), "cuda:0")
    with pytest.raises(ValueError, match="^pairs must be torch.int32, got torch.int64$"):
        ops.check_agent_pairs(torch.zeros(1, 2, dtype=torch.int64), "cuda:0")
    with pytest.raises(ValueError, match=r"^pairs must live on a HIP device \(there is no CPU path\)$"):
        ops.check_agent_pairs(torch.zeros(1, 2, dtype=torch.int32), "cuda:0")


# ---- agent_obs_ref against vector_obs_ref on oracle states ---------------------------------------------------------------------------
SWAPPED = ("x", "y", "psi", "v", "len", "wid", "present")


@pytest.mark.parametrize("lights", [False, True], ids=["nolights", "lights"])
@pytest.mark.parametrize("A", [4, 16])
def test_obs_ref_equals_vector_obs_ref_for_slot_0_and_on_states_with_rows_swapped(A, lights):
    """after a reset and 3 oracle steps: a slot-0 pair is vector_obs_ref's row; for a >= 1 the speed / size entries, the step and light
    entries and the neighbour and ray blocks are vector_obs_ref's on a copy of the state whose rows 0 and a are swapped - in the envs
    where no two candidates of any observer are equally far (the order among ties is by slot index, which the swap changes)"""
    B = 6
    world = config_zoo.world(None, A)
    cfg = config_zoo.config(None, A, flags=config_zoo.FLAGS if lights else config_zoo.FLAGS & ~_abi.F_TRAFFIC_LIGHTS)
    hs = EnvState(B, A)
    oracle.env_reset(cfg, world, hs)
    acts = config_zoo.actions(None, B, A, T=3)
    for t in range(3):
        hs["action"][...] = acts[t]
        oracle.env_step(cfg, world, hs)
    h = hs.host()
    vo = VectorObs(k_neighbours=3, n_rays=5, ray_range=10.0, ray_step=0.5, neighbour_radius=40.0)
    e, a = np.divmod(np.arange(B * A), A)
    pairs = np.stack([e, a], -1)
    rows, track = ref.agent_obs(cfg, world, h, vo, pairs)
    rows = rows.reshape(B, A, -1)
    want0 = vector_obs_ref.vector_obs(cfg, world, h, vo)
    assert np.array_equal(bits(rows[:, 0]), bits(want0)) and np.any(want0[:, 10:] != 0)
    x, y, pres = (np.asarray(h[k]).reshape(B, A) for k in ("x", "y", "present"))
    keep = [0, 1, 2, 8, 9] + list(range(10, vo.dim))
    tie_free, compared = 0, 0
    for env in range(B):
        ties = False
        for obs in np.flatnonzero(pres[env]):
            o = np.flatnonzero(pres[env] & (np.arange(A) != obs))
            dx, dy = x[env, o] - x[env, obs], y[env, o] - y[env, obs]
            d2 = (dx * dx + dy * dy).astype(np.float32)
            ties |= len(np.unique(d2.view(np.uint32))) != len(d2)
        if ties:
            continue
        tie_free += 1
        only = np.zeros(B, np.uint8)
        only[env] = 1
        for obs in range(1, A):
            if not pres[env, obs]:
                assert not rows[env, obs].any() and not track[env * A + obs]["present"]
                continue
            sw = {k: np.array(v, copy=True) for k, v in h.items()}
            for k in SWAPPED:
                r = sw[k].reshape(B, A)
                r[env, 0], r[env, obs] = r[env, obs].copy(), r[env, 0].copy()
            want = vector_obs_ref.vector_obs(cfg, world, sw, vo, only=only)[env]
            assert np.array_equal(bits(rows[env, obs][keep]), bits(want[keep])), (env, obs)
            compared += 1
    assert tie_free >= 1 and compared >= 2
    assert np.all(track["present"].reshape(B, A) == (pres != 0))
    live = pres != 0
    assert np.array_equal(bits(track["x"].reshape(B, A)[live]), bits(x[live])) and np.array_equal(track["steps"].reshape(B, A)[live], np.repeat(h["steps"], A).reshape(B, A)[live])


def test_obs_ref_takes_the_waypoint_entries_of_a_slot_from_its_route_or_its_slot_route_word():
    A, B = 16, 4
    world = config_zoo.world(None, A)
    cfg = config_zoo.config(None, A)
    hs = EnvState(B, A, with_slot_route=True)
    oracle.env_reset(cfg, world, hs)
    h = hs.host()
    rec = world.arrays["spawn"].reshape(-1, A)[h["scn"]]
    e, a = np.nonzero((rec["route"] >= 0) & (rec["route_n"] > 2) & (h["present"].reshape(B, A) != 0) & (np.arange(A) > 0))
    assert len(e) >= 2
    e0, a0, e1, a1 = e[0], a[0], e[1], a[1]
    other = int(rec["route"][e1, a1])
    h["slot_route"].reshape(B, A)[e0, a0] = (other + 1) | (2 << 20)          # two waypoints of another route
    h["route_wp"].reshape(B, A)[e0, a0] = 1
    vo = VectorObs(k_neighbours=0, n_rays=0)
    rows, _ = ref.agent_obs(cfg, world, h, vo, [[e0, a0], [e1, a1]])
    route_xy = world.arrays["route_xy"].reshape(-1, world.ints["RW"], 2)
    s, c = oracle.sincosf(np.asarray(h["psi"], np.float32))
    for row, (ee, aa, route, j, n) in zip(rows, [(e0, a0, other, 1, 2), (e1, a1, other, int(h["route_wp"].reshape(B, A)[e1, a1]), int(rec["route_n"][e1, a1]))]):
        g = ee * A + aa
        dx, dy = route_xy[route, j, 0] - h["x"][g], route_xy[route, j, 1] - h["y"][g]
        assert row[3] == dx * c[g] + dy * s[g] and row[4] == dy * c[g] - dx * s[g]
        assert row[7] == min(n - j, 2) and (row[7] == 2 or (row[5] == 0 and row[6] == 0))


# ---- agent_outcomes_ref against the oracle's reward ----------------------------------------------------------------------------------
def test_outcomes_ref_with_the_egos_poses_gives_the_oracles_distance_and_heading_terms():
    """slot 1 of a made-up state holds the ego's pose after an oracle step and the track its pose before it, with no waypoint reached:
    the reward is the oracle's waypoint_reward for those poses with no target left, bit for bit, over 12 steps of 6 envs"""
    A, B = 16, 6
    world = config_zoo.world(None, A)
    cfg = config_zoo.config(None, A, distance_cutoff=0.25)
    hs = EnvState(B, A)
    oracle.env_reset(cfg, world, hs)
    acts = config_zoo.actions(None, B, A, T=12)
    ego, pairs = np.arange(B) * A, np.stack([np.arange(B), np.ones(B, np.int64)], -1)
    four = lambda d: np.stack([np.asarray(d[k], np.float32)[ego] for k in ("x", "y", "psi", "v")], -1)      # noqa: E731
    seen = set()
    for t in range(12):
        hs["action"][...] = acts[t]
        pre = hs.host()
        oracle.env_step(cfg, world, hs)
        post = hs.host()
        same = post["episode"] == pre["episode"]
        track = np.zeros(B, ref.TRACK)
        for k in ("x", "y", "psi", "v"):
            track[k] = pre[k][ego]
        track["present"], track["episode"] = 1, 7
        fake = {k: np.array(v, copy=True) for k, v in post.items()}
        fake["episode"][:] = 7
        for k in ("x", "y", "psi"):
            fake[k][ego + 1] = post[k][ego]
        fake["present"][ego + 1], fake["collided"][ego + 1], fake["offroad"][ego + 1], fake["route_wp"][ego + 1] = 1, 0, 0, 0
        got, flags = ref.agent_outcomes(cfg, world, fake, pairs, track)
        zeros = np.zeros(B, np.int32)
        want = oracle.waypoint_reward(cfg, four(pre), four(post), np.zeros(B, np.uint8), np.zeros(B, np.uint8), None,
                                      world.arrays["wp_xy"].reshape(-1, world.ints["NW"], 2), np.zeros(world.n_scn, np.int32), pre["scn"],
                                      zeros.copy(), zeros.copy(), zeros.copy())
        assert np.array_equal(bits(got[same]), bits(want["reward"][same])), t
        assert np.all(flags == _abi.AG_VALID)
        seen |= set(np.round(want["info"][same, 3]).astype(int))           # the distance term: 0 and distance_bonus
    assert seen == {0, 1}
    fake["route_wp"][ego + 1] = 1                                              # a waypoint reached: the bonus, ahead of the other terms
    got2, flags2 = ref.agent_outcomes(cfg, world, fake, pairs, track)
    assert np.all(flags2 == _abi.AG_VALID | _abi.AG_REACHED)
    assert np.array_equal(got2, ((cfg.waypoint_bonus + want["info"][:, 3]) + want["info"][:, 2]).astype(np.float32))


# ---- the closed loop of the GPU test, on the references alone ------------------------------------------------------------------------
def test_the_closed_loop_scene_holds_every_flag_on_the_references_alone():
    from tests.test_gpu_driven import AGENT, ENV, ref_step

    world, cfg = ac.loop_world(), ac.loop_config()
    hs = EnvState(ac.B, ac.A)
    oracle.env_reset(cfg, world, hs)
    h = hs.host()
    ac.loop_stage(h)
    aa, drv = ac.loop_actions()
    pairs = ac.loop_pairs()
    acts = config_zoo.actions(None, ac.B, ac.A, T=ac.T)
    vo = VectorObs(k_neighbours=1, n_rays=0)
    count = dict.fromkeys((_abi.AG_COLLIDED, _abi.AG_OFFROAD, _abi.AG_REACHED, _abi.AG_ENDED), 0)
    respawns = 0
    for t in range(ac.T):
        h["action"] = acts[t]
        _, track = ref.agent_obs(cfg, world, h, vo, pairs)
        exp = ref_step(cfg, world, h, aa, drv)
        h = {k: exp[k] for k in AGENT + ENV}
        reward, flags = ref.agent_outcomes(cfg, world, h, pairs, track)
        for b in count:
            count[b] += int(((flags & b) != 0).sum())
        respawns += int(exp["_done"].sum())
        e, a = pairs[:, 0], pairs[:, 1]
        assert not flags[(a == 0) | (e >= ac.B) | (a >= ac.A)].any() and not reward[(flags & _abi.AG_ENDED) != 0].any()
    assert all(count.values()) and respawns >= ac.B, count
