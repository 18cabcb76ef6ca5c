"""CPU checks of tde_score_plans and config.PlanRefine: the numpy restatement (tests/plan_set_ref.py) pinned to the planner's
(tests/planner_ref.py) before any GPU is seen, the inputs of the GPU tests proved meaningful by the restatement alone, the brake
tail's known answer, PlanRefine and its validation, tde_plan_set against the header, and the argument checks that need no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import plan_set_ref as S
from tests import planner_ref as R
from torchdriveenv_amd import _abi
from torchdriveenv_amd.config import Planner, PlanRefine, check_plan_refine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _lattice_seq(pl, B, K=1):
    lat = S.lattice(pl)
    return np.ascontiguousarray(np.broadcast_to(lat[None, :, None, :], (B, len(lat), K, 2)))


def _equals_planner_ref(cfg, world, hs, pl):
    B = len(hs["scn"])
    act, dg, f, cost = R.plan(cfg, world, hs, pl, detail=True)
    got = S.score(cfg, world, hs, pl, _lattice_seq(pl, B), pl.horizon, 0)
    assert np.array_equal(got["f"], f) and np.array_equal(_bits(got["cost"]), _bits(cost))
    assert np.array_equal(_bits(got["action"]), _bits(act))
    for n in dg.dtype.names:
        assert np.array_equal(got["diag"][n].view(np.uint32), dg[n].view(np.uint32)), n
    return f


def test_one_knot_no_tail_lattice_equals_planner_ref_on_junctions_with_lights(small_world):
    cfg = S.lights_cfg(small_world, seed=3)
    assert cfg.flags & _abi.F_TRAFFIC_LIGHTS
    hs = S.reset_state(cfg, small_world, 48)
    hs["steps"][...] = np.arange(48) * 7
    f = _equals_planner_ref(cfg, small_world, hs, Planner())
    assert (f <= 32).any() and (f == 33).any()
    # K constant knots and no tail: the same again (a constant sequence's steering term is d * d)
    got = S.score(cfg, small_world, hs, Planner(), _lattice_seq(Planner(), 48, K=4), 3, 0)
    assert np.array_equal(got["f"], f)


def test_one_knot_no_tail_lattice_equals_planner_ref_on_128_slots():
    from torchdriveenv_amd.synth import synthetic_world

    world = synthetic_world(n_scn=4, A=128, seed=5, n_maps=2)
    cfg = S.lights_cfg(world, seed=5)
    hs = S.reset_state(cfg, world, 6)
    hs["present"][...] = 1
    _equals_planner_ref(cfg, world, hs, Planner(horizon=20))


@pytest.mark.parametrize("name", list(S.CASES))
def test_the_gpu_tests_inputs_are_meaningful(small_world, name):
    """by the restatement alone: at least 10 % of the scored pairs are safe and 10 % fail, every cause is some pair's first failure
    (the red line on the lights inputs), and with a tail some pair fails inside it"""
    cfg, world, hs, pl, seq, knot_len, tail, only = S.case_inputs(name, small_world)
    c = S.CASES[name]
    assert seq.shape[1:] == (c["N"], c["K"], 2) and 1 <= c["N"] <= _abi.PLAN_MAX_SET
    got = S.score(cfg, world, hs, pl, seq, knot_len, tail, only=only)
    sel = np.ones(len(seq), bool) if only is None else only != 0
    assert sel.any() and (only is None or not sel.all())
    f, cause = got["f"][sel], got["cause"][sel]
    H, HT = pl.horizon, pl.horizon + tail
    print(name, "safe", np.mean(f == HT + 1), "fail", np.mean(f <= HT), "causes", [int((cause == k).sum()) for k in (1, 2, 3)],
          "in the tail", int(((f > H) & (f <= HT)).sum()))
    assert np.mean(f == HT + 1) >= 0.1 and np.mean(f <= HT) >= 0.1
    assert (cause == S.OFFROAD).any() and (cause == S.BOX).any()
    if c.get("lights"):
        assert (cause == S.RED).any()
        # the phase changes inside the window the case names
        from tests.vector_obs_ref import red_mask
        m = world.map_of_scn()[hs["scn"]]
        lo, hi = (1, H) if name.endswith("horizon") else (H + 1, HT)
        assert any(len({int(red_mask(world, m[e], int(hs["steps"][e]) + h)) for h in range(lo, hi + 1)}) > 1 for e in range(len(m)))
    if tail > 0:
        assert ((f > H) & (f <= HT)).any()
    last = min((H - 1) // knot_len, c["K"] - 1)
    if "cut" in name:
        assert last == c["K"] - 1 and c["K"] * knot_len > H           # the last knot is reached and H cuts it short
    if "stretched" in name:
        assert c["K"] * knot_len < H                                  # the last knot is held beyond its length
    if c.get("wild"):
        assert np.isnan(seq).any() and (np.abs(seq[..., 0]) > 1).any() and (np.abs(seq[..., 1]) > f32(0.3)).any()
        assert np.isfinite(got["cost"]).all()


def test_clamp_rule():
    cfg, world, st, pl, _ = S.tail_corridor()
    seq = np.array([[[[np.nan, np.nan]], [[-1.0, -0.3]], [[7.0, 0.5]], [[1.0, 0.3]]]], f32)
    got = S.score(cfg, world, st, pl, seq, 32, 10)
    assert _bits(got["cost"][0, 0]) == _bits(got["cost"][0, 1]) and got["f"][0, 0] == got["f"][0, 1]     # a NaN becomes the lower bound
    assert _bits(got["cost"][0, 2]) == _bits(got["cost"][0, 3]) and got["f"][0, 2] == got["f"][0, 3]


def test_brake_tail_known_answer():
    """coasting at 4 m/s covers 12.8 m in the horizon and needs 8 m more to stop; braking from the start needs 8 m: with the line's
    near edge 16 m ahead of the bumper the coasting sequence fails in the tail, the braking one is safe, and without a tail both are"""
    for near in (13.5, 16.0, 20.0):
        cfg, world, st, pl, seq = S.tail_corridor(near)
        H = pl.horizon
        for tail in (40, 64):
            got = S.score(cfg, world, st, pl, seq, H, tail)
            f = got["f"][0]
            assert H < f[0] <= H + tail and got["cause"][0, 0] == S.RED, (near, tail, f)
            assert f[1] == H + tail + 1, (near, tail, f)
            assert got["diag"]["winner"][0] == 1 and got["diag"]["n_safe"][0] == 1 and got["action"][0, 0] == -1
            # worse than any sequence that can be stopped, better than any that fails inside the horizon
            assert got["cost"][0, 1] < got["cost"][0, 0] < f32(tail + 1) * f32(_abi.PLAN_FAIL_UNIT)
        got = S.score(cfg, world, st, pl, seq, H, 0)
        assert (got["f"][0] == H + 1).all() and got["diag"]["winner"][0] == 0        # without the tail coasting looks fine, and wins
    # the line far enough to stop in front of it after the horizon: coasting is safe with the tail too
    cfg, world, st, pl, seq = S.tail_corridor(22.0)
    assert (S.score(cfg, world, st, pl, seq, pl.horizon, 64)["f"][0] == pl.horizon + 65).all()


def test_refinement_rounds_never_raise_the_winning_cost(small_world):
    cfg = S.lights_cfg(small_world, seed=9)
    hs = S.reset_state(cfg, small_world, 12)
    pl, pr = Planner(), PlanRefine()
    act, dg, costs = S.refine(cfg, small_world, hs, pl, pr)
    assert len(costs) == 3
    for a, b in zip(costs, costs[1:]):
        assert (R.ordered(_bits(b)) <= R.ordered(_bits(a))).all()
    assert (np.abs(act[:, 0]) <= 1).all() and (np.abs(act[:, 1]) <= f32(0.3)).all()
    # rounds = 0, tail = 0, knots = 1 is the plain planner
    a0, d0, _ = S.refine(cfg, small_world, hs, pl, PlanRefine(rounds=0, tail=0, knots=1))
    a1, d1 = R.plan(cfg, small_world, hs, pl)
    assert np.array_equal(_bits(a0), _bits(a1)) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))


def test_plan_refine_defaults_and_validation():
    pr = check_plan_refine(PlanRefine(), Planner())
    assert (pr.rounds, pr.knots, pr.tail, pr.shrink) == (2, 2, 40, 0.5)
    assert check_plan_refine(dict(rounds=1), Planner()).rounds == 1
    for bad in (dict(rounds=-1), dict(rounds=9), dict(rounds=1.5), dict(knots=0), dict(knots=33), dict(tail=-1), dict(tail=65),
                dict(shrink=0.0), dict(shrink=1.5), dict(shrink=float("nan")), dict(knots=17)):
        with pytest.raises(ValueError):
            check_plan_refine(PlanRefine(**bad), Planner())
    with pytest.raises(ValueError):
        check_plan_refine(PlanRefine(knots=8), Planner(horizon=4))
    with pytest.raises(TypeError):
        check_plan_refine(3, Planner())
    assert check_plan_refine(PlanRefine(knots=17, rounds=0), Planner()).knots == 17     # (no refinement round: no 1024 limit)


def test_struct_matches_header(tmp_path):
    c = tmp_path / "ps.c"
    names = ("seq", "N", "K", "knot_len", "tail")
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tde_hip.h"\nint main(void){printf("%zu", sizeof(tde_plan_set));' +
                 "".join(f'printf(" %zu", offsetof(tde_plan_set, {n}));' for n in names) +
                 'printf(" %d %d %d %g %g\\n", TDE_ABI_VERSION, TDE_PLAN_MAX_SET, TDE_PLAN_MAX_TAIL, TDE_PLAN_BOX_ACCEL, TDE_PLAN_BOX_STEER);'
                 ' return 0;}\n')
    exe = str(tmp_path / "ps")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    got = [float(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    T = _abi.TdePlanSet
    assert got[0] == C.sizeof(T) and got[1:6] == [getattr(T, n).offset for n in names]
    assert got[6:9] == [_abi.TDE_ABI_VERSION, _abi.PLAN_MAX_SET, _abi.PLAN_MAX_TAIL] and _abi.TDE_ABI_VERSION == 14
    assert f32(got[9]) == f32(_abi.PLAN_BOX_ACCEL) and f32(got[10]) == f32(_abi.PLAN_BOX_STEER)
    # every cost keeps the running cost's bits apart
    assert (_abi.PLAN_MAX_H + _abi.PLAN_MAX_TAIL) * _abi.PLAN_FAIL_UNIT + _abi.PLAN_RUN_MAX < 2 ** 24


def test_library_rejects_bad_arguments():
    """the entry point's own checks (before any launch: no GPU needed)"""
    from torchdriveenv_amd import _lib, ops
    from torchdriveenv_amd.state import EnvState
    from torchdriveenv_amd.synth import synthetic_world

    L = _lib.load()
    assert "tde_score_plans" in _lib.SYMBOLS
    w = synthetic_world(n_scn=2, A=8, seed=0, n_maps=1)
    st = EnvState(4, 8)
    cfg = _abi.default_config(seed=1)
    seq = np.zeros((4, 3, 2, 2), f32)
    cost, fail = np.zeros((4, 3), f32), np.zeros((4, 3), np.int32)

    def call(pl=None, cost_p=cost.ctypes.data, fail_p=fail.ctypes.data, null_set=False, **over):
        ps = _abi.TdePlanSet(seq.ctypes.data, 3, 2, 16, 0)
        for k, v in over.items():
            setattr(ps, k, v)
        pl = pl if pl is not None else ops.planner_struct(Planner())
        return L.tde_score_plans(C.byref(cfg), C.byref(w.host_struct()), C.byref(st.struct), C.byref(pl), None if null_set else C.byref(ps),
                                 None, cost_p, fail_p, None, None, None)

    for over, msg in ((dict(N=0), b"N must"), (dict(N=1025), b"N must"), (dict(K=0), b"K must"), (dict(K=33), b"K must"),
                      (dict(knot_len=0), b"knot_len"), (dict(tail=-1), b"tail"), (dict(tail=65), b"tail"), (dict(seq=None), b"NULL")):
        assert call(**over) != 0 and msg in L.tde_last_error(), over
    assert call(cost_p=None) != 0 and b"NULL" in L.tde_last_error()
    assert call(fail_p=None) != 0 and b"NULL" in L.tde_last_error()
    assert call(null_set=True) != 0 and b"NULL" in L.tde_last_error()
    for k, v, msg in (("horizon", 0, b"horizon"), ("horizon", 33, b"horizon"), ("margin", float("inf"), b"finite"),
                      ("w_speed", float("nan"), b"finite"), ("v_target", -1.0, b"finite")):
        pl = ops.planner_struct(Planner())
        setattr(pl, k, v)
        assert call(pl=pl) != 0 and msg in L.tde_last_error(), k
    # the lattice is not read: an empty one is no error of this entry point (a B = 0 state returns before any launch)
    st0 = EnvState(4, 8)
    st0.struct.B = 0
    pl = ops.planner_struct(Planner())
    pl.n_a = 0
    ps = _abi.TdePlanSet(seq.ctypes.data, 3, 2, 16, 0)
    assert L.tde_score_plans(C.byref(cfg), C.byref(w.host_struct()), C.byref(st0.struct), C.byref(pl), C.byref(ps), None, cost.ctypes.data,
                             fail.ctypes.data, None, None, None) == 0


# What each entry point of the planner / forecast family refuses as NULL, name by name (written from the entry points' checks; the
# library's own grouping is "what the judge reads" and "what the scene controller reads").  `free`: a pointer it does not ask for.
_JUDGE_STATE = ("x", "y", "psi", "v", "len", "wid", "lr", "present", "scn", "steps", "target_idx")
_SCENE_STATE = ("x", "y", "psi", "v", "len", "wid", "lr", "vdes", "route_wp", "present", "scn", "steps")
_JUDGE_WORLD = ("maps", "scn", "wp_xy", "cell_word", "cell_cls2", "cell_coarse", "cell_tri")
_REQUIRED = {
    "tde_plan_action": dict(state=_JUDGE_STATE, world=_JUDGE_WORLD, free=("vdes", "route_wp"), wfree=("spawn", "route_xy", "replay_states")),
    "tde_score_plans": dict(state=_JUDGE_STATE, world=_JUDGE_WORLD, free=("vdes", "route_wp"), wfree=("spawn", "route_xy", "replay_states")),
    "tde_score_plans_forecast": dict(state=_JUDGE_STATE, world=_JUDGE_WORLD, free=("vdes", "route_wp"),
                                     wfree=("spawn", "route_xy", "replay_states")),
    # (world.maps: not without lights)
    "tde_forecast_agents": dict(state=_SCENE_STATE, world=("spawn", "scn"), free=("target_idx",), wfree=("maps", "wp_xy", "cell_word"),
                                routes=True),
    # (world.maps: under lights or the offroad flag, which the default flags hold)
    "tde_forecast_scene": dict(state=_SCENE_STATE, world=("spawn", "scn", "maps"), free=("target_idx",), wfree=("wp_xy", "cell_word"),
                               routes=True),
    "tde_score_plans_scene": dict(state=_SCENE_STATE + ("target_idx",), world=_JUDGE_WORLD + ("spawn",), free=("reached", "collided"),
                                  wfree=("tri", "start_psi"), routes=True),
}


def test_every_planner_and_forecast_entry_point_holds_the_shared_checks():
    """the checks the family shares, held to all callers at once: the same bad plan set, planner and dt are refused by each entry
    point that takes them, under its own name; each required pointer is, one at a time; one it does not ask for is not.  Every call
    is on an empty batch (B = 0): a refusal comes before that return, and a check that let something through launches nothing."""
    from torchdriveenv_amd import _lib, ops
    from torchdriveenv_amd.state import EnvState
    from torchdriveenv_amd.synth import synthetic_world

    L = _lib.load()
    w = synthetic_world(n_scn=2, A=8, seed=0, n_maps=1)
    good_cfg = _abi.default_config(seed=1)
    assert good_cfg.flags & _abi.F_NPC and good_cfg.flags & _abi.F_REPLAY and good_cfg.flags & _abi.F_OFFROAD
    assert not good_cfg.flags & _abi.F_TRAFFIC_LIGHTS
    seq = np.zeros((4, 3, 2, 2), f32)
    cost, fail = np.zeros((4, 3), f32), np.zeros((4, 3), np.int32)
    out, act = np.zeros((4, 96, 8, 4), f32), np.zeros((4, 2), f32)

    def state(null=None):
        st = EnvState(4, 8)
        st.struct.B = 0
        if null is not None:
            assert getattr(st.struct, null) is not None
            setattr(st.struct, null, None)
        return st

    def world(null=None):
        ws = _abi.TdeWorld.from_buffer_copy(w.host_struct())
        if null is not None:
            assert getattr(ws, null) is not None
            setattr(ws, null, None)
        return ws

    def call(name, cfg=good_cfg, st=None, ws=None, pl=None, **over):
        st, ws = st if st is not None else state(), ws if ws is not None else world()
        pl = pl if pl is not None else ops.planner_struct(Planner())
        ps = _abi.TdePlanSet(seq.ctypes.data, 3, 2, 16, 0)
        for k, v in over.items():
            setattr(ps, k, v)
        a = (C.byref(cfg), C.byref(ws), C.byref(st.struct))
        judged = (C.byref(pl), C.byref(ps), None, cost.ctypes.data, fail.ctypes.data, None, None)
        if name == "tde_plan_action":
            return L.tde_plan_action(*a, C.byref(pl), None, act.ctypes.data, None, None)
        if name == "tde_score_plans":
            return L.tde_score_plans(*a, *judged, None)
        if name == "tde_score_plans_forecast":
            return L.tde_score_plans_forecast(*a, *judged, out.ctypes.data, 96, None)
        if name == "tde_score_plans_scene":
            return L.tde_score_plans_scene(*a, *judged, None)
        if name == "tde_forecast_agents":
            return L.tde_forecast_agents(*a, 8, None, out.ctypes.data, None)
        assert name == "tde_forecast_scene"
        return L.tde_forecast_scene(*a, 8, None, None, out.ctypes.data, None)

    def refused(name, fragment, **kw):
        rc, err = call(name, **kw), L.tde_last_error()
        assert rc != 0 and fragment in err and name.encode() + b":" in err, (name, fragment, sorted(kw), rc, err)

    def planner(**over):
        pl = ops.planner_struct(Planner())
        for k, v in over.items():
            setattr(pl, k, v)
        return pl

    assert sorted(_REQUIRED) == sorted(n for n in _lib.SYMBOLS if n.startswith(("tde_plan_", "tde_score_plans", "tde_forecast_")))
    for name in _REQUIRED:
        assert call(name) == 0, (name, L.tde_last_error())                # the good arguments, empty batch
    # one plan set, one planner
    for name in ("tde_score_plans", "tde_score_plans_forecast", "tde_score_plans_scene"):
        for over, msg in ((dict(N=0), b"N must be in [1, TDE_PLAN_MAX_SET]"), (dict(K=33), b"K must be in [1, TDE_PLAN_MAX_H]"),
                          (dict(knot_len=0), b"knot_len must be >= 1"), (dict(tail=65), b"tail must be in [0, TDE_PLAN_MAX_TAIL]")):
            refused(name, msg, **over)
    for name in ("tde_plan_action", "tde_score_plans", "tde_score_plans_forecast", "tde_score_plans_scene"):
        refused(name, b"horizon must be in [1, TDE_PLAN_MAX_H]", pl=planner(horizon=0))
        refused(name, b"v_target, margin and the weights must be finite and >= 0", pl=planner(margin=-0.1))
    # one dt, the lights' tables, the controller's routes and records
    lights = _abi.default_config(seed=1, flags=good_cfg.flags | _abi.F_TRAFFIC_LIGHTS)
    for name, req in _REQUIRED.items():
        for dt in (0.0, float("nan")):
            refused(name, b"config.dt must be finite and > 0", cfg=_abi.default_config(seed=1, dt=dt))
        for tab in ("stoplines", "phases"):
            assert call(name, ws=world(tab)) == 0, (name, tab)
            refused(name, b"TDE_F_TRAFFIC_LIGHTS without stop lines / phases", cfg=lights, ws=world(tab))
        for tab, count, flag in (("route_xy", "n_routes", _abi.F_NPC), ("replay_states", "n_replay", _abi.F_REPLAY)):
            assert w.ints[count] > 0
            if req.get("routes"):
                refused(name, b"world." + tab.encode() + b" is NULL", ws=world(tab))
                assert call(name, cfg=_abi.default_config(seed=1, flags=good_cfg.flags & ~flag), ws=world(tab)) == 0, (name, tab)
                none = world(tab)
                setattr(none, count, 0)
                assert call(name, ws=none) == 0, (name, tab)
    refused("tde_forecast_agents", b"TDE_F_TRAFFIC_LIGHTS without stop lines / phases", cfg=lights, ws=world("maps"))
    assert call("tde_forecast_scene", cfg=_abi.default_config(seed=1, flags=good_cfg.flags & ~_abi.F_OFFROAD), ws=world("maps")) == 0
    # the pointer lists, name by name
    for name, req in _REQUIRED.items():
        for p in req["state"]:
            refused(name, b"pointer is NULL", st=state(p))
        for p in req["world"]:
            refused(name, b"world.maps is NULL" if (name, p) == ("tde_forecast_scene", "maps") else b"pointer is NULL", ws=world(p))
        for p in req["free"]:
            assert call(name, st=state(p)) == 0, (name, p, L.tde_last_error())
        for p in req["wfree"]:
            assert call(name, ws=world(p)) == 0, (name, p, L.tde_last_error())


def test_sequence_tensor_checks_need_no_gpu():
    import torch

    from torchdriveenv_amd import ops

    seq = torch.zeros((4, 6, 2, 2), dtype=torch.float32)
    assert ops.check_plan_set(seq, 4, 32) == (6, 2, 16, 0)
    assert ops.check_plan_set(seq, 4, 31, tail=64) == (6, 2, 16, 64) and ops.check_plan_set(seq, 4, 32, knot_len=3) == (6, 2, 3, 0)
    for bad, kw in ((seq.permute(0, 2, 1, 3), {}), (torch.zeros((4, 6, 2, 4))[..., ::2], {}), (seq.double(), {}), (seq[:3], {}),
                    (torch.zeros((4, 6, 2, 3)), {}), (torch.zeros((4, 1025, 1, 2)), {}), (torch.zeros((4, 2, 33, 2)), {}),
                    (torch.zeros((4, 0, 1, 2)), {}), (seq, dict(knot_len=0)), (seq, dict(tail=65)), (seq, dict(tail=-1)),
                    (seq, dict(knot_len=1.5)), (seq.numpy(), {})):
        with pytest.raises(ValueError):
            ops.check_plan_set(bad, 4, 32, **kw)
