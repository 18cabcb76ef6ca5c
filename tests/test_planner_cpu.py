"""CPU checks of the sampling planner (tde_plan_action): config.Planner and its validation, tde_planner / tde_plan_diag against the
header, the library's own argument checks (they return before any launch), known answers of the numpy restatement
(tests/planner_ref.py) that the GPU tests hold the kernel against, and a small closed loop of the restatement with the oracle's
step."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests import planner_ref as R
from torchdriveenv_amd import _abi
from torchdriveenv_amd.config import Planner, check_planner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_defaults_hold_zero_and_fit_a_wavefront():
    pl = check_planner(Planner())
    a, s = pl.tables()
    assert a.dtype == np.float32 and s.dtype == np.float32 and len(a) == 9 and len(s) == 7 and pl.n_candidates == 63 <= 64
    assert (a == 0).sum() == 1 and (s == 0).sum() == 1 and a.min() == -1 and a.max() == 1 and s.min() == f32(-0.3) and s.max() == f32(0.3)
    assert 1 <= pl.horizon <= 32
    assert pl.candidate(3 * 7 + 2) == (a[3], s[2])
    assert check_planner(dict(horizon=5)).horizon == 5


@pytest.mark.parametrize("bad", [dict(accelerations=(0.0, 1.5)), dict(accelerations=(-1.01, 0.0)), dict(steerings=(0.0, 0.31)),
                                 dict(steerings=(0.0, float("nan"))), dict(accelerations=(0.5, 1.0)), dict(steerings=(0.1, 0.2)),
                                 dict(accelerations=()), dict(accelerations=tuple(np.linspace(-1, 1, 11)) + (0.0,)),
                                 dict(horizon=0), dict(horizon=33), dict(horizon=2.5), dict(v_target=-1.0), dict(margin=float("inf")),
                                 dict(w_steer=-0.1), dict(w_progress=float("nan"))])
def test_validation_rejects(bad):
    with pytest.raises(ValueError):
        check_planner(Planner(**bad))


def test_structs_match_header(tmp_path):
    c = tmp_path / "pl.c"
    names = ("accel", "steer", "n_a", "n_s", "horizon", "v_target", "margin", "w_progress", "w_speed", "w_steer")
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tde_hip.h"\nint main(void){printf("%zu %zu", sizeof(tde_planner), '
                 'sizeof(tde_plan_diag));' + "".join(f'printf(" %zu", offsetof(tde_planner, {n}));' for n in names) +
                 "".join(f'printf(" %zu", offsetof(tde_plan_diag, {n}));' for n in ("winner", "fail_step", "cost", "n_safe")) +
                 'printf(" %d %d %d %g %g %g\\n", TDE_ABI_VERSION, TDE_PLAN_MAX_CAND, TDE_PLAN_MAX_H, TDE_PLAN_FAIL_UNIT, TDE_PLAN_RUN_MAX, '
                 'TDE_PLAN_RUN_BIAS); return 0;}\n')
    exe = str(tmp_path / "pl")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    got = [float(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    S, D = _abi.TdePlanner, _abi.PLAN_DIAG_DTYPE
    assert got[:2] == [C.sizeof(S), D.itemsize]
    assert got[2:12] == [getattr(S, n).offset for n in names]
    assert got[12:16] == [D.fields[n][1] for n in ("winner", "fail_step", "cost", "n_safe")]
    assert got[16:] == [_abi.TDE_ABI_VERSION, _abi.PLAN_MAX_CAND, _abi.PLAN_MAX_H, _abi.PLAN_FAIL_UNIT, _abi.PLAN_RUN_MAX, _abi.PLAN_RUN_BIAS]
    assert _abi.PLAN_MAX_H * _abi.PLAN_FAIL_UNIT + _abi.PLAN_RUN_MAX < 2 ** 24     # every cost keeps the running cost's bits apart
    assert _abi.PLAN_RUN_MAX < _abi.PLAN_FAIL_UNIT                               # an earlier failure always costs more


def test_library_rejects_bad_arguments():
    """the entry point's own checks (before any launch: no GPU needed)"""
    from torchdriveenv_amd import _lib, ops
    from torchdriveenv_amd.state import EnvState
    from torchdriveenv_amd.synth import synthetic_world

    L = _lib.load()
    w = synthetic_world(n_scn=2, A=8, seed=0, n_maps=1)
    st = EnvState(4, 8)
    cfg = _abi.default_config(seed=1)
    out = np.zeros((4, 2), np.float32)

    def call(pl, cfg=cfg, out_p=out.ctypes.data):
        return L.tde_plan_action(C.byref(cfg), C.byref(w.host_struct()), C.byref(st.struct), C.byref(pl) if pl is not None else None,
                                 None, out_p, None, None)

    def made(**over):
        t = ops.planner_struct(Planner())
        for k, v in over.items():
            if k in ("accel", "steer"):
                getattr(t, k)[v[0]] = v[1]
            else:
                setattr(t, k, v)
        return t

    for over, msg in ((dict(n_a=0), b"n_a"), (dict(n_s=0), b"n_a"), (dict(n_a=10), b"n_a"), (dict(n_a=65, n_s=1), b"n_a"),
                      (dict(horizon=0), b"horizon"), (dict(horizon=33), b"horizon"), (dict(accel=(2, 1.25)), b"acceleration"),
                      (dict(accel=(0, float("nan"))), b"acceleration"), (dict(steer=(6, 0.31)), b"steering"),
                      (dict(steer=(1, -0.5)), b"steering"), (dict(v_target=-1.0), b"finite"), (dict(margin=float("inf")), b"finite"),
                      (dict(w_speed=float("nan")), b"finite")):
        assert call(made(**over)) != 0 and msg in L.tde_last_error(), over
    assert call(None) != 0 and b"NULL" in L.tde_last_error()
    assert call(made(), out_p=None) != 0 and b"NULL" in L.tde_last_error()
    c0 = _abi.default_config(seed=1)
    c0.dt = 0.0
    assert call(made(), cfg=c0) != 0 and b"dt" in L.tde_last_error()


def test_array_overlap_is_the_oracles():
    rng = np.random.default_rng(0)
    n = 4000
    b = rng.uniform(-4, 4, (n, 2, 2)).astype(f32)
    ang = rng.uniform(-3.2, 3.2, (n, 2)).astype(f32)
    s, c = oracle.sincosf(ang.ravel())
    s, c = s.reshape(n, 2), c.reshape(n, 2)
    h = rng.uniform(0.2, 3.0, (n, 2, 2)).astype(f32)
    got = R.obb_overlap(b[:, 0, 0], b[:, 0, 1], c[:, 0], s[:, 0], h[:, 0, 0], h[:, 0, 1], b[:, 1, 0], b[:, 1, 1], c[:, 1], s[:, 1],
                        h[:, 1, 0], h[:, 1, 1])
    want = [oracle.obb_overlap((b[i, 0, 0], b[i, 0, 1], c[i, 0], s[i, 0], h[i, 0, 0], h[i, 0, 1]),
                               (b[i, 1, 0], b[i, 1, 1], c[i, 1], s[i, 1], h[i, 1, 0], h[i, 1, 1])) != 0 for i in range(n)]
    assert np.array_equal(got, np.array(want)) and 0.1 < got.mean() < 0.9


# ---- known answers of the restatement -------------------------------------------------------------------------------------------------


def _world(polyline, waypoints, A=8, lights=None, width=12.0):
    from torchdriveenv_amd.world import assemble_world, corridor_mesh

    mesh = corridor_mesh([polyline], width=width)
    scn = dict(map=0, waypoints=waypoints, start_heading=0.0, agents=[], ego_attr=(4.5, 2.0, 1.5))
    return assemble_world([mesh], [scn], A, threshold=0.5, cell=0.25, lights=lights)


def _corridor(lights=None):
    return _world([(0.0, 0.0), (200.0, 0.0)], [(150.0, 0.0), (190.0, 0.0)], lights=lights)


FREE = 15      # candidates of the default lattice that stay on the empty 12 m corridor for the default horizon from 4 m/s


def _state(B, A, x=100.0, v=4.0):
    from torchdriveenv_amd.state import EnvState

    st = EnvState(B, A)
    for k in ("x", "y", "psi", "v"):
        st[k][...] = 0
    st["len"][...] = 4.5
    st["wid"][...] = 2.0
    st["lr"][...] = 1.5
    st["present"][...] = 0
    st["present"][::A] = 1
    st["x"][::A] = x
    st["v"][::A] = v
    st["scn"][...] = 0
    st["steps"][...] = 0
    st["target_idx"][...] = 0
    return st


def test_straight_corridor_at_target_speed_keeps_the_wheel_straight():
    world, cfg, pl = _corridor(), _abi.default_config(seed=1), Planner()
    st = _state(1, 8, v=pl.v_target)
    act, dg, f, cost = R.plan(cfg, world, st, pl, detail=True)
    a, d = pl.candidate(dg["winner"][0])
    assert d == 0 and act[0, 1] == 0 and act[0, 0] == a
    _, ste = pl.tables()
    straight = ste[np.arange(63) % 7] == 0
    assert dg["fail_step"][0] == pl.horizon + 1 and (f[0][straight] == pl.horizon + 1).all()
    assert dg["n_safe"][0] == (f[0] == pl.horizon + 1).sum() == FREE   # (held steering leaves the 12 m corridor within the horizon)
    assert dg["cost"][0] == cost[0].min() and abs(a) <= 0.25
    # slower than the target: the plan accelerates; a finished route plans a stop
    st["v"][0] = 1.0
    assert R.plan(cfg, world, st, pl)[0][0, 0] > 0
    st["v"][0] = 4.0
    st["target_idx"][0] = 2
    assert R.plan(cfg, world, st, pl)[0][0, 0] == -1
    # standing with a finished route: the no-reverse rule turns every braking candidate's first action into 0
    st["v"][0] = 0.0
    act, dg = R.plan(cfg, world, st, pl)
    assert act[0, 0] == 0 and act[0, 1] == 0


def test_a_parked_car_across_the_lane_makes_the_plan_brake_hardest():
    world, cfg, pl = _corridor(), _abi.default_config(seed=1), Planner()
    st = _state(1, 8, v=4.0)
    st["present"][1], st["x"][1], st["psi"][1] = 1, 108.0, np.pi / 2
    act, dg, f, cost = R.plan(cfg, world, st, pl, detail=True)
    acc, ste = pl.tables()
    ia = np.arange(63) // 7
    assert (f[0][acc[ia] >= 0] <= pl.horizon).all()                  # every non-braking candidate fails
    assert dg["n_safe"][0] == 0 and (f[0] <= pl.horizon).all()       # here the braking ones do too: no safe plan ...
    assert act[0, 0] == -1 and dg["fail_step"][0] == f[0].max()      # ... and the one that fails last brakes hardest
    assert (cost[0][f[0] < f[0].max()] > dg["cost"][0]).all()
    # the car far ahead: nothing fails
    st["x"][1] = 160.0
    assert R.plan(cfg, world, st, pl)[1]["n_safe"][0] == FREE


def test_a_red_line_brakes_and_a_green_one_does_not():
    lt = [dict(stoplines=[(108.0, 0.0, 0.0, 2.0, 9.0, 0)], phases=[(40, [0]), (40, [])])]
    world, pl = _corridor(lights=lt), Planner()
    cfg = _abi.default_config(seed=1)
    cfg.flags |= _abi.F_TRAFFIC_LIGHTS
    st = _state(2, 8, v=4.0)
    st["steps"][0], st["steps"][1] = 0, 40                            # env 0: red through the horizon; env 1: green through it
    act, dg, f, cost = R.plan(cfg, world, st, pl, detail=True)
    acc, _ = pl.tables()
    assert (f[0][acc[np.arange(63) // 7] >= 0] <= pl.horizon).all()
    assert act[0, 0] == -1 and dg["fail_step"][0] == f[0].max()
    assert dg["n_safe"][1] == FREE and act[1, 0] >= 0 and act[1, 1] == 0
    # the phase turns green inside the horizon: crossing after the change is allowed (the line is 4.75 m ahead of the bumper)
    st["steps"][0] = 35
    act, dg = R.plan(cfg, world, st, pl)
    assert dg["n_safe"][0] > 0 and dg["fail_step"][0] == pl.horizon + 1
    # without the flag the line is not there
    cfg.flags &= ~_abi.F_TRAFFIC_LIGHTS
    st["steps"][0] = 0
    assert R.plan(cfg, world, st, pl)[1]["n_safe"][0] == FREE


def test_a_bend_is_steered_into():
    R_, n = 20.0, 40
    for sign in (1.0, -1.0):
        arc = [(-30.0, 0.0), (0.0, 0.0)] + [(R_ * np.sin(t), sign * R_ * (1 - np.cos(t))) for t in np.linspace(0, np.pi / 2, n)[1:]]
        world = _world(arc, [(R_, sign * R_), (R_, sign * (R_ + 5.0))], width=6.0)
        cfg, pl = _abi.default_config(seed=1), Planner()
        st = _state(1, 8, x=0.0, v=4.0)
        act, dg, f, cost = R.plan(cfg, world, st, pl, detail=True)
        assert act[0, 1] * sign > 0, (sign, act, dg)
        _, ste = pl.tables()
        assert (f[0][ste[np.arange(63) % 7] * sign < 0] <= pl.horizon).all()    # steering away from the bend leaves the road


def test_exact_ties_go_to_the_lower_index_and_horizon_one():
    world, cfg = _corridor(), _abi.default_config(seed=1)
    pl = Planner(accelerations=(0.0, 0.0, 0.0), steerings=(0.0,), horizon=1)
    st = _state(1, 8)
    act, dg, f, cost = R.plan(cfg, world, st, pl, detail=True)
    assert cost[0, 0] == cost[0, 1] == cost[0, 2] and dg["winner"][0] == 0
    # off the road already: every candidate fails at step one, the tie still goes to index 0
    st["y"][0] = 30.0
    act, dg, f, cost = R.plan(cfg, world, st, pl, detail=True)
    assert (f == 1).all() and dg["winner"][0] == 0 and dg["n_safe"][0] == 0 and dg["fail_step"][0] == 1
    assert dg["cost"][0] == f32(_abi.PLAN_FAIL_UNIT) + f32(_abi.PLAN_RUN_BIAS)


def test_only_mask_keeps_rows():
    world, cfg, pl = _corridor(), _abi.default_config(seed=1), Planner(horizon=4)
    st = _state(3, 8)
    prev = np.full((3, 2), 7.0, f32)
    act, dg = R.plan(cfg, world, st, pl, only=np.array([0, 1, 0], np.uint8), out=prev)
    assert (act[[0, 2]] == 7.0).all() and (act[1] != 7.0).all() and dg["n_safe"][1] > 0 and dg["n_safe"][0] == 0


def _closed_loop(world, cfg, B, T, policy):
    """B envs for T steps of the oracle's step with auto-reset -> (episodes, ended by infraction, waypoints reached)"""
    from torchdriveenv_amd.state import EnvState

    hs = EnvState(B, world.A)
    oracle.env_reset(cfg, world, hs)
    ep = inf = wps = 0
    for t in range(T):
        hs["action"][...] = policy(hs, t)
        reached = hs["reached"].copy()
        oracle.env_step(cfg, world, hs)
        term, trunc = hs["terminated"] != 0, hs["truncated"] != 0
        ep += int((term | trunc).sum())
        inf += int(term.sum())
        wps += int(np.maximum(hs["info_reached"] - reached, 0).sum()) if hs["info_reached"] is not None else 0
    return ep, inf, wps


def test_closed_loop_of_the_restatement_outdrives_the_zero_policy():
    """the restatement drives the oracle's env: fewer episodes ended by an infraction than the zero action, on a world where the
    zero action ends most of its episodes that way (the world the GPU behaviour test uses, at a size that runs in under a minute)"""
    from torchdriveenv_amd.synth import synthetic_world

    world = synthetic_world(n_scn=4, A=16, seed=0, n_maps=2)
    cfg = _abi.default_config(seed=5, distance_cutoff=0.25)
    if world.has_lights:
        cfg.flags |= _abi.F_TRAFFIC_LIGHTS
    B, T = 12, 100
    pl = Planner()
    zero = _closed_loop(world, cfg, B, T, lambda hs, t: 0.0)
    plan = _closed_loop(world, cfg, B, T, lambda hs, t: R.plan(cfg, world, hs, pl)[0])
    print("zero (episodes, infractions, waypoints):", zero, " planner:", plan)
    assert zero[1] >= 0.5 * max(zero[0], 1) and zero[1] > 0
    assert plan[1] < zero[1]
