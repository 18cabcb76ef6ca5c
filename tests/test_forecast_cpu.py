"""CPU checks of tde_forecast_agents and tde_score_plans_forecast: known answers of the numpy restatement (tests/forecast_ref.py; the
judge: plan_set_ref.score(forecast=)), the restatement held against the C oracle's step on a hand-made world in which no agent ever
enters another's cone (the environment is the oracle: bit for bit, every step), the judge's forecast branch on a constant-velocity
forecast giving its line branch's bits, the new prototypes and constants against the header, and the argument checks that need no
GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests import forecast_ref as Fr
from tests import plan_set_ref as S
from torchdriveenv_amd import _abi
from torchdriveenv_amd.config import Planner, check_planner
from torchdriveenv_amd.state import EnvState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _reset(cfg, world, B=Fr.ORACLE_B):
    hs = EnvState(B, world.A)
    hs["episode"][...] = 0
    oracle.env_reset(cfg, world, hs)
    return hs


@pytest.fixture(scope="module")
def hand_world():
    return Fr.oracle_world()


def test_environment_is_the_oracle(hand_world):
    """32 steps of the C oracle (zero ego action, no auto-reset, no termination at an infraction): after step h the slots >= 1 hold
    the forecast's row h, bit for bit"""
    cfg, world = hand_world
    hs = _reset(cfg, world)
    assert set(hs["scn"].tolist()) == {0, 1, 2, 3}                      # every scenario is drawn: lights, a short route, no route
    assert not (cfg.flags & _abi.F_AUTORESET) and cfg.terminated_at_infraction == 0
    fc = Fr.forecast(cfg, world, hs, Fr.ORACLE_STEPS)
    assert not fc[:, :, 0].any() and fc[:, :, 1:, 3].all()
    hs["action"][...] = 0
    B, A = Fr.ORACLE_B, world.A
    wp0 = hs["route_wp"].copy()
    for h in range(1, Fr.ORACLE_STEPS + 1):
        oracle.env_step(cfg, world, hs)
        got = np.stack([hs[n].reshape(B, A) for n in ("x", "y", "psi", "v")], -1)[:, 1:]
        bad = np.argwhere(_bits(got) != _bits(fc[:, h - 1, 1:]))
        assert len(bad) == 0, (h, bad[:4].tolist(), got[tuple(bad[0][:2])], fc[:, h - 1, 1:][tuple(bad[0][:2])])
    assert (hs["steps"] == Fr.ORACLE_STEPS).all()
    assert (hs["route_wp"] > wp0).any()                                 # route targets advanced inside the run


def test_replayed_slot_follows_its_record_then_the_bicycle(hand_world):
    cfg0, world = hand_world
    cfg = _abi.default_config(seed=11, terminated_at_infraction=0)
    cfg.flags = _abi.F_REPLAY | _abi.F_OFFROAD | _abi.F_REWARD          # no controller: after the record the slot coasts
    hs = _reset(cfg, world)
    fc = Fr.forecast(cfg, world, hs, 20)
    rec = world.arrays["spawn"].reshape(-1, world.A)[hs["scn"], 3]
    assert (rec["replay"] >= 0).all() and (rec["replay_len"] == 11).all()
    rows = world.arrays["replay_states"].reshape(-1, world.ints["RT"], 4)[rec["replay"]]
    assert np.array_equal(_bits(fc[:, :10, 3]), _bits(rows[:, 1:11]))
    x, y, psi, v = (np.ascontiguousarray(fc[:, 9, 3, i]) for i in range(4))
    lr = np.ascontiguousarray(hs["lr"].reshape(-1, world.A)[:, 3])
    for h in range(11, 21):
        oracle.kinematics_step(x, y, psi, v, lr, np.ones(len(x), np.uint8), np.zeros((len(x), 2), f32), float(cfg.dt))
        assert np.array_equal(_bits(np.stack([x, y, psi, v], -1)), _bits(fc[:, h - 1, 3])), h
    # a state in the middle of the record: the rows go on from steps + 1
    hs["steps"][...] = 6
    fc = Fr.forecast(cfg, world, hs, 8)
    assert np.array_equal(_bits(fc[:, :4, 3]), _bits(rows[:, 7:11])) and not np.array_equal(_bits(fc[:, 4, 3]), _bits(rows[:, 10]))


def test_finished_route_brakes_to_rest(hand_world):
    cfg, world = hand_world
    hs = _reset(cfg, world)
    fc = Fr.forecast(cfg, world, hs, 96)
    e = np.flatnonzero(hs["scn"] == 1)
    assert len(e)
    v = fc[e, :, 2, 3]
    assert (v[:, 0] > 5.0).all() and (v[:, -1] < 1e-6).all() and (np.diff(v[:, 12:], axis=1) <= 0).all()
    assert np.abs(fc[e, -1, 2, 0] - fc[e, -11, 2, 0]).max() < 1e-4      # ... and stays
    e2 = np.flatnonzero(hs["scn"] == 2)                                 # no route at all: brakes from the first controlled step
    assert (fc[e2, -1, 2, 3] < 1e-6).all()


def test_red_line_stops_the_npc_and_green_releases_it():
    cfg, world = Fr.oracle_world(red_steps=400)
    hs = _reset(cfg, world)
    e = np.flatnonzero(hs["scn"] == 3)
    assert len(e)
    fc = Fr.forecast(cfg, world, hs, 96)
    x, v = fc[e, :, 1, 0], fc[e, :, 1, 3]
    hl = 0.5 * hs["len"].reshape(-1, world.A)[e, 1]
    assert (v[:, -1] < 0.2).all() and (v[:, -1] < v[:, 5]).all()        # the speed falls ...
    assert (x[:, -1] + hl < Fr.STOP_X).all() and (x[:, -1] + hl > Fr.STOP_X - 3.0).all()    # ... and the bumper stops short of the line
    free = np.flatnonzero(hs["scn"] == 0)                               # the same road without the line: drives on
    assert (fc[free, -1, 1, 0] > Fr.STOP_X + 10.0).all()
    # green from step h0 = 61 on: it moves again
    cfg2, world2 = Fr.oracle_world(red_steps=61)
    hs2 = _reset(cfg2, world2)
    assert np.array_equal(hs2["scn"], hs["scn"])
    fc2 = Fr.forecast(cfg2, world2, hs2, 96)
    assert np.array_equal(_bits(fc2[e, :59]), _bits(fc[e, :59]))        # (the decision at step k reads the lights of step k)
    v2 = fc2[e, :, 1, 3]
    assert (v2[:, 58] < 2.0).all() and (v2[:, -1] > v2[:, 58] + 3.0).all() and (fc2[e, -1, 1, 0] > fc[e, -1, 1, 0] + 5.0).all()


def test_first_step_rule_and_only_mask(hand_world):
    cfg, world = hand_world
    hs = _reset(cfg, world)
    cfg1 = _abi.default_config(seed=11, terminated_at_infraction=0)
    cfg1.flags = cfg.flags & ~_abi.F_NPC_FIRST_STEP
    a, b = Fr.forecast(cfg, world, hs, 4), Fr.forecast(cfg1, world, hs, 4)
    lr = hs["lr"].reshape(-1, world.A)
    x, y, psi, v = (np.ascontiguousarray(hs[n].reshape(-1, world.A)[:, 1]) for n in ("x", "y", "psi", "v"))
    oracle.kinematics_step(x, y, psi, v, np.ascontiguousarray(lr[:, 1]), np.ones(len(x), np.uint8), np.zeros((len(x), 2), f32), 0.1)
    assert np.array_equal(_bits(b[:, 0, 1]), _bits(np.stack([x, y, psi, v], -1))) and not np.array_equal(_bits(a[:, 0, 1]), _bits(b[:, 0, 1]))
    hs["steps"][...] = 1                                                 # past the first step the flag changes nothing
    assert np.array_equal(_bits(Fr.forecast(cfg, world, hs, 4)), _bits(Fr.forecast(cfg1, world, hs, 4)))
    only = np.array([1, 0, 1, 0, 0, 1, 1, 0], np.uint8)
    pre = np.full((Fr.ORACLE_B, 4, world.A, 4), -7.0, f32)
    got = Fr.forecast(cfg, world, hs, 4, only=only, out=pre)
    full = Fr.forecast(cfg, world, hs, 4)
    assert (got[only == 0] == -7.0).all() and np.array_equal(_bits(got[only != 0]), _bits(full[only != 0]))


@pytest.mark.parametrize("N,K,tail", [(63, 1, 0), (70, 2, 40)])
def test_constant_velocity_forecast_gives_plan_set_refs_bits(small_world, N, K, tail):
    cfg = S.lights_cfg(small_world, seed=3)
    hs = S.reset_state(cfg, small_world, 12)
    hs["steps"][...] = np.arange(12) * 5
    pl = Planner()
    seq = S.random_knots(np.random.default_rng(5), 12, N, K)
    want = S.score(cfg, small_world, hs, pl, seq, None, tail)
    got = S.score(cfg, small_world, hs, pl, seq, None, tail, forecast=Fr.constant_velocity(cfg, small_world, hs, pl.horizon + tail))
    assert np.array_equal(got["f"], want["f"]) and np.array_equal(_bits(got["cost"]), _bits(want["cost"]))
    assert np.array_equal(_bits(got["action"]), _bits(want["action"])) and got["diag"].tobytes() == want["diag"].tobytes()
    assert (want["f"] < pl.horizon + tail + 1).any() and (want["f"] == pl.horizon + tail + 1).any()
    # and a forecast that differs is read: the others parked far away take every box failure with them
    away = Fr.constant_velocity(cfg, small_world, hs, pl.horizon + tail)
    away[..., 0] += f32(1e4)
    assert (S.score(cfg, small_world, hs, pl, seq, None, tail, forecast=away)["f"] >= want["f"]).all()


def test_real_forecasts_change_the_verdicts(small_world):
    """on the junction world the route forecast and the constant-velocity line put the others in different places: the GPU tests'
    inputs tell the two apart"""
    cfg = S.lights_cfg(small_world, seed=3)
    hs = S.reset_state(cfg, small_world, 16)
    fc, cv = Fr.forecast(cfg, small_world, hs, 72), Fr.constant_velocity(cfg, small_world, hs, 72)
    pres = hs["present"].reshape(16, -1)[:, 1:] != 0
    assert np.abs(fc[:, -1, 1:, :2] - cv[:, -1, 1:, :2])[pres].max() > 5.0
    assert not fc[:, :, 1:][~pres[:, None].repeat(72, 1)].any()


def test_prototypes_and_constants_match_the_header(tmp_path):
    from torchdriveenv_amd import _lib

    c = tmp_path / "fc.c"
    c.write_text('#include <stdio.h>\n#include "tde_hip.h"\n'
                 "int (*p1)(const tde_config *, const tde_world *, const tde_state *, int32_t, const uint8_t *, float *, void *) = tde_forecast_agents;\n"
                 "int (*p2)(const tde_config *, const tde_world *, const tde_state *, const tde_planner *, const tde_plan_set *, const uint8_t *, "
                 "float *, int32_t *, float *, tde_plan_diag *, const float *, int32_t, void *) = tde_score_plans_forecast;\n"
                 'int main(void){printf("%d %d %d %d\\n", TDE_ABI_VERSION, TDE_FORECAST_MAX_T, TDE_PLAN_MAX_H, TDE_PLAN_MAX_TAIL); return p1 == 0 || p2 == 0;}\n')
    obj = str(tmp_path / "fc.o")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", obj], check=True)
    exe = str(tmp_path / "fc")
    lib = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", obj, "-o", exe, "-L", lib, "-ltde_hip", f"-Wl,-rpath,{lib}", "-Wl,--allow-shlib-undefined"], check=True)
    got = [int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [_abi.TDE_ABI_VERSION, _abi.FORECAST_MAX_T, _abi.PLAN_MAX_H, _abi.PLAN_MAX_TAIL] and got[:2] == [14, 96]
    L = _lib.load()
    assert {"tde_forecast_agents", "tde_score_plans_forecast"} <= set(_lib.SYMBOLS)
    assert len(L.tde_forecast_agents.argtypes) == 7 and len(L.tde_score_plans_forecast.argtypes) == 13
    assert L.tde_forecast_agents.argtypes[3] is C.c_int32 and L.tde_score_plans_forecast.argtypes[11] is C.c_int32


def test_library_rejects_bad_arguments():
    """the entry points' own checks (before any launch: no GPU needed)"""
    from torchdriveenv_amd import _lib, ops
    from torchdriveenv_amd.synth import synthetic_world

    L = _lib.load()
    w = synthetic_world(n_scn=2, A=8, seed=0, n_maps=1)
    st = EnvState(4, 8)
    cfg = _abi.default_config(seed=1)
    out = np.zeros((4, 96, 8, 4), f32)

    def fa(T=8, out_p=out.ctypes.data, cfg_=cfg, st_=st):
        return L.tde_forecast_agents(C.byref(cfg_) if cfg_ is not None else None, C.byref(w.host_struct()),
                                     C.byref(st_.struct) if st_ is not None else None, T, None, out_p, None)

    for kw, msg in ((dict(T=0), b"T must"), (dict(T=97), b"T must"), (dict(T=-1), b"T must"), (dict(out_p=None), b"NULL"),
                    (dict(cfg_=None), b"NULL"), (dict(st_=None), b"NULL")):
        assert fa(**kw) != 0 and msg in L.tde_last_error(), kw
    for dt in (0.0, -0.1, float("inf"), float("nan")):
        assert fa(cfg_=_abi.default_config(seed=1, dt=dt)) != 0 and b"dt" in L.tde_last_error(), dt
    st0 = EnvState(4, 8)
    st0.struct.B = 0
    assert fa(st_=st0) == 0                                              # (an empty batch returns before any launch)

    seq = np.zeros((4, 3, 2, 2), f32)
    cost, fail = np.zeros((4, 3), f32), np.zeros((4, 3), np.int32)
    pl = ops.planner_struct(Planner())

    def sp(fc_p=out.ctypes.data, fT=96, tail=0, st_=st):
        ps = _abi.TdePlanSet(seq.ctypes.data, 3, 2, 16, tail)
        return L.tde_score_plans_forecast(C.byref(cfg), C.byref(w.host_struct()), C.byref(st_.struct), C.byref(pl), C.byref(ps), None,
                                          cost.ctypes.data, fail.ctypes.data, None, None, fc_p, fT, None)

    assert sp(fc_p=None) != 0 and b"forecast is NULL" in L.tde_last_error()
    for kw in (dict(fT=31), dict(fT=71, tail=40), dict(fT=97), dict(fT=0)):
        assert sp(**kw) != 0 and b"forecast_T" in L.tde_last_error(), kw
    assert sp(tail=65) != 0 and b"tail" in L.tde_last_error()            # tde_score_plans' own checks hold
    assert sp(st_=st0) == 0 and sp(fT=32, st_=st0) == 0 and sp(fT=72, tail=40, st_=st0) == 0


def test_planner_predict_and_forecast_tensor_checks_need_no_gpu():
    import torch

    from torchdriveenv_amd import ops

    assert Planner().predict == "constant" and check_planner(Planner(predict="route")).predict == "route"
    assert check_planner(dict(predict="route")).predict == "route"
    for junk in ("Route", "", "cv", None, 1):
        with pytest.raises(ValueError):
            check_planner(Planner(predict=junk))
    fc = torch.zeros((4, 72, 8, 4), dtype=torch.float32)
    assert ops.check_forecast(fc, 4, 8, 72) == 72 and ops.check_forecast(fc, 4, 8, 32) == 72
    for bad, need in ((fc, 73), (fc[:, :40], 32), (fc.permute(0, 2, 1, 3), 8), (torch.zeros((4, 72, 8, 8))[..., ::2], 32), (fc.double(), 32),
                      (fc[:3], 32), (torch.zeros((4, 72, 4, 4)), 32), (torch.zeros((4, 97, 8, 4)), 32), (torch.zeros((4, 72, 8, 3)), 32),
                      (fc.numpy(), 32)):
        with pytest.raises(ValueError):
            ops.check_forecast(bad, 4, 8, need)
    assert ops.check_forecast(fc[:, :40].contiguous(), 4, 8, 32) == 40
