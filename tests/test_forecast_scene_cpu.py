"""CPU checks of tde_forecast_scene: the numpy restatement (tests/forecast_scene_ref.py) held against the C oracle's step on worlds full
of queues - the environment is the oracle: bit for bit, every slot, the ego included, every step, under zero and under random ego actions,
at 4, 8, 16 and 128 slots per env -, free flow as the special case (tests/forecast_ref.py's bits where nobody is ever in a cone), the ego
row and the argument forms, the prototype against the header, the entry point's own argument checks and the Python-side checks that need
no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle
from tests import forecast_ref as Fr
from tests import forecast_scene_ref as Sr
from tests import plan_set_ref as S
from torchdriveenv_amd import _abi
from torchdriveenv_amd.config import PLANNER_PREDICT, Planner, check_planner
from torchdriveenv_amd.state import EnvState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
B_Q, T_Q = 32, 96


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _queue_cfg(world, seed=3):
    cfg = S.lights_cfg(world, seed=seed, terminated_at_infraction=0)
    cfg.flags &= ~_abi.F_AUTORESET
    return cfg


def _actions(B, T, seed):
    if seed is None:
        return np.zeros((B, T, 2), f32)
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-1.0, 1.0, (B, T)), rng.uniform(-0.3, 0.3, (B, T))], -1).astype(f32)


def _state_rows(hs, B, A):
    pres = np.asarray(hs["present"]).reshape(B, A) != 0
    rows = np.stack([np.asarray(hs[n]).reshape(B, A) for n in ("x", "y", "psi", "v")], -1).astype(f32)
    return np.where(pres[..., None], rows, f32(0))


def _run_env_as_oracle(cfg, world, B, T, act, hs=None):
    """T steps of the C oracle under `act` from a fresh reset (or from `hs`): after step h every slot holds row h of the forecast made
    before the first step -> (forecast, the state the forecast was made from)"""
    assert not (cfg.flags & _abi.F_AUTORESET) and cfg.terminated_at_infraction == 0
    hs = S.reset_state(cfg, world, B) if hs is None else hs
    hs0 = {k: np.array(v, copy=True) for k, v in hs.host().items()}
    fc = Sr.forecast_scene(cfg, world, hs0, T, ego_action=act)
    A = world.A
    for h in range(1, T + 1):
        hs["action"][...] = act[:, h - 1]
        oracle.env_step(cfg, world, hs)
        got = _state_rows(hs, B, A)
        bad = np.argwhere(_bits(got) != _bits(fc[:, h - 1]))
        assert len(bad) == 0, (h, len(bad), bad[:4].tolist(), got[tuple(bad[0][:2])], fc[:, h - 1][tuple(bad[0][:2])])
    assert (np.asarray(hs["steps"]) == np.asarray(hs0["steps"]) + T).all()                    # nobody re-spawned
    return fc, hs0


def _queue_world(A):
    from torchdriveenv_amd.synth import synthetic_world

    return synthetic_world(n_scn=8, A=A, seed={16: 0, 8: 1, 4: 3}[A], n_maps=2)


@pytest.mark.parametrize("A,share", [(16, 0.25), (8, 0.15), (4, 0.10)])
@pytest.mark.parametrize("act_seed", [None, 17])
def test_environment_is_the_oracle_with_queues(A, share, act_seed):
    world = _queue_world(A)
    cfg = _queue_cfg(world)
    assert cfg.flags & _abi.F_TRAFFIC_LIGHTS
    fc, hs0 = _run_env_as_oracle(cfg, world, B_Q, T_Q, _actions(B_Q, T_Q, act_seed))
    if act_seed is None:
        # the run exercised the sweep: that many present NPC slots leave the free-flow forecast somewhere in the 96 steps
        free = Fr.forecast(cfg, world, hs0, T_Q)
        pres = np.asarray(hs0["present"]).reshape(B_Q, A)[:, 1:] != 0
        differs = (_bits(fc[:, :, 1:]) != _bits(free[:, :, 1:])).any(axis=(1, 3))
        got = differs[pres].sum() / pres.sum()
        assert got >= share, (A, int(differs[pres].sum()), int(pres.sum()))
        assert not differs[~pres].any()


def test_environment_is_the_oracle_at_128_slots():
    from torchdriveenv_amd.synth import synthetic_town

    world = synthetic_town(n_scn=2, A=128, seed=5, n_streets=4, spacing=100.0, ext=160.0, min_gap=3.4, n_signals=4)
    cfg = _queue_cfg(world, seed=21)
    B, T = 2, 24
    fc, hs0 = _run_env_as_oracle(cfg, world, B, T, _actions(B, T, 5))
    pres = np.asarray(hs0["present"]).reshape(B, 128) != 0
    assert pres[:, 64:].any() and (~pres).any()                         # slots beyond one wavefront, and absent ones
    free = Fr.forecast(cfg, world, hs0, T)
    assert (_bits(fc[:, :, 65:]) != _bits(free[:, :, 65:])).any()       # a leader is found for slots of the second half


def test_free_flow_is_the_special_case():
    cfg, world = Fr.oracle_world()
    hs = S.reset_state(cfg, world, Fr.ORACLE_B)
    fc = Sr.forecast_scene(cfg, world, hs, T_Q)
    free = Fr.forecast(cfg, world, hs, T_Q)
    assert np.array_equal(_bits(fc[:, :, 1:]), _bits(free[:, :, 1:])) and fc[:, :, 0].any() and not free[:, :, 0].any()


def test_ego_row_and_argument_forms(small_world):
    cfg = _queue_cfg(small_world)
    B, A, T = 12, small_world.A, 20
    hs = S.reset_state(cfg, small_world, B)
    act = _actions(B, T, 9)
    fc = Sr.forecast_scene(cfg, small_world, hs, T, ego_action=act)
    # row 0 is the iterated bicycle under the given actions: no clamp, no scaling
    x, y, psi, v, lr = (np.ascontiguousarray(np.asarray(hs[n]).reshape(B, A)[:, 0], f32) for n in ("x", "y", "psi", "v", "lr"))
    for h in range(1, T + 1):
        oracle.kinematics_step(x, y, psi, v, lr, np.ones(B, np.uint8), np.ascontiguousarray(act[:, h - 1]), float(cfg.dt))
        assert np.array_equal(_bits(np.stack([x, y, psi, v], -1)), _bits(fc[:, h - 1, 0])), h
    wild = act.copy()
    wild[..., 0] *= f32(3.0)                                            # outside the action box: taken as given
    assert not np.array_equal(_bits(Sr.forecast_scene(cfg, small_world, hs, T, ego_action=wild)[:, :, 0]), _bits(fc[:, :, 0]))
    # None is zeros
    a, b = Sr.forecast_scene(cfg, small_world, hs, T), Sr.forecast_scene(cfg, small_world, hs, T, ego_action=np.zeros((B, T, 2), f32))
    assert np.array_equal(_bits(a), _bits(b)) and not np.array_equal(_bits(a[:, :, 0]), _bits(fc[:, :, 0]))
    # the ego's actions reach the others through the sweep
    assert (_bits(a[:, :, 1:]) != _bits(fc[:, :, 1:])).any()
    # absent slots hold zeros
    pres = np.asarray(hs["present"]).reshape(B, A) != 0
    assert (~pres).any() and not a[~pres[:, None].repeat(T, 1)].any() and a[pres[:, None].repeat(T, 1)].any()
    # the only mask, with a sentinel
    only = (np.arange(B) % 3 != 1).astype(np.uint8)
    got = Sr.forecast_scene(cfg, small_world, hs, T, ego_action=act, only=only, out=np.full((B, T, A, 4), -7.0, f32))
    assert (got[only == 0] == -7.0).all() and np.array_equal(_bits(got[only != 0]), _bits(fc[only != 0]))


def test_first_step_rule_and_differing_steps(small_world):
    cfg = _queue_cfg(small_world)
    cfg1 = _queue_cfg(small_world)
    cfg1.flags &= ~_abi.F_NPC_FIRST_STEP
    B, A, T = 12, small_world.A, 6
    hs = S.reset_state(cfg, small_world, B)
    assert (np.asarray(hs["steps"]) == 0).all() and (cfg.flags & _abi.F_NPC_FIRST_STEP)
    a, b = Sr.forecast_scene(cfg, small_world, hs, T), Sr.forecast_scene(cfg1, small_world, hs, T)
    # without the flag every NPC coasts through step one: the bicycle with the zero action
    x, y, psi, v, lr = (np.ascontiguousarray(np.asarray(hs[n], f32).ravel()) for n in ("x", "y", "psi", "v", "lr"))
    pres = np.ascontiguousarray(np.asarray(hs["present"], np.uint8).ravel())
    oracle.kinematics_step(x, y, psi, v, lr, pres, np.zeros((B * A, 2), f32), float(cfg.dt))
    coast = np.where(pres[:, None] != 0, np.stack([x, y, psi, v], -1), f32(0)).reshape(B, A, 4)
    rec = small_world.arrays["spawn"].reshape(-1, A)[np.asarray(hs["scn"])]
    free_slot = (rec["replay"] < 0) | (rec["replay_len"] <= 1)           # (a replayed slot takes its record at step one)
    free_slot[:, 0] = True
    assert np.array_equal(_bits(b[:, 0][free_slot]), _bits(coast[free_slot])) and not np.array_equal(_bits(a[:, 0]), _bits(b[:, 0]))
    # both rules against the oracle's first steps
    for c in (cfg, cfg1):
        _run_env_as_oracle(c, small_world, B, T, _actions(B, T, 3))
    # states with differing step counters: past step one the flag changes nothing, the lights' phase follows each env's counter
    hs = S.reset_state(cfg, small_world, B)
    hs["steps"][...] = 1 + np.arange(B) * 13
    a, b = Sr.forecast_scene(cfg, small_world, hs, T), Sr.forecast_scene(cfg1, small_world, hs, T)
    assert np.array_equal(_bits(a), _bits(b))
    _run_env_as_oracle(cfg, small_world, B, 40, _actions(B, 40, 4), hs=hs)


def test_prototype_matches_the_header(tmp_path):
    from torchdriveenv_amd import _lib

    c = tmp_path / "fs.c"
    c.write_text('#include <stdio.h>\n#include "tde_hip.h"\n'
                 "int (*p1)(const tde_config *, const tde_world *, const tde_state *, int32_t, const float *, const uint8_t *, float *, void *) = "
                 "tde_forecast_scene;\n"
                 'int main(void){printf("%d %d\\n", TDE_ABI_VERSION, TDE_FORECAST_MAX_T); return p1 == 0;}\n')
    obj = str(tmp_path / "fs.o")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", obj], check=True)
    exe = str(tmp_path / "fs")
    lib = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", obj, "-o", exe, "-L", lib, "-ltde_hip", f"-Wl,-rpath,{lib}", "-Wl,--allow-shlib-undefined"], check=True)
    got = [int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [14, 96] and _abi.TDE_ABI_VERSION == 14
    L = _lib.load()
    assert "tde_forecast_scene" in _lib.SYMBOLS and _lib.SYMBOLS.index("tde_forecast_scene") > _lib.SYMBOLS.index("tde_score_plans_forecast")
    assert len(L.tde_forecast_scene.argtypes) == 8 and L.tde_forecast_scene.argtypes[3] is C.c_int32
    assert L.tde_abi_version() == 14


def test_library_rejects_bad_arguments():
    """the entry point's own checks (before any launch: no GPU needed)"""
    from torchdriveenv_amd import _lib
    from torchdriveenv_amd.synth import synthetic_world

    L = _lib.load()
    w = synthetic_world(n_scn=2, A=8, seed=0, n_maps=1)
    st = EnvState(4, 8)
    cfg = _abi.default_config(seed=1)
    out = np.zeros((4, 96, 8, 4), f32)
    act = np.zeros((4, 96, 2), f32)

    def fs(T=8, out_p=out.ctypes.data, cfg_=cfg, st_=st, w_=w, act_p=act.ctypes.data):
        return L.tde_forecast_scene(C.byref(cfg_) if cfg_ is not None else None, C.byref(w_.host_struct()) if w_ is not None else None,
                                    C.byref(st_.struct) if st_ is not None else None, T, act_p, None, out_p, None)

    for kw, msg in ((dict(T=0), b"T must"), (dict(T=97), b"T must"), (dict(T=-1), b"T must"), (dict(out_p=None), b"NULL"),
                    (dict(cfg_=None), b"NULL"), (dict(st_=None), b"NULL"), (dict(w_=None), b"NULL")):
        assert fs(**kw) != 0 and msg in L.tde_last_error() and b"tde_forecast_scene" in L.tde_last_error(), kw
    for dt in (0.0, -0.1, float("inf"), float("nan")):
        assert fs(cfg_=_abi.default_config(seed=1, dt=dt)) != 0 and b"dt" in L.tde_last_error(), dt
    # the state arrays tde_forecast_agents rejects
    for name in ("x", "y", "psi", "v", "len", "wid", "lr", "vdes", "route_wp", "present", "scn", "steps"):
        st1 = EnvState(4, 8)
        setattr(st1.struct, name, None)
        assert fs(st_=st1) != 0 and b"pointer is NULL" in L.tde_last_error(), name
    st0 = EnvState(4, 8)
    st0.struct.B = 0
    assert fs(st_=st0) == 0 and fs(st_=st0, act_p=None) == 0            # (an empty batch returns before any launch)


def test_planner_predict_and_ego_action_checks_need_no_gpu():
    import torch

    from torchdriveenv_amd import ops

    assert PLANNER_PREDICT == ("constant", "route", "queue") and Planner().predict == "constant"
    assert check_planner(Planner(predict="queue")).predict == "queue" and check_planner(dict(predict="queue")).predict == "queue"
    assert check_planner(Planner(predict="route")).predict == "route"
    for junk in ("Queue", "queues", "", None):
        with pytest.raises(ValueError):
            check_planner(Planner(predict=junk))
    ea = torch.zeros((4, 72, 2), dtype=torch.float32)
    ops.check_ego_actions(ea, 4, 72)
    for bad, T in ((ea, 71), (ea[:3], 72), (ea.double(), 72), (ea.numpy(), 72), (torch.zeros((4, 72, 3)), 72), (torch.zeros((4, 72)), 72),
                   (torch.zeros((4, 72, 4))[..., ::2], 72), (ea.permute(1, 0, 2), 72), (ea.int(), 72)):
        with pytest.raises(ValueError):
            ops.check_ego_actions(bad, 4, T)
