"""CPU checks of tde_score_plans_scene: the restatement by composition (tests/plan_scene_ref.py) held against the C oracle's step - with
margin = 0 the judge's fail_step is the step at which the environment ends the episode by an infraction -, the reaction shown to be
live (verdicts differ from those against one coasting-ego scene), the entry point's own argument checks (before any launch: no GPU
needed) and the configuration checks of PlanReact."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle
from tests import forecast_scene_ref as Sr
from tests import plan_scene_ref as Pr
from tests import plan_set_ref as S
from torchdriveenv_amd import _abi
from torchdriveenv_amd.config import PLANNER_PREDICT, PlanReact, Planner, PlanRefine, check_plan_react
from torchdriveenv_amd.state import EnvState

f32 = np.float32
H, TAIL = 32, 10


def _world(A):
    from torchdriveenv_amd.synth import synthetic_world

    return synthetic_world(n_scn=8, A=A, seed={16: 0, 4: 3}[A], n_maps=2)


def lookahead_inputs(world, B, N, seed, drive=12):
    """(cfg with default flags + lights, host state a few steps into its episodes, Planner(margin = 0), seq [B, N, 2, 2])"""
    cfg = S.lights_cfg(world, seed=seed)
    assert cfg.flags & _abi.F_TRAFFIC_LIGHTS and cfg.flags & _abi.F_AUTORESET and cfg.terminated_at_infraction == 1
    hs = S.reset_state(cfg, world, B)
    rng = np.random.default_rng(seed)
    for _ in range(drive):
        hs["action"][...] = np.stack([rng.uniform(-0.2, 0.6, B), rng.uniform(-0.03, 0.03, B)], -1).astype(f32)
        oracle.env_step(cfg, world, hs)
    seq = S.calm_knots(rng, S.random_knots(rng, B, N, 2))
    return cfg, hs, Planner(horizon=H, margin=0.0), seq


def oracle_stepper(cfg, world, hs, N):
    """step(h, actions) over a tiled COPY of the host state through the C oracle -> done_bits of that step"""
    tiled = Pr.tile_state(hs, N)
    V = len(tiled["scn"])
    st = EnvState(V, world.A)
    st.load(tiled)

    def step(h, act):
        st["action"][...] = act
        oracle.env_step(cfg, world, st)
        return np.array(st["done_bits"], copy=True)

    return step


@pytest.mark.parametrize("A,B,N", [(16, 16, 12), (4, 24, 9)])
def test_lookahead_equals_the_environment(A, B, N):
    """every predicate agrees with the step here: collision, offroad and red line are all followed (INFRACTION)"""
    world = _world(A)
    cfg, hs, pl, seq = lookahead_inputs(world, B, N, seed=40 + A)
    res = Pr.score(cfg, world, hs, pl, seq, 16, TAIL)
    ea, moved = Pr.effective_actions(cfg, hs, pl, seq, 16, TAIL, with_steps=True)
    n_fail, n_safe = Pr.check_lookahead(res["f"].ravel(), ea, moved, H + TAIL, oracle_stepper(cfg, world, hs, N))
    V = B * N
    print(f"lookahead A={A}: {n_fail} of {V} end by an infraction, {n_safe} survive; f <= H+tail for {(res['f'] <= H + TAIL).sum()}")
    assert (res["f"] <= H + TAIL).sum() >= 0.10 * V and n_fail >= 0.10 * V, (n_fail, V)
    assert n_safe >= 0.10 * V, (n_safe, V)


def reaction_inputs(world, B, seed):
    """hard-braking and accelerating one-knot sequences on a junction world a few steps in"""
    cfg, hs, pl, _ = lookahead_inputs(world, B, 1, seed)
    acc = np.array([-1.0, -1.0, -0.6, 0.5, 1.0, 1.0], f32)
    ste = np.array([0.0, 0.02, 0.0, 0.0, 0.0, -0.02], f32)
    seq = np.ascontiguousarray(np.broadcast_to(np.stack([acc, ste], -1)[None, :, None, :], (B, len(acc), 1, 2)))
    return cfg, hs, pl, seq


def test_the_reaction_is_live():
    world = _world(16)
    B = 32
    cfg, hs, pl, seq = reaction_inputs(world, B, seed=77)
    react = Pr.score(cfg, world, hs, pl, seq, H, 40)
    fc = Sr.forecast_scene(cfg, world, hs, H + 40)                      # plan_queued's way: one scene for all, the ego coasting
    coast = S.score(cfg, world, hs, pl, seq, H, 40, forecast=fc)
    differ = int((react["f"] != coast["f"]).sum())
    print(f"reaction: fail_step differs for {differ} of {react['f'].size} (e, n) pairs ({100.0 * differ / react['f'].size:.1f} %)")
    assert differ > 0


def test_library_rejects_bad_arguments():
    """the entry point's own checks (before any launch: no GPU needed)"""
    from torchdriveenv_amd import _lib
    from torchdriveenv_amd.synth import synthetic_world

    L = _lib.load()
    assert "tde_score_plans_scene" in _lib.SYMBOLS and len(L.tde_score_plans_scene.argtypes) == 11 and L.tde_abi_version() == 14
    w = synthetic_world(n_scn=2, A=8, seed=0, n_maps=1)
    st = EnvState(4, 8)
    cfg = _abi.default_config(seed=1)
    N, K = 5, 2
    seq = np.zeros((4, N, K, 2), f32)
    cost, fail = np.zeros((4, N), f32), np.zeros((4, N), np.int32)
    from torchdriveenv_amd import ops

    def planner(**kw):
        return ops.planner_struct(Planner(**kw))

    def call(cfg_=cfg, w_=w, st_=st, pl_=planner(), set_=True, seq_p=seq.ctypes.data, N_=N, K_=K, L_=16, tail=0, cost_p=cost.ctypes.data,
             fail_p=fail.ctypes.data):
        ps = _abi.TdePlanSet(seq_p, N_, K_, L_, tail)
        return L.tde_score_plans_scene(C.byref(cfg_) if cfg_ is not None else None, C.byref(w_.host_struct()) if w_ is not None else None,
                                       C.byref(st_.struct) if st_ is not None else None, C.byref(pl_) if pl_ is not None else None,
                                       C.byref(ps) if set_ else None, None, cost_p, fail_p, None, None, None)

    for kw in (dict(cfg_=None), dict(w_=None), dict(st_=None), dict(pl_=None), dict(set_=False), dict(seq_p=None), dict(cost_p=None),
               dict(fail_p=None)):
        assert call(**kw) != 0 and b"NULL" in L.tde_last_error() and b"tde_score_plans_scene" in L.tde_last_error(), kw
    for kw, msg in ((dict(N_=0), b"N must"), (dict(N_=1025), b"N must"), (dict(K_=0), b"K must"), (dict(K_=33), b"K must"),
                    (dict(L_=0), b"knot_len"), (dict(tail=-1), b"tail must"), (dict(tail=65), b"tail must")):
        assert call(**kw) != 0 and msg in L.tde_last_error() and b"tde_score_plans_scene" in L.tde_last_error(), kw
    for hz in (0, 33):
        p = planner()
        p.horizon = hz
        assert call(pl_=p) != 0 and b"horizon" in L.tde_last_error()
    p = planner()
    p.margin = -0.1
    assert call(pl_=p) != 0 and b"margin" in L.tde_last_error()
    for dt in (0.0, float("nan")):
        assert call(cfg_=_abi.default_config(seed=1, dt=dt)) != 0 and b"dt" in L.tde_last_error()
    # what tde_score_plans reads and what tde_forecast_scene reads
    for name in ("x", "y", "psi", "v", "len", "wid", "lr", "vdes", "route_wp", "present", "scn", "steps", "target_idx"):
        st1 = EnvState(4, 8)
        setattr(st1.struct, name, None)
        assert call(st_=st1) != 0 and b"pointer is NULL" in L.tde_last_error(), name
    # the launch grid: B * N * A <= 2^31 - 256
    big = EnvState(4, 8)
    big.struct.B = 1 << 22
    assert call(st_=big, N_=1024) != 0 and b"TDE_PLAN_SCENE_MAX_LANES" in L.tde_last_error()
    assert _abi.PLAN_SCENE_MAX_LANES == 2 ** 31 - 256 and (1 << 22) * 1024 * 8 > _abi.PLAN_SCENE_MAX_LANES
    st0 = EnvState(4, 8)
    st0.struct.B = 0
    assert call(st_=st0) == 0                                           # (an empty batch returns before any launch)


def test_plan_react_configuration():
    assert PLANNER_PREDICT == ("constant", "route", "queue") and Planner().predict == "constant"
    assert PlanReact().tail == 40 and check_plan_react(PlanReact(tail=0)).tail == 0 and check_plan_react(dict(tail=64)).tail == 64
    assert check_plan_react(PlanReact(), Planner()).tail == 40
    for bad in (-1, 65, 1.5, True):
        with pytest.raises(ValueError):
            check_plan_react(PlanReact(tail=bad))
    with pytest.raises(TypeError):
        check_plan_react(PlanRefine())
    with pytest.raises(ValueError, match="plan_refine"):
        check_plan_react(PlanReact(), Planner(), PlanRefine(rounds=0))
    for predict in ("route", "queue"):
        with pytest.raises(ValueError, match="predict"):
            check_plan_react(PlanReact(), Planner(predict=predict))


def test_env_refuses_react_with_refine_or_a_forecast_before_it_needs_a_gpu():
    """the three ValueErrors of the public surface: they are raised by the configuration checks the constructor runs first, and by
    score_plans ahead of any device work"""
    import torch

    from torchdriveenv_amd.config import EnvConfig
    from torchdriveenv_amd.env import BatchedWaypointEnv

    for kw in (dict(plan_react=PlanReact(), plan_refine=PlanRefine(rounds=0)), dict(plan_react=PlanReact(), planner=Planner(predict="queue")),
               dict(plan_react=dict(tail=99))):
        with pytest.raises(ValueError, match="plan_react"):
            BatchedWaypointEnv(EnvConfig(), None, num_envs=1, **kw)
    env = object.__new__(BatchedWaypointEnv)                            # (no device: score_plans refuses before it touches one)
    with pytest.raises(ValueError, match="react=True"):
        BatchedWaypointEnv.score_plans(env, torch.zeros((1, 1, 1, 2)), react=True, forecast=torch.zeros((1, 32, 16, 4)))
