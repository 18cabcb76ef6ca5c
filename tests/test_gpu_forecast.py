"""tde_forecast_agents and tde_score_plans_forecast on the GPU against their numpy restatements (tests/forecast_ref.py; the judge:
plan_set_ref.score(forecast=)), bit for bit and through both bindings: the forecast kernel at T = 96 on the junction, town and
128-slot worlds, from fresh and from driven states; the environment as the oracle (32 steps of the hand-made world of
tests/test_forecast_cpu.py leave what the forecast said); the judge on a constant-velocity forecast against tde_score_plans; the judge
on real forecasts against the restatement; plan_actions() under each Planner.predict; and graph capture."""
import numpy as np
import pytest
import torch

from tests import forecast_ref as Fr
from tests import plan_set_ref as S
from tests.plan_gpu_util import bits, check_score_plans, on_device
from torchdriveenv_amd import _abi, _ext, ops
from torchdriveenv_amd.config import EnvConfig, Planner, PlanRefine
from torchdriveenv_amd.env import BatchedWaypointEnv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_MAX = _abi.FORECAST_MAX_T
WORLDS = {"junctions": 64, "town": 32, "slots128": 8}          # world -> envs
STATES = ("reset", "reset_coast_first", "driven")
_cache = {}


def _world(name, small_world, small_town):
    if name == "slots128":
        if name not in _cache:
            # the crowded town of tests/test_gpu_wide.py, with signals: ~122 of the 128 slots taken at a reset (a junction map has
            # spawn room for some 20 cars only, which leaves every slot past the first wavefront absent)
            from torchdriveenv_amd.synth import synthetic_town

            _cache[name] = synthetic_town(n_scn=4, A=128, seed=5, n_streets=4, spacing=100.0, ext=160.0, min_gap=3.4, n_signals=4)
        return _cache[name]
    return small_world if name == "junctions" else small_town


def _state(wname, sname, small_world, small_town):
    """(cfg, world, host state): right after a reset (steps = 0; with and without TDE_F_NPC_FIRST_STEP), or 40 steps under
    plan_actions() with auto-reset - route targets advanced, queues, and on every other env a step counter moved late into the
    episode, where the parked cars' replay records (220 rows) run out in the middle of a 96-step forecast"""
    key = (wname, sname)
    if key in _cache:
        return _cache[key]
    world, B = _world(wname, small_world, small_town), WORLDS[wname]
    if sname == "driven":
        env = BatchedWaypointEnv(EnvConfig(seed=21, distance_cutoff=0.25, max_environment_steps=200), world, num_envs=B, device=DEV,
                                 obs_mode="state", planner=Planner())
        env.reset()
        for _ in range(40):
            env.step(env.plan_actions())
        torch.cuda.synchronize()
        hs = env.state.host()
        cfg = env.tde_cfg
        assert (hs["route_wp"] > 0).any()
        hs["steps"][::2] += 140
    else:
        cfg = S.lights_cfg(world, seed=21)
        if sname == "reset_coast_first":
            cfg.flags &= ~_abi.F_NPC_FIRST_STEP
        hs = S.reset_state(cfg, world, B)
        assert (hs["steps"] == 0).all()
    _cache[key] = (cfg, world, hs)
    return _cache[key]


def _want_forecast(wname, sname, small_world, small_town):
    key = (wname, sname, "fc")
    if key not in _cache:
        cfg, world, hs = _state(wname, sname, small_world, small_town)
        _cache[key] = Fr.forecast(cfg, world, hs, T_MAX)
    return _cache[key]


# ---- 1. the forecast kernel == the restatement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sname", STATES)
@pytest.mark.parametrize("wname", list(WORLDS))
def test_forecast_equals_the_restatement(small_world, small_town, wname, sname):
    cfg, world, hs = _state(wname, sname, small_world, small_town)
    want = _want_forecast(wname, sname, small_world, small_town)
    B, A = len(hs["scn"]), world.A
    pres = np.asarray(hs["present"]).reshape(B, A) != 0
    assert not want[:, :, 0].any() and not want[~pres[:, None].repeat(T_MAX, 1)].any()
    if wname == "slots128":
        assert (~pres).any() and pres[:, 64:].any()                     # absent slots, and slots beyond one wavefront
    if sname == "driven":
        rec = world.arrays["spawn"].reshape(-1, A)[hs["scn"]]
        out_mid = (rec["replay"] >= 0) & pres & (hs["steps"][:, None] < rec["replay_len"]) & (hs["steps"][:, None] + T_MAX > rec["replay_len"])
        assert out_mid.any()                                            # a replay record runs out inside the forecast
    dw, ds = on_device(world, hs)
    only = (np.arange(B) % 3 != 1).astype(np.uint8)
    m = torch.from_numpy(only).to(DEV)
    for binding in ("ctypes", "ext"):
        out = torch.full((B, T_MAX, A, 4), -7.0, dtype=torch.float32, device=DEV)
        masked = out.clone()
        if binding == "ctypes":
            ops.forecast_agents(cfg, dw, ds, T_MAX, None, out)
            ops.forecast_agents(cfg, dw, ds, T_MAX, m, masked)
        else:
            h = _ext.env_handle(cfg, dw, ds)
            h.forecast_agents(out, None, int(cfg.flags))
            h.forecast_agents(masked, m, int(cfg.flags))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        bad = np.argwhere(bits(got) != bits(want))
        assert len(bad) == 0, (wname, sname, binding, len(bad), bad[:6].tolist(), got[tuple(bad[0][:3])], want[tuple(bad[0][:3])])
        gm = masked.cpu().numpy()
        assert (gm[only == 0] == -7.0).all() and np.array_equal(bits(gm[only != 0]), bits(want[only != 0])), (wname, sname, binding)
    short = ops.forecast_agents(cfg, dw, ds, 5)                         # a shorter forecast is the longer one's head
    assert np.array_equal(bits(short.cpu().numpy()), bits(want[:, :5]))


# ---- 2. the environment as oracle -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("binding", ["ext", "ctypes"])
def test_environment_is_the_oracle(binding):
    cfg0, world = Fr.oracle_world()
    B, A = Fr.ORACLE_B, world.A
    env = BatchedWaypointEnv(EnvConfig(seed=11, terminated_at_infraction=False, max_environment_steps=200), world, num_envs=B, device=DEV,
                             obs_mode="state", auto_reset=False, binding=binding)
    assert not (env.tde_cfg.flags & _abi.F_AUTORESET) and (env.tde_cfg.flags & _abi.F_TRAFFIC_LIGHTS)
    env.reset()
    assert set(env.state["scn"].cpu().numpy().tolist()) == {0, 1, 2, 3}
    fc = env.forecast_agents(T=Fr.ORACLE_STEPS)
    assert tuple(fc.shape) == (B, Fr.ORACLE_STEPS, A, 4) and not fc[:, :, 0].any()
    zeros = torch.zeros((B, 2), dtype=torch.float32, device=DEV)
    for h in range(1, Fr.ORACLE_STEPS + 1):
        env.step(zeros)
        got = torch.stack([env.state[n].view(B, A) for n in ("x", "y", "psi", "v")], -1)[:, 1:]
        same = torch.equal(got.view(torch.int32), fc[:, h - 1, 1:].view(torch.int32))
        assert same, (binding, h, torch.nonzero(got.view(torch.int32) != fc[:, h - 1, 1:].view(torch.int32))[:4].tolist())
    assert (env.state["steps"] == Fr.ORACLE_STEPS).all()


# ---- 3. a constant-velocity forecast gives tde_score_plans' bits ------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,tail", [(63, 1, 0), (126, 2, 40)])
@pytest.mark.parametrize("wname", ["junctions", "slots128"])
def test_constant_velocity_forecast_equals_score_plans(small_world, small_town, wname, N, K, tail):
    cfg, world, hs = _state(wname, "driven", small_world, small_town)
    B = len(hs["scn"])
    pl = Planner()
    dw, ds = on_device(world, hs)
    fc = torch.from_numpy(Fr.constant_velocity(cfg, world, hs, pl.horizon + tail)).to(DEV)   # (c, s) = sincos_f32's values: the restatement's
    seq = torch.from_numpy(S.random_knots(np.random.default_rng(41), B, N, K)).to(DEV)
    res = []
    for f in (None, fc):
        cost = torch.zeros((B, N), dtype=torch.float32, device=DEV)
        fail = torch.zeros((B, N), dtype=torch.int32, device=DEV)
        act = torch.zeros((B, 2), dtype=torch.float32, device=DEV)
        dg = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
        ops.score_plans(cfg, dw, ds, pl, seq, None, tail, None, cost, fail, act, dg, forecast=f)
        res.append((cost, fail, act, dg))
    torch.cuda.synchronize()
    for a, b, what in zip(res[0], res[1], ("cost", "fail_step", "action", "diag")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (wname, N, K, tail, what)
    f = res[0][1].cpu().numpy()
    assert (f < pl.horizon + tail + 1).any() and (f == pl.horizon + tail + 1).any()


# ---- 4. the judge on real forecasts == the restatement ----------------------------------------------------------------------------------

@pytest.mark.parametrize("N,K,tail", [(N, K, tail) for N in (5, 63, 130) for K in (1, 4) for tail in (0, 40)])
@pytest.mark.parametrize("sname", STATES)
@pytest.mark.parametrize("wname", list(WORLDS))
def test_score_plans_forecast_equals_the_restatement(small_world, small_town, wname, sname, N, K, tail):
    """(the envs of a stride are judged - `only` - so that the restatement's brute-force road test stays a second or two per case)"""
    cfg, world, hs = _state(wname, sname, small_world, small_town)
    fc = _want_forecast(wname, sname, small_world, small_town)
    B = len(hs["scn"])
    pl = Planner()
    stride = {"junctions": 6, "town": 4, "slots128": 2}[wname]
    only = (np.arange(B) % stride == (N + K) % stride).astype(np.uint8)
    rng = np.random.default_rng(1000 * N + 10 * K + tail)
    seq = S.calm_knots(rng, S.random_knots(rng, B, N, K, wild=True))    # knots outside the action box, one NaN knot per env
    check_score_plans(cfg, world, hs, pl, seq, -(-pl.horizon // K), tail, only=only, forecast=fc, what=(wname, sname, N, K, tail))


# ---- 5. plan_actions() under each Planner.predict ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("binding", ["ext", "ctypes"])
def test_plan_actions_follows_planner_predict(small_world, binding):
    B = 48
    envs = {}
    for predict, pr in (("constant", None), ("route", None), ("route", PlanRefine(rounds=0, tail=40))):
        env = BatchedWaypointEnv(EnvConfig(seed=23, distance_cutoff=0.25, max_environment_steps=200), small_world, num_envs=B, device=DEV,
                                 obs_mode="state", binding=binding, planner=Planner(predict=predict), plan_refine=pr)
        env.reset()
        envs[(predict, pr is not None)] = env
    zeros = torch.zeros((B, 2), dtype=torch.float32, device=DEV)
    for t in range(3):
        for (predict, tailed), env in envs.items():
            a, d = env.plan_actions(diag=True)
            torch.cuda.synchronize()
            hs = env.state.host()
            if predict == "constant":
                # the parent's path: tde_plan_action itself, the same kernel with the same output
                out = torch.zeros((B, 2), dtype=torch.float32, device=DEV)
                dg = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
                ops.plan_action(env.tde_cfg, env.dworld, env.state, env.planner, out, None, dg)
                assert torch.equal(a.view(torch.int32), out.view(torch.int32)) and torch.equal(d, dg), (binding, t)
                assert env._plan_fc is None and env._plan_lat is None
            else:
                wa, wd = Fr.plan_routed(env.tde_cfg, small_world, hs, env.planner, tail=40 if tailed else 0)
                assert np.array_equal(bits(a.cpu().numpy()), bits(wa)), (binding, t, tailed)
                assert np.array_equal(d.cpu().numpy().view(np.uint32), wd.view(np.uint32).reshape(B, 4)), (binding, t, tailed)
                assert tuple(env._plan_fc.shape) == (B, 72 if tailed else 32, small_world.A, 4)
            for _ in range(20):                                         # (a common drive, so that the three envs see the same kind of state)
                env.step(env.plan_actions() if predict == "constant" else zeros)


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------------------

def test_forecast_and_judge_are_graph_capturable(small_world, small_town):
    cfg, world, hs = _state("junctions", "driven", small_world, small_town)
    B, A, N, tail = len(hs["scn"]), world.A, 130, 40
    pl = Planner()
    T = pl.horizon + tail
    dw, ds = on_device(world, hs)
    seq = torch.from_numpy(S.random_knots(np.random.default_rng(3), B, N, 2)).to(DEV)
    bufs = [dict(fc=torch.zeros((B, T, A, 4), dtype=torch.float32, device=DEV), cost=torch.zeros((B, N), dtype=torch.float32, device=DEV),
                 fail=torch.zeros((B, N), dtype=torch.int32, device=DEV), act=torch.zeros((B, 2), dtype=torch.float32, device=DEV),
                 dg=torch.zeros((B, 4), dtype=torch.int32, device=DEV)) for _ in range(2)]

    def run(b):
        ops.forecast_agents(cfg, dw, ds, T, None, b["fc"])
        ops.score_plans(cfg, dw, ds, pl, seq, None, tail, None, b["cost"], b["fail"], b["act"], b["dg"], forecast=b["fc"])

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(bufs[0])                                                    # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    run(bufs[1])
    for v in bufs[0].values():
        v.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(bufs[0])
    g.replay()
    torch.cuda.synchronize()
    for k in bufs[0]:
        assert torch.equal(bufs[0][k].view(torch.int32), bufs[1][k].view(torch.int32)), k
    assert bufs[1]["fc"].any() and (bufs[1]["fail"] < T + 1).any()
