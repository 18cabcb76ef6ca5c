"""tde_forecast_scene on the GPU: the kernel against its numpy restatement (tests/forecast_scene_ref.py), bit for bit and through both
bindings, at the smallest shapes at which it can go wrong - 4 slots x 65 envs (64 envs per workgroup plus a ragged one), 16 x 33 (two
workgroups plus one env), 64 slots at the kernel matrix's batch, 128 x 3 (an env across two wavefronts plus a half-filled workgroup) -
with lights on and off, on junction and town worlds, from mid-episode states with differing step counters (some at step 0), under
random ego actions and none, T = 1 and 96, with an `only` mask over a sentinel; the kernel against 32 real tde_env_step launches; and
plan_actions() under Planner(predict="queue")."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import forecast_scene_ref as Sr
from tests import kernel_matrix as km
from tests import plan_set_ref as S
from tests.plan_gpu_util import bits, on_device
from torchdriveenv_amd import _abi, _ext, ops
from torchdriveenv_amd.config import EnvConfig, Planner, PlanRefine
from torchdriveenv_amd.env import BatchedWaypointEnv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_MAX = _abi.FORECAST_MAX_T
_worlds = {}


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _world(kind, A):
    """the kernel matrix's worlds (tests/test_gpu_kernel_matrix.py): the junction maps, and the crowded signalised town whose 64- and
    128-slot scenes are full"""
    if (kind, A) not in _worlds:
        from torchdriveenv_amd.synth import synthetic_town, synthetic_world

        if kind == "town":
            w = synthetic_town(n_scn=4, A=A, n_streets=4, spacing=100.0, ext=160.0, min_gap=3.4, n_signals=4)
        else:
            w = synthetic_world(n_scn=8, A=A, seed=A, n_maps=2)
        assert w.has_lights
        _worlds[(kind, A)] = w
    return _worlds[(kind, A)]


def _batch(A):
    return {4: 65, 16: 33, 64: km._small_B(64)(_cu()), 128: 3}[A]


def _mid_episode_state(cfg, world, B, seed, **over):
    """25 oracle steps under random ego actions with auto-reset, then every fourth env reset again (step 0: the first-step rule) and
    every other env's step counter moved on (the lights' phase and the replay records follow it).  over: tde_config fields of the drive
    (tests/test_gpu_config_zoo.py)"""
    drive = S.lights_cfg(world, seed=seed, terminated_at_infraction=1, **over)
    drive.flags = cfg.flags | _abi.F_AUTORESET
    hs = S.reset_state(drive, world, B)
    rng = np.random.default_rng(seed)
    for _ in range(25):
        hs["action"][...] = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
        oracle.env_step(drive, world, hs)
    fresh = (np.arange(B) % 4 == 3).astype(np.uint8)
    oracle.env_reset(drive, world, hs, mask=fresh)
    hs["steps"][::2] += 7 * (1 + np.arange(len(hs["steps"][::2]), dtype=np.int32) % 9)
    assert (np.asarray(hs["steps"])[fresh != 0] == 0).all() and len(set(np.asarray(hs["steps"]).tolist())) > 2
    return hs


def _random_actions(B, T, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-1.0, 1.0, (B, T)), rng.uniform(-0.3, 0.3, (B, T))], -1).astype(np.float32)


def _call(binding, cfg, dw, ds, T, act, only, out):
    if binding == "ctypes":
        ops.forecast_scene(cfg, dw, ds, T, act, only, out)
    else:
        _ext.env_handle(cfg, dw, ds).forecast_scene(out, act, only, int(cfg.flags))


# ---- 1. the kernel == the restatement ----------------------------------------------------------------------------------------------------

# 128 slots only on the town: a junction map has spawn room for some 20 cars, so a 128-slot junction world would leave the second
# wavefront's slots absent; the crowded town fills them (asserted below: slots >= 64 present, and some absent)
@pytest.mark.parametrize("lights", [True, False], ids=["lit", "dark"])
@pytest.mark.parametrize("kind,A", [("junctions", 4), ("junctions", 16), ("junctions", 64), ("town", 4), ("town", 16), ("town", 64),
                                    ("town", 128)])
def test_kernel_equals_the_restatement(kind, A, lights):
    world = _world(kind, A)
    B = _batch(A)
    cfg = S.lights_cfg(world, seed=100 + A, terminated_at_infraction=0)
    cfg.flags &= ~_abi.F_AUTORESET
    if not lights:
        cfg.flags &= ~_abi.F_TRAFFIC_LIGHTS
    hs = _mid_episode_state(cfg, world, B, seed=A + (1 if lights else 0))
    pres = np.asarray(hs["present"]).reshape(B, A) != 0
    if A == 128:
        assert pres[:, 64:].any() and (~pres).any()
    act = _random_actions(B, T_MAX, 5 * A)
    want = Sr.forecast_scene(cfg, world, hs, T_MAX, ego_action=act)
    only = (np.arange(B) % 3 != 1).astype(np.uint8)
    want_null = Sr.forecast_scene(cfg, world, hs, T_MAX, only=only, out=np.full((B, T_MAX, A, 4), -7.0, np.float32))
    assert want[:, :, 0].any() and not want[~pres[:, None].repeat(T_MAX, 1)].any()
    assert (bits(want[only != 0][:, :, 1:]) != bits(want_null[only != 0][:, :, 1:])).any()   # the ego's actions reach the others
    dw, ds = on_device(world, hs)
    dact = torch.from_numpy(act).to(DEV)
    dact1 = dact[:, :1].contiguous()
    m = torch.from_numpy(only).to(DEV)
    for binding in ("ctypes", "ext"):
        out = torch.full((B, T_MAX, A, 4), -7.0, dtype=torch.float32, device=DEV)
        masked = out.clone()
        one = torch.full((B, 1, A, 4), -7.0, dtype=torch.float32, device=DEV)
        _call(binding, cfg, dw, ds, T_MAX, dact, None, out)
        _call(binding, cfg, dw, ds, T_MAX, None, m, masked)
        _call(binding, cfg, dw, ds, 1, dact1, None, one)
        torch.cuda.synchronize()
        for got, ref, what in ((out.cpu().numpy(), want, "actions"), (masked.cpu().numpy(), want_null, "coasting, only"),
                               (one.cpu().numpy(), want[:, :1], "T = 1")):
            bad = np.argwhere(bits(got) != bits(ref))
            assert len(bad) == 0, (kind, A, lights, binding, what, len(bad), bad[:6].tolist(), got[tuple(bad[0][:3])], ref[tuple(bad[0][:3])])
    # the device state is not written
    after = ds.host()
    for n in ("x", "y", "psi", "v", "route_wp", "steps"):
        assert np.array_equal(np.asarray(after[n]), np.asarray(hs[n])), n


# ---- 2. the environment as oracle: 32 real tde_env_step launches --------------------------------------------------------------------------

@pytest.mark.parametrize("binding", ["ext", "ctypes"])
@pytest.mark.parametrize("kind,A,B", [("junctions", 16, 33), ("town", 128, 3)])
def test_kernel_equals_32_real_steps(kind, A, B, binding):
    world = _world(kind, A)
    env = BatchedWaypointEnv(EnvConfig(seed=31, terminated_at_infraction=False, max_environment_steps=200), world, num_envs=B, device=DEV,
                             obs_mode="state", auto_reset=False, binding=binding)
    assert not (env.tde_cfg.flags & _abi.F_AUTORESET) and (env.tde_cfg.flags & _abi.F_TRAFFIC_LIGHTS)
    env.reset()
    T = 32
    act = torch.from_numpy(_random_actions(B, T, 77)).to(DEV)
    fc = env.forecast_scene(T=T, ego_actions=act)
    free = env.forecast_agents(T=T)
    assert tuple(fc.shape) == (B, T, A, 4)
    pres = (env.state["present"].view(B, A) != 0)[..., None]
    for h in range(1, T + 1):
        env.step(act[:, h - 1].contiguous())
        got = torch.stack([env.state[n].view(B, A) for n in ("x", "y", "psi", "v")], -1)
        got = torch.where(pres, got, torch.zeros_like(got))
        diff = got.view(torch.int32) != fc[:, h - 1].view(torch.int32)
        assert not diff.any(), (kind, binding, h, torch.nonzero(diff)[:4].tolist())
    assert (env.state["steps"] == T).all()
    # the run had queues in it: the free-flow forecast is somewhere else
    assert (fc[:, :, 1:].view(torch.int32) != free[:, :, 1:].view(torch.int32)).any()


# ---- 3. the planner -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("binding", ["ext", "ctypes"])
@pytest.mark.parametrize("tail", [0, 40])
def test_plan_actions_under_predict_queue(small_world, binding, tail):
    B, A = 48, small_world.A
    pl = Planner(predict="queue")
    env = BatchedWaypointEnv(EnvConfig(seed=23, distance_cutoff=0.25, max_environment_steps=200), small_world, num_envs=B, device=DEV,
                             obs_mode="state", binding=binding, planner=pl, plan_refine=PlanRefine(rounds=0, tail=tail) if tail else None)
    env.reset()
    zeros = torch.zeros((B, 2), dtype=torch.float32, device=DEV)
    acc, ste = pl.tables()
    lat = np.stack([np.repeat(acc, len(ste)), np.tile(ste, len(acc))], -1).astype(np.float32)
    seq = torch.from_numpy(lat).to(DEV)[None, :, None, :].expand(B, len(lat), 1, 2).contiguous()
    for t in range(3):
        a, d = env.plan_actions(diag=True)
        a, d = a.clone(), d.clone()
        T = pl.horizon + tail
        assert tuple(env._plan_fc.shape) == (B, T, A, 4)
        fc = env.forecast_scene(T=T)
        assert torch.equal(fc.view(torch.int32), env._plan_fc.view(torch.int32))
        cost = torch.zeros((B, len(lat)), dtype=torch.float32, device=DEV)
        fail = torch.zeros((B, len(lat)), dtype=torch.int32, device=DEV)
        wa = torch.zeros((B, 2), dtype=torch.float32, device=DEV)
        wd = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
        ops.score_plans(env.tde_cfg, env.dworld, env.state, pl, seq, int(pl.horizon), tail, None, cost, fail, wa, wd, forecast=fc)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), wa.view(torch.int32)) and torch.equal(d, wd), (binding, tail, t)
        free = env.forecast_agents(T=T)
        assert (fc[:, :, 1:].view(torch.int32) != free[:, :, 1:].view(torch.int32)).any(), (binding, tail, t)
        assert not free[:, :, 0].any() and fc[:, :, 0].any()
        for _ in range(15):
            env.step(zeros)
