"""Routed near-field traffic on the GPU (NearField(routes=True), tde_state.slot_route): the spawner with its route words against the
restatement, the routed one-role step (env_step_routed_kernel) against the composed oracle (tests/near_field_routes_ref.py) on every
form its launcher chooses, the auto-reset closed loop of BatchedWaypointEnv, evaluate("planner"), the moving / standing pair at 128
slots, and the Python surface."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import near_field_routes_ref as RR
from torchdriveenv_amd import _abi, ops
from torchdriveenv_amd.config import EnvConfig, NearField, PlanReact, Planner
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.state import EnvState
from torchdriveenv_amd.synth import synthetic_town, synthetic_world

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTED = NearField(routes=True)
_WORLDS = {}


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _world(kind, A):
    """(world, table, device world, device table) per (kind, A) for the module: the junction world (two trips per lane at 128 slots) or
    the large-grid town, both signalised, a quarter of the slots the scenario's own agents, the rest free for the spawner"""
    if (kind, A) not in _WORLDS:
        if kind == "town":
            w = synthetic_town(n_scn=4, A=A, n_streets=4, spacing=100.0, ext=160.0, min_gap=3.4, n_signals=4)
            assert w.ints["hints"] & _abi.WORLD_LARGE_GRID
        else:
            w = synthetic_world(n_scn=4, A=A, seed=A, n_maps=2)
            assert not w.ints["hints"] & _abi.WORLD_LARGE_GRID
        assert w.has_lights
        w, tab = RR.junction_near_field(w, ROUTED, trips=2 if A == 128 else 1)
        assert (tab.cand["route"] != 0).any()
        _WORLDS[(kind, A)] = (w, tab, w.to_device(DEV, first_gap=False), tab.to_device(DEV))
    return _WORLDS[(kind, A)]


def _spawned_pair(world, tab, dw, dnf, cfg, B, mask=None, stale=None, **state_kw):
    """(host state, device state) after reset + spawner on both sides (`stale`: the word every slot_route entry holds before)"""
    A = world.A
    hs, ds = EnvState(B, A, with_slot_route=True), EnvState(B, A, device=DEV, with_slot_route=True, **state_kw)
    if stale is not None:
        RR.words(hs)[...] = stale
        ds["slot_route"].copy_(torch.from_numpy(hs["slot_route"]))
    oracle.env_reset(cfg, world, hs)
    ops.env_reset(cfg, dw, ds)
    RR.spawn(cfg, world, tab, hs, mask)
    ops.near_field_spawn(cfg, dw, ds, dnf, None if mask is None else torch.from_numpy(mask).to(DEV))
    torch.cuda.synchronize()
    return hs, ds


@pytest.mark.parametrize("A", [16, 128])
def test_spawner_writes_state_and_route_words_bit_for_bit(A):
    world, tab, dw, dnf = _world("junctions", A)
    B = 8
    cfg = _abi.default_config(seed=40 + A)
    mask = np.array([1, 1, 0, 1, 0, 1, 1, 1], np.uint8)
    for m in (None, mask):
        hs, ds = _spawned_pair(world, tab, dw, dnf, cfg, B, m, stale=0x00C0FFEE)
        d = ds.host()
        RR.same(hs, d, (A, m is None), keys=RR.AGENT + ("len", "wid", "lr", "vdes", "scn", "episode", "slot_route"))
        sr = d["slot_route"].view(np.uint32).reshape(B, A)
        assert (sr[:, 0] == 0x00C0FFEE).all()                               # the ego's entry is nobody's to write
        if m is not None:
            assert (sr[m == 0] == 0x00C0FFEE).all() and (sr[m != 0][:, 1:] != 0x00C0FFEE).all()
        assert ((sr[:, 1:] != 0) & (sr[:, 1:] != 0x00C0FFEE)).any()


def _step_parity(kind, A, B, lights, obs, mag, envs=None, steps=40):
    world, tab, dw, dnf = _world(kind, A)
    flags = (_abi.F_ALL | (_abi.F_TRAFFIC_LIGHTS if lights else 0)) & ~_abi.F_AUTORESET
    if not lights:
        flags &= ~_abi.F_TRAFFIC_LIGHTS
    cfg = _abi.default_config(seed=7 * A + lights, flags=flags, distance_cutoff=0.25)
    ds = EnvState(B, A, device=DEV, with_obs=obs, with_magnitudes=mag, with_slot_route=True)
    ops.env_reset(cfg, dw, ds)
    ops.near_field_spawn(cfg, dw, ds, dnf)
    torch.cuda.synchronize()
    envs = np.arange(B) if envs is None else np.asarray(envs)
    h0 = ds.host()
    hs = RR.sub_state(h0, envs, A)
    assert (RR.words(hs) != 0).any()
    cw = RR.compose(world, hs)
    rng = np.random.default_rng(A + B)
    moved = 0.0
    x0 = hs["x"].copy()
    for t in range(steps):
        act = np.stack([rng.uniform(-0.2, 1.0, B), rng.normal(0.0, 0.06, B).clip(-0.3, 0.3)], -1).astype(np.float32)
        ops.env_step(cfg, dw, ds, action=torch.from_numpy(act).to(DEV))
        hs["action"][...] = act[envs]
        RR.oracle_step(cfg, cw, hs)
        if t % 4 == 3 or t < 2 or t == steps - 1:
            torch.cuda.synchronize()
            RR.same(hs, ds.host(), (kind, A, B, lights, obs, mag, t), envs=envs)
    routed = RR.words(hs) != 0
    moved = np.abs(hs["x"] - x0)[routed].max()
    assert moved > 5.0, moved                                               # the routed agents drove


@pytest.mark.parametrize("lights,obs,mag", [(False, False, False), (True, False, False), (False, True, False), (True, True, True),
                                            (False, False, True)])
def test_routed_step_equals_the_composed_oracle_at_16_slots(lights, obs, mag):
    _step_parity("junctions", 16, 8, lights, obs, mag)


@pytest.mark.parametrize("A", [32, 64])
def test_routed_step_on_the_large_grid_town(A):
    _step_parity("town", A, 8, True, False, False)


@pytest.mark.parametrize("wide", [False, True])
def test_routed_step_at_128_slots(wide):
    """the default wave count (a small batch) and the 4-wave form (more than 6 envs per CU; the oracle on slices of the batch)"""
    if not wide:
        return _step_parity("junctions", 128, 8, True, False, False)
    B = 6 * _cu() + 1
    _step_parity("junctions", 128, B, False, False, True, envs=[0, 1, 2, B // 2, B - 2, B - 1], steps=40)


def test_auto_reset_closed_loop_rebuilds_the_composition_after_every_respawn():
    world, tab, _, _ = _world("junctions", 16)
    B, A, T = 8, 16, 40
    cfg = EnvConfig(seed=21, distance_cutoff=0.25, max_environment_steps=12, use_background_traffic=False)
    env = BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, near_field=tab, obs_mode="state")
    assert env.state["slot_route"] is not None and env.auto_reset
    c = env.tde_cfg
    c2 = _abi.TdeConfig.from_buffer_copy(c)
    c2.flags = c.flags & ~_abi.F_AUTORESET
    hs = EnvState(B, A, with_slot_route=True)
    env.reset()
    oracle.env_reset(c, world, hs)
    RR.spawn(c, world, tab, hs)
    RR.same(hs, env.state.host(), "reset", keys=RR.AGENT + ("slot_route", "scn"))
    cw = RR.compose(world, hs)
    rng = np.random.default_rng(3)
    respawns = np.zeros(B, np.int64)
    for t in range(T):
        act = np.stack([rng.uniform(0.0, 1.0, B), rng.normal(0.0, 0.03, B).clip(-0.3, 0.3)], -1).astype(np.float32)
        _, rew, term, trunc, _ = env.step(torch.from_numpy(act).to(DEV))
        hs["action"][...] = act
        RR.oracle_step(c2, cw, hs)
        done = (hs["terminated"] | hs["truncated"]).astype(np.uint8)
        assert np.array_equal(rew.cpu().numpy(), hs["reward"]) and np.array_equal((term | trunc).cpu().numpy(), done.astype(bool)), t
        if done.any():
            keep = {k: hs[k].copy() for k in ("reward", "terminated", "truncated", "tl_violation", "done_bits", "info", "info_reached")}
            oracle.env_reset(c, world, hs, done)
            for k, v in keep.items():
                hs[k][...] = v
            RR.spawn(c, world, tab, hs, done)
            cw = RR.compose(world, hs)
            respawns += done
        RR.same(hs, env.state.host(), t, keys=RR.AGENT + RR.ENV + ("slot_route", "scn", "episode"))
    assert respawns.min() >= 2, respawns


def test_evaluate_planner_is_repeatable_with_routed_traffic():
    world, tab, _, _ = _world("junctions", 16)
    cfg = EnvConfig(seed=5, max_environment_steps=30, use_background_traffic=False)
    recs = []
    for _ in range(2):
        env = BatchedWaypointEnv(cfg, world, num_envs=4, device=DEV, near_field=tab, obs_mode="state", auto_reset=False)
        res = env.evaluate("planner", cases=[0, 1, 2])
        recs.append(res)
    a, b = recs
    assert len(a.length) == 3 and int(a.length.min()) > 0
    for f in ("episode_return", "length", "reached", "scenario", "bits"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def test_routed_agents_drive_and_unrouted_ones_stand_at_128_slots():
    world, tab, dw, dnf = _world("junctions", 128)
    B, A = 8, 128
    cfg = _abi.default_config(seed=2, flags=_abi.F_ALL & ~_abi.F_AUTORESET)
    act = torch.zeros(B, 2, device=DEV)
    out = {}
    for routes in (True, False):
        ds = EnvState(B, A, device=DEV, with_slot_route=True)
        ops.env_reset(cfg, dw, ds)
        ops.near_field_spawn(cfg, dw, ds, dnf)
        if not routes:
            ds["slot_route"].zero_()
        h = ds.host()
        spawned = (h["present"].reshape(B, A) != 0) & (world.arrays["spawn"]["present"].reshape(-1, A)[h["scn"]] == 0)
        for _ in range(80):
            ops.env_step(cfg, dw, ds, action=act)
        torch.cuda.synchronize()
        out[routes] = (spawned, ds.host()["v"].reshape(B, A))
    sp, v = out[True]
    assert sp.sum(1).min() > 0 and ((v > 1.0) & sp).any(1).all()
    sp0, v0 = out[False]
    assert np.array_equal(sp, sp0) and not ((v0 > 1.0) & sp0).any()


def test_python_surface():
    world, tab, _, _ = _world("junctions", 16)
    cfg = EnvConfig(seed=1, use_background_traffic=False)
    for kw in (dict(planner=Planner(predict="route")), dict(planner=Planner(predict="queue")), dict(plan_react=PlanReact())):
        with pytest.raises(ValueError, match="routed near-field"):
            BatchedWaypointEnv(cfg, world, num_envs=8, device=DEV, near_field=tab, **kw)
    env = BatchedWaypointEnv(cfg, world, num_envs=8, device=DEV, near_field=tab, obs_mode="state")
    env.reset()
    with pytest.raises(ValueError, match="routed near-field"):
        env.rollout(torch.zeros(4, 8, 2, device=DEV))
    with pytest.raises(Exception, match="slot_route is set"):
        env.forecast_agents(8)
    sd = env.state_dict()
    assert "slot_route" in sd and bool((sd["slot_route"] != 0).any())
    for _ in range(3):
        env.step(torch.zeros(8, 2, device=DEV))
    other = {k: v.clone() for k, v in env.state_dict().items()}
    env.load_state_dict(sd)
    for k, v in sd.items():
        assert torch.equal(env.state.arrays[k], v), k
    assert not torch.equal(other["x"], sd["x"])
