"""tde_near_field_spawn on the GPU against its numpy restatement (tests/near_field_ref.py): the spawn itself bit for bit through both
bindings, with and without a mask; the safety of what it spawns; the closed loop of BatchedWaypointEnv(near_field=...) against the
oracle's step plus the restatement; sharding; the density on a town; the forms that refuse a near field."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import near_field_ref as R
from torchdriveenv_amd import _abi, _ext, ops
from torchdriveenv_amd.config import EnvConfig, NearField
from torchdriveenv_amd.env import BatchedWaypointEnv, world_from_waypoint_suite
from torchdriveenv_amd.state import EnvState

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AGENT = ("x", "y", "psi", "v", "len", "wid", "lr", "vdes", "route_wp", "present", "collided", "offroad")


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    d = tmp_path_factory.mktemp("nf")
    return {A: [R.validation_world(case, A, d) for case in range(5)] for A in (16, 64, 128)}


@pytest.fixture(scope="module")
def town():
    data, meshes, field = R.town_suite(n_scn=2, n_streets=4)
    return world_from_waypoint_suite(data, agents_per_env=128, road_meshes=meshes, start_headings=field, near_field=NearField(),
                                     near_field_seed=3)


def _same(h, d, keys, what):
    for k in keys:
        if k == "info":
            # psi_reward = (1 - cos(dpsi)) * -heading_penalty in float64: the kernels' cosine (tde_device.h: cos_heading_f64) and the
            # C library's differ by an ulp now and then, which the cancellation in 1 - cos turns into ~1e-15 absolute (seen at
            # 64 slots on an ego pose both sides hold bit for bit); the other three columns are exact
            hi, di = np.asarray(h[k]), d[k]
            exact = lambda a: np.ascontiguousarray(a[:, [0, 1, 3]]).view(np.uint8)    # noqa: E731
            assert np.array_equal(exact(hi), exact(di)), (what, k)
            assert np.allclose(hi[:, 2], di[:, 2], rtol=0.0, atol=1e-13), (what, k)
            continue
        assert np.array_equal(np.asarray(h[k]).view(np.uint8), d[k].view(np.uint8)), (what, k)


@pytest.mark.parametrize("A", [16, 64, 128])
def test_spawn_is_bit_exact_through_both_bindings(worlds, A):
    B = 1024
    for case, (world, tab) in enumerate(worlds[A]):
        cfg = _abi.default_config(seed=100 + case, distance_cutoff=0.25)
        dw, dnf = world.to_device(DEV, first_gap=False), tab.to_device(DEV)
        spawned = 0
        for ep in range(3):
            hs = EnvState(B, A)
            hs["episode"][...] = ep
            oracle.env_reset(cfg, world, hs)
            R.spawn(cfg, world, tab, hs)
            free = world.arrays["spawn"]["present"][hs["scn"]] == 0
            new = (hs["present"].reshape(B, A) != 0) & free
            spawned += int(new.sum())
            for binding in ("ctypes", "ext"):
                ds = EnvState(B, A, device=DEV)
                ds["episode"].fill_(ep)
                if binding == "ctypes":
                    ops.env_reset(cfg, dw, ds)
                    ops.near_field_spawn(cfg, dw, ds, dnf)
                else:
                    h = _ext.env_handle(cfg, dw, ds)
                    h.reset(None, int(cfg.flags))
                    h.near_field_spawn(_ext.near_field_of(dnf), None, int(cfg.flags))
                torch.cuda.synchronize()
                _same(hs, ds.host(), AGENT + ("scn", "episode"), (case, ep, binding))
            # safety: no spawned agent collides or is off the road right after the spawn
            args = (hs["x"], hs["y"], hs["psi"], hs["len"], hs["wid"], hs["present"])
            col = oracle.compute_collision(B, A, *args).reshape(B, A)
            off = oracle.compute_offroad(B, A, *args, world, world.map_of_scn()[hs["scn"]], world.threshold).reshape(B, A)
            assert not (col & new).any() and not (off & new).any(), (case, ep)
            # with a mask: the masked envs as the restatement has them, the others byte for byte as they were
            mask = (np.random.default_rng(ep).random(B) < 0.3).astype(np.uint8)
            ds = EnvState(B, A, device=DEV)
            ds["episode"].fill_(ep)
            ops.env_reset(cfg, dw, ds)
            before = ds.host()
            ops.near_field_spawn(cfg, dw, ds, dnf, torch.from_numpy(mask).to(DEV))
            after = ds.host()
            hm = EnvState(B, A)
            hm["episode"][...] = ep
            oracle.env_reset(cfg, world, hm)
            R.spawn(cfg, world, tab, hm, mask)
            _same(hm, after, AGENT, (case, ep, "mask"))
            keep = np.repeat(mask == 0, A)
            for k in AGENT:
                assert np.array_equal(before[k][keep], after[k][keep]), k
        assert spawned > 0, case


@pytest.mark.parametrize("A,path,binding", [(32, "step", "ext"), (64, "step", "ctypes"), (128, "step", "ext"), (32, "post_step", "ctypes")])
def test_closed_loop_matches_oracle_plus_restatement(tmp_path, A, path, binding):
    world, tab = R.validation_world(0, A, tmp_path)
    B, T = 64, 200
    cfg = EnvConfig(seed=31, distance_cutoff=0.25, max_environment_steps=40, use_background_traffic=False)
    env = BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, near_field=tab, binding=binding)
    c = env.tde_cfg
    hs = EnvState(B, A)
    obs = env.reset()
    oracle.env_reset(c, world, hs)
    R.spawn(c, world, tab, hs)
    assert np.array_equal(obs.cpu().numpy(), oracle.render_ego(c, world, hs, flags=env._rflags))
    rng = np.random.default_rng(A)
    respawned = 0
    for t in range(T):
        act = np.stack([rng.uniform(-0.2, 1.0, B), rng.normal(0.0, 0.08, B).clip(-0.3, 0.3)], -1).astype(np.float32)
        a = torch.from_numpy(act).to(DEV)
        if path == "step":
            obs, rew, term, trunc, info = env.step(a)
        else:
            obs, rew, term, trunc, info = env._step_then_post_step(a)
        hs["action"][...] = act
        oracle.env_step(c, world, hs)
        done = (hs["terminated"] | hs["truncated"]).astype(np.uint8)
        R.spawn(c, world, tab, hs, done)
        d = env.state.host()
        keys = [k for k in d if k not in ("action", "slot_cache", "env_cache", "act_cache") and hs[k] is not None]
        _same(hs, d, keys, (A, path, t))
        assert np.array_equal(rew.cpu().numpy(), hs["reward"]) and np.array_equal(term.cpu().numpy(), hs["terminated"].astype(bool))
        assert np.array_equal(info["psi_smoothness"].cpu().numpy(), hs["info"][:, 0])
        assert np.array_equal(info["dist_reward"].cpu().numpy(), hs["info"][:, 3])
        if done.any():
            respawned += int(done.sum())
            if respawned == int(done.sum()) or t == T - 1:    # the birdview right after a re-spawn draws the spawned agents
                assert np.array_equal(obs.cpu().numpy(), oracle.render_ego(c, world, hs, flags=env._rflags)), t
    assert respawned > 0


@pytest.mark.parametrize("obs_mode,binding", [("state", "ext"), ("birdview", "ctypes")])
def test_vec_env_path(tmp_path, obs_mode, binding):
    A = 32
    world, tab = R.validation_world(1, A, tmp_path)
    B = 32
    cfg = EnvConfig(seed=5, distance_cutoff=0.25, max_environment_steps=20, use_background_traffic=False)
    env = BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, near_field=tab, binding=binding, obs_mode=obs_mode)
    venv = env.as_vec_env()
    c = env.tde_cfg
    hs = EnvState(B, A)
    venv.reset()
    oracle.env_reset(c, world, hs)
    R.spawn(c, world, tab, hs)
    rng = np.random.default_rng(1)
    n_done = 0
    for t in range(50):
        act = np.stack([rng.uniform(0.0, 1.0, B), rng.normal(0.0, 0.05, B).clip(-0.3, 0.3)], -1).astype(np.float32)
        _, rew, dones, infos = venv.step(act)
        hs["action"][...] = act
        c2 = _abi.TdeConfig.from_buffer_copy(c)
        c2.flags = c.flags & ~_abi.F_AUTORESET
        oracle.env_step(c2, world, hs)
        done = (hs["terminated"] | hs["truncated"]).astype(np.uint8)
        assert np.array_equal(dones, done.astype(bool)) and np.array_equal(rew, hs["reward"])
        oracle.env_reset(c, world, hs, done)
        R.spawn(c, world, tab, hs, done)
        n_done += int(done.sum())
        _same(hs, env.state.host(), AGENT + ("scn", "episode", "steps"), t)
    assert n_done > 0


def test_two_shards_reproduce_the_unsharded_spawns(worlds):
    world, tab = worlds[64][2]
    B, A = 256, 64
    dw, dnf = world.to_device(DEV, first_gap=False), tab.to_device(DEV)
    cfg = _abi.default_config(seed=9)
    full = EnvState(B, A, device=DEV)
    ops.env_reset(cfg, dw, full)
    ops.near_field_spawn(cfg, dw, full, dnf)
    whole = full.host()
    for lo, hi in ((0, 100), (100, 256)):
        cs = _abi.default_config(seed=9, env_base=lo)
        part = EnvState(hi - lo, A, device=DEV)
        ops.env_reset(cs, dw, part)
        ops.near_field_spawn(cs, dw, part, dnf)
        p = part.host()
        for k in AGENT:
            assert np.array_equal(p[k], whole[k][lo * A:hi * A]), k


def test_density_on_a_town(town):
    """the reference tops the scene up to max(95 - n, agent_density) agents within 120 m of the ego: on a town's streets the
    table reaches that (the candidates within 150 m of the start are the town lattice's)"""
    world, tab = town
    B, A = 256, 128
    cfg = _abi.default_config(seed=2)
    dw, dnf = world.to_device(DEV, first_gap=False), tab.to_device(DEV)
    ds = EnvState(B, A, device=DEV)
    ops.env_reset(cfg, dw, ds)
    ops.near_field_spawn(cfg, dw, ds, dnf)
    h = ds.host()
    x, y = h["x"].reshape(B, A), h["y"].reshape(B, A)
    live = h["present"].reshape(B, A) != 0
    near = live & (np.hypot(x - x[:, :1], y - y[:, :1]) < 120.0)
    assert near.sum(1).mean() >= 60, near.sum(1).mean()


def test_rollout_and_multi_stream_step_refuse_a_near_field(tmp_path):
    world, tab = R.validation_world(0, 16, tmp_path)
    cfg = EnvConfig(seed=1, use_background_traffic=False)
    env = BatchedWaypointEnv(cfg, world, num_envs=64, device=DEV, near_field=tab)
    env.reset()
    with pytest.raises(NotImplementedError, match="near"):
        env.rollout(torch.zeros(4, 64, 2, device=DEV))
    with pytest.raises(NotImplementedError, match="near"):
        ops.env_step_render(env.tde_cfg, env.dworld, env.state, [torch.cuda.Stream(DEV)])
    assert env.dworld.struct.first_gap is None               # near-field envs run without the first-step gap cache
