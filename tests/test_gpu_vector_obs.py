"""tde_vector_obs on the GPU against its numpy restatement (tests/vector_obs_ref.py), bit for bit: the kernel through both bindings on
a junction world, a validation world, a town (the large-grid path), 128 crowded slots, a lights world across its phases, egos near
and beyond the grid edge and off the road, `only` masks; BatchedWaypointEnv(obs_mode="vector") in closed loop with auto-reset and a
near field; the VecEnv's terminal observations; two shards against one unsharded batch."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import near_field_ref as NF
from tests import plan_set_ref as S
from tests import vector_obs_ref as R
from tests.plan_gpu_util import bits, on_device
from torchdriveenv_amd import _abi, _ext, ops
from torchdriveenv_amd.config import EnvConfig, VectorObs
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.state import EnvState

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(cfg, world, hs, vo, only=None, what=""):
    """the kernel (both bindings) on the device copy of host state `hs` == the restatement; returns the rows"""
    B = len(hs["scn"])
    want = R.vector_obs(cfg, world, hs, vo, only=only, out=np.full((B, vo.dim), -3.0, np.float32) if only is not None else None)
    dw, ds = on_device(world, hs)
    rd = torch.from_numpy(vo.ray_directions()).to(DEV)
    m = torch.from_numpy(np.asarray(only, np.uint8)).to(DEV) if only is not None else None
    for binding in ("ctypes", "ext"):
        out = torch.full((B, vo.dim), -3.0, dtype=torch.float32, device=DEV)
        if binding == "ctypes":
            ops.vector_obs(cfg, dw, ds, vo, rd, out, m)
        else:
            _ext.env_handle(cfg, dw, ds).vector_obs(out, rd, vo.k_neighbours, vo.n_rays, vo.neighbour_radius, vo.ray_range,
                                                    vo.ray_step, m, int(cfg.flags))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        bad = np.argwhere(bits(got) != bits(want))
        assert len(bad) == 0, (what, binding, bad[:8].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return want


VOS = [VectorObs(), VectorObs(k_neighbours=16, n_rays=64, ray_range=30.0, ray_step=0.25, neighbour_radius=80.0),
       VectorObs(k_neighbours=3, n_rays=7, ray_range=120.0, ray_step=2.0, neighbour_radius=15.0)]


@pytest.mark.parametrize("v", range(len(VOS)))
def test_junction_world_at_16_slots(small_world, v):
    cfg = S.lights_cfg(small_world, seed=3)
    hs = S.reset_state(cfg, small_world, 256)
    rows = _check(cfg, small_world, hs, VOS[v], what="junctions")
    vo = VOS[v]
    sl = vo.slices()
    assert (rows[:, sl["road"]] < vo.ray_range).any() and (rows[:, sl["car"]] < vo.ray_range).any()
    assert rows[:, sl["neighbours"]][:, 0::9].any()


def test_validation_world_and_only_masks(tmp_path):
    world, _ = NF.validation_world(0, 16, tmp_path)
    cfg = _abi.default_config(seed=8)
    hs = S.reset_state(cfg, world, 200)
    _check(cfg, world, hs, VectorObs(), what="validation")
    only = (np.random.default_rng(0).random(200) < 0.3).astype(np.uint8)
    _check(cfg, world, hs, VectorObs(), only=only, what="validation only")
    _check(cfg, world, hs, VectorObs(), only=np.zeros(200, np.uint8), what="validation none")


def test_town_large_grid(small_town):
    cfg = S.lights_cfg(small_town, seed=4)
    hs = S.reset_state(cfg, small_town, 128)
    hs["steps"][...] = np.arange(128) * 3
    rows = _check(cfg, small_town, hs, VectorObs(n_rays=48), what="town")
    assert (rows[:, VectorObs(n_rays=48).slices()["road"]] < 50.0).any()


def test_town_reference_size_large_grid(town):
    assert town.arrays["maps"]["nx"].max() * town.arrays["maps"]["ny"].max() > 2 ** 21       # (TDE_WORLD_LARGE_GRID)
    cfg = S.lights_cfg(town, seed=6)
    hs = S.reset_state(cfg, town, 64)
    _check(cfg, town, hs, VectorObs(k_neighbours=4, n_rays=16), what="town 1 km")


def test_128_crowded_slots():
    from torchdriveenv_amd.synth import synthetic_world

    world = synthetic_world(n_scn=4, A=128, seed=5, n_maps=2)
    cfg = S.lights_cfg(world, seed=5)
    B, A = 64, 128
    hs = S.reset_state(cfg, world, B)
    rng = np.random.default_rng(7)
    x, y = hs["x"].reshape(B, A), hs["y"].reshape(B, A)
    # every slot present, scattered within 40 m of the ego; a few exact distance ties
    x[:, 1:] = x[:, :1] + rng.uniform(-40, 40, (B, A - 1)).astype(np.float32)
    y[:, 1:] = y[:, :1] + rng.uniform(-40, 40, (B, A - 1)).astype(np.float32)
    x[:, 20], y[:, 20] = x[:, 0] + 3.0, y[:, 0]
    x[:, 90], y[:, 90] = x[:, 0] - 3.0, y[:, 0]
    hs["psi"].reshape(B, A)[:, 1:] = rng.uniform(-3.1, 3.1, (B, A - 1)).astype(np.float32)
    hs["v"].reshape(B, A)[:, 1:] = rng.uniform(0, 12, (B, A - 1)).astype(np.float32)
    hs["present"][...] = 1
    for vo in (VectorObs(k_neighbours=16, n_rays=64), VectorObs(k_neighbours=5, n_rays=3, neighbour_radius=20.0)):
        rows = _check(cfg, world, hs, vo, what="crowded")
        assert rows[:, vo.slices()["neighbours"]].reshape(B, -1, 9)[:, :, 0].all()


def test_lights_across_phase_changes(small_world):
    cfg = S.lights_cfg(small_world, seed=11)
    assert cfg.flags & _abi.F_TRAFFIC_LIGHTS
    B = 256
    hs = S.reset_state(cfg, small_world, B)
    vo = VectorObs(n_rays=64, ray_range=60.0)
    seen = []
    for k in (0, 40, 79, 80, 95, 120, 145, 159, 160, 400):
        hs["steps"][...] = k
        rows = _check(cfg, small_world, hs, vo, what=("lights", k))
        seen.append((rows[:, vo.slices()["red_line"]] < vo.ray_range).sum())
    assert min(seen) > 0 and len(set(seen)) > 1                      # red lines seen, and which ones changes with the phase


def test_egos_near_the_grid_edge_and_offroad(small_world):
    cfg = S.lights_cfg(small_world, seed=12)
    B, A = 192, small_world.A
    hs = S.reset_state(cfg, small_world, B)
    mp = small_world.arrays["maps"]
    m = small_world.map_of_scn()[hs["scn"]]
    ox, oy = mp["ox"][m], mp["oy"][m]
    h = mp["ny"][m] * mp["cell"][m]
    rng = np.random.default_rng(2)
    x0, y0 = hs["x"][::A].astype(np.float64), hs["y"][::A].astype(np.float64)
    a, b = slice(0, B // 3), slice(B // 3, 2 * (B // 3))
    n = B // 3
    # near the edge (inside), beyond it by 1 to 30 m (the clamp to the EMPTY border), and a few metres off the road
    x0[a] = ox[a] + rng.uniform(0.2, 3.0, n)
    y0[a] = oy[a] + rng.uniform(0.0, 1.0, n) * h[a]
    x0[b] = ox[b] - rng.uniform(1.0, 30.0, n)
    y0[b] = oy[b] + rng.uniform(-10.0, 30.0, n) + h[b]
    x0[2 * n:] += rng.uniform(8.0, 14.0, B - 2 * n)
    hs["x"][::A], hs["y"][::A] = x0.astype(np.float32), y0.astype(np.float32)
    hs["psi"][::A] = rng.uniform(-3.14, 3.14, B).astype(np.float32)
    vo = VectorObs(n_rays=64, ray_range=40.0, ray_step=0.5)
    rows = _check(cfg, small_world, hs, vo, what="edge")
    road = rows[:, vo.slices()["road"]]
    assert (road[b] == vo.ray_step).all()                            # off the grid: the first sample is already off the road
    assert (road[a] < vo.ray_range).any()


@pytest.mark.parametrize("binding", ["ext", "ctypes"])
def test_closed_loop_with_auto_reset_and_near_field(tmp_path, binding):
    A = 16
    world, tab = NF.validation_world(0, A, tmp_path)
    B = 48
    cfg = EnvConfig(seed=21, distance_cutoff=0.25, max_environment_steps=20, use_background_traffic=False)
    vo = VectorObs(k_neighbours=6, n_rays=24, ray_range=40.0)
    env = BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, near_field=tab, binding=binding, obs_mode="vector", vector_obs=vo)
    assert env.observation_space.shape == (vo.dim,) and env.observation_space.dtype == np.float32
    c = env.tde_cfg
    hs = EnvState(B, A)
    obs = env.reset()
    oracle.env_reset(c, world, hs)
    NF.spawn(c, world, tab, hs)
    assert np.array_equal(bits(obs.cpu().numpy()), bits(R.vector_obs(c, world, hs, vo)))
    rng = np.random.default_rng(4)
    respawned = 0
    for t in range(50):
        act = np.stack([rng.uniform(-0.2, 1.0, B), rng.normal(0.0, 0.08, B).clip(-0.3, 0.3)], -1).astype(np.float32)
        obs, rew, term, trunc, info = env.step(torch.from_numpy(act).to(DEV))
        hs["action"][...] = act
        oracle.env_step(c, world, hs)
        done = (hs["terminated"] | hs["truncated"]).astype(np.uint8)
        NF.spawn(c, world, tab, hs, done)
        respawned += int(done.sum())
        assert np.array_equal(bits(obs.cpu().numpy()), bits(R.vector_obs(c, world, hs, vo))), t
    assert respawned > 0
    # masked reset: only the masked rows change
    before = obs.clone()
    mask = np.zeros(B, np.uint8)
    mask[::5] = 1
    obs = env.reset(mask=torch.from_numpy(mask).to(DEV))
    keep = mask == 0
    assert torch.equal(obs[torch.from_numpy(keep).to(DEV)], before[torch.from_numpy(keep).to(DEV)])
    hs2 = env.state.host()
    assert np.array_equal(bits(obs.cpu().numpy()), bits(R.vector_obs(c, world, hs2, vo)))


def test_vec_env_terminal_observations(small_world):
    cfg = EnvConfig(seed=33, distance_cutoff=0.25, max_environment_steps=15)
    B = 64
    vo = VectorObs(k_neighbours=4, n_rays=16)
    venv = BatchedWaypointEnv(cfg, small_world, num_envs=B, device=DEV, obs_mode="vector", vector_obs=vo).as_vec_env()
    ref = BatchedWaypointEnv(cfg, small_world, num_envs=B, device=DEV, obs_mode="vector", vector_obs=vo, auto_reset=False)
    o1 = venv.reset()
    o2 = ref.reset().cpu().numpy()
    assert o1.shape == (B, vo.dim) and o1.dtype == np.float32 and np.array_equal(bits(o1), bits(o2))
    rng = np.random.default_rng(9)
    n_done = 0
    for t in range(40):
        act = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
        o1, r1, d1, infos = venv.step(act)
        pre, _, term, trunc, _ = ref.step(torch.from_numpy(act).to(DEV))
        pre = pre.cpu().numpy().copy()
        done = (term | trunc).cpu().numpy()
        assert np.array_equal(d1, done)
        if done.any():
            post = ref.reset(mask=torch.from_numpy(done.astype(np.uint8)).to(DEV)).cpu().numpy()
        else:
            post = pre
        assert np.array_equal(bits(o1), bits(post)), t
        for i in np.flatnonzero(done):
            assert np.array_equal(bits(infos[i]["terminal_observation"]), bits(pre[i])), (t, i)
        n_done += int(done.sum())
    assert n_done > 0


def test_two_shards_equal_the_unsharded_batch(small_world):
    from torchdriveenv_amd.sharding import ShardedBatchedEnv

    cfg = EnvConfig(seed=52, distance_cutoff=0.25, max_environment_steps=25)
    B = 64
    vo = VectorObs(k_neighbours=5, n_rays=12)
    one = BatchedWaypointEnv(cfg, small_world, num_envs=B, device=DEV, obs_mode="vector", vector_obs=vo).as_vec_env()
    two = ShardedBatchedEnv(cfg, small_world, B, n_shards=2, devices=[0, 0], obs_mode="vector", vector_obs=vo)
    try:
        oa, ob = one.reset(), two.reset()
        assert ob.shape == (B, vo.dim) and ob.dtype == np.float32 and np.array_equal(bits(oa), bits(ob))
        rng = np.random.default_rng(3)
        n_done = 0
        for t in range(40):
            acts = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
            oa, ra, da, ia = one.step(acts)
            ob, rb, db, ib = two.step(acts)
            assert np.array_equal(bits(oa), bits(ob)) and np.array_equal(da, db), t
            for i in np.nonzero(da)[0]:
                assert np.array_equal(bits(ia[i]["terminal_observation"]), bits(ib[i]["terminal_observation"]))
            n_done += int(da.sum())
        assert n_done > 0
    finally:
        two.close()
