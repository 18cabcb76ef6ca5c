"""tde_agent_obs and tde_agent_outcomes on the GPU (include/tde_agents.h) against tests/agent_obs_ref.py.  Nothing here has a tolerance:
observation rows, tracks, rewards and flags are compared by bits.  The observation cases share one edited state per (slots, lights) and
one reference per (slots, lights, rays) - the rows of every slot, from which the shorter pair lists take theirs; the closed loop is
tests/agents_cases.py's, which tests/test_agents_cpu.py shows to hold every outcome flag on the references alone."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import agent_obs_ref as ref
from tests import agents_cases as ac
from tests import config_zoo
from torchdriveenv_amd import _abi, ops
from torchdriveenv_amd.config import EnvConfig, RendererConfig, SimulatorConfig, VectorObs
from torchdriveenv_amd.env import AgentGroup, BatchedWaypointEnv
from torchdriveenv_amd.state import EnvState

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 6
K = 8
SENTINEL = np.float32(-7.5)
_DW, _SCENE, _DS, _REF = {}, {}, {}, {}


def _dworld(world):
    if id(world) not in _DW:
        _DW[id(world)] = (world, world.to_device(DEV))
    return _DW[id(world)][1]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def vobs(n_rays):
    return VectorObs(k_neighbours=K, n_rays=n_rays, ray_range=10.0, ray_step=0.5)


def host_scene(A, lights):
    """(cfg, world, host dict) after a reset and two oracle steps, then edited: absent slots; in env 2 the ego and slot 2
    at (x +- 3, y) of slot 1 (equally far: their order is by slot index); in env 3 slot 1 in the corner cell of the map's grid; in
    env 4 slot 1 thirty metres to the side of where it stood (off the road); in env 5 slot 3 and every fourth slot behind it absent"""
    key = (A, lights)
    if key not in _SCENE:
        world = config_zoo.world(None, A)
        cfg = config_zoo.config(None, A, flags=config_zoo.FLAGS if lights else config_zoo.FLAGS & ~_abi.F_TRAFFIC_LIGHTS)
        hs = EnvState(B, A)
        oracle.env_reset(cfg, world, hs)
        acts = config_zoo.actions(None, B, A, T=2)
        for t in range(2):
            hs["action"][...] = acts[t]
            oracle.env_step(cfg, world, hs)
        h = hs.host()
        x, y, psi, pres = (h[k].reshape(B, A) for k in ("x", "y", "psi", "present"))
        pres[1, 2] = 0
        pres[5, 3::4] = 0
        pres[2, 1] = pres[2, 2] = pres[3, 1] = pres[4, 1] = 1
        x[2, 1] = np.round(x[2, 1] * np.float32(4.0)) / np.float32(4.0)              # (a multiple of 0.25: x +- 3 and both differences are exact)
        x[2, 0], y[2, 0] = x[2, 1] + np.float32(3.0), y[2, 1]
        x[2, 2], y[2, 2] = x[2, 1] - np.float32(3.0), y[2, 1]
        m = world.arrays["maps"][int(world.arrays["scn"]["map"][h["scn"][3]])]
        x[3, 1], y[3, 1] = np.float32(m["ox"]) + np.float32(0.3), np.float32(m["oy"]) + np.float32(0.3)
        x[4, 1], y[4, 1] = x[4, 1] - np.float32(30.0) * np.sin(psi[4, 1]), y[4, 1] + np.float32(30.0) * np.cos(psi[4, 1])
        _SCENE[key] = (cfg, world, h)
    return _SCENE[key]


def scene(A, lights):
    """host_scene and the device state that holds it"""
    cfg, world, h = host_scene(A, lights)
    if (A, lights) not in _DS:
        _DS[A, lights] = EnvState(B, A, device=DEV)
        _DS[A, lights].load(h)
    return cfg, world, h, _DS[A, lights]


def all_pairs(A):
    """every slot of every env, then pairs out of range (env and slot, below and above) and duplicates"""
    e, a = np.divmod(np.arange(B * A), A)
    return np.concatenate([np.stack([e, a], -1), [[B, 1], [-1, 0], [0, A], [1, -1], [2, 1], [2, 1], [0, 0]]]).astype(np.int32)


def reference(A, lights, n_rays):
    key = (A, lights, n_rays)
    if key not in _REF:
        cfg, world, h = host_scene(A, lights)
        _REF[key] = ref.agent_obs(cfg, world, h, vobs(n_rays), all_pairs(A))
    return _REF[key]


def gpu_obs(cfg, world, ds, vo, pairs):
    """(rows, track bytes) of ops.agent_obs, with a guard row behind both outputs that must stay as it was"""
    n = len(pairs)
    out = torch.full((n + 1, vo.dim), float(SENTINEL), device=DEV)
    track = torch.full((n + 1, 32), 0xA5, dtype=torch.uint8, device=DEV)
    got = ops.agent_obs(cfg, _dworld(world), ds, vo, dev(pairs), out=out[:n], track=track[:n])
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    assert bool((out[n] == float(SENTINEL)).all()) and bool((track[n] == 0xA5).all())
    return out[:n].cpu().numpy(), track[:n].cpu().numpy()


@pytest.mark.parametrize("lights", [False, True], ids=["nolights", "lights"])
@pytest.mark.parametrize("n_rays", [0, 5, 32])
@pytest.mark.parametrize("A", [4, 16, 128])
def test_agent_obs_equals_the_reference_by_bits(A, n_rays, lights):
    cfg, world, h, ds = scene(A, lights)
    vo = vobs(n_rays)
    pairs = all_pairs(A)
    want, want_track = reference(A, lights, n_rays)
    # the lists: one pair, five (not a multiple of the four pairs of a workgroup; an absent slot, a pair out of range and a duplicate
    # among them), every slot and more
    five = np.array([B * A - 1, 1 * A + 2, B * A + 2, 2 * A + 1, 2 * A + 1])
    for pick in (np.array([2 * A + 1]), five, np.arange(len(pairs))):
        rows, track = gpu_obs(cfg, world, ds, vo, pairs[pick])
        bad = np.flatnonzero((rows.view(np.uint32) != want[pick].view(np.uint32)).any(1))
        assert len(bad) == 0, (len(pick), pairs[pick][bad[:4]], rows[bad[:1]], want[pick][bad[:1]])
        assert np.array_equal(bits(track), bits(want_track[pick]))
    # what the scene was edited for, read from the reference the GPU rows equal
    pres = h["present"].reshape(B, A) != 0
    for i, (e, a) in enumerate(pairs):
        gone = not (0 <= e < B and 0 <= a < A) or not pres[e, a]
        assert gone == (not want_track[i]["present"]) and (not gone or not want[i].any())
    tie = want[2 * A + 1, 10:28].reshape(2, 9)                                       # env 2, slot 1: the ego first, then slot 2, both 3 m away
    xs = h["x"].reshape(B, A)[2]
    assert tie[0, 0] == 1 and tie[1, 0] == 1 and xs[0] - xs[1] == 3.0 and xs[2] - xs[1] == -3.0     # d2 = 9 twice, to the bit
    h0 = np.array([h["len"][2 * A], h["wid"][2 * A]], np.float32)
    assert np.array_equal(tie[0, 7:9], h0) and np.array_equal(tie[1, 7:9], np.array([h["len"][2 * A + 2], h["wid"][2 * A + 2]], np.float32))
    n_valid = want[:B * A, 10:10 + 9 * K:9].sum(1)
    x, y = h["x"].reshape(B, A), h["y"].reshape(B, A)
    d2 = (x[:, :, None] - x[:, None, :]) ** 2 + (y[:, :, None] - y[:, None, :]) ** 2          # [e, observer, other]
    n_cand = ((d2 < np.float32(50.0) ** 2) & pres[:, None, :] & pres[:, :, None] & ~np.eye(A, dtype=bool)).sum(2)
    assert np.array_equal(n_valid.reshape(B, A), np.minimum(n_cand, K))
    assert n_cand.max() < K if A == 4 else n_cand.max() > K and (n_cand[pres] < K).any()   # fewer candidates than entries, and more
    if n_rays:
        road = want[:B * A, 10 + 9 * K::3]
        assert road[3 * A + 1].max() <= 0.5 and road[4 * A + 1].max() <= 0.5      # off the road: the first sample already is
        assert (road == 10.0).any() and (want[:B * A, 11 + 9 * K::3] < 10.0).any() # rays that stay on the road, rays that meet a car


@pytest.mark.parametrize("A", [4, 16, 128])
def test_slot_0_pairs_equal_the_rows_of_tde_vector_obs_and_n_0_launches_nothing(A):
    cfg, world, h, ds = scene(A, True)
    vo = vobs(32)
    pairs = np.stack([np.arange(B), np.zeros(B, np.int64)], -1).astype(np.int32)
    rows, _ = gpu_obs(cfg, world, ds, vo, pairs)
    ego = ops.vector_obs(cfg, _dworld(world), ds, vo).cpu().numpy()
    assert np.array_equal(bits(rows), bits(ego)) and np.any(ego[:, 10:] != 0)
    out = torch.full((3, vo.dim), float(SENTINEL), device=DEV)
    track = torch.full((3, 32), 0xA5, dtype=torch.uint8, device=DEV)
    empty = torch.zeros((0, 2), dtype=torch.int32, device=DEV)
    got = ops.agent_obs(cfg, _dworld(world), ds, vo, empty, out=out[:0], track=track[:0])
    r, f = ops.agent_outcomes(cfg, _dworld(world), ds, empty, track[:0])
    torch.cuda.synchronize()
    assert tuple(got.shape) == (0, vo.dim) and r.numel() == 0 and f.numel() == 0
    assert bool((out == float(SENTINEL)).all()) and bool((track == 0xA5).all())


def test_a_batch_without_envs_gives_zero_rows_and_zero_tracks():
    """B == 0: every pair is out of range; the rows and tracks are zeroed on the stream without a kernel"""
    import ctypes as C

    from torchdriveenv_amd import _lib

    cfg, world, h, ds = scene(4, False)
    vo = vobs(5)
    st = _abi.TdeState.from_buffer_copy(ds.struct)
    st.B = 0
    rd = dev(vo.ray_directions())
    s = _abi.TdeVectorObs(rd.data_ptr(), vo.k_neighbours, vo.n_rays, vo.neighbour_radius, vo.ray_range, vo.ray_step, 0)
    pairs = dev(np.array([[0, 0], [0, 1], [-1, 2]], np.int32))
    out = torch.full((4, vo.dim), float(SENTINEL), device=DEV)
    track = torch.full((4, 32), 0xA5, dtype=torch.uint8, device=DEV)
    rc = _lib.load().tde_agent_obs(C.byref(cfg), C.byref(_dworld(world).struct), C.byref(st), C.byref(s), pairs.data_ptr(), 3, out.data_ptr(),
                                   track.data_ptr(), _lib.current_stream(DEV))
    torch.cuda.synchronize()
    assert rc == 0 and not bool(out[:3].any()) and not bool(track[:3].any())
    assert bool((out[3] == float(SENTINEL)).all()) and bool((track[3] == 0xA5).all())


def test_a_state_with_slot_route_words_takes_the_waypoint_entries_from_them():
    A = 16
    cfg, world, h0, _ = scene(A, False)
    h = {k: np.array(v, copy=True) for k, v in h0.items()}
    rec = world.arrays["spawn"].reshape(-1, A)[h["scn"]]
    e, a = np.nonzero((rec["route"] >= 0) & (rec["route_n"] > 2) & (h["present"].reshape(B, A) != 0) & (np.arange(A) > 0))
    assert len(e) >= 3
    words = np.zeros((B, A), np.uint32)
    words[e[0], a[0]] = (int(rec["route"][e[1], a[1]]) + 1) | (2 << 20)              # two waypoints of another slot's route
    words[e[2], a[2]] = (int(rec["route"][e[0], a[0]]) + 1) | (int(rec["route_n"][e[0], a[0]]) << 20)
    h["slot_route"] = words.reshape(-1)
    h["route_wp"].reshape(B, A)[e[0], a[0]] = 1
    h["route_wp"].reshape(B, A)[e[2], a[2]] = 0
    ds = EnvState(B, A, device=DEV, with_slot_route=True)
    ds.load(h)
    assert ds["slot_route"] is not None and int(ds["slot_route"].count_nonzero()) == 2
    vo = vobs(5)
    pairs = all_pairs(A)
    want, want_track = ref.agent_obs(cfg, world, h, vo, pairs)
    rows, track = gpu_obs(cfg, world, ds, vo, pairs)
    assert np.array_equal(bits(rows), bits(want)) and np.array_equal(bits(track), bits(want_track))
    plain = reference(A, False, 5)[0]
    changed = np.flatnonzero((want[:B * A, 3:8] != plain[:B * A, 3:8]).any(1))
    assert set(changed) == {e[0] * A + a[0], e[2] * A + a[2]} and want[e[0] * A + a[0], 7] == 1


# ---- the closed loop ------------------------------------------------------------------------------------------------------------------
def test_observe_step_outcomes_over_twelve_steps_equal_the_reference_and_hold_every_flag():
    world, cfg = ac.loop_world(), ac.loop_config()
    dw = _dworld(world)
    hs = EnvState(ac.B, ac.A)
    oracle.env_reset(cfg, world, hs)
    h = hs.host()
    ac.loop_stage(h)
    ds = EnvState(ac.B, ac.A, device=DEV)
    ops.env_reset(cfg, dw, ds)
    ds.load(h)
    aa, drv = ac.loop_actions()
    d_aa, d_drv = dev(aa), dev(drv)
    pairs = ac.loop_pairs()
    d_pairs = dev(pairs)
    n = len(pairs)
    acts = config_zoo.actions(None, ac.B, ac.A, T=ac.T)
    vo = VectorObs(k_neighbours=4, n_rays=8, ray_range=10.0, ray_step=0.5)
    track = torch.zeros((n, 32), dtype=torch.uint8, device=DEV)
    count = dict.fromkeys((_abi.AG_COLLIDED, _abi.AG_OFFROAD, _abi.AG_REACHED, _abi.AG_ENDED), 0)
    respawns = 0
    for t in range(ac.T):
        pre = ds.host()
        rows = ops.agent_obs(cfg, dw, ds, vo, d_pairs, track=track)
        ds["action"].copy_(dev(acts[t]))
        ops.env_step_driven(cfg, dw, ds, d_aa, d_drv)
        reward, flags = ops.agent_outcomes(cfg, dw, ds, d_pairs, track)
        post = ds.host()
        want_rows, want_track = ref.agent_obs(cfg, world, pre, vo, pairs)
        want_reward, want_flags = ref.agent_outcomes(cfg, world, post, pairs, want_track)
        assert np.array_equal(bits(rows.cpu().numpy()), bits(want_rows)), t
        assert np.array_equal(bits(track.cpu().numpy()), bits(want_track)), t
        got_flags, got_reward = flags.cpu().numpy(), reward.cpu().numpy()
        assert np.array_equal(got_flags, want_flags), (t, np.flatnonzero(got_flags != want_flags)[:8])
        diff = np.flatnonzero(got_reward.view(np.uint32) != want_reward.view(np.uint32))
        assert len(diff) == 0, (t, pairs[diff[:4]], got_reward[diff[:4]], want_reward[diff[:4]])
        for b in count:
            count[b] += int(((got_flags & b) != 0).sum())
        respawns += int((post["episode"] != pre["episode"]).sum())
        assert (got_reward[(got_flags & _abi.AG_VALID) != 0] != 0).any() or (got_flags & _abi.AG_ENDED).any()
    assert all(count.values()) and respawns >= ac.B, count


# ---- the env --------------------------------------------------------------------------------------------------------------------------
def make_env(world, n, obs_mode, **kw):
    cfg = EnvConfig(seed=11, distance_cutoff=0.25, max_environment_steps=3, simulator=SimulatorConfig(renderer=RendererConfig(res=64)))
    return BatchedWaypointEnv(cfg, world, num_envs=n, device=DEV, obs_mode=obs_mode, **kw)


@pytest.mark.parametrize("obs_mode,kw", [("state", {}), ("vector", dict(vector_obs=VectorObs(k_neighbours=2, n_rays=4)))], ids=["state", "vector"])
def test_an_agent_group_of_the_env_gives_what_the_ops_calls_give(obs_mode, kw):
    A, n_envs = 16, 6
    world = config_zoo.world(None, A)
    env = make_env(world, n_envs, obs_mode, **kw)
    env.reset()
    envs, slots = [0, 1, 2, 3, 4, 5, 5, 0], [1, 1, 2, 3, 1, 15, 15, 0]
    group = env.agents(envs, slots)
    assert isinstance(group, AgentGroup) and group.n == 8
    assert group.vector_obs == (kw["vector_obs"] if kw else VectorObs())
    own = env.agents(torch.tensor(envs), torch.tensor(slots), vector_obs=dict(k_neighbours=1, n_rays=0))
    assert own.vector_obs.dim == 19
    pairs = dev(np.stack([envs, slots], -1).astype(np.int32))
    assert torch.equal(group.pairs, pairs)
    drv = torch.zeros((n_envs, A), dtype=torch.bool, device=DEV)
    drv[envs, slots] = True
    aa = torch.zeros((n_envs, A, 2), device=DEV)
    aa[..., 0] = 2.0
    acts = config_zoo.actions(None, n_envs, A, T=4)
    ended = 0
    for t in range(4):
        obs = group.observe()
        track = torch.zeros((8, 32), dtype=torch.uint8, device=DEV)
        want = ops.agent_obs(env.tde_cfg, env.dworld, env.state, group.vector_obs, pairs, track=track)
        assert obs.dtype == torch.float32 and tuple(obs.shape) == (8, group.vector_obs.dim) and torch.equal(obs.view(torch.int32), want.view(torch.int32))
        assert torch.equal(group.track, track) and int(track[:, 28].sum()) >= 6
        assert tuple(own.observe().shape) == (8, 19)
        env.step(dev(acts[t]), aa, drv)
        out = group.outcomes()
        reward, flags = out
        want_r, want_f = ops.agent_outcomes(env.tde_cfg, env.dworld, env.state, pairs, track)
        assert reward.dtype == torch.float32 and flags.dtype == torch.uint8 and tuple(reward.shape) == tuple(flags.shape) == (8,)
        assert torch.equal(reward.view(torch.int32), want_r.view(torch.int32)) and torch.equal(flags, want_f)
        for name, bit in (("valid", 1), ("collided", 2), ("offroad", 4), ("reached", 8), ("ended", 16)):
            view = getattr(out, name)
            assert view.dtype == torch.bool and torch.equal(view, (flags & bit) != 0)
        assert not bool(out.valid[7]) and bool(out.valid[:5].all())                  # slot 0 is reported invalid
        ended += int(out.ended.sum())
    assert ended > 0                                                               # 3-step episodes: the envs were re-spawned
    with pytest.raises(ValueError, match=r"^slots must be in \[0, 16\)$"):
        env.agents([0], [16])
    with pytest.raises(ValueError, match=r"^envs must be in \[0, 6\)$"):
        env.agents([6], [1])
    with pytest.raises(ValueError, match="^envs and slots must have one length, got 2 and 1$"):
        env.agents([0, 1], [1])
