"""GPU parity / semantics of the round-2 additions, through the C-ABI: stop-line layer and left-handed raster pixel-exact
against the oracle, masked / fresh frame-stack calls, both readings of the offroad threshold, Monitor-style episode
statistics, VecFrameStack semantics of the batched env (device path and SB3 path), the SB3 VecEnv adapter."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle  # noqa: E402
from torchdriveenv_amd import _abi, ops  # noqa: E402
from torchdriveenv_amd.config import EnvConfig, RendererConfig, SimulatorConfig  # noqa: E402
from torchdriveenv_amd.env import BatchedWaypointEnv, LazyInfos, WaypointVecEnv  # noqa: E402
from torchdriveenv_amd.state import EnvState  # noqa: E402

DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _pair(world, B, A, cfg):
    hs, ds = EnvState(B, A), EnvState(B, A, device=DEV)
    oracle.env_reset(cfg, world, hs)
    ds.load(hs.host())
    return hs, ds, world.to_device(DEV)


def _step_both(cfg, world, dw, hs, ds, rng, n=1):
    for _ in range(n):
        act = np.stack([rng.uniform(0, 1, hs.B), rng.uniform(-0.2, 0.2, hs.B)], -1).astype(np.float32)
        hs["action"][...] = act
        ds["action"].copy_(dev(act))
        oracle.env_step(cfg, world, hs)
        ops.env_step(cfg, dw, ds)


@pytest.mark.parametrize("A,flags", [(16, 0), (16, _abi.RENDER_LEFT_HANDED), (32, _abi.RENDER_LEFT_HANDED | _abi.RENDER_PLAIN_EGO)])
def test_render_with_lights_and_flags_bit_exact(A, flags):
    """every pixel equals the oracle's with the traffic-control layer on (stop lines coloured by the light state at the
    env's step), in the right- and left-handed raster, with and without the ego highlight; BASELINE configs[4] shape"""
    from torchdriveenv_amd.synth import synthetic_world

    world = synthetic_world(n_scn=6, A=A, seed=3, n_maps=2)
    cfg = _abi.default_config(seed=8, flags=_abi.F_ALL | _abi.F_TRAFFIC_LIGHTS, terminated_at_infraction=0)
    B = 24
    hs, ds, dw = _pair(world, B, A, cfg)
    rng = np.random.default_rng(4)
    RED, GO = _abi.PALETTE[_abi.LAYER_STOP_RED], _abi.PALETTE[_abi.LAYER_STOP_GO]
    seen = {RED: 0, GO: 0}
    maps, stops, scn_map = world.arrays["maps"], world.arrays["stoplines"], world.arrays["scn"]["map"]
    for t in range(10):
        _step_both(cfg, world, dw, hs, ds, rng, 4)
        if t % 2:                                         # park half of the egos in front of a stop line of their map
            for e in range(0, B, 2):
                m = maps[scn_map[hs["scn"][e]]]
                sl = stops[m["stop_base"] + (e // 2) % m["n_stop"]]
                g = e * A
                hs["x"][g], hs["y"][g] = sl["x"] - 5.0 * sl["c"], sl["y"] - 5.0 * sl["s"]
                hs["psi"][g] = np.arctan2(sl["s"], sl["c"]) + 0.3
            ds.load(hs.host())
        want = oracle.render_ego(cfg, world, hs, flags=flags)
        got = ops.render_ego(cfg, dw, ds, flags=flags).cpu().numpy()
        assert np.array_equal(got, want), f"{(got != want).sum()} pixels differ at t={t}"
        px = want.transpose(0, 2, 3, 1).reshape(-1, 3)
        for col in seen:
            seen[col] += int((px == np.array(col)).all(1).sum())
    assert seen[RED] > 50 and seen[GO] > 50               # both light states were on screen


def test_render_overlapping_stop_lines_paint_in_index_order():
    """two stop lines that overlap and show different light states: the oracle paints them in index order (the later one
    wins where they overlap); the rasteriser culls them with an order-preserving compaction and paints one after the
    other inside one wavefront, so it must give the same pixels whatever the lights show"""
    from torchdriveenv_amd.synth import synthetic_world

    world = synthetic_world(n_scn=4, A=16, seed=3, n_maps=2)
    st = world.arrays["stoplines"]
    maps = world.arrays["maps"]
    for m in maps:                                        # line 1 of every map is laid across line 0, rotated by 0.5 rad
        a, b = st[m["stop_base"]], st[m["stop_base"] + 1]
        b["x"], b["y"] = a["x"] + 0.4, a["y"] - 0.3
        ang = np.arctan2(a["s"], a["c"]) + 0.5
        b["c"], b["s"] = np.cos(ang), np.sin(ang)
    world._host_struct = None
    cfg = _abi.default_config(seed=2, flags=_abi.F_ALL | _abi.F_TRAFFIC_LIGHTS, terminated_at_infraction=0, max_steps=10**6)
    B, A = 16, 16
    hs, ds, dw = _pair(world, B, A, cfg)
    scn_map = world.arrays["scn"]["map"]
    RED, GO = _abi.PALETTE[_abi.LAYER_STOP_RED], _abi.PALETTE[_abi.LAYER_STOP_GO]
    both = 0
    for k in (3, 85, 100, 150):                           # different phases of the cycle: (red, go), (red, red), (go, red) ...
        for e in range(B):
            m = maps[scn_map[hs["scn"][e]]]
            sl = st[m["stop_base"]]
            g = e * A
            hs["x"][g], hs["y"][g] = sl["x"] - 3.0 * sl["c"], sl["y"] - 3.0 * sl["s"]
            hs["psi"][g] = np.arctan2(sl["s"], sl["c"]) + 0.1 * e
            hs["steps"][e] = k + e
        ds.load(hs.host())
        want = oracle.render_ego(cfg, world, hs)
        got = ops.render_ego(cfg, dw, ds).cpu().numpy()
        assert np.array_equal(got, want), f"{(got != want).sum()} pixels differ at k={k}"
        px = want.transpose(0, 2, 3, 1).reshape(B, -1, 3)
        both += sum(int((p == np.array(RED)).all(1).any() and (p == np.array(GO)).all(1).any()) for p in px)
    assert both > 4                                       # views showing a red and a green line at once


def test_state_load_of_an_edited_device_snapshot_drops_the_step_caches(small_world):
    """`h = st.host(); h['x'] += ...; st.load(h)`: the snapshot of a DEVICE state carries its lookup / action caches, keyed
    by the episode / step counters only - reloading them would apply NPC actions computed for the old poses"""
    cfg = _abi.default_config(seed=4, distance_cutoff=0.25)
    B, A = 64, 16
    hs, ds, dw = _pair(small_world, B, A, cfg)
    rng = np.random.default_rng(1)
    _step_both(cfg, small_world, dw, hs, ds, rng, 5)      # (the three-role step kernel fills the caches)
    akeys = lambda: ds["act_cache"].view(ds.B, ds.A + 1, 2)[:, ds.A, 0]   # noqa: E731  (the per-env key entries: episode)
    assert int((akeys() >= 0).sum()) > 0
    h = ds.host()
    shift = rng.uniform(-1.5, 1.5, B * A).astype(np.float32)
    h["x"] = h["x"] + shift
    ds.load(h)
    assert int((akeys() >= 0).sum()) == 0   # invalidated, not restored
    hs["x"][...] = hs["x"] + shift
    _step_both(cfg, small_world, dw, hs, ds, rng, 3)
    for k in ("x", "y", "psi", "v", "collided", "offroad", "reward"):
        assert np.array_equal(ds[k].cpu().numpy().view(np.uint8), hs[k].view(np.uint8)), k


def test_operator_level_entry_points_through_the_extension(small_world, golden):
    """the four SimulatorInterface-level entry points bound in the PyTorch-ROCm extension (kinematics_step,
    compute_collision, compute_offroad, waypoint_reward) give the bits of the ctypes binding and of the oracle"""
    import ctypes as C

    from tests.golden_util import case_config, case_expected, case_inputs
    from torchdriveenv_amd import _ext

    X = _ext.load()
    cfg = _abi.default_config(seed=9)
    B, A = 48, 16
    hs, ds, dw = _pair(small_world, B, A, cfg)
    rng = np.random.default_rng(3)
    _step_both(cfg, small_world, dw, hs, ds, rng, 8)
    h = hs.host()
    n = B * A
    # kinematics
    act = np.stack([rng.uniform(-1, 1, n), rng.uniform(-0.3, 0.3, n)], -1).astype(np.float32)
    a1 = [dev(h[k].copy()) for k in ("x", "y", "psi", "v")]
    a2 = [dev(h[k].copy()) for k in ("x", "y", "psi", "v")]
    X.kinematics_step(*a1, dev(h["lr"]), dev(act), dev(h["present"]), 0.1)
    ops.kinematics_step(*a2, dev(h["lr"]), dev(act), present=dev(h["present"]), dt=0.1)
    want = [h[k].copy() for k in ("x", "y", "psi", "v")]
    oracle.kinematics_step(*want, h["lr"], h["present"], act, 0.1)
    for t1, t2, w in zip(a1, a2, want):
        assert torch.equal(t1, t2) and np.array_equal(t1.cpu().numpy().view(np.uint32), w.view(np.uint32))
    # collision / offroad
    args = [dev(h[k]) for k in ("x", "y", "psi", "len", "wid", "present")]
    c1, c2 = X.compute_collision(B, A, *args), ops.compute_collision(B, A, *args)
    assert torch.equal(c1, c2) and np.array_equal(c1.cpu().numpy(), oracle.compute_collision(B, A, *[h[k] for k in ("x", "y", "psi", "len", "wid", "present")]))
    mo = np.ascontiguousarray(small_world.arrays["scn"]["map"][h["scn"]].astype(np.int32))
    o1 = X.compute_offroad(B, A, *args, _ext.world_of(dw), dev(mo), 0.5)
    o2 = ops.compute_offroad(B, A, *args, dw, dev(mo), threshold=0.5)
    assert torch.equal(o1, o2) and np.array_equal(o1.cpu().numpy(), oracle.compute_offroad(B, A, *[h[k] for k in ("x", "y", "psi", "len", "wid", "present")], small_world, mo, threshold=0.5))
    # the reference-owned reward logic on a golden case
    case = golden["cases"][0]
    ccfg, inp, exp = case_config(case), case_inputs(case), case_expected(case)
    steps, target, reached = dev(inp["steps"].copy()), dev(inp["target"].copy()), dev(inp["reached"].copy())
    out = X.waypoint_reward(_ext.config_of(ccfg), dev(np.ascontiguousarray(inp["pre"].T)), dev(np.ascontiguousarray(inp["post"].T)),
                            dev(inp["off"]), dev(inp["col"]), dev(inp["tl"]), dev(inp["wp"]), dev(inp["wp_n"]), dev(inp["scn"]),
                            steps, target, reached)
    reward, term, trunc, info, info_reached = [t.cpu().numpy() for t in out]
    assert np.array_equal(reward.astype(np.float64), exp["reward"]) and np.array_equal(term, exp["terminated"])
    assert np.array_equal(trunc, exp["truncated"]) and np.array_equal(target.cpu().numpy(), exp["target_after"])
    assert np.array_equal(info_reached, exp["reached"]) and np.allclose(info, exp["info"], rtol=1e-12, atol=1e-15)
    with pytest.raises(RuntimeError):
        X.compute_collision(B, A, *[t.cpu() for t in args])                   # host tensors are refused, not dereferenced
    # typed carriers: no raw address is accepted any more; wrong sizes / dtypes / unknown names are refused with the field's name
    with pytest.raises(TypeError):
        X.compute_offroad(B, A, *args, C.addressof(dw.struct), dev(mo), 0.5)
    with pytest.raises(RuntimeError, match="bytes"):
        X.Config(b"\0" * 8)
    st = EnvState(B, A, device=DEV)
    tens = {k: v for k, v in st.arrays.items() if v is not None}
    with pytest.raises(RuntimeError, match="psi"):
        X.EnvHandle(_ext.config_of(ccfg), _ext.world_of(dw), {**tens, "psi": tens["psi"][:-1]}, B, A)
    with pytest.raises(RuntimeError, match="steps"):
        X.EnvHandle(_ext.config_of(ccfg), _ext.world_of(dw), {**tens, "steps": tens["steps"].float()}, B, A)
    with pytest.raises(RuntimeError, match="lacks"):
        X.EnvHandle(_ext.config_of(ccfg), _ext.world_of(dw), {k: v for k, v in tens.items() if k != "x"}, B, A)
    with pytest.raises(RuntimeError, match="no field"):
        X.EnvHandle(_ext.config_of(ccfg), _ext.world_of(dw), {**tens, "bogus": tens["x"]}, B, A)


def test_sharded_env_argument_checks(small_world):
    from torchdriveenv_amd.sharding import ShardedBatchedEnv

    with pytest.raises(ValueError, match="n_shards"):
        ShardedBatchedEnv(EnvConfig(seed=1), small_world, total_envs=3, n_shards=4)


def test_render_masked_and_fresh_calls_match_oracle(small_world):
    """tde_render.only / .fresh with the in-place stack and with the layer ring: same pixels as the oracle"""
    cfg = _abi.default_config(seed=12, flags=_abi.F_ALL | _abi.F_TRAFFIC_LIGHTS)
    B, A = 20, 16
    hs, ds, dw = _pair(small_world, B, A, cfg)
    rng = np.random.default_rng(2)
    ring = ops.FrameStack(B, 3, device=DEV)
    hout = dout = None
    for t in range(9):
        _step_both(cfg, small_world, dw, hs, ds, rng, 2)
        fresh = np.zeros(B, np.uint8)
        if t % 3 == 1:
            fresh[rng.integers(0, B, 4)] = rng.integers(1, 4, 4)                 # done-bit patterns
            fresh[rng.integers(0, B, 2)] = 4 | 8                                  # infraction bits only: not fresh
        hout = oracle.render_ego(cfg, small_world, hs, n_stack=3, out=hout, fresh=fresh)
        dout = ops.render_ego(cfg, dw, ds, n_stack=3, out=dout, fresh=dev(fresh))
        r = ring.render(cfg, dw, ds, fresh=dev(fresh))
        assert np.array_equal(dout.cpu().numpy(), hout) and np.array_equal(r.cpu().numpy(), hout), t
        if t % 3 == 2:                                    # some envs are re-spawned between two steps: masked call
            mask = np.zeros(B, np.uint8)
            mask[rng.integers(0, B, 5)] = 1
            oracle.env_reset(cfg, small_world, hs, mask)
            ops.env_reset(cfg, dw, ds, dev(mask))
            hout = oracle.render_ego(cfg, small_world, hs, n_stack=3, out=hout, fresh=mask, only=mask)
            dout = ops.render_ego(cfg, dw, ds, n_stack=3, out=dout, fresh=dev(mask), only=dev(mask))
            r = ring.rerender(cfg, dw, ds, dev(mask))
            assert np.array_equal(dout.cpu().numpy(), hout) and np.array_equal(r.cpu().numpy(), hout), t
        if t % 3 == 0 and t:                              # the same as ONE call: tde_env_reset_render (in place and on the ring)
            mask = np.zeros(B, np.uint8)
            mask[rng.integers(0, B, 6)] = 1
            ds2 = EnvState(B, A, device=DEV)              # a second device state for the in-place form
            ds2.load(hs.host())
            oracle.env_reset(cfg, small_world, hs, mask)
            hout = oracle.render_ego(cfg, small_world, hs, n_stack=3, out=hout, fresh=mask, only=mask)
            dout = ops.env_reset_render(cfg, dw, ds2, dev(mask), dout, n_stack=3)
            r = ring.reset_rerender(cfg, dw, ds, dev(mask))
            assert np.array_equal(dout.cpu().numpy(), hout) and np.array_equal(r.cpu().numpy(), hout), t
            for k in ("x", "y", "psi", "v", "episode", "steps", "scn", "target_idx", "present", "route_wp"):
                assert np.array_equal(ds[k].cpu().numpy().view(np.uint8), hs.host()[k].view(np.uint8)), k
                assert np.array_equal(ds2[k].cpu().numpy().view(np.uint8), hs.host()[k].view(np.uint8)), k
    with pytest.raises(Exception, match="mask"):
        ops.env_reset_render(cfg, dw, ds, None, dout, n_stack=3)
    assert ring.phase in (0, 1, 2)
    with pytest.raises(Exception):
        ops.render_ego(cfg, dw, ds, n_stack=3, out=dout, layers=ring.layers, phase=-1)


@pytest.mark.parametrize("squared", [False, True])
def test_offroad_threshold_both_readings_bit_exact(squared):
    """grid index (built for the effective distance) vs the oracle's brute force, threshold on the distance and on the
    squared distance: masks equal, and the two readings differ on agents that straddle the road edge"""
    from torchdriveenv_amd.synth import synthetic_world
    from torchdriveenv_amd.world import effective_offroad_distance

    world = synthetic_world(n_scn=8, A=16, seed=0, n_maps=2, threshold=effective_offroad_distance(0.5, squared))
    cfg = _abi.default_config(seed=3, offroad_threshold=0.5, offroad_threshold_squared=int(squared),
                              terminated_at_infraction=0)
    B, A = 96, 16
    hs, ds, dw = _pair(world, B, A, cfg)
    rng = np.random.default_rng(7)
    n_off = 0
    for t in range(40):
        act = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
        hs["action"][...] = act
        ds["action"].copy_(dev(act))
        oracle.env_step(cfg, world, hs)
        ops.env_step(cfg, dw, ds)
        assert np.array_equal(ds["offroad"].cpu().numpy(), hs["offroad"]), t
        n_off += int(hs["offroad"].sum())
    for k in ("x", "y", "psi", "v", "reward"):
        assert np.array_equal(ds[k].cpu().numpy().view(np.uint32), hs[k].view(np.uint32)), k
    assert n_off > 0
    # operator form against brute force on boxes pushed across the road edge
    h = hs.host()
    y = (h["y"] + rng.uniform(-4, 4, B * A)).astype(np.float32)
    mo = np.ascontiguousarray(world.arrays["scn"]["map"][h["scn"]].astype(np.int32))
    thr = float(np.sqrt(0.5)) if squared else 0.5
    want = oracle.compute_offroad(B, A, h["x"], y, h["psi"], h["len"], h["wid"], h["present"], world, mo, threshold=thr)
    got = ops.compute_offroad(B, A, dev(h["x"]), dev(y), dev(h["psi"]), dev(h["len"]), dev(h["wid"]), dev(h["present"]),
                              dw, dev(mo), threshold=thr).cpu().numpy()
    assert np.array_equal(got, want) and 0 < want.sum() < want.size


def test_env_step_episode_statistics_bit_exact(small_world):
    """ep_return / ep_final / ep_final_len of tde_env_step equal the oracle's (float64 sums: same order, same bits), with
    in-place re-spawn and without"""
    for flags in (_abi.F_ALL, _abi.F_ALL & ~_abi.F_AUTORESET):
        cfg = _abi.default_config(seed=14, distance_cutoff=0.25, flags=flags, max_steps=60)
        B, A = 160, 16
        hs, ds, dw = _pair(small_world, B, A, cfg)
        rng = np.random.default_rng(5)
        for t in range(150):
            act = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
            hs["action"][...] = act
            ds["action"].copy_(dev(act))
            oracle.env_step(cfg, small_world, hs)
            ops.env_step(cfg, dw, ds)
            if t % 10 == 9:
                for k in ("ep_return", "ep_final"):
                    assert np.array_equal(ds[k].cpu().numpy().view(np.uint64), hs[k].view(np.uint64)), (k, t)
                assert np.array_equal(ds["ep_final_len"].cpu().numpy(), hs["ep_final_len"]), t
            if not (flags & _abi.F_AUTORESET) and t % 40 == 39:
                m = (hs["terminated"] | hs["truncated"]).astype(np.uint8)
                oracle.env_reset(cfg, small_world, hs, m)
                ops.env_reset(cfg, dw, ds, dev(m))
        assert hs["ep_final_len"].max() > 0 and hs["ep_final"].any()


def _single_frames(env):
    """the current single frame of every env, rendered independently of the env's own stack"""
    return ops.render_ego(env.tde_cfg, env.dworld, env.state, 64, 64, env._fov, 1, flags=env._rflags).clone()


def test_device_frame_stack_restarts_blank_on_in_kernel_respawn(small_world):
    """auto_reset=True: an env that finishes is re-spawned inside the step kernel; its stacked observation of that very
    step must be (blank, blank, first frame of the new episode), and every other env keeps (t-1, t, t+1)"""
    cfg = EnvConfig(seed=21, distance_cutoff=0.25, max_environment_steps=25)
    B = 96
    env = BatchedWaypointEnv(cfg, small_world, num_envs=B, device=DEV, frame_stack=3)
    obs = env.reset()
    assert not obs[:, :6].any() and torch.equal(obs[:, 6:], _single_frames(env))
    hist = [torch.zeros_like(obs[:, :3]), torch.zeros_like(obs[:, :3]), obs[:, 6:].clone()]
    g = torch.Generator().manual_seed(3)
    n_done = 0
    for t in range(70):
        a = torch.stack([torch.rand(B, generator=g) * 2 - 1, torch.rand(B, generator=g) * 0.6 - 0.3], -1)
        obs, rew, term, trunc, info = env.step(a)
        done = (term | trunc)
        cur = _single_frames(env)
        hist = [hist[1], hist[2], cur]
        for j in range(2):
            hist[j] = torch.where(done[:, None, None, None], torch.zeros_like(cur), hist[j])
        want = torch.cat(hist, 1)
        assert torch.equal(obs, want), (t, int((obs != want).any(3).any(2).any(1).sum()))
        n_done += int(done.sum())
    assert n_done > B                                      # many episodes ended and restarted along the way
    sd = env.state_dict()
    o1, *_ = env.step(torch.zeros(B, 2))
    o1 = o1.clone()
    env.step(torch.ones(B, 2) * 0.1)
    env.load_state_dict(sd)
    o2, *_ = env.step(torch.zeros(B, 2))
    assert torch.equal(o1, o2)                             # the ring and its phase are part of the checkpoint


@pytest.mark.parametrize("copy_obs", [True, False])
def test_vecenv_frame_stack_terminal_observation_and_episode_stats(small_world, copy_obs):
    """the SB3 path at frame_stack=3 (the reference's VecFrameStack(n_stack=3)): envs that did not finish keep
    (t-1, t, t+1) - the masked reset must not touch their stack -, finished envs return (blank, blank, first frame) with
    the pre-reset stack in info['terminal_observation'], and Monitor's info['episode'] = {r, l, t}"""
    cfg = EnvConfig(seed=31, distance_cutoff=0.25, max_environment_steps=30)
    B = 64
    env = BatchedWaypointEnv(cfg, small_world, num_envs=B, device=DEV, frame_stack=3)
    venv = WaypointVecEnv(env, copy_obs=copy_obs)
    assert venv.num_envs == B and venv.observation_space.shape == (9, 64, 64) and venv.action_space.shape == (2,)
    obs = venv.reset()
    assert obs.shape == (B, 9, 64, 64) and obs.dtype == np.uint8 and not obs[:, :6].any()
    hist = [np.zeros_like(obs[:, :3]), np.zeros_like(obs[:, :3]), obs[:, 6:].copy()]
    rng = np.random.default_rng(1)
    ret, length, n_done = np.zeros(B), np.zeros(B, np.int64), 0
    for t in range(80):
        acts = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1)
        obs, rew, done, infos = venv.step(acts)
        assert obs.shape == (B, 9, 64, 64) and rew.shape == (B,) and rew.dtype == np.float32 and done.dtype == bool
        assert isinstance(infos, LazyInfos) and len(infos) == B
        ret += rew.astype(np.float64)
        length += 1
        cur = obs[:, 6:].copy()                            # newest frame: post-reset for the finished envs
        pre = [hist[1], hist[2]]
        for i in range(B):
            info = infos[i]
            if done[i]:
                n_done += 1
                tob = info["terminal_observation"]
                assert tob.shape == (9, 64, 64)
                assert np.array_equal(tob[:3], pre[0][i]) and np.array_equal(tob[3:6], pre[1][i])
                assert not obs[i, :6].any()                # the new episode's stack restarts blank
                ep = info["episode"]
                assert ep["l"] == length[i] and ep["r"] == round(ret[i], 6) and ep["t"] >= 0
                assert info["TimeLimit.truncated"] == (info["is_success"] and not
                                                        (info["offroad"] or info["collision"] or info["traffic_light_violation"]))
                ret[i], length[i] = 0.0, 0
            else:
                assert "terminal_observation" not in info and "episode" not in info
                assert np.array_equal(obs[i, :3], pre[0][i]) and np.array_equal(obs[i, 3:6], pre[1][i]), (t, i)
        hist = [np.where(done[:, None, None, None], 0, pre[0]), np.where(done[:, None, None, None], 0, pre[1]), cur]
        hist = [h.astype(np.uint8) for h in hist]
        assert (env.state["steps"].cpu().numpy()[done] == 0).all()
    assert n_done > B
    assert venv.env_is_wrapped(object) == [False] * B and venv.get_attr("num_envs", [0, 1]) == [B, B]
    assert len(venv.get_images()) == B and venv.seed(1) == [None] * B
    venv.close()


def test_vecenv_state_obs_matches_device_api(small_world):
    """numpy path == device path on the same seeds (obs_mode 'state'), infos columns included"""
    cfg = EnvConfig(seed=41, distance_cutoff=0.25, max_environment_steps=40)
    B = 128
    a = BatchedWaypointEnv(cfg, small_world, num_envs=B, device=DEV, obs_mode="state")
    b = BatchedWaypointEnv(cfg, small_world, num_envs=B, device=DEV, obs_mode="state")
    venv = b.as_vec_env()
    oa, ob = a.reset(), venv.reset()
    assert np.array_equal(oa.cpu().numpy(), ob)
    rng = np.random.default_rng(2)
    for t in range(90):
        acts = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
        oa, ra, ta, tra, ia = a.step(torch.from_numpy(acts))
        ob, rb, db, ib = venv.step(acts)
        assert np.array_equal(oa.cpu().numpy(), ob) and np.array_equal(ra.cpu().numpy(), rb)
        assert np.array_equal((ta | tra).cpu().numpy(), db)
        assert np.array_equal(ia["offroad"].cpu().numpy(), ib.column("offroad"))
        assert np.array_equal(ia["reached_waypoint_num"].cpu().numpy(), ib.column("reached_waypoint_num"))
        assert np.array_equal(ia["psi_reward"].cpu().numpy(), ib.column("psi_reward"))


def test_config_rejections_and_world_threshold_on_the_env(small_world):
    with pytest.raises(NotImplementedError):
        BatchedWaypointEnv(EnvConfig(render_mode="video"), small_world, num_envs=2, device=DEV)
    with pytest.raises(NotImplementedError):
        BatchedWaypointEnv(EnvConfig(simulator=SimulatorConfig(collision_metric="iou")), small_world, num_envs=2, device=DEV)
    with pytest.raises(ValueError):                        # the prebuilt World's grid index was built for 0.5 m
        BatchedWaypointEnv(EnvConfig(simulator=SimulatorConfig(offroad_threshold=0.8)), small_world, num_envs=2, device=DEV)
    with pytest.raises(ValueError):                        # outside the controller's sqrt domain (tde_env_* reject it too)
        BatchedWaypointEnv(EnvConfig(simulator=SimulatorConfig(npc_max_accel=1e-9)), small_world, num_envs=2, device=DEV)
    raw = _abi.default_config(seed=1)
    raw.npc_max_accel = 1e-9
    st = EnvState(2, small_world.A, device=DEV)
    with pytest.raises(RuntimeError, match="npc_max_accel"):
        ops.env_reset(raw, small_world.to_device(DEV), st)
    # left-handed (the reference's default) vs right-handed observation of the same state: mirror images
    lh = BatchedWaypointEnv(EnvConfig(seed=5), small_world, num_envs=8, device=DEV)
    rh = BatchedWaypointEnv(EnvConfig(seed=5, simulator=SimulatorConfig(
        renderer=RendererConfig(left_handed_coordinates=False), left_handed_coordinates=False)), small_world, num_envs=8,
        device=DEV)
    ol, orr = lh.reset(), rh.reset()
    assert torch.equal(ol, orr.flip(-1)) and not torch.equal(ol, orr)


def test_sharded_env_two_processes_equal_the_unsharded_batch(small_world):
    """ShardedBatchedEnv: two worker processes (sharing this box's GPU), env_base 0 and B/2, host-gathered observations /
    rewards / dones / state equal the unsharded HIP env bit for bit through re-spawns"""
    from torchdriveenv_amd.sharding import ShardedBatchedEnv

    cfg = EnvConfig(seed=51, distance_cutoff=0.25, max_environment_steps=35)
    B = 96
    one = BatchedWaypointEnv(cfg, small_world, num_envs=B, device=DEV, obs_mode="state").as_vec_env()
    two = ShardedBatchedEnv(cfg, small_world, B, n_shards=2, devices=[0, 0], obs_mode="state")
    try:
        assert two.ranges == [(0, B // 2), (B // 2, B)]
        oa, ob = one.reset(), two.reset()
        assert np.array_equal(oa, ob)
        rng = np.random.default_rng(3)
        n_done = 0
        for t in range(80):
            acts = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
            oa, ra, da, ia = one.step(acts)
            ob, rb, db, ib = two.step(acts)
            assert np.array_equal(oa, ob) and np.array_equal(ra.view(np.uint32), rb.view(np.uint32)) and np.array_equal(da, db)
            for i in np.nonzero(da)[0]:
                assert ia[i]["episode"]["r"] == ib[i]["episode"]["r"] and ia[i]["episode"]["l"] == ib[i]["episode"]["l"]
                assert np.array_equal(ia[i]["terminal_observation"], ib[i]["terminal_observation"])
            assert np.array_equal(ia.column("reached_waypoint_num"), ib.column("reached_waypoint_num"))
            n_done += int(da.sum())
        assert n_done > B // 2
        full = {k: v.cpu().numpy() for k, v in one.env.state.arrays.items() if v is not None}
        got = two.gather_state()
        for k in ("x", "y", "psi", "v", "scn", "episode", "steps", "ep_return"):
            assert np.array_equal(got[k].view(np.uint8), full[k].view(np.uint8)), k
    finally:
        two.close()


def test_extension_equals_ctypes_equals_oracle(small_world):
    """the PyTorch-ROCm C++ extension and the ctypes binding call the same C-ABI entry points: stepping the same batch
    through either gives the same bits as the oracle (state, rewards, flags, episode statistics, observations)"""
    cfg = EnvConfig(seed=61, distance_cutoff=0.25, max_environment_steps=40)
    B = 96
    e_ext = BatchedWaypointEnv(cfg, small_world, num_envs=B, device=DEV, obs_mode="state", binding="ext")
    e_ct = BatchedWaypointEnv(cfg, small_world, num_envs=B, device=DEV, obs_mode="state", binding="ctypes")
    from torchdriveenv_amd import _ext

    assert type(e_ext._h) is _ext.load().EnvHandle and type(e_ct._h) is ops.CtypesHandle
    assert e_ext.binding == "ext" and e_ct.binding == "ctypes"
    hs = EnvState(B, small_world.A)
    ocfg = e_ext.tde_cfg
    oracle.env_reset(ocfg, small_world, hs)
    o1, o2 = e_ext.reset(), e_ct.reset()
    assert torch.equal(o1, o2)
    rng = np.random.default_rng(6)
    for t in range(100):
        act = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
        a = dev(act)
        o1, r1, t1, tr1, i1 = e_ext.step(a)
        o2, r2, t2, tr2, i2 = e_ct.step(a)
        hs["action"][...] = act
        oracle.env_step(ocfg, small_world, hs)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(t1, t2) and torch.equal(tr1, tr2)
        assert np.array_equal(r1.cpu().numpy().view(np.uint32), hs["reward"].view(np.uint32))
    h = hs.host()
    for k in ("x", "y", "psi", "v", "episode", "steps", "ep_return", "ep_final", "collided", "offroad", "done_bits"):
        a1, a2 = e_ext.state[k].cpu().numpy(), e_ct.state[k].cpu().numpy()
        assert np.array_equal(a1.view(np.uint8), h[k].view(np.uint8)) and np.array_equal(a2.view(np.uint8), h[k].view(np.uint8)), k
    # rollout and birdview through the extension
    acts = torch.zeros(30, B, 2, device=DEV)
    acts[..., 0] = 0.4
    ra, da = e_ext.rollout(acts)
    rb, db = e_ct.rollout(acts)
    assert torch.equal(ra, rb) and torch.equal(da, db)
    with pytest.raises(RuntimeError):
        e_ext._h.step(torch.zeros(B, 2), int(e_ext.tde_cfg.flags))            # a CPU tensor is refused, not dereferenced
    with pytest.raises(RuntimeError):
        e_ext._h.step(torch.zeros(B, 3, device=DEV), int(e_ext.tde_cfg.flags))
    b1 = BatchedWaypointEnv(cfg, small_world, num_envs=16, device=DEV, frame_stack=3, binding="ext")
    b2 = BatchedWaypointEnv(cfg, small_world, num_envs=16, device=DEV, frame_stack=3, binding="ctypes")
    assert torch.equal(b1.reset(), b2.reset())
    for t in range(50):
        a = torch.rand(16, 2, device=DEV) * 0.6 - 0.3
        assert torch.equal(b1.step(a)[0], b2.step(a)[0])
        if t % 10 == 9:                                   # a caller's masked reset: tde_env_reset_render through both bindings
            m = torch.rand(16, device=DEV) < 0.3
            assert torch.equal(b1.reset(mask=m), b2.reset(mask=m))
            assert torch.equal(b1.state["x"], b2.state["x"]) and torch.equal(b1.state["episode"], b2.state["episode"])


@pytest.mark.parametrize("A", [8, 16, 32])
@pytest.mark.parametrize("flags", [_abi.F_ALL | _abi.F_TRAFFIC_LIGHTS, _abi.F_ALL & ~_abi.F_AUTORESET, _abi.F_NPC | _abi.F_OFFROAD])
def test_step_three_role_kernel_and_caches_bit_exact(A, flags):
    """tde_env_step with the lookup caches (three-role kernel) and without them (one-role kernel) against the oracle, over
    re-spawns, masked resets, rollouts in between (which leave the caches keyed for an older state) and state
    overwritten from the host (caches stale or empty): every array equal bit for bit at every checkpoint"""
    from torchdriveenv_amd.synth import synthetic_world

    world = synthetic_world(n_scn=8, A=A, seed=2, n_maps=2)
    cfg = _abi.default_config(seed=17, distance_cutoff=0.25, flags=flags, max_steps=45)
    B = 100                                               # not a multiple of the group size: partly filled last group
    hs = EnvState(B, A)
    # (100 envs: far below the size at which tde_env_step switches back to the one-role kernel)
    fast, slow = EnvState(B, A, device=DEV, with_obs=True), EnvState(B, A, device=DEV, with_obs=True, with_cache=False)
    assert fast["slot_cache"] is not None and slow["slot_cache"] is None
    dw = world.to_device(DEV)
    oracle.env_reset(cfg, world, hs)
    for ds in (fast, slow):
        ops.env_reset(cfg, dw, ds)
    rng = np.random.default_rng(8)

    def check(tag):
        h = hs.host()
        for ds in (fast, slow):
            d = ds.host()
            for k, v in h.items():
                if k == "info":       # float64 psi_reward: libm vs OCML cos may differ in the last bit (test_reward_cos_bits_...)
                    assert np.array_equal(v[:, [0, 1, 3]], d[k][:, [0, 1, 3]]) and np.abs(v[:, 2] - d[k][:, 2]).max() < 1e-14, (tag, ds is fast)
                elif k != "action":
                    assert np.array_equal(v.view(np.uint8), d[k].view(np.uint8)), (tag, k, ds is fast)
        assert torch.equal(fast["obs"], slow["obs"]) and torch.equal(fast["obs"], ops.state_obs(dw, fast)), tag

    for t in range(140):
        act = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
        hs["action"][...] = act
        oracle.env_step(cfg, world, hs)
        for ds in (fast, slow):
            ds["action"].copy_(dev(act))
            ops.env_step(cfg, dw, ds)
        if t % 7 == 6:
            check(t)
        if t % 40 == 39:                                  # masked reset of the finished (or a few random) envs
            m = ((hs["terminated"] | hs["truncated"]) | (rng.uniform(size=B) < 0.1)).astype(np.uint8)
            oracle.env_reset(cfg, world, hs, m)
            for ds in (fast, slow):
                ops.env_reset(cfg, dw, ds, dev(m))
        if t == 60:                                       # a rollout moves the state on without touching the caches
            acts = np.stack([rng.uniform(-1, 1, (9, B)), rng.uniform(-0.3, 0.3, (9, B))], -1).astype(np.float32)
            oracle.env_rollout(cfg, world, hs, acts)
            for ds in (fast, slow):
                ops.env_rollout(cfg, dw, ds, dev(acts))
        if t == 100:                                      # state overwritten from the host: cache entries keyed for the old one
            for ds in (fast, slow):
                ds.load(hs.host())
    check("end")
    assert hs["episode"].max() > 1 and bool((fast["slot_cache"][:, 1] & (1 << 30)).any())


@pytest.mark.parametrize("B,n_streams", [(256, 2), (200, 2), (320, 3), (96, 4), (256, 1)])
def test_step_render_on_streams_equals_whole_batch_and_oracle(small_world, B, n_streams):
    """tde_env_step_render (sub-batches on their own HIP streams: step, then the birdview) against tde_env_step + tde_render_ego
    on the whole batch and against the oracle, over re-spawns; through ctypes and through the extension; single frames and the
    layer-ring frame stack with `fresh` = the step's done bits"""
    import ctypes

    from torchdriveenv_amd import _ext

    A = small_world.A
    cfg = _abi.default_config(seed=33, distance_cutoff=0.25, max_steps=30)
    hs, whole, dw = _pair(small_world, B, A, cfg)
    split, viaext = EnvState(B, A, device=DEV), EnvState(B, A, device=DEV)
    split.load(hs.host()); viaext.load(hs.host())
    streams = [torch.cuda.Stream(device=DEV) for _ in range(n_streams)]
    h = _ext.env_handle(cfg, dw, viaext)
    img_w = torch.zeros((B, 3, 64, 64), dtype=torch.uint8, device=DEV)
    img_s, img_e = torch.zeros_like(img_w), torch.zeros_like(img_w)
    # frame stack of 3 through the layer ring (split path) vs the same on the whole batch
    ring_w = torch.full((B, 3, 64 * 64), 5, dtype=torch.uint8, device=DEV)
    ring_s = ring_w.clone()
    stk_w = torch.zeros((B, 9, 64, 64), dtype=torch.uint8, device=DEV)
    stk_s = torch.zeros_like(stk_w)
    rng = np.random.default_rng(12)
    n_done = 0
    for t in range(70):
        act = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
        a = dev(act)
        hs["action"][...] = act
        oracle.env_step(cfg, small_world, hs)
        ops.env_step(cfg, dw, whole, action=a)
        ops.render_ego(cfg, dw, whole, out=img_w)
        ops.render_ego(cfg, dw, whole, n_stack=3, out=stk_w, layers=ring_w, phase=t % 3, fresh=whole["done_bits"])
        ops.fork_streams(streams, DEV)
        ops.env_step_render(cfg, dw, split, streams, action=a, out=img_s)
        ops.join_streams(streams, DEV)
        # (the stacked call re-renders the state the step above produced: render-only would need a second step, so the stack
        #  goes through plain render_ego on the sub-batch streams' joined state)
        ops.render_ego(cfg, dw, split, n_stack=3, out=stk_s, layers=ring_s, phase=t % 3, fresh=split["done_bits"])
        ops.fork_streams(streams, DEV)
        h.step_render(a, int(cfg.flags), img_e, 64, 64, 35.0, 1, None, 0, 0, None, [s.cuda_stream for s in streams])
        ops.join_streams(streams, DEV)
        assert torch.equal(img_w, img_s) and torch.equal(img_w, img_e) and torch.equal(stk_w, stk_s), t
        n_done += int((hs["terminated"] | hs["truncated"]).sum())
        if t % 10 == 9:
            want = oracle.render_ego(cfg, small_world, hs)
            assert np.array_equal(img_s.cpu().numpy(), want), t
    assert n_done > B // 2
    host = hs.host()
    for ds in (whole, split, viaext):
        d = ds.host()
        for k, v in host.items():
            if k not in ("action", "info"):
                assert np.array_equal(v.view(np.uint8), d[k].view(np.uint8)), k
    # the step alone (render = NULL) and the stacked render inside the call
    ops.fork_streams(streams, DEV)
    ops.env_step_render(cfg, dw, split, streams, action=a, render=False)
    ops.join_streams(streams, DEV)
    ops.env_step(cfg, dw, whole, action=a)
    assert torch.equal(split["x"], whole["x"]) and torch.equal(split["reward"], whole["reward"])
    ops.fork_streams(streams, DEV)
    ops.env_step_render(cfg, dw, split, streams, action=a, out=stk_s, n_stack=3, layers=ring_s, phase=1, fresh=split["done_bits"])
    ops.join_streams(streams, DEV)
    ops.env_step(cfg, dw, whole, action=a)
    ops.render_ego(cfg, dw, whole, n_stack=3, out=stk_w, layers=ring_w, phase=1, fresh=whole["done_bits"])
    assert torch.equal(stk_w, stk_s) and torch.equal(ring_w, ring_s)
    with pytest.raises(Exception):
        ops.env_step_render(cfg, dw, split, [], action=a)


@pytest.mark.parametrize("A", [16, 32])
def test_step_forms_alternating_on_one_state_and_flag_changes_bit_exact(A):
    """a state stepped by the one-role kernel alone (it ignores the lookup caches), and one stepped by the one- and three-role
    forms in alternation (tde_kernel_override: the three-role kernel finds entries keyed for a state the other form has moved
    on), over re-spawns, masked resets, a rollout in between, a host-side overwrite and a change of the NPC / REPLAY flags
    between launches (part of the slot entries' key), equal the oracle bit for bit at every checkpoint"""
    from torchdriveenv_amd import _lib
    from torchdriveenv_amd.synth import synthetic_world

    world = synthetic_world(n_scn=8, A=A, seed=3, n_maps=2)
    F = _abi.F_ALL | _abi.F_TRAFFIC_LIGHTS
    cfg = _abi.default_config(seed=29, distance_cutoff=0.25, flags=F, max_steps=40)
    cfg_b = _abi.default_config(seed=29, distance_cutoff=0.25, flags=F & ~_abi.F_NPC, max_steps=40)
    # what the stored NPC actions depend on besides the state (ABI 9: hashed into the action cache's key): the lights flag, a
    # controller constant
    cfg_c = _abi.default_config(seed=29, distance_cutoff=0.25, flags=F & ~_abi.F_TRAFFIC_LIGHTS, max_steps=40)
    cfg_d = _abi.default_config(seed=29, distance_cutoff=0.25, flags=F, max_steps=40, npc_k_speed=1.5, npc_gap_s0=4.0)
    B = 100
    hs = EnvState(B, A)
    solo, mixed = EnvState(B, A, device=DEV, with_obs=True), EnvState(B, A, device=DEV, with_obs=True)
    dw = world.to_device(DEV)
    oracle.env_reset(cfg, world, hs)
    for ds in (solo, mixed):
        ops.env_reset(cfg, dw, ds)
    rng = np.random.default_rng(5)

    def check(tag):
        h = hs.host()
        for ds in (solo, mixed):
            d = ds.host()
            for k, v in h.items():
                if k == "info":
                    assert np.array_equal(v[:, [0, 1, 3]], d[k][:, [0, 1, 3]]) and np.abs(v[:, 2] - d[k][:, 2]).max() < 1e-14, (tag, ds is solo)
                elif k != "action":
                    assert np.array_equal(v.view(np.uint8), d[k].view(np.uint8)), (tag, k, ds is solo)
        assert torch.equal(solo["obs"], mixed["obs"]) and torch.equal(solo["obs"], ops.state_obs(dw, solo)), tag

    try:
        for t in range(150):
            # ten steps without the NPC controller, six without the lights, six with other controller constants
            c = cfg_b if 70 <= t < 80 else cfg_c if 90 <= t < 96 else cfg_d if 108 <= t < 114 else cfg
            act = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
            hs["action"][...] = act
            oracle.env_step(c, world, hs)
            _lib.kernel_override(step="solo")
            solo["action"].copy_(dev(act))
            ops.env_step(c, dw, solo)
            _lib.kernel_override(step="solo" if (t // 3) % 2 else "trio")
            mixed["action"].copy_(dev(act))
            ops.env_step(c, dw, mixed)
            if t % 7 == 6 or t in (70, 71, 80, 81, 90, 91, 96, 97, 108, 109, 114, 115):
                check(t)
            if t % 40 == 39:
                m = ((hs["terminated"] | hs["truncated"]) | (rng.uniform(size=B) < 0.1)).astype(np.uint8)
                oracle.env_reset(cfg, world, hs, m)
                for ds in (solo, mixed):
                    ops.env_reset(cfg, dw, ds, dev(m))
            if t == 55:
                acts = np.stack([rng.uniform(-1, 1, (9, B)), rng.uniform(-0.3, 0.3, (9, B))], -1).astype(np.float32)
                oracle.env_rollout(cfg, world, hs, acts)
                for ds in (solo, mixed):
                    ops.env_rollout(cfg, dw, ds, dev(acts))
            if t == 100:
                for ds in (solo, mixed):
                    ds.load(hs.host())
        check("end")
    finally:
        _lib.kernel_override()
    assert hs["episode"].max() > 1 and bool((mixed["slot_cache"][:, 1] & (1 << 30)).any())


def test_step_render_on_streams_at_configs4_size_and_odd_shapes():
    """tde_env_step_render at BASELINE configs[4]'s full size (8192 envs x 32 agents, three streams, as bench.py runs it) against
    tde_env_step + tde_render_ego on the whole batch: state, outputs and every pixel equal after 12 steps with re-spawns; and
    at shapes that do not divide (1, 63, 65 envs; more streams than 64-env groups)"""
    from torchdriveenv_amd.synth import synthetic_world

    def run(world, B, n_streams, steps, seed):
        A = world.A
        cfg = _abi.default_config(seed=seed, distance_cutoff=0.25, max_steps=8)
        dw = world.to_device(DEV)
        whole, split = EnvState(B, A, device=DEV), EnvState(B, A, device=DEV)
        ops.env_reset(cfg, dw, whole)
        ops.env_reset(cfg, dw, split)
        streams = [torch.cuda.Stream(device=DEV) for _ in range(n_streams)]
        img_w = torch.zeros((B, 3, 64, 64), dtype=torch.uint8, device=DEV)
        img_s = torch.zeros_like(img_w)
        g = torch.Generator().manual_seed(seed)
        ops.fork_streams(streams, DEV)
        for t in range(steps):
            a = torch.stack([torch.rand(B, generator=g) * 2 - 1, torch.rand(B, generator=g) * 0.6 - 0.3], -1).to(DEV)
            ops.env_step(cfg, dw, whole, action=a)
            ops.render_ego(cfg, dw, whole, out=img_w)
            ops.env_step_render(cfg, dw, split, streams, action=a, out=img_s)      # (consecutive calls: ordered per sub-batch)
        ops.join_streams(streams, DEV)
        torch.cuda.synchronize()
        assert torch.equal(img_w, img_s)
        for k in ("x", "y", "psi", "v", "route_wp", "collided", "offroad", "scn", "steps", "episode", "reward", "terminated",
                  "truncated", "target_idx", "reached", "done_bits"):
            assert torch.equal(whole[k], split[k]), (B, n_streams, k)
        assert int(whole["episode"].max()) >= 1

    run(synthetic_world(n_scn=64, A=32, seed=0, n_maps=4), 8192, 3, 12, 5)
    small = synthetic_world(n_scn=8, A=8, seed=1, n_maps=2)
    for B, n in ((1, 2), (63, 3), (65, 2), (130, 16)):
        run(small, B, n, 12, 7 + B)


def test_world_beyond_the_packed_cache_entry_takes_the_one_role_kernel(small_world):
    """a world whose route / replay ids or lengths do not fit tde_slot_cache's packed words (>= 2^20 - 1 ids, >= 4096 entries) is
    stepped by the one-role kernel although the caches are present: results equal the oracle's, no cache entry is ever written"""
    import copy

    cfg = _abi.default_config(seed=8, distance_cutoff=0.25, max_steps=20)
    B, A = 64, small_world.A
    hs, ds, dw = _pair(small_world, B, A, cfg)
    big = copy.copy(dw)
    big.struct = type(dw.struct).from_buffer_copy(dw.struct)
    big.struct.n_routes = 1 << 20                          # (a count only: nothing indexes with it)
    rng = np.random.default_rng(2)
    for t in range(30):
        act = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
        hs["action"][...] = act
        ds["action"].copy_(dev(act))
        oracle.env_step(cfg, small_world, hs)
        ops.env_step(cfg, big, ds)
    h, d = hs.host(), ds.host()
    for k in ("x", "y", "psi", "v", "steps", "episode", "reward", "collided", "offroad", "terminated", "truncated"):
        assert np.array_equal(h[k].view(np.uint8), d[k].view(np.uint8)), k
    assert not bool((ds["slot_cache"][:, 1] & (1 << 30)).any())
    ops.env_step(cfg, dw, ds)                              # the same state under the real counts: three roles, entries appear
    assert bool((ds["slot_cache"][:, 1] & (1 << 30)).any())


@pytest.mark.parametrize("copy_obs", [True, False])
def test_vecenv_one_synchronisation_path_equals_the_two_synchronisation_path(small_world, copy_obs):
    """WaypointVecEnv with the compact observation: through the extension a step is ONE stream synchronisation (the finished envs
    re-spawned by tde_env_post_step behind the output copy, every observation row copied twice); through the ctypes binding it is
    the round-4 sequence (masked reset, gather of the finished rows, a second synchronisation).  Same observations, rewards,
    dones, info columns, terminal observations and episode statistics, step by step - with fresh arrays and with ring views"""
    from torchdriveenv_amd.config import EnvConfig
    from torchdriveenv_amd.env import BatchedWaypointEnv, WaypointVecEnv

    B = 128
    cfg = EnvConfig(seed=21, distance_cutoff=0.25, max_environment_steps=30)
    kw = dict(num_envs=B, agents_per_env=16, obs_mode="state")
    one = WaypointVecEnv(BatchedWaypointEnv(cfg, small_world, binding="ext", **kw), copy_obs=copy_obs)
    two = WaypointVecEnv(BatchedWaypointEnv(cfg, small_world, binding="ctypes", **kw), copy_obs=copy_obs)
    assert np.array_equal(one.reset(), two.reset())
    rng = np.random.default_rng(5)
    n_done = 0
    keep = []                                                   # (ring views must survive the next two steps)
    for t in range(80):
        acts = np.stack([rng.uniform(-0.5, 1, B), rng.uniform(-0.3, 0.3, B)], -1)
        o1, r1, d1, i1 = one.step(acts)
        o2, r2, d2, i2 = two.step(acts)
        assert np.array_equal(o1, o2) and np.array_equal(r1, r2) and np.array_equal(d1, d2), t
        for k in i1.columns:
            assert np.array_equal(i1.column(k), i2.column(k)), (t, k)
        for i in np.nonzero(d1)[0]:
            a, b = i1[int(i)], i2[int(i)]
            assert np.array_equal(a["terminal_observation"], b["terminal_observation"]), (t, i)
            assert a["episode"]["r"] == b["episode"]["r"] and a["episode"]["l"] == b["episode"]["l"]
            assert a["TimeLimit.truncated"] == b["TimeLimit.truncated"]
            n_done += 1
        if not copy_obs:
            keep.append((o1, o1.copy(), r1, r1.copy()))
            if len(keep) > 2:
                v, c, rv, rc = keep.pop(0)
                assert np.array_equal(v, c) and np.array_equal(rv, rc), t        # still intact two steps later
    for k in ("x", "y", "psi", "episode", "scn", "steps"):
        assert torch.equal(one.env.state[k], two.env.state[k]), k
    assert n_done > 40
