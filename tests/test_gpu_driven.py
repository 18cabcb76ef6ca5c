"""tde_env_step_driven on the GPU (include/tde_driven.h): chosen NPC slots take their actions from outside.  Nothing here has a
tolerance.  With nothing driven the call must equal tde_env_step's one-role kernel on every array; with every NPC echoing the
controller's own action it must equal the oracle's step; with seeded random actions the motion must equal tests/driven_ref.py and
everything behind the motion the oracle's own operators on those poses (compute_collision, compute_offroad, waypoint_reward, env_reset of
the finished envs): ref_step below composes them into the whole expected state."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import oracle
from tests import config_zoo, driven_ref
from torchdriveenv_amd import _abi, _lib, ops
from torchdriveenv_amd.config import EnvConfig, RendererConfig, SimulatorConfig, VectorObs
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.state import EnvState
from torchdriveenv_amd.world import effective_offroad_distance

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CACHES = ("slot_cache", "env_cache", "act_cache")
AGENT = ("x", "y", "psi", "v", "route_wp", "len", "wid", "lr", "vdes", "present", "collided", "offroad")
ENV = ("scn", "steps", "target_idx", "reached", "episode", "reward", "terminated", "truncated", "done_bits")
NOLIGHTS = config_zoo.FLAGS & ~_abi.F_TRAFFIC_LIGHTS
_DW = {}


def _dworld(world):
    if id(world) not in _DW:
        _DW[id(world)] = (world, world.to_device(DEV))
    return _DW[id(world)][1]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def assert_same(got, want, keys, what=""):
    for k in keys:
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k, np.flatnonzero(np.asarray(got[k]).ravel() != np.asarray(want[k]).ravel())[:8])


def reset_pair(cfg, world, B, edit=None, **kw):
    """(host dict, device state) of one reset; `edit(h)` changes the host dict before it is loaded into the device state"""
    hs = EnvState(B, world.A)
    oracle.env_reset(cfg, world, hs)
    h = hs.host()
    if edit is not None:
        edit(h)
    ds = EnvState(B, world.A, device=DEV, **kw)
    ops.env_reset(cfg, _dworld(world), ds)
    ds.load(h)
    return h, ds


def ref_step(cfg, world, pre, agent_action=None, driven=None, tl=None):
    """the whole state a driven step leaves, from the host dict `pre` (its "action" is the egos'): driven_ref's motion, then the oracle's
    operators on those poses, then - with TDE_F_AUTORESET - the oracle's reset of the envs that finished.  tl: the ego's red-light
    violations [B] (None: none; the tests that pass it run without lights)."""
    B, A, F = len(pre["scn"]), world.A, int(cfg.flags)
    m = driven_ref.step_motion(cfg, world, pre, agent_action, driven)
    exp = {k: np.array(pre[k], copy=True) for k in AGENT + ENV if k in pre}
    for k in ("x", "y", "psi", "v", "route_wp"):
        exp[k] = m[k]
    pose = [m["x"], m["y"], m["psi"], pre["len"], pre["wid"], pre["present"]]
    exp["collided"] = oracle.compute_collision(B, A, *pose)
    moe = world.arrays["scn"]["map"][pre["scn"]].astype(np.int32)
    thr = effective_offroad_distance(cfg.offroad_threshold, bool(cfg.offroad_threshold_squared))
    exp["offroad"] = oracle.compute_offroad(B, A, *pose, world, moe, threshold=thr) if F & _abi.F_OFFROAD else np.zeros(B * A, np.uint8)
    ego = np.arange(B) * A
    four = lambda d: np.stack([np.asarray(d[k], np.float32)[ego] for k in ("x", "y", "psi", "v")], -1)      # noqa: E731
    steps, target, reached = (np.array(pre[k], np.int32, copy=True) for k in ("steps", "target_idx", "reached"))
    tl = np.zeros(B, np.uint8) if tl is None else np.asarray(tl, np.uint8)
    out = oracle.waypoint_reward(cfg, four(pre), four(m), exp["offroad"][ego], exp["collided"][ego], tl,
                                 world.arrays["wp_xy"].reshape(-1, world.ints["NW"], 2), world.arrays["scn"]["wp_n"], pre["scn"], steps, target, reached)
    exp.update(steps=steps, target_idx=target, reached=reached, reward=out["reward"], terminated=out["terminated"], truncated=out["truncated"])
    exp["done_bits"] = (out["terminated"] | (out["truncated"] << 1) | (exp["offroad"][ego] << 2) | (exp["collided"][ego] << 3) | (tl << 4)).astype(np.uint8)
    done = (out["terminated"] | out["truncated"]) != 0
    if (F & _abi.F_AUTORESET) and done.any():
        hs = EnvState(B, A)
        hs.load({k: exp[k] for k in AGENT + ("scn", "steps", "target_idx", "reached", "episode")})
        oracle.env_reset(cfg, world, hs, mask=done.astype(np.uint8))
        for k in AGENT + ("scn", "steps", "target_idx", "reached", "episode"):
            exp[k] = np.array(hs[k], copy=True)
        for k in ("collided", "offroad"):                      # (the flags of a re-spawned agent are cleared)
            exp[k].reshape(B, A)[done] = 0
    exp["_done"], exp["_driven"], exp["_pre_respawn"] = done, m["driven"], m
    return exp


def random_drive(rng, h, A, p=0.4):
    """a seeded subset of the slots and seeded actions within |acc| <= 3, |steer| <= 0.3; the rows of undriven slots (and row 0) are NaN"""
    B = len(h["scn"])
    drv = (rng.uniform(size=(B, A)) < p).astype(np.uint8)
    drv[:, 0] = 1                                              # (row 0 is never read: a set byte there must change nothing)
    aa = np.stack([rng.uniform(-3, 3, (B, A)), rng.uniform(-0.3, 0.3, (B, A))], -1).astype(np.float32)
    aa[drv == 0] = np.nan
    aa[:, 0] = np.nan
    return aa, drv


# ---- 1. nothing driven ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", [False, True], ids=["plain", "obs_mag"])
@pytest.mark.parametrize("lights", [False, True], ids=["nolights", "lights"])
@pytest.mark.parametrize("A,B", [(4, 33), (16, 5), (16, 17), (64, 5), (128, 3)])
def test_nothing_driven_equals_the_one_role_step_on_every_array(A, B, lights, outputs):
    """driven=None and an all-zero mask over NaN actions against tde_env_step forced to its one-role kernel: 3 steps of 2-step episodes, so
    every env is re-spawned inside the run; every array of the state, the caches included (the fresh act-cache key is the invalid one)"""
    world = config_zoo.world(None, A)
    dw = _dworld(world)
    cfg = config_zoo.config(None, A, flags=config_zoo.FLAGS if lights else NOLIGHTS, max_steps=2)
    kw = dict(with_obs=outputs, with_magnitudes=outputs)
    states = [reset_pair(cfg, world, B, **kw)[1] for _ in range(3)]
    acts = config_zoo.actions(None, B, A, T=3)
    nan = torch.full((B, A, 2), float("nan"), device=DEV)
    zero = torch.zeros((B, A), dtype=torch.uint8, device=DEV)
    ended = 0
    try:
        _lib.kernel_override(step="solo")
        for t in range(3):
            for ds in states:
                ds["action"].copy_(dev(acts[t]))
            ops.env_step(cfg, dw, states[0])
            ops.env_step_driven(cfg, dw, states[1])
            ops.env_step_driven(cfg, dw, states[2], nan, zero)
            torch.cuda.synchronize()
            want = states[0].host()
            ended += int((want["done_bits"] & 3 != 0).sum())
            for ds in states[1:]:
                assert_same(ds.host(), want, list(want), t)
    finally:
        _lib.kernel_override()
    assert ended >= B and (not outputs or ("obs" in want and "magnitudes" in want))


# ---- 2. echo ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zoo", [None, "fast_narrow"], ids=["default", "fast_narrow"])
@pytest.mark.parametrize("A,B", [(4, 33), (16, 17), (64, 5), (128, 3)])
def test_every_npc_echoing_the_controller_equals_the_oracle_step(A, B, zoo):
    """every present NPC slot without a live replay record (a driven slot leaves its record, the oracle's does not) is driven with the
    controller's own action of that step: the oracle's step, re-spawns included, bit for bit over 3 steps"""
    world = config_zoo.world(zoo, A)
    dw = _dworld(world)
    cfg = config_zoo.config(zoo, A, max_steps=2)
    hs = EnvState(B, A)
    oracle.env_reset(cfg, world, hs)
    ds = EnvState(B, A, device=DEV)
    ops.env_reset(cfg, dw, ds)
    acts = config_zoo.actions(zoo, B, A, T=3)
    n_driven = 0
    for t in range(3):
        hs["action"][...] = acts[t]
        pre = hs.host()
        s = driven_ref._scene(cfg, world, pre)
        mask = (s["other"] & ~((s["replay"] >= 0) & (s["k"] < s["replay_len"]))).reshape(B, A)
        echo = driven_ref.npc_actions(cfg, world, pre)
        echo[~mask] = np.nan
        n_driven += int(mask.sum())
        ds["action"].copy_(dev(acts[t]))
        ops.env_step_driven(cfg, dw, ds, dev(echo), dev(mask.astype(np.uint8)))
        oracle.env_step(cfg, world, hs)
        want, got = hs.host(), ds.host()
        assert_same(got, want, [k for k in want if k != "action"], t)
    assert n_driven > B and int(want["episode"].min()) >= 2


# ---- 3. perturbed -----------------------------------------------------------------------------------------------------------------------
def _stage(A):
    """the reset state with, in env 0, slot 1 standing half a car behind the ego at its heading (it hits the ego whatever it is told) and,
    in env 1, slot 2 thirty metres to the side of where it stood (off the road)"""
    def edit(h):
        x, y, psi = (h[k].reshape(-1, A) for k in ("x", "y", "psi"))
        x[0, 1], y[0, 1], psi[0, 1] = x[0, 0] - np.float32(2.5) * np.cos(psi[0, 0]), y[0, 0] - np.float32(2.5) * np.sin(psi[0, 0]), psi[0, 0]
        x[1, 2], y[1, 2] = x[1, 2] - np.float32(30.0) * np.sin(psi[1, 2]), y[1, 2] + np.float32(30.0) * np.cos(psi[1, 2])
    return edit


@pytest.mark.parametrize("A,B", [(4, 33), (16, 17), (64, 5), (128, 3)])
def test_perturbed_slots_move_as_driven_ref_and_are_judged_as_the_oracle_judges(A, B):
    world = config_zoo.world(None, A)
    dw = _dworld(world)
    cfg = config_zoo.config(None, A, flags=NOLIGHTS & ~_abi.F_AUTORESET)
    h, ds = reset_pair(cfg, world, B, edit=_stage(A))
    rng = np.random.default_rng(100 + A)
    acts = config_zoo.actions(None, B, A, T=2)
    hit_ego = left_road = False
    for t in range(2):
        pre = ds.host()
        pre["action"] = acts[t]
        aa, drv = random_drive(rng, pre, A)
        drv[0, 1] = drv[1, 2] = 1
        aa[0, 1], aa[1, 2] = (3.0, 0.0), (1.0, 0.3)
        exp = ref_step(cfg, world, pre, aa, drv)
        ds["action"].copy_(dev(acts[t]))
        ops.env_step_driven(cfg, dw, ds, dev(aa), dev(drv))
        got = ds.host()
        assert_same(got, exp, AGENT + ENV, t)
        col, off = got["collided"].reshape(B, A), got["offroad"].reshape(B, A)
        hit_ego |= bool(col[0, 1] and col[0, 0] and got["done_bits"][0] & 8 and exp["_driven"].reshape(B, A)[0, 1])
        left_road |= bool(off[1, 2] and exp["_driven"].reshape(B, A)[1, 2])
        assert exp["_driven"].sum() > 2 and not exp["_driven"].reshape(B, A)[:, 0].any()
    assert hit_ego and left_road


# ---- 4. replay --------------------------------------------------------------------------------------------------------------------------
def test_a_driven_replayed_slot_follows_its_action_and_the_undriven_one_its_record():
    A, B = 16, 6
    world = config_zoo.world(None, A)
    cfg = config_zoo.config(None, A, flags=NOLIGHTS & ~_abi.F_AUTORESET)
    h, ds = reset_pair(cfg, world, B)
    rec = world.arrays["spawn"].reshape(-1, A)[h["scn"]]
    e, a = np.nonzero((rec["replay"] >= 0) & (rec["replay_len"] > 3) & (h["present"].reshape(B, A) != 0))
    assert len(e) >= 2 and (a > 0).all()
    drv = np.zeros((B, A), np.uint8)
    drv[e[::2], a[::2]] = 1                                    # every other replayed slot is driven, the ones between follow their record
    aa = np.full((B, A, 2), np.nan, np.float32)
    aa[drv != 0] = (2.0, 0.1)
    states = world.arrays["replay_states"].reshape(-1, world.ints["RT"], 4)
    for t in range(2):
        pre = ds.host()
        exp = ref_step(cfg, world, pre, aa, drv)
        ops.env_step_driven(cfg, _dworld(world), ds, dev(aa), dev(drv))
        got = ds.host()
        assert_same(got, exp, AGENT + ENV, t)
        pose = np.stack([got[k].reshape(B, A) for k in ("x", "y", "psi", "v")], -1)
        for i, (ee, sa) in enumerate(zip(e, a)):
            on_record = np.array_equal(pose[ee, sa], states[rec["replay"][ee, sa], t + 1])
            assert on_record == (i % 2 == 1), (t, ee, sa)


# ---- 5. flags ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [NOLIGHTS & ~_abi.F_NPC_FIRST_STEP, NOLIGHTS & ~_abi.F_NPC, config_zoo.FLAGS & ~_abi.F_NPC_FIRST_STEP & ~_abi.F_REPLAY],
                         ids=["no_first_step", "no_npc", "lights_no_replay"])
def test_a_driven_slot_acts_at_the_first_step_and_without_the_controller(flags):
    A, B = 16, 9
    world = config_zoo.world(None, A)
    cfg = config_zoo.config(None, A, flags=flags & ~_abi.F_AUTORESET)
    h, ds = reset_pair(cfg, world, B)
    rng = np.random.default_rng(5)
    for t in range(2):
        pre = ds.host()
        aa, drv = random_drive(rng, pre, A)
        exp = ref_step(cfg, world, pre, aa, drv, tl=None)
        ops.env_step_driven(cfg, _dworld(world), ds, dev(aa), dev(drv))
        got = ds.host()
        keys = [k for k in AGENT + ENV if not (flags & _abi.F_TRAFFIC_LIGHTS and k in ("reward", "terminated", "truncated", "done_bits"))]
        assert_same(got, exp, keys, t)                         # (with lights the ego's red-line term is not restated here: motion and flags only)
        if t == 0:                                             # k == 1: the undriven NPCs coast (or have no controller), the driven ones act
            v0, v1 = pre["v"].reshape(B, A), got["v"].reshape(B, A)
            d = exp["_driven"].reshape(B, A)
            assert (v1[d] != v0[d]).any() and (int(pre["steps"].max()) == 0)


# ---- 6. absent slots --------------------------------------------------------------------------------------------------------------------
def test_absent_slots_marked_driven_stay_absent_and_untouched():
    A, B = 16, 7

    def edit(h):
        h["present"].reshape(B, A)[:, 3::4] = 0

    world = config_zoo.world(None, A)
    cfg = config_zoo.config(None, A, flags=NOLIGHTS & ~_abi.F_AUTORESET)
    h, ds = reset_pair(cfg, world, B, edit=edit)
    drv = np.ones((B, A), np.uint8)
    aa = np.full((B, A, 2), 1.0, np.float32)
    aa.reshape(B, A, 2)[:, 3::4] = np.nan                      # (absent rows are never read)
    pre = ds.host()
    exp = ref_step(cfg, world, pre, aa, drv)
    ops.env_step_driven(cfg, _dworld(world), ds, dev(aa), dev(drv))
    got = ds.host()
    assert_same(got, exp, AGENT + ENV)
    gone = np.zeros((B, A), bool)
    gone[:, 3::4] = True
    for k in AGENT:
        assert np.array_equal(bits(got[k].reshape(B, A)[gone]), bits(pre[k].reshape(B, A)[gone])), k
    assert not np.isnan(got["x"]).any() and not np.isnan(got["reward"]).any()


# ---- 7. interleaving with the default step ----------------------------------------------------------------------------------------------
def make_env(world, B, obs_mode="state", frame_stack=1, max_steps=3, **kw):
    cfg = EnvConfig(seed=11, distance_cutoff=0.25, max_environment_steps=max_steps, frame_stack=frame_stack,
                    simulator=SimulatorConfig(renderer=RendererConfig(res=64)))
    return BatchedWaypointEnv(cfg, world, num_envs=B, device=DEV, obs_mode=obs_mode, frame_stack=frame_stack, **kw)


def test_driven_and_plain_steps_interleave_on_an_env_with_the_trio_kernel_and_all_caches():
    """driven, plain, driven, plain over 3-step episodes: the plain steps (three-role kernel, lookup and action caches) must equal the oracle
    from the state before them, the driven ones ref_step; after each driven step the act cache's key of every env reads invalid"""
    A, B = 16, 12
    world = config_zoo.world(None, A)
    env = make_env(world, B)
    st = env.state
    assert all(st[k] is not None for k in CACHES)
    env.reset()
    rng = np.random.default_rng(3)
    acts = config_zoo.actions(None, B, A, T=4)
    respawns = 0
    for t in range(4):
        pre = st.host()
        pre["action"] = acts[t]
        a = dev(acts[t])
        if t % 2 == 0:
            aa, drv = random_drive(rng, pre, A)
            env.step(a, dev(aa), dev(drv))
            got = st.host()
            exp = ref_step(env.tde_cfg, world, pre, aa, drv, tl=got["tl_violation"])
            assert_same(got, exp, AGENT + ENV, t)
            keys = got["act_cache"].reshape(B, A + 1, 2)[:, A].view(np.int32)
            assert (keys[:, 0] < 0).all()
            respawns += int(exp["_done"].sum())
        else:
            env.step(a)
            hs = EnvState(B, A)
            hs.load(pre)
            oracle.env_step(env.tde_cfg, world, hs)
            got, want = st.host(), hs.host()
            assert_same(got, want, [k for k in want if k not in CACHES + ("action", "obs", "magnitudes")], t)
            respawns += int((want["done_bits"] & 3 != 0).sum())
    assert respawns >= B


# ---- 8. the env -------------------------------------------------------------------------------------------------------------------------
MODES = [("vector", 1, dict(vector_obs=VectorObs(k_neighbours=2, n_rays=4))), ("state", 1, {}), ("birdview", 3, {})]


@pytest.mark.parametrize("binding", ["ext", "ctypes"])
@pytest.mark.parametrize("obs_mode,frame_stack,kw", MODES, ids=[m[0] for m in MODES])
def test_env_step_with_driven_slots_equals_the_c_abi_call_and_observes_the_new_state(obs_mode, frame_stack, kw, binding):
    A, B = 16, 6
    world = config_zoo.world(None, A)
    env = make_env(world, B, obs_mode, frame_stack, binding=binding, **kw)
    term = make_env(world, B, obs_mode, frame_stack, binding=binding, terminal_obs=True, **kw)
    env.reset(), term.reset()
    rng = np.random.default_rng(8)
    acts = config_zoo.actions(None, B, A, T=4)
    ended = 0
    for t in range(4):
        pre = env.state.host()
        aa, drv = random_drive(rng, pre, A)
        twin = EnvState(B, A, device=DEV, with_obs=env.state["obs"] is not None, with_magnitudes=True)
        twin.load(pre)
        twin["action"].copy_(dev(acts[t]))
        ops.env_step_driven(env.tde_cfg, env.dworld, twin, dev(aa), dev(drv.astype(bool)))
        out = env.step(dev(acts[t]), dev(aa), dev(drv.astype(bool)))
        out_t = term.step(dev(acts[t]), dev(aa), dev(drv))
        got, want = env.state.host(), twin.host()
        assert_same(got, want, [k for k in want if k not in CACHES], t)
        assert np.array_equal(bits(out[1].cpu().numpy()), bits(want["reward"]))
        assert np.array_equal(out[2].cpu().numpy(), want["terminated"] != 0) and np.array_equal(out[3].cpu().numpy(), want["truncated"] != 0)
        for x, y in zip(out[:4], out_t[:4]):                  # terminal_obs=True: the same results
            assert torch.equal(x, y), t
        assert_same(term.state.host(), got, AGENT + ENV, t)
        obs = out[0].clone()
        if frame_stack > 1:                                    # (get_obs would push a frame: the newest one against a fresh single render)
            fresh = ops.render_ego(env.tde_cfg, env.dworld, env.state, 64, 64, env._fov, 1, flags=env._rflags)
            assert torch.equal(obs[:, -3:], fresh)
        else:
            assert torch.equal(obs, env.get_obs())
        ended += int((want["done_bits"] & 3 != 0).sum())
    assert ended > 0


def test_env_refusals_by_message():
    A, B = 16, 4
    world = config_zoo.world(None, A)
    env = make_env(world, B)
    env.reset()
    a = torch.zeros(B, 2, device=DEV)
    aa, drv = torch.zeros(B, A, 2, device=DEV), torch.ones(B, A, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError, match="^agent_action is required when driven is given$"):
        env.step(a, None, drv)
    with pytest.raises(ValueError, match=r"^driven must have shape \[4, 16\], got \[16, 4\]$"):
        env.step(a, aa, drv.reshape(A, B))
    with pytest.raises(ValueError, match=r"^agent_action must have shape \[4, 16, 2\], got \[4, 32\]$"):
        ops.env_step_driven(env.tde_cfg, env.dworld, env.state, aa.reshape(B, 2 * A), drv)
    with pytest.raises(ValueError, match="^agent_action must have 128 elements, got 64$"):
        env.step(a, aa[:, :8].contiguous(), drv)
    with pytest.raises(ValueError, match="^driven must be contiguous$"):
        env.step(a, aa, torch.ones(A, B, dtype=torch.uint8, device=DEV).t())
    with pytest.raises(ValueError, match="^agent_action is on cpu|^agent_action must live on a HIP device"):
        env.step(a, aa.cpu(), drv)
    routed = EnvState(B, A, device=DEV, with_slot_route=True)
    with pytest.raises(_lib.TdeError, match="^tde_env_step_driven: tde_env_step_driven: state.slot_route is set: "):
        ops.env_step_driven(env.tde_cfg, env.dworld, routed, aa, drv)
    L = _lib.load()
    rc = L.tde_env_step_driven(C.byref(env.tde_cfg), C.byref(env.dworld.struct), C.byref(env.state.struct), None, drv.view(torch.uint8).data_ptr(), None)
    assert rc != 0 and L.tde_last_error().decode() == "tde_env_step_driven: driven is set and agent_action is NULL"
    before = env.state.host()
    torch.cuda.synchronize()
    assert_same(env.state.host(), before, AGENT + ENV)         # nothing was launched


def test_render_agents_equals_render_scene_with_hand_built_views():
    A, B = 16, 5
    world = config_zoo.world(None, A)
    env = make_env(world, B)
    env.reset()
    envs, slots = [0, 3, 3, 4, 1], [0, 5, 15, 1, 7]
    got = env.render_agents(envs, slots)
    h = env.state.host()
    g = np.array(envs) * A + np.array(slots)
    cam = dev(np.stack([h["x"][g], h["y"][g], h["psi"][g]], -1).astype(np.float32))
    want = ops.render_scene(env.tde_cfg, env.dworld, env.state, envs, 64, 64, env._fov, cam, flags=env._rflags)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, 3, 64, 64) and torch.equal(got, want)
    ego = ops.render_scene(env.tde_cfg, env.dworld, env.state, [0], 64, 64, env._fov, "ego", flags=env._rflags)
    assert torch.equal(got[:1], ego) and len(torch.unique(got)) > 2
    wide = env.render_agents([2], [4], H=48, W=80, fov=60.0)
    assert tuple(wide.shape) == (1, 3, 48, 80)
    with pytest.raises(ValueError, match=r"^slots must be in \[0, 16\)$"):
        env.render_agents([0], [16])


def test_a_driven_step_is_captured_in_and_replayed_from_a_graph():
    A, B = 16, 6
    world = config_zoo.world(None, A)
    graphed, eager = make_env(world, B, max_steps=20), make_env(world, B, max_steps=20)
    graphed.reset(), eager.reset()
    rng = np.random.default_rng(2)
    aa_h, drv_h = random_drive(rng, graphed.state.host(), A)
    act, aa, drv = dev(config_zoo.actions(None, B, A, T=1)[0]), dev(aa_h), dev(drv_h)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        graphed.step(act, aa, drv)                             # warm-up on the capturing stream
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):                 # (one stream: no parallel branches)
            graphed.step(act, aa, drv)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    for _ in range(2):
        eager.step(act, aa, drv)
    torch.cuda.synchronize()
    assert_same(graphed.state.host(), eager.state.host(), AGENT + ENV + ("obs",))
    assert int(eager.state.host()["steps"].max()) == 2
