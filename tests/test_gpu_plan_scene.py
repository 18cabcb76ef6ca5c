"""GPU tests of tde_score_plans_scene (csrc/tde_plan_scene.hip): the kernel through both bindings held bit for bit against the
restatement by composition (tests/plan_scene_ref.py) at the edges of the virtual-env packing; against the existing kernels
(replicated state -> tde_forecast_scene -> tde_score_plans_forecast); its look-ahead against real tde_env_step launches; plan_actions()
under config.PlanReact; graph capture."""
import numpy as np
import pytest
import torch

from oracle import oracle
from tests import plan_scene_ref as Pr
from tests import plan_set_ref as S
from tests.plan_gpu_util import DEV, bits, on_device
from tests.test_gpu_forecast_scene import _world
from tests.test_plan_scene_cpu import H, TAIL, lookahead_inputs
from torchdriveenv_amd import _abi, _ext, ops
from torchdriveenv_amd.config import EnvConfig, PlanReact, Planner
from torchdriveenv_amd.env import BatchedWaypointEnv
from torchdriveenv_amd.state import EnvState

pytestmark = pytest.mark.gpu


def _call(binding, cfg, dw, ds, pl, dseq, knot_len, tail, m, cost, fail, act, dg):
    if binding == "ctypes":
        ops.score_plans_scene(cfg, dw, ds, pl, dseq, knot_len, tail, m, cost, fail, act, dg)
    else:
        _ext.env_handle(cfg, dw, ds).score_plans_scene(dseq, int(knot_len), int(tail), cost, fail, int(pl.horizon), float(pl.v_target),
                                                       float(pl.margin), float(pl.w_progress), float(pl.w_speed), float(pl.w_steer), m, act,
                                                       dg, int(cfg.flags))


def check_scene(cfg, world, hs, pl, seq, knot_len, tail, only=None, what=""):
    """the kernel (both bindings) on the device copy of `hs` == the restatement, every output, over sentinel-filled buffers; without
    action / diag the same cost and fail_step; returns the restatement's result"""
    B, N = seq.shape[:2]
    c0, f0 = np.full((B, N), -5.0, np.float32), np.full((B, N), -9, np.int32)
    a0, d0 = np.full((B, 2), -3.0, np.float32), np.full((B, 4), -7, np.int32)
    want = Pr.score(cfg, world, hs, pl, seq, knot_len, tail, only=only, cost=c0, fail_step=f0, out=a0, diag=d0)
    dw, ds = on_device(world, hs)
    m = torch.from_numpy(np.asarray(only, np.uint8)).to(DEV) if only is not None else None
    dseq = torch.from_numpy(np.ascontiguousarray(seq)).to(DEV)
    for binding in ("ctypes", "ext"):
        cost, fail = torch.from_numpy(c0).to(DEV), torch.from_numpy(f0).to(DEV)
        act, dg = torch.from_numpy(a0).to(DEV), torch.from_numpy(d0).to(DEV)
        cost2, fail2 = torch.from_numpy(c0).to(DEV), torch.from_numpy(f0).to(DEV)
        _call(binding, cfg, dw, ds, pl, dseq, knot_len, tail, m, cost, fail, act, dg)
        _call(binding, cfg, dw, ds, pl, dseq, knot_len, tail, m, cost2, fail2, None, None)
        torch.cuda.synchronize()
        got_f, got_c = fail.cpu().numpy(), cost.cpu().numpy()
        bad = np.argwhere(got_f != want["f"])
        assert len(bad) == 0, (what, binding, "fail_step", len(bad), bad[:6].tolist(), got_f[tuple(bad[0])], want["f"][tuple(bad[0])])
        bad = np.argwhere(bits(got_c) != bits(want["cost"]))
        assert len(bad) == 0, (what, binding, "cost", len(bad), bad[:6].tolist(), got_c[tuple(bad[0])], want["cost"][tuple(bad[0])])
        got_d = dg.cpu().numpy().view(_abi.PLAN_DIAG_DTYPE).reshape(B)
        for n in ("winner", "fail_step", "n_safe"):
            bad = np.flatnonzero(got_d[n] != want["diag"][n])
            assert len(bad) == 0, (what, binding, n, bad[:8].tolist(), got_d[bad[:4]], want["diag"][bad[:4]])
        assert np.array_equal(got_d["cost"].view(np.uint32), want["diag"]["cost"].view(np.uint32)), (what, binding, "diag cost")
        assert np.array_equal(bits(act.cpu().numpy()), bits(want["action"])), (what, binding, "action")
        assert torch.equal(cost2.view(torch.int32), cost.view(torch.int32)) and torch.equal(fail2, fail), (what, binding, "no action / diag")
    after = ds.host()
    for n in ("x", "y", "psi", "v", "route_wp", "steps", "target_idx"):
        assert np.array_equal(np.asarray(after[n]), np.asarray(hs[n])), n       # the device state is not written
    return want


# (A, B, N): 16 virtual envs per wavefront; four; one; two wavefronts per virtual env.  N is never a multiple of 256 / A: workgroups
# straddle envs and the last one is partial
SHAPES = {4: ("junctions", 9, 65), 16: ("junctions", 5, 63), 64: ("junctions", 3, 7), 128: ("town", 2, 5)}
_inputs = {}


def _mid_episode_state(cfg, world, B, seed):
    """25 oracle steps under random ego actions with auto-reset, then the last env reset again (step 0: the first-step rule) and every
    other env's step counter moved on (the lights' phase and the replay records follow it)"""
    drive = S.lights_cfg(world, seed=seed, terminated_at_infraction=1)
    drive.flags = cfg.flags | _abi.F_AUTORESET
    hs = S.reset_state(drive, world, B)
    rng = np.random.default_rng(seed)
    for _ in range(25):
        hs["action"][...] = np.stack([rng.uniform(-1, 1, B), rng.uniform(-0.3, 0.3, B)], -1).astype(np.float32)
        oracle.env_step(drive, world, hs)
    fresh = (np.arange(B) == B - 1).astype(np.uint8)
    oracle.env_reset(drive, world, hs, mask=fresh)
    hs["steps"][::2] += 7 * (1 + np.arange(len(hs["steps"][::2]), dtype=np.int32) % 9)
    assert len(set(np.asarray(hs["steps"]).tolist())) >= 2
    return hs


def _scene_inputs(A, lights=True):
    """(cfg, world, mid-episode host state) of SHAPES[A], made once"""
    if (A, lights) not in _inputs:
        kind, B, _ = SHAPES[A]
        world = _world(kind, A)
        cfg = S.lights_cfg(world, seed=200 + A)
        if not lights:
            cfg.flags &= ~_abi.F_TRAFFIC_LIGHTS
        hs = _mid_episode_state(cfg, world, B, seed=A + 3)
        if A == 128:
            pres = np.asarray(hs["present"]).reshape(B, A) != 0
            assert pres[:, 64:].any() and (~pres).any()
        _inputs[(A, lights)] = (cfg, world, hs)
    return _inputs[(A, lights)]


@pytest.mark.parametrize("K,knot_len,tail", [(1, 32, 0), (2, 16, 40), (32, 1, 64)])
@pytest.mark.parametrize("A", [4, 16, 64, 128])
def test_kernel_equals_the_restatement(A, K, knot_len, tail):
    cfg, world, hs = _scene_inputs(A)
    _, B, N = SHAPES[A]
    rng = np.random.default_rng(10 * A + K)
    seq = S.calm_knots(rng, S.random_knots(rng, B, N, K))
    want = check_scene(cfg, world, hs, Planner(), seq, knot_len, tail, what=(A, K, tail))
    if A <= 16 and tail:
        HT = 32 + tail
        assert (want["f"] <= HT).any() and (want["f"] == HT + 1).any()         # both verdicts occur


@pytest.mark.parametrize("A", [16, 128])
def test_lights_off_only_mask_and_wild_knots(A):
    cfg, world, hs = _scene_inputs(A, lights=False)
    _, B, N = SHAPES[A]
    rng = np.random.default_rng(3 * A)
    seq = S.calm_knots(rng, S.random_knots(rng, B, N, 4, wild=True))
    assert np.isnan(seq).any() and (np.abs(seq[..., 0]) > 1).any()
    only = (np.arange(B) % 3 != 1).astype(np.uint8)
    want = check_scene(cfg, world, hs, Planner(margin=0.0), seq, 8, 10, only=only, what=(A, "dark, only, wild"))
    assert (want["cost"][only == 0] == -5.0).all() and (want["f"][only == 0] == -9).all() and (want["f"][only != 0] > 0).all()


@pytest.mark.parametrize("A", [16, 128])
def test_kernel_equals_the_existing_kernels(A):
    """replicate the device state with torch, tde_forecast_scene under the effective actions, tde_score_plans_forecast with N = 1 per
    virtual env: the same bits"""
    cfg, world, hs = _scene_inputs(A)
    _, B, N = SHAPES[A]
    K, knot_len, tail = 2, 16, 40
    pl = Planner()
    rng = np.random.default_rng(A + 1)
    seq = S.calm_knots(rng, S.random_knots(rng, B, N, K))
    dw, ds = on_device(world, hs)
    dseq = torch.from_numpy(seq).to(DEV)
    cost = torch.zeros((B, N), dtype=torch.float32, device=DEV)
    fail = torch.zeros((B, N), dtype=torch.int32, device=DEV)
    ops.score_plans_scene(cfg, dw, ds, pl, dseq, knot_len, tail, None, cost, fail)
    big = EnvState(B * N, A, device=DEV)
    for k, a in ds.arrays.items():
        if a is None or k in ("slot_cache", "env_cache", "act_cache"):
            continue
        big.arrays[k].copy_(a.reshape(B, -1).repeat_interleave(N, dim=0).reshape(big.arrays[k].shape))
    ea = torch.from_numpy(Pr.effective_actions(cfg, hs, pl, seq, knot_len, tail)).to(DEV)
    fc = ops.forecast_scene(cfg, dw, big, 32 + tail, ea)
    c1, f1 = ops.score_plans(cfg, dw, big, pl, dseq.view(B * N, 1, K, 2), knot_len, tail, forecast=fc)
    torch.cuda.synchronize()
    assert torch.equal(fail.view(-1), f1.view(-1)), torch.nonzero(fail.view(-1) != f1.view(-1))[:6].tolist()
    assert torch.equal(cost.view(torch.int32).view(-1), c1.view(torch.int32).view(-1))
    if A == 16:
        assert (fail <= 32 + tail).any() and (fail == 33 + tail).any()


def test_lookahead_equals_real_env_steps():
    """margin = 0: fail_step is the step at which tde_env_step ends the episode by an infraction (the CPU test's assertion, with the
    kernel as judge and real launches as environment): 8 sequences per env of one batch, stepped on copies of the state"""
    world = _world("junctions", 16)
    B, N = 24, 8
    cfg, hs, pl, seq = lookahead_inputs(world, B, N, seed=61)
    dw, ds = on_device(world, hs)
    cost, fail = ops.score_plans_scene(cfg, dw, ds, pl, torch.from_numpy(seq).to(DEV), 16, TAIL)
    ea, moved = Pr.effective_actions(cfg, hs, pl, seq, 16, TAIL, with_steps=True)
    _, big = on_device(world, Pr.tile_state(hs, N))

    def step(h, act):
        big["action"].copy_(torch.from_numpy(act))
        ops.env_step(cfg, dw, big)
        return big["done_bits"].cpu().numpy()

    n_fail, n_safe = Pr.check_lookahead(fail.cpu().numpy().ravel(), ea, moved, H + TAIL, step)
    assert n_fail >= 0.10 * B * N and n_safe >= 0.10 * B * N, (n_fail, n_safe)


@pytest.mark.parametrize("binding", ["ext", "ctypes"])
def test_plan_actions_under_plan_react(small_world, binding):
    B = 40
    pl = Planner()
    kw = dict(num_envs=B, device=DEV, obs_mode="state", binding=binding, planner=pl)
    env = BatchedWaypointEnv(EnvConfig(seed=23, distance_cutoff=0.25, max_environment_steps=200), small_world, plan_react=PlanReact(tail=0), **kw)
    plain = BatchedWaypointEnv(EnvConfig(seed=23, distance_cutoff=0.25, max_environment_steps=200), small_world, **kw)
    env.reset()
    plain.reset()
    lat = S.lattice(pl)
    seq = torch.from_numpy(lat).to(DEV)[None, :, None, :].expand(B, len(lat), 1, 2).contiguous()
    zeros = torch.zeros((B, 2), dtype=torch.float32, device=DEV)
    for t in range(2):
        a, d = env.plan_actions(diag=True)
        wa = torch.zeros((B, 2), dtype=torch.float32, device=DEV)
        wd = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
        ops.score_plans_scene(env.tde_cfg, env.dworld, env.state, pl, seq, int(pl.horizon), 0, None, None, None, wa, wd)
        # plan_react=None: the path as it was (tde_plan_action)
        b, g = plain.plan_actions(diag=True)
        pa = torch.zeros((B, 2), dtype=torch.float32, device=DEV)
        pd = torch.zeros((B, 4), dtype=torch.int32, device=DEV)
        ops.plan_action(plain.tde_cfg, plain.dworld, plain.state, pl, pa, None, pd)
        torch.cuda.synchronize()
        assert torch.equal(a.view(torch.int32), wa.view(torch.int32)) and torch.equal(d, wd), (binding, t)
        assert torch.equal(b.view(torch.int32), pa.view(torch.int32)) and torch.equal(g, pd), (binding, t)
        for _ in range(12):
            env.step(zeros)
            plain.step(zeros)
    cost, fail = env.score_plans(seq, react=True)
    assert tuple(cost.shape) == (B, len(lat)) and (fail >= 1).all()
    with pytest.raises(ValueError, match="react=True"):
        env.score_plans(seq, react=True, forecast=env.forecast_scene())


def test_graph_capture():
    """one call under stream capture (an allocation or a synchronisation inside the entry point would fail the capture); the replay
    writes the bits of a plain call"""
    cfg, world, hs = _scene_inputs(16)
    _, B, N = SHAPES[16]
    pl = Planner()
    rng = np.random.default_rng(5)
    dseq = torch.from_numpy(S.calm_knots(rng, S.random_knots(rng, B, N, 2))).to(DEV)
    dw, ds = on_device(world, hs)
    bufs = [dict(cost=torch.zeros((B, N), dtype=torch.float32, device=DEV), fail=torch.zeros((B, N), dtype=torch.int32, device=DEV),
                 act=torch.zeros((B, 2), dtype=torch.float32, device=DEV), dg=torch.zeros((B, 4), dtype=torch.int32, device=DEV))
            for _ in range(2)]

    def run(b):
        ops.score_plans_scene(cfg, dw, ds, pl, dseq, 16, 40, None, b["cost"], b["fail"], b["act"], b["dg"])

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
    assert (bufs[1]["fail"] < 73).any() and (bufs[1]["fail"] == 73).any()
