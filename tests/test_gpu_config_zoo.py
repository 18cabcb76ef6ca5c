"""The kernel matrix crossed with the config zoo (tests/config_zoo.py; its CPU conditions: tests/test_config_zoo_cpu.py).  Every other
GPU test runs the step and rollout kernels at one point of tde_config - the defaults; here every compiled form of them at 4, 16, 64
and 128 slots runs under each zoo entry against the oracle, bit for bit, with the kernel matrix's own helpers and checks; two
configurations alternate on one device world (the shared first-step gap table, the action-cache key and the argument-block pool see
both); and the forecasts, the planner and the plan judge - each a restatement of the step body - are held to their numpy checkers and
to real steps under the two entries that move every constant they read."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle  # noqa: E402
from tests import config_zoo as Z  # noqa: E402
from tests import forecast_ref as Fr  # noqa: E402
from tests import forecast_scene_ref as Sr  # noqa: E402
from tests import kernel_matrix as km  # noqa: E402
from tests import plan_set_ref as S  # noqa: E402
from tests.plan_gpu_util import bits, check_plan_action, check_score_plans, on_device  # noqa: E402
from tests.test_gpu_forecast_scene import _mid_episode_state, _random_actions  # noqa: E402
from tests.test_gpu_kernel_matrix import _Oracle, _cut, _rollout_case, _slices, _step_case  # noqa: E402
from tests.test_gpu_parity import assert_state_equal, dev  # noqa: E402
from torchdriveenv_amd import _abi, _lib, ops  # noqa: E402
from torchdriveenv_amd.config import Planner  # noqa: E402
from torchdriveenv_amd.state import EnvState  # noqa: E402

DEV = "cuda:0"
_dev_worlds = {}


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _on_device(world):
    """one device copy per host world for the module"""
    if id(world) not in _dev_worlds:
        _dev_worlds[id(world)] = (world, world.to_device(DEV))
    return _dev_worlds[id(world)][1]


def _cases(A, kind):
    """the kernel matrix's lit cases of A slots on world `kind`, dispatch edges aside: every rollout form, the step forms with obs and
    magnitudes; and the two operator cases that launch step-path kernels (they are listed in the unlit group only)"""
    lit = [c for c in km.CASES if c.A == A and c.world == kind and c.lights and not c.edge and
           (c.entry == "rollout" or (c.entry == "step" and c.obs and c.mag))]
    ops_ = [c for c in km.CASES if c.A == A and c.world == kind and not c.lights and not c.edge and c.entry in ("post_step", "first_gaps")]
    return ops_ + lit


# ---- (a) every form, per entry ------------------------------------------------------------------------------------------------------------

def _edge_state(cfg, world, want, acts, B, A):
    """the oracle's last state of the run driven 8 steps further without auto-reset, so that the infractions of those steps are still
    in it (a re-spawned ego has none)"""
    hs = EnvState(B, A)
    hs.load(want.snap[want.T - 1][0])
    cfg_na = _abi.TdeConfig.from_buffer_copy(cfg)
    cfg_na.flags &= ~_abi.F_AUTORESET
    for t in range(8):
        hs["action"][...] = acts[t]
        oracle.env_step(cfg_na, world, hs)
    return hs


@pytest.mark.parametrize("A", Z.SLOTS)
@pytest.mark.parametrize("name", Z.NAMES)
def test_every_form_under_the_entry(name, A):
    cu = _cu()
    B, T = Z.batch(A, cu), Z.steps(name)
    cfg = Z.config(name, A)
    acts_h = Z.actions(name, B, A)
    acts = dev(acts_h)
    forms = 0
    # (the junction maps up to 64 slots, the town at 128 - and the town below 128 for the forms compiled for the large grid)
    for kind in (("town",) if A == 128 else ("junctions", "town")):
        cases = _cases(A, kind)
        if not cases:
            continue
        world = Z.world(name, A, kind)
        dw = _on_device(world)
        want = _Oracle(cfg, world, A, _slices(B, ()), acts_h, T=T)
        n_end, n_hit, n_red = want.events()
        assert n_end > 0 and n_hit > 0 and n_red > 0, (name, A, kind, n_end, n_hit, n_red)        # nothing passes vacuously
        for c in sorted(cases, key=lambda c: c.entry != "first_gaps"):
            assert c.B(cu) == B
            if c.entry == "first_gaps":
                fg = dw.tensors["first_gap"].view(torch.int32)
                fg.zero_()
                ops.first_gaps(cfg, dw)
                torch.cuda.synchronize()
                keyed = (fg.view(world.n_scn, A, 2)[:, :, 1] != 0).cpu().numpy()
                assert not keyed[:, 0].any() and keyed[:, 1:].all(), c.id()
            elif c.entry == "rollout":
                _rollout_case(c, cfg, dw, B, A, acts, want, T=T)
            else:
                _step_case(c, cfg, dw, B, A, acts, want, T=T)
            forms += 1
        if name in ("thin_edge", "thick_edge") and kind == ("town" if A == 128 else "junctions"):
            hs = _edge_state(cfg, world, want, acts_h, B, A)
            mag = oracle.ego_infractions(cfg, world, hs)
            assert (mag[:, 0] > 0).any() and (mag[:, 0] == 0).any(), (name, A)
            ds = EnvState(B, A, device=DEV)
            ds.load(hs.host())
            got = ops.ego_infractions(cfg, dw, ds).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), mag.view(np.uint32)), (name, A, "ego_infractions")
            img = ops.render_ego(cfg, dw, ds, H=64, W=64, fov=35.0).cpu().numpy()
            ref = oracle.render_ego(cfg, world, hs, H=64, W=64, fov=35.0)
            assert np.array_equal(img, ref), (name, A, "render_ego", int((img != ref).sum()))
    assert forms >= 5, (name, A, forms)


# ---- (b) two configurations, one device world ---------------------------------------------------------------------------------------------

def _same_state(hs, d, B, A, where, skip=()):
    want, got = _cut(hs.host(), A, 0, B, skip), _cut(d.host(), A, 0, B, skip)
    assert_state_equal({k: v for k, v in want.items() if k in got}, got, where)


@pytest.mark.parametrize("A", [16, 128])
def test_two_configurations_alternate_on_one_device_world(A):
    """the default configuration and slow_wide step two states in turn on ONE device world: at 16 slots the three-role step, then a
    10-step two-role rollout on each state; at 128 slots the wide step.  Each state equals its own oracle run at every step (reward,
    done bits, magnitudes) and as a whole after the check steps."""
    cu = _cu()
    B, T = Z.batch(A, cu), Z.steps("slow_wide")
    assert Z.threshold("slow_wide") == Z.threshold(None)
    world = Z.world(None, A)
    dw = _on_device(world)
    names = (None, "slow_wide")
    cfgs = [Z.config(n, A) for n in names]
    assert bytes(cfgs[0]) != bytes(cfgs[1])
    acts_h = [Z.actions("slow_wide", B, A, T + 10), Z.actions("slow_wide", B, A + 1, T + 10)]
    acts = [dev(a) for a in acts_h]
    hs = [EnvState(B, A) for _ in names]
    ds = [EnvState(B, A, device=DEV, with_obs=True, with_magnitudes=True) for _ in names]
    for i in range(2):
        oracle.env_reset(cfgs[i], world, hs[i])
        ops.env_reset(cfgs[i], dw, ds[i])
        _same_state(hs[i], ds[i], B, A, f"{names[i]} (reset)")
    ended = [0, 0]
    for t in range(T):
        for i in range(2):
            hs[i]["action"][...] = acts_h[i][t]
            oracle.env_step(cfgs[i], world, hs[i])
            ops.env_step(cfgs[i], dw, ds[i], action=acts[i][t])
            where = f"{names[i]}, A = {A}, step {t}"
            for k in ("reward", "magnitudes"):
                assert np.array_equal(ds[i][k].cpu().numpy().view(np.uint32), hs[i][k].view(np.uint32)), (k, where)
            assert np.array_equal(ds[i]["done_bits"].cpu().numpy(), hs[i]["done_bits"]), where
            ended[i] += int((hs[i]["done_bits"] & 3 != 0).sum())
            if t in (0, 1, 2, T // 2, T - 1):
                _same_state(hs[i], ds[i], B, A, where, skip=("magnitudes",))
    assert min(ended) > 0                                                            # re-spawns (first steps again) under both
    if A == 16:
        _lib.kernel_override(rollout="duo")
        try:
            for i in range(2):
                r, dn = ops.env_rollout(cfgs[i], dw, ds[i], acts[i][T:T + 10].contiguous())
                torch.cuda.synchronize()
                wr, wd = oracle.env_rollout(cfgs[i], world, hs[i], acts_h[i][T:T + 10])
                assert np.array_equal(r.cpu().numpy().view(np.uint32), wr.view(np.uint32)), (names[i], "rollout reward")
                assert np.array_equal(dn.cpu().numpy(), wd), (names[i], "rollout done")
        finally:
            _lib.kernel_override()
        for i in range(2):
            _same_state(hs[i], ds[i], B, A, f"{names[i]} after the rollout",
                        skip=("done_bits", "magnitudes", "ep_return", "ep_final", "ep_final_len"))


# ---- (c) the restated consumers -----------------------------------------------------------------------------------------------------------

T_MAX = _abi.FORECAST_MAX_T


def _consumer_scene(name):
    A, B = 16, 33
    world = Z.world(name, A)
    over = Z.overrides(name)
    cfg = S.lights_cfg(world, seed=300 + Z.NAMES.index(name), terminated_at_infraction=0, **over)
    cfg.flags &= ~_abi.F_AUTORESET
    assert cfg.flags & _abi.F_TRAFFIC_LIGHTS
    hs = _mid_episode_state(cfg, world, B, seed=40 + Z.NAMES.index(name), **over)
    return cfg, world, hs, A, B


@pytest.mark.parametrize("name", ["slow_wide", "fast_narrow"])
def test_forecasts_under_the_entry(name):
    """tde_forecast_agents and tde_forecast_scene at T = 96 == their restatements, and tde_forecast_scene == 32 real tde_env_step
    launches, the config handed to ops directly (dt is not an EnvConfig field)"""
    cfg, world, hs, A, B = _consumer_scene(name)
    act = _random_actions(B, T_MAX, 5 * A)
    want_free = Fr.forecast(cfg, world, hs, T_MAX)
    want = Sr.forecast_scene(cfg, world, hs, T_MAX, ego_action=act)
    assert (bits(want[:, :, 1:]) != bits(want_free[:, :, 1:])).any()                 # queues: the leader sweep decides somewhere
    dw, ds = on_device(world, hs)
    dact = torch.from_numpy(act).to(DEV)
    got_free = ops.forecast_agents(cfg, dw, ds, T_MAX).cpu().numpy()
    got = ops.forecast_scene(cfg, dw, ds, T_MAX, dact).cpu().numpy()
    for g, w, what in ((got_free, want_free, "forecast_agents"), (got, want, "forecast_scene")):
        bad = np.argwhere(bits(g) != bits(w))
        assert len(bad) == 0, (name, what, len(bad), bad[:6].tolist(), g[tuple(bad[0][:3])], w[tuple(bad[0][:3])])
    # the environment as oracle
    fc = torch.from_numpy(got[:, :32]).to(DEV)
    pres = (ds["present"].view(B, A) != 0)[..., None]
    for h in range(1, 33):
        ops.env_step(cfg, dw, ds, action=dact[:, h - 1].contiguous())
        now = torch.stack([ds[n].view(B, A) for n in ("x", "y", "psi", "v")], -1)
        now = torch.where(pres, now, torch.zeros_like(now))
        diff = now.view(torch.int32) != fc[:, h - 1].view(torch.int32)
        assert not diff.any(), (name, h, torch.nonzero(diff)[:4].tolist())


@pytest.mark.parametrize("name", ["slow_wide", "fast_narrow"])
def test_planner_and_plan_judge_under_the_entry(name):
    """tde_plan_action and tde_score_plans, without and with forecast=, == their restatements (both bindings), with an `only` mask"""
    cfg, world, hs, A, B = _consumer_scene(name)
    pl = Planner()
    only = (np.arange(B) % 4 != 1).astype(np.uint8)
    a, d = check_plan_action(cfg, world, hs, pl, only=only, what=name)
    picked = d[only != 0]
    assert (picked["n_safe"] < pl.n_candidates).any() and len(np.unique(picked["winner"])) > 1, name
    rng = np.random.default_rng(9)
    N, K, tail = 63, 4, 10
    seq = S.calm_knots(rng, S.random_knots(rng, B, N, K))
    fc = Sr.forecast_scene(cfg, world, hs, pl.horizon + tail)
    for f in (None, fc):
        res = check_score_plans(cfg, world, hs, pl, seq, -(-pl.horizon // K), tail, only=only, forecast=f, what=(name, f is not None))
        fs = res["f"][only != 0]
        assert (fs < pl.horizon + tail + 1).any() and (fs == pl.horizon + tail + 1).any(), name
