"""tde_env_reset_to, tde_eval_advance and BatchedWaypointEnv.evaluate on the GPU.  Every comparison is exact: the new kernels add no
floating-point expression beyond float64 additions in step order.  The reference of a forced-scenario reset is tde_env_reset (and
the oracle's reset) on the world that holds only that scenario (tests/eval_ref.py); the reference of the advance is the numpy
restatement there, driven by the oracle's step."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle  # noqa: E402
from tests import config_zoo as zoo  # noqa: E402
from tests import eval_ref as E  # noqa: E402
from tests.test_gpu_parity import assert_state_equal, dev  # noqa: E402
from torchdriveenv_amd import _abi, ops  # noqa: E402
from torchdriveenv_amd.state import EnvState  # noqa: E402

DEV = "cuda:0"
REC = _abi.EPISODE_RECORD_DTYPE
FLAGS = (_abi.F_ALL | _abi.F_TRAFFIC_LIGHTS) & ~_abi.F_AUTORESET
SHAPES = [(6, 4), (6, 16), (2, 128)]          # a partial last workgroup at 4 and 16 slots; at 128 an env spans two wavefronts
_cache = {}


def _worlds(A):
    """the 4-scenario world of A slots, its single-scenario worlds and all five on the device (once per A)"""
    if A not in _cache:
        from torchdriveenv_amd.synth import synthetic_world

        w = synthetic_world(n_scn=4, A=A, seed=40 + A, n_maps=2)
        singles = E.singles_of(w)
        _cache[A] = (w, singles, w.to_device(DEV), [s.to_device(DEV) for s in singles])
    return _cache[A]


def _same_but(a, b, skip, where):
    """every array of two device states byte for byte, but those in `skip`"""
    ha, hb = a.host(), b.host()
    assert set(ha) == set(hb)
    for k in ha:
        if k not in skip:
            assert np.array_equal(ha[k].view(np.uint8), hb[k].view(np.uint8)), (where, k)


@pytest.mark.parametrize("B,A", SHAPES)
def test_reset_to_equals_reset_on_the_single_scenario_world(B, A):
    w, singles, dw, dsingles = _worlds(A)
    cfg = _abi.default_config(seed=77 + A, flags=FLAGS)
    for s in range(4):
        full, one, host = EnvState(B, A, device=DEV), EnvState(B, A, device=DEV), EnvState(B, A)
        ids = torch.full((B,), s, dtype=torch.int32, device=DEV)
        for episode in range(2):
            ops.env_reset_to(cfg, dw, full, ids)
            ops.env_reset(cfg, dsingles[s], one)
            oracle.env_reset(cfg, singles[s], host)
            _same_but(full, one, ("scn",), (s, episode))
            assert full["scn"].tolist() == [s] * B and one["scn"].tolist() == [0] * B and full["episode"].tolist() == [episode + 1] * B
            hh = host.host()
            hh["scn"][:] = s
            assert_state_equal(hh, full.host(), f"reset_to({s}) vs the oracle, episode {episode}")
            # the episodes differ (another random key), and another scenario gives another spawn
            if episode == 0:
                first = full.host()
        assert not np.array_equal(first["x"], full.host()["x"])


@pytest.mark.parametrize("B,A", SHAPES)
def test_reset_to_draws_masks_and_leaves_bad_ids_alone(B, A):
    w, singles, dw, _ = _worlds(A)
    cfg = _abi.default_config(seed=5, flags=FLAGS)
    ref, got = EnvState(B, A, device=DEV), EnvState(B, A, device=DEV)
    ops.env_reset(cfg, dw, ref)
    ops.env_reset_to(cfg, dw, got, None)                                        # scn = NULL
    _same_but(ref, got, (), "scn NULL")
    ops.env_reset(cfg, dw, ref)
    ops.env_reset_to(cfg, dw, got, torch.full((B,), -1, dtype=torch.int32, device=DEV))
    _same_but(ref, got, (), "every id -1")
    mask = torch.tensor([1, 0] * (B // 2), dtype=torch.uint8, device=DEV)
    ops.env_reset(cfg, dw, ref, mask)
    ops.env_reset_to(cfg, dw, got, torch.full((B,), -7, dtype=torch.int32, device=DEV), mask)
    _same_but(ref, got, (), "masked, negative ids")
    assert ref["episode"].tolist() == [3, 2] * (B // 2)
    # mixed: env 0 forced to 2, env 1 drawn, the last env an id past the world - left exactly as it is, counters included
    before = got.host()
    ids = np.full(B, -1, np.int32)
    ids[0], ids[-1] = 2, 4
    ops.env_reset_to(cfg, dw, got, dev(ids))
    host = EnvState(B, A)
    host.load(before)
    E.reset_to(cfg, w, host, ids, None, singles)
    assert_state_equal(host.host(), got.host(), "mixed ids vs the restatement")
    after = got.host()
    for k, a in before.items():
        n = len(a) // B                                              # rows per env of this array
        assert np.array_equal(a[(B - 1) * n:].view(np.uint8), after[k][(B - 1) * n:].view(np.uint8)), k
    assert after["scn"][0] == 2 and after["episode"].tolist() == [before["episode"][e] + (e != B - 1) for e in range(B)]
    ids[-1] = 2 ** 31 - 1
    ops.env_reset_to(cfg, dw, got, dev(ids), dev(np.array([0] * (B - 1) + [1], np.uint8)))
    for k, a in after.items():
        assert np.array_equal(a.view(np.uint8), got.host()[k].view(np.uint8)), k


def test_reset_to_under_a_64_bit_seed_and_ego_only_attributes():
    A, B = 16, 6
    cfg = zoo.config("wide_seed", A, flags=(zoo.FLAGS | _abi.F_EGO_ONLY_ATTRS) & ~_abi.F_AUTORESET)
    assert cfg.seed > 2 ** 32 and cfg.flags & _abi.F_EGO_ONLY_ATTRS
    w = zoo.world("wide_seed", A)
    dw = w.to_device(DEV)
    for s in (1, 6):
        ws = E.single_scenario_world(w, s)
        full, one = EnvState(B, A, device=DEV), EnvState(B, A, device=DEV)
        for episode in range(2):
            ops.env_reset_to(cfg, dw, full, torch.full((B,), s, dtype=torch.int32, device=DEV))
            ops.env_reset(cfg, ws.to_device(DEV), one)
            _same_but(full, one, ("scn",), (s, episode))
        ego_len = full.host()["len"].reshape(B, A)[:, 0]
        assert len(set(ego_len.tolist())) == B and (ego_len >= 4.8).all() and (ego_len <= 5.5).all()


def _scripted(hs):
    a = np.zeros((hs.B, 2), np.float32)
    a[:, 0] = 0.5
    a[:, 1] = np.where((hs["scn"] % 2 == 1) & (hs["steps"] >= 3), np.float32(0.3), np.float32(0.0))
    return a


@pytest.mark.parametrize("B,A", SHAPES)
def test_eval_advance_equals_the_restatement_after_every_step(B, A):
    w, singles, dw, _ = _worlds(A)
    cfg = _abi.default_config(seed=300 + A, flags=FLAGS, max_steps=12, distance_cutoff=0.25)
    R = 3
    plan = np.array([[(e + r) % 4 for e in range(B)] for r in range(R)], np.int32)
    plan[1, 1] = -1                                                  # env 1's plan ends early: one episode, the third row never read
    hs, ds = EnvState(B, A), EnvState(B, A, device=DEV, with_obs=True)
    hev = E.new_eval(plan)
    dev_ev = ops.EvalBuffers(plan, DEV)
    dev_ev.active.copy_(dev(hev["active"]))
    E.reset_to(cfg, w, hs, plan[0], None, singles)
    ops.env_reset_to(cfg, dw, ds, dev(plan[0]))
    assert_state_equal(hs.host(), ds.host(), "reset_to")
    obs2 = torch.zeros((B, 8), dtype=torch.float32, device=DEV)
    t = n_respawn = 0
    while hev["active"].any():
        assert t < R * 12
        act = _scripted(hs)
        hs["action"][...] = act
        oracle.env_step(cfg, w, hs)
        n_respawn += int(E.advance(cfg, w, hs, hev, singles).sum())
        ops.env_step(cfg, dw, ds, action=dev(act))
        ops.eval_advance(cfg, dw, ds, dev_ev)
        assert_state_equal(hs.host(), ds.host(), f"step {t}")
        assert dev_ev.round.cpu().numpy().tolist() == hev["round"].tolist(), t
        assert dev_ev.active.cpu().numpy().tolist() == hev["active"].tolist(), t
        assert dev_ev.acc.cpu().numpy().tobytes() == hev["acc"].tobytes(), t
        assert dev_ev.results.cpu().numpy().tobytes() == hev["results"].tobytes(), t
        ops.state_obs(dw, ds, obs2)
        assert torch.equal(obs2, ds["obs"]), t
        t += 1
    rec = hev["results"]
    done = np.array([[r < hev["round"][e] for e in range(B)] for r in range(R)])
    assert hev["round"].tolist() == [3, 1] + [3] * (B - 2) and n_respawn == 2 * (B - 1)
    assert np.array_equal(rec["scn"][done], plan[done]) and not rec[~done].view(np.uint8).any()
    assert (rec["bits"][done] & 2).any() and (rec["bits"][done] & 4).any() and (rec["length"][done] == 12).any()
    assert (rec["length"][done] < 12).any() and (rec["psi_sum"][done] != 0).any()
    # an inactive env is not touched: one more step + advance changes no eval array
    ops.env_step(cfg, dw, ds, action=dev(act))
    ops.eval_advance(cfg, dw, ds, dev_ev)
    assert dev_ev.results.cpu().numpy().tobytes() == rec.tobytes() and not dev_ev.acc.cpu().numpy().any() and not dev_ev.active.any()


def test_evaluate_planner_records_every_job_once_under_its_scenario():
    from torchdriveenv_amd.config import EnvConfig
    from torchdriveenv_amd.env import BatchedWaypointEnv

    w = _worlds(16)[0]
    res = {}
    for B in (3, 8):
        env = BatchedWaypointEnv(EnvConfig(seed=9, max_environment_steps=24, distance_cutoff=0.25), w, num_envs=B, agents_per_env=16,
                                 obs_mode="state")
        full = int(env.tde_cfg.flags)
        res[B] = env.evaluate("planner", repeats=2)
        assert int(env.tde_cfg.flags) == full and env.auto_reset
        r = res[B]
        assert len(r) == 8 and r.scenario.tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
        assert ((r.bits & 3) != 0).all() and (r.length >= 1).all() and (r.length <= 24).all()
        m = r.metrics()
        n = 8
        bits = r.bits.numpy()
        want = {"mean_episode_reward": sum(r.episode_return.tolist()) / n, "mean_episode_length": sum(r.length.tolist()) / n,
                "offroad_rate": int(((bits >> 2) & 1).sum()) / n, "collision_rate": int(((bits >> 3) & 1).sum()) / n,
                "traffic_light_violation_rate": int(((bits >> 4) & 1).sum()) / n, "success_percentage": int(((bits >> 1) & 1).sum()) / n,
                "reached_waypoint_num": sum(r.reached.tolist()) / n, "psi_smoothness": sum(r.psi_smoothness.tolist()) / n,
                "speed_smoothness": sum(r.speed_smoothness.tolist()) / n}
        assert m == want and all(np.isfinite(v) for v in m.values())
        env.reset()                                                   # (a training env resets after an evaluation)
    # jobs 0..2 are (env j, episode 0) in both batches: the same episodes, bit for bit; the others only share their scenario
    for f in ("episode_return", "length", "reached", "scenario", "bits", "psi_smoothness", "speed_smoothness"):
        a, b = getattr(res[3], f)[:3], getattr(res[8], f)[:3]
        assert a.numpy().tobytes() == b.numpy().tobytes(), f
    # a callable policy and the scenario option through the env's reset
    env = BatchedWaypointEnv(EnvConfig(seed=9, max_environment_steps=8), w, num_envs=3, agents_per_env=16, obs_mode="state")
    coast = torch.zeros((3, 2), dtype=torch.float32, device=DEV)
    r = env.evaluate(lambda obs: coast, cases=[3, 3, 1, 0])
    assert r.scenario.tolist() == [3, 3, 1, 0] and (r.length <= 8).all()
    env.reset(options={"scenario": [2, -1, 0]})
    assert env.state["scn"][0] == 2 and env.state["scn"][2] == 0
    with pytest.raises(ValueError):
        env.reset(options={"scenario": 4})


_both = {}                                    # (obs_mode, frame_stack) -> the ext and the ctypes env, kept for the reset test


@pytest.mark.parametrize("obs_mode,frame_stack", [("state", 1), ("birdview", 2)])
def test_evaluate_is_the_same_through_both_bindings(obs_mode, frame_stack):
    """evaluate() through the extension's handle and through ops.CtypesHandle: every field of the results byte for byte, the flags
    restored.  3 envs x 8 jobs: envs re-spawn mid-evaluation (eval_advance, and with the birdview FrameStack.rerender with a mask)"""
    from torchdriveenv_amd.config import EnvConfig
    from torchdriveenv_amd.env import BatchedWaypointEnv

    w = _worlds(16)[0]
    res = {}
    for binding in ("ext", "ctypes"):
        env = BatchedWaypointEnv(EnvConfig(seed=9, max_environment_steps=24, distance_cutoff=0.25), w, num_envs=3, agents_per_env=16,
                                 obs_mode=obs_mode, frame_stack=frame_stack, binding=binding)
        assert env.binding == binding
        full = int(env.tde_cfg.flags)
        res[binding] = env.evaluate("planner", repeats=2)
        assert int(env.tde_cfg.flags) == full and env.auto_reset, binding
        _both.setdefault((obs_mode, frame_stack), {})[binding] = env
    assert len(res["ext"]) == 8 and res["ext"].scenario.tolist() == [0, 1, 2, 3, 0, 1, 2, 3]
    for f in ("episode_return", "length", "reached", "scenario", "bits", "psi_smoothness", "speed_smoothness"):
        a, b = getattr(res["ext"], f), getattr(res["ctypes"], f)
        assert a.dtype == b.dtype and a.numpy().tobytes() == b.numpy().tobytes(), f


@pytest.mark.parametrize("obs_mode,frame_stack", [("state", 1), ("birdview", 2)])
def test_reset_to_scenario_and_masked_reset_are_the_same_through_both_bindings(obs_mode, frame_stack):
    """on the envs the evaluation above left: reset(options={"scenario": ...}), then reset(mask=...), through either handle"""
    if (obs_mode, frame_stack) not in _both:                         # (run alone: the evaluation makes the envs)
        test_evaluate_is_the_same_through_both_bindings(obs_mode, frame_stack)
    e_ext, e_ct = (_both[(obs_mode, frame_stack)][b] for b in ("ext", "ctypes"))
    for kw in (dict(options={"scenario": [2, -1, 0]}), dict(mask=[1, 0, 1])):
        o_ext, o_ct = e_ext.reset(**kw), e_ct.reset(**kw)
        assert torch.equal(o_ext, o_ct), kw
        for k in ("x", "scn", "episode"):
            assert torch.equal(e_ext.state[k], e_ct.state[k]), (kw, k)
        if "options" in kw:
            assert e_ext.state["scn"][0] == 2 and e_ext.state["scn"][2] == 0


def test_graph_capture_of_step_and_advance_replays_to_the_same_records():
    B, A = 6, 16
    w, _, dw, _ = _worlds(A)
    cfg = _abi.default_config(seed=12, flags=FLAGS, max_steps=10, distance_cutoff=0.25)
    plan = np.array([[(e + r) % 4 for e in range(B)] for r in range(2)], np.int32)
    act = np.zeros((B, 2), np.float32)
    act[:, 0], act[1::2, 1] = 0.5, 0.3
    states, evs = [], []
    for _ in range(2):
        ds = EnvState(B, A, device=DEV)
        ds["action"].copy_(dev(act))
        ev = ops.EvalBuffers(plan, DEV)
        ev.active.fill_(1)
        ops.env_reset_to(cfg, dw, ds, dev(plan[0]))
        states.append(ds); evs.append(ev)
    ops.first_gaps(cfg, dw)                                          # (outside the capture)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        # warm-up on the capturing stream, on the eager twin: one step + advance
        ops.env_step(cfg, dw, states[1])
        ops.eval_advance(cfg, dw, states[1], evs[1])
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):                   # one capture, one stream: no parallel branches
            ops.env_step(cfg, dw, states[0])
            ops.eval_advance(cfg, dw, states[0], evs[0])
    torch.cuda.synchronize()
    for t in range(20):
        graph.replay()
        if t:
            ops.env_step(cfg, dw, states[1])
            ops.eval_advance(cfg, dw, states[1], evs[1])
    torch.cuda.synchronize()
    assert not evs[0].active.any() and evs[0].round.tolist() == [2] * B
    for n in ("round", "active", "acc", "results"):
        assert torch.equal(getattr(evs[0], n), getattr(evs[1], n)), n
    rec = evs[0].records()
    assert np.array_equal(rec["scn"], plan) and ((rec["bits"] & 3) != 0).all()
    _same_but(states[0], states[1], (), "captured vs eager")
