"""CPU checks of the evaluation entry points (tde_env_reset_to, tde_eval_advance) and their Python surface: the two structs against
the header, every host-side rejection (before any launch: no GPU needed), the reset(options={"scenario": ...}) validation, the
static schedule, EvalResult.metrics() on hand-made records, and the numpy restatement (tests/eval_ref.py) run by the oracle alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import eval_ref as E
from torchdriveenv_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = _abi.EPISODE_RECORD_DTYPE
FLAGS = (_abi.F_ALL | _abi.F_TRAFFIC_LIGHTS) & ~_abi.F_AUTORESET


@pytest.fixture(scope="module")
def world4():
    from torchdriveenv_amd.synth import synthetic_world

    return synthetic_world(n_scn=4, A=4, seed=11, n_maps=2)


def test_structs_match_header(tmp_path):
    rec = ("ret", "psi_sum", "speed_sum", "length", "reached", "scn", "bits", "_pad0", "_pad1")
    evn = ("plan", "round", "active", "acc", "results", "R", "_pad0")
    c = tmp_path / "ev.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tde_hip.h"\nint main(void){printf("%zu", sizeof(tde_episode_record));' +
                 "".join(f'printf(" %zu", offsetof(tde_episode_record, {n}));' for n in rec) + 'printf(" %zu", sizeof(tde_eval));' +
                 "".join(f'printf(" %zu", offsetof(tde_eval, {n}));' for n in evn) +
                 'printf(" %d %d\\n", TDE_ABI_VERSION, (int)(sizeof(&tde_env_reset_to) + sizeof(&tde_eval_advance))); return 0;}\n')
    exe = str(tmp_path / "ev")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    got = [int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    R, V = _abi.TdeEpisodeRecord, _abi.TdeEval
    assert got[0] == C.sizeof(R) == 48 == REC.itemsize and got[1:10] == [getattr(R, n).offset for n in rec]
    assert [REC.fields[n][1] for n in rec] == got[1:10]
    assert got[10] == C.sizeof(V) == 48 and got[11:18] == [getattr(V, n).offset for n in evn]
    assert got[18] == _abi.TDE_ABI_VERSION == 14
    # the three 16-byte words of a record: (ret, psi_sum) (speed_sum, length, reached) (scn, bits, padding)
    assert (R.psi_sum.offset, R.speed_sum.offset, R.length.offset, R.reached.offset, R.scn.offset, R.bits.offset) == (8, 16, 24, 28, 32, 36)


def _lib_and_args():
    from torchdriveenv_amd import _lib
    from torchdriveenv_amd.state import EnvState
    from torchdriveenv_amd.synth import synthetic_world

    L = _lib.load()
    assert {"tde_env_reset_to", "tde_eval_advance"} <= set(_lib.SYMBOLS) and len(_lib.SYMBOLS) == 31
    assert len(L.tde_env_reset_to.argtypes) == 6 and len(L.tde_eval_advance.argtypes) == 5 and L.tde_abi_version() == 14
    w = synthetic_world(n_scn=2, A=8, seed=0, n_maps=1)
    return L, w, EnvState(4, 8), _abi.default_config(seed=1, flags=FLAGS)


def test_reset_to_rejects_bad_arguments_without_a_launch():
    """tde_env_reset's rejections under the new name; every pointer here is a host pointer or NULL, so a check that let something
    through would be seen at once - the accepted calls are on an empty batch, which returns before any launch"""
    L, w, st, cfg = _lib_and_args()
    ws = w.host_struct()

    def refused(fragment, cfg_=cfg, ws_=ws, st_=None):
        st_ = st.struct if st_ is None else st_
        rc = L.tde_env_reset_to(None if cfg_ is None else C.byref(cfg_), None if ws_ is None else C.byref(ws_),
                                None if st_ is False else C.byref(st_), None, None, None)
        err = L.tde_last_error()
        assert rc != 0 and fragment in err and b"tde_env_reset_to:" in err, (fragment, rc, err)

    refused(b"NULL argument", cfg_=None)
    refused(b"NULL argument", ws_=None)
    refused(b"NULL argument", st_=False)
    bad_a = _abi.TdeState.from_buffer_copy(st.struct)
    bad_a.A = 6
    refused(b"power of two", st_=bad_a)
    other = _abi.TdeWorld.from_buffer_copy(ws)
    other.A = 16
    refused(b"world.A (16) != state.A (8)", ws_=other)
    refused(b"npc_max_steer", cfg_=_abi.default_config(seed=1, flags=FLAGS, npc_max_steer=-0.1))
    refused(b"npc_max_accel", cfg_=_abi.default_config(seed=1, flags=FLAGS, npc_max_accel=0.0))
    empty = _abi.TdeState.from_buffer_copy(st.struct)
    empty.B = 0
    scn = np.zeros(4, np.int32)
    assert L.tde_env_reset_to(C.byref(cfg), C.byref(ws), C.byref(empty), None, scn.ctypes.data, None) == 0
    assert L.tde_env_reset_to(C.byref(cfg), C.byref(ws), C.byref(empty), None, None, None) == 0


def test_eval_advance_rejects_bad_arguments_without_a_launch():
    L, w, st, cfg = _lib_and_args()
    ws = w.host_struct()
    plan, rnd, act = np.zeros((2, 4), np.int32), np.zeros(4, np.int32), np.ones(4, np.uint8)
    acc, res = np.zeros(4, REC), np.zeros((2, 4), REC)

    def ev(**over):
        e = _abi.TdeEval(plan.ctypes.data, rnd.ctypes.data, act.ctypes.data, acc.ctypes.data, res.ctypes.data, 2, 0)
        for k, v in over.items():
            setattr(e, k, v)
        return e

    def state(null=None, B=4):
        s = _abi.TdeState.from_buffer_copy(st.struct)
        s.B = B
        if null is not None:
            assert getattr(s, null) is not None
            setattr(s, null, None)
        return s

    def call(cfg_=cfg, ws_=ws, st_=None, ev_=None, null_ev=False):
        st_ = state() if st_ is None else st_
        e = ev() if ev_ is None else ev_
        return L.tde_eval_advance(None if cfg_ is None else C.byref(cfg_), None if ws_ is None else C.byref(ws_),
                                  None if st_ is False else C.byref(st_), None if null_ev else C.byref(e), None)

    def refused(fragment, **kw):
        rc, err = call(**kw), L.tde_last_error()
        assert rc != 0 and fragment in err and b"tde_eval_advance:" in err, (fragment, sorted(kw), rc, err)

    refused(b"NULL argument", cfg_=None)
    refused(b"NULL argument", ws_=None)
    refused(b"NULL argument", st_=False)
    refused(b"NULL argument", null_ev=True)
    for n in ("plan", "round", "active", "acc", "results"):
        refused(b"a NULL array in eval", ev_=ev(**{n: None}))
    for R in (0, -3):
        refused(b"eval.R must be >= 1", ev_=ev(R=R))
    for n in ("reward", "terminated", "truncated", "done_bits", "info", "info_reached", "steps", "scn"):
        refused(b"the state lacks", st_=state(n))
    refused(b"TDE_F_AUTORESET is set", cfg_=_abi.default_config(seed=1, flags=FLAGS | _abi.F_AUTORESET))
    bad_a = state()
    bad_a.A = 3
    refused(b"power of two", st_=bad_a)
    # an empty batch returns 0 before any launch; a pointer the entry point does not ask for may be NULL
    assert call(st_=state(B=0)) == 0, L.tde_last_error()
    for n in ("obs", "ep_return", "magnitudes", "tl_violation"):
        s = state(B=0)
        setattr(s, n, None)
        assert call(st_=s) == 0, (n, L.tde_last_error())
    # nothing was written by any of the calls above
    assert not rnd.any() and act.all() and not acc.view(np.uint8).any() and not res.view(np.uint8).any()


def test_scenario_option_validation_needs_no_gpu():
    import torch

    from torchdriveenv_amd import ops

    chk = ops.check_scenario_ids
    assert chk(2, 5, 4).tolist() == [2] * 5 and chk(-1, 3, 4).tolist() == [-1] * 3 and chk(np.int64(3), 2, 4).tolist() == [3, 3]
    assert chk([0, -1, 3], 3, 4).tolist() == [0, -1, 3] and chk((1, 2), 2, 4).dtype == torch.int32
    assert chk(torch.tensor([3, 0, -1, 1]), 4, 4).tolist() == [3, 0, -1, 1] and chk(torch.tensor(1, dtype=torch.int32), 3, 4).tolist() == [1, 1, 1]
    assert chk(np.array([1, 0], np.int16), 2, 2).tolist() == [1, 0]
    for bad, B in ((4, 3), (-2, 3), ([0, 1], 3), ([0, 1, 4], 3), ([0, -2, 1], 3), (1.5, 3), ([0.0, 1.0, 2.0], 3), (True, 3), ("1", 3),
                   (torch.tensor([0.0, 1.0, 2.0]), 3), (torch.tensor([True, False, True]), 3), (torch.zeros((2, 3), dtype=torch.int32), 3),
                   (None, 3), ([[0, 1, 2]], 4)):
        with pytest.raises(ValueError):
            chk(bad, B, 4)


def test_schedule_is_static_and_by_job_index():
    from torchdriveenv_amd.env import eval_plan

    plan, jobs = eval_plan(4, 3, None, 2)
    assert jobs.tolist() == [0, 1, 2, 3, 0, 1, 2, 3] and plan.dtype == np.int32
    assert plan.tolist() == [[0, 1, 2], [3, 0, 1], [2, 3, -1]]
    for j, s in enumerate(jobs):
        assert plan[j // 3, j % 3] == s
    plan, jobs = eval_plan(4, 8, [3, 1], 1)
    assert plan.tolist() == [[3, 1, -1, -1, -1, -1, -1, -1]] and jobs.tolist() == [3, 1]
    assert eval_plan(4, 1, [2, 2, 0], 1)[0].tolist() == [[2], [2], [0]]
    for kw in (dict(cases=[]), dict(cases=[4]), dict(cases=[-1]), dict(cases=[0.5]), dict(cases=[[0, 1]]), dict(repeats=0), dict(repeats=1.5)):
        with pytest.raises(ValueError):
            eval_plan(4, 3, **{"cases": None, "repeats": 1, **kw})


def test_metrics_arithmetic_on_hand_made_records():
    from torchdriveenv_amd.env import EvalResult

    rec = np.zeros(4, REC)
    rec["ret"] = [10.0, -2.5, 0.25, 4.0]
    rec["psi_sum"] = [1.0, 0.5, 0.0, 3.0]
    rec["speed_sum"] = [2.0, 2.0, 9.0, 0.0]
    rec["length"] = [4, 2, 3, 12]
    rec["reached"] = [1, 0, 0, 5]
    rec["scn"] = [0, 1, 2, 3]
    rec["bits"] = [1 | 4, 1 | 8 | 16, 1 | 4 | 8, 2]
    res = EvalResult.from_records(rec, jobs=[0, 1, 2, 3])
    assert len(res) == 4 and res.scenario.tolist() == [0, 1, 2, 3] and res.bits.tolist() == rec["bits"].tolist()
    assert res.psi_smoothness.tolist() == [0.25, 0.25, 0.0, 0.25] and res.speed_smoothness.tolist() == [0.5, 1.0, 3.0, 0.0]
    m = res.metrics()
    assert list(m) == ["mean_episode_reward", "mean_episode_length", "offroad_rate", "collision_rate", "traffic_light_violation_rate",
                       "success_percentage", "reached_waypoint_num", "psi_smoothness", "speed_smoothness"]
    assert m == {"mean_episode_reward": 11.75 / 4, "mean_episode_length": 21 / 4, "offroad_rate": 0.5, "collision_rate": 0.5,
                 "traffic_light_violation_rate": 0.25, "success_percentage": 0.25, "reached_waypoint_num": 1.5, "psi_smoothness": 0.75 / 4,
                 "speed_smoothness": 4.5 / 4}
    with pytest.raises(RuntimeError):
        EvalResult.from_records(rec, jobs=[0, 1, 2, 2])
    with pytest.raises(ValueError):
        EvalResult.from_records(rec[:0]).metrics()


def test_single_scenario_world_reset_is_the_drawn_reset_with_another_scenario_id(world4):
    """the restatement's premise, on the oracle alone: an env whose draw in the whole world is scenario s gets, from the oracle's
    reset on the single-scenario world of s, the very same bytes in every state array but scn (0 there)"""
    from oracle import oracle
    from torchdriveenv_amd.state import EnvState

    cfg = _abi.default_config(seed=0x1234567, flags=FLAGS | _abi.F_EGO_ONLY_ATTRS)
    B, A = 64, world4.A
    full = EnvState(B, A)
    oracle.env_reset(cfg, world4, full)
    drawn = full["scn"].copy()
    assert set(drawn.tolist()) == {0, 1, 2, 3}
    for s, ws in enumerate(E.singles_of(world4)):
        assert ws.n_scn == 1 and ws.arrays["route_xy"].shape == world4.arrays["route_xy"].shape
        one = EnvState(B, A)
        oracle.env_reset(cfg, ws, one)
        assert not one["scn"].any()
        m = drawn == s
        for k, a in full.host().items():
            if k in ("scn", "action"):
                continue
            b = one.host()[k]
            rows = np.repeat(m, A) if len(a) == B * A else m
            assert np.array_equal(a[rows].view(np.uint8), b[rows].view(np.uint8)), (s, k)
    # and reset_to with every id -1 is the plain reset
    again = EnvState(B, A)
    E.reset_to(cfg, world4, again, np.full(B, -1), None)
    assert all(np.array_equal(v.view(np.uint8), again.host()[k].view(np.uint8)) for k, v in full.host().items())


def _scripted(t, hs):
    """actions that depend on the episode's own clock alone: steady at first, a hard steer from step 4 in odd scenarios"""
    a = np.zeros((hs.B, 2), np.float32)
    a[:, 0] = 0.5
    a[:, 1] = np.where((hs["scn"] % 2 == 1) & (hs["steps"] >= 4), np.float32(0.3), np.float32(0.0))
    return a


def test_reference_evaluation_of_a_three_case_suite_at_one_and_three_envs(world4):
    """the schedule does not depend on the batch: with one env or three, every job is recorded exactly once, in job order, under its
    own scenario, and nothing else is written.  The records' VALUES are equal only where the episode's random key (env index, episode
    counter) coincides - here job 0 (env 0, episode 0 either way): the start point, speed and heading noise of an episode are drawn
    from that key, so job 1 as env 0's second episode is another episode than job 1 as env 1's first; that job is compared byte for
    byte, the others by what the schedule alone fixes."""
    cfg = _abi.default_config(seed=21, flags=FLAGS, max_steps=12)
    cases = [2, 1, 3]
    singles = E.singles_of(world4)
    out = {}
    for B in (1, 3):
        from torchdriveenv_amd.env import eval_plan

        plan, jobs = eval_plan(world4.n_scn, B, cases, 1)
        seen = []
        ev, hs, T = E.run(cfg, world4, B, plan, _scripted, singles=singles,
                          on_step=lambda t, hs, ev, re: seen.append((int(ev["round"].sum()), int(ev["active"].sum()))))
        rec = E.jobs_of(ev, len(jobs))
        assert rec["scn"].tolist() == cases and (rec["length"] >= 1).all() and (rec["length"] <= 12).all()
        assert ((rec["bits"] & 3) != 0).all() and not rec["_pad0"].any() and not rec["_pad1"].any()
        assert ev["round"].tolist() == [len(jobs) // B] * B and not ev["active"].any() and not ev["acc"].view(np.uint8).any()
        assert [r for r, _ in seen] == sorted(r for r, _ in seen) and seen[-1] == (3, 0)
        assert T == (int(rec["length"].sum()) if B == 1 else int(rec["length"].max()))
        out[B] = rec.copy()
    assert out[1][0].tobytes() == out[3][0].tobytes()
    assert out[1]["scn"].tolist() == out[3]["scn"].tolist()
    assert (out[1]["bits"] & 2).any() or (out[3]["bits"] & 2).any()          # some episode runs to max_steps ...
    assert (out[1]["bits"] & 4).any() or (out[3]["bits"] & 4).any()          # ... and the hard steer ends another off the road
