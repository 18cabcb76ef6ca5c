"""CPU checks of the terminal pool beside the replay ring (include/tde_terminal.h, torchdriveenv_amd/replay.py, onpolicy.py, env.py): the
numpy restatement (tests/terminal_ref.py) against hand-made cases, the header's constants and struct (the header beside the others, its
symbols and the loader's refusals: tests/test_abi_families_cpu.py), and every host-side rejection of the entry points, of the ops wrappers and of the Python arguments (all before any launch: no GPU needed)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from tests import terminal_ref as T
from tests.test_abi_families_cpu import c_status
from tests.test_replay_cpu import BAD_STRUCTS, _Host
from torchdriveenv_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT, HAS = _abi.REPLAY_CUT, _abi.TERMINAL_HAS


# ---- the restatement's own properties -----------------------------------------------------------------------------------------------
def test_rank_rule_on_a_hand_made_mask():
    #            env:  0  1  2  3  4       5  6   7
    db = np.array([0, 1, 4, 2, 8 | 16, 3, 0, 2 | 4], np.uint8)     # bits 2-4 alone finish nothing
    assert T.ranks(db, 8).tolist() == [-1, 0, -1, 1, -1, 2, -1, 3]
    assert T.ranks(db, 4).tolist() == [-1, 0, -1, 1, -1, 2, -1, 3]
    assert T.ranks(np.zeros(5, np.uint8), 2).tolist() == [-1] * 5
    assert T.ranks(np.full(5, 2, np.uint8), 5).tolist() == [0, 1, 2, 3, 4]


def test_overflow_keeps_the_first_m():
    db = np.array([0, 1, 4, 2, 8, 3, 0, 2], np.uint8)
    assert T.ranks(db, 2).tolist() == [-1, 0, -1, 1, -1, -1, -1, -1]
    assert T.ranks(db, 1).tolist() == [-1, 0, -1, -1, -1, -1, -1, -1]
    ring = T.TerminalRing(4, 8, 2, D=3)
    rows = lambda k: np.arange(24, dtype=np.float32).reshape(8, 3) + 100 * k
    ring.begin(rows(0))
    ring.push(np.zeros((8, 2), np.float32), np.zeros(8, np.float32), db, rows(1), rows(9))
    assert ring.ref[0].tolist() == [-1, 0, -1, 1, -1, -1, -1, -1]
    assert np.array_equal(ring.pool[0], rows(9)[[1, 3]]) and not ring.pool[1:].any()
    g = ring.gather([(0, 1), (0, 3), (0, 5), (0, 7), (0, 0)])
    assert g["dones"].tolist() == [1 | HAS, 2 | HAS, 3, 2, 0]           # envs 5 and 7 overflowed: as without a pool
    assert np.array_equal(g["next_observations"][:2], rows(9)[[1, 3]]) and not g["next_observations"][2:4].any()
    assert np.array_equal(g["next_observations"][4], rows(1)[0])        # a step that did not end: the next slot's row
    assert T.bootstrap_mask(g["dones"]).tolist() == [False, True, False, False, True]


def test_an_overwritten_slot_loses_its_refs():
    ring = T.TerminalRing(4, 2, 2, D=1)
    z2, z, none = np.zeros((2, 2), np.float32), np.zeros(2, np.float32), np.zeros(2, np.uint8)
    row = lambda k: np.full((2, 1), k, np.float32)
    ring.begin(row(0))
    ring.push(z2, z, np.array([2, 0], np.uint8), row(1), row(10))       # slot 0: env 0 ends
    ring.push(z2, z, np.array([0, 1], np.uint8), row(2), row(20))       # slot 1: env 1 ends
    ring.push(z2, z, none, row(3), row(30))                             # slot 2
    assert ring.ref.tolist() == [[0, -1], [-1, 0], [-1, -1], [-1, -1]]
    g = ring.gather([(0, 0), (1, 1), (0, 1)])
    assert g["dones"].tolist() == [2 | HAS, 1 | HAS, 0] and g["next_observations"][:, 0].tolist() == [10.0, 20.0, 1.0]
    ring.push(z2, z, none, row(4), row(40))                             # slot 3; the ring is full, slot 0 is the open one
    assert (ring.first, ring.w, ring.count) == (1, 0, 3) and ring.ref[0].tolist() == [0, -1]
    g = ring.gather([(0, 0), (1, 1)])                                   # an open slot is no stored transition, whatever its refs say
    assert g["dones"].tolist() == [0, 1 | HAS] and g["next_observations"][:, 0].tolist() == [0.0, 20.0]
    ring.push(z2, z, none, row(5), row(50))                             # slot 0 again: every ref of the slot is rewritten
    assert (ring.first, ring.w, ring.count) == (2, 1, 3) and ring.ref.tolist() == [[-1, -1], [-1, 0], [-1, -1], [-1, -1]]
    assert ring.pool[0, 0, 0] == 10                                     # (pool rows at or above the number kept are not written)
    g = ring.gather([(0, 0), (1, 1)])
    assert g["dones"].tolist() == [0, 0] and g["next_observations"][:, 0].tolist() == [5.0, 0.0]


def test_a_transition_that_is_cut_and_ended_keeps_its_frame():
    P = 16
    ring = T.TerminalRing(5, 2, 1, n_stack=3, plane=P)
    frame = lambda k: np.full((2, P), k, np.uint8)
    z2, z = np.zeros((2, 2), np.float32), np.zeros(2, np.float32)
    ring.begin(frame(0))
    ring.push(z2, z, np.zeros(2, np.uint8), frame(1), frame(7))
    ring.push(z2, z, np.array([2, 0], np.uint8), frame(2), frame(3))    # slot 1: env 0 is truncated, its terminal frame is layer 3
    ring.begin(frame(4), mask=np.array([1, 1], np.uint8))               # the caller resets both envs right after
    assert ring.done[1].tolist() == [2 | CUT, CUT]
    g = ring.gather([(1, 0), (1, 1)])
    assert g["dones"].tolist() == [2 | CUT | HAS, CUT]
    nxt, obs = g["next_observations"].reshape(2, 3, 3, P), g["observations"].reshape(2, 3, 3, P)
    assert np.array_equal(nxt[0, :2], obs[0, 1:]) and (nxt[0, 2] == np.array(_abi.PALETTE[3], np.uint8)[:, None]).all()
    assert not obs[0, 0].any() and obs[0, 1].any()                      # age 1 at slot 1: the oldest frame is blank, and stays blank one down
    assert not nxt[1].any()                                             # only cut: zeros, no HAS
    assert T.bootstrap_mask(g["dones"]).tolist() == [True, False]       # truncated with its frame: bootstrapped, cut or not


# ---- header, symbols, constants -----------------------------------------------------------------------------------------------------
def test_constants_and_struct_match_header(tmp_path):
    assert c_status(tmp_path, ["tde_terminal.h"], "(TDE_TERMINAL_HAS & (TDE_REPLAY_CUT | 31)) | (sizeof(tde_terminal) != 24)") == 0
    text = open(os.path.join(ROOT, "include", "tde_terminal.h")).read()
    assert int(re.search(r"#define TDE_TERMINAL_HAS (0x[0-9a-fA-F]+)", text).group(1), 16) == _abi.TERMINAL_HAS == 0x40
    assert not _abi.TERMINAL_HAS & (_abi.REPLAY_CUT | 31)               # free beside done_bits (bits 0-4) and the cut bit
    assert [f[0] for f in _abi.TdeTerminal._fields_] == ["M", "pool", "ref"] and C.sizeof(_abi.TdeTerminal) == 24
    assert _abi.TdeTerminal.pool.offset == 8 and _abi.TdeTerminal.ref.offset == 16


# ---- every host-side refusal, before any launch -------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments_without_a_launch():
    from torchdriveenv_amd import _lib

    L = _lib.load()
    h = _Host()                                             # C = 6, B = 3, n_stack = 3, plane = 64
    M = 2
    pool, ref = np.zeros((6, M, 64), np.uint8), np.zeros((6, 3), np.int32)
    db, term = np.zeros(3, np.uint8), np.zeros((3, 64), np.uint8)
    idx, obs, nxt = np.zeros((4, 2), np.int32), np.zeros((4, 9, 64), np.uint8), np.zeros((4, 9, 64), np.uint8)
    oa, orw, od = np.zeros((4, 2), np.float32), np.zeros(4, np.float32), np.zeros(4, np.uint8)
    dst = np.zeros((3, 64), np.uint8)
    ptr = lambda a: a.ctypes.data

    def tm(**over):
        a = {**dict(M=M, pool=ptr(pool), ref=ptr(ref)), **over}
        return _abi.TdeTerminal(a["M"], a["pool"], a["ref"])

    def push(rp=None, t=None, w=0, d=ptr(db), src=ptr(term), stride=64, null_rp=False, null_tm=False):
        return L.tde_terminal_push(None if null_rp else C.byref(rp or h.rp()), None if null_tm else C.byref(t or tm()), w, d, src, stride, None)

    def sample(rp=None, t=None, first=0, count=4, N=4, idx_in=None, out=None, null_rp=False, null_tm=False):
        o = {**dict(idx=ptr(idx), obs=ptr(obs), next_obs=ptr(nxt), action=ptr(oa), reward=ptr(orw), done=ptr(od)), **(out or {})}
        return L.tde_terminal_sample(None if null_rp else C.byref(rp or h.rp()), None if null_tm else C.byref(t or tm()), first, count, N,
                                     idx_in, 1, 0, o["idx"], o["obs"], o["next_obs"], o["action"], o["reward"], o["done"], None)

    def stash(B=3, row=64, d=ptr(db), src=ptr(term), stride=64, to=ptr(dst)):
        return L.tde_terminal_stash(B, row, d, src, stride, to, None)

    names = {push: b"tde_terminal_push: ", sample: b"tde_terminal_sample: ", stash: b"tde_terminal_stash: "}

    def refused(fn, fragment, **kw):
        rc, err = fn(**kw), L.tde_last_error()
        assert rc != 0 and fragment in err and err.startswith(names[fn]), (fn.__name__, fragment, sorted(kw), rc, err)

    for fn in (push, sample):
        refused(fn, b"NULL argument", null_rp=True)
        refused(fn, b"NULL argument", null_tm=True)
        for over, fragment in BAD_STRUCTS:                  # the ring's own rules, as every replay entry point states them
            refused(fn, fragment, rp=h.rp(**over))
        refused(fn, b"16-byte aligned", rp=h.rp(frames=h.frames.ctypes.data + 4))
        for bad_m in (0, -1, 4):
            refused(fn, b"M must be in [1, B]", t=tm(M=bad_m))
        refused(fn, b"a NULL array in the terminal pool", t=tm(pool=None))
        refused(fn, b"a NULL array in the terminal pool", t=tm(ref=None))
        refused(fn, b"pool must be 16-byte aligned", t=tm(pool=ptr(pool) + 8))
        refused(fn, b"ref 4-byte", t=tm(ref=ptr(ref) + 2))
    for w in (-1, 6):
        refused(push, b"w must be in [0, C)", w=w)
    refused(push, b"NULL argument", d=None)
    refused(push, b"term_src is NULL", src=None)
    refused(push, b"term_stride is smaller", stride=48)
    refused(push, b"multiples of 16", stride=64 + 8)
    refused(push, b"multiples of 16", src=ptr(term) + 4)
    for N in (0, -2):
        refused(sample, b"N must be >= 1", N=N)
    for count in (0, -1):
        refused(sample, b"count must be >= 1", count=count)
    refused(sample, b"count must be <= C - 1", count=6)
    for first in (-1, 6):
        refused(sample, b"first must be in [0, C)", first=first)
    for name in ("idx", "obs", "next_obs", "action", "reward", "done"):
        refused(sample, b"a NULL output", out={name: None})
    for count in (1, 2):
        refused(sample, b"count must be > n_stack - 1", count=count)
    refused(sample, b"16-byte aligned", out={"obs": ptr(obs) + 8})
    refused(sample, b"16-byte aligned", out={"next_obs": ptr(nxt) + 8})
    refused(sample, b"action 8-byte", out={"action": ptr(oa) + 4})
    # rows mode: the pool needs 4-byte alignment only, and gets it checked
    hr = _Host(n_stack=1, plane=0, D=5)
    rpool = np.zeros((6, M, 5), np.float32)
    refused(push, b"(rows mode: 4)", rp=hr.rp(), t=tm(pool=ptr(rpool) + 2), stride=20)
    refused(push, b"term_stride is smaller", rp=hr.rp(), t=tm(pool=ptr(rpool)), stride=16)
    refused(push, b"(rows mode: 4)", rp=hr.rp(), t=tm(pool=ptr(rpool)), stride=22)
    for B in (0, -1):
        refused(stash, b"B must be >= 1", B=B)
    for row in (0, -4, 6):
        refused(stash, b"row_bytes must be a positive multiple of 4", row=row)
    for name in ("d", "src", "to"):
        refused(stash, b"NULL argument", **{name: None})
    refused(stash, b"src_stride is smaller", stride=32)
    refused(stash, b"multiples of 16", stride=72)
    refused(stash, b"multiples of 16", src=ptr(term) + 4)
    refused(stash, b"multiples of 16", to=ptr(dst) + 8)
    refused(stash, b"multiples of 16", row=20, stride=22)
    # nothing was written by any of the calls above
    for a in (h.frames, h.action, h.reward, h.done, h.age, pool, ref, rpool, dst, idx, obs, nxt, oa, orw, od):
        assert not a.view(np.uint8).any()


def test_ops_wrappers_reject_host_tensors_and_bad_shapes():
    import torch

    from torchdriveenv_amd import ops

    z = torch.zeros
    rp = _abi.TdeReplay(6, 4, 3, 64, 0, None, None, None, None, None)
    for M in (0, 5):
        with pytest.raises(ValueError, match=r"M must be in \[1, B = 4\]"):
            ops.terminal_struct(rp, M, z((6, 1, 64), dtype=torch.uint8), z((6, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="pool must be torch.uint8"):
        ops.terminal_struct(rp, 2, z((6, 2, 64)), z((6, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="pool must live on a HIP device"):
        ops.terminal_struct(rp, 2, z((6, 2, 64), dtype=torch.uint8), z((6, 4), dtype=torch.int32))
    tm = _abi.TdeTerminal(2, None, None)
    with pytest.raises(ValueError, match="done_bits must live on a HIP device"):
        ops.terminal_push(rp, tm, "cuda:0", 0, z(4, dtype=torch.uint8), z((4, 64), dtype=torch.uint8))
    with pytest.raises(ValueError, match="done_bits must be torch.uint8"):
        ops.terminal_push(rp, tm, "cuda:0", 0, z(4), z((4, 64), dtype=torch.uint8))
    with pytest.raises(ValueError, match="done_bits must live on a HIP device"):
        ops.terminal_stash("cuda:0", z(4, dtype=torch.uint8), z((4, 64), dtype=torch.uint8), 0, 64, z((4, 64), dtype=torch.uint8))
    with pytest.raises(ValueError, match="scratch must live on a HIP device"):
        ops.replay_pack_struct(4, 64, z(64, dtype=torch.uint8))
    with pytest.raises(ValueError, match="scratch must be torch.uint8"):
        ops.replay_pack_struct(4, 64, z(64))
    with pytest.raises(ValueError, match="n must be >= 1"):
        ops.terminal_sample(rp, tm, "cuda:0", 0, 4, 0, {})
    with pytest.raises(ValueError, match="observations must live on a HIP device"):
        ops.terminal_sample(rp, tm, "cuda:0", 0, 4, 2, {"observations": z((2, 9, 64), dtype=torch.uint8),
                                                      "next_observations": z((2, 9, 64), dtype=torch.uint8)})


def _fake_env(**over):
    kw = dict(auto_reset=True, state={"done_bits": object()}, num_envs=4, torch_device="cuda:0", obs_mode="birdview", frame_stack=3, _res=64)
    kw.update(over)
    from torchdriveenv_amd.config import EnvConfig, RendererConfig, SimulatorConfig
    from torchdriveenv_amd.observe import make_observer

    env = type("FakeEnv", (types.SimpleNamespace,), {})(config=EnvConfig(simulator=SimulatorConfig(renderer=RendererConfig(res=kw["_res"]))), **kw)
    env.observer = make_observer(env)                    # (the observers of birdview and state touch no device when they are made)
    return env


def test_python_arguments_are_refused_without_a_gpu():
    import inspect

    import torch

    from torchdriveenv_amd.config import EnvConfig
    from torchdriveenv_amd.env import BatchedWaypointEnv
    from torchdriveenv_amd.onpolicy import RolloutBuffer
    from torchdriveenv_amd.replay import ReplayBuffer, ReplaySamples

    # the option's own requirements come before the env touches a device
    for kw in (dict(auto_reset=False), dict(with_info=False)):
        with pytest.raises(ValueError, match="terminal_obs=True needs auto_reset=True and with_info=True"):
            BatchedWaypointEnv(EnvConfig(seed=1), None, num_envs=2, terminal_obs=True, **kw)
    with pytest.raises(ValueError, match="terminal_obs=True with near_field"):
        BatchedWaypointEnv(EnvConfig(seed=1), None, num_envs=2, terminal_obs=True, near_field={})
    assert inspect.signature(BatchedWaypointEnv.__init__).parameters["terminal_obs"].default is False
    assert inspect.signature(BatchedWaypointEnv.replay_buffer).parameters["terminal_per_step"].default is None
    assert inspect.signature(BatchedWaypointEnv.rollout_buffer).parameters["terminal_per_step"].default is None
    # on an env without the option terminal_per_step must be None
    with pytest.raises(ValueError, match="terminal_per_step needs an env built with terminal_obs=True"):
        ReplayBuffer(_fake_env(), 8, terminal_per_step=2)
    with pytest.raises(ValueError, match="terminal_per_step needs an env built with terminal_obs=True"):
        RolloutBuffer(_fake_env(terminal_obs=False), 8, terminal_per_step=1)
    for m in (0, 5, -1):
        with pytest.raises(ValueError, match=r"terminal_per_step must be in \[1, num_envs = 4\]"):
            ReplayBuffer(_fake_env(terminal_obs=True), 8, terminal_per_step=m)
    # a rollout env refuses on such an env; terminal_observations() refuses without the option
    env = BatchedWaypointEnv.__new__(BatchedWaypointEnv)
    env.terminal_obs = True
    with pytest.raises(ValueError, match=r"rollout\(\) on a terminal_obs env"):
        env.rollout(None)
    rb = RolloutBuffer.__new__(RolloutBuffer)
    rb.ring = types.SimpleNamespace(tstruct=None)
    with pytest.raises(ValueError, match="needs an env built with terminal_obs=True"):
        rb.terminal_observations()
    rb.ring, rb.pos, rb.finished = types.SimpleNamespace(tstruct=object()), 0, False
    with pytest.raises(ValueError, match=r"follows a push\(\)"):
        rb.terminal_observations()
    with pytest.raises(ValueError, match=r"follows a push\(\)"):
        rb.bootstrap(torch.zeros(0, dtype=torch.int64), torch.zeros(0))
    # .bootstrap and .terminal of a sample, on host tensors: every done byte against the restatement
    d = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    s = ReplaySamples(None, None, None, d, None, None)
    assert np.array_equal(s.bootstrap.numpy(), T.bootstrap_mask(d.numpy()))
    assert np.array_equal(s.terminal.numpy(), (d.numpy() & (3 | CUT)) != 0)
    assert s.bootstrap[0] and not s.bootstrap[2] and s.bootstrap[2 | HAS] and not s.bootstrap[1 | HAS] and not s.bootstrap[3 | HAS]
    assert s.bootstrap[2 | HAS | CUT] and not s.bootstrap[CUT] and not s.bootstrap[2 | CUT] and s.bootstrap[4 | 8 | 16]
