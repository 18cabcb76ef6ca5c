"""CPU checks of the replay buffer (include/tde_replay.h, torchdriveenv_amd/replay.py): the struct and constants against the header
(the header beside the others, its symbols and the loader's refusals: tests/test_abi_families_cpu.py), every host-side rejection of the entry points, of the ops wrappers and of ReplayBuffer's arguments
(all before any launch: no GPU needed), and the numpy restatement (tests/replay_ref.py) against a hand-written known answer."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

from tests import replay_ref as R
from torchdriveenv_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("C", "B", "n_stack", "plane", "D", "frames", "action", "reward", "done", "age")


def test_struct_and_constants_match_header(tmp_path):
    c = tmp_path / "rp.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tde_replay.h"\nint main(void){printf("%zu", sizeof(tde_replay));' +
                 "".join(f'printf(" %zu", offsetof(tde_replay, {n}));' for n in FIELDS) +
                 'printf(" %d %d %u %d %d %d %d\\n", TDE_REPLAY_VERSION, TDE_REPLAY_CUT, TDE_REPLAY_TAG, TDE_ABI_VERSION, TDE_REPLAY_MAX_STACK,'
                 ' TDE_REPLAY_MAX_PLANE, (int)(sizeof(&tde_replay_begin) + sizeof(&tde_replay_push) + sizeof(&tde_replay_sample) + sizeof(&tde_replay_pack)));'
                 ' return 0;}\n')
    exe = str(tmp_path / "rp")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    got = [int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    S = _abi.TdeReplay
    assert got[0] == C.sizeof(S) == 64 and got[1:11] == [getattr(S, n).offset for n in FIELDS] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56]
    assert got[11:17] == [_abi.TDE_REPLAY_VERSION, _abi.REPLAY_CUT, _abi.REPLAY_TAG, _abi.TDE_ABI_VERSION, _abi.REPLAY_MAX_STACK, _abi.REPLAY_MAX_PLANE]
    assert got[11:17] == [1, 0x80, 0x5250, 14, 8, 4096]


def _loaded():
    from torchdriveenv_amd import _lib

    return _lib, _lib.load()


class _Host:
    """a ring in host memory: every entry point must refuse before it launches, so nothing here is ever dereferenced"""

    def __init__(self, C_=6, B=3, n_stack=3, plane=64, D=0):
        self.frames = np.zeros((C_, B, plane if plane else D), np.uint8 if plane else np.float32)
        self.action, self.reward = np.zeros((C_, B, 2), np.float32), np.zeros((C_, B), np.float32)
        self.done, self.age = np.zeros((C_, B), np.uint8), np.zeros((C_, B), np.uint8)
        self.args = dict(C=C_, B=B, n_stack=n_stack, plane=plane, D=D, frames=self.frames.ctypes.data, action=self.action.ctypes.data,
                         reward=self.reward.ctypes.data, done=self.done.ctypes.data, age=self.age.ctypes.data)
        self.src = np.zeros((B, n_stack, max(plane, 4 * D)), np.uint8)

    def rp(self, **over):
        a = {**self.args, **over}
        return _abi.TdeReplay(*[a[n] for n in FIELDS])


BAD_STRUCTS = [(dict(B=0), b"B must be >= 1"), (dict(plane=0), b"exactly one of plane"), (dict(D=4), b"exactly one of plane"),
               (dict(n_stack=0), b"n_stack must be in [1, 8]"), (dict(n_stack=9, C=12), b"n_stack must be in [1, 8]"),
               (dict(plane=72), b"multiple of 16"), (dict(plane=8192), b"at most 4096"), (dict(C=1), b"C must be >= 2"),
               (dict(C=3), b">= n_stack + 1"), (dict(plane=0, D=8, n_stack=2), b"n_stack must be 1 in rows mode"),
               (dict(frames=None), b"a NULL array"), (dict(action=None), b"a NULL array"), (dict(reward=None), b"a NULL array"),
               (dict(done=None), b"a NULL array"), (dict(age=None), b"a NULL array")]


def test_entry_points_reject_bad_arguments_without_a_launch():
    _, L = _loaded()
    h = _Host()
    src, stride = h.src.ctypes.data, 3 * 64
    act, rew, db = np.zeros((3, 2), np.float32), np.zeros(3, np.float32), np.zeros(3, np.uint8)
    idx, obs, nxt = np.zeros((4, 2), np.int32), np.zeros((4, 9, 64), np.uint8), np.zeros((4, 9, 64), np.uint8)
    oa, orw, od = np.zeros((4, 2), np.float32), np.zeros(4, np.float32), np.zeros(4, np.uint8)
    rgb, planes = np.zeros((3, 3, 64), np.uint8), np.zeros((3, 64), np.uint8)

    def begin(rp=None, w=0, src_=src, stride_=stride, null_rp=False):
        return L.tde_replay_begin(None if null_rp else C.byref(rp or h.rp()), w, src_, stride_, None, None)

    def push(rp=None, w=0, a=act.ctypes.data, r=rew.ctypes.data, d=db.ctypes.data, src_=src, stride_=stride, null_rp=False):
        return L.tde_replay_push(None if null_rp else C.byref(rp or h.rp()), w, a, r, d, src_, stride_, None)

    def sample(rp=None, first=0, count=4, N=4, idx_in=None, out=None, null_rp=False):
        o = {**dict(idx=idx.ctypes.data, obs=obs.ctypes.data, next_obs=nxt.ctypes.data, action=oa.ctypes.data, reward=orw.ctypes.data,
                    done=od.ctypes.data), **(out or {})}
        return L.tde_replay_sample(None if null_rp else C.byref(rp or h.rp()), first, count, N, idx_in, 1, 0, o["idx"], o["obs"], o["next_obs"],
                                   o["action"], o["reward"], o["done"], None)

    def pack(rp=None, rgb_=rgb.ctypes.data, rs=3 * 64, pl=planes.ctypes.data, ps=64, null_rp=False):
        return L.tde_replay_pack(None if null_rp else C.byref(rp or h.rp()), rgb_, rs, pl, ps, None)

    def refused(fn, fragment, **kw):
        rc, err = fn(**kw), L.tde_last_error()
        assert rc != 0 and fragment in err and fn.__name__.encode() in err and b"tde_replay_" in err, (fn.__name__, fragment, sorted(kw), rc, err)

    for fn in (begin, push, sample, pack):
        refused(fn, b"NULL argument", null_rp=True)
        for over, fragment in BAD_STRUCTS:
            refused(fn, fragment, rp=h.rp(**over))
        refused(fn, b"16-byte aligned", rp=h.rp(frames=h.frames.ctypes.data + 4))
    for fn in (begin, push):
        for w in (-1, 6):
            refused(fn, b"w must be in [0, C)", w=w)
        refused(fn, b"src is NULL", src_=None)
        refused(fn, b"src_stride is smaller", stride_=48)
        refused(fn, b"multiples of 16", stride_=3 * 64 + 8)
        refused(fn, b"multiples of 16", src_=src + 4)
    for name in ("a", "r", "d"):
        refused(push, b"NULL argument", **{name: None})
    refused(push, b"8-byte aligned", a=act.ctypes.data + 4)
    for N in (0, -2):
        refused(sample, b"N must be >= 1", N=N)
    for count in (0, -1):
        refused(sample, b"count must be >= 1", count=count)
    refused(sample, b"count must be <= C - 1", count=6)
    for first in (-1, 6):
        refused(sample, b"first must be in [0, C)", first=first)
    for name in ("idx", "obs", "next_obs", "action", "reward", "done"):
        refused(sample, b"a NULL output", out={name: None})
    for count in (1, 2):                  # n_stack = 3: nothing to draw from until more than two steps are stored ...
        refused(sample, b"count must be > n_stack - 1", count=count)
    refused(sample, b"16-byte aligned", out={"obs": obs.ctypes.data + 8})
    refused(pack, b"NULL argument", rgb_=None)
    refused(pack, b"NULL argument", pl=None)
    refused(pack, b"a stride is smaller", rs=64)
    refused(pack, b"a stride is smaller", ps=32)
    refused(pack, b"multiples of 16", ps=72)
    hr = _Host(n_stack=1, plane=0, D=5)
    refused(pack, b"planes mode only", rp=hr.rp())
    refused(begin, b"multiples of 16 (rows mode: 4)", rp=hr.rp(), stride_=22)
    refused(begin, b"src_stride is smaller", rp=hr.rp(), stride_=16)
    # nothing was written by any of the calls above
    for a in (h.frames, h.action, h.reward, h.done, h.age, idx, obs, nxt, oa, orw, od, planes):
        assert not a.view(np.uint8).any()


def test_ops_wrappers_reject_host_tensors_and_bad_shapes():
    import torch

    from torchdriveenv_amd import ops

    z = torch.zeros
    ring = dict(frames=z((4, 2, 64), dtype=torch.uint8), action=z((4, 2, 2)), reward=z((4, 2)), done=z((4, 2), dtype=torch.uint8),
                age=z((4, 2), dtype=torch.uint8))
    with pytest.raises(ValueError, match="HIP device"):
        ops.replay_struct(4, 2, 3, 64, 0, **ring)
    with pytest.raises(ValueError, match="exactly one of plane"):
        ops.replay_struct(4, 2, 3, 64, 8, **ring)
    with pytest.raises(ValueError, match="frames must be torch.uint8"):
        ops.replay_struct(4, 2, 3, 64, 0, **{**ring, "frames": z((4, 2, 64))})
    rp = _abi.TdeReplay(4, 2, 3, 64, 0, None, None, None, None, None)
    with pytest.raises(ValueError, match="src must live on a HIP device"):
        ops.replay_begin(rp, "cuda:0", 0, z((2, 3, 64), dtype=torch.uint8))
    with pytest.raises(ValueError, match="src must be torch.uint8"):
        ops.replay_push(rp, "cuda:0", 0, z((2, 2)), z(2), z(2, dtype=torch.uint8), z((2, 3, 64)))
    with pytest.raises(ValueError, match="n must be >= 1"):
        ops.replay_sample(rp, "cuda:0", 0, 1, 0, {})
    with pytest.raises(ValueError, match="observations must live on a HIP device"):
        ops.replay_sample(rp, "cuda:0", 0, 1, 2, {"observations": z((2, 9, 64), dtype=torch.uint8), "next_observations": None})
    with pytest.raises(ValueError, match="rgb must live on a HIP device"):
        ops.replay_pack(rp, "cuda:0", z((2, 3, 64), dtype=torch.uint8), z((2, 64), dtype=torch.uint8))


def _fake_env(**over):
    kw = dict(auto_reset=True, state={"done_bits": object()}, num_envs=4, torch_device="cuda:0", obs_mode="birdview", frame_stack=3, _res=64)
    kw.update(over)
    from torchdriveenv_amd.config import EnvConfig, RendererConfig, SimulatorConfig
    from torchdriveenv_amd.observe import make_observer

    env = type("FakeEnv", (types.SimpleNamespace,), {})(config=EnvConfig(simulator=SimulatorConfig(renderer=RendererConfig(res=kw["_res"]))), **kw)
    env.observer = make_observer(env)                    # (the observers of birdview and state touch no device when they are made)
    return env


def test_replay_buffer_argument_checks_need_no_gpu():
    from torchdriveenv_amd.replay import ReplayBuffer, ReplaySamples

    with pytest.raises(ValueError, match="auto_reset=True"):
        ReplayBuffer(_fake_env(auto_reset=False), 16)
    with pytest.raises(ValueError, match="with_info=True"):
        ReplayBuffer(_fake_env(state={"done_bits": None}), 16)
    for cap in (3, 1, 0, -4):
        with pytest.raises(ValueError, match=r"capacity_steps must be >= frame_stack \+ 1 = 4"):
            ReplayBuffer(_fake_env(), cap)
    with pytest.raises(ValueError, match=r"capacity_steps must be >= frame_stack \+ 1 = 2"):
        ReplayBuffer(_fake_env(obs_mode="state", frame_stack=1), 1)
    with pytest.raises(ValueError, match=r"H \* W = 36 must be a multiple of 16"):
        ReplayBuffer(_fake_env(_res=6), 16)
    with pytest.raises(ValueError, match=r"H \* W = 16384 exceeds 4096"):
        ReplayBuffer(_fake_env(_res=128), 16)
    assert ReplaySamples._fields == ("observations", "actions", "next_observations", "dones", "rewards", "indices")
    from torchdriveenv_amd.env import BatchedWaypointEnv

    assert callable(BatchedWaypointEnv.replay_buffer)


def _host_buffer(**over):
    """a buffer in host memory with the attributes the refusals read and nothing else: every refusal comes before the first device call"""
    import torch

    from torchdriveenv_amd.replay import ReplayBuffer

    buf = ReplayBuffer.__new__(ReplayBuffer)
    buf.dev, buf.C, buf.B, buf.n_stack, buf.first, buf.count, buf.draws = torch.device("cpu"), 6, 3, 3, 1, 4, 5
    buf.age = torch.tensor([[0] * 3, [0, 1, 2], [1, 2, 3], [2, 0, 4], [3, 1, 5], [4, 2, 6]], dtype=torch.uint8)
    for k, v in over.items():
        setattr(buf, k, v)
    return buf


def test_sample_refuses_what_sample_nstep_refuses():
    buf = _host_buffer()
    for n in (0, -1, None):
        with pytest.raises(ValueError, match="n must be >= 1"):
            buf.sample(n)
    with pytest.raises(ValueError, match=r"idx must hold 3 \(slot, env\) pairs"):
        buf.sample(3, idx=[(1, 0), (2, 0)])
    # slot 0 is the open slot's successor, (1, 2) lacks its older frames (age 2 at off 0), env 3 and slot 6 do not exist
    for bad in ((0, 0), (1, 2), (2, 2), (5, 0), (2, 3), (6, 0), (-1, 0), (2, -1)):
        with pytest.raises(ValueError, match=r"not stored transitions with their whole frame stack in the ring \(valid_pairs\(\)\)"):
            buf.sample(None, idx=[(1, 0), bad, (3, 1)])
    buf.count = 2
    with pytest.raises(ValueError, match=r"sample\(\) draws steps .* needs more than 2 stored steps, the buffer holds 2"):
        buf.sample(4)
    buf.count = 0
    with pytest.raises(ValueError, match="holds no transition yet"):
        buf.sample(4)
    assert buf.draws == 5                                   # a refused call draws nothing


def test_which_refusal_wins_when_a_call_is_bad_twice():
    from torchdriveenv_amd.config import Prioritized

    def message(call):
        with pytest.raises(ValueError) as err:
            call()
        return str(err.value)

    buf = _host_buffer()
    assert message(lambda: buf.sample_nstep(0, 0)) == "n_steps must be in [1, 64], got 0"
    assert message(lambda: buf.sample_sequence(0, 0)) == "length must be in [1, 256], got 0"
    assert message(lambda: buf.sample_prioritized(0, 0)) == "sample_prioritized() needs a buffer built with prioritized=Prioritized(...)"
    assert (message(lambda: buf.sample_sequence(4, 8, prioritized=True))
            == "sample_sequence(prioritized=True) needs a buffer built with prioritized=Prioritized(...)")
    assert message(lambda: buf.sample_sequence(4, 8, beta=0.5)) == "beta needs prioritized=True"
    buf = _host_buffer(pstruct=object(), prioritized=Prioritized())
    assert message(lambda: buf.sample_sequence(4, 8, idx=[(1, 0)] * 4, prioritized=True)) == "sample_sequence() takes idx or prioritized=True, not both"
    assert message(lambda: buf.sample_prioritized(4, 65, 2.0, 2.0)) == "n_steps must be in [1, 64], got 65"
    assert buf.draws == 5


# ---- the numpy restatement against a hand-written answer: two envs, five steps, env 0 ends its episode at the third step, n_stack 3 ----
WHITE, GREY, GREEN, BLUE, RED, BLACK = (255, 255, 255), (128, 128, 128), (44, 160, 44), (31, 119, 180), (214, 39, 40), (0, 0, 0)
P = 16


def _obs(*colours):
    """uint8 [9, P]: three frames, oldest first, each of one colour"""
    return np.concatenate([np.full((P, 3), c, np.uint8).T for c in colours])


def _five_steps():
    codes = np.array([[0, 1], [1, 2], [2, 3], [3, 4], [4, 0], [1, 2]], np.uint8)           # layer code of frame t of env e
    done = np.array([[0, 0], [0, 0], [1 | 4, 0], [0, 0], [0, 8]], np.uint8)                # env 0: terminated off the road at step 2
    ring = R.Ring(8, 2, n_stack=3, plane=P)
    frame = lambda t: np.repeat(codes[t][:, None], P, 1)
    ring.begin(frame(0))
    for t in range(5):
        ring.push(np.full((2, 2), t, np.float32) + [[0.0, 0.5], [10.0, 10.5]], np.array([t, -t], np.float32), done[t], frame(t + 1))
    return ring, codes, frame


def test_reference_ring_against_a_hand_written_answer():
    ring, codes, frame = _five_steps()
    assert (ring.first, ring.w, ring.count) == (0, 5, 5)
    assert ring.age[:6].tolist() == [[0, 0], [1, 1], [2, 2], [0, 3], [1, 4], [2, 5]]
    assert ring.done[:5].tolist() == [[0, 0], [0, 0], [5, 0], [0, 0], [0, 8]]
    assert ring.valid_pairs().tolist() == [[s, e] for s in range(5) for e in range(2)]
    g = ring.gather([(2, 0), (3, 0), (0, 1), (4, 1), (4, 0)])
    # env 0, step 2: the full stack, and no next observation (it ended there)
    assert np.array_equal(g["observations"][0], _obs(WHITE, GREY, GREEN)) and not g["next_observations"][0].any()
    # env 0, step 3: the first frame of the next episode - the older frames are blank, not the previous episode's
    assert np.array_equal(g["observations"][1], _obs(BLACK, BLACK, BLUE)) and np.array_equal(g["next_observations"][1], _obs(BLACK, BLUE, RED))
    # env 1, step 0: nothing before the first frame
    assert np.array_equal(g["observations"][2], _obs(BLACK, BLACK, GREY)) and np.array_equal(g["next_observations"][2], _obs(BLACK, GREY, GREEN))
    # env 1, step 4: a collision flag that does not end the episode keeps its next observation
    assert np.array_equal(g["observations"][3], _obs(BLUE, RED, WHITE)) and np.array_equal(g["next_observations"][3], _obs(RED, WHITE, GREEN))
    assert g["dones"].tolist() == [5, 0, 0, 8, 0] and g["rewards"].tolist() == [2.0, 3.0, 0.0, -4.0, 4.0]
    assert g["actions"].tolist() == [[2.0, 2.5], [3.0, 3.5], [10.0, 10.5], [14.0, 14.5], [4.0, 4.5]]
    assert np.array_equal(g["next_observations"][4], _obs(BLUE, RED, GREY))
    # the caller resets env 0: its last stored step is cut, its stack restarts
    ring.begin(np.full((2, P), 3, np.uint8), mask=[1, 0])
    assert ring.done[4].tolist() == [0x80, 8] and ring.age[5].tolist() == [0, 5] and ring.frames[5, :, 0].tolist() == [3, 2]
    g = ring.gather([(4, 0), (4, 1)])
    assert not g["next_observations"][0].any() and g["dones"].tolist() == [0x80, 8]
    assert np.array_equal(g["observations"][0], _obs(BLACK, BLUE, RED)) and np.array_equal(g["next_observations"][1], _obs(RED, WHITE, GREEN))
    # four more steps wrap the ring of eight: one slot is open, seven hold steps, and the two oldest have lost older frames
    for t in range(5, 9):
        ring.push(np.zeros((2, 2), np.float32), np.zeros(2, np.float32), np.zeros(2, np.uint8), frame(t % 6))
    assert (ring.first, ring.w, ring.count) == (2, 1, 7)
    assert ring.age[[5, 6, 7, 0, 1]].tolist() == [[0, 5], [1, 6], [2, 7], [3, 8], [4, 9]]
    valid = set(map(tuple, ring.valid_pairs().tolist()))
    assert valid == {(s, e) for s in (2, 3, 4, 5, 6, 7, 0) for e in (0, 1)} - {(2, 0), (2, 1), (3, 1)}
    # a pair outside the stored range gathers zeros
    g = ring.gather([(1, 0), (9, 0), (3, 2)])
    assert not any(v.any() for k, v in g.items() if k != "indices")
    # a frame that was overwritten is blank, never another time's frame: (3, 1) has age 3 but only slot 2 behind it
    g = ring.gather([(3, 1)])
    assert np.array_equal(g["observations"][0], _obs(BLACK, BLUE, RED))


def test_reference_draw_stays_inside_the_drawable_range():
    ring, _, frame = _five_steps()
    a, b, c = ring.draw(7, 0, 256), ring.draw(7, 0, 256), ring.draw(7, 1, 256)
    assert a.dtype == np.int32 and np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(a, ring.draw(8, 0, 256))
    assert set(a[:, 0].tolist()) == {2, 3, 4} and set(a[:, 1].tolist()) == {0, 1}
    assert not np.array_equal(ring.draw(7, 1 << 32, 256), a)                 # the high word of the counter is a counter word too
    valid = set(map(tuple, ring.valid_pairs().tolist()))
    for t in range(5, 12):                                                  # across the wrap: every drawn pair keeps its whole stack
        ring.push(np.zeros((2, 2), np.float32), np.zeros(2, np.float32), np.array([0, 2 * (t == 7)], np.uint8), frame(t % 6))
        valid = set(map(tuple, ring.valid_pairs().tolist()))
        d = ring.draw(3, t, 128)
        assert set(map(tuple, d.tolist())) <= valid and (ring.offset(d[:, 0]) >= ring.skip).all() and (ring.offset(d[:, 0]) < ring.count).all()
    small = R.Ring(4, 2, n_stack=3, plane=P)
    small.begin(frame(0))
    small.push(np.zeros((2, 2)), np.zeros(2), np.zeros(2, np.uint8), frame(1))
    with pytest.raises(AssertionError):
        small.draw(0, 0, 4)


def test_reference_palette_inverse():
    codes = np.arange(8, dtype=np.uint8)
    rgb = R.PAL[codes].T[None]                                               # [1, 3, 8]
    assert R.layers_of_rgb(rgb).tolist() == [[0, 1, 2, 3, 4, 5, 6, 7]]
    assert R.layers_of_rgb(np.array([[[1], [2], [3]]], np.uint8)).tolist() == [[_abi.LAYER_BLANK]]
