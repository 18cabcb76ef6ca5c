"""CPU checks of the on-policy view of the replay ring (include/tde_onpolicy.h, torchdriveenv_amd/onpolicy.py; the header beside the
others, its symbols and the loader's refusals: tests/test_abi_families_cpu.py): every host-side rejection of the two entry points, of the ops wrappers and of RolloutBuffer's
arguments and call order (all before any launch: no GPU needed), and the numpy restatement (tests/onpolicy_ref.py) against
hand-computed known answers."""
import ctypes as C
import types

import numpy as np
import pytest

from tests import onpolicy_ref as O
from tests.test_replay_cpu import BAD_STRUCTS, _Host
from torchdriveenv_amd import _abi

CUT = _abi.REPLAY_CUT


def _loaded():
    from torchdriveenv_amd import _lib

    return _lib, _lib.load()


def test_entry_points_reject_bad_arguments_without_a_launch():
    _, L = _loaded()
    h = _Host()                                             # C = 6, B = 3, n_stack = 3, plane = 64
    T, N = 4, 5
    side = {k: np.zeros((T, 3), np.float32) for k in ("values", "log_prob", "advantages", "returns")}
    lastv = np.zeros(3, np.float32)
    idx = np.zeros(N, np.int32)
    out = dict(obs=np.zeros((N, 9, 64), np.uint8), action=np.zeros((N, 2), np.float32), old_values=np.zeros(N, np.float32),
               old_log_prob=np.zeros(N, np.float32), adv_out=np.zeros(N, np.float32), ret_out=np.zeros(N, np.float32))
    ptr = lambda a: a.ctypes.data

    def gae(rp=None, first=0, count=5, T_=T, null_rp=False, **over):
        a = {**dict(values=ptr(side["values"]), last_values=ptr(lastv), advantages=ptr(side["advantages"]), returns=ptr(side["returns"])), **over}
        return L.tde_gae(None if null_rp else C.byref(rp or h.rp()), first, count, T_, a["values"], a["last_values"], 0.99, 0.95,
                         a["advantages"], a["returns"], None)

    def gather(rp=None, first=0, count=5, T_=T, N_=N, null_rp=False, **over):
        a = {**dict(idx=ptr(idx)), **{k: ptr(v) for k, v in side.items()}, **{k: ptr(v) for k, v in out.items()}, **over}
        return L.tde_onpolicy_gather(None if null_rp else C.byref(rp or h.rp()), first, count, T_, N_, a["idx"], a["values"], a["log_prob"],
                                     a["advantages"], a["returns"], a["obs"], a["action"], a["old_values"], a["old_log_prob"], a["adv_out"],
                                     a["ret_out"], None)

    names = {gae: b"tde_gae: ", gather: b"tde_onpolicy_gather: "}

    def refused(fn, fragment, **kw):
        rc, err = fn(**kw), L.tde_last_error()
        assert rc != 0 and fragment in err and err.startswith(names[fn]), (fn.__name__, fragment, sorted(kw), rc, err)

    for fn in (gae, gather):
        refused(fn, b"NULL argument", null_rp=True)
        for over, fragment in BAD_STRUCTS:                  # the ring's own rules, as every replay entry point states them
            refused(fn, fragment, rp=h.rp(**over))
        refused(fn, b"16-byte aligned", rp=h.rp(frames=h.frames.ctypes.data + 4))
        for T_ in (0, -3):
            refused(fn, b"T must be >= 1", T_=T_)
        for count in (3, 0, -1):
            refused(fn, b"count must be >= T", count=count)
        refused(fn, b"count must be <= C - 1", count=6)
        refused(fn, b"count must be <= C - 1", count=6, T_=6)
        for first in (-1, 6):
            refused(fn, b"first must be in [0, C)", first=first)
    for name in ("values", "last_values", "advantages", "returns"):
        refused(gae, b"NULL argument", **{name: None})
        refused(gae, b"4-byte aligned", **{name: ptr(side["values"]) + 2})
    for N_ in (0, -2):
        refused(gather, b"N must be >= 1", N_=N_)
    for name in ("idx", "values", "log_prob", "advantages", "returns"):
        refused(gather, b"NULL argument", **{name: None})
        refused(gather, b"4-byte", **{name: ptr(side["values"]) + 2})
    for name in out:
        refused(gather, b"a NULL output", **{name: None})
    refused(gather, b"obs must be 16-byte aligned", obs=ptr(out["obs"]) + 8)
    refused(gather, b"action 8-byte", action=ptr(out["action"]) + 4)
    for name in ("old_values", "old_log_prob", "adv_out", "ret_out"):
        refused(gather, b"4-byte", **{name: ptr(out[name]) + 2})
    # idx is int32: a rollout whose t * B + e does not fit is refused
    refused(gather, b"T * B must be <= INT32_MAX", rp=h.rp(C=2 ** 31 - 1, B=2 ** 30), T_=2, count=2)
    hr = _Host(n_stack=1, plane=0, D=5)
    refused(gather, b"(rows mode: 4)", rp=hr.rp(), obs=ptr(out["obs"]) + 2)
    # nothing was written by any of the calls above
    for a in (h.frames, h.action, h.reward, h.done, h.age, lastv, idx, *side.values(), *out.values()):
        assert not a.view(np.uint8).any()


def test_ops_wrappers_reject_host_tensors_and_bad_shapes():
    import torch

    from torchdriveenv_amd import ops

    z = torch.zeros
    rp = _abi.TdeReplay(6, 2, 3, 64, 0, None, None, None, None, None)
    with pytest.raises(ValueError, match="T must be >= 1"):
        ops.gae(rp, "cuda:0", 0, 4, 0, z((4, 2)), z(2), 0.99, 0.95, z((4, 2)), z((4, 2)))
    with pytest.raises(ValueError, match="values must live on a HIP device"):
        ops.gae(rp, "cuda:0", 0, 4, 4, z((4, 2)), z(2), 0.99, 0.95, z((4, 2)), z((4, 2)))
    with pytest.raises(ValueError, match="values must be torch.float32"):
        ops.gae(rp, "cuda:0", 0, 4, 4, z((4, 2), dtype=torch.float64), z(2), 0.99, 0.95, z((4, 2)), z((4, 2)))
    with pytest.raises(ValueError, match="T must be >= 1"):
        ops.onpolicy_gather(rp, "cuda:0", 0, 4, 0, z(3, dtype=torch.int32), z((4, 2)), z((4, 2)), z((4, 2)), z((4, 2)), {})
    with pytest.raises(ValueError, match="idx must be torch.int32"):
        ops.onpolicy_gather(rp, "cuda:0", 0, 4, 4, z(3, dtype=torch.int64), z((4, 2)), z((4, 2)), z((4, 2)), z((4, 2)), {})
    with pytest.raises(ValueError, match="idx must live on a HIP device"):
        ops.onpolicy_gather(rp, "cuda:0", 0, 4, 4, z(3, dtype=torch.int32), z((4, 2)), z((4, 2)), z((4, 2)), z((4, 2)), {})


def _fake_env(**over):
    kw = dict(auto_reset=True, state={"done_bits": object()}, num_envs=4, torch_device="cuda:0", obs_mode="birdview", frame_stack=3, _res=64)
    kw.update(over)
    from torchdriveenv_amd.config import EnvConfig, RendererConfig, SimulatorConfig
    from torchdriveenv_amd.observe import make_observer

    env = type("FakeEnv", (types.SimpleNamespace,), {})(config=EnvConfig(simulator=SimulatorConfig(renderer=RendererConfig(res=kw["_res"]))), **kw)
    env.observer = make_observer(env)                    # (the observers of birdview and state touch no device when they are made)
    return env


def _bare(pos, finished, n_steps=3, B=4):
    """a RolloutBuffer without its device tensors: the call-order and shape checks come before anything touches them"""
    import torch

    from torchdriveenv_amd.onpolicy import RolloutBuffer

    b = RolloutBuffer.__new__(RolloutBuffer)
    b.n_steps, b.B, b.dev, b.pos, b.finished, b.calls, b.seed = n_steps, B, torch.device("cuda:0"), pos, finished, 0, 0
    return b


def test_rollout_buffer_argument_and_order_checks_need_no_gpu():
    import torch

    from torchdriveenv_amd.env import BatchedWaypointEnv
    from torchdriveenv_amd.onpolicy import RolloutBuffer, RolloutSamples

    for n in (0, -1):
        with pytest.raises(ValueError, match="n_steps must be >= 1"):
            RolloutBuffer(_fake_env(), n)
    with pytest.raises(ValueError, match="auto_reset=True"):
        RolloutBuffer(_fake_env(auto_reset=False), 8)
    with pytest.raises(ValueError, match="with_info=True"):
        RolloutBuffer(_fake_env(state={"done_bits": None}), 8)
    with pytest.raises(ValueError, match=r"H \* W = 16384 exceeds 4096"):
        RolloutBuffer(_fake_env(_res=128), 8)
    assert RolloutSamples._fields == ("observations", "actions", "old_values", "old_log_prob", "advantages", "returns", "indices")
    assert callable(BatchedWaypointEnv.rollout_buffer)
    row, act = torch.zeros(4), torch.zeros(4, 2)
    full, filling, done = _bare(3, False), _bare(2, False), _bare(3, True)
    assert full.full and not filling.full and done.full and len(filling) == 8
    with pytest.raises(ValueError, match=r"already holds n_steps = 3 steps: call finish\(\)"):
        full.push(act, row, row)
    with pytest.raises(ValueError, match=r"finish\(\) needs a full rollout: 2 of n_steps = 3"):
        filling.finish(row)
    for b in (full, filling):
        with pytest.raises(ValueError, match=r"need finish\(\)"):
            b.get()
        with pytest.raises(ValueError, match=r"need finish\(\)"):
            b.get(16)
        with pytest.raises(ValueError, match=r"need finish\(\)"):
            b.gather(torch.zeros(2, dtype=torch.int32))
    for bs in (0, -5):
        with pytest.raises(ValueError, match="batch_size must be >= 1 or None"):
            done.get(bs)
    for bad in (torch.zeros(3), torch.zeros(4, 2), torch.zeros(4, dtype=torch.float64), [0.0] * 4, None):
        with pytest.raises(ValueError, match="values must be a float32 tensor of 4 elements"):
            filling.push(act, bad, row)
        with pytest.raises(ValueError, match="log_probs must be a float32 tensor of 4 elements"):
            filling.push(act, row, bad)
        with pytest.raises(ValueError, match="last_values must be a float32 tensor of 4 elements"):
            full.finish(bad)
    with pytest.raises(ValueError, match="values is on cpu, expected cuda:0"):
        filling.push(act, row, row)
    with pytest.raises(ValueError, match="last_values is on cpu, expected cuda:0"):
        done.finish(row)
    assert (filling.pos, full.pos, done.pos, done.finished) == (2, 3, 3, True)      # a refused call changes nothing


# ---- the numpy restatement against hand-computed answers: T = 3, B = 2, gamma = lambda = 0.5 (gl = 0.25), every intermediate exact ----
REWARD = np.array([[1, 1], [2, 2], [4, 4]], np.float32)
VALUES = np.array([[2, 2], [4, 4], [8, 8]], np.float32)
LAST = np.array([16, 16], np.float32)
# without an ending:  t = 2: delta = 4 + 0.5 * 16 - 8 = 4,  last = 4;   t = 1: delta = 2 + 4 - 4 = 2,  last = 2 + 0.25 * 4 = 3;
#                     t = 0: delta = 1 + 2 - 2 = 1,  last = 1 + 0.25 * 3 = 1.75
OPEN_ADV, OPEN_RET = [1.75, 3.0, 4.0], [3.75, 7.0, 12.0]
# ended at t = 1:     t = 2 as above;   t = 1: delta = 2 + 0 - 4 = -2,  last = -2;   t = 0: delta = 1,  last = 1 + 0.25 * -2 = 0.5
MID_ADV, MID_RET = [0.5, -2.0, 4.0], [2.5, 2.0, 12.0]
# ended at t = 2 (last_values masked):  t = 2: delta = 4 + 0 - 8 = -4,  last = -4;   t = 1: delta = 2,  last = 2 + 0.25 * -4 = 1;
#                     t = 0: delta = 1,  last = 1 + 0.25 * 1 = 1.25
END_ADV, END_RET = [1.25, 1.0, -4.0], [3.25, 5.0, 4.0]


@pytest.mark.parametrize("bit", [1, 2, CUT, 1 | 4, 2 | 8 | 16, CUT | 8])
def test_reference_gae_against_a_hand_computed_answer(bit):
    done = np.array([[0, 0], [bit, 0], [0, 0]], np.uint8)        # env 0 ends at t = 1 (REPLAY_CUT alone among the cases), env 1 never
    adv, ret = O.gae(REWARD, done, VALUES, LAST, 0.5, 0.5)
    assert adv.dtype == ret.dtype == np.float32
    assert adv[:, 0].tolist() == MID_ADV and ret[:, 0].tolist() == MID_RET
    assert adv[:, 1].tolist() == OPEN_ADV and ret[:, 1].tolist() == OPEN_RET
    # at the last step the bootstrap from last_values is masked
    done_end = np.array([[0, 0], [0, 0], [bit, 0]], np.uint8)
    adv, ret = O.gae(REWARD, done_end, VALUES, LAST, 0.5, 0.5)
    assert adv[:, 0].tolist() == END_ADV and ret[:, 0].tolist() == END_RET and adv[:, 1].tolist() == OPEN_ADV


def test_reference_gae_ignores_the_infraction_bits_and_keeps_float32_rounding():
    done = np.array([[4, 8], [16, 4 | 8 | 16], [8, 0]], np.uint8)    # offroad / collided / red light alone end nothing
    adv, ret = O.gae(REWARD, done, VALUES, LAST, 0.5, 0.5)
    assert adv.T.tolist() == [OPEN_ADV] * 2 and ret.T.tolist() == [OPEN_RET] * 2
    # T = 1: delta = r + gamma * last_value - v, one rounding per operation (0.99 and 0.1 are not exact in binary)
    f = np.float32
    adv, ret = O.gae([[f(0.1)]], [[0]], [[f(0.3)]], [f(0.7)], 0.99, 0.95)
    want = f(f(f(0.1) + f(f(0.99) * f(0.7))) - f(0.3)) + f(f(f(0.99) * f(0.95)) * f(0))
    assert adv[0, 0] == want and ret[0, 0] == f(want + f(0.3))


def test_reference_slots_and_gather():
    assert O.slots(first=5, count=6, T=4, C=8).tolist() == [7, 0, 1, 2]
    assert O.slots(first=0, count=3, T=3, C=8).tolist() == [0, 1, 2]
    P = 16
    ring = O.Ring(6, 2, n_stack=3, plane=P)
    frame = lambda t: np.full((2, P), t % 5, np.uint8) + np.array([[0], [1]], np.uint8)
    ring.begin(frame(0))
    for t in range(7):                                      # wraps: first = 2, count = 5, the rollout T = 3 is slots 4, 5, 0
        ring.push(np.full((2, 2), t, np.float32), np.full(2, t, np.float32), np.zeros(2, np.uint8), frame(t + 1))
    assert (ring.first, ring.count) == (2, 5) and O.slots(ring.first, ring.count, 3, 6).tolist() == [4, 5, 0]
    side = [np.arange(6, dtype=np.float32).reshape(3, 2) + 10 * k for k in range(4)]
    g = O.gather(ring, 3, [0, 5, 6, -1, 3], *side)
    want = ring.gather([(4, 0), (0, 1), (-1, 0), (-1, 0), (5, 1)])
    assert np.array_equal(g["observations"], want["observations"]) and g["observations"][:2].any() and not g["observations"][2:4].any()
    assert g["actions"][:, 0].tolist() == [4.0, 6.0, 0.0, 0.0, 5.0]
    assert g["old_values"].tolist() == [0.0, 5.0, 0.0, 0.0, 3.0] and g["returns"].tolist() == [30.0, 35.0, 0.0, 0.0, 33.0]
    assert g["old_log_prob"].tolist() == [10.0, 15.0, 0.0, 0.0, 13.0] and g["advantages"].tolist() == [20.0, 25.0, 0.0, 0.0, 23.0]
