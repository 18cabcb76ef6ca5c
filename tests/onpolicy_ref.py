"""numpy statement of the on-policy view of the replay ring (include/tde_onpolicy.h): which slots the rollout is, generalised advantage
estimation in float32 with one numpy float32 operation per written operation, and the minibatch gather built on tests/replay_ref.Ring."""
import numpy as np

from tests.replay_ref import ENDED, Ring

F = np.float32


def slots(first, count, T, C):
    """the slot of every step of the rollout: the newest T of the `count` valid slots from `first`"""
    assert T >= 1 and count >= T
    return (first + count - T + np.arange(T)) % C


def gae(reward, done, values, last_values, gamma, lam):
    """reward float32 [T, B] and done uint8 [T, B] in TIME order, values float32 [T, B], last_values float32 [B] ->
    advantages, returns float32 [T, B]"""
    reward, values, last_values = np.asarray(reward, F), np.asarray(values, F), np.asarray(last_values, F)
    done = np.asarray(done, np.uint8)
    T, B = values.shape
    gamma, zero = F(gamma), np.zeros(B, F)
    gl = F(gamma * F(lam))
    adv, ret = np.zeros((T, B), F), np.zeros((T, B), F)
    last = np.zeros(B, F)
    for t in range(T - 1, -1, -1):
        nnt = (done[t] & ENDED) == 0
        nv = last_values if t == T - 1 else values[t + 1]
        boot = np.where(nnt, gamma * nv, zero)
        delta = (reward[t] + boot) - values[t]
        carry = np.where(nnt, gl * last, zero)
        last = delta + carry
        adv[t] = last
        ret[t] = last + values[t]
    assert adv.dtype == F and ret.dtype == F and last.dtype == F
    return adv, ret


def ring_gae(ring, T, values, last_values, gamma, lam):
    """gae over the newest T stored steps of a replay_ref.Ring"""
    s = slots(ring.first, ring.count, T, ring.C)
    return gae(ring.reward[s], ring.done[s], values, last_values, gamma, lam)


def gather(ring, T, idx, values, log_prob, advantages, returns):
    """the samples idx (t * B + e over the newest T stored steps of `ring`); an index outside [0, T * B) gathers zeros"""
    idx = np.asarray(idx, np.int64).reshape(-1)
    n, B = len(idx), ring.B
    s = slots(ring.first, ring.count, T, ring.C)
    ok = (idx >= 0) & (idx < T * B)
    t, e = np.where(ok, idx // B, 0), np.where(ok, idx % B, 0)
    # Ring.gather zeroes a pair outside the ring: (-1, 0) is one
    g = ring.gather(np.stack([np.where(ok, s[t], -1), e], 1))
    side = [np.where(ok, np.asarray(a, F)[t, e], F(0)).astype(F) for a in (values, log_prob, advantages, returns)]
    assert g["observations"].shape[0] == n
    return {"observations": g["observations"], "actions": g["actions"], "old_values": side[0], "old_log_prob": side[1],
            "advantages": side[2], "returns": side[3], "indices": idx.astype(np.int32)}


__all__ = ["Ring", "gae", "gather", "ring_gae", "slots"]
