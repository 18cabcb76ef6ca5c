"""numpy restatement of tde_score_plans_scene (include/tde_hip.h) BY COMPOSITION, the checker of the scene-judge tests: test
infrastructure only, nothing in the package imports it.  No new physics is written here: the host state is tiled N times into B * N
virtual envs, each sequence's effective actions are formed with the ego alone (the clamp, the no-reverse rule, the tail, the oracle's
bicycle), tests/forecast_scene_ref.forecast_scene moves the tiled scenes under those actions and tests/plan_set_ref.score judges one
sequence per tiled env on those rows.  Also the look-ahead check both test files share: the judge's fail_step against an environment
that is really stepped."""
import numpy as np

from oracle import oracle
from tests import forecast_scene_ref as Sr
from tests import plan_set_ref as S
from tests.planner_ref import ordered
from torchdriveenv_amd import _abi

f32 = np.float32
INFRACTION = 4 | 8 | 16                 # tde_state.done_bits: offroad, collided, red-light violation
ENDED = 1 | 2                           # terminated, truncated


def arrays_of(hs):
    return {k: np.asarray(v) for k, v in (hs.arrays if hasattr(hs, "arrays") else hs).items() if v is not None}


def tile_state(hs, N):
    """the host state's arrays with every env repeated N times in place (virtual env e * N + n = env e): a dict of numpy arrays"""
    out = {}
    for k, a in arrays_of(hs).items():
        if k in ("slot_cache", "env_cache", "act_cache"):
            continue
        B = len(np.asarray(arrays_of(hs)["scn"]))
        out[k] = np.ascontiguousarray(np.repeat(a.reshape(B, -1), N, axis=0).reshape((a.shape[0] * N,) + a.shape[1:]))
    return out


def effective_actions(cfg, hs, pl, seq, knot_len=None, tail=0, with_steps=False):
    """float32 [B * N, H + tail, 2]: what the ego of each sequence does at every step while it is judged - (a_h, d_h) under the
    knots, a_h after the no-reverse rule; (-1, d_H) through the tail until it stands (zeros after: those rows are never read).
    with_steps: (actions, int64 [B * N] number of steps each sequence moves: H + tail unless it stands before)"""
    st = arrays_of(hs)
    seq = np.asarray(seq, f32)
    B, N, K = seq.shape[:3]
    A = len(st["x"]) // B
    H, T = int(pl.horizon), int(tail)
    L = -(-H // K) if knot_len is None else int(knot_len)
    dt = f32(cfg.dt)
    box_a, box_d = f32(_abi.PLAN_BOX_ACCEL), f32(_abi.PLAN_BOX_STEER)
    KA = np.fmin(np.fmax(seq[..., 0], -box_a), box_a).astype(f32).reshape(B * N, K)
    KD = np.fmin(np.fmax(seq[..., 1], -box_d), box_d).astype(f32).reshape(B * N, K)
    x, y, psi, v, lr = (np.ascontiguousarray(np.repeat(st[n].reshape(B, A)[:, 0].astype(f32), N)) for n in ("x", "y", "psi", "v", "lr"))
    act = np.zeros((B * N, H + T, 2), f32)
    going = np.ones(B * N, bool)
    moved = np.zeros(B * N, np.int64)
    d = KD[:, 0]
    for h in range(1, H + T + 1):
        if h > H:
            a = np.full(B * N, -box_a, f32)
            going &= ~(v + a * dt < f32(0))
        else:
            k = min((h - 1) // L, K - 1)
            a, d = KA[:, k], KD[:, k]
        ah = np.where(v + a * dt < f32(0), f32(0), a).astype(f32)
        ix = np.flatnonzero(going)
        if len(ix) == 0:
            break
        act[ix, h - 1, 0], act[ix, h - 1, 1] = ah[ix], d[ix]
        moved[ix] = h
        xs, ys, ps, vs = (np.ascontiguousarray(q[ix]) for q in (x, y, psi, v))
        oracle.kinematics_step(xs, ys, ps, vs, np.ascontiguousarray(lr[ix]), np.ones(len(ix), np.uint8), np.ascontiguousarray(act[ix, h - 1]),
                               float(dt))
        x[ix], y[ix], psi[ix], v[ix] = xs, ys, ps, vs
    return (act, moved) if with_steps else act


def score(cfg, world, hs, pl, seq, knot_len=None, tail=0, only=None, cost=None, fail_step=None, out=None, diag=None):
    """what tde_score_plans_scene writes -> dict(cost float32 [B, N], f int32 [B, N], action float32 [B, 2], diag PLAN_DIAG_DTYPE [B]);
    rows with only[e] == 0 are those of `cost` / `fail_step` / `out` / `diag` (zeros without them)"""
    seq = np.asarray(seq, f32)
    B, N, K = seq.shape[:3]
    H, T = int(pl.horizon), int(tail)
    L = -(-H // K) if knot_len is None else int(knot_len)
    r_cost = np.zeros((B, N), f32) if cost is None else np.array(cost, f32, copy=True).reshape(B, N)
    r_f = np.zeros((B, N), np.int32) if fail_step is None else np.array(fail_step, np.int32, copy=True).reshape(B, N)
    act = np.zeros((B, 2), f32) if out is None else np.array(out, f32, copy=True).reshape(B, 2)
    dg = np.zeros(B, _abi.PLAN_DIAG_DTYPE) if diag is None else np.array(diag, copy=True).view(_abi.PLAN_DIAG_DTYPE).reshape(B)
    res = dict(cost=r_cost, f=r_f, action=act, diag=dg)
    envs = np.array([e for e in range(B) if only is None or only[e]], np.int64)
    if len(envs) == 0:
        return res
    tiled = tile_state(hs, N)
    only_t = None if only is None else np.repeat(np.asarray(only, np.uint8), N)
    ea = effective_actions(cfg, hs, pl, seq, L, T)
    fc = Sr.forecast_scene(cfg, world, tiled, H + T, ego_action=ea, only=only_t)
    one = S.score(cfg, world, tiled, pl, seq.reshape(B * N, 1, K, 2), L, T, only=only_t, forecast=fc)
    c, f = one["cost"].reshape(B, N)[envs], one["f"].reshape(B, N)[envs]
    a1 = one["action"].reshape(B, N, 2)[envs]
    key = (ordered(c.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | np.arange(N)[None].astype(np.uint64)
    win = key.argmin(1)
    r = np.arange(len(envs))
    r_cost[envs], r_f[envs] = c, f
    act[envs] = a1[r, win]
    dg["winner"][envs], dg["fail_step"][envs], dg["cost"][envs] = win, f[r, win], c[r, win]
    dg["n_safe"][envs] = (f == H + T + 1).sum(1)
    return res


def check_lookahead(f, ea, moved, HT, step):
    """the judge's fail_step `f` [V] of V virtual envs against an environment that is really stepped under their effective actions
    `ea` [V, HT, 2] (effective_actions; moved [V]: the steps each sequence moves): step(h, actions [V, 2]) -> done_bits [V] of step
    h (uint8, tde_state.done_bits).  A virtual env is followed until its episode ends (a re-spawn follows) or its sequence stands.  Returns (number that failed inside the horizon, number that
    survived it); raises AssertionError on a disagreement."""
    V = len(f)
    f = np.asarray(f).reshape(V)
    open_ = np.ones(V, bool)
    moved = np.asarray(moved).reshape(V)
    first = np.zeros(V, np.int64)               # step of the first infraction, 0: none while followed
    other_end = np.zeros(V, np.int64)           # step at which the episode ended without an infraction, 0: it did not
    for h in range(1, HT + 1):
        open_ &= h <= moved
        if not open_.any():
            break
        bits = np.asarray(step(h, np.ascontiguousarray(ea[:, h - 1]))).reshape(V)
        inf = open_ & ((bits & INFRACTION) != 0)
        first[inf] = h
        end = open_ & ~inf & ((bits & ENDED) != 0)
        other_end[end] = h
        open_ &= ~(inf | end)
    hit = first > 0
    bad = np.flatnonzero(hit & (f != first))
    assert len(bad) == 0, ("the step ends the episode at another step than the judge", len(bad), bad[:6].tolist(), f[bad[:6]], first[bad[:6]])
    bad = np.flatnonzero((other_end > 0) & ~(f > other_end))
    assert len(bad) == 0, ("the judge fails a sequence before its episode ends clean", len(bad), bad[:6].tolist(), f[bad[:6]], other_end[bad[:6]])
    clean = ~hit & (other_end == 0)
    bad = np.flatnonzero(clean & (f != HT + 1))
    assert len(bad) == 0, ("the judge fails a sequence the step never faults", len(bad), bad[:6].tolist(), f[bad[:6]])
    return int(hit.sum()), int((f == HT + 1).sum())
