"""float32 numpy restatement of tde_score_plans and tde_score_plans_forecast (include/tde_hip.h; one `score`, forecast= chooses) and
of the refinement rounds of config.PlanRefine, the checker of the plan-set and forecast tests: test infrastructure only, nothing in the
package imports it.  Built on the helpers of tests/planner_ref.py (obb_overlap, box_offroad, ordered, red_hits; the oracle's sincosf,
bicycle and brute-force road predicate), and written the same way: every expression is the header's, in float32.  Also the
module-level tables of inputs that the CPU tests prove meaningful and the GPU tests then run (CASES, tail_corridor)."""
import numpy as np

from oracle import oracle
from tests.planner_ref import box_offroad, obb_overlap, ordered, red_hits
from torchdriveenv_amd import _abi

f32 = np.float32
NONE, OFFROAD, BOX, RED = 0, 1, 2, 3          # cause of a sequence's first failure (the first predicate that holds, in the header's order)


def lattice(pl):
    """float32 [n_a * n_s, 2]: candidate i = ia * n_s + is of a config.Planner as (acceleration, steering)"""
    acc, ste = pl.tables()
    return np.stack([np.repeat(acc, len(ste)), np.tile(ste, len(acc))], -1).astype(f32)


def score(cfg, world, st, pl, seq, knot_len=None, tail=0, only=None, cost=None, fail_step=None, out=None, diag=None, forecast=None):
    """what tde_score_plans writes -> dict(cost float32 [B, N], f int32 [B, N], action float32 [B, 2], diag PLAN_DIAG_DTYPE [B],
    cause int8 [B, N]); rows with only[e] == 0 are those of `cost` / `fail_step` / `out` / `diag` (zeros without them).  forecast (float32
    [B, T, A, 4], horizon + tail <= T <= FORECAST_MAX_T): what tde_score_plans_forecast writes, the same specification with the box of
    present slot j at step h = (x, y, c, s, 0.5f * len_j + margin, 0.5f * wid_j + margin), (x, y, psi) = forecast[e][h - 1][j]; without
    one the others move on the constant-velocity line from the state."""
    B, A = len(st["scn"]), world.A
    seq = np.asarray(seq, f32)
    assert seq.ndim == 4 and seq.shape[0] == B and seq.shape[3] == 2
    N, K = seq.shape[1], seq.shape[2]
    H, T = int(pl.horizon), int(tail)
    L = -(-H // K) if knot_len is None else int(knot_len)
    HT = H + T
    fs = np.shape(forecast)
    assert forecast is None or (fs[0] == B and fs[2:] == (A, 4) and HT <= fs[1] <= _abi.FORECAST_MAX_T)
    r_cost = np.zeros((B, N), f32) if cost is None else np.array(cost, f32, copy=True).reshape(B, N)
    r_f = np.zeros((B, N), np.int32) if fail_step is None else np.array(fail_step, np.int32, copy=True).reshape(B, N)
    act = np.zeros((B, 2), f32) if out is None else np.array(out, f32, copy=True).reshape(B, 2)
    dg = np.zeros(B, _abi.PLAN_DIAG_DTYPE) if diag is None else np.array(diag, copy=True).view(_abi.PLAN_DIAG_DTYPE).reshape(B)
    r_cause = np.zeros((B, N), np.int8)
    res = dict(cost=r_cost, f=r_f, action=act, diag=dg, cause=r_cause)
    envs = np.array([e for e in range(B) if only is None or only[e]], np.int64)
    E = len(envs)
    if E == 0:
        return res
    dt, margin = f32(cfg.dt), f32(pl.margin)
    vt, wp_, ws_, wd_ = f32(pl.v_target), f32(pl.w_progress), f32(pl.w_speed), f32(pl.w_steer)
    rr = f32(cfg.reach_radius)
    box_a, box_d = f32(_abi.PLAN_BOX_ACCEL), f32(_abi.PLAN_BOX_STEER)
    X, Y, P, V, LN, WD, LR = (np.asarray(st[n], f32).reshape(B, A)[envs] for n in ("x", "y", "psi", "v", "len", "wid", "lr"))
    pres = np.asarray(st["present"]).reshape(B, A)[envs] != 0
    scn_t, wp = world.arrays["scn"], world.arrays["wp_xy"]
    sidx = np.asarray(st["scn"])[envs].astype(np.int64)
    maps = scn_t["map"][sidx].astype(np.int32)
    wp_n = scn_t["wp_n"][sidx].astype(np.int64)
    steps = np.asarray(st["steps"])[envs].astype(np.int64)
    # the knots, clamped into the action box (fminf(fmaxf(v, lo), hi): a NaN becomes lo)
    sq = seq[envs]
    KA = np.fmin(np.fmax(sq[..., 0], -box_a), box_a).astype(f32)       # [E, N, K]
    KD = np.fmin(np.fmax(sq[..., 1], -box_d), box_d).astype(f32)
    rep = lambda col: np.repeat(col[:, None], N, 1).astype(col.dtype)   # noqa: E731
    x, y, psi, v = rep(X[:, 0]), rep(Y[:, 0]), rep(P[:, 0]), rep(V[:, 0])
    lr0 = rep(LR[:, 0])
    len0, wid0 = rep(LN[:, 0]), rep(WD[:, 0])
    hl0, hw0 = f32(0.5) * len0, f32(0.5) * wid0
    mapc = np.repeat(maps[:, None], N, 1)
    hlo, hwo = f32(0.5) * LN[:, 1:] + margin, f32(0.5) * WD[:, 1:] + margin
    po = pres[:, 1:]
    # boxes(h) -> (bx, by, Co, So), each [E, A - 1]: the others' centres and headings at step h
    if forecast is None:
        So0, Co0 = oracle.sincosf(P[:, 1:].ravel())
        So0, Co0 = So0.reshape(E, A - 1), Co0.reshape(E, A - 1)
        ux, uy = (V[:, 1:] * Co0) * dt, (V[:, 1:] * So0) * dt

        def boxes(h):
            fh = f32(h)
            return X[:, 1:] + fh * ux, Y[:, 1:] + fh * uy, Co0, So0
    else:
        FC = np.asarray(forecast, f32)[envs]

        def boxes(h):
            So_, Co_ = oracle.sincosf(np.ascontiguousarray(FC[:, h - 1, 1:, 2]).ravel())
            return FC[:, h - 1, 1:, 0], FC[:, h - 1, 1:, 1], Co_.reshape(E, A - 1), So_.reshape(E, A - 1)
    ti = rep(np.asarray(st["target_idx"])[envs].astype(np.int64))
    wpn = rep(wp_n)
    sc_ = rep(sidx)
    NW = wp.shape[1]

    def target(ti_):
        j = np.clip(ti_, 0, NW - 1)
        return wp[sc_, j, 0].astype(f32), wp[sc_, j, 1].astype(f32)

    def dist(wx_, wy_, x_, y_):
        dx, dy = wx_ - x_, wy_ - y_
        return np.sqrt(dx * dx + dy * dy)

    wx, wy = target(ti)
    has = ti < wpn
    dp = np.where(has, dist(wx, wy, x, y), f32(0)).astype(f32)
    gain, sv, dm = np.zeros((E, N), f32), np.zeros((E, N), f32), np.zeros((E, N), f32)
    a1 = np.where(v + KA[..., 0] * dt < f32(0), f32(0), KA[..., 0]).astype(f32)
    d1 = KD[..., 0].copy()
    alive = np.ones((E, N), bool)
    f = np.full((E, N), HT + 1, np.int64)
    cause = np.zeros((E, N), np.int8)
    lights_on = bool(cfg.flags & _abi.F_TRAFFIC_LIGHTS)
    d = KD[..., 0]
    for h in range(1, HT + 1):
        if not alive.any():
            break
        in_tail = h > H
        if in_tail:
            a = np.full((E, N), -box_a, f32)                           # (d stays that of step H)
            alive &= ~(v + a * dt < f32(0))                            # at rest: safe
            if not alive.any():
                break
        else:
            k = min((h - 1) // L, K - 1)
            a, d = KA[..., k], KD[..., k]
            dm = np.where(alive, np.fmax(dm, d * d), dm).astype(f32)
        ah = np.where(v + a * dt < f32(0), f32(0), a).astype(f32)
        ix = np.flatnonzero(alive.ravel())
        xs, ys, ps, vs = (np.ascontiguousarray(q.ravel()[ix]) for q in (x, y, psi, v))
        oracle.kinematics_step(xs, ys, ps, vs, np.ascontiguousarray(lr0.ravel()[ix]), np.ones(len(ix), np.uint8),
                               np.ascontiguousarray(np.stack([ah.ravel()[ix], d.ravel()[ix]], -1)), float(dt))
        for q, qs in ((x, xs), (y, ys), (psi, ps), (v, vs)):
            q.ravel()[ix] = qs
        sn, cs = oracle.sincosf(psi.ravel())
        sn, cs = sn.reshape(E, N), cs.reshape(E, N)
        off = np.zeros((E, N), bool)
        off.ravel()[ix] = box_offroad(cfg, world, mapc.ravel()[ix], xs, ys, ps, len0.ravel()[ix], wid0.ravel()[ix])
        bx, by, Co, So = boxes(h)
        hit = np.zeros((E, N), bool)
        for j in range(A - 1):                                          # (slot by slot: [E, N, A - 1] temporaries are large at N = 1024)
            if not po[:, j].any():
                continue
            hj = obb_overlap(x, y, cs, sn, hl0, hw0, bx[:, j, None], by[:, j, None], Co[:, j, None], So[:, j, None], hlo[:, j, None],
                             hwo[:, j, None])
            hit |= hj & po[:, j, None]
        red = red_hits(world, maps, steps, h, x, y, cs, sn, hl0, hw0) if lights_on else np.zeros((E, N), bool)
        fail = off | hit | red
        died = alive & fail
        f[died] = h
        cause[died] = np.where(off, OFFROAD, np.where(hit, BOX, RED))[died]
        alive &= ~fail
        if in_tail:
            continue
        has = alive & (ti < wpn)
        dn = dist(wx, wy, x, y)
        gain = np.where(has, gain + (dp - dn), gain).astype(f32)
        dp = np.where(has, dn, dp).astype(f32)
        adv = has & (dn < rr)
        ti = ti + adv
        nwx, nwy = target(ti)
        more = adv & (ti < wpn)
        wx, wy = np.where(more, nwx, wx).astype(f32), np.where(more, nwy, wy).astype(f32)
        dp = np.where(more, dist(wx, wy, x, y), dp).astype(f32)
        ev = v - np.where(ti < wpn, vt, f32(0)).astype(f32)
        sv = np.where(alive, sv + ev * ev, sv).astype(f32)
    run = (ws_ * sv + wd_ * dm) - wp_ * gain
    c = ((HT + 1 - f).astype(f32) * f32(_abi.PLAN_FAIL_UNIT) +
         np.fmin(np.fmax(run + f32(_abi.PLAN_RUN_BIAS), f32(0)), f32(_abi.PLAN_RUN_MAX))).astype(f32)
    key = (ordered(c.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | np.arange(N)[None].astype(np.uint64)
    win = key.argmin(1)
    r = np.arange(E)
    r_cost[envs], r_f[envs], r_cause[envs] = c, f, cause
    act[envs, 0], act[envs, 1] = a1[r, win], d1[r, win]
    dg["winner"][envs], dg["fail_step"][envs], dg["cost"][envs] = win, f[r, win], c[r, win]
    dg["n_safe"][envs] = (f == HT + 1).sum(1)
    return res


def refine(cfg, world, st, pl, pr, only=None, out=None, diag=None):
    """BatchedWaypointEnv.plan_actions() under a config.PlanRefine -> (action [B, 2], diag [B], [the winning cost of every round,
    float32 [B]]); rows with only[e] == 0 are those of `out` / `diag`"""
    B = len(st["scn"])
    lat = lattice(pl)
    nc, K, R = len(lat), int(pr.knots), int(pr.rounds)
    L = -(-int(pl.horizon) // K)
    seqs = np.ascontiguousarray(np.broadcast_to(lat[None, :, None, :], (B, nc, K, 2)))
    res = score(cfg, world, st, pl, seqs, L, pr.tail, only=only, out=out, diag=diag)
    costs = [res["diag"]["cost"].copy()]
    lo, hi = np.array([-_abi.PLAN_BOX_ACCEL, -_abi.PLAN_BOX_STEER], f32), np.array([_abi.PLAN_BOX_ACCEL, _abi.PLAN_BOX_STEER], f32)
    s = f32(1.0)
    for _ in range(R):
        s = f32(s * f32(pr.shrink))
        delta = (lat * s).astype(f32)
        win = np.clip(res["diag"]["winner"], 0, seqs.shape[1] - 1)
        w = seqs[np.arange(B), win]                                    # [B, K, 2]
        cand = np.ascontiguousarray(np.broadcast_to(w[:, None, None, :, :], (B, K, nc, K, 2)))
        for k in range(K):
            cand[:, k, :, k, :] = np.minimum(np.maximum(w[:, k, None, :] + delta[None], lo), hi)
        seqs = cand.reshape(B, K * nc, K, 2)
        res = score(cfg, world, st, pl, seqs, L, pr.tail, only=only, out=res["action"], diag=res["diag"])
        costs.append(res["diag"]["cost"].copy())
    return res["action"], res["diag"], costs


# ---- inputs shared by the CPU tests (which prove them meaningful by the restatement alone) and the GPU tests ---------------------

def reset_state(cfg, world, B, episode=0):
    from torchdriveenv_amd.state import EnvState

    hs = EnvState(B, world.A)
    hs["episode"][...] = episode
    oracle.env_reset(cfg, world, hs)
    return hs


def lights_cfg(world, **kw):
    cfg = _abi.default_config(**kw)
    if world.has_lights:
        cfg.flags |= _abi.F_TRAFFIC_LIGHTS
    return cfg


def random_knots(rng, B, N, K, wild=False):
    """seeded knot sequences: accelerations and steerings uniform over the action box (wild: over twice the box, with one NaN knot
    per env, for the clamp rule)"""
    sc = 2.0 if wild else 1.0
    seq = np.stack([rng.uniform(-sc, sc, (B, N, K)), rng.uniform(-0.3 * sc, 0.3 * sc, (B, N, K))], -1).astype(f32)
    if wild:
        seq[:, N // 2, K // 2, :] = np.nan
    return seq


def calm_knots(rng, seq):
    """`seq` [B, N, K, 2] with a third of its sequences overwritten in place by ones that brake gently and steer little, so that some
    are safe whatever the scene"""
    calm = rng.random(seq.shape[:2]) < 0.35
    seq[calm] = np.stack([rng.uniform(-1.0, 0.1, seq[calm].shape[:-1]), rng.uniform(-0.02, 0.02, seq[calm].shape[:-1])], -1).astype(f32)
    return seq


# name -> dict(world, B, seed, N, K, knot_len, tail, H, lights, steps, edge, squared, only, wild): the parametrised inputs of GPU tests
# 2 and 3.  H = 32 throughout but where stated.  knot_len: K * knot_len > H cuts the last knot short, K * knot_len < H stretches it.
CASES = {
    "n1_k1": dict(B=48, seed=21, N=1, K=1, knot_len=32, tail=0),
    "n63_k2_cut": dict(B=32, seed=22, N=63, K=2, knot_len=20, tail=10),
    "n64_k4_stretched": dict(B=32, seed=23, N=64, K=4, knot_len=5, tail=64),
    "n65_k4_cut": dict(B=24, seed=24, N=65, K=4, knot_len=9, tail=10),
    "n200_k32": dict(B=16, seed=25, N=200, K=32, knot_len=1, tail=0),
    "n200_k32_h20_knots_unused": dict(B=12, seed=26, N=200, K=32, knot_len=1, tail=64, H=20),
    "n1024_k2": dict(B=6, seed=27, N=1024, K=2, knot_len=16, tail=10),
    "lights_phase_in_horizon": dict(B=32, seed=28, N=65, K=2, knot_len=16, tail=10, lights=True, steps=60),
    "lights_phase_in_tail": dict(B=32, seed=29, N=63, K=2, knot_len=16, tail=64, lights=True, steps=30),
    "grid_edge": dict(B=48, seed=30, N=65, K=2, knot_len=16, tail=10, edge=True),
    "squared_threshold": dict(B=6, seed=31, N=65, K=2, knot_len=6, tail=10, H=10, squared=True),
    "only_mask": dict(B=40, seed=32, N=130, K=4, knot_len=8, tail=10, only=True),
    "clamp_and_nan": dict(B=32, seed=33, N=64, K=4, knot_len=8, tail=10, wild=True),
}


def case_inputs(name, small_world=None):
    """(cfg, world, host state, Planner, seq [B, N, K, 2], knot_len, tail, only or None) of CASES[name]"""
    from torchdriveenv_amd.config import Planner
    from torchdriveenv_amd.synth import synthetic_world
    from torchdriveenv_amd.world import effective_offroad_distance

    c = CASES[name]
    B, seed = c["B"], c["seed"]
    rng = np.random.default_rng(seed)
    if c.get("squared"):
        world = synthetic_world(n_scn=8, A=16, seed=0, n_maps=2, threshold=effective_offroad_distance(0.5, True))
        cfg = lights_cfg(world, seed=seed, offroad_threshold=0.5, offroad_threshold_squared=1)
    else:
        world = small_world if small_world is not None else synthetic_world(n_scn=8, A=16, seed=0, n_maps=2)
        cfg = lights_cfg(world, seed=seed)
    A = world.A
    hs = reset_state(cfg, world, B)
    hs["steps"][...] = c.get("steps", 0)
    if c.get("lights"):
        # half of the egos a few metres in front of a stop line of their map, heading across it (tests/test_gpu_planner.py's scene)
        assert cfg.flags & _abi.F_TRAFFIC_LIGHTS
        mp, stop = world.arrays["maps"], world.arrays["stoplines"]
        m = world.map_of_scn()[hs["scn"]]
        for e in range(0, B, 2):
            n = int(mp["n_stop"][m[e]])
            if n == 0:
                continue
            ln = stop[int(mp["stop_base"][m[e]]) + int(rng.integers(n))]
            back = rng.uniform(3.0, 16.0)
            hs["x"][e * A], hs["y"][e * A] = ln["x"] - back * ln["c"], ln["y"] - back * ln["s"]
            hs["psi"][e * A] = np.arctan2(ln["s"], ln["c"])
            hs["v"][e * A] = rng.uniform(2.0, 8.0)
        hs["steps"][1::4] += 15                                         # (more than one phase offset in the batch)
    if c.get("edge"):
        mp = world.arrays["maps"]
        m = world.map_of_scn()[hs["scn"]]
        ox, oy = mp["ox"][m], mp["oy"][m]
        hgt = mp["ny"][m] * mp["cell"][m]
        x0, y0 = hs["x"][::A].astype(np.float64), hs["y"][::A].astype(np.float64)
        n = B // 4
        a, b = slice(0, n), slice(n, 2 * n)
        x0[a] = ox[a] + rng.uniform(0.2, 3.0, n)                        # near the edge, inside
        y0[a] = oy[a] + rng.uniform(0.0, 1.0, n) * hgt[a]
        x0[b] = ox[b] - rng.uniform(1.0, 30.0, n)                       # beyond it
        y0[b] = oy[b] + rng.uniform(-10.0, 30.0, n) + hgt[b]
        hs["x"][::A], hs["y"][::A] = x0.astype(f32), y0.astype(f32)
        hs["psi"][:2 * n * A:A] = rng.uniform(-3.14, 3.14, 2 * n).astype(f32)
    pl = Planner(horizon=c.get("H", 32))
    seq = calm_knots(rng, random_knots(rng, B, c["N"], c["K"], wild=bool(c.get("wild"))))
    only = (rng.random(B) < 0.5).astype(np.uint8) if c.get("only") else None
    return cfg, world, hs, pl, seq, c["knot_len"], c["tail"], only


def tail_corridor(line_near=16.0):
    """the tail's known answer: a 200 m corridor with one stop line red for the whole window, an ego at 4 m/s whose front bumper is
    `line_near` metres short of the line's near edge -> (cfg, world, host state, Planner, seq [1, 2, 1, 2] = (coast, full brake)).
    Coasting covers 12.8 m in H = 32 steps and needs 8 m more to stop; braking from the start needs 8 m in all."""
    from torchdriveenv_amd.config import Planner
    from torchdriveenv_amd.state import EnvState
    from torchdriveenv_amd.world import assemble_world, corridor_mesh

    x0, hl, line_hl, A = 100.0, 2.25, 0.5, 8
    centre = x0 + hl + line_near + line_hl
    scn = dict(map=0, waypoints=[(150.0, 0.0), (190.0, 0.0)], start_heading=0.0, agents=[], ego_attr=(4.5, 2.0, 1.5))
    world = assemble_world([corridor_mesh([[(0.0, 0.0), (200.0, 0.0)]], width=12.0)], [scn], A, threshold=0.5, cell=0.25,
                           lights=[dict(stoplines=[(centre, 0.0, 0.0, line_hl, 9.0, 0)], phases=[(400, [0]), (1, [])])])
    cfg = _abi.default_config(seed=1)
    cfg.flags |= _abi.F_TRAFFIC_LIGHTS
    st = EnvState(1, A)
    for k in ("x", "y", "psi", "v", "present", "scn", "steps", "target_idx"):
        st[k][...] = 0
    st["len"][...], st["wid"][...], st["lr"][...] = 4.5, 2.0, 1.5
    st["present"][0], st["x"][0], st["v"][0] = 1, x0, 4.0
    seq = np.array([[[[0.0, 0.0]], [[-1.0, 0.0]]]], f32)
    return cfg, world, st, Planner(), seq
