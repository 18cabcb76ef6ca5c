"""float32 numpy restatement of tde_plan_action (include/tde_hip.h), the checker of the planner tests: test infrastructure only, nothing
in the package imports it.  Takes a World, a HOST state (EnvState without a device, or a dict of its numpy arrays), the tde_config and
a config.Planner; every expression is the header's, in float32 (numpy rounds once per operation and never contracts).  Headings go
through the oracle's sincosf, the trajectories through the oracle's bicycle (kinematics_step: tde_oracle_bicycle per row), the road
predicate through the oracle's brute force over the map's triangles (compute_offroad of the ego's box; point_near_mesh per corner
under the squared reading).  The overlap test is tde_device.h's obb_overlap written out on arrays (obb_overlap below; the CPU tests
hold it against oracle.obb_overlap).  tests/plan_set_ref.py restates the plan judge on these helpers; of `plan` itself it shares
the stop-line walk (red_hits) and nothing else, so that the tests which hold the two equal compare two statements."""
import numpy as np

from oracle import oracle
from tests.vector_obs_ref import red_mask
from torchdriveenv_amd import _abi

f32 = np.float32


def obb_overlap(xi, yi, ci, si, hli, hwi, xj, yj, cj, sj, hlj, hwj):
    """strict separating-axis overlap of box i with box j (float32 arrays, broadcast): the expressions of tde_device.h: obb_overlap"""
    dx, dy = xj - xi, yj - yi
    c = ci * cj + si * sj
    s = ci * sj - si * cj
    ac, asn = np.abs(c), np.abs(s)
    ok = np.abs(dx * ci + dy * si) < hli + (hlj * ac + hwj * asn)
    ok = ok & (np.abs(dy * ci - dx * si) < hwi + (hlj * asn + hwj * ac))
    ok = ok & (np.abs(dx * cj + dy * sj) < hlj + (hli * ac + hwi * asn))
    ok = ok & (np.abs(dy * cj - dx * sj) < hwj + (hli * asn + hwi * ac))
    return ok


def box_offroad(cfg, world, maps, x, y, psi, ln, wd):
    """the step's offroad predicate of boxes (x, y, psi, len, wid), maps[i] = the map of box i -> bool [n]"""
    n = len(x)
    if n == 0:
        return np.zeros(0, bool)
    x, y, psi, ln, wd = (np.ascontiguousarray(a, f32) for a in (x, y, psi, ln, wd))
    if not cfg.offroad_threshold_squared:
        off = oracle.compute_offroad(n, 1, x, y, psi, ln, wd, np.ones(n, np.uint8), world, np.ascontiguousarray(maps, np.int32),
                                     f32(cfg.offroad_threshold))
        return off != 0
    sn, cs = oracle.sincosf(psi)
    hl, hw = f32(0.5) * ln, f32(0.5) * wd
    lx, ly, wx, wy = hl * cs, hl * sn, hw * sn, hw * cs
    cx = [(x + lx) - wx, (x + lx) + wx, (x - lx) + wx, (x - lx) - wx]
    cy = [(y + ly) + wy, (y + ly) - wy, (y - ly) - wy, (y - ly) + wy]
    tri, mp = world.arrays["tri"], world.arrays["maps"]
    out = np.zeros(n, bool)
    for i in range(n):
        m = mp[maps[i]]
        t = tri[int(m["tri_base"]):int(m["tri_base"]) + int(m["n_tri"])]
        out[i] = any(not oracle.point_near_mesh(cx[k][i], cy[k][i], t, f32(cfg.offroad_threshold)) for k in range(4))
    return out


def ordered(bits):
    """the cost's bits (uint32) as an ordered unsigned integer"""
    b = np.asarray(bits, np.uint32)
    return np.where(b >> np.uint32(31), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def red_hits(world, maps, steps, h, x, y, cs, sn, hl0, hw0):
    """the stop-line walk of step h -> bool [E, n]: box (x, y, cs, sn, hl0, hw0)[i][c] overlaps a stop line of map maps[i] whose light
    is red at step steps[i] + h; maps without stop lines or without a cycle are skipped"""
    mp, stop = world.arrays["maps"], world.arrays["stoplines"]
    red = np.zeros(x.shape, bool)
    for i in range(len(maps)):
        m = mp[maps[i]]
        n_stop = int(m["n_stop"])
        if n_stop <= 0 or int(m["cycle_steps"]) <= 0:
            continue
        rm = red_mask(world, maps[i], steps[i] + h)
        lines = stop[int(m["stop_base"]):int(m["stop_base"]) + n_stop]
        lines = lines[((rm >> (lines["light"].astype(np.int64) & 31)) & 1) != 0]
        if len(lines):
            hit = obb_overlap(x[i][:, None], y[i][:, None], cs[i][:, None], sn[i][:, None], hl0[i][:, None], hw0[i][:, None],
                              lines["x"][None], lines["y"][None], lines["c"][None], lines["s"][None], lines["hl"][None],
                              lines["hw"][None])
            red[i] = hit.any(1)
    return red


def plan(cfg, world, st, pl, only=None, out=None, diag=None, detail=False):
    """what tde_plan_action writes: (action float32 [B, 2], diag PLAN_DIAG_DTYPE [B]); rows with only[e] == 0 are those of `out` /
    `diag` (zeros without them).  detail=True: also (f int [E, nc], cost float32 [E, nc]) of the planned envs."""
    B, A = len(st["scn"]), world.A
    acc, ste = pl.tables()
    n_s, nc = len(ste), len(acc) * len(ste)
    H = int(pl.horizon)
    act = np.zeros((B, 2), f32) if out is None else np.array(out, f32, copy=True).reshape(B, 2)
    dg = np.zeros(B, _abi.PLAN_DIAG_DTYPE) if diag is None else np.array(diag, copy=True).view(_abi.PLAN_DIAG_DTYPE).reshape(B)
    envs = np.array([e for e in range(B) if only is None or only[e]], np.int64)
    E = len(envs)
    if E == 0:
        return (act, dg, None, None) if detail else (act, dg)
    dt, margin = f32(cfg.dt), f32(pl.margin)
    vt, wp_, ws_, wd_ = f32(pl.v_target), f32(pl.w_progress), f32(pl.w_speed), f32(pl.w_steer)
    rr = f32(cfg.reach_radius)
    X, Y, P, V, LN, WD, LR = (np.asarray(st[n], f32).reshape(B, A)[envs] for n in ("x", "y", "psi", "v", "len", "wid", "lr"))
    pres = np.asarray(st["present"]).reshape(B, A)[envs] != 0
    scn_t, wp = world.arrays["scn"], world.arrays["wp_xy"]
    sidx = np.asarray(st["scn"])[envs].astype(np.int64)
    maps = scn_t["map"][sidx].astype(np.int32)
    wp_n = scn_t["wp_n"][sidx].astype(np.int64)
    steps = np.asarray(st["steps"])[envs].astype(np.int64)
    # candidates [E, nc]
    ci = np.arange(nc)
    a = np.broadcast_to(acc[ci // n_s][None], (E, nc)).astype(f32)
    d = np.broadcast_to(ste[ci % n_s][None], (E, nc)).astype(f32)
    rep = lambda col: np.repeat(col[:, None], nc, 1).astype(col.dtype)   # noqa: E731
    x, y, psi, v = rep(X[:, 0]), rep(Y[:, 0]), rep(P[:, 0]), rep(V[:, 0])
    lr0 = rep(LR[:, 0])
    len0, wid0 = rep(LN[:, 0]), rep(WD[:, 0])
    hl0, hw0 = f32(0.5) * len0, f32(0.5) * wid0
    mapc = np.repeat(maps[:, None], nc, 1)
    # the others [E, 1, A - 1]
    So, Co = oracle.sincosf(P[:, 1:].ravel())
    So, Co = So.reshape(E, A - 1), Co.reshape(E, A - 1)
    ux, uy = (V[:, 1:] * Co) * dt, (V[:, 1:] * So) * dt
    hlo, hwo = f32(0.5) * LN[:, 1:] + margin, f32(0.5) * WD[:, 1:] + margin
    po = pres[:, 1:]
    # waypoints
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
    gain, sv = np.zeros((E, nc), f32), np.zeros((E, nc), f32)
    a1 = np.where(v + a * dt < f32(0), f32(0), a).astype(f32)
    alive = np.ones((E, nc), bool)
    f = np.full((E, nc), H + 1, np.int64)
    lights_on = bool(cfg.flags & _abi.F_TRAFFIC_LIGHTS)
    for h in range(1, H + 1):
        if not alive.any():
            break
        ah = np.where(v + a * dt < f32(0), f32(0), a).astype(f32)
        k = np.flatnonzero(alive.ravel())
        xs, ys, ps, vs = (np.ascontiguousarray(q.ravel()[k]) for q in (x, y, psi, v))
        oracle.kinematics_step(xs, ys, ps, vs, np.ascontiguousarray(lr0.ravel()[k]), np.ones(len(k), np.uint8),
                               np.ascontiguousarray(np.stack([ah.ravel()[k], d.ravel()[k]], -1)), float(dt))
        for q, qs in ((x, xs), (y, ys), (psi, ps), (v, vs)):
            q.ravel()[k] = qs                                          # (x .. v are contiguous: ravel is a view)
        sn, cs = oracle.sincosf(psi.ravel())
        sn, cs = sn.reshape(E, nc), cs.reshape(E, nc)
        fail = np.zeros((E, nc), bool)
        fail.ravel()[k] = box_offroad(cfg, world, mapc.ravel()[k], xs, ys, ps, len0.ravel()[k], wid0.ravel()[k])
        # (ii) predicted boxes
        fh = f32(h)
        bx, by = X[:, 1:] + fh * ux, Y[:, 1:] + fh * uy
        hit = obb_overlap(x[:, :, None], y[:, :, None], cs[:, :, None], sn[:, :, None], hl0[:, :, None], hw0[:, :, None],
                          bx[:, None, :], by[:, None, :], Co[:, None, :], So[:, None, :], hlo[:, None, :], hwo[:, None, :])
        fail |= (hit & po[:, None, :]).any(2)
        # (iii) red lines
        if lights_on:
            fail |= red_hits(world, maps, steps, h, x, y, cs, sn, hl0, hw0)
        died = alive & fail
        f[died] = h
        alive &= ~fail
        # cost terms of the candidates still alive
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
    run = (ws_ * sv + wd_ * (d * d)) - wp_ * gain
    cost = ((H + 1 - f).astype(f32) * f32(_abi.PLAN_FAIL_UNIT) +
            np.fmin(np.fmax(run + f32(_abi.PLAN_RUN_BIAS), f32(0)), f32(_abi.PLAN_RUN_MAX))).astype(f32)
    key = (ordered(cost.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | ci[None].astype(np.uint64)
    win = key.argmin(1)
    r = np.arange(E)
    act[envs, 0], act[envs, 1] = a1[r, win], d[r, win]
    dg["winner"][envs], dg["fail_step"][envs], dg["cost"][envs] = win, f[r, win], cost[r, win]
    dg["n_safe"][envs] = (f == H + 1).sum(1)
    return (act, dg, f, cost) if detail else (act, dg)
