"""float32 numpy restatement of tde_forecast_scene (include/tde_hip.h), the checker of the scene-forecast tests: test infrastructure only,
nothing in the package imports it.  Written like tests/forecast_ref.py, whose pieces it shares (the oracle's sincosf and bicycle, red_mask):
every expression is the header's, in float32.  The leader rule is the header's predicates in a plain loop over the slots j of the env -
no prefilter, no candidate masks: an independent statement of what the kernel's sweep has to find."""
import numpy as np

from oracle import oracle
from tests.forecast_ref import FAR, _clamp
from tests.vector_obs_ref import red_mask
from torchdriveenv_amd import _abi

f32 = np.float32


def leader_gap(cfg, X, Y, C_, S_, HL, HW, present):
    """[E, A] arrays of the pre-step scene -> lead [E, A]: the least g over the taken slots j of each slot i's env (FAR: none)"""
    E, A = X.shape
    lane_half, cone_k, cone_range = f32(cfg.npc_lane_half), f32(cfg.npc_cone_k), f32(cfg.npc_cone_range)
    i = np.arange(A)[None, :]
    lead = np.full((E, A), FAR, f32)
    with np.errstate(all="ignore"):
        for j in range(A):
            xj, yj, cj, sj, hlj, hwj = (a[:, j:j + 1] for a in (X, Y, C_, S_, HL, HW))
            ex, ey = xj - X, yj - Y
            fj = ex * C_ + ey * S_
            lj = ey * C_ - ex * S_
            al = np.abs(lj)
            halfw = lane_half + hwj
            hd = C_ * cj + S_ * sj
            g = fj - (HL + hlj)
            inlane = al < halfw
            cone = (j < i) & (fj < cone_range) & (al < halfw + cone_k * fj) & (hd > f32(-0.5))
            taken = present[:, j:j + 1] & (i != j) & (fj > f32(0.0)) & (inlane | cone)
            lead = np.where(taken, np.fmin(lead, g), lead).astype(f32)
    return lead


def forecast_scene(cfg, world, hs, T, ego_action=None, only=None, out=None):
    """what tde_forecast_scene writes: float32 [B, T, A, 4], row 0 the ego's; rows of envs with only[e] == 0 are those of `out` (zeros
    without it).  ego_action: float32 [B, T, 2] or None (the ego coasts)"""
    st = hs
    B, A = len(st["scn"]), world.A
    T = int(T)
    res = np.zeros((B, T, A, 4), f32) if out is None else np.array(out, f32, copy=True).reshape(B, T, A, 4)
    envs = np.array([e for e in range(B) if only is None or only[e]], np.int64)
    E = len(envs)
    if E == 0:
        return res
    act = np.zeros((E, T, 2), f32) if ego_action is None else np.asarray(ego_action, f32).reshape(B, T, 2)[envs]
    F = int(cfg.flags)
    npc_on, replay_on = bool(F & _abi.F_NPC), bool(F & _abi.F_REPLAY)
    first_step, lights_on = bool(F & _abi.F_NPC_FIRST_STEP), bool(F & _abi.F_TRAFFIC_LIGHTS)
    dt = f32(cfg.dt)
    amax, smax = f32(cfg.npc_max_accel), f32(cfg.npc_max_steer)
    k_speed, k_steer, s0g, reach = f32(cfg.npc_k_speed), f32(cfg.npc_k_steer), f32(cfg.npc_gap_s0), f32(cfg.npc_reach)
    col = lambda n, t: np.asarray(st[n]).reshape(B, A)[envs].astype(t).ravel()   # noqa: E731
    x, y, psi, v, ln, wd, lr, vdes = (col(n, f32) for n in ("x", "y", "psi", "v", "len", "wid", "lr", "vdes"))
    hl, hw = f32(0.5) * ln, f32(0.5) * wd
    wp = col("route_wp", np.int64)
    slot = np.tile(np.arange(A), E)
    live = col("present", np.int64) != 0
    other = live & (slot > 0)
    scn = np.repeat(np.asarray(st["scn"])[envs].astype(np.int64), A)
    steps = np.repeat(np.asarray(st["steps"])[envs].astype(np.int64), A)
    rec = world.arrays["spawn"].reshape(-1, A)[scn, slot]
    n = E * A
    none = np.full(n, -1, np.int64)
    route = np.where(slot > 0, rec["route"].astype(np.int64), none) if npc_on else none
    route_n = rec["route_n"].astype(np.int64) if npc_on else np.zeros(n, np.int64)
    replay = np.where(slot > 0, rec["replay"].astype(np.int64), none) if replay_on else none
    replay_len = rec["replay_len"].astype(np.int64) if replay_on else np.zeros(n, np.int64)
    route_xy = world.arrays["route_xy"].reshape(-1, max(world.ints["RW"], 1), 2)
    replay_states = world.arrays["replay_states"].reshape(-1, max(world.ints["RT"], 1), 4)
    maps = world.arrays["scn"]["map"][scn].astype(np.int64)
    mp, stop = world.arrays["maps"], world.arrays["stoplines"]
    tx, ty = np.zeros(n, f32), np.zeros(n, f32)

    def load_target(mask):
        i = np.flatnonzero(mask & (route >= 0) & (wp < route_n))
        tx[i], ty[i] = route_xy[route[i], wp[i], 0], route_xy[route[i], wp[i], 1]

    load_target(other)
    pres = live.astype(np.uint8)
    sq = lambda a: a.reshape(E, A)                                               # noqa: E731
    for h in range(1, T + 1):
        k = steps + h
        sp, cp = oracle.sincosf(psi)
        has = other & npc_on & (route >= 0) & (wp < route_n)
        acc, beta = np.zeros(n, f32), np.zeros(n, f32)
        if npc_on:
            ctrl = other & ((k > 1) | first_step)
            red_gap = np.full(n, FAR, f32)
            if lights_on:
                for m in np.unique(maps[has]):
                    if int(mp["n_stop"][m]) <= 0:
                        continue
                    mine = has & (maps == m)
                    red = np.zeros(n, np.int64)
                    for kk in np.unique(k[mine]):
                        red[mine & (k == kk)] = red_mask(world, m, kk)
                    for q in stop[int(mp["stop_base"][m]):int(mp["stop_base"][m]) + int(mp["n_stop"][m])]:
                        ex, ey = q["x"] - x, q["y"] - y
                        fj = ex * cp + ey * sp
                        lj = ey * cp - ex * sp
                        hd = cp * q["c"] + sp * q["s"]
                        g = fj - f32(0.5) * ln
                        on = mine & (((red >> int(q["light"])) & 1) != 0) & (g > f32(0)) & (np.abs(lj) < q["hw"]) & (hd > f32(0.5))
                        red_gap = np.where(on, np.fmin(red_gap, g + s0g - f32(1.0)), red_gap).astype(f32)
            lead = leader_gap(cfg, sq(x), sq(y), sq(cp), sq(sp), sq(hl), sq(hw), sq(live)).ravel()
            with np.errstate(all="ignore"):
                a_stop = _clamp(k_speed * (f32(0.0) - v), -amax, amax)
                dx, dy = tx - x, ty - y
                fwd = dx * cp + dy * sp
                lat = dy * cp - dx * sp
                dist = np.sqrt(dx * dx + dy * dy)
                sin_err = lat / np.fmax(dist, f32(1e-3))
                b_t = np.where(fwd < f32(0), np.copysign(smax, lat), _clamp(k_steer * sin_err, -smax, smax)).astype(f32)
                gap = np.fmin(lead, red_gap)
                vd = np.fmin(vdes, np.sqrt(amax * np.fmax(gap - s0g, f32(0.0))))
                a_t = _clamp(k_speed * (vd - v), -amax, amax)
            acc = np.where(ctrl, np.where(has, a_t, a_stop), f32(0)).astype(f32)
            beta = np.where(ctrl & has, b_t, f32(0)).astype(f32)
        ego = np.flatnonzero(slot == 0)
        acc[ego], beta[ego] = act[:, h - 1, 0], act[:, h - 1, 1]
        oracle.kinematics_step(x, y, psi, v, lr, pres, np.ascontiguousarray(np.stack([acc, beta], -1)), float(dt))
        i = np.flatnonzero(other & (replay >= 0) & (k < replay_len))
        if len(i):
            r = replay_states[replay[i], k[i]]
            x[i], y[i], psi[i], v[i] = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
        dx, dy = tx - x, ty - y
        adv = has & (dx * dx + dy * dy < reach * reach)
        wp = wp + adv
        load_target(adv)
        row = np.where(live[:, None], np.stack([x, y, psi, v], -1), f32(0)).astype(f32)
        res[envs, h - 1] = row.reshape(E, A, 4)
    return res


def plan_queued(cfg, world, hs, pl, tail=0, only=None, out=None, diag=None):
    """BatchedWaypointEnv.plan_actions() under Planner(predict="queue") without refinement rounds -> (action [B, 2], diag [B]): the
    lattice as one-knot sequences judged on tde_forecast_scene's rows of horizon + tail steps with the ego coasting"""
    from tests.plan_set_ref import lattice, score

    B = len(hs["scn"])
    lat = lattice(pl)
    seq = np.ascontiguousarray(np.broadcast_to(lat[None, :, None, :], (B, len(lat), 1, 2)))
    fc = forecast_scene(cfg, world, hs, int(pl.horizon) + int(tail), only=only)
    res = score(cfg, world, hs, pl, seq, int(pl.horizon), tail, only=only, out=out, diag=diag, forecast=fc)
    return res["action"], res["diag"]
