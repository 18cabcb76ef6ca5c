"""float32 numpy restatement of tde_forecast_agents (include/tde_hip.h), the checker of the forecast tests: test infrastructure only,
nothing in the package imports it.  Written like tests/planner_ref.py and tests/plan_set_ref.py (red_mask; the oracle's sincosf and
bicycle): every expression is the header's, in float32.  tde_score_plans_forecast is restated by plan_set_ref.score(forecast=): the one
judge, given these rows (forecast, constant_velocity) for the others' boxes; plan_routed puts the two together.  Also the hand-made world of the environment-as-oracle tests (oracle_world), shared by the CPU and GPU tests."""
import numpy as np

from oracle import oracle
from tests.vector_obs_ref import red_mask
from torchdriveenv_amd import _abi

f32 = np.float32
FAR = f32(1e30)                                   # what the leader sweep returns when it takes no slot (tde_kernels.h: npc_gap)


def _clamp(u, lo, hi):
    return np.fmin(np.fmax(u, lo), hi).astype(f32)


def forecast(cfg, world, st, T, only=None, out=None):
    """what tde_forecast_agents writes: float32 [B, T, A, 4]; rows of envs with only[e] == 0 are those of `out` (zeros without it)"""
    B, A = len(st["scn"]), world.A
    T = int(T)
    res = np.zeros((B, T, A, 4), f32) if out is None else np.array(out, f32, copy=True).reshape(B, T, A, 4)
    envs = np.array([e for e in range(B) if only is None or only[e]], np.int64)
    E = len(envs)
    if E == 0:
        return res
    F = int(cfg.flags)
    npc_on, replay_on = bool(F & _abi.F_NPC), bool(F & _abi.F_REPLAY)
    first_step, lights_on = bool(F & _abi.F_NPC_FIRST_STEP), bool(F & _abi.F_TRAFFIC_LIGHTS)
    dt = f32(cfg.dt)
    amax, smax = f32(cfg.npc_max_accel), f32(cfg.npc_max_steer)
    k_speed, k_steer, s0g, reach = f32(cfg.npc_k_speed), f32(cfg.npc_k_steer), f32(cfg.npc_gap_s0), f32(cfg.npc_reach)
    col = lambda n, t: np.asarray(st[n]).reshape(B, A)[envs].astype(t).ravel()   # noqa: E731
    x, y, psi, v, ln, lr, vdes = (col(n, f32) for n in ("x", "y", "psi", "v", "len", "lr", "vdes"))
    wp = col("route_wp", np.int64)
    slot = np.tile(np.arange(A), E)
    live = (col("present", np.int64) != 0) & (slot > 0)
    scn = np.repeat(np.asarray(st["scn"])[envs].astype(np.int64), A)
    steps = np.repeat(np.asarray(st["steps"])[envs].astype(np.int64), A)
    rec = world.arrays["spawn"].reshape(-1, A)[scn, slot]
    n = E * A
    route = rec["route"].astype(np.int64) if npc_on else np.full(n, -1, np.int64)
    route_n = rec["route_n"].astype(np.int64) if npc_on else np.zeros(n, np.int64)
    replay = rec["replay"].astype(np.int64) if replay_on else np.full(n, -1, np.int64)
    replay_len = rec["replay_len"].astype(np.int64) if replay_on else np.zeros(n, np.int64)
    route_xy = world.arrays["route_xy"].reshape(-1, max(world.ints["RW"], 1), 2)
    replay_states = world.arrays["replay_states"].reshape(-1, max(world.ints["RT"], 1), 4)
    maps = world.arrays["scn"]["map"][scn].astype(np.int64)
    mp, stop = world.arrays["maps"], world.arrays["stoplines"]
    tx, ty = np.zeros(n, f32), np.zeros(n, f32)

    def load_target(mask):
        i = np.flatnonzero(mask & (route >= 0) & (wp < route_n))
        tx[i], ty[i] = route_xy[route[i], wp[i], 0], route_xy[route[i], wp[i], 1]

    load_target(live)
    pres = live.astype(np.uint8)
    for h in range(1, T + 1):
        k = steps + h
        sp, cp = oracle.sincosf(psi)
        has = live & npc_on & (route >= 0) & (wp < route_n)
        acc, beta = np.zeros(n, f32), np.zeros(n, f32)
        if npc_on:
            ctrl = live & ((k > 1) | first_step)
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
            a_stop = _clamp(k_speed * (f32(0.0) - v), -amax, amax)
            dx, dy = tx - x, ty - y
            fwd = dx * cp + dy * sp
            lat = dy * cp - dx * sp
            dist = np.sqrt(dx * dx + dy * dy)
            sin_err = lat / np.fmax(dist, f32(1e-3))
            b_t = np.where(fwd < f32(0), np.copysign(smax, lat), _clamp(k_steer * sin_err, -smax, smax)).astype(f32)
            gap = np.fmin(FAR, red_gap)
            vd = np.fmin(vdes, np.sqrt(amax * np.fmax(gap - s0g, f32(0.0))))
            a_t = _clamp(k_speed * (vd - v), -amax, amax)
            acc = np.where(ctrl, np.where(has, a_t, a_stop), f32(0)).astype(f32)
            beta = np.where(ctrl & has, b_t, f32(0)).astype(f32)
        oracle.kinematics_step(x, y, psi, v, lr, pres, np.ascontiguousarray(np.stack([acc, beta], -1)), float(dt))
        i = np.flatnonzero(live & (replay >= 0) & (k < replay_len))
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


def constant_velocity(cfg, world, st, T):
    """the forecast that makes tde_score_plans_forecast equal tde_score_plans: float32 [B, T, A, 4] rows (x_j + (float)h * ((v_j * c_j)
    * dt), y_j + (float)h * ((v_j * s_j) * dt), psi_j, v_j) with (s_j, c_j) = sincos_f32(psi_j)"""
    B, A = len(st["scn"]), world.A
    X, Y, P, V = (np.asarray(st[n], f32).reshape(B, A) for n in ("x", "y", "psi", "v"))
    S, Cc = oracle.sincosf(P.ravel())
    S, Cc = S.reshape(B, A), Cc.reshape(B, A)
    dt = f32(cfg.dt)
    ux, uy = (V * Cc) * dt, (V * S) * dt
    out = np.zeros((B, T, A, 4), f32)
    for h in range(1, T + 1):
        out[:, h - 1, :, 0], out[:, h - 1, :, 1] = X + f32(h) * ux, Y + f32(h) * uy
        out[:, h - 1, :, 2], out[:, h - 1, :, 3] = P, V
    return out


def plan_routed(cfg, world, st, pl, tail=0, only=None, out=None, diag=None):
    """BatchedWaypointEnv.plan_actions() under Planner(predict="route") without refinement rounds -> (action [B, 2], diag [B]): the
    lattice as one-knot sequences judged on tde_forecast_agents' rows of horizon + tail steps"""
    from tests.plan_set_ref import lattice, score

    B = len(st["scn"])
    lat = lattice(pl)
    seq = np.ascontiguousarray(np.broadcast_to(lat[None, :, None, :], (B, len(lat), 1, 2)))
    fc = forecast(cfg, world, st, int(pl.horizon) + int(tail), only=only)
    res = score(cfg, world, st, pl, seq, int(pl.horizon), tail, only=only, out=out, diag=diag, forecast=fc)
    return res["action"], res["diag"]


# ---- the hand-made world of the environment-as-oracle tests ------------------------------------------------------------------------------

ORACLE_STEPS = 32
ORACLE_B = 8
STOP_X = 75.0
LANE_GAP = 40.0          # metres between the four parallel roads: the controller's cone reaches npc_cone_k * npc_cone_range + npc_lane_half
                         # + half a width = 15.3 m sideways at most, so no agent ever has another in its cone or lane


def oracle_world(red_steps=14):
    """(cfg, world): one mesh of four parallel 400 m roads LANE_GAP apart, four scenarios, each the ego on road 0 plus three NPCs, one
    per road: slot 1 eastbound on a route that drifts half a metre sideways (it steers), slot 2 westbound (scenario 1: on a short
    route it finishes inside the run, so it brakes to rest; scenario 2: no route at all), slot 3 replayed for its first 10 steps and
    on a route after that.  Scenario 3 sees a stop line across road 1 (centre at x = STOP_X) that is red for the first `red_steps` steps of
    an episode."""
    from torchdriveenv_amd.world import assemble_world, corridor_mesh

    ys = [0.0, LANE_GAP, 2 * LANE_GAP, 3 * LANE_GAP]
    mesh = corridor_mesh([[(0.0, yy), (400.0, yy)] for yy in ys], width=10.0)
    attr = (4.6, 1.9, 1.4)

    def line(x0, x1, yy, step, drift=0.0):
        n = int(abs(x1 - x0) / step)
        sgn = 1.0 if x1 > x0 else -1.0
        return [(x0 + sgn * step * (i + 1), yy + drift * ((i % 3) - 1)) for i in range(n)]

    def replay_rows(x0, yy, v0):
        rows, xx = [], x0
        for k in range(11):                        # records 0 .. 10: the step takes record k at step k < 11
            rows.append((xx, yy + 0.02 * k, 0.01 * k, v0 + 0.1 * k))
            xx += (v0 + 0.1 * k) * 0.1
        return rows

    scns = []
    for s in range(4):
        a1 = dict(state=(30.0 + 5.0 * s, ys[1], 0.0, 6.0), attr=attr, vdes=8.0 + s, route=line(30.0 + 5.0 * s, 330.0, ys[1], 12.0, 0.5), replay=None)
        r2 = None if s == 2 else line(300.0, 290.0 if s == 1 else 60.0, ys[2], 5.0 if s == 1 else 15.0)
        a2 = dict(state=(300.0, ys[2] + 0.3, np.pi, 5.0 + s), attr=attr, vdes=7.0, route=r2, replay=None)
        a3 = dict(state=(50.0, ys[3], 0.0, 4.0), attr=attr, vdes=9.0, route=line(60.0, 360.0, ys[3], 20.0), replay=replay_rows(50.0, ys[3], 4.0))
        sc = dict(map=0, waypoints=[(20.0, 0.0), (60.0, 0.0), (200.0, 0.0), (380.0, 0.0)], start_heading=0.0, agents=[a1, a2, a3], ego_attr=attr)
        if s == 3:
            sc["lights"] = 0
        scns.append(sc)
    groups = [dict(map=0, stoplines=[(STOP_X, ys[1], 0.0, 1.0, 8.0, 0)], phases=[(int(red_steps), [0]), (200, [])])]
    world = assemble_world([mesh], scns, 4, threshold=0.5, cell=0.5, light_groups=groups)
    cfg = _abi.default_config(seed=11, terminated_at_infraction=0, max_steps=200)
    cfg.flags = (_abi.F_ALL & ~_abi.F_AUTORESET) | _abi.F_TRAFFIC_LIGHTS
    return cfg, world
