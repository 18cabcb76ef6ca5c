"""float32 numpy statement of the MOTION half of tde_env_step_driven (include/tde_driven.h), the checker of the driven-step tests: test
infrastructure only, nothing in the package imports it.  One step of every slot from a host state: the controller of
tests/forecast_scene_ref.py (its leader rule, the oracle's sincosf and bicycle, red_mask - imported, not restated) with the header's
one difference: a present slot a >= 1 with driven[e, a] != 0 integrates agent_action[e, a], at every step count and with or without
TDE_F_NPC, and is not pulled to its replay record; its route bookkeeping stays an NPC's.  Judges, reward and re-spawn are not here:
the tests take them from the oracle's operators on the poses this module returns."""
import numpy as np

from oracle import oracle
from tests.forecast_ref import FAR, _clamp
from tests.forecast_scene_ref import leader_gap
from tests.vector_obs_ref import red_mask
from torchdriveenv_amd import _abi

f32 = np.float32


def _scene(cfg, world, hs):
    """the columns of the state and the table entries of every slot, flat [B * A]"""
    B, A = len(hs["scn"]), world.A
    F = int(cfg.flags)
    s = dict(B=B, A=A, n=B * A, npc_on=bool(F & _abi.F_NPC), replay_on=bool(F & _abi.F_REPLAY),
             first_step=bool(F & _abi.F_NPC_FIRST_STEP), lights_on=bool(F & _abi.F_TRAFFIC_LIGHTS))
    for k in ("x", "y", "psi", "v", "len", "wid", "lr", "vdes"):
        s[k] = np.array(hs[k], f32).ravel()
    s["wp"] = np.array(hs["route_wp"], np.int64).ravel()
    s["slot"] = np.tile(np.arange(A), B)
    s["live"] = np.asarray(hs["present"]).ravel() != 0
    s["other"] = s["live"] & (s["slot"] > 0)
    s["scn"] = np.repeat(np.asarray(hs["scn"]).astype(np.int64), A)
    s["k"] = np.repeat(np.asarray(hs["steps"]).astype(np.int64), A) + 1
    rec = world.arrays["spawn"].reshape(-1, A)[s["scn"], s["slot"]]
    none = np.full(s["n"], -1, np.int64)
    s["route"] = np.where(s["slot"] > 0, rec["route"].astype(np.int64), none) if s["npc_on"] else none
    s["route_n"] = rec["route_n"].astype(np.int64) if s["npc_on"] else np.zeros(s["n"], np.int64)
    s["replay"] = np.where(s["slot"] > 0, rec["replay"].astype(np.int64), none) if s["replay_on"] else none
    s["replay_len"] = rec["replay_len"].astype(np.int64) if s["replay_on"] else np.zeros(s["n"], np.int64)
    route_xy = world.arrays["route_xy"].reshape(-1, max(world.ints["RW"], 1), 2)
    s["has"] = s["other"] & s["npc_on"] & (s["route"] >= 0) & (s["wp"] < s["route_n"])
    s["tx"], s["ty"] = np.zeros(s["n"], f32), np.zeros(s["n"], f32)
    i = np.flatnonzero(s["has"])
    s["tx"][i], s["ty"][i] = route_xy[s["route"][i], s["wp"][i], 0], route_xy[s["route"][i], s["wp"][i], 1]
    return s


def _controller(cfg, world, s):
    """(acc, beta) float32 [B * A] the step applies to every slot when nobody is driven; the ego's entries are zero"""
    n, B, A = s["n"], s["B"], s["A"]
    acc, beta = np.zeros(n, f32), np.zeros(n, f32)
    if not s["npc_on"]:
        return acc, beta
    amax, smax = f32(cfg.npc_max_accel), f32(cfg.npc_max_steer)
    k_speed, k_steer, s0g = f32(cfg.npc_k_speed), f32(cfg.npc_k_steer), f32(cfg.npc_gap_s0)
    x, y, v, ln, k, has = s["x"], s["y"], s["v"], s["len"], s["k"], s["has"]
    sp, cp = oracle.sincosf(s["psi"])
    ctrl = s["other"] & ((k > 1) | s["first_step"])
    red_gap = np.full(n, FAR, f32)
    if s["lights_on"]:
        maps = world.arrays["scn"]["map"][s["scn"]].astype(np.int64)
        mp, stop = world.arrays["maps"], world.arrays["stoplines"]
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
    sq = lambda a: a.reshape(B, A)                                               # noqa: E731
    lead = leader_gap(cfg, sq(x), sq(y), sq(cp), sq(sp), sq(f32(0.5) * ln), sq(f32(0.5) * s["wid"]), sq(s["live"])).ravel()
    with np.errstate(all="ignore"):
        a_stop = _clamp(k_speed * (f32(0.0) - v), -amax, amax)
        dx, dy = s["tx"] - x, s["ty"] - y
        fwd = dx * cp + dy * sp
        lat = dy * cp - dx * sp
        dist = np.sqrt(dx * dx + dy * dy)
        sin_err = lat / np.fmax(dist, f32(1e-3))
        b_t = np.where(fwd < f32(0), np.copysign(smax, lat), _clamp(k_steer * sin_err, -smax, smax)).astype(f32)
        gap = np.fmin(lead, red_gap)
        vd = np.fmin(s["vdes"], np.sqrt(amax * np.fmax(gap - s0g, f32(0.0))))
        a_t = _clamp(k_speed * (vd - v), -amax, amax)
    acc = np.where(ctrl, np.where(has, a_t, a_stop), f32(0)).astype(f32)
    beta = np.where(ctrl & has, b_t, f32(0)).astype(f32)
    return acc, beta


def npc_actions(cfg, world, hs):
    """float32 [B, A, 2]: the (acceleration, steering) the next step's controller applies to every slot of the host state `hs` - what
    an echo hands back; zero for slot 0, for absent slots and where the controller does not act (k == 1 without NPC_FIRST_STEP)"""
    s = _scene(cfg, world, hs)
    acc, beta = _controller(cfg, world, s)
    return np.ascontiguousarray(np.stack([acc, beta], -1).reshape(s["B"], s["A"], 2))


def step_motion(cfg, world, hs, agent_action=None, driven=None):
    """one step of every slot of `hs` (not modified; the ego takes hs["action"]) -> dict of x, y, psi, v (float32) and route_wp (int32),
    flat [B * A], as the step leaves them BEFORE any re-spawn; the rows of absent slots are those of `hs`"""
    s = _scene(cfg, world, hs)
    n, B, A = s["n"], s["B"], s["A"]
    acc, beta = _controller(cfg, world, s)
    ego = np.flatnonzero(s["slot"] == 0)
    act = np.asarray(hs["action"], f32).reshape(B, 2)
    acc[ego], beta[ego] = act[:, 0], act[:, 1]
    drv = np.zeros(n, bool)
    if driven is not None:
        drv = s["other"] & (np.asarray(driven).reshape(n) != 0)
        aa = np.asarray(agent_action, f32).reshape(n, 2)
        acc[drv], beta[drv] = aa[drv, 0], aa[drv, 1]
    x, y, psi, v = (s[k].copy() for k in ("x", "y", "psi", "v"))
    oracle.kinematics_step(x, y, psi, v, s["lr"], s["live"].astype(np.uint8), np.ascontiguousarray(np.stack([acc, beta], -1)), float(f32(cfg.dt)))
    replay_states = world.arrays["replay_states"].reshape(-1, max(world.ints["RT"], 1), 4)
    i = np.flatnonzero(s["other"] & ~drv & (s["replay"] >= 0) & (s["k"] < s["replay_len"]))
    if len(i):
        r = replay_states[s["replay"][i], s["k"][i]]
        x[i], y[i], psi[i], v[i] = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    reach = f32(cfg.npc_reach)
    dx, dy = s["tx"] - x, s["ty"] - y
    adv = s["has"] & (dx * dx + dy * dy < reach * reach)
    return dict(x=x, y=y, psi=psi, v=v, route_wp=(s["wp"] + adv).astype(np.int32), driven=drv)
