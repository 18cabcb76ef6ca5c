"""numpy restatement of tde_agent_obs and tde_agent_outcomes (include/tde_agents.h), the checker of the agents tests: test infrastructure
only, nothing in the package imports it.  agent_obs is tests/vector_obs_ref.py's statement with the pair's slot as the observer - every
expression float32, one rounding per operation; the slab test, the road predicate and the light phases are imported from there, not
restated (the road predicate is handed the triangles near each observer only: road_off_near).  agent_outcomes forms the reward as the reference's Python does: float64 on the float32 state, math.cos and the square root."""
import math

import numpy as np

from oracle import oracle
from tests.vector_obs_ref import _road_off, entry_distance, red_mask
from torchdriveenv_amd import _abi

f32 = np.float32
TRACK = np.dtype([("x", f32), ("y", f32), ("psi", f32), ("v", f32), ("route_wp", np.int32), ("episode", np.int32), ("steps", np.int32),
                  ("present", np.uint32)])
assert TRACK.itemsize == 32


class _NearWorld:
    """the world with one map per observer that holds only the triangles near it (host_struct() for the oracle's operators)"""

    def __init__(self, world, maps, tri):
        self.arrays = dict(world.arrays, maps=maps, tri=np.ascontiguousarray(tri, f32))
        self.ints = dict(world.ints, n_maps=len(maps))
        self._struct = _abi.fill_world_struct(self.arrays, self.ints)

    def host_struct(self):
        return self._struct


def road_off_near(cfg, world, groups):
    """vector_obs_ref._road_off for the samples of several observers - groups of (map, x0, y0, px, py) whose samples lie within `reach`
    = max |p - (x0, y0)| of their observer - with the oracle's brute force run over the triangles near each observer only: a triangle
    whose bounding box is farther than reach + threshold + 1 m from (x0, y0) is farther than the threshold from every sample, so leaving
    it out changes no truth value (the same operator on fewer triangles; a town mesh has 15 000 of them).  -> bool, concatenated"""
    if not groups:
        return np.zeros(0, bool)
    if cfg.offroad_threshold_squared:
        return _road_off(cfg, world, np.concatenate([np.full(g[3].size, g[0], np.int32) for g in groups]),
                         np.concatenate([g[3].ravel() for g in groups]), np.concatenate([g[4].ravel() for g in groups]))
    tri, mp = world.arrays["tri"].reshape(-1, 6), world.arrays["maps"]
    maps = np.zeros(len(groups), mp.dtype)
    kept, base = [], 0
    for i, (m, x0, y0, px, py) in enumerate(groups):
        t = tri[int(mp[m]["tri_base"]):int(mp[m]["tri_base"]) + int(mp[m]["n_tri"])]
        reach = float(np.max(np.hypot(px.astype(np.float64) - float(x0), py.astype(np.float64) - float(y0)))) if px.size else 0.0
        gx = np.maximum(np.maximum(t[:, 0::2].min(1) - x0, x0 - t[:, 0::2].max(1)), 0).astype(np.float64)
        gy = np.maximum(np.maximum(t[:, 1::2].min(1) - y0, y0 - t[:, 1::2].max(1)), 0).astype(np.float64)
        near = t[np.hypot(gx, gy) <= reach + float(cfg.offroad_threshold) + 1.0]
        maps[i] = mp[m]
        maps[i]["tri_base"], maps[i]["n_tri"] = base, len(near)
        kept.append(near)
        base += len(near)
    kept.append(np.zeros((1, 6), f32))                                    # (never an empty table)
    sub = _NearWorld(world, maps, np.concatenate(kept))
    idx = np.concatenate([np.full(g[3].size, i, np.int32) for i, g in enumerate(groups)])
    return _road_off(cfg, sub, idx, np.concatenate([g[3].ravel() for g in groups]), np.concatenate([g[4].ravel() for g in groups]))


def slot_route_of(world, st, e, a):
    """(route, route_n) of slot a >= 1 of env e: the slot_route word when the state has the array and the word is not 0, else the spawn
    record's; route < 0 or past the table: no route"""
    A = world.A
    sr = st["slot_route"] if "slot_route" in st else None
    word = 0 if sr is None else int(np.asarray(sr).reshape(-1)[e * A + a])
    if word:
        route, n = (word & 0xFFFFF) - 1, word >> 20
    else:
        rec = world.arrays["spawn"].reshape(-1, A)[int(st["scn"][e]), a]
        route, n = int(rec["route"]), int(rec["route_n"])
    if route < 0 or route >= int(world.ints["n_routes"]):
        return -1, 0
    return route, n


def agent_obs(cfg, world, st, vo, pairs):
    """(rows float32 [n, D], track TRACK [n]) of tde_agent_obs for the (env, slot) rows of `pairs` on the host state `st`"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    B, A = len(st["scn"]), world.A
    k, nr = int(vo.k_neighbours), int(vo.n_rays)
    D = vo.dim
    res = np.zeros((len(pairs), D), f32)
    track = np.zeros(len(pairs), TRACK)
    L, h, r = f32(vo.ray_range), f32(vo.ray_step), f32(vo.neighbour_radius)
    M = int(L / h)
    rd = vo.ray_directions()
    x, y, psi, v = (np.asarray(st[n], f32).reshape(B, A) for n in ("x", "y", "psi", "v"))
    ln, wd = np.asarray(st["len"], f32).reshape(B, A), np.asarray(st["wid"], f32).reshape(B, A)
    pres = np.asarray(st["present"]).reshape(B, A) != 0
    route_wp = np.asarray(st["route_wp"]).reshape(B, A)
    S, C = oracle.sincosf(psi.ravel())
    S, C = S.reshape(B, A), C.reshape(B, A)
    scn, mp, wp = world.arrays["scn"], world.arrays["maps"], world.arrays["wp_xy"].reshape(-1, world.ints["NW"], 2)
    route_xy = world.arrays["route_xy"].reshape(-1, max(world.ints["RW"], 1), 2)
    stop = world.arrays["stoplines"]
    lights_on = bool(cfg.flags & _abi.F_TRAFFIC_LIGHTS)
    road_pts = []                                     # (row, map, x0, y0, px [nr, M], py [nr, M])
    for i, (e, a) in enumerate(pairs):
        if not (0 <= e < B and 0 <= a < A) or not pres[e, a]:
            continue
        s = int(st["scn"][e])
        m = int(scn[s]["map"])
        steps = int(st["steps"][e])
        x0, y0, v0, s0, c0 = x[e, a], y[e, a], v[e, a], S[e, a], C[e, a]
        track[i] = (x0, y0, psi[e, a], v0, route_wp[e, a], st["episode"][e], steps, 1)
        row = np.zeros(D, f32)
        row[0], row[1], row[2] = v0, ln[e, a], wd[e, a]
        if a == 0:
            n_wp, ti = int(scn[s]["wp_n"]), int(st["target_idx"][e])
            pts = [(f32(wp[s, j, 0]), f32(wp[s, j, 1])) if j < n_wp else None for j in (ti, ti + 1)]
        else:
            route, n_wp = slot_route_of(world, st, e, a)
            ti = int(route_wp[e, a]) if route >= 0 else 0
            pts = [(route_xy[route, j, 0], route_xy[route, j, 1]) if 0 <= j < n_wp else None for j in (ti, ti + 1)]
        for q, p in enumerate(pts):
            if p is not None:
                dx, dy = p[0] - x0, p[1] - y0
                row[3 + 2 * q], row[4 + 2 * q] = dx * c0 + dy * s0, dy * c0 - dx * s0
        row[7] = f32(min(max(n_wp - ti, 0), 2))
        row[8] = f32(steps) / f32(cfg.max_steps)
        row[9] = f32(1.0 if int(mp[m]["n_stop"]) > 0 and int(mp[m]["cycle_steps"]) > 0 else 0.0)
        # neighbours: the present slots other than the observer, the ego included
        others = np.flatnonzero(pres[e] & (np.arange(A) != a))
        dx, dy = x[e, others] - x0, y[e, others] - y0
        d2 = dx * dx + dy * dy
        cand = d2 < r * r
        oc, dxc, dyc, d2c = others[cand], dx[cand], dy[cand], d2[cand]
        order = np.lexsort((oc, d2c.view(np.uint32)))[:k]
        for q, j in enumerate(order):
            b = oc[j]
            cr = C[e, b] * c0 + S[e, b] * s0
            sr = S[e, b] * c0 - C[e, b] * s0
            row[10 + 9 * q:19 + 9 * q] = [f32(1), dxc[j] * c0 + dyc[j] * s0, dyc[j] * c0 - dxc[j] * s0, cr, sr, v[e, b] * cr - v0,
                                          v[e, b] * sr, ln[e, b], wd[e, b]]
        if nr:
            rx, ry = rd[:, 0], rd[:, 1]
            ux, uy = rx * c0 - ry * s0, rx * s0 + ry * c0
            r0 = 10 + 9 * k
            car = np.full(nr, L, f32)
            if len(others):
                t = entry_distance(x0, y0, ux[:, None], uy[:, None], x[e, others][None], y[e, others][None], C[e, others][None],
                                   S[e, others][None], (f32(0.5) * ln[e, others])[None], (f32(0.5) * wd[e, others])[None])
                car = np.minimum(car, t.min(1))
            red = np.full(nr, L, f32)
            n_stop = int(mp[m]["n_stop"])
            if lights_on and n_stop > 0:
                rm = red_mask(world, m, steps)
                lines = stop[int(mp[m]["stop_base"]):int(mp[m]["stop_base"]) + n_stop]
                lines = lines[((rm >> (lines["light"].astype(np.int64) & 31)) & 1) != 0]
                if len(lines):
                    t = entry_distance(x0, y0, ux[:, None], uy[:, None], lines["x"][None], lines["y"][None], lines["c"][None],
                                       lines["s"][None], lines["hl"][None], lines["hw"][None])
                    red = np.minimum(red, t.min(1))
            row[r0 + 1:r0 + 3 * nr:3] = car
            row[r0 + 2:r0 + 3 * nr:3] = red
            tj = np.arange(1, M + 1).astype(f32) * h                       # (float)j * ray_step
            road_pts.append((i, m, x0, y0, x0 + tj[None, :] * ux[:, None], y0 + tj[None, :] * uy[:, None]))
        res[i] = row
    if road_pts and nr:
        off = road_off_near(cfg, world, [p[1:] for p in road_pts]).reshape(len(road_pts), nr, M)
        tj = np.arange(1, M + 1).astype(f32) * h
        r0 = 10 + 9 * k
        for n, p in enumerate(road_pts):
            i = p[0]
            first = np.where(off[n].any(1), off[n].argmax(1), -1)
            res[i, r0:r0 + 3 * nr:3] = np.where(first >= 0, tj[np.maximum(first, 0)], L)
    return res, track


def agent_outcomes(cfg, world, st, pairs, track):
    """(reward float32 [n], flags uint8 [n]) of tde_agent_outcomes on the host state `st` for the tracks an earlier agent_obs returned"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    B, A = len(st["scn"]), world.A
    reward, flags = np.zeros(len(pairs), f32), np.zeros(len(pairs), np.uint8)
    for i, (e, a) in enumerate(pairs):
        tr = track[i]
        if not tr["present"] or not (0 <= e < B and 1 <= a < A):
            continue
        g = e * A + a
        if int(st["episode"][e]) != int(tr["episode"]) or not st["present"][g]:
            flags[i] = _abi.AG_VALID | _abi.AG_ENDED
            continue
        reach = int(st["route_wp"][g]) > int(tr["route_wp"])
        flags[i] = (_abi.AG_VALID | (_abi.AG_COLLIDED if st["collided"][g] else 0) | (_abi.AG_OFFROAD if st["offroad"][g] else 0)
                    | (_abi.AG_REACHED if reach else 0))
        ddx, ddy = float(st["x"][g]) - float(tr["x"]), float(st["y"][g]) - float(tr["y"])
        dist_r = float(cfg.distance_bonus) if math.sqrt(ddx * ddx + ddy * ddy) > float(cfg.distance_cutoff) else 0.0
        dpsi = f32(st["psi"][g]) - f32(tr["psi"])
        psi_r = (1.0 - math.cos(float(dpsi))) * (-float(cfg.heading_penalty))
        reward[i] = f32(((float(cfg.waypoint_bonus) if reach else 0.0) + dist_r) + psi_r)
    return reward, flags
