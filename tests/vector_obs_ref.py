"""float32 numpy restatement of tde_vector_obs (include/tde_hip.h), the checker of the GPU tests: test infrastructure only, nothing in
the package imports it.  Takes a World, a HOST state (EnvState without a device, or a dict of its numpy arrays), the tde_config and a
config.VectorObs; every expression is the header's, in float32 (numpy rounds once per operation and never contracts).  Headings go
through the oracle's sincosf (the shared specification of tde_device.h: sincos_f32); the road samples through the oracle's brute
force over the map's triangles (compute_offroad of zero-size boxes, whose four corners are the sample itself)."""
import numpy as np

from oracle import oracle
from torchdriveenv_amd import _abi

f32 = np.float32


def red_mask(world, m, k):
    """lights of map m that are red at env step k (tde_kernels.h: red_mask)"""
    mp = world.arrays["maps"][m]
    cyc = int(mp["cycle_steps"])
    if cyc <= 0:
        return 0
    t = int(k) % cyc
    ph = world.arrays["phases"]
    for p in range(int(mp["n_phase"])):
        q = ph[int(mp["phase_base"]) + p]
        if t < int(q["end_step"]):
            return int(q["red_mask"])
    return 0


def entry_distance(x0, y0, ux, uy, bx, by, bc, bs, h0, h1):
    """the header's slab test, rays [n, 1] against boxes [1, k] -> float32 [n, k] (+inf on a miss)"""
    rx, ry = f32(x0) - bx, f32(y0) - by
    o0, o1 = rx * bc + ry * bs, ry * bc - rx * bs
    d0, d1 = ux * bc + uy * bs, uy * bc - ux * bs
    inf = f32(np.inf)

    def slab(o, d, h):
        with np.errstate(divide="ignore", invalid="ignore"):
            ta, tb = (-h - o) / d, (h - o) / d
        inside = (-h <= o) & (o <= h)
        lo = np.where(d == 0, np.where(inside, -inf, inf), np.minimum(ta, tb))
        hi = np.where(d == 0, np.where(inside, inf, -inf), np.maximum(ta, tb))
        return lo.astype(f32), hi.astype(f32)

    lo0, hi0 = slab(o0, d0, h0)
    lo1, hi1 = slab(o1, d1, h1)
    tn, tf = np.maximum(lo0, lo1), np.minimum(hi0, hi1)
    return np.where((tn <= tf) & (tf >= 0), np.maximum(tn, f32(0)), inf).astype(f32)


def _road_off(cfg, world, maps, px, py):
    """the offroad predicate of the step's box corners at every point (maps[i]: the map of point i) -> bool [n]"""
    n = len(px)
    if n == 0:
        return np.zeros(0, bool)
    if cfg.offroad_threshold_squared:
        tri, mp = world.arrays["tri"], world.arrays["maps"]
        out = np.zeros(n, bool)
        for i in range(n):
            m = mp[maps[i]]
            t = tri[int(m["tri_base"]):int(m["tri_base"]) + int(m["n_tri"])]
            out[i] = not oracle.point_near_mesh(px[i], py[i], t, f32(cfg.offroad_threshold))
        return out
    z = np.zeros(n, f32)
    off = oracle.compute_offroad(n, 1, np.ascontiguousarray(px, f32), np.ascontiguousarray(py, f32), z.copy(), z.copy(), z.copy(),
                                 np.ones(n, np.uint8), world, np.ascontiguousarray(maps, np.int32), f32(cfg.offroad_threshold))
    return off != 0


def vector_obs(cfg, world, st, vo, only=None, out=None):
    """the rows tde_vector_obs writes: float32 [B, D]; rows with only[e] == 0 are those of `out` (zeros without it)"""
    B, A = len(st["scn"]), world.A
    k, nr = int(vo.k_neighbours), int(vo.n_rays)
    D = vo.dim
    res = np.zeros((B, D), f32) if out is None else np.array(out, f32, copy=True).reshape(B, D)
    L, h, r = f32(vo.ray_range), f32(vo.ray_step), f32(vo.neighbour_radius)
    M = int(L / h)
    rd = vo.ray_directions()
    x, y, psi, v = (np.asarray(st[n], f32).reshape(B, A) for n in ("x", "y", "psi", "v"))
    ln, wd = np.asarray(st["len"], f32).reshape(B, A), np.asarray(st["wid"], f32).reshape(B, A)
    pres = np.asarray(st["present"]).reshape(B, A) != 0
    S, C = oracle.sincosf(psi.ravel())
    S, C = S.reshape(B, A), C.reshape(B, A)
    scn, mp, wp = world.arrays["scn"], world.arrays["maps"], world.arrays["wp_xy"]
    stop = world.arrays["stoplines"]
    lights_on = bool(cfg.flags & _abi.F_TRAFFIC_LIGHTS)
    envs = [e for e in range(B) if only is None or only[e]]
    road_pts = []                                     # (env, ray, px [M], py [M])
    for e in envs:
        s = int(st["scn"][e])
        m = int(scn[s]["map"])
        n_wp, ti, steps = int(scn[s]["wp_n"]), int(st["target_idx"][e]), int(st["steps"][e])
        x0, y0, v0, s0, c0 = x[e, 0], y[e, 0], v[e, 0], S[e, 0], C[e, 0]
        row = np.zeros(D, f32)
        row[0], row[1], row[2] = v0, ln[e, 0], wd[e, 0]
        for q, j in enumerate((ti, ti + 1)):
            if j < n_wp:
                dx, dy = f32(wp[s, j, 0]) - x0, f32(wp[s, j, 1]) - y0
                row[3 + 2 * q], row[4 + 2 * q] = dx * c0 + dy * s0, dy * c0 - dx * s0
        row[7] = f32(min(max(n_wp - ti, 0), 2))
        row[8] = f32(steps) / f32(cfg.max_steps)
        row[9] = f32(1.0 if int(mp[m]["n_stop"]) > 0 and int(mp[m]["cycle_steps"]) > 0 else 0.0)
        # neighbours
        others = np.flatnonzero(pres[e] & (np.arange(A) > 0))
        dx, dy = x[e, others] - x0, y[e, others] - y0
        d2 = dx * dx + dy * dy
        cand = d2 < r * r
        oc, dxc, dyc, d2c = others[cand], dx[cand], dy[cand], d2[cand]
        order = np.lexsort((oc, d2c.view(np.uint32)))[:k]
        for q, i in enumerate(order):
            a = oc[i]
            cr = C[e, a] * c0 + S[e, a] * s0
            sr = S[e, a] * c0 - C[e, a] * s0
            row[10 + 9 * q:19 + 9 * q] = [f32(1), dxc[i] * c0 + dyc[i] * s0, dyc[i] * c0 - dxc[i] * s0, cr, sr, v[e, a] * cr - v0,
                                          v[e, a] * sr, ln[e, a], wd[e, a]]
        # rays
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
            px = x0 + tj[None, :] * ux[:, None]
            py = y0 + tj[None, :] * uy[:, None]
            road_pts.append((e, m, px, py))
        res[e] = row
    if road_pts and nr:
        px = np.concatenate([p[2].ravel() for p in road_pts])
        py = np.concatenate([p[3].ravel() for p in road_pts])
        maps = np.concatenate([np.full(p[2].size, p[1], np.int32) for p in road_pts])
        off = _road_off(cfg, world, maps, px, py).reshape(len(road_pts), nr, M)
        tj = np.arange(1, M + 1).astype(f32) * h
        r0 = 10 + 9 * k
        for n, (e, _, _, _) in enumerate(road_pts):
            first = np.where(off[n].any(1), off[n].argmax(1), -1)
            res[e, r0:r0 + 3 * nr:3] = np.where(first >= 0, tj[np.maximum(first, 0)], L)
    return res
