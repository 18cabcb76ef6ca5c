"""Host-side mirror of the reference's env surface over the HIP step path.

  * `BatchedWaypointEnv`  — B envs per GPU in one fused kernel per step; device-resident torch outputs (fast path) and
    an SB3-`VecEnv`-shaped numpy API (`step_async/step_wait`, auto-reset with `terminal_observation`), so
    `SubprocVecEnv` (ref examples/rl_training.py:159) is unnecessary.
  * `WaypointSuiteEnv` + `SingleAgentWrapper` — the B=1, one-exposed-agent interface the reference registers as
    'torchdriveenv-v0' (ref __init__.py:10, gym_env.py:303-487): same signatures, shapes, dtypes and info keys.

What stays in Python is only argument marshalling; every number comes from libtde_hip.so.  There is no CPU fallback.
"""
import contextlib
import dataclasses
import math
import warnings

import numpy as np
import torch

from . import _abi, ops
from .config import (EnvConfig, NearField, Planner, VectorObs, WaypointSuite, check_near_field, check_plan_react, check_plan_refine, check_planner, check_vector_obs, observation_layout,
                     render_flags, to_tde_config, validate)
from .observe import make_observer
from .state import EnvState
from .video import VideoRecorder
from .world import (NearFieldTable, World, assemble_world, build_near_field, check_threshold, corridor_mesh,
                    effective_offroad_distance, mesh_distance)

try:  # optional: neither gymnasium nor SB3 ships in this image
    import gymnasium as gym
    _GymEnvBase, _GymWrapperBase = gym.Env, gym.Wrapper
except Exception:  # pragma: no cover
    gym = None
    _GymEnvBase = object

    class _GymWrapperBase:
        def __init__(self, env):
            self.env = env

        def __getattr__(self, name):
            if name == "env":
                raise AttributeError(name)
            return getattr(self.env, name)


class Box:
    """stand-in for gym.spaces.Box when gymnasium is absent (same attributes)"""

    def __init__(self, low, high, shape=None, dtype=np.float32):
        self.low = np.asarray(low, dtype=dtype) if shape is None else np.full(shape, low, dtype=dtype)
        self.high = np.asarray(high, dtype=dtype) if shape is None else np.full(shape, high, dtype=dtype)
        self.shape = self.low.shape
        self.dtype = np.dtype(dtype)

    def sample(self):
        return np.random.uniform(self.low, self.high).astype(self.dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and np.all(x >= self.low) and np.all(x <= self.high)


def _box(low, high, shape=None, dtype=np.float32):
    if gym is not None:
        return gym.spaces.Box(low=low, high=high, shape=shape, dtype=dtype) if shape is not None else \
            gym.spaces.Box(low=np.asarray(low, dtype=dtype), high=np.asarray(high, dtype=dtype), dtype=dtype)
    return Box(low, high, shape, dtype)


# action space of the reference: acceleration in [-1, 1], steering in [-0.3, 0.3], raw units (ref gym_env.py:83-94)
ACTION_LOW, ACTION_HIGH = (-1.0, -0.3), (1.0, 0.3)


def _straight_route(x, y, psi, v):
    ahead = max(30.0, 25.0 * max(v, 1.0))
    return [(x + math.cos(psi) * d, y + math.sin(psi) * d) for d in np.arange(8.0, ahead, 8.0)]


def _mesh_of_location(road_meshes, loc):
    """the caller's drivable mesh for a location as a [n, 3, 2] float array, or None (-> synthetic corridor)"""
    if road_meshes is None:
        return None
    tri = road_meshes(loc) if callable(road_meshes) else road_meshes.get(loc)
    if tri is None:
        return None
    if isinstance(tri, (str, bytes)) or hasattr(tri, "__fspath__"):
        tri = np.load(tri)                                   # a .npy file of the triangles
    tri = np.asarray(tri, dtype=np.float64)
    if tri.ndim == 2 and tri.shape[1] == 6:
        tri = tri.reshape(-1, 3, 2)
    if tri.ndim != 3 or tri.shape[1:] != (3, 2) or len(tri) == 0 or not np.isfinite(tri).all():
        raise ValueError(f"road mesh of location {loc!r} must be a finite [n, 3, 2] (or [n, 6]) array of triangle vertices, "
                         f"got shape {tri.shape}")
    return tri


def mesh_from_verts_faces(verts, faces):
    """(V, 2+) vertices and (F, 3) vertex indices - the layout of torchdrivesim's `road_mesh` (ref gym_env.py:184: verts / faces of
    `map_cfg.road_mesh`) - as the [F, 3, 2] triangle soup `road_meshes` takes"""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, np.asarray(verts).shape[-1])[:, :2]
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return v[f]


def traffic_lights_from_controller(stoplines, light_states, durations, dt=0.1):
    """The per-location traffic-light description `traffic_lights=` takes, from the pieces the reference's map config holds
    (ref gym_env.py:181-189: `map_cfg.stoplines` with agent_type 'traffic_light' and `map_cfg.traffic_light_controller`):

      stoplines     iterable of stop lines: objects / dicts with actor_id, x, y, orientation (or psi), length, width
                    (an `agent_type` other than 'traffic_light' - stop / yield signs - is skipped, as at gym_env.py:183)
      light_states  the controller's cycle: one mapping actor_id -> 'red' | 'yellow' | 'green' (anything but 'red' lets traffic
                    pass: compute_traffic_lights_violations only counts red lights) per phase
      durations     seconds each phase lasts (rounded to whole steps of `dt`, at least one)

    -> dict(stoplines=[(x, y, psi, length, width, light)], phases=[(n_steps, [red lights])], actor_ids=[...]) with `light` the
    index of the line's actor in actor_ids."""
    def get(o, *names, default=None):
        for n in names:
            v = o.get(n) if isinstance(o, dict) else getattr(o, n, None)
            if v is not None:
                return v
        return default

    ids, lines = [], []
    for sl in stoplines:
        if get(sl, "agent_type", default="traffic_light") != "traffic_light":
            continue
        aid = get(sl, "actor_id")
        if aid not in ids:
            ids.append(aid)
        lines.append((float(get(sl, "x")), float(get(sl, "y")), float(get(sl, "orientation", "psi", default=0.0)),
                      float(get(sl, "length", default=1.0)), float(get(sl, "width", default=3.5)), ids.index(aid)))
    assert len(light_states) == len(durations) and len(durations) >= 1, "one duration per phase of the light cycle"
    phases = []
    for states, sec in zip(light_states, durations):
        red = sorted(ids.index(a) for a, st in states.items() if a in ids and str(st).lower() == "red")
        phases.append((max(1, int(round(float(sec) / dt))), red))
    return dict(stoplines=lines, phases=phases, actor_ids=ids)


def _lights_of_location(traffic_lights, loc):
    """the caller's traffic lights of a location as dict(stoplines=[(x, y, psi, length, width, light)], phases=[(n_steps, [red])])
    with validated shapes, or None"""
    if traffic_lights is None or loc is None:
        return None
    spec = traffic_lights(loc) if callable(traffic_lights) else traffic_lights.get(loc)
    if spec is None or not spec.get("stoplines"):
        return None
    lines = [tuple(float(t) for t in sl[:5]) + (int(sl[5]),) for sl in spec["stoplines"]]
    phases = [(int(n), sorted(int(i) for i in red)) for n, red in spec["phases"]]
    if not phases or min(n for n, _ in phases) < 1 or min(sl[5] for sl in lines) < 0 or not np.isfinite(np.asarray([sl[:5] for sl in lines])).all():
        raise ValueError(f"traffic lights of location {loc!r}: stop lines are (x, y, psi, length, width, light >= 0), phases (n_steps >= 1, "
                         f"[red lights]) and there is at least one phase")
    return dict(stoplines=lines, phases=phases)


MAX_GROUP_LIGHTS = 32        # a light is a bit of a 32-bit mask (tde_light_phase.red_mask)


def _light_group(spec, polylines, radius):
    """The stop lines of `spec` a scenario sees: all of them when the location is small (at most 32 lights), else those within
    `radius` metres of the scenario's polylines - at most 32 distinct lights, the nearest ones (a light is a bit of a 32-bit mask
    and the kernels walk every stop line of a scenario's map descriptor) - with the lights re-numbered 0 .. n-1 inside the group.
    -> (sorted tuple of the kept stop-line indices, dict(stoplines, phases)) or (None, None) when nothing is in reach."""
    lines = spec["stoplines"]
    lights = sorted({sl[5] for sl in lines})
    keep = list(range(len(lines)))
    if len(lights) > MAX_GROUP_LIGHTS:
        pts = np.concatenate([np.asarray(pl, np.float64).reshape(-1, 2) for pl in polylines], 0)
        ctr = np.asarray([sl[:2] for sl in lines], np.float64)
        d = np.sqrt(((ctr[:, None, :] - pts[None, :, :]) ** 2).sum(-1)).min(1)
        near = [i for i in range(len(lines)) if d[i] <= radius]
        by_light = {}
        for i in near:
            by_light[lines[i][5]] = min(by_light.get(lines[i][5], np.inf), d[i])
        if len(by_light) > MAX_GROUP_LIGHTS:
            order = sorted(by_light, key=lambda g: (by_light[g], g))
            warnings.warn(f"{len(by_light)} traffic lights within {radius:g} m of a scenario: the nearest {MAX_GROUP_LIGHTS} are kept "
                          f"(lower light_radius to choose differently)", stacklevel=3)
            by_light = {g: by_light[g] for g in order[:MAX_GROUP_LIGHTS]}
        keep = [i for i in near if lines[i][5] in by_light]
        lights = sorted(by_light)
    if not keep:
        return None, None
    local = {g: n for n, g in enumerate(lights)}
    grp = dict(stoplines=[lines[i][:5] + (local[lines[i][5]],) for i in keep],
               phases=[(n, [local[g] for g in red if g in local]) for n, red in spec["phases"]])
    return tuple(keep), grp


def _heading_table(start_headings, loc, p0, p1, n):
    """the lane direction at n points along the first waypoint segment p0 -> p1 (entry j at fraction (j + 0.5) / n), from the
    caller's heading field: what the reference reads with find_lanelet_directions(lanelet_map, x, y)[0] at the sampled start point
    (ref gym_env.py:359-361).  None when the caller gives no field for the location."""
    if start_headings is None or loc is None:
        return None
    f = start_headings
    if isinstance(f, dict):
        f = f.get(loc)
        if f is None:
            return None
        field = f if callable(f) else (lambda x, y, c=float(f): c)
    else:
        field = lambda x, y: start_headings(loc, x, y)       # noqa: E731
    out = []
    for j in range(n):
        t = (j + 0.5) / n
        psi = field(p0[0] + t * (p1[0] - p0[0]), p0[1] + t * (p1[1] - p0[1]))
        if psi is None:
            return None
        out.append(float(np.asarray(psi, dtype=np.float64).reshape(-1)[0]))    # (find_lanelet_directions returns a list: its first entry)
    if not np.isfinite(out).all():
        raise ValueError(f"start_headings of location {loc!r} returned a non-finite heading")
    return out


def _heading_field(start_headings, loc):
    """the caller's lane-direction field of a location as a callable (x, y) -> psi or None, or None"""
    if start_headings is None or loc is None:
        return None
    f = start_headings
    if isinstance(f, dict):
        f = f.get(loc)
        if f is None:
            return None
        return f if callable(f) else (lambda x, y, c=float(f): c)
    return lambda x, y: start_headings(loc, x, y)


def _resample_polyline(pl, pitch, where=None):
    """(x, y, psi) every `pitch` metres of arc length along a polyline, psi = the direction of the segment (`where`: a list that
    receives (segment, metres into it) of every point)"""
    p = np.asarray(pl, np.float64).reshape(-1, 2)
    out = []
    carry = 0.0
    for i, (a, b) in enumerate(zip(p[:-1], p[1:])):
        d = float(np.hypot(*(b - a)))
        if d <= 0:
            continue
        psi = math.atan2(b[1] - a[1], b[0] - a[0])
        t = carry
        while t <= d:
            out.append((a[0] + (b[0] - a[0]) * t / d, a[1] + (b[1] - a[1]) * t / d, psi))
            if where is not None:
                where.append((i, t))
            t += pitch
        carry = t - d
    return np.asarray(out, np.float64).reshape(-1, 3)


def near_field_positions(world, nf, scn_polylines, locations, start_headings=None, with_routes=False):
    """candidate positions [m, 3] of (x, y, psi) per scenario, from the first source that applies: the `nf.candidates` hook
    (location, scenario_index) -> [n, 3]; the location's lane-direction field (`start_headings`) on a lattice of pitch `nf.pitch`
    over the scenario's drivable mesh, where the field gives a heading; the scenario's polylines (waypoints, NPC routes, replay
    paths) every `nf.pitch` metres with the segment's direction.  -> (positions, source names)
    with_routes: -> (positions, source names, tracers), tracers[s](i, x, y, psi) = the waypoints ahead of candidate i of scenario s
    for world.build_near_field, from the candidate's own source: the field stepped `route_pitch` at a time; the rest of the polyline
    it was resampled from, every `route_pitch` metres; the route the hook gave for it, else the field's trace (None: no tracer)"""
    from .world import polyline_ahead, trace_heading_field

    thr = 0.5 if world.threshold is None else float(world.threshold)
    tri_all = world.arrays["tri"].reshape(-1, 3, 2).astype(np.float64)
    rp = float(nf.route_pitch if nf.route_pitch is not None else nf.pitch)
    n_pts = int(nf.route_points)
    pos, src, tracers = [], [], []

    def field_tracer(field):
        return None if field is None else (lambda i, x, y, psi: trace_heading_field(field, x, y, psi, rp, n_pts))

    for si in range(world.n_scn):
        loc = locations[si]
        if nf.candidates is not None:
            try:
                got = nf.candidates(loc, si)
                own = None
                # (points, routes) only under `routes`, and only a pair whose first member is the [n, 3] array: any other return is
                # the points themselves, as it always was
                if nf.routes and isinstance(got, tuple) and len(got) == 2 and np.ndim(got[0]) == 2:
                    got, own = got
                P = np.asarray(got, np.float64)
            except (TypeError, ValueError) as ex:
                raise ValueError(f"near_field.candidates({loc!r}, {si}) failed: {ex}") from ex
            if own is not None and len(own) != len(P):
                raise ValueError(f"near_field.candidates({loc!r}, {si}) gave {len(own)} routes for {len(P)} candidates")
            by_field = field_tracer(_heading_field(start_headings, loc))
            tracers.append((lambda i, x, y, psi, own=own, f=by_field:
                            own[i] if own is not None and own[i] is not None else f(i, x, y, psi) if f is not None else None))
            if P.size == 0:
                P = P.reshape(0, 3)
            if P.ndim != 2 or P.shape[1] != 3:
                raise ValueError(f"near_field.candidates({loc!r}, {si}) must return an array [n, 3] of (x, y, psi), got shape {P.shape}")
            pos.append(P)
            src.append("candidates")
            continue
        field = _heading_field(start_headings, loc)
        if field is not None:
            p0, p1 = world.arrays["wp_xy"][si, 0], world.arrays["wp_xy"][si, 1]
            reach = float(nf.radius) + float(np.hypot(*(p1 - p0)))
            g = float(nf.pitch)
            xs = np.arange(math.floor((p0[0] - reach) / g), math.ceil((p0[0] + reach) / g) + 1) * g
            ys = np.arange(math.floor((p0[1] - reach) / g), math.ceil((p0[1] + reach) / g) + 1) * g
            X, Y = np.meshgrid(xs, ys, indexing="xy")
            pts = np.stack([X.reshape(-1), Y.reshape(-1)], -1)
            pts = pts[np.hypot(pts[:, 0] - p0[0], pts[:, 1] - p0[1]) <= reach]
            md = world.arrays["maps"][int(world.arrays["scn"]["map"][si])]
            mesh = tri_all[int(md["tri_base"]):int(md["tri_base"]) + int(md["n_tri"])]
            pts = pts[mesh_distance(pts, mesh, thr) <= thr]
            P = []
            for x, y in pts:
                psi = field(float(x), float(y))
                if psi is None:
                    continue
                psi = float(np.asarray(psi, np.float64).reshape(-1)[0])
                if np.isfinite(psi):
                    P.append((x, y, psi))
            pos.append(np.asarray(P, np.float64).reshape(-1, 3))
            src.append("lattice")
            tracers.append(field_tracer(field))
            continue
        where = [[] for _ in scn_polylines[si]]
        pls = [_resample_polyline(pl, float(nf.pitch), w) for pl, w in zip(scn_polylines[si], where)]
        pos.append(np.concatenate(pls, 0) if pls else np.zeros((0, 3)))
        src.append("polylines")
        flat = [(pl, seg, t) for pl, w in zip(scn_polylines[si], where) for seg, t in w]
        tracers.append(lambda i, x, y, psi, flat=flat: polyline_ahead(*flat[i], rp, n_pts))
    return (pos, src, tracers) if with_routes else (pos, src)


def world_from_waypoint_suite(data: WaypointSuite, agents_per_env=8, road_width=12.0, threshold=0.5,
                              background=None, background_radius=250.0, ego_only=False, road_meshes=None, near_range=None,
                              traffic_lights=None, light_radius=150.0, start_headings=None, heading_samples=16,
                              near_field=None, near_field_seed=0):
    """WaypointSuite -> World, or (World, NearFieldTable) with `near_field`.  Agent ordering follows the reference: slot 0 ego, then the scenario's agents
    (ref gym_env.py:219-228); `car_sequence_suite[i][k]` replays slot k (ref gym_env.py:275-283).
    The CARLA town meshes the reference takes from torchdrivesim's package data are not available, so each scenario
    gets a synthetic drivable corridor around its waypoints, scenario agents and replay paths; non-replayed scenario
    agents get a straight route along their initial heading for the heuristic NPC controller.

    `background`: directory of background-traffic JSON files (ref gym_env.py:200-235), or a callable
    location -> dict from `loaders.load_background_traffic`.  As in the reference the ego takes the attributes of the
    file's first agent (:223) and the file's agents farther than 100 m from the ego start are kept (:227-231); the
    near field, which the reference fills through a remote INITIALIZE call (:232-235), stays empty unless `near_field` is given.  Of the kept
    agents the nearest ones (within `background_radius`, so the synthetic corridor mesh stays local) fill the free
    slots after the scenario's own agents.  `ego_only`: the ego alone, no scenario / replay / background agents
    (ref gym_env.py:192-198).

    `road_meshes`: the drivable surface per location, as the reference takes it from `find_map_config(location).road_mesh`
    (ref gym_env.py:312, 184, 260): a dict location -> triangles ([n, 3, 2] or [n, 6] array, or the path of a .npy file holding
    one; `mesh_from_verts_faces` converts a verts / faces pair), or a callable location -> the same or None.  Scenarios of a
    location that has a mesh all run on ONE map built from it (one grid index per location); a location without one falls back to
    the synthetic corridor of its scenario.

    `traffic_lights`: the stop lines and light cycle per location, as the reference takes them from the map config
    (`map_cfg.stoplines` / `map_cfg.traffic_light_controller`, ref gym_env.py:181-189; fed to the NPCs :290-291, to is_terminated
    :415 and get_info :429): a dict location -> dict(stoplines=[(x, y, psi, length, width, light)], phases=[(n_steps, [red
    lights])]) or a callable location -> the same or None (`traffic_lights_from_controller` builds one from stop-line objects and
    a controller's state sequence).  The cycle restarts with every episode.  A location with more than 32 lights is cut into
    per-scenario neighbourhoods (the lines within `light_radius` metres of the scenario's waypoints, agents and replay paths; a
    light is a bit of a 32-bit mask): each distinct set becomes a light group - a map descriptor of its own that shares the
    location's mesh (assemble_world).  A world with lights steps with TDE_F_TRAFFIC_LIGHTS (BatchedWaypointEnv sets it): the ego's
    stop-line violation terminates the episode and shows in info["traffic_light_violation"], the NPCs stop at red lines, the
    birdview paints the lines.

    `start_headings`: the lane direction at the ego's start - what the reference reads with find_lanelet_directions(lanelet_map,
    x, y)[0] at the point it drew on the first waypoint segment (ref gym_env.py:357-361) - as a callable (location, x, y) -> psi
    or a dict location -> callable (x, y) -> psi (or a constant).  Sampled at `heading_samples` points along every scenario's
    first segment into the world's heading table (tde_world.start_psi); the episode's start heading is the entry of its drawn
    fraction + normal(0, 0.1).  Without it: the direction of the first segment.

    `near_range` (metres; default world.NEAR_RANGE = 2): how far beyond the offroad threshold the grid index carries NEAR LISTS, from
    which the MAGNITUDE of the offroad infraction (info["offroad"], ref gym_env.py:427) is two table look-ups; a corner farther out
    is still exact but found by scanning the grid, and beyond the reach where that square would hold more cells than the map has
    triangles by a walk over all the map's triangles (tens of microseconds per such ego and step).  Raise it (it costs table memory:
    a few records per square metre of the band) for `terminated_at_infraction=False` runs whose egos keep driving off the road.

    `near_field` (config.NearField): traffic within `radius` of the ego at every reset, the local stand-in for the reference's
    iai_conditional_initialize (ref gym_env.py:232-238, iai.py:6-60).  The candidate table (world.build_near_field) is built here
    from the first source that applies per scenario: the `candidates` hook, the location's `start_headings` field on a lattice over
    its mesh, or the scenario's polylines (near_field_positions); attributes from a generator seeded by (`near_field_seed`,
    scenario).  `density` None: the background file's agent_density (the largest over the scenarios) with `background`, else 0.
    Returns (world, table); tde_near_field_spawn (BatchedWaypointEnv(near_field=...)) draws from the table per episode."""
    from . import loaders
    if near_field is not None:
        near_field = check_near_field(near_field)
        if ego_only:
            raise ValueError("near_field with ego_only=True: the reference spawns no traffic in ego-only mode (gym_env.py:192-198)")
    scn_polylines, scn_locations, densities = [], [], []
    meshes, scenarios = [], []
    map_of_location = {}
    light_groups, group_of = [], {}                  # (map id, kept stop lines) -> index into light_groups
    n = len(data.waypoint_suite)
    for i in range(n):
        wps = [tuple(p) for p in data.waypoint_suite[i]]
        scen = data.scenarios[i] if data.scenarios is not None and not ego_only else None
        seqs = (data.car_sequence_suite[i] if data.car_sequence_suite is not None and not ego_only else None) or {}
        seqs = {int(k): v for k, v in seqs.items()}
        polylines = [wps]
        agents = []
        if scen is not None and scen.agent_states:
            for k, (s, a) in enumerate(zip(scen.agent_states, scen.agent_attributes)):
                slot = k + 1
                x, y, psi, v = [float(t) for t in s[:4]]
                replay = seqs.get(slot)
                route = None
                if replay is None:
                    route = _straight_route(x, y, psi, v)
                    polylines.append([(x, y)] + route)
                else:
                    polylines.append([(r[0], r[1]) for r in replay[::10]] + [(replay[-1][0], replay[-1][1])])
                agents.append(dict(state=(x, y, psi, v), attr=tuple(float(t) for t in a[:3]), vdes=v, route=route,
                                   replay=[tuple(float(t) for t in r[:4]) for r in replay] if replay else None))
        for slot, replay in seqs.items():          # replay cars that are not scenario agents
            if slot - 1 >= len(agents) and replay:
                r0 = replay[0]
                agents.append(dict(state=tuple(float(t) for t in r0[:4]), attr=(5.0, 2.0, 1.9), vdes=0.0, route=None,
                                   replay=[tuple(float(t) for t in r[:4]) for r in replay]))
                polylines.append([(r[0], r[1]) for r in replay[::10]] + [(replay[-1][0], replay[-1][1])])
        ego_attr = None
        if background is not None and not ego_only:
            loc = data.locations[i] if data.locations else ""
            bt = background(loc) if callable(background) else loaders.pick_background_traffic(loc, background)
            if bt is not None:
                densities.append(int(bt.get("agent_density") or 0))
            if bt is not None and bt["agent_states"]:
                ego_attr = tuple(float(t) for t in bt["agent_attributes"][0][:3])
                far = [(math.dist(wps[0], s[:2]), k) for k, s in enumerate(bt["agent_states"])]
                far = sorted((d, k) for d, k in far if 100.0 < d <= background_radius)
                for _, k in far[:max(0, agents_per_env - 1 - len(agents))]:
                    x, y, psi, v = [float(t) for t in bt["agent_states"][k][:4]]
                    route = _straight_route(x, y, psi, v)
                    polylines.append([(x, y)] + route)
                    agents.append(dict(state=(x, y, psi, v), attr=tuple(float(t) for t in bt["agent_attributes"][k][:3]),
                                       vdes=v, route=route, replay=None))
        heading = math.atan2(wps[1][1] - wps[0][1], wps[1][0] - wps[0][0])
        loc = data.locations[i] if data.locations else None
        if loc is not None and loc in map_of_location:
            map_id = map_of_location[loc]
        else:
            tri = _mesh_of_location(road_meshes, loc) if loc is not None else None
            map_id = len(meshes)
            if tri is not None:
                map_of_location[loc] = map_id
                meshes.append(tri)
            else:
                meshes.append(corridor_mesh(polylines, width=road_width))
        if len(agents) > agents_per_env - 1:
            # the reference assembles up to ~100 agents per env (gym_env.py:216-237); an env here has agents_per_env slots
            # (a power of two <= TDE_MAX_AGENTS = 128): the scenario's own agents come first, what does not fit is dropped - loudly
            warnings.warn(f"scenario {i}: {len(agents)} non-ego agents but only {agents_per_env - 1} NPC slots "
                          f"(agents_per_env={agents_per_env}): the last {len(agents) - (agents_per_env - 1)} are dropped; "
                          f"raise agents_per_env (a power of two, at most {_abi.TDE_MAX_AGENTS})", stacklevel=2)
        scn = dict(map=map_id, waypoints=wps, start_heading=heading, agents=agents[:agents_per_env - 1])
        if ego_attr is not None:
            scn["ego_attr"] = ego_attr
        spec = _lights_of_location(traffic_lights, loc)
        if spec is not None:
            key, grp = _light_group(spec, polylines, float(light_radius))
            if key is not None:
                if (map_id, loc, key) not in group_of:
                    group_of[(map_id, loc, key)] = len(light_groups)
                    light_groups.append(dict(map=map_id, **grp))
                scn["lights"] = group_of[(map_id, loc, key)]
        table = _heading_table(start_headings, loc, wps[0], wps[1], int(heading_samples))
        if table is not None:
            scn["start_headings"] = table
        scenarios.append(scn)
        scn_polylines.append(polylines)
        scn_locations.append(loc)
    if any("start_headings" in sc for sc in scenarios):      # one table size per world: the others repeat their segment's direction
        for sc in scenarios:
            sc.setdefault("start_headings", [sc["start_heading"]] * int(heading_samples))
    from .world import NEAR_RANGE
    world = assemble_world(meshes, scenarios, agents_per_env, threshold=threshold, light_groups=light_groups,
                           near_range=NEAR_RANGE if near_range is None else float(near_range))
    if near_field is None:
        return world
    positions, sources, tracers = near_field_positions(world, near_field, scn_polylines, scn_locations, start_headings, with_routes=True)
    density = int(near_field.density) if near_field.density is not None else max(densities, default=0)
    table = build_near_field(world, positions, near_field, near_field_seed, density, tracers if near_field.routes else None)
    table.sources = sources
    return world, table


def eval_plan(n_scn, B, cases=None, repeats=1):
    """the static schedule of BatchedWaypointEnv.evaluate -> (plan int32 [R, B] numpy, jobs int32 [J]): jobs = `cases` (default:
    every scenario) repeated `repeats` times; job j is episode j // B of env j % B; -1 where an env has no further episode"""
    cases = np.arange(int(n_scn)) if cases is None else np.asarray(cases)
    if cases.ndim != 1 or len(cases) == 0 or cases.dtype.kind not in "iu":
        raise ValueError("cases must be a non-empty sequence of scenario indices")
    if int(cases.min()) < 0 or int(cases.max()) >= int(n_scn):
        raise ValueError(f"cases must be in [0, {int(n_scn)})")
    if int(repeats) != repeats or int(repeats) < 1:
        raise ValueError("repeats must be an integer >= 1")
    jobs = np.tile(cases.astype(np.int32), int(repeats))
    R = -(-len(jobs) // int(B))
    plan = np.full(R * int(B), -1, np.int32)
    plan[:len(jobs)] = jobs
    return plan.reshape(R, int(B)), jobs


@dataclasses.dataclass
class EvalResult:
    """the finished episodes of BatchedWaypointEnv.evaluate, one entry per job in job order (host tensors)"""
    episode_return: torch.Tensor    # float64 [J]: sum of the episode's rewards
    length: torch.Tensor            # int32 [J]: its number of steps
    reached: torch.Tensor           # int32 [J]: reached_waypoint_num at its last step
    scenario: torch.Tensor          # int32 [J]: the scenario it ran
    bits: torch.Tensor              # uint8 [J]: the done bits of its last step (1 terminated, 2 truncated, 4 offroad, 8 collided, 16 red light)
    psi_smoothness: torch.Tensor    # float64 [J]: mean of info["psi_smoothness"] over its steps (psi_sum / length)
    speed_smoothness: torch.Tensor  # float64 [J]: mean of info["speed_smoothness"] over its steps

    @classmethod
    def from_records(cls, rec, jobs=None):
        """from tde_episode_record rows (_abi.EPISODE_RECORD_DTYPE) in job order; `jobs`: the scenario of every job, checked"""
        rec = np.ascontiguousarray(rec)
        if jobs is not None and not np.array_equal(rec["scn"], np.asarray(jobs)):
            raise RuntimeError("evaluate(): a job was not recorded under its scenario")
        n = rec["length"].astype(np.float64)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))      # noqa: E731
        return cls(t(rec["ret"]), t(rec["length"]), t(rec["reached"]), t(rec["scn"]), t(rec["bits"]), t(rec["psi_sum"] / n),
                   t(rec["speed_sum"] / n))

    def __len__(self):
        return int(self.length.numel())

    def metrics(self):
        """the nine values the reference's callback logs, with its arithmetic (ref examples/rl_training.py:96-108): means over
        the episodes; the rates count the episodes whose last step had the bit set (offroad 4, collision 8, red light 16, success =
        truncated 2); the smoothness values are means of the per-episode means"""
        n = len(self)
        if n == 0:
            raise ValueError("metrics() of an empty result")
        bit = lambda k: int(((self.bits >> k) & 1).sum()) / n        # noqa: E731
        mean = lambda t: sum(t.tolist()) / n                         # noqa: E731  (Python floats summed in episode order, as there)
        return {"mean_episode_reward": mean(self.episode_return), "mean_episode_length": mean(self.length),
                "offroad_rate": bit(2), "collision_rate": bit(3), "traffic_light_violation_rate": bit(4), "success_percentage": bit(1),
                "reached_waypoint_num": mean(self.reached), "psi_smoothness": mean(self.psi_smoothness),
                "speed_smoothness": mean(self.speed_smoothness)}


class _LazyInfo(dict):
    """dict of per-env info tensors (ref gym_env.py:419-437) whose values are built when first read.  The entries are VIEWS of the
    env's own output buffers (like reward / terminated / truncated): valid until the next step() overwrites them - clone what
    must be kept."""

    KEYS = ("offroad", "collision", "traffic_light_violation", "is_success")
    EXTRA = ("reached_waypoint_num", "psi_smoothness", "speed_smoothness", "psi_reward", "dist_reward")

    ALL = KEYS + EXTRA

    def __init__(self, st, B, A, magnitudes=None):
        self._st, self._BA = st, (B, A)
        self._mag = magnitudes                # float32 [B, 4] (offroad, collision, count, -) of tde_ego_infractions, or None: 0 / 1 indicators

    @property
    def _keys(self):
        return self.ALL if self._st["info"] is not None else self.KEYS

    @property
    def _ego(self):
        return slice(0, self._BA[0] * self._BA[1], self._BA[1])

    def _make(self, k):
        st = self._st
        bits = st["done_bits"]                # the ego's flags of this step, kept when the env re-spawned in place
        if k == "offroad":
            if self._mag is not None:
                return self._mag[:, 0]
            return ((bits >> 2) & 1).float() if bits is not None else st["offroad"][self._ego].float()
        if k == "collision":
            if self._mag is not None:
                return self._mag[:, 1]
            return ((bits >> 3) & 1).float() if bits is not None else st["collided"][self._ego].float()
        if k == "traffic_light_violation":
            return st["tl_violation"].float()
        if k == "is_success":
            return st["truncated"].view(torch.bool)
        if k == "reached_waypoint_num":
            return st["info_reached"]
        return st["info"][:, ("psi_smoothness", "speed_smoothness", "psi_reward", "dist_reward").index(k)]

    def __missing__(self, k):
        if k not in self._keys:
            raise KeyError(k)
        v = self._make(k)
        dict.__setitem__(self, k, v)
        return v

    def __contains__(self, k):
        return k in self._keys

    def __iter__(self):
        return iter(self._keys)

    def __len__(self):
        return len(self._keys)

    def keys(self):
        return list(self._keys)

    def items(self):
        return [(k, self[k]) for k in self._keys]

    def values(self):
        return [self[k] for k in self._keys]

    def get(self, k, default=None):
        return self[k] if k in self._keys else default


class AgentOutcomes(tuple):
    """(reward float32 [n], flags uint8 [n]) of AgentGroup.outcomes(), with the flag bits (_abi.AG_*) as bool [n] views"""
    reward, flags = property(lambda s: s[0]), property(lambda s: s[1])
    valid = property(lambda s: (s[1] & _abi.AG_VALID) != 0)
    collided = property(lambda s: (s[1] & _abi.AG_COLLIDED) != 0)
    offroad = property(lambda s: (s[1] & _abi.AG_OFFROAD) != 0)
    reached = property(lambda s: (s[1] & _abi.AG_REACHED) != 0)
    ended = property(lambda s: (s[1] & _abi.AG_ENDED) != 0)


class AgentGroup:
    """Chosen (env, slot) pairs of a BatchedWaypointEnv (env.agents): observe() before a step, outcomes() after it.  Pairs, track and
    outputs stay on the device; each call is one launch on the current stream (tde_agent_obs / tde_agent_outcomes)."""

    def __init__(self, env, pairs, vector_obs):
        self.env, self.pairs, self.vector_obs = env, pairs, vector_obs
        n, dev = pairs.shape[0], env.torch_device
        self.n = n
        self.ray_dir = torch.from_numpy(vector_obs.ray_directions()).to(dev)
        self.obs = torch.zeros((n, vector_obs.dim), dtype=torch.float32, device=dev)
        self.track = torch.zeros((n, 32), dtype=torch.uint8, device=dev)      # (all zero: nothing observed yet, outcomes() says invalid)
        self.reward = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flags = torch.zeros(n, dtype=torch.uint8, device=dev)

    def observe(self):
        """float32 [n, D]: the vector observation from every pair's slot on the state as it is (zeros for an absent slot); the track
        that outcomes() scores against is refreshed"""
        e = self.env
        return ops.agent_obs(e.tde_cfg, e.dworld, e.state, self.vector_obs, self.pairs, self.ray_dir, self.obs, self.track)

    def outcomes(self):
        """(reward float32 [n], flags uint8 [n]) of every pair since the last observe(), with .valid / .collided / .offroad / .reached /
        .ended as bool [n]; slot 0 pairs are invalid (the ego's outcome is the step's own result)"""
        e = self.env
        return AgentOutcomes(ops.agent_outcomes(e.tde_cfg, e.dworld, e.state, self.pairs, self.track, self.reward, self.flags))


class BatchedWaypointEnv:
    """`num_envs` independent WaypointSuite envs stepped by one fused HIP kernel per timestep.

    step(actions [B,2]) -> (obs, reward f32[B], terminated bool[B], truncated bool[B], info dict of [B] tensors), all
    device-resident torch tensors.  obs is the ego-centred birdview uint8 [B, 3*frame_stack, 64, 64] (obs_mode
    "birdview", the reference's observation, ref gym_env.py:95,122-124), a compact float32 [B, 8] kinematic vector
    (obs_mode "state") or the float32 [B, D] vector observation of config.VectorObs (obs_mode "vector": nearest agents, road-edge,
    car and red-line rays).  Finished envs are re-spawned inside the same kernel (auto_reset=True); with a frame stack their
    older frames restart blank in the same observation (VecFrameStack semantics, ref examples/rl_training.py:160).
    reward / terminated / truncated are the env's own buffers, overwritten by the next step (clone what must be
    kept).  (Replaying step + observation from a captured HIP graph was measured and is slower than the two direct
    launches: 27.9 vs 18.5 us per step at 8192 envs.)

    The SB3 `VecEnv` interface (numpy in / out, `terminal_observation`, `TimeLimit.truncated`, Monitor's
    `info["episode"]`) is `as_vec_env()` -> WaypointVecEnv."""

    metadata = {"render_modes": ["rgb_array"], "render_fps": 10}   # ref gym_env.py:73-76

    def __init__(self, cfg: EnvConfig, data, num_envs, agents_per_env=16, device=None, obs_mode="birdview",
                 frame_stack=1, auto_reset=True, with_info=True, background=None, env_base=0, binding="ext",
                 info_magnitudes=True, road_meshes=None, near_range=None, traffic_lights=None, start_headings=None, light_radius=150.0,
                 heading_samples=16, near_field=None, vector_obs=None, planner=None, plan_refine=None, plan_react=None, terminal_obs=False):
        """binding: "ext" = launches go through the PyTorch-ROCm C++ extension (csrc/tde_torch_ext.cpp: its EnvHandle), "ctypes" =
        through the ctypes binding of the same C-ABI (ops.py: ops.CtypesHandle, which has EnvHandle's methods); both call the very same
        entry points of libtde_hip.so, and the env launches through whichever handle it holds (`self.binding` names it).
        info_magnitudes (default): info["offroad"] / info["collision"] hold the MAGNITUDES the reference reports there (ref
        gym_env.py:427-428: sum over the ego's corners of clamp(distance - threshold, 0); sum of the IoUs with the agents the ego
        overlaps), written by the step kernel itself for the egos it flagged, before a finished env is re-spawned
        (tde_state.magnitudes: still ONE launch per step).  False: 0 / 1 indicators (the kernel then skips the magnitudes).
        traffic_lights / start_headings (light_radius, heading_samples): the stop lines + light cycle and the lane-direction field per
        location, as the reference takes them from the map config (ref gym_env.py:181-189, 359-361): world_from_waypoint_suite.
        road_meshes / near_range: the drivable mesh per location and the reach of the grid index's near lists when `data` is a
        WaypointSuite (world_from_waypoint_suite).  With `terminated_at_infraction=False` an ego may drive far off the road, where
        the exact offroad magnitude is found by a scan of the grid or a walk over the map's triangles (tens of microseconds per such
        ego and step; `near_range` moves that point outwards, info_magnitudes=False skips the work).
        near_field: traffic around the ego at every reset and re-spawn (tde_near_field_spawn, the stand-in for the reference's
        iai_conditional_initialize, ref gym_env.py:232-238): a config.NearField (or a dict of its fields) when `data` is a
        WaypointSuite, or a world.NearFieldTable built for the World `data` is (world_from_waypoint_suite(..., near_field=)).  Every
        (re)spawn - reset(), auto-reset in step(), the VecEnv's re-spawn - then runs the spawner before the state is observed;
        rollout() and the multi-stream step raise.  With NearField(routes=True) the spawned agents drive along routes of their own
        (tde_state.slot_route; step() then runs the routed one-role kernel); rollout(), plan_react= and Planner(predict="route" | "queue")
        raise ValueError.  None (default): no near field, every path as it was.
        vector_obs: the config.VectorObs (or a dict of its fields) of obs_mode="vector" (None: VectorObs()); the observation is
        float32 [B, vector_obs.dim] (tde_vector_obs), taken after every reset, step and re-spawn (after the near-field spawner).
        planner: the config.Planner (or a dict of its fields) of plan_actions() (None: Planner()).
        plan_refine: a config.PlanRefine (or a dict of its fields): plan_actions() then judges the lattice with a brake tail and
        refines the winner knot by knot through tde_score_plans.  None (default): plan_actions() is tde_plan_action as it was.
        plan_react: a config.PlanReact (or a dict of its fields): plan_actions() then judges every lattice candidate in a scene that
        reacts to it (tde_score_plans_scene).  Not with plan_refine, and only with Planner(predict="constant").  None (default):
        nothing changes.
        terminal_obs: keep the observation each finished env showed BEFORE it was re-spawned (SB3's info["terminal_observation"], on
        the device).  step() then runs the step without the in-kernel re-spawn, observes, copies the newest frame of the finished envs
        into `terminal_frames` (tde_terminal_stash: uint8 [B, H * W] layer planes, or the float32 [B, D] rows of obs_mode "vector" /
        "state"; the other envs' entries keep what they held) and re-spawns them with reset(mask=done).  Everything step() returns and
        the whole state equal, bit for bit, those of the same env without the option; a step costs a few small launches more.  Needs
        auto_reset=True and with_info=True; rollout() raises (it re-spawns inside one launch); not offered with near_field (the match
        with the in-kernel re-spawn has not been established there).  replay_buffer() / rollout_buffer() of such an env store the
        frames (include/tde_terminal.h).  False (default): nothing changes."""
        validate(cfg)
        self.terminal_obs = bool(terminal_obs)
        if self.terminal_obs and not (auto_reset and with_info):
            raise ValueError("terminal_obs=True needs auto_reset=True and with_info=True: it keeps the frame of the envs the step "
                             "finished (done_bits) before it re-spawns them")
        if self.terminal_obs and near_field is not None:
            raise ValueError("terminal_obs=True with near_field: the two-launch step (step, observe, re-spawn by reset(mask)) has not been "
                             "shown to match the in-kernel re-spawn followed by the near-field spawner bit for bit, so it is not offered")
        self.planner = check_planner(planner if planner is not None else Planner())
        self.plan_refine = check_plan_refine(plan_refine, self.planner) if plan_refine is not None else None
        self.plan_react = check_plan_react(plan_react, self.planner, self.plan_refine) if plan_react is not None else None
        if near_field is not None and not isinstance(near_field, NearFieldTable):
            near_field = check_near_field(near_field, cfg)
        if near_field is not None and cfg.ego_only:
            raise ValueError("near_field with ego_only=True: the reference spawns no traffic in ego-only mode (gym_env.py:192-198)")
        if isinstance(near_field, NearField) and isinstance(data, World):
            raise ValueError("near_field=NearField(...) needs a WaypointSuite as `data`; with a prebuilt World pass the NearFieldTable "
                             "that world_from_waypoint_suite(..., near_field=) returned with it")
        if isinstance(near_field, NearFieldTable) and not isinstance(data, World):
            raise ValueError("a NearFieldTable belongs to the World it was built for: pass that World as `data`")
        if binding not in ("ext", "ctypes"):
            raise ValueError("binding must be 'ext' or 'ctypes'")                                              # ref gym_env.py:79-80 and the fields this path rejects
        observation_layout(cfg, obs_mode, frame_stack, vector_obs)  # (raises on an obs_mode / frame_stack / vector_obs that does not exist)
        self.config = cfg
        dev = device or cfg.device or ("cuda" if torch.cuda.is_available() else None)
        if dev is None or not torch.cuda.is_available():
            raise RuntimeError("torchdriveenv_amd needs a HIP device: there is no CPU path")
        self.torch_device = torch.device(dev if str(dev) != "cuda" else "cuda:0")
        if background is None and cfg.use_background_traffic:        # ref gym_env.py:200-203: the packaged directory
            from .loaders import pick_background_traffic
            background = pick_background_traffic                     # (searched under TORCHDRIVEENV_DATA; None if absent)
        sim = cfg.simulator
        seed = cfg.seed if cfg.seed is not None else int(np.random.randint(0, 2**31 - 1))  # ref helpers.py:39-41
        self.world = data if isinstance(data, World) else world_from_waypoint_suite(
            data, agents_per_env,
            threshold=effective_offroad_distance(sim.offroad_threshold, sim.offroad_threshold_squared),
            background=background if cfg.use_background_traffic else None, ego_only=cfg.ego_only, road_meshes=road_meshes,
            near_range=near_range, traffic_lights=traffic_lights, light_radius=light_radius, start_headings=start_headings,
            heading_samples=heading_samples, near_field=near_field if isinstance(near_field, NearField) else None,
            near_field_seed=seed)
        if isinstance(near_field, NearField):
            self.world, near_field = self.world
        if near_field is not None and (near_field.S != self.world.n_scn or near_field.A != self.world.A):
            raise ValueError(f"the near-field table is for {near_field.S} scenarios x {near_field.A} slots, the world has "
                             f"{self.world.n_scn} x {self.world.A}")
        self.near_field = near_field                                 # world.NearFieldTable or None
        # routed near-field traffic: the state carries per-slot routes (tde_state.slot_route), which only step() and the spawner know
        self._nf_routed = near_field is not None and bool(getattr(near_field, "routes", False))
        if self._nf_routed and self.planner.predict in ("route", "queue"):
            raise ValueError(f"Planner(predict={self.planner.predict!r}) with routed near-field traffic (NearField(routes=True)): the "
                             "forecasts read routes from the spawn records and would see the spawned agents stopping; use predict='constant'")
        if self._nf_routed and self.plan_react is not None:
            raise ValueError("plan_react= with routed near-field traffic (NearField(routes=True)): the reacting scene reads routes from "
                             "the spawn records and would see the spawned agents stopping")
        check_threshold(self.world, sim.offroad_threshold, sim.offroad_threshold_squared,
                        "EnvConfig.simulator.offroad_threshold")   # a prebuilt World bakes its threshold into the grid
        self.A = self.world.A
        self.num_envs = int(num_envs)
        self.seed_value = seed
        flags = _abi.F_NPC | _abi.F_REPLAY | _abi.F_OFFROAD | _abi.F_REWARD
        if auto_reset:
            flags |= _abi.F_AUTORESET
        if cfg.ego_only:
            flags |= _abi.F_EGO_ONLY_ATTRS
        if self.world.has_lights:
            flags |= _abi.F_TRAFFIC_LIGHTS
        if cfg.simulator.npc_first_step:                             # ref gym_env.py:285-294: the NPCs act from step one
            flags |= _abi.F_NPC_FIRST_STEP
        self.tde_cfg = to_tde_config(cfg, seed, flags)
        self.tde_cfg.env_base = int(env_base)                        # shard of a larger batch: sharding.ShardedBatchedEnv
        # near-field envs run without the first-step gap cache (tde_world.first_gap = NULL): it assumes the NPCs sit exactly at the
        # scenario's spawn records on the first step, which the spawner's agents make untrue
        self.dworld = self.world.to_device(self.torch_device, first_gap=near_field is None)
        self.dnf = None
        if near_field is not None:
            self.dnf = near_field.to_device(self.torch_device)
            self.dworld.near_field = self.dnf                        # (ops.env_rollout / env_step_render refuse such a world)
        self.obs_mode, self.frame_stack = obs_mode, max(1, int(frame_stack))
        r = cfg.simulator.renderer
        self._res, self._fov = int(r.res), float(r.fov)
        self._rflags = render_flags(cfg)
        self.observer = make_observer(self, vector_obs)              # (observe.py: every observation buffer and what refreshes it)
        self.vector_obs, self._after_step = self.observer.vector_obs, self.observer.after_step    # (bound once: every step() calls it)
        self.info_magnitudes = bool(info_magnitudes)
        self.state = EnvState(self.num_envs, self.A, device=self.torch_device, with_info=with_info,
                              with_obs=self.observer.state_obs, with_magnitudes=self.info_magnitudes, with_slot_route=self._nf_routed)
        self.action_space = _box(ACTION_LOW, ACTION_HIGH)
        shape, dtype = self.observer.layout
        self.observation_space = _box(0, 255, shape, np.uint8) if dtype is torch.uint8 else _box(-np.inf, np.inf, shape, np.float32)
        self._plan_out = self._plan_diag = self._refine = None
        self._plan_fc = self._plan_lat = None          # planner.predict == "route" / "queue": the forecast buffer, the lattice as one-knot sequences
        self.reward_range = (-float("inf"), float("inf"))           # ref gym_env.py:97
        self._vec = None
        self._mag = self.state["magnitudes"]                         # float32 [B, 4] written by the step (None: indicators)
        self._nf_mask = None
        # every launch goes through self._h: the extension's EnvHandle or ops.CtypesHandle, which have the same methods
        self.binding = binding
        if binding == "ext":
            from . import _ext
            self._h = _ext.env_handle(self.tde_cfg, self.dworld, self.state)
            self._hnf = _ext.near_field_of(self.dnf) if self.dnf is not None else None
        else:
            self._h, self._hnf = ops.CtypesHandle(self.tde_cfg, self.dworld, self.state), self.dnf
        # terminal_obs: the newest frame each env showed when it last finished (tde_terminal_stash), and what step() needs around it
        self.terminal_frames = self._term_mask = None
        if self.terminal_obs:
            plane = self.observer.plane                              # (0: the observation is float rows)
            if plane % 16 != 0:
                raise ValueError(f"terminal_obs=True: H * W = {plane} must be a multiple of 16 (the planes move as 16-byte words)")
            self.terminal_frames = (torch.full((self.num_envs, plane), _abi.LAYER_BLANK, dtype=torch.uint8, device=self.torch_device) if plane else
                                    torch.zeros((self.num_envs, shape[0]), dtype=torch.float32, device=self.torch_device))
            self._term_mask = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.torch_device)
        if self.dnf is None:
            # the world's first-step gap cache for this configuration, now - not inside the first step() (which may be under a stream capture)
            ops.first_gaps(self.tde_cfg, self.dworld)

    @property
    def auto_reset(self):
        return bool(self.tde_cfg.flags & _abi.F_AUTORESET)

    # ---- device-resident API ------------------------------------------------------------------------------
    def reset(self, seed=None, options=None, mask=None):
        """re-spawn all envs (or those in `mask`, uint8/bool [B]).  `seed` is ignored like in the reference
        (ref gym_env.py:107-109); seeding is EnvConfig.seed.  With a mask only the re-spawned envs' observations
        change: their newest frame is re-rendered in place and their older frames are blanked; the other envs keep
        their frame stack exactly as the last step left it.
        options={"scenario": ids}: the scenario each re-spawned env starts in (tde_env_reset_to) - an int (every env), a sequence
        or an integer tensor [B]; -1 = drawn as without the option; ids outside [-1, n_scn) raise ValueError.  Everything else of
        the episode (start point, speed, heading noise, the slots' spawn) is what the same reset would give had it drawn that
        scenario; observations, near-field traffic and the frame stack are handled as without the option.  Other keys of `options`
        are ignored, like the reference ignores them all (ref gym_env.py:107-109)."""
        m = None
        if mask is not None:
            # 0 / 1 bytes: the rasteriser reads bits 0-1 of a `fresh` byte (tde_render.fresh), so a mask like done_bits with only
            # infraction bits set must not re-spawn an env and leave its older stack frames un-blanked
            # (step() of a terminal_obs env hands over its own 0 / 1 mask: nothing to convert)
            m = mask if mask is self._term_mask else (torch.as_tensor(mask, device=self.torch_device) != 0).to(torch.uint8).contiguous()
        scn = None
        if options is not None and options.get("scenario") is not None:
            scn = ops.check_scenario_ids(options["scenario"], self.num_envs, self.world.n_scn).to(self.torch_device)
        # the SB3-style auto-reset: the re-spawn and the re-spawned views' first observation in ONE C-ABI call, where there is one
        obs = self.observer.reset_reobserve(m) if scn is None and m is not None else None
        if obs is not None:
            return obs
        if scn is not None:
            self._h.reset_to(scn, m, int(self.tde_cfg.flags))
        else:
            self._h.reset(m, int(self.tde_cfg.flags))
        self._spawn_near_field(m)                                    # (near-field envs: reset -> spawn -> render)
        if m is not None:
            return self.observer.reobserve(m)
        self.observer.clear()                                        # VecFrameStack clears the stack on reset
        return self.observer.observe()

    def _spawn_near_field(self, mask=None, done=False):
        """tde_near_field_spawn on the envs in `mask` (all: None), or - done=True - on the envs the last step finished (the
        terminated / truncated flags it left: their in-place re-spawn just happened).  No-op without a near field."""
        if self.dnf is None:
            return
        if done:
            st = self.state
            if self._nf_mask is None:
                self._nf_mask = torch.empty(self.num_envs, dtype=torch.uint8, device=self.torch_device)
            mask = torch.bitwise_or(st["terminated"], st["truncated"], out=self._nf_mask)
        self._h.near_field_spawn(self._hnf, mask, int(self.tde_cfg.flags))

    @contextlib.contextmanager
    def _without_autoreset(self):
        """tde_cfg.flags without F_AUTORESET inside the block (a step then leaves the envs it finished as they ended), restored after it"""
        full = int(self.tde_cfg.flags)
        self.tde_cfg.flags = full & ~_abi.F_AUTORESET
        try:
            yield
        finally:
            self.tde_cfg.flags = full

    def step(self, actions, agent_actions=None, driven=None):
        """driven (bool / uint8 [B, A] on the env's device) with agent_actions (float32 [B, A, 2]): the present slots a >= 1 whose mask
        entry is set take agent_actions[e, a] = (acceleration, steering) in this step as slot 0 takes actions[e] - raw units, at every
        step count, instead of the controller's result or the slot's replay record (tde_env_step_driven, include/tde_driven.h).  Row 0
        and the rows of absent or undriven slots are never read.  The mask is by slot index: an env re-spawned in the step keeps it for
        its new agents.  Only the launch differs: observations, terminal_obs, info and episode statistics are the plain step's.
        driven=None (default): the plain step."""
        # (the host side of a step is what a closed loop of small kernels waits for: no tensor op that is not needed)
        a = actions
        if not (torch.is_tensor(a) and a.dtype is torch.float32 and a.device == self.torch_device and a.dim() == 2
                and a.shape[0] == self.num_envs and a.shape[1] == 2 and a.is_contiguous()):
            a = torch.as_tensor(actions, dtype=torch.float32, device=self.torch_device).reshape(self.num_envs, 2).contiguous()
        launch = self._h.step if driven is None else self._driven_launch(agent_actions, driven)
        if self.terminal_obs and self.auto_reset:                    # (the VecEnv adapter clears the flag and re-spawns the envs itself)
            return self._step_terminal(a, launch)
        launch(a, int(self.tde_cfg.flags))
        if self.dnf is not None and self.auto_reset:
            self._spawn_near_field(done=True)                        # the envs the step re-spawned, before they are observed
        return self._result(self._after_step())

    def _driven_launch(self, agent_actions, driven):
        """the launch of a step with outside actions for the slots in `driven`, in the shape of the handle's step(action, flags): the two
        tensors are checked here, before anything is queued; the ego actions go to state["action"], which the C ABI reads; the call
        goes through ctypes under either binding (ops.env_step_driven)"""
        if self._nf_routed:
            raise ValueError("step(driven=) with routed near-field traffic (NearField(routes=True)): tde_env_step_driven refuses a state "
                             "with per-slot routes")
        ops.check_driven(agent_actions, driven, self.num_envs, self.A, self.torch_device)

        def launch(a, flags):
            self.tde_cfg.flags = flags
            act = self.state["action"]
            if a is not act:
                act.copy_(a)
            ops.env_step_driven(self.tde_cfg, self.dworld, self.state, agent_actions, driven)
        return launch

    def _result(self, obs):
        """what a step returns with the observation `obs`: the state's terminated / truncated bytes seen as bool (no copy; the views are
        formed once: the buffers never move); info entries are only computed when they are read"""
        v = self.__dict__.get("_tt_views")
        st = self.state
        if v is None or v[0] is not st["terminated"]:
            v = self._tt_views = (st["terminated"], st["terminated"].view(torch.bool), st["truncated"].view(torch.bool))
        return obs, st["reward"], v[1], v[2], _LazyInfo(st, self.num_envs, self.A, magnitudes=self._mag)

    def _step_terminal(self, a, launch):
        """step() of a terminal_obs env: the step without the in-kernel re-spawn (the kernel form WaypointVecEnv.step_wait uses) ->
        the observation, which for a finished env is its terminal one -> tde_terminal_stash of the finished envs' newest frame into
        terminal_frames -> reset(mask=done): the masked re-spawn and re-render.  Same results as step() without the option."""
        st = self.state
        with self._without_autoreset():
            launch(a, int(self.tde_cfg.flags))
            self._after_step()
        ops.terminal_stash(self.torch_device, st["done_bits"], *self.observer.newest_frame(), self.terminal_frames)
        return self._result(self.reset(mask=torch.bitwise_or(st["terminated"], st["truncated"], out=self._term_mask)))

    def _step_then_post_step(self, a):
        """the round-4 form of a step with magnitudes, kept for A/B runs and as a second witness of the fused path
        (tests/test_gpu_magnitudes.py): step without in-kernel re-spawn -> tde_env_post_step (the magnitudes of the infractions the
        step flagged + the re-spawn of the envs it finished, one launch) -> the observation.  Same results as step(), one launch
        more."""
        if self._mag is None:
            raise RuntimeError("needs info_magnitudes=True")
        full = int(self.tde_cfg.flags)                      # (WaypointVecEnv.step_wait clears F_AUTORESET: it re-spawns the envs itself)
        with self._without_autoreset():
            self._h.step(a, int(self.tde_cfg.flags))
            self._h.post_step(self._mag, full)
        if self.auto_reset:
            self._spawn_near_field(done=True)
        return self._result(self._after_step())

    def rollout(self, actions):
        """K open-loop steps from a resident [K,B,2] action tensor -> (reward [K,B], done bits [K,B]).  (The Monitor-style
        episode statistics of the closed-loop API are not maintained across a rollout: they follow from the returned
        arrays.)"""
        if self.terminal_obs:
            raise ValueError("rollout() on a terminal_obs env: the rollout kernels re-spawn finished envs inside one launch, where no "
                             "terminal observation can be taken; step() the envs instead")
        if self._nf_routed:
            raise ValueError("rollout() with routed near-field traffic (NearField(routes=True)): the rollout kernels read routes from the "
                             "spawn records; step() the envs instead")
        if self.dnf is not None:
            raise NotImplementedError("rollout() with near_field: the rollout kernels re-spawn finished envs inside one launch, where "
                                      "the near-field spawner cannot run; step() the envs instead")
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.torch_device).contiguous()
        reward = torch.empty(a.shape[:2], dtype=torch.float32, device=self.torch_device)
        done = torch.empty(a.shape[:2], dtype=torch.uint8, device=self.torch_device)
        self._h.rollout(a, reward, done, int(self.tde_cfg.flags))
        return reward, done

    def get_obs(self, fresh=None):
        return self.observer.observe(fresh)

    def plan_actions(self, out=None, only=None, diag=False):
        """the sampling planner's action for every ego on the state as it is (tde_plan_action with self.planner) -> float32 [B, 2] on
        the device, usable as step(plan_actions()).  out: a float32 [B, 2] device tensor to write into (default: the env's own
        buffer, overwritten by the next call); only: uint8 [B] on the device, the other rows are left as they are; diag=True: returns
        (actions, int32 [B, 4] rows of winner, fail_step, the cost's float32 bits, n_safe - n_safe == 0: no candidate is safe).
        With planner.predict == "route" the other agents are where tde_forecast_agents puts them (one forecast per call, horizon + tail
        steps) and the lattice is judged as one-knot sequences by tde_score_plans_forecast; with "queue" they are where tde_forecast_scene
        puts them while the ego coasts (the leader sweep kept), judged the same way; "constant" (default) is the path as it was.
        With self.plan_react the lattice is judged as one-knot sequences by tde_score_plans_scene (every candidate in a scene that
        reacts to it) with plan_react.tail steps of brake tail."""
        if out is None:
            if self._plan_out is None:
                self._plan_out = torch.zeros((self.num_envs, 2), dtype=torch.float32, device=self.torch_device)
            out = self._plan_out
        d = None
        if diag:
            if self._plan_diag is None:
                self._plan_diag = torch.zeros((self.num_envs, 4), dtype=torch.int32, device=self.torch_device)
            d = self._plan_diag
        only = self._as_only(only)
        pl = self.planner
        if self.plan_react is not None:
            la = self._plan_lattice()
            self._score_plans(la["seq"], int(pl.horizon), int(self.plan_react.tail), only, la["cost"], la["fail"], out, d, react=True)
            return (out, d) if diag else out
        fc = None
        if pl.predict in ("route", "queue"):
            T = int(pl.horizon) + (int(self.plan_refine.tail) if self.plan_refine is not None else 0)
            if self._plan_fc is None:
                self._plan_fc = self._forecast_args(T, only, None)[0]
            fc = self._plan_fc
            if pl.predict == "route":
                self._h.forecast_agents(fc, only, int(self.tde_cfg.flags))
            else:
                self._h.forecast_scene(fc, None, only, int(self.tde_cfg.flags))
        if self.plan_refine is not None:
            if self._plan_diag is None:
                self._plan_diag = torch.zeros((self.num_envs, 4), dtype=torch.int32, device=self.torch_device)
            self._plan_refined(out, only, self._plan_diag, fc)
            return (out, self._plan_diag) if diag else out
        if fc is not None:
            la = self._plan_lattice()
            self._score_plans(la["seq"], int(pl.horizon), 0, only, la["cost"], la["fail"], out, d, fc)
            return (out, d) if diag else out
        self._h.plan_action(out, [float(v) for v in pl.accelerations], [float(v) for v in pl.steerings], *self._plan_scalars(), only, d,
                            int(self.tde_cfg.flags))
        return (out, d) if diag else out

    def _plan_lattice(self):
        """the planner's lattice as one-knot sequences [B, nc, 1, 2] with their cost / fail_step buffers (made once)"""
        if self._plan_lat is None:
            B, nc, dev = self.num_envs, self.planner.n_candidates, self.torch_device
            self._plan_lat = {"seq": self._lattice(1)[1],
                              "cost": torch.zeros((B, nc), dtype=torch.float32, device=dev),
                              "fail": torch.zeros((B, nc), dtype=torch.int32, device=dev)}
        return self._plan_lat

    def _lattice(self, K):
        """the planner's lattice -> (float32 [nc, 2] on the host, candidate i = ia * n_s + is; the same as sequences of K equal knots,
        float32 [B, nc, K, 2] on the device, contiguous)"""
        acc, ste = self.planner.tables()
        lat = np.stack([np.repeat(acc, len(ste)), np.tile(ste, len(acc))], -1).astype(np.float32)
        seq = torch.from_numpy(lat).to(self.torch_device)[None, :, None, :].expand(self.num_envs, len(lat), K, 2).contiguous()
        return lat, seq

    def _as_only(self, only):
        """an `only` mask as the uint8 [B] device tensor the entry points read (None stays None)"""
        return None if only is None else torch.as_tensor(only, device=self.torch_device).to(torch.uint8)

    def _plan_scalars(self):
        """self.planner's (horizon, v_target, margin, w_progress, w_speed, w_steer) as the extension takes them"""
        pl = self.planner
        return int(pl.horizon), float(pl.v_target), float(pl.margin), float(pl.w_progress), float(pl.w_speed), float(pl.w_steer)

    def _score_plans(self, seq, knot_len, tail, only, cost, fail_step, action, diag, forecast=None, react=False):
        """tde_score_plans (forecast: tde_score_plans_forecast; react: tde_score_plans_scene) through the env's handle (arguments
        already checked)"""
        args = (seq, knot_len, tail, cost, fail_step, *self._plan_scalars(), only, action, diag, int(self.tde_cfg.flags))
        if react:
            self._h.score_plans_scene(*args)
        else:
            self._h.score_plans(*args, forecast)

    def _forecast_args(self, T, only, out):
        """what forecast_agents() and forecast_scene() share: T (None: the planner's horizon) an integer in range, `out` checked, or
        allocated - zeroed when `only` leaves rows unwritten -, `only` as the entry points read it -> (out, only)"""
        T = int(self.planner.horizon) if T is None else T
        if int(T) != T or not 1 <= int(T) <= _abi.FORECAST_MAX_T:
            raise ValueError(f"T must be an integer in [1, {_abi.FORECAST_MAX_T}]")
        shape = (self.num_envs, int(T), self.A, 4)
        if out is None:
            out = (torch.empty if only is None else torch.zeros)(shape, dtype=torch.float32, device=self.torch_device)
        elif not torch.is_tensor(out) or out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 tensor of shape {shape}")
        return out, self._as_only(only)

    def forecast_scene(self, T=None, ego_actions=None, only=None, out=None):
        """where the environment's own rules put EVERY agent, the ego included, at each of the next T steps when the ego takes
        `ego_actions` (tde_forecast_scene) -> float32 [B, T, A, 4] on the device: row [e, h - 1, j] = (x, y, psi, v) of slot j at
        environment step steps[e] + h; row 0 is the ego's pose; zeros for absent slots.  Unlike forecast_agents() the controller's leader
        sweep is kept: NPCs queue behind one another and behind the ego, so the next T step() calls with these actions leave exactly
        these rows, bit for bit, for as long as the env does not re-spawn (nothing is judged here: rows past an episode's end go on
        as if it had not ended).  T: 1 .. 96 (None: the planner's horizon); ego_actions: a contiguous float32 [B, T, 2] device tensor of
        (acceleration, steering), taken as given - no clamp, no scaling; None: the ego coasts; only: uint8 [B], the other envs' rows
        are left as they are (zeros in a fresh buffer); out: a float32 [B, T, A, 4] device tensor to write into.  The state is not
        written.  score_plans(forecast=) takes the result (it ignores row 0)."""
        out, only = self._forecast_args(T, only, out)
        if ego_actions is not None:
            ops.check_ego_actions(ego_actions, self.num_envs, out.shape[1])
            if ego_actions.device != self.torch_device:
                raise ValueError(f"ego_actions is on {ego_actions.device}, expected {self.torch_device}")
        self._h.forecast_scene(out, ego_actions, only, int(self.tde_cfg.flags))
        return out

    def forecast_agents(self, T=None, only=None, out=None):
        """where the environment's own rules put every other agent at each of the next T steps when nobody is in its cone
        (tde_forecast_agents) -> float32 [B, T, A, 4] on the device: row [e, h - 1, j] = (x, y, psi, v) of slot j at environment step
        steps[e] + h; zeros for the ego (slot 0) and absent slots.  Replayed agents follow their records, NPCs their routes, braking
        for red lines and at the route's end; an agent that meets nobody does exactly this in the next T step() calls.  T: 1 .. 96
        (None: the planner's horizon); only: uint8 [B], the other envs' rows are left as they are (zeros in a fresh buffer); out: a
        float32 [B, T, A, 4] device tensor to write into (16 * B * T * A bytes the caller keeps).  score_plans(forecast=) takes the
        result."""
        out, only = self._forecast_args(T, only, out)
        self._h.forecast_agents(out, only, int(self.tde_cfg.flags))
        return out

    def score_plans(self, seq, knot_len=None, tail=0, only=None, forecast=None, react=False):
        """how each of N action sequences per ego fares on the state as it is (tde_score_plans with self.planner's horizon, margin,
        v_target and weights) -> (cost float32 [B, N], fail_step int32 [B, N]) on the device.  seq: float32 [B, N, K, 2] device tensor
        of (acceleration, steering) knots, contiguous (raises otherwise: no copy is made); knot k holds knot_len steps (None:
        ceil(horizon / K)), the last one to the end of the horizon; then `tail` steps of full braking.  fail_step is the first step
        off the road, on a predicted box of another agent or on a red stop line, horizon + tail + 1 for a safe sequence; a lower cost
        is better and any earlier failure costs more than any later one.  only: uint8 [B]; the other rows are not written.
        forecast: a contiguous float32 [B, T >= horizon + tail, A, 4] device tensor of the other agents' (x, y, psi, v) per step -
        forecast_agents()'s, or any predictor's in that layout - judged through tde_score_plans_forecast; None: constant velocity.
        react=True: every sequence is judged in a scene of its own in which the other agents run the controller against the ego that
        follows it (tde_score_plans_scene; no forecast is materialised): with planner.margin == 0 fail_step is the step at which
        step() would end the episode by an infraction under those actions.  Not together with forecast=."""
        if react and forecast is not None:
            raise ValueError("score_plans: react=True builds its own scene per sequence; forecast= cannot be given with it")
        N, K, knot_len, tail = ops.check_plan_set(seq, self.num_envs, self.planner.horizon, knot_len, tail)
        if react and self.num_envs * N * self.A > _abi.PLAN_SCENE_MAX_LANES:
            raise ValueError(f"score_plans: react=True needs num_envs * N * A <= {_abi.PLAN_SCENE_MAX_LANES}")
        if forecast is not None:
            ops.check_forecast(forecast, self.num_envs, self.A, int(self.planner.horizon) + tail)
        only = self._as_only(only)
        cost = torch.zeros((self.num_envs, N), dtype=torch.float32, device=self.torch_device)
        fail_step = torch.zeros((self.num_envs, N), dtype=torch.int32, device=self.torch_device)
        self._score_plans(seq, knot_len, tail, only, cost, fail_step, None, None, forecast, react=bool(react))
        return cost, fail_step

    def _plan_refined(self, out, only, diag, forecast=None):
        """plan_actions() under self.plan_refine (config.PlanRefine states the rounds): device work only, no synchronisation"""
        pl, pr = self.planner, self.plan_refine
        B, nc, K, R = self.num_envs, pl.n_candidates, int(pr.knots), int(pr.rounds)
        dev = self.torch_device
        if self._refine is None:
            lat, seq0 = self._lattice(K)
            rf = {"seq0": seq0,
                  "cost0": torch.zeros((B, nc), dtype=torch.float32, device=dev), "fail0": torch.zeros((B, nc), dtype=torch.int32, device=dev),
                  "lo": torch.tensor([-_abi.PLAN_BOX_ACCEL, -_abi.PLAN_BOX_STEER], dtype=torch.float32, device=dev),
                  "hi": torch.tensor([_abi.PLAN_BOX_ACCEL, _abi.PLAN_BOX_STEER], dtype=torch.float32, device=dev)}
            if R:
                s, deltas = np.float32(1.0), []
                for _ in range(R):
                    s = np.float32(s * np.float32(pr.shrink))
                    deltas.append(lat * s)
                rf["delta"] = torch.from_numpy(np.stack(deltas)).to(dev)                                        # [R, nc, 2]
                rf["cand"] = torch.zeros((B, K * nc, K, 2), dtype=torch.float32, device=dev)
                rf["cost"] = torch.zeros((B, K * nc), dtype=torch.float32, device=dev)
                rf["fail"] = torch.zeros((B, K * nc), dtype=torch.int32, device=dev)
            self._refine = rf
        rf = self._refine
        knot_len, tail = -(-int(pl.horizon) // K), int(pr.tail)
        self._score_plans(rf["seq0"], knot_len, tail, only, rf["cost0"], rf["fail0"], out, diag, forecast)
        seqs = rf["seq0"]
        for r in range(R):
            # (rows outside `only` keep an older winner in diag: clamped, their candidates are built and never judged)
            win = diag[:, 0].long().clamp_(0, seqs.shape[1] - 1)
            w = torch.gather(seqs, 1, win.view(B, 1, 1, 1).expand(B, 1, K, 2)).squeeze(1)                       # [B, K, 2]
            cv = rf["cand"].view(B, K, nc, K, 2)
            cv.copy_(w[:, None, None, :, :].expand(B, K, nc, K, 2))
            for k in range(K):
                cv[:, k, :, k, :] = torch.minimum(torch.maximum(w[:, k, None, :] + rf["delta"][r][None], rf["lo"]), rf["hi"])
            seqs = rf["cand"]
            self._score_plans(seqs, knot_len, tail, only, rf["cost"], rf["fail"], out, diag, forecast)

    def evaluate(self, policy, cases=None, repeats=1):
        """run `policy` once (or `repeats` times) on each of the scenarios `cases` (default: every scenario of the world) and
        collect whole-episode results on the device -> EvalResult: what the reference's EvalNTimestepsCallback does with its
        eval env over validation_cases.yml (ref examples/rl_training.py:39-108), with the cases chosen instead of drawn.
        policy: a callable observation -> float32 [B, 2] actions on the device (it sees the observation of every env, idle ones
        included), or "planner" (plan_actions()).  The job list is `cases` repeated `repeats` times; job j runs on env j % B as that
        env's (j // B)-th episode, so for a deterministic policy the results do not depend on timing.  Per step: the step without
        in-kernel re-spawn, tde_eval_advance (fold the step into the running records, record finished episodes, re-spawn their envs
        to the next planned scenario), the near-field spawner and the observation rows of the envs just re-spawned.  The host looks
        at the `active` flags every 8 steps; at most ceil(jobs / B) * max_steps steps are made.  An episode ends with terminated |
        truncated (the callback's `infraction or is_success` under terminated_at_infraction=True).
        The env is left mid-evaluation (finished envs are not re-spawned at the end): reset() it before training on it again, or
        evaluate on a second env as the reference does."""
        if self.state["info"] is None:
            raise ValueError("evaluate() needs with_info=True (the per-step psi / speed smoothness and the done bits)")
        if not (callable(policy) or (isinstance(policy, str) and policy == "planner")):
            raise ValueError("policy must be a callable obs -> actions [B, 2] or 'planner'")
        B, S, dev = self.num_envs, self.world.n_scn, self.torch_device
        plan, jobs = eval_plan(S, B, cases, repeats)
        ev = ops.EvalBuffers(plan, dev)
        ev.active.copy_((ev.plan[0] >= 0).to(torch.uint8))
        obs = self.reset(options={"scenario": ev.plan[0].clamp(min=-1)})
        st = self.state
        respawned = torch.empty(B, dtype=torch.uint8, device=dev)
        with self._without_autoreset():
            flags = int(self.tde_cfg.flags)
            for t in range(ev.R * int(self.tde_cfg.max_steps)):
                if t % 8 == 0 and not bool(ev.active.any()):
                    break
                a = self.plan_actions() if isinstance(policy, str) else policy(obs)
                obs = self.step(a)[0]
                self._h.eval_advance(ev.plan, ev.round, ev.active, ev.acc, ev.results, flags)
                if self.dnf is not None or not self.observer.state_obs:
                    # the envs the advance re-spawned: finished at this step and still evaluating (it rewrites a state observation's rows itself)
                    torch.bitwise_or(st["terminated"], st["truncated"], out=respawned).bitwise_and_(ev.active)
                    self._spawn_near_field(respawned)
                    if not self.observer.state_obs:
                        obs = self.observer.reobserve(respawned)
        if bool(ev.active.any()):
            raise RuntimeError("evaluate(): envs still active after ceil(jobs / B) * max_steps steps")
        return EvalResult.from_records(ev.records().reshape(-1)[:len(jobs)], jobs)

    def get_info(self):
        """info schema of the reference (ref gym_env.py:419-437), one entry per env; a mapping whose tensors are formed
        on first access (a training loop that never reads `psi_smoothness` does not pay for it)"""
        return _LazyInfo(self.state, self.num_envs, self.A, magnitudes=self._mag)

    def render_scene(self, envs=None, H=1024, W=1024, fov=500.0, camera="map", out=None):
        """uint8 [n, 3, H, W] on the device: view i of env envs[i] (default: every env) at any H, W in [1, 4096] from `camera` ("map":
        the centre of the env's map, heading pi/2 - an UNPINNED reading of torchdrivesim's default camera; "ego": slot 0's pose; or a
        float32 tensor [n, 3] of (x, y, psi)), with this env's render flags, on the current stream: the frames of the reference's
        render_mode="video" (BirdviewRecordingWrapper, ref gym_env.py:295-297), which this batched API does not take as a mode
        (ops.render_scene)."""
        return ops.render_scene(self.tde_cfg, self.dworld, self.state, envs, H, W, fov, camera, out, flags=self._rflags)

    def render_agents(self, envs, slots, H=64, W=64, fov=None):
        """uint8 [n, 3, H, W] on the device: the birdview centred on slot slots[i] of env envs[i], its heading up - the observation a
        policy that drives that slot (step(driven=)) can use.  The tde_scene_view rows are gathered on the device from the state and
        handed to tde_render_scene with this env's render flags; fov defaults to the ego observation's.  Slot 0 stays painted as the
        ego whichever slot the view is centred on; an absent slot gives the view from the pose its row holds.  envs and slots are
        integer sequences or tensors of one length, envs in [0, B), slots in [0, A) (checked on the host)."""
        dev = self.torch_device
        envs = torch.as_tensor(envs, dtype=torch.int64).reshape(-1)
        slots = torch.as_tensor(slots, dtype=torch.int64).reshape(-1)
        if envs.numel() != slots.numel():
            raise ValueError(f"envs and slots must have one length, got {envs.numel()} and {slots.numel()}")
        if envs.numel() and not bool(((envs >= 0) & (envs < self.num_envs)).all()):
            raise ValueError(f"envs must be in [0, {self.num_envs})")
        if slots.numel() and not bool(((slots >= 0) & (slots < self.A)).all()):
            raise ValueError(f"slots must be in [0, {self.A})")
        H, W = int(H), int(W)
        if not (1 <= H <= 4096 and 1 <= W <= 4096):
            raise ValueError("H and W must be in [1, 4096]")
        fov = self._fov if fov is None else float(fov)
        if not (np.isfinite(fov) and fov > 0):
            raise ValueError("fov must be finite and positive")
        envs, slots = envs.to(dev), slots.to(dev)
        n = envs.numel()
        out = torch.empty((n, 3, H, W), dtype=torch.uint8, device=dev)
        if n == 0:
            return out
        g = envs * self.A + slots
        views = torch.empty((n, 4), dtype=torch.int32, device=dev)
        views[:, 0] = envs
        pose = views[:, 1:].view(torch.float32)                      # (the state's own bits)
        pose[:, 0], pose[:, 1], pose[:, 2] = self.state["x"][g], self.state["y"][g], self.state["psi"][g]
        return ops.render_scene_views(self.tde_cfg, self.dworld, self.state, views, H, W, fov, out, flags=self._rflags)

    def agents(self, envs, slots, vector_obs=None):
        """an AgentGroup over slot slots[i] of env envs[i]: the vector observation from those slots and, after the step(s) that follow,
        each one's reward and flags - with step(driven=) the loop of a policy that drives them (tde_agent_obs / tde_agent_outcomes,
        include/tde_agents.h).  vector_obs: a config.VectorObs (or a dict of its fields); default: this env's (obs_mode="vector"), else
        VectorObs().  Works under every obs_mode.  envs and slots are integer sequences or tensors of one length, envs in [0, B), slots
        in [0, A) (checked on the host); duplicates are allowed."""
        envs = torch.as_tensor(envs, dtype=torch.int64).reshape(-1).cpu()
        slots = torch.as_tensor(slots, dtype=torch.int64).reshape(-1).cpu()
        if envs.numel() != slots.numel():
            raise ValueError(f"envs and slots must have one length, got {envs.numel()} and {slots.numel()}")
        if envs.numel() and not bool(((envs >= 0) & (envs < self.num_envs)).all()):
            raise ValueError(f"envs must be in [0, {self.num_envs})")
        if slots.numel() and not bool(((slots >= 0) & (slots < self.A)).all()):
            raise ValueError(f"slots must be in [0, {self.A})")
        vo = vector_obs if vector_obs is not None else (self.vector_obs if self.vector_obs is not None else VectorObs())
        pairs = torch.stack([envs, slots], -1).to(torch.int32).contiguous().to(self.torch_device)
        return AgentGroup(self, pairs, check_vector_obs(vo))

    def render(self):
        """(B, H, W, 3) uint8 of the current ego views (ref gym_env.py:152-155)"""
        img = ops.render_ego(self.tde_cfg, self.dworld, self.state, self._res, self._res, self._fov, 1, flags=self._rflags)
        return img.permute(0, 2, 3, 1).cpu().numpy()

    def close(self):
        pass

    def state_dict(self):
        """snapshot of every mutable buffer (checkpoint / parity replays), the frame-stack ring included"""
        sd = {k: v.clone() for k, v in self.state.arrays.items() if v is not None}
        ring = self.observer.state_dict()
        if ring is not None:
            sd["_frame_stack"] = ring
        if self.terminal_frames is not None:
            sd["_terminal_frames"] = self.terminal_frames.clone()
        return sd

    def load_state_dict(self, sd):
        for k, v in sd.items():
            if k == "_frame_stack":
                self.observer.load_state_dict(v)
            elif k == "_terminal_frames":
                if self.terminal_frames is None:
                    raise ValueError("the state holds terminal frames, this env was built without terminal_obs=True")
                self.terminal_frames.copy_(v)
            else:
                self.state.arrays[k].copy_(v)

    # ---- per-env snapshots, forks and recordings (snapshot.py, include/tde_snapshot.h) ---------------------
    def snapshot(self, envs):
        """the rows of the envs `envs` (indices, no duplicates) as they are now -> snapshot.EnvSnapshot: an EnvState of len(envs) rows
        without caches - the step's outputs included - with the rows of the frame-stack ring and stacked observation (or of the single
        birdview frame, or of the vector observation) and of the terminal frames, and the indices it was taken from.  One tde_state_copy
        launch (plus a torch gather for vector observations and terminal frames); the live state, the sample counters of buffers and
        the observation are untouched.  Every per-env buffer the env holds is in it (snapshot.py lists them); replay and rollout
        buffers are not."""
        from . import snapshot as S

        return S.EnvSnapshot(self, envs)

    def restore(self, snap, envs=None):
        """put the rows of `snap` back into the envs `envs` (default: the indices they were taken from) and return the observation
        buffer, whose rows for those envs are the saved ones - what the last step() / reset() before the snapshot returned for them.
        (get_obs() of a frame-stacked env pushes a new frame onto every env's stack, as it always has: use the returned buffer.)  The
        step's caches of the rows are invalidated in the same launch.  The RNG rule: the re-spawn draws are keyed by (seed, global env
        index, episode counter) and nothing else is keyed by the index, so a row restored into its own index continues bit for bit for
        ever, and a row put into another index continues bit for bit until that env next re-spawns.  A snapshot taken from an env with
        other options (observation mode, frame stack, resolution, info / magnitudes / routed near field, terminal_obs) raises
        ValueError naming what does not fit."""
        from . import snapshot as S

        return S.restore(self, snap, envs)

    def fork(self, src_env, dst_envs):
        """copy env `src_env` into the envs `dst_envs` (which must not hold src_env) within the live state, frames included, in one
        launch -> the observation buffer.  The copies continue bit for bit like the source until they next re-spawn (restore()'s RNG
        rule); give them different actions to branch."""
        from . import snapshot as S

        return S.fork(self, src_env, dst_envs)

    def recorder(self, envs, video_length=200):
        """a snapshot.EpisodeRecorder of the envs `envs`: capture() after each reset() / step() records their state rows (one launch, no
        rendering), frames() / save() render them later with the scene renderer.  Nothing is allocated before this call."""
        from . import snapshot as S

        return S.EpisodeRecorder(self, envs, video_length)

    def replay_buffer(self, capacity_steps, seed=None, terminal_per_step=None, prioritized=None):
        """a replay.ReplayBuffer of `capacity_steps` time slots bound to this env (index draws seeded by `seed`; None: the env's seed).
        On a terminal_obs env the buffer also keeps up to `terminal_per_step` terminal frames per step (None: max(1, num_envs // 8));
        that pool costs capacity_steps * terminal_per_step * (H * W, or 4 * D) bytes beside the ring's capacity_steps * num_envs * ... -
        an eighth more by default - plus 4 * capacity_steps * num_envs bytes of references.  Without the option it must be None.
        prioritized: a config.Prioritized - the buffer keeps an integer priority per transition (4 bytes, and an eighth of a byte of
        sums) and offers sample_prioritized() / update_priorities(); None: nothing is allocated and nothing about the buffer changes."""
        from .replay import ReplayBuffer

        return ReplayBuffer(self, capacity_steps, seed=self.seed_value if seed is None else seed, terminal_per_step=terminal_per_step,
                            prioritized=prioritized)

    def rollout_buffer(self, n_steps, gamma=0.99, gae_lambda=0.95, seed=None, terminal_per_step=None):
        """an onpolicy.RolloutBuffer of `n_steps` steps bound to this env (minibatch permutations seeded by `seed`; None: the env's seed;
        terminal_per_step: as replay_buffer's, for the ring behind it)"""
        from .onpolicy import RolloutBuffer

        return RolloutBuffer(self, n_steps, gamma=gamma, gae_lambda=gae_lambda, seed=seed, terminal_per_step=terminal_per_step)

    # ---- SB3 VecEnv-shaped numpy API --------------------------------------------------------------------
    def as_vec_env(self, **kw):
        """the SB3 `VecEnv` over this batch (one shared adapter per env object)"""
        if self._vec is None:
            self._vec = WaypointVecEnv(self, **kw)
        return self._vec

    def step_async(self, actions):
        self.as_vec_env().step_async(actions)

    def step_wait(self):
        return self.as_vec_env().step_wait()

    def vec_step(self, actions):
        return self.as_vec_env().step(actions)

    def vec_reset(self):
        return self.as_vec_env().reset()


try:  # optional: stable_baselines3 does not ship in this image
    from stable_baselines3.common.vec_env import VecEnv as _SB3VecEnv
except Exception:  # pragma: no cover
    _SB3VecEnv = None


class LazyInfos:
    """The `infos` list of a VecEnv step (one mapping per env) without building num_envs dicts per step: entry i is
    assembled from the per-env arrays when it is read.  Behaves like a list of dicts for the consumers SB3 has
    (`infos[i]`, iteration, `len`, `.get("episode")`, `.get("terminal_observation")`, `.get("TimeLimit.truncated")`)."""

    INFO_COLS = ("psi_smoothness", "speed_smoothness", "psi_reward", "dist_reward")

    def __init__(self, n, cols, terminal):
        self._n, self._cols, self._terminal = n, cols, terminal   # cols: name -> [n] array; terminal: env -> extra entries
        self._made = {}                                           # env -> the dict handed out (writes to it stick)

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(self._n))]
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        d = self._made.get(i)
        if d is None:
            # the SAME dict on every access: SB3 wrappers rewrite infos[i]["terminal_observation"] in step_wait
            # (VecNormalize, VecTransposeImage, VecFrameStack) and read it back through infos[i] later
            d = {k: v[i].item() for k, v in self._cols.items()}
            extra = self._terminal.get(i)
            if extra:
                d.update(extra)
            self._made[i] = d
        return d

    def __setitem__(self, i, d):
        if i < 0:
            i += self._n
        if not 0 <= i < self._n:
            raise IndexError(i)
        self._made[i] = d

    @property
    def columns(self):
        """name -> per-env array of every info column (what ShardedBatchedEnv concatenates)"""
        return self._cols

    @property
    def terminal(self):
        """env -> the extra entries of the envs that finished at this step (terminal_observation, episode)"""
        return self._terminal

    def __iter__(self):
        return (self[i] for i in range(self._n))

    def column(self, key):
        """the whole per-env column of `key` as one array (what a vectorised consumer should read)"""
        return self._cols[key]


class LazyTerminal:
    """env -> the extra info entries of the envs that finished at a step (`terminal_observation`, Monitor's `episode`), as a
    read-only mapping that builds an entry when it is asked for: at 8192 envs some env finishes at every step, and a dict per
    finished env per step was a Python loop on the step's critical path.  `idx`: the finished envs, ascending; `obs_of(n)`: the
    terminal observation of the n-th of them; ep_r / ep_l: per-ENV arrays (or None)."""

    def __init__(self, idx, obs_of, ep_r, ep_l, t):
        self._idx, self._obs_of, self._r, self._l, self._t = idx, obs_of, ep_r, ep_l, t

    def _n(self, i):
        n = int(np.searchsorted(self._idx, i))
        return n if n < len(self._idx) and self._idx[n] == i else None

    def get(self, i, default=None):
        n = self._n(i)
        if n is None:
            return default
        ex = {"terminal_observation": self._obs_of(n)}
        if self._r is not None:                                  # Monitor: round(sum(rewards), 6), len(rewards), elapsed
            ex["episode"] = {"r": round(float(self._r[i]), 6), "l": int(self._l[i]), "t": self._t}
        return ex

    def __contains__(self, i):
        return self._n(i) is not None

    def __len__(self):
        return len(self._idx)

    def __iter__(self):
        return (int(i) for i in self._idx)

    def __getitem__(self, i):
        ex = self.get(i)
        if ex is None:
            raise KeyError(i)
        return ex

    def keys(self):
        return [int(i) for i in self._idx]

    def items(self):
        return ((int(i), self.get(int(i))) for i in self._idx)


class WaypointVecEnv(_SB3VecEnv if _SB3VecEnv is not None else object):
    """stable_baselines3 `VecEnv` over a BatchedWaypointEnv, replacing `SubprocVecEnv` + `Monitor` + `VecFrameStack` of the
    reference's trainer (ref examples/rl_training.py:121-129, 159-160): numpy actions in, (obs, rewards, dones, infos)
    out, finished envs re-spawned at once with `terminal_observation`, `TimeLimit.truncated` and Monitor's
    `episode = {"r", "l", "t"}` in their info.  Subclasses SB3's VecEnv when stable_baselines3 is importable; otherwise
    the same methods on a plain class (tests/test_features_cpu.py walks the abstract interface).

    Per step: one fused step launch, one observation launch, ONE packed device-to-host copy of all per-env outputs and
    one of the observation, one stream synchronisation; `infos` is a LazyInfos.  copy_obs=False hands out views of
    rings of three pinned buffers (observations, rewards, info columns and terminal observations stay valid for the two following
    steps) instead of fresh arrays.  With the compact observation (obs_mode="state") a step is ONE stream synchronisation, the
    re-spawn of the finished envs included; the birdview needs a second one for the re-spawned envs' first frames."""

    def __init__(self, env, copy_obs=True, info_keywords=("offroad", "collision", "traffic_light_violation", "is_success",
                                                           "reached_waypoint_num", "psi_smoothness", "speed_smoothness",
                                                           "psi_reward", "dist_reward"), obs_buffers=None,
                 record_video_trigger=None, video_length=200, video_folder=None):
        """record_video_trigger / video_length / video_folder: stable_baselines3's VecVideoRecorder (ref examples/rl_training.py:163-164)
        built in - a callable step -> bool; when it holds after reset() (step 0) or after a step, the state rows of the next video_length
        frames are recorded on the device (one launch per step, snapshot.EpisodeRecorder) and then rendered and written to
        `video_folder` as rl-video-step-{start}-to-step-{start + video_length}.mp4, all envs tiled (snapshot.VecRecording; `recording`).
        A finished env was re-spawned before the frame is taken, as under SB3's recorder.  None (default): nothing is allocated and
        nothing changes.
        obs_buffers: optional list of host tensors (pinned, or page-locked by the caller with hipHostRegister) of the
        observation's shape to use as the ring the device-to-host copies land in - how a shard of ShardedBatchedEnv lets
        its observations arrive directly in its slice of the gathered buffer"""
        import time

        self.env = env
        if _SB3VecEnv is not None:
            _SB3VecEnv.__init__(self, env.num_envs, env.observation_space, env.action_space)
        else:
            self.num_envs, self.observation_space, self.action_space = env.num_envs, env.observation_space, env.action_space
            self.reset_infos = [{} for _ in range(env.num_envs)]
            self._seeds = [None] * env.num_envs
            self._options = [{} for _ in range(env.num_envs)]
        self.render_mode = "rgb_array"
        self.copy_obs = bool(copy_obs)
        self.info_keywords = tuple(k for k in info_keywords
                                   if env.state["info"] is not None or k not in LazyInfos.INFO_COLS + ("reached_waypoint_num",))
        self._t_start = time.time()
        self._pending = None
        shape, odt = env.observer.layout
        shape = (env.num_envs,) + shape
        if obs_buffers is not None:
            for b in obs_buffers:
                if tuple(b.shape) != shape or b.dtype != odt or b.is_cuda or not b.is_contiguous():
                    raise ValueError(f"obs_buffers must be contiguous host tensors of shape {shape} and dtype {odt}")
            self._obs_ring = list(obs_buffers)
        else:
            self._obs_ring = [torch.empty(shape, dtype=odt, pin_memory=True) for _ in range(1 if copy_obs else 3)]
        self._turn = 0
        self._act_pin = self._act_np = self._act_dev = None
        self._obs2_ring = None
        self.recording, self._step_id = None, 0
        if record_video_trigger is not None:
            from .snapshot import VecRecording

            self.recording = VecRecording(env, record_video_trigger, video_length, video_folder)

    # ---- helpers
    def _obs_to_host(self, obs, rows=None):
        buf = self._obs_ring[self._turn % len(self._obs_ring)]
        buf.copy_(obs, non_blocking=True)
        return buf

    def reset(self):
        obs = self.env.reset()
        buf = self._obs_to_host(obs)
        torch.cuda.current_stream(self.env.torch_device).synchronize()
        self._turn += 1
        self.reset_infos = [{} for _ in range(self.num_envs)]
        if self.recording is not None:
            self.recording.after(self._step_id)
        out = buf.numpy()
        return out.copy() if self.copy_obs else out

    def plan_actions(self, only=None, diag=False):
        """the sampling planner's actions on the current state (BatchedWaypointEnv.plan_actions) as a float32 [B, 2] numpy array, what
        step() takes; diag=True: (actions, int32 [B, 4] diag rows)"""
        r = self.env.plan_actions(only=only, diag=diag)
        return (r[0].cpu().numpy(), r[1].cpu().numpy()) if diag else r.cpu().numpy()

    def step_async(self, actions):
        self._pending = np.asarray(actions, dtype=np.float32)

    def step_wait(self):
        import time

        if self._pending is None:
            raise RuntimeError("step_wait() without step_async()")
        env = self.env
        st = env.state
        acts, self._pending = self._pending, None
        auto = env.auto_reset
        # the actions cross the bus from a pinned staging buffer, asynchronously (a pageable source makes the copy synchronous)
        if self._act_pin is None:
            self._act_pin = torch.empty((self.num_envs, 2), dtype=torch.float32, pin_memory=True)
            self._act_np = self._act_pin.numpy()
            self._act_dev = torch.empty((self.num_envs, 2), dtype=torch.float32, device=env.torch_device)
        self._act_np[...] = acts.reshape(self.num_envs, 2)
        self._act_dev.copy_(self._act_pin, non_blocking=True)
        # terminal_observation needs the pre-reset frame: run the step without in-kernel reset, then re-spawn the
        # finished envs with the masked reset kernel
        with env._without_autoreset():
            obs, _, _, _, _ = env.step(self._act_dev)
        one_sync = auto and env.obs_mode == "state" and env.binding == "ext"
        pre = None
        if one_sync:
            # compact observation: the observation the step left goes to an internal ring (the finished envs' terminal
            # observations), then the re-spawn of the finished envs (tde_env_post_step: one launch, it rewrites exactly their
            # observation rows) and the copy of the 32-byte rows into the caller-visible ring are queued behind it - ONE
            # synchronisation per step, no mask upload, no gather of the finished rows (round 4: two synchronisations per step)
            if self._obs2_ring is None:
                self._obs2_ring = [torch.empty(self._obs_ring[0].shape, dtype=self._obs_ring[0].dtype, pin_memory=True) for _ in range(3)]
            pre = self._obs2_ring[self._turn % 3]
            pre.copy_(obs, non_blocking=True)
            st.copy_outputs_async(ring=3)                            # ONE copy of every per-env output, queued (no synchronisation yet)
            env._h.post_step(None, int(env.tde_cfg.flags))
            env._spawn_near_field(done=True)                         # (near field: the re-spawned envs' traffic, still one synchronisation)
            buf = self._obs_to_host(st["obs"])
        else:
            buf = self._obs_to_host(obs)
            st.copy_outputs_async(ring=3)
        torch.cuda.current_stream(env.torch_device).synchronize()
        out = st.outputs_views()
        self._turn += 1
        obs_np = buf.numpy()
        pre_np = pre.numpy() if one_sync else obs_np                 # the observation the step left (terminal for the finished envs)
        term, trunc = out["terminated"].view(np.bool_), out["truncated"].view(np.bool_)      # (0 / 1 bytes seen as bool: no copy)
        done = term | trunc
        bits = out.get("done_bits")
        cols = {"TimeLimit.truncated": trunc & ~term}
        mag = out.get("magnitudes")                                  # (the reference's magnitudes, part of the same packed copy)
        for k in self.info_keywords:
            if k == "offroad":
                cols[k] = mag[:, 0] if mag is not None else ((bits >> 2) & 1).astype(np.float32) if bits is not None else None
            elif k == "collision":
                cols[k] = mag[:, 1] if mag is not None else ((bits >> 3) & 1).astype(np.float32) if bits is not None else None
            elif k == "traffic_light_violation":
                cols[k] = out["tl_violation"].astype(np.float32)
            elif k == "is_success":
                cols[k] = trunc
            elif k == "reached_waypoint_num":
                cols[k] = out["info_reached"]
            else:
                cols[k] = out["info"][:, LazyInfos.INFO_COLS.index(k)]
        cols = {k: v for k, v in cols.items() if v is not None}
        rew = out["reward"]
        if self.copy_obs:                                            # fresh arrays: nothing handed out aliases a staging buffer
            cols = {k: v.copy() for k, v in cols.items()}
            rew = rew.copy()
        terminal = {}
        idx = np.flatnonzero(done)
        if len(idx):
            ep_r, ep_l = out.get("ep_final"), out.get("ep_final_len")
            t = round(time.time() - self._t_start, 6)
            if one_sync and not self.copy_obs:
                obs_of = lambda n: pre_np[idx[n]]                    # noqa: E731  (a view of the internal ring: valid for the next two steps)
            else:
                term_rows = pre_np[idx]                              # (fancy index: a copy, taken before the rows are overwritten below)
                obs_of = lambda n: term_rows[n]                      # noqa: E731
            if auto and not one_sync:
                # Only the re-spawned envs are reset and re-rendered; only their first observations cross the bus.  The reset
                # mask is formed ON the device from the step's own outputs (no upload), the gathered rows land in a pinned
                # staging buffer with an asynchronous copy, and the stream is synchronised a second time
                new = env.reset(mask=st["terminated"] | st["truncated"])
                sel = new.index_select(0, torch.from_numpy(idx).to(env.torch_device, non_blocking=True))
                pin = self._sel_staging(len(idx), sel)
                pin.copy_(sel, non_blocking=True)
                torch.cuda.current_stream(env.torch_device).synchronize()
                obs_np[idx] = pin.numpy()
            if self.copy_obs and ep_r is not None:
                ep_r, ep_l = ep_r.copy(), ep_l.copy()
            terminal = LazyTerminal(idx, obs_of, ep_r, ep_l, t)
        if self.copy_obs:
            obs_np = obs_np.copy()
        if self.recording is not None:
            self._step_id += 1
            self.recording.after(self._step_id)
        return obs_np, rew, done, LazyInfos(self.num_envs, cols, terminal)

    def _sel_staging(self, n, like):
        """pinned host rows for the first observations of the envs that re-spawned at this step (grown on demand)"""
        cap = getattr(self, "_sel_pin", None)
        if cap is None or cap.shape[0] < n:
            rows = max(256, 1 << (int(n) - 1).bit_length())
            self._sel_pin = cap = torch.empty((rows,) + tuple(like.shape[1:]), dtype=like.dtype, pin_memory=True)
        return cap[:n]

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        if self.recording is not None:
            self.recording.close()
        self.env.close()

    def get_attr(self, attr_name, indices=None):
        return [getattr(self.env, attr_name)] * len(self._indices(indices))

    def set_attr(self, attr_name, value, indices=None):
        setattr(self.env, attr_name, value)

    def env_method(self, method_name, *method_args, indices=None, **method_kwargs):
        return [getattr(self.env, method_name)(*method_args, **method_kwargs)] * len(self._indices(indices))

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False] * len(self._indices(indices))

    def seed(self, seed=None):                                      # ref gym_env.py:149-150 (a no-op there too)
        return [None] * self.num_envs

    def get_images(self):
        return list(self.env.render())

    def render(self, mode=None):
        return self.env.render()

    def _indices(self, indices):
        if indices is None:
            return range(self.num_envs)
        return [indices] if isinstance(indices, int) else list(indices)


class WaypointSuiteEnv(_GymEnvBase):
    """B = 1 env with the reference's (B, A_exposed) = (1, 1) tensor interface (ref gym_env.py:303-437): `step` takes
    a (1,1,2) float32 tensor and returns obs (1,1,3,64,64) uint8 ndarray, reward float, terminated bool, truncated
    bool, info with (1,1) tensors — what `SingleAgentWrapper` then squeezes."""

    metadata = {"render_modes": ["video", "rgb_array"], "render_fps": 10}

    def __init__(self, cfg: EnvConfig, data, agents_per_env=8, road_meshes=None, traffic_lights=None, start_headings=None,
                 video_camera="map", background=None, near_field=None, planner=None, plan_refine=None, plan_react=None):
        """render_mode="video": every reset() and step() records a video_res x video_res frame at video_fov metres across (the
        reference's BirdviewRecordingWrapper, gym_env.py:295-297) from `video_camera` ("map": the centre of the map, heading pi/2;
        "ego"; or (x, y, psi)); get_birdviews() returns them, close() writes video_filename (video.save_video).
        background / near_field: the background-traffic files and the near-field traffic of every reset, as BatchedWaypointEnv
        takes them (the reference's background mode: gym_env.py:200-238).  planner / plan_refine: the config.Planner and the optional
        config.PlanRefine / config.PlanReact of expert_action()."""
        self.config = cfg
        if cfg.render_mode == "video":               # the batched env renders rgb_array; the frames are recorded here
            cfg = dataclasses.replace(cfg, render_mode="rgb_array")
        # info["offroad"] / info["collision"] carry the MAGNITUDES of compute_offroad() / compute_collision(), as the reference's
        # get_info reports them (ref gym_env.py:427-428; Monitor logs them, examples/rl_training.py:128)
        self._env = BatchedWaypointEnv(cfg, data, num_envs=1, agents_per_env=agents_per_env, obs_mode="birdview",
                                       frame_stack=1, auto_reset=False, info_magnitudes=True, road_meshes=road_meshes,
                                       traffic_lights=traffic_lights, start_headings=start_headings, background=background,
                                       near_field=near_field, planner=planner, plan_refine=plan_refine, plan_react=plan_react)
        self.torch_device = self._env.torch_device
        self.render_mode = self.config.render_mode
        self._video = None
        if self.render_mode == "video":
            res = int(self.config.video_res)
            self._video = VideoRecorder(self.config.video_filename, fps=self.metadata["render_fps"])
            self._video_res, self._video_fov = res, float(self.config.video_fov)
            if isinstance(video_camera, str):
                if video_camera not in ("map", "ego"):
                    raise ValueError("video_camera must be 'map', 'ego' or (x, y, psi)")
                self._video_cam = video_camera
            else:
                self._video_cam = torch.tensor([list(video_camera)], dtype=torch.float32, device=self.torch_device).reshape(1, 3)
            self._video_envs = torch.zeros(1, dtype=torch.int32, device=self.torch_device)
            self._video_views = None
            self._video_dev = torch.empty((1, 3, res, res), dtype=torch.uint8, device=self.torch_device)
            self._video_pin = torch.empty((1, 3, res, res), dtype=torch.uint8, pin_memory=True)
        self.max_environment_steps = cfg.max_environment_steps
        self.action_space = _box(ACTION_LOW, ACTION_HIGH)
        self.observation_space = _box(0, 255, (3, 64, 64), np.uint8)
        self.reward_range = (-float("inf"), float("inf"))
        self.collision_threshold = 0.0
        self.offroad_threshold = 0.0
        self._obs_pin = None

    @property
    def environment_steps(self):
        return int(self._env.state["steps"][0])

    @property
    def current_target_idx(self):
        return int(self._env.state["target_idx"][0])

    @property
    def reached_waypoint_num(self):
        return int(self._env.state["reached"][0])

    def reset(self, seed=None, options=None):                       # ref gym_env.py:319-349
        """options={"scenario": i}: start in scenario i of the suite instead of a drawn one (BatchedWaypointEnv.reset)"""
        obs = self._env.reset(options=options)
        if self._video is not None:
            self._video.start()                                      # (the reference builds a new recording wrapper per reset)
            self._video_views = None                                 # (the env's map may have changed)
            self._record_frame()
        obs = obs.cpu().numpy().reshape(1, 1, 3, 64, 64).astype(np.uint8)
        if self._video is not None:
            self._video.append(self._video_pin.clone())
        return obs, {}

    def _record_frame(self):
        """queue this state's video frame and its copy to the pinned staging buffer (the caller's synchronisation completes it)"""
        e = self._env
        v = self._video_views
        if v is None or (isinstance(self._video_cam, str) and self._video_cam == "ego"):
            v = ops.scene_views(e.dworld, e.state, self._video_envs, self._video_cam)
            self._video_views = v                                    # (a map or fixed camera holds until the next reset)
        ops.render_scene_views(e.tde_cfg, e.dworld, e.state, v, self._video_res, self._video_res, self._video_fov, self._video_dev,
                               flags=e._rflags)
        self._video_pin.copy_(self._video_dev, non_blocking=True)

    def get_birdviews(self):
        """the frames recorded since the last reset (render_mode="video"): uint8 CPU tensors [1, 3, video_res, video_res]"""
        return self._video.frames if self._video is not None else []

    def step(self, action):                                         # ref gym_env.py:369-389
        """one timestep.  Everything the reference's step returns crosses the bus in TWO asynchronous copies - the observation
        and the packed per-env outputs - behind ONE stream synchronisation (a `.item()` / `.cpu()` per returned value was a dozen
        synchronisations per step); the (1, 1) info tensors are therefore host tensors (the reference's live on `torch_device`;
        SingleAgentWrapper moves them to the CPU either way, gym_env.py:463-472)."""
        env = self._env
        st = env.state
        obs, _, _, _, _ = env.step(torch.as_tensor(action, dtype=torch.float32).reshape(1, 2))
        if self._obs_pin is None:
            self._obs_pin = torch.empty((1, 3, 64, 64), dtype=torch.uint8, pin_memory=True)
        self._obs_pin.copy_(obs, non_blocking=True)
        if self._video is not None:
            self._record_frame()                                     # (its copy is ahead of the synchronisation too)
        out = st.fetch_outputs()                                     # (the one synchronisation: the observation copy is ahead of it)
        if self._video is not None:
            self._video.append(self._video_pin.clone())
        mag = out["magnitudes"][0]
        t11 = lambda v: torch.tensor([[v]], dtype=torch.float32)    # noqa: E731
        trunc = bool(out["truncated"][0])
        info = {"offroad": t11(mag[0]), "collision": t11(mag[1]), "traffic_light_violation": t11(float(out["tl_violation"][0])),
                "is_success": trunc}
        if "info" in out:
            inf = out["info"][0]
            info.update(reached_waypoint_num=int(out["info_reached"][0]), psi_smoothness=float(inf[0]), speed_smoothness=float(inf[1]),
                        psi_reward=float(inf[2]), dist_reward=float(inf[3]))
        return (self._obs_pin.numpy().reshape(1, 1, 3, 64, 64).copy(), float(out["reward"][0]), bool(out["terminated"][0]), trunc, info)

    def expert_action(self):
        """the sampling planner's action on the current state (BatchedWaypointEnv.plan_actions): a float32 (2,) array, what
        SingleAgentWrapper.step takes"""
        return self._env.plan_actions().cpu().numpy().reshape(2).copy()

    def render(self):                                               # ref gym_env.py:152-157
        if self.render_mode == "rgb_array":
            return self._env.render()[0]
        raise NotImplementedError

    def close(self):
        """render_mode="video": writes video_filename from the frames of the current episode when there are more than one (ref
        gym_env.py:172-176; video.VideoRecorder for the one-frame case)"""
        if self._video is not None:
            self._video.close()

    def seed(self, seed=None):
        pass


class SingleAgentWrapper(_GymWrapperBase):
    """Removes batch and agent dimensions (ref gym_env.py:440-487): numpy (2,) action in, obs (3,64,64) uint8,
    reward float, terminated bool, truncated bool, info with 0-d CPU tensors out."""

    def __init__(self, env):
        super().__init__(env)

    def reset(self, **kwargs):
        obs, info = self.env.reset(**kwargs)
        return self.transform_out(obs), info

    def step(self, action):
        action = torch.Tensor(action).unsqueeze(0).unsqueeze(0).to(self.env.torch_device)   # ref :454
        obs, reward, terminated, truncated, info = self.env.step(action)
        return (self.transform_out(obs), self.transform_out(reward), self.transform_out(terminated), truncated,
                self.transform_out(info))

    def transform_out(self, x):                                     # ref gym_env.py:463-472
        if torch.is_tensor(x):
            return x.squeeze(0).squeeze(0).cpu()
        if isinstance(x, dict):
            return {k: self.transform_out(v) for k, v in x.items()}
        if isinstance(x, np.ndarray):
            return self.transform_out(torch.tensor(x)).cpu().numpy()
        return x

    def transform_in(self, x):                                      # ref gym_env.py:474-481 (unused upstream too: kept for the surface)
        if torch.is_tensor(x):
            return x.unsqueeze(0).unsqueeze(0)
        if isinstance(x, dict):
            return {k: self.transform_in(v) for k, v in x.items()}
        return x

    def expert_action(self):
        return self.env.expert_action()

    def render(self, *args, **kwargs):
        return self.env.render(*args, **kwargs)

    def close(self):
        self.env.close()


def make(cfg: EnvConfig, data, agents_per_env=8, road_meshes=None, traffic_lights=None, start_headings=None, video_camera="map",
         background=None, near_field=None, planner=None, plan_refine=None, plan_react=None):
    """what gym.make('torchdriveenv-v0', args={'cfg': cfg, 'data': data}) returns in the reference (ref __init__.py:10).
    `road_meshes`, `traffic_lights`, `start_headings`: what the reference takes from torchdrivesim's map config of the location
    (`find_map_config`: road mesh ref gym_env.py:184, stop lines + light controller :181-189, lanelet directions :359) - see
    world_from_waypoint_suite.  `video_camera`: the camera of render_mode="video" frames (WaypointSuiteEnv).  `background`: the
    background-traffic files (ref gym_env.py:200-231; default: the packaged directory when cfg.use_background_traffic);
    `near_field`: a config.NearField - traffic around the ego at every reset (ref gym_env.py:232-238; BatchedWaypointEnv)"""
    return SingleAgentWrapper(WaypointSuiteEnv(cfg=cfg, data=data, agents_per_env=agents_per_env, road_meshes=road_meshes,
                                               traffic_lights=traffic_lights, start_headings=start_headings,
                                               video_camera=video_camera, background=background, near_field=near_field,
                                               planner=planner, plan_refine=plan_refine, plan_react=plan_react))


if gym is not None:  # pragma: no cover
    try:
        gym.register('torchdriveenv-v0', entry_point=lambda args: make(args['cfg'], args['data'], road_meshes=args.get('road_meshes'),
                                                                       traffic_lights=args.get('traffic_lights'),
                                                                       start_headings=args.get('start_headings')))
    except Exception:
        pass
