"""CPU checks of routed near-field traffic (NearField(routes=True)): the route builder of world.build_near_field on four kinds of
world, the restated spawner with its per-slot route words (tests/near_field_routes_ref.py), the composed oracle - spawned agents that
still drive after 80 steps, against the unrouted control that stands - the host-side rules of the entry points, and the layout of the
new struct members.  (BatchedWaypointEnv needs a device: its ValueErrors and the state_dict round trip are in
tests/test_gpu_near_field_routes.py.)"""
import ctypes as C

import numpy as np
import pytest

from tests import near_field_ref as R
from tests import near_field_routes_ref as RR
from torchdriveenv_amd import _abi
from torchdriveenv_amd.config import NearField, Planner, check_near_field
from torchdriveenv_amd.state import EnvState
from torchdriveenv_amd.synth import synthetic_world
from torchdriveenv_amd.world import NF_ROAD_SLACK, mesh_distance

ROUTED = NearField(routes=True)


def _junction(nf, A=16, n_scn=4):
    return RR.junction_near_field(synthetic_world(n_scn=n_scn, A=A, seed=0, n_maps=2), nf)


def _town(nf, **kw):
    from torchdriveenv_amd.env import world_from_waypoint_suite

    data, meshes, field = R.town_suite(n_scn=2, n_streets=4)
    return world_from_waypoint_suite(data, agents_per_env=32, road_meshes=meshes, start_headings=field, near_field=nf, near_field_seed=3, **kw)


def _hook_world(tmp_path, own_routes):
    """a validation case whose candidates come from a hook: points along the first waypoint segment's direction, with or without routes"""
    from tests.golden_util import write_validation_suite_yaml
    from torchdriveenv_amd.config import WaypointSuite
    from torchdriveenv_amd.env import world_from_waypoint_suite
    from torchdriveenv_amd.loaders import load_waypoint_suite_data

    val = load_waypoint_suite_data(write_validation_suite_yaml(str(tmp_path / "val.yml")))
    one = WaypointSuite(locations=val.locations[:1], waypoint_suite=val.waypoint_suite[:1], scenarios=val.scenarios[:1],
                        car_sequence_suite=val.car_sequence_suite[:1])
    w = np.asarray(one.waypoint_suite[0], np.float64)
    d = (w[1] - w[0]) / np.hypot(*(w[1] - w[0]))
    psi = float(np.arctan2(d[1], d[0]))
    P = np.asarray([(*(w[0] + d * (12.0 + 7.0 * k)), psi) for k in range(8)])

    def hook(loc, si):
        if not own_routes:
            return P
        return P, [np.asarray([p[:2] + d * 4.0 * (q + 1) for q in range(6)]) if k % 2 == 0 else None for k, p in enumerate(P)]

    # (the field: the first segment's direction everywhere - what traces the candidates the hook gives no route for)
    return world_from_waypoint_suite(one, agents_per_env=16, near_field=NearField(routes=True, candidates=hook, route_pitch=4.0),
                                     near_field_seed=7, start_headings=lambda loc, x, y: psi)


@pytest.fixture(scope="module")
def routed_worlds(tmp_path_factory):
    d = tmp_path_factory.mktemp("nfr")
    return {"junction": _junction(ROUTED), "town": _town(NearField(routes=True, route_pitch=5.0, route_points=24)),
            "polylines": R.validation_world(0, 16, d, nf=ROUTED), "hook": _hook_world(d, False), "hook+routes": _hook_world(d, True)}


def _mesh_of(world, s):
    md = world.arrays["maps"][int(world.arrays["scn"]["map"][s])]
    return world.arrays["tri"].reshape(-1, 3, 2).astype(np.float64)[int(md["tri_base"]):int(md["tri_base"]) + int(md["n_tri"])]


@pytest.mark.parametrize("name", ["junction", "town", "polylines", "hook", "hook+routes"])
def test_route_builder(routed_worlds, name):
    world, tab = routed_worlds[name]
    nf_points = 24 if name == "town" else 32
    rt = world.arrays["route_xy"].reshape(-1, world.ints["RW"], 2)
    assert world.ints["RW"] >= nf_points and world.ints["n_routes"] == len(rt) < (1 << 20) - 1 and world.ints["RW"] < 4096
    assert tab.routes
    n_routed = 0
    for s in range(tab.S):
        cand = tab.cand[s, :tab.n_cand[s]]
        assert (tab.cand[s, tab.n_cand[s]:]["route"] == 0).all()
        mesh = _mesh_of(world, s)
        for cd in cand:
            if cd["route"] == 0:
                assert cd["route_wp"] == 0 and cd["route_n"] == 0
                continue
            n_routed += 1
            rid, n, w0 = int(cd["route"]) - 1, int(cd["route_n"]), int(cd["route_wp"])
            assert 0 <= rid < world.ints["n_routes"] and 2 <= n - w0 and n <= nf_points and n < 4096 and rid + 1 < (1 << 20) - 1
            pts = rt[rid, :n].astype(np.float64)
            assert (rt[rid, n:] == 0).all()                                    # padded as the scenario routes are
            assert (mesh_distance(pts, mesh, world.threshold) <= world.threshold - NF_ROAD_SLACK).all()
            x, y, psi = float(cd["x"]), float(cd["y"]), float(cd["psi"])
            assert (pts[w0, 0] - x) * np.cos(psi) + (pts[w0, 1] - y) * np.sin(psi) > 0.0
            if name == "town":                                                   # a field trace: route_pitch between waypoints
                step = np.hypot(*np.diff(np.concatenate([[[x, y]], pts]), axis=0).T)
                assert np.allclose(step, 5.0, atol=1e-3), step
    assert n_routed > 0
    if name == "hook+routes":                                                    # even candidates drive the hook's own 4 m polyline
        cd = tab.cand[0, :tab.n_cand[0]]
        own = [c for c in cd if c["route"] and c["route_n"] <= 6]
        assert own and all(np.allclose(np.hypot(*np.diff(rt[int(c["route"]) - 1, :c["route_n"]], axis=0).T), 4.0, atol=1e-3) for c in own)


def test_a_candidate_at_a_dead_end_has_no_route():
    """the last candidates of a polyline have fewer than two waypoints ahead of them before the polyline (and the road) ends"""
    world, tab = _junction(NearField(routes=True, route_pitch=20.0))
    cand = tab.cand[0, :tab.n_cand[0]]
    assert (cand["route"] == 0).any() and (cand["route"] != 0).any()
    none = cand[cand["route"] == 0]
    assert (none["route_wp"] == 0).all() and (none["route_n"] == 0).all()


def test_routes_false_is_byte_identical_to_the_parent_builder(tmp_path):
    """routes=False: the candidate tables and the world are what the builder gave before the field existed - the route words are the
    pad words (zero), no row is added to the route table"""
    for build in (lambda nf: _junction(nf), lambda nf: _town(nf), lambda nf: R.validation_world(0, 16, tmp_path, nf=nf)):
        w0, t0 = build(NearField())
        w1, t1 = build(NearField(routes=False, route_pitch=3.0, route_points=8))
        w2, t2 = build(NearField(routes=True))
        for k in ("cand", "nbr", "nbr_n", "fixed", "n_cand"):
            assert getattr(t0, k).tobytes() == getattr(t1, k).tobytes(), k
        raw = t0.cand.reshape(-1).view(np.uint32).reshape(-1, 12)
        assert not raw[:, 9:].any() and not t0.routes and not t1.routes
        for k in w0.arrays:
            assert w0.arrays[k].tobytes() == w1.arrays[k].tobytes(), k
        assert w0.ints == w1.ints
        # ... and the routed table is that table with the three words filled: nothing else of a candidate depends on `routes`
        raw2 = t2.cand.reshape(-1).view(np.uint32).reshape(-1, 12)
        assert np.array_equal(raw[:, :9], raw2[:, :9]) and raw2[:, 9].any()
        assert w2.ints["n_routes"] > w0.ints["n_routes"]
        n0, RW0 = w0.ints["n_routes"], w0.ints["RW"]
        assert np.array_equal(w2.arrays["route_xy"].reshape(-1, w2.ints["RW"], 2)[:n0, :RW0], w0.arrays["route_xy"].reshape(-1, RW0, 2)[:n0])


def test_parameter_validation():
    for bad in (dict(route_pitch=0.0), dict(route_pitch=float("inf")), dict(route_points=1), dict(route_points=4096), dict(route_points=2.5)):
        with pytest.raises(ValueError, match="route_"):
            check_near_field(NearField(routes=True, **bad))
    assert check_near_field(dict(routes=True, route_pitch=4.0, route_points=16)).routes


def test_struct_layout_matches_the_header(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tde_abi.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(tde_nf_cand), offsetof(tde_nf_cand, route), offsetof(tde_nf_cand, route_wp), offsetof(tde_nf_cand, route_n), '
                   'sizeof(tde_state), offsetof(tde_state, slot_route), offsetof(tde_state, B), offsetof(tde_state, magnitudes)); return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["cc", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    d, S = _abi.NF_CAND_DTYPE, _abi.TdeState
    assert got == [d.itemsize, d.fields["route"][1], d.fields["route_wp"][1], d.fields["route_n"][1], C.sizeof(S), S.slot_route.offset,
                   S.B.offset, S.magnitudes.offset]
    assert got[0] == 48 and got[1] == 36


def _reset(world, cfg, B, ep=0):
    from oracle import oracle

    hs = EnvState(B, world.A, with_slot_route=True)
    hs["episode"][...] = ep
    oracle.env_reset(cfg, world, hs)
    return hs


def test_restated_spawner_writes_every_slot_of_a_masked_env(routed_worlds):
    from oracle import oracle

    world, tab = routed_worlds["junction"]
    cfg = _abi.default_config(seed=4)
    B, A = 8, world.A
    hs = _reset(world, cfg, B)
    RR.words(hs)[...] = 0xDEAD0001                                               # stale words of an earlier episode, every slot
    mask = np.array([1, 0, 1, 1, 0, 1, 1, 1], np.uint8)
    before = hs.host()
    RR.spawn(cfg, world, tab, hs, mask)
    sr, free = RR.words(hs).reshape(B, A), world.arrays["spawn"]["present"].reshape(-1, A)[hs["scn"]] == 0
    new = (hs["present"].reshape(B, A) != 0) & free
    assert (sr[mask == 0] == 0xDEAD0001).all() and (sr[mask != 0, 0] == 0xDEAD0001).all()      # unmasked envs and the ego's entry untouched
    assert new[mask != 0].any() and not new[mask == 0].any()
    m = mask != 0
    assert (sr[m][:, 1:][~new[m][:, 1:]] == 0).all()                             # every other slot of a masked env: 0
    ids, lens = (sr & 0xFFFFF).astype(np.int64) - 1, sr >> 20
    routed = m[:, None] & new & (sr != 0)
    assert routed.any() and (ids[routed] >= 0).all() and (ids[routed] < world.ints["n_routes"]).all() and (lens[routed] >= 2).all()
    for k in ("x", "present", "route_wp"):
        assert np.array_equal(before[k].reshape(B, A)[~m], hs[k].reshape(B, A)[~m])
    # episode k + 1: the reset leaves the words (it does not know them), the spawner that follows it clears what it does not rewrite
    stale = RR.words(hs).copy()
    oracle.env_reset(cfg, world, hs)
    assert np.array_equal(RR.words(hs), stale)
    RR.spawn(cfg, world, tab, hs)
    sr2 = RR.words(hs).reshape(B, A)
    new2 = (hs["present"].reshape(B, A) != 0) & (world.arrays["spawn"]["present"].reshape(-1, A)[hs["scn"]] == 0)
    assert (sr2[:, 1:][~new2[:, 1:]] == 0).all() and not np.array_equal(sr2, stale.reshape(B, A))


@pytest.mark.parametrize("name", ["junction", "town"])
def test_routed_agents_still_drive_after_80_steps_and_unrouted_ones_stand(routed_worlds, name):
    world, tab = routed_worlds[name]
    cfg = _abi.default_config(seed=1, flags=(_abi.F_ALL | (_abi.F_TRAFFIC_LIGHTS if world.has_lights else 0)) & ~_abi.F_AUTORESET)
    B = 4
    spawned, v, dist = RR.moving_share(cfg, world, tab, B, steps=80, routes=True)
    assert spawned.sum(1).min() > 0
    assert ((v > 1.0) & spawned).any(1).all(), ((v > 1.0) & spawned).sum(1)
    spawned0, v0, dist0 = RR.moving_share(cfg, world, tab, B, steps=80, routes=False)
    assert np.array_equal(spawned, spawned0)
    assert not ((v0 > 1.0) & spawned0).any(), v0[spawned0].max()
    assert dist[spawned].mean() > 2.0 * dist0[spawned0].mean()


def test_host_rules_need_no_gpu():
    """every entry point that reads routes from the spawn records refuses a state with slot_route, under its own name and before any
    launch; the others take it (an empty batch returns before a launch)"""
    from torchdriveenv_amd import _lib, ops

    L = _lib.load()
    w = synthetic_world(n_scn=2, A=8, seed=0, n_maps=1)
    cfg = _abi.default_config(seed=1, flags=_abi.F_ALL & ~_abi.F_AUTORESET)
    f32 = np.float32
    seq, cost, fail = np.zeros((4, 3, 2, 2), f32), np.zeros((4, 3), f32), np.zeros((4, 3), np.int32)
    out, act, rew = np.zeros((4, 96, 8, 4), f32), np.zeros((4, 2), f32), np.zeros((2, 4), f32)
    pl, ps = ops.planner_struct(Planner()), _abi.TdePlanSet(seq.ctypes.data, 3, 2, 16, 0)
    ro = _abi.TdeRollout(act.ctypes.data, rew.ctypes.data, None, 1, 0)
    ev_arr = [np.zeros(4, np.int32) for _ in range(2)]
    streams = (C.c_void_p * 1)(None)
    img, rays, vout, mask = np.zeros((4, 3, 64, 64), np.uint8), np.array([[1.0, 0.0]], f32), np.zeros((4, 32), f32), np.zeros(4, np.uint8)
    rd = _abi.TdeRender(img.ctypes.data, 64, 64, 35.0, 1, None, 0, 0, None, None)
    vo = _abi.TdeVectorObs(rays.ctypes.data, 1, 1, 50.0, 40.0, 0.5, 0)
    recs = np.zeros((2, 4), _abi.EPISODE_RECORD_DTYPE)
    ev = _abi.TdeEval(ev_arr[0].ctypes.data, ev_arr[1].ctypes.data, mask.ctypes.data, recs[0].ctypes.data, recs.ctypes.data, 1, 0)

    def call(name, routed):
        st = EnvState(4, 8, with_slot_route=routed)
        st.struct.B = 0
        a = (C.byref(cfg), C.byref(w.host_struct()), C.byref(st.struct))
        judged = (C.byref(pl), C.byref(ps), None, cost.ctypes.data, fail.ctypes.data, None, None)
        return {
            "tde_env_rollout": lambda: L.tde_env_rollout(*a, C.byref(ro), None),
            "tde_env_step_render": lambda: L.tde_env_step_render(*a, None, streams, 1),
            "tde_forecast_agents": lambda: L.tde_forecast_agents(*a, 8, None, out.ctypes.data, None),
            "tde_forecast_scene": lambda: L.tde_forecast_scene(*a, 8, None, None, out.ctypes.data, None),
            "tde_score_plans_scene": lambda: L.tde_score_plans_scene(*a, *judged, None),
            "tde_env_step": lambda: L.tde_env_step(*a, None),
            "tde_plan_action": lambda: L.tde_plan_action(*a, C.byref(pl), None, act.ctypes.data, None, None),
            "tde_score_plans": lambda: L.tde_score_plans(*a, *judged, None),
            "tde_score_plans_forecast": lambda: L.tde_score_plans_forecast(*a, *judged, out.ctypes.data, 96, None),
            "tde_env_post_step": lambda: L.tde_env_post_step(*a, None, None),
            "tde_env_reset": lambda: L.tde_env_reset(*a, None, None),
            "tde_env_reset_to": lambda: L.tde_env_reset_to(*a, None, ev_arr[0].ctypes.data, None),
            "tde_vector_obs": lambda: L.tde_vector_obs(*a, C.byref(vo), None, vout.ctypes.data, None),
            "tde_render_ego": lambda: L.tde_render_ego(*a, C.byref(rd), None),
            "tde_render_scene": lambda: L.tde_render_scene(*a, None, 0, 64, 64, 35.0, 0, None, None),
            "tde_env_reset_render": lambda: L.tde_env_reset_render(*a, mask.ctypes.data, C.byref(rd), None),
            "tde_eval_advance": lambda: L.tde_eval_advance(*a, C.byref(ev), None),
        }[name]()

    refuse = ("tde_env_rollout", "tde_env_step_render", "tde_forecast_agents", "tde_forecast_scene", "tde_score_plans_scene")
    accept = ("tde_env_step", "tde_plan_action", "tde_score_plans", "tde_score_plans_forecast", "tde_env_post_step", "tde_env_reset",
              "tde_env_reset_to", "tde_vector_obs", "tde_render_ego", "tde_render_scene", "tde_env_reset_render", "tde_eval_advance")
    for name in refuse + accept:
        assert call(name, False) == 0, (name, L.tde_last_error())
    for name in refuse:
        rc, err = call(name, True), L.tde_last_error()
        assert rc != 0 and name.encode() + b":" in err and b"state.slot_route is set" in err, (name, rc, err)
    for name in accept:
        assert call(name, True) == 0, (name, L.tde_last_error())
    # fewer than four slots per env: no routed form
    st = EnvState(4, 2, with_slot_route=True)
    w2 = synthetic_world(n_scn=2, A=2, seed=0, n_maps=1)
    assert L.tde_env_step(C.byref(cfg), C.byref(w2.host_struct()), C.byref(st.struct), None) != 0
    assert b"slot_route needs at least 4" in L.tde_last_error()


def test_state_carries_slot_route_only_on_request():
    assert EnvState(2, 8)["slot_route"] is None and EnvState(2, 8).struct.slot_route is None
    st = EnvState(2, 8, with_slot_route=True)
    assert st["slot_route"].shape == (16,) and st["slot_route"].dtype == np.int32 and st.struct.slot_route == st["slot_route"].ctypes.data
    assert "slot_route" in st.host()
    # ... and keeps it through host() and load(): a checkpoint of a host state carries the route words
    st["slot_route"].view(np.uint32)[...] = np.arange(16, dtype=np.uint32) | np.uint32(5 << 20)
    st["route_wp"][...] = 3
    snap = st.host()
    other = EnvState(2, 8, with_slot_route=True)
    other.load(snap)
    assert np.array_equal(other["slot_route"], st["slot_route"]) and np.array_equal(other["route_wp"], st["route_wp"])
    EnvState(2, 8).load(snap)                                                    # a state without the array ignores the words


def test_a_hook_that_returns_a_tuple_of_rows_is_read_as_points_without_routes(tmp_path):
    """routes=False: whatever the `candidates` hook returns goes through np.asarray as before - a tuple of (x, y, psi) rows, two of
    them included, is the points and never (points, routes)"""
    from torchdriveenv_amd.env import near_field_positions

    world = synthetic_world(n_scn=1, A=8, seed=0, n_maps=1)
    rows = ((1.0, 2.0, 0.5), (3.0, 4.0, 0.25))
    for n in (2, 3):
        hook = lambda loc, si, n=n: (rows * 2)[:n]                           # noqa: E731
        pos, src = near_field_positions(world, NearField(candidates=hook), [[]], [None])
        assert src == ["candidates"] and np.array_equal(pos[0], np.asarray((rows * 2)[:n]))
    # under routes=True the pair form needs a 2-D first member: two bare rows are still points
    pos, src, tr = near_field_positions(world, NearField(candidates=lambda loc, si: rows, routes=True), [[]], [None], with_routes=True)
    assert np.array_equal(pos[0], np.asarray(rows))
