"""CPU checks of the near-field spawner's host side: the candidate tables world_from_waypoint_suite(near_field=) builds (on the road,
exact neighbour lists and fixed-conflict bits), the tde_near_field layout, parameter validation, and the numpy restatement of
tde_near_field_spawn (tests/near_field_ref.py) that the GPU tests hold the kernel against."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import near_field_ref as R
from torchdriveenv_amd import _abi
from torchdriveenv_amd.config import EnvConfig, NearField, WaypointSuite, check_near_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    d = tmp_path_factory.mktemp("nf")
    out = [R.validation_world(case, 16, d) for case in range(5)]
    data, meshes, field = R.town_suite(n_scn=2, n_streets=4)
    from torchdriveenv_amd.env import world_from_waypoint_suite

    out.append(world_from_waypoint_suite(data, agents_per_env=128, road_meshes=meshes, start_headings=field, near_field=NearField(),
                                         near_field_seed=3))
    return out


def _boxes(rec, inflate=0.0):
    psi = rec["psi"].astype(np.float64)
    return (rec["x"].astype(np.float64), rec["y"].astype(np.float64), np.cos(psi), np.sin(psi),
            0.5 * rec["len"].astype(np.float64) + inflate, 0.5 * rec["wid"].astype(np.float64) + inflate)


def _corners(b):
    x, y, c, s, hl, hw = b
    out = []
    for a, w in ((1, 1), (1, -1), (-1, -1), (-1, 1)):
        out.append(np.stack([x + a * hl * c - w * hw * s, y + a * hl * s + w * hw * c], -1))
    return np.stack(out, -2)                                   # [..., 4, 2]


def _brute_overlap(P, Q):
    """strict overlap of two convex quads (corners [4, 2]) by projecting both on the four edge normals - a second formulation of the
    separating-axis test"""
    for K in (P, Q):
        for k in range(4):
            e = K[(k + 1) % 4] - K[k]
            nrm = np.array([-e[1], e[0]])
            p, q = P @ nrm, Q @ nrm
            if p.max() <= q.min() or q.max() <= p.min():
                return False
    return True


def test_candidates_are_on_the_road(tables):
    from oracle import oracle

    for world, tab in tables:
        for s in range(tab.S):
            n = int(tab.n_cand[s])
            assert n > 0
            rec = tab.cand[s, :n]
            one = np.ones(n, np.uint8)
            thr = world.threshold
            off = oracle.compute_offroad(1, n, rec["x"].copy(), rec["y"].copy(), rec["psi"].copy(), rec["len"].copy(), rec["wid"].copy(),
                                         one, world, np.array([world.map_of_scn()[s]], np.int32), thr)
            assert not off.any(), (s, np.flatnonzero(off))
            p0, p1 = world.arrays["wp_xy"][s, 0], world.arrays["wp_xy"][s, 1]
            assert (np.hypot(rec["x"] - p0[0], rec["y"] - p0[1]) <= tab.radius + np.hypot(*(p1 - p0)) + 1e-3).all()
            assert ((rec["len"] >= 4.8) & (rec["len"] <= 5.5) & (rec["wid"] >= 1.8) & (rec["wid"] <= 2.2)).all()
            assert ((rec["lr"] >= 0.82) & (rec["lr"] <= 0.97) & (rec["vdes"] >= 5.0) & (rec["vdes"] <= 12.0)).all()


def test_neighbour_lists_are_symmetric_and_exact(tables):
    for world, tab in tables:
        hm = 0.5 * 0.5
        for s in range(tab.S):
            n = int(tab.n_cand[s])
            K = _corners(_boxes(tab.cand[s, :n], hm))
            want = [set() for _ in range(n)]
            for i in range(n):
                for j in range(i + 1, n):
                    if _brute_overlap(K[i], K[j]):
                        want[i].add(j)
                        want[j].add(i)
            got = [set(tab.neighbours(s, i).tolist()) for i in range(n)]
            assert got == want, s
            for i in range(n):
                assert all(i in got[j] for j in got[i])
                assert len(got[i]) <= tab.K <= _abi.NF_MAX_NBR


def test_fixed_conflict_bits(tables):
    hm = 0.25
    seen = 0
    for world, tab in tables:
        for s in range(tab.S):
            n = int(tab.n_cand[s])
            K = _corners(_boxes(tab.cand[s, :n], hm))
            ag = world.arrays["spawn"][s, 1:]
            ag = ag[ag["present"] != 0]
            Q = _corners(_boxes(ag, hm)) if len(ag) else np.zeros((0, 4, 2))
            want = np.array([any(_brute_overlap(K[i], q) for q in Q) for i in range(n)], np.uint8)
            assert np.array_equal(tab.fixed[s, :n], want), s
            seen += int(want.sum())
    assert seen > 0                                          # some candidates do sit on a scenario agent


def test_near_field_struct_matches_header(tmp_path):
    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "tde_abi.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(tde_near_field), sizeof(tde_nf_cand),
         offsetof(tde_near_field, cand), offsetof(tde_near_field, nbr), offsetof(tde_near_field, nbr_n), offsetof(tde_near_field, fixed),
         offsetof(tde_near_field, n_cand), offsetof(tde_near_field, S), offsetof(tde_near_field, A), offsetof(tde_near_field, NC),
         offsetof(tde_near_field, K), offsetof(tde_near_field, radius), offsetof(tde_near_field, clear_ego),
         offsetof(tde_near_field, count), offsetof(tde_near_field, density), offsetof(tde_nf_cand, vdes), (size_t)TDE_NF_TAG);
  return 0; }'''
    c = tmp_path / "s.c"
    c.write_text(prog)
    exe = str(tmp_path / "s")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    got = [int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    T = _abi.TdeNearField
    want = [C.sizeof(T), _abi.NF_CAND_DTYPE.itemsize] + [getattr(T, f).offset for f in (
        "cand", "nbr", "nbr_n", "fixed", "n_cand", "S", "A", "NC", "K", "radius", "clear_ego", "count", "density")] + [
        _abi.NF_CAND_DTYPE.fields["vdes"][1], _abi.NF_TAG]
    assert got == want


def test_parameter_validation(tmp_path):
    from torchdriveenv_amd.env import world_from_waypoint_suite

    with pytest.raises(ValueError, match="ego_only"):
        check_near_field(NearField(), EnvConfig(ego_only=True))
    data = WaypointSuite(locations=["x"], waypoint_suite=[[[0.0, 0.0], [30.0, 0.0], [60.0, 0.0]]], car_sequence_suite=[None],
                         scenarios=[None])
    with pytest.raises(ValueError, match="ego_only"):
        world_from_waypoint_suite(data, agents_per_env=16, ego_only=True, near_field=NearField())
    with pytest.raises(ValueError, match="clear_ego"):
        world_from_waypoint_suite(data, agents_per_env=16, near_field=NearField(clear_ego=5.0))
    with pytest.raises(ValueError, match="candidates"):
        check_near_field(NearField(candidates=[(1.0, 2.0, 0.0)]))
    with pytest.raises(ValueError, match="candidates"):
        world_from_waypoint_suite(data, agents_per_env=16, near_field=NearField(candidates=lambda loc, i: np.zeros((4, 2))))
    with pytest.raises(ValueError):
        check_near_field(NearField(radius=-1.0))
    with pytest.raises(ValueError):
        check_near_field(NearField(speed=(8.0, 2.0)))
    # the hook is the first source: its poses (those on the road, within reach) are the candidates
    hook = lambda loc, i: np.array([[10.0, -1.75, 0.0], [40.0, 1.75, np.pi], [500.0, 0.0, 0.0]])    # noqa: E731
    world, tab = world_from_waypoint_suite(data, agents_per_env=16, near_field=NearField(candidates=hook))
    assert tab.sources == ["candidates"] and int(tab.n_cand[0]) == 2
    assert np.allclose(tab.cand[0, :2]["x"], [10.0, 40.0])
    # without near_field nothing changes: a World, not a pair
    from torchdriveenv_amd.world import World

    assert isinstance(world_from_waypoint_suite(data, agents_per_env=16), World)


def test_philox_restatement_equals_the_oracle():
    from oracle import oracle

    rng = np.random.default_rng(0)
    for _ in range(20):
        seed = int(rng.integers(0, 2**63))
        c = [int(v) for v in rng.integers(0, 2**32, 4)]
        want = list(oracle.philox(seed, *c))
        got = R.philox_np(seed, *[np.array([v]) for v in c])[:, 0].tolist()
        assert got == want


def _reset_state(world, cfg, B, A, ep=0):
    from oracle import oracle
    from torchdriveenv_amd.state import EnvState

    hs = EnvState(B, A)
    hs["episode"][...] = ep
    oracle.env_reset(cfg, world, hs)
    return hs


def test_restatement_is_deterministic_and_shard_invariant(tables):
    world, tab = tables[5]                                   # the town: many candidates, many conflicts
    B, A = 32, world.A
    cfg = _abi.default_config(seed=11)
    a = _reset_state(world, cfg, B, A)
    b = _reset_state(world, cfg, B, A)
    R.spawn(cfg, world, tab, a)
    R.spawn(cfg, world, tab, b)
    for k in ("x", "y", "psi", "v", "present", "vdes"):
        assert np.array_equal(a[k], b[k])
    added = a["present"].reshape(B, A).sum(1) - world.arrays["spawn"]["present"][a["scn"]].sum(1)
    assert added.min() > 0
    # two shards [0, 12) and [12, 32) keyed by env_base replay the unsharded batch
    for lo, hi in ((0, 12), (12, 32)):
        cs = _abi.default_config(seed=11, env_base=lo)
        h = _reset_state(world, cs, hi - lo, A)
        R.spawn(cs, world, tab, h)
        for k in ("x", "y", "psi", "v", "len", "wid", "lr", "vdes", "present", "route_wp"):
            assert np.array_equal(h[k], a[k][lo * A:hi * A]), k
    # another episode draws other traffic
    c = _reset_state(world, cfg, B, A, ep=1)
    R.spawn(cfg, world, tab, c)
    assert not np.array_equal(c["x"], a["x"])


def test_restatement_spawns_safely_and_tops_up_to_the_count(tables):
    from oracle import oracle

    world, tab = tables[5]
    B, A = 32, world.A
    cfg = _abi.default_config(seed=4)
    hs = _reset_state(world, cfg, B, A)
    want_T = [R.target(tab, world, hs, e)[0] for e in range(B)]
    R.spawn(cfg, world, tab, hs)
    args = (hs["x"], hs["y"], hs["psi"], hs["len"], hs["wid"], hs["present"])
    assert not oracle.compute_collision(B, A, *args).any()
    assert not oracle.compute_offroad(B, A, *args, world, world.map_of_scn()[hs["scn"]], world.threshold).any()
    added = hs["present"].reshape(B, A).sum(1) - world.arrays["spawn"]["present"][hs["scn"]].sum(1)
    assert (added <= np.asarray(want_T)).all() and added.mean() >= 60
