"""CPU checks of the vector observation (obs_mode="vector", tde_vector_obs): config.VectorObs and its validation, the row layout,
struct tde_vector_obs against the header, the library's own argument checks (they return before any launch), and known answers of
the numpy restatement (tests/vector_obs_ref.py) that the GPU tests hold the kernel against."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import vector_obs_ref as R
from torchdriveenv_amd import _abi
from torchdriveenv_amd.config import EnvConfig, VectorObs, check_vector_obs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_defaults_dim_and_slices():
    vo = check_vector_obs(VectorObs())
    assert (vo.k_neighbours, vo.n_rays, vo.ray_range, vo.ray_step, vo.neighbour_radius) == (8, 32, 50.0, 0.5, 50.0)
    assert vo.dim == 10 + 9 * 8 + 3 * 32 == 178
    sl = vo.slices()
    row = np.arange(vo.dim)
    covered = np.concatenate([row[sl[k]] for k in ("ego", "neighbours", "rays")])
    assert np.array_equal(covered, row)
    assert np.array_equal(np.concatenate([row[sl[k]] for k in ("v", "length", "width", "target", "next_target", "targets_left",
                                                               "progress", "has_lights")]), row[:10])
    assert row[sl["neighbours"]].reshape(8, 9)[3, 0] == 10 + 27
    rays = row[sl["rays"]].reshape(32, 3)
    assert np.array_equal(rays[:, 0], row[sl["road"]]) and np.array_equal(rays[:, 1], row[sl["car"]])
    assert np.array_equal(rays[:, 2], row[sl["red_line"]])
    d = vo.ray_directions()
    assert d.shape == (32, 2) and d.dtype == np.float32 and d.flags.c_contiguous
    assert np.allclose(np.hypot(d[:, 0], d[:, 1]), 1.0, atol=1e-6)
    assert np.allclose(d[0], [1, 0]) and np.allclose(d[8], [0, 1], atol=1e-7)      # counter-clockwise from straight ahead
    assert check_vector_obs(dict(k_neighbours=0, n_rays=0)).dim == 10


@pytest.mark.parametrize("bad", [dict(k_neighbours=17), dict(k_neighbours=-1), dict(n_rays=65), dict(n_rays=-1),
                                 dict(ray_range=0.0), dict(ray_step=-0.5), dict(neighbour_radius=float("nan")),
                                 dict(ray_range=float("inf")), dict(ray_range=50.0, ray_step=0.3), dict(ray_range=1000.0, ray_step=0.5),
                                 dict(ray_range=0.25, ray_step=0.5)])
def test_validation_rejects(bad):
    with pytest.raises(ValueError):
        check_vector_obs(VectorObs(**bad))


def test_env_obs_mode_validation():
    from torchdriveenv_amd.env import BatchedWaypointEnv
    from torchdriveenv_amd.synth import synthetic_world

    w = synthetic_world(n_scn=2, A=8, seed=0, n_maps=1)
    with pytest.raises(ValueError, match="frame_stack"):
        BatchedWaypointEnv(EnvConfig(), w, num_envs=4, agents_per_env=8, obs_mode="vector", frame_stack=2)
    with pytest.raises(ValueError, match="obs_mode"):
        BatchedWaypointEnv(EnvConfig(), w, num_envs=4, agents_per_env=8, obs_mode="lidar")
    with pytest.raises(ValueError):
        BatchedWaypointEnv(EnvConfig(), w, num_envs=4, agents_per_env=8, obs_mode="vector", vector_obs=VectorObs(n_rays=99))


def test_struct_matches_header(tmp_path):
    c = tmp_path / "vo.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "tde_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu '
                 '%d %d %d %d %d %d %d\\n", sizeof(struct tde_vector_obs), offsetof(struct tde_vector_obs, ray_dir), '
                 'offsetof(struct tde_vector_obs, k_nbr), offsetof(struct tde_vector_obs, n_rays), offsetof(struct tde_vector_obs, '
                 'nbr_radius), offsetof(struct tde_vector_obs, ray_range), offsetof(struct tde_vector_obs, ray_step), '
                 '(size_t)TDE_ABI_VERSION, TDE_VO_MAX_NBR, TDE_VO_MAX_RAYS, TDE_VO_MAX_SAMPLES, TDE_VO_EGO, TDE_VO_NBR, TDE_VO_RAY, '
                 'TDE_CELL_FULL); return 0;}\n')
    exe = str(tmp_path / "vo")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    got = [int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    S = _abi.TdeVectorObs
    assert got[:8] == [C.sizeof(S), S.ray_dir.offset, S.k_nbr.offset, S.n_rays.offset, S.nbr_radius.offset, S.ray_range.offset,
                       S.ray_step.offset, _abi.TDE_ABI_VERSION]
    assert got[8:14] == [_abi.VO_MAX_NBR, _abi.VO_MAX_RAYS, _abi.VO_MAX_SAMPLES, _abi.VO_EGO, _abi.VO_NBR, _abi.VO_RAY]


def test_library_rejects_bad_arguments():
    """the entry point's own checks (before any launch: no GPU needed)"""
    from torchdriveenv_amd import _lib
    from torchdriveenv_amd.state import EnvState
    from torchdriveenv_amd.synth import synthetic_world

    L = _lib.load()
    w = synthetic_world(n_scn=2, A=8, seed=0, n_maps=1)
    st = EnvState(4, 8)
    cfg = _abi.default_config(seed=1)
    out = np.zeros(4 * 64, np.float32)
    rd = np.zeros((4, 2), np.float32)

    def call(vo, cfg=cfg, out_p=out.ctypes.data):
        return L.tde_vector_obs(C.byref(cfg), C.byref(w.host_struct()), C.byref(st.struct), C.byref(vo) if vo is not None else None,
                                None, out_p, None)

    good = dict(ray_dir=rd.ctypes.data, k_nbr=2, n_rays=4, nbr_radius=30.0, ray_range=20.0, ray_step=0.5)
    for over, msg in ((dict(k_nbr=17), b"k_nbr"), (dict(n_rays=65), b"n_rays"), (dict(ray_dir=None), b"ray_dir"),
                      (dict(nbr_radius=0.0), b"finite"), (dict(ray_range=float("inf")), b"finite"), (dict(ray_step=float("nan")), b"finite"),
                      (dict(ray_step=0.3), b"integer"), (dict(ray_range=2000.0, ray_step=1.0), b"integer")):
        vo = _abi.TdeVectorObs(**dict(good, **over))
        assert call(vo) != 0 and msg in L.tde_last_error(), over
    assert call(None) != 0 and b"NULL" in L.tde_last_error()
    assert call(_abi.TdeVectorObs(**good), out_p=None) != 0 and b"NULL" in L.tde_last_error()
    c0 = _abi.default_config(seed=1)
    c0.max_steps = 0
    assert call(_abi.TdeVectorObs(**good), cfg=c0) != 0 and b"max_steps" in L.tde_last_error()


# ---- known answers of the restatement -------------------------------------------------------------------------------------------------


def _corridor_world(A=8, lights=True):
    from torchdriveenv_amd.world import assemble_world, corridor_mesh

    mesh = corridor_mesh([[(0.0, 0.0), (200.0, 0.0)]], width=12.0)
    scn = dict(map=0, waypoints=[(100.0, 0.0), (150.0, 0.0), (190.0, 0.0)], start_heading=0.0, agents=[], ego_attr=(4.5, 2.0, 1.5))
    lt = [dict(stoplines=[(130.0, 0.0, 0.0, 2.0, 9.0, 0)], phases=[(10, [0]), (10, [])])] if lights else None
    return assemble_world([mesh], [scn], A, threshold=0.5, cell=0.25, lights=lt)


def _state(B, A):
    from torchdriveenv_amd.state import EnvState

    st = EnvState(B, A)
    for k in ("x", "y", "psi", "v"):
        st[k][...] = 0
    st["len"][...] = 4.5
    st["wid"][...] = 2.0
    st["present"][...] = 0
    st["present"][::A] = 1
    st["x"][::A] = 100.0
    return st


def test_known_answers_corridor_box_and_red_line():
    world = _corridor_world()
    assert world.arrays["maps"]["n_stop"][0] == 1
    cfg = _abi.default_config(seed=1)
    cfg.flags |= _abi.F_TRAFFIC_LIGHTS
    vo = VectorObs(k_neighbours=2, n_rays=4, ray_range=60.0, ray_step=0.3, neighbour_radius=40.0)
    B, A = 2, 8
    st = _state(B, A)
    # env 0: an agent 20 m straight ahead; env 1: none.  Red light at steps 0..9, green at 10..19
    st["present"][1] = 1
    st["x"][1] = 120.0
    st["len"][1] = 5.0
    st["v"][1] = 3.0
    st["steps"][0], st["steps"][1] = 3, 12
    st["target_idx"][...] = 0
    row = R.vector_obs(cfg, world, st, vo)
    sl = vo.slices()
    road, car, red = row[:, sl["road"]], row[:, sl["car"]], row[:, sl["red_line"]]
    # the corridor is 12 m wide: the left / right rays leave the road at the first sample past 6 + 0.5 m
    want = np.float32(22) * np.float32(0.3)
    assert want > 6.5 and np.float32(21) * np.float32(0.3) <= 6.5
    assert road[0, 1] == want and road[0, 3] == want and road[1, 1] == want
    assert road[0, 0] == 60.0                                        # 100 m of road ahead
    assert road[0, 2] == 60.0
    # a box straight ahead at d = 20 with half length 2.5: 17.5; nothing behind
    assert car[0, 0] == np.float32(17.5) and car[0, 2] == 60.0 and car[1, 0] == 60.0
    # the red line 30 m ahead (half length 1): 29 while red, nothing while green
    assert red[0, 0] == np.float32(29.0) and red[1, 0] == 60.0 and red[0, 2] == 60.0
    cfg.flags &= ~_abi.F_TRAFFIC_LIGHTS
    assert (R.vector_obs(cfg, world, st, vo)[:, sl["red_line"]] == 60.0).all()
    # ego block: v, len, wid, target (0, 0) at the ego, next target 50 m ahead, 2 targets left (of 3), steps / 200, lights
    assert list(row[0, :10]) == [0.0, 4.5, 2.0, 0.0, 0.0, 50.0, 0.0, 2.0, np.float32(3) / np.float32(200), 1.0]
    # the neighbour: valid, 20 m ahead, same heading, relative velocity (3, 0), length 5, width 2; the second entry is empty
    assert list(row[0, sl["neighbours"]].reshape(2, 9)[0]) == [1.0, 20.0, 0.0, 1.0, 0.0, 3.0, 0.0, 5.0, 2.0]
    assert not row[0, sl["neighbours"]].reshape(2, 9)[1].any() and not row[1, sl["neighbours"]].any()


def test_ties_are_ordered_by_slot_and_the_radius_is_strict():
    world = _corridor_world(lights=False)
    cfg = _abi.default_config(seed=1)
    vo = VectorObs(k_neighbours=3, n_rays=0, ray_range=10.0, ray_step=0.5, neighbour_radius=10.0)
    B, A = 1, 8
    st = _state(B, A)
    # slots 5, 2, 6 at the same distance 4 (ahead, left, behind), slot 3 nearer, slot 4 on the radius, slot 7 absent
    for a, (dx, dy) in {5: (4.0, 0.0), 2: (0.0, 4.0), 6: (-4.0, 0.0), 3: (1.0, 0.0), 4: (0.0, -10.0), 7: (2.0, 0.0)}.items():
        st["x"][a], st["y"][a] = 100.0 + dx, dy
        st["present"][a] = a != 7
        st["psi"][a] = 0.5 * a
    row = R.vector_obs(cfg, world, st, vo)
    nb = row[0, vo.slices()["neighbours"]].reshape(3, 9)
    assert list(nb[:, 1]) == [1.0, 0.0, 4.0] and list(nb[:, 2]) == [0.0, 4.0, 0.0]        # slot 3, then 2 before 5; 6 and 4 dropped
    s, c = R.oracle.sincosf(np.float32([1.0]))
    assert nb[1, 3] == c[0] and nb[1, 4] == s[0]                    # slot 2's heading 1.0 against the ego's 0


def test_only_mask_keeps_rows():
    world = _corridor_world(lights=False)
    cfg = _abi.default_config(seed=1)
    vo = VectorObs(k_neighbours=1, n_rays=2, ray_range=10.0, ray_step=0.5)
    st = _state(3, 8)
    prev = np.full((3, vo.dim), 7.0, np.float32)
    row = R.vector_obs(cfg, world, st, vo, only=np.array([0, 1, 0], np.uint8), out=prev)
    assert (row[[0, 2]] == 7.0).all() and (row[1] != 7.0).any()
