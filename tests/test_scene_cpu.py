"""CPU side of tde_render_scene and render_mode="video": the C-ABI's argument checks (nothing is launched), the map camera, the
video writer's choice and the reference's one-frame quirk, and validate() still refusing "video" for the batched env."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

from torchdriveenv_amd import _abi
from torchdriveenv_amd.config import EnvConfig, validate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _structs(A=16):
    """host structs that pass check_env_args (no pointer is dereferenced before the checks fail)"""
    cfg = _abi.default_config()
    w, st = _abi.TdeWorld(), _abi.TdeState()
    w.A = st.A = A
    st.B = 2
    for k in ("cell_word", "cell_tri", "cell_cls2", "cell_sub", "cell_coarse"):
        setattr(w, k, 4096)            # non-NULL: the calls below fail (or return) before any device access
    return cfg, w, st


def test_render_scene_argument_checks_through_ctypes():
    from torchdriveenv_amd import _lib, build

    build.build()
    L = _lib.load()
    cfg, w, st = _structs()
    v, o = C.c_void_p(4096), C.c_void_p(8192)

    def call(n=1, H=64, W=64, fov=35.0, views=v, out=o, A=None):
        s = st
        if A is not None:
            s = _abi.TdeState()
            s.A, s.B = A, 2
        return L.tde_render_scene(C.byref(cfg), C.byref(w), C.byref(s), views, n, H, W, fov, 0, out, None)

    assert call(n=0) == 0                                             # a no-op: nothing launched
    assert call(n=0, views=None, out=None) == 0
    for kw, what in ((dict(H=0), "H and W"), (dict(W=0), "H and W"), (dict(H=4097), "H and W"), (dict(W=5000), "H and W"),
                     (dict(fov=0.0), "fov"), (dict(fov=-1.0), "fov"), (dict(fov=float("inf")), "fov"), (dict(fov=float("nan")), "fov"),
                     (dict(n=-1), "n_views"), (dict(views=None), "NULL"), (dict(out=None), "NULL"), (dict(A=3), "power of two")):
        assert call(**kw) != 0, kw
        err = L.tde_last_error()
        assert b"tde_render_scene" in err and what.encode() in err, (kw, err)
    assert L.tde_render_scene(None, C.byref(w), C.byref(st), v, 1, 8, 8, 1.0, 0, o, None) != 0
    w2 = _abi.TdeWorld()
    w2.A = 16
    assert L.tde_render_scene(C.byref(cfg), C.byref(w2), C.byref(st), v, 1, 8, 8, 1.0, 0, o, None) != 0
    assert b"grid index" in L.tde_last_error()


def test_scene_view_struct_matches_header(tmp_path):
    import subprocess

    prog = r'''
#include <stdio.h>
#include <stddef.h>
#include "tde_hip.h"
int main(void) { printf("%zu %zu %zu %zu\n", sizeof(tde_scene_view), offsetof(tde_scene_view, x), offsetof(tde_scene_view, y),
                        offsetof(tde_scene_view, psi)); return 0; }'''
    c = tmp_path / "s.c"
    c.write_text(prog)
    exe = str(tmp_path / "s")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", exe], check=True)
    got = [int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    T = _abi.TdeSceneView
    assert got == [C.sizeof(T), T.x.offset, T.y.offset, T.psi.offset] == [16, 4, 8, 12]


def test_map_camera_is_the_centre_of_the_mesh_bounding_box():
    from torchdriveenv_amd.synth import synthetic_world
    from torchdriveenv_amd.world import World, map_centres

    maps = np.zeros(3, _abi.MAP_DTYPE)
    maps["tri_base"], maps["n_tri"] = (0, 2, 2), (2, 1, 0)
    tri = np.array([[0, 0, 10, 0, 0, 4], [-6, 2, 1, 1, 3, 20], [100, 50, 102, 51, 101, 58]], np.float32)
    c = map_centres(maps, tri)
    assert c.dtype == np.float32 and np.array_equal(c, np.array([[2.0, 10.0], [101.0, 54.0], [0.0, 0.0]], np.float32))
    w = synthetic_world(n_scn=6, A=8, seed=1, n_maps=2)
    cam = w.scene_cameras()
    m = w.arrays["maps"]
    for s, mi in enumerate(w.map_of_scn()):
        t = w.arrays["tri"][m["tri_base"][mi]:m["tri_base"][mi] + m["n_tri"][mi]].reshape(-1, 2).astype(np.float64)
        assert np.allclose(cam[s, :2], 0.5 * (t.min(0) + t.max(0)), atol=1e-4)
    assert (cam[:, 2] == np.float32(np.pi / 2)).all()
    # a World rebuilt from its tables (a cache file) has the same cameras
    assert np.array_equal(World(w.arrays, w.ints).scene_cameras(), cam)


def _frames(n, H=6, W=5):
    import torch

    rng = np.random.default_rng(0)
    return [torch.from_numpy(rng.integers(0, 256, (1, 3, H, W), dtype=np.uint8)) for _ in range(n)]


class _Writer:
    made = []

    def __init__(self, filename, fourcc, fps, frameSize):
        self.args = (filename, fourcc, fps, frameSize)
        self.frames = []
        self.released = False
        _Writer.made.append(self)

    def write(self, f):
        self.frames.append(np.array(f, copy=True))

    def release(self):
        self.released = True


def _fake_cv2():
    m = types.ModuleType("cv2")
    m.VideoWriter = _Writer
    m.VideoWriter_fourcc = lambda *c: "".join(c)
    return m


def test_close_writes_bgr_hwc_mp4v_with_cv2(tmp_path, monkeypatch):
    from torchdriveenv_amd.video import VideoRecorder

    monkeypatch.setitem(sys.modules, "cv2", _fake_cv2())
    _Writer.made.clear()
    rec = VideoRecorder(str(tmp_path / "v.mp4"))
    frames = _frames(3)
    for f in frames:
        rec.append(f)
    assert rec.close() == str(tmp_path / "v.mp4")
    (wr,) = _Writer.made
    assert wr.args == (str(tmp_path / "v.mp4"), "mp4v", 10, (5, 6)) and wr.released
    for got, f in zip(wr.frames, frames):
        assert np.array_equal(got, f[0].numpy().transpose(1, 2, 0)[:, :, ::-1])


def test_close_falls_back_to_a_gif_then_raises(tmp_path, monkeypatch):
    from torchdriveenv_amd.video import VideoRecorder

    pytest.importorskip("PIL")
    from PIL import Image

    monkeypatch.setitem(sys.modules, "cv2", None)                     # import cv2 -> ImportError
    rec = VideoRecorder(str(tmp_path / "v.mp4"))
    frames = _frames(4)
    for f in frames:
        rec.append(f)
    with pytest.warns(UserWarning, match="GIF"):
        path = rec.close()
    assert path == str(tmp_path / "v.gif") and not os.path.exists(tmp_path / "v.mp4")
    with Image.open(path) as im:
        assert im.size == (5, 6) and im.n_frames == 4
    monkeypatch.setitem(sys.modules, "PIL", None)
    with pytest.raises(ImportError, match="cv2"):
        rec.close()
    assert len(rec.frames) == 4                                       # the frames are kept


def test_one_frame_list_writes_nothing(tmp_path, monkeypatch):
    """the reference's quirk: a VecEnv auto-reset on the last step starts a new list (one frame) and close() writes nothing"""
    from torchdriveenv_amd.video import VideoRecorder

    monkeypatch.setitem(sys.modules, "cv2", _fake_cv2())
    _Writer.made.clear()
    rec = VideoRecorder(str(tmp_path / "v.mp4"))
    for f in _frames(5):
        rec.append(f)
    rec.start()
    rec.append(_frames(1)[0])
    assert rec.close() is None and not _Writer.made


def test_validate_still_rejects_video_for_the_batched_env():
    with pytest.raises(NotImplementedError, match="video"):
        validate(EnvConfig(render_mode="video"))


def test_reference_surface_declares_video():
    from torchdriveenv_amd.env import WaypointSuiteEnv, make

    assert "video" in WaypointSuiteEnv.metadata["render_modes"]
    import inspect
    assert "video_camera" in inspect.signature(make).parameters
