"""tde_render_scene timings (render_mode="video" frames): one and 64 views of 1024 x 1024 at fov 500 (junction world, town), and
WaypointSuiteEnv.step with and without video mode at 256^2 and 1024^2.  Prints one JSON line.  Run it under
`rocprofv3 --kernel-trace --stats` for the kernels' own durations (profiles/README.md)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from torchdriveenv_amd import _abi, ops  # noqa: E402
from torchdriveenv_amd.state import EnvState  # noqa: E402
from torchdriveenv_amd.synth import synthetic_town, synthetic_world  # noqa: E402

dev = torch.device("cuda:0")


def time_us(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = None
    for _ in range(2):                      # the faster of two timed regions (a host hiccup is not device time)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / n
        best = us if best is None else min(best, us)
    return best


out = {}
for name, world in (("junctions", synthetic_world(n_scn=64, A=16, seed=0, n_maps=4)), ("town", synthetic_town(n_scn=64, A=16, seed=0))):
    dw = world.to_device(dev)
    cfg = _abi.default_config(seed=1)
    B = 64
    st = EnvState(B, 16, device=dev, with_info=False)
    ops.env_reset(cfg, dw, st)
    for n in (1, 64):
        envs = torch.arange(n, dtype=torch.int32, device=dev)
        img = torch.empty((n, 3, 1024, 1024), dtype=torch.uint8, device=dev)
        views = ops.scene_views(dw, st, envs, "map")
        from torchdriveenv_amd import _lib
        import ctypes as C
        L = _lib.load()
        strm = _lib.current_stream(dev)

        def call():
            _lib.check(L.tde_render_scene(C.byref(cfg), C.byref(dw.struct), C.byref(st.struct), views.data_ptr(), n, 1024, 1024,
                                          500.0, _abi.RENDER_LEFT_HANDED, img.data_ptr(), strm))
        us = time_us(call)
        wbytes = n * 3 * 1024 * 1024
        out[f"{name}_views{n}_1024_fov500"] = dict(us=us, write_GBps=wbytes / us / 1e3)
        del img

# WaypointSuiteEnv.step, with and without video mode
from tests.golden_util import write_validation_suite_yaml  # noqa: E402
from torchdriveenv_amd.config import EnvConfig, WaypointSuite  # noqa: E402
from torchdriveenv_amd.env import make  # noqa: E402
from torchdriveenv_amd.loaders import load_waypoint_suite_data  # noqa: E402
import tempfile  # noqa: E402

d = tempfile.mkdtemp()
val = load_waypoint_suite_data(write_validation_suite_yaml(os.path.join(d, "v.yml")))
one = WaypointSuite(locations=val.locations[:1], waypoint_suite=val.waypoint_suite[:1], scenarios=val.scenarios[:1],
                    car_sequence_suite=val.car_sequence_suite[:1])
a = torch.tensor([0.3, 0.0])
for mode, res in (("rgb_array", None), ("video", 256), ("video", 1024)):
    kw = dict(seed=4, use_background_traffic=False, max_environment_steps=100000, terminated_at_infraction=False, device="cuda:0")
    if res:
        kw.update(video_res=res, video_fov=120.0 if res == 256 else 500.0, video_filename=os.path.join(d, "v.mp4"))
    env = make(EnvConfig(render_mode=mode, **kw), one)
    env.reset()
    for _ in range(10):
        env.step(a)
    best = None
    for _ in range(2):
        if mode == "video":
            env.reset()                       # (keeps the frame list short)
        t0 = time.perf_counter()
        for _ in range(50):
            env.step(a)
        us = (time.perf_counter() - t0) * 1e6 / 50
        best = us if best is None else min(best, us)
    out[f"suite_step_{mode}" + (f"_{res}" if res else "")] = dict(us=best)
print(json.dumps(out))
