"""Static world tables of the batched env: drivable meshes + their grid index, scenarios (WaypointSuite entries),
NPC routes and replay rows.  Host side (numpy); `World.to_device()` uploads them once per GPU (they are
replicated per GPU) and returns the `tde_world` struct of device pointers the C-ABI takes.

Reference anchors:
  * drivable mesh = `map_cfg.road_mesh` handed to `Simulator(road_mesh=...)`      ref gym_env.py:184,260
  * waypoints / car sequences / scenarios = `WaypointSuite`                         ref gym_env.py:63-68,314-316
  * replay rows = `car_sequences` -> replay_states/replay_mask                      ref gym_env.py:275-283
  * agent ordering: slot 0 ego, then scenario agents                                ref gym_env.py:219-228
The real CARLA meshes/lanelets live inside torchdrivesim's package data, which is not part of the reference
repository, so meshes here are synthetic ("Out of scope").
"""
import math

import numpy as np

from . import _abi

# margin that makes the grid classification robust to fp32 evaluation and to the fp32 cell lookup
GRID_MARGIN = 0.05
# grid sizes are rounded up to multiples of GRID_TILE cells
GRID_TILE = 8


def row_shift_of(nx):
    """log2 of the row pitch the cell words of an nx-cell-wide grid are stored with (next power of two >= nx, at least 128:
    a line of the coarse table is 64 cells wide, a 2-bit class tile 32)"""
    return max(7, max(0, int(nx) - 1).bit_length())


CLS2_TILE_W, CLS2_TILE_H = 32, 16          # cells per 128-byte tile of tde_world.cell_cls2
CLEARANCE_UNIT = 0.125   # metres per count of the clearance field (TDE_CLEARANCE_UNIT)


def sub_tiles(a, nx, ny):
    """row-major per-cell words [ny * nx] -> the same words in 8 x 4-cell tiles (tde_abi.h: cell_sub), as many as
    pitch_cells() gives (ny is a multiple of GRID_TILE)"""
    assert ny % 4 == 0
    pitch = 1 << row_shift_of(nx)
    full = np.zeros((ny, pitch), dtype=a.dtype)
    full[:, :nx] = a.reshape(ny, nx)
    return np.ascontiguousarray(full.reshape(ny // 4, 4, pitch // 8, 8).transpose(0, 2, 1, 3)).reshape(-1)


def class_tiles(cls, nx, ny):
    """cell classes [ny * nx] -> uint32 words of the 2-bit class map in 32 x 16-cell tiles (tde_abi.h: cell_cls2); the
    padding holds EMPTY cells.  Returns (words, number of tiles)."""
    pitch = 1 << row_shift_of(nx)
    tx, ty = pitch // CLS2_TILE_W, -(-ny // CLS2_TILE_H)
    full = np.full((ty * CLS2_TILE_H, pitch), _abi.CELL_EMPTY, dtype=np.uint32)
    full[:ny, :nx] = np.asarray(cls, dtype=np.uint32).reshape(ny, nx)
    # 16 cells -> one word, cell ix at bits 2 * (ix & 15)
    w = (full.reshape(ty * CLS2_TILE_H, pitch // 16, 16) << (2 * np.arange(16, dtype=np.uint32))[None, None]).sum(2)
    w = w.astype(np.uint32).reshape(ty, CLS2_TILE_H, tx, 2)                 # [tile row][row in tile][tile col][word]
    return np.ascontiguousarray(w.transpose(0, 2, 1, 3)).reshape(-1), tx * ty


COARSE, COARSE_UNIT = 4, 0.25               # TDE_COARSE_CELLS, TDE_COARSE_UNIT
LARGE_GRID_CELLS = 1 << 21                  # a map with more cells sets TDE_WORLD_LARGE_GRID (tde_abi.h)


def coarse_tiles(cls, count, nx, ny):
    """cell classes and count fields [ny * nx] -> bytes of the coarse table (tde_abi.h: cell_coarse) in 128-byte lines of
    16 x 8 coarse tiles, and the number of lines.  A tile of 4 x 4 cells is FULL / EMPTY when all its cells are, with the
    smallest of their clearances (the distance between the tile and the nearest cell of another class), else MIXED / 0."""
    pitch = 1 << row_shift_of(nx)
    lx, ly = pitch // 64, -(-ny // 32)
    c = np.full((ly * 32, pitch), _abi.CELL_EMPTY, np.uint8)
    k = np.zeros((ly * 32, pitch), np.uint8)
    c[:ny, :nx] = np.asarray(cls, np.uint8).reshape(ny, nx)
    k[:ny, :nx] = np.asarray(count, np.uint8).reshape(ny, nx)
    c4 = c.reshape(ly * 8, COARSE, pitch // COARSE, COARSE)
    lo, hi = c4.min((1, 3)), c4.max((1, 3))
    uni = (lo == hi) & (lo != _abi.CELL_MIXED)
    clear = np.floor(k.reshape(ly * 8, COARSE, pitch // COARSE, COARSE).min((1, 3)) * (CLEARANCE_UNIT / COARSE_UNIT))
    byte = np.where(uni, lo | (np.minimum(clear, 63).astype(np.uint8) << 2), _abi.CELL_MIXED).astype(np.uint8)
    return np.ascontiguousarray(byte.reshape(ly, 8, lx, 16).transpose(0, 2, 1, 3)).reshape(-1), lx * ly


def pitch_cells(a, nx, ny):
    """row-major [ny*nx] cell array -> rows of 2^row_shift words (the padding holds EMPTY cells): the kernels form a
    cell's index as (iy << row_shift) + ix, one instruction (round 1 stored 8x8-cell tiles: ten per lookup with a
    quarter-rate integer multiply, for a cache-line saving that the 4-byte words of a 140 x 140-cell view never showed)"""
    pitch = 1 << row_shift_of(nx)
    out = np.full((ny, pitch), _abi.CELL_EMPTY, dtype=a.dtype)
    out[:, :nx] = a.reshape(ny, nx)
    return out.reshape(-1)


# ------------------------------------------------------------------------------------------------
# grid index of a drivable mesh: built by the library's host code (csrc/tde_gridbuild.h)
# ------------------------------------------------------------------------------------------------
SUB = 4                  # a MIXED cell carries SUB x SUB sub-cell classes (TDE_CELL_SUB)


_GRID_LIB = None


def _grid_lib():
    """the library that holds tde_grid_build / tde_grid_free: libtde_hip.so - or, under TDE_GRID_LIB, a host-compiler build of
    the same source (csrc/tde_gridbuild.h through csrc/tde_grid_host.cpp) with AddressSanitizer / UBSan in it
    (`make -C torchdriveenv_amd/csrc san` -> torchdriveenv_amd/_san/; tests/test_sanitizers.py).  The tables do not depend on which
    one built them."""
    global _GRID_LIB
    import ctypes as C
    import os

    from . import _lib

    path = os.environ.get("TDE_GRID_LIB")
    if not path:
        return _lib.load()
    if _GRID_LIB is None:
        L = C.CDLL(path)
        if L.tde_abi_version() != _abi.TDE_ABI_VERSION:
            raise _lib.TdeError(f"{path}: ABI {L.tde_abi_version()}, expected {_abi.TDE_ABI_VERSION}")
        L.tde_last_error.restype = C.c_char_p
        L.tde_grid_build.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int32,
                                     C.POINTER(C.POINTER(_abi.TdeGrid))]
        L.tde_grid_build.restype = C.c_int
        L.tde_grid_free.argtypes = [C.POINTER(_abi.TdeGrid)]
        L.tde_grid_free.restype = None
        _GRID_LIB = L
    return _GRID_LIB


NEAR_RANGE = 2.0         # metres beyond the threshold the coarse tiles carry a near list for (tde_world.tile_near)


def build_grid_index(tri32, threshold=0.5, cell=0.5, margin=GRID_MARGIN, n_threads=0, near_range=NEAR_RANGE):
    """Uniform-grid index over a triangle soup `tri32` [n,3,2] (fp32 vertices, what kernels and oracle see) for the offroad
    test, through `tde_grid_build` (include/tde_hip.h; rounds 1-3 did this in numpy, seconds per 200-triangle junction).

    Per cell a class - EMPTY: every corner falling in the cell is offroad; FULL: never offroad; MIXED: test the cell's
    candidate triangles - plus, for MIXED cells, the candidate list (identical lists share their records) and the classes
    of its SUB x SUB sub-cells, and for FULL / EMPTY cells a clearance.  All conservative by `margin`, so the HIP kernels'
    masks equal the oracle's brute force (tests/test_oracle_math.py::test_grid_index_equals_brute_force).
    `near_range`: coarse tiles (4 x 4 cells) within threshold + near_range of the mesh also get a NEAR LIST - the triangles among
    which the nearest triangle of any point of the tile is found - for the MAGNITUDE of the offroad infraction
    (ref gym_env.py:427); `tile_near` [ny/4 * nx/4] holds 1 + its first record, `rec_len` its length at that record.
    Returns row-major [ny * nx] numpy arrays (copies) and `rec_tri`, the triangle of every record."""
    import ctypes as C

    from . import _lib

    L = _grid_lib()
    tri32 = np.ascontiguousarray(np.asarray(tri32, dtype=np.float32).reshape(-1, 6))
    gp = C.POINTER(_abi.TdeGrid)()
    rc = L.tde_grid_build(tri32.ctypes.data, len(tri32), float(threshold), float(cell), float(margin), float(near_range),
                          int(n_threads), C.byref(gp))
    if rc != 0:
        raise _lib.TdeError("tde_grid_build: " + (L.tde_last_error().decode() or f"error {rc}"))
    try:
        g = gp.contents
        n = g.nx * g.ny
        out = dict(ox=float(g.ox), oy=float(g.oy), cell=float(g.cell), nx=int(g.nx), ny=int(g.ny), n_lists=int(g.n_lists),
                   cell_class=np.ctypeslib.as_array(g.cell_class, (n,)).copy(),
                   cell_count=np.ctypeslib.as_array(g.cell_count, (n,)).copy(),
                   cell_first=np.ctypeslib.as_array(g.cell_first, (n,)).copy(),
                   cell_sub=np.ctypeslib.as_array(g.cell_sub, (n,)).copy(),
                   rec_tri=np.ctypeslib.as_array(g.rec_tri, (max(1, int(g.n_records)),))[:int(g.n_records)].copy(),
                   rec_len=np.ctypeslib.as_array(g.rec_len, (max(1, int(g.n_records)),))[:int(g.n_records)].copy(),
                   tile_near=np.ctypeslib.as_array(g.tile_near, ((g.nx // COARSE) * (g.ny // COARSE),)).copy(),
                   n_near_lists=int(g.n_near_lists))
    finally:
        L.tde_grid_free(gp)
    return out


def pack_triangles(tri32):
    """Device-side triangle records [n,12] fp32: ax,ay,bx,by | cx,cy,inv|ab|^2,inv|bc|^2 | inv|ca|^2,0,0,0.
    The reciprocals are computed in fp32 exactly as the oracle's `1.0f / len2` so the kernel's distances keep every
    bit while doing no division."""
    t = np.asarray(tri32, dtype=np.float32).reshape(-1, 3, 2)
    out = np.zeros((len(t), 12), dtype=np.float32)
    out[:, 0:6] = t.reshape(-1, 6)
    one = np.float32(1.0)
    for e, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):
        abx = t[:, j, 0] - t[:, i, 0]
        aby = t[:, j, 1] - t[:, i, 1]
        len2 = abx * abx + aby * aby
        with np.errstate(divide="ignore"):
            inv = np.where(len2 > 0, one / np.where(len2 > 0, len2, one), np.float32(0.0)).astype(np.float32)
        out[:, 6 + e] = inv
    return out


# ------------------------------------------------------------------------------------------------
# synthetic drivable meshes
# ------------------------------------------------------------------------------------------------
def strip_mesh(polyline, width, seg_len=5.0):
    """Triangulated road strip of `width` metres around a polyline (list of (x,y)); quads of ~seg_len."""
    pts = np.asarray(polyline, dtype=np.float64)
    tris = []
    for a, b in zip(pts[:-1], pts[1:]):
        d = b - a
        L = float(np.hypot(*d))
        if L == 0:
            continue
        t = d / L
        n = np.array([-t[1], t[0]]) * (0.5 * width)
        k = max(1, int(round(L / seg_len)))
        for i in range(k):
            p = a + d * (i / k)
            q = a + d * ((i + 1) / k)
            tris.append([p - n, q - n, q + n])
            tris.append([p - n, q + n, p + n])
    return np.asarray(tris, dtype=np.float64).reshape(-1, 3, 2)


def disc_mesh(center, radius, n=12):
    c = np.asarray(center, dtype=np.float64)
    ang = np.linspace(0, 2 * math.pi, n + 1)
    ring = c + radius * np.stack([np.cos(ang), np.sin(ang)], -1)
    return np.asarray([[c, ring[i], ring[i + 1]] for i in range(n)], dtype=np.float64)


def corridor_mesh(polylines, width=12.0, seg_len=6.0, joint_radius=None):
    """Drivable corridor around a set of polylines (used to give the shipped WaypointSuite scenarios a mesh:
    their CARLA town meshes are not in the reference repository)."""
    parts = []
    for pl in polylines:
        pl = np.asarray(pl, dtype=np.float64).reshape(-1, 2)
        keep = [0] + [i for i in range(1, len(pl)) if np.hypot(*(pl[i] - pl[i - 1])) > 1.0]   # drop repeated points
        dedup = [keep[0]]
        for i in keep[1:]:
            if np.hypot(*(pl[i] - pl[dedup[-1]])) > 1.0:
                dedup.append(i)
        pl = pl[dedup]
        if len(pl) >= 2:
            parts.append(strip_mesh(pl, width, seg_len))
        r = joint_radius if joint_radius is not None else 0.5 * width
        for p in pl:
            parts.append(disc_mesh(p, r, 8))
    return np.concatenate(parts, 0)


# ------------------------------------------------------------------------------------------------
# World container
# ------------------------------------------------------------------------------------------------
def map_centres(maps, tri):
    """float32 [n_maps, 2]: the centre of the bounding box of every map's mesh (the default camera of render_scene: our reading of
    torchdrivesim, whose `camera_xy` defaults to the world centre - UNPINNED, that package is not available here); (0, 0) for a map
    without triangles.  Light-group descriptors share their mesh's triangles, so they share its centre."""
    maps = np.asarray(maps)
    tri = np.asarray(tri, np.float32).reshape(-1, 3, 2)
    out = np.zeros((len(maps), 2), np.float32)
    for m in range(len(maps)):
        t = tri[int(maps["tri_base"][m]):int(maps["tri_base"][m]) + int(maps["n_tri"][m])].reshape(-1, 2).astype(np.float64)
        if len(t):
            out[m] = 0.5 * (t.min(0) + t.max(0))
    return out


class World:
    """Host copy of every static table the step path reads (numpy, dtypes of _abi.WORLD_DTYPES)."""

    def __init__(self, arrays, ints, threshold=None):
        self.arrays = {k: np.ascontiguousarray(arrays[k], dtype=_abi.WORLD_DTYPES[k]) for k in _abi.WORLD_PTRS}
        self.ints = {k: int(ints[k]) for k in _abi.WORLD_INTS}
        # The offroad distance the grid index was built for: cell classes and candidate lists bake it in
        # (build_grid_index), so kernels run with another threshold would silently return wrong masks.  Checked by
        # check_threshold() wherever a threshold meets a World.  None: unknown (tables assembled by hand).
        self.threshold = None if threshold is None else float(threshold)
        self.has_lights = bool(np.asarray(arrays["maps"])["cycle_steps"].max() > 0)
        self.map_centre = map_centres(self.arrays["maps"], self.arrays["tri"])
        # zero-length tables still need a valid pointer
        for k, a in self.arrays.items():
            if a.size == 0:
                self.arrays[k] = np.zeros(max(1, 1), dtype=a.dtype)
        self._host_struct = None

    def __getstate__(self):                      # the cached ctypes struct holds raw pointers: never pickled
        d = dict(self.__dict__)
        d["_host_struct"] = None
        return d

    @property
    def A(self):
        return self.ints["A"]

    @property
    def n_scn(self):
        return self.ints["n_scn"]

    def host_struct(self):
        """tde_world of HOST pointers (what the CPU oracle takes in the tests)."""
        if self._host_struct is None:
            self._host_struct = _abi.fill_world_struct(self.arrays, self.ints)
        return self._host_struct

    def to_device(self, device, first_gap=True):
        """first_gap=False: the device world has no first-step gap cache (tde_world.first_gap = NULL): every first step runs the
        NPC controller's sweep (what near-field envs need: the cache assumes the NPCs at their spawn records)"""
        import torch

        tens = {}
        for k, a in self.arrays.items():
            if k == "first_gap" and not first_gap:
                tens[k] = None
                continue
            if a.dtype.names is not None:      # record arrays travel as raw bytes
                t = torch.from_numpy(a.reshape(-1).view(np.uint8).copy())
            else:
                t = torch.from_numpy(a.copy())
            tens[k] = t.to(device)
        dw = DeviceWorld(tens, self.ints, self.threshold)
        dw.scene_camera_host = self.scene_cameras()       # (uploaded at the first render_scene(camera="map"), not here)
        return dw

    def map_of_scn(self):
        return np.ascontiguousarray(self.arrays["scn"]["map"])

    def scene_cameras(self):
        """float32 [n_scn, 3]: the "map" camera of every scenario's map (render_scene): the centre of the bounding box of its mesh,
        heading pi/2"""
        cam = np.empty((self.n_scn, 3), np.float32)
        cam[:, :2] = self.map_centre[self.map_of_scn()]
        cam[:, 2] = np.float32(math.pi / 2)
        return cam

    def save(self, path):
        """cache the assembled tables (grid indexes of town-sized meshes take seconds per scenario to build)"""
        blobs = {f"a_{k}": a.reshape(-1).view(np.uint8) if a.dtype.names is not None else a
                 for k, a in self.arrays.items()}
        ints = np.array([self.ints[k] for k in _abi.WORLD_INTS], dtype=np.int64)
        with open(path, "wb") as f:
            np.savez(f, abi=np.int64(_abi.TDE_ABI_VERSION), ints=ints,
                     threshold=np.float64(-1.0 if self.threshold is None else self.threshold), **blobs)

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            if int(z["abi"]) != _abi.TDE_ABI_VERSION:
                raise ValueError(f"{path}: built for ABI {int(z['abi'])}, this library is ABI {_abi.TDE_ABI_VERSION}")
            ints = dict(zip(_abi.WORLD_INTS, (int(v) for v in z["ints"])))
            arrays = {}
            for k in _abi.WORLD_PTRS:
                dt = np.dtype(_abi.WORLD_DTYPES[k])
                a = z[f"a_{k}"]
                arrays[k] = a.view(dt) if dt.names is not None else a
            thr = float(z["threshold"]) if "threshold" in z.files else -1.0
        return cls(arrays, ints, None if thr < 0 else thr)


def cached_world(key, builder, cache_dir=None):
    """`builder()` -> World, built ONCE per machine for a given `key` and shared through a file: the first caller (a file lock
    decides) builds and saves it (World.save), everybody else - the other ranks of a multi-GPU job, whose grid-index builds would
    otherwise run side by side on the same host cores before the first launch - loads the tables (World.load: a read of the page
    cache).  The key is extended by the ABI version and the modification times of the library and of the Python that assembles
    worlds, so a rebuilt package never meets a stale file.  Returns (world, "built" | "loaded")."""
    import fcntl
    import hashlib
    import os
    import tempfile

    here = os.path.dirname(os.path.abspath(__file__))
    stamp = [str(_abi.TDE_ABI_VERSION)]
    for f in ("libtde_hip.so", "world.py", "synth.py", "_abi.py"):
        try:
            stamp.append(str(os.stat(os.path.join(here, f)).st_mtime_ns))
        except OSError:
            stamp.append("-")
    h = hashlib.sha1(("|".join([str(key)] + stamp)).encode()).hexdigest()[:20]
    d = cache_dir or os.environ.get("TDE_WORLD_CACHE") or os.path.join(tempfile.gettempdir(), f"tde_worlds_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, f"world_{h}.npz")
    with open(path + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if os.path.exists(path):
                try:
                    return World.load(path), "loaded"
                except Exception:
                    os.unlink(path)                         # (a torn or foreign file: rebuild)
            w = builder()
            tmp = path + f".tmp{os.getpid()}"
            w.save(tmp)
            os.replace(tmp, path)
            return w, "built"
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def effective_offroad_distance(threshold, squared=False):
    """the distance a box corner may be from the mesh: `threshold`, or sqrt(threshold) when the threshold is applied to
    the SQUARED distance (tde_config.offroad_threshold_squared)"""
    return float(np.sqrt(threshold)) if squared else float(threshold)


def check_threshold(world, threshold, squared=False, what="offroad_threshold"):
    """raise if `world`'s grid index was built for another offroad distance than (threshold, squared) asks for"""
    built = getattr(world, "threshold", None)
    want = effective_offroad_distance(threshold, squared)
    if built is not None and abs(built - want) > 1e-6 * max(1.0, want):
        raise ValueError(f"{what} asks for an offroad distance of {want:g} m but the World's grid index was built for "
                         f"{built:g} m: rebuild the World (assemble_world(..., threshold={want:g}))")


class DeviceWorld:
    def __init__(self, tensors, ints, threshold=None):
        self.tensors = tensors  # keeps the device memory alive
        self.ints = dict(ints)
        self.threshold = threshold
        self.struct = _abi.fill_world_struct(tensors, ints)
        self.scene_camera_host = None   # float32 [n_scn, 3] "map" camera of every scenario (World.scene_cameras; render_scene)
        self._scene_camera = None
        self.near_field = None          # the DeviceNearField of the envs that use this copy (BatchedWaypointEnv(near_field=...))

    @property
    def scene_camera(self):
        """the "map" cameras on the device, uploaded on first use: a world that never renders a scene view allocates nothing more
        than its tables"""
        if self._scene_camera is None and self.scene_camera_host is not None:
            import torch

            self._scene_camera = torch.from_numpy(self.scene_camera_host).to(self.tensors["maps"].device)
        return self._scene_camera


def assemble_world(meshes, scenarios, A, threshold=0.5, cell=0.5, lights=None, light_groups=None, near_range=NEAR_RANGE):
    """meshes: list of [n,3,2] triangle arrays; scenarios: list of dicts with keys
         map (int), waypoints [(x,y)...], start_heading (float),
         start_headings (optional): the lane direction at NH points along the first waypoint segment, entry j at
           p0 + (j + 0.5) / NH * (p1 - p0) - the heading field the reference samples with find_lanelet_directions at the drawn
           start point (ref gym_env.py:359-361); every scenario that gives one must give the same NH, the others get their
           start_heading repeated.  An episode that starts at fraction f of the segment reads entry floor(f * NH)
         agents: list (slots 1..) of dict(state=(x,y,psi,v), attr=(L,W,lr), vdes, route=[(x,y)..] or None,
                                         replay=[(x,y,psi,v)...] or None)
         ego_attr (L,W,lr)
         lights (int, optional): index into `light_groups`
       lights: per mesh None or dict(stoplines=[(x, y, psi, length, width, light)...], phases=[(n_steps, red_lights)...]) - the
         traffic lights every scenario on that mesh sees.
       light_groups: list of dict(map=mesh index, stoplines=..., phases=...) - the lights of ONE NEIGHBOURHOOD of a large map.  The
         kernels walk all stop lines of a scenario's map descriptor and a light is a bit of a 32-bit mask, so a town with hundreds of
         signals is cut up at build time: every group becomes a map descriptor of its own (tde_map: 80 bytes) that SHARES the mesh's
         grid tables and carries only its stop lines and phases; a scenario with `lights=k` is bound to descriptor n_meshes + k.
    """
    assert A >= 1 and (A & (A - 1)) == 0 and A <= _abi.TDE_MAX_AGENTS, f"A must be a power of two <= {_abi.TDE_MAX_AGENTS}"
    lights = lights or [None] * len(meshes)
    light_groups = list(light_groups or [])
    stop_all, phase_all = [], []

    def add_lights(lt):
        """-> (stop_base, n_stop, phase_base, n_phase, cycle_steps) of one set of lights appended to the world's tables"""
        if not lt:
            return len(stop_all), 0, len(phase_all), 0, 0
        n_stop, n_phase, cycle = len(lt["stoplines"]), len(lt["phases"]), 0
        assert n_phase >= 1 and n_stop >= 1 and max(sl[5] for sl in lt["stoplines"]) < 32, "light indices are bits of a 32-bit mask"
        for (x, y, psi, length, width, light) in lt["stoplines"]:
            stop_all.append((x, y, math.cos(psi), math.sin(psi), 0.5 * length, 0.5 * width, light, 0))
        for (n_steps, red) in lt["phases"]:
            cycle += int(n_steps)
            phase_all.append((cycle, sum(1 << int(i) for i in red)))
        return len(stop_all) - n_stop, n_stop, len(phase_all) - n_phase, n_phase, cycle

    maps = np.zeros(len(meshes) + len(light_groups), dtype=_abi.MAP_DTYPE)
    tri_all, word_all, rec_all, cls2_all, sub_all, coarse_all, near_all = [], [], [], [], [], [], []
    tri_base = cell_base = rec_base = cls2_base = coarse_base = near_base = 0
    for m, tri in enumerate(meshes):
        tri = np.asarray(tri, dtype=np.float64).reshape(-1, 3, 2)
        # the kernels see fp32 vertices: index the fp32-rounded mesh
        tri32 = tri.astype(np.float32)
        g = build_grid_index(tri32, threshold, cell, near_range=near_range)
        stop_base, n_stop, phase_base, n_phase, cycle = add_lights(lights[m])
        maps[m] = (g["ox"], g["oy"], g["cell"], np.float32(1.0) / np.float32(g["cell"]), g["nx"], g["ny"], cell_base,
                   tri_base, len(tri), stop_base, n_stop, phase_base, n_phase, cycle,
                   row_shift_of(g["nx"]), cls2_base, rec_base, coarse_base, near_base, 0)
        # cell word = class | count << 2 | first record << 10: the count of a MIXED cell is the length of its candidate list
        # (records from the map's rec_base + first on), that of a FULL / EMPTY cell its clearance (TDE_CLEARANCE_UNITs, rounded
        # down): every point within that distance of ANY point of the cell lies in a cell of the same class - the rasteriser
        # classifies a whole block of pixels with one look-up
        word_all.append(pitch_cells(g["cell_class"].astype(np.uint32) | (g["cell_count"].astype(np.uint32) << 2) |
                                    (g["cell_first"] << 10), g["nx"], g["ny"]))
        recs = pack_triangles(tri32)[g["rec_tri"]]           # per-list copies: one dependent load less in the kernel
        recs[:, 9] = g["rec_len"].astype(np.int32).view(np.float32)   # (the length of a near list rides in its first record)
        rec_all.append(recs)
        near_all.append(g["tile_near"])
        near_base += len(g["tile_near"])
        sub_all.append(sub_tiles(g["cell_sub"], g["nx"], g["ny"]))   # sub-cell classes of the MIXED cells, 8 x 4 cells per line
        c2, ntile = class_tiles(g["cell_class"], g["nx"], g["ny"])
        cls2_all.append(c2)
        cls2_base += ntile
        cb, nline = coarse_tiles(g["cell_class"], g["cell_count"], g["nx"], g["ny"])
        coarse_all.append(cb)
        coarse_base += nline
        tri_all.append(tri32.reshape(-1, 6))
        tri_base += len(tri)
        cell_base += (1 << row_shift_of(g["nx"])) * g["ny"]
        rec_base += len(g["rec_tri"])
        assert cell_base < (1 << 30) and cls2_base < (1 << 26), "world too large for 32-bit cell indices"
    for k, lt in enumerate(light_groups):            # a descriptor per light group: the mesh's grid, the group's lights
        assert 0 <= lt["map"] < len(meshes), "light group on an unknown mesh"
        maps[len(meshes) + k] = maps[lt["map"]]
        d = maps[len(meshes) + k:len(meshes) + k + 1]
        d["stop_base"], d["n_stop"], d["phase_base"], d["n_phase"], d["cycle_steps"] = add_lights(lt)
    S = len(scenarios)
    NW = max(2, max(len(s["waypoints"]) for s in scenarios))
    wp_xy = np.zeros((S, NW, 2), np.float64)
    scn = np.zeros(S, _abi.SCN_DTYPE)
    nhs = {len(sc["start_headings"]) for sc in scenarios if sc.get("start_headings") is not None}
    assert len(nhs) <= 1 and 0 not in nhs, f"scenarios disagree on the number of start-heading samples: {sorted(nhs)}"
    NH = nhs.pop() if nhs else 0
    start_psi = np.zeros((S, max(NH, 1)), np.float32)
    spawn = np.zeros((S, A), _abi.SPAWN_DTYPE)
    spawn["len"], spawn["wid"], spawn["lr"] = 1.0, 1.0, 1.0
    spawn["route"], spawn["replay"] = -1, -1
    routes, replays = [], []
    for si, s in enumerate(scenarios):
        w = np.asarray(s["waypoints"], np.float64)
        assert len(w) >= 2, "a scenario needs at least two waypoints (gym_env.py:353-354)"
        wp_xy[si, :len(w)] = w
        m_of = s["map"]
        if s.get("lights") is not None:
            assert light_groups[s["lights"]]["map"] == s["map"], f"scenario {si}: its light group belongs to another mesh"
            m_of = len(meshes) + s["lights"]
        scn[si] = (m_of, len(w), s["start_heading"], 0)
        start_psi[si] = s["start_heading"] if s.get("start_headings") is None else np.asarray(s["start_headings"], np.float64)
        ego = spawn[si, 0]
        ego["present"] = 1
        ego["len"], ego["wid"], ego["lr"] = s.get("ego_attr", (5.0, 2.0, 1.9))
        ego["x"], ego["y"], ego["psi"] = w[0, 0], w[0, 1], s["start_heading"]
        ags = s.get("agents", [])
        assert len(ags) <= A - 1, f"scenario {si} has {len(ags)} NPCs but only {A - 1} NPC slots"
        for k, ag in enumerate(ags):
            r = spawn[si, k + 1]
            r["present"] = 1
            r["x"], r["y"], r["psi"], r["v"] = ag["state"]
            r["len"], r["wid"], r["lr"] = ag["attr"]
            r["vdes"] = ag.get("vdes", ag["state"][3])
            if ag.get("route") is not None and len(ag["route"]) > 0:
                r["route"], r["route_n"], r["route_wp"] = len(routes), len(ag["route"]), ag.get("route_wp", 0)
                routes.append(np.asarray(ag["route"], np.float32))
                if r["route_wp"] < r["route_n"]:
                    r["tgx0"], r["tgy0"] = routes[-1][r["route_wp"]]          # the first target rides in the record
            if ag.get("replay") is not None and len(ag["replay"]) > 0:
                r["replay"], r["replay_len"] = len(replays), len(ag["replay"])
                replays.append(np.asarray(ag["replay"], np.float32))
    RW = max([len(r) for r in routes], default=1)
    route_xy = np.zeros((max(1, len(routes)), RW, 2), np.float32)
    for i, r in enumerate(routes):
        route_xy[i, :len(r)] = r
    RT = max([len(r) for r in replays], default=1)
    replay_states = np.zeros((max(1, len(replays)), RT, 4), np.float32)
    for i, r in enumerate(replays):
        replay_states[i, :len(r)] = r
    # (16 zero records at the end: the magnitude kernels fetch the first 16 records of a near list before they know its length)
    rec_cat = np.concatenate(rec_all + [np.zeros((16, 12), np.float32)], 0)
    arrays = dict(maps=maps, tri=np.concatenate(tri_all, 0), cell_word=np.concatenate(word_all), cell_tri=rec_cat,
                  cell_cls2=np.concatenate(cls2_all), cell_sub=np.concatenate(sub_all), cell_coarse=np.concatenate(coarse_all),
                  tile_near=np.concatenate(near_all), scn=scn, wp_xy=wp_xy, spawn=spawn, route_xy=route_xy, replay_states=replay_states,
                  stoplines=np.asarray(stop_all, dtype=_abi.STOPLINE_DTYPE) if stop_all
                  else np.zeros(1, _abi.STOPLINE_DTYPE),
                  phases=np.asarray(phase_all, dtype=_abi.PHASE_DTYPE) if phase_all else np.zeros(1, _abi.PHASE_DTYPE),
                  start_psi=start_psi,
                  # the first-step gap cache (tde_first_gap [S][A]): scratch of the device copy, all entries invalid
                  first_gap=np.zeros((S * A, 2), np.uint32))
    large = bool((maps["nx"].astype(np.int64) * maps["ny"]).max() > LARGE_GRID_CELLS)
    ints = dict(n_maps=len(maps), n_scn=S, NW=NW, A=A, n_routes=len(routes), RW=RW, n_replay=len(replays), RT=RT,
                hints=_abi.WORLD_LARGE_GRID if large else 0, NH=NH)
    return World(arrays, ints, threshold)


# ---- near-field candidate tables (tde_near_field; tde_near_field_spawn) ----------------------------------------------------------
NF_LEN, NF_WID, NF_LR = (4.8, 5.5), (1.8, 2.2), (0.82, 0.97)    # the reference's attribute ranges (gym_env.py:193-195)
NF_ROAD_SLACK = 0.05        # a candidate's corners lie this far inside the offroad distance (float64 here, fp32 in the kernels)


def _pt_tri_dist(P, T):
    """float64 distances [q, t] of points P [q, 2] to the (filled) triangles T [t, 3, 2]"""
    Pq = P[:, None, :]
    a, b, c = T[None, :, 0], T[None, :, 1], T[None, :, 2]

    def side(o, u):
        return (u[..., 0] - o[..., 0]) * (Pq[..., 1] - o[..., 1]) - (u[..., 1] - o[..., 1]) * (Pq[..., 0] - o[..., 0])

    def seg(o, u):
        d = u - o
        dd = (d * d).sum(-1)
        t = np.clip(((Pq - o) * d).sum(-1) / np.where(dd > 0, dd, 1.0), 0.0, 1.0)
        q = o + t[..., None] * d - Pq
        return np.sqrt((q * q).sum(-1))

    s1, s2, s3 = side(a, b), side(b, c), side(c, a)
    inside = ((s1 >= 0) & (s2 >= 0) & (s3 >= 0)) | ((s1 <= 0) & (s2 <= 0) & (s3 <= 0))
    return np.where(inside, 0.0, np.minimum(np.minimum(seg(a, b), seg(b, c)), seg(c, a)))


def mesh_distance(pts, tri, reach, cell=8.0):
    """float64 distance of every point of pts [m, 2] to the mesh tri [n, 3, 2], exact up to `reach` (farther: inf)"""
    pts = np.asarray(pts, np.float64).reshape(-1, 2)
    out = np.full(len(pts), np.inf)
    if len(pts) == 0:
        return out
    tri = np.asarray(tri, np.float64).reshape(-1, 3, 2)
    lo, hi = tri.min(1) - reach, tri.max(1) + reach
    pl, ph = pts.min(0), pts.max(0)
    sel = (hi >= pl).all(1) & (lo <= ph).all(1)
    tri, lo, hi = tri[sel], lo[sel], hi[sel]
    if len(tri) == 0:
        return out
    n = np.floor((ph - pl) / cell).astype(np.int64) + 1
    c0 = np.clip(np.floor((lo - pl) / cell).astype(np.int64), 0, n - 1)
    c1 = np.clip(np.floor((hi - pl) / cell).astype(np.int64), 0, n - 1)
    buckets = {}
    for t in range(len(tri)):
        for ix in range(c0[t, 0], c1[t, 0] + 1):
            for iy in range(c0[t, 1], c1[t, 1] + 1):
                buckets.setdefault(ix * n[1] + iy, []).append(t)
    pc = np.floor((pts - pl) / cell).astype(np.int64)
    key = pc[:, 0] * n[1] + pc[:, 1]
    for k in np.unique(key):
        ts = buckets.get(int(k))
        if not ts:
            continue
        q = np.flatnonzero(key == k)
        d = _pt_tri_dist(pts[q], tri[np.asarray(ts)]).min(1)
        out[q] = np.where(d <= reach, d, np.inf)
    return out


def box_corners(x, y, c, s, hl, hw):
    """[n, 4, 2] float64 corners of boxes centred at (x, y), heading (c, s), half extents hl (along) and hw (across)"""
    fx, fy, lx, ly = c * hl, s * hl, -s * hw, c * hw
    return np.stack([np.stack([x + fx + lx, y + fy + ly], -1), np.stack([x + fx - lx, y + fy - ly], -1),
                     np.stack([x - fx - lx, y - fy - ly], -1), np.stack([x - fx + lx, y - fy + ly], -1)], 1)


def sat_overlap(a, b):
    """strict overlap of oriented boxes, pairwise: a and b are tuples (x, y, c, s, hl, hw) of float64 arrays of one length; True
    where no axis of the four separates the pair (touching boxes do not overlap)"""
    dx, dy = b[0] - a[0], b[1] - a[1]
    over = np.ones(np.broadcast(dx, dy).shape, bool)
    for ux, uy in ((a[2], a[3]), (-a[3], a[2]), (b[2], b[3]), (-b[3], b[2])):
        ra = a[4] * np.abs(a[2] * ux + a[3] * uy) + a[5] * np.abs(-a[3] * ux + a[2] * uy)
        rb = b[4] * np.abs(b[2] * ux + b[3] * uy) + b[5] * np.abs(-b[3] * ux + b[2] * uy)
        over &= np.abs(dx * ux + dy * uy) < ra + rb
    return over


def _pairs_overlapping(box):
    """(i, j) index arrays, i < j, of the overlapping pairs among the boxes `box` = (x, y, c, s, hl, hw)"""
    x, y = box[0], box[1]
    r = np.hypot(box[4], box[5])
    n = len(x)
    I, J = [], []
    for i0 in range(0, n, 256):                      # (blocks of rows: the circumcircle filter, then the exact test)
        i = np.arange(i0, min(n, i0 + 256))
        near = (x[i, None] - x[None, :]) ** 2 + (y[i, None] - y[None, :]) ** 2 < (r[i, None] + r[None, :]) ** 2
        near &= np.arange(n)[None, :] > i[:, None]
        ii, jj = np.nonzero(near)
        ii = i[ii]
        ov = sat_overlap(tuple(v[ii] for v in box), tuple(v[jj] for v in box))
        I.append(ii[ov])
        J.append(jj[ov])
    return np.concatenate(I) if I else np.zeros(0, np.int64), np.concatenate(J) if J else np.zeros(0, np.int64)


class NearFieldTable:
    """Host copy of a world's near-field candidate tables (tde_near_field): cand [S][NC] (NF_CAND_DTYPE), nbr [S][NC][K] uint16,
    nbr_n / fixed [S][NC] uint8, n_cand [S] int32, and the parameters of the draw."""

    def __init__(self, cand, nbr, nbr_n, fixed, n_cand, A, radius, clear_ego, count, density, sources=None, routes=False):
        self.cand, self.nbr, self.nbr_n, self.fixed = cand, nbr, nbr_n, fixed
        self.routes = bool(routes)                 # built with NearField(routes=True): envs over it carry tde_state.slot_route
        self.n_cand = np.ascontiguousarray(n_cand, np.int32)
        self.S, self.NC, self.K = cand.shape[0], cand.shape[1], nbr.shape[2]
        self.A, self.radius, self.clear_ego = int(A), float(radius), float(clear_ego)
        self.count, self.density = int(count), int(density)
        self.sources = sources or []

    def struct_of(self, arrays):
        st = _abi.TdeNearField()
        for k in ("cand", "nbr", "nbr_n", "fixed", "n_cand"):
            setattr(st, k, _abi.ptr_of(arrays[k]))
        st.S, st.A, st.NC, st.K = self.S, self.A, self.NC, self.K
        st.radius, st.clear_ego, st.count, st.density = self.radius, self.clear_ego, self.count, self.density
        return st

    def neighbours(self, s, i):
        """scenario-local indices of the neighbours of candidate i of scenario s"""
        return self.nbr[s, i, :self.nbr_n[s, i]].astype(np.int64)

    def to_device(self, device):
        import torch

        tens = dict(cand=torch.from_numpy(self.cand.reshape(-1).view(np.float32).copy()).to(device),
                    nbr=torch.from_numpy(self.nbr.reshape(-1).view(np.int16).copy()).to(device),
                    nbr_n=torch.from_numpy(self.nbr_n.reshape(-1).copy()).to(device),
                    fixed=torch.from_numpy(self.fixed.reshape(-1).copy()).to(device),
                    n_cand=torch.from_numpy(self.n_cand.copy()).to(device))
        return DeviceNearField(self, tens)


class DeviceNearField:
    def __init__(self, table, tensors):
        self.table, self.tensors = table, tensors          # (the tensors keep the device memory alive)
        self.struct = table.struct_of(tensors)


def trace_heading_field(field, x, y, psi, pitch, n):
    """float64 [n, 2]: n points ahead of (x, y), each `pitch` metres from the last along the lane direction `field(x, y)` gives
    there (the candidate's own heading for the first step; where the field gives none - a junction's interior - straight on)"""
    out = np.empty((n, 2))
    for k in range(n):
        x, y = x + pitch * math.cos(psi), y + pitch * math.sin(psi)
        out[k] = x, y
        h = field(float(x), float(y))
        if h is not None:
            h = float(np.asarray(h, np.float64).reshape(-1)[0])
            if np.isfinite(h):
                psi = h
    return out


def polyline_ahead(pl, seg, t, pitch, n):
    """float64 [<= n, 2]: points every `pitch` metres of arc length along the polyline `pl` past the point `t` metres into its segment
    `seg`, up to the polyline's end"""
    p = np.asarray(pl, np.float64).reshape(-1, 2)
    out = []
    need = pitch
    for i in range(int(seg), len(p) - 1):
        a, b = p[i], p[i + 1]
        d = float(np.hypot(*(b - a)))
        at = t if i == seg else 0.0
        while d > 0 and at + need <= d and len(out) < n:
            at += need
            need = pitch
            out.append(a + (b - a) * (at / d))
        need -= max(0.0, d - at)
        if len(out) >= n:
            break
    return np.asarray(out, np.float64).reshape(-1, 2)


def _append_routes(world, rows, route_points):
    """the polylines `rows` (float32 [k, 2] each) as rows n_routes, n_routes + 1, ... of the world's route table, in place: RW grows to
    max(RW, route_points), the new rows are padded with zeros as the others are"""
    n0, RW0 = world.ints["n_routes"], world.ints["RW"]
    RW = max(RW0, int(route_points))
    n = n0 + len(rows)
    id_max, len_max = (1 << _abi.CACHE_ID_BITS) - 1, 1 << (32 - _abi.CACHE_ID_BITS)
    if n >= id_max or RW >= len_max:
        raise ValueError(f"near-field routes: {n} routes of up to {RW} waypoints, the per-slot route word holds ids below {id_max} and "
                         f"lengths below {len_max}: thin the candidates (near_field.pitch) or shorten the routes (route_points)")
    table = np.zeros((n, RW, 2), np.float32)
    if n0:
        table[:n0, :RW0] = world.arrays["route_xy"].reshape(-1, RW0, 2)[:n0]
    for i, r in enumerate(rows):
        table[n0 + i, :len(r)] = r
    world.arrays["route_xy"] = np.ascontiguousarray(table)
    world.ints["n_routes"], world.ints["RW"] = n, RW
    world._host_struct = None


def build_near_field(world, positions, nf, seed, density=0, tracers=None):
    """The near-field candidate table of `world` (NearFieldTable) from candidate positions per scenario (`positions[s]`: float
    array [m, 3] of x, y, psi) and a config.NearField: candidates within radius + |p1 - p0| of the first waypoint p0 (every ego
    start on the first segment), whose boxes are on the drivable surface (every corner within the world's offroad distance minus
    NF_ROAD_SLACK of the scenario's mesh, float64); attributes and desired speeds drawn from a generator seeded by (seed, scenario);
    at most TDE_NF_MAX_CAND per scenario (the nearest to p0); neighbour lists and fixed-conflict bits from an exact float64 SAT of
    the boxes inflated by margin / 2 each; candidates with more than TDE_NF_MAX_NBR neighbours dropped.

    With `nf.routes` every kept candidate also gets a route: `tracers[s](i, x, y, psi)` -> float64 [k, 2], the waypoints ahead of entry i
    of `positions[s]` (env.near_field_positions builds the tracers: the lane-direction field stepped `route_pitch` at a time, the rest of
    the polyline the candidate was resampled from, or the `candidates` hook's own route; None: none).  Of those, leading points that are
    not ahead of the candidate in its own frame are dropped; the route then ends before the first waypoint (float32, as stored) farther
    than the offroad distance minus NF_ROAD_SLACK from the mesh - the predicate the box corners pass - and after `route_points` waypoints.
    A route of fewer than two waypoints is no route (the candidate's route words stay 0).  The routes are appended to THE WORLD'S route
    table in place (rows past the scenario routes; equal polylines share a row), so build the table before the world is uploaded."""
    import warnings

    S, A = world.n_scn, world.A
    if len(positions) != S:
        raise ValueError(f"positions for {len(positions)} scenarios, the world has {S}")
    thr = 0.5 if world.threshold is None else float(world.threshold)
    tri_all = world.arrays["tri"].reshape(-1, 3, 2).astype(np.float64)
    maps, scn, wp, spawn = world.arrays["maps"], world.arrays["scn"], world.arrays["wp_xy"], world.arrays["spawn"]
    hm = 0.5 * float(nf.margin)
    lo_v, hi_v = (float(v) for v in nf.speed)
    r_cand = math.hypot(0.5 * NF_LEN[1], 0.5 * NF_WID[1])
    r_ego = float(np.hypot(0.5 * spawn["len"][:, 0].astype(np.float64), 0.5 * spawn["wid"][:, 0].astype(np.float64)).max())
    if float(nf.clear_ego) < r_cand + r_ego + float(nf.margin):
        raise ValueError(f"near_field.clear_ego = {nf.clear_ego:g} m is below the largest circumradii of the ego ({r_ego:.3f}) and of a "
                         f"candidate ({r_cand:.3f}) plus margin ({nf.margin:g}): a spawned car could overlap the ego")
    rows = []
    routes = bool(getattr(nf, "routes", False)) and tracers is not None
    n_pts = int(getattr(nf, "route_points", 32))
    new_routes, row_of = [], {}                                 # polylines to append to the world's route table; bytes -> row
    for si in range(S):
        P = np.asarray(positions[si], np.float64).reshape(-1, 3)
        orig = np.flatnonzero(np.isfinite(P).all(1))           # (index into positions[si]: what a tracer is asked for)
        P = P[orig]
        p0, p1 = wp[si, 0], wp[si, 1]
        reach = float(nf.radius) + float(np.hypot(*(p1 - p0)))
        near = np.hypot(P[:, 0] - p0[0], P[:, 1] - p0[1]) <= reach
        P, orig = P[near], orig[near]
        m = len(P)
        rng = np.random.default_rng([int(seed) & 0xFFFFFFFFFFFFFFFF, si])
        L = rng.uniform(*NF_LEN, m).astype(np.float32)
        W = rng.uniform(*NF_WID, m).astype(np.float32)
        LR = rng.uniform(*NF_LR, m).astype(np.float32)
        V = rng.uniform(lo_v, hi_v, m).astype(np.float32)
        x32, y32, p32 = P[:, 0].astype(np.float32), P[:, 1].astype(np.float32), P[:, 2].astype(np.float32)
        X, Y, psi = x32.astype(np.float64), y32.astype(np.float64), p32.astype(np.float64)
        c, s = np.cos(psi), np.sin(psi)
        hl, hw = 0.5 * L.astype(np.float64), 0.5 * W.astype(np.float64)
        md = maps[int(scn["map"][si])]
        mesh = tri_all[int(md["tri_base"]):int(md["tri_base"]) + int(md["n_tri"])]
        d = mesh_distance(box_corners(X, Y, c, s, hl, hw).reshape(-1, 2), mesh, thr).reshape(m, 4)
        keep = np.flatnonzero((d <= thr - NF_ROAD_SLACK).all(1))
        if len(keep) > _abi.NF_MAX_CAND:
            dist = np.hypot(X[keep] - p0[0], Y[keep] - p0[1])
            warnings.warn(f"near field, scenario {si}: {len(keep)} candidates, the {_abi.NF_MAX_CAND} nearest to the first waypoint are "
                          f"kept (raise near_field.pitch to thin them)", stacklevel=3)
            keep = np.sort(keep[np.argsort(dist, kind="stable")[:_abi.NF_MAX_CAND]])
        while True:                                                 # (dropping the crowded ones only lowers the others' counts)
            box = (X[keep], Y[keep], c[keep], s[keep], hl[keep] + hm, hw[keep] + hm)
            I, J = _pairs_overlapping(box)
            cnt = np.bincount(np.concatenate([I, J]), minlength=len(keep))
            crowded = cnt > _abi.NF_MAX_NBR
            if not crowded.any():
                break
            warnings.warn(f"near field, scenario {si}: {int(crowded.sum())} candidates overlap more than {_abi.NF_MAX_NBR} others and are "
                          f"dropped (raise near_field.pitch)", stacklevel=3)
            keep = keep[~crowded]
        n = len(keep)
        fixed = np.zeros(n, np.uint8)
        ag = spawn[si, 1:][spawn[si, 1:]["present"] != 0]
        if len(ag) and n:
            ca = ag["psi"].astype(np.float64)
            abox = (ag["x"].astype(np.float64), ag["y"].astype(np.float64), np.cos(ca), np.sin(ca),
                    0.5 * ag["len"].astype(np.float64) + hm, 0.5 * ag["wid"].astype(np.float64) + hm)
            ov = sat_overlap(tuple(v[:, None] for v in box), tuple(v[None, :] for v in abox))
            fixed = ov.any(1).astype(np.uint8)
        nbrs = [[] for _ in range(n)]
        for i, j in zip(I.tolist(), J.tolist()):
            nbrs[i].append(j)
            nbrs[j].append(i)
        rec = np.zeros(n, _abi.NF_CAND_DTYPE)
        k = keep
        rec["x"], rec["y"], rec["psi"] = x32[k], y32[k], p32[k]
        rec["c"], rec["s"] = c[k].astype(np.float32), s[k].astype(np.float32)
        rec["len"], rec["wid"], rec["lr"], rec["vdes"] = L[k], W[k], LR[k], V[k]
        if routes and tracers[si] is not None and n:
            traced = []
            for j in k:
                r = tracers[si](int(orig[j]), X[j], Y[j], psi[j])
                r = np.zeros((0, 2)) if r is None else np.asarray(r, np.float64).reshape(-1, 2)
                r = r[np.isfinite(r).all(1)].astype(np.float32)
                ahead = (r[:, 0].astype(np.float64) - X[j]) * c[j] + (r[:, 1].astype(np.float64) - Y[j]) * s[j] > 0.0
                traced.append(r[int(np.argmax(ahead)) if ahead.any() else len(r):][:n_pts])
            flat = np.concatenate(traced, 0).astype(np.float64)
            on = mesh_distance(flat, mesh, thr) <= thr - NF_ROAD_SLACK
            at = 0
            for q, r in enumerate(traced):
                ok = on[at:at + len(r)]
                at += len(r)
                r = r[:len(r) if ok.all() else int(np.argmin(ok))]
                if len(r) < 2:
                    continue
                key = r.tobytes()
                if key not in row_of:
                    row_of[key] = world.ints["n_routes"] + len(new_routes)
                    new_routes.append(r)
                rec["route"][q], rec["route_wp"][q], rec["route_n"][q] = row_of[key] + 1, 0, len(r)
        rows.append((rec, [sorted(v) for v in nbrs], fixed))
    NC = max(1, max(len(r[0]) for r in rows))
    K = max(1, max((len(v) for r in rows for v in r[1]), default=1))
    cand = np.zeros((S, NC), _abi.NF_CAND_DTYPE)
    nbr = np.zeros((S, NC, K), np.uint16)
    nbr_n = np.zeros((S, NC), np.uint8)
    fixed = np.zeros((S, NC), np.uint8)
    n_cand = np.zeros(S, np.int32)
    for si, (rec, nb, fx) in enumerate(rows):
        n = len(rec)
        n_cand[si] = n
        cand[si, :n] = rec
        fixed[si, :n] = fx
        for i, v in enumerate(nb):
            nbr_n[si, i] = len(v)
            nbr[si, i, :len(v)] = v
    if new_routes:
        _append_routes(world, new_routes, n_pts)
    return NearFieldTable(cand, nbr, nbr_n, fixed, n_cand, A, nf.radius, nf.clear_ego, nf.count, density,
                          routes=bool(getattr(nf, "routes", False)))
