"""The tables of the grid index themselves, for every world of the mesh zoo (tests/mesh_zoo.py) at both cell sizes and at the squared
reading of the threshold: cell classes, sub-cell classes and candidate lists against brute force; the 2-bit class map; the clearance
of every FULL / EMPTY cell word and of every coarse tile, exactly over the cell rectangles and by brute force at random points; the
saturated clearances of `islands`.  The kernels and the oracle share one float32 contract, so these are equalities, no tolerances.

The specifications are include/tde_abi.h's (tde_world.cell_word / cell_cls2 / cell_sub / cell_coarse), their addressing written out
in numpy here; the truth is oracle.point_mesh_d2 over every triangle of the mesh."""
import numpy as np
import pytest

from oracle import oracle
from tests import mesh_zoo as Z
from torchdriveenv_amd import _abi, _lib
from torchdriveenv_amd.world import CLEARANCE_UNIT, COARSE_UNIT, LARGE_GRID_CELLS, build_grid_index

EMPTY, MIXED, FULL = _abi.CELL_EMPTY, _abi.CELL_MIXED, _abi.CELL_FULL
CASES = [(n, c, False) for n in Z.NAMES for c in Z.CELLS] + [(Z.SQUARED, c, True) for c in Z.CELLS]
IDS = [f"{n}-{c}{'-squared' if s else ''}" for n, c, s in CASES]
zoo = pytest.mark.parametrize("name,cell,squared", CASES, ids=IDS)
_CTX = {}


class Ctx:
    """a zoo world with its cell words unpacked [ny, nx], its poses and the distances between cell rectangles"""

    def __init__(self, name, cell, squared):
        self.where = Z.where(name, cell, squared)
        self.w = w = Z.world(name, cell, squared)
        self.m = m = w.arrays["maps"][0]
        self.nx, self.ny, self.rs = int(m["nx"]), int(m["ny"]), int(m["row_shift"])
        assert int(m["cell_base"]) == 0 and int(m["cls2_base"]) == 0 and int(m["coarse_base"]) == 0 and int(m["rec_base"]) == 0
        assert float(m["cell"]) == cell and float(m["inv_cell"]) == 1.0 / cell
        self.words = w.arrays["cell_word"].reshape(self.ny, 1 << self.rs)
        assert (self.words[:, self.nx:] == EMPTY).all(), f"{self.where}: padding words are not EMPTY / 0"
        wd = self.words[:, :self.nx]
        self.cls, self.cnt = (wd & 3).astype(np.int64), ((wd >> 2) & 255).astype(np.int64)
        self.tri = w.arrays["tri"][int(m["tri_base"]):int(m["tri_base"]) + int(m["n_tri"])]
        self.thr = float(w.threshold)
        self.thr2 = np.float32(0.5) if squared else np.float32(0.5) * np.float32(0.5)        # (tde_config.offroad_threshold_squared)
        self.poses = Z.poses(w, 320, np.random.default_rng([5, Z.NAMES.index(name)]))
        # cells the clearance field can reach, plus the one-cell dilation and one to spare: a distance capped there decides every
        # clearance up to the cap of 255 units
        self.rmax = int(np.ceil(255 * CLEARANCE_UNIT / cell)) + 2
        self.D2 = {c: rect_distance2(self.cls, c, self.rmax, outside_is_other=(c == FULL)) for c in (EMPTY, FULL)}

    def brute_near(self, x, y):
        """brute force over every triangle: the point is within the threshold of the mesh"""
        return np.array([oracle.point_mesh_d2(a, b, self.tri) <= self.thr2 for a, b in zip(np.float32(x), np.float32(y))])


def ctx(name, cell, squared):
    k = (name, cell, squared)
    if k not in _CTX:
        _CTX[k] = Ctx(*k)
    return _CTX[k]


def rect_distance2(cls, c, rmax, outside_is_other):
    """int64 [ny, nx]: the squared distance, in cells, between the rectangle of every cell and the nearest rectangle of a cell of
    another class than c, capped at rmax^2 - exact, by dilating on the class array: two cell rectangles dx, dy cells apart are
    sqrt(max(|dx| - 1, 0)^2 + max(|dy| - 1, 0)^2) cells from each other, which is the distance between the cells' indices after the
    other-class set has been dilated by one cell.  Points outside the grid are off the road: they count as another class than FULL
    (outside_is_other) and as EMPTY."""
    ny, nx = cls.shape
    other = np.full((ny + 2, nx + 2), bool(outside_is_other))
    other[1:-1, 1:-1] = cls != c
    dil = np.zeros_like(other)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            dil[max(0, dy):ny + 2 + min(0, dy), max(0, dx):nx + 2 + min(0, dx)] |= other[max(0, -dy):ny + 2 + min(0, -dy), max(0, -dx):nx + 2 + min(0, -dx)]
    dil = dil[1:-1, 1:-1]
    # along the rows: the distance to the nearest dilated cell on either side
    idx = np.arange(nx)[None, :]
    big = 4 * (nx + rmax)
    left = idx - np.maximum.accumulate(np.where(dil, idx, -big), axis=1)
    right = np.minimum.accumulate(np.where(dil, idx, big)[:, ::-1], axis=1)[:, ::-1] - idx
    g = np.minimum(np.minimum(left, right), rmax).astype(np.int64)
    g2 = g * g
    d2 = g2.copy()
    for dy in range(1, rmax):
        np.minimum(d2[dy:], g2[:-dy] + dy * dy, out=d2[dy:])
        np.minimum(d2[:-dy], g2[dy:] + dy * dy, out=d2[:-dy])
    return np.minimum(d2, rmax * rmax)


def points_within(rng, x0, y0, w, h, reach, n):
    """n float32 points within `reach` of the rectangle [x0, x0 + w] x [y0, y0 + h]: a point of it plus a vector no longer than
    0.999 reach"""
    ang, r = rng.uniform(0, 2 * np.pi, n), 0.999 * reach * np.sqrt(rng.uniform(0, 1, n))
    return (np.float32(x0 + rng.uniform(0, w, n) + r * np.cos(ang)), np.float32(y0 + rng.uniform(0, h, n) + r * np.sin(ang)))


def sample_uniform_cells(c, field, cls_of, rng, n):
    """indices (iy, ix) of up to n entries of class cls_of with a positive clearance `field`, the largest clearances among them"""
    iy, ix = np.nonzero((c == cls_of) & (field > 0))
    if len(iy) == 0:
        return iy, ix
    pick = rng.choice(len(iy), size=min(n, len(iy)), replace=False)
    top = np.argsort(field[iy, ix], kind="stable")[-8:]
    pick = np.unique(np.concatenate([pick, top]))
    return iy[pick], ix[pick]


@zoo
def test_the_world_is_worth_testing(name, cell, squared):
    """what keeps the other tests honest, from the oracle and the mesh alone: all three cell classes; MIXED cells with sub-cells of
    all three classes; between 15 % and 85 % of the pose corners off the road by brute force; at least 5 % of the poses outside
    the grid; some poses 400 m away"""
    c = ctx(name, cell, squared)
    assert all((c.cls == k).any() for k in (EMPTY, MIXED, FULL)), f"{c.where}: classes {np.bincount(c.cls.ravel(), minlength=3)}"
    iy, ix = np.nonzero(c.cls == MIXED)
    sub = c.w.arrays["cell_sub"][((((iy >> 2) << (c.rs - 3)) + (ix >> 3)) << 5) + ((iy & 3) << 3) + (ix & 7)]
    codes = (sub[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None]) & 3
    assert all((codes == k).any() for k in (EMPTY, MIXED, FULL)), f"{c.where}: sub-cell classes {np.bincount(codes.ravel(), minlength=3)}"
    cx, cy = Z.pose_corners(c.w, c.poses)
    off = ~c.brute_near(cx, cy)
    assert 0.15 <= off.mean() <= 0.85, f"{c.where}: {off.mean():.3f} of the pose corners are off the road"
    out = Z.outside_grid(c.w, cx, cy).reshape(-1, 4).all(1)
    assert out.mean() >= 0.05, f"{c.where}: {out.mean():.3f} of the poses lie outside the grid"
    d = np.sqrt(np.array([oracle.point_mesh_d2(a, b, c.tri) for a, b in zip(c.poses["x"], c.poses["y"])]))
    assert (d > 300.0).sum() >= 3, f"{c.where}: {(d > 300.0).sum()} poses far from the mesh"
    if name == "islands":
        large = c.nx * c.ny > LARGE_GRID_CELLS
        assert large == (cell == 0.25) and bool(c.w.ints["hints"] & _abi.WORLD_LARGE_GRID) == large, f"{c.where}: {c.nx} x {c.ny} cells"
    if name == "speck":
        assert c.nx % 16 and c.ny % 16 and c.nx % 32 and c.ny % 32, f"{c.where}: {c.nx} x {c.ny} cells"     # (always multiples of 8)
        assert np.ptp(c.tri.reshape(-1, 2), 0).max() < 4 * cell
    if name == "fan":
        longest = int(c.cnt[c.cls == MIXED].max())
        assert 65 <= longest <= 255, f"{c.where}: the longest candidate list has {longest} records"
    if name == "far_ribbon":
        assert c.w.has_lights and int(c.m["n_stop"]) == 1 and int(c.m["n_phase"]) == 2


@zoo
def test_lookup_equals_brute_force(name, cell, squared):
    """cell classes, candidate lists and sub-cell classes: the kernels' lookup (grid_offroad_numpy, with and without the sub-cell
    classes) == brute force over every triangle, on the corners of the poses and on points around the mesh's edges; no point is
    left out"""
    c = ctx(name, cell, squared)
    cx, cy = Z.pose_corners(c.w, c.poses)
    ex, ey = Z.edge_points(c.tri, 1500, np.random.default_rng([6, Z.NAMES.index(name)]), spread=0.5 if name != "speck" else 0.3)
    if name == "fan":
        # fan's long lists must MATTER (from the oracle alone): points on the road through records late in a long list only -
        # beyond position 64, beyond 128, the last of 255 - among the pose corners, and among the edge points with the 90 points
        # beyond the long wedges' tips
        wx, wy = Z.fan_witness_points(90, np.random.default_rng(10)).T.astype(np.float32)
        ex, ey = np.concatenate([ex, wx]), np.concatenate([ey, wy])
        for what, (qx, qy) in (("pose corners", (cx, cy)), ("edge points", (ex, ey))):
            n64, n128, n_last = Z.late_record_witnesses(c.w, qx, qy, c.thr2)
            assert n64 >= 40 and n128 >= 15 and n_last >= 5, f"{c.where}, {what}: {n64}, {n128}, {n_last} points hang on records beyond 64, beyond 128, on the 255th"
    px, py = np.concatenate([cx, ex]), np.concatenate([cy, ey])
    want = ~c.brute_near(px, py)
    for use_sub in (False, True):
        got = Z.grid_offroad_numpy(c.w, 0, px, py, c.thr, use_sub=use_sub, thr2=c.thr2)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (f"{c.where}, use_sub={use_sub}: {len(bad)} of {len(want)} points differ from brute force, first at "
                               f"({px[bad[0]]}, {py[bad[0]]})")
    assert 0.1 < want[len(cx):].mean() < 0.9, f"{c.where}: {want[len(cx):].mean():.3f} of the edge points are off the road"


@zoo
def test_class_map_decodes_to_the_cell_classes(name, cell, squared):
    """cell_cls2 with the rasteriser's addressing (tde_abi.h): tile (ix >> 5, iy >> 4) at (ty << (row_shift - 5)) + tx, 32 words a
    tile, word 2 * (iy & 15) + ((ix >> 4) & 1), cell ix at bits 2 * (ix & 15) - exactly the class of every cell, EMPTY in the padding"""
    c = ctx(name, cell, squared)
    pitch, rows = 1 << c.rs, -(-c.ny // 16) * 16
    iy, ix = np.meshgrid(np.arange(rows), np.arange(pitch), indexing="ij")
    tile = ((iy >> 4) << (c.rs - 5)) + (ix >> 5)
    word = c.w.arrays["cell_cls2"][tile * 32 + 2 * (iy & 15) + ((ix >> 4) & 1)]
    got = ((word >> (2 * (ix & 15)).astype(np.uint32)) & 3).astype(np.int64)
    want = np.full((rows, pitch), EMPTY, np.int64)
    want[:c.ny, :c.nx] = c.cls
    n_bad = int((got != want).sum())
    assert n_bad == 0, f"{c.where}: {n_bad} of {want.size} cells decode to another class"
    assert len(c.w.arrays["cell_cls2"]) == (rows // 16) * (pitch // 32) * 32


@zoo
def test_cell_word_clearances(name, cell, squared):
    """a FULL / EMPTY cell with clearance k: every cell whose rectangle comes within k * TDE_CLEARANCE_UNIT of it has its class
    (exact, over the rectangles), and brute force agrees at random points within that distance of a sample of such cells - within
    the threshold around FULL cells, beyond it around EMPTY cells.  And the field is not idle: the specification rounds down, the
    builder keeps 1 mm back, so k is at most one unit short of the distance to the nearest cell of another class, 255 where that
    distance is beyond the cap."""
    c = ctx(name, cell, squared)
    per = int(round((cell / CLEARANCE_UNIT) ** 2))                         # (k UNIT)^2 < D2 cell^2  <=>  k^2 < D2 (cell / UNIT)^2
    assert per == (cell / CLEARANCE_UNIT) ** 2
    rng = np.random.default_rng([7, Z.NAMES.index(name)])
    for cls_of in (EMPTY, FULL):
        sel = c.cls == cls_of
        k, d2 = c.cnt[sel], c.D2[cls_of][sel]
        bad = int(((k > 0) & (k * k >= d2 * per)).sum())                  # (a clearance of 0 promises nothing)
        assert bad == 0, f"{c.where}: {bad} of {sel.sum()} class-{cls_of} cells claim a clearance that reaches a cell of another class"
        reach = np.floor(np.sqrt(d2.astype(np.float64)) * (cell / CLEARANCE_UNIT))
        idle = int((k < np.minimum(reach - 1, 255)).sum())
        assert idle == 0, f"{c.where}: {idle} of {sel.sum()} class-{cls_of} cells carry less than their clearance less one unit"
        iy, ix = sample_uniform_cells(c.cls, c.cnt, cls_of, rng, 120)
        if name != "speck" or cls_of == EMPTY:                               # (every FULL cell of speck touches a MIXED one)
            assert len(iy) > 0, f"{c.where}: no class-{cls_of} cell with a clearance"
        for y, x in zip(iy, ix):
            px, py = points_within(rng, float(c.m["ox"]) + x * cell, float(c.m["oy"]) + y * cell, cell, cell, c.cnt[y, x] * CLEARANCE_UNIT, 6)
            near = c.brute_near(px, py)
            assert (near == (cls_of == FULL)).all(), (f"{c.where}: {int((near != (cls_of == FULL)).sum())} of 6 points within {c.cnt[y, x]} units of "
                                                      f"class-{cls_of} cell ({x}, {y}) are on the other side of the threshold")
    assert (c.cnt[c.cls == MIXED] > 0).all()                                # (a MIXED cell's field is the length of its list)


def coarse_bytes(c):
    """the bytes of cell_coarse of every coarse tile of the pitch, [rows of tiles, tiles of the pitch], with tde_abi.h's addressing"""
    tx, ty = (1 << c.rs) // 4, -(-c.ny // 32) * 8
    cy, cx = np.meshgrid(np.arange(ty), np.arange(tx), indexing="ij")
    at = ((((cy >> 3) << (c.rs - 6)) + (cx >> 4)) << 7) + ((cy & 7) << 4) + (cx & 15)
    assert len(c.w.arrays["cell_coarse"]) == tx * ty
    return c.w.arrays["cell_coarse"][at].astype(np.int64)


@zoo
def test_coarse_tiles(name, cell, squared):
    """cell_coarse: the byte is tde_abi.h's - the class of the tile's 16 cells when they agree and are not MIXED, with the smallest of
    their clearances converted to TDE_COARSE_UNITs, rounded down and capped at 63; MIXED / 0 otherwise; EMPTY / 0 in the padding - and
    the clearance keeps its promise: every cell whose rectangle comes within it of the tile has the tile's class (exact), brute
    force agrees at random points that close to a sample of tiles"""
    c = ctx(name, cell, squared)
    got = coarse_bytes(c)
    ty, tx = c.ny // 4, c.nx // 4
    blk = lambda a: a.reshape(ty, 4, tx, 4).transpose(0, 2, 1, 3).reshape(ty, tx, 16)     # noqa: E731
    cl, k = blk(c.cls), blk(c.cnt)
    uni = (cl.min(2) == cl.max(2)) & (cl[:, :, 0] != MIXED)
    q = np.minimum(np.floor(k.min(2) * (CLEARANCE_UNIT / COARSE_UNIT)).astype(np.int64), 63)
    want = np.zeros_like(got)
    want[:ty, :tx] = np.where(uni, cl[:, :, 0] | (q << 2), MIXED)
    n_bad = int((got != want).sum())
    assert n_bad == 0, f"{c.where}: {n_bad} of {want.size} coarse bytes differ from the specification"
    tcls, tq = got[:ty, :tx] & 3, got[:ty, :tx] >> 2
    assert (tq[tcls == MIXED] == 0).all(), f"{c.where}: a MIXED tile carries a clearance"
    assert all((tcls == v).any() for v in (EMPTY, MIXED) + ((FULL,) if name != "speck" else ())), f"{c.where}: tile classes {np.bincount(tcls.ravel(), minlength=3)}"
    per = int(round((cell / COARSE_UNIT) ** 2))                             # (q UNIT)^2 < D2 cell^2  <=>  q^2 < D2 (cell / UNIT)^2
    assert per == (cell / COARSE_UNIT) ** 2
    rng = np.random.default_rng([8, Z.NAMES.index(name)])
    for cls_of in (EMPTY, FULL):
        d2 = blk(c.D2[cls_of]).min(2)                                       # (the distance of a union is the smallest of its parts')
        sel = tcls == cls_of
        bad = int(((tq[sel] > 0) & (tq[sel] ** 2 >= d2[sel] * per)).sum())
        assert bad == 0, f"{c.where}: {bad} of {sel.sum()} class-{cls_of} tiles claim a clearance that reaches a cell of another class"
        # (not idle either: each cell word is at most one of its units short, halving rounds down: at most one coarse unit short)
        reach = np.floor(np.sqrt(d2[sel].astype(np.float64)) * (cell / COARSE_UNIT))
        idle = int((tq[sel] < np.minimum(reach - 1, 63)).sum())
        assert idle == 0, f"{c.where}: {idle} of {sel.sum()} class-{cls_of} tiles carry less than their clearance less one unit"
        iy, ix = sample_uniform_cells(tcls, tq, cls_of, rng, 60)
        if name != "speck" or cls_of == EMPTY:                               # (speck's road is narrower than a tile)
            assert len(iy) > 0, f"{c.where}: no class-{cls_of} tile with a clearance"
        for y, x in zip(iy, ix):
            px, py = points_within(rng, float(c.m["ox"]) + 4 * x * cell, float(c.m["oy"]) + 4 * y * cell, 4 * cell, 4 * cell,
                                   tq[y, x] * COARSE_UNIT, 6)
            near = c.brute_near(px, py)
            assert (near == (cls_of == FULL)).all(), (f"{c.where}: {int((near != (cls_of == FULL)).sum())} of 6 points within {tq[y, x]} units of "
                                                      f"class-{cls_of} tile ({x}, {y}) are on the other side of the threshold")


@pytest.mark.parametrize("cell", Z.CELLS)
def test_islands_saturate_both_clearance_fields(cell):
    """between and inside the two discs of `islands` the clearances sit at their caps - 255 units in the cell words, 63 in the coarse
    bytes, for both classes - and the promise still holds around exactly those cells and tiles: brute force at random points within
    the capped distance"""
    c = ctx("islands", cell, False)
    tq_all = coarse_bytes(c)[:c.ny // 4, :c.nx // 4]
    rng = np.random.default_rng(9)
    for cls_of in (EMPTY, FULL):
        for field, cls, cap, unit, size in ((c.cnt, c.cls, 255, CLEARANCE_UNIT, cell), (tq_all >> 2, tq_all & 3, 63, COARSE_UNIT, 4 * cell)):
            iy, ix = np.nonzero((cls == cls_of) & (field == cap))
            assert len(iy) > 0, f"{c.where}: no class-{cls_of} entry at the cap of {cap}"
            assert (field[cls != MIXED] <= cap).all()
            for j in rng.choice(len(iy), size=min(80, len(iy)), replace=False):
                px, py = points_within(rng, float(c.m["ox"]) + ix[j] * size, float(c.m["oy"]) + iy[j] * size, size, size, cap * unit, 6)
                near = c.brute_near(px, py)
                assert (near == (cls_of == FULL)).all(), (f"{c.where}: {int((near != (cls_of == FULL)).sum())} of 6 points within the capped clearance of "
                                                          f"class-{cls_of} entry ({ix[j]}, {iy[j]}) are on the other side of the threshold")


@pytest.mark.parametrize("cell", Z.CELLS)
def test_fan_valence_at_and_past_the_builders_limit(cell):
    """the zoo's fan fills the 8-bit count of a cell word to the last record (255; test_lookup_equals_brute_force holds points that
    hang on that record alone); one more triangle at the same vertex and the builder refuses the mesh by name of the limit"""
    c = ctx("fan", cell, False)
    assert int(c.cnt[c.cls == MIXED].max()) == 255
    with pytest.raises(_lib.TdeError, match="more than 255 candidate triangles"):
        build_grid_index(Z.fan(Z.FAN_VALENCE + 1).astype(np.float32), threshold=0.5, cell=cell)
