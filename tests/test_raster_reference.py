"""The numpy restatement of the map raster's contract (raster_reference.py) against figures that do not come from it:
the bundled reference cloud's cell statistics and scipy's Euclidean distance transform, hand-made rasters for the tie
rule and the select modes, and the shade formula evaluated by hand on a tilted plane.  No GPU."""
import os

import numpy as np
import pytest

import raster_reference as rr
from conftest import GOLDEN

F32 = np.float32


def golden_cloud():
    v = np.load(os.path.join(GOLDEN, "cloud_ply.npz"))["vertices"]
    xyz = np.stack([v["x"], v["y"], v["z"]], 1).astype(F32)
    rgba = (np.uint32(255) << 24) | (v["r"].astype(np.uint32) << 16) | (v["g"].astype(np.uint32) << 8) | v["b"].astype(np.uint32)
    return xyz, rgba


def cells_to_xyz(cells, z=None, cell=1.0):
    """one point in the middle of every (cx, cy) cell"""
    c = np.asarray(cells, np.float64).reshape(-1, 2)
    zz = np.zeros(len(c)) if z is None else np.asarray(z, np.float64)
    return np.column_stack([(c[:, 0] + 0.5) * cell, (c[:, 1] + 0.5) * cell, zz]).astype(F32)


@pytest.fixture(scope="module")
def golden():
    return golden_cloud()


def test_reference_cloud_is_a_355_by_376_raster_of_55940_cells(golden):
    xyz, rgba = golden
    assert rr.extent(xyz, 0.05)[2:] == (355, 376)
    o = rr.rasterize(xyz, rgba, 0.05)
    i = o.info
    assert (i["width"], i["height"], i["n_inside"], i["n_outside"]) == (355, 376, 55940, 0)
    assert (i["n_occupied"], i["n_shadowed"], i["n_filled"], i["n_empty"]) == (55940, 0, 0, 355 * 376 - 55940)
    assert i["z_min"] == float(xyz[:, 2].min()) and i["z_max"] == float(xyz[:, 2].max())
    assert o.height_map.shape == (376, 355) and o.color.shape == (376, 355, 3) and o.shade is None
    # every point sits in its own cell, with its own height and colour
    cx, cy = rr.cells_of(xyz, 0.05)
    r, c = cy - i["cy0"], cx - i["cx0"]
    assert np.array_equal(o.source[r, c], np.arange(len(xyz))) and (o.distance2[r, c] == 0).all()
    assert np.array_equal(o.height_map[r, c].view(np.uint32), xyz[:, 2].view(np.uint32))
    assert np.array_equal(o.color[r, c, 0], rgba & 255) and np.array_equal(o.color[r, c, 2], (rgba >> 16) & 255)
    assert np.isnan(o.height_map[o.source < 0]).all() and not o.color[o.source < 0].any() and (o.distance2[o.source < 0] == -1).all()


@pytest.mark.parametrize("R,n_filled", [(1, 1259), (2, 2309), (3, 3644), (4, 4637), (8, 9179)])
def test_reference_cloud_fill_counts_and_distances(golden, R, n_filled):
    """the counts were computed with scipy.ndimage.distance_transform_edt; where scipy is installed the squared distances
    are compared too"""
    xyz, rgba = golden
    o = rr.rasterize(xyz, rgba, 0.05, fill_radius=R)
    assert o.info["n_filled"] == n_filled and o.info["n_empty"] == 355 * 376 - 55940 - n_filled
    filled = o.distance2 > 0
    assert filled.sum() == n_filled and (o.distance2[filled] <= R * R).all()
    # a filled cell shows an occupied cell's point, and that cell is as far as distance2 says
    own = rr.rasterize(xyz, rgba, 0.05).source
    rr_, cc = np.nonzero(filled)
    cx, cy = rr.cells_of(xyz, 0.05)
    sr, sc = cy[o.source[filled]] - o.info["cy0"], cx[o.source[filled]] - o.info["cx0"]
    assert np.array_equal(own[sr, sc], o.source[filled])
    assert np.array_equal((sr - rr_) ** 2 + (sc - cc) ** 2, o.distance2[filled])
    try:
        from scipy import ndimage
    except ImportError:  # the counts above came from it; without it only the distances go unchecked
        return
    d = ndimage.distance_transform_edt(own < 0)
    d2 = np.rint(d * d).astype(np.int64)
    assert np.array_equal(np.where(d2 <= R * R, d2, -1), o.distance2)


def test_tie_rule_on_a_7_by_7_raster():
    """sources at equal distance to the left, right, above and below the centre: the lowest (cy, cx) wins"""
    box = (0, 0, 7, 7)
    rgba = np.arange(4, dtype=np.uint32)
    # index: 0 right (5, 3), 1 above (3, 5), 2 left (1, 3), 3 below (3, 1)
    xyz = cells_to_xyz([(5, 3), (3, 5), (1, 3), (3, 1)], z=[10, 11, 12, 13])
    o = rr.rasterize(xyz, rgba, 1.0, bounds=box, fill_radius=2)
    assert o.source[3, 3] == 3 and o.distance2[3, 3] == 4 and o.height_map[3, 3] == 13  # below: the lowest cy
    o = rr.rasterize(xyz[:3], rgba[:3], 1.0, bounds=box, fill_radius=2)
    assert o.source[3, 3] == 2 and o.height_map[3, 3] == 12  # left and right share cy: the lowest cx
    o = rr.rasterize(xyz[:2], rgba[:2], 1.0, bounds=box, fill_radius=2)
    assert o.source[3, 3] == 0  # right (cy 3) before above (cy 5)
    # a nearer source beats every tie rule; one beyond R is no source
    near = np.concatenate([xyz, cells_to_xyz([(4, 4)], z=[20])])
    o = rr.rasterize(near, np.arange(5, dtype=np.uint32), 1.0, bounds=box, fill_radius=2)
    assert o.source[3, 3] == 4 and o.distance2[3, 3] == 2
    o = rr.rasterize(xyz, rgba, 1.0, bounds=box, fill_radius=1)
    assert o.source[3, 3] == -1 and o.distance2[3, 3] == -1 and np.isnan(o.height_map[3, 3])
    assert o.source[3, 4] == 0 and o.distance2[3, 4] == 1
    # a fill never feeds a fill: (0, 0) is 2 * sqrt(2) from the source, although its filled neighbour (1, 1) is next to it
    one = cells_to_xyz([(2, 2)])
    o = rr.rasterize(one, rgba[:1], 1.0, bounds=box, fill_radius=2)
    assert o.source[1, 1] == 0 and o.distance2[1, 1] == 2 and o.source[0, 0] == -1
    assert o.info["n_filled"] == 12 and o.info["n_empty"] == 49 - 13  # the disc of radius 2 holds 13 cells
    diag = rr.rasterize(cells_to_xyz([(2, 2), (4, 4)]), rgba[:2], 1.0, bounds=box, fill_radius=2)
    assert diag.source[3, 3] == 0 and diag.source[2, 4] == 0 and diag.source[4, 2] == 0  # ties at d2 = 2 and 4: the lower cy


@pytest.mark.parametrize("select,want", [("first", 0), ("top", 2), ("bottom", 1)])
def test_select_modes_in_one_cell(select, want):
    # index:            0     1     2     3     4
    z = np.array([0.5, -1.0, 2.0, 2.0, -1.0], F32)
    xyz = np.column_stack([np.full(5, 0.5), np.full(5, 0.5), z]).astype(F32)
    o = rr.rasterize(xyz, np.arange(5, dtype=np.uint32) + 7, 1.0, select=select)
    assert o.source.tolist() == [[want]] and o.height_map[0, 0] == z[want] and o.color[0, 0, 0] == want + 7
    assert o.info["n_occupied"] == 1 and o.info["n_shadowed"] == 4 and o.info["z_min"] == z[want] == o.info["z_max"]


@pytest.mark.parametrize("select", ["first", "top", "bottom"])
def test_the_two_zeros_are_equal(select):
    for z in ([-0.0, 0.0], [0.0, -0.0]):
        xyz = np.column_stack([[0.5, 0.5], [0.5, 0.5], z]).astype(F32)
        o = rr.rasterize(xyz, np.zeros(2, np.uint32), 1.0, select=select)
        assert o.source[0, 0] == 0  # a tie in every mode: the lowest index
        assert np.signbit(o.height_map[0, 0]) == np.signbit(F32(z[0]))  # the height is a copy of that point's z
        assert o.info["z_min"] == 0.0 and not np.signbit(o.info["z_min"]) and not np.signbit(o.info["z_max"])
    # with other values around them: -0.0 is not below 0.0 for BOTTOM, nor 0.0 above -0.0 for TOP
    xyz = np.column_stack([np.full(4, 0.5), np.full(4, 0.5), [1.0, 0.0, -0.0, -1.0]]).astype(F32)
    o = rr.rasterize(xyz[:3], np.zeros(3, np.uint32), 1.0, select="bottom")
    assert o.source[0, 0] == 1
    o = rr.rasterize(xyz[1:][::-1], np.zeros(3, np.uint32), 1.0, select="top")  # -1, -0, 0
    assert o.source[0, 0] == 1


def shade_by_hand(gx, gy, light):
    lx, ly, lz = (np.float64(v) for v in light)
    ln = np.sqrt((lx * lx + ly * ly) + lz * lz)
    s = (((-gx) * (lx / ln) + (-gy) * (ly / ln)) + lz / ln) / np.sqrt((gx * gx + gy * gy) + 1.0)
    return 1 if not s > 0 else min(255, 1 + int(np.floor(s * 254.0 + 0.5)))


def test_shade_of_a_tilted_plane():
    """z = 0.25 cx + 0.5 cy on a 9 x 6 raster of 0.5 m cells (every height and difference exact in fp32): the interior has
    one value, the contract's formula by hand; a border cell's one-sided difference has the same slope"""
    W, H, cell = 9, 6, 0.5
    gx_, gy_ = np.meshgrid(np.arange(W), np.arange(H))
    cells = np.column_stack([gx_.ravel(), gy_.ravel()])
    z = 0.25 * cells[:, 0] + 0.5 * cells[:, 1]
    xyz = cells_to_xyz(cells, z, cell)
    light = (-1.0, 1.0, 1.0)
    o = rr.rasterize(xyz, np.zeros(len(xyz), np.uint32), cell, light=light)
    want = shade_by_hand(np.float64(0.5) / (2 * cell), np.float64(1.0) / (2 * cell), light)
    assert 1 < want < 255 and (o.shade == want).all()  # the borders divide one difference by one cell: the same slope
    # hand-made borders: a single row has gy = 0, a single cell is flat
    row = rr.rasterize(xyz[:W], np.zeros(W, np.uint32), cell, light=light)
    assert (row.shade == shade_by_hand(np.float64(0.5), 0.0, light)).all()
    one = rr.rasterize(xyz[:1], np.zeros(1, np.uint32), cell, light=light)
    assert one.shade.tolist() == [[shade_by_hand(0.0, 0.0, light)]]
    # a hole: its neighbours fall back to one-sided differences, the hole itself is 0
    keep = np.ones(len(xyz), bool)
    keep[2 * W + 4] = False
    holed = rr.rasterize(xyz[keep], np.zeros(keep.sum(), np.uint32), cell, bounds=(0, 0, W, H), light=light)
    assert holed.shade[2, 4] == 0 and holed.info["n_empty"] == 1
    assert (np.delete(holed.shade.ravel(), 2 * W + 4) == want).all()
    # a surface facing away from the light is 1, straight at it 255
    away = rr.rasterize(xyz, np.zeros(len(xyz), np.uint32), cell, light=(1.0, 2.0, 0.1))
    assert (away.shade == 1).all()
    flat = rr.rasterize(cells_to_xyz(cells, None, cell), np.zeros(len(xyz), np.uint32), cell, light=(0.0, 0.0, 3.0))
    assert (flat.shade == 255).all()


def test_bounds_and_counts():
    rng = np.random.default_rng(5)
    xyz = np.column_stack([rng.uniform(-3, 3, 500), rng.uniform(-2, 2, 500), rng.normal(0, 1, 500)]).astype(F32)
    rgba = rng.integers(0, 1 << 24, 500, dtype=np.uint32)
    full = rr.rasterize(xyz, rgba, 0.25, fill_radius=2)
    assert full.info["n_outside"] == 0 and full.info["n_shadowed"] > 0
    part = rr.rasterize(xyz, rgba, 0.25, bounds=(-4, -3, 9, 7), fill_radius=2)
    i = part.info
    assert i["n_outside"] > 0 and i["n_inside"] + i["n_outside"] == 500 and i["n_occupied"] + i["n_shadowed"] == i["n_inside"]
    assert i["n_occupied"] + i["n_filled"] + i["n_empty"] == 63
    # inside the smaller box the own cells are the same; the fill may only lose sources that lie outside it
    r0, c0 = -3 - full.info["cy0"], -4 - full.info["cx0"]
    sub = full.distance2[r0:r0 + 7, c0:c0 + 9] == 0
    assert np.array_equal(sub, part.distance2 == 0) and np.array_equal(full.source[r0:r0 + 7, c0:c0 + 9][sub], part.source[sub])
    none = rr.rasterize(xyz, rgba, 0.25, bounds=(100, 100, 3, 2), fill_radius=4, light=(0, 0, 1))
    assert none.info["n_inside"] == 0 and none.info["n_empty"] == 6 and np.isnan(none.info["z_min"]) and not none.shade.any()
    empty = rr.rasterize(np.zeros((0, 3), F32), np.zeros(0, np.uint32), 0.25, bounds=(0, 0, 4, 3), fill_radius=1)
    assert empty.info["n_empty"] == 12 and np.isnan(empty.height_map).all() and (empty.source == -1).all()


def test_height_png16_quantisation():
    h = np.array([[np.nan, 1.0, 1.5], [3.0, 2.0, np.nan]], F32)
    q, step = rr.height_png16(h, 1.0, 3.0)
    assert step == 2.0 / 65534.0 and q.dtype == np.uint16
    assert q[0, 0] == 0 and q[1, 2] == 0 and q[0, 1] == 1 and q[1, 0] == 65535 and q[1, 1] in (32767, 32768, 32769)
    q, step = rr.height_png16(np.full((2, 2), 7.0, F32), 7.0, 7.0)  # a flat map: the smallest step, every cell 1
    assert step == 2.0 ** -15 and (q == 1).all()
