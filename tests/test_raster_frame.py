"""The raster frame (RasterFrame in csrc/o3dr_device.h, DESIGN.md "Raster frame"): the map raster's winner pass, the ground
filter's point pass and the raster sample decide "which cell of the box" with one device function.  These tests hold the
three passes to one another, and to numpy's fp32 floor(x * inv) with inv = float32(1) / float32(cell_size), through the
public Python API.  The winner and the ground point pass have their launch-shape tests in test_map_operators_scale.py; the
sample pass has them here."""
import numpy as np
import pytest

import interpolate_reference as R
from test_rasterize_map import _pts

F32 = np.float32
CELL = 0.5
BOX = (-3, -2, 5, 4)    # (cx0, cy0, width, height): straddles the origin
POINT_CAP = 262144      # kCellRangeBlocks * 256 (o3dr_device.h): point POINT_CAP is the first a workgroup reaches by stride


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.ascontiguousarray(a, F32).view(np.uint32)


def host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def inside_of(xyz, box):
    """numpy's verdict: the boolean mask of the points inside the box and their dense cell ids dy * width + dx"""
    inv = F32(1) / F32(CELL)
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    cx, cy = np.floor(xyz[:, 0] * inv).astype(np.int64), np.floor(xyz[:, 1] * inv).astype(np.int64)
    dx, dy = cx - box[0], cy - box[1]
    inside = (dx >= 0) & (dx < box[2]) & (dy >= 0) & (dy < box[3])
    return inside, dy * box[2] + dx


def in_memory(device, pts, raster):
    if not device:
        return pts, raster
    import torch
    return torch.from_numpy(pts.view(np.int32).reshape(-1, 4).copy()).cuda(), torch.from_numpy(raster).cuda()


def three_passes(ctx, xyz, box, device=False):
    """-> ((n_inside, n_outside) of the raster, of the ground filter, of the sample; the source image; the sampled values)"""
    zeros = np.zeros((box[3], box[2]), F32)
    pts, raster = in_memory(device, _pts(xyz), zeros)
    *_, source, rinfo = ctx.rasterizeMap(pts, CELL, bounds=box, return_source=True, return_info=True)
    _, ginfo = ctx.groundFilter(pts, CELL, bounds=box, return_info=True)
    _, value, counts = ctx.sampleRaster(pts, raster, CELL, box, return_value=True, return_info=True)
    assert (rinfo.cx0, rinfo.cy0, rinfo.width, rinfo.height) == box == (ginfo.cx0, ginfo.cy0, ginfo.width, ginfo.height)
    return ((rinfo.n_inside, rinfo.n_outside), (ginfo.n_inside, ginfo.n_outside), counts[:2]), host(source), host(value)


def assert_agreement(ctx, xyz, box, device, n_inside):
    inside, dense = inside_of(xyz, box)
    assert int(inside.sum()) == n_inside  # (the case is the one that was meant)
    verdicts, source, value = three_passes(ctx, xyz, box, device)
    for who, v in zip(("rasterizeMap", "groundFilter", "sampleRaster"), verdicts):
        assert tuple(v) == (n_inside, len(xyz) - n_inside), (who, v)
    # one point per cell: the source image holds exactly the inside set, every point at its own dense id
    assert source.shape == (box[3], box[2]) and source.dtype == np.int32
    assert set(source[source >= 0].tolist()) == set(np.flatnonzero(inside).tolist())
    assert np.array_equal(source.ravel()[dense[inside]], np.flatnonzero(inside))
    assert value.shape == (len(xyz),) and np.array_equal(~np.isnan(value), inside)


@pytest.fixture(scope="module")
def fctx():
    import online_3d_reconstruction_amd as o3dr
    with o3dr.Context(0) as c:
        yield c


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_one_box_three_passes_same_verdict(fctx, device):
    cx, cy = np.meshgrid(np.arange(-5, 4), np.arange(-4, 4))  # the 9 x 8 block of cells around the 5 x 4 box
    xyz = np.column_stack([(cx.ravel() + 0.5) * CELL, (cy.ravel() + 0.5) * CELL, np.linspace(-1.0, 1.0, cx.size)]).astype(F32)
    xyz = xyz[np.random.default_rng(1).permutation(len(xyz))]
    assert len(xyz) == 72
    assert_agreement(fctx, xyz, BOX, device, n_inside=20)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_points_on_cell_borders(fctx, device):
    """x = k * 0.5 and y = m * 0.5 exactly, and inv = 2 is exact: floor puts every point on the upper cell, so k = cx0 is the
    box's first column and k = cx0 + width the first outside it"""
    cx0, cy0, W, H = BOX
    k, m = np.meshgrid(np.arange(cx0 - 1, cx0 + W + 2), np.arange(cy0 - 1, cy0 + H + 2))
    xyz = np.column_stack([k.ravel() * CELL, m.ravel() * CELL, np.linspace(2.0, -2.0, k.size)]).astype(F32)
    xyz = xyz[np.random.default_rng(2).permutation(len(xyz))]
    inside, dense = inside_of(xyz, BOX)
    on = lambda kk, mm: inside[(xyz[:, 0] == F32(kk * CELL)) & (xyz[:, 1] == F32(mm * CELL))].tolist()
    assert on(cx0, cy0) == [True] and on(cx0 + W, cy0) == [False] and on(cx0, cy0 + H) == [False] and on(cx0 - 1, cy0) == [False]
    corner = (xyz[:, 0] == F32((cx0 + W - 1) * CELL)) & (xyz[:, 1] == F32((cy0 + H - 1) * CELL))
    assert dense[corner].tolist() == [W * H - 1]  # the last dense id
    assert_agreement(fctx, xyz, BOX, device, n_inside=W * H)


_SAMPLE = {}


def sample_case():
    """POINT_CAP + 1 points around a 64 x 64 box, a raster of distinct values with a few holes: made once, never written to"""
    if not _SAMPLE:
        rng = np.random.default_rng(3)
        box = (-20, -30, 64, 64)
        raster = (np.arange(64 * 64, dtype=F32).reshape(64, 64) * F32(0.25) - F32(100.0)).astype(F32)
        raster.ravel()[rng.choice(64 * 64, 16, replace=False)] = np.nan
        lo, hi = np.array([box[0] - 4, box[1] - 4, -10]) * CELL, np.array([box[0] + 68, box[1] + 68, 10]) * CELL
        xyz = rng.uniform(lo, hi, (POINT_CAP + 1, 3)).astype(F32)
        xyz[[0, 255, 256, POINT_CAP], :2] = (box[0] + 10.5) * CELL, (box[1] + 20.5) * CELL  # the last point of every n: on a value
        raster[20, 10] = F32(7.125)
        pts = _pts(xyz)
        for a in (xyz, raster, pts):
            a.setflags(write=False)
        _SAMPLE.update(box=box, raster=raster, xyz=xyz, pts=pts)
    return _SAMPLE


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 256, 257, POINT_CAP + 1])
def test_launch_shapes_of_the_sample_pass(fctx, n):
    s = sample_case()
    rv, ra, rc = R.sample(s["xyz"][:n], s["raster"], CELL, s["box"])
    assert rv[n - 1] == F32(7.125) and (n < 257 or 0 < rc[1] < n)  # the last point is inside; there are points outside
    above, value, counts = fctx.sampleRaster(s["pts"][:n], s["raster"], CELL, s["box"], return_value=True, return_info=True)
    assert value.dtype == F32 and above.dtype == F32 and value.shape == above.shape == (n,)
    assert np.array_equal(bits(value), bits(rv)), int((bits(value) != bits(rv)).sum())
    assert np.array_equal(bits(above), bits(ra)), int((bits(above) != bits(ra)).sum())
    assert counts == rc


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["1x1", "n=0"])
def test_a_degenerate_frame(fctx, case):
    if case == "1x1":  # three points in the one cell, one of them on its lower corner, and four around it
        box = (-1, 2, 1, 1)
        xy = [(-0.25, 1.25), (-0.5, 1.0), (-0.01, 1.49), (0.0, 1.25), (-0.25, 1.5), (-0.51, 1.25), (-0.25, 0.99)]
        xyz = np.array([(x, y, 0.1 * i) for i, (x, y) in enumerate(xy)], F32)
        n_inside = 3
    else:
        box, xyz, n_inside = BOX, np.zeros((0, 3), F32), 0
    n, (cx0, cy0, W, H) = len(xyz), box
    inside, _ = inside_of(xyz, box)
    assert int(inside.sum()) == n_inside
    pts = _pts(xyz)
    hm, color, source, rinfo = fctx.rasterizeMap(pts, CELL, bounds=box, return_source=True, return_info=True)
    ground, hag, dtm, state, ginfo = fctx.groundFilter(pts, CELL, bounds=box, return_height=True, return_dtm=True, return_state=True,
                                                       return_info=True)
    above, value, counts = fctx.sampleRaster(pts, np.zeros((H, W), F32), CELL, box, return_value=True, return_info=True)
    for who, (n_in, n_out) in (("rasterizeMap", (rinfo.n_inside, rinfo.n_outside)), ("groundFilter", (ginfo.n_inside, ginfo.n_outside)),
                               ("sampleRaster", counts[:2])):
        assert (n_in, n_out) == (n_inside, n - n_inside), (who, n_in, n_out)
    assert hm.shape == source.shape == dtm.shape == state.shape == (H, W) and color.shape == (H, W, 3)
    assert ground.shape == hag.shape == above.shape == value.shape == (n,)
    assert (hm.dtype, color.dtype, source.dtype, dtm.dtype, state.dtype) == (F32, np.uint8, np.int32, F32, np.uint8)
    assert (ground.dtype, hag.dtype, above.dtype, value.dtype) == (np.uint8, F32, F32, F32)
    assert np.array_equal(~np.isnan(value), inside)
    if n:
        assert source[0, 0] == int(np.flatnonzero(inside)[0])  # select "first": the lowest input index of the cell
