"""Map raster on the GPU (o3dr_raster_extent, o3dr_rasterize_map, Context.rasterExtent / rasterizeMap): every output image
and every counter bit for bit against the numpy restatement of the contract (raster_reference.py), on rasters small
enough for a few seconds in total but past one tile of the row pass (64 x 4 cells) in both directions."""
import ctypes as C

import numpy as np
import pytest

import raster_reference as rr
from test_raster_reference import cells_to_xyz, golden_cloud

ERR_INVALID_ARG = -1
F32 = np.float32
LIGHT = (-1.0, 1.0, 1.0)


def _pts(xyz, rgba=None):
    from online_3d_reconstruction_amd import POINT
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    p = np.zeros(len(xyz), POINT)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["rgba"] = np.arange(len(xyz), dtype=np.uint32) * np.uint32(2654435761) if rgba is None else rgba
    return p


def grid_cloud(w, h, cell=0.05, holes=0.0, seed=0, x0=0, y0=0, extra=0):
    """one jittered point per cell of a w x h grid from cell (x0, y0), a fraction `holes` left empty, `extra` more points
    in random cells of the grid, shuffled"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(w) + x0, np.arange(h) + y0)
    cells = np.column_stack([gx.ravel(), gy.ravel()])[rng.random(w * h) >= holes]
    if extra:
        cells = np.concatenate([cells, cells[rng.integers(0, len(cells), extra)]])
    u = rng.uniform(0.05, 0.95, (len(cells), 2))
    xy = (cells + u) * cell
    z = 0.3 * np.sin(xy[:, 0] * 3.0) * np.cos(xy[:, 1] * 2.0) + rng.normal(0, 0.01, len(xy))
    xyz = np.column_stack([xy, z]).astype(F32)
    return xyz[rng.permutation(len(xyz))]


def assert_same(got, ref, what=""):
    """got: rasterizeMap's tuple with every output asked for; ref: raster_reference.rasterize's namespace"""
    names = ["height_map", "color"] + (["shade"] if ref.shade is not None else []) + ["source", "distance2"]
    assert len(got) == len(names) + 1, what
    for name, g in zip(names, got):
        r = getattr(ref, name)
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.dtype == r.dtype and g.shape == r.shape, (what, name, g.dtype, g.shape, r.shape)
        same = np.array_equal(g.view(np.uint32), r.view(np.uint32)) if name == "height_map" else np.array_equal(g, r)
        assert same, (what, name, int((g != r).sum()) if name != "height_map" else int((g.view(np.uint32) != r.view(np.uint32)).sum()))
    info = dict(got[-1].__dict__)
    for k in ("z_min", "z_max"):
        a, b = F32(info.pop(k)), F32(ref.info[k])
        assert a.view(np.uint32) == b.view(np.uint32) or (np.isnan(a) and np.isnan(b)), (what, k, a, b)
    assert info == {k: v for k, v in ref.info.items() if k not in ("z_min", "z_max")}, (what, info, ref.info)


def check(ctx, xyz, cell, rgba=None, what="", **kw):
    p = _pts(xyz, rgba)
    ref = rr.rasterize(xyz, p["rgba"], cell, **kw)
    got = ctx.rasterizeMap(p, cell, return_source=True, return_distance=True, return_info=True, **kw)
    assert_same(got, ref, what or str(kw))
    return got, ref


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments_without_a_gpu():
    from online_3d_reconstruction_amd import _lib
    L = _lib.load_library()
    prm = _lib.RasterParamsStruct()
    prm.cell_size, prm.fill_radius, prm.use_light = 9.0, 9, 9
    L.o3dr_raster_default_params(C.byref(prm))
    assert (prm.cell_size, prm.select, prm.fill_radius, prm.width, prm.height, prm.use_light) == (0.0, 0, 0, 0, 0, 0)
    assert list(prm.light) == [-1.0, 1.0, 1.0] and C.sizeof(prm) == 64 and C.sizeof(_lib.RasterResultStruct) == 72
    p = _pts(cells_to_xyz([(0, 0), (1, 1)]))
    box = [C.c_int32(7) for _ in range(4)]
    rc = L.o3dr_raster_extent(None, p.ctypes.data, 2, 1.0, *[C.byref(b) for b in box], 0)
    assert rc == ERR_INVALID_ARG and [b.value for b in box] == [0, 0, 0, 0] and b"ctx" in L.o3dr_last_error()
    prm.cell_size, prm.width, prm.height = 1.0, 2, 2
    h = np.full((2, 2), 5, F32)
    col = np.full((2, 2, 3), 5, np.uint8)
    outs = _lib.RasterOutputsStruct(h.ctypes.data, col.ctypes.data, None, None, None)
    res = _lib.RasterResultStruct()
    res.n_inside = 3
    rc = L.o3dr_rasterize_map(None, p.ctypes.data, 2, C.byref(prm), C.byref(outs), C.byref(res), 0)
    assert rc == ERR_INVALID_ARG and not h.any() and not col.any() and res.n_inside == 0


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rctx():
    import online_3d_reconstruction_amd as o3dr
    with o3dr.Context(0) as c:
        yield c


@pytest.mark.gpu
@pytest.mark.parametrize("R", [0, 1, 3, 32])
def test_67_by_35_cloud_with_random_holes(rctx, R):
    xyz = grid_cloud(67, 35, holes=0.35, seed=R, extra=200)
    assert rr.extent(xyz, 0.05)[2:] == (67, 35)
    got, ref = check(rctx, xyz, 0.05, fill_radius=R, light=LIGHT)
    assert ref.info["n_shadowed"] > 0 and (ref.info["n_filled"] > 0) == (R > 0)
    check(rctx, xyz, 0.05, fill_radius=R, select="top")


@pytest.mark.gpu
def test_hole_wider_than_twice_the_radius_keeps_empty_cells(rctx):
    xyz = grid_cloud(67, 35, seed=11)
    cx, cy = rr.cells_of(xyz, 0.05)
    xyz = xyz[~((cx >= 20) & (cx < 43) & (cy >= 8) & (cy < 29))]  # a 23 x 21 hole
    for R in (3, 12):
        got, ref = check(rctx, xyz, 0.05, fill_radius=R, light=LIGHT)
        assert ref.info["n_filled"] > 0 and (ref.info["n_empty"] > 0) == (R == 3)


@pytest.mark.gpu
def test_single_cell_fills_its_disc_clipped_by_the_raster_edge(rctx):
    xyz = cells_to_xyz([(10, 40)], z=[1.5])
    got, ref = check(rctx, xyz, 1.0, bounds=(0, 0, 80, 80), fill_radius=32, light=LIGHT)
    d2 = got[4]
    yy, xx = np.mgrid[0:80, 0:80]
    want = (yy - 40) ** 2 + (xx - 10) ** 2
    assert np.array_equal(d2, np.where(want <= 32 * 32, want, -1))
    assert d2[40, 42] == 1024 and d2[40, 43] == -1  # exactly R away, and one cell farther
    # a source at R*R exactly is taken, one at R*R + 1 is not
    got, ref = check(rctx, cells_to_xyz([(0, 0)]), 1.0, bounds=(0, 0, 7, 7), fill_radius=5)
    assert got[3][4, 3] == 25 and got[3][3, 4] == 25 and got[3][1, 5] == -1 and got[3][5, 1] == -1 and got[3][0, 5] == 25


@pytest.mark.gpu
def test_sources_across_tile_borders_and_in_the_apron(rctx):
    """the row pass works on 64 x 4 cell tiles with a fill_radius-wide apron to the left and right"""
    # sources on both sides of the tile borders at column 64 and row 4 / 8, and at the far end of the apron
    cells = [(63, 3), (64, 4), (31, 7), (97, 8), (128, 0), (0, 12), (129, 12)]
    for R in (1, 7, 32):
        check(rctx, cells_to_xyz(cells, z=np.arange(len(cells))), 1.0, bounds=(0, 0, 130, 13), fill_radius=R, light=LIGHT, what=f"R={R}")
    # sparse random sources: most cells are filled from another tile
    rng = np.random.default_rng(3)
    sparse = np.unique(np.column_stack([rng.integers(0, 200, 90), rng.integers(0, 37, 90)]), axis=0)
    for R in (5, 32):
        got, ref = check(rctx, cells_to_xyz(sparse, z=rng.normal(0, 1, len(sparse))), 1.0, bounds=(0, 0, 200, 37), fill_radius=R,
                         light=LIGHT)
        assert ref.info["n_filled"] > 10 * len(sparse) * (R == 32)
    # equidistant sources in different tiles: the tie rule across the border
    check(rctx, cells_to_xyz([(62, 5), (66, 5), (64, 3), (64, 7)]), 1.0, bounds=(0, 0, 130, 13), fill_radius=4)


@pytest.mark.gpu
def test_cloud_across_the_origin(rctx):
    xyz = grid_cloud(70, 41, holes=0.2, seed=4, x0=-33, y0=-20)
    assert rr.extent(xyz, 0.05) == (-33, -20, 70, 41)
    assert rctx.rasterExtent(_pts(xyz), 0.05) == (-33, -20, 70, 41)
    check(rctx, xyz, 0.05, fill_radius=2, light=LIGHT)
    edge = np.array([[-0.05, -0.05, 1], [0.0, 0.0, 2], [-1e-9, 0.05, 3], [0.05, -1e-9, 4]], F32)  # points on cell edges
    check(rctx, edge, 0.05, fill_radius=1)


@pytest.mark.gpu
def test_one_point_and_one_cell(rctx):
    got, ref = check(rctx, np.array([[3.21, -7.65, 0.5]], F32), 0.05, fill_radius=32, light=LIGHT)
    assert got[0].shape == (1, 1) and ref.info["n_occupied"] == 1
    rng = np.random.default_rng(8)
    xyz = np.column_stack([rng.uniform(0.1001, 0.1499, 400), rng.uniform(-0.0499, -0.0001, 400), rng.normal(0, 1, 400)]).astype(F32)
    for select in ("first", "top", "bottom"):
        got, ref = check(rctx, xyz, 0.05, select=select, fill_radius=3)
        assert got[0].shape == (1, 1) and ref.info["n_shadowed"] == 399


@pytest.mark.gpu
@pytest.mark.parametrize("select", ["first", "top", "bottom"])
def test_300_points_in_5_cells_with_repeated_z(rctx, select):
    rng = np.random.default_rng(21)
    cells = np.array([(0, 0), (2, 0), (1, 1), (4, 2), (3, 2)])[rng.integers(0, 5, 300)]
    z = rng.choice(np.array([-1.5, -0.0, 0.0, 0.25, 2.0], F32), 300)
    got, ref = check(rctx, cells_to_xyz(cells, z), 1.0, select=select, fill_radius=1, light=LIGHT)
    assert ref.info["n_occupied"] == 5 and ref.info["n_shadowed"] == 295
    if select != "first":  # the extreme z, and among its repeats the lowest index
        src = got[3][got[4] == 0]
        for s in src:
            same = np.nonzero((cells == cells[s]).all(1))[0]
            zs = z[same]
            best = zs.max() if select == "top" else zs.min()
            assert z[s] == best and s == same[zs == best][0]


@pytest.mark.gpu
def test_given_boxes(rctx):
    xyz = grid_cloud(67, 35, holes=0.3, seed=6, x0=-10, y0=5, extra=100)
    for name, box in (("smaller", (0, 10, 30, 20)), ("larger", (-40, -3, 140, 50)), ("disjoint", (500, 500, 70, 9)),
                      ("row", (-10, 20, 67, 1)), ("column", (20, 5, 1, 35))):
        got, ref = check(rctx, xyz, 0.05, bounds=box, fill_radius=4, light=LIGHT, what=name)
        assert (ref.info["n_outside"] > 0) == (name != "larger") and (ref.info["n_inside"] == 0) == (name == "disjoint")
    got, ref = check(rctx, np.zeros((0, 3), F32), 0.05, bounds=(-2, -2, 70, 9), fill_radius=4, light=LIGHT, what="n = 0")
    assert ref.info["n_empty"] == 630 and np.isnan(got[-1].z_min)


@pytest.mark.gpu
def test_reference_cloud_with_fill_and_shade(rctx):
    xyz, rgba = golden_cloud()
    got, ref = check(rctx, xyz, 0.05, rgba=rgba, fill_radius=4, light=LIGHT)
    assert (got[-1].width, got[-1].height, got[-1].n_occupied, got[-1].n_filled) == (355, 376, 55940, 4637)
    assert len(np.unique(got[2])) > 50  # the relief has contrast


@pytest.mark.gpu
def test_device_tensors_repeated_calls_and_host_arrays_agree(rctx):
    import torch
    xyz = grid_cloud(150, 37, holes=0.4, seed=13, extra=500)
    p = _pts(xyz)
    kw = dict(fill_radius=6, light=LIGHT, select="bottom", return_source=True, return_distance=True, return_info=True)
    first = rctx.rasterizeMap(p, 0.05, **kw)
    assert_same(first, rr.rasterize(xyz, p["rgba"], 0.05, fill_radius=6, light=LIGHT, select="bottom"))
    dev = torch.from_numpy(p.view(np.int32).reshape(-1, 4).copy()).cuda()
    assert rctx.rasterExtent(dev, 0.05) == rctx.rasterExtent(p, 0.05)
    for _ in range(2):
        again = rctx.rasterizeMap(p, 0.05, **kw)
        on_dev = rctx.rasterizeMap(dev, 0.05, **kw)
        assert all(t.is_cuda for t in on_dev[:5]) and on_dev[0].dtype == torch.float32 and on_dev[1].dtype == torch.uint8
        assert on_dev[3].dtype == torch.int32 and tuple(on_dev[1].shape) == first[1].shape
        for a, b, d in zip(first[:5], again[:5], on_dev[:5]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), d.cpu().numpy().view(np.uint8))
        assert first[5] == again[5] or (np.isnan(first[5].z_min) and np.isnan(again[5].z_min))
        assert first[5] == on_dev[5]


@pytest.mark.gpu
def test_optional_outputs(rctx):
    """every output pointer may be NULL; the shade alone still sees the filled heights"""
    from online_3d_reconstruction_amd import _lib
    L = _lib.load_library()
    xyz = grid_cloud(67, 35, holes=0.4, seed=17)
    p = _pts(xyz)
    ref = rr.rasterize(xyz, p["rgba"], 0.05, fill_radius=3, light=LIGHT)
    got = rctx.rasterizeMap(p, 0.05, fill_radius=3, light=LIGHT)
    assert len(got) == 3 and np.array_equal(got[2], ref.shade)
    prm = _lib.RasterParamsStruct()
    L.o3dr_raster_default_params(C.byref(prm))
    prm.cell_size, prm.fill_radius, prm.use_light = 0.05, 3, 1
    prm.cx0, prm.cy0, prm.width, prm.height = 0, 0, 67, 35
    for name in ("shade", "source", "color", "distance2", "height_map", None):
        arr = {"shade": np.zeros((35, 67), np.uint8), "source": np.zeros((35, 67), np.int32), "color": np.zeros((35, 67, 3), np.uint8),
               "distance2": np.zeros((35, 67), np.int32), "height_map": np.zeros((35, 67), F32), None: None}[name]
        outs = _lib.RasterOutputsStruct()
        if name:
            setattr(outs, name, arr.ctypes.data)
        res = _lib.RasterResultStruct()
        _lib.check(L.o3dr_rasterize_map(rctx._h, p.ctypes.data, len(p), C.byref(prm), C.byref(outs) if name else None, C.byref(res), 0))
        assert (res.n_occupied, res.n_filled, res.n_empty) == tuple(ref.info[k] for k in ("n_occupied", "n_filled", "n_empty"))
        if name:
            assert np.array_equal(arr.view(np.uint8), getattr(ref, name).view(np.uint8)), name
    _lib.check(L.o3dr_rasterize_map(rctx._h, p.ctypes.data, len(p), C.byref(prm), None, None, 0))


@pytest.mark.gpu
def test_errors(rctx):
    import torch

    from online_3d_reconstruction_amd import O3drError
    xyz = grid_cloud(20, 10, seed=2)
    p = _pts(xyz)

    def fails(text, pts=p, cell=0.05, **kw):
        with pytest.raises(O3drError) as e:
            rctx.rasterizeMap(pts, cell, **kw)
        assert e.value.code == ERR_INVALID_ARG and text in str(e.value), str(e.value)

    bad = p.copy()
    bad["y"][7] = np.nan
    fails("non-finite", pts=bad)
    fails("non-finite", pts=bad, bounds=(0, 0, 20, 10))
    bad["y"][7] = np.inf
    fails("non-finite", pts=bad, bounds=(0, 0, 20, 10))
    with pytest.raises(O3drError):
        rctx.rasterExtent(bad, 0.05)
    for cell in (0.0, -0.05, np.nan, np.inf, 1e-60):
        fails("cell_size", cell=cell)
        fails("cell_size", cell=cell, bounds=(0, 0, 20, 10))
    fails("fill_radius", fill_radius=33)
    fails("fill_radius", fill_radius=-1)
    for light in ((0.0, 0.0, 0.0), (np.nan, 0.0, 1.0), (np.inf, 0.0, 1.0), (1e200, 1e200, 0.0)):
        fails("light", light=light, bounds=(0, 0, 20, 10))
    with pytest.raises(O3drError):
        rctx.rasterizeMap(p, 0.05, select="middle")
    far = _pts(np.array([[0.0, 0.0, 0.0], [1e12, 0.0, 0.0]], F32))
    fails("int32", pts=far)
    fails("int32", pts=far, bounds=(0, 0, 4, 4))
    # two points whose own box holds 20001 x 20001 cells: refused before anything of that size is allocated
    free0 = torch.cuda.mem_get_info()[0]
    wide = _pts(np.array([[0.0, 0.0, 0.0], [1000.0, 1000.0, 0.0]], F32))
    fails("2^28", pts=wide)
    fails("2^28", bounds=(0, 0, (1 << 28) + 1, 1))  # a given box of 2^28 + 1 cells
    fails("2^28", bounds=(0, 0, 1 << 14, (1 << 14) + 1))
    assert free0 - torch.cuda.mem_get_info()[0] < (256 << 20)
    fails("width, height", bounds=(0, 0, 0, 5))
    fails("width, height", bounds=(0, 0, 5, -1))
    fails("int32", bounds=(2 ** 31 - 4, 0, 5, 1))
    with pytest.raises(O3drError) as e:  # n = 0 without a box
        rctx.rasterizeMap(np.zeros(0, p.dtype), 0.05)
    assert e.value.code == ERR_INVALID_ARG and "empty cloud" in str(e.value)
    # the context still works, and a failed host call leaves zeroed outputs
    from online_3d_reconstruction_amd import _lib
    L = _lib.load_library()
    prm = _lib.RasterParamsStruct()
    L.o3dr_raster_default_params(C.byref(prm))
    prm.cell_size, prm.fill_radius, prm.width, prm.height = 0.05, 33, 20, 10
    h = np.full((10, 20), 3, F32)
    res = _lib.RasterResultStruct()
    res.width = 5
    outs = _lib.RasterOutputsStruct(h.ctypes.data, None, None, None, None)
    assert L.o3dr_rasterize_map(rctx._h, p.ctypes.data, len(p), C.byref(prm), C.byref(outs), C.byref(res), 0) == ERR_INVALID_ARG
    assert not h.any() and res.width == 0
    outs = _lib.RasterOutputsStruct(None, None, h.ctypes.data, None, None)  # a shade without a light
    prm.fill_radius = 0
    assert L.o3dr_rasterize_map(rctx._h, p.ctypes.data, len(p), C.byref(prm), C.byref(outs), C.byref(res), 0) == ERR_INVALID_ARG
    check(rctx, xyz, 0.05, fill_radius=2)
