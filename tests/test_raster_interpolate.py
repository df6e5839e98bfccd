"""GPU raster interpolation and raster sample (Context.interpolateRaster / sampleRaster, groundFilter(interpolate=True);
contract: include/o3dr_dem.h): every output and every counter bit for bit against the numpy restatement of the contract
(tests/interpolate_reference.py), over the shapes at which the kernels take another path: one cell, one row, one
column, one 64 x 64 region and one past it, several pull and push tiles, 18 levels, and rasters past the launch caps."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import interpolate_reference as R
from conftest import ROOT

ERR_INVALID_ARG = -1
F32 = np.float32
NAMES = ("o3dr_interpolate_default_params", "o3dr_raster_interpolate", "o3dr_raster_sample")
# csrc/o3dr_device.h
PULL_TILE = 32      # kInterpPullTile: cells a side of a pull tile, five levels a launch
REGION = 64         # kInterpRegion: a push tile with its apron of `smooth` cells; a level this small is the one-workgroup kernel's
MAX_BLOCKS = 1024   # kInterpMaxBlocks: workgroups of a tiled launch, the other tiles by stride


def tiles(n, t):
    return (n + t - 1) // t


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else a
    return np.ascontiguousarray(a, F32).view(np.uint32)


_REF = {}


def reference(key, make, smooth, max_level=0):
    """(raster, reference outputs) of a named case: computed once, shared, never written to"""
    if key not in _REF:
        _REF[key] = make()
        _REF[key].setflags(write=False)
    k = (key, smooth, max_level)
    if k not in _REF:
        _REF[k] = R.interpolate(_REF[key], smooth, max_level)
    return _REF[key], _REF[k]


def assert_same(got, ref, what=""):
    filled, level, info = got
    rf, rl, ri = ref
    level = level.cpu().numpy() if hasattr(level, "cpu") else level
    assert level.dtype == np.uint8 and np.array_equal(level, rl), (what, "level", int((level != rl).sum()))
    d = bits(filled) != bits(rf)
    assert bits(filled).shape == rf.shape and not d.any(), (what, "filled", int(d.sum()), np.argwhere(d)[:4].tolist(), bits(filled)[d][:4], bits(rf)[d][:4])
    want = dict(ri, n_by_level=tuple(ri["n_by_level"][:ri["n_levels"]]))
    assert dict(info.__dict__) == want, (what, info, want)
    assert info.n_data + info.n_filled + info.n_empty == rf.size


def check(ctx, key, make, smooth, max_level=0):
    Z, ref = reference(key, make, smooth, max_level)
    got = ctx.interpolateRaster(Z, smooth=smooth, max_level=max_level, return_level=True, return_info=True)
    assert_same(got, ref, f"{key} smooth {smooth} max_level {max_level}")
    return got, ref


def half_data(h, w, seed):
    def make():
        rng = np.random.default_rng(seed)
        Z = (rng.normal(size=(h, w)) * 3 + 10).astype(F32)
        Z[rng.random((h, w)) < 0.5] = np.nan
        Z[rng.integers(0, h), rng.integers(0, w)] = 1.5  # (never without data)
        return Z
    return make


def rectangles(h, w, seed, removed=0.0):
    def make():
        rng = np.random.default_rng(seed)
        y, x = np.mgrid[0:h, 0:w]
        Z = (np.sin(x / 17.0) * np.cos(y / 13.0) + rng.normal(0, 0.05, (h, w))).astype(F32)
        Z[rng.random((h, w)) < removed] = np.nan
        for _ in range(max(3, h * w // 40000)):
            rh, rw = (int(v) for v in rng.integers(5, max(6, min(h, w, 400) // 2), 2))
            r0, c0 = int(rng.integers(0, h)), int(rng.integers(0, w))
            Z[r0:r0 + rh, c0:c0 + rw] = np.nan
        return Z
    return make


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_the_three_functions_are_declared_in_the_dem_header_exported_and_bound():
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib

    def declared(name):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        return set(re.findall(r"\b(o3dr_[a-z0-9_]+)\s*\(", txt))
    assert declared("o3dr_dem.h") == set(NAMES)
    for other in ("o3dr.h", "o3dr_terrain.h", "o3dr_objects.h", "o3dr_testing.h"):
        assert not declared(other) & set(NAMES), other
    L = _lib.load_library()  # first: it imports torch before the library, so that the process holds one HIP runtime
    lib = C.CDLL(_lib.lib_path())
    assert all(hasattr(lib, n) for n in NAMES) and set(NAMES) <= {n for n, _, _ in _lib.SYMBOLS}
    assert C.sizeof(_lib.InterpolateParamsStruct) == 16 and C.sizeof(_lib.InterpolateOutputsStruct) == 16
    assert C.sizeof(_lib.InterpolateResultStruct) == 16 + 3 * 8 + 32 * 8
    assert (_lib.INTERPOLATE_MAX_SMOOTH, _lib.INTERPOLATE_MAX_LEVELS) == (8, 32)
    assert (_lib.K_INTERP_PULL, _lib.K_INTERP_PUSH, _lib.K_RASTER_SAMPLE) == (40, 41, 42)
    assert _lib.DEM_KERNEL_NAMES == ["interp_pull", "interp_push", "raster_sample"]
    header = open(os.path.join(ROOT, "include", "o3dr.h")).read()
    for name, k in (("O3DR_K_INTERP_PULL", 40), ("O3DR_K_INTERP_PUSH", 41), ("O3DR_K_RASTER_SAMPLE", 42), ("O3DR_K_NUM", 43)):
        assert re.search(rf"#define {name}\s+{k}\b", header), name
    assert [f.name for f in o3dr.InterpolateInfo.__dataclass_fields__.values()] == [
        "width", "height", "n_levels", "n_data", "n_filled", "n_empty", "n_by_level"]
    prm = _lib.InterpolateParamsStruct(9, 9, 9, 9)
    L.o3dr_interpolate_default_params(C.byref(prm))
    assert (prm.width, prm.height, prm.smooth, prm.max_level) == (0, 0, 2, 0)
    L.o3dr_interpolate_default_params(None)


def test_null_context_is_rejected():
    """both calls, with the host outputs, the result and the counts zeroed"""
    from online_3d_reconstruction_amd import _lib
    from test_rasterize_map import _pts
    L = _lib.load_library()
    Z, filled, level = np.ones((2, 2), F32), np.full((2, 2), 5, F32), np.full((2, 2), 5, np.uint8)
    prm = _lib.InterpolateParamsStruct(2, 2, 2, 0)
    outs = _lib.InterpolateOutputsStruct(filled.ctypes.data, level.ctypes.data)
    res = _lib.InterpolateResultStruct()
    res.n_data, res.n_by_level[31] = 3, 3
    assert L.o3dr_raster_interpolate(None, Z.ctypes.data, C.byref(prm), C.byref(outs), C.byref(res), 0) == ERR_INVALID_ARG
    assert b"ctx" in L.o3dr_last_error()
    assert not filled.any() and not level.any() and res.n_data == 0 and res.n_by_level[31] == 0
    p = _pts(np.zeros((2, 3), F32))
    value, above, counts = np.full(2, 5, F32), np.full(2, 5, F32), (C.c_int64 * 3)(7, 7, 7)
    rc = L.o3dr_raster_sample(None, p.ctypes.data, 2, 1.0, 0, 0, 2, 2, Z.ctypes.data, value.ctypes.data, above.ctypes.data, counts, 0)
    assert rc == ERR_INVALID_ARG and b"ctx" in L.o3dr_last_error()
    assert not value.any() and not above.any() and list(counts) == [0, 0, 0]


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ictx():
    import online_3d_reconstruction_amd as o3dr
    with o3dr.Context(0) as c:
        yield c


SHAPES = [(1, 1), (1, 2), (2, 1), (1, 7), (5, 3), (33, 65), (64, 64), (65, 64), (130, 257)]  # [height, width]


@pytest.mark.gpu
@pytest.mark.parametrize("smooth", [0, 1, 2, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_shapes(ictx, shape, smooth):
    """1 x 1: no level above 0; up to 64 x 64: the one-workgroup kernel does every level above 0 and one push tile level 0;
    65 x 64 and 130 x 257: tiled pulls, and push tiles that end inside the raster (64 - 2 smooth cells a side)"""
    h, w = shape
    _, (_, _, info) = check(ictx, f"half {h}x{w}", half_data(h, w, 100 * h + w), smooth)
    assert info["n_levels"] == len(R.level_shapes(w, h))
    if h * w > 2:
        assert info["n_filled"] > 0


PATTERN_SHAPE = (70, 133)  # past one push tile and one pull tile both ways at every smooth; level 1 (35 x 67) is past one region


def pattern(name):
    h, w = PATTERN_SHAPE
    rng = np.random.default_rng(len(name))
    base = (rng.normal(size=(h, w)) * 2).astype(F32)

    def make():
        Z = np.full((h, w), np.nan, F32)
        if name.startswith("corner"):
            r, c = {"corner00": (0, 0), "corner0w": (0, w - 1), "cornerh0": (h - 1, 0), "cornerhw": (h - 1, w - 1)}[name]
            Z[r, c] = F32(-7.3125)
        elif name == "checkerboard":
            y, x = np.mgrid[0:h, 0:w]
            Z = np.where((x + y) & 1, base, np.nan).astype(F32)
        elif name in ("data5", "data95"):
            keep = rng.random((h, w)) < (0.05 if name == "data5" else 0.95)
            Z = np.where(keep, base, np.nan).astype(F32)
        elif name == "rectangles":
            Z = rectangles(h, w, 11)()
        elif name == "special":  # -0.0f, denormals, +-1e30 side by side, between holes
            vals = np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, -3e-41, 1e30, -1e30, 3.4e38, -3.4e38, 1.0, -1.0], F32)
            Z = vals[rng.integers(0, len(vals), (h, w))]
            Z[rng.random((h, w)) < 0.4] = np.nan
            Z[10:40, 20:90] = np.nan
        return Z
    return make


@pytest.mark.gpu
@pytest.mark.parametrize("smooth", [0, 2])
@pytest.mark.parametrize("name", ["corner00", "corner0w", "cornerh0", "cornerhw", "checkerboard", "data5", "data95", "rectangles", "special"])
def test_patterns(ictx, name, smooth):
    (filled, _, _), (_, _, info) = check(ictx, name, pattern(name), smooth)
    if name.startswith("corner"):  # the one value's bits everywhere
        assert (bits(filled) == bits(np.array([-7.3125], F32))[0]).all() and info["n_by_level"][0] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("max_level", [1, 3])
def test_max_level(ictx, max_level):
    _, (_, lev, info) = check(ictx, "rectangles", pattern("rectangles"), 2, max_level)
    assert info["n_empty"] == (lev > max_level).sum() > 0 and info["n_filled"] > 0


@pytest.mark.gpu
def test_no_data_and_holes_of_every_payload(ictx):
    Z = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF, 0xFF800123, 0x7FC00000], np.uint32).view(F32).reshape(2, 3)
    for key, make in (("nan 2x3", lambda: Z.copy()), ("nan 1x1", lambda: Z[:1, :1].copy()), ("nan 70x133", lambda: np.full(PATTERN_SHAPE, np.nan, F32))):
        (filled, level, info), _ = check(ictx, key, make, 2)
        assert (bits(filled) == R.NAN_BITS).all() and (level == 255).all() and info.n_empty == filled.size and not any(info.n_by_level)

    def payloads():
        big = half_data(40, 50, 8)()
        big[np.isnan(big)] = np.resize(Z.ravel(), int(np.isnan(big).sum()))
        return big
    check(ictx, "payloads", payloads, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 100000), (100000, 1)], ids=["1x100000", "100000x1"])
def test_long_rasters(ictx, shape):
    """18 levels (L = 17): three tiled pulls of five levels, the one-workgroup kernel from level 16 (2 cells) down to level 11
    (49 cells), eleven tiled pushes of one tile column"""
    h, w = shape

    def make():
        Z = half_data(h, w, 5)()
        Z[:, 30000:52000] = np.nan
        Z[30000:52000, :] = np.nan
        return Z
    _, (_, _, info) = check(ictx, f"long {h}x{w}", make, 2)
    assert info["n_levels"] == 18 and info["n_by_level"][15] > 0


@pytest.mark.gpu
def test_large_raster_past_the_pull_cap(ictx):
    """1100 x 1500 with half the cells removed plus rectangles.  Level 0 has 35 x 47 = 1645 pull tiles of 32 x 32, past the
    1024 workgroups of a launch (621 workgroups take two tiles); the push of level 0 has 19 x 25 = 475 tiles of 60 x 60
    at smooth = 2, past one tile both ways."""
    h, w = 1100, 1500
    assert tiles(h, PULL_TILE) * tiles(w, PULL_TILE) == 1645 > MAX_BLOCKS
    assert tiles(h, REGION - 4) * tiles(w, REGION - 4) == 475
    _, (_, _, info) = check(ictx, "large", rectangles(h, w, 21, removed=0.5), 2)
    assert info["n_filled"] > h * w // 2 and info["n_by_level"][6] > 0


@pytest.mark.gpu
def test_narrow_raster_past_the_push_cap(ictx):
    """24960 x 49 at smooth = 8: 520 x 2 = 1040 push tiles of 48 x 48 at level 0, past the 1024 workgroups of a launch (16
    workgroups take two tiles), and 780 x 2 = 1560 pull tiles"""
    h, w = 24960, 49
    assert tiles(h, REGION - 16) * tiles(w, REGION - 16) == 1040 > MAX_BLOCKS
    assert tiles(h, PULL_TILE) * tiles(w, PULL_TILE) == 1560 > MAX_BLOCKS
    check(ictx, "narrow", rectangles(h, w, 22, removed=0.5), 8)


@pytest.mark.gpu
def test_host_and_device_memory_and_a_second_call(ictx):
    import torch
    Z, ref = reference("rectangles", pattern("rectangles"), 2)
    zd = torch.from_numpy(np.array(Z)).cuda()
    for k in range(2):
        got = ictx.interpolateRaster(zd, return_level=True, return_info=True)
        assert got[0].is_cuda and got[1].is_cuda and got[0].dtype == torch.float32 and got[1].dtype == torch.uint8
        assert_same(got, ref, f"device call {k}")
        assert_same(ictx.interpolateRaster(Z, return_level=True, return_info=True), ref, f"host call {k}")
    assert np.array_equal(bits(zd), bits(Z))  # the input is not written
    only = ictx.interpolateRaster(Z)  # the level and the record are optional
    assert isinstance(only, np.ndarray) and np.array_equal(bits(only), bits(ref[0]))


@pytest.mark.gpu
def test_result_does_not_depend_on_old_scratch_contents():
    """after 0xFF and 0x00 over every scratch block, and after a larger call (DESIGN.md "Scratch contract")"""
    from test_scratch_independence import blob, fill, hooked_context
    cases = [("rectangles", pattern("rectangles"), 2), ("half 65x64", half_data(65, 64, 6564), 8), ("special", pattern("special"), 0)]

    def call(ctx):
        return [ctx.interpolateRaster(reference(k, m, s)[0], smooth=s, return_level=True, return_info=True) for k, m, s in cases]
    with hooked_context() as ctx:
        first = call(ctx)
        for got, (k, m, s) in zip(first, cases):
            assert_same(got, reference(k, m, s)[1], k)
        want = blob(first)
        assert fill(ctx, 0xFF) > 0
        assert blob(call(ctx)) == want, "after 0xFF over the scratch"
        assert fill(ctx, 0x00) > 0
        assert blob(call(ctx)) == want, "after 0x00 over the scratch"
        check(ctx, "half 130x257", half_data(130, 257, 13257), 2)
        check(ctx, "large", rectangles(1100, 1500, 21, removed=0.5), 2)
        assert blob(call(ctx)) == want, "after larger calls"


@pytest.mark.gpu
def test_errors_in_the_contracts_order(ictx):
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib
    L, h = _lib.load_library(), ictx._h
    Z = np.ones((3, 4), F32)
    Z[1, 1] = np.inf
    filled, level = np.full((3, 4), 5, F32), np.full((3, 4), 5, np.uint8)

    def call(prm, raster=Z, outs=True, mem=0, res=None):
        filled[:], level[:] = 5, 5
        o = _lib.InterpolateOutputsStruct(filled.ctypes.data, level.ctypes.data)
        rc = L.o3dr_raster_interpolate(h, None if raster is None else raster.ctypes.data, None if prm is None else C.byref(prm),
                                       C.byref(o) if outs else None, None if res is None else C.byref(res), mem)
        return rc, L.o3dr_last_error().decode()

    def P(width=4, height=3, smooth=2, max_level=0):
        return _lib.InterpolateParamsStruct(width, height, smooth, max_level)
    # every later error is present as well: the earlier one is reported
    steps = [("NULL", dict(prm=None, mem=7)), ("NULL", dict(prm=P(0, 0, 9, 99), raster=None, mem=7)),
             ("NULL", dict(prm=P(0, 0, 9, 99), outs=False, mem=7)), ("mem", dict(prm=P(0, 0, 9, 99), mem=7)),
             ("width, height", dict(prm=P(0, 3, 9, 99))), ("width, height", dict(prm=P(4, -1, 9, 99))), ("smooth", dict(prm=P(4, 3, 9, 99))),
             ("smooth", dict(prm=P(4, 3, -1, 99))), ("max_level", dict(prm=P(4, 3, 8, 32))), ("max_level", dict(prm=P(4, 3, 0, -1))),
             ("2^28", dict(prm=P(1 << 14, (1 << 14) + 1, 2, 0))), ("infinite", dict(prm=P()))]
    for text, kw in steps:
        res = _lib.InterpolateResultStruct()
        res.n_data = 3
        rc, err = call(res=res, **kw)
        assert rc == ERR_INVALID_ARG and text in err, (text, err)
        assert res.n_data == 0 and res.width == 0
        if text in ("smooth", "max_level", "infinite"):  # host outputs zeroed (where the parameters give their size)
            assert not filled.any() and not level.any(), text
    o = _lib.InterpolateOutputsStruct(None, level.ctypes.data)
    assert L.o3dr_raster_interpolate(h, Z.ctypes.data, C.byref(P()), C.byref(o), None, 0) == ERR_INVALID_ARG
    Z[1, 1] = -np.inf
    with pytest.raises(o3dr.O3drError) as e:
        ictx.interpolateRaster(Z)
    assert e.value.code == ERR_INVALID_ARG and "infinite" in str(e.value)
    for bad in (dict(smooth=9), dict(max_level=32)):
        with pytest.raises(o3dr.O3drError):
            ictx.interpolateRaster(np.ones((2, 2), F32), **bad)
    # the limits themselves are fine, and the context still works
    Z[1, 1] = np.nan
    for kw in (dict(smooth=8, max_level=31), dict(smooth=0, max_level=1)):
        assert_same(ictx.interpolateRaster(Z, return_level=True, return_info=True, **kw), R.interpolate(Z, **kw), str(kw))


# ---- sampleRaster and groundFilter(interpolate=True) ------------------------------------------------------------------------
def ground_scene():
    """the 50 %-occupancy scene of tests/test_ground_filter.py with points outside the box that is given"""
    from test_ground_filter import random_cells
    if "ground" not in _REF:
        xyz = random_cells(150, 90, 3, cell=0.5, occupancy=0.5)
        _REF["ground"] = (xyz, (10, 5, 120, 70))  # the cloud covers cells 0..149 x 0..89
    return _REF["ground"]


KW = dict(max_window_radius=16, slope=0.3)


@pytest.mark.gpu
@pytest.mark.parametrize("fill_radius", [0, 3])
def test_sample_equals_the_ground_filters_height_above_ground(ictx, fill_radius):
    import torch
    from test_ground_filter import run
    from test_rasterize_map import _pts
    xyz, box = ground_scene()
    pts = _pts(xyz)
    _, hag, dtm, _, ginfo = run(ictx, pts, 0.5, bounds=box, fill_radius=fill_radius, **KW)
    assert ginfo.n_outside > 1000 and ginfo.n_dtm_empty > 0 and np.isnan(hag).sum() > ginfo.n_outside
    above, value, counts = ictx.sampleRaster(pts, dtm, 0.5, box, return_value=True, return_info=True)
    assert above.dtype == F32 and np.array_equal(bits(above), bits(hag)), int((bits(above) != bits(hag)).sum())
    rv, ra, rc = R.sample(xyz, dtm, 0.5, box)
    assert np.array_equal(bits(value), bits(rv)) and np.array_equal(bits(above), bits(ra)) and counts == rc
    assert counts[0] == ginfo.n_inside and counts[1] == ginfo.n_outside and counts[2] > 0
    assert (bits(above)[np.isnan(above)] == R.NAN_BITS).all()
    # device memory, and each output alone
    pd, dd = torch.from_numpy(pts.view(np.int32).reshape(-1, 4).copy()).cuda(), torch.from_numpy(dtm).cuda()
    a2, v2, c2 = ictx.sampleRaster(pd, dd, 0.5, box, return_value=True, return_info=True)
    assert a2.is_cuda and np.array_equal(bits(a2), bits(hag)) and np.array_equal(bits(v2), bits(rv)) and c2 == rc
    assert np.array_equal(bits(ictx.sampleRaster(pts, dtm, 0.5, box)), bits(hag))
    # no point at all
    a0, c0 = ictx.sampleRaster(pts[:0], dtm, 0.5, box, return_info=True)
    assert len(a0) == 0 and c0 == (0, 0, 0)


@pytest.mark.gpu
def test_sample_errors(ictx):
    import online_3d_reconstruction_amd as o3dr
    from test_rasterize_map import _pts
    xyz, box = ground_scene()
    pts, dtm = _pts(xyz[:100]), np.zeros((box[3], box[2]), F32)
    for text, kw in (("cell_size", dict(cell_size=0.0)), ("width, height", dict(bounds=(0, 0, 0, 5))), ("int32", dict(bounds=(2 ** 31 - 3, 0, 5, 5)))):
        b = kw.get("bounds", box)
        with pytest.raises(o3dr.O3drError) as e:
            ictx.sampleRaster(pts, np.zeros((b[3], b[2]), F32), kw.get("cell_size", 0.5), b)
        assert e.value.code == ERR_INVALID_ARG and text in str(e.value), (text, str(e.value))
    bad = pts.copy()
    bad["y"][7] = np.nan
    with pytest.raises(o3dr.O3drError) as e:
        ictx.sampleRaster(bad, dtm, 0.5, box)
    assert "non-finite" in str(e.value)


@pytest.mark.gpu
def test_ground_filter_with_an_interpolated_dtm(ictx):
    import torch
    from test_ground_filter import run
    from test_rasterize_map import _pts
    xyz, box = ground_scene()
    pts = _pts(xyz)
    ground, _, dtm0, state, ginfo = run(ictx, pts, 0.5, bounds=box, **KW)
    g2, hag, dtm, s2, ginfo2, dinfo = run(ictx, pts, 0.5, bounds=box, interpolate=True, **KW)
    assert np.array_equal(g2, ground) and np.array_equal(s2, state) and ginfo2 == ginfo  # the mask and the states: unchanged
    want, winfo = ictx.interpolateRaster(dtm0, return_info=True)
    assert np.array_equal(bits(dtm), bits(want)) and dinfo == winfo and dinfo.n_data == ginfo.n_ground_cells and dinfo.n_empty == 0
    assert np.array_equal(bits(dtm), bits(R.interpolate(dtm0)[0]))
    inside = ~np.isnan(R.sample(xyz, np.zeros_like(dtm), 0.5, box)[0])
    assert inside.sum() == ginfo.n_inside and np.isfinite(hag[inside]).all() and np.isnan(hag[~inside]).all()
    assert np.array_equal(bits(hag), bits(R.sample(xyz, dtm, 0.5, box)[1]))
    # smooth is passed on; the outputs that are not asked for are not returned
    g3, dtm3 = ictx.groundFilter(pts, 0.5, bounds=box, interpolate=True, smooth=0, return_dtm=True, **KW)
    assert np.array_equal(g3, ground) and np.array_equal(bits(dtm3), bits(R.interpolate(dtm0, 0)[0]))
    assert np.array_equal(ictx.groundFilter(pts, 0.5, bounds=box, interpolate=True, **KW), ground)
    # device tensors stay on the device
    pd = torch.from_numpy(pts.view(np.int32).reshape(-1, 4).copy()).cuda()
    gd, hd, dd = ictx.groundFilter(pd, 0.5, bounds=box, interpolate=True, return_height=True, return_dtm=True, **KW)
    assert gd.is_cuda and hd.is_cuda and dd.is_cuda
    assert np.array_equal(gd.cpu().numpy(), ground) and np.array_equal(bits(hd), bits(hag)) and np.array_equal(bits(dd), bits(dtm))
    with pytest.raises(ValueError):
        ictx.groundFilter(pts, 0.5, bounds=box, interpolate=True, fill_radius=2, **KW)
    # without the keyword nothing changes
    assert np.array_equal(bits(run(ictx, pts, 0.5, bounds=box, interpolate=False, **KW)[2]), bits(dtm0))
