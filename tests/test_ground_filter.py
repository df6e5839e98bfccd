"""Ground filter on the GPU (o3dr_ground_filter, o3dr_ground_schedule, Context.groundFilter / groundSchedule; contract:
include/o3dr_terrain.h): every output and every counter bit for bit against the numpy restatement of the contract
(ground_reference.py), on rasters small enough for a few seconds in total but past one row segment (256 cells), one
block of 2r + 1 rows and one workgroup of the column passes in both directions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ground_reference as gr
from conftest import ROOT
from test_ground_reference import SCHEDULES, scene_result
from test_raster_reference import cells_to_xyz
from test_rasterize_map import _pts

ERR_INVALID_ARG = -1
F32 = np.float32
NAMES = ("o3dr_ground_default_params", "o3dr_ground_filter", "o3dr_ground_schedule")
TILE = dict(max_window_radius=128, slope=0.02, initial_distance=0.15, max_distance=10.0)  # radii 1, 2, 4, ..., 128


def run(ctx, pts, cell, **kw):
    return ctx.groundFilter(pts, cell, return_height=True, return_dtm=True, return_state=True, return_info=True, **kw)


def assert_same(got, ref, what=""):
    """got: groundFilter's tuple with every output asked for; ref: ground_reference.ground_filter's namespace.  The states
    first: they say which iteration differs."""
    ground, hag, dtm, state, info = [g.cpu().numpy() if hasattr(g, "cpu") else g for g in got]
    assert state.dtype == np.uint8 and state.shape == ref.cell_state.shape, (what, state.shape, ref.cell_state.shape)
    diff = state != ref.cell_state
    assert not diff.any(), (what, "cell_state", int(diff.sum()), sorted(set(ref.cell_state[diff].tolist())), sorted(set(state[diff].tolist())))
    for name, g, r in (("dtm", dtm, ref.dtm), ("height_above_ground", hag, ref.height_above_ground)):
        assert g.dtype == F32 and g.shape == r.shape, (what, name, g.shape, r.shape)
        assert np.array_equal(g.view(np.uint32), r.view(np.uint32)), (what, name, int((g.view(np.uint32) != r.view(np.uint32)).sum()))
    assert ground.dtype == np.uint8 and np.array_equal(ground, ref.ground), (what, "ground")
    assert dict(info.__dict__) == ref.info, (what, info, ref.info)


def check(ctx, xyz, cell, what="", **kw):
    ref = gr.ground_filter(xyz, cell, **kw)
    got = run(ctx, _pts(xyz), cell, **kw)
    assert_same(got, ref, what or str(kw))
    return got, ref


def random_cells(w, h, seed, cell=0.5, occupancy=0.5, x0=0, y0=0):
    """`occupancy` of the cells of a w x h raster, one point each: rough ground, spikes, and plateaus 2 - 8 m high whose
    sides are log-uniform from one cell to past the raster, so that windows of every size find something to remove"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(w) + x0, np.arange(h) + y0)
    zz = rng.normal(0, 0.05, (h, w)) + (rng.random((h, w)) < 0.05) * rng.uniform(0, 8, (h, w))
    for _ in range(max(4, w * h // 1500)):
        pw, ph = (int(np.exp(rng.uniform(0, np.log(1.3 * s + 1)))) for s in (w, h))
        c0, r0 = rng.integers(-pw // 2, w), rng.integers(-ph // 2, h)
        zz[max(r0, 0):r0 + ph, max(c0, 0):c0 + pw] = rng.uniform(2, 8) + rng.normal(0, 0.02)
    keep = rng.random(w * h) < occupancy
    keep[rng.integers(0, w * h)] = True
    cells = np.column_stack([gx.ravel(), gy.ravel()])[keep]
    z = zz.ravel()[keep]
    xyz = cells_to_xyz(cells, z, cell)
    return xyz[rng.permutation(len(xyz))]


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_the_three_functions_are_declared_in_the_terrain_header_exported_and_bound():
    from online_3d_reconstruction_amd import _lib

    def declared(name):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
        return set(re.findall(r"\b(o3dr_[a-z0-9_]+)\s*\(", txt))
    assert declared("o3dr_terrain.h") == set(NAMES)
    assert not any("ground" in n for n in declared("o3dr.h"))
    lib = C.CDLL(_lib.lib_path())
    assert all(hasattr(lib, n) for n in NAMES) and set(NAMES) <= {n for n, _, _ in _lib.SYMBOLS}
    assert (_lib.O3DR_GROUND_MAX_WINDOW_RADIUS, _lib.O3DR_GROUND_MAX_ITERATIONS) == (128, 16)
    assert C.sizeof(_lib.GroundParamsStruct) == 72 and C.sizeof(_lib.GroundResultStruct) == 208


def test_defaults_are_pcls():
    from online_3d_reconstruction_amd import _lib
    L = _lib.load_library()
    prm = _lib.GroundParamsStruct()
    prm.cell_size, prm.width, prm.fill_radius = 9.0, 9, 9
    L.o3dr_ground_default_params(C.byref(prm))
    assert (prm.cell_size, prm.cx0, prm.cy0, prm.width, prm.height, prm.fill_radius) == (0.0, 0, 0, 0, 0, 0)
    assert (prm.max_window_radius, prm.window_base, prm.exponential) == (16, 2, 1)
    assert (prm.slope, prm.initial_distance, prm.max_distance) == (0.7, 0.15, 10.0)


def test_schedule_agrees_with_the_reference_on_a_grid():
    import online_3d_reconstruction_amd as o3dr
    n = 0
    for cell in (0.05, 0.1, 1.0 / 3.0, 2.5):
        for rmax in (1, 2, 3, 16, 33, 127, 128):
            for base, exponential in ((2, True), (3, True), (10, True), (1, False), (2, False), (4, False), (7, False)):
                for slope, d0, dmax in ((0.7, 0.15, 10.0), (0.3, 0.15, 2.0), (0.0, 0.0, 0.0), (1.1, 0.07, 0.5), (1e-3, 1e-3, 1e6)):
                    if not exponential and base > rmax:
                        continue
                    r, t = o3dr.groundSchedule(cell, rmax, base, exponential, slope, d0, dmax)
                    rr_, tt = gr.schedule(cell, rmax, base, exponential, slope, d0, dmax)
                    assert r.dtype == np.int32 and t.dtype == F32 and np.array_equal(r, rr_), (cell, rmax, base, exponential)
                    assert np.array_equal(t.view(np.uint32), tt.view(np.uint32)), (cell, rmax, base, exponential, slope, d0, dmax)
                    n += 1
    assert n > 800


def test_schedule_rejects_bad_parameters():
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib
    L = _lib.load_library()
    for text, kw in (("cell_size", dict(cell_size=0.0)), ("cell_size", dict(cell_size=np.nan)), ("max_window_radius", dict(max_window_radius=0)),
                     ("max_window_radius", dict(max_window_radius=129)), ("window_base", dict(window_base=1)),
                     ("window_base", dict(window_base=0, exponential=False)), ("slope", dict(slope=-0.1)), ("slope", dict(slope=np.inf)),
                     ("initial_distance", dict(initial_distance=np.nan)), ("max_distance", dict(max_distance=-1.0)),
                     ("no iteration", dict(window_base=17, exponential=False))):
        with pytest.raises(o3dr.O3drError) as e:
            o3dr.groundSchedule(**{"cell_size": 0.1, **kw})
        assert e.value.code == ERR_INVALID_ARG and text in str(e.value), (text, str(e.value))
    prm = _lib.GroundParamsStruct()
    L.o3dr_ground_default_params(C.byref(prm))
    prm.cell_size, prm.max_window_radius = 0.1, 0
    radii, thr, n = np.full(16, 7, np.int32), np.full(16, 7, F32), C.c_int32(7)
    assert L.o3dr_ground_schedule(C.byref(prm), radii.ctypes.data, thr.ctypes.data, C.byref(n)) == ERR_INVALID_ARG
    assert not radii.any() and not thr.any() and n.value == 0
    assert L.o3dr_ground_schedule(None, radii.ctypes.data, thr.ctypes.data, C.byref(n)) == ERR_INVALID_ARG


def test_null_context_is_rejected():
    from online_3d_reconstruction_amd import _lib
    L = _lib.load_library()
    prm = _lib.GroundParamsStruct()
    L.o3dr_ground_default_params(C.byref(prm))
    prm.cell_size, prm.width, prm.height = 1.0, 2, 2
    p = _pts(cells_to_xyz([(0, 0), (1, 1)]))
    ground, dtm = np.full(2, 5, np.uint8), np.full((2, 2), 5, F32)
    outs = _lib.GroundOutputsStruct(ground.ctypes.data, None, dtm.ctypes.data, None)
    res = _lib.GroundResultStruct()
    res.n_inside, res.n_removed[3] = 3, 3
    rc = L.o3dr_ground_filter(None, p.ctypes.data, 2, C.byref(prm), C.byref(outs), C.byref(res), 0)
    assert rc == ERR_INVALID_ARG and b"ctx" in L.o3dr_last_error()
    assert not ground.any() and not dtm.any() and res.n_inside == 0 and res.n_removed[3] == 0


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gctx():
    import online_3d_reconstruction_amd as o3dr
    with o3dr.Context(0) as c:
        yield c


@pytest.mark.gpu
@pytest.mark.parametrize("fill_radius", [0, 32])
@pytest.mark.parametrize("sched", list(SCHEDULES))
def test_scene_of_buildings_and_posts(gctx, sched, fill_radius):
    sc, ref = scene_result(0, sched, fill_radius)
    got = run(gctx, _pts(sc.xyz), gr.SCENE_CELL, bounds=gr.SCENE_BOX, fill_radius=fill_radius, **gr.SCENE_PARAMS, **SCHEDULES[sched])
    assert_same(got, ref, f"{sched} fill {fill_radius}")
    assert sum(1 for v in ref.info["n_removed"] if v) >= 4 and (ref.info["n_dtm_filled"] > 0) == (fill_radius > 0)
    assert gctx.rasterExtent(_pts(sc.xyz), gr.SCENE_CELL) == gr.SCENE_BOX  # bounds=None is this box
    if fill_radius == 0:
        assert_same(run(gctx, _pts(sc.xyz), gr.SCENE_CELL, **gr.SCENE_PARAMS, **SCHEDULES[sched]), ref, "the cloud's own box")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1), (65, 33), (130, 70), (300, 40), (40, 300), (257, 3), (513, 259)])
def test_windows_past_the_raster_the_row_segments_and_the_row_blocks(gctx, w, h):
    """radii 1 .. 128: larger than the raster, an apron over several 256-cell segments, blocks of 3 .. 257 rows"""
    xyz = random_cells(w, h, seed=w * 1000 + h, x0=-7, y0=3)
    got, ref = check(gctx, xyz, 0.5, bounds=(-7, 3, w, h), fill_radius=5, **TILE)
    assert ref.info["n_iterations"] == 8 and ref.info["n_occupied"] == len(xyz)
    if w * h > 2000:
        assert sum(1 for v in ref.info["n_removed"] if v) >= 3 and ref.info["n_ground_cells"] > 0, ref.info
    if (w, h) == (513, 259):
        assert all(ref.info["n_removed"]), "every radius up to 128 removes something here"
    check(gctx, xyz, 0.5, bounds=(-7, 3, w, h), max_window_radius=21, window_base=3, exponential=False, slope=0.2)  # radii 3, 6, ..., 21


@pytest.mark.gpu
def test_three_points_per_cell(gctx):
    """the mask of step 5: a ground cell's points within initial_distance of its lowest are ground, the others are not"""
    rng = np.random.default_rng(9)
    xyz = random_cells(90, 50, seed=9, cell=0.5, occupancy=0.8)
    extra = np.concatenate([xyz + np.array([0.1, -0.1, dz], F32) for dz in (0.1499, 0.1501)])
    extra[:, 2] += rng.choice(np.array([0.0, 1e-4, -1e-4], F32), len(extra))
    pts = np.concatenate([xyz, extra])[rng.permutation(3 * len(xyz))]
    got, ref = check(gctx, pts, 0.5, max_window_radius=8, fill_radius=2)
    assert ref.info["n_inside"] == 3 * ref.info["n_occupied"] and ref.info["n_ground_cells"] < ref.info["n_ground_points"] < 3 * ref.info["n_ground_cells"]
    assert (ref.height_above_ground[ref.ground == 1] <= F32(0.15)).all() and (ref.height_above_ground[ref.ground == 0] > F32(0.15)).sum() > 100
    # repeated z in a cell, the two zeros among them: ties go to the lowest index, and a zero's sign survives the copy
    cells = np.array([(0, 0), (2, 0), (1, 1), (4, 2), (3, 2)])[rng.integers(0, 5, 300)]
    z = rng.choice(np.array([-0.0, 0.0, 0.1, 0.2], F32), 300)
    check(gctx, cells_to_xyz(cells, z), 1.0, max_window_radius=2, fill_radius=1)


@pytest.mark.gpu
def test_given_boxes_and_an_empty_cloud(gctx):
    xyz = random_cells(90, 50, seed=4, x0=-10, y0=5)
    for name, box in (("smaller", (0, 10, 30, 20)), ("larger", (-40, -3, 140, 70)), ("disjoint", (500, 500, 70, 9)), ("row", (-10, 20, 90, 1)),
                      ("column", (20, 5, 1, 50))):
        got, ref = check(gctx, xyz, 0.5, bounds=box, fill_radius=4, max_window_radius=8, what=name)
        assert (ref.info["n_outside"] > 0) == (name != "larger") and (ref.info["n_inside"] == 0) == (name == "disjoint")
        outside = np.ones(len(xyz), bool) if name == "disjoint" else None
        if name == "smaller":
            cx, cy = gr.rr.cells_of(xyz, 0.5)
            outside = ~((cx >= 0) & (cx < 30) & (cy >= 10) & (cy < 30))
        if outside is not None:
            assert outside.any() and not got[0][outside].any() and np.isnan(got[1][outside]).all()
    got, ref = check(gctx, np.zeros((0, 3), F32), 0.5, bounds=(-2, -2, 70, 9), fill_radius=4, what="n = 0")
    assert ref.info["n_dtm_empty"] == 630 and got[0].shape == (0,) and got[1].shape == (0,) and not got[3].any() and np.isnan(got[2]).all()


@pytest.mark.gpu
def test_cloud_40_km_from_the_origin(gctx):
    xyz = random_cells(140, 60, seed=12, cell=0.5, x0=80000, y0=-80000)
    got, ref = check(gctx, xyz, 0.5, max_window_radius=16, fill_radius=3)
    assert (ref.info["cx0"], ref.info["cy0"], ref.info["width"], ref.info["height"]) == (80000, -80000, 140, 60)
    near = xyz - np.array([40000.0, -40000.0, 0.0], F32)  # an exact translation by whole cells: the same outcome
    assert_same(run(gctx, _pts(near), 0.5, max_window_radius=16, fill_radius=3)[:4] + (got[4],), ref, "translated back")


@pytest.mark.gpu
def test_sixteen_linear_iterations(gctx):
    xyz = random_cells(150, 37, seed=13)
    got, ref = check(gctx, xyz, 0.5, max_window_radius=16, window_base=1, exponential=False, slope=0.1)
    assert ref.info["n_iterations"] == 16 and sum(1 for v in ref.info["n_removed"] if v) >= 5
    got, ref = check(gctx, xyz, 0.5, max_window_radius=128, window_base=1, exponential=False, slope=0.1)  # the schedule stops at 16
    assert ref.info["n_iterations"] == 16


@pytest.mark.gpu
def test_device_tensors_repeated_calls_and_optional_outputs(gctx):
    import torch
    from online_3d_reconstruction_amd import _lib
    xyz = random_cells(300, 41, seed=21)
    p = _pts(xyz)
    kw = dict(max_window_radius=32, fill_radius=6)
    ref = gr.ground_filter(xyz, 0.5, **kw)
    first = run(gctx, p, 0.5, **kw)
    assert_same(first, ref)
    dev = torch.from_numpy(p.view(np.int32).reshape(-1, 4).copy()).cuda()
    for _ in range(2):
        again, on_dev = run(gctx, p, 0.5, **kw), run(gctx, dev, 0.5, **kw)
        assert all(t.is_cuda for t in on_dev[:4]) and on_dev[0].dtype == torch.uint8 and on_dev[2].dtype == torch.float32
        assert_same(on_dev, ref, "device tensors")
        for a, b in zip(first[:4], again[:4]):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        assert first[4] == again[4] == on_dev[4]
    # every output pointer may be NULL: the point pass still sees the DTM and the states
    only = gctx.groundFilter(p, 0.5, **kw)
    assert isinstance(only, np.ndarray) and np.array_equal(only, ref.ground)
    hag, info = gctx.groundFilter(p, 0.5, return_height=True, return_info=True, **kw)[1:]
    assert np.array_equal(hag.view(np.uint32), ref.height_above_ground.view(np.uint32)) and dict(info.__dict__) == ref.info
    L = _lib.load_library()
    prm = _lib.GroundParamsStruct()
    L.o3dr_ground_default_params(C.byref(prm))
    prm.cell_size, prm.max_window_radius, prm.fill_radius = 0.5, 32, 6
    prm.cx0, prm.cy0, prm.width, prm.height = (ref.info[k] for k in ("cx0", "cy0", "width", "height"))
    res = _lib.GroundResultStruct()
    _lib.check(L.o3dr_ground_filter(gctx._h, p.ctypes.data, len(p), C.byref(prm), None, C.byref(res), 0))
    assert (res.n_ground_cells, res.n_ground_points, res.n_dtm_filled) == tuple(ref.info[k] for k in ("n_ground_cells", "n_ground_points", "n_dtm_filled"))
    _lib.check(L.o3dr_ground_filter(gctx._h, p.ctypes.data, len(p), C.byref(prm), None, None, 0))


@pytest.mark.gpu
def test_errors_in_the_contracts_order(gctx):
    import torch

    from online_3d_reconstruction_amd import O3drError, _lib
    xyz = random_cells(20, 10, seed=2)
    p = _pts(xyz)
    bad = p.copy()
    bad["y"][7] = np.nan
    far = _pts(np.array([[0.0, 0.0, 0.0], [1e12, 0.0, 0.0]], F32))
    box = (0, 0, 20, 10)

    def fails(text, pts=p, cell=0.5, **kw):
        with pytest.raises(O3drError) as e:
            gctx.groundFilter(pts, cell, **{"bounds": box, **kw})
        assert e.value.code == ERR_INVALID_ARG and text in str(e.value), (text, str(e.value))

    # every parameter in the struct's order, each with the later ones bad too; then the cloud; then the box's size
    later = [("cell_size", dict(cell=0.0)), ("width, height", dict(bounds=(0, 0, 0, 5))), ("max_window_radius", dict(max_window_radius=129)),
             ("window_base", dict(window_base=1)), ("slope", dict(slope=np.nan)), ("initial_distance", dict(initial_distance=-1.0)),
             ("max_distance", dict(max_distance=np.inf)), ("fill_radius", dict(fill_radius=33))]
    for i, (text, kw) in enumerate(later):
        merged = {}
        for _, k in later[i:][::-1]:
            merged.update(k)
        fails(text, pts=bad, **merged)
        fails(text, **kw)
    for cell in (-0.5, np.nan, np.inf, 1e-60):
        fails("cell_size", cell=cell)
    fails("width, height", bounds=(0, 0, 5, -1))
    fails("int32", bounds=(2 ** 31 - 4, 0, 5, 1))
    fails("max_window_radius", max_window_radius=0)
    fails("window_base", window_base=0, exponential=False)
    fails("fill_radius", fill_radius=-1)
    fails("no iteration", window_base=17, exponential=False, pts=bad)
    fails("non-finite", pts=bad)
    fails("non-finite", pts=bad, bounds=(0, 0, 1 << 14, (1 << 14) + 1))
    fails("int32", pts=far)
    free0 = torch.cuda.mem_get_info()[0]
    fails("2^28", bounds=(0, 0, (1 << 28) + 1, 1))  # refused before anything of that size is allocated
    fails("2^28", bounds=(0, 0, 1 << 14, (1 << 14) + 1))
    assert free0 - torch.cuda.mem_get_info()[0] < (256 << 20)
    with pytest.raises(O3drError) as e:  # n = 0 without a box
        gctx.groundFilter(np.zeros(0, p.dtype), 0.5)
    assert e.value.code == ERR_INVALID_ARG and "empty cloud" in str(e.value)
    # a failed host call leaves zeroed outputs and a zeroed result, and the context still works
    L = _lib.load_library()
    prm = _lib.GroundParamsStruct()
    L.o3dr_ground_default_params(C.byref(prm))
    prm.cell_size, prm.fill_radius, prm.width, prm.height = 0.5, 33, 20, 10
    ground, hag = np.full(len(p), 3, np.uint8), np.full(len(p), 3, F32)
    dtm, state = np.full((10, 20), 3, F32), np.full((10, 20), 3, np.uint8)
    res = _lib.GroundResultStruct()
    res.width, res.n_removed[0] = 5, 5
    outs = _lib.GroundOutputsStruct(ground.ctypes.data, hag.ctypes.data, dtm.ctypes.data, state.ctypes.data)
    assert L.o3dr_ground_filter(gctx._h, p.ctypes.data, len(p), C.byref(prm), C.byref(outs), C.byref(res), 0) == ERR_INVALID_ARG
    assert not ground.any() and not hag.any() and not dtm.any() and not state.any() and res.width == 0 and res.n_removed[0] == 0
    prm.fill_radius = 0
    assert L.o3dr_ground_filter(gctx._h, p.ctypes.data, len(p), C.byref(prm), C.byref(outs), C.byref(res), 7) == ERR_INVALID_ARG  # mem kind
    assert L.o3dr_ground_filter(gctx._h, None, len(p), C.byref(prm), C.byref(outs), C.byref(res), 0) == ERR_INVALID_ARG
    assert L.o3dr_ground_filter(gctx._h, p.ctypes.data, len(p), None, C.byref(outs), C.byref(res), 0) == ERR_INVALID_ARG
    check(gctx, xyz, 0.5, fill_radius=2)


# ---- scratch: the check tests/test_scratch_independence.py makes of the entry points of include/o3dr.h -------------------------
SCRATCH = {"small": (67, 35, dict(max_window_radius=16, fill_radius=3)), "large": (300, 141, dict(max_window_radius=128, fill_radius=3))}


def scratch_call(ctx, size):
    w, h, kw = SCRATCH[size]
    return run(ctx, _pts(random_cells(w, h, seed=w)), 0.5, **kw)


@pytest.mark.gpu
def test_result_does_not_depend_on_old_scratch_contents():
    from test_scratch_independence import blob, fill, hooked_context
    want = {}
    for size, (w, h, kw) in SCRATCH.items():
        with hooked_context() as ctx:
            outs = scratch_call(ctx, size)
        assert_same(outs, gr.ground_filter(random_cells(w, h, seed=w), 0.5, **kw), f"scratch {size}")
        want[size] = blob(outs)
    with hooked_context() as ctx:
        first = blob(scratch_call(ctx, "small"))
        n_ff = fill(ctx, 0xFF)
        after_ff = blob(scratch_call(ctx, "small"))
        n_00 = fill(ctx, 0x00)
        after_00 = blob(scratch_call(ctx, "small"))
        large = blob(scratch_call(ctx, "large"))
        after_large = blob(scratch_call(ctx, "small"))
        large_again = blob(scratch_call(ctx, "large"))
    assert n_ff > 0 and n_00 > 0
    assert first == want["small"], "the same call on two new contexts"
    assert after_ff == want["small"], "after 0xFF over the scratch"
    assert after_00 == want["small"], "after 0x00 over the scratch"
    assert large == want["large"] and large_again == want["large"], "large after small"
    assert after_large == want["small"], "small after a larger call of itself"
