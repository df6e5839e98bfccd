"""The three map operators (Context.clusterCloud, rasterizeMap, groundFilter) past their launch caps, bit for bit against
the numpy references the small-cloud modules use (cluster_reference with its KD-tree pair search, raster_reference,
ground_reference):
  - more than 262 144 points: the grid-stride loops of k_raster_winner and k_ground_points take a second trip, the
    workgroups' trip counts differ, and k_fold4_u32 folds the partials of 1024 such workgroups;
  - more than 4096 row blocks in the ground filter's column passes: k_ground_col_suffix and k_ground_col_window reach the
    blocks past the grid by B += stride;
  - one component of 300 800 points in random index order (1175 linking workgroups on one union-find), and more than
    16 384 clusters (the third radix pass of `indices`).
Every test first asserts, from the reference or the launch arithmetic alone, that its scene reaches the path it names."""
import functools

import numpy as np
import pytest

import cluster_reference as cr
import ground_reference as gr
import raster_reference as rr
from test_cluster_cloud import assert_same as cluster_same
from test_cluster_cloud import run as cluster_run
from test_ground_filter import assert_same as ground_same
from test_ground_filter import random_cells
from test_ground_filter import run as ground_run
from test_rasterize_map import LIGHT, _pts, grid_cloud
from test_rasterize_map import assert_same as raster_same
from test_search_grid_stress import OFFSETS, map_like, on_grid, translated

F32 = np.float32
POINT_CAP = 262144     # kCellRangeBlocks * 256 (o3dr_device.h): from here cell_range_parts(n) stays at 1024 workgroups
ROW_BLOCK_CAP = 4096   # kGroundColRowsMax (o3dr_device.h): the row blocks a column pass spreads over workgroups at most
RADIX_BITS = 7         # kMaxRadixBits: launch_sort_keys takes ceil(nbits / 7) passes
CLUSTER_THREADS = 256  # kClusterThreads: points per workgroup of k_cluster_link


def col_blocks(height, r):
    """ground_col_rows (o3dr_device.h) before its cap: the blocks of 2r + 1 rows and the one before row 0"""
    return (height + 2 * r) // (2 * r + 1) + 1


@pytest.fixture(scope="module")
def sctx():
    import online_3d_reconstruction_amd as o3dr
    with o3dr.Context(0) as c:
        yield c


# ---- clustering ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def map_cloud():
    """300 800 points on the 2^-10 m grid, one per 0.05 m cell, in random index order (treat as read-only)"""
    xyz = map_like(640, 470, seed=3)
    xyz.setflags(write=False)
    return xyz


@functools.lru_cache(maxsize=None)
def map_result(tolerance, min_size=1, max_size=cr.MAX_SIZE, head=None, offset=OFFSETS[0]):
    """the reference on (the first `head` points of) the map cloud moved by `offset`, once per parameter set (read-only)"""
    return cr.cluster(translated(map_cloud()[:head], offset), tolerance, min_size, max_size, pairs="tree")


def radix_passes(n_clusters):
    """the passes launch_cluster_outputs sorts with: the keys are 0 .. n_clusters"""
    return -(-int(n_clusters).bit_length() // RADIX_BITS)


@pytest.mark.gpu
def test_one_component_of_the_whole_map_in_random_index_order(sctx):
    """every point ends under root 0 through links made by 1175 workgroups at once; with max_size = n - 1 the one
    component is rejected and nothing is left to number, sort or record"""
    xyz = map_cloud()
    n = len(xyz)
    ref = map_result(0.1)
    assert n == 300800 and -(-n // CLUSTER_THREADS) > 1000
    assert ref.info["n_components"] == 1 and ref.info["largest"] == n and ref.info["n_pairs"] > 5 * n
    assert len(ref.clusters) == 1 and len(ref.indices) == n and not ref.raw.any()
    cluster_same(cluster_run(sctx, _pts(xyz), 0.1), ref, "one component")
    none = map_result(0.1, 1, n - 1)
    assert none.info["n_too_large"] == 1 and none.info["n_clusters"] == 0 and len(none.clusters) == 0 and len(none.indices) == 0
    assert (none.label == -1).all() and none.info["n_rejected_points"] == n
    cluster_same(cluster_run(sctx, _pts(xyz), 0.1, min_size=1, max_size=n - 1), none, "rejected as too large")


@pytest.mark.gpu
@pytest.mark.parametrize("min_size", [2, 1])
def test_more_than_16384_clusters_take_the_third_radix_pass(sctx, min_size):
    """min_size 2: the rejected points carry the key n_clusters through the three passes and are cut off `indices`;
    min_size 1: every point is in `indices`.  (A fourth pass needs 2^21 clusters: out of this module's scope.)"""
    xyz = map_cloud()
    ref = map_result(0.045, min_size)
    assert ref.info["n_clusters"] >= 16384 and radix_passes(ref.info["n_clusters"]) == 3
    assert ref.info["n_components"] > ref.info["n_clusters"] or min_size == 1
    if min_size == 2:
        assert ref.info["n_too_small"] > 0 and len(ref.indices) < len(xyz) and ref.info["largest"] > 2
    else:
        assert ref.info["n_too_small"] == 0 and len(ref.indices) == len(xyz) and ref.info["n_clusters"] == ref.info["n_components"]
    cluster_same(cluster_run(sctx, _pts(xyz), 0.045, min_size=min_size), ref, f"min_size {min_size}")


@pytest.mark.gpu
def test_clusters_do_not_change_under_exact_translations(sctx):
    """the first 40 000 points at (1024, -1024) and (-8192, 8192): every fp32 difference, and with it every link, is the
    untranslated cloud's.  The records are compared with their own reference only: the centroid adds `lo` in fp64."""
    head = 40000
    xyz = map_cloud()[:head]
    assert np.array_equal(on_grid(xyz), xyz)
    base_ref = map_result(0.1, head=head)
    assert base_ref.info["n_components"] > 1000 and base_ref.info["largest"] > 8 and base_ref.info["n_pairs"] > 10000
    base = cluster_run(sctx, _pts(xyz), 0.1)
    cluster_same(base, base_ref, OFFSETS[0])
    for off in OFFSETS[1:]:
        moved = translated(xyz, off)
        assert np.array_equal(moved[:, :2].astype(np.float64), xyz[:, :2].astype(np.float64) + np.asarray(off))
        got = cluster_run(sctx, _pts(moved), 0.1)
        cluster_same(got, map_result(0.1, head=head, offset=off), off)
        for k, name in ((0, "label"), (2, "raw"), (3, "size"), (4, "indices")):
            assert np.array_equal(got[k], base[k]), (off, name)
        assert got[5].n_pairs == base[5].n_pairs and got[5] == base[5], off


@pytest.mark.gpu
def test_the_one_component_again_and_from_device_memory(sctx):
    import torch
    p = _pts(map_cloud())
    ref = map_result(0.1)
    assert ref.info["n_components"] == 1 and len(p) > POINT_CAP
    dev = torch.from_numpy(p.view(np.int32).reshape(-1, 4).copy()).cuda()
    first, again, on_dev = cluster_run(sctx, p, 0.1), cluster_run(sctx, p, 0.1), cluster_run(sctx, dev, 0.1)
    assert all(t.is_cuda for t in on_dev[:5])
    cluster_same(first, ref, "first")
    cluster_same(on_dev, ref, "device tensors")
    for a, b, d in zip(first[:5], again[:5], on_dev[:5]):
        assert a.tobytes() == b.tobytes() == d.cpu().numpy().tobytes()
    assert first[5] == again[5] == on_dev[5]


# ---- raster and ground filter past 262 144 points -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def raster_cloud():
    xyz = grid_cloud(640, 420, holes=0.3, seed=5, extra=100000)
    xyz.setflags(write=False)
    return xyz


@pytest.mark.gpu
@pytest.mark.parametrize("select", ["first", "top", "bottom"])
def test_raster_of_more_points_than_the_winner_pass_has_threads(sctx, select):
    xyz = raster_cloud()
    p = _pts(xyz)
    assert len(xyz) > POINT_CAP and len(xyz) < 2 * POINT_CAP  # some threads take two points, the others one
    ref = rr.rasterize(xyz, p["rgba"], 0.05, select=select, fill_radius=3, light=LIGHT)
    assert ref.info["n_inside"] == len(xyz) and ref.info["n_shadowed"] >= 100000 and ref.info["n_filled"] > 0
    got = sctx.rasterizeMap(p, 0.05, select=select, fill_radius=3, light=LIGHT, return_source=True, return_distance=True, return_info=True)
    raster_same(got, ref, select)
    if select == "first":
        assert (ref.source[ref.distance2 == 0] >= POINT_CAP).sum() > 1000  # cells won by a point of the second trip


@pytest.mark.gpu
def test_raster_box_smaller_than_the_cloud_and_the_extent(sctx):
    xyz = raster_cloud()
    p = _pts(xyz)
    assert len(xyz) > POINT_CAP
    assert sctx.rasterExtent(p, 0.05) == rr.extent(xyz, 0.05) == (0, 0, 640, 420)
    box = (37, 11, 500, 333)
    ref = rr.rasterize(xyz, p["rgba"], 0.05, bounds=box, select="top", fill_radius=3, light=LIGHT)
    cx, cy = rr.cells_of(xyz[POINT_CAP:], 0.05)
    out = (cx < box[0]) | (cx >= box[0] + box[2]) | (cy < box[1]) | (cy >= box[1] + box[3])
    assert out.any() and not out.all() and ref.info["n_outside"] > out.sum() > 0  # both counts grow on the second trip
    got = sctx.rasterizeMap(p, 0.05, bounds=box, select="top", fill_radius=3, light=LIGHT, return_source=True, return_distance=True,
                           return_info=True)
    raster_same(got, ref, "smaller box")


@pytest.mark.gpu
def test_ground_filter_of_more_points_than_the_point_pass_has_threads(sctx):
    rng = np.random.default_rng(10)
    base = random_cells(640, 420, seed=9, occupancy=0.7)
    up = base[rng.integers(0, len(base), 90000)].copy()
    up[:, 2] += rng.uniform(0.0, 0.3, len(up)).astype(F32)
    xyz = np.concatenate([base, up])[rng.permutation(len(base) + len(up))]
    kw = dict(max_window_radius=8, slope=0.02, initial_distance=0.15, max_distance=10.0, fill_radius=2)
    ref = gr.ground_filter(xyz, 0.5, **kw)
    assert len(xyz) > POINT_CAP and ref.info["n_inside"] == len(xyz)
    assert ref.info["n_ground_points"] > ref.info["n_ground_cells"] > 0 and ref.ground[POINT_CAP:].any() and not ref.ground[POINT_CAP:].all()
    assert ref.info["n_iterations"] == 4 and all(ref.info["n_removed"][:4])
    ground_same(ground_run(sctx, _pts(xyz), 0.5, **kw), ref, "second trip of the point pass")


# ---- ground filter past 4096 row blocks -----------------------------------------------------------------------------------
BOX = dict(fill_radius=2)  # with cell 0.5


def tall_box(sctx, w, h, seed, max_window_radius, blocks):
    """random_cells(w, h) at half occupancy through groundFilter with the box given (the cloud's own extent can be a row
    short); `blocks`: the block count of ground_col_rows per radius, asserted before anything runs"""
    radii = gr.schedule(0.5, max_window_radius)[0].tolist()
    assert [col_blocks(h, r) for r in radii] == list(blocks)
    xyz = random_cells(w, h, seed=seed, occupancy=0.5)
    kw = dict(bounds=(0, 0, w, h), max_window_radius=max_window_radius, **BOX)
    ref = gr.ground_filter(xyz, 0.5, **kw)
    assert ref.cell_state.shape == (h, w) and ref.info["n_iterations"] == len(radii)
    assert all(ref.info["n_removed"][:len(radii)]), ref.info["n_removed"]
    ground_same(ground_run(sctx, _pts(xyz), 0.5, **kw), ref, f"{w} x {h}")
    return ref


@pytest.mark.gpu
def test_ground_column_passes_stride_over_10001_row_blocks(sctx):
    """3 x 30 000 cells: a workgroup takes two or three blocks at r = 1, one or two at r = 2, one at r = 4"""
    blocks = (10001, 6001, 3335)
    assert blocks[0] > 2 * ROW_BLOCK_CAP and 2 * ROW_BLOCK_CAP > blocks[1] > ROW_BLOCK_CAP > blocks[2]
    tall_box(sctx, 3, 30000, 3, 4, blocks)


@pytest.mark.gpu
def test_ground_column_passes_stride_in_two_column_groups(sctx):
    """257 x 16 000 cells: 2 x 4096 workgroups at r = 1, blockIdx.x % groups_x the column group and / groups_x the block"""
    blocks = (5335, 3201, 1779)
    assert blocks[0] > ROW_BLOCK_CAP > blocks[1] and -(-257 // 256) == 2
    tall_box(sctx, 257, 16000, 257, 4, blocks)


@pytest.mark.gpu
@pytest.mark.parametrize("h,blocks", [(12285, 4096), (12286, 4097), (12287, 4097), (12289, 4098)])
def test_ground_column_passes_around_the_first_strided_block(sctx, h, blocks):
    """3 cells wide, radius 1 alone.  12 285 rows are the most with one block per workgroup (4096 blocks: the cap itself);
    at 12 286 the count passes the cap, the grid stays at 4096 and workgroup 0 looks for a second block that both kernels'
    loops find past the raster; at 12 287 the window pass has it (block 4095 starts at row 12 286), at 12 289 the suffix
    pass too (block 4096 starts at row 12 288)"""
    assert (blocks > ROW_BLOCK_CAP) == (h > 12285)
    window_second = (ROW_BLOCK_CAP - 1) * 3 + 1 < h   # k_ground_col_window: B = b0 - 1 + 4096 for b0 = 0
    suffix_second = ROW_BLOCK_CAP * 3 < h             # k_ground_col_suffix: B = b0 + 4096 for b0 = 0
    assert (window_second, suffix_second) == {12285: (False, False), 12286: (False, False), 12287: (True, False), 12289: (True, True)}[h]
    tall_box(sctx, 3, h, 3, 1, (blocks,))
