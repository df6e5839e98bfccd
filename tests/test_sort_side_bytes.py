"""The last scatter pass of a point sort leaves, instead of the sorted indices, one byte per record that says whether
the record starts a run of equal indices (Workspace::side): decided inside the part's sorted order, and for the first
record of a digit by a look-back over the input before the part; k_side_heads packs those bytes for k_run_starts, and
k_run_heads' pass over the sorted indices is gone.  A wrong flag moves a run border, so the bar is the usual one -
cloud_big, the merged cloud and stand-alone voxel grids bit for bit against the CPU oracle - plus the device counter
that says the path ran (o3dr_profile_stats out[5]: records flagged by their last pass = every record of a point
sort).  Inputs: batched frames whose first pass runs over candidate-aligned tiles (parts that start off 16-byte
boundaries, tiles of a few hundred records, a pass-through frame between sorted ones), a cloud built so that runs of
equal indices and changes of the top digit straddle a part border of the last pass, and one to five passes over part and
tile borders (with one pass the look-back runs across whole parts)."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_points_equal

pytestmark = pytest.mark.gpu

ROWS, COLS = 360, 640  # 320 x 540 candidates at jump 1: 169 emit tiles, 22 sort tiles (tests/test_emit_digit_count.py)


def _params(**kw):
    import online_3d_reconstruction_amd as o3dr
    kw.setdefault("sor_enable", False)
    return o3dr.Params(**kw)


def _frames(start, F, invalid_frac, rows=ROWS, cols=COLS):
    from online_3d_reconstruction_amd import synth
    disp, bgr = synth.make_frames(start, F, rows, cols, invalid_frac=invalid_frac)
    return disp, bgr, synth.make_poses(start, F), synth.camera_Q(rows, cols)


def _side_stats(c):
    """(record-passes, records, records flagged by their last pass) since the context was made"""
    s = c.profileStatsAll()
    return s[0], s[4], s[5]


def _check_batched(orc, Q, disp, bgr, poses, what, vs=0.05, minpts=1):
    import online_3d_reconstruction_amd as o3dr
    with o3dr.Context(0, Q=Q, params=_params(jump_pixels=1, voxel_size=vs, min_points_per_voxel=minpts)) as c:
        c.accumulateFrames(disp, bgr, poses)
        _rec_passes, recs, flagged = _side_stats(c)
        big = c.cloudBigRead()
        small = c.finalize()
    clouds, sts = [], []
    for i in range(len(disp)):
        pts, st = orc.create_and_transform_pt_cloud(disp[i], bgr[i], Q, poses[i], vs, jump_pixels=1)
        clouds.append(pts)
        sts.append(st)
    rbig = np.concatenate(clouds)
    rsmall, _ = orc.downsample_pt_cloud(rbig, vs, True, minpts)
    assert flagged == recs > 0, (what, recs, flagged)  # (per-frame sorts are point sorts)
    assert_points_equal(big, rbig, f"{what}: cloud_big")
    assert_points_equal(small, rsmall, f"{what}: merged cloud")
    return sts


@pytest.mark.parametrize("invalid_frac", [0.0, 0.3, 0.97])
def test_batched_frames(orc, invalid_frac):
    """dense frames, 30 % invalid (candidate-aligned parts start off 16-byte boundaries), 97 % invalid (about 250 records
    per sort tile)"""
    disp, bgr, poses, Q = _frames(110, 3, invalid_frac)
    _check_batched(orc, Q, disp, bgr, poses, f"invalid_frac {invalid_frac}")


def test_batched_frames_min_points_3(orc):
    disp, bgr, poses, Q = _frames(120, 3, 0.3)
    _check_batched(orc, Q, disp, bgr, poses, "min_points 3", minpts=3)


def test_pass_through_frame_between_sorted_frames(orc):
    """voxel_size 0.019: a full 720p frame trips PCL's overflow guard and passes through without a sort; the frames
    around it keep a window of near pixels and are sorted"""
    disp, bgr, poses, Q = _frames(130, 3, 0.02, 720, 1280)
    for f in (0, 2):
        keep = np.zeros(disp[f].shape, bool)
        keep[300:420, 500:760] = True
        near = disp[f] >= np.percentile(disp[f][300:420, 500:760], 50)
        disp[f][~(keep & near)] = 0
    sts = _check_batched(orc, Q, disp, bgr, poses, "pass-through between sorted", vs=0.019, minpts=3)
    assert [s != 0 for s in sts] == [False, True, False] and orc.STATUS_VOXEL_OVERFLOW in sts


# ---- stand-alone voxel grids over clouds whose indices are placed by hand -------------------------------------------------

def _cloud_from_cells(cells, leaf, seed):
    """one point per row of `cells` (ix, iy, iz), at a random place well inside its cell, with a random colour"""
    from oracle.orc import POINT
    rng = np.random.default_rng(seed)
    p = np.empty(len(cells), POINT)
    for k, ax in enumerate("xyz"):
        p[ax] = ((cells[:, k] + 0.2 + 0.6 * rng.random(len(cells))) * np.float64(leaf[k])).astype(np.float32)
    p["rgba"] = rng.integers(0, 1 << 24, len(cells), dtype=np.uint32)
    return p


def _voxel_grid_check(orc, pts, leaf, passes, what, min_points_list=(0,)):
    import online_3d_reconstruction_amd as o3dr
    for mp in min_points_list:
        with o3dr.Context(0, params=_params()) as c:
            got, st = c.voxelGrid(pts, leaf, min_points=mp, return_status=True)
            stats = _side_stats(c)
        want, rst = orc.voxel_grid(pts, leaf, mp)
        assert st == rst == 0, what
        assert stats == (len(pts) * passes, len(pts), len(pts)), (what, stats)
        assert_points_equal(got, want, f"{what}, min_points {mp}")


def test_run_boundaries_across_a_part_border_of_the_last_pass(orc):
    """1024 x 512 x 512 cells at leaf 0.01: 28-bit indices, four 7-bit passes, top digit = iz >> 2.  In the input of the
    last pass (sorted by the low 21 bits): 36 points of one (ix, iy, iz & 3) with top digits 5,5,9,5,9,9,7,5,7,9,5,5 (x3)
    at places 12282..12317 - across the part border at 12288 - and behind them 8292 points of ONE voxel, over parts 3..5."""
    leaf = (0.01, 0.01, 0.01)
    n_fill, n_one = 3 * 4096 - 7, 8292
    tops = [5, 5, 9, 5, 9, 9, 7, 5, 7, 9, 5, 5] * 3
    rng = np.random.default_rng(7)
    j = np.arange(1, n_fill + 1)
    cells = [np.array([[0, 0, 0]]),
             np.stack([j & 1023, j >> 10, 4 * rng.integers(0, 128, n_fill)], axis=1),  # distinct low bits 1..n_fill
             np.array([[5, 20, 4 * t + 1] for t in tops]),
             np.tile([[7, 30, 4 * 64 + 2]], (n_one, 1)),
             np.array([[1023, 511, 511]])]
    cells = np.concatenate(cells)
    n = len(cells)
    assert n == 20611
    # shuffled input; the 36 points keep their relative order (a stable sort shows them to the last pass in this order)
    place = rng.permutation(n)
    grp = np.arange(1 + n_fill, 1 + n_fill + len(tops))
    place[grp] = np.sort(place[grp])
    pts = np.empty_like(_cloud_from_cells(cells, leaf, 8))
    pts[place] = _cloud_from_cells(cells, leaf, 8)
    # what the construction is for, checked on the oracle's own indices
    keys, _min_b, div_b, st = orc.voxel_keys(pts, leaf)
    assert st == 0 and list(div_b) == [1024, 512, 512]
    seq = keys[np.argsort(keys & ((1 << 21) - 1), kind="stable")]
    mid = seq[12282:12318]
    assert list(mid >> 21) == tops and len(set(mid & ((1 << 21) - 1))) == 1 and 12282 < 3 * 4096 < 12317
    assert len(set(seq[12318:20610])) == 1 and seq[12317] != seq[12318] and seq[20609] != seq[20610]
    assert 12318 < 4 * 4096 < 5 * 4096 < 20609
    _voxel_grid_check(orc, pts, leaf, 4, "run boundaries", (0, 2))


# cells per axis whose product needs 7, 14, 21, 28 and 31 bits (more trips PCL's overflow guard): one to five passes
_GRIDS = {1: (8, 4, 4), 2: (32, 32, 16), 3: (128, 128, 128), 4: (1024, 512, 512), 5: (2048, 1024, 1023)}
_clouds = {}


def _pass_cloud(passes, n):
    """corner points that pin the grid, a few heavy voxels of thousands of points each (with one pass: the whole cloud
    is such voxels, and equal indices run across whole parts) and points spread over random cells, shuffled"""
    if (passes, n) not in _clouds:
        dims = np.array(_GRIDS[passes])
        leaf = (0.01, 0.02, 0.015)
        rng = np.random.default_rng(1000 * passes + n % 997)
        heavy = rng.integers(0, dims, (5, 3))
        n_heavy = n - 2 if passes == 1 else (n - 2) // 2
        cells = np.concatenate([np.zeros((1, 3), np.int64), (dims - 1)[None, :],
                                heavy[rng.integers(0, 5, n_heavy) if passes > 1 else np.sort(rng.integers(0, 5, n_heavy))],
                                rng.integers(0, dims, (n - 2 - n_heavy, 3))])
        pts = _cloud_from_cells(cells, leaf, n + passes)
        if passes > 1:
            pts = pts[rng.permutation(n)]
        _clouds[(passes, n)] = (pts, leaf, dims)
    return _clouds[(passes, n)]


@pytest.mark.parametrize("n", [8193, 12288, 12289, 16385])
@pytest.mark.parametrize("passes", [1, 2, 3, 4, 5])
def test_pass_counts(orc, passes, n):
    """sizes on part and tile borders and one past them (a last part of one record)"""
    pts, leaf, dims = _pass_cloud(passes, n)
    _keys, _min_b, div_b, st = orc.voxel_keys(pts, leaf)
    assert st == 0 and list(div_b) == list(dims)
    _voxel_grid_check(orc, pts, leaf, passes, f"{passes} passes, {n} points", (0, 2) if n == 12289 else (0,))


def test_gather_guard_on_a_batched_call(orc, monkeypatch):
    """no sorted indices are left behind the last pass; the guard of the gather reads the ids only and still turns a
    payload outside the frame into O3DR_ERR_INTERNAL, and the context goes on after a reset"""
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    monkeypatch.setenv("O3DR_TEST_HOOKS", "1")
    disp, bgr, poses, Q = _frames(140, 2, 0.1)
    with o3dr.Context(0, Q=Q, params=_params(jump_pixels=1, voxel_size=0.05)) as c:
        L.check(c._lib.o3dr_test_corrupt_next_gather(c._h))
        c.accumulateFrames(disp, bgr, poses)
        assert _side_stats(c)[2] > 0
        with pytest.raises(o3dr.O3drError) as e:
            c.cloudBigRead()
        assert e.value.code == L.ERR_INTERNAL
        c.cloudBigReset()
        c.accumulateFrames(disp, bgr, poses)  # the hook was one-shot
        big = c.cloudBigRead()
    want = np.concatenate([orc.create_and_transform_pt_cloud(disp[i], bgr[i], Q, poses[i], 0.05, jump_pixels=1)[0] for i in range(2)])
    assert_points_equal(big, want, "after the guard tripped")
