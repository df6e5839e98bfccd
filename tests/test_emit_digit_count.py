"""The batched call when the emit pass counts the first radix digit itself (k_reproject_emit<.., KEYS> with `hist`): the
first pass of every per-frame sort then runs over CANDIDATE-ALIGNED tiles - sort tile t = the records of emit tiles
[8 t, 8 t + 8), each scatter part = four emit tiles - whose record ranges come from the scanned valid counts.  The inputs
below are the ones that addressing can get wrong: tiles far below 8192 records, parts without any record, a last tile
of one record, all-invalid frames anywhere in the batch, a pass-through frame (PCL's overflow guard, no sort) next to a
sorted one.  Bar: cloud_big and the merged cloud bit for bit against the CPU oracle."""
import numpy as np
import pytest

from conftest import assert_points_equal

pytestmark = pytest.mark.gpu

ROWS, COLS = 360, 640  # 320 x 540 candidates at jump 1: 169 emit tiles, 22 sort tiles (the last one: a single emit tile)


def _params(**kw):
    import online_3d_reconstruction_amd as o3dr
    kw.setdefault("sor_enable", False)
    return o3dr.Params(**kw)


def _roi(disp, jump=1):
    """the grid pass's candidates of a frame, as a view (bounding box 20, column start cols / 8)"""
    rows, cols = disp.shape[-2:]
    return disp[..., 20:rows - 20:jump, cols // 8:cols - 20:jump]


def _frames(start, F, invalid_frac, rows=ROWS, cols=COLS):
    from online_3d_reconstruction_amd import synth
    disp, bgr = synth.make_frames(start, F, rows, cols, invalid_frac=invalid_frac)
    return disp, bgr, synth.make_poses(start, F), synth.camera_Q(rows, cols)


def _oracle_run(orc, Q, disp, bgr, poses, vs, jump, minpts):
    clouds, sts = [], []
    for i in range(len(disp)):
        pts, st = orc.create_and_transform_pt_cloud(disp[i], bgr[i], Q, poses[i], vs, jump_pixels=jump)
        clouds.append(pts)
        sts.append(st)
    big = np.concatenate(clouds)
    small, _ = orc.downsample_pt_cloud(big, vs, True, minpts)
    return big, small, sts, [len(c) for c in clouds]


def _check(orc, Q, disp, bgr, poses, what, vs=0.05, jump=1, minpts=1):
    """the batched call (one call, HBM-resident path through host arrays) against the oracle; returns the oracle's
    per-frame statuses and sizes"""
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    with o3dr.Context(0, Q=Q, params=_params(jump_pixels=jump, voxel_size=vs, min_points_per_voxel=minpts)) as c:
        c.profileEnable(L.K_SORT_HIST)
        c.accumulateFrames(disp, bgr, poses)
        # the path under test was taken: one launch group of five passes, the first of them without a histogram launch
        # (five launches where k_radix_hist still counts the first digit)
        assert c.profileRead(L.K_SORT_HIST)[1] == 4, "the emit pass did not count the first digit"
        c.profileEnable(L.K_SORT_HIST, False)
        big = c.cloudBigRead()
        small = c.finalize()
    rbig, rsmall, sts, sizes = _oracle_run(orc, Q, disp, bgr, poses, vs, jump, minpts)
    assert_points_equal(big, rbig, f"{what}: cloud_big")
    assert_points_equal(small, rsmall, f"{what}: merged cloud")
    return sts, sizes


@pytest.mark.parametrize("invalid_frac", [0.0, 0.3, 0.97])
def test_invalid_fractions(orc, invalid_frac):
    """dense frames (candidate-aligned = record-aligned tiles), 30 % invalid (every part starts off a 16-byte boundary),
    97 % invalid (about 250 records per sort tile)"""
    disp, bgr, poses, Q = _frames(10, 3, invalid_frac)
    _, sizes = _check(orc, Q, disp, bgr, poses, f"invalid_frac {invalid_frac}")
    assert min(sizes) > 0


def test_full_size_frames_30_percent_invalid(orc):
    """the headline frame size (92 sort tiles per frame, the last one of three emit tiles)"""
    disp, bgr, poses, Q = _frames(20, 2, 0.3, 720, 1280)
    _check(orc, Q, disp, bgr, poses, "720p, invalid_frac 0.3")


def test_last_tile_of_one_record_and_empty_parts(orc):
    """frame 0: the last sort tile holds ONE record (its last candidate); frame 1: only the first and the last candidate
    of the frame are valid (two one-record tiles, twenty empty ones between them); frame 2: a whole sort tile's worth of
    candidates invalid in the middle of the frame, and a second part without records elsewhere"""
    disp, bgr, poses, Q = _frames(30, 3, 0.1)
    n_cand = _roi(disp[0]).size
    assert n_cand == 172800 and -(-n_cand // 8192) == 22
    for f in range(3):
        roi = _roi(disp[f])
        flat = roi.reshape(-1).copy()  # (the view is not contiguous)
        if f == 0:
            flat[21 * 8192:] = 0
            flat[-1] = 100
        elif f == 1:
            flat[:] = 0
            flat[0] = 90
            flat[-1] = 100
        else:
            flat[5 * 8192:6 * 8192] = 0
            flat[9 * 8192 + 4096:10 * 8192] = 0
        roi[...] = flat.reshape(roi.shape)
    _, sizes = _check(orc, Q, disp, bgr, poses, "one-record tiles")
    assert sizes[1] == 2


def test_all_invalid_frames_first_middle_last_min_points_3(orc):
    """seven frames (not a multiple of anything the kernels tile by), frames 0, 3 and 6 without a valid pixel; the merge
    keeps voxels of at least 3 points"""
    disp, bgr, poses, Q = _frames(40, 7, 0.05)
    for f in (0, 3, 6):
        disp[f] = 0
    _, sizes = _check(orc, Q, disp, bgr, poses, "all-invalid frames", minpts=3)
    assert [s == 0 for s in sizes] == [True, False, False, True, False, False, True]


@pytest.mark.parametrize("invalid_frac", [0.0, 0.3])
def test_jump_pixels_4(orc, invalid_frac):
    """jump_pixels 4 without keypoints takes the same path through the generic (non-vectorised) pixel loads:
    170 x 275 candidates, 46 emit tiles, 6 sort tiles"""
    disp, bgr, poses, Q = _frames(50, 5, invalid_frac, 720, 1280)
    _check(orc, Q, disp, bgr, poses, f"jump 4, invalid_frac {invalid_frac}", jump=4)


def test_overflow_frame_next_to_sorted_frames(orc):
    """voxel_size 0.019: a full frame's per-frame grid trips PCL's overflow guard (the frame passes through, no sort
    passes); a frame that only keeps a window of near pixels has a small box and is sorted.  Order: sorted, pass-through,
    sorted, pass-through."""
    disp, bgr, poses, Q = _frames(60, 4, 0.02, 720, 1280)
    for f in (0, 2):
        keep = np.zeros(disp[f].shape, bool)
        keep[300:420, 500:760] = True
        near = disp[f] >= np.percentile(disp[f][300:420, 500:760], 50)
        disp[f][~(keep & near)] = 0
    sts, sizes = _check(orc, Q, disp, bgr, poses, "overflow next to sorted", vs=0.019, minpts=3)
    assert [s != 0 for s in sts] == [False, True, False, True] and orc.STATUS_VOXEL_OVERFLOW in sts
    assert min(sizes) > 0
