"""The batch path around its large kernels: the count pass that reads the disparities as 16-byte groups
(k_reproject_count_cbox, wide layout), the tile-count scan and the grid geometry in one launch (k_scan_counts_geom), the
exact-box pass behind the conservative box as a looping grid whose workgroups walk a frame's tiles, one kernel for the run
heads of both kinds of frame (k_run_heads), and what follows k_centroid (head flags between its waves, cloud_big's
running box), over several calls.

Bar: cloud_big and the merged cloud bit for bit against the CPU oracle; for the count pass also against a context that
always takes the exact box (O3DR_EXACT_BOX=1), for the running box against one that takes the box by a pass over the
cloud (O3DR_NO_CLOUD_BOX=1).  Shapes: ROI rows of 540 candidates (540 % 16 == 12: 16-candidate groups cross row ends,
last tile of 768 candidates), of 512 (no group crosses), of 1100 (720p); jump_pixels 4 keeps the dword loads."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_points_equal

pytestmark = pytest.mark.gpu


def _params(**kw):
    import online_3d_reconstruction_amd as o3dr
    kw.setdefault("sor_enable", False)
    return o3dr.Params(**kw)


def _roi(disp, jump=1):
    """the grid pass's candidates of a frame, as a view (bounding box 20, column start cols / 8)"""
    rows, cols = disp.shape[-2:]
    return disp[..., 20:rows - 20:jump, cols // 8:cols - 20:jump]


def _frames(start, F, invalid_frac, rows, cols):
    from online_3d_reconstruction_amd import synth
    disp, bgr = synth.make_frames(start, F, rows, cols, invalid_frac=invalid_frac)
    return disp, bgr, synth.make_poses(start, F), synth.camera_Q(rows, cols)


def _oracle_clouds(orc, Q, disp, bgr, poses, vs, jump):
    clouds, sts = [], []
    for i in range(len(disp)):
        pts, st = orc.create_and_transform_pt_cloud(disp[i], bgr[i], Q, poses[i], vs, jump_pixels=jump)
        clouds.append(pts)
        sts.append(st)
    return clouds, sts


def _gpu_run(monkeypatch, Q, disp, bgr, poses, vs, jump, minpts, env=None):
    """(cloud_big, merged cloud) of one batched call on a context of its own (the switches are read when it is made)"""
    import online_3d_reconstruction_amd as o3dr
    with monkeypatch.context() as mp:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        c = o3dr.Context(0, Q=Q, params=_params(jump_pixels=jump, voxel_size=vs, min_points_per_voxel=minpts))
    with c:
        c.accumulateFrames(disp, bgr, poses)
        return c.cloudBigRead(), c.finalize()


def _check(monkeypatch, orc, Q, disp, bgr, poses, what, vs=0.05, jump=1, minpts=1):
    """default context and exact-box context against the oracle; returns the oracle's statuses and per-frame sizes"""
    clouds, sts = _oracle_clouds(orc, Q, disp, bgr, poses, vs, jump)
    rbig = np.concatenate(clouds)
    rsmall, _ = orc.downsample_pt_cloud(rbig, vs, True, minpts)
    for env in (None, {"O3DR_EXACT_BOX": "1"}):
        big, small = _gpu_run(monkeypatch, Q, disp, bgr, poses, vs, jump, minpts, env)
        assert_points_equal(big, rbig, f"{what}, {env}: cloud_big")
        assert_points_equal(small, rsmall, f"{what}, {env}: merged cloud")
    return sts, [len(c) for c in clouds]


# ---- the count pass -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("invalid_frac", [0.0, 0.3, 0.97])
@pytest.mark.parametrize("cols", [640, 608])
def test_row_ends(monkeypatch, orc, cols, invalid_frac):
    """360 x 640: rows of 540 candidates, every row end inside a 16-candidate group, a last tile of 768 candidates;
    360 x 608: rows of 512 candidates, no group crosses a row"""
    disp, bgr, poses, Q = _frames(210, 3, invalid_frac, 360, cols)
    nx = _roi(disp[0]).shape[1]
    assert nx == {640: 540, 608: 512}[cols] and (nx % 16 == 12) == (cols == 640)
    if cols == 640:
        assert _roi(disp[0]).size % 1024 == 768
    _, sizes = _check(monkeypatch, orc, Q, disp, bgr, poses, f"cols {cols}, invalid_frac {invalid_frac}")
    assert min(sizes) > 0


def test_only_first_and_last_candidate_valid(monkeypatch, orc):
    """a frame whose only valid pixels are the first and the last candidate (the last one in a group that ends with the
    frame), between two ordinary frames"""
    disp, bgr, poses, Q = _frames(220, 3, 0.1, 360, 640)
    roi = _roi(disp[1])
    roi[...] = 0
    roi[0, 0] = 90
    roi[-1, -1] = 100
    _, sizes = _check(monkeypatch, orc, Q, disp, bgr, poses, "first and last candidate")
    assert sizes[1] == 2


def test_all_invalid_frames_first_middle_last(monkeypatch, orc):
    disp, bgr, poses, Q = _frames(230, 7, 0.05, 360, 640)
    for f in (0, 3, 6):
        disp[f] = 0
    _, sizes = _check(monkeypatch, orc, Q, disp, bgr, poses, "all-invalid frames")
    assert [s == 0 for s in sizes] == [True, False, False, True, False, False, True]


def test_full_width_720p(monkeypatch, orc):
    """rows of 1100 candidates (1100 % 16 == 12), 731 tiles: the last workgroup of the count pass covers 3 of its 8"""
    disp, bgr, poses, Q = _frames(240, 2, 0.02, 720, 1280)
    assert _roi(disp[0]).shape == (680, 1100)
    _check(monkeypatch, orc, Q, disp, bgr, poses, "720p")


def test_jump_pixels_4_keeps_the_dword_loads(monkeypatch, orc):
    """the generic pixel loads (not the wide layout): 170 x 275 candidates per frame"""
    disp, bgr, poses, Q = _frames(250, 3, 0.3, 720, 1280)
    _check(monkeypatch, orc, Q, disp, bgr, poses, "jump 4", jump=4)


# ---- PCL's overflow guard: the exact-box pass behind the conservative box --------------------------------------------------------

def _overflow_batch(start, sorted_frames):
    """voxel_size 0.019 (tests/test_emit_digit_count.py): a full 720p frame trips the guard and passes through; a frame
    that keeps only a window of near pixels has a small box and is sorted"""
    disp, bgr, poses, Q = _frames(start, 4, 0.02, 720, 1280)
    for f in sorted_frames:
        keep = np.zeros(disp[f].shape, bool)
        keep[300:420, 500:760] = True
        near = disp[f] >= np.percentile(disp[f][300:420, 500:760], 50)
        disp[f][~(keep & near)] = 0
    return disp, bgr, poses, Q


def test_overflow_frames_between_sorted_frames(monkeypatch, orc):
    """sorted, pass-through, sorted, pass-through: the walking workgroups take frames 1 and 3 and return for 0 and 2"""
    disp, bgr, poses, Q = _overflow_batch(260, (0, 2))
    sts, sizes = _check(monkeypatch, orc, Q, disp, bgr, poses, "overflow next to sorted", vs=0.019, minpts=3)
    assert [s != 0 for s in sts] == [False, True, False, True] and orc.STATUS_VOXEL_OVERFLOW in sts
    assert min(sizes) > 0


def test_no_overflow_frame_in_the_batch(monkeypatch, orc):
    """the same leaf, every frame a window: every workgroup of the exact-box pass returns"""
    disp, bgr, poses, Q = _overflow_batch(270, (0, 1, 2, 3))
    sts, sizes = _check(monkeypatch, orc, Q, disp, bgr, poses, "no overflow frame", vs=0.019, minpts=3)
    assert sts == [0, 0, 0, 0] and min(sizes) > 0


# ---- behind k_centroid: head flags, running box ---------------------------------------------------------------------------------

_tail = {}


def _tail_case(orc):
    """7 frames at 720p (two calls put cloud_big past the size from which the merge sorts group runs); the oracle's
    cloud_big and merged cloud after two calls (frames 0-2, 3-6) and after a third (frames 0-1 again); computed once"""
    if not _tail:
        disp, bgr, poses, Q = _frames(280, 7, 0.01, 720, 1280)
        clouds, sts = _oracle_clouds(orc, Q, disp, bgr, poses, 0.05, 1)
        assert not any(sts)
        bigs = [np.concatenate(clouds), np.concatenate(clouds + clouds[:2])]
        assert len(bigs[0]) > (1 << 20)
        _tail.update(disp=disp, bgr=bgr, poses=poses, Q=Q, bigs=bigs,
                     smalls=[orc.downsample_pt_cloud(b, 0.05, True, 1)[0] for b in bigs])
    return _tail


def _tail_sequence(c, t, what, grouped):
    """two calls and a merge, a third call and a merge; every result against the oracle's"""
    outs = []
    for stage, calls in enumerate([(slice(0, 3), slice(3, 7)), (slice(0, 2),)]):
        for fr in calls:
            c.accumulateFrames(t["disp"][fr], t["bgr"][fr], t["poses"][fr])
        big = c.cloudBigRead()
        assert_points_equal(big, t["bigs"][stage], f"{what}: cloud_big, stage {stage}")
        mn, mx, n = c.cloudBigBBox()
        assert n == len(big)
        for k, ax in enumerate("xyz"):
            assert mn[k] == big[ax].min() and mx[k] == big[ax].max(), (what, stage, ax)
        c.profileReset()
        small = c.finalize()
        recs = c.profileStatsAll()[4]
        assert_points_equal(small, t["smalls"][stage], f"{what}: merged cloud, stage {stage}")
        if grouped:  # the merge started from the recorded heads: its sort's records were group runs
            assert recs * 8 <= len(big), (what, stage, recs, len(big))
        outs += [big, small]
    return outs


def test_tail_over_three_calls(orc):
    import online_3d_reconstruction_amd as o3dr
    t = _tail_case(orc)
    with o3dr.Context(0, Q=t["Q"], params=_params(jump_pixels=1, voxel_size=0.05)) as c:
        _tail_sequence(c, t, "tracked box and heads", True)


def test_box_against_a_pass_over_the_cloud(monkeypatch, orc):
    """O3DR_NO_CLOUD_BOX=1: box and heads from passes over the cloud at merge time; same results"""
    import online_3d_reconstruction_amd as o3dr
    t = _tail_case(orc)
    with monkeypatch.context() as mp:
        mp.setenv("O3DR_NO_CLOUD_BOX", "1")
        c = o3dr.Context(0, Q=t["Q"], params=_params(jump_pixels=1, voxel_size=0.05))
    with c:
        ref = _tail_sequence(c, t, "box by a pass", False)
    with o3dr.Context(0, Q=t["Q"], params=_params(jump_pixels=1, voxel_size=0.05)) as c:
        got = _tail_sequence(c, t, "tracked box", True)
    for a, b in zip(got, ref):
        assert_points_equal(a, b, "tracked box against a pass over the cloud")


def test_scratch_contents_do_not_matter(monkeypatch, orc):
    """the batched call and the merge after o3dr_test_fill_scratch with all ones and with zeros: the bytes of the
    unfilled run (the count pass now sets the keypoint slot and n_kp that a launch of its own used to set)"""
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    disp, bgr, poses, Q = _frames(290, 3, 0.3, 360, 640)
    with monkeypatch.context() as mp:
        mp.setenv("O3DR_TEST_HOOKS", "1")
        c = o3dr.Context(0, Q=Q, params=_params(jump_pixels=1, voxel_size=0.05))
    runs = []
    with c:
        for byte in (None, 0xFF, 0x00):
            c.cloudBigReset()
            if byte is not None:
                n = C.c_int64(0)
                L.check(c._lib.o3dr_test_fill_scratch(c._h, byte, C.byref(n)))
                assert n.value > 0
            c.accumulateFrames(disp[:2], bgr[:2], poses[:2])
            c.accumulateFrames(disp[2:], bgr[2:], poses[2:])
            big = c.cloudBigRead()
            mn, mx, _ = c.cloudBigBBox()
            runs.append((big, c.finalize(), mn, mx))
    clouds, _ = _oracle_clouds(orc, Q, disp, bgr, poses, 0.05, 1)
    assert_points_equal(runs[0][0], np.concatenate(clouds), "unfilled: cloud_big")
    for k, ax in enumerate("xyz"):
        assert runs[0][2][k] == runs[0][0][ax].min() and runs[0][3][k] == runs[0][0][ax].max()
    for byte, r in zip((0xFF, 0x00), runs[1:]):
        assert_points_equal(r[0], runs[0][0], f"fill {byte:#x}: cloud_big")
        assert_points_equal(r[1], runs[0][1], f"fill {byte:#x}: merged cloud")
        assert r[2].tobytes() == runs[0][2].tobytes() and r[3].tobytes() == runs[0][3].tobytes(), f"fill {byte:#x}: box"


# ---- launches --------------------------------------------------------------------------------------------------------------------

PARENT_SCOPES = 25


def test_profile_scopes_of_one_call(orc):
    """Every kind profiled, one accumulateFrames call of 3 frames (360 x 640, jump_pixels 1, five-pass plan, emit pass
    counts the first digit).  The profiler counts SCOPES, each around one or more launches.  The build before this
    change: 25 scopes (measured on that build: reproject_count 2, reproject_emit 1, radix_hist 4, radix_scatter 5,
    run_segments 2, centroid 1, other 10) around 30 launches.  Three launches are gone - k_minmax_init, k_voxel_geom behind
    the tile-count scan, k_side_heads - and with them the one scope that held nothing else (k_minmax_init's): 24."""
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    disp, bgr, poses, Q = _frames(300, 3, 0.1, 360, 640)
    with o3dr.Context(0, Q=Q, params=_params(jump_pixels=1, voxel_size=0.05)) as c:
        c.profileEnable(-1)
        c.accumulateFrames(disp, bgr, poses)
        scopes = [c.profileRead(k)[1] for k in range(len(L.KERNEL_NAMES))]
        c.profileEnable(-1, False)
        big = c.cloudBigRead()
    print("scopes per kind:", dict(zip(L.KERNEL_NAMES, scopes)), "sum:", sum(scopes))
    assert sum(scopes) == PARENT_SCOPES - 1
    clouds, _ = _oracle_clouds(orc, Q, disp, bgr, poses, 0.05, 1)
    assert_points_equal(big, np.concatenate(clouds), "profiled call: cloud_big")
