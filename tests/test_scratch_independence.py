"""No operator's result may depend on what its scratch memory held (DESIGN.md "Scratch contract").

Every operator runs out of blocks the context owns and reuses from call to call: the shared operator blocks, the sort /
voxel workspace, the staging buffers, the incremental merge's per-call buffers, the 4 KiB misc block.  The first context
of a process gets them from hipMalloc zeroed, in practice, and nearly every other test runs one operator on a new or
per-module context.  Here every operator runs (1) after o3dr_test_fill_scratch wrote 0xFF and then 0x00 over all of it - all ones is the right initial
value of every atomicMin word and empty key, zero that of every counter, so each pattern is poison for the other kind;
(2) after a larger call of itself, which leaves real data beyond this call's n; (3) after every other operator, in table
order and in reverse.  Results are compared byte for byte, NaN through their bits, and the first one with the operator's
own reference, through the checkers of the operator's own test file (imported, not copied).

One table of cases.  Every entry point of include/o3dr.h has a case or stands in NOT_COVERED because it launches no
kernel and touches no scratch; test_every_entry_point_has_a_case_or_a_reason holds the table to that."""
import contextlib
import ctypes as C
import dataclasses
import os
import re
import threading

import numpy as np
import pytest

import orb_reference
import pose_chain_reference as PR
import ransac_rigid_reference as RR
import raster_reference as rr
import rectify_reference as RectR
import test_cell_order as t_cell
import test_disparity_filter as t_dfilt
import test_feature_matching as t_match
import test_icp_align as t_icp
import test_mesh_surface as t_mesh
import test_mls_smooth as t_mls
import test_multiview_filter as t_mvf
import test_multiview_fuse as t_mvfuse
import test_orb_boundaries as t_orb
import test_plane_disparity as t_pdisp
import test_plane_segmentation as t_plane
import test_pose_chain as t_chain
import test_pose_chain_robust as t_robust
import test_pose_graph as t_graph
import test_ransac_rigid as t_ransac
import test_rasterize_map as t_raster
import test_segment_image as t_seg
import test_stereo_disparity as t_stereo
from conftest import GOLDEN, ROOT, assert_points_equal, load_frame, random_cloud

SIZES = ("small", "large")
THR = 0.05  # the robust fits' threshold (tests/test_ransac_rigid.py)


# ---- contexts, the hook, bytes ----------------------------------------------------------------------------------------------
@contextlib.contextmanager
def hooked_context():
    """a context of its own with the test hooks on (they are read at o3dr_ctx_create)"""
    import online_3d_reconstruction_amd as o3dr
    mp = pytest.MonkeyPatch()
    mp.setenv("O3DR_TEST_HOOKS", "1")
    try:
        c = o3dr.Context(0)
    finally:
        mp.undo()
    try:
        yield c
    finally:
        c.close()


def fill(ctx, byte):
    from online_3d_reconstruction_amd import _lib as L
    n = C.c_int64(0)
    L.check(ctx._lib.o3dr_test_fill_scratch(ctx._h, byte, C.byref(n)))
    return n.value


def blob(x):
    """every output of a call as one bytes object: arrays through their bytes (NaN by bit pattern), with dtype and shape"""
    if x is None:
        return b"N;"
    if isinstance(x, (bytes, bytearray)):
        return b"B" + bytes(x) + b";"
    if isinstance(x, (bool, np.bool_)):
        return b"b1;" if x else b"b0;"
    if isinstance(x, (int, np.integer)):
        return b"i%d;" % int(x)
    if isinstance(x, (float, np.floating)):
        return b"f" + np.float64(x).tobytes() + b";"
    if isinstance(x, str):
        return b"s" + x.encode() + b";"
    if type(x).__module__.startswith("torch"):
        import torch
        t = x.detach().contiguous()
        for u, s in (("uint16", torch.int16), ("uint32", torch.int32), ("uint64", torch.int64)):
            if hasattr(torch, u) and t.dtype == getattr(torch, u):
                t = t.view(s)
        return blob(t.cpu().numpy())
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        return b"A" + str(a.dtype).encode() + str(a.shape).encode() + a.tobytes() + b";"
    if isinstance(x, np.void):
        return blob(np.asarray(x))
    if isinstance(x, dict):
        return b"{" + b"".join(blob(k) + blob(v) for k, v in sorted(x.items())) + b"}"
    if isinstance(x, (tuple, list)):
        return b"(" + b"".join(blob(v) for v in x) + b")"
    if dataclasses.is_dataclass(x):
        return blob(dataclasses.asdict(x))
    if hasattr(x, "__dict__"):
        return blob(dict(vars(x)))
    raise TypeError(f"no byte form for {type(x)}")


class Replay:
    """stands in for a context in the existing `check(ctx, ...)` helpers: every method gives back a result that a real
    context already produced, so that the helper's comparison runs on it unchanged"""

    def __init__(self, **results):
        self._results = results

    def __getattr__(self, name):
        if name.startswith("_") or name not in self._results:
            raise AttributeError(name)
        return lambda *a, **k: self._results[name]


_MEMO = {}


def memo(key, make):
    """inputs and references: computed once, shared, never written to"""
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def orc():
    from oracle import orc as o
    return memo("orc", lambda: (o.build(), o)[1])


def params(**kw):
    import online_3d_reconstruction_amd as o3dr
    kw.setdefault("sor_enable", False)
    return o3dr.Params(**kw)


def golden_Q():
    return memo("Q", lambda: np.load(os.path.join(GOLDEN, "cam13calib_Q.npy")))


def pose(i):
    from online_3d_reconstruction_amd import synth
    return synth.make_pose(i)


class Case:
    def __init__(self, name, entries, call, check):
        self.name, self.entries, self.call, self.check = name, tuple(entries), call, check


CASES = {}


def case(name, *entries):
    def deco(cls):
        CASES[name] = Case(name, entries, cls.call, cls.check)
        return cls
    return deco


# ---- point clouds ----------------------------------------------------------------------------------------------------------------
N_CLOUD = {"small": 1025, "large": 20481}  # one workgroup (kernels/small.inc takes up to 8192 points) / three sort tiles
GRIDS = [((0.05, 0.05, 0.05), 0), ((0.011, 0.013, 0.017), 0), ((0.2, 0.2, 0.2), 3)]  # tests/test_gpu_parity.py, tile-edge sizes


def cloud(size):
    n = N_CLOUD[size]
    return memo(("cloud", n), lambda: random_cloud(n, 1000 + n, extent=(0.9, 0.7, 0.4)))


@case("voxel_grid", "o3dr_voxel_grid")
class _VoxelGrid:
    def call(ctx, size):
        return [ctx.voxelGrid(cloud(size), leaf, mp, return_status=True) for leaf, mp in GRIDS]

    def check(size, outs):
        for (got, st), (leaf, mp) in zip(outs, GRIDS):
            ref, rst = orc().voxel_grid(cloud(size), leaf, mp)
            assert st == rst
            assert_points_equal(got, ref, f"voxel grid {size} leaf {leaf} min_points {mp}")


@case("downsample", "o3dr_downsample_pt_cloud")
class _Downsample:
    def call(ctx, size):
        ctx.set_params(params(voxel_size=0.05, min_points_per_voxel=1))
        return [ctx.downsamplePtCloud(cloud(size), combined, return_status=True) for combined in (False, True)]

    def check(size, outs):
        for (got, st), combined in zip(outs, (False, True)):
            ref, rst = orc().downsample_pt_cloud(cloud(size), 0.05, combined, 1)
            assert st == rst
            assert_points_equal(got, ref, f"downsample {size} combined {combined}")


@case("transform", "o3dr_transform_pt_cloud")
class _Transform:
    def call(ctx, size):
        return ctx.transformPtCloud(cloud(size), pose(7))

    def check(size, out):
        assert_points_equal(out, orc().transform_pt_cloud(cloud(size), pose(7)), f"transform {size}")


def sor_cloud(size):
    """2 000 points (the one-workgroup path) and 20 000 (the general one)"""
    n, extent = {"small": (2000, (1.0, 1.0, 0.02)), "large": (20000, (2.0, 1.5, 0.1))}[size]
    return memo(("sor", n), lambda: random_cloud(n, 500 + n % 13, extent=extent))


@case("outlier_removal", "o3dr_statistical_outlier_removal")
class _Sor:
    def call(ctx, size):
        return ctx.statisticalOutlierRemoval(sor_cloud(size))

    def check(size, out):
        ref, _ = orc().statistical_outlier_removal(sor_cloud(size))
        assert 0 < len(ref) < len(sor_cloud(size))
        assert_points_equal(out, ref, f"outlier removal {size}")


@case("cloud_big", "o3dr_cloud_big_reset", "o3dr_cloud_big_append", "o3dr_cloud_big_transform", "o3dr_cloud_big_bbox",
      "o3dr_cloud_big_size", "o3dr_cloud_big_read", "o3dr_cloud_big_recv_buffer", "o3dr_cloud_big_adopt", "o3dr_cloud_big_view",
      "o3dr_cloud_big_capacity", "o3dr_cloud_big_reserve")
class _CloudBig:
    def call(ctx, size):
        import torch
        pts = cloud(size)
        ctx.cloudBigReset()
        ctx.cloudBigReserve(len(pts))
        ctx.cloudBigAppend(pts)
        ctx.cloudBigTransform(pose(5))
        box = ctx.cloudBigBBox()
        moved, n = ctx.cloudBigRead(), ctx.cloudBigSize()
        recv = ctx.cloudBigRecvBuffer(len(pts))
        recv.copy_(torch.from_numpy(np.ascontiguousarray(pts[::-1]).view(np.int32).reshape(-1, 4)))
        torch.cuda.synchronize()
        ctx.cloudBigAdopt(len(pts))
        view = ctx.cloudBigView().clone()
        adopted = ctx.cloudBigRead()
        assert ctx.cloudBigCapacity()[0] >= len(pts)  # (the capacities themselves depend on what the context ran before)
        ctx.cloudBigReset()
        return box, moved, n, view, adopted

    def check(size, outs):
        (mn, mx, nb), moved, n, view, adopted = outs
        ref = orc().transform_pt_cloud(cloud(size), pose(5))
        assert_points_equal(moved, ref, f"cloud_big transform {size}")
        assert n == (len(ref), 0) and nb == len(ref)
        xyz = np.stack([ref["x"], ref["y"], ref["z"]], 1)
        assert np.array_equal(mn, xyz.min(0)) and np.array_equal(mx, xyz.max(0))
        assert_points_equal(adopted, cloud(size)[::-1], f"cloud_big adopt {size}")
        assert np.array_equal(view.cpu().numpy().view(np.uint32), np.ascontiguousarray(adopted).view(np.uint32).reshape(-1, 4))


# ---- single frames -----------------------------------------------------------------------------------------------------------------
JUMP = {"small": 15, "large": 2}      # 3 600 candidates: one workgroup; 187 000: the general path
JUMP_SOR = {"small": 15, "large": 4}  # tests/test_gpu_parity.py::test_A6_with_sor_matches_reference_pipeline


def frame_setup(ctx, jump, **kw):
    ctx.set_camera(golden_Q())
    ctx.set_params(params(jump_pixels=jump, voxel_size=0.05, **kw))
    return load_frame("1248")


@case("create_single", "o3dr_create_single_img_pt_cloud")
class _CreateSingle:
    def call(ctx, size):
        disp, bgr = frame_setup(ctx, JUMP[size])
        return ctx.createSingleImgPtCloud(disp, bgr)

    def check(size, out):
        disp, bgr = load_frame("1248")
        assert_points_equal(out, orc().create_single_img_pt_cloud(disp, bgr, golden_Q(), jump_pixels=JUMP[size]), f"A1 {size}")


@case("reproject_transform", "o3dr_reproject_transform")
class _ReprojectTransform:
    def call(ctx, size):
        disp, bgr = frame_setup(ctx, JUMP[size])
        return ctx.reprojectTransform(disp, bgr, pose(11))

    def check(size, out):
        disp, bgr = load_frame("1248")
        ref = orc().transform_pt_cloud(orc().create_single_img_pt_cloud(disp, bgr, golden_Q(), jump_pixels=JUMP[size]), pose(11))
        assert_points_equal(out, ref, f"A1+A2 {size}")


@case("create_and_transform", "o3dr_create_and_transform_pt_cloud")
class _CreateAndTransform:
    """without and with the outlier removal in front of the per-frame grid"""

    def call(ctx, size):
        disp, bgr = frame_setup(ctx, JUMP[size])
        plain = ctx.createAndTransformPtCloud(disp, bgr, pose(3), return_status=True)
        disp, bgr = frame_setup(ctx, JUMP_SOR[size], sor_enable=True)
        return plain, ctx.createAndTransformPtCloud(disp, bgr, pose(3), return_status=True)

    def check(size, outs):
        from test_gpu_parity import _sor_oracle_pipeline
        disp, bgr = load_frame("1248")
        (got, st), (got_sor, st_sor) = outs
        ref, rst = orc().create_and_transform_pt_cloud(disp, bgr, golden_Q(), pose(3), 0.05, jump_pixels=JUMP[size])
        assert st == rst == 0 and st_sor == 0
        assert_points_equal(got, ref, f"A6 {size}")
        ref_sor, _ = _sor_oracle_pipeline(orc(), golden_Q(), disp, bgr, pose(3), 0.05, JUMP_SOR[size])
        assert_points_equal(got_sor, ref_sor, f"A6 with outlier removal {size}")


def kp_case(size):
    def make():
        rows, cols = load_frame("1248")[0].shape
        return t_match._keypoints(np.random.default_rng(13), rows, cols, {"small": 300, "large": 3000}[size])
    return memo(("kp3", size), make)


@case("keypoints_3d", "o3dr_keypoints_3d")
class _Keypoints3D:
    def call(ctx, size):
        disp, bgr = frame_setup(ctx, 1)
        return ctx.keypoints3D(disp, kp_case(size), poses=pose(2), bgr=bgr)

    def check(size, out):
        disp, bgr = load_frame("1248")
        kp = kp_case(size)
        ok = t_match._accepted(disp, kp)
        assert ok.sum() > 20 and (~ok).sum() > 20 and len(out) == len(kp)
        assert np.array_equal(np.isfinite(out["x"]), ok)
        ref = orc().create_single_img_pt_cloud(disp, bgr, golden_Q(), jump_pixels=0, kp_xy=kp)
        assert_points_equal(out[ok], orc().transform_pt_cloud(ref, pose(2)), f"keypoints3D {size}")
        assert np.isnan(out["y"][~ok]).all() and np.isnan(out["z"][~ok]).all() and (out["rgba"][~ok] == 0).all()


# ---- images: 33 x 70 and 67 x 131 ----------------------------------------------------------------------------------------------------
SHAPE = {"small": (33, 70), "large": (67, 131)}


def grey(size, seed=0):
    H, W = SHAPE[size]
    return memo(("grey", size, seed), lambda: np.random.default_rng(100 + seed).integers(0, 256, (H, W)).astype(np.uint8))


@case("bilateral", "o3dr_bilateral_filter_u8")
class _Bilateral:
    def call(ctx, size):
        return ctx.bilateralFilter(grey(size), 9, 18.0, 4.0)

    def check(size, out):
        assert np.array_equal(out, orc().bilateral_filter(grey(size), 9, 18.0, 4.0))


def variance_stack(size):
    return memo(("var", size), lambda: np.stack([load_frame(n)[0] for n in (("1248",) if size == "small" else ("1248", "1249", "1251"))]))


@case("disparity_variance", "o3dr_disparity_variance")
class _DisparityVariance:
    def call(ctx, size):
        ctx.set_params(params(jump_pixels=1, voxel_size=0.05))
        return ctx.disparityVariance(variance_stack(size))

    def check(size, out):
        ref = np.array([orc().disparity_variance(d) for d in variance_stack(size)])
        assert (np.abs(out - ref) <= 1e-9 * ref).all()  # (tests/test_gpu_parity.py::test_disparity_variance_gate)


def plane_disp_case(size):
    def make():
        H, W = SHAPE[size]
        labels = np.ascontiguousarray(t_pdisp.blocky(H, W, 6, 5).astype(np.uint16))
        disp = t_pdisp.rand_disp((H, W), 15)
        n_labels = int(labels.max()) + 1
        return disp, labels, n_labels, t_pdisp.ref_plane_fit(disp[None], labels[None], n_labels)
    return memo(("plane_disp", size), make)


@case("plane_fit_disparity", "o3dr_plane_fit_disparity")
class _PlaneFitDisparity:
    def call(ctx, size):
        disp, labels, n_labels, _ = plane_disp_case(size)
        return ctx.planeFitDisparity(disp, labels, n_labels=n_labels, return_segments=True)

    def check(size, outs):
        disp, labels, n_labels, (ref_img, fits) = plane_disp_case(size)
        got, rec = outs
        t_pdisp.assert_bits_equal(got.reshape(ref_img.shape), ref_img, f"plane fit {size}")
        t_pdisp.assert_records_equal(rec.reshape(len(fits), n_labels), fits, f"plane fit {size}")


ORB = {"small": (lambda: t_orb._crop(300, 600, 192), dict(n_features=64, n_levels=2)),     # tests/test_orb_boundaries.py, frame groups
       "large": (lambda: t_orb._crop(200, 500, 384), dict(n_features=300, n_levels=3))}


@case("orb_detect", "o3dr_orb_detect")
class _Orb:
    def call(ctx, size):
        make, kw = ORB[size]
        return ctx.findFeatures(memo(("orb img", size), make), return_levels=True, **kw)

    def check(size, outs):
        make, kw = ORB[size]
        want = memo(("orb ref", size), lambda: orb_reference.detect(memo(("orb img", size), make), **kw))
        assert len(want["kp"]) > 20
        t_orb._assert_equal(outs, want, f"orb {size}")
        t_orb._assert_levels(outs[4], want, f"orb {size}")


RECTIFY = {"small": (41, 50), "large": (83, 101)}


def rectify_case(size):
    def make():
        c = RectR.GENERAL
        maps = RectR.rectify_maps(c["K"], c["D"], c["R"], c["P"], RECTIFY[size])
        frames = np.stack([RectR.test_image(37, 53, 3, seed=10 + f) for f in range(5)])
        return maps, frames, RectR.rectify_remap_frames(frames, maps, 9)
    return memo(("rectify", size), make)


@case("rectify", "o3dr_rectify_maps", "o3dr_rectify_remap")
class _Rectify:
    """five frames in groups of two: the multi-group case of tests/test_rectify.py"""

    def call(ctx, size):
        c = RectR.GENERAL
        maps, frames, _ = rectify_case(size)
        got = ctx.rectifyMaps(c["K"], c["D"], c["R"], c["P"], RECTIFY[size])
        return got, ctx.rectify(frames, maps, border=9, return_valid=True, group_frames=2)

    def check(size, outs):
        maps, frames, (want, want_valid) = rectify_case(size)
        got_maps, (got, valid) = outs
        assert got_maps.dtype == np.int32 and np.array_equal(got_maps, maps)
        assert got.dtype == np.uint8 and np.array_equal(got, want) and np.array_equal(valid, want_valid) and want_valid.any()


STEREO_D = {"small": 32, "large": 64}


def stereo_case(size):
    def make():
        H, W = SHAPE[size]
        left, right = t_stereo.make_pair(H, W, seed=H * 1000 + W)
        return left, right, t_stereo.reference(left, right, n_disparities=STEREO_D[size])
    return memo(("stereo", size), make)


@case("stereo", "o3dr_stereo_disparity")
class _Stereo:
    def call(ctx, size):
        left, right, _ = stereo_case(size)
        return t_stereo.run(ctx, left, right, n_disparities=STEREO_D[size])

    def check(size, outs):
        t_stereo.check(outs, stereo_case(size)[2], f"stereo {size}")


DFILT = {"small": (33, 70, 3, "uint8"), "large": (67, 131, 5, "uint16")}


@case("disparity_filter", "o3dr_disparity_filter")
class _DisparityFilter:
    def call(ctx, size):
        img, _ = t_dfilt.shape_case(*DFILT[size])
        return t_dfilt.run(ctx, img, DFILT[size][2], 3, t_dfilt.unit(img.dtype.type))

    def check(size, outs):
        t_dfilt.check(outs, t_dfilt.shape_case(*DFILT[size])[1], f"disparity filter {size}")


SEG = (8, 20, 5, None)  # step, compactness, iterations, min_size


@case("segment_image", "o3dr_segment_image")
class _SegmentImage:
    def call(ctx, size):
        return t_seg.run(ctx, t_seg.image(*SHAPE[size], 3), *SEG)

    def check(size, outs):
        img = t_seg.image(*SHAPE[size], 3)
        t_seg.check(outs, memo(("seg", size), lambda: t_seg.reference(img, *SEG)), f"segmentation {size}")


MV = {"small": t_mvf.MULTI_TILE[3], "large": t_mvf.MULTI_TILE[0]}  # 33 x 70 and 67 x 131


@case("multiview_filter", "o3dr_multiview_filter")
class _MultiviewFilter:
    def call(ctx, size):
        c = MV[size]
        disp, Q, poses, nb, _ = t_mvf.case(c)
        return t_mvf.run(ctx, disp, Q, poses, nb, c[5], c[6], c[7])

    def check(size, outs):
        t_mvf.same(outs, t_mvf.case(MV[size])[4], f"multi-view filter {size}")


@case("multiview_fuse", "o3dr_multiview_fuse")
class _MultiviewFuse:
    def call(ctx, size):
        c = MV[size]
        disp, Q, poses, nb, _ = t_mvfuse.case(c)
        return t_mvfuse.run(ctx, disp, Q, poses, nb, c[5], c[6], c[7])

    def check(size, outs):
        t_mvfuse.same(outs, t_mvfuse.case(MV[size])[4], f"multi-view fusion {size}")


# ---- search grids ----------------------------------------------------------------------------------------------------------------------
def nn_case(size):
    def make():
        rng = np.random.default_rng(1)
        nt, nq = {"small": (3000, 2000), "large": (30000, 20000)}[size]
        t = (rng.random((nt, 3)) * [20, 15, 4] + [-3, 7, -1]).astype(np.float32)
        q = (rng.random((nq, 3)) * [40, 35, 12] + [-13, -3, -5]).astype(np.float32)  # about 3/4 outside the target's box
        return q, t
    return memo(("nn", size), make)


@case("nearest_neighbors", "o3dr_nearest_neighbors")
class _NearestNeighbors:
    def call(ctx, size):
        q, t = nn_case(size)
        return ctx.nearestNeighbors(t_icp._pts(q), t_icp._pts(t)), ctx.nearestNeighbors(t_icp._pts(q[:1000]), t_icp._pts(t), 0.4)

    def check(size, outs):
        q, t = nn_case(size)
        t_icp._check_nn(Replay(nearestNeighbors=outs[0]), q, t, oracle=t_icp.nn_tree)
        idx, _ = t_icp._check_nn(Replay(nearestNeighbors=outs[1]), q[:1000], t, 0.4, oracle=t_icp.nn_tree)
        assert (idx == t_icp.NONE).any() and (idx != t_icp.NONE).any()


def icp_case(size):
    def make():
        n, step = {"small": (5000, 2), "large": (20000, 3)}[size]
        tgt = t_icp.synthetic_surface(n, 8)
        G = t_icp.rigid(0.01, 0.008, -0.012, [0.03, 0.02, -0.01])
        src = t_icp.a2(np.linalg.inv(G), tgt[::step])
        return src, tgt, t_icp.icp_numpy(src, tgt, max_iterations=5)
    return memo(("icp", size), make)


@case("icp_align", "o3dr_icp_align")
class _Icp:
    def call(ctx, size):
        src, tgt, _ = icp_case(size)
        return ctx.icpAlign(t_icp._pts(src), t_icp._pts(tgt), max_iterations=5)

    def check(size, r):
        ref = icp_case(size)[2]  # the bounds of tests/test_icp_align.py's recovery tests
        assert np.abs(r.T - ref[0]).max() < 1e-6 and r.n_correspondences == ref[2]
        assert abs(r.fitness - ref[1]) <= 1e-6 * max(ref[1], 1e-12) + 1e-12


def mls_case(size):
    def make():
        if size == "small":
            return t_mls.tilted_sphere_cap(3000, 5)[0], 0.06, 0.0005
        return t_mls.wavy_surface(12000, 4), 0.08, 0.0
    return memo(("mls", size), make)


@case("mls_smooth", "o3dr_mls_smooth")
class _Mls:
    def call(ctx, size):
        xyz, r, h = mls_case(size)
        return t_mls._run(ctx, xyz, r, 2, h)

    def check(size, outs):
        xyz, r, h = mls_case(size)
        pts, out, nrm, cnt, fit, info = outs
        obs = t_mls.check_against_numpy(xyz, out, nrm, cnt, fit, r, 2, h, rgba=pts["rgba"])
        assert obs["n"] == len(xyz) and (fit != t_mls.NONE).any()


# ---- the 67 x 35 cell cloud (and 141 x 77) ---------------------------------------------------------------------------------------------
def cell_cloud(size):
    w, h = {"small": (67, 35), "large": (141, 77)}[size]
    return memo(("cells", size), lambda: t_raster.grid_cloud(w, h, holes=0.3, seed=6, extra=200))


PLANE = dict(t=0.05, H=8, s=0.5, seed=7)


@case("segment_plane", "o3dr_segment_plane")
class _SegmentPlane:
    def call(ctx, size):
        p = PLANE
        return ctx.segmentPlane(t_mesh._pts(cell_cloud(size)), p["t"], p["H"], p["s"], p["seed"], False, project=True, return_tile_index=True)

    def check(size, outs):
        p, xyz = PLANE, cell_cloud(size)
        inl, tiles, prj, til = outs
        got = t_cell.check_plane(Replay(segmentPlane=(inl, tiles, til)), xyz, p["s"], p["H"], p["seed"], p["t"])
        assert len(got) > 8 and (tiles["status"] == 0).any()
        t_plane._check_labels(t_mesh._pts(xyz), p["t"], inl, prj, tiles, [idx for *_, idx in t_plane.tiles_numpy(xyz, p["s"])])


@case("mesh_surface", "o3dr_mesh_surface")
class _Mesh:
    def call(ctx, size):
        return ctx.meshSurface(t_mesh._pts(cell_cloud(size)), 0.05, 0.09, return_normals=True, return_info=True)

    def check(size, outs):
        info = t_cell.check_mesh(Replay(meshSurface=outs), cell_cloud(size), 0.05, 0.09)
        assert info.n_triangles > 100 and info.n_shadowed > 0 and info.n_rejected_length > 0


RASTER = dict(fill_radius=3, light=t_raster.LIGHT)


@case("rasterize_map", "o3dr_raster_extent", "o3dr_rasterize_map")
class _Raster:
    def call(ctx, size):
        p = t_raster._pts(cell_cloud(size))
        return ctx.rasterExtent(p, 0.05), ctx.rasterizeMap(p, 0.05, return_source=True, return_distance=True, return_info=True, **RASTER)

    def check(size, outs):
        xyz = cell_cloud(size)
        assert tuple(outs[0]) == tuple(rr.extent(xyz, 0.05))
        _, ref = t_raster.check(Replay(rasterizeMap=outs[1]), xyz, 0.05, what=f"raster {size}", **RASTER)
        assert ref.info["n_shadowed"] > 0 and ref.info["n_filled"] > 0


# ---- the 8- and 16-frame worlds ----------------------------------------------------------------------------------------------------------
def world(size, corrupted=False):
    """world A of tests/test_pose_chain.py (8 frames) and the loop world of tests/test_pose_graph.py (16) with their plain
    reference chains; corrupted: 20 % of every frame's 3-D keypoints wrong (tests/test_pose_chain_robust.py)"""
    def make():
        # (the wrong points are found by a threshold: the corrupted loop is the one without keypoint noise)
        w, ch = t_chain.world_a() if size == "small" else t_graph.loop_world(0.0 if corrupted else 0.02)
        if corrupted:
            w = RR.corrupt_world(w, 0.2, 100)
            ch = PR.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=t_chain.DIST)
        return w, ch
    return memo(("world", size, corrupted), make)


def pair_rows(size, corrupted):
    """what a chain gathers for the pairs (i, i - 1): every query row with its best train row's 3-D point, the good mask"""
    def make():
        w, _ = world(size, corrupted)
        off = w["offsets"]
        src, tgt, mask, seg = [], [], [], [0]
        for i in range(1, len(off) - 1):
            q, t = slice(off[i], off[i + 1]), slice(off[i - 1], off[i])
            idx, dist = PR.knn2_ref(w["desc"][q], w["desc"][t])
            src.append(w["kp3"][q])
            tgt.append(w["kp3"][t][np.clip(idx[:, 0].astype(np.int64), 0, off[i] - off[i - 1] - 1)])
            mask.append(PR.good_ref(dist))
            seg.append(seg[-1] + len(idx))
        return (np.concatenate(src).astype(np.float32), np.concatenate(tgt).astype(np.float32), np.array(seg, np.int64),
                np.concatenate(mask).astype(np.uint8))
    return memo(("rows", size, corrupted), make)


@case("match", "o3dr_match_knn2_hamming")
class _Match:
    def call(ctx, size):
        w, ch = world(size)
        return ctx.matchDescriptors(w["desc"], w["offsets"], ch["pairs"])

    def check(size, outs):
        w, ch = world(size)
        rec, good = outs
        idx, dist, g = memo(("match ref", size), lambda: t_match.batch_ref(w["desc"], w["offsets"], ch["pairs"]))
        gi, gd = t_match._records(rec)
        assert np.array_equal(gi, idx) and np.array_equal(gd, dist) and np.array_equal(good, g) and g.any() and not g.all()


@case("rigid_fit", "o3dr_estimate_rigid_transform")
class _Rigid:
    def call(ctx, size):
        src, tgt, seg, mask = pair_rows(size, False)
        return ctx.estimateRigidTransform(PR.points(src), PR.points(tgt), seg_offsets=seg, mask=mask)

    def check(size, outs):
        from online_3d_reconstruction_amd import _lib as L
        src, tgt, seg, mask = pair_rows(size, False)
        assert len(outs) == len(seg) - 1
        for s, r in enumerate(outs):
            a, b = seg[s], seg[s + 1]
            used = mask[a:b] != 0
            assert r.status == L.RIGID_OK and r.n_used == used.sum() > 30
            assert np.abs(r.T - t_match.kabsch_ref(src[a:b][used], tgt[a:b][used])).max() < 1e-9
            assert abs(r.rms - t_match._rms(r.T, src[a:b][used], tgt[a:b][used])) < 1e-9


@case("ransac_rigid", "o3dr_ransac_rigid")
class _Ransac:
    def call(ctx, size):
        src, tgt, seg, mask = pair_rows(size, True)
        return t_ransac._run(ctx, src, tgt, threshold=THR, iterations=64, seed=0, seg_offsets=seg, mask=mask)

    def check(size, outs):
        src, tgt, seg, mask = pair_rows(size, True)
        ref = memo(("ransac ref", size), lambda: RR.ransac_ref(src, tgt, THR, 64, 0, seg, mask))
        assert ref["gap"] > t_ransac.GAP and (ref["status"] == RR.OK).all()
        assert (ref["n_inliers"] < ref["n_candidates"]).all()
        t_ransac.assert_equal(outs, ref, f"ransac {size}")


def chain_floor(size, robust):
    """four times the reference chain's own one-ulp sensitivity (tests/test_pose_chain.py::test_whole_chain_poses)"""
    def make():
        w, _ = world(size, robust)
        kw = dict(ransac_threshold=THR) if robust else {}
        f = RR.robust_chain_ref if robust else PR.chain_ref
        ref = f(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=t_chain.DIST, **kw)
        floor = max(t_chain.max_pose_diff(f(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=t_chain.DIST, nudge=s, **kw)["poses"],
                                          ref["poses"]) for s in (1, -1))
        assert 0 < floor < 1e-4
        return ref, floor
    return memo(("chain ref", size, robust), make)


@case("pose_chain", "o3dr_pose_chain")
class _PoseChain:
    def call(ctx, size):
        return t_chain.run(ctx, world(size)[0], return_pairs=True)

    def check(size, outs):
        ref, floor = chain_floor(size, False)
        poses, rec, pairs = outs
        t_chain.assert_integers_equal(rec, ref, pairs)
        assert t_chain.max_pose_diff(poses, ref["poses"]) <= 4 * floor
        assert np.allclose(rec["rms"], ref["rms"], rtol=0, atol=4 * floor)


@case("pose_chain_robust", "o3dr_pose_chain_robust")
class _PoseChainRobust:
    def call(ctx, size):
        return t_robust.run(ctx, world(size, True)[0], ransac_threshold=THR, return_pairs=True, return_ransac=True)

    def check(size, outs):
        ref, floor = chain_floor(size, True)
        poses, rec, pairs, recs = outs
        assert ref["gap"] > t_robust.GAP
        assert [tuple(p) for p in pairs.tolist()] == ref["pairs"]
        t_robust.assert_integers_equal(rec, ref)
        RR.assert_ransac_equal(recs, ref)
        assert t_chain.max_pose_diff(poses, ref["poses"]) <= 4 * floor
        assert np.allclose(rec["rms"], ref["rms"], rtol=0, atol=4 * floor)


def graph_case(size):
    """the line world with a rejected frame (8 frames, tests/test_pose_graph.py::test_roles_on_the_gpu) and the loop world (16)"""
    if size == "large":
        w, ch = t_graph.loop_world()
        return w, ch, "floor", dict(gn_iterations=t_graph.GN, cg_iterations=t_graph.CG)
    w, ch = t_graph.line_world()
    status = ch["status"].copy()
    status[3] = PR.TOO_FEW
    return w, ch, "nm", dict(status=status)


@case("pose_graph", "o3dr_pose_graph_refine")
class _PoseGraph:
    def call(ctx, size):
        w, ch, _, kw = graph_case(size)
        return t_graph.run(ctx, w, ch, return_edges=True, **kw)

    def check(size, outs):
        w, ch, rule, kw = graph_case(size)
        t_graph.assert_parity(Replay(refinePoses=outs), w, ch, f"scratch {size}", rule=rule, **kw)


# ---- frame calls and merges --------------------------------------------------------------------------------------------------------------
GOLDEN_FRAMES = ("1248", "1249", "1251")
MERGE_JUMP = {"small": 6, "large": 2}  # 20 700 and 187 000 candidates a frame
VS = 0.05


def golden_stack():
    def make():
        fr = [load_frame(n) for n in GOLDEN_FRAMES]
        from online_3d_reconstruction_amd import synth
        return np.stack([f[0] for f in fr]), np.stack([f[1] for f in fr]), synth.make_poses(40, len(fr))
    return memo("golden stack", make)


def golden_kps():
    rng = np.random.default_rng(77)
    return memo("golden kps", lambda: [np.stack([rng.uniform(0, 1279, 400), rng.uniform(0, 719, 400)], 1).astype(np.float32) for _ in GOLDEN_FRAMES])


def merge_oracle(jump, minpts, sor, kp):
    """cloud_big and the merged cloud of the three frames by the CPU oracle"""
    def make():
        disp, bgr, poses = golden_stack()
        clouds = []
        for i in range(len(disp)):
            k = golden_kps()[i] if kp else None
            if sor:
                from test_gpu_parity import _sor_oracle_pipeline
                clouds.append(_sor_oracle_pipeline(orc(), golden_Q(), disp[i], bgr[i], poses[i], VS, jump, kp_xy=k)[0])
            else:
                clouds.append(orc().create_and_transform_pt_cloud(disp[i], bgr[i], golden_Q(), poses[i], VS, jump_pixels=jump, kp_xy=k)[0])
        big = np.concatenate(clouds)
        return big, orc().downsample_pt_cloud(big, VS, True, minpts)
    return memo(("merge oracle", jump, minpts, sor, kp), make)


def merge_run(ctx, jump, minpts=1, sor=False, kp=False, between=lambda: None):
    """frame by frame with an incremental merge after the second and the third frame, then the merge, the cloud and its
    box; `between` runs between any two of those calls"""
    disp, bgr, poses = golden_stack()
    ctx.set_camera(golden_Q())
    ctx.set_params(params(jump_pixels=jump, voxel_size=VS, min_points_per_voxel=minpts, sor_enable=sor))
    ctx.cloudBigReset()
    outs = []
    for i in range(len(disp)):
        between()
        ctx.accumulateFrames(disp[i:i + 1], bgr[i:i + 1], poses[i:i + 1], keypoints=[golden_kps()[i]] if kp else None)
        if i >= 1:
            between()
            merged = ctx.finalizeIncremental(return_status=True)
            stats = ctx.finalizeIncrementalStats()
            stats.pop("state_bytes")  # (capacities: they depend on what the context allocated before, by design)
            outs.append((merged, stats))
    between()
    outs.append(ctx.finalize(return_status=True))
    between()
    outs.append(ctx.cloudBigBBox())
    between()
    outs.append((ctx.cloudBigRead(), ctx.cloudBigSize()))
    between()
    outs.append(ctx.finalizeIncremental(return_status=True))
    ctx.cloudBigReset()
    return outs


def merge_check(outs, jump, minpts=1, sor=False, kp=False):
    (inc2, s2), (inc3, s3), (small, st), (mn, mx, nb), (big, n), (again, st2) = outs
    rbig, (rsmall, rst) = merge_oracle(jump, minpts, sor, kp)
    assert st == st2 == inc3[1] == rst == 0 and n == (len(rbig), 0) and nb == len(rbig)
    assert_points_equal(big, rbig, "cloud_big")
    assert_points_equal(small, rsmall, "finalize")
    assert_points_equal(inc3[0], rsmall, "finalizeIncremental after the third frame")
    assert_points_equal(again[0] if isinstance(again, tuple) else again, rsmall, "finalizeIncremental, nothing appended")
    assert s2["from_empty"] == 1 and s3["from_empty"] == 0 and s2["fallback"] == s3["fallback"] == 0
    assert s2["points_folded"] + s3["points_folded"] == len(rbig) and 0 < len(inc2[0]) <= len(rsmall)
    xyz = np.stack([rbig["x"], rbig["y"], rbig["z"]], 1)
    assert np.array_equal(mn, xyz.min(0)) and np.array_equal(mx, xyz.max(0))


@case("frames_and_merges", "o3dr_accumulate_frames", "o3dr_finalize", "o3dr_finalize_incremental", "o3dr_finalize_incremental_stats")
class _Frames:
    def call(ctx, size):
        return merge_run(ctx, MERGE_JUMP[size])

    def check(size, outs):
        merge_check(outs, MERGE_JUMP[size])


@case("frames_with_keypoints", "o3dr_accumulate_frames_kp")
class _FramesKp:
    """keypoints join the candidates iff jump_pixels != 1; the outlier removal in front of every frame's grid; min_points 3"""
    J = {"small": 15, "large": 4}

    def call(ctx, size):
        return merge_run(ctx, _FramesKp.J[size], 3, True, True)

    def check(size, outs):
        merge_check(outs, _FramesKp.J[size], 3, True, True)


# ---- the exchange: two virtual ranks, this context is rank 0 -----------------------------------------------------------------------------
RANK_SHAPE = {"small": (120, 160), "large": (240, 320)}  # 9 600 and 52 000 points a frame at jump_pixels 1
RANK_FRAMES = 4


def rank_case(size):
    def make():
        from online_3d_reconstruction_amd import synth
        rows, cols = RANK_SHAPE[size]
        disp, bgr = synth.make_frames(340, RANK_FRAMES, rows, cols, invalid_frac=0.01)
        poses = synth.make_poses(340, RANK_FRAMES)
        Q = synth.camera_Q(rows, cols)
        _, merged = orc().run_frames(disp, bgr, Q, poses, VS, jump_pixels=1, threads=4)
        return disp, bgr, poses, Q, merged
    return memo(("ranks", size), make)


def two_ranks(ctx, size, body):
    """ctx holds the first half of the frames, a second context the other half"""
    disp, bgr, poses, Q, _ = rank_case(size)
    h = RANK_FRAMES // 2
    with hooked_context() as other:
        for c, sl in ((ctx, slice(0, h)), (other, slice(h, None))):
            c.set_camera(Q)
            c.set_params(params(jump_pixels=1, voxel_size=VS))
            c.cloudBigReset()
            c.accumulateFrames(disp[sl], bgr[sl], poses[sl])
        try:
            return body([ctx, other])
        finally:
            ctx.cloudBigReset()


def exchange_by_hand(ctxs, counts, sends, gmin, gmax):
    outs = []
    for dst, c in enumerate(ctxs):
        c.cloudBigReset()
        for src in range(len(ctxs)):  # segments in source-rank order
            off = sum(counts[src][:dst])
            seg = sends[src][off: off + counts[src][dst]]
            if len(seg):
                c.cloudBigAppend(seg)
        outs.append(c.finalize(gmin=gmin, gmax=gmax, return_status=True))
    return outs


@case("partition", "o3dr_cloud_big_header_dev", "o3dr_cloud_big_partition", "o3dr_cloud_big_partition_dev", "o3dr_finalize_global")
class _Partition:
    """tests/test_gpu_parity.py::_virtual_rank_merge with two ranks: rank 0 partitions through the headers in HBM, rank 1 by
    the host box, and rank 0 once more by the host box on a copy of its cloud"""

    def call(ctx, size):
        import torch
        from online_3d_reconstruction_amd.dist import _parse_headers

        def body(ctxs):
            hdrs = [c.cloudBigHeaderDev() for c in ctxs]
            torch.cuda.synchronize()
            all_hdrs = torch.cat(hdrs)
            gmin, gmax, hcounts = _parse_headers(all_hdrs.cpu().numpy(), 2)
            before = ctxs[0].cloudBigRead()
            row = ctxs[0].cloudBigPartitionDev(all_hdrs, 2)
            ctxs[0].synchronize()
            row = [int(v) for v in row.cpu().tolist()]
            counts = [row[:2], None]
            sends = [ctxs[0].cloudBigRead(), None]
            counts[1], st1 = ctxs[1].cloudBigPartition(gmin, gmax, 2)
            sends[1] = ctxs[1].cloudBigRead()
            ctxs[0].cloudBigReset()
            ctxs[0].cloudBigAppend(before)
            again = ctxs[0].cloudBigPartition(gmin, gmax, 2)
            sends_again = ctxs[0].cloudBigRead()
            merged = exchange_by_hand(ctxs, counts, sends, gmin, gmax)
            return all_hdrs, row, st1, counts, sends, again, sends_again, merged
        return two_ranks(ctx, size, body)

    def check(size, outs):
        all_hdrs, row, st1, counts, sends, again, sends_again, merged = outs
        assert row[2] == 0 and st1 == 0 and again == (counts[0], 0)
        assert_points_equal(sends_again, sends[0], "the two forms of the partition")
        assert all(sum(counts[r]) == len(sends[r]) for r in (0, 1)) and min(counts[0] + counts[1]) > 0
        assert all(st == 0 for _, st in merged)
        assert_points_equal(np.concatenate([m for m, _ in merged]), rank_case(size)[4], f"partitioned merge {size}")


@case("two_phase_partition", "o3dr_cloud_big_slice_counts_dev", "o3dr_cloud_big_assume_size", "o3dr_cloud_big_place_slices",
      "o3dr_cloud_big_raw_view", "o3dr_cloud_big_set_size")
class _TwoPhase:
    """tests/test_gpu_parity.py::test_two_phase_partition_virtual_ranks with two ranks"""

    def call(ctx, size):
        import torch
        from online_3d_reconstruction_amd.dist import _parse_headers

        def body(ctxs):
            hdrs = [c.cloudBigHeaderDev() for c in ctxs]
            torch.cuda.synchronize()
            all_hdrs = torch.cat(hdrs)
            gmin, gmax, hcounts = _parse_headers(all_hdrs.cpu().numpy(), 2)
            rows = []
            for c in ctxs:
                row = c.cloudBigSliceCountsDev(all_hdrs, 2)
                c.synchronize()
                rows.append([int(v) for v in row.cpu().tolist()])
            sends = np.array([r[:2] for r in rows], np.int64)  # sends[s, r]
            raws, starts = [], []
            for r, c in enumerate(ctxs):
                n_before, n_after = int(sends[:r, r].sum()), int(sends[r + 1:, r].sum())
                c.cloudBigAssumeSize(int(hcounts[r]))
                starts.append(c.cloudBigPlaceSlices(r, rows[r][:2], n_before, n_after))
                raws.append(c.cloudBigRawView())
            torch.cuda.synchronize()
            # (rank 0's own slice and the slice that leaves; the gap between them is whatever the buffer held)
            placed = torch.cat([raws[0][: int(sends[0, 0])], raws[0][starts[0]: starts[0] + int(sends[0, 1])]])
            raws[0][int(sends[0, 0]): int(sends[0, 0]) + int(sends[1, 0])] = raws[1][starts[1]: starts[1] + int(sends[1, 0])]
            raws[1][: int(sends[0, 1])] = raws[0][starts[0]: starts[0] + int(sends[0, 1])]
            torch.cuda.synchronize()
            merged = []
            for r, c in enumerate(ctxs):
                c.cloudBigSetSize(int(sends[:, r].sum()))
                merged.append(c.finalize(gmin=gmin, gmax=gmax, return_status=True))
            return rows, starts, placed, merged
        return two_ranks(ctx, size, body)

    def check(size, outs):
        rows, starts, placed, merged = outs
        assert all(r[2] == 0 and min(r[:2]) > 0 for r in rows) and all(st == 0 for _, st in merged)
        assert starts[0] == rows[0][0] + rows[1][0]
        assert_points_equal(np.concatenate([m for m, _ in merged]), rank_case(size)[4], f"two-phase partition {size}")


@case("merge_partitioned", "o3dr_merge_partitioned", "o3dr_merge_partitioned_stats")
class _MergePartitioned:
    """o3dr_merge_partitioned's own code over the local transport of include/o3dr_testing.h (RCCL refuses two ranks on one
    device; only the two transport primitives differ), one host thread a rank, twice: the second exchange reuses the
    buffers the first one grew"""

    def call(ctx, size):
        from online_3d_reconstruction_amd import POINT, _lib as L
        lib = L.load_library()
        merged = rank_case(size)[4]

        def body(ctxs):
            comm = C.c_void_p()
            L.check(lib.o3dr_test_local_comm_create(2, C.byref(comm)))
            res = [[], []]

            def run(r):
                out = np.zeros(len(merged) + 64, POINT)
                n, tot, st = C.c_int64(0), C.c_int64(0), C.c_uint32(0)
                rc = lib.o3dr_test_merge_partitioned_local(ctxs[r]._h, comm, r, 1, out.ctypes.data, len(out), C.byref(n), C.byref(tot),
                                                           C.byref(st), L.MEM_HOST)
                res[r].append((rc, tot.value, st.value, out[: n.value].copy(), ctxs[r].mergePartitionedStats()))
            try:
                for _ in range(2):
                    th = [threading.Thread(target=run, args=(r,)) for r in (0, 1)]
                    for t in th:
                        t.start()
                    for t in th:
                        t.join(120)
                    assert not any(t.is_alive() for t in th), "a rank is stuck inside the exchange"
            finally:
                lib.o3dr_test_local_comm_destroy(comm)
            return res[0]
        return two_ranks(ctx, size, body)

    def check(size, outs):
        for k, (rc, tot, st, out, stats) in enumerate(outs):
            assert rc == 0 and st == 0 and tot == stats["points_all_ranks"] and (stats["points_sent_off_rank"] > 0) == (k == 0)
            assert_points_equal(out, rank_case(size)[4], f"merge_partitioned {size}, exchange {k}")


# ---- the table against the header ------------------------------------------------------------------------------------------------------
_NO_KERNEL = "launches no kernel and touches no scratch: "
NOT_COVERED = {
    "o3dr_version": _NO_KERNEL + "a constant",
    "o3dr_last_error": _NO_KERNEL + "a host string",
    "o3dr_ctx_create": _NO_KERNEL + "allocations and the counters' first memsets",
    "o3dr_ctx_destroy": _NO_KERNEL + "frees",
    "o3dr_ctx_set_stream": _NO_KERNEL + "a stream handle",
    "o3dr_ctx_synchronize": _NO_KERNEL + "a stream wait",
    "o3dr_set_camera": _NO_KERNEL + "host matrix and one upload of the cached Q table (state)",
    "o3dr_set_params": _NO_KERNEL + "host struct",
    "o3dr_get_params": _NO_KERNEL + "host struct",
    "o3dr_max_points": _NO_KERNEL + "a size query",
    "o3dr_comm_init_all": _NO_KERNEL + "RCCL communicators",
    "o3dr_comm_destroy": _NO_KERNEL + "RCCL communicators",
    "o3dr_host_register": _NO_KERNEL + "pins host memory",
    "o3dr_host_unregister": _NO_KERNEL + "unpins host memory",
    "o3dr_nearby_frames": _NO_KERNEL + "host arithmetic",
    "o3dr_multiview_homographies": _NO_KERNEL + "host arithmetic on the stored camera",
    "o3dr_orb_pattern": _NO_KERNEL + "host table",
    "o3dr_orb_level_sizes": _NO_KERNEL + "a size query",
    "o3dr_profile_enable": _NO_KERNEL + "host flags",
    "o3dr_profile_read": _NO_KERNEL + "event times",
    "o3dr_profile_reset": _NO_KERNEL + "host counters and a memset of the statistics (state)",
    "o3dr_profile_stats": _NO_KERNEL + "a copy of the statistics (state)",
    "o3dr_device_info": _NO_KERNEL + "device properties",
}


def test_every_entry_point_has_a_case_or_a_reason():
    from online_3d_reconstruction_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "o3dr.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(o3dr_[a-z0-9_]+)\s*\(", header))
    names = [n for n, _, _ in _lib.SYMBOLS if n in declared]
    assert len(names) > 80 and "o3dr_test_fill_scratch" not in names
    covered = {e for c in CASES.values() for e in c.entries}
    for n in names:
        if n.endswith("_default_params"):  # fills a host struct
            assert n not in covered
            continue
        assert (n in covered) != (n in NOT_COVERED), f"{n}: a case in CASES or a reason in NOT_COVERED (and not both)"
    assert covered <= set(names) and set(NOT_COVERED) <= set(names)
    assert all(r.startswith(_NO_KERNEL) for r in NOT_COVERED.values())


def test_fill_hook_needs_a_context():
    from online_3d_reconstruction_amd import _lib as L
    n = C.c_int64(7)
    assert L.load_library().o3dr_test_fill_scratch(None, 0, C.byref(n)) == L.ERR_INVALID_ARG and n.value == 0


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------------
_SOLO = {}


def solo(name, size):
    """(outputs, their bytes) of one call on a context of its own, checked against the operator's reference; once"""
    if (name, size) not in _SOLO:
        with hooked_context() as ctx:
            outs = CASES[name].call(ctx, size)
        CASES[name].check(size, outs)
        _SOLO[(name, size)] = blob(outs)
    return _SOLO[(name, size)]


@pytest.mark.gpu
def test_fill_hook_guards(monkeypatch):
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    lib = L.load_library()
    n = C.c_int64(7)
    monkeypatch.delenv("O3DR_TEST_HOOKS", raising=False)
    with o3dr.Context(0) as c:
        assert lib.o3dr_test_fill_scratch(c._h, 0xFF, C.byref(n)) == L.ERR_INVALID_ARG and n.value == 0
        assert b"test hooks are off" in lib.o3dr_last_error()
    with hooked_context() as c:
        for byte in (-1, 256):
            n.value = 7
            assert lib.o3dr_test_fill_scratch(c._h, byte, C.byref(n)) == L.ERR_INVALID_ARG and n.value == 0
        assert lib.o3dr_test_fill_scratch(c._h, 0, None) == L.ERR_INVALID_ARG
        first = fill(c, 0xA5)
        assert first >= 4096  # a new context owns the misc block and the single-shot counters
        c.voxelGrid(cloud("large"), (0.05, 0.05, 0.05))
        assert fill(c, 0xA5) > first + 16 * len(cloud("large"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_filled_scratch(name):
    a = solo(name, "small")
    with hooked_context() as ctx:
        first = blob(CASES[name].call(ctx, "small"))
        n_ff = fill(ctx, 0xFF)
        b = blob(CASES[name].call(ctx, "small"))
        n_00 = fill(ctx, 0x00)
        c = blob(CASES[name].call(ctx, "small"))
    assert n_ff > 0 and n_00 > 0
    assert first == a, "the same call on two new contexts"
    assert b == a, "after 0xFF over the scratch"
    assert c == a, "after 0x00 over the scratch"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_large_then_small(name):
    want = {s: solo(name, s) for s in SIZES}
    with hooked_context() as ctx:
        got = [blob(CASES[name].call(ctx, s)) for s in ("large", "small", "large")]
    assert got[0] == want["large"], "large on a new context"
    assert got[1] == want["small"], "small after large"
    assert got[2] == want["large"], "large after small"


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(minpts=3, sor=True, kp=True)], ids=["plain", "keypoints-sor-min3"])
@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_state_survives_the_fill(byte, kw):
    """the fill between any two of the frame calls, the incremental merges, the merge and the reads: the cloud, its box,
    its recorded run heads and the incremental state are not scratch"""
    jump = 15 if kw else MERGE_JUMP["small"]
    with hooked_context() as ctx:
        plain = merge_run(ctx, jump, **kw)
    merge_check(plain, jump, **kw)
    filled = []
    with hooked_context() as ctx:
        got = merge_run(ctx, jump, between=lambda: filled.append(fill(ctx, byte)), **kw)
    assert len(filled) == 9 and min(filled) > 0
    assert blob(got) == blob(plain)


@pytest.mark.gpu
def test_a_pending_slice_table_does_not_outlive_a_call_that_uses_the_workspace():
    """o3dr_cloud_big_slice_counts_dev leaves its (slice, tile) table in the sort workspace for o3dr_cloud_big_place_slices;
    the fill, and any call that lays the workspace out again, drops it: the placement then asks for the counts again
    instead of moving points by what the workspace holds now"""
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    pts = cloud("large")
    for spoil in (lambda c: fill(c, 0xFF), lambda c: c.voxelGrid(cloud("small"), (0.05, 0.05, 0.05)), None):
        with hooked_context() as ctx:
            ctx.set_params(params(voxel_size=VS))
            ctx.cloudBigAppend(pts)
            hdr = ctx.cloudBigHeaderDev()
            row = ctx.cloudBigSliceCountsDev(hdr, 2)
            ctx.synchronize()
            row = [int(v) for v in row.cpu().tolist()]
            assert row[2] == 0 and sum(row[:2]) == len(pts) and min(row[:2]) > 0
            if spoil is None:
                assert ctx.cloudBigPlaceSlices(0, row[:2], 0, 5) == row[0] + 5
                continue
            spoil(ctx)
            with pytest.raises(o3dr.O3drError) as e:
                ctx.cloudBigPlaceSlices(0, row[:2], 0, 5)
            assert e.value.code == L.ERR_INVALID_ARG
            assert_points_equal(ctx.cloudBigRead(), pts, "the cloud is as it was")


@pytest.mark.gpu
def test_round_robin_of_all_operators():
    want = {name: solo(name, "small") for name in CASES}
    with hooked_context() as ctx:
        for order in (list(CASES), list(CASES)[::-1]):
            for name in order:
                assert blob(CASES[name].call(ctx, "small")) == want[name], f"{name} after {order[:order.index(name)][-3:]}"
