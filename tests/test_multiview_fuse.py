"""GPU tests of o3dr_multiview_fuse / Context.multiviewFuse (include/o3dr.h "multi-view fusion"): out (through its bytes),
votes, support, violations and every info field bit for bit against tests/multiview_fuse_reference.py.  The kernel shares
the filter's mapping (a 32 x 8 tile per workgroup, one pixel per lane), so the shapes are the filter tests': 67 x 131 and
131 x 67 have at least two tile borders in each axis, 33 x 70 a one-pixel and a six-pixel remainder tile.  No tolerance:
the fusion adds two products and sums, one division and an ordered sum per support to arithmetic that the filter already
reproduces bit for bit under the same build flags.

The scenes' own conditions are checked on the CPU, by the reference alone, before anything is compared: every vote count
0..3 occurs over the plane scenes, and the deep-baseline noise case has both votes and dropped votes."""
import ctypes as C

import numpy as np
import pytest

import multiview_fuse_reference as RF
import multiview_reference as R
from test_multiview_filter import MULTI_TILE, SMALL, scene

pytestmark = pytest.mark.gpu

U8, U16, F64 = np.uint8, np.uint16, np.float64


@pytest.fixture(scope="module")
def mv():
    """a context of this module's own: every case sets the camera of its image size"""
    import online_3d_reconstruction_amd as o3dr
    c = o3dr.Context(0)
    yield c
    c.close()


_refs = {}


def case(c):
    """(disp, Q, poses, neighbours, the reference's five results) of a case of the filter tests' lists, computed once"""
    if c not in _refs:
        rows, cols, F, k, dtype, tol, ms, mv_, seed = c
        disp, Q, poses = scene(rows, cols, F, seed, dtype, max_shift=0.08 if min(rows, cols) >= 16 else 0.002)
        nb = R.nearby_frames(poses, k)
        _refs[c] = (disp, Q, poses, nb, RF.multiview_fuse(disp, Q, poses, nb, tol, ms, mv_))
    return _refs[c]


def run(ctx, disp, Q, poses, nb, tol=1.0, ms=1, mv_=-1):
    ctx.set_camera(Q)
    return ctx.multiviewFuse(disp, poses, nb, tolerance=tol, min_support=ms, max_violations=mv_, return_votes=True,
                             return_support=True, return_violations=True, return_info=True)


def flat(i):
    return tuple(i.filter) + (i.n_votes, i.n_votes_dropped, i.n_fused)


def same(got, want, what=""):
    import dataclasses
    out, votes, sup, vio, info = (g.cpu().numpy() if hasattr(g, "cpu") else g for g in got)
    assert out.dtype == F64 and out.shape == want[0].shape
    assert np.array_equal(out.view(np.uint8), want[0].view(np.uint8)), f"{what}: out"
    assert np.array_equal(votes, want[1]), f"{what}: votes"
    assert np.array_equal(sup, want[2]), f"{what}: support"
    assert np.array_equal(vio, want[3]), f"{what}: violations"
    got_info = [dataclasses.astuple(i.filter) + (i.n_votes, i.n_votes_dropped, i.n_fused) for i in info]
    assert got_info == [flat(w) for w in want[4]], f"{what}: info"


_ids = ["%dx%d-F%d-k%d-%s-t%g-s%d-v%d" % (c[:4] + (np.dtype(c[4]).name,) + c[5:8]) for c in MULTI_TILE + SMALL]


def test_every_vote_count_occurs_in_the_plane_scenes():
    """the CPU-side condition of the plane cases: with tolerance > 0 every vote count 0..3 occurs at a valid pixel"""
    seen = set()
    for c in MULTI_TILE + SMALL:
        disp, _, _, _, want = case(c)
        valid = R.levels(disp)[1]
        counts = np.bincount(want[1][valid], minlength=4)
        print(c[:4], np.dtype(c[4]).name, c[5:], "votes 0..:", counts.tolist(), "kept", int((want[0] > 0).sum()))
        if c[5] > 0:
            seen |= {int(v) for v in np.nonzero(counts)[0]}
    assert seen >= {0, 1, 2, 3}, seen
    out, votes = case(MULTI_TILE[0])[4][:2]
    assert all(((out > 0) & (votes == n)).any() for n in (1, 2, 3))
    # tolerance = 0: nobody votes, and the output is the kept pixels' own levels
    disp, _, _, _, (out, votes, _, _, infos) = case(MULTI_TILE[3])
    assert not votes.any() and (out > 0).any() and all(i.n_fused == 0 for i in infos)
    assert np.array_equal(out[out > 0], disp[out > 0].astype(F64))


@pytest.mark.parametrize("c", MULTI_TILE + SMALL, ids=_ids)
def test_plane_scenes(mv, c):
    disp, Q, poses, nb, want = case(c)
    same(run(mv, disp, Q, poses, nb, c[5], c[6], c[7]), want)


def deep_scene(dtype):
    """three cameras 20 m above and 12 m below each other looking at noise: at a tolerance of 200 levels nearly every test
    that lands inside is a support, and many of them vote for a level behind the camera or beyond infinity"""
    from online_3d_reconstruction_amd import synth
    rows, cols = 33, 70
    Q = synth.camera_Q(rows, cols)
    poses = np.stack([np.asarray(synth.make_pose(3), np.float32).reshape(4, 4)] * 3).copy()
    for f, dz in enumerate((0.0, 20.0, -12.0)):
        poses[f, 2, 3] += dz
    rng = np.random.default_rng(21)
    if dtype == U8:
        noise = rng.integers(0, 256, (3, rows, cols)).astype(U8)
        noise[rng.random(noise.shape) < 0.1] = 0
    else:
        noise = rng.uniform(1.0, 255.0, (3, rows, cols))
    return noise, Q, poses, R.nearby_frames(poses, 2)


@pytest.mark.parametrize("dtype, ms, mv_", [(U8, 1, -1), (U8, 0, 2), (F64, 1, -1)], ids=["uint8", "uint8-s0-v2", "float64"])
def test_dropped_votes(mv, dtype, ms, mv_):
    noise, Q, poses, nb = deep_scene(dtype)
    want = RF.multiview_fuse(noise, Q, poses, nb, 200.0, ms, mv_)
    n_sup = sum(i.filter.n_support for i in want[4])
    n_votes = sum(i.n_votes for i in want[4])
    kept = want[0] > 0
    print("supports", n_sup, "votes", n_votes, "kept", int(kept.sum()), "kept without a vote", int((kept & (want[1] == 0)).sum()))
    assert 0 < n_votes < n_sup  # the CPU-side condition: both branches
    assert (kept & (want[1] == 0) & (want[2] > 0)).any()  # a kept pixel all of whose supports were dropped
    assert np.isfinite(want[0]).all() and (want[0] >= 0).all()
    same(run(mv, noise, Q, poses, nb, 200.0, ms, mv_), want)


def test_float64_special_values(mv):
    _, Q, poses = scene(67, 131, 4, 10)
    nb = R.nearby_frames(poses, 3)
    rng = np.random.default_rng(11)
    f = rng.uniform(60.0, 160.0, (4, 67, 131))
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -3.0, 5e-324, 1e300])
    hit = rng.random(f.shape) < 0.2
    f[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    want = RF.multiview_fuse(f, Q, poses, nb, 20.0, 1, 1)
    assert all(sum(getattr(i.filter, n) for i in want[4]) > 0 for n in R.Info._fields) and sum(i.n_votes for i in want[4]) > 0
    got = run(mv, f, Q, poses, nb, 20.0, 1, 1)
    same(got, want, "float64 noise")
    assert np.isfinite(got[0]).all() and (got[0] >= 0).all()
    assert not got[0][~R.levels(f)[1]].any() and not got[1][~R.levels(f)[1]].any()  # an invalid pixel: 0.0 and no votes


def test_the_order_of_the_neighbour_list(mv):
    disp, Q, poses, nb, want = case(MULTI_TILE[0])
    gap = nb.copy()
    gap[:, 1] = -1
    ref_gap = RF.multiview_fuse(disp, Q, poses, gap)
    same(run(mv, disp, Q, poses, gap), ref_gap, "-1 in the middle")
    same(run(mv, disp, Q, poses, np.ascontiguousarray(nb[:, [0, 2]])), ref_gap, "the same lists without the gap")
    dup = nb.copy()
    dup[:, 1] = dup[:, 0]
    ref_dup = RF.multiview_fuse(disp, Q, poses, dup)
    assert ref_dup[1].max() == 3 and not np.array_equal(ref_dup[1], want[1])  # a frame listed twice votes twice
    same(run(mv, disp, Q, poses, dup), ref_dup, "duplicate")
    # the lists backwards: the same votes, summed in another order
    swapped = np.ascontiguousarray(nb[:, ::-1])
    ref_sw = RF.multiview_fuse(disp, Q, poses, swapped)
    assert np.array_equal(ref_sw[1], want[1]) and np.array_equal(ref_sw[2], want[2])
    # (at most four positive terms: either order is within 3 roundings of the exact sum, the division adds one each)
    assert np.allclose(ref_sw[0], want[0], rtol=8 * np.finfo(F64).eps, atol=0)
    same(run(mv, disp, Q, poses, swapped), ref_sw, "swapped")


def test_layouts_and_memory_kinds_agree(mv):
    import torch
    for c in (MULTI_TILE[0], MULTI_TILE[1], MULTI_TILE[2]):
        disp, Q, poses, nb, want = case(c)
        F, rows, cols = disp.shape
        tol, ms, mv_ = c[5:8]
        t = torch.from_numpy(disp.view(np.int16) if disp.dtype == U16 else disp).cuda()  # (uint16 bits in an int16 tensor)
        got = run(mv, t, Q, poses, nb, tol, ms, mv_)
        assert all(g.is_cuda for g in got[:4]) and got[0].dtype == torch.float64 and got[1].dtype == torch.uint8
        same(got, want, "CUDA")
        big = np.full((F, rows + 3, cols + 5), 77, disp.dtype)
        big[:, :rows, :cols] = disp
        view = big[:, :rows, :cols]
        assert not view.flags.c_contiguous
        same(run(mv, view, Q, poses, nb, tol, ms, mv_), want, "padded host")
        tbig = torch.from_numpy(big.view(np.int16) if disp.dtype == U16 else big).cuda()
        same(run(mv, tbig[:, :rows, :cols], Q, poses, nb, tol, ms, mv_), want, "padded CUDA")
    # the image alone is returned when nothing else is asked for
    disp, Q, poses, nb, want = case(MULTI_TILE[0])
    mv.set_camera(Q)
    out = mv.multiviewFuse(disp, poses, nb)
    assert isinstance(out, np.ndarray) and np.array_equal(out.view(np.uint8), want[0].view(np.uint8))
    out, info = mv.multiviewFuse(disp, poses, k=3, return_info=True)  # (the neighbours of nearbyFrames)
    assert np.array_equal(out.view(np.uint8), want[0].view(np.uint8)) and [flat(w) for w in want[4]] == \
        [tuple(getattr(i.filter, n) for n in R.Info._fields) + (i.n_votes, i.n_votes_dropped, i.n_fused) for i in info]


def test_one_frame_without_neighbours(mv):
    disp, Q, poses, _, _ = case(MULTI_TILE[0])
    d, p = disp[:1], poses[:1]
    mv.set_camera(Q)
    for kw in (dict(neighbors=np.zeros((1, 0), np.int32)), dict(k=3)):
        out, votes, info = mv.multiviewFuse(d, p, min_support=1, return_votes=True, return_info=True, **kw)
        assert out.dtype == F64 and not out.any() and not votes.any()
        assert info[0].filter.n_no_support == int((d != 0).sum()) and info[0].n_votes == info[0].n_fused == 0
        out, info = mv.multiviewFuse(d, p, min_support=0, max_violations=0, return_info=True, **kw)
        assert np.array_equal(out.view(np.uint8), d.astype(F64).view(np.uint8)) and info[0].filter.n_kept == info[0].filter.n_valid
        assert info[0].n_fused == 0


def test_the_identities_with_the_filter(mv):
    """on the device: the fusion's counts are the filter's, and out > 0 exactly where the filter keeps a pixel"""
    for c in MULTI_TILE:
        disp, Q, poses, nb, _ = case(c)
        mv.set_camera(Q)
        kw = dict(tolerance=c[5], min_support=c[6], max_violations=c[7], return_support=True, return_violations=True, return_info=True)
        f_out, f_sup, f_vio, f_info = mv.multiviewFilter(disp, poses, nb, **kw)
        out, sup, vio, info = mv.multiviewFuse(disp, poses, nb, **kw)
        assert np.array_equal(out > 0, f_out != 0) and np.array_equal(sup, f_sup) and np.array_equal(vio, f_vio)
        assert [i.filter for i in info] == f_info
        assert all(i.n_votes + i.n_votes_dropped == i.filter.n_support for i in info)


def test_launches_depend_on_the_sizes_alone(mv):
    from online_3d_reconstruction_amd import _lib as L
    disp, Q, poses, nb, _ = case(MULTI_TILE[0])
    mv.profileEnable(-1, True)
    try:
        counts = []
        for d in (disp, np.zeros_like(disp), np.full_like(disp, 200)):
            mv.profileReset()
            run(mv, d, Q, poses, nb)
            counts.append([mv.profileRead(k)[1] for k in range(len(L.KERNEL_NAMES))])
        assert counts[0][L.K_MULTIVIEW] == 1 and sum(counts[0]) == 1 and counts[1] == counts[0] and counts[2] == counts[0]
    finally:
        mv.profileEnable(-1, False)
        mv.profileReset()


def test_bad_arguments_zero_host_outputs_and_launch_nothing(mv):
    from online_3d_reconstruction_amd import _lib as L
    lib = L.load_library()
    c9 = (7, 9, 4, 3, U8, 0.5, 2, -1, 9)
    disp, Q, poses, nb, want = case(c9)
    F, H, W = disp.shape
    n = F * H * W
    good = dict(elem_bytes=1, tolerance=0.5, min_support=2, max_violations=-1)
    poses = np.ascontiguousarray(poses, np.float32)

    def call(E=1, pitch=None, fs=None, rows=H, cols=W, n_frames=F, k=3, mem=0, in_shift=0, out_shift=0, nbs=nb, overlap=False, **kw):
        prm = L.MultiviewParamsStruct(**{**good, "elem_bytes": E, **kw})
        B = E if E in (1, 2, 8) else 1  # (the bytes the input is made for)
        arena = np.zeros(n * B + n * 8 + 64, np.uint8)  # (the input, and room for an output that overlaps it)
        src = arena[in_shift:]
        src[:n * B] = disp.astype({1: U8, 2: U16, 8: F64}[B]).view(np.uint8).ravel()
        raw = [np.full(n * e + 16, 0x5A, np.uint8) for e in (8, 1, 1, 1)]
        out, votes, sup, vio = (r[s:s + n * e] for r, s, e in zip(raw, (out_shift, 0, 0, 0), (8, 1, 1, 1)))
        info = (L.MultiviewFuseInfoStruct * F)()
        for i in info:
            i.filter.n_valid = i.n_fused = 0x5A
        nbs = np.ascontiguousarray(nbs, np.int32)
        pitch = W * B if pitch is None else pitch
        fs = H * W * B if fs is None else fs
        dst = arena[in_shift + 8:in_shift + 8 + n * 8] if overlap else out
        rc = lib.o3dr_multiview_fuse(mv._h, src.ctypes.data, fs, pitch, rows, cols, n_frames, poses.ctypes.data, nbs.ctypes.data, k,
                                     C.byref(prm), dst.ctypes.data, votes.ctypes.data, sup.ctypes.data, vio.ctypes.data,
                                     C.cast(info, C.c_void_p), mem)
        return rc, out, votes, sup, vio, info

    def good_call_matches():
        rc, out, votes, sup, vio, info = call()
        assert rc == 0 and np.array_equal(out, want[0].view(np.uint8).ravel()) and np.array_equal(votes.reshape(F, H, W), want[1])
        assert np.array_equal(sup.reshape(F, H, W), want[2]) and [i.n_votes for i in info] == [w.n_votes for w in want[4]]

    mv.set_camera(Q)
    good_call_matches()
    rc, out, votes, sup, vio, info = call(n_frames=0)  # O3DR_OK, nothing touched
    assert rc == 0 and (out == 0x5A).all() and (votes == 0x5A).all() and info[0].n_fused == 0x5A

    def listed(i, m, v):
        a = nb.copy()
        a[i, m] = v
        return a

    mv.profileEnable(-1, True)
    mv.profileReset()
    # the filter's list, then what the float64 output adds: an `out` off its 8-byte alignment whatever the input's element
    # size, and an `out` over the input
    bad = [dict(E=0), dict(E=3), dict(E=4), dict(k=17), dict(k=-1), dict(nbs=listed(2, 1, 2)), dict(nbs=listed(0, 0, F)),
           dict(nbs=listed(3, 2, -2)), dict(tolerance=-0.5), dict(tolerance=float("nan")), dict(tolerance=float("inf")),
           dict(min_support=-1), dict(min_support=17), dict(max_violations=-2), dict(max_violations=17), dict(overlap=True),
           dict(E=2, in_shift=1), dict(E=2, out_shift=2), dict(E=2, pitch=2 * W + 1), dict(E=8, in_shift=4), dict(E=8, out_shift=2),
           dict(E=8, fs=8 * H * W + 4), dict(pitch=W - 1), dict(fs=H * W - 1), dict(mem=2),
           dict(out_shift=1), dict(out_shift=4), dict(E=8, out_shift=4), dict(E=2, overlap=True), dict(E=8, overlap=True)]
    for kw in bad:
        rc, out, votes, sup, vio, info = call(**kw)
        assert rc == L.ERR_INVALID_ARG, kw
        if kw.get("mem") != 2:  # (an unknown memory kind is no host memory: nothing is written)
            assert not votes.any() and not sup.any() and not vio.any(), kw
            assert all(i.filter.n_valid == 0 and i.n_fused == 0 for i in info), kw
            if not kw.get("overlap"):  # (float64 whatever elem_bytes says: the size of `out` is always known)
                assert not out.any(), kw
    mv.set_camera(np.array([[1, 0, 0, -4.0], [0, 1, 0, -3.0], [0, 0, 0, 4230.0], [0, 0, 0, 0]]))  # a singular Q
    rc, out, votes, sup, vio, info = call()
    assert rc == L.ERR_INVALID_ARG and not out.any() and not votes.any()
    mv.set_camera(Q)
    for kw in (dict(rows=0), dict(cols=0), dict(rows=8193), dict(cols=8193), dict(n_frames=-1)):  # sizes unknown: nothing is written
        rc, out, votes, sup, vio, info = call(**kw)
        assert rc == L.ERR_INVALID_ARG and (out == 0x5A).all() and (votes == 0x5A).all(), kw
    buf = np.zeros(n, F64)
    src = np.ascontiguousarray(disp)
    args = (H * W, W, H, W, F, poses.ctypes.data, np.ascontiguousarray(nb).ctypes.data, 3, None)
    assert lib.o3dr_multiview_fuse(mv._h, None, *args, buf.ctypes.data, None, None, None, None, 0) == L.ERR_INVALID_ARG
    assert lib.o3dr_multiview_fuse(mv._h, src.ctypes.data, *args, None, None, None, None, None, 0) == L.ERR_INVALID_ARG
    assert lib.o3dr_multiview_fuse(None, src.ctypes.data, *args, buf.ctypes.data, None, None, None, None, 0) == L.ERR_INVALID_ARG
    assert all(mv.profileRead(k)[1] == 0 for k in range(len(L.KERNEL_NAMES))), "a rejected call launched a kernel"
    good_call_matches()  # the good call still works after the rejected ones
    assert mv.profileRead(L.K_MULTIVIEW)[1] == 1
    assert lib.o3dr_multiview_fuse(mv._h, src.ctypes.data, *args, buf.ctypes.data, None, None, None, None, 0) == 0  # p == NULL: the defaults
    assert np.array_equal(buf.reshape(F, H, W).view(np.uint8), RF.multiview_fuse(disp, Q, poses.reshape(F, 4, 4), nb)[0].view(np.uint8))
    mv.profileEnable(-1, False)
    mv.profileReset()
    import online_3d_reconstruction_amd as o3dr
    with o3dr.Context(0) as bare:  # no camera
        with pytest.raises(o3dr.O3drError) as e:
            bare.multiviewFuse(disp, poses, nb)
        assert e.value.code == L.ERR_NOT_CONFIGURED
