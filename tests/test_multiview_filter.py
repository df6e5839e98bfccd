"""GPU tests of o3dr_multiview_filter / Context.multiviewFilter (include/o3dr.h "multi-view filter"): out, support, violations
and every info field bit for bit against tests/multiview_reference.py, at the smallest shapes at which the kernel can go
wrong.  The kernel's tile is 32 x 8 pixels (kMvTileX x kMvTileY, one pixel per lane, a wave covers 32 x 2): 67 x 131 and
131 x 67 have at least two tile borders in each axis, 33 x 70 has a one-pixel and a six-pixel remainder tile.

Every multi-tile scene with neighbour tests is first checked on the CPU, by the reference alone: each of the five test
classes must occur, and both removal reasons.  Three exceptions follow from the contract itself and are computed, not
observed: at tolerance 0 no test is a support (dp is never an exact level); with min_support = 0 nothing is removed for
lack of support; and a pixel is removed for its violations only where s supports and v violations with s >= min_support
that fail the rule fit into k tests (s = v = min_support under the majority rule, v = max_violations + 1 otherwise)."""
import ctypes as C

import numpy as np
import pytest

import multiview_reference as R

pytestmark = pytest.mark.gpu

U8, U16, F64 = np.uint8, np.uint16, np.float64


@pytest.fixture(scope="module")
def mv():
    """a context of this module's own: every case sets the camera of its image size"""
    import online_3d_reconstruction_amd as o3dr
    c = o3dr.Context(0)
    yield c
    c.close()


def scene(rows, cols, F, seed, dtype=U8, max_shift=0.08):
    """the planted-blob plane scene with 10 % of the pixels zeroed: a 5 x 5 blob 10 levels nearer in frame 1 and one 10
    levels farther in the last frame, where the image has room for them"""
    blobs = []
    if rows >= 16 and cols >= 16 and F >= 2:
        blobs = [(1, rows // 2 - 2, cols // 2 - 2, +10), (F - 1, rows // 4, (3 * cols) // 4 - 2, -10)]
    disp, Q, poses, _ = R.plane_scene(rows, cols, F, seed, dtype, holes=0.1, blobs=blobs, max_shift=max_shift)
    return disp, Q, poses


# rows, cols, F, k, dtype, tolerance, min_support, max_violations, seed
MULTI_TILE = [
    (67, 131, 4, 3, U8, 1.0, 1, -1, 0),
    (131, 67, 4, 3, U16, 0.5, 2, 0, 1),
    (67, 131, 2, 1, F64, 1.0, 0, -1, 2),
    (33, 70, 4, 3, U8, 0.0, 0, 1, 3),
    (131, 67, 4, 3, U8, 0.5, 1, 1, 4),
]
SMALL = [
    (1, 1, 4, 3, U8, 1.0, 1, -1, 5),
    (1, 40, 4, 3, U8, 1.0, 1, -1, 6),
    (40, 1, 4, 3, U16, 1.0, 1, -1, 7),
    (7, 9, 2, 1, F64, 1.0, 1, 0, 8),
    (7, 9, 4, 3, U8, 0.5, 2, -1, 9),
]
_refs = {}


def case(c):
    """(disp, Q, poses, neighbours, the reference's four results) of a case, computed once"""
    if c not in _refs:
        rows, cols, F, k, dtype, tol, ms, mv_, seed = c
        disp, Q, poses = scene(rows, cols, F, seed, dtype, max_shift=0.08 if min(rows, cols) >= 16 else 0.002)
        nb = R.nearby_frames(poses, k)
        _refs[c] = (disp, Q, poses, nb, R.multiview_filter(disp, Q, poses, nb, tol, ms, mv_))
    return _refs[c]


def expected_classes_and_reasons(k, tol, ms, mv_):
    classes = ["n_outside", "n_hole", "n_violation", "n_occluded"] + (["n_support"] if tol > 0 else [])
    need = 2 * ms if mv_ < 0 else ms + mv_ + 1  # the fewest tests of a pixel that is removed for its violations
    reasons = (["n_no_support"] if ms >= 1 else []) + (["n_violated"] if need <= k else [])
    return classes, reasons


def run(ctx, disp, Q, poses, nb, tol=1.0, ms=1, mv_=-1):
    ctx.set_camera(Q)
    return ctx.multiviewFilter(disp, poses, nb, tolerance=tol, min_support=ms, max_violations=mv_, return_support=True,
                               return_violations=True, return_info=True)


def same(got, want, what=""):
    out, sup, vio, info = (g.cpu().numpy() if hasattr(g, "cpu") else g for g in got)
    assert out.dtype == want[0].dtype and np.array_equal(out.view(np.uint8), want[0].view(np.uint8)), f"{what}: out"  # (bits: NaN too)
    assert np.array_equal(sup, want[1]), f"{what}: support"
    assert np.array_equal(vio, want[2]), f"{what}: violations"
    assert [tuple(getattr(i, n) for n in R.Info._fields) for i in info] == [tuple(w) for w in want[3]], f"{what}: info"


@pytest.mark.parametrize("c", MULTI_TILE, ids=lambda c: "%dx%d-F%d-k%d-%s-t%g-s%d-v%d" % (c[:4] + (np.dtype(c[4]).name,) + c[5:8]))
def test_plane_scenes_over_several_tiles(mv, c):
    disp, Q, poses, nb, want = case(c)
    classes, reasons = expected_classes_and_reasons(c[3], c[5], c[6], c[7])
    totals = {n: sum(getattr(i, n) for i in want[3]) for n in R.Info._fields}
    print(totals)
    assert all(totals[n] > 0 for n in classes + reasons), (totals, classes, reasons)  # the CPU-side condition
    assert totals["n_kept"] > 0
    same(run(mv, disp, Q, poses, nb, c[5], c[6], c[7]), want)


@pytest.mark.parametrize("c", SMALL, ids=lambda c: "%dx%d-F%d-k%d-%s" % (c[:4] + (np.dtype(c[4]).name,)))
def test_small_shapes(mv, c):
    disp, Q, poses, nb, want = case(c)
    same(run(mv, disp, Q, poses, nb, c[5], c[6], c[7]), want)


def test_noise_hits_every_branch_at_every_pixel(mv):
    _, Q, poses = scene(67, 131, 4, 10)
    nb = R.nearby_frames(poses, 3)
    rng = np.random.default_rng(11)
    noise = rng.integers(0, 256, (4, 67, 131)).astype(U8)
    noise[rng.random(noise.shape) < 0.2] = 0
    want = R.multiview_filter(noise, Q, poses, nb, 20.0, 1, -1)
    assert all(sum(getattr(i, n) for i in want[3]) > 0 for n in R.Info._fields)
    same(run(mv, noise, Q, poses, nb, 20.0), want, "uint8 noise")
    # float64 levels between the values no level can have: NaN, the infinities, zero, negatives, a denormal
    f = rng.uniform(60.0, 160.0, (4, 67, 131))
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -3.0, 5e-324, 1e300])
    hit = rng.random(f.shape) < 0.2
    f[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    want = R.multiview_filter(f, Q, poses, nb, 20.0, 1, 1)
    assert all(sum(getattr(i, n) for i in want[3]) > 0 for n in R.Info._fields)
    same(run(mv, f, Q, poses, nb, 20.0, 1, 1), want, "float64 noise")


def test_a_gap_and_a_duplicate_in_the_neighbour_list(mv):
    disp, Q, poses, nb, want = case(MULTI_TILE[0])
    gap = nb.copy()
    gap[:, 1] = -1
    ref_gap = R.multiview_filter(disp, Q, poses, gap)
    same(run(mv, disp, Q, poses, gap), ref_gap, "-1 in the middle")
    same(run(mv, disp, Q, poses, np.ascontiguousarray(nb[:, [0, 2]])), ref_gap, "the same lists without the gap")
    dup = nb.copy()
    dup[:, 1] = dup[:, 0]
    ref_dup = R.multiview_filter(disp, Q, poses, dup)
    assert ref_dup[1].max() == 3 and not np.array_equal(ref_dup[1], want[1])  # a frame listed twice votes twice
    same(run(mv, disp, Q, poses, dup), ref_dup, "duplicate")


def test_homographies_are_the_references(mv):
    import online_3d_reconstruction_amd as o3dr
    disp, Q, poses, nb, _ = case(MULTI_TILE[0])
    mv.set_camera(Q)
    nb = nb.copy()
    nb[2, 1] = -1
    H = mv.multiviewHomographies(poses, nb)
    assert H.shape == (4, 3, 4, 4) and H.dtype == np.float64
    assert np.array_equal(H, R.homographies(Q, poses, nb)) and not H[2, 1].any() and H[0, 0].any()
    assert np.array_equal(o3dr.nearbyFrames(poses, 3), R.nearby_frames(poses, 3))
    assert np.array_equal(o3dr.nearbyFrames(poses, 2, 0.1), R.nearby_frames(poses, 2, 0.1))
    # the bundled rig's camera and the track's poses, 40 m apart
    from online_3d_reconstruction_amd import synth
    Qb, track = synth.camera_Q(), synth.make_poses(0, 6)
    mv.set_camera(Qb)
    nbt = R.nearby_frames(track, 4, 2.5)
    assert (nbt == -1).any() and np.array_equal(o3dr.nearbyFrames(track, 4, 2.5), nbt)
    assert np.array_equal(mv.multiviewHomographies(track, nbt), R.homographies(Qb, track, nbt))


def test_layouts_and_batchings_agree(mv):
    import torch
    for c in (MULTI_TILE[0], MULTI_TILE[1], MULTI_TILE[2]):
        disp, Q, poses, nb, want = case(c)
        F, rows, cols = disp.shape
        tol, ms, mv_ = c[5:8]
        # a CUDA tensor
        t = torch.from_numpy(disp.view(np.int16) if disp.dtype == U16 else disp).cuda()
        got = run(mv, t, Q, poses, nb, tol, ms, mv_)
        assert got[0].is_cuda and got[1].is_cuda and got[0].dtype == t.dtype
        same((got[0].cpu().numpy().view(disp.dtype),) + got[1:], want, "CUDA")
        # a padded pitch and frame stride, on the host and on the device
        big = np.full((F, rows + 3, cols + 5), 77, disp.dtype)
        big[:, :rows, :cols] = disp
        view = big[:, :rows, :cols]
        assert not view.flags.c_contiguous
        same(run(mv, view, Q, poses, nb, tol, ms, mv_), want, "padded host")
        tbig = torch.from_numpy(big.view(np.int16) if disp.dtype == U16 else big).cuda()
        got = run(mv, tbig[:, :rows, :cols], Q, poses, nb, tol, ms, mv_)
        same((got[0].cpu().numpy().view(disp.dtype),) + got[1:], want, "padded CUDA")
        # a fifth, unrelated frame appended: the first frames do not change
        extra = np.concatenate([disp, np.full((1, rows, cols), 50, disp.dtype)])
        poses5 = np.concatenate([poses, poses[:1]])
        poses5[-1, :3, 3] += 1000.0
        nb5 = np.concatenate([nb, np.full((1, nb.shape[1]), -1, np.int32)])
        got = run(mv, extra, Q, poses5, nb5, tol, ms, mv_)
        same((got[0][:F], got[1][:F], got[2][:F], got[3][:F]), want, "one frame more")
        assert got[3][F].n_valid == rows * cols and got[3][F].n_outside == 0


def test_without_neighbours_the_rule_alone_decides(mv):
    disp, Q, poses, nb, _ = case(MULTI_TILE[0])
    valid = disp != 0
    for d, p, kw in ((disp[:1], poses[:1], dict(neighbors=np.zeros((1, 0), np.int32))),          # F = 1, k = 0
                     (disp[:1], poses[:1], dict(k=3)),                                            # F = 1: nearbyFrames finds nobody
                     (disp, poses, dict(neighbors=np.zeros((4, 0), np.int32))),                   # k = 0
                     (disp, poses, dict(neighbors=np.full((4, 3), -1, np.int32)))):
        mv.set_camera(Q)
        out, sup, vio, info = mv.multiviewFilter(d, p, min_support=1, return_support=True, return_violations=True, return_info=True, **kw)
        assert not out.any() and not sup.any() and not vio.any()
        assert [i.n_no_support for i in info] == [int(v.sum()) for v in valid[:len(d)]] and all(i.n_kept == 0 and i.n_outside == 0 for i in info)
        out, info = mv.multiviewFilter(d, p, min_support=0, max_violations=0, return_info=True, **kw)
        assert np.array_equal(out, d) and [i.n_kept for i in info] == [i.n_valid for i in info]


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
    disp, Q, poses, nb, want = case((7, 9, 4, 3, U8, 0.5, 2, -1, 9))
    F, H, W = disp.shape
    good = dict(elem_bytes=1, tolerance=0.5, min_support=2, max_violations=-1)
    poses = np.ascontiguousarray(poses, np.float32)

    def call(E=1, pitch=None, fs=None, rows=H, cols=W, n_frames=F, k=3, mem=0, in_shift=0, out_shift=0, nbs=nb, overlap=False, **kw):
        prm = L.MultiviewParamsStruct(**{**good, "elem_bytes": E, **kw})
        B = E if E in (1, 2, 8) else 1  # (the bytes the buffers are made for)
        src = np.zeros(F * H * W * B + 16, np.uint8)
        src[in_shift:in_shift + F * H * W * B] = disp.astype({1: U8, 2: U16, 8: F64}[B]).view(np.uint8).ravel()
        raw = [np.full(F * H * W * e + 16, 0x5A, np.uint8) for e in (B, 1, 1)]
        out, sup, vio = (r[s:s + F * H * W * e] for r, s, e in zip(raw, (out_shift, 0, 0), (B, 1, 1)))
        info = (L.MultiviewInfoStruct * F)()
        for i in info:
            i.n_valid = i.n_occluded = 0x5A
        nbs = np.ascontiguousarray(nbs, np.int32)
        pitch = W * B if pitch is None else pitch
        fs = H * W * B if fs is None else fs
        dst = src[in_shift + 8:] if overlap else out
        rc = lib.o3dr_multiview_filter(mv._h, src[in_shift:].ctypes.data, fs, pitch, rows, cols, n_frames, poses.ctypes.data, nbs.ctypes.data, k,
                                       C.byref(prm), dst.ctypes.data, sup.ctypes.data, vio.ctypes.data, C.cast(info, C.c_void_p), mem)
        return rc, out, sup, vio, info

    mv.set_camera(Q)
    rc, out, sup, vio, info = call()
    assert rc == 0 and np.array_equal(out.reshape(F, H, W), want[0]) and np.array_equal(sup.reshape(F, H, W), want[1])
    assert [i.n_kept for i in info] == [w.n_kept for w in want[3]]
    rc, out, sup, vio, info = call(n_frames=0)  # O3DR_OK, nothing touched
    assert rc == 0 and (out == 0x5A).all() and (sup == 0x5A).all() and info[0].n_valid == 0x5A

    def listed(i, n, v):
        m = nb.copy()
        m[i, n] = v
        return m

    mv.profileEnable(-1, True)
    mv.profileReset()
    bad = [dict(E=0), dict(E=3), dict(E=4), dict(k=17), dict(k=-1), dict(nbs=listed(2, 1, 2)), dict(nbs=listed(0, 0, F)),
           dict(nbs=listed(3, 2, -2)), dict(tolerance=-0.5), dict(tolerance=float("nan")), dict(tolerance=float("inf")),
           dict(min_support=-1), dict(min_support=17), dict(max_violations=-2), dict(max_violations=17), dict(overlap=True),
           dict(E=2, in_shift=1), dict(E=2, out_shift=1), dict(E=2, pitch=2 * W + 1), dict(E=8, in_shift=4), dict(E=8, out_shift=2),
           dict(E=8, fs=8 * H * W + 4), dict(pitch=W - 1), dict(fs=H * W - 1), dict(mem=2)]
    for kw in bad:
        rc, out, sup, vio, info = call(**kw)
        assert rc == L.ERR_INVALID_ARG, kw
        if kw.get("mem") != 2:  # (an unknown memory kind is no host memory: nothing is written)
            assert not sup.any() and not vio.any() and all(i.n_valid == 0 and i.n_occluded == 0 for i in info), kw
            if kw.get("E", 1) in (1, 2, 8) and not kw.get("overlap"):  # (the size of `out` is known only with a valid element size)
                assert not out.any(), kw
    mv.set_camera(np.array([[1, 0, 0, -4.0], [0, 1, 0, -3.0], [0, 0, 0, 4230.0], [0, 0, 0, 0]]))  # a singular Q
    rc, out, sup, vio, info = call()
    assert rc == L.ERR_INVALID_ARG and not out.any() and not sup.any()
    Hm = np.full((F, 3, 16), 7.0)
    assert lib.o3dr_multiview_homographies(mv._h, poses.ctypes.data, F, np.ascontiguousarray(nb).ctypes.data, 3, Hm.ctypes.data) == L.ERR_INVALID_ARG
    assert not Hm.any()
    mv.set_camera(Q)
    for kw in (dict(rows=0), dict(cols=0), dict(rows=8193), dict(cols=8193), dict(n_frames=-1)):  # sizes unknown: nothing is written
        rc, out, sup, vio, info = call(**kw)
        assert rc == L.ERR_INVALID_ARG and (out == 0x5A).all() and (sup == 0x5A).all(), kw
    buf = np.zeros(F * H * W, np.uint8)
    src = np.ascontiguousarray(disp)
    args = (H * W, W, H, W, F, poses.ctypes.data, np.ascontiguousarray(nb).ctypes.data, 3, None)
    assert lib.o3dr_multiview_filter(mv._h, None, *args, buf.ctypes.data, None, None, None, 0) == L.ERR_INVALID_ARG
    assert lib.o3dr_multiview_filter(mv._h, src.ctypes.data, *args, None, None, None, None, 0) == L.ERR_INVALID_ARG
    assert lib.o3dr_multiview_filter(None, src.ctypes.data, *args, buf.ctypes.data, None, None, None, 0) == L.ERR_INVALID_ARG
    assert lib.o3dr_nearby_frames(poses.ctypes.data, F, 17, 1.0, buf.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.o3dr_nearby_frames(poses.ctypes.data, F, 3, -1.0, buf.ctypes.data) == L.ERR_INVALID_ARG
    assert lib.o3dr_nearby_frames(poses.ctypes.data, F, 3, float("nan"), buf.ctypes.data) == L.ERR_INVALID_ARG
    assert all(mv.profileRead(k)[1] == 0 for k in range(len(L.KERNEL_NAMES))), "a rejected call launched a kernel"
    rc, out = call()[:2]  # the good call still works after the rejected ones
    assert rc == 0 and np.array_equal(out.reshape(F, H, W), want[0]) and mv.profileRead(L.K_MULTIVIEW)[1] == 1
    assert lib.o3dr_multiview_filter(mv._h, src.ctypes.data, *args, buf.ctypes.data, None, None, None, 0) == 0  # p == NULL: the defaults
    assert np.array_equal(buf.reshape(F, H, W), R.multiview_filter(disp, Q, poses.reshape(F, 4, 4), nb)[0]) and not np.array_equal(buf.reshape(F, H, W), want[0])
    mv.profileEnable(-1, False)
    mv.profileReset()
    import online_3d_reconstruction_amd as o3dr
    with o3dr.Context(0) as bare:  # no camera
        with pytest.raises(o3dr.O3drError) as e:
            bare.multiviewFilter(disp, poses, nb)
        assert e.value.code == L.ERR_NOT_CONFIGURED
