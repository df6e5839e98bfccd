"""GPU tests of o3dr_disparity_filter / Context.filterDisparity (include/o3dr.h "disparity filter"): out, labels, sizes and
every info field bit for bit against tests/disparity_filter_reference.py, at the smallest shapes at which each piece can go
wrong.  The kernels' tile is 64 x 16 pixels: 67 x 131 has two tile borders in x and four in y, 131 x 67 one and eight.
That is 15 to 18 tiles and three workgroups of border pairs; images of 256 tiles are in tests/test_labelling_scale.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import disparity_filter_reference as R

pytestmark = pytest.mark.gpu

FIELDS = ("n_valid", "n_components", "n_speckles", "n_removed", "largest")


def to_np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def reference(img, median=0, size=0, diff=1):
    """per-frame reference of a [H, W] image or a stack -> out, labels, sizes, [Info]"""
    if img.ndim == 2:
        out, labels, sizes, info = R.filter_disparity(img, median, size, diff)
        return out, labels, sizes, [info]
    return R.filter_frames(img, median_size=median, max_speckle_size=size, max_diff=diff)


def run(ctx, img, median=0, size=0, diff=1, **kw):
    return ctx.filterDisparity(img, median, size, diff, return_labels=True, return_sizes=True, return_info=True, **kw)


def check(got, ref, what):
    out, labels, sizes, infos = got
    for name, g, r in (("out", out, ref[0]), ("labels", labels, ref[1]), ("sizes", sizes, ref[2])):
        g = to_np(g)
        if g.dtype == np.int16:
            g = g.view(np.uint16)
        assert g.dtype == r.dtype and g.shape == r.shape, f"{what}: {name} is {g.dtype} {g.shape}, expected {r.dtype} {r.shape}"
        if not np.array_equal(g, r):
            bad = np.argwhere(g != r)[0]
            idx = tuple(int(v) for v in ((0,) * (3 - len(bad)) + tuple(bad)))
            raise AssertionError(f"{what}: {name} differs first at (frame, y, x) = {idx}: {g[tuple(bad)]} vs {r[tuple(bad)]}, "
                                 f"{int((g != r).sum())} pixels in all")
    assert len(infos) == len(ref[3])
    for f, (gi, ri) in enumerate(zip(infos, ref[3])):
        for k in FIELDS:
            assert getattr(gi, k) == getattr(ri, k), f"{what}: info[{f}].{k} = {getattr(gi, k)}, expected {getattr(ri, k)}"


def levels(H, W, dtype, seed, hi=4):
    """random values in {0..hi-1}; uint16: times 20000, so that one level is 1 (uint8) or 20000 (uint16) apart"""
    v = np.random.RandomState(seed).randint(0, hi, (H, W))
    return (v * (20000 if dtype == np.uint16 else 1)).astype(dtype)


def unit(dtype):
    return 20000 if dtype == np.uint16 else 1


SHAPES = [(1, 1), (1, 40), (40, 1), (2, 2), (7, 9), (33, 70), (70, 33), (67, 131)]


@functools.lru_cache(maxsize=None)
def shape_case(H, W, median, dt):
    img = levels(H, W, np.dtype(dt).type, seed=H * 1000 + W)
    img.setflags(write=False)
    return img, reference(img, median, 3, unit(np.dtype(dt).type))


@pytest.mark.parametrize("dt", ["uint8", "uint16"])
@pytest.mark.parametrize("median", [0, 3, 5])
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_matches_the_reference(ctx, H, W, median, dt):
    img, ref = shape_case(H, W, median, dt)
    check(run(ctx, img, median, 3, unit(img.dtype.type)), ref, f"{H}x{W} median {median} {dt}")


@pytest.mark.parametrize("dt", ["uint8", "uint16"])
@pytest.mark.parametrize("median", [3, 5])
def test_median_of_full_range_values(ctx, median, dt):
    """every value of the type, speckle removal off: on uint16 the low byte decides the order as often as the high one,
    which the four levels above never ask of the compare-exchange network"""
    t = np.dtype(dt).type
    img = np.random.RandomState(100 + median).randint(0, int(np.iinfo(t).max) + 1, (67, 131)).astype(t)
    assert len(np.unique(img)) > 250 and (dt == "uint8" or len(np.unique(img & 255)) == 256)
    ref = reference(img, median, 0, 1)
    assert not np.array_equal(ref[0], img)
    check(run(ctx, img, median, 0, 1), ref, f"full range median {median} {dt}")


def checkerboard(H, W):
    img = np.zeros((H, W), np.uint8)
    img[0::2, 0::2] = 9
    img[1::2, 1::2] = 9
    return img


STRESS = {
    "serpentine": lambda H, W: R.serpentine(H, W),
    "serpentine transposed": lambda H, W: np.ascontiguousarray(R.serpentine(W, H).T),
    "comb": lambda H, W: R.comb(H, W),
    "comb upside down": lambda H, W: np.ascontiguousarray(R.comb(H, W)[::-1]),
    "checkerboard": checkerboard,
    "all equal": lambda H, W: np.full((H, W), 77, np.uint8),
    "all zero": lambda H, W: np.zeros((H, W), np.uint8),
}
STRESS_SHAPES = [(67, 131), (40, 70), (131, 67)]


@pytest.mark.parametrize("H,W", STRESS_SHAPES, ids=[f"{h}x{w}" for h, w in STRESS_SHAPES])
@pytest.mark.parametrize("name", list(STRESS))
def test_labelling_stress(ctx, name, H, W):
    img = STRESS[name](H, W)
    assert img.shape == (H, W)
    ref = reference(img, 0, 100, 1)
    check(run(ctx, img, 0, 100, 1), ref, f"{name} {H}x{W}")
    info = ref[3][0]
    if name.startswith(("serpentine", "comb", "all equal")):
        assert info.n_components == 1 and info.largest == info.n_valid and ref[1][img != 0].max() == 0
    if name == "all equal":
        assert info.largest == H * W
    if name == "checkerboard":
        assert info.n_components == info.n_valid == (H * W + 1) // 2 and info.n_removed == info.n_valid
    if name == "all zero":
        assert info == R.Info(0, 0, 0, 0, 0)


@pytest.mark.parametrize("H,W", STRESS_SHAPES, ids=[f"{h}x{w}" for h, w in STRESS_SHAPES])
@pytest.mark.parametrize("diff", [0, 1, 255])
def test_random_levels(ctx, H, W, diff):
    img = levels(H, W, np.uint8, seed=7 * H + W)
    check(run(ctx, img, 0, 4, diff), reference(img, 0, 4, diff), f"random {H}x{W} max_diff {diff}")


def test_the_inputs_bite():
    """the parametrised cases are worth something only if the reference removes some pixels but not all of them, and the
    components come in more than one size"""
    for diff in (0, 1):
        img = levels(67, 131, np.uint8, seed=7 * 67 + 131)
        out, labels, sizes, (info,) = reference(img, 0, 4, diff)
        assert 0 < info.n_removed < info.n_valid and 0 < info.n_speckles < info.n_components
        assert len(np.unique(sizes[sizes > 0])) > 1 and info.largest > 4
    img, ref = shape_case(67, 131, 3, "uint16")
    assert 0 < ref[3][0].n_removed < ref[3][0].n_valid and not np.array_equal(ref[0], img)


def test_thresholds(ctx):
    ramp = R.ramp()
    for diff, n in ((2, 100), (3, 1)):
        ref = reference(ramp, 0, 0, diff)
        assert ref[3][0].n_components == n
        check(run(ctx, ramp, 0, 0, diff), ref, f"ramp max_diff {diff}")
    wide = np.array([[1, 65535], [0, 65535]], np.uint16)
    for diff, n in ((65534, 1), (65533, 2)):
        ref = reference(wide, 0, 0, diff)
        assert ref[3][0].n_components == n
        check(run(ctx, wide, 0, 0, diff), ref, f"1 | 65535 max_diff {diff}")


@pytest.mark.parametrize("corner", [(64, 32), (32, 16)], ids=["corner 64,32", "corner 32,16"])
def test_speckle_size_limit_across_a_tile_corner(ctx, corner):
    """rectangles of exactly max_speckle_size pixels go, of one pixel more stay; one of each straddles the corner"""
    cx, cy = corner
    for extra, stays in ((0, False), (1, True)):
        img = np.full((67, 131), 50, np.uint8)
        img[cy - 2:cy + 2, cx - 3:cx + 3] = 90          # 4 x 6 = 24 pixels, two rows and three columns on each side
        if extra:
            img[cy + 2, cx] = 90                         # 25
        img[3:7, 100:106] = 120                          # the same away from every corner
        if extra:
            img[7, 100] = 120
        ref = reference(img, 0, 24, 1)
        assert ref[3][0].n_speckles == (0 if stays else 2) and ref[3][0].n_removed == (0 if stays else 48)
        assert (ref[0][cy, cx] == 90) == stays and ref[2][cy, cx] == 24 + extra
        check(run(ctx, img, 0, 24, 1), ref, f"rectangle of {24 + extra} pixels at {corner}")


def frames_case():
    """F = 3 at 17 x 67: the last row of a frame and the first row of the next are valid and equal"""
    img = np.stack([levels(17, 67, np.uint8, seed=40 + f) for f in range(3)])
    img[:, 0, :] = 2
    img[:, -1, :] = 2
    return img


def test_frames_are_separate(ctx):
    img = frames_case()
    ref = reference(img, 3, 5, 1)
    assert all(r.min() >= -1 and r.max() < 17 * 67 for r in ref[1])  # labels are per frame
    assert ref[1][1, 0, 0] == 0 and ref[1][2, 0, 0] == 0
    check(run(ctx, img, 3, 5, 1), ref, "F = 3, one group")
    ref0 = reference(img, 0, 5, 1)
    check(run(ctx, img, 0, 5, 1), ref0, "F = 3, no median")


def test_groups_pitch_and_memory_kinds(ctx):
    import torch
    for dtype in (np.uint8, np.uint16):
        img = (frames_case().astype(dtype) * unit(dtype)).astype(dtype)
        F, H, W = img.shape
        kw = dict(median=3, size=5, diff=unit(dtype))
        ref = reference(img, **kw)
        check(run(ctx, img, group_frames=0, **kw), ref, "group_frames 0")
        check(run(ctx, img, group_frames=2, **kw), ref, "group_frames 2")
        singles = [run(ctx, img[f], **kw) for f in range(F)]
        check(tuple(np.stack([to_np(s[k]) for s in singles]) for k in range(3)) + ([s[3][0] for s in singles],), ref, "three single calls")
        big = np.full((F, H + 3, W + 5), 0xEE, dtype)  # pitch > cols * elem_bytes, frame_stride > rows * pitch
        pad = big[:, :H, :W]
        pad[...] = img
        assert pad.strides[0] > H * pad.strides[1] and pad.strides[1] > W * img.itemsize and not pad.flags["C_CONTIGUOUS"]
        check(run(ctx, pad, **kw), ref, "padded")
        check(run(ctx, pad, group_frames=1, median=0, size=5, diff=unit(dtype)), reference(img, 0, 5, unit(dtype)), "padded, no median")
        t = torch.from_numpy(img.view(np.int16) if dtype == np.uint16 else img).cuda()
        dev = run(ctx, t, group_frames=2, **kw)
        assert all(d.is_cuda for d in dev[:3]) and dev[0].dtype == t.dtype and dev[1].dtype == torch.int32
        check(dev, ref, "CUDA tensors")
        tp = torch.from_numpy(big.view(np.int16) if dtype == np.uint16 else big).cuda()[:, :H, :W]
        check(run(ctx, tp, **kw), ref, "CUDA tensors, padded")


def launches(ctx, kinds):
    return [ctx.profileRead(k)[1] for k in kinds]


def test_launch_counts(ctx):
    from online_3d_reconstruction_amd import _lib as L
    kinds = (L.K_DISP_MEDIAN, L.K_DISP_LABEL, L.K_DISP_SPECKLE)
    img = levels(67, 131, np.uint8, seed=3)
    ctx.profileEnable(-1, True)
    try:
        ctx.profileReset()
        out = ctx.filterDisparity(img, median=3)
        assert np.array_equal(out, R.median(img, 3))
        n = launches(ctx, kinds)
        assert n[0] > 0 and n[1] == 0 and n[2] == 0, n
        ctx.profileReset()
        out = ctx.filterDisparity(img, max_speckle_size=4)
        assert np.array_equal(out, reference(img, 0, 4, 1)[0])
        n = launches(ctx, kinds)
        assert n[0] == 0 and n[1] > 0 and n[2] > 0, n
        ctx.profileReset()
        out = ctx.filterDisparity(img)
        assert out is not img and np.array_equal(out, img)
        assert launches(ctx, kinds) == [0, 0, 0]
        # the number of launches does not depend on the image
        ctx.profileReset()
        run(ctx, img, 3, 4, 1)
        a = launches(ctx, kinds)
        ctx.profileReset()
        run(ctx, R.serpentine(67, 131), 3, 4, 1)
        assert launches(ctx, kinds) == a
    finally:
        ctx.profileEnable(-1, False)
        ctx.profileReset()


def test_bad_arguments_zero_host_outputs_and_launch_nothing(ctx):
    from online_3d_reconstruction_amd import _lib as L
    lib = L.load_library()
    H, W, F = 9, 33, 2
    img16 = np.stack([levels(H, W, np.uint16, seed=s) for s in (1, 2)])
    good = dict(elem_bytes=2, median_size=3, max_speckle_size=3, max_diff=20000, group_frames=0)
    kinds = (L.K_DISP_MEDIAN, L.K_DISP_LABEL, L.K_DISP_SPECKLE, L.K_OTHER)

    def call(pitch=2 * W, fs=2 * H * W, rows=H, cols=W, n_frames=F, mem=0, in_shift=0, out_shift=0, lab_shift=0, siz_shift=0, **kw):
        prm = L.DisparityFilterParamsStruct(**{**good, **kw})
        src = np.zeros(F * H * W * 2 + 2, np.uint8)
        src[in_shift:in_shift + F * H * W * 2] = img16.view(np.uint8).ravel()
        raw = [np.full(F * H * W * e + 4, 0x5A, np.uint8) for e in (2, 4, 4)]
        out, lab, siz = (r[s:s + F * H * W * e] for r, s, e in zip(raw, (out_shift, lab_shift, siz_shift), (2, 4, 4)))
        info = (L.DisparityFilterInfoStruct * F)()
        for i in info:
            i.n_valid = i.largest = 0x5A
        rc = lib.o3dr_disparity_filter(ctx._h, src[in_shift:].ctypes.data, fs, pitch, rows, cols, n_frames, C.byref(prm), out.ctypes.data,
                                       lab.ctypes.data, siz.ctypes.data, C.cast(info, C.c_void_p), mem)
        return rc, out, lab, siz, info

    ref = reference(img16, 3, 3, 20000)
    rc, out, lab, siz, info = call()
    assert rc == 0
    assert np.array_equal(out.view(np.uint16).reshape(F, H, W), ref[0]) and np.array_equal(lab.view(np.int32).reshape(F, H, W), ref[1])
    assert np.array_equal(siz.view(np.int32).reshape(F, H, W), ref[2]) and [i.n_removed for i in info] == [r.n_removed for r in ref[3]]
    # n_frames = 0: O3DR_OK, nothing touched
    rc, out, lab, siz, info = call(n_frames=0)
    assert rc == 0 and (out == 0x5A).all() and (lab == 0x5A).all() and info[0].n_valid == 0x5A

    ctx.profileEnable(-1, True)
    ctx.profileReset()
    bad = [dict(median_size=1), dict(median_size=2), dict(median_size=4), dict(median_size=7), dict(elem_bytes=0), dict(elem_bytes=3),
           dict(max_diff=-1), dict(max_diff=65536), dict(max_speckle_size=-1), dict(group_frames=-1), dict(pitch=2 * W - 1),
           dict(pitch=2 * W - 2), dict(fs=2 * H * W - 2), dict(mem=2), dict(in_shift=1), dict(out_shift=1), dict(lab_shift=2),
           dict(siz_shift=1)]
    for kw in bad:
        rc, out, lab, siz, info = call(**kw)
        assert rc == L.ERR_INVALID_ARG, kw
        if kw.get("mem") != 2:  # (an unknown memory kind is no host memory: nothing is written)
            assert not lab.any() and not siz.any() and all(i.n_valid == 0 and i.largest == 0 for i in info), kw
            if "elem_bytes" not in kw:  # (the size of `out` is known only with a valid element size)
                assert not out.any(), kw
    # shapes outside their limits: the outputs' sizes are unknown, nothing is written
    for kw in (dict(rows=0), dict(cols=0), dict(rows=8193), dict(cols=8193), dict(n_frames=-1)):
        rc, out, lab, siz, info = call(**kw)
        assert rc == L.ERR_INVALID_ARG and (out == 0x5A).all() and (lab == 0x5A).all(), kw
    buf = np.zeros(F * H * W, np.uint16)
    args = (2 * H * W, 2 * W, H, W, F, C.byref(L.DisparityFilterParamsStruct(**good)))
    assert lib.o3dr_disparity_filter(ctx._h, None, *args, buf.ctypes.data, None, None, None, 0) == L.ERR_INVALID_ARG
    assert lib.o3dr_disparity_filter(ctx._h, img16.ctypes.data, *args, None, None, None, None, 0) == L.ERR_INVALID_ARG
    assert lib.o3dr_disparity_filter(None, img16.ctypes.data, *args, buf.ctypes.data, None, None, None, 0) == L.ERR_INVALID_ARG
    assert all(ctx.profileRead(k)[1] == 0 for k in kinds), "a rejected call launched a kernel"
    rc, out = call()[:2]
    assert rc == 0 and np.array_equal(out.view(np.uint16).reshape(F, H, W), ref[0])
    assert all(ctx.profileRead(k)[1] > 0 for k in kinds[:3])
    ctx.profileEnable(-1, False)
    ctx.profileReset()


def test_through_the_matcher(ctx):
    import stereo_reference as S
    left, right, _ = S.synthetic_pair(48, 96, 12, 20, (16, 30), seed=2)
    sref = S.stereo_disparity(left, right, n_disparities=32, min_disparity=0, p1=10, p2=120, n_paths=8, uniqueness=10, lr_max_diff=1)
    rdisp, rq4 = sref[0], sref[1]
    want = R.filter_disparity(rdisp, 3, 20, 1)[0]
    got, cost = ctx.stereoDisparity(left, right, 32, median=3, speckle_size=20, speckle_diff=1, return_cost=True)
    assert got.dtype == np.uint8 and np.array_equal(got, want) and np.array_equal(cost, sref[2])
    assert not np.array_equal(want, rdisp)  # the filter changes this image
    want4 = R.filter_disparity(rq4, 3, 20, 16)[0]
    sub = ctx.stereoDisparity(left, right, 32, subpixel=True, median=3, speckle_size=20, speckle_diff=1)
    assert sub.dtype == np.float64 and np.array_equal(sub, want4.astype(np.float64) / 16.0)
    # the keywords at their defaults: today's output
    assert np.array_equal(ctx.stereoDisparity(left, right, 32), rdisp)
    assert np.array_equal(ctx.stereoDisparity(left, right, 32, median=0, speckle_size=0, speckle_diff=1, subpixel=True) * 16.0, rq4.astype(np.float64))


def test_both_routes_into_accumulate_frames(Q):
    import online_3d_reconstruction_amd as o3dr
    import stereo_reference as S
    import torch
    left, right, _ = S.synthetic_pair(48, 96, 12, 20, (16, 30), seed=2)
    bgr = np.repeat(left[..., None], 3, -1)
    poses = np.stack([np.eye(4, dtype=np.float32)])
    with o3dr.Context(0, Q=Q, params=o3dr.Params(jump_pixels=1, sor_enable=False, bounding_box=2, min_disparity=4.0)) as c:
        disp = c.stereoDisparity(left, right, 32)
        filt = c.filterDisparity(disp, 3, 20, 1)
        c.accumulateFrames(np.stack([filt]), np.stack([bgr]), poses)
        a = c.cloudBigRead()
        c.cloudBigReset()
        tfilt = c.filterDisparity(torch.from_numpy(disp).cuda(), 3, 20, 1)
        assert tfilt.is_cuda and tfilt.dtype == torch.uint8 and np.array_equal(tfilt.cpu().numpy(), filt)
        c.accumulateFrames(tfilt[None].contiguous(), torch.from_numpy(bgr).cuda()[None].contiguous(), torch.from_numpy(poses).cuda())
        d = c.cloudBigRead()
    assert len(a) > 1000 and np.array_equal(a.view(np.uint32), d.view(np.uint32))
