"""GPU tests of o3dr_segment_image / Context.segmentImage (include/o3dr.h "image segmentation"): labels, raw, sizes and
every info field bit for bit against tests/segment_reference.py, at the smallest shapes at which each piece can go wrong.
The kernels' tile is 64 x 16 pixels: 67 x 131 has two tile borders in x and four in y, 70 x 33 none in x and four in y.
That is 15 tiles and the single-workgroup scan; images of 256 tiles and the chunked scan are in tests/test_labelling_scale.py."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import segment_reference as R

pytestmark = pytest.mark.gpu

FIELDS = ("n_centres", "n_components", "n_merged", "n_labels", "largest", "smallest")


def to_np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


@functools.lru_cache(maxsize=None)
def image(H, W, channels):
    img = R.random_image(H, W, channels, seed=H * 1000 + W)
    img.setflags(write=False)
    return img


def reference(img, S, m, K, min_size):
    """-> labels, raw, sizes, [info] of one image or of a stack (channels by the last axis, as the API reads it)"""
    stack = img.ndim == 4 or (img.ndim == 3 and img.shape[-1] != 3)
    res = [R.segment(f, S, m, K, min_size) for f in (img if stack else [img])]
    out = tuple(np.stack([r[k] for r in res]) if stack else res[0][k] for k in ("labels", "raw", "sizes"))
    return out + ([r["info"] for r in res],)


def run(ctx, img, S, m, K, min_size, **kw):
    return ctx.segmentImage(img, S, m, K, min_size, return_raw=True, return_sizes=True, return_info=True, **kw)


def check(got, ref, what):
    labels, raw, sizes, infos = got
    for name, g, r in (("raw", raw, ref[1]), ("labels", labels, ref[0]), ("sizes", sizes, ref[2])):
        g = to_np(g)
        if name == "labels" and g.dtype == np.int32:  # (device tensors: int32 holding the same values)
            g = g.view(np.uint32)
        assert g.dtype == r.dtype and g.shape == r.shape, f"{what}: {name} is {g.dtype} {g.shape}, expected {r.dtype} {r.shape}"
        if not np.array_equal(g, r):
            bad = np.argwhere(g != r)[0]
            idx = tuple(int(v) for v in ((0,) * (3 - len(bad)) + tuple(bad)))
            raise AssertionError(f"{what}: {name} differs first at (frame, y, x) = {idx}: {g[tuple(bad)]} vs {r[tuple(bad)]}, "
                                 f"{int((g != r).sum())} pixels in all")
    assert len(infos) == len(ref[3])
    for f, (gi, ri) in enumerate(zip(infos, ref[3])):
        for k in FIELDS:
            assert getattr(gi, k) == ri[k], f"{what}: info[{f}].{k} = {getattr(gi, k)}, expected {ri[k]}"


SHAPES = [(1, 1), (1, 40), (40, 1), (7, 9), (33, 70), (70, 33), (67, 131)]
COMBOS = list(itertools.product((0, 1, 5), (0, None, 10000), (0, 20)))  # K, min_size, m


@pytest.mark.parametrize("channels", [1, 3], ids=["grey", "bgr"])
@pytest.mark.parametrize("S", [4, 8])
@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_matches_the_reference(ctx, H, W, S, channels):
    img = image(H, W, channels)
    for K, min_size, m in COMBOS:
        check(run(ctx, img, S, m, K, min_size), reference(img, S, m, K, min_size), f"{H}x{W} S {S} m {m} K {K} min_size {min_size}")


def test_the_inputs_bite():
    """the cases above are worth something only if some components are merged and others are not, the updates move the
    centres, and the two compactness values and the tie-break give different images"""
    img = image(67, 131, 3)
    a = R.segment(img, 8, 20, 5)
    assert 0 < a["info"]["n_merged"] < a["info"]["n_components"] and a["info"]["n_labels"] > 50
    assert not np.array_equal(a["raw"], R.segment(img, 8, 20, 0)["raw"])
    assert not np.array_equal(a["raw"], R.segment(img, 8, 0, 5)["raw"])
    assert not np.array_equal(a["labels"], R.segment(img, 8, 20, 5, 0)["labels"])
    assert R.segment(img, 8, 20, 5, 10000)["info"]["n_labels"] == 1
    grey = image(67, 131, 1)
    assert not np.array_equal(R.segment(grey, 4, 0, 1)["raw"], R.segment(grey, 4, 0, 1, highest_k_wins=True)["raw"])


STRESS = {
    "constant": (lambda H, W: R.constant_image(H, W), 8, 0),
    "constant, compact": (lambda H, W: R.constant_image(H, W), 8, 20),
    "checkerboard": (lambda H, W: R.checkerboard(H, W), 5, 0),
    # two colours at m = 0 with at most 2 x 2 centres, every one a candidate of every pixel: a pixel takes the lowest centre
    # of its own colour, so the bright pixels are one raw label and one component.  The steps put a seed on either colour.
    "serpentine": (lambda H, W: R.serpentine(H, W), 66, 0),
    "serpentine transposed": (lambda H, W: np.ascontiguousarray(R.serpentine(W, H).T), 67, 0),
    "comb": (lambda H, W: R.comb(H, W), 67, 0),
    "comb upside down": (lambda H, W: np.ascontiguousarray(R.comb(H, W)[::-1]), 67, 0),
}


@pytest.mark.parametrize("name", list(STRESS))
def test_stress_images(ctx, name):
    H, W = 67, 131
    make, S, m = STRESS[name]
    img = make(H, W)
    assert img.shape == (H, W)
    for K, min_size in ((1, 10000), (3, None), (0, 0)):
        ref = reference(img, S, m, K, min_size)
        check(run(ctx, img, S, m, K, min_size), ref, f"{name} K {K} min_size {min_size}")
        info = ref[3][0]
        if name == "checkerboard":  # every pixel is its own component; with a min_size above 1 the chain runs to pixel 0
            assert info["n_components"] == H * W and info["n_labels"] == (H * W if min_size == 0 else 1)
    if name.startswith(("serpentine", "comb")):  # the bright component winds across every tile border
        raw = reference(img, S, m, 1, 0)[1]
        root = R.components(raw)
        bright = root[img == 255]
        assert (bright == bright[0]).all() and len(bright) > H * W // 4 and len(np.unique(root)) > 1


def test_large_coordinates(ctx):
    """9 x 8192: x up to 8191 in the distances, the sums and the first pixels"""
    H, W = 9, 8192
    img = image(H, W, 1)
    ref = reference(img, 8, 20, 2, None)
    assert ref[3][0]["n_centres"] == 2 * 1024
    check(run(ctx, img, 8, 20, 2, None), ref, "9 x 8192")


def frames_case(channels=3):
    return np.stack([R.random_image(35, 70, channels, seed=60 + f) for f in range(3)])


def test_groups_strides_and_memory_kinds(ctx):
    import torch
    for channels in (3, 1):
        img = frames_case(channels)
        F, H, W = img.shape[:3]
        args = (8, 20, 3, None)
        ref = reference(img, *args)
        assert len({i["n_labels"] for i in ref[3]}) > 1 or not np.array_equal(ref[0][0], ref[0][1])
        for g in (0, 1, 2):
            check(run(ctx, img, *args, group_frames=g), ref, f"group_frames {g}")
        singles = [run(ctx, img[f], *args) for f in range(F)]
        check(tuple(np.stack([to_np(s[k]) for s in singles]) for k in range(3)) + ([s[3][0] for s in singles],), ref, "three single calls")
        check(run(ctx, img, *args), ref, "a second call")
        big = np.full((F, H + 3, W + 5) + img.shape[3:], 0xEE, np.uint8)  # pitch > a row, frame_stride > rows * pitch
        pad = big[:, :H, :W]
        pad[...] = img
        assert not pad.flags["C_CONTIGUOUS"]
        check(run(ctx, pad, *args), ref, "strided view")
        t = torch.from_numpy(img).cuda()
        dev = run(ctx, t, *args, group_frames=2)
        assert all(d.is_cuda and d.dtype == torch.int32 for d in dev[:3])
        check(dev, ref, "CUDA tensors")
        check(run(ctx, torch.from_numpy(big).cuda()[:, :H, :W], *args), ref, "CUDA tensors, strided view")
        only = ctx.segmentImage(img, *args)
        assert only.dtype == np.uint32 and np.array_equal(only, ref[0])


def launches(ctx, kinds):
    return [ctx.profileRead(k)[1] for k in kinds]


def test_launch_counts_do_not_depend_on_the_image(ctx):
    from online_3d_reconstruction_amd import _lib as L
    kinds = (L.K_SEG_ASSIGN, L.K_SEG_LABEL)
    ctx.profileEnable(-1, True)
    try:
        counts = []
        for img in (image(67, 131, 1), R.checkerboard(67, 131), R.constant_image(67, 131)):
            ctx.profileReset()
            run(ctx, img, 5, 0, 3, 10000)
            counts.append(launches(ctx, kinds))
        assert counts[0] == counts[1] == counts[2] and all(c > 0 for c in counts[0]), counts
        ctx.profileReset()
        ctx.profileEnable(L.K_SEG_ASSIGN, False)  # the two highest kinds are switched one by one
        run(ctx, image(67, 131, 1), 5, 0, 3, 10000)
        assert launches(ctx, kinds) == [0, counts[0][1]]
    finally:
        ctx.profileEnable(-1, False)
        ctx.profileReset()


def test_bad_arguments_zero_host_outputs_and_launch_nothing(ctx):
    from online_3d_reconstruction_amd import _lib as L
    lib = L.load_library()
    H, W, F = 9, 33, 2
    img = np.stack([R.random_image(H, W, 3, seed=s) for s in (1, 2)])
    good = dict(channels=3, step=4, compactness=20, iterations=2, min_size=-1, group_frames=0)
    kinds = (L.K_SEG_ASSIGN, L.K_SEG_LABEL, L.K_OTHER)

    def call(pitch=3 * W, fs=3 * H * W, rows=H, cols=W, n_frames=F, mem=0, lab_shift=0, raw_shift=0, siz_shift=0, **kw):
        prm = L.SegmentParamsStruct(**{**good, **kw})
        bufs = [np.full(F * H * W * 4 + 4, 0x5A, np.uint8) for _ in range(3)]
        lab, raw, siz = (b[s:s + F * H * W * 4] for b, s in zip(bufs, (lab_shift, raw_shift, siz_shift)))
        info = (L.SegmentInfoStruct * F)()
        for i in info:
            i.n_centres = i.smallest = 0x5A
        rc = lib.o3dr_segment_image(ctx._h, img.ctypes.data, fs, pitch, rows, cols, n_frames, C.byref(prm), lab.ctypes.data,
                                    raw.ctypes.data, siz.ctypes.data, C.cast(info, C.c_void_p), mem)
        return rc, lab, raw, siz, info

    ref = reference(img, 4, 20, 2, None)
    rc, lab, raw, siz, info = call()
    assert rc == 0
    assert np.array_equal(lab.view(np.uint32).reshape(F, H, W), ref[0]) and np.array_equal(raw.view(np.int32).reshape(F, H, W), ref[1])
    assert np.array_equal(siz.view(np.int32).reshape(F, H, W), ref[2]) and [i.n_labels for i in info] == [r["n_labels"] for r in ref[3]]
    # a negative min_size of any value is the default
    assert np.array_equal(call(min_size=-7)[1], lab)
    # n_frames = 0: O3DR_OK, nothing touched
    rc, lab0, raw0, siz0, info0 = call(n_frames=0)
    assert rc == 0 and (lab0 == 0x5A).all() and (raw0 == 0x5A).all() and info0[0].n_centres == 0x5A

    ctx.profileEnable(-1, True)
    ctx.profileReset()
    bad = [dict(channels=0), dict(channels=2), dict(channels=4), dict(step=3), dict(step=257), dict(compactness=-1), dict(compactness=256),
           dict(iterations=-1), dict(iterations=33), dict(group_frames=-1), dict(pitch=3 * W - 1), dict(fs=3 * H * W - 1), dict(mem=2),
           dict(lab_shift=2), dict(raw_shift=1), dict(siz_shift=3)]
    for kw in bad:
        rc, lab1, raw1, siz1, info1 = call(**kw)
        assert rc == L.ERR_INVALID_ARG, kw
        if kw.get("mem") != 2:  # (an unknown memory kind is no host memory: nothing is written)
            assert not lab1.any() and not raw1.any() and not siz1.any(), kw
            assert all(i.n_centres == 0 and i.smallest == 0 for i in info1), kw
    # shapes outside their limits: the outputs' sizes are unknown, nothing is written
    for kw in (dict(rows=0), dict(cols=0), dict(rows=8193), dict(cols=8193), dict(n_frames=-1)):
        rc, lab1, raw1, siz1, info1 = call(**kw)
        assert rc == L.ERR_INVALID_ARG and (lab1 == 0x5A).all() and (raw1 == 0x5A).all(), kw
    buf = np.zeros(F * H * W, np.int32)
    args = (3 * H * W, 3 * W, H, W, F, C.byref(L.SegmentParamsStruct(**good)))
    assert lib.o3dr_segment_image(ctx._h, None, *args, buf.ctypes.data, None, None, None, 0) == L.ERR_INVALID_ARG
    assert lib.o3dr_segment_image(ctx._h, img.ctypes.data, *args, None, None, None, None, 0) == L.ERR_INVALID_ARG
    assert lib.o3dr_segment_image(None, img.ctypes.data, *args, buf.ctypes.data, None, None, None, 0) == L.ERR_INVALID_ARG
    assert all(ctx.profileRead(k)[1] == 0 for k in kinds), "a rejected call launched a kernel"
    # NULL params: the defaults (B G R, step 16, compactness 20, 5 iterations)
    assert lib.o3dr_segment_image(ctx._h, img.ctypes.data, *args[:5], None, buf.ctypes.data, None, None, None, 0) == 0
    assert np.array_equal(buf.view(np.uint32).reshape(F, H, W), reference(img, 16, 20, 5, None)[0])
    assert all(ctx.profileRead(k)[1] > 0 for k in kinds[:2])
    ctx.profileEnable(-1, False)
    ctx.profileReset()


def test_chain_with_the_plane_fit(ctx):
    """segmentImage -> planeFitDisparity on device tensors equals the numpy route bit for bit, and the fitted image is
    closer to the true planes than half the raw image's error (the condition of test_segment_reference.py)"""
    import torch
    img, region, disp, true = R.region_image()
    for S in (8, 16):
        labels = ctx.segmentImage(img, S, 20)
        assert labels.dtype == np.uint32 and np.array_equal(labels, R.segment(img, S, 20)["labels"])
        host = ctx.planeFitDisparity(disp, labels)
        tl = ctx.segmentImage(torch.from_numpy(img).cuda(), S, 20)
        assert tl.is_cuda and tl.dtype == torch.int32
        dev = ctx.planeFitDisparity(torch.from_numpy(disp).cuda(), tl)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy().reshape(host.shape).view(np.uint64), host.view(np.uint64))
        raw_rms = float(np.sqrt(np.mean((disp.astype(np.float64) - true) ** 2)))
        fit_rms = float(np.sqrt(np.mean((host.reshape(true.shape) - true) ** 2)))
        print(f"S={S}: plane-fit RMS {fit_rms:.3f} against raw {raw_rms:.3f}")
        assert fit_rms < 0.5 * raw_rms
