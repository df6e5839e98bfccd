"""GPU tests of o3dr_stereo_disparity / Context.stereoDisparity (include/o3dr.h "stereo disparity"): disp, disp_q4, cost and
the S volume bit for bit against tests/stereo_reference.py, at the smallest shapes at which each piece can go wrong."""
import ctypes as C

import numpy as np
import pytest

import stereo_reference as R

pytestmark = pytest.mark.gpu


def make_pair(H, W, seed, channels=1, t=5):
    """textured pair with a known shift in its left part and independent noise elsewhere: ties are rare, rejections are not"""
    rng = np.random.RandomState(seed)
    shape = (H, W) if channels == 1 else (H, W, 3)
    right = rng.randint(0, 256, shape).astype(np.uint8)
    left = rng.randint(0, 256, shape).astype(np.uint8)
    if W > 2 * t:
        left[:, t:W - W // 4] = right[:, :W - W // 4 - t]
    return left, right


def reference(left, right, **kw):
    """per-frame reference of a [H, W(, 3)] pair or a stack of them -> disp, q4, cost, S (stacked like the input)"""
    prm = dict(n_disparities=32, min_disparity=0, p1=10, p2=120, n_paths=8, uniqueness=10, lr_max_diff=1)
    prm.update(kw)
    if left.ndim == 2 or (left.ndim == 3 and left.shape[-1] == 3):
        return R.stereo_disparity(left, right, **prm)
    outs = [R.stereo_disparity(l, r, **prm) for l, r in zip(left, right)]
    return tuple(np.stack(o) for o in zip(*outs))


def run(ctx, left, right, **kw):
    prm = dict(n_disparities=32)
    prm.update(kw)
    disp, cost, S = ctx.stereoDisparity(left, right, return_cost=True, return_volume=True, **prm)
    q4 = ctx.stereoDisparity(left, right, subpixel=True, **prm)
    return disp, q4, cost, S


def to_np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def check(got, ref, what):
    disp, q4f, cost, S = (to_np(g) for g in got)
    rdisp, rq4, rcost, rS = ref
    S = S.view(np.uint16) if S.dtype != np.uint16 else S
    if not np.array_equal(S, rS):
        bad = np.argwhere(S.reshape(rS.shape) != rS)[0]
        idx = tuple(int(v) for v in ((0,) * (4 - len(bad)) + tuple(bad)))
        raise AssertionError(f"{what}: S differs first at (frame, y, x, d) = {idx}: {S.reshape(rS.shape)[tuple(bad)]} vs {rS[tuple(bad)]}")
    assert np.array_equal(cost.view(np.uint16) if cost.dtype != np.uint16 else cost, rcost), f"{what}: cost"
    assert disp.dtype == np.uint8 and np.array_equal(disp, rdisp), f"{what}: disp, {int((disp != rdisp).sum())} pixels"
    assert q4f.dtype == np.float64 and np.array_equal(q4f * 16.0, rq4.astype(np.float64)), f"{what}: disp_q4"


CASES = [
    # window larger than the image: every clamp
    ("1x1", 1, 1, {}),
    ("1x40", 1, 40, {}),
    ("40x1", 40, 1, {}),
    ("7x9", 7, 9, {}),
    # W < D: nearly every candidate takes the xr < 0 branch
    ("24x40 D64", 24, 40, dict(n_disparities=64)),
    # diagonals on wide and tall images, no multiple of 64 or of a tile
    ("33x70", 33, 70, {}),
    ("70x33", 70, 33, {}),
    # half a wave, an uneven split over the lanes, four candidates per lane with d +- 1 crossing registers
    ("10x130 D32", 10, 130, dict(n_disparities=32)),
    ("10x130 D96", 10, 130, dict(n_disparities=96)),
    ("20x300 D256", 20, 300, dict(n_disparities=256)),
    ("12x280 D192 d0 64", 12, 280, dict(n_disparities=192, min_disparity=64)),
    # the winner pass's first wave stops D - 1 columns past its 256 (256 + 31 < 330) and hands over to the next one
    ("6x330 D32", 6, 330, dict(n_disparities=32)),
    ("5x600 D64 d0 3", 5, 600, dict(n_disparities=64, min_disparity=3)),
    ("4 paths", 19, 75, dict(n_paths=4)),
    ("P1 = P2 = 0", 19, 75, dict(p1=0, p2=0)),
    ("P1 = 0, P2 = 255", 19, 75, dict(p1=0, p2=255)),
    ("P1 = P2 = 255", 19, 75, dict(p1=255, p2=255)),
    ("uniqueness 0", 19, 75, dict(uniqueness=0)),
    ("uniqueness 50", 19, 75, dict(uniqueness=50)),
    ("lr -1", 19, 75, dict(lr_max_diff=-1)),
    ("lr 0", 19, 75, dict(lr_max_diff=0)),
    ("lr 3", 19, 75, dict(lr_max_diff=3)),
]


@pytest.mark.parametrize("name,H,W,kw", CASES, ids=[c[0] for c in CASES])
def test_matches_the_reference(ctx, name, H, W, kw):
    left, right = make_pair(H, W, seed=H * 1000 + W)
    check(run(ctx, left, right, **kw), reference(left, right, **kw), name)


def test_four_paths_differ_from_eight(ctx):
    left, right = make_pair(19, 75, seed=19075)
    S4 = ctx.stereoDisparity(left, right, 32, n_paths=4, return_volume=True)[1]
    S8 = ctx.stereoDisparity(left, right, 32, n_paths=8, return_volume=True)[1]
    assert (S8 >= S4).all() and (S8 > S4).any()


def test_rejections_happen(ctx):
    """the cases above are worth something only if every rejection rule fires on that input"""
    left, right = make_pair(19, 75, seed=19075)
    none = reference(left, right, uniqueness=0, lr_max_diff=-1)[0]
    uniq = reference(left, right, uniqueness=50, lr_max_diff=-1)[0]
    lr = reference(left, right, uniqueness=0, lr_max_diff=0)[0]
    assert (none != 0).sum() > (uniq != 0).sum() > 0 and (none != 0).sum() > (lr != 0).sum() > 0


def test_constant_and_identical_pairs(ctx):
    const = np.full((21, 90), 128, np.uint8)
    got = run(ctx, const, const)
    check(got, reference(const, const), "constant pair")
    assert not to_np(got[0]).any()  # ties everywhere: the lowest candidate, d0 + best = 0
    img = make_pair(21, 90, seed=5)[1]
    got = run(ctx, img, img)
    check(got, reference(img, img), "identical pair")
    assert not to_np(got[0]).any() and not to_np(got[2]).any()  # best = 0 at cost 0
    got = run(ctx, img, img, n_disparities=64, min_disparity=3)
    check(got, reference(img, img, n_disparities=64, min_disparity=3), "identical pair, d0 = 3")


@pytest.mark.parametrize("channels", [1, 3])
def test_channels_pitch_and_frame_stride(ctx, channels):
    H, W, F = 17, 67, 2
    pairs = [make_pair(H, W, seed=70 + f, channels=channels) for f in range(F)]
    left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    ref = reference(left, right)
    check(run(ctx, left, right), ref, "tight")

    def padded(a):  # pitch > cols * channels, frame_stride > rows * pitch
        big = np.full((F, H + 3, (W + 5) * channels), 0xEE, np.uint8)
        v = np.lib.stride_tricks.as_strided(big, (F, H, W) + ((3,) if channels == 3 else ()),
                                            (big.strides[0], big.strides[1]) + ((3, 1) if channels == 3 else (1,)))
        v[...] = a
        return v
    pl, pr = padded(left), padded(right)
    assert pl.strides[0] > H * pl.strides[1] and pl.strides[1] > W * channels and not pl.flags["C_CONTIGUOUS"]
    check(run(ctx, pl, pr), ref, "padded")
    check(run(ctx, left[0], right[0]), tuple(r[0] for r in ref), "single frame")


def test_groups_batches_and_memory_kinds(ctx):
    import torch
    H, W, F = 23, 71, 5
    pairs = [make_pair(H, W, seed=300 + f) for f in range(F)]
    left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    ref = reference(left, right)
    whole = run(ctx, left, right)
    check(whole, ref, "F = 5, one group")
    check(run(ctx, left, right, group_frames=2), ref, "F = 5, groups of 2")
    singles = [run(ctx, left[f], right[f]) for f in range(F)]
    check(tuple(np.stack([to_np(s[k]) for s in singles]) for k in range(4)), ref, "five single calls")
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    dev = run(ctx, tl, tr, group_frames=2)
    assert all(d.is_cuda for d in dev)
    assert dev[3].dtype == torch.uint16 and dev[2].dtype == torch.uint16 and dev[0].dtype == torch.uint8
    dev = (dev[0], dev[1], dev[2].view(torch.int16), dev[3].view(torch.int16))
    check(dev, ref, "CUDA tensors")


def test_bad_arguments_zero_host_outputs_and_launch_nothing(ctx):
    from online_3d_reconstruction_amd import _lib as L
    lib = L.load_library()
    H, W, F = 9, 33, 2
    left, right = (np.stack([make_pair(H, W, seed=s)[k] for s in (1, 2)]) for k in (0, 1))
    good = dict(n_disparities=32, min_disparity=0, p1=10, p2=120, n_paths=8, uniqueness=10, lr_max_diff=1, channels=1, group_frames=0)
    kinds = (L.K_STEREO_CENSUS, L.K_STEREO_PATHS, L.K_STEREO_WINNER)

    def call(pitch=W, fs=H * W, rows=H, cols=W, n_frames=F, mem=0, q4_shift=0, **kw):
        prm = L.StereoParamsStruct(**{**good, **kw})
        disp = np.full((F, H, W), 0x5A, np.uint8)
        raw = np.full(F * H * W * 2 + 2, 0x5A, np.uint8)
        q4 = raw[q4_shift:q4_shift + F * H * W * 2]
        cost = np.full((F, H, W), 0x5A5A, np.uint16)
        vol = np.full((F, H, W, 256), 0x5A5A, np.uint16)[..., :prm.n_disparities if 32 <= prm.n_disparities <= 256 else 32]
        vol = np.ascontiguousarray(vol)
        rc = lib.o3dr_stereo_disparity(ctx._h, left.ctypes.data, right.ctypes.data, fs, pitch, rows, cols, n_frames, C.byref(prm),
                                       disp.ctypes.data, q4.ctypes.data, cost.ctypes.data, vol.ctypes.data, mem)
        return rc, disp, q4, cost, vol

    rc, disp, q4, cost, vol = call()
    assert rc == 0
    ref = reference(left, right)
    assert np.array_equal(disp, ref[0]) and np.array_equal(q4.view(np.uint16).reshape(F, H, W), ref[1])
    assert np.array_equal(cost, ref[2]) and np.array_equal(vol, ref[3])
    # n_frames = 0: O3DR_OK, nothing touched
    rc, disp, q4, cost, vol = call(n_frames=0)
    assert rc == 0 and (disp == 0x5A).all() and (vol == 0x5A5A).all()

    ctx.profileEnable(-1, True)
    ctx.profileReset()
    bad = [dict(n_disparities=0), dict(n_disparities=16), dict(n_disparities=48), dict(n_disparities=288), dict(min_disparity=-1),
           dict(n_disparities=64, min_disparity=193), dict(p1=-1), dict(p1=256, p2=256), dict(p1=11, p2=10), dict(p2=256),
           dict(n_paths=5), dict(n_paths=0), dict(uniqueness=-1), dict(uniqueness=100), dict(lr_max_diff=-2), dict(lr_max_diff=256),
           dict(channels=2), dict(group_frames=-1), dict(pitch=W - 1), dict(fs=H * W - 1), dict(mem=2), dict(q4_shift=1)]
    for kw in bad:
        rc, disp, q4, cost, vol = call(**kw)
        assert rc == L.ERR_INVALID_ARG, kw
        if kw.get("mem") != 2:  # (an unknown memory kind is no host memory: nothing is written)
            assert not disp.any() and not q4.any() and not cost.any(), kw
            if kw.get("n_disparities", 32) % 32 == 0 and 32 <= kw.get("n_disparities", 32) <= 256:
                assert not vol.any(), kw
    # shapes outside their limits: the outputs' sizes are unknown, nothing is written
    for kw in (dict(rows=0), dict(cols=0), dict(rows=8193), dict(cols=8193), dict(n_frames=-1)):
        rc, disp, q4, cost, vol = call(**kw)
        assert rc == L.ERR_INVALID_ARG and (disp == 0x5A).all(), kw
    assert lib.o3dr_stereo_disparity(ctx._h, None, right.ctypes.data, H * W, W, H, W, F, None, None, None, None, None, 0) == L.ERR_INVALID_ARG
    assert lib.o3dr_stereo_disparity(None, left.ctypes.data, right.ctypes.data, H * W, W, H, W, F, None, None, None, None, None, 0) == L.ERR_INVALID_ARG
    assert all(ctx.profileRead(k)[1] == 0 for k in kinds), "a rejected call launched a kernel"
    rc = call()[0]
    assert rc == 0 and all(ctx.profileRead(k)[1] > 0 for k in kinds)
    ctx.profileEnable(-1, False)
    ctx.profileReset()


def test_both_routes_into_accumulate_frames(Q):
    import online_3d_reconstruction_amd as o3dr
    import torch
    left, right, t = R.synthetic_pair(48, 96, 12, 20, (16, 30), seed=2)
    bgr_l, bgr_r = (np.repeat(a[..., None], 3, -1) for a in (left, right))
    poses = np.stack([np.eye(4, dtype=np.float32)])
    frames = np.stack([bgr_l])  # (a[None] has a frame stride of 0, which the frame calls refuse)
    with o3dr.Context(0, Q=Q, params=o3dr.Params(jump_pixels=1, sor_enable=False, bounding_box=2, min_disparity=4.0)) as c:
        disp = c.stereoDisparity(bgr_l, bgr_r, 32)
        assert disp.dtype == np.uint8 and (disp == t).mean() > 0.5
        c.accumulateFrames(np.stack([disp]), frames, poses)
        a = c.cloudBigRead()
        c.cloudBigReset()
        # the same through HBM: CUDA tensors in, CUDA tensor out, straight into the frame call
        tdisp = c.stereoDisparity(torch.from_numpy(bgr_l).cuda(), torch.from_numpy(bgr_r).cuda(), 32)
        assert tdisp.is_cuda and np.array_equal(tdisp.cpu().numpy(), disp)
        c.accumulateFrames(tdisp[None].contiguous(), torch.from_numpy(bgr_l).cuda()[None].contiguous(), torch.from_numpy(poses).cuda())
        d = c.cloudBigRead()
    # the region of interest is 44 x 82 pixels (bounding_box 2, cutout 96 / 8), 0.4 m apart at these depths: one cell each
    assert len(a) > 1000 and np.array_equal(a.view(np.uint32), d.view(np.uint32))
    with o3dr.Context(0, Q=Q, params=o3dr.Params(jump_pixels=1, sor_enable=False, bounding_box=2, min_disparity=4.0, disparity_f64=True)) as c:
        sub = c.stereoDisparity(bgr_l, bgr_r, 32, subpixel=True)
        assert sub.dtype == np.float64 and ((sub == 0) == (disp == 0)).all() and np.abs(sub - disp)[disp != 0].max() <= 0.5
        assert (sub != disp).any()
        c.accumulateFrames(np.stack([sub]), frames, poses)
        s = c.cloudBigRead()
    assert len(s) > 1000
