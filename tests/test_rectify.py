"""GPU tests of o3dr_rectify_maps / o3dr_rectify_remap and Context.rectifyMaps / rectify / stereoDisparity(rectify=...)
(include/o3dr.h "stereo rectification"): every comparison with tests/rectify_reference.py is bit for bit, at the smallest
shapes at which each piece can go wrong (widths off and on a multiple of 4, heights below one block, aligned and
unaligned rows, padded strides, one and several launch groups)."""
import ctypes as C

import numpy as np
import pytest

import rectify_reference as R

pytestmark = pytest.mark.gpu

CASES = {"identity": R.IDENTITY, "general": R.GENERAL, "sentinel": R.SENTINEL, "pole": R.POLE,
         "D4": dict(R.GENERAL, D=R.D_GENERAL[:4]), "D5": dict(R.GENERAL, D=R.D_GENERAL[:5])}
SIZES = [(41, 50), (1, 1), (3, 67), (64, 64)]


@pytest.fixture(scope="module")
def general_maps():
    """the reference's general-case maps at the two destination sizes of the remap tests, computed once"""
    return {size: R.maps_of(R.GENERAL, size) for size in ((41, 50), (40, 52))}


@pytest.mark.parametrize("name", list(CASES))
def test_maps_equal_the_reference_in_host_and_device_memory(ctx, name):
    import torch
    c = CASES[name]
    for size in SIZES:
        want = R.rectify_maps(c["K"], c["D"], c["R"], c["P"], size)
        got = ctx.rectifyMaps(c["K"], c["D"], c["R"], c["P"], size)
        assert got.dtype == np.int32 and got.shape == size + (2,)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{name} {size}: first difference at {bad[0]}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"
        dev = ctx.rectifyMaps(c["K"], c["D"], c["R"], c["P"], size, device="cuda:0")
        assert dev.is_cuda and dev.dtype == torch.int32 and np.array_equal(dev.cpu().numpy(), want), f"{name} {size}: device memory"
    # a 3 x 3 projection is the 3 x 4 one without its last column
    assert np.array_equal(ctx.rectifyMaps(c["K"], c["D"], c["R"], c["P"][:, :3], (41, 50)), R.maps_of(c, (41, 50)))


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [(41, 50), (40, 52)])
def test_remap_equals_the_reference(ctx, general_maps, channels, size):
    import torch
    maps = general_maps[size]
    F = 5
    frames = np.stack([R.test_image(37, 53, channels, seed=10 + f) for f in range(F)])
    for border in (0, 9):
        want, want_valid = R.rectify_remap_frames(frames, maps, border)
        got, valid = ctx.rectify(frames, maps, border=border, return_valid=True)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), f"border {border}"
        assert valid.dtype == np.uint8 and np.array_equal(valid, want_valid)
        for g in (1, 2):  # several launch groups, the last one short: identical outputs
            again, valid_g = ctx.rectify(frames, maps, border=border, return_valid=True, group_frames=g)
            assert np.array_equal(again, want) and np.array_equal(valid_g, want_valid), f"group_frames {g}"
        assert np.array_equal(ctx.rectify(frames, maps, border=border), want)  # valid_out not asked for
        one = ctx.rectify(frames[2], maps, border=border)  # n_frames = 1
        assert one.shape == want.shape[1:] and np.array_equal(one, want[2])
    # a padded pitch and frame stride pass through as they are
    tail = (3,) if channels == 3 else ()
    big = np.full((F, 37 + 2, 53 + 7) + tail, 255, np.uint8)
    view = big[:, :37, :53]
    view[...] = frames
    assert view.strides[0] > 37 * view.strides[1] and view.strides[1] > 53 * channels
    assert np.array_equal(ctx.rectify(view, maps, border=9), R.rectify_remap_frames(frames, maps, 9)[0])
    # CUDA tensors in, CUDA tensors out
    want, want_valid = R.rectify_remap_frames(frames, maps, 9)
    tf, tm = torch.from_numpy(frames).cuda(), torch.from_numpy(maps).cuda()
    out, valid = ctx.rectify(tf, tm, border=9, return_valid=True, group_frames=2)
    assert out.is_cuda and valid.is_cuda and np.array_equal(out.cpu().numpy(), want) and np.array_equal(valid.cpu().numpy(), want_valid)
    tbig = torch.from_numpy(big).cuda()
    assert np.array_equal(ctx.rectify(tbig[:, :37, :53], tm, border=9).cpu().numpy(), want)


@pytest.mark.parametrize("channels", [1, 3])
def test_narrow_sources(ctx, channels):
    """sources of one, two and four columns: a one-column image has no two-pixel tap window, a two-column one exactly one;
    the map walks from beyond one border to beyond the other in steps that hit every fraction"""
    rng = np.random.RandomState(8)
    for rows, cols in ((5, 1), (4, 2), (1, 1), (1, 4), (2, 2)):  # (not 3 columns: a [2, H, 3] stack reads as one B G R image)
        src = np.stack([R.test_image(rows, cols, channels, seed=20 + f) for f in range(2)])
        maps = np.empty((6, 23, 2), np.int32)
        maps[..., 0] = np.linspace(-40, cols * 32 + 40, 23).astype(np.int32)[None, :] + rng.randint(0, 3, (6, 23))
        maps[..., 1] = np.linspace(-40, rows * 32 + 40, 6).astype(np.int32)[:, None] + rng.randint(0, 3, (6, 23))
        want, want_valid = R.rectify_remap_frames(src, maps, 9)
        got, valid = ctx.rectify(src, maps, border=9, return_valid=True)
        assert np.array_equal(got, want) and np.array_equal(valid, want_valid), (rows, cols)
        assert want_valid.any() or cols == 1 or rows == 1


def test_sentinel_entries_read_the_border(ctx):
    maps = R.maps_of(R.SENTINEL)
    img = R.test_image(37, 53, 3, seed=5)
    out, valid = ctx.rectify(img, maps, border=9, return_valid=True)
    want, want_valid = R.rectify_remap(img, maps, 9)
    assert np.array_equal(out, want) and np.array_equal(valid, want_valid)
    assert (out[:, 24] == 9).all() and not valid[:, 24].any()


def test_identity_maps_return_the_input(ctx):
    c = R.IDENTITY
    maps = ctx.rectifyMaps(c["K"], c["D"], c["R"], c["P"], (37, 53))
    for ch in (1, 3):
        img = R.test_image(37, 53, ch, seed=6)
        out, valid = ctx.rectify(img, maps, return_valid=True)
        assert np.array_equal(out, img) and valid.all()


def test_stereo_disparity_with_rectify(ctx):
    H, W = 48, 96
    rng = np.random.RandomState(7)
    right = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    left = np.roll(right, 5, axis=1)
    K = np.array([[90.0, 0, 47.5], [0, 90, 23.5], [0, 0, 1]])
    P = np.hstack([K, np.zeros((3, 1))])
    D = 0.1 * R.D_GENERAL
    ml = ctx.rectifyMaps(K, D, R.rodrigues((0.004, -0.006, 0.003)), P, (H, W))
    mr = ctx.rectifyMaps(K, -D, R.rodrigues((-0.003, 0.005, -0.002)), P, (H, W))
    kw = dict(n_disparities=32, return_cost=True)
    got = ctx.stereoDisparity(left, right, rectify=(ml, mr), **kw)
    want = ctx.stereoDisparity(ctx.rectify(left, ml), ctx.rectify(right, mr), **kw)
    assert all(np.array_equal(g, w) for g, w in zip(got, want)) and want[0].any()
    plain = ctx.stereoDisparity(left, right, **kw)
    assert not np.array_equal(plain[0], want[0])  # the maps really took part
    ident = ctx.rectifyMaps(K, np.zeros(4), np.eye(3), P, (H, W))
    same = ctx.stereoDisparity(left, right, rectify=(ident, ident), **kw)
    assert all(np.array_equal(g, w) for g, w in zip(same, plain))


def test_bad_arguments_zero_host_outputs_and_launch_nothing(ctx, general_maps):
    from online_3d_reconstruction_amd import _lib as L
    lib = L.load_library()
    H, W, F, HO, WO = 37, 53, 2, 41, 50
    src = np.stack([R.test_image(H, W, 1, seed=s) for s in (1, 2)])
    maps = general_maps[(HO, WO)]
    kinds = (L.K_RECTIFY_MAPS, L.K_RECTIFY_REMAP)

    def camera(case=R.GENERAL, **kw):
        cam = L.RectifyCameraStruct()
        v = dict(K=case["K"], D=R.pad_D(case["D"]), R=case["R"], P=case["P"])
        v.update(kw)
        for name in "KDRP":
            getattr(cam, name)[:] = np.asarray(v[name], np.float64).reshape(-1).tolist()
        return cam

    def call_maps(cam, rows_out=HO, cols_out=WO, mem=0):
        out = np.full((HO, WO, 2), 0x5A5A5A5A, np.int32)
        return lib.o3dr_rectify_maps(ctx._h, C.byref(cam), rows_out, cols_out, out.ctypes.data, mem), out

    def call_remap(pitch=W, fs=H * W, rows=H, cols=W, channels=1, n_frames=F, rows_out=HO, cols_out=WO, border=0, group_frames=0, mem=0,
                   out=None):
        buf = np.full((F, HO, WO), 0x5A, np.uint8) if out is None else out
        valid = np.full((HO, WO), 0x5A, np.uint8)
        rc = lib.o3dr_rectify_remap(ctx._h, src.ctypes.data, fs, pitch, rows, cols, channels, n_frames, maps.ctypes.data, rows_out, cols_out,
                                    border, group_frames, buf.ctypes.data, valid.ctypes.data, mem)
        return rc, buf, valid

    rc, out = call_maps(camera())
    assert rc == 0 and np.array_equal(out, maps)
    rc, buf, valid = call_remap()
    want, want_valid = R.rectify_remap_frames(src, maps, 0)
    assert rc == 0 and np.array_equal(buf, want) and np.array_equal(valid, want_valid)
    rc, buf, valid = call_remap(n_frames=0)  # O3DR_OK, nothing touched
    assert rc == 0 and (buf == 0x5A).all() and (valid == 0x5A).all()

    ctx.profileEnable(-1, True)
    ctx.profileReset()
    singular = np.array([[44.0, 0, 24.5, 0], [0, 0, 20.25, 0], [0, 0, 1, 0]])  # fy = 0: with R = I the determinant is exactly 0
    with pytest.raises(ValueError):
        R.inverse_PR(np.eye(3), singular)
    k_skew = R.GENERAL["K"].copy()
    k_skew[0, 1] = 0.5
    d_nan = R.pad_D(R.D_GENERAL)
    d_nan[3] = np.nan
    r_inf = R.GENERAL["R"].copy()
    r_inf[1, 1] = np.inf
    for what, cam in (("singular P R", camera(P=singular, R=np.eye(3))), ("K[1] != 0", camera(K=k_skew)), ("NaN in D", camera(D=d_nan)),
                      ("inf in R", camera(R=r_inf))):
        rc, out = call_maps(cam)
        assert rc == L.ERR_INVALID_ARG and not out.any(), what
    for kw in (dict(rows_out=0), dict(cols_out=0), dict(rows_out=8193), dict(cols_out=8193)):  # sizes unknown: nothing is written
        rc, out = call_maps(camera(), **kw)
        assert rc == L.ERR_INVALID_ARG and (out == 0x5A5A5A5A).all(), kw
    rc, out = call_maps(camera(), mem=2)
    assert rc == L.ERR_INVALID_ARG and (out == 0x5A5A5A5A).all()
    assert lib.o3dr_rectify_maps(ctx._h, None, HO, WO, out.ctypes.data, 0) == L.ERR_INVALID_ARG and not out.any()

    for kw in (dict(channels=2), dict(border=256), dict(border=-1), dict(group_frames=-1), dict(pitch=W - 1), dict(fs=H * W - 1),
               dict(rows=0), dict(cols=0), dict(rows=8193), dict(cols=8193)):
        rc, buf, valid = call_remap(**kw)
        assert rc == L.ERR_INVALID_ARG and not valid.any(), kw
        assert not buf.any() or kw.get("channels") == 2, kw  # (channels outside 1 / 3: the size of `out` is unknown)
    for kw in (dict(rows_out=0), dict(cols_out=0), dict(rows_out=8193), dict(cols_out=8193), dict(n_frames=-1), dict(mem=2)):
        rc, buf, valid = call_remap(**kw)
        assert rc == L.ERR_INVALID_ARG and (buf == 0x5A).all() and (valid == 0x5A).all(), kw
    # `out` inside the source's bytes
    both = np.zeros(F * H * W + F * HO * WO, np.uint8)
    both[:F * H * W] = src.reshape(-1)
    rc = lib.o3dr_rectify_remap(ctx._h, both.ctypes.data, H * W, W, H, W, 1, F, maps.ctypes.data, HO, WO, 0, 0, both.ctypes.data + F * H * W - 1,
                                None, 0)
    assert rc == L.ERR_INVALID_ARG
    assert lib.o3dr_rectify_remap(ctx._h, src.ctypes.data, H * W, W, H, W, 1, F, None, HO, WO, 0, 0, buf.ctypes.data, None, 0) == L.ERR_INVALID_ARG
    assert lib.o3dr_rectify_remap(None, src.ctypes.data, H * W, W, H, W, 1, F, maps.ctypes.data, HO, WO, 0, 0, buf.ctypes.data, None, 0) == L.ERR_INVALID_ARG
    # maps of another memory kind than the image
    import torch
    with pytest.raises(L.O3drError) as e:
        ctx.rectify(src, torch.from_numpy(maps).cuda())
    assert e.value.code == L.ERR_INVALID_ARG
    with pytest.raises(L.O3drError) as e:
        ctx.rectify(torch.from_numpy(src).cuda(), maps)
    assert e.value.code == L.ERR_INVALID_ARG
    assert all(ctx.profileRead(k)[1] == 0 for k in kinds), "a rejected call launched a kernel"

    # the launches depend on the sizes and the switches alone: one for a map, one per group of frames
    assert call_maps(camera())[0] == 0 and call_maps(camera(R.SENTINEL))[0] == 0
    assert ctx.profileRead(L.K_RECTIFY_MAPS)[1] == 2
    for g, n in ((0, 1), (1, 2), (2, 1)):
        ctx.profileReset()
        assert call_remap(group_frames=g)[0] == 0
        assert ctx.profileRead(L.K_RECTIFY_REMAP)[1] == n and ctx.profileRead(L.K_RECTIFY_MAPS)[1] == 0, g
    ctx.profileEnable(-1, False)
    ctx.profileReset()
