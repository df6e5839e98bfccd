"""Plane-fitted disparity per segment label (--use_segment_labels): o3dr_plane_fit_disparity / Context.planeFitDisparity
against the contract of include/o3dr.h restated in numpy - int64 sums, then the fp64 fit operation by operation (numpy's
elementwise *, -, / are single correctly rounded IEEE operations, like the library built with -ffp-contract=off).  Every
comparison on the GPU is bit for bit, on the f64 image and on the (frame, label) records."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT, load_frame

POSE_BIN = os.path.join(ROOT, "online_3d_reconstruction_amd", "bin", "pose")
TOL = 2.0 ** -20
NONE, MEAN, PLANE = 0, 1, 2


# ---- the contract in numpy -------------------------------------------------------------------------------------------
def ref_sums(disp, labels, n_labels, min_disparity=0.0):
    """[n_labels, 11] int64: n Sx Sy Sxx Sxy Syy Sd Sxd Syd Sdd over the participating pixels, then the pixel count"""
    rows, cols = disp.shape
    y, x = np.mgrid[0:rows, 0:cols].astype(np.int64)
    d = disp.astype(np.int64)
    lab = labels.astype(np.int64).ravel()
    part = (disp.astype(np.float64) > min_disparity).ravel()
    out = np.zeros((n_labels, 11), np.int64)
    terms = [np.ones_like(d), x, y, x * x, x * y, y * y, d, x * d, y * d, d * d]
    for k, t in enumerate(terms):  # (every partial sum is an integer < 2^53: bincount's fp64 accumulation is exact)
        out[:, k] = np.bincount(lab[part], weights=t.ravel()[part].astype(np.float64), minlength=n_labels).astype(np.int64)
    out[:, 10] = np.bincount(lab, minlength=n_labels)
    return out


def ref_fit(sums, min_pixels=3, max_mse=0.0):
    """include/o3dr.h steps 3 and 4 -> dict of arrays a b c0 mx my mse n_pixels n status"""
    s = sums.astype(np.float64)  # exact: every sum < 2^53
    n_int = sums[:, 0]
    has = n_int > 0
    n = np.where(has, s[:, 0], 1.0)
    Sx, Sy, Sxx, Sxy, Syy, Sd, Sxd, Syd, Sdd = (s[:, k] for k in range(1, 10))
    mx, my, c0 = Sx / n, Sy / n, Sd / n
    cxx, cxy, cyy = Sxx - Sx * mx, Sxy - Sx * my, Syy - Sy * my
    cxd, cyd, cdd = Sxd - Sd * mx, Syd - Sd * my, Sdd - Sd * c0
    det = cxx * cyy - cxy * cxy
    degenerate = det <= (TOL * cxx) * cyy
    plane = has & ~(n_int < min_pixels) & ~degenerate
    safe = np.where(plane, det, 1.0)
    a = np.where(plane, (cxd * cyy - cyd * cxy) / safe, 0.0)
    b = np.where(plane, (cyd * cxx - cxd * cxy) / safe, 0.0)
    mse = ((cdd - a * cxd) - b * cyd) / n
    status = np.where(plane, PLANE, MEAN)
    if max_mse > 0:
        status = np.where(mse > max_mse, NONE, status)
    status = np.where(has, status, NONE)
    z = lambda v: np.where(has, v, 0.0)  # noqa: E731
    return dict(a=z(a), b=z(b), c0=z(c0), mx=z(mx), my=z(my), mse=z(mse), n_pixels=sums[:, 10], n=n_int, status=status)


def ref_image(disp, labels, fit, min_disparity=0.0, fill=True):
    rows, cols = disp.shape
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    lab = labels.astype(np.int64)
    d = disp.astype(np.float64)
    val = (fit["c0"][lab] + fit["a"][lab] * (x - fit["mx"][lab])) + fit["b"][lab] * (y - fit["my"][lab])
    use = fit["status"][lab] != NONE
    if not fill:
        use &= d > min_disparity
    return np.where(use, val, d)


def ref_plane_fit(disp, labels, n_labels, min_disparity=0.0, min_pixels=3, max_mse=0.0, fill=True):
    """stack in, (f64 stack, list of fits) out"""
    imgs, fits = [], []
    for d, l in zip(disp, labels):
        fit = ref_fit(ref_sums(d, l, n_labels, min_disparity), min_pixels, max_mse)
        fits.append(fit)
        imgs.append(ref_image(d, l, fit, min_disparity, fill))
    return np.stack(imgs), fits


def assert_bits_equal(got, ref, what):
    got, ref = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(ref, np.float64)
    assert got.shape == ref.shape, what
    bad = got.view(np.uint64) != ref.view(np.uint64)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def assert_records_equal(rec, fits, what):
    for f, fit in enumerate(fits):
        r = rec[f]
        for k in ("a", "b", "c0", "mx", "my", "mse"):
            assert_bits_equal(r[k], fit[k], f"{what}: frame {f} {k}")
        for k in ("n_pixels", "n", "status"):
            assert np.array_equal(r[k].astype(np.int64), fit[k].astype(np.int64)), f"{what}: frame {f} {k}"
        assert not r["reserved"].any()


# ---- label maps --------------------------------------------------------------------------------------------------------
def blocky(rows, cols, bh, bw):
    y, x = np.mgrid[0:rows, 0:cols]
    return (y // bh) * ((cols + bw - 1) // bw) + x // bw


def voronoi(rows, cols, n_seeds, seed):
    rng = np.random.default_rng(seed)
    sy, sx = rng.integers(0, rows, n_seeds), rng.integers(0, cols, n_seeds)
    y, x = np.mgrid[0:rows, 0:cols]
    return np.argmin((y[..., None] - sy) ** 2 + (x[..., None] - sx) ** 2, axis=-1)


def rand_disp(shape, seed, zero_frac=0.1):
    rng = np.random.default_rng(seed)
    d = rng.integers(1, 256, shape).astype(np.uint8)
    d[rng.random(shape) < zero_frac] = 0
    return d


# ---- CPU: the restatement on hand cases --------------------------------------------------------------------------------
def _fit_of(points, d, n_labels=1, shape=None, **kw):
    """one segment (label 0) holding `points` (x, y) with disparities d in an otherwise d = 0, label 0 image"""
    pts = np.asarray(points)
    shape = shape or (int(pts[:, 1].max()) + 1, int(pts[:, 0].max()) + 1)
    sums = np.zeros((n_labels, 11), np.int64)
    x, y, d = pts[:, 0].astype(np.int64), pts[:, 1].astype(np.int64), np.asarray(d, np.int64)
    sums[0, :10] = [len(x), x.sum(), y.sum(), (x * x).sum(), (x * y).sum(), (y * y).sum(), d.sum(), (x * d).sum(), (y * d).sum(),
                    (d * d).sum()]
    sums[0, 10] = len(x)
    return ref_fit(sums, **kw)


def test_restatement_recovers_an_exact_plane():
    disp = np.zeros((8, 8), np.uint8)
    y, x = np.mgrid[0:4, 0:4]
    disp[2:6, 3:7] = 2 * (x + 3) + 3 * (y + 2) + 5
    labels = np.zeros((8, 8), np.uint8)
    labels[2:6, 3:7] = 1
    fit = ref_fit(ref_sums(disp, labels, 2))
    assert fit["status"].tolist() == [NONE, PLANE] and fit["n"].tolist() == [0, 16] and fit["n_pixels"].tolist() == [48, 16]
    assert fit["a"][1] == 2.0 and fit["b"][1] == 3.0 and fit["mse"][1] == 0.0
    assert fit["mx"][1] == 4.5 and fit["my"][1] == 3.5 and fit["c0"][1] == 2 * 4.5 + 3 * 3.5 + 5
    img = ref_image(disp, labels, fit)
    assert np.array_equal(img, disp.astype(np.float64))  # the plane reproduces its own samples, label 0 keeps d


@pytest.mark.parametrize("at", [0, 4000, 8191 - 40])
def test_restatement_rows_columns_and_diagonals_are_mean(at):
    t = np.arange(40)
    rng = np.random.default_rng(at)
    for pts in ([(at + i, at + 7) for i in t], [(at + 7, at + i) for i in t], [(at + i, at + i) for i in t],
                [(at + i, at + 39 - i) for i in t], [(at + 2 * i, at + 3 * i) for i in range(13)], [(at, at), (at + 1, at + 1)],
                [(8191, 8191)], [(at + i, at + 3) for i in (0, 5, 6, 30)]):
        fit = _fit_of(pts, rng.integers(1, 256, len(pts)))
        assert fit["status"][0] == MEAN and fit["a"][0] == 0 and fit["b"][0] == 0, pts[:3]
    # a whole row, column and diagonal of the largest image
    full = np.arange(8192)
    for pts in (np.stack([full, np.full(8192, 8191)], 1), np.stack([np.full(8192, 8191), full], 1), np.stack([full, full], 1)):
        assert _fit_of(pts, rng.integers(1, 256, 8192))["status"][0] == MEAN


def test_restatement_l_triple_is_a_plane_anywhere():
    for cx, cy in ((0, 0), (8190, 8190), (8190, 0), (0, 8190), (4095, 8190)):
        for tri in ([(0, 0), (1, 0), (0, 1)], [(1, 1), (1, 0), (0, 1)], [(0, 0), (1, 1), (0, 1)], [(0, 0), (1, 0), (1, 1)]):
            pts = [(cx + px, cy + py) for px, py in tri]
            d = [10 + 3 * px + 7 * py for px, py in tri]
            fit = _fit_of(pts, d)
            assert fit["status"][0] == PLANE, pts
            assert abs(fit["a"][0] - 3) < 1e-5 and abs(fit["b"][0] - 7) < 1e-5 and abs(fit["mse"][0]) < 1e-5
    assert _fit_of([(8190, 8190), (8191, 8190), (8190, 8191)], [1, 2, 3], min_pixels=4)["status"][0] == MEAN


def test_restatement_empty_segment_gate_and_fill():
    disp = np.array([[0, 0, 9, 9], [0, 0, 9, 0], [5, 6, 0, 0], [5, 7, 0, 0]], np.uint8)
    labels = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [2, 2, 3, 3], [2, 2, 3, 3]], np.uint8)
    fit = ref_fit(ref_sums(disp, labels, 5))
    assert fit["status"].tolist() == [NONE, PLANE, PLANE, NONE, NONE] and fit["n_pixels"].tolist() == [4, 4, 4, 4, 0]
    # three equal samples: the constant plane, up to the rounding of mx = 7/3 (a few ulp of Sd * mx = 63, over det = 1/3)
    assert abs(fit["a"][1]) < 1e-12 and abs(fit["b"][1]) < 1e-12 and abs(fit["mse"][1]) < 1e-12
    filled = ref_image(disp, labels, fit, fill=True)
    kept = ref_image(disp, labels, fit, fill=False)
    assert abs(filled[1, 3] - 9.0) < 1e-12 and kept[1, 3] == 0.0  # the hole is filled only with fill
    assert np.array_equal(filled[:2, :2], np.zeros((2, 2))) and np.array_equal(filled[2:, 2:], np.zeros((2, 2)))
    gated = ref_fit(ref_sums(disp, labels, 5), max_mse=1e-3)
    assert gated["status"].tolist() == [NONE, PLANE, NONE, NONE, NONE] and gated["mse"][2] > 1e-3
    assert ref_fit(ref_sums(disp, labels, 5, min_disparity=8.0))["status"].tolist() == [NONE, PLANE, NONE, NONE, NONE]


# ---- CPU: the ABI without a device and the 16-bit PNG reader -------------------------------------------------------------
def test_defaults_and_record_layout():
    from online_3d_reconstruction_amd import _lib
    L = _lib.load_library()
    p = _lib.PlaneDispParamsStruct(1.0, 1, 1.0, 0)
    L.o3dr_plane_disp_default_params(C.byref(p))
    assert (p.min_disparity, p.min_pixels, p.max_mse, p.fill) == (0.0, 3, 0.0, 1)
    assert _lib.PLANE_DISP_SEGMENT.itemsize == 64 and _lib.PLANE_DISP_SEGMENT.fields["status"][1] == 56
    st = C.c_uint32(7)
    assert L.o3dr_plane_fit_disparity(None, None, 0, 0, None, 1, 0, 0, 1, 1, 1, 0, None, None, None, C.byref(st), 0) == -1
    assert st.value == 0 and b"ctx" in L.o3dr_last_error()


def _png_chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def write_png_grey(path, img, depth):
    """greyscale PNG of 8 or 16 bits, rows filtered None / Sub / Up in turn"""
    rows, cols = img.shape
    raw = img.astype(">u2" if depth == 16 else np.uint8).view(np.uint8).reshape(rows, -1).astype(np.int32)
    bpp = depth // 8
    out = bytearray()
    for y in range(rows):
        ft = y % 3
        left = np.concatenate([np.zeros(bpp, np.int32), raw[y, :-bpp]])
        up = raw[y - 1] if y else np.zeros_like(raw[y])
        line = raw[y] if ft == 0 else (raw[y] - left if ft == 1 else raw[y] - up)
        out += bytes([ft]) + (line & 255).astype(np.uint8).tobytes()
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, depth, 0, 0, 0, 0)) +
                _png_chunk(b"IDAT", zlib.compress(bytes(out))) + _png_chunk(b"IEND", b""))


@pytest.mark.parametrize("depth", [16, 8])
def test_label_png_reader(tmp_path, depth):
    rng = np.random.default_rng(depth)
    img = rng.integers(0, 65536 if depth == 16 else 256, (13, 21))
    img[0, :3] = [0, 65535 if depth == 16 else 255, 256 if depth == 16 else 1]
    path = str(tmp_path / "labels.png")
    write_png_grey(path, img, depth)
    res = subprocess.run([POSE_BIN, "--print_label_png", path], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.strip().splitlines()
    assert lines[0].split() == ["13", "21"]
    assert np.array_equal(np.array([l.split() for l in lines[1:]], np.int64), img)
    if depth == 16:  # a second writer
        from PIL import Image
        Image.fromarray(img.astype(np.uint16)).save(path)
        res = subprocess.run([POSE_BIN, "--print_label_png", path], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0 and np.array_equal(np.array([l.split() for l in res.stdout.strip().splitlines()[1:]], np.int64), img)
        Image.fromarray(rng.integers(0, 255, (4, 4, 3)).astype(np.uint8), "RGB").save(path)  # not a label image
        assert subprocess.run([POSE_BIN, "--print_label_png", path], capture_output=True, text=True, timeout=60).returncode != 0


def test_cli_refuses_the_flag_where_it_is_not_supported(tmp_path):
    for extra in (["--gpus", "2"], ["--partitioned_merge"], ["--reference_fanout"], ["--blur_kernel", "5"]):
        res = subprocess.run([POSE_BIN, "1", "2", "--use_segment_labels", "--data_dir", str(tmp_path) + "/"] + extra,
                             capture_output=True, text=True, timeout=60)
        assert res.returncode != 0 and "--use_segment_labels" in res.stdout + res.stderr, extra
        assert "ignored in this build" not in res.stdout


# ---- GPU ---------------------------------------------------------------------------------------------------------------
CASES = {
    # name: (labels [F,H,W] or [H,W], dtype, disp seed or array, kwargs)
    "blocky_37x53_u8": lambda: (blocky(37, 53, 5, 7), np.uint8, 1, {}),
    "blocky_odd_u16": lambda: (blocky(131, 259, 9, 11), np.uint16, 2, {}),
    "blocky_u32_stack": lambda: (np.stack([blocky(70, 300, 8 + f, 13) for f in range(3)]), np.uint32, 3, {}),
    "voronoi_u16": lambda: (voronoi(96, 150, 40, 4), np.uint16, 4, {}),
    "voronoi_min_disparity": lambda: (voronoi(96, 150, 40, 5), np.uint8, 5, dict(min_disparity=100.5)),
    "column_stripes": lambda: (np.mgrid[0:40, 0:300][1] % 300, np.uint16, 6, {}),
    "row_stripes": lambda: (np.mgrid[0:300, 0:40][0], np.uint16, 7, {}),
    "diagonal_stripes": lambda: (np.add(*np.mgrid[0:64, 0:200]) % 97, np.uint8, 8, {}),
    "stripes_alias_the_lds_slots": lambda: (np.mgrid[0:40, 0:384][1] * 256 % 65536 + np.mgrid[0:40, 0:384][1] // 256, np.uint16, 9, {}),
    "one_label": lambda: (np.zeros((45, 130), np.int64), np.uint8, 10, {}),
    "65536_labels": lambda: (blocky(512, 512, 2, 2), np.uint16, 11, dict(n_labels=65536)),
    "65536_labels_u32_stack": lambda: (np.stack([blocky(256, 256, 1, 1), blocky(256, 256, 2, 2)]), np.uint32, 12, dict(n_labels=65536)),
    "min_pixels_above_the_block": lambda: (blocky(60, 90, 3, 3), np.uint8, 13, dict(min_pixels=10)),
    "max_mse": lambda: (blocky(60, 90, 6, 6), np.uint8, 14, dict(max_mse=5000.0)),
    "no_fill": lambda: (blocky(61, 93, 6, 5), np.uint16, 15, dict(fill=False, min_disparity=30.0)),
    "rows_8192": lambda: (blocky(8192, 9, 100, 4), np.uint16, 16, {}),
    "cols_8192": lambda: (blocky(5, 8192, 2, 300), np.uint16, 17, {}),
    "all_invalid": lambda: (blocky(20, 20, 4, 4), np.uint8, np.zeros((20, 20), np.uint8), {}),
}


def _case(name):
    labels, dtype, disp, kw = CASES[name]()
    labels = np.ascontiguousarray(labels.astype(dtype))
    if not isinstance(disp, np.ndarray):
        disp = rand_disp(labels.shape, disp)
    kw = dict(kw)
    n_labels = kw.pop("n_labels", int(labels.max()) + 1)
    return disp, labels, n_labels, kw


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_plane_fit_equals_the_restatement(ctx, name):
    import torch
    disp, labels, n_labels, kw = _case(name)
    d3, l3 = (disp[None], labels[None]) if disp.ndim == 2 else (disp, labels)
    ref_img, fits = ref_plane_fit(d3, l3, n_labels, **kw)
    got, rec = ctx.planeFitDisparity(disp, labels, n_labels=n_labels, return_segments=True, **kw)
    assert got.dtype == np.float64 and got.shape == disp.shape
    assert_bits_equal(got.reshape(ref_img.shape), ref_img, name)
    assert_records_equal(rec.reshape(len(fits), n_labels), fits, name)
    # device tensors: the same bits, nothing leaves HBM
    lt = torch.from_numpy(labels.view({1: np.uint8, 2: np.int16, 4: np.int32}[labels.itemsize])).cuda()
    got_d, rec_d = ctx.planeFitDisparity(torch.from_numpy(disp).cuda(), lt, n_labels=n_labels, return_segments=True, **kw)
    assert got_d.is_cuda and got_d.dtype == torch.float64
    assert_bits_equal(got_d.cpu().numpy().reshape(ref_img.shape), ref_img, name + " (device)")
    assert rec_d.tobytes() == rec.tobytes()
    # without the records
    assert_bits_equal(ctx.planeFitDisparity(disp, labels, n_labels=n_labels, **kw).reshape(ref_img.shape), ref_img, name + " (no records)")


@pytest.mark.gpu
def test_golden_frames_strided_stack_and_batching(Q, frame_1248, frame_B):
    """the bundled frames under synthetic labels, as views with row and frame strides; another frame batching (another
    launch geometry: O3DR_BATCH_FRAMES is read at context creation) gives the same bits"""
    import online_3d_reconstruction_amd as o3dr
    frames = [frame_1248[0], load_frame("1249")[0], load_frame("1251")[0]]
    rows, cols = frames[0].shape
    pad_d = np.zeros((3, rows + 3, cols + 21), np.uint8)
    pad_l = np.full((3, rows + 1, cols + 6), 60000, np.uint16)
    disp, labels = pad_d[:, 2:rows + 2, 5:cols + 5], pad_l[:, :rows, 3:cols + 3]
    for f, d in enumerate(frames):
        disp[f] = d
        labels[f] = blocky(rows, cols, 24 + 7 * f, 40 - 3 * f) if f != 1 else voronoi(rows // 4, cols // 4, 60, 1).repeat(4, 0).repeat(4, 1)
    n_labels = int(labels.max()) + 1
    ref_img, fits = ref_plane_fit(disp, labels, n_labels)
    results = []
    for batch in ("1", "2", None):
        old = os.environ.pop("O3DR_BATCH_FRAMES", None)
        if batch:
            os.environ["O3DR_BATCH_FRAMES"] = batch
        try:
            with o3dr.Context(0, Q=Q) as c:
                results.append(c.planeFitDisparity(disp, labels, n_labels=n_labels, return_segments=True))
        finally:
            os.environ.pop("O3DR_BATCH_FRAMES", None)
            if old is not None:
                os.environ["O3DR_BATCH_FRAMES"] = old
    for got, rec in results:
        assert_bits_equal(got, ref_img, "strided stack")
        assert_records_equal(rec, fits, "strided stack")
    bd, bb = frame_B
    lb = blocky(bd.shape[0], bd.shape[1], 17, 29).astype(np.uint16)
    with o3dr.Context(0, Q=Q) as c:
        got = c.planeFitDisparity(bd, lb)
    assert_bits_equal(got, ref_plane_fit(bd[None], lb[None], int(lb.max()) + 1)[0][0], "frame_B")


@pytest.mark.gpu
def test_far_corner_of_the_largest_image(ctx):
    """8192 x 8192 on the device: an L triple, a 2-pixel diagonal and a column at the far corner, everything else d = 0 in
    label 0 (no participating pixel).  The records against the restatement from the few pixels; the image by region."""
    import torch
    N = 8192
    disp = torch.zeros((N, N), dtype=torch.uint8, device="cuda")
    labels = torch.zeros((N, N), dtype=torch.uint8, device="cuda")
    segs = {1: [(8190, 8190), (8191, 8190), (8190, 8191)], 2: [(8000, 8190), (8001, 8191)], 3: [(8100, 8180 + i) for i in range(12)]}
    vals = {1: [10, 13, 17], 2: [200, 100], 3: [5 + 20 * i for i in range(12)]}
    for lab, pts in segs.items():
        for (x, y), v in zip(pts, vals[lab]):
            disp[y, x], labels[y, x] = v, lab
    out, rec = ctx.planeFitDisparity(disp, labels, n_labels=4, return_segments=True)
    assert rec["status"].tolist() == [NONE, PLANE, MEAN, MEAN] and int(rec["n_pixels"][0]) == N * N - 17
    for lab, pts in segs.items():
        fit = _fit_of(pts, vals[lab])
        for k in ("a", "b", "c0", "mx", "my", "mse"):
            assert_bits_equal(rec[k][lab], fit[k][0], f"label {lab} {k}")
        for x, y in pts:
            want = (fit["c0"][0] + fit["a"][0] * (np.float64(x) - fit["mx"][0])) + fit["b"][0] * (np.float64(y) - fit["my"][0])
            assert np.float64(out[y, x].item()).tobytes() == np.float64(want).tobytes()
    assert int(torch.count_nonzero(out).item()) == 17 and bool(torch.isfinite(out).all().item())


@pytest.mark.gpu
def test_chain_into_create_single_img_pt_cloud(ctx, orc, Q, frame_1248):
    """planeFitDisparity -> createSingleImgPtCloud / accumulateFrames under Params(disparity_f64=True) equals the oracle's
    f64 A1 (and A6) on the numpy-restated image"""
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import synth
    disp, bgr = frame_1248
    labels = blocky(disp.shape[0], disp.shape[1], 45, 64).astype(np.uint16)
    ref_img = ref_plane_fit(disp[None], labels[None], int(labels.max()) + 1)[0][0]
    fitted = ctx.planeFitDisparity(disp, labels)
    assert_bits_equal(fitted, ref_img, "fitted image")
    T = synth.make_pose(2)
    ctx.set_camera(Q)
    ctx.set_params(o3dr.Params(jump_pixels=7, voxel_size=0.05, sor_enable=False, disparity_f64=True))
    try:
        ref1 = orc.create_single_img_pt_cloud(ref_img, bgr, Q, jump_pixels=7)
        got1 = ctx.createSingleImgPtCloud(fitted, bgr)
        assert len(ref1) > 1000 and got1.tobytes() == ref1.tobytes()
        ref6 = orc.downsample_pt_cloud(orc.transform_pt_cloud(ref1, T), 0.05, False, 1)[0]
        ctx.cloudBigReset()
        stack = ctx.planeFitDisparity(np.stack([disp, disp]), np.stack([labels, labels]))  # [F,H,W] in, [F,H,W] out
        ctx.accumulateFrames(stack, np.stack([bgr, bgr]), np.stack([T, T]).astype(np.float32))
        assert ctx.cloudBigRead().tobytes() == np.concatenate([ref6, ref6]).tobytes()
    finally:
        ctx.set_params(o3dr.Params())
        ctx.cloudBigReset()


@pytest.mark.gpu
def test_errors(ctx):
    import torch
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib
    disp = rand_disp((20, 30), 1)
    labels = blocky(20, 30, 4, 4).astype(np.uint16)
    n_labels = int(labels.max()) + 1
    good = ctx.planeFitDisparity(disp, labels)
    bad = labels.copy()
    bad[7, 11] = n_labels  # one label out of range: the status bit, an error, host outputs zeroed
    L, h = ctx._lib, ctx._h
    out = np.ones((20, 30), np.float64)
    rec = np.ones(n_labels, _lib.PLANE_DISP_SEGMENT)
    st = C.c_uint32(0)
    call = lambda **k: L.o3dr_plane_fit_disparity(  # noqa: E731
        h, k.get("disp", disp.ctypes.data), k.get("dp", 30), 600, k.get("labels", bad.ctypes.data), k.get("es", 2), k.get("lp", 60), 1200,
        k.get("n_labels", n_labels), k.get("rows", 20), k.get("cols", 30), k.get("F", 1), None, k.get("out", out.ctypes.data),
        rec.ctypes.data, C.byref(st), k.get("mem", 0))
    assert call() == _lib.ERR_INVALID_ARG and st.value == _lib.STATUS_LABEL_RANGE
    assert not out.any() and not rec.view(np.uint8).any()
    with pytest.raises(o3dr.O3drError):
        ctx.planeFitDisparity(torch.from_numpy(disp).cuda(), torch.from_numpy(bad.view(np.int16)).cuda(), n_labels=n_labels)
    with pytest.raises(o3dr.O3drError):  # 0xFFFFFFFF in 4-byte labels
        ctx.planeFitDisparity(disp, np.full((20, 30), 0xFFFFFFFF, np.uint32), n_labels=65536)
    for k in (dict(es=3), dict(es=8), dict(rows=8193), dict(cols=8193), dict(rows=0), dict(cols=0), dict(n_labels=0), dict(n_labels=65537),
              dict(F=-1), dict(mem=2), dict(disp=None), dict(labels=None), dict(out=None), dict(dp=29), dict(lp=58), dict(lp=61),
              dict(labels=bad.ctypes.data + 1), dict(out=out.ctypes.data + 4)):
        st.value = 5
        assert call(**k) == _lib.ERR_INVALID_ARG and st.value == 0, k
    assert call(F=0, disp=None, labels=None, out=None) == 0  # empty input: nothing read, nothing written
    for prm in ((float("nan"), 3, 0.0, 1), (0.0, 3, float("nan"), 1), (0.0, 3, -1.0, 1)):
        p = _lib.PlaneDispParamsStruct(*prm)
        assert L.o3dr_plane_fit_disparity(h, disp.ctypes.data, 30, 600, labels.ctypes.data, 2, 60, 1200, n_labels, 20, 30, 1, C.byref(p),
                                          out.ctypes.data, None, None, 0) == _lib.ERR_INVALID_ARG
    assert ctx.planeFitDisparity(disp[:0].reshape(0, 20, 30), labels[:0].reshape(0, 20, 30), n_labels=3).shape == (0, 20, 30)
    assert_bits_equal(ctx.planeFitDisparity(disp, labels), good, "the context stays usable after the errors")


@pytest.mark.gpu
def test_cli_use_segment_labels(tmp_path, Q):
    """pose first last --use_segment_labels on a small data directory: cloud.ply equals the Python chain
    (planeFitDisparity -> accumulateFrames under disparity_f64 -> finalize); a frame without a label image is rejected"""
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import synth
    from PIL import Image
    from test_cli_pose import _read_ply, _write_dataset, pose_row_for_image
    tmp = str(tmp_path)
    names = ("1248", "1249", "1251")
    _write_dataset(tmp, names)
    os.makedirs(tmp + "/labels")
    labels = {}
    for i, name in enumerate(names[:2]):  # 1251 has no label image
        rows, cols = load_frame(name)[0].shape
        labels[name] = (blocky(rows, cols, 30 + 5 * i, 40) * 50).astype(np.uint16)  # (labels above 255: 16 bits needed)
        Image.fromarray(labels[name]).save(tmp + "/labels/" + name + ".png")
    cmd = [POSE_BIN, "1247", "1252", "--jump_pixels", "15", "--voxel_size", "0.05", "--only_MAVLink", "--sor", "0",
           "--data_dir", tmp + "/data_files/", "--image_dir", tmp + "/images/", "--disparity_dir", tmp + "/disparities/",
           "--output_dir", tmp + "/output/", "--use_segment_labels", "--segment_labels_dir", tmp + "/labels/", "--plane_min_pixels", "4"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "ignored in this build" not in res.stdout and "plane-fitted disparity: 2 frames" in res.stdout
    assert "1251 could not read segment label image" in res.stdout and res.stdout.count("Accepted!") == 2
    got = _read_ply(tmp + "/output/cloud.ply")
    disp = np.stack([load_frame(n)[0] for n in names[:2]])
    bgr = np.stack([load_frame(n)[1] for n in names[:2]])
    lab = np.stack([labels[n] for n in names[:2]])
    poses = np.stack([synth.generate_tmat(*(lambda r: (r[3:6], r[6:10]))(pose_row_for_image(int(n))[1])) for n in names[:2]])
    with o3dr.Context(0, Q=Q, params=o3dr.Params(jump_pixels=15, voxel_size=0.05, sor_enable=False, disparity_f64=True)) as c:
        fitted = c.planeFitDisparity(disp, lab, min_pixels=4)
        c.accumulateFrames(fitted, bgr, poses.astype(np.float32))
        ref = c.finalize()
    assert len(ref) > 100 and len(got) == len(ref)
    for ax in "xyz":
        assert np.array_equal(got[ax], ref[ax]), ax
    assert np.array_equal(got["r"], (ref["rgba"] >> 16) & 255) and np.array_equal(got["b"], ref["rgba"] & 255)
