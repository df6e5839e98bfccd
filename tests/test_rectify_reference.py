"""CPU tests of the stereo-rectification contract (include/o3dr.h "stereo rectification") through its numpy restatement,
tests/rectify_reference.py: the identity, a general calibration checked against an independent inversion of the camera
model, the sentinel, the border and the zero-weight tap; and the host-only helper rectifiedQ."""
import numpy as np

import rectify_reference as R


def test_identity_map_and_remap():
    c = R.IDENTITY
    maps = R.maps_of(c)
    v, u = np.mgrid[0:37, 0:53]
    assert maps.dtype == np.int32 and np.array_equal(maps[..., 0], 32 * u) and np.array_equal(maps[..., 1], 32 * v)
    for ch in (1, 3):
        img = R.test_image(37, 53, ch, seed=1)
        out, valid = R.rectify_remap(img, maps)
        assert np.array_equal(out, img) and valid.all()


def _undistort(xd, yd, D, iterations=200):
    """the inverse of the distortion by fixed-point iteration (an independent route: not a restatement of the contract)"""
    k1, k2, p1, p2, k3, k4, k5, k6 = D
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (xd - dx) / kr, (yd - dy) / kr
    return x, y


def test_general_case_inverts_the_camera_model():
    c = R.GENERAL
    mx, my = R.source_positions(c["K"], c["D"], c["R"], c["P"], c["size"])
    K = c["K"]
    x, y = _undistort((mx - K[0, 2]) / K[0, 0], (my - K[1, 2]) / K[1, 1], R.pad_D(c["D"]))
    ray = np.einsum("ij,jhw->ihw", c["R"], np.stack([x, y, np.ones_like(x)]))
    pr = np.einsum("ij,jhw->ihw", c["P"][:, :3], ray)
    v, u = np.mgrid[0:41, 0:50]
    err = max(np.abs(pr[0] / pr[2] - u).max(), np.abs(pr[1] / pr[2] - v).max())
    print(f"round trip error {err:.3g} px")
    assert err < 1e-9

    maps = R.maps_of(c)
    assert not (maps == R.OUTSIDE).any()
    out, valid = R.rectify_remap(R.test_image(37, 53, 3, seed=2), maps, border=9)
    assert out.shape == (41, 50, 3) and valid.shape == (41, 50)
    print(f"valid {100.0 * valid.mean():.1f} %")
    assert round(100.0 * valid.mean(), 1) == 87.1  # both branches are exercised


def test_sentinel_column_and_pole():
    c = R.SENTINEL
    maps = R.maps_of(c)
    outside = (maps == R.OUTSIDE).all(axis=2)
    assert np.array_equal((maps == R.OUTSIDE).any(axis=2), outside)  # never one coordinate alone
    want = np.zeros((41, 50), bool)
    want[:, 24] = True
    assert np.array_equal(outside, want) and outside.sum() == 41
    out, valid = R.rectify_remap(R.test_image(37, 53, 1, seed=3), maps, border=9)
    assert (out[:, 24] == 9).all() and not valid[:, 24].any()
    pole = R.maps_of(R.POLE)
    hit = (pole == R.OUTSIDE).all(axis=2)
    assert hit.any() and not hit.all()
    out, valid = R.rectify_remap(R.test_image(37, 53, 1, seed=3), pole, border=200)
    assert (out[hit] == 200).all() and not valid[hit].any()


def test_border_value_appears_exactly_where_a_weighted_tap_is_outside():
    img = np.full((37, 53), 100, np.uint8)
    maps = R.maps_of(R.GENERAL)
    out, valid = R.rectify_remap(img, maps, border=9)
    # a constant image: the output is 100 wherever no border value was mixed in, and lower wherever one was (the least
    # share, 1 / 1024 of 91 grey levels, rounds away; so "lower" is checked on the shares that can show)
    assert (out[valid == 1] == 100).all()
    qx, qy = maps[..., 0].astype(np.int64), maps[..., 1].astype(np.int64)
    x0, y0, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
    w_out = np.zeros(qx.shape, np.int64)
    for dx, dy, w in ((0, 0, (32 - ax) * (32 - ay)), (1, 0, ax * (32 - ay)), (0, 1, (32 - ax) * ay), (1, 1, ax * ay)):
        x, y = x0 + dx, y0 + dy
        w_out += np.where((x < 0) | (x >= 53) | (y < 0) | (y >= 37), w, 0)
    assert np.array_equal(valid == 0, w_out > 0)
    assert np.array_equal(out, ((100 * (1024 - w_out) + 9 * w_out + 512) >> 10).astype(np.uint8))
    assert (out[w_out == 1024] == 9).all() and (w_out == 1024).any() and ((w_out > 0) & (w_out < 1024)).any()


def test_zero_weight_tap_outside_keeps_valid():
    img = R.test_image(37, 53, 1, seed=4)
    maps = np.zeros((2, 3, 2), np.int32)
    maps[0, :, 0] = (52 * 32, 52 * 32 + 1, 51 * 32 + 31)  # the last column exactly, one step past it, one step before it
    maps[0, :, 1] = 36 * 32                               # the last row exactly: the row below weighs nothing
    maps[1, :, 0] = (0, -1, 32 * 7)
    maps[1, :, 1] = (0, 5 * 32, 36 * 32 + 1)
    out, valid = R.rectify_remap(img, maps, border=9)
    assert valid.tolist() == [[1, 0, 1], [1, 0, 0]]
    assert out[0, 0] == img[36, 52] and out[1, 0] == img[0, 0]
    assert out[0, 1] == ((31 * 32 * int(img[36, 52]) + 32 * 9 + 512) >> 10)


def test_rectifiedQ_against_a_hand_computed_case():
    from online_3d_reconstruction_amd import rectifiedQ
    P1 = [[500.0, 0, 320, 0], [0, 500, 240, 0], [0, 0, 1, 0]]
    P2 = [[500.0, 0, 310, -60], [0, 500, 240, 0], [0, 0, 1, 0]]
    # Tx = -60 / 500 = -0.12; -1 / Tx = 25 / 3; (cx1 - cx2) / Tx = 10 / -0.12
    want = np.array([[1, 0, 0, -320], [0, 1, 0, -240], [0, 0, 0, 500], [0, 0, 1.0 / 0.12, 10.0 / -0.12]])
    got = rectifiedQ(P1, P2)
    assert got.shape == (4, 4) and got.dtype == np.float64 and np.array_equal(got, want)
