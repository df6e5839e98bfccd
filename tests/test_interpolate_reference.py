"""tests/interpolate_reference.py against answers known by hand (no GPU): the contract of include/o3dr_dem.h."""
import numpy as np
import pytest

import interpolate_reference as R

F32 = np.float32
NAN = np.nan


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@pytest.mark.parametrize("smooth", [0, 1, 2, 8])
@pytest.mark.parametrize("shape,at", [((1, 1), (0, 0)), ((5, 3), (0, 0)), ((5, 3), (4, 2)), ((7, 1), (3, 0)), ((33, 65), (17, 40))])
def test_one_data_cell_gives_its_bits_everywhere(shape, at, smooth):
    """the pull is c m / c, the push 16 a / 16, a sweep k a / k: all exact"""
    W, H = shape
    for value in (F32(-3.7251), F32(1e30), F32(-0.0), F32(1e-41)):
        Z = np.full((H, W), NAN, F32)
        Z[at[1], at[0]] = value
        filled, lev, info = R.interpolate(Z, smooth)
        want = bits(np.full((H, W), value, F32))
        if value == 0:  # 0.0 + (-0.0) = +0.0: the sums lose the sign of a zero, the data cell keeps its bits
            want[:] = 0
            want[at[1], at[0]] = 0x80000000
        assert np.array_equal(bits(filled), want)
        assert info["n_data"] == 1 and info["n_filled"] == W * H - 1 and info["n_empty"] == 0
        assert info["n_levels"] == len(R.level_shapes(W, H)) and sum(info["n_by_level"]) == W * H


def test_level_of_a_single_corner_cell():
    W, H = 5, 3
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    Z = np.full((H, W), NAN, F32)
    Z[0, 0] = 1
    _, lev, info = R.interpolate(Z)
    want = np.maximum(np.maximum(np.ceil(np.log2(x + 1)), np.ceil(np.log2(y + 1))), 1).astype(np.uint8)  # the bit length of max(x, y)
    want[0, 0] = 0
    assert np.array_equal(lev, want) and lev.max() == 3 and info["n_levels"] == 4
    assert info["n_by_level"][:4] == [1, 3, 8, 3]
    Z = np.full((H, W), NAN, F32)
    Z[2, 4] = 1  # (4, 2): alone under its level-1 cell (2, 1); the level-2 cell (1, 0) covers x 4..7, y 0..3
    _, lev, _ = R.interpolate(Z)
    assert lev.tolist() == [[3, 3, 3, 3, 2], [3, 3, 3, 3, 2], [3, 3, 3, 3, 0]]


def test_a_raster_without_holes_returns_its_own_bits():
    rng = np.random.default_rng(3)
    Z = rng.normal(size=(37, 21)).astype(F32)
    Z[0, :4] = [-0.0, 1e-42, 1e30, -1e30]
    for smooth in (0, 2):
        filled, lev, info = R.interpolate(Z, smooth)
        assert np.array_equal(bits(filled), bits(Z)) and not lev.any()
        assert (info["n_data"], info["n_filled"], info["n_empty"]) == (Z.size, 0, 0) and info["n_by_level"][0] == Z.size


def test_an_all_nan_raster():
    Z = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF, 0xFF800123, 0x7FC00000], np.uint32).view(F32).reshape(2, 3)
    filled, lev, info = R.interpolate(Z)
    assert (bits(filled) == R.NAN_BITS).all() and (lev == 255).all()
    assert (info["n_data"], info["n_filled"], info["n_empty"]) == (0, 0, 6) and not any(info["n_by_level"])


def test_two_by_two_by_hand():
    """m_1 = (1 + 2 + 6) / 3 = 3; the hole is 16 * 3 / 16 = 3, and after a sweep (up 1 + right 6) / 2 = 3.5"""
    Z = np.array([[1, 2], [NAN, 6]], F32)
    c, m = R.pull(Z)
    assert c[1].tolist() == [[3]] and m[1].tolist() == [[3.0]]
    assert R.interpolate(Z, 0)[0].tolist() == [[1, 2], [3, 6]]
    for smooth in (1, 2, 8):
        assert R.interpolate(Z, smooth)[0].tolist() == [[1, 2], [3.5, 6]]
    assert R.interpolate(Z)[1].tolist() == [[0, 0], [1, 0]]


def test_three_by_one_by_hand():
    """W 3 -> 2 -> 1.  Level 1 is (2, 10), both data; the hole at x = 1 has X = 0, Xn = 1 and one row of parents:
    (9 * 2 + 3 * 10 + 3 * 2 + 10) / 16 = 4; a sweep gives (2 + 10) / 2 = 6"""
    Z = np.array([[2, NAN, 10]], F32)
    c, m = R.pull(Z)
    assert [v.tolist() for v in c] == [[[1, 0, 1]], [[1, 1]], [[2]]] and m[1].tolist() == [[2, 10]] and m[2].tolist() == [[6]]
    assert R.interpolate(Z, 0)[0].tolist() == [[2, 4, 10]]
    assert R.interpolate(Z, 1)[0].tolist() == [[2, 6, 10]]
    filled, lev, info = R.interpolate(Z, 2)
    assert filled.tolist() == [[2, 6, 10]] and lev.tolist() == [[0, 1, 0]] and info["n_levels"] == 3
    # the column form: the same numbers
    assert R.interpolate(Z.T.copy(), 0)[0].tolist() == [[2], [4], [10]]


@pytest.mark.parametrize("smooth", [0, 2, 8])
def test_outputs_lie_within_the_data_range(smooth):
    """every value is a weighted mean with non-negative weights, rounded monotonically"""
    rng = np.random.default_rng(5)
    Z = (rng.normal(size=(70, 131)) * 50).astype(F32)
    Z[rng.random(Z.shape) < 0.9] = NAN
    Z[20:60, 30:110] = NAN
    filled, _, info = R.interpolate(Z, smooth)
    assert info["n_empty"] == 0 and not np.isnan(filled).any()
    assert filled.min() >= np.nanmin(Z) and filled.max() <= np.nanmax(Z)


def test_max_level_only_masks():
    rng = np.random.default_rng(6)
    Z = rng.normal(size=(40, 50)).astype(F32)
    Z[rng.random(Z.shape) < 0.6] = NAN
    Z[5:30, 10:45] = NAN
    full, lev, info = R.interpolate(Z, 2)
    assert lev.max() >= 4
    for M in (1, 3):
        got, lev_m, info_m = R.interpolate(Z, 2, max_level=M)
        masked = lev > M
        assert masked.any() and np.array_equal(lev_m, lev) and info_m["n_by_level"] == info["n_by_level"]
        assert (bits(got)[masked] == R.NAN_BITS).all() and np.array_equal(bits(got)[~masked], bits(full)[~masked])
        assert info_m["n_empty"] == masked.sum() and info_m["n_filled"] == info["n_filled"] - masked.sum()


def test_sample_by_hand():
    raster = np.array([[1, NAN, 3], [4, 5, 6]], F32)
    xyz = np.array([[0.05, 0.05, 10], [0.15, 0.05, 10], [0.29, 0.19, 10], [-0.01, 0.0, 10], [0.3, 0.0, 10], [0.0, 0.2, 10]], F32)
    value, above, counts = R.sample(xyz, raster, 0.1, (0, 0, 3, 2))
    assert bits(value).tolist() == bits(np.array([1, NAN, 6, NAN, NAN, NAN], F32)).tolist()
    assert bits(above).tolist() == bits(np.array([9, NAN, 4, NAN, NAN, NAN], F32)).tolist()
    assert counts == (3, 3, 1)


def test_quality_scene():
    """300 x 420 undulating terrain, 0.02 noise, 14 rectangular holes of 10..89 cells a side (25 % holes with this
    generator): the RMS error inside the holes against the noise-free surface.  Measured with this reference: nearest
    cell 0.382, smooth = 2 0.169 (pull-push alone 0.226, smooth = 1 0.175, smooth = 8 0.175); with 30 % of the cells
    removed at random in addition (48 % holes): nearest 0.280, smooth = 2 0.124, pull-push alone 0.166.  The bound is
    0.75 of the nearest-cell fill's, the margin of tests/test_multiview_fuse_reference.py: it catches a broken pyramid."""
    Z, truth, hole = R.quality_scene()
    assert 0.15 < hole.mean() < 0.35
    filled, _, info = R.interpolate(Z, 2)
    assert info["n_empty"] == 0 and np.array_equal(bits(filled)[~hole], bits(Z)[~hole])
    ours = R.rms_in_holes(filled, truth, hole)
    plain = R.rms_in_holes(R.interpolate(Z, 0)[0], truth, hole)
    print(f"rms in holes: smooth 2 {ours:.4f}, pull-push alone {plain:.4f}")
    assert ours < plain  # the sweeps help
    try:
        import scipy  # noqa: F401
    except ImportError:
        return  # (the comparison with the nearest-cell fill needs scipy's distance transform)
    nearest = R.rms_in_holes(R.nearest_fill(Z), truth, hole)
    print(f"rms in holes: nearest cell {nearest:.4f}, ratio {ours / nearest:.3f}")
    assert ours < 0.75 * nearest
