"""tests/merge_reference.py (the torch restatement of the voxel grid and the merge that the full-size GPU tests compare
libo3dr with) against the C oracle, on CPU tensors: bit for bit, at the shapes and edges where the restatement could go wrong.
A negative control shows that bit equality pins the summation order, and the exact means are checked against fp64."""
from fractions import Fraction

import numpy as np
import pytest
import torch
from hypothesis import given, settings
from hypothesis import strategies as st

import merge_reference as mr
from conftest import assert_points_equal, random_cloud
from test_properties_hypothesis import SETTINGS, clouds


def _same(ref, want, what):
    pts, status = want
    assert ref.status == status, what
    assert_points_equal(ref.points, pts, what)
    if status == 0:
        assert ref.counts.sum() <= 10 ** 12 and np.all(np.diff(ref.idx) > 0), what


def _alpha(pts, seed):
    pts["rgba"] = np.random.default_rng(seed).integers(0, 1 << 32, len(pts), dtype=np.uint64).astype(np.uint32)
    return pts


@pytest.mark.parametrize("leaf", [0.05, 0.1, 0.37, (0.02, 0.3, 1.7)])
@pytest.mark.parametrize("minpts", [0, 1, 2, 3, 4])
def test_voxel_grid_random_clouds(orc, leaf, minpts):
    pts = random_cloud(60_000, 3, extent=(4.0, 3.0, 2.0))
    leaf = np.broadcast_to(np.asarray(leaf, np.float32), 3)
    ref = mr.voxel_grid(pts, leaf, minpts)
    _same(ref, orc.voxel_grid(pts, leaf, minpts), f"leaf {leaf} min_points {minpts}")
    if ref.status == 0:
        assert ref.counts.min() >= max(minpts, 1)


@pytest.mark.parametrize("origin", [(-9.0, -7.0, -5.0), (-1.5, -2.0, -0.5), (-1e3, 250.0, -3.0)])
def test_negative_and_mixed_sign_coordinates(orc, origin):
    pts = random_cloud(50_000, 4, extent=(3.0, 4.0, 1.0), origin=origin)
    for leaf, minpts in ((0.05, 0), (0.25, 3)):
        _same(mr.voxel_grid(pts, (leaf,) * 3, minpts), orc.voxel_grid(pts, (leaf,) * 3, minpts), f"{origin} leaf {leaf}")
    _same(mr.downsample_pt_cloud(pts, 0.05, True, 2), orc.downsample_pt_cloud(pts, 0.05, True, 2), f"{origin} combined")


def test_heavy_cell_and_single_cell_cloud(orc):
    heavy = random_cloud(30_000, 5)
    heavy[:2500]["x"] = np.float32(5.01) + np.float32(1e-3) * np.arange(2500, dtype=np.float32) % np.float32(0.03)
    heavy[:2500]["y"], heavy[:2500]["z"] = np.float32(-1.02), np.float32(0.51)
    ref = mr.voxel_grid(heavy, (0.05,) * 3, 1)
    _same(ref, orc.voxel_grid(heavy, (0.05,) * 3, 1), "a cell of more than 2000 points")
    assert ref.counts.max() >= 2500
    one = random_cloud(5000, 6, extent=(0.04, 0.04, 0.04), origin=(1.003, -2.047, 0.301))
    ref = mr.voxel_grid(one, (0.05,) * 3, 0)
    _same(ref, orc.voxel_grid(one, (0.05,) * 3, 0), "one cell")
    assert len(ref.points) == 1 and ref.counts[0] == 5000
    _same(mr.downsample_pt_cloud(one, 0.05, True, 5000), orc.downsample_pt_cloud(one, 0.05, True, 5000), "one cell, combined")
    _same(mr.voxel_grid(one, (0.05,) * 3, 5001), orc.voxel_grid(one, (0.05,) * 3, 5001), "one cell below min_points")


def test_overflow_fallback_and_the_edge_of_the_guard(orc):
    pts = random_cloud(20_000, 7)
    ref = mr.voxel_grid(pts, (1e-4,) * 3, 2)
    assert ref.status == orc.STATUS_VOXEL_OVERFLOW
    _same(ref, orc.voxel_grid(pts, (1e-4,) * 3, 2), "overflow fallback")
    _same(mr.downsample_pt_cloud(pts, 1e-4, True, 3), orc.downsample_pt_cloud(pts, 1e-4, True, 3), "combined overflow (z +- 500)")
    # integer box, leaf 1: dx*dy*dz = 1290^3 = 2 146 689 000 passes, 1291 * 1290^2 = 2 148 353 100 trips the guard
    sides = set()
    for ext, want in ((1289.0, 0), (1290.0, mr.STATUS_VOXEL_OVERFLOW)):
        box = random_cloud(4000, 8, extent=(1289.0, 1289.0, 1289.0), origin=(-600.0, 10.0, -1000.0))
        box[0]["x"], box[1]["x"] = np.float32(-600.0), np.float32(-600.0 + ext)
        box[0]["y"], box[1]["y"], box[0]["z"], box[1]["z"] = np.float32(10.0), np.float32(1299.0), np.float32(-1000.0), np.float32(289.0)
        ref = mr.voxel_grid(box, (1.0, 1.0, 1.0), 0)
        assert ref.status == want
        _same(ref, orc.voxel_grid(box, (1.0, 1.0, 1.0), 0), f"box {ext} at the guard's edge")
    # fp32 leaves walking the guard across a random cloud: both sides, same side as the oracle each time
    cloud = random_cloud(30_000, 9, extent=(8.0, 6.0, 3.0))
    for leaf in np.linspace(0.00400, 0.00412, 13, dtype=np.float32):
        ref = mr.voxel_grid(cloud, (leaf,) * 3, 0)
        sides.add(ref.status)
        _same(ref, orc.voxel_grid(cloud, (leaf,) * 3, 0), f"leaf {leaf} at the guard's edge")
    assert sides == {0, mr.STATUS_VOXEL_OVERFLOW}


@pytest.mark.parametrize("vs,minpts", [(0.05, 1), (0.05, 3), (0.2, 2), (0.013, 0)])
def test_combined_merge_with_alpha(orc, vs, minpts):
    pts = _alpha(random_cloud(80_000, 10, extent=(3.0, 2.0, 30.0), origin=(-1.0, -1.0, -12.0)), 11)
    for combined in (True, False):
        ref = mr.downsample_pt_cloud(pts, vs, combined, minpts)
        _same(ref, orc.downsample_pt_cloud(pts, vs, combined, minpts), f"vs {vs} combined {combined}")
        assert ref.status or (ref.points["rgba"] >> 24).max() > 0


def test_empty_input(orc):
    empty = np.zeros(0, mr.POINT)
    for ref in (mr.voxel_grid(empty, (0.05,) * 3, 0), mr.downsample_pt_cloud(empty, 0.05, True, 1),
                mr.voxel_grid(torch.zeros((0, 4), dtype=torch.int32), (0.05,) * 3, 3)):
        assert len(ref.points) == 0 and ref.status == 0
    out, status = orc.downsample_pt_cloud(empty, 0.05, True, 1)
    assert len(out) == 0 and status == 0


def test_torch_rows_input_equals_numpy_input(orc):
    pts = random_cloud(10_000, 12)
    rows = torch.from_numpy(pts.view(np.int32).reshape(-1, 4).copy())
    a, b = mr.downsample_pt_cloud(rows, 0.1, True, 2), mr.downsample_pt_cloud(pts, 0.1, True, 2)
    assert_points_equal(a.points, b.points, "[N, 4] int32 tensor vs POINT array")
    assert np.array_equal(a.counts, b.counts) and np.array_equal(a.exact, b.exact)


def test_colour_sums_past_fp32_exactness_raise():
    pts = random_cloud(70_000, 13, extent=(0.01, 0.01, 0.01))
    with pytest.raises(ValueError, match="order-dependent"):
        mr.voxel_grid(pts, (0.05,) * 3, 0)


@settings(**SETTINGS)
@given(clouds(), st.integers(0, 4), st.booleans())
def test_hypothesis_clouds_bit_equal_to_the_oracle(orc, cloud, minpts, combined):
    pts, leaf = cloud
    if combined:
        _same(mr.downsample_pt_cloud(pts, leaf, True, minpts), orc.downsample_pt_cloud(pts, leaf, True, minpts), "combined")
    else:
        _same(mr.voxel_grid(pts, (leaf,) * 3, minpts), orc.voxel_grid(pts, (leaf,) * 3, minpts), "voxel grid")


def _reverse_inside_cells(pts, leaf, every=2):
    """the same multiset of points per cell, the points of every other cell in reversed input order"""
    from oracle import orc
    keys, _, _, st_ = orc.voxel_keys(pts, leaf)
    assert st_ == 0
    order = np.argsort(keys, kind="stable")
    heads = np.flatnonzero(np.r_[True, keys[order][1:] != keys[order][:-1]])
    out = pts.copy()
    for c, (a, b) in enumerate(zip(heads, np.r_[heads[1:], len(pts)])):
        if c % every == 0 and b - a > 2:
            pos = order[a:b]
            out[pos] = pts[pos[::-1]]
    return out


def test_negative_control_summation_order_is_pinned(orc):
    """reversing the points inside some cells keeps every cell's multiset: the oracle on the original input and the
    reference on the reversed one agree in occupancy, order and colours, but NOT in every bit - bit equality above is a
    statement about the summation order, not only about the cells"""
    pts = random_cloud(400_000, 14, extent=(2.0, 2.0, 1.0))
    vs = np.float32(0.05)
    rev = _reverse_inside_cells(pts, (vs,) * 3)
    want, _ = orc.voxel_grid(pts, (vs,) * 3, 0)
    got = mr.voxel_grid(rev, (vs,) * 3, 0)
    assert len(got.points) == len(want) and np.array_equal(got.points["rgba"], want["rgba"])
    differ = (got.points.view(np.uint32).reshape(-1, 4) != want.view(np.uint32).reshape(-1, 4)).any(axis=1)
    assert differ.sum() > 0
    assert_points_equal(got.points, orc.voxel_grid(rev, (vs,) * 3, 0)[0], "reversed cells, both sides on the same input")


def test_exact_means_are_the_correctly_rounded_fp64_truth(orc):
    """the exact means are never further from the fp64 mean than the fp32 result of either summation order, and every
    fp32 order stays inside error_bound"""
    pts = random_cloud(600_000, 15, extent=(1.0, 1.0, 5.0), origin=(-0.5, 3.0, -2.0))
    ref = mr.downsample_pt_cloud(pts, 0.05, True, 1)
    assert ref.exact_sum.all() and ref.counts.min() >= 1
    # the fp64 truth of z is the mean of z' = fp32(z + 500), shifted by 500 in exact arithmetic
    z1 = (pts["z"] + np.float32(500)).astype(np.float64)
    keys, _, _, _ = orc.voxel_keys(np.rec.fromarrays([pts["x"], pts["y"], pts["z"] + np.float32(500), pts["rgba"]], dtype=mr.POINT),
                                   (np.float32(0.05), np.float32(0.05), np.float32(1000)))
    _, inv = np.unique(keys, return_inverse=True)
    n = np.bincount(inv).astype(np.float64)
    truth = np.stack([np.bincount(inv, pts["x"].astype(np.float64)) / n, np.bincount(inv, pts["y"].astype(np.float64)) / n,
                      np.bincount(inv, z1) / n - 500.0], axis=1)
    assert np.array_equal(n, ref.counts)
    bound = mr.error_bound(ref)
    for order in (orc.ORDER_STABLE, orc.ORDER_STDSORT):
        res, _ = orc.downsample_pt_cloud(pts, 0.05, True, 1, order)
        for a, ax in enumerate("xyz"):
            r = res[ax].astype(np.float64)
            assert np.all(np.abs(ref.exact[:, a] - truth[:, a]) <= np.abs(r - truth[:, a])), (order, ax)
            assert np.all(np.abs(r - ref.exact[:, a]) <= bound[:, a]), (order, ax)
    # x and y: within half an ulp of the truth (the fp64 sums are exact: correctly rounded)
    for a in range(2):
        assert np.all(np.abs(ref.exact[:, a] - truth[:, a]) <= np.spacing(np.abs(ref.exact[:, a])).astype(np.float64) / 2)


def test_round_f32_settles_double_rounding_ties_exactly():
    # s / n whose fp64 quotient is an fp32 midpoint while the true quotient is not
    s = np.array([float(1 + 2 ** -24 + 2 ** -60) * 3, 3.0 * (1 + 2 ** -24)])
    n = np.array([3, 3])
    r = mr._round_f32(s, n)
    for i in range(2):
        true = Fraction(float(s[i])) / 3
        cands = [np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2))]
        best = min(cands, key=lambda c: (abs(Fraction(float(c)) - true), int(np.float32(c).view(np.uint32)) & 1))
        assert r[i] == best, (i, r[i], best)
