"""Pins tests/disparity_filter_reference.py, the numpy statement of the disparity-filter contract (include/o3dr.h "disparity
filter"), on inputs whose result is known by construction, and against scipy where scipy is installed."""
import numpy as np
import pytest

import disparity_filter_reference as R


def test_planted_speckles_are_removed_exactly():
    img, clean, counts = R.planted_speckles()
    assert sorted(counts) == [1, 1, 1, 3, 8] and img[47, 95] != 60
    out, labels, sizes, info = R.filter_disparity(img, max_speckle_size=8, max_diff=1)
    assert out.dtype == np.uint8 and np.array_equal(out, clean)
    assert info.n_speckles == 5 and info.n_removed == sum(counts) and info.n_components == 7
    assert info.n_valid == int((img != 0).sum()) and info.largest == int(sizes.max())
    # labels and sizes describe the image before the removal
    assert sorted(np.unique(sizes[(img != 40) & (img != 60) & (img != 0)]).tolist()) == [1, 3, 8]
    assert (labels[img == 0] == -1).all() and (sizes[img == 0] == 0).all() and labels[0, 0] == 0 and labels[0, 48] == 48
    # one pixel more than the limit survives
    out7 = R.filter_disparity(img, max_speckle_size=7, max_diff=1)[0]
    blob8 = img == 100
    assert blob8.sum() == 8 and np.array_equal(out7[blob8], img[blob8]) and np.array_equal(out7[~blob8], clean[~blob8])
    # no removal asked for: the image itself
    assert np.array_equal(R.filter_disparity(img)[0], img)


def test_median_removes_single_pixels_and_leaves_the_2x4_blob():
    img, _, _ = R.planted_speckles()
    out = R.filter_disparity(img, median_size=3)[0]
    assert out[5, 7] == 40 and out[47, 95] == 60 and out[40, 70] == 60 and (out[30, 10:13] == 40).all()
    assert (out[10:12, 61:63] == 100).all()  # the interior of the 2 x 4 blob: six of its nine window values are the blob's
    # an isolated hole goes like an isolated wrong pixel: zero is a value like any other
    hole = np.full((9, 9), 33, np.uint8)
    hole[4, 4] = 0
    assert (R.median(hole, 3) == 33).all() and (R.median(hole, 5) == 33).all()
    assert np.array_equal(R.median(img, 0), img)


def test_serpentine_is_one_component():
    img = R.serpentine(67, 131)
    _, labels, sizes, info = R.filter_disparity(img, max_speckle_size=100)
    assert info.n_components == 1 and info.largest == 4487 and info.n_valid == 4487 and info.n_removed == 0
    assert (labels[img != 0] == 0).all() and (sizes[img != 0] == 4487).all()


def test_comb_joined_by_its_last_row():
    img = R.comb(40, 70)
    _, labels, sizes, info = R.filter_disparity(img)
    assert info.n_components == 1 and labels[0, 68] == 0 and labels[0, 69] == -1 and sizes[0, 68] == info.n_valid


def test_ramp_threshold():
    img = R.ramp()
    assert img.dtype == np.uint16
    assert R.filter_disparity(img, max_diff=3)[3].n_components == 1
    info = R.filter_disparity(img, max_diff=2)[3]
    assert info.n_components == 100 and info.largest == 3
    wide = np.array([[1, 65535]], np.uint16)  # the difference is taken in a type that holds it
    assert R.filter_disparity(wide, max_diff=65534)[3].n_components == 1
    assert R.filter_disparity(wide, max_diff=65533)[3].n_components == 2


def test_partition_equals_scipy_label():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(11)
    img = (rng.randint(0, 100, (67, 131)) * (rng.rand(67, 131) < 0.55)).astype(np.uint16)
    _, labels, sizes, _ = R.filter_disparity(img, max_diff=65535)
    ref, n = ndi.label(img != 0)  # (the default structure is the 4-neighbourhood)
    assert n > 10
    # the same partition: each reference component carries exactly one label, and distinct ones carry distinct labels
    first = np.full(n + 1, -2, np.int64)
    for lab, r in zip(labels.ravel(), ref.ravel()):
        if r:
            assert first[r] in (-2, lab)
            first[r] = lab
    assert len(set(first[1:].tolist())) == n and (labels[ref == 0] == -1).all()
    assert np.array_equal(sizes[ref != 0], np.bincount(ref.ravel())[ref[ref != 0]])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("k", [3, 5])
def test_median_equals_scipy_median_filter(k, dtype):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(k)
    img = rng.randint(0, np.iinfo(dtype).max + 1, (33, 70)).astype(dtype)
    assert np.array_equal(R.median(img, k), ndi.median_filter(img, size=k, mode="nearest"))
