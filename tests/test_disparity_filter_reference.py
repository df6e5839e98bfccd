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


# ---- the inputs of tests/test_labelling_scale.py -------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(255, 1023), (67, 131)], ids=["255x1023", "67x131"])
@pytest.mark.parametrize("name", ["maze", "spiral"])
def test_maze_and_spiral_are_one_component(name, H, W):
    img = R.maze(H, W, 1) if name == "maze" else R.spiral(H, W)
    assert img.shape == (H, W) and img.dtype == np.uint8 and len(np.unique(img)) == 2 and img[0, 0] != 0
    n_valid = int((img != 0).sum())
    if name == "maze":  # the cells and one opened wall per edge of their spanning tree
        assert n_valid == 2 * ((H + 1) // 2) * ((W + 1) // 2) - 1
        assert (img[0::2, 0::2] != 0).all() and not img[1::2, 1::2].any()
    else:               # one pixel wide: no 2 x 2 block of the arm, and every pixel but the two ends has two neighbours
        v = np.pad(img != 0, 1)
        assert not (v[:-1, :-1] & v[1:, :-1] & v[:-1, 1:] & v[1:, 1:]).any()
        nb = (v[:-2, 1:-1].astype(int) + v[2:, 1:-1] + v[1:-1, :-2] + v[1:-1, 2:])[v[1:-1, 1:-1]]
        assert sorted(np.unique(nb).tolist()) == [1, 2] and (nb == 1).sum() == 2 and n_valid > H * W // 2 - 2 * (H + W)
    _, labels, sizes, info = R.filter_disparity(img, max_speckle_size=100)
    assert info.n_components == 1 and info.largest == n_valid and info.n_valid == n_valid and info.n_removed == 0
    assert (labels[img != 0] == 0).all() and (labels[img == 0] == -1).all() and (sizes[img != 0] == n_valid).all()


@pytest.mark.parametrize("H,W", [(255, 1023), (67, 131)], ids=["255x1023", "67x131"])
@pytest.mark.parametrize("name", ["maze", "spiral"])
def test_maze_and_spiral_cross_every_tile_border(name, H, W):
    """serpentine has one valid pair per horizontal tile border and comb one per vertical one; these two cross every border
    of either kind, at 255 x 1023 with at least 500 pairs of each kind (67 x 131 has 134 and 524 pairs in all)"""
    img = R.maze(H, W, 1) if name == "maze" else R.spiral(H, W)
    vert, horz = R.border_pairs(img)
    assert len(vert) == (W - 1) // 64 and len(horz) == (H - 1) // 16 and vert.min() >= 1 and horz.min() >= 1
    print(f"{name} {H}x{W}: {int(vert.sum())} pairs across vertical tile borders, {int(horz.sum())} across horizontal ones")
    if (H, W) == (255, 1023):
        assert vert.sum() >= 500 and horz.sum() >= 500
        assert R.border_pairs(R.serpentine(H, W))[1].sum() == 15 and R.border_pairs(R.comb(H, W))[0].sum() == 15


def csgraph_partition(joined_right, joined_down, valid):
    """labels and sizes as R.components gives them, by scipy's connected components of the graph of the joined 4-neighbour
    pairs (joined_right [H, W - 1]: pixel (y, x) with (y, x + 1); joined_down [H - 1, W]: with (y + 1, x))"""
    sparse = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    H, W = valid.shape
    idx = np.arange(H * W).reshape(H, W)
    a = np.concatenate([idx[:, :-1][joined_right], idx[:-1][joined_down]])
    b = np.concatenate([idx[:, 1:][joined_right], idx[1:][joined_down]])
    graph = sparse.coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(H * W, H * W))
    n, comp = csgraph.connected_components(graph, directed=False)
    lowest = np.full(n, H * W, np.int64)
    np.minimum.at(lowest, comp, np.arange(H * W))
    labels = np.where(valid.ravel(), lowest[comp], -1).astype(np.int32)
    sizes = np.where(valid.ravel(), np.bincount(comp, minlength=n)[comp], 0).astype(np.int32)
    return labels.reshape(H, W), sizes.reshape(H, W)


SCALE_PARTITIONS = [("maze", 1), ("spiral", 1), ("levels uint8", 0), ("levels uint8", 1), ("levels uint16", 0), ("levels uint16", 20000)]


@pytest.mark.parametrize("name,max_diff", SCALE_PARTITIONS, ids=[f"{n} max_diff {d}" for n, d in SCALE_PARTITIONS])
def test_components_equal_csgraph_at_255x1023(name, max_diff):
    import labelling_scale_cases as X
    img = X.df_input(name, 255, 1023)
    v = img.astype(np.int64)
    ok = v != 0
    right = ok[:, :-1] & ok[:, 1:] & (np.abs(v[:, :-1] - v[:, 1:]) <= max_diff)
    down = ok[:-1] & ok[1:] & (np.abs(v[:-1] - v[1:]) <= max_diff)
    labels, sizes = csgraph_partition(right, down, ok)
    got = R.components(img, max_diff)
    assert got[0].dtype == labels.dtype and got[1].dtype == sizes.dtype
    assert np.array_equal(got[0], labels) and np.array_equal(got[1], sizes)
    assert sizes.max() > 20 and (labels[ok].max() == 0) == (name in ("maze", "spiral"))
