"""Pins tests/segment_reference.py, the numpy statement of the segmentation contract (include/o3dr.h "image segmentation"):
the structure of its result, the tie-breaks on hand-worked cases, the fallback chain, and its accuracy on an image whose
regions are known."""
import numpy as np
import pytest

import segment_reference as R


def first_pixels(labels):
    flat = labels.reshape(-1).astype(np.int64)
    first = np.full(int(flat.max()) + 1, flat.size, np.int64)
    np.minimum.at(first, flat, np.arange(flat.size))
    return first


def check_structure(img, res, S, min_size):
    labels, sizes, info = res["labels"].astype(np.int64), res["sizes"], res["info"]
    H, W = labels.shape
    n = info["n_labels"]
    # 0..n-1 by ascending first pixel
    assert sorted(np.unique(labels).tolist()) == list(range(n))
    assert (np.diff(first_pixels(labels)) > 0).all() and labels[0, 0] == 0
    # every label is 4-connected: as many components of equal labels as labels
    assert len(np.unique(R.components(labels))) == n
    # sizes and info add up
    cnt = np.bincount(labels.reshape(-1))
    assert np.array_equal(sizes, cnt[labels]) and cnt.sum() == H * W
    assert info["n_centres"] == -(-W // S) * -(-H // S)
    assert info["n_components"] == len(np.unique(R.components(res["raw"])))
    assert info["n_components"] - info["n_merged"] == n
    assert info["largest"] == cnt.max() and info["smallest"] == cnt.min()
    # a label below min_size holds pixel 0, or touches no not-small component: then every component is small
    root = R.components(res["raw"])
    comp_size = np.bincount(root.reshape(-1), minlength=H * W)
    for l in np.nonzero(cnt < min_size)[0]:
        assert l == 0 or (comp_size[np.unique(root)] < min_size).all()
    if (comp_size[np.unique(root)] < min_size).all() and min_size > 0:
        assert n == 1


@pytest.mark.parametrize("S,m,K,min_size", [(8, 20, 5, None), (4, 0, 1, 0), (8, 20, 0, 10000), (16, 10, 3, 7), (5, 20, 2, None)])
@pytest.mark.parametrize("channels", [1, 3])
def test_structure(S, m, K, min_size, channels):
    img = R.random_image(45, 70, channels, seed=3)
    res = R.segment(img, S, m, K, min_size)
    check_structure(img, res, S, R.default_min_size(S) if min_size is None else min_size)
    assert res["labels"].dtype == np.uint32 and res["raw"].dtype == np.int32 and res["sizes"].dtype == np.int32


def test_components_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    for img in (R.serpentine(21, 30), R.comb(21, 30), R.random_image(30, 41, 1, 5) // 64):
        root = R.components(img.astype(np.int64))
        n = 0
        for v in np.unique(img):
            lab, k = ndimage.label(img == v)
            for i in range(1, k + 1):
                sel = lab == i
                assert (root[sel] == np.flatnonzero(sel.reshape(-1))[0]).all()
            n += k
        assert len(np.unique(root)) == n


def test_hand_worked_assignment_ties():
    img = np.full((1, 8), 50, np.uint8)  # nx = 2: centres at x = 2 and x = 6
    # m = 0 on one colour: every D is 0, the lowest k wins everywhere
    assert R.raw_labels(img, 4, 0, 0)[0].tolist() == [[0] * 8]
    # m = 1: D = (x - xk)^2; x = 4 is 2 away from both centres and goes to the lower one
    raw, c = R.raw_labels(img, 4, 1, 1)
    assert raw.tolist() == [[0, 0, 0, 0, 0, 1, 1, 1]]
    # the update: x of centre 0 = (2 * 10 + 5) / 10 = 2, of centre 1 = (2 * 18 + 3) / 6 = 6 (6.5 floored)
    assert c[:, 0].tolist() == [2, 6] and c[:, 2:].tolist() == [[50] * 3] * 2
    # negative control: ties to the highest k give another image
    assert R.raw_labels(img, 4, 1, 1, highest_k_wins=True)[0].tolist() == [[0, 0, 0, 0, 1, 1, 1, 1]]
    # min_size 0 keeps both; the default 4 merges the component of 3 into its only neighbour
    assert R.segment(img, 4, 1, 1, 0)["labels"].tolist() == [[0, 0, 0, 0, 0, 1, 1, 1]]
    res = R.segment(img, 4, 1, 1)
    assert res["labels"].tolist() == [[0] * 8] and res["info"]["n_merged"] == 1 and res["sizes"].tolist() == [[8] * 8]


def test_hand_worked_merge_ties():
    lab = np.array([[0, 0, 0, 1, 2, 2, 2]], np.int64)
    root = R.components(lab)
    assert root.tolist() == [[0, 0, 0, 3, 4, 4, 4]]
    c = np.zeros((3, 5), np.int64)
    c[:, 2:] = [[10] * 3, [20] * 3, [30] * 3]  # the middle component is as far from the left as from the right: 300
    assert R.merge(root, lab, c, 2)[0].tolist() == [[0, 0, 0, 0, 1, 1, 1]]  # the lower first pixel wins
    c[2, 2:] = [29, 30, 30]                     # the right one is nearer now: 281
    assert R.merge(root, lab, c, 2)[0].tolist() == [[0, 0, 0, 1, 1, 1, 1]]
    # a small component that touches only small ones goes left; the not-small one further right does not count
    lab = np.array([[0, 1, 2, 2, 2]], np.int64)
    c[:, 2:] = [[10] * 3, [200] * 3, [201] * 3]
    labels, sizes, n_comp, n_merged, n_labels = R.merge(R.components(lab), lab, c, 2)
    # component 1 touches the not-small 2 and joins it; component 0 touches only the small 1, holds pixel 0 and stays
    assert labels.tolist() == [[0, 1, 1, 1, 1]] and (n_comp, n_merged, n_labels) == (3, 1, 2) and sizes.tolist() == [[1, 4, 4, 4, 4]]


def test_checkerboard_fallback_chain():
    img = R.checkerboard(19, 23)
    # an odd step puts neighbouring seeds on either colour: at m = 0 a pixel takes the lowest centre of its own colour
    res = R.segment(img, 5, 0, 1, 10000)
    # every pixel is its own component, none touches a not-small one: the chain runs left and up to pixel 0
    assert res["info"]["n_components"] == 19 * 23 and res["info"]["n_labels"] == 1 and res["info"]["n_merged"] == 19 * 23 - 1
    assert (res["labels"] == 0).all() and (res["sizes"] == 19 * 23).all()
    assert R.segment(img, 5, 0, 1, 0)["info"]["n_labels"] == 19 * 23
    # negative control of the tie-break on a full-size image
    const = R.constant_image(19, 23)
    assert not np.array_equal(R.raw_labels(const, 4, 0, 0)[0], R.raw_labels(const, 4, 0, 0, highest_k_wins=True)[0])


@pytest.mark.parametrize("S,m", [(8, 20), (16, 20)])
def test_accuracy_on_known_regions(S, m):
    img, region, disp, true = R.region_image()
    assert img.shape == (64, 96, 3)
    res = R.segment(img, S, m)
    check_structure(img, res, S, R.default_min_size(S))
    labels = res["labels"].astype(np.int64)
    # pixels outside their label's majority region
    table = np.zeros((labels.max() + 1, 4), np.int64)
    np.add.at(table, (labels.reshape(-1), region.reshape(-1)), 1)
    outside = int((table.sum(axis=1) - table.max(axis=1)).sum())
    print(f"S={S} m={m}: {outside} pixels outside their label's majority region, {res['info']}")
    assert outside <= 0.01 * labels.size
    # a plane per label brings the disparity's error against the true planes below half of the raw image's
    raw_rms = float(np.sqrt(np.mean((disp.astype(np.float64) - true) ** 2)))
    fit_rms = R.plane_fit_rms(labels, disp, true)
    print(f"S={S} m={m}: plane-fit RMS {fit_rms:.3f} against raw {raw_rms:.3f}")
    assert fit_rms < 0.5 * raw_rms


def _scale_cases():
    import labelling_scale_cases as X
    return X.SEG_CASES


@pytest.mark.parametrize("case", _scale_cases(), ids=lambda c: f"{c[0]} {c[1]}x{c[2]} S {c[3]} K {c[5]}")
def test_components_equal_csgraph_on_the_scale_cases(case):
    """the raw labels of every segmentation tests/test_labelling_scale.py asks for: R.components against scipy's connected
    components of the graph of equal-label 4-neighbour pairs, the root being the lowest index of the component"""
    import labelling_scale_cases as X
    from test_disparity_filter_reference import csgraph_partition
    raw = X.seg_reference(*case)[1].astype(np.int64)
    labels, sizes = csgraph_partition(raw[:, :-1] == raw[:, 1:], raw[:-1] == raw[1:], np.ones(raw.shape, bool))
    root = R.components(raw)
    assert np.array_equal(root, labels)
    assert np.array_equal(np.bincount(root.ravel(), minlength=raw.size)[root], sizes)
    assert X.seg_reference(*case)[3][0]["n_components"] == len(np.unique(labels))
