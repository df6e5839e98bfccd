"""tests/cluster_reference.py against answers known by hand (no GPU): the contract of include/o3dr_objects.h."""
import functools

import numpy as np
import pytest

import cluster_reference as cr

F32 = np.float32


def line(n=600, step=0.25, offset=0.0):
    """n points `step` apart along x at (offset, offset, 0): multiples of 0.25 are exact in fp32, also at 8192 m"""
    xyz = np.zeros((n, 3), F32)
    xyz[:, 0] = F32(offset) + np.arange(n, dtype=F32) * F32(step)
    xyz[:, 1] = F32(offset)
    return xyz


def column(n=300, step=0.5):
    xyz = np.zeros((n, 3), F32)
    xyz[:, 0], xyz[:, 1] = F32(1.25), F32(-3.5)
    xyz[:, 2] = np.arange(n, dtype=F32) * F32(step)
    return xyz


def random_scene():
    rng = np.random.default_rng(1)
    return (rng.random((4096, 3)) * np.array([20.0, 20.0, 2.0])).astype(F32)


@functools.lru_cache(maxsize=None)
def random_result(tolerance, min_size=1, max_size=cr.MAX_SIZE):
    """the reference on the random scene, computed once per parameter set and shared (treat as read-only)"""
    return cr.cluster(random_scene(), tolerance, min_size, max_size)


@pytest.mark.parametrize("offset", [0.0, 8192.0])
def test_a_chain_at_exactly_the_tolerance_is_one_cluster_and_just_below_it_none(offset):
    xyz = line(offset=offset)
    one = cr.cluster(xyz, 0.25)
    assert one.info["n_components"] == 1 and one.info["largest"] == 600 and one.info["n_pairs"] == 599
    assert not one.raw.any() and (one.label == 0).all() and np.array_equal(one.indices, np.arange(600))
    below = float(np.nextafter(F32(0.25), F32(0)))
    each = cr.cluster(xyz, below)
    assert each.info["n_components"] == 600 and each.info["n_pairs"] == 0 and np.array_equal(each.label, np.arange(600))


def test_a_column_of_points_is_linked_through_z_alone():
    assert cr.cluster(column(), 0.5).info["n_components"] == 1
    assert cr.cluster(column(), 0.49).info["n_components"] == 300


def test_a_record_by_hand():
    # cluster 0: points 0, 2, 5; cluster 1: points 1, 3; point 4 alone and rejected by min_size 2
    xyz = np.array([[1.0, 2.0, -0.0], [10.0, 0.0, 0.0], [1.5, 2.0, 0.25], [10.25, 0.0, 0.0], [50.0, 50.0, 50.0], [1.25, 1.5, 0.0]], F32)
    r = cr.cluster(xyz, 0.75, min_size=2)
    assert r.label.tolist() == [0, 1, 0, 1, -1, 0] and r.raw.tolist() == [0, 1, 0, 1, 4, 0] and r.size.tolist() == [3, 2, 3, 2, 1, 3]
    assert r.indices.tolist() == [0, 2, 5, 1, 3]
    a, b = r.clusters
    assert (a["first"], a["size"], a["begin"], a["reserved"]) == (0, 3, 0, 0) and (b["first"], b["size"], b["begin"]) == (1, 2, 3)
    assert a["lo"].tolist() == [1.0, 1.5, 0.0] and a["hi"].tolist() == [1.5, 2.0, 0.25] and not np.signbit(a["lo"][2])
    assert a["centroid"].tolist() == [1.0 + (0.75 / 3.0), 1.5 + (1.0 / 3.0), 0.0 + (0.25 / 3.0)]
    assert b["centroid"].tolist() == [10.125, 0.0, 0.0]
    assert r.info == dict(n_components=3, n_clusters=2, n_too_small=1, n_too_large=0, n_clustered_points=5, n_rejected_points=1,
                          largest=3, n_pairs=4)


def test_duplicates_are_linked_and_an_empty_cloud_has_no_component():
    xyz = np.array([[1, 1, 1], [1, 1, 1], [1, 1, 1], [9, 9, 9]], F32)
    r = cr.cluster(xyz, 1e-3)
    assert r.raw.tolist() == [0, 0, 0, 3] and r.info["n_pairs"] == 3 and r.clusters["centroid"][0].tolist() == [1.0, 1.0, 1.0]
    e = cr.cluster(np.zeros((0, 3), F32), 1.0)
    assert e.info["n_components"] == 0 and e.info["largest"] == 0 and len(e.label) == 0 and len(e.clusters) == 0


def test_the_random_scene():
    r = random_result(0.5)
    assert (r.info["n_components"], r.info["largest"], r.info["n_pairs"]) == (860, 116, 4949)
    assert [random_result(t).info["n_components"] for t in (0.3, 0.4, 0.5)] == [3031, 1983, 860]
    lim = random_result(0.5, 5, 50)
    assert lim.info["n_too_small"] > 0 and lim.info["n_clusters"] > 0 and lim.info["n_too_large"] > 0
    assert lim.info["n_too_small"] + lim.info["n_clusters"] + lim.info["n_too_large"] == 860
    assert lim.info["n_clustered_points"] + lim.info["n_rejected_points"] == 4096
    # the records against the labels, without the reference's own loops
    xyz = random_scene()
    for k in (0, len(lim.clusters) // 2, len(lim.clusters) - 1):
        rec, m = lim.clusters[k], xyz[lim.label == k]
        assert rec["size"] == len(m) and rec["first"] == np.nonzero(lim.label == k)[0][0]
        assert np.array_equal(rec["lo"], m.min(0)) and np.array_equal(rec["hi"], m.max(0))
        assert np.abs(rec["centroid"] - m.astype(np.float64).mean(0)).max() < 2.0 ** -16
    assert np.array_equal(np.diff(lim.clusters["first"]) > 0, np.ones(len(lim.clusters) - 1, bool))


def test_components_agree_with_scipy_where_it_is_installed():
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components
    xyz = random_scene()
    for tol in (0.3, 0.4, 0.5):
        I, J = cr.linked_pairs(xyz, tol)
        g = sp.coo_matrix((np.ones(len(I), np.int8), (I, J)), shape=(len(xyz), len(xyz)))
        k, lab = connected_components(g, directed=False)
        r = random_result(tol)
        assert k == r.info["n_components"]
        first = np.full(k, len(xyz))
        np.minimum.at(first, lab, np.arange(len(xyz)))
        assert np.array_equal(first[lab], r.raw)


# ---- the pair search and the components that scale (cluster(..., pairs="tree")) against the brute force --------------------
BELOW_QUARTER = float(np.nextafter(F32(0.25), F32(0)))


def duplicated_scene():
    """300 points, 100 of them twice more and 50 a fourth time, in random order: pairs at d2 == 0"""
    rng = np.random.default_rng(7)
    base = (rng.random((300, 3)) * 4.0).astype(F32)
    xyz = np.concatenate([base, base[:100], base[:100], base[:50]])
    return xyz[rng.permutation(len(xyz))]


def far_scene():
    """the random scene moved by 8192 m in x and y (fp32 sums: the coordinates keep 2^-10 m)"""
    xyz = random_scene()
    xyz[:, :2] += F32(8192.0)
    return xyz


SCENES = {"random 0.3": (random_scene, 0.3), "random 0.4": (random_scene, 0.4), "random 0.5": (random_scene, 0.5),
          "line at the tolerance": (line, 0.25), "line just below": (line, BELOW_QUARTER), "column": (column, 0.5),
          "column below": (column, 0.49), "duplicates": (duplicated_scene, 1e-3), "duplicates 0.3": (duplicated_scene, 0.3),
          "far 0.4": (far_scene, 0.4)}


def records_by_loop(xyz, r):
    """step 5 of the contract cluster by cluster, as the reference computed it before records() was vectorised"""
    rec = r.clusters.copy()
    for name in ("lo", "hi", "centroid"):
        rec[name] = 0
    for k in range(len(rec)):
        m = xyz[r.indices[rec["begin"][k]:rec["begin"][k] + rec["size"][k]]]
        c = m + F32(0)
        lo, hi = c.min(0), c.max(0)
        q = np.floor((m.astype(np.float64) - lo.astype(np.float64)) * 65536.0 + 0.5).astype(np.int64)
        S = q.sum(0, dtype=np.int64)
        rec["lo"][k], rec["hi"][k] = lo, hi
        rec["centroid"][k] = lo.astype(np.float64) + (S.astype(np.float64) / 65536.0) / np.float64(rec["size"][k])
    return rec


def assert_identical(a, b, what):
    assert sorted(vars(a)) == sorted(vars(b)) == ["clusters", "indices", "info", "label", "raw", "size"]
    for name in ("label", "raw", "size", "indices"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y), (what, name)
    assert a.info == b.info, (what, a.info, b.info)
    assert a.clusters.dtype == b.clusters.dtype == cr.CLUSTER and a.clusters.tobytes() == b.clusters.tobytes(), (what, "records")


@pytest.mark.parametrize("scene", list(SCENES))
def test_the_tree_search_finds_the_pairs_of_the_brute_force(scene):
    make, tolerance = SCENES[scene]
    xyz = make()
    I, J = cr.linked_pairs(xyz, tolerance)
    It, Jt = cr.linked_pairs_tree(xyz, tolerance)
    assert It.dtype == Jt.dtype == np.int64 and (It > Jt).all() and len(np.unique(It * len(xyz) + Jt)) == len(It)
    assert np.array_equal(np.sort(It * len(xyz) + Jt), np.sort(I * len(xyz) + J))
    assert np.array_equal(cr.components_graph(len(xyz), It, Jt), cr.components(len(xyz), I, J))
    if scene.startswith("line"):  # d2 == r2 decides every pair here
        assert len(I) == (599 if tolerance == 0.25 else 0)
    if scene == "duplicates":
        assert len(I) == 50 * 3 + 50 * 6  # a point three / four times: 3 / 6 pairs at distance 0


@pytest.mark.parametrize("limits", [(1, cr.MAX_SIZE), (2, 50)])
@pytest.mark.parametrize("scene", list(SCENES))
def test_the_tree_cluster_is_the_brute_force_cluster_and_the_records_are_the_loops(scene, limits):
    make, tolerance = SCENES[scene]
    xyz = make()
    brute = random_result(tolerance, *limits) if make is random_scene else cr.cluster(xyz, tolerance, *limits)
    assert_identical(cr.cluster(xyz, tolerance, *limits, pairs="tree"), brute, scene)
    assert brute.clusters.tobytes() == records_by_loop(xyz, brute).tobytes(), scene
    if limits == (2, 50) and scene in ("random 0.5", "duplicates 0.3", "far 0.4"):
        assert brute.info["n_too_small"] > 0 and brute.info["n_clusters"] > 0 and brute.info["n_rejected_points"] > 0


def test_the_tree_search_on_an_empty_cloud_and_a_single_point():
    for n in (0, 1):
        xyz = np.full((n, 3), 2.5, F32)
        assert_identical(cr.cluster(xyz, 0.5, pairs="tree"), cr.cluster(xyz, 0.5), n)
    # the slack of the candidate radius is above the gate's rounding (cluster_reference.tree_radius) at every magnitude
    for tol in (1e-22, 1e-3, 0.1, 1.0, 1e4):
        assert cr.tree_radius(tol) > tol * (1 + 2.0 ** -24) ** 3 + np.sqrt(3.0) * 2.0 ** -75
