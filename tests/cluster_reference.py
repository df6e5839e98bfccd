"""The contract of o3dr_cluster_euclidean (include/o3dr_objects.h) restated in numpy, operation for operation: the fp32
link gate over all pairs, the components of its closure, the clusters numbered by lowest index, PCL's PointIndices, one
record per cluster with an exact centroid, and the counters.  The default pair search is brute force, meant for clouds of
a few thousand points; cluster(..., pairs="tree") finds the same pairs through a KD-tree and the same components through
scipy's graph search, for clouds of the map's size."""
from types import SimpleNamespace

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

F32 = np.float32
CLUSTER = np.dtype([("first", np.int32), ("size", np.int32), ("begin", np.int32), ("reserved", np.int32),
                    ("lo", np.float32, (3,)), ("hi", np.float32, (3,)), ("centroid", np.float64, (3,))])
MAX_SIZE = 2 ** 31 - 1
ROWS = 512


def r2_of(tolerance):
    return F32(np.float64(tolerance) * np.float64(tolerance))


def linked_pairs(xyz, tolerance):
    """step 1 -> (I, J) int64 with I > J: every linked pair once; d2 in fp32, in row chunks"""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    n, r2 = len(xyz), r2_of(tolerance)
    col = np.arange(n)
    I, J = [], []
    for s in range(0, n, ROWS):
        q = xyz[s:s + ROWS]
        dx = q[:, None, 0] - xyz[None, :, 0]
        dy = q[:, None, 1] - xyz[None, :, 1]
        dz = q[:, None, 2] - xyz[None, :, 2]
        d2 = ((F32(0) + dx * dx) + dy * dy) + dz * dz
        assert d2.dtype == F32
        i, j = np.nonzero((d2 <= r2) & (col[None, :] < (s + np.arange(len(q)))[:, None]))
        I.append(i + s)
        J.append(j)
    if not I:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(I).astype(np.int64), np.concatenate(J).astype(np.int64)


def tree_radius(tolerance):
    """a radius no pair the fp32 gate accepts can exceed in exact arithmetic.  With u = 2^-24: each difference is rounded
    once, each square once, and the first term passes through two sums, so the fp32 d2 is at least d2 / (1 + u)^5 less
    3 * 2^-150 (three squares that may underflow); r2 <= tolerance^2 (1 + u).  An accepted pair therefore has
    d <= tolerance (1 + u)^3 + sqrt(3) 2^-75 < tolerance (1 + 2e-7) + 2^-74.  The factor used is 1 + 1e-5, fifty times
    that, which also covers the tree's own fp64 rounding (about 1e-15 relative); every candidate is re-checked in fp32."""
    return float(tolerance) * (1.0 + 1e-5) + 2.0 ** -74


def linked_pairs_tree(xyz, tolerance):
    """step 1 as linked_pairs gives it (the same set of pairs, I > J, in another order): candidates from a KD-tree in fp64
    at tree_radius(tolerance), each one decided by linked_pairs' own fp32 expression"""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    r2 = r2_of(tolerance)
    if len(xyz) < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    cand = cKDTree(xyz.astype(np.float64)).query_pairs(tree_radius(tolerance), output_type="ndarray").reshape(-1, 2)
    J, I = cand[:, 0].astype(np.int64), cand[:, 1].astype(np.int64)  # query_pairs returns i < j
    assert (I > J).all()
    dx, dy, dz = xyz[I, 0] - xyz[J, 0], xyz[I, 1] - xyz[J, 1], xyz[I, 2] - xyz[J, 2]
    d2 = ((F32(0) + dx * dx) + dy * dy) + dz * dz
    assert d2.dtype == F32
    keep = d2 <= r2
    return I[keep], J[keep]


def components(n, I, J):
    """step 2 -> raw [n]: the lowest index of every point's component (minimum-label propagation with pointer jumping)"""
    raw = np.arange(n, dtype=np.int64)
    while True:
        m = np.minimum(raw[I], raw[J])
        new = raw.copy()
        np.minimum.at(new, I, m)
        np.minimum.at(new, J, m)
        new = new[new]
        if np.array_equal(new, raw):
            return raw
        raw = new


def components_graph(n, I, J):
    """step 2 as components gives it: scipy's connected components, each named by its lowest index"""
    g = coo_matrix((np.ones(len(I), np.int8), (I, J)), shape=(n, n))
    k, lab = connected_components(g, directed=False)
    first = np.unique(lab, return_index=True)[1]        # the first occurrence of every component number: its lowest index
    assert len(first) == k
    return first[lab].astype(np.int64)


def records(xyz, indices, firsts, sizes):
    """step 5 -> CLUSTER [K]: per cluster the box, and the centroid as lo + (the int64 sum of the offsets from lo,
    quantised to 2^-16) / 2^16 / size; `indices` holds the clusters one after another"""
    rec = np.zeros(len(firsts), CLUSTER)
    rec["first"], rec["size"] = firsts, sizes
    rec["begin"] = np.cumsum(sizes) - sizes
    if not len(firsts):
        return rec
    begin = rec["begin"].astype(np.int64)
    m = xyz[indices]
    c = m + F32(0)
    lo, hi = np.minimum.reduceat(c, begin, axis=0), np.maximum.reduceat(c, begin, axis=0)
    q = np.floor((m.astype(np.float64) - np.repeat(lo, sizes, axis=0).astype(np.float64)) * 65536.0 + 0.5).astype(np.int64)
    S = np.add.reduceat(q, begin, axis=0, dtype=np.int64)
    rec["lo"], rec["hi"] = lo, hi
    rec["centroid"] = lo.astype(np.float64) + (S.astype(np.float64) / 65536.0) / rec["size"].astype(np.float64)[:, None]
    return rec


def cluster(xyz, tolerance, min_size=1, max_size=MAX_SIZE, pairs="brute"):
    """-> label, raw, size (int32 [n]), indices (int32), clusters (CLUSTER [K]), info (dict of the result's counters).
    pairs: "brute" (linked_pairs, components) or "tree" (linked_pairs_tree, components_graph); the result is the same"""
    assert pairs in ("brute", "tree")
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    n = len(xyz)
    assert np.isfinite(xyz).all() and 1 <= min_size <= max_size and tolerance > 0 and np.isfinite(r2_of(tolerance)) and r2_of(tolerance) > 0
    if n:
        assert ((xyz.max(0).astype(np.float64) - xyz.min(0).astype(np.float64)) < 32768.0).all()
    I, J = (linked_pairs_tree if pairs == "tree" else linked_pairs)(xyz, tolerance)
    raw = (components_graph if pairs == "tree" else components)(n, I, J)
    counts = np.bincount(raw, minlength=n)
    size = counts[raw]
    roots = np.nonzero(counts)[0]                       # ascending raw
    kept = (counts[roots] >= min_size) & (counts[roots] <= max_size)
    firsts = roots[kept]                                # step 3: numbered in ascending raw
    number = np.full(n, -1, np.int64)
    number[firsts] = np.arange(len(firsts))
    label = number[raw] if n else number
    clustered = np.nonzero(label >= 0)[0]
    indices = clustered[np.argsort(label[clustered], kind="stable")]  # step 4
    rec = records(xyz, indices, firsts, counts[firsts])  # step 5
    sizes = counts[roots]
    info = dict(n_components=len(roots), n_clusters=len(firsts), n_too_small=int((sizes < min_size).sum()),
                n_too_large=int((sizes > max_size).sum()), n_clustered_points=len(clustered), n_rejected_points=n - len(clustered),
                largest=int(sizes.max()) if n else 0, n_pairs=len(I))
    return SimpleNamespace(label=label.astype(np.int32), raw=raw.astype(np.int32), size=size.astype(np.int32),
                           indices=indices.astype(np.int32), clusters=rec, info=info)
