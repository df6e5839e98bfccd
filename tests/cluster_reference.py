"""The contract of o3dr_cluster_euclidean (include/o3dr_objects.h) restated in numpy, operation for operation: the fp32
link gate over all pairs, the components of its closure, the clusters numbered by lowest index, PCL's PointIndices, one
record per cluster with an exact centroid, and the counters.  Brute force: meant for clouds of a few thousand points."""
from types import SimpleNamespace

import numpy as np

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


def cluster(xyz, tolerance, min_size=1, max_size=MAX_SIZE):
    """-> label, raw, size (int32 [n]), indices (int32), clusters (CLUSTER [K]), info (dict of the result's counters)"""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    n = len(xyz)
    assert np.isfinite(xyz).all() and 1 <= min_size <= max_size and tolerance > 0 and np.isfinite(r2_of(tolerance)) and r2_of(tolerance) > 0
    if n:
        assert ((xyz.max(0).astype(np.float64) - xyz.min(0).astype(np.float64)) < 32768.0).all()
    I, J = linked_pairs(xyz, tolerance)
    raw = components(n, I, J)
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
    rec = np.zeros(len(firsts), CLUSTER)
    rec["first"], rec["size"] = firsts, counts[firsts]
    rec["begin"] = np.cumsum(counts[firsts]) - counts[firsts]
    for k in range(len(firsts)):                        # step 5
        c = xyz[indices[rec["begin"][k]:rec["begin"][k] + rec["size"][k]]] + F32(0)
        lo, hi = c.min(0), c.max(0)
        m = xyz[indices[rec["begin"][k]:rec["begin"][k] + rec["size"][k]]]
        q = np.floor((m.astype(np.float64) - lo.astype(np.float64)) * 65536.0 + 0.5).astype(np.int64)
        S = q.sum(0, dtype=np.int64)
        rec["lo"][k], rec["hi"][k] = lo, hi
        rec["centroid"][k] = lo.astype(np.float64) + (S.astype(np.float64) / 65536.0) / np.float64(rec["size"][k])
    sizes = counts[roots]
    info = dict(n_components=len(roots), n_clusters=len(firsts), n_too_small=int((sizes < min_size).sum()),
                n_too_large=int((sizes > max_size).sum()), n_clustered_points=len(clustered), n_rejected_points=n - len(clustered),
                largest=int(sizes.max()) if n else 0, n_pairs=len(I))
    return SimpleNamespace(label=label.astype(np.int32), raw=raw.astype(np.int32), size=size.astype(np.int32),
                           indices=indices.astype(np.int32), clusters=rec, info=info)
