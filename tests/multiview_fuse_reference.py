"""The multi-view fusion contract (include/o3dr.h "multi-view fusion") in numpy, operation for operation.  Steps 1 to 4 are
the filter's and come from multiview_reference; steps 5 and 6 - the vote of every supporting neighbour and their ordered
sum - are restated here: every product is rounded before it is added, the divisions are true divisions (numpy's
elementwise ufuncs never fuse)."""
from collections import namedtuple

import numpy as np

from multiview_reference import SUPPORT, classify, homographies, levels, multiview_filter

FuseInfo = namedtuple("FuseInfo", "filter n_votes n_votes_dropped n_fused")


def votes_of(disp, i, j, H, tolerance):
    """the test of every pixel of frame i against frame j through H -> (is a SUPPORT, the level v it votes for, is a vote);
    v is meaningful where the first holds"""
    cls = classify(disp, i, j, H, tolerance)
    lv_i, _ = levels(disp[i])
    lv_j, _ = levels(disp[j])
    rows, cols = lv_i.shape
    x = np.arange(cols, dtype=np.float64)[None, :] + np.zeros((rows, 1))
    y = np.arange(rows, dtype=np.float64)[:, None] + np.zeros((1, cols))
    is_sup = cls == SUPPORT
    with np.errstate(all="ignore"):
        # the pixel of frame j the test read (step 3's own operations; a SUPPORT is inside)
        h = [((H[r][0] * x + H[r][1] * y) + H[r][2] * lv_i) + H[r][3] for r in range(4)]
        xr, yr = np.floor(h[0] / h[3] + 0.5), np.floor(h[1] / h[3] + 0.5)
        xi = np.where(is_sup, xr, 0).astype(np.int64)
        yi = np.where(is_sup, yr, 0).astype(np.int64)
        e = lv_j[yi, xi]
        # step 5
        a2 = (H[2][0] * x + H[2][1] * y) + H[2][3]
        a3 = (H[3][0] * x + H[3][1] * y) + H[3][3]
        num = e * a3 - a2
        den = H[2][2] - e * H[3][2]
        v = num / den
        is_vote = is_sup & (v > 0) & np.isfinite(v)
    return is_sup, v, is_vote


def multiview_fuse(disp, Q, poses, neighbors, tolerance=1.0, min_support=1, max_violations=-1):
    """[F, rows, cols] -> out (float64 levels), votes (uint8), support (uint8), violations (uint8), the list of FuseInfo"""
    disp = np.asarray(disp)
    F = disp.shape[0]
    neighbors = np.asarray(neighbors, np.int32).reshape(F, -1)
    filtered, support, violations, finfos = multiview_filter(disp, Q, poses, neighbors, tolerance, min_support, max_violations)
    H = homographies(Q, poses, neighbors)
    out = np.zeros(disp.shape, np.float64)
    votes = np.zeros(disp.shape, np.uint8)
    infos = []
    for i in range(F):
        lv, valid = levels(disp[i])
        acc = np.where(valid, lv, 0.0)
        n_votes = n_dropped = 0
        for n in range(neighbors.shape[1]):
            j = int(neighbors[i, n])
            if j < 0:
                continue
            is_sup, v, is_vote = votes_of(disp, i, j, H[i, n], tolerance)
            is_sup, is_vote = is_sup & valid, is_vote & valid
            with np.errstate(all="ignore"):
                acc = np.where(is_vote, acc + v, acc)
            votes[i] += is_vote.astype(np.uint8)
            n_votes += int(is_vote.sum())
            n_dropped += int((is_sup & ~is_vote).sum())
        s, w = support[i].astype(np.int64), violations[i].astype(np.int64)
        keep = valid & (s >= min_support) & ((w < s) if max_violations < 0 else (w <= max_violations))
        with np.errstate(all="ignore"):
            fused = acc / (1 + votes[i]).astype(np.float64)
        out[i] = np.where(keep, fused, 0.0)
        infos.append(FuseInfo(finfos[i], n_votes, n_dropped, int((keep & (votes[i] > 0)).sum())))
    return out, votes, support, violations, infos
