"""The robust rigid fit's contract (include/o3dr.h "robust rigid fit") restated in numpy, operation for operation in fp64,
and the robust pose chain on top of tests/pose_chain_reference.py.

hypothesis: the model of three pairs (python floats: every +, -, *, / and sqrt is one rounded IEEE fp64 operation, in the
header's order).  ransac_ref: candidates, the splitmix64 sampler, exact scores, the winner, the mask and the records - and
the smallest relative distance of any (hypothesis, candidate) d^2 from threshold^2, the tests' precondition: above it no
last-bit difference of a d^2 can flip an inlier.  robust_chain_ref: chain_ref with the per-pair filter.  corrupt_world:
wrong 3-D points behind right descriptors."""
import math

import numpy as np

import pose_chain_reference as R

OK, TOO_FEW, NO_MODEL = range(3)
M64 = (1 << 64) - 1


# ---- the contract -------------------------------------------------------------------------------------------------------
def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draws(seed, key, h, m):
    S = splitmix64((int(seed) ^ int(key)) & M64)
    return [(((splitmix64((S + 3 * h + k) & M64) >> 32) * m) >> 32) for k in range(3)]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def frame(p0, p1, p2):
    """-> (e1, e2, e3, centroid), or None: degenerate"""
    p0, p1, p2 = ([float(v) for v in p] for p in (p0, p1, p2))
    u = tuple(p1[k] - p0[k] for k in range(3))
    v = tuple(p2[k] - p0[k] for k in range(3))
    w = _cross(u, v)
    uu, vv, ww = _dot3(u, u), _dot3(v, v), _dot3(w, w)
    c = tuple(((p0[k] + p1[k]) + p2[k]) / 3.0 for k in range(3))
    if ww <= (1e-12 * uu) * vv:
        return None
    lu, lw = math.sqrt(uu), math.sqrt(ww)
    e1 = tuple(x / lu for x in u)
    e3 = tuple(x / lw for x in w)
    e2 = _cross(e3, e1)
    return e1, e2, e3, c


def hypothesis(src3, tgt3):
    """src3, tgt3: three points each (fp32 values) -> T [3, 4] fp64, or None: degenerate"""
    fs, ft = frame(*src3), frame(*tgt3)
    if fs is None or ft is None:
        return None
    T = np.zeros((3, 4))
    for i in range(3):
        for j in range(3):
            T[i, j] = (ft[0][i] * fs[0][j] + ft[1][i] * fs[1][j]) + ft[2][i] * fs[2][j]
        T[i, 3] = ft[3][i] - ((float(T[i, 0]) * fs[3][0] + float(T[i, 1]) * fs[3][1]) + float(T[i, 2]) * fs[3][2])
    return T


def residual2(T, a, b):
    """d^2 of every pair (a, b: [m, 3] fp64) under T, in the contract's order"""
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    d = [(((T[i, 0] * x + T[i, 1] * y) + T[i, 2] * z) + T[i, 3]) - b[:, i] for i in range(3)]
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def ransac_segment(src, tgt, cand, threshold, iterations, seed, key, exact_ok=False):
    """One segment: src, tgt [n, 3] float32, cand [n] bool (mask and finite).  -> (inlier [n] bool, record dict, gap).
    exact_ok: a d^2 that equals threshold^2 exactly is left out of the gap (the caller argues why it is computed exactly)."""
    n = len(src)
    pos = np.nonzero(cand)[0]
    m = len(pos)
    rec = dict(T=np.eye(4)[:3].reshape(12).copy(), n_candidates=m, n_inliers=0, best_hypothesis=-1, sample=[-1, -1, -1],
               status=TOO_FEW if m < 3 else NO_MODEL)
    inl = np.zeros(n, bool)
    gap = np.inf
    if m < 3:
        return inl, rec, gap
    a = src[pos].astype(np.float64)
    b = tgt[pos].astype(np.float64)
    thr2 = float(threshold) * float(threshold)
    best = (0, -1, None, None)
    for h in range(int(iterations)):
        loc = draws(seed, key, h, m)
        score, T = 0, None
        if len(set(loc)) == 3:
            T = hypothesis(src[pos[loc]], tgt[pos[loc]])
        if T is not None:
            d2 = residual2(T, a, b)
            score = int((d2 <= thr2).sum())
            g = np.abs(d2 - thr2) / thr2
            if exact_ok:
                g = g[d2 != thr2]
            if len(g):
                gap = min(gap, float(g.min()))
        if score > best[0]:
            best = (score, h, T, loc)
    if best[0] >= 3:
        score, h, T, loc = best
        inl[pos] = residual2(T, a, b) <= thr2
        rec.update(T=T.reshape(12).copy(), n_inliers=score, best_hypothesis=h, sample=[int(pos[k]) for k in loc], status=OK)
    return inl, rec, gap


def candidates(src, tgt, mask=None):
    c = np.isfinite(src).all(1) & np.isfinite(tgt).all(1)
    return c if mask is None else c & (np.asarray(mask) != 0)


def ransac_ref(src, tgt, threshold, iterations=256, seed=0, seg_offsets=None, mask=None, seg_keys=None, exact_ok=False):
    """-> dict(inlier [n] bool, T [S, 12], n_candidates, n_inliers, best_hypothesis, sample [S, 3], status, gap)"""
    src = np.asarray(src, np.float32).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float32).reshape(-1, 3)
    off = np.array([0, len(src)], np.int64) if seg_offsets is None else np.asarray(seg_offsets, np.int64)
    S = len(off) - 1
    cand = candidates(src, tgt, mask)
    out = dict(inlier=np.zeros(len(src), bool), T=np.zeros((S, 12)), sample=np.zeros((S, 3), np.int32), gap=np.inf)
    for k in ("n_candidates", "n_inliers", "best_hypothesis", "status"):
        out[k] = np.zeros(S, np.int32)
    for s in range(S):
        a0, a1 = int(off[s]), int(off[s + 1])
        key = s if seg_keys is None else int(seg_keys[s])
        inl, rec, gap = ransac_segment(src[a0:a1], tgt[a0:a1], cand[a0:a1], threshold, iterations, seed, key, exact_ok)
        out["inlier"][a0:a1] = inl
        out["gap"] = min(out["gap"], gap)
        for k, v in rec.items():
            out[k][s] = v
    return out


# ---- the robust chain -----------------------------------------------------------------------------------------------------
def pair_key(i, j):
    return (int(i) << 32) | int(j)


def robust_chain_ref(desc, offsets, kp3, prior, n_fixed=0, poses_in=None, status_in=None, dist_nearby=2.0, range_width=8,
                     min_matches=30, max_rms=np.inf, ratio=0.5, max_distance=40, nudge=0, ransac_threshold=None,
                     ransac_iterations=256, ransac_seed=0, static=None):
    """chain_ref of pose_chain_reference.py with the per-pair RANSAC filter (ransac_threshold None: chain_ref itself, plus
    the empty extras).  Extra keys: ransac (one record dict per pair of the list), inlier {(i, j): bool per query row},
    n_dropped [F] (slots the filter alone dropped), gap, match {(i, j): (idx, good)} of every pair.  static: an earlier
    result for the same inputs and parameters but another nudge - the matching and the filter work in camera coordinates
    and do not depend on the poses, so they are taken from it."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 32)
    off = np.asarray(offsets, np.int64)
    xyz = np.asarray(kp3, np.float32).reshape(-1, 3)
    prior = np.asarray(prior, np.float32).reshape(-1, 16)
    F = len(off) - 1
    pairs = R.pair_list(prior, dist_nearby, range_width, n_fixed)
    # static: matching and the filter of every pair, in camera coordinates
    match, inlier, rrec, gap = {}, {}, [], np.inf
    if static is not None:
        assert static["pairs"] == pairs
        match, inlier, rrec, gap = static["match"], static["inlier"], static["ransac"], static["gap"]
    for (i, j) in (pairs if static is None else []):
        idx, dist = R.knn2_ref(desc[off[i]:off[i + 1]], desc[off[j]:off[j + 1]])
        good = R.good_ref(dist, ratio, max_distance)
        match[(i, j)] = (idx, good)
        if ransac_threshold is not None:
            s = xyz[off[i]:off[i + 1]]
            t = np.full_like(s, np.nan)
            t[good] = xyz[off[j]:off[j + 1]][idx[good, 0].astype(np.int64)]
            inl, rec, g = ransac_segment(s, t, candidates(s, t, good), ransac_threshold, ransac_iterations, ransac_seed, pair_key(i, j))
            inlier[(i, j)] = inl
            rrec.append(rec)
            gap = min(gap, g)
    poses = prior.copy()
    r = dict(status=np.zeros(F, np.int32), n_pairs=np.zeros(F, np.int32), n_pairs_accepted=np.zeros(F, np.int32),
             n_good=np.zeros(F, np.int32), n_used=np.zeros(F, np.int32), rms=np.zeros(F), T=np.zeros((F, 12)), pairs=pairs,
             gathered={}, ransac=rrec, inlier=inlier, n_dropped=np.zeros(F, np.int32), gap=gap, match=match)
    for f in range(n_fixed):
        poses[f] = np.asarray(poses_in, np.float32).reshape(-1, 16)[f]
        r["status"][f] = status_in[f]
    for i in range(n_fixed, F):
        mine = [j for (q, j) in pairs if q == i]
        r["n_pairs"][i] = len(mine)
        if not mine:
            r["status"][i] = R.ANCHOR
            continue
        q3 = xyz[off[i]:off[i + 1]]
        src, tgt = [], []
        for j in mine:
            if r["status"][j] > R.MATCHED:
                continue
            r["n_pairs_accepted"][i] += 1
            idx, good = match[(i, j)]
            r["n_good"][i] += int(good.sum())
            rows = np.nonzero(good)[0]
            s = q3[rows]
            t = R.a2(poses[j], xyz[off[j]:off[j + 1]][idx[rows, 0].astype(np.int64)])
            use = np.isfinite(s).all(1) & np.isfinite(t).all(1)
            if ransac_threshold is not None:
                keep = use & inlier[(i, j)][rows]
                r["n_dropped"][i] += int(use.sum() - keep.sum())
                use = keep
            src.append(s[use])
            tgt.append(t[use])
        src = np.concatenate(src) if src else np.zeros((0, 3), np.float32)
        tgt = np.concatenate(tgt) if tgt else np.zeros((0, 3), np.float32)
        r["n_used"][i] = len(src)
        r["gathered"][i] = (src, tgt)
        if len(src) < min_matches:
            r["status"][i] = R.TOO_FEW
            continue
        T = R.kabsch_rank_ref(src, tgt)
        if T is None:
            r["status"][i] = R.DEGENERATE
            continue
        e = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3] - tgt.astype(np.float64)
        rms = float(np.sqrt((e * e).sum() / len(src)))
        r["rms"][i] = rms
        if not rms <= max_rms:
            r["status"][i] = R.RMS
            continue
        r["status"][i] = R.MATCHED
        r["T"][i] = T[:3].reshape(12)
        p = T.astype(np.float32).reshape(16)
        if nudge:
            p[:12] = np.nextafter(p[:12], np.float32(np.inf if nudge > 0 else -np.inf))
        p[12:] = (0, 0, 0, 1)
        poses[i] = p
    for i in range(F):
        if r["status"][i] != R.MATCHED or i < n_fixed:
            r["T"][i] = poses[i, :12].astype(np.float64)
    r["poses"] = poses
    return r


def assert_ransac_equal(rr, ref):
    """the library's per-pair RANSAC records against robust_chain_ref's: integers exactly, T within 1e-9"""
    assert len(rr) == len(ref["ransac"])
    for k, want in enumerate(ref["ransac"]):
        for f in ("n_candidates", "n_inliers", "best_hypothesis", "status"):
            assert rr[f][k] == want[f], (k, f)
        assert rr["sample"][k].tolist() == want["sample"], k
        assert np.abs(rr["T"][k] - want["T"]).max() <= 1e-9, k


# ---- the corrupted world --------------------------------------------------------------------------------------------------
def corrupt_world(world, share, seed, lo=0.5, hi=3.0):
    """make_world's output with the kp3 of `share` of the rows (chosen per frame) replaced by a point lo .. hi metres away, in
    a random direction: the descriptor match stays right, the 3-D point is wrong.  -> a new dict with `corrupted` [N] bool."""
    rng = np.random.default_rng(seed)
    w = dict(world)
    kp3 = np.array(world["kp3"], np.float32)
    off = world["offsets"]
    bad = np.zeros(len(kp3), bool)
    for f in range(len(off) - 1):
        n = int(off[f + 1] - off[f])
        rows = int(off[f]) + rng.choice(n, int(round(share * n)), replace=False)
        d = rng.normal(size=(len(rows), 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        kp3[rows] = (kp3[rows].astype(np.float64) + d * rng.uniform(lo, hi, (len(rows), 1))).astype(np.float32)
        bad[rows] = True
    w["kp3"], w["corrupted"] = kp3, bad
    return w
