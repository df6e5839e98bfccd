"""The rigid core (DESIGN.md "Rigid core": rigid_moments, rigid_residual2, wave_fields / tree4, fold_partials, rigid_solve,
draw3) through the operators that share it, bit for bit against tests/rigid_core_reference.py: estimateRigidTransform over
every segment size at which the partition or the fold takes another path (262 145 points: the first size at which a thread
of the fold takes two partials), the pose chain's device-side solve against the host's, one ICP step, and the samplers of
ransacRigid and segmentPlane.  Inputs are built so that the matching is known; every reference is computed once."""
import numpy as np
import pytest

import pose_chain_reference as R
import rigid_core_reference as rc

pytestmark = pytest.mark.gpu

I12 = np.eye(4)[:3].reshape(12)
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1024, 262144, 262145]
_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _motion(seed, angle=0.3):
    rng = np.random.default_rng(seed)
    T = np.eye(4)
    T[:3, :3] = R.rot(rng.normal(size=3), angle)
    T[:3, 3] = rng.uniform(-1, 1, 3)
    return T


def _same(a, b):
    return np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes()


def _expected(src, tgt, used, fold, threads):
    """(n_used, ok, T [12] - the identity without a solve -, rms) of one fit as the library reports it"""
    fit = rc.rigid_fit(src, tgt, used, fold, threads)
    T = fit["T"] if fit["ok"] else I12
    fin = np.asarray(used, bool) & rc.pair_finite(src, tgt)
    return fit["n_used"], fit["ok"], T, rc.residual_rms(T, src, tgt, fin, fit["n_used"], fold, threads)


# ---- 1. estimateRigidTransform: the segment sizes ------------------------------------------------------------------------
def _segments():
    rng = np.random.default_rng(5)
    off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(off[-1])
    src = rng.uniform(-4, 4, (n, 3)).astype(np.float32)
    tgt = np.empty_like(src)
    for k in range(len(SIZES)):
        T = _motion(100 + k)
        s = src[off[k]:off[k + 1]].astype(np.float64)
        tgt[off[k]:off[k + 1]] = (s @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 0.01, s.shape)).astype(np.float32)
    mask = (rng.random(n) > 1.0 / 3.0).astype(np.uint8)
    mask[off[2]:off[3]] = 1          # the three-point segment keeps its solve
    mask[off[5]] = 0                 # the first row of two segments: c0 is then not the segment's first tgt
    mask[off[10]] = 0
    src[off[5] + 7, 1] = np.nan      # NaN in three rows, all with mask 1
    tgt[off[10] + 100000, 0] = np.nan
    tgt[off[11] + 1, 2] = np.nan
    for r in (off[5] + 7, off[10] + 100000, off[11] + 1):
        mask[r] = 1
    return src, tgt, mask, off


def test_segment_sizes_against_the_reference_and_single_calls(ctx):
    src, tgt, mask, off = _memo("segments", _segments)
    res = ctx.estimateRigidTransform(R.points(src), R.points(tgt), seg_offsets=off, mask=mask)
    assert len(res) == len(SIZES)
    assert abs(float(mask.mean()) - 2.0 / 3.0) < 0.01
    for k, n in enumerate(SIZES):
        s, t, m = src[off[k]:off[k + 1]], tgt[off[k]:off[k + 1]], mask[off[k]:off[k + 1]]
        n_used, ok, T, rms = _expected(s, t, m != 0, rc.fold_strided, rc.RUN)
        assert res[k].n_used == n_used == int(((m != 0) & rc.pair_finite(s, t)).sum()), n
        assert (res[k].status == 0) == ok and ok == (n_used >= 3), n
        assert _same(res[k].T[:3], T), (n, res[k].T, T)
        assert _same(res[k].rms, rms), (n, res[k].rms, rms)
        one = ctx.estimateRigidTransform(R.points(s), R.points(t), mask=m)
        assert _same(one.T, res[k].T) and _same(one.rms, res[k].rms) and (one.n_used, one.status) == (res[k].n_used, res[k].status), n


# ---- 2. the pose chain: the device-side solve ------------------------------------------------------------------------------
def _two_frames(n, gaps):
    """Frame 0 (the train frame, an anchor at the identity) and frame 1 with n rows each: query row r carries train row
    perm[r]'s descriptor, so the best match is perm[r] at distance 0.  gaps: every fifth query row has a descriptor of its
    own (not good), two keypoints are NaN and four matched rows are a metre off (the RANSAC's outliers)."""
    rng = np.random.default_rng([n, int(gaps)])
    dt = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    perm = rng.permutation(n)
    dq = dt[perm].copy()
    kt = np.stack([rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(3, 9, n)], 1).astype(np.float32)
    T = _motion(7 + n, 0.1)
    inv = np.linalg.inv(T)
    kq = (kt[perm].astype(np.float64) @ inv[:3, :3].T + inv[:3, 3] + rng.normal(0, 0.003, (n, 3))).astype(np.float32)
    good = np.ones(n, bool)
    if gaps:
        bad = np.arange(0, n, 5)
        dq[bad] = rng.integers(0, 256, (len(bad), 32), dtype=np.uint8)
        good[bad] = False
        kq[1 % n, 0] = np.nan
        kt[perm[2 % n], 2] = np.nan
        if n >= 64:
            kq[[11, 23, 36, 47]] += np.float32(1.0)
    prior = np.tile(np.eye(4, dtype=np.float32).reshape(16), (2, 1))
    return dict(desc=np.concatenate([dt, dq]), offsets=np.array([0, n, 2 * n], np.int64), kp3=np.concatenate([kt, kq]), prior=prior,
                src=kq, tgt=kt[perm], good=good)


@pytest.mark.parametrize("gaps", [False, True])
@pytest.mark.parametrize("robust", [False, True])
def test_pose_chain_solve_equals_the_reference_and_the_host_solve(ctx, robust, gaps):
    for n in (3, 64, 65, 256, 257, 1100):
        w = _memo(("frames", n, gaps), lambda: _two_frames(n, gaps))
        kw = dict(min_matches=3, ransac_threshold=0.05, ransac_seed=3, return_ransac=True) if robust else dict(min_matches=3)
        out = ctx.poseChain(w["desc"], w["offsets"], R.points(w["kp3"]), w["prior"], **kw)
        rec = out[1]
        src, tgt, used = w["src"], w["tgt"], w["good"] & rc.pair_finite(w["src"], w["tgt"])
        assert rec["status"][0] == R.ANCHOR and rec["n_pairs"][1] == 1 and rec["n_good"][1] == w["good"].sum(), n
        if robust:  # the pair's mask from its record: the candidates within the threshold of the winning model
            rr = out[2][0]
            assert rr["n_candidates"] == used.sum(), n
            thr = np.float64(0.05)
            inl = used & (rc.residual_field(rr["T"], src, tgt, used)[:, 0] <= thr * thr) & (rr["status"] == 0)
            assert rr["n_inliers"] == (inl.sum() if rr["status"] == 0 else 0), n
            if gaps and n >= 64:
                assert rr["status"] == 0 and not inl[[11, 23, 36, 47]].any() and inl.sum() >= used.sum() - 8, n
            used = inl
        n_used, ok, T, rms = _expected(src, tgt, used, rc.fold_chain, rc.CHAIN_THREADS)
        assert rec["n_used"][1] == n_used, n
        if n_used < 3:
            assert rec["status"][1] == R.TOO_FEW, n
            continue
        assert ok and rec["status"][1] == R.MATCHED, n
        assert _same(rec["T"][1], T), (n, rec["T"][1], T)
        assert _same(rec["rms"][1], rms), (n, rec["rms"][1], rms)
        if n <= 256:  # one run: the host solves the same record (the device solve against the host solve)
            fit = ctx.estimateRigidTransform(R.points(src), R.points(tgt), mask=used.astype(np.uint8))
            assert fit.n_used == n_used and _same(fit.T[:3], rec["T"][1]) and _same(fit.rms, rec["rms"][1]), n


# ---- 3. one ICP step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [257, 262145])
def test_one_icp_step_equals_the_reference(ctx, n):
    """target: a lattice of one-metre cells; source point i: lattice point perm[i] moved by less than 0.2 m per axis, so its
    nearest neighbour is that point"""
    rng = np.random.default_rng(n)
    side = int(np.ceil(np.sqrt(n))) + 1
    gx, gy = np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64))
    tgt = np.stack([gx.ravel(), gy.ravel(), rng.uniform(0, 0.3, side * side)], 1).astype(np.float32)
    perm = rng.permutation(len(tgt))[:n]
    src = (tgt[perm].astype(np.float64) + (0.1, -0.05, 0.02) + rng.uniform(-0.1, 0.1, (n, 3))).astype(np.float32)
    idx, _d2 = ctx.nearestNeighbors(R.points(src), R.points(tgt))
    assert np.array_equal(idx.astype(np.int64), perm)
    res = ctx.icpAlign(R.points(src), R.points(tgt), max_iterations=1)
    assert res.iterations == 1 and res.n_correspondences == n
    lo, hi = tgt.min(0).astype(np.float64), tgt.max(0).astype(np.float64)
    c0 = (lo + hi) * 0.5
    rec = rc.fold_strided(rc.run_partials(rc.moment_fields(src, tgt[perm], np.ones(n, bool), c0)))
    ok, T = rc.rigid_solve(rec, c0)
    assert ok and _same(res.T[:3], T), (res.T, T)
    assert _same(res.T[3], [0.0, 0.0, 0.0, 1.0])


# ---- 4. the sampler ------------------------------------------------------------------------------------------------------------
def test_ransac_rigid_and_segment_plane_draw_the_reference_indices(ctx):
    rng = np.random.default_rng(7)
    m = 200
    src = rng.uniform(-2, 2, (m, 3)).astype(np.float32)
    T = _motion(1)
    tgt = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    _inl, rr = ctx.ransacRigid(R.points(src), R.points(tgt), 0.05, iterations=64, seed=7)
    assert rr["status"][0] == 0 and rr["n_candidates"][0] == m
    h = int(rr["best_hypothesis"][0])
    assert rr["sample"][0].tolist() == rc.draw3(7, 0, h, m)  # (every row is a candidate: position = rank = local index)
    flat = np.stack([rng.uniform(-2, 2, m), rng.uniform(-2, 2, m), rng.normal(0, 0.002, m)], 1).astype(np.float32)
    _mask, tiles = ctx.segmentPlane(R.points(flat), 0.01, max_iterations=64, tile_size=0.0, seed=7)
    assert len(tiles) == 1 and tiles["status"][0] == 0 and (tiles["ix"][0], tiles["iy"][0]) == (0, 0)
    hp = int(tiles["hypothesis"][0])
    assert tiles["sample"][0].tolist() == rc.draw3(7, 0, hp, m)
    assert len({tuple(rc.draw3(7, 0, k, m)) for k in range(64)}) > 60  # (the hypotheses do differ: equality means something)
