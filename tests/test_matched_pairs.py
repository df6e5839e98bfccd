"""GPU test that holds the three readers of a matching pass - the pose chain (k_pose_chain), the chain form of the RANSAC
(k_ransac_rigid<true>) and the pose graph's moments (k_graph_moments) - to numpy and to one another: each of them looks a
query row up in the matcher's records, mask and the pool's 3-D keypoints, and all must see the same rows.

One pool of four frames with 5, 70, 300 and 1100 rows.  A pair's query frame is the later one, so the frames ascend in
size: the 1100-row frame is then the query of three pairs.  1100 is past the RANSAC's 1024 staged candidates (the pair
against the 300-row frame has more than 1024 candidates, the rest go through the `over` list) and past four runs of 256
slots with a partial last run; 300 crosses one run; 70 is two waves, one partial; 5 is under a wave.

The scene: landmarks with random 256-bit descriptors, a frame's rows are permuted copies with up to 8 flipped bits
(pose_chain_reference.make_world), several query rows may copy one train row.  Rows of landmarks the train frame lacks or
holds twice are unmatched (good = 0).  kp3 is the frame's rigid motion of the landmark, a handful of rows of every frame
have one non-finite coordinate (they meet as query and as train rows) and a handful are gross outliers.  The priors are
0.1 m apart: the chain's pair list is every (i, j < i)."""
import functools

import numpy as np
import pytest

import pose_chain_reference as PC
import ransac_rigid_reference as RR

SIZES = (5, 70, 300, 1100)
THRESHOLD, ITERATIONS, SEED = 0.05, 64, 12345
MIN_MATCHES = 4
BIG = (3, 2)  # the pair with more than RANSAC_STAGE candidates


def views(seed):
    """per frame the landmark of every row: frame 0 holds 0..4; frame 1 these three times and 5..59; frame 2 both groups
    twice and 60..239; frame 3 copies of 60..239 (1076 rows), of 5..59 (10), of 0..4 (10) and 4 landmarks of its own"""
    rng = np.random.default_rng(seed)
    a, b, c = np.arange(0, 5), np.arange(5, 60), np.arange(60, 240)
    v = [a,
         np.concatenate([a, a, a, b]),
         np.concatenate([a, a, b, b, c]),
         np.concatenate([rng.choice(c, 1076), rng.choice(b, 10), rng.choice(a, 10), np.arange(240, 244)])]
    assert tuple(len(x) for x in v) == SIZES
    return [rng.permutation(x) for x in v]


@functools.lru_cache(maxsize=None)
def scene(seed=7):
    w = PC.make_world(seed, views(seed), 244, step=0.1, prior_err=0.01)
    rng = np.random.default_rng([seed, 1])
    kp3 = w["kp3"].copy()
    off = w["offsets"]
    for f, n in enumerate(SIZES):
        rows = off[f] + rng.choice(n, min(8, n // 2), replace=False)  # half of them non-finite, half outliers
        bad, out = rows[:len(rows) // 2], rows[len(rows) // 2:]
        kp3[bad, rng.integers(0, 3, len(bad))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), len(bad))
        kp3[out] += rng.uniform(1.0, 3.0, (len(out), 3)).astype(np.float32)
    w["kp3"] = kp3
    w["points"] = PC.points(kp3)
    w["pairs"] = np.array([(i, j) for i in range(len(SIZES)) for j in range(i - 1, -1, -1)], np.int32)
    return w


def numpy_rows(w, rec, good):
    """per pair of w["pairs"], from the matcher's records and mask and kp3's finiteness alone:
    dict(good, cand (bool per query row), src, tgt (float32 [nq, 3], tgt = the best match's point, row 0's where none))"""
    off, xyz = w["offsets"], w["kp3"]
    out, at = [], 0
    for i, j in w["pairs"]:
        nq, nt = int(off[i + 1] - off[i]), int(off[j + 1] - off[j])
        ti = rec["train_idx"][at:at + nq, 0].astype(np.int64)
        g = np.asarray(good[at:at + nq], bool)
        hit = g & (ti < nt)
        src = xyz[off[i]:off[i + 1]]
        tgt = xyz[off[j]:off[j + 1]][np.where(hit, ti, 0)]
        out.append(dict(good=g, hit=hit, cand=hit & np.isfinite(src).all(1) & np.isfinite(tgt).all(1), src=src, tgt=tgt))
        at += nq
    assert at == len(rec)
    return out


def per_frame(w, per_pair):
    return np.array([sum(int(v) for (i, _), v in zip(w["pairs"], per_pair) if i == f) for f in range(len(SIZES))])


def test_scene_on_the_cpu():
    """(no GPU work: the conditions the GPU test relies on, from the numpy matcher)"""
    w = scene()
    off, desc = w["offsets"], w["desc"]
    recs, goods = [], []
    for i, j in w["pairs"]:
        idx, dist = PC.knn2_ref(desc[off[i]:off[i + 1]], desc[off[j]:off[j + 1]])
        r = np.zeros(len(idx), [("train_idx", "<u4", (2,)), ("distance", "<u4", (2,))])
        r["train_idx"], r["distance"] = idx, dist
        recs.append(r)
        goods.append(PC.good_ref(dist))
    rows = numpy_rows(w, np.concatenate(recs), np.concatenate(goods))
    by_pair = {tuple(p): r for p, r in zip(w["pairs"].tolist(), rows)}
    assert all(int(r["cand"].sum()) >= 3 for r in rows), [int(r["cand"].sum()) for r in rows]
    assert int(by_pair[BIG]["cand"].sum()) > 1024
    assert all(0 < int(r["good"].sum()) < len(r["good"]) for r in rows[1:]), "every larger pair has matched and unmatched rows"
    assert any((r["good"] & ~r["cand"]).any() for r in rows), "a non-finite coordinate meets a good row"


@pytest.mark.gpu
def test_three_readers_agree():
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib as L
    w = scene()
    desc, off, pts, prior, pairs = w["desc"], w["offsets"], w["points"], w["prior"], w["pairs"]
    F = len(SIZES)
    robust = dict(ransac_threshold=THRESHOLD, ransac_iterations=ITERATIONS, ransac_seed=SEED)
    with o3dr.Context(0) as ctx:
        rec, good = ctx.matchDescriptors(desc, off, pairs)
        poses, frames, plist = ctx.poseChain(desc, off, pts, prior, min_matches=MIN_MATCHES, return_pairs=True)
        edges = ctx.refinePoses(desc, off, pts, poses, frames["status"], plist, return_edges=True)[3]
        rposes, rframes, rlist, rres = ctx.poseChain(desc, off, pts, prior, min_matches=MIN_MATCHES, return_pairs=True,
                                                     return_ransac=True, **robust)
        redges = ctx.refinePoses(desc, off, pts, rposes, rframes["status"], rlist, return_edges=True, **robust)[3]
        big = next(k for k, p in enumerate(pairs.tolist()) if tuple(p) == BIG)
        rows = numpy_rows(w, rec, good)
        b = rows[big]
        inl, alone = ctx.ransacRigid(PC.points(b["src"]), PC.points(b["tgt"]), THRESHOLD, ITERATIONS, SEED, mask=b["hit"],
                                     seg_keys=[RR.pair_key(*BIG)])
    # the pair list is every (i, j < i), and every frame is accepted: the identities below need both
    assert np.array_equal(plist, pairs) and np.array_equal(rlist, pairs)
    for fr in (frames, rframes):
        assert fr["status"].tolist() == [L.CHAIN_ANCHOR] + [L.CHAIN_MATCHED] * (F - 1), fr["status"].tolist()
    n_good = [int(r["good"].sum()) for r in rows]
    n_cand = [int(r["cand"].sum()) for r in rows]
    assert min(n_cand) >= 3, n_cand
    assert n_cand[big] > L.RANSAC_STAGE, n_cand[big]
    # 1. numpy's used set against the three readers
    assert edges["n_good"].tolist() == n_good and edges["n_used"].tolist() == n_cand, (edges[["n_good", "n_used"]], n_good, n_cand)
    assert frames["n_good"].tolist() == per_frame(w, n_good).tolist(), (frames["n_good"], n_good)
    assert frames["n_used"].tolist() == per_frame(w, n_cand).tolist(), (frames["n_used"], n_cand)
    assert rres["n_candidates"].tolist() == n_cand, (rres["n_candidates"], n_cand)
    # 2. with the RANSAC: the moments and the chain read the bytes the RANSAC wrote
    assert (rres["status"] == L.RANSAC_OK).all(), rres["status"]
    assert redges["n_good"].tolist() == n_good
    assert redges["n_used"].tolist() == rres["n_inliers"].tolist(), (redges["n_used"], rres["n_inliers"])
    assert rframes["n_good"].tolist() == per_frame(w, n_good).tolist()
    assert rframes["n_used"].tolist() == per_frame(w, rres["n_inliers"]).tolist(), (rframes["n_used"], rres["n_inliers"])
    assert any(int(i) < c for i, c in zip(rres["n_inliers"], n_cand)), "the outliers are candidates, not inliers"
    # 4. the stand-alone kernel on the rows numpy gathered: the chain stage's record of that pair, byte for byte
    assert alone[0].tobytes() == rres[big].tobytes(), (alone[0], rres[big])
    assert int(np.count_nonzero(inl)) == int(rres["n_inliers"][big]) and not inl[~b["cand"]].any()
