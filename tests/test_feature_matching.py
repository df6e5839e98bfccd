"""Hamming 2-NN descriptor matching, index-aligned 3-D keypoints and the batched rigid fit (o3dr_match_knn2_hamming,
o3dr_keypoints_3d, o3dr_estimate_rigid_transform; Context.matchDescriptors, keypoints3D, estimateRigidTransform,
matchFeatures).

The contract (include/o3dr.h, DESIGN.md "Feature matching") is restated here in numpy: distances are popcounts of the
XOR, the two smallest keys (d, j) in lexicographic order, the good-match test in fp32 with strict comparisons.  Records are
integers, so the GPU must match them exactly.  The keypoints must equal the CPU oracle's keypoint pass bit for bit.  The
rigid fit is compared with a numpy fp64 Kabsch within 1e-9 (a different SVD and summation order), and with itself bit
for bit across calls, memory kinds and segment batchings."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import assert_points_equal

NONE = 0xFFFFFFFF
POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint32)


# ---- the contract in numpy ----------------------------------------------------------------------------------------------
def knn2_ref(q, t):
    """-> (train_idx [n, 2], distance [n, 2]) uint32, 0xFFFFFFFF where missing"""
    q = np.asarray(q, np.uint8).reshape(-1, 32)
    t = np.asarray(t, np.uint8).reshape(-1, 32)
    n, m = len(q), len(t)
    idx = np.full((n, 2), NONE, np.uint32)
    dist = np.full((n, 2), NONE, np.uint32)
    if m == 0 or n == 0:
        return idx, dist
    j = np.arange(m, dtype=np.uint64)
    for a in range(0, n, 128):
        d = POP8[q[a:a + 128, None, :] ^ t[None, :, :]].sum(-1, dtype=np.uint64)
        key = (d << np.uint64(32)) | j[None, :]
        k = np.sort(np.partition(key, 1, axis=1)[:, :2], axis=1) if m >= 2 else key
        for c in range(k.shape[1]):
            idx[a:a + 128, c] = (k[:, c] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
            dist[a:a + 128, c] = (k[:, c] >> np.uint64(32)).astype(np.uint32)
    return idx, dist


def good_ref(dist, ratio=0.5, max_distance=40):
    d1, d2 = dist[:, 0], dist[:, 1]
    has2 = d2 != NONE
    with np.errstate(invalid="ignore"):
        return has2 & (d1 < max_distance) & (d1.astype(np.float32) < np.float32(ratio) * d2.astype(np.float32))


def batch_ref(desc, offsets, pairs, ratio=0.5, max_distance=40):
    idx, dist = [], []
    for qs, ts in pairs:
        i, d = knn2_ref(desc[offsets[qs]:offsets[qs + 1]], desc[offsets[ts]:offsets[ts + 1]])
        idx.append(i)
        dist.append(d)
    idx = np.concatenate(idx) if idx else np.zeros((0, 2), np.uint32)
    dist = np.concatenate(dist) if dist else np.zeros((0, 2), np.uint32)
    return idx, dist, good_ref(dist, ratio, max_distance)


def kabsch_ref(src, tgt):
    """fp64 Kabsch without scale, the reflection corrected -> 4x4 T mapping src onto tgt"""
    a = np.asarray(src, np.float64)
    b = np.asarray(tgt, np.float64)
    ma, mb = a.mean(0), b.mean(0)
    H = (a - ma).T @ (b - mb)
    U, S, Vt = np.linalg.svd(H)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mb - R @ ma
    return T


def _pts(xyz, rgba=None):
    from online_3d_reconstruction_amd import POINT
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = np.zeros(len(xyz), POINT)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if rgba is not None:
        p["rgba"] = rgba
    return p


def _xyz(p):
    return np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float32)


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _apply(T, xyz):
    return (np.asarray(xyz, np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def _row_bits(k):
    """a descriptor whose first k bits are set"""
    bits = np.zeros(256, np.uint8)
    bits[:k] = 1
    return np.packbits(bits, bitorder="little")


def _flip(row, n, rng):
    bits = np.unpackbits(row, bitorder="little")
    pos = rng.choice(256, n, replace=False)
    bits[pos] ^= 1
    return np.packbits(bits, bitorder="little")


def _records(rec):
    return rec["train_idx"].astype(np.uint32), rec["distance"].astype(np.uint32)


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_defaults():
    from online_3d_reconstruction_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "o3dr.h")).read()
    names = ["o3dr_match_default_params", "o3dr_match_knn2_hamming", "o3dr_keypoints_3d", "o3dr_estimate_rigid_transform"]
    L = C.CDLL(_lib.lib_path())
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in names:
        assert n + "(" in hdr.replace(" (", "("), n
        assert hasattr(L, n), n
        assert n in bound, n
    p = _lib.MatchParamsStruct()
    _lib.load_library().o3dr_match_default_params(C.byref(p))
    assert (p.ratio, p.max_distance) == (0.5, 40)
    assert C.sizeof(_lib.MatchParamsStruct) == 8 and _lib.KNN2.itemsize == 16 and _lib.RIGID_RESULT.itemsize == 152


def test_contract_restatement_on_small_cases():
    q = np.stack([_row_bits(0), _row_bits(3)])
    t = np.stack([_row_bits(5), _row_bits(1), _row_bits(1), _row_bits(256)])
    idx, dist = knn2_ref(q, t)
    assert idx.tolist() == [[1, 2], [0, 1]] and dist.tolist() == [[1, 1], [2, 2]]  # equal distances: lower index first
    assert good_ref(np.array([[39, 78], [39, 79], [40, 200], [0, NONE]], np.uint32)).tolist() == [False, True, False, False]


# ---- matching on the GPU ------------------------------------------------------------------------------------------------
def _pool(rng, sizes):
    desc = rng.integers(0, 256, (int(sum(sizes)), 32), dtype=np.uint8)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return desc, offsets


@pytest.mark.gpu
def test_records_equal_brute_force(ctx):
    rng = np.random.default_rng(11)
    train_sizes = [0, 1, 2, 63, 64, 65, 1500, 5000]
    query_sizes = [1, 7, 64, 65, 300, 1500]
    desc, off = _pool(rng, train_sizes + query_sizes + [4, 3])
    nt = len(train_sizes)
    # planted ties: duplicate train rows inside the 1500 / 5000 sets
    for s in (6, 7):
        a = off[s]
        desc[a + 10] = desc[a + 3]
        desc[a + 11] = desc[a + 3]
        desc[a + 500:a + 520] = desc[a + 100:a + 120]
    # queries equal to a duplicated row: d1 == d2 == 0
    desc[off[nt + 4]:off[nt + 4] + 2] = desc[off[6] + 3]
    # all-zero queries against all-ones rows (distance 256)
    zs, os_ = nt + len(query_sizes), nt + len(query_sizes) + 1
    desc[off[zs]:off[zs + 1]] = 0
    desc[off[os_]:off[os_ + 1]] = 255
    pairs = [(nt + k, s) for k in range(len(query_sizes)) for s in range(nt)]
    pairs += [(zs, os_), (os_, zs), (nt + 3, nt + 3), (6, 6)]  # query_set == train_set: distance 0 to itself
    rec, good = ctx.matchDescriptors(desc, off, pairs)
    idx, dist, g = batch_ref(desc, off, pairs)
    gi, gd = _records(rec)
    assert np.array_equal(gi, idx) and np.array_equal(gd, dist)
    assert np.array_equal(good, g)
    b = sum(off[q + 1] - off[q] for q, _ in pairs[:-4])
    assert (gd[b:b + 4] == 256).all()
    self_rows = gd[-1500:]
    assert (self_rows[:, 0] == 0).all()


@pytest.mark.gpu
def test_batched_equals_one_by_one_and_memory_kinds(ctx):
    import torch
    rng = np.random.default_rng(12)
    sizes = [0, 5, 700, 1, 129, 0, 2000, 64, 33]
    desc, off = _pool(rng, sizes)
    pairs = [(2, 6), (0, 2), (4, 1), (6, 2), (2, 0), (8, 3), (5, 5), (7, 4), (1, 1), (6, 6), (3, 8)]
    rec, good = ctx.matchDescriptors(desc, off, pairs)
    parts = [ctx.matchDescriptors(desc, off, [p]) for p in pairs]
    assert np.array_equal(rec.view(np.uint32), np.concatenate([r for r, _ in parts]).view(np.uint32))
    assert np.array_equal(good, np.concatenate([g for _, g in parts]))
    rec_d, good_d = ctx.matchDescriptors(torch.from_numpy(desc).cuda(), off, pairs)
    assert np.array_equal(rec.view(np.uint32).reshape(-1, 4), rec_d.cpu().numpy().view(np.uint32))
    assert np.array_equal(good, good_d.cpu().numpy())
    rec2, _ = ctx.matchDescriptors(desc, off, pairs)
    assert np.array_equal(rec.view(np.uint32), rec2.view(np.uint32))
    # no pairs, or only empty query sets: no records
    assert len(ctx.matchDescriptors(desc, off, np.zeros((0, 2), np.int32))[0]) == 0
    assert len(ctx.matchDescriptors(desc, off, [(0, 2), (5, 6)])[0]) == 0


@pytest.mark.gpu
def test_good_mask_edges(ctx):
    q = _row_bits(0)[None]
    cases = [  # (train rows by popcount, ratio, max_distance, expected good)
        ([39, 79], 0.5, 40, True),    # d1 = max_distance - 1
        ([40, 200], 0.5, 40, False),  # d1 == max_distance
        ([39, 78], 0.5, 40, False),   # 2 d1 == d2: not strictly below
        ([10, 21], 0.5, 40, True),
        ([3], 0.5, 40, False),        # one-row train set: no second neighbour
        ([200, 251], 0.8, 257, True),
        ([256, 256], 0.8, 257, False),
        ([0, 0], 0.5, 40, False),     # 0 < 0.5 * 0 fails
        ([0, 1], 0.5, 0, False),      # max_distance 0: nothing is good
    ]
    for rows, ratio, md, want in cases:
        desc = np.concatenate([q, np.stack([_row_bits(k) for k in rows])])
        off = np.array([0, 1, 1 + len(rows)], np.int64)
        rec, good = ctx.matchDescriptors(desc, off, [(0, 1)], ratio=ratio, max_distance=md)
        _, dist = _records(rec)
        assert dist[0, 0] == sorted(rows)[0]
        assert bool(good[0]) == want == bool(good_ref(dist, ratio, md)[0]), (rows, ratio, md)


@pytest.mark.gpu
def test_match_rejections(ctx):
    from online_3d_reconstruction_amd import O3drError, _lib
    desc = np.zeros((4, 32), np.uint8)
    off = np.array([0, 2, 4], np.int64)
    for kw in ({"ratio": 0.0}, {"ratio": float("nan")}, {"max_distance": 258}, {"max_distance": -1}):
        with pytest.raises(O3drError):
            ctx.matchDescriptors(desc, off, [(0, 1)], **kw)
    with pytest.raises(O3drError):
        ctx.matchDescriptors(desc, off, [(0, 2)])
    with pytest.raises(O3drError):
        ctx.matchDescriptors(desc, np.array([0, 3, 2], np.int64), [(0, 1)])
    L = _lib.load_library()
    out = np.ones(1, _lib.KNN2)
    n = C.c_int64(-1)
    prs = np.array([0, 1], np.int32)
    rc = L.o3dr_match_knn2_hamming(ctx._h, desc.ctypes.data, off.ctypes.data, 2, prs.ctypes.data, 1, None, out.ctypes.data, None, 1,
                                   C.byref(n), _lib.MEM_HOST)
    assert rc == _lib.ERR_CAPACITY and n.value == 2


# ---- 3-D keypoints ------------------------------------------------------------------------------------------------------
def _keypoints(rng, rows, cols, n):
    kp = np.stack([rng.uniform(-3, cols + 3, n), rng.uniform(-3, rows + 3, n)], 1).astype(np.float32)
    kp[: n // 4] = np.floor(kp[: n // 4])  # whole-pixel coordinates next to fractional ones
    kp[n // 4: n // 4 + 4] = [[0.0, 0.0], [cols / 8 - 0.5, 100.5], [cols - 20.0, 300.0], [cols - 20.5, 300.0]]
    return kp


def _accepted(disp, kp, bb=20, ratio=8, min_disp=64.0):
    rows, cols = disp.shape
    x = np.trunc(kp[:, 0]).astype(np.int64)
    y = np.trunc(kp[:, 1]).astype(np.int64)
    roi = (x >= int(cols / ratio)) & (x < cols - bb) & (y >= bb) & (y < rows - bb)
    ok = np.zeros(len(kp), bool)
    ok[roi] = disp[y[roi], x[roi]] > min_disp
    return ok


@pytest.mark.gpu
def test_keypoints3d_equal_the_keypoint_pass(ctx, orc, Q, frame_1248, frame_1249):
    import torch
    rng = np.random.default_rng(13)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = _rot([0.3, -1.0, 0.2], 0.7)
    T[:3, 3] = [12.5, -3.25, 40.0]
    for disp, bgr in (frame_1248, frame_1249):
        rows, cols = disp.shape
        kp = _keypoints(rng, rows, cols, 3000)
        # keypoints inside the ROI on disparity <= 64 (64 itself: the test is strict)
        disp = disp.copy()
        inside = np.nonzero(_accepted(np.full_like(disp, 255), kp))[0][:200]
        disp[kp[inside, 1].astype(int), kp[inside, 0].astype(int)] = np.where(np.arange(len(inside)) % 2 == 0, 64, 7)
        ok = _accepted(disp, kp)
        assert ok.sum() > 100 and (~ok).sum() > 300
        ref = orc.create_single_img_pt_cloud(disp, bgr, Q, jump_pixels=0, kp_xy=kp)
        got = ctx.keypoints3D(disp, kp, bgr=bgr)
        assert len(got) == len(kp)
        fin = np.isfinite(got["x"])
        assert np.array_equal(fin, ok)
        assert_points_equal(got[ok], ref, "camera frame")
        assert np.isnan(got["y"][~ok]).all() and np.isnan(got["z"][~ok]).all() and (got["rgba"][~ok] == 0).all()
        posed = ctx.keypoints3D(disp, kp, poses=T, bgr=bgr)
        assert_points_equal(posed[ok], orc.transform_pt_cloud(ref, T), "posed")
        nob = ctx.keypoints3D(disp, kp)
        assert (nob["rgba"] == 0).all() and np.array_equal(nob.view(np.uint32).reshape(-1, 4)[:, :3], got.view(np.uint32).reshape(-1, 4)[:, :3])
        dev = ctx.keypoints3D(torch.from_numpy(disp).cuda(), torch.from_numpy(kp).cuda(), poses=torch.from_numpy(T).cuda(),
                              bgr=torch.from_numpy(bgr).cuda())
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), posed.view(np.uint32).reshape(-1, 4))
    # a stack of two frames with their own poses and keypoint lists (one of them empty in between)
    d2 = np.stack([frame_1248[0], frame_1249[0]])
    b2 = np.stack([frame_1248[1], frame_1249[1]])
    kps = [_keypoints(rng, *d2.shape[1:], 500), _keypoints(rng, *d2.shape[1:], 700)]
    poses = np.stack([T, np.eye(4, dtype=np.float32)])
    got = ctx.keypoints3D(d2, kps, poses=poses, bgr=b2)
    one = [ctx.keypoints3D(d2[f], kps[f], poses=poses[f], bgr=b2[f]) for f in range(2)]
    assert np.array_equal(got.view(np.uint32), np.concatenate(one).view(np.uint32))


# ---- rigid fit ----------------------------------------------------------------------------------------------------------
def _fit_case(rng, n, R, t, planar=False):
    src = rng.uniform(-10, 10, (n, 3))
    if planar:
        src[:, 2] = 0.0
    src = src.astype(np.float32)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return src, _apply(T, src), T


def _rms(T, src, tgt):
    e = np.asarray(src, np.float64) @ T[:3, :3].T + T[:3, 3] - np.asarray(tgt, np.float64)
    return np.sqrt((e * e).sum(1).mean())


@pytest.mark.gpu
def test_rigid_recovers_known_transforms(ctx):
    from online_3d_reconstruction_amd import _lib
    rng = np.random.default_rng(14)
    cases = [
        (_rot([1, 2, 3], 0.4), [1.0, -2.0, 3.0], False),
        (_rot([0.2, -0.5, 1.0], np.pi - 1e-3), [20.0, 5.0, -7.0], False),  # near 180 degrees
        (_rot([0, 0, 1], np.pi), [0.5, 0.5, 0.5], False),                   # exactly 180 degrees
        (_rot([1, 1, 0], 1.1), [-3.0, 0.0, 8.0], True),                      # a planar set: the SVD may reflect
        (np.eye(3), [0.0, 0.0, 0.0], False),
    ]
    for R, t, planar in cases:
        src, tgt, T = _fit_case(rng, 700, R, t, planar)
        r = ctx.estimateRigidTransform(_pts(src), _pts(tgt))
        assert r.status == _lib.RIGID_OK and r.n_used == 700
        ref = kabsch_ref(src, tgt)
        assert np.abs(r.T - ref).max() < 1e-9, (np.abs(r.T - ref).max(), planar)
        assert np.abs(r.T - T).max() < 1e-4
        assert abs(np.linalg.det(r.T[:3, :3]) - 1.0) < 1e-12
        assert abs(r.rms - _rms(r.T, src, tgt)) < 1e-9


@pytest.mark.gpu
def test_rigid_too_few_degenerate_mask_and_nonfinite(ctx):
    from online_3d_reconstruction_amd import _lib
    rng = np.random.default_rng(15)
    r = ctx.estimateRigidTransform(_pts([[0, 0, 0], [1, 0, 0]]), _pts([[1, 2, 3], [2, 2, 3]]))
    assert r.status == _lib.RIGID_TOO_FEW and r.n_used == 2 and np.array_equal(r.T, np.eye(4))
    line = np.stack([np.arange(50, dtype=np.float32), np.zeros(50, np.float32), np.zeros(50, np.float32)], 1)
    r = ctx.estimateRigidTransform(_pts(line), _pts(line + np.float32([1, 2, 3])))
    assert r.status == _lib.RIGID_DEGENERATE and r.n_used == 50 and np.array_equal(r.T, np.eye(4))
    e = ctx.estimateRigidTransform(_pts(np.zeros((0, 3))), _pts(np.zeros((0, 3))))
    assert e.status == _lib.RIGID_TOO_FEW and e.n_used == 0 and e.rms == 0.0
    # masked-out pairs and pairs with a non-finite coordinate (either side) are skipped
    src, tgt, T = _fit_case(rng, 900, _rot([3, -1, 2], 0.9), [4.0, 1.0, -2.0])
    mask = rng.random(900) < 0.8
    tgt_bad = tgt.copy()
    src_bad = src.copy()
    tgt_bad[~mask] += rng.normal(0, 5, ((~mask).sum(), 3)).astype(np.float32)  # outliers, masked out
    src_bad[5] = np.nan
    tgt_bad[17, 1] = np.inf
    src_bad[33, 2] = -np.inf
    used = mask.copy()
    used[[5, 17, 33]] = False
    r = ctx.estimateRigidTransform(_pts(src_bad), _pts(tgt_bad), mask=mask)
    assert r.status == _lib.RIGID_OK and r.n_used == used.sum()
    assert np.abs(r.T - kabsch_ref(src[used], tgt[used])).max() < 1e-9
    assert abs(r.rms - _rms(r.T, src[used], tgt[used])) < 1e-9


@pytest.mark.gpu
def test_rigid_segments_equal_separate_calls_and_reproducible(ctx):
    import torch
    rng = np.random.default_rng(16)
    sizes = [700, 0, 2, 300, 1, 257, 256, 5000]
    srcs, tgts = [], []
    for k, n in enumerate(sizes):
        s, t, _ = _fit_case(rng, n, _rot(rng.normal(size=3), rng.uniform(0, np.pi)), rng.normal(0, 10, 3))
        srcs.append(s)
        tgts.append(t + rng.normal(0, 1e-3, t.shape).astype(np.float32))
    src, tgt = _pts(np.concatenate(srcs)), _pts(np.concatenate(tgts))
    mask = (rng.random(len(src)) < 0.9).astype(np.uint8)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    batched = ctx.estimateRigidTransform(src, tgt, seg_offsets=off, mask=mask)
    again = ctx.estimateRigidTransform(src, tgt, seg_offsets=off, mask=mask)
    dev = ctx.estimateRigidTransform(torch.from_numpy(src.view(np.int32).reshape(-1, 4)).cuda(),
                                     torch.from_numpy(tgt.view(np.int32).reshape(-1, 4)).cuda(), seg_offsets=off,
                                     mask=torch.from_numpy(mask).cuda())
    for s in range(len(sizes)):
        a, b = off[s], off[s + 1]
        one = ctx.estimateRigidTransform(src[a:b], tgt[a:b], mask=mask[a:b])
        for other in (one, again[s], dev[s]):
            assert np.array_equal(batched[s].T, other.T) and batched[s].rms == other.rms
            assert batched[s].n_used == other.n_used and batched[s].status == other.status
        assert batched[s].n_used == int(mask[a:b].sum())


# ---- end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_match_features_end_to_end_on_frame_1248(ctx, frame_1248):
    import torch
    rng = np.random.default_rng(17)
    disp, bgr = frame_1248
    rows, cols = disp.shape
    ys, xs = np.nonzero(disp > 64)
    keep = (xs >= cols // 8) & (xs < cols - 20) & (ys >= 20) & (ys < rows - 20)
    sel = rng.choice(np.nonzero(keep)[0], 1000, replace=False)
    kp = np.stack([xs[sel] + 0.25, ys[sel] + 0.75], 1).astype(np.float32)
    kp3_q = ctx.keypoints3D(disp, kp, bgr=bgr)
    assert np.isfinite(kp3_q["x"]).all()
    T = np.eye(4)
    T[:3, :3] = _rot([0.1, 1.0, -0.3], 0.35)
    T[:3, 3] = [2.0, -1.5, 0.75]
    n_true = 700  # 30 % of the queries are outliers with no counterpart
    desc_q = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    n_dis = 400
    perm = rng.permutation(n_true + n_dis)  # train row of true pair i: perm[i]
    desc_t = rng.integers(0, 256, (n_true + n_dis, 32), dtype=np.uint8)
    xyz_t = rng.uniform(-30, 30, (n_true + n_dis, 3)).astype(np.float32)
    for i in range(n_true):
        desc_t[perm[i]] = _flip(desc_q[i], int(rng.integers(0, 9)), rng)
        xyz_t[perm[i]] = _apply(T, _xyz(kp3_q[i:i + 1]))[0]
    kp3_t = _pts(xyz_t)
    rec, kept, res = ctx.matchFeatures(desc_q, desc_t, kp3_q, kp3_t)
    planted = np.zeros(1000, bool)
    planted[:n_true] = True
    assert np.array_equal(kept, planted)
    assert np.array_equal(rec["train_idx"][:n_true, 0], perm[:n_true])
    assert res.status == 0 and res.n_used == n_true
    assert np.abs(res.T - T).max() < 1e-5
    rec_d, kept_d, res_d = ctx.matchFeatures(torch.from_numpy(desc_q).cuda(), torch.from_numpy(desc_t).cuda(),
                                             torch.from_numpy(kp3_q.view(np.int32).reshape(-1, 4)).cuda(),
                                             torch.from_numpy(kp3_t.view(np.int32).reshape(-1, 4)).cuda())
    assert np.array_equal(kept_d.cpu().numpy(), kept) and np.array_equal(res_d.T, res.T)


# ---- scale --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_scale_against_chunked_torch_reference(ctx):
    import torch
    rng = np.random.default_rng(18)
    n_sets, rows = 200, 1500
    desc = rng.integers(0, 256, (n_sets * rows, 32), dtype=np.uint8)
    desc[rows * 7 + 5] = desc[rows * 3 + 9]  # a few planted duplicates across sets
    desc[rows * 7 + 6] = desc[rows * 3 + 9]
    off = np.arange(n_sets + 1, dtype=np.int64) * rows
    pairs = np.array([(s, (s + k) % n_sets) for s in range(n_sets) for k in range(1, 9)], np.int32)
    dd = torch.from_numpy(desc).cuda()
    rec, good = ctx.matchDescriptors(dd, off, pairs)
    got = rec.view(torch.int64).reshape(-1, 2)  # (idx0 | idx1 << 32), (d0 | d1 << 32)
    pop = torch.tensor(POP8, dtype=torch.int32, device="cuda")
    j = torch.arange(rows, device="cuda", dtype=torch.int64)
    for p0 in range(0, len(pairs), 8):
        q = torch.stack([dd[int(off[a]):int(off[a + 1])] for a, _ in pairs[p0:p0 + 8]]).to(torch.int32)
        t = torch.stack([dd[int(off[b]):int(off[b + 1])] for _, b in pairs[p0:p0 + 8]]).to(torch.int32)
        d = torch.zeros((len(q), rows, rows), dtype=torch.int64, device="cuda")
        for k in range(32):
            d += pop[q[:, :, None, k] ^ t[:, None, :, k]]
        key = (d << 32) | j
        best = torch.topk(key, 2, dim=2, largest=False, sorted=True).values
        idx = (best[..., 0] & 0xFFFFFFFF) | ((best[..., 1] & 0xFFFFFFFF) << 32)
        dist = (best[..., 0] >> 32) | ((best[..., 1] >> 32) << 32)
        g = got[p0 * rows:(p0 + len(q)) * rows]
        assert torch.equal(g[:, 0], idx.reshape(-1)) and torch.equal(g[:, 1], dist.reshape(-1)), p0
        d1, d2 = (best[..., 0] >> 32).reshape(-1), (best[..., 1] >> 32).reshape(-1)
        gr = (d1 < 40) & (d1.to(torch.float32) < 0.5 * d2.to(torch.float32))
        assert torch.equal(good[p0 * rows:(p0 + len(q)) * rows], gr), p0


# ---- chunk sizes other than 64 ------------------------------------------------------------------------------------------
BIG_TRAIN = [127, 128, 129, 5000, 1]
BIG_QUERY = [1, 65, 300]
BIG_FILLERS = {128: (6400, 8000), 192: (6400, 12000)}  # chunk_rows -> (nq, nt) of a filler pair that raises the call's chunk size


def _chunk_rows(pairs_sizes):
    """match_plan's chunk size (o3dr_api.hip) restated: work = sum over the pairs of ceil(nq / 64) nt, aimed at 8192 work
    items, rounded up to a multiple of 64, at least 64"""
    work = sum(-(-nq // 64) * nt for nq, nt in pairs_sizes)
    return max(64, -(-(-(-work // 8192)) // 64) * 64)


def _big_chunk_pool(chunk):
    """-> (desc, offsets, the checked pairs, the filler pair).  Sets: BIG_TRAIN, BIG_QUERY, the filler's query and train set.
    Duplicate train rows straddle the chunk boundaries 128 (rows 127 | 128), 192 (191 | 192) and 4992 = 39 x 128 = 26 x 192
    (4991 | 4992), and queries equal them: d1 == d2 == 0, decided by the lower row, across two chunks."""
    rng = np.random.default_rng(19 + chunk)
    fq, ft = BIG_FILLERS[chunk]
    desc, off = _pool(rng, BIG_TRAIN + BIG_QUERY + [fq, ft])
    nt = len(BIG_TRAIN)
    t129, t5000 = int(off[2]), int(off[3])
    desc[t129 + 128] = desc[t129 + 127]
    for a in (127, 191, 4991):
        desc[t5000 + a + 1] = desc[t5000 + a]
    for qs in (nt + 1, nt + 2):  # the 65- and the 300-row query sets
        q0 = int(off[qs])
        desc[q0 + 3] = desc[t5000 + 127]
        desc[q0 + 20] = desc[t5000 + 191]
        desc[q0 + 64] = desc[t5000 + 4991]
        desc[q0 + 40] = desc[t129 + 127]
    checked = [(nt + k, s) for k in range(len(BIG_QUERY)) for s in range(nt)]
    filler = (nt + len(BIG_QUERY), nt + len(BIG_QUERY) + 1)
    return desc, off, checked, filler


@pytest.mark.parametrize("chunk", sorted(BIG_FILLERS))
def test_filler_pair_raises_the_chunk_size(chunk):
    """CPU twin of test_multi_chunk_pairs_with_a_larger_chunk: with the filler the call's chunk is 128 / 192, so the
    5000-row train set takes 40 / 27 chunks with a partial last one; without it the checked pairs run at 64."""
    desc, off, checked, filler = _big_chunk_pool(chunk)
    size = lambda s: int(off[s + 1] - off[s])  # noqa: E731
    sizes = [(size(q), size(t)) for q, t in checked]
    assert sorted(set(sizes)) == sorted((q, t) for q in BIG_QUERY for t in BIG_TRAIN)
    assert _chunk_rows(sizes) == 64
    c = _chunk_rows(sizes + [(size(filler[0]), size(filler[1]))])
    assert c == chunk > 64 and 5000 % c != 0 and c < 5000 and 4992 % c == 0 and size(filler[1]) % c != 0
    assert _chunk_rows([(1500, 1500)] * 1600) == 7040  # test_scale_against_chunked_torch_reference: one chunk per pair
    idx, dist, _ = batch_ref(desc, off, [(len(BIG_TRAIN) + 2, 3), (len(BIG_TRAIN) + 2, 2)])
    assert idx[[3, 20, 64]].tolist() == [[127, 128], [191, 192], [4991, 4992]] and not dist[[3, 20, 64]].any()
    assert idx[300 + 40].tolist() == [127, 128] and not dist[300 + 40].any()


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", sorted(BIG_FILLERS))
def test_multi_chunk_pairs_with_a_larger_chunk(ctx, chunk):
    """Checked pairs next to a filler pair that raises chunk_rows to 128 / 192 (test_filler_pair_raises_the_chunk_size):
    their records and good mask equal the brute force and, bit for bit, the same pairs run alone at chunk 64.  The filler
    itself is checked against a torch top-2 on the device, 400 query rows at a time."""
    import torch
    desc, off, checked, filler = _big_chunk_pool(chunk)
    rec, good = ctx.matchDescriptors(desc, off, [filler] + checked)
    fq = int(off[filler[0] + 1] - off[filler[0]])
    n = sum(int(off[q + 1] - off[q]) for q, _ in checked)
    assert len(rec) == fq + n
    mid, gmid = rec[fq:fq + n], good[fq:fq + n]
    idx, dist, g = batch_ref(desc, off, checked)
    gi, gd = _records(mid)
    assert np.array_equal(gi, idx) and np.array_equal(gd, dist) and np.array_equal(gmid, g)
    alone, galone = ctx.matchDescriptors(desc, off, checked)
    assert alone.tobytes() == mid.tobytes() and np.array_equal(galone, gmid)
    # the filler: (d << 32 | row) keys, the two smallest per query row
    dd = torch.from_numpy(desc).cuda()
    pop = torch.tensor(POP8, dtype=torch.int32, device="cuda")
    q = dd[int(off[filler[0]]):int(off[filler[0] + 1])].to(torch.int32)
    t = dd[int(off[filler[1]]):int(off[filler[1] + 1])].to(torch.int32)
    j = torch.arange(len(t), device="cuda", dtype=torch.int64)
    got = torch.from_numpy(np.ascontiguousarray(rec[:fq]).view(np.uint32).reshape(-1, 4).astype(np.int64)).cuda()
    for a in range(0, fq, 400):
        d = torch.zeros((len(q[a:a + 400]), len(t)), dtype=torch.int64, device="cuda")
        for k in range(32):
            d += pop[q[a:a + 400, None, k] ^ t[None, :, k]]
        best = torch.topk((d << 32) | j, 2, dim=1, largest=False, sorted=True).values
        want = torch.stack([best[:, 0] & 0xFFFFFFFF, best[:, 1] & 0xFFFFFFFF, best[:, 0] >> 32, best[:, 1] >> 32], 1)
        assert torch.equal(got[a:a + 400], want), a
        d1, d2 = want[:, 2], want[:, 3]
        gr = (d1 < 40) & (d1.to(torch.float32) < 0.5 * d2.to(torch.float32))
        assert np.array_equal(good[a:a + 400], gr.cpu().numpy()), a
