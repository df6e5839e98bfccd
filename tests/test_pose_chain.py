"""The pose chain (o3dr_pose_chain / Context.poseChain, Context.trackFrames; contract: include/o3dr.h "pose chain") against
its numpy restatement (tests/pose_chain_reference.py) on small synthetic worlds: 6-9 frames of 40-150 rows.

Integer outputs (pair list, statuses, counts) must equal the reference's.  Poses cannot: the reference's SVD and summation
order differ in the last bits of fp64, which now and then rounds an fp32 pose entry the other way, and later frames inherit
it.  The bound is therefore measured on the reference itself (test_whole_chain_poses)."""
import ctypes as C

import numpy as np
import pytest

import pose_chain_reference as R

DIST = 1.2  # with 0.5 m per frame and priors off by at most 0.05 m per axis: the two frames before, never the third
MIN_MATCHES = 30


def _world_a():
    return R.make_world(11, R.random_views(12, 8, 260, 150), 260)


_CACHE = {}


def world_a():
    if "a" not in _CACHE:
        w = _world_a()
        _CACHE["a"] = (w, R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=DIST))
    return _CACHE["a"]


def run(ctx, w, **kw):
    kw.setdefault("dist_nearby", DIST)
    return ctx.poseChain(w["desc"], w["offsets"], R.points(w["kp3"]), w["prior"], **kw)


def assert_integers_equal(rec, ref, pairs=None):
    for k in ("status", "n_pairs", "n_pairs_accepted", "n_good", "n_used"):
        assert np.array_equal(rec[k], ref[k]), (k, rec[k], ref[k])
    if pairs is not None:
        assert [tuple(p) for p in pairs.tolist()] == ref["pairs"]


def max_pose_diff(a, b):
    return float(np.abs(np.asarray(a, np.float64).reshape(-1, 16) - np.asarray(b, np.float64).reshape(-1, 16)).max())


# ---- CPU: the generator gives what the tests need, the reference recovers the truth -----------------------------------------
def test_world_and_reference_on_the_cpu():
    """Every true correspondence passes the ratio test and the distance gate and is the best match, no false one passes,
    and the reference alone recovers the true poses relative to frame 0.  Pose bound 1e-4: kp3 is rounded to fp32 (half an
    ulp of 10 m is 5e-7), a moved tgt adds a few fp32 roundings of the same size, the fit averages ~170 of them and eight
    frames chain up; 1e-4 is two orders above that and four below the 0.5 m between frames."""
    w, ref = world_a()
    off, lm = w["offsets"], w["landmark"]
    assert len(ref["pairs"]) == 1 + 2 * 6 and ref["pairs"][:3] == [(1, 0), (2, 1), (2, 0)]
    for i, j in ref["pairs"]:
        idx, dist = R.knn2_ref(w["desc"][off[i]:off[i + 1]], w["desc"][off[j]:off[j + 1]])
        good = R.good_ref(dist)
        lq, lt = lm[off[i]:off[i + 1]], lm[off[j]:off[j + 1]]
        shared = np.isin(lq, lt)
        assert np.array_equal(good, shared)
        assert np.array_equal(lt[idx[shared, 0].astype(np.int64)], lq[shared])
    assert ref["status"].tolist() == [R.ANCHOR] + [R.MATCHED] * 7
    assert (np.abs(ref["n_used"][1:] - MIN_MATCHES) >= 10).all()
    assert ref["n_pairs"].tolist() == [0, 1] + [2] * 6 and (ref["n_pairs"][2:] * 150 > 256).all()  # crosses a run boundary
    E = ref["poses"][0].reshape(4, 4).astype(np.float64) @ np.linalg.inv(w["true"][0])
    for i in range(8):
        assert np.abs(ref["poses"][i].reshape(4, 4) - E @ w["true"][i]).max() < 1e-4
    assert ref["rms"][1:].max() < 1e-5


def test_pair_list_rules():
    prior = np.tile(np.eye(4, dtype=np.float32).reshape(16), (6, 1))
    prior[:, 3] = [0, 1, 2, 3, 3, 10]
    assert R.pair_list(prior, 1.0, 8) == [(1, 0), (2, 1), (3, 2), (4, 3), (4, 2)]      # non-strict, frame 5 isolated
    assert R.pair_list(prior, 2.0, 2) == [(1, 0), (2, 1), (2, 0), (3, 2), (3, 1), (4, 3), (4, 2)]  # the most recent two
    assert R.pair_list(prior, 2.0, 2, n_fixed=3) == [(3, 2), (3, 1), (4, 3), (4, 2)]   # the split drops whole frames only
    prior[:, 3] = np.arange(6)
    assert R.pair_list(prior, 0.0, 8) == []


# ---- GPU --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_exact_parity(ctx):
    w, ref = world_a()
    poses, rec, pairs = run(ctx, w, return_pairs=True)
    assert rec.dtype.itemsize == 128 and poses.shape == (8, 4, 4) and poses.dtype == np.float32
    assert_integers_equal(rec, ref, pairs)
    assert np.array_equal(poses[0].reshape(16), w["prior"][0])
    assert (poses[:, 3] == np.array([0, 0, 0, 1], np.float32)).all()
    m = rec["status"] == R.MATCHED
    assert np.array_equal(rec["T"][m].astype(np.float32), poses[m].reshape(-1, 16)[:, :12])
    assert np.array_equal(rec["T"][~m], poses[~m].reshape(-1, 16)[:, :12].astype(np.float64))


@pytest.mark.gpu
def test_single_fit_agrees_with_estimate_rigid_transform(ctx):
    """Frame 5 alone (history = the reference's own poses, so both sides gather the same correspondences): T within 1e-9 of
    estimateRigidTransform on the reference's gathered pairs, rms within 1e-9 relative - the bound
    tests/test_feature_matching.py uses for a different SVD and summation order."""
    w, ref = world_a()
    i = 5
    poses, rec = run(ctx, w, n_fixed=i, poses_in=ref["poses"][:i], status_in=ref["status"][:i])
    src, tgt = ref["gathered"][i]
    assert len(src) == rec["n_used"][i] > 100
    fit = ctx.estimateRigidTransform(R.points(src), R.points(tgt))
    assert fit.status == 0 and rec["status"][i] == R.MATCHED
    assert np.abs(rec["T"][i].reshape(3, 4) - fit.T[:3]).max() <= 1e-9
    assert abs(rec["rms"][i] - fit.rms) <= 1e-9 * fit.rms
    assert np.abs(rec["T"][i] - ref["T"][i]).max() <= 1e-9


@pytest.mark.gpu
def test_whole_chain_poses(ctx):
    """Poses against the reference chain.  The floor is the reference's own sensitivity to the last bit of a pose: the
    reference chain with every fitted fp32 pose entry moved one ulp up, and one ulp down, differs from itself by at most
    FLOOR (measured on the CPU for this world: 1.6e-06, largest absolute difference of a pose entry).  4 x the floor is
    allowed: an fp32 pose entry near a tie may round the other way under another fp64 summation order, and later frames
    inherit it."""
    w, ref = world_a()
    floor = max(max_pose_diff(R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=DIST, nudge=s)["poses"],
                              ref["poses"]) for s in (1, -1))
    poses, rec = run(ctx, w)
    diff = max_pose_diff(poses, ref["poses"])
    print(f"pose chain: floor {floor:.3e}, gpu vs reference {diff:.3e}")
    assert 0 < floor < 1e-4
    assert diff <= 4 * floor
    assert np.allclose(rec["rms"], ref["rms"], rtol=0, atol=4 * floor)


@pytest.mark.gpu
def test_middle_rejection(ctx):
    """Frame 3 shares 5 landmarks with the others: TOO_FEW.  Frames 4 and 5 skip it as a train frame and match the older
    one."""
    views = R.random_views(21, 7, 260, 120)
    views[3] = np.concatenate([np.arange(260, 360), views[2][:5]])
    w = R.make_world(22, views, 360)
    ref = R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=DIST)
    assert ref["status"].tolist() == [R.ANCHOR, R.MATCHED, R.MATCHED, R.TOO_FEW, R.MATCHED, R.MATCHED, R.MATCHED]
    assert ref["n_pairs"][4] == 2 and ref["n_pairs_accepted"][4] == 1 and ref["n_pairs_accepted"][5] == 1
    poses, rec, pairs = run(ctx, w, return_pairs=True)
    assert_integers_equal(rec, ref, pairs)
    assert np.array_equal(poses[3].reshape(16), w["prior"][3]) and rec["n_used"][3] < MIN_MATCHES
    assert max_pose_diff(poses, ref["poses"]) < 1e-4


@pytest.mark.gpu
def test_isolated_frame_is_an_anchor(ctx):
    true = np.stack([R.true_pose(k) for k in range(6)])
    true[4:, 1, 3] += 20.0
    w = R.make_world(31, R.random_views(32, 6, 200, 120), 200, poses=true)
    ref = R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=DIST)
    assert ref["status"].tolist() == [R.ANCHOR, R.MATCHED, R.MATCHED, R.MATCHED, R.ANCHOR, R.MATCHED]
    poses, rec, pairs = run(ctx, w, return_pairs=True)
    assert_integers_equal(rec, ref, pairs)
    assert np.array_equal(poses[4].reshape(16), w["prior"][4]) and rec["n_pairs"][4] == 0
    assert not any(q == 4 for q, _ in pairs.tolist()) and [5, 4] in pairs.tolist()


@pytest.mark.gpu
def test_nan_rows_are_skipped(ctx):
    w = dict(_world_a())
    w["kp3"] = w["kp3"].copy()
    off = w["offsets"]
    w["kp3"][off[2]:off[2] + 40, 0] = np.nan  # as query rows of frame 2 and as train rows of frames 3 and 4
    w["kp3"][off[5] + 7:off[5] + 30, 2] = np.nan
    ref = R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=DIST)
    assert (ref["n_used"][[2, 3, 4, 5, 6, 7]] < ref["n_good"][[2, 3, 4, 5, 6, 7]]).all()
    assert np.array_equal(ref["n_used"][:2], ref["n_good"][:2])
    poses, rec = run(ctx, w)
    assert_integers_equal(rec, ref)
    assert np.isfinite(poses).all() and max_pose_diff(poses, ref["poses"]) < 1e-4


@pytest.mark.gpu
def test_degenerate_frame(ctx):
    """Frame 3's points lie on one line (exact in fp32): the cross-covariance has rank 1."""
    w = dict(_world_a())
    w["kp3"] = w["kp3"].copy()
    off = w["offsets"]
    n = int(off[4] - off[3])
    w["kp3"][off[3]:off[4]] = np.stack([np.arange(n) / 8.0, np.full(n, 1.0), np.full(n, 2.0)], 1).astype(np.float32)
    ref = R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=DIST)
    assert ref["status"][3] == R.DEGENERATE and (ref["status"][4:] == R.MATCHED).all()
    poses, rec = run(ctx, w)
    assert_integers_equal(rec, ref)
    assert np.array_equal(poses[3].reshape(16), w["prior"][3]) and rec["rms"][3] == 0.0
    assert rec["n_pairs_accepted"][4] == 1 and rec["n_pairs_accepted"][5] == 1


@pytest.mark.gpu
def test_rms_gate(ctx):
    """Six of frame 3's 3-D keypoints swapped with six others: metres of residual on a dozen correspondences.  The other
    frames fit to ~1e-6 (test_world_and_reference_on_the_cpu), so a gate of 0.05 m rejects frame 3 alone."""
    w = dict(_world_a())
    w["kp3"] = w["kp3"].copy()
    o = int(w["offsets"][3])
    a, b = np.arange(o, o + 6), np.arange(o + 70, o + 76)
    w["kp3"][np.concatenate([a, b])] = w["kp3"][np.concatenate([b, a])]
    ref = R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=DIST, max_rms=0.05)
    assert ref["status"].tolist() == [R.ANCHOR, R.MATCHED, R.MATCHED, R.RMS] + [R.MATCHED] * 4 and ref["rms"][3] > 0.2
    poses, rec = run(ctx, w, max_rms=0.05)
    assert_integers_equal(rec, ref)
    assert np.array_equal(poses[3].reshape(16), w["prior"][3])
    assert abs(rec["rms"][3] - ref["rms"][3]) < 1e-4
    _, rec2 = run(ctx, w)  # without the gate the same fit is accepted
    assert rec2["status"][3] == R.MATCHED and rec2["rms"][3] == rec["rms"][3]


@pytest.mark.gpu
def test_range_width_keeps_the_most_recent(ctx):
    w, _ = world_a()
    ref = R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=10.0, range_width=3)
    assert [j for q, j in ref["pairs"] if q == 6] == [5, 4, 3] and ref["n_pairs"].tolist() == [0, 1, 2, 3, 3, 3, 3, 3]
    poses, rec, pairs = run(ctx, w, dist_nearby=10.0, range_width=3, return_pairs=True)
    assert_integers_equal(rec, ref, pairs)
    _, rec8 = run(ctx, w, dist_nearby=10.0)
    assert rec8["n_pairs"].tolist() == list(range(8))


@pytest.mark.gpu
def test_bit_reproducibility_memory_kinds_and_splits(ctx):
    import torch
    w, _ = world_a()
    off = w["offsets"]
    pts = R.points(w["kp3"])
    poses, rec = run(ctx, w)
    again = run(ctx, w)
    assert poses.tobytes() == again[0].tobytes() and rec.tobytes() == again[1].tobytes()
    d_desc = torch.from_numpy(w["desc"]).cuda()
    d_kp3 = torch.from_numpy(pts.view(np.int32).reshape(-1, 4)).cuda()
    dp, drec = ctx.poseChain(d_desc, off, d_kp3, w["prior"], dist_nearby=DIST)
    assert dp.is_cuda and dp.cpu().numpy().tobytes() == poses.tobytes() and drec.tobytes() == rec.tobytes()
    for k in range(9):
        p1, r1 = ctx.poseChain(w["desc"][:off[k]], off[:k + 1], pts[:off[k]], w["prior"][:k], dist_nearby=DIST)
        p2, r2 = run(ctx, w, n_fixed=k, poses_in=p1, status_in=r1["status"])
        assert p1.tobytes() == poses[:k].tobytes() and r1.tobytes() == rec[:k].tobytes(), k
        assert p2.tobytes() == poses.tobytes() and r2[k:].tobytes() == rec[k:].tobytes(), k
        assert np.array_equal(r2["status"][:k], rec["status"][:k]) and not r2["n_pairs"][:k].any()


@pytest.mark.gpu
def test_empty_frames_and_no_frames(ctx):
    views = R.random_views(41, 6, 200, 120)
    views[2] = views[2][:0]
    views[5] = views[5][:0]
    w = R.make_world(42, views, 200)
    ref = R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=DIST)
    assert ref["status"].tolist() == [R.ANCHOR, R.MATCHED, R.TOO_FEW, R.MATCHED, R.MATCHED, R.TOO_FEW]
    poses, rec, pairs = run(ctx, w, return_pairs=True)
    assert_integers_equal(rec, ref, pairs)
    assert rec["n_used"][2] == 0 and rec["n_pairs"][5] == 2 and rec["n_good"][5] == 0
    poses, rec, pairs = ctx.poseChain(np.zeros((0, 32), np.uint8), [0], R.points(np.zeros((0, 3))), np.zeros((0, 16), np.float32),
                                      return_pairs=True)
    assert poses.shape == (0, 4, 4) and len(rec) == 0 and len(pairs) == 0


@pytest.mark.gpu
def test_argument_errors_zero_the_outputs(ctx):
    from online_3d_reconstruction_amd import _lib as L
    w, ref = world_a()
    pts = R.points(w["kp3"])
    off = w["offsets"]
    F = 8

    def call(n_fixed=0, status=None, **prm):
        p = L.ChainParamsStruct()
        ctx._lib.o3dr_chain_default_params(C.byref(p))
        for k, v in prm.items():
            setattr(p, k, v)
        poses = np.full((F, 16), 7.0, np.float32)
        rec = np.full(F * 128, 0xFF, np.uint8).view(L.CHAIN_FRAME)
        pairs = np.full((F * 32, 2), 9, np.int32)
        n = C.c_int64(5)
        st = np.asarray(ref["status"] if status is None else status, np.int32)
        rc = ctx._lib.o3dr_pose_chain(ctx._h, w["desc"].ctypes.data, off.ctypes.data, pts.ctypes.data, w["prior"].ctypes.data, F, n_fixed,
                                      ref["poses"].ctypes.data, st.ctypes.data, C.byref(p), poses.ctypes.data, rec.ctypes.data,
                                      pairs.ctypes.data, F * 32, C.byref(n), L.MEM_HOST)
        return rc, poses, rec, pairs, n.value

    p = L.ChainParamsStruct()
    ctx._lib.o3dr_chain_default_params(C.byref(p))
    assert (p.dist_nearby, p.range_width, p.min_matches, p.ratio, p.max_distance) == (2.0, 8, 30, 0.5, 40) and p.max_rms == np.inf
    bad_status = ref["status"].copy()
    bad_status[1] = 5
    for kw in (dict(n_fixed=F + 1), dict(range_width=0), dict(range_width=33), dict(min_matches=2), dict(dist_nearby=-1.0),
               dict(dist_nearby=float("nan")), dict(dist_nearby=float("inf")), dict(max_rms=0.0), dict(n_fixed=2, status=bad_status),
               dict(n_fixed=-1)):
        rc, poses, rec, pairs, n = call(**kw)
        assert rc == L.ERR_INVALID_ARG, kw
        assert not poses.any() and not rec.view(np.uint8).any() and not pairs.any() and n == 0, kw
    rc, poses, rec, pairs, n = call(n_fixed=2, dist_nearby=DIST)
    assert rc == 0 and n == len(ref["pairs"]) - 1 and rec["status"].tolist() == ref["status"].tolist()
    with pytest.raises(L.O3drError):
        run(ctx, w, range_width=0)


@pytest.mark.gpu
def test_track_frames_equals_the_three_calls(ctx, frame_1248):
    """Three crops of one frame, each a few pixels further along: trackFrames = findFeatures, keypoints3D(poses=None),
    poseChain, byte for byte."""
    disp, bgr = frame_1248
    img = np.stack([np.ascontiguousarray(bgr[250:506, 500 + 6 * k:820 + 6 * k]) for k in range(3)])
    dsp = np.stack([np.ascontiguousarray(disp[250:506, 500 + 6 * k:820 + 6 * k]) for k in range(3)])
    prior = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1))
    prior[:, 0, 3] = [0.0, 0.1, 0.2]
    kw = dict(n_features=400, n_levels=3)
    poses, rec, (xy, off) = ctx.trackFrames(img, dsp, prior, min_matches=10, **kw)
    _, xy2, desc, off2 = ctx.findFeatures(img, **kw)
    kp3 = ctx.keypoints3D(dsp, [xy2[off2[f]:off2[f + 1]] for f in range(3)], poses=None)
    poses2, rec2 = ctx.poseChain(desc, off2, kp3, prior, min_matches=10)
    assert len(xy) > 100 and xy.tobytes() == xy2.tobytes() and np.array_equal(off, off2)
    assert poses.tobytes() == poses2.tobytes() and rec.tobytes() == rec2.tobytes()
    assert rec["status"][0] == R.ANCHOR and rec["n_pairs"].tolist() == [0, 1, 2]
