"""Pose-graph refinement (o3dr_pose_graph_refine / Context.refinePoses; contract: include/o3dr.h "pose graph") against
tests/pose_graph_reference.py on small synthetic worlds (pose_chain_reference.make_world).

The loop world: 16 frames on a closed circle, 300 landmarks, 120 rows per frame, 2 cm of noise on every 3-D keypoint, the
static pair list at dist_nearby = 1.2 (the two frames before, and the first frames again for the last ones: the loop closes).
Pose tolerance on the GPU: four times the distance between the reference and its own run with every pair's rows summed in
reverse order, measured in the test (the pose chain tests' rule)."""
import ctypes as C

import numpy as np
import pytest

import pose_chain_reference as R
import pose_graph_reference as G
import ransac_rigid_reference as RR
from online_3d_reconstruction_amd import _lib as L

DIST = 1.2
GN, CG = 5, 48
_CACHE = {}


def loop_world(noise=0.02):
    key = ("loop", noise)
    if key not in _CACHE:
        w = R.make_world(21, R.random_views(22, 16, 300, 120), 300, poses=G.loop_poses(16), kp3_noise=noise)
        ch = R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=DIST)
        _CACHE[key] = (w, ch)
    return _CACHE[key]


def ref_of(w, ch, status=None, pairs=None, **kw):
    return G.refine_ref(w["desc"], w["offsets"], w["kp3"], ch["poses"], ch["status"] if status is None else status,
                        ch["pairs"] if pairs is None else pairs, match=ch.get("match"), **kw)


def loop_ref(reverse=False):
    key = ("loop_ref", reverse)
    if key not in _CACHE:
        w, ch = loop_world()
        _CACHE[key] = ref_of(w, ch, gn_iterations=GN, cg_iterations=CG, reverse=reverse)
    return _CACHE[key]


def run(ctx, w, ch, status=None, pairs=None, **kw):
    return ctx.refinePoses(w["desc"], w["offsets"], R.points(w["kp3"]), ch["poses"], ch["status"] if status is None else status,
                           np.asarray(ch["pairs"] if pairs is None else pairs, np.int32).reshape(-1, 2), **kw)


def direct(ref, T12, **kw):
    """energy and gradient norm at the fp64 poses T12 by the per-correspondence sums"""
    Rs, ts = G.state_of(T12)
    g = G.direct_gradient(ref["rows"], Rs, ts, ref["free"], **kw)
    return G.direct_energy(ref["rows"], Rs, ts, free=ref["free"], **kw), float(np.sqrt(sum(float(v @ v) for v in g.values())))


def input_T(ch):
    return np.stack([np.concatenate([a, b[:, None]], 1).reshape(12) for a, b in (G.orthonormal(p) for p in ch["poses"])])


def assert_integers_equal(frames, edges, res, ref):
    assert np.array_equal(frames["role"], ref["role"]), (frames["role"], ref["role"])
    assert np.array_equal(frames["degree"], ref["degree"])
    for k in ("n_good", "n_used", "edge"):
        assert np.array_equal(edges[k], ref[k]), (k, edges[k], ref[k])
    assert (edges["reserved"] == 0).all()
    assert (res.n_free, res.n_gauge, res.n_floating, res.n_rejected, res.n_edges, res.n_used) == \
        (ref["n_free"], ref["n_gauge"], ref["n_floating"], ref["n_rejected"], ref["n_edges"], ref["n_used_total"])
    assert res.flags == ref["flags"], (res.flags, ref["flags"])


def pose_distance(ref, Ta, Tb):
    """the largest entry difference of two [F, 12] fp64 pose sets over the reference's free frames; a held frame's T is its
    input pose widened, which has no rounding in it and may be NaN (a rejected frame's pose): those are equal, NaN to NaN"""
    free = ref["role"] == G.FREE
    assert np.array_equal(Ta[~free], Tb[~free], equal_nan=True)
    return float(np.abs(Ta[free] - Tb[free]).max()) if free.any() else 0.0


def assert_parity(ctx, w, ch, label, rule="floor", refs=None, **kw):
    """integers, flags, energies within 1e-9 relative, poses against the reference -> the GPU's outputs.  refs: the reference
    of this very call and its reverse=True run, where the caller has them already.
    rule "floor" (the loop world): within four times the reversed-summation floor.  rule "nm" (the boundary worlds, where
    the floor is a few ulps and some solves stop before their fixed point): within 1e-9 m.  What those tests look for - a
    row lost at a run boundary, an entry lost past a stride, a neighbour lost past a wave - moves a pose by the order of
    the keypoint noise, 1e-2 m, over the few tens of rows of an edge: 1e-4 m at the least; 1e-9 m is five orders below
    that, two below the 1e-7 m resolution of the fp32 poses, and six above one ulp of fp64.  rule None
    (test_role_rules_on_the_cpu's weakly held case, whose truncated CG is far from its fixed point): the integers, the
    input energy and the held poses are compared, and the energy must fall."""
    ref, rev = refs if refs is not None else (ref_of(w, ch, **kw), ref_of(w, ch, reverse=True, **kw))
    floor = pose_distance(ref, ref["T"], rev["T"])
    poses, frames, res, edges = run(ctx, w, ch, return_edges=True, **kw)
    assert_integers_equal(frames, edges, res, ref)
    diff = pose_distance(ref, frames["T"], ref["T"])
    print(f"pose graph, {label}: floor {floor:.3e}, gpu vs reference {diff:.3e}, energy {res.energy_before:.6g} -> "
          f"{res.energy_after:.6g}, gradient {res.grad_before:.3e} -> {res.grad_after:.3e}")
    assert abs(res.energy_before - ref["energy_before"]) <= 1e-9 * ref["energy_before"]
    assert np.allclose(edges["energy_before"], ref["e_before"], rtol=1e-9, atol=1e-9 * ref["energy_before"])
    if rule == "floor":
        assert 0 < floor < 1e-5
        assert diff <= 4 * floor
    elif rule == "nm":
        assert floor < 1e-9 and diff <= 1e-9
    else:
        assert res.energy_after < res.energy_before
    free = ref["role"] == G.FREE
    assert np.array_equal(poses.reshape(-1, 16)[free, :12], frames["T"][free].astype(np.float32))
    assert np.array_equal(poses.reshape(-1, 16)[~free].view(np.uint32), np.asarray(ch["poses"], np.float32)[~free].view(np.uint32))
    return poses, frames, res, edges, ref


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_energy_from_moments_equals_the_direct_sum():
    w, ch = loop_world()
    ref = loop_ref()
    assert ref["n_edges"] == len(ch["pairs"]) == 32 and ref["n_free"] == 15
    E0, _ = direct(ref, input_T(ch))
    E1, _ = direct(ref, ref["T"])
    assert abs(E0 - ref["energy_before"]) <= 1e-9 * E0
    assert abs(E1 - ref["energy_after"]) <= 1e-9 * E1
    k = 5
    i, j, a, b = ref["rows"][k]
    Rs, ts = G.state_of(input_T(ch))
    assert abs(G.direct_energy([ref["rows"][k]], Rs, ts) - ref["e_before"][k]) <= 1e-9 * ref["e_before"][k]


def test_invert6_restates_the_cholesky_inverse_on_the_cpu():
    """the reference's inverse is the library's Cholesky, pivot by pivot: on the loop world's positive definite blocks it is
    the inverse (1e-9 relative: cond ~ 1e4 x 2e-16), and on the block of one point a - whose rotation about a costs nothing,
    a (0; a) = 0 in exact arithmetic for this a - it reports "not positive definite" where np.linalg.inv returns numbers"""
    ref = loop_ref()
    blocks = {f: np.zeros((6, 6)) for f in ref["free"]}
    for (i, j, a, b) in ref["rows"]:
        for f, x in ((i, a), (j, b)):
            if f in blocks:
                blocks[f] += G.diag_block(float(len(x)), x.sum(0), x.T @ x)
    assert len(blocks) == 15
    for H in blocks.values():
        inv, want = G.invert6(H), np.linalg.inv(H)
        assert inv is not None and np.abs(inv - want).max() <= 1e-9 * np.abs(want).max()
    a = np.array([0.5, -0.25, 2.0])
    assert G.invert6(G.diag_block(1, a, np.outer(a, a))) is None


def test_noisy_loop_converges_on_the_cpu():
    w, ch = loop_world()
    ref = loop_ref()
    assert ch["status"].tolist() == [R.ANCHOR] + [R.MATCHED] * 15
    assert (15, 0) in ch["pairs"] and (14, 0) in ch["pairs"]  # the loop closes
    assert ref["energy_after"] < ref["energy_before"]
    assert ref["grad_after"] <= 1e-6 * ref["grad_before"]
    _, g1 = direct(ref, ref["T"])
    _, g0 = direct(ref, input_T(ch))
    assert abs(g0 - ref["grad_before"]) <= 1e-9 * g0 and g1 <= 1e-6 * g0
    floor = float(np.abs(ref["T"] - loop_ref(reverse=True)["T"]).max())
    assert 0 < floor < 1e-5


def test_noise_free_world_barely_moves():
    """Without noise the chain's residuals are fp32 roundings of kp3 (half an ulp of 10 m is 5e-7; the chain test bounds the
    rms by 1e-5).  A least-squares optimum over rows that are off by that much moves a pose by the order of those residuals,
    and the fp32 output adds 6e-8 |t| <= 5e-7: 1e-5 is an order above both."""
    w, ch = loop_world(noise=0.0)
    assert ch["rms"].max() < 1e-5
    ref = ref_of(w, ch, gn_iterations=GN, cg_iterations=CG)
    assert ref["n_free"] == 15
    assert np.abs(ref["poses"].astype(np.float64) - ch["poses"].astype(np.float64)).max() < 1e-5
    assert np.abs(ref["T"] - input_T(ch)).max() < 1e-5


def line_world():
    """eight frames in a line, consecutive pairs only (dist_nearby 0.6 < two steps)"""
    if "line" not in _CACHE:
        w = R.make_world(31, R.random_views(32, 8, 200, 100), 200, kp3_noise=0.01)
        ch = R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=0.6)
        assert ch["pairs"] == [(i, i - 1) for i in range(1, 8)] and ch["status"].tolist() == [R.ANCHOR] + [R.MATCHED] * 7
        _CACHE["line"] = (w, ch)
    return _CACHE["line"]


def test_role_rules_on_the_cpu():
    w, ch = line_world()
    fixed = np.zeros(8, bool)
    fixed[2] = True
    ref = ref_of(w, ch, fixed=fixed)
    assert ref["role"].tolist() == [G.FIXED, G.FREE, G.FIXED] + [G.FREE] * 5 and ref["n_gauge"] == 2
    assert np.array_equal(ref["poses"][[0, 2]], ch["poses"][[0, 2]]) and not np.array_equal(ref["poses"][1], ch["poses"][1])
    # a rejected frame: its pairs are no edges, and the frames behind it have no gauge frame
    status = ch["status"].copy()
    status[3] = R.TOO_FEW
    ref = ref_of(w, ch, status=status)
    assert ref["edge"].tolist() == [1, 1, 0, 0, 1, 1, 1] and ref["n_used"][2] == ref["n_used"][3] == 0 and ref["n_good"][2] > 0
    assert ref["role"].tolist() == [G.FIXED, G.FREE, G.FREE, G.REJECTED] + [G.FLOATING] * 4
    assert np.array_equal(ref["poses"][3:], ch["poses"][3:]) and ref["n_floating"] == 4 and ref["n_rejected"] == 1
    ref = ref_of(w, ch, status=status, prior_weight=50.0, prior_poses=w["prior"])
    assert ref["role"].tolist() == [G.FIXED, G.FREE, G.FREE, G.REJECTED] + [G.FREE] * 4
    # (translation priors on four frames that are nearly in a line hold the rotation about that line only weakly: the
    # truncated CG is still on its way after five iterations, so the energy is all that is asked of this case)
    assert ref["energy_after"] < ref["energy_before"] and ref["grad_after"] < ref["grad_before"]
    assert not np.array_equal(ref["poses"][5], ch["poses"][5])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_loop_world_equals_reference(ctx):
    """Measured on the MI355X for this world: see DESIGN.md "Pose-graph refinement"."""
    w, ch = loop_world()
    poses, frames, res, edges, ref = assert_parity(ctx, w, ch, "loop world", gn_iterations=GN, cg_iterations=CG)
    # the library's own numbers, recomputed from its output poses by the direct sums
    E0, g0 = direct(ref, input_T(ch))
    E1, g1 = direct(ref, frames["T"])
    assert E1 < E0 and g1 <= 1e-6 * g0
    assert abs(res.energy_after - E1) <= 1e-9 * E1 and res.energy_after < res.energy_before
    assert res.grad_after <= 1e-6 * res.grad_before and abs(res.grad_before - g0) <= 1e-9 * g0
    assert abs(edges["energy_after"].sum() - E1) <= 1e-9 * E1
    # and from the fp32 poses a caller gets: the energy still falls
    E32, _ = direct(ref, np.asarray(poses, np.float64).reshape(-1, 16)[:, :12])
    assert E32 < E0


@pytest.mark.gpu
def test_bit_identical_across_calls_memory_and_edges(ctx):
    import torch
    w, ch = loop_world()
    a = run(ctx, w, ch, return_edges=True)
    b = run(ctx, w, ch, return_edges=True)
    c = run(ctx, w, ch)
    d = ctx.refinePoses(torch.from_numpy(w["desc"]).cuda(), w["offsets"],
                        torch.from_numpy(R.points(w["kp3"]).view(np.int32).reshape(-1, 4)).cuda(), ch["poses"], ch["status"],
                        np.asarray(ch["pairs"], np.int32), return_edges=True)
    assert d[0].is_cuda
    for o in (b, c, (d[0].cpu().numpy(),) + d[1:]):
        assert o[0].tobytes() == a[0].tobytes() and o[1].tobytes() == a[1].tobytes() and o[2] == a[2]
        assert len(o) == 3 or o[3].tobytes() == a[3].tobytes()


@pytest.mark.gpu
def test_one_pair_call_equals_its_record_in_the_full_call(ctx):
    """An edge's moments are those of a call with that pair alone: everything in its record that is a function of the pair
    and the input poses (the counts, the flag, energy_before) is equal bit for bit.  energy_after is taken at the output
    poses, which a one-pair solve moves elsewhere; with every frame held nothing moves, and then the whole record is equal."""
    w, ch = loop_world()
    full = run(ctx, w, ch, return_edges=True)[3]
    held = run(ctx, w, ch, fixed=np.ones(16, bool), return_edges=True)[3]
    for f in ("n_good", "n_used", "edge", "energy_before"):
        assert held[f].tobytes() == full[f].tobytes(), f
    assert np.array_equal(held["energy_after"], held["energy_before"])
    for k in (0, 7, 31):
        one = run(ctx, w, ch, pairs=[ch["pairs"][k]], return_edges=True)[3]
        assert len(one) == 1 and one["edge"][0] == 1
        for f in ("n_good", "n_used", "edge", "reserved", "energy_before"):
            assert one[f][0].tobytes() == full[f][k].tobytes(), (k, f)
        one = run(ctx, w, ch, pairs=[ch["pairs"][k]], fixed=np.ones(16, bool), return_edges=True)[3]
        assert one[0].tobytes() == held[k].tobytes()


@pytest.mark.gpu
def test_query_frame_of_300_rows(ctx):
    """a pair's rows cross the 256-row run"""
    if "w300" not in _CACHE:
        w = R.make_world(41, R.random_views(42, 4, 400, 300), 400, kp3_noise=0.01)
        _CACHE["w300"] = (w, R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=DIST))
    w, ch = _CACHE["w300"]
    _, _, _, edges, ref = assert_parity(ctx, w, ch, "300 rows", rule="nm", gn_iterations=GN, cg_iterations=CG)
    assert all(np.nonzero(ch["match"][p][1])[0].max() >= 256 for p in ch["pairs"]) and (edges["n_used"] > 200).all()


@pytest.mark.gpu
def test_min_pair_matches_boundary(ctx):
    w, ch = loop_world()
    u = int(loop_ref()["n_used"].min())
    for m, n_edges in ((u, 32), (u + 1, 32 - int((loop_ref()["n_used"] == u).sum()))):
        ref = ref_of(w, ch, min_pair_matches=m)
        _, frames, res, edges = run(ctx, w, ch, min_pair_matches=m, return_edges=True)
        assert_integers_equal(frames, edges, res, ref)
        assert res.n_edges == n_edges and (edges["energy_before"][edges["edge"] == 0] == 0).all()


@pytest.mark.gpu
def test_48_frames_exceed_one_stride_of_the_solver(ctx):
    if "w48" not in _CACHE:
        w = R.make_world(51, R.random_views(52, 48, 60, 40), 60, kp3_noise=0.01)
        _CACHE["w48"] = (w, R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=DIST, min_matches=10))
    w, ch = _CACHE["w48"]
    assert (ch["status"][1:] == R.MATCHED).all() and 6 * 48 > 256
    assert_parity(ctx, w, ch, "48 frames", rule="nm", gn_iterations=GN, cg_iterations=CG)


@pytest.mark.gpu
def test_star_of_70_frames_around_one_anchor(ctx):
    """frame 0's adjacency is longer than a wave; the poses are the priors (5 cm off), the statuses set by hand"""
    if "star" not in _CACHE:
        w = R.make_world(61, R.random_views(62, 71, 60, 40), 60, step=0.05, kp3_noise=0.01)
        _CACHE["star"] = (w, dict(poses=w["prior"], status=np.array([R.ANCHOR] + [R.MATCHED] * 70, np.int32),
                                  pairs=[(k, 0) for k in range(1, 71)]))
    w, ch = _CACHE["star"]
    _, frames, res, _, _ = assert_parity(ctx, w, ch, "star", rule="nm", gn_iterations=GN, cg_iterations=4)
    assert frames["degree"][0] == 70 and res.n_free == 70 and res.energy_after < 0.1 * res.energy_before


@pytest.mark.gpu
def test_nothing_to_refine(ctx):
    w, ch = loop_world()
    same = lambda p: np.array_equal(p.reshape(-1, 16).view(np.uint32), ch["poses"].view(np.uint32))  # noqa: E731
    poses, frames, res, edges = run(ctx, w, ch, min_pair_matches=10000, return_edges=True)  # zero edges
    assert same(poses) and res.n_edges == res.n_free == 0 and res.energy_before == res.energy_after == 0.0
    assert (edges["edge"] == 0).all() and (edges["n_used"] > 30).all() and (frames["degree"] == 0).all()
    poses, frames, res = run(ctx, w, ch, fixed=np.ones(16, bool))  # zero free frames
    assert same(poses) and res.n_free == 0 and res.n_edges == 32 and res.n_gauge == 16
    assert res.energy_before == res.energy_after > 0 and res.grad_before == res.grad_after == 0.0
    assert abs(res.energy_before - loop_ref()["energy_before"]) <= 1e-9 * res.energy_before
    poses, frames, res = ctx.refinePoses(np.zeros((0, 32), np.uint8), np.zeros(1, np.int64), R.points(np.zeros((0, 3))),
                                         np.zeros((0, 16), np.float32), np.zeros(0, np.int32), np.zeros((0, 2), np.int32))
    assert poses.shape == (0, 4, 4) and len(frames) == 0 and res.n_edges == 0


@pytest.mark.gpu
def test_roles_on_the_gpu(ctx):
    w, ch = line_world()
    status = ch["status"].copy()
    status[3] = R.TOO_FEW
    fixed = np.zeros(8, bool)
    fixed[1] = True
    for n, kw in enumerate((dict(fixed=fixed), dict(), dict(prior_weight=50.0, prior_poses=w["prior"]))):
        _, frames, res, _, ref = assert_parity(ctx, w, ch, f"roles {n}", rule="nm" if n < 2 else None, status=status, **kw)
        assert res.n_floating == (4 if n < 2 else 0) and res.n_rejected == 1 and frames["role"][3] == G.REJECTED


@pytest.mark.gpu
def test_ransac_filter(ctx):
    """tests/test_pose_chain_robust.py's world: 20 % of every frame's 3-D keypoints are wrong"""
    if "rob" not in _CACHE:
        w = RR.corrupt_world(R.make_world(11, R.random_views(12, 8, 260, 150), 260), 0.2, 100)
        _CACHE["rob"] = (w, RR.robust_chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=DIST, ransac_threshold=0.05))
    w, ch = _CACHE["rob"]
    assert ch["gap"] > 1e-9
    ref = ref_of(w, ch, inlier=ch["inlier"])
    plain_ref = ref_of(w, ch)
    _, frames, res, edges = run(ctx, w, ch, ransac_threshold=0.05, return_edges=True)
    assert_integers_equal(frames, edges, res, ref)
    assert edges["n_used"].tolist() == [r["n_inliers"] for r in ch["ransac"]]
    _, frames0, res0, edges0 = run(ctx, w, ch, return_edges=True)
    assert_integers_equal(frames0, edges0, res0, plain_ref)
    assert res.n_used < res0.n_used and res.energy_after / res.n_used < res0.energy_after / res0.n_used


@pytest.mark.gpu
def test_pose_chain_refine_keyword(ctx):
    w, ch = loop_world()
    kw = dict(dist_nearby=DIST, return_pairs=True)
    pts = R.points(w["kp3"])
    poses, rec, pairs = ctx.poseChain(w["desc"], w["offsets"], pts, w["prior"], **kw)
    off = ctx.poseChain(w["desc"], w["offsets"], pts, w["prior"], refine=False, **kw)
    assert off[0].tobytes() == poses.tobytes() and off[1].tobytes() == rec.tobytes() and np.array_equal(off[2], pairs) and len(off) == 3
    want = ctx.refinePoses(w["desc"], w["offsets"], pts, poses, rec["status"], pairs, gn_iterations=3)
    got = ctx.poseChain(w["desc"], w["offsets"], pts, w["prior"], refine=True, refine_kw=dict(gn_iterations=3), **kw)
    assert len(got) == 4 and got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == rec.tobytes()
    assert np.array_equal(got[2], pairs) and got[3] == want[2] and got[3].n_free == 15
    assert not np.array_equal(got[0], poses)
    # history frames are held
    h = ctx.poseChain(w["desc"], w["offsets"], pts, w["prior"], n_fixed=6, poses_in=poses[:6], status_in=rec["status"][:6], refine=True,
                      dist_nearby=DIST)
    assert np.array_equal(h[0][:6], poses[:6]) and h[2].n_free == 10 and not np.array_equal(h[0][6:], poses[6:])


def raw_call(ctx, w, ch, pairs, prm, rp=None, prior=None, status=None):
    """o3dr_pose_graph_refine with every output pre-filled with 0x55 -> (code, poses, frames, edges, res bytes)"""
    F, P = len(ch["poses"]), len(pairs)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    status = np.ascontiguousarray(ch["status"] if status is None else status, np.int32)
    pts = R.points(w["kp3"])
    poses = np.frombuffer(bytes([0x55]) * (F * 64), np.float32).reshape(F, 16).copy()
    frames = np.frombuffer(bytes([0x55]) * (F * 104), L.REFINE_FRAME).copy()
    edges = np.frombuffer(bytes([0x55]) * (max(P, 1) * 32), L.REFINE_EDGE).copy()
    res = np.full(72, 0x55, np.uint8)
    pin = np.ascontiguousarray(ch["poses"], np.float32)
    code = ctx._lib.o3dr_pose_graph_refine(
        ctx._h, w["desc"].ctypes.data, w["offsets"].ctypes.data, pts.ctypes.data, F, pin.ctypes.data, status.ctypes.data, None,
        None if prior is None else np.ascontiguousarray(prior, np.float32).ctypes.data, pairs.ctypes.data, P,
        None if prm is None else C.byref(prm), None if rp is None else C.byref(rp), poses.ctypes.data, frames.ctypes.data,
        edges.ctypes.data, C.cast(res.ctypes.data, C.POINTER(L.RefineResultStruct)), L.MEM_HOST)
    return code, poses, frames, edges, res


@pytest.mark.gpu
def test_invalid_arguments(ctx):
    w, ch = loop_world()
    good = lambda **kw: L.RefineParamsStruct(**{**dict(prior_weight=0.0, gn_iterations=5, cg_iterations=32, min_pair_matches=3,  # noqa: E731
                                                       ratio=0.5, max_distance=40, reserved=0), **kw})
    pairs = np.asarray(ch["pairs"], np.int32)
    bad_status = ch["status"].copy()
    bad_status[4] = 5
    cases = [dict(prm=good(gn_iterations=0)), dict(prm=good(gn_iterations=65)), dict(prm=good(cg_iterations=0)),
             dict(prm=good(cg_iterations=1025)), dict(prm=good(min_pair_matches=0)), dict(prm=good(prior_weight=-1.0)),
             dict(prm=good(prior_weight=float("nan"))), dict(prm=good(prior_weight=float("inf"))), dict(prm=good(prior_weight=1.0)),
             dict(prm=good(ratio=0.0)), dict(prm=good(max_distance=258)),
             dict(prm=good(), rp=L.RansacParamsStruct(0.0, 0, 256, 0)), dict(prm=good(), rp=L.RansacParamsStruct(0.05, 0, 0, 0)),
             dict(prm=good(), pairs=np.vstack([pairs, [[16, 0]]])), dict(prm=good(), pairs=np.vstack([pairs, [[3, -1]]])),
             dict(prm=good(), pairs=np.vstack([pairs, [[3, 3]]])), dict(prm=good(), pairs=np.vstack([pairs, pairs[4:5]])),
             dict(prm=good(), status=bad_status)]
    for kw in cases:
        kw.setdefault("pairs", pairs)
        code, poses, frames, edges, res = raw_call(ctx, w, ch, **kw)
        assert code == L.ERR_INVALID_ARG, kw
        assert not poses.view(np.uint8).any() and not frames.view(np.uint8).any() and not edges.view(np.uint8).any() and not res.any()
    # (j, i) next to (i, j) is another pair, and the same call with good arguments succeeds and writes every output
    code, poses, frames, edges, res = raw_call(ctx, w, ch, pairs=np.vstack([pairs, pairs[4:5, ::-1]]), prm=good())
    assert code == L.OK and edges["edge"].all() and len(edges) == 33
    code, poses, frames, edges, res = raw_call(ctx, w, ch, pairs=pairs, prm=good(prior_weight=1.0), prior=w["prior"])
    assert code == L.OK and (frames["role"][1:] == G.FREE).all()
    code, poses2, frames2, edges2, res2 = raw_call(ctx, w, ch, pairs=pairs, prm=None)
    want = run(ctx, w, ch, return_edges=True)
    assert code == L.OK and poses2.tobytes() == want[0].tobytes() and frames2.tobytes() == want[1].tobytes() and edges2.tobytes() == want[3].tobytes()
    with pytest.raises(L.O3drError) as e:
        run(ctx, w, ch, gn_iterations=0)
    assert e.value.code == L.ERR_INVALID_ARG
