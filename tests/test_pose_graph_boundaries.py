"""Pose-graph refinement (k_graph_moments, k_graph_solve; contract: include/o3dr.h "pose graph") past the sizes of
tests/test_pose_graph.py: more than 256 frames and more than 256 edges (every loop of the one-workgroup solve takes a second
and a third stride of kGraphThreads), pairs of three and four runs of kGraphRun rows with a used row alone in its run, both
orders of every pair with adjacencies of 46, a gradient that is exactly zero, and a diagonal block that is not positive
definite.  Every case compares res.flags with the reference's (assert_integers_equal).

The worlds carry 1 cm of noise on the 3-D keypoints: a frame, an edge or a row that is lost moves a pose by 1e-4 m or more,
or changes an integer.  The bound is test_pose_graph.py's "nm" rule, unchanged (assert_parity's docstring): the reference's
reversed-summation floor below 1e-9 m and the GPU within 1e-9 m of the reference.

test_worlds_reach_their_boundaries_without_a_gpu shows with the restatement alone (tests/pose_graph_reference.py) that every
world reaches what its GPU test is named for; it says nothing about the library.  Worlds and references are computed once
and shared, and nobody writes to them."""
import numpy as np
import pytest

import pose_chain_reference as R
import pose_graph_reference as G
from test_pose_graph import _CACHE, assert_integers_equal, assert_parity, input_T, pose_distance, ref_of, run

STRIDE = 256    # kGraphThreads: frames, edges and vector entries per stride of the solve
RUN = 256       # kGraphRun: query rows per run of the moments
GN, CG = 5, 48
POISON = 0x7FC00123  # a quiet NaN with a payload: a held frame's pose goes out byte for byte


def _case(name, make):
    """-> dict(w, ch, kw, ref, rev): a world, the chain outputs that go in, the call's keywords, the reference and its
    reverse=True run"""
    key = ("boundaries", name)
    if key not in _CACHE:
        w, ch, kw = make()
        _CACHE[key] = dict(w=w, ch=ch, kw=kw, ref=ref_of(w, ch, **kw), rev=ref_of(w, ch, reverse=True, **kw))
    return _CACHE[key]


def _floor(c):
    return pose_distance(c["ref"], c["ref"]["T"], c["rev"]["T"])


def _parity(ctx, c, label):
    return assert_parity(ctx, c["w"], c["ch"], label, rule="nm", refs=(c["ref"], c["rev"]), **c["kw"])


def _by_hand(w, pairs, match=None):
    """the poses are the priors (5 cm off), frame 0 the anchor, every other frame MATCHED"""
    F = len(w["offsets"]) - 1
    ch = dict(poses=w["prior"], status=np.array([R.ANCHOR] + [R.MATCHED] * (F - 1), np.int32), pairs=list(pairs))
    if match is not None:
        ch["match"] = match
    return ch


def _match(w, pairs):
    """{(i, j): (idx, good)} by brute force, once for the reference and its reverse run"""
    off, out = w["offsets"], {}
    for (i, j) in pairs:
        idx, dist = R.knn2_ref(w["desc"][off[i]:off[i + 1]], w["desc"][off[j]:off[j + 1]])
        out[(i, j)] = (idx, R.good_ref(dist))
    return out


# ---- the worlds -------------------------------------------------------------------------------------------------------------
def _world_300():
    """300 frames in a line, 40 of 60 landmarks each, the chain's own pair list; frame 290 rejected with a poisoned pose"""
    if ("boundaries", "w300") not in _CACHE:
        w = R.make_world(71, R.random_views(72, 300, 60, 40), 60, kp3_noise=0.01)
        ch = R.chain_ref(w["desc"], w["offsets"], w["kp3"], w["prior"], dist_nearby=1.2, min_matches=10)
        assert ch["status"].tolist() == [R.ANCHOR] + [R.MATCHED] * 299 and len(ch["pairs"]) == 597
        status = ch["status"].copy()
        status[290] = R.TOO_FEW
        poses = ch["poses"].copy()
        poses[290].view(np.uint32)[:] = POISON
        _CACHE[("boundaries", "w300")] = (w, dict(poses=poses, status=status, pairs=ch["pairs"], match=ch["match"]))
    return _CACHE[("boundaries", "w300")]


def frames_300():
    def make():
        w, ch = _world_300()
        fixed = np.zeros(300, bool)
        fixed[::8] = True
        return w, ch, dict(gn_iterations=GN, cg_iterations=CG, fixed=fixed, status=ch["status"])
    return _case("300 frames", make)


def frames_300_prior():
    def make():
        w, ch = _world_300()
        return w, ch, dict(gn_iterations=GN, cg_iterations=CG, status=ch["status"], prior_weight=50.0, prior_poses=w["prior"])
    return _case("300 frames, prior", make)


def edges_552():
    def make():
        w = R.make_world(81, R.random_views(82, 24, 60, 40), 60, step=0.05, kp3_noise=0.01)
        return w, _by_hand(w, [(i, j) for i in range(24) for j in range(24) if i != j]), dict(gn_iterations=GN, cg_iterations=CG)
    return _case("552 edges", make)


ROWS = [300, 255, 256, 257, 511, 512, 513, 600, 769]


def runs():
    def make():
        rng = np.random.default_rng(5)
        views = [np.concatenate([rng.choice(np.arange(1, 900), n - 1, replace=False), [0]]) for n in ROWS]
        w = R.make_world(91, views, 900, step=0.05, kp3_noise=0.01)
        pairs = [(i, j) for i in range(len(ROWS)) for j in range(i)]
        return w, _by_hand(w, pairs, _match(w, pairs)), dict(gn_iterations=GN, cg_iterations=CG)
    return _case("runs", make)


def zero_gradient():
    """three frames that see the same twelve points from the same place: every residual is exactly zero"""
    def make():
        rng = np.random.default_rng(7)
        lm = (rng.integers(-16, 17, (12, 3)) / 4.0 + np.array([0.0, 0.0, 8.0])).astype(np.float32)
        desc = rng.integers(0, 256, (12, 32), dtype=np.uint8)
        w = dict(desc=np.concatenate([desc] * 3), offsets=np.array([0, 12, 24, 36], np.int64), kp3=np.concatenate([lm] * 3))
        ch = dict(poses=np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (3, 1)),
                  status=np.array([R.ANCHOR, R.MATCHED, R.MATCHED], np.int32), pairs=[(1, 0), (2, 0), (2, 1)])
        return w, ch, dict(gn_iterations=GN, cg_iterations=CG)
    return _case("zero gradient", make)


A_POINT, B_POINT = (0.5, -0.25, 2.0), (0.75, -0.25, 2.5)


def singular():
    """frame 3's only edge has one used row: its diagonal block is diag_block(1, a, a a^T), every entry and every Cholesky
    step of which is exact for this a, and the pivot after the translation's three is exactly 0"""
    def make():
        w = R.make_world(41, R.random_views(42, 4, 100, 60), 100, step=0.05, kp3_noise=0.01)
        pairs = [(1, 0), (2, 0), (2, 1), (3, 2)]
        match = _match(w, pairs)
        idx, good = match[(3, 2)]
        row = int(np.nonzero(good)[0][0])
        off = w["offsets"]
        w["kp3"][off[3]:off[4]] = np.nan
        w["kp3"][off[3] + row] = A_POINT
        w["kp3"][off[2] + int(idx[row, 0])] = B_POINT
        return w, _by_hand(w, pairs, match), dict(gn_iterations=GN, cg_iterations=CG, min_pair_matches=1)
    return _case("singular", make)


def singular_not_an_edge():
    c = singular()
    key = ("boundaries", "singular, 2 matches")
    if key not in _CACHE:
        _CACHE[key] = ref_of(c["w"], c["ch"], **{**c["kw"], "min_pair_matches": 2})
    return _CACHE[key]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_worlds_reach_their_boundaries_without_a_gpu():
    # (a) 300 frames, 593 edges: second strides of the per-frame loops, second and third of the edge loop
    c = frames_300()
    ref, ch = c["ref"], c["ch"]
    assert (ref["n_edges"], ref["n_free"], ref["n_gauge"], ref["n_rejected"], ref["n_floating"], ref["flags"]) == (593, 261, 38, 1, 0, 0)
    assert ref["n_edges"] > 2 * STRIDE and _floor(c) < 1e-9
    assert ref["grad_after"] <= 1e-10 * ref["grad_before"]
    far = [f for f in ref["free"] if f >= STRIDE]
    moved = np.linalg.norm((ref["T"] - input_T(ch)).reshape(-1, 3, 4)[far][:, :, 3], axis=1)
    assert len(far) > 30 and moved.min() > 1e-3, moved.min()  # (a free frame lost in the second stride would stand still)
    held = np.nonzero(ref["role"] != G.FREE)[0]
    assert 290 in held and ref["role"][290] == G.REJECTED and (held >= STRIDE).sum() == 7
    assert (ch["poses"][290].view(np.uint32) == POISON).all() and (ref["poses"][290].view(np.uint32) == POISON).all()
    # (b) the same with a prior: nothing is held but the anchor, the solve is still on its way
    c = frames_300_prior()
    ref = c["ref"]
    assert (ref["n_free"], ref["n_gauge"], ref["n_rejected"], ref["n_edges"], ref["flags"]) == (298, 1, 1, 593, 0) and _floor(c) < 1e-9
    assert 1e-4 * ref["grad_before"] < ref["grad_after"] < ref["grad_before"]
    # (c) both orders of every pair: 552 edges over 24 frames
    c = edges_552()
    ref = c["ref"]
    assert ref["n_edges"] == 552 > 2 * STRIDE and (ref["degree"] == 46).all() and ref["n_used"].min() == 23
    assert ref["flags"] == 0 and _floor(c) < 1e-9
    assert all((j, i) in ref["pairs"] for (i, j) in ref["pairs"])
    # (d) runs: rows 256, 512 and 768 are used rows alone in their run
    c = runs()
    ref, w, ch = c["ref"], c["w"], c["ch"]
    off = w["offsets"]
    assert np.diff(off).tolist() == ROWS and ref["n_edges"] == 36 and ref["flags"] == 0 and _floor(c) < 1e-9
    for (i, j) in ch["pairs"]:
        idx, good = ch["match"][(i, j)]
        last = ROWS[i] - 1
        assert good[last] and np.isfinite(w["kp3"][off[i] + last]).all() and np.isfinite(w["kp3"][off[j] + int(idx[last, 0])]).all()
    queries = sorted({ROWS[i] for (i, _) in ch["pairs"]})
    assert [n for n in queries if n % RUN == 1] == [257, 513, 769] and {-(-n // RUN) for n in queries} == {1, 2, 3, 4}
    assert (ref["n_used"] > 50).all() and ref["edge"].all()
    # (e) a gradient that is exactly zero stops the solve, and nothing moves
    c = zero_gradient()
    ref, ch = c["ref"], c["ch"]
    assert ref["flags"] == G.FLAG_CG_STOPPED and ref["n_edges"] == 3 and ref["n_free"] == 2 and (ref["n_used"] == 12).all()
    assert ref["energy_before"] == ref["energy_after"] == ref["grad_before"] == ref["grad_after"] == ref["last_step"] == 0.0
    assert not ref["e_before"].any() and not ref["e_after"].any()
    assert ref["poses"].tobytes() == ch["poses"].tobytes() and _floor(c) == 0.0
    # (f) a block that is not positive definite holds its frame and sets the flag; the other frames move
    c = singular()
    ref, ch = c["ref"], c["ch"]
    assert ref["flags"] == G.FLAG_SINGULAR and ref["n_used"].tolist() == [34, 32, 37, 1] and ref["edge"].all()
    assert ref["role"].tolist() == [G.FIXED, G.FREE, G.FREE, G.FREE]
    a = np.array(A_POINT)
    assert G.invert6(G.diag_block(1.0, a, np.outer(a, a))) is None
    assert np.array_equal(ref["T"][3], input_T(ch)[3]) and np.abs(ref["T"][1:3] - input_T(ch)[1:3]).max() > 1e-3
    assert _floor(c) < 1e-9
    ref2 = singular_not_an_edge()
    assert ref2["edge"].tolist() == [1, 1, 1, 0] and ref2["role"].tolist() == [G.FIXED, G.FREE, G.FREE, G.FIXED] and ref2["flags"] == 0
    assert ref2["degree"][3] == 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_300_frames_and_593_edges(ctx):
    """Measured on the MI355X: see DESIGN.md "Pose-graph refinement"."""
    c = frames_300()
    _, frames, res, _, ref = _parity(ctx, c, "300 frames, 593 edges")
    assert res.n_free == 261 and res.n_edges == 593 and res.grad_after <= 1e-9 * res.grad_before
    assert frames["role"][290] == G.REJECTED


@pytest.mark.gpu
def test_300_frames_with_a_prior(ctx):
    """five steps do not reach the fixed point here: the case most exposed to the order of the sums"""
    c = frames_300_prior()
    _, _, res, _, _ = _parity(ctx, c, "300 frames, prior")
    assert res.n_free == 298 and res.n_gauge == 1


@pytest.mark.gpu
def test_552_edges_both_orders_of_every_pair(ctx):
    c = edges_552()
    _, frames, res, _, _ = _parity(ctx, c, "552 edges over 24 frames")
    assert res.n_edges == 552 and (frames["degree"] == 46).all()


@pytest.mark.gpu
def test_pairs_of_one_to_four_runs_and_a_row_alone_in_its_run(ctx):
    """n_used is compared exactly: one lost row fails"""
    c = runs()
    _, _, res, edges, _ = _parity(ctx, c, "runs")
    assert res.n_edges == 36 and (edges["n_used"] > 50).all()


@pytest.mark.gpu
def test_zero_gradient_stops_the_solve(ctx):
    c = zero_gradient()
    poses, frames, res, edges, ref = _parity(ctx, c, "zero gradient")
    assert res.flags == G.FLAG_CG_STOPPED
    assert res.energy_before == res.energy_after == res.grad_before == res.grad_after == res.last_step == 0.0
    assert not edges["energy_before"].any() and not edges["energy_after"].any()
    assert poses.tobytes() == c["ch"]["poses"].tobytes()
    assert np.array_equal(frames["T"], ref["T"])


@pytest.mark.gpu
def test_singular_block_holds_its_frame_and_sets_the_flag(ctx):
    c = singular()
    _, frames, res, _, ref = _parity(ctx, c, "singular block")
    assert res.flags == G.FLAG_SINGULAR and frames["role"][3] == G.FREE
    assert np.array_equal(frames["T"][3], input_T(c["ch"])[3])
    # one match more asked of a pair: (3, 2) is no edge, frame 3 is held by its role, and nothing is singular
    ref2 = singular_not_an_edge()
    _, frames, res, edges = run(ctx, c["w"], c["ch"], return_edges=True, **{**c["kw"], "min_pair_matches": 2})
    assert_integers_equal(frames, edges, res, ref2)
    assert res.flags == 0 and frames["role"][3] == G.FIXED
