"""Pins tests/multiview_reference.py, the numpy statement of the multi-view filter contract (include/o3dr.h "multi-view
filter"), against facts that do not come from itself: the identities of the homographies, np.linalg.inv, exactly consistent
views of a plane, planted blobs, a brute-force neighbour sort.  CPU only."""
import numpy as np
import pytest

import multiview_reference as R
from online_3d_reconstruction_amd import synth

ROWS, COLS = 67, 131


def _exact_poses():
    """poses whose rotation is orthonormal exactly (signed permutations): the rigid inverse is then the inverse"""
    rots = [np.eye(3), [[0, 1, 0], [1, 0, 0], [0, 0, -1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[-1, 0, 0], [0, 1, 0], [0, 0, -1]]]
    rng = np.random.default_rng(5)
    poses = np.zeros((len(rots), 4, 4), np.float32)
    for f, r in enumerate(rots):
        poses[f, :3, :3] = r
        poses[f, :3, 3] = rng.uniform(-30, 30, 3)
        poses[f, 3, 3] = 1
    return poses


def _float_poses():
    return R.plane_poses(np.random.default_rng(6), 4, synth.make_pose(3))


def test_adjugate_inverse_is_the_inverse():
    Q = synth.camera_Q(ROWS, COLS)
    inv, det = R.adjugate_inverse(R._f64(Q))
    assert np.allclose(np.array(inv), np.linalg.inv(Q), rtol=1e-13, atol=0)
    assert np.isclose(det, np.linalg.det(Q), rtol=1e-13)
    rng = np.random.default_rng(1)
    for _ in range(20):
        M = rng.normal(size=(4, 4))
        inv, det = R.adjugate_inverse(R._f64(M))
        assert np.allclose(np.array(inv) @ M, np.eye(4), atol=1e-9 * max(1.0, np.linalg.cond(M)))
    with pytest.raises(ValueError):
        R.adjugate_inverse(R._f64(np.zeros((4, 4))))


def test_homography_of_a_frame_onto_itself_is_the_identity():
    """within 1e-12 where the pose's rotation is orthonormal exactly.  A float pose's rotation is orthonormal to about 1e-7
    only, the contract accepts that, and H_ii is then the identity up to that defect carried through Q: the bound is
    |Q^-1| |E - I| |Q| with E = T^-1 T taken from the pose itself, plus the rounding of the products."""
    Q = synth.camera_Q(ROWS, COLS)
    for T in _exact_poses():
        assert np.abs(R.homography(Q, T, T) - np.eye(4)).max() <= 1e-12
    Qinv = np.linalg.inv(Q)
    for T in _float_poses():
        T64 = T.astype(np.float64)
        E = np.array(R.rigid_inverse(R._f64(T64))) @ T64
        defect = np.abs(E - np.eye(4))
        assert 0 < defect.max() < 1e-5
        bound = np.abs(Qinv) @ defect @ np.abs(Q) + 1e-12
        assert (np.abs(R.homography(Q, T, T) - np.eye(4)) <= bound).all()


def test_homographies_there_and_back_are_the_identity():
    Q = synth.camera_Q(ROWS, COLS)
    poses = _exact_poses()
    for i in range(len(poses)):
        for j in range(len(poses)):
            P = R.homography(Q, poses[i], poses[j]) @ R.homography(Q, poses[j], poses[i])
            assert np.abs(P - np.eye(4)).max() <= 1e-9, (i, j)


def test_homography_carries_a_world_point_between_the_frames():
    """(x, y, d) of frame i and H_ij (x, y, d, 1) of frame j are the same world point, by plain numpy"""
    Q = synth.camera_Q(ROWS, COLS)
    poses = _float_poses().astype(np.float64)
    v = np.array([40.0, 20.0, 108.0, 1.0])
    H = R.homography(Q, poses[0], poses[1])
    w = H @ v
    Xi, Xj = poses[0] @ Q @ v, poses[1] @ Q @ (w / w[3])
    assert np.allclose(Xi[:3] / Xi[3], Xj[:3] / Xj[3], atol=1e-4)


@pytest.fixture(scope="module")
def plane():
    disp, Q, poses, real = R.plane_scene(ROWS, COLS, 4, seed=0)
    return disp, Q, poses, real, R.nearby_frames(poses, 3)


def _tests_inside(disp, Q, poses, nb, tolerance=1.0):
    """per pixel: the neighbour tests that are neither outside nor hole"""
    H = R.homographies(Q, poses, nb)
    n = np.zeros(disp.shape, np.int64)
    for i in range(len(disp)):
        for k, j in enumerate(nb[i]):
            if j >= 0:
                n[i] += R.classify(disp, i, int(j), H[i, k], tolerance) >= R.SUPPORT
    return n


def test_consistent_views_of_a_plane_support_each_other(plane):
    """uint8 rounding puts each side within half a level of the plane, hence tolerance 1; the neighbour's pixel is also up to
    half a pixel off the landing point, which on this slope (7 levels over the image) adds 0.03 at most: this scene's largest
    |e - dp| is 0.98"""
    disp, Q, poses, real, nb = plane
    assert all(f.max() - f.min() >= 6 for f in real), "the plane must span at least 6 levels in every frame"
    assert (disp != 0).all() and np.abs(poses[1:, :3, 3] - poses[0, :3, 3]).max() <= 0.16
    out, support, violations, infos = R.multiview_filter(disp, Q, poses, nb, tolerance=1.0)
    n = _tests_inside(disp, Q, poses, nb)
    seen = n > 0
    assert seen.mean() > 0.5
    assert (violations == 0).all()
    assert np.array_equal(support[seen], n[seen])
    assert np.array_equal(out[seen], disp[seen])
    assert sum(i.n_violation + i.n_occluded for i in infos) == 0 and sum(i.n_outside for i in infos) > 0


def test_planted_blobs_are_removed(plane):
    disp0, Q, poses, _, nb = plane
    disp = disp0.copy()
    near, far = (slice(30, 35), slice(60, 65)), (slice(12, 17), slice(90, 95))
    disp[1][near] += 10
    disp[2][far] -= 10
    planted = np.zeros(disp.shape, bool)
    planted[1][near] = planted[2][far] = True
    out, support, violations, infos = R.multiview_filter(disp, Q, poses, nb)
    n = _tests_inside(disp, Q, poses, nb)
    assert (n[planted] >= 2).all()
    assert (support[1][near] == 0).all() and np.array_equal(violations[1][near], n[1][near])
    assert (support[2][far] == 0).all() and (violations[2][far] == 0).all()
    assert (out[planted] == 0).all()
    assert not (out[~planted & (support >= 2)] == 0).any()
    assert infos[1].n_no_support >= 25 and infos[2].n_no_support >= 25


def test_keep_rules():
    disp0, Q, poses, _ = R.plane_scene(ROWS, COLS, 4, seed=0)
    disp = disp0.copy()
    disp[2, 12:17, 90:95] -= 10  # the other frames' pixels that land on it see something farther through their point
    nb = R.nearby_frames(poses, 3)
    _, s, v, _ = R.multiview_filter(disp, Q, poses, nb)
    hit = (v > 0) & (s > 0)
    assert hit.any()
    strict = R.multiview_filter(disp, Q, poses, nb, max_violations=0)[0]
    loose = R.multiview_filter(disp, Q, poses, nb, max_violations=1)[0]
    assert (strict[hit] == 0).all() and np.array_equal(loose[hit], disp[hit])
    alone = R.multiview_filter(disp, Q, poses, np.full((4, 3), -1, np.int32), min_support=0)
    assert not alone[0].any() and alone[3][0].n_violated == alone[3][0].n_valid  # 0 < 0 fails the majority rule
    kept = R.multiview_filter(disp, Q, poses, np.full((4, 3), -1, np.int32), min_support=0, max_violations=0)
    assert np.array_equal(kept[0], disp)


def test_nearby_frames_against_a_brute_force_sort():
    rng = np.random.default_rng(2)
    poses = np.tile(np.eye(4, dtype=np.float32), (9, 1, 1))
    poses[:, :3, 3] = rng.uniform(-5, 5, (9, 3)).astype(np.float32)
    poses[0, :3, 3] = [1, 2, 3]
    poses[4, :3, 3] = poses[0, :3, 3] + np.float32([3, 0, 0])  # frames 4 and 7 at exactly one distance from frame 0
    poses[7, :3, 3] = poses[0, :3, 3] - np.float32([3, 0, 0])
    pos = poses[:, :3, 3].astype(np.float64)
    for k, lim in ((3, np.inf), (8, np.inf), (12, np.inf), (8, 4.0), (2, 0.0)):
        got = R.nearby_frames(poses, k, lim)
        assert got.shape == (9, k) and got.dtype == np.int32
        for i in range(9):
            d2 = ((pos - pos[i]) ** 2).sum(axis=1)
            order = [j for j in np.lexsort((np.arange(9), d2)) if j != i and d2[j] <= lim * lim][:k]
            assert list(got[i]) == order + [-1] * (k - len(order))
    full = list(R.nearby_frames(poses, 8)[0])
    assert full.index(4) + 1 == full.index(7)  # the tie goes to the lower index
    cut = R.nearby_frames(poses, 8, 4.0)
    assert (cut == -1).any() and (cut >= 0).any()
