"""Exact nearest neighbour and point-to-point ICP (o3dr_nearest_neighbors, o3dr_icp_align, `pose --align_point_cloud`).

The contract (include/o3dr.h, DESIGN.md "ICP") is restated here in numpy: a brute-force fp32 nearest neighbour with the
(d2, original index) key, the fp64 Kabsch solve and the loop with its stop reasons.  The larger ICP runs restate the loop
with a scipy cKDTree pre-filter whose candidates are re-checked with the exact fp32 key."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

POSE_BIN = os.path.join(ROOT, "online_3d_reconstruction_amd", "bin", "pose")
NONE = np.uint32(0xFFFFFFFF)
UNCHANGED_OR_SMALL = ("UNCHANGED", "SMALL_STEP")


# ---- the contract in numpy ----------------------------------------------------------------------------------------------
def _pts(xyz, rgba=None):
    from online_3d_reconstruction_amd import POINT
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = np.zeros(len(xyz), POINT)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["rgba"] = np.arange(len(xyz), dtype=np.uint32) if rgba is None else rgba
    return p


def _xyz(p):
    return np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float32)


def _r2(max_distance):
    return np.float32(np.float64(max_distance) * np.float64(max_distance))


def _d2(q, t):
    """fp32 ((0 + dx*dx) + dy*dy) + dz*dz of every query row against every target column (numpy does not fuse)"""
    dx = q[:, None, 0] - t[None, :, 0]
    dy = q[:, None, 1] - t[None, :, 1]
    dz = q[:, None, 2] - t[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def nn_brute(q, t, max_distance=np.inf, chunk=256):
    """the contract's nearest neighbour by brute force: key (fp32 d2, index), d2 <= r2, none -> 0xFFFFFFFF / inf"""
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    r2 = _r2(max_distance)
    idx = np.full(len(q), NONE, np.uint32)
    d2 = np.full(len(q), np.inf, np.float32)
    if len(t) == 0:
        return idx, d2
    for s in range(0, len(q), chunk):
        d = _d2(q[s:s + chunk], t)
        d = np.where(d <= r2, d, np.float32(np.inf))
        j = np.argmin(d, axis=1)  # first minimum = lowest index
        v = d[np.arange(len(j)), j]
        ok = (v <= r2) & np.isfinite(v) & np.all(np.isfinite(q[s:s + chunk]), axis=1)
        idx[s:s + chunk][ok] = j[ok]
        d2[s:s + chunk][ok] = v[ok]
    return idx, d2


def nn_tree(q, t, max_distance=np.inf, k=8, stats=None):
    """the same key with a cKDTree pre-filter (k candidates in fp64) re-checked in fp32; rows whose k-th candidate does not
    certify the result (possible ties just outside the k) fall back to brute force (stats, a dict: their number is added
    to stats["fallback"], the number of rows to stats["rows"])"""
    from scipy.spatial import cKDTree
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    r2 = _r2(max_distance)
    k = min(k, len(t))
    dist, cand = cKDTree(t.astype(np.float64)).query(q.astype(np.float64), k=k)
    dist, cand = dist.reshape(len(q), k), cand.reshape(len(q), k)
    tc = t[cand]
    dx, dy, dz = q[:, None, 0] - tc[..., 0], q[:, None, 1] - tc[..., 1], q[:, None, 2] - tc[..., 2]
    d = (dx * dx + dy * dy) + dz * dz
    key = np.where(d <= r2, d.view(np.uint32).astype(np.uint64) << np.uint64(32) | cand.astype(np.uint64), np.uint64(~0 & (2**64 - 1)))
    best = key.min(axis=1)
    found = best != np.uint64(2**64 - 1)
    idx = np.where(found, (best & np.uint64(0xFFFFFFFF)).astype(np.uint32), NONE)
    d2 = np.where(found, (best >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.inf))
    bd = np.where(found, d2.astype(np.float64), np.inf)
    # certified: the k-th candidate is clearly farther than the best (nothing outside the k can tie or beat it)
    unsure = ~(dist[:, -1] ** 2 > np.minimum(bd, np.float64(r2)) * (1 + 1e-5) + 1e-12) if k < len(t) else np.zeros(len(q), bool)
    if stats is not None:
        stats["fallback"] = stats.get("fallback", 0) + int(unsure.sum())
        stats["rows"] = stats.get("rows", 0) + len(q)
    if unsure.any():
        i2, d22 = nn_brute(q[unsure], t, max_distance)
        idx[unsure], d2[unsure] = i2, d22
    return idx, d2


def a2(T, p):
    """o3dr_transform_pt_cloud's arithmetic: ((m0*x + m1*y) + m2*z) + m3 in fp32"""
    m = np.asarray(T, np.float32).reshape(-1)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3] for r in range(3)], 1).astype(np.float32)


def kabsch(P, Q):
    """fp64 rigid solve P -> Q (no scale, det +1) -> (4x4, degenerate)"""
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    mp, mq = P.mean(0), Q.mean(0)
    H = (P - mp).T @ (Q - mq)
    U, S, Vt = np.linalg.svd(H)
    if not (S[0] > 0 and S[1] > 1e-12 * S[0]):
        return None, True
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    R = Vt.T @ D @ U.T
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, mq - R @ mp
    return T, False


def icp_numpy(src, tgt, T_init=None, max_iterations=10, max_correspondence_distance=np.inf, transformation_epsilon=0.0, nn=nn_tree):
    """the loop of the contract -> (T, fitness, n_correspondences, iterations, reason)"""
    T = np.eye(4) if T_init is None else np.asarray(T_init, np.float32).astype(np.float64).reshape(4, 4)
    if len(src) == 0 or len(tgt) == 0:
        return T, np.finfo(np.float64).max, 0, 0, "TOO_FEW"
    prev, it, reason, last = None, 0, None, None

    def one_pass():
        P = a2(T, src)
        idx, d2 = nn(P, tgt, max_correspondence_distance)
        return P, idx, d2

    while True:
        if it >= max_iterations:
            reason = "MAX_ITERATIONS"
            break
        P, idx, d2 = last = one_pass()
        if prev is not None and np.array_equal(idx, prev):
            reason = "UNCHANGED"
            break
        prev = idx
        m = idx != NONE
        if m.sum() < 3:
            reason = "TOO_FEW"
            break
        dT, degenerate = kabsch(P[m], tgt[idx[m]])
        if degenerate:
            reason = "DEGENERATE"
            break
        T = dT @ T
        last = None
        it += 1
        if np.abs(dT[:3] - np.eye(4)[:3]).max() <= transformation_epsilon:
            reason = "SMALL_STEP"
            break
    P, idx, d2 = last if last is not None else one_pass()
    m = idx != NONE
    fit = float(d2[m].astype(np.float64).mean()) if m.any() else np.finfo(np.float64).max
    return T, fit, int(m.sum()), it, reason


def rigid(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ \
        np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def rot_trans_err(T, G):
    R = T[:3, :3] @ G[:3, :3].T
    ang = float(np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1)))
    return ang, float(np.linalg.norm(T[:3, 3] - G[:3, 3]))


def bundled_cloud():
    v = np.load(os.path.join(GOLDEN, "cloud_ply.npz"))["vertices"]
    return np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32)


def synthetic_surface(n, seed):
    """a non-planar 2.5-D scene: a wavy ground, a ramp and a box-shaped building with walls"""
    rng = np.random.default_rng(seed)
    n1, n2 = n * 6 // 10, n * 2 // 10
    x, y = rng.uniform(0, 12, n1), rng.uniform(0, 10, n1)
    ground = np.stack([x, y, 0.4 * np.sin(0.9 * x) * np.cos(0.7 * y)], 1)
    u, w = rng.uniform(0, 3, n2), rng.uniform(0, 2.5, n2)
    wall = np.stack([2 + 0 * u + 0.002 * rng.standard_normal(n2), 2 + u, w], 1)
    roof = np.stack([rng.uniform(2, 5, n - n1 - n2), rng.uniform(2, 5, n - n1 - n2), 2.5 + 0.3 * rng.uniform(0, 1, n - n1 - n2)], 1)
    return np.concatenate([ground, wall, roof]).astype(np.float32)


def _torch_pts(p):
    import torch
    return torch.from_numpy(np.ascontiguousarray(p).view(np.int32).reshape(-1, 4)).cuda()


def _as_np(x):
    if type(x).__module__.startswith("torch"):
        import torch
        if x.dtype == torch.int32:
            return x.cpu().numpy().view(np.uint32)
        if hasattr(torch, "uint32") and x.dtype == torch.uint32:
            return x.view(torch.int32).cpu().numpy().view(np.uint32)
        return x.cpu().numpy()
    return x


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_icp_symbols_declared_exported_and_bound():
    from online_3d_reconstruction_amd import _lib
    L = C.CDLL(_lib.lib_path())
    bound = {n: r for n, r, _ in _lib.SYMBOLS}
    for name in ("o3dr_nearest_neighbors", "o3dr_icp_align", "o3dr_icp_default_params"):
        assert hasattr(L, name) and name in bound
        assert name in open(os.path.join(ROOT, "include", "o3dr.h")).read()
    assert bound["o3dr_nearest_neighbors"] is C.c_int and bound["o3dr_icp_align"] is C.c_int
    assert C.sizeof(_lib.IcpResultStruct) == 16 * 8 + 8 + 8 + 4 + 4 and C.sizeof(_lib.IcpParamsStruct) == 24


def test_icp_default_params_are_pcl_registration_defaults():
    from online_3d_reconstruction_amd import _lib
    L = _lib.load_library()
    p = _lib.IcpParamsStruct(-5, 1.0, 7.0)
    L.o3dr_icp_default_params(C.byref(p))
    assert (p.max_iterations, p.max_correspondence_distance, p.transformation_epsilon) == (10, float("inf"), 0.0)


def test_nn_and_icp_reject_null_ctx_and_bad_arguments_without_a_gpu():
    from online_3d_reconstruction_amd import _lib
    L = _lib.load_library()
    pts = _pts(np.ones((4, 3)))
    for n_q, n_t, with_out, mem in ((4, 4, True, 0), (-1, 4, True, 0), (4, -3, True, 0), (4, 4, False, 0), (4, 4, True, 7)):
        idx = np.full(4, 77, np.uint32)
        d2 = np.full(4, 5.0, np.float32)
        rc = L.o3dr_nearest_neighbors(None, pts.ctypes.data, n_q, pts.ctypes.data, n_t, float("inf"),
                                      idx.ctypes.data if with_out else None, d2.ctypes.data if with_out else None, mem)
        assert rc == _lib.ERR_INVALID_ARG and L.o3dr_last_error().decode()
        if with_out and mem == 0 and n_q > 0:
            assert not idx.any() and not d2.any()  # host outputs zeroed
    prm = _lib.IcpParamsStruct(10, float("inf"), 0.0)
    for n_s, n_t, with_res, mem in ((4, 4, True, 0), (-1, 4, True, 0), (4, -2, True, 1), (4, 4, False, 0), (4, 4, True, 9)):
        res = _lib.IcpResultStruct()
        for k in range(16):
            res.T[k] = 3.0
        res.fitness, res.n_correspondences, res.iterations, res.reason = 1.0, 9, 9, 9
        rc = L.o3dr_icp_align(None, pts.ctypes.data, n_s, pts.ctypes.data, n_t, None, C.byref(prm),
                              C.byref(res) if with_res else None, mem)
        assert rc == _lib.ERR_INVALID_ARG and L.o3dr_last_error().decode()
        if with_res:
            assert not any(res.T) and res.fitness == 0 and res.n_correspondences == 0 and res.iterations == 0 and res.reason == 0


def test_cli_align_point_cloud_reports_a_missing_argument(tmp_path):
    res = subprocess.run([POSE_BIN, "--align_point_cloud", str(tmp_path / "onlyone.ply")], capture_output=True, text=True, timeout=60)
    out = res.stdout + res.stderr
    assert res.returncode != 0 and "missing argument" in out and "unknown flag" not in out, out
    usage = subprocess.run([POSE_BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--align_point_cloud source.ply target.ply" in usage


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def icp_ctx():
    import online_3d_reconstruction_amd as o3dr
    c = o3dr.Context(0)
    yield c
    c.close()


def _check_nn(ctx, q, t, max_distance=np.inf, oracle=nn_brute):
    idx, d2 = ctx.nearestNeighbors(_pts(q), _pts(t), max_distance)
    ridx, rd2 = oracle(q, t, max_distance)
    assert np.array_equal(idx, ridx), np.nonzero(idx != ridx)[0][:10]
    assert np.array_equal(d2.view(np.uint32), rd2.view(np.uint32))
    return idx, d2


@pytest.mark.gpu
def test_nn_bit_exact_random_clouds_and_queries_outside_the_box(icp_ctx):
    rng = np.random.default_rng(1)
    t = (rng.random((30000, 3)) * [20, 15, 4] + [-3, 7, -1]).astype(np.float32)
    q = (rng.random((20000, 3)) * [40, 35, 12] + [-13, -3, -5]).astype(np.float32)  # about 3/4 outside the target's box
    _check_nn(icp_ctx, q, t, oracle=nn_tree)
    _check_nn(icp_ctx, q[:4000], t, max_distance=0.15)  # finite: some queries have no neighbour
    idx, d2 = icp_ctx.nearestNeighbors(_pts(q[:4000]), _pts(t), 0.15)
    assert (idx == NONE).any() and (idx != NONE).any() and np.isinf(d2[idx == NONE]).all()


@pytest.mark.gpu
def test_nn_duplicates_take_the_lowest_index_and_queries_on_target_points(icp_ctx):
    rng = np.random.default_rng(2)
    base = (rng.random((3000, 3)) * [5, 5, 1]).astype(np.float32)
    t = np.concatenate([base, base[::3], base[::7], base[:10]])  # duplicates at higher indices
    perm = rng.permutation(len(t))
    t = t[perm]
    q = np.concatenate([base[::2], (rng.random((2000, 3)) * [5, 5, 1]).astype(np.float32)])
    idx, d2 = _check_nn(icp_ctx, q, t)
    assert (d2[:1500] == 0).all()
    # every exact hit is the FIRST occurrence of that point in the target
    for i in range(0, 1500, 37):
        hits = np.nonzero((t == q[i]).all(1))[0]
        assert idx[i] == hits.min()


@pytest.mark.gpu
def test_nn_single_column_target_with_a_large_z_spread(icp_ctx):
    rng = np.random.default_rng(3)
    n = 6000
    t = np.stack([1.0 + 1e-4 * rng.random(n), 2.0 + 1e-4 * rng.random(n), rng.uniform(-50, 50, n)], 1).astype(np.float32)
    q = np.stack([rng.uniform(-2, 4, 3000), rng.uniform(-1, 5, 3000), rng.uniform(-60, 60, 3000)], 1).astype(np.float32)
    _check_nn(icp_ctx, q, t)
    _check_nn(icp_ctx, q, t[:1])


@pytest.mark.gpu
def test_nn_empty_clouds(icp_ctx):
    q = np.random.default_rng(4).random((100, 3)).astype(np.float32)
    idx, d2 = icp_ctx.nearestNeighbors(_pts(q), _pts(np.zeros((0, 3))))
    assert len(idx) == 100 and (idx == NONE).all() and np.isinf(d2).all()
    idx, d2 = icp_ctx.nearestNeighbors(_pts(np.zeros((0, 3))), _pts(q))
    assert len(idx) == 0 and len(d2) == 0


@pytest.mark.gpu
def test_nn_host_and_device_memory_agree(icp_ctx):
    rng = np.random.default_rng(5)
    t = (rng.random((20000, 3)) * [10, 10, 2]).astype(np.float32)
    q = (rng.random((8000, 3)) * [12, 12, 3] - 1).astype(np.float32)
    hi, hd = icp_ctx.nearestNeighbors(_pts(q), _pts(t), 0.3)
    di, dd = icp_ctx.nearestNeighbors(_torch_pts(_pts(q)), _torch_pts(_pts(t)), 0.3)
    assert np.array_equal(hi, _as_np(di)) and np.array_equal(hd.view(np.uint32), _as_np(dd).view(np.uint32))
    # a device pointer from o3dr_cloud_big_view as the target
    icp_ctx.cloudBigReset()
    icp_ctx.cloudBigAppend(_pts(t))
    vi, vd = icp_ctx.nearestNeighbors(_torch_pts(_pts(q)), icp_ctx.cloudBigView(), 0.3)
    icp_ctx.cloudBigReset()
    assert np.array_equal(hi, _as_np(vi)) and np.array_equal(hd.view(np.uint32), _as_np(vd).view(np.uint32))


@pytest.mark.gpu
def test_icp_first_step_is_exact(icp_ctx):
    rng = np.random.default_rng(6)
    tgt = synthetic_surface(5000, 7)
    src = tgt[rng.permutation(len(tgt))[:3000]] + rng.normal(0, 0.01, (3000, 3)).astype(np.float32)
    T0 = rigid(0.02, -0.01, 0.05, [0.1, -0.05, 0.02]).astype(np.float32)
    r = icp_ctx.icpAlign(_pts(src), _pts(tgt), T_init=T0, max_iterations=1)
    # the correspondences of the pass: A2(fp32(T_init), source) -> exact nearest neighbours
    P = a2(T0, src)
    assert np.array_equal(_xyz(icp_ctx.transformPtCloud(_pts(src), T0)).view(np.uint32), P.view(np.uint32))
    gidx, _ = icp_ctx.nearestNeighbors(_pts(P), _pts(tgt))
    ridx, _ = nn_brute(P, tgt)
    assert np.array_equal(gidx, ridx)
    dT, deg = kabsch(P, tgt[ridx])
    assert not deg and r.iterations == 1 and r.reason_name == "MAX_ITERATIONS"
    T1 = dT @ T0.astype(np.float64)
    assert np.abs(r.T - T1).max() < 1e-9, np.abs(r.T - T1).max()
    ref = icp_numpy(src, tgt, T0, max_iterations=1, nn=nn_brute)
    assert r.n_correspondences == ref[2] == len(src)
    assert abs(r.fitness - ref[1]) <= 1e-9 * ref[1]


@pytest.mark.gpu
def test_icp_recovers_a_known_transform_on_the_bundled_cloud(icp_ctx):
    """target: the reference's bundled cloud.ply (55 940 points, ~18 x 19 x 4 m); source: every 4th point moved by the
    inverse of G = 0.02 / -0.015 / 0.03 rad about x / y / z and (0.06, -0.04, 0.03) m; the numpy loop converges from there"""
    tgt = bundled_cloud()
    G = rigid(0.02, -0.015, 0.03, [0.06, -0.04, 0.03])
    src = a2(np.linalg.inv(G), tgt[::4])
    r = icp_ctx.icpAlign(_pts(src), _pts(tgt), max_iterations=60)
    ref = icp_numpy(src, tgt, max_iterations=60)
    ang, tr = rot_trans_err(r.T, G)
    assert ang < 1e-4 and tr < 1e-3, (ang, tr, r)
    assert r.reason_name in UNCHANGED_OR_SMALL and ref[4] in UNCHANGED_OR_SMALL
    assert abs(r.fitness - ref[1]) <= 1e-6 * max(ref[1], 1e-12) + 1e-12 and r.n_correspondences == ref[2]
    assert np.abs(r.T - ref[0]).max() < 1e-6


@pytest.mark.gpu
def test_icp_recovers_a_known_transform_on_a_synthetic_scene(icp_ctx):
    """a wavy ground with a building (20 000 points); source: every 3rd point moved by the inverse of
    G = 0.01 / 0.008 / -0.012 rad and (0.03, 0.02, -0.01) m"""
    tgt = synthetic_surface(20000, 8)
    G = rigid(0.01, 0.008, -0.012, [0.03, 0.02, -0.01])
    src = a2(np.linalg.inv(G), tgt[::3])
    r = icp_ctx.icpAlign(_pts(src), _pts(tgt), max_iterations=60)
    ref = icp_numpy(src, tgt, max_iterations=60)
    ang, tr = rot_trans_err(r.T, G)
    assert ang < 1e-4 and tr < 1e-3, (ang, tr, r)
    assert r.reason_name in UNCHANGED_OR_SMALL and ref[4] in UNCHANGED_OR_SMALL
    assert abs(r.fitness - ref[1]) <= 1e-6 * max(ref[1], 1e-12) + 1e-12


@pytest.mark.gpu
def test_icp_is_deterministic_and_memory_kind_independent(icp_ctx):
    rng = np.random.default_rng(9)
    tgt = synthetic_surface(30000, 10)
    src = a2(rigid(0.03, 0.0, 0.02, [0.1, 0.0, -0.05]), tgt[rng.permutation(len(tgt))[:12000]])
    a = icp_ctx.icpAlign(_pts(src), _pts(tgt), max_iterations=8, max_correspondence_distance=0.5)
    b = icp_ctx.icpAlign(_pts(src), _pts(tgt), max_iterations=8, max_correspondence_distance=0.5)
    d = icp_ctx.icpAlign(_torch_pts(_pts(src)), _torch_pts(_pts(tgt)), max_iterations=8, max_correspondence_distance=0.5)
    for x in (b, d):
        assert np.array_equal(a.T.view(np.uint64), x.T.view(np.uint64))
        assert np.float64(a.fitness).view(np.uint64) == np.float64(x.fitness).view(np.uint64)
        assert (a.n_correspondences, a.iterations, a.reason) == (x.n_correspondences, x.iterations, x.reason)


@pytest.mark.gpu
def test_icp_stop_reasons(icp_ctx):
    tgt = synthetic_surface(8000, 11)
    same = icp_ctx.icpAlign(_pts(tgt), _pts(tgt))
    assert same.reason_name in UNCHANGED_OR_SMALL and np.abs(same.T - np.eye(4)).max() < 1e-9
    assert same.n_correspondences == len(tgt) and same.fitness < 1e-20
    T0 = rigid(0.0, 0.0, 0.1, [100.0, 0.0, 0.0]).astype(np.float32)
    few = icp_ctx.icpAlign(_pts(tgt[:500]), _pts(tgt), T_init=T0, max_correspondence_distance=0.01)
    assert few.reason_name == "TOO_FEW" and few.n_correspondences == 0 and few.iterations == 0
    assert np.array_equal(few.T, T0.astype(np.float64))
    line = np.stack([np.linspace(0, 10, 400), np.full(400, 1.5), np.full(400, -2.0)], 1).astype(np.float32)
    deg = icp_ctx.icpAlign(_pts(line[::2] + np.float32([0.05, 0, 0])), _pts(line))
    assert deg.reason_name == "DEGENERATE" and deg.iterations == 0 and np.array_equal(deg.T, np.eye(4))
    far = rigid(0.3, -0.2, 0.4, [1.0, -0.7, 0.4]).astype(np.float32)
    mx = icp_ctx.icpAlign(_pts(tgt[::2]), _pts(tgt), T_init=far, max_iterations=2)
    assert mx.reason_name == "MAX_ITERATIONS" and mx.iterations == 2
    ref = icp_numpy(tgt[::2], tgt, far, max_iterations=2)
    assert np.abs(mx.T - ref[0]).max() < 1e-9 and mx.n_correspondences == ref[2]
    assert icp_ctx.icpAlign(_pts(np.zeros((0, 3))), _pts(tgt)).reason_name == "TOO_FEW"


@pytest.mark.gpu
def test_icp_leaves_the_accumulated_cloud_and_drops_a_pending_slice_table():
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import synth
    disp, bgr = synth.make_frames(0, 3)
    poses = synth.make_poses(0, 3)
    prm = o3dr.Params(jump_pixels=4, voxel_size=0.05, sor_enable=False)
    tgt = synthetic_surface(20000, 12)
    outs = []
    for with_icp in (False, True):
        with o3dr.Context(0, Q=synth.camera_Q(), params=prm) as c:
            c.accumulateFrames(disp, bgr, poses)
            if with_icp:
                r = c.icpAlign(_pts(tgt[::5]), _pts(tgt), max_iterations=3)
                assert r.n_correspondences > 0
            outs.append(c.finalize())
    assert len(outs[0]) == len(outs[1]) and np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    with o3dr.Context(0, Q=synth.camera_Q(), params=prm) as c:
        c.accumulateFrames(disp, bgr, poses)
        counts = c.cloudBigSliceCountsDev(c.cloudBigHeaderDev(), 2).cpu().numpy()
        c.icpAlign(_pts(tgt[::5]), _pts(tgt), max_iterations=1)
        with pytest.raises(o3dr.O3drError) as e:
            c.cloudBigPlaceSlices(0, counts[:2], 0, 0)
        assert e.value.code == -1
        counts = c.cloudBigSliceCountsDev(c.cloudBigHeaderDev(), 2).cpu().numpy()
        c.cloudBigPlaceSlices(0, counts[:2], 0, 0)  # without the ICP call in between it is accepted


def _write_ply(path, xyz):
    z = np.load(os.path.join(GOLDEN, "cloud_ply.npz"))
    header = z["header"].tobytes().replace(b"element vertex 55940", b"element vertex %d" % len(xyz))
    v = np.zeros(len(xyz), z["vertices"].dtype)
    v["x"], v["y"], v["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    v["r"], v["g"], v["b"] = 10, 20, 30
    with open(path, "wb") as f:
        f.write(header + v.tobytes() + z["tail"].tobytes())


@pytest.mark.gpu
def test_cli_align_point_cloud_end_to_end(tmp_path, icp_ctx):
    from test_cli_pose import _read_ply
    tgt = bundled_cloud()
    src = a2(np.linalg.inv(rigid(0.01, 0.0, -0.02, [0.05, 0.02, 0.0])), tgt[::5])
    sp, tp = str(tmp_path / "src.ply"), str(tmp_path / "tgt.ply")
    _write_ply(sp, src)
    _write_ply(tp, tgt)
    res = subprocess.run([POSE_BIN, "--align_point_cloud", sp, tp, "--icp_max_iterations", "30"], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    k = lines.index("ICP transformation (source -> target):")
    T = np.array([[float(v) for v in lines[k + 1 + r].split()] for r in range(4)])
    r = icp_ctx.icpAlign(_pts(src), _pts(tgt), max_iterations=30)
    assert np.array_equal(T, r.T)
    assert f"reason {r.reason_name}" in res.stdout and f"correspondences {r.n_correspondences}" in res.stdout
    got = _read_ply(str(tmp_path / "aligned_src.ply"))
    ref = icp_ctx.transformPtCloud(_pts(src), r.T.astype(np.float32))
    for ax in "xyz":
        assert np.array_equal(got[ax].view(np.uint32), ref[ax].view(np.uint32))
