"""Moving-least-squares smoothing and normals (o3dr_mls_smooth, Context.mlsSmooth, `pose --smooth_surface`).

The contract (include/o3dr.h, DESIGN.md "MLS") is restated here in numpy, batched over padded neighbour lists: neighbours
from a cKDTree ball query at r (1 + 1e-5) re-checked with the exact fp32 d2 <= r2, fp64 moments, np.linalg.eigh for the
normal and np.linalg.solve for the fit.  The restatement also reports every point's margin to each decision threshold
(the k limits, l1 / l2, the Cholesky pivot ratio) and its eigen gap (l1 - l0) / l2, so that comparisons can set aside the
points that sit on a threshold."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

POSE_BIN = os.path.join(ROOT, "online_3d_reconstruction_amd", "bin", "pose")
NONE, PLANE, POLY = 0, 1, 2


# ---- the contract in numpy ----------------------------------------------------------------------------------------------
def _pts(xyz, rgba=None):
    from online_3d_reconstruction_amd import POINT
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    p = np.zeros(len(xyz), POINT)
    p["x"], p["y"], p["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    p["rgba"] = np.arange(len(xyz), dtype=np.uint32) * np.uint32(2654435761) if rgba is None else rgba
    return p


def _xyz(p):
    return np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float32)


def _r2(r):
    return np.float32(np.float64(r) * np.float64(r))


def neighbours(xyz, r, rows=None):
    """padded neighbour lists -> (J (n, K) int64 with -1 padding, d2 (n, K) fp32, mask): exactly d2 <= r2.
    rows (a slice): the lists of those points only, neighbours still taken from the whole cloud"""
    from scipy.spatial import cKDTree
    xyz = np.asarray(xyz, np.float32)
    q = xyz if rows is None else xyz[rows]
    n = len(q)
    if n == 0:
        return np.zeros((0, 1), np.int64), np.zeros((0, 1), np.float32), np.zeros((0, 1), bool)
    lists = cKDTree(xyz.astype(np.float64)).query_ball_point(q.astype(np.float64), r * (1 + 1e-5))
    K = max(len(l) for l in lists)
    J = np.full((n, K), -1, np.int64)
    for i, l in enumerate(lists):
        J[i, :len(l)] = l
    P = xyz[np.maximum(J, 0)]
    dx, dy, dz = q[:, None, 0] - P[..., 0], q[:, None, 1] - P[..., 1], q[:, None, 2] - P[..., 2]
    d2 = (dx * dx + dy * dy) + dz * dz  # fp32, numpy does not fuse
    mask = (J >= 0) & (d2 <= _r2(r))
    return J, d2, mask


def mls_numpy(xyz, r, order=2, h=0.0, rows=None, chunk=None):
    """-> dict of out (n, 3) fp64, normal (n, 3), curvature, k, fit and the margins (k, ratio, pivot, gap).
    rows (a slice): the results of those points only (their neighbours are still taken from the whole cloud);
    chunk: the whole cloud, worked through in slices of `chunk` points (the padded lists of a large cloud do not fit at once)"""
    xyz = np.asarray(xyz, np.float32)
    if chunk is not None and rows is None and len(xyz) > chunk:
        parts = [mls_numpy(xyz, r, order, h, rows=slice(s, s + chunk)) for s in range(0, len(xyz), chunk)]
        return {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}
    n = len(xyz) if rows is None else len(xyz[rows])
    h = float(h) if h > 0 else float(r) * float(r)
    J, d2, mask = neighbours(xyz, r, rows)
    p = (xyz if rows is None else xyz[rows]).astype(np.float64)
    P = xyz.astype(np.float64)[np.maximum(J, 0)]
    k = mask.sum(1)
    E = np.where(mask[..., None], P - p[:, None], 0.0)
    kk = np.maximum(k, 1)[:, None]
    mean = E.sum(1) / kk
    Cv = np.einsum("nki,nkj->nij", E, E) / kk[..., None] - mean[:, :, None] * mean[:, None, :]
    lam, V = np.linalg.eigh(Cv)
    l0, l1, l2 = lam[:, 0], lam[:, 1], lam[:, 2]
    nrm = V[:, :, 0] / np.linalg.norm(V[:, :, 0], axis=1, keepdims=True)
    nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    flip = (nz < 0) | ((nz == 0) & ((ny < 0) | ((ny == 0) & (nx < 0))))
    nrm[flip] *= -1
    tr = l0 + l1 + l2
    curv = np.where(tr != 0, l0 / np.where(tr != 0, tr, 1), 0.0)
    fit = np.where((k < 3) | ~(l1 > 1e-12 * l2), NONE, PLANE)
    m = p + np.einsum("ni,ni->n", nrm, mean)[:, None] * nrm  # p - (n . (p - c)) n with p - c = -mean
    out, onrm = m.copy(), nrm.copy()
    with np.errstate(all="ignore"):
        ratio_margin = np.where(l2 > 0, l1 / np.where(l2 > 0, l2, 1) - 1e-12, -1.0)
    pivot_margin = np.full(n, np.inf)
    nc = (order + 1) * (order + 2) // 2
    if order >= 1:
        v = np.where((np.abs(nrm[:, 2]) <= 0.9)[:, None], np.stack([-nrm[:, 1], nrm[:, 0], np.zeros(n)], 1),
                     np.stack([np.zeros(n), -nrm[:, 2], nrm[:, 1]], 1))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        u = np.cross(nrm, v)
        E2 = P - m[:, None]
        U = np.einsum("nki,ni->nk", E2, u) / r
        Vv = np.einsum("nki,ni->nk", E2, v) / r
        F = np.einsum("nki,ni->nk", E2, nrm)
        W = np.where(mask, np.exp(-d2.astype(np.float64) / h), 0.0)
        mono = [(a, b) for a in range(order + 1) for b in range(order + 1 - a)]
        Phi = np.stack([U ** a * Vv ** b for a, b in mono], -1)
        M = np.einsum("nk,nki,nkj->nij", W, Phi, Phi)
        rhs = np.einsum("nk,nk,nki->ni", W, F, Phi)
        dmax = np.max(np.diagonal(M, axis1=1, axis2=2), axis=1)
        L = np.zeros_like(M)  # Cholesky without pivoting: the pivots
        piv = np.zeros((n, nc))
        for i in range(nc):
            for j in range(i + 1):
                s = M[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(1)
                if i == j:
                    piv[:, i] = s
                    L[:, i, i] = np.sqrt(np.maximum(s, 0))
                else:
                    with np.errstate(all="ignore"):
                        L[:, i, j] = np.where(L[:, j, j] > 0, s / np.where(L[:, j, j] > 0, L[:, j, j], 1), 0)
        with np.errstate(all="ignore"):
            pivot_margin = np.min(piv, 1) / np.where(dmax > 0, dmax, 1) - 1e-12
        ok = (fit == PLANE) & (k >= nc) & (pivot_margin > 0)
        coef = np.zeros((n, nc))
        if ok.any():
            coef[ok] = np.linalg.solve(M[ok], rhs[ok][..., None])[..., 0]
        ok &= np.isfinite(coef).all(1)
        fit = np.where(ok, POLY, fit)
        a0, av, au = coef[:, 0], coef[:, 1] / r, coef[:, order + 1] / r
        out = np.where(ok[:, None], m + a0[:, None] * nrm, m)
        tn = nrm - au[:, None] * u - av[:, None] * v
        tn /= np.linalg.norm(tn, axis=1, keepdims=True)
        onrm = np.where(ok[:, None], tn, nrm)
    none = fit == NONE
    out[none] = p[none]
    onrm[none] = np.nan
    curv = np.where(none, np.nan, curv)
    with np.errstate(all="ignore"):
        gap = (l1 - l0) / np.where(l2 > 0, l2, 1)
    k_margin = np.minimum(np.abs(k - 2.5), np.abs(k - (nc - 0.5)) if order >= 1 else np.inf)
    return dict(out=out, normal=onrm, curv=curv, k=k, fit=fit, k_margin=k_margin, ratio_margin=ratio_margin,
                pivot_margin=pivot_margin, gap=gap)


def _angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs(np.einsum("ni,ni->n", a, b)))


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def check_against_numpy(xyz, out, nrm, cnt, fit, r, order, h=0.0, rgba=None, chunk=None, decided_by_k=False):
    """the tolerances of the contract's test plan; -> the observed maxima and the number of points each comparison set aside
    (n_unsure: fit kind not compared, n_differ: fit kind differs there so nothing else is compared, n_small_gap: fitted
    but the normal is not compared).  decided_by_k: a point whose fit kind the (exactly compared) neighbour count
    already decides - k < 3, or k below the number of coefficients for the polynomial - is not set aside for an l1 / l2
    or a pivot that only looks threshold-adjacent because its matrix is singular by construction"""
    ref = mls_numpy(xyz, r, order, h, chunk=chunk)
    assert np.array_equal(cnt, ref["k"])
    # fit kinds: equal except where the point sits within 1e-9 of a decision threshold
    sure = (np.abs(ref["ratio_margin"]) >= 1e-9) & ((order == 0) | (np.abs(ref["pivot_margin"]) >= 1e-9) | (ref["fit"] == NONE))
    if decided_by_k:
        nc = (order + 1) * (order + 2) // 2
        sure = (ref["k"] < 3) | ((np.abs(ref["ratio_margin"]) >= 1e-9) & ((ref["k"] < nc) | sure))
    assert np.array_equal(fit[sure], ref["fit"][sure]), np.nonzero((fit != ref["fit"]) & sure)[0][:10]
    same = fit == ref["fit"]
    got = _xyz(out).astype(np.float64)
    err = np.abs(got - ref["out"])[same]
    tol = _ulp(ref["out"])[same] + 1e-9
    assert (err <= tol).all(), (err / tol).max()
    if rgba is not None:
        assert np.array_equal(out["rgba"], rgba)
    fitted = same & (ref["fit"] != NONE)
    good = fitted & (ref["gap"] >= 1e-4)
    ang = _angle(nrm[good, :3], ref["normal"][good])
    assert (ang <= 1e-6).all(), ang.max()
    assert np.allclose(np.linalg.norm(nrm[fitted, :3].astype(np.float64), axis=1), 1.0, atol=1e-6)
    cerr = np.abs(nrm[fitted, 3].astype(np.float64) - ref["curv"][fitted])
    assert (cerr <= _ulp(ref["curv"][fitted]) + 1e-9).all(), cerr.max()
    assert np.isnan(nrm[fit == NONE]).all()
    none = fit == NONE
    assert np.array_equal(_xyz(out)[none].view(np.uint32), np.asarray(xyz, np.float32)[none].view(np.uint32))
    return dict(xyz_ulps=float((err / _ulp(ref["out"])[same]).max()) if err.size else 0.0,
                normal_rad=float(ang.max()) if ang.size else 0.0, curv=float(cerr.max()) if cerr.size else 0.0,
                n=len(fit), n_unsure=int((~sure).sum()), n_differ=int((~same).sum()), n_small_gap=int((fitted & ~good).sum()))


def bundled_cloud():
    z = np.load(os.path.join(GOLDEN, "cloud_ply.npz"))
    v = z["vertices"]
    return np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float32)


def tilted_sphere_cap(n, seed, radius=1.0, cap=0.25):
    """n points on a sphere of `radius` about the origin within `cap` rad of a tilted pole -> (xyz fp32, pole)"""
    rng = np.random.default_rng(seed)
    ct = rng.uniform(np.cos(cap), 1.0, n)
    st, ph = np.sqrt(1 - ct * ct), rng.uniform(0, 2 * np.pi, n)
    d = np.stack([st * np.cos(ph), st * np.sin(ph), ct], 1)
    R = _rot(0.4, -0.3, 0.2)
    return (radius * d @ R.T).astype(np.float32), R[:, 2]


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def wavy_surface(n, seed):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n)
    z = 0.2 * np.sin(1.3 * x) * np.cos(0.9 * y) + 0.05 * x + rng.normal(0, 0.002, n)
    return np.stack([x, y, z], 1).astype(np.float32)


# ---- without a GPU ------------------------------------------------------------------------------------------------------
def test_mls_symbols_declared_exported_and_bound():
    from online_3d_reconstruction_amd import _lib
    L = C.CDLL(_lib.lib_path())
    bound = {n: r for n, r, _ in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "o3dr.h")).read()
    for name in ("o3dr_mls_smooth", "o3dr_mls_default_params"):
        assert hasattr(L, name) and name in bound and name in header
    for name in ("O3DR_MLS_NONE  0", "O3DR_MLS_PLANE 1", "O3DR_MLS_POLY  2"):
        assert name in header
    assert bound["o3dr_mls_smooth"] is C.c_int
    assert C.sizeof(_lib.MlsParamsStruct) == 24 and C.sizeof(_lib.MlsResultStruct) == 32


def test_mls_default_params():
    from online_3d_reconstruction_amd import _lib
    L = _lib.load_library()
    p = _lib.MlsParamsStruct(3.0, 7, 5.0)
    L.o3dr_mls_default_params(C.byref(p))
    assert (p.search_radius, p.polynomial_order, p.sqr_gauss_param) == (0.0, 2, 0.0)


def test_mls_rejects_a_null_ctx_without_a_gpu():
    from online_3d_reconstruction_amd import _lib
    L = _lib.load_library()
    pts = _pts(np.ones((4, 3)))
    out = _pts(np.full((4, 3), 9.0))
    nrm = np.full((4, 4), 5.0, np.float32)
    cnt = np.full(4, 7, np.uint32)
    fit = np.full(4, 3, np.uint8)
    res = _lib.MlsResultStruct(1, 2, 3, 4)
    prm = _lib.MlsParamsStruct(0.1, 2, 0.0)
    rc = L.o3dr_mls_smooth(None, pts.ctypes.data, 4, C.byref(prm), out.ctypes.data, nrm.ctypes.data, cnt.ctypes.data,
                           fit.ctypes.data, C.byref(res), 0)
    assert rc == _lib.ERR_INVALID_ARG and L.o3dr_last_error().decode()
    assert not out.view(np.uint32).any() and not nrm.any() and not cnt.any() and not fit.any()
    assert (res.n_poly, res.n_plane, res.n_none, res.max_neighbors) == (0, 0, 0, 0)


def test_cli_smooth_surface_usage_errors(tmp_path):
    for argv in ([str(tmp_path / "a.ply")], [str(tmp_path / "a.ply"), "--mls_normals"], ["--search_radius", "0.1"], []):
        res = subprocess.run([POSE_BIN, "--smooth_surface"] + argv, capture_output=True, text=True, timeout=60)
        out = res.stdout + res.stderr
        assert res.returncode != 0 and "missing argument" in out and "unknown flag" not in out, (argv, out)
    usage = subprocess.run([POSE_BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--smooth_surface file.ply --search_radius r" in usage and "--mls_normals" in usage


def test_cli_search_radius_is_still_ignored_in_a_reconstruction_run(tmp_path):
    base = [POSE_BIN, "1", "2", "--data_dir", str(tmp_path / "nothing") + "/"]
    a = subprocess.run(base, capture_output=True, text=True, timeout=60)
    b = subprocess.run(base + ["--search_radius", "0.3"], capture_output=True, text=True, timeout=60)
    assert a.returncode == b.returncode != 0 and a.stdout == b.stdout and a.stderr == b.stderr
    assert "unknown flag" not in b.stdout and "missing argument" not in b.stdout


def test_numpy_restatement_on_a_plane_without_a_gpu():
    """the restatement itself: a tilted plane gives its normal and points on it"""
    rng = np.random.default_rng(0)
    xy = rng.uniform(-1, 1, (3000, 2))
    nrm = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    z = -(nrm[0] * xy[:, 0] + nrm[1] * xy[:, 1]) / nrm[2] + 0.1
    xyz = np.stack([xy[:, 0], xy[:, 1], z], 1).astype(np.float32)
    for order in (0, 1, 2):
        ref = mls_numpy(xyz, 0.15, order)
        assert (ref["fit"] == (POLY if order else PLANE)).all()
        assert _angle(ref["normal"], np.tile(nrm, (len(xyz), 1))).max() < 1e-6
        assert np.abs((ref["out"] - [0, 0, 0.1]) @ nrm).max() < 1e-6


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mls_ctx():
    import online_3d_reconstruction_amd as o3dr
    c = o3dr.Context(0)
    yield c
    c.close()


def _run(ctx, xyz, r, order=2, h=0.0, rgba=None):
    pts = _pts(xyz, rgba)
    out, nrm, cnt, fit, info = ctx.mlsSmooth(pts, r, order, h, return_normals=True, return_info=True)
    assert info.n_poly == (fit == POLY).sum() and info.n_plane == (fit == PLANE).sum() and info.n_none == (fit == NONE).sum()
    assert info.max_neighbors == (cnt.max() if len(cnt) else 0)
    return pts, out, nrm, cnt, fit, info


def _as_np(x):
    import torch
    if hasattr(torch, "uint32") and x.dtype == torch.uint32:
        x = x.view(torch.int32)
    return x.cpu().numpy()


@pytest.mark.gpu
def test_mls_exact_neighbour_counts(mls_ctx):
    rng = np.random.default_rng(1)
    cases = [((rng.random((20000, 3)) * [6, 5, 1]).astype(np.float32), 0.08)]
    base = (rng.random((2000, 3)) * [2, 2, 0.5]).astype(np.float32)
    cases.append((np.concatenate([base, base[::3], base[::5], np.repeat(base[:3], 4, 0)])[rng.permutation(2000 + 667 + 400 + 12)], 0.1))
    # pairs at exactly d2 == r2 in fp32 (kept) and one fp32 step beyond (dropped)
    g = np.stack(np.meshgrid(np.arange(30), np.arange(30), indexing="ij"), -1).reshape(-1, 2).astype(np.float32) * 0.5
    edge = np.concatenate([np.c_[g, np.zeros(len(g))], np.c_[g[:, 0] + np.float32(0.25), g[:, 1], np.zeros(len(g))]]).astype(np.float32)
    cases.append((edge, 0.25))
    col = np.stack([1.0 + 1e-4 * rng.random(6000), 2.0 + 1e-4 * rng.random(6000), rng.uniform(-50, 50, 6000)], 1).astype(np.float32)
    cases.append((col, 0.05))
    cases.append((bundled_cloud(), 0.1))
    cases.append((bundled_cloud(), 0.15))
    for xyz, r in cases:
        _, _, _, cnt, _, _ = _run(mls_ctx, xyz, r)
        _, _, mask = neighbours(xyz, r)
        assert np.array_equal(cnt, mask.sum(1)), (r, np.nonzero(cnt != mask.sum(1))[0][:10])
    # the d2 == r2 pairs are neighbours: every edge point has at least its partner
    _, _, _, cnt, _, _ = _run(mls_ctx, edge, 0.25)
    assert (cnt >= 2).all()
    # the bundled cloud at r = 0.1 has all three fit kinds
    _, _, _, cnt, fit, _ = _run(mls_ctx, bundled_cloud(), 0.1)
    assert (cnt < 3).any() and (fit == NONE).any() and (fit == PLANE).any() and (fit == POLY).any()
    for n in (0, 1, 2):
        xyz = np.arange(3 * n, dtype=np.float32).reshape(n, 3) * 0.01
        pts, out, nrm, cnt, fit, info = _run(mls_ctx, xyz, 1.0)
        assert len(out) == n and (cnt == n).all() and (fit == NONE).all() and info.n_none == n
        assert np.array_equal(out.view(np.uint32), pts.view(np.uint32)) and np.isnan(nrm).all()


@pytest.mark.gpu
@pytest.mark.parametrize("order,h", [(0, 0.0), (1, 0.0), (2, 0.0), (2, 0.004)])
def test_mls_agrees_with_numpy_on_the_bundled_cloud(mls_ctx, order, h):
    xyz = bundled_cloud()
    pts, out, nrm, cnt, fit, _ = _run(mls_ctx, xyz, 0.1, order, h)
    obs = check_against_numpy(xyz, out, nrm, cnt, fit, 0.1, order, h, rgba=pts["rgba"])
    print("bundled cloud, order", order, "h", h, obs)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [0, 1, 2])
def test_mls_agrees_with_numpy_on_random_surfaces(mls_ctx, order):
    xyz = wavy_surface(30000, 2 + order)
    pts, out, nrm, cnt, fit, _ = _run(mls_ctx, xyz, 0.06, order)
    obs = check_against_numpy(xyz, out, nrm, cnt, fit, 0.06, order, rgba=pts["rgba"])
    print("wavy surface, order", order, obs)
    sphere, _ = tilted_sphere_cap(8000, 5 + order)
    pts, out, nrm, cnt, fit, _ = _run(mls_ctx, sphere, 0.04, order, 0.0005)
    print("sphere cap, order", order, check_against_numpy(sphere, out, nrm, cnt, fit, 0.04, order, 0.0005, rgba=pts["rgba"]))


@pytest.mark.gpu
def test_mls_tilted_plane_all_orders(mls_ctx):
    rng = np.random.default_rng(7)
    xy = rng.uniform(-1, 1, (20000, 2))
    nrm = np.array([0.3, -0.2, 1.0]) / np.linalg.norm([0.3, -0.2, 1.0])
    z = -(nrm[0] * xy[:, 0] + nrm[1] * xy[:, 1]) / nrm[2] + 0.1
    xyz = np.stack([xy[:, 0], xy[:, 1], z], 1).astype(np.float32)
    for order in (0, 1, 2):
        _, out, nv, cnt, fit, _ = _run(mls_ctx, xyz, 0.1, order)
        assert (fit == (POLY if order else PLANE)).all()
        dist = np.abs((_xyz(out).astype(np.float64) - [0, 0, 0.1]) @ nrm)
        assert dist.max() < 1e-6, dist.max()
        assert _angle(nv[:, :3], np.tile(nrm, (len(xyz), 1))).max() < 1e-6
        assert (nv[:, 3] < 1e-9).all() and (nv[:, 2] > 0).all()


@pytest.mark.gpu
def test_mls_sphere_cap_order_two_fits_the_curvature(mls_ctx):
    xyz, pole = tilted_sphere_cap(20000, 8)
    r = 0.05
    interior = (xyz.astype(np.float64) @ pole) > np.cos(0.25 - 3 * r)
    res = {}
    for order in (0, 2):
        _, out, nv, _, fit, _ = _run(mls_ctx, xyz, r, order)
        o = _xyz(out).astype(np.float64)[interior]
        assert (fit[interior] == (POLY if order else PLANE)).all()
        res[order] = np.abs(np.linalg.norm(o, axis=1) - 1.0)
        if order == 2:
            ang = _angle(nv[interior, :3], o / np.linalg.norm(o, axis=1, keepdims=True))
            assert res[2].max() < 2e-6 and ang.max() < 2e-5, (res[2].max(), ang.max())
            print("sphere cap order 2: surface error", res[2].max(), "normal error", ang.max())
    assert res[0].mean() > 1e-4, res[0].mean()
    print("sphere cap order 0: mean bias", res[0].mean())


@pytest.mark.gpu
def test_mls_halves_the_noise_of_a_noisy_plane(mls_ctx):
    rng = np.random.default_rng(9)
    xy = rng.uniform(-2, 2, (40000, 2))
    xyz = np.stack([xy[:, 0], xy[:, 1], 0.5 + rng.normal(0, 0.005, len(xy))], 1).astype(np.float32)
    rms_in = np.sqrt(np.mean((xyz[:, 2].astype(np.float64) - 0.5) ** 2))
    inner = (np.abs(xy) < 1.8).all(1)
    for order in (0, 1, 2):
        _, out, _, _, fit, _ = _run(mls_ctx, xyz, 0.1, order)
        rms = np.sqrt(np.mean((out["z"][inner].astype(np.float64) - 0.5) ** 2))
        assert (fit != NONE).all() and rms <= 0.5 * rms_in, (order, rms, rms_in)
        print("noisy plane order", order, "rms", rms_in, "->", rms)


@pytest.mark.gpu
def test_mls_determinism_memory_kinds_in_place_and_permutation(mls_ctx):
    import torch
    xyz = wavy_surface(25000, 11)
    pts = _pts(xyz)
    a = mls_ctx.mlsSmooth(pts, 0.07, return_normals=True, return_info=True)
    b = mls_ctx.mlsSmooth(pts, 0.07, return_normals=True, return_info=True)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8))
    dev = torch.from_numpy(pts.view(np.int32).reshape(-1, 4).copy()).cuda()
    d = mls_ctx.mlsSmooth(dev, 0.07, return_normals=True, return_info=True)
    torch.cuda.synchronize()
    assert np.array_equal(_as_np(d[0]).reshape(-1).view(np.uint32), a[0].view(np.uint32))
    assert np.array_equal(_as_np(d[1]).view(np.uint32), a[1].view(np.uint32))
    assert np.array_equal(_as_np(d[2]).view(np.uint32), a[2]) and np.array_equal(_as_np(d[3]), a[3])
    inplace = dev.clone()
    mls_ctx.mlsSmooth(inplace, 0.07, out=inplace)
    torch.cuda.synchronize()
    assert np.array_equal(_as_np(inplace).reshape(-1).view(np.uint32), a[0].view(np.uint32))
    host_inplace = pts.copy()
    mls_ctx.mlsSmooth(host_inplace, 0.07, out=host_inplace)
    assert np.array_equal(host_inplace.view(np.uint32), a[0].view(np.uint32))
    perm = np.random.default_rng(12).permutation(len(xyz))
    p_out, _, p_cnt, p_fit, _ = mls_ctx.mlsSmooth(pts[perm], 0.07, return_normals=True, return_info=True)
    ref = mls_numpy(xyz, 0.07, 2)
    sure = (np.abs(ref["ratio_margin"]) >= 1e-9) & (np.abs(ref["pivot_margin"]) >= 1e-9)
    assert sure.all()  # nothing on a threshold here: the fit kinds compare exactly
    assert np.array_equal(p_cnt, a[2][perm]) and np.array_equal(p_fit, a[3][perm])
    err = np.abs(_xyz(p_out).astype(np.float64) - ref["out"][perm])
    assert (err <= _ulp(ref["out"][perm]) + 1e-9).all()
    # a cloudBigView() is smoothed where it lives
    mls_ctx.cloudBigReset()
    mls_ctx.cloudBigAppend(pts)
    v = mls_ctx.mlsSmooth(mls_ctx.cloudBigView(), 0.07)
    torch.cuda.synchronize()
    mls_ctx.cloudBigReset()
    assert np.array_equal(_as_np(v).reshape(-1).view(np.uint32), a[0].view(np.uint32))


@pytest.mark.gpu
def test_mls_fitted_only_keeps_the_fitted_points_in_order(mls_ctx):
    xyz = bundled_cloud()
    out, nrm, cnt, fit, info = mls_ctx.mlsSmooth(_pts(xyz), 0.1, return_normals=True, return_info=True)
    kept, knrm = mls_ctx.mlsSmooth(_pts(xyz), 0.1, return_normals=True, fitted_only=True)
    keep = fit != NONE
    assert len(kept) == info.n_poly + info.n_plane
    assert np.array_equal(kept.view(np.uint32), out[keep].view(np.uint32))
    assert np.array_equal(knrm.view(np.uint32), nrm[keep].view(np.uint32))


@pytest.mark.gpu
def test_mls_rejects_non_finite_points_and_bad_parameters(mls_ctx):
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import _lib
    xyz = wavy_surface(5000, 13)
    good = mls_ctx.mlsSmooth(_pts(xyz), 0.1)
    for pos in (0, 2500, 4999):
        for bad in (np.nan, np.inf, -np.inf):
            x = xyz.copy()
            x[pos, pos % 3] = bad
            pts = _pts(x)
            out = _pts(np.full((len(x), 3), 3.0))
            nrm = np.full((len(x), 4), 5.0, np.float32)
            cnt = np.full(len(x), 7, np.uint32)
            fit = np.full(len(x), 3, np.uint8)
            res = _lib.MlsResultStruct(1, 2, 3, 4)
            prm = _lib.MlsParamsStruct(0.1, 2, 0.0)
            rc = mls_ctx._lib.o3dr_mls_smooth(mls_ctx._h, pts.ctypes.data, len(x), C.byref(prm), out.ctypes.data, nrm.ctypes.data,
                                              cnt.ctypes.data, fit.ctypes.data, C.byref(res), 0)
            assert rc == _lib.ERR_INVALID_ARG
            assert not out.view(np.uint32).any() and not nrm.any() and not cnt.any() and not fit.any()
            assert (res.n_poly, res.n_plane, res.n_none, res.max_neighbors) == (0, 0, 0, 0)
    for kw in (dict(search_radius=0.0), dict(search_radius=-0.1), dict(search_radius=np.nan), dict(search_radius=np.inf),
               dict(search_radius=0.1, polynomial_order=3), dict(search_radius=0.1, polynomial_order=-1),
               dict(search_radius=0.1, sqr_gauss_param=-1.0), dict(search_radius=0.1, sqr_gauss_param=np.nan),
               dict(search_radius=0.1, sqr_gauss_param=np.inf)):
        with pytest.raises(o3dr.O3drError) as e:
            mls_ctx.mlsSmooth(_pts(xyz), **kw)
        assert e.value.code == _lib.ERR_INVALID_ARG
    again = mls_ctx.mlsSmooth(_pts(xyz), 0.1)  # the context is still usable
    assert np.array_equal(again.view(np.uint32), good.view(np.uint32))


@pytest.mark.gpu
def test_mls_leaves_the_accumulated_cloud_and_drops_a_pending_slice_table():
    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import synth
    disp, bgr = synth.make_frames(0, 3)
    poses = synth.make_poses(0, 3)
    prm = o3dr.Params(jump_pixels=4, voxel_size=0.05, sor_enable=False)
    other = wavy_surface(20000, 14)
    outs = []
    for with_mls in (False, True):
        with o3dr.Context(0, Q=synth.camera_Q(), params=prm) as c:
            c.accumulateFrames(disp, bgr, poses)
            if with_mls:
                _, _, _, info = c.mlsSmooth(_pts(other), 0.1, return_info=True)
                assert info.n_poly > 0
            outs.append(c.finalize())
    assert len(outs[0]) == len(outs[1]) and np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    with o3dr.Context(0, Q=synth.camera_Q(), params=prm) as c:
        c.accumulateFrames(disp, bgr, poses)
        counts = c.cloudBigSliceCountsDev(c.cloudBigHeaderDev(), 2).cpu().numpy()
        c.mlsSmooth(_pts(other), 0.1)
        with pytest.raises(o3dr.O3drError) as e:
            c.cloudBigPlaceSlices(0, counts[:2], 0, 0)
        assert e.value.code == -1
        counts = c.cloudBigSliceCountsDev(c.cloudBigHeaderDev(), 2).cpu().numpy()
        c.cloudBigPlaceSlices(0, counts[:2], 0, 0)  # without the MLS call in between it is accepted


def _read_any_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + 11
    head = raw[:end].decode()
    n = int(head.split("element vertex ")[1].split("\n")[0])
    fields = []
    for line in head.split("element vertex")[1].split("element camera")[0].splitlines()[1:]:
        _, t, name = line.split()
        fields.append((name, {"float": "<f4", "uchar": "u1"}[t]))
    dt = np.dtype(fields)
    assert len(raw) == end + n * dt.itemsize + 84
    return np.frombuffer(raw, dt, n, end)


@pytest.mark.gpu
def test_cli_smooth_surface_end_to_end(tmp_path, mls_ctx):
    z = np.load(os.path.join(GOLDEN, "cloud_ply.npz"))
    src = str(tmp_path / "cloud.ply")
    with open(src, "wb") as f:
        f.write(z["header"].tobytes() + z["vertices"].tobytes() + z["tail"].tobytes())
    v = z["vertices"]
    rgba = (np.uint32(255) << 24) | (v["r"].astype(np.uint32) << 16) | (v["g"].astype(np.uint32) << 8) | v["b"].astype(np.uint32)
    pts = _pts(np.stack([v["x"], v["y"], v["z"]], 1), rgba)
    kept, knrm = mls_ctx.mlsSmooth(pts, 0.1, 2, return_normals=True, fitted_only=True)
    res = subprocess.run([POSE_BIN, "--smooth_surface", src, "--search_radius", "0.1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert f"points in {len(pts)}" in res.stdout and f"fitted {len(kept)}" in res.stdout and "max neighbors" in res.stdout
    got = _read_any_ply(str(tmp_path / "smoothed_cloud.ply"))
    assert len(got) == len(kept)
    for ax in "xyz":
        assert np.array_equal(got[ax].view(np.uint32), kept[ax].view(np.uint32))
    assert np.array_equal(got["red"], (kept["rgba"] >> 16) & 255) and np.array_equal(got["blue"], kept["rgba"] & 255)
    plain = open(str(tmp_path / "smoothed_cloud.ply"), "rb").read()
    res = subprocess.run([POSE_BIN, "--smooth_surface", src, "--search_radius", "0.1", "--mls_normals"], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    got = _read_any_ply(str(tmp_path / "smoothed_cloud.ply"))
    assert [n for n in got.dtype.names] == ["x", "y", "z", "red", "green", "blue", "normal_x", "normal_y", "normal_z", "curvature"]
    for ax in "xyz":
        assert np.array_equal(got[ax].view(np.uint32), kept[ax].view(np.uint32))
    for k, name in enumerate(("normal_x", "normal_y", "normal_z", "curvature")):
        assert np.array_equal(got[name].view(np.uint32), knrm[:, k].view(np.uint32))
    # the normals file reads back by name: --downsample gives what it gives for the plain file
    with_n = str(tmp_path / "with_normals.ply")
    os.rename(str(tmp_path / "smoothed_cloud.ply"), with_n)
    with open(str(tmp_path / "plain.ply"), "wb") as f:
        f.write(plain)
    for name in ("with_normals.ply", "plain.ply"):
        r = subprocess.run([POSE_BIN, "--downsample", str(tmp_path / name), "--voxel_size", "0.2"], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
    a = open(str(tmp_path / "downsampled_with_normals.ply"), "rb").read()
    b = open(str(tmp_path / "downsampled_plain.ply"), "rb").read()
    assert a == b and len(a) > 1000
    r = subprocess.run([POSE_BIN, "--align_point_cloud", with_n, src, "--icp_max_iterations", "5"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ICP transformation (source -> target):" in r.stdout
    assert len(_read_any_ply(str(tmp_path / "aligned_with_normals.ply"))) == len(kept)
