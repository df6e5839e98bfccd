"""Height-field surface mesh (o3dr_mesh_surface, Context.meshSurface, `pose --mesh_surface`).

The contract (include/o3dr.h, DESIGN.md "Surface mesh") is restated here in numpy: fp32 cells, the lowest-index point of
a cell as its vertex, quads in (cy, cx) order, the diagonal choice, the orientation and edge-length gates and the fp64
vertex normals, every component written out (numpy never fuses a multiply-add).  Every value is an integer, a comparison
or a correctly rounded operation in a fixed order, so the GPU must match the restatement bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

POSE_BIN = os.path.join(ROOT, "online_3d_reconstruction_amd", "bin", "pose")
ERR_INVALID_ARG, ERR_CAPACITY = -1, -4
F32 = np.float32


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


def orient(p, q, r):
    """(qx-px)*(ry-py) - (qy-py)*(rx-px) in fp64 from fp32 coordinates (rows of [.., 3] arrays)"""
    p, q, r = (np.asarray(a, np.float64) for a in (p, q, r))
    return (q[..., 0] - p[..., 0]) * (r[..., 1] - p[..., 1]) - (q[..., 1] - p[..., 1]) * (r[..., 0] - p[..., 0])


def d2(p, q):
    """((0 + dx*dx) + dy*dy) + dz*dz in fp32, d = q - p"""
    d = np.asarray(q, F32) - np.asarray(p, F32)
    return ((F32(0) + d[..., 0] * d[..., 0]) + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def mesh_numpy(xyz, cell_size, L, normals=False):
    """-> (tris int32 [T, 3], counts dict, normals [n, 3] float32 or None)"""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    n = len(xyz)
    inv = F32(1.0) / F32(cell_size)
    lf = F32(float(L) * float(L))
    cx = np.floor(xyz[:, 0] * inv).astype(np.int64)
    cy = np.floor(xyz[:, 1] * inv).astype(np.int64)
    order = np.lexsort((np.arange(n), cx, cy))  # (cy, cx) ascending, the lowest index first inside a cell
    head = np.ones(n, bool)
    head[1:] = (cx[order][1:] != cx[order][:-1]) | (cy[order][1:] != cy[order][:-1])
    vidx = order[head]  # the vertices in cell order
    V = len(vidx)
    vcx, vcy = cx[vidx], cy[vidx]
    P = xyz[vidx]
    counts = dict(n_vertices=V, n_shadowed=n - V, n_triangles=0, n_quads_full=0, n_rejected_orientation=0, n_rejected_length=0)
    nrm = np.full((n, 3), np.nan, F32) if normals else None
    if V == 0:
        return np.zeros((0, 3), np.int32), counts, nrm
    x0, y0 = vcx.min() - 1, vcy.min() - 1
    W = int(vcx.max() - x0) + 3
    vkey = (vcy - y0) * W + (vcx - x0)  # ascending

    def lookup(qx, qy):
        k = (qy - y0) * W + (qx - x0)
        j = np.clip(np.searchsorted(vkey, k), 0, V - 1)
        return np.where(vkey[j] == k, j, -1)

    # every quad with >= 3 corners has a or b occupied: the vertices' own quads and the ones to their left
    qk = np.unique(np.concatenate([vkey, vkey - 1]))
    qy, qx = qk // W + y0, qk % W + x0
    cor = np.stack([lookup(qx, qy), lookup(qx + 1, qy), lookup(qx + 1, qy + 1), lookup(qx, qy + 1)], 1)  # a b c d
    present = (cor >= 0).sum(1)
    cor = cor[present >= 3]
    full = (cor >= 0).all(1)
    counts["n_quads_full"] = int(full.sum())
    A, B, Cc, D = (P[np.maximum(cor[:, k], 0)] for k in range(4))
    ac_ok = (orient(A, B, Cc) > 0) & (orient(A, Cc, D) > 0)
    bd_ok = (orient(A, B, D) > 0) & (orient(B, Cc, D) > 0)
    bd = bd_ok & (~ac_ok | (d2(B, D) < d2(A, Cc)))
    a, b, c, d = (cor[:, k] for k in range(4))
    t0 = np.where(bd[:, None], np.stack([a, b, d], 1), np.stack([a, b, c], 1))
    t1 = np.where(bd[:, None], np.stack([b, c, d], 1), np.stack([a, c, d], 1))
    # three corners: the present ones in a b c d order
    missing = np.argmin(cor[~full] >= 0, 1)
    t0[~full] = np.take_along_axis(cor[~full], np.array([[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]])[missing], 1)
    cand = np.stack([t0, t1], 1)  # [Q, 2, 3]
    is_cand = np.stack([np.ones(len(cor), bool), full], 1)
    tp, tq, tr = (P[np.maximum(cand[..., k], 0)] for k in range(3))
    o_ok = orient(tp, tq, tr) > 0
    l_ok = (d2(tp, tq) <= lf) & (d2(tq, tr) <= lf) & (d2(tr, tp) <= lf)
    kept = is_cand & o_ok & l_ok
    counts["n_rejected_orientation"] = int((is_cand & ~o_ok).sum())
    counts["n_rejected_length"] = int((is_cand & o_ok & ~l_ok).sum())
    tv = cand[kept]  # vertex ordinals, emission order (row-major: quads ascending, then their triangles)
    counts["n_triangles"] = len(tv)
    if normals and len(tv):
        p, q, r = (P[tv[:, k]].astype(np.float64) for k in range(3))
        ex, ey, ez = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1], q[:, 2] - p[:, 2]
        fx, fy, fz = r[:, 0] - p[:, 0], r[:, 1] - p[:, 1], r[:, 2] - p[:, 2]
        fn = np.stack([ey * fz - ez * fy, ez * fx - ex * fz, ex * fy - ey * fx], 1)
        # a vertex's quads (cx-1,cy-1), (cx,cy-1), (cx-1,cy), (cx,cy) are in emission order: sum its triangles in that order
        owner = tv.reshape(-1)
        tri_of = np.repeat(np.arange(len(tv)), 3)
        srt = np.lexsort((tri_of, owner))
        owner, tri_of = owner[srt], tri_of[srt]
        first = np.searchsorted(owner, owner)
        rank = np.arange(len(owner)) - first
        slots = np.zeros((V, int(rank.max()) + 1, 3))
        slots[owner, rank] = fn[tri_of]
        s = np.zeros((V, 3))
        for k in range(slots.shape[1]):
            s = s + slots[:, k]
        has = np.zeros(V, bool)
        has[owner] = True
        ln = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        with np.errstate(invalid="ignore", divide="ignore"):
            vn = (s / ln[:, None]).astype(F32)
        nrm[vidx[has]] = vn[has]
    return vidx[tv].astype(np.int32).reshape(-1, 3), counts, nrm


def jittered_grid(k, m, cell=0.05, holes=0.0, seed=0, margin=1e-3, z_amp=0.2):
    """one point per cell of a k x m grid, at least `margin` cells inside it, a random fraction `holes` left empty"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(k), np.arange(m), indexing="xy")
    u = rng.uniform(margin, 1 - margin, (m, k, 2))
    x = ((gx + u[..., 0]) * cell).astype(F32).reshape(-1)
    y = ((gy + u[..., 1]) * cell).astype(F32).reshape(-1)
    z = (z_amp * np.sin(x * 3.0) * np.cos(y * 2.0) + rng.normal(0, 0.005, x.shape)).astype(F32)
    xyz = np.stack([x, y, z], 1)
    keep = rng.random(len(xyz)) >= holes
    xyz = xyz[keep]
    return xyz[rng.permutation(len(xyz))]


# ---- hand-checked cases of the restatement (no GPU) ---------------------------------------------------------------------
def _unit_square(a=(0.5, 0.5, 0.0), b=(1.5, 0.5, 0.0), c=(1.5, 1.5, 0.0), d=(0.5, 1.5, 0.0)):
    return np.array([a, b, c, d], F32)


def test_full_quad_takes_the_shorter_diagonal():
    # a-c shorter (c pulled towards a)
    xyz = _unit_square(c=(1.1, 1.1, 0.0))
    t, cnt, _ = mesh_numpy(xyz, 1.0, np.inf)
    assert t.tolist() == [[0, 1, 2], [0, 2, 3]] and cnt["n_quads_full"] == 1 and cnt["n_triangles"] == 2
    # b-d shorter (d pulled towards b)
    xyz = _unit_square(d=(0.9, 1.1, 0.0))
    t, cnt, _ = mesh_numpy(xyz, 1.0, np.inf)
    assert t.tolist() == [[0, 1, 3], [1, 2, 3]]
    # z counts in d2: a tall c makes a-c the longer diagonal
    xyz = _unit_square(c=(1.5, 1.5, 3.0))
    t, _, _ = mesh_numpy(xyz, 1.0, np.inf)
    assert t.tolist() == [[0, 1, 3], [1, 2, 3]]


def test_diagonal_tie_takes_a_c():
    t, cnt, _ = mesh_numpy(_unit_square(), 1.0, np.inf)
    assert t.tolist() == [[0, 1, 2], [0, 2, 3]]
    assert cnt == dict(n_vertices=4, n_shadowed=0, n_triangles=2, n_quads_full=1, n_rejected_orientation=0, n_rejected_length=0)


@pytest.mark.parametrize("missing,want", [(0, [1, 2, 3]), (1, [0, 2, 3]), (2, [0, 1, 3]), (3, [0, 1, 2])])
def test_three_corners(missing, want):
    xyz = _unit_square()
    keep = [i for i in range(4) if i != missing]
    t, cnt, _ = mesh_numpy(xyz[keep], 1.0, np.inf)
    assert [keep[i] for i in t[0]] == want and len(t) == 1 and cnt["n_quads_full"] == 0


def test_non_convex_quad_has_one_valid_split():
    # reflex corner at c (inside the triangle a, b, d): only a-c is valid, although b-d is the shorter diagonal
    xyz = _unit_square(a=(0.1, 0.1, 0.0), b=(1.9, 0.9, 0.0), c=(1.2, 1.2, 0.0), d=(0.9, 1.9, 0.0))
    assert orient(xyz[0], xyz[1], xyz[2]) > 0 and orient(xyz[0], xyz[2], xyz[3]) > 0
    assert not orient(xyz[1], xyz[2], xyz[3]) > 0 and d2(xyz[1], xyz[3]) < d2(xyz[0], xyz[2])
    t, _, _ = mesh_numpy(xyz, 1.0, np.inf)
    assert t.tolist() == [[0, 1, 2], [0, 2, 3]]
    # reflex corner at b (inside the triangle a, c, d): only b-d is valid
    xyz = _unit_square(a=(0.9, 0.1, 0.0), b=(1.05, 0.9, 0.0), c=(1.9, 1.9, 0.0), d=(0.1, 1.9, 0.0))
    assert not orient(xyz[0], xyz[1], xyz[2]) > 0
    assert orient(xyz[0], xyz[1], xyz[3]) > 0 and orient(xyz[1], xyz[2], xyz[3]) > 0
    t, _, _ = mesh_numpy(xyz, 1.0, np.inf)
    assert t.tolist() == [[0, 1, 3], [1, 2, 3]]


def test_edge_exactly_at_the_gate_is_kept():
    xyz = np.array([[0.25, 0.25, 0.0], [1.25, 0.25, 0.0], [1.25, 1.25, 0.0]], F32)  # a b c: edges 1, 1, sqrt(2)
    L = float(np.sqrt(2.0))
    assert d2(xyz[0], xyz[2]) == F32(L * L)  # 2.0000000000000004 rounds to 2.0f
    t, cnt, _ = mesh_numpy(xyz, 1.0, L)
    assert t.tolist() == [[0, 1, 2]] and cnt["n_rejected_length"] == 0
    t, cnt, _ = mesh_numpy(xyz, 1.0, float(np.nextafter(L, 0)))  # (float)(L*L) is still 2.0f: kept
    assert len(t) == 1
    t, cnt, _ = mesh_numpy(xyz, 1.0, L * (1 - 1e-7))  # below 2.0f: rejected
    assert len(t) == 0 and cnt["n_rejected_length"] == 1


def test_shadowed_point_is_counted_and_never_referenced():
    xyz = np.concatenate([_unit_square()[:1] + F32(0.1), _unit_square()])  # index 0 is a, the old a is shadowed
    t, cnt, nrm = mesh_numpy(xyz, 1.0, np.inf, normals=True)
    assert cnt["n_shadowed"] == 1 and cnt["n_vertices"] == 4
    assert 1 not in t and t.tolist() == [[0, 2, 3], [0, 3, 4]]
    assert np.isnan(nrm[1]).all() and not np.isnan(nrm[[0, 2, 3, 4]]).any()


def test_orientation_reject_and_normals_up():
    # a in the top-right corner of its cell, b and d in the far corners of theirs: (a, b, d) is clockwise
    bad = np.array([[0.999, 0.999, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], F32)
    assert orient(bad[0], bad[1], bad[2]) < 0
    t, cnt, nrm = mesh_numpy(bad, 1.0, np.inf, normals=True)
    assert len(t) == 0 and cnt["n_rejected_orientation"] == 1 and cnt["n_rejected_length"] == 0 and np.isnan(nrm).all()
    # a flat counter-clockwise triangle: every vertex normal is +z exactly
    flat = np.array([[0.5, 0.5, 0.0], [1.5, 0.5, 0.0], [0.1, 1.1, 0.0]], F32)
    t, cnt, nrm = mesh_numpy(flat, 1.0, np.inf, normals=True)
    assert t.tolist() == [[0, 1, 2]] and np.array_equal(nrm, np.tile(np.array([0, 0, 1], F32), (3, 1)))
    # a vertex without a triangle gets NaN
    t, cnt, nrm = mesh_numpy(np.concatenate([flat, [[5.5, 5.5, 0.0]]]).astype(F32), 1.0, np.inf, normals=True)
    assert np.isnan(nrm[3]).all() and not np.isnan(nrm[:3]).any()


def test_restatement_on_a_full_grid():
    k, m = 13, 9
    xyz = jittered_grid(k, m, seed=3)
    t, cnt, nrm = mesh_numpy(xyz, 0.05, np.inf, normals=True)
    assert len(t) == 2 * (k - 1) * (m - 1) and cnt["n_quads_full"] == (k - 1) * (m - 1)
    assert not np.isnan(nrm).any() and (nrm[:, 2] > 0).all()
    assert np.allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1, atol=1e-6)
    _check_valid(xyz, t)


def _check_valid(xyz, t, probes=2000, seed=0):
    """CCW, every undirected edge used at most twice and then in opposite directions, XY probes in at most one triangle"""
    assert (orient(xyz[t[:, 0]], xyz[t[:, 1]], xyz[t[:, 2]]) > 0).all()
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    directed = {tuple(x) for x in e.tolist()}
    assert len(directed) == len(e)  # a directed edge at most once
    und, cnt = np.unique(np.sort(e, 1), axis=0, return_counts=True)
    assert cnt.max() <= 2
    rng = np.random.default_rng(seed)
    lo, hi = xyz[:, :2].min(0), xyz[:, :2].max(0)
    pr = rng.uniform(lo, hi, (probes, 2))
    P0, P1, P2 = xyz[t[:, 0], :2].astype(np.float64), xyz[t[:, 1], :2].astype(np.float64), xyz[t[:, 2], :2].astype(np.float64)
    for q in pr:
        def side(a, b):
            return (b[:, 0] - a[:, 0]) * (q[1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (q[0] - a[:, 0])
        inside = (side(P0, P1) > 0) & (side(P1, P2) > 0) & (side(P2, P0) > 0)
        assert inside.sum() <= 1


# ---- ABI and CLI without a GPU --------------------------------------------------------------------------------------------
def test_abi_rejects_bad_arguments_without_a_gpu():
    from online_3d_reconstruction_amd import _lib
    L = _lib.load_library()
    prm = _lib.MeshParamsStruct()
    L.o3dr_mesh_default_params(C.byref(prm))
    assert prm.cell_size == 0.0 and prm.max_edge_length == 0.0
    pts = _pts(_unit_square())
    tris = np.full((8, 3), 7, np.int32)
    nt = C.c_int64(9)
    res = _lib.MeshResultStruct(1, 1, 1, 1, 1, 1)
    prm = _lib.MeshParamsStruct(0.05, 0.1)
    rc = L.o3dr_mesh_surface(None, pts.ctypes.data, 4, C.byref(prm), tris.ctypes.data, 8, C.byref(nt), None, C.byref(res), 0)
    assert rc == ERR_INVALID_ARG and nt.value == 0 and b"ctx" in L.o3dr_last_error()
    assert not tris.any() and (res.n_vertices, res.n_triangles, res.n_quads_full) == (0, 0, 0)
    rc = L.o3dr_mesh_surface(None, pts.ctypes.data, 4, None, tris.ctypes.data, 8, C.byref(nt), None, None, 0)
    assert rc == ERR_INVALID_ARG


def test_cli_mesh_surface_usage_errors(tmp_path):
    for argv in ([str(tmp_path / "a.ply")], [str(tmp_path / "a.ply"), "--mesh_normals"], [str(tmp_path / "a.ply"), "--voxel_size",
                                                                                            "0.05"], ["--search_radius", "0.1"], []):
        res = subprocess.run([POSE_BIN, "--mesh_surface"] + argv, capture_output=True, text=True, timeout=60)
        out = res.stdout + res.stderr
        assert res.returncode != 0 and "missing argument" in out and "unknown flag" not in out, (argv, out)
    usage = subprocess.run([POSE_BIN, "--help"], capture_output=True, text=True, timeout=60).stdout
    assert "--mesh_surface file.ply --search_radius L" in usage and "--mesh_normals" in usage
    assert "the mesh tool" not in usage


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mesh_ctx():
    import online_3d_reconstruction_amd as o3dr
    with o3dr.Context(0) as c:
        yield c


def _check_equal(ctx, xyz, cell, L, rgba=None):
    t_ref, cnt_ref, n_ref = mesh_numpy(xyz, cell, L, normals=True)
    t, nrm, info = ctx.meshSurface(_pts(xyz, rgba), cell, L, return_normals=True, return_info=True)
    assert t.dtype == np.int32 and t.shape == t_ref.shape and np.array_equal(t, t_ref)
    assert info.__dict__ == cnt_ref
    assert nrm.dtype == np.float32 and np.array_equal(nrm.view(np.uint32), n_ref.view(np.uint32))
    return t, nrm, info


@pytest.mark.gpu
@pytest.mark.parametrize("seed,holes,L", [(0, 0.0, np.inf), (1, 0.1, np.inf), (2, 0.3, 0.09), (3, 0.05, 0.07)])
def test_jittered_grids_with_holes_match_the_restatement(mesh_ctx, seed, holes, L):
    xyz = jittered_grid(157, 91, holes=holes, seed=seed)
    t, nrm, info = _check_equal(mesh_ctx, xyz, 0.05, L)
    assert info.n_shadowed == 0 and info.n_triangles > 0
    _check_valid(xyz, t, probes=500, seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
def test_random_clouds_with_several_points_per_cell_match_the_restatement(mesh_ctx, seed):
    rng = np.random.default_rng(100 + seed)
    n = 60000
    xyz = np.stack([rng.uniform(-3.0, 4.0, n), rng.uniform(-2.0, 2.5, n), rng.normal(0, 0.3, n)], 1).astype(F32)
    xyz[:2000] = np.round(xyz[:2000] / 0.1) * 0.1  # points on cell edges
    _, _, info = _check_equal(mesh_ctx, xyz, 0.1, 0.25)
    assert info.n_shadowed > 10000 and info.n_rejected_orientation > 0 and info.n_rejected_length > 0


@pytest.mark.gpu
def test_reference_cloud_matches_the_restatement(mesh_ctx):
    v = np.load(os.path.join(GOLDEN, "cloud_ply.npz"))["vertices"]
    xyz = np.stack([v["x"], v["y"], v["z"]], 1).astype(F32)
    t, nrm, info = _check_equal(mesh_ctx, xyz, 0.05, np.inf)
    assert info.n_vertices == 55940 and info.n_shadowed == 0 and info.n_quads_full == 54837
    assert info.n_triangles + info.n_rejected_orientation + info.n_rejected_length == 2 * 54837 + 878
    _check_equal(mesh_ctx, xyz, 0.05, 0.1)


@pytest.mark.gpu
def test_full_grid_gives_every_triangle(mesh_ctx):
    for k, m in ((2, 2), (64, 1), (1, 50), (130, 77), (301, 5)):
        xyz = jittered_grid(k, m, seed=k * m)
        t, info = mesh_ctx.meshSurface(_pts(xyz), 0.05, np.inf, return_info=True)
        assert len(t) == 2 * (k - 1) * (m - 1) == info.n_triangles
        if len(t):
            _check_valid(xyz, np.asarray(t), probes=300)


@pytest.mark.gpu
def test_merged_map_in_hbm_matches_the_restatement_and_host_memory():
    import torch

    import online_3d_reconstruction_amd as o3dr
    from online_3d_reconstruction_amd import synth
    with o3dr.Context(0, Q=synth.camera_Q(), params=o3dr.Params(jump_pixels=2, voxel_size=0.05, sor_enable=False)) as ctx:
        disp, bgr = synth.make_frames(0, 24)
        ctx.accumulateFrames(disp, bgr, synth.make_poses(0, 24))
        mp = ctx.finalize(device=torch.device("cuda", 0))
        mp = mp if torch.is_tensor(mp) else torch.from_numpy(np.ascontiguousarray(mp).view(np.int32).reshape(-1, 4)).cuda()
        mp = mp.contiguous()
        t_d, n_d, info_d = ctx.meshSurface(mp, 0.05, 0.2, return_normals=True, return_info=True)
        assert t_d.is_cuda and n_d.is_cuda and t_d.dtype == torch.int32 and tuple(n_d.shape) == (mp.shape[0], 3)
        host = mp.cpu().numpy().view(o3dr.POINT).reshape(-1)
        t_h, n_h, info_h = _check_equal(ctx, _xyz(host), 0.05, 0.2)
        assert info_d == info_h and np.array_equal(t_d.cpu().numpy(), t_h)
        assert np.array_equal(n_d.cpu().numpy().view(np.uint32), n_h.view(np.uint32))
        assert info_h.n_triangles > 0.5 * info_h.n_vertices


@pytest.mark.gpu
def test_repeated_calls_and_memory_kinds_are_identical(mesh_ctx):
    import torch
    xyz = jittered_grid(200, 120, holes=0.2, seed=9)
    xyz = np.concatenate([xyz, xyz[:3000] + F32(0.001)])
    pts = _pts(xyz)
    first = mesh_ctx.meshSurface(pts, 0.05, 0.08, return_normals=True, return_info=True)
    dev = torch.from_numpy(pts.view(np.int32).reshape(-1, 4)).cuda()
    for k in range(3):
        again = mesh_ctx.meshSurface(pts, 0.05, 0.08, return_normals=True, return_info=True)
        t_d, n_d, i_d = mesh_ctx.meshSurface(dev, 0.05, 0.08, return_normals=True, return_info=True)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1].view(np.uint32), again[1].view(np.uint32))
        assert first[2] == again[2] == i_d and np.array_equal(first[0], t_d.cpu().numpy())
        assert np.array_equal(first[1].view(np.uint32), n_d.cpu().numpy().view(np.uint32))


@pytest.mark.gpu
def test_capacity_protocol_and_counts_only(mesh_ctx):
    from online_3d_reconstruction_amd import _lib
    L = mesh_ctx._lib
    xyz = jittered_grid(40, 30, seed=5)
    want = mesh_ctx.meshSurface(_pts(xyz), 0.05, np.inf)
    T = len(want)
    pts = _pts(xyz)
    prm = _lib.MeshParamsStruct(0.05, float("inf"))
    nt = C.c_int64(0)
    res = _lib.MeshResultStruct()
    small = np.full((T - 1, 3), -5, np.int32)
    nrm = np.full((len(xyz), 3), 7, np.float32)
    rc = L.o3dr_mesh_surface(mesh_ctx._h, pts.ctypes.data, len(pts), C.byref(prm), small.ctypes.data, T - 1, C.byref(nt),
                             nrm.ctypes.data, C.byref(res), 0)
    assert rc == ERR_CAPACITY and nt.value == T
    assert (small == -5).all() and (nrm == 7).all()  # nothing else written
    rc = L.o3dr_mesh_surface(mesh_ctx._h, pts.ctypes.data, len(pts), C.byref(prm), None, 0, C.byref(nt), None, C.byref(res), 0)
    assert rc == 0 and nt.value == T == res.n_triangles
    exact = np.empty((T, 3), np.int32)
    rc = L.o3dr_mesh_surface(mesh_ctx._h, pts.ctypes.data, len(pts), C.byref(prm), exact.ctypes.data, T, C.byref(nt), None, None, 0)
    assert rc == 0 and np.array_equal(exact, want)


@pytest.mark.gpu
def test_empty_cloud_and_rejections(mesh_ctx):
    import online_3d_reconstruction_amd as o3dr
    t, nrm, info = mesh_ctx.meshSurface(_pts(np.zeros((0, 3))), 0.05, 0.1, return_normals=True, return_info=True)
    assert t.shape == (0, 3) and nrm.shape == (0, 3) and info.n_vertices == 0 and info.n_triangles == 0
    xyz = jittered_grid(10, 10, seed=1)
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy()
        x[37, 2] = bad
        with pytest.raises(o3dr.O3drError) as e:
            mesh_ctx.meshSurface(_pts(x), 0.05, 0.1)
        assert e.value.code == ERR_INVALID_ARG
    for cell, L in ((0.0, 0.1), (-0.05, 0.1), (np.nan, 0.1), (np.inf, 0.1), (1e-50, 0.1), (0.05, 0.0), (0.05, -1.0), (0.05, np.nan)):
        with pytest.raises(o3dr.O3drError) as e:
            mesh_ctx.meshSurface(_pts(xyz), cell, L)
        assert e.value.code == ERR_INVALID_ARG, (cell, L)
    # a cell index outside int32
    with pytest.raises(o3dr.O3drError) as e:
        mesh_ctx.meshSurface(_pts([[0.0, 0.0, 0.0], [2.0e8, 0.0, 0.0]]), 0.05, 0.1)
    assert e.value.code == ERR_INVALID_ARG
    # the mesh still works after the errors
    assert len(mesh_ctx.meshSurface(_pts(xyz), 0.05, np.inf)) == 2 * 9 * 9


@pytest.mark.gpu
def test_cell_box_limit(mesh_ctx):
    import online_3d_reconstruction_amd as o3dr
    corner = jittered_grid(3, 3, cell=0.05, seed=2)
    # 2^32 cells (65536 x 65536 at 1 m) and 3.2 km x 3.2 km at 0.05 m work: a small patch in each corner
    for cell, w in ((1.0, 65536), (0.05, 64000)):
        xyz = np.concatenate([corner / F32(0.05) * F32(cell), corner / F32(0.05) * F32(cell) + F32((w - 3) * cell) * np.array([1, 1, 0], F32)])
        xyz = xyz.astype(F32)
        t_ref, cnt, _ = mesh_numpy(xyz, cell, np.inf)
        cx = np.floor(xyz[:, 0] * (F32(1) / F32(cell))).astype(np.int64)
        cy = np.floor(xyz[:, 1] * (F32(1) / F32(cell))).astype(np.int64)
        assert (cx.max() - cx.min() + 1) * (cy.max() - cy.min() + 1) <= 2 ** 32
        t = mesh_ctx.meshSurface(_pts(xyz), cell, np.inf)
        assert np.array_equal(t, t_ref) and len(t) == 16
    # one cell more in each direction than 2^32 allows
    xyz = np.array([[0.5, 0.5, 0.0], [65536.5, 0.5, 0.0], [0.5, 65535.5, 0.0]], F32)
    with pytest.raises(o3dr.O3drError) as e:
        mesh_ctx.meshSurface(_pts(xyz), 1.0, np.inf)
    assert e.value.code == ERR_INVALID_ARG


def _read_mesh_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + 11
    head = raw[:end].decode()
    n = int(head.split("element vertex ")[1].split("\n")[0])
    nf = int(head.split("element face ")[1].split("\n")[0])
    assert "property list uchar int vertex_indices" in head
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")]
    if "property float nx" in head:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    dt = np.dtype(fields)
    v = np.frombuffer(raw, dt, n, end)
    fdt = np.dtype([("k", "u1"), ("i", "<i4", (3,))])
    f = np.frombuffer(raw, fdt, nf, end + n * dt.itemsize)
    assert len(raw) == end + n * dt.itemsize + nf * fdt.itemsize and (f["k"] == 3).all()
    return v, f["i"].copy()


@pytest.mark.gpu
def test_cli_mesh_surface_end_to_end(tmp_path, mesh_ctx):
    z = np.load(os.path.join(GOLDEN, "cloud_ply.npz"))
    src = str(tmp_path / "cloud.ply")
    with open(src, "wb") as f:
        f.write(z["header"].tobytes() + z["vertices"].tobytes() + z["tail"].tobytes())
    v = z["vertices"]
    rgba = (np.uint32(255) << 24) | (v["r"].astype(np.uint32) << 16) | (v["g"].astype(np.uint32) << 8) | v["b"].astype(np.uint32)
    pts = _pts(np.stack([v["x"], v["y"], v["z"]], 1), rgba)
    t, nrm, info = mesh_ctx.meshSurface(pts, 0.05, 0.15, return_normals=True, return_info=True)
    for normals in (False, True):
        argv = [POSE_BIN, "--mesh_surface", src, "--voxel_size", "0.05", "--search_radius", "0.15"] + (["--mesh_normals"] if normals else [])
        res = subprocess.run(argv, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout + res.stderr
        assert f"points in {len(pts)}" in res.stdout and f"vertices {info.n_vertices} (shadowed points 0)" in res.stdout
        assert f"triangles {info.n_triangles} (full quads {info.n_quads_full})" in res.stdout and "mesh time" in res.stdout
        mv, faces = _read_mesh_ply(str(tmp_path / "mesh_cloud.ply"))
        assert np.array_equal(faces, t) and len(mv) == len(pts)
        for ax in "xyz":
            assert np.array_equal(mv[ax].view(np.uint32), pts[ax].view(np.uint32))
        assert np.array_equal(mv["red"], v["r"]) and np.array_equal(mv["blue"], v["b"])
        if normals:
            got = np.stack([mv["nx"], mv["ny"], mv["nz"]], 1)
            assert np.array_equal(got.view(np.uint32), nrm.view(np.uint32))
    # the mesh's vertices go back through --downsample
    res = subprocess.run([POSE_BIN, "--downsample", str(tmp_path / "mesh_cloud.ply"), "--voxel_size", "0.2"], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert os.path.exists(str(tmp_path / "downsampled_mesh_cloud.ply"))
    res2 = subprocess.run([POSE_BIN, "--downsample", src, "--voxel_size", "0.2"], capture_output=True, text=True, timeout=300)
    assert res2.returncode == 0
    a = open(str(tmp_path / "downsampled_mesh_cloud.ply"), "rb").read()
    b = open(str(tmp_path / "downsampled_cloud.ply"), "rb").read()
    assert a == b
