"""The grid-search operators (exact nearest neighbour / ICP, MLS, and the tiling of plane segmentation and meshing) on the
inputs the other modules do not have: clouds kilometres from the origin, the map's size (480 000 points, 300 000 queries
/ sources), densities and extents that decide the search grid by its clamps, counts at the wave and workgroup edges, and
queries where the ring walk's stop test is tight.

Nothing is restated here but the search grid itself (sor_plan_of / sor_cell, to place queries on cell boundaries): the
references are the other modules' (nn_brute, nn_tree, kabsch, icp_numpy, neighbours, mls_numpy, check_against_numpy,
plane_numpy, tiles_numpy, mesh_numpy).  Every coordinate a generator returns lies on the 2^-10 m grid, so the translations by
(1024, -1024) and (-8192, 8192) are exact in fp32: differences of coordinates, and with them every fp32 distance, are
the same numbers at every translation, and a result that changes with the translation is a bound that rounds with |min|."""
import numpy as np
import pytest

from test_icp_align import NONE, UNCHANGED_OR_SMALL, a2, icp_numpy, kabsch, nn_brute, nn_tree, rigid, rot_trans_err, synthetic_surface
from test_icp_align import _pts, _torch_pts
from test_mls_smooth import PLANE, POLY, check_against_numpy, mls_numpy, neighbours
from test_mls_smooth import NONE as MLS_NONE

GRID = 1024.0  # coordinates are multiples of 1 / GRID
OFFSETS = ((0.0, 0.0), (1024.0, -1024.0), (-8192.0, 8192.0))
FAR = OFFSETS[1:]
EDGE_COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
MLS_CHUNK = 60000
F32 = np.float32


# ---- generators (numpy only) --------------------------------------------------------------------------------------------
def on_grid(xyz):
    return (np.round(np.asarray(xyz, np.float64) * GRID) / GRID + 0.0).astype(F32)  # (+ 0.0: no negative zero)


def translated(xyz, off):
    """fp32 addition of off to x and y"""
    out = np.array(xyz, F32, copy=True)
    out[:, 0] = out[:, 0] + F32(off[0])
    out[:, 1] = out[:, 1] + F32(off[1])
    return out


def untranslated(xyz, off):
    return translated(xyz, (-off[0], -off[1]))


def map_like(nx, ny, seed, cell=0.05):
    """a 2.5-D map: one point per XY cell of `cell` m, jittered inside it, wavy z with a little noise, in random order"""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny), indexing="xy")
    u = rng.uniform(0.05, 0.95, (ny, nx, 2))
    x, y = ((gx + u[..., 0]) * cell).reshape(-1), ((gy + u[..., 1]) * cell).reshape(-1)
    z = 0.3 * np.sin(0.9 * x) * np.cos(0.7 * y) + 0.02 * x + rng.normal(0, 0.003, x.shape)
    xyz = on_grid(np.stack([x, y, z], 1))
    return xyz[rng.permutation(len(xyz))]


def skewed(n, seed, clump=1.0):
    """9 of 10 points in a clump of `clump` x `clump` m, the rest spread over a box 101 clumps wide (the clump covers 1e-4 of
    it) whose corners are four of the points, 50 clump sizes from the clump"""
    rng = np.random.default_rng(seed)
    nc = n * 9 // 10
    c = np.stack([rng.uniform(0, clump, nc), rng.uniform(0, clump, nc), 0.05 * rng.standard_normal(nc)], 1)
    c[:, 2] += 0.2 * np.sin(5 * c[:, 0])
    lo, hi = -50.0 * clump, 51.0 * clump
    s = np.stack([rng.uniform(lo, hi, n - nc - 4), rng.uniform(lo, hi, n - nc - 4), rng.uniform(-1, 1, n - nc - 4)], 1)
    corners = np.array([[lo, lo, 0.0], [hi, lo, 0.5], [lo, hi, -0.5], [hi, hi, 0.25]])
    xyz = on_grid(np.concatenate([c, s, corners]))
    return xyz[rng.permutation(n)]


def degenerate():
    """named clouds whose extent or ties decide the grid -> {name: xyz}, near the origin"""
    rng = np.random.default_rng(77)
    t = on_grid(np.sort(rng.uniform(0, 10, (500, 1)), 0))[:, 0].astype(np.float64)
    g = np.arange(24) / 128.0
    lat = np.stack(np.meshgrid(g, g, g[:3], indexing="ij"), -1).reshape(-1, 3)  # every distance is a tie of many
    out = {
        "line_x": np.stack([t, np.full(500, 1.5), np.full(500, -2.0)], 1),
        "line_y": np.stack([np.full(500, -3.25), t, np.full(500, 0.5)], 1),
        "diagonal": np.stack([t, t, 2.0 * t], 1),  # exactly one line, after the rounding too
        "copies": np.tile([[1.25, -2.5, 0.75]], (4000, 1)),
        "two_points": np.array([[0.5, 0.25, 0.0], [0.75, 1.0, 0.125]]),
        "wall": np.stack([np.full(3000, 3.0), rng.uniform(0, 5, 3000), rng.uniform(0, 3, 3000)], 1),
        "lattice": lat[rng.permutation(len(lat))],
    }
    return {k: on_grid(v) for k, v in out.items()}


def degenerate_everywhere():
    return [(f"{name}@{off}", translated(xyz, off)) for name, xyz in degenerate().items() for off in OFFSETS]


# the search grid of kernels/sor.inc, restated: sor_plan_of (with the nearest-neighbour search's 8 points per column and
# its cell budget max(n / 2, 1024)) and sor_cell.  The library also clamps the budget to what the context's workspace was
# sized for; the workspace grows with the largest call, so that clamp never binds.  The restatement only decides where
# edge_queries puts its points, never what is asserted.
def plan_numpy(xyz, cell_points=8.0):
    xyz = np.asarray(xyz, F32)
    n = len(xyz)
    mn, mx = xyz[:, :2].min(0), xyz[:, :2].max(0)
    max_cells = max(n // 2, 1024)
    ex, ey = (max(float(mx[a]) - float(mn[a]), 1e-9) for a in range(2))
    h = max(np.sqrt(cell_points * ex * ey / max(n, 1)), 1e-6)
    gx, gy = int(ex / h) + 1, int(ey / h) + 1
    while gx * gy > max_cells:
        h *= 1.25
        gx, gy = int(ex / h) + 1, int(ey / h) + 1
    return dict(mn=mn, h=F32(h), inv_h=F32(1.0 / h), gx=gx, gy=gy, max_cells=max_cells)


def cell_numpy(sg, xy):
    """-> (cx, cy, unclamped cx, unclamped cy); the conversion to int truncates and saturates like the device's"""
    xy = np.asarray(xy, F32).reshape(-1, 2)
    raw = []
    for a in range(2):
        f = ((xy[:, a] - sg["mn"][a]) * sg["inv_h"]).astype(np.float64)  # the fp32 product, widened only to truncate it
        raw.append(np.trunc(np.clip(f, -2.0**31, 2.0**31 - 1)).astype(np.int64))
    return np.clip(raw[0], 0, sg["gx"] - 1), np.clip(raw[1], 0, sg["gy"] - 1), raw[0], raw[1]


def _steps(v, k):
    v = np.asarray(v, F32)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf))
    return v


def edge_queries(target, sg, seed=0):
    """queries where the ring walk's stop test is tight: the 8 corners of the target's box, points on its 6 faces, points
    on the computed cell boundaries fp32(mn + k h) and one fp32 step either side, and 100 points 10 km outside the box"""
    rng = np.random.default_rng(seed)
    t = np.asarray(target, F32)
    lo, hi = t.min(0), t.max(0)

    def inside(m):
        return (lo + (hi - lo) * rng.random((m, 3))).astype(F32)

    q = [np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in range(2) for j in range(2) for k in range(2)], F32)]
    for a in range(3):
        for side in (lo, hi):
            f = inside(12)
            f[:, a] = side[a]
            q.append(f)
    for a, g in ((0, sg["gx"]), (1, sg["gy"])):
        ks = np.unique(np.concatenate([np.arange(min(g + 1, 4)), rng.integers(0, g + 1, 24), [g - 1, g, g + 1]]))
        b = (np.float64(sg["mn"][a]) + ks * np.float64(sg["h"])).astype(F32)
        for step in (-1, 0, 1):
            f = inside(len(b))
            f[:, a] = _steps(b, step)
            if step == 0:  # and on a boundary of the other axis too
                o = 1 - a
                f[::2, o] = F32(np.float64(sg["mn"][o]) + (sg["gy"] if a == 0 else sg["gx"]) // 2 * np.float64(sg["h"]))
            q.append(f)
    ang = rng.uniform(0, 2 * np.pi, 100)
    far = inside(100).astype(np.float64)
    far[:, 0] += 1e4 * np.cos(ang) + np.sign(np.cos(ang)) * float(hi[0] - lo[0])
    far[:, 1] += 1e4 * np.sin(ang) + np.sign(np.sin(ang)) * float(hi[1] - lo[1])
    far[::10, 2] += 1e4
    q.append(far.astype(F32))
    return np.concatenate(q)


def kabsch_centred(P, Q, c):
    """kabsch with both clouds moved by -c first (what the library does with the centre of the target's box): the same
    solve in exact arithmetic, a second evaluation of the reference whose rounding differs"""
    c = np.asarray(c, np.float64)
    T, deg = kabsch(P.astype(np.float64) - c, Q.astype(np.float64) - c)
    if deg:
        return None, True
    T = T.copy()
    T[:3, 3] = T[:3, 3] + c - T[:3, :3] @ c
    return T, False


def conjugated(T, off):
    """T about the translated origin -> the same motion about the untranslated one"""
    S = np.eye(4)
    S[:2, 3] = off
    return np.linalg.inv(S) @ np.asarray(T, np.float64) @ S


@pytest.fixture(scope="module")
def big_map():
    return map_like(800, 600, 1)


def big_queries(tgt, n=300000, seed=2, sigma=0.01):
    rng = np.random.default_rng(seed)
    pick = rng.permutation(len(tgt))[:n]
    return on_grid(tgt[pick].astype(np.float64) + rng.normal(0, sigma, (n, 3)))


# ---- without a GPU: the generators and the references' own conditions -------------------------------------------------------
def test_generators_translate_exactly_without_a_gpu():
    clouds = dict(degenerate(), map=map_like(200, 150, 3), skewed=skewed(22000, 4), queries=big_queries(map_like(200, 150, 3), 9000))
    for name, xyz in clouds.items():
        assert xyz.dtype == F32 and np.array_equal(on_grid(xyz), xyz), name
        for off in FAR:
            t = translated(xyz, off)
            assert np.array_equal(untranslated(t, off).view(np.uint32), xyz.view(np.uint32)), (name, off)
            # and in real arithmetic: the fp32 sum is the exact sum
            assert np.array_equal(t[:, :2].astype(np.float64), xyz[:, :2].astype(np.float64) + np.asarray(off)), (name, off)
    d = degenerate()
    assert len(np.unique(d["copies"], axis=0)) == 1 and len(d["copies"]) == 4000 and len(d["two_points"]) == 2
    assert np.ptp(d["line_x"][:, 1]) == 0 and np.ptp(d["line_y"][:, 0]) == 0 and np.ptp(d["wall"][:, 0]) == 0
    assert np.array_equal(d["diagonal"][:, 0], d["diagonal"][:, 1]) and np.array_equal(d["diagonal"][:, 2], d["diagonal"][:, 0] * F32(2))
    s = skewed(22000, 4)
    in_clump = ((s[:, :2] >= 0) & (s[:, :2] <= 1)).all(1)
    box = np.ptp(s[:, :2], 0)
    assert 0.89 < in_clump.mean() < 0.91 and 1.0 / (box[0] * box[1]) <= 1e-3 and (box == 101).all()
    m = map_like(200, 150, 3)
    assert len(m) == 30000 and len(np.unique(np.floor(m[:, :2].astype(np.float64) / 0.05), axis=0)) > 29900


def test_restated_cells_are_in_range_and_edge_queries_sit_on_boundaries_without_a_gpu():
    clouds = [("map", map_like(200, 150, 3)), ("skewed", skewed(22000, 4))] + degenerate_everywhere()
    for name, xyz in clouds:
        sg = plan_numpy(xyz)
        assert sg["gx"] >= 1 and sg["gy"] >= 1 and sg["gx"] * sg["gy"] <= sg["max_cells"] and sg["h"] >= F32(1e-6), name
        cx, cy, rx, ry = cell_numpy(sg, xyz[:, :2])
        assert (rx >= 0).all() and (rx < sg["gx"]).all() and (ry >= 0).all() and (ry < sg["gy"]).all(), name
        # the assignment is monotone in the coordinate (what the MLS window relies on)
        o = np.argsort(xyz[:, 0], kind="stable")
        assert (np.diff(cx[o]) >= 0).all(), name
        q = edge_queries(xyz, sg)
        assert np.isfinite(q).all() and len(q) >= 8 + 72 + 100, name
        qx, qy, _, _ = cell_numpy(sg, q[:, :2])
        if sg["gx"] > 2:  # queries one fp32 step apart fall in neighbouring columns: the boundaries are hit
            assert len(np.unique(qx)) >= min(sg["gx"], 5), name
        lo, hi = xyz.min(0), xyz.max(0)
        gap = np.maximum(np.maximum(lo[:2] - q[:, :2].astype(np.float64), q[:, :2] - hi[:2].astype(np.float64)), 0)
        assert (np.hypot(gap[:, 0], gap[:, 1]) >= 9999).sum() == 100, name
    # the grids the degenerate extents give: one cell for the copies, a single row / column for the lines
    d = degenerate()
    assert (plan_numpy(d["copies"])["gx"], plan_numpy(d["copies"])["gy"]) == (1, 1)
    assert plan_numpy(d["line_x"])["gy"] == 1 and plan_numpy(d["line_y"])["gx"] == 1 and plan_numpy(d["wall"])["gx"] == 1
    sk = skewed(22000, 4)
    sg = plan_numpy(sk)
    cx, cy, _, _ = cell_numpy(sg, sk[:, :2])
    pop = np.bincount(cy * sg["gx"] + cx, minlength=sg["gx"] * sg["gy"])
    assert pop.max() > 4000 and (pop == 0).mean() > 0.4 and np.median(pop) <= 1  # a column of thousands among empty and sparse ones


def test_reference_fallback_share_on_a_map_without_a_gpu():
    """nn_tree certifies (nearly) every row of a map-like case at every translation: the 480 000-point cases stay cheap"""
    tgt = map_like(300, 200, 5)
    q = big_queries(tgt, 40000, 6)
    base = None
    for off in OFFSETS:
        for md in (np.inf, 0.03):
            stats = {}
            idx, d2 = nn_tree(translated(q, off), translated(tgt, off), md, stats=stats)
            assert stats["rows"] == len(q) and stats["fallback"] <= 1e-3 * len(q), (off, md, stats)
            if md == np.inf:
                if base is None:
                    base = (idx, d2)
                    bi, bd = nn_brute(q[:3000], tgt)
                    assert np.array_equal(idx[:3000], bi) and np.array_equal(d2[:3000].view(np.uint32), bd.view(np.uint32))
                # the reference itself is translation-invariant on these inputs
                assert np.array_equal(idx, base[0]) and np.array_equal(d2.view(np.uint32), base[1].view(np.uint32))
            else:
                assert (idx == NONE).any() and (idx != NONE).any()


def _excluded(ref, order):
    """what check_against_numpy(..., decided_by_k=True) sets aside, from the reference alone -> (fit kind, normal)"""
    nc = (order + 1) * (order + 2) // 2
    ratio_ok = np.abs(ref["ratio_margin"]) >= 1e-9
    pivot_ok = (order == 0) | (ref["k"] < nc) | (np.abs(ref["pivot_margin"]) >= 1e-9) | (ref["fit"] == MLS_NONE)
    sure = (ref["k"] < 3) | (ratio_ok & pivot_ok)
    return int((~sure).sum()), int(((ref["fit"] != MLS_NONE) & (ref["gap"] < 1e-4)).sum())


def _checked(xyz, got, r, order, chunk=None):
    """check_against_numpy with the cap on what it may leave out: at most 0.1 % of the cloud"""
    obs = check_against_numpy(xyz, got[0], got[1], got[2], got[3], r, order, chunk=chunk, decided_by_k=True)
    assert obs["n"] == len(xyz) and obs["n_unsure"] + obs["n_differ"] + obs["n_small_gap"] <= 1e-3 * len(xyz), obs
    return obs


COUNT_POOL_SEED, COUNT_R = 33, 0.25
HAND_POINTS = [[0, 0, 0], [0.1, 0, 0.01], [0, 0.1, 0.02], [0.1, 0.1, 0.0], [0.05, 0.03, 0.01], [0.02, 0.07, 0.0]]


def test_mls_reference_sets_aside_nothing_of_the_small_clouds_without_a_gpu():
    """on the reference alone: every other cloud that goes through check_against_numpy here stays under the cap of 0.1 %
    (for these sizes: nothing set aside), at every translation and order it is run at"""
    pool = map_like(20, 13, COUNT_POOL_SEED)
    for n in (1, 2, 3, 5, 6, 63, 64, 65, 255, 256, 257):
        for off in (OFFSETS[0], OFFSETS[2]):
            for order in (0, 1, 2):
                assert _excluded(mls_numpy(translated(pool[:n], off), COUNT_R, order), order) == (0, 0), (n, off, order)
    for n in (5, 6):
        ref = mls_numpy(translated(on_grid(HAND_POINTS)[:n], OFFSETS[2]), 1.0, 2)
        assert _excluded(ref, 2) == (0, 0) and (ref["k"] == n).all() and (ref["fit"] == (POLY if n == 6 else PLANE)).all()
    strip, wall, clump = map_like(400, 6, 34), degenerate()["wall"], skewed(8000, 31)
    for off in OFFSETS:
        for order in (0, 2):
            assert sum(_excluded(mls_numpy(translated(strip, off), 0.35, order), order)) <= 1e-3 * len(strip), (off, order)
            assert sum(_excluded(mls_numpy(translated(wall, off), 0.3, order), order)) <= 1e-3 * len(wall), (off, order)
    assert sum(_excluded(mls_numpy(clump, 0.3, 2, chunk=500), 2)) <= 1e-3 * len(clump)


def test_mls_reference_sets_aside_few_points_of_a_map_without_a_gpu():
    """on the reference alone: a slice of a map at r = 0.1, every order and translation, sets aside at most 0.1 % of its
    points (threshold-adjacent fit kinds, small eigen gaps); the slice and chunk forms of mls_numpy agree with the whole"""
    xyz = map_like(300, 200, 7)
    rows = slice(20000, 30000)
    for off in OFFSETS:
        t = translated(xyz, off)
        for order in (0, 1, 2):
            ref = mls_numpy(t, 0.1, order, rows=rows)
            unsure, small_gap = _excluded(ref, order)
            assert unsure + small_gap <= 1e-3 * 10000, (off, order, unsure, small_gap)
            assert ref["k"].max() <= 30 and (ref["fit"] == (POLY if order else PLANE)).mean() > 0.95
    small = map_like(60, 50, 8)
    whole, chunked, part = mls_numpy(small, 0.1, 2), mls_numpy(small, 0.1, 2, chunk=700), mls_numpy(small, 0.1, 2, rows=slice(1000, 1700))
    for key in whole:
        assert np.array_equal(whole[key], chunked[key], equal_nan=True), key
        assert np.array_equal(whole[key][1000:1700], part[key], equal_nan=True), key


def test_kabsch_centred_is_kabsch_without_a_gpu():
    rng = np.random.default_rng(9)
    P = translated(on_grid(rng.uniform(0, 30, (5000, 3))), FAR[1])
    Q = a2(rigid(0.001, -0.002, 0.0015, [0.02, 0.01, -0.01]).astype(F32), P)
    T0, _ = kabsch(P, Q)
    T1, _ = kabsch_centred(P, Q, P.mean(0))
    assert np.abs(T0[:3, :3] - T1[:3, :3]).max() < 1e-12 and np.abs(T0[:3, 3] - T1[:3, 3]).max() < 1e-7
    G = rigid(0.01, 0.02, -0.03, [0.1, 0.2, 0.3])
    S = np.eye(4)
    S[:2, 3] = FAR[1]
    assert np.abs(conjugated(S @ G @ np.linalg.inv(S), FAR[1]) - G).max() < 1e-9


# ---- on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sg_ctx():
    import online_3d_reconstruction_amd as o3dr
    c = o3dr.Context(0)
    yield c
    c.close()


def _nn(ctx, q, t, md=np.inf):
    return ctx.nearestNeighbors(_pts(q), _pts(t), md)


def _same_nn(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _check_nn(ctx, q, t, md=np.inf, oracle=nn_brute, what=""):
    got = _nn(ctx, q, t, md)
    ref = oracle(q, t, md)
    bad = np.nonzero((got[0] != ref[0]) | (got[1].view(np.uint32) != ref[1].view(np.uint32)))[0]
    assert bad.size == 0, (what, md, bad.size, bad[:5], q[bad[:5]], got[0][bad[:5]], ref[0][bad[:5]], got[1][bad[:5]], ref[1][bad[:5]])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("md", [np.inf, 0.03])
def test_nn_map_scale_bit_exact_at_every_translation(sg_ctx, big_map, md):
    """480 000 targets, 300 000 queries (targets + 1 cm noise): idx and d2 equal the reference at (0, 0), (1024, -1024) and
    (-8192, 8192), and the far results equal the untranslated ones bit for bit"""
    q = big_queries(big_map)
    base = None
    for off in OFFSETS:
        stats = {}
        got = _check_nn(sg_ctx, translated(q, off), translated(big_map, off), md, what=off,
                        oracle=lambda a, b, m: nn_tree(a, b, m, stats=stats))
        assert stats["fallback"] <= 1e-3 * len(q), stats  # the reference stays cheap (not a property of the kernel)
        if base is None:
            base = got
            assert (got[0] != NONE).sum() > 1000 and (md == np.inf or (got[0] == NONE).sum() > 1000)
        assert _same_nn(got, base), off


@pytest.mark.gpu
def test_nn_target_one_point_past_the_one_workgroup_histogram_scan(sg_ctx):
    """95 sort tiles of 8192 records are the most whose digit histograms one workgroup scans in LDS (hist_tm in
    o3dr_kernels.hip); a target of 95 * 8192 + 1 points is the smallest whose search-grid sort takes the chunked scan"""
    n = 95 * 8192 + 1
    t = map_like(1024, 761, 31)[:n]
    assert len(t) == n
    q = big_queries(t, 20000, 32)
    stats = {}
    got = _check_nn(sg_ctx, q, t, what=n, oracle=lambda a, b, m: nn_tree(a, b, m, stats=stats))
    assert stats["fallback"] <= 1e-3 * len(q), stats  # the reference stays cheap (not a property of the kernel)
    assert (got[0] != NONE).all() and len(np.unique(got[0])) > 15000


@pytest.mark.gpu
def test_nn_skewed_density(sg_ctx):
    """20 000 points in one or two columns of a grid that four far corners stretch: finite and infinite radius"""
    t = skewed(22222, 11)
    rng = np.random.default_rng(12)
    q = np.concatenate([on_grid(t[::8].astype(np.float64) + rng.normal(0, 0.02, (len(t[::8]), 3))), t[-50:],
                        on_grid(rng.uniform(-60, 60, (500, 3)))])
    for off in OFFSETS:
        tt, qq = translated(t, off), translated(q, off)
        a = _check_nn(sg_ctx, qq, tt, what=off)
        b = _check_nn(sg_ctx, qq, tt, 0.05, what=off)
        assert (b[0] == NONE).any() and (b[0] != NONE).any()
        if off == OFFSETS[0]:
            base = (a, b)
        assert _same_nn(a, base[0]) and _same_nn(b, base[1]), off


@pytest.mark.gpu
def test_nn_degenerate_clouds_and_edge_queries(sg_ctx):
    """lines, copies, two points, a wall and a lattice, at every translation: their own points, points around them and the
    queries on box corners, faces, computed cell boundaries (+-1 fp32 step) and 10 km outside"""
    rng = np.random.default_rng(13)
    for name, t in degenerate_everywhere():
        lo, hi = t.min(0).astype(np.float64), t.max(0).astype(np.float64)
        ext = np.maximum(hi - lo, 0.5)
        around = on_grid(lo - ext + (hi - lo + 2 * ext) * rng.random((600, 3)))
        q = np.concatenate([t[:: max(1, len(t) // 400)], around, edge_queries(t, plan_numpy(t), seed=len(t))])
        _check_nn(sg_ctx, q, t, what=name)
        r = float(np.linalg.norm(ext)) * 0.25
        got = _check_nn(sg_ctx, q, t, r, what=name)
        assert (got[0] == NONE).any() and (got[0] != NONE).any(), name
    for off in OFFSETS:  # the same queries against a map and a skewed cloud
        for t in (translated(map_like(160, 120, 14), off), translated(skewed(6000, 15), off)):
            q = edge_queries(t, plan_numpy(t), seed=3)
            _check_nn(sg_ctx, q, t, what=("edges", off))
            _check_nn(sg_ctx, q, t, 0.2, what=("edges", off))


@pytest.mark.gpu
def test_nn_lattice_radius_on_and_just_below_a_tie(sg_ctx):
    """a 2^-7 lattice, queries on lattice sites one and two steps outside it: with max_distance = k 2^-7 the neighbour at
    d2 == r2 exactly is kept, one fp32 step below it is dropped"""
    lat = degenerate()["lattice"]
    s = 1.0 / 128
    for off in OFFSETS:
        t = translated(lat, off)
        for k in (1, 2):
            g = np.arange(24) * s
            q = np.stack(np.meshgrid(g, g, [2 * s + k * s], indexing="ij"), -1).reshape(-1, 3).astype(F32)  # k steps above the top
            q = translated(np.concatenate([q, q * [1, 1, 0] + [0, 0, -k * s]]).astype(F32), off)
            md = k * s
            assert np.float32(md * md) == np.float32(k * k) * np.float32(s * s)
            kept = _check_nn(sg_ctx, q, t, md, what=(off, k))
            assert (kept[0] != NONE).all() and (kept[1] == np.float32(md * md)).all()
            below = float(np.nextafter(np.float32(md), np.float32(0)))
            assert np.float32(below * below) < np.float32(md * md)
            dropped = _check_nn(sg_ctx, q, t, below, what=(off, k, "below"))
            assert (dropped[0] == NONE).all() and np.isinf(dropped[1]).all()
            _check_nn(sg_ctx, q, t, what=(off, k, "inf"))


@pytest.mark.gpu
def test_nn_counts_at_wave_and_workgroup_edges(sg_ctx):
    rng = np.random.default_rng(16)
    pool_t = on_grid(rng.uniform(0, 6, (1025, 3)) * [1, 1, 0.2])
    pool_q = on_grid(rng.uniform(-1, 7, (1025, 3)) * [1, 1, 0.2])
    for i, nt in enumerate(EDGE_COUNTS):
        for nq in sorted({EDGE_COUNTS[i], EDGE_COUNTS[(i + 3) % 11], EDGE_COUNTS[(i + 7) % 11]}):
            for off in (OFFSETS[0], OFFSETS[2]):
                t, q = translated(pool_t[:nt], off), translated(pool_q[-nq:], off)
                _check_nn(sg_ctx, q, t, what=(nt, nq, off))
                _check_nn(sg_ctx, q, t, 0.4, what=(nt, nq, off))


# ---- ICP ------------------------------------------------------------------------------------------------------------------
def _icp_bits(r):
    return (r.T.view(np.uint64).tolist(), np.float64(r.fitness).view(np.uint64), r.n_correspondences, r.iterations, r.reason)


@pytest.mark.gpu
def test_icp_one_pass_of_300000_sources_on_the_map(sg_ctx, big_map):
    """300 000 sources = 1172 workgroups of 256: k_icp_fold's stride-1024 loop takes its second trip.  T, the correspondence
    count and the fitness of one pass against icp_numpy at the three translations.  Near the origin |dT| < 1e-9 as in
    test_icp_first_step_is_exact; far from it the rotation block keeps 1e-9 and the translation column gets 16 x the
    reference's own noise floor there: the largest difference between kabsch and kabsch_centred on the same correspondences"""
    src = big_queries(big_map, 300000, 21, sigma=0.005)
    assert -(-len(src) // 256) == 1172 > 1024
    T0 = rigid(0.0, 0.0, 0.0, [0.004, -0.003, 0.002]).astype(F32)  # a pure shift: exact at every translation
    cases, floor = [], 0.0
    for off in OFFSETS:
        s, t = translated(src, off), translated(big_map, off)
        r = sg_ctx.icpAlign(_pts(s), _pts(t), T_init=T0, max_iterations=1)
        ref = icp_numpy(s, t, T0, max_iterations=1, nn=nn_tree)
        P = a2(T0, s)
        idx, _ = nn_tree(P, t)
        Ta, _ = kabsch(P, t[idx])
        Tb, _ = kabsch_centred(P, t[idx], (t.min(0).astype(np.float64) + t.max(0).astype(np.float64)) / 2)
        assert np.abs(Ta[:3, :3] - Tb[:3, :3]).max() < 1e-9
        if off != OFFSETS[0]:
            floor = max(floor, float(np.abs(Ta[:3, 3] - Tb[:3, 3]).max()))
        cases.append((off, r, ref))
    tol = 16 * floor
    print("ICP one pass, 300000 sources: reference noise floor of the translation column far from the origin", floor, "tolerance", tol)
    for off, r, ref in cases:
        err_r, err_t = np.abs(r.T[:3, :3] - ref[0][:3, :3]).max(), np.abs(r.T[:3, 3] - ref[0][:3, 3]).max()
        print("ICP one pass at", off, "rotation error", err_r, "translation error", err_t, "fitness", r.fitness, ref[1])
        assert r.iterations == 1 and r.reason_name == "MAX_ITERATIONS" and r.n_correspondences == ref[2] == len(src)
        assert abs(r.fitness - ref[1]) <= 1e-9 * ref[1]
        assert np.array_equal(r.T[3], [0, 0, 0, 1]) and err_r < 1e-9, (off, err_r)
        assert err_t < (1e-9 if off == OFFSETS[0] else tol), (off, err_t, tol)


@pytest.mark.gpu
def test_icp_ten_iterations_recover_a_small_misalignment_on_the_map(sg_ctx, big_map):
    """300 000 points of the map moved by the inverse of G (1e-4 rad, a few mm: within half the point spacing, so the
    correspondences are the true ones after the first passes); the run stops where icp_numpy stops, at G"""
    G = rigid(1e-4, -0.8e-4, 1.2e-4, [0.005, -0.004, 0.003])
    rng = np.random.default_rng(22)
    pick = rng.permutation(len(big_map))[:300000]
    src = on_grid(a2(np.linalg.inv(G), big_map[pick]))
    for off in OFFSETS:
        s, t = translated(src, off), translated(big_map, off)
        r = sg_ctx.icpAlign(_pts(s), _pts(t), max_iterations=10)
        ref = icp_numpy(s, t, max_iterations=10)
        ang, tr = rot_trans_err(conjugated(r.T, off), G)
        print("ICP 10 iterations at", off, r.reason_name, r.iterations, "angle", ang, "translation", tr,
              "|T - ref|", np.abs(conjugated(r.T, off) - conjugated(ref[0], off)).max())
        assert ref[4] in UNCHANGED_OR_SMALL and r.reason_name == ref[4] and r.iterations == ref[3], (off, r, ref[3:])
        assert r.n_correspondences == ref[2] == len(src)
        assert ang < 1e-4 and tr < 1e-3, (off, ang, tr)
        assert np.abs(conjugated(r.T, off) - conjugated(ref[0], off)).max() < 1e-6
        assert abs(r.fitness - ref[1]) <= 1e-6 * max(ref[1], 1e-12) + 1e-12


@pytest.mark.gpu
def test_icp_source_counts_at_wave_and_workgroup_edges(sg_ctx):
    tgt = on_grid(synthetic_surface(5000, 23))
    rng = np.random.default_rng(24)
    for off in (OFFSETS[0], OFFSETS[2]):
        t = translated(tgt, off)
        floor, rows = 0.0, []
        for n in (3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025):
            s = translated(on_grid(tgt[rng.permutation(len(tgt))[:n]].astype(np.float64) + rng.normal(0, 0.01, (n, 3))), off)
            r = sg_ctx.icpAlign(_pts(s), _pts(t), max_iterations=1)
            idx, d2 = nn_brute(s, t)
            Ta, deg = kabsch(s, t[idx])
            Tb, _ = kabsch_centred(s, t[idx], (t.min(0).astype(np.float64) + t.max(0).astype(np.float64)) / 2)
            assert not deg and r.iterations == 1 and r.n_correspondences == n
            floor = max(floor, float(np.abs(Ta[:3, 3] - Tb[:3, 3]).max()))
            rows.append((n, r, Ta))
        tol = 1e-9 if off == OFFSETS[0] else 16 * floor
        print("ICP edge counts at", off, "reference floor", floor, "translation tolerance", tol, "largest error",
              max(np.abs(r.T[:3, 3] - Ta[:3, 3]).max() for _, r, Ta in rows))
        for n, r, Ta in rows:
            assert np.abs(r.T[:3, :3] - Ta[:3, :3]).max() < 1e-9, (off, n)
            assert np.abs(r.T[:3, 3] - Ta[:3, 3]).max() < tol, (off, n, np.abs(r.T[:3, 3] - Ta[:3, 3]).max(), tol)


@pytest.mark.gpu
def test_icp_partials_of_workgroups_without_correspondences(sg_ctx):
    """1024 sources = 4 workgroups, most of them 100 m from the target with max_correspondence_distance 0.05: only the last
    lane of the last workgroup / only the last three lanes / only workgroup 0 / only workgroup 2 has correspondences"""
    tgt = on_grid(synthetic_surface(5000, 25))
    rng = np.random.default_rng(26)
    near = on_grid(tgt[rng.permutation(len(tgt))[:1024]].astype(np.float64) + rng.normal(0, 0.004, (1024, 3)))
    for off in (OFFSETS[0], OFFSETS[2]):
        t = translated(tgt, off)
        centre = (t.min(0).astype(np.float64) + t.max(0).astype(np.float64)) / 2
        floor, rows = 0.0, []
        for name, keep in (("last lane", slice(1023, 1024)), ("last three", slice(1021, 1024)), ("workgroup 0", slice(0, 256)),
                           ("workgroup 2", slice(512, 768)), ("lane 0 of each", slice(0, 1024, 256))):
            s = near + F32([0, 0, 100])
            s[keep] = near[keep]
            s = translated(s, off)
            for _ in range(2):  # the second call runs on the first call's buffers
                r = sg_ctx.icpAlign(_pts(s), _pts(t), max_iterations=1, max_correspondence_distance=0.05)
                idx, d2 = nn_brute(s, t, 0.05)
                m = idx != NONE
                assert m.sum() == len(near[keep]), (name, off)
                if m.sum() < 3:
                    assert r.reason_name == "TOO_FEW" and r.iterations == 0 and np.array_equal(r.T, np.eye(4)) and r.n_correspondences == 1
                    assert r.fitness == pytest.approx(d2[m].astype(np.float64).mean(), rel=1e-12), (name, off)
                    continue
                Ta, deg = kabsch(s[m], t[idx[m]])
                Tb, _ = kabsch_centred(s[m], t[idx[m]], centre)
                floor = max(floor, float(np.abs(Ta[:3, 3] - Tb[:3, 3]).max()))
                ref = icp_numpy(s, t, None, 1, 0.05, nn=nn_brute)  # count and fitness are those of the pass after the step
                assert not deg and r.reason_name == "MAX_ITERATIONS" and r.n_correspondences == ref[2] == m.sum()
                assert abs(r.fitness - ref[1]) <= 1e-9 * ref[1], (name, off)
                rows.append((name, r, Ta))
        tol = 1e-9 if off == OFFSETS[0] else 16 * floor
        print("ICP sparse workgroups at", off, "reference floor", floor, "translation tolerance", tol, "largest error",
              max(np.abs(r.T[:3, 3] - Ta[:3, 3]).max() for _, r, Ta in rows))
        for name, r, Ta in rows:
            assert np.abs(r.T[:3, :3] - Ta[:3, :3]).max() < 1e-9, (name, off)
            assert np.abs(r.T[:3, 3] - Ta[:3, 3]).max() < tol, (name, off, np.abs(r.T[:3, 3] - Ta[:3, 3]).max(), tol)


@pytest.mark.gpu
def test_icp_is_deterministic_at_300000_sources(sg_ctx, big_map):
    src = big_queries(big_map, 300000, 27, sigma=0.004)
    s, t = translated(src, OFFSETS[1]), translated(big_map, OFFSETS[1])
    a = sg_ctx.icpAlign(_pts(s), _pts(t), max_iterations=2, max_correspondence_distance=0.008)
    b = sg_ctx.icpAlign(_pts(s), _pts(t), max_iterations=2, max_correspondence_distance=0.008)
    d = sg_ctx.icpAlign(_torch_pts(_pts(s)), _torch_pts(_pts(t)), max_iterations=2, max_correspondence_distance=0.008)
    assert 1000 < a.n_correspondences < len(s) and a.iterations == 2
    assert _icp_bits(a) == _icp_bits(b) == _icp_bits(d)


# ---- MLS ------------------------------------------------------------------------------------------------------------------
def _mls(ctx, xyz, r, order=2):
    pts = _pts(xyz, np.arange(len(xyz), dtype=np.uint32) * np.uint32(2654435761))
    out, nrm, cnt, fit, info = ctx.mlsSmooth(pts, r, order, return_normals=True, return_info=True)
    assert info.n_poly == (fit == POLY).sum() and info.n_plane == (fit == PLANE).sum() and info.n_none == (fit == MLS_NONE).sum()
    assert info.max_neighbors == (cnt.max() if len(cnt) else 0)
    assert np.array_equal(out["rgba"], pts["rgba"])
    return out, nrm, cnt, fit


def _out_xyz(out):
    return np.stack([out["x"], out["y"], out["z"]], 1)


def _check_mls_translation(base, got, off, what):
    """k and fit kinds exactly; the points minus the offset within one fp32 ulp at the translated magnitude (what the
    output's rounding permits) plus, for z, what the fp64 evaluation itself permits.  z is not translated, so its ulp is at
    its own magnitude and shrinks to nothing where a fit cancels to z ~ 0; but the second pass forms p - m with m rounded
    to fp64 at the translated magnitude M, so the fitted height carries errors of the order of np.spacing(M) (2.3e-13 at
    1024, 1.8e-12 at 8192) whatever z is.  z gets 16 of those steps on top of its ulp - the factor the ICP translation
    tolerance uses for the same kind of floor - which is 3.6e-12 / 2.9e-11 m, far below one ulp of any |z| > 1e-4.
    (Observed on the 480 000-point map at order 2: 6 points with |z| < 2e-8 differ by up to 3.3e-14 at 1024.)"""
    (o0, _, c0, f0), (o1, _, c1, f1) = base, got
    assert np.array_equal(c0, c1) and np.array_equal(f0, f1), (what, np.nonzero((c0 != c1) | (f0 != f1))[0][:10])
    a, b = _out_xyz(o0).astype(np.float64), _out_xyz(o1).astype(np.float64)
    b[:, 0] -= off[0]
    b[:, 1] -= off[1]
    ulp = np.spacing(np.abs(_out_xyz(o1))).astype(np.float64)
    err = np.abs(a - b)
    if not len(err):
        return 0.0
    eval_floor = 16 * float(np.spacing(np.abs(_out_xyz(o1)[:, :2]).astype(np.float64).max()))
    assert (err[:, :2] <= ulp[:, :2]).all(), (what, (err[:, :2] / ulp[:, :2]).max())
    assert (err[:, 2] <= ulp[:, 2] + eval_floor).all(), (what, (err[:, 2] - ulp[:, 2]).max(), eval_floor)
    return float((err[:, :2] / ulp[:, :2]).max())


@pytest.mark.gpu
@pytest.mark.parametrize("order", [0, 1, 2])
def test_mls_map_scale_at_every_translation(sg_ctx, big_map, order):
    """480 000 points at r = 0.1 (two voxels): the contract's tolerances through check_against_numpy (its reference worked
    through in slices of 60 000), at most 0.1 % of the points set aside by it, and the far results against the untranslated"""
    base = None
    for off in OFFSETS:
        xyz = translated(big_map, off)
        got = _mls(sg_ctx, xyz, 0.1, order)
        obs = _checked(xyz, got, 0.1, order, chunk=MLS_CHUNK)
        print("MLS map, order", order, "at", off, obs)
        if base is None:
            base = got
        else:
            print("MLS map, order", order, "at", off, "largest shift of x / y against the untranslated call (ulps there)",
                  _check_mls_translation(base, got, off, (order, off)))


@pytest.mark.gpu
def test_mls_skewed_density(sg_ctx):
    """clump points with thousands of neighbours (long fp64 moment sums), sparse points with fewer than 3 (no fit)"""
    xyz0 = skewed(8000, 31)
    base = {}
    for off in OFFSETS:
        xyz = translated(xyz0, off)
        for order in (0, 2):
            got = _mls(sg_ctx, xyz, 0.3, order)
            clump = ((xyz0[:, :2] >= 0) & (xyz0[:, :2] <= 1)).all(1)
            assert np.median(got[2][clump]) > 1000 and (got[2][~clump] < 3).mean() > 0.9 and (got[3][got[2] < 3] == MLS_NONE).all()
            obs = _checked(xyz, got, 0.3, order, chunk=500)
            print("MLS skewed, order", order, "at", off, obs)
            if off == OFFSETS[0]:
                base[order] = got
            else:
                _check_mls_translation(base[order], got, off, ("skewed", order, off))


@pytest.mark.gpu
def test_mls_degenerate_clouds(sg_ctx):
    """lines, copies and two points come back unfitted and unchanged with NaN normals; the wall meets the contract's
    tolerances; the lattice's neighbour counts (every distance a tie, r on a tie) are exact; all at every translation"""
    lattice_r = 2.0 / 128
    radius = dict(line_x=0.5, line_y=0.5, diagonal=0.5, copies=0.1, two_points=2.0, wall=0.3, lattice=lattice_r)
    base = {}
    for name, xyz0 in degenerate().items():
        for off in OFFSETS:
            xyz, r = translated(xyz0, off), radius[name]
            k_ref = neighbours(xyz, r)[2].sum(1)
            for order in (0, 2):
                out, nrm, cnt, fit = got = _mls(sg_ctx, xyz, r, order)
                assert np.array_equal(cnt, k_ref), (name, off, np.nonzero(cnt != k_ref)[0][:10])
                if name in ("line_x", "line_y", "diagonal", "copies", "two_points"):
                    assert (fit == MLS_NONE).all() and np.isnan(nrm).all(), (name, off)
                    assert np.array_equal(_out_xyz(out).view(np.uint32), xyz.view(np.uint32)), (name, off)
                    assert cnt.max() >= 2 and (name != "copies" or (cnt == 4000).all())
                elif name == "wall":
                    print("MLS wall, order", order, "at", off, _checked(xyz, got, r, order))
                else:
                    assert cnt.max() == 13 + 2 * 9 and cnt.min() == 6 + 5  # sites within 2 steps in a slab three sites thick
                if off == OFFSETS[0]:
                    base[name, order] = got
                elif name != "lattice":  # (the lattice's eigenvalues tie: its fits are not compared)
                    _check_mls_translation(base[name, order], got, off, (name, order, off))
                else:
                    assert np.array_equal(base[name, order][2], cnt)


@pytest.mark.gpu
def test_mls_counts_at_wave_and_workgroup_edges(sg_ctx):
    pool = map_like(20, 13, COUNT_POOL_SEED)
    for n in (1, 2, 3, 5, 6, 63, 64, 65, 255, 256, 257):
        for off in (OFFSETS[0], OFFSETS[2]):
            xyz = translated(pool[:n], off)
            for order in (0, 1, 2):
                _checked(xyz, _mls(sg_ctx, xyz, COUNT_R, order), COUNT_R, order)
    for n in (5, 6):  # everything within r: k == n, on either side of the six coefficients of order 2
        xyz = translated(on_grid(HAND_POINTS)[:n], OFFSETS[2])
        got = _mls(sg_ctx, xyz, 1.0, 2)
        assert (got[2] == n).all() and (got[3] == (POLY if n == 6 else PLANE)).all()
        _checked(xyz, got, 1.0, 2)


@pytest.mark.gpu
def test_mls_window_clamped_to_the_box_and_radius_below_one_ulp(sg_ctx):
    """r larger than the cloud's whole extent in y (every window is clamped to the box on both sides, points on the box's
    faces included), and r smaller than one fp32 step of the far-translated coordinates (the window's pad adds nothing
    there: k still counts the point itself and its exact duplicates)"""
    strip = map_like(400, 6, 34)  # 20 m x 0.3 m
    for off in OFFSETS:
        xyz = translated(strip, off)
        for order in (0, 2):
            obs = _checked(xyz, _mls(sg_ctx, xyz, 0.35, order), 0.35, order)
            print("MLS strip, order", order, "at", off, obs)
    rng = np.random.default_rng(35)
    base = map_like(60, 50, 36)
    dup = np.concatenate([base, base[::3], base[::3], base[:7]])
    dup = dup[rng.permutation(len(dup))]
    want = np.unique(dup, axis=0, return_inverse=True, return_counts=True)
    want = want[2][want[1].reshape(-1)]
    for off in OFFSETS:
        xyz = translated(dup, off)
        for r in (1e-5, 2.0**-12, 1e-18):  # all below the 2^-10 grid: only exact duplicates are neighbours
            out, nrm, cnt, fit = _mls(sg_ctx, xyz, r, 2)
            assert np.array_equal(cnt, want), (off, r, np.nonzero(cnt != want)[0][:10])
            _, _, mask = neighbours(xyz, r)
            assert np.array_equal(cnt, mask.sum(1))
            assert (fit == MLS_NONE).all() and np.array_equal(_out_xyz(out).view(np.uint32), xyz.view(np.uint32))


# ---- plane segmentation and meshing: what of them is invariant under an exact translation ------------------------------------
@pytest.mark.gpu
def test_plane_tiling_under_exact_translations_and_against_numpy_far_out(sg_ctx):
    """offsets that are multiples of tile_size: the tiles' point counts, order and every point's tile ordinal are the
    untranslated call's, the tile indices shift by offset / tile_size.  Equality of hypotheses, samples and inliers across
    translations, which was first asked for, cannot hold under the contract: a tile's draws are splitmix64(seed ^ key)
    with key = (iy << 32 | ix), so moving the cloud by whole tiles changes every draw (and the fp32 score rounds at the
    coordinates' magnitude).  They are checked against the restatement at (-8192, 8192) instead."""
    from test_plane_segmentation import OK, _check_labels, _check_record, plane_numpy, tiles_numpy
    xyz0 = map_like(200, 150, 41)
    s, thr, H, seed = 2.0, 0.02, 48, 0xC0FFEE
    base = None
    for off in OFFSETS:
        xyz = translated(xyz0, off)
        pts = _pts(xyz)
        inl, tiles, prj, til = sg_ctx.segmentPlane(pts, thr, H, s, seed, False, project=True, return_tile_index=True)
        if base is None:
            base = (tiles.copy(), til.copy())
            assert len(tiles) == 5 * 4 and tiles["n_points"].sum() == len(xyz)
        assert len(tiles) == len(base[0]) and np.array_equal(til, base[1]) and np.array_equal(tiles["n_points"], base[0]["n_points"])
        assert np.array_equal(tiles["ix"], base[0]["ix"] + int(off[0] / s)) and np.array_equal(tiles["iy"], base[0]["iy"] + int(off[1] / s))
        if off == OFFSETS[1]:
            continue
        tl = tiles_numpy(xyz, s)
        assert len(tl) == len(tiles)
        for k, (ix, iy, key, idx) in enumerate(tl):
            assert (tiles["ix"][k], tiles["iy"][k]) == (ix, iy) and (til[idx] == k).all()
            r = plane_numpy(xyz[idx], thr, H, seed, key, optimize=False)
            assert r["status"] == OK
            _check_record(tiles[k], r, idx, exact_coeff=True)  # without the refinement every value is correctly rounded
        _check_labels(pts, thr, inl, prj, tiles, [idx for *_, idx in tl])
        # with the refinement: the labels and the projection follow the returned coefficients bit for bit
        inl, tiles2, prj, til2 = sg_ctx.segmentPlane(pts, thr, H, s, seed, True, project=True, return_tile_index=True)
        assert np.array_equal(til2, til) and np.array_equal(tiles2["hypothesis"], tiles["hypothesis"]) and (tiles2["refined"] == 1).all()
        _check_labels(pts, thr, inl, prj, tiles2, [idx for *_, idx in tl])


@pytest.mark.gpu
def test_mesh_under_exact_translations_and_against_numpy_far_out(sg_ctx):
    """cell_size 2^-4 (so x / cell_size is exact at every magnitude) and offsets that are multiples of it: the triangle
    list, the counts and the normals are the untranslated call's bit for bit; at cell_size 0.05 the mesh far out equals the
    restatement"""
    from test_mesh_surface import _check_equal
    xyz0 = map_like(300, 200, 42)
    base = None
    for off in OFFSETS:
        xyz = translated(xyz0, off)
        t, nrm, info = _check_equal(sg_ctx, xyz, 0.0625, 0.2)
        if base is None:
            base = (t, nrm, info)
            assert info.n_triangles > 50000 and info.n_shadowed > 1000
        assert np.array_equal(t, base[0]) and info.__dict__ == base[2].__dict__
        assert np.array_equal(nrm.view(np.uint32), base[1].view(np.uint32))
    _, _, info = _check_equal(sg_ctx, translated(xyz0, OFFSETS[2]), 0.05, np.inf)
    assert info.n_triangles > 50000
