"""The contracts of o3dr_raster_interpolate and o3dr_raster_sample (include/o3dr_dem.h) restated in numpy, operation for
operation: every fp64 sum in the contract's order, every rounding to fp32 where the contract rounds.  Whole levels at a
time (pad and slice), no tiling: what the kernels must reproduce bit for bit."""
import numpy as np

F32, F64 = np.float32, np.float64
NAN_BITS = 0x7FC00000
NAN = np.array([NAN_BITS], np.uint32).view(F32)[0]
MAX_LEVELS = 32
KIDS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (i, j): the child (2X + i, 2Y + j)


def level_shapes(width, height):
    """[(W_l, H_l)] for l = 0 .. L"""
    shapes = [(int(width), int(height))]
    while shapes[-1] != (1, 1):
        w, h = shapes[-1]
        shapes.append(((w + 1) >> 1, (h + 1) >> 1))
    return shapes


def pull(raster):
    """-> (c, m): per level the int32 counts and the fp32 means (steps 1 and 2)"""
    Z = np.ascontiguousarray(raster, F32)
    data = ~np.isnan(Z)
    c, m = [data.astype(np.int32)], [np.where(data, Z, F32(0.0))]
    while c[-1].shape != (1, 1):
        h, w = c[-1].shape
        h2, w2 = (h + 1) >> 1, (w + 1) >> 1
        cp, mp = np.zeros((2 * h2, 2 * w2), np.int32), np.zeros((2 * h2, 2 * w2), F32)  # a child outside: c = 0, m = +0.0f
        cp[:h, :w], mp[:h, :w] = c[-1], m[-1]
        n, s = np.zeros((h2, w2), np.int32), np.zeros((h2, w2), F64)
        for i, j in KIDS:
            ck, mk = cp[j::2, i::2], mp[j::2, i::2]
            n = n + ck
            s = s + ck.astype(F64) * mk.astype(F64)
        mean = (s / np.maximum(n, 1).astype(F64)).astype(F32)
        c.append(n)
        m.append(np.where(n > 0, mean, F32(0.0)))
    return c, m


def _parents(n, n_up):
    x = np.arange(n)
    X = x >> 1
    Xn = np.clip(np.where(x & 1, X + 1, X - 1), 0, n_up - 1)
    return X, Xn


def sweep(G, fixed):
    """one Jacobi sweep over a level (step 4): the cells that are not fixed take the mean of their neighbours"""
    h, w = G.shape
    pad, one = np.zeros((h + 2, w + 2), F64), np.zeros((h + 2, w + 2), np.int32)  # a neighbour outside adds +0.0, is not counted
    pad[1:-1, 1:-1], one[1:-1, 1:-1] = G.astype(F64), 1
    s = ((pad[:-2, 1:-1] + pad[1:-1, :-2]) + pad[1:-1, 2:]) + pad[2:, 1:-1]  # up, left, right, down
    k = ((one[:-2, 1:-1] + one[1:-1, :-2]) + one[1:-1, 2:]) + one[2:, 1:-1]
    new = np.where(k > 0, (s / np.maximum(k, 1).astype(F64)).astype(F32), G)
    return np.where(fixed, G, new)


def push(c, m, smooth):
    """-> F_0 (step 4)"""
    F = m[-1]
    for l in range(len(c) - 2, -1, -1):
        h, w = c[l].shape
        hu, wu = F.shape
        X, Xn = _parents(w, wu)
        Y, Yn = _parents(h, hu)
        Fd = F.astype(F64)
        a, b = Fd[Y[:, None], X[None, :]], Fd[Y[:, None], Xn[None, :]]
        cc, d = Fd[Yn[:, None], X[None, :]], Fd[Yn[:, None], Xn[None, :]]
        P = ((((9.0 * a + 3.0 * b) + 3.0 * cc) + d) * 0.0625).astype(F32)
        fixed = c[l] > 0
        G = np.where(fixed, m[l], P)
        for _ in range(smooth):
            G = sweep(G, fixed)
        F = G
    return F


def levels_of(c):
    """the level output (step 5): 0 on a data cell, the smallest l >= 1 with data under the cell's ancestor, 255 if none"""
    h, w = c[0].shape
    x, y = np.arange(w), np.arange(h)
    lev = np.where(c[0] > 0, 0, 255).astype(np.uint8)
    for l in range(1, len(c)):
        has = c[l][(y >> l)[:, None], (x >> l)[None, :]] > 0
        lev = np.where((lev == 255) & has, l, lev).astype(np.uint8)
    return lev


def interpolate(raster, smooth=2, max_level=0):
    """-> (filled float32 [H, W], level uint8 [H, W], info dict)"""
    Z = np.ascontiguousarray(raster, F32)
    assert Z.ndim == 2 and Z.size > 0 and 0 <= smooth <= 8 and 0 <= max_level <= 31 and not np.isinf(Z).any()
    c, m = pull(Z)
    lev = levels_of(c)
    if c[-1][0, 0] == 0:  # step 3
        filled = np.full(Z.shape, NAN, F32)
        by_level = [0] * MAX_LEVELS
    else:
        filled = push(c, m, smooth).copy()
        by_level = [int((lev == l).sum()) for l in range(MAX_LEVELS)]
    hole = lev != 0
    empty = hole & ((lev == 255) | ((max_level > 0) & (lev > max_level)))
    filled[empty] = NAN
    info = dict(width=Z.shape[1], height=Z.shape[0], n_levels=len(c), n_data=int((~hole).sum()), n_filled=int((hole & ~empty).sum()),
                n_empty=int(empty.sum()), n_by_level=by_level)
    return filled, lev, info


def cells_of(xyz, cell_size):
    """the map raster's step 1: (cx, cy) int64 per point"""
    inv = F32(1.0) / F32(cell_size)
    xyz = np.asarray(xyz, F32)
    return np.floor(xyz[:, 0] * inv).astype(np.int64), np.floor(xyz[:, 1] * inv).astype(np.int64)


def sample(xyz, raster, cell_size, bounds):
    """-> (value float32 [n], height_above float32 [n], (inside, outside, on a NaN cell))"""
    xyz, raster = np.asarray(xyz, F32).reshape(-1, 3), np.ascontiguousarray(raster, F32)
    cx0, cy0, W, H = (int(v) for v in bounds)
    assert raster.shape == (H, W)
    cx, cy = cells_of(xyz, cell_size)
    dx, dy = cx - cx0, cy - cy0
    inside = (dx >= 0) & (dx < W) & (dy >= 0) & (dy < H)
    value = np.full(len(xyz), NAN, F32)
    got = raster[dy[inside], dx[inside]]
    value[inside] = np.where(np.isnan(got), NAN, got)
    ok = ~np.isnan(value)
    above = np.full(len(xyz), NAN, F32)
    above[ok] = xyz[ok, 2] - value[ok]
    return value, above, (int(inside.sum()), int((~inside).sum()), int((inside & ~ok).sum()))


# ---- the quality scene of tests/test_interpolate_reference.py (and profiles/interpolate_probe.py's small case) -------------
def quality_scene(height=300, width=420, seed=7, extra_random=0.0):
    """undulating terrain with 0.02 noise and 14 rectangular holes of 10 .. 89 cells a side -> (noisy raster with NaN
    holes, the noise-free surface, the hole mask)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:height, 0:width].astype(F64)
    truth = 2.0 * np.sin(x / 60.0) * np.cos(y / 45.0) + 0.01 * x
    Z = (truth + rng.normal(0.0, 0.02, truth.shape)).astype(F32)
    hole = np.zeros(Z.shape, bool)
    for _ in range(14):
        w, h = (int(v) for v in rng.integers(10, 90, 2))
        x0, y0 = int(rng.integers(0, width - w + 1)), int(rng.integers(0, height - h + 1))
        hole[y0:y0 + h, x0:x0 + w] = True
    if extra_random > 0:
        hole |= rng.random(Z.shape) < extra_random
    Z[hole] = NAN
    return Z, truth.astype(F32), hole


def nearest_fill(Z):
    """every hole takes its nearest data cell (scipy's Euclidean distance transform)"""
    from scipy import ndimage
    hole = np.isnan(Z)
    idx = ndimage.distance_transform_edt(hole, return_distances=False, return_indices=True)
    return Z[tuple(idx)]


def rms_in_holes(filled, truth, hole):
    d = filled[hole].astype(F64) - truth[hole].astype(F64)
    return float(np.sqrt((d * d).mean()))
