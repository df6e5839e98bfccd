"""The ground filter's contract (include/o3dr_terrain.h "ground filter") restated in numpy, step for step: the raster's
cells, the minimum surface, the window schedule in fp64, every iteration's window minima and maxima by plain shifted
np.minimum / np.maximum over the live cells, the fp32 removal test, the point mask, the DTM with the raster's fill and
the height above it.  Every value is an integer, a copy, a comparison, a min / max or one fp32 subtraction, so the GPU
must match bit for bit.  The cell rule and the fill are raster_reference's."""
from types import SimpleNamespace

import numpy as np

import raster_reference as rr

F32 = np.float32
MAX_WINDOW_RADIUS, MAX_ITERATIONS = 128, 16


def schedule(cell_size, max_window_radius=16, window_base=2, exponential=True, slope=0.7, initial_distance=0.15, max_distance=10.0):
    """step 3 -> (radii int32, thresholds float32)"""
    assert 1 <= max_window_radius <= MAX_WINDOW_RADIUS and window_base >= (2 if exponential else 1)
    radii, thr = [], []
    for k in range(MAX_ITERATIONS):
        r = window_base ** k if exponential else (k + 1) * window_base
        if r > max_window_radius:
            break
        t = np.float64(initial_distance)
        if k > 0:
            t = np.float64(slope) * (np.float64(2 * (r - radii[-1])) * np.float64(cell_size)) + np.float64(initial_distance)
        radii.append(r)
        thr.append(F32(min(t, np.float64(max_distance))))
    assert radii, "a schedule without an iteration"
    return np.array(radii, np.int32), np.array(thr, F32)


def window(a, r, op, ident):
    """op over the (2r + 1)^2 window of every cell, cells outside the raster being `ident`: one shifted copy per offset,
    along x and then along y"""
    H, W = a.shape
    for axis, size in ((1, W), (0, H)):
        pad = [(0, 0), (0, 0)]
        m = min(r, size - 1)  # (an offset past the raster reaches nothing)
        pad[axis] = (m, m)
        p = np.pad(a, pad, constant_values=ident)
        out = a.copy()
        for d in range(-m, m + 1):
            sl = [slice(None), slice(None)]
            sl[axis] = slice(m + d, m + d + size)
            out = op(out, p[tuple(sl)])
        a = out
    return a


def ground_filter(xyz, cell_size, bounds=None, fill_radius=0, **kw):
    """-> namespace: ground uint8 [n], height_above_ground float32 [n], dtm float32 [H, W], cell_state uint8 [H, W], Z (the
    minimum surface, NaN where empty) and info (a dict of the result record's fields)"""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    n = len(xyz)
    radii, thr = schedule(cell_size, **kw)
    cx0, cy0, W, H = rr.extent(xyz, cell_size) if bounds is None else (int(v) for v in bounds)
    assert W >= 1 and H >= 1 and W * H <= rr.MAX_CELLS
    cx, cy = rr.cells_of(xyz, cell_size)
    inside = (cx >= cx0) & (cx < cx0 + W) & (cy >= cy0) & (cy < cy0 + H)
    idx = np.nonzero(inside)[0]
    cell = (cy[idx] - cy0) * W + (cx[idx] - cx0)
    # step 2: the lowest point per cell, ties to the lowest index, the two zeros as one value
    z = xyz[idx, 2] + F32(0)
    order = np.lexsort((idx, z, cell))
    head = np.ones(len(idx), bool)
    head[1:] = cell[order][1:] != cell[order][:-1]
    own = np.full(W * H, -1, np.int64)
    own[cell[order][head]] = idx[order][head]
    own = own.reshape(H, W)
    occupied = own >= 0
    Z = np.full((H, W), np.nan, F32)
    Z[occupied] = xyz[own[occupied], 2]  # a copy
    state = occupied.astype(np.uint8)
    live = occupied.copy()
    removed = []
    for k, (r, t) in enumerate(zip(radii, thr)):  # step 4
        zl = np.where(live, Z, F32(np.inf)).astype(F32)
        E = np.where(live, window(zl, int(r), np.minimum, F32(np.inf)), F32(-np.inf)).astype(F32)
        O = window(E, int(r), np.maximum, F32(-np.inf))
        with np.errstate(invalid="ignore"):
            diff = (np.where(live, Z, F32(0)) - np.where(live, O, F32(0))).astype(F32)
        rem = live & (diff > t)
        state[rem] = 2 + k
        live &= ~rem
        removed.append(int(rem.sum()))
    ground_cell = state == 1
    # step 6: the raster's fill with the ground cells' points as the only sources (one point per ground cell)
    src = own[ground_cell]
    ras = rr.rasterize(xyz[src], np.zeros(len(src), np.uint32), cell_size, bounds=(cx0, cy0, W, H), select="first", fill_radius=fill_radius)
    dtm = ras.height_map
    assert ras.info["n_occupied"] == int(ground_cell.sum())
    # steps 5 and 7
    ground = np.zeros(n, np.uint8)
    hag = np.full(n, np.nan, F32)
    r_i, c_i = cy[idx] - cy0, cx[idx] - cx0
    with np.errstate(invalid="ignore"):
        d = dtm[r_i, c_i]
        hag[idx] = np.where(np.isnan(d), F32(np.nan), xyz[idx, 2] - d)  # (one NaN: 0x7fc00000, as in the DTM)
        ground[idx] = ground_cell[r_i, c_i] & ((xyz[idx, 2] - Z[r_i, c_i]).astype(F32) <= thr[0])
    info = dict(cx0=cx0, cy0=cy0, width=W, height=H, n_inside=len(idx), n_outside=n - len(idx), n_occupied=int(occupied.sum()),
                n_ground_cells=int(ground_cell.sum()), n_ground_points=int(ground.sum()), n_dtm_filled=ras.info["n_filled"],
                n_dtm_empty=ras.info["n_empty"], n_iterations=len(radii), n_removed=tuple(removed))
    return SimpleNamespace(ground=ground, height_above_ground=hag, dtm=dtm, cell_state=state, Z=Z, info=info)


# ---- the test scene ---------------------------------------------------------------------------------------------------
SCENE_W, SCENE_H, SCENE_CELL = 240, 160, 0.1
SCENE_X0, SCENE_Y0 = -120, -80  # the box's first cell: the scene is centred on the origin
SCENE_BOX = (SCENE_X0, SCENE_Y0, SCENE_W, SCENE_H)
SCENE_PARAMS = dict(max_window_radius=32, slope=0.3, initial_distance=0.15, max_distance=2.0)


def terrain(x, y):
    return 0.03 * x - 0.02 * y + 0.3 * np.sin(0.4 * x) * np.cos(0.3 * y)


def scene(seed):
    """240 x 160 cells of 0.1 m, one point per cell, 10 % of the cells missing: undulating ground with +-0.01 m noise, four
    flat-roofed buildings 3-4 m wide and 2-4 m high, ten 0.4 m posts of 1 m.  The scene is centred on the origin: the
    contract's windows end at the raster's border, so ground that rises towards a border loses up to slope * r * cell_size
    there, and across the borders of this box the terrain rises by at most 0.08 m/m * 3.2 m = 0.26 m, below the linear
    schedule's 0.39 m threshold (from x = 0 .. 24 m it rises by 0.47 m towards the border at x = 24).
    -> namespace: xyz (shuffled), object [H, W] (cells under a building or a post), truth [H, W] (the ground's height at
    the cell centres), present [H, W]"""
    rng = np.random.default_rng(seed)
    W, H, cs = SCENE_W, SCENE_H, SCENE_CELL
    gx, gy = np.meshgrid(np.arange(W), np.arange(H))
    x, y = (gx + 0.5 + SCENE_X0) * cs, (gy + 0.5 + SCENE_Y0) * cs
    truth = terrain(x, y)
    z = truth + rng.uniform(-0.01, 0.01, (H, W))
    obj = np.zeros((H, W), bool)
    for b in range(4):  # one building per quarter of the scene's width: they do not touch
        w, d = rng.integers(30, 41, 2)
        c0 = b * 60 + rng.integers(5, 56 - w)
        r0 = rng.integers(10, H - 10 - d)
        base = terrain((c0 + w / 2 + SCENE_X0) * cs, (r0 + d / 2 + SCENE_Y0) * cs)
        z[r0:r0 + d, c0:c0 + w] = base + rng.uniform(2.0, 4.0)
        obj[r0:r0 + d, c0:c0 + w] = True
    for _ in range(10):
        c0, r0 = rng.integers(2, W - 6), rng.integers(2, H - 6)
        if obj[r0 - 1:r0 + 5, c0 - 1:c0 + 5].any():
            continue
        z[r0:r0 + 4, c0:c0 + 4] = truth[r0:r0 + 4, c0:c0 + 4] + 1.0
        obj[r0:r0 + 4, c0:c0 + 4] = True
    present = rng.random((H, W)) >= 0.1
    u = rng.uniform(-0.4, 0.4, (2, H, W)) * cs
    xyz = np.stack([(x + u[0])[present], (y + u[1])[present], z[present]], 1).astype(F32)
    return SimpleNamespace(xyz=xyz[rng.permutation(len(xyz))], object=obj, truth=truth, present=present)
