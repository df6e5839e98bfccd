"""The map raster's contract (include/o3dr.h "map raster") restated in numpy, operation for operation: fp32 cells, one
point per cell by `select`, the hole fill as its plain definition (a search over the disc in the order of the tie rule,
not the separable passes the GPU runs), the four output images, the fp64 shaded relief and the counts.  numpy never fuses
a multiply-add, every value is an integer, a comparison, a copy or a correctly rounded fp64 operation in the stated
order, so the GPU must match bit for bit."""
from types import SimpleNamespace

import numpy as np

F32 = np.float32
MAX_FILL_RADIUS, MAX_CELLS = 32, 1 << 28


def cells_of(xyz, cell_size):
    """cx, cy (int64) by the mesh's rule: floorf(x * inv) in fp32, inv = 1.0f / (float)cell_size"""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    inv = F32(1.0) / F32(cell_size)
    return np.floor(xyz[:, 0] * inv).astype(np.int64), np.floor(xyz[:, 1] * inv).astype(np.int64)


def extent(xyz, cell_size):
    """the cloud's own cell box (cx0, cy0, width, height)"""
    cx, cy = cells_of(xyz, cell_size)
    assert len(cx) > 0, "an empty cloud has no cell box"
    return int(cx.min()), int(cy.min()), int(cx.max() - cx.min()) + 1, int(cy.max() - cy.min()) + 1


def disc_offsets(R):
    """(dy, dx, d2) of every cell offset with 0 < d2 <= R*R, in the order a target prefers its sources: the smallest d2,
    then the lowest cy, then the lowest cx"""
    o = [(dy * dy + dx * dx, dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if 0 < dy * dy + dx * dx <= R * R]
    return [(dy, dx, d) for d, dy, dx in sorted(o)]


def rasterize(xyz, rgba, cell_size, bounds=None, select="first", fill_radius=0, light=None):
    """-> namespace: height_map, color, shade (None without a light), source, distance2 and info (a dict of the result
    record's fields)"""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    rgba = np.asarray(rgba, np.uint32).reshape(-1)
    n, R = len(xyz), int(fill_radius)
    assert 0 <= R <= MAX_FILL_RADIUS and select in ("first", "top", "bottom")
    cx0, cy0, W, H = extent(xyz, cell_size) if bounds is None else (int(v) for v in bounds)
    assert W >= 1 and H >= 1 and W * H <= MAX_CELLS
    cx, cy = cells_of(xyz, cell_size)
    inside = (cx >= cx0) & (cx < cx0 + W) & (cy >= cy0) & (cy < cy0 + H)
    idx = np.nonzero(inside)[0]
    cell = (cy[idx] - cy0) * W + (cx[idx] - cx0)
    # one point per cell: sort by (cell, z rule, index) and keep the first of every cell
    z = xyz[idx, 2] + F32(0)  # -0.0f + 0.0f = 0.0f: the two zeros compare equal and order as one value
    zkey = np.zeros(len(idx), F32) if select == "first" else (-z if select == "top" else z)
    order = np.lexsort((idx, zkey, cell))
    head = np.ones(len(idx), bool)
    head[1:] = cell[order][1:] != cell[order][:-1]
    own = np.full(W * H, -1, np.int64)
    own[cell[order][head]] = idx[order][head]
    own = own.reshape(H, W)
    occupied = own >= 0
    # hole fill, the plain definition: every empty cell looks through the disc in its order of preference
    source, distance2 = own.copy(), np.where(occupied, 0, -1).astype(np.int64)
    if R > 0 and occupied.any() and not occupied.all():
        pad = np.full((H + 2 * R, W + 2 * R), -1, np.int64)
        pad[R:R + H, R:R + W] = own
        for dy, dx, d in disc_offsets(R):
            cand = pad[R + dy:R + dy + H, R + dx:R + dx + W]
            take = (source < 0) & (cand >= 0)
            source[take] = cand[take]
            distance2[take] = d
    has = source >= 0
    safe = np.maximum(source, 0)
    height_map = np.where(has, xyz[safe, 2] if n else F32(0), F32(np.nan)).astype(F32)
    if n:
        height_map[has] = xyz[source[has], 2]  # a copy: the sign of a zero survives
    color = np.zeros((H, W, 3), np.uint8)
    if n:
        c = rgba[safe]
        color = np.where(has[..., None], np.stack([c & 255, (c >> 8) & 255, (c >> 16) & 255], -1), 0).astype(np.uint8)
    shade = None
    if light is not None:
        lx, ly, lz = (np.float64(v) for v in light)
        ln = np.sqrt((lx * lx + ly * ly) + lz * lz)
        assert np.isfinite(ln) and ln > 0
        shade = shade_of(height_map, has, float(cell_size), lx / ln, ly / ln, lz / ln)
    zo = xyz[own[occupied], 2] + F32(0) if n else np.zeros(0, F32)
    n_in, n_occ = int(inside.sum()), int(occupied.sum())
    info = dict(cx0=cx0, cy0=cy0, width=W, height=H, n_inside=n_in, n_outside=n - n_in, n_occupied=n_occ, n_shadowed=n_in - n_occ,
                n_filled=int((distance2 > 0).sum()), n_empty=int((~has).sum()),
                z_min=float(zo.min()) if n_occ else float("nan"), z_max=float(zo.max()) if n_occ else float("nan"))
    return SimpleNamespace(height_map=height_map, color=color, shade=shade, source=source.astype(np.int32),
                           distance2=distance2.astype(np.int32), info=info)


def shade_of(height_map, has, cell_size, lx, ly, lz):
    """step 5 of the contract on the filled heights; (lx, ly, lz) normalised"""
    H, W = height_map.shape
    h = height_map.astype(np.float64)

    def neighbour(dr, dc):
        """the neighbour's height where it is inside the raster and has a source, else the cell's own; and which it was"""
        nb, ok = h.copy(), np.zeros((H, W), bool)
        dst = (slice(max(0, -dr), H - max(0, dr)), slice(max(0, -dc), W - max(0, dc)))
        src = (slice(max(0, dr), H - max(0, -dr)), slice(max(0, dc), W - max(0, -dc)))
        ok[dst] = has[src]
        nb[dst] = np.where(has[src], h[src], h[dst])
        return nb, ok

    hR, okR = neighbour(0, 1)
    hL, okL = neighbour(0, -1)
    hU, okU = neighbour(1, 0)
    hD, okD = neighbour(-1, 0)
    kx, ky = okR.astype(np.int64) + okL, okU.astype(np.int64) + okD
    with np.errstate(invalid="ignore", divide="ignore"):
        gx = np.where(kx == 0, 0.0, (hR - hL) / (kx.astype(np.float64) * np.float64(cell_size)))
        gy = np.where(ky == 0, 0.0, (hU - hD) / (ky.astype(np.float64) * np.float64(cell_size)))
        s = (((-gx) * lx + (-gy) * ly) + lz) / np.sqrt((gx * gx + gy * gy) + 1.0)
        t = np.floor(s * 254.0 + 0.5)
    v = np.where(s > 0, np.where(t >= 254.0, 255, 1 + np.where(s > 0, t, 0).astype(np.int64)), 1)
    return np.where(has, v, 0).astype(np.uint8)


def height_png16(height_map, z_min, z_max):
    """the CLI's 16-bit quantisation of the heights: 0 = no data, else 1 + min(65534, floor((z - z_min) / step)) with
    step = max((z_max - z_min) / 65534, 2^-15), in fp64 -> (uint16 image, step)"""
    step = max((np.float64(z_max) - np.float64(z_min)) / 65534.0, 2.0 ** -15) if np.isfinite(z_min) else 2.0 ** -15
    has = ~np.isnan(height_map)
    with np.errstate(invalid="ignore"):
        q = np.floor((height_map.astype(np.float64) - np.float64(z_min)) / step)
    q = np.where(has, 1 + np.clip(np.where(has, q, 0), 0, 65534), 0)
    return q.astype(np.uint16), float(step)
