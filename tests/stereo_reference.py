"""The stereo-disparity contract of include/o3dr.h ("stereo disparity") in numpy, operation for operation: grey, 9 x 7
census, Hamming cost, semi-global aggregation along 4 or 8 directions, winner with uniqueness, parabola and left-right
check.  Vectorised over the candidates and over the axis across a path; a plain loop runs along the path."""
import numpy as np

DIRECTIONS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int32)
_INF = 1 << 20


def grey(img):
    """step 1: [H, W] stays, [H, W, 3] B G R -> (1868 B + 9617 G + 4899 R + 8192) >> 14"""
    img = np.asarray(img)
    if img.ndim == 2:
        return img.astype(np.int32)
    b, g, r = (img[..., k].astype(np.int64) for k in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.int32)


def census(g):
    """step 2: uint64 [H, W]; neighbour k in the order dy = -3..3 (outer), dx = -4..4 (inner), (0, 0) skipped"""
    H, W = g.shape
    pad = np.pad(g, ((3, 3), (4, 4)), mode="edge")
    out = np.zeros((H, W), np.uint64)
    k = 0
    for dy in range(-3, 4):
        for dx in range(-4, 5):
            if dx == 0 and dy == 0:
                continue
            nb = pad[3 + dy:3 + dy + H, 4 + dx:4 + dx + W]
            out |= (nb < g).astype(np.uint64) << np.uint64(k)
            k += 1
    assert k == 62
    return out


def popcount64(x):
    return _POP8[np.ascontiguousarray(x).view(np.uint8).reshape(x.shape + (8,))].sum(-1)


def cost_volume(cl, cr, D, d0):
    """step 3: int32 [H, W, D]"""
    H, W = cl.shape
    C = np.full((H, W, D), 63, np.int32)
    for d in range(D):
        s = d0 + d
        if s < W:
            C[:, s:, d] = popcount64(cl[:, s:] ^ cr[:, :W - s])
    return C


def _step(Cp, prev, p1, p2):
    """L_r of the pixels Cp [n, D] from their predecessors' prev [n, D]"""
    m = prev.min(-1, keepdims=True)
    lo = np.full_like(prev, _INF)
    hi = np.full_like(prev, _INF)
    lo[:, 1:] = prev[:, :-1]
    hi[:, :-1] = prev[:, 1:]
    return Cp + np.minimum(np.minimum(prev, m + p2), np.minimum(lo, hi) + p1) - m


def path(C, dx, dy, p1, p2):
    """step 4 for one direction of travel: int32 [H, W, D]"""
    H, W, D = C.shape
    L = np.empty_like(C)
    if dy == 0:
        xs = range(W) if dx > 0 else range(W - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(C[:, x], L[:, x - dx], p1, p2)
        return L
    ys = range(H) if dy > 0 else range(H - 1, -1, -1)
    for i, y in enumerate(ys):
        L[y] = C[y]
        if i == 0:
            continue
        # the pixels x whose predecessor (x - dx, y - dy) lies inside the image
        x_lo, x_hi = max(0, dx), W + min(0, dx)
        if x_hi > x_lo:
            L[y, x_lo:x_hi] = _step(C[y, x_lo:x_hi], L[y - dy, x_lo - dx:x_hi - dx], p1, p2)
    return L


def aggregate(C, p1, p2, n_paths):
    """step 5: S, int32 [H, W, D]"""
    S = np.zeros_like(C)
    for dx, dy in DIRECTIONS[:n_paths]:
        S += path(C, dx, dy, p1, p2)
    return S


def winners(S, d0, uniqueness, lr_max_diff):
    """steps 6 and 7 -> disp uint8, disp_q4 uint16, cost uint16 (each [H, W])"""
    H, W, D = S.shape
    best = S.argmin(-1)  # the lowest minimiser
    b = np.take_along_axis(S, best[..., None], -1)[..., 0]
    x = np.arange(W)[None, :]
    xr = x - d0 - best
    rej = xr < 0
    if uniqueness > 0:
        k = np.arange(D)[None, None, :]
        far = np.abs(k - best[..., None]) > 1
        rej |= (far & (S * (100 - uniqueness) < 100 * b[..., None])).any(-1)
    if lr_max_diff >= 0:
        SR = np.full((H, W, D), _INF, np.int64)  # SR[y, xr, d] = S[y, xr + d0 + d, d]
        for d in range(D):
            s = d0 + d
            if s < W:
                SR[:, :W - s, d] = S[:, s:, d]
        bestR = SR.argmin(-1)
        br = np.take_along_axis(bestR, np.clip(xr, 0, W - 1), 1)
        rej |= (xr >= 0) & (np.abs(br - best) > lr_max_diff)
    a = np.take_along_axis(S, np.clip(best - 1, 0, D - 1)[..., None], -1)[..., 0].astype(np.int64)
    c = np.take_along_axis(S, np.clip(best + 1, 0, D - 1)[..., None], -1)[..., 0].astype(np.int64)
    den = a - 2 * b.astype(np.int64) + c
    ok = (best > 0) & (best < D - 1) & (den > 0)
    den1 = np.where(ok, den, 1)
    off = np.where(ok, (16 * (a - c) + den1) // (2 * den1), 0)
    disp = np.where(rej, 0, d0 + best).astype(np.uint8)
    q4 = np.where(rej, 0, 16 * (d0 + best) + off).astype(np.uint16)
    return disp, q4, b.astype(np.uint16)


def stereo_disparity(left, right, n_disparities=256, min_disparity=0, p1=10, p2=120, n_paths=8, uniqueness=10, lr_max_diff=1):
    """One pair ([H, W] grey or [H, W, 3] B G R) -> (disp uint8, disp_q4 uint16, cost uint16, S uint16 [H, W, D])"""
    cl, cr = census(grey(left)), census(grey(right))
    S = aggregate(cost_volume(cl, cr, n_disparities, min_disparity), p1, p2, n_paths)
    disp, q4, cost = winners(S, min_disparity, uniqueness, lr_max_diff)
    return disp, q4, cost, S.astype(np.uint16)


def synthetic_pair(H=64, W=96, t_back=12, t_front=20, rect=(24, 36), seed=7):
    """A right image of smoothed uniform noise and left(x, y) = right(x - t(x, y), y), t = t_back but t_front inside the
    centred rect (rows, cols).  -> (left, right, t) with t int [H, W]"""
    rng = np.random.RandomState(seed)
    # wide enough that x - t never leaves the noise
    noise = rng.randint(0, 256, (H + 2, W + t_front + 2)).astype(np.float64)
    sm = (noise[:-2, :-2] + noise[:-2, 1:-1] + noise[:-2, 2:] + noise[1:-1, :-2] + 2 * noise[1:-1, 1:-1] + noise[1:-1, 2:]
          + noise[2:, :-2] + noise[2:, 1:-1] + noise[2:, 2:]) / 10.0
    wide = np.clip(np.floor(sm + 0.5), 0, 255).astype(np.uint8)  # [H, W + t_front]; right = its columns t_front..
    right = np.ascontiguousarray(wide[:, t_front:])
    t = np.full((H, W), t_back, np.int64)
    y0, x0 = (H - rect[0]) // 2, (W - rect[1]) // 2
    t[y0:y0 + rect[0], x0:x0 + rect[1]] = t_front
    xs = np.arange(W)[None, :] - t + t_front
    left = np.ascontiguousarray(np.take_along_axis(wide, xs, 1))
    return left, right, t
