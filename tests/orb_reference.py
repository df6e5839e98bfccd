"""The ORB contract of include/o3dr.h restated in numpy, stage by stage.  Nothing here comes from the package: the
tests compare the library with these functions exactly (integers and IEEE-exact floats, no tolerances)."""
import numpy as np

M64 = (1 << 64) - 1
PATTERN_SEED = 0x4F5242
RING = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
        (-2, -2), (-1, -3)]
KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("angle_deg", "<f4"), ("size", "<f4"), ("response", "<i8"), ("xl", "<i2"),
                     ("yl", "<i2"), ("level", "u1"), ("angle_bin", "u1"), ("reserved", "<u2")])


def splitmix64(x):
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def directions():
    k = np.arange(64)
    return np.stack([np.round(16384 * np.cos(2 * np.pi * k / 64)), np.round(16384 * np.sin(2 * np.pi * k / 64))], 1).astype(np.int64)


def base_pattern():
    S = splitmix64(PATTERN_SEED)
    n = 0
    tests = []
    while len(tests) < 256:
        v = []
        for _ in range(4):
            s = 0
            for _ in range(4):
                s += (splitmix64((S + n) & M64) >> 32) % 7
                n += 1
            v.append(s - 12)
        if (v[0], v[1]) == (v[2], v[3]) or v[0] ** 2 + v[1] ** 2 > 169 or v[2] ** 2 + v[3] ** 2 > 169:
            continue
        tests.append(v)
    return np.array(tests, np.int64)


_PATTERN = None


def steered_pattern():
    """[64, 256, 4] int8"""
    global _PATTERN
    if _PATTERN is None:
        D, b = directions(), base_pattern()
        out = np.zeros((64, 256, 4), np.int64)
        for h in (0, 2):
            px, py = b[:, h][None, :], b[:, h + 1][None, :]
            out[:, :, h] = (px * D[:, 0:1] - py * D[:, 1:2] + 8192) >> 14
            out[:, :, h + 1] = (px * D[:, 1:2] + py * D[:, 0:1] + 8192) >> 14
        _PATTERN = out.astype(np.int8)
    return _PATTERN


def level_sizes(rows, cols, n_features=1500, scale_factor=1.3, n_levels=5):
    """-> (list of (W_l, H_l), list of quota_l)"""
    s, f = 1.0, float(np.float32(scale_factor))
    wh = []
    for l in range(n_levels):
        sc = 65536 if l == 0 else int(np.floor(65536.0 * s + 0.5))
        w, h = (cols * 65536 + sc // 2) // sc, (rows * 65536 + sc // 2) // sc
        if w == 0 or h == 0:
            w = h = 0
        wh.append((w, h))
        s *= f
    sw = sum(w for w, _ in wh)
    quota = [n_features * w // sw for w, _ in wh]
    quota[0] += n_features - sum(quota)
    return wh, quota


def grey(bgr):
    b, g, r = (bgr[..., i].astype(np.int64) for i in range(3))
    return ((1868 * b + 9617 * g + 4899 * r + 8192) >> 14).astype(np.uint8)


def _axis(n_src, n_dst):
    r = (n_src << 16) // n_dst
    f = np.maximum(0, ((2 * np.arange(n_dst, dtype=np.int64) + 1) * r - 65536) >> 1)
    i0 = np.minimum(f >> 16, n_src - 1)
    i1 = np.minimum(i0 + 1, n_src - 1)
    return i0, i1, (f & 0xFFFF) >> 5


def downsample(src, w, h):
    hs, ws = src.shape
    x0, x1, wx = _axis(ws, w)
    y0, y1, wy = _axis(hs, h)
    s = src.astype(np.int64)
    wx, wy = wx[None, :], wy[:, None]
    v = (s[y0][:, x0] * (2048 - wx) * (2048 - wy) + s[y0][:, x1] * wx * (2048 - wy) + s[y1][:, x0] * (2048 - wx) * wy
         + s[y1][:, x1] * wx * wy)
    return ((v + (1 << 21)) >> 22).astype(np.uint8)


def pyramid(g0, scale_factor=1.3, n_levels=5):
    wh, _ = level_sizes(g0.shape[0], g0.shape[1], 1, scale_factor, n_levels)
    out = [g0]
    for l in range(1, n_levels):
        w, h = wh[l]
        if w == 0:
            break
        out.append(downsample(out[-1], w, h))
    return out


def fast_scores(img, thr):
    """u8 score map: best 9-arc contrast where it exceeds thr, else 0; 0 within 3 pixels of the border"""
    H, W = img.shape
    out = np.zeros((H, W), np.int64)
    if H < 7 or W < 7:
        return out
    I = img.astype(np.int64)
    c = I[3:H - 3, 3:W - 3]
    d = np.stack([I[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - c for dx, dy in RING])
    best = np.full(c.shape, -255, np.int64)
    for sign in (1, -1):
        e = sign * d
        for a in range(16):
            best = np.maximum(best, np.min(e[[(a + i) % 16 for i in range(9)]], axis=0))
    out[3:H - 3, 3:W - 3] = np.where(best > thr, best, 0)
    return out


def candidates(score, edge):
    """kept corners inside the margin, row-major: -> (ys, xs)"""
    H, W = score.shape
    if W <= 2 * edge or H <= 2 * edge:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    p = np.pad(score, 1)
    keep = score > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= p[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] < score
    m = np.zeros_like(keep)
    m[edge:H - edge, edge:W - edge] = True
    return np.nonzero(keep & m)


def harris(img, ys, xs):
    I = np.pad(img.astype(np.int64), 1)
    H, W = img.shape
    sh = lambda dy, dx: I[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]  # noqa: E731
    Ix = 2 * (sh(0, 1) - sh(0, -1)) + (sh(-1, 1) - sh(-1, -1)) + (sh(1, 1) - sh(1, -1))
    Iy = 2 * (sh(1, 0) - sh(-1, 0)) + (sh(1, -1) - sh(-1, -1)) + (sh(1, 1) - sh(-1, 1))
    R = np.zeros(len(ys), np.int64)
    for i, (y, x) in enumerate(zip(ys, xs)):
        wx, wy = Ix[y - 3:y + 4, x - 3:x + 4], Iy[y - 3:y + 4, x - 3:x + 4]
        a, b, c = int((wx * wx).sum()), int((wy * wy).sum()), int((wx * wy).sum())
        R[i] = 25 * (a * b - c * c) - (a + b) ** 2
    return R


def select(R, ys, xs, quota):
    """indices (into the row-major candidate list) of the kept candidates, ascending"""
    order = sorted(range(len(R)), key=lambda i: (-int(R[i]), int(ys[i]), int(xs[i])))
    return np.array(sorted(order[:quota]), np.int64)


_DISC = [(u, v) for v in range(-15, 16) for u in range(-15, 16) if u * u + v * v <= 240]


def orientation(img, y, x):
    """-> (bin, unique): unique is False when the largest dot product is shared by two bins (or the moments vanish)"""
    m10 = sum(u * int(img[y + v, x + u]) for u, v in _DISC)
    m01 = sum(v * int(img[y + v, x + u]) for u, v in _DISC)
    if m10 == 0 and m01 == 0:
        return 0, False
    D = directions()
    dots = [m10 * int(D[k, 0]) + m01 * int(D[k, 1]) for k in range(64)]
    best = max(dots)
    return dots.index(best), dots.count(best) == 1


def box_sums(img):
    I = np.pad(img.astype(np.int64), 2)
    H, W = img.shape
    return sum(I[dy:H + dy, dx:W + dx] for dy in range(5) for dx in range(5))


def describe(box, y, x, bin_):
    t = steered_pattern()[bin_].astype(np.int64)
    bits = box[y + t[:, 1], x + t[:, 0]] < box[y + t[:, 3], x + t[:, 2]]
    return np.packbits(bits.astype(np.uint8), bitorder="little")


def detect(img, n_features=1500, scale_factor=1.3, n_levels=5, fast_threshold=20, edge=31):
    """One frame ([H, W] grey or [H, W, 3] B G R) -> dict(kp, kp_xy, desc, levels, unique, n_candidates)"""
    g0 = grey(img) if img.ndim == 3 else img
    H, W = g0.shape
    levels = pyramid(g0, scale_factor, n_levels)
    _, quota = level_sizes(H, W, n_features, scale_factor, n_levels)
    recs, descs, uniq, ncand = [], [], [], []
    for l, im in enumerate(levels):
        Hl, Wl = im.shape
        ys, xs = candidates(fast_scores(im, fast_threshold), edge)
        ncand.append(len(ys))
        if not len(ys):
            continue
        R = harris(im, ys, xs)
        box = box_sums(im)
        for i in select(R, ys, xs, quota[l]):
            y, x = int(ys[i]), int(xs[i])
            b, u = orientation(im, y, x)
            r = np.zeros((), KEYPOINT)
            r["x"] = np.float32((np.float64(x) + 0.5) * np.float64(W) / np.float64(Wl) - 0.5)
            r["y"] = np.float32((np.float64(y) + 0.5) * np.float64(H) / np.float64(Hl) - 0.5)
            r["angle_deg"] = np.float32(b * 5.625)
            r["size"] = np.float32(np.float64(31.0) * np.float64(W) / np.float64(Wl))
            r["response"], r["xl"], r["yl"], r["level"], r["angle_bin"] = R[i], x, y, l, b
            recs.append(r)
            descs.append(describe(box, y, x, b))
            uniq.append(u)
    kp = np.array(recs, KEYPOINT) if recs else np.zeros(0, KEYPOINT)
    return dict(kp=kp, kp_xy=np.stack([kp["x"], kp["y"]], 1).astype(np.float32).reshape(-1, 2),
                desc=np.array(descs, np.uint8).reshape(-1, 32), levels=levels, unique=np.array(uniq, bool), n_candidates=ncand)
