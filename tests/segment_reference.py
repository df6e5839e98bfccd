"""numpy restatement of include/o3dr.h "image segmentation" (o3dr_segment_image), operation for operation, and the test
images of the segmentation tests.  Everything is an integer; int64 holds every intermediate value."""
import numpy as np

import disparity_filter_reference


def _bgr(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    if img.ndim == 2:
        img = np.repeat(img[:, :, None], 3, axis=2)  # a grey pixel counts as B = G = R
    assert img.shape[2] == 3
    return img.astype(np.int64)


def default_min_size(step):
    return step * step // 4


def seeds(img3, S):
    """-> centres int64 [ny * nx, 5]: x, y, B, G, R"""
    H, W = img3.shape[:2]
    nx, ny = -(-W // S), -(-H // S)
    gy, gx = np.divmod(np.arange(nx * ny), nx)
    x = np.minimum(gx * S + S // 2, W - 1)
    y = np.minimum(gy * S + S // 2, H - 1)
    return np.concatenate([x[:, None], y[:, None], img3[y, x]], axis=1)


def assign(img3, centres, S, m, highest_k_wins=False):
    """Step 2.  highest_k_wins: the negative control of the tie-break (not the contract)."""
    H, W = img3.shape[:2]
    nx, ny = -(-W // S), -(-H // S)
    yy, xx = np.mgrid[0:H, 0:W]
    hx, hy = xx // S, yy // S
    best_d = np.full((H, W), -1, np.int64)
    best_k = np.full((H, W), -1, np.int64)
    for dy in (-1, 0, 1):          # ascending k: a strict < keeps the lowest k of a tie
        for dx in (-1, 0, 1):
            cx, cy = hx + dx, hy + dy
            ok = (cx >= 0) & (cx < nx) & (cy >= 0) & (cy < ny)
            k = np.where(ok, cy * nx + cx, 0)
            c = centres[k]
            dc = ((img3 - c[:, :, 2:5]) ** 2).sum(axis=2)
            ds = (xx - c[:, :, 0]) ** 2 + (yy - c[:, :, 1]) ** 2
            D = S * S * dc + m * m * ds
            better = ok & ((best_k < 0) | ((D <= best_d) if highest_k_wins else (D < best_d)))
            best_d = np.where(better, D, best_d)
            best_k = np.where(better, k, best_k)
    return best_k


def update(img3, centres, lab):
    """Step 3: exact integer sums, (2 sum + n) / (2 n) floored; an empty centre keeps its values."""
    H, W = img3.shape[:2]
    nc = len(centres)
    yy, xx = np.mgrid[0:H, 0:W]
    flat = lab.reshape(-1)
    n = np.bincount(flat, minlength=nc).astype(np.int64)
    out = centres.copy()
    vals = [xx.reshape(-1), yy.reshape(-1), img3[:, :, 0].reshape(-1), img3[:, :, 1].reshape(-1), img3[:, :, 2].reshape(-1)]
    for j, v in enumerate(vals):
        s = np.zeros(nc, np.int64)
        np.add.at(s, flat, v)
        out[:, j] = np.where(n > 0, (2 * s + n) // np.maximum(2 * n, 1), centres[:, j])
    return out


def raw_labels(img, S, m, K, highest_k_wins=False):
    """Steps 1 to 4 -> (L0 int64 [H, W], centres after the K updates)"""
    img3 = _bgr(img)
    c = seeds(img3, S)
    for _ in range(K):
        c = update(img3, c, assign(img3, c, S, m, highest_k_wins))
    return assign(img3, c, S, m, highest_k_wins), c


def components(lab):
    """Step 5 -> root int64 [H, W]: the lowest pixel index of the pixel's 4-connected equal-label component."""
    H, W = lab.shape
    n = H * W
    idx = np.arange(n).reshape(H, W)
    eh = lab[:, 1:] == lab[:, :-1]
    ev = lab[1:, :] == lab[:-1, :]
    a = np.concatenate([idx[:, :-1][eh], idx[:-1, :][ev]])
    b = np.concatenate([idx[:, 1:][eh], idx[1:, :][ev]])
    p = np.arange(n)
    while True:  # hook the larger root under the smaller, then jump: ends when every edge lies within one tree
        ra, rb = p[a], p[b]
        lo = np.minimum(ra, rb)
        q = p.copy()
        np.minimum.at(q, ra, lo)
        np.minimum.at(q, rb, lo)
        while True:
            q2 = q[q]
            if np.array_equal(q2, q):
                break
            q = q2
        if np.array_equal(q, p):
            break
        p = q
    return p.reshape(H, W)


NO_KEY = (1 << 63) - 1


def merge(root, lab, centres, min_size):
    """Steps 6 and 7 -> (labels, sizes, n_components, n_merged, n_labels)"""
    H, W = root.shape
    n = H * W
    r = root.reshape(-1)
    cnt = np.bincount(r, minlength=n).astype(np.int64)  # at the roots
    is_root = r == np.arange(n)
    small = cnt[r] < min_size                            # per pixel
    col = centres[lab.reshape(-1)][:, 2:5]               # per pixel: its component's centre colour
    key = np.full(n, NO_KEY, np.int64)
    idx = np.arange(n).reshape(H, W)
    pairs = [(idx[:, :-1].reshape(-1), idx[:, 1:].reshape(-1)), (idx[:-1, :].reshape(-1), idx[1:, :].reshape(-1))]
    for p, q in pairs:
        for s, t in ((p, q), (q, p)):  # s in a small component, t in a not-small one
            sel = small[s] & ~small[t]
            s2, t2 = s[sel], t[sel]
            d = ((col[s2] - col[t2]) ** 2).sum(axis=1)
            np.minimum.at(key, r[s2], (d << 32) | r[t2])
    link = np.arange(n)
    roots = np.nonzero(is_root)[0]
    for c in roots:
        if not small[c]:
            continue
        if key[c] != NO_KEY:
            link[c] = key[c] & 0xFFFFFFFF
        elif c % W > 0:
            link[c] = r[c - 1]
        elif c >= W:
            link[c] = r[c - W]
    fin = np.arange(n)
    for c in roots:  # ascending: a link goes to a lower first pixel (already resolved) or to a not-small root (itself for good)
        fin[c] = fin[link[c]]
    survivor = is_root & (fin == np.arange(n))
    first = np.full(n, n, np.int64)          # at the surviving roots: the lowest first pixel of what ended up in them
    np.minimum.at(first, fin[roots], roots)
    flag = np.zeros(n, np.int64)
    flag[first[survivor]] = 1
    number = np.cumsum(flag) - flag          # exclusive scan in pixel order
    final_root = fin[r]
    labels = number[first[final_root]]
    size_at = np.bincount(final_root, minlength=n)
    sizes = size_at[final_root]
    n_comp = int(is_root.sum())
    n_labels = int(survivor.sum())
    return labels.reshape(H, W), sizes.reshape(H, W), n_comp, n_comp - n_labels, n_labels


def segment(img, step=16, compactness=20, iterations=5, min_size=None, highest_k_wins=False):
    """-> dict(labels uint32, raw int32, sizes int32, info dict) of one image"""
    S, m, K = int(step), int(compactness), int(iterations)
    if min_size is None or min_size < 0:
        min_size = default_min_size(S)
    raw, c = raw_labels(img, S, m, K, highest_k_wins)
    root = components(raw)
    labels, sizes, n_comp, n_merged, n_labels = merge(root, raw, c, int(min_size))
    info = dict(n_centres=len(c), n_components=n_comp, n_merged=n_merged, n_labels=n_labels, largest=int(sizes.max()),
                smallest=int(sizes.min()))
    return dict(labels=labels.astype(np.uint32), raw=raw.astype(np.int32), sizes=sizes.astype(np.int32), info=info)


# ---- test images -----------------------------------------------------------------------------------------------------
REGION_COLOURS = np.array([(40, 90, 60), (200, 60, 80), (90, 180, 220), (150, 150, 30)], np.int64)
REGION_PLANES = [(100.0, 0.05, 0.10), (130.0, -0.10, 0.02), (160.0, 0.08, -0.06), (115.0, 0.0, 0.15)]  # d = a + b x + c y


def region_image(H=64, W=96, seed=7):
    """-> (img uint8 [H, W, 3], region int [H, W], disp uint8 [H, W], true_disp float64 [H, W])"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    region = np.zeros((H, W), np.int64)
    region[(yy >= 10) & (yy <= 39) & (xx >= 20) & (xx <= 59)] = 1
    region[(yy > 30) & (xx + yy > 110)] = 2
    region[(xx - 20) ** 2 + (yy - 50) ** 2 <= 81] = 3
    img = REGION_COLOURS[region] + rs.randint(-6, 7, (H, W, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    true = np.zeros((H, W))
    for i, (a, b, c) in enumerate(REGION_PLANES):
        true = np.where(region == i, a + b * xx + c * yy, true)
    disp = np.clip(np.rint(true + rs.randint(-2, 3, (H, W))), 0, 255).astype(np.uint8)
    return img, region, disp, true


def random_image(H, W, channels, seed):
    """blocks of a few colours under noise: superpixels with real borders, ties and small components"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    cell = ((yy // 11) * 7 + (xx // 13) * 3) % 5
    base = rs.randint(0, 256, (5, 3))[cell]
    img = np.clip(base + rs.randint(-8, 9, (H, W, 3)), 0, 255).astype(np.uint8)
    return img if channels == 3 else np.ascontiguousarray(img[:, :, 1])


def constant_image(H, W):
    return np.full((H, W), 77, np.uint8)


def checkerboard(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((xx + yy) & 1) * 255).astype(np.uint8)


def serpentine(H, W):
    """two colours; the bright one is a one-pixel path that winds down the whole image, row pairs joined at alternating ends"""
    img = np.zeros((H, W), np.uint8)
    img[0::2, :] = 255
    for i, y in enumerate(range(1, H, 2)):
        img[y, W - 1 if i % 2 == 0 else 0] = 255
    return img


def comb(H, W):
    """two colours; a bright spine along the top row with a one-pixel tooth down every second column"""
    img = np.zeros((H, W), np.uint8)
    img[0, :] = 255
    img[:H - 1, 0::2] = 255
    return img


def maze(H, W, seed):
    """two colours; the bright one is disparity_filter_reference.maze: a random spanning tree, one component"""
    return ((disparity_filter_reference.maze(H, W, seed) != 0) * 255).astype(np.uint8)


def spiral(H, W):
    """two colours; the bright one is disparity_filter_reference.spiral: one arm that winds inwards, one component"""
    return ((disparity_filter_reference.spiral(H, W) != 0) * 255).astype(np.uint8)


def plane_fit_rms(labels, disp, true):
    """RMS of (least-squares plane per label over disp) against true"""
    H, W = labels.shape
    yy, xx = np.mgrid[0:H, 0:W]
    fit = np.zeros((H, W))
    for l in np.unique(labels):
        sel = labels == l
        A = np.stack([np.ones(sel.sum()), xx[sel], yy[sel]], axis=1).astype(np.float64)
        coef = np.linalg.lstsq(A, disp[sel].astype(np.float64), rcond=None)[0]
        fit[sel] = A @ coef
    return float(np.sqrt(np.mean((fit - true) ** 2)))
