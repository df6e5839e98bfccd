"""The disparity-filter contract (include/o3dr.h "disparity filter") in numpy: k x k median with clamped borders, connected
components of near-equal 4-neighbours labelled by their lowest pixel index, removal of the small ones."""
from collections import namedtuple

import numpy as np

Info = namedtuple("Info", "n_valid n_components n_speckles n_removed largest")


def median(img, k):
    """element k * k // 2 of the ascending sort of the k x k clamped window; k = 0: the image itself"""
    img = np.asarray(img)
    if k == 0:
        return img.copy()
    assert k in (3, 5) and img.ndim == 2
    H, W = img.shape
    r = k // 2
    ys = np.clip(np.arange(-r, H + r), 0, H - 1)
    xs = np.clip(np.arange(-r, W + r), 0, W - 1)
    pad = img[ys][:, xs]
    stack = np.stack([pad[dy:dy + H, dx:dx + W] for dy in range(k) for dx in range(k)])
    return np.sort(stack, axis=0)[k * k // 2]


def components(m, max_diff):
    """-> labels (int32: the lowest y * W + x of the pixel's component, -1: invalid), sizes (int32: its pixel count, 0: invalid)"""
    m = np.asarray(m)
    H, W = m.shape
    v = m.astype(np.int64).ravel()  # a type that holds every difference
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    def join(i, j):
        if v[i] != 0 and v[j] != 0 and abs(v[i] - v[j]) <= max_diff:
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)  # the smaller root wins: the root is the lowest index

    for y in range(H):
        for x in range(W):
            i = y * W + x
            if x + 1 < W:
                join(i, i + 1)
            if y + 1 < H:
                join(i, i + W)
    roots = np.array([find(i) for i in range(H * W)], np.int64)
    valid = v != 0
    count = np.bincount(roots[valid], minlength=H * W)
    labels = np.where(valid, roots, -1).astype(np.int32)
    sizes = np.where(valid, count[roots], 0).astype(np.int32)
    return labels.reshape(H, W), sizes.reshape(H, W)


def filter_disparity(img, median_size=0, max_speckle_size=0, max_diff=1):
    """one frame -> out (the input's dtype), labels, sizes, Info"""
    img = np.asarray(img)
    assert img.dtype in (np.uint8, np.uint16) and img.ndim == 2
    m = median(img, median_size)
    labels, sizes = components(m, max_diff)
    valid = m != 0
    small = valid & (sizes <= max_speckle_size) if max_speckle_size > 0 else np.zeros_like(valid)
    out = np.where(small, 0, m).astype(img.dtype)
    is_root = labels.ravel() == np.arange(labels.size)
    info = Info(int(valid.sum()), int(is_root.sum()), int((is_root & small.ravel()).sum()), int(small.sum()),
                int(sizes.max()) if sizes.size else 0)
    return out, labels, sizes, info


def filter_frames(imgs, **kw):
    """[F, H, W] -> stacked out, labels, sizes and the list of Info"""
    res = [filter_disparity(f, **kw) for f in imgs]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.stack([r[2] for r in res]), [r[3] for r in res]


# ---- the inputs the tests share ---------------------------------------------------------------------------------------
def planted_speckles():
    """48 x 96 uint8: left half 40, right half 60, a 4 x 5 hole, five blobs of 1 to 8 pixels, each more than 1 away from
    what surrounds it, one in the last corner pixel.  -> (image, the image without the blobs, the blobs' pixel counts)"""
    base = np.full((48, 96), 40, np.uint8)
    base[:, 48:] = 60
    base[20:24, 30:35] = 0
    img = base.copy()
    blobs = [(slice(5, 6), slice(7, 8), 90), (slice(47, 48), slice(95, 96), 10), (slice(10, 12), slice(60, 64), 100),
             (slice(30, 31), slice(10, 13), 20), (slice(40, 41), slice(70, 71), 200)]
    for ys, xs, val in blobs:
        img[ys, xs] = val
    clean = base.copy()
    for ys, xs, _ in blobs:
        clean[ys, xs] = 0
    return img, clean, [1, 1, 8, 3, 1]


def serpentine(H, W, dtype=np.uint8):
    """even rows full, odd rows one connector at alternating ends: one component that snakes through every row"""
    img = np.zeros((H, W), dtype)
    img[0::2] = 7
    for k, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            img[y, W - 1 if k % 2 == 0 else 0] = 7
    return img


def comb(H, W, dtype=np.uint8):
    """even columns joined by the bottom row"""
    img = np.zeros((H, W), dtype)
    img[:, 0::2] = 5
    img[H - 1] = 5
    return img


def ramp():
    """3 x 100 uint16, steps of 3 along x"""
    return np.tile((1000 + 3 * np.arange(100)).astype(np.uint16), (3, 1))
