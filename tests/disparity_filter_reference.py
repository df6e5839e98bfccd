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


def maze(H, W, seed, dtype=np.uint8, value=6):
    """a random spanning tree of the cells at even (y, x): every cell and every opened wall pixel carries `value`, the rest
    is 0.  One component of 2 * cells - 1 pixels whose path turns at random, so its tile-border crossings are spread over
    every border and its union-find trees have no regular shape.  The tree is an iterative depth-first walk that takes a
    random unvisited neighbour."""
    rs = np.random.RandomState(seed)
    ch, cw = (H + 1) // 2, (W + 1) // 2
    draws = rs.randint(0, 12, ch * cw).tolist()  # one per step forward; 12 is a multiple of every number of choices
    img = np.zeros((H, W), dtype)
    seen = bytearray(ch * cw)
    seen[0] = 1
    img[0, 0] = value
    stack = [0]
    k = 0
    while stack:
        c = stack[-1]
        y, x = divmod(c, cw)
        free = [(dy, dx) for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0))
                if 0 <= y + dy < ch and 0 <= x + dx < cw and not seen[c + dy * cw + dx]]
        if not free:
            stack.pop()
            continue
        dy, dx = free[draws[k] % len(free)]
        k += 1
        img[2 * y + dy, 2 * x + dx] = value            # the wall between the two cells
        img[2 * (y + dy), 2 * (x + dx)] = value
        seen[c + dy * cw + dx] = 1
        stack.append(c + dy * cw + dx)
    return img


def spiral(H, W, dtype=np.uint8, value=4):
    """one arm, one pixel wide, with one pixel of 0 between turns: from (0, 0) clockwise inwards until it can go no further.
    One component that crosses every tile border once per turn; consecutive pixels of the path lie up to a whole image
    side apart in index order."""
    rows = [bytearray(W) for _ in range(H)]
    rows[0][0] = 1
    y = x = d = 0
    steps = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def free(y, x, dy, dx):
        """the next pixel is inside and touches no pixel of the arm but the one it comes from"""
        y1, x1 = y + dy, x + dx
        if not (0 <= y1 < H and 0 <= x1 < W) or rows[y1][x1]:
            return False
        return not any(0 <= y2 < H and 0 <= x2 < W and rows[y2][x2] for y2, x2 in ((y1 - 1, x1), (y1 + 1, x1), (y1, x1 - 1), (y1, x1 + 1))
                       if (y2, x2) != (y, x))

    while True:
        dy, dx = steps[d]
        if not free(y, x, dy, dx):
            d = (d + 1) % 4
            dy, dx = steps[d]
            if not free(y, x, dy, dx):
                break
        y, x = y + dy, x + dx
        rows[y][x] = 1
    return (np.frombuffer(b"".join(rows), np.uint8).reshape(H, W) * value).astype(dtype)


def border_pairs(img):
    """-> (valid-valid pixel pairs across each vertical tile border: x a multiple of 64, across each horizontal one: y a
    multiple of 16), the tile being the kernels' 64 x 16"""
    v = np.asarray(img) != 0
    return (v[:, 63:-1:64] & v[:, 64::64]).sum(axis=0), (v[15:-1:16] & v[16::16]).sum(axis=1)


def ramp():
    """3 x 100 uint16, steps of 3 along x"""
    return np.tile((1000 + 3 * np.arange(100)).astype(np.uint16), (3, 1))
