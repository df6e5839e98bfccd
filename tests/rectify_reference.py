"""numpy restatement of the stereo-rectification contract (include/o3dr.h "stereo rectification"), operation for operation:
rectify_maps is o3dr_rectify_maps (fp64, every + - * / in the contract's order; numpy's elementwise ufuncs round each
operation once and fuse nothing), rectify_remap is o3dr_rectify_remap (integers).  Also the calibrations the tests share."""
import numpy as np

OUTSIDE = -1048576  # O3DR_RECTIFY_OUTSIDE


def pad_D(D):
    D = np.asarray(D, np.float64).reshape(-1)
    assert D.size in (4, 5, 8)
    return np.concatenate([D, np.zeros(8 - D.size)])


def inverse_PR(R, P):
    """steps 1-4 of the contract: I = inverse of (left 3x3 of P) R, by cofactors, as python floats (IEEE doubles)"""
    R = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
    P = np.asarray(P, np.float64)
    if P.shape == (3, 3):
        P = np.hstack([P, np.zeros((3, 1))])
    P = [float(v) for v in P.reshape(12)]
    A = [[(P[4 * i] * R[j] + P[4 * i + 1] * R[3 + j]) + P[4 * i + 2] * R[6 + j] for j in range(3)] for i in range(3)]
    c = [[0.0] * 3 for _ in range(3)]
    c[0][0] = A[1][1] * A[2][2] - A[1][2] * A[2][1]
    c[0][1] = A[1][2] * A[2][0] - A[1][0] * A[2][2]
    c[0][2] = A[1][0] * A[2][1] - A[1][1] * A[2][0]
    c[1][0] = A[0][2] * A[2][1] - A[0][1] * A[2][2]
    c[1][1] = A[0][0] * A[2][2] - A[0][2] * A[2][0]
    c[1][2] = A[0][1] * A[2][0] - A[0][0] * A[2][1]
    c[2][0] = A[0][1] * A[1][2] - A[0][2] * A[1][1]
    c[2][1] = A[0][2] * A[1][0] - A[0][0] * A[1][2]
    c[2][2] = A[0][0] * A[1][1] - A[0][1] * A[1][0]
    det = (A[0][0] * c[0][0] + A[0][1] * c[0][1]) + A[0][2] * c[0][2]
    if det == 0.0 or not np.isfinite(det):
        raise ValueError("P R is singular")
    return [[c[j][i] / det for j in range(3)] for i in range(3)]


def source_positions(K, D, R, P, size):
    """the kernel's steps up to (mx, my): the unquantised source position of every destination pixel, float64 [H, W] each"""
    K = np.asarray(K, np.float64).reshape(3, 3)
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in pad_D(D))
    fx, cx, fy, cy = float(K[0, 0]), float(K[0, 2]), float(K[1, 1]), float(K[1, 2])
    I = inverse_PR(R, P)
    rows, cols = size
    v, u = np.meshgrid(np.arange(rows, dtype=np.float64), np.arange(cols, dtype=np.float64), indexing="ij")
    with np.errstate(all="ignore"):
        X = (I[0][0] * u + I[0][1] * v) + I[0][2]
        Y = (I[1][0] * u + I[1][1] * v) + I[1][2]
        Wc = (I[2][0] * u + I[2][1] * v) + I[2][2]
        iw = 1.0 / Wc
        x = X * iw
        y = Y * iw
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        xy2 = 2.0 * (x * y)
        num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2
        den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2
        kr = num / den
        xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2)
        yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2
        mx = fx * xd + cx
        my = fy * yd + cy
    return mx, my


def rectify_maps(K, D, R, P, size):
    """o3dr_rectify_maps -> int32 [rows_out, cols_out, 2] = (qx, qy)"""
    mx, my = source_positions(K, D, R, P, size)
    with np.errstate(all="ignore"):
        qx = np.floor(mx * 32.0 + 0.5)
        qy = np.floor(my * 32.0 + 0.5)
        ok = (qx >= -1048576.0) & (qx < 1048576.0) & (qy >= -1048576.0) & (qy < 1048576.0)  # (a NaN fails)
    out = np.full(qx.shape + (2,), OUTSIDE, np.int32)
    out[..., 0][ok] = qx[ok].astype(np.int32)
    out[..., 1][ok] = qy[ok].astype(np.int32)
    return out


def rectify_remap(src, maps, border=0):
    """o3dr_rectify_remap of one image [H, W] or [H, W, 3] (uint8) -> (out uint8 [H_out, W_out(, 3)], valid uint8 [H_out, W_out])"""
    src = np.asarray(src)
    assert src.dtype == np.uint8
    grey = src.ndim == 2
    img = (src[..., None] if grey else src).astype(np.int64)
    rows, cols = img.shape[:2]
    qx, qy = maps[..., 0].astype(np.int64), maps[..., 1].astype(np.int64)
    x0, y0, ax, ay = qx >> 5, qy >> 5, qx & 31, qy & 31
    total = np.zeros(qx.shape + (img.shape[2],), np.int64)
    valid = np.ones(qx.shape, bool)
    for dx, dy, w in ((0, 0, (32 - ax) * (32 - ay)), (1, 0, ax * (32 - ay)), (0, 1, (32 - ax) * ay), (1, 1, ax * ay)):
        x, y = x0 + dx, y0 + dy
        inside = (x >= 0) & (x < cols) & (y >= 0) & (y < rows)
        t = np.where(inside[..., None], img[np.clip(y, 0, rows - 1), np.clip(x, 0, cols - 1)], int(border))
        total += w[..., None] * t
        valid &= inside | (w == 0)
    out = ((total + 512) >> 10).astype(np.uint8)
    return (out[..., 0] if grey else out), valid.astype(np.uint8)


def rectify_remap_frames(src, maps, border=0):
    """a stack [F, H, W(, 3)] frame by frame -> (out [F, ...], valid)"""
    outs = [rectify_remap(f, maps, border) for f in src]
    return np.stack([o for o, _ in outs]), outs[0][1]


def rodrigues(r):
    """the rotation matrix of an axis-angle vector"""
    r = np.asarray(r, np.float64)
    th = float(np.linalg.norm(r))
    if th == 0.0:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


# ---- the calibrations of the issue's cases: (K, D, R, P, source size, destination size) --------------------------------
K_ID = np.array([[48.0, 0, 26], [0, 48, 18], [0, 0, 1]])
IDENTITY = dict(K=K_ID, D=np.zeros(8), R=np.eye(3), P=np.hstack([K_ID, np.zeros((3, 1))]), src=(37, 53), size=(37, 53))
D_GENERAL = np.array([-0.28, 0.09, 0.0012, -0.0007, -0.011, 0.02, -0.01, 0.003])
P_GENERAL = np.array([[44.0, 0, 24.5, -5.3], [0, 44, 20.25, 0], [0, 0, 1, 0]])
GENERAL = dict(K=np.array([[48.0, 0, 26.3], [0, 47.5, 18.1], [0, 0, 1]]), D=D_GENERAL, R=rodrigues((0.02, -0.03, 0.015)), P=P_GENERAL,
               src=(37, 53), size=(41, 50))
P_SENTINEL = np.array([[44.0, 0, 24, 0], [0, 44, 20, 0], [0, 0, 1, 0]])
SENTINEL = dict(K=K_ID, D=np.zeros(8), R=rodrigues((0.0, np.pi / 2, 0.0)), P=P_SENTINEL, src=(37, 53), size=(41, 50))
POLE = dict(K=K_ID, D=np.array([0, 0, 0, 0, 0, -4.0, 0, 0]), R=np.eye(3), P=P_SENTINEL, src=(37, 53), size=(41, 50))


def maps_of(case, size=None):
    return rectify_maps(case["K"], case["D"], case["R"], case["P"], size or case["size"])


def test_image(rows, cols, channels=1, seed=0):
    """a smooth gradient plus noise: interpolation errors show, and so does any misplaced tap"""
    rng = np.random.RandomState(seed)
    shape = (rows, cols) if channels == 1 else (rows, cols, 3)
    y, x = np.mgrid[0:rows, 0:cols]
    base = (3 * x + 5 * y) % 200
    img = (base if channels == 1 else base[..., None] + np.array([0, 20, 40])) + rng.randint(0, 56, shape)
    return np.clip(img, 0, 255).astype(np.uint8)


test_image.__test__ = False  # (a helper, not a test)
