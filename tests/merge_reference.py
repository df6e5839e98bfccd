"""An independent restatement of the voxel grid and the merge in torch.

TEST INFRASTRUCTURE ONLY.  The C oracle (oracle/o3dr_oracle.c, orc_voxel_grid / orc_downsample_pt_cloud) is single-pass
CPU code and takes minutes past ~100 M points; this module computes the same output, bit for bit, with torch's own sort and
elementwise ops and none of libo3dr's kernels, so it can run on the GPU next to a full-size cloud_big
(Context.cloudBigView()).  tests/test_merge_reference.py holds it equal to the oracle on CPU tensors.

The arithmetic, step by step (PCL 1.8 VoxelGrid::applyFilter as the oracle restates it):
  * box: fp32 min / max; inv = float32(1.0f / leaf); dx = int64(fp32(max - min) * inv) + 1 per axis; dx*dy*dz > INT32_MAX
    (int64 product) is PCL's overflow guard: output = input, status VOXEL_OVERFLOW;
  * key: min_b = floor(fp32(min * inv)), i = floor(fp32(p * inv)) - min_b, idx = i0 + i1*div_x + i2*div_x*div_y in int64,
    then & 0xFFFFFFFF (PCL's uint32 wrap);
  * order: ONE sort of (idx << 31) | input_index (int64), which is the stable order by idx while N < 2^31; runs shorter than
    min_points are dropped;
  * sums: per cell an fp32 running sum from 0.0f in ascending input index - a loop over the position in the run, with the
    cells sorted by descending count so that the cells still active are a prefix (no cumsum, atomics or index_add_, whose
    order is not the oracle's).  The same loop keeps fp64 sums (error-free-transformation checked: `exact_sum` says where
    they are exact) and exact int64 colour sums;
  * division: on the host in numpy float32 (IEEE), `sum / float32(n)`, `uint32(float32(channel_sum) / float32(n))`.  The
    colour formula equals the oracle's fp32 running sum only while n * 255 < 2^24: a cell beyond that raises;
  * combined mode (downsample_pt_cloud(..., combined=True), A5): z' = fp32(z + 500) before, leaf (vs, vs, 1000), and
    fp32(z - 500) after, also under the overflow fallback.

Beyond the oracle it returns the exactly rounded means fl32(sum x / n), fl32(sum y / n) and fl32(fl32(sum z' / n) - 500) from
the fp64 sums, and `error_bound` gives every cell's order-independent bound, which ANY fp32 summation order meets.

Peak extra device memory is about 48 bytes per input point (int64 keys, torch.sort's values + indices + scratch, then the
sorted [N, 4] rows): 44.0 GiB measured on an MI355X at the 982 M points of configs[2]'s 2000-frame merge, next to its 15.7 GB
cloud_big - well inside one MI355X's 288 GB, so no slabs.  tests/test_gpu_parity.py prints the peak it measures at full size.  Every gather
goes through `_take` in chunks (see there for why).
"""
from dataclasses import dataclass
from fractions import Fraction

import numpy as np
import torch

POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])
STATUS_VOXEL_OVERFLOW = 1
INT32_MAX = (1 << 31) - 1
_M32 = 0xFFFFFFFF
_U = 2.0 ** -24  # unit roundoff of fp32
_CHUNK = 1 << 22


@dataclass
class Merge:
    points: np.ndarray              # POINT [M], bit-exact to the canonical (stable) order
    status: int                     # 0 or STATUS_VOXEL_OVERFLOW
    counts: np.ndarray = None       # int64 [M] points per output cell (None under the overflow fallback)
    idx: np.ndarray = None          # int64 [M] PCL linear cell index (uint32 value), strictly ascending
    exact: np.ndarray = None        # float32 [M, 3] exactly rounded means of x, y, z (z after the -500 in combined mode)
    abs_sum: np.ndarray = None      # float64 [M, 3] sum |v| per cell (v = z' for z in combined mode)
    exact_sum: np.ndarray = None    # bool [M, 3] the fp64 sum of the cell is the exact sum
    z_offset: float = 0.0           # 500 in combined mode


def _as_rows(points, device=None):
    """[N, 4] int32 tensor (the layout of Context.cloudBigView()) from such a tensor or a numpy POINT array"""
    if isinstance(points, torch.Tensor):
        t = points
        assert t.dtype == torch.int32 and t.dim() == 2 and t.shape[1] == 4, (t.dtype, t.shape)
    else:
        a = np.ascontiguousarray(points, POINT)
        t = torch.from_numpy(a.view(np.int32).reshape(-1, 4))
    return t if device is None else t.to(device)


def _take(src, index):
    """src[index] along dim 0, at most 2^22 output rows per gather: torch's gather (ROCm 7.0 build of torch 2.10) has been
    seen to return wrong rows for the LAST 2^26 rows of a 98 M-row [N, 4] int32 gather, while chunked gathers are exact"""
    out = torch.empty((index.numel(),) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    for a in range(0, index.numel(), _CHUNK):
        torch.index_select(src, 0, index[a:a + _CHUNK], out=out[a:a + _CHUNK])
    return out


def _rows_to_points(t):
    return t.detach().cpu().numpy().view(POINT).reshape(-1).copy()


def _int64_wrap(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def _round_f32(s, n):
    """fl32(s / n) for fp64 sums s and counts n.  The fp64 quotient is rounded once more to fp32; that double rounding can only
    differ from a single rounding where the fp64 quotient lands exactly on an fp32 midpoint, and those cells are settled with
    exact rationals."""
    q = s / n
    r = q.astype(np.float32)
    r64 = r.astype(np.float64)
    toward = np.where(q > r64, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    other = np.nextafter(r, toward)
    mid = (r64 + other.astype(np.float64)) / 2  # exact: 25 significant bits
    for i in np.nonzero((q != r64) & (q == mid))[0]:
        true, m = Fraction(float(s[i])) / int(n[i]), Fraction(float(mid[i]))
        if true > m:
            r[i] = max(r[i], other[i])
        elif true < m:
            r[i] = min(r[i], other[i])
    return r


def _merge(rows, leaf, min_points, z_offset):
    """rows: [N, 4] int32 tensor (any device); leaf: 3 float32; z_offset 0 or 500 (combined mode)"""
    dev = rows.device
    n = rows.shape[0]
    f = rows.view(torch.float32)
    off = np.float32(z_offset)
    if n == 0:
        return Merge(np.zeros(0, POINT), 0, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), np.float32),
                     np.zeros((0, 3)), np.zeros((0, 3), bool), float(z_offset))
    cols = [f[:, 0], f[:, 1], f[:, 2] + torch.tensor(off, device=dev) if z_offset else f[:, 2]]  # z' = fp32(z + 500)

    # --- box, overflow guard, geometry (host scalars in float32: IEEE like the oracle's)
    leaf = np.asarray(leaf, np.float32).reshape(3)
    inv = np.float32(1.0) / leaf
    mn = np.array([c.min().item() for c in cols], np.float32)
    mx = np.array([c.max().item() for c in cols], np.float32)
    d = [int(np.float32(mx[a] - mn[a]) * inv[a]) + 1 for a in range(3)]
    if _int64_wrap(d[0] * d[1] * d[2]) > INT32_MAX:
        out = rows.clone()
        if z_offset:
            out.view(torch.float32)[:, 2] = cols[2] - torch.tensor(off, device=dev)
        return Merge(_rows_to_points(out), STATUS_VOXEL_OVERFLOW, z_offset=float(z_offset))
    min_b = [int(np.floor(np.float32(mn[a] * inv[a]))) for a in range(3)]
    max_b = [int(np.floor(np.float32(mx[a] * inv[a]))) for a in range(3)]
    div_b = [max_b[a] - min_b[a] + 1 for a in range(3)]
    mul = [1, div_b[0] & _M32, (div_b[0] * div_b[1]) & _M32]

    # --- keys: fp32 product, floor, int64 arithmetic, uint32 wrap
    inv_t = torch.from_numpy(inv).to(dev)
    key = torch.zeros(n, dtype=torch.int64, device=dev)
    for a in range(3):
        i = torch.floor(cols[a] * inv_t[a]).to(torch.int64) - min_b[a]
        key += (i & _M32) * mul[a]
        del i
    key &= _M32
    del cols

    # --- canonical order: one sort of (idx << 31) | input index == the stable order by idx (N < 2^31)
    assert n < (1 << 31)
    key <<= 31
    key |= torch.arange(n, dtype=torch.int64, device=dev)
    key = torch.sort(key).values
    cell = key >> 31
    key &= (1 << 31) - 1
    srt = _take(rows, key)  # [N, 4] rows in canonical order
    del key
    head = torch.ones(n, dtype=torch.bool, device=dev)
    head[1:] = cell[1:] != cell[:-1]
    starts = torch.nonzero(head).flatten()
    del head
    counts = torch.diff(starts, append=torch.tensor([n], device=dev))
    cell = _take(cell, starts)
    keep = counts >= min_points
    keep = torch.nonzero(keep).flatten()
    starts, counts, cell = _take(starts, keep), _take(counts, keep), _take(cell, keep)
    m = starts.numel()
    if m == 0:
        return Merge(np.zeros(0, POINT), 0, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), np.float32),
                     np.zeros((0, 3)), np.zeros((0, 3), bool), float(z_offset))
    cnt = counts.cpu().numpy()
    if (cnt * 255 >= (1 << 24)).any():
        raise ValueError(f"a cell of {cnt.max()} points: fp32 colour sums of that many points are order-dependent")

    # --- sums: position-in-run loop over cells in descending count (active cells = a prefix)
    by_count = torch.sort(counts, descending=True, stable=True).indices
    starts_d = _take(starts, by_count)
    cnt_d = cnt[by_count.cpu().numpy()]
    active = np.searchsorted(-cnt_d, -np.arange(int(cnt_d[0])), side="left")  # cells with count > j
    s32 = torch.zeros((m, 3), dtype=torch.float32, device=dev)
    s64 = torch.zeros((m, 3), dtype=torch.float64, device=dev)
    a64 = torch.zeros((m, 3), dtype=torch.float64, device=dev)
    inexact = torch.zeros((m, 3), dtype=torch.bool, device=dev)
    csum = torch.zeros((m, 4), dtype=torch.int64, device=dev)
    shifts = torch.tensor([16, 8, 0, 24], dtype=torch.int32, device=dev)  # r, g, b, a
    zo = torch.tensor([0.0, 0.0, off], dtype=torch.float32, device=dev)
    for j, k in enumerate(active.tolist()):
        r = _take(srt, starts_d[:k] + j)
        v = r.view(torch.float32)[:, :3]
        if z_offset:
            v = v + zo  # z' = fp32(z + 500); + 0.0f leaves x and y unchanged
        s32[:k] += v
        v = v.double()
        s, t = s64[:k], s64[:k] + v  # TwoSum: e is the exact rounding error of the fp64 add
        bp = t - s
        e = (s - (t - bp)) + (v - bp)
        inexact[:k] |= e != 0
        s64[:k] = t
        a64[:k] += v.abs()
        csum[:k] += ((r[:, 3:4] >> shifts) & 255).to(torch.int64)
    del srt

    # --- back to ascending idx, divisions on the host
    undo = torch.sort(by_count).indices  # inverse permutation
    s32, s64, a64, inexact, csum = (_take(t, undo).cpu().numpy() for t in (s32, s64, a64, inexact, csum))
    nf = cnt.astype(np.float32)
    out = np.empty(m, POINT)
    for a, ax in enumerate("xyz"):
        out[ax] = s32[:, a] / nf
    out["z"] -= off
    ch = (csum.astype(np.float32) / nf[:, None]).astype(np.uint32)
    out["rgba"] = (ch[:, 3] << 24) | (ch[:, 0] << 16) | (ch[:, 1] << 8) | ch[:, 2]
    exact = np.stack([_round_f32(s64[:, a], cnt) for a in range(3)], axis=1)
    exact[:, 2] -= off
    return Merge(out, 0, cnt, cell.cpu().numpy(), exact, a64, ~inexact, float(z_offset))


def voxel_grid(points, leaf, min_points=0, device=None):
    """orc.voxel_grid(points, leaf, min_points, ORDER_STABLE) restated; points: [N, 4] int32 tensor or numpy POINT"""
    return _merge(_as_rows(points, device), leaf, int(min_points), 0)


def downsample_pt_cloud(points, voxel_size, combined, min_points_per_voxel=1, device=None):
    """orc.downsample_pt_cloud(points, voxel_size, combined, min_points_per_voxel, ORDER_STABLE) restated: the merge when
    combined (pose_functions.cpp:1660-1704: z + 500, leaf (vs, vs, 1000), min_points_per_voxel, z - 500), else the per-frame
    grid (leaf vs / 5, PCL's default min_points 0).  voxel_size is a double narrowed to float, like the reference's."""
    rows = _as_rows(points, device)
    if combined:
        vs = np.float32(voxel_size)
        return _merge(rows, (vs, vs, np.float32(1000)), int(min_points_per_voxel), 500)
    leaf = np.float32(float(voxel_size) / 5)
    return _merge(rows, (leaf, leaf, leaf), 0, 0)


def error_bound(ref):
    """[M, 3] float64: how far ANY fp32 summation order's result may lie from ref.exact, per cell and axis.
    Recursive summation of n terms in any order errs by at most gamma_(n-1) * sum|v|, gamma_k = k u / (1 - k u), u = 2^-24
    (Higham, Accuracy and Stability of Numerical Algorithms, (4.4)); dividing by n scales that, and the division, the exact
    mean's own rounding and (combined mode) the two -500 roundings add at most one ulp each at the magnitudes involved.  Where
    the fp64 sum was not exact (exact_sum False) one more ulp is allowed."""
    n = ref.counts.astype(np.float64)[:, None]
    k = n - 1
    e = k * _U / (1 - k * _U) * ref.abs_sum / n
    mean = np.abs(ref.exact.astype(np.float64))
    mean[:, 2] = np.abs(ref.exact[:, 2].astype(np.float64) + ref.z_offset)  # the fp32 mean of z' before the -500
    ulp = np.spacing(np.float32(mean + e)).astype(np.float64)
    bound = e + ulp * np.where(ref.exact_sum, 1.0, 2.0)
    if ref.z_offset:
        bound[:, 2] += np.spacing(np.float32(np.abs(ref.exact[:, 2].astype(np.float64)) + bound[:, 2])).astype(np.float64)
    return bound
