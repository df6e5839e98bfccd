"""Python mirror of the reference's operator surface for the hot path.

`Context` methods carry the reference's member-function names (pose.h:198,199,216,231):
createSingleImgPtCloud, transformPtCloud, downsamplePtCloud, createAndTransformPtCloud — plus the
fan-out/accumulate loop (pose.cpp:365-434) and the final merge (pose.cpp:527-532).  All compute
happens in libo3dr.so; numpy arrays are staged by the library, torch CUDA tensors are passed as
HBM pointers (torch is only device memory + streams here).
"""
import ctypes as C
from collections import namedtuple
from dataclasses import dataclass, fields

import numpy as np

from . import _lib as L
from ._lib import POINT


@dataclass
class Params:
    """The `Pose` members the hot path reads (pose.h:93-126), reference defaults."""
    min_disparity: float = 64.0
    voxel_size: float = 0.1
    bounding_box: int = 20
    cutout_ratio: int = 8
    jump_pixels: int = 10
    min_points_per_voxel: int = 1
    dont_downsample: bool = False
    sor_enable: bool = True      # the reference always runs it when !combined && jump_pixels > 0 (pose_functions.cpp:1673)
    blur_kernel: int = 1
    disparity_f64: bool = False  # --use_segment_labels: disparity images are float64

    def to_struct(self):
        return L.ParamsStruct(float(self.min_disparity), float(self.voxel_size), int(self.bounding_box),
                              int(self.cutout_ratio), int(self.jump_pixels), int(self.min_points_per_voxel),
                              int(bool(self.dont_downsample)), int(bool(self.sor_enable)), int(self.blur_kernel),
                              int(bool(self.disparity_f64)))


@dataclass
class IcpResult:
    """o3dr_icp_align's result: T (float64 4x4, source -> target), the mean squared distance of the correspondences at
    fp32(T) (pcl::Registration::getFitnessScore), their number, the solves applied and why the loop stopped (ICP_REASONS)."""
    T: np.ndarray
    fitness: float
    n_correspondences: int
    iterations: int
    reason: int

    @property
    def reason_name(self):
        return L.ICP_REASONS[self.reason]


@dataclass
class MlsResult:
    """o3dr_mls_smooth's counts: points per fit kind (MLS_POLY, MLS_PLANE, MLS_NONE) and the largest neighbour count."""
    n_poly: int
    n_plane: int
    n_none: int
    max_neighbors: int


@dataclass
class MeshResult:
    """o3dr_mesh_surface's counts: vertices (occupied cells), shadowed points, kept triangles, quads with four corners and
    the candidate triangles dropped by the orientation and the edge-length rule."""
    n_vertices: int
    n_shadowed: int
    n_triangles: int
    n_quads_full: int
    n_rejected_orientation: int
    n_rejected_length: int


@dataclass
class RasterInfo:
    """o3dr_rasterize_map's record: the raster's box in cells, the points inside and outside it, the occupied cells and the
    points their cells did not choose, the filled and the empty cells, and the occupied cells' z range (NaN: none)."""
    cx0: int
    cy0: int
    width: int
    height: int
    n_inside: int
    n_outside: int
    n_occupied: int
    n_shadowed: int
    n_filled: int
    n_empty: int
    z_min: float
    z_max: float


@dataclass
class GroundInfo:
    """o3dr_ground_filter's record (include/o3dr_terrain.h): the box in cells, the points inside and outside it, the
    occupied cells, the ground cells and points, the cells the DTM's fill reached and those without a value, and the
    cells every iteration removed (n_removed has n_iterations entries)."""
    cx0: int
    cy0: int
    width: int
    height: int
    n_inside: int
    n_outside: int
    n_occupied: int
    n_ground_cells: int
    n_ground_points: int
    n_dtm_filled: int
    n_dtm_empty: int
    n_iterations: int
    n_removed: tuple


@dataclass
class InterpolateInfo:
    """o3dr_raster_interpolate's record (include/o3dr_dem.h): the raster's shape, the pyramid's levels, the data cells, the
    holes that got a value and those left NaN (max_level), and the cells per level (n_by_level has n_levels entries)."""
    width: int
    height: int
    n_levels: int
    n_data: int
    n_filled: int
    n_empty: int
    n_by_level: tuple


@dataclass
class ContourInfo:
    """o3dr_raster_contours' record (include/o3dr_contour.h): the quads without a NaN corner and those a level
    crosses, the segments, the lines and how many of them are closed, the polyline vertices (n_segments + n_lines), the
    segments of the longest line, the least and the greatest level index emitted (both 0 when nothing is)."""
    n_quads: int
    n_quads_crossed: int
    n_segments: int
    n_lines: int
    n_closed: int
    n_vertices: int
    n_longest: int
    k_lo: int
    k_hi: int


def contourPolylines(lines, vertices):
    """contourRaster's lines and vertices as a list of float64 [n_segments + 1, 2] arrays, one per line in line order (a
    closed line's last vertex is its first).  Host only: CUDA tensors are copied back first."""
    if _is_torch(lines):
        lines = lines.cpu().numpy()
    if _is_torch(vertices):
        vertices = vertices.cpu().numpy()
    lines = np.ascontiguousarray(lines)
    if lines.dtype != L.CONTOUR_LINE:
        lines = lines.view(L.CONTOUR_LINE).reshape(-1)
    vertices = np.asarray(vertices, np.float64).reshape(-1, 2)
    return [vertices[int(b):int(b) + int(n) + 1].copy() for b, n in zip(lines["begin"], lines["n_segments"])]


@dataclass
class ClusterInfo:
    """o3dr_cluster_euclidean's counters (include/o3dr_objects.h): the components of the links' closure, those kept as
    clusters and those rejected as too small / too large, the points in clusters and in rejected components, the size of
    the largest component, and the linked pairs i < j."""
    n_components: int
    n_clusters: int
    n_too_small: int
    n_too_large: int
    n_clustered_points: int
    n_rejected_points: int
    largest: int
    n_pairs: int


def _ground_params(cell_size, max_window_radius, window_base, exponential, slope, initial_distance, max_distance):
    prm = L.GroundParamsStruct()
    L.load_library().o3dr_ground_default_params(C.byref(prm))
    prm.cell_size, prm.max_window_radius, prm.window_base = float(cell_size), int(max_window_radius), int(window_base)
    prm.exponential = 1 if exponential else 0
    prm.slope, prm.initial_distance, prm.max_distance = float(slope), float(initial_distance), float(max_distance)
    return prm


def groundSchedule(cell_size, max_window_radius=16, window_base=2, exponential=True, slope=0.7, initial_distance=0.15,
                   max_distance=10.0):
    """The ground filter's window schedule (contract: include/o3dr_terrain.h "ground filter", step 3) -> (radii int32,
    thresholds float32), one entry per iteration.  Host only: needs the built library, not a GPU."""
    prm = _ground_params(cell_size, max_window_radius, window_base, exponential, slope, initial_distance, max_distance)
    radii, thr, n = np.zeros(16, np.int32), np.zeros(16, np.float32), C.c_int32(0)
    L.check(L.load_library().o3dr_ground_schedule(C.byref(prm), radii.ctypes.data, thr.ctypes.data, C.byref(n)))
    return radii[:n.value].copy(), thr[:n.value].copy()


@dataclass
class RigidResult:
    """o3dr_estimate_rigid_transform's result for one segment: T (float64 4x4, src -> tgt), the rms residual at T over the
    used pairs, their number and the status (RIGID_OK, RIGID_TOO_FEW, RIGID_DEGENERATE; T is the identity unless OK)."""
    T: np.ndarray
    rms: float
    n_used: int
    status: int

    @staticmethod
    def from_record(r):
        return _result(RigidResult, r, T=np.array(r["T"], np.float64).reshape(4, 4))


@dataclass
class RefineResult:
    """o3dr_pose_graph_refine's result: the energy and the 2-norm of the gradient over the free frames at the input and at
    the output poses, max |step| of the last Gauss-Newton iteration, the frames per role, the edges, the correspondences
    over the edges and the flags (REFINE_FLAG_CG_STOPPED, REFINE_FLAG_SINGULAR)."""
    energy_before: float
    energy_after: float
    grad_before: float
    grad_after: float
    last_step: float
    n_free: int
    n_gauge: int
    n_floating: int
    n_rejected: int
    n_edges: int
    n_used: int
    flags: int


@dataclass
class DisparityFilterInfo:
    """o3dr_disparity_filter's counts for one frame: non-zero pixels after the median, components among them, components
    and pixels removed as speckles, and the size of the largest component (0: none)."""
    n_valid: int
    n_components: int
    n_speckles: int
    n_removed: int
    largest: int


@dataclass
class MultiviewInfo:
    """o3dr_multiview_filter's counts for one frame: valid pixels, those kept, those removed for lack of support and for
    their violations, and the neighbour tests of each class over (valid pixel, listed neighbour)."""
    n_valid: int
    n_kept: int
    n_no_support: int
    n_violated: int
    n_outside: int
    n_hole: int
    n_support: int
    n_violation: int
    n_occluded: int


@dataclass
class MultiviewFuseInfo:
    """o3dr_multiview_fuse's counts for one frame: the filter's counts for the same call, the supports that voted and
    those that did not (their sum is filter.n_support), and the kept pixels with at least one vote."""
    filter: MultiviewInfo
    n_votes: int
    n_votes_dropped: int
    n_fused: int


@dataclass
class SegmentInfo:
    """o3dr_segment_image's counts for one frame: k-means centres, components of equal raw labels, components merged into
    another one, final labels, and the pixel counts of the largest and the smallest label."""
    n_centres: int
    n_components: int
    n_merged: int
    n_labels: int
    largest: int
    smallest: int


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def rectifiedQ(P1, P2):
    """The 4 x 4 disparity-to-depth matrix Q (what set_camera takes) of a rectified pair from its two projections (3 x 4,
    OpenCV's P1 / P2), by stereoRectify's formula: Tx = P2[0][3] / P2[0][0]; rows [1, 0, 0, -cx1], [0, 1, 0, -cy1],
    [0, 0, 0, f], [0, 0, -1 / Tx, (cx1 - cx2) / Tx].  Host only."""
    P1, P2 = np.asarray(P1, np.float64).reshape(3, 4), np.asarray(P2, np.float64).reshape(3, 4)
    f, cx1, cy1, cx2 = P1[0, 0], P1[0, 2], P1[1, 2], P2[0, 2]
    Tx = P2[0, 3] / P2[0, 0]
    return np.array([[1.0, 0.0, 0.0, -cx1], [0.0, 1.0, 0.0, -cy1], [0.0, 0.0, 0.0, f], [0.0, 0.0, -1.0 / Tx, (cx1 - cx2) / Tx]])


def nearbyFrames(poses, k=4, max_distance=float("inf")):
    """Per frame the k nearest other frames by the distance of the poses' translation columns, none farther than
    max_distance (contract: include/o3dr.h "multi-view filter", step 1).  poses: [F, 4, 4] or [F, 16] float32 -> int32
    [F, k], padded with -1.  Host only: needs the built library, not a GPU."""
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
    out = np.full((len(poses), int(k)), -1, np.int32)
    L.check(L.load_library().o3dr_nearby_frames(poses.ctypes.data, len(poses), int(k), float(max_distance), out.ctypes.data))
    return out


StackLayout = namedtuple("StackLayout", "single F rows cols ch pitch fs copy")


def image_stack_layout(shape, strides, itemsize, colour, contiguous=False):
    """How the image operators read an array as a stack of images (the library's side of the contract:
    csrc/o3dr_image_stack.h).  shape / strides (in bytes) / itemsize: the array's; colour=True: uint8 images, [H, W] or
    [F, H, W] grey, [H, W, 3] or [F, H, W, 3] B G R (a 3-D array whose last axis is 3 is one B G R image); colour=False:
    images of itemsize-byte elements, [H, W] or [F, H, W].  -> StackLayout: single (one image, no frame axis), F, rows, cols,
    ch, pitch and fs in bytes (fs 0 for a single image) and copy: whether the array must be made contiguous first - pitch and
    fs are then those of the copy.  Dense pixels with rows at least a row apart and frames at least a frame apart pass through as
    they are, padding included; contiguous=True asks for the copy regardless.  Pure: no array is touched."""
    nd, E = len(shape), int(itemsize)
    ch = 3 if colour and (nd == 4 or (nd == 3 and int(shape[-1]) == 3)) else 1
    assert nd in ((3, 4) if ch == 3 else (2, 3))
    single = nd == (3 if ch == 3 else 2)
    row_axis = -3 if ch == 3 else -2
    F, rows, cols = (1 if single else int(shape[0])), int(shape[row_axis]), int(shape[row_axis + 1])
    st = [int(v) for v in strides]
    passes = st[-1] == E and (ch == 1 or st[-2] == 3 * E) and st[row_axis] >= cols * ch * E and (single or st[0] >= rows * st[row_axis])
    if passes and not contiguous:
        return StackLayout(single, F, rows, cols, ch, st[row_axis], 0 if single else st[0], False)
    pitch = cols * ch * E
    return StackLayout(single, F, rows, cols, ch, pitch, 0 if single else rows * pitch, True)


_TORCH_DTYPE = {np.uint8: "uint8", np.uint16: "int16", np.int32: "int32", np.uint32: "int32", np.float32: "float32",
                np.float64: "float64"}


def _dtype_name(x):
    """"uint8", "int16", ...: of a numpy array or a torch tensor"""
    return str(x.dtype).replace("torch.", "")


def _itemsize(x):
    return x.element_size() if _is_torch(x) else x.itemsize


def _addr(x, n=1):
    """the address of an array or tensor; None (NULL) for one not asked for and for one of n = 0 elements the library
    neither reads nor writes"""
    return None if x is None or not n else (x.data_ptr() if _is_torch(x) else x.ctypes.data)


def _head(x, n):
    """the first n rows of an output (None: not asked for)"""
    return None if x is None else x[:n]


def _unsigned(x):
    """A returned int16 / int32 tensor that holds unsigned bits, viewed as uint16 / uint32 where torch has the type (a
    numpy output is unsigned as it is made)."""
    if not _is_torch(x):
        return x
    import torch
    u = getattr(torch, "u" + _dtype_name(x), None)
    return x if u is None else x.view(u)


def _mem(x):
    """the MEM kind of an array or tensor (a torch host tensor is host memory)"""
    return L.MEM_DEVICE if _is_torch(x) and x.is_cuda else L.MEM_HOST


# An array the library reads, as an intake hands it on: the array or tensor to keep alive, its rows, its address (None:
# no rows - the entry points return on n = 0 before they look at the pointer) and its MEM kind.
Input = namedtuple("Input", "x n addr mem")
Raster = namedtuple("Raster", "raster H W addr mem")

# Output specs of Context._empty_like besides (shape, dtype): n rows, never fewer than one allocated (a tensor is never
# empty, a capacity never 0), which the caller slices on return.  A numpy record dtype gives records on the host and on the
# device the tensor the operators return for it: int32 [n, itemsize / 4] for the records of 4-byte fields listed in
# _WORD_RECORDS (words: another 4-byte type for them, such as the one of the cloud the points come from), uint8
# [n, itemsize] for the others.
_Rows = namedtuple("_Rows", "n dtype tail words")
_WORD_RECORDS = (POINT, L.ORB_KEYPOINT, L.KNN2)


def _rows(n, dtype, *tail, words=np.int32):
    return _Rows(int(n), dtype, tail, words)


def _out_spec(sp, host):
    """(shape, dtype) of one _empty_like spec in host or device memory"""
    if not isinstance(sp, _Rows):
        return sp
    n, dtype = max(sp.n, 1), sp.dtype
    if host or getattr(dtype, "names", None) is None:
        return (n,) + sp.tail, dtype
    words = dtype in _WORD_RECORDS
    return (n, dtype.itemsize // (4 if words else 1)), sp.words if words else np.uint8


def _result(cls, res, **override):
    """A ctypes result struct (or a numpy record) as its dataclass, by field name - the dataclass's order may differ from
    the struct's: integers through int, floats through float, ctypes arrays as tuples, a nested struct as the field's
    own dataclass; override: the fields that are not a plain copy."""
    def value(f):
        v = res[f.name] if isinstance(res, np.void) else getattr(res, f.name)
        if isinstance(v, C.Structure):
            return _result(f.type, v)
        if isinstance(v, C.Array):
            return tuple(v)
        return int(v) if isinstance(v, (int, np.integer)) else float(v)
    return cls(**{f.name: override[f.name] if f.name in override else value(f) for f in fields(cls)})


def _returned(always, *optional):
    """A method's return value: the values it always returns, then the value of every (flag, value) pair whose flag is
    set; the bare value when that is exactly one."""
    ret = tuple(always) + tuple(v for on, v in optional if on)
    return ret[0] if len(ret) == 1 else ret


def _ptr(x):
    """(address, MEM kind, keepalive) of a numpy array or a torch tensor."""
    if _is_torch(x):
        assert x.is_contiguous()
        return x.data_ptr(), (L.MEM_DEVICE if x.is_cuda else L.MEM_HOST), x
    return x.ctypes.data, L.MEM_HOST, x


class Context:
    def __init__(self, device=0, Q=None, params=None, stream=None):
        self._lib = L.load_library()
        h = C.c_void_p()
        L.check(self._lib.o3dr_ctx_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)
        self.stream_raw = 0
        self.params = Params()
        if Q is not None:
            self.set_camera(Q)
        if params is not None:
            self.set_params(params)
        if stream is not None:
            self.set_stream(stream)

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self._lib.o3dr_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- configuration ----------------------------------------------------------------------------
    def set_camera(self, Q):
        Q = np.ascontiguousarray(Q, np.float64).reshape(16)
        L.check(self._lib.o3dr_set_camera(self._h, Q.ctypes.data))

    def set_params(self, params):
        s = params.to_struct()
        L.check(self._lib.o3dr_set_params(self._h, C.byref(s)))
        self.params = params

    def set_stream(self, stream):
        """stream: a torch.cuda.Stream, a raw hipStream_t integer, or None for the context's own."""
        raw = getattr(stream, "cuda_stream", stream)
        L.check(self._lib.o3dr_ctx_set_stream(self._h, C.c_void_p(raw or 0)))
        self.stream_raw = int(raw or 0)  # 0: the context's own stream (dist.py orders collectives against it)

    def synchronize(self):
        L.check(self._lib.o3dr_ctx_synchronize(self._h))

    def max_points(self, rows, cols):
        return int(self._lib.o3dr_max_points(self._h, rows, cols))

    def device_info(self):
        name = C.create_string_buffer(256)
        cu, mem = C.c_int32(0), C.c_int64(0)
        L.check(self._lib.o3dr_device_info(self._h, name, 256, C.byref(cu), C.byref(mem)))
        return name.value.decode(), cu.value, mem.value

    # -- helpers ----------------------------------------------------------------------------------
    @staticmethod
    def _images(disp, bgr):
        if _is_torch(disp):
            rows, cols = disp.shape
            assert tuple(bgr.shape) == (rows, cols, 3)
            return rows, cols, disp.stride(0) * disp.element_size(), bgr.stride(0)
        rows, cols = disp.shape
        # u8 disparities, or float64 with Params.disparity_f64 (--use_segment_labels)
        assert disp.dtype in (np.uint8, np.float64) and bgr.dtype == np.uint8 and bgr.shape == (rows, cols, 3)
        assert disp.strides[1] == disp.itemsize and bgr.strides[2] == 1 and bgr.strides[1] == 3
        return rows, cols, disp.strides[0], bgr.strides[0]

    def _mem_after_torch(self, x):
        """_mem(x), after ordering the library behind the work torch's stream holds now when x is a CUDA tensor: an
        intake's last step, behind every torch operation that prepares what the call reads."""
        if _mem(x) == L.MEM_DEVICE:
            self._order_after_torch()
        return _mem(x)

    def _cloud(self, pts):
        """A cloud as the library reads it -> Input: a numpy array made contiguous POINT records, or a contiguous torch
        [N, 4] tensor of 4-byte elements as it is."""
        if _is_torch(pts):
            assert pts.is_contiguous() and tuple(pts.shape[1:]) == (4,) and pts.element_size() == 4
        else:
            pts = np.ascontiguousarray(pts, POINT)
        n = int(pts.shape[0])
        return Input(pts, n, _addr(pts, n), self._mem_after_torch(pts))

    def _raster(self, raster):
        """A float32 [height, width] raster as the library reads it, made contiguous -> Raster."""
        if _is_torch(raster):
            assert _dtype_name(raster) == "float32" and raster.dim() == 2
            raster = raster.contiguous()
        else:
            raster = np.ascontiguousarray(raster, np.float32)
            assert raster.ndim == 2
        H, W = (int(v) for v in raster.shape)
        return Raster(raster, H, W, _addr(raster, W * H), self._mem_after_torch(raster))

    def _empty_like(self, like, *specs, device=None, zeros=False):
        """Outputs in `like`'s memory (or on `device`), one per spec and None per None: (shape, dtype), or _rows(n, dtype,
        ...) for n rows or records that the caller slices on return.  dtype: a numpy type - a tensor gets the torch type
        of _TORCH_DTYPE, for uint16 / uint32 the int16 / int32 that holds the bits - or a torch type as it is.
        Uninitialised, or zeros.  The library call may follow at once: it is ordered behind torch's work."""
        if device is None and _mem(like) == L.MEM_HOST:  # (a torch host tensor is read as host memory: numpy outputs)
            make = np.zeros if zeros else np.empty
            return [None if sp is None else make(*_out_spec(sp, True)) for sp in specs]
        import torch
        make = torch.zeros if zeros else torch.empty

        def tensor(shape, dt):
            dt = dt if isinstance(dt, torch.dtype) else getattr(torch, _TORCH_DTYPE[dt])
            return make(shape, dtype=dt, device=like.device if device is None else device)
        outs = [None if sp is None else tensor(*_out_spec(sp, False)) for sp in specs]
        self._order_after_torch()
        return outs

    @staticmethod
    def _kp(kp_xy, like):
        if kp_xy is None:
            return 0, 0, None
        if _is_torch(kp_xy):
            return kp_xy.data_ptr(), int(kp_xy.shape[0]), kp_xy
        kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
        if _is_torch(like) and like.is_cuda:
            import torch
            t = torch.from_numpy(kp).to(like.device)
            return t.data_ptr(), len(kp), t
        return kp.ctypes.data, len(kp), kp

    @staticmethod
    def _T(T):
        return np.ascontiguousarray(T, np.float32).reshape(16)

    def _frame(self, fn_name, disp, bgr, T, kp_xy, with_status):
        rows, cols, dp, bp = self._images(disp, bgr)
        pd, mem, _k1 = _ptr(disp)
        pb, mem2, _k2 = _ptr(bgr)
        assert mem == mem2
        kp_ptr, n_kp, _k3 = self._kp(kp_xy, disp)
        cap = self.max_points(rows, cols) + n_kp
        out, = self._empty_like(disp, _rows(cap, POINT))
        n = C.c_int64(0)
        st = C.c_uint32(0)
        fn = getattr(self._lib, fn_name)
        args = [self._h, pd, dp, pb, bp, rows, cols]
        if T is not None:
            Tn = self._T(T)
            args.append(Tn.ctypes.data)
        args += [kp_ptr, n_kp, _addr(out), cap, C.byref(n)]
        if with_status:
            args.append(C.byref(st))
        args.append(mem)
        L.check(fn(*args))
        return out[: n.value], st.value

    # -- the reference's four entry points ---------------------------------------------------------
    def createSingleImgPtCloud(self, disp, bgr, kp_xy=None):
        """pose.h:198 / pose_functions.cpp:1030-1134 (camera-frame cloud of one frame)."""
        return self._frame("o3dr_create_single_img_pt_cloud", disp, bgr, None, kp_xy, False)[0]

    def transformPtCloud(self, pts, T):
        """pose.h:199 / pose_functions.cpp:1358-1362."""
        Tn = self._T(T)
        pts, n, p_in, mem = self._cloud(pts)
        out, = self._empty_like(pts, _rows(n, POINT))
        L.check(self._lib.o3dr_transform_pt_cloud(self._h, p_in, n, Tn.ctypes.data, _addr(out), mem))
        return out[:n]

    def reprojectTransform(self, disp, bgr, T, kp_xy=None):
        """A1+A2 fused: createSingleImgPtCloud followed by transformPtCloud (pose.cpp:603-607)."""
        return self._frame("o3dr_reproject_transform", disp, bgr, T, kp_xy, False)[0]

    def downsamplePtCloud(self, pts, combinedPtCloud, return_status=False):
        """pose.h:216 / pose_functions.cpp:1654-1709."""
        pts, n_in, p_in, mem = self._cloud(pts)
        out, = self._empty_like(pts, _rows(n_in, POINT))
        n = C.c_int64(0)
        st = C.c_uint32(0)
        L.check(self._lib.o3dr_downsample_pt_cloud(self._h, p_in, n_in, int(bool(combinedPtCloud)), _addr(out), len(out),
                                                  C.byref(n), C.byref(st), mem))
        return _returned((out[: n.value],), (return_status, st.value))

    def bilateralFilter(self, img, d, sigma_color, sigma_space):
        """cv::bilateralFilter on a u8 image (pose_functions.cpp:1044); numpy in/out or torch CUDA in/out."""
        if _is_torch(img):
            import torch
            assert img.dtype == torch.uint8 and img.dim() == 2 and img.stride(1) == 1
            out = torch.empty_like(img, memory_format=torch.contiguous_format)
            L.check(self._lib.o3dr_bilateral_filter_u8(self._h, img.data_ptr(), img.stride(0), img.shape[0], img.shape[1], int(d),
                                                       float(sigma_color), float(sigma_space), out.data_ptr(), out.stride(0),
                                                       L.MEM_DEVICE if img.is_cuda else L.MEM_HOST))
            if img.is_cuda:
                L.check(self._lib.o3dr_ctx_synchronize(self._h))  # the library's stream is not torch's
            return out
        img = np.asarray(img, np.uint8)
        assert img.ndim == 2 and img.strides[1] == 1
        out = np.empty(img.shape, np.uint8)
        L.check(self._lib.o3dr_bilateral_filter_u8(self._h, img.ctypes.data, img.strides[0], img.shape[0], img.shape[1], int(d),
                                                   float(sigma_color), float(sigma_space), out.ctypes.data, out.strides[0],
                                                   L.MEM_HOST))
        return out

    def disparityVariance(self, disp):
        """Pose::getVariance per frame (pose_functions.cpp:1007-1028) of a [F,H,W] or [H,W] u8 stack -> float64 [F]"""
        if disp.ndim == 2:
            disp = disp[None]
        F, rows, cols = (int(v) for v in disp.shape)
        if _is_torch(disp):
            assert disp.stride(2) == 1
            ptr, mem, fs, pitch = disp.data_ptr(), (L.MEM_DEVICE if disp.is_cuda else L.MEM_HOST), disp.stride(0), disp.stride(1)
        else:
            disp = np.asarray(disp, np.uint8)
            assert disp.strides[2] == 1
            ptr, mem, fs, pitch = disp.ctypes.data, L.MEM_HOST, disp.strides[0], disp.strides[1]
        out = np.zeros(F, np.float64)
        L.check(self._lib.o3dr_disparity_variance(self._h, ptr, pitch, fs, rows, cols, F, out.ctypes.data, mem))
        return out

    def planeFitDisparity(self, disp, labels, n_labels=None, min_disparity=0.0, min_pixels=3, max_mse=0.0, fill=True,
                          return_segments=False):
        """--use_segment_labels: a least-squares plane over the disparity of every label's pixels (contract: include/o3dr.h,
        DESIGN.md "Plane-fitted disparity").  disp: [H,W] or [F,H,W] uint8; labels: the same shape, uint8 / uint16 / uint32
        (numpy), uint8 / int16 / int32 read as unsigned (torch), every value < n_labels (None: the largest label + 1).
        -> float64 image(s) of the same shape, what Params(disparity_f64=True) reads; with return_segments also the
        [F, n_labels] (or [n_labels]) PLANE_DISP_SEGMENT records (numpy).  numpy in, numpy out; torch CUDA tensors in, a
        CUDA float64 tensor out (nothing leaves HBM)."""
        single = disp.ndim == 2
        if single:
            disp, labels = disp[None], labels[None]
        F, rows, cols = (int(v) for v in disp.shape)
        assert tuple(int(v) for v in labels.shape) == (F, rows, cols), "disp and labels differ in shape"
        torch_in = _is_torch(disp)
        if torch_in:
            import torch
            assert _is_torch(labels) and disp.dtype == torch.uint8 and disp.device == labels.device
            assert labels.dtype in (torch.uint8, torch.int16, torch.int32, getattr(torch, "uint16", None), getattr(torch, "uint32", None))
            assert F == 0 or (disp.stride(2) == 1 and labels.stride(2) == 1)
            es = labels.element_size()
            pd, dfs, dp = disp.data_ptr(), disp.stride(0), disp.stride(1)
            pl, lfs, lp = labels.data_ptr(), labels.stride(0) * es, labels.stride(1) * es
            mem = L.MEM_DEVICE if disp.is_cuda else L.MEM_HOST
            if n_labels is None:
                n_labels = int(labels.max().item()) + 1 if labels.numel() else 1
        else:
            disp = np.asarray(disp)
            labels = np.asarray(labels)
            assert disp.dtype == np.uint8 and labels.dtype in (np.uint8, np.uint16, np.uint32)
            assert F == 0 or (disp.strides[2] == 1 and labels.strides[2] == labels.itemsize)
            es = labels.itemsize
            pd, dfs, dp = disp.ctypes.data, disp.strides[0], disp.strides[1]
            pl, lfs, lp = labels.ctypes.data, labels.strides[0], labels.strides[1]
            mem = L.MEM_HOST
            if n_labels is None:
                n_labels = int(labels.max()) + 1 if labels.size else 1
        n_labels = int(n_labels)
        prm = L.PlaneDispParamsStruct(float(min_disparity), int(min_pixels), float(max_mse), 1 if fill else 0)
        n_rec = F * n_labels if 1 <= n_labels <= L.PLANE_DISP_MAX_LABELS else 0
        st = C.c_uint32(0)
        if mem == L.MEM_DEVICE:
            out = torch.empty((F, rows, cols), dtype=torch.float64, device=disp.device)
            rec = torch.empty((max(n_rec, 1), 64), dtype=torch.uint8, device=disp.device) if return_segments else None
            self._order_after_torch()
            po, pr = out.data_ptr(), (rec.data_ptr() if return_segments else None)
        else:
            out = np.empty((F, rows, cols), np.float64)
            rec = np.empty(max(n_rec, 1), L.PLANE_DISP_SEGMENT) if return_segments else None
            po, pr = out.ctypes.data, (rec.ctypes.data if return_segments else None)
        L.check(self._lib.o3dr_plane_fit_disparity(self._h, pd, dp, dfs, pl, es, lp, lfs, n_labels, rows, cols, F, C.byref(prm),
                                                   po, pr, C.byref(st), mem))
        if torch_in and mem == L.MEM_HOST:
            out = torch.from_numpy(out)
        if single:
            out = out[0]
        if not return_segments:
            return out
        if mem == L.MEM_DEVICE:
            rec = rec.cpu().numpy().view(L.PLANE_DISP_SEGMENT).reshape(-1)
        rec = rec[:n_rec].reshape(F, n_labels)
        return out, (rec[0] if single else rec)

    def statisticalOutlierRemoval(self, pts):
        """pcl::StatisticalOutlierRemoval, mean_k 50, 1 sigma (pose_functions.cpp:1679-1684)."""
        pts, n_in, p_in, mem = self._cloud(pts)
        out, = self._empty_like(pts, _rows(n_in, POINT))
        n = C.c_int64(0)
        L.check(self._lib.o3dr_statistical_outlier_removal(self._h, p_in, n_in, _addr(out), len(out), C.byref(n), mem))
        return out[: n.value]

    # -- alignment (pcl::IterativeClosestPoint, pose.cpp:46-112 / pose_functions.cpp:1634-1652) -----------------------
    def nearestNeighbors(self, query, target, max_distance=float("inf")):
        """Exact nearest neighbour of every query point in `target`: -> (idx uint32, d2 float32), the point minimising
        (fp32 d2, original index); idx 0xFFFFFFFF / d2 inf where no target point lies within max_distance.  numpy POINT
        arrays, or torch [N,4] 4-byte CUDA tensors (results are then CUDA tensors too)."""
        q, t = self._cloud(query), self._cloud(target)
        if q.n and t.n:
            assert q.mem == t.mem, "query and target must live in the same memory"
        idx, d2 = self._empty_like(q.x, _rows(q.n, np.uint32), _rows(q.n, np.float32))
        L.check(self._lib.o3dr_nearest_neighbors(self._h, q.addr, q.n, t.addr, t.n, float(max_distance), _addr(idx), _addr(d2), q.mem))
        return _unsigned(idx[:q.n]), d2[:q.n]

    def icpAlign(self, source, target, T_init=None, max_iterations=10, max_correspondence_distance=float("inf"),
                 transformation_epsilon=0.0):
        """Point-to-point ICP of `source` onto `target` (contract: include/o3dr.h, DESIGN.md "ICP") -> IcpResult."""
        s, t = self._cloud(source), self._cloud(target)
        if s.n and t.n:
            assert s.mem == t.mem, "source and target must live in the same memory"
        Tn = None if T_init is None else self._T(T_init)
        prm = L.IcpParamsStruct(int(max_iterations), float(max_correspondence_distance), float(transformation_epsilon))
        res = L.IcpResultStruct()
        L.check(self._lib.o3dr_icp_align(self._h, s.addr, s.n, t.addr, t.n, _addr(Tn), C.byref(prm), C.byref(res),
                                         s.mem if s.n else t.mem))
        return _result(IcpResult, res, T=np.array(res.T[:], np.float64).reshape(4, 4))

    # -- surface smoothing (pcl::MovingLeastSquares, pose.cpp:27-112 / pose_functions.cpp:1711-1813) ---------------------
    def mlsSmooth(self, pts, search_radius, polynomial_order=2, sqr_gauss_param=0.0, return_normals=False, return_info=False,
                  fitted_only=False, out=None):
        """Moving-least-squares smoothing of every point (contract: include/o3dr.h, DESIGN.md "MLS").  numpy POINT arrays,
        or torch [N,4] 4-byte CUDA tensors such as cloudBigView() or finalize(device=...) (results are then CUDA tensors).
        -> the smoothed points, index-aligned with `pts`; with return_normals also [N,4] float32 (nx, ny, nz, curvature;
        NaN where no fit); with return_info also nn_count (uint32 / int32), fit (uint8, MLS_*) and an MlsResult.
        fitted_only: keep only the fitted points (fit != MLS_NONE), in input order.  out: where the points go (may be
        `pts` itself: in place)."""
        pts, n, p_in, mem = self._cloud(pts)
        prm = L.MlsParamsStruct(float(search_radius), int(polynomial_order), float(sqr_gauss_param))
        res = L.MlsResultStruct()
        per_point = return_info or fitted_only
        o, nrm, cnt, fit = self._empty_like(pts, _rows(n, POINT, words=pts.dtype) if out is None else None,
                                            _rows(n, np.float32, 4) if return_normals else None,
                                            _rows(n, np.uint32) if per_point else None, _rows(n, np.uint8) if per_point else None)
        if out is not None:
            o = out
            if mem == L.MEM_DEVICE:
                assert o.is_cuda and o.is_contiguous() and o.shape == pts.shape and o.element_size() == 4
            else:
                assert isinstance(o, np.ndarray) and o.dtype == POINT and o.shape == (n,) and o.flags.c_contiguous
        L.check(self._lib.o3dr_mls_smooth(self._h, p_in, n, C.byref(prm), _addr(o, n), _addr(nrm), _addr(cnt), _addr(fit), C.byref(res),
                                          mem))
        o, nrm, cnt, fit = o[:n], _head(nrm, n), _head(cnt, n), _head(fit, n)
        if fitted_only:
            keep = fit != L.MLS_NONE
            o, nrm, cnt, fit = o[keep], (None if nrm is None else nrm[keep]), cnt[keep], fit[keep]
        return _returned((o,), (return_normals, nrm), (return_info, _unsigned(cnt)), (return_info, fit),
                         (return_info, _result(MlsResult, res)))

    # -- plane segmentation (pcl::SACSegmentation + ProjectInliers, segmentCloud: pose_functions.cpp:2094-2249) -----------
    def segmentPlane(self, pts, distance_threshold, max_iterations=1000, tile_size=0.0, seed=0, optimize=True, project=False,
                     return_tile_index=False):
        """RANSAC plane segmentation of the whole cloud (tile_size 0) or of every XY tile (contract: include/o3dr.h,
        DESIGN.md "Plane segmentation").  numpy POINT arrays, or torch [N,4] 4-byte CUDA tensors such as cloudBigView() or
        finalize(device=...) (per-point results are then CUDA tensors).  -> (inlier mask (bool, index-aligned with `pts`),
        tile records (numpy PLANE_TILE array, tile order)); with project also the points with the inliers projected onto
        their tile's plane; with return_tile_index also every point's tile ordinal (int32)."""
        pts, n, p_in, mem = self._cloud(pts)
        prm = L.PlaneParamsStruct(float(distance_threshold), int(max_iterations), float(tile_size), int(seed) & (2**64 - 1),
                                  1 if optimize else 0)
        n_tiles = C.c_int64(0)
        cap = 1 if tile_size == 0 else 64
        for attempt in range(2):  # one retry with the tile count the first call reported
            inl, til, prj, rec = self._empty_like(pts, _rows(n, np.uint8), _rows(n, np.int32) if return_tile_index else None,
                                                  _rows(n, POINT, words=pts.dtype) if project else None, _rows(cap, L.PLANE_TILE))
            rc = self._lib.o3dr_segment_plane(self._h, p_in, n, C.byref(prm), _addr(inl, n), _addr(til, n), _addr(prj, n), _addr(rec),
                                              cap, C.byref(n_tiles), mem)
            if rc == L.ERR_CAPACITY and attempt == 0:
                cap = int(n_tiles.value)
                continue
            L.check(rc)
            break
        nt = int(n_tiles.value)
        if _is_torch(rec):  # (the tile records come back on the host)
            tiles = rec[:nt].cpu().numpy().view(L.PLANE_TILE).reshape(nt)
        else:
            tiles = rec[:nt].copy()
        return _returned((inl[:n] != 0, tiles), (project, _head(prj, n)), (return_tile_index, _head(til, n)))

    # -- image stacks: the inputs and outputs of the image operators below ------------------------------------------------
    @staticmethod
    def _image_stack(x, colour, contiguous=False):
        """A numpy array or a torch CUDA tensor as the library reads it (image_stack_layout) -> (x, made contiguous where
        its layout does not pass through; its StackLayout; its address; its MEM kind)."""
        if _is_torch(x):
            assert x.is_cuda
            E = _itemsize(x)
            lay = image_stack_layout(tuple(x.shape), [v * E for v in x.stride()], E, colour, contiguous)
            x = x.contiguous() if lay.copy else x
            return x, lay, x.data_ptr(), L.MEM_DEVICE
        x = np.asarray(x)
        lay = image_stack_layout(x.shape, x.strides, x.itemsize, colour, contiguous)
        x = np.ascontiguousarray(x) if lay.copy else x
        return x, lay, x.ctypes.data, L.MEM_HOST

    # -- ORB features (the reference's findFeatures / OrbFeaturesFinder, pose.cpp:127,210) -------------------------------
    def findFeatures(self, img, n_features=1500, scale_factor=1.3, n_levels=5, fast_threshold=20, edge=31, return_levels=False):
        """oFAST keypoints and steered-BRIEF descriptors (contract: include/o3dr.h "ORB features").  img: uint8 [H, W] or
        [F, H, W] grey, [H, W, 3] or [F, H, W, 3] B G R; numpy, or a torch CUDA tensor (the outputs are then CUDA tensors and
        nothing leaves HBM).  -> (keypoints, kp_xy [n, 2] float32, desc [n, 32] uint8, offsets): keypoints is an
        ORB_KEYPOINT array (torch: int32 [n, 8], the same bytes); offsets (numpy int64, F + 1) delimits the frames' rows.
        kp_xy / desc / offsets go straight into matchDescriptors, keypoints3D and accumulateFrames(keypoints=(kp_xy,
        offsets)) (accumulateFrames splits the pair into per-frame lists on the host: a CUDA kp_xy is read back there).
        return_levels: a fifth value, every frame's grey pyramid as a flat uint8 array (frame-major, levels back to back,
        rows tight)."""
        img, (_, F, rows, cols, ch, pitch, fs, _), pi, mem = self._image_stack(img, colour=True)
        assert _dtype_name(img) == "uint8"
        prm = L.OrbParamsStruct(int(n_features), float(scale_factor), int(n_levels), int(fast_threshold), int(edge), ch)
        wh = np.zeros(2 * max(int(n_levels), 1), np.int32)
        L.check(self._lib.o3dr_orb_level_sizes(rows, cols, C.byref(prm), wh.ctypes.data, None))
        cap = max(F * int(n_features), 1)
        n_lev = F * int(sum(int(wh[2 * l]) * int(wh[2 * l + 1]) for l in range(int(n_levels)))) if return_levels else 0
        kp, xy, desc, lev = self._empty_like(img, _rows(cap, L.ORB_KEYPOINT), ((cap, 2), np.float32), ((cap, 32), np.uint8),
                                             _rows(n_lev, np.uint8) if return_levels else None)
        off = np.zeros(F + 1, np.int64)
        n = C.c_int64(0)
        L.check(self._lib.o3dr_orb_detect(self._h, pi, fs, pitch, rows, cols, F, C.byref(prm), _addr(kp), _addr(xy), _addr(desc),
                                          off.ctypes.data, _addr(lev), cap, C.byref(n), mem))
        k = int(n.value)
        return _returned((kp[:k], xy[:k], desc[:k], off), (return_levels, _head(lev, n_lev)))

    # -- stereo rectification (initUndistortRectifyMap + remap: what makes the pair the matcher takes) -------------------------
    def rectifyMaps(self, K, D, R, P, size, device=None):
        """The Q5 fixed-point undistort-rectify map of one camera (contract: include/o3dr.h "stereo rectification").  K: the
        3 x 3 camera matrix; D: 4, 5 or 8 distortion coefficients in OpenCV's order (zero-padded); R: the rectifying
        rotation (R1 / R2); P: the new projection (P1 / P2), 3 x 4 or 3 x 3; size = (rows_out, cols_out).  -> int32
        [rows_out, cols_out, 2] = (qx, qy), RECTIFY_OUTSIDE in both where the source position is out of the map's range;
        numpy, or with device= a torch CUDA tensor."""
        K = np.asarray(K, np.float64).reshape(3, 3)
        D = np.asarray(D, np.float64).reshape(-1)
        assert D.size in (4, 5, 8), "D must have 4, 5 or 8 entries"
        R = np.asarray(R, np.float64).reshape(3, 3)
        P = np.asarray(P, np.float64)
        assert P.shape in ((3, 4), (3, 3))
        P34 = np.zeros((3, 4))
        P34[:, :P.shape[1]] = P
        cam = L.RectifyCameraStruct()
        cam.K[:] = K.reshape(-1).tolist()
        cam.D[:] = D.tolist() + [0.0] * (8 - D.size)
        cam.R[:] = R.reshape(-1).tolist()
        cam.P[:] = P34.reshape(-1).tolist()
        rows_out, cols_out = int(size[0]), int(size[1])
        shape = (max(rows_out, 0), max(cols_out, 0), 2)
        maps, = self._empty_like(None, (shape, np.int32), device=device)
        L.check(self._lib.o3dr_rectify_maps(self._h, C.byref(cam), rows_out, cols_out, _addr(maps), _mem(maps)))
        return maps

    def rectify(self, img, maps, border=0, return_valid=False, group_frames=0):
        """Bilinear remap of img through one rectifyMaps result (contract: include/o3dr.h "stereo rectification").  img: uint8
        [H, W] or [F, H, W] grey, [H, W, 3] or [F, H, W, 3] B G R (a 3-D input whose last axis is 3 is one B G R image, as in
        stereoDisparity); a padded pitch or frame stride passes through.  maps: int32 [H_out, W_out, 2], of img's memory
        kind: numpy in gives numpy out, torch CUDA tensors in give CUDA tensors out and nothing leaves HBM.  -> the uint8
        image(s) of the map's size; a tap outside the source reads `border`.  return_valid: a uint8 [H_out, W_out] image
        follows, 1 where every tap of non-zero weight is inside the source.  group_frames: at most that many frames per
        launch; results do not depend on it."""
        dev = _is_torch(img)
        if dev != _is_torch(maps):
            raise L.O3drError(L.ERR_INVALID_ARG, "maps must be of the same memory kind as img")
        img, (single, F, rows, cols, ch, pitch, fs, _), pi, mem = self._image_stack(img, colour=True)
        assert _dtype_name(img) == "uint8"
        assert len(maps.shape) == 3 and int(maps.shape[2]) == 2
        rows_out, cols_out = int(maps.shape[0]), int(maps.shape[1])
        if dev:
            assert maps.is_cuda and _dtype_name(maps) == "int32"
            maps = maps.contiguous()
        else:
            maps = np.ascontiguousarray(maps, np.int32)
        shape = (() if single else (F,)) + (rows_out, cols_out) + ((3,) if ch == 3 else ())
        out, valid = self._empty_like(img, (shape, np.uint8), ((rows_out, cols_out), np.uint8) if return_valid else None)
        L.check(self._lib.o3dr_rectify_remap(self._h, pi, fs, pitch, rows, cols, ch, F, _addr(maps), rows_out, cols_out, int(border),
                                             int(group_frames), _addr(out), _addr(valid), mem))
        return _returned((out,), (return_valid, valid))

    # -- stereo disparity (the image every frame call starts from; the reference reads it from files) ----------------------
    def stereoDisparity(self, left, right, n_disparities=256, min_disparity=0, p1=10, p2=120, n_paths=8, uniqueness=10,
                        lr_max_diff=1, subpixel=False, return_cost=False, return_volume=False, group_frames=0, median=0,
                        speckle_size=0, speckle_diff=1, rectify=None):
        """Census-transform semi-global matching of a rectified pair (contract: include/o3dr.h "stereo disparity").  left /
        right: uint8 [H, W] or [F, H, W] grey, [H, W, 3] or [F, H, W, 3] B G R, same shape; numpy, or torch CUDA tensors (the
        outputs are then CUDA tensors and nothing leaves HBM).  A 3-D input whose last axis is 3 is taken as one B G R image
        (as findFeatures does): pass a grey stack of 3-pixel-wide frames one frame at a time.  -> the uint8 disparity image ([H, W] or [F, H, W]; 0: rejected):
        what accumulateFrames, disparityVariance and keypoints3D take.  subpixel=True: a float64 image instead, disp_q4 / 16.0
        (exact; rejected pixels 0.0): what the frame calls read under Params(disparity_f64=True).  return_cost: S at the winner
        (uint16) follows; return_volume: S itself (uint16 [..., H, W, D]) follows that.  group_frames: at most that many frames
        per launch group (0: as many as the scratch budget allows); results do not depend on it.  median (0, 3, 5) /
        speckle_size > 0: the image to be returned goes through filterDisparity first - disp with max_diff = speckle_diff,
        under subpixel=True disp_q4 with max_diff = 16 * speckle_diff before the division; cost and volume stay as they are.
        rectify=(maps_left, maps_right), two rectifyMaps results of one size: both inputs go through rectify() first and
        everything is computed on the rectified pair."""
        if rectify is not None:
            ml, mr = rectify
            assert tuple(ml.shape) == tuple(mr.shape), "the two rectification maps must have one size"
            left, right = self.rectify(left, ml, group_frames=group_frames), self.rectify(right, mr, group_frames=group_frames)
        dev = _is_torch(left)
        assert dev == _is_torch(right) and tuple(left.shape) == tuple(right.shape)
        (left, lay, pl, mem), (right, lay_r, pr, _) = (self._image_stack(x, colour=True) for x in (left, right))
        if lay != lay_r:  # (a padded layout passes through where both share it; anything else is made contiguous)
            (left, lay, pl, mem), (right, _, pr, _) = (self._image_stack(x, colour=True, contiguous=True) for x in (left, right))
        assert _dtype_name(left) == _dtype_name(right) == "uint8"
        single, F, rows, cols, ch, pitch, fs, _ = lay
        prm = L.StereoParamsStruct(int(n_disparities), int(min_disparity), int(p1), int(p2), int(n_paths), int(uniqueness),
                                   int(lr_max_diff), ch, int(group_frames))
        shape = (rows, cols) if single else (F, rows, cols)
        D = max(int(n_disparities), 1)
        # (a tensor holds uint16 bits as int16; viewed below)
        disp, q4, cost, vol = self._empty_like(left, None if subpixel else (shape, np.uint8), (shape, np.uint16) if subpixel else None,
                                               (shape, np.uint16) if return_cost else None,
                                               (shape + (D,), np.uint16) if return_volume else None)
        L.check(self._lib.o3dr_stereo_disparity(self._h, pl, pr, fs, pitch, rows, cols, F, C.byref(prm), _addr(disp), _addr(q4),
                                                _addr(cost), _addr(vol), mem))
        if median or speckle_size:
            if subpixel:
                q4 = self.filterDisparity(q4, median, speckle_size, 16 * int(speckle_diff), group_frames=group_frames)
            else:
                disp = self.filterDisparity(disp, median, speckle_size, speckle_diff, group_frames=group_frames)
        if dev:  # (every value is below 2^15, so the int16 tensors hold the uint16 bits and their values)
            import torch
            out = q4.to(torch.float64) / 16.0 if subpixel else disp
            cost = None if cost is None else cost.view(torch.uint16)
            vol = None if vol is None else vol.view(torch.uint16)
        else:
            out = q4.astype(np.float64) / 16.0 if subpixel else disp
        return _returned((out,), (return_cost, cost), (return_volume, vol))

    # -- disparity filter (what production matchers end with: medianBlur, then filterSpeckles) --------------------------------
    def filterDisparity(self, disp, median=0, max_speckle_size=0, max_diff=1, return_labels=False, return_sizes=False,
                        return_info=False, group_frames=0):
        """k x k median (0: off, 3, 5), then removal of the connected components of at most max_speckle_size pixels (0: off;
        4-neighbours are joined iff both are non-zero and differ by at most max_diff) - contract: include/o3dr.h "disparity
        filter".  disp: uint8 or uint16, [H, W] or [F, H, W], a padded pitch or frame stride passes through; numpy, or a
        torch CUDA tensor (uint8, or uint16 / int16 holding the uint16 bits; the outputs are then CUDA tensors and nothing
        leaves HBM).  -> the filtered image in the input's type; return_labels / return_sizes: int32 images follow (the
        lowest pixel index of the pixel's component, -1 for a zero pixel; its pixel count), as they are before the removal;
        return_info: a list of DisparityFilterInfo, one per frame, follows.  group_frames: at most that many frames per
        launch group; results do not depend on it."""
        disp, (single, F, rows, cols, _, pitch, fs, _), pi, mem = self._image_stack(disp, colour=False)
        assert _dtype_name(disp) in (("uint8", "uint16", "int16") if _is_torch(disp) else ("uint8", "uint16"))
        prm = L.DisparityFilterParamsStruct(_itemsize(disp), int(median), int(max_speckle_size), int(max_diff), int(group_frames))
        shape = (rows, cols) if single else (F, rows, cols)
        out, labels, sizes = self._empty_like(disp, (shape, disp.dtype), (shape, np.int32) if return_labels else None,
                                              (shape, np.int32) if return_sizes else None)
        info = (L.DisparityFilterInfoStruct * F)() if return_info else None
        L.check(self._lib.o3dr_disparity_filter(self._h, pi, fs, pitch, rows, cols, F, C.byref(prm), _addr(out), _addr(labels),
                                                _addr(sizes), C.cast(info, C.c_void_p) if return_info else None, mem))
        infos = [_result(DisparityFilterInfo, i) for i in info or ()]
        return _returned((out,), (return_labels, labels), (return_sizes, sizes), (return_info, infos))

    # -- multi-view filter (the consistency test across frames that multi-view stereo pipelines end on) -----------------------
    def multiviewHomographies(self, poses, neighbors):
        """The matrices multiviewFilter uses: H[i, n] carries (x, y, level, 1) of frame i to frame neighbors[i, n]
        (contract: include/o3dr.h "multi-view filter", step 2).  -> float64 [F, k, 4, 4], zeros for a -1 entry.  No device work."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 16)
        F = len(poses)
        neighbors = np.ascontiguousarray(neighbors, np.int32).reshape(F, -1)
        k = int(neighbors.shape[1])
        H = np.zeros((F, k, 4, 4), np.float64)
        L.check(self._lib.o3dr_multiview_homographies(self._h, poses.ctypes.data, F, neighbors.ctypes.data, k, H.ctypes.data))
        return H

    def multiviewFilter(self, disp, poses, neighbors=None, k=4, max_distance=float("inf"), tolerance=1.0, min_support=1,
                        max_violations=-1, return_support=False, return_violations=False, return_info=False):
        """Every valid pixel of every frame is carried into each of the frame's neighbours by their poses and compared with
        what the neighbour saw there; it stays iff at least min_support neighbours agree within `tolerance` levels and (
        max_violations = -1) fewer of them see through it than agree, or (n >= 0) at most n see through it - contract:
        include/o3dr.h "multi-view filter".  disp: [F, H, W] uint8 (levels), uint16 (sixteenths) or float64 (levels), a
        padded pitch or frame stride passes through; numpy, or a torch CUDA tensor (int16 holding the uint16 bits is taken
        as uint16; the outputs are then CUDA tensors and nothing leaves HBM).  poses: [F, 4, 4] float32 camera-to-world,
        host.  neighbors: int32 [F, k'] (-1: none), or None: nearbyFrames(poses, k, max_distance).  -> the filtered images
        in the input's type; return_support / return_violations: uint8 count images follow; return_info: a list of
        MultiviewInfo, one per frame, follows."""
        dev = _is_torch(disp)
        nd = disp.dim() if dev else np.ndim(disp)
        assert nd == 3
        F, rows, cols = (int(v) for v in disp.shape)
        poses = np.ascontiguousarray(poses.cpu().numpy() if _is_torch(poses) else poses, np.float32).reshape(-1, 16)
        assert len(poses) == F
        if neighbors is None:
            neighbors = nearbyFrames(poses, k, max_distance)
        neighbors = np.ascontiguousarray(neighbors.cpu().numpy() if _is_torch(neighbors) else neighbors, np.int32).reshape(F, -1)
        kk = int(neighbors.shape[1])
        disp, (_, _, _, _, _, pitch, fs, _), pi, mem = self._image_stack(disp, colour=False)
        assert _dtype_name(disp) in (("uint8", "uint16", "int16", "float64") if dev else ("uint8", "uint16", "float64"))
        prm = L.MultiviewParamsStruct(_itemsize(disp), float(tolerance), int(min_support), int(max_violations))
        shape = (F, rows, cols)
        out, support, violations = self._empty_like(disp, (shape, disp.dtype), (shape, np.uint8) if return_support else None,
                                                    (shape, np.uint8) if return_violations else None)
        info = (L.MultiviewInfoStruct * F)() if return_info else None
        L.check(self._lib.o3dr_multiview_filter(self._h, pi, fs, pitch, rows, cols, F, poses.ctypes.data, neighbors.ctypes.data, kk,
                                                C.byref(prm), _addr(out), _addr(support), _addr(violations),
                                                C.cast(info, C.c_void_p) if return_info else None, mem))
        infos = [_result(MultiviewInfo, i) for i in info or ()]
        return _returned((out,), (return_support, support), (return_violations, violations), (return_info, infos))

    def multiviewFuse(self, disp, poses, neighbors=None, k=4, max_distance=float("inf"), tolerance=1.0, min_support=1,
                      max_violations=-1, return_votes=False, return_support=False, return_violations=False, return_info=False):
        """multiviewFilter's tests and keep rule, and for every kept pixel the mean of its own level and the levels its
        supporting neighbours vote for (the level on the pixel's own ray at which the neighbour would have seen exactly what
        it saw), summed in the order of the neighbour list - contract: include/o3dr.h "multi-view fusion".  Inputs as in
        multiviewFilter.  -> float64 levels [F, H, W], 0.0 at a removed or invalid pixel: what Params(disparity_f64=True)
        and the frame calls read; numpy in gives numpy out, a torch CUDA tensor gives CUDA tensors and nothing leaves HBM.
        return_votes / return_support / return_violations: uint8 count images follow in that order; return_info: a list of
        MultiviewFuseInfo, one per frame, follows."""
        dev = _is_torch(disp)
        nd = disp.dim() if dev else np.ndim(disp)
        assert nd == 3
        F, rows, cols = (int(v) for v in disp.shape)
        poses = np.ascontiguousarray(poses.cpu().numpy() if _is_torch(poses) else poses, np.float32).reshape(-1, 16)
        assert len(poses) == F
        if neighbors is None:
            neighbors = nearbyFrames(poses, k, max_distance)
        neighbors = np.ascontiguousarray(neighbors.cpu().numpy() if _is_torch(neighbors) else neighbors, np.int32).reshape(F, -1)
        kk = int(neighbors.shape[1])
        disp, (_, _, _, _, _, pitch, fs, _), pi, mem = self._image_stack(disp, colour=False)
        assert _dtype_name(disp) in (("uint8", "uint16", "int16", "float64") if dev else ("uint8", "uint16", "float64"))
        prm = L.MultiviewParamsStruct(_itemsize(disp), float(tolerance), int(min_support), int(max_violations))
        shape = (F, rows, cols)
        out, votes, support, violations = self._empty_like(disp, (shape, np.float64), (shape, np.uint8) if return_votes else None,
                                                           (shape, np.uint8) if return_support else None,
                                                           (shape, np.uint8) if return_violations else None)
        info = (L.MultiviewFuseInfoStruct * F)() if return_info else None
        L.check(self._lib.o3dr_multiview_fuse(self._h, pi, fs, pitch, rows, cols, F, poses.ctypes.data, neighbors.ctypes.data, kk,
                                              C.byref(prm), _addr(out), _addr(votes), _addr(support), _addr(violations),
                                              C.cast(info, C.c_void_p) if return_info else None, mem))
        infos = [_result(MultiviewFuseInfo, i) for i in info or ()]
        return _returned((out,), (return_votes, votes), (return_support, support), (return_violations, violations), (return_info, infos))

    # -- image segmentation (the label image planeFitDisparity reads; the reference takes it from offline files) ---------------
    def segmentImage(self, img, step=16, compactness=20, iterations=5, min_size=None, return_raw=False, return_sizes=False,
                     return_info=False, group_frames=0):
        """Superpixel labels of a colour image: grid-seeded integer k-means (step, compactness, iterations), connected
        components, merge of the components below min_size pixels (None: step * step / 4; 0: none) into their nearest
        neighbour in colour, labels numbered 0 .. n - 1 by first pixel - contract: include/o3dr.h "image segmentation".
        img: uint8 [H, W] or [F, H, W] grey, [H, W, 3] or [F, H, W, 3] B G R (a 3-D input whose last axis is 3 is one B G R
        image, as in stereoDisparity); a padded pitch or frame stride passes through.  numpy in gives a numpy uint32 label
        image, a torch CUDA tensor gives an int32 CUDA tensor and nothing leaves HBM: either goes into
        planeFitDisparity(disp, labels) as it is.  return_raw / return_sizes: int32 images follow (the k-means centre of
        every pixel; the pixel count of its label); return_info: a list of SegmentInfo, one per frame, follows.
        group_frames: at most that many frames per launch group; results do not depend on it."""
        img, (single, F, rows, cols, ch, pitch, fs, _), pi, mem = self._image_stack(img, colour=True)
        assert _dtype_name(img) == "uint8"
        prm = L.SegmentParamsStruct(ch, int(step), int(compactness), int(iterations), -1 if min_size is None else int(min_size),
                                    int(group_frames))
        shape = (rows, cols) if single else (F, rows, cols)
        labels, raw, sizes = self._empty_like(img, (shape, np.int32), (shape, np.int32) if return_raw else None,
                                              (shape, np.int32) if return_sizes else None)
        info = (L.SegmentInfoStruct * F)() if return_info else None
        L.check(self._lib.o3dr_segment_image(self._h, pi, fs, pitch, rows, cols, F, C.byref(prm), _addr(labels), _addr(raw), _addr(sizes),
                                             C.cast(info, C.c_void_p) if return_info else None, mem))
        if not _is_torch(img):
            labels = labels.view(np.uint32)  # (never negative)
        infos = [_result(SegmentInfo, i) for i in info or ()]
        return _returned((labels,), (return_raw, raw), (return_sizes, sizes), (return_info, infos))

    # -- feature matching (BFMatcher NORM_HAMMING knnMatch k=2 + ratio test, pose.h:180 / pose_functions.cpp:2017, and
    #    TransformationEstimationSVD, pose.cpp:213-235) --------------------------------------------------------------------
    def _desc(self, desc):
        """Descriptor rows as the library reads them -> Input: a numpy array made contiguous uint8 [N, 32], or a
        contiguous torch [N, 32] tensor of 1-byte elements as it is."""
        if _is_torch(desc):
            assert desc.is_contiguous() and desc.element_size() == 1 and desc.dim() == 2 and desc.shape[1] == 32
        else:
            desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = int(desc.shape[0])
        return Input(desc, n, _addr(desc, n), self._mem_after_torch(desc))

    def _point_pairs(self, src, tgt, mask, seg_offsets):
        """The index-aligned point pairs of estimateRigidTransform / ransacRigid as the library reads them -> (src, tgt
        (Input), mask (uint8, kept alive; None: absent), segs (int64 array or None), n_segs)."""
        if mask is not None:  # (before the intakes: they order the call behind this conversion too)
            mask = mask.byte().contiguous() if _is_torch(mask) else np.ascontiguousarray(mask).astype(np.uint8)
        s, t = self._cloud(src), self._cloud(tgt)
        assert s.n == t.n, "src and tgt must be index-aligned"
        if s.n:
            assert s.mem == t.mem, "src and tgt must live in the same memory"
        segs = None if seg_offsets is None else np.ascontiguousarray(seg_offsets, np.int64).reshape(-1)
        return s, t, mask, segs, 1 if segs is None else len(segs) - 1

    def _feature_pool(self, desc, kp3, offsets):
        """The pool of poseChain / refinePoses as the library reads it -> (desc, kp3 (Input), off (int64 array), F)."""
        d, k = self._desc(desc), self._cloud(kp3)
        assert d.n == k.n, "kp3 must be index-aligned with desc"
        if d.n:
            assert d.mem == k.mem, "desc and kp3 must live in the same memory"
        off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        return d, k, off, len(off) - 1

    @staticmethod
    def _ransac_params(threshold, seed, iterations):
        return L.RansacParamsStruct(float(threshold), int(seed) & 0xFFFFFFFFFFFFFFFF, int(iterations), 0)

    def matchDescriptors(self, desc, offsets, pairs, ratio=0.5, max_distance=40):
        """Brute-force Hamming 2-NN of every query row of every (query_set, train_set) pair (contract: include/o3dr.h,
        DESIGN.md "Feature matching").  desc: uint8 [N, 32] (numpy, or a torch CUDA tensor: results are then CUDA tensors);
        offsets: the n_sets + 1 row offsets of the sets; pairs: [P, 2] set indices.  -> (records (numpy KNN2 array, or a
        torch int32 [n, 4] tensor: train_idx[2], distance[2] as bits), good (bool mask)); pair p's records follow those of
        the pairs before it."""
        d = self._desc(desc)
        off = np.ascontiguousarray(offsets, np.int64).reshape(-1)
        prs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        n_sets = len(off) - 1
        n_rec = int(sum(int(off[q + 1] - off[q]) for q, _ in prs)) if n_sets > 0 else 0
        prm = L.MatchParamsStruct(float(ratio), int(max_distance))
        n = C.c_int64(0)
        rec, good = self._empty_like(d.x, _rows(n_rec, L.KNN2), _rows(n_rec, np.uint8))
        L.check(self._lib.o3dr_match_knn2_hamming(self._h, d.addr, off.ctypes.data, n_sets, _addr(prs, len(prs)), len(prs),
                                                  C.byref(prm), _addr(rec), _addr(good), len(rec), C.byref(n), d.mem))
        assert n.value == n_rec
        return rec[:n_rec], good[:n_rec] != 0

    def keypoints3D(self, disp, kp_xy, poses=None, bgr=None):
        """One point per keypoint, index-aligned (what findFeatures does with Q; contract: include/o3dr.h): the point A1's
        keypoint pass emits for an accepted keypoint (posed by poses[f] when given, rgba 0 without bgr), NaN x y z and rgba
        0 for a rejected one.  disp: one frame [H, W] with kp_xy [n, 2], or a stack [F, H, W] with a list of F arrays;
        poses: None, [4, 4] or [F, 4, 4] float32; bgr: None or [H, W, 3] / [F, H, W, 3] uint8.  numpy, or torch CUDA
        tensors (the result is then a CUDA [n, 4] tensor)."""
        dev = _is_torch(disp)
        single = (disp.dim() if dev else np.ndim(disp)) == 2
        F = 1 if single else int(disp.shape[0])
        rows, cols = int(disp.shape[-2]), int(disp.shape[-1])
        kps = [kp_xy] if single else list(kp_xy)
        if dev:
            import torch
            assert disp.is_cuda
            disp = disp.contiguous()
            kp = torch.cat([torch.as_tensor(k, dtype=torch.float32, device=disp.device).reshape(-1, 2) for k in kps]).contiguous()
            counts = [int(torch.as_tensor(k).reshape(-1, 2).shape[0]) for k in kps]
            ps = None if poses is None else torch.as_tensor(poses, dtype=torch.float32, device=disp.device).contiguous()
            bg = None if bgr is None else bgr.contiguous()
        else:
            disp = np.ascontiguousarray(disp)
            kp = np.ascontiguousarray(np.concatenate([np.asarray(k, np.float32).reshape(-1, 2) for k in kps]))
            counts = [len(np.asarray(k).reshape(-1, 2)) for k in kps]
            ps = None if poses is None else np.ascontiguousarray(poses, np.float32)
            bg = None if bgr is None else np.ascontiguousarray(bgr, np.uint8)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        n_kp, es = int(off[-1]), _itemsize(disp)
        out, = self._empty_like(disp, _rows(n_kp, POINT))
        n = C.c_int64(0)
        L.check(self._lib.o3dr_keypoints_3d(self._h, _addr(disp), rows * cols * es, cols * es, _addr(bg), rows * cols * 3, cols * 3, rows,
                                            cols, _addr(ps), F, _addr(kp, n_kp), off.ctypes.data, _addr(out), len(out), C.byref(n),
                                            _mem(disp)))
        return out[:n_kp]

    def estimateRigidTransform(self, src, tgt, seg_offsets=None, mask=None):
        """Batched TransformationEstimationSVD (contract: include/o3dr.h, DESIGN.md "Feature matching"): per segment the
        rigid T mapping src onto tgt over the index-aligned pairs with mask != 0 and finite coordinates.  numpy POINT arrays,
        or torch [N,4] 4-byte CUDA tensors (mask then a CUDA uint8 / bool tensor).  -> RigidResult, or a list of them with
        seg_offsets (the n_segs + 1 segment boundaries)."""
        s, t, mask, segs, n_segs = self._point_pairs(src, tgt, mask, seg_offsets)
        res = np.zeros(max(n_segs, 1), L.RIGID_RESULT)
        L.check(self._lib.o3dr_estimate_rigid_transform(self._h, s.addr, t.addr, s.n, _addr(segs), n_segs, _addr(mask), res.ctypes.data,
                                                        s.mem))
        out = [RigidResult.from_record(r) for r in res[:n_segs]]
        return out[0] if segs is None else out

    def ransacRigid(self, src, tgt, threshold, iterations=256, seed=0, seg_offsets=None, mask=None, seg_keys=None):
        """Batched three-point RANSAC for a rigid transform (contract: include/o3dr.h "robust rigid fit", DESIGN.md "Robust
        fit"): per segment the hypothesis with the most pairs within `threshold` metres, of `iterations` hypotheses drawn
        with `seed` and the segment's key (seg_keys, uint64 per segment; default: its ordinal).  Inputs as
        estimateRigidTransform's.  -> (inlier: bool mask index-aligned with src - numpy, or a CUDA tensor for CUDA inputs -,
        records: a numpy RANSAC_RESULT array, one per segment)."""
        s, t, mask, segs, n_segs = self._point_pairs(src, tgt, mask, seg_offsets)
        keys = None if seg_keys is None else np.ascontiguousarray(seg_keys, np.uint64).reshape(-1)
        assert keys is None or len(keys) == n_segs, "one key per segment"
        prm = self._ransac_params(threshold, seed, iterations)
        res = np.zeros(max(n_segs, 1), L.RANSAC_RESULT)
        inl, = self._empty_like(s.x, _rows(s.n, np.uint8), zeros=True)
        L.check(self._lib.o3dr_ransac_rigid(self._h, s.addr, t.addr, s.n, _addr(segs), n_segs, _addr(mask), _addr(keys), C.byref(prm),
                                            _addr(inl), res.ctypes.data, s.mem))
        return inl[:s.n] != 0, res[:n_segs]

    def matchFeatures(self, desc_q, desc_t, kp3_q, kp3_t, ratio=0.5, max_distance=40, ransac_threshold=None, ransac_iterations=256,
                      ransac_seed=0):
        """One frame pair of the reference's feature-matched mode (generate_tf_of_Matched_Keypoints, pose.cpp:213-235):
        2-NN match desc_q against desc_t, keep the good matches whose 3-D keypoints (kp3_q, kp3_t: index-aligned with the
        descriptors, e.g. from keypoints3D) are finite on both sides, and fit T mapping the query's points onto the
        train's.  With ransac_threshold (metres) the kept matches first go through ransacRigid (key 0) and the fit runs on
        its inliers: the kept mask is then the inlier mask.  All numpy, or all torch CUDA tensors (the gather then stays on
        the device).  -> (records, kept mask (bool, one per query row), RigidResult)."""
        (dq, nq, _, _), (dt, nt, _, _) = self._desc(desc_q), self._desc(desc_t)
        (kq, nkq, _, _), (kt, nkt, _, _) = self._cloud(kp3_q), self._cloud(kp3_t)
        assert nkq == nq and nkt == nt, "the 3-D keypoints must be index-aligned with the descriptors"
        pairs = np.array([[0, 1]], np.int32)
        offsets = np.array([0, nq, nq + nt], np.int64)
        if _is_torch(dq):
            import torch
            rec, good = self.matchDescriptors(torch.cat([dq, dt]), offsets, pairs, ratio, max_distance)
            idx = rec[:, 0].to(torch.int64)  # 0xFFFFFFFF reads as -1
            tgt = kt[idx.clamp(0, max(nt - 1, 0))] if nt else torch.zeros_like(kq)
            fin = lambda p: torch.isfinite(p.view(torch.float32)[:, :3]).all(1)  # noqa: E731
            keep = good & (idx >= 0) & fin(kq) & fin(tgt)
            tgt = tgt.contiguous()
            if ransac_threshold is not None:
                keep, _r = self.ransacRigid(kq, tgt, ransac_threshold, ransac_iterations, ransac_seed, mask=keep)
            res = self.estimateRigidTransform(kq, tgt, mask=keep)
            return rec, keep, res
        rec, good = self.matchDescriptors(np.concatenate([dq, dt]), offsets, pairs, ratio, max_distance)
        idx = rec["train_idx"][:, 0].astype(np.int64)
        tgt = np.ascontiguousarray(kt[np.clip(idx, 0, max(nt - 1, 0))]) if nt else np.zeros_like(kq)
        fin = lambda p: np.isfinite(p["x"]) & np.isfinite(p["y"]) & np.isfinite(p["z"])  # noqa: E731
        keep = good & fin(kq) & fin(tgt)
        if ransac_threshold is not None:
            keep, _r = self.ransacRigid(kq, tgt, ransac_threshold, ransac_iterations, ransac_seed, mask=keep)
        res = self.estimateRigidTransform(kq, tgt, mask=keep)
        return rec, keep, res

    # -- pose chain (the reference's default mode: generate_tf_of_Matched_Keypoints per frame, pose.cpp:213-235) -----------
    def poseChain(self, desc, offsets, kp3, prior_poses, n_fixed=0, poses_in=None, status_in=None, dist_nearby=2.0, range_width=8,
                  min_matches=30, max_rms=float("inf"), ratio=0.5, max_distance=40, return_pairs=False, ransac_threshold=None,
                  ransac_iterations=256, ransac_seed=0, return_ransac=False, refine=False, refine_kw=None):
        """Every frame's pose from descriptor matches against earlier nearby frames (contract: include/o3dr.h "pose chain",
        DESIGN.md "Pose chain"): the static pair list from prior_poses, one batched matching pass, one launch that walks the
        frames n_fixed .. F - 1 in order.  desc uint8 [N, 32], kp3 N points in the camera frame (keypoints3D with poses=None),
        offsets the F + 1 row offsets (findFeatures'); all numpy, or desc / kp3 torch CUDA tensors.  prior_poses [F, 4, 4];
        the first n_fixed frames are history with poses_in [n_fixed, 4, 4] and status_in [n_fixed] (an earlier call's
        outputs).  These three are read on the host (a CUDA tensor is copied back first).
        With ransac_threshold (metres) every pair's correspondences first go through the three-point RANSAC of ransacRigid
        in camera coordinates (key = query frame << 32 | train frame) and the walk uses the inliers only.
        -> (poses [F, 4, 4] float32: numpy, or a CUDA tensor for CUDA inputs; records: a numpy CHAIN_FRAME array, one per
        frame), with return_pairs the pair list, int32 [P, 2] (query frame, train frame), and with return_ransac a numpy
        RANSAC_RESULT array, one per pair of the list (empty without ransac_threshold).
        refine=True: refinePoses runs on the outputs and the pair list (the history frames fixed; ratio, max_distance and
        the ransac_* keywords passed through; refine_kw: its other keywords); the poses returned are the refined ones, the
        records stay the chain's, and the RefineResult is appended to the tuple."""
        d, k3, off, F = self._feature_pool(desc, kp3, offsets)
        host = lambda a, dt: np.ascontiguousarray(a.detach().cpu().numpy() if _is_torch(a) else a, dt)  # noqa: E731
        prior = host(prior_poses, np.float32).reshape(-1, 16)
        assert F >= 0 and len(prior) == F, "one prior pose per frame"
        n_fixed = int(n_fixed)
        pin = host(poses_in, np.float32).reshape(-1, 16) if poses_in is not None else np.zeros((0, 16), np.float32)
        sin = host(status_in, np.int32).reshape(-1) if status_in is not None else np.zeros(0, np.int32)
        if 0 < n_fixed <= F:
            assert len(pin) >= n_fixed and len(sin) >= n_fixed, "poses_in / status_in must cover the history"
        prm = L.ChainParamsStruct(float(dist_nearby), float(max_rms), int(range_width), int(min_matches), float(ratio),
                                  int(max_distance))
        rec = np.zeros(max(F, 1), L.CHAIN_FRAME)
        robust = ransac_threshold is not None
        want_pairs = return_pairs or (robust and return_ransac) or refine
        cap = max(F * L.CHAIN_MAX_RANGE, 1) if want_pairs else 0
        prs = np.zeros((cap, 2), np.int32) if want_pairs else None
        rprm = self._ransac_params(ransac_threshold, ransac_seed, ransac_iterations) if robust else None
        rres = np.zeros(cap, L.RANSAC_RESULT) if robust and return_ransac else None
        n_pairs = C.c_int64(0)
        poses, = self._empty_like(d.x, _rows(F, np.float32, 16), zeros=True)
        args = (self._h, d.addr, off.ctypes.data, k3.addr, prior.ctypes.data, F, n_fixed, _addr(pin, len(pin)), _addr(sin, len(sin)),
                C.byref(prm), _addr(poses), rec.ctypes.data, _addr(prs), cap, C.byref(n_pairs), d.mem)
        if robust:
            L.check(self._lib.o3dr_pose_chain_robust(*args, C.byref(rprm), _addr(rres)))
        else:
            L.check(self._lib.o3dr_pose_chain(*args))
        res = (poses[:F].reshape(F, 4, 4), rec[:F])
        rr = None
        if refine:
            kw = dict(refine_kw or {})
            fx = np.zeros(F, bool)
            fx[:max(min(n_fixed, F), 0)] = True
            kw.setdefault("fixed", fx)
            if kw.get("prior_weight", 0.0) > 0.0:
                kw.setdefault("prior_poses", prior)
            refined, _frames, rr = self.refinePoses(d.x, off, k3.x, res[0], rec["status"][:F], prs[: n_pairs.value], ratio=ratio,
                                                    max_distance=max_distance, ransac_threshold=ransac_threshold,
                                                    ransac_iterations=ransac_iterations, ransac_seed=ransac_seed, **kw)
            res = (refined, rec[:F])
        return _returned(res, (return_pairs, _head(prs, n_pairs.value)),
                         (return_ransac, rres[: n_pairs.value] if rres is not None else np.zeros(0, L.RANSAC_RESULT)), (refine, rr))

    # -- pose-graph refinement (the bundle adjustment the reference leaves commented out: pose_functions.cpp:1876-1921) -----
    def refinePoses(self, desc, offsets, kp3, poses, status, pairs, fixed=None, prior_poses=None, prior_weight=0.0, gn_iterations=5,
                    cg_iterations=32, min_pair_matches=3, ratio=0.5, max_distance=40, ransac_threshold=None, ransac_iterations=256,
                    ransac_seed=0, return_edges=False):
        """One joint least-squares refinement of a pose chain's accepted frames over all `pairs` at once (contract:
        include/o3dr.h "pose graph", DESIGN.md "Pose-graph refinement").  desc, offsets, kp3 as in poseChain; poses
        [F, 4, 4] and status [F] are poseChain's outputs, pairs its pair list (int32 [P, 2]); these, fixed ([F] bool: frames
        to hold) and prior_poses ([F, 4, 4], needed iff prior_weight > 0) are read on the host.  The ransac_* keywords are
        poseChain's.  -> (poses [F, 4, 4] float32: numpy, or a CUDA tensor for CUDA desc / kp3; records: a numpy
        REFINE_FRAME array, one per frame; RefineResult), with return_edges a numpy REFINE_EDGE array, one per pair."""
        d, k3, off, F = self._feature_pool(desc, kp3, offsets)
        host = lambda a, dt: np.ascontiguousarray(a.detach().cpu().numpy() if _is_torch(a) else a, dt)  # noqa: E731
        pin = host(poses, np.float32).reshape(-1, 16)
        sin = host(status, np.int32).reshape(-1)
        assert F >= 0 and len(pin) == F and len(sin) == F, "one pose and one status per frame"
        prs = host(pairs, np.int32).reshape(-1, 2)
        P = len(prs)
        fx = None if fixed is None else np.ascontiguousarray(host(fixed, np.bool_).reshape(-1).astype(np.uint8))
        assert fx is None or len(fx) == F, "one fixed flag per frame"
        pri = None if prior_poses is None else host(prior_poses, np.float32).reshape(-1, 16)
        assert pri is None or len(pri) == F, "one prior pose per frame"
        prm = L.RefineParamsStruct(float(prior_weight), int(gn_iterations), int(cg_iterations), int(min_pair_matches), float(ratio),
                                   int(max_distance), 0)
        rprm = None if ransac_threshold is None else self._ransac_params(ransac_threshold, ransac_seed, ransac_iterations)
        rec = np.zeros(max(F, 1), L.REFINE_FRAME)
        edg = np.zeros(max(P, 1), L.REFINE_EDGE) if return_edges else None
        res = L.RefineResultStruct()
        out, = self._empty_like(d.x, _rows(F, np.float32, 16), zeros=True)
        L.check(self._lib.o3dr_pose_graph_refine(
            self._h, d.addr, off.ctypes.data, k3.addr, F, _addr(pin, F), _addr(sin, F), _addr(fx, F), _addr(pri, F), _addr(prs, P), P,
            C.byref(prm), None if rprm is None else C.byref(rprm), _addr(out), rec.ctypes.data, _addr(edg), C.byref(res), d.mem))
        return _returned((out[:F].reshape(F, 4, 4), rec[:F], _result(RefineResult, res)), (return_edges, _head(edg, P)))

    def trackFrames(self, img, disp, prior_poses, n_features=1500, scale_factor=1.3, n_levels=5, fast_threshold=20, edge=31,
                    **chain_kwargs):
        """findFeatures(img), keypoints3D(disp, poses=None) and poseChain over a stack of frames (img [F, H, W] or
        [F, H, W, 3] uint8, disp [F, H, W]; numpy or torch CUDA tensors).  chain_kwargs: poseChain's keywords (the
        ransac_* ones and refine / refine_kw among them).
        -> (poses, records, (kp_xy, offsets)) and poseChain's further outputs; the pair feeds accumulateFrames(keypoints=...)
        for the accepted frames."""
        _kp, xy, desc, off = self.findFeatures(img, n_features=n_features, scale_factor=scale_factor, n_levels=n_levels,
                                               fast_threshold=fast_threshold, edge=edge)
        kp3 = self.keypoints3D(disp, [xy[int(off[f]):int(off[f + 1])] for f in range(len(off) - 1)], poses=None)
        res = self.poseChain(desc, off, kp3, prior_poses, **chain_kwargs)
        return res[:2] + ((xy, off),) + res[2:]

    # -- surface mesh (pcl::GreedyProjectionTriangulation at --mesh_surface: pose_functions.cpp:1711-1813) -----------------
    def meshSurface(self, pts, cell_size, max_edge_length, return_normals=False, return_info=False):
        """Height-field triangulation of the occupied XY cells (contract: include/o3dr.h, DESIGN.md "Surface mesh").
        numpy POINT arrays, or torch [N,4] 4-byte CUDA tensors such as finalize(device=...) (results are then CUDA
        tensors).  -> int32 [T, 3] triangles (input indices, counter-clockwise in XY, in quad order); with return_normals
        also [N, 3] float32 vertex normals (NaN for shadowed points and vertices without a triangle); with return_info
        also a MeshResult.  One library call: the triangle buffer holds the bound of 2 n triangles."""
        pts, n, p_in, mem = self._cloud(pts)
        prm = L.MeshParamsStruct(float(cell_size), float(max_edge_length))
        res = L.MeshResultStruct()
        n_tris = C.c_int64(0)
        cap = 2 * n
        tri, nrm = self._empty_like(pts, _rows(cap, np.int32, 3), _rows(n, np.float32, 3) if return_normals else None)
        L.check(self._lib.o3dr_mesh_surface(self._h, p_in, n, C.byref(prm), _addr(tri), cap, C.byref(n_tris), _addr(nrm), C.byref(res),
                                            mem))
        return _returned((tri[:int(n_tris.value)],), (return_normals, _head(nrm, n)), (return_info, _result(MeshResult, res)))

    # -- map raster: orthophoto, elevation raster, shaded relief (this build's own) ---------------
    def rasterExtent(self, pts, cell_size):
        """The cloud's own cell box (cx0, cy0, width, height) at cell_size: what rasterizeMap(bounds=None) covers."""
        pts, n, p_in, mem = self._cloud(pts)
        box = [C.c_int32(0) for _ in range(4)]
        L.check(self._lib.o3dr_raster_extent(self._h, p_in, n, float(cell_size), *[C.byref(b) for b in box], mem))
        return tuple(int(b.value) for b in box)

    def rasterizeMap(self, pts, cell_size, bounds=None, select="first", fill_radius=0, light=None, return_source=False,
                     return_distance=False, return_info=False):
        """The map as [height, width] images, one pixel per XY cell of cell_size, rows ascending in cy (contract:
        include/o3dr.h "map raster", DESIGN.md "Map raster").  bounds = (cx0, cy0, width, height) in cells, None: the
        cloud's own box (rasterExtent).  select "first" | "top" | "bottom" picks a cell's point, fill_radius (0..32 cells)
        fills empty cells from the nearest occupied one, light = (lx, ly, lz) adds the shaded relief.  numpy POINT arrays
        give numpy arrays, torch [N,4] 4-byte CUDA tensors such as finalize(device=...) give CUDA tensors.
        -> (height_map float32, color uint8 [.., 3] B G R[, shade uint8][, source int32][, distance2 int32][, RasterInfo])"""
        pts, n, p_in, mem = self._cloud(pts)
        if select not in L.RASTER_SELECT:
            raise L.O3drError(L.ERR_INVALID_ARG, "select must be 'first', 'top' or 'bottom'")
        cx0, cy0, W, H = (int(v) for v in (self.rasterExtent(pts, cell_size) if bounds is None else bounds))
        prm = L.RasterParamsStruct()
        self._lib.o3dr_raster_default_params(C.byref(prm))
        prm.cell_size, prm.select, prm.fill_radius = float(cell_size), L.RASTER_SELECT[select], int(fill_radius)
        prm.cx0, prm.cy0, prm.width, prm.height = cx0, cy0, W, H
        if light is not None:
            prm.use_light = 1
            prm.light[:] = [float(v) for v in light]
        ok = 1 <= W and 1 <= H and W * H <= L.RASTER_MAX_CELLS  # (else the call fails before it writes anything)
        shape = (H, W) if ok else (1, 1)
        want = [("height_map", np.float32, ()), ("color", np.uint8, (3,))]
        want += [("shade", np.uint8, ())] if light is not None else []
        want += [("source", np.int32, ())] if return_source else []
        want += [("distance2", np.int32, ())] if return_distance else []
        outs = L.RasterOutputsStruct()
        arrays = self._empty_like(pts, *[(shape + tail, dt) for _, dt, tail in want])
        for (name, _, _), t in zip(want, arrays):
            setattr(outs, name, _addr(t))
        res = L.RasterResultStruct()
        L.check(self._lib.o3dr_rasterize_map(self._h, p_in, n, C.byref(prm), C.byref(outs), C.byref(res), mem))
        return _returned(arrays, (return_info, _result(RasterInfo, res)))

    # -- ground filter: ground mask, DTM, height above ground (this build's own) -----------------
    def groundFilter(self, pts, cell_size, bounds=None, max_window_radius=16, window_base=2, exponential=True, slope=0.7,
                     initial_distance=0.15, max_distance=10.0, fill_radius=0, return_height=False, return_dtm=False,
                     return_state=False, return_info=False, interpolate=False, smooth=2):
        """The bare-earth ground mask of a cloud by a progressive morphological filter on the XY cells of cell_size
        (contract: include/o3dr_terrain.h "ground filter", DESIGN.md "Ground filter").  bounds = (cx0, cy0, width, height)
        in cells, None: the cloud's own box (rasterExtent).  The windows grow to max_window_radius cells (1..128) by
        window_base, exponentially or linearly; slope, initial_distance and max_distance give every window's height
        threshold; fill_radius (0..32 cells) fills the DTM under what was removed.  interpolate=True (fill_radius must be
        0) interpolates the DTM from the ground cells instead, at any distance (interpolateRaster with `smooth`), and takes
        the heights above that DTM (sampleRaster): finite for every point inside the box; the mask and the states do not
        change.  numpy POINT arrays give numpy arrays, torch [N,4] 4-byte CUDA tensors such as finalize(device=...) give
        CUDA tensors.
        -> ground uint8 [n][, height_above_ground float32 [n]][, dtm float32 [height, width]][, cell_state uint8
        [height, width]][, GroundInfo[, InterpolateInfo with interpolate]]"""
        if interpolate and int(fill_radius) != 0:
            raise ValueError("groundFilter(interpolate=True) needs fill_radius = 0: the interpolation is the fill")
        pts, n, p_in, mem = self._cloud(pts)
        cx0, cy0, W, H = (int(v) for v in (self.rasterExtent(pts, cell_size) if bounds is None else bounds))
        prm = _ground_params(cell_size, max_window_radius, window_base, exponential, slope, initial_distance, max_distance)
        prm.cx0, prm.cy0, prm.width, prm.height, prm.fill_radius = cx0, cy0, W, H, int(fill_radius)
        ok = 1 <= W and 1 <= H and W * H <= L.RASTER_MAX_CELLS  # (else the call fails before it writes anything)
        shape = (H, W) if ok else (1, 1)
        want = [("ground", np.uint8, (n,))]
        want += [("height_above_ground", np.float32, (n,))] if return_height else []
        want += [("dtm", np.float32, shape)] if return_dtm or interpolate else []
        want += [("cell_state", np.uint8, shape)] if return_state else []
        if interpolate:  # (the heights come from sampleRaster)
            want = [w for w in want if w[0] != "height_above_ground"]
        outs = L.GroundOutputsStruct()
        arrays = self._empty_like(pts, *[(shp, dt) for _, dt, shp in want])
        for (name, _, shp), t in zip(want, arrays):
            setattr(outs, name, _addr(t, int(np.prod(shp))))
        res = L.GroundResultStruct()
        L.check(self._lib.o3dr_ground_filter(self._h, p_in, n, C.byref(prm), C.byref(outs), C.byref(res), mem))
        info, dem_info = _result(GroundInfo, res, n_removed=tuple(res.n_removed[:res.n_iterations])), None
        if interpolate:  # the DTM from the ground cells alone, at any distance; the heights above it
            got = dict(zip((name for name, _, _ in want), arrays))
            dtm, dem_info = self.interpolateRaster(got["dtm"], smooth=smooth, return_info=True)
            above = self.sampleRaster(pts, dtm, cell_size, (cx0, cy0, W, H)) if return_height else None
            arrays = [got["ground"]] + ([above] if return_height else []) + ([dtm] if return_dtm else [])
            arrays += [got["cell_state"]] if return_state else []
        return _returned(arrays, (return_info, info), (return_info and interpolate, dem_info))

    # -- raster interpolation and raster sample (this build's own) -------------------------------
    def interpolateRaster(self, raster, smooth=2, max_level=0, return_level=False, return_info=False):
        """Every hole (NaN) of a float32 [height, width] raster filled from the data around it, at any distance: pull-push
        over an image pyramid with `smooth` (0..8) Jacobi sweeps per level on the way down (contract: include/o3dr_dem.h
        "raster interpolation", DESIGN.md "Raster interpolation").  max_level (1..31) leaves the holes whose nearest data
        lies under a higher pyramid level NaN; 0: no limit.  A numpy array gives numpy arrays, a torch CUDA tensor gives
        CUDA tensors without leaving HBM.  -> filled float32[, level uint8][, InterpolateInfo]"""
        raster, H, W, p_in, mem = self._raster(raster)
        prm = L.InterpolateParamsStruct()
        self._lib.o3dr_interpolate_default_params(C.byref(prm))
        prm.width, prm.height, prm.smooth, prm.max_level = W, H, int(smooth), int(max_level)
        filled, level = self._empty_like(raster, ((H, W), np.float32), ((H, W), np.uint8) if return_level else None)
        outs = L.InterpolateOutputsStruct(_addr(filled, W * H), _addr(level, W * H))
        res = L.InterpolateResultStruct()
        L.check(self._lib.o3dr_raster_interpolate(self._h, p_in, C.byref(prm), C.byref(outs), C.byref(res), mem))
        info = _result(InterpolateInfo, res, n_by_level=tuple(res.n_by_level[:res.n_levels]))
        return _returned((filled,), (return_level, level), (return_info, info))

    def sampleRaster(self, pts, raster, cell_size, bounds, return_value=False, return_info=False):
        """A float32 [height, width] raster read back at every point: bounds = (cx0, cy0, width, height) is the raster's box
        in cells of cell_size (contract: include/o3dr_dem.h "raster sample").  The points and the raster live in the same
        memory: numpy POINT array and numpy raster, or torch CUDA tensors.
        -> height_above float32 [n] (z minus the raster at the point's cell; NaN outside the box or on a NaN cell)[, value
        float32 [n]][, (points inside the box, outside it, inside it on a NaN cell)]"""
        pts, n, p_in, mem = self._cloud(pts)
        cx0, cy0, W, H = (int(v) for v in bounds)
        raster, rH, rW, _, rmem = self._raster(raster)
        assert (rH, rW) == (H, W), "the raster's shape is (height, width) of bounds"
        assert rmem == mem, "the points and the raster live in the same memory"
        above, value = self._empty_like(pts, (n, np.float32), (n, np.float32) if return_value else None)
        counts = (C.c_int64 * 3)()
        # (the raster's address goes as it is: the library wants one even for a raster of no cells)
        L.check(self._lib.o3dr_raster_sample(self._h, p_in, n, float(cell_size), cx0, cy0, W, H, _addr(raster), _addr(value, n),
                                             _addr(above, n), counts, mem))
        return _returned((above,), (return_value, value), (return_info, tuple(int(v) for v in counts)))

    # -- contour lines of a raster (this build's own) ---------------------------------------------
    def contourRaster(self, raster, interval, base=0.0, cell_size=1.0, origin=(0, 0), return_lines=False, return_vertices=False,
                      return_info=False):
        """The contour lines of a float32 [height, width] raster at the levels base + k * interval: marching squares over
        the quads of four cell centres, the segments linked into lines and ranked along them (contract: include/o3dr_dem.h
        "contour lines", DESIGN.md "Contour lines").  A NaN is a hole: lines end beside it.  Element [r, c] is the value at
        the centre of cell (origin[0] + c, origin[1] + r) of cell_size, as rasterizeMap and groundFilter lay their rasters
        out with origin = bounds[:2].  A numpy array gives numpy records, a torch CUDA tensor gives CUDA tensors without
        leaving HBM (the same bytes: `.cpu().numpy().view(CONTOUR_SEGMENT)`).
        -> segments CONTOUR_SEGMENT [S] (torch: uint8 [S, 48])[, lines CONTOUR_LINE [n] (uint8 [n, 32])][, vertices float64
        [S + n, 2]: contourPolylines(lines, vertices) splits them][, ContourInfo]"""
        raster, H, W, p_in, mem = self._raster(raster)  # (the count call reads the raster before any output is made)
        prm = L.ContourParamsStruct()
        self._lib.o3dr_contour_default_params(C.byref(prm))
        prm.width, prm.height, prm.interval, prm.base, prm.cell_size = W, H, float(interval), float(base), float(cell_size)
        prm.cx0, prm.cy0 = int(origin[0]), int(origin[1])
        count = C.c_int64(0)
        L.check(self._lib.o3dr_raster_contours_count(self._h, p_in, C.byref(prm), C.byref(count), mem))
        S = int(count.value)  # n_lines <= S and n_vertices <= 2 S
        if S > L.CONTOUR_MAX_SEGMENTS:
            raise L.O3drError(L.ERR_CAPACITY, "the raster has more than 2^28 contour segments at this interval")
        seg, lin, ver = self._empty_like(raster, _rows(S, L.CONTOUR_SEGMENT), _rows(S, L.CONTOUR_LINE) if return_lines else None,
                                         _rows(2 * S, np.float64, 2) if return_vertices else None)
        outs = L.ContourOutputsStruct(_addr(seg, S), S, _addr(lin, S), S, _addr(ver, S), 2 * S)
        res = L.ContourResultStruct()
        L.check(self._lib.o3dr_raster_contours(self._h, p_in, C.byref(prm), C.byref(outs), C.byref(res), mem))
        return _returned((seg[:int(res.n_segments)],), (return_lines, _head(lin, int(res.n_lines))),
                         (return_vertices, _head(ver, int(res.n_vertices))), (return_info, _result(ContourInfo, res)))

    # -- Euclidean clustering: object labels and per-object records (this build's own) ----------
    def clusterCloud(self, pts, tolerance, min_size=1, max_size=None, return_clusters=False, return_raw=False, return_sizes=False,
                     return_indices=False, return_info=False):
        """Which points belong to the same object: points closer than `tolerance` are linked, a component of the links'
        closure with min_size <= points <= max_size (None: no limit) is a cluster, numbered by its lowest point index
        (contract: include/o3dr_objects.h, DESIGN.md "Euclidean clustering").  numpy POINT arrays give numpy arrays, torch
        [N,4] 4-byte CUDA tensors such as finalize(device=...) give CUDA tensors (the records then as a CUDA uint8
        [K, 64] tensor: `.cpu().numpy().view(CLUSTER)`).
        -> label int32 [n] (-1: rejected)[, clusters CLUSTER [K]][, raw int32 [n]][, sizes int32 [n]][, indices int32
        [n_clustered_points]][, ClusterInfo]"""
        pts, n, p_in, mem = self._cloud(pts)
        prm = L.ClusterParamsStruct()
        self._lib.o3dr_cluster_default_params(C.byref(prm))
        prm.tolerance, prm.min_size = float(tolerance), int(min_size)
        if max_size is not None:
            prm.max_size = int(max_size)
        cap = n // int(min_size) if return_clusters and int(min_size) >= 1 else 0  # no more clusters fit in n points
        want = ["label"] + [name for name, on in (("raw", return_raw), ("size", return_sizes), ("indices", return_indices)) if on]
        outs = L.ClusterOutputsStruct()
        rec, *made = self._empty_like(pts, _rows(cap, L.CLUSTER), *[(n, np.int32)] * len(want))
        arrays = dict(zip(want, made))
        for name in want:
            setattr(outs, name, _addr(arrays[name], n))
        res, k = L.ClusterResultStruct(), C.c_int64(0)
        L.check(self._lib.o3dr_cluster_euclidean(self._h, p_in, n, C.byref(prm), C.byref(outs), _addr(rec, cap), cap, C.byref(k),
                                                 C.byref(res), mem))
        return _returned((arrays["label"],), (return_clusters, rec[:min(int(k.value), cap)]), (return_raw, arrays.get("raw")),
                         (return_sizes, arrays.get("size")), (return_indices, _head(arrays.get("indices"), int(res.n_clustered_points))),
                         (return_info, _result(ClusterInfo, res)))

    def voxelGrid(self, pts, leaf, min_points=0, z_offset=0.0, return_status=False):
        """pcl::VoxelGrid<PointXYZRGB> as the reference configures it (pose_functions.cpp:1689-1700)."""
        pts, n_in, p_in, mem = self._cloud(pts)
        leaf = np.ascontiguousarray(leaf, np.float32).reshape(3)
        out, = self._empty_like(pts, _rows(n_in, POINT))
        n = C.c_int64(0)
        st = C.c_uint32(0)
        L.check(self._lib.o3dr_voxel_grid(self._h, p_in, n_in, leaf.ctypes.data, int(min_points), float(z_offset), _addr(out),
                                         len(out), C.byref(n), C.byref(st), mem))
        return _returned((out[: n.value],), (return_status, st.value))

    def createAndTransformPtCloud(self, disp, bgr, T, kp_xy=None, return_status=False):
        """pose.h:231 / pose.cpp:596-636."""
        out, st = self._frame("o3dr_create_and_transform_pt_cloud", disp, bgr, T, kp_xy, True)
        return (out, st) if return_status else out

    # -- fan-out / accumulate / final merge ---------------------------------------------------------
    def accumulateFrames(self, disp, bgr, poses, keypoints=None):
        """pose.cpp:365-434 for a stack of frames: disp [F,H,W] u8, bgr [F,H,W,3] u8, poses [F,4,4] f32;
        keypoints: optional list of F arrays [n_f,2] of (x,y) floats (KeyPoint::pt), or findFeatures' (kp_xy, offsets) pair
        (split into such lists on the host; a CUDA kp_xy is copied back first, which synchronises), used iff jump_pixels != 1."""
        F, rows, cols = disp.shape
        if _is_torch(disp):
            assert disp.is_contiguous() and bgr.is_contiguous() and poses.is_contiguous()
            es = disp.element_size()  # 1, or 8 with Params.disparity_f64
            dfs, dp, bfs, bp = disp.stride(0) * es, disp.stride(1) * es, bgr.stride(0), bgr.stride(1)
            assert poses.dtype.__str__() == "torch.float32" and poses.numel() == F * 16
        else:
            disp = np.ascontiguousarray(disp, np.float64 if np.asarray(disp).dtype == np.float64 else np.uint8)
            bgr = np.ascontiguousarray(bgr, np.uint8)
            poses = np.ascontiguousarray(poses, np.float32).reshape(F, 16)
            dfs, dp, bfs, bp = disp.strides[0], disp.strides[1], bgr.strides[0], bgr.strides[1]
        pd, mem, _k1 = _ptr(disp)
        pb, mem2, _k2 = _ptr(bgr)
        pp, mem3, _k3 = _ptr(poses)
        assert mem == mem2 == mem3
        if isinstance(keypoints, tuple):  # (kp_xy, offsets) as findFeatures returns them
            kxy, koff = keypoints
            if _is_torch(kxy):
                kxy = kxy.detach().cpu().numpy()
            kxy = np.asarray(kxy, np.float32).reshape(-1, 2)
            keypoints = [kxy[int(koff[f]):int(koff[f + 1])] for f in range(F)]
        if keypoints is not None:
            assert len(keypoints) == F
            kps = [np.ascontiguousarray(k, np.float32).reshape(-1, 2) for k in keypoints]
            offs = np.zeros(F + 1, np.int64)
            offs[1:] = np.cumsum([len(k) for k in kps])
            kp = np.concatenate(kps) if offs[-1] else np.zeros((0, 2), np.float32)
            if mem == L.MEM_DEVICE:
                import torch
                kp_t = torch.from_numpy(kp).to(disp.device)
                kp_ptr = kp_t.data_ptr()
            else:
                kp_ptr = kp.ctypes.data
            L.check(self._lib.o3dr_accumulate_frames_kp(self._h, pd, dfs, dp, pb, bfs, bp, rows, cols, pp, F, kp_ptr,
                                                        offs.ctypes.data, mem))
            if mem == L.MEM_DEVICE:
                L.check(self._lib.o3dr_ctx_synchronize(self._h))  # kp_t must outlive the launches
            return
        L.check(self._lib.o3dr_accumulate_frames(self._h, pd, dfs, dp, pb, bfs, bp, rows, cols, pp, F, mem))

    def cloudBigReserve(self, n_points):
        L.check(self._lib.o3dr_cloud_big_reserve(self._h, int(n_points)))

    def cloudBigReset(self):
        L.check(self._lib.o3dr_cloud_big_reset(self._h))

    def cloudBigSize(self):
        n = C.c_int64(0)
        st = C.c_uint32(0)
        L.check(self._lib.o3dr_cloud_big_size(self._h, C.byref(n), C.byref(st)))
        return n.value, st.value

    def cloudBigRead(self, device=None):
        n, _ = self.cloudBigSize()
        if device is not None:
            import torch
            out = torch.empty((max(n, 1), 4), dtype=torch.int32, device=device)
        else:
            out = np.empty(max(n, 1), POINT)
        po, mem, _k = _ptr(out)
        m = C.c_int64(0)
        L.check(self._lib.o3dr_cloud_big_read(self._h, po, max(n, 1), C.byref(m), mem))
        return out[: m.value]

    def cloudBigAppend(self, pts):
        if not _is_torch(pts):
            pts = np.ascontiguousarray(pts, POINT)
        pi, mem, _k = _ptr(pts)
        L.check(self._lib.o3dr_cloud_big_append(self._h, pi, int(pts.shape[0]), mem))

    def cloudBigTransform(self, T):
        Tn = self._T(T)
        L.check(self._lib.o3dr_cloud_big_transform(self._h, Tn.ctypes.data))

    # zero-copy views for the multi-GPU exchange (torch tensors over the library's HBM buffers)
    def cloudBigView(self):
        """[n,4] int32 CUDA tensor aliasing cloud_big (no copy); valid until the cloud is modified"""
        ptr = C.c_void_p()
        n = C.c_int64(0)
        L.check(self._lib.o3dr_cloud_big_view(self._h, C.byref(ptr), C.byref(n)))
        return _device_tensor(ptr.value, n.value, self.device)

    def cloudBigRecvBuffer(self, n_points):
        """[n_points,4] int32 CUDA tensor over the library's receive buffer"""
        ptr = C.c_void_p()
        L.check(self._lib.o3dr_cloud_big_recv_buffer(self._h, int(n_points), C.byref(ptr)))
        return _device_tensor(ptr.value, int(n_points), self.device)

    def cloudBigAdopt(self, n_points):
        """the first n_points of the receive buffer become cloud_big"""
        L.check(self._lib.o3dr_cloud_big_adopt(self._h, int(n_points)))

    def cloudBigHeaderDev(self):
        """this rank's 32-byte exchange header {min xyz, max xyz (f32), count (i64)} as a uint8 CUDA tensor; asynchronous"""
        import torch
        hdr = torch.empty(32, dtype=torch.uint8, device=torch.device("cuda", self.device))
        self._order_after_torch()
        L.check(self._lib.o3dr_cloud_big_header_dev(self._h, hdr.data_ptr()))
        return hdr

    def _order_after_torch(self):
        """The library writes on the context's stream into a block torch's allocator handed out on torch's current
        stream: when the two differ, the block's previous use on torch's stream must finish first."""
        import torch
        cur = torch.cuda.current_stream(self.device)
        if self.stream_raw != cur.cuda_stream:
            cur.synchronize()

    def cloudBigPartitionDev(self, hdrs, n_parts):
        """hdrs: the all-gathered headers ([world*32] uint8, CUDA).  Stable reorder of cloud_big by index slice of the
        combined grid over the box the headers span; -> int64 CUDA tensor [n_parts + 1]: slice counts, then the status
        word.  Asynchronous (no host round trip)."""
        import torch
        assert hdrs.is_cuda and hdrs.is_contiguous() and hdrs.numel() % 32 == 0
        counts = torch.empty(n_parts + 1, dtype=torch.int64, device=hdrs.device)
        self._order_after_torch()
        L.check(self._lib.o3dr_cloud_big_partition_dev(self._h, hdrs.data_ptr(), hdrs.numel() // 32, int(n_parts), counts.data_ptr()))
        self._keep = hdrs  # (the launches read it)
        return counts

    def cloudBigSliceCountsDev(self, hdrs, n_parts):
        """hdrs: the all-gathered headers ([world*32] uint8, CUDA).  Slice sizes of cloud_big over the box the headers span,
        NOTHING MOVED: -> int64 CUDA tensor [n_parts + 1] (sizes, then the status word).  Asynchronous."""
        import torch
        assert hdrs.is_cuda and hdrs.is_contiguous() and hdrs.numel() % 32 == 0
        counts = torch.empty(n_parts + 1, dtype=torch.int64, device=hdrs.device)
        self._order_after_torch()
        L.check(self._lib.o3dr_cloud_big_slice_counts_dev(self._h, hdrs.data_ptr(), hdrs.numel() // 32, int(n_parts), counts.data_ptr()))
        self._keep = hdrs  # (the launches read it)
        return counts

    def cloudBigPlaceSlices(self, own_part, counts, n_before, n_after):
        """lay cloud_big out as [n_before free | own slice | n_after free | leaving slices]; -> offset of the leaving slices"""
        arr = (C.c_int64 * len(counts))(*[int(v) for v in counts])
        off = C.c_int64(0)
        L.check(self._lib.o3dr_cloud_big_place_slices(self._h, len(counts), int(own_part), arr, int(n_before), int(n_after), C.byref(off)))
        return off.value

    def cloudBigSetSize(self, n_points):
        """the first n_points of the cloud buffer are the cloud (after the exchange filled the gaps); stream-ordered"""
        L.check(self._lib.o3dr_cloud_big_set_size(self._h, int(n_points)))

    def cloudBigRawView(self):
        """[capacity,4] int32 CUDA tensor over the whole cloud buffer (valid until the next call that may reallocate it)"""
        ptr = C.c_void_p()
        cap = C.c_int64(0)
        L.check(self._lib.o3dr_cloud_big_raw_view(self._h, C.byref(ptr), C.byref(cap)))
        return _device_tensor(ptr.value, cap.value, self.device)

    def cloudBigCapacity(self):
        """(points cloud_big holds, points the receive buffer holds) without reallocating"""
        a, b = C.c_int64(0), C.c_int64(0)
        L.check(self._lib.o3dr_cloud_big_capacity(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def mergePartitionedStats(self):
        """what this context's last o3dr_merge_partitioned moved (include/o3dr.h)"""
        out = (C.c_int64 * 8)()
        L.check(self._lib.o3dr_merge_partitioned_stats(self._h, out))
        keys = ("points_local", "points_sent_off_rank", "points_received_off_rank", "bytes_sent", "bytes_received",
                "points_into_merge", "agreement_rounds", "points_all_ranks")
        return dict(zip(keys, (int(v) for v in out)))

    def cloudBigAssumeSize(self, n_points):
        """the caller read this rank's header back: cloud_big holds exactly n_points (saves the library its own round trips)"""
        L.check(self._lib.o3dr_cloud_big_assume_size(self._h, int(n_points)))

    def cloudBigBBox(self):
        """(min xyz, max xyz, count) of cloud_big; (+inf, -inf, 0) when empty"""
        mn = np.empty(3, np.float32)
        mx = np.empty(3, np.float32)
        n = C.c_int64(0)
        L.check(self._lib.o3dr_cloud_big_bbox(self._h, mn.ctypes.data, mx.ctypes.data, C.byref(n)))
        return mn, mx, n.value

    def cloudBigPartition(self, gmin, gmax, n_parts):
        """stable reorder of cloud_big by index slice of the combined grid over [gmin, gmax]; -> (counts, status)"""
        gmin = np.ascontiguousarray(gmin, np.float32)
        gmax = np.ascontiguousarray(gmax, np.float32)
        counts = (C.c_int64 * n_parts)()
        st = C.c_uint32(0)
        L.check(self._lib.o3dr_cloud_big_partition(self._h, gmin.ctypes.data, gmax.ctypes.data, n_parts, counts, C.byref(st)))
        return [int(v) for v in counts], st.value

    def finalize(self, device=None, return_status=False, gmin=None, gmax=None, n_hint=None):
        """cloud_small = downsamplePtCloud(cloud_big, true) (pose.cpp:530); with gmin/gmax the grid is laid
        over that (global) bounding box instead of cloud_big's own (multi-GPU merge).  n_hint: the caller knows
        cloud_big's size (after an adopt): the output is sized without asking the device."""
        n = int(n_hint) if n_hint is not None else self.cloudBigSize()[0]
        if device is not None:
            import torch
            out = torch.empty((max(n, 1), 4), dtype=torch.int32, device=device)
        else:
            out = np.empty(max(n, 1), POINT)
        po, mem, _k = _ptr(out)
        m = C.c_int64(0)
        st = C.c_uint32(0)
        if gmin is None:
            L.check(self._lib.o3dr_finalize(self._h, po, max(n, 1), C.byref(m), C.byref(st), mem))
        else:
            gmin = np.ascontiguousarray(gmin, np.float32)
            gmax = np.ascontiguousarray(gmax, np.float32)
            L.check(self._lib.o3dr_finalize_global(self._h, gmin.ctypes.data, gmax.ctypes.data, po, max(n, 1), C.byref(m),
                                                  C.byref(st), mem))
        return (out[: m.value], st.value) if return_status else out[: m.value]

    def finalizeIncremental(self, device=None, return_status=False):
        """finalize()'s result, bit for bit, folding only the points appended to cloud_big since the previous call
        (the reference's per-cycle preview, pose.cpp:437-448, 638-674); sized exactly by a size query first"""
        m = C.c_int64(0)
        st = C.c_uint32(0)
        L.check(self._lib.o3dr_finalize_incremental(self._h, None, 0, C.byref(m), C.byref(st), 0))
        q = self._inc_stats_raw()
        n = m.value
        if device is not None:
            import torch
            out = torch.empty((max(n, 1), 4), dtype=torch.int32, device=device)
        else:
            out = np.empty(max(n, 1), POINT)
        po, mem, _k = _ptr(out)
        L.check(self._lib.o3dr_finalize_incremental(self._h, po, max(n, 1), C.byref(m), C.byref(st), mem))
        w = self._inc_stats_raw()
        # the size query folded, the second call only wrote: the statistics of the pair
        both = dict(w, points_folded=q["points_folded"] + w["points_folded"], from_empty=q["from_empty"] | w["from_empty"],
                    fallback=q["fallback"] | w["fallback"])
        self._inc_last = (w, both)
        return (out[: m.value], st.value) if return_status else out[: m.value]

    def _inc_stats_raw(self):
        out = (C.c_int64 * 8)()
        L.check(self._lib.o3dr_finalize_incremental_stats(self._h, out))
        keys = ("points_folded", "from_empty", "fallback", "cells", "groups", "state_bytes")
        return dict(zip(keys, (int(v) for v in out)))

    def finalizeIncrementalStats(self):
        """what the last finalizeIncremental did (include/o3dr.h; both of its calls), or the last o3dr_finalize_incremental
        made through the C ABI directly"""
        raw = self._inc_stats_raw()
        last = getattr(self, "_inc_last", None)
        return dict(last[1]) if last is not None and last[0] == raw else raw

    # -- measurement hooks --------------------------------------------------------------------------
    def profileEnable(self, kernel_id=-1, enable=True):
        L.check(self._lib.o3dr_profile_enable(self._h, int(kernel_id), int(bool(enable))))

    def profileReset(self):
        L.check(self._lib.o3dr_profile_reset(self._h))

    def profileStats(self):
        """(sort record-passes, voxel-grid points in, voxel-grid points out) since profileReset()"""
        return self.profileStats4()[:3]

    def profileStats4(self):
        """profileStats() + the number of frames that took the pixel-window path"""
        return self.profileStatsAll()[:4]

    def profileStatsAll(self):
        """all eight counters of o3dr_profile_stats (include/o3dr.h)"""
        out = (C.c_int64 * 8)()
        L.check(self._lib.o3dr_profile_stats(self._h, out))
        return tuple(int(v) for v in out)

    def profileRead(self, kernel_id):
        ms = C.c_double(0)
        n = C.c_int64(0)
        L.check(self._lib.o3dr_profile_read(self._h, int(kernel_id), C.byref(ms), C.byref(n)))
        return ms.value, n.value


class _DevMem:
    """minimal __cuda_array_interface__ holder so torch can alias library-owned HBM"""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n, 4), "typestr": "<i4", "data": (ptr, False), "version": 2}


def _device_tensor(ptr, n, device_index):
    import torch
    if n == 0 or not ptr:
        return torch.empty((0, 4), dtype=torch.int32, device=torch.device("cuda", device_index))
    return torch.as_tensor(_DevMem(ptr, n), device=torch.device("cuda", device_index))


def points_from_torch(t):
    """[N,4] int32 CUDA/CPU tensor -> numpy POINT array (host copy)."""
    return t.detach().cpu().numpy().view(POINT).reshape(-1)
