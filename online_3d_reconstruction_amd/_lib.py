"""ctypes loader of libo3dr.so.  Fails loudly when the HIP library is missing: no fallback."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = os.path.join(_HERE, "lib", "libo3dr.so")

POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("rgba", "<u4")])

OK = 0
ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_CAPACITY, ERR_NOT_CONFIGURED, ERR_ALLOC, ERR_INTERNAL, ERR_PEER = -1, -2, -3, -4, -5, -6, -7, -8
MEM_HOST, MEM_DEVICE = 0, 1
STATUS_VOXEL_OVERFLOW = 1
STATUS_LABEL_RANGE = 2
STATUS_INTERNAL = 0x80000000
K_COUNT, K_REPROJECT, K_KEYGEN, K_SORT_HIST, K_SORT_SCATTER, K_SEGMENT, K_CENTROID, K_OTHER, K_CENTROID_RUNS = range(9)
K_PLANE_DISP_SUMS, K_PLANE_DISP_FIT, K_PLANE_DISP_EVAL = 9, 10, 11
K_ORB_PYRAMID, K_ORB_FAST, K_ORB_CANDIDATES, K_ORB_SELECT, K_ORB_DESCRIBE = 12, 13, 14, 15, 16
K_MATCH, K_POSE_CHAIN, K_RANSAC = 17, 18, 19
K_GRAPH_MOMENTS, K_GRAPH_SOLVE = 20, 21
K_STEREO_CENSUS, K_STEREO_PATHS, K_STEREO_WINNER = 22, 23, 24
K_DISP_MEDIAN, K_DISP_LABEL, K_DISP_SPECKLE = 25, 26, 27
K_RECTIFY_MAPS, K_RECTIFY_REMAP = 28, 29
K_SEG_ASSIGN, K_SEG_LABEL = 30, 31
K_MULTIVIEW = 32
K_GROUND_WINNER, K_GROUND_ITER, K_GROUND_FILL, K_GROUND_POINTS = 33, 34, 35, 36
K_CLUSTER_LINK, K_CLUSTER_NUMBER, K_CLUSTER_RECORDS = 37, 38, 39
K_INTERP_PULL, K_INTERP_PUSH, K_RASTER_SAMPLE = 40, 41, 42
KERNEL_NAMES = ["reproject_count", "reproject_emit", "voxel_keys", "radix_hist", "radix_scatter", "run_segments",
                "centroid", "other", "centroid_runs", "plane_disp_sums", "plane_disp_fit", "plane_disp_eval",
                "orb_pyramid", "orb_fast", "orb_candidates", "orb_select", "orb_describe", "match", "pose_chain", "ransac",
                "graph_moments", "graph_solve", "stereo_census", "stereo_paths", "stereo_winner", "disp_median", "disp_label",
                "disp_speckle", "rectify_maps", "rectify_remap", "seg_assign", "seg_label", "multiview", "ground_winner", "ground_iter",
                "ground_fill", "ground_points", "cluster_link", "cluster_number", "cluster_records"]
# the ids of include/o3dr_dem.h's operators, from K_INTERP_PULL on: a list of their own, KERNEL_NAMES stays the 40 ids that
# the benchmark and the clustering test enumerate
DEM_KERNEL_NAMES = ["interp_pull", "interp_push", "raster_sample"]


class O3drError(RuntimeError):
    def __init__(self, code, text):
        super().__init__(f"libo3dr error {code}: {text}")
        self.code = code


class ParamsStruct(C.Structure):
    _fields_ = [("min_disparity", C.c_double), ("voxel_size", C.c_double), ("bounding_box", C.c_int32),
                ("cutout_ratio", C.c_int32), ("jump_pixels", C.c_int32), ("min_points_per_voxel", C.c_uint32),
                ("dont_downsample", C.c_int32), ("sor_enable", C.c_int32), ("blur_kernel", C.c_int32), ("disparity_f64", C.c_int32)]


class IcpParamsStruct(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("max_correspondence_distance", C.c_double), ("transformation_epsilon", C.c_double)]


class IcpResultStruct(C.Structure):
    _fields_ = [("T", C.c_double * 16), ("fitness", C.c_double), ("n_correspondences", C.c_int64), ("iterations", C.c_int32),
                ("reason", C.c_int32)]


ICP_MAX_ITERATIONS, ICP_UNCHANGED, ICP_SMALL_STEP, ICP_TOO_FEW, ICP_DEGENERATE = range(5)
ICP_REASONS = ["MAX_ITERATIONS", "UNCHANGED", "SMALL_STEP", "TOO_FEW", "DEGENERATE"]


class MlsParamsStruct(C.Structure):
    _fields_ = [("search_radius", C.c_double), ("polynomial_order", C.c_int32), ("sqr_gauss_param", C.c_double)]


class MlsResultStruct(C.Structure):
    _fields_ = [("n_poly", C.c_int64), ("n_plane", C.c_int64), ("n_none", C.c_int64), ("max_neighbors", C.c_int32)]


MLS_NONE, MLS_PLANE, MLS_POLY = range(3)


class PlaneParamsStruct(C.Structure):
    _fields_ = [("distance_threshold", C.c_double), ("max_iterations", C.c_int32), ("tile_size", C.c_double),
                ("seed", C.c_uint64), ("optimize", C.c_int32)]


# o3dr_plane_tile (64 bytes), as a numpy record: Context.segmentPlane returns the tile records in this layout
PLANE_TILE = np.dtype([("coeff", "<f4", (4,)), ("ix", "<i4"), ("iy", "<i4"), ("n_points", "<u4"), ("n_inliers", "<u4"),
                       ("ransac_inliers", "<u4"), ("hypothesis", "<i4"), ("sample", "<u4", (3,)), ("refined", "<i4"),
                       ("status", "<i4"), ("reserved", "<u4")])
assert PLANE_TILE.itemsize == 64
PLANE_OK, PLANE_TOO_FEW, PLANE_DEGENERATE = range(3)
PLANE_MAX_ITERATIONS = 1 << 20


class MeshParamsStruct(C.Structure):
    _fields_ = [("cell_size", C.c_double), ("max_edge_length", C.c_double)]


class MeshResultStruct(C.Structure):
    _fields_ = [("n_vertices", C.c_int64), ("n_shadowed", C.c_int64), ("n_triangles", C.c_int64), ("n_quads_full", C.c_int64),
                ("n_rejected_orientation", C.c_int64), ("n_rejected_length", C.c_int64)]


class RasterParamsStruct(C.Structure):
    _fields_ = [("cell_size", C.c_double), ("select", C.c_int32), ("fill_radius", C.c_int32), ("cx0", C.c_int32), ("cy0", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("use_light", C.c_int32), ("reserved", C.c_int32),
                ("light", C.c_double * 3)]


class RasterOutputsStruct(C.Structure):
    _fields_ = [("height_map", C.c_void_p), ("color", C.c_void_p), ("shade", C.c_void_p), ("source", C.c_void_p),
                ("distance2", C.c_void_p)]


class RasterResultStruct(C.Structure):
    _fields_ = [("cx0", C.c_int32), ("cy0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("n_inside", C.c_int64),
                ("n_outside", C.c_int64), ("n_occupied", C.c_int64), ("n_shadowed", C.c_int64), ("n_filled", C.c_int64),
                ("n_empty", C.c_int64), ("z_min", C.c_float), ("z_max", C.c_float)]


RASTER_SELECT = {"first": 0, "top": 1, "bottom": 2}
RASTER_MAX_FILL_RADIUS, RASTER_MAX_CELLS = 32, 1 << 28


# include/o3dr_terrain.h
class GroundParamsStruct(C.Structure):
    _fields_ = [("cell_size", C.c_double), ("cx0", C.c_int32), ("cy0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("max_window_radius", C.c_int32), ("window_base", C.c_int32), ("exponential", C.c_int32), ("reserved0", C.c_int32),
                ("slope", C.c_double), ("initial_distance", C.c_double), ("max_distance", C.c_double), ("fill_radius", C.c_int32),
                ("reserved1", C.c_int32)]


class GroundOutputsStruct(C.Structure):
    _fields_ = [("ground", C.c_void_p), ("height_above_ground", C.c_void_p), ("dtm", C.c_void_p), ("cell_state", C.c_void_p)]


class GroundResultStruct(C.Structure):
    _fields_ = [("cx0", C.c_int32), ("cy0", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("n_inside", C.c_int64),
                ("n_outside", C.c_int64), ("n_occupied", C.c_int64), ("n_ground_cells", C.c_int64), ("n_ground_points", C.c_int64),
                ("n_dtm_filled", C.c_int64), ("n_dtm_empty", C.c_int64), ("n_iterations", C.c_int32), ("reserved", C.c_int32),
                ("n_removed", C.c_int64 * 16)]


O3DR_GROUND_MAX_WINDOW_RADIUS = 128
O3DR_GROUND_MAX_ITERATIONS = 16


# include/o3dr_dem.h
class InterpolateParamsStruct(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("smooth", C.c_int32), ("max_level", C.c_int32)]


class InterpolateOutputsStruct(C.Structure):
    _fields_ = [("filled", C.c_void_p), ("level", C.c_void_p)]


class InterpolateResultStruct(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("n_levels", C.c_int32), ("reserved", C.c_int32),
                ("n_data", C.c_int64), ("n_filled", C.c_int64), ("n_empty", C.c_int64), ("n_by_level", C.c_int64 * 32)]


INTERPOLATE_MAX_SMOOTH, INTERPOLATE_MAX_LEVELS = 8, 32


# include/o3dr_contour.h
class ContourParamsStruct(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("interval", C.c_double), ("base", C.c_double),
                ("cell_size", C.c_double), ("cx0", C.c_int32), ("cy0", C.c_int32)]


class ContourOutputsStruct(C.Structure):
    _fields_ = [("segments", C.c_void_p), ("seg_capacity", C.c_int64), ("lines", C.c_void_p), ("line_capacity", C.c_int64),
                ("vertices", C.c_void_p), ("vertex_capacity", C.c_int64)]


class ContourResultStruct(C.Structure):
    _fields_ = [("n_quads", C.c_int64), ("n_quads_crossed", C.c_int64), ("n_segments", C.c_int64), ("n_lines", C.c_int64),
                ("n_closed", C.c_int64), ("n_vertices", C.c_int64), ("n_longest", C.c_int64), ("k_lo", C.c_int32),
                ("k_hi", C.c_int32)]


# o3dr_contour_segment (48 bytes) and o3dr_contour_line (32 bytes), as numpy records
CONTOUR_SEGMENT = np.dtype([("x0", "<f8"), ("y0", "<f8"), ("x1", "<f8"), ("y1", "<f8"), ("k", "<i4"), ("line", "<i4"),
                            ("rank", "<i4"), ("next", "<i4")])
CONTOUR_LINE = np.dtype([("head", "<i4"), ("n_segments", "<i4"), ("k", "<i4"), ("closed", "<i4"), ("begin", "<i8"),
                         ("level", "<f8")])
assert CONTOUR_SEGMENT.itemsize == 48 and CONTOUR_LINE.itemsize == 32 and C.sizeof(ContourResultStruct) == 64
CONTOUR_MAX_SEGMENTS = 1 << 28


# include/o3dr_objects.h
class ClusterParamsStruct(C.Structure):
    _fields_ = [("tolerance", C.c_double), ("min_size", C.c_int32), ("max_size", C.c_int32)]


class ClusterOutputsStruct(C.Structure):
    _fields_ = [("label", C.c_void_p), ("raw", C.c_void_p), ("size", C.c_void_p), ("indices", C.c_void_p)]


class ClusterResultStruct(C.Structure):
    _fields_ = [("n_components", C.c_int64), ("n_clusters", C.c_int64), ("n_too_small", C.c_int64), ("n_too_large", C.c_int64),
                ("n_clustered_points", C.c_int64), ("n_rejected_points", C.c_int64), ("largest", C.c_int64), ("n_pairs", C.c_int64)]


# o3dr_cluster: one record per cluster, 64 bytes
CLUSTER = np.dtype([("first", np.int32), ("size", np.int32), ("begin", np.int32), ("reserved", np.int32),
                    ("lo", np.float32, (3,)), ("hi", np.float32, (3,)), ("centroid", np.float64, (3,))])
assert CLUSTER.itemsize == 64


class PlaneDispParamsStruct(C.Structure):
    _fields_ = [("min_disparity", C.c_double), ("min_pixels", C.c_int32), ("max_mse", C.c_double), ("fill", C.c_int32)]


# o3dr_plane_disp_segment (64 bytes), as a numpy record: Context.planeFitDisparity returns the segment records in this layout
PLANE_DISP_SEGMENT = np.dtype([("a", "<f8"), ("b", "<f8"), ("c0", "<f8"), ("mx", "<f8"), ("my", "<f8"), ("mse", "<f8"),
                               ("n_pixels", "<u4"), ("n", "<u4"), ("status", "<i4"), ("reserved", "<i4")])
assert PLANE_DISP_SEGMENT.itemsize == 64
PLANE_DISP_NONE, PLANE_DISP_MEAN, PLANE_DISP_PLANE = range(3)
PLANE_DISP_TOL = 2.0 ** -20
PLANE_DISP_MAX_SIDE, PLANE_DISP_MAX_LABELS = 8192, 65536


class OrbParamsStruct(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32), ("fast_threshold", C.c_int32),
                ("edge", C.c_int32), ("channels", C.c_int32)]


# o3dr_orb_keypoint (32 bytes), as a numpy record: Context.findFeatures returns the keypoints in this layout
ORB_KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("angle_deg", "<f4"), ("size", "<f4"), ("response", "<i8"), ("xl", "<i2"),
                         ("yl", "<i2"), ("level", "u1"), ("angle_bin", "u1"), ("reserved", "<u2")])
assert ORB_KEYPOINT.itemsize == 32
ORB_MAX_SIDE, ORB_MAX_LEVELS = 8192, 8


class StereoParamsStruct(C.Structure):
    _fields_ = [("n_disparities", C.c_int32), ("min_disparity", C.c_int32), ("p1", C.c_int32), ("p2", C.c_int32),
                ("n_paths", C.c_int32), ("uniqueness", C.c_int32), ("lr_max_diff", C.c_int32), ("channels", C.c_int32),
                ("group_frames", C.c_int32)]


STEREO_MAX_SIDE = 8192


class DisparityFilterParamsStruct(C.Structure):
    _fields_ = [("elem_bytes", C.c_int32), ("median_size", C.c_int32), ("max_speckle_size", C.c_int32), ("max_diff", C.c_int32),
                ("group_frames", C.c_int32)]


class DisparityFilterInfoStruct(C.Structure):
    _fields_ = [("n_valid", C.c_int64), ("n_components", C.c_int64), ("n_speckles", C.c_int64), ("n_removed", C.c_int64),
                ("largest", C.c_int64)]


DISPARITY_FILTER_MAX_SIDE = 8192


class MultiviewParamsStruct(C.Structure):
    _fields_ = [("elem_bytes", C.c_int32), ("tolerance", C.c_double), ("min_support", C.c_int32), ("max_violations", C.c_int32)]


class MultiviewInfoStruct(C.Structure):
    _fields_ = [("n_valid", C.c_int64), ("n_kept", C.c_int64), ("n_no_support", C.c_int64), ("n_violated", C.c_int64),
                ("n_outside", C.c_int64), ("n_hole", C.c_int64), ("n_support", C.c_int64), ("n_violation", C.c_int64),
                ("n_occluded", C.c_int64)]


class MultiviewFuseInfoStruct(C.Structure):
    _fields_ = [("filter", MultiviewInfoStruct), ("n_votes", C.c_int64), ("n_votes_dropped", C.c_int64), ("n_fused", C.c_int64)]


MULTIVIEW_MAX_SIDE, MULTIVIEW_MAX_NEIGHBORS = 8192, 16


class SegmentParamsStruct(C.Structure):
    _fields_ = [("channels", C.c_int32), ("step", C.c_int32), ("compactness", C.c_int32), ("iterations", C.c_int32),
                ("min_size", C.c_int32), ("group_frames", C.c_int32)]


class SegmentInfoStruct(C.Structure):
    _fields_ = [("n_centres", C.c_int64), ("n_components", C.c_int64), ("n_merged", C.c_int64), ("n_labels", C.c_int64),
                ("largest", C.c_int64), ("smallest", C.c_int64)]


SEGMENT_MAX_SIDE = 8192


class RectifyCameraStruct(C.Structure):
    _fields_ = [("K", C.c_double * 9), ("D", C.c_double * 8), ("R", C.c_double * 9), ("P", C.c_double * 12)]


RECTIFY_MAX_SIDE = 8192
RECTIFY_OUTSIDE = -1048576


class MatchParamsStruct(C.Structure):
    _fields_ = [("ratio", C.c_float), ("max_distance", C.c_int32)]


class RigidResultStruct(C.Structure):
    _fields_ = [("T", C.c_double * 16), ("rms", C.c_double), ("n_used", C.c_int64), ("status", C.c_int32), ("reserved", C.c_int32)]


# o3dr_knn2 (16 bytes) and o3dr_rigid_result (152 bytes), as numpy records
KNN2 = np.dtype([("train_idx", "<u4", (2,)), ("distance", "<u4", (2,))])
assert KNN2.itemsize == 16
RIGID_RESULT = np.dtype([("T", "<f8", (16,)), ("rms", "<f8"), ("n_used", "<i8"), ("status", "<i4"), ("reserved", "<i4")])
assert RIGID_RESULT.itemsize == C.sizeof(RigidResultStruct) == 152
MATCH_NONE = 0xFFFFFFFF
RIGID_OK, RIGID_TOO_FEW, RIGID_DEGENERATE = range(3)


class ChainParamsStruct(C.Structure):
    _fields_ = [("dist_nearby", C.c_double), ("max_rms", C.c_double), ("range_width", C.c_int32), ("min_matches", C.c_int32),
                ("ratio", C.c_float), ("max_distance", C.c_int32)]


# o3dr_chain_frame (128 bytes), as a numpy record: Context.poseChain returns one per frame
CHAIN_FRAME = np.dtype([("status", "<i4"), ("n_pairs", "<i4"), ("n_pairs_accepted", "<i4"), ("n_good", "<i4"), ("n_used", "<i4"),
                        ("reserved", "<i4"), ("rms", "<f8"), ("T", "<f8", (12,))])
assert CHAIN_FRAME.itemsize == 128
CHAIN_ANCHOR, CHAIN_MATCHED, CHAIN_TOO_FEW, CHAIN_DEGENERATE, CHAIN_RMS = range(5)
CHAIN_STATUS_NAMES = ["ANCHOR", "MATCHED", "TOO_FEW", "DEGENERATE", "RMS"]
CHAIN_MAX_RANGE = 32


class RansacParamsStruct(C.Structure):
    _fields_ = [("threshold", C.c_double), ("seed", C.c_uint64), ("iterations", C.c_int32), ("reserved", C.c_int32)]


# o3dr_ransac_result (128 bytes), as a numpy record: one per segment (Context.ransacRigid) or pair (Context.poseChain)
RANSAC_RESULT = np.dtype([("T", "<f8", (12,)), ("n_candidates", "<i4"), ("n_inliers", "<i4"), ("best_hypothesis", "<i4"),
                          ("sample", "<i4", (3,)), ("status", "<i4"), ("reserved", "<i4")])
assert RANSAC_RESULT.itemsize == 128
RANSAC_OK, RANSAC_TOO_FEW, RANSAC_NO_MODEL = range(3)
RANSAC_MAX_ITERATIONS = 65536
RANSAC_STAGE = 1024  # candidates of a segment the kernel stages in LDS (kRansacStage); larger segments read the rest through a list


class RefineParamsStruct(C.Structure):
    _fields_ = [("prior_weight", C.c_double), ("gn_iterations", C.c_int32), ("cg_iterations", C.c_int32),
                ("min_pair_matches", C.c_int32), ("ratio", C.c_float), ("max_distance", C.c_int32), ("reserved", C.c_int32)]


class RefineResultStruct(C.Structure):
    _fields_ = [("energy_before", C.c_double), ("energy_after", C.c_double), ("grad_before", C.c_double), ("grad_after", C.c_double),
                ("last_step", C.c_double), ("n_used", C.c_int64), ("n_free", C.c_int32), ("n_gauge", C.c_int32),
                ("n_floating", C.c_int32), ("n_rejected", C.c_int32), ("n_edges", C.c_int32), ("flags", C.c_int32)]


# o3dr_refine_frame (104 bytes) and o3dr_refine_edge (32 bytes), as numpy records: Context.refinePoses returns one per frame / pair
REFINE_FRAME = np.dtype([("role", "<i4"), ("degree", "<i4"), ("T", "<f8", (12,))])
REFINE_EDGE = np.dtype([("n_good", "<i4"), ("n_used", "<i4"), ("edge", "<i4"), ("reserved", "<i4"), ("energy_before", "<f8"),
                        ("energy_after", "<f8")])
assert REFINE_FRAME.itemsize == 104 and REFINE_EDGE.itemsize == 32 and C.sizeof(RefineResultStruct) == 72
REFINE_FIXED, REFINE_FREE, REFINE_FLOATING, REFINE_REJECTED = range(4)
REFINE_ROLE_NAMES = ["FIXED", "FREE", "FLOATING", "REJECTED"]
REFINE_FLAG_CG_STOPPED, REFINE_FLAG_SINGULAR = 1, 2


def lib_path():
    return _LIB


# every symbol include/o3dr.h declares: (name, restype, argtypes)
_vp, _i64, _i32, _u32, _f = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_float
_pi64, _pu32 = C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
SYMBOLS = [
    ("o3dr_version", C.c_int, []),
    ("o3dr_last_error", C.c_char_p, []),
    ("o3dr_default_params", None, [C.POINTER(ParamsStruct)]),
    ("o3dr_ctx_create", C.c_int, [C.c_int, C.POINTER(_vp)]),
    ("o3dr_ctx_destroy", C.c_int, [_vp]),
    ("o3dr_ctx_set_stream", C.c_int, [_vp, _vp]),
    ("o3dr_ctx_synchronize", C.c_int, [_vp]),
    ("o3dr_set_camera", C.c_int, [_vp, _vp]),
    ("o3dr_set_params", C.c_int, [_vp, C.POINTER(ParamsStruct)]),
    ("o3dr_get_params", C.c_int, [_vp, C.POINTER(ParamsStruct)]),
    ("o3dr_create_single_img_pt_cloud", C.c_int, [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _i64, _pi64, _i32]),
    ("o3dr_max_points", _i64, [_vp, _i32, _i32]),
    ("o3dr_transform_pt_cloud", C.c_int, [_vp, _vp, _i64, _vp, _vp, _i32]),
    ("o3dr_reproject_transform", C.c_int, [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _i64, _pi64, _i32]),
    ("o3dr_voxel_grid", C.c_int, [_vp, _vp, _i64, _vp, _u32, _f, _vp, _i64, _pi64, _pu32, _i32]),
    ("o3dr_statistical_outlier_removal", C.c_int, [_vp, _vp, _i64, _vp, _i64, _pi64, _i32]),
    ("o3dr_bilateral_filter_u8", C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, C.c_double, C.c_double, _vp, _i64, _i32]),
    ("o3dr_disparity_variance", C.c_int, [_vp, _vp, _i64, _i64, _i32, _i32, _i32, _vp, _i32]),
    ("o3dr_downsample_pt_cloud", C.c_int, [_vp, _vp, _i64, _i32, _vp, _i64, _pi64, _pu32, _i32]),
    ("o3dr_create_and_transform_pt_cloud", C.c_int, [_vp, _vp, _i64, _vp, _i64, _i32, _i32, _vp, _vp, _i32, _vp, _i64, _pi64, _pu32, _i32]),
    ("o3dr_accumulate_frames", C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i32, _i32]),
    ("o3dr_accumulate_frames_kp", C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _i32]),
    ("o3dr_cloud_big_reserve", C.c_int, [_vp, _i64]),
    ("o3dr_cloud_big_reset", C.c_int, [_vp]),
    ("o3dr_cloud_big_size", C.c_int, [_vp, _pi64, _pu32]),
    ("o3dr_cloud_big_read", C.c_int, [_vp, _vp, _i64, _pi64, _i32]),
    ("o3dr_cloud_big_append", C.c_int, [_vp, _vp, _i64, _i32]),
    ("o3dr_cloud_big_transform", C.c_int, [_vp, _vp]),
    ("o3dr_finalize", C.c_int, [_vp, _vp, _i64, _pi64, _pu32, _i32]),
    ("o3dr_finalize_incremental", C.c_int, [_vp, _vp, _i64, _pi64, _pu32, _i32]),
    ("o3dr_finalize_incremental_stats", C.c_int, [_vp, _pi64]),
    ("o3dr_cloud_big_bbox", C.c_int, [_vp, _vp, _vp, _pi64]),
    ("o3dr_cloud_big_partition", C.c_int, [_vp, _vp, _vp, _i32, _pi64, _pu32]),
    ("o3dr_finalize_global", C.c_int, [_vp, _vp, _vp, _vp, _i64, _pi64, _pu32, _i32]),
    ("o3dr_cloud_big_view", C.c_int, [_vp, C.POINTER(_vp), _pi64]),
    ("o3dr_cloud_big_recv_buffer", C.c_int, [_vp, _i64, C.POINTER(_vp)]),
    ("o3dr_cloud_big_adopt", C.c_int, [_vp, _i64]),
    ("o3dr_cloud_big_header_dev", C.c_int, [_vp, _vp]),
    ("o3dr_cloud_big_assume_size", C.c_int, [_vp, _i64]),
    ("o3dr_cloud_big_partition_dev", C.c_int, [_vp, _vp, _i32, _i32, _vp]),
    ("o3dr_cloud_big_slice_counts_dev", C.c_int, [_vp, _vp, _i32, _i32, _vp]),
    ("o3dr_cloud_big_place_slices", C.c_int, [_vp, _i32, _i32, _vp, _i64, _i64, _pi64]),
    ("o3dr_cloud_big_set_size", C.c_int, [_vp, _i64]),
    ("o3dr_cloud_big_raw_view", C.c_int, [_vp, C.POINTER(_vp), _pi64]),
    ("o3dr_merge_partitioned", C.c_int, [_vp, _vp, _i32, _vp, _i64, _pi64, _pi64, C.POINTER(C.c_uint32), _i32]),
    ("o3dr_merge_partitioned_stats", C.c_int, [_vp, _pi64]),
    ("o3dr_cloud_big_capacity", C.c_int, [_vp, _pi64, _pi64]),
    ("o3dr_comm_init_all", C.c_int, [_i32, _vp, _vp]),
    ("o3dr_comm_destroy", C.c_int, [_vp]),
    ("o3dr_host_register", C.c_int, [_vp, _i64]),
    ("o3dr_host_unregister", C.c_int, [_vp]),
    ("o3dr_icp_default_params", None, [C.POINTER(IcpParamsStruct)]),
    ("o3dr_nearest_neighbors", C.c_int, [_vp, _vp, _i64, _vp, _i64, C.c_double, _vp, _vp, _i32]),
    ("o3dr_icp_align", C.c_int, [_vp, _vp, _i64, _vp, _i64, _vp, C.POINTER(IcpParamsStruct), C.POINTER(IcpResultStruct), _i32]),
    ("o3dr_match_default_params", None, [C.POINTER(MatchParamsStruct)]),
    ("o3dr_match_knn2_hamming", C.c_int, [_vp, _vp, _vp, _i32, _vp, _i64, C.POINTER(MatchParamsStruct), _vp, _vp, _i64, _pi64, _i32]),
    ("o3dr_keypoints_3d", C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i64, _pi64, _i32]),
    ("o3dr_estimate_rigid_transform", C.c_int, [_vp, _vp, _vp, _i64, _vp, _i32, _vp, _vp, _i32]),
    ("o3dr_mls_default_params", None, [C.POINTER(MlsParamsStruct)]),
    ("o3dr_mls_smooth", C.c_int, [_vp, _vp, _i64, C.POINTER(MlsParamsStruct), _vp, _vp, _vp, _vp, C.POINTER(MlsResultStruct), _i32]),
    ("o3dr_plane_default_params", None, [C.POINTER(PlaneParamsStruct)]),
    ("o3dr_segment_plane", C.c_int, [_vp, _vp, _i64, C.POINTER(PlaneParamsStruct), _vp, _vp, _vp, _vp, _i64, _pi64, _i32]),
    ("o3dr_mesh_default_params", None, [C.POINTER(MeshParamsStruct)]),
    ("o3dr_mesh_surface", C.c_int, [_vp, _vp, _i64, C.POINTER(MeshParamsStruct), _vp, _i64, _pi64, _vp,
                                    C.POINTER(MeshResultStruct), _i32]),
    ("o3dr_raster_default_params", None, [C.POINTER(RasterParamsStruct)]),
    ("o3dr_raster_extent", C.c_int, [_vp, _vp, _i64, C.c_double, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), _i32]),
    ("o3dr_rasterize_map", C.c_int, [_vp, _vp, _i64, C.POINTER(RasterParamsStruct), C.POINTER(RasterOutputsStruct),
                                     C.POINTER(RasterResultStruct), _i32]),
    ("o3dr_ground_default_params", None, [C.POINTER(GroundParamsStruct)]),
    ("o3dr_ground_schedule", C.c_int, [C.POINTER(GroundParamsStruct), _vp, _vp, C.POINTER(_i32)]),
    ("o3dr_ground_filter", C.c_int, [_vp, _vp, _i64, C.POINTER(GroundParamsStruct), C.POINTER(GroundOutputsStruct),
                                     C.POINTER(GroundResultStruct), _i32]),
    ("o3dr_interpolate_default_params", None, [C.POINTER(InterpolateParamsStruct)]),
    ("o3dr_raster_interpolate", C.c_int, [_vp, _vp, C.POINTER(InterpolateParamsStruct), C.POINTER(InterpolateOutputsStruct),
                                          C.POINTER(InterpolateResultStruct), _i32]),
    ("o3dr_raster_sample", C.c_int, [_vp, _vp, _i64, C.c_double, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _pi64, _i32]),
    ("o3dr_contour_default_params", None, [C.POINTER(ContourParamsStruct)]),
    ("o3dr_raster_contours_count", C.c_int, [_vp, _vp, C.POINTER(ContourParamsStruct), _pi64, _i32]),
    ("o3dr_raster_contours", C.c_int, [_vp, _vp, C.POINTER(ContourParamsStruct), C.POINTER(ContourOutputsStruct),
                                       C.POINTER(ContourResultStruct), _i32]),
    ("o3dr_cluster_default_params", None, [C.POINTER(ClusterParamsStruct)]),
    ("o3dr_cluster_euclidean", C.c_int, [_vp, _vp, _i64, C.POINTER(ClusterParamsStruct), C.POINTER(ClusterOutputsStruct), _vp, _i64,
                                         C.POINTER(_i64), C.POINTER(ClusterResultStruct), _i32]),
    ("o3dr_plane_disp_default_params", None, [C.POINTER(PlaneDispParamsStruct)]),
    ("o3dr_plane_fit_disparity", C.c_int, [_vp, _vp, _i64, _i64, _vp, _i32, _i64, _i64, _i32, _i32, _i32, _i32,
                                           C.POINTER(PlaneDispParamsStruct), _vp, _vp, _pu32, _i32]),
    ("o3dr_orb_default_params", None, [C.POINTER(OrbParamsStruct)]),
    ("o3dr_orb_pattern", C.c_int, [_vp]),
    ("o3dr_orb_level_sizes", C.c_int, [_i32, _i32, C.POINTER(OrbParamsStruct), _vp, _vp]),
    ("o3dr_orb_detect", C.c_int, [_vp, _vp, _i64, _i64, _i32, _i32, _i32, C.POINTER(OrbParamsStruct), _vp, _vp, _vp, _vp, _vp, _i64,
                                  _pi64, _i32]),
    ("o3dr_stereo_default_params", None, [C.POINTER(StereoParamsStruct)]),
    ("o3dr_stereo_disparity", C.c_int, [_vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, C.POINTER(StereoParamsStruct), _vp, _vp, _vp, _vp,
                                        _i32]),
    ("o3dr_disparity_filter_default_params", None, [C.POINTER(DisparityFilterParamsStruct)]),
    ("o3dr_disparity_filter", C.c_int, [_vp, _vp, _i64, _i64, _i32, _i32, _i32, C.POINTER(DisparityFilterParamsStruct), _vp, _vp, _vp,
                                        _vp, _i32]),
    ("o3dr_multiview_default_params", None, [C.POINTER(MultiviewParamsStruct)]),
    ("o3dr_nearby_frames", C.c_int, [_vp, _i32, _i32, C.c_double, _vp]),
    ("o3dr_multiview_homographies", C.c_int, [_vp, _vp, _i32, _vp, _i32, _vp]),
    ("o3dr_multiview_filter", C.c_int, [_vp, _vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _i32, C.POINTER(MultiviewParamsStruct), _vp, _vp,
                                        _vp, _vp, _i32]),
    ("o3dr_multiview_fuse", C.c_int, [_vp, _vp, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _i32, C.POINTER(MultiviewParamsStruct), _vp, _vp,
                                      _vp, _vp, _vp, _i32]),
    ("o3dr_segment_default_params", None, [C.POINTER(SegmentParamsStruct)]),
    ("o3dr_segment_image", C.c_int, [_vp, _vp, _i64, _i64, _i32, _i32, _i32, C.POINTER(SegmentParamsStruct), _vp, _vp, _vp, _vp, _i32]),
    ("o3dr_rectify_maps", C.c_int, [_vp, C.POINTER(RectifyCameraStruct), _i32, _i32, _vp, _i32]),
    ("o3dr_rectify_remap", C.c_int, [_vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32]),
    ("o3dr_chain_default_params", None, [C.POINTER(ChainParamsStruct)]),
    ("o3dr_pose_chain", C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, C.POINTER(ChainParamsStruct), _vp, _vp, _vp, _i64,
                                  _pi64, _i32]),
    ("o3dr_ransac_default_params", None, [C.POINTER(RansacParamsStruct)]),
    ("o3dr_ransac_rigid", C.c_int, [_vp, _vp, _vp, _i64, _vp, _i32, _vp, _vp, C.POINTER(RansacParamsStruct), _vp, _vp, _i32]),
    ("o3dr_pose_chain_robust", C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, C.POINTER(ChainParamsStruct), _vp, _vp, _vp,
                                         _i64, _pi64, _i32, C.POINTER(RansacParamsStruct), _vp]),
    ("o3dr_refine_default_params", None, [C.POINTER(RefineParamsStruct)]),
    ("o3dr_pose_graph_refine", C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i64, C.POINTER(RefineParamsStruct),
                                         C.POINTER(RansacParamsStruct), _vp, _vp, _vp, C.POINTER(RefineResultStruct), _i32]),
    ("o3dr_profile_enable", C.c_int, [_vp, _i32, _i32]),
    ("o3dr_profile_read", C.c_int, [_vp, _i32, C.POINTER(C.c_double), _pi64]),
    ("o3dr_profile_reset", C.c_int, [_vp]),
    ("o3dr_profile_stats", C.c_int, [_vp, _pi64]),
    ("o3dr_test_corrupt_next_gather", C.c_int, [_vp]),
    ("o3dr_test_sor_distances", C.c_int, [_vp, _vp, _i64]),
    ("o3dr_test_local_comm_create", C.c_int, [_i32, C.POINTER(_vp)]),
    ("o3dr_test_local_comm_destroy", C.c_int, [_vp]),
    ("o3dr_test_merge_partitioned_local", C.c_int, [_vp, _vp, _i32, _i32, _vp, _i64, _pi64, _pi64, C.POINTER(C.c_uint32), _i32]),
    ("o3dr_test_fail_at", C.c_int, [_vp, _i32]),
    ("o3dr_test_plane_hypotheses", C.c_int, [_vp, _vp, _vp, _i64, _pi64]),
    ("o3dr_test_orb_scratch_limit", C.c_int, [_vp, _i64]),
    ("o3dr_test_fill_scratch", C.c_int, [_vp, _i32, _pi64]),
    ("o3dr_device_info", C.c_int, [_vp, C.c_char_p, _i32, C.POINTER(_i32), _pi64]),
]

_lib = None


def load_library():
    """dlopen libo3dr.so and bind every exported symbol; raises if the library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB):
            raise O3drError(ERR_NO_DEVICE, f"{_LIB} is not built: run `python __graft_entry__.py` or `make` "
                                           "(there is no CPU fallback)")
        # PyTorch-ROCm wheels bundle their own libamdhip64.so.7.  A process must hold ONE HIP/HSA
        # runtime, so when torch is installed it is imported first: libo3dr's DT_NEEDED
        # libamdhip64.so.7 then binds to the copy torch already loaded instead of /opt/rocm's
        # (loading both leaves the second one with "No HIP GPUs are available").
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(_LIB)
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)  # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(code):
    if code != OK:
        raise O3drError(code, load_library().o3dr_last_error().decode(errors="replace"))
