"""MI355X-native per-frame reconstruction hot path of pk17r/online_3d_reconstruction.

The product is libo3dr.so (hand-written HIP for gfx950 behind the C ABI of include/o3dr.h).  This
package is the thin Python host layer over that ABI: `Context` mirrors the four `Pose` member
functions of the reference (pose.h:198,199,216,231) plus the fan-out/accumulate loop, `synth`
generates the benchmark inputs of SURVEY.md section 8d, `dist` shards frames over ranks.

There is no CPU fallback: importing works anywhere, but creating a `Context` without the built
library or without a GPU raises.
"""
from ._lib import CHAIN_FRAME, CLUSTER, CONTOUR_LINE, CONTOUR_SEGMENT, KNN2, ORB_KEYPOINT, PLANE_DISP_SEGMENT, PLANE_TILE, POINT, RANSAC_RESULT, REFINE_EDGE, REFINE_FRAME, RIGID_RESULT, O3drError, lib_path, load_library  # noqa: F401
from .api import ClusterInfo, ContourInfo, Context, DisparityFilterInfo, GroundInfo, IcpResult, InterpolateInfo, MeshResult, MlsResult, MultiviewFuseInfo, MultiviewInfo, Params, RasterInfo, RefineResult, RigidResult, SegmentInfo, contourPolylines, groundSchedule, nearbyFrames, rectifiedQ  # noqa: F401

__all__ = ["CHAIN_FRAME", "CLUSTER", "CONTOUR_LINE", "CONTOUR_SEGMENT", "ClusterInfo", "ContourInfo", "Context", "DisparityFilterInfo", "GroundInfo", "IcpResult", "InterpolateInfo", "KNN2", "MeshResult", "MlsResult", "MultiviewFuseInfo", "MultiviewInfo", "ORB_KEYPOINT", "Params", "PLANE_DISP_SEGMENT", "PLANE_TILE", "POINT", "RANSAC_RESULT", "RasterInfo", "REFINE_EDGE", "REFINE_FRAME", "RIGID_RESULT", "RefineResult", "RigidResult", "SegmentInfo", "O3drError",
           "contourPolylines", "groundSchedule", "lib_path", "load_library", "nearbyFrames", "rectifiedQ"]
