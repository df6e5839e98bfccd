/*
 * o3dr.h — C ABI of libo3dr, the MI355X (gfx950) implementation of the per-frame
 * reconstruction hot path of pk17r/online_3d_reconstruction:
 *
 *   disparity image [-> bilateral filter] -> 3D back-projection through Q -> rigid
 *   transform into the world frame [-> statistical outlier removal] -> voxel-grid
 *   downsample -> accumulate -> 2.5-D global merge.
 *
 * The reference has no FFI/plugin interface; the seam is four `Pose` member
 * functions plus the fan-out/accumulate loop around them.  Every entry point
 * below names the reference interface (file:line under the reference tree) it
 * replaces.  Plain pointers and sizes only: no C++, HIP or torch types.
 *
 * Conventions
 *   - every function returns O3DR_OK (0) or a negative O3DR_ERR_* code; on error
 *     every `n_out` is set to 0 ("output cloud left empty", pose.cpp:620-635).
 *   - `mem` says where ALL data pointers of that call live: O3DR_MEM_HOST
 *     (copied into HBM staging buffers with hipMemcpyAsync straight from the
 *     caller's pointers: page-locked caller memory transfers by DMA, pageable
 *     memory goes through the HIP runtime's own bounce buffers; the batched
 *     o3dr_accumulate_frames uploads batch k+1 on a second stream while batch
 *     k computes) or O3DR_MEM_DEVICE (HBM pointers of the context's device;
 *     nothing is copied).  Small
 *     parameter arrays (Q, poses of the single-frame calls, leaf) are always
 *     host pointers; the batched `o3dr_accumulate_frames` takes its pose array
 *     in `mem` like the images.
 *   - images are OpenCV-layout: disparity CV_8UC1 row-major with a byte pitch (CV_64F
 *     with o3dr_params.disparity_f64: pitch and frame stride stay in bytes),
 *     colour CV_8UC3 interleaved B,G,R with a byte pitch (pose_functions.cpp:526,548).
 *   - points are 16 bytes: x,y,z float + packed colour (a<<24|r<<16|g<<8|b), the
 *     same packing pose_functions.cpp:1120-1121 stores in PointXYZRGB::rgb.
 *   - 4x4 matrices are ROW-major float[16] (only the top three rows are read),
 *     Q is ROW-major double[16] (pose.h:128, cam13calib.yml:91-97).
 *   - a context is single-threaded; the reference's 7 concurrent callers
 *     (pose.cpp:392-413) each own a context.  Work is issued on the context's
 *     stream; calls with host outputs synchronise before returning, calls with
 *     device outputs that report a count synchronise only for that count.
 */
#ifndef O3DR_H
#define O3DR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define O3DR_VERSION 100 /* 0.1.0 */

/* return codes */
#define O3DR_OK                  0
#define O3DR_ERR_INVALID_ARG    -1
#define O3DR_ERR_NO_DEVICE      -2 /* no usable gfx950 device / HIP runtime failure at create */
#define O3DR_ERR_HIP            -3 /* a HIP call failed; o3dr_last_error() has the text */
#define O3DR_ERR_CAPACITY       -4 /* caller's output buffer is too small */
#define O3DR_ERR_NOT_CONFIGURED -5 /* o3dr_set_camera not called yet */
#define O3DR_ERR_ALLOC          -6
#define O3DR_ERR_INTERNAL       -7 /* a device-side consistency guard tripped (O3DR_STATUS_INTERNAL): results are invalid */
#define O3DR_ERR_PEER           -8 /* o3dr_merge_partitioned: another rank failed; every rank left the exchange together */

/* `mem` values */
#define O3DR_MEM_HOST   0
#define O3DR_MEM_DEVICE 1

/* bits of `*status` */
#define O3DR_STATUS_VOXEL_OVERFLOW 1u /* PCL VoxelGrid "Leaf size is too small ... Integer indices
                                         would overflow": output = input, unfiltered [PCL 1.8
                                         filters/impl/voxel_grid.hpp applyFilter] */

#define O3DR_STATUS_INTERNAL 0x80000000u /* a gather guard found a record or point id outside its cloud (library
                                            bug, never expected); calls that read the status return
                                            O3DR_ERR_INTERNAL and an empty output */

typedef struct o3dr_point {
    float    x, y, z;
    uint32_t rgba;
} o3dr_point;

/* Hot-path parameters = the `Pose` members the four functions read. */
typedef struct o3dr_params {
    double   min_disparity;        /* pose.h:93  minDisparity = 64, strict '>' (pose_functions.cpp:1107) */
    double   voxel_size;           /* pose.h:118 voxel_size = 0.1 */
    int32_t  bounding_box;         /* pose.h:94  boundingBox = 20 */
    int32_t  cutout_ratio;         /* pose.h:126 cutout_ratio = 8; cols_start_aft_cutout=(int)(cols/ratio) pose_functions.cpp:638 */
    int32_t  jump_pixels;          /* pose.h:96  jump_pixels = 10; 0 = keypoints only, 1 = dense (no keypoint pass) */
    uint32_t min_points_per_voxel; /* pose.h:108 = 1; only the combined merge uses it (pose_functions.cpp:1693) */
    int32_t  dont_downsample;      /* --dont_downsample, pose.cpp:609 */
    int32_t  sor_enable;           /* statistical outlier removal of the per-frame path (pose_functions.cpp:1673-1686:
                                      mean_k 50, 1 sigma, active iff !combined && jump_pixels > 0).  1 = on, as in the
                                      reference (the default); 0 = off (the measured GPU configs) */
    int32_t  blur_kernel;          /* pose.h:98 blur_kernel = 1; > 1: the disparity image goes through
                                      cv::bilateralFilter(d = blur_kernel, sigmaColor = 2*blur_kernel,
                                      sigmaSpace = blur_kernel/2 (integer division)) first, pose_functions.cpp:1040-1047 */
    int32_t  disparity_f64;        /* --use_segment_labels (pose_functions.cpp:1037,1102): the disparity images handed to
                                      the frame calls are CV_64F (doubles, pitch and frame stride still in bytes) and
                                      are read with at<double>; 0 = CV_8UC1.  Not combinable with blur_kernel > 1
                                      (cv::bilateralFilter rejects CV_64F) */
} o3dr_params;

typedef struct o3dr_ctx o3dr_ctx; /* opaque */

/* ---- library ------------------------------------------------------------------------------ */
int         o3dr_version(void);
/* text of the last failure on the calling thread ("" if none) */
const char* o3dr_last_error(void);
/* fills *p with the reference defaults (pose.h:92-126) */
void        o3dr_default_params(o3dr_params* p);

/* ---- context ------------------------------------------------------------------------------ */
/* One context = one stream + workspaces on device `device_id`.  Fails with O3DR_ERR_NO_DEVICE
 * when there is no GPU: there is no CPU fallback behind this ABI. */
int o3dr_ctx_create(int device_id, o3dr_ctx** out_ctx);
int o3dr_ctx_destroy(o3dr_ctx* ctx);
/* Issue work on a caller-owned hipStream_t (e.g. torch's current stream); NULL restores the
 * context's own stream. */
int o3dr_ctx_set_stream(o3dr_ctx* ctx, void* hip_stream);
int o3dr_ctx_synchronize(o3dr_ctx* ctx);
/* Q of the rectified stereo pair: Pose::Q, pose.h:128, read at pose_functions.cpp:467-476 */
int o3dr_set_camera(o3dr_ctx* ctx, const double Q[16]);
int o3dr_set_params(o3dr_ctx* ctx, const o3dr_params* p);
int o3dr_get_params(o3dr_ctx* ctx, o3dr_params* p);

/* ---- A1: Pose::createSingleImgPtCloud (pose.h:198, pose_functions.cpp:1030-1134) ---------------
 * Camera-frame cloud of one frame: keypoint pass (iff jump_pixels != 1; `kp_xy` = n_kp pairs of
 * float KeyPoint::pt.x,.y, truncated to int like pose_functions.cpp:1061) followed by the row-major
 * grid pass (iff jump_pixels > 0).  `out_capacity` must be >= o3dr_max_points(rows, cols) + n_kp. */
int o3dr_create_single_img_pt_cloud(o3dr_ctx* ctx,
                                    const uint8_t* disp, int64_t disp_pitch,
                                    const uint8_t* bgr, int64_t bgr_pitch,
                                    int32_t rows, int32_t cols,
                                    const float* kp_xy, int32_t n_kp,
                                    o3dr_point* out, int64_t out_capacity, int64_t* n_out,
                                    int32_t mem);
/* number of grid-pass candidates for the context's current params: Ny*Nx of SURVEY section 8 */
int64_t o3dr_max_points(o3dr_ctx* ctx, int32_t rows, int32_t cols);

/* ---- disparity pre-passes -------------------------------------------------------------------
 * cv::bilateralFilter on a CV_8UC1 image — replaces the call at pose_functions.cpp:1044 (OpenCV 3.1
 * bilateralFilter_8u, BORDER_DEFAULT, fp32 sums grouped as an x86-64 build groups them).  d <= 0 derives the
 * radius from sigma_space like OpenCV; radius (d/2) above 64 is O3DR_ERR_INVALID_ARG.  src and dst must not
 * overlap.  With O3DR_MEM_DEVICE the call is asynchronous on the context's stream.  Runs inside the frame calls
 * by itself when o3dr_params.blur_kernel > 1. */
int o3dr_bilateral_filter_u8(o3dr_ctx* ctx, const uint8_t* src, int64_t src_pitch, int32_t rows, int32_t cols, int32_t d,
                             double sigma_color, double sigma_space, uint8_t* dst, int64_t dst_pitch, int32_t mem);
/* Pose::getVariance(disp, false) of n_frames disparity images (pose_functions.cpp:987-1028; the frame gate of
 * pose.cpp:187-196 rejects a frame when it exceeds 5), over the ROI set by o3dr_params.  variance_out: n_frames
 * doubles in HOST memory.  The mean is bit-identical to the reference's; the variance is summed per disparity
 * level instead of per pixel and agrees to fp64 rounding (within N * 2^-53 relative, N = ROI pixels). */
int o3dr_disparity_variance(o3dr_ctx* ctx, const uint8_t* disp, int64_t disp_pitch, int64_t disp_frame_stride, int32_t rows,
                            int32_t cols, int32_t n_frames, double* variance_out, int32_t mem);

/* ---- A2: Pose::transformPtCloud (pose.h:199, pose_functions.cpp:1358-1362) ----------------------
 * out[i].xyz = T * in[i].xyz in fp32, ((m0*x + m1*y) + m2*z) + m3, no fused multiply-add
 * [PCL 1.8 common/impl/transforms.hpp, dense branch]; colour copied.  in == out is allowed
 * (the in-place re-transform of cloud_big after ICP, pose.cpp:353). */
int o3dr_transform_pt_cloud(o3dr_ctx* ctx, const o3dr_point* in, int64_t n,
                            const float T[16], o3dr_point* out, int32_t mem);

/* ---- A1+A2 fused: what createAndTransformPtCloud does before downsampling (pose.cpp:603-607) -- */
int o3dr_reproject_transform(o3dr_ctx* ctx,
                             const uint8_t* disp, int64_t disp_pitch,
                             const uint8_t* bgr, int64_t bgr_pitch,
                             int32_t rows, int32_t cols,
                             const float T[16],
                             const float* kp_xy, int32_t n_kp,
                             o3dr_point* out, int64_t out_capacity, int64_t* n_out,
                             int32_t mem);

/* ---- A4: pcl::VoxelGrid<PointXYZRGB>::applyFilter as used at pose_functions.cpp:1689-1700 ------
 * One output point per occupied voxel with >= min_points points: fp32 centroid, truncated mean
 * colour, ascending linear voxel index (x fastest, then y, then z).  `z_offset` is added to z in
 * fp32 on load and subtracted in fp32 on store (pose_functions.cpp:1666,1702-1704; 0 = none).
 * Points of one voxel are summed in input order (see DESIGN.md "summation order").
 * `out_capacity` must be >= n_in (the overflow fallback returns the input unchanged). */
int o3dr_voxel_grid(o3dr_ctx* ctx, const o3dr_point* in, int64_t n_in,
                    const float leaf[3], uint32_t min_points, float z_offset,
                    o3dr_point* out, int64_t out_capacity, int64_t* n_out, uint32_t* status,
                    int32_t mem);

/* ---- A3b: pcl::StatisticalOutlierRemoval<PointXYZRGB> as configured at pose_functions.cpp:1679-1684 ---
 * (setMeanK(50), setStddevMulThresh(1.0)) on its own: exact 51-nearest-neighbour search, mean neighbour
 * distance per point, global mean + 1 sigma gate; inliers keep their order.  Clouds of <= 50 points
 * pass through (the reference reads past its neighbour list there).  out_capacity >= n_in. */
int o3dr_statistical_outlier_removal(o3dr_ctx* ctx, const o3dr_point* in, int64_t n_in, o3dr_point* out,
                                     int64_t out_capacity, int64_t* n_out, int32_t mem);

/* ---- A3a / A5: Pose::downsamplePtCloud (pose.h:216, pose_functions.cpp:1654-1709) --------------
 * combined == 0: per-frame mode, leaf (voxel_size/5)^3, min_points 0   (:1698)
 * combined != 0: 2.5-D merge, z += 500, leaf (voxel_size, voxel_size, 1000),
 *                min_points_per_voxel, z -= 500                        (:1666,1693-1694,1702-1704) */
int o3dr_downsample_pt_cloud(o3dr_ctx* ctx, const o3dr_point* in, int64_t n_in, int32_t combined,
                             o3dr_point* out, int64_t out_capacity, int64_t* n_out,
                             uint32_t* status, int32_t mem);

/* ---- A6: Pose::createAndTransformPtCloud (pose.h:231, pose.cpp:596-636) -------------------------
 * A1 -> A2 -> (A3a unless dont_downsample) for one frame into a caller-owned cloud. */
int o3dr_create_and_transform_pt_cloud(o3dr_ctx* ctx,
                                       const uint8_t* disp, int64_t disp_pitch,
                                       const uint8_t* bgr, int64_t bgr_pitch,
                                       int32_t rows, int32_t cols,
                                       const float T[16],
                                       const float* kp_xy, int32_t n_kp,
                                       o3dr_point* out, int64_t out_capacity, int64_t* n_out,
                                       uint32_t* status, int32_t mem);

/* ---- A7: fan-out + accumulate (pose.cpp:365-434) and the final merge (pose.cpp:527-532) --------
 * The context owns `cloud_big` in HBM.  o3dr_accumulate_frames runs A6 for `n_frames` frames
 * (frame f at base + f*frame_stride; pose f at poses + 16*f) and appends the per-frame results in
 * frame order, entirely on the device and asynchronously (no host round trip per frame).
 * o3dr_accumulate_frames_kp also runs the keypoint pass (active iff jump_pixels != 1, pose_functions.cpp:1057-1091):
 * frame f's keypoints are kp_xy[2*kp_offsets[f] .. 2*kp_offsets[f+1]) (x,y float pairs, memory kind `mem`);
 * kp_offsets is a HOST array of n_frames+1 non-decreasing entries; NULL = no keypoints.
 * `status_or` (host pointer, may be NULL) is written by o3dr_cloud_big_size/o3dr_finalize. */
int o3dr_accumulate_frames(o3dr_ctx* ctx,
                           const uint8_t* disp, int64_t disp_frame_stride, int64_t disp_pitch,
                           const uint8_t* bgr, int64_t bgr_frame_stride, int64_t bgr_pitch,
                           int32_t rows, int32_t cols,
                           const float* poses, int32_t n_frames, int32_t mem);
int o3dr_accumulate_frames_kp(o3dr_ctx* ctx,
                              const uint8_t* disp, int64_t disp_frame_stride, int64_t disp_pitch,
                              const uint8_t* bgr, int64_t bgr_frame_stride, int64_t bgr_pitch,
                              int32_t rows, int32_t cols,
                              const float* poses, int32_t n_frames,
                              const float* kp_xy, const int64_t* kp_offsets, int32_t mem);
/* reserve HBM for cloud_big (points); optional — it grows on demand */
int o3dr_cloud_big_reserve(o3dr_ctx* ctx, int64_t n_points);
int o3dr_cloud_big_reset(o3dr_ctx* ctx);
/* synchronises; *status = OR of the per-frame O3DR_STATUS_* bits since the last reset */
int o3dr_cloud_big_size(o3dr_ctx* ctx, int64_t* n, uint32_t* status);
int o3dr_cloud_big_read(o3dr_ctx* ctx, o3dr_point* out, int64_t out_capacity, int64_t* n_out, int32_t mem);
/* append externally produced points (a peer rank's shard after the RCCL all-gather, or a PLY) */
int o3dr_cloud_big_append(o3dr_ctx* ctx, const o3dr_point* pts, int64_t n, int32_t mem);
/* in-place rigid re-transform of cloud_big (pose.cpp:353) */
int o3dr_cloud_big_transform(o3dr_ctx* ctx, const float T[16]);
/* cloud_small = downsamplePtCloud(cloud_big, true) (pose.cpp:530); cloud_big is left intact */
int o3dr_finalize(o3dr_ctx* ctx, o3dr_point* out, int64_t out_capacity, int64_t* n_out,
                  uint32_t* status, int32_t mem);
/* cloud_small = downsamplePtCloud(cloud_big, true), like o3dr_finalize and bit-identical to it, but the context keeps
 * every merged cell's running sums: a call folds only the points appended since the previous call and then writes the
 * cells (the reference's per-cycle preview, pose.cpp:437-448, 638-674).  out == NULL with out_capacity == 0: fold and
 * report the result's size in *n_out without writing it.  Output and *status are o3dr_finalize's at that moment
 * (*status includes the per-frame bits OR-ed since the last reset); O3DR_ERR_CAPACITY when out_capacity is below the
 * result's size (not cloud_big's).  A failed call leaves the state empty: the next call folds from the first point.
 * Nothing is allocated or launched before the first call.
 * The state is dropped (the next call refolds cloud_big from its first point) by o3dr_cloud_big_reset, _transform,
 * _partition, _partition_dev, _place_slices, _adopt, _set_size, o3dr_merge_partitioned, an o3dr_set_params that changes
 * voxel_size, and an o3dr_cloud_big_assume_size below the points folded.  Appends (frame calls, o3dr_cloud_big_append)
 * are ordinary tails.  min_points_per_voxel is applied when the cells are written.  Writes into cloud_big through the
 * pointers of o3dr_cloud_big_view / o3dr_cloud_big_raw_view are NOT tracked: after such a write outside the calls above,
 * the state describes points that are no longer there.
 * dont_downsample, PCL's overflow guard for the cloud's box, a cell coordinate of magnitude >= 2^24, or a grid of 2^32
 * cells or more: the call runs o3dr_finalize's own code (and drops the state). */
int o3dr_finalize_incremental(o3dr_ctx* ctx, o3dr_point* out, int64_t out_capacity, int64_t* n_out,
                              uint32_t* status, int32_t mem);
/* what the last o3dr_finalize_incremental did: [0] points folded, [1] 1 = started from an empty state,
 * [2] 1 = answered by o3dr_finalize's own code (see above), [3] cells held, [4] groups held,
 * [5] device bytes held by the state, [6..7] 0 */
int o3dr_finalize_incremental_stats(o3dr_ctx* ctx, int64_t out[8]);

/* ---- multi-GPU merge (frames sharded over ranks) ------------------------------
 * The reference's final merge (pose.cpp:530) runs one voxel grid over ALL frames' per-frame voxels.
 * With one rank per GPU: (1) every rank takes o3dr_cloud_big_bbox and the ranks min/max-reduce it;
 * (2) o3dr_cloud_big_partition lays the combined grid (params: voxel_size, +500 z offset) over that
 * GLOBAL box, cuts its linear index range into n_parts equal slices and stably reorders cloud_big so
 * that slice 0's points come first: counts[p] = points of slice p; (3) the ranks exchange slices
 * (all-to-all over RCCL; received segments appended in source-rank order keep global order);
 * (4) o3dr_finalize_global merges the local slice with the grid over the same global box.  The
 * concatenation of the ranks' outputs in rank order equals the single-GPU result bit for bit.
 * When PCL's overflow guard fires for the global box, *status carries O3DR_STATUS_VOXEL_OVERFLOW, the
 * cloud is left as is and all counts are 0 (the merge then returns its input: skip the exchange). */
int o3dr_cloud_big_bbox(o3dr_ctx* ctx, float mn[3], float mx[3], int64_t* n);
int o3dr_cloud_big_partition(o3dr_ctx* ctx, const float gmin[3], const float gmax[3], int32_t n_parts,
                             int64_t* counts, uint32_t* status);
int o3dr_finalize_global(o3dr_ctx* ctx, const float gmin[3], const float gmax[3], o3dr_point* out,
                         int64_t out_capacity, int64_t* n_out, uint32_t* status, int32_t mem);
/* Zero-copy plumbing for step (3): *ptr = HBM address of cloud_big and its length (the send buffer; valid
 * until the next append/partition/adopt); an HBM receive buffer for n_points points; and "the first
 * n_points of the receive buffer are the new cloud_big" (status bits are kept). */
int o3dr_cloud_big_view(o3dr_ctx* ctx, void** ptr, int64_t* n);
int o3dr_cloud_big_recv_buffer(o3dr_ctx* ctx, int64_t n_points, void** ptr);
int o3dr_cloud_big_adopt(o3dr_ctx* ctx, int64_t n_points);
/* The same two steps with their small data kept in HBM, so that the whole exchange needs ONE host read-back (the
 * all-to-all's sizes): o3dr_cloud_big_header_dev writes this rank's 32-byte header {float min[3], max[3]; int64 count}
 * to the DEVICE buffer hdr_dev; after the ranks all-gathered their headers, o3dr_cloud_big_partition_dev folds the
 * n_hdrs headers at hdrs_dev into the global box and partitions as above, leaving n_parts int64 slice counts
 * followed by one int64 status word (O3DR_STATUS_VOXEL_OVERFLOW: all counts 0, cloud unchanged) in the DEVICE buffer
 * counts_dev.  Both are asynchronous on the context's stream.  o3dr_cloud_big_adopt is stream-ordered as well: what
 * fills the receive buffer must be ordered before the stream's next work by the caller (same stream, or an event).
 * o3dr_cloud_big_assume_size: the caller read its own header back (with the all-to-all's sizes) and tells the library
 * the exact size of cloud_big, so that o3dr_cloud_big_view / o3dr_finalize* need no round trip of their own for it. */
int o3dr_cloud_big_header_dev(o3dr_ctx* ctx, void* hdr_dev);
/* The partition in two halves, so that a rank's own points move ONCE and are never sent to itself (round 4; what
 * o3dr_merge_partitioned and dist.merge_partitioned use):
 *   o3dr_cloud_big_slice_counts_dev - like o3dr_cloud_big_partition_dev, but nothing moves: n_parts int64 slice sizes + the
 *     status word in the DEVICE buffer counts_dev; the (slice, tile) table stays in the workspace;
 *   o3dr_cloud_big_place_slices - after the ranks exchanged their counts: `counts` = this rank's n_parts slice sizes (host),
 *     n_before / n_after = points it will receive from lower / higher ranks.  One pass lays cloud_big out as
 *     [n_before free | own slice | n_after free | the slices that leave, in rank order]; *send_offset = where those start.
 *     A rank that neither sends nor receives keeps its cloud untouched.  The exchange then receives straight into the gaps
 *     (o3dr_cloud_big_raw_view: address and capacity of the buffer) and o3dr_cloud_big_set_size(n_before + own + n_after)
 *     makes that prefix the cloud (stream-ordered, like o3dr_cloud_big_adopt). */
int o3dr_cloud_big_slice_counts_dev(o3dr_ctx* ctx, const void* hdrs_dev, int32_t n_hdrs, int32_t n_parts, int64_t* counts_dev);
int o3dr_cloud_big_place_slices(o3dr_ctx* ctx, int32_t n_parts, int32_t own_part, const int64_t* counts, int64_t n_before,
                                int64_t n_after, int64_t* send_offset);
int o3dr_cloud_big_set_size(o3dr_ctx* ctx, int64_t n_points);
int o3dr_cloud_big_raw_view(o3dr_ctx* ctx, void** ptr, int64_t* capacity_points);
int o3dr_cloud_big_assume_size(o3dr_ctx* ctx, int64_t n_points);
int o3dr_cloud_big_partition_dev(o3dr_ctx* ctx, const void* hdrs_dev, int32_t n_hdrs, int32_t n_parts, int64_t* counts_dev);

/* The whole exchange in ONE call, for C++ hosts (the reference's merge sits in its C++ main flow, pose.cpp:527-532): one
 * host thread and one context per GPU, `nccl_comm` = that GPU's ncclComm_t (RCCL over xGMI; libo3dr resolves RCCL with
 * dlopen at first use and has no link-time dependency on it).  Steps (1)-(4) above with the small data kept in HBM (two
 * all-gathers of a few bytes, ONE host read-back, the slices placed in one pass, one grouped send/receive all-to-all
 * straight into the gaps left for it - the rank's own slice is not sent -, the local merge over the global box), then,
 * with gather_result != 0, an all-gather of the merged
 * slices: `out` receives the whole merged cloud (the single-GPU result, bit for bit); with gather_result == 0 this
 * rank's slice.  A rank that does not want the result passes out = NULL, out_capacity = 0 (it still takes part in every
 * collective).  *n_total = points merged over all ranks.  Must be called by all ranks of the communicator.
 * o3dr_comm_init_all / o3dr_comm_destroy wrap ncclCommInitAll / ncclCommDestroy for single-process hosts (devices ==
 * NULL: 0 .. n_devices-1). */
int o3dr_merge_partitioned(o3dr_ctx* ctx, void* nccl_comm, int32_t gather_result, o3dr_point* out, int64_t out_capacity,
                           int64_t* n_out, int64_t* n_total, uint32_t* status, int32_t mem);
/* Failure is COLLECTIVE: a rank whose own step fails (its header, the partition, an allocation, the local merge) keeps
 * taking part in the collectives that remain with an error word in place of its data - the header's count, a word next
 * to the slice counts, the merged size - and every rank returns at the same point: the failing rank with its own code,
 * the others with O3DR_ERR_PEER.  No rank is left waiting inside a collective its peer never enters.  (Buffers that
 * have to grow between the count matrix and the all-to-all are agreed on with one more 8-byte all-gather, only in calls
 * in which some rank - known to all from the capacities sent with the counts - has to grow one.)  After an error every
 * context stays usable and cloud_big keeps its points (possibly reordered by slice: a later merge gives the same
 * result).  What cannot be made collective is a failure of RCCL itself (O3DR_ERR_HIP).
 * o3dr_merge_partitioned_stats: what the last call of this context moved - out[0] points of this rank before the
 * exchange, [1] points sent to other ranks, [2] points received from other ranks, [3] / [4] the same in bytes (what
 * crosses xGMI), [5] points entering this rank's merge, [6] agreement rounds (0 or 1), [7] points of all ranks.
 * o3dr_cloud_big_capacity: points the cloud buffer and the receive buffer hold without reallocating. */
int o3dr_merge_partitioned_stats(o3dr_ctx* ctx, int64_t out[8]);
int o3dr_cloud_big_capacity(o3dr_ctx* ctx, int64_t* cloud_points, int64_t* recv_points);
int o3dr_comm_init_all(int32_t n_devices, const int32_t* devices, void** comms_out);
int o3dr_comm_destroy(void* comm);
/* hipHostRegister / hipHostUnregister for hosts that link nothing but this ABI: page-locked frame stacks handed to
 * o3dr_accumulate_frames with O3DR_MEM_HOST cross PCIe by DMA instead of through the runtime's bounce buffers */
int o3dr_host_register(void* ptr, int64_t bytes);
int o3dr_host_unregister(void* ptr);

/* ---- point-cloud alignment: pcl::IterativeClosestPoint as the reference runs it (pose.cpp:46-112 --align_point_cloud,
 * runICPalignment pose_functions.cpp:1634-1652): point-to-point ICP with the SVD estimate.  The contract below is this
 * library's own (PCL's results are not bit-pinned); where PCL leaves something open it is made exact and deterministic.
 *
 * Nearest neighbour: for each query q the target point t minimising the key (d2, original target index) in lexicographic
 * order, d2 = ((0 + dx*dx) + dy*dy) + dz*dz in fp32 without FMA (the d2 of A3b); ties go to the lowest index (duplicate
 * target points are well defined).  A candidate counts only if d2 <= r2, r2 = (float)(max_distance * max_distance) (the
 * product in fp64, then rounded; max_distance = +inf: no limit).  No qualifying point (or a query with a non-finite
 * coordinate): idx = 0xFFFFFFFF, d2 = +inf.  Indices refer to the caller's target array.  Target points must be finite.
 *
 * ICP: the cumulative transform T is kept in fp64, starting from T_init (float[16] row-major like o3dr_transform_pt_cloud's
 * T; NULL = identity).  Pass k:
 *   1. P = A2(fp32(T), source): the ORIGINAL source through the fp32-rounded T, bit-identical to o3dr_transform_pt_cloud;
 *   2. every P_i's nearest neighbour within max_correspondence_distance; the correspondences are the points that have one;
 *   3. k > 0 and every source point has the neighbour index it had in pass k-1: stop, O3DR_ICP_UNCHANGED (T is the fixed point);
 *   4. fewer than 3 correspondences: stop, O3DR_ICP_TOO_FEW (T as it is);
 *   5. fp64 moments about c0 = the target's bounding-box centre (count, sum a, sum b, sum a b^T, sum d2 with a = P_i - c0,
 *      b = t_idx(i) - c0) in a fixed order: per-workgroup partials over a fixed partition of the source, folded in a fixed
 *      order - no float atomics, bit-reproducible;
 *   6. dT by Kabsch / Umeyama without scale (fp64, host; proper rotation, reflections corrected); a cross-covariance of rank
 *      < 2 (s2 <= 1e-12 s1): stop, O3DR_ICP_DEGENERATE;
 *   7. T <- dT * T; max |dT - I| over the top three rows <= transformation_epsilon: stop, O3DR_ICP_SMALL_STEP;
 *   8. max_iterations solves applied: stop, O3DR_ICP_MAX_ITERATIONS (max_iterations = 0: T_init with this reason).
 * Then fitness = mean d2 over the correspondences at fp32(T_out) (pcl::Registration::getFitnessScore; DBL_MAX without
 * correspondences) and n_correspondences = their count; UNCHANGED, TOO_FEW and DEGENERATE end on a pass at T_out already,
 * the other reasons take one more pass.  iterations = solves applied.  An empty source or target: O3DR_OK, T = T_init,
 * O3DR_ICP_TOO_FEW, no correspondence.
 * Clouds of at most 2^32-1 points in `mem` (a device pointer such as o3dr_cloud_big_view's works as either).  Both calls
 * synchronise.  They reuse the sort workspace: a pending o3dr_cloud_big_slice_counts_dev table is dropped (a following
 * o3dr_cloud_big_place_slices fails with O3DR_ERR_INVALID_ARG).  On error *res / host outputs are zeroed. */
typedef struct o3dr_icp_params {
    int32_t max_iterations;              /* default 10 (PCL Registration) */
    double  max_correspondence_distance; /* default +inf (no limit) */
    double  transformation_epsilon;      /* default 0 */
} o3dr_icp_params;
typedef struct o3dr_icp_result {
    double  T[16];                       /* row-major 4x4, fp64 */
    double  fitness;
    int64_t n_correspondences;
    int32_t iterations;
    int32_t reason;                      /* O3DR_ICP_* */
} o3dr_icp_result;
#define O3DR_ICP_MAX_ITERATIONS 0
#define O3DR_ICP_UNCHANGED      1
#define O3DR_ICP_SMALL_STEP     2
#define O3DR_ICP_TOO_FEW        3
#define O3DR_ICP_DEGENERATE     4
void o3dr_icp_default_params(o3dr_icp_params* p);
/* idx_out / d2_out: n_query entries each, in `mem` */
int  o3dr_nearest_neighbors(o3dr_ctx* ctx, const o3dr_point* query, int64_t n_query, const o3dr_point* target, int64_t n_target,
                            double max_distance, uint32_t* idx_out, float* d2_out, int32_t mem);
/* the target's search grid is built once per call; only the queries move between passes */
int  o3dr_icp_align(o3dr_ctx* ctx, const o3dr_point* source, int64_t n_source, const o3dr_point* target, int64_t n_target,
                    const float T_init[16], const o3dr_icp_params* p, o3dr_icp_result* res, int32_t mem);

/* ---- feature matching: cv::cuda::DescriptorMatcher::createBFMatcher(NORM_HAMMING)->knnMatch(query, train, k = 2) on
 * 32-byte ORB descriptors, the ratio test and the distance gate (pose.h:180, pose_functions.cpp:2017), and
 * pcl::registration::TransformationEstimationSVD on the matched 3-D keypoints (pose.cpp:213-235).  OpenCV's tie order and
 * PCL's rounding cannot be pinned here, so the contract below is this library's own; where they leave something open it is
 * made exact.
 *
 * o3dr_match_knn2_hamming - batched brute-force 2-NN.  `desc` holds rows of 32 bytes (memory kind `mem`); set s is rows
 * [desc_offsets[s], desc_offsets[s+1]) (HOST array of n_sets + 1 non-decreasing entries, desc_offsets[0] >= 0: the layout of
 * o3dr_accumulate_frames_kp's kp_offsets).  `pairs` (HOST) holds n_pairs (query_set, train_set) int32 pairs; query_set ==
 * train_set is allowed.  For query row i of pair p: d(i, j) = popcount(q_i XOR t_j) over the 256 bits for every row j of the
 * train set, j local to the train set (OpenCV's trainIdx).  The best and second-best rows are the two smallest keys (d, j) in
 * lexicographic order: equal distances go to the lower index.  A missing neighbour (train set of 0 or 1 rows): index and
 * distance 0xFFFFFFFF.  good (n bytes, or NULL: not written) is 1 iff the second neighbour exists, d1 < max_distance and
 * (float)d1 < ratio * (float)d2 in fp32 (all comparisons strict).  Pair p's records start at the exclusive prefix sum of
 * its query-set sizes, in pair order; *n_out = their total, out_capacity below it: O3DR_ERR_CAPACITY with *n_out set and
 * nothing written.  Limits, else O3DR_ERR_INVALID_ARG (host outputs zeroed): the pool desc_offsets[n_sets] -
 * desc_offsets[0] at most 2^32-1 rows, set indices in [0, n_sets), ratio finite and > 0, 0 <= max_distance <= 257.  The
 * call synchronises once at the end; it does not use the sort workspace and leaves cloud_big alone.  Records are integers:
 * results are identical across calls, batchings and memory kinds.
 *
 * o3dr_keypoints_3d - what findFeatures does with Q: one point per keypoint, index-aligned with the keypoints.  Frames in
 * o3dr_accumulate_frames_kp's layout (kp_xy in `mem`, kp_offsets a HOST array of n_frames + 1 non-decreasing entries; bgr
 * may be NULL; poses may be NULL for the camera frame, else 16 floats per frame in `mem`).  Keypoint i of frame f is
 * accepted iff A1's keypoint pass accepts it with the context's params (truncation to int, the ROI, d > min_disparity,
 * disparity_f64, the blur of blur_kernel > 1); it then gets exactly the point that pass emits (posed by poses[f] like
 * o3dr_accumulate_frames_kp; rgba 0 when bgr is NULL).  A rejected keypoint gets NaN x y z and rgba 0.  out_capacity >= the
 * keypoint count; *n_out = that count.  Fewer than 2^31 keypoints.  The call synchronises.
 *
 * o3dr_estimate_rigid_transform - batched TransformationEstimationSVD.  src and tgt: n index-aligned points each (`mem`);
 * segments [seg_offsets[s], seg_offsets[s+1]) (HOST, n_segs + 1 non-decreasing entries within [0, n], each segment at most
 * 2^32-1 points; seg_offsets NULL: one segment [0, n) and n_segs must be 1); mask: n bytes in `mem` or NULL.  Per segment:
 *   1. the used pairs are those with mask != 0 (or no mask) whose six coordinates are all finite;
 *   2. c0 = the segment's first used target point; fp64 moments about c0 (count, sum a, sum b, sum a b^T with a = src - c0,
 *      b = tgt - c0) over the partition and fold of ICP step 5: per-workgroup partials over runs of 256 consecutive points
 *      from the segment's first point, folded per segment in workgroup order - no float atomics;
 *   3. the ICP's host Kabsch (proper rotation, reflection corrected); fewer than 3 used pairs: O3DR_RIGID_TOO_FEW; a
 *      cross-covariance of rank < 2 (s2 <= 1e-12 s1): O3DR_RIGID_DEGENERATE; T is the identity in both cases;
 *   4. rms = sqrt(mean |T src - tgt|^2) over the used pairs in fp64 (same partition and fold; 0 without used pairs).
 * T maps src -> tgt (PCL's convention), row-major fp64.  Results are bit-identical across calls, host and device memory and
 * segment batchings: a segment equals a call on that segment alone.  The call synchronises; it does not use the sort
 * workspace.  On error the host results are zeroed. */
typedef struct o3dr_match_params {
    float   ratio;          /* default 0.5 (the reference's ratio test) */
    int32_t max_distance;   /* default 40 (d1 < 40) */
} o3dr_match_params;
typedef struct o3dr_knn2 {  /* 16 bytes */
    uint32_t train_idx[2];  /* best, second best; 0xFFFFFFFF if missing */
    uint32_t distance[2];   /* Hamming distances; 0xFFFFFFFF if missing */
} o3dr_knn2;
typedef struct o3dr_rigid_result {
    double  T[16];          /* row-major 4x4, src -> tgt */
    double  rms;
    int64_t n_used;
    int32_t status;         /* O3DR_RIGID_* */
    int32_t reserved;       /* 0 */
} o3dr_rigid_result;
#define O3DR_RIGID_OK         0
#define O3DR_RIGID_TOO_FEW    1
#define O3DR_RIGID_DEGENERATE 2
void o3dr_match_default_params(o3dr_match_params* p);
int  o3dr_match_knn2_hamming(o3dr_ctx* ctx, const uint8_t* desc, const int64_t* desc_offsets, int32_t n_sets, const int32_t* pairs,
                             int64_t n_pairs, const o3dr_match_params* p, o3dr_knn2* out, uint8_t* good, int64_t out_capacity,
                             int64_t* n_out, int32_t mem);
int  o3dr_keypoints_3d(o3dr_ctx* ctx, const uint8_t* disp, int64_t disp_frame_stride, int64_t disp_pitch, const uint8_t* bgr,
                       int64_t bgr_frame_stride, int64_t bgr_pitch, int32_t rows, int32_t cols, const float* poses, int32_t n_frames,
                       const float* kp_xy, const int64_t* kp_offsets, o3dr_point* out, int64_t out_capacity, int64_t* n_out,
                       int32_t mem);
int  o3dr_estimate_rigid_transform(o3dr_ctx* ctx, const o3dr_point* src, const o3dr_point* tgt, int64_t n, const int64_t* seg_offsets,
                                   int32_t n_segs, const uint8_t* mask, o3dr_rigid_result* res, int32_t mem);

/* ---- moving-least-squares smoothing and normals: pcl::MovingLeastSquares as the reference's --smooth_surface tool uses it
 * (pose.cpp:27-112, pose_functions.cpp:1711-1813), upsampling NONE, polynomial fit on.  The reference's exact call
 * parameters and PCL's rounding cannot be pinned here, so the contract below is this library's own; where PCL leaves
 * something open it is made exact.
 *
 * Input: n points, every coordinate finite.  r = search_radius (finite, > 0), order = polynomial_order (0, 1 or 2; 0: no
 * polynomial), h = sqr_gauss_param (finite, >= 0; 0 means r*r).  For every point i, p = P_i:
 *   1. Neighbours N(i) = { j : d2(p, P_j) <= r2 }, d2 = ((0 + dx*dx) + dy*dy) + dz*dz in fp32 without FMA (the d2 of
 *      o3dr_nearest_neighbors), r2 = (float)(r*r) with the product in fp64.  p is in N(i); k = |N(i)|.  The set is exact.
 *   2. Plane: the unweighted centroid c and covariance C of N(i) in fp64 (accumulated about p, then shifted; divided by k).
 *      Eigenvalues l0 <= l1 <= l2, the normal n = the unit eigenvector of l0, curvature = l0 / (l0 + l1 + l2) (0 when the
 *      trace is 0).  Orientation: n_z > 0; if n_z == 0 then n_y > 0, then n_x > 0.  k < 3 or l1 <= 1e-12 l2: no fit
 *      (O3DR_MLS_NONE): the point passes through unchanged, normal and curvature are NaN, k is still reported.
 *   3. m = p - (n . (p - c)) n.
 *   4. Polynomial (order >= 1 and k >= nc monomials: 3 for order 1, 6 for order 2): v = normalize(-n_y, n_x, 0) if
 *      |n_z| <= 0.9, else normalize(0, -n_z, n_y); u = n x v.  For j in N(i), e = P_j - m: (u_j, v_j) = (e.u, e.v) / r,
 *      f_j = e.n, w_j = exp(-d2_j / h) with d2_j the fp32 distance of step 1.  Monomials u^a v^b, a + b <= order, a outer
 *      and b inner (1, v, v^2, u, uv, u^2).  (sum w phi phi^T) a = sum w f phi in fp64 by Cholesky without pivoting; a pivot
 *      <= 1e-12 x the largest diagonal entry, k < nc or a non-finite solution: plane (O3DR_MLS_PLANE).  Output point
 *      (float)(m + a_0 n), normal normalize(n - (a_u / r) u - (a_v / r) v), a_v = coefficient 1, a_u = coefficient
 *      order + 1 (PCL 1.8 projectPointToMLSSurface at u = v = 0); curvature stays the plane's.
 *      Order 0 or the plane fallback: the point (float)m, the normal n.
 *   5. The output copies the input point's rgba bits.
 * Each point's sums run in a fixed order (the cells of its search window row by row, points in cell order - by original
 * index inside a cell), with no atomics: results are bit-identical across calls, host and device memory, and in-place
 * (out == cloud) and out-of-place calls.  The cost grows with the sum of k over the cloud.
 * Outputs are index-aligned with the input: out (n points, may equal cloud), normals (4 n floats: nx ny nz curvature, or
 * NULL), nn_count (n, or NULL), fit (n O3DR_MLS_* bytes, or NULL), all in `mem`; *res the counts per fit kind and the
 * largest k.  Clouds of at most 2^32-1 points; n == 0 is OK (zero counts).  A non-finite coordinate anywhere, a bad radius,
 * order or h: O3DR_ERR_INVALID_ARG (host outputs and *res zeroed).  The call synchronises.  It reuses the sort workspace
 * (the search grid of o3dr_nearest_neighbors): a pending o3dr_cloud_big_slice_counts_dev table is dropped; cloud_big is
 * left alone. */
typedef struct o3dr_mls_params {
    double  search_radius;     /* > 0, finite; no usable default (0 is rejected) */
    int32_t polynomial_order;  /* 0, 1, 2; default 2 */
    double  sqr_gauss_param;   /* 0 = search_radius^2 (default) */
} o3dr_mls_params;
typedef struct o3dr_mls_result {
    int64_t n_poly, n_plane, n_none;  /* points per fit kind */
    int32_t max_neighbors;
} o3dr_mls_result;
#define O3DR_MLS_NONE  0
#define O3DR_MLS_PLANE 1
#define O3DR_MLS_POLY  2
void o3dr_mls_default_params(o3dr_mls_params* p);
/* out: n points (may equal cloud); normals: 4n floats nx ny nz curvature, or NULL; nn_count: n or NULL; fit: n or NULL */
int  o3dr_mls_smooth(o3dr_ctx* ctx, const o3dr_point* cloud, int64_t n, const o3dr_mls_params* p, o3dr_point* out,
                     float* normals, uint32_t* nn_count, uint8_t* fit, o3dr_mls_result* res, int32_t mem);

/* ---- RANSAC plane segmentation, whole cloud or per XY tile: pcl::SACSegmentation (SACMODEL_PLANE, SAC_RANSAC,
 * optimizeCoefficients) and pcl::ProjectInliers as the reference's segmentCloud uses them (pose_functions.cpp:2094-2249).
 * The reference's call parameters and PCL's host random sampler cannot be pinned here, so the contract below is this
 * library's own; where PCL leaves something open it is made exact.
 *
 * Input: n points, every coordinate finite.  t = distance_threshold (finite, > 0), H = max_iterations (1 <= H <= 2^20),
 * s = tile_size (0: the whole cloud is one tile, else finite and > 0), seed, optimize (0 or 1).
 *   1. Tiles: ix = floor((double)x / s), iy = floor((double)y / s), both within int32.  Only non-empty tiles exist, ordered
 *      by (iy, ix) ascending; a tile's points are listed in input order.  key = ((uint64)(uint32)iy << 32) | (uint32)ix;
 *      s = 0: one tile, ix = iy = 0, key 0.  m = the tile's point count.
 *   2. Sampling: splitmix64(x) = mix(x + 0x9E3779B97F4A7C15) with mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9,
 *      z = (z ^ (z >> 27)) * 0x94D049BB133111EB, z ^ (z >> 31) (all mod 2^64).  A tile's stream S = splitmix64(seed ^ key);
 *      draw k (0, 1, 2) of hypothesis h (0 <= h < H) is r = splitmix64(S + 3h + k), local index ((r >> 32) * m) >> 32.
 *      A tile's result therefore equals a call with s = 0 on that tile's points (input order) and seed ^ key.
 *   3. Hypothesis plane in fp64 without FMA from the fp32 points p0 p1 p2: e1 = p1 - p0, e2 = p2 - p0, (a, b, c) = e1 x e2
 *      (a = e1y e2z - e1z e2y, b = e1z e2x - e1x e2z, c = e1x e2y - e1y e2x), L2 = (a a + b b) + c c.  Degenerate if two
 *      indices are equal or L2 <= 1e-12 (e1.e1)(e2.e2) (dots as (x x + y y) + z z).  n = (a, b, c) / sqrt(L2),
 *      d = -((nx x0 + ny y0) + nz z0); oriented so that nz > 0 (nz == 0: ny > 0; both 0: nx > 0) by flipping all four; the
 *      scored plane (A, B, C, D) is the four rounded to fp32.
 *   4. Score: the points of the tile with |((A x + B y) + C z) + D| < (float)t in fp32 without FMA (PCL's strict test).
 *      Every hypothesis is scored (no adaptive stop).  The chosen one has the largest count, the smallest h on a tie;
 *      degenerate hypotheses never win.  Status O3DR_PLANE_TOO_FEW (m < 3: nothing drawn) or O3DR_PLANE_DEGENERATE (every
 *      hypothesis degenerate): coefficients NaN, hypothesis -1, sample 0xffffffff, every point of the tile an outlier.
 *   5. Refinement (optimize = 1, the chosen plane has >= 3 inliers): centroid c and covariance (divided by k) of those
 *      inliers in fp64, accumulated about the chosen sample's p0 and then shifted.  Order: every run of 128 consecutive
 *      points of the tile (listing order) is summed by 64 lanes (lane j: points j and 64 + j, in that order), then by an
 *      xor butterfly over the lanes (distance 32, 16, .., 1); lane j of one wave sums the runs j, j + 64, .. in ascending
 *      order, then the same butterfly.  The unit eigenvector of the smallest eigenvalue l0 <= l1 <= l2 by the cyclic Jacobi
 *      of o3dr_mls_smooth.  l1 <= 1e-12 l2: the hypothesis plane stays (refined 0).  Else n is oriented as in 3,
 *      d = -((nx cx + ny cy) + nz cz) in fp64, both rounded to fp32 (refined 1).
 *   6. Labels: the score test of 4 with the final fp32 plane.  Projection: an inlier becomes q = p - dist (A, B, C) in fp32
 *      (dist the test's signed value, the product then the difference); outliers are copied; rgba is always copied.
 * Every count is an integer sum and every fp64 sum runs in the fixed order above: results are bit-identical across calls
 * and across host and device memory.
 * Outputs, all in `mem`, each optional (NULL: skipped), per point index-aligned with the input: inlier (n bytes, 1/0),
 * tile (n int32: the point's tile ordinal), projected (n points), tiles (up to tiles_capacity records in tile order);
 * *n_tiles (host) = the tile count.  tiles_capacity < that count: O3DR_ERR_CAPACITY with *n_tiles set and nothing else
 * written.  Limits, else O3DR_ERR_INVALID_ARG: n <= 2^32-1; tile indices within int32;
 * (ix_max - ix_min + 1)(iy_max - iy_min + 1) <= 2^32-1 (the dense tile id is a 32-bit sort key); n_tiles H <= 2^31.
 * n == 0 is OK (no tiles).  A non-finite
 * coordinate anywhere or a bad parameter: O3DR_ERR_INVALID_ARG.  On an error other than CAPACITY the host outputs are
 * zeroed and *n_tiles is 0.  The call synchronises.  It reuses the sort workspace: a pending
 * o3dr_cloud_big_slice_counts_dev table is dropped; cloud_big is left alone. */
typedef struct o3dr_plane_params {
    double   distance_threshold;  /* > 0, finite; no usable default (0 is rejected) */
    int32_t  max_iterations;      /* hypotheses per tile, 1 .. 2^20; default 1000 */
    double   tile_size;           /* 0 (default): one tile; else > 0, finite */
    uint64_t seed;                /* default 0 */
    int32_t  optimize;            /* 1 (default): least-squares refinement; 0: the RANSAC plane */
} o3dr_plane_params;
typedef struct o3dr_plane_tile {  /* 64 bytes */
    float    coeff[4];            /* A B C D (fp32), NaN unless status OK */
    int32_t  ix, iy;              /* tile indices (0, 0 when tile_size is 0) */
    uint32_t n_points;            /* m */
    uint32_t n_inliers;           /* final inliers (step 6) */
    uint32_t ransac_inliers;      /* the chosen hypothesis's count (step 4) */
    int32_t  hypothesis;          /* the chosen h, -1 if none */
    uint32_t sample[3];           /* its three input indices, 0xffffffff if none */
    int32_t  refined;             /* 1: the plane of step 5 */
    int32_t  status;              /* O3DR_PLANE_* */
    uint32_t reserved;            /* 0 */
} o3dr_plane_tile;
#define O3DR_PLANE_OK         0
#define O3DR_PLANE_TOO_FEW    1
#define O3DR_PLANE_DEGENERATE 2
#define O3DR_PLANE_MAX_ITERATIONS (1 << 20)
void o3dr_plane_default_params(o3dr_plane_params* p);
int  o3dr_segment_plane(o3dr_ctx* ctx, const o3dr_point* cloud, int64_t n, const o3dr_plane_params* p, uint8_t* inlier,
                        int32_t* tile, o3dr_point* projected, o3dr_plane_tile* tiles, int64_t tiles_capacity, int64_t* n_tiles,
                        int32_t mem);

/* ---- height-field surface mesh: the reference's --mesh_surface runs pcl::GreedyProjectionTriangulation (pose.cpp:27-112,
 * pose_functions.cpp:1711-1813).  GP3 is a sequential advancing front whose output depends on processing order; the map
 * this library merges is a height field (at most one point per XY cell of voxel_size), so this is a 2.5-D triangulation of
 * the occupied XY cells instead, exact and parallel.  The contract is this library's own (INTEGRATION.md lists the
 * differences from GP3).
 *
 * Input: n points, n < 2^31, every coordinate finite.  cell_size finite and > 0, with (float)cell_size and
 * 1.0f / (float)cell_size both finite and > 0; L = max_edge_length > 0 (may be +inf).
 *   1. Cells: inv = 1.0f / (float)cell_size; a point's cell is cx = (int)floorf(x * inv), cy = (int)floorf(y * inv) (fp32:
 *      the cell function of the voxel grid, so a map made with voxel_size vs meshes with cell_size = vs).  A cell's vertex
 *      is its lowest-index point; the cell's other points are shadowed: counted, never referenced.
 *   2. Quads: the quad with lower-left cell (cx, cy) has corners a = (cx, cy), b = (cx+1, cy), c = (cx+1, cy+1),
 *      d = (cx, cy+1), counter-clockwise in XY.  Only quads with at least 3 occupied corners emit anything (a may be the
 *      empty one).
 *   3. Predicates: orient(p, q, r) = (qx-px)*(ry-py) - (qy-py)*(rx-px) in fp64 from the fp32 coordinates, as written, no
 *      FMA.  An edge's d2 = ((0 + dx*dx) + dy*dy) + dz*dz in fp32 without FMA (d = q - p; the d2 of o3dr_nearest_neighbors);
 *      it passes the gate iff d2 <= (float)(L*L), the product in fp64.  A triangle is kept iff orient > 0 and all three
 *      of its edges pass the gate.
 *   4. Four corners: diagonal a-c splits into (a,b,c), (a,c,d); diagonal b-d into (a,b,d), (b,c,d).  A split is valid iff
 *      both of its triangles have orient > 0.  Both valid: the one whose diagonal has the smaller d2, a-c on a tie; one
 *      valid: that one; neither: a-c.  Then the keep rule of 3 applies to each triangle of the chosen split.
 *   5. Three corners: the one triangle (b,c,d), (a,c,d), (a,b,d) or (a,b,c) for a missing a, b, c or d; the keep rule
 *      applies.  A candidate that is not kept counts in n_rejected_orientation (orient <= 0) or else n_rejected_length.
 *   6. Output: tris holds 3 int32 input indices per kept triangle (so vertices stay index-aligned with the input), in
 *      ascending (cy, cx) of the quad (y outer, x inner), a quad's triangles in the order of 4 / 5 and their vertices as
 *      listed there (counter-clockwise in XY).  At most 2 n_vertices triangles.  *n_tris (host) = their count;
 *      tris_capacity (in triangles) below it: O3DR_ERR_CAPACITY with *n_tris set and nothing else written.  tris NULL
 *      (capacity 0): only the counts.
 *   7. vertex_normals (3n floats, optional), index-aligned with the input: for the vertex of cell (cx, cy), the kept
 *      triangles that use it, from the quads with lower-left cells (cx-1,cy-1), (cx,cy-1), (cx-1,cy), (cx,cy) in that
 *      order and each quad's triangles in emission order.  Their unnormalised fp64 face normals (q-p) x (r-p), with
 *      e = q - p, f = r - p in fp64: (ey fz - ez fy, ez fx - ex fz, ex fy - ey fx), are summed in that order from 0; the
 *      sum s is divided by sqrt((sx sx + sy sy) + sz sz) in fp64, then rounded to fp32.  A vertex without a triangle and a
 *      shadowed point get NaN.  Kept triangles are counter-clockwise, so normals have nz > 0 (the MLS orientation).
 * Limits, else O3DR_ERR_INVALID_ARG: cell indices within int32; the cell box (cx_max - cx_min + 1)(cy_max - cy_min + 1)
 * <= 2^32 cells (the dense cell id is a 32-bit sort key: 65536 x 65536 cells, 3.2 km x 3.2 km at 0.05 m and more).  A
 * non-finite coordinate anywhere (found before any grid work) or a bad parameter: O3DR_ERR_INVALID_ARG.  On an error other
 * than CAPACITY the host outputs are zeroed and *n_tris is 0.  n == 0 is OK.  Every count is an integer sum and every
 * value a fixed-order computation: results are bit-identical across calls and across host and device memory.  The call
 * synchronises.  It reuses the sort workspace: a pending o3dr_cloud_big_slice_counts_dev table is dropped; cloud_big is
 * left alone. */
typedef struct o3dr_mesh_params {
    double cell_size;        /* > 0, finite; no usable default (0 is rejected): the map's voxel_size */
    double max_edge_length;  /* > 0, may be +inf; no usable default: GP3's setSearchRadius */
} o3dr_mesh_params;
typedef struct o3dr_mesh_result {
    int64_t n_vertices;              /* occupied cells */
    int64_t n_shadowed;              /* points not chosen as their cell's vertex (n - n_vertices) */
    int64_t n_triangles;
    int64_t n_quads_full;            /* quads with 4 vertices */
    int64_t n_rejected_orientation;  /* candidate triangles dropped, by rule (checked in that order) */
    int64_t n_rejected_length;
} o3dr_mesh_result;
void o3dr_mesh_default_params(o3dr_mesh_params* p);
int  o3dr_mesh_surface(o3dr_ctx* ctx, const o3dr_point* cloud, int64_t n, const o3dr_mesh_params* p, int32_t* tris,
                       int64_t tris_capacity, int64_t* n_tris, float* vertex_normals, o3dr_mesh_result* res, int32_t mem);

/* ---- map raster: the merged map as images, one pixel per XY cell - the orthophoto (the cells' colours), the elevation
 * raster (their heights) and a shaded relief.  The reference shows its map in a PCLVisualizer window only (SURVEY section 2
 * row 15); the contract is this library's own.  Every value is an integer, a comparison, a copy or a correctly rounded
 * fp64 operation in the stated order, no FMA: results are bit-identical across calls and across host and device memory.
 *
 * Input: n points, n < 2^31, every coordinate finite.  cell_size as for the mesh (finite and > 0, with (float)cell_size and
 * 1.0f / (float)cell_size finite and > 0).
 *   1. Cells: the mesh's rule, inv = 1.0f / (float)cell_size, cx = (int)floorf(x * inv), cy = (int)floorf(y * inv) in fp32.
 *      The raster covers width x height cells from (cx0, cy0); element [r, c] of every output is cell (cx0 + c, cy0 + r),
 *      rows ascending in cy.  o3dr_raster_extent returns the cloud's own cell box; any other box may be given (several maps
 *      in one raster frame).  Points outside the box are counted in n_outside and ignored.  Limits: width, height >= 1,
 *      cx0 + width - 1 and cy0 + height - 1 within int32, width * height <= 2^28.
 *   2. One point per cell, by `select`: O3DR_RASTER_FIRST the lowest input index (the mesh's vertex rule); O3DR_RASTER_TOP
 *      the greatest z by fp32 >, ties to the lowest index; O3DR_RASTER_BOTTOM the smallest z, ties to the lowest index.
 *      -0.0f and 0.0f are equal.  The cell's other points are shadowed: counted, never used.  A cell with a point is
 *      occupied.
 *   3. Hole fill, fill_radius = R cells, 0 <= R <= 32: an empty cell takes the occupied cell with the smallest
 *      dx*dx + dy*dy <= R*R, ties to the lowest (cy, cx).  Only the occupied cells of 2 are sources: a fill never feeds a
 *      fill.  R = 0: no fill.
 *   4. Outputs, [height, width] each, every pointer optional (NULL: not written): source int32, the input index that
 *      supplies the cell (its own point or the filled one), -1 if none; distance2 int32, 0 for an occupied cell, the squared
 *      cell distance for a filled one, -1 if none; height_map float32, the source point's z copied, NaN if none; color uint8
 *      [.., 3], the source point's colour bytes blue green red (rgba & 255, >> 8, >> 16), 0 if none.
 *   5. shade uint8 (written iff use_light): l' = l / sqrt((lx*lx + ly*ly) + lz*lz), fp64 on the host, the length finite and
 *      > 0.  Per cell with a source, on the heights after the fill: hR = the height of the cell to the right if that cell is
 *      inside the raster and has a source, else the cell's own; hL, hU (row r + 1), hD (row r - 1) likewise; kx = the number
 *      of present horizontal neighbours, ky of vertical ones; gx = kx == 0 ? 0.0 : ((double)hR - (double)hL) /
 *      ((double)kx * cell_size), gy likewise from hU - hD; s = (((-gx) * l'x + (-gy) * l'y) + l'z) /
 *      sqrt((gx*gx + gy*gy) + 1.0); shade = s > 0 ? min(255, 1 + (int)floor(s * 254.0 + 0.5)) : 1 (also for a NaN s);
 *      0 where there is no source.
 *   6. o3dr_raster_result: the box, n_inside + n_outside = n, n_occupied + n_shadowed = n_inside, n_occupied + n_filled +
 *      n_empty = width * height; z_min / z_max over the occupied cells' points (-0.0f taken as 0.0f), NaN when no cell is
 *      occupied.
 * Errors, O3DR_ERR_INVALID_ARG, in this order: a bad parameter (cell_size, select, fill_radius, the light, a box with a
 * side < 1 or a corner outside int32); a non-finite coordinate; a cell index outside int32; a box of more than 2^28 cells
 * (o3dr_raster_extent: the cloud's own).  All are found before any raster work and before anything of the raster's size is
 * allocated.  On an error the host outputs and the result are zeroed.  o3dr_raster_extent needs n > 0;
 * o3dr_rasterize_map takes n == 0 (every cell empty).  Both synchronise, and reuse the operators' scratch: cloud_big and
 * the sort workspace are left alone. */
#define O3DR_RASTER_FIRST 0
#define O3DR_RASTER_TOP 1
#define O3DR_RASTER_BOTTOM 2
#define O3DR_RASTER_MAX_FILL_RADIUS 32
#define O3DR_RASTER_MAX_CELLS (1 << 28)
typedef struct o3dr_raster_params {
    double cell_size;     /* > 0, finite; no usable default (0 is rejected): the map's voxel_size */
    int32_t select;       /* O3DR_RASTER_FIRST */
    int32_t fill_radius;  /* 0 */
    int32_t cx0, cy0, width, height; /* the box; no default (0 x 0 is rejected): o3dr_raster_extent's, or the caller's own */
    int32_t use_light;    /* 0: no shaded relief */
    int32_t reserved;
    double light[3];      /* the direction towards the light (-1, 1, 1: from the north-west, 35 degrees up) */
} o3dr_raster_params;
typedef struct o3dr_raster_outputs {
    float* height_map;    /* width * height */
    uint8_t* color;       /* 3 * width * height */
    uint8_t* shade;       /* width * height; needs use_light */
    int32_t* source;      /* width * height */
    int32_t* distance2;   /* width * height */
} o3dr_raster_outputs;
typedef struct o3dr_raster_result {
    int32_t cx0, cy0, width, height;
    int64_t n_inside, n_outside;    /* points inside / outside the box */
    int64_t n_occupied, n_shadowed; /* cells with a point; points inside the box that their cell did not choose */
    int64_t n_filled, n_empty;      /* empty cells that took a neighbour; cells without a source */
    float z_min, z_max;             /* over the occupied cells' points; NaN when there is none */
} o3dr_raster_result;
void o3dr_raster_default_params(o3dr_raster_params* p);
int  o3dr_raster_extent(o3dr_ctx* ctx, const o3dr_point* cloud, int64_t n, double cell_size, int32_t* cx0, int32_t* cy0,
                        int32_t* width, int32_t* height, int32_t mem);
int  o3dr_rasterize_map(o3dr_ctx* ctx, const o3dr_point* cloud, int64_t n, const o3dr_raster_params* p,
                        const o3dr_raster_outputs* out, o3dr_raster_result* res, int32_t mem);

/* ---- plane-fitted disparity per segment label: the reference's --use_segment_labels front end (SURVEY section 2 row 13:
 * "per-segment least-squares plane over disparity -> CV_64F disparity").  The reference's source for it is not available
 * to this build, so the contract below is this library's own (INTEGRATION.md lists the differences); every input is an
 * integer, so it is exact: results are bit-identical across calls, launch geometries, frame batchings and memory kinds.
 *
 * Inputs: n_frames images of rows x cols pixels.  disp: u8, byte pitch and byte frame stride as in
 * o3dr_disparity_variance.  labels: unsigned integers of label_elem_size bytes (1, 2 or 4) with their own byte pitch and
 * frame stride (multiples of the element size, like the base address); every value must be < n_labels.  Limits, else
 * O3DR_ERR_INVALID_ARG: 1 <= rows, cols <= 8192, 1 <= n_labels <= 65536 - with them every sum below is an integer
 * < 2^53 and converts to fp64 exactly.  p == NULL: the defaults.
 *   1. A pixel participates in its segment's fit iff (double)d > min_disparity (default 0: d == 0 is the stereo matcher's
 *      "no value").
 *   2. Per (frame, label) ten exact integer sums over the participating pixels, x the column and y the row:
 *      n, Sx, Sy, Sxx, Sxy, Syy, Sd, Sxd, Syd, Sdd (64-bit integer adds: no order dependence, no floating-point atomics),
 *      and the segment's pixel count (participating or not).
 *   3. Fit in fp64, every operation one correctly rounded IEEE operation in exactly this order (no FMA), the sums
 *      converted to fp64 first:  mx = Sx / n, my = Sy / n, c0 = Sd / n;
 *        cxx = Sxx - Sx * mx, cxy = Sxy - Sx * my, cyy = Syy - Sy * my,
 *        cxd = Sxd - Sd * mx, cyd = Syd - Sd * my, cdd = Sdd - Sd * c0;
 *        det = cxx * cyy - cxy * cxy;  degenerate iff det <= (O3DR_PLANE_DISP_TOL * cxx) * cyy;
 *        a = (cxd * cyy - cyd * cxy) / det, b = (cyd * cxx - cxd * cxy) / det;
 *        mse = ((cdd - a * cxd) - b * cyd) / n   (mean squared residual, no square root, not clamped).
 *   4. Status: n == 0: O3DR_PLANE_DISP_NONE, the record's numbers all 0.  Else n < min_pixels or degenerate:
 *      O3DR_PLANE_DISP_MEAN, a = b = 0 (mse by the same formula: cdd / n).  Else O3DR_PLANE_DISP_PLANE.  Then, if max_mse > 0
 *      and mse > max_mse: O3DR_PLANE_DISP_NONE (a, b, c0, mse stay in the record as computed).
 *   5. Output pixel (f64, dense [n_frames][rows][cols]): in a PLANE or MEAN segment
 *      out(x, y) = (c0 + a * ((double)x - mx)) + b * ((double)y - my), not clamped, for every pixel of the segment when
 *      fill != 0 (hole filling, the default) and for the participating pixels only when fill == 0; every other pixel keeps
 *      (double)d.  The image is what o3dr_params.disparity_f64 = 1 reads.
 *
 * O3DR_PLANE_DISP_TOL = 2^-20.  Rounding bound of step 3 at the 8192 limit, u = 2^-53: mx carries one rounding, Sx * mx a
 * second, the subtraction a third, and Sx^2 / n <= Sxx, so |cxx' - cxx| <= (3u + 4u^2) Sxx; likewise for cyy, and for cxy
 * with sqrt(Sxx Syy).  (1) An exactly collinear set: on a row all y are equal, so my = Sy / n and Sy * my are exact and
 * cyy' = 0 exactly (a column: cxx' = 0); then det' = -cxy'^2 <= 0 = the right-hand side.  On any other line the n >= 2
 * pixels have n distinct x and n distinct y, so cxx, cyy >= n (n^2 - 1) / 12 and Sxx / cxx <= 1 + 12 * 8191^2 / (n^2 - 1)
 * < 2^28: the three moments carry relative errors <= 3u * 2^28 = 3 * 2^-25, and with cxy^2 = cxx cyy exactly,
 * |det'| <= (4 * 3 * 2^-25 + O(u)) cxx cyy = 0.375 * 2^-20 cxx cyy, below TOL * cxx' * cyy' with a factor 2.6 to spare.
 * (2) Three pixels in an L: cxx = cyy = 2/3, cxy = -+1/3, det = 1/3 = 0.75 cxx cyy; Sxx <= 3 * 8191^2 bounds the absolute
 * errors of the moments by 9 * 2^-27, so det' = 1/3 +- 2^-22, far above TOL * 4/9.
 *
 * Outputs: out (n_frames * rows * cols doubles, 8-byte aligned) and, optional (NULL: skipped), segments: one record per
 * (frame, label) in (frame, label) order, n_frames * n_labels of them; both in `mem`.  *status (host, optional) receives
 * O3DR_STATUS_LABEL_RANGE when a label >= n_labels was found: the call then returns O3DR_ERR_INVALID_ARG (such a pixel is
 * never used as an index).  Checks, in this order, each O3DR_ERR_INVALID_ARG and all before any device work: ctx, mem
 * kind, n_frames < 0 / rows / cols / n_labels / label_elem_size, the parameters (min_disparity NaN, max_mse NaN or < 0);
 * then n_frames == 0 returns O3DR_OK and writes nothing; then NULL disp / labels / out, then pitches, strides and
 * alignments; the label range is found last, on the device.  On error the host outputs are zeroed.  The call
 * synchronises once, at its end; it does not use the sort workspace and leaves cloud_big alone. */
typedef struct o3dr_plane_disp_params {
    double  min_disparity;  /* default 0 */
    int32_t min_pixels;     /* default 3 */
    double  max_mse;        /* default 0: no gate */
    int32_t fill;           /* default 1 */
} o3dr_plane_disp_params;
typedef struct o3dr_plane_disp_segment {  /* 64 bytes */
    double   a, b;          /* slopes along x and y (0 unless PLANE, or NONE by the mse gate) */
    double   c0;            /* the intercept: the mean disparity, the plane's value at (mx, my) */
    double   mx, my;        /* centroid of the participating pixels */
    double   mse;
    uint32_t n_pixels;      /* pixels of the segment */
    uint32_t n;             /* participating pixels */
    int32_t  status;        /* O3DR_PLANE_DISP_* */
    int32_t  reserved;      /* 0 */
} o3dr_plane_disp_segment;
#define O3DR_PLANE_DISP_NONE  0
#define O3DR_PLANE_DISP_MEAN  1
#define O3DR_PLANE_DISP_PLANE 2
#define O3DR_PLANE_DISP_TOL   9.5367431640625e-07 /* 2^-20 */
#define O3DR_PLANE_DISP_MAX_SIDE   8192
#define O3DR_PLANE_DISP_MAX_LABELS 65536
#define O3DR_STATUS_LABEL_RANGE 2u /* o3dr_plane_fit_disparity: a label >= n_labels in the data */
void o3dr_plane_disp_default_params(o3dr_plane_disp_params* p);
int  o3dr_plane_fit_disparity(o3dr_ctx* ctx, const uint8_t* disp, int64_t disp_pitch, int64_t disp_frame_stride, const void* labels,
                              int32_t label_elem_size, int64_t labels_pitch, int64_t labels_frame_stride, int32_t n_labels,
                              int32_t rows, int32_t cols, int32_t n_frames, const o3dr_plane_disp_params* p, double* out,
                              o3dr_plane_disp_segment* segments, uint32_t* status, int32_t mem);

/* ---- ORB features: what the reference's findFeatures gets from OpenCV's OrbFeaturesFinder (SURVEY section 2 row 10,
 * pose.cpp:127,210): oFAST keypoints over a scale pyramid, ranked by a Harris response, oriented by the intensity centroid,
 * described by 256 steered BRIEF tests on 5 x 5 box sums.  OpenCV's learned test pattern and its float rounding cannot be
 * pinned here, so the contract below is this library's own; every step is an exact integer computation, so results are
 * bit-identical across calls, frame batchings and memory kinds.  Not included: OrbFeaturesFinder's 3 x 1 grid.
 *
 * Input: n_frames images of rows x cols pixels (1..8192 each), byte `pitch` and byte `frame_stride`, channels = 3
 * (interleaved B, G, R) or 1 (grey), in `mem`.  W = cols, H = rows.
 *   1. Grey: g = (1868 B + 9617 G + 4899 R + 8192) >> 14 (channels = 1: the byte itself).
 *   2. Pyramid: sc_0 = 65536, sc_l = floor(65536 s^l + 0.5) with s^l built by repeated fp64 multiplication of
 *      (double)scale_factor.  W_l = (W * 65536 + sc_l / 2) / sc_l, H_l likewise (integer division).  A level with W_l = 0 or
 *      H_l = 0 does not exist (nor do the levels after it).  Level l is resampled from level l - 1: rx = (W_{l-1} << 16) /
 *      W_l; fx = max(0, ((2x + 1) rx - 65536) >> 1) (arithmetic shift, 64-bit), x0 = min(fx >> 16, W_{l-1} - 1),
 *      x1 = min(x0 + 1, W_{l-1} - 1), wx = (fx & 0xFFFF) >> 5; y likewise; the pixel is
 *      (p00 (2048 - wx)(2048 - wy) + p01 wx (2048 - wy) + p10 (2048 - wx) wy + p11 wx wy + (1 << 21)) >> 22, p01 at (x1, y0).
 *   3. FAST-9/16 on every level: ring offsets (dx, dy), clockwise from the top with y down: (0,-3) (1,-3) (2,-2) (3,-1) (3,0)
 *      (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3).  With c the centre and p_i the ring,
 *      score = max over the 16 arcs of 9 contiguous ring pixels of max(min_i (p_i - c), min_i (c - p_i)); a pixel is a corner
 *      iff score > fast_threshold; non-corners, and pixels within 3 pixels of the level's border, score 0.  A corner is
 *      kept iff its score is strictly greater than the scores of all 8 neighbours (equal neighbours suppress each other).
 *      Candidates: kept corners with edge <= x < W_l - edge and edge <= y < H_l - edge (none when W_l <= 2 edge).
 *   4. Harris response of a candidate: Ix = 2 (p[y][x+1] - p[y][x-1]) + (p[y-1][x+1] - p[y-1][x-1]) + (p[y+1][x+1] -
 *      p[y+1][x-1]), Iy its transpose; a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy over the 7 x 7 window centred on the
 *      candidate; R = 25 (a b - c^2) - (a + b)^2 in int64 (k = 1/25; |R| < 2^57).
 *   5. Selection: quota_l = floor(n_features W_l / sum_k W_k) over all n_levels levels, the remainder added to level 0.
 *      Per (frame, level) the quota_l candidates that come first under (R descending, y ascending, x ascending) are kept,
 *      all of them if there are fewer; nothing is redistributed.  Output order per frame: level, then y, then x ascending.
 *   6. Orientation: m10 = sum u I, m01 = sum v I over the disc u^2 + v^2 <= 240 of the level image around the keypoint.
 *      D[k] = (round(16384 cos(2 pi k / 64)), round(16384 sin(2 pi k / 64))), k = 0..63.  angle_bin = the k with the largest
 *      m10 D[k].x + m01 D[k].y (int64), the lowest k on a tie; m10 = m01 = 0: bin 0.
 *   7. Descriptor.  Base pattern: test i = (ax, ay, bx, by); the stream is r_n = splitmix64(S + n), n = 0, 1, 2, ... with
 *      S = splitmix64(O3DR_ORB_PATTERN_SEED) (splitmix64 as in the plane segmentation above); a coordinate is the sum of
 *      four consecutive draws (r >> 32) % 7, minus 12; a test takes 16 draws (ax, ay, bx, by in that order) and is drawn
 *      again (the next 16) if a == b or ax^2 + ay^2 > 169 or bx^2 + by^2 > 169.  Steered: rot_k(p) = ((p.x D[k].x - p.y D[k].y
 *      + 8192) >> 14, (p.x D[k].y + p.y D[k].x + 8192) >> 14), arithmetic shifts; every component stays within [-13, 13].
 *      o3dr_orb_pattern returns the table [64][256][4] of (rot_k(a).x, rot_k(a).y, rot_k(b).x, rot_k(b).y) as int8.
 *      S(p) = the sum of the 5 x 5 pixels of the level image centred at keypoint + rot_bin(p).  Bit i = S(a_i) < S(b_i),
 *      stored in byte i >> 3, bit i & 7.
 *   8. Reported: x = (float)(((double)xl + 0.5) * W / W_l - 0.5) (the product, then the quotient, then the difference, each
 *      in fp64), y likewise with H and H_l; size = (float)(31.0 * W / W_l); angle_deg = angle_bin * 5.625.
 *
 * Outputs: kp (records), kp_xy ([n, 2] floats: x, y) and desc ([n, 32] bytes) in `mem`, index-aligned, each optional (NULL:
 * skipped); kp and desc must be 16-byte aligned, kp_xy 8-byte.  offsets: HOST array of n_frames + 1 entries, frame f's rows
 * are [offsets[f], offsets[f+1]): with kp_xy exactly what o3dr_accumulate_frames_kp, o3dr_keypoints_3d and (with desc)
 * o3dr_match_knn2_hamming take.  *n_out = offsets[n_frames].  out_capacity (rows of each output) must be at least n_frames *
 * n_features: below it O3DR_ERR_CAPACITY and none of kp, kp_xy, desc, levels_out is written (offsets and *n_out are zeroed, as
 * on every error).  With O3DR_MEM_HOST the rows from *n_out up to n_frames *
 * n_features are zeroed.  levels_out (or NULL), in `mem`: every frame's grey pyramid, frame-major, the existing levels back
 * to back, rows tight: n_frames * sum_l W_l H_l bytes (o3dr_orb_level_sizes gives the sizes).
 * o3dr_orb_level_sizes: wh[2l] = W_l, wh[2l+1] = H_l (0 0: no such level), quota[l]; either may be NULL.  Host only.
 * Limits, else O3DR_ERR_INVALID_ARG (offsets and *n_out zeroed, host outputs zeroed): 1 <= n_features <= 65535,
 * 1 < scale_factor <= 2, 1 <= n_levels <= 8, 1 <= fast_threshold <= 254, 16 <= edge <= 255, channels 1 or 3, rows and cols in
 * 1..8192, pitch >= cols * channels, n_frames >= 0 (0: O3DR_OK, offsets[0] = 0).  p == NULL: the defaults.  The call
 * synchronises the stream once, at its end (with O3DR_MEM_HOST the copies into pageable caller memory - offsets, levels_out -
 * may block inside the runtime before that, as every host-memory call's do); it carves its own scratch block, does not use the sort workspace and leaves cloud_big
 * alone. */
#define O3DR_ORB_PATTERN_SEED 0x4F5242ull /* "ORB" */
#define O3DR_ORB_MAX_SIDE     8192
#define O3DR_ORB_MAX_LEVELS   8
typedef struct o3dr_orb_params {
    int32_t n_features;     /* default 1500; 1..65535, per frame */
    float   scale_factor;   /* default 1.3f; (1, 2] */
    int32_t n_levels;       /* default 5; 1..8 */
    int32_t fast_threshold; /* default 20; 1..254 */
    int32_t edge;           /* default 31; 16..255: margin inside every level image */
    int32_t channels;       /* default 3: B G R interleaved; 1: grey */
} o3dr_orb_params;
typedef struct o3dr_orb_keypoint {   /* 32 bytes */
    float    x, y;            /* level-0 pixel coordinates */
    float    angle_deg, size; /* angle_bin * 5.625; 31 * W / W_l */
    int64_t  response;        /* the integer Harris response R */
    int16_t  xl, yl;          /* position in its level image */
    uint8_t  level, angle_bin;
    uint16_t reserved;        /* 0 */
} o3dr_orb_keypoint;
void o3dr_orb_default_params(o3dr_orb_params* p);
/* host only, no context: the steered table, 64 * 256 * 4 int8 */
int  o3dr_orb_pattern(int8_t* out);
int  o3dr_orb_level_sizes(int32_t rows, int32_t cols, const o3dr_orb_params* p, int32_t* wh, int32_t* quota);
int  o3dr_orb_detect(o3dr_ctx* ctx, const uint8_t* img, int64_t frame_stride, int64_t pitch, int32_t rows, int32_t cols,
                     int32_t n_frames, const o3dr_orb_params* p, o3dr_orb_keypoint* kp, float* kp_xy, uint8_t* desc,
                     int64_t* offsets, uint8_t* levels_out, int64_t out_capacity, int64_t* n_out, int32_t mem);

/* ---- stereo rectification: what stands between the camera and o3dr_stereo_disparity (OpenCV's initUndistortRectifyMap,
 * then cv::remap with INTER_LINEAR and a constant border).  The reference reads rectified images, so there is nothing of
 * its to pin: the contract below is this library's own; the map is a fixed sequence of correctly rounded fp64 operations
 * (+ - * / and floor, never fused, no reciprocal approximation), the remap is integer arithmetic, so results are
 * bit-identical across calls, frame batchings and memory kinds; tests/rectify_reference.py restates both in numpy.
 * Not included: stereoRectify itself (R1 / R2 / P1 / P2 from R and T come from the calibration file), the fisheye and the
 * thin-prism / tilt models, and masking the disparity image with `valid`.
 *
 * o3dr_rectify_maps - the fixed-point map of one camera.  On the host, in fp64 and in this order:
 *   1. A[i][j] = (P[4i] R[j] + P[4i+1] R[3+j]) + P[4i+2] R[6+j]      (A = the left 3x3 of P, times R)
 *   2. the cofactors, each a difference of two products:
 *      c00 = A11 A22 - A12 A21   c01 = A12 A20 - A10 A22   c02 = A10 A21 - A11 A20
 *      c10 = A02 A21 - A01 A22   c11 = A00 A22 - A02 A20   c12 = A01 A20 - A00 A21
 *      c20 = A01 A12 - A02 A11   c21 = A02 A10 - A00 A12   c22 = A00 A11 - A01 A10
 *   3. det = (A00 c00 + A01 c01) + A02 c02
 *   4. I[i][j] = c[j][i] / det                                       (I = the inverse of A)
 * In the kernel, per destination pixel (u = column, v = row, both converted to double), with fx = K[0], cx = K[2],
 * fy = K[4], cy = K[5] and D = k1 k2 p1 p2 k3 k4 k5 k6, in fp64 and in this order:
 *      X = (I00 u + I01 v) + I02;  Y = (I10 u + I11 v) + I12;  Wc = (I20 u + I21 v) + I22
 *      iw = 1.0 / Wc;  x = X iw;  y = Y iw
 *      x2 = x x;  y2 = y y;  r2 = x2 + y2;  xy2 = 2.0 (x y)
 *      num = 1.0 + ((k3 r2 + k2) r2 + k1) r2;  den = 1.0 + ((k6 r2 + k5) r2 + k4) r2;  kr = num / den
 *      xd = (x kr + p1 xy2) + p2 (r2 + 2.0 x2);  yd = (y kr + p1 (r2 + 2.0 y2)) + p2 xy2
 *      mx = fx xd + cx;  my = fy yd + cy
 *      qx = floor(mx 32.0 + 0.5);  qy = floor(my 32.0 + 0.5)
 * If both qx and qy satisfy -1048576.0 <= q < 1048576.0 (a NaN does not) the pixel stores (int32 qx, int32 qy), else
 * (O3DR_RECTIFY_OUTSIDE, O3DR_RECTIFY_OUTSIDE).  The map is Q5 fixed point (five fractional bits, OpenCV's INTER_BITS);
 * its limits do not depend on the source image's size.  `map`: [rows_out][cols_out][2] int32, in `mem`, 4-byte aligned;
 * with O3DR_MEM_HOST it is computed on the device and copied out.  Limits, else O3DR_ERR_INVALID_ARG before any device
 * work (a host map zeroed where rows_out and cols_out are within their limits): rows_out and cols_out in 1..8192; every
 * entry of `cam` finite; K[1], K[3], K[6], K[7] zero and K[8] one; det finite and not zero.  One launch; the stream is
 * synchronised once, at the end.
 *
 * o3dr_rectify_remap - n_frames images (rows x cols, channels = 1 or 3 interleaved, byte `pitch` and `frame_stride`)
 * through one map (rows_out x cols_out), all integer.  Per destination pixel with map entry (qx, qy):
 *   x0 = qx >> 5 (arithmetic shift: floor), ax = qx & 31; y0 and ay likewise.  The taps (x0, y0), (x0 + 1, y0),
 *   (x0, y0 + 1), (x0 + 1, y0 + 1) weigh (32 - ax)(32 - ay), ax (32 - ay), (32 - ax) ay, ax ay (their sum is 1024).  A tap
 *   outside [0, cols) x [0, rows) reads `border` in every channel.  Per channel out = (sum of w t + 512) >> 10.
 *   valid = 1 iff every tap of non-zero weight is inside, else 0: a sentinel entry gives `border` and 0.
 * src, map, out ([n_frames][rows_out][cols_out][channels], tight) and valid_out (optional, [rows_out][cols_out], one per
 * map: it does not depend on the frame) are all in `mem`; out must not overlap src; map 4-byte aligned.  Limits, else
 * O3DR_ERR_INVALID_ARG before any device work (host outputs zeroed wherever the sizes that give their extent are within
 * their limits): rows, cols, rows_out, cols_out in 1..8192; channels 1 or 3; border in 0..255; group_frames >= 0;
 * pitch >= cols * channels; frame_stride >= rows * pitch when n_frames > 1; n_frames >= 0 (0: O3DR_OK, nothing is
 * touched).  pitch and frame_stride have no upper limit: with O3DR_MEM_HOST the images are staged as frame_stride *
 * (n_frames - 1) + pitch * (rows - 1) + cols * channels bytes, and a stride too large for that returns O3DR_ERR_ALLOC
 * (host outputs zeroed).  group_frames = n > 0 caps the frames one launch takes (default: all of them); results do not
 * depend on it.  One launch per group, whatever the content; the map is read once per launch, not once per frame;
 * valid_out is written by the first launch alone and only when asked for.  The stream is synchronised once, at the end. */
#define O3DR_RECTIFY_MAX_SIDE 8192
#define O3DR_RECTIFY_OUTSIDE (-1048576)   /* -32768 * 32 */
typedef struct o3dr_rectify_camera {
    double K[9];   /* source camera matrix, row-major: K[0]=fx K[2]=cx K[4]=fy K[5]=cy; K[1],K[3],K[6],K[7] must be 0, K[8] 1 */
    double D[8];   /* k1 k2 p1 p2 k3 k4 k5 k6 (OpenCV's order); unused ones 0 */
    double R[9];   /* rectifying rotation (OpenCV R1 / R2), row-major */
    double P[12];  /* new projection (OpenCV P1 / P2), row-major 3x4; only its left 3x3 is used */
} o3dr_rectify_camera;
int  o3dr_rectify_maps(o3dr_ctx* ctx, const o3dr_rectify_camera* cam, int32_t rows_out, int32_t cols_out, int32_t* map, int32_t mem);
int  o3dr_rectify_remap(o3dr_ctx* ctx, const uint8_t* src, int64_t frame_stride, int64_t pitch, int32_t rows, int32_t cols,
                        int32_t channels, int32_t n_frames, const int32_t* map, int32_t rows_out, int32_t cols_out, int32_t border,
                        int32_t group_frames, uint8_t* out, uint8_t* valid_out, int32_t mem);

/* ---- stereo disparity: the 8-bit disparity image every frame call starts from, made here from a rectified pair by
 * census-transform semi-global matching.  The reference reads its disparities as files an offline matcher wrote (SURVEY
 * section 2), so there is nothing of its to pin: the contract below is this library's own; every step is an exact
 * integer computation, so results are bit-identical across calls, frame batchings and memory kinds;
 * tests/stereo_reference.py restates it in numpy.  Median and speckle filtering are a call of their own
 * (o3dr_disparity_filter, below).  Not included: an adaptive P2.  The pair must arrive rectified: o3dr_rectify_maps and
 * o3dr_rectify_remap ("stereo rectification", below) make it so from the raw images and the calibration.
 *
 * Input: `left` and `right`, n_frames images each of rows x cols pixels (1..8192 each), byte `pitch` and byte
 * `frame_stride` (the same for both), channels = 3 (interleaved B, G, R) or 1 (grey), both in `mem`.  W = cols, H = rows,
 * D = n_disparities, d0 = min_disparity; a candidate d in [0, D) stands for the disparity d0 + d.
 *   1. Grey: g = (1868 B + 9617 G + 4899 R + 8192) >> 14 (the ORB contract's step 1; channels = 1: the byte itself).
 *   2. Census, 9 x 7: for pixel (x, y) walk dy = -3..3 (outer) and dx = -4..4 (inner), skipping (0, 0); neighbour number
 *      k = 0..61 in that order; bit k = 1 iff g(clamp(x + dx, 0, W - 1), clamp(y + dy, 0, H - 1)) < g(x, y).  The result is
 *      a uint64, bits 62 and 63 are 0.
 *   3. Matching cost: xr = x - d0 - d; C(x, y, d) = popcount(cenL(x, y) ^ cenR(xr, y)) if xr >= 0, else 63.
 *   4. Paths: the directions (dx, dy) of travel are, in this order, (1,0) (-1,0) (0,1) (0,-1), and for n_paths = 8 also
 *      (1,1) (-1,-1) (1,-1) (-1,1).  q = p - r is the predecessor of p along r.  q outside the image: L_r(p, d) = C(p, d).
 *      Otherwise m = min_k L_r(q, k) and L_r(p, d) = C(p, d) + min(L_r(q, d), L_r(q, d-1) + P1, L_r(q, d+1) + P1, m + P2) - m,
 *      the d-1 term only when d > 0, the d+1 term only when d < D - 1.  All integers; L_r <= 63 + P2 <= 318.
 *   5. Sum: S(p, d) = sum over r of L_r(p, d) (<= 2544 with 8 paths: a uint16).
 *   6. Winner: best(p) = the lowest d that minimises S(p, d).  The pixel is rejected if
 *      (a) x - d0 - best < 0; or
 *      (b) uniqueness > 0 and some k with |k - best| > 1 has S(p, k) (100 - uniqueness) < 100 S(p, best); or
 *      (c) lr_max_diff >= 0 and |bestR(xr, y) - best| > lr_max_diff, where xr = x - d0 - best and bestR(xr, y) = the lowest
 *          d that minimises S((xr + d0 + d, y), d) over the d with xr + d0 + d < W.  lr_max_diff = -1: no such check.
 *   7. Outputs, all in `mem`, each optional (NULL: skipped), [n_frames][H][W] with rows tight:
 *      disp (uint8): d0 + best for an accepted pixel, 0 for a rejected one (a winner with d0 + best = 0 also reads 0): the
 *        image every frame call, o3dr_disparity_variance and o3dr_keypoints_3d take.
 *      disp_q4 (uint16): 16 (d0 + best) + off for an accepted pixel, 0 for a rejected one.  With a = S(best - 1),
 *        b = S(best), c = S(best + 1), den = a - 2 b + c: off = floor((16 (a - c) + den) / (2 den)) (floor division), in
 *        [-8, 8]; best = 0, best = D - 1 or den <= 0: off = 0.
 *      cost (uint16): S(p, best) of every pixel, the rejected ones included.
 *      volume_out (uint16, [n_frames][H][W][D]): S itself (what levels_out is to the ORB call: it tells which stage differs).
 * Limits, else O3DR_ERR_INVALID_ARG before any device work (host outputs zeroed wherever rows, cols, n_frames - and for
 * volume_out n_disparities - are themselves within their limits, so that the outputs' sizes are known): n_disparities a
 * multiple of 32 in 32..256; min_disparity >= 0 with min_disparity + n_disparities <= 256; 0 <= p1 <= p2 <= 255; n_paths
 * 4 or 8; uniqueness in 0..99; lr_max_diff in -1..255; channels 1 or 3; group_frames >= 0; rows and cols in 1..8192;
 * pitch >= cols * channels; frame_stride >= rows * pitch when n_frames > 1; disp_q4, cost and volume_out 2-byte aligned;
 * n_frames >= 0 (0: O3DR_OK, nothing is touched).  pitch and frame_stride have no upper limit: with O3DR_MEM_HOST the images are
 * staged as frame_stride * (n_frames - 1) + pitch * (rows - 1) + cols * channels bytes each, and a stride too large for that
 * returns O3DR_ERR_ALLOC (host outputs zeroed), not O3DR_ERR_INVALID_ARG.  p == NULL: the defaults.  group_frames: the frames of a call go
 * through the kernels in groups whose scratch (two census images, S, the winners: rows * cols * (2 D + 21) bytes a frame)
 * fits 1 GiB - one frame always forms a group -; group_frames = n > 0 caps a group at n frames.  A layout choice inside
 * the scratch block: results do not depend on it.  The call carves its own scratch block, does not use the sort
 * workspace, leaves cloud_big alone and synchronises the stream once, at its end (with O3DR_MEM_HOST the copy of
 * volume_out into pageable caller memory may block inside the runtime before that). */
#define O3DR_STEREO_MAX_SIDE 8192
typedef struct o3dr_stereo_params {
    int32_t n_disparities; /* default 256; a multiple of 32 in 32..256 */
    int32_t min_disparity; /* default 0; >= 0, min_disparity + n_disparities <= 256 */
    int32_t p1;            /* default 10; 0..255 */
    int32_t p2;            /* default 120; p1..255 */
    int32_t n_paths;       /* default 8; 4 or 8 */
    int32_t uniqueness;    /* default 10; 0..99 (percent), 0: no check */
    int32_t lr_max_diff;   /* default 1; -1..255, -1: no left-right check */
    int32_t channels;      /* default 3: B G R interleaved; 1: grey */
    int32_t group_frames;  /* default 0: as many frames per launch group as the scratch budget allows; n > 0: at most n */
} o3dr_stereo_params;
void o3dr_stereo_default_params(o3dr_stereo_params* p);
int  o3dr_stereo_disparity(o3dr_ctx* ctx, const uint8_t* left, const uint8_t* right, int64_t frame_stride, int64_t pitch,
                           int32_t rows, int32_t cols, int32_t n_frames, const o3dr_stereo_params* p, uint8_t* disp,
                           uint16_t* disp_q4, uint16_t* cost, uint16_t* volume_out, int32_t mem);

/* ---- disparity filter: what every production semi-global matcher ends with (OpenCV's medianBlur, then filterSpeckles):
 * a k x k median of the disparity image, then the removal of small connected components.  The reference reads finished
 * disparity files, so there is nothing of its to pin: the contract below is this library's own; every step is an exact
 * integer computation, so results are bit-identical across calls, frame batchings and memory kinds;
 * tests/disparity_filter_reference.py restates it in numpy.
 *
 * Input: `disp`, n_frames images of rows x cols elements (1..8192 each) of elem_bytes bytes (1: uint8, o3dr_stereo_disparity's
 * disp; 2: uint16, its disp_q4), byte `pitch` and byte `frame_stride`, in `mem`.  W = cols, H = rows, v(x, y) the input.
 *   1. Median, median_size = k in {3, 5}: m(x, y) = element k * k / 2 (0-based) of the ascending sort of the k x k values
 *      v(clamp(x + dx, 0, W - 1), clamp(y + dy, 0, H - 1)), dx and dy in -(k / 2)..k / 2.  Zero (the rejected pixel) is a
 *      value like any other: an isolated wrong pixel goes, and so does an isolated hole.  k = 0: m = v.
 *   2. Components: a pixel is valid iff m != 0.  Two 4-neighbours of the same frame are joined iff both are valid and
 *      |m(p) - m(q)| <= max_diff, the difference taken in a type that holds it (65535 against 1 differs by 65534).
 *      Components are the transitive closure of the joins.  label(p) = the lowest y * W + x (within the frame) of p's
 *      component, -1 for an invalid pixel; size(p) = the component's pixel count, 0 for an invalid pixel.
 *   3. Speckles, max_speckle_size = n > 0: a valid pixel with size(p) <= n becomes 0 (OpenCV's <=); every other pixel
 *      keeps m.  n = 0: every pixel keeps m.
 *   4. Outputs, all in `mem`, [n_frames][H][W] with rows tight: out (required, the input's element type, must not overlap
 *      disp): the image after step 3.  labels_out, sizes_out (int32, each optional, NULL: skipped): label and size of
 *      step 2, before any removal.  info (HOST, optional, one per frame): n_valid = valid pixels, n_components =
 *      components among them, n_speckles = components removed, n_removed = pixels removed (both 0 with
 *      max_speckle_size = 0), largest = the size of the largest component (0: none).
 *      With max_speckle_size = 0 and none of labels_out, sizes_out and info asked for no labelling kernel is launched;
 *      with median_size = 0 as well, out = disp.
 * Limits, else O3DR_ERR_INVALID_ARG before any device work (host outputs zeroed wherever rows, cols, n_frames - and for
 * out elem_bytes - are themselves within their limits, so that the outputs' sizes are known): elem_bytes 1 or 2;
 * median_size 0, 3 or 5; max_speckle_size >= 0; max_diff in 0..65535; group_frames >= 0; rows and cols in 1..8192;
 * pitch >= cols * elem_bytes; frame_stride >= rows * pitch when n_frames > 1; disp and out 2-byte aligned (and pitch and
 * frame_stride even) when elem_bytes = 2; labels_out and sizes_out 4-byte aligned; the bytes of out apart from the bytes of disp (as staged, below); n_frames >= 0 (0: O3DR_OK,
 * nothing is touched).  pitch and frame_stride have no upper limit: with O3DR_MEM_HOST the image is staged as
 * frame_stride * (n_frames - 1) + pitch * (rows - 1) + cols * elem_bytes bytes, and a stride too large for that returns
 * O3DR_ERR_ALLOC (host outputs zeroed), not O3DR_ERR_INVALID_ARG.  p == NULL: the defaults.  group_frames: the frames of a
 * call go through the kernels in groups whose scratch (label and count, 8 bytes a pixel) fits 1 GiB - one frame always
 * forms a group -; group_frames = n > 0 caps a group at n frames.  A layout choice inside the scratch block: results do
 * not depend on it.  The number of launches of a group depends on the switches and the image's size alone, never on its
 * content.  The call carves its own scratch block, does not use the sort workspace, leaves cloud_big alone and
 * synchronises the stream once, at its end. */
#define O3DR_DISPARITY_FILTER_MAX_SIDE 8192
typedef struct o3dr_disparity_filter_params {
    int32_t elem_bytes;       /* default 1: uint8 image (disp); 2: uint16 image (disp_q4) */
    int32_t median_size;      /* default 0: no median; 3 or 5 */
    int32_t max_speckle_size; /* default 0: no speckle removal; n > 0: components of <= n pixels are removed */
    int32_t max_diff;         /* default 1; 0..65535, in the image's own units */
    int32_t group_frames;     /* default 0: as many frames per launch group as the scratch budget allows; n > 0: at most n */
} o3dr_disparity_filter_params;
typedef struct o3dr_disparity_filter_info {   /* one per frame, HOST */
    int64_t n_valid;        /* non-zero pixels after the median */
    int64_t n_components;   /* components among them */
    int64_t n_speckles;     /* components removed */
    int64_t n_removed;      /* pixels removed */
    int64_t largest;        /* size of the largest component (0: none) */
} o3dr_disparity_filter_info;
void o3dr_disparity_filter_default_params(o3dr_disparity_filter_params* p);
int  o3dr_disparity_filter(o3dr_ctx* ctx, const void* disp, int64_t frame_stride, int64_t pitch, int32_t rows, int32_t cols,
                           int32_t n_frames, const o3dr_disparity_filter_params* p, void* out, int32_t* labels_out,
                           int32_t* sizes_out, o3dr_disparity_filter_info* info, int32_t mem);

/* ---- multi-view filter: the geometric consistency test multi-view stereo pipelines end on.  Every rejection test before it
 * (uniqueness, left-right, median, speckles) looks at one stereo pair; this one relates a frame's disparity image to those
 * of other frames of the same ground through their poses: a depth is kept when other views see the same surface there,
 * and dropped when nobody confirms it or when it floats in space that other views see through.  The reference has no
 * such step, so there is nothing of its to pin: the contract below is this library's own; every value is computed in
 * fp64 in a stated order without fused multiply-add, so results are bit-identical across calls, frame batchings and
 * memory kinds; tests/multiview_reference.py restates it in numpy.
 *
 * Input: `disp`, n_frames images of rows x cols elements (1..8192 each) of elem_bytes bytes (1: uint8, level = v; 2: uint16,
 * o3dr_stereo_disparity's disp_q4, level = v / 16; 8: float64, level = v), byte `pitch` and byte `frame_stride`, in `mem`.
 * A pixel is valid iff v != 0; a float64 pixel iff v > 0 and finite.  `poses`: [n_frames][16] float32, row-major
 * camera-to-world (what o3dr_accumulate_frames takes), always HOST.  `neighbors`: [n_frames][k] int32, always HOST, k in
 * 0..16: the frames each frame is tested against; -1: none; an entry that equals its own frame or lies outside
 * 0..n_frames - 1 is O3DR_ERR_INVALID_ARG; a frame listed twice votes twice.  Q is the context's camera (o3dr_set_camera).
 *   1. Neighbours (o3dr_nearby_frames, host only, no context): a frame's position is the fp64 of its pose's translation
 *      column; dist2 = (dx * dx + dy * dy) + dz * dz; frame i's list is the frames j != i with dist2 <= max_distance *
 *      max_distance (an infinite max_distance takes all), ordered by (dist2, j), the first k, padded with -1.  Earlier and
 *      later frames both count (unlike the pose chain's rule).  NULL poses or neighbors_out with n_frames * k > 0, n_frames
 *      < 0, k outside 0..16, a negative or NaN max_distance: O3DR_ERR_INVALID_ARG.
 *   2. Homographies: Q maps (x, y, d, 1) to a homogeneous camera point, a pose maps that to the world, so one matrix per
 *      ordered pair carries a pixel of frame i and its level to the pixel of frame j it should appear at and the level it
 *      should have there: H_ij = Q^-1 (T_j^-1 T_i) Q.  All fp64; every product of two 4 x 4 matrices has the elements
 *      ((a_r0 b_0c + a_r1 b_1c) + a_r2 b_2c) + a_r3 b_3c.  T^-1 of a pose is the rigid inverse of its upper 3 x 4: rows
 *      (R_0r, R_1r, R_2r, -((R_0r t_0 + R_1r t_1) + R_2r t_2)), r = 0..2, then (0, 0, 0, 1) - a float pose's rotation is
 *      orthonormal to about 1e-7 only, and that is accepted: H_ii is the identity to that precision, not exactly.
 *      E = T_j^-1 T_i, G = E Q, H = Q^-1 G.  Q^-1 is the adjugate over the determinant, with a = Q:
 *        s0 = a00 a11 - a10 a01   s1 = a00 a12 - a10 a02   s2 = a00 a13 - a10 a03
 *        s3 = a01 a12 - a11 a02   s4 = a01 a13 - a11 a03   s5 = a02 a13 - a12 a03
 *        c5 = a22 a33 - a32 a23   c4 = a21 a33 - a31 a23   c3 = a21 a32 - a31 a22
 *        c2 = a20 a33 - a30 a23   c1 = a20 a32 - a30 a22   c0 = a20 a31 - a30 a21
 *        det = ((((s0 c5 - s1 c4) + s2 c3) + s3 c2) - s4 c1) + s5 c0
 *        b00 = (a11 c5 - a12 c4) + a13 c3   b01 = (a02 c4 - a01 c5) - a03 c3
 *        b02 = (a31 s5 - a32 s4) + a33 s3   b03 = (a22 s4 - a21 s5) - a23 s3
 *        b10 = (a12 c2 - a10 c5) - a13 c1   b11 = (a00 c5 - a02 c2) + a03 c1
 *        b12 = (a32 s2 - a30 s5) - a33 s1   b13 = (a20 s5 - a22 s2) + a23 s1
 *        b20 = (a10 c4 - a11 c2) + a13 c0   b21 = (a01 c2 - a00 c4) - a03 c0
 *        b22 = (a30 s4 - a31 s2) + a33 s0   b23 = (a21 s2 - a20 s4) - a23 s0
 *        b30 = (a11 c1 - a10 c3) - a12 c0   b31 = (a00 c3 - a01 c1) + a02 c0
 *        b32 = (a31 s1 - a30 s3) - a32 s0   b33 = (a20 s3 - a21 s1) + a22 s0
 *      and Q^-1[r][c] = b_rc / det (a true division).  A zero or non-finite determinant is O3DR_ERR_INVALID_ARG.
 *      o3dr_multiview_homographies returns exactly the matrices the filter uses ([n_frames][k][16], row-major, HOST; zeros
 *      for a -1 entry), so that a wrong matrix can be told from a wrong kernel; it does no device work.
 *   3. Tests: per valid pixel (x, y) of frame i with level d, for each listed neighbour j with H = H_ij:
 *      h_r = ((H[r][0] x + H[r][1] y) + H[r][2] d) + H[r][3]; xp = h0 / h3, yp = h1 / h3, dp = h2 / h3 (true divisions, no
 *      reciprocal); xr = floor(xp + 0.5), yr = floor(yp + 0.5).  The test is OUTSIDE unless h3 > 0, dp > 0, 0 <= xr < cols
 *      and 0 <= yr < rows (every comparison is false on NaN).  Otherwise, with e the level of frame j's INPUT pixel
 *      (xr, yr): HOLE if that pixel is invalid; SUPPORT if |e - dp| <= tolerance; VIOLATION if e < dp (j sees something
 *      farther through the place this point claims); OCCLUDED otherwise.
 *   4. Keep rule: support(p) and violations(p) count the tests of those two classes.  A valid pixel is kept iff support >=
 *      min_support and (max_violations = -1: violations < support; max_violations = n >= 0: violations <= n).  A removed
 *      pixel becomes 0; an invalid pixel passes through unchanged with both counts 0.  Neighbours are always read from
 *      the input, never from `out`.
 *   5. Outputs, all in `mem`, [n_frames][H][W] with rows tight: out (required, the input's element type, must not overlap
 *      disp).  support_out, violations_out (uint8, each optional, NULL: skipped).  info (HOST, optional, one per frame):
 *      n_valid; n_kept; n_no_support = removed with support < min_support; n_violated = removed otherwise; n_outside,
 *      n_hole, n_support, n_violation, n_occluded = the tests of each class over (valid pixel, listed neighbour).
 * Limits, else O3DR_ERR_INVALID_ARG before any device work (host outputs zeroed wherever rows, cols, n_frames - and for
 * out elem_bytes - are themselves within their limits, so that the outputs' sizes are known): elem_bytes 1, 2 or 8;
 * tolerance finite and >= 0; min_support in 0..16; max_violations in -1..16; k in 0..16; rows and cols in 1..8192; pitch >=
 * cols * elem_bytes; frame_stride >= rows * pitch when n_frames > 1; disp, out, pitch and frame_stride aligned to
 * elem_bytes; the neighbour entries as above; a singular Q; the bytes of out apart from the bytes of disp; n_frames >= 0
 * (0: O3DR_OK, nothing is touched).  Without o3dr_set_camera: O3DR_ERR_NOT_CONFIGURED.  p == NULL: the defaults.  Frames
 * read each other, so a HOST image is staged whole (frame_stride * (n_frames - 1) + pitch * (rows - 1) + cols *
 * elem_bytes bytes): a call that does not fit returns O3DR_ERR_ALLOC (host outputs zeroed).  The matrices are made on the
 * host and uploaded (128 bytes a pair).  One launch per 65535 frames: the number of launches depends on the sizes alone,
 * never on the content.  The call carves its own scratch block, does not use the sort workspace, leaves cloud_big alone
 * and synchronises the stream once, at its end. */
#define O3DR_MULTIVIEW_MAX_SIDE 8192
#define O3DR_MULTIVIEW_MAX_NEIGHBORS 16
typedef struct o3dr_multiview_params {
    int32_t elem_bytes;      /* default 1: uint8 levels; 2: uint16 sixteenths of a level (disp_q4); 8: float64 levels */
    double  tolerance;       /* default 1.0 levels; finite, >= 0 */
    int32_t min_support;     /* default 1; 0..16 */
    int32_t max_violations;  /* default -1: fewer violations than supports; n in 0..16: at most n violations */
} o3dr_multiview_params;
typedef struct o3dr_multiview_info {   /* one per frame, HOST */
    int64_t n_valid;        /* valid input pixels */
    int64_t n_kept;         /* ... that stay */
    int64_t n_no_support;   /* removed with support < min_support */
    int64_t n_violated;     /* removed otherwise */
    int64_t n_outside;      /* tests per class, over (valid pixel, listed neighbour) */
    int64_t n_hole;
    int64_t n_support;
    int64_t n_violation;
    int64_t n_occluded;
} o3dr_multiview_info;
void o3dr_multiview_default_params(o3dr_multiview_params* p);
int  o3dr_nearby_frames(const float* poses, int32_t n_frames, int32_t k, double max_distance, int32_t* neighbors_out);
int  o3dr_multiview_homographies(o3dr_ctx* ctx, const float* poses, int32_t n_frames, const int32_t* neighbors, int32_t k,
                                 double* H_out);
int  o3dr_multiview_filter(o3dr_ctx* ctx, const void* disp, int64_t frame_stride, int64_t pitch, int32_t rows, int32_t cols,
                           int32_t n_frames, const float* poses, const int32_t* neighbors, int32_t k,
                           const o3dr_multiview_params* p, void* out, uint8_t* support_out, uint8_t* violations_out,
                           o3dr_multiview_info* info, int32_t mem);

/* ---- multi-view fusion: the filter above finds, for every pixel, the views that agree with it, uses that to keep or zero
 * the pixel, and forgets what those views measured.  The fusion keeps it: several frames see the same ground from slightly
 * different places, so their quantisation phases differ, and the mean of the pixel's own level and the levels its
 * supporting neighbours vote for lies nearer the real-valued level than any one of them (on the filter tests' plane scene,
 * 5 uint8 frames: RMS error 0.16 levels against the input's 0.29).  It needs no segmentation and assumes no planes
 * (o3dr_plane_fit_disparity does both) and works on any input (o3dr_stereo_disparity's disp_q4 only on what this library
 * matched itself).  The output is a float64 level image: what o3dr_params.disparity_f64 and the frame calls read.
 * tests/multiview_fuse_reference.py restates the contract in numpy.
 *
 * Steps 1 to 4 of the filter hold word for word: inputs, validity, neighbours, H_ij, the five test classes, the keep rule,
 * o3dr_multiview_params and the limits.  Two steps are added, both in fp64, in the stated order, without fused multiply-add:
 *   5. Votes: for a valid pixel (x, y) of frame i with level d, each listed neighbour whose test is SUPPORT, with e the
 *      neighbour's level at (xr, yr) and H = H_ij:
 *        a2  = (H[2][0] x + H[2][1] y) + H[2][3]
 *        a3  = (H[3][0] x + H[3][1] y) + H[3][3]
 *        num = e * a3 - a2
 *        den = H[2][2] - e * H[3][2]
 *        v   = num / den        (a true division)
 *      v is the level on this pixel's own ray at which the neighbour would have seen exactly e: it solves dp(v) = e.  The
 *      support is a VOTE iff v > 0 and v is finite (both comparisons are false on NaN), a DROPPED VOTE otherwise.  A dropped
 *      vote still counts as support for the keep rule.
 *   6. Fusion: acc = d; acc = acc + v for each vote in the order of the neighbour list (a frame listed twice votes twice);
 *      fused = acc / (double)(1 + votes).  A kept pixel with no vote returns d exactly.  A removed pixel and an invalid pixel
 *      give 0.0 (an invalid float64 pixel does not pass through, unlike in the filter).  For uint16 input d and e are
 *      v / 16.0: the output is always in levels.  A kept pixel is positive and never NaN; it is finite wherever the sum of
 *      at most 17 levels is.
 * Outputs, all in `mem`, [n_frames][rows][cols] with rows tight: out (required, float64, 8-byte aligned, must not overlap
 * disp).  votes_out (uint8, optional): the votes of every valid pixel, as support_out counts its supports; 0 at an invalid
 * pixel.  support_out, violations_out: the filter's.  info (HOST, optional, one per frame): `filter` is exactly what
 * o3dr_multiview_filter reports for the same call; n_votes and n_votes_dropped count the supports of either kind over
 * (valid pixel, listed neighbour), so n_votes + n_votes_dropped == filter.n_support; n_fused counts the kept pixels with
 * at least one vote.  Three identities follow: out > 0 exactly where the filter keeps a valid pixel (its out != 0, for
 * integer input); support_out, violations_out and info.filter equal the filter's; and where no test is a support
 * (tolerance = 0 on real data: dp is never an exact level) out is the filtered image's levels exactly.
 * Errors are the filter's: the same codes in the same order, host outputs zeroed, nothing launched (out's size is known
 * whatever elem_bytes is).  One launch per 65535 frames, counted under O3DR_K_MULTIVIEW; the same scratch, staging and the
 * one synchronise at the end. */
typedef struct o3dr_multiview_fuse_info {   /* one per frame, HOST */
    o3dr_multiview_info filter;   /* exactly what o3dr_multiview_filter reports for the same call */
    int64_t n_votes;              /* over (valid pixel, listed neighbour): supports that voted */
    int64_t n_votes_dropped;      /* ... supports that did not; n_votes + n_votes_dropped == filter.n_support */
    int64_t n_fused;              /* kept pixels with at least one vote */
} o3dr_multiview_fuse_info;
int  o3dr_multiview_fuse(o3dr_ctx* ctx, const void* disp, int64_t frame_stride, int64_t pitch, int32_t rows, int32_t cols,
                         int32_t n_frames, const float* poses, const int32_t* neighbors, int32_t k,
                         const o3dr_multiview_params* p, double* out, uint8_t* votes_out, uint8_t* support_out,
                         uint8_t* violations_out, o3dr_multiview_fuse_info* info, int32_t mem);

/* ---- image segmentation: the segment label image that o3dr_plane_fit_disparity reads (the reference takes it from offline
 * files, segmentlabels/<n>.png): grid-seeded k-means superpixels on the colour image (SLIC-like), connected components, a
 * merge of the small ones, labels numbered compactly.  There is nothing of the reference's to pin: the contract below is
 * this library's own; every step is an exact integer computation (int64 holds every intermediate value), so results are
 * bit-identical across calls, frame batchings and memory kinds; tests/segment_reference.py restates it in numpy.
 *
 * Input: `img`, n_frames uint8 images of rows x cols pixels (1..8192 each) of `channels` bytes (3: B G R; 1: grey, which
 * counts as B = G = R), byte `pitch` and byte `frame_stride`, in `mem`.  W = cols, H = rows, S = step, m = compactness,
 * K = iterations; every division below is the floored integer division of non-negative values.
 *   1. Seeds: nx = ceil(W / S), ny = ceil(H / S); centre k = gy * nx + gx starts at x_k = min(gx * S + S / 2, W - 1),
 *      y_k = min(gy * S + S / 2, H - 1) with that pixel's colour (B_k, G_k, R_k).  Centres are integers throughout.
 *   2. Assignment: pixel (x, y) has the home cell (x / S, y / S); its candidates are the centres of the up to 9 cells
 *      (hx + dx, hy + dy), dx and dy in -1..1, that exist.  Its label is the candidate k with the lowest
 *      D = S^2 ((B - B_k)^2 + (G - G_k)^2 + (R - R_k)^2) + m^2 ((x - x_k)^2 + (y - y_k)^2)  (below 2^37); ties go to the
 *      lowest k.  The colour is raw B G R, not Lab (cube roots cannot be pinned); m = 20 is the default that fits it.
 *   3. Update: per centre the exact sums n, sum x, sum y, sum B, sum G, sum R over its pixels; each new value is
 *      (2 sum + n) / (2 n) - the mean rounded half up.  A centre with n = 0 keeps its values and stays a candidate.  A
 *      centre only ever receives pixels of the 9 cells around its own, so n <= 9 S^2 and sum x < 9 * 2^16 * 2^13 < 2^33:
 *      the sums are 64-bit, and integer adds carry no order dependence.
 *   4. Raw labels: K rounds of (assignment, update), then one more assignment: L0, whose values are centre indices.
 *   5. Components: two 4-neighbours of one frame are joined iff their L0 is equal.  A component is identified by its
 *      lowest pixel index y * W + x, its first pixel.  It is small iff its pixel count is below min_size.
 *   6. Merge: a small component c joins the component c' that minimises the 64-bit key (d << 32 | first pixel of c') over
 *      all not-small components c' 4-adjacent to any pixel of c, d = the squared B G R distance (< 2^18) between the
 *      centres (after step 4) whose indices are the two components' L0.  If c touches no not-small component - every
 *      component next to it is small - it goes where the component of the pixel left of its first pixel goes (the
 *      pixel above it where x = 0); the component that holds pixel 0 then stays as it is.  That neighbour is not in c and
 *      has a lower index, so its component's first pixel is strictly lower than c's: every chain of such steps ends, at a
 *      not-small component or at the component of pixel 0.  Not-small components never move.  Every final label is
 *      4-connected.
 *   7. Numbering: the final labels are numbered 0 .. n_labels - 1 by ascending first pixel, the first pixel of a label
 *      being the lowest first pixel of the components that went into it.
 * Outputs, [n_frames][H][W] with rows tight, in `mem`: labels (int32, required; never negative, so uint32 readers take
 * it as it is).  raw_out (int32, optional): L0.  sizes_out (int32, optional): the pixel count of the pixel's final label.
 * info (HOST, optional, one per frame): n_centres = nx ny, n_components (step 5), n_merged = components that joined
 * another one, n_labels = n_components - n_merged, largest / smallest = pixel counts of the largest and smallest label.
 * Limits, else O3DR_ERR_INVALID_ARG before any device work (host outputs zeroed wherever rows, cols and n_frames are
 * themselves within their limits, so that the outputs' sizes are known), checked in this order: mem kind; n_frames >= 0;
 * rows and cols in 1..8192; channels 1 or 3; step in 4..256; compactness in 0..255; iterations in 0..32; group_frames
 * >= 0; then n_frames == 0 returns O3DR_OK and touches nothing; img and labels not NULL; pitch >= cols * channels;
 * frame_stride >= rows * pitch when n_frames > 1; labels, raw_out and sizes_out 4-byte aligned.  min_size: any negative
 * value means S S / 4; 0: nothing is merged.  p == NULL: the defaults.  pitch and frame_stride have no upper limit (as in
 * o3dr_disparity_filter: a host image too large to stage returns O3DR_ERR_ALLOC).  group_frames: the frames of a call go
 * through the kernels in groups whose scratch (28 bytes a pixel, 68 bytes a centre) fits 1 GiB - one frame always forms a
 * group -; group_frames = n > 0 caps a group at n frames.  Results do not depend on it.  The number of launches of a
 * group depends on the parameters and the image's size alone, never on its content.  The call carves its own scratch
 * block, does not use the sort workspace, leaves cloud_big alone and synchronises the stream once, at its end. */
#define O3DR_SEGMENT_MAX_SIDE 8192
typedef struct o3dr_segment_params {
    int32_t channels;      /* default 3: B G R; 1: grey */
    int32_t step;          /* default 16; 4..256 */
    int32_t compactness;   /* default 20; 0..255 */
    int32_t iterations;    /* default 5; 0..32 */
    int32_t min_size;      /* default -1: step * step / 4; 0: no merging */
    int32_t group_frames;  /* default 0: as many frames per launch group as the scratch budget allows; n > 0: at most n */
} o3dr_segment_params;
typedef struct o3dr_segment_info {   /* one per frame, HOST */
    int64_t n_centres;      /* nx * ny */
    int64_t n_components;   /* components of equal raw labels */
    int64_t n_merged;       /* components that joined another one */
    int64_t n_labels;       /* final labels */
    int64_t largest;        /* pixel count of the largest label */
    int64_t smallest;       /* ... of the smallest */
} o3dr_segment_info;
void o3dr_segment_default_params(o3dr_segment_params* p);
int  o3dr_segment_image(o3dr_ctx* ctx, const uint8_t* img, int64_t frame_stride, int64_t pitch, int32_t rows, int32_t cols,
                        int32_t n_frames, const o3dr_segment_params* p, int32_t* labels, int32_t* raw_out, int32_t* sizes_out,
                        o3dr_segment_info* info, int32_t mem);

/* ---- pose chain: the reference's default mode (pose.cpp:213-235, generate_tf_of_Matched_Keypoints): every frame gets its
 * pose from descriptor matches against earlier nearby frames, whose keypoints are moved by THEIR fitted poses - a serial
 * chain.  The reference's selection rules and PCL's rounding cannot be pinned here, so the contract below is this library's
 * own; tests/pose_chain_reference.py restates it in numpy.
 *
 * Inputs.  desc ([N, 32] bytes) and kp3 (N points, index-aligned with desc: o3dr_keypoints_3d with poses = NULL; a row
 * with a NaN is a rejected keypoint) in `mem`; frame f's rows are [offsets[f], offsets[f+1]) (HOST, n_frames + 1
 * non-decreasing entries, offsets[0] >= 0: o3dr_orb_detect's offsets).  prior_poses (HOST, [n_frames, 16] fp32 row-major
 * 4x4): the recorded pose of every frame.  The first n_fixed frames are history: poses_in ([n_fixed, 16] fp32) and
 * status_in ([n_fixed] int32, each an O3DR_CHAIN_* value), both HOST, are copied to the outputs unchanged and the chain
 * starts at frame n_fixed.
 *   1. Static pair list, a function of prior_poses and the parameters alone, built on the host before any kernel runs:
 *      frame i is paired with every j < i whose prior translation (T[3], T[7], T[11], taken in fp64) lies within
 *      dist_nearby of frame i's (squared distance ((dx dx + dy dy) + dz dz) <= dist_nearby^2 in fp64); of those the
 *      range_width largest j are kept, listed in descending j.  j may be a history frame; the list of a frame does not
 *      depend on n_fixed.  The call's list holds the pairs of the frames n_fixed .. n_frames - 1, in frame order.
 *   2. Matching: one batched o3dr_match_knn2_hamming pass over that list (query set i, train set j; ratio, max_distance).
 *   3. Chain, for i = n_fixed .. n_frames - 1 in order.  No pair: O3DR_CHAIN_ANCHOR, the pose is the prior, the frame is
 *      accepted.  Else its slots are (pair, query row), pair-major in list order; a slot is used iff frame j is accepted
 *      (ANCHOR or MATCHED), the row is good, src = kp3[i][row] is finite and tgt is finite, tgt = kp3[j][train_idx[0]] moved
 *      by frame j's fp32 output pose in A2's arithmetic (fp32, ((m0 x + m1 y) + m2 z) + m3, no contraction).
 *      n_used < min_matches: O3DR_CHAIN_TOO_FEW.  Else the 16 fp64 moments of o3dr_estimate_rigid_transform step 2 about
 *      c0 = the first used tgt, summed per run of 256 consecutive slots from the frame's first slot (wave sums, the run =
 *      the tree of its four waves) and folded over the runs left to right - no float atomics; the Kabsch of step 3 (same
 *      Jacobi, same rank test, reflection corrected): rank < 2 gives O3DR_CHAIN_DEGENERATE; rms = sqrt(mean |T src -
 *      tgt|^2) in fp64 over the same partition and fold; !(rms <= max_rms): O3DR_CHAIN_RMS; else O3DR_CHAIN_MATCHED with
 *      the pose fp32(T), bottom row 0 0 0 1.  Every rejected frame (TOO_FEW, DEGENERATE, RMS) keeps its prior as its pose
 *      and is never a train frame of a later one.
 * Outputs.  poses_out ([n_frames, 16] fp32, `mem`).  frames_out (HOST, n_frames records): status; n_pairs;
 * n_pairs_accepted (pairs whose train frame is accepted); n_good (good rows over the accepted train frames); n_used; rms (the
 * fit's, also when it failed the gate; else 0); T (3 x 4 row-major fp64: the fit when MATCHED, else the frame's pose
 * widened).  A history frame's record is its status_in, its pose widened and zeros.  pairs_out (HOST, or NULL): the list as
 * int32 (query, train) frame pairs; *n_pairs_out (or NULL) = its length; pairs_capacity (in pairs) below it with pairs_out
 * given: O3DR_ERR_CAPACITY with *n_pairs_out set and nothing else written.
 * Records and poses are bit-identical across calls, across host and device memory and across any split into history and
 * new frames (feeding a call's poses and statuses back as poses_in / status_in).
 * Limits, else O3DR_ERR_INVALID_ARG (host outputs zeroed): 0 <= n_fixed <= n_frames (n_frames == 0: O3DR_OK), dist_nearby
 * finite and >= 0, 1 <= range_width <= 32, min_matches >= 3, max_rms > 0 (+inf: no gate), ratio and max_distance as in
 * o3dr_match_params, status_in within the enum, the pool at most 2^31-1 rows, a frame's slots (pairs x rows) at most
 * 2^31-1.  p == NULL: the defaults.  The call synchronises once, at its end; it does not use the sort workspace and leaves
 * cloud_big alone. */
typedef struct o3dr_chain_params {
    double  dist_nearby;    /* default 2.0 (metres; this build's own) */
    double  max_rms;        /* default +inf: no gate */
    int32_t range_width;    /* default 8; 1..32 */
    int32_t min_matches;    /* default 30; >= 3 */
    float   ratio;          /* default 0.5 */
    int32_t max_distance;   /* default 40 */
} o3dr_chain_params;
typedef struct o3dr_chain_frame {  /* 128 bytes */
    int32_t status;            /* O3DR_CHAIN_* */
    int32_t n_pairs, n_pairs_accepted;
    int32_t n_good, n_used;
    int32_t reserved;          /* 0 */
    double  rms;
    double  T[12];
} o3dr_chain_frame;
#define O3DR_CHAIN_ANCHOR     0
#define O3DR_CHAIN_MATCHED    1
#define O3DR_CHAIN_TOO_FEW    2
#define O3DR_CHAIN_DEGENERATE 3
#define O3DR_CHAIN_RMS        4
#define O3DR_CHAIN_MAX_RANGE  32
void o3dr_chain_default_params(o3dr_chain_params* p);
int  o3dr_pose_chain(o3dr_ctx* ctx, const uint8_t* desc, const int64_t* offsets, const o3dr_point* kp3, const float* prior_poses,
                     int32_t n_frames, int32_t n_fixed, const float* poses_in, const int32_t* status_in, const o3dr_chain_params* p,
                     float* poses_out, o3dr_chain_frame* frames_out, int32_t* pairs_out, int64_t pairs_capacity, int64_t* n_pairs_out,
                     int32_t mem);

/* ---- robust rigid fit: three-point RANSAC for a rigid transform, the outlier rejection in front of
 * o3dr_estimate_rigid_transform and inside the pose chain.  The contract is this library's own;
 * tests/ransac_rigid_reference.py restates it in numpy, operation for operation.
 *
 * o3dr_ransac_rigid - batched over segments.  src, tgt, seg_offsets, n_segs and mask as in o3dr_estimate_rigid_transform
 * (src / tgt / mask in `mem`, seg_offsets HOST; seg_offsets NULL: one segment [0, n) and n_segs must be 1); each segment at
 * most 2^31-1 points.  seg_keys: HOST, n_segs uint64, or NULL: segment s has the key s.  p: threshold (metres, finite, > 0),
 * iterations H (1 .. O3DR_RANSAC_MAX_ITERATIONS), seed; p == NULL: the defaults.  Per segment:
 *   1. Candidates: the pairs with mask != 0 (or no mask) whose six coordinates are finite, in ascending index; m of them.  A
 *      candidate's local index is its rank in that list.
 *   2. Sampler (that of o3dr_segment_plane): S = splitmix64(seed ^ key); draw k = 0, 1, 2 of hypothesis h = 0 .. H - 1 is
 *      r = splitmix64(S + 3 h + k) (64-bit wrap-around), local index ((r >> 32) * m) >> 32.  splitmix64(x): z = x +
 *      0x9E3779B97F4A7C15; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31).
 *   3. Hypothesis, from the drawn pairs (a_k, b_k) = (src, tgt), every coordinate widened to fp64, every operation below a
 *      single rounded fp64 operation (no contraction), IEEE division and square root.  On each side, with (p0, p1, p2) the
 *      three points: u = p1 - p0, v = p2 - p0; w = u x v = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx); uu = (ux ux + uy uy)
 *      + uz uz, vv and ww likewise; e1 = u / sqrt(uu), e3 = w / sqrt(ww) (each component divided), e2 = e3 x e1 by the same
 *      cross-product formula; centroid c = ((p0 + p1) + p2) / 3.0 per component.  With e the src side's and e' the tgt
 *      side's frame: R[i][j] = (e1'[i] e1[j] + e2'[i] e2[j]) + e3'[i] e3[j]; t[i] = c'[i] - ((R[i][0] c[0] + R[i][1] c[1]) +
 *      R[i][2] c[2]).  The hypothesis is degenerate and scores 0 if two of its local indices coincide, or if on either side
 *      ww <= (1e-12 * uu) * vv (zero-length edges included).
 *   4. Score: the number of candidates with (dx dx + dy dy) + dz dz <= threshold * threshold (the product in fp64), d[i] =
 *      (((R[i][0] x + R[i][1] y) + R[i][2] z) + t[i]) - b[i] for the candidate's src (x, y, z) and tgt b.  An exact integer.
 *   5. Winner: the greatest score, ties to the lowest h.  No early exit: all H hypotheses are evaluated.
 * Outputs.  inlier (n bytes, `mem`, index-aligned with src / tgt): 1 for the winner's inliers, 0 everywhere else
 * (non-candidates included; bytes outside every segment are not written).  res (HOST, n_segs records): T (3 x 4 row-major
 * fp64, src -> tgt: the winning hypothesis), n_candidates = m, n_inliers = the winning score, best_hypothesis = its h,
 * sample (the three drawn pairs, as indices relative to the segment's first pair, in draw order), status.
 * O3DR_RANSAC_TOO_FEW: m < 3.  O3DR_RANSAC_NO_MODEL: the best score is below 3 (every hypothesis degenerate, for one).  Both
 * leave the segment's bytes 0, T the identity, n_inliers 0, best_hypothesis and sample -1.
 * A segment's results equal those of a call on that segment alone with the same key; results are bit-identical across
 * calls, batchings and memory kinds.  Limits, else O3DR_ERR_INVALID_ARG with the host outputs zeroed: the threshold, the
 * iteration count, the segment list.  The call synchronises once, at its end; it does not use the sort workspace and leaves
 * cloud_big alone.
 *
 * o3dr_pose_chain_robust - o3dr_pose_chain with that filter per pair of the static list.  rp == NULL: no filter, byte for
 * byte o3dr_pose_chain (which is this call with rp = NULL, ransac_out = NULL).  Else, between the matching (step 2) and the
 * chain (step 3), every pair (i, j) of the call's list is one segment of the contract above: its positions are the query
 * rows of frame i, src = kp3[i][row], tgt = kp3[j][train_idx[0]] - both in camera coordinates: whether a correspondence fits
 * a rigid model does not change when the target set is moved rigidly, so no pose is needed -, candidates = the good rows
 * with both points finite, key = ((uint64)i << 32) | j with i, j the frame numbers: it does not depend on where the pair
 * stands in the call's list, so the split into history and new frames stays bit-identical.  Every pair goes through it,
 * whether or not frame j ends up accepted.  In step 3 a slot is used iff o3dr_pose_chain's conditions hold AND its pair's
 * inlier byte is 1; n_good keeps its meaning, n_used and everything after it see the filtered set; reserved stays 0.
 * ransac_out (HOST, or NULL): one o3dr_ransac_result per pair of the list, in list order (at least *n_pairs_out records:
 * size it like pairs_out); sample holds query rows.  Its length is an output of the call, so an error does not zero it; it
 * is written by a successful call only, and ignored when rp == NULL. */
typedef struct o3dr_ransac_params {
    double   threshold;     /* default 0.05 (metres) */
    uint64_t seed;          /* default 0 */
    int32_t  iterations;    /* default 256; 1 .. 65536 */
    int32_t  reserved;      /* 0 */
} o3dr_ransac_params;
typedef struct o3dr_ransac_result {  /* 128 bytes */
    double  T[12];
    int32_t n_candidates, n_inliers;
    int32_t best_hypothesis;
    int32_t sample[3];
    int32_t status;         /* O3DR_RANSAC_* */
    int32_t reserved;       /* 0 */
} o3dr_ransac_result;
#define O3DR_RANSAC_OK       0
#define O3DR_RANSAC_TOO_FEW  1
#define O3DR_RANSAC_NO_MODEL 2
#define O3DR_RANSAC_MAX_ITERATIONS 65536
void o3dr_ransac_default_params(o3dr_ransac_params* p);
int  o3dr_ransac_rigid(o3dr_ctx* ctx, const o3dr_point* src, const o3dr_point* tgt, int64_t n, const int64_t* seg_offsets,
                       int32_t n_segs, const uint8_t* mask, const uint64_t* seg_keys, const o3dr_ransac_params* p, uint8_t* inlier,
                       o3dr_ransac_result* res, int32_t mem);
int  o3dr_pose_chain_robust(o3dr_ctx* ctx, const uint8_t* desc, const int64_t* offsets, const o3dr_point* kp3, const float* prior_poses,
                            int32_t n_frames, int32_t n_fixed, const float* poses_in, const int32_t* status_in,
                            const o3dr_chain_params* p, float* poses_out, o3dr_chain_frame* frames_out, int32_t* pairs_out,
                            int64_t pairs_capacity, int64_t* n_pairs_out, int32_t mem, const o3dr_ransac_params* rp,
                            o3dr_ransac_result* ransac_out);

/* ---- pose graph: one joint least-squares refinement of the pose chain's accepted frames over all pairs at once.  The chain
 * (above) fits frame i once, against earlier frames, and never moves it again; here every pair pulls on both of its frames.
 * The contract is this library's own; tests/pose_graph_reference.py restates it in numpy, DESIGN.md "Pose-graph refinement"
 * derives the formulas.
 *
 * Inputs.  desc, offsets, kp3, n_frames and mem as in o3dr_pose_chain.  poses_in (HOST, [n_frames, 16] fp32) and status_in
 * (HOST, [n_frames] O3DR_CHAIN_* values): a chain call's outputs.  fixed (HOST, [n_frames] bytes, or NULL: none): a non-zero
 * byte holds the frame.  prior_poses (HOST, [n_frames, 16] fp32, or NULL): required iff prior_weight > 0; only its
 * translations are used.  pairs (HOST, n_pairs int32 (i, j) frame pairs, i != j, any order, no pair twice - (i, j) and (j, i)
 * are different pairs): o3dr_pose_chain's pairs_out goes straight in.  rp: NULL, or the filter of o3dr_pose_chain_robust.
 *   1. Matching: one batched o3dr_match_knn2_hamming pass over `pairs` (query set i, train set j; ratio, max_distance); with
 *      rp every pair then goes through the RANSAC of o3dr_pose_chain_robust, key ((uint64)i << 32) | j.
 *   2. Pair moments.  A query row of pair (i, j) is used iff both frames are accepted (ANCHOR or MATCHED), the row is good,
 *      a = kp3[i][row] and b = kp3[j][train_idx[0]] are finite and, with rp, the inlier byte is set.  Both points stay in
 *      camera coordinates.  Per pair 28 fp64 sums, no contraction: n, sum a (3), sum b (3), sum a a^T (xx xy xz yy yz zz),
 *      sum b b^T (6), sum a b^T (9, row-major), over runs of 256 consecutive rows from the pair's first (wave sums, the run =
 *      the tree of its four waves), the runs folded left to right - no float atomics.  n_good = the pair's good rows
 *      (whatever the statuses), n_used = the used rows.  A pair is an edge iff both frames are accepted and n_used >=
 *      min_pair_matches.  An edge's moments equal those of a call with that pair alone.
 *   3. Roles (host).  degree = the edges a frame is part of.  A frame is O3DR_REFINE_FREE iff it is MATCHED, not fixed and
 *      degree > 0; a rejected frame (TOO_FEW, DEGENERATE, RMS) is O3DR_REFINE_REJECTED; every other frame is
 *      O3DR_REFINE_FIXED, and holds the gauge where degree > 0.  With prior_weight == 0 the free frames of a connected
 *      component (over the edges) without a gauge frame become O3DR_REFINE_FLOATING: held, and reported.
 *   4. Solve, one launch of one workgroup.  State (R, t) per frame in fp64: t = (m3, m7, m11) of the fp32 pose, R its rows
 *      0..2 orthonormalised once: e1 = r1 / |r1|, u = r2 - (r2 . e1) e1, e2 = u / |u|, e3 = e1 x e2.  Energy
 *        E = sum_edges sum_k |R_i a + t_i - R_j b - t_j|^2 + prior_weight sum_free |t_i - prior_t_i|^2,
 *      evaluated from the moments.  gn_iterations Gauss-Newton steps, all of them always: the 6 x 6 blocks and gradient
 *      halves of every edge in the right perturbation R <- R C(w), t <- t + R v; per frame the diagonal block and g summed
 *      over its (edge, side) list in pair order; each diagonal block inverted by Cholesky; exactly cg_iterations steps of
 *      block-Jacobi preconditioned CG on H x = -g over the free frames from x = 0 (a dot product: thread t of 256 sums the
 *      entries t, t + 256, .. in ascending order, wave sums, then (w0 + w1) + (w2 + w3)); p^T H p <= 0 or a non-finite
 *      scalar stops that solve with what it has and sets O3DR_REFINE_FLAG_CG_STOPPED (a gradient that is exactly zero does
 *      so too); a diagonal block that is not positive definite holds its frame for that step and sets
 *      O3DR_REFINE_FLAG_SINGULAR; then every free frame is retracted, C(w) = the rotation of the unit quaternion
 *      (1, w / 2) / |.|.  Only + - * / sqrt.
 * Outputs.  poses_out ([n_frames, 16] fp32, `mem`): fp32(R | t) with the bottom row 0 0 0 1 for a free frame, the 64 bytes
 * of poses_in for every other.  frames_out (HOST, n_frames records): role, degree, T (3 x 4 row-major fp64: the state of a
 * free frame, else the input pose widened).  edges_out (HOST, n_pairs records, or NULL): n_good, n_used, edge (0 / 1), the
 * edge's energy at the input and at the output poses (0 for a pair that is no edge).  res (HOST): energy_before /
 * energy_after; grad_before / grad_after = the 2-norm of g over the free frames at the input / output poses; last_step =
 * max |x| of the last iteration; n_free, n_gauge (FIXED frames with degree > 0), n_floating, n_rejected, n_edges, n_used
 * (over the edges), flags.  No free frame or no edge: O3DR_OK, the poses are copied, energy_after == energy_before.
 * Results are bit-identical across calls and across host and device memory.
 * Limits, else O3DR_ERR_INVALID_ARG (host outputs and *res zeroed): 1 <= gn_iterations <= 64, 1 <= cg_iterations <= 1024,
 * min_pair_matches >= 1, prior_weight finite and >= 0, prior_poses given when prior_weight > 0, ratio and max_distance as in
 * o3dr_match_params, rp as in o3dr_ransac_rigid, status_in within the enum, pair indices within [0, n_frames), i != j, no
 * pair twice, the pool at most 2^31-1 rows; n_frames == 0: O3DR_OK.  p == NULL: the defaults.  The call synchronises twice:
 * after the per-pair counts and at its end; it does not use the sort workspace and leaves cloud_big alone. */
typedef struct o3dr_refine_params {
    double  prior_weight;      /* default 0: no prior */
    int32_t gn_iterations;     /* default 5; 1..64 */
    int32_t cg_iterations;     /* default 32; 1..1024 */
    int32_t min_pair_matches;  /* default 3; >= 1 */
    float   ratio;             /* default 0.5 */
    int32_t max_distance;      /* default 40 */
    int32_t reserved;          /* 0 */
} o3dr_refine_params;
typedef struct o3dr_refine_frame {  /* 104 bytes */
    int32_t role;              /* O3DR_REFINE_* */
    int32_t degree;
    double  T[12];
} o3dr_refine_frame;
typedef struct o3dr_refine_edge {  /* 32 bytes */
    int32_t n_good, n_used;
    int32_t edge;              /* 1: the pair is an edge */
    int32_t reserved;          /* 0 */
    double  energy_before, energy_after;
} o3dr_refine_edge;
typedef struct o3dr_refine_result {  /* 72 bytes */
    double  energy_before, energy_after;
    double  grad_before, grad_after;
    double  last_step;
    int64_t n_used;
    int32_t n_free, n_gauge, n_floating, n_rejected;
    int32_t n_edges;
    int32_t flags;             /* O3DR_REFINE_FLAG_* */
} o3dr_refine_result;
#define O3DR_REFINE_FIXED    0
#define O3DR_REFINE_FREE     1
#define O3DR_REFINE_FLOATING 2
#define O3DR_REFINE_REJECTED 3
#define O3DR_REFINE_FLAG_CG_STOPPED 1
#define O3DR_REFINE_FLAG_SINGULAR   2
#define O3DR_REFINE_MAX_GN 64
#define O3DR_REFINE_MAX_CG 1024
void o3dr_refine_default_params(o3dr_refine_params* p);
int  o3dr_pose_graph_refine(o3dr_ctx* ctx, const uint8_t* desc, const int64_t* offsets, const o3dr_point* kp3, int32_t n_frames,
                            const float* poses_in, const int32_t* status_in, const uint8_t* fixed, const float* prior_poses,
                            const int32_t* pairs, int64_t n_pairs, const o3dr_refine_params* p, const o3dr_ransac_params* rp,
                            float* poses_out, o3dr_refine_frame* frames_out, o3dr_refine_edge* edges_out, o3dr_refine_result* res,
                            int32_t mem);

/* ---- measurement hooks (bench.py; not part of the reference surface) ------------------------ */
/* kernel ids for o3dr_profile_* */
#define O3DR_K_COUNT        0  /* grid-pass valid count per tile */
#define O3DR_K_REPROJECT    1  /* fused reproject + SE(3) + ordered compaction */
#define O3DR_K_KEYGEN       2  /* voxel linear index per point */
#define O3DR_K_SORT_HIST    3  /* radix digit histogram */
#define O3DR_K_SORT_SCATTER 4  /* radix stable scatter */
#define O3DR_K_SEGMENT      5  /* voxel run heads + counts */
#define O3DR_K_CENTROID     6  /* ordered per-voxel sums -> centroid */
#define O3DR_K_OTHER        7  /* scans, grid setup, copies */
#define O3DR_K_CENTROID_RUNS 8 /* ordered per-voxel sums over group runs of points, one wave per voxel group (whole-cloud calls) */
#define O3DR_K_PLANE_DISP_SUMS 9   /* plane-fitted disparity: per-(frame, label) integer sums */
#define O3DR_K_PLANE_DISP_FIT  10  /* ... the fp64 fit of every (frame, label) */
#define O3DR_K_PLANE_DISP_EVAL 11  /* ... the f64 image */
#define O3DR_K_ORB_PYRAMID    12  /* ORB: grey + pyramid levels */
#define O3DR_K_ORB_FAST       13  /* ... FAST score map + 5 x 5 box sums */
#define O3DR_K_ORB_CANDIDATES 14  /* ... suppression, margin, Harris response, ordered compaction */
#define O3DR_K_ORB_SELECT     15  /* ... radix select of the cut per (frame, level), output offsets */
#define O3DR_K_ORB_DESCRIBE   16  /* ... orientation + steered BRIEF, one wave per keypoint */
#define O3DR_K_MATCH          17  /* Hamming 2-NN: chunk scans + fold (o3dr_match_knn2_hamming, o3dr_pose_chain) */
#define O3DR_K_POSE_CHAIN     18  /* pose chain: the one-workgroup walk over the frames */
#define O3DR_K_RANSAC         19  /* three-point RANSAC for a rigid transform, one workgroup per segment (o3dr_ransac_rigid, o3dr_pose_chain_robust) */
#define O3DR_K_GRAPH_MOMENTS 20  /* pose graph: the 28 fp64 moments of every pair, one workgroup per pair */
#define O3DR_K_GRAPH_SOLVE   21  /* ... Gauss-Newton + preconditioned CG, the one-workgroup solve */
#define O3DR_K_STEREO_CENSUS 22  /* stereo disparity: grey + census of both images */
#define O3DR_K_STEREO_PATHS  23  /* ... the aggregation, one launch per direction, one wave per scan line */
#define O3DR_K_STEREO_WINNER 24  /* ... winners of left and right pixels, rejections, outputs */
#define O3DR_K_DISP_MEDIAN  25  /* disparity filter: the k x k median */
#define O3DR_K_DISP_LABEL   26  /* ... components: tile labelling in LDS, border merge, flatten + sizes */
#define O3DR_K_DISP_SPECKLE 27  /* ... removal of the small components and the per-frame counts */
#define O3DR_K_RECTIFY_MAPS  28  /* stereo rectification: the Q5 map of one camera, one thread per pixel */
#define O3DR_K_RECTIFY_REMAP 29  /* ... the bilinear remap of a group of frames through one map */
#define O3DR_K_SEG_ASSIGN   30  /* image segmentation: seeds, the K + 1 assignments with their tile sums, the updates */
#define O3DR_K_SEG_LABEL    31  /* ... components, merge of the small ones, ordered numbering, outputs */
#define O3DR_K_MULTIVIEW    32  /* multi-view filter and fusion: the one launch of a call */
#define O3DR_K_GROUND_WINNER 33  /* ground filter (o3dr_terrain.h): the minimum surface */
#define O3DR_K_GROUND_ITER   34  /* ... the iterations: four sliding min / max passes each */
#define O3DR_K_GROUND_FILL   35  /* ... the DTM: ground words, the raster's fill passes */
#define O3DR_K_GROUND_POINTS 36  /* ... the pass over the points: mask, height above ground */
#define O3DR_K_CLUSTER_LINK    37  /* Euclidean clustering (o3dr_objects.h): the radius walk with its union-find */
#define O3DR_K_CLUSTER_NUMBER  38  /* ... flatten, sizes, flags, the two scans */
#define O3DR_K_CLUSTER_RECORDS 39  /* ... point outputs, boxes, centroid sums, records, indices */
#define O3DR_K_INTERP_PULL   40  /* raster interpolation (o3dr_dem.h): the tiled pull launches and the one-workgroup top of the pyramid */
#define O3DR_K_INTERP_PUSH   41  /* ... the tiled push launches with their sweeps, the outputs, the counters' fold */
#define O3DR_K_RASTER_SAMPLE 42  /* raster sample (o3dr_dem.h): the pass over the points */
#define O3DR_K_NUM          43
/* Bracket every launch of kernel `kernel_id` (or all kernels if -1) with HIP events on the
 * context's stream; 0 launches are bracketed when disabled (the default). */
int o3dr_profile_enable(o3dr_ctx* ctx, int32_t kernel_id, int32_t enable);
/* Synchronises; total milliseconds and launch count of `kernel_id` since enable/reset. */
int o3dr_profile_read(o3dr_ctx* ctx, int32_t kernel_id, double* total_ms, int64_t* launches);
int o3dr_profile_reset(o3dr_ctx* ctx);
/* Synchronises; counters since the last o3dr_profile_reset, for algorithmic-byte accounting:
 * out[0] = sum over voxel grids of (records x radix passes actually run), out[1] = points that entered
 * voxel grids, out[2] = points that left them, out[3] = 0, out[4] = records that entered the sorts (points or runs
 * of points), out[5] = records whose run-head flag the last scatter pass of their sort wrote (in place of the sorted index
 * and of the run-head pass over it: the point sorts of the voxel grids), out[6..7] = 0. */
int o3dr_profile_stats(o3dr_ctx* ctx, int64_t out[8]);
/* device name / arch / CU count of the context's device, for bench headers */
int o3dr_device_info(o3dr_ctx* ctx, char* name, int32_t name_len, int32_t* cu_count, int64_t* hbm_bytes);

#ifdef __cplusplus
}
#endif
#endif /* O3DR_H */
