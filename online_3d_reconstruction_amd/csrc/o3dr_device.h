// o3dr_device.h — device-side data structures and kernel launchers shared by the C-ABI layer.
// gfx950 only (64-wide wavefronts are assumed throughout).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/o3dr.h"
#include "../../include/o3dr_contour.h"
#include "../../include/o3dr_dem.h"
#include "../../include/o3dr_objects.h"
#include "../../include/o3dr_terrain.h"
#include "o3dr_rigid_solve.h"

namespace o3dr {

// ---- tiling constants -------------------------------------------------------------------------
constexpr int kWave = 64;
// reprojection: one 256-thread workgroup covers 1024 grid-pass candidates (4 per lane)
constexpr int kEmitThreads = 256;
constexpr int kEmitPerLane = 4;
constexpr int kEmitTile = kEmitThreads * kEmitPerLane;
// radix sort: 8 waves x 16 records per lane x 64 lanes = 8192 records per workgroup
constexpr int kSortWaves = 8;
constexpr int kSortThreads = kSortWaves * kWave;
constexpr int kSortRounds = 16;
constexpr int kSortWaveItems = kSortRounds * kWave;
constexpr int kSortTile = kSortWaves * kSortWaveItems;
// the scatter takes a tile in kScatParts parts, one workgroup of kScatWaves waves each (k_radix_scatter_lane): more and
// smaller workgroups per CU overlap their LDS phases better; the histograms keep the 8192-record tile
constexpr int kScatParts = 2;
constexpr int kScatWaves = kSortWaves / kScatParts;
constexpr int kScatThreads = kScatWaves * kWave;
constexpr int kScatTile = kScatWaves * kSortWaveItems;
// emit tiles per sort tile: a KEYS workgroup of k_reproject_emit walks that many, and the first radix pass of the fused
// batch path sorts over tiles cut at those candidate borders (emit_part_range in kernels/radix_sort.inc)
constexpr int kEmitGroup = kSortTile / kEmitTile;
static_assert(kEmitGroup * kEmitTile == kSortTile && kEmitGroup % kScatParts == 0, "a scatter part is a whole number of emit tiles");
constexpr int kMaxRadixBits = 7;           // digits are 1..7 bits wide, chosen per frame (k_voxel_geom).  Measured with
                                          // the ballot scatter: 7-bit passes 3.8 TB/s, 10-bit ones 2.5 TB/s (32-byte
                                          // output runs); the lane-counting scatter keeps 128 x 17 counters per wave
constexpr int kMaxRadix = 1 << kMaxRadixBits;
constexpr int kMaxPasses = 5;            // 5 x 7 bits covers a full 32-bit index
static_assert(kMaxRadix <= 2 * kSortThreads, "k_radix_scatter handles two digits per thread");
// bytes between the frames of Workspace::side (one byte per record): frames start on 16-byte boundaries
static inline int64_t side_frame_stride(int64_t cap) { return (cap + 15) & ~(int64_t)15; }
// generic per-point kernels
constexpr int kSlabClasses = 4;  // layout classes inside an emit tile of the fused batch path (slab_class)
constexpr int kXcds = 8;   // accelerator complex dies of an MI355X, each with its own L2 (xcd_chunk_item)
constexpr int kPtThreads = 256;
constexpr int kSegTile = 1024;  // sorted keys per workgroup in the run-head kernels
constexpr int kMinmaxBlocks = 1024;  // workgroups (= bounding-box slots) of the stand-alone min/max pass
constexpr int kPartWords = 8;  // words per workgroup partial of the whole-cloud integer reductions (k_fold4_u32 in kernels/util.inc)
constexpr int kSmallMax = 8192;      // points one workgroup takes through the whole path in one launch (kernels/small.inc)
// whole-cloud voxel grids (the merge): records of the sort are runs of consecutive points inside one GROUP of
// 2^kGroupBits consecutive voxel indices; one wave then sums a group, lane = voxel (k_centroid_groups)
constexpr int kGroupBits = 5;
constexpr int kGroupCells = 1 << kGroupBits;
static_assert(kGroupCells <= kWave, "one lane per voxel of a group");
constexpr int kGroupWaves = 4;            // groups per workgroup of k_centroid_groups
// grouped records are used when the runs average at least kGroupMinRunNum / kGroupMinRunDen points.  Round 4 measured the
// break-even again (round 2 had set 8): forced on BASELINE configs[4]'s shape (4.1 points per run) 9.03 -> 6.94 ms per
// 200-frame step, on configs[3]'s (raw pixel-order points, 1.6 per run) 9.49 -> 7.75 ms - the run sort moves fewer
// records and k_centroid_groups reads the cloud once, coalesced, where k_centroid gathers 16 bytes per 64-byte sector
constexpr int kGroupMinRunNum = 5, kGroupMinRunDen = 4;
constexpr int64_t kGroupMinCloud = 1 << 20;  // whole-cloud calls on fewer points sort the points
constexpr int64_t kGroupMinSlots = 1 << 20;  // result slots (16 bytes each) a context always has for the grouped path

// ---- per-frame voxel grid geometry (PCL VoxelGrid members), written by k_voxel_geom -----------
struct VoxelGeom {
    float inv[3];       // inverse_leaf_size_
    int32_t min_b[3];   // min_b_
    int32_t div_b[3];   // div_b_
    uint32_t mul1, mul2;  // divb_mul_[1], divb_mul_[2]
    uint32_t overflow;    // dx*dy*dz > INT32_MAX  -> output = input
    uint32_t n;           // points in this frame
    uint32_t passes;      // radix passes this frame's index needs (0 when overflow)
    uint32_t bpp;         // bits per pass
    uint32_t buf0;        // buffer the first pass reads (sorted records end in buffer (passes + buf0) & 1)
    uint32_t grouped;     // 1: the records are runs of consecutive points of one voxel group (n = number of records, payload =
                          // record id into Workspace::run_start); 0: the records are the points (payload = point id)
};

// ---- statistical outlier removal (A3b): search grid + threshold, written by k_sor_plan / k_sor_threshold ----
constexpr int kSorMeanK = 50;  // sor0.setMeanK(50), pose_functions.cpp:1681
#ifndef O3DR_SOR_CELLPTS
#define O3DR_SOR_CELLPTS 30.0
#endif
constexpr double kSorCellPoints = O3DR_SOR_CELLPTS;  // points per column of the search grid, on average
struct SorGeom {
    float mnx, mny, inv_h, h;
    int32_t gx, gy;
    uint32_t n, active;
    double threshold;
};
// ---- the XY search grid of one cloud, as a kernel sees it (by value).  launch_nn_grid builds and returns it; SOR's own
// search kernels read the same arrays of a batch of clouds through Workspace::grid_*. ----
struct SearchGrid {
    const SorGeom* geom;         // the plan (n == 0 or inactive: no points)
    const float4* xyz;           // points in cell order, .w = original index bits
    const uint32_t* cell_first;  // cells + 1: exclusive scan of the populations
    const float4* cell_lo;       // exact box of every cell's points (k_nn_cell_box)
    const float4* cell_hi;
    const float* box6;           // the cloud's box, min xyz then max xyz
};
// the grid never has more cells than points / 2 (at least 1024, at most 2^22): it is only a search structure, and the cell
// ids of clouds of at most `cap` points then need few sort passes
inline uint32_t search_grid_max_cells(int64_t cap)
{
    const int64_t cells = cap / 2 > 1024 ? cap / 2 : 1024;
    return (uint32_t)(cells < (1 << 22) ? cells : (1 << 22));
}
// half the side of the box whose cells a radius walk visits (grid_radius_walk, kernels/util.inc): max(r (1 + 1e-5), 1e-18)
inline float grid_pad_radius(double r)
{
    const double pad = r * (1.0 + 1e-5);
    return (float)(pad > 1e-18 ? pad : 1e-18);
}

// disparity-byte table of the rectified-stereo fast path: alpha = 1./(Q[14]*d + Q[15]), z = float(t2*alpha + 0)
struct QLutEntry {
    double alpha;
    float z, pad;
};

// ---- arguments of the fused reprojection kernels (A1 + A2) ------------------------------------
struct ReprojectArgs {
    const uint8_t* disp;  // frame f at disp + f*disp_fstride
    const uint8_t* bgr;
    int64_t disp_pitch, bgr_pitch, disp_fstride, bgr_fstride;
    const float* poses;   // xf_mode 2: 16 floats per frame (row-major) in HBM
    int32_t xf_mode;      // 0: camera frame (A1 only); 1: T below (single frame); 2: poses[f]
    float T[12];          // top three rows of the 4x4 pose, row-major
    int32_t rows, cols, bb, cs, jump;
    int32_t Ny, Nx;       // grid-pass extent
    int32_t n_tiles;      // ceil(Ny*Nx / kEmitTile)
    int32_t vec4;         // 1: jump==1, Nx%4==0, cs%4==0, pitches%4==0 -> packed 4-pixel loads
    double Q[16];
    double min_disp;
    int32_t min_disp_u8;  // for disparity BYTES: d > min_disp  <=>  (int)d > min_disp_u8 (set next to min_disp)
    int64_t out_fstride;  // points between consecutive frames' output regions
    int64_t mm_stride;    // bounding-box slots per frame
    const QLutEntry* lut; // 256 entries in HBM when Q has the rectified-stereo sparsity, else nullptr
    int32_t disp_f64;     // disparity image holds doubles (CV_64F, --use_segment_labels) instead of bytes
    // fused batch path only: the points of an emit tile are written class by class (grid slabs, see slab_class)
    float slab_inv[3];    // inverse leaf of the grid the points are meant for
    int32_t slab_shift;   // log2 of the slab thickness in cells; < 0: one class, plain pixel order
};

// All per-batch device buffers.  Sizes are for `frames` frames of at most `cap` points each.
struct Workspace {
    int32_t frames = 0;
    int64_t cap = 0;
    int32_t n_emit_tiles = 0, n_sort_tiles = 0, n_seg_tiles = 0;
    o3dr_point* pts = nullptr;     // frames*cap       transformed points (A1+A2 output)
    uint32_t* keys[2] = {nullptr, nullptr};  // frames*cap ping-pong
    uint32_t* vals[2] = {nullptr, nullptr};  // frames*cap ping-pong
    uint32_t* seg_start = nullptr; // frames*(cap+1)   start of each voxel run in the sorted order
    uint32_t* tile_cnt = nullptr;  // frames*n_emit_tiles
    uint32_t* hist = nullptr;      // frames*kMaxRadix*n_sort_tiles
    uint32_t* hist_part = nullptr; // frames*kMaxRadix*n_sort_tiles: digit counts of the FIRST scatter part of every tile
    uint32_t* seg_cnt = nullptr;   // frames*n_seg_tiles (run heads per tile, then kept runs per tile)
    uint8_t* head_bits = nullptr;  // frames*n_seg_tiles*256: run-head flags, 4 records per byte (k_run_heads -> k_run_starts)
    uint8_t* side = nullptr;       // frames*side_frame_stride(cap): one byte per record of a point sort, 1 = starts a run of equal
                                   // indices, written by the last scatter pass instead of the sorted indices (k_radix_scatter_lane
                                   // -> k_run_heads packs them); nullptr: the indices are written and k_run_heads compares them
    uint32_t* scan_partial = nullptr;  // chunk sums of the multi-workgroup scan
    // the search grids of `frames` clouds (grid_ensure; SearchGrid above is one cloud's, with its cells' boxes)
    SorGeom* grid_geom = nullptr;        // frames
    float4* grid_xyz = nullptr;          // frames*cap      coordinates in cell order
    uint32_t* grid_cell_first = nullptr; // frames*(grid_max_cells+1): points in cells below c (exclusive scan of the populations)
    float2* sor_cell_z = nullptr;        // frames*(grid_max_cells+1): z range of every cell's points (SOR's handed-over queries;
                                         // carved with the grid, whose cell stride it shares)
    uint32_t grid_max_cells = 0;
    // statistical outlier removal (sor_ensure)
    float* sor_dist = nullptr;          // frames*cap      mean neighbour distance per point
    double* sor_partial = nullptr;      // frames*256*2
    o3dr_point* sor_pts = nullptr;      // frames*cap      inliers
    uint32_t* sor_n = nullptr;          // frames          inlier count
    uint32_t* sor_left = nullptr;       // frames*cap      queries (cell-sorted index) left to k_sor_knn_left
    uint32_t* sor_left_cnt = nullptr;   // frames
    uint32_t* keep_idx = nullptr;  // frames*cap  (only when min_points > 1)
    uint32_t* run_start = nullptr; // frames*(cap+1)  first point of every group run (grouped path), + sentinel
    uint32_t* grp_cnt = nullptr;   // grp_slots/64 + 2: output voxels per group -> exclusive prefix (grouped path, frames == 1)
    int64_t grp_slots = 0;         // 16-byte result slots available in `pts` for the grouped path (0: pts not reserved)
    uint32_t* n_runs = nullptr;    // frames
    uint32_t* n_grp_out = nullptr; // frames: output voxels of a grouped cloud
    VoxelGeom* geom_runs = nullptr;  // frames: geom with n = number of group runs, records starting in buffer 1
    float* out_mm = nullptr;         // frames*ceil(cap/256)*4*6: bounding boxes of what k_centroid's waves appended
    float* out_mm_partial = nullptr; // kBoxFoldBlocks*6
    int32_t* wave_gc = nullptr;      // frames*ceil(cap/256)*4*6: voxel groups of the first / last point k_centroid's waves appended
    float* mm = nullptr;           // frames*mm_stride*6  per-workgroup bounding boxes (min xyz, max xyz)
    int64_t mm_stride = 0;         // slots per frame
    uint32_t* n_valid = nullptr;   // frames     points per frame after A1
    uint32_t* n_kp = nullptr;      // frames     keypoint-pass points (single-frame API), else 0
    uint32_t* n_vox = nullptr;     // frames     voxel runs
    uint32_t* n_out = nullptr;     // frames     output points (kept runs, or n_valid on overflow)
    uint64_t* out_off = nullptr;   // frames     absolute output offset of each frame
    VoxelGeom* geom = nullptr;     // frames
    size_t bytes = 0;
};

// device-resident statistics for bench.py's byte accounting
struct SortStats {
    uint64_t sort_record_passes;  // sum over voxel jobs of points * radix passes
    uint64_t voxel_points_in;     // points entering voxel grids (not counting overflow/passthrough)
    uint64_t voxel_points_out;    // points leaving them
    uint64_t reserved;
    uint64_t sort_records;        // records entering the sorts (points, or runs of points)
    uint64_t side_head_records;   // records whose run-head flag the last scatter pass wrote (no sorted indices, no k_run_heads pass)
    uint64_t pad[2];
};

// where cloud_big records the heads of its group runs while it is appended to (k_centroid): the flags (4 records per
// byte, see k_run_heads) and the merge grid they are meant for
struct CloudHeads {
    uint32_t* flags;  // nullptr: not recorded
    float inv[3];     // inverse leaf of the merge's grid
    float z_offset;
    int32_t* wave_gc; // workspace: groups of the first and the last point every wave of k_centroid appended (6 ints per wave)
};

// device-resident counters of the accumulating cloud
struct CloudCounters {
    uint64_t count;     // points in cloud_big / in the current output buffer
    uint32_t status;    // OR of O3DR_STATUS_* bits
    uint32_t pad;
};

// ---- incremental merge state (o3dr_finalize_incremental, kernels/incremental.inc) --------------------------------------
// an occupied voxel group of the combined grid: ABSOLUTE coordinates (block of kGroupCells cells along x, row, layer) and
// which of its cells are occupied; the state keeps them sorted by (iz, iy, bx) = ascending linear voxel index
struct IncGroup {
    int32_t bx, iy, iz;
    uint32_t mask;
};
// an occupied cell: CentroidPoint's seven running fp32 sums (x, y, z + z_offset, r, g, b, a) and its point count
struct IncCell {
    float s[7];
    uint32_t n;
};
static_assert(sizeof(IncCell) == 32, "32-byte cell records");

// ---- launchers (o3dr_kernels.hip).  All are asynchronous on `s`. -------------------------------
struct Profiler;  // o3dr_api.hip

void launch_minmax_init(Profiler* pf, hipStream_t s, float* mm, int64_t mm_stride, int slot, uint32_t* n_kp, int frames);
// keypoint pass of `frames` frames (one workgroup each); kp_off = nullptr: a single frame with n_kp keypoints
void launch_keypoint_pass(Profiler* pf, hipStream_t s, const ReprojectArgs& a, const float* kp_xy, int n_kp,
                          o3dr_point* out, uint32_t* n_kp_out, float* mm, const int32_t* kp_off = nullptr, int frames = 1);
void launch_reproject(Profiler* pf, hipStream_t s, const ReprojectArgs& a, int frames, o3dr_point* out,
                      uint32_t* tile_cnt, const uint32_t* n_kp, uint32_t* n_valid, float* mm,
                      uint32_t* scan_partial);
// A1 + A2 of a batch with the per-frame grid's index produced in the same pass over the pixels as the points
// (bounding boxes and counts first, then PCL's geometry, then the points): for launch_voxel_grid with
// v.keys_ready = 1.  No keypoint pass (n_kp must hold zeros).  Returns what v.emit_tiles must be set to: the emit tiles
// per frame when the pass also counted the digits of the first radix pass (over candidate-aligned sort tiles, whose record
// ranges are the scanned counts it leaves in ws.tile_cnt), else 0.
int launch_reproject_fused(Profiler* pf, hipStream_t s, Workspace& ws, const ReprojectArgs& a, int frames, int64_t cap,
                            const float leaf[3], bool conservative_box = true);
// ... whose first pass also does launch_minmax_init's job (neutral keypoint slot, ws.n_kp = 0) for these arguments: the
// caller then leaves that launch out
bool reproject_fused_inits(const ReprojectArgs& a, bool conservative_box);
void launch_transform(Profiler* pf, hipStream_t s, const o3dr_point* in, int64_t n, const float* T16_host,
                      o3dr_point* out);
int launch_points_minmax(Profiler* pf, hipStream_t s, const o3dr_point* in, int64_t in_fstride,
                         const uint32_t* n_dev, int frames, int64_t cap, int64_t mm_stride, float* mm);
// voxel grid over `frames` independent clouds (cloud f = in + f*in_fstride, n_dev[f] points);
// results are appended at out_base[cc->count + ...] in frame order and cc->count is advanced.
struct VoxelArgs {
    const o3dr_point* in = nullptr;
    int64_t in_fstride = 0;
    const uint32_t* n_dev = nullptr;
    int frames = 0;
    int64_t cap = 0;
    float leaf[3] = {0.f, 0.f, 0.f};
    uint32_t min_points = 0;
    float z_offset = 0.f;
    o3dr_point* out_base = nullptr;
    CloudCounters* cc = nullptr;
    int passthrough = 0;  // dont_downsample: append the input unchanged
    int mm_used = 0;      // bounding-box slots to fold per frame
    SortStats* stats = nullptr;  // optional device statistics
    int use_runs = 0;     // whole-cloud calls (frames == 1): sort runs of consecutive points of one voxel group instead of points
                      // when they are long enough (decided on the device; 2: whenever the result slots allow it); needs
                      // ws.grp_slots result slots in ws.pts, which must not be the input
    float* cloud_box = nullptr;  // device, 6 floats: running bounding box of out_base's cloud, extended by this call
    CloudHeads cloud_heads = {nullptr, {0.f, 0.f, 0.f}, 0.f, nullptr};  // appending to cloud_big: record the group-run heads of what is appended
    const uint8_t* heads_in = nullptr;  // whole-cloud call on a cloud whose group-run heads are recorded already (for this leaf)
    int keys_ready = 0;  // launch_reproject_fused ran: ws.geom and the indices in ws.keys[0] exist
    int emit_tiles = 0;  // ... and it returned this: the first radix pass's histograms exist too (ws.hist, ws.hist_part)
    int test_corrupt = 0;  // o3dr_test_corrupt_next_gather: poison one sorted payload before the gather (guard test)
};
constexpr int kBoxFoldBlocks = 1024;  // workgroups (and partial boxes) of the running-bounding-box fold
void launch_voxel_grid(Profiler* pf, hipStream_t s, Workspace& ws, const VoxelArgs& v);
void launch_set_counts(Profiler* pf, hipStream_t s, uint32_t* n_dev, uint32_t value, int frames);
// Small clouds (at most kSmallMax points) in ONE launch of ONE workgroup (kernels/small.inc).
//  launch_small_frame: A1 (+ A2 by a.xf_mode) of one frame, keypoints first; downsample != 0: followed by the voxel grid
//    with `leaf` (pts: scratch for kSmallMax points); out / cc receive the result and its size; n_out_dev / box_out6
//    (optional): the size as a plain word and the bounding box of the points, for launch_sor.
//  launch_small_voxel: the voxel grid of a cloud that already exists (n_in_dev == nullptr: n_in points), over its own
//    bounding box or over box6 (device).
void launch_small_frame(Profiler* pf, hipStream_t s, const ReprojectArgs& a, const float* kp_xy, int n_kp, int downsample,
                        const float leaf[3], o3dr_point* pts, o3dr_point* out, CloudCounters* cc, uint32_t* n_out_dev,
                        float* box_out6);
// statistical outlier removal of ONE cloud of at most kSmallMax points (n_dev[0] of them, cap >= that): preparation and
// closing stages as one workgroup each around the unchanged search kernels (5 launches instead of 30); inliers -> out in
// input order, their number -> n_out_dev[0]
void launch_sor_small(Profiler* pf, hipStream_t s, Workspace& ws, const o3dr_point* in, const uint32_t* n_dev, int64_t cap,
                      double stddev_mul, o3dr_point* out, uint32_t* n_out_dev);
void launch_small_voxel(Profiler* pf, hipStream_t s, const o3dr_point* in, const uint32_t* n_in_dev, uint32_t n_in,
                        const float* box6, const float leaf[3], uint32_t min_points, float z_offset, o3dr_point* out,
                        CloudCounters* cc);
// cv::bilateralFilter on u8 images; tab = color_weight[256] | space_weight[maxk] | tile offsets [maxk] (device)
constexpr int kBilMaxRadius = 64;
void launch_bilateral(Profiler* pf, hipStream_t s, const uint8_t* src, int64_t src_pitch, int64_t src_fstride, int rows,
                      int cols, int frames, int radius, int maxk, const float* tab, uint8_t* dst, int64_t dst_pitch,
                      int64_t dst_fstride);
int bilateral_tile_width(int radius);
void launch_disp_variance(Profiler* pf, hipStream_t s, const uint8_t* disp, int64_t pitch, int64_t fstride, int rows, int cols,
                          int frames, int bb, int cs, double min_disp, unsigned long long* hist, double* var_out);
void launch_bbox(Profiler* pf, hipStream_t s, const float* mm, int used, float* out6);
// statistical outlier removal of `frames` clouds (cloud f = in + f*in_fstride, n_dev[f] points, bounding boxes in ws.mm
// slots [0, mm_used) of frame f): inliers -> out + f*out_fstride in input order, counts -> n_out_dev[f], their bounding
// boxes -> ws.mm slots [0, returned value) of frame f.  The sort buffers of ws (keys/vals/hist/geom) are used.
int launch_sor(Profiler* pf, hipStream_t s, Workspace& ws, const o3dr_point* in, int64_t in_fstride, const uint32_t* n_dev,
               int frames, int64_t cap, int mm_used, double stddev_mul, o3dr_point* out, int64_t out_fstride,
               uint32_t* n_out_dev);
// the search grid of `frames` clouds (plan with ~cell_points points per column, active above active_above points, cell ids,
// radix sort, populations -> ws.grid_cell_first, points in cell order with their original index in .w -> ws.grid_xyz);
// bounding boxes in ws.mm slots [0, mm_used) of every frame.  Part of launch_sor; the nearest-neighbour target grid too.
void launch_search_grid(Workspace& ws, hipStream_t s, const o3dr_point* in, int64_t in_fstride, const uint32_t* n_dev, int frames,
                        int64_t cap, int mm_used, double cell_points, uint32_t active_above);
// exact nearest neighbour (kernels/nn.inc).  launch_nn_grid: the target's grid (n points, also in ws.n_valid[0]; bounding-box
// slots ws.mm [0, mm_used)) in ws.grid_*, its box -> box6 (device, 6 floats), the cells' boxes -> cell_lo / cell_hi
// (ws.grid_max_cells + 1 each); returns the view of it that the kernels below search, good until the next grid is built in
// ws.  launch_nn_query: idx (+ d2) of n queries (T12 != nullptr: each query is A2(T12, point) first);
// partial != nullptr: the ICP epilogue (changed against idx_prev, moments about c0) and its fold into rec[kIcpRecord]
constexpr int kIcpRecord = 18;  // the rigid record (o3dr_rigid_solve.h), then sum d2, changed queries
enum : int { ICP_D2 = kRigidFields, ICP_CHANGED = kRigidFields + 1 };
static_assert(RIGID_N == 0 && RIGID_SA == 1 && RIGID_SB == 4 && RIGID_SAB == 7 && kRigidFields == 16 && kIcpRecord == kRigidFields + 2,
              "an ICP record's first 16 fields are the rigid record: rigid_solve reads either");
SearchGrid launch_nn_grid(Profiler* pf, hipStream_t s, Workspace& ws, const o3dr_point* target, int64_t n, int mm_used, float* box6,
                          float4* cell_lo, float4* cell_hi);
void launch_nn_query(Profiler* pf, hipStream_t s, const SearchGrid& grid, const o3dr_point* query, int64_t n, const float* T12,
                     float r2, uint32_t* idx_out, float* d2_out, const uint32_t* idx_prev, const double c0[3], double* partial,
                     double* rec);
inline int64_t nn_partial_blocks(int64_t n) { return (n + 255) / 256; }  // workgroups of launch_nn_query (kNnThreads queries each)
// launch_cloud_finite: flag[0] = 1 if a coordinate of the n points is not finite.
// moving least squares (kernels/mls.inc).  launch_mls: o3dr_mls_smooth over the grid launch_nn_grid built for `cloud`;
// counters (device, 4 x u64): n_none, n_plane, n_poly, max neighbours
void launch_cloud_finite(Profiler* pf, hipStream_t s, const o3dr_point* in, int64_t n, uint32_t* flag);
void launch_mls(Profiler* pf, hipStream_t s, const SearchGrid& grid, const o3dr_point* cloud, int64_t n, double r, int order,
                double h, o3dr_point* out, float* normals, uint32_t* nn_count, uint8_t* fit, unsigned long long* counters);
// feature matching (kernels/match.inc)
struct MatchPair {      // one (query set, train set) pair of a call; rows relative to the pool
    uint32_t qbase, nq, tbase, nt;
    uint32_t chunks;    // ceil(nt / chunk_rows)
    uint32_t qwaves;    // ceil(nq / 64)
    uint64_t item0;     // first work item (wave); the pair has qwaves * chunks
    uint64_t rec0;      // first record (exclusive prefix of nq)
    uint64_t part0;     // first partial slot; chunk c's row i at part0 + c * nq + i
};
struct MatchArgs {
    const uint4* desc;  // the pool, 32 bytes per row
    uint32_t n_pairs;
    uint32_t chunk_rows;
    uint64_t n_items, n_rec;
    uint4* rec;         // n_rec o3dr_knn2
    uint8_t* good;      // n_rec or nullptr
    float ratio;
    uint32_t max_distance;
};
constexpr uint32_t kMatchMaxChunk = 1u << 23;  // train rows per chunk at most (kMatchKeyBits)
constexpr int64_t kMatchSliceItems = 1 << 24;  // work items per k_match_scan launch at most
void launch_match(Profiler* pf, hipStream_t s, const MatchArgs& a, const MatchPair* pairs, uint2* partial);
// What a matching pass leaves for the kernel that reads next (the chain, the chain form of the RANSAC, the graph's moments):
// the pool's 3-D keypoints, launch_match's table, its records and mask, and the RANSAC's byte per record.  One device
// function reads a row through it: matched_row (kernels/match.inc).
struct MatchedPairs {
    const o3dr_point* kp3;   // the pool
    const MatchPair* pairs;  // qbase / nq / tbase / nt / rec0
    const uint4* rec;        // o3dr_knn2 per record
    const uint8_t* good;
    const uint8_t* inlier;   // launch_ransac's byte per record, or nullptr: no filter
};
// index-aligned 3-D keypoints: kp_off (n_frames + 1 int32, device) relative to kp_xy
void launch_keypoints_3d(Profiler* pf, hipStream_t s, const ReprojectArgs& a, const float* kp_xy, const int32_t* kp_off, int n_frames,
                         int n_kp, o3dr_point* out);
// batched rigid fit (segments of at most 2^32-1 points)
constexpr int kRigidPoints = 256;  // points per workgroup of the sums (ICP's kNnThreads)
struct RigidSeg {
    uint64_t start;     // first point
    uint32_t n;         // points
    uint32_t block0;    // first workgroup of the sums (ceil(n / kRigidPoints) workgroups)
};
struct RigidArgs {
    const o3dr_point* src;
    const o3dr_point* tgt;
    const uint8_t* mask;  // or nullptr
    const RigidSeg* seg;
    uint32_t n_segs, n_blocks;
    uint32_t* first;      // n_segs: first used pair inside the segment (0xFFFFFFFF: none)
    double* partial;      // kRigidFields * n_blocks (field-major)
    double* rec;          // n_segs * kRigidFields moments, then n_segs residual sums
    double* c0;           // n_segs * 3
    const double* T;      // n_segs * 12 (the residual pass)
};
// residual == false: first used pairs, moments about c0 and their fold into rec / c0; true: the squared residuals at T
// folded into rec
void launch_rigid(Profiler* pf, hipStream_t s, const RigidArgs& a, bool residual);
// pose chain (kernels/pose_chain.inc): one launch of one workgroup for the whole call
constexpr int kChainThreads = 1024;
constexpr int kChainRun = 256;      // slots per run of the moment sums (kRigidPoints)
constexpr int kChainMaxPairs = 32;  // pairs per frame at most (range_width's limit)
struct ChainFrameIn {   // one frame of the call; rows relative to the pool
    uint32_t pair0, n_pairs;  // its pairs in the static list (a history frame: none)
    uint32_t qbase, nq;
};
struct ChainArgs {
    MatchedPairs m;
    const int32_t* pair_train;   // the train frame of every pair
    const ChainFrameIn* frames;  // n_frames
    const float* prior;          // n_frames * 16
    float* poses;                // n_frames * 16: history on entry, every frame on exit
    int32_t* status;             // n_frames: likewise
    o3dr_chain_frame* out;       // n_frames records (written from n_fixed on)
    uint32_t n_frames, n_fixed, min_matches;
    double max_rms;
};
void launch_pose_chain(Profiler* pf, hipStream_t s, const ChainArgs& a);
// three-point RANSAC for a rigid transform (kernels/ransac.inc): one workgroup per segment
constexpr int kRansacThreads = 256;
constexpr int kRansacStage = 1024;  // candidates of a segment staged in LDS (6 floats + the position each: 28 KiB); the rest go through `over`
struct RansacSeg {
    uint64_t start;     // first point (o3dr_ransac_rigid) / first record of the pair (the chain): where its inlier bytes start too
    uint64_t key;       // the sampler's key
    uint64_t over0;     // its slice of `over`: max(n - kRansacStage, 0) entries
    uint32_t n;         // points / query rows
    uint32_t reserved;
};
struct RansacArgs {
    const o3dr_point* src;       // o3dr_ransac_rigid: index-aligned points and the mask (or nullptr)
    const o3dr_point* tgt;
    const uint8_t* mask;
    MatchedPairs m;              // the chain: one segment per pair.  m.inlier stays nullptr: the kernel reads no filter, it
                                 // writes one, so its mask is the writable member below, not the read-only one in `m`
    const RansacSeg* seg;        // n_segs
    uint32_t* over;              // positions of the candidates past kRansacStage, per segment
    uint8_t* inlier;             // one byte per point / record
    o3dr_ransac_result* res;     // n_segs
    uint64_t seed;
    double thr2;                 // threshold^2
    uint32_t iterations, n_segs;
};
void launch_ransac(Profiler* pf, hipStream_t s, const RansacArgs& a, bool chain);
// pose-graph refinement (kernels/pose_graph.inc)
constexpr int kGraphRun = 256;      // rows per run of the moment sums (kChainRun): one workgroup step
constexpr int kGraphFields = 29;    // the contract's 28 moments, then the pair's good rows
constexpr int kGraphThreads = 256;  // the solve's one workgroup
struct GraphMomArgs {
    MatchedPairs m;
    const uint8_t* pair_ok;      // n_pairs: both frames accepted
    double* mom;                 // n_pairs * kGraphFields
    uint32_t* counts;            // n_pairs * 2: n_good, n_used
    uint32_t n_pairs;
};
void launch_graph_moments(Profiler* pf, hipStream_t s, const GraphMomArgs& a);
struct GraphFrameIn {
    uint32_t adj0, n_adj;        // its (edge, side) entries in `adj`
    uint32_t role;               // O3DR_REFINE_*
    uint32_t reserved;
};
struct GraphEdgeIn {
    uint32_t i, j;               // the frames
    uint32_t pair;               // its place in the pair list (moments)
    uint32_t reserved;
};
struct GraphArgs {
    const double* mom;           // launch_graph_moments' records
    const GraphEdgeIn* edges;    // n_edges, in pair order
    const GraphFrameIn* frames;  // n_frames
    const uint32_t* adj;         // 2 n_edges: edge << 1 | side, per frame in pair order
    const float* poses_in;       // n_frames * 16
    const float* prior;          // n_frames * 16, or nullptr
    float* poses_out;            // n_frames * 16
    double* state;               // n_frames * 12: R (row-major), t
    double* Hij;                 // n_edges * 36
    double* ge;                  // n_edges * 12: g_i, g_j
    double* Ee;                  // n_edges * 2: the edge's energy at the input, at the output poses
    double* Hd;                  // n_frames * 36 diagonal blocks, then n_frames * 36 inverses
    double* vec;                 // 5 vectors of 6 n_frames: r, x, z, p, H p
    o3dr_refine_frame* frames_out;
    o3dr_refine_result* res;     // one record; the counts come from the host
    o3dr_refine_result counts;
    double prior_weight;
    uint32_t n_frames, n_edges, gn_iterations, cg_iterations;
};
void launch_graph_solve(Profiler* pf, hipStream_t s, const GraphArgs& a);
// The dense XY cell order of a cloud (kernels/cell_order.inc): the points sorted by the dense id
// (iy - y0) * wx + (ix - x0) of their cell, input order kept inside a cell.  The operator's Args (PlaneArgs, MeshArgs:
// cloud, n, the parameter of its index rule, `cells`) select the index rule; a RasterFrame takes the range pass alone.
struct CellOrder {
    int32_t x0, y0;               // the index box's lower corner
    uint64_t wx, wy;              // its widths (wx * wy within the operator's limit, at most 2^32)
    uint32_t n;                   // points
    const uint32_t* keys;         // n sorted dense cell ids
    const uint32_t* perm;         // n input indices in sorted order
    const uint32_t* ord;          // n: exclusive scan of the run heads (the cell ordinal at every run head)
    const uint32_t* n_runs;       // device: the number of occupied cells
};
constexpr int kCellRangeBlocks = 1024;  // workgroups (and partials) of the range pass at most
inline int64_t cell_range_parts(int64_t n) { return n < (int64_t)kCellRangeBlocks * 256 ? (n + 255) / 256 : kCellRangeBlocks; }
// launch_cell_range: the order-preserving index range of a.n points (range[0..3]: ix_min ix_max iy_min iy_max, each as
// int32 ^ 0x80000000; range[4] = 1 if an index leaves int32; range[4..7] are written), through `part` (kPartWords words
// for each of cell_range_parts(n) workgroups).  launch_cell_order (a.cells' box set): the sort of the dense cell ids
// (nbits wide) in ws and the run heads scanned into cell ordinals (head, n words; the cell count -> *n_runs_dev); fills
// the rest of a.cells.
template <class Args>
void launch_cell_range(Profiler* pf, hipStream_t s, const Args& a, uint32_t* part, uint32_t* range);
template <class Args>
void launch_cell_order(Profiler* pf, hipStream_t s, Workspace& ws, Args& a, int nbits, uint32_t* head, uint32_t* n_runs_dev);
// RANSAC plane segmentation (kernels/plane.inc; the fields are filled by o3dr_segment_plane step by step)
struct PlaneArgs {
    const float4* pts;            // points in tile order: (x, y, z, original index bits) when tiled, else the cloud itself
    const o3dr_point* cloud;      // the cloud in input order
    int tiled;                    // 1: pts is the gathered tile order
    uint32_t n, n_tiles, H;
    CellOrder cells;              // tiled: the tiles are the cells
    double s;                     // tile size
    float tf;                     // (float)distance_threshold
    uint64_t seed;
    uint32_t* tstart;             // n_tiles + 1: first point of every tile in tile order
    uint32_t* cfirst;             // n_tiles + 1: first chunk of every tile; cfirst[n_tiles] = the chunk count
    o3dr_plane_tile* rec;         // n_tiles records
    float4* hyp;                  // n_tiles * H hypothesis planes (NaN: degenerate)
    uint32_t* counts;             // n_tiles * H scores
    double* partial;              // kPlaneMoments per chunk
    uint8_t* inlier;              // n or nullptr
    int32_t* tile;                // n or nullptr
    o3dr_point* projected;        // n or nullptr
};
constexpr int kPlaneChunkPoints = 128;  // points per wave chunk (kPlaneChunk)
constexpr int kPlaneMomentsHost = 10;   // fp64 moments per chunk (kPlaneMoments)
// launch_plane_tiles: tiled, the points gathered into tile order (pts, which a.pts names); tile starts, records and
// chunks (a.n_tiles set).  launch_plane_fit: hypotheses, scores, the choice, refinement (optimize) and labels.
void launch_plane_tiles(Profiler* pf, hipStream_t s, Workspace& ws, const PlaneArgs& a, float4* pts);
void launch_plane_fit(Profiler* pf, hipStream_t s, const PlaneArgs& a, int64_t max_chunks, int optimize);
// height-field surface mesh (kernels/mesh.inc; the fields are filled by o3dr_mesh_surface step by step)
struct MeshArgs {
    const o3dr_point* cloud;      // the cloud in input order
    uint32_t n;
    float inv;                    // 1.0f / (float)cell_size
    float lf;                     // (float)(L * L): the edge gate on d2
    CellOrder cells;              // the cell of a vertex; cells.n_runs: V, the vertex count
    uint32_t* vkey;               // V cell ids in cell order
    float4* vpt;                  // V vertices: x y z, input index bits in .w
    int4* nbr;                    // V: the ordinals of the right, upper-right, upper and upper-left cells (-1: empty)
    uint32_t* cnt;                // n: kept triangles per vertex, then their exclusive scan (the first triangle's slot)
    uint32_t* part;               // kPartWords words per workgroup of the whole-cloud reductions
    uint32_t* counters;           // full quads, rejected by orientation, rejected by length
    int32_t* tris;                // 3 T
    float* normals;               // 3 n
};
// launch_mesh_count: the vertices gathered, their neighbours, triangles per vertex scanned into offsets
// (T -> *n_tris_dev) and the counters.  launch_mesh_emit: the triangles (a.tris) and the vertex normals (a.normals),
// each if set.
void launch_mesh_count(Profiler* pf, hipStream_t s, Workspace& ws, const MeshArgs& a, uint32_t* n_tris_dev);
void launch_mesh_emit(Profiler* pf, hipStream_t s, const MeshArgs& a);
// The raster frame (DESIGN.md "Raster frame"): what a pass over the points of a box of XY cells needs and nothing else.
// Held by value by every operator of the raster family; o3dr_raster_extent builds a frame alone, for launch_cell_range.
struct RasterFrame {
    const o3dr_point* cloud;      // the cloud in input order
    uint32_t n;
    float inv;                    // 1.0f / (float)cell_size
    int32_t cx0, cy0, width, height;  // the box: cells cx0 .. cx0 + width - 1, cy0 .. cy0 + height - 1
    uint32_t* part;               // kPartWords words per workgroup of the operator's passes (cell_range_parts(n) for a point pass)
};
// map raster (kernels/raster.inc; the fields are filled by o3dr_rasterize_map step by step)
struct RasterArgs {
    RasterFrame f;                // f.part: raster_winner_parts(n) records of the winner pass, then one per tile
    int32_t select, R;            // O3DR_RASTER_*, the fill radius in cells
    double cell_size, light[3];   // light: normalised (read when shade is set)
    unsigned long long* win;      // width * height: the chosen point's (z key, input index), all ones = empty
    int8_t* col;                  // width * height (R > 0): the offset in cy of the column's nearest occupied cell, kRasterNone = none
    uint32_t* counters;           // 12 words: n_inside n_outside - - | n_occupied n_filled n_empty - | z_min z_max (ordered) - -
    float* height_map;            // the outputs (nullptr: not asked for; height_map is scratch when only the shade needs it)
    uint8_t* color;
    uint8_t* shade;
    int32_t* source;
    int32_t* distance2;
};
constexpr int kRasterTileW = 64, kRasterTileH = 4;  // cells per workgroup of the row pass
inline int64_t raster_tiles(int64_t width, int64_t height)
{
    return ((width + kRasterTileW - 1) / kRasterTileW) * ((height + kRasterTileH - 1) / kRasterTileH);
}
inline int64_t raster_winner_parts(int64_t n) { return cell_range_parts(n); }
// launch_raster: a.win set to empty, the winner pass, the column pass (R > 0), the row pass with the outputs and the shade
// stencil; the counters folded into a.counters
void launch_raster(Profiler* pf, hipStream_t s, const RasterArgs& a);
// ground filter (kernels/ground.inc; contract: include/o3dr_terrain.h "ground filter").  The raster's own passes run on
// `r`: the winner pass (select = BOTTOM) into r.win, and at the end the fill passes on r.win with every cell that is not
// ground set empty, r.height_map = the DTM (r.R = fill_radius; r.color, r.shade, r.source, r.distance2 unset).
struct GroundArgs {
    RasterArgs r;
    int32_t n_iter;
    int32_t radius[O3DR_GROUND_MAX_ITERATIONS];
    float thr[O3DR_GROUND_MAX_ITERATIONS];
    float* zl;                    // width * height: Z of a live cell, +inf for an empty or removed one
    float* t1;                    // width * height: the row passes' results
    float* t2;                    // width * height: E masked to the live cells (-inf elsewhere)
    float* run;                   // width * height: the column passes' suffix minima / maxima per block of 2r + 1 rows
    uint8_t* state;               // width * height: 0 empty, 1 live / ground, 2 + k removed by iteration k
    uint32_t* counters;           // 80 words: n_inside n_outside - - | n_ground_cells n_dtm_filled n_dtm_empty - | (the resolve's z range) |
                                  //   n_ground_points - - - | n_removed[k] - - - for k = 0..15
    uint8_t* ground;              // n or nullptr
    float* hag;                   // n or nullptr
};
constexpr int kGroundTileW = 256;         // cells of one row per workgroup of the row passes
constexpr int kGroundColRowsMax = 4096;   // row blocks a column pass spreads over workgroups at most (the others by stride)
constexpr int kGroundCounterWords = 16 + 4 * O3DR_GROUND_MAX_ITERATIONS;
inline int64_t ground_col_groups(int64_t width) { return (width + 255) / 256; }
inline int64_t ground_col_rows(int64_t height, int r)
{
    const int64_t blocks = (height + 2 * (int64_t)r) / (2 * (int64_t)r + 1) + 1;  // blocks of 2r + 1 rows, and the one before row 0
    return blocks < kGroundColRowsMax ? blocks : kGroundColRowsMax;
}
// workgroup partials of a call: the winner and the point pass, the raster's tiles, the column pass of every iteration
inline int64_t ground_parts(const GroundArgs& a)
{
    const RasterFrame& f = a.r.f;
    int64_t parts = raster_tiles(f.width, f.height);
    if (raster_winner_parts(f.n) > parts) parts = raster_winner_parts(f.n);
    for (int k = 0; k < a.n_iter; ++k) {
        const int64_t g = ground_col_groups(f.width) * ground_col_rows(f.height, a.radius[k]);
        if (g > parts) parts = g;
    }
    return parts;
}
// launch_ground: the minimum surface, the iterations (enqueued back to back: nothing is read back), the DTM with its fill,
// the point pass; every count folded into a.counters
void launch_ground(Profiler* pf, hipStream_t s, const GroundArgs& a);
// raster interpolation (kernels/interpolate.inc; contract: include/o3dr_dem.h "raster interpolation").  Level 0 is the
// input itself (the NaN test is its count); the levels 1 .. L live one after the other in cnt / val, level l from lv[l].off.
// val holds m_l after the pull and F_l after the push: the push writes the cells with c_l = 0 only, and nobody reads m_l there.
struct InterpLevel {
    int32_t W, H;
    int64_t off;                  // the level's first cell in cnt / val (level 0: unused)
};
struct InterpArgs {
    const float* raster;          // level 0
    int32_t L;                    // the top level
    int32_t smooth, max_level;
    InterpLevel lv[O3DR_INTERPOLATE_MAX_LEVELS];
    int32_t* cnt;                 // c_l, l >= 1
    float* val;                   // m_l, then F_l, l >= 1
    float* filled;                // width * height
    uint8_t* level;               // width * height or nullptr
    uint32_t* part;               // kInterpPartWords words per workgroup of the level-0 push
    uint32_t* counters;           // kInterpPartWords words: n_by_level[0..31], n_filled, n_empty, - ...
    uint32_t* bad;                // 1: an infinite input value
};
constexpr int kInterpPullTile = 32;       // cells a side of a pull tile: five levels per launch (32 -> 16 -> 8 -> 4 -> 2 -> 1)
constexpr int kInterpPullLevels = 5;
constexpr int kInterpRegion = 64;         // cells a side of a push tile with its apron of `smooth` cells; a level that fits
                                          // in one region is finished by the one-workgroup kernel
constexpr int kInterpMaxBlocks = 1024;    // workgroups of a tiled launch at most (the other tiles by stride)
constexpr int kInterpPartWords = 40;
inline int64_t interp_blocks(int64_t tiles) { return tiles < kInterpMaxBlocks ? tiles : kInterpMaxBlocks; }
inline int64_t interp_pull_tiles(const InterpLevel& v)
{
    return (((int64_t)v.W + kInterpPullTile - 1) / kInterpPullTile) * (((int64_t)v.H + kInterpPullTile - 1) / kInterpPullTile);
}
inline int interp_push_tile(int smooth) { return kInterpRegion - 2 * smooth; }
inline int64_t interp_push_tiles(const InterpLevel& v, int smooth)
{
    const int64_t t = interp_push_tile(smooth);
    return (((int64_t)v.W + t - 1) / t) * (((int64_t)v.H + t - 1) / t);
}
// the first level that fits in one region (0 for a raster of at most 64 x 64 cells)
inline int interp_top_level(const InterpArgs& a)
{
    int l = 0;
    while (a.lv[l].W > kInterpRegion || a.lv[l].H > kInterpRegion) ++l;
    return l;
}
// launch_interpolate: the pulls, the one-workgroup top, the pushes down to level 0 with the outputs; the counters folded
// into a.counters, a.bad set (it is cleared first)
void launch_interpolate(Profiler* pf, hipStream_t s, const InterpArgs& a);
// raster sample (kernels/interpolate.inc; contract: include/o3dr_dem.h "raster sample")
struct SampleArgs {
    RasterFrame f;
    const float* raster;          // width * height: the raster of the frame's box
    float* value;                 // n or nullptr
    float* hag;                   // n or nullptr
    uint32_t* counters;           // 4 words: inside, outside, on a NaN cell, -
};
void launch_raster_sample(Profiler* pf, hipStream_t s, const SampleArgs& a);
// contour lines (kernels/contour.inc; contract: include/o3dr_contour.h).  Every array is the call's own scratch
// but lines_out / seg_out / vertices.  The first block is what the count pass needs; the second is sized by the segments
// counted (n_seg).
struct ContourVertex {
    double x, y;
};
struct ContourArgs {
    const float* raster;          // W * H
    int32_t W, H, cx0, cy0;
    double interval, base, cell_size;
    uint32_t n_quads;             // (W - 1) * (H - 1)
    int32_t* kc;                  // W * H: K(z) of every cell, kContourHole on a NaN
    uint32_t* off;                // n_quads: a quad's segments -> its first segment (exclusive scan)
    uint32_t* part;               // contour_blocks(max(cells, n_quads, n_seg)) * kPartWords
    uint32_t* scan_partial;       // contour_scan_words(max(n_quads, n_seg))
    uint32_t* counters;           // kContourCounterWords: n_quads n_crossed k_lo k_hi (order-preserving words) | n_closed
                                  //   n_longest - - | n_lines n_vertices (the scans' totals) - - | the segments (low, high word) - -
    uint32_t* flags;              // 2 words: an infinite value, a level index outside +-2^30
    uint32_t n_seg;
    double4* xy;                  // n_seg: x0 y0 x1 y1
    int2* kn;                     // n_seg: k, next
    int* parent;                  // n_seg: the union-find, then every segment's root = its line's lowest index
    int* prev;                    // n_seg: the inverse of next, -1
    int* head;                    // n_seg, at a root: the line's head
    uint32_t* cnt;                // n_seg, at a root: the line's segments
    uint32_t* num;                // n_seg: 1 at a root -> the line's number (exclusive scan)
    uint32_t* beg;                // n_seg: n_segments + 1 at a root -> the line's begin (exclusive scan)
    int2* jump[2];                // n_seg each: (the predecessor 2^round steps back or -1, the steps taken): the rank
    o3dr_contour_segment* seg_out;  // n_seg or nullptr
    o3dr_contour_line* lines_out;   // n_lines or nullptr
    ContourVertex* vertices;        // n_seg + n_lines or nullptr
};
constexpr int kContourThreads = 256;      // quads (cells, segments) per workgroup turn
constexpr int kContourMaxBlocks = 1024;   // workgroups of a launch over cells or quads at most (the others by stride)
constexpr int kContourCounterWords = 16;
constexpr int32_t kContourHole = INT32_MIN;
constexpr int32_t kContourMaxLevel = 1 << 30;
inline int64_t contour_blocks(int64_t n) { return (n + kContourThreads - 1) / kContourThreads; }
inline int64_t contour_scan_words(int64_t n) { return n / 4096 + 16; }
inline int contour_rank_rounds(uint32_t n_seg)  // the bit length of n_seg: 2^rounds > every rank
{
    int r = 0;
    while ((n_seg >> r) != 0) ++r;
    return r;
}
// launch_contour_count: flags cleared, K per cell, the quads' counts with the result's first counters and the 64-bit
// sum, the exclusive scan of the counts.  launch_contour_lines (n_seg > 0, after the sum was read back): the segments,
// links, components, heads, sizes, numbers, begins and ranks.  launch_contour_outputs: the caller's arrays.
void launch_contour_count(Profiler* pf, hipStream_t s, const ContourArgs& a);
void launch_contour_lines(Profiler* pf, hipStream_t s, const ContourArgs& a);
void launch_contour_outputs(Profiler* pf, hipStream_t s, const ContourArgs& a);
// Euclidean clustering (kernels/cluster.inc; contract: include/o3dr_objects.h).  The grid is launch_nn_grid's; every array
// below it is the call's own scratch but the outputs.
struct ClusterArgs {
    uint32_t n;
    SearchGrid grid;              // the cloud's
    float r2;                     // (float)(tolerance * tolerance)
    float pad_r;                  // grid_pad_radius(tolerance): half the side of a point's box
    int32_t min_size, max_size;
    int* parent;                  // n, by original index: the union-find, then every point's final root (raw)
    uint32_t* cnt;                // n: the size of the component at its root
    uint32_t* num;                // n: 1 at a root that is a cluster -> its number (exclusive scan)
    uint32_t* beg;                // n: the size at such a root -> its begin in indices (exclusive scan)
    uint32_t* part;               // cluster_blocks(n) * kPartWords
    uint32_t* counters;           // 12 words: n_components n_too_small n_too_large largest | n_clustered_points - - - |
                                  //   n_clusters (the first scan's total), n_clustered_points (the second's), - -
    unsigned long long* n_pairs;
    int32_t* label;               // n or nullptr
    int32_t* raw;                 // n or nullptr
    int32_t* size;                // n or nullptr
    int32_t* indices;             // n_clustered_points or nullptr
    o3dr_cluster* rec;            // n_clusters or nullptr
    uint32_t* box_lo;             // 3 * n_clusters: order-preserving words of the boxes' minima (with rec)
    uint32_t* box_hi;             // 3 * n_clusters: ... maxima
    unsigned long long* sums;     // 3 * n_clusters: the quantised offsets' sums
};
constexpr int kClusterCounterWords = 12;
inline int64_t cluster_blocks(int64_t n) { return (n + 255) / 256; }
// launch_cluster_link: parent initialised, the links joined and counted, every point flattened to its root, the sizes, the
// cluster flags with the result's counters, the two scans.  Nothing of the caller's is written.
void launch_cluster_link(Profiler* pf, hipStream_t s, Workspace& ws, const ClusterArgs& a);
// launch_cluster_outputs: after the counts were read back: the point outputs, the records (a.rec), indices (a stable sort
// of the points by cluster number through ws.keys / ws.vals: only the passes n_clusters needs)
void launch_cluster_outputs(Profiler* pf, hipStream_t s, Workspace& ws, const ClusterArgs& a, uint32_t n_clusters, uint32_t n_clustered);
// plane-fitted disparity per segment label (kernels/plane_disparity.inc).  `table`: kPdSums 64-bit sums per (frame, label) -
// n Sx Sy Sxx Sxy Syy Sd Sxd Syd Sdd and the pixel count -, zeroed here; thr: d participates iff (int)d > thr; flag: a
// device word, bit 0 set when a label >= n_labels was seen.  launch_plane_disp runs the three steps for `frames` frames:
// the sums, the fit of every (frame, label) into rec (frames * n_labels records) and the dense f64 image `out`.
constexpr int kPdSums = 11;
struct PlaneDispArgs {
    const uint8_t* disp;
    int64_t dpitch, dfs;
    const uint8_t* labels;
    int64_t lpitch, lfs;
    int32_t elem;  // bytes per label: 1, 2, 4
    int32_t rows, cols, frames;
    uint32_t n_labels;
    int32_t thr, min_pixels, fill;
    double max_mse;
    unsigned long long* table;
    o3dr_plane_disp_segment* rec;
    double* out;
    uint32_t* flag;
};
void launch_plane_disp(Profiler* pf, hipStream_t s, const PlaneDispArgs& a);
// ORB features (kernels/orb.inc; contract: include/o3dr.h "ORB features").  One OrbArgs describes a group of `frames`
// frames.  Per frame the grey pyramid, the FAST score map (u8) and the 5 x 5 box sums (u16) share one layout: level l at
// element lv[l].off (a multiple of 256), rows tight, `P` elements per frame.  Candidates are found over chunks of
// kOrbChunk consecutive pixels of a level in row-major order: chunk_cnt holds chunks_per_frame words per frame (counts,
// then their exclusive scan per level), cand_r / cand_pos cands_per_frame slots per frame (level l from lv[l].cand0,
// row-major order; pos = y << 16 | x).  The selection compacts a (frame, level) segment's kept candidates to the front of
// its slots.  seg_cand / seg_sel / seg_out: frames * n_levels entries (candidates, kept, first output row).
constexpr int kOrbMaxLevels = 8;
constexpr int kOrbChunk = 1024;
// D[k] = (round(16384 cos(2 pi k / 64)), round(16384 sin(2 pi k / 64))), k = 0..63
#define O3DR_ORB_DIRECTIONS                                                                                                  \
    {16384, 0}, {16305, 1606}, {16069, 3196}, {15679, 4756}, {15137, 6270}, {14449, 7723}, {13623, 9102}, {12665, 10394},    \
    {11585, 11585}, {10394, 12665}, {9102, 13623}, {7723, 14449}, {6270, 15137}, {4756, 15679}, {3196, 16069},               \
    {1606, 16305}, {0, 16384}, {-1606, 16305}, {-3196, 16069}, {-4756, 15679}, {-6270, 15137}, {-7723, 14449},               \
    {-9102, 13623}, {-10394, 12665}, {-11585, 11585}, {-12665, 10394}, {-13623, 9102}, {-14449, 7723}, {-15137, 6270},       \
    {-15679, 4756}, {-16069, 3196}, {-16305, 1606}, {-16384, 0}, {-16305, -1606}, {-16069, -3196}, {-15679, -4756},          \
    {-15137, -6270}, {-14449, -7723}, {-13623, -9102}, {-12665, -10394}, {-11585, -11585}, {-10394, -12665},                 \
    {-9102, -13623}, {-7723, -14449}, {-6270, -15137}, {-4756, -15679}, {-3196, -16069}, {-1606, -16305}, {0, -16384},       \
    {1606, -16305}, {3196, -16069}, {4756, -15679}, {6270, -15137}, {7723, -14449}, {9102, -13623}, {10394, -12665},         \
    {11585, -11585}, {12665, -10394}, {13623, -9102}, {14449, -7723}, {15137, -6270}, {15679, -4756}, {16069, -3196},        \
    {16305, -1606}
struct OrbLevel {
    int32_t w, h;        // 0 x 0: the level does not exist
    int32_t chunks;      // ceil(w * h / kOrbChunk)
    int32_t chunk0;      // its first chunk within a frame
    int32_t quota;       // keypoints kept at most
    int32_t qprefix;     // sum of the quotas of the levels before it
    int64_t off;         // first element within a frame's pyramid
    int64_t cand0;       // first candidate slot within a frame
};
struct OrbArgs {
    const uint8_t* img;
    int64_t fstride, pitch;
    int32_t rows, cols, channels, frames, n_levels, n_features, thr, edge;
    OrbLevel lv[kOrbMaxLevels];
    int64_t P, cands_per_frame;
    int32_t chunks_per_frame;
    int32_t f0;               // index of the group's first frame in the call
    uint8_t *pyr, *score;
    uint16_t* box;
    uint32_t* chunk_cnt;
    long long* cand_r;
    uint32_t* cand_pos;
    uint32_t *seg_cand, *seg_sel;
    long long* seg_out;
    long long* run_total;     // device word: keypoints of the groups before this one
    long long* offsets;       // device copy of the call's offsets (n_frames + 1)
    const int8_t* pattern;    // the steered table, 64 x 256 x 4
    o3dr_orb_keypoint* kp;    // each nullptr: not asked for
    float* kp_xy;
    uint8_t* desc;
};
void launch_orb(Profiler* pf, hipStream_t s, const OrbArgs& a);
// Stereo disparity (kernels/stereo.inc; contract: include/o3dr.h "stereo disparity").  One StereoArgs describes a group of
// `frames` frames.  Per frame: the two census images (rows * cols words each), S (rows * cols * D uint16, candidate
// fastest), the left winners `win` (cost << 16 | rejected << 15 | (off + 8) << 8 | best) and the right winners bestR.
struct StereoArgs {
    const uint8_t *left, *right;
    int64_t fstride, pitch;
    int32_t rows, cols, channels, frames;
    int32_t D, d0, p1, p2, n_paths, uniq, lr;
    unsigned long long *cenL, *cenR;
    uint16_t* S;
    uint32_t* win;
    uint8_t* bestR;
    uint8_t* disp;   // the group's first frame in each output, rows tight; each nullptr: not asked for
    uint16_t *q4, *cost;
};
void launch_stereo(Profiler* pf, hipStream_t s, const StereoArgs& a);
// Disparity filter (kernels/disparity_filter.inc; contract: include/o3dr.h "disparity filter").  One DfArgs describes a
// group of `frames` frames.  in: the caller's image with its strides; median != 0 writes the median of it to `out` (rows
// tight) and the components are then taken of `out`, else of `in`.  parent / cnt: one int32 per pixel each, the
// union-find forest (-1: invalid pixel) and the pixel counts at the roots; nullptr: the call needs no labelling.
struct DfView {
    const void* p;
    int64_t fstride, pitch;  // bytes
};
struct DfArgs {
    DfView in, src;      // src: set by the launcher (the image after the median)
    int32_t rows, cols, frames, elem, median, max_diff, max_size;
    int32_t* parent;
    int32_t* cnt;
    int32_t *labels_out, *sizes_out;  // the group's first frame in each output, rows tight; each nullptr: not asked for
    unsigned long long* info;         // [frames][5]: n_valid, n_components, n_speckles, n_removed, largest; nullptr: not asked for
    void* out;
};
void launch_disparity_filter(Profiler* pf, hipStream_t s, const DfArgs& a);
// Multi-view filter (kernels/multiview.inc; contract: include/o3dr.h "multi-view filter").  One MvArgs describes the whole
// call: `in` with its byte strides, the neighbour lists [frames][k] and their matrices [frames][k][16] (row-major, made on
// the host), the outputs with rows tight.  info: [frames][9] in o3dr_multiview_info's order; nullptr: not asked for.
// launch_multiview_fuse (contract: "multi-view fusion") takes the same struct: it writes fused_out (float64 levels) and
// votes_out in place of `out`, and its info is [frames][12]: the filter's nine, then n_votes, n_votes_dropped, n_fused.
struct MvArgs {
    const void* in;
    int64_t fstride, pitch;
    int32_t rows, cols, frames, f0, elem, k, min_support, max_violations;  // f0: set by the launcher (a launch's first frame)
    double tolerance;
    const int32_t* neighbors;
    const double* H;
    void* out;
    uint8_t *support_out, *violations_out;  // each nullptr: not asked for
    unsigned long long* info;
    double* fused_out;   // the fusion alone
    uint8_t* votes_out;  // the fusion alone; nullptr: not asked for
};
void launch_multiview_filter(Profiler* pf, hipStream_t s, const MvArgs& a);
void launch_multiview_fuse(Profiler* pf, hipStream_t s, const MvArgs& a);
// Image segmentation (kernels/segment_image.inc; contract: include/o3dr.h "image segmentation").  One SegArgs describes a
// group of `frames` frames; every array holds the group's frames one after the other.  centres: [nx * ny][5] int32 x, y,
// B, G, R; sums: [nx * ny][6] n, sum x, sum y, sum B, sum G, sum R.  Per pixel: raw (the centre index), parent / cnt (the
// union-find forest of disparity_filter.inc and the pixel counts at the roots), key (the 64-bit bid of a small component,
// later its final root and its label's first pixel), link, flag (root flags, then their exclusive scan).
struct SegArgs {
    const uint8_t* img;  // the group's first frame
    int64_t fstride, pitch;
    int32_t rows, cols, channels, frames, S, m, iterations, min_size, nx, ny;
    int32_t* centres;
    unsigned long long* sums;
    int32_t *raw, *parent, *cnt, *link;
    unsigned long long* key;
    uint32_t *flag, *partial;         // partial: the scan's chunk sums, frames * ceil(rows * cols / 4096) words
    int32_t *labels_out, *sizes_out;  // the group's first frame, rows tight; sizes_out nullptr: not asked for
    unsigned long long* info;         // [frames][5]: n_components, n_merged, n_labels, largest, 2^32 - 1 - smallest; nullptr: not asked for
};
void launch_segment_image(Profiler* pf, hipStream_t s, const SegArgs& a);
// Stereo rectification (kernels/rectify.inc; contract: include/o3dr.h "stereo rectification").  RectMapArgs: the inverse of
// P R (host fp64), the camera and the distortion, by value.  RectArgs: one launch group of `frames` frames through one map.
struct RectMapArgs {
    double I[9], k[8], fx, fy, cx, cy;
    int32_t rows_out, cols_out;
    int32_t* map;
};
void launch_rectify_maps(Profiler* pf, hipStream_t s, const RectMapArgs& a);
struct RectArgs {
    const uint8_t* src;   // the group's first frame
    int64_t fstride, pitch;
    int32_t rows, cols, channels, frames, rows_out, cols_out, border;
    const int32_t* map;
    uint8_t* out;         // the group's first frame, tight
    uint8_t* valid;       // nullptr: not asked for (or already written by an earlier group)
};
void launch_rectify_remap(Profiler* pf, hipStream_t s, const RectArgs& a);
void launch_partition(Profiler* pf, hipStream_t s, Workspace& ws, const VoxelArgs& v, int n_parts, o3dr_point* out,
                      uint64_t* counts_dev, uint32_t* overflow_dev, const void* hdrs_dev = nullptr, int n_hdrs = 0);
// its two halves: slice sizes without moving anything (the (part, tile) table stays in ws for the second half), then the move
// with part p's records shifted by part_shift_dev[p] against the plain "parts one after the other" layout
void launch_partition_count(Profiler* pf, hipStream_t s, Workspace& ws, const VoxelArgs& v, int n_parts, uint64_t* counts_dev,
                            uint32_t* overflow_dev, const void* hdrs_dev = nullptr, int n_hdrs = 0);
void launch_partition_move(Profiler* pf, hipStream_t s, Workspace& ws, const VoxelArgs& v, int n_parts, o3dr_point* out,
                           const int64_t* part_shift_dev);
// the exchange's small data, kept on the device (kernels/multigpu.inc)
void launch_pack_header(hipStream_t s, const float* box6_dev, const CloudCounters* cc, void* hdr32_dev);
void launch_count_from_cc(hipStream_t s, const CloudCounters* cc, uint32_t* n_dev);
void launch_set_cloud_count(hipStream_t s, CloudCounters* cc, uint64_t n);
// incremental merge (kernels/incremental.inc).  launch_inc_runs: the n points at `in` (the tail) as group runs sorted by
// group, over the grid of the box in ws.mm slot 0 (ws.n_valid[0] = n); heads from rec_heads (cloud_big's recorded flags,
// the tail starting at point `first`) or, rec_heads == nullptr, from the points.  Leaves ws.n_vox[0] groups.
void launch_inc_runs(Profiler* pf, hipStream_t s, Workspace& ws, const o3dr_point* in, int64_t n, const float leaf[3], float z_offset,
                     const uint8_t* rec_heads, int64_t first, int test_corrupt);
struct IncFoldArgs {
    const IncGroup* old_g;
    const uint32_t* old_off;
    const IncCell* old_cells;
    uint32_t n_old, n_old_cells;
    IncCell* scratch;  // 32 cells per tail group
    IncGroup* tg;      // per tail group: coordinates + new mask
    uint32_t* tmatch;  // per tail group: the state group it extends, or none
    uint32_t nt;       // tail groups (ws.n_vox[0], read back)
    uint32_t* flag;    // nt + 1 words: exclusive scan of "new group"
    uint32_t* n_new_only;  // device word: new groups
    CloudCounters* cc;
};
void launch_inc_fold(Profiler* pf, hipStream_t s, Workspace& ws, const o3dr_point* in, float z_offset, const IncFoldArgs& a,
                     uint32_t* partial);
// the merged group list (n_new groups) and its cell offsets: new_off (n_new + 1 words) ends in the cell count, also in *n_cells_dev
void launch_inc_place(Profiler* pf, hipStream_t s, const IncFoldArgs& a, uint32_t n_new, IncGroup* new_g, uint32_t* src,
                      uint32_t* new_off, uint32_t* n_cells_dev, uint32_t* partial);
void launch_inc_copy(Profiler* pf, hipStream_t s, const IncFoldArgs& a, const IncGroup* new_g, const uint32_t* new_off,
                     const uint32_t* src, uint32_t n_new, IncCell* cells, uint32_t cells_cap);
// snapshot: keep_cnt == nullptr: every cell is kept (out_off = off); else kept cells per group -> their exclusive scan in
// keep_cnt, the total in *n_keep_dev (launch_inc_keep), then the centroids (launch_inc_snapshot)
void launch_inc_keep(Profiler* pf, hipStream_t s, const IncGroup* grp, const uint32_t* off, const IncCell* cells, uint32_t n_groups,
                     uint32_t n_cells, uint32_t need, uint32_t* keep_cnt, uint32_t* n_keep_dev, uint32_t* partial);
void launch_inc_snapshot(Profiler* pf, hipStream_t s, const IncGroup* grp, const uint32_t* off, const IncCell* cells, uint32_t n_groups,
                         uint32_t n_cells, uint32_t need, const uint32_t* out_off, float z_offset, o3dr_point* out, uint32_t out_cap,
                         CloudCounters* cc);
void launch_inc_box_fold(hipStream_t s, float* box6, const float* tail6, float* mm6);

}  // namespace o3dr
