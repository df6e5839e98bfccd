// o3dr_kernels.hip — hand-written gfx950 kernels of the reconstruction hot path.
//
//   K1  k_reproject_count / k_reproject_emit   A1+A2: (u,v,disparity) -> Q -> SE(3) -> ordered cloud
//       (batched A6: k_reproject_bbox_count, then k_reproject_emit also writes the voxel index and counts the first
//       radix pass's digits over candidate-aligned sort tiles)
//   K2  k_voxel_geom / k_voxel_keys_*          A4 steps 1-5: PCL VoxelGrid geometry and linear index
//       k_radix_hist / k_radix_scatter_lane    A4 step 6: stable LSD radix sort of (index, point id)
//       k_run_heads / k_run_starts / k_centroid  A4 steps 7-8: runs -> ordered fp32 centroid
//       (the last scatter pass of a point sort leaves run-head flags, not sorted indices: k_run_heads packs them)
//
// Everything here is HBM-bound integer/byte/fp32 work: no MFMA.  The whole translation unit is
// compiled with -ffp-contract=off because the reference arithmetic (unoptimised x86 build,
// SURVEY.md section 7 "hard parts") never fuses a multiply-add, and a 1-ulp difference in a world
// coordinate flips voxel occupancy.
//
// Reference lines each kernel follows are cited at the kernel.  Wavefront size is 64.
//
// The device code lives in kernels/*.inc, one file per subsystem, all included below into this one translation
// unit (a kernel and the launcher that names it must share a TU unless device code is built relocatable):
//   util         wave/workgroup scans and reductions, helpers of the sort and run records
//   reproject    K1: count / bbox + count / emit (+ index, first histogram) / keypoint pass / in-place transform
//   bookkeeping  slot initialisation, exclusive scans, bounding box of a cloud
//   prepass      bilateral filter and variance gate on the disparity image
//   voxel_index  PCL VoxelGrid geometry, linear indices (+ fused first histogram / run-head counts)
//   radix_sort   digit histograms and the stable lane-counting scatter
//   voxel_runs   run heads/starts, min_points filter, centroid kernels, run-compressed variants, running bbox
//   multigpu     bounding-box fold, index-slice partition
//   sor          statistical outlier removal
//   small        clouds of at most kSmallMax points: the whole path in one launch of one workgroup
//   incremental  the combined merge kept as running per-cell sums (o3dr_finalize_incremental)
//   nn           exact nearest neighbour into a target's search grid, the fused ICP pass and its fold
//   mls          moving-least-squares smoothing and normals over the same grid
//   cell_order   the dense XY cell order of a cloud: index box, keys, run heads (plane tiles, mesh cells)
//   plane        RANSAC plane segmentation per XY tile
//   mesh         height-field surface mesh over the XY cells
//   raster       the merged map as images: one point per XY cell, separable hole fill, the output images, shaded relief
//   ground       bare-earth ground filter on the raster's cells: sliding window minima / maxima, DTM, height above ground
//   interpolate  hole-free rasters: pull-push over an image pyramid with Jacobi sweeps in LDS on the way down; a raster read at points
//   contour      contour lines of a raster: K per cell, counted and emitted marching-squares segments, union-find lines, pointer-jumped ranks
//   cluster      Euclidean clustering: radius walk + union-find, sizes, numbering, per-cluster records, indices
//   match        Hamming 2-NN descriptor matching, index-aligned 3-D keypoints, the batched rigid fit
//   orb          ORB features: grey pyramid, FAST score + box sums, candidates, exact selection, steered BRIEF
//   stereo       stereo disparity: grey + census, semi-global aggregation (one wave per scan line), winner + left-right check
//   disparity_filter  median and speckle removal of a disparity image: LDS median network, tiled union-find labelling
//   multiview    multi-view consistency and fusion of a stack of disparity images: one fp64 matrix per (frame, neighbour), one gather per test
//   segment_image  superpixel labels of a colour image: tiled k-means with LDS sums, the filter's union-find, merge, ordered numbering
//   rectify      stereo rectification: the fp64 Q5 map of one camera, the integer bilinear remap of a group of frames
//   pose_chain   the feature-matched pose chain: one workgroup walks the frames (gather, moments, Kabsch, residual)
//   ransac       three-point RANSAC for a rigid transform: one workgroup per segment / pair of the chain
// The launchers follow in this file.
#include <string.h>

#include "o3dr_device.h"
#include "o3dr_profile.h"

namespace o3dr {

#include "kernels/util.inc"
#include "kernels/reproject.inc"
#include "kernels/bookkeeping.inc"
#include "kernels/prepass.inc"
#include "kernels/voxel_index.inc"
#include "kernels/radix_sort.inc"
#include "kernels/voxel_runs.inc"
#include "kernels/incremental.inc"
#include "kernels/multigpu.inc"
#include "kernels/sor.inc"
#include "kernels/small.inc"
#include "kernels/rigid_core.inc"
#include "kernels/nn.inc"
#include "kernels/mls.inc"
#include "kernels/cluster.inc"
#include "kernels/cell_order.inc"
#include "kernels/plane.inc"
#include "kernels/mesh.inc"
#include "kernels/raster.inc"
#include "kernels/ground.inc"
#include "kernels/interpolate.inc"
#include "kernels/contour.inc"
#include "kernels/match.inc"
#include "kernels/plane_disparity.inc"
#include "kernels/orb.inc"
#include "kernels/stereo.inc"
#include "kernels/disparity_filter.inc"
#include "kernels/multiview.inc"
#include "kernels/segment_image.inc"
#include "kernels/rectify.inc"
#include "kernels/pose_chain.inc"
#include "kernels/ransac.inc"
#include "kernels/pose_graph.inc"

// =================================================================================================
// launchers
// =================================================================================================
static inline int cdiv64(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// exclusive scan of `frames` rows of length L in place; totals[f] = row sum (+ add[f]).
// With geom != nullptr the rows are radix histograms of pass `pass` (live length per frame).
static void launch_scan(hipStream_t s, uint32_t* data, int64_t L, int64_t row_stride, int frames, uint32_t* totals,
                        const uint32_t* add, uint32_t* partial, const VoxelGeom* geom = nullptr, int pass = 0,
                        int n_tiles = 0)
{
    if (L <= 4 * kScanChunk) {  // one 1024-thread workgroup per row is faster than three launches up to ~16k words
        k_scan_rows<<<frames, 1024, 0, s>>>(data, L, row_stride, totals, add, geom, pass, n_tiles, 0);
        return;
    }
    const int n_chunks = cdiv64(L, kScanChunk);
    k_scan_chunk_sums<<<dim3(n_chunks, frames), 256, 0, s>>>(data, L, row_stride, n_chunks, partial, geom, pass, n_tiles);
    k_scan_rows<<<frames, 1024, 0, s>>>(partial, L, n_chunks, totals, add, geom, pass, n_tiles, 1);
    k_scan_chunk_apply<<<dim3(n_chunks, frames), 256, 0, s>>>(data, L, row_stride, n_chunks, partial, geom, pass, n_tiles);
}

void launch_minmax_init(Profiler* pf, hipStream_t s, float* mm, int64_t mm_stride, int slot, uint32_t* n_kp, int frames)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    k_minmax_init<<<cdiv64(frames * 6, 256), 256, 0, s>>>(mm, mm_stride, slot, n_kp, frames);
}

void launch_set_counts(Profiler* pf, hipStream_t s, uint32_t* n_dev, uint32_t value, int frames)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    k_set_counts<<<cdiv64(frames, 256), 256, 0, s>>>(n_dev, value, frames);
}

void launch_small_frame(Profiler* pf, hipStream_t s, const ReprojectArgs& a, const float* kp_xy, int n_kp, int downsample,
                        const float leaf[3], o3dr_point* pts, o3dr_point* out, CloudCounters* cc, uint32_t* n_out_dev,
                        float* box_out6)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    SmallArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.reproject = 1;
    sa.kp_xy = kp_xy;
    sa.n_kp = n_kp;
    sa.downsample = downsample;
    for (int i = 0; i < 3; ++i) sa.leaf[i] = leaf[i];
    sa.pts = pts;
    sa.out = out;
    sa.cc = cc;
    sa.n_out_dev = n_out_dev;
    sa.box_out6 = box_out6;
    k_small<<<1, kSmallThreads, 0, s>>>(a, sa);
}

void launch_sor_small(Profiler* pf, hipStream_t s, Workspace& ws, const o3dr_point* in, const uint32_t* n_dev, int64_t cap,
                      double stddev_mul, o3dr_point* out, uint32_t* n_out_dev)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    const int64_t cell_stride = (int64_t)ws.grid_max_cells + 1;
    uint32_t max_cells = search_grid_max_cells(cap);
    if (max_cells > ws.grid_max_cells) max_cells = ws.grid_max_cells;
    k_sor_small_prep<<<1, kSmallThreads, 0, s>>>(in, n_dev, max_cells, ws.grid_geom, ws.geom, ws.vals[0], ws.grid_cell_first, ws.grid_xyz,
                                                 ws.sor_left_cnt);
    k_sor_knn<<<dim3(cdiv64(cap, kWave), 1), kWave, 0, s>>>(ws.grid_xyz, ws.vals[0], ws.vals[1], ws.geom, ws.grid_cell_first, cell_stride,
                                                           ws.grid_geom, cap, ws.sor_dist, ws.sor_left, ws.sor_left_cnt);
    int lg = cdiv64(cap, kWave * kSorLeftWaves);
    if (lg > 1024) lg = 1024;
    int zg = cdiv64((int64_t)max_cells, 256);
    if (zg > 256) zg = 256;
    k_sor_cell_z<<<dim3(zg, 1), 256, 0, s>>>(ws.grid_xyz, ws.grid_cell_first, cell_stride, ws.grid_geom, cap, ws.sor_left_cnt, ws.sor_cell_z);
    k_sor_knn_left<<<dim3(lg, 1), kSorLeftWaves * kWave, 0, s>>>(ws.grid_xyz, ws.vals[0], ws.vals[1], ws.geom, ws.grid_cell_first, cell_stride,
                                                                ws.grid_geom, cap, ws.sor_dist, ws.sor_left, ws.sor_left_cnt, ws.sor_cell_z);
    k_sor_small_tail<<<1, kSmallThreads, 0, s>>>(in, ws.sor_dist, ws.grid_geom, stddev_mul, out, n_out_dev);
}

void launch_small_voxel(Profiler* pf, hipStream_t s, const o3dr_point* in, const uint32_t* n_in_dev, uint32_t n_in,
                        const float* box6, const float leaf[3], uint32_t min_points, float z_offset, o3dr_point* out,
                        CloudCounters* cc)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    ReprojectArgs a;
    memset(&a, 0, sizeof a);
    SmallArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.downsample = 1;
    sa.in = in;
    sa.n_in_dev = n_in_dev;
    sa.n_in = n_in;
    sa.box6 = box6;
    for (int i = 0; i < 3; ++i) sa.leaf[i] = leaf[i];
    sa.min_points = min_points;
    sa.z_offset = z_offset;
    sa.out = out;
    sa.cc = cc;
    k_small<<<1, kSmallThreads, 0, s>>>(a, sa);
}

void launch_keypoint_pass(Profiler* pf, hipStream_t s, const ReprojectArgs& a, const float* kp_xy, int n_kp,
                          o3dr_point* out, uint32_t* n_kp_out, float* mm, const int32_t* kp_off, int frames)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    k_keypoint_pass<<<frames, 256, 0, s>>>(a, kp_xy, n_kp, kp_off, out, n_kp_out, mm);
}

void launch_reproject(Profiler* pf, hipStream_t s, const ReprojectArgs& a, int frames, o3dr_point* out,
                      uint32_t* tile_cnt, const uint32_t* n_kp, uint32_t* n_valid, float* mm,
                      uint32_t* scan_partial)
{
    if (a.n_tiles <= 0) {  // jump_pixels == 0: keypoints only
        ProfScope ps(pf, O3DR_K_OTHER, s);
        (void)hipMemcpyAsync(n_valid, n_kp, sizeof(uint32_t) * frames, hipMemcpyDeviceToDevice, s);
        return;
    }
    const dim3 grid(a.n_tiles, frames);
    {
        ProfScope ps(pf, O3DR_K_COUNT, s);
        if (a.disp_f64)
            k_reproject_count<true><<<grid, kEmitThreads, 0, s>>>(a, tile_cnt);
        else
            k_reproject_count<false><<<grid, kEmitThreads, 0, s>>>(a, tile_cnt);
    }
    {
        ProfScope ps(pf, O3DR_K_OTHER, s);
        launch_scan(s, tile_cnt, a.n_tiles, a.n_tiles, frames, n_valid, n_kp, scan_partial);
    }
    {
        ProfScope ps(pf, O3DR_K_REPROJECT, s);
        if (a.disp_f64)
            k_reproject_emit<true, false><<<grid, kEmitThreads, 0, s>>>(a, out, tile_cnt, n_kp, mm, nullptr, 0, nullptr, nullptr, nullptr, 0);
        else
            k_reproject_emit<false, false><<<grid, kEmitThreads, 0, s>>>(a, out, tile_cnt, n_kp, mm, nullptr, 0, nullptr, nullptr, nullptr, 0);
    }
}

static inline int xcd_grid(int64_t n) { return (int)((n + kXcds - 1) / kXcds * kXcds); }  // see xcd_chunk_item
// tile-major histogram rows (hist_at in kernels/radix_sort.inc) where a frame's row fits the one-workgroup scan's LDS
static inline size_t hist_tm_lds(int n_sort_tiles) { return (size_t)n_sort_tiles * (kMaxRadix + 1) * sizeof(uint32_t); }
static inline int hist_tm(int n_sort_tiles) { return hist_tm_lds(n_sort_tiles) <= 48 * 1024 ? 1 : 0; }

// What the launches of a sort of `frames` frames of at most `cap` records are sized by
struct SortShape {
    int64_t cap;
    int frames;
    int n_sort_tiles, n_seg_tiles;
    int64_t hist_row;  // words of one frame's histograms
    int tm;            // tile-major histogram rows, scanned by one workgroup per frame (hist_tm)
    size_t tm_lds;
    SortShape(int64_t cap_, int frames_)
        : cap(cap_), frames(frames_), n_sort_tiles(cdiv64(cap_, kSortTile)), n_seg_tiles(cdiv64(cap_, kSegTile)),
          hist_row((int64_t)kMaxRadix * n_sort_tiles), tm(hist_tm(n_sort_tiles)), tm_lds(hist_tm_lds(n_sort_tiles))
    {
    }
};

// One stable radix pass over ws.keys / ws.vals by the plan in `geom`: digit histograms, their scan, the scatter.
//   have_hist   pass 0 only: ws.hist / ws.hist_part hold the pass's histograms already
//   emit_tiles  > 0: pass 0 runs over the candidate-aligned tiles the emit pass counted (emit_part_range, ws.tile_cnt)
//   side        the last pass of a frame's sort leaves run-head flags there, one byte per record, not the sorted indices
// Always launched; frames whose plan has fewer passes drop out on the device.
static void radix_pass(Profiler* pf, hipStream_t s, Workspace& ws, const SortShape& sh, const VoxelGeom* geom, int pass,
                       bool have_hist = false, int emit_tiles = 0, uint8_t* side = nullptr, int64_t side_stride = 0)
{
    const bool emit = pass == 0 && emit_tiles > 0;
    if (!(pass == 0 && have_hist)) {
        ProfScope ps(pf, O3DR_K_SORT_HIST, s);
        k_radix_hist<<<dim3(sh.n_sort_tiles, sh.frames), kSortThreads, 0, s>>>(ws.keys[0], ws.keys[1], sh.cap, geom, pass, sh.n_sort_tiles,
                                                                                ws.hist, ws.hist_part, sh.tm);
    }
    {
        ProfScope ps(pf, O3DR_K_OTHER, s);
        if (sh.tm)
            k_scan_hist_tm<<<sh.frames, 1024, sh.tm_lds, s>>>(ws.hist, geom, pass, sh.n_sort_tiles, emit ? 1 : 0);
        else
            launch_scan(s, ws.hist, sh.hist_row, sh.hist_row, sh.frames, nullptr, nullptr, ws.scan_partial, geom, pass, sh.n_sort_tiles);
    }
    {
        ProfScope ps(pf, O3DR_K_SORT_SCATTER, s);
        k_radix_scatter_lane<<<dim3(xcd_grid((int64_t)sh.n_sort_tiles * kScatParts), sh.frames), kScatThreads, 0, s>>>(
            ws.keys[0], ws.vals[0], ws.keys[1], ws.vals[1], sh.cap, geom, pass, sh.n_sort_tiles, ws.hist, ws.hist_part, sh.tm,
            emit ? ws.tile_cnt : nullptr, emit_tiles, side, side_stride);
    }
}

// The front of a group-run sort of one cloud: the heads of its group runs (runs of consecutive points of one voxel group)
// per segment tile, their scan -> ws.n_runs, the runs' plan -> ws.geom_runs, the (group, run id) records -> buffer 1 and the
// runs' starts -> ws.run_start.  The heads: recorded while the cloud was appended to (rec_heads: used in place, or with
// shift_n > 0 the shift_n flags from flag shift_first on, moved to ws.head_bits first), else from one read of the points.
static void group_run_front(Profiler* pf, hipStream_t s, Workspace& ws, const SortShape& sh, const o3dr_point* in, float z_offset,
                            const uint8_t* rec_heads, int64_t shift_first, int64_t shift_n, int force_runs, int64_t grp_slots)
{
    const int F = sh.frames, n_seg_tiles = sh.n_seg_tiles;
    const uint8_t* hb = rec_heads && shift_n <= 0 ? rec_heads : ws.head_bits;
    {
        ProfScope ps(pf, O3DR_K_KEYGEN, s);
        if (rec_heads && shift_n > 0) {
            const int64_t bytes = (int64_t)n_seg_tiles * 256;
            k_inc_heads_shift<<<cdiv64(bytes, 256), 256, 0, s>>>(rec_heads, (uint64_t)shift_first, (uint64_t)shift_n, ws.head_bits,
                                                                 (uint64_t)bytes);
        }
        if (rec_heads)
            k_head_counts<<<cdiv64(n_seg_tiles, 4), 256, 0, s>>>(hb, ws.geom, n_seg_tiles, ws.seg_cnt);
        else
            k_group_heads<<<n_seg_tiles, 256, 0, s>>>(in, ws.geom, z_offset, n_seg_tiles, ws.seg_cnt, ws.head_bits);
    }
    {
        ProfScope ps(pf, O3DR_K_OTHER, s);
        launch_scan(s, ws.seg_cnt, n_seg_tiles, n_seg_tiles, F, ws.n_runs, nullptr, ws.scan_partial);
    }
    {
        ProfScope ps(pf, O3DR_K_SEGMENT, s);
        // group runs or points?  (decided per cloud on the device; force_runs: group runs whenever they fit grp_slots)
        k_run_geom<<<cdiv64(F, 64), 64, 0, s>>>(ws.geom, ws.n_runs, F, ws.geom_runs, force_runs, grp_slots);
        // (group, run id) records in buffer 1
        k_run_starts<<<dim3(cdiv64(n_seg_tiles, kStartWaves), F), kStartWaves * kWave, 0, s>>>(
            ws.keys[0], ws.keys[1], sh.cap, ws.geom, n_seg_tiles, ws.seg_cnt, ws.n_runs, ws.run_start, 0, ws.keys[1], ws.geom_runs, in,
            z_offset, hb);
    }
}

// Behind the sort: the runs of equal keys.  Their heads per segment tile (from the sorted keys, or packed from the side bytes
// the last pass left: one launch, every frame by the source of its kind), the scan
// -> ws.n_vox, the runs' starts -> ws.seg_start.
static void segment_runs(Profiler* pf, hipStream_t s, Workspace& ws, const SortShape& sh, const VoxelGeom* geom, const uint8_t* side,
                         int64_t side_stride)
{
    const int F = sh.frames, n_seg_tiles = sh.n_seg_tiles;
    {
        ProfScope ps(pf, O3DR_K_SEGMENT, s);
        const dim3 hgrid(cdiv64(n_seg_tiles, kHeadWaves), F);
        k_run_heads<<<hgrid, kHeadWaves * kWave, 0, s>>>(ws.keys[0], ws.keys[1], sh.cap, geom, n_seg_tiles, ws.seg_cnt, -1, ws.head_bits,
                                                         side, side_stride);
    }
    {
        ProfScope ps(pf, O3DR_K_OTHER, s);
        launch_scan(s, ws.seg_cnt, n_seg_tiles, n_seg_tiles, F, ws.n_vox, nullptr, ws.scan_partial);
    }
    {
        ProfScope ps(pf, O3DR_K_SEGMENT, s);
        k_run_starts<<<dim3(cdiv64(n_seg_tiles, kStartWaves), F), kStartWaves * kWave, 0, s>>>(
            ws.keys[0], ws.keys[1], sh.cap, geom, n_seg_tiles, ws.seg_cnt, ws.n_vox, ws.seg_start, -1, nullptr, nullptr, nullptr, 0.f,
            ws.head_bits);
    }
}

// o3dr_test_corrupt_next_gather: poison one sorted payload in front of the kernels that gather by it
static void corrupt_payload(hipStream_t s, Workspace& ws, const VoxelGeom* geom)
{
    k_test_corrupt_payload<<<1, 1, 0, s>>>(ws.vals[0], ws.vals[1], geom);
}

// rectified-stereo Q and byte disparities: counts + a conservative box from the corners of (x, y, disparity) ranges
// (k_reproject_count_cbox); the exact box only for frames whose conservative one trips PCL's overflow guard
static inline bool fused_cbox(const ReprojectArgs& a, bool conservative_box) { return a.lut != nullptr && !a.disp_f64 && conservative_box; }
bool reproject_fused_inits(const ReprojectArgs& a, bool conservative_box) { return fused_cbox(a, conservative_box); }

// Workgroups of the exact-box pass behind the conservative one.  Nearly always no frame needs it and every workgroup
// returns at once; when frames do (a leaf near PCL's overflow guard, where the conservative box of every frame trips it) the
// grid must still fill the chip: about kExactGrid workgroups over the batch, each walking its share of a frame's tile groups.
// (Four per frame cost such batches 0.2 ms per step: 1080p at voxel_size 0.02 7.68 -> 7.92 ms, 4096x2160 at jump_pixels 4
// 3.12 -> 3.32.)
constexpr int kExactGrid = 8192;
int launch_reproject_fused(Profiler* pf, hipStream_t s, Workspace& ws, const ReprojectArgs& a, int frames, int64_t cap,
                            const float leaf[3], bool conservative_box)
{
    // the emit pass counts the first radix pass's digits where its workgroups own whole rows of the histograms: tile-major
    // rows, and as many sort tiles as groups of kEmitGroup emit tiles (cap = the frame's candidates)
    const SortShape sh(cap, frames);
    const bool counts = sh.tm && cdiv64(a.n_tiles, kEmitGroup) == sh.n_sort_tiles;
    uint32_t* const hist = counts ? ws.hist : nullptr;
    const dim3 grid(cdiv64(a.n_tiles, kEmitGroup), frames);
    const bool cbox = fused_cbox(a, conservative_box);
    const int n_cgroups = cdiv64(a.n_tiles, kCountTiles);
    const dim3 cgrid(n_cgroups, frames);
    {
        ProfScope ps(pf, O3DR_K_COUNT, s);
        const dim3 bgrid(cdiv64(a.n_tiles, kCboxTiles), frames);
        if (cbox && a.vec4 && a.Nx >= 32)  // (with reproject_fused_inits: ws.n_kp and the keypoint slot are this launch's to set)
            k_reproject_count_cbox<kCboxTiles, true><<<bgrid, kEmitThreads, 0, s>>>(a, ws.tile_cnt, ws.mm, ws.n_kp);
        else if (cbox)
            k_reproject_count_cbox<kCboxTiles, false><<<bgrid, kEmitThreads, 0, s>>>(a, ws.tile_cnt, ws.mm, ws.n_kp);
        else if (a.disp_f64)
            k_reproject_bbox_count<true><<<cgrid, kEmitThreads, 0, s>>>(a, ws.tile_cnt, ws.mm, nullptr);
        else
            k_reproject_bbox_count<false><<<cgrid, kEmitThreads, 0, s>>>(a, ws.tile_cnt, ws.mm, nullptr);
    }
    {
        ProfScope ps(pf, O3DR_K_OTHER, s);
        if (a.n_tiles <= 4 * kScanChunk) {  // (launch_scan's one-workgroup form) scan and geometry in one launch
            k_scan_counts_geom<<<frames, 1024, 0, s>>>(ws.tile_cnt, a.n_tiles, ws.n_valid, ws.n_kp, ws.mm, ws.mm_stride, a.n_tiles + 1,
                                                       leaf[0], leaf[1], leaf[2], ws.geom);
        } else {
            launch_scan(s, ws.tile_cnt, a.n_tiles, a.n_tiles, frames, ws.n_valid, ws.n_kp, ws.scan_partial);
            k_voxel_geom<<<frames, 256, 0, s>>>(ws.mm, ws.mm_stride, a.n_tiles + 1, ws.n_valid, leaf[0], leaf[1], leaf[2], 0.f, ws.geom);
        }
    }
    if (cbox) {
        ProfScope ps(pf, O3DR_K_COUNT, s);
        int walkers = cdiv64(kExactGrid, frames);
        if (walkers < 4) walkers = 4;
        const dim3 wgrid(n_cgroups < walkers ? n_cgroups : walkers, frames);
        k_reproject_bbox_count<false><<<wgrid, kEmitThreads, 0, s>>>(a, ws.tile_cnt, ws.mm, ws.geom);
        k_voxel_geom<<<frames, 256, 0, s>>>(ws.mm, ws.mm_stride, a.n_tiles + 1, ws.n_valid, leaf[0], leaf[1], leaf[2], 0.f, ws.geom, 1);
    }
    {
        ProfScope ps(pf, O3DR_K_REPROJECT, s);
        if (a.disp_f64)
            k_reproject_emit<true, true><<<grid, kEmitThreads, 0, s>>>(a, ws.pts, ws.tile_cnt, ws.n_kp, ws.mm, ws.geom, cap, ws.keys[0], hist,
                                                                       ws.hist_part, sh.n_sort_tiles);
        else
            k_reproject_emit<false, true><<<grid, kEmitThreads, 0, s>>>(a, ws.pts, ws.tile_cnt, ws.n_kp, ws.mm, ws.geom, cap, ws.keys[0], hist,
                                                                        ws.hist_part, sh.n_sort_tiles);
    }
    return counts ? a.n_tiles : 0;
}

void launch_transform(Profiler* pf, hipStream_t s, const o3dr_point* in, int64_t n, const float* T16_host,
                      o3dr_point* out)
{
    if (n <= 0) return;
    Mat34 T;
    for (int i = 0; i < 12; ++i) T.m[i] = T16_host[i];
    ProfScope ps(pf, O3DR_K_OTHER, s);
    k_transform<<<cdiv64(n, kPtThreads), kPtThreads, 0, s>>>(in, n, T, out);
}

int launch_points_minmax(Profiler* pf, hipStream_t s, const o3dr_point* in, int64_t in_fstride,
                         const uint32_t* n_dev, int frames, int64_t cap, int64_t mm_stride, float* mm)
{
    if (cap <= 0) return 0;
    int nblk = cdiv64(cap, kPtThreads * 4);
    if (nblk > kMinmaxBlocks) nblk = kMinmaxBlocks;
    ProfScope ps(pf, O3DR_K_OTHER, s);
    k_points_minmax<<<dim3(nblk, frames), kPtThreads, 0, s>>>(in, in_fstride, n_dev, mm_stride, mm);
    return nblk;  // slots written per frame
}

// The voxel grid proper.  Expects ws.mm slots [0, v.mm_used) of every frame to hold bounding boxes of
// the (un-offset) inputs.  In order: geometry, group-run front, keys and first histogram, radix passes, run segmentation,
// min_points filter, (test hook), grouped sums, frame offsets, gather, heads fix, box fold.
void launch_voxel_grid(Profiler* pf, hipStream_t s, Workspace& ws, const VoxelArgs& v)
{
    const int F = v.frames;
    const int64_t cap = v.cap;
    const SortShape sh(cap, F);
    const int n_seg_tiles = sh.n_seg_tiles;
    if (!v.keys_ready) {
        ProfScope ps(pf, O3DR_K_OTHER, s);
        k_voxel_geom<<<F, 256, 0, s>>>(ws.mm, ws.mm_stride, v.mm_used, v.n_dev, v.leaf[0], v.leaf[1], v.leaf[2],
                                       v.z_offset, ws.geom);
    }
    uint32_t* n_keep = nullptr;
    // grouped records: whole-cloud calls only (one cloud; its result slots live in ws.pts)
    // (below ~a million points the extra launches cost more than the point sort saves; use_runs == 2 still forces it)
    const bool use_runs = v.use_runs && !v.passthrough && F == 1 && v.in != ws.pts && (v.use_runs > 1 || cap >= kGroupMinCloud);
    const int64_t grp_slots = use_runs ? ws.grp_slots : 0;
    const int64_t max_groups = grp_slots / kGroupCells;
    // what the sort and the run/cell kernels count (group runs or points)
    const VoxelGeom* sort_geom = use_runs ? ws.geom_runs : ws.geom;
    if (!v.passthrough && cap > 0) {
        // the heads of the group runs: recorded while the cloud was appended to, or from one read of the points
        // (use_runs == 2: group runs whenever they fit the result slots)
        if (use_runs) group_run_front(pf, s, ws, sh, v.in, v.z_offset, v.heads_in, 0, 0, v.use_runs > 1 ? 1 : 0, grp_slots);
        if (use_runs || !v.keys_ready) {
            // PCL's index per point and, for a point sort, the histogram of the first radix pass (a cloud k_run_geom leaves to
            // the point sort needs the indices after all)
            ProfScope ps(pf, O3DR_K_KEYGEN, s);
            k_voxel_keys_hist0<<<dim3(sh.n_sort_tiles, F), kSortThreads, 0, s>>>(v.in, v.in_fstride, ws.geom, v.z_offset, cap, ws.keys[0],
                                                                                 sh.n_sort_tiles, ws.hist, ws.hist_part,
                                                                                 use_runs ? ws.geom_runs : nullptr, sh.tm);
        }
        // the first histogram exists: k_reproject_emit counted it over its candidate-aligned tiles (v.emit_tiles), or
        // k_voxel_keys_hist0 did just now for a point sort (a group-run sort counts its own records in pass 0)
        const bool have_hist0 = v.emit_tiles > 0 || (!use_runs && !v.keys_ready);
        // the last pass of a point sort leaves, instead of the sorted indices, whether each record starts a run, one byte per
        // record (nothing but the run heads reads those indices; the group-run sort's are read by k_centroid_groups)
        uint8_t* const side = use_runs ? nullptr : ws.side;
        const int64_t side_stride = side_frame_stride(cap);
        for (int pass = 0; pass < kMaxPasses; ++pass) radix_pass(pf, s, ws, sh, sort_geom, pass, have_hist0, v.emit_tiles, side, side_stride);
        segment_runs(pf, s, ws, sh, sort_geom, side, side_stride);
        const dim3 sgrid(n_seg_tiles, F);
        if (v.min_points > 1) {  // (grouped clouds filter inside k_centroid_groups and drop out of these on the device)
            {
                ProfScope ps(pf, O3DR_K_SEGMENT, s);
                k_keep_count<<<sgrid, 256, 0, s>>>(ws.seg_start, cap, sort_geom, ws.n_vox, v.min_points, n_seg_tiles, ws.seg_cnt);
            }
            {
                ProfScope ps(pf, O3DR_K_OTHER, s);
                launch_scan(s, ws.seg_cnt, n_seg_tiles, n_seg_tiles, F, ws.n_out, nullptr, ws.scan_partial);
            }
            {
                ProfScope ps(pf, O3DR_K_SEGMENT, s);
                k_keep_write<<<sgrid, 256, 0, s>>>(ws.seg_start, cap, sort_geom, ws.n_vox, v.min_points, n_seg_tiles, ws.seg_cnt,
                                                  ws.keep_idx);
            }
            n_keep = ws.n_out;
        }
        if (v.test_corrupt) corrupt_payload(s, ws, sort_geom);
    }
    if (cap > 0 && use_runs) {
        // one wave per voxel group; the groups' output counts are only known afterwards
        {
            ProfScope ps(pf, O3DR_K_OTHER, s);
            (void)hipMemsetAsync(ws.grp_cnt, 0, sizeof(uint32_t) * (size_t)(max_groups + 1), s);
        }
        {
            ProfScope ps(pf, O3DR_K_CENTROID_RUNS, s);
            int64_t nwg = cdiv64(max_groups < cap ? max_groups : cap, kGroupWaves);
            if (nwg > 16384) nwg = 16384;
            if (nwg < 1) nwg = 1;
            k_centroid_groups<<<(int)nwg, kGroupWaves * kWave, 0, s>>>(
                v.in, ws.keys[0], ws.keys[1], ws.vals[0], ws.vals[1], ws.seg_start, ws.run_start, ws.geom_runs, ws.geom, ws.n_vox,
                v.z_offset, v.min_points, reinterpret_cast<uint4*>(ws.pts), grp_slots, ws.grp_cnt, v.cc);
        }
        {
            ProfScope ps(pf, O3DR_K_OTHER, s);
            launch_scan(s, ws.grp_cnt, max_groups + 1, max_groups + 1, 1, ws.n_grp_out, nullptr, ws.scan_partial);
        }
    }
    {
        ProfScope ps(pf, O3DR_K_OTHER, s);
        k_frame_offsets<<<1, 256, 0, s>>>(ws.geom, ws.n_vox, n_keep, use_runs ? ws.n_grp_out : nullptr, F, v.passthrough,
                                          ws.n_out, ws.out_off, v.cc, v.stats, sort_geom,
                                          (!use_runs && ws.side && !v.passthrough && cap > 0) ? 1 : 0);
    }
    const int nbx = cdiv64(cap, kPtThreads);
    if (cap > 0 && use_runs) {
        ProfScope ps(pf, O3DR_K_CENTROID_RUNS, s);
        int64_t nwg = cdiv64(cap, 256);
        if (nwg > 8192) nwg = 8192;
        k_group_compact<<<(int)nwg, 256, 0, s>>>(v.in, ws.geom_runs, ws.geom, ws.n_vox, ws.grp_cnt,
                                                reinterpret_cast<const uint4*>(ws.pts), ws.out_off, v.z_offset, v.out_base);
    }
    if (cap > 0) {
        ProfScope ps(pf, O3DR_K_CENTROID, s);
        float* out_mm = v.cloud_box ? ws.out_mm : nullptr;
        CloudHeads heads = v.cloud_heads;
        heads.wave_gc = ws.wave_gc;
        const uint32_t* keep = (v.min_points > 1 && !v.passthrough) ? ws.keep_idx : nullptr;
        if (use_runs)  // only for clouds k_run_geom left to the point sort: a small looping grid
            k_centroid<true><<<dim3(nbx < 4096 ? nbx : 4096, F), kPtThreads, 0, s>>>(
                v.in, v.in_fstride, ws.vals[0], ws.vals[1], cap, ws.seg_start, keep, ws.geom_runs, ws.n_out, ws.out_off,
                v.z_offset, v.passthrough, v.out_base, out_mm, nbx, v.cc, CloudHeads{nullptr, {0.f, 0.f, 0.f}, 0.f, nullptr});
        else
            k_centroid<false><<<dim3(xcd_grid(nbx), F), kPtThreads, 0, s>>>(
                v.in, v.in_fstride, ws.vals[0], ws.vals[1], cap, ws.seg_start, keep, ws.geom, ws.n_out, ws.out_off,
                v.z_offset, v.passthrough, v.out_base, out_mm, nbx, v.cc, heads);
        if (!use_runs && v.cloud_heads.flags) {  // the first point of every wave against the last one of the wave before it
            const int wpf = nbx * (kPtThreads / 64);
            k_cloud_heads_fix<<<dim3(cdiv64(wpf, 256), F), 256, 0, s>>>(ws.n_out, ws.out_off, wpf, heads);
        }
    }
    if (v.cloud_box && cap > 0 && !use_runs) {
        ProfScope ps(pf, O3DR_K_OTHER, s);
        const int nbx = cdiv64(cap, kPtThreads) * (kPtThreads / 64);
        k_cloud_bbox_fold<<<kBoxFoldBlocks, 256, 0, s>>>(ws.out_mm, nbx, F, ws.n_out, ws.out_mm_partial);
        k_cloud_bbox_merge<<<1, 384, 0, s>>>(ws.out_mm_partial, kBoxFoldBlocks, v.cloud_box);
    }
}

// The grouped steps of launch_voxel_grid up to the group list (group_run_front, the passes, segment_runs), on the tail of
// an incremental merge; the cloud always takes group runs (its groups are folded by k_inc_fold, which has no point path)
void launch_inc_runs(Profiler* pf, hipStream_t s, Workspace& ws, const o3dr_point* in, int64_t n, const float leaf[3], float z_offset,
                     const uint8_t* rec_heads, int64_t first, int test_corrupt)
{
    const SortShape sh(n, 1);
    {
        ProfScope ps(pf, O3DR_K_OTHER, s);
        k_voxel_geom<<<1, 256, 0, s>>>(ws.mm, ws.mm_stride, 1, ws.n_valid, leaf[0], leaf[1], leaf[2], z_offset, ws.geom);
    }
    group_run_front(pf, s, ws, sh, in, z_offset, rec_heads, first, n, 1, INT64_MAX);
    for (int pass = 0; pass < kMaxPasses; ++pass) radix_pass(pf, s, ws, sh, ws.geom_runs, pass);
    segment_runs(pf, s, ws, sh, ws.geom_runs, nullptr, 0);
    if (test_corrupt) corrupt_payload(s, ws, ws.geom_runs);
}

void launch_inc_fold(Profiler* pf, hipStream_t s, Workspace& ws, const o3dr_point* in, float z_offset, const IncFoldArgs& a,
                     uint32_t* partial)
{
    {
        ProfScope ps(pf, O3DR_K_CENTROID_RUNS, s);
        int64_t nwg = cdiv64(a.nt, kGroupWaves);
        if (nwg > 16384) nwg = 16384;
        if (nwg < 1) nwg = 1;
        k_inc_fold<<<(int)nwg, kGroupWaves * kWave, 0, s>>>(in, ws.keys[0], ws.keys[1], ws.vals[0], ws.vals[1], ws.seg_start, ws.run_start,
                                                            ws.geom_runs, ws.geom, ws.n_vox, z_offset, a.old_g, a.old_off, a.old_cells,
                                                            a.n_old, a.n_old_cells, a.scratch, a.nt, a.tg, a.tmatch, a.cc);
    }
    ProfScope ps(pf, O3DR_K_OTHER, s);
    k_inc_new_flags<<<cdiv64((int64_t)a.nt + 1, 256), 256, 0, s>>>(a.tmatch, a.nt, a.flag);
    launch_scan(s, a.flag, (int64_t)a.nt + 1, (int64_t)a.nt + 1, 1, a.n_new_only, nullptr, partial);
}

void launch_inc_place(Profiler* pf, hipStream_t s, const IncFoldArgs& a, uint32_t n_new, IncGroup* new_g, uint32_t* src,
                      uint32_t* new_off, uint32_t* n_cells_dev, uint32_t* partial)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    (void)hipMemsetAsync(new_off, 0, sizeof(uint32_t) * ((size_t)n_new + 1), s);
    if (a.n_old > 0)
        k_inc_place_old<<<cdiv64(a.n_old, 256), 256, 0, s>>>(a.old_g, a.n_old, a.tg, a.tmatch, a.nt, a.flag, new_g, src, new_off, n_new, a.cc);
    if (a.nt > 0)
        k_inc_place_new<<<cdiv64(a.nt, 256), 256, 0, s>>>(a.old_g, a.n_old, a.tg, a.tmatch, a.nt, a.flag, new_g, src, new_off, n_new, a.cc);
    launch_scan(s, new_off, (int64_t)n_new + 1, (int64_t)n_new + 1, 1, n_cells_dev, nullptr, partial);
}

void launch_inc_copy(Profiler* pf, hipStream_t s, const IncFoldArgs& a, const IncGroup* new_g, const uint32_t* new_off,
                     const uint32_t* src, uint32_t n_new, IncCell* cells, uint32_t cells_cap)
{
    if (n_new == 0) return;
    ProfScope ps(pf, O3DR_K_OTHER, s);
    k_inc_copy<<<cdiv64((int64_t)n_new * kGroupCells, 256), 256, 0, s>>>(new_g, new_off, src, n_new, a.old_off, a.old_cells, a.n_old,
                                                                         a.n_old_cells, a.scratch, a.nt, cells, cells_cap, a.cc);
}

void launch_inc_keep(Profiler* pf, hipStream_t s, const IncGroup* grp, const uint32_t* off, const IncCell* cells, uint32_t n_groups,
                     uint32_t n_cells, uint32_t need, uint32_t* keep_cnt, uint32_t* n_keep_dev, uint32_t* partial)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    (void)hipMemsetAsync(keep_cnt + n_groups, 0, sizeof(uint32_t), s);
    if (n_groups > 0) k_inc_keep_count<<<cdiv64(n_groups, 4), 256, 0, s>>>(grp, off, cells, n_groups, n_cells, need, keep_cnt);
    launch_scan(s, keep_cnt, (int64_t)n_groups + 1, (int64_t)n_groups + 1, 1, n_keep_dev, nullptr, partial);
}

void launch_inc_snapshot(Profiler* pf, hipStream_t s, const IncGroup* grp, const uint32_t* off, const IncCell* cells, uint32_t n_groups,
                         uint32_t n_cells, uint32_t need, const uint32_t* out_off, float z_offset, o3dr_point* out, uint32_t out_cap,
                         CloudCounters* cc)
{
    if (n_groups == 0) return;
    ProfScope ps(pf, O3DR_K_CENTROID, s);
    k_inc_snapshot<<<cdiv64(n_groups, 4), 256, 0, s>>>(grp, off, cells, n_groups, n_cells, need, out_off, z_offset,
                                                       reinterpret_cast<uint4*>(out), out_cap, cc);
}

void launch_inc_box_fold(hipStream_t s, float* box6, const float* tail6, float* mm6) { k_inc_box_fold<<<1, 64, 0, s>>>(box6, tail6, mm6); }

void launch_bilateral(Profiler* pf, hipStream_t s, const uint8_t* src, int64_t src_pitch, int64_t src_fstride, int rows,
                      int cols, int frames, int radius, int maxk, const float* tab, uint8_t* dst, int64_t dst_pitch,
                      int64_t dst_fstride)
{
    if (rows <= 0 || cols <= 0 || frames <= 0) return;
    const int tiles_x = cdiv64(cols, kBilTX), tiles_y = cdiv64(rows, kBilTY);
    const size_t lds = 1024 + (size_t)(kBilTX + 2 * radius) * (kBilTY + 2 * radius);
    ProfScope ps(pf, O3DR_K_OTHER, s);
    k_bilateral_u8<<<dim3(tiles_x * tiles_y, frames), 256, lds, s>>>(src, src_pitch, src_fstride, rows, cols, radius, maxk, tab,
                                                                    dst, dst_pitch, dst_fstride, tiles_x);
}
int bilateral_tile_width(int radius) { return kBilTX + 2 * radius; }

void launch_disp_variance(Profiler* pf, hipStream_t s, const uint8_t* disp, int64_t pitch, int64_t fstride, int rows, int cols,
                          int frames, int bb, int cs, double min_disp, unsigned long long* hist, double* var_out)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    (void)hipMemsetAsync(hist, 0, sizeof(unsigned long long) * 256 * (size_t)frames, s);
    const int roi_rows = rows - 2 * bb;
    for (int f0 = 0; roi_rows > 0 && f0 < frames; f0 += 65535) {  // (a grid's y extent is 16 bits)
        const int nf = frames - f0 < 65535 ? frames - f0 : 65535;
        k_disp_hist<<<dim3(roi_rows, nf), 256, 0, s>>>(disp + (int64_t)f0 * fstride, pitch, fstride, rows, cols, bb, cs, min_disp,
                                                       hist + (int64_t)f0 * 256);
    }
    k_disp_variance<<<cdiv64(frames, 64), 64, 0, s>>>(hist, frames, rows, cols, bb, cs, var_out);
}

template <typename LT>
static void plane_disp_frames(Profiler* pf, hipStream_t s, const PlaneDispArgs& a, int f0, int nf)
{
    const uint8_t* disp = a.disp + (int64_t)f0 * a.dfs;
    const uint8_t* labels = a.labels + (int64_t)f0 * a.lfs;
    unsigned long long* table = a.table + (size_t)f0 * a.n_labels * kPdSums;
    o3dr_plane_disp_segment* rec = a.rec + (size_t)f0 * a.n_labels;
    const int64_t npix = (int64_t)a.rows * a.cols;
    const int tiles_x = cdiv64(a.cols, kPdTileX), tiles_y = cdiv64(a.rows, kPdTileY);
    const int vec = (((uintptr_t)disp | (uintptr_t)labels | (uintptr_t)a.dpitch | (uintptr_t)a.dfs | (uintptr_t)a.lpitch |
                      (uintptr_t)a.lfs) & 15) == 0;
    {
        ProfScope ps(pf, O3DR_K_PLANE_DISP_SUMS, s);
        k_pd_accumulate<LT><<<dim3(tiles_x * tiles_y, nf), 256, 0, s>>>(disp, a.dpitch, a.dfs, labels, a.lpitch, a.lfs, a.rows, a.cols,
                                                                         a.n_labels, a.thr, tiles_x, vec, table, a.flag);
    }
    {
        ProfScope ps(pf, O3DR_K_PLANE_DISP_FIT, s);
        const int64_t n_rec = (int64_t)nf * a.n_labels;
        k_pd_fit<<<cdiv64(n_rec, 256), 256, 0, s>>>(table, n_rec, a.min_pixels, a.max_mse, rec);
    }
    {
        ProfScope ps(pf, O3DR_K_PLANE_DISP_EVAL, s);
        const int64_t pairs = npix / 2 + 1;  // (one more than half: a frame may start on the odd half of a 16-byte pair)
        k_pd_evaluate<LT><<<dim3(cdiv64(pairs, 256 * kPdEvalIter), nf), 256, 0, s>>>(disp, a.dpitch, a.dfs, labels, a.lpitch, a.lfs, a.rows,
                                                                                   a.cols, a.n_labels, a.thr, a.fill, rec,
                                                                                   a.out + (int64_t)f0 * npix);
    }
}
void launch_plane_disp(Profiler* pf, hipStream_t s, const PlaneDispArgs& a)
{
    if (a.frames <= 0 || a.rows <= 0 || a.cols <= 0) return;
    (void)hipMemsetAsync(a.table, 0, sizeof(unsigned long long) * kPdSums * (size_t)a.frames * a.n_labels, s);
    // one launch group: plane_fit_disparity passes at most O3DR_BATCH_FRAMES <= 512 frames, far below a grid's y extent
    if (a.elem == 1) plane_disp_frames<uint8_t>(pf, s, a, 0, a.frames);
    else if (a.elem == 2) plane_disp_frames<uint16_t>(pf, s, a, 0, a.frames);
    else plane_disp_frames<uint32_t>(pf, s, a, 0, a.frames);
}

// ORB features of one group of frames (a.frames <= 65535: the grid's y extent)
void launch_orb(Profiler* pf, hipStream_t s, const OrbArgs& a)
{
    if (a.frames <= 0) return;
    const int F = a.frames;
    {
        ProfScope ps(pf, O3DR_K_ORB_PYRAMID, s);
        const int64_t n0 = (int64_t)a.rows * a.cols;
        if (a.channels == 3)
            k_orb_level0<3, 4><<<dim3(cdiv64(n0, 256 * 4), F), 256, 0, s>>>(a);
        else
            k_orb_level0<1, 16><<<dim3(cdiv64(n0, 256 * 16), F), 256, 0, s>>>(a);
        for (int l = 1; l < a.n_levels; ++l)
            if (a.lv[l].chunks > 0) k_orb_down<<<dim3(cdiv64((int64_t)a.lv[l].w * a.lv[l].h, 256 * 4), F), 256, 0, s>>>(a, l);
    }
    {
        ProfScope ps(pf, O3DR_K_ORB_FAST, s);
        for (int l = 0; l < a.n_levels; ++l) {
            if (a.lv[l].chunks == 0) continue;
            const int tiles_x = cdiv64(a.lv[l].w, kOrbTileX), tiles_y = cdiv64(a.lv[l].h, kOrbTileY);
            k_orb_fast<<<dim3(tiles_x * tiles_y, F), 256, 0, s>>>(a, l, tiles_x);
        }
    }
    {
        ProfScope ps(pf, O3DR_K_ORB_CANDIDATES, s);
        k_orb_candidates<false><<<dim3(a.chunks_per_frame, F), 256, 0, s>>>(a);
        k_orb_scan<<<dim3(a.n_levels, F), 256, 0, s>>>(a);
        k_orb_candidates<true><<<dim3(a.chunks_per_frame, F), 256, 0, s>>>(a);
    }
    {
        ProfScope ps(pf, O3DR_K_ORB_SELECT, s);
        k_orb_select<<<dim3(a.n_levels, F), 256, 0, s>>>(a);
        k_orb_offsets<<<1, 256, 0, s>>>(a);
    }
    {
        ProfScope ps(pf, O3DR_K_ORB_DESCRIBE, s);
        k_orb_describe<<<cdiv64((int64_t)F * a.n_features, kOrbDescWaves), 64 * kOrbDescWaves, 0, s>>>(a);
    }
}

// stereo disparity of one group of frames (a.frames <= 65535: the grid's y extent)
template <int KJ>
static void stereo_frames(Profiler* pf, hipStream_t s, const StereoArgs& a)
{
    static const int kDir[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};
    const int F = a.frames;
    {
        ProfScope ps(pf, O3DR_K_STEREO_PATHS, s);
        for (int r = 0; r < a.n_paths; ++r) {
            const int dx = kDir[r][0], dy = kDir[r][1];
            const int lines = dy == 0 ? a.rows : dx == 0 ? a.cols : a.rows + a.cols - 1;
            k_stereo_path<KJ><<<dim3(cdiv64(lines, 4), F), 256, 0, s>>>(a, dx, dy, r == 0);
        }
    }
    {
        ProfScope ps(pf, O3DR_K_STEREO_WINNER, s);
        const int n_seg = cdiv64(a.cols, kStSeg);
        k_stereo_winner<KJ><<<dim3(cdiv64((int64_t)a.rows * n_seg, 4), F), 256, 0, s>>>(a, n_seg);
        k_stereo_finish<<<dim3(cdiv64((int64_t)a.rows * a.cols, 256), F), 256, 0, s>>>(a);
    }
}
void launch_stereo(Profiler* pf, hipStream_t s, const StereoArgs& a)
{
    if (a.frames <= 0) return;
    {
        ProfScope ps(pf, O3DR_K_STEREO_CENSUS, s);
        const int tiles_x = cdiv64(a.cols, kStTileX), tiles_y = cdiv64(a.rows, kStTileY);
        k_stereo_census<<<dim3(tiles_x * tiles_y, a.frames, 2), 256, 0, s>>>(a, tiles_x);
    }
    switch ((a.D + 63) / 64) {
    case 1: stereo_frames<1>(pf, s, a); break;
    case 2: stereo_frames<2>(pf, s, a); break;
    case 3: stereo_frames<3>(pf, s, a); break;
    default: stereo_frames<4>(pf, s, a); break;
    }
}

// disparity filter of one group of frames (a.frames <= 65535: the grid's y extent); the launches depend on the call's
// switches and the image's size alone
template <class T>
static void disparity_filter_frames(Profiler* pf, hipStream_t s, DfArgs a)
{
    const int F = a.frames;
    const int tiles_x = cdiv64(a.cols, kDfTileX), tiles_y = cdiv64(a.rows, kDfTileY);
    const int px_blocks = cdiv64((int64_t)a.rows * a.cols, 256);
    a.src = a.in;
    if (a.median) {
        ProfScope ps(pf, O3DR_K_DISP_MEDIAN, s);
        if (a.median == 3)
            k_df_median<T, 3><<<dim3(tiles_x * tiles_y, F), 256, 0, s>>>(a.in, a.rows, a.cols, tiles_x, (T*)a.out);
        else
            k_df_median<T, 5><<<dim3(tiles_x * tiles_y, F), 256, 0, s>>>(a.in, a.rows, a.cols, tiles_x, (T*)a.out);
        a.src = DfView{a.out, (int64_t)a.rows * a.cols * (int64_t)sizeof(T), (int64_t)a.cols * (int64_t)sizeof(T)};
    }
    if (a.parent) {
        ProfScope ps(pf, O3DR_K_DISP_LABEL, s);
        k_df_local<T><<<dim3(tiles_x * tiles_y, F), 256, 0, s>>>(a, tiles_x);
        const int n_vert = (tiles_x - 1) * a.rows, n_all = n_vert + (tiles_y - 1) * a.cols;
        if (n_all > 0) k_df_merge<T><<<dim3(cdiv64(n_all, 256), F), 256, 0, s>>>(a, n_vert, n_all);
        k_df_flatten<<<dim3(px_blocks, F), 256, 0, s>>>(a);
        if (a.labels_out || a.sizes_out) k_df_sizes<<<dim3(px_blocks, F), 256, 0, s>>>(a);
    }
    if (a.max_size > 0 || a.info) {
        ProfScope ps(pf, O3DR_K_DISP_SPECKLE, s);
        k_df_apply<T><<<dim3(px_blocks, F), 256, 0, s>>>(a);
    } else if (!a.median) {  // neither filter: out = in
        ProfScope ps(pf, O3DR_K_OTHER, s);
        k_df_apply<T><<<dim3(px_blocks, F), 256, 0, s>>>(a);
    }
}
void launch_disparity_filter(Profiler* pf, hipStream_t s, const DfArgs& a)
{
    if (a.frames <= 0) return;
    if (a.elem == 1)
        disparity_filter_frames<uint8_t>(pf, s, a);
    else
        disparity_filter_frames<uint16_t>(pf, s, a);
}

// multi-view filter and fusion: one launch per 65535 frames (the grid's y extent); the launches depend on the sizes alone
template <class T, bool kFuse>
static void multiview_frames(Profiler* pf, hipStream_t s, MvArgs a)
{
    ProfScope ps(pf, O3DR_K_MULTIVIEW, s);
    const int tiles_x = cdiv64(a.cols, kMvTileX), tiles_y = cdiv64(a.rows, kMvTileY);
    for (int f0 = 0; f0 < a.frames; f0 += 65535) {
        a.f0 = f0;
        const int nf = a.frames - f0 < 65535 ? a.frames - f0 : 65535;
        if (kFuse)
            k_multiview_fuse<T><<<dim3(tiles_x * tiles_y, nf), kMvTileX * kMvTileY, 0, s>>>(a, tiles_x);
        else
            k_multiview_filter<T><<<dim3(tiles_x * tiles_y, nf), kMvTileX * kMvTileY, 0, s>>>(a, tiles_x);
    }
}
template <bool kFuse>
static void multiview_launch(Profiler* pf, hipStream_t s, const MvArgs& a)
{
    if (a.frames <= 0) return;
    if (a.elem == 1)
        multiview_frames<uint8_t, kFuse>(pf, s, a);
    else if (a.elem == 2)
        multiview_frames<uint16_t, kFuse>(pf, s, a);
    else
        multiview_frames<double, kFuse>(pf, s, a);
}
void launch_multiview_filter(Profiler* pf, hipStream_t s, const MvArgs& a) { multiview_launch<false>(pf, s, a); }
void launch_multiview_fuse(Profiler* pf, hipStream_t s, const MvArgs& a) { multiview_launch<true>(pf, s, a); }

// image segmentation of one group of frames (a.frames <= 65535: the grid's y extent); the launches depend on the
// parameters and the image's size alone
void launch_segment_image(Profiler* pf, hipStream_t s, const SegArgs& a)
{
    if (a.frames <= 0) return;
    const int F = a.frames;
    const int tiles_x = cdiv64(a.cols, kDfTileX), tiles_y = cdiv64(a.rows, kDfTileY);
    const int64_t n = (int64_t)a.rows * a.cols;
    const int px_blocks = cdiv64(n, 256), c_blocks = cdiv64((int64_t)a.nx * a.ny, 256);
    {
        ProfScope ps(pf, O3DR_K_SEG_ASSIGN, s);
        k_seg_init<<<dim3(c_blocks, F), 256, 0, s>>>(a);
        for (int k = 0; k < a.iterations; ++k) {
            k_seg_assign<true><<<dim3(tiles_x * tiles_y, F), 256, 0, s>>>(a, tiles_x);
            k_seg_update<<<dim3(c_blocks, F), 256, 0, s>>>(a);
        }
        k_seg_assign<false><<<dim3(tiles_x * tiles_y, F), 256, 0, s>>>(a, tiles_x);
    }
    {
        ProfScope ps(pf, O3DR_K_SEG_LABEL, s);
        DfArgs d;
        memset(&d, 0, sizeof d);
        d.src = DfView{a.raw, n * (int64_t)sizeof(int32_t), (int64_t)a.cols * (int64_t)sizeof(int32_t)};
        d.rows = a.rows, d.cols = a.cols, d.frames = F, d.max_diff = 0;
        d.parent = a.parent, d.cnt = a.cnt;
        k_df_local<DfLabel><<<dim3(tiles_x * tiles_y, F), 256, 0, s>>>(d, tiles_x);
        const int n_vert = (tiles_x - 1) * a.rows, n_all = n_vert + (tiles_y - 1) * a.cols;
        if (n_all > 0) k_df_merge<DfLabel><<<dim3(cdiv64(n_all, 256), F), 256, 0, s>>>(d, n_vert, n_all);
        k_df_flatten<<<dim3(px_blocks, F), 256, 0, s>>>(d);
        k_seg_key<<<dim3(px_blocks, F), 256, 0, s>>>(a);
        k_seg_link<<<dim3(px_blocks, F), 256, 0, s>>>(a);
        k_seg_chase<<<dim3(px_blocks, F), 256, 0, s>>>(a);
        k_seg_flag<<<dim3(px_blocks, F), 256, 0, s>>>(a);
        launch_scan(s, a.flag, n, n, F, nullptr, nullptr, a.partial);
        k_seg_relabel<<<dim3(px_blocks, F), 256, 0, s>>>(a);
    }
}

// stereo rectification: the map of one camera, then one launch per group of frames; both depend on the sizes alone
void launch_rectify_maps(Profiler* pf, hipStream_t s, const RectMapArgs& a)
{
    ProfScope ps(pf, O3DR_K_RECTIFY_MAPS, s);
    k_rectify_maps<<<cdiv64((int64_t)a.rows_out * a.cols_out, 256), 256, 0, s>>>(a);
}
void launch_rectify_remap(Profiler* pf, hipStream_t s, const RectArgs& a)
{
    if (a.frames <= 0) return;
    ProfScope ps(pf, O3DR_K_RECTIFY_REMAP, s);
    const int quads_x = cdiv64(a.cols_out, 4);
    const int blocks = cdiv64((int64_t)a.rows_out * quads_x, 256);
    if (a.channels == 1)
        k_rectify_remap<1><<<blocks, 256, 0, s>>>(a, quads_x);
    else
        k_rectify_remap<3><<<blocks, 256, 0, s>>>(a, quads_x);
}

void launch_bbox(Profiler* pf, hipStream_t s, const float* mm, int used, float* out6)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    k_bbox_fold<<<1, 256, 0, s>>>(mm, used, out6);
}

// Stable partition of `in` (n points, count also in v.n_dev[0]) by index slice of the voxel grid whose
// bounding box sits in ws.mm slot 0.  out = reordered points, counts_dev[n_parts], overflow_dev = 1 when
// PCL's overflow guard fires for that box (then out = in and every count is 0).
void launch_pack_header(hipStream_t s, const float* box6_dev, const CloudCounters* cc, void* hdr32_dev)
{
    k_pack_header<<<1, 1, 0, s>>>(box6_dev, cc, reinterpret_cast<CloudHeader*>(hdr32_dev));
}
void launch_count_from_cc(hipStream_t s, const CloudCounters* cc, uint32_t* n_dev) { k_count_from_cc<<<1, 1, 0, s>>>(cc, n_dev); }
void launch_set_cloud_count(hipStream_t s, CloudCounters* cc, uint64_t n) { k_set_cloud_count<<<1, 1, 0, s>>>(cc, n); }

// hdrs_dev (optional): the box in ws.mm slot 0 is first folded from n_hdrs 32-byte rank headers in HBM
// the two halves of the stable partition by index slice: counts per (part, tile) + their scan (ws.hist, ws.geom: kept for the
// second half) and the slice sizes; then the move, optionally with a shift per part (k_part_move)
void launch_partition_count(Profiler* pf, hipStream_t s, Workspace& ws, const VoxelArgs& v, int n_parts, uint64_t* counts_dev,
                            uint32_t* overflow_dev, const void* hdrs_dev, int n_hdrs)
{
    const SortShape sh(v.cap, 1);
    const int n_sort_tiles = sh.n_sort_tiles;
    ProfScope ps(pf, O3DR_K_OTHER, s);
    if (hdrs_dev) k_fold_headers<<<1, 1, 0, s>>>(reinterpret_cast<const CloudHeader*>(hdrs_dev), n_hdrs, ws.mm);
    k_voxel_geom<<<1, 256, 0, s>>>(ws.mm, ws.mm_stride, 1, v.n_dev, v.leaf[0], v.leaf[1], v.leaf[2], v.z_offset, ws.geom);
    // count per (part, tile), scan; n_parts <= kMaxRadix
    k_part_plan<<<1, 1, 0, s>>>(ws.geom, n_parts);
    k_part_count<<<n_sort_tiles, kSortThreads, 0, s>>>(v.in, ws.geom, v.z_offset, n_parts, n_sort_tiles, ws.hist);
    launch_scan(s, ws.hist, sh.hist_row, sh.hist_row, 1, nullptr, nullptr, ws.scan_partial, ws.geom, 0, n_sort_tiles);
    k_part_counts_scanned<<<cdiv64(n_parts, 64), 64, 0, s>>>(ws.hist, ws.geom, n_parts, n_sort_tiles, counts_dev, overflow_dev);
}
void launch_partition_move(Profiler* pf, hipStream_t s, Workspace& ws, const VoxelArgs& v, int n_parts, o3dr_point* out,
                           const int64_t* part_shift_dev)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    const int n_sort_tiles = cdiv64(v.cap, kSortTile);
    k_part_move<<<n_sort_tiles, kSortThreads, 0, s>>>(v.in, ws.geom, v.z_offset, n_parts, n_sort_tiles, ws.hist, out, part_shift_dev);
}
void launch_partition(Profiler* pf, hipStream_t s, Workspace& ws, const VoxelArgs& v, int n_parts, o3dr_point* out,
                      uint64_t* counts_dev, uint32_t* overflow_dev, const void* hdrs_dev, int n_hdrs)
{
    // (two reads and one write of the cloud)
    launch_partition_count(pf, s, ws, v, n_parts, counts_dev, overflow_dev, hdrs_dev, n_hdrs);
    launch_partition_move(pf, s, ws, v, n_parts, out, nullptr);
}

// `passes` stable radix passes over ws.keys[0] / ws.vals (the plan in ws.geom, frames of at most cap records); the records
// end in buffer passes & 1.  (Runs inside its caller's profiler scope: no scopes of its own.)
static void launch_radix_passes(Workspace& ws, hipStream_t s, int64_t cap, int passes, int frames = 1)
{
    const SortShape sh(cap, frames);
    for (int pass = 0; pass < passes && pass < kMaxPasses; ++pass) radix_pass(nullptr, s, ws, sh, ws.geom, pass);
}

// The search grid of a batch of clouds (see o3dr_device.h): plan, cell ids, radix sort of the cell ids, cell populations,
// points gathered into cell order.  SOR and the nearest-neighbour search (kernels/nn.inc) both build theirs here.
void launch_search_grid(Workspace& ws, hipStream_t s, const o3dr_point* in, int64_t in_fstride, const uint32_t* n_dev, int frames,
                        int64_t cap, int mm_used, double cell_points, uint32_t active_above)
{
    const int F = frames;
    const int64_t cell_stride = (int64_t)ws.grid_max_cells + 1;
    // The cell ids of clouds of at most `cap` points need ceil(log2(max_cells) / 7) sort passes, and only those are launched
    // (a --jump_pixels 15 frame: 2 instead of 5 launch groups that find nothing to do).  The grid is a search structure: the
    // neighbours found do not depend on it.
    uint32_t max_cells = search_grid_max_cells(cap);
    if (max_cells > ws.grid_max_cells) max_cells = ws.grid_max_cells;
    int cell_bits = 1;
    while ((1u << cell_bits) < max_cells) ++cell_bits;
    const int sort_passes = (cell_bits + kMaxRadixBits - 1) / kMaxRadixBits;
    k_sor_plan<<<F, 256, 0, s>>>(ws.mm, ws.mm_stride, mm_used, n_dev, max_cells, ws.grid_geom, ws.geom, cell_points, active_above);
    (void)hipMemsetAsync(ws.grid_cell_first, 0, (size_t)F * (size_t)cell_stride * 4, s);
    k_sor_cells<<<dim3(cdiv64(cap, 256), F), 256, 0, s>>>(in, in_fstride, ws.grid_geom, cap, ws.keys[0]);
    launch_radix_passes(ws, s, cap, sort_passes, F);
    k_sor_cell_counts<<<dim3(cdiv64(cap, 256), F), 256, 0, s>>>(ws.keys[0], ws.keys[1], ws.geom, ws.grid_geom, cap, cell_stride, ws.grid_cell_first);
    launch_scan(s, ws.grid_cell_first, cell_stride, cell_stride, F, nullptr, nullptr, ws.scan_partial);
    k_sor_gather<<<dim3(cdiv64(cap, 256), F), 256, 0, s>>>(in, in_fstride, ws.vals[0], ws.vals[1], ws.grid_geom, ws.geom, cap, ws.grid_xyz);
}

// Statistical outlier removal of a batch of clouds (see o3dr_device.h).  cap, at most what ws.grid_* and ws.sor_* were
// carved for, sizes the grids and is the arrays' frame stride.
int launch_sor(Profiler* pf, hipStream_t s, Workspace& ws, const o3dr_point* in, int64_t in_fstride, const uint32_t* n_dev,
               int frames, int64_t cap, int mm_used, double stddev_mul, o3dr_point* out, int64_t out_fstride,
               uint32_t* n_out_dev)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    const int F = frames;
    const int n_tiles = cdiv64(cap, 1024);
    const int64_t cell_stride = (int64_t)ws.grid_max_cells + 1;
    launch_search_grid(ws, s, in, in_fstride, n_dev, F, cap, mm_used, kSorCellPoints, (uint32_t)kSorMeanK);
    (void)hipMemsetAsync(ws.sor_left_cnt, 0, (size_t)F * 4, s);
    k_sor_knn<<<dim3(cdiv64(cap, kWave), F), kWave, 0, s>>>(ws.grid_xyz, ws.vals[0], ws.vals[1], ws.geom, ws.grid_cell_first, cell_stride,
                                                           ws.grid_geom, cap, ws.sor_dist, ws.sor_left, ws.sor_left_cnt);
    {   // the queries the wave-shared search handed over (a looping grid: their number is only known on the device)
        int lg = cdiv64(cap, kWave * kSorLeftWaves);
        if (lg > 1024) lg = 1024;
        int zg = cdiv64((int64_t)ws.grid_max_cells, 256);
        if (zg > 256) zg = 256;
        k_sor_cell_z<<<dim3(zg, F), 256, 0, s>>>(ws.grid_xyz, ws.grid_cell_first, cell_stride, ws.grid_geom, cap, ws.sor_left_cnt, ws.sor_cell_z);
        k_sor_knn_left<<<dim3(lg, F), kSorLeftWaves * kWave, 0, s>>>(ws.grid_xyz, ws.vals[0], ws.vals[1], ws.geom, ws.grid_cell_first, cell_stride,
                                                                    ws.grid_geom, cap, ws.sor_dist, ws.sor_left, ws.sor_left_cnt, ws.sor_cell_z);
    }
    k_sor_partial<<<dim3(kSorStatBlocks, F), 256, 0, s>>>(ws.sor_dist, cap, ws.grid_geom, ws.sor_partial);
    k_sor_threshold<<<cdiv64(F, 64), 64, 0, s>>>(ws.sor_partial, stddev_mul, ws.grid_geom, F);
    k_sor_count<<<dim3(n_tiles, F), 256, 0, s>>>(ws.sor_dist, cap, ws.grid_geom, n_tiles, ws.tile_cnt);
    launch_scan(s, ws.tile_cnt, n_tiles, n_tiles, F, n_out_dev, nullptr, ws.scan_partial);
    k_sor_emit<<<dim3(n_tiles, F), 256, 0, s>>>(in, in_fstride, ws.sor_dist, cap, ws.grid_geom, n_tiles, ws.tile_cnt, out, out_fstride,
                                                ws.mm_stride, ws.mm);
    return n_tiles;
}

// Nearest neighbour (kernels/nn.inc).  launch_nn_grid: the target's search grid in ws.grid_* (its n points counted in
// ws.n_valid[0], its bounding-box slots in ws.mm [0, mm_used)), the folded box -> box6 and the cells' exact boxes.  The
// one place that knows where the members of a SearchGrid live.
SearchGrid launch_nn_grid(Profiler* pf, hipStream_t s, Workspace& ws, const o3dr_point* target, int64_t n, int mm_used, float* box6,
                          float4* cell_lo, float4* cell_hi)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    k_bbox_fold<<<1, 256, 0, s>>>(ws.mm, mm_used, box6);
    launch_search_grid(ws, s, target, 0, ws.n_valid, 1, n, mm_used, kNnCellPoints, 0u);
    int cg = cdiv64((int64_t)ws.grid_max_cells, 256);
    if (cg > 4096) cg = 4096;
    k_nn_cell_box<<<cg, 256, 0, s>>>(ws.grid_xyz, ws.grid_cell_first, ws.grid_geom, cell_lo, cell_hi);
    return SearchGrid{ws.grid_geom, ws.grid_xyz, ws.grid_cell_first, cell_lo, cell_hi, box6};
}

void launch_nn_query(Profiler* pf, hipStream_t s, const SearchGrid& grid, const o3dr_point* query, int64_t n, const float* T12,
                     float r2, uint32_t* idx_out, float* d2_out, const uint32_t* idx_prev, const double c0[3], double* partial,
                     double* rec)
{
    if (n <= 0) return;
    ProfScope ps(pf, O3DR_K_OTHER, s);
    NnArgs a;
    memset(&a, 0, sizeof a);
    a.query = query;
    a.n = (uint32_t)n;
    a.xf = T12 ? 1 : 0;
    for (int k = 0; k < 12; ++k) a.T.m[k] = T12 ? T12[k] : 0.f;
    a.grid = grid;
    a.r2 = r2;
    a.idx_out = idx_out;
    a.d2_out = d2_out;
    a.idx_prev = idx_prev;
    for (int k = 0; k < 3; ++k) a.c0[k] = c0 ? c0[k] : 0.0;
    a.partial = partial;
    a.n_blocks = (uint32_t)cdiv64(n, kNnThreads);
    k_nn_query<<<a.n_blocks, kNnThreads, 0, s>>>(a);
    if (partial) k_icp_fold<<<kIcpFields, kRigidFoldThreads, 0, s>>>(partial, a.n_blocks, rec);
}

void launch_cloud_finite(Profiler* pf, hipStream_t s, const o3dr_point* in, int64_t n, uint32_t* flag)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    (void)hipMemsetAsync(flag, 0, 4, s);
    if (n <= 0) return;
    int g = cdiv64(n, 256);
    if (g > 4096) g = 4096;
    k_cloud_finite<<<g, 256, 0, s>>>(in, n, flag);
}

// Moving least squares (kernels/mls.inc) over the grid launch_nn_grid built for `cloud`
void launch_mls(Profiler* pf, hipStream_t s, const SearchGrid& grid, const o3dr_point* cloud, int64_t n, double r, int order,
                double h, o3dr_point* out, float* normals, uint32_t* nn_count, uint8_t* fit, unsigned long long* counters)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    (void)hipMemsetAsync(counters, 0, 4 * sizeof(unsigned long long), s);
    if (n <= 0) return;
    MlsArgs a;
    memset(&a, 0, sizeof a);
    a.cloud = cloud;
    a.n = (uint32_t)n;
    a.grid = grid;
    a.r2 = (float)(r * r);
    a.r = r;
    a.inv_h = 1.0 / h;
    a.pad_r = grid_pad_radius(r);
    a.out = out;
    a.normals = normals;
    a.nn_count = nn_count;
    a.fit = fit;
    a.counters = counters;
    const int blocks = cdiv64(n, kMlsThreads);
    if (order == 0)
        k_mls<0><<<blocks, kMlsThreads, 0, s>>>(a);
    else if (order == 1)
        k_mls<1><<<blocks, kMlsThreads, 0, s>>>(a);
    else
        k_mls<2><<<blocks, kMlsThreads, 0, s>>>(a);
}

// Stable sort of the n nbits-wide keys in ws.keys[0], the payload being the input position: at least one pass (it also
// writes the payload).  Returns the buffer the sorted records end in.
__global__ void k_set_sort_geom(VoxelGeom* geom, VoxelGeom g) { *geom = g; }
static int launch_sort_keys(Workspace& ws, hipStream_t s, uint32_t n, int nbits)
{
    VoxelGeom g;
    memset(&g, 0, sizeof g);
    for (int k = 0; k < 3; ++k) g.inv[k] = 1.f, g.div_b[k] = 1;
    g.mul1 = g.mul2 = 1;
    g.n = n;
    if (nbits < 1) nbits = 1;
    g.passes = (uint32_t)((nbits + kMaxRadixBits - 1) / kMaxRadixBits);
    g.bpp = (uint32_t)((nbits + (int)g.passes - 1) / (int)g.passes);
    k_set_sort_geom<<<1, 1, 0, s>>>(ws.geom, g);
    launch_radix_passes(ws, s, n, (int)g.passes);
    return (int)(g.passes & 1u);
}

// The dense XY cell order (kernels/cell_order.inc); cell_of(a) is the operator's index rule
template <class Args>
void launch_cell_range(Profiler* pf, hipStream_t s, const Args& a, uint32_t* part, uint32_t* range)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    const int g = (int)cell_range_parts(a.n);
    k_cell_range<<<g, kCellThreads, 0, s>>>(a.cloud, (int64_t)a.n, cell_of(a), part);
    k_fold4_u32<<<1, kFoldThreads, 0, s>>>(part, g, 0, 0, 1, 0, 1, range);
    k_fold4_u32<<<1, kFoldThreads, 0, s>>>(part, g, 4, 1, 1, 1, 1, range + 4);
}
template <class Args>
void launch_cell_order(Profiler* pf, hipStream_t s, Workspace& ws, Args& a, int nbits, uint32_t* head, uint32_t* n_runs_dev)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    CellOrder& o = a.cells;
    o.n = a.n;
    const int g = cdiv64(o.n, kCellThreads);
    k_cell_keys<<<g, kCellThreads, 0, s>>>(a.cloud, o.n, cell_of(a), o.x0, o.y0, o.wx, ws.keys[0]);
    const int sorted = launch_sort_keys(ws, s, o.n, nbits);
    o.keys = ws.keys[sorted];
    o.perm = ws.vals[sorted];
    o.ord = head;
    o.n_runs = n_runs_dev;
    k_cell_heads<<<g, kCellThreads, 0, s>>>(o, head);
    launch_scan(s, head, o.n, o.n, 1, n_runs_dev, nullptr, ws.scan_partial);
}
template void launch_cell_range<PlaneArgs>(Profiler*, hipStream_t, const PlaneArgs&, uint32_t*, uint32_t*);
template void launch_cell_range<MeshArgs>(Profiler*, hipStream_t, const MeshArgs&, uint32_t*, uint32_t*);
template void launch_cell_range<RasterFrame>(Profiler*, hipStream_t, const RasterFrame&, uint32_t*, uint32_t*);
template void launch_cell_order<PlaneArgs>(Profiler*, hipStream_t, Workspace&, PlaneArgs&, int, uint32_t*, uint32_t*);
template void launch_cell_order<MeshArgs>(Profiler*, hipStream_t, Workspace&, MeshArgs&, int, uint32_t*, uint32_t*);

// RANSAC plane segmentation (kernels/plane.inc)
void launch_plane_tiles(Profiler* pf, hipStream_t s, Workspace& ws, const PlaneArgs& a, float4* pts)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    if (a.tiled) k_plane_gather<<<cdiv64(a.n, 256), 256, 0, s>>>(a, pts);
    k_plane_tiles<<<a.tiled ? cdiv64(a.n, 256) : 1, 256, 0, s>>>(a);
    k_plane_chunks<<<cdiv64(a.n_tiles, 256), 256, 0, s>>>(a);
    launch_scan(s, a.cfirst, a.n_tiles, a.n_tiles, 1, a.cfirst + a.n_tiles, nullptr, ws.scan_partial);
}

void launch_plane_fit(Profiler* pf, hipStream_t s, const PlaneArgs& a, int64_t max_chunks, int optimize)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    const uint64_t nh = (uint64_t)a.n_tiles * a.H;
    (void)hipMemsetAsync(a.counts, 0, nh * sizeof(uint32_t), s);
    k_plane_sample<<<(unsigned)((nh + 255) / 256), 256, 0, s>>>(a);
    constexpr int wpb = kPlaneThreads / kWave;
    const int chunk_blocks = cdiv64(max_chunks, wpb);  // waves past the chunk count return at once
    k_plane_score<<<chunk_blocks, kPlaneThreads, 0, s>>>(a, a.hyp, a.counts);
    k_plane_best<<<a.n_tiles, kWave, 0, s>>>(a);
    if (optimize) {
        k_plane_moments<<<chunk_blocks, kPlaneThreads, 0, s>>>(a);
        k_plane_refine<<<a.n_tiles, kWave, 0, s>>>(a);
    }
    k_plane_label<<<chunk_blocks, kPlaneThreads, 0, s>>>(a);
}

// feature matching (kernels/match.inc)
void launch_match(Profiler* pf, hipStream_t s, const MatchArgs& a, const MatchPair* pairs, uint2* partial)
{
    ProfScope ps(pf, O3DR_K_MATCH, s);
    constexpr int wpb = kMatchThreads / kWave;
    for (int64_t off = 0; off < (int64_t)a.n_items; off += kMatchSliceItems) {
        const int64_t items = (int64_t)a.n_items - off < kMatchSliceItems ? (int64_t)a.n_items - off : kMatchSliceItems;
        k_match_scan<<<cdiv64(items, wpb), kMatchThreads, 0, s>>>(a, pairs, a.desc, partial, (uint64_t)off);
    }
    int64_t g = cdiv64((int64_t)a.n_rec, 256);
    if (g > 65536) g = 65536;
    if (g > 0) k_match_fold<<<(unsigned)g, 256, 0, s>>>(a, pairs, partial);
}

void launch_keypoints_3d(Profiler* pf, hipStream_t s, const ReprojectArgs& a, const float* kp_xy, const int32_t* kp_off, int n_frames,
                         int n_kp, o3dr_point* out)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    if (n_kp > 0) k_keypoints_3d<<<cdiv64(n_kp, 256), 256, 0, s>>>(a, kp_xy, kp_off, n_frames, n_kp, out);
}

void launch_rigid(Profiler* pf, hipStream_t s, const RigidArgs& a, bool residual)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    const int F = residual ? 1 : kRigidFields;
    if (a.n_blocks > 0) {
        if (residual) {
            k_rigid_sums<true><<<a.n_blocks, kRigidThreads, 0, s>>>(a);
        } else {
            (void)hipMemsetAsync(a.first, 0xff, (size_t)a.n_segs * 4, s);
            k_rigid_first<<<a.n_blocks, kRigidThreads, 0, s>>>(a);
            k_rigid_sums<false><<<a.n_blocks, kRigidThreads, 0, s>>>(a);
        }
    } else if (!residual) {
        (void)hipMemsetAsync(a.first, 0xff, (size_t)a.n_segs * 4, s);
    }
    RigidArgs b = a;
    if (residual) {
        b.rec = a.rec + (size_t)a.n_segs * kRigidFields;
        b.c0 = nullptr;
    }
    k_rigid_fold<<<dim3(a.n_segs, F), kRigidFoldThreads, 0, s>>>(b, F);
}

// pose chain (kernels/pose_chain.inc): one workgroup, the frames in order
void launch_pose_chain(Profiler* pf, hipStream_t s, const ChainArgs& a)
{
    ProfScope ps(pf, O3DR_K_POSE_CHAIN, s);
    if (a.n_fixed < a.n_frames) k_pose_chain<<<1, kChainThreads, 0, s>>>(a);
}

// three-point RANSAC (kernels/ransac.inc): one workgroup per segment / pair
void launch_ransac(Profiler* pf, hipStream_t s, const RansacArgs& a, bool chain)
{
    ProfScope ps(pf, O3DR_K_RANSAC, s);
    if (a.n_segs == 0) return;
    if (chain)
        k_ransac_rigid<true><<<a.n_segs, kRansacThreads, 0, s>>>(a);
    else
        k_ransac_rigid<false><<<a.n_segs, kRansacThreads, 0, s>>>(a);
}

// pose-graph refinement (kernels/pose_graph.inc): the moments, one workgroup per pair; the solve, one workgroup
void launch_graph_moments(Profiler* pf, hipStream_t s, const GraphMomArgs& a)
{
    ProfScope ps(pf, O3DR_K_GRAPH_MOMENTS, s);
    if (a.n_pairs > 0) k_graph_moments<<<a.n_pairs, kGraphRun, 0, s>>>(a);
}

void launch_graph_solve(Profiler* pf, hipStream_t s, const GraphArgs& a)
{
    ProfScope ps(pf, O3DR_K_GRAPH_SOLVE, s);
    if (a.n_frames > 0) k_graph_solve<<<1, kGraphThreads, 0, s>>>(a);
}

// height-field surface mesh (kernels/mesh.inc)
void launch_mesh_count(Profiler* pf, hipStream_t s, Workspace& ws, const MeshArgs& a, uint32_t* n_tris_dev)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    const int64_t n = a.n;
    const int g = cdiv64(n, kMeshThreads);
    k_mesh_vertices<<<g, kMeshThreads, 0, s>>>(a);
    k_mesh_count<<<g, kMeshThreads, 0, s>>>(a);
    k_fold4_u32<<<1, kFoldThreads, 0, s>>>(a.part, g, 0, 2, 2, 2, 2, a.counters);
    launch_scan(s, a.cnt, n, n, 1, n_tris_dev, nullptr, ws.scan_partial);
}

void launch_mesh_emit(Profiler* pf, hipStream_t s, const MeshArgs& a)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    const int64_t n = a.n;
    if (a.tris) k_mesh_emit<<<cdiv64(n, kMeshThreads), kMeshThreads, 0, s>>>(a);
    if (a.normals) k_mesh_normals<<<cdiv64(n, kMeshThreads), kMeshThreads, 0, s>>>(a);
}

// map raster (kernels/raster.inc)
void launch_raster(Profiler* pf, hipStream_t s, const RasterArgs& a)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    const RasterFrame& f = a.f;
    const int64_t cells = (int64_t)f.width * f.height;
    (void)hipMemsetAsync(a.win, 0xff, (size_t)cells * sizeof(unsigned long long), s);
    const int gw = (int)raster_winner_parts(f.n);
    if (gw > 0) k_raster_winner<<<gw, kRasterThreads, 0, s>>>(a);
    k_fold4_u32<<<1, kFoldThreads, 0, s>>>(f.part, gw, 0, 2, 2, 2, 2, a.counters);
    const int gc = cdiv64(cells, kRasterThreads);
    if (a.R > 0) k_raster_fill_col<<<gc, kRasterThreads, 0, s>>>(a);
    const int gt = (int)raster_tiles(f.width, f.height);
    k_raster_resolve<<<gt, kRasterThreads, 0, s>>>(a);
    k_fold4_u32<<<1, kFoldThreads, 0, s>>>(f.part, gt, 0, 2, 2, 2, 2, a.counters + 4);
    k_fold4_u32<<<1, kFoldThreads, 0, s>>>(f.part, gt, 4, 0, 1, 2, 2, a.counters + 8);
    if (a.shade) k_raster_shade<<<gc, kRasterThreads, 0, s>>>(a);
}

// ground filter (kernels/ground.inc)
void launch_ground(Profiler* pf, hipStream_t s, const GroundArgs& a)
{
    const RasterArgs& r = a.r;
    const RasterFrame& f = r.f;
    const int64_t cells = (int64_t)f.width * f.height;
    const int gc = cdiv64(cells, kGroundThreads);
    const int gw = (int)raster_winner_parts(f.n);
    {
        ProfScope ps(pf, O3DR_K_GROUND_WINNER, s);
        (void)hipMemsetAsync(r.win, 0xff, (size_t)cells * sizeof(unsigned long long), s);
        if (gw > 0) k_raster_winner<<<gw, kRasterThreads, 0, s>>>(r);
        k_fold4_u32<<<1, kFoldThreads, 0, s>>>(f.part, gw, 0, 2, 2, 2, 2, a.counters);
        k_ground_init<<<gc, kGroundThreads, 0, s>>>(a);
    }
    const int64_t tiles_x = ((int64_t)f.width + kGroundTileW - 1) / kGroundTileW, gx = ground_col_groups(f.width);
    const unsigned g_row = (unsigned)(tiles_x * f.height);
    for (int k = 0; k < a.n_iter; ++k) {
        ProfScope ps(pf, O3DR_K_GROUND_ITER, s);
        const int rad = a.radius[k];
        int p = 1;
        while (2 * p <= 2 * rad + 1) p *= 2;  // the largest power of two within the window
        const unsigned g_col = (unsigned)(gx * ground_col_rows(f.height, rad));
        k_ground_row<false><<<g_row, kGroundThreads, 0, s>>>(a.zl, a.t1, f.width, tiles_x, rad, p);
        k_ground_col_suffix<false><<<g_col, kGroundThreads, 0, s>>>(a.t1, a.run, f.width, f.height, gx, rad);
        k_ground_col_window<false><<<g_col, kGroundThreads, 0, s>>>(a, a.t1, gx, rad, 0.f, 0);
        k_ground_row<true><<<g_row, kGroundThreads, 0, s>>>(a.t2, a.t1, f.width, tiles_x, rad, p);
        k_ground_col_suffix<true><<<g_col, kGroundThreads, 0, s>>>(a.t1, a.run, f.width, f.height, gx, rad);
        k_ground_col_window<true><<<g_col, kGroundThreads, 0, s>>>(a, a.t1, gx, rad, a.thr[k], (uint8_t)(2 + k));
        k_fold4_u32<<<1, kFoldThreads, 0, s>>>(f.part, (int)g_col, 0, 2, 2, 2, 2, a.counters + 16 + 4 * k);
    }
    {
        ProfScope ps(pf, O3DR_K_GROUND_FILL, s);
        k_ground_ground_words<<<gc, kGroundThreads, 0, s>>>(a);
        if (r.R > 0) k_raster_fill_col<<<gc, kRasterThreads, 0, s>>>(r);
        const int gt = (int)raster_tiles(f.width, f.height);
        k_raster_resolve<<<gt, kRasterThreads, 0, s>>>(r);
        k_fold4_u32<<<1, kFoldThreads, 0, s>>>(f.part, gt, 0, 2, 2, 2, 2, a.counters + 4);
    }
    {
        ProfScope ps(pf, O3DR_K_GROUND_POINTS, s);
        if (gw > 0) k_ground_points<<<gw, kGroundThreads, 0, s>>>(a);
        k_fold4_u32<<<1, kFoldThreads, 0, s>>>(f.part, gw, 0, 2, 2, 2, 2, a.counters + 12);
    }
}

// raster interpolation (kernels/interpolate.inc)
void launch_interpolate(Profiler* pf, hipStream_t s, const InterpArgs& a)
{
    const int lt = interp_top_level(a);
    {
        ProfScope ps(pf, O3DR_K_INTERP_PULL, s);
        (void)hipMemsetAsync(a.bad, 0, sizeof(uint32_t), s);
        int pulled = 0;
        while (pulled < lt) {  // (level pulled + 1 then has at most 32 x 32 cells)
            const int nl = a.L - pulled < kInterpPullLevels ? a.L - pulled : kInterpPullLevels;
            const int64_t tiles = interp_pull_tiles(a.lv[pulled]), tiles_x = ((int64_t)a.lv[pulled].W + kInterpPullTile - 1) / kInterpPullTile;
            k_interp_pull<<<(unsigned)interp_blocks(tiles), kInterpThreads, 0, s>>>(a, pulled, nl, tiles_x, tiles);
            pulled += nl;
        }
        if (a.L > 0) k_interp_top<<<1, kInterpThreads, 0, s>>>(a, pulled, lt);
    }
    {
        ProfScope ps(pf, O3DR_K_INTERP_PUSH, s);
        const int64_t t = interp_push_tile(a.smooth);
        for (int l = (lt > 1 ? lt : 1) - 1; l >= 0; --l) {
            const int64_t tiles = interp_push_tiles(a.lv[l], a.smooth), tiles_x = ((int64_t)a.lv[l].W + t - 1) / t;
            const unsigned g = (unsigned)interp_blocks(tiles);
            if (l > 0) {
                k_interp_push<false><<<g, kInterpThreads, 0, s>>>(a, l, tiles_x, tiles);
            } else {
                k_interp_push<true><<<g, kInterpThreads, 0, s>>>(a, l, tiles_x, tiles);
                k_interp_fold<<<1, kFoldThreads, 0, s>>>(a.part, (int)g, a.counters);
            }
        }
    }
}

// raster sample (kernels/interpolate.inc)
void launch_raster_sample(Profiler* pf, hipStream_t s, const SampleArgs& a)
{
    ProfScope ps(pf, O3DR_K_RASTER_SAMPLE, s);
    const int g = (int)raster_winner_parts(a.f.n);
    if (g > 0) k_raster_sample<<<g, kInterpThreads, 0, s>>>(a);
    k_fold4_u32<<<1, kFoldThreads, 0, s>>>(a.f.part, g, 0, 2, 2, 2, 2, a.counters);
}

// contour lines (kernels/contour.inc)
static inline unsigned contour_grid(int64_t n)
{
    const int64_t b = contour_blocks(n);
    return (unsigned)(b < kContourMaxBlocks ? b : kContourMaxBlocks);
}
void launch_contour_count(Profiler* pf, hipStream_t s, const ContourArgs& a)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    (void)hipMemsetAsync(a.flags, 0, 2 * sizeof(uint32_t), s);
    (void)hipMemsetAsync(a.counters, 0, kContourCounterWords * sizeof(uint32_t), s);
    k_contour_levels<<<contour_grid((int64_t)a.W * a.H), kContourThreads, 0, s>>>(a);
    if (a.n_quads == 0) return;
    const unsigned g = contour_grid(a.n_quads);
    k_contour_count<<<g, kContourThreads, 0, s>>>(a);
    k_fold4_u32<<<1, kFoldThreads, 0, s>>>(a.part, (int)g, 0, 2, 2, 0, 1, a.counters);
    launch_scan(s, a.off, a.n_quads, a.n_quads, 1, nullptr, nullptr, a.scan_partial);
}

void launch_contour_lines(Profiler* pf, hipStream_t s, const ContourArgs& a)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    const int g = (int)contour_blocks(a.n_seg);
    k_contour_emit<<<contour_grid(a.n_quads), kContourThreads, 0, s>>>(a);
    (void)hipMemsetAsync(a.prev, 0xff, (size_t)a.n_seg * sizeof(int), s);
    (void)hipMemsetAsync(a.head, 0xff, (size_t)a.n_seg * sizeof(int), s);
    (void)hipMemsetAsync(a.cnt, 0, (size_t)a.n_seg * sizeof(uint32_t), s);
    k_cluster_init<<<g, kClusterThreads, 0, s>>>(a.parent, a.n_seg);
    k_contour_link<<<g, kContourThreads, 0, s>>>(a);
    k_contour_flatten<<<g, kContourThreads, 0, s>>>(a);
    k_contour_flags<<<g, kContourThreads, 0, s>>>(a);
    k_fold4_u32<<<1, kFoldThreads, 0, s>>>(a.part, g, 0, 2, 1, 2, 2, a.counters + 4);
    launch_scan(s, a.num, a.n_seg, a.n_seg, 1, a.counters + 8, nullptr, a.scan_partial);
    launch_scan(s, a.beg, a.n_seg, a.n_seg, 1, a.counters + 9, nullptr, a.scan_partial);
    const int rounds = contour_rank_rounds(a.n_seg);
    for (int r = 0; r < rounds; ++r) k_contour_jump<<<g, kContourThreads, 0, s>>>(a.jump[r & 1], a.jump[(r + 1) & 1], a.n_seg);
}

void launch_contour_outputs(Profiler* pf, hipStream_t s, const ContourArgs& a)
{
    ProfScope ps(pf, O3DR_K_OTHER, s);
    k_contour_outputs<<<(int)contour_blocks(a.n_seg), kContourThreads, 0, s>>>(a, a.jump[contour_rank_rounds(a.n_seg) & 1]);
}

// Euclidean clustering (kernels/cluster.inc) over the grid launch_nn_grid left in ws.sor_*
void launch_cluster_link(Profiler* pf, hipStream_t s, Workspace& ws, const ClusterArgs& a)
{
    const int g = (int)cluster_blocks(a.n);
    {
        ProfScope ps(pf, O3DR_K_CLUSTER_LINK, s);
        (void)hipMemsetAsync(a.n_pairs, 0, sizeof(unsigned long long), s);
        k_cluster_init<<<g, kClusterThreads, 0, s>>>(a.parent, a.n);
        k_cluster_link<<<g, kClusterThreads, 0, s>>>(a);
    }
    {
        ProfScope ps(pf, O3DR_K_CLUSTER_NUMBER, s);
        (void)hipMemsetAsync(a.cnt, 0, (size_t)a.n * sizeof(uint32_t), s);
        k_cluster_flatten<<<g, kClusterThreads, 0, s>>>(a);
        k_cluster_flags<<<g, kClusterThreads, 0, s>>>(a);
        k_fold4_u32<<<1, kFoldThreads, 0, s>>>(a.part, g, 0, 2, 2, 2, 1, a.counters);
        k_fold4_u32<<<1, kFoldThreads, 0, s>>>(a.part, g, 4, 2, 2, 2, 2, a.counters + 4);
        launch_scan(s, a.num, a.n, a.n, 1, a.counters + 8, nullptr, ws.scan_partial);
        launch_scan(s, a.beg, a.n, a.n, 1, a.counters + 9, nullptr, ws.scan_partial);
    }
}

void launch_cluster_outputs(Profiler* pf, hipStream_t s, Workspace& ws, const ClusterArgs& a, uint32_t n_clusters, uint32_t n_clustered)
{
    ProfScope ps(pf, O3DR_K_CLUSTER_RECORDS, s);
    const int g = (int)cluster_blocks(a.n);
    k_cluster_points<<<g, kClusterThreads, 0, s>>>(a);
    if (a.rec && n_clusters > 0) {
        (void)hipMemsetAsync(a.box_lo, 0xff, (size_t)n_clusters * 3 * sizeof(uint32_t), s);
        (void)hipMemsetAsync(a.box_hi, 0, (size_t)n_clusters * 3 * sizeof(uint32_t), s);
        (void)hipMemsetAsync(a.sums, 0, (size_t)n_clusters * 3 * sizeof(unsigned long long), s);
        k_cluster_boxes<<<g, kClusterThreads, 0, s>>>(a);
        k_cluster_sums<<<g, kClusterThreads, 0, s>>>(a);
        k_cluster_records<<<(int)cluster_blocks(n_clusters), kClusterThreads, 0, s>>>(a, n_clusters);
    }
    if (a.indices && n_clustered > 0) {
        int nbits = 0;
        while (nbits < 32 && (n_clusters >> nbits) != 0) ++nbits;  // the keys are 0 .. n_clusters
        k_cluster_keys<<<g, kClusterThreads, 0, s>>>(a, n_clusters, ws.keys[0]);
        const int sorted = launch_sort_keys(ws, s, a.n, nbits);
        k_cluster_indices<<<(int)cluster_blocks(n_clustered), kClusterThreads, 0, s>>>(ws.vals[sorted], n_clustered, a.indices);
    }
}

}  // namespace o3dr
