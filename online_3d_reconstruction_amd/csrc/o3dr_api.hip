// o3dr_api.hip — the C ABI of include/o3dr.h on top of the kernels in o3dr_kernels.hip.
//
// Host-side responsibilities only: argument checking, HBM workspaces, staging of host buffers,
// batching of frames, the device-resident cloud_big, error codes.  There is no CPU compute path:
// without a GPU o3dr_ctx_create fails and nothing else can be called.
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <string>
#include <vector>

#include <rccl/rccl.h>  // types and enumerators only: the functions are resolved with dlsym (no link-time dependency on RCCL)

#include "../../include/o3dr_testing.h"
#include "o3dr_device.h"
#include "o3dr_image_stack.h"
#include "o3dr_profile.h"

using namespace o3dr;

// -------------------------------------------------------------------------------------------------
// errors
// -------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
static int fail(int code, const char* what)
{
    g_err = what;
    return code;
}
#define HIPCHK(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            char buf_[512];                                                                      \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            g_err = buf_;                                                                        \
            return O3DR_ERR_HIP;                                                                 \
        }                                                                                        \
    } while (0)
#define CHK(expr)                  \
    do {                           \
        int r_ = (expr);           \
        if (r_ != O3DR_OK) return r_; \
    } while (0)

// -------------------------------------------------------------------------------------------------
// context
// -------------------------------------------------------------------------------------------------
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct o3dr_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    o3dr_params params;
    double Q[16];
    bool has_Q = false;
    QLutEntry* q_lut = nullptr;  // device table for rectified-stereo Q (nullptr: general 4x4 product per pixel)
    bool q_lut_on = false;
    // cv::bilateralFilter tables (colour weights | space weights | tile offsets) for the last (d, sigmas) used
    DevBuf bil_tab, st_blur, st_blur_in, st_hist;
    int bil_d = 0, bil_radius = 0, bil_maxk = 0;
    double bil_sc = 0, bil_ss = 0;
    bool bil_valid = false;
    int max_batch = 256;  // frames per launch group (O3DR_BATCH_FRAMES); also bounded by a workspace budget
    int slab_shift_env = -2;  // O3DR_SLABS=0: plain pixel order in the fused batch path; O3DR_SLABS=sN: slabs of 2^N cells; else automatic
    int exact_box = 0;       // O3DR_EXACT_BOX=1: the batch path always takes the exact bounding box (k_reproject_bbox_count)
    int use_runs = 1;        // O3DR_RUNS=0: whole-cloud voxel grids sort points instead of runs; 2: always runs
    int small_path = 1;      // O3DR_SMALL=0: clouds of at most kSmallMax points take the general path too

    Workspace ws;
    size_t ws_elems = 0;   // frames*(cap+1) the per-point arrays were allocated for
    size_t ws_pts_elems = 0;
    int ws_frames = 0;
    size_t ws_emit_tiles = 0, ws_sort_tiles = 0, ws_seg_tiles = 0, ws_mm_floats = 0;
    DevBuf ws_block, ws_pts_block, ws_grid_block, ws_sor_block;
    int64_t ws_grid_cap = 0, ws_sor_cap = 0;  // points per cloud and clouds the search grids / SOR's arrays are carved for
    int ws_grid_frames = 0, ws_sor_frames = 0;

    // accumulating cloud (pose.cpp:434 cloud_big)
    o3dr_point* cloud_big = nullptr;
    int64_t cloud_cap = 0;
    o3dr_point* cloud_alt = nullptr;  // second buffer: partition target / receive buffer of the exchange
    int64_t cloud_alt_cap = 0;
    int64_t cloud_ub = 0;          // host-side upper bound of cc_big->count
    bool cloud_n_exact = true;     // cloud_ub IS the count (set by reads, resets and adopt; cleared by calls that append a bound)
    // running bounding box of cloud_big (min xyz, max xyz; device), kept by the frame calls so that the merge and
    // o3dr_cloud_big_bbox need no pass over the cloud; invalid after appends / transforms / exchanges
    float* cloud_box = nullptr;
    bool cloud_box_valid = false;
    // cloud_big's group-run heads for the merge's grid, recorded by the frame calls while it grows (4 points per byte);
    // valid under the same conditions as the running box, and for the leaf they were recorded with
    uint32_t* cloud_heads = nullptr;
    int64_t cloud_heads_cap = 0;  // points the flag buffer covers
    bool cloud_heads_valid = false;
    float cloud_heads_leaf[3] = {0.f, 0.f, 0.f};
    float cloud_heads_zo = 0.f;
    int cloud_box_enable = 1;  // O3DR_NO_CLOUD_BOX=1: always take the bounding box with a pass over the cloud
    CloudCounters* cc_big = nullptr;   // device
    CloudCounters* cc_tmp = nullptr;   // device, for single-shot calls
    CloudCounters* cc_host = nullptr;  // pinned
    CloudCounters* cc_host_dev = nullptr;  // ... as the device sees it: a one-workgroup call (kernels/small.inc) writes its result's
                                           // size straight into it, and the host reads it after the one synchronisation
    uint8_t* small_host = nullptr;     // pinned staging for the outputs of those calls (kSmallMax points)
    uint32_t* n_host = nullptr;        // pinned scratch (4 words)
    uint8_t* misc_dev = nullptr;       // 4 KiB device scratch: bbox (6 f32) | overflow (u32) | part counts (256 u64)
    uint8_t* misc_host = nullptr;      // pinned mirror
    uint8_t* misc_host_lut = nullptr;  // pinned staging of the Q table
    SortStats* stats_dev = nullptr;    // device statistics (bench.py byte accounting)
    SortStats* stats_host = nullptr;   // pinned

    DevBuf st_disp, st_bgr, st_in, st_out, st_kp, st_kpoff, st_poses;
    DevBuf st_xchg, st_merge, st_gather;  // o3dr_merge_partitioned: headers + count matrix, the merged slice, the gathered slices
    uint8_t* xchg_host = nullptr;         // pinned mirror of st_xchg
    size_t xchg_host_cap = 0;
    // host-input streaming of o3dr_accumulate_frames: two staging sets, uploads on their own stream
    DevBuf st2_disp[2], st2_bgr[2], st2_poses[2];
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_done[2] = {nullptr, nullptr};
    int test_corrupt = 0;  // o3dr_test_corrupt_next_gather: consumed by the next voxel grid
    int test_fail_at = 0;  // o3dr_test_fail_at: the numbered step of the next o3dr_merge_partitioned fails on this rank
    int64_t xchg_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // o3dr_merge_partitioned_stats
    // o3dr_nearest_neighbors / o3dr_icp_align: staged host clouds, the per-call source arrays (indices of this and the previous
    // pass, d2, the moment partials and their folded record).  nn_t also holds the staged cloud of MLS, clustering, plane
    // segmentation and meshing.  nn_cells: the part of a SearchGrid that is not in ws_grid_block, the cells' exact boxes and
    // the cloud's box (search_grid_build, for every operator that searches one cloud's grid).
    DevBuf nn_q, nn_t, nn_cells, nn_src;
    // Scratch of the operators after that (MLS, plane, mesh, match, keypoints, rigid fit, the image-stack operators), shared:
    // nothing in it outlives a call, and within one call every block is laid out by one carve().  OP_IN: staged host inputs
    // (descriptor pool; src / tgt / mask; image stacks).  OP_WORK: the arrays sized from the arguments (plane: points in tile
    // order + run heads; mesh: run heads + vertex tables; raster: the cells' words + column offsets; ground: those and
    // four fp32 rasters; clustering: the union-find, sizes, numbers, begins; match: pair table + chunk partials; rigid:
    // segment table + sums; ORB, stereo, the disparity and multi-view filters, segmentation: a group
    // of frames' arrays and the per-frame counters; rectification: the staged host map).  OP_LATE: the arrays sized from a
    // count read back mid-call (plane: tile tables; clustering: the clusters' boxes and sums).
    // OP_OUT: the staged outputs of a host call.  OP_FLAGS: the flags / ranges / counters of one operator (MlsFlags,
    // PlaneFlags, MeshFlags, RasterFlags, ClusterFlags, InterpFlags: 256 bytes; GroundFlags: 384; SampleFlags: 128).
    // Raster interpolation: OP_IN the staged raster, OP_WORK the partials and the pyramid's levels above 0.
    enum { OP_IN, OP_WORK, OP_LATE, OP_OUT, OP_FLAGS, OP_BUFS };
    DevBuf op[OP_BUFS];
    DevBuf orb_pat;  // o3dr_orb_detect: the steered table
    bool orb_pat_valid = false;
    std::vector<int8_t> orb_pat_h;  // (outlives the asynchronous upload)
    int64_t test_orb_scratch = 0;   // o3dr_test_orb_scratch_limit: stands in for kOrbScratchBytes when positive
    DevBuf pl_hyp;             // o3dr_segment_plane: hypotheses + scores (plane_hyp_layout), kept for the test hook
    uint64_t pl_last_hyp = 0;  // hypotheses of the last call in pl_hyp (o3dr_test_plane_hypotheses)
    std::vector<MatchPair> mt_tab_h;  // host copies of the match pair table, the rigid fit's segment table and transforms
    std::vector<int32_t> ch_pairs_h, ch_train_h, ch_status_h;  // ... and the pose chain's pair list, train frames, statuses, frames
    std::vector<ChainFrameIn> ch_frames_h;
    std::vector<RigidSeg> rg_seg_h;
    std::vector<RansacSeg> rs_seg_h;  // the RANSAC's segment table (o3dr_ransac_rigid; the chain's pairs)
    std::vector<double> rg_T_h;
    // o3dr_pose_graph_refine: pair keys (the duplicate check), accepted-pair bytes, per-pair counts, edges, frames, adjacency,
    // component ids and gauge bytes, the edges' energies
    std::vector<uint64_t> gr_keys_h;
    std::vector<uint8_t> gr_ok_h, gr_gauge_h;
    std::vector<uint32_t> gr_counts_h, gr_adj_h, gr_comp_h;
    std::vector<GraphEdgeIn> gr_edges_h;
    std::vector<GraphFrameIn> gr_frames_h;
    std::vector<double> gr_energy_h;
    int64_t place_ub = -1;   // o3dr_cloud_big_slice_counts_dev ran for a cloud of at most this many points and place_parts slices:
    int place_parts = 0;     // the (slice, tile) table in the workspace is what o3dr_cloud_big_place_slices moves by
    int test_hooks = 0;    // O3DR_TEST_HOOKS=1 at o3dr_ctx_create: the entry points of include/o3dr_testing.h act
    int host_batch = 32;  // frames per upload while the previous batch computes (O3DR_HOST_BATCH_FRAMES)
    // bumped by every call that rewrites points of cloud_big already in place (or shrinks it) and by a change of the merge's
    // leaf: the incremental merge's state then describes points that are gone
    uint64_t cloud_gen = 0;
    // o3dr_finalize_incremental: the occupied cells of the combined grid over cloud_big's first inc_folded points, with
    // their running sums (kernels/incremental.inc).  Two sets of (groups, cell offsets, cells) that swap; nothing exists
    // before the first call.
    struct {
        bool valid = false;
        int64_t folded = 0;
        uint64_t gen = 0;
        float leaf[3] = {0.f, 0.f, 0.f};
        float zo = 0.f;
        uint32_t n_groups = 0, n_cells = 0;
        int cur = 0;
        DevBuf grp[2], off[2], cells[2], box;                         // state
        DevBuf scratch, tg, tmatch, flag, src, keep, partial, words;  // per-call workspace
        DevBuf fb;                                                    // fallback: o3dr_finalize's result
        int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    } inc;
    Profiler prof;
};

static int dev_ensure(o3dr_ctx* c, DevBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return O3DR_OK;
    if (b.p) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;
    if (hipMalloc(&b.p, want) != hipSuccess) {
        (void)hipGetLastError();
        want = bytes;
        if (hipMalloc(&b.p, want) != hipSuccess) {
            b.p = nullptr;
            return fail(O3DR_ERR_ALLOC, "hipMalloc failed (workspace)");
        }
    }
    b.cap = want;
    return O3DR_OK;
}
static void dev_release(DevBuf& b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Walks a block of scratch: take() hands out the next array, each starting on a 256-byte boundary.  A layout is written
// once, as a function over the walker, and run twice: without a base for the block's size, with it for the pointers.
struct Carve {
    char* base = nullptr;
    size_t off = 0;
    template <class T>
    void take(T*& p, size_t count)
    {
        p = base ? (T*)(base + off) : nullptr;
        off += align256(count * sizeof(T));
    }
};
// grows block `b` to hold `layout` and points the layout's arrays into it
template <class Layout>
static int carve(o3dr_ctx* c, DevBuf& b, Layout&& layout)
{
    Carve size;
    layout(size);
    CHK(dev_ensure(c, b, size.off));
    Carve w{(char*)b.p, 0};
    layout(w);
    return O3DR_OK;
}

// (re)carve the per-batch workspace for `frames` clouds of at most `cap` points
// need_pts: ws.pts holds frames*cap points (A1 + A2 output); grp_tmp: ws.pts holds the result slots of the grouped
// whole-cloud voxel grid (one cloud, not in ws.pts itself)
static int ws_ensure(o3dr_ctx* c, int frames, int64_t cap, bool need_pts, bool grp_tmp = false)
{
    if (cap < 1) cap = 1;
    // whoever sizes the workspace is about to write it: a pending (slice, tile) table of o3dr_cloud_big_slice_counts_dev
    // is gone, and o3dr_cloud_big_place_slices must not move points by what the arrays hold afterwards
    c->place_ub = -1;
    const size_t elems = (size_t)frames * (size_t)(cap + 1);
    const size_t emit_tiles = (size_t)frames * (size_t)((cap + kEmitTile - 1) / kEmitTile);
    const size_t sort_tiles = (size_t)frames * (size_t)((cap + kSortTile - 1) / kSortTile);
    const size_t seg_tiles = (size_t)frames * (size_t)((cap + kSegTile - 1) / kSegTile);
    // bounding-box slots per frame: one per reprojection tile + the keypoint slot, or kMinmaxBlocks
    size_t mm_slots = (size_t)((cap + kEmitTile - 1) / kEmitTile) + 1;
    if (mm_slots < (size_t)kMinmaxBlocks) mm_slots = kMinmaxBlocks;
    const size_t mm_floats = (size_t)frames * mm_slots * 6;
    if (elems > c->ws_elems || frames > c->ws_frames || emit_tiles > c->ws_emit_tiles ||
        sort_tiles > c->ws_sort_tiles || seg_tiles > c->ws_seg_tiles || mm_floats > c->ws_mm_floats) {
        const size_t MM = mm_floats > c->ws_mm_floats ? mm_floats : c->ws_mm_floats;
        const size_t E = elems > c->ws_elems ? elems : c->ws_elems;
        const int F = frames > c->ws_frames ? frames : c->ws_frames;
        const size_t TE = emit_tiles > c->ws_emit_tiles ? emit_tiles : c->ws_emit_tiles;
        const size_t TS = sort_tiles > c->ws_sort_tiles ? sort_tiles : c->ws_sort_tiles;
        const size_t TG = seg_tiles > c->ws_seg_tiles ? seg_tiles : c->ws_seg_tiles;
        Workspace& w = c->ws;
        const size_t boxes = E / 64 + 8 * (size_t)F + 64;
        CHK(carve(c, c->ws_block, [&](Carve& k) {
            k.take(w.keys[0], E);
            k.take(w.keys[1], E);
            k.take(w.vals[0], E);
            k.take(w.vals[1], E);
            k.take(w.seg_start, E);
            k.take(w.keep_idx, E);
            k.take(w.run_start, E);
            k.take(w.grp_cnt, (E > (size_t)kGroupMinSlots ? E : (size_t)kGroupMinSlots) / kGroupCells + 2);
            k.take(w.tile_cnt, TE);
            k.take(w.hist, TS * kMaxRadix);
            k.take(w.hist_part, TS * kMaxRadix);
            k.take(w.seg_cnt, TG);
            k.take(w.head_bits, TG * 256);
            k.take(w.side, E + 16 * (size_t)F);  // (frames * side_frame_stride(cap) <= elems + 14 frames)
            k.take(w.scan_partial, (TS * kMaxRadix + TG + TE + E) / 4096 + 8 * (size_t)F + 16);
            k.take(w.mm, MM);
            k.take(w.n_valid, (size_t)F);
            k.take(w.n_kp, (size_t)F);
            k.take(w.n_vox, (size_t)F);
            k.take(w.n_out, (size_t)F);
            k.take(w.out_off, (size_t)F);
            k.take(w.geom, (size_t)F);
            k.take(w.geom_runs, (size_t)F);
            k.take(w.n_runs, (size_t)F);
            k.take(w.n_grp_out, (size_t)F);
            k.take(w.out_mm, boxes * 6);
            k.take(w.out_mm_partial, (size_t)kBoxFoldBlocks * 6);
            k.take(w.wave_gc, boxes * 6);
            w.bytes = k.off;
        }));
        c->ws_elems = E;
        c->ws_frames = F;
        c->ws_emit_tiles = TE;
        c->ws_sort_tiles = TS;
        c->ws_seg_tiles = TG;
        c->ws_mm_floats = MM;
    }
    c->ws.mm_stride = (int64_t)mm_slots;
    c->ws.grp_slots = 0;
    if (need_pts || grp_tmp) {
        size_t pe = (size_t)frames * (size_t)cap;
        if (grp_tmp && pe < (size_t)kGroupMinSlots) pe = (size_t)kGroupMinSlots;
        if (grp_tmp) c->ws.grp_slots = (int64_t)pe;
        if (pe > c->ws_pts_elems) {
            CHK(dev_ensure(c, c->ws_pts_block, pe * sizeof(o3dr_point)));
            c->ws_pts_elems = pe;
        }
        c->ws.pts = (o3dr_point*)c->ws_pts_block.p;
    }
    c->ws.frames = frames;
    c->ws.cap = cap;
    return O3DR_OK;
}

// the search grids of `frames` clouds of at most `cap` points (ws.grid_*), for SOR and for the operators that search one
// cloud's grid (search_grid_build).  sor_cell_z is SOR's but lives here: it is strided by grid_max_cells + 1 like
// grid_cell_first, and in SOR's block it would have to be carved again whenever the grid grows.
static int grid_ensure(o3dr_ctx* c, int frames, int64_t cap)
{
    if (cap < 1) cap = 1;
    if (frames < 1) frames = 1;
    if (cap > c->ws_grid_cap || frames > c->ws_grid_frames) {
        const int64_t C = cap > c->ws_grid_cap ? cap : c->ws_grid_cap;
        const size_t F = (size_t)(frames > c->ws_grid_frames ? frames : c->ws_grid_frames);
        const uint32_t max_cells = search_grid_max_cells(C);
        Workspace& w = c->ws;
        CHK(carve(c, c->ws_grid_block, [&](Carve& k) {
            k.take(w.grid_xyz, F * (size_t)C);
            k.take(w.grid_cell_first, F * ((size_t)max_cells + 1));
            k.take(w.sor_cell_z, F * ((size_t)max_cells + 1));
            k.take(w.grid_geom, F);
        }));
        w.grid_max_cells = max_cells;
        c->ws_grid_cap = C;
        c->ws_grid_frames = (int)F;
    }
    return O3DR_OK;
}
// ... and the arrays of the statistical outlier removal itself (allocated on first use: the measured configs run without
// it, and the map operators that only search a grid never pay for them)
static int sor_ensure(o3dr_ctx* c, int frames, int64_t cap)
{
    CHK(grid_ensure(c, frames, cap));
    if (cap < 1) cap = 1;
    if (frames < 1) frames = 1;
    if (cap > c->ws_sor_cap || frames > c->ws_sor_frames) {
        const int64_t C = cap > c->ws_sor_cap ? cap : c->ws_sor_cap;
        const size_t F = (size_t)(frames > c->ws_sor_frames ? frames : c->ws_sor_frames);
        Workspace& w = c->ws;
        CHK(carve(c, c->ws_sor_block, [&](Carve& k) {
            k.take(w.sor_pts, F * (size_t)C);
            k.take(w.sor_dist, F * (size_t)C);
            k.take(w.sor_partial, F * 256 * 2);
            k.take(w.sor_n, F);
            k.take(w.sor_left, F * (size_t)C);
            k.take(w.sor_left_cnt, F);
        }));
        c->ws_sor_cap = C;
        c->ws_sor_frames = (int)F;
    }
    return O3DR_OK;
}
static inline bool sor_on(const o3dr_ctx* c) { return c->params.sor_enable && c->params.jump_pixels > 0; }  // :1673

// The voxel grid job over `frames` clouds (cloud f = in + f*in_fstride, n_dev[f] of at most `cap` points) with this leaf,
// z offset and min_points.  Everything else is off; a caller states what is particular to it.
static VoxelArgs voxel_args(const o3dr_point* in, int64_t in_fstride, const uint32_t* n_dev, int frames, int64_t cap,
                            const float leaf[3], float z_offset = 0.f, uint32_t min_points = 0)
{
    VoxelArgs v;
    v.in = in;
    v.in_fstride = in_fstride;
    v.n_dev = n_dev;
    v.frames = frames;
    v.cap = cap;
    for (int a = 0; a < 3; ++a) v.leaf[a] = leaf[a];
    v.z_offset = z_offset;
    v.min_points = min_points;
    return v;
}
// Outlier removal in front of v's grid (pose_functions.cpp:1673-1686): the grid then reads the inliers and folds the
// bounding-box slots launch_sor left.  ensure: size the removal's buffers for this job first.
static int sor_in_front(o3dr_ctx* c, VoxelArgs& v, bool ensure = true)
{
    if (ensure) CHK(sor_ensure(c, v.frames, v.cap));
    v.mm_used = launch_sor(&c->prof, c->stream, c->ws, v.in, v.in_fstride, v.n_dev, v.frames, v.cap, v.mm_used, 1.0, c->ws.sor_pts,
                           v.in_fstride, c->ws.sor_n);
    v.in = c->ws.sor_pts;
    v.n_dev = c->ws.sor_n;
    return O3DR_OK;
}

extern "C" int o3dr_version(void) { return O3DR_VERSION; }
extern "C" const char* o3dr_last_error(void) { return g_err.c_str(); }

extern "C" void o3dr_default_params(o3dr_params* p)
{
    if (!p) return;
    p->min_disparity = 64;          // pose.h:93
    p->voxel_size = 0.1;            // pose.h:118
    p->bounding_box = 20;           // pose.h:94
    p->cutout_ratio = 8;            // pose.h:126
    p->jump_pixels = 10;            // pose.h:96
    p->min_points_per_voxel = 1;    // pose.h:108
    p->dont_downsample = 0;
    p->sor_enable = 1;              // pose_functions.cpp:1673-1686: always on in the reference's per-frame path
    p->blur_kernel = 1;             // pose.h:98
    p->disparity_f64 = 0;           // use_segment_labels off
}

static int cloud_box_clear(o3dr_ctx* c);

extern "C" int o3dr_ctx_create(int device_id, o3dr_ctx** out_ctx)
{
    if (!out_ctx) return fail(O3DR_ERR_INVALID_ARG, "out_ctx is NULL");
    *out_ctx = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(O3DR_ERR_NO_DEVICE, "no HIP device: libo3dr has no CPU path");
    }
    if (device_id < 0 || device_id >= n) return fail(O3DR_ERR_INVALID_ARG, "device_id out of range");
    if (hipSetDevice(device_id) != hipSuccess) return fail(O3DR_ERR_NO_DEVICE, "hipSetDevice failed");
    o3dr_ctx* c = new o3dr_ctx();
    c->device = device_id;
    o3dr_default_params(&c->params);
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(O3DR_ERR_NO_DEVICE, "hipStreamCreate failed");
    }
    c->stream = c->own_stream;
    if (hipMalloc((void**)&c->cloud_box, 6 * sizeof(float)) != hipSuccess ||
        hipMalloc((void**)&c->cc_big, sizeof(CloudCounters)) != hipSuccess ||
        hipMalloc((void**)&c->cc_tmp, sizeof(CloudCounters)) != hipSuccess ||
        hipHostMalloc((void**)&c->cc_host, 2 * sizeof(CloudCounters), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&c->n_host, 4 * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&c->small_host, (size_t)kSmallMax * sizeof(o3dr_point), hipHostMallocDefault) != hipSuccess ||
        hipHostGetDevicePointer((void**)&c->cc_host_dev, c->cc_host, 0) != hipSuccess ||
        hipMalloc((void**)&c->stats_dev, sizeof(SortStats)) != hipSuccess ||
        hipMalloc((void**)&c->misc_dev, 4096) != hipSuccess ||
        hipHostMalloc((void**)&c->misc_host, 4096, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&c->misc_host_lut, 256 * sizeof(QLutEntry), hipHostMallocDefault) != hipSuccess ||
        hipMalloc((void**)&c->q_lut, 256 * sizeof(QLutEntry)) != hipSuccess ||
        hipHostMalloc((void**)&c->stats_host, sizeof(SortStats), hipHostMallocDefault) != hipSuccess) {
        delete c;
        return fail(O3DR_ERR_ALLOC, "counter allocation failed");
    }
    (void)hipMemsetAsync(c->cc_big, 0, sizeof(CloudCounters), c->stream);
    (void)hipMemsetAsync(c->cc_tmp, 0, sizeof(CloudCounters), c->stream);
    (void)hipMemsetAsync(c->stats_dev, 0, sizeof(SortStats), c->stream);
    (void)hipMemsetAsync(c->misc_dev, 0, 4096, c->stream);
    // the only environment switches, all read here, once per context (tests drive them)
    const char* hb_env = getenv("O3DR_HOST_BATCH_FRAMES");
    if (hb_env && atoi(hb_env) > 0) c->host_batch = atoi(hb_env);
    const char* ru_env = getenv("O3DR_RUNS");
    if (ru_env && atoi(ru_env) == 0) c->use_runs = 0;       // whole-cloud grids always sort points
    else if (ru_env && atoi(ru_env) == 2) c->use_runs = 2;  // ... always sort runs (default: decided per cloud on the device)
    if (getenv("O3DR_NO_CLOUD_BOX")) c->cloud_box_enable = 0;
    const char* eb_env = getenv("O3DR_EXACT_BOX");
    c->exact_box = eb_env && atoi(eb_env) == 1;
    const char* sm_env = getenv("O3DR_SMALL");
    if (sm_env) c->small_path = atoi(sm_env) != 0;
    const char* th_env = getenv("O3DR_TEST_HOOKS");
    c->test_hooks = th_env && atoi(th_env) == 1;
    const char* sl_env = getenv("O3DR_SLABS");
    if (sl_env && sl_env[0] == '0') c->slab_shift_env = -1;
    else if (sl_env && sl_env[0] == 's' && atoi(sl_env + 1) >= 0 && atoi(sl_env + 1) <= 20) c->slab_shift_env = atoi(sl_env + 1);
    const char* env = getenv("O3DR_BATCH_FRAMES");
    if (env && atoi(env) > 0) c->max_batch = atoi(env) > 512 ? 512 : atoi(env);
    (void)cloud_box_clear(c);
    *out_ctx = c;
    return O3DR_OK;
}

extern "C" int o3dr_ctx_destroy(o3dr_ctx* c)
{
    if (!c) return O3DR_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (DevBuf* b : {&c->ws_block, &c->ws_pts_block, &c->ws_grid_block, &c->ws_sor_block, &c->st_disp, &c->st_bgr, &c->st_in, &c->st_out,
                      &c->st_kp, &c->st_kpoff, &c->st_poses, &c->st_xchg, &c->st_merge, &c->st_gather, &c->bil_tab, &c->st_blur,
                      &c->st_blur_in, &c->st_hist})
        dev_release(*b);
    if (c->xchg_host) (void)hipHostFree(c->xchg_host);
    if (c->cloud_big) (void)hipFree(c->cloud_big);
    if (c->cloud_alt) (void)hipFree(c->cloud_alt);
    if (c->cloud_box) (void)hipFree(c->cloud_box);
    if (c->cloud_heads) (void)hipFree(c->cloud_heads);
    if (c->cc_big) (void)hipFree(c->cc_big);
    if (c->cc_tmp) (void)hipFree(c->cc_tmp);
    if (c->cc_host) (void)hipHostFree(c->cc_host);
    if (c->n_host) (void)hipHostFree(c->n_host);
    if (c->small_host) (void)hipHostFree(c->small_host);
    if (c->stats_dev) (void)hipFree(c->stats_dev);
    if (c->misc_dev) (void)hipFree(c->misc_dev);
    if (c->misc_host) (void)hipHostFree(c->misc_host);
    if (c->misc_host_lut) (void)hipHostFree(c->misc_host_lut);
    if (c->q_lut) (void)hipFree(c->q_lut);
    if (c->stats_host) (void)hipHostFree(c->stats_host);
    for (int i = 0; i < 2; ++i) {
        dev_release(c->st2_disp[i]);
        dev_release(c->st2_bgr[i]);
        dev_release(c->st2_poses[i]);
        dev_release(c->inc.grp[i]);
        dev_release(c->inc.off[i]);
        dev_release(c->inc.cells[i]);
        if (c->ev_copied[i]) (void)hipEventDestroy(c->ev_copied[i]);
        if (c->ev_done[i]) (void)hipEventDestroy(c->ev_done[i]);
    }
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    for (DevBuf* b : {&c->inc.box, &c->inc.scratch, &c->inc.tg, &c->inc.tmatch, &c->inc.flag, &c->inc.src, &c->inc.keep,
                      &c->inc.partial, &c->inc.words, &c->inc.fb, &c->nn_q, &c->nn_t, &c->nn_cells, &c->nn_src, &c->pl_hyp, &c->orb_pat})
        dev_release(*b);
    for (DevBuf& b : c->op) dev_release(b);
    delete c;
    return O3DR_OK;
}

#define CTX_ENTER(c)                                                        \
    do {                                                                    \
        if (!(c)) return fail(O3DR_ERR_INVALID_ARG, "ctx is NULL");         \
        HIPCHK(hipSetDevice((c)->device));                                  \
    } while (0)

// CTX_ENTER, then the implementation: for the entry points that clean their outputs up after a failure of either
template <class Impl>
static int entered(o3dr_ctx* c, Impl&& impl)
{
    CTX_ENTER(c);
    return impl();
}

extern "C" int o3dr_ctx_set_stream(o3dr_ctx* c, void* hip_stream)
{
    CTX_ENTER(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return O3DR_OK;
}
extern "C" int o3dr_ctx_synchronize(o3dr_ctx* c)
{
    CTX_ENTER(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}
extern "C" int o3dr_set_camera(o3dr_ctx* c, const double Q[16])
{
    CTX_ENTER(c);
    if (!Q) return fail(O3DR_ERR_INVALID_ARG, "Q is NULL");
    memcpy(c->Q, Q, sizeof c->Q);
    c->has_Q = true;
    // Rectified stereo Q (cv::stereoRectify): X and Y rows use one pixel coordinate each, Z and W only the
    // disparity.  Then 1./W and Z are functions of the 8-bit disparity alone: tabulate them with the very
    // operations the per-pixel path would execute (IEEE fp64 on both sides), drop the exact-zero terms.
    static const int zeros[] = {1, 2, 4, 6, 8, 9, 12, 13};
    bool sparse = true;
    for (int z : zeros) sparse = sparse && (Q[z] == 0.0);
    c->q_lut_on = false;
    if (sparse) {
        QLutEntry* h = (QLutEntry*)c->misc_host_lut;
        for (int d = 0; d < 256; ++d) {
            const double dd = (double)d;
            const double t2 = ((Q[8] * 0.0 + Q[9] * 0.0) + Q[10] * dd) + Q[11];
            const double t3 = ((Q[12] * 0.0 + Q[13] * 0.0) + Q[14] * dd) + Q[15];
            const double alpha = 1. / t3;
            h[d].alpha = alpha;
            h[d].z = (float)(t2 * alpha + 0.0);
            h[d].pad = 0.f;
        }
        HIPCHK(hipMemcpyAsync(c->q_lut, h, 256 * sizeof(QLutEntry), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->q_lut_on = true;
    }
    return O3DR_OK;
}
extern "C" int o3dr_set_params(o3dr_ctx* c, const o3dr_params* p)
{
    CTX_ENTER(c);
    if (!p) return fail(O3DR_ERR_INVALID_ARG, "params is NULL");
    if (p->bounding_box < 0 || p->cutout_ratio <= 0 || p->jump_pixels < 0 || !(p->voxel_size > 0))
        return fail(O3DR_ERR_INVALID_ARG, "params out of range");
    if (p->voxel_size != c->params.voxel_size) ++c->cloud_gen;  // the merge's leaf (an incremental merge refolds)
    c->params = *p;
    return O3DR_OK;
}
extern "C" int o3dr_get_params(o3dr_ctx* c, o3dr_params* p)
{
    CTX_ENTER(c);
    if (!p) return fail(O3DR_ERR_INVALID_ARG, "params is NULL");
    *p = c->params;
    return O3DR_OK;
}

// -------------------------------------------------------------------------------------------------
// helpers
// -------------------------------------------------------------------------------------------------
struct GridShape {
    int cs, Ny, Nx;
    int64_t n;
};
// pose_functions.cpp:638 and the loop bounds of :1094-1096
static GridShape grid_shape(const o3dr_params& p, int rows, int cols)
{
    GridShape g;
    g.cs = (int)(cols / p.cutout_ratio);
    g.Ny = g.Nx = 0;
    if (p.jump_pixels > 0) {
        const int h = rows - 2 * p.bounding_box, w = cols - p.bounding_box - g.cs;
        g.Ny = h > 0 ? (h + p.jump_pixels - 1) / p.jump_pixels : 0;
        g.Nx = w > 0 ? (w + p.jump_pixels - 1) / p.jump_pixels : 0;
    }
    g.n = (int64_t)g.Ny * g.Nx;
    return g;
}

extern "C" int64_t o3dr_max_points(o3dr_ctx* c, int32_t rows, int32_t cols)
{
    if (!c) return 0;
    return grid_shape(c->params, rows, cols).n;
}

static int check_images(const o3dr_ctx* c, const uint8_t* disp, int64_t disp_pitch, const uint8_t* bgr, int64_t bgr_pitch,
                        int rows, int cols, int64_t disp_frame_stride = 0)
{
    if (!disp || !bgr) return fail(O3DR_ERR_INVALID_ARG, "image pointer is NULL");
    if (rows <= 0 || cols <= 0) return fail(O3DR_ERR_INVALID_ARG, "rows/cols must be positive");
    const int64_t esz = c->params.disparity_f64 ? 8 : 1;
    if (disp_pitch < esz * cols || bgr_pitch < 3 * (int64_t)cols) return fail(O3DR_ERR_INVALID_ARG, "pitch smaller than a row");
    if (esz == 8 && (((uintptr_t)disp | (uintptr_t)disp_pitch | (uintptr_t)disp_frame_stride) & 7))
        return fail(O3DR_ERR_INVALID_ARG, "CV_64F disparities must be 8-byte aligned (pointer, pitch, frame stride)");
    return O3DR_OK;
}

static void fill_args(o3dr_ctx* c, ReprojectArgs& a, const uint8_t* disp, int64_t disp_pitch, int64_t disp_fstride,
                      const uint8_t* bgr, int64_t bgr_pitch, int64_t bgr_fstride, int rows, int cols,
                      const GridShape& g, int64_t out_fstride)
{
    memset(&a, 0, sizeof a);
    a.disp = disp;
    a.bgr = bgr;
    a.disp_pitch = disp_pitch;
    a.bgr_pitch = bgr_pitch;
    a.disp_fstride = disp_fstride;
    a.bgr_fstride = bgr_fstride;
    a.rows = rows;
    a.cols = cols;
    a.bb = c->params.bounding_box;
    a.cs = g.cs;
    a.jump = c->params.jump_pixels;
    a.Ny = g.Ny;
    a.Nx = g.Nx;
    a.n_tiles = (int)((g.n + kEmitTile - 1) / kEmitTile);
    a.disp_f64 = c->params.disparity_f64 ? 1 : 0;
    a.vec4 = (!a.disp_f64 && a.jump == 1 && (g.Nx % 4) == 0 && (g.cs % 4) == 0 && (disp_pitch % 4) == 0 && (bgr_pitch % 4) == 0 &&
              (disp_fstride % 4) == 0 && (bgr_fstride % 4) == 0 && ((uintptr_t)disp % 4) == 0 &&
              ((uintptr_t)bgr % 4) == 0)
                 ? 1
                 : 0;
    memcpy(a.Q, c->Q, sizeof a.Q);
    a.min_disp = c->params.min_disparity;
    {   // the same comparison on integers (no fp64 convert + compare per pixel): d > m <=> d > floor(m) for integer d
        const double m = a.min_disp;
        a.min_disp_u8 = !(m == m) || m >= 255.0 ? 255 : (m < 0.0 ? -1 : (int32_t)floor(m));
    }
    a.out_fstride = out_fstride;
    a.mm_stride = c->ws.mm_stride;
    a.lut = (c->q_lut_on && !a.disp_f64) ? c->q_lut : nullptr;
}

// Thickness (log2, in cells) of the grid slabs the fused batch path sorts a frame's points into (slab_class in
// kernels/reproject.inc): about two thirds of the distance between the depth sheets of two neighbouring disparity levels
// at a nominal disparity, so that the sheets one line of pixels lands on fall into different classes.  A layout choice
// only: results do not depend on it.  -1: plain pixel order (O3DR_SLABS=0).
static int slab_shift_for(const o3dr_ctx* c, int rows, int cols, const float leaf[3])
{
    if (c->slab_shift_env >= -1) return c->slab_shift_env;
    const double* Q = c->Q;
    auto point = [&](double d, double out[3]) {
        const double v[4] = {0.5 * cols, 0.5 * rows, d, 1.0};
        double t[4];
        for (int r = 0; r < 4; ++r) t[r] = ((Q[4 * r] * v[0] + Q[4 * r + 1] * v[1]) + Q[4 * r + 2] * v[2]) + Q[4 * r + 3];
        for (int r = 0; r < 3; ++r) out[r] = t[r] / t[3];
    };
    double p0[3], p1[3];
    point(128.0, p0);
    point(129.0, p1);
    const double dist = sqrt((p1[0] - p0[0]) * (p1[0] - p0[0]) + (p1[1] - p0[1]) * (p1[1] - p0[1]) + (p1[2] - p0[2]) * (p1[2] - p0[2]));
    const double lf = leaf[0] > leaf[1] ? (leaf[0] > leaf[2] ? leaf[0] : leaf[2]) : (leaf[1] > leaf[2] ? leaf[1] : leaf[2]);
    const double cells = dist / lf / 1.5;
    if (!(cells >= 2.0)) return 0;  // (also NaN / inf from a degenerate Q)
    int sh = 0;
    while (sh < 16 && (double)(2 << sh) <= cells) ++sh;
    return sh;
}

// stage a host buffer into HBM (or pass a device pointer through)
static int stage_in(o3dr_ctx* c, DevBuf& b, const void* src, size_t bytes, int mem, const void** dev)
{
    if (mem == O3DR_MEM_DEVICE) {
        *dev = src;
        return O3DR_OK;
    }
    CHK(dev_ensure(c, b, bytes ? bytes : 1));
    if (bytes) HIPCHK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    *dev = b.p;
    return O3DR_OK;
}

// read a CloudCounters back (synchronises)
// The outputs of one call, named once: add() for each (the caller's pointer, nullptr if not asked for, and the elements
// it holds).  stage() then gives each its device pointer - the caller's own for O3DR_MEM_DEVICE, a slice of the one
// staging block for O3DR_MEM_HOST -, copy_back() enqueues the device-to-host copies behind the launches, and zero() clears
// the host outputs where the operator's contract says so.
struct Outputs {
    struct Item {
        void* user;
        size_t elem, cap, count;  // bytes per element, elements the caller's array holds, elements this call writes
        void* dev;
    };
    int mem, n = 0;
    Item item[5];
    template <class T>
    void add(T* user, int64_t capacity)
    {
        const size_t cap = user && capacity > 0 ? (size_t)capacity : 0;
        item[n++] = Item{(void*)user, sizeof(T), cap, cap, (void*)user};
    }
    Item* find(const void* user)
    {
        for (int i = 0; i < n; ++i)
            if (user && item[i].user == user) return &item[i];
        return nullptr;
    }
    // the call writes only the first `count` elements of this output
    void set_count(const void* user, int64_t count)
    {
        if (Item* it = find(user)) it->count = (size_t)count;
    }
    int stage(o3dr_ctx* c)
    {
        if (mem != O3DR_MEM_HOST) return O3DR_OK;
        return carve(c, c->op[o3dr_ctx::OP_OUT], [&](Carve& w) {
            for (Item* it = item; it < item + n; ++it) {
                char* d;
                w.take(d, it->count * it->elem);
                it->dev = it->count ? d : nullptr;
            }
        });
    }
    // where the kernels write this output (nullptr: not asked for)
    template <class T>
    T* dev(T* user)
    {
        Item* it = find(user);
        return it ? (T*)it->dev : nullptr;
    }
    int copy_back(o3dr_ctx* c) const
    {
        for (const Item* it = item; mem == O3DR_MEM_HOST && it < item + n; ++it)
            if (it->count) HIPCHK(hipMemcpyAsync(it->user, it->dev, it->count * it->elem, hipMemcpyDeviceToHost, c->stream));
        return O3DR_OK;
    }
    // all of every host output, but for `keep` (an output that is also the call's input)
    void zero(const void* keep = nullptr) const
    {
        for (const Item* it = item; mem == O3DR_MEM_HOST && it < item + n; ++it)
            if (it->cap && it->user != keep) memset(it->user, 0, it->cap * it->elem);
    }
};

// What the front ends of the image-stack operators share (o3dr_image_stack.h holds the layout contract itself).
// a check of that header: its text, if any, is the call's error
#define STACKCHK(expr)                                                 \
    do {                                                               \
        if (const char* m_ = (expr)) return fail(O3DR_ERR_INVALID_ARG, m_); \
    } while (0)
// the two checks every one of them opens with
static const char* stack_call_error(int32_t mem, int32_t n_frames)
{
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return "bad mem kind";
    return n_frames < 0 ? "bad frame count" : nullptr;
}
// stages one stack, or two of one layout, of `bytes` each into op[OP_IN] (device pointers pass through): the first at
// offset 0, the second at align256(bytes)
static int stage_stacks(o3dr_ctx* c, size_t bytes, int mem, const void* a, const void** a_d, const void* b = nullptr,
                        const void** b_d = nullptr)
{
    DevBuf& in = c->op[o3dr_ctx::OP_IN];
    if (!b) return stage_in(c, in, a, bytes, mem, a_d);
    if (mem == O3DR_MEM_DEVICE) {
        *a_d = a, *b_d = b;
        return O3DR_OK;
    }
    CHK(dev_ensure(c, in, 2 * align256(bytes)));
    char* base = (char*)in.p;
    HIPCHK(hipMemcpyAsync(base, a, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(base + align256(bytes), b, bytes, hipMemcpyHostToDevice, c->stream));
    *a_d = base, *b_d = base + align256(bytes);
    return O3DR_OK;
}
// The per-frame counters behind an operator's *_info: `words` per frame (none where the caller asks for no info), carved
// with the call's other arrays, zeroed on the stream, copied back behind the launches and valid after the call's one
// synchronise.
struct FrameCounters {
    size_t frames, words;  // frames = 0: not asked for
    unsigned long long* dev = nullptr;
    std::vector<unsigned long long> host;
    FrameCounters(const void* info, int32_t n_frames, size_t words_) : frames(info ? (size_t)n_frames : 0), words(words_) {}
    void take(Carve& w)
    {
        if (frames) w.take(dev, frames * words);
    }
    int zero(o3dr_ctx* c)
    {
        if (frames) HIPCHK(hipMemsetAsync(dev, 0, frames * words * sizeof(unsigned long long), c->stream));
        return O3DR_OK;
    }
    unsigned long long* of_frame(size_t f) const { return dev ? dev + f * words : nullptr; }
    int copy_back(o3dr_ctx* c)
    {
        host.resize(frames * words);
        if (frames) HIPCHK(hipMemcpyAsync(host.data(), dev, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        return O3DR_OK;
    }
};

static int read_counters(o3dr_ctx* c, const CloudCounters* dev, CloudCounters* host, const CloudCounters* dev2 = nullptr,
                         CloudCounters* host2 = nullptr)
{
    HIPCHK(hipMemcpyAsync(c->cc_host, dev, sizeof(CloudCounters), hipMemcpyDeviceToHost, c->stream));
    if (dev2) HIPCHK(hipMemcpyAsync(c->cc_host + 1, dev2, sizeof(CloudCounters), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *host = *c->cc_host;
    if (dev2) {
        *host2 = c->cc_host[1];
        if (dev2 == c->cc_big) {
            c->cloud_ub = (int64_t)host2->count;
            c->cloud_n_exact = true;
        }
    }
    if (dev == c->cc_big) {  // every read of the cloud's counters makes the host-side bound exact
        c->cloud_ub = (int64_t)host->count;
        c->cloud_n_exact = true;
    }
    if ((host->status | (dev2 ? host2->status : 0u)) & O3DR_STATUS_INTERNAL)
        return fail(O3DR_ERR_INTERNAL, "a device-side gather guard tripped (record or point id outside its cloud); results are invalid");
    return O3DR_OK;
}

static int zero_counters(o3dr_ctx* c, CloudCounters* dev)
{
    HIPCHK(hipMemsetAsync(dev, 0, sizeof(CloudCounters), c->stream));
    return O3DR_OK;
}

// weight tables of cv::bilateralFilter (OpenCV 3.1 smooth.cpp bilateralFilter_8u), built with the host's exp()
static int bilateral_prepare(o3dr_ctx* c, int d, double sigma_color, double sigma_space)
{
    if (sigma_color <= 0) sigma_color = 1;
    if (sigma_space <= 0) sigma_space = 1;
    if (c->bil_valid && c->bil_d == d && c->bil_sc == sigma_color && c->bil_ss == sigma_space) return O3DR_OK;
    const double gauss_color_coeff = -0.5 / (sigma_color * sigma_color);
    const double gauss_space_coeff = -0.5 / (sigma_space * sigma_space);
    int radius = d <= 0 ? (int)lrint(sigma_space * 1.5) : d / 2;  // cvRound
    if (radius < 1) radius = 1;
    if (radius > kBilMaxRadius) return fail(O3DR_ERR_INVALID_ARG, "bilateral filter radius above 64 is not supported");
    const int dd = 2 * radius + 1, tw = bilateral_tile_width(radius);
    std::vector<float> tab(256 + 2 * (size_t)dd * dd);
    for (int i = 0; i < 256; ++i) tab[i] = (float)std::exp(i * i * gauss_color_coeff);
    int maxk = 0;
    for (int i = -radius; i <= radius; ++i)
        for (int j = -radius; j <= radius; ++j) {
            const double r = std::sqrt((double)i * i + (double)j * j);
            if (r > radius) continue;
            ++maxk;
        }
    int k = 0;
    for (int i = -radius; i <= radius; ++i)
        for (int j = -radius; j <= radius; ++j) {
            const double r = std::sqrt((double)i * i + (double)j * j);
            if (r > radius) continue;
            tab[256 + k] = (float)std::exp(r * r * gauss_space_coeff);
            const int32_t ofs = i * tw + j;
            memcpy(&tab[256 + maxk + k], &ofs, sizeof ofs);
            ++k;
        }
    HIPCHK(hipStreamSynchronize(c->stream));  // earlier launches may still read the old table
    c->bil_valid = false;
    CHK(dev_ensure(c, c->bil_tab, (256 + 2 * (size_t)maxk) * sizeof(float)));
    HIPCHK(hipMemcpy(c->bil_tab.p, tab.data(), (256 + 2 * (size_t)maxk) * sizeof(float), hipMemcpyHostToDevice));
    c->bil_d = d;
    c->bil_sc = sigma_color;
    c->bil_ss = sigma_space;
    c->bil_radius = radius;
    c->bil_maxk = maxk;
    c->bil_valid = true;
    return O3DR_OK;
}

// blur_kernel > 1 (pose_functions.cpp:1040-1047): the frames' disparity images are filtered into a scratch
// buffer the reprojection then reads.  Rewrites (disp, pitch, frame stride) in place.
static int maybe_blur(o3dr_ctx* c, const uint8_t** disp_d, int64_t* pitch, int64_t* fstride, int rows, int cols, int frames)
{
    const int bk = c->params.blur_kernel;
    if (bk <= 1) return O3DR_OK;
    if (c->params.disparity_f64)
        return fail(O3DR_ERR_INVALID_ARG, "blur_kernel > 1 needs CV_8UC1 disparities (cv::bilateralFilter rejects CV_64F)");
    CHK(bilateral_prepare(c, bk, (double)(bk * 2), (double)(bk / 2)));
    const int64_t out_pitch = cols, out_fstride = (int64_t)rows * cols;
    CHK(dev_ensure(c, c->st_blur, (size_t)out_fstride * (size_t)frames + 16));
    launch_bilateral(&c->prof, c->stream, *disp_d, *pitch, *fstride, rows, cols, frames, c->bil_radius, c->bil_maxk,
                     (const float*)c->bil_tab.p, (uint8_t*)c->st_blur.p, out_pitch, out_fstride);
    HIPCHK(hipGetLastError());
    *disp_d = (const uint8_t*)c->st_blur.p;
    *pitch = out_pitch;
    *fstride = out_fstride;
    return O3DR_OK;
}

// A1 (+A2) of one frame into `dst` (device).  n_valid ends up in ws.n_valid[0].
static int run_reproject_single(o3dr_ctx* c, const uint8_t* disp_d, int64_t disp_pitch, const uint8_t* bgr_d,
                                int64_t bgr_pitch, int rows, int cols, const GridShape& g, const float* T,
                                const float* kp_d, int n_kp, o3dr_point* dst, const float* T_dev = nullptr)
{
    int64_t disp_fstride = 0;
    CHK(maybe_blur(c, &disp_d, &disp_pitch, &disp_fstride, rows, cols, 1));
    ReprojectArgs a;
    fill_args(c, a, disp_d, disp_pitch, 0, bgr_d, bgr_pitch, 0, rows, cols, g, 0);
    if (T_dev) {  // pose already in HBM (one frame of a batched call)
        a.xf_mode = 2;
        a.poses = T_dev;
    } else if (T) {
        a.xf_mode = 1;
        for (int i = 0; i < 12; ++i) a.T[i] = T[i];
    }
    launch_minmax_init(&c->prof, c->stream, c->ws.mm, c->ws.mm_stride, a.n_tiles, c->ws.n_kp, 1);
    if (c->params.jump_pixels != 1 && n_kp > 0)
        launch_keypoint_pass(&c->prof, c->stream, a, kp_d, n_kp, dst, c->ws.n_kp, c->ws.mm);
    launch_reproject(&c->prof, c->stream, a, 1, dst, c->ws.tile_cnt, c->ws.n_kp, c->ws.n_valid, c->ws.mm,
                     c->ws.scan_partial);
    HIPCHK(hipGetLastError());
    return O3DR_OK;
}

static int read_u32(o3dr_ctx* c, const uint32_t* dev, uint32_t* host)
{
    HIPCHK(hipMemcpyAsync(c->n_host, dev, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *host = c->n_host[0];
    return O3DR_OK;
}

// common body of A1, A1+A2 and A6
static int frame_call(o3dr_ctx* c, const uint8_t* disp, int64_t disp_pitch, const uint8_t* bgr, int64_t bgr_pitch,
                      int rows, int cols, const float* T, const float* kp_xy, int n_kp, bool downsample,
                      o3dr_point* out, int64_t out_capacity, int64_t* n_out, uint32_t* status, int mem)
{
    if (n_out) *n_out = 0;
    if (status) *status = 0;
    CTX_ENTER(c);
    if (!c->has_Q) return fail(O3DR_ERR_NOT_CONFIGURED, "o3dr_set_camera has not been called");
    if (!n_out || !out) return fail(O3DR_ERR_INVALID_ARG, "out / n_out is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    CHK(check_images(c, disp, disp_pitch, bgr, bgr_pitch, rows, cols));
    if (n_kp < 0 || (n_kp > 0 && !kp_xy)) return fail(O3DR_ERR_INVALID_ARG, "bad keypoint list");
    if (c->params.jump_pixels == 1) n_kp = 0;  // :1057 keypoints are skipped when every pixel is taken
    const GridShape g = grid_shape(c->params, rows, cols);
    const int64_t cap = g.n + n_kp;
    if (mem == O3DR_MEM_DEVICE && out_capacity < cap)
        return fail(O3DR_ERR_CAPACITY, "device output must hold o3dr_max_points()+n_kp points");
    if (cap == 0) return O3DR_OK;

    const void *disp_d, *bgr_d, *kp_d = nullptr;
    CHK(stage_in(c, c->st_disp, disp, (size_t)rows * disp_pitch, mem, &disp_d));
    CHK(stage_in(c, c->st_bgr, bgr, (size_t)rows * bgr_pitch, mem, &bgr_d));
    if (n_kp > 0) CHK(stage_in(c, c->st_kp, kp_xy, (size_t)n_kp * 2 * sizeof(float), mem, &kp_d));
    CHK(ws_ensure(c, 1, cap, downsample));

    o3dr_point* final_dst = out;
    if (mem == O3DR_MEM_HOST) {
        CHK(dev_ensure(c, c->st_out, (size_t)cap * sizeof(o3dr_point)));
        final_dst = (o3dr_point*)c->st_out.p;
    }
    int64_t n_final = 0;
    uint32_t st = 0;
    // Frames of at most kSmallMax candidates - the reference's own configuration, --jump_pixels 10 .. 15 - take the whole
    // path in ONE launch of one workgroup (kernels/small.inc) instead of ~45 launches that cost their latency and nothing
    // else; with the outlier removal on, its kernels run between the two halves.  O3DR_SMALL=0 switches it off.
    const bool small = c->small_path && cap <= kSmallMax && !c->params.disparity_f64 && !c->test_corrupt;
    if (small) {
        const uint8_t* dsp = (const uint8_t*)disp_d;
        int64_t dsp_pitch = disp_pitch, dsp_fstride = 0;
        CHK(maybe_blur(c, &dsp, &dsp_pitch, &dsp_fstride, rows, cols, 1));
        ReprojectArgs a;
        fill_args(c, a, dsp, dsp_pitch, 0, (const uint8_t*)bgr_d, bgr_pitch, 0, rows, cols, g, 0);
        if (T) {
            a.xf_mode = 1;
            for (int i = 0; i < 12; ++i) a.T[i] = T[i];
        }
        float leaf[3];
        leaf[0] = leaf[1] = leaf[2] = (float)(c->params.voxel_size / 5);  // pose_functions.cpp:1698
        const bool with_sor = downsample && sor_on(c);
        // the result's size lands in pinned host memory, written by the kernel itself; host outputs come back in the same
        // wait (all `cap` slots, at most 128 KiB, through a pinned staging buffer): ONE synchronisation per call
        if (with_sor) {
            CHK(sor_ensure(c, 1, cap));
            launch_small_frame(&c->prof, c->stream, a, (const float*)kp_d, n_kp, 0, leaf, nullptr, c->ws.pts, c->cc_tmp, c->ws.n_valid, c->ws.mm);
            launch_sor_small(&c->prof, c->stream, c->ws, c->ws.pts, c->ws.n_valid, cap, 1.0, c->ws.sor_pts, c->ws.sor_n);
            launch_small_voxel(&c->prof, c->stream, c->ws.sor_pts, c->ws.sor_n, 0, nullptr, leaf, 0, 0.f, final_dst, c->cc_host_dev);
        } else {
            launch_small_frame(&c->prof, c->stream, a, (const float*)kp_d, n_kp, downsample ? 1 : 0, leaf, c->ws.pts, final_dst, c->cc_host_dev,
                               nullptr, nullptr);
        }
        HIPCHK(hipGetLastError());
        if (mem == O3DR_MEM_HOST)
            HIPCHK(hipMemcpyAsync(c->small_host, final_dst, (size_t)cap * sizeof(o3dr_point), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        const CloudCounters cc = *c->cc_host;
        if (cc.status & O3DR_STATUS_INTERNAL)
            return fail(O3DR_ERR_INTERNAL, "a device-side gather guard tripped (record or point id outside its cloud); results are invalid");
        if ((int64_t)cc.count > cap) return fail(O3DR_ERR_INTERNAL, "the one-workgroup path returned more points than it was given");
        if (mem == O3DR_MEM_HOST) {
            if ((int64_t)cc.count > out_capacity) return fail(O3DR_ERR_CAPACITY, "output buffer too small");
            memcpy(out, c->small_host, (size_t)cc.count * sizeof(o3dr_point));
        }
        *n_out = (int64_t)cc.count;
        if (status) *status = cc.status;
        return O3DR_OK;
    } else if (!downsample) {
        CHK(run_reproject_single(c, (const uint8_t*)disp_d, disp_pitch, (const uint8_t*)bgr_d, bgr_pitch, rows, cols, g,
                                 T, (const float*)kp_d, n_kp, final_dst));
        uint32_t nv = 0;
        CHK(read_u32(c, c->ws.n_valid, &nv));
        n_final = nv;
    } else {
        CHK(run_reproject_single(c, (const uint8_t*)disp_d, disp_pitch, (const uint8_t*)bgr_d, bgr_pitch, rows, cols, g,
                                 T, (const float*)kp_d, n_kp, c->ws.pts));
        CHK(zero_counters(c, c->cc_tmp));
        const float lf = (float)(c->params.voxel_size / 5);  // pose_functions.cpp:1698
        const float leaf[3] = {lf, lf, lf};
        VoxelArgs v = voxel_args(c->ws.pts, 0, c->ws.n_valid, 1, cap, leaf);
        v.out_base = final_dst;
        v.cc = c->cc_tmp;
        v.mm_used = (int)((g.n + kEmitTile - 1) / kEmitTile) + 1;
        v.stats = c->stats_dev;
        if (sor_on(c)) CHK(sor_in_front(c, v));  // in front of the per-frame voxel grid
        launch_voxel_grid(&c->prof, c->stream, c->ws, v);
        HIPCHK(hipGetLastError());
        CloudCounters cc;
        CHK(read_counters(c, c->cc_tmp, &cc));
        n_final = (int64_t)cc.count;
        st = cc.status;
    }
    if (mem == O3DR_MEM_HOST) {
        if (n_final > out_capacity) return fail(O3DR_ERR_CAPACITY, "output buffer too small");
        if (n_final > 0) {
            HIPCHK(hipMemcpyAsync(out, final_dst, (size_t)n_final * sizeof(o3dr_point), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
    }
    *n_out = n_final;
    if (status) *status = st;
    return O3DR_OK;
}

extern "C" int o3dr_create_single_img_pt_cloud(o3dr_ctx* c, const uint8_t* disp, int64_t disp_pitch, const uint8_t* bgr,
                                               int64_t bgr_pitch, int32_t rows, int32_t cols, const float* kp_xy,
                                               int32_t n_kp, o3dr_point* out, int64_t out_capacity, int64_t* n_out,
                                               int32_t mem)
{
    return frame_call(c, disp, disp_pitch, bgr, bgr_pitch, rows, cols, nullptr, kp_xy, n_kp, false, out, out_capacity,
                      n_out, nullptr, mem);
}

extern "C" int o3dr_reproject_transform(o3dr_ctx* c, const uint8_t* disp, int64_t disp_pitch, const uint8_t* bgr,
                                        int64_t bgr_pitch, int32_t rows, int32_t cols, const float T[16],
                                        const float* kp_xy, int32_t n_kp, o3dr_point* out, int64_t out_capacity,
                                        int64_t* n_out, int32_t mem)
{
    if (!T) {
        if (n_out) *n_out = 0;
        return fail(O3DR_ERR_INVALID_ARG, "T is NULL");
    }
    return frame_call(c, disp, disp_pitch, bgr, bgr_pitch, rows, cols, T, kp_xy, n_kp, false, out, out_capacity, n_out,
                      nullptr, mem);
}

extern "C" int o3dr_create_and_transform_pt_cloud(o3dr_ctx* c, const uint8_t* disp, int64_t disp_pitch,
                                                  const uint8_t* bgr, int64_t bgr_pitch, int32_t rows, int32_t cols,
                                                  const float T[16], const float* kp_xy, int32_t n_kp, o3dr_point* out,
                                                  int64_t out_capacity, int64_t* n_out, uint32_t* status, int32_t mem)
{
    if (!T) {
        if (n_out) *n_out = 0;
        return fail(O3DR_ERR_INVALID_ARG, "T is NULL");
    }
    const bool ds = c ? !c->params.dont_downsample : true;
    return frame_call(c, disp, disp_pitch, bgr, bgr_pitch, rows, cols, T, kp_xy, n_kp, ds, out, out_capacity, n_out,
                      status, mem);
}

extern "C" int o3dr_transform_pt_cloud(o3dr_ctx* c, const o3dr_point* in, int64_t n, const float T[16], o3dr_point* out,
                                       int32_t mem)
{
    CTX_ENTER(c);
    if (n < 0 || !T || (n > 0 && (!in || !out))) return fail(O3DR_ERR_INVALID_ARG, "bad arguments");
    if (n == 0) return O3DR_OK;
    if (mem == O3DR_MEM_DEVICE) {
        launch_transform(&c->prof, c->stream, in, n, T, out);
        HIPCHK(hipGetLastError());
        return O3DR_OK;
    }
    const void* in_d;
    CHK(stage_in(c, c->st_in, in, (size_t)n * sizeof(o3dr_point), mem, &in_d));
    launch_transform(&c->prof, c->stream, (const o3dr_point*)in_d, n, T, (o3dr_point*)c->st_in.p);  // in place
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, c->st_in.p, (size_t)n * sizeof(o3dr_point), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

// one stand-alone voxel grid over a device cloud -> device destination; returns count + status
// write a host-supplied bounding box (min xyz, max xyz) into bounding-box slot 0 of frame 0
static int put_bbox(o3dr_ctx* c, const float mn[3], const float mx[3])
{
    float* h = (float*)c->misc_host;
    for (int a = 0; a < 3; ++a) h[a] = mn[a], h[3 + a] = mx[a];
    HIPCHK(hipMemcpyAsync(c->ws.mm, h, 6 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return O3DR_OK;
}

static int voxel_single(o3dr_ctx* c, const o3dr_point* in_d, int64_t n_in, const float leaf[3], uint32_t min_points,
                        float z_offset, o3dr_point* out_d, int64_t* n_out, uint32_t* status,
                        const float* gmin = nullptr, const float* gmax = nullptr, bool do_sor = false,
                        const float* box_dev = nullptr, const uint8_t* heads_in = nullptr, CloudCounters* big_out = nullptr)
{
    CHK(ws_ensure(c, 1, n_in, false, c->use_runs != 0));
    if (c->small_path && n_in <= kSmallMax && !c->test_corrupt) {  // one launch of one workgroup (kernels/small.inc)
        const float* box = box_dev;
        if (gmin && gmax) {
            CHK(put_bbox(c, gmin, gmax));
            box = c->ws.mm;
        }
        if (do_sor) {  // ... after the outlier removal's five
            CHK(sor_ensure(c, 1, n_in));
            launch_set_counts(&c->prof, c->stream, c->ws.n_valid, (uint32_t)n_in, 1);
            launch_sor_small(&c->prof, c->stream, c->ws, in_d, c->ws.n_valid, n_in, 1.0, c->ws.sor_pts, c->ws.sor_n);
            launch_small_voxel(&c->prof, c->stream, c->ws.sor_pts, c->ws.sor_n, 0, box, leaf, min_points, z_offset, out_d, c->cc_tmp);
        } else {
            launch_small_voxel(&c->prof, c->stream, in_d, nullptr, (uint32_t)n_in, box, leaf, min_points, z_offset, out_d, c->cc_tmp);
        }
        HIPCHK(hipGetLastError());
        CloudCounters cc;
        if (big_out)
            CHK(read_counters(c, c->cc_tmp, &cc, c->cc_big, big_out));
        else
            CHK(read_counters(c, c->cc_tmp, &cc));
        *n_out = (int64_t)cc.count;
        if (status) *status = cc.status;
        return O3DR_OK;
    }
    launch_set_counts(&c->prof, c->stream, c->ws.n_valid, (uint32_t)n_in, 1);
    int mm_used = 1;
    if (gmin && gmax)  // grid laid over a caller-supplied (global) box instead of this cloud's own
        CHK(put_bbox(c, gmin, gmax));
    else if (box_dev)  // the cloud's own box is already known on the device
        HIPCHK(hipMemcpyAsync(c->ws.mm, box_dev, 6 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    else
        mm_used = launch_points_minmax(&c->prof, c->stream, in_d, 0, c->ws.n_valid, 1, n_in, c->ws.mm_stride, c->ws.mm);
    CHK(zero_counters(c, c->cc_tmp));
    VoxelArgs v = voxel_args(in_d, 0, c->ws.n_valid, 1, n_in, leaf, z_offset, min_points);
    v.out_base = out_d;
    v.cc = c->cc_tmp;
    v.mm_used = mm_used;
    v.stats = c->stats_dev;
    v.use_runs = c->use_runs;
    v.heads_in = heads_in;
    v.test_corrupt = c->test_corrupt;
    c->test_corrupt = 0;
    if (do_sor) CHK(sor_in_front(c, v));
    launch_voxel_grid(&c->prof, c->stream, c->ws, v);
    HIPCHK(hipGetLastError());
    CloudCounters cc;
    if (big_out)
        CHK(read_counters(c, c->cc_tmp, &cc, c->cc_big, big_out));
    else
        CHK(read_counters(c, c->cc_tmp, &cc));
    *n_out = (int64_t)cc.count;
    if (status) *status = cc.status;
    return O3DR_OK;
}

static int voxel_grid_impl(o3dr_ctx* c, const o3dr_point* in, int64_t n_in, const float leaf[3], uint32_t min_points,
                           float z_offset, o3dr_point* out, int64_t out_capacity, int64_t* n_out, uint32_t* status,
                           int32_t mem, bool do_sor)
{
    if (n_out) *n_out = 0;
    if (status) *status = 0;
    CTX_ENTER(c);
    if (!n_out || n_in < 0 || !leaf || (n_in > 0 && (!in || !out))) return fail(O3DR_ERR_INVALID_ARG, "bad arguments");
    if (!(leaf[0] > 0) || !(leaf[1] > 0) || !(leaf[2] > 0)) return fail(O3DR_ERR_INVALID_ARG, "leaf must be positive");
    if (n_in >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "more than 2^32-1 points in one cloud");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (n_in == 0) return O3DR_OK;
    if (out_capacity < n_in && mem == O3DR_MEM_DEVICE)
        return fail(O3DR_ERR_CAPACITY, "device output must hold n_in points (overflow fallback returns the input)");
    const void* in_d;
    CHK(stage_in(c, c->st_in, in, (size_t)n_in * sizeof(o3dr_point), mem, &in_d));
    o3dr_point* out_d = out;
    if (mem == O3DR_MEM_HOST) {
        CHK(dev_ensure(c, c->st_out, (size_t)n_in * sizeof(o3dr_point)));
        out_d = (o3dr_point*)c->st_out.p;
    }
    int64_t m = 0;
    uint32_t st = 0;
    CHK(voxel_single(c, (const o3dr_point*)in_d, n_in, leaf, min_points, z_offset, out_d, &m, &st, nullptr, nullptr, do_sor));
    if (mem == O3DR_MEM_HOST) {
        if (m > out_capacity) return fail(O3DR_ERR_CAPACITY, "output buffer too small");
        if (m > 0) {
            HIPCHK(hipMemcpyAsync(out, out_d, (size_t)m * sizeof(o3dr_point), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
    }
    *n_out = m;
    if (status) *status = st;
    return O3DR_OK;
}

extern "C" int o3dr_voxel_grid(o3dr_ctx* c, const o3dr_point* in, int64_t n_in, const float leaf[3], uint32_t min_points,
                               float z_offset, o3dr_point* out, int64_t out_capacity, int64_t* n_out, uint32_t* status,
                               int32_t mem)
{
    return voxel_grid_impl(c, in, n_in, leaf, min_points, z_offset, out, out_capacity, n_out, status, mem, false);
}

// A3b alone: pcl::StatisticalOutlierRemoval with mean_k 50, stddev_mul 1.0 (pose_functions.cpp:1679-1684)
extern "C" int o3dr_statistical_outlier_removal(o3dr_ctx* c, const o3dr_point* in, int64_t n_in, o3dr_point* out,
                                                int64_t out_capacity, int64_t* n_out, int32_t mem)
{
    if (n_out) *n_out = 0;
    CTX_ENTER(c);
    if (!n_out || n_in < 0 || (n_in > 0 && (!in || !out))) return fail(O3DR_ERR_INVALID_ARG, "bad arguments");
    if (n_in >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "more than 2^32-1 points in one cloud");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (n_in == 0) return O3DR_OK;
    if (out_capacity < n_in) return fail(O3DR_ERR_CAPACITY, "output must hold n_in points");
    const void* in_d;
    CHK(stage_in(c, c->st_in, in, (size_t)n_in * sizeof(o3dr_point), mem, &in_d));
    CHK(ws_ensure(c, 1, n_in, false));
    CHK(sor_ensure(c, 1, n_in));
    launch_set_counts(&c->prof, c->stream, c->ws.n_valid, (uint32_t)n_in, 1);
    o3dr_point* dst = mem == O3DR_MEM_DEVICE ? out : c->ws.sor_pts;
    if (c->small_path && n_in <= kSmallMax) {  // 6 launches instead of ~32 (kernels/small.inc)
        launch_sor_small(&c->prof, c->stream, c->ws, (const o3dr_point*)in_d, c->ws.n_valid, n_in, 1.0, dst, c->ws.sor_n);
    } else {
        const int used = launch_points_minmax(&c->prof, c->stream, (const o3dr_point*)in_d, 0, c->ws.n_valid, 1, n_in, c->ws.mm_stride, c->ws.mm);
        launch_sor(&c->prof, c->stream, c->ws, (const o3dr_point*)in_d, 0, c->ws.n_valid, 1, n_in, used, 1.0, dst, 0, c->ws.sor_n);
    }
    HIPCHK(hipGetLastError());
    uint32_t m = 0;
    CHK(read_u32(c, c->ws.sor_n, &m));
    if (mem == O3DR_MEM_HOST && m > 0) {
        HIPCHK(hipMemcpyAsync(out, dst, (size_t)m * sizeof(o3dr_point), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    *n_out = (int64_t)m;
    return O3DR_OK;
}

static void downsample_leaf(const o3dr_params& p, int combined, float leaf[3], uint32_t* min_pts, float* z_offset)
{
    if (combined) {  // pose_functions.cpp:1666,1693-1694
        leaf[0] = leaf[1] = (float)p.voxel_size;
        leaf[2] = 1000.f;
        *min_pts = p.min_points_per_voxel;
        *z_offset = 500.f;
    } else {  // :1698
        leaf[0] = leaf[1] = leaf[2] = (float)(p.voxel_size / 5);
        *min_pts = 0;
        *z_offset = 0.f;
    }
}

extern "C" int o3dr_downsample_pt_cloud(o3dr_ctx* c, const o3dr_point* in, int64_t n_in, int32_t combined,
                                        o3dr_point* out, int64_t out_capacity, int64_t* n_out, uint32_t* status,
                                        int32_t mem)
{
    if (!c) {
        if (n_out) *n_out = 0;
        return fail(O3DR_ERR_INVALID_ARG, "ctx is NULL");
    }
    float leaf[3], zo;
    uint32_t mp;
    downsample_leaf(c->params, combined, leaf, &mp, &zo);
    // statistical outlier removal iff !combinedPtCloud && jump_pixels > 0 (pose_functions.cpp:1673), when enabled
    return voxel_grid_impl(c, in, n_in, leaf, mp, zo, out, out_capacity, n_out, status, mem, !combined && sor_on(c));
}

// -------------------------------------------------------------------------------------------------
// A7: device-resident accumulation
// -------------------------------------------------------------------------------------------------
// the group-run head flags of cloud_big: one byte per 4 points (+ slack for the last wave's word), tied to cloud_cap.
// keep: carry the flags recorded so far over.  On failure the old buffer is gone and nothing is recorded.
static inline size_t heads_bytes(int64_t points) { return ((size_t)points / 4 + 64 + 3) & ~(size_t)3; }
static int heads_resize(o3dr_ctx* c, int64_t points, bool keep)
{
    if (c->cloud_heads && c->cloud_heads_cap >= points) return O3DR_OK;
    const size_t bytes = heads_bytes(points);
    uint32_t* nf = nullptr;
    if (hipMalloc((void**)&nf, bytes) != hipSuccess) {
        (void)hipGetLastError();
        nf = nullptr;
    }
    if (nf && hipMemsetAsync(nf, 0, bytes, c->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(nf);
        nf = nullptr;
    }
    if (c->cloud_heads) {
        if (nf && keep) {
            const size_t old = heads_bytes(c->cloud_heads_cap);
            (void)hipMemcpyAsync(nf, c->cloud_heads, old < bytes ? old : bytes, hipMemcpyDeviceToDevice, c->stream);
        }
        (void)hipStreamSynchronize(c->stream);  // earlier launches may still write the old flags
        (void)hipFree(c->cloud_heads);
    }
    c->cloud_heads = nf;
    c->cloud_heads_cap = nf ? points : 0;
    return nf ? O3DR_OK : fail(O3DR_ERR_ALLOC, "hipMalloc failed (cloud_big run heads)");
}

static int cloud_reserve(o3dr_ctx* c, int64_t need)
{
    if (need <= c->cloud_cap) return O3DR_OK;
    int64_t want = c->cloud_cap * 2;
    if (want < need) want = need;
    o3dr_point* nb = nullptr;
    if (hipMalloc((void**)&nb, (size_t)want * sizeof(o3dr_point)) != hipSuccess) {
        (void)hipGetLastError();
        want = need;
        if (hipMalloc((void**)&nb, (size_t)want * sizeof(o3dr_point)) != hipSuccess)
            return fail(O3DR_ERR_ALLOC, "hipMalloc failed (cloud_big)");
    }
    if (c->cloud_big) {
        CloudCounters cc;
        CHK(read_counters(c, c->cc_big, &cc));
        if (cc.count)
            HIPCHK(hipMemcpyAsync(nb, c->cloud_big, (size_t)cc.count * sizeof(o3dr_point), hipMemcpyDeviceToDevice,
                                  c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(c->cloud_big));
        c->cloud_ub = (int64_t)cc.count;
    }
    c->cloud_big = nb;
    c->cloud_cap = want;
    // the flag buffer follows the cloud's capacity (zeros where nothing was recorded yet); without it the heads are
    // simply not recorded (the merge then reads the points for them): never a reason to fail the reservation
    if (c->cloud_box_enable && heads_resize(c, want, true) != O3DR_OK) c->cloud_heads_valid = false;
    return O3DR_OK;
}

// make room for `extra` more points; tightens the host-side bound with one sync when it must
static int cloud_make_room(o3dr_ctx* c, int64_t extra)
{
    if (c->cloud_ub + extra > c->cloud_cap) {
        CloudCounters cc;
        CHK(read_counters(c, c->cc_big, &cc));
        c->cloud_ub = (int64_t)cc.count;
        if (c->cloud_ub + extra > c->cloud_cap) CHK(cloud_reserve(c, c->cloud_ub + extra));
    }
    return O3DR_OK;
}

// the alternate cloud buffer with room for `need` points (contents undefined)
static int alt_reserve(o3dr_ctx* c, int64_t need)
{
    if (need <= c->cloud_alt_cap) return O3DR_OK;
    if (c->cloud_alt) {
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipFree(c->cloud_alt));
        c->cloud_alt = nullptr;
        c->cloud_alt_cap = 0;
    }
    if (hipMalloc((void**)&c->cloud_alt, (size_t)need * sizeof(o3dr_point)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(O3DR_ERR_ALLOC, "hipMalloc failed (alternate cloud buffer)");
    }
    c->cloud_alt_cap = need;
    return O3DR_OK;
}
static void swap_clouds(o3dr_ctx* c)
{
    o3dr_point* p = c->cloud_big;
    const int64_t cap = c->cloud_cap;
    c->cloud_big = c->cloud_alt;
    c->cloud_cap = c->cloud_alt_cap;
    c->cloud_alt = p;
    c->cloud_alt_cap = cap;
}

extern "C" int o3dr_cloud_big_reserve(o3dr_ctx* c, int64_t n_points)
{
    CTX_ENTER(c);
    if (n_points < 0) return fail(O3DR_ERR_INVALID_ARG, "negative size");
    return cloud_reserve(c, n_points);
}

static int cloud_box_clear(o3dr_ctx* c)
{
    static const float empty[6] = {__builtin_inff(), __builtin_inff(), __builtin_inff(),
                                   -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    HIPCHK(hipMemcpyAsync(c->cloud_box, empty, sizeof empty, hipMemcpyHostToDevice, c->stream));
    c->cloud_box_valid = c->cloud_box_enable != 0;
    // the flag buffer must cover the cloud buffer in use NOW: partition / adopt swap in the alternate buffer, whose
    // capacity the flags know nothing about (a smaller flag buffer would be written past its end by the next appends)
    if (c->cloud_box_enable && c->cloud_cap > 0 && c->cloud_heads_cap < c->cloud_cap) (void)heads_resize(c, c->cloud_cap, false);
    if (c->cloud_heads) HIPCHK(hipMemsetAsync(c->cloud_heads, 0, heads_bytes(c->cloud_heads_cap), c->stream));
    c->cloud_heads_valid = c->cloud_box_enable != 0 && c->cloud_heads && c->cloud_heads_cap >= c->cloud_cap;
    return O3DR_OK;
}

// frame calls that append to cloud_big also record where its group runs start, for the merge's grid
static void heads_for_append(o3dr_ctx* c, VoxelArgs& v)
{
    if (!c->cloud_heads_valid || !c->cloud_heads) return;
    if (c->cloud_heads_cap < c->cloud_cap) {  // (never expected: cloud_reserve and cloud_box_clear keep them together)
        c->cloud_heads_valid = false;
        return;
    }
    float leaf[3], zo;
    uint32_t mp;
    downsample_leaf(c->params, 1, leaf, &mp, &zo);
    const bool same = leaf[0] == c->cloud_heads_leaf[0] && leaf[1] == c->cloud_heads_leaf[1] && leaf[2] == c->cloud_heads_leaf[2] &&
                      zo == c->cloud_heads_zo;
    if (c->cloud_ub == 0) {  // an empty cloud takes the current leaf
        for (int a = 0; a < 3; ++a) c->cloud_heads_leaf[a] = leaf[a];
        c->cloud_heads_zo = zo;
    } else if (!same) {  // voxel_size changed while the cloud was growing: the flags describe no single grid
        c->cloud_heads_valid = false;
        return;
    }
    v.cloud_heads.flags = c->cloud_heads;
    for (int a = 0; a < 3; ++a) v.cloud_heads.inv[a] = 1.0f / leaf[a];
    v.cloud_heads.z_offset = zo;
}
// ... and the merge takes them instead of reading the cloud once more
static const uint8_t* heads_for_merge(o3dr_ctx* c, const float leaf[3], float zo)
{
    if (!c->cloud_heads_valid || !c->cloud_heads) return nullptr;
    if (leaf[0] != c->cloud_heads_leaf[0] || leaf[1] != c->cloud_heads_leaf[1] || leaf[2] != c->cloud_heads_leaf[2] ||
        zo != c->cloud_heads_zo)
        return nullptr;
    return reinterpret_cast<const uint8_t*>(c->cloud_heads);
}

extern "C" int o3dr_cloud_big_reset(o3dr_ctx* c)
{
    CTX_ENTER(c);
    ++c->cloud_gen;
    CHK(zero_counters(c, c->cc_big));
    CHK(cloud_box_clear(c));
    c->cloud_ub = 0;
    c->cloud_n_exact = true;
    return O3DR_OK;
}

extern "C" int o3dr_cloud_big_size(o3dr_ctx* c, int64_t* n, uint32_t* status)
{
    if (n) *n = 0;
    CTX_ENTER(c);
    CloudCounters cc;
    CHK(read_counters(c, c->cc_big, &cc));
    c->cloud_ub = (int64_t)cc.count;
    if (n) *n = (int64_t)cc.count;
    if (status) *status = cc.status;
    return O3DR_OK;
}

extern "C" int o3dr_cloud_big_read(o3dr_ctx* c, o3dr_point* out, int64_t out_capacity, int64_t* n_out, int32_t mem)
{
    if (n_out) *n_out = 0;
    CTX_ENTER(c);
    if (!n_out) return fail(O3DR_ERR_INVALID_ARG, "n_out is NULL");
    CloudCounters cc;
    CHK(read_counters(c, c->cc_big, &cc));
    const int64_t n = (int64_t)cc.count;
    if (n > out_capacity) return fail(O3DR_ERR_CAPACITY, "output buffer too small");
    if (n > 0) {
        if (!out) return fail(O3DR_ERR_INVALID_ARG, "out is NULL");
        HIPCHK(hipMemcpyAsync(out, c->cloud_big, (size_t)n * sizeof(o3dr_point),
                              mem == O3DR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    *n_out = n;
    return O3DR_OK;
}

// appends n points and bumps the device counter (passthrough voxel job with a known count)
extern "C" int o3dr_cloud_big_append(o3dr_ctx* c, const o3dr_point* pts, int64_t n, int32_t mem)
{
    CTX_ENTER(c);
    if (n < 0 || (n > 0 && !pts)) return fail(O3DR_ERR_INVALID_ARG, "bad arguments");
    if (n == 0) return O3DR_OK;
    if (n >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "more than 2^32-1 points in one append");
    CHK(cloud_make_room(c, n));
    const void* src;
    CHK(stage_in(c, c->st_in, pts, (size_t)n * sizeof(o3dr_point), mem, &src));
    CHK(ws_ensure(c, 1, 1, false));
    launch_set_counts(&c->prof, c->stream, c->ws.n_valid, (uint32_t)n, 1);
    const float unit_leaf[3] = {1.f, 1.f, 1.f};
    VoxelArgs v = voxel_args((const o3dr_point*)src, 0, c->ws.n_valid, 1, n, unit_leaf);
    v.out_base = c->cloud_big;
    v.cc = c->cc_big;
    v.passthrough = 1;
    c->cloud_box_valid = false;  // appended points are not tracked
    c->cloud_heads_valid = false;
    launch_voxel_grid(&c->prof, c->stream, c->ws, v);
    HIPCHK(hipGetLastError());
    c->cloud_ub += n;
    if (mem == O3DR_MEM_HOST) HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_cloud_big_transform(o3dr_ctx* c, const float T[16])
{
    CTX_ENTER(c);
    if (!T) return fail(O3DR_ERR_INVALID_ARG, "T is NULL");
    CloudCounters cc;
    CHK(read_counters(c, c->cc_big, &cc));
    ++c->cloud_gen;
    launch_transform(&c->prof, c->stream, c->cloud_big, (int64_t)cc.count, T, c->cloud_big);
    HIPCHK(hipGetLastError());
    c->cloud_box_valid = false;
    c->cloud_heads_valid = false;
    return O3DR_OK;
}

static int accumulate_impl(o3dr_ctx* c, const uint8_t* disp, int64_t disp_frame_stride, int64_t disp_pitch,
                           const uint8_t* bgr, int64_t bgr_frame_stride, int64_t bgr_pitch, int32_t rows, int32_t cols,
                           const float* poses, int32_t n_frames, const float* kp_xy, const int64_t* kp_offsets, int32_t mem)
{
    CTX_ENTER(c);
    if (!c->has_Q) return fail(O3DR_ERR_NOT_CONFIGURED, "o3dr_set_camera has not been called");
    if (n_frames < 0 || (n_frames > 0 && !poses)) return fail(O3DR_ERR_INVALID_ARG, "bad frame list");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (n_frames == 0) return O3DR_OK;
    CHK(check_images(c, disp, disp_pitch, bgr, bgr_pitch, rows, cols, disp_frame_stride));
    if (disp_frame_stride < (int64_t)rows * disp_pitch || bgr_frame_stride < (int64_t)rows * bgr_pitch)
        return fail(O3DR_ERR_INVALID_ARG, "frame stride smaller than a frame");
    const GridShape g = grid_shape(c->params, rows, cols);
    // keypoint pass (pose_functions.cpp:1057-1091): active iff jump_pixels != 1, emitted before the grid points
    int64_t kp_total = 0, kp_max = 0;
    if (kp_offsets && c->params.jump_pixels != 1) {
        for (int f = 0; f < n_frames; ++f) {
            const int64_t k = kp_offsets[f + 1] - kp_offsets[f];
            if (k < 0) return fail(O3DR_ERR_INVALID_ARG, "kp_offsets must not decrease");
            if (k > kp_max) kp_max = k;
        }
        kp_total = kp_offsets[n_frames] - kp_offsets[0];
        if (kp_total > 0 && !kp_xy) return fail(O3DR_ERR_INVALID_ARG, "kp_xy is NULL");
        if (kp_total >= (int64_t)INT32_MAX) return fail(O3DR_ERR_INVALID_ARG, "too many keypoints");
    }
    const bool use_kp = kp_total > 0;
    const int64_t cap = g.n + kp_max;  // points a frame can produce: capacity of every per-frame buffer below
    if (cap == 0) return O3DR_OK;      // jump_pixels == 0 without keypoints: nothing to add
    const float* kp_d = nullptr;
    const int32_t* kpoff_d = nullptr;
    std::vector<int32_t> kp_rel;
    if (use_kp) {
        const void* p;
        CHK(stage_in(c, c->st_kp, kp_xy + 2 * kp_offsets[0], (size_t)kp_total * 2 * sizeof(float), mem, &p));
        kp_d = (const float*)p;
        kp_rel.resize((size_t)n_frames + 1);
        for (int f = 0; f <= n_frames; ++f) kp_rel[f] = (int32_t)(kp_offsets[f] - kp_offsets[0]);
        HIPCHK(hipStreamSynchronize(c->stream));  // an earlier call's launches may still read the offsets
        CHK(dev_ensure(c, c->st_kpoff, kp_rel.size() * sizeof(int32_t)));
        HIPCHK(hipMemcpy(c->st_kpoff.p, kp_rel.data(), kp_rel.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        kpoff_d = (const int32_t*)c->st_kpoff.p;
    }
    float leaf[3], zo;
    uint32_t mp;
    downsample_leaf(c->params, 0, leaf, &mp, &zo);
    // statistical outlier removal (pose_functions.cpp:1673-1686, in front of every per-frame voxel grid): batched like
    // everything else - grid y = frame in all of its kernels, no host round trip per frame
    const bool with_sor = sor_on(c) && !c->params.dont_downsample;
    int B = n_frames < c->max_batch ? n_frames : c->max_batch;
    {   // ~56 bytes of workspace per candidate point; keep a batch under 12 GiB of HBM (of 288)
        const int64_t per_frame = (with_sor ? 56 + 50 : 56) * cap + (1 << 20);
        const int64_t fit = ((int64_t)12 << 30) / per_frame;
        if (fit < B) B = fit < 1 ? 1 : (int)fit;
    }
    // Host buffers: frames cross PCIe once.  Upload batch k+1 on a second stream while batch k
    // computes (two staging sets); smaller batches than the HBM-resident path so that they overlap
    // (clamped BEFORE the workspaces are sized: a streaming call never launches more than host_batch frames)
    const bool streaming = mem == O3DR_MEM_HOST;
    if (streaming && c->host_batch < B) B = c->host_batch;
    CHK(ws_ensure(c, B, cap, true));
    if (with_sor) CHK(sor_ensure(c, B, cap));

    if (streaming) {
        if (!c->copy_stream) HIPCHK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        for (int i = 0; i < 2; ++i) {
            if (!c->ev_copied[i]) HIPCHK(hipEventCreateWithFlags(&c->ev_copied[i], hipEventDisableTiming));
            if (!c->ev_done[i]) HIPCHK(hipEventCreateWithFlags(&c->ev_done[i], hipEventDisableTiming));
        }
        HIPCHK(hipStreamSynchronize(c->stream));  // staging sets are free, events start clean
    }
    int slot = 0;
    for (int f0 = 0; f0 < n_frames; f0 += B, slot ^= 1) {
        const int nb = (n_frames - f0) < B ? (n_frames - f0) : B;
        CHK(cloud_make_room(c, (int64_t)nb * cap));
        const void *disp_d, *bgr_d, *poses_d;
        if (streaming) {
            const size_t db = (size_t)nb * disp_frame_stride, cb = (size_t)nb * bgr_frame_stride, pb = (size_t)nb * 16 * sizeof(float);
            CHK(dev_ensure(c, c->st2_disp[slot], db));
            CHK(dev_ensure(c, c->st2_bgr[slot], cb));
            CHK(dev_ensure(c, c->st2_poses[slot], pb));
            if (f0 >= 2 * B) HIPCHK(hipStreamWaitEvent(c->copy_stream, c->ev_done[slot], 0));  // set's previous user finished
            HIPCHK(hipMemcpyAsync(c->st2_disp[slot].p, disp + (int64_t)f0 * disp_frame_stride, db, hipMemcpyHostToDevice, c->copy_stream));
            HIPCHK(hipMemcpyAsync(c->st2_bgr[slot].p, bgr + (int64_t)f0 * bgr_frame_stride, cb, hipMemcpyHostToDevice, c->copy_stream));
            HIPCHK(hipMemcpyAsync(c->st2_poses[slot].p, poses + 16 * (int64_t)f0, pb, hipMemcpyHostToDevice, c->copy_stream));
            HIPCHK(hipEventRecord(c->ev_copied[slot], c->copy_stream));
            HIPCHK(hipStreamWaitEvent(c->stream, c->ev_copied[slot], 0));
            disp_d = c->st2_disp[slot].p;
            bgr_d = c->st2_bgr[slot].p;
            poses_d = c->st2_poses[slot].p;
        } else {
            disp_d = disp + (int64_t)f0 * disp_frame_stride;
            bgr_d = bgr + (int64_t)f0 * bgr_frame_stride;
            poses_d = poses + 16 * (int64_t)f0;
        }
        const uint8_t* dsp = (const uint8_t*)disp_d;
        int64_t dsp_pitch = disp_pitch, dsp_fstride = disp_frame_stride;
        CHK(maybe_blur(c, &dsp, &dsp_pitch, &dsp_fstride, rows, cols, nb));
        ReprojectArgs a;
        fill_args(c, a, dsp, dsp_pitch, dsp_fstride, (const uint8_t*)bgr_d, bgr_pitch,
                  bgr_frame_stride, rows, cols, g, cap);
        a.xf_mode = 2;
        a.poses = (const float*)poses_d;
        for (int i = 0; i < 3; ++i) a.slab_inv[i] = 1.0f / leaf[i];
        a.slab_shift = slab_shift_for(c, rows, cols, leaf);
        // no keypoint pass in front of the grid pass and a voxel grid behind it: index and first digit histogram are
        // produced by the pass that writes the points (the keypoint pass would need them too: it keeps the two-step form)
        const bool fused = !use_kp && !c->params.dont_downsample && a.n_tiles > 0 && !with_sor;
        // the neutral keypoint slot and n_kp = 0 (nothing in front of the passes below writes either; the keypoint pass
        // overwrites both): a launch of its own, or the work of the fused path's first pass
        if (!(fused && reproject_fused_inits(a, !c->exact_box)))
            launch_minmax_init(&c->prof, c->stream, c->ws.mm, c->ws.mm_stride, a.n_tiles, c->ws.n_kp, nb);
        if (use_kp)
            launch_keypoint_pass(&c->prof, c->stream, a, kp_d, 0, c->ws.pts, c->ws.n_kp, c->ws.mm, kpoff_d + f0, nb);
        int emit_tiles = 0;
        if (fused)
            emit_tiles = launch_reproject_fused(&c->prof, c->stream, c->ws, a, nb, cap, leaf, !c->exact_box);
        else
            launch_reproject(&c->prof, c->stream, a, nb, c->ws.pts, c->ws.tile_cnt, c->ws.n_kp, c->ws.n_valid, c->ws.mm,
                             c->ws.scan_partial);
        VoxelArgs v = voxel_args(c->ws.pts, cap, c->ws.n_valid, nb, cap, leaf, zo, mp);
        v.keys_ready = fused ? 1 : 0;
        v.emit_tiles = emit_tiles;
        v.cloud_box = c->cloud_box_valid ? c->cloud_box : nullptr;
        heads_for_append(c, v);
        v.out_base = c->cloud_big;
        v.cc = c->cc_big;
        v.passthrough = c->params.dont_downsample ? 1 : 0;
        v.mm_used = a.n_tiles + 1;
        v.stats = c->stats_dev;
        v.test_corrupt = c->test_corrupt;  // (o3dr_test_corrupt_next_gather: the first batch takes it)
        c->test_corrupt = 0;
        if (with_sor) CHK(sor_in_front(c, v, false));  // (the buffers were sized for all batches above)
        launch_voxel_grid(&c->prof, c->stream, c->ws, v);
        HIPCHK(hipGetLastError());
        c->cloud_ub += (int64_t)nb * cap;
        c->cloud_n_exact = false;
        if (streaming) HIPCHK(hipEventRecord(c->ev_done[slot], c->stream));
    }
    if (streaming) HIPCHK(hipStreamSynchronize(c->stream));  // the caller may reuse its host buffers
    return O3DR_OK;
}

extern "C" int o3dr_accumulate_frames(o3dr_ctx* c, const uint8_t* disp, int64_t disp_frame_stride, int64_t disp_pitch,
                                      const uint8_t* bgr, int64_t bgr_frame_stride, int64_t bgr_pitch, int32_t rows,
                                      int32_t cols, const float* poses, int32_t n_frames, int32_t mem)
{
    return accumulate_impl(c, disp, disp_frame_stride, disp_pitch, bgr, bgr_frame_stride, bgr_pitch, rows, cols, poses, n_frames,
                           nullptr, nullptr, mem);
}
extern "C" int o3dr_accumulate_frames_kp(o3dr_ctx* c, const uint8_t* disp, int64_t disp_frame_stride, int64_t disp_pitch,
                                         const uint8_t* bgr, int64_t bgr_frame_stride, int64_t bgr_pitch, int32_t rows,
                                         int32_t cols, const float* poses, int32_t n_frames, const float* kp_xy,
                                         const int64_t* kp_offsets, int32_t mem)
{
    return accumulate_impl(c, disp, disp_frame_stride, disp_pitch, bgr, bgr_frame_stride, bgr_pitch, rows, cols, poses, n_frames,
                           kp_xy, kp_offsets, mem);
}

static int finalize_impl(o3dr_ctx* c, const float* gmin, const float* gmax, o3dr_point* out, int64_t out_capacity,
                         int64_t* n_out, uint32_t* status, int32_t mem)
{
    if (n_out) *n_out = 0;
    if (status) *status = 0;
    CTX_ENTER(c);
    if (!n_out) return fail(O3DR_ERR_INVALID_ARG, "n_out is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    // the host knows the count exactly after a read, a reset or an adopt (the multi-GPU exchange): then the status bits
    // accumulated in cc_big come back with the result's count, in the one round trip the merge needs anyway
    CloudCounters cc;
    const bool known = c->cloud_n_exact && !c->params.dont_downsample && c->cloud_ub > 0;
    if (known) {
        cc.count = (uint64_t)c->cloud_ub;
        cc.status = 0;
    } else {
        CHK(read_counters(c, c->cc_big, &cc));
    }
    const int64_t n = (int64_t)cc.count;
    if (n == 0) return O3DR_OK;
    if (n >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "cloud_big exceeds 2^32-1 points");
    if (!out) return fail(O3DR_ERR_INVALID_ARG, "out is NULL");
    if (c->params.dont_downsample) {  // pose.cpp:534-537: cloud_small = cloud_big
        if (n > out_capacity) return fail(O3DR_ERR_CAPACITY, "output buffer too small");
        return o3dr_cloud_big_read(c, out, out_capacity, n_out, mem);
    }
    float leaf[3], zo;
    uint32_t mp;
    downsample_leaf(c->params, 1, leaf, &mp, &zo);
    o3dr_point* out_d = out;
    if (mem == O3DR_MEM_HOST) {
        CHK(dev_ensure(c, c->st_out, (size_t)n * sizeof(o3dr_point)));
        out_d = (o3dr_point*)c->st_out.p;
    } else if (out_capacity < n) {
        return fail(O3DR_ERR_CAPACITY, "device output must hold cloud_big (overflow fallback returns the input)");
    }
    int64_t m = 0;
    uint32_t st = 0;
    CHK(voxel_single(c, c->cloud_big, n, leaf, mp, zo, out_d, &m, &st, gmin, gmax, false,
                     c->cloud_box_valid ? c->cloud_box : nullptr, heads_for_merge(c, leaf, zo), known ? &cc : nullptr));
    if ((int64_t)cc.count != n) return fail(O3DR_ERR_INTERNAL, "cloud_big's device count differs from the host's");
    if (mem == O3DR_MEM_HOST) {
        if (m > out_capacity) return fail(O3DR_ERR_CAPACITY, "output buffer too small");
        if (m > 0) {
            HIPCHK(hipMemcpyAsync(out, out_d, (size_t)m * sizeof(o3dr_point), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
    }
    *n_out = m;
    if (status) *status = st | cc.status;
    return O3DR_OK;
}

extern "C" int o3dr_finalize(o3dr_ctx* c, o3dr_point* out, int64_t out_capacity, int64_t* n_out, uint32_t* status,
                             int32_t mem)
{
    return finalize_impl(c, nullptr, nullptr, out, out_capacity, n_out, status, mem);
}

// ---- incremental merge (kernels/incremental.inc): the combined merge of cloud_big kept as running per-cell sums ----------
static void inc_drop(o3dr_ctx* c)
{
    c->inc.valid = false;
    c->inc.folded = 0;
    c->inc.n_groups = c->inc.n_cells = 0;
}
static int64_t inc_state_bytes(const o3dr_ctx* c)
{
    size_t b = c->inc.box.cap;
    for (int i = 0; i < 2; ++i) b += c->inc.grp[i].cap + c->inc.off[i].cap + c->inc.cells[i].cap;
    return (int64_t)b;
}
// PCL's geometry of the combined grid over the box [mn, mx] (voxel_geom_of, in the same fp32 steps): 0 = the running sums
// give the merge's result; 1 = PCL's overflow guard fires; 2 = a cell coordinate reaches 2^24 in magnitude (floor(x * inv)
// and its difference to min_b are no longer exact); 3 = the uint32 linear index can wrap (distinct cells could merge)
static int inc_geometry_check(const float mn_in[3], const float mx_in[3], const float leaf[3], float zo)
{
    float inv[3], mn[3], mx[3];
    for (int a = 0; a < 3; ++a) {
        inv[a] = 1.0f / leaf[a];
        mn[a] = mn_in[a];
        mx[a] = mx_in[a];
    }
    mn[2] = mn[2] + zo;
    mx[2] = mx[2] + zo;
    double prod = 1.0;  // dx * dy * dz > INT32_MAX, d = int64((max - min) * inv) + 1
    for (int a = 0; a < 3; ++a) {
        const float e = (mx[a] - mn[a]) * inv[a];
        if (!(e < 2147483648.f)) return 1;
        prod *= (double)((int64_t)e + 1);
    }
    if (prod > (double)INT32_MAX) return 1;
    double cells = 1.0;
    for (int a = 0; a < 3; ++a) {
        const float lo = floorf(mn[a] * inv[a]), hi = floorf(mx[a] * inv[a]);
        if (!(lo > -16777216.f && hi < 16777216.f)) return 2;
        cells *= (double)(hi - lo) + 1.0;
    }
    return cells >= 4294967296.0 ? 3 : 0;
}
// o3dr_finalize's own code into a buffer of the state, then to the caller
static int inc_fallback(o3dr_ctx* c, int64_t n, o3dr_point* out, int64_t out_capacity, int64_t* n_out, uint32_t* status,
                        int32_t mem, int64_t* st)
{
    inc_drop(c);
    st[2] = 1;
    CHK(dev_ensure(c, c->inc.fb, (size_t)n * sizeof(o3dr_point)));
    int64_t m = 0;
    uint32_t s = 0;
    const int r = finalize_impl(c, nullptr, nullptr, (o3dr_point*)c->inc.fb.p, n, &m, &s, O3DR_MEM_DEVICE);
    if (r == O3DR_OK && !(out == nullptr && out_capacity == 0)) {
        if (m > out_capacity) {
            dev_release(c->inc.fb);
            return fail(O3DR_ERR_CAPACITY, "output buffer too small");
        }
        if (m > 0) {
            HIPCHK(hipMemcpyAsync(out, c->inc.fb.p, (size_t)m * sizeof(o3dr_point),
                                  mem == O3DR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    dev_release(c->inc.fb);  // (a fallback result is as large as the cloud: not kept)
    if (r != O3DR_OK) return r;
    *n_out = m;
    if (status) *status = s;
    return O3DR_OK;
}
// device words of the state's per-call workspace: [0] new groups, [1] cells, [2] kept cells
static int inc_read_word(o3dr_ctx* c, int w, uint32_t* v)
{
    HIPCHK(hipMemcpyAsync(c->n_host, (uint32_t*)c->inc.words.p + w, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(c->cc_host, c->cc_tmp, sizeof(CloudCounters), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->cc_host->status & O3DR_STATUS_INTERNAL)
        return fail(O3DR_ERR_INTERNAL, "a device-side guard of the incremental merge tripped (record or point id outside its range)");
    *v = c->n_host[0];
    return O3DR_OK;
}

static int inc_run(o3dr_ctx* c, o3dr_point* out, int64_t out_capacity, int64_t* n_out, uint32_t* status, int32_t mem, int64_t* st)
{
    auto& S = c->inc;
    float leaf[3], zo;
    uint32_t mp;
    downsample_leaf(c->params, 1, leaf, &mp, &zo);
    const uint32_t need = mp > 1u ? mp : 1u;
    const bool query = out == nullptr && out_capacity == 0;
    // 1. the cloud's size and status bits (and its running box, when the frame calls keep it) in one round trip
    const bool box_kept = c->cloud_box_valid;
    if (box_kept) HIPCHK(hipMemcpyAsync(c->misc_host, c->cloud_box, 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    CloudCounters cc;
    CHK(read_counters(c, c->cc_big, &cc));
    const int64_t n = (int64_t)cc.count;
    if (n >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "cloud_big exceeds 2^32-1 points");
    if (S.valid && (S.gen != c->cloud_gen || n < S.folded || leaf[0] != S.leaf[0] || leaf[1] != S.leaf[1] || leaf[2] != S.leaf[2] ||
                    zo != S.zo))
        inc_drop(c);
    if (c->params.dont_downsample) return inc_fallback(c, n, out, out_capacity, n_out, status, mem, st);
    st[1] = S.valid ? 0 : 1;
    if (!S.valid) {  // start from an empty state
        static const float empty[6] = {__builtin_inff(), __builtin_inff(), __builtin_inff(),
                                       -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        CHK(dev_ensure(c, S.box, 6 * sizeof(float)));
        HIPCHK(hipMemcpyAsync(S.box.p, empty, sizeof empty, hipMemcpyHostToDevice, c->stream));
        inc_drop(c);
        S.gen = c->cloud_gen;
        for (int a = 0; a < 3; ++a) S.leaf[a] = leaf[a];
        S.zo = zo;
        S.valid = true;
    }
    if (n == 0) return O3DR_OK;  // (like o3dr_finalize: no points, no status)
    CHK(zero_counters(c, c->cc_tmp));
    CHK(dev_ensure(c, S.words, 64));
    const int64_t tail = n - S.folded;
    if (tail > 0) {
        // 2. the combined box: the cloud's running box, or the state's extended by one pass over the tail
        CHK(ws_ensure(c, 1, tail, false));
        launch_set_counts(&c->prof, c->stream, c->ws.n_valid, (uint32_t)tail, 1);
        const o3dr_point* tp = c->cloud_big + S.folded;
        float hb[6];
        if (box_kept) {
            memcpy(hb, c->misc_host, sizeof hb);
            HIPCHK(hipMemcpyAsync(S.box.p, c->cloud_box, 6 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(c->ws.mm, c->cloud_box, 6 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        } else {
            const int used = launch_points_minmax(&c->prof, c->stream, tp, 0, c->ws.n_valid, 1, tail, c->ws.mm_stride, c->ws.mm);
            launch_bbox(&c->prof, c->stream, c->ws.mm, used, (float*)c->misc_dev);
            launch_inc_box_fold(c->stream, (float*)S.box.p, (const float*)c->misc_dev, c->ws.mm);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(c->misc_host, S.box.p, 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            memcpy(hb, c->misc_host, sizeof hb);
        }
        if (inc_geometry_check(hb, hb + 3, leaf, zo) != 0) return inc_fallback(c, n, out, out_capacity, n_out, status, mem, st);
        // 3. the tail's group runs sorted by group (heads as recorded while cloud_big grew, else from its points)
        launch_inc_runs(&c->prof, c->stream, c->ws, tp, tail, leaf, zo, heads_for_merge(c, leaf, zo), S.folded, c->test_corrupt);
        c->test_corrupt = 0;
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(S.words.p, c->ws.n_vox, sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        uint32_t nt = 0;
        CHK(inc_read_word(c, 0, &nt));
        if ((int64_t)nt > tail) return fail(O3DR_ERR_INTERNAL, "more groups than points in the tail");
        // 4. fold the tail's groups into the state's sums, merge the group lists, move the cells
        const int o = S.cur, q = 1 - o;
        const size_t nt1 = (size_t)nt + 1, np = ((size_t)S.n_groups + nt1) / 4096 + 64;
        CHK(dev_ensure(c, S.scratch, nt1 * kGroupCells * sizeof(IncCell)));
        CHK(dev_ensure(c, S.tg, nt1 * sizeof(IncGroup)));
        CHK(dev_ensure(c, S.tmatch, nt1 * sizeof(uint32_t)));
        CHK(dev_ensure(c, S.flag, nt1 * sizeof(uint32_t)));
        CHK(dev_ensure(c, S.partial, np * sizeof(uint32_t)));
        IncFoldArgs a;
        a.old_g = (const IncGroup*)S.grp[o].p;
        a.old_off = (const uint32_t*)S.off[o].p;
        a.old_cells = (const IncCell*)S.cells[o].p;
        a.n_old = S.n_groups;
        a.n_old_cells = S.n_cells;
        a.scratch = (IncCell*)S.scratch.p;
        a.tg = (IncGroup*)S.tg.p;
        a.tmatch = (uint32_t*)S.tmatch.p;
        a.nt = nt;
        a.flag = (uint32_t*)S.flag.p;
        a.n_new_only = (uint32_t*)S.words.p;
        a.cc = c->cc_tmp;
        launch_inc_fold(&c->prof, c->stream, c->ws, tp, zo, a, (uint32_t*)S.partial.p);
        HIPCHK(hipGetLastError());
        uint32_t new_only = 0;
        CHK(inc_read_word(c, 0, &new_only));
        if (new_only > nt) return fail(O3DR_ERR_INTERNAL, "more new groups than tail groups");
        const uint64_t n_new = (uint64_t)S.n_groups + new_only;
        if (n_new >= (1ull << 31)) return fail(O3DR_ERR_INTERNAL, "more than 2^31 groups");
        CHK(dev_ensure(c, S.grp[q], (size_t)(n_new + 1) * sizeof(IncGroup)));
        CHK(dev_ensure(c, S.off[q], (size_t)(n_new + 1) * sizeof(uint32_t)));
        CHK(dev_ensure(c, S.src, (size_t)(n_new + 1) * sizeof(uint32_t)));
        launch_inc_place(&c->prof, c->stream, a, (uint32_t)n_new, (IncGroup*)S.grp[q].p, (uint32_t*)S.src.p, (uint32_t*)S.off[q].p,
                         (uint32_t*)S.words.p + 1, (uint32_t*)S.partial.p);
        HIPCHK(hipGetLastError());
        uint32_t n_cells = 0;
        CHK(inc_read_word(c, 1, &n_cells));
        if ((uint64_t)n_cells > (uint64_t)S.n_cells + (uint64_t)tail || (uint64_t)n_cells > n_new * kGroupCells)
            return fail(O3DR_ERR_INTERNAL, "cell count of the merged state out of range");
        CHK(dev_ensure(c, S.cells[q], ((size_t)n_cells + 1) * sizeof(IncCell)));
        launch_inc_copy(&c->prof, c->stream, a, (const IncGroup*)S.grp[q].p, (const uint32_t*)S.off[q].p, (const uint32_t*)S.src.p,
                        (uint32_t)n_new, (IncCell*)S.cells[q].p, n_cells);
        HIPCHK(hipGetLastError());
        S.cur = q;
        S.n_groups = (uint32_t)n_new;
        S.n_cells = n_cells;
        S.folded = n;
        st[0] = tail;
    }
    // 5. the snapshot: cells with at least max(min_points_per_voxel, 1) points, in cell order
    const IncGroup* grp = (const IncGroup*)S.grp[S.cur].p;
    const uint32_t* off = (const uint32_t*)S.off[S.cur].p;
    const IncCell* cells = (const IncCell*)S.cells[S.cur].p;
    uint32_t m = S.n_cells;
    const uint32_t* out_off = off;
    if (need > 1u) {
        CHK(dev_ensure(c, S.keep, ((size_t)S.n_groups + 1) * sizeof(uint32_t)));
        CHK(dev_ensure(c, S.partial, (((size_t)S.n_groups + 1) / 4096 + 64) * sizeof(uint32_t)));
        launch_inc_keep(&c->prof, c->stream, grp, off, cells, S.n_groups, S.n_cells, need, (uint32_t*)S.keep.p, (uint32_t*)S.words.p + 2,
                        (uint32_t*)S.partial.p);
        HIPCHK(hipGetLastError());
        CHK(inc_read_word(c, 2, &m));
        if (m > S.n_cells) return fail(O3DR_ERR_INTERNAL, "more kept cells than cells");
        out_off = (const uint32_t*)S.keep.p;
    }
    if (!query && (int64_t)m > out_capacity) return fail(O3DR_ERR_CAPACITY, "output buffer too small");
    o3dr_point* dst = out;
    if (!query && mem == O3DR_MEM_HOST && m > 0) {
        CHK(dev_ensure(c, c->st_out, (size_t)m * sizeof(o3dr_point)));
        dst = (o3dr_point*)c->st_out.p;
    }
    if (!query && m > 0) {
        launch_inc_snapshot(&c->prof, c->stream, grp, off, cells, S.n_groups, S.n_cells, need, out_off, zo, dst, m, c->cc_tmp);
        HIPCHK(hipGetLastError());
        if (mem == O3DR_MEM_HOST)
            HIPCHK(hipMemcpyAsync(out, dst, (size_t)m * sizeof(o3dr_point), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipMemcpyAsync(c->cc_host, c->cc_tmp, sizeof(CloudCounters), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->cc_host->status & O3DR_STATUS_INTERNAL)
        return fail(O3DR_ERR_INTERNAL, "a device-side guard of the incremental merge tripped (record or point id outside its range)");
    *n_out = (int64_t)m;
    if (status) *status = cc.status;
    return O3DR_OK;
}

extern "C" int o3dr_finalize_incremental(o3dr_ctx* c, o3dr_point* out, int64_t out_capacity, int64_t* n_out, uint32_t* status,
                                         int32_t mem)
{
    if (n_out) *n_out = 0;
    if (status) *status = 0;
    CTX_ENTER(c);
    if (!n_out) return fail(O3DR_ERR_INVALID_ARG, "n_out is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (out_capacity < 0 || (out_capacity > 0 && !out)) return fail(O3DR_ERR_INVALID_ARG, "out is NULL with a capacity, or a negative capacity");
    int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int r = inc_run(c, out, out_capacity, n_out, status, mem, st);
    if (r != O3DR_OK) {  // never half-folded: the next call rebuilds
        inc_drop(c);
        *n_out = 0;
        if (status) *status = 0;
    }
    st[3] = c->inc.n_cells;
    st[4] = c->inc.n_groups;
    st[5] = inc_state_bytes(c);
    memcpy(c->inc.stats, st, sizeof st);
    return r;
}

extern "C" int o3dr_finalize_incremental_stats(o3dr_ctx* c, int64_t out[8])
{
    CTX_ENTER(c);
    if (!out) return fail(O3DR_ERR_INVALID_ARG, "out is NULL");
    memcpy(out, c->inc.stats, sizeof c->inc.stats);
    return O3DR_OK;
}

// ---- multi-GPU merge: global box -> index-slice partition -> exchange -> local merge ----
extern "C" int o3dr_finalize_global(o3dr_ctx* c, const float gmin[3], const float gmax[3], o3dr_point* out,
                                    int64_t out_capacity, int64_t* n_out, uint32_t* status, int32_t mem)
{
    if (!gmin || !gmax) {
        if (n_out) *n_out = 0;
        return fail(O3DR_ERR_INVALID_ARG, "bounding box is NULL");
    }
    return finalize_impl(c, gmin, gmax, out, out_capacity, n_out, status, mem);
}

// Zero-copy access for the exchange: the HBM address of cloud_big (valid until the next call that
// appends, partitions or adopts), a receive buffer of the requested size, and "make what I received
// the new cloud_big".
extern "C" int o3dr_cloud_big_view(o3dr_ctx* c, void** ptr, int64_t* n)
{
    CTX_ENTER(c);
    if (!ptr || !n) return fail(O3DR_ERR_INVALID_ARG, "ptr / n is NULL");
    if (!c->cloud_n_exact) {  // (no round trip when the host already knows the size: reads, resets, adopt, assume_size)
        CloudCounters cc;
        CHK(read_counters(c, c->cc_big, &cc));
    }
    *ptr = c->cloud_big;
    *n = c->cloud_ub;
    return O3DR_OK;
}
// The caller learnt cloud_big's exact size by other means (its own header from o3dr_cloud_big_header_dev, read back
// with the all-to-all's sizes): later calls then need no round trip for it.  A wrong value is caught by the merge
// (O3DR_ERR_INTERNAL), never used to address memory beyond the cloud's capacity.
extern "C" int o3dr_cloud_big_assume_size(o3dr_ctx* c, int64_t n_points)
{
    CTX_ENTER(c);
    if (n_points < 0 || n_points > c->cloud_ub) return fail(O3DR_ERR_INVALID_ARG, "size above what the calls so far can have produced");
    if (n_points < c->inc.folded) ++c->cloud_gen;
    c->cloud_ub = n_points;
    c->cloud_n_exact = true;
    return O3DR_OK;
}
extern "C" int o3dr_cloud_big_recv_buffer(o3dr_ctx* c, int64_t n_points, void** ptr)
{
    CTX_ENTER(c);
    if (!ptr || n_points < 0) return fail(O3DR_ERR_INVALID_ARG, "bad arguments");
    CHK(alt_reserve(c, n_points > 0 ? n_points : 1));
    *ptr = c->cloud_alt;
    return O3DR_OK;
}
extern "C" int o3dr_cloud_big_adopt(o3dr_ctx* c, int64_t n_points)
{
    CTX_ENTER(c);
    if (n_points < 0 || n_points > c->cloud_alt_cap) return fail(O3DR_ERR_INVALID_ARG, "more points than the receive buffer holds");
    if (n_points >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "cloud_big exceeds 2^32-1 points");
    // stream-ordered, no host round trip: the count is set by a one-thread kernel (the status bits accumulated so far
    // are kept); what filled the receive buffer must be ordered before this stream's next work by the caller
    ++c->cloud_gen;
    launch_set_cloud_count(c->stream, c->cc_big, (uint64_t)n_points);
    HIPCHK(hipGetLastError());
    swap_clouds(c);
    c->cloud_box_valid = false;
    c->cloud_heads_valid = false;
    c->cloud_ub = n_points;
    c->cloud_n_exact = true;
    return O3DR_OK;
}

// ---- the exchange's small data on the device: header (box + count) and slice counts without a host round trip ----------
extern "C" int o3dr_cloud_big_header_dev(o3dr_ctx* c, void* hdr_dev)
{
    CTX_ENTER(c);
    if (!hdr_dev) return fail(O3DR_ERR_INVALID_ARG, "hdr_dev is NULL");
    const float* box = c->cloud_box;
    if (!c->cloud_box_valid) {
        float* tmp = (float*)c->misc_dev;
        if (c->cloud_ub == 0 || !c->cloud_big) {
            static const float empty[6] = {__builtin_inff(), __builtin_inff(), __builtin_inff(),
                                           -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
            HIPCHK(hipMemcpyAsync(tmp, empty, sizeof empty, hipMemcpyHostToDevice, c->stream));
        } else {  // appends / transforms / exchanges dropped the running box: one pass over the cloud, sized by the bound
            if (c->cloud_ub >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "cloud_big exceeds 2^32-1 points");
            CHK(ws_ensure(c, 1, c->cloud_ub, false));
            launch_count_from_cc(c->stream, c->cc_big, c->ws.n_valid);
            const int used = launch_points_minmax(&c->prof, c->stream, c->cloud_big, 0, c->ws.n_valid, 1, c->cloud_ub, c->ws.mm_stride, c->ws.mm);
            launch_bbox(&c->prof, c->stream, c->ws.mm, used, tmp);
        }
        box = tmp;
    }
    launch_pack_header(c->stream, box, c->cc_big, hdr_dev);
    HIPCHK(hipGetLastError());
    return O3DR_OK;
}

// the merge's grid over cloud_big (at most ub points, counted in ws.n_valid): its index slices are what the partitions cut
static VoxelArgs slice_args(o3dr_ctx* c, int64_t ub)
{
    float leaf[3], zo;
    uint32_t mp;
    downsample_leaf(c->params, 1, leaf, &mp, &zo);
    return voxel_args(c->cloud_big, 0, c->ws.n_valid, 1, ub, leaf, zo);
}

extern "C" int o3dr_cloud_big_partition_dev(o3dr_ctx* c, const void* hdrs_dev, int32_t n_hdrs, int32_t n_parts, int64_t* counts_dev)
{
    CTX_ENTER(c);
    if (!hdrs_dev || !counts_dev || n_hdrs < 1 || n_parts < 1 || n_parts > kMaxRadix)
        return fail(O3DR_ERR_INVALID_ARG, "bad arguments (1 <= n_parts <= 128)");
    HIPCHK(hipMemsetAsync(counts_dev, 0, sizeof(int64_t) * ((size_t)n_parts + 1), c->stream));
    const int64_t ub = c->cloud_ub;  // kernels take the count from the device; the bound sizes grids and buffers
    if (ub == 0 || !c->cloud_big) return O3DR_OK;
    if (ub >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "cloud_big exceeds 2^32-1 points");
    CHK(ws_ensure(c, 1, ub, false));
    CHK(alt_reserve(c, ub));
    o3dr_point* nb = c->cloud_alt;
    launch_count_from_cc(c->stream, c->cc_big, c->ws.n_valid);
    const VoxelArgs v = slice_args(c, ub);
    ++c->cloud_gen;
    launch_partition(&c->prof, c->stream, c->ws, v, n_parts, nb, (uint64_t*)counts_dev, (uint32_t*)(counts_dev + n_parts), hdrs_dev, n_hdrs);
    if (hipGetLastError() != hipSuccess) return fail(O3DR_ERR_HIP, "partition launch failed");
    swap_clouds(c);  // the partitioned copy becomes cloud_big; the old buffer is kept as the alternate
    c->cloud_heads_valid = false;
    return O3DR_OK;
}

// ---- the partition in two halves: slice sizes first (nothing moves), then ONE pass that places the slices where the
// exchange wants them - [room for what the lower ranks send | this rank's own slice | room for the higher ranks' | the
// slices that leave, in rank order] - so that the all-to-all receives straight into the gaps and the own slice (95 % of the
// cloud at the benchmark shapes) is never sent to itself
extern "C" int o3dr_cloud_big_slice_counts_dev(o3dr_ctx* c, const void* hdrs_dev, int32_t n_hdrs, int32_t n_parts, int64_t* counts_dev)
{
    CTX_ENTER(c);
    if (!hdrs_dev || !counts_dev || n_hdrs < 1 || n_parts < 1 || n_parts > kMaxRadix)
        return fail(O3DR_ERR_INVALID_ARG, "bad arguments (1 <= n_parts <= 128)");
    c->place_ub = -1;
    HIPCHK(hipMemsetAsync(counts_dev, 0, sizeof(int64_t) * ((size_t)n_parts + 1), c->stream));
    const int64_t ub = c->cloud_ub;  // kernels take the count from the device; the bound sizes grids and buffers
    if (ub == 0 || !c->cloud_big) {
        c->place_ub = 0;
        c->place_parts = n_parts;
        return O3DR_OK;
    }
    if (ub >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "cloud_big exceeds 2^32-1 points");
    CHK(ws_ensure(c, 1, ub, false));
    launch_count_from_cc(c->stream, c->cc_big, c->ws.n_valid);
    const VoxelArgs v = slice_args(c, ub);
    launch_partition_count(&c->prof, c->stream, c->ws, v, n_parts, (uint64_t*)counts_dev, (uint32_t*)(counts_dev + n_parts), hdrs_dev, n_hdrs);
    if (hipGetLastError() != hipSuccess) return fail(O3DR_ERR_HIP, "slice count launch failed");
    c->place_ub = ub;
    c->place_parts = n_parts;
    return O3DR_OK;
}

extern "C" int o3dr_cloud_big_place_slices(o3dr_ctx* c, int32_t n_parts, int32_t own_part, const int64_t* counts, int64_t n_before,
                                           int64_t n_after, int64_t* send_offset)
{
    CTX_ENTER(c);
    if (!counts || n_parts < 1 || n_parts > kMaxRadix || own_part < 0 || own_part >= n_parts || n_before < 0 || n_after < 0)
        return fail(O3DR_ERR_INVALID_ARG, "bad arguments");
    if (c->place_ub < 0 || c->place_parts != n_parts) return fail(O3DR_ERR_INVALID_ARG, "o3dr_cloud_big_slice_counts_dev must run first, for the same slices");
    int64_t n_local = 0;
    for (int p = 0; p < n_parts; ++p) {
        if (counts[p] < 0) return fail(O3DR_ERR_INVALID_ARG, "negative slice size");
        n_local += counts[p];
    }
    if (n_local > c->place_ub) return fail(O3DR_ERR_INVALID_ARG, "slice sizes above the cloud's size");
    const int64_t own = counts[own_part], send_start = n_before + own + n_after, total = send_start + (n_local - own);
    if (send_offset) *send_offset = send_start;
    const int64_t cap_counted = c->place_ub;  // the (slice, tile) table is laid out for this many points: the move must use the same tiling
    c->place_ub = -1;                         // (the table is consumed)
    if (n_before == 0 && n_after == 0 && own == n_local) return O3DR_OK;  // nothing leaves, nothing arrives: the cloud stays as it is
    if (total >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "the exchange buffer exceeds 2^32-1 points");
    ++c->cloud_gen;
    CHK(alt_reserve(c, total > 0 ? total : 1));
    // part p's records start at sum(counts[0..p)) in the plain layout; where they go instead
    int64_t* sh = (int64_t*)(c->misc_host + 2560);
    int64_t nat = 0, out_off = send_start;
    for (int p = 0; p < n_parts; ++p) {
        if (p == own_part) {
            sh[p] = n_before - nat;
        } else {
            sh[p] = out_off - nat;
            out_off += counts[p];
        }
        nat += counts[p];
    }
    HIPCHK(hipMemcpyAsync(c->misc_dev + 2560, sh, sizeof(int64_t) * (size_t)n_parts, hipMemcpyHostToDevice, c->stream));
    if (n_local > 0) {
        const VoxelArgs v = slice_args(c, cap_counted);
        launch_partition_move(&c->prof, c->stream, c->ws, v, n_parts, c->cloud_alt, (const int64_t*)(c->misc_dev + 2560));
        if (hipGetLastError() != hipSuccess) return fail(O3DR_ERR_HIP, "slice placement launch failed");
        // (the pinned shift table is only written here, and every exchange ends in a stream wait - the merged slice's size -
        // before the next one can begin)
    }
    swap_clouds(c);  // the laid-out copy becomes cloud_big (its device count is stale until o3dr_cloud_big_set_size)
    c->cloud_box_valid = false;
    c->cloud_heads_valid = false;
    c->cloud_ub = total;
    c->cloud_n_exact = false;
    return O3DR_OK;
}

extern "C" int o3dr_cloud_big_set_size(o3dr_ctx* c, int64_t n_points)
{
    CTX_ENTER(c);
    if (n_points < 0 || n_points > c->cloud_cap) return fail(O3DR_ERR_INVALID_ARG, "more points than the cloud buffer holds");
    if (n_points >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "cloud_big exceeds 2^32-1 points");
    ++c->cloud_gen;
    launch_set_cloud_count(c->stream, c->cc_big, (uint64_t)n_points);  // stream-ordered, like o3dr_cloud_big_adopt
    HIPCHK(hipGetLastError());
    c->cloud_box_valid = false;
    c->cloud_heads_valid = false;
    c->cloud_ub = n_points;
    c->cloud_n_exact = true;
    return O3DR_OK;
}

extern "C" int o3dr_cloud_big_raw_view(o3dr_ctx* c, void** ptr, int64_t* capacity_points)
{
    CTX_ENTER(c);
    if (!ptr || !capacity_points) return fail(O3DR_ERR_INVALID_ARG, "ptr / capacity is NULL");
    *ptr = c->cloud_big;
    *capacity_points = c->cloud_cap;
    return O3DR_OK;
}

extern "C" int o3dr_cloud_big_bbox(o3dr_ctx* c, float mn[3], float mx[3], int64_t* n_out)
{
    CTX_ENTER(c);
    if (!mn || !mx) return fail(O3DR_ERR_INVALID_ARG, "bounding box is NULL");
    CloudCounters cc;
    CHK(read_counters(c, c->cc_big, &cc));
    const int64_t n = (int64_t)cc.count;
    c->cloud_ub = n;
    if (n_out) *n_out = n;
    for (int a = 0; a < 3; ++a) mn[a] = __builtin_inff(), mx[a] = -__builtin_inff();
    if (n == 0) return O3DR_OK;
    if (n >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "cloud_big exceeds 2^32-1 points");
    if (c->cloud_box_valid) {
        HIPCHK(hipMemcpyAsync(c->misc_host, c->cloud_box, 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    } else {
        CHK(ws_ensure(c, 1, n, false));
        launch_set_counts(&c->prof, c->stream, c->ws.n_valid, (uint32_t)n, 1);
        const int used = launch_points_minmax(&c->prof, c->stream, c->cloud_big, 0, c->ws.n_valid, 1, n, c->ws.mm_stride, c->ws.mm);
        launch_bbox(&c->prof, c->stream, c->ws.mm, used, (float*)c->misc_dev);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c->misc_host, c->misc_dev, 6 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    const float* h = (const float*)c->misc_host;
    for (int a = 0; a < 3; ++a) mn[a] = h[a], mx[a] = h[3 + a];
    return O3DR_OK;
}

extern "C" int o3dr_cloud_big_partition(o3dr_ctx* c, const float gmin[3], const float gmax[3], int32_t n_parts,
                                        int64_t* counts, uint32_t* status)
{
    if (status) *status = 0;
    CTX_ENTER(c);
    if (!gmin || !gmax || !counts || n_parts < 1 || n_parts > kMaxRadix)
        return fail(O3DR_ERR_INVALID_ARG, "bad arguments (1 <= n_parts <= 128)");
    for (int p = 0; p < n_parts; ++p) counts[p] = 0;
    CloudCounters cc;
    CHK(read_counters(c, c->cc_big, &cc));
    const int64_t n = (int64_t)cc.count;
    c->cloud_ub = n;
    if (n == 0) return O3DR_OK;
    if (n >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "cloud_big exceeds 2^32-1 points");
    CHK(ws_ensure(c, 1, n, false));
    CHK(alt_reserve(c, n));
    o3dr_point* nb = c->cloud_alt;
    launch_set_counts(&c->prof, c->stream, c->ws.n_valid, (uint32_t)n, 1);
    CHK(put_bbox(c, gmin, gmax));
    const VoxelArgs v = slice_args(c, n);
    uint32_t* ovf_dev = (uint32_t*)(c->misc_dev + 32);
    uint64_t* cnt_dev = (uint64_t*)(c->misc_dev + 64);
    ++c->cloud_gen;
    launch_partition(&c->prof, c->stream, c->ws, v, n_parts, nb, cnt_dev, ovf_dev);
    if (hipGetLastError() != hipSuccess) return fail(O3DR_ERR_HIP, "partition launch failed");
    HIPCHK(hipMemcpyAsync(c->misc_host, c->misc_dev, 64 + 8 * (size_t)n_parts, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    swap_clouds(c);  // the partitioned copy becomes cloud_big; the old buffer is kept as the alternate
    c->cloud_heads_valid = false;
    const uint32_t ovf = *(const uint32_t*)(c->misc_host + 32);
    const uint64_t* hc = (const uint64_t*)(c->misc_host + 64);
    for (int p = 0; p < n_parts; ++p) counts[p] = (int64_t)hc[p];
    if (status) *status = ovf ? O3DR_STATUS_VOXEL_OVERFLOW : 0u;
    return O3DR_OK;
}

// -------------------------------------------------------------------------------------------------
// The whole multi-GPU exchange behind one entry point, for C++ hosts that own RCCL communicators (one host thread and
// one context per GPU; the reference's merge sits in its C++ main flow, pose.cpp:527-532).  RCCL is resolved with
// dlopen/dlsym at first use: libo3dr.so itself carries no dependency on it.
// -------------------------------------------------------------------------------------------------
struct RcclApi {
    void* handle = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
    bool ok = false;
};
static RcclApi* rccl_api()
{
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, []() {
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            api.handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (api.handle) break;
        }
        if (!api.handle) return;
        bool all = true;
        auto sym = [&](const char* n) {
            void* p = dlsym(api.handle, n);
            all = all && p != nullptr;
            return p;
        };
        api.AllGather = (decltype(api.AllGather))sym("ncclAllGather");
        api.Send = (decltype(api.Send))sym("ncclSend");
        api.Recv = (decltype(api.Recv))sym("ncclRecv");
        api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
        api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
        api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
        api.CommInitAll = (decltype(api.CommInitAll))sym("ncclCommInitAll");
        api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
        api.CommCount = (decltype(api.CommCount))sym("ncclCommCount");
        api.CommUserRank = (decltype(api.CommUserRank))sym("ncclCommUserRank");
        api.ok = all;
    });
    return api.ok ? &api : nullptr;
}
#define NCCLCHK(R, expr)                                                                              \
    do {                                                                                              \
        ncclResult_t r_ = (expr);                                                                     \
        if (r_ != ncclSuccess) {                                                                      \
            char buf_[512];                                                                           \
            snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, (R)->GetErrorString(r_), __FILE__, __LINE__); \
            g_err = buf_;                                                                             \
            return O3DR_ERR_HIP;                                                                      \
        }                                                                                             \
    } while (0)

extern "C" int o3dr_comm_init_all(int32_t n_devices, const int32_t* devices, void** comms_out)
{
    if (n_devices < 1 || n_devices > kMaxRadix || !comms_out) return fail(O3DR_ERR_INVALID_ARG, "bad arguments (1 <= n_devices <= 128)");
    RcclApi* R = rccl_api();
    if (!R) return fail(O3DR_ERR_HIP, "RCCL (librccl.so.1) could not be loaded");
    std::vector<int> devs((size_t)n_devices);
    for (int i = 0; i < n_devices; ++i) devs[(size_t)i] = devices ? devices[i] : i;
    std::vector<ncclComm_t> comms((size_t)n_devices);
    NCCLCHK(R, R->CommInitAll(comms.data(), n_devices, devs.data()));
    for (int i = 0; i < n_devices; ++i) comms_out[i] = comms[(size_t)i];
    return O3DR_OK;
}
extern "C" int o3dr_comm_destroy(void* comm)
{
    if (!comm) return O3DR_OK;
    RcclApi* R = rccl_api();
    if (!R) return fail(O3DR_ERR_HIP, "RCCL (librccl.so.1) could not be loaded");
    NCCLCHK(R, R->CommDestroy((ncclComm_t)comm));
    return O3DR_OK;
}

// ---- transports of the exchange -----------------------------------------------------------------------------------------
// The protocol below only needs "all-gather a few bytes" and "move my slice segments to their owners"; RCCL provides
// both for real ranks.  The LOCAL transport (include/o3dr_testing.h) connects W contexts of ONE process - one host thread
// each, all on the same device - through device-to-device copies and a host barrier, so that the very code that runs over
// RCCL (sizes, slices, failure agreement, statistics) is exercised with W > 1 on a one-GPU box, where RCCL refuses two
// ranks on one device.
struct Transport {
    int W = 1, rank = 0;
    virtual ~Transport() {}
    // every rank contributes `bytes` at send_dev; recv_dev receives W * bytes in rank order (ordered on c->stream)
    virtual int all_gather(o3dr_ctx* c, const void* send_dev, void* recv_dev, size_t bytes) = 0;
    // send[p] points at base + send_off[p] go to rank p; recv[p] points from rank p land at base + recv_off[p] (same buffer,
    // disjoint regions).  Nothing is sent to the rank itself: its own slice is already where it belongs.
    virtual int all_to_all(o3dr_ctx* c, o3dr_point* base, const int64_t* send_off, const int64_t* send, const int64_t* recv_off,
                           const int64_t* recv) = 0;
};

struct RcclTransport : Transport {
    RcclApi* R = nullptr;
    ncclComm_t comm = nullptr;
    int all_gather(o3dr_ctx* c, const void* send_dev, void* recv_dev, size_t bytes) override
    {
        NCCLCHK(R, R->AllGather(send_dev, recv_dev, bytes, ncclUint8, comm, c->stream));
        return O3DR_OK;
    }
    int all_to_all(o3dr_ctx* c, o3dr_point* base, const int64_t* send_off, const int64_t* send, const int64_t* recv_off,
                   const int64_t* recv) override
    {
        // every peer pair has its own xGMI link.  An error inside the group must not leave it open: ncclGroupEnd is
        // always reached, the first error is reported after it.
        NCCLCHK(R, R->GroupStart());
        ncclResult_t first = ncclSuccess;
        for (int p = 0; p < W; ++p) {
            if (p == rank) continue;
            if (send[p] && first == ncclSuccess) first = R->Send(base + send_off[p], (size_t)send[p] * sizeof(o3dr_point), ncclUint8, p, comm, c->stream);
            if (recv[p] && first == ncclSuccess) first = R->Recv(base + recv_off[p], (size_t)recv[p] * sizeof(o3dr_point), ncclUint8, p, comm, c->stream);
        }
        const ncclResult_t endr = R->GroupEnd();
        NCCLCHK(R, first);
        NCCLCHK(R, endr);
        return O3DR_OK;
    }
};

struct LocalComm {  // test transport: shared by the W rank threads
    int W = 1;
    std::mutex m;
    std::condition_variable cv;
    int waiting = 0;
    uint64_t generation = 0;
    bool broken = false;
    std::vector<const void*> ptr;
    std::vector<const int64_t*> cnt, off;
    // false: a rank did not show up within 30 s (it left the protocol: exactly what the tests look for)
    bool barrier()
    {
        std::unique_lock<std::mutex> lk(m);
        if (broken) return false;
        const uint64_t g = generation;
        if (++waiting == W) {
            waiting = 0;
            ++generation;
            cv.notify_all();
            return true;
        }
        if (!cv.wait_for(lk, std::chrono::seconds(30), [&] { return generation != g || broken; })) {
            broken = true;
            cv.notify_all();
            return false;
        }
        return !broken;
    }
};
struct LocalTransport : Transport {
    LocalComm* L = nullptr;
    int all_gather(o3dr_ctx* c, const void* send_dev, void* recv_dev, size_t bytes) override
    {
        HIPCHK(hipStreamSynchronize(c->stream));
        L->ptr[(size_t)rank] = send_dev;
        if (!L->barrier()) return fail(O3DR_ERR_PEER, "local transport: a rank left the exchange (all-gather)");
        for (int r = 0; r < W; ++r)
            HIPCHK(hipMemcpyAsync((char*)recv_dev + (size_t)r * bytes, L->ptr[(size_t)r], bytes, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (!L->barrier()) return fail(O3DR_ERR_PEER, "local transport: a rank left the exchange (all-gather)");
        return O3DR_OK;
    }
    int all_to_all(o3dr_ctx* c, o3dr_point* base, const int64_t* send_off, const int64_t* send, const int64_t* recv_off,
                   const int64_t* recv) override
    {
        HIPCHK(hipStreamSynchronize(c->stream));
        L->ptr[(size_t)rank] = base;
        L->cnt[(size_t)rank] = send;
        L->off[(size_t)rank] = send_off;
        if (!L->barrier()) return fail(O3DR_ERR_PEER, "local transport: a rank left the exchange (all-to-all)");
        int rc = O3DR_OK;
        for (int p = 0; p < W && rc == O3DR_OK; ++p) {
            if (p == rank) continue;
            if (L->cnt[(size_t)p][rank] != recv[p]) rc = fail(O3DR_ERR_INTERNAL, "local transport: send and receive counts differ");
            else if (recv[p] && hipMemcpyAsync(base + recv_off[p], (const o3dr_point*)L->ptr[(size_t)p] + L->off[(size_t)p][rank],
                                               (size_t)recv[p] * sizeof(o3dr_point), hipMemcpyDeviceToDevice, c->stream) != hipSuccess)
                rc = fail(O3DR_ERR_HIP, "local transport: copy failed");
        }
        if (hipStreamSynchronize(c->stream) != hipSuccess && rc == O3DR_OK) rc = fail(O3DR_ERR_HIP, "local transport: sync failed");
        if (!L->barrier()) return fail(O3DR_ERR_PEER, "local transport: a rank left the exchange (all-to-all)");
        return rc;
    }
};

// What one rank tells the others with the slice counts (all-gather #2): W counts, then
//   [W]     status word of the partition (bit 0: PCL's overflow guard on the global box)
//   [W + 1] this rank's error so far (0, or a negative O3DR_ERR_* code: every rank then leaves the exchange together)
//   [W + 2] points its receive buffer (the alternate cloud) holds now
//   [W + 3] points its merged-slice buffer holds now
//   [W + 4] points its gather buffer holds now
// With the capacities every rank knows whether ANY rank has to grow a buffer before the all-to-all.  If none has to
// (every call after the first of a run), nothing can fail locally between the count matrix and the merge, and the
// exchange goes on without another word; else the ranks that must allocate do so and one more 8-byte all-gather
// carries the outcome, so that a failed allocation stops every rank before the all-to-all instead of leaving the
// others inside it.
static constexpr int kRowExtra = 5;

static int peer_error(int own, int first_rank, int64_t first_code, const std::string& own_msg)
{
    char buf[256];
    if (own != O3DR_OK) {
        snprintf(buf, sizeof buf, "%s [every rank left the exchange]", own_msg.c_str());
        g_err = buf;
        return own;
    }
    snprintf(buf, sizeof buf, "rank %d failed with code %lld: every rank left the exchange together", first_rank, (long long)first_code);
    g_err = buf;
    return O3DR_ERR_PEER;
}

static int merge_partitioned_impl(o3dr_ctx* c, Transport& T, int32_t gather_result, o3dr_point* out, int64_t out_capacity,
                                  int64_t* n_out, int64_t* n_total, uint32_t* status, int32_t mem)
{
    const int W = T.W, rank = T.rank;
    if (W < 1 || W > kMaxRadix || rank < 0 || rank >= W) return fail(O3DR_ERR_INVALID_ARG, "communicators of 1..128 ranks are supported");
    ++c->cloud_gen;  // (the exchange reorders and replaces cloud_big)
    const size_t RW = (size_t)W + kRowExtra;
    // device scratch: own header | all headers | own row | row matrix (read back in one copy from o_hdrs on).  The one
    // allocation in front of the first collective (a few KiB); everything after it is decided by all ranks together.
    const size_t o_hdr = 0, o_hdrs = 32, o_row = o_hdrs + 32 * (size_t)W, o_mat = o_row + 8 * RW;
    const size_t total_bytes = o_mat + 8 * (size_t)W * RW;
    CHK(dev_ensure(c, c->st_xchg, total_bytes));
    if (c->xchg_host_cap < total_bytes) {
        if (c->xchg_host) (void)hipHostFree(c->xchg_host);
        c->xchg_host = nullptr;
        c->xchg_host_cap = 0;
        if (hipHostMalloc((void**)&c->xchg_host, total_bytes, hipHostMallocDefault) != hipSuccess) return fail(O3DR_ERR_ALLOC, "hipHostMalloc failed");
        c->xchg_host_cap = total_bytes;
    }
    memset(c->xchg_stats, 0, sizeof c->xchg_stats);
    char* d = (char*)c->st_xchg.p;
    struct Hdr {
        float mn[3], mx[3];
        int64_t count;  // negative: this rank's O3DR_ERR_* code
    };
    int local = O3DR_OK;  // this rank's first failure; it keeps taking part in the collectives that remain
    std::string local_msg;
    auto note = [&](int rc) {
        if (rc != O3DR_OK && local == O3DR_OK) {
            local = rc;
            local_msg = g_err;
        }
    };
    auto injected = [&](int point) {  // o3dr_test_fail_at
        if (c->test_fail_at != point) return false;
        c->test_fail_at = 0;
        (void)fail(O3DR_ERR_ALLOC, "failure injected by o3dr_test_fail_at");
        return true;
    };
    // 1. headers
    note(injected(1) ? O3DR_ERR_ALLOC : o3dr_cloud_big_header_dev(c, d + o_hdr));
    if (local != O3DR_OK) {
        Hdr* eh = (Hdr*)c->xchg_host;
        for (int a = 0; a < 3; ++a) eh->mn[a] = __builtin_inff(), eh->mx[a] = -__builtin_inff();
        eh->count = (int64_t)local;
        HIPCHK(hipMemcpyAsync(d + o_hdr, eh, 32, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));  // (the pinned word is reused below)
    }
    CHK(T.all_gather(c, d + o_hdr, d + o_hdrs, 32));
    // 2. slice sizes over the box the headers span (nothing moves yet: the slices are placed once the counts are known)
    if (local == O3DR_OK) note(injected(2) ? O3DR_ERR_ALLOC : o3dr_cloud_big_slice_counts_dev(c, d + o_hdrs, W, W, (int64_t*)(d + o_row)));
    if (local != O3DR_OK) HIPCHK(hipMemsetAsync(d + o_row, 0, 8 * ((size_t)W + 1), c->stream));
    int64_t* extra = (int64_t*)c->xchg_host;
    extra[0] = (int64_t)local;
    extra[1] = c->cloud_alt_cap;
    extra[2] = (int64_t)(c->st_merge.cap / sizeof(o3dr_point));
    extra[3] = (int64_t)(c->st_gather.cap / sizeof(o3dr_point));
    HIPCHK(hipMemcpyAsync(d + o_row + 8 * ((size_t)W + 1), extra, 8 * (kRowExtra - 1), hipMemcpyHostToDevice, c->stream));
    // 3. row matrix and the ONE read-back
    CHK(T.all_gather(c, d + o_row, d + o_mat, 8 * RW));
    HIPCHK(hipMemcpyAsync(c->xchg_host + o_hdrs, d + o_hdrs, total_bytes - o_hdrs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const Hdr* hdrs = (const Hdr*)(c->xchg_host + o_hdrs);
    const int64_t* mat = (const int64_t*)(c->xchg_host + o_mat);
    for (int r = 0; r < W; ++r) {  // a failure anywhere so far: every rank sees it here and leaves before the all-to-all
        const int64_t code = hdrs[r].count < 0 ? hdrs[r].count : mat[(size_t)r * RW + W + 1];
        if (code < 0) return peer_error(local, r, code, local_msg);
    }
    float gmin[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, gmax[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    int64_t total_pts = 0;
    for (int r = 0; r < W; ++r) {
        if (hdrs[r].count <= 0) continue;
        total_pts += hdrs[r].count;
        for (int a = 0; a < 3; ++a) {
            gmin[a] = std::min(gmin[a], hdrs[r].mn[a]);
            gmax[a] = std::max(gmax[a], hdrs[r].mx[a]);
        }
    }
    if (n_total) *n_total = total_pts;
    const int64_t n_local = hdrs[rank].count;
    bool overflow = false;
    for (int r = 0; r < W; ++r) overflow = overflow || ((mat[(size_t)r * RW + W] & 1) != 0);  // (same global box everywhere: all agree)
    // what every rank sends, receives and merges (the same arithmetic on the same matrix everywhere)
    auto sends = [&](int from, int to) { return overflow ? (from == to ? hdrs[from].count : (int64_t)0) : mat[(size_t)from * RW + to]; };
    std::vector<int64_t> send((size_t)W, 0), recv((size_t)W, 0), slice_in((size_t)W, 0);
    for (int p = 0; p < W; ++p) {
        send[(size_t)p] = sends(rank, p);
        recv[(size_t)p] = sends(p, rank);
        for (int r = 0; r < W; ++r) slice_in[(size_t)p] += sends(r, p);
    }
    int64_t n_recv = 0, max_slice = 0;
    for (int p = 0; p < W; ++p) n_recv += recv[(size_t)p], max_slice = std::max(max_slice, slice_in[(size_t)p]);
    if (total_pts == 0) return O3DR_OK;
    if (max_slice >= (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "a slice exceeds 2^32-1 points");  // (every rank: same matrix)
    // an upper bound of any rank's merged slice, for the gather buffer: no more cells than points in the slice, and a
    // slice covers at most ~cells / W linear indices of the combined grid over the global box (part_of: multiply-shift)
    int64_t pad_bound = max_slice;
    if (!overflow) {
        float leaf[3], zo;
        uint32_t mp;
        downsample_leaf(c->params, 1, leaf, &mp, &zo);
        double cells = 1.0;
        const double lo[3] = {gmin[0], gmin[1], (double)gmin[2] + zo}, hi[3] = {gmax[0], gmax[1], (double)gmax[2] + zo};
        for (int a = 0; a < 3; ++a) cells *= std::floor((hi[a] - lo[a]) / (double)leaf[a]) + 3.0;
        const double per_slice = 2.0 * cells / W + 4.0;
        if (per_slice < (double)pad_bound) pad_bound = (int64_t)per_slice;
    }
    c->xchg_stats[0] = n_local;
    c->xchg_stats[1] = n_local - send[(size_t)rank];                                   // points sent to other ranks
    c->xchg_stats[2] = n_recv - recv[(size_t)rank];                                    // points received from other ranks
    c->xchg_stats[3] = c->xchg_stats[1] * (int64_t)sizeof(o3dr_point);                 // bytes sent over the links
    c->xchg_stats[4] = c->xchg_stats[2] * (int64_t)sizeof(o3dr_point);
    c->xchg_stats[5] = n_recv;                                                         // points entering this rank's merge
    c->xchg_stats[7] = total_pts;
    // Where this rank's points go: its own slice stays with it, placed once with room in front for what the lower ranks
    // send and behind for the higher ranks'; the slices that leave follow.  A rank that neither sends nor receives
    // anything keeps its cloud as it is (its recorded box and run heads stay valid).
    auto placed = [&](int r, int64_t& off_rank, int64_t& nr) {  // points rank r's exchange buffer must hold (0: nothing moves there)
        nr = 0;
        for (int p = 0; p < W; ++p) nr += sends(p, r);
        off_rank = hdrs[r].count - sends(r, r);
        return (off_rank == 0 && nr == sends(r, r)) ? (int64_t)0 : nr + off_rank;
    };
    int64_t n_off = 0, nr_me = 0;
    const int64_t need_alt = overflow ? 0 : placed(rank, n_off, nr_me);
    const bool moves = need_alt != 0;
    // does any rank have to grow a buffer before the all-to-all?  (every rank evaluates every rank: no disagreement)
    bool any_grows = false;
    for (int r = 0; r < W; ++r) {
        int64_t o_r = 0, n_r = 0;
        const int64_t need_r = overflow ? 0 : placed(r, o_r, n_r);
        const int64_t* ex = mat + (size_t)r * RW + W + 2;
        any_grows = any_grows || need_r > ex[0] || max_slice > ex[1] || (gather_result && (int64_t)W * pad_bound > ex[2]);
    }
    if (any_grows) {
        int rc = O3DR_OK;
        if (injected(3)) rc = O3DR_ERR_ALLOC;
        if (rc == O3DR_OK && need_alt > 0) rc = alt_reserve(c, need_alt);
        if (rc == O3DR_OK) rc = dev_ensure(c, c->st_merge, (size_t)(max_slice > 0 ? max_slice : 1) * sizeof(o3dr_point));
        if (rc == O3DR_OK && gather_result) rc = dev_ensure(c, c->st_gather, (size_t)W * (size_t)(pad_bound > 0 ? pad_bound : 1) * sizeof(o3dr_point));
        note(rc);
        extra[0] = (int64_t)local;
        HIPCHK(hipMemcpyAsync(d + o_row, extra, 8, hipMemcpyHostToDevice, c->stream));
        CHK(T.all_gather(c, d + o_row, d + o_mat, 8));
        HIPCHK(hipMemcpyAsync(c->xchg_host + o_mat, d + o_mat, 8 * (size_t)W, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->xchg_stats[6] = 1;  // agreement rounds of this call
        for (int r = 0; r < W; ++r)
            if (mat[r] < 0) return peer_error(local, r, mat[r], local_msg);
    }
    c->cloud_ub = n_local;  // (its own header told the host)
    c->cloud_n_exact = true;
    if (!overflow) {
        // one pass places the slices; the all-to-all then receives straight into the gaps (every peer pair has its own
        // xGMI link; segments land in source-rank order = global frame order); the own slice is never sent
        int64_t n_before = 0, n_after = 0;
        for (int p = 0; p < W; ++p) (p < rank ? n_before : n_after) += p == rank ? 0 : recv[(size_t)p];
        std::vector<int64_t> send_off((size_t)W, 0), recv_off((size_t)W, 0), send_x(send), recv_x(recv);
        send_x[(size_t)rank] = recv_x[(size_t)rank] = 0;
        if (moves) {
            int64_t send_start = 0;
            CHK(o3dr_cloud_big_place_slices(c, W, rank, send.data(), n_before, n_after, &send_start));
            int64_t so = send_start, lo = 0, hi = n_before + send[(size_t)rank];
            for (int p = 0; p < W; ++p) {
                if (p == rank) continue;
                send_off[(size_t)p] = so;
                so += send[(size_t)p];
                int64_t& ro = p < rank ? lo : hi;
                recv_off[(size_t)p] = ro;
                ro += recv[(size_t)p];
            }
        }
        CHK(T.all_to_all(c, c->cloud_big, send_off.data(), send_x.data(), recv_off.data(), recv_x.data()));
        if (moves) CHK(o3dr_cloud_big_set_size(c, n_recv));
    }
    // 4. local merge of the slice over the global box (the second host wait: its size).  A failure here travels with
    //    the merged sizes of the final gather, so that no rank waits in a collective the failed one never enters.
    int64_t m = 0;
    uint32_t st = 0;
    if (n_recv > 0) note(injected(4) ? O3DR_ERR_ALLOC : finalize_impl(c, gmin, gmax, (o3dr_point*)c->st_merge.p, max_slice, &m, &st, O3DR_MEM_DEVICE));
    if (overflow) st |= O3DR_STATUS_VOXEL_OVERFLOW;
    if (status) *status = st;
    const hipMemcpyKind kind = mem == O3DR_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (!gather_result) {  // (no collective follows: a local failure is this rank's alone)
        if (local != O3DR_OK) {
            g_err = local_msg;
            return local;
        }
        if (out_capacity > 0) {
            if (m > out_capacity) return fail(O3DR_ERR_CAPACITY, "output buffer too small");
            if (m > 0) HIPCHK(hipMemcpyAsync(out, c->st_merge.p, (size_t)m * sizeof(o3dr_point), kind, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            *n_out = m;
        }
        return O3DR_OK;
    }
    // 5. final gather: sizes (or error codes), then the slices padded to the largest (rank order = ascending voxel index)
    int64_t* mh = (int64_t*)c->xchg_host;
    mh[0] = local != O3DR_OK ? (int64_t)local : m;
    HIPCHK(hipMemcpyAsync(d + o_row, mh, sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    CHK(T.all_gather(c, d + o_row, d + o_mat, 8));
    HIPCHK(hipMemcpyAsync(c->xchg_host + o_mat, d + o_mat, 8 * (size_t)W, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int64_t pad = 0, merged_total = 0;
    for (int r = 0; r < W; ++r) {
        if (mat[r] < 0) return peer_error(local, r, mat[r], local_msg);
        pad = std::max(pad, mat[r]), merged_total += mat[r];
    }
    if (pad > pad_bound) return fail(O3DR_ERR_INTERNAL, "a merged slice exceeds its bound");  // (every rank: same sizes, same bound)
    if (pad > 0) CHK(T.all_gather(c, c->st_merge.p, c->st_gather.p, (size_t)pad * sizeof(o3dr_point)));
    if (out_capacity > 0) {  // (a rank that does not want the result passes no buffer; it still took part in the collectives)
        if (merged_total > out_capacity) {
            HIPCHK(hipStreamSynchronize(c->stream));
            return fail(O3DR_ERR_CAPACITY, "output buffer too small");
        }
        int64_t off = 0;
        for (int r = 0; r < W; ++r) {
            if (mat[r] > 0)
                HIPCHK(hipMemcpyAsync(out + off, (const o3dr_point*)c->st_gather.p + (size_t)r * (size_t)pad, (size_t)mat[r] * sizeof(o3dr_point), kind, c->stream));
            off += mat[r];
        }
        *n_out = merged_total;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_merge_partitioned(o3dr_ctx* c, void* nccl_comm, int32_t gather_result, o3dr_point* out, int64_t out_capacity,
                                      int64_t* n_out, int64_t* n_total, uint32_t* status, int32_t mem)
{
    if (n_out) *n_out = 0;
    if (n_total) *n_total = 0;
    if (status) *status = 0;
    CTX_ENTER(c);
    if (!nccl_comm || !n_out) return fail(O3DR_ERR_INVALID_ARG, "nccl_comm / n_out is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (out_capacity < 0 || (out_capacity > 0 && !out)) return fail(O3DR_ERR_INVALID_ARG, "out is NULL");
    RcclTransport T;
    T.R = rccl_api();
    if (!T.R) return fail(O3DR_ERR_HIP, "RCCL (librccl.so.1) could not be loaded");
    T.comm = (ncclComm_t)nccl_comm;
    NCCLCHK(T.R, T.R->CommCount(T.comm, &T.W));
    NCCLCHK(T.R, T.R->CommUserRank(T.comm, &T.rank));
    return merge_partitioned_impl(c, T, gather_result, out, out_capacity, n_out, n_total, status, mem);
}

extern "C" int o3dr_merge_partitioned_stats(o3dr_ctx* c, int64_t out[8])
{
    CTX_ENTER(c);
    if (!out) return fail(O3DR_ERR_INVALID_ARG, "out is NULL");
    memcpy(out, c->xchg_stats, sizeof c->xchg_stats);
    return O3DR_OK;
}

extern "C" int o3dr_cloud_big_capacity(o3dr_ctx* c, int64_t* cloud_points, int64_t* recv_points)
{
    CTX_ENTER(c);
    if (cloud_points) *cloud_points = c->cloud_cap;
    if (recv_points) *recv_points = c->cloud_alt_cap;
    return O3DR_OK;
}

// ---- test-only: the exchange among W contexts of one process (include/o3dr_testing.h) -----------------------------------
extern "C" int o3dr_test_local_comm_create(int32_t n_ranks, void** comm_out)
{
    if (n_ranks < 1 || n_ranks > kMaxRadix || !comm_out) return fail(O3DR_ERR_INVALID_ARG, "bad arguments (1 <= n_ranks <= 128)");
    LocalComm* L = new LocalComm;
    L->W = n_ranks;
    L->ptr.assign((size_t)n_ranks, nullptr);
    L->cnt.assign((size_t)n_ranks, nullptr);
    L->off.assign((size_t)n_ranks, nullptr);
    *comm_out = L;
    return O3DR_OK;
}
extern "C" int o3dr_test_local_comm_destroy(void* comm)
{
    delete (LocalComm*)comm;
    return O3DR_OK;
}
extern "C" int o3dr_test_merge_partitioned_local(o3dr_ctx* c, void* local_comm, int32_t rank, int32_t gather_result, o3dr_point* out,
                                                 int64_t out_capacity, int64_t* n_out, int64_t* n_total, uint32_t* status, int32_t mem)
{
    if (n_out) *n_out = 0;
    if (n_total) *n_total = 0;
    if (status) *status = 0;
    CTX_ENTER(c);
    if (!c->test_hooks) return fail(O3DR_ERR_INVALID_ARG, "test hooks are off (create the context with O3DR_TEST_HOOKS=1)");
    if (!local_comm || !n_out) return fail(O3DR_ERR_INVALID_ARG, "local_comm / n_out is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (out_capacity < 0 || (out_capacity > 0 && !out)) return fail(O3DR_ERR_INVALID_ARG, "out is NULL");
    LocalTransport T;
    T.L = (LocalComm*)local_comm;
    T.W = T.L->W;
    T.rank = rank;
    return merge_partitioned_impl(c, T, gather_result, out, out_capacity, n_out, n_total, status, mem);
}
extern "C" int o3dr_test_fail_at(o3dr_ctx* c, int32_t point)
{
    CTX_ENTER(c);
    if (!c->test_hooks) return fail(O3DR_ERR_INVALID_ARG, "test hooks are off (create the context with O3DR_TEST_HOOKS=1)");
    c->test_fail_at = point;
    return O3DR_OK;
}

// page-locking of caller memory (frame stacks handed to o3dr_accumulate_frames with O3DR_MEM_HOST then move by DMA)
extern "C" int o3dr_host_register(void* ptr, int64_t bytes)
{
    if (!ptr || bytes <= 0) return fail(O3DR_ERR_INVALID_ARG, "bad arguments");
    // (callers treat this as best effort: HIP's sticky last error must not outlive the failure, or the next
    // hipGetLastError() after a kernel launch would report it as that launch's)
    const hipError_t e = hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        char buf[256];
        snprintf(buf, sizeof buf, "hipHostRegister failed: %s", hipGetErrorString(e));
        return fail(O3DR_ERR_HIP, buf);
    }
    return O3DR_OK;
}
extern "C" int o3dr_host_unregister(void* ptr)
{
    if (!ptr) return O3DR_OK;
    const hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        char buf[256];
        snprintf(buf, sizeof buf, "hipHostUnregister failed: %s", hipGetErrorString(e));
        return fail(O3DR_ERR_HIP, buf);
    }
    return O3DR_OK;
}

// -------------------------------------------------------------------------------------------------
// measurement hooks
// -------------------------------------------------------------------------------------------------
extern "C" int o3dr_bilateral_filter_u8(o3dr_ctx* c, const uint8_t* src, int64_t src_pitch, int32_t rows, int32_t cols, int32_t d,
                                        double sigma_color, double sigma_space, uint8_t* dst, int64_t dst_pitch, int32_t mem)
{
    CTX_ENTER(c);
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (rows < 0 || cols < 0) return fail(O3DR_ERR_INVALID_ARG, "negative image size");
    if (rows == 0 || cols == 0) return O3DR_OK;
    if (!src || !dst) return fail(O3DR_ERR_INVALID_ARG, "src / dst is NULL");
    if (src_pitch < cols || dst_pitch < cols) return fail(O3DR_ERR_INVALID_ARG, "pitch smaller than a row");
    CHK(bilateral_prepare(c, d, sigma_color, sigma_space));
    const uint8_t* src_d = src;
    uint8_t* dst_d = dst;
    if (mem == O3DR_MEM_HOST) {
        const void* p;
        CHK(stage_in(c, c->st_blur_in, src, (size_t)src_pitch * rows, mem, &p));
        src_d = (const uint8_t*)p;
        CHK(dev_ensure(c, c->st_blur, (size_t)dst_pitch * rows));
        dst_d = (uint8_t*)c->st_blur.p;
    }
    launch_bilateral(&c->prof, c->stream, src_d, src_pitch, 0, rows, cols, 1, c->bil_radius, c->bil_maxk,
                     (const float*)c->bil_tab.p, dst_d, dst_pitch, 0);
    HIPCHK(hipGetLastError());
    if (mem == O3DR_MEM_HOST) {
        // only the pixels are written back: padding bytes of the caller's rows stay untouched
        HIPCHK(hipMemcpy2DAsync(dst, (size_t)dst_pitch, dst_d, (size_t)dst_pitch, (size_t)cols, (size_t)rows,
                                hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return O3DR_OK;
}

extern "C" int o3dr_disparity_variance(o3dr_ctx* c, const uint8_t* disp, int64_t disp_pitch, int64_t disp_frame_stride,
                                       int32_t rows, int32_t cols, int32_t n_frames, double* variance_out, int32_t mem)
{
    CTX_ENTER(c);
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (n_frames < 0 || rows <= 0 || cols <= 0) return fail(O3DR_ERR_INVALID_ARG, "bad image size / frame count");
    if (n_frames == 0) return O3DR_OK;
    if (!disp || !variance_out) return fail(O3DR_ERR_INVALID_ARG, "disp / variance_out is NULL");
    if (disp_pitch < cols) return fail(O3DR_ERR_INVALID_ARG, "pitch smaller than a row");
    if (c->params.disparity_f64) return fail(O3DR_ERR_INVALID_ARG, "o3dr_disparity_variance takes CV_8UC1 images");
    if (n_frames > 1 && disp_frame_stride < (int64_t)rows * disp_pitch)
        return fail(O3DR_ERR_INVALID_ARG, "frame stride smaller than a frame");
    const GridShape g = grid_shape(c->params, rows, cols);
    const void* disp_d;
    CHK(stage_in(c, c->st_blur_in, disp, (size_t)disp_frame_stride * (n_frames - 1) + (size_t)disp_pitch * rows, mem, &disp_d));
    const size_t hist_bytes = sizeof(unsigned long long) * 256 * (size_t)n_frames;
    CHK(dev_ensure(c, c->st_hist, hist_bytes + sizeof(double) * (size_t)n_frames));
    unsigned long long* hist = (unsigned long long*)c->st_hist.p;
    double* var_d = (double*)((char*)c->st_hist.p + hist_bytes);
    launch_disp_variance(&c->prof, c->stream, (const uint8_t*)disp_d, disp_pitch, disp_frame_stride, rows, cols, n_frames,
                         c->params.bounding_box, g.cs, c->params.min_disparity, hist, var_d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(variance_out, var_d, sizeof(double) * (size_t)n_frames, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_test_corrupt_next_gather(o3dr_ctx* c)
{
    CTX_ENTER(c);
    if (!c->test_hooks) return fail(O3DR_ERR_INVALID_ARG, "test hooks are off (create the context with O3DR_TEST_HOOKS=1)");
    c->test_corrupt = 1;
    return O3DR_OK;
}

extern "C" int o3dr_test_sor_distances(o3dr_ctx* c, float* out, int64_t n)
{
    CTX_ENTER(c);
    if (!c->test_hooks) return fail(O3DR_ERR_INVALID_ARG, "test hooks are off (create the context with O3DR_TEST_HOOKS=1)");
    if (!out || n < 0 || n > c->ws_sor_cap || !c->ws.sor_dist) return fail(O3DR_ERR_INVALID_ARG, "no outlier removal of that size has run");
    if (n == 0) return O3DR_OK;
    HIPCHK(hipMemcpyAsync(out, c->ws.sor_dist, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

// Every per-call scratch block the context owns, over its whole capacity (DESIGN.md "Scratch contract": the scratch list).
// Not here, because they carry something from one call to the next: cloud_big, cloud_alt, cc_big, cloud_box, cloud_heads;
// inc.grp / off / cells / box; bil_tab, orb_pat, q_lut; pl_hyp; stats_dev.
extern "C" int o3dr_test_fill_scratch(o3dr_ctx* c, int32_t byte, int64_t* bytes_filled)
{
    if (bytes_filled) *bytes_filled = 0;
    CTX_ENTER(c);
    if (!c->test_hooks) return fail(O3DR_ERR_INVALID_ARG, "test hooks are off (create the context with O3DR_TEST_HOOKS=1)");
    if (byte < 0 || byte > 255 || !bytes_filled) return fail(O3DR_ERR_INVALID_ARG, "byte must be 0..255, bytes_filled not NULL");
    c->place_ub = -1;  // a pending (slice, tile) table lives in the workspace
    int64_t total = 0;
    std::vector<DevBuf*> blocks = {&c->ws_block, &c->ws_pts_block, &c->ws_grid_block, &c->ws_sor_block, &c->st_disp, &c->st_bgr,
                                   &c->st_in, &c->st_out, &c->st_kp, &c->st_kpoff, &c->st_poses, &c->st_blur, &c->st_blur_in,
                                   &c->st_hist, &c->st_xchg, &c->st_merge, &c->st_gather, &c->nn_q, &c->nn_t, &c->nn_cells,
                                   &c->nn_src, &c->inc.scratch, &c->inc.tg, &c->inc.tmatch, &c->inc.flag, &c->inc.src,
                                   &c->inc.keep, &c->inc.partial, &c->inc.words, &c->inc.fb};
    for (int i = 0; i < 2; ++i) {
        blocks.push_back(&c->st2_disp[i]);
        blocks.push_back(&c->st2_bgr[i]);
        blocks.push_back(&c->st2_poses[i]);
    }
    for (DevBuf& b : c->op) blocks.push_back(&b);
    // (the uploads of a host frame call run on their own stream, but c->stream has waited for each of them)
    for (DevBuf* b : blocks) {
        if (!b->p || !b->cap) continue;
        HIPCHK(hipMemsetAsync(b->p, byte, b->cap, c->stream));
        total += (int64_t)b->cap;
    }
    HIPCHK(hipMemsetAsync(c->misc_dev, byte, 4096, c->stream));
    HIPCHK(hipMemsetAsync(c->cc_tmp, byte, sizeof(CloudCounters), c->stream));
    *bytes_filled = total + 4096 + (int64_t)sizeof(CloudCounters);
    return O3DR_OK;
}

// -------------------------------------------------------------------------------------------------
// exact nearest neighbour and point-to-point ICP (kernels/nn.inc; DESIGN.md "ICP")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_icp_default_params(o3dr_icp_params* p)
{
    if (!p) return;
    p->max_iterations = 10;                     // pcl::Registration max_iterations_
    p->max_correspondence_distance = HUGE_VAL;  // pcl::Registration corr_dist_threshold_: no limit
    p->transformation_epsilon = 0.0;
}

// One cloud's search grid, built once per call: the grid in ws.grid_* (which the SOR path rebuilds whenever it runs: *grid
// is good for this call only), the cells' boxes and the cloud's box in c->nn_cells.  The sort workspace is reused: the
// exchange's pending slice table is gone.  mm_used >= 0: the cloud's min/max slots are in ws.mm [0, mm_used) and
// ws.n_valid[0] is set already (by a caller whose ws_ensure had the arguments of the one here); < 0: taken here.
static int search_grid_build(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, int mem, int mm_used, SearchGrid* grid)
{
    c->place_ub = -1;
    const void* t_d;
    CHK(stage_in(c, c->nn_t, cloud, (size_t)n * sizeof(o3dr_point), mem, &t_d));
    CHK(ws_ensure(c, 1, n, false));
    CHK(grid_ensure(c, 1, n));
    const size_t cells = (size_t)c->ws.grid_max_cells + 1;
    float* box6;
    float4 *cell_lo, *cell_hi;
    CHK(carve(c, c->nn_cells, [&](Carve& w) {
        w.take(cell_lo, cells);
        w.take(cell_hi, cells);
        w.take(box6, 6);
    }));
    if (mm_used < 0) {
        launch_set_counts(&c->prof, c->stream, c->ws.n_valid, (uint32_t)n, 1);
        mm_used = launch_points_minmax(&c->prof, c->stream, (const o3dr_point*)t_d, 0, c->ws.n_valid, 1, n, c->ws.mm_stride, c->ws.mm);
    }
    *grid = launch_nn_grid(&c->prof, c->stream, c->ws, (const o3dr_point*)t_d, n, mm_used, box6, cell_lo, cell_hi);
    HIPCHK(hipGetLastError());
    return O3DR_OK;
}

// per-call source arrays: idx of two passes, d2, kIcpRecord partials per workgroup, the folded record
struct NnSrc {
    uint32_t* idx[2];
    float* d2;
    double* partial;
    double* rec;
};
static int nn_source(o3dr_ctx* c, int64_t n, NnSrc* o)
{
    return carve(c, c->nn_src, [&](Carve& w) {
        w.take(o->idx[0], (size_t)n);
        w.take(o->idx[1], (size_t)n);
        w.take(o->d2, (size_t)n);
        w.take(o->partial, (size_t)kIcpRecord * (size_t)nn_partial_blocks(n));
        w.take(o->rec, (size_t)kIcpRecord);
    });
}

constexpr int64_t kCloudMax = 0xffffffffLL, kMeshCloudMax = 0x7fffffffLL;  // points in one cloud (the mesh's indices are int32)
static int nn_check_cloud(int64_t n, const void* p, int64_t max_points = kCloudMax)
{
    if (n < 0 || (n > 0 && !p)) return fail(O3DR_ERR_INVALID_ARG, "bad arguments (cloud pointer / size)");
    if (n > max_points)
        return fail(O3DR_ERR_INVALID_ARG, max_points == kCloudMax ? "more than 2^32-1 points in one cloud" : "2^31 or more points in one cloud");
    return O3DR_OK;
}
// n if it can be a cloud's size, else 0: what an entry point sizes its host outputs by before anything is validated
static inline int64_t cloud_points(int64_t n, int64_t max_points = kCloudMax) { return n > 0 && n <= max_points ? n : 0; }

// What MLS, plane segmentation and meshing do with a checked cloud of n > 0 points: stage it (c->nn_t), and have every
// coordinate checked for being finite before a grid sees the cloud.  `flag` is the operator's device flag word, of which
// the first flag_bytes are read into flag_h; `also` enqueues what else the operator wants done before that one
// synchronisation.
template <class Also>
static int cloud_stage_finite(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, int mem, uint32_t* flag, uint32_t* flag_h, size_t flag_bytes,
                              const o3dr_point** cloud_d, Also&& also)
{
    const void* d;
    CHK(stage_in(c, c->nn_t, cloud, (size_t)n * sizeof(o3dr_point), mem, &d));
    *cloud_d = (const o3dr_point*)d;
    launch_cloud_finite(&c->prof, c->stream, *cloud_d, n, flag);
    CHK(also());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(flag_h, flag, flag_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (flag_h[0]) return fail(O3DR_ERR_INVALID_ARG, "the cloud has a non-finite coordinate");
    return O3DR_OK;
}
static int nothing_else() { return O3DR_OK; }
// the operators' device flags, ranges and counters (c->op[OP_FLAGS]), 64 bytes apart: each group is read back on its own
struct MlsFlags {
    alignas(64) unsigned long long counters[4];  // none, plane, poly, max neighbours
    alignas(64) uint32_t bad;                    // non-finite
};
// the non-finite flag and the cell index range (launch_cell_range), read back together
struct CellFlags {
    uint32_t bad;           // non-finite
    uint32_t range[4];      // ix_min ix_max iy_min iy_max (order-preserving)
    uint32_t off_int32[4];  // [0]: an index leaves int32 (the fold writes four words)
};
struct PlaneFlags {
    alignas(64) CellFlags cell;
    alignas(64) uint32_t n_tiles;
};
struct MeshFlags {
    alignas(64) CellFlags cell;
    alignas(64) uint32_t cnt[2];       // V, T
    alignas(64) uint32_t counters[3];  // full quads, rejected by orientation, rejected by length
};
// the raster family (a RasterFrame's range pass, then the operator's own counters)
template <int N>
struct FrameFlags {
    alignas(64) CellFlags cell;
    alignas(64) uint32_t counters[N];
};
using RasterFlags = FrameFlags<12>;                   // RasterArgs::counters
using GroundFlags = FrameFlags<kGroundCounterWords>;  // GroundArgs::counters
using SampleFlags = FrameFlags<4>;                    // SampleArgs::counters
// The index box of a read-back range: its corner and widths -> o, the width of the largest dense cell id -> *nbits.
// Fails, with the operator's texts, if an index left int32 or the box holds more than `limit` cells.
static int cell_box(const CellFlags& h, uint64_t limit, const char* off_int32_text, const char* limit_text, CellOrder* o, int* nbits)
{
    if (h.off_int32[0]) return fail(O3DR_ERR_INVALID_ARG, off_int32_text);
    o->x0 = (int32_t)(h.range[0] ^ 0x80000000u);
    o->y0 = (int32_t)(h.range[2] ^ 0x80000000u);
    o->wx = (uint64_t)(h.range[1] - h.range[0]) + 1;
    o->wy = (uint64_t)(h.range[3] - h.range[2]) + 1;
    if (o->wx > limit / o->wy) return fail(O3DR_ERR_INVALID_ARG, limit_text);
    const uint64_t max_key = o->wx * o->wy - 1;
    *nbits = 0;
    while (*nbits < 32 && (max_key >> *nbits) != 0) ++*nbits;
    return O3DR_OK;
}
template <class Flags>
static int op_flags(o3dr_ctx* c, Flags** f)
{
    return carve(c, c->op[o3dr_ctx::OP_FLAGS], [&](Carve& w) { w.take(*f, 1); });
}

extern "C" int o3dr_nearest_neighbors(o3dr_ctx* c, const o3dr_point* query, int64_t n_query, const o3dr_point* target,
                                      int64_t n_target, double max_distance, uint32_t* idx_out, float* d2_out, int32_t mem)
{
    Outputs outs{mem};
    outs.add(idx_out, cloud_points(n_query));
    outs.add(d2_out, cloud_points(n_query));
    outs.zero();  // outputs zeroed first
    CTX_ENTER(c);
    CHK(nn_check_cloud(n_query, query));
    CHK(nn_check_cloud(n_target, target));
    if (n_query > 0 && (!idx_out || !d2_out)) return fail(O3DR_ERR_INVALID_ARG, "idx_out / d2_out is NULL");
    if (!(max_distance >= 0.0)) return fail(O3DR_ERR_INVALID_ARG, "max_distance must be >= 0 (+inf: no limit)");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    c->place_ub = -1;
    if (n_query == 0) return O3DR_OK;
    const float r2 = (float)(max_distance * max_distance);
    CHK(outs.stage(c));
    uint32_t* idx_d = outs.dev(idx_out);
    float* d2_d = outs.dev(d2_out);
    if (n_target == 0) {  // no target point: none found
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)idx_d, (int)0xFFFFFFFFu, (size_t)n_query, c->stream));
        HIPCHK(hipMemsetD32Async((hipDeviceptr_t)d2_d, (int)0x7f800000u, (size_t)n_query, c->stream));
    } else {
        SearchGrid grid;
        CHK(search_grid_build(c, target, n_target, mem, -1, &grid));
        const void* q_d;
        CHK(stage_in(c, c->nn_q, query, (size_t)n_query * sizeof(o3dr_point), mem, &q_d));
        launch_nn_query(&c->prof, c->stream, grid, (const o3dr_point*)q_d, n_query, nullptr, r2, idx_d, d2_d, nullptr, nullptr, nullptr,
                        nullptr);
        HIPCHK(hipGetLastError());
    }
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_icp_align(o3dr_ctx* c, const o3dr_point* source, int64_t n_source, const o3dr_point* target, int64_t n_target,
                              const float T_init[16], const o3dr_icp_params* p, o3dr_icp_result* res, int32_t mem)
{
    if (res) memset(res, 0, sizeof *res);
    CTX_ENTER(c);
    if (!res) return fail(O3DR_ERR_INVALID_ARG, "res is NULL");
    CHK(nn_check_cloud(n_source, source));
    CHK(nn_check_cloud(n_target, target));
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    o3dr_icp_params prm;
    o3dr_icp_default_params(&prm);
    if (p) prm = *p;
    if (prm.max_iterations < 0 || !(prm.max_correspondence_distance >= 0.0) || !(prm.transformation_epsilon >= 0.0))
        return fail(O3DR_ERR_INVALID_ARG, "bad parameters (max_iterations >= 0, max_correspondence_distance >= 0, transformation_epsilon >= 0)");
    c->place_ub = -1;
    double T[16];
    for (int k = 0; k < 16; ++k) T[k] = T_init ? (double)T_init[k] : (k % 5 == 0 ? 1.0 : 0.0);
    for (int k = 0; k < 16; ++k) res->T[k] = T[k];
    res->fitness = DBL_MAX;  // pcl::Registration::getFitnessScore without correspondences
    res->reason = O3DR_ICP_TOO_FEW;
    if (n_source == 0 || n_target == 0) return O3DR_OK;

    SearchGrid grid;
    CHK(search_grid_build(c, target, n_target, mem, -1, &grid));
    const void* s_d;
    CHK(stage_in(c, c->nn_q, source, (size_t)n_source * sizeof(o3dr_point), mem, &s_d));
    NnSrc o;
    CHK(nn_source(c, n_source, &o));
    float box_h[6];
    HIPCHK(hipMemcpyAsync(box_h, grid.box6, sizeof box_h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const double c0[3] = {((double)box_h[0] + (double)box_h[3]) * 0.5, ((double)box_h[1] + (double)box_h[4]) * 0.5,
                          ((double)box_h[2] + (double)box_h[5]) * 0.5};
    const float r2 = (float)(prm.max_correspondence_distance * prm.max_correspondence_distance);
    double rec[kIcpRecord];
    int cur = 0, passes = 0;
    // one pass at fp32(T): A2 of the original source, nearest neighbours, the record of the moments
    auto pass = [&](bool compare) -> int {
        float Tf[12];
        for (int k = 0; k < 12; ++k) Tf[k] = (float)T[k];
        launch_nn_query(&c->prof, c->stream, grid, (const o3dr_point*)s_d, n_source, Tf, r2, o.idx[cur], nullptr,
                        compare ? o.idx[cur ^ 1] : nullptr, c0, o.partial, o.rec);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rec, o.rec, sizeof rec, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        cur ^= 1;
        ++passes;
        return O3DR_OK;
    };
    int iterations = 0, reason = O3DR_ICP_MAX_ITERATIONS;
    bool rec_at_T = false;  // rec describes a pass at fp32 of the current T
    for (;;) {
        if (iterations >= prm.max_iterations) {
            reason = O3DR_ICP_MAX_ITERATIONS;
            break;
        }
        CHK(pass(passes > 0));
        rec_at_T = true;
        if (passes > 1 && rec[ICP_CHANGED] == 0.0) {
            reason = O3DR_ICP_UNCHANGED;
            break;
        }
        if (rec[RIGID_N] < 3.0) {
            reason = O3DR_ICP_TOO_FEW;
            break;
        }
        double dT[16] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0};
        if (!rigid_solve(rec, c0, dT)) {  // (the Kabsch of the rigid core: o3dr_rigid_solve.h)
            reason = O3DR_ICP_DEGENERATE;
            break;
        }
        double Tn[16];
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j)
                Tn[4 * i + j] = dT[4 * i] * T[j] + dT[4 * i + 1] * T[4 + j] + dT[4 * i + 2] * T[8 + j] + dT[4 * i + 3] * T[12 + j];
        for (int k = 0; k < 16; ++k) T[k] = Tn[k];
        rec_at_T = false;
        ++iterations;
        double step = 0.0;
        for (int k = 0; k < 12; ++k) step = std::max(step, std::fabs(dT[k] - (k % 5 == 0 ? 1.0 : 0.0)));
        if (step <= prm.transformation_epsilon) {
            reason = O3DR_ICP_SMALL_STEP;
            break;
        }
    }
    if (!rec_at_T) CHK(pass(false));  // fitness at T_out
    for (int k = 0; k < 16; ++k) res->T[k] = T[k];
    res->n_correspondences = (int64_t)rec[RIGID_N];
    res->fitness = rec[RIGID_N] > 0.0 ? rec[ICP_D2] / rec[RIGID_N] : DBL_MAX;
    res->iterations = iterations;
    res->reason = reason;
    return O3DR_OK;
}

// -------------------------------------------------------------------------------------------------
// moving-least-squares smoothing and normals (kernels/mls.inc; DESIGN.md "MLS")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_mls_default_params(o3dr_mls_params* p)
{
    if (!p) return;
    p->search_radius = 0.0;    // no usable default: the caller sets it
    p->polynomial_order = 2;   // pcl::MovingLeastSquares order_
    p->sqr_gauss_param = 0.0;  // search_radius^2, as PCL's setSearchRadius sets it
}

extern "C" int o3dr_mls_smooth(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, const o3dr_mls_params* p, o3dr_point* out,
                               float* normals, uint32_t* nn_count, uint8_t* fit, o3dr_mls_result* res, int32_t mem)
{
    if (res) memset(res, 0, sizeof *res);
    Outputs outs{mem};
    outs.add(out, cloud_points(n));
    outs.add(normals, 4 * cloud_points(n));
    outs.add(nn_count, cloud_points(n));
    outs.add(fit, cloud_points(n));
    outs.zero(cloud);  // outputs zeroed first (out may be the input)
    CTX_ENTER(c);
    CHK(nn_check_cloud(n, cloud));
    if (!p) return fail(O3DR_ERR_INVALID_ARG, "params is NULL");
    if (n > 0 && !out) return fail(O3DR_ERR_INVALID_ARG, "out is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    const double r = p->search_radius;
    if (!(std::isfinite(r) && r > 0.0)) return fail(O3DR_ERR_INVALID_ARG, "search_radius must be finite and > 0");
    if (p->polynomial_order < 0 || p->polynomial_order > 2) return fail(O3DR_ERR_INVALID_ARG, "polynomial_order must be 0, 1 or 2");
    if (!(std::isfinite(p->sqr_gauss_param) && p->sqr_gauss_param >= 0.0))
        return fail(O3DR_ERR_INVALID_ARG, "sqr_gauss_param must be finite and >= 0 (0: search_radius^2)");
    const double h = p->sqr_gauss_param > 0.0 ? p->sqr_gauss_param : r * r;
    if (!(h > 0.0 && std::isfinite(h))) return fail(O3DR_ERR_INVALID_ARG, "search_radius^2 is not a usable sqr_gauss_param");
    c->place_ub = -1;
    if (n == 0) return O3DR_OK;
    MlsFlags* f;
    CHK(op_flags(c, &f));
    const o3dr_point* cloud_d;
    uint32_t bad = 0;
    const int staged = cloud_stage_finite(c, cloud, n, mem, &f->bad, &bad, 4, &cloud_d, nothing_else);
    if (bad && mem == O3DR_MEM_HOST && out == cloud) memset(out, 0, (size_t)n * sizeof(o3dr_point));
    CHK(staged);
    SearchGrid grid;
    CHK(search_grid_build(c, cloud_d, n, O3DR_MEM_DEVICE, -1, &grid));
    CHK(outs.stage(c));
    launch_mls(&c->prof, c->stream, grid, cloud_d, n, r, p->polynomial_order, h, outs.dev(out), outs.dev(normals),
               outs.dev(nn_count), outs.dev(fit), f->counters);
    HIPCHK(hipGetLastError());
    unsigned long long cnt_h[4];
    HIPCHK(hipMemcpyAsync(cnt_h, f->counters, sizeof cnt_h, hipMemcpyDeviceToHost, c->stream));
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (res) {
        res->n_none = (int64_t)cnt_h[0];
        res->n_plane = (int64_t)cnt_h[1];
        res->n_poly = (int64_t)cnt_h[2];
        res->max_neighbors = (int32_t)std::min<unsigned long long>(cnt_h[3], 0x7fffffffull);
    }
    return O3DR_OK;
}

// -------------------------------------------------------------------------------------------------
// RANSAC plane segmentation per XY tile (kernels/plane.inc; DESIGN.md "Plane segmentation")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_plane_default_params(o3dr_plane_params* p)
{
    if (!p) return;
    p->distance_threshold = 0.0;  // no usable default: the caller sets it
    p->max_iterations = 1000;     // pcl::SACSegmentation max_iterations_ (50 in PCL 1.8 is for the adaptive loop)
    p->tile_size = 0.0;           // the whole cloud
    p->seed = 0;
    p->optimize = 1;              // setOptimizeCoefficients(true)
}

// pl_hyp: nh hypothesis planes, then their scores
static void plane_hyp_layout(Carve& w, uint64_t nh, float4** hyp, uint32_t** counts)
{
    w.take(*hyp, nh);
    w.take(*counts, nh);
}

static int segment_plane(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, const o3dr_plane_params* p, uint8_t* inlier,
                         int32_t* tile, o3dr_point* projected, Outputs& outs, o3dr_plane_tile* tiles, int64_t tiles_capacity,
                         int64_t* n_tiles, int32_t mem)
{
    CHK(nn_check_cloud(n, cloud));
    if (!p) return fail(O3DR_ERR_INVALID_ARG, "params is NULL");
    if (!n_tiles) return fail(O3DR_ERR_INVALID_ARG, "n_tiles is NULL");
    if (tiles_capacity < 0 || (tiles_capacity > 0 && !tiles)) return fail(O3DR_ERR_INVALID_ARG, "bad tiles / tiles_capacity");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    const double t = p->distance_threshold, ts = p->tile_size;
    if (!(std::isfinite(t) && t > 0.0)) return fail(O3DR_ERR_INVALID_ARG, "distance_threshold must be finite and > 0");
    if (p->max_iterations < 1 || p->max_iterations > O3DR_PLANE_MAX_ITERATIONS)
        return fail(O3DR_ERR_INVALID_ARG, "max_iterations must be in [1, 2^20]");
    if (!(std::isfinite(ts) && ts >= 0.0)) return fail(O3DR_ERR_INVALID_ARG, "tile_size must be 0 or finite and > 0");
    if (p->optimize != 0 && p->optimize != 1) return fail(O3DR_ERR_INVALID_ARG, "optimize must be 0 or 1");
    c->place_ub = -1;
    if (n == 0) return O3DR_OK;
    const bool tiled = ts > 0.0;
    PlaneFlags* f;
    CHK(op_flags(c, &f));
    PlaneArgs a;
    memset(&a, 0, sizeof a);
    a.tiled = tiled ? 1 : 0;
    a.n = (uint32_t)n;
    a.H = (uint32_t)p->max_iterations;
    a.s = ts;
    a.tf = (float)t;
    a.seed = p->seed;
    float4* pts = nullptr;
    uint32_t *head = nullptr, *part = nullptr;
    if (tiled)
        CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
            w.take(pts, (size_t)n);
            w.take(head, (size_t)n);
            w.take(part, (size_t)cell_range_parts(n) * kPartWords);
        }));
    CellFlags h;
    CHK(cloud_stage_finite(c, cloud, n, mem, &f->cell.bad, &h.bad, tiled ? sizeof h : 4, &a.cloud, [&]() -> int {
        if (tiled) launch_cell_range(&c->prof, c->stream, a, part, f->cell.range);
        return O3DR_OK;
    }));
    a.pts = tiled ? pts : (const float4*)a.cloud;
    uint64_t T = 1;
    if (tiled) {
        int nbits;
        CHK(cell_box(h, 0xffffffffull, "a tile index does not fit in int32 (tile_size too small)",
                     "the tiles' index box holds more than 2^32-1 tiles", &a.cells, &nbits));
        CHK(ws_ensure(c, 1, n, false));
        launch_cell_order(&c->prof, c->stream, c->ws, a, nbits, head, &f->n_tiles);
        HIPCHK(hipGetLastError());
        uint32_t th = 0;
        HIPCHK(hipMemcpyAsync(&th, &f->n_tiles, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        T = th;
    }
    *n_tiles = (int64_t)T;
    if ((int64_t)T > tiles_capacity && tiles) return fail(O3DR_ERR_CAPACITY, "tiles_capacity is below the tile count");
    if (T * (uint64_t)a.H > (1ull << 31)) return fail(O3DR_ERR_INVALID_ARG, "n_tiles * max_iterations exceeds 2^31");
    a.n_tiles = (uint32_t)T;
    const int64_t max_chunks = n / kPlaneChunkPoints + (int64_t)T;
    if (!tiled) CHK(ws_ensure(c, 1, 1, false));  // (the scan's chunk partials)
    CHK(carve(c, c->op[o3dr_ctx::OP_LATE], [&](Carve& w) {
        w.take(a.tstart, T + 1);
        w.take(a.cfirst, T + 1);
        w.take(a.rec, T);
        w.take(a.partial, (size_t)max_chunks * kPlaneMomentsHost);
    }));
    CHK(carve(c, c->pl_hyp, [&](Carve& w) { plane_hyp_layout(w, T * a.H, &a.hyp, &a.counts); }));
    CHK(outs.stage(c));  // labels, tile ordinals, projected points
    a.inlier = outs.dev(inlier);
    a.tile = outs.dev(tile);
    a.projected = outs.dev(projected);
    c->pl_last_hyp = 0;
    launch_plane_tiles(&c->prof, c->stream, c->ws, a, pts);
    launch_plane_fit(&c->prof, c->stream, a, max_chunks, p->optimize);
    HIPCHK(hipGetLastError());
    const hipMemcpyKind back = mem == O3DR_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (tiles) HIPCHK(hipMemcpyAsync(tiles, a.rec, T * sizeof(o3dr_plane_tile), back, c->stream));
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->pl_last_hyp = T * a.H;
    return O3DR_OK;
}

extern "C" int o3dr_test_plane_hypotheses(o3dr_ctx* c, float* planes, uint32_t* counts, int64_t capacity, int64_t* n_out)
{
    CTX_ENTER(c);
    if (!c->test_hooks) return fail(O3DR_ERR_INVALID_ARG, "test hooks are off (create the context with O3DR_TEST_HOOKS=1)");
    if (!n_out || capacity < 0 || (capacity > 0 && (!planes || !counts))) return fail(O3DR_ERR_INVALID_ARG, "bad arguments");
    const uint64_t nh = c->pl_last_hyp;
    *n_out = (int64_t)nh;
    if ((uint64_t)capacity < nh) return fail(O3DR_ERR_CAPACITY, "capacity is below the hypothesis count");
    if (nh == 0) return O3DR_OK;
    Carve w{(char*)c->pl_hyp.p, 0};
    float4* hyp_d;
    uint32_t* counts_d;
    plane_hyp_layout(w, nh, &hyp_d, &counts_d);
    HIPCHK(hipMemcpyAsync(planes, hyp_d, nh * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(counts, counts_d, nh * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_segment_plane(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, const o3dr_plane_params* p, uint8_t* inlier,
                                  int32_t* tile, o3dr_point* projected, o3dr_plane_tile* tiles, int64_t tiles_capacity,
                                  int64_t* n_tiles, int32_t mem)
{
    if (n_tiles) *n_tiles = 0;
    Outputs outs{mem};
    outs.add(inlier, cloud_points(n));
    outs.add(tile, cloud_points(n));
    outs.add(projected, cloud_points(n));
    const int rc = entered(c, [&] { return segment_plane(c, cloud, n, p, inlier, tile, projected, outs, tiles, tiles_capacity, n_tiles, mem); });
    if (rc != O3DR_OK && rc != O3DR_ERR_CAPACITY) {  // host outputs zeroed on error (projected may be the input)
        if (n_tiles) *n_tiles = 0;
        outs.zero(cloud);
        if (mem == O3DR_MEM_HOST && tiles && tiles_capacity > 0) memset(tiles, 0, (size_t)tiles_capacity * sizeof(o3dr_plane_tile));
    }
    return rc;
}

// -------------------------------------------------------------------------------------------------
// The raster frame's host side (RasterFrame in o3dr_device.h; DESIGN.md "Raster frame"): what the map raster, the ground
// filter and the raster sample check and stage alike.  Each operator calls these where its contract's error order has them.
// -------------------------------------------------------------------------------------------------
// inv = 1.0f / (float)cell_size of the floor rule (the surface mesh's too)
static int frame_cell_size(double cs, float* inv)
{
    const float csf = (float)cs;
    *inv = 1.0f / csf;
    if (!(std::isfinite(cs) && cs > 0.0 && std::isfinite(csf) && csf > 0.f && std::isfinite(*inv) && *inv > 0.f))
        return fail(O3DR_ERR_INVALID_ARG, "cell_size must be finite and > 0 (and usable in fp32)");
    return O3DR_OK;
}
static int box_check(int32_t cx0, int32_t cy0, int32_t width, int32_t height)
{
    if (width < 1 || height < 1) return fail(O3DR_ERR_INVALID_ARG, "the raster's box needs width, height >= 1");
    if ((int64_t)cx0 + width - 1 > INT32_MAX || (int64_t)cy0 + height - 1 > INT32_MAX)
        return fail(O3DR_ERR_INVALID_ARG, "the raster's box leaves int32");
    return O3DR_OK;
}
// width * height of a box or raster the outputs can be sized by before anything else is validated: 0 outside the limits
static int64_t box_cells(int32_t width, int32_t height)
{
    if (width < 1 || height < 1) return 0;
    const int64_t cells = (int64_t)width * height;
    return cells <= (int64_t)O3DR_RASTER_MAX_CELLS ? cells : 0;
}
constexpr const char* kRasterTooLarge = "the raster's box holds more than 2^28 cells";
// the cells of a box that has passed box_check
static int box_limit(const RasterFrame& f, int64_t* cells)
{
    *cells = box_cells(f.width, f.height);
    return *cells ? O3DR_OK : fail(O3DR_ERR_INVALID_ARG, kRasterTooLarge);
}
// The frame of a call filled: the box, and for n > 0 the cloud staged, every coordinate checked for being finite and every
// cell index for fitting int32 in one synchronisation (dev: the operator's device flags; the cloud's cell range in *h).
// f->part is the range pass's partials, all of OP_WORK until the operator carves its own.
static int raster_frame(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, int mem, float inv, const int32_t box[4], CellFlags* dev,
                        CellFlags* h, RasterFrame* f)
{
    f->n = (uint32_t)n, f->inv = inv;
    f->cx0 = box[0], f->cy0 = box[1], f->width = box[2], f->height = box[3];
    if (n == 0) return O3DR_OK;
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) { w.take(f->part, (size_t)cell_range_parts(n) * kPartWords); }));
    CHK(cloud_stage_finite(c, cloud, n, mem, &dev->bad, &h->bad, sizeof *h, &f->cloud, [&]() -> int {
        launch_cell_range(&c->prof, c->stream, *f, f->part, dev->range);
        return O3DR_OK;
    }));
    if (h->off_int32[0]) return fail(O3DR_ERR_INVALID_ARG, "a cell index does not fit in int32 (cell_size too small)");
    return O3DR_OK;
}
// An entry point of the family: the result (res, res_bytes; may be NULL) cleared, the call under `entered`, and on any
// error the result cleared again and the host outputs zeroed.
template <class Impl>
static int raster_entry(o3dr_ctx* c, const Outputs& outs, void* res, size_t res_bytes, Impl&& impl)
{
    if (res) memset(res, 0, res_bytes);
    const int rc = entered(c, impl);
    if (rc != O3DR_OK) {
        if (res) memset(res, 0, res_bytes);
        outs.zero();
    }
    return rc;
}

// -------------------------------------------------------------------------------------------------
// height-field surface mesh (kernels/mesh.inc; DESIGN.md "Surface mesh")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_mesh_default_params(o3dr_mesh_params* p)
{
    if (!p) return;
    p->cell_size = 0.0;        // no usable default: the map's voxel_size
    p->max_edge_length = 0.0;  // no usable default: GP3's search radius
}

static int mesh_surface(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, const o3dr_mesh_params* p, int32_t* tris,
                        int64_t tris_capacity, int64_t* n_tris, float* normals, Outputs& outs, o3dr_mesh_result* res, int32_t mem)
{
    CHK(nn_check_cloud(n, cloud, kMeshCloudMax));
    if (!p) return fail(O3DR_ERR_INVALID_ARG, "params is NULL");
    if (!n_tris) return fail(O3DR_ERR_INVALID_ARG, "n_tris is NULL");
    if (tris_capacity < 0 || (tris_capacity > 0 && !tris)) return fail(O3DR_ERR_INVALID_ARG, "bad tris / tris_capacity");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    const double L = p->max_edge_length;
    float inv;
    CHK(frame_cell_size(p->cell_size, &inv));
    if (!(L > 0.0)) return fail(O3DR_ERR_INVALID_ARG, "max_edge_length must be > 0 (+inf: no gate)");
    c->place_ub = -1;
    if (n == 0) return O3DR_OK;
    MeshFlags* f;
    CHK(op_flags(c, &f));
    MeshArgs a;
    memset(&a, 0, sizeof a);
    uint32_t* head;
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(head, (size_t)n);
        w.take(a.cnt, (size_t)n);
        w.take(a.vkey, (size_t)n);
        w.take(a.vpt, (size_t)n);
        w.take(a.nbr, (size_t)n);
        w.take(a.part, (size_t)((n + 255) / 256) * kPartWords);  // one record per 256-thread workgroup
    }));
    a.n = (uint32_t)n;
    a.inv = inv;
    a.lf = (float)(L * L);
    CellFlags h;
    CHK(cloud_stage_finite(c, cloud, n, mem, &f->cell.bad, &h.bad, sizeof h, &a.cloud, [&]() -> int {
        launch_cell_range(&c->prof, c->stream, a, a.part, f->cell.range);
        return O3DR_OK;
    }));
    int nbits;
    CHK(cell_box(h, 1ull << 32, "a cell index does not fit in int32 (cell_size too small)",
                 "the cells' index box holds more than 2^32 cells", &a.cells, &nbits));
    CHK(ws_ensure(c, 1, n, false));
    a.counters = f->counters;
    launch_cell_order(&c->prof, c->stream, c->ws, a, nbits, head, &f->cnt[0]);
    launch_mesh_count(&c->prof, c->stream, c->ws, a, &f->cnt[1]);
    HIPCHK(hipGetLastError());
    uint32_t vt_h[2], cnt_h[3];
    HIPCHK(hipMemcpyAsync(vt_h, f->cnt, sizeof vt_h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(cnt_h, f->counters, sizeof cnt_h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int64_t V = vt_h[0], T = vt_h[1];
    *n_tris = T;
    if (tris && T > tris_capacity) return fail(O3DR_ERR_CAPACITY, "tris_capacity is below the triangle count");
    outs.set_count(tris, 3 * T);
    CHK(outs.stage(c));  // triangles, normals
    a.tris = T > 0 ? outs.dev(tris) : nullptr;
    a.normals = outs.dev(normals);
    launch_mesh_emit(&c->prof, c->stream, a);
    HIPCHK(hipGetLastError());
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (res) {
        res->n_vertices = V;
        res->n_shadowed = n - V;
        res->n_triangles = T;
        res->n_quads_full = (int64_t)cnt_h[0];
        res->n_rejected_orientation = (int64_t)cnt_h[1];
        res->n_rejected_length = (int64_t)cnt_h[2];
    }
    return O3DR_OK;
}

extern "C" int o3dr_mesh_surface(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, const o3dr_mesh_params* p, int32_t* tris,
                                 int64_t tris_capacity, int64_t* n_tris, float* vertex_normals, o3dr_mesh_result* res, int32_t mem)
{
    if (n_tris) *n_tris = 0;
    if (res) memset(res, 0, sizeof *res);
    Outputs outs{mem};
    outs.add(tris, 3 * cloud_points(tris_capacity));
    outs.add(vertex_normals, 3 * cloud_points(n, kMeshCloudMax));
    const int rc = entered(c, [&] { return mesh_surface(c, cloud, n, p, tris, tris_capacity, n_tris, vertex_normals, outs, res, mem); });
    if (rc != O3DR_OK && rc != O3DR_ERR_CAPACITY) {  // host outputs zeroed on error
        if (n_tris) *n_tris = 0;
        outs.zero();
    }
    return rc;
}

// -------------------------------------------------------------------------------------------------
// map raster: orthophoto, elevation raster, shaded relief (kernels/raster.inc; DESIGN.md "Map raster")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_raster_default_params(o3dr_raster_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);  // cell_size and the box: no usable default
    p->select = O3DR_RASTER_FIRST;
    p->light[0] = -1.0, p->light[1] = 1.0, p->light[2] = 1.0;
}

static int raster_extent(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, double cell_size, int32_t* box[4], int32_t mem)
{
    CHK(nn_check_cloud(n, cloud, kMeshCloudMax));
    if (!box[0] || !box[1] || !box[2] || !box[3]) return fail(O3DR_ERR_INVALID_ARG, "cx0 / cy0 / width / height is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    float inv;
    CHK(frame_cell_size(cell_size, &inv));
    if (n == 0) return fail(O3DR_ERR_INVALID_ARG, "an empty cloud has no cell box");
    c->place_ub = -1;
    RasterFlags* f;
    CHK(op_flags(c, &f));
    const int32_t no_box[4] = {0, 0, 0, 0};  // (the cloud's own box is what is asked for)
    RasterFrame frame{};
    CellFlags h;
    CHK(raster_frame(c, cloud, n, mem, inv, no_box, &f->cell, &h, &frame));
    CellOrder o;
    int nbits;
    CHK(cell_box(h, (uint64_t)O3DR_RASTER_MAX_CELLS, "", kRasterTooLarge, &o, &nbits));
    *box[0] = o.x0, *box[1] = o.y0, *box[2] = (int32_t)o.wx, *box[3] = (int32_t)o.wy;
    return O3DR_OK;
}

extern "C" int o3dr_raster_extent(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, double cell_size, int32_t* cx0, int32_t* cy0,
                                  int32_t* width, int32_t* height, int32_t mem)
{
    int32_t* box[4] = {cx0, cy0, width, height};
    for (int32_t* b : box)
        if (b) *b = 0;
    const int rc = entered(c, [&] { return raster_extent(c, cloud, n, cell_size, box, mem); });
    if (rc != O3DR_OK)
        for (int32_t* b : box)
            if (b) *b = 0;
    return rc;
}

static int rasterize_map(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, const o3dr_raster_params* p, const o3dr_raster_outputs* out,
                         Outputs& outs, o3dr_raster_result* res, int32_t mem)
{
    CHK(nn_check_cloud(n, cloud, kMeshCloudMax));
    if (!p) return fail(O3DR_ERR_INVALID_ARG, "params is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    RasterArgs a;
    memset(&a, 0, sizeof a);
    float inv;
    CHK(frame_cell_size(p->cell_size, &inv));
    if (p->select != O3DR_RASTER_FIRST && p->select != O3DR_RASTER_TOP && p->select != O3DR_RASTER_BOTTOM)
        return fail(O3DR_ERR_INVALID_ARG, "select must be O3DR_RASTER_FIRST, _TOP or _BOTTOM");
    if (p->fill_radius < 0 || p->fill_radius > O3DR_RASTER_MAX_FILL_RADIUS) return fail(O3DR_ERR_INVALID_ARG, "fill_radius must be in 0..32");
    if (p->use_light) {
        const double* l = p->light;
        const double ln = std::sqrt((l[0] * l[0] + l[1] * l[1]) + l[2] * l[2]);
        if (!(std::isfinite(ln) && ln > 0.0)) return fail(O3DR_ERR_INVALID_ARG, "the light vector must be finite and not zero");
        for (int k = 0; k < 3; ++k) a.light[k] = l[k] / ln;
    } else if (out && out->shade) {
        return fail(O3DR_ERR_INVALID_ARG, "the shade output needs use_light");
    }
    CHK(box_check(p->cx0, p->cy0, p->width, p->height));
    c->place_ub = -1;
    a.select = p->select, a.R = p->fill_radius;
    a.cell_size = p->cell_size;
    RasterFlags* f;
    CHK(op_flags(c, &f));
    const int32_t box[4] = {p->cx0, p->cy0, p->width, p->height};
    CellFlags h;
    CHK(raster_frame(c, cloud, n, mem, inv, box, &f->cell, &h, &a.f));
    int64_t cells;
    CHK(box_limit(a.f, &cells));
    const int64_t tiles = raster_tiles(p->width, p->height), parts = std::max(tiles, raster_winner_parts(n));
    float* height_tmp = nullptr;  // the shade reads the filled heights: scratch when the caller does not ask for them
    const bool want_shade = p->use_light && out && out->shade;
    CHK(outs.stage(c));
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(a.f.part, (size_t)parts * kPartWords);
        w.take(a.win, (size_t)cells);
        if (a.R > 0) w.take(a.col, (size_t)cells);
        if (want_shade && !out->height_map) w.take(height_tmp, (size_t)cells);
    }));
    a.counters = f->counters;
    if (out) {
        a.height_map = outs.dev(out->height_map), a.color = outs.dev(out->color), a.source = outs.dev(out->source);
        a.distance2 = outs.dev(out->distance2);
        a.shade = want_shade ? outs.dev(out->shade) : nullptr;
    }
    if (!a.height_map) a.height_map = height_tmp;
    launch_raster(&c->prof, c->stream, a);
    HIPCHK(hipGetLastError());
    uint32_t cnt[12];
    HIPCHK(hipMemcpyAsync(cnt, f->counters, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (res) {
        res->cx0 = p->cx0, res->cy0 = p->cy0, res->width = p->width, res->height = p->height;
        res->n_inside = cnt[0], res->n_outside = cnt[1];
        res->n_occupied = cnt[4], res->n_shadowed = (int64_t)cnt[0] - (int64_t)cnt[4];
        res->n_filled = cnt[5], res->n_empty = cnt[6];
        const auto ordered = [](uint32_t u) {  // (ordered_f32 of kernels/util.inc)
            u ^= ((u >> 31) - 1u) | 0x80000000u;
            float z;
            memcpy(&z, &u, sizeof z);
            return z;
        };
        res->z_min = cnt[4] ? ordered(cnt[8]) : NAN;
        res->z_max = cnt[4] ? ordered(cnt[9]) : NAN;
    }
    return O3DR_OK;
}

extern "C" int o3dr_rasterize_map(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, const o3dr_raster_params* p,
                                  const o3dr_raster_outputs* out, o3dr_raster_result* res, int32_t mem)
{
    Outputs outs{mem};
    const int64_t cells = p ? box_cells(p->width, p->height) : 0;
    if (out) {
        outs.add(out->height_map, cells);
        outs.add(out->color, 3 * cells);
        outs.add(out->shade, cells);
        outs.add(out->source, cells);
        outs.add(out->distance2, cells);
    }
    return raster_entry(c, outs, res, sizeof *res, [&] { return rasterize_map(c, cloud, n, p, out, outs, res, mem); });
}

// -------------------------------------------------------------------------------------------------
// ground filter: ground mask, DTM, height above ground (kernels/ground.inc; contract: include/o3dr_terrain.h; DESIGN.md
// "Ground filter")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_ground_default_params(o3dr_ground_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);  // cell_size and the box: no usable default
    p->max_window_radius = 16, p->window_base = 2, p->exponential = 1;  // pcl::ProgressiveMorphologicalFilter's defaults
    p->slope = 0.7, p->initial_distance = 0.15, p->max_distance = 10.0;
}

// the parameters in the struct's order (whole: with the box and fill_radius), then the schedule of the contract's step 3
static int ground_schedule(const o3dr_ground_params* p, bool whole, float* inv, int32_t radii[16], float thr[16], int32_t* n_iter)
{
    CHK(frame_cell_size(p->cell_size, inv));
    if (whole) CHK(box_check(p->cx0, p->cy0, p->width, p->height));
    if (p->max_window_radius < 1 || p->max_window_radius > O3DR_GROUND_MAX_WINDOW_RADIUS)
        return fail(O3DR_ERR_INVALID_ARG, "max_window_radius must be in 1..128");
    if (p->window_base < (p->exponential ? 2 : 1))
        return fail(O3DR_ERR_INVALID_ARG, "window_base must be >= 2 (exponential) or >= 1 (linear)");
    if (!(std::isfinite(p->slope) && p->slope >= 0.0)) return fail(O3DR_ERR_INVALID_ARG, "slope must be finite and >= 0");
    if (!(std::isfinite(p->initial_distance) && p->initial_distance >= 0.0))
        return fail(O3DR_ERR_INVALID_ARG, "initial_distance must be finite and >= 0");
    if (!(std::isfinite(p->max_distance) && p->max_distance >= 0.0)) return fail(O3DR_ERR_INVALID_ARG, "max_distance must be finite and >= 0");
    if (whole && (p->fill_radius < 0 || p->fill_radius > O3DR_RASTER_MAX_FILL_RADIUS))
        return fail(O3DR_ERR_INVALID_ARG, "fill_radius must be in 0..32");
    int n = 0;
    int64_t r = p->exponential ? 1 : p->window_base, prev = 0;
    while (n < O3DR_GROUND_MAX_ITERATIONS && r <= p->max_window_radius) {
        const double t = n == 0 ? p->initial_distance : p->slope * ((double)(2 * (r - prev)) * p->cell_size) + p->initial_distance;
        radii[n] = (int32_t)r;
        thr[n] = (float)std::min(t, p->max_distance);
        ++n;
        prev = r;
        r = p->exponential ? r * p->window_base : r + p->window_base;
    }
    if (n == 0) return fail(O3DR_ERR_INVALID_ARG, "the window schedule has no iteration (window_base > max_window_radius)");
    *n_iter = n;
    return O3DR_OK;
}

extern "C" int o3dr_ground_schedule(const o3dr_ground_params* p, int32_t radii[16], float thresholds[16], int32_t* n_iterations)
{
    if (radii) memset(radii, 0, 16 * sizeof(int32_t));
    if (thresholds) memset(thresholds, 0, 16 * sizeof(float));
    if (n_iterations) *n_iterations = 0;
    if (!p || !radii || !thresholds || !n_iterations) return fail(O3DR_ERR_INVALID_ARG, "params / radii / thresholds / n_iterations is NULL");
    int32_t r[16] = {0};
    float t[16] = {0.f}, inv;
    int32_t n = 0;
    CHK(ground_schedule(p, false, &inv, r, t, &n));
    memcpy(radii, r, sizeof r);
    memcpy(thresholds, t, sizeof t);
    *n_iterations = n;
    return O3DR_OK;
}

static int ground_filter(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, const o3dr_ground_params* p, const o3dr_ground_outputs* out,
                         Outputs& outs, o3dr_ground_result* res, int32_t mem)
{
    if (!p) return fail(O3DR_ERR_INVALID_ARG, "params is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    GroundArgs a;
    memset(&a, 0, sizeof a);
    RasterArgs& r = a.r;
    float inv;
    CHK(ground_schedule(p, true, &inv, a.radius, a.thr, &a.n_iter));
    CHK(nn_check_cloud(n, cloud, kMeshCloudMax));
    c->place_ub = -1;
    r.select = O3DR_RASTER_BOTTOM, r.R = p->fill_radius;
    r.cell_size = p->cell_size;
    GroundFlags* f;
    CHK(op_flags(c, &f));
    const int32_t box[4] = {p->cx0, p->cy0, p->width, p->height};
    CellFlags h;
    CHK(raster_frame(c, cloud, n, mem, inv, box, &f->cell, &h, &r.f));
    int64_t cells;
    CHK(box_limit(r.f, &cells));
    const int64_t parts = ground_parts(a);
    float* dtm_tmp = nullptr;  // the point pass reads the DTM and the states: scratch when the caller does not ask for them
    uint8_t* state_tmp = nullptr;
    CHK(outs.stage(c));
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(r.f.part, (size_t)parts * kPartWords);
        w.take(r.win, (size_t)cells);
        w.take(a.zl, (size_t)cells);
        w.take(a.t1, (size_t)cells);
        w.take(a.t2, (size_t)cells);
        w.take(a.run, (size_t)cells);
        if (r.R > 0) w.take(r.col, (size_t)cells);
        if (!(out && out->dtm)) w.take(dtm_tmp, (size_t)cells);
        if (!(out && out->cell_state)) w.take(state_tmp, (size_t)cells);
    }));
    a.counters = f->counters;
    if (out) {
        a.ground = outs.dev(out->ground), a.hag = outs.dev(out->height_above_ground);
        r.height_map = outs.dev(out->dtm), a.state = outs.dev(out->cell_state);
    }
    if (!r.height_map) r.height_map = dtm_tmp;
    if (!a.state) a.state = state_tmp;
    launch_ground(&c->prof, c->stream, a);
    HIPCHK(hipGetLastError());
    uint32_t cnt[kGroundCounterWords];
    HIPCHK(hipMemcpyAsync(cnt, f->counters, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (res) {
        res->cx0 = p->cx0, res->cy0 = p->cy0, res->width = p->width, res->height = p->height;
        res->n_inside = cnt[0], res->n_outside = cnt[1];
        res->n_ground_cells = cnt[4], res->n_dtm_filled = cnt[5], res->n_dtm_empty = cnt[6];
        res->n_ground_points = cnt[12];
        res->n_iterations = a.n_iter;
        res->n_occupied = res->n_ground_cells;
        for (int k = 0; k < a.n_iter; ++k) res->n_occupied += (res->n_removed[k] = cnt[16 + 4 * k]);
    }
    return O3DR_OK;
}

extern "C" int o3dr_ground_filter(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, const o3dr_ground_params* p,
                                  const o3dr_ground_outputs* out, o3dr_ground_result* res, int32_t mem)
{
    Outputs outs{mem};
    const int64_t cells = p ? box_cells(p->width, p->height) : 0;
    if (out) {
        outs.add(out->ground, cloud_points(n, kMeshCloudMax));
        outs.add(out->height_above_ground, cloud_points(n, kMeshCloudMax));
        outs.add(out->dtm, cells);
        outs.add(out->cell_state, cells);
    }
    return raster_entry(c, outs, res, sizeof *res, [&] { return ground_filter(c, cloud, n, p, out, outs, res, mem); });
}

// -------------------------------------------------------------------------------------------------
// raster interpolation and raster sample (kernels/interpolate.inc; contract: include/o3dr_dem.h; DESIGN.md "Raster
// interpolation")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_interpolate_default_params(o3dr_interpolate_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);  // the raster's shape: no usable default
    p->smooth = 2;
}

struct InterpFlags {
    alignas(64) uint32_t counters[kInterpPartWords];  // InterpArgs::counters
    alignas(64) uint32_t bad;                         // an infinite input value
};

static int raster_interpolate(o3dr_ctx* c, const float* raster, const o3dr_interpolate_params* p, const o3dr_interpolate_outputs* out,
                              Outputs& outs, o3dr_interpolate_result* res, int32_t mem)
{
    if (!p || !raster || !out || !out->filled) return fail(O3DR_ERR_INVALID_ARG, "params / raster / outputs / outputs->filled is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (p->width < 1 || p->height < 1) return fail(O3DR_ERR_INVALID_ARG, "the raster needs width, height >= 1");
    if (p->smooth < 0 || p->smooth > O3DR_INTERPOLATE_MAX_SMOOTH) return fail(O3DR_ERR_INVALID_ARG, "smooth must be in 0..8");
    if (p->max_level < 0 || p->max_level > O3DR_INTERPOLATE_MAX_LEVELS - 1) return fail(O3DR_ERR_INVALID_ARG, "max_level must be in 0..31");
    const int64_t cells = (int64_t)p->width * p->height;
    if (cells > (int64_t)O3DR_RASTER_MAX_CELLS) return fail(O3DR_ERR_INVALID_ARG, "the raster holds more than 2^28 cells");
    c->place_ub = -1;
    InterpArgs a;
    memset(&a, 0, sizeof a);
    a.smooth = p->smooth, a.max_level = p->max_level;
    a.lv[0].W = p->width, a.lv[0].H = p->height;
    int64_t upper = 0;  // cells of the levels 1 .. L
    while (a.lv[a.L].W > 1 || a.lv[a.L].H > 1) {
        InterpLevel& v = a.lv[a.L + 1];
        v.W = (a.lv[a.L].W + 1) >> 1, v.H = (a.lv[a.L].H + 1) >> 1;
        v.off = upper;
        upper += (int64_t)v.W * v.H;
        ++a.L;
    }
    InterpFlags* f;
    CHK(op_flags(c, &f));
    const void* raster_d;
    CHK(stage_in(c, c->op[o3dr_ctx::OP_IN], raster, (size_t)cells * sizeof(float), mem, &raster_d));
    a.raster = (const float*)raster_d;
    CHK(outs.stage(c));
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(a.part, (size_t)interp_blocks(interp_push_tiles(a.lv[0], a.smooth)) * kInterpPartWords);
        w.take(a.cnt, (size_t)upper);
        w.take(a.val, (size_t)upper);
    }));
    a.counters = f->counters, a.bad = &f->bad;
    a.filled = outs.dev(out->filled), a.level = outs.dev(out->level);
    launch_interpolate(&c->prof, c->stream, a);
    HIPCHK(hipGetLastError());
    InterpFlags h;
    HIPCHK(hipMemcpyAsync(&h, f, sizeof h, hipMemcpyDeviceToHost, c->stream));
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h.bad) return fail(O3DR_ERR_INVALID_ARG, "the raster has an infinite value (a hole is a NaN)");
    if (res) {
        res->width = p->width, res->height = p->height, res->n_levels = a.L + 1;
        for (int l = 0; l < O3DR_INTERPOLATE_MAX_LEVELS; ++l) res->n_by_level[l] = h.counters[l];
        res->n_data = h.counters[0];
        res->n_filled = h.counters[O3DR_INTERPOLATE_MAX_LEVELS], res->n_empty = h.counters[O3DR_INTERPOLATE_MAX_LEVELS + 1];
    }
    return O3DR_OK;
}

extern "C" int o3dr_raster_interpolate(o3dr_ctx* c, const float* raster, const o3dr_interpolate_params* p,
                                       const o3dr_interpolate_outputs* out, o3dr_interpolate_result* res, int32_t mem)
{
    Outputs outs{mem};
    const int64_t cells = p ? box_cells(p->width, p->height) : 0;
    if (out) {
        outs.add(out->filled, cells);
        outs.add(out->level, cells);
    }
    return raster_entry(c, outs, res, sizeof *res, [&] { return raster_interpolate(c, raster, p, out, outs, res, mem); });
}

static int raster_sample(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, double cell_size, const int32_t box[4], const float* raster,
                         float* value, float* height_above, Outputs& outs, int64_t counts[3], int32_t mem)
{
    if (!raster) return fail(O3DR_ERR_INVALID_ARG, "raster is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    SampleArgs a;
    memset(&a, 0, sizeof a);
    float inv;
    CHK(frame_cell_size(cell_size, &inv));
    CHK(box_check(box[0], box[1], box[2], box[3]));
    CHK(nn_check_cloud(n, cloud, kMeshCloudMax));
    c->place_ub = -1;
    SampleFlags* f;
    CHK(op_flags(c, &f));
    CellFlags h;
    CHK(raster_frame(c, cloud, n, mem, inv, box, &f->cell, &h, &a.f));
    int64_t cells;
    CHK(box_limit(a.f, &cells));
    const void* raster_d;
    CHK(stage_in(c, c->op[o3dr_ctx::OP_IN], raster, (size_t)cells * sizeof(float), mem, &raster_d));
    a.raster = (const float*)raster_d;
    CHK(outs.stage(c));
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) { w.take(a.f.part, (size_t)std::max<int64_t>(raster_winner_parts(n), 1) * kPartWords); }));
    a.counters = f->counters;
    a.value = outs.dev(value), a.hag = outs.dev(height_above);
    launch_raster_sample(&c->prof, c->stream, a);
    HIPCHK(hipGetLastError());
    uint32_t cnt[4];
    HIPCHK(hipMemcpyAsync(cnt, f->counters, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (counts) counts[0] = cnt[0], counts[1] = cnt[1], counts[2] = cnt[2];
    return O3DR_OK;
}

extern "C" int o3dr_raster_sample(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, double cell_size, int32_t cx0, int32_t cy0,
                                  int32_t width, int32_t height, const float* raster, float* value, float* height_above,
                                  int64_t counts[3], int32_t mem)
{
    Outputs outs{mem};
    outs.add(value, cloud_points(n, kMeshCloudMax));
    outs.add(height_above, cloud_points(n, kMeshCloudMax));
    const int32_t box[4] = {cx0, cy0, width, height};
    return raster_entry(c, outs, counts, 3 * sizeof(int64_t),
                        [&] { return raster_sample(c, cloud, n, cell_size, box, raster, value, height_above, outs, counts, mem); });
}

// -------------------------------------------------------------------------------------------------
// contour lines (kernels/contour.inc; contract: include/o3dr_contour.h; DESIGN.md "Contour lines")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_contour_default_params(o3dr_contour_params* p)
{
    if (!p) return;
    memset(p, 0, sizeof *p);  // the raster's shape and the interval: no usable default
    p->cell_size = 1.0;
}

struct ContourFlags {
    alignas(64) uint32_t counters[kContourCounterWords];  // ContourArgs::counters
    alignas(64) uint32_t flags[2];                        // ContourArgs::flags
};

// The checks of both entry points, the staged raster, the count pass and its read-back: a.n_seg is not set, *n_seg is the
// 64-bit sum, h the counters.
static int contour_count(o3dr_ctx* c, const float* raster, const o3dr_contour_params* p, int32_t mem, ContourArgs& a, ContourFlags** f,
                         ContourFlags& h, int64_t* n_seg)
{
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (p->width < 1 || p->height < 1) return fail(O3DR_ERR_INVALID_ARG, "the raster needs width, height >= 1");
    if (!(std::isfinite(p->interval) && std::isfinite(p->base) && p->interval > 0.0))
        return fail(O3DR_ERR_INVALID_ARG, "interval must be finite and > 0, base finite");
    if (!(std::isfinite(p->cell_size) && p->cell_size > 0.0)) return fail(O3DR_ERR_INVALID_ARG, "cell_size must be finite and > 0");
    const int64_t cells = (int64_t)p->width * p->height;
    if (cells > (int64_t)O3DR_RASTER_MAX_CELLS) return fail(O3DR_ERR_INVALID_ARG, "the raster holds more than 2^28 cells");
    c->place_ub = -1;
    memset(&a, 0, sizeof a);
    a.W = p->width, a.H = p->height, a.cx0 = p->cx0, a.cy0 = p->cy0;
    a.interval = p->interval, a.base = p->base, a.cell_size = p->cell_size;
    const int64_t quads = (int64_t)(p->width - 1) * (p->height - 1);
    a.n_quads = (uint32_t)quads;
    CHK(op_flags(c, f));
    const void* raster_d;
    CHK(stage_in(c, c->op[o3dr_ctx::OP_IN], raster, (size_t)cells * sizeof(float), mem, &raster_d));
    a.raster = (const float*)raster_d;
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(a.kc, (size_t)cells);
        w.take(a.off, (size_t)std::max<int64_t>(quads, 1));
        w.take(a.part, (size_t)kContourMaxBlocks * kPartWords);
        w.take(a.scan_partial, (size_t)contour_scan_words(quads));
    }));
    a.counters = (*f)->counters, a.flags = (*f)->flags;
    launch_contour_count(&c->prof, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&h, *f, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h.flags[0]) return fail(O3DR_ERR_INVALID_ARG, "the raster has an infinite value (a hole is a NaN)");
    if (h.flags[1]) return fail(O3DR_ERR_INVALID_ARG, "a level index of the raster lies outside +-2^30 (the levels are too fine for its values)");
    *n_seg = (int64_t)(((uint64_t)h.counters[13] << 32) | h.counters[12]);
    return O3DR_OK;
}

extern "C" int o3dr_raster_contours_count(o3dr_ctx* c, const float* raster, const o3dr_contour_params* p, int64_t* n_segments, int32_t mem)
{
    if (n_segments) *n_segments = 0;
    const int rc = entered(c, [&] {
        if (!raster || !p || !n_segments) return fail(O3DR_ERR_INVALID_ARG, "raster / params / n_segments is NULL");
        ContourArgs a;
        ContourFlags *f, h;
        return contour_count(c, raster, p, mem, a, &f, h, n_segments);
    });
    if (rc != O3DR_OK && n_segments) *n_segments = 0;
    return rc;
}

static int raster_contours(o3dr_ctx* c, const float* raster, const o3dr_contour_params* p, const o3dr_contour_outputs* out, Outputs& outs,
                           o3dr_contour_result* res, int32_t mem)
{
    if (!raster || !p || !out || !res) return fail(O3DR_ERR_INVALID_ARG, "raster / params / outputs / result is NULL");
    ContourArgs a;
    ContourFlags *f, h;
    int64_t S = 0;
    CHK(contour_count(c, raster, p, mem, a, &f, h, &S));
    res->n_quads = h.counters[0], res->n_quads_crossed = h.counters[1], res->n_segments = S;
    if (S > 0) res->k_lo = (int32_t)(h.counters[2] ^ 0x80000000u), res->k_hi = (int32_t)(h.counters[3] ^ 0x80000000u);
    if (S > (int64_t)O3DR_CONTOUR_MAX_SEGMENTS) return fail(O3DR_ERR_CAPACITY, "the raster has more than 2^28 contour segments at this interval");
    ContourVertex* vertices = (ContourVertex*)out->vertices;
    if (S == 0) {
        outs.set_count(out->segments, 0), outs.set_count(out->lines, 0), outs.set_count(vertices, 0);
        return O3DR_OK;
    }
    a.n_seg = (uint32_t)S;
    CHK(carve(c, c->op[o3dr_ctx::OP_LATE], [&](Carve& w) {
        w.take(a.xy, (size_t)S);
        w.take(a.kn, (size_t)S);
        w.take(a.parent, (size_t)S);
        w.take(a.prev, (size_t)S);
        w.take(a.head, (size_t)S);
        w.take(a.cnt, (size_t)S);
        w.take(a.num, (size_t)S);
        w.take(a.beg, (size_t)S);
        w.take(a.jump[0], (size_t)S);
        w.take(a.jump[1], (size_t)S);
        w.take(a.part, (size_t)contour_blocks(S) * kPartWords);
        w.take(a.scan_partial, (size_t)contour_scan_words(S));
    }));
    launch_contour_lines(&c->prof, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&h, f, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int64_t n_lines = h.counters[8], n_vertices = h.counters[9];
    res->n_lines = n_lines, res->n_closed = h.counters[4], res->n_longest = h.counters[5], res->n_vertices = n_vertices;
    if ((out->segments && out->seg_capacity < S) || (out->lines && out->line_capacity < n_lines) ||
        (vertices && out->vertex_capacity < n_vertices))
        return fail(O3DR_ERR_CAPACITY, "seg_capacity / line_capacity / vertex_capacity is below what the raster's contours need");
    outs.set_count(out->segments, S), outs.set_count(out->lines, n_lines), outs.set_count(vertices, n_vertices);
    CHK(outs.stage(c));
    a.seg_out = outs.dev(out->segments), a.lines_out = outs.dev(out->lines), a.vertices = outs.dev(vertices);
    if (a.seg_out || a.lines_out || a.vertices) launch_contour_outputs(&c->prof, c->stream, a);
    HIPCHK(hipGetLastError());
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_raster_contours(o3dr_ctx* c, const float* raster, const o3dr_contour_params* p, const o3dr_contour_outputs* out,
                                    o3dr_contour_result* res, int32_t mem)
{
    if (res) memset(res, 0, sizeof *res);
    Outputs outs{mem};
    const int64_t bound = O3DR_CONTOUR_MAX_SEGMENTS;  // (a capacity above what any call writes is as good as that)
    if (out) {
        outs.add(out->segments, std::min(out->seg_capacity, bound));
        outs.add(out->lines, std::min(out->line_capacity, bound));
        outs.add((ContourVertex*)out->vertices, std::min(out->vertex_capacity, 2 * bound));
    }
    const int rc = entered(c, [&] { return raster_contours(c, raster, p, out, outs, res, mem); });
    if (rc != O3DR_OK && rc != O3DR_ERR_CAPACITY) {  // host outputs and the result zeroed on an error
        if (res) memset(res, 0, sizeof *res);
        outs.zero();
    }
    return rc;
}

// -------------------------------------------------------------------------------------------------
// Euclidean clustering: object labels and per-object records (kernels/cluster.inc; contract: include/o3dr_objects.h;
// DESIGN.md "Euclidean clustering")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_cluster_default_params(o3dr_cluster_params* p)
{
    if (!p) return;
    p->tolerance = 0.0;  // no usable default: the caller sets it
    p->min_size = 1, p->max_size = INT32_MAX;  // pcl::EuclideanClusterExtraction's defaults
}

struct ClusterFlags {
    alignas(64) uint32_t bad;  // non-finite; read back with the box
    float box6[6];
    alignas(64) uint32_t counters[kClusterCounterWords];  // ClusterArgs::counters
    alignas(64) unsigned long long n_pairs;
};
struct ClusterHead {  // the first words of ClusterFlags on the host
    uint32_t bad;
    float box6[6];
};
static_assert(offsetof(ClusterFlags, box6) == offsetof(ClusterHead, box6), "bad and the box are read back together");

static int cluster_euclidean(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, const o3dr_cluster_params* p, const o3dr_cluster_outputs* out,
                             o3dr_cluster* clusters, int64_t clusters_capacity, int64_t* n_clusters, Outputs& outs,
                             o3dr_cluster_result* res, int32_t mem)
{
    CHK(nn_check_cloud(n, cloud, kMeshCloudMax));
    if (!p) return fail(O3DR_ERR_INVALID_ARG, "params is NULL");
    if (!n_clusters) return fail(O3DR_ERR_INVALID_ARG, "n_clusters is NULL");
    if (clusters_capacity < 0 || (clusters_capacity > 0 && !clusters))
        return fail(O3DR_ERR_INVALID_ARG, "bad clusters / clusters_capacity");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    const double tol = p->tolerance;
    const float r2 = (float)(tol * tol);
    if (!(std::isfinite(tol) && tol > 0.0 && std::isfinite(r2) && r2 > 0.f))
        return fail(O3DR_ERR_INVALID_ARG, "tolerance must be finite and > 0 (and its square usable in fp32)");
    if (p->min_size < 1) return fail(O3DR_ERR_INVALID_ARG, "min_size must be >= 1");
    if (p->max_size < p->min_size) return fail(O3DR_ERR_INVALID_ARG, "max_size must be >= min_size");
    c->place_ub = -1;
    if (n == 0) return O3DR_OK;
    ClusterFlags* f;
    CHK(op_flags(c, &f));
    const o3dr_point* cloud_d = nullptr;
    ClusterHead h;
    memset(&h, 0, sizeof h);
    int used = 0;
    CHK(cloud_stage_finite(c, cloud, n, mem, &f->bad, &h.bad, sizeof h, &cloud_d, [&]() -> int {
        CHK(ws_ensure(c, 1, n, false));  // the cloud's box, before any grid work
        launch_set_counts(&c->prof, c->stream, c->ws.n_valid, (uint32_t)n, 1);
        used = launch_points_minmax(&c->prof, c->stream, cloud_d, 0, c->ws.n_valid, 1, n, c->ws.mm_stride, c->ws.mm);
        launch_bbox(&c->prof, c->stream, c->ws.mm, used, f->box6);
        return O3DR_OK;
    }));
    for (int k = 0; k < 3; ++k)
        if (!((double)h.box6[3 + k] - (double)h.box6[k] < 32768.0))
            return fail(O3DR_ERR_INVALID_ARG, "a side of the cloud's bounding box is 32768 m or more");
    // The grid is built from the min/max slots and the count taken above: ws_ensure(c, 1, n, false) in front of them has the
    // arguments of the one inside the build, so ws_block is not carved again in between, and nothing else has run in it.
    SearchGrid grid;
    CHK(search_grid_build(c, cloud_d, n, O3DR_MEM_DEVICE, used, &grid));
    ClusterArgs a;
    memset(&a, 0, sizeof a);
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(a.parent, (size_t)n);
        w.take(a.cnt, (size_t)n);
        w.take(a.num, (size_t)n);
        w.take(a.beg, (size_t)n);
        w.take(a.part, (size_t)cluster_blocks(n) * kPartWords);
    }));
    a.n = (uint32_t)n;
    a.grid = grid;
    a.r2 = r2;
    a.pad_r = grid_pad_radius(tol);
    a.min_size = p->min_size, a.max_size = p->max_size;
    a.counters = f->counters, a.n_pairs = &f->n_pairs;
    launch_cluster_link(&c->prof, c->stream, c->ws, a);
    HIPCHK(hipGetLastError());
    uint32_t cnt[kClusterCounterWords];
    unsigned long long pairs = 0;
    HIPCHK(hipMemcpyAsync(cnt, f->counters, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&pairs, &f->n_pairs, sizeof pairs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int64_t K = cnt[8], n_clustered = cnt[9];
    *n_clusters = K;
    if (clusters && K > clusters_capacity) return fail(O3DR_ERR_CAPACITY, "clusters_capacity is below the cluster count");
    outs.set_count(clusters, K);
    if (out) outs.set_count(out->indices, n_clustered);
    CHK(outs.stage(c));
    if (out) a.label = outs.dev(out->label), a.raw = outs.dev(out->raw), a.size = outs.dev(out->size), a.indices = outs.dev(out->indices);
    a.rec = K > 0 ? outs.dev(clusters) : nullptr;
    if (a.rec)
        CHK(carve(c, c->op[o3dr_ctx::OP_LATE], [&](Carve& w) {
            w.take(a.box_lo, (size_t)K * 3);
            w.take(a.box_hi, (size_t)K * 3);
            w.take(a.sums, (size_t)K * 3);
        }));
    launch_cluster_outputs(&c->prof, c->stream, c->ws, a, (uint32_t)K, (uint32_t)n_clustered);
    HIPCHK(hipGetLastError());
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (res) {
        res->n_components = cnt[0], res->n_clusters = K, res->n_too_small = cnt[1], res->n_too_large = cnt[2];
        res->n_clustered_points = n_clustered, res->n_rejected_points = n - n_clustered;
        res->largest = cnt[3];
        res->n_pairs = (int64_t)pairs;
    }
    return O3DR_OK;
}

extern "C" int o3dr_cluster_euclidean(o3dr_ctx* c, const o3dr_point* cloud, int64_t n, const o3dr_cluster_params* p,
                                      const o3dr_cluster_outputs* out, o3dr_cluster* clusters, int64_t clusters_capacity,
                                      int64_t* n_clusters, o3dr_cluster_result* res, int32_t mem)
{
    if (n_clusters) *n_clusters = 0;
    if (res) memset(res, 0, sizeof *res);
    Outputs outs{mem};
    const int64_t pts = cloud_points(n, kMeshCloudMax);
    if (out) {
        outs.add(out->label, pts);
        outs.add(out->raw, pts);
        outs.add(out->size, pts);
        outs.add(out->indices, pts);
    }
    outs.add(clusters, cloud_points(clusters_capacity, kMeshCloudMax));
    const int rc = entered(c, [&] {
        return cluster_euclidean(c, cloud, n, p, out, clusters, clusters_capacity, n_clusters, outs, res, mem);
    });
    if (rc != O3DR_OK && rc != O3DR_ERR_CAPACITY) {  // host outputs zeroed on error
        if (n_clusters) *n_clusters = 0;
        outs.zero();
    }
    if (rc != O3DR_OK && res) memset(res, 0, sizeof *res);
    return rc;
}

// -------------------------------------------------------------------------------------------------
// feature matching: Hamming 2-NN, index-aligned 3-D keypoints, batched rigid fit (kernels/match.inc; DESIGN.md
// "Feature matching")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_match_default_params(o3dr_match_params* p)
{
    if (!p) return;
    p->ratio = 0.5f;       // the reference's ratio test
    p->max_distance = 40;  // and its distance gate
}

// work items (waves) the chunk size aims at: enough to fill 256 CUs several times over
constexpr uint64_t kMatchTargetItems = 8192;

// ---- the checks the feature-pose entry points share; every caller keeps its own texts and limits ----
// row offsets of n sets / frames: `name` is the array's name in the text
static int offsets_check(const int64_t* off, int32_t n, const char* name)
{
    if (off[0] < 0) return fail(O3DR_ERR_INVALID_ARG, (std::string(name) + "[0] must be >= 0").c_str());
    for (int32_t s = 0; s < n; ++s)
        if (off[s + 1] < off[s]) return fail(O3DR_ERR_INVALID_ARG, (std::string(name) + " must not decrease").c_str());
    return O3DR_OK;
}

static int match_params_check(float ratio, int32_t max_distance)
{
    if (!(std::isfinite(ratio) && ratio > 0.f)) return fail(O3DR_ERR_INVALID_ARG, "ratio must be finite and > 0");
    if (max_distance < 0 || max_distance > 257) return fail(O3DR_ERR_INVALID_ARG, "max_distance must be in [0, 257]");
    return O3DR_OK;
}

// the pool of the chain and the graph: descriptors and 3-D keypoints, row for row
static int feature_pool_check(const uint8_t* desc, const o3dr_point* kp3, const int64_t* off, int32_t n_frames)
{
    CHK(offsets_check(off, n_frames, "offsets"));
    const int64_t pool = off[n_frames] - off[0];
    if (pool > (int64_t)INT32_MAX) return fail(O3DR_ERR_INVALID_ARG, "more than 2^31-1 rows");
    if (pool > 0 && (!desc || !kp3)) return fail(O3DR_ERR_INVALID_ARG, "desc / kp3 is NULL");
    return O3DR_OK;
}

static int chain_status_check(const int32_t* status, int32_t n)
{
    for (int32_t f = 0; f < n; ++f)
        if (status[f] < O3DR_CHAIN_ANCHOR || status[f] > O3DR_CHAIN_RMS) return fail(O3DR_ERR_INVALID_ARG, "status_in holds a value outside O3DR_CHAIN_*");
    return O3DR_OK;
}

// the RANSAC sampler's key of the pair (query frame i, train frame j)
static inline uint64_t pair_key(int32_t i, int32_t j) { return ((uint64_t)(uint32_t)i << 32) | (uint64_t)(uint32_t)j; }

// the pair table of a call (c->mt_tab_h; the pairs are checked) and its totals
struct MatchPlan {
    uint64_t chunk, items, rec, part;  // train rows per chunk; work items, records and partial slots of the call
};
static MatchPlan match_plan(o3dr_ctx* c, const int64_t* off, const int32_t* pairs, int64_t n_pairs)
{
    uint64_t work = 0;  // sum of ceil(nq / 64) nt: it sizes the chunk
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int32_t qs = pairs[2 * k], ts = pairs[2 * k + 1];
        work += ((uint64_t)(off[qs + 1] - off[qs]) + kWave - 1) / kWave * (uint64_t)(off[ts + 1] - off[ts]);
    }
    uint64_t chunk = (work + kMatchTargetItems - 1) / kMatchTargetItems;
    chunk = (chunk + kWave - 1) / kWave * kWave;
    if (chunk < (uint64_t)kWave) chunk = kWave;
    if (chunk > kMatchMaxChunk) chunk = kMatchMaxChunk;
    std::vector<MatchPair>& tab = c->mt_tab_h;
    tab.resize((size_t)n_pairs);
    uint64_t items = 0, rec = 0, part = 0;
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int32_t qs = pairs[2 * k], ts = pairs[2 * k + 1];
        MatchPair& P = tab[(size_t)k];
        P.qbase = (uint32_t)(off[qs] - off[0]);
        P.nq = (uint32_t)(off[qs + 1] - off[qs]);
        P.tbase = (uint32_t)(off[ts] - off[0]);
        P.nt = (uint32_t)(off[ts + 1] - off[ts]);
        P.chunks = (uint32_t)(((uint64_t)P.nt + chunk - 1) / chunk);
        P.qwaves = (P.nq + kWave - 1) / kWave;
        P.item0 = items;
        P.rec0 = rec;
        P.part0 = part;
        items += (uint64_t)P.qwaves * P.chunks;
        rec += P.nq;
        part += (uint64_t)P.nq * P.chunks;
    }
    return MatchPlan{chunk, items, rec, part};
}

// launch_match's arguments for a planned call: the staged pool, the parameters, where the records and the mask go
static MatchArgs match_args(const MatchPlan& plan, const void* desc_d, int64_t n_pairs, float ratio, int32_t max_distance, uint4* rec,
                            uint8_t* good)
{
    return MatchArgs{(const uint4*)desc_d, (uint32_t)n_pairs, (uint32_t)plan.chunk, plan.items, plan.rec, rec, good, ratio,
                     (uint32_t)max_distance};
}

static int match_knn2(o3dr_ctx* c, const uint8_t* desc, const int64_t* off, int32_t n_sets, const int32_t* pairs, int64_t n_pairs,
                      const o3dr_match_params* p, o3dr_knn2* out, uint8_t* good, Outputs& outs, int64_t out_capacity, int64_t* n_out,
                      int32_t mem)
{
    if (!n_out) return fail(O3DR_ERR_INVALID_ARG, "n_out is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    o3dr_match_params prm;
    o3dr_match_default_params(&prm);
    if (p) prm = *p;
    CHK(match_params_check(prm.ratio, prm.max_distance));
    if (n_sets < 0 || n_pairs < 0 || !off || (n_pairs > 0 && !pairs)) return fail(O3DR_ERR_INVALID_ARG, "bad sets / pairs");
    if (n_pairs > (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "too many pairs");
    CHK(offsets_check(off, n_sets, "desc_offsets"));
    const int64_t pool = off[n_sets] - off[0];
    if (pool > (int64_t)0xffffffffLL) return fail(O3DR_ERR_INVALID_ARG, "more than 2^32-1 descriptor rows");
    if (pool > 0 && !desc) return fail(O3DR_ERR_INVALID_ARG, "desc is NULL");
    uint64_t n_rec = 0;
    for (int64_t k = 0; k < n_pairs; ++k) {
        const int32_t qs = pairs[2 * k], ts = pairs[2 * k + 1];
        if (qs < 0 || qs >= n_sets || ts < 0 || ts >= n_sets) return fail(O3DR_ERR_INVALID_ARG, "a pair names a set outside [0, n_sets)");
        n_rec += (uint64_t)(off[qs + 1] - off[qs]);
    }
    *n_out = (int64_t)n_rec;
    if ((int64_t)n_rec > out_capacity) return fail(O3DR_ERR_CAPACITY, "out_capacity is below the record count");
    if (n_rec > 0 && !out) return fail(O3DR_ERR_INVALID_ARG, "out is NULL");
    if (n_rec == 0) return O3DR_OK;
    // the pair table, the chunk size and the totals
    const MatchPlan plan = match_plan(c, off, pairs, n_pairs);
    const std::vector<MatchPair>& tab = c->mt_tab_h;
    const void* desc_d = nullptr;
    if (pool > 0) CHK(stage_in(c, c->op[o3dr_ctx::OP_IN], desc + 32 * off[0], (size_t)pool * 32, mem, &desc_d));
    MatchPair* tab_d;
    uint2* part_d;
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(tab_d, tab.size());
        w.take(part_d, (size_t)(plan.part ? plan.part : 1));
    }));
    HIPCHK(hipMemcpyAsync(tab_d, tab.data(), tab.size() * sizeof(MatchPair), hipMemcpyHostToDevice, c->stream));
    outs.set_count(out, (int64_t)n_rec);
    outs.set_count(good, (int64_t)n_rec);
    CHK(outs.stage(c));  // records, then the mask
    const MatchArgs a = match_args(plan, desc_d, n_pairs, prm.ratio, prm.max_distance, (uint4*)outs.dev(out), outs.dev(good));
    launch_match(&c->prof, c->stream, a, tab_d, part_d);
    HIPCHK(hipGetLastError());
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_match_knn2_hamming(o3dr_ctx* c, const uint8_t* desc, const int64_t* desc_offsets, int32_t n_sets, const int32_t* pairs,
                                       int64_t n_pairs, const o3dr_match_params* p, o3dr_knn2* out, uint8_t* good, int64_t out_capacity,
                                       int64_t* n_out, int32_t mem)
{
    if (n_out) *n_out = 0;
    Outputs outs{mem};
    outs.add(out, out_capacity);
    outs.add(good, out_capacity);
    const int rc = entered(c, [&] { return match_knn2(c, desc, desc_offsets, n_sets, pairs, n_pairs, p, out, good, outs, out_capacity, n_out, mem); });
    if (rc != O3DR_OK && rc != O3DR_ERR_CAPACITY) {  // host outputs zeroed on error
        if (n_out) *n_out = 0;
        outs.zero();
    }
    return rc;
}

static int keypoints_3d(o3dr_ctx* c, const uint8_t* disp, int64_t disp_frame_stride, int64_t disp_pitch, const uint8_t* bgr,
                        int64_t bgr_frame_stride, int64_t bgr_pitch, int32_t rows, int32_t cols, const float* poses, int32_t n_frames,
                        const float* kp_xy, const int64_t* kp_offsets, o3dr_point* out, Outputs& outs, int64_t out_capacity, int64_t* n_out,
                        int32_t mem)
{
    if (!n_out) return fail(O3DR_ERR_INVALID_ARG, "n_out is NULL");
    if (!c->has_Q) return fail(O3DR_ERR_NOT_CONFIGURED, "o3dr_set_camera has not been called");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (n_frames < 0 || (n_frames > 0 && !kp_offsets)) return fail(O3DR_ERR_INVALID_ARG, "bad frame list");
    if (n_frames == 0) return O3DR_OK;
    const uint8_t* bgr_chk = bgr ? bgr : disp;  // (check_images wants both; without bgr only the disparities are read)
    CHK(check_images(c, disp, disp_pitch, bgr_chk, bgr ? bgr_pitch : 3 * (int64_t)cols, rows, cols, disp_frame_stride));
    if (disp_frame_stride < (int64_t)rows * disp_pitch || (bgr && bgr_frame_stride < (int64_t)rows * bgr_pitch))
        return fail(O3DR_ERR_INVALID_ARG, "frame stride smaller than a frame");
    CHK(offsets_check(kp_offsets, n_frames, "kp_offsets"));
    const int64_t n_kp = kp_offsets[n_frames] - kp_offsets[0];
    if (n_kp >= (int64_t)INT32_MAX) return fail(O3DR_ERR_INVALID_ARG, "too many keypoints");
    *n_out = n_kp;
    if (n_kp > out_capacity) return fail(O3DR_ERR_CAPACITY, "out_capacity is below the keypoint count");
    if (n_kp == 0) return O3DR_OK;
    if (!kp_xy || !out) return fail(O3DR_ERR_INVALID_ARG, "kp_xy / out is NULL");
    const int64_t last_d = (int64_t)(n_frames - 1) * disp_frame_stride + (int64_t)rows * disp_pitch;
    const int64_t last_b = bgr ? (int64_t)(n_frames - 1) * bgr_frame_stride + (int64_t)rows * bgr_pitch : 0;
    const void *disp_d, *bgr_d = nullptr, *poses_d = nullptr, *kp_d;
    CHK(stage_in(c, c->st_disp, disp, (size_t)last_d, mem, &disp_d));
    if (bgr) CHK(stage_in(c, c->st_bgr, bgr, (size_t)last_b, mem, &bgr_d));
    if (poses) CHK(stage_in(c, c->st_poses, poses, (size_t)n_frames * 16 * sizeof(float), mem, &poses_d));
    CHK(stage_in(c, c->st_kp, kp_xy + 2 * kp_offsets[0], (size_t)n_kp * 2 * sizeof(float), mem, &kp_d));
    std::vector<int32_t> kp_rel((size_t)n_frames + 1);
    for (int32_t f = 0; f <= n_frames; ++f) kp_rel[f] = (int32_t)(kp_offsets[f] - kp_offsets[0]);
    HIPCHK(hipStreamSynchronize(c->stream));  // an earlier call's launches may still read the offsets
    CHK(dev_ensure(c, c->st_kpoff, kp_rel.size() * sizeof(int32_t)));
    HIPCHK(hipMemcpy(c->st_kpoff.p, kp_rel.data(), kp_rel.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    const uint8_t* dsp = (const uint8_t*)disp_d;
    int64_t dsp_pitch = disp_pitch, dsp_fstride = disp_frame_stride;
    CHK(maybe_blur(c, &dsp, &dsp_pitch, &dsp_fstride, rows, cols, n_frames));
    const GridShape g = grid_shape(c->params, rows, cols);
    ReprojectArgs a;
    fill_args(c, a, dsp, dsp_pitch, dsp_fstride, (const uint8_t*)bgr_d, bgr_pitch, bgr_frame_stride, rows, cols, g, 0);
    if (poses) {
        a.xf_mode = 2;
        a.poses = (const float*)poses_d;
    }
    outs.set_count(out, n_kp);
    CHK(outs.stage(c));
    launch_keypoints_3d(&c->prof, c->stream, a, (const float*)kp_d, (const int32_t*)c->st_kpoff.p, n_frames, (int)n_kp, outs.dev(out));
    HIPCHK(hipGetLastError());
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_keypoints_3d(o3dr_ctx* c, const uint8_t* disp, int64_t disp_frame_stride, int64_t disp_pitch, const uint8_t* bgr,
                                 int64_t bgr_frame_stride, int64_t bgr_pitch, int32_t rows, int32_t cols, const float* poses,
                                 int32_t n_frames, const float* kp_xy, const int64_t* kp_offsets, o3dr_point* out, int64_t out_capacity,
                                 int64_t* n_out, int32_t mem)
{
    if (n_out) *n_out = 0;
    Outputs outs{mem};
    outs.add(out, out_capacity);
    const int rc = entered(c, [&] { return keypoints_3d(c, disp, disp_frame_stride, disp_pitch, bgr, bgr_frame_stride, bgr_pitch, rows, cols,
                                                        poses, n_frames, kp_xy, kp_offsets, out, outs, out_capacity, n_out, mem); });
    if (rc != O3DR_OK && rc != O3DR_ERR_CAPACITY) {
        if (n_out) *n_out = 0;
        outs.zero();
    }
    return rc;
}

// the index-aligned point pairs of the two rigid operators, as the kernels read them: a host call's src / tgt / mask go to
// OP_IN (a NULL mask stays NULL: its slot only keeps the layout the same)
static int stage_point_pairs(o3dr_ctx* c, const o3dr_point* src, const o3dr_point* tgt, const uint8_t* mask, int64_t n, int32_t mem,
                             const o3dr_point*& src_d, const o3dr_point*& tgt_d, const uint8_t*& mask_d)
{
    src_d = src, tgt_d = tgt, mask_d = mask;
    if (mem != O3DR_MEM_HOST) return O3DR_OK;
    CHK(carve(c, c->op[o3dr_ctx::OP_IN], [&](Carve& w) {
        w.take(src_d, (size_t)n);
        w.take(tgt_d, (size_t)n);
        w.take(mask_d, (size_t)n + 1);
    }));
    if (n > 0) {
        HIPCHK(hipMemcpyAsync((void*)src_d, src, (size_t)n * sizeof(o3dr_point), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync((void*)tgt_d, tgt, (size_t)n * sizeof(o3dr_point), hipMemcpyHostToDevice, c->stream));
        if (mask) HIPCHK(hipMemcpyAsync((void*)mask_d, mask, (size_t)n, hipMemcpyHostToDevice, c->stream));
    }
    if (!mask) mask_d = nullptr;
    return O3DR_OK;
}

// the segment table of the two rigid operators: every segment is checked against [0, n] and the operator's own limit, then
// fill(s, first point, points) writes the operator's record
template <class Fill>
static int segments_walk(const int64_t* seg_offsets, int32_t n_segs, int64_t n, int64_t limit, const char* limit_text, Fill&& fill)
{
    for (int32_t s = 0; s < n_segs; ++s) {
        const int64_t a0 = seg_offsets ? seg_offsets[s] : 0, a1 = seg_offsets ? seg_offsets[s + 1] : n;
        if (a0 < 0 || a1 < a0 || a1 > n) return fail(O3DR_ERR_INVALID_ARG, "seg_offsets must not decrease and stay within [0, n]");
        if (a1 - a0 > limit) return fail(O3DR_ERR_INVALID_ARG, limit_text);
        CHK(fill(s, (uint64_t)a0, (uint32_t)(a1 - a0)));
    }
    return O3DR_OK;
}

static int rigid_transform(o3dr_ctx* c, const o3dr_point* src, const o3dr_point* tgt, int64_t n, const int64_t* seg_offsets, int32_t n_segs,
                           const uint8_t* mask, o3dr_rigid_result* res, int32_t mem)
{
    if (!res) return fail(O3DR_ERR_INVALID_ARG, "res is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (n < 0 || (n > 0 && (!src || !tgt))) return fail(O3DR_ERR_INVALID_ARG, "bad src / tgt / n");
    if (n_segs < 1) return fail(O3DR_ERR_INVALID_ARG, "n_segs must be >= 1");
    if (!seg_offsets && n_segs != 1) return fail(O3DR_ERR_INVALID_ARG, "seg_offsets is NULL with n_segs != 1");
    std::vector<RigidSeg>& seg = c->rg_seg_h;
    seg.resize((size_t)n_segs);
    uint64_t blocks = 0;
    CHK(segments_walk(seg_offsets, n_segs, n, (int64_t)0xffffffffLL, "a segment holds more than 2^32-1 points",
                      [&](int32_t s, uint64_t start, uint32_t len) {
                          seg[s] = RigidSeg{start, len, (uint32_t)blocks};
                          blocks += ((uint64_t)len + kRigidPoints - 1) / kRigidPoints;
                          return blocks > 0x7fffffffull ? fail(O3DR_ERR_INVALID_ARG, "too many points") : O3DR_OK;
                      }));
    for (int32_t s = 0; s < n_segs; ++s) {
        memset(&res[s], 0, sizeof res[s]);
        for (int k = 0; k < 16; ++k) res[s].T[k] = k % 5 == 0 ? 1.0 : 0.0;
        res[s].status = O3DR_RIGID_TOO_FEW;
    }
    RigidArgs a;
    memset(&a, 0, sizeof a);
    CHK(stage_point_pairs(c, src, tgt, mask, n, mem, a.src, a.tgt, a.mask));
    const size_t S = (size_t)n_segs;
    a.n_segs = (uint32_t)n_segs;
    a.n_blocks = (uint32_t)blocks;
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(a.seg, S);
        w.take(a.first, S);
        w.take(a.partial, (size_t)kRigidFields * (size_t)(blocks ? blocks : 1));
        w.take(a.rec, S * (kRigidFields + 1));
        w.take(a.c0, S * 3);
        w.take(a.T, S * 12);
    }));
    HIPCHK(hipMemcpyAsync((void*)a.seg, seg.data(), S * sizeof(RigidSeg), hipMemcpyHostToDevice, c->stream));
    launch_rigid(&c->prof, c->stream, a, false);
    HIPCHK(hipGetLastError());
    std::vector<double> rec(S * kRigidFields), c0(S * 3);
    HIPCHK(hipMemcpyAsync(rec.data(), a.rec, rec.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(c0.data(), a.c0, c0.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // the ICP's host Kabsch per segment (rigid_solve; res[s].T is the identity, so its bottom row stands)
    std::vector<double>& Th = c->rg_T_h;
    Th.assign(S * 12, 0.0);
    for (size_t s = 0; s < S; ++s) {
        const double* r = &rec[s * kRigidFields];
        res[s].n_used = (int64_t)r[RIGID_N];
        double T[12];
        if (r[RIGID_N] < 3.0) {
            res[s].status = O3DR_RIGID_TOO_FEW;
        } else if (!rigid_solve(r, &c0[3 * s], T)) {
            res[s].status = O3DR_RIGID_DEGENERATE;
        } else {
            res[s].status = O3DR_RIGID_OK;
            for (int k = 0; k < 12; ++k) res[s].T[k] = T[k];
        }
        for (int k = 0; k < 12; ++k) Th[12 * s + k] = res[s].T[k];
    }
    HIPCHK(hipMemcpyAsync((void*)a.T, Th.data(), S * 12 * 8, hipMemcpyHostToDevice, c->stream));
    launch_rigid(&c->prof, c->stream, a, true);
    HIPCHK(hipGetLastError());
    std::vector<double> d2(S);
    HIPCHK(hipMemcpyAsync(d2.data(), a.rec + S * kRigidFields, S * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t s = 0; s < S; ++s) res[s].rms = res[s].n_used > 0 ? std::sqrt(d2[s] / (double)res[s].n_used) : 0.0;
    return O3DR_OK;
}

extern "C" int o3dr_estimate_rigid_transform(o3dr_ctx* c, const o3dr_point* src, const o3dr_point* tgt, int64_t n,
                                             const int64_t* seg_offsets, int32_t n_segs, const uint8_t* mask, o3dr_rigid_result* res,
                                             int32_t mem)
{
    const int rc = entered(c, [&] { return rigid_transform(c, src, tgt, n, seg_offsets, n_segs, mask, res, mem); });
    if (rc != O3DR_OK && res && n_segs > 0) memset(res, 0, (size_t)n_segs * sizeof(o3dr_rigid_result));
    return rc;
}

// -------------------------------------------------------------------------------------------------
// robust rigid fit (kernels/ransac.inc; contract: include/o3dr.h "robust rigid fit", DESIGN.md "Robust fit")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_ransac_default_params(o3dr_ransac_params* p)
{
    if (!p) return;
    p->threshold = 0.05;
    p->seed = 0;
    p->iterations = 256;
    p->reserved = 0;
}

static int ransac_check(const o3dr_ransac_params& p)
{
    if (!(std::isfinite(p.threshold) && p.threshold > 0.0)) return fail(O3DR_ERR_INVALID_ARG, "the RANSAC threshold must be finite and > 0");
    if (p.iterations < 1 || p.iterations > O3DR_RANSAC_MAX_ITERATIONS) return fail(O3DR_ERR_INVALID_ARG, "RANSAC iterations must be in [1, 65536]");
    return O3DR_OK;
}

// one segment's record; `over` runs on by the candidates it may have past kRansacStage
static RansacSeg ransac_seg(uint64_t start, uint64_t key, uint32_t n, uint64_t& over)
{
    const RansacSeg g{start, key, over, n, 0};
    if (n > (uint32_t)kRansacStage) over += n - (uint32_t)kRansacStage;
    return g;
}

static int ransac_rigid(o3dr_ctx* c, const o3dr_point* src, const o3dr_point* tgt, int64_t n, const int64_t* seg_offsets, int32_t n_segs,
                        const uint8_t* mask, const uint64_t* seg_keys, const o3dr_ransac_params* p, uint8_t* inlier, Outputs& outs,
                        o3dr_ransac_result* res, int32_t mem)
{
    if (!res) return fail(O3DR_ERR_INVALID_ARG, "res is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (n < 0 || (n > 0 && (!src || !tgt || !inlier))) return fail(O3DR_ERR_INVALID_ARG, "bad src / tgt / inlier / n");
    if (n_segs < 1) return fail(O3DR_ERR_INVALID_ARG, "n_segs must be >= 1");
    if (!seg_offsets && n_segs != 1) return fail(O3DR_ERR_INVALID_ARG, "seg_offsets is NULL with n_segs != 1");
    o3dr_ransac_params prm;
    o3dr_ransac_default_params(&prm);
    if (p) prm = *p;
    CHK(ransac_check(prm));
    std::vector<RansacSeg>& seg = c->rs_seg_h;
    seg.resize((size_t)n_segs);
    uint64_t over = 0;
    CHK(segments_walk(seg_offsets, n_segs, n, (int64_t)INT32_MAX, "a segment holds more than 2^31-1 points",
                      [&](int32_t s, uint64_t start, uint32_t len) {
                          seg[s] = ransac_seg(start, seg_keys ? seg_keys[s] : (uint64_t)s, len, over);
                          return O3DR_OK;
                      }));
    c->place_ub = -1;
    RansacArgs a;
    memset(&a, 0, sizeof a);
    CHK(stage_point_pairs(c, src, tgt, mask, n, mem, a.src, a.tgt, a.mask));
    const size_t S = (size_t)n_segs;
    RansacSeg* seg_d;
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(seg_d, S);
        w.take(a.over, (size_t)over + 1);
        w.take(a.res, S);
    }));
    CHK(outs.stage(c));
    a.seg = seg_d;
    a.inlier = outs.dev(inlier);
    a.seed = prm.seed;
    a.thr2 = prm.threshold * prm.threshold;
    a.iterations = (uint32_t)prm.iterations;
    a.n_segs = (uint32_t)n_segs;
    HIPCHK(hipMemcpyAsync(seg_d, seg.data(), S * sizeof(RansacSeg), hipMemcpyHostToDevice, c->stream));
    // (bytes outside every segment are not the kernel's: a host output starts from zeros)
    if (mem == O3DR_MEM_HOST && n > 0) HIPCHK(hipMemsetAsync(a.inlier, 0, (size_t)n, c->stream));
    launch_ransac(&c->prof, c->stream, a, false);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(res, a.res, S * sizeof(o3dr_ransac_result), hipMemcpyDeviceToHost, c->stream));
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_ransac_rigid(o3dr_ctx* c, const o3dr_point* src, const o3dr_point* tgt, int64_t n, const int64_t* seg_offsets,
                                 int32_t n_segs, const uint8_t* mask, const uint64_t* seg_keys, const o3dr_ransac_params* p,
                                 uint8_t* inlier, o3dr_ransac_result* res, int32_t mem)
{
    Outputs outs{mem};
    outs.add(inlier, n > 0 ? n : 0);
    const int rc = entered(c, [&] { return ransac_rigid(c, src, tgt, n, seg_offsets, n_segs, mask, seg_keys, p, inlier, outs, res, mem); });
    if (rc != O3DR_OK) {  // host outputs zeroed on error
        outs.zero();
        if (res && n_segs > 0) memset(res, 0, (size_t)n_segs * sizeof(o3dr_ransac_result));
    }
    return rc;
}

// -------------------------------------------------------------------------------------------------
// The static stage the pose chain and the pose-graph refinement share: the pair table of a list of (query frame, train
// frame) pairs, the staged pool, one batched matching pass and, with RANSAC parameters, the filter of every pair in camera
// coordinates (keyed by its two frame numbers).  pair_stage_plan before the caller's OP_WORK layout, pair_stage_take inside
// it, pair_stage_run after the caller's own uploads.
// -------------------------------------------------------------------------------------------------
struct PairStage {
    MatchPlan plan;
    uint64_t over;               // candidates past kRansacStage, over all pairs
    const uint8_t* desc_d;       // the descriptors of the pool (staged for a host call)
    MatchedPairs m;              // what the stage leaves: the pool's keypoints, the table, plan.rec records and good bytes,
                                 // and the filter's bytes (nullptr without it)
    uint2* part_d;
    RansacSeg* rseg_d;
    uint32_t* over_d;
    uint8_t* inlier_d;           // plan.rec bytes, as the filter writes them
    o3dr_ransac_result* rres_d;  // one per pair (with the filter)
};

static int pair_stage_plan(o3dr_ctx* c, const uint8_t* desc, const int64_t* off, const o3dr_point* kp3, int32_t n_frames,
                           const int32_t* pl, int64_t n_pairs, bool robust, int32_t mem, PairStage& S)
{
    memset(&S, 0, sizeof S);
    S.plan = match_plan(c, off, pl, n_pairs);
    const std::vector<MatchPair>& tab = c->mt_tab_h;
    const int64_t pool = off[n_frames] - off[0];
    S.desc_d = desc ? desc + 32 * off[0] : nullptr;
    S.m.kp3 = kp3 ? kp3 + off[0] : nullptr;
    if (mem == O3DR_MEM_HOST) {
        CHK(carve(c, c->op[o3dr_ctx::OP_IN], [&](Carve& w) {
            w.take(S.desc_d, (size_t)pool * 32 + 1);
            w.take(S.m.kp3, (size_t)pool + 1);
        }));
        if (pool > 0) {
            HIPCHK(hipMemcpyAsync((void*)S.desc_d, desc + 32 * off[0], (size_t)pool * 32, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync((void*)S.m.kp3, kp3 + off[0], (size_t)pool * sizeof(o3dr_point), hipMemcpyHostToDevice, c->stream));
        }
    }
    // the RANSAC's segments: one per pair, keyed by its two frame numbers
    std::vector<RansacSeg>& rseg = c->rs_seg_h;
    rseg.clear();
    if (robust) {
        rseg.resize((size_t)n_pairs);
        for (size_t k = 0; k < (size_t)n_pairs; ++k) rseg[k] = ransac_seg(tab[k].rec0, pair_key(pl[2 * k], pl[2 * k + 1]), tab[k].nq, S.over);
    }
    return O3DR_OK;
}

static void pair_stage_take(o3dr_ctx* c, Carve& w, PairStage& S, bool robust)
{
    w.take(S.m.pairs, c->mt_tab_h.size() + 1);
    w.take(S.part_d, (size_t)S.plan.part + 1);
    w.take(S.m.rec, (size_t)S.plan.rec + 1);
    w.take(S.m.good, (size_t)S.plan.rec + 1);
    w.take(S.rseg_d, c->rs_seg_h.size() + 1);
    w.take(S.over_d, (size_t)S.over + 1);
    w.take(S.inlier_d, robust ? (size_t)S.plan.rec + 1 : 1);
    w.take(S.rres_d, c->rs_seg_h.size() + 1);
    S.m.inlier = robust ? S.inlier_d : nullptr;
}

// (the stage writes what S.m shows its readers as const: the table, the records and the mask)
static int pair_stage_run(o3dr_ctx* c, const PairStage& S, int64_t n_pairs, float ratio, int32_t max_distance, const o3dr_ransac_params* rp)
{
    const std::vector<MatchPair>& tab = c->mt_tab_h;
    if (n_pairs > 0) HIPCHK(hipMemcpyAsync((void*)S.m.pairs, tab.data(), tab.size() * sizeof(MatchPair), hipMemcpyHostToDevice, c->stream));
    if (S.plan.rec > 0) {
        const MatchArgs m = match_args(S.plan, S.desc_d, n_pairs, ratio, max_distance, const_cast<uint4*>(S.m.rec), const_cast<uint8_t*>(S.m.good));
        launch_match(&c->prof, c->stream, m, S.m.pairs, S.part_d);
        HIPCHK(hipGetLastError());
    }
    // the pairs' inlier masks, in camera coordinates: static like the matching, one workgroup per pair
    if (rp && n_pairs > 0) {
        const std::vector<RansacSeg>& rseg = c->rs_seg_h;
        RansacArgs g;
        memset(&g, 0, sizeof g);
        g.m = S.m;
        g.m.inlier = nullptr;  // (the kernel writes the mask: g.inlier)
        g.seg = S.rseg_d;
        g.over = S.over_d;
        g.inlier = S.inlier_d;
        g.res = S.rres_d;
        g.seed = rp->seed;
        g.thr2 = rp->threshold * rp->threshold;
        g.iterations = (uint32_t)rp->iterations;
        g.n_segs = (uint32_t)n_pairs;
        HIPCHK(hipMemcpyAsync(S.rseg_d, rseg.data(), rseg.size() * sizeof(RansacSeg), hipMemcpyHostToDevice, c->stream));
        launch_ransac(&c->prof, c->stream, g, true);
        HIPCHK(hipGetLastError());
    }
    return O3DR_OK;
}

// -------------------------------------------------------------------------------------------------
// pose chain (kernels/pose_chain.inc; contract: include/o3dr.h "pose chain", DESIGN.md "Pose chain")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_chain_default_params(o3dr_chain_params* p)
{
    if (!p) return;
    p->dist_nearby = 2.0;
    p->max_rms = HUGE_VAL;  // no gate
    p->range_width = 8;
    p->min_matches = 30;
    p->ratio = 0.5f;
    p->max_distance = 40;
}

static int pose_chain(o3dr_ctx* c, const uint8_t* desc, const int64_t* off, const o3dr_point* kp3, const float* prior, int32_t n_frames,
                      int32_t n_fixed, const float* poses_in, const int32_t* status_in, const o3dr_chain_params* p, float* poses_out,
                      o3dr_chain_frame* frames_out, Outputs& outs, int32_t* pairs_out, int64_t pairs_capacity, int64_t* n_pairs_out,
                      int32_t mem, const o3dr_ransac_params* rp, o3dr_ransac_result* ransac_out)
{
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (rp) CHK(ransac_check(*rp));
    o3dr_chain_params prm;
    o3dr_chain_default_params(&prm);
    if (p) prm = *p;
    if (!(std::isfinite(prm.dist_nearby) && prm.dist_nearby >= 0.0)) return fail(O3DR_ERR_INVALID_ARG, "dist_nearby must be finite and >= 0");
    if (prm.range_width < 1 || prm.range_width > O3DR_CHAIN_MAX_RANGE) return fail(O3DR_ERR_INVALID_ARG, "range_width must be in [1, 32]");
    if (prm.min_matches < 3) return fail(O3DR_ERR_INVALID_ARG, "min_matches must be >= 3");
    if (!(prm.max_rms > 0.0)) return fail(O3DR_ERR_INVALID_ARG, "max_rms must be > 0");
    CHK(match_params_check(prm.ratio, prm.max_distance));
    if (n_frames < 0 || n_fixed < 0 || n_fixed > n_frames) return fail(O3DR_ERR_INVALID_ARG, "0 <= n_fixed <= n_frames must hold");
    if (n_frames == 0) return O3DR_OK;
    if (!off || !prior || !poses_out || !frames_out) return fail(O3DR_ERR_INVALID_ARG, "offsets / prior_poses / poses_out / frames_out is NULL");
    if (n_fixed > 0 && (!poses_in || !status_in)) return fail(O3DR_ERR_INVALID_ARG, "poses_in / status_in is NULL with n_fixed > 0");
    CHK(feature_pool_check(desc, kp3, off, n_frames));
    CHK(chain_status_check(status_in, n_fixed));
    c->place_ub = -1;
    // 1. the static pair list (host, fp64)
    const size_t F = (size_t)n_frames;
    std::vector<int32_t>& pl = c->ch_pairs_h;
    std::vector<int32_t>& train = c->ch_train_h;
    std::vector<ChainFrameIn>& fr = c->ch_frames_h;
    pl.clear();
    train.clear();
    fr.resize(F);
    const double r2 = prm.dist_nearby * prm.dist_nearby;
    for (int32_t i = 0; i < n_frames; ++i) {
        ChainFrameIn& f = fr[(size_t)i];
        f.pair0 = (uint32_t)train.size();
        f.n_pairs = 0;
        f.qbase = (uint32_t)(off[i] - off[0]);
        f.nq = (uint32_t)(off[i + 1] - off[i]);
        if (i < n_fixed) continue;
        const double x = prior[16 * (size_t)i + 3], y = prior[16 * (size_t)i + 7], z = prior[16 * (size_t)i + 11];
        for (int32_t j = i - 1; j >= 0 && (int32_t)f.n_pairs < prm.range_width; --j) {
            const double dx = (double)prior[16 * (size_t)j + 3] - x, dy = (double)prior[16 * (size_t)j + 7] - y,
                         dz = (double)prior[16 * (size_t)j + 11] - z;
            if (!(((dx * dx + dy * dy) + dz * dz) <= r2)) continue;
            pl.push_back(i);
            pl.push_back(j);
            train.push_back(j);
            ++f.n_pairs;
        }
        if ((uint64_t)f.n_pairs * f.nq > (uint64_t)INT32_MAX) return fail(O3DR_ERR_INVALID_ARG, "a frame has more than 2^31-1 slots");
    }
    const int64_t n_pairs = (int64_t)train.size();
    if (n_pairs_out) *n_pairs_out = n_pairs;
    if (pairs_out && n_pairs > pairs_capacity) return fail(O3DR_ERR_CAPACITY, "pairs_capacity is below the pair count");
    if (pairs_out && n_pairs > 0) memcpy(pairs_out, pl.data(), (size_t)n_pairs * 2 * sizeof(int32_t));
    // history: records on the host, poses and statuses to the device
    std::vector<int32_t>& st_h = c->ch_status_h;
    st_h.assign(F, 0);
    for (int32_t f = 0; f < n_fixed; ++f) {
        o3dr_chain_frame& r = frames_out[f];
        memset(&r, 0, sizeof r);
        r.status = st_h[(size_t)f] = status_in[f];
        for (int k = 0; k < 12; ++k) r.T[k] = (double)poses_in[16 * (size_t)f + k];
    }
    // 2. staging and scratch
    PairStage S;
    CHK(pair_stage_plan(c, desc, off, kp3, n_frames, pl.data(), n_pairs, rp != nullptr, mem, S));
    int32_t *train_d, *status_d;
    ChainFrameIn* frames_d;
    float* prior_d;
    o3dr_chain_frame* out_d;
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        pair_stage_take(c, w, S, rp != nullptr);
        w.take(train_d, train.size() + 1);
        w.take(status_d, F);
        w.take(frames_d, F);
        w.take(prior_d, F * 16);
        w.take(out_d, F);
    }));
    CHK(outs.stage(c));
    float* poses_d = outs.dev(poses_out);
    if (n_pairs > 0) HIPCHK(hipMemcpyAsync(train_d, train.data(), train.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(frames_d, fr.data(), F * sizeof(ChainFrameIn), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(prior_d, prior, F * 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (n_fixed > 0) {
        HIPCHK(hipMemcpyAsync(status_d, st_h.data(), (size_t)n_fixed * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(poses_d, poses_in, (size_t)n_fixed * 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    }
    // 3. one batched matching pass (and the pairs' inlier masks), then the chain: one launch
    CHK(pair_stage_run(c, S, n_pairs, prm.ratio, prm.max_distance, rp));
    ChainArgs a;
    memset(&a, 0, sizeof a);
    a.m = S.m;
    a.pair_train = train_d;
    a.frames = frames_d;
    a.prior = prior_d;
    a.poses = poses_d;
    a.status = status_d;
    a.out = out_d;
    a.n_frames = (uint32_t)n_frames;
    a.n_fixed = (uint32_t)n_fixed;
    a.min_matches = (uint32_t)prm.min_matches;
    a.max_rms = prm.max_rms;
    launch_pose_chain(&c->prof, c->stream, a);
    HIPCHK(hipGetLastError());
    if (n_fixed < n_frames)
        HIPCHK(hipMemcpyAsync(frames_out + n_fixed, out_d + n_fixed, (size_t)(n_frames - n_fixed) * sizeof(o3dr_chain_frame),
                              hipMemcpyDeviceToHost, c->stream));
    if (rp && ransac_out && n_pairs > 0)
        HIPCHK(hipMemcpyAsync(ransac_out, S.rres_d, (size_t)n_pairs * sizeof(o3dr_ransac_result), hipMemcpyDeviceToHost, c->stream));
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_pose_chain_robust(o3dr_ctx* c, const uint8_t* desc, const int64_t* offsets, const o3dr_point* kp3,
                                      const float* prior_poses, int32_t n_frames, int32_t n_fixed, const float* poses_in,
                                      const int32_t* status_in, const o3dr_chain_params* p, float* poses_out, o3dr_chain_frame* frames_out,
                                      int32_t* pairs_out, int64_t pairs_capacity, int64_t* n_pairs_out, int32_t mem,
                                      const o3dr_ransac_params* rp, o3dr_ransac_result* ransac_out)
{
    if (n_pairs_out) *n_pairs_out = 0;
    if (!rp) ransac_out = nullptr;
    Outputs outs{mem};
    outs.add(poses_out, n_frames > 0 ? 16 * (int64_t)n_frames : 0);
    const int rc = entered(c, [&] {
        return pose_chain(c, desc, offsets, kp3, prior_poses, n_frames, n_fixed, poses_in, status_in, p, poses_out, frames_out, outs,
                          pairs_out, pairs_capacity, n_pairs_out, mem, rp, ransac_out);
    });
    if (rc != O3DR_OK && rc != O3DR_ERR_CAPACITY) {  // host outputs zeroed on error
        if (n_pairs_out) *n_pairs_out = 0;
        outs.zero();
        if (frames_out && n_frames > 0) memset(frames_out, 0, (size_t)n_frames * sizeof(o3dr_chain_frame));
        if (pairs_out && pairs_capacity > 0) memset(pairs_out, 0, (size_t)pairs_capacity * 2 * sizeof(int32_t));
        // (ransac_out's length is the pair count, an output of the call: it is not zeroed; its copy is the call's last but one)
    }
    return rc;
}

extern "C" int o3dr_pose_chain(o3dr_ctx* c, const uint8_t* desc, const int64_t* offsets, const o3dr_point* kp3, const float* prior_poses,
                               int32_t n_frames, int32_t n_fixed, const float* poses_in, const int32_t* status_in,
                               const o3dr_chain_params* p, float* poses_out, o3dr_chain_frame* frames_out, int32_t* pairs_out,
                               int64_t pairs_capacity, int64_t* n_pairs_out, int32_t mem)
{
    return o3dr_pose_chain_robust(c, desc, offsets, kp3, prior_poses, n_frames, n_fixed, poses_in, status_in, p, poses_out, frames_out,
                                  pairs_out, pairs_capacity, n_pairs_out, mem, nullptr, nullptr);
}

// -------------------------------------------------------------------------------------------------
// pose-graph refinement (kernels/pose_graph.inc; contract: include/o3dr.h "pose graph", DESIGN.md "Pose-graph refinement")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_refine_default_params(o3dr_refine_params* p)
{
    if (!p) return;
    p->prior_weight = 0.0;
    p->gn_iterations = 5;
    p->cg_iterations = 32;
    p->min_pair_matches = 3;
    p->ratio = 0.5f;
    p->max_distance = 40;
    p->reserved = 0;
}

static int pose_graph_refine(o3dr_ctx* c, const uint8_t* desc, const int64_t* off, const o3dr_point* kp3, int32_t n_frames,
                             const float* poses_in, const int32_t* status_in, const uint8_t* fixed, const float* prior, const int32_t* pairs,
                             int64_t n_pairs, const o3dr_refine_params* p, const o3dr_ransac_params* rp, float* poses_out,
                             o3dr_refine_frame* frames_out, o3dr_refine_edge* edges_out, o3dr_refine_result* res, Outputs& outs,
                             int32_t mem)
{
    if (!res) return fail(O3DR_ERR_INVALID_ARG, "res is NULL");
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (rp) CHK(ransac_check(*rp));
    o3dr_refine_params prm;
    o3dr_refine_default_params(&prm);
    if (p) prm = *p;
    if (prm.gn_iterations < 1 || prm.gn_iterations > O3DR_REFINE_MAX_GN) return fail(O3DR_ERR_INVALID_ARG, "gn_iterations must be in [1, 64]");
    if (prm.cg_iterations < 1 || prm.cg_iterations > O3DR_REFINE_MAX_CG) return fail(O3DR_ERR_INVALID_ARG, "cg_iterations must be in [1, 1024]");
    if (prm.min_pair_matches < 1) return fail(O3DR_ERR_INVALID_ARG, "min_pair_matches must be >= 1");
    if (!(std::isfinite(prm.prior_weight) && prm.prior_weight >= 0.0)) return fail(O3DR_ERR_INVALID_ARG, "prior_weight must be finite and >= 0");
    CHK(match_params_check(prm.ratio, prm.max_distance));
    if (n_frames < 0 || n_pairs < 0) return fail(O3DR_ERR_INVALID_ARG, "n_frames and n_pairs must be >= 0");
    memset(res, 0, sizeof *res);
    if (n_frames == 0) {
        if (n_pairs > 0) return fail(O3DR_ERR_INVALID_ARG, "a pair names a frame outside [0, n_frames)");
        return O3DR_OK;
    }
    if (!off || !poses_in || !status_in || !poses_out || !frames_out) return fail(O3DR_ERR_INVALID_ARG, "offsets / poses_in / status_in / poses_out / frames_out is NULL");
    if (n_pairs > 0 && !pairs) return fail(O3DR_ERR_INVALID_ARG, "pairs is NULL");
    if (n_pairs > (int64_t)INT32_MAX) return fail(O3DR_ERR_INVALID_ARG, "more than 2^31-1 pairs");
    if (prm.prior_weight > 0.0 && !prior) return fail(O3DR_ERR_INVALID_ARG, "prior_poses is NULL with prior_weight > 0");
    CHK(feature_pool_check(desc, kp3, off, n_frames));
    CHK(chain_status_check(status_in, n_frames));
    const size_t F = (size_t)n_frames, P = (size_t)n_pairs;
    {
        std::vector<uint64_t>& keys = c->gr_keys_h;
        keys.resize(P);
        for (size_t k = 0; k < P; ++k) {
            const int32_t i = pairs[2 * k], j = pairs[2 * k + 1];
            if (i < 0 || i >= n_frames || j < 0 || j >= n_frames) return fail(O3DR_ERR_INVALID_ARG, "a pair names a frame outside [0, n_frames)");
            if (i == j) return fail(O3DR_ERR_INVALID_ARG, "a pair names one frame twice");
            keys[k] = pair_key(i, j);
        }
        std::sort(keys.begin(), keys.end());
        if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return fail(O3DR_ERR_INVALID_ARG, "a pair is listed twice");
    }
    c->place_ub = -1;
    auto accepted = [&](int32_t f) { return status_in[f] <= O3DR_CHAIN_MATCHED; };
    std::vector<uint8_t>& ok_h = c->gr_ok_h;
    ok_h.resize(P);
    for (size_t k = 0; k < P; ++k) ok_h[k] = accepted(pairs[2 * k]) && accepted(pairs[2 * k + 1]) ? 1 : 0;
    // 1. matching (and the filter): the chain's stage.  2. the moments of every pair
    PairStage S;
    CHK(pair_stage_plan(c, desc, off, kp3, n_frames, pairs, n_pairs, rp != nullptr, mem, S));
    GraphMomArgs ma;
    memset(&ma, 0, sizeof ma);
    GraphArgs a;
    memset(&a, 0, sizeof a);
    uint8_t* ok_d;
    float *pin_d, *prior_d;
    GraphEdgeIn* edges_d;
    GraphFrameIn* frames_d;
    uint32_t* adj_d;
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        pair_stage_take(c, w, S, rp != nullptr);
        w.take(ok_d, P + 1);
        w.take(ma.mom, P * kGraphFields + 1);
        w.take(ma.counts, 2 * P + 1);
        w.take(pin_d, F * 16);
        w.take(prior_d, F * 16);
        w.take(edges_d, P + 1);      // (the edges are a subset of the pairs: sized before the counts are known)
        w.take(frames_d, F);
        w.take(adj_d, 2 * P + 1);
        w.take(a.state, F * 12);
        w.take(a.Hij, P * 36 + 1);
        w.take(a.ge, P * 12 + 1);
        w.take(a.Ee, P * 2 + 1);
        w.take(a.Hd, F * 72);
        w.take(a.vec, F * 30);
        w.take(a.frames_out, F);
        w.take(a.res, 1);
    }));
    CHK(outs.stage(c));
    if (P > 0) HIPCHK(hipMemcpyAsync(ok_d, ok_h.data(), P, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(pin_d, poses_in, F * 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (prior) HIPCHK(hipMemcpyAsync(prior_d, prior, F * 16 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    CHK(pair_stage_run(c, S, n_pairs, prm.ratio, prm.max_distance, rp));
    ma.m = S.m;
    ma.pair_ok = ok_d;
    ma.n_pairs = (uint32_t)n_pairs;
    launch_graph_moments(&c->prof, c->stream, ma);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t>& cnt = c->gr_counts_h;
    cnt.assign(2 * P + 1, 0u);
    if (P > 0) HIPCHK(hipMemcpyAsync(cnt.data(), ma.counts, 2 * P * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // (the first of the call's two)
    // 3. edges, roles and the adjacency
    std::vector<GraphEdgeIn>& ed = c->gr_edges_h;
    std::vector<GraphFrameIn>& fr = c->gr_frames_h;
    std::vector<uint32_t>& adj = c->gr_adj_h;
    ed.clear();
    fr.assign(F, GraphFrameIn{0, 0, 0, 0});
    int64_t n_used = 0;
    for (size_t k = 0; k < P; ++k) {
        if (!ok_h[k] || cnt[2 * k + 1] < (uint32_t)prm.min_pair_matches) continue;
        ed.push_back(GraphEdgeIn{(uint32_t)pairs[2 * k], (uint32_t)pairs[2 * k + 1], (uint32_t)k, 0});
        ++fr[(size_t)pairs[2 * k]].n_adj;
        ++fr[(size_t)pairs[2 * k + 1]].n_adj;
        n_used += cnt[2 * k + 1];
    }
    const size_t E = ed.size();
    uint32_t at = 0;
    for (size_t f = 0; f < F; ++f) {
        fr[f].adj0 = at;
        at += fr[f].n_adj;
        fr[f].n_adj = 0;
    }
    adj.assign(2 * E + 1, 0u);
    for (size_t e = 0; e < E; ++e) {
        GraphFrameIn& fi = fr[ed[e].i];
        adj[fi.adj0 + fi.n_adj++] = (uint32_t)(e << 1);
        GraphFrameIn& fj = fr[ed[e].j];
        adj[fj.adj0 + fj.n_adj++] = (uint32_t)(e << 1) | 1u;
    }
    for (size_t f = 0; f < F; ++f) {
        if (!accepted((int32_t)f))
            fr[f].role = O3DR_REFINE_REJECTED;
        else if (status_in[f] == O3DR_CHAIN_MATCHED && !(fixed && fixed[f]) && fr[f].n_adj > 0)
            fr[f].role = O3DR_REFINE_FREE;
        else
            fr[f].role = O3DR_REFINE_FIXED;
    }
    if (prm.prior_weight == 0.0) {  // components without a gauge frame float
        std::vector<uint32_t>& comp = c->gr_comp_h;
        comp.resize(F);
        for (size_t f = 0; f < F; ++f) comp[f] = (uint32_t)f;
        auto find = [&](uint32_t x) {
            while (comp[x] != x) x = comp[x] = comp[comp[x]];
            return x;
        };
        for (size_t e = 0; e < E; ++e) comp[find(ed[e].i)] = find(ed[e].j);
        std::vector<uint8_t>& gauge = c->gr_gauge_h;
        gauge.assign(F, 0);
        for (size_t f = 0; f < F; ++f)
            if (fr[f].role == O3DR_REFINE_FIXED && fr[f].n_adj > 0) gauge[find((uint32_t)f)] = 1;
        for (size_t f = 0; f < F; ++f)
            if (fr[f].role == O3DR_REFINE_FREE && !gauge[find((uint32_t)f)]) fr[f].role = O3DR_REFINE_FLOATING;
    }
    o3dr_refine_result cn;
    memset(&cn, 0, sizeof cn);
    for (size_t f = 0; f < F; ++f) {
        cn.n_free += fr[f].role == O3DR_REFINE_FREE;
        cn.n_gauge += fr[f].role == O3DR_REFINE_FIXED && fr[f].n_adj > 0;
        cn.n_floating += fr[f].role == O3DR_REFINE_FLOATING;
        cn.n_rejected += fr[f].role == O3DR_REFINE_REJECTED;
    }
    cn.n_edges = (int32_t)E;
    cn.n_used = n_used;
    // 4. the solve: one launch
    if (E > 0) HIPCHK(hipMemcpyAsync(edges_d, ed.data(), E * sizeof(GraphEdgeIn), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(frames_d, fr.data(), F * sizeof(GraphFrameIn), hipMemcpyHostToDevice, c->stream));
    if (E > 0) HIPCHK(hipMemcpyAsync(adj_d, adj.data(), 2 * E * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    a.mom = ma.mom;
    a.edges = edges_d;
    a.frames = frames_d;
    a.adj = adj_d;
    a.poses_in = pin_d;
    a.prior = prior && prm.prior_weight > 0.0 ? prior_d : nullptr;
    a.poses_out = outs.dev(poses_out);
    a.counts = cn;
    a.prior_weight = prm.prior_weight;
    a.n_frames = (uint32_t)n_frames;
    a.n_edges = (uint32_t)E;
    a.gn_iterations = cn.n_free > 0 && E > 0 ? (uint32_t)prm.gn_iterations : 0u;  // (nothing to move: one evaluation)
    a.cg_iterations = (uint32_t)prm.cg_iterations;
    launch_graph_solve(&c->prof, c->stream, a);
    HIPCHK(hipGetLastError());
    std::vector<double>& ee = c->gr_energy_h;
    ee.assign(2 * E + 1, 0.0);
    HIPCHK(hipMemcpyAsync(frames_out, a.frames_out, F * sizeof(o3dr_refine_frame), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(res, a.res, sizeof(o3dr_refine_result), hipMemcpyDeviceToHost, c->stream));
    if (edges_out && E > 0) HIPCHK(hipMemcpyAsync(ee.data(), a.Ee, 2 * E * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (edges_out) {
        for (size_t k = 0; k < P; ++k) edges_out[k] = o3dr_refine_edge{(int32_t)cnt[2 * k], (int32_t)cnt[2 * k + 1], 0, 0, 0.0, 0.0};
        for (size_t e = 0; e < E; ++e) {
            o3dr_refine_edge& r = edges_out[ed[e].pair];
            r.edge = 1;
            r.energy_before = ee[2 * e];
            r.energy_after = ee[2 * e + 1];
        }
    }
    return O3DR_OK;
}

extern "C" int o3dr_pose_graph_refine(o3dr_ctx* c, const uint8_t* desc, const int64_t* offsets, const o3dr_point* kp3, int32_t n_frames,
                                      const float* poses_in, const int32_t* status_in, const uint8_t* fixed, const float* prior_poses,
                                      const int32_t* pairs, int64_t n_pairs, const o3dr_refine_params* p, const o3dr_ransac_params* rp,
                                      float* poses_out, o3dr_refine_frame* frames_out, o3dr_refine_edge* edges_out,
                                      o3dr_refine_result* res, int32_t mem)
{
    Outputs outs{mem};
    outs.add(poses_out, n_frames > 0 ? 16 * (int64_t)n_frames : 0);
    const int rc = entered(c, [&] {
        return pose_graph_refine(c, desc, offsets, kp3, n_frames, poses_in, status_in, fixed, prior_poses, pairs, n_pairs, p, rp, poses_out,
                                 frames_out, edges_out, res, outs, mem);
    });
    if (rc != O3DR_OK) {  // host outputs zeroed on error
        outs.zero();
        if (frames_out && n_frames > 0) memset(frames_out, 0, (size_t)n_frames * sizeof(o3dr_refine_frame));
        if (edges_out && n_pairs > 0) memset(edges_out, 0, (size_t)n_pairs * sizeof(o3dr_refine_edge));
        if (res) memset(res, 0, sizeof *res);
    }
    return rc;
}

// -------------------------------------------------------------------------------------------------
// plane-fitted disparity per segment label (kernels/plane_disparity.inc; DESIGN.md "Plane-fitted disparity")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_plane_disp_default_params(o3dr_plane_disp_params* p)
{
    if (!p) return;
    p->min_disparity = 0.0;  // d == 0: the stereo matcher's "no value"
    p->min_pixels = 3;
    p->max_mse = 0.0;        // no gate
    p->fill = 1;
}

constexpr size_t kPlaneDispTableBytes = (size_t)64 << 20;  // the sums table covers this many bytes of frames at a time

static int plane_fit_disparity(o3dr_ctx* c, const uint8_t* disp, int64_t disp_pitch, int64_t disp_fs, const void* labels, int32_t es,
                               int64_t lab_pitch, int64_t lab_fs, int32_t n_labels, int32_t rows, int32_t cols, int32_t n_frames,
                               const o3dr_plane_disp_params* p, double* out, o3dr_plane_disp_segment* segments, Outputs& outs,
                               uint32_t* status, int32_t mem)
{
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (n_frames < 0) return fail(O3DR_ERR_INVALID_ARG, "bad frame count");
    if (rows < 1 || rows > O3DR_PLANE_DISP_MAX_SIDE || cols < 1 || cols > O3DR_PLANE_DISP_MAX_SIDE)
        return fail(O3DR_ERR_INVALID_ARG, "rows and cols must be in 1..8192");
    if (n_labels < 1 || n_labels > O3DR_PLANE_DISP_MAX_LABELS) return fail(O3DR_ERR_INVALID_ARG, "n_labels must be in 1..65536");
    if (es != 1 && es != 2 && es != 4) return fail(O3DR_ERR_INVALID_ARG, "label_elem_size must be 1, 2 or 4");
    o3dr_plane_disp_params prm;
    o3dr_plane_disp_default_params(&prm);
    if (p) prm = *p;
    if (prm.min_disparity != prm.min_disparity) return fail(O3DR_ERR_INVALID_ARG, "min_disparity is NaN");
    if (!(prm.max_mse >= 0.0)) return fail(O3DR_ERR_INVALID_ARG, "max_mse must be >= 0 (0: no gate)");
    if (n_frames == 0) return O3DR_OK;
    if (!disp || !labels || !out) return fail(O3DR_ERR_INVALID_ARG, "disp / labels / out is NULL");
    if (disp_pitch < cols || lab_pitch < (int64_t)cols * es) return fail(O3DR_ERR_INVALID_ARG, "pitch smaller than a row");
    if (n_frames > 1 && (disp_fs < (int64_t)rows * disp_pitch || lab_fs < (int64_t)rows * lab_pitch))
        return fail(O3DR_ERR_INVALID_ARG, "frame stride smaller than a frame");
    if (((uintptr_t)labels | (uintptr_t)lab_pitch | (uintptr_t)lab_fs) % (uintptr_t)es)
        return fail(O3DR_ERR_INVALID_ARG, "labels, their pitch and frame stride must be multiples of the element size");
    if ((uintptr_t)out % 8 || (uintptr_t)segments % 8) return fail(O3DR_ERR_INVALID_ARG, "out / segments must be 8-byte aligned");

    const size_t npix = (size_t)rows * cols, F = (size_t)n_frames;
    const void *disp_d, *lab_d;
    CHK(stage_in(c, c->st_blur_in, disp, (size_t)disp_fs * (F - 1) + (size_t)disp_pitch * rows, mem, &disp_d));
    CHK(stage_in(c, c->op[o3dr_ctx::OP_IN], labels, (size_t)lab_fs * (F - 1) + (size_t)lab_pitch * rows, mem, &lab_d));
    // frames per pass: the table of sums stays within its budget (and within O3DR_BATCH_FRAMES); results do not depend on it
    size_t chunk = kPlaneDispTableBytes / ((size_t)n_labels * kPdSums * sizeof(unsigned long long));
    chunk = std::max<size_t>(1, std::min<size_t>(std::min<size_t>(chunk, (size_t)c->max_batch), F));
    uint32_t* flag;
    CHK(op_flags(c, &flag));
    unsigned long long* table;
    o3dr_plane_disp_segment* rec_scratch;
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(table, chunk * (size_t)n_labels * kPdSums);
        w.take(rec_scratch, segments ? 0 : chunk * (size_t)n_labels);
    }));
    CHK(outs.stage(c));  // the image, the records
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(uint32_t), c->stream));
    PlaneDispArgs a;
    memset(&a, 0, sizeof a);
    a.dpitch = disp_pitch, a.dfs = disp_fs, a.lpitch = lab_pitch, a.lfs = lab_fs;
    a.elem = es, a.rows = rows, a.cols = cols, a.n_labels = (uint32_t)n_labels;
    {   // (double)d > m  <=>  d > floor(m) for an integer d: the comparison on integers
        const double m = prm.min_disparity;
        a.thr = m >= 255.0 ? 255 : (m < 0.0 ? -1 : (int32_t)floor(m));
    }
    a.min_pixels = prm.min_pixels, a.fill = prm.fill ? 1 : 0, a.max_mse = prm.max_mse;
    a.table = table, a.flag = flag;
    for (size_t f0 = 0; f0 < F; f0 += chunk) {
        a.frames = (int32_t)std::min(chunk, F - f0);
        a.disp = (const uint8_t*)disp_d + (int64_t)f0 * disp_fs;
        a.labels = (const uint8_t*)lab_d + (int64_t)f0 * lab_fs;
        a.rec = segments ? outs.dev(segments) + f0 * (size_t)n_labels : rec_scratch;
        a.out = outs.dev(out) + f0 * npix;
        launch_plane_disp(&c->prof, c->stream, a);
    }
    HIPCHK(hipGetLastError());
    uint32_t flag_h = 0;
    HIPCHK(hipMemcpyAsync(&flag_h, flag, sizeof flag_h, hipMemcpyDeviceToHost, c->stream));
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (flag_h) {
        if (status) *status |= O3DR_STATUS_LABEL_RANGE;
        return fail(O3DR_ERR_INVALID_ARG, "a label is >= n_labels");
    }
    return O3DR_OK;
}

extern "C" int o3dr_plane_fit_disparity(o3dr_ctx* c, const uint8_t* disp, int64_t disp_pitch, int64_t disp_frame_stride,
                                        const void* labels, int32_t label_elem_size, int64_t labels_pitch, int64_t labels_frame_stride,
                                        int32_t n_labels, int32_t rows, int32_t cols, int32_t n_frames, const o3dr_plane_disp_params* p,
                                        double* out, o3dr_plane_disp_segment* segments, uint32_t* status, int32_t mem)
{
    if (status) *status = 0;
    // what the host outputs hold, for the zeroing after an error: only sizes within the contract's limits count
    const bool sized = n_frames > 0 && rows >= 1 && rows <= O3DR_PLANE_DISP_MAX_SIDE && cols >= 1 && cols <= O3DR_PLANE_DISP_MAX_SIDE &&
                       n_labels >= 1 && n_labels <= O3DR_PLANE_DISP_MAX_LABELS;
    Outputs outs{mem};
    outs.add(out, sized ? (int64_t)n_frames * rows * cols : 0);
    outs.add(segments, sized ? (int64_t)n_frames * n_labels : 0);
    const int rc = entered(c, [&] {
        return plane_fit_disparity(c, disp, disp_pitch, disp_frame_stride, labels, label_elem_size, labels_pitch, labels_frame_stride,
                                   n_labels, rows, cols, n_frames, p, out, segments, outs, status, mem);
    });
    if (rc != O3DR_OK) outs.zero();
    return rc;
}

// -------------------------------------------------------------------------------------------------
// ORB features (kernels/orb.inc; DESIGN.md "ORB features")
// -------------------------------------------------------------------------------------------------
extern "C" void o3dr_orb_default_params(o3dr_orb_params* p)
{
    if (!p) return;
    p->n_features = 1500;
    p->scale_factor = 1.3f;
    p->n_levels = 5;
    p->fast_threshold = 20;
    p->edge = 31;
    p->channels = 3;
}

extern "C" int o3dr_orb_pattern(int8_t* out)
{
    if (!out) return fail(O3DR_ERR_INVALID_ARG, "out is NULL");
    static const int16_t dir[64][2] = {O3DR_ORB_DIRECTIONS};
    const uint64_t S = splitmix64(O3DR_ORB_PATTERN_SEED);
    uint64_t n = 0;
    int base[256][4];
    for (int i = 0; i < 256;) {
        int v[4];
        for (int k = 0; k < 4; ++k) {
            int sum = 0;
            for (int d = 0; d < 4; ++d) sum += (int)((splitmix64(S + n++) >> 32) % 7);
            v[k] = sum - 12;
        }
        if ((v[0] == v[2] && v[1] == v[3]) || v[0] * v[0] + v[1] * v[1] > 169 || v[2] * v[2] + v[3] * v[3] > 169) continue;
        memcpy(base[i++], v, sizeof v);
    }
    for (int k = 0; k < 64; ++k)
        for (int i = 0; i < 256; ++i)
            for (int h = 0; h < 2; ++h) {
                const int px = base[i][2 * h], py = base[i][2 * h + 1];
                out[((k * 256 + i) * 4) + 2 * h] = (int8_t)((px * dir[k][0] - py * dir[k][1] + 8192) >> 14);
                out[((k * 256 + i) * 4) + 2 * h + 1] = (int8_t)((px * dir[k][1] + py * dir[k][0] + 8192) >> 14);
            }
    return O3DR_OK;
}

static int orb_check_params(const o3dr_orb_params& p, int32_t rows, int32_t cols)
{
    STACKCHK(stack_sides_error(rows, cols, O3DR_ORB_MAX_SIDE));
    if (p.n_features < 1 || p.n_features > 65535) return fail(O3DR_ERR_INVALID_ARG, "n_features must be in 1..65535");
    if (!(p.scale_factor > 1.f && p.scale_factor <= 2.f)) return fail(O3DR_ERR_INVALID_ARG, "scale_factor must be in (1, 2]");
    if (p.n_levels < 1 || p.n_levels > O3DR_ORB_MAX_LEVELS) return fail(O3DR_ERR_INVALID_ARG, "n_levels must be in 1..8");
    if (p.fast_threshold < 1 || p.fast_threshold > 254) return fail(O3DR_ERR_INVALID_ARG, "fast_threshold must be in 1..254");
    if (p.edge < 16 || p.edge > 255) return fail(O3DR_ERR_INVALID_ARG, "edge must be in 16..255");
    if (p.channels != 1 && p.channels != 3) return fail(O3DR_ERR_INVALID_ARG, "channels must be 1 or 3");
    return O3DR_OK;
}

// level sizes and quotas (include/o3dr.h steps 2 and 5)
static void orb_levels(const o3dr_orb_params& p, int32_t rows, int32_t cols, int32_t* wh, int32_t* quota)
{
    double s = 1.0;
    int64_t sum_w = 0;
    for (int l = 0; l < p.n_levels; ++l) {
        const int64_t sc = l == 0 ? 65536 : (int64_t)floor(65536.0 * s + 0.5);
        int64_t w = ((int64_t)cols * 65536 + sc / 2) / sc, h = ((int64_t)rows * 65536 + sc / 2) / sc;
        if (w == 0 || h == 0) w = h = 0;
        wh[2 * l] = (int32_t)w;
        wh[2 * l + 1] = (int32_t)h;
        sum_w += w;
        s *= (double)p.scale_factor;
    }
    int64_t given = 0;
    for (int l = 0; l < p.n_levels; ++l) {
        quota[l] = (int32_t)((int64_t)p.n_features * wh[2 * l] / sum_w);
        given += quota[l];
    }
    quota[0] += (int32_t)(p.n_features - given);
}

extern "C" int o3dr_orb_level_sizes(int32_t rows, int32_t cols, const o3dr_orb_params* p, int32_t* wh, int32_t* quota)
{
    o3dr_orb_params prm;
    o3dr_orb_default_params(&prm);
    if (p) prm = *p;
    CHK(orb_check_params(prm, rows, cols));
    int32_t wh_[2 * O3DR_ORB_MAX_LEVELS], q_[O3DR_ORB_MAX_LEVELS];
    orb_levels(prm, rows, cols, wh_, q_);
    if (wh) memcpy(wh, wh_, sizeof(int32_t) * 2 * prm.n_levels);
    if (quota) memcpy(quota, q_, sizeof(int32_t) * prm.n_levels);
    return O3DR_OK;
}

constexpr size_t kOrbScratchBytes = (size_t)1 << 30;  // a group of frames keeps its scratch within this (one frame always fits)

static int orb_detect(o3dr_ctx* c, const uint8_t* img, int64_t fs, int64_t pitch, int32_t rows, int32_t cols, int32_t n_frames,
                      const o3dr_orb_params* p, o3dr_orb_keypoint* kp, float* kp_xy, uint8_t* desc, Outputs& outs, int64_t* offsets,
                      uint8_t* levels_out, int64_t out_capacity, int64_t* n_out, int32_t mem)
{
    if (!n_out || !offsets) return fail(O3DR_ERR_INVALID_ARG, "n_out / offsets is NULL");
    STACKCHK(stack_call_error(mem, n_frames));
    o3dr_orb_params prm;
    o3dr_orb_default_params(&prm);
    if (p) prm = *p;
    CHK(orb_check_params(prm, rows, cols));
    if (n_frames == 0) return O3DR_OK;
    if (!img) return fail(O3DR_ERR_INVALID_ARG, "img is NULL");
    const ImageStack in{img, fs, pitch, rows, cols, n_frames, prm.channels};
    STACKCHK(stack_layout_error(in));
    if ((uintptr_t)kp % 16 || (uintptr_t)desc % 16 || (uintptr_t)kp_xy % 8)
        return fail(O3DR_ERR_INVALID_ARG, "kp / desc must be 16-byte aligned, kp_xy 8-byte");
    int64_t in_bytes;
    STACKCHK(stack_extent(in, &in_bytes));
    const int64_t bound = (int64_t)n_frames * prm.n_features;
    if (out_capacity < bound) return fail(O3DR_ERR_CAPACITY, "out_capacity is below n_frames * n_features");

    OrbArgs a;
    memset(&a, 0, sizeof a);
    int32_t wh[2 * O3DR_ORB_MAX_LEVELS], quota[O3DR_ORB_MAX_LEVELS];
    orb_levels(prm, rows, cols, wh, quota);
    int64_t tight = 0;  // pixels of a frame's pyramid, levels back to back
    for (int l = 0; l < prm.n_levels; ++l) {
        OrbLevel& L = a.lv[l];
        L.w = wh[2 * l], L.h = wh[2 * l + 1];
        const int64_t n = (int64_t)L.w * L.h;
        L.chunks = (int32_t)((n + kOrbChunk - 1) / kOrbChunk);
        L.chunk0 = a.chunks_per_frame;
        L.quota = quota[l];
        L.qprefix = l ? a.lv[l - 1].qprefix + a.lv[l - 1].quota : 0;
        L.off = a.P;
        L.cand0 = a.cands_per_frame;
        // kept corners are never 8-neighbours of each other: at most one per 2 x 2 block of the margin's interior
        const int64_t iw = L.w - 2 * prm.edge, ih = L.h - 2 * prm.edge;
        const int64_t cap = iw > 0 && ih > 0 ? ((iw + 1) / 2) * ((ih + 1) / 2) : 0;
        a.chunks_per_frame += L.chunks;
        a.P += (int64_t)align256((size_t)n);
        a.cands_per_frame += (int64_t)align256((size_t)cap);
        tight += n;
    }
    a.rows = rows, a.cols = cols, a.channels = prm.channels, a.n_levels = prm.n_levels, a.n_features = prm.n_features;
    a.thr = prm.fast_threshold, a.edge = prm.edge;
    a.fstride = fs, a.pitch = pitch;

    const void* img_d;
    CHK(stage_stacks(c, (size_t)in_bytes, mem, img, &img_d));
    if (!c->orb_pat_valid) {
        std::vector<int8_t>& pat = c->orb_pat_h;
        pat.resize(64 * 256 * 4);
        CHK(o3dr_orb_pattern(pat.data()));
        CHK(dev_ensure(c, c->orb_pat, pat.size()));
        HIPCHK(hipMemcpyAsync(c->orb_pat.p, pat.data(), pat.size(), hipMemcpyHostToDevice, c->stream));
        c->orb_pat_valid = true;
    }
    a.pattern = (const int8_t*)c->orb_pat.p;

    const size_t per_frame = (size_t)a.P * 4 + (size_t)a.cands_per_frame * 12 + (size_t)a.chunks_per_frame * 4 + (size_t)prm.n_levels * 16;
    const size_t limit = c->test_orb_scratch > 0 ? (size_t)c->test_orb_scratch : kOrbScratchBytes;
    const size_t group = frames_per_group(limit, per_frame, n_frames, 0);
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(a.pyr, group * (size_t)a.P);
        w.take(a.score, group * (size_t)a.P);
        w.take(a.box, group * (size_t)a.P);
        w.take(a.chunk_cnt, group * (size_t)a.chunks_per_frame);
        w.take(a.cand_r, group * (size_t)a.cands_per_frame);
        w.take(a.cand_pos, group * (size_t)a.cands_per_frame);
        w.take(a.seg_cand, group * (size_t)prm.n_levels);
        w.take(a.seg_sel, group * (size_t)prm.n_levels);
        w.take(a.seg_out, group * (size_t)prm.n_levels);
        w.take(a.run_total, 1);
        w.take(a.offsets, (size_t)n_frames + 1);
    }));
    outs.set_count(kp, bound);
    outs.set_count(kp_xy, bound);
    outs.set_count(desc, bound);
    CHK(outs.stage(c));
    a.kp = outs.dev(kp), a.kp_xy = outs.dev(kp_xy), a.desc = outs.dev(desc);
    if (mem == O3DR_MEM_HOST)  // the rows past *n_out are copied back as well
        for (int i = 0; i < outs.n; ++i)
            if (outs.item[i].dev && outs.item[i].count)
                HIPCHK(hipMemsetAsync(outs.item[i].dev, 0, outs.item[i].count * outs.item[i].elem, c->stream));
    HIPCHK(hipMemsetAsync(a.run_total, 0, sizeof(long long), c->stream));
    HIPCHK(hipMemsetAsync(a.offsets, 0, sizeof(long long), c->stream));
    for (size_t f0 = 0; f0 < (size_t)n_frames; f0 += group) {
        a.frames = (int32_t)std::min(group, (size_t)n_frames - f0);
        a.f0 = (int32_t)f0;
        a.img = (const uint8_t*)img_d + (int64_t)f0 * fs;
        launch_orb(&c->prof, c->stream, a);
        if (levels_out) {
            int64_t done = 0;
            for (int l = 0; l < prm.n_levels; ++l) {
                const size_t n = (size_t)a.lv[l].w * a.lv[l].h;
                if (!n) continue;
                HIPCHK(hipMemcpy2DAsync(levels_out + (int64_t)f0 * tight + done, (size_t)tight, a.pyr + a.lv[l].off, (size_t)a.P, n,
                                        (size_t)a.frames, mem == O3DR_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                        c->stream));
                done += (int64_t)n;
            }
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(offsets, a.offsets, sizeof(int64_t) * ((size_t)n_frames + 1), hipMemcpyDeviceToHost, c->stream));
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    *n_out = offsets[n_frames];
    return O3DR_OK;
}

extern "C" int o3dr_test_orb_scratch_limit(o3dr_ctx* c, int64_t bytes)
{
    CTX_ENTER(c);
    if (!c->test_hooks) return fail(O3DR_ERR_INVALID_ARG, "test hooks are off (create the context with O3DR_TEST_HOOKS=1)");
    if (bytes < 0) return fail(O3DR_ERR_INVALID_ARG, "bytes is negative");
    c->test_orb_scratch = bytes;
    return O3DR_OK;
}

extern "C" int o3dr_orb_detect(o3dr_ctx* c, const uint8_t* img, int64_t frame_stride, int64_t pitch, int32_t rows, int32_t cols,
                               int32_t n_frames, const o3dr_orb_params* p, o3dr_orb_keypoint* kp, float* kp_xy, uint8_t* desc,
                               int64_t* offsets, uint8_t* levels_out, int64_t out_capacity, int64_t* n_out, int32_t mem)
{
    if (n_out) *n_out = 0;
    if (offsets && n_frames >= 0) memset(offsets, 0, sizeof(int64_t) * ((size_t)n_frames + 1));
    Outputs outs{mem};
    outs.add(kp, out_capacity);
    outs.add(kp_xy, out_capacity);
    outs.add(desc, out_capacity);
    // (kp_xy's element is one float: two per row)
    if (Outputs::Item* it = outs.find(kp_xy)) it->elem = 2 * sizeof(float);
    if (Outputs::Item* it = outs.find(desc)) it->elem = 32;
    const int rc = entered(c, [&] {
        return orb_detect(c, img, frame_stride, pitch, rows, cols, n_frames, p, kp, kp_xy, desc, outs, offsets, levels_out, out_capacity,
                          n_out, mem);
    });
    if (rc != O3DR_OK && rc != O3DR_ERR_CAPACITY) {
        if (n_out) *n_out = 0;
        if (offsets && n_frames >= 0) memset(offsets, 0, sizeof(int64_t) * ((size_t)n_frames + 1));
        outs.zero();
    }
    return rc;
}

// =================================================================================================
// stereo disparity (kernels/stereo.inc; DESIGN.md "Stereo disparity")
// =================================================================================================
extern "C" void o3dr_stereo_default_params(o3dr_stereo_params* p)
{
    if (!p) return;
    p->n_disparities = 256;
    p->min_disparity = 0;
    p->p1 = 10;
    p->p2 = 120;
    p->n_paths = 8;
    p->uniqueness = 10;
    p->lr_max_diff = 1;
    p->channels = 3;
    p->group_frames = 0;
}

static bool stereo_disparities_ok(int32_t D) { return D >= 32 && D <= 256 && D % 32 == 0; }

static int stereo_check_params(const o3dr_stereo_params& p, int32_t rows, int32_t cols)
{
    STACKCHK(stack_sides_error(rows, cols, O3DR_STEREO_MAX_SIDE));
    if (!stereo_disparities_ok(p.n_disparities)) return fail(O3DR_ERR_INVALID_ARG, "n_disparities must be a multiple of 32 in 32..256");
    if (p.min_disparity < 0 || p.min_disparity + p.n_disparities > 256)
        return fail(O3DR_ERR_INVALID_ARG, "min_disparity must be >= 0 with min_disparity + n_disparities <= 256");
    if (p.p1 < 0 || p.p1 > 255) return fail(O3DR_ERR_INVALID_ARG, "p1 must be in 0..255");
    if (p.p2 < p.p1 || p.p2 > 255) return fail(O3DR_ERR_INVALID_ARG, "p2 must be in p1..255");
    if (p.n_paths != 4 && p.n_paths != 8) return fail(O3DR_ERR_INVALID_ARG, "n_paths must be 4 or 8");
    if (p.uniqueness < 0 || p.uniqueness > 99) return fail(O3DR_ERR_INVALID_ARG, "uniqueness must be in 0..99");
    if (p.lr_max_diff < -1 || p.lr_max_diff > 255) return fail(O3DR_ERR_INVALID_ARG, "lr_max_diff must be in -1..255");
    if (p.channels != 1 && p.channels != 3) return fail(O3DR_ERR_INVALID_ARG, "channels must be 1 or 3");
    if (p.group_frames < 0) return fail(O3DR_ERR_INVALID_ARG, "group_frames is negative");
    return O3DR_OK;
}

constexpr size_t kStereoScratchBytes = (size_t)1 << 30;  // a group of frames keeps its scratch within this (one frame always forms a group)

static int stereo_disparity(o3dr_ctx* c, const uint8_t* left, const uint8_t* right, int64_t fs, int64_t pitch, int32_t rows,
                            int32_t cols, int32_t n_frames, const o3dr_stereo_params* p, uint8_t* disp, uint16_t* disp_q4,
                            uint16_t* cost, Outputs& outs, uint16_t* volume_out, int32_t mem)
{
    STACKCHK(stack_call_error(mem, n_frames));
    o3dr_stereo_params prm;
    o3dr_stereo_default_params(&prm);
    if (p) prm = *p;
    CHK(stereo_check_params(prm, rows, cols));
    if (n_frames == 0) return O3DR_OK;
    if (!left || !right) return fail(O3DR_ERR_INVALID_ARG, "left / right is NULL");
    const ImageStack in{left, fs, pitch, rows, cols, n_frames, prm.channels};  // (the right images have the left ones' layout)
    STACKCHK(stack_layout_error(in));
    if ((uintptr_t)disp_q4 % 2 || (uintptr_t)cost % 2 || (uintptr_t)volume_out % 2)
        return fail(O3DR_ERR_INVALID_ARG, "disp_q4 / cost / volume_out must be 2-byte aligned");
    int64_t in_bytes;
    STACKCHK(stack_extent(in, &in_bytes));

    StereoArgs a;
    memset(&a, 0, sizeof a);
    a.rows = rows, a.cols = cols, a.channels = prm.channels;
    a.D = prm.n_disparities, a.d0 = prm.min_disparity, a.p1 = prm.p1, a.p2 = prm.p2, a.n_paths = prm.n_paths;
    a.uniq = prm.uniqueness, a.lr = prm.lr_max_diff;
    a.fstride = fs, a.pitch = pitch;
    const size_t n = (size_t)rows * (size_t)cols, D = (size_t)prm.n_disparities;
    const void *left_d, *right_d;
    CHK(stage_stacks(c, (size_t)in_bytes, mem, left, &left_d, right, &right_d));

    const size_t group = frames_per_group(kStereoScratchBytes, n * (2 * D + 21), n_frames, prm.group_frames);
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(a.cenL, group * n);
        w.take(a.cenR, group * n);
        w.take(a.S, group * n * D);
        w.take(a.win, group * n);
        w.take(a.bestR, group * n);
    }));
    CHK(outs.stage(c));
    uint8_t* disp_d = outs.dev(disp);
    uint16_t *q4_d = outs.dev(disp_q4), *cost_d = outs.dev(cost);
    for (size_t f0 = 0; f0 < (size_t)n_frames; f0 += group) {
        a.frames = (int32_t)std::min(group, (size_t)n_frames - f0);
        a.left = (const uint8_t*)left_d + (int64_t)f0 * fs;
        a.right = (const uint8_t*)right_d + (int64_t)f0 * fs;
        a.disp = disp_d ? disp_d + f0 * n : nullptr;
        a.q4 = q4_d ? q4_d + f0 * n : nullptr;
        a.cost = cost_d ? cost_d + f0 * n : nullptr;
        launch_stereo(&c->prof, c->stream, a);
        if (volume_out)
            HIPCHK(hipMemcpyAsync(volume_out + f0 * n * D, a.S, (size_t)a.frames * n * D * sizeof(uint16_t),
                                  mem == O3DR_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(hipGetLastError());
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_stereo_disparity(o3dr_ctx* c, const uint8_t* left, const uint8_t* right, int64_t frame_stride, int64_t pitch,
                                     int32_t rows, int32_t cols, int32_t n_frames, const o3dr_stereo_params* p, uint8_t* disp,
                                     uint16_t* disp_q4, uint16_t* cost, uint16_t* volume_out, int32_t mem)
{
    // the outputs' sizes are known only where the shape itself is within its limits
    const int64_t px = stack_pixels(rows, cols, n_frames, O3DR_STEREO_MAX_SIDE);
    Outputs outs{mem};
    outs.add(disp, px);
    outs.add(disp_q4, px);
    outs.add(cost, px);
    const int rc = entered(c, [&] {
        return stereo_disparity(c, left, right, frame_stride, pitch, rows, cols, n_frames, p, disp, disp_q4, cost, outs, volume_out, mem);
    });
    if (rc != O3DR_OK) {
        outs.zero();
        o3dr_stereo_params prm;
        o3dr_stereo_default_params(&prm);
        if (p) prm = *p;
        if (mem == O3DR_MEM_HOST && volume_out && px > 0 && stereo_disparities_ok(prm.n_disparities))
            memset(volume_out, 0, (size_t)px * (size_t)prm.n_disparities * sizeof(uint16_t));
    }
    return rc;
}

// =================================================================================================
// disparity filter (kernels/disparity_filter.inc; DESIGN.md "Disparity filter")
// =================================================================================================
extern "C" void o3dr_disparity_filter_default_params(o3dr_disparity_filter_params* p)
{
    if (!p) return;
    p->elem_bytes = 1;
    p->median_size = 0;
    p->max_speckle_size = 0;
    p->max_diff = 1;
    p->group_frames = 0;
}

static bool dfilter_elem_ok(int32_t e) { return e == 1 || e == 2; }

constexpr size_t kDfilterScratchBytes = (size_t)1 << 30;  // a group of frames keeps its scratch within this (one frame always forms a group)

static int disparity_filter(o3dr_ctx* c, const void* disp, int64_t fs, int64_t pitch, int32_t rows, int32_t cols, int32_t n_frames,
                            const o3dr_disparity_filter_params* p, uint8_t* out, int32_t* labels_out, int32_t* sizes_out,
                            o3dr_disparity_filter_info* info, Outputs& outs, int32_t mem)
{
    STACKCHK(stack_call_error(mem, n_frames));
    o3dr_disparity_filter_params prm;
    o3dr_disparity_filter_default_params(&prm);
    if (p) prm = *p;
    STACKCHK(stack_sides_error(rows, cols, O3DR_DISPARITY_FILTER_MAX_SIDE));
    if (!dfilter_elem_ok(prm.elem_bytes)) return fail(O3DR_ERR_INVALID_ARG, "elem_bytes must be 1 or 2");
    if (prm.median_size != 0 && prm.median_size != 3 && prm.median_size != 5) return fail(O3DR_ERR_INVALID_ARG, "median_size must be 0, 3 or 5");
    if (prm.max_speckle_size < 0) return fail(O3DR_ERR_INVALID_ARG, "max_speckle_size is negative");
    if (prm.max_diff < 0 || prm.max_diff > 65535) return fail(O3DR_ERR_INVALID_ARG, "max_diff must be in 0..65535");
    if (prm.group_frames < 0) return fail(O3DR_ERR_INVALID_ARG, "group_frames is negative");
    if (n_frames == 0) return O3DR_OK;
    if (!disp || !out) return fail(O3DR_ERR_INVALID_ARG, "disp / out is NULL");
    const int64_t E = prm.elem_bytes;
    const ImageStack in{disp, fs, pitch, rows, cols, n_frames, prm.elem_bytes};
    STACKCHK(stack_layout_error(in));
    if (!stack_aligned(in, E) || (uintptr_t)out % (uintptr_t)E) return fail(O3DR_ERR_INVALID_ARG, "uint16 images must be 2-byte aligned");
    if ((uintptr_t)labels_out % 4 || (uintptr_t)sizes_out % 4) return fail(O3DR_ERR_INVALID_ARG, "labels_out / sizes_out must be 4-byte aligned");
    int64_t in_bytes;
    STACKCHK(stack_extent(in, &in_bytes));

    DfArgs a;
    memset(&a, 0, sizeof a);
    a.rows = rows, a.cols = cols, a.elem = prm.elem_bytes, a.median = prm.median_size;
    a.max_diff = prm.max_diff, a.max_size = prm.max_speckle_size;
    const size_t n = (size_t)rows * (size_t)cols;
    if (ranges_overlap(disp, (size_t)in_bytes, out, (size_t)n_frames * n * (size_t)E)) return fail(O3DR_ERR_INVALID_ARG, "out must not overlap disp");
    const void* disp_d;
    CHK(stage_stacks(c, (size_t)in_bytes, mem, disp, &disp_d));

    // (without labelling a frame needs no scratch: the budget does not bound the group)
    const bool labelling = prm.max_speckle_size > 0 || labels_out || sizes_out || info;
    const size_t group = frames_per_group(labelling ? kDfilterScratchBytes : SIZE_MAX, n * 2 * sizeof(int32_t), n_frames, prm.group_frames);
    FrameCounters counts(info, n_frames, 5);
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        if (labelling) w.take(a.parent, group * n);
        if (labelling) w.take(a.cnt, group * n);
        counts.take(w);
    }));
    CHK(counts.zero(c));
    CHK(outs.stage(c));
    uint8_t* out_d = outs.dev(out);
    int32_t *labels_d = outs.dev(labels_out), *sizes_d = outs.dev(sizes_out);
    for (size_t f0 = 0; f0 < (size_t)n_frames; f0 += group) {
        a.frames = (int32_t)std::min(group, (size_t)n_frames - f0);
        a.in = DfView{(const char*)disp_d + (int64_t)f0 * fs, fs, pitch};
        a.out = out_d + f0 * n * (size_t)E;
        a.labels_out = labels_d ? labels_d + f0 * n : nullptr;
        a.sizes_out = sizes_d ? sizes_d + f0 * n : nullptr;
        a.info = counts.of_frame(f0);
        launch_disparity_filter(&c->prof, c->stream, a);
    }
    HIPCHK(hipGetLastError());
    CHK(outs.copy_back(c));
    CHK(counts.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t f = 0; f < counts.frames; ++f) {
        const unsigned long long* k = &counts.host[f * 5];
        info[f] = o3dr_disparity_filter_info{(int64_t)k[0], (int64_t)k[1], (int64_t)k[2], (int64_t)k[3], (int64_t)k[4]};
    }
    return O3DR_OK;
}

extern "C" int o3dr_disparity_filter(o3dr_ctx* c, const void* disp, int64_t frame_stride, int64_t pitch, int32_t rows, int32_t cols,
                                     int32_t n_frames, const o3dr_disparity_filter_params* p, void* out, int32_t* labels_out,
                                     int32_t* sizes_out, o3dr_disparity_filter_info* info, int32_t mem)
{
    // the outputs' sizes are known only where the shape itself (and for `out` the element size) is within its limits
    const int64_t px = stack_pixels(rows, cols, n_frames, O3DR_DISPARITY_FILTER_MAX_SIDE);
    const int32_t elem = p ? p->elem_bytes : 1;
    Outputs outs{mem};
    outs.add((uint8_t*)out, dfilter_elem_ok(elem) ? px * elem : 0);
    outs.add(labels_out, px);
    outs.add(sizes_out, px);
    const int rc = entered(c, [&] {
        return disparity_filter(c, disp, frame_stride, pitch, rows, cols, n_frames, p, (uint8_t*)out, labels_out, sizes_out, info, outs, mem);
    });
    if (rc != O3DR_OK) {
        outs.zero();
        if (info && px > 0) memset(info, 0, sizeof(o3dr_disparity_filter_info) * (size_t)n_frames);
    }
    return rc;
}

// =================================================================================================
// multi-view filter (kernels/multiview.inc; DESIGN.md "Multi-view filter")
// =================================================================================================
extern "C" void o3dr_multiview_default_params(o3dr_multiview_params* p)
{
    if (!p) return;
    p->elem_bytes = 1;
    p->tolerance = 1.0;
    p->min_support = 1;
    p->max_violations = -1;
}

extern "C" int o3dr_nearby_frames(const float* poses, int32_t n_frames, int32_t k, double max_distance, int32_t* neighbors_out)
{
    if (n_frames < 0) return fail(O3DR_ERR_INVALID_ARG, "bad frame count");
    if (k < 0 || k > O3DR_MULTIVIEW_MAX_NEIGHBORS) return fail(O3DR_ERR_INVALID_ARG, "k must be in 0..16");
    if (!(max_distance >= 0.0)) return fail(O3DR_ERR_INVALID_ARG, "max_distance is negative or NaN");
    if ((int64_t)n_frames * k == 0) return O3DR_OK;
    if (!poses || !neighbors_out) return fail(O3DR_ERR_INVALID_ARG, "poses / neighbors_out is NULL");
    const double lim = max_distance * max_distance;
    std::vector<std::pair<double, int32_t>> cand;
    for (int32_t i = 0; i < n_frames; ++i) {
        cand.clear();
        const float* a = poses + 16 * (size_t)i;
        for (int32_t j = 0; j < n_frames; ++j) {
            if (j == i) continue;
            const float* b = poses + 16 * (size_t)j;
            const double dx = (double)b[3] - (double)a[3], dy = (double)b[7] - (double)a[7], dz = (double)b[11] - (double)a[11];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (d2 <= lim) cand.emplace_back(d2, j);
        }
        std::sort(cand.begin(), cand.end());  // (dist2, j)
        for (int32_t n = 0; n < k; ++n) neighbors_out[(size_t)i * k + n] = n < (int32_t)cand.size() ? cand[(size_t)n].second : -1;
    }
    return O3DR_OK;
}

// 4 x 4 fp64 products and inverses of the contract, every sum in its stated order (this file is built with -ffp-contract=off)
static void mv_mul4(const double* a, const double* b, double* out)
{
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            out[4 * r + c] = ((a[4 * r] * b[c] + a[4 * r + 1] * b[4 + c]) + a[4 * r + 2] * b[8 + c]) + a[4 * r + 3] * b[12 + c];
}
static void mv_rigid_inverse(const float* T, double* inv)
{
    double t[16];
    for (int i = 0; i < 16; ++i) t[i] = (double)T[i];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) inv[4 * r + c] = t[4 * c + r];
        inv[4 * r + 3] = -((t[r] * t[3] + t[4 + r] * t[7]) + t[8 + r] * t[11]);
    }
    inv[12] = inv[13] = inv[14] = 0.0;
    inv[15] = 1.0;
}
static bool mv_adjugate_inverse(const double* a, double* inv)
{
    const double a00 = a[0], a01 = a[1], a02 = a[2], a03 = a[3], a10 = a[4], a11 = a[5], a12 = a[6], a13 = a[7];
    const double a20 = a[8], a21 = a[9], a22 = a[10], a23 = a[11], a30 = a[12], a31 = a[13], a32 = a[14], a33 = a[15];
    const double s0 = a00 * a11 - a10 * a01, s1 = a00 * a12 - a10 * a02, s2 = a00 * a13 - a10 * a03;
    const double s3 = a01 * a12 - a11 * a02, s4 = a01 * a13 - a11 * a03, s5 = a02 * a13 - a12 * a03;
    const double c5 = a22 * a33 - a32 * a23, c4 = a21 * a33 - a31 * a23, c3 = a21 * a32 - a31 * a22;
    const double c2 = a20 * a33 - a30 * a23, c1 = a20 * a32 - a30 * a22, c0 = a20 * a31 - a30 * a21;
    const double det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0;
    if (det == 0.0 || !std::isfinite(det)) return false;
    const double b[16] = {(a11 * c5 - a12 * c4) + a13 * c3, (a02 * c4 - a01 * c5) - a03 * c3, (a31 * s5 - a32 * s4) + a33 * s3,
                          (a22 * s4 - a21 * s5) - a23 * s3, (a12 * c2 - a10 * c5) - a13 * c1, (a00 * c5 - a02 * c2) + a03 * c1,
                          (a32 * s2 - a30 * s5) - a33 * s1, (a20 * s5 - a22 * s2) + a23 * s1, (a10 * c4 - a11 * c2) + a13 * c0,
                          (a01 * c2 - a00 * c4) - a03 * c0, (a30 * s4 - a31 * s2) + a33 * s0, (a21 * s2 - a20 * s4) - a23 * s0,
                          (a11 * c1 - a10 * c3) - a12 * c0, (a00 * c3 - a01 * c1) + a02 * c0, (a31 * s1 - a30 * s3) - a32 * s0,
                          (a20 * s3 - a21 * s1) + a22 * s0};
    for (int i = 0; i < 16; ++i) inv[i] = b[i] / det;
    return true;
}

// the checks the two entry points share, then H [n_frames][k][16] (zeros for a -1 entry)
static int multiview_matrices(o3dr_ctx* c, const float* poses, int32_t n_frames, const int32_t* neighbors, int32_t k, double* H)
{
    if (!c->has_Q) return fail(O3DR_ERR_NOT_CONFIGURED, "o3dr_set_camera has not been called");
    if (!poses) return fail(O3DR_ERR_INVALID_ARG, "poses is NULL");
    if (k > 0 && !neighbors) return fail(O3DR_ERR_INVALID_ARG, "neighbors is NULL");
    for (int64_t e = 0; e < (int64_t)n_frames * k; ++e) {
        const int32_t j = neighbors[e];
        if (j == -1) continue;
        if (j < 0 || j >= n_frames) return fail(O3DR_ERR_INVALID_ARG, "a neighbour lies outside 0..n_frames - 1");
        if (j == (int32_t)(e / k)) return fail(O3DR_ERR_INVALID_ARG, "a frame is listed as its own neighbour");
    }
    double Qinv[16];
    if (!mv_adjugate_inverse(c->Q, Qinv)) return fail(O3DR_ERR_INVALID_ARG, "Q is singular");
    std::vector<double> Tinv((size_t)n_frames * 16), Td((size_t)n_frames * 16);
    for (int32_t f = 0; f < n_frames; ++f) {
        mv_rigid_inverse(poses + 16 * (size_t)f, &Tinv[16 * (size_t)f]);
        for (int i = 0; i < 16; ++i) Td[16 * (size_t)f + i] = (double)poses[16 * (size_t)f + i];
    }
    for (int64_t e = 0; e < (int64_t)n_frames * k; ++e) {
        const int32_t j = neighbors[e];
        double* out = H + 16 * e;
        if (j < 0) {
            memset(out, 0, 16 * sizeof(double));
            continue;
        }
        double E[16], G[16];
        mv_mul4(&Tinv[16 * (size_t)j], &Td[16 * (size_t)(e / k)], E);
        mv_mul4(E, c->Q, G);
        mv_mul4(Qinv, G, out);
    }
    return O3DR_OK;
}

extern "C" int o3dr_multiview_homographies(o3dr_ctx* c, const float* poses, int32_t n_frames, const int32_t* neighbors, int32_t k,
                                           double* H_out)
{
    const bool sized = n_frames >= 0 && k >= 0 && k <= O3DR_MULTIVIEW_MAX_NEIGHBORS;
    const int rc = entered(c, [&] {
        if (n_frames < 0) return fail(O3DR_ERR_INVALID_ARG, "bad frame count");
        if (k < 0 || k > O3DR_MULTIVIEW_MAX_NEIGHBORS) return fail(O3DR_ERR_INVALID_ARG, "k must be in 0..16");
        if ((int64_t)n_frames * k == 0) return (int)O3DR_OK;
        if (!H_out) return fail(O3DR_ERR_INVALID_ARG, "H_out is NULL");
        return multiview_matrices(c, poses, n_frames, neighbors, k, H_out);
    });
    if (rc != O3DR_OK && sized && H_out) memset(H_out, 0, (size_t)n_frames * (size_t)k * 16 * sizeof(double));
    return rc;
}

static bool multiview_elem_ok(int32_t e) { return e == 1 || e == 2 || e == 8; }

// The filter and the fusion: one front end.  The filter writes `out` (the input's element type) and nine counters a frame
// into `info`; the fusion (fused != nullptr in a valid call; `fuse` says which entry point this is) writes `fused` and
// `votes_out` instead and twelve counters a frame into `finfo`.
static int multiview_run(o3dr_ctx* c, const void* disp, int64_t fs, int64_t pitch, int32_t rows, int32_t cols, int32_t n_frames,
                         const float* poses, const int32_t* neighbors, int32_t k, const o3dr_multiview_params* p, bool fuse, uint8_t* out,
                         double* fused, uint8_t* votes_out, uint8_t* support_out, uint8_t* violations_out, o3dr_multiview_info* info,
                         o3dr_multiview_fuse_info* finfo, Outputs& outs, int32_t mem)
{
    STACKCHK(stack_call_error(mem, n_frames));
    o3dr_multiview_params prm;
    o3dr_multiview_default_params(&prm);
    if (p) prm = *p;
    STACKCHK(stack_sides_error(rows, cols, O3DR_MULTIVIEW_MAX_SIDE));
    if (!multiview_elem_ok(prm.elem_bytes)) return fail(O3DR_ERR_INVALID_ARG, "elem_bytes must be 1, 2 or 8");
    if (!(prm.tolerance >= 0.0) || !std::isfinite(prm.tolerance)) return fail(O3DR_ERR_INVALID_ARG, "tolerance must be finite and >= 0");
    if (prm.min_support < 0 || prm.min_support > O3DR_MULTIVIEW_MAX_NEIGHBORS) return fail(O3DR_ERR_INVALID_ARG, "min_support must be in 0..16");
    if (prm.max_violations < -1 || prm.max_violations > O3DR_MULTIVIEW_MAX_NEIGHBORS)
        return fail(O3DR_ERR_INVALID_ARG, "max_violations must be in -1..16");
    if (k < 0 || k > O3DR_MULTIVIEW_MAX_NEIGHBORS) return fail(O3DR_ERR_INVALID_ARG, "k must be in 0..16");
    if (n_frames == 0) return O3DR_OK;
    const void* dst = fuse ? (const void*)fused : (const void*)out;
    if (!disp || !dst) return fail(O3DR_ERR_INVALID_ARG, "disp / out is NULL");
    const int64_t E = prm.elem_bytes, E_out = fuse ? (int64_t)sizeof(double) : E;
    const ImageStack in{disp, fs, pitch, rows, cols, n_frames, prm.elem_bytes};
    STACKCHK(stack_layout_error(in));
    if (!stack_aligned(in, E) || (uintptr_t)dst % (uintptr_t)E_out) return fail(O3DR_ERR_INVALID_ARG, "images must be aligned to their element size");
    const size_t n = (size_t)rows * (size_t)cols;
    int64_t in_bytes;
    STACKCHK(stack_extent(in, &in_bytes));
    if (ranges_overlap(disp, (size_t)in_bytes, dst, (size_t)n_frames * n * (size_t)E_out)) return fail(O3DR_ERR_INVALID_ARG, "out must not overlap disp");
    const size_t n_pairs = (size_t)n_frames * (size_t)k;
    std::vector<double> H(n_pairs * 16);  // (outlives the upload: the call synchronises at its end)
    CHK(multiview_matrices(c, poses, n_frames, neighbors, k, H.data()));

    const void* disp_d;
    CHK(stage_stacks(c, (size_t)in_bytes, mem, disp, &disp_d));
    MvArgs a;
    memset(&a, 0, sizeof a);
    a.in = disp_d, a.fstride = fs, a.pitch = pitch;
    a.rows = rows, a.cols = cols, a.frames = n_frames, a.elem = prm.elem_bytes, a.k = k;
    a.min_support = prm.min_support, a.max_violations = prm.max_violations, a.tolerance = prm.tolerance;
    double* H_d = nullptr;
    int32_t* nb_d = nullptr;
    const size_t words = fuse ? 12 : 9;
    FrameCounters counts(fuse ? (const void*)finfo : (const void*)info, n_frames, words);
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(H_d, n_pairs * 16);
        w.take(nb_d, n_pairs);
        counts.take(w);
    }));
    if (n_pairs) {
        HIPCHK(hipMemcpyAsync(H_d, H.data(), n_pairs * 16 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(nb_d, neighbors, n_pairs * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    }
    CHK(counts.zero(c));
    CHK(outs.stage(c));
    a.H = H_d, a.neighbors = nb_d, a.info = counts.dev;
    a.support_out = outs.dev(support_out), a.violations_out = outs.dev(violations_out);
    if (fuse) {
        a.fused_out = outs.dev(fused), a.votes_out = outs.dev(votes_out);
        launch_multiview_fuse(&c->prof, c->stream, a);
    } else {
        a.out = outs.dev(out);
        launch_multiview_filter(&c->prof, c->stream, a);
    }
    HIPCHK(hipGetLastError());
    CHK(outs.copy_back(c));
    CHK(counts.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t f = 0; f < counts.frames; ++f) {
        const unsigned long long* q = &counts.host[f * words];
        const o3dr_multiview_info fi{(int64_t)q[0], (int64_t)q[1], (int64_t)q[2], (int64_t)q[3], (int64_t)q[4],
                                     (int64_t)q[5], (int64_t)q[6], (int64_t)q[7], (int64_t)q[8]};
        if (fuse)
            finfo[f] = o3dr_multiview_fuse_info{fi, (int64_t)q[9], (int64_t)q[10], (int64_t)q[11]};
        else
            info[f] = fi;
    }
    return O3DR_OK;
}

extern "C" int o3dr_multiview_filter(o3dr_ctx* c, const void* disp, int64_t frame_stride, int64_t pitch, int32_t rows, int32_t cols,
                                     int32_t n_frames, const float* poses, const int32_t* neighbors, int32_t k,
                                     const o3dr_multiview_params* p, void* out, uint8_t* support_out, uint8_t* violations_out,
                                     o3dr_multiview_info* info, int32_t mem)
{
    // the outputs' sizes are known only where the shape itself (and for `out` the element size) is within its limits
    const int64_t px = stack_pixels(rows, cols, n_frames, O3DR_MULTIVIEW_MAX_SIDE);
    const int32_t elem = p ? p->elem_bytes : 1;
    Outputs outs{mem};
    outs.add((uint8_t*)out, multiview_elem_ok(elem) ? px * elem : 0);
    outs.add(support_out, px);
    outs.add(violations_out, px);
    const int rc = entered(c, [&] {
        return multiview_run(c, disp, frame_stride, pitch, rows, cols, n_frames, poses, neighbors, k, p, false, (uint8_t*)out, nullptr,
                             nullptr, support_out, violations_out, info, nullptr, outs, mem);
    });
    if (rc != O3DR_OK) {
        outs.zero();
        if (info && px > 0) memset(info, 0, sizeof(o3dr_multiview_info) * (size_t)n_frames);
    }
    return rc;
}

// multi-view fusion (contract: include/o3dr.h "multi-view fusion"): the filter's checks and staging, the fusion's kernel
extern "C" int o3dr_multiview_fuse(o3dr_ctx* c, const void* disp, int64_t frame_stride, int64_t pitch, int32_t rows, int32_t cols,
                                   int32_t n_frames, const float* poses, const int32_t* neighbors, int32_t k,
                                   const o3dr_multiview_params* p, double* out, uint8_t* votes_out, uint8_t* support_out,
                                   uint8_t* violations_out, o3dr_multiview_fuse_info* info, int32_t mem)
{
    const int64_t px = stack_pixels(rows, cols, n_frames, O3DR_MULTIVIEW_MAX_SIDE);
    Outputs outs{mem};
    outs.add(out, px);  // (float64 whatever the input's element size)
    outs.add(votes_out, px);
    outs.add(support_out, px);
    outs.add(violations_out, px);
    const int rc = entered(c, [&] {
        return multiview_run(c, disp, frame_stride, pitch, rows, cols, n_frames, poses, neighbors, k, p, true, nullptr, out, votes_out,
                             support_out, violations_out, nullptr, info, outs, mem);
    });
    if (rc != O3DR_OK) {
        outs.zero();
        if (info && px > 0) memset(info, 0, sizeof(o3dr_multiview_fuse_info) * (size_t)n_frames);
    }
    return rc;
}

// =================================================================================================
// image segmentation (kernels/segment_image.inc; DESIGN.md "Image segmentation")
// =================================================================================================
extern "C" void o3dr_segment_default_params(o3dr_segment_params* p)
{
    if (!p) return;
    p->channels = 3;
    p->step = 16;
    p->compactness = 20;
    p->iterations = 5;
    p->min_size = -1;
    p->group_frames = 0;
}

constexpr size_t kSegmentScratchBytes = (size_t)1 << 30;  // a group of frames keeps its scratch within this (one frame always forms a group)

static int segment_image(o3dr_ctx* c, const uint8_t* img, int64_t fs, int64_t pitch, int32_t rows, int32_t cols, int32_t n_frames,
                         const o3dr_segment_params* p, int32_t* labels, int32_t* raw_out, int32_t* sizes_out, o3dr_segment_info* info,
                         Outputs& outs, int32_t mem)
{
    STACKCHK(stack_call_error(mem, n_frames));
    o3dr_segment_params prm;
    o3dr_segment_default_params(&prm);
    if (p) prm = *p;
    STACKCHK(stack_sides_error(rows, cols, O3DR_SEGMENT_MAX_SIDE));
    if (prm.channels != 1 && prm.channels != 3) return fail(O3DR_ERR_INVALID_ARG, "channels must be 1 or 3");
    if (prm.step < 4 || prm.step > 256) return fail(O3DR_ERR_INVALID_ARG, "step must be in 4..256");
    if (prm.compactness < 0 || prm.compactness > 255) return fail(O3DR_ERR_INVALID_ARG, "compactness must be in 0..255");
    if (prm.iterations < 0 || prm.iterations > 32) return fail(O3DR_ERR_INVALID_ARG, "iterations must be in 0..32");
    if (prm.group_frames < 0) return fail(O3DR_ERR_INVALID_ARG, "group_frames is negative");
    if (n_frames == 0) return O3DR_OK;
    if (!img || !labels) return fail(O3DR_ERR_INVALID_ARG, "img / labels is NULL");
    const ImageStack in{img, fs, pitch, rows, cols, n_frames, prm.channels};
    STACKCHK(stack_layout_error(in));
    if ((uintptr_t)labels % 4 || (uintptr_t)raw_out % 4 || (uintptr_t)sizes_out % 4)
        return fail(O3DR_ERR_INVALID_ARG, "labels / raw_out / sizes_out must be 4-byte aligned");
    int64_t in_bytes;
    STACKCHK(stack_extent(in, &in_bytes));

    SegArgs a;
    memset(&a, 0, sizeof a);
    a.rows = rows, a.cols = cols, a.channels = prm.channels, a.S = prm.step, a.m = prm.compactness, a.iterations = prm.iterations;
    a.min_size = prm.min_size < 0 ? prm.step * prm.step / 4 : prm.min_size;
    a.nx = (cols + prm.step - 1) / prm.step, a.ny = (rows + prm.step - 1) / prm.step;
    a.fstride = fs, a.pitch = pitch;
    const size_t n = (size_t)rows * (size_t)cols, nc = (size_t)a.nx * (size_t)a.ny;
    const size_t n_chunks = (n + 4095) / 4096;
    const void* img_d;
    CHK(stage_stacks(c, (size_t)in_bytes, mem, img, &img_d));

    const size_t group = frames_per_group(kSegmentScratchBytes, n * 28 + nc * 68 + n_chunks * 4, n_frames, prm.group_frames);
    FrameCounters counts(info, n_frames, 5);
    int32_t* raw_scratch = nullptr;
    CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) {
        w.take(a.key, group * n);
        w.take(a.sums, group * nc * 6);
        counts.take(w);
        if (!raw_out) w.take(raw_scratch, group * n);
        w.take(a.parent, group * n);
        w.take(a.cnt, group * n);
        w.take(a.link, group * n);
        w.take(a.flag, group * n);
        w.take(a.centres, group * nc * 5);
        w.take(a.partial, group * n_chunks);
    }));
    CHK(counts.zero(c));
    CHK(outs.stage(c));
    int32_t *labels_d = outs.dev(labels), *raw_d = outs.dev(raw_out), *sizes_d = outs.dev(sizes_out);
    for (size_t f0 = 0; f0 < (size_t)n_frames; f0 += group) {
        a.frames = (int32_t)std::min(group, (size_t)n_frames - f0);
        a.img = (const uint8_t*)img_d + (int64_t)f0 * fs;
        a.labels_out = labels_d + f0 * n;
        a.raw = raw_d ? raw_d + f0 * n : raw_scratch;
        a.sizes_out = sizes_d ? sizes_d + f0 * n : nullptr;
        a.info = counts.of_frame(f0);
        launch_segment_image(&c->prof, c->stream, a);
    }
    HIPCHK(hipGetLastError());
    CHK(outs.copy_back(c));
    CHK(counts.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t f = 0; f < counts.frames; ++f) {
        const unsigned long long* k = &counts.host[f * 5];
        info[f] = o3dr_segment_info{(int64_t)nc, (int64_t)k[0], (int64_t)k[1], (int64_t)k[2], (int64_t)k[3], (int64_t)(0xffffffffull - k[4])};
    }
    return O3DR_OK;
}

extern "C" int o3dr_segment_image(o3dr_ctx* c, const uint8_t* img, int64_t frame_stride, int64_t pitch, int32_t rows, int32_t cols,
                                  int32_t n_frames, const o3dr_segment_params* p, int32_t* labels, int32_t* raw_out, int32_t* sizes_out,
                                  o3dr_segment_info* info, int32_t mem)
{
    // the outputs' sizes are known only where the shape itself is within its limits
    const int64_t px = stack_pixels(rows, cols, n_frames, O3DR_SEGMENT_MAX_SIDE);
    Outputs outs{mem};
    outs.add(labels, px);
    outs.add(raw_out, px);
    outs.add(sizes_out, px);
    const int rc = entered(c, [&] {
        return segment_image(c, img, frame_stride, pitch, rows, cols, n_frames, p, labels, raw_out, sizes_out, info, outs, mem);
    });
    if (rc != O3DR_OK) {
        outs.zero();
        if (info && px > 0) memset(info, 0, sizeof(o3dr_segment_info) * (size_t)n_frames);
    }
    return rc;
}

// =================================================================================================
// stereo rectification (kernels/rectify.inc; DESIGN.md "Stereo rectification")
// =================================================================================================
static int rectify_maps(o3dr_ctx* c, const o3dr_rectify_camera* cam, int32_t rows_out, int32_t cols_out, int32_t* map, Outputs& outs,
                        int32_t mem)
{
    if (mem != O3DR_MEM_HOST && mem != O3DR_MEM_DEVICE) return fail(O3DR_ERR_INVALID_ARG, "bad mem kind");
    if (!stack_pixels(rows_out, cols_out, 1, O3DR_RECTIFY_MAX_SIDE)) return fail(O3DR_ERR_INVALID_ARG, "rows_out and cols_out must be in 1..8192");
    if (!cam || !map) return fail(O3DR_ERR_INVALID_ARG, "cam / map is NULL");
    if ((uintptr_t)map % 4) return fail(O3DR_ERR_INVALID_ARG, "map must be 4-byte aligned");
    {
        const double* v = cam->K;  // K, D, R, P lie one after the other: 38 doubles
        static_assert(sizeof(o3dr_rectify_camera) == 38 * sizeof(double), "o3dr_rectify_camera is 38 doubles");
        for (int i = 0; i < 38; ++i)
            if (!std::isfinite(v[i])) return fail(O3DR_ERR_INVALID_ARG, "a non-finite entry in the camera");
    }
    const double *K = cam->K, *R = cam->R, *P = cam->P;
    if (K[1] != 0.0 || K[3] != 0.0 || K[6] != 0.0 || K[7] != 0.0 || K[8] != 1.0)
        return fail(O3DR_ERR_INVALID_ARG, "K must be [fx 0 cx; 0 fy cy; 0 0 1]");
    // the contract's host part, operation for operation (this file is built with -ffp-contract=off)
    double A[3][3], cf[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = (P[4 * i] * R[j] + P[4 * i + 1] * R[3 + j]) + P[4 * i + 2] * R[6 + j];
    cf[0][0] = A[1][1] * A[2][2] - A[1][2] * A[2][1];
    cf[0][1] = A[1][2] * A[2][0] - A[1][0] * A[2][2];
    cf[0][2] = A[1][0] * A[2][1] - A[1][1] * A[2][0];
    cf[1][0] = A[0][2] * A[2][1] - A[0][1] * A[2][2];
    cf[1][1] = A[0][0] * A[2][2] - A[0][2] * A[2][0];
    cf[1][2] = A[0][1] * A[2][0] - A[0][0] * A[2][1];
    cf[2][0] = A[0][1] * A[1][2] - A[0][2] * A[1][1];
    cf[2][1] = A[0][2] * A[1][0] - A[0][0] * A[1][2];
    cf[2][2] = A[0][0] * A[1][1] - A[0][1] * A[1][0];
    const double det = (A[0][0] * cf[0][0] + A[0][1] * cf[0][1]) + A[0][2] * cf[0][2];
    if (det == 0.0 || !std::isfinite(det)) return fail(O3DR_ERR_INVALID_ARG, "P R is singular");
    RectMapArgs a;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a.I[3 * i + j] = cf[j][i] / det;
    for (int i = 0; i < 8; ++i) a.k[i] = cam->D[i];
    a.fx = K[0], a.cx = K[2], a.fy = K[4], a.cy = K[5];
    a.rows_out = rows_out, a.cols_out = cols_out;
    CHK(outs.stage(c));
    a.map = outs.dev(map);
    launch_rectify_maps(&c->prof, c->stream, a);
    HIPCHK(hipGetLastError());
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_rectify_maps(o3dr_ctx* c, const o3dr_rectify_camera* cam, int32_t rows_out, int32_t cols_out, int32_t* map, int32_t mem)
{
    Outputs outs{mem};
    outs.add(map, stack_pixels(rows_out, cols_out, 1, O3DR_RECTIFY_MAX_SIDE) * 2);
    const int rc = entered(c, [&] { return rectify_maps(c, cam, rows_out, cols_out, map, outs, mem); });
    if (rc != O3DR_OK) outs.zero();
    return rc;
}

static int rectify_remap(o3dr_ctx* c, const uint8_t* src, int64_t fs, int64_t pitch, int32_t rows, int32_t cols, int32_t channels,
                         int32_t n_frames, const int32_t* map, int32_t rows_out, int32_t cols_out, int32_t border, int32_t group_frames,
                         uint8_t* out, uint8_t* valid_out, Outputs& outs, int32_t mem)
{
    STACKCHK(stack_call_error(mem, n_frames));
    if (stack_sides_error(rows, cols, O3DR_RECTIFY_MAX_SIDE) || stack_sides_error(rows_out, cols_out, O3DR_RECTIFY_MAX_SIDE))
        return fail(O3DR_ERR_INVALID_ARG, "rows, cols, rows_out and cols_out must be in 1..8192");
    if (channels != 1 && channels != 3) return fail(O3DR_ERR_INVALID_ARG, "channels must be 1 or 3");
    if (border < 0 || border > 255) return fail(O3DR_ERR_INVALID_ARG, "border must be in 0..255");
    if (group_frames < 0) return fail(O3DR_ERR_INVALID_ARG, "group_frames is negative");
    if (n_frames == 0) return O3DR_OK;
    if (!src || !map || !out) return fail(O3DR_ERR_INVALID_ARG, "src / map / out is NULL");
    if ((uintptr_t)map % 4) return fail(O3DR_ERR_INVALID_ARG, "map must be 4-byte aligned");
    const ImageStack in{src, fs, pitch, rows, cols, n_frames, channels};
    STACKCHK(stack_layout_error(in));
    const size_t n_out = (size_t)rows_out * (size_t)cols_out;
    int64_t in_bytes;
    STACKCHK(stack_extent(in, &in_bytes));
    if (ranges_overlap(src, (size_t)in_bytes, out, (size_t)n_frames * n_out * (size_t)channels)) return fail(O3DR_ERR_INVALID_ARG, "out must not overlap src");
    RectArgs a;
    memset(&a, 0, sizeof a);
    a.rows = rows, a.cols = cols, a.channels = channels, a.rows_out = rows_out, a.cols_out = cols_out, a.border = border;
    a.fstride = fs, a.pitch = pitch;
    const void* src_d;
    CHK(stage_stacks(c, (size_t)in_bytes, mem, src, &src_d));
    a.map = map;
    if (mem == O3DR_MEM_HOST) {
        int32_t* map_d = nullptr;
        CHK(carve(c, c->op[o3dr_ctx::OP_WORK], [&](Carve& w) { w.take(map_d, n_out * 2); }));
        HIPCHK(hipMemcpyAsync(map_d, map, n_out * 2 * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        a.map = map_d;
    }
    CHK(outs.stage(c));
    uint8_t* out_d = outs.dev(out);
    a.valid = outs.dev(valid_out);
    const size_t group = group_frames > 0 ? std::min<size_t>((size_t)group_frames, (size_t)n_frames) : (size_t)n_frames;
    for (size_t f0 = 0; f0 < (size_t)n_frames; f0 += group) {
        a.frames = (int32_t)std::min(group, (size_t)n_frames - f0);
        a.src = (const uint8_t*)src_d + (int64_t)f0 * fs;
        a.out = out_d + f0 * n_out * (size_t)channels;
        launch_rectify_remap(&c->prof, c->stream, a);
        a.valid = nullptr;  // one per map: the first group has written it
    }
    HIPCHK(hipGetLastError());
    CHK(outs.copy_back(c));
    HIPCHK(hipStreamSynchronize(c->stream));
    return O3DR_OK;
}

extern "C" int o3dr_rectify_remap(o3dr_ctx* c, const uint8_t* src, int64_t frame_stride, int64_t pitch, int32_t rows, int32_t cols,
                                  int32_t channels, int32_t n_frames, const int32_t* map, int32_t rows_out, int32_t cols_out,
                                  int32_t border, int32_t group_frames, uint8_t* out, uint8_t* valid_out, int32_t mem)
{
    // the outputs' sizes are known only where the sizes that give them are within their limits
    const int64_t px = stack_pixels(rows_out, cols_out, 1, O3DR_RECTIFY_MAX_SIDE);
    Outputs outs{mem};
    outs.add(out, n_frames > 0 && (channels == 1 || channels == 3) ? px * n_frames * channels : 0);
    outs.add(valid_out, n_frames > 0 ? px : 0);
    const int rc = entered(c, [&] {
        return rectify_remap(c, src, frame_stride, pitch, rows, cols, channels, n_frames, map, rows_out, cols_out, border, group_frames, out,
                             valid_out, outs, mem);
    });
    if (rc != O3DR_OK) outs.zero();
    return rc;
}

extern "C" int o3dr_profile_enable(o3dr_ctx* c, int32_t kernel_id, int32_t enable)
{
    CTX_ENTER(c);
    if (kernel_id >= O3DR_K_NUM) return fail(O3DR_ERR_INVALID_ARG, "bad kernel id");
    static_assert(O3DR_K_NUM < 64, "the profile mask is 64 bits wide");
    const uint64_t bits = kernel_id < 0 ? (((uint64_t)1 << O3DR_K_NUM) - 1u) : ((uint64_t)1 << kernel_id);
    if (enable)
        c->prof.mask |= bits;
    else
        c->prof.mask &= ~bits;
    return O3DR_OK;
}
extern "C" int o3dr_profile_read(o3dr_ctx* c, int32_t kernel_id, double* total_ms, int64_t* launches)
{
    CTX_ENTER(c);
    if (kernel_id < 0 || kernel_id >= O3DR_K_NUM) return fail(O3DR_ERR_INVALID_ARG, "bad kernel id");
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.drain();
    if (total_ms) *total_ms = c->prof.total_ms[kernel_id];
    if (launches) *launches = c->prof.launches[kernel_id];
    return O3DR_OK;
}
extern "C" int o3dr_profile_reset(o3dr_ctx* c)
{
    CTX_ENTER(c);
    HIPCHK(hipMemsetAsync(c->stats_dev, 0, sizeof(SortStats), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->prof.reset();
    return O3DR_OK;
}
extern "C" int o3dr_profile_stats(o3dr_ctx* c, int64_t out[8])
{
    CTX_ENTER(c);
    if (!out) return fail(O3DR_ERR_INVALID_ARG, "out is NULL");
    HIPCHK(hipMemcpyAsync(c->stats_host, c->stats_dev, sizeof(SortStats), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    out[0] = (int64_t)c->stats_host->sort_record_passes;
    out[1] = (int64_t)c->stats_host->voxel_points_in;
    out[2] = (int64_t)c->stats_host->voxel_points_out;
    out[3] = 0;
    out[4] = (int64_t)c->stats_host->sort_records;
    out[5] = (int64_t)c->stats_host->side_head_records;
    out[6] = out[7] = 0;
    return O3DR_OK;
}
extern "C" int o3dr_device_info(o3dr_ctx* c, char* name, int32_t name_len, int32_t* cu_count, int64_t* hbm_bytes)
{
    CTX_ENTER(c);
    hipDeviceProp_t p;
    HIPCHK(hipGetDeviceProperties(&p, c->device));
    if (name && name_len > 0) snprintf(name, (size_t)name_len, "%s (%s)", p.name, p.gcnArchName);
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
    return O3DR_OK;
}
