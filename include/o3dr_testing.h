/*
 * o3dr_testing.h — TEST-ONLY entry points of libo3dr.  Not part of the installed surface of include/o3dr.h: nothing a
 * caller of the reconstruction path needs is declared here, and every function below refuses to act
 * (O3DR_ERR_INVALID_ARG) unless the context was created with the environment variable O3DR_TEST_HOOKS=1.
 */
#ifndef O3DR_TESTING_H
#define O3DR_TESTING_H
#include "o3dr.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Test hook for the gather guards: the next o3dr_voxel_grid / o3dr_downsample_pt_cloud / o3dr_finalize of this
 * context finds one of its sorted payloads pointing outside the cloud, as a bookkeeping error upstream would leave it.
 * That call must return O3DR_ERR_INTERNAL with *n_out = 0 (never a GPU fault), and the context stays usable.
 * o3dr_accumulate_frames takes the hook too (frame 0 of its first batch): the call itself is asynchronous and returns
 * O3DR_OK; the next read of cloud_big or its size returns O3DR_ERR_INTERNAL, until o3dr_cloud_big_reset. */
int o3dr_test_corrupt_next_gather(o3dr_ctx* ctx);

/* The mean neighbour distances (pcl::StatisticalOutlierRemoval's `distances`, one per input point, input order) the
 * last o3dr_statistical_outlier_removal of this context computed for its n_in points: the inlier set alone says little
 * about an outlier's own distance, so the parity tests compare these with the oracle's bit for bit.  out: n floats in
 * host memory; n must not exceed that call's n_in. */
int o3dr_test_sor_distances(o3dr_ctx* ctx, float* out, int64_t n);

/* o3dr_merge_partitioned with W > 1 ranks on ONE GPU.  RCCL refuses two ranks on one device, so the multi-rank paths of
 * the exchange (slice sizes, segment order, failure agreement, statistics) would otherwise only ever run with one rank:
 * a LOCAL communicator connects n_ranks contexts of one process - one host thread each, all on the same device - through
 * device-to-device copies and a host barrier (a rank that does not show up within 30 s breaks it: O3DR_ERR_PEER).  The
 * protocol code is the one o3dr_merge_partitioned runs over RCCL; only the two transport primitives differ.
 * o3dr_test_fail_at: step `point` of this context's next exchange fails on this rank as an allocation would
 * (1 header, 2 partition, 3 buffers before the all-to-all, 4 local merge). */
int o3dr_test_local_comm_create(int32_t n_ranks, void** comm_out);
int o3dr_test_local_comm_destroy(void* comm);
int o3dr_test_merge_partitioned_local(o3dr_ctx* ctx, void* local_comm, int32_t rank, int32_t gather_result, o3dr_point* out,
                                      int64_t out_capacity, int64_t* n_out, int64_t* n_total, uint32_t* status, int32_t mem);
int o3dr_test_fail_at(o3dr_ctx* ctx, int32_t point);
/* The hypotheses of the last successful o3dr_segment_plane of this context with at least one tile: n_tiles * H planes
 * (4 floats each, NaN for a degenerate hypothesis) and their scores, tile-major, into host memory.  *n_out = n_tiles * H;
 * capacity (in hypotheses) below it: O3DR_ERR_CAPACITY with *n_out set.  The scores are what the choice of step 4 of the
 * contract reads, so the tests compare every one of them with a restatement. */
int o3dr_test_plane_hypotheses(o3dr_ctx* ctx, float* planes, uint32_t* counts, int64_t capacity, int64_t* n_out);
/* Later o3dr_orb_detect calls of this context split their frames into groups whose scratch fits `bytes` instead of the
 * built-in 1 GiB, so that a handful of small frames runs the group loop (frame base, running total, offsets, pyramid
 * copies).  bytes = 0 restores the default; a value below one frame's need still gives groups of one frame.  The
 * results must not depend on it. */
int o3dr_test_orb_scratch_limit(o3dr_ctx* ctx, int64_t bytes);
/* Fills every per-call scratch block this context currently owns with `byte` (0..255), over the block's whole capacity
 * and not just the last call's layout, in stream order on the context's stream: one hipMemsetAsync per block, no kernel.
 * *bytes_filled = the sum.  No later call's result may depend on it (DESIGN.md "Scratch contract").
 * Filled: the shared operator blocks op[0..4]; the sort / voxel workspace, its point block, the search grids' block and
 * the outlier removal's block; the staging buffers (st_*, st2_*, st_blur*, st_hist, st_xchg, st_merge, st_gather); nn_q, nn_t, nn_cells, nn_src;
 * the incremental merge's per-call buffers (scratch, tg, tmatch, flag, src, keep, partial, words) and its fallback result;
 * the 4 KiB misc block and the single-shot counters.
 * Never touched, because they carry state from call to call: cloud_big, its second buffer, its counters, running bounding
 * box and recorded run heads; the incremental merge's groups, cell offsets, cells and box; the cached tables (bilateral
 * weights, ORB pattern, Q table); the plane hypotheses kept for o3dr_test_plane_hypotheses; the sort statistics.
 * Two things that live in scratch are lost: a pending o3dr_cloud_big_slice_counts_dev table (dropped, as the ICP calls
 * drop it: o3dr_cloud_big_place_slices then asks for the counts again) and the distances o3dr_test_sor_distances reads.
 * O3DR_ERR_INVALID_ARG: null context, hooks off, byte outside 0..255, bytes_filled NULL. */
int o3dr_test_fill_scratch(o3dr_ctx* ctx, int32_t byte, int64_t* bytes_filled);

#ifdef __cplusplus
}
#endif
#endif /* O3DR_TESTING_H */
