/* o3dr_terrain.h - terrain operators on the merged map (libo3dr.so; o3dr.h holds the context, the point layout, the error
 * codes and the map raster this header builds on). */
#ifndef O3DR_TERRAIN_H
#define O3DR_TERRAIN_H
#include "o3dr.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- ground filter: the bare-earth ground mask of a cloud, its terrain model (DTM) and every point's height above it.
 * The family is pcl::ProgressiveMorphologicalFilter (Zhang et al. 2003): the minimum surface is opened with growing
 * windows, and what rises above the opening by more than a threshold that grows with the window is removed.  The
 * reference has no such tool (its segmentCloud is one RANSAC plane per tile: SURVEY section 2 row 16); the contract is
 * this library's own, as the map raster's.  Every step is an integer, a copy, a comparison, a min / max or one correctly
 * rounded fp32 subtraction: results are bit-identical across calls, memory kinds and whatever algorithm computes the
 * window minima.
 *
 * Input: n points, n < 2^31, every coordinate finite.
 *   1. Cells and box: the map raster's step 1 (o3dr.h): inv = 1.0f / (float)cell_size, cx = (int)floorf(x * inv),
 *      cy = (int)floorf(y * inv); the raster covers width x height cells from (cx0, cy0), element [r, c] of a raster output
 *      is cell (cx0 + c, cy0 + r); o3dr_raster_extent gives the cloud's own box.  Points outside the box are counted in
 *      n_outside and ignored.  The same limits: width, height >= 1, the far corner within int32, width * height <= 2^28.
 *   2. Minimum surface: per cell the point with the smallest z, ties to the lowest index, -0.0f taken as 0.0f
 *      (O3DR_RASTER_BOTTOM's rule); Z[c] is that point's z (a copy).  Every occupied cell starts live, state 1; an empty
 *      cell has state 0.
 *   3. Schedule (host, fp64; o3dr_ground_schedule returns it): r_k = window_base^k when exponential, (k + 1) * window_base
 *      when linear, for k = 0, 1, ... while r_k <= max_window_radius, at most O3DR_GROUND_MAX_ITERATIONS of them; a schedule
 *      with none is an error.  t_0 = initial_distance; for k > 0,
 *      t_k = slope * ((double)(2 * (r_k - r_{k-1})) * cell_size) + initial_distance; thr_k = (float)min(t_k, max_distance).
 *   4. Iteration k, on the set L of the cells live at its start: for every c in L, E[c] = min Z[c'] over the c' in L with
 *      |dx| <= r_k, |dy| <= r_k inside the raster; O[c] = max E[c'] over the same window and the same L; c is removed iff
 *      Z[c] - O[c] > thr_k (an fp32 subtraction, an fp32 compare): its state becomes 2 + k and it is not live from
 *      iteration k + 1 on.  Cells outside L take no part: E is defined on L only.
 *   5. Point mask: ground[i] = 1 iff point i is inside the box, its cell ends in state 1 and z_i - Z[cell] <= thr_0 in
 *      fp32; else 0.  A ground cell's lowest point is always ground.
 *   6. DTM: a ground cell (state 1) has Z[c]; every other cell, empty or removed, takes the nearest ground cell by the map
 *      raster's step 3 (the smallest dx*dx + dy*dy <= fill_radius^2, ties to the lowest (cy, cx); a fill never feeds a
 *      fill); NaN where there is none.
 *   7. height_above_ground[i] = z_i - dtm[cell(i)] in fp32; NaN for a point outside the box or on a NaN cell.
 *   8. o3dr_ground_result: the box; n_inside + n_outside = n; n_occupied = n_ground_cells + the sum of n_removed;
 *      n_ground_cells + n_dtm_filled + n_dtm_empty = width * height; n_ground_points; n_iterations and n_removed[k], the
 *      cells iteration k removed (0 past n_iterations).
 * Errors, O3DR_ERR_INVALID_ARG, in this order: a bad parameter, in the struct's order (cell_size as for the raster; a box
 * with a side < 1 or a corner outside int32; max_window_radius outside 1..128; window_base < 2 when exponential, < 1 when
 * linear; slope, initial_distance, max_distance not finite or < 0; fill_radius outside 0..32; a schedule without an
 * iteration); the cloud (a non-finite coordinate, a cell index outside int32); a box of more than 2^28 cells.  All are
 * found before any raster work and before anything of the raster's size is allocated.  On an error the host outputs and
 * the result are zeroed.  n == 0 is allowed: every cell is empty.  The call synchronises and reuses the operators'
 * scratch: cloud_big and the sort workspace are left alone.
 * o3dr_ground_schedule runs on the host and needs no context: it checks cell_size, max_window_radius, window_base and
 * the three distances as above (not the box, not fill_radius) and fills radii[0..15], thresholds[0..15] (0 past
 * *n_iterations) and *n_iterations. */
#define O3DR_GROUND_MAX_WINDOW_RADIUS 128
#define O3DR_GROUND_MAX_ITERATIONS 16
typedef struct o3dr_ground_params {
    double cell_size;            /* > 0, finite; no usable default (0 is rejected): the map's voxel_size */
    int32_t cx0, cy0, width, height; /* the box; no default (0 x 0 is rejected): o3dr_raster_extent's, or the caller's own */
    int32_t max_window_radius;   /* 16: the largest window half-width in cells, 1..128 */
    int32_t window_base;         /* 2 */
    int32_t exponential;         /* 1: r_k = window_base^k; 0: r_k = (k + 1) * window_base */
    int32_t reserved0;
    double slope;                /* 0.7: threshold growth per metre of window growth */
    double initial_distance;     /* 0.15 metres */
    double max_distance;         /* 10.0 metres */
    int32_t fill_radius;         /* 0: the DTM's hole fill in cells, 0..32 */
    int32_t reserved1;
} o3dr_ground_params;
typedef struct o3dr_ground_outputs {
    uint8_t* ground;             /* n: 1 = ground */
    float* height_above_ground;  /* n */
    float* dtm;                  /* width * height; NaN: no value */
    uint8_t* cell_state;         /* width * height: 0 empty, 1 ground, 2 + k removed by iteration k */
} o3dr_ground_outputs;
typedef struct o3dr_ground_result {
    int32_t cx0, cy0, width, height;
    int64_t n_inside, n_outside;   /* points inside / outside the box */
    int64_t n_occupied;            /* cells with a point */
    int64_t n_ground_cells, n_ground_points;
    int64_t n_dtm_filled, n_dtm_empty; /* cells that are not ground and took a neighbour's value; cells without a value */
    int32_t n_iterations, reserved;
    int64_t n_removed[O3DR_GROUND_MAX_ITERATIONS];
} o3dr_ground_result;
void o3dr_ground_default_params(o3dr_ground_params* p);
int  o3dr_ground_schedule(const o3dr_ground_params* p, int32_t radii[16], float thresholds[16], int32_t* n_iterations);
int  o3dr_ground_filter(o3dr_ctx* ctx, const o3dr_point* cloud, int64_t n, const o3dr_ground_params* p,
                        const o3dr_ground_outputs* out, o3dr_ground_result* res, int32_t mem);

#ifdef __cplusplus
}
#endif
#endif
