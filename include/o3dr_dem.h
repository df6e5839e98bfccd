/* o3dr_dem.h - elevation-model operators on a float32 raster (libo3dr.so; o3dr.h holds the context, the point layout, the
 * error codes, the memory kinds and the map raster this header builds on). */
#ifndef O3DR_DEM_H
#define O3DR_DEM_H
#include "o3dr.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- raster interpolation: every hole of a float32 raster filled from the data around it, at any distance.  The method is
 * pull-push over an image pyramid with a few Jacobi relaxations per level on the way down (a cascadic multigrid): a fixed
 * number of passes whatever the size of a hole.  The reference has no such tool; the contract is
 * this library's own.  Every value is defined per cell by a fixed sequence of fp64 operations, each correctly rounded:
 * results are bit-identical across calls, memory kinds and whatever tiling computes them.
 *
 * Input: `raster`, row-major float32 [height, width].  A NaN of any payload is a hole; every other value must be finite.
 *   1. Level 0: on a data cell c_0 = 1, m_0 = the value; on a hole c_0 = 0, m_0 = +0.0f.  Level l has W_l = (W_{l-1} + 1) >> 1
 *      columns and H_l = (H_{l-1} + 1) >> 1 rows.  The top level L is the first with W_L = H_L = 1; n_levels = L + 1 (a
 *      1 x 1 raster has L = 0).
 *   2. Pull, for l = 1 .. L: cell (X, Y) has the children (2X + i, 2Y + j) of level l - 1, taken in the order (i, j) =
 *      (0, 0), (1, 0), (0, 1), (1, 1); a child outside level l - 1 has c = 0, m = +0.0f.  n = the sum of the four c (int32).
 *      s = 0.0; s = s + (double)c * (double)m for the four children in that order.  m_l = n > 0 ? (float)(s / (double)n) :
 *      +0.0f; c_l = n.  The products are exact in fp64 (c <= 2^28, 24-bit significands), so the result does not depend on
 *      multiply-add contraction: it is the count-weighted mean of the data under the cell.
 *   3. No data: if c_L = 0, every cell of `filled` is NaN, every cell of `level` is 255 and n_empty = width * height.
 *   4. Push, for l = L - 1 down to 0, from F_L = m_L.  A cell with c_l > 0 has F_l = m_l (at level 0: the input's bits).  A
 *      cell (x, y) with c_l = 0 has X = x >> 1, Xn = clamp(x odd ? X + 1 : X - 1, 0, W_{l+1} - 1), and Y, Yn likewise from y
 *      and H_{l+1}; with a = F_{l+1}(X, Y), b = F_{l+1}(Xn, Y), c = F_{l+1}(X, Yn), d = F_{l+1}(Xn, Yn) taken as doubles,
 *      F_l = (float)((((9.0 * a + 3.0 * b) + 3.0 * c) + d) * 0.0625) (the products by 9 and 3 are exact in fp64).  Then
 *      `smooth` Jacobi sweeps run over level l, every sweep reading the values the sweep before it left: a cell with
 *      c_l = 0 becomes (float)(s / (double)k), s = ((up + left) + right) + down in fp64 over the neighbours (x, y - 1),
 *      (x - 1, y), (x + 1, y), (x, y + 1); a neighbour outside the level adds +0.0 and is not counted in k; k = 0 leaves
 *      the cell as it is.  Cells with c_l > 0 never change.
 *   5. Outputs: level[cell] = 0 on a data cell, else the smallest l >= 1 with c_l(x >> l, y >> l) > 0.  filled = F_0, except
 *      that with max_level = M > 0 a cell whose level exceeds M is NaN and is counted in n_empty (its level stays).  Every
 *      NaN written is 0x7fc00000.  n_by_level[l] counts the cells of level l, n_by_level[0] = n_data; n_filled counts the
 *      holes that got a value; n_data + n_filled + n_empty = width * height.
 * Errors, O3DR_ERR_INVALID_ARG, in this order: params, raster, outputs or outputs->filled is NULL; a bad mem; width or
 * height < 1; smooth outside 0..8; max_level outside 0..31; more than O3DR_RASTER_MAX_CELLS cells; an infinite input value.
 * On an error the host outputs and the result are zeroed.  With O3DR_MEM_DEVICE `raster` and `filled` must not overlap.
 * The call synchronises once and reuses the operators' scratch: cloud_big and the sort workspace are left alone. */
#define O3DR_INTERPOLATE_MAX_SMOOTH 8
#define O3DR_INTERPOLATE_MAX_LEVELS 32
typedef struct o3dr_interpolate_params {
    int32_t width, height;  /* no default (0 x 0 is rejected) */
    int32_t smooth;         /* 2: Jacobi sweeps per level, 0..8 */
    int32_t max_level;      /* 0: no limit; 1..31: cells of a higher level stay NaN */
} o3dr_interpolate_params;
typedef struct o3dr_interpolate_outputs {
    float* filled;          /* width * height */
    uint8_t* level;         /* width * height, may be NULL */
} o3dr_interpolate_outputs;
typedef struct o3dr_interpolate_result {
    int32_t width, height, n_levels, reserved;
    int64_t n_data, n_filled, n_empty;
    int64_t n_by_level[O3DR_INTERPOLATE_MAX_LEVELS];
} o3dr_interpolate_result;
void o3dr_interpolate_default_params(o3dr_interpolate_params* p);
int  o3dr_raster_interpolate(o3dr_ctx* ctx, const float* raster, const o3dr_interpolate_params* p,
                             const o3dr_interpolate_outputs* out, o3dr_interpolate_result* res, int32_t mem);

/* ---- raster sample: a raster read back at every point of a cloud, and the point's height above it.
 *   1. Cells and box: the map raster's step 1 (o3dr.h): inv = 1.0f / (float)cell_size, cx = (int)floorf(x * inv), cy
 *      likewise; element [r, c] of `raster` (float32 [height, width]) is cell (cx0 + c, cy0 + r).
 *   2. value[i] = the raster at point i's cell, copied; 0x7fc00000 for a point outside the box or on a NaN cell.
 *      height_above[i] = z_i - value[i] in fp32, or that NaN where value[i] is NaN: with the ground filter's own DTM it is the
 *      filter's height_above_ground.  Either output may be NULL.
 *   3. counts (may be NULL): [0] the points inside the box, [1] the points outside it, [2] the points inside it on a NaN
 *      cell; counts[0] + counts[1] = n.
 * Errors, O3DR_ERR_INVALID_ARG, in this order: raster is NULL; a bad mem; cell_size (as for the raster); a box with a side
 * < 1 or a corner outside int32; the cloud (pointer / size, n < 2^31; a non-finite coordinate, a cell index outside int32);
 * a box of more than 2^28 cells.  On an error the host outputs and counts are zeroed.  n == 0 is allowed.  `raster`, the
 * cloud and the outputs live in the one memory kind `mem`.  The call synchronises and reuses the operators' scratch. */
int  o3dr_raster_sample(o3dr_ctx* ctx, const o3dr_point* cloud, int64_t n, double cell_size, int32_t cx0, int32_t cy0,
                        int32_t width, int32_t height, const float* raster, float* value, float* height_above,
                        int64_t counts[3], int32_t mem);

#ifdef __cplusplus
}
#endif
#endif
