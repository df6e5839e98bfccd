// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Ground filter (o3dr_ground_filter; contract: include/o3dr_terrain.h, DESIGN.md "Ground filter")
//   Minimum surface: k_raster_winner (select = BOTTOM) leaves the cells' words; k_ground_init copies every occupied
//   cell's z into zl and sets the states.  zl is "Z on the live cells": +inf for an empty or a removed cell, so a window
//   minimum over zl is the minimum over L, and -inf plays the same part for the maxima (every z is finite).
//   Iteration k, radius r, four passes over fp32 rasters:
//     k_ground_row<min>   t1 = min of zl over |dx| <= r      a row segment with an r-wide apron in LDS, window minima by
//     k_ground_col_*      t2 = min of t1 over |dy| <= r      doubling: M_p[i] = min x[i .. i + p - 1] for the largest power
//     k_ground_row<max>   t1 = max of t2 over |dx| <= r      of two p <= 2r + 1 in log2 p steps, the window = two of them
//     k_ground_col_*      O  = max of t1 over |dy| <= r      that overlap.
//   A column pass is van Herk / Gil-Werman over blocks of w = 2r + 1 rows with the threads along x, every access a
//   coalesced row segment: k_ground_col_suffix walks each block upwards and stores its suffix minima (run); the second
//   kernel walks the outputs y = B w + r + i downwards with the prefix minimum of block B + 1 in a register, so the window
//   [y - r, y + r] is min(run[y - r], prefix).  Work per cell: log2 p in a row pass, constant in a column pass.
//   k_ground_col_min writes E masked to L (-inf elsewhere); k_ground_col_max does not store O: it compares, writes the
//   new state and zl = +inf, and leaves the removed count in per-workgroup partials (k_fold4_u32).
//   DTM: k_ground_ground_words sets the word of every cell that is not ground to empty, and the raster's own fill passes
//   (k_raster_fill_col, k_raster_resolve) give the DTM and its counts: the nearest-cell rule lives in raster.inc alone.
//   k_ground_points is the one pass over the points.
// =================================================================================================
constexpr int kGroundThreads = kFoldThreads;  // (block_reduce4_u32)
static_assert(kGroundTileW == kGroundThreads, "one thread per cell of a row segment");
static_assert(2 * O3DR_GROUND_MAX_WINDOW_RADIUS <= kGroundTileW, "two loads per thread fill a segment with its apron");

template <bool MAX>
__device__ __forceinline__ float ground_ident()
{
    return MAX ? -__builtin_inff() : __builtin_inff();
}
template <bool MAX>
__device__ __forceinline__ float ground_op(float a, float b)
{
    return MAX ? fmaxf(a, b) : fminf(a, b);
}

// per cell: zl = the z of its word's point (+inf: empty), state = 1 / 0
__global__ __launch_bounds__(kGroundThreads) void k_ground_init(GroundArgs a)
{
    const int64_t cells = (int64_t)a.r.f.width * a.r.f.height;
    const int64_t id = (int64_t)blockIdx.x * kGroundThreads + threadIdx.x;
    if (id >= cells) return;
    const unsigned long long w = a.r.win[id];
    const bool occupied = w != kRasterEmpty;
    a.zl[id] = occupied ? reinterpret_cast<const float4*>(a.r.f.cloud)[raster_index(w)].z : __builtin_inff();
    a.state[id] = occupied ? 1 : 0;
}

// one row segment of kGroundTileW cells per workgroup: out = min / max of in over |dx| <= r inside the raster
template <bool MAX>
__global__ __launch_bounds__(kGroundThreads) void k_ground_row(const float* __restrict__ in, float* __restrict__ out, int32_t width,
                                                              int64_t tiles_x, int r, int p)
{
    __shared__ float seg[kGroundTileW + 2 * O3DR_GROUND_MAX_WINDOW_RADIUS];
    const int64_t row = (int64_t)blockIdx.x / tiles_x, c0 = ((int64_t)blockIdx.x % tiles_x) * kGroundTileW;
    const int n_el = kGroundTileW + 2 * r, t = threadIdx.x;
    const float* src = in + row * width;
    float v[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {  // columns c0 - r .. c0 + kGroundTileW + r - 1, outside the raster = the identity
        const int j = t + k * kGroundThreads;
        const int64_t cc = c0 - r + j;
        v[k] = (j < n_el && cc >= 0 && cc < width) ? src[cc] : ground_ident<MAX>();
        if (j < n_el) seg[j] = v[k];
    }
    __syncthreads();
    for (int s = 1; s < p; s <<= 1) {  // seg[j] = op over in[j .. j + 2s - 1]; an element short of its span is never read
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int j = t + k * kGroundThreads;
            if (j + s < n_el) v[k] = ground_op<MAX>(v[k], seg[j + s]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int j = t + k * kGroundThreads;
            if (j < n_el) seg[j] = v[k];
        }
        __syncthreads();
    }
    if (c0 + t < width) out[row * width + c0 + t] = ground_op<MAX>(seg[t], seg[t + 2 * r + 1 - p]);
}

// the workgroup's column group and first row block of a column pass (ground_col_groups x ground_col_rows workgroups)
__device__ __forceinline__ void ground_col_place(int64_t groups_x, int64_t& x, int64_t& b0, int64_t& stride)
{
    x = ((int64_t)blockIdx.x % groups_x) * kGroundThreads + threadIdx.x;
    b0 = (int64_t)blockIdx.x / groups_x;
    stride = (int64_t)gridDim.x / groups_x;
}

// per block of w = 2r + 1 rows and column: run[y] = min / max of in over the rows y .. the block's last
template <bool MAX>
__global__ __launch_bounds__(kGroundThreads) void k_ground_col_suffix(const float* __restrict__ in, float* __restrict__ run, int32_t width,
                                                                     int32_t height, int64_t groups_x, int r)
{
    int64_t x, b0, stride;
    ground_col_place(groups_x, x, b0, stride);
    if (x >= width) return;
    const int64_t w = 2 * (int64_t)r + 1;
    for (int64_t B = b0; B * w < height; B += stride) {
        const int64_t y0 = B * w, y1 = y0 + w < height ? y0 + w : (int64_t)height;
        float m = ground_ident<MAX>();
#pragma unroll 4
        for (int64_t y = y1 - 1; y >= y0; --y) {
            m = ground_op<MAX>(m, in[y * width + x]);
            run[y * width + x] = m;
        }
    }
}

// The outputs y = B w + r + i, i = 0 .. w - 1, of row block B = -1, 0, ...: the window [y - r, y + r] is the rows
// B w + i .. of block B (run[y - r]) and the first i rows of block B + 1 (m).  FINAL = false: t2 = that minimum on the live
// cells, -inf elsewhere.  FINAL = true: the maximum is O; a live cell with Z - O > thr gets state `code` and leaves L.
template <bool FINAL>
__global__ __launch_bounds__(kGroundThreads) void k_ground_col_window(GroundArgs a, const float* __restrict__ in, int64_t groups_x, int r,
                                                                     float thr, uint8_t code)
{
    constexpr bool MAX = FINAL;
    int64_t x, b0, stride;
    ground_col_place(groups_x, x, b0, stride);
    const int64_t width = a.r.f.width, height = a.r.f.height, w = 2 * (int64_t)r + 1;
    uint32_t removed = 0;
    if (x < width) {
        for (int64_t B = b0 - 1; B * w + r < height; B += stride) {
            float m = ground_ident<MAX>();
#pragma unroll 4
            for (int64_t i = 0; i < w; ++i) {
                const int64_t y = B * w + r + i, yt = y + r, yb = y - r;
                if (i > 0 && yt < height) m = ground_op<MAX>(m, in[yt * width + x]);
                if (y < 0) continue;
                if (y >= height) break;
                const int64_t id = y * width + x;
                const float v = yb >= 0 ? ground_op<MAX>(m, a.run[yb * width + x]) : m;
                const float z = a.zl[id];
                const bool live = z != __builtin_inff();
                if (!FINAL) {
                    a.t2[id] = live ? v : -__builtin_inff();
                } else if (live && z - v > thr) {
                    a.state[id] = code;
                    a.zl[id] = __builtin_inff();
                    ++removed;
                }
            }
        }
    }
    if (FINAL) {
        uint32_t cnt[4] = {removed, 0u, 0u, 0u};
        const int op[4] = {2, 2, 2, 2};
        block_reduce4_u32(cnt, op, a.r.f.part + (int64_t)blockIdx.x * kPartWords);
    }
}

// per cell that is not ground: its word set to empty (the DTM's sources are the ground cells)
__global__ __launch_bounds__(kGroundThreads) void k_ground_ground_words(GroundArgs a)
{
    const int64_t cells = (int64_t)a.r.f.width * a.r.f.height;
    const int64_t id = (int64_t)blockIdx.x * kGroundThreads + threadIdx.x;
    if (id < cells && a.state[id] != 1) a.r.win[id] = kRasterEmpty;
}

// per point: the mask and the height above the DTM.  Per workgroup: ground points.
__global__ __launch_bounds__(kGroundThreads) void k_ground_points(GroundArgs a)
{
    const RasterFrame& f = a.r.f;
    const float thr0 = a.thr[0];
    uint32_t n_ground = 0;
    for (int64_t i = (int64_t)blockIdx.x * kGroundThreads + threadIdx.x; i < (int64_t)f.n; i += (int64_t)gridDim.x * kGroundThreads) {
        const float4 p = reinterpret_cast<const float4*>(f.cloud)[i];
        const int64_t id = frame_cell(f, p);
        uint8_t g = 0;
        float h = __builtin_nanf("");
        if (id >= 0) {
            const float d = a.r.height_map[id];
            if (d == d) h = p.z - d;  // (a cell without a value: the one NaN of every output, not the subtraction's)
            g = (a.state[id] == 1 && h <= thr0) ? 1 : 0;  // a ground cell's DTM is its Z
        }
        n_ground += g;
        if (a.ground) a.ground[i] = g;
        if (a.hag) a.hag[i] = h;
    }
    uint32_t v[4] = {n_ground, 0u, 0u, 0u};
    const int op[4] = {2, 2, 2, 2};
    block_reduce4_u32(v, op, a.r.f.part + (int64_t)blockIdx.x * kPartWords);
}
