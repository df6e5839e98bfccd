// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Map raster (o3dr_rasterize_map; contract: include/o3dr.h, DESIGN.md "Map raster")
//   Cells: the caller's box as a RasterFrame (frame_cell in cell_order.inc).  One 64-bit word per cell holds the chosen point as
//   (z key << 32 | input index), all ones = empty, and k_raster_winner folds every point of the box into its cell's word
//   with an integer atomicMin: the minimum of a set does not depend on the order of arrival, so the choice is exact.  The
//   z key is 0 (FIRST), the order-preserving integer of z (BOTTOM) or its complement (TOP), -0.0f taken as 0.0f.
//   Hole fill, separable: k_raster_fill_col keeps per cell the signed offset in cy of the nearest occupied cell of its
//   column within R (the lower cy on a tie); k_raster_resolve minimises dx*dx + g*g over |dx| <= R from an LDS tile of
//   these offsets with an R-wide apron, ties to the lower cy, then the lower cx.  If an occupied cell wins for a target,
//   its column's candidate is at most as far and wins ties against it, so it is that cell: the result is the plain
//   search over the disc.  k_raster_resolve also gathers the four output images and counts the cells;
//   k_raster_shade is the stencil on the filled heights.  All counts are per-workgroup partials folded by one workgroup
//   (k_fold4_u32).
// =================================================================================================
constexpr int kRasterThreads = kFoldThreads;  // (block_reduce4_u32)
constexpr int kRasterNone = -128;             // k_raster_fill_col: no occupied cell within R in this column
constexpr int kRasterApron = O3DR_RASTER_MAX_FILL_RADIUS;
constexpr unsigned long long kRasterEmpty = ~0ull;
static_assert(kRasterTileW * kRasterTileH == kRasterThreads, "one thread per cell of the tile");
static_assert(kRasterTileW + 2 * kRasterApron <= 2 * kRasterTileW, "two loads per thread fill a tile row");

// the input index of a cell's word (-1: empty; the index is below 2^31)
__device__ __forceinline__ int32_t raster_index(unsigned long long w) { return (int32_t)(uint32_t)w; }

// per point inside the box: its cell's word takes the minimum of (z key, index).  Per workgroup: points inside, outside.
__global__ __launch_bounds__(kRasterThreads) void k_raster_winner(RasterArgs a)
{
    uint32_t inside = 0, outside = 0;
    for (int64_t i = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x; i < (int64_t)a.f.n; i += (int64_t)gridDim.x * kRasterThreads) {
        const float4 p = reinterpret_cast<const float4*>(a.f.cloud)[i];
        const int64_t id = frame_cell(a.f, p);
        if (id < 0) {
            ++outside;
            continue;
        }
        ++inside;
        const uint32_t zo = f32_ordered(p.z == 0.f ? 0.f : p.z);  // both zeros -> one key
        const uint32_t zk = a.select == O3DR_RASTER_TOP ? ~zo : a.select == O3DR_RASTER_BOTTOM ? zo : 0u;
        atomicMin(a.win + id, ((unsigned long long)zk << 32) | (unsigned long long)(uint32_t)i);
    }
    uint32_t v[4] = {inside, outside, 0u, 0u};
    const int op[4] = {2, 2, 2, 2};
    block_reduce4_u32(v, op, a.f.part + (int64_t)blockIdx.x * kPartWords);
}

// per cell: the offset in cy of the nearest occupied cell of its column within R, the lower cy on a tie (0: its own)
__global__ __launch_bounds__(kRasterThreads) void k_raster_fill_col(RasterArgs a)
{
    const int64_t cells = (int64_t)a.f.width * a.f.height;
    const int64_t id = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
    if (id >= cells) return;
    const int64_t r = id / a.f.width;
    int g = kRasterNone;
    if (a.win[id] != kRasterEmpty) g = 0;
    for (int k = 1; g == kRasterNone && k <= a.R; ++k) {
        if (r - k >= 0 && a.win[id - (int64_t)k * a.f.width] != kRasterEmpty) g = -k;
        else if (r + k < a.f.height && a.win[id + (int64_t)k * a.f.width] != kRasterEmpty) g = k;
    }
    a.col[id] = (int8_t)g;
}

// per cell of a kRasterTileW x kRasterTileH tile: its source (own, filled or none), the four output images and the counts
__global__ __launch_bounds__(kRasterThreads) void k_raster_resolve(RasterArgs a)
{
    __shared__ int8_t tile[kRasterTileH][kRasterTileW + 2 * kRasterApron];
    const int64_t tiles_x = ((int64_t)a.f.width + kRasterTileW - 1) / kRasterTileW;
    const int64_t c0 = ((int64_t)blockIdx.x % tiles_x) * kRasterTileW, r0 = ((int64_t)blockIdx.x / tiles_x) * kRasterTileH;
    const int tx = threadIdx.x % kRasterTileW, ty = threadIdx.x / kRasterTileW;
    const int64_t c = c0 + tx, r = r0 + ty;
    const bool valid = c < a.f.width && r < a.f.height;
    const int R = a.R;
    if (R > 0) {  // the tile's rows with the apron: columns c0 - R .. c0 + kRasterTileW + R - 1, outside the raster = none
        for (int j = tx; j < kRasterTileW + 2 * R; j += kRasterTileW) {
            const int64_t cc = c0 - R + j;
            tile[ty][j] = (r < a.f.height && cc >= 0 && cc < a.f.width) ? a.col[r * a.f.width + cc] : (int8_t)kRasterNone;
        }
        __syncthreads();
    }
    int32_t src = -1, d2 = -1;
    float h = __builtin_nanf("");
    if (valid) {
        const int64_t id = r * a.f.width + c;
        const unsigned long long own = a.win[id];
        if (own != kRasterEmpty) {
            src = raster_index(own), d2 = 0;
        } else if (R > 0) {
            int best = R * R + 1, best_g = 0, best_dx = 0;
            for (int dx = -R; dx <= R; ++dx) {  // ascending cx: a later candidate must be nearer, or as near with a lower cy
                const int g = tile[ty][tx + R + dx];
                if (g == kRasterNone) continue;
                const int d = dx * dx + g * g;
                if (d < best || (d == best && d <= R * R && g < best_g)) best = d, best_g = g, best_dx = dx;
            }
            if (best <= R * R) {
                src = raster_index(a.win[id + (int64_t)best_g * a.f.width + best_dx]);
                d2 = best;
            }
        }
        uint32_t rgba = 0u;
        if (src >= 0) {
            const float4 p = reinterpret_cast<const float4*>(a.f.cloud)[src];
            h = p.z, rgba = __float_as_uint(p.w);
        }
        if (a.source) a.source[id] = src;
        if (a.distance2) a.distance2[id] = d2;
        if (a.height_map) a.height_map[id] = h;
        if (a.color) {
            uint8_t* dst = a.color + id * 3;
            dst[0] = (uint8_t)rgba, dst[1] = (uint8_t)(rgba >> 8), dst[2] = (uint8_t)(rgba >> 16);
        }
    }
    uint32_t* out = a.f.part + (int64_t)blockIdx.x * kPartWords;
    uint32_t v[4] = {d2 == 0 ? 1u : 0u, d2 > 0 ? 1u : 0u, (valid && d2 < 0) ? 1u : 0u, 0u};
    const int op[4] = {2, 2, 2, 2};
    block_reduce4_u32(v, op, out);
    uint32_t zmin = 0xffffffffu, zmax = 0u;
    if (d2 == 0) zmin = zmax = f32_ordered(h == 0.f ? 0.f : h);
    uint32_t z[4] = {zmin, zmax, 0u, 0u};
    const int opz[4] = {0, 1, 2, 2};
    block_reduce4_u32(z, opz, out + 4);
}

// per cell with a source: the shaded relief of the contract from the heights after the fill (a height is NaN exactly
// where there is no source: every z of the cloud is finite)
__global__ __launch_bounds__(kRasterThreads) void k_raster_shade(RasterArgs a)
{
    const int64_t cells = (int64_t)a.f.width * a.f.height;
    const int64_t id = (int64_t)blockIdx.x * kRasterThreads + threadIdx.x;
    if (id >= cells) return;
    const int64_t r = id / a.f.width, c = id - r * a.f.width;
    const float h = a.height_map[id];
    if (h != h) {
        a.shade[id] = 0;
        return;
    }
    float hL = h, hR = h, hD = h, hU = h;
    int kx = 0, ky = 0;
    if (c > 0) {
        const float t = a.height_map[id - 1];
        if (t == t) hL = t, ++kx;
    }
    if (c + 1 < a.f.width) {
        const float t = a.height_map[id + 1];
        if (t == t) hR = t, ++kx;
    }
    if (r > 0) {
        const float t = a.height_map[id - a.f.width];
        if (t == t) hD = t, ++ky;
    }
    if (r + 1 < a.f.height) {
        const float t = a.height_map[id + a.f.width];
        if (t == t) hU = t, ++ky;
    }
    const double gx = kx == 0 ? 0.0 : ((double)hR - (double)hL) / ((double)kx * a.cell_size);
    const double gy = ky == 0 ? 0.0 : ((double)hU - (double)hD) / ((double)ky * a.cell_size);
    const double s = (((-gx) * a.light[0] + (-gy) * a.light[1]) + a.light[2]) / sqrt((gx * gx + gy * gy) + 1.0);
    int v = 1;
    if (s > 0.0) {
        const double t = floor(s * 254.0 + 0.5);
        v = t >= 254.0 ? 255 : 1 + (int)t;
    }
    a.shade[id] = (uint8_t)v;
}
