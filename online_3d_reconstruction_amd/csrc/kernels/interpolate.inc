// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Raster interpolation and raster sample (o3dr_raster_interpolate, o3dr_raster_sample; contract: include/o3dr_dem.h,
// DESIGN.md "Raster interpolation")
//   The contract defines every value per cell, so the tiling is free.  Level 0 is the input (a cell's count is its NaN
//   test); the levels 1 .. L are (cnt, val) arrays one after the other.
//   k_interp_pull   a 32 x 32 tile of level `base` in LDS per workgroup turn, and from it the tile's cells of up to five
//                   levels: tiles start on multiples of 32, so every descendant of a cell of those levels is in the tile.
//   k_interp_top    one workgroup: the pulls above the tiled ones from global memory (32 x 32 cells at most), then the
//                   pushes of every level that fits in one 64 x 64 region, each with its sweeps in LDS.
//   k_interp_push   one level, tiled: a workgroup fills its tile plus an apron of `smooth` cells (64 x 64 with the apron)
//                   from level l + 1 and sweeps it in LDS.  A cell d cells inside the region's border that is not the
//                   level's border is right after k <= d sweeps (a wrong value moves one cell a sweep), so the tile is
//                   right after all of them; the region's cells are all swept every time, which is simpler than a
//                   shrinking region and costs (64 / tile)^2.  It writes the cells with c_l = 0 only: val keeps m_l on
//                   the others, which is F_l there, and nobody reads val on a cell with c_l = 0 before the level is done.
//                   Level 0 writes the outputs and counts: n_data and the fills in registers, the holes' levels by LDS
//                   atomics, one partial of kInterpPartWords words per workgroup, folded by k_interp_fold.
//   k_raster_sample one pass over the points, k_ground_points without the mask.
// =================================================================================================
constexpr int kInterpThreads = kFoldThreads;  // (block_reduce4_u32)
static_assert(kInterpThreads == 4 * kInterpRegion, "four rows of a region per workgroup step");
static_assert(kInterpRegion == 2 * kInterpPullTile, "the level above a region-sized level is a pull tile");
static_assert(kInterpPartWords >= O3DR_INTERPOLATE_MAX_LEVELS + 2 && kInterpPartWords % 4 == 0, "n_by_level, n_filled, n_empty");

struct InterpTile {
    float v[2][kInterpRegion * kInterpRegion];  // the region's values, this sweep's and the one's before
    uint8_t fix[kInterpRegion * kInterpRegion];  // 1: c_l > 0
};

// (c, m) of cell (x, y) of level l; outside the level, and on a cell without data, c = 0 and m = +0.0f
template <bool CHECK>
__device__ __forceinline__ void interp_cell(const InterpArgs& a, int l, int64_t x, int64_t y, int32_t& c, float& m)
{
    c = 0, m = 0.f;
    const int64_t W = a.lv[l].W, H = a.lv[l].H;
    if (x >= W || y >= H) return;
    if (l == 0) {
        const float z = a.raster[y * W + x];
        if (z == z) c = 1, m = z;
        if (CHECK && (z == __builtin_inff() || z == -__builtin_inff())) *a.bad = 1u;  // (every writer stores the same value)
    } else {
        const int64_t id = a.lv[l].off + y * W + x;
        c = a.cnt[id];
        if (c > 0) m = a.val[id];
    }
}

// the contract's step 2 on the four children in their order
__device__ __forceinline__ void interp_pull4(const int32_t c[4], const float m[4], int32_t& n, float& mm)
{
    n = ((c[0] + c[1]) + c[2]) + c[3];
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) s = s + (double)c[k] * (double)m[k];
    mm = n > 0 ? (float)(s / (double)n) : 0.f;
}

// the contract's step 4 for a cell with c_l = 0, l < L: from the four parents in val
__device__ __forceinline__ float interp_push_value(const InterpArgs& a, int l, int64_t x, int64_t y)
{
    const int64_t W = a.lv[l + 1].W, H = a.lv[l + 1].H;
    const int64_t X = x >> 1, Y = y >> 1;
    int64_t Xn = (x & 1) ? X + 1 : X - 1, Yn = (y & 1) ? Y + 1 : Y - 1;
    Xn = Xn < 0 ? 0 : Xn > W - 1 ? W - 1 : Xn;
    Yn = Yn < 0 ? 0 : Yn > H - 1 ? H - 1 : Yn;
    const float* F = a.val + a.lv[l + 1].off;
    const double pa = (double)F[Y * W + X], pb = (double)F[Y * W + Xn], pc = (double)F[Yn * W + X], pd = (double)F[Yn * W + Xn];
    return (float)((((9.0 * pa + 3.0 * pb) + 3.0 * pc) + pd) * 0.0625);
}

__global__ __launch_bounds__(kInterpThreads) void k_interp_pull(InterpArgs a, int base, int nl, int64_t tiles_x, int64_t tiles)
{
    constexpr int T = kInterpPullTile;
    __shared__ __attribute__((aligned(8))) int32_t sc[2][T * T];
    __shared__ __attribute__((aligned(8))) float sm[2][T * T];
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t x0 = (tile % tiles_x) * T, y0 = (tile / tiles_x) * T;
        for (int i = threadIdx.x; i < T * T; i += kInterpThreads)
            interp_cell<true>(a, base, x0 + i % T, y0 + i / T, sc[0][i], sm[0][i]);
        __syncthreads();
        int side = T;  // cells a side of the level in LDS
        for (int k = 1; k <= nl; ++k) {
            const int src = (k - 1) & 1, dst = k & 1, half = side >> 1;
            const int64_t W = a.lv[base + k].W, H = a.lv[base + k].H, off = a.lv[base + k].off;
            for (int i = threadIdx.x; i < half * half; i += kInterpThreads) {
                const int lx = i % half, ly = i / half;
                const int2 c0 = *reinterpret_cast<const int2*>(&sc[src][(2 * ly) * side + 2 * lx]);
                const int2 c1 = *reinterpret_cast<const int2*>(&sc[src][(2 * ly + 1) * side + 2 * lx]);
                const float2 m0 = *reinterpret_cast<const float2*>(&sm[src][(2 * ly) * side + 2 * lx]);
                const float2 m1 = *reinterpret_cast<const float2*>(&sm[src][(2 * ly + 1) * side + 2 * lx]);
                const int32_t c[4] = {c0.x, c0.y, c1.x, c1.y};
                const float m[4] = {m0.x, m0.y, m1.x, m1.y};
                int32_t n;
                float mm;
                interp_pull4(c, m, n, mm);
                sc[dst][ly * half + lx] = n;
                sm[dst][ly * half + lx] = mm;
                const int64_t X = (x0 >> k) + lx, Y = (y0 >> k) + ly;
                if (X < W && Y < H) {
                    a.cnt[off + Y * W + X] = n;
                    a.val[off + Y * W + X] = mm;
                }
            }
            __syncthreads();
            side = half;
        }
    }
}

// The region [rx0, rx0 + rw) x [ry0, ry0 + rh) of level l (inside the level, at most kInterpRegion a side): F_l before the
// sweeps, then a.smooth sweeps over all of it, a neighbour outside the region taken as one outside the level.  Returns the
// buffer of t.v that holds the result; the workgroup is synchronised.
__device__ __forceinline__ int interp_push_region(const InterpArgs& a, int l, int64_t rx0, int64_t ry0, int rw, int rh, InterpTile& t)
{
    constexpr int R = kInterpRegion;
    const int lx = threadIdx.x & (R - 1), ly0 = threadIdx.x / R;
    for (int ly = ly0; ly < rh; ly += kInterpThreads / R) {
        if (lx >= rw) continue;
        int32_t c;
        float m;
        interp_cell<false>(a, l, rx0 + lx, ry0 + ly, c, m);
        if (c == 0 && l < a.L) m = interp_push_value(a, l, rx0 + lx, ry0 + ly);
        t.v[0][ly * R + lx] = m;
        t.fix[ly * R + lx] = c > 0 ? 1 : 0;
    }
    __syncthreads();
    int cur = 0;
    for (int k = 0; k < a.smooth; ++k) {
        const float* in = t.v[cur];
        float* out = t.v[cur ^ 1];
        for (int ly = ly0; ly < rh; ly += kInterpThreads / R) {
            if (lx >= rw) continue;
            const int i = ly * R + lx;
            float z = in[i];
            if (!t.fix[i]) {
                int n = 0;
                double up = 0.0, left = 0.0, right = 0.0, down = 0.0;
                if (ly > 0) up = (double)in[i - R], ++n;
                if (lx > 0) left = (double)in[i - 1], ++n;
                if (lx + 1 < rw) right = (double)in[i + 1], ++n;
                if (ly + 1 < rh) down = (double)in[i + R], ++n;
                const double s = ((up + left) + right) + down;
                if (n > 0) z = (float)(s / (double)n);
            }
            out[i] = z;
        }
        __syncthreads();
        cur ^= 1;
    }
    return cur;
}

// One workgroup.  The levels pulled + 1 .. L from the level below in global memory, then the pushes of the levels
// L - 1 .. max(lt, 1): each is one region.
__global__ __launch_bounds__(kInterpThreads) void k_interp_top(InterpArgs a, int pulled, int lt)
{
    __shared__ InterpTile t;
    for (int l = pulled + 1; l <= a.L; ++l) {
        const int W = a.lv[l].W, H = a.lv[l].H;
        const int64_t off = a.lv[l].off;
        for (int i = threadIdx.x; i < W * H; i += kInterpThreads) {
            const int X = i % W, Y = i / W;
            int32_t c[4], n;
            float m[4], mm;
#pragma unroll
            for (int k = 0; k < 4; ++k) interp_cell<true>(a, l - 1, 2 * X + (k & 1), 2 * Y + (k >> 1), c[k], m[k]);
            interp_pull4(c, m, n, mm);
            a.cnt[off + i] = n;
            a.val[off + i] = mm;
        }
        __syncthreads();  // (the next level reads this one: one workgroup, one CU)
    }
    constexpr int R = kInterpRegion;
    const int lx = threadIdx.x & (R - 1), ly0 = threadIdx.x / R;
    for (int l = a.L - 1; l >= (lt > 1 ? lt : 1); --l) {
        const int W = a.lv[l].W, H = a.lv[l].H;
        const int cur = interp_push_region(a, l, 0, 0, W, H, t);
        for (int ly = ly0; ly < H; ly += kInterpThreads / R)
            if (lx < W && !t.fix[ly * R + lx]) a.val[a.lv[l].off + (int64_t)ly * W + lx] = t.v[cur][ly * R + lx];
        __syncthreads();  // (the level below reads this one; t is reused)
    }
}

// level l, one tile of (kInterpRegion - 2 smooth)^2 cells per workgroup turn; LEVEL0: the outputs and the counts
template <bool LEVEL0>
__global__ __launch_bounds__(kInterpThreads) void k_interp_push(InterpArgs a, int l, int64_t tiles_x, int64_t tiles)
{
    constexpr int R = kInterpRegion;
    __shared__ InterpTile t;
    __shared__ uint32_t hist[kInterpPartWords];
    const int T = R - 2 * a.smooth, lx = threadIdx.x & (R - 1), ly0 = threadIdx.x / R;
    const int64_t W = a.lv[l].W, H = a.lv[l].H;
    uint32_t n_data = 0, n_filled = 0, n_empty = 0;
    if (LEVEL0) {
        if (threadIdx.x < kInterpPartWords) hist[threadIdx.x] = 0;
        __syncthreads();
    }
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t ox0 = (tile % tiles_x) * T, oy0 = (tile / tiles_x) * T;
        const int64_t ox1 = ox0 + T < W ? ox0 + T : W, oy1 = oy0 + T < H ? oy0 + T : H;
        const int64_t rx0 = ox0 - a.smooth > 0 ? ox0 - a.smooth : 0, ry0 = oy0 - a.smooth > 0 ? oy0 - a.smooth : 0;
        const int64_t rx1 = ox1 + a.smooth < W ? ox1 + a.smooth : W, ry1 = oy1 + a.smooth < H ? oy1 + a.smooth : H;
        const int cur = interp_push_region(a, l, rx0, ry0, (int)(rx1 - rx0), (int)(ry1 - ry0), t);
        const int64_t x = rx0 + lx;
        for (int ly = ly0; ly < (int)(ry1 - ry0); ly += kInterpThreads / R) {
            const int64_t y = ry0 + ly;
            if (x < ox0 || x >= ox1 || y < oy0 || y >= oy1) continue;
            const int i = ly * R + lx;
            const bool fixed = t.fix[i] != 0;
            const float z = t.v[cur][i];
            if (!LEVEL0) {
                if (!fixed) a.val[a.lv[l].off + y * W + x] = z;
                continue;
            }
            int lev = fixed ? 0 : 255;
            for (int ll = 1; ll <= a.L && __any(lev == 255); ++ll)
                if (lev == 255 && a.cnt[a.lv[ll].off + (y >> ll) * a.lv[ll].W + (x >> ll)] > 0) lev = ll;
            const bool empty = lev == 255 || (a.max_level > 0 && lev > a.max_level);
            a.filled[y * W + x] = empty ? __builtin_nanf("") : z;  // (a data cell: the input's bits)
            if (a.level) a.level[y * W + x] = (uint8_t)lev;
            if (fixed) {
                ++n_data;
            } else {
                if (lev < O3DR_INTERPOLATE_MAX_LEVELS) atomicAdd(&hist[lev], 1u);
                ++(empty ? n_empty : n_filled);
            }
        }
        __syncthreads();  // (t is reused)
    }
    if (LEVEL0) {
        if (n_data) atomicAdd(&hist[0], n_data);
        if (n_filled) atomicAdd(&hist[O3DR_INTERPOLATE_MAX_LEVELS], n_filled);
        if (n_empty) atomicAdd(&hist[O3DR_INTERPOLATE_MAX_LEVELS + 1], n_empty);
        __syncthreads();
        if (threadIdx.x < kInterpPartWords) a.part[(int64_t)blockIdx.x * kInterpPartWords + threadIdx.x] = hist[threadIdx.x];
    }
}

// one workgroup: the kInterpPartWords-word partials of `blocks` workgroups summed into out
__global__ __launch_bounds__(kFoldThreads) void k_interp_fold(const uint32_t* __restrict__ part, int blocks, uint32_t* __restrict__ out)
{
    const int op[4] = {2, 2, 2, 2};
    for (int w = 0; w < kInterpPartWords; w += 4) {
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        for (int b = threadIdx.x; b < blocks; b += kFoldThreads)
            for (int k = 0; k < 4; ++k) v[k] += part[(int64_t)b * kInterpPartWords + w + k];
        block_reduce4_u32(v, op, out + w);
    }
}

// per point: the raster at its cell and the height above it.  Per workgroup: points inside the box, outside, on a NaN cell.
__global__ __launch_bounds__(kInterpThreads) void k_raster_sample(SampleArgs a)
{
    uint32_t inside = 0, outside = 0, on_nan = 0;
    for (int64_t i = (int64_t)blockIdx.x * kInterpThreads + threadIdx.x; i < (int64_t)a.f.n; i += (int64_t)gridDim.x * kInterpThreads) {
        const float4 p = reinterpret_cast<const float4*>(a.f.cloud)[i];
        const int64_t id = frame_cell(a.f, p);
        float v = __builtin_nanf(""), h = __builtin_nanf("");
        if (id >= 0) {
            ++inside;
            const float d = a.raster[id];
            if (d == d)
                v = d, h = p.z - d;  // (a NaN cell: the one NaN of every output, not the cell's own or the subtraction's)
            else
                ++on_nan;
        } else {
            ++outside;
        }
        if (a.value) a.value[i] = v;
        if (a.hag) a.hag[i] = h;
    }
    uint32_t cnt[4] = {inside, outside, on_nan, 0u};
    const int op[4] = {2, 2, 2, 2};
    block_reduce4_u32(cnt, op, a.f.part + (int64_t)blockIdx.x * kPartWords);
}
