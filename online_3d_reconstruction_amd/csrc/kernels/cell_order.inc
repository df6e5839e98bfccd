// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// The dense XY cell order of a cloud (CellOrder in o3dr_device.h; DESIGN.md "Cell order"): what plane segmentation
// (tiles) and the surface mesh (cells) start with.
//   A CELL FUNCTOR is the operator's index rule: bool operator()(const float4& p, int32_t& ix, int32_t& iy), false when
//   an index leaves int32 (PlaneCell in plane.inc, FloorCell below; the arithmetic is part of the ABI contract).
//   k_cell_range: the index box, kept order-preserving as int32 ^ 0x80000000, and "an index leaves int32", as
//   per-workgroup partials folded by one workgroup (k_fold4_u32): no atomics.  The host reads the box back (cell_box in
//   o3dr_api.hip) and checks that the dense id (iy - y0) * wx + (ix - x0) fits a 32-bit sort key.
//   k_cell_keys writes that id per point; the stable radix sort orders the points by (iy, ix), input order kept inside a
//   cell (launch_sort_keys, payload = input position); k_cell_heads flags the first point of every cell and the scan of
//   the flags numbers the cells (ordinals, in cell order; their count is the run count).
//   What is gathered into that order is the operator's business (k_plane_gather, k_mesh_vertices).
//   The raster family does not sort: its box is the caller's (RasterFrame in o3dr_device.h; DESIGN.md "Raster frame"), the
//   range pass only proves that every index fits int32, and frame_cell is the dense id of a point's cell in that box.
// =================================================================================================
constexpr int kCellThreads = kFoldThreads;

// the contract's cell index floorf(x * inv) with inv = 1.0f / (float)cell_size, in fp32: the cell functor of the surface
// mesh, the map raster, the ground filter and the raster sample
struct FloorCell {
    float inv;
    __device__ __forceinline__ bool operator()(const float4& p, int32_t& ix, int32_t& iy) const
    {
        const float fx = floorf(p.x * inv), fy = floorf(p.y * inv);
        if (!(fx >= -2147483648.f && fx < 2147483648.f && fy >= -2147483648.f && fy < 2147483648.f)) return false;
        ix = (int32_t)fx, iy = (int32_t)fy;
        return true;
    }
};
static inline FloorCell cell_of(const RasterFrame& f) { return FloorCell{f.inv}; }

// the dense id dy * width + dx of p's cell in the frame's box (64-bit differences: a box may span all of int32), -1 outside
// the box or off int32
__device__ __forceinline__ int64_t frame_cell(const RasterFrame& f, const float4& p)
{
    int32_t ix, iy;
    if (!FloorCell{f.inv}(p, ix, iy)) return -1;
    const int64_t dx = (int64_t)ix - f.cx0, dy = (int64_t)iy - f.cy0;
    return (dx < 0 || dx >= f.width || dy < 0 || dy >= f.height) ? -1 : dy * f.width + dx;
}

// per workgroup: words 0..3 the index range (min ix, max ix, min iy, max iy, order-preserving), word 4 "out of int32"
template <class Cell>
__global__ __launch_bounds__(kCellThreads) void k_cell_range(const o3dr_point* __restrict__ in, int64_t n, Cell cell,
                                                             uint32_t* __restrict__ part)
{
    uint32_t v[4] = {0xffffffffu, 0u, 0xffffffffu, 0u};
    uint32_t bad = 0u;
    for (int64_t i = (int64_t)blockIdx.x * kCellThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kCellThreads) {
        int32_t ix, iy;
        if (!cell(reinterpret_cast<const float4*>(in)[i], ix, iy)) {
            bad = 1u;
            continue;
        }
        const uint32_t ux = (uint32_t)ix ^ 0x80000000u, uy = (uint32_t)iy ^ 0x80000000u;
        v[0] = u32_min(v[0], ux), v[1] = u32_max(v[1], ux);
        v[2] = u32_min(v[2], uy), v[3] = u32_max(v[3], uy);
    }
    const int op[4] = {0, 1, 0, 1};
    uint32_t* out = part + (int64_t)blockIdx.x * kPartWords;
    block_reduce4_u32(v, op, out);
    uint32_t b[4] = {bad, 0u, 0u, 0u};
    const int opb[4] = {1, 1, 1, 1};
    block_reduce4_u32(b, opb, out + 4);
}

// the dense cell id of every point: the sort key (the host has checked that it fits 32 bits; taken modulo 2^32, so a
// width of 2^32 - then the other is 1 - needs no special case)
template <class Cell>
__global__ __launch_bounds__(kCellThreads) void k_cell_keys(const o3dr_point* __restrict__ in, uint32_t n, Cell cell, int32_t x0, int32_t y0,
                                                            uint64_t wx, uint32_t* __restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * kCellThreads + threadIdx.x;
    if (i >= (int64_t)n) return;
    int32_t ix = x0, iy = y0;
    cell(reinterpret_cast<const float4*>(in)[i], ix, iy);  // (in range: k_cell_range found no index outside int32)
    const uint64_t dx = (uint64_t)((int64_t)ix - x0), dy = (uint64_t)((int64_t)iy - y0);
    keys[i] = (uint32_t)(dy * wx + dx);
}

// is sorted position i the first of its cell
__device__ __forceinline__ bool cell_head(const CellOrder& o, int64_t i) { return i == 0 || o.keys[i - 1] != o.keys[i]; }

// after the sort: 1 for the first point of every cell, 0 for the others
__global__ __launch_bounds__(kCellThreads) void k_cell_heads(CellOrder o, uint32_t* __restrict__ head)
{
    const int64_t i = (int64_t)blockIdx.x * kCellThreads + threadIdx.x;
    if (i >= (int64_t)o.n) return;
    head[i] = cell_head(o, i) ? 1u : 0u;
}
