// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// K2a — PCL VoxelGrid geometry and per-point linear index
//   [PCL 1.8 filters/impl/voxel_grid.hpp applyFilter; called from pose_functions.cpp:1689-1700]
// =================================================================================================
// cells of the grid (the linear index is below it)
__device__ __forceinline__ uint64_t geom_cells(const VoxelGeom& g)
{
    return (uint64_t)(uint32_t)g.div_b[0] * (uint64_t)(uint32_t)g.div_b[1] * (uint64_t)(uint32_t)g.div_b[2];
}
// sort plan: the linear index is < div_b.x*div_b.y*div_b.z, so only that many bits are sorted, in the fewest passes of
// at most kMaxRadixBits bits (a wrapped 32-bit index sorts all 32 bits); `cells` = number of values the sort key can take
__device__ __forceinline__ void sort_plan(VoxelGeom& g, uint64_t cells)
{
    uint32_t nbits = 32;
    if (cells <= (1ull << 32)) nbits = cells > 1 ? 64u - (uint32_t)__clzll((long long)(cells - 1)) : 1u;
    if (nbits < 1) nbits = 1;
    g.passes = (nbits + kMaxRadixBits - 1) / kMaxRadixBits;
    g.bpp = (nbits + g.passes - 1) / g.passes;  // <= kMaxRadixBits by construction
}

// PCL's grid geometry from the cloud's bounding box (getMinMax3D's result, taken BEFORE any z offset), leaf and size:
// inverse leaf, overflow guard, min_b / div_b / divb_mul, and the sort plan.  One statement of it for every kernel that
// needs it (k_voxel_geom per frame, the one-workgroup path of small clouds).
__device__ __forceinline__ VoxelGeom voxel_geom_of(const float mn_in[3], const float mx_in[3], const float leaf[3], float z_offset,
                                                   uint32_t n)
{
    VoxelGeom g;
    g.n = n;
    g.overflow = 0;
    g.passes = 0;
    g.bpp = 1;  // never above kMaxRadixBits: every consumer sizes LDS tables and histogram rows by kMaxRadix
    g.buf0 = 0;
    g.grouped = 0;
    float mn[3], mx[3];
    for (int a = 0; a < 3; ++a) {
        g.inv[a] = 1.0f / leaf[a];  // inverse_leaf_size_ = Array4f::Ones() / leaf_size_
        mn[a] = mn_in[a];
        mx[a] = mx_in[a];
    }
    // the bounding box was taken before `z += 500` (pose_functions.cpp:1666); fp32 add is monotonic
    mn[2] = mn[2] + z_offset;
    mx[2] = mx[2] + z_offset;
    if (g.n == 0) {
        for (int a = 0; a < 3; ++a) g.min_b[a] = 0, g.div_b[a] = 1;
        g.mul1 = g.mul2 = 1;
        return g;
    }
    // int64_t dx = static_cast<int64_t>((max_p[0]-min_p[0])*inverse_leaf_size_[0]) + 1; ...
    int64_t d[3];
    for (int a = 0; a < 3; ++a) d[a] = (int64_t)((mx[a] - mn[a]) * g.inv[a]) + 1;
    g.overflow = (d[0] * d[1] * d[2]) > (int64_t)INT32_MAX ? 1u : 0u;
    for (int a = 0; a < 3; ++a) {
        g.min_b[a] = (int32_t)floorf(mn[a] * g.inv[a]);
        const int32_t max_b = (int32_t)floorf(mx[a] * g.inv[a]);
        g.div_b[a] = max_b - g.min_b[a] + 1;
    }
    g.mul1 = (uint32_t)g.div_b[0];
    g.mul2 = (uint32_t)g.div_b[0] * (uint32_t)g.div_b[1];
    if (!g.overflow) sort_plan(g, geom_cells(g));
    return g;
}

// only_if_overflow: recompute just the frames whose geometry (from a conservative box) tripped PCL's overflow guard
__global__ __launch_bounds__(256) void k_voxel_geom(const float* __restrict__ mm, int64_t mm_stride, int mm_used,
                                                    const uint32_t* __restrict__ n_dev, float leaf0, float leaf1,
                                                    float leaf2, float z_offset, VoxelGeom* __restrict__ geom,
                                                    int only_if_overflow = 0)
{
    __shared__ float red[6 * 4];
    const int f = blockIdx.x;
    if (only_if_overflow && geom[f].overflow == 0u) return;
    // getMinMax3D: fold the per-workgroup boxes of this frame (min/max are order independent)
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    const float* row = mm + (int64_t)f * mm_stride * 6;
    for (int sidx = threadIdx.x; sidx < mm_used; sidx += 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], row[sidx * 6 + a]);
            hi[a] = fmaxf(hi[a], row[sidx * 6 + 3 + a]);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = wave_min_f32(lo[a]), h = wave_max_f32(hi[a]);
        if ((threadIdx.x & 63) == 0) {
            red[(threadIdx.x >> 6) * 6 + a] = l;
            red[(threadIdx.x >> 6) * 6 + 3 + a] = h;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const float leaf[3] = {leaf0, leaf1, leaf2};
    float mn[3], mx[3];
    for (int a = 0; a < 3; ++a) {
        mn[a] = fminf(fminf(red[a], red[6 + a]), fminf(red[12 + a], red[18 + a]));
        mx[a] = fmaxf(fmaxf(red[3 + a], red[9 + a]), fmaxf(red[15 + a], red[21 + a]));
    }
    geom[f] = voxel_geom_of(mn, mx, leaf, z_offset, n_dev[f]);
}

// The front of the fused batch path in one launch, one 1024-thread workgroup per frame: the exclusive scan of the frame's
// tile counts in place (k_scan_rows' job: cnt[f * L + i], totals[f] = the row's sum + add[f]) and then the frame's
// geometry from its boxes and that total (k_voxel_geom's job).  Both read what the count pass left and nothing of each
// other but the total.  For rows the one-workgroup scan takes (launch_scan: L <= 4 * kScanChunk).
__global__ __launch_bounds__(1024) void k_scan_counts_geom(uint32_t* __restrict__ cnt, int L, uint32_t* __restrict__ totals,
                                                           const uint32_t* __restrict__ add, const float* __restrict__ mm,
                                                           int64_t mm_stride, int mm_used, float leaf0, float leaf1, float leaf2,
                                                           VoxelGeom* __restrict__ geom)
{
    __shared__ uint32_t lds[1024 / 64 + 1];
    __shared__ float red[6 * 16];
    const int f = blockIdx.x;
    // the boxes first: their loads are in flight while the counts are scanned
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    const float* box = mm + (int64_t)f * mm_stride * 6;
    for (int sidx = threadIdx.x; sidx < mm_used; sidx += 1024) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], box[sidx * 6 + a]);
            hi[a] = fmaxf(hi[a], box[sidx * 6 + 3 + a]);
        }
    }
    uint32_t* row = cnt + (int64_t)f * L;
    const int chunk = (L + 1023) / 1024;
    const int b = (int)threadIdx.x * chunk;
    const int e = (b + chunk < L) ? b + chunk : L;
    uint32_t s = 0;
    for (int i = b; i < e; ++i) s += row[i];
    uint32_t total;
    uint32_t run = block_excl_scan_u32<16>(s, lds, total);
    for (int i = b; i < e; ++i) {
        const uint32_t v = row[i];
        row[i] = run;
        run += v;
    }
    total += add ? add[f] : 0u;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = wave_min_f32(lo[a]), h = wave_max_f32(hi[a]);
        if ((threadIdx.x & 63) == 0) {
            red[(threadIdx.x >> 6) * 6 + a] = l;
            red[(threadIdx.x >> 6) * 6 + 3 + a] = h;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    totals[f] = total;
    const float leaf[3] = {leaf0, leaf1, leaf2};
    float mn[3], mx[3];
    for (int a = 0; a < 3; ++a) {
        mn[a] = red[a];
        mx[a] = red[3 + a];
        for (int w = 1; w < 16; ++w) {
            mn[a] = fminf(mn[a], red[w * 6 + a]);
            mx[a] = fmaxf(mx[a], red[w * 6 + 3 + a]);
        }
    }
    geom[f] = voxel_geom_of(mn, mx, leaf, 0.f, total);
}

// Whole-cloud calls: the head flags of the GROUP RUNS (a point starts one iff its voxel group differs from its
// predecessor's; util.inc: group_coord_of) and their number per segment tile, in one read of the points.  One workgroup
// = one segment tile (kSegTile points, 4 sub-rows of 256 consecutive points).  Flags: see k_run_heads.
__global__ __launch_bounds__(256) void k_group_heads(const o3dr_point* __restrict__ in, const VoxelGeom* __restrict__ geom,
                                                     float z_offset, int n_tiles, uint32_t* __restrict__ seg_cnt,
                                                     uint8_t* __restrict__ head_bits)
{
    static_assert(kSegTile == 4 * 256, "one workgroup per segment tile");
    __shared__ uint32_t lds[4];
    const int tile = blockIdx.x;
    const VoxelGeom g = geom[0];
    if (g.overflow) return;
    const uint4* src = reinterpret_cast<const uint4*>(in);
    const int64_t base = (int64_t)tile * kSegTile;
    const int lane = threadIdx.x & 63;
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = base + k * 256 + threadIdx.x;
        GroupCoord gc = {0, 0, 0};
        uint32_t cell;
        if (i < g.n) gc = group_coord_of(src[i], g.inv, z_offset, cell);
        GroupCoord prev;
        prev.bx = __shfl_up(gc.bx, 1, 64);
        prev.iy = __shfl_up(gc.iy, 1, 64);
        prev.iz = __shfl_up(gc.iz, 1, 64);
        if (lane == 0 && i > 0 && i < g.n) prev = group_coord_of(src[i - 1], g.inv, z_offset, cell);  // previous wave's point
        const bool head = i < g.n && (i == 0 || group_differs(gc, prev));
        c += head ? 1u : 0u;
        // one byte per 4 consecutive points (this wave's 64 points = 16 bytes; bytes past the cloud's end get zeros)
        const unsigned long long hm = __ballot(head);
        if (lane < 16)
            head_bits[(int64_t)tile * 256 + k * 64 + (threadIdx.x >> 6) * 16 + lane] = (uint8_t)((hm >> (4 * lane)) & 15ull);
    }
    c = wave_sum_u32(c);
    if (lane == 0) lds[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) seg_cnt[tile] = lds[0] + lds[1] + lds[2] + lds[3];
}
// the same counts from flags that exist already (cloud_big records them while it grows: k_centroid / k_cloud_heads_fix)
__global__ __launch_bounds__(256) void k_head_counts(const uint8_t* __restrict__ head_bits, const VoxelGeom* __restrict__ geom,
                                                     int n_tiles, uint32_t* __restrict__ seg_cnt)
{
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const VoxelGeom g = geom[0];
    if (g.overflow || tile >= n_tiles) return;
    const int64_t base = (int64_t)tile * kSegTile;
    uint32_t c = 0;
    if (base < g.n) {
        uint32_t bits = reinterpret_cast<const uint32_t*>(head_bits + (int64_t)tile * 256)[lane];
        // flags of records past the end of the cloud are not defined here (the buffer outlives the cloud's size)
        const int64_t i0 = base + lane * 16;
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (i0 + q >= (int64_t)g.n) bits &= ~(1u << ((q >> 2) * 8 + (q & 3)));
        c = (uint32_t)__popc(bits & 0x0f0f0f0fu);
    }
    c = wave_sum_u32(c);
    if (lane == 0) seg_cnt[tile] = c;
}
