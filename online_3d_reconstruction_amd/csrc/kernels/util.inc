// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// small device helpers
// =================================================================================================
// Streaming loads (data read once per kernel, far larger than the caches).  Measured, same box: k_radix_hist 0.59 ->
// 0.455 ms per 200-frame step with the non-temporal hint, while the scatter that reads the same indices next loses
// 0.10 ms (it no longer finds part of them in the Infinity Cache): net -0.03..-0.07 ms.  The hint on the scatter's own
// loads costs +12 %, on its stores +30 %, on k_reproject_emit's stores +1.5 %; on k_run_heads / k_centroid_groups nothing.
// XCD-contiguous work order.  The workgroups of a grid go round-robin over the 8 XCDs in dispatch order (x fastest), and
// every XCD has its own L2: two workgroups that write (or read) the two halves of one 128-byte line meet in L2 only when
// they run on the same XCD.  With gridDim.x a multiple of 8, workgroup bx runs on XCD bx & 7; this hands XCD x the
// contiguous block [x * chunk, (x + 1) * chunk) of the n_active work items of the row (-1: nothing to do).
__device__ __forceinline__ int xcd_chunk_item(int bx, int n_active)
{
    const int chunk = (n_active + kXcds - 1) / kXcds, q = bx / kXcds;
    const int item = (bx % kXcds) * chunk + q;
    return (q < chunk && item < n_active) ? item : -1;
}
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_a4_t __attribute__((ext_vector_type(4), aligned(4)));  // 16-byte load from a 4-byte boundary
__device__ __forceinline__ uint4 stream_load_u4(const uint4* p)
{
    const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
// inclusive wave scan on the DPP path (row shifts inside the 16-lane rows, then the row totals): no LDS round trips
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return v;
}
// the value of the lane below (lane 0 keeps its own): one DPP move, no LDS round trip
__device__ __forceinline__ int32_t wave_shr1_i32(int32_t v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)  // the maximum over the wave, in every lane
{
    auto mx = [](uint32_t a, int b) { return a > (uint32_t)b ? a : (uint32_t)b; };
    v = mx(v, __builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));
    v = mx(v, __builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));
    v = mx(v, __builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));
    v = mx(v, __builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));
    v = mx(v, __builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
    v = mx(v, __builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)  // the minimum over the wave, in every lane
{
    auto mn = [](uint32_t a, int b) { return a < (uint32_t)b ? a : (uint32_t)b; };
    v = mn(v, __builtin_amdgcn_update_dpp(-1, (int)v, 0x111, 0xf, 0xf, false));
    v = mn(v, __builtin_amdgcn_update_dpp(-1, (int)v, 0x112, 0xf, 0xf, false));
    v = mn(v, __builtin_amdgcn_update_dpp(-1, (int)v, 0x114, 0xf, 0xf, false));
    v = mn(v, __builtin_amdgcn_update_dpp(-1, (int)v, 0x118, 0xf, 0xf, false));
    v = mn(v, __builtin_amdgcn_update_dpp(-1, (int)v, 0x142, 0xa, 0xf, false));
    v = mn(v, __builtin_amdgcn_update_dpp(-1, (int)v, 0x143, 0xc, 0xf, false));
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// wave reductions on the DPP path (no LDS round trips); the result is wave-uniform
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_u32(v), 63);
}
// the fp64 sum over the wave as a fixed butterfly (lane ^ 32, 16, .. 1), the same value in every lane: the order is part
// of the contract of every fp64 sum built on it (kernels/rigid_core.inc)
__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// fp32 min / max over the wave, in every lane.  Reduced as order-preserving integers: fminf / fmaxf cost a
// canonicalising v_max_f32 per operand in front of every step (IEEE NaN rules), v_min_u32 / v_max_u32 take the DPP
// operand directly - a third of the instructions.  (No NaNs reach these; -0 orders below +0, which no consumer
// can tell apart: the boxes only go through floor(x * inv) and differences.)
__device__ __forceinline__ uint32_t f32_ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float ordered_f32(uint32_t u) { return __uint_as_float(u ^ (((u >> 31) - 1u) | 0x80000000u)); }
#define O3DR_WAVE_REDUCE_ORD(name, op, ident)                                                                                  \
    __device__ __forceinline__ float name(float f)                                                                       \
    {                                                                                                                    \
        /* lanes without a source get the operation's identity: the compiler folds move and op into one DPP instruction */ \
        uint32_t v = f32_ordered(f);                                                                                     \
        v = op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)(ident), (int)v, 0x111, 0xf, 0xf, false));                  \
        v = op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)(ident), (int)v, 0x112, 0xf, 0xf, false));                  \
        v = op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)(ident), (int)v, 0x114, 0xf, 0xf, false));                  \
        v = op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)(ident), (int)v, 0x118, 0xf, 0xf, false));                  \
        v = op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)(ident), (int)v, 0x142, 0xa, 0xf, false));                  \
        v = op(v, (uint32_t)__builtin_amdgcn_update_dpp((int)(ident), (int)v, 0x143, 0xc, 0xf, false));                  \
        return ordered_f32((uint32_t)__builtin_amdgcn_readlane((int)v, 63));                                             \
    }
__device__ __forceinline__ uint32_t u32_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t u32_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
O3DR_WAVE_REDUCE_ORD(wave_min_f32, u32_min, 0xffffffffu)
O3DR_WAVE_REDUCE_ORD(wave_max_f32, u32_max, 0u)
#undef O3DR_WAVE_REDUCE_ORD
// exclusive scan of one value per thread over a workgroup of NW waves; returns the exclusive
// prefix, `total` = sum over the workgroup.  `lds` holds NW+1 words.
template <int NW>
__device__ __forceinline__ uint32_t block_excl_scan_u32(uint32_t v, uint32_t* lds, uint32_t& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan_u32(v);
    if (lane == 63) lds[w] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const uint32_t t = lds[i];
            lds[i] = run;
            run += t;
        }
        lds[NW] = run;
    }
    __syncthreads();
    const uint32_t r = lds[w] + incl - v;
    total = lds[NW];
    __syncthreads();
    return r;
}
// the same for N values per thread at once (one pair of barriers for all of them); `lds` holds (NW+1)*N words
template <int NW, int N>
__device__ __forceinline__ void block_excl_scan_multi_u32(uint32_t (&v)[N], uint32_t* lds, uint32_t (&total)[N])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t incl[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        incl[j] = wave_incl_scan_u32(v[j]);
        if (lane == 63) lds[w * N + j] = incl[j];
    }
    __syncthreads();
    if ((int)threadIdx.x < N) {
        uint32_t run = 0;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const uint32_t t = lds[i * N + threadIdx.x];
            lds[i * N + threadIdx.x] = run;
            run += t;
        }
        lds[NW * N + threadIdx.x] = run;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) {
        v[j] = lds[w * N + j] + incl[j] - v[j];
        total[j] = lds[NW * N + j];
    }
    __syncthreads();
}
// digit values of one radix pass; clamped so that no VoxelGeom, however it was filled, can make a kernel step
// outside its kMaxRadix-sized LDS tables and histogram rows
__device__ __forceinline__ int geom_bins(const VoxelGeom& g)
{
    const uint32_t bpp = g.bpp < (uint32_t)kMaxRadixBits ? g.bpp : (uint32_t)kMaxRadixBits;
    return 1 << bpp;
}
// PCL's linear voxel index: idx = ijk0*divb_mul[0] + ijk1*divb_mul[1] + ijk2*divb_mul[2] with
// ijk = int(floor(p*inverse_leaf) - float(min_b));  floor and subtraction are exact here, so the difference is taken
// in integers [PCL 1.8 filters/impl/voxel_grid.hpp applyFilter, first pass]
__device__ __forceinline__ uint32_t voxel_key_of(const uint4 v, const VoxelGeom& g, float z_offset)
{
    const float x = __uint_as_float(v.x), y = __uint_as_float(v.y), z = __uint_as_float(v.z) + z_offset;
    const int32_t i0 = (int32_t)floorf(x * g.inv[0]) - g.min_b[0];
    const int32_t i1 = (int32_t)floorf(y * g.inv[1]) - g.min_b[1];
    const int32_t i2 = (int32_t)floorf(z * g.inv[2]) - g.min_b[2];
    return (uint32_t)i0 + (uint32_t)i1 * g.mul1 + (uint32_t)i2 * g.mul2;
}
// Voxel GROUPS of the whole-cloud grids (see k_centroid_groups): kGroupCells consecutive voxels along x, aligned to the
// ABSOLUTE voxel coordinate (floor(x * inverse_leaf) >> kGroupBits), so that "do two points share a group" does not
// depend on the grid's bounding box: cloud_big's group-run heads can be recorded while it is being appended to.
// A group's coordinates: (block along x, row, layer), all absolute.
struct GroupCoord {
    int32_t bx, iy, iz;
};
__device__ __forceinline__ GroupCoord group_coord_of(const uint4 v, const float inv[3], float z_offset, uint32_t& cell)
{
    const float x = __uint_as_float(v.x), y = __uint_as_float(v.y), z = __uint_as_float(v.z) + z_offset;
    const int32_t i0 = (int32_t)floorf(x * inv[0]);
    cell = (uint32_t)(i0 & (kGroupCells - 1));
    GroupCoord c;
    c.bx = i0 >> kGroupBits;
    c.iy = (int32_t)floorf(y * inv[1]);
    c.iz = (int32_t)floorf(z * inv[2]);
    return c;
}
__device__ __forceinline__ bool group_differs(const GroupCoord& a, const GroupCoord& b)
{
    return a.bx != b.bx || a.iy != b.iy || a.iz != b.iz;
}
// blocks along x the grid spans, and the sort key of a group: ascending key = ascending PCL index
// (idx = i0 + i1*div_x + i2*div_x*div_y orders by layer, row, x; inside a group the voxels ascend with x)
__device__ __forceinline__ uint32_t group_blocks_x(const VoxelGeom& g)
{
    return (uint32_t)(((g.min_b[0] + g.div_b[0] - 1) >> kGroupBits) - (g.min_b[0] >> kGroupBits) + 1);
}
__device__ __forceinline__ uint32_t group_key_of(const GroupCoord& c, const VoxelGeom& g)
{
    const uint32_t i1 = (uint32_t)(c.iy - g.min_b[1]), i2 = (uint32_t)(c.iz - g.min_b[2]);
    return (uint32_t)(c.bx - (g.min_b[0] >> kGroupBits)) + group_blocks_x(g) * (i1 + (uint32_t)g.div_b[1] * i2);
}
// where the head flag of record i lives: one byte per 4 records, flags in the low nibble (bit q of byte b = record 4 b + q)
__device__ __forceinline__ void head_flag_place(uint64_t i, uint64_t& word, uint32_t& bit)
{
    word = i >> 4;
    bit = (uint32_t)(((i >> 2) & 3u) * 8u + (i & 3u));
}
// the buffer (of the ping-pong pair) a frame's records end up in after its sort passes
__device__ __forceinline__ const uint32_t* sorted_buf(const VoxelGeom& g, const uint32_t* b0, const uint32_t* b1)
{
    return ((g.passes + g.buf0) & 1u) ? b1 : b0;
}
// workgroup min/max of per-thread (lo[3], hi[3]) -> one 6-float slot (min xyz, max xyz); a workgroup
// without points stores (+inf, -inf).  Slots are reduced by k_voxel_geom: no same-address atomics.
template <int NW>
__device__ __forceinline__ void block_minmax_store(const float lo[3], const float hi[3], bool any,
                                                   float* lds /*6*NW*/, float* __restrict__ slot6)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float l = wave_min_f32(any ? lo[a] : __builtin_inff());
        const float h = wave_max_f32(any ? hi[a] : -__builtin_inff());
        if (lane == 0) {
            lds[w * 6 + a] = l;
            lds[w * 6 + 3 + a] = h;
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        float v = lds[a];
#pragma unroll
        for (int i = 1; i < NW; ++i) v = (a < 3) ? fminf(v, lds[i * 6 + a]) : fmaxf(v, lds[i * 6 + a]);
        slot6[a] = v;
    }
    __syncthreads();
}

// Whole-cloud integer reductions go through per-workgroup partials (kPartWords words each) and a one-workgroup fold: one
// atomic per wave on the same few words serialises in L2 and cost ~0.3 ms per kernel at 453k points.
constexpr int kFoldThreads = 256;
constexpr int kFoldWaves = kFoldThreads / kWave;
// the four values of every thread reduced over the workgroup (op: 0 min, 1 max, 2 sum per word), written by thread 0
__device__ __forceinline__ void block_reduce4_u32(uint32_t v[4], const int op[4], uint32_t* __restrict__ out)
{
    __shared__ uint32_t lds[kFoldWaves][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = op[k] == 0 ? wave_min_u32(v[k]) : op[k] == 1 ? wave_max_u32(v[k]) : wave_sum_u32(v[k]);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 4; ++k) lds[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kFoldWaves; ++w)
            for (int k = 0; k < 4; ++k) {
                const uint32_t u = lds[w][k];
                v[k] = op[k] == 0 ? u32_min(v[k], u) : op[k] == 1 ? u32_max(v[k], u) : v[k] + u;
            }
        for (int k = 0; k < 4; ++k) out[k] = v[k];
    }
    __syncthreads();  // (lds is reused by the next call)
}
// one workgroup: the partials of `blocks` workgroups folded (word-wise op) into out[0..3]
__global__ __launch_bounds__(kFoldThreads) void k_fold4_u32(const uint32_t* __restrict__ part, int blocks, int word0, int op0, int op1,
                                                            int op2, int op3, uint32_t* __restrict__ out)
{
    const int op[4] = {op0, op1, op2, op3};
    uint32_t v[4];
    for (int k = 0; k < 4; ++k) v[k] = op[k] == 0 ? 0xffffffffu : 0u;
    for (int b = threadIdx.x; b < blocks; b += kFoldThreads)
        for (int k = 0; k < 4; ++k) {
            const uint32_t u = part[(int64_t)b * kPartWords + word0 + k];
            v[k] = op[k] == 0 ? u32_min(v[k], u) : op[k] == 1 ? u32_max(v[k], u) : v[k] + u;
        }
    block_reduce4_u32(v, op, out);
}

// 1 in flag[0] if any coordinate of the n points is not finite (every writer stores the same value)
__global__ __launch_bounds__(256) void k_cloud_finite(const o3dr_point* __restrict__ in, int64_t n, uint32_t* __restrict__ flag)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float4 p = reinterpret_cast<const float4*>(in)[i];
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) flag[0] = 1u;
    }
}

// Lower bound of the fp32 d2 from (qx, qy, qz) to every point of a cell with the exact bounding box lo .. hi, in the
// arithmetic of the distance itself (monotone roundings): never above a computed distance.  An empty cell's box
// (+inf .. -inf) gives +inf.
__device__ __forceinline__ float cell_box_d2_lower_bound(const float4& lo, const float4& hi, float qx, float qy, float qz)
{
    const float gx = fmaxf(fmaxf(lo.x - qx, qx - hi.x), 0.f);
    const float gy = fmaxf(fmaxf(lo.y - qy, qy - hi.y), 0.f);
    const float gz = fmaxf(fmaxf(lo.z - qz, qz - hi.z), 0.f);
    return (gx * gx + gy * gy) + gz * gz;
}

// shared by MLS (kernels/mls.inc) and the plane refinement (kernels/plane.inc)
constexpr int kMlsJacobiSweeps = 8;  // cyclic (0,1) (0,2) (1,2): converged to fp64 rounding well before
// symmetric 3x3 eigen-decomposition by cyclic Jacobi: A (upper triangle used) -> eigenvalues on the diagonal, V's columns
__device__ __forceinline__ void mls_jacobi3(double A[3][3], double V[3][3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    A[1][0] = A[0][1], A[2][0] = A[0][2], A[2][1] = A[1][2];
#pragma unroll
    for (int sweep = 0; sweep < kMlsJacobiSweeps; ++sweep) {
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2, r = 3 - p - q;
            const double apq = A[p][q];
            if (apq == 0.0) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
            A[p][p] -= t * apq;
            A[q][q] += t * apq;
            A[p][q] = A[q][p] = 0.0;
            const double arp = A[r][p], arq = A[r][q];
            A[r][p] = A[p][r] = cs * arp - sn * arq;
            A[r][q] = A[q][r] = sn * arp + cs * arq;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double vp = V[i][p], vq = V[i][q];
                V[i][p] = cs * vp - sn * vq;
                V[i][q] = sn * vp + cs * vq;
            }
        }
    }
}

// the search grid's cell of a point: its column and row (clamped: the outermost ones are open-ended), and the cell id
__device__ __forceinline__ int sor_col(const SorGeom& g, float x)
{
    const int cx = (int)((x - g.mnx) * g.inv_h);
    return cx < 0 ? 0 : (cx >= g.gx ? g.gx - 1 : cx);
}
__device__ __forceinline__ int sor_row(const SorGeom& g, float y)
{
    const int cy = (int)((y - g.mny) * g.inv_h);
    return cy < 0 ? 0 : (cy >= g.gy ? g.gy - 1 : cy);
}
__device__ __forceinline__ int sor_cell(const SorGeom& g, float x, float y, int& cx, int& cy)
{
    cx = sor_col(g, x), cy = sor_row(g, y);
    return cy * g.gx + cx;
}

// The exact radius walk over a search grid (launch_nn_grid), shared by MLS (kernels/mls.inc) and the clustering
// (kernels/cluster.inc): f(p, d2) for every point p of the cloud with the fp32 d2 <= r2, in the fixed order of the MLS
// contract.  g is *grid.geom, loaded by the caller.  The window is every cell between the cells of the query's box
// (q -/+ pad_r = grid_pad_radius(r), clamped to the cloud's box) in x and y: the cell assignment is monotone in the
// coordinate, so no neighbour lies outside it.  A cell whose exact box is farther than r2 is skipped.
template <class F>
__device__ __forceinline__ void grid_radius_walk(const SearchGrid& grid, const SorGeom& g, const float4& q, float pad_r, float r2, F&& f)
{
    const float x0f = fmaxf(q.x - pad_r, grid.box6[0]), x1f = fminf(q.x + pad_r, grid.box6[3]);
    const float y0f = fmaxf(q.y - pad_r, grid.box6[1]), y1f = fminf(q.y + pad_r, grid.box6[4]);
    const int x0 = sor_col(g, x0f), x1 = sor_col(g, x1f), y0 = sor_row(g, y0f), y1 = sor_row(g, y1f);
    for (int yy = y0; yy <= y1; ++yy) {
        const int64_t row = (int64_t)yy * g.gx;
        for (int xx = x0; xx <= x1; ++xx) {
            const int64_t c = row + xx;
            const float4 lo = grid.cell_lo[c], hi = grid.cell_hi[c];
            if (!(cell_box_d2_lower_bound(lo, hi, q.x, q.y, q.z) <= r2)) continue;
            const uint32_t s = grid.cell_first[c], e = grid.cell_first[c + 1];
            for (uint32_t j = s; j < e; ++j) {
                const float4 p = grid.xyz[j];
                const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
                const float d = (dx * dx + dy * dy) + dz * dz;
                if (d <= r2) f(p, d);
            }
        }
    }
}

// ---- union-find, shared by the disparity filter (kernels/disparity_filter.inc) and the clustering (kernels/cluster.inc).
// `Mem` reads and lowers parent words: in LDS (workgroup scope) or in global memory (agent scope).
struct DfLds {
    static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    static __device__ __forceinline__ int lower(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
struct DfGlobal {
    static __device__ __forceinline__ int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ int lower(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
template <class Mem>
__device__ __forceinline__ int df_find(const int* parent, int x)
{
    // Ends: parent[i] <= i for every i at every moment (words start at i and are only ever lowered), so each step goes
    // to a strictly smaller index, and indices are >= 0.  A stale value is a former ancestor: still of the same tree.
    for (int p = Mem::load(parent + x); p < x; p = Mem::load(parent + x)) x = p;
    return x;
}
// df_find that halves the path it walks: every other node on it is lowered to its grandparent.  The grandparent is an
// ancestor, so the word is only lowered and the node stays in its tree; a min that meets a word another thread lowered
// meanwhile keeps the smaller of two ancestors.  Ends as df_find does: x strictly decreases.  (The clustering's trees are
// linked by point index in whatever order the lanes meet: without this their depth is not bounded by a tile.)
template <class Mem>
__device__ __forceinline__ int df_find_halve(int* parent, int x)
{
    for (;;) {
        const int p = Mem::load(parent + x);
        if (p >= x) return x;
        const int g = Mem::load(parent + p);
        if (g >= p) return p;
        Mem::lower(parent + x, g);
        x = g;
    }
}
template <class Mem>
__device__ __forceinline__ void df_union(int* parent, int a, int b)
{
    // Ends: a retry happens only when the atomic min returned old < a, and the next round starts from old: the larger
    // index of the pair strictly decreases from round to round (find only lowers it further), and indices are >= 0.
    // Nothing waits for another thread.  The link a -> old that the min may have replaced is carried on by this
    // thread, which goes on to join old and b.
    for (;;) {
        a = df_find<Mem>(parent, a);
        b = df_find<Mem>(parent, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = Mem::lower(parent + a, b);  // the larger root goes under the smaller
        if (old == a) return;                       // a was a root: linked
        a = old;                                    // old < a: a had been linked meanwhile
    }
}
