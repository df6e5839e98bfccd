// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// A3b — pcl::StatisticalOutlierRemoval<PointXYZRGB> (pose_functions.cpp:1673-1686: mean_k 50, 1 sigma)
//   [PCL 1.8 filters/impl/statistical_outlier_removal.hpp on KdTreeFLANN / flann::L2_Simple<float>]
//   d2 = ((0 + dx*dx) + dy*dy) + dz*dz in fp32; the 51 smallest d2 per point (the point itself
//   included), mean of sqrt over the 50 non-first ones in fp64 (ascending order), global mean/stddev in fp64, keep
//   iff !(dist > mean + 1*stddev).  Exact k-NN: a uniform XY grid (cells sorted with the radix sort above), ring
//   expansion, conservative stop (no unvisited column can hold a point closer than 0.999*r*h).
//   Every kernel takes grid y = frame: a batch of clouds goes through one set of launches.
// =================================================================================================
// the search grid of one cloud (~cell_points points per column of cells, at most max_cells cells) and the sort plan of its
// cell ids; one statement of it for k_sor_plan and for the one-workgroup path of small clouds (kernels/small.inc).
// The grid is active for clouds of more than active_above points (SOR: kSorMeanK; the nearest-neighbour search: 0).
__device__ __forceinline__ void sor_plan_of(const float mn[2], const float mx[2], uint32_t n, uint32_t max_cells, SorGeom& g_out,
                                            VoxelGeom& v_out, double cell_points = kSorCellPoints,
                                            uint32_t active_above = (uint32_t)kSorMeanK)
{
    SorGeom g;
    g.n = n;
    g.active = g.n > active_above ? 1u : 0u;  // SOR: fewer points - the reference reads past its list; pass through
    g.mnx = mn[0];
    g.mny = mn[1];
    const float mxx = mx[0];
    const float mxy = mx[1];
    double ex = (double)mxx - (double)g.mnx, ey = (double)mxy - (double)g.mny;
    if (!(ex > 1e-9)) ex = 1e-9;
    if (!(ey > 1e-9)) ey = 1e-9;
    double h = sqrt(cell_points * ex * ey / (double)(g.n ? g.n : 1u));  // ~cell_points points per column
    if (h < 1e-6) h = 1e-6;
    int64_t gx = (int64_t)(ex / h) + 1, gy = (int64_t)(ey / h) + 1;
    while (gx * gy > (int64_t)max_cells) {
        h *= 1.25;
        gx = (int64_t)(ex / h) + 1;
        gy = (int64_t)(ey / h) + 1;
    }
    g.h = (float)h;
    g.inv_h = (float)(1.0 / h);
    g.gx = (int)gx;
    g.gy = (int)gy;
    g.threshold = 0.0;
    g_out = g;
    // sort plan for the cell ids
    VoxelGeom v;
    for (int a = 0; a < 3; ++a) v.inv[a] = 1.f, v.min_b[a] = 0, v.div_b[a] = 1;
    v.mul1 = v.mul2 = 1;
    v.n = g.n;
    v.buf0 = 0;
    v.grouped = 0;
    v.overflow = g.active ? 0u : 1u;  // inactive: every sort kernel returns at once
    const uint64_t cells = (uint64_t)gx * (uint64_t)gy;
    uint32_t nbits = cells > 1 ? 64u - (uint32_t)__clzll((long long)(cells - 1)) : 1u;
    v.passes = (nbits + kMaxRadixBits - 1) / kMaxRadixBits;
    v.bpp = (nbits + v.passes - 1) / v.passes;
    v_out = v;
}

__global__ __launch_bounds__(256) void k_sor_plan(const float* __restrict__ mm_all, int64_t mm_stride, int mm_used,
                                                  const uint32_t* __restrict__ n_dev, uint32_t max_cells,
                                                  SorGeom* __restrict__ sg, VoxelGeom* __restrict__ geom, double cell_points,
                                                  uint32_t active_above)
{
    __shared__ float red[6 * 4];
    const int f = blockIdx.x;
    const float* mm = mm_all + (int64_t)f * mm_stride * 6;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (int sidx = threadIdx.x; sidx < mm_used; sidx += 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], mm[sidx * 6 + a]);
            hi[a] = fmaxf(hi[a], mm[sidx * 6 + 3 + a]);
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
    const float mn2[2] = {fminf(fminf(red[0], red[6]), fminf(red[12], red[18])), fminf(fminf(red[1], red[7]), fminf(red[13], red[19]))};
    const float mx2[2] = {fmaxf(fmaxf(red[3], red[9]), fmaxf(red[15], red[21])), fmaxf(fmaxf(red[4], red[10]), fmaxf(red[16], red[22]))};
    sor_plan_of(mn2, mx2, n_dev[f], max_cells, sg[f], geom[f], cell_points, active_above);
}

// cell id per point (the sort key; sor_cell and its column / row are in util.inc, next to the radius walk that shares them)
__global__ __launch_bounds__(256) void k_sor_cells(const o3dr_point* __restrict__ in, int64_t in_fstride, const SorGeom* __restrict__ sg,
                                                   int64_t cap, uint32_t* __restrict__ keys)
{
    const int f = blockIdx.y;
    const SorGeom g = sg[f];
    if (!g.active) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    const uint4 v = reinterpret_cast<const uint4*>(in + (int64_t)f * in_fstride)[i];
    int cx, cy;
    keys[(int64_t)f * cap + i] = (uint32_t)sor_cell(g, __uint_as_float(v.x), __uint_as_float(v.y), cx, cy);
}

// the cells' populations from the SORTED cell ids (-> cell_first by an exclusive scan): the first record of a cell's run
// subtracts its position, the last adds the position behind it - two atomics per occupied cell instead of one per point
// on counters that ~30 points share (k_sor_cells with the counting atomics took 30 us per dense 720p frame, 5 % of the path)
__global__ __launch_bounds__(256) void k_sor_cell_counts(const uint32_t* __restrict__ keys0, const uint32_t* __restrict__ keys1,
                                                         const VoxelGeom* __restrict__ geom, const SorGeom* __restrict__ sg, int64_t cap,
                                                         int64_t cell_stride, uint32_t* __restrict__ cell_cnt)
{
    const int f = blockIdx.y;
    const SorGeom g = sg[f];
    if (!g.active) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    const uint32_t* k = sorted_buf(geom[f], keys0, keys1) + (int64_t)f * cap;
    const uint32_t key = k[i];
    const uint32_t cells = (uint32_t)g.gx * (uint32_t)g.gy;
    if (key >= cells) return;  // (never expected: sor_cell clamps)
    uint32_t* cnt = cell_cnt + (int64_t)f * cell_stride;
    if (i == 0 || k[i - 1] != key) atomicSub(&cnt[key], (uint32_t)i);
    if (i + 1 == (int64_t)g.n || k[i + 1] != key) atomicAdd(&cnt[key], (uint32_t)i + 1u);
}

// after the sort: coordinates in cell order (coalesced candidate reads); w = the point's original index (its bit pattern:
// the nearest-neighbour search reports it, SOR does not read it)
__global__ __launch_bounds__(256) void k_sor_gather(const o3dr_point* __restrict__ in, int64_t in_fstride, const uint32_t* __restrict__ ids0,
                                                    const uint32_t* __restrict__ ids1, const SorGeom* __restrict__ sg,
                                                    const VoxelGeom* __restrict__ geom, int64_t cap, float4* __restrict__ sxyz)
{
    const int f = blockIdx.y;
    const SorGeom g = sg[f];
    if (!g.active) return;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= g.n) return;
    const uint32_t* id = sorted_buf(geom[f], ids0, ids1) + (int64_t)f * cap;
    const uint32_t src = id[j];
    const uint4 v = reinterpret_cast<const uint4*>(in + (int64_t)f * in_fstride)[src < g.n ? src : 0u];
    sxyz[(int64_t)f * cap + j] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(src));
}

// ---- exact 51-NN, one query per lane, ONE candidate stream per wave -------------------------------------------------
// A wave takes 64 consecutive queries of the cell-sorted array (a few neighbouring cells of one grid row).  All its lanes
// walk the same candidates - the rows [row - r, row + r] x columns [first cell - r, last cell + r] of ring r, each row
// piece one contiguous range of the sorted array - so a candidate is one coalesced load per 64 and three lane
// broadcasts, and the wave never diverges over "who visits which cell".  A lane keeps the squared distances below its
// current bound in two places: its 64 smallest so far, SORTED, in registers (KEPT) and up to 64 entries APPENDED since in
// a private LDS column (one store per candidate, at a write position that only advances for candidates below the bound).
// When a column fills up the wave MERGES together: every lane sorts its appended entries with a bitonic network in
// registers, takes the element-wise minimum of the kept entries and the reversed appended ones (the 64 smallest of both, a
// bitonic sequence) and merges that: 543 + 32 + 192 compare-exchanges of two instructions each, no memory, no data-dependent trip
// count, and the bound becomes the lane's exact 51st smallest distance so far - the tightest bound there is, so the fewest
// candidates are appended afterwards.  (Round 3's first version bisected for a threshold with 51..64 entries below it over
// 128 unsorted entries and compacted through LDS: every pass cost 256 instructions, a wave needed as many passes as its
// slowest lane - up to ~20 where a lattice of points puts neighbours on shells of equal distance - and most of the
// kernel's 29 k vector instructions per wave were prunes.  Before that: a 51-entry max-heap per lane in LDS, 3.4 ms per frame.)
// At the end the kept entries ARE the ascending order the reference's fp64 mean is summed in.
constexpr int kSorKeep = 64;                // registers: the smallest entries so far, ascending (bit patterns; NaN padding last)
constexpr int kSorAdd = 64;                 // LDS column: entries appended since the last merge
// A lane's row is a COLUMN of the wave's LDS block: slot i of lane l is word 64 i + l, so the 64 lanes of any LDS
// instruction - whatever their write positions - fall on 64 different words of consecutive banks: every append and every
// row read is conflict-free.  (Rows of 68 consecutive words per lane put lanes l and l + 8 of a 32-lane half on one bank:
// every append, the hot instruction of the kernel, cost 4 LDS cycles per half instead of 1: 1 079 -> 1 162 frames/s.)
constexpr int kSorAddStride = kSorAdd + 1;  // slots per lane (the write position may reach kSorAdd)
#define SOR_AT(row, i) (row)[(i) * kWave]
constexpr int kSorMergeAt = kSorAdd - 16;   // columns are checked every 16 candidates
constexpr int kSorK = kSorMeanK + 1;        // neighbours wanted: the point itself + mean_k
#ifndef O3DR_SOR_RING_CAP
#define O3DR_SOR_RING_CAP 2
#endif
constexpr int kSorRingCap = O3DR_SOR_RING_CAP;  // rings a wave walks whatever happens; beyond them it goes on only while ...
#ifndef O3DR_SOR_MIN_LIVE
#define O3DR_SOR_MIN_LIVE 12
#endif
constexpr int kSorMinLive = O3DR_SOR_MIN_LIVE;  // ... at least this many lanes still search; else they go to k_sor_knn_left
static_assert(kSorKeep >= kSorK && kSorAdd == kSorKeep, "the merge pairs kept[i] with the appended entry 63 - i");

struct SorLane {
    float worst;    // the 51st smallest entry so far; candidates must be below it; +inf until there are 51
    uint32_t cnt;   // entries in the LDS column
    uint32_t nk;    // real entries kept in registers
};

// c += (a < b) as compare-into-VCC + add-with-carry: two instructions and no wait states (the compiler's own choice -
// compare into a scalar pair, select, add - needs s_nops between the compare and the select)
__device__ __forceinline__ void sor_inc_if_lt(uint32_t& c, float a, float b)
{
    asm("v_cmp_lt_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc" : "+v"(c) : "v"(a), "v"(b) : "vcc");
}

// fills a lane's LDS column with NaN: appended entries then sit in front of NaN padding (except the one slot at the write
// position, which holds the last candidate that was not taken), and a merge can load the column without index masks
__device__ __forceinline__ void sor_row_clear(float* __restrict__ row)
{
    const float kNaN = __uint_as_float(0x7fc00000u);
#pragma unroll
    for (int i = 0; i < kSorAddStride; ++i) SOR_AT(row, i) = kNaN;
}

// compare-exchange of two bit patterns: a <= b afterwards (v_min_u32 + v_max_u32).  Squared distances are non-negative,
// so they order like their bit patterns; the NaN padding (0x7fc00000) lies above +inf and sorts last.
#define SOR_CE(a, b)                             \
    {                                            \
        const uint32_t lo_ = (a) < (b) ? (a) : (b); \
        const uint32_t hi_ = (a) < (b) ? (b) : (a); \
        (a) = lo_;                               \
        (b) = hi_;                               \
    }

// Wave-uniform merge (see above); straight-line code over registers.  Afterwards every lane's LDS column is empty (all NaN),
// `kept` holds the 64 smallest entries the lane has seen, ascending and NaN-padded, and the bound is the 51st of them.
// N = the column slots that can hold entries (no lane has appended more than N): the merges in front of a stop test
// mostly find 32 or fewer (80 % of them on the headline frames) and take the half-size network - 191 + 192 compare-
// exchanges instead of 543 + 192.
template <int N>
__device__ __forceinline__ void sor_merge(float* __restrict__ row, SorLane& L, uint32_t (&kept)[kSorKeep])
{
    static_assert(N == kSorAdd || N == kSorAdd / 2, "whole or half column");
    const float kNaN = __uint_as_float(0x7fc00000u);
    SOR_AT(row, L.cnt) = kNaN;  // the slot at the write position (<= N)
    uint32_t add[N];
#pragma unroll
    for (int i = 0; i < N; ++i) add[i] = __float_as_uint(SOR_AT(row, i));
#pragma unroll
    for (int i = 0; i <= N; ++i) SOR_AT(row, i) = kNaN;  // (the slots above N hold NaN already)
    // the appended entries, ascending: Batcher's odd-even merge sort (543 compare-exchanges for 64 entries; a bitonic
    // sorting network takes 672); every index is a compile-time constant once the loops are unrolled
#pragma unroll
    for (int p = 1; p < N; p <<= 1) {
#pragma unroll
        for (int k = p; k >= 1; k >>= 1) {
#pragma unroll
            for (int j = k % p; j <= N - 1 - k; j += 2 * k) {
#pragma unroll
                for (int i = 0; i < k; ++i) {
                    if (i + j + k < N && (i + j) / (2 * p) == (i + j + k) / (2 * p)) SOR_CE(add[i + j], add[i + j + k]);
                }
            }
        }
    }
    // the 64 smallest of both sets (ascending against descending - the appended entries padded with "infinity" to 64 - : the
    // minima form a bitonic sequence) ...
    // (a kept entry ranked 52nd or worse can never be among the 51 smallest again: those slots take the appended entry as it
    // is, and the comparators of the previous merge that only fed them are dead code)
#pragma unroll
    for (int i = 0; i < kSorKeep; ++i) {
        const int j = kSorKeep - 1 - i;
        if (j < N)
            kept[i] = (i < kSorK && kept[i] < add[j]) ? kept[i] : add[j];
        else if (i >= kSorK)
            kept[i] = 0x7fc00000u;
    }
    // ... merged into ascending order
#pragma unroll
    for (int j = kSorKeep >> 1; j > 0; j >>= 1) {
#pragma unroll
        for (int i = 0; i < kSorKeep; ++i) {
            const int l = i ^ j;
            if (l > i) SOR_CE(kept[i], kept[l]);
        }
    }
    L.nk = L.nk + L.cnt < (uint32_t)kSorKeep ? L.nk + L.cnt : (uint32_t)kSorKeep;
    L.cnt = 0;
    if (kept[kSorK - 1] < 0x7f800000u) L.worst = __uint_as_float(kept[kSorK - 1]);  // (appended distances are finite)
}

// Two candidates (wave-uniform coordinates) against every lane's query, with packed fp32 arithmetic (v_pk_add_f32 /
// v_pk_mul_f32: two IEEE operations per instruction, nothing fused): each squared distance is stored at the lane's write
// position, which advances only when the candidate is below the lane's bound (`bound` = -1 for lanes that are not
// searching).  ((0 + dx*dx) + ... : adding +0 to a product of equal factors changes no bit and is left out.)
typedef float sor_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void sor_candidate_pair(float* __restrict__ row, SorLane& L, float bound, sor_f32x2 qx, sor_f32x2 qy,
                                                   sor_f32x2 qz, sor_f32x2 px, sor_f32x2 py, sor_f32x2 pz)
{
    const sor_f32x2 dx = qx - px, dy = qy - py, dz = qz - pz;
    const sor_f32x2 d = (dx * dx + dy * dy) + dz * dz;
    SOR_AT(row, L.cnt) = d.x;
    sor_inc_if_lt(L.cnt, d.x, bound);
    SOR_AT(row, L.cnt) = d.y;
    sor_inc_if_lt(L.cnt, d.y, bound);
}

// the wave's LDS stage for a chunk of 64 candidates, as three arrays (pairs of neighbouring candidates are one 8-byte read)
struct SorStage {
    float x[kWave], y[kWave], z[kWave];
};

// the points of grid row yy, columns [c0, c1], against the lanes with `live` set
__device__ __forceinline__ void sor_scan_segment(const float4* __restrict__ sxyz, const uint32_t* __restrict__ cell_first, const SorGeom& g,
                                                 int yy, int c0, int c1, float* __restrict__ row, SorStage* __restrict__ stage, SorLane& L,
                                                 uint32_t (&kept)[kSorKeep], bool live, float qx, float qy, float qz)
{
    float bound = live ? L.worst : -1.f;
    if (yy < 0 || yy >= g.gy) return;
    c0 = c0 < 0 ? 0 : c0;
    c1 = c1 >= g.gx ? g.gx - 1 : c1;
    if (c0 > c1) return;
    const int lane = threadIdx.x & 63;
    const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)cell_first[(int64_t)yy * g.gx + c0]);
    const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)cell_first[(int64_t)yy * g.gx + c1 + 1]);
    const sor_f32x2 qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};
    for (uint32_t j0 = s; j0 < e; j0 += kWave) {
        const uint32_t j = j0 + (uint32_t)lane;
        // the chunk's 64 candidates go through a small LDS stage: broadcast reads instead of lane broadcasts through scalar
        // registers (single-wave workgroup: LDS operations of a wave complete in order).  Slots past the end of the
        // segment hold +inf: their distances are +inf, which is below no bound
        const float4 p = sxyz[j < e ? j : e - 1u];
        const bool in = j < e;
        stage->x[lane] = in ? p.x : __builtin_huge_valf();
        stage->y[lane] = in ? p.y : __builtin_huge_valf();
        stage->z[lane] = in ? p.z : __builtin_huge_valf();
        const uint32_t nb = e - j0 < (uint32_t)kWave ? e - j0 : (uint32_t)kWave;
        for (uint32_t b = 0; b < nb; b += 16) {
            sor_f32x2 cx[8], cy[8], cz[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                cx[k] = *reinterpret_cast<const sor_f32x2*>(&stage->x[(b + 2 * k) & 63u]);
                cy[k] = *reinterpret_cast<const sor_f32x2*>(&stage->y[(b + 2 * k) & 63u]);
                cz[k] = *reinterpret_cast<const sor_f32x2*>(&stage->z[(b + 2 * k) & 63u]);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) sor_candidate_pair(row, L, bound, qx2, qy2, qz2, cx[k], cy[k], cz[k]);
            if (__ballot(L.cnt > (uint32_t)kSorMergeAt) != 0ull) {
                sor_merge<kSorAdd>(row, L, kept);
                bound = live ? L.worst : -1.f;
            }
        }
    }
}

__global__ __launch_bounds__(kWave) void k_sor_knn(const float4* __restrict__ sxyz_all, const uint32_t* __restrict__ ids0,
                                                   const uint32_t* __restrict__ ids1, const VoxelGeom* __restrict__ geom,
                                                   const uint32_t* __restrict__ cell_first_all, int64_t cell_stride,
                                                   const SorGeom* __restrict__ sg, int64_t cap, float* __restrict__ dist_all,
                                                   uint32_t* __restrict__ left_list, uint32_t* __restrict__ left_cnt)
{
    __shared__ __attribute__((aligned(16))) float buf[kWave * kSorAddStride];
    __shared__ __attribute__((aligned(16))) SorStage stage_lds;
    SorStage* stage = &stage_lds;
    const int f = blockIdx.y;
    const SorGeom g = sg[f];
    if (!g.active) return;
    const int64_t base = (int64_t)blockIdx.x * kWave;
    if (base >= (int64_t)g.n) return;
    const int lane = threadIdx.x & 63;
    const float4* sxyz = sxyz_all + (int64_t)f * cap;
    const uint32_t* cell_first = cell_first_all + (int64_t)f * cell_stride;
    float* row = buf + lane;
    const bool valid = base + lane < (int64_t)g.n;
    const int64_t qi = valid ? base + lane : (int64_t)g.n - 1;
    const float4 qv = sxyz[qi];
    const float qx = qv.x, qy = qv.y, qz = qv.z;
    const uint32_t out_index = (sorted_buf(geom[f], ids0, ids1) + (int64_t)f * cap)[qi];
    int cx, cy;
    sor_cell(g, qx, qy, cx, cy);
    SorLane L;
    L.worst = __builtin_huge_valf();
    L.cnt = 0;
    L.nk = 0;
    sor_row_clear(row);
    uint32_t kept[kSorKeep];
#pragma unroll
    for (int i = 0; i < kSorKeep; ++i) kept[i] = 0x7fc00000u;
    const int rmax = g.gx > g.gy ? g.gx : g.gy;
    // The shared stream pays as long as most lanes still search.  Real frames have a heavy tail (a depth discontinuity
    // leaves a few points whose 51st neighbour is 0.1 .. 1 m away, the very outliers this filter removes): one such lane
    // would drag its wave through tens of rings.  After ring kSorRingCap the lanes that are not done are handed to
    // k_sor_knn_left (one wave per query, candidates across the lanes).
    bool left = false;
    // the wave's queries sit in one grid row, or (where the sorted array wraps to the next row) in a few: one pass each
    unsigned long long todo = __ballot(valid);
    while (todo != 0ull) {
        const int leader = __builtin_ctzll(todo);
        const int grow = __builtin_amdgcn_readlane(cy, leader);
        const bool mine = valid && cy == grow;
        todo &= ~__ballot(mine);
        const int ca = (int)wave_min_u32(mine ? (uint32_t)cx : 0x7fffffffu);  // first and last cell of the group (cx >= 0)
        const int cb = (int)wave_max_u32(mine ? (uint32_t)cx : 0u);
        bool live = mine;  // still searching
        for (int r = 0; r <= rmax; ++r) {
            // ring r: the full rows grow - r and grow + r, and one cell on either side of every row between them
            const int n_seg = r == 0 ? 1 : 4 * r;
            for (int sg_i = 0; sg_i < n_seg; ++sg_i) {
                int yy = grow, c0 = ca, c1 = cb;
                if (r > 0) {
                    if (sg_i < 2) {
                        yy = sg_i == 0 ? grow - r : grow + r;
                        c0 = ca - r;
                        c1 = cb + r;
                    } else {
                        yy = grow - r + 1 + ((sg_i - 2) >> 1);
                        c0 = c1 = (sg_i & 1) ? cb + r : ca - r;
                    }
                }
                sor_scan_segment(sxyz, cell_first, g, yy, c0, c1, row, stage, L, kept, live, qx, qy, qz);
            }
            // (no test where even the average density cannot have put 51 points within the radius the test certifies)
            if (r > 0 && 3.14159 * r * r * kSorCellPoints >= (double)kSorK) {
                // conservative stop: every cell within the lane's own ring r has been visited (its column lies inside
                // [ca, cb]), so no unvisited point is closer than r*h in XY; the bound is the lane's 51st distance so far
                if (__ballot(live && L.nk + L.cnt >= (uint32_t)kSorK) != 0ull) {
                    const uint32_t most = wave_max_u32(L.cnt);
                    if (most > (uint32_t)(kSorAdd / 2))
                        sor_merge<kSorAdd>(row, L, kept);
                    else if (most != 0u)
                        sor_merge<kSorAdd / 2>(row, L, kept);
                    const double bound = 0.999 * (double)r * (double)g.h;
                    if (live && L.nk >= (uint32_t)kSorK && L.worst < __builtin_huge_valf() && (double)L.worst <= bound * bound) live = false;
                }
            }
            if (__ballot(live) == 0ull) break;
            // (r == rmax: the whole grid has been visited, every lane is exact)
            if (r >= kSorRingCap && r < rmax && __popcll(__ballot(live)) < kSorMinLive) {
                left = left || live;
                break;
            }
        }
    }
    if (left) left_list[(int64_t)f * cap + atomicAdd(&left_cnt[f], 1u)] = (uint32_t)qi;
    // the 51 smallest in ascending order are the front of the kept set: add the square roots front to back
    if (__ballot(L.cnt != 0u) != 0ull) sor_merge<kSorAdd>(row, L, kept);
    double dist_sum = 0.0;
#pragma unroll
    for (int k = 1; k < kSorK; ++k) dist_sum += sqrt((double)__uint_as_float(kept[k]));
    // a query that is handed over leaves its bound - its 51st distance among the candidates of the rings walked here, an
    // upper bound of the final one - in its result slot: k_sor_knn_left starts from it
    if (valid) dist_all[(int64_t)f * cap + out_index] = left ? L.worst : (float)(dist_sum / (double)kSorMeanK);
}

// z range of every cell's points (cell order), for k_sor_knn_left's lower bounds; only for frames that handed queries over
__global__ __launch_bounds__(256) void k_sor_cell_z(const float4* __restrict__ sxyz_all, const uint32_t* __restrict__ cell_first_all,
                                                    int64_t cell_stride, const SorGeom* __restrict__ sg, int64_t cap,
                                                    const uint32_t* __restrict__ left_cnt, float2* __restrict__ cell_z_all)
{
    const int f = blockIdx.y;
    const SorGeom g = sg[f];
    if (!g.active || left_cnt[f] == 0u) return;
    const float4* sxyz = sxyz_all + (int64_t)f * cap;
    const uint32_t* cell_first = cell_first_all + (int64_t)f * cell_stride;
    float2* cell_z = cell_z_all + (int64_t)f * cell_stride;
    const int64_t cells = (int64_t)g.gx * g.gy;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < cells; c += (int64_t)gridDim.x * 256) {
        uint32_t s = cell_first[c], e = cell_first[c + 1];
        if (e > g.n) e = g.n;
        float lo = __builtin_huge_valf(), hi = -__builtin_huge_valf();
        for (uint32_t j = s; j < e; ++j) {
            const float z = sxyz[j].z;
            lo = fminf(lo, z);
            hi = fmaxf(hi, z);
        }
        cell_z[c] = make_float2(lo, hi);  // (an empty cell: +inf, -inf - an infinite gap to every query)
    }
}

// The queries k_sor_knn left over: ONE WAVE PER QUERY, the candidates across the lanes.  The 64 smallest squared distances
// so far sit sorted across the lanes (lane i = i-th smallest); a chunk of 64 candidates is one coalesced load and one
// distance per lane, the ones below the current 51st are inserted one by one (a lane broadcast and a DPP shift each).
// Same distances, same 51 smallest, same ascending fp64 sum as k_sor_knn: bit-identical results.
// These queries are the outliers: a depth spike half a metre off the surface has its 51 nearest neighbours within a few
// cells in XY, but the stop test (XY only) cannot certify that before the square of cells reaches half a metre - 33 x 33
// cells of ~30 points.  So the lanes first take a CELL each: a lower bound of the distance to anything in the cell from
// the cell's rectangle (shrunk by 1e-3 h against the roundings of the cell assignment) and the z range of its points
// (k_sor_cell_z), in the arithmetic and order of the distance itself - every operation is monotone, so the bound is never
// above a computed distance - and only runs of cells whose bound is below the current 51st distance are read.
constexpr int kSorLeftWaves = 4;
__global__ __launch_bounds__(kSorLeftWaves * kWave) void k_sor_knn_left(const float4* __restrict__ sxyz_all, const uint32_t* __restrict__ ids0,
                                                                        const uint32_t* __restrict__ ids1, const VoxelGeom* __restrict__ geom,
                                                                        const uint32_t* __restrict__ cell_first_all, int64_t cell_stride,
                                                                        const SorGeom* __restrict__ sg, int64_t cap,
                                                                        float* __restrict__ dist_all, const uint32_t* __restrict__ left_list,
                                                                        const uint32_t* __restrict__ left_cnt,
                                                                        const float2* __restrict__ cell_z_all)
{
    const int f = blockIdx.y;
    const SorGeom g = sg[f];
    if (!g.active) return;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float2* cell_z = cell_z_all + (int64_t)f * cell_stride;
    const float margin = 1e-3f * g.h;
    const float4* sxyz = sxyz_all + (int64_t)f * cap;
    const uint32_t* cell_first = cell_first_all + (int64_t)f * cell_stride;
    const uint32_t* ids = sorted_buf(geom[f], ids0, ids1) + (int64_t)f * cap;
    const uint32_t n_left = left_cnt[f];
    const int rmax = g.gx > g.gy ? g.gx : g.gy;
    for (uint32_t li = blockIdx.x * kSorLeftWaves + w; li < n_left; li += gridDim.x * kSorLeftWaves) {
        uint32_t qi = left_list[(int64_t)f * cap + li];
        if (qi >= g.n) qi = 0u;  // (never expected)
        const float4 qv = sxyz[qi];
        int cx, cy;
        sor_cell(g, qv.x, qv.y, cx, cy);
        const float seed = dist_all[(int64_t)f * cap + ids[qi]];  // k_sor_knn's bound: nothing above it can be among the 51 smallest
        float best = __builtin_huge_valf();  // ascending across the lanes
        // the square of cells around the query grows geometrically (reach 2, 4, 8, ...: these queries are the outliers, their
        // 51st neighbour is far): a step adds the rows beyond the old reach whole and two side pieces to the rows inside
        // it - long contiguous ranges, 4 R of them per step instead of 2 R^2 single-ring pieces in all
        int reach_old = -1;
        for (int reach = kSorRingCap; ; reach *= 2) {
            if (reach > rmax) reach = rmax;
            for (int yy = cy - reach; yy <= cy + reach; ++yy) {
                if (yy < 0 || yy >= g.gy) continue;
                const bool whole = yy < cy - reach_old || yy > cy + reach_old;
                for (int side = 0; side < (whole ? 1 : 2); ++side) {
                    int c0 = whole ? cx - reach : (side == 0 ? cx - reach : cx + reach_old + 1);
                    int c1 = whole ? cx + reach : (side == 0 ? cx - reach_old - 1 : cx + reach);
                    c0 = c0 < 0 ? 0 : c0;
                    c1 = c1 >= g.gx ? g.gx - 1 : c1;
                    if (c0 > c1) continue;
                    // this row of cells against the query: y gap (the outermost rows are open-ended: sor_cell clamps)
                    // (gaps in the frame of the cell assignment, sor_cell's (x - mn) * inv_h: the roundings then scale with
                    // the cloud's EXTENT, which the margin covers, not with its distance from the origin - a cloud 1 km
                    // out has 6e-5 m per ulp of mn + cell * h, as much as the margin itself)
                    const float ry0 = (float)yy * g.h, uqy = qv.y - g.mny;
                    float gap_y = fmaxf(yy > 0 ? ry0 - uqy : 0.f, yy < g.gy - 1 ? uqy - (ry0 + g.h) : 0.f);
                    gap_y = fmaxf(gap_y - margin, 0.f);
                    for (int cb = c0; cb <= c1; cb += kWave) {
                        const int cc = cb + lane;
                        float lb = __builtin_huge_valf();
                        if (cc <= c1) {
                            const float2 zr = cell_z[(int64_t)yy * g.gx + cc];
                            const float rx0 = (float)cc * g.h, uqx = qv.x - g.mnx;
                            float gap_x = fmaxf(cc > 0 ? rx0 - uqx : 0.f, cc < g.gx - 1 ? uqx - (rx0 + g.h) : 0.f);
                            gap_x = fmaxf(gap_x - margin, 0.f);
                            const float gap_z = fmaxf(fmaxf(zr.x - qv.z, qv.z - zr.y), 0.f);
                            lb = (gap_x * gap_x + gap_y * gap_y) + gap_z * gap_z;
                        }
                        const float w51c = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(best), kSorK - 1));
                        unsigned long long pm = __ballot(lb < w51c && lb <= seed);
                        while (pm != 0ull) {  // runs of neighbouring cells that may hold a neighbour: one contiguous range each
                            const int a = __builtin_ctzll(pm);
                            const unsigned long long rest = ~(pm >> a);
                            const int run = rest != 0ull ? __builtin_ctzll(rest) : kWave - a;
                            pm &= ~((run >= kWave ? ~0ull : ((1ull << run) - 1ull)) << a);
                            const uint32_t s = cell_first[(int64_t)yy * g.gx + cb + a], e = cell_first[(int64_t)yy * g.gx + cb + a + run];
                            for (uint32_t j0 = s; j0 < e; j0 += kWave) {
                                const uint32_t j = j0 + (uint32_t)lane;
                                float d = __builtin_huge_valf();
                                if (j < e) {
                                    const float4 p = sxyz[j];
                                    const float dx = qv.x - p.x, dy = qv.y - p.y, dz = qv.z - p.z;
                                    d = (dx * dx + dy * dy) + dz * dz;
                                }
                                const float w51 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(best), kSorK - 1));
                                unsigned long long m = __ballot(d < w51 && d <= seed);
                                while (m != 0ull) {
                                    const int src = __builtin_ctzll(m);
                                    m &= m - 1ull;
                                    const float v = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(d), src));
                                    // lanes holding more than v move up by one, v lands behind the last lane that holds less or as much
                                    float prev = __uint_as_float((uint32_t)wave_shr1_i32((int32_t)__float_as_uint(best)));
                                    if (lane == 0) prev = -__builtin_huge_valf();
                                    best = best <= v ? best : (prev <= v ? v : prev);
                                }
                            }
                        }
                    }
                }
            }
            // conservative stop: every cell within `reach` of the query's has been visited
            const float w51 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(best), kSorK - 1));
            const double bound = 0.999 * (double)reach * (double)g.h;
            if (reach >= rmax || (w51 < __builtin_huge_valf() && (double)w51 <= bound * bound)) break;
            reach_old = reach;
        }
        // every lane takes the square root of its own entry; the sum walks the lanes in ascending order
        const double root = sqrt((double)best);
        const int root_lo = (int)(uint32_t)__double_as_longlong(root), root_hi = (int)(uint32_t)(__double_as_longlong(root) >> 32);
        double dist_sum = 0.0;
#pragma unroll
        for (int k = 1; k < kSorK; ++k) {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane(root_lo, k), hi = (uint32_t)__builtin_amdgcn_readlane(root_hi, k);
            dist_sum += __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        }
        if (lane == 0) dist_all[(int64_t)f * cap + ids[qi]] = (float)(dist_sum / (double)kSorMeanK);
    }
}

// sum and sum of squares (float product like PCL, fp64 sums): fixed-shape two-level reduction
constexpr int kSorStatBlocks = 256;
__global__ __launch_bounds__(256) void k_sor_partial(const float* __restrict__ dist_all, int64_t cap, const SorGeom* __restrict__ sg,
                                                     double* __restrict__ partial_all /*[frames][blocks][2]*/)
{
    __shared__ double red[2 * 4];
    const int f = blockIdx.y;
    const SorGeom g = sg[f];
    const float* dist = dist_all + (int64_t)f * cap;
    double* partial = partial_all + (int64_t)f * kSorStatBlocks * 2;
    double s = 0.0, q = 0.0;
    if (g.active) {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < g.n; i += (int64_t)gridDim.x * 256) {
            const float d = dist[i];
            s += (double)d;
            q += (double)(d * d);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        q += __shfl_xor(q, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[(threadIdx.x >> 6) * 2] = s;
        red[(threadIdx.x >> 6) * 2 + 1] = q;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = (red[0] + red[2]) + (red[4] + red[6]);
        partial[2 * blockIdx.x + 1] = (red[1] + red[3]) + (red[5] + red[7]);
    }
}
__global__ void k_sor_threshold(const double* __restrict__ partial_all, double stddev_mul, SorGeom* __restrict__ sg, int frames)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= frames) return;
    const double* partial = partial_all + (int64_t)f * kSorStatBlocks * 2;
    double sum = 0.0, sq = 0.0;
    for (int b = 0; b < kSorStatBlocks; ++b) {
        sum += partial[2 * b];
        sq += partial[2 * b + 1];
    }
    const double n = (double)sg[f].n;
    const double mean = sum / n;
    const double variance = (sq - sum * sum / n) / (n - 1.0);
    sg[f].threshold = mean + stddev_mul * sqrt(variance);
}

// ordered compaction of the inliers (count per 1024-point tile, scan, emit) + their bounding boxes
__global__ __launch_bounds__(256) void k_sor_count(const float* __restrict__ dist_all, int64_t cap, const SorGeom* __restrict__ sg,
                                                   int n_tiles, uint32_t* __restrict__ tile_cnt)
{
    __shared__ uint32_t lds[4];
    const int f = blockIdx.y;
    const SorGeom g = sg[f];
    const float* dist = dist_all + (int64_t)f * cap;
    uint32_t c = 0;
    const int64_t base = (int64_t)blockIdx.x * 1024;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        if (i < g.n) c += (!g.active || !((double)dist[i] > g.threshold)) ? 1u : 0u;
    }
    c = wave_sum_u32(c);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[(int64_t)f * n_tiles + blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}
__global__ __launch_bounds__(256) void k_sor_emit(const o3dr_point* __restrict__ in_all, int64_t in_fstride, const float* __restrict__ dist_all,
                                                  int64_t cap, const SorGeom* __restrict__ sg, int n_tiles,
                                                  const uint32_t* __restrict__ tile_off, o3dr_point* __restrict__ out_all,
                                                  int64_t out_fstride, int64_t mm_stride, float* __restrict__ mm)
{
    __shared__ uint32_t scan_lds[5];
    __shared__ float mm_lds[6 * 4];
    const int f = blockIdx.y;
    const SorGeom g = sg[f];
    const float* dist = dist_all + (int64_t)f * cap;
    const o3dr_point* in = in_all + (int64_t)f * in_fstride;
    o3dr_point* out = out_all + (int64_t)f * out_fstride;
    const int64_t base = (int64_t)blockIdx.x * 1024;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    bool any = false;
    uint32_t off = tile_off[(int64_t)f * n_tiles + blockIdx.x];
    for (int j = 0; j < 4; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        const bool keep = (i < g.n) && (!g.active || !((double)dist[i] > g.threshold));
        uint32_t total;
        const uint32_t pos = block_excl_scan_u32<4>(keep ? 1u : 0u, scan_lds, total);
        if (keep) {
            const uint4 v = reinterpret_cast<const uint4*>(in)[i];
            reinterpret_cast<uint4*>(out)[off + pos] = v;
            const float x = __uint_as_float(v.x), y = __uint_as_float(v.y), z = __uint_as_float(v.z);
            lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
            lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
            lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
            any = true;
        }
        off += total;
    }
    block_minmax_store<4>(lo, hi, any, mm_lds, mm + ((int64_t)f * mm_stride + blockIdx.x) * 6);
}
