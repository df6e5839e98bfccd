// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Exact nearest neighbour and the ICP pass (o3dr_nearest_neighbors, o3dr_icp_align; DESIGN.md "ICP")
//   The target's search grid is SOR's (launch_search_grid: cells sorted with the radix sort, points gathered into cell
//   order with their original index in .w), built with ~kNnCellPoints points per column.  For every query the point of
//   the target minimising the key (d2, original index) with d2 = ((0 + dx*dx) + dy*dy) + dz*dz in fp32 and d2 <= r2.
//   ONE LANE PER QUERY, queries in the caller's order: the lane walks rings of cells around its own cell; a cell is read
//   only when the lower bound of its points' distances - from the cell's exact bounding box, in the arithmetic of the
//   distance itself, so never above a computed distance - is <= the best distance so far and <= r2.  After ring r the lane
//   stops once no unvisited cell can hold a point as close as its best (or within r2): the cells outside the ring's square
//   lie in four strips of the target's box whose distance from the query is bounded from below (cell assignment
//   (x - mn) * inv_h in fp32: within 4 ulps of the real quotient, taken as 1e-6 relative).
//   The ICP pass fuses the query transform (A2, a2_apply), the search and the epilogue: index (+ d2), "index changed since
//   the previous pass" per workgroup and the fp64 moments per workgroup (rigid_moments, wave_fields, tree4 of
//   kernels/rigid_core.inc), folded in workgroup order by k_icp_fold (fold_partials); the host solves the record with
//   rigid_solve (o3dr_rigid_solve.h).
// =================================================================================================
constexpr double kNnCellPoints = 8.0;  // target points per column of the grid (SOR's grid: kSorCellPoints)
constexpr int kNnThreads = 256;        // queries per workgroup = the fixed partition of the moment sums
constexpr int kIcpFields = kIcpRecord;  // the rigid record, ICP_D2, ICP_CHANGED

// exact bounding box of every cell's points (empty cell: +inf .. -inf, a lower bound of +inf)
__global__ __launch_bounds__(256) void k_nn_cell_box(const float4* __restrict__ sxyz, const uint32_t* __restrict__ cell_first,
                                                     const SorGeom* __restrict__ sg, float4* __restrict__ cell_lo,
                                                     float4* __restrict__ cell_hi)
{
    const SorGeom g = sg[0];
    const int64_t cells = (int64_t)g.gx * g.gy;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < cells; c += (int64_t)gridDim.x * 256) {
        uint32_t s = cell_first[c], e = cell_first[c + 1];
        if (e > g.n) e = g.n;
        float4 lo = make_float4(__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf(), 0.f);
        float4 hi = make_float4(-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf(), 0.f);
        for (uint32_t j = s; j < e; ++j) {
            const float4 p = sxyz[j];
            lo.x = fminf(lo.x, p.x); hi.x = fmaxf(hi.x, p.x);
            lo.y = fminf(lo.y, p.y); hi.y = fmaxf(hi.y, p.y);
            lo.z = fminf(lo.z, p.z); hi.z = fmaxf(hi.z, p.z);
        }
        cell_lo[c] = lo;
        cell_hi[c] = hi;
    }
}

struct NnArgs {
    const o3dr_point* query;  // n queries in the caller's order
    uint32_t n;
    int32_t xf;               // 1: the query is a2_apply(T, point) (the ICP pass); 0: the point as it is
    Mat34 T;
    SearchGrid grid;          // the target's
    float r2;
    uint32_t* idx_out;        // n
    float* d2_out;            // n or nullptr
    const uint32_t* idx_prev; // n or nullptr: the previous pass's indices ("changed" is counted against them)
    double c0[3];             // centre of the moments
    double* partial;          // kIcpFields * n_blocks (field-major) or nullptr
    uint32_t n_blocks;
};

__device__ __forceinline__ void nn_visit(const NnArgs& a, int64_t c, float qx, float qy, float qz, float r2,
                                         unsigned long long& best, float4& bp)
{
    const float bd = best != ~0ull ? __uint_as_float((uint32_t)(best >> 32)) : __builtin_huge_valf();
    const float4 lo = a.grid.cell_lo[c], hi = a.grid.cell_hi[c];
    const float lb = cell_box_d2_lower_bound(lo, hi, qx, qy, qz);
    if (!(lb <= bd && lb <= r2)) return;
    const uint32_t s = a.grid.cell_first[c], e = a.grid.cell_first[c + 1];
    for (uint32_t j = s; j < e; ++j) {
        const float4 p = a.grid.xyz[j];
        const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned long long)__float_as_uint(p.w);
        if (d <= r2 && key < best) {  // d >= 0: the key orders like (d2, index)
            best = key;
            bp = p;
        }
    }
}

// lower bound (real arithmetic, in double) of the squared XY distance from q to every target point outside the cells within
// ring r of (cx, cy); +inf when no such cell exists
__device__ __forceinline__ double nn_unvisited_bound(const SorGeom& g, const float* box6, int cx, int cy, int r, double qx, double qy)
{
    const double h = (double)g.h, mnx = (double)g.mnx, mny = (double)g.mny;
    const double bx0 = (double)box6[0], by0 = (double)box6[1], bx1 = (double)box6[3], by1 = (double)box6[4];
    const double ox = qx < bx0 ? bx0 - qx : (qx > bx1 ? qx - bx1 : 0.0);  // distance to the box along x / y
    const double oy = qy < by0 ? by0 - qy : (qy > by1 ? qy - by1 : 0.0);
    double lb = __builtin_huge_val();
    if (cx - r > 0) {  // columns < cx - r: x < mn + (cx - r) h
        const double u = mnx + (double)(cx - r) * h * (1.0 + 1e-6), d = qx > u ? qx - u : 0.0;
        lb = fmin(lb, d * d + oy * oy);
    }
    if (cx + r < g.gx - 1) {  // columns > cx + r: x >= mn + (cx + r + 1) h
        const double l = mnx + (double)(cx + r + 1) * h * (1.0 - 1e-6), d = l > qx ? l - qx : 0.0;
        lb = fmin(lb, d * d + oy * oy);
    }
    if (cy - r > 0) {
        const double u = mny + (double)(cy - r) * h * (1.0 + 1e-6), d = qy > u ? qy - u : 0.0;
        lb = fmin(lb, d * d + ox * ox);
    }
    if (cy + r < g.gy - 1) {
        const double l = mny + (double)(cy + r + 1) * h * (1.0 - 1e-6), d = l > qy ? l - qy : 0.0;
        lb = fmin(lb, d * d + ox * ox);
    }
    return lb;
}

__global__ __launch_bounds__(kNnThreads) void k_nn_query(NnArgs a)
{
    __shared__ double red[kIcpFields][kNnThreads / kWave];
    const int64_t i = (int64_t)blockIdx.x * kNnThreads + threadIdx.x;
    const bool valid = i < (int64_t)a.n;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (valid) {
        const float4 v = reinterpret_cast<const float4*>(a.query)[i];
        if (a.xf)
            a2_apply(a.T.m, v.x, v.y, v.z, qx, qy, qz);
        else
            qx = v.x, qy = v.y, qz = v.z;
    }
    unsigned long long best = ~0ull;
    float4 bp = make_float4(0.f, 0.f, 0.f, 0.f);
    const SorGeom g = *a.grid.geom;
    const float r2 = a.r2;
    // (a query with a non-finite coordinate has no neighbour)
    if (valid && g.active && g.n > 0 && isfinite(qx) && isfinite(qy) && isfinite(qz)) {
        int cx, cy;
        sor_cell(g, qx, qy, cx, cy);
        for (int r = 0;; ++r) {
            const int y0 = cy - r < 0 ? 0 : cy - r, y1 = cy + r >= g.gy ? g.gy - 1 : cy + r;
            const int x0 = cx - r < 0 ? 0 : cx - r, x1 = cx + r >= g.gx ? g.gx - 1 : cx + r;
            for (int yy = y0; yy <= y1; ++yy) {
                const int64_t row = (int64_t)yy * g.gx;
                if (yy == cy - r || yy == cy + r) {
                    for (int xx = x0; xx <= x1; ++xx) nn_visit(a, row + xx, qx, qy, qz, r2, best, bp);
                } else {
                    if (cx - r >= 0) nn_visit(a, row + cx - r, qx, qy, qz, r2, best, bp);
                    if (cx + r < g.gx) nn_visit(a, row + cx + r, qx, qy, qz, r2, best, bp);
                }
            }
            const double lb = nn_unvisited_bound(g, a.grid.box6, cx, cy, r, (double)qx, (double)qy);
            if (lb == __builtin_huge_val()) break;  // every cell visited
            const double thr = lb * (1.0 - 4e-6) - 1e-30;  // below the computed d2 of every unvisited point
            const double bd = best != ~0ull ? (double)__uint_as_float((uint32_t)(best >> 32)) : __builtin_huge_val();
            if (bd < thr || (double)r2 < thr) break;
        }
    }
    const bool found = best != ~0ull;
    const uint32_t idx = found ? (uint32_t)best : 0xFFFFFFFFu;
    const float d2 = found ? __uint_as_float((uint32_t)(best >> 32)) : __builtin_huge_valf();
    if (valid) {
        a.idx_out[i] = idx;
        if (a.d2_out) a.d2_out[i] = d2;
    }
    if (!a.partial) return;
    // the epilogue of the ICP pass: fixed partition (kNnThreads queries per workgroup), fixed reduction tree
    const bool corr = valid && found;
    double v[kIcpFields];
    rigid_moments(corr, make_float4(qx, qy, qz, 0.f), bp, a.c0, v);
    v[ICP_D2] = corr ? (double)d2 : 0.0;
    v[ICP_CHANGED] = (valid && a.idx_prev && a.idx_prev[i] != idx) ? 1.0 : 0.0;
    wave_fields<kIcpFields>(v, red, threadIdx.x & 63, threadIdx.x >> 6);
    __syncthreads();
    if (threadIdx.x < kIcpFields) {
        const int k = threadIdx.x;
        a.partial[(int64_t)k * a.n_blocks + blockIdx.x] = tree4(red[k]);
    }
}
static_assert(kNnThreads == 4 * kWave && kNnThreads == 256, "tree4 adds four waves; nn_partial_blocks");

// one workgroup per field: the per-workgroup partials summed in a fixed order (fold_partials) -> rec[field]
__global__ __launch_bounds__(kRigidFoldThreads) void k_icp_fold(const double* __restrict__ partial, uint32_t n_blocks, double* __restrict__ rec)
{
    __shared__ double red[kRigidFoldThreads / kWave];
    const int k = blockIdx.x;
    const double t = fold_partials(partial + (int64_t)k * n_blocks, n_blocks, red);
    if (threadIdx.x == 0) rec[k] = t;
}
