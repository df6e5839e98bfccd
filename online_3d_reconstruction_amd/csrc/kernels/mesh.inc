// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Height-field surface mesh (o3dr_mesh_surface; contract: include/o3dr.h, DESIGN.md "Surface mesh")
//   Cells: the cloud's cell order (kernels/cell_order.inc) with FloorCell as the index rule: cells in (cy, cx) order, the
//   lowest input index first inside a cell.  The first point of every cell is its vertex, the cell ordinals are the
//   vertex ordinals, and k_mesh_vertices gathers them (key = the dense cell id (cy - cy_min) * wx + (cx - cx_min),
//   x y z + input index).
//   Neighbours: the left and right cells are the adjacent ordinals when their keys are; the three cells of the row above
//   (ul, u, ur) are consecutive keys, found by one binary search; the row below (normals only) likewise.
//   A quad belongs to its first present corner in a, b, c, d order, so to `a` or, when `a` is empty, to `b`: a vertex owns
//   the quad to its left (it is that quad's b) and then its own.  Walking the vertices in cell order walks the quads in
//   ascending (cy, cx): k_mesh_count counts every vertex's kept triangles, an exclusive scan gives the offsets and
//   k_mesh_emit writes them, recomputing the same quads (mesh_quad is the one place that decides a quad).
//   k_mesh_normals gathers the up to four quads around every vertex.  All counts are integer sums: per-workgroup partials
//   folded by one workgroup (k_fold4_u32), no atomics.
// =================================================================================================
constexpr int kMeshThreads = kFoldThreads;  // (block_reduce4_u32)

// orient(p, q, r) of the contract: fp64 from the fp32 coordinates, no FMA (the file is built with -ffp-contract=off)
__device__ __forceinline__ double mesh_orient(const float4& p, const float4& q, const float4& r)
{
    return ((double)q.x - (double)p.x) * ((double)r.y - (double)p.y) - ((double)q.y - (double)p.y) * ((double)r.x - (double)p.x);
}
// the edge's d2 in fp32, as o3dr_nearest_neighbors computes it
__device__ __forceinline__ float mesh_d2(const float4& p, const float4& q)
{
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    return ((0.f + dx * dx) + dy * dy) + dz * dz;
}

// The candidate triangles of one quad (corner ordinals a b c d, -1 = empty) and which of them are kept.  Returns the
// candidate count (0, 1 or 2); tri[k] are vertex ordinals, counter-clockwise in XY; why[k]: 0 kept, 1 orientation, 2 length.
__device__ __forceinline__ int mesh_quad(const float4* __restrict__ vpt, float lf, const int32_t cor[4], int32_t tri[2][3], int why[2])
{
    const int present = (cor[0] >= 0) + (cor[1] >= 0) + (cor[2] >= 0) + (cor[3] >= 0);
    if (present < 3) return 0;
    int cand;
    if (present == 4) {
        const float4 A = vpt[cor[0]], B = vpt[cor[1]], C = vpt[cor[2]], D = vpt[cor[3]];
        const bool ac_ok = mesh_orient(A, B, C) > 0.0 && mesh_orient(A, C, D) > 0.0;
        const bool bd_ok = mesh_orient(A, B, D) > 0.0 && mesh_orient(B, C, D) > 0.0;
        const bool bd = bd_ok && (!ac_ok || mesh_d2(B, D) < mesh_d2(A, C));
        if (bd) {
            tri[0][0] = cor[0], tri[0][1] = cor[1], tri[0][2] = cor[3];
            tri[1][0] = cor[1], tri[1][1] = cor[2], tri[1][2] = cor[3];
        } else {
            tri[0][0] = cor[0], tri[0][1] = cor[1], tri[0][2] = cor[2];
            tri[1][0] = cor[0], tri[1][1] = cor[2], tri[1][2] = cor[3];
        }
        cand = 2;
    } else {  // the corners in a b c d order, the empty one skipped: (b,c,d), (a,c,d), (a,b,d) or (a,b,c)
        int k = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (cor[j] >= 0 && k < 3) tri[0][k++] = cor[j];
        cand = 1;
    }
    for (int t = 0; t < cand; ++t) {
        const float4 P = vpt[tri[t][0]], Q = vpt[tri[t][1]], R = vpt[tri[t][2]];
        if (!(mesh_orient(P, Q, R) > 0.0)) why[t] = 1;
        else if (!(mesh_d2(P, Q) <= lf && mesh_d2(Q, R) <= lf && mesh_d2(R, P) <= lf)) why[t] = 2;
        else why[t] = 0;
    }
    return cand;
}

// first j in [lo, hi) with keys[j] >= key (hi if none)
__device__ __forceinline__ uint32_t mesh_lower_bound(const uint32_t* __restrict__ keys, uint32_t lo, uint32_t hi, uint64_t key)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// the vertices of cells (cx-1, cx, cx+1) of the row dy (keys row * wx + ...), searched in [lo, hi); -1 where empty
__device__ __forceinline__ void mesh_row3(const MeshArgs& a, uint64_t row, uint64_t dx, uint32_t lo, uint32_t hi, int32_t out[3])
{
    out[0] = out[1] = out[2] = -1;
    const uint64_t base = row * a.cells.wx + dx;  // the key of cell dx of that row
    const uint64_t first = dx > 0 ? base - 1 : base, last = dx + 1 < a.cells.wx ? base + 1 : base;
    uint32_t j = mesh_lower_bound(a.vkey, lo, hi, first);
    for (; j < hi && (uint64_t)a.vkey[j] <= last; ++j) out[(int)((uint64_t)a.vkey[j] + 1 - base)] = (int32_t)j;
}

// ---- cells ---------------------------------------------------------------------------------------
static inline FloorCell cell_of(const MeshArgs& a) { return FloorCell{a.inv}; }

// the vertices in cell order (the first point of every cell, at its ordinal): key, and x y z with the input index in .w
__global__ __launch_bounds__(kMeshThreads) void k_mesh_vertices(MeshArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (i >= (int64_t)a.n) return;
    if (!cell_head(a.cells, i)) return;
    const uint32_t o = a.cells.ord[i], idx = a.cells.perm[i];
    const float4 p = reinterpret_cast<const float4*>(a.cloud)[idx];
    a.vkey[o] = a.cells.keys[i];
    a.vpt[o] = make_float4(p.x, p.y, p.z, __uint_as_float(idx));
}

// a vertex's two quads (left: it is b and a is empty; own: it is a) as corner ordinals; nbr = right, ur, u, ul.  When the
// left cell is occupied the left quad belongs to that vertex: b is blanked too, which leaves at most two corners.
__device__ __forceinline__ void mesh_owned(const MeshArgs& a, uint32_t o, uint32_t V, int32_t left_quad[4], int32_t own_quad[4],
                                           int4& nbr)
{
    const uint64_t key = a.vkey[o], dx = key % a.cells.wx, dy = key / a.cells.wx;
    const bool has_left = dx > 0 && o > 0 && (uint64_t)a.vkey[o - 1] + 1 == key;
    const int32_t right = (dx + 1 < a.cells.wx && o + 1 < V && (uint64_t)a.vkey[o + 1] == key + 1) ? (int32_t)(o + 1) : -1;
    int32_t up[3] = {-1, -1, -1};
    if (dy + 1 < a.cells.wy) mesh_row3(a, dy + 1, dx, o + 1, V, up);
    nbr = make_int4(right, up[2], up[1], up[0]);
    left_quad[0] = -1, left_quad[1] = has_left ? -1 : (int32_t)o, left_quad[2] = up[1], left_quad[3] = up[0];
    own_quad[0] = (int32_t)o, own_quad[1] = right, own_quad[2] = up[2], own_quad[3] = up[1];
}

// per vertex: its kept triangles (-> cnt, scanned into offsets next); full quads and rejections summed per workgroup.
// Ordinals >= V (up to n) write 0 so that the scan can run over n words.
__global__ __launch_bounds__(kMeshThreads) void k_mesh_count(MeshArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    const uint32_t V = *a.cells.n_runs;
    uint32_t kept = 0, full = 0, rej_o = 0, rej_l = 0;
    if (i < (int64_t)V) {
        int32_t q[2][4];
        int4 nbr;
        mesh_owned(a, (uint32_t)i, V, q[0], q[1], nbr);
        a.nbr[i] = nbr;
        for (int k = 0; k < 2; ++k) {
            int32_t tri[2][3];
            int why[2];
            const int cand = mesh_quad(a.vpt, a.lf, q[k], tri, why);
            if (cand == 2) ++full;
            for (int t = 0; t < cand; ++t) kept += why[t] == 0, rej_o += why[t] == 1, rej_l += why[t] == 2;
        }
    }
    if (i < (int64_t)a.n) a.cnt[i] = kept;
    uint32_t v[4] = {full, rej_o, rej_l, 0u};
    const int op[4] = {2, 2, 2, 2};
    block_reduce4_u32(v, op, a.part + (int64_t)blockIdx.x * kPartWords);
}

// per vertex: its kept triangles at its scanned offset, as input indices
__global__ __launch_bounds__(kMeshThreads) void k_mesh_emit(MeshArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    const uint32_t V = *a.cells.n_runs;
    if (i >= (int64_t)V) return;
    const int4 nbr = a.nbr[i];
    const uint64_t key = a.vkey[i];
    const bool has_left = key % a.cells.wx > 0 && i > 0 && (uint64_t)a.vkey[i - 1] + 1 == key;
    const int32_t q[2][4] = {{-1, has_left ? -1 : (int32_t)i, nbr.z, nbr.w}, {(int32_t)i, nbr.x, nbr.y, nbr.z}};
    int64_t at = (int64_t)a.cnt[i] * 3;
    for (int k = 0; k < 2; ++k) {
        int32_t tri[2][3];
        int why[2];
        const int cand = mesh_quad(a.vpt, a.lf, q[k], tri, why);
        for (int t = 0; t < cand; ++t) {
            if (why[t] != 0) continue;
#pragma unroll
            for (int j = 0; j < 3; ++j) a.tris[at + j] = (int32_t)__float_as_uint(a.vpt[tri[t][j]].w);
            at += 3;
        }
    }
}

// per sorted point: a cell's vertex gets the normalised fp64 sum of the face normals of the kept triangles that use it,
// from the quads with lower-left cells (cx-1,cy-1), (cx,cy-1), (cx-1,cy), (cx,cy) in that order; shadowed points and
// vertices without a triangle get NaN
__global__ __launch_bounds__(kMeshThreads) void k_mesh_normals(MeshArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kMeshThreads + threadIdx.x;
    if (i >= (int64_t)a.n) return;
    const uint32_t idx = a.cells.perm[i];
    float* dst = a.normals + (int64_t)idx * 3;
    const float nan = __builtin_nanf("");
    if (!cell_head(a.cells, i)) {
        dst[0] = nan, dst[1] = nan, dst[2] = nan;
        return;
    }
    const uint32_t o = a.cells.ord[i];
    const int4 nbr = a.nbr[o];
    const uint64_t key = a.vkey[o], dx = key % a.cells.wx, dy = key / a.cells.wx;
    const int32_t left = (dx > 0 && o > 0 && (uint64_t)a.vkey[o - 1] + 1 == key) ? (int32_t)(o - 1) : -1;
    int32_t down[3] = {-1, -1, -1};
    if (dy > 0) mesh_row3(a, dy - 1, dx, 0, o, down);
    const int32_t me = (int32_t)o;
    const int32_t q[4][4] = {{down[0], down[1], me, left}, {down[1], down[2], nbr.x, me}, {left, me, nbr.z, nbr.w}, {me, nbr.x, nbr.y, nbr.z}};
    double sx = 0.0, sy = 0.0, sz = 0.0;
    bool any = false;
    for (int k = 0; k < 4; ++k) {
        int32_t tri[2][3];
        int why[2];
        const int cand = mesh_quad(a.vpt, a.lf, q[k], tri, why);
        for (int t = 0; t < cand; ++t) {
            if (why[t] != 0 || (tri[t][0] != me && tri[t][1] != me && tri[t][2] != me)) continue;
            const float4 P = a.vpt[tri[t][0]], Q = a.vpt[tri[t][1]], R = a.vpt[tri[t][2]];
            const double ex = (double)Q.x - (double)P.x, ey = (double)Q.y - (double)P.y, ez = (double)Q.z - (double)P.z;
            const double fx = (double)R.x - (double)P.x, fy = (double)R.y - (double)P.y, fz = (double)R.z - (double)P.z;
            sx = sx + (ey * fz - ez * fy);
            sy = sy + (ez * fx - ex * fz);
            sz = sz + (ex * fy - ey * fx);
            any = true;
        }
    }
    const double len = sqrt((sx * sx + sy * sy) + sz * sz);
    if (!any || !(len > 0.0)) {
        dst[0] = nan, dst[1] = nan, dst[2] = nan;
        return;
    }
    dst[0] = (float)(sx / len), dst[1] = (float)(sy / len), dst[2] = (float)(sz / len);
}
