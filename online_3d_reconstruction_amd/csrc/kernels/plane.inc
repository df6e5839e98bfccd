// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// RANSAC plane segmentation per XY tile (o3dr_segment_plane; contract: include/o3dr.h, DESIGN.md "Plane segmentation")
//   Tiles: the cloud's cell order (kernels/cell_order.inc) with PlaneCell as the index rule: tiles in (iy, ix) order, input
//   order inside a tile; the points are gathered into it (x y z, original index in .w).  With tile_size 0 the cloud is
//   one tile and the cloud itself is read in place.  Every tile is cut into CHUNKS of kPlaneChunk consecutive points
//   (the last one partial); one wave owns one chunk, two points per lane (lane j: points j and 64 + j of the chunk).
//   k_plane_sample: one lane per (tile, hypothesis): the three draws (draw3, kernels/rigid_core.inc) and the fp64 plane, rounded to fp32 (NaN: degenerate).
//   k_plane_score: a wave keeps its chunk in registers and walks its tile's H hypotheses, whose coefficients are uniform
//   (scalar loads); each test's lane masks are popcounted, lane j of a 64-hypothesis block keeps hypothesis j's count and
//   adds it with one integer atomic per (wave, hypothesis): exact counts, no order dependence.
//   k_plane_best: one wave per tile (largest count, smallest h).  k_plane_moments / k_plane_refine: the fp64 moments of
//   the chosen plane's inliers per chunk, folded per tile in a fixed order (as k_icp_fold), then the Jacobi of MLS.
//   k_plane_label: labels, projection and tile ordinals, scattered to input order, and the final counts per tile.
// =================================================================================================
constexpr int kPlaneChunk = kPlaneChunkPoints;  // points per wave chunk: two per lane
constexpr int kPlaneThreads = 256;      // four chunks per workgroup
constexpr int kPlaneMoments = kPlaneMomentsHost;  // k, sum e, sum e e^T (upper triangle), e = p - p0
typedef float f32x2_t __attribute__((ext_vector_type(2)));
static_assert(kPlaneChunk == 2 * kWave, "two points per lane");

__device__ __forceinline__ uint64_t plane_tile_key(const o3dr_plane_tile& r)
{
    return ((uint64_t)(uint32_t)r.iy << 32) | (uint64_t)(uint32_t)r.ix;
}
// orientation rule of the contract: nz > 0, then ny > 0, then nx > 0
__device__ __forceinline__ bool plane_flip(double nx, double ny, double nz)
{
    return nz < 0.0 || (nz == 0.0 && (ny < 0.0 || (ny == 0.0 && nx < 0.0)));
}
// the tile a wave's chunk belongs to: t with cfirst[t] <= w < cfirst[t + 1] (every tile has at least one chunk)
__device__ __forceinline__ uint32_t plane_chunk_tile(const uint32_t* cfirst, uint32_t n_tiles, uint32_t w)
{
    uint32_t lo = 0, hi = n_tiles;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cfirst[mid] <= w) lo = mid;
        else hi = mid;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)lo);
}
// a wave's chunk: tile t, its points [b, e) in tile order; false past the last chunk
struct PlaneChunk {
    uint32_t t, b, e, m;
};
__device__ __forceinline__ bool plane_chunk(const PlaneArgs& a, uint32_t w, PlaneChunk& c)
{
    if (w >= a.cfirst[a.n_tiles]) return false;
    c.t = plane_chunk_tile(a.cfirst, a.n_tiles, w);
    const uint32_t t0 = a.tstart[c.t], t1 = a.tstart[c.t + 1];
    c.m = t1 - t0;
    c.b = t0 + (w - a.cfirst[c.t]) * (uint32_t)kPlaneChunk;
    c.e = c.b + (uint32_t)kPlaneChunk < t1 ? c.b + (uint32_t)kPlaneChunk : t1;
    return true;
}
// the lane's two points of the chunk (NaN past its end: no test passes on them)
__device__ __forceinline__ void plane_load2(const PlaneArgs& a, const PlaneChunk& c, int lane, float4 p[2], bool ok[2])
{
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const uint32_t i = c.b + (uint32_t)(lane + k * kWave);
        ok[k] = i < c.e;
        const float nan = __builtin_nanf("");
        p[k] = ok[k] ? a.pts[i] : make_float4(nan, nan, nan, 0.f);
    }
}
__device__ __forceinline__ uint32_t plane_index(const PlaneArgs& a, const float4& p, uint32_t pos)
{
    return a.tiled ? __float_as_uint(p.w) : pos;
}
// the contract's signed distance: ((A x + B y) + C z) + D in fp32, two points per packed operation
__device__ __forceinline__ f32x2_t plane_dist2(const float4& c, f32x2_t X, f32x2_t Y, f32x2_t Z)
{
    return ((c.x * X + c.y * Y) + c.z * Z) + c.w;
}

// ---- tiles ----------------------------------------------------------------------------------------
// the contract's tile index floor((double)x / s), in double (the cell functor of kernels/cell_order.inc)
struct PlaneCell {
    double s;
    __device__ __forceinline__ bool operator()(const float4& p, int32_t& ix, int32_t& iy) const
    {
        const double fx = floor((double)p.x / s), fy = floor((double)p.y / s);
        if (!(fx >= -2147483648.0 && fx <= 2147483647.0 && fy >= -2147483648.0 && fy <= 2147483647.0)) return false;
        ix = (int32_t)fx, iy = (int32_t)fy;
        return true;
    }
};
static inline PlaneCell cell_of(const PlaneArgs& a) { return PlaneCell{a.s}; }

// the points gathered into tile order: x y z, the input index in .w
__global__ __launch_bounds__(256) void k_plane_gather(PlaneArgs a, float4* __restrict__ pts)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.n) return;
    const uint32_t idx = a.cells.perm[i];
    const float4 p = reinterpret_cast<const float4*>(a.cloud)[idx];
    pts[i] = make_float4(p.x, p.y, p.z, __uint_as_float(idx));
}
// tile starts and indices from the cell order (tiled), or the one tile of the whole cloud
__global__ __launch_bounds__(256) void k_plane_tiles(PlaneArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (!a.tiled) {
        if (i == 0) {
            a.tstart[0] = 0u, a.tstart[1] = a.n;
            a.rec[0].ix = 0, a.rec[0].iy = 0;
        }
        return;
    }
    if (i >= (int64_t)a.n) return;
    if (i == 0) a.tstart[a.n_tiles] = a.n;
    if (!cell_head(a.cells, i)) return;
    const uint32_t t = a.cells.ord[i];
    a.tstart[t] = (uint32_t)i;
    const uint32_t key = a.cells.keys[i], wx = (uint32_t)a.cells.wx;  // (at most 2^32-1 tiles: wx fits)
    a.rec[t].ix = (int32_t)((uint32_t)a.cells.x0 + key % wx);
    a.rec[t].iy = (int32_t)((uint32_t)a.cells.y0 + key / wx);
}
// per tile: its chunk count (-> cfirst by an exclusive scan) and the record's defaults
__global__ __launch_bounds__(256) void k_plane_chunks(PlaneArgs a)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_tiles) return;
    const uint32_t m = a.tstart[t + 1] - a.tstart[t];
    a.cfirst[t] = (m + (uint32_t)kPlaneChunk - 1) / (uint32_t)kPlaneChunk;
    o3dr_plane_tile& r = a.rec[t];
    const float nan = __builtin_nanf("");
    r.coeff[0] = nan, r.coeff[1] = nan, r.coeff[2] = nan, r.coeff[3] = nan;
    r.n_points = m;
    r.n_inliers = 0u;
    r.ransac_inliers = 0u;
    r.hypothesis = -1;
    r.sample[0] = 0xffffffffu, r.sample[1] = 0xffffffffu, r.sample[2] = 0xffffffffu;
    r.refined = 0;
    r.status = m < 3u ? O3DR_PLANE_TOO_FEW : O3DR_PLANE_DEGENERATE;  // OK once k_plane_best finds a plane
    r.reserved = 0u;
}

// ---- hypotheses -----------------------------------------------------------------------------------
// the tile-order position of local index `loc` of tile t, and the point there
__device__ __forceinline__ float4 plane_point(const PlaneArgs& a, uint32_t t0, uint32_t loc) { return a.pts[t0 + loc]; }

__global__ __launch_bounds__(256) void k_plane_sample(PlaneArgs a)
{
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (uint64_t)a.n_tiles * a.H) return;
    const uint32_t t = (uint32_t)(g / a.H), h = (uint32_t)(g % a.H);
    const uint32_t t0 = a.tstart[t], m = a.tstart[t + 1] - t0;
    const float nan = __builtin_nanf("");
    float4 out = make_float4(nan, nan, nan, nan);
    if (m >= 3u) {
        uint32_t loc[3];
        draw3(splitmix64(a.seed ^ plane_tile_key(a.rec[t])), h, m, loc);
        const float4 p0 = plane_point(a, t0, loc[0]), p1 = plane_point(a, t0, loc[1]), p2 = plane_point(a, t0, loc[2]);
        const double x0 = p0.x, y0 = p0.y, z0 = p0.z;
        const double e1x = (double)p1.x - x0, e1y = (double)p1.y - y0, e1z = (double)p1.z - z0;
        const double e2x = (double)p2.x - x0, e2y = (double)p2.y - y0, e2z = (double)p2.z - z0;
        const double ca = e1y * e2z - e1z * e2y, cb = e1z * e2x - e1x * e2z, cc = e1x * e2y - e1y * e2x;
        const double L2 = (ca * ca + cb * cb) + cc * cc;
        const double n1 = (e1x * e1x + e1y * e1y) + e1z * e1z, n2 = (e2x * e2x + e2y * e2y) + e2z * e2z;
        const bool same = loc[0] == loc[1] || loc[0] == loc[2] || loc[1] == loc[2];
        if (!same && L2 > 1e-12 * n1 * n2) {
            const double len = sqrt(L2);
            double nx = ca / len, ny = cb / len, nz = cc / len;
            double d = -((nx * x0 + ny * y0) + nz * z0);
            if (plane_flip(nx, ny, nz)) nx = -nx, ny = -ny, nz = -nz, d = -d;
            out = make_float4((float)nx, (float)ny, (float)nz, (float)d);
        }
    }
    a.hyp[g] = out;
}

// the hot loop: every hypothesis of the wave's tile against the wave's chunk.  hyp / counts come as separate restrict
// arguments: the coefficient loads then become wave-uniform scalar loads, issued eight hypotheses ahead of their tests
constexpr int kPlaneAhead = 8;
__global__ __launch_bounds__(kPlaneThreads) void k_plane_score(PlaneArgs a, const float4* __restrict__ hyp, uint32_t* __restrict__ counts)
{
    const uint32_t w = (uint32_t)blockIdx.x * (kPlaneThreads / kWave) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    PlaneChunk c;
    if (!plane_chunk(a, w, c) || c.m < 3u) return;
    float4 p[2];
    bool ok[2];
    plane_load2(a, c, lane, p, ok);
    const f32x2_t X = {p[0].x, p[1].x}, Y = {p[0].y, p[1].y}, Z = {p[0].z, p[1].z};
    const float tf = a.tf;
    const uint32_t H = a.H;
    const float4* hp = hyp + (uint64_t)c.t * H;
    uint32_t* cnt = counts + (uint64_t)c.t * H;
    for (uint32_t h0 = 0; h0 < H; h0 += (uint32_t)kWave) {
        const uint32_t nh = H - h0 < (uint32_t)kWave ? H - h0 : (uint32_t)kWave;
        uint32_t acc = 0;
        for (uint32_t j = 0; j < nh; j += kPlaneAhead) {
            float4 cf[kPlaneAhead];
#pragma unroll
            for (int u = 0; u < kPlaneAhead; ++u) {
                const uint32_t h = h0 + j + (uint32_t)u;
                cf[u] = hp[h < H ? h : H - 1];  // (past the end: a repeat, its count is never added)
            }
#pragma unroll
            for (int u = 0; u < kPlaneAhead; ++u) {
                const f32x2_t d = plane_dist2(cf[u], X, Y, Z);
                const uint32_t k = (uint32_t)__popcll(__ballot(fabsf(d.x) < tf)) + (uint32_t)__popcll(__ballot(fabsf(d.y) < tf));
                acc = lane == (int)(j + (uint32_t)u) ? k : acc;  // lane j keeps hypothesis h0 + j
            }
        }
        if ((uint32_t)lane < nh && acc) atomicAdd(&cnt[h0 + lane], acc);
    }
}
static_assert(kWave % kPlaneAhead == 0, "a 64-hypothesis block is whole groups");

// one wave per tile: the chosen hypothesis (largest count, smallest h; degenerate ones never win) and its sample
__global__ __launch_bounds__(kWave) void k_plane_best(PlaneArgs a)
{
    const uint32_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t t0 = a.tstart[t], m = a.tstart[t + 1] - t0;
    if (m < 3u) return;
    const float4* hp = a.hyp + (uint64_t)t * a.H;
    const uint32_t* cnt = a.counts + (uint64_t)t * a.H;
    uint64_t best = 0;  // (count << 32) | ~h, 0: none
    for (uint32_t h = lane; h < a.H; h += kWave) {
        if (isnan(hp[h].x)) continue;
        const uint64_t k = ((uint64_t)cnt[h] << 32) | (uint64_t)(0xffffffffu - h);
        best = k > best ? k : best;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint64_t x = (uint64_t)__shfl_xor((unsigned long long)best, o, 64);
        best = x > best ? x : best;
    }
    if (lane != 0 || best == 0) return;
    const uint32_t h = 0xffffffffu - (uint32_t)best;
    o3dr_plane_tile& r = a.rec[t];
    uint32_t loc[3];
    draw3(splitmix64(a.seed ^ plane_tile_key(r)), h, m, loc);
    const float4 c = hp[h];
    r.coeff[0] = c.x, r.coeff[1] = c.y, r.coeff[2] = c.z, r.coeff[3] = c.w;
    r.ransac_inliers = (uint32_t)(best >> 32);
    r.hypothesis = (int32_t)h;
#pragma unroll
    for (int k = 0; k < 3; ++k) r.sample[k] = plane_index(a, plane_point(a, t0, loc[k]), t0 + loc[k]);
    r.status = O3DR_PLANE_OK;
}

// ---- refinement -----------------------------------------------------------------------------------
__device__ __forceinline__ double plane_butterfly(double v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ bool plane_refinable(const o3dr_plane_tile& r) { return r.status == O3DR_PLANE_OK && r.ransac_inliers >= 3u; }

// the moments of the chosen plane's inliers over one chunk, about the sample's p0: lane j sums its points j, 64 + j
__global__ __launch_bounds__(kPlaneThreads) void k_plane_moments(PlaneArgs a)
{
    const uint32_t w = (uint32_t)blockIdx.x * (kPlaneThreads / kWave) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    PlaneChunk c;
    if (!plane_chunk(a, w, c)) return;
    const o3dr_plane_tile& r = a.rec[c.t];
    if (!plane_refinable(r)) return;
    const float4 q = reinterpret_cast<const float4*>(a.cloud)[r.sample[0]];
    const float4 pl = make_float4(r.coeff[0], r.coeff[1], r.coeff[2], r.coeff[3]);
    float4 p[2];
    bool ok[2];
    plane_load2(a, c, lane, p, ok);
    const f32x2_t d = plane_dist2(pl, f32x2_t{p[0].x, p[1].x}, f32x2_t{p[0].y, p[1].y}, f32x2_t{p[0].z, p[1].z});
    double m[kPlaneMoments];
#pragma unroll
    for (int f = 0; f < kPlaneMoments; ++f) m[f] = 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!(fabsf(k ? d.y : d.x) < a.tf)) continue;
        const double ex = (double)p[k].x - (double)q.x, ey = (double)p[k].y - (double)q.y, ez = (double)p[k].z - (double)q.z;
        m[0] += 1.0;
        m[1] += ex, m[2] += ey, m[3] += ez;
        m[4] += ex * ex, m[5] += ex * ey, m[6] += ex * ez;
        m[7] += ey * ey, m[8] += ey * ez, m[9] += ez * ez;
    }
    double* out = a.partial + (uint64_t)w * kPlaneMoments;
#pragma unroll
    for (int f = 0; f < kPlaneMoments; ++f) {
        const double v = plane_butterfly(m[f]);
        if (lane == f) out[f] = v;
    }
}

// one wave per tile: the chunk moments folded in a fixed order (lane j: chunks j, j + 64, .. ascending; the butterfly),
// then the plane of the smallest eigenvalue
__global__ __launch_bounds__(kWave) void k_plane_refine(PlaneArgs a)
{
    const uint32_t t = blockIdx.x;
    const int lane = threadIdx.x;
    o3dr_plane_tile& r = a.rec[t];
    if (!plane_refinable(r)) return;
    const uint32_t w0 = a.cfirst[t], w1 = a.cfirst[t + 1];
    double m[kPlaneMoments];
#pragma unroll
    for (int f = 0; f < kPlaneMoments; ++f) m[f] = 0.0;
    for (uint32_t w = w0 + lane; w < w1; w += kWave) {
        const double* pp = a.partial + (uint64_t)w * kPlaneMoments;
#pragma unroll
        for (int f = 0; f < kPlaneMoments; ++f) m[f] += pp[f];
    }
#pragma unroll
    for (int f = 0; f < kPlaneMoments; ++f) m[f] = plane_butterfly(m[f]);
    if (lane != 0) return;
    const float4 q = reinterpret_cast<const float4*>(a.cloud)[r.sample[0]];
    const double inv_k = 1.0 / m[0];
    const double mx = m[1] * inv_k, my = m[2] * inv_k, mz = m[3] * inv_k;  // centroid - p0
    double A[3][3], V[3][3];
    A[0][0] = m[4] * inv_k - mx * mx, A[0][1] = m[5] * inv_k - mx * my, A[0][2] = m[6] * inv_k - mx * mz;
    A[1][1] = m[7] * inv_k - my * my, A[1][2] = m[8] * inv_k - my * mz, A[2][2] = m[9] * inv_k - mz * mz;
    mls_jacobi3(A, V);
    // ascending eigenvalues (ties keep the lower column), as in k_mls
    const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
    int i0 = 0, i1 = 1, i2 = 2;
    auto ev = [&](int i) { return i == 0 ? d0 : (i == 1 ? d1 : d2); };
    if (ev(i1) < ev(i0)) { const int s = i0; i0 = i1; i1 = s; }
    if (ev(i2) < ev(i1)) { const int s = i1; i1 = i2; i2 = s; }
    if (ev(i1) < ev(i0)) { const int s = i0; i0 = i1; i1 = s; }
    const double l1 = ev(i1), l2 = ev(i2);
    if (!(l1 > 1e-12 * l2)) return;  // the hypothesis plane stays
    double nx = i0 == 0 ? V[0][0] : (i0 == 1 ? V[0][1] : V[0][2]);
    double ny = i0 == 0 ? V[1][0] : (i0 == 1 ? V[1][1] : V[1][2]);
    double nz = i0 == 0 ? V[2][0] : (i0 == 1 ? V[2][1] : V[2][2]);
    const double nl = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);
    nx *= nl, ny *= nl, nz *= nl;
    if (plane_flip(nx, ny, nz)) nx = -nx, ny = -ny, nz = -nz;
    const double cx = (double)q.x + mx, cy = (double)q.y + my, cz = (double)q.z + mz;
    const double d = -((nx * cx + ny * cy) + nz * cz);
    r.coeff[0] = (float)nx, r.coeff[1] = (float)ny, r.coeff[2] = (float)nz, r.coeff[3] = (float)d;
    r.refined = 1;
}

// ---- labels -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPlaneThreads) void k_plane_label(PlaneArgs a)
{
    const uint32_t w = (uint32_t)blockIdx.x * (kPlaneThreads / kWave) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    PlaneChunk c;
    if (!plane_chunk(a, w, c)) return;
    o3dr_plane_tile& r = a.rec[c.t];
    const bool fit = r.status == O3DR_PLANE_OK;
    const float4 pl = make_float4(r.coeff[0], r.coeff[1], r.coeff[2], r.coeff[3]);
    float4 p[2];
    bool ok[2];
    plane_load2(a, c, lane, p, ok);
    const f32x2_t d = plane_dist2(pl, f32x2_t{p[0].x, p[1].x}, f32x2_t{p[0].y, p[1].y}, f32x2_t{p[0].z, p[1].z});
    uint32_t n_in = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float dist = k ? d.y : d.x;
        const bool in = ok[k] && fit && fabsf(dist) < a.tf;
        n_in += (uint32_t)__popcll(__ballot(in));
        if (!ok[k]) continue;
        const uint32_t pos = c.b + (uint32_t)(lane + k * kWave);
        const uint32_t idx = plane_index(a, p[k], pos);
        if (a.inlier) a.inlier[idx] = in ? 1u : 0u;
        if (a.tile) a.tile[idx] = (int32_t)c.t;
        if (a.projected) {
            o3dr_point o = a.cloud[idx];
            if (in) o.x = p[k].x - dist * pl.x, o.y = p[k].y - dist * pl.y, o.z = p[k].z - dist * pl.z;
            a.projected[idx] = o;
        }
    }
    if (lane == 0 && n_in) atomicAdd(&r.n_inliers, n_in);
}
static_assert(kPlaneThreads % kWave == 0 && kPlaneMoments <= kWave, "one chunk per wave; one lane per moment");
