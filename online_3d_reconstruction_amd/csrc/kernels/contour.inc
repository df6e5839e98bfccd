// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Contour lines of a float32 raster (o3dr_raster_contours, o3dr_raster_contours_count; contract: include/o3dr_contour.h,
// DESIGN.md "Contour lines").  K(z), the one place where the levels meet floating point, is taken once per
// cell; from there on a quad's levels, its segment count, its marching-squares case per level and the index of any of its
// segments are integer functions of its four K, so that a neighbour's segment index is recomputed, not looked up.  The
// vertices are the only fp64 work, from the two values of an edge.  No thread waits for another; every counter is an
// integer sum, min or max.
//   k_contour_levels   one lane per cell: K(z), the infinity and range flags
//   k_contour_count    one lane per quad: its segment count, the result's first counters, the 64-bit sum
//   (launch_scan)      counts -> offsets
//   k_contour_emit     one lane per quad over its levels: the segments' vertices, k and next
//   k_contour_link     one lane per segment: prev[next[i]] = i, union(i, next[i]) (df_union<DfGlobal>, util.inc: the root is
//                      the lowest index)
//   k_contour_flatten  parent[i] = the root; the segments per root, equal roots of a wave folded first; the open lines' heads
//   k_contour_flags    roots -> num / beg (scanned next), closed lines get their root as head, the first jump table
//   k_contour_jump     one round of pointer jumping over prev, double-buffered: after contour_rank_rounds rounds the steps
//                      taken are the rank
//   k_contour_outputs  one lane per segment: its record, its vertex, and at a root the line's record
// =================================================================================================
static_assert(kContourThreads == kFoldThreads, "block_reduce4_u32 folds kFoldThreads threads");
static_assert(sizeof(o3dr_contour_segment) == 48 && sizeof(o3dr_contour_line) == 32 && sizeof(ContourVertex) == 16,
              "the record layout of include/o3dr_contour.h");

// the contract's step 1
__device__ __forceinline__ double contour_level(const ContourArgs& a, int k) { return a.base + (double)k * a.interval; }

// K(z) for a finite z; ok = false where it lies outside +-2^30 (the value is then not used)
__device__ __forceinline__ int contour_K(const ContourArgs& a, float z, bool& ok)
{
    constexpr int M = kContourMaxLevel + 1;
    const double zd = (double)z;
    const double q = floor((zd - a.base) / a.interval);
    ok = false;
    if (!(fabs(q) <= 2147483000.0)) return 0;  // (also an overflowed quotient)
    int k = (int)q;
    // the quotient is K but for the roundings of the product, the sum and the division: the predicate decides
    while (k > -M && !(zd >= contour_level(a, k))) --k;
    while (k < M && zd >= contour_level(a, k + 1)) ++k;
    ok = k >= -kContourMaxLevel && k <= kContourMaxLevel;
    return k;
}

__global__ __launch_bounds__(kContourThreads) void k_contour_levels(ContourArgs a)
{
    const int64_t cells = (int64_t)a.W * a.H;
    for (int64_t i = (int64_t)blockIdx.x * kContourThreads + threadIdx.x; i < cells; i += (int64_t)gridDim.x * kContourThreads) {
        const float z = a.raster[i];
        int k = kContourHole;
        if (z == z) {
            k = 0;
            if (z == __builtin_inff() || z == -__builtin_inff()) {
                a.flags[0] = 1u;  // (every writer stores the same value)
            } else {
                bool ok;
                k = contour_K(a, z, ok);
                if (!ok) a.flags[1] = 1u, k = 0;
            }
        }
        a.kc[i] = k;
    }
}

// The four K of quad (r, c) in the order b0 b1 b2 b3; false with a NaN corner.
__device__ __forceinline__ bool contour_quad_K(const ContourArgs& a, int r, int c, int K[4])
{
    const int32_t* p = a.kc + (int64_t)r * a.W + c;
    K[0] = p[0], K[1] = p[1], K[2] = p[a.W + 1], K[3] = p[a.W];
    return K[0] != kContourHole && K[1] != kContourHole && K[2] != kContourHole && K[3] != kContourHole;
}
__device__ __forceinline__ int i32_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int i32_max(int a, int b) { return a > b ? a : b; }
// A quad's levels are kmin + 1 .. kmax.  Level k is a saddle with b0, b2 inside iff max(K1, K3) < k <= min(K0, K2), with b1,
// b3 inside iff max(K0, K2) < k <= min(K1, K3): at most one of the two ranges is not empty.
struct ContourQuad {
    int kmin, kmax, lo, hi;  // the saddle levels are lo + 1 .. hi (hi <= lo: none)
};
__device__ __forceinline__ ContourQuad contour_quad(const int K[4])
{
    ContourQuad q;
    q.kmin = i32_min(i32_min(K[0], K[1]), i32_min(K[2], K[3]));
    q.kmax = i32_max(i32_max(K[0], K[1]), i32_max(K[2], K[3]));
    const int a02 = i32_min(K[0], K[2]), b02 = i32_max(K[0], K[2]), a13 = i32_min(K[1], K[3]), b13 = i32_max(K[1], K[3]);
    if (a02 > b13)
        q.lo = b13, q.hi = a02;
    else
        q.lo = b02, q.hi = a13;
    if (q.hi < q.lo) q.hi = q.lo;
    return q;
}
// the segments a quad emits at the levels below k (kmin < k <= kmax + 1): one per level and one more per saddle level
__device__ __forceinline__ int64_t contour_below(const ContourQuad& q, int k)
{
    const int top = i32_min(q.hi, k - 1);
    return ((int64_t)(k - 1) - q.kmin) + (top > q.lo ? (int64_t)top - q.lo : 0);
}

// part: kPartWords words per workgroup: quads without a NaN corner, quads that emit, the least / the greatest level
// emitted as order-preserving words (none: all ones / zero)
__global__ __launch_bounds__(kContourThreads) void k_contour_count(ContourArgs a)
{
    __shared__ unsigned long long wave_total[kContourThreads / kWave];
    const uint32_t qw = (uint32_t)(a.W - 1);
    uint32_t v[4] = {0u, 0u, 0xffffffffu, 0u};
    unsigned long long mine = 0;
    for (int64_t t = (int64_t)blockIdx.x * kContourThreads + threadIdx.x; t < (int64_t)a.n_quads; t += (int64_t)gridDim.x * kContourThreads) {
        const uint32_t r = (uint32_t)t / qw, c = (uint32_t)t - r * qw;
        int K[4];
        unsigned long long n = 0;
        if (contour_quad_K(a, (int)r, (int)c, K)) {
            const ContourQuad q = contour_quad(K);
            n = (unsigned long long)contour_below(q, q.kmax + 1);
            ++v[0];
            if (n) {
                ++v[1];
                v[2] = u32_min(v[2], (uint32_t)(q.kmin + 1) ^ 0x80000000u);
                v[3] = u32_max(v[3], (uint32_t)q.kmax ^ 0x80000000u);
            }
        }
        a.off[t] = n < 0xffffffffull ? (uint32_t)n : 0xffffffffu;  // (such a sum is refused before the offsets are used)
        mine += n;
    }
    // the lanes' sums (each < 2^48) added per workgroup in 64 bits from 16-bit pieces, one integer atomic per workgroup
    unsigned long long s = 0;
#pragma unroll
    for (int piece = 0; piece < 3; ++piece)
        s += (unsigned long long)wave_sum_u32((uint32_t)(mine >> (16 * piece)) & 0xffffu) << (16 * piece);
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot = 0;
#pragma unroll
        for (int w = 0; w < kContourThreads / kWave; ++w) tot += wave_total[w];
        if (tot) atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + 12), tot);
    }
    const int op[4] = {2, 2, 0, 1};
    block_reduce4_u32(v, op, a.part + (int64_t)blockIdx.x * kPartWords);
}

// the contract's step 4 on h(r, c) (horizontal) or v(r, c): A = the value at (r, c), B at the cell after it
__device__ __forceinline__ void contour_vertex(const ContourArgs& a, bool horizontal, int r, int c, float zA, float zB, double level, double& x,
                                               double& y)
{
    const double t = (level - (double)zA) / ((double)zB - (double)zA);
    const double u = (double)((int64_t)a.cx0 + c) + 0.5, w = (double)((int64_t)a.cy0 + r) + 0.5;
    x = (horizontal ? u + t : u) * a.cell_size;
    y = (horizontal ? w : w + t) * a.cell_size;
}
// the crossing of `level` on edge e (0 B, 1 R, 2 T, 3 L) of quad (r, c) with the corner values z[4]
__device__ __forceinline__ void contour_edge_vertex(const ContourArgs& a, int e, int r, int c, const float z[4], double level, double& x, double& y)
{
    switch (e) {
    case 0: contour_vertex(a, true, r, c, z[0], z[1], level, x, y); break;
    case 1: contour_vertex(a, false, r, c + 1, z[1], z[2], level, x, y); break;
    case 2: contour_vertex(a, true, r + 1, c, z[3], z[2], level, x, y); break;
    default: contour_vertex(a, false, r, c, z[0], z[3], level, x, y); break;
    }
}

// The segment across end edge e of quad (r, c) at level k: in the neighbour the edge is (e + 2) & 3 and a start.  Its index
// is the neighbour's offset, plus what the neighbour emits below k, plus its place within a saddle level.
__device__ __forceinline__ int contour_next(const ContourArgs& a, int e, int r, int c, int k)
{
    const int nr = r + (e == 2) - (e == 0), nc = c + (e == 1) - (e == 3);
    if (nr < 0 || nc < 0 || nr >= a.H - 1 || nc >= a.W - 1) return -1;
    int K[4];
    if (!contour_quad_K(a, nr, nc, K)) return -1;
    const ContourQuad q = contour_quad(K);
    const bool saddle = k > q.lo && k <= q.hi;
    const int64_t i = (int64_t)a.off[(int64_t)nr * (a.W - 1) + nc] + contour_below(q, k) + (saddle ? ((e + 2) & 3) >> 1 : 0);
    return (int)i;
}

__global__ __launch_bounds__(kContourThreads) void k_contour_emit(ContourArgs a)
{
    const uint32_t qw = (uint32_t)(a.W - 1);
    for (int64_t t = (int64_t)blockIdx.x * kContourThreads + threadIdx.x; t < (int64_t)a.n_quads; t += (int64_t)gridDim.x * kContourThreads) {
        const int r = (int)((uint32_t)t / qw), c = (int)((uint32_t)t - (uint32_t)r * qw);
        int K[4];
        if (!contour_quad_K(a, r, c, K)) continue;
        const ContourQuad q = contour_quad(K);
        if (q.kmax == q.kmin) continue;
        const float* p = a.raster + (int64_t)r * a.W + c;
        const float z[4] = {p[0], p[1], p[a.W + 1], p[a.W]};
        int64_t o = a.off[t];
        for (int k = q.kmin + 1; k <= q.kmax; ++k) {
            const double level = contour_level(a, k);
            const bool in[4] = {K[0] >= k, K[1] >= k, K[2] >= k, K[3] >= k};
            const bool saddle = k > q.lo && k <= q.hi;
            bool centre_in = false;
            int end = 0;
            if (saddle) {
                centre_in = ((((double)z[0] + (double)z[1]) + (double)z[3]) + (double)z[2]) * 0.25 >= level;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (!in[e] && in[(e + 1) & 3]) end = e;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (!(in[s] && !in[(s + 1) & 3])) continue;  // not a start
                const int e = saddle ? (centre_in ? (s + 1) & 3 : (s + 3) & 3) : end;
                double4 xy;
                contour_edge_vertex(a, s, r, c, z, level, xy.x, xy.y);
                contour_edge_vertex(a, e, r, c, z, level, xy.z, xy.w);
                a.xy[o] = xy;
                a.kn[o] = make_int2(k, contour_next(a, e, r, c, k));
                ++o;
            }
        }
    }
}

__global__ __launch_bounds__(kContourThreads) void k_contour_link(ContourArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kContourThreads + threadIdx.x;
    if (i >= (int64_t)a.n_seg) return;
    const int n = a.kn[i].y;
    if (n < 0) return;
    a.prev[n] = (int)i;  // (next is one-to-one: nobody else writes this word)
    df_union<DfGlobal>(a.parent, (int)i, n);
}

// cnt zeroed, head all ones
__global__ __launch_bounds__(kContourThreads) void k_contour_flatten(ContourArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kContourThreads + threadIdx.x;
    const bool valid = i < (int64_t)a.n_seg;
    int root = 0;
    if (valid) {
        root = df_find_halve<DfGlobal>(a.parent, (int)i);
        if (root != (int)i) DfGlobal::lower(a.parent + i, root);  // an ancestor: the word is only lowered
        if (a.prev[i] < 0) a.head[root] = (int)i;                 // (an open line has one such segment)
    }
    const int lane = threadIdx.x & 63;
    cluster_for_each_key(valid, (uint32_t)root, [&](uint32_t k, unsigned long long same, int leader) {
        if (lane == leader) atomicAdd(a.cnt + k, (uint32_t)__popcll(same));
    });
}

// part: kPartWords words per workgroup: closed lines, the longest line's segments, -, -
__global__ __launch_bounds__(kContourThreads) void k_contour_flags(ContourArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kContourThreads + threadIdx.x;
    uint32_t v[4] = {0u, 0u, 0u, 0u};
    if (i < (int64_t)a.n_seg) {
        const bool is_root = a.parent[i] == (int)i;
        const uint32_t n = is_root ? a.cnt[i] : 0u;
        const bool closed = is_root && a.head[i] < 0;  // no segment of the line is without a predecessor
        if (closed) a.head[i] = (int)i;
        a.num[i] = is_root ? 1u : 0u;
        a.beg[i] = is_root ? n + 1u : 0u;
        const int p = closed ? -1 : a.prev[i];  // the predecessor of a closed line's head is cut
        a.jump[0][i] = make_int2(p, p >= 0 ? 1 : 0);
        v[0] = closed, v[1] = n;
    }
    const int op[4] = {2, 1, 2, 2};
    block_reduce4_u32(v, op, a.part + (int64_t)blockIdx.x * kPartWords);
}

__global__ __launch_bounds__(kContourThreads) void k_contour_jump(const int2* __restrict__ in, int2* __restrict__ out, uint32_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kContourThreads + threadIdx.x;
    if (i >= (int64_t)n) return;
    int2 j = in[i];
    if (j.x >= 0) {
        const int2 b = in[j.x];
        j.x = b.x, j.y += b.y;
    }
    out[i] = j;
}

// rank: the jump table after the last round
__global__ __launch_bounds__(kContourThreads) void k_contour_outputs(ContourArgs a, const int2* __restrict__ rank)
{
    const int64_t i = (int64_t)blockIdx.x * kContourThreads + threadIdx.x;
    if (i >= (int64_t)a.n_seg) return;
    const int root = a.parent[i];
    const int32_t line = (int32_t)a.num[root], rk = rank[i].y;
    const uint32_t n = a.cnt[root];
    const int64_t begin = a.beg[root];
    const double4 xy = a.xy[i];
    const int2 kn = a.kn[i];
    if (a.seg_out) {
        o3dr_contour_segment* s = a.seg_out + i;
        s->x0 = xy.x, s->y0 = xy.y, s->x1 = xy.z, s->y1 = xy.w;
        s->k = kn.x, s->line = line, s->rank = rk, s->next = kn.y;
    }
    if (a.vertices) {
        a.vertices[begin + rk] = ContourVertex{xy.x, xy.y};
        if ((uint32_t)rk + 1u == n) a.vertices[begin + n] = ContourVertex{xy.z, xy.w};
    }
    if (a.lines_out && root == (int)i) {
        o3dr_contour_line* l = a.lines_out + line;
        const int head = a.head[i];
        l->head = head, l->n_segments = (int32_t)n, l->k = kn.x, l->closed = a.prev[head] >= 0 ? 1 : 0;
        l->begin = begin, l->level = contour_level(a, kn.x);
    }
}
