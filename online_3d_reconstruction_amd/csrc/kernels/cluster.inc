// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Euclidean clustering (contract: include/o3dr_objects.h; DESIGN.md "Euclidean clustering").  The cloud's search grid is
// the nearest-neighbour grid (launch_nn_grid), the links come from MLS's exact radius walk (grid_radius_walk, util.inc) and the
// components from the disparity filter's lock-free union-find (df_find_halve / df_union<DfGlobal>, util.inc) over `parent`, one
// int32 per point indexed by ORIGINAL index: parent[i] <= i always, a larger root only ever goes under a smaller one, so
// a component's final root is its lowest index whatever the order of the links.  No thread waits for another, no
// workgroup depends on another; every counter and every record field is an integer sum, an integer min / max or a copy.
//   k_cluster_link     one lane per point in cell order: joins the point with every linked point of a lower index, counts
//                      the pairs
//   k_cluster_flatten  parent[i] = the final root; the size of every root, equal roots of a wave folded first
//   k_cluster_flags    one lane per index: roots that are clusters -> num / beg (scanned next), the result's counters
//   k_cluster_points   one lane per index: label / raw / size, and the roots' record fields first / size / begin
//   k_cluster_boxes    cell order: lo / hi per cluster by integer min / max on the order-preserving words
//   k_cluster_sums     cell order: the quantised offsets from lo added into the int64 sums
//   k_cluster_records  one lane per cluster: lo, hi, centroid
//   k_cluster_keys     the sort key of every point (its cluster's number, K for a rejected point) for `indices`
// =================================================================================================
constexpr int kClusterThreads = 256;
constexpr int kClusterWaves = kClusterThreads / kWave;

__global__ __launch_bounds__(kClusterThreads) void k_cluster_init(int* __restrict__ parent, uint32_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
    if (i < (int64_t)n) parent[i] = (int)i;
}

__global__ __launch_bounds__(kClusterThreads) void k_cluster_link(ClusterArgs a)
{
    __shared__ unsigned long long wave_pairs[kClusterWaves];
    const int64_t t = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
    uint32_t pairs = 0;
    if (t < (int64_t)a.n) {
        const SorGeom g = *a.grid.geom;
        const float4 q = a.grid.xyz[t];
        const int idx = (int)__float_as_uint(q.w);
        // The lane's current root stays in a register: in a dense cloud most neighbours are in the lane's tree already,
        // and one find of the neighbour tells.  A stale root only costs a union that finds nothing to do.
        int root = df_find_halve<DfGlobal>(a.parent, idx);
        grid_radius_walk(a.grid, g, q, a.pad_r, a.r2, [&](const float4& p, float) {
            const int j = (int)__float_as_uint(p.w);
            if (j >= idx) return;  // every pair once, from its higher index (the point itself and later duplicates: not here)
            ++pairs;
            const int rj = df_find_halve<DfGlobal>(a.parent, j);
            if (rj == root) return;
            df_union<DfGlobal>(a.parent, root, rj);
            root = df_find_halve<DfGlobal>(a.parent, rj < root ? rj : root);
        });
    }
    // n_pairs: the lanes' counts (each < 2^31) summed per workgroup in 64 bits, one integer atomic per workgroup
    const uint32_t lo16 = wave_sum_u32(pairs & 0xffffu), hi16 = wave_sum_u32(pairs >> 16);
    if ((threadIdx.x & 63) == 0) wave_pairs[threadIdx.x >> 6] = ((unsigned long long)hi16 << 16) + lo16;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kClusterWaves; ++w) s += wave_pairs[w];
        if (s) atomicAdd(a.n_pairs, s);
    }
}

// For every distinct key among the wave's active lanes, once: f(key, mask of the lanes that hold it, leader), with the same
// wave-uniform arguments in every lane.  In cell order a wave mostly holds one or two roots: one atomic
// per distinct key and wave instead of one per lane.
template <class F>
__device__ __forceinline__ void cluster_for_each_key(bool active, uint32_t key, F&& f)
{
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t k = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);
        const unsigned long long same = __ballot(active && key == k) & todo;
        f(k, same, leader);
        todo &= ~same;
    }
}

__global__ __launch_bounds__(kClusterThreads) void k_cluster_flatten(ClusterArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
    const bool valid = t < (int64_t)a.n;
    int root = 0;
    if (valid) {
        const int idx = (int)__float_as_uint(a.grid.xyz[t].w);
        root = df_find_halve<DfGlobal>(a.parent, idx);
        if (root != idx) DfGlobal::lower(a.parent + idx, root);  // an ancestor: the word is only lowered
    }
    const int lane = threadIdx.x & 63;
    cluster_for_each_key(valid, (uint32_t)root, [&](uint32_t k, unsigned long long same, int leader) {
        if (lane == leader) atomicAdd(a.cnt + k, (uint32_t)__popcll(same));
    });
}

// part: kPartWords words per workgroup: components, too small, too large, the largest size | clusters' points, -, -, -
__global__ __launch_bounds__(kClusterThreads) void k_cluster_flags(ClusterArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
    uint32_t v[4] = {0u, 0u, 0u, 0u}, w[4] = {0u, 0u, 0u, 0u};
    if (i < (int64_t)a.n) {
        const bool is_root = a.parent[i] == (int)i;
        const uint32_t s = is_root ? a.cnt[i] : 0u;
        const bool small = is_root && s < (uint32_t)a.min_size, large = is_root && s > (uint32_t)a.max_size;
        const bool kept = is_root && !small && !large;
        a.num[i] = kept ? 1u : 0u;
        a.beg[i] = kept ? s : 0u;
        v[0] = is_root, v[1] = small, v[2] = large, v[3] = s;
        w[0] = kept ? s : 0u;
    }
    const int op_v[4] = {2, 2, 2, 1}, op_w[4] = {2, 2, 2, 2};
    uint32_t* part = a.part + (int64_t)blockIdx.x * kPartWords;
    block_reduce4_u32(v, op_v, part);
    block_reduce4_u32(w, op_w, part + 4);
}
static_assert(kClusterThreads == kFoldThreads, "block_reduce4_u32 folds kFoldThreads threads");

// after the scans: num[r] = the number and beg[r] = the begin of a root r that is a cluster
__device__ __forceinline__ bool cluster_kept(const ClusterArgs& a, uint32_t size) { return size >= (uint32_t)a.min_size && size <= (uint32_t)a.max_size; }

__global__ __launch_bounds__(kClusterThreads) void k_cluster_points(ClusterArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
    if (i >= (int64_t)a.n) return;
    const int root = a.parent[i];
    const uint32_t s = a.cnt[root];
    const bool kept = cluster_kept(a, s);
    const int32_t number = kept ? (int32_t)a.num[root] : -1;
    if (a.label) a.label[i] = number;
    if (a.raw) a.raw[i] = root;
    if (a.size) a.size[i] = (int32_t)s;
    if (a.rec && kept && root == (int)i) {
        o3dr_cluster* r = a.rec + number;
        r->first = root, r->size = (int32_t)s, r->begin = (int32_t)a.beg[i], r->reserved = 0;
    }
}

// the cluster number of the point in lane t of the cell order, or no number
__device__ __forceinline__ bool cluster_number_of(const ClusterArgs& a, const float4& p, uint32_t& number)
{
    const int root = a.parent[__float_as_uint(p.w)];
    number = a.num[root];
    return cluster_kept(a, a.cnt[root]);
}

// box_lo / box_hi: 3 order-preserving words per cluster each, initialised to all ones / to zero
__global__ __launch_bounds__(kClusterThreads) void k_cluster_boxes(ClusterArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t number = 0;
    bool kept = false;
    if (t < (int64_t)a.n) {
        p = a.grid.xyz[t];
        kept = cluster_number_of(a, p, number);
    }
    const uint32_t c[3] = {f32_ordered(p.x + 0.0f), f32_ordered(p.y + 0.0f), f32_ordered(p.z + 0.0f)};
    const int lane = threadIdx.x & 63;
    cluster_for_each_key(kept, number, [&](uint32_t k, unsigned long long same, int leader) {
        const bool mine = (same >> lane) & 1ull;
        uint32_t lo[3], hi[3];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            lo[x] = wave_min_u32(mine ? c[x] : 0xffffffffu);
            hi[x] = wave_max_u32(mine ? c[x] : 0u);
        }
        if (lane == leader) {
#pragma unroll
            for (int x = 0; x < 3; ++x) {
                atomicMin(a.box_lo + (int64_t)k * 3 + x, lo[x]);
                atomicMax(a.box_hi + (int64_t)k * 3 + x, hi[x]);
            }
        }
    });
}

// sums: 3 int64 per cluster, zeroed.  q < 2^31 + 1 per point: its two 16-bit halves sum over a wave within 32 bits.
__global__ __launch_bounds__(kClusterThreads) void k_cluster_sums(ClusterArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    uint32_t number = 0;
    bool kept = false;
    if (t < (int64_t)a.n) {
        p = a.grid.xyz[t];
        kept = cluster_number_of(a, p, number);
    }
    unsigned long long q[3] = {0ull, 0ull, 0ull};
    if (kept) {
        const uint32_t* b = a.box_lo + (int64_t)number * 3;
        const float c[3] = {p.x, p.y, p.z};
#pragma unroll
        for (int x = 0; x < 3; ++x) q[x] = (unsigned long long)(long long)floor(((double)c[x] - (double)ordered_f32(b[x])) * 65536.0 + 0.5);
    }
    const int lane = threadIdx.x & 63;
    cluster_for_each_key(kept, number, [&](uint32_t k, unsigned long long same, int leader) {
        const bool mine = (same >> lane) & 1ull;
        unsigned long long s[3];
#pragma unroll
        for (int x = 0; x < 3; ++x) {
            const uint32_t l = wave_sum_u32(mine ? (uint32_t)(q[x] & 0xffffu) : 0u);
            const uint32_t h = wave_sum_u32(mine ? (uint32_t)(q[x] >> 16) : 0u);
            s[x] = ((unsigned long long)h << 16) + l;
        }
        if (lane == leader) {
#pragma unroll
            for (int x = 0; x < 3; ++x) atomicAdd(a.sums + (int64_t)k * 3 + x, s[x]);
        }
    });
}

__global__ __launch_bounds__(kClusterThreads) void k_cluster_records(ClusterArgs a, uint32_t n_clusters)
{
    const int64_t k = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
    if (k >= (int64_t)n_clusters) return;
    o3dr_cluster* r = a.rec + k;
    const double size = (double)r->size;
#pragma unroll
    for (int x = 0; x < 3; ++x) {
        const float lo = ordered_f32(a.box_lo[k * 3 + x]);
        r->lo[x] = lo;
        r->hi[x] = ordered_f32(a.box_hi[k * 3 + x]);
        r->centroid[x] = (double)lo + ((double)(long long)a.sums[k * 3 + x] / 65536.0) / size;
    }
}

// `indices`: the key of point i is its cluster's number, n_clusters (after every cluster) for a rejected point
__global__ __launch_bounds__(kClusterThreads) void k_cluster_keys(ClusterArgs a, uint32_t n_clusters, uint32_t* __restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
    if (i >= (int64_t)a.n) return;
    const int root = a.parent[i];
    keys[i] = cluster_kept(a, a.cnt[root]) ? a.num[root] : n_clusters;
}
__global__ __launch_bounds__(kClusterThreads) void k_cluster_indices(const uint32_t* __restrict__ sorted, uint32_t n_clustered,
                                                                     int32_t* __restrict__ indices)
{
    const int64_t i = (int64_t)blockIdx.x * kClusterThreads + threadIdx.x;
    if (i < (int64_t)n_clustered) indices[i] = (int32_t)sorted[i];
}
static_assert(kClusterThreads % kWave == 0, "equal keys are folded per wave");
static_assert(sizeof(o3dr_cluster) == 64 && sizeof(o3dr_cluster_result) == 64, "the record layout of include/o3dr_objects.h");
