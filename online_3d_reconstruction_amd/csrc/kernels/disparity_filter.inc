// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Disparity filter: k x k median, connected components of near-equal 4-neighbours, removal of the small ones
// (contract: include/o3dr.h "disparity filter"; DESIGN.md "Disparity filter").  Every value is an integer and every
// result is the same whatever the schedule: the root of a component is its lowest pixel index because a larger root is
// only ever linked under a smaller one, and sizes are integer sums.  All stores are plain vector stores or atomics.
//
// Labelling is a union-find over `parent` (one int32 per pixel, -1: invalid pixel): parent[i] <= i always, a root has
// parent[i] == i.  Four launches, each a later phase of the one before, no waiting between workgroups:
//   k_df_local    a 64 x 16 tile in LDS: joins inside the tile, flatten, pixel count per tile root -> parent / cnt
//   k_df_merge    one thread per pixel pair across a tile border: joins in global memory
//   k_df_flatten  every pixel takes its final root; every tile root adds its count to the final root
//   k_df_sizes    labels_out / sizes_out (only when asked for)
// =================================================================================================
constexpr int kDfTileX = 64, kDfTileY = 16;  // pixels per workgroup of the median and the local labelling (1 x 4 per lane)
constexpr int kDfTile = kDfTileX * kDfTileY;

__device__ __forceinline__ void df_cx(uint32_t& a, uint32_t& b)
{
    const uint32_t lo = min(a, b);
    b = max(a, b);
    a = lo;
}
// min of v[0..N) to v[0], max to v[N - 1]: a fixed network
template <int N>
__device__ __forceinline__ void df_minmax(uint32_t* v)
{
#pragma unroll
    for (int i = 0; i < N / 2; ++i) df_cx(v[i], v[N - 1 - i]);
#pragma unroll
    for (int i = 1; i <= (N - 1) / 2; ++i) df_cx(v[0], v[i]);
#pragma unroll
    for (int i = N / 2; i < N - 1; ++i) df_cx(v[i], v[N - 1]);
}
// Element N / 2 of the ascending sort of v[0..N), N odd, by forgetful selection: of N / 2 + 2 values neither the least nor
// the greatest can be the median, so both are dropped and the next value takes a free place; the set shrinks by one a
// round until one value is left.  A fixed sequence of compare-exchanges: no sort, no data-dependent control flow.
template <int N, int S = N / 2 + 2>
struct DfSelect {
    static __device__ __forceinline__ uint32_t run(uint32_t* v, const uint32_t* next)
    {
        df_minmax<S>(v);
        if constexpr (S == 3) {
            return v[1];
        } else {
            v[0] = v[S - 2];  // the least and the greatest leave: S - 2 stay, one joins
            v[S - 2] = *next;
            return DfSelect<N, S - 1>::run(v, next + 1);
        }
    }
};
template <int K>
__device__ __forceinline__ uint32_t df_median(uint32_t* v)
{
    constexpr int N = K * K;
    return DfSelect<N>::run(v, v + N / 2 + 2);
}

template <class T>
__device__ __forceinline__ uint32_t df_load(const DfView& v, int f, int y, int x)
{
    return *(const T*)((const char*)v.p + (int64_t)f * v.fstride + (int64_t)y * v.pitch + (int64_t)x * (int64_t)sizeof(T));
}
// The equal-label predicate (segment_image.inc): an element type whose value is the int32 label plus one, so that every
// label >= 0 is a valid pixel and df_joined with max_diff = 0 joins equal labels alone.
struct DfLabel {
    int32_t v;
    __device__ __forceinline__ operator uint32_t() const { return (uint32_t)v + 1u; }
};
__device__ __forceinline__ bool df_joined(uint32_t a, uint32_t b, uint32_t max_diff)
{
    return a != 0 && b != 0 && (a > b ? a - b : b - a) <= max_diff;
}

// Median of one tile; the tile and its halo go through LDS, clamped at the image border.
template <class T, int K>
__global__ __launch_bounds__(256) void k_df_median(DfView in, int rows, int cols, int tiles_x, T* out)
{
    constexpr int R = K / 2, TP = kDfTileX + 2 * R, TR = kDfTileY + 2 * R;
    __shared__ T tile[TR * TP];
    const int f = blockIdx.y, W = cols, H = rows;
    const int x0 = (int)(blockIdx.x % tiles_x) * kDfTileX, y0 = (int)(blockIdx.x / tiles_x) * kDfTileY;
    for (int i = threadIdx.x; i < TR * TP; i += 256) {
        const int ty = i / TP, tx = i - ty * TP;
        const int gx = min(max(x0 + tx - R, 0), W - 1), gy = min(max(y0 + ty - R, 0), H - 1);
        tile[i] = (T)df_load<T>(in, f, gy, gx);
    }
    __syncthreads();
    const int px = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int py = (int)(threadIdx.x >> 6) + 4 * k;
        const int x = x0 + px, y = y0 + py;
        if (x >= W || y >= H) continue;
        uint32_t v[K * K];
#pragma unroll
        for (int dy = 0; dy < K; ++dy)
#pragma unroll
            for (int dx = 0; dx < K; ++dx) v[dy * K + dx] = tile[(py + dy) * TP + px + dx];
        out[((int64_t)f * H + y) * W + x] = (T)df_median<K>(v);
    }
}

// (the union-find the labelling runs on - DfLds / DfGlobal, df_find, df_union - is in util.inc: the clustering shares it)

template <class T>
__global__ __launch_bounds__(256) void k_df_local(DfArgs a, int tiles_x)
{
    __shared__ uint32_t val[kDfTile];
    __shared__ int par[kDfTile];
    __shared__ int cnt[kDfTile];
    const int f = blockIdx.y, W = a.cols, H = a.rows;
    const int x0 = (int)(blockIdx.x % tiles_x) * kDfTileX, y0 = (int)(blockIdx.x / tiles_x) * kDfTileY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = (int)threadIdx.x + 256 * k, lx = l & 63, ly = l >> 6;
        const int x = x0 + lx, y = y0 + ly;
        val[l] = (x < W && y < H) ? df_load<T>(a.src, f, y, x) : 0u;  // outside the image: invalid, joins nothing
        par[l] = l;
        cnt[l] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = (int)threadIdx.x + 256 * k, lx = l & 63, ly = l >> 6;
        const uint32_t v = val[l];
        if (lx + 1 < kDfTileX && df_joined(v, val[l + 1], (uint32_t)a.max_diff)) df_union<DfLds>(par, l, l + 1);
        if (ly + 1 < kDfTileY && df_joined(v, val[l + kDfTileX], (uint32_t)a.max_diff)) df_union<DfLds>(par, l, l + kDfTileX);
    }
    __syncthreads();
    int root[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = (int)threadIdx.x + 256 * k;
        root[k] = df_find<DfLds>(par, l);
        if (val[l]) atomicAdd(&cnt[root[k]], 1);
    }
    __syncthreads();
    // the order of the tile's local indices is the order of the pixels' frame indices: the lowest stays the lowest
    int32_t* parent = a.parent + (int64_t)f * W * H;
    int32_t* count = a.cnt + (int64_t)f * W * H;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int l = (int)threadIdx.x + 256 * k, lx = l & 63, ly = l >> 6;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const int r = root[k];
        const bool valid = val[l] != 0;
        parent[y * W + x] = valid ? (y0 + (r >> 6)) * W + x0 + (r & 63) : -1;
        count[y * W + x] = valid && r == l ? cnt[l] : 0;
    }
}

// the pixel pairs across tile borders: n_vert pairs (x, y) | (x + 1, y) with x + 1 a multiple of 64, then the pairs
// (x, y) | (x, y + 1) with y + 1 a multiple of 16
template <class T>
__global__ __launch_bounds__(256) void k_df_merge(DfArgs a, int n_vert, int n_all)
{
    const int f = blockIdx.y, W = a.cols, H = a.rows;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n_all) return;
    int x, y, x2, y2;
    if (i < n_vert) {  // row by row, so that neighbouring lanes stay in one image row and not a pitch apart
        const int nb = n_vert / H;  // borders per row: tiles_x - 1 >= 1 here
        x = (i % nb + 1) * kDfTileX - 1, y = i / nb;
        x2 = x + 1, y2 = y;
    } else {
        const int j = i - n_vert;
        x = j % W, y = (j / W + 1) * kDfTileY - 1;
        x2 = x, y2 = y + 1;
    }
    if (df_joined(df_load<T>(a.src, f, y, x), df_load<T>(a.src, f, y2, x2), (uint32_t)a.max_diff))
        df_union<DfGlobal>(a.parent + (int64_t)f * W * H, y * W + x, y2 * W + x2);
}

__global__ __launch_bounds__(256) void k_df_flatten(DfArgs a)
{
    const int f = blockIdx.y, n = a.cols * a.rows;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    int32_t* parent = a.parent + (int64_t)f * n;
    int32_t* count = a.cnt + (int64_t)f * n;
    if (DfGlobal::load(parent + i) < 0) return;
    // no link is made in this launch: the trees are fixed, and a word another thread has already set to its root is
    // still an ancestor
    const int r = df_find<DfGlobal>(parent, i);
    __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // a tile root that is not the final root hands its count on: one add per (tile, component).  Only final roots
    // receive adds, so count[i] is not changing under this read.
    const int c = count[i];
    if (c > 0 && r != i) atomicAdd(count + r, c);
}

__global__ __launch_bounds__(256) void k_df_sizes(DfArgs a)
{
    const int f = blockIdx.y, n = a.cols * a.rows;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const int r = a.parent[(int64_t)f * n + i];
    if (a.labels_out) a.labels_out[(int64_t)f * n + i] = r;
    if (a.sizes_out) a.sizes_out[(int64_t)f * n + i] = r < 0 ? 0 : a.cnt[(int64_t)f * n + r];
}

// out = src with the pixels of small components zeroed (a.parent == nullptr: the copy alone), and the frame's counts
template <class T>
__global__ __launch_bounds__(256) void k_df_apply(DfArgs a)
{
    __shared__ unsigned int s[5];
    const int f = blockIdx.y, W = a.cols, n = a.cols * a.rows;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (threadIdx.x < 5) s[threadIdx.x] = 0;
    __syncthreads();
    const bool in = i < n;
    uint32_t v = 0;
    int r = -1, size = 0;
    if (in) {
        v = df_load<T>(a.src, f, i / W, i % W);
        if (a.parent) {
            r = a.parent[(int64_t)f * n + i];
            size = r < 0 ? 0 : a.cnt[(int64_t)f * n + r];
        }
    }
    const bool valid = v != 0, is_root = in && r == i;
    const bool small = a.max_size > 0 && valid && size <= a.max_size;
    if (in) ((T*)a.out)[(int64_t)f * n + i] = small ? (T)0 : (T)v;
    if (a.info) {  // (wave-uniform)
        const unsigned long long bv = __ballot(valid), bc = __ballot(is_root), bs = __ballot(is_root && small), br = __ballot(small);
        int largest = is_root ? size : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) largest = max(largest, __shfl_xor(largest, o));
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&s[0], (unsigned int)__popcll(bv));
            atomicAdd(&s[1], (unsigned int)__popcll(bc));
            atomicAdd(&s[2], (unsigned int)__popcll(bs));
            atomicAdd(&s[3], (unsigned int)__popcll(br));
            atomicMax(&s[4], (unsigned int)largest);
        }
        __syncthreads();
        if (threadIdx.x < 4 && s[threadIdx.x]) atomicAdd(a.info + (int64_t)f * 5 + threadIdx.x, (unsigned long long)s[threadIdx.x]);
        if (threadIdx.x == 4 && s[4]) atomicMax(a.info + (int64_t)f * 5 + 4, (unsigned long long)s[4]);
    }
}
