// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Image segmentation: grid-seeded k-means superpixels, connected components, merge of the small ones, compact numbering
// (contract: include/o3dr.h "image segmentation"; DESIGN.md "Image segmentation").  Every value is an integer and every
// result is the same whatever the schedule: sums are integer adds, the winner of a pixel and the neighbour of a small
// component are plain integer minima, a component's root is its lowest pixel index (disparity_filter.inc), and the
// numbers come from an ordered scan.  All stores are plain vector stores or atomics.
//   k_seg_init     seeds, sums zeroed                                            one thread per (frame, centre)
//   k_seg_assign   a 64 x 16 tile: its candidate centres staged in LDS, the winner of every pixel; <true>: the tile's
//                  sums per centre reduced in LDS, one global add per (tile, centre, field); <false>: the raw labels
//   k_seg_update   (2 sum + n) / (2 n), sums zeroed                               one thread per (frame, centre)
//   k_df_local / k_df_merge / k_df_flatten <DfLabel>   the components of equal raw labels (disparity_filter.inc)
//   k_seg_key      one thread per pixel, its right and lower neighbour: where a small component meets a not-small one,
//                  a 64-bit atomic min of (colour distance^2 << 32 | the neighbour's root) at the small one's root
//   k_seg_link     per root: itself (not small), the key's root, or the root left of / above its first pixel
//   k_seg_chase    per root: follow the links to the surviving root; sizes and the lowest first pixel gather there
//   k_seg_flag     per surviving root: a flag at its label's first pixel; the frame's counts
//   (launch_scan)  exclusive scan of the flags in pixel order: the numbers
//   k_seg_relabel  labels_out / sizes_out
// =================================================================================================
constexpr int kSegMaxCand = 19 * 7;  // centres a tile can see: ceil(63 / S) + 3 cells across, ceil(15 / S) + 3 down, S >= 4
constexpr unsigned long long kSegNoKey = ~0ull;

struct SegBgr {
    int b, g, r;
};
__device__ __forceinline__ SegBgr seg_load(const SegArgs& a, int f, int y, int x)
{
    const uint8_t* p = a.img + (int64_t)f * a.fstride + (int64_t)y * a.pitch + (int64_t)x * a.channels;
    if (a.channels == 3) return SegBgr{p[0], p[1], p[2]};
    return SegBgr{p[0], p[0], p[0]};
}

__global__ __launch_bounds__(256) void k_seg_init(SegArgs a)
{
    const int f = blockIdx.y, nc = a.nx * a.ny;
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k >= nc) return;
    const int gy = k / a.nx, gx = k - gy * a.nx;
    const int x = min(gx * a.S + a.S / 2, a.cols - 1), y = min(gy * a.S + a.S / 2, a.rows - 1);
    const SegBgr c = seg_load(a, f, y, x);
    int32_t* cen = a.centres + ((int64_t)f * nc + k) * 5;
    cen[0] = x, cen[1] = y, cen[2] = c.b, cen[3] = c.g, cen[4] = c.r;
    unsigned long long* s = a.sums + ((int64_t)f * nc + k) * 6;
#pragma unroll
    for (int j = 0; j < 6; ++j) s[j] = 0;
}

template <bool SUMS>
__global__ __launch_bounds__(256) void k_seg_assign(SegArgs a, int tiles_x)
{
    __shared__ int cen[kSegMaxCand * 5];
    __shared__ unsigned int sum[SUMS ? kSegMaxCand * 6 : 1];
    const int f = blockIdx.y, W = a.cols, H = a.rows, S = a.S, nc = a.nx * a.ny;
    const int x0 = (int)(blockIdx.x % tiles_x) * kDfTileX, y0 = (int)(blockIdx.x / tiles_x) * kDfTileY;
    // the cells whose centres a pixel of this tile can take: the home cells of the tile's pixels and one ring around them
    const int cx0 = max(x0 / S - 1, 0), cx1 = min(min(x0 + kDfTileX - 1, W - 1) / S + 1, a.nx - 1);
    const int cy0 = max(y0 / S - 1, 0), cy1 = min(min(y0 + kDfTileY - 1, H - 1) / S + 1, a.ny - 1);
    const int cnx = cx1 - cx0 + 1, ncand = cnx * (cy1 - cy0 + 1);  // <= kSegMaxCand
    for (int i = threadIdx.x; i < ncand * 5; i += 256) {
        const int c = i / 5, j = i - c * 5;
        const int k = (cy0 + c / cnx) * a.nx + cx0 + c % cnx;
        cen[i] = a.centres[((int64_t)f * nc + k) * 5 + j];
    }
    if (SUMS)
        for (int i = threadIdx.x; i < ncand * 6; i += 256) sum[i] = 0;
    __syncthreads();
    const unsigned long long s2 = (unsigned long long)(S * S), m2 = (unsigned long long)(a.m * a.m);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int x = x0 + (int)(threadIdx.x & 63), y = y0 + (int)(threadIdx.x >> 6) + 4 * r;
        if (x >= W || y >= H) continue;
        const SegBgr v = seg_load(a, f, y, x);
        const int hx = x / S, hy = y / S;
        unsigned long long best = 0;
        int best_c = -1;
        for (int dy = -1; dy <= 1; ++dy) {  // ascending k: the strict < keeps the lowest k of a tie
            const int cy = hy + dy;
            if (cy < 0 || cy >= a.ny) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int cx = hx + dx;
                if (cx < 0 || cx >= a.nx) continue;
                const int c = (cy - cy0) * cnx + cx - cx0;
                const int* q = cen + c * 5;
                const int ex = x - q[0], ey = y - q[1], eb = v.b - q[2], eg = v.g - q[3], er = v.r - q[4];
                const unsigned long long D =
                    s2 * (unsigned long long)(eb * eb + eg * eg + er * er) + m2 * (unsigned long long)(ex * ex + ey * ey);
                if (best_c < 0 || D < best) best = D, best_c = c;
            }
        }
        if (SUMS) {
            unsigned int* s = sum + best_c * 6;  // a tile's sums fit 32 bits: 1024 pixels of at most 8191
            atomicAdd(s + 0, 1u);
            atomicAdd(s + 1, (unsigned int)x);
            atomicAdd(s + 2, (unsigned int)y);
            atomicAdd(s + 3, (unsigned int)v.b);
            atomicAdd(s + 4, (unsigned int)v.g);
            atomicAdd(s + 5, (unsigned int)v.r);
        } else {
            const int64_t i = (int64_t)f * W * H + (int64_t)y * W + x;
            a.raw[i] = (cy0 + best_c / cnx) * a.nx + cx0 + best_c % cnx;
            a.key[i] = kSegNoKey;
        }
    }
    if (SUMS) {
        __syncthreads();
        for (int i = threadIdx.x; i < ncand * 6; i += 256) {
            const unsigned int v = sum[i];
            if (v == 0) continue;
            const int c = i / 6, j = i - c * 6;
            const int k = (cy0 + c / cnx) * a.nx + cx0 + c % cnx;
            atomicAdd(a.sums + ((int64_t)f * nc + k) * 6 + j, (unsigned long long)v);
        }
    }
}

__global__ __launch_bounds__(256) void k_seg_update(SegArgs a)
{
    const int f = blockIdx.y, nc = a.nx * a.ny;
    const int k = (int)(blockIdx.x * 256 + threadIdx.x);
    if (k >= nc) return;
    unsigned long long* s = a.sums + ((int64_t)f * nc + k) * 6;
    int32_t* cen = a.centres + ((int64_t)f * nc + k) * 5;
    const unsigned long long n = s[0];
    s[0] = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const unsigned long long v = s[j + 1];
        s[j + 1] = 0;
        if (n) cen[j] = (int32_t)((2 * v + n) / (2 * n));  // an empty centre keeps its values
    }
}

__device__ __forceinline__ unsigned long long seg_key(const SegArgs& a, int f, int la, int lb, int root_b)
{
    const int nc = a.nx * a.ny;
    const int32_t *p = a.centres + ((int64_t)f * nc + la) * 5, *q = a.centres + ((int64_t)f * nc + lb) * 5;
    const int eb = p[2] - q[2], eg = p[3] - q[3], er = p[4] - q[4];
    return ((unsigned long long)(eb * eb + eg * eg + er * er) << 32) | (unsigned long long)(unsigned int)root_b;
}

// pixel i against its neighbour j: where exactly one of the two components is small, the other one bids at its root
__device__ __forceinline__ void seg_bid(const SegArgs& a, int f, int64_t base, int i, int j)
{
    const int p = a.parent[base + i], q = a.parent[base + j];
    if (p == q) return;
    const bool sp = a.cnt[base + p] < a.min_size, sq = a.cnt[base + q] < a.min_size;
    if (sp == sq) return;
    const int li = a.raw[base + i], lj = a.raw[base + j];
    if (sp)
        atomicMin(a.key + base + p, seg_key(a, f, li, lj, q));
    else
        atomicMin(a.key + base + q, seg_key(a, f, lj, li, p));
}

__global__ __launch_bounds__(256) void k_seg_key(SegArgs a)
{
    const int f = blockIdx.y, W = a.cols, n = a.cols * a.rows;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const int64_t base = (int64_t)f * n;
    if (i % W + 1 < W) seg_bid(a, f, base, i, i + 1);
    if (i + W < n) seg_bid(a, f, base, i, i + W);
}

__global__ __launch_bounds__(256) void k_seg_link(SegArgs a)
{
    const int f = blockIdx.y, W = a.cols, n = a.cols * a.rows;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const int64_t base = (int64_t)f * n;
    a.flag[base + i] = 0;
    if (a.parent[base + i] != i) return;
    const unsigned long long k = a.key[base + i];
    int l = i;
    if (a.cnt[base + i] < a.min_size) {
        if (k != kSegNoKey)
            l = (int)(unsigned int)(k & 0xffffffffull);
        else if (i % W > 0)
            l = a.parent[base + i - 1];  // a component whose first pixel is lower: the chain ends
        else if (i >= W)
            l = a.parent[base + i - W];
    }
    a.link[base + i] = l;
    // the key's word is free from here on: it holds the root's final root and its label's first pixel
    int* ff = (int*)(a.key + base + i);
    ff[0] = i, ff[1] = i;
}

__global__ __launch_bounds__(256) void k_seg_chase(SegArgs a)
{
    const int f = blockIdx.y, n = a.cols * a.rows;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const int64_t base = (int64_t)f * n;
    if (a.parent[base + i] != i) return;
    // Ends: a link leads to a not-small root, whose link is itself, or to a root with a lower first pixel.  `link` is
    // not written in this launch.
    int t = i;
    for (int l = a.link[base + t]; l != t; l = a.link[base + t]) t = l;
    int* ff = (int*)(a.key + base);
    ff[2 * (int64_t)i] = t;
    if (t == i) return;
    // only surviving roots receive, only the others give: cnt[i] is not changing under this read
    atomicAdd(a.cnt + base + t, a.cnt[base + i]);
    atomicMin(ff + 2 * (int64_t)t + 1, i);
}

// info: [frames][5] n_components, n_merged, n_labels, largest, 2^32 - 1 - smallest (all start at 0)
__global__ __launch_bounds__(256) void k_seg_flag(SegArgs a)
{
    __shared__ unsigned int s[5];
    const int f = blockIdx.y, n = a.cols * a.rows;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (threadIdx.x < 5) s[threadIdx.x] = 0;
    __syncthreads();
    const int64_t base = (int64_t)f * n;
    const int* ff = (const int*)(a.key + base);
    const bool root = i < n && a.parent[base + i] == i;
    const bool keeps = root && ff[2 * (int64_t)i] == i;
    unsigned int size = 0;
    if (keeps) {
        a.flag[base + ff[2 * (int64_t)i + 1]] = 1;
        size = (unsigned int)a.cnt[base + i];
    }
    if (a.info) {  // (wave-uniform)
        const unsigned long long br = __ballot(root), bk = __ballot(keeps);
        unsigned int largest = size, inv = keeps ? 0xffffffffu - size : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            largest = max(largest, (unsigned int)__shfl_xor((int)largest, o));
            inv = max(inv, (unsigned int)__shfl_xor((int)inv, o));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&s[0], (unsigned int)__popcll(br));
            atomicAdd(&s[1], (unsigned int)(__popcll(br) - __popcll(bk)));
            atomicAdd(&s[2], (unsigned int)__popcll(bk));
            atomicMax(&s[3], largest);
            atomicMax(&s[4], inv);
        }
        __syncthreads();
        unsigned long long* info = a.info + (int64_t)f * 5;
        if (threadIdx.x < 3 && s[threadIdx.x]) atomicAdd(info + threadIdx.x, (unsigned long long)s[threadIdx.x]);
        if ((threadIdx.x == 3 || threadIdx.x == 4) && s[threadIdx.x]) atomicMax(info + threadIdx.x, (unsigned long long)s[threadIdx.x]);
    }
}

__global__ __launch_bounds__(256) void k_seg_relabel(SegArgs a)
{
    const int f = blockIdx.y, n = a.cols * a.rows;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= n) return;
    const int64_t base = (int64_t)f * n;
    const int* ff = (const int*)(a.key + base);
    const int t = ff[2 * (int64_t)a.parent[base + i]];
    a.labels_out[base + i] = (int32_t)a.flag[base + ff[2 * (int64_t)t + 1]];
    if (a.sizes_out) a.sizes_out[base + i] = a.cnt[base + t];
}
