// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// small bookkeeping kernels
// =================================================================================================
// neutral bounding-box slot `slot` of every frame (the keypoint-pass slot when there is no keypoint pass)
__global__ void k_minmax_init(float* mm, int64_t mm_stride, int slot, uint32_t* n_kp, int frames)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < frames * 6) {
        const int f = i / 6, a = i % 6;
        mm[((int64_t)f * mm_stride + slot) * 6 + a] = (a < 3) ? __builtin_inff() : -__builtin_inff();
    }
    if (n_kp && i < frames) n_kp[i] = 0;
}
__global__ void k_set_counts(uint32_t* n_dev, uint32_t value, int frames)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < frames) n_dev[i] = value;
}

// Exclusive scan of `frames` independent rows of length L (row f at data + f*row_stride), in place.
// One 1024-thread workgroup per row; each thread owns a contiguous chunk.  totals[f] (optional)
// receives the row sum plus add[f] (optional).  With `geom` the row is a radix histogram of pass
// `pass`: its live length is bins(f)*n_tiles, or nothing when that frame skips the pass.
__device__ __forceinline__ int64_t scan_row_len(const VoxelGeom* __restrict__ geom, int f, int pass, int n_tiles,
                                                int64_t L)
{
    if (!geom) return L;
    const VoxelGeom g = geom[f];
    if (g.overflow || pass >= (int)g.passes) return 0;
    return (int64_t)geom_bins(g) * n_tiles;
}
// tiles of a frame's histogram row that hold records: the histogram kernels leave the others unwritten (12 k workgroups
// storing 128 lone zeros each, per pass of a whole-cloud sort, cost more than the sort's own work) and the scans read
// them as zero
__device__ __forceinline__ int scan_live_tiles(const VoxelGeom* __restrict__ geom, int f, int n_tiles)
{
    if (!geom) return n_tiles;
    const int64_t live = ((int64_t)geom[f].n + kSortTile - 1) / kSortTile;
    return live < n_tiles ? (int)live : n_tiles;
}
__global__ __launch_bounds__(1024) void k_scan_rows(uint32_t* __restrict__ data, int64_t L_in, int64_t row_stride,
                                                    uint32_t* __restrict__ totals, const uint32_t* __restrict__ add,
                                                    const VoxelGeom* __restrict__ geom, int pass, int n_tiles,
                                                    int chunked)
{
    __shared__ uint32_t lds[1024 / 64 + 1];
    uint32_t* row = data + (int64_t)blockIdx.x * row_stride;
    int64_t L = scan_row_len(geom, blockIdx.x, pass, n_tiles, L_in);
    if (chunked) L = (L + 4095) / 4096;  // scanning the chunk sums of a chunked scan
    if (L == 0 && !totals) return;
    const int64_t chunk = (L + 1023) / 1024;
    const int64_t b = (int64_t)threadIdx.x * chunk;
    const int64_t e = (b + chunk < L) ? b + chunk : L;
    // (histogram rows, not their chunk sums: entry i belongs to tile i % n_tiles)
    const bool tiles = geom != nullptr && !chunked;
    const int live = tiles ? scan_live_tiles(geom, blockIdx.x, n_tiles) : 0;
    uint32_t s = 0;
    {
        int t = tiles ? (int)(b % n_tiles) : 0;
        for (int64_t i = b; i < e; ++i) {
            if (!tiles || t < live) s += row[i];
            if (tiles && ++t == n_tiles) t = 0;
        }
    }
    uint32_t total;
    uint32_t run = block_excl_scan_u32<16>(s, lds, total);
    {
        int t = tiles ? (int)(b % n_tiles) : 0;
        for (int64_t i = b; i < e; ++i) {
            const uint32_t v = (!tiles || t < live) ? row[i] : 0u;
            row[i] = run;
            run += v;
            if (tiles && ++t == n_tiles) t = 0;
        }
    }
    if (totals && threadIdx.x == 0) totals[blockIdx.x] = total + (add ? add[blockIdx.x] : 0u);
}

// Exclusive scan of the frames' TILE-MAJOR histogram rows ([tile][kMaxRadix], see hist_at in radix_sort.inc) in
// digit-major order (all tiles of digit 0, then digit 1, ...), in place: one 1024-thread workgroup per frame stages the
// row in LDS (row stride kMaxRadix + 1 words: conflict-free walks along a digit), so that the global loads and stores
// are whole lines.  Dynamic LDS: n_tiles * (kMaxRadix + 1) words.  all_live: every one of the n_tiles rows was written
// (the candidate-aligned tiles k_reproject_emit counts: records may sit in any of them, however few the frame has).
__global__ __launch_bounds__(1024) void k_scan_hist_tm(uint32_t* __restrict__ hist, const VoxelGeom* __restrict__ geom, int pass,
                                                       int n_tiles, int all_live)
{
    extern __shared__ uint32_t tm_row[];
    __shared__ uint32_t lds[1024 / 64 + 1];
    const int f = blockIdx.x;
    const VoxelGeom g = geom[f];
    if (g.overflow || pass >= (int)g.passes) return;
    const int bins = geom_bins(g);
    uint32_t* row = hist + (int64_t)f * kMaxRadix * n_tiles;
    const int words = n_tiles * kMaxRadix;
    const int live = all_live ? n_tiles : scan_live_tiles(geom, f, n_tiles);
    for (int i = threadIdx.x; i < words; i += 1024)
        tm_row[(i >> kMaxRadixBits) * (kMaxRadix + 1) + (i & (kMaxRadix - 1))] = (i >> kMaxRadixBits) < live ? row[i] : 0u;
    __syncthreads();
    const int L = bins * n_tiles;  // entries in scan order: i = digit * n_tiles + tile
    const int chunk = (L + 1023) / 1024;
    const int b = (int)threadIdx.x * chunk, e = b + chunk < L ? b + chunk : L;
    uint32_t s = 0;
    {
        int d = b / n_tiles, t = b - d * n_tiles;
        for (int i = b; i < e; ++i) {
            s += tm_row[t * (kMaxRadix + 1) + d];
            if (++t == n_tiles) t = 0, ++d;
        }
    }
    uint32_t total;
    uint32_t run = block_excl_scan_u32<16>(s, lds, total);
    {
        int d = b / n_tiles, t = b - d * n_tiles;
        for (int i = b; i < e; ++i) {
            const uint32_t v = tm_row[t * (kMaxRadix + 1) + d];
            tm_row[t * (kMaxRadix + 1) + d] = run;
            run += v;
            if (++t == n_tiles) t = 0, ++d;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < words; i += 1024)
        if ((i & (kMaxRadix - 1)) < bins) row[i] = tm_row[(i >> kMaxRadixBits) * (kMaxRadix + 1) + (i & (kMaxRadix - 1))];
}

// Multi-workgroup form for long rows (radix histograms, big merges): chunk sums -> k_scan_rows over
// the chunk sums -> per-chunk scan with the chunk's base.  A chunk is 4096 words, 16 per lane.
constexpr int kScanChunk = 4096;
__global__ __launch_bounds__(256) void k_scan_chunk_sums(const uint32_t* __restrict__ data, int64_t L_in,
                                                         int64_t row_stride, int n_chunks,
                                                         uint32_t* __restrict__ partial,
                                                         const VoxelGeom* __restrict__ geom, int pass, int n_tiles)
{
    __shared__ uint32_t lds[4];
    const int64_t L = scan_row_len(geom, blockIdx.y, pass, n_tiles, L_in);
    if ((int64_t)blockIdx.x * kScanChunk >= L) return;
    const uint32_t* row = data + (int64_t)blockIdx.y * row_stride;
    const int64_t b = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * 16;
    const int live = scan_live_tiles(geom, blockIdx.y, n_tiles);
    int t = geom ? (int)(b % n_tiles) : 0;
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (b + k < L && (!geom || t < live)) s += row[b + k];
        if (geom && ++t == n_tiles) t = 0;
    }
    s = wave_sum_u32(s);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.y * n_chunks + blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}
__global__ __launch_bounds__(256) void k_scan_chunk_apply(uint32_t* __restrict__ data, int64_t L_in, int64_t row_stride,
                                                          int n_chunks, const uint32_t* __restrict__ partial_scanned,
                                                          const VoxelGeom* __restrict__ geom, int pass, int n_tiles)
{
    __shared__ uint32_t lds[5];
    const int64_t L = scan_row_len(geom, blockIdx.y, pass, n_tiles, L_in);
    if ((int64_t)blockIdx.x * kScanChunk >= L) return;
    uint32_t* row = data + (int64_t)blockIdx.y * row_stride;
    const int64_t b = (int64_t)blockIdx.x * kScanChunk + (int64_t)threadIdx.x * 16;
    const int live = scan_live_tiles(geom, blockIdx.y, n_tiles);
    int t = geom ? (int)(b % n_tiles) : 0;
    uint32_t v[16];
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        v[k] = (b + k < L && (!geom || t < live)) ? row[b + k] : 0u;
        s += v[k];
        if (geom && ++t == n_tiles) t = 0;
    }
    uint32_t total;
    uint32_t run = block_excl_scan_u32<4>(s, lds, total) + partial_scanned[(int64_t)blockIdx.y * n_chunks + blockIdx.x];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (b + k < L) row[b + k] = run;
        run += v[k];
    }
}

// fp32 min/max of arbitrary clouds (stand-alone voxel grid calls; the fused path gets its
// bounding box from k_reproject_emit).  The `z += 500` of the combined mode (pose_functions.cpp:1666)
// is applied to the box afterwards by k_voxel_geom: fp32 addition is monotonic.
__global__ __launch_bounds__(kPtThreads) void k_points_minmax(const o3dr_point* __restrict__ in, int64_t in_fstride,
                                                              const uint32_t* __restrict__ n_dev, int64_t mm_stride,
                                                              float* __restrict__ mm)
{
    __shared__ float mm_lds[6 * (kPtThreads / 64)];
    const int f = blockIdx.y;
    const int64_t n = n_dev[f];
    const uint4* src = reinterpret_cast<const uint4*>(in + (int64_t)f * in_fstride);
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    bool any = false;
    const int64_t stride = (int64_t)gridDim.x * (kPtThreads * 4);
    for (int64_t base = (int64_t)blockIdx.x * (kPtThreads * 4); base < n; base += stride) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int64_t i = base + k * kPtThreads + threadIdx.x;
            if (i < n) {
                const uint4 v = src[i];
                const float x = __uint_as_float(v.x), y = __uint_as_float(v.y), z = __uint_as_float(v.z);
                lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
                lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
                lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
                any = true;
            }
        }
    }
    block_minmax_store<kPtThreads / 64>(lo, hi, any, mm_lds, mm + ((int64_t)f * mm_stride + blockIdx.x) * 6);
}
