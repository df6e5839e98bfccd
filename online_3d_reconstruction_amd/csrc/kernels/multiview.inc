// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Multi-view filter: every valid pixel of a frame is carried into each listed neighbour frame by one 4 x 4 fp64 matrix
// and compared with what that frame saw there (contract: include/o3dr.h "multi-view filter"; DESIGN.md "Multi-view
// filter"); the fusion ("multi-view fusion") runs the same tests and averages what the agreeing frames saw.  One launch,
// one thread per pixel, a 32 x 8 tile per workgroup, the frame in blockIdx.y: the neighbour list and the matrices of a
// workgroup are the same for every lane, so the compiler fetches them with scalar loads and the loop over the neighbours
// is wave-uniform.  The neighbour's pixel is a plain gather from the input - H is smooth, so the lanes of a wave land next
// to each other and the lines come out of L2.  Neighbours are read from the input only: no pixel's result depends on
// another's, hence on no schedule.  The translation unit is built with -ffp-contract=off: every product below is rounded
// before it is added, as the contract's numpy restatement does it.
//
// The per-frame counts are integers: ballots and a packed wave sum, LDS atomics per wave, then one 64-bit atomic per
// counter and workgroup.  All stores are plain vector stores or atomics.
// =================================================================================================
constexpr int kMvTileX = 32, kMvTileY = 8;  // pixels per workgroup (one per lane; a wave covers 32 x 2)

// the level of an element and whether the pixel is valid (uint8: v; uint16: v / 16; float64: v, valid iff > 0 and finite)
__device__ __forceinline__ bool mv_level(uint8_t v, double& d)
{
    d = (double)v;
    return v != 0;
}
__device__ __forceinline__ bool mv_level(uint16_t v, double& d)
{
    d = (double)v / 16.0;
    return v != 0;
}
__device__ __forceinline__ bool mv_level(double v, double& d)
{
    d = v;
    return v > 0.0 && v <= 1.7976931348623157e308;  // (false on NaN and on +inf)
}

// One pixel of the filter (kFuse = false) or of the fusion (kFuse = true; contract: include/o3dr.h "multi-view fusion").  The
// fusion runs the filter's tests unchanged and adds, per supporting neighbour, the level v on this pixel's own ray at which
// the neighbour would have seen exactly what it saw (two products and sums that the test already has in part, one more
// division), the sum of those votes in the order of the neighbour list, an 8-byte store per lane in place of the filter's
// element, and three more counters: a second packed wave sum for the two per-support counts, a ballot for the third.
template <class T, bool kFuse>
__device__ __forceinline__ void mv_pixel(const MvArgs& a, int tiles_x)
{
    constexpr int kWords = kFuse ? 12 : 9;
    __shared__ unsigned int s_cnt[kWords];
    const int f = a.f0 + (int)blockIdx.y, W = a.cols, Hh = a.rows;
    const int tid = (int)threadIdx.x;
    const int x = (int)(blockIdx.x % tiles_x) * kMvTileX + (tid & (kMvTileX - 1));
    const int y = (int)(blockIdx.x / tiles_x) * kMvTileY + tid / kMvTileX;
    if (tid < kWords) s_cnt[tid] = 0;
    __syncthreads();
    const bool in = x < W && y < Hh;
    const char* base = (const char*)a.in;
    T v = T(0);
    double d = 0.0;
    bool valid = false;
    if (in) {
        v = *(const T*)(base + (int64_t)f * a.fstride + (int64_t)y * a.pitch + (int64_t)x * (int64_t)sizeof(T));
        valid = mv_level(v, d);
    }
    const double xd = (double)x, yd = (double)y, Wd = (double)W, Hd = (double)Hh;
    unsigned int sup = 0, vio = 0, n_out = 0, n_hole = 0, n_occ = 0, votes = 0;
    double acc = d;  // (fusion: the pixel's own level, then every vote)
    const int32_t* __restrict__ nb = a.neighbors + (int64_t)f * a.k;
    const double* __restrict__ Hf = a.H + (int64_t)f * a.k * 16;
    for (int n = 0; n < a.k; ++n) {  // (wave-uniform: nb and Hf depend on the workgroup alone)
        const int j = nb[n];
        if (j < 0) continue;
        const double* __restrict__ M = Hf + n * 16;
        const double h0 = ((M[0] * xd + M[1] * yd) + M[2] * d) + M[3];
        const double h1 = ((M[4] * xd + M[5] * yd) + M[6] * d) + M[7];
        const double h2 = ((M[8] * xd + M[9] * yd) + M[10] * d) + M[11];
        const double h3 = ((M[12] * xd + M[13] * yd) + M[14] * d) + M[15];
        const double xp = h0 / h3, yp = h1 / h3, dp = h2 / h3;
        const double xr = floor(xp + 0.5), yr = floor(yp + 0.5);
        // (every comparison is false on NaN)
        const bool inside = valid && h3 > 0.0 && dp > 0.0 && 0.0 <= xr && xr < Wd && 0.0 <= yr && yr < Hd;
        double e = 0.0;
        bool ok = false;
        if (inside) {  // 0 <= xr < cols and 0 <= yr < rows hold here, and the host checked 0 <= j < n_frames
            const T w = *(const T*)(base + (int64_t)j * a.fstride + (int64_t)(int)yr * a.pitch + (int64_t)(int)xr * (int64_t)sizeof(T));
            ok = mv_level(w, e);
        }
        const bool is_sup = inside && ok && fabs(e - dp) <= a.tolerance;
        const bool is_vio = inside && ok && !is_sup && e < dp;
        sup += is_sup;
        vio += is_vio;
        n_out += valid && !inside;
        n_hole += inside && !ok;
        n_occ += inside && ok && !is_sup && !is_vio;
        if constexpr (kFuse) {
            const double a2 = (M[8] * xd + M[9] * yd) + M[11];
            const double a3 = (M[12] * xd + M[13] * yd) + M[15];
            const double num = e * a3 - a2;
            const double den = M[10] - e * M[14];
            const double vt = num / den;  // dp(vt) = e
            if (is_sup && vt > 0.0 && vt <= 1.7976931348623157e308) {  // (false on NaN and on +inf)
                acc = acc + vt;
                ++votes;
            }
        }
    }
    const bool enough = (int)sup >= a.min_support;
    const bool calm = a.max_violations < 0 ? vio < sup : (int)vio <= a.max_violations;
    const bool keep = valid && enough && calm;
    if (in) {
        const int64_t o = ((int64_t)f * Hh + y) * W + x;
        if constexpr (kFuse) {
            a.fused_out[o] = keep ? acc / (double)(1u + votes) : 0.0;
            if (a.votes_out) a.votes_out[o] = (uint8_t)votes;
        } else {
            ((T*)a.out)[o] = valid && !keep ? T(0) : v;
        }
        if (a.support_out) a.support_out[o] = (uint8_t)sup;
        if (a.violations_out) a.violations_out[o] = (uint8_t)vio;
    }
    if (a.info) {  // (wave-uniform)
        const unsigned long long bv = __ballot(valid), bk = __ballot(keep), bn = __ballot(valid && !enough),
                                 bc = __ballot(valid && enough && !calm);
        // five counts of at most 16 each (all 0 at an invalid pixel), 12 bits apart: a wave's sums stay below 2^12
        unsigned long long pk = (unsigned long long)n_out | (unsigned long long)n_hole << 12 | (unsigned long long)sup << 24 |
                                (unsigned long long)vio << 36 | (unsigned long long)n_occ << 48;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) pk += __shfl_xor(pk, o);
        // fusion: the votes and the supports that did not vote (at most 16 each, both 0 at an invalid pixel), and the kept
        // pixels that were fused
        unsigned int pv = kFuse ? votes | (sup - votes) << 12 : 0u;
        unsigned long long bf = 0;
        if constexpr (kFuse) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) pv += __shfl_xor(pv, o);
            bf = __ballot(keep && votes > 0);
        }
        if ((tid & 63) == 0) {
            atomicAdd(&s_cnt[0], (unsigned int)__popcll(bv));
            atomicAdd(&s_cnt[1], (unsigned int)__popcll(bk));
            atomicAdd(&s_cnt[2], (unsigned int)__popcll(bn));
            atomicAdd(&s_cnt[3], (unsigned int)__popcll(bc));
#pragma unroll
            for (int q = 0; q < 5; ++q) atomicAdd(&s_cnt[4 + q], (unsigned int)(pk >> (12 * q)) & 0xFFFu);
            if constexpr (kFuse) {
                atomicAdd(&s_cnt[9], pv & 0xFFFu);
                atomicAdd(&s_cnt[10], pv >> 12);
                atomicAdd(&s_cnt[11], (unsigned int)__popcll(bf));
            }
        }
        __syncthreads();
        if (tid < kWords && s_cnt[tid]) atomicAdd(a.info + (int64_t)f * kWords + tid, (unsigned long long)s_cnt[tid]);
    }
}

template <class T>
__global__ __launch_bounds__(kMvTileX* kMvTileY) void k_multiview_filter(MvArgs a, int tiles_x)
{
    mv_pixel<T, false>(a, tiles_x);
}
template <class T>
__global__ __launch_bounds__(kMvTileX* kMvTileY) void k_multiview_fuse(MvArgs a, int tiles_x)
{
    mv_pixel<T, true>(a, tiles_x);
}
