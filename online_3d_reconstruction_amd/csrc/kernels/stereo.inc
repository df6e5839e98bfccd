// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Stereo disparity: grey + 9 x 7 census of both images, semi-global aggregation of the Hamming cost along 4 or 8
// directions, winner with uniqueness, parabola and left-right check (contract: include/o3dr.h "stereo disparity";
// DESIGN.md "Stereo disparity").  Every value is an integer: nothing below depends on the launch geometry.  All stores
// are plain vector stores.
//
// Candidate layout of a wave: register j of lane l holds candidate e = 64 j + l (KJ = ceil(D / 64) registers; e >= D
// holds kStInf).  A wave's load or store of one register is then 64 consecutive elements, and d - 1 / d + 1 are the
// neighbouring lanes (DPP wave_shr:1 / wave_shl:1) with the edge lanes filled from the register below / above.
// =================================================================================================
constexpr int kStTileX = 64, kStTileY = 16;   // pixels per workgroup of the census pass (1 x 4 per lane)
constexpr int kStHaloX = 4, kStHaloY = 3;     // the 9 x 7 window
constexpr int kStTilePitch = kStTileX + 2 * kStHaloX;
constexpr int kStTileRows = kStTileY + 2 * kStHaloY;
constexpr int kStSeg = 256;                   // right-image columns per wave of the winner pass
constexpr uint32_t kStInf = 0x3fffu;          // above every L (<= 318) and every S (<= 2544), with room for + P
constexpr uint32_t kStKeyInf = 0xffffffffu;   // above every key S << 8 | d

// the value of the lane below, lane 0 takes `fill` (wave_shr:1); of the lane above, lane 63 takes `fill` (wave_shl:1)
__device__ __forceinline__ uint32_t st_from_below(uint32_t v, uint32_t fill)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t st_from_above(uint32_t v, uint32_t fill)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)fill, (int)v, 0x130, 0xf, 0xf, false);
}

// Grey and census of one tile of one image (blockIdx.z: 0 left, 1 right).  The tile and its halo go through LDS as grey
// bytes, clamped at the image border.
__global__ __launch_bounds__(256) void k_stereo_census(StereoArgs a, int tiles_x)
{
    __shared__ uint8_t tile[kStTileRows * kStTilePitch];
    const int f = blockIdx.y, W = a.cols, H = a.rows;
    const int x0 = (int)(blockIdx.x % tiles_x) * kStTileX, y0 = (int)(blockIdx.x / tiles_x) * kStTileY;
    const uint8_t* src = (blockIdx.z ? a.right : a.left) + (int64_t)f * a.fstride;
    unsigned long long* dst = (blockIdx.z ? a.cenR : a.cenL) + (int64_t)f * W * H;
    for (int i = threadIdx.x; i < kStTileRows * kStTilePitch; i += 256) {
        const int ty = i / kStTilePitch, tx = i - ty * kStTilePitch;
        const int gx = min(max(x0 + tx - kStHaloX, 0), W - 1), gy = min(max(y0 + ty - kStHaloY, 0), H - 1);
        const uint8_t* p = src + (int64_t)gy * a.pitch + (int64_t)gx * a.channels;
        tile[i] = a.channels == 3 ? (uint8_t)orb_grey(p[0], p[1], p[2]) : p[0];
    }
    __syncthreads();
    const int px = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int py = (int)(threadIdx.x >> 6) + 4 * k;
        const int x = x0 + px, y = y0 + py;
        if (x >= W || y >= H) continue;
        const uint8_t* c = tile + (py + kStHaloY) * kStTilePitch + px + kStHaloX;
        const uint32_t g = c[0];
        unsigned long long bits = 0;
        int n = 0;
#pragma unroll
        for (int dy = -kStHaloY; dy <= kStHaloY; ++dy)
#pragma unroll
            for (int dx = -kStHaloX; dx <= kStHaloX; ++dx) {
                if (dx == 0 && dy == 0) continue;
                bits |= (unsigned long long)(c[dy * kStTilePitch + dx] < g) << n;
                ++n;
            }
        dst[(int64_t)y * W + x] = bits;
    }
}

// One direction of the aggregation, one wave per scan line.  The wave walks its line from the border pixel inwards;
// the matching cost comes from the two census images on the way and S takes L_r: stored by the call's first direction,
// read, added and stored by the others (the launches of a group are ordered, so no atomics).  The loads of the next
// pixel are issued before the current pixel's chain step.
template <int KJ>
__global__ __launch_bounds__(256) void k_stereo_path(StereoArgs a, int dx, int dy, int first_dir)
{
    const int lane = threadIdx.x & 63, W = a.cols, H = a.rows, D = a.D;
    const int line = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int n_lines = dy == 0 ? H : dx == 0 ? W : W + H - 1;
    if (line >= n_lines) return;  // (wave-uniform)
    int x, y;
    if (dy == 0) {
        x = dx > 0 ? 0 : W - 1, y = line;
    } else if (line < W) {
        x = line, y = dy > 0 ? 0 : H - 1;
    } else {
        const int k = line - W + 1;
        x = dx > 0 ? 0 : W - 1, y = dy > 0 ? k : H - 1 - k;
    }
    const int64_t n = (int64_t)W * H;
    const unsigned long long* cl = a.cenL + (int64_t)blockIdx.y * n;
    const unsigned long long* cr = a.cenR + (int64_t)blockIdx.y * n;
    uint16_t* S = a.S + (int64_t)blockIdx.y * n * D;
    const uint32_t P1 = (uint32_t)a.p1, P2 = (uint32_t)a.p2;

    unsigned long long c_cur = 0, c_nxt = 0, r_cur[KJ], r_nxt[KJ];
    uint32_t s_cur[KJ], s_nxt[KJ], L[KJ];
    auto load = [&](int px, int py, unsigned long long& c, unsigned long long* r, uint32_t* s) {
        const int64_t p = (int64_t)py * W + px;
        c = cl[p];
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
            const int e = 64 * j + lane, xr = px - a.d0 - e;
            r[j] = (e < D && xr >= 0) ? cr[p - a.d0 - e] : 0ull;
            s[j] = (!first_dir && e < D) ? (uint32_t)S[p * D + e] : 0u;
        }
    };
    load(x, y, c_cur, r_cur, s_cur);
#pragma unroll
    for (int j = 0; j < KJ; ++j) L[j] = kStInf;
    uint32_t m = 0;
    bool first = true;
    while (true) {
        const int xn = x + dx, yn = y + dy;
        const bool more = xn >= 0 && xn < W && yn >= 0 && yn < H;  // (wave-uniform)
        if (more) load(xn, yn, c_nxt, r_nxt, s_nxt);
        uint32_t fill_lo[KJ], fill_hi[KJ];
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
            fill_lo[j] = j > 0 ? (uint32_t)__builtin_amdgcn_readlane((int)L[j > 0 ? j - 1 : 0], 63) : kStInf;
            fill_hi[j] = j < KJ - 1 ? (uint32_t)__builtin_amdgcn_readlane((int)L[j < KJ - 1 ? j + 1 : j], 0) : kStInf;
        }
        uint32_t lmin = kStInf;
        const int64_t p = (int64_t)y * W + x;
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
            const int e = 64 * j + lane, xr = x - a.d0 - e;
            const uint32_t C = xr >= 0 ? (uint32_t)__popcll(c_cur ^ r_cur[j]) : 63u;
            uint32_t v = C;
            if (!first) {
                const uint32_t lo = st_from_below(L[j], fill_lo[j]), hi = st_from_above(L[j], fill_hi[j]);
                v = C + u32_min(u32_min(L[j], m + P2), u32_min(lo, hi) + P1) - m;
            }
            v = e < D ? v : kStInf;
            L[j] = v;
            lmin = u32_min(lmin, v);
            if (e < D) S[p * D + e] = (uint16_t)(s_cur[j] + v);
        }
        if (!more) break;
        m = wave_min_u32(lmin);
        first = false;
        x = xn, y = yn;
        c_cur = c_nxt;
#pragma unroll
        for (int j = 0; j < KJ; ++j) r_cur[j] = r_nxt[j], s_cur[j] = s_nxt[j];
    }
}

// Winner of every left pixel and of every right pixel, one read of S.  A wave owns columns [c0, c0 + kStSeg) of row y,
// as left pixels and as right pixels, and walks x from c0 to the last column that holds a candidate of its right
// pixels.  Left: the lowest minimiser, uniqueness and the parabola go into `win` as cost << 16 | rejected << 15 |
// (off + 8) << 8 | best.  Right: lane e keeps the running minimum key of right pixel x - d0 - e; every step the keys
// move up one candidate, the top one is complete and goes out, a fresh one enters at candidate 0; what is left at the
// end of the row goes out as it is (those right pixels have fewer than D candidates inside the image).
template <int KJ>
__global__ __launch_bounds__(256) void k_stereo_winner(StereoArgs a, int n_seg)
{
    const int lane = threadIdx.x & 63, W = a.cols, H = a.rows, D = a.D;
    const int wv = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (wv >= H * n_seg) return;  // (wave-uniform)
    const int y = wv / n_seg, c0 = (wv - y * n_seg) * kStSeg, c1 = min(c0 + kStSeg, W);
    const int x_end = min(W, c1 + a.d0 + D - 1);
    const int64_t n = (int64_t)W * H, row = (int64_t)y * W;
    const uint16_t* S = a.S + (int64_t)blockIdx.y * n * D;
    uint32_t* win = a.win + (int64_t)blockIdx.y * n;
    uint8_t* bestR = a.bestR + (int64_t)blockIdx.y * n;
    const int top_j = (D - 1) >> 6, top_lane = (D - 1) & 63;

    uint32_t acc[KJ], s[KJ], s_nxt[KJ];
#pragma unroll
    for (int j = 0; j < KJ; ++j) acc[j] = kStKeyInf;
    auto load = [&](int px, uint32_t* v) {
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
            const int e = 64 * j + lane;
            v[j] = e < D ? (uint32_t)S[(row + px) * D + e] : kStInf;
        }
    };
    auto at = [&](int d) {  // S(x, d), d wave-uniform
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < KJ; ++j)
            if ((d >> 6) == j) v = (uint32_t)__builtin_amdgcn_readlane((int)s[j], d & 63);
        return v;
    };
    load(c0, s);
    for (int x = c0; x < x_end; ++x) {
        if (x + 1 < x_end) load(x + 1, s_nxt);
        uint32_t key[KJ], kmin = kStKeyInf;
#pragma unroll
        for (int j = 0; j < KJ; ++j) {
            const int e = 64 * j + lane;
            key[j] = e < D ? (s[j] << 8 | (uint32_t)e) : kStKeyInf;
            kmin = u32_min(kmin, key[j]);
            acc[j] = u32_min(acc[j], key[j]);
        }
        if (x < c1) {  // (wave-uniform) the left pixel
            kmin = wave_min_u32(kmin);
            const int best = (int)(kmin & 255u);
            const uint32_t b = kmin >> 8;
            uint32_t rej = x - a.d0 - best < 0;
            if (a.uniq > 0) {
                uint32_t other = kStInf;
#pragma unroll
                for (int j = 0; j < KJ; ++j) {
                    const int e = 64 * j + lane;
                    if (e < D && (e < best - 1 || e > best + 1)) other = u32_min(other, s[j]);
                }
                other = wave_min_u32(other);
                if (other != kStInf && other * (uint32_t)(100 - a.uniq) < 100u * b) rej = 1;
            }
            int off = 0;
            if (best > 0 && best < D - 1) {
                const int sa = (int)at(best - 1), sc = (int)at(best + 1);
                const int den = sa - 2 * (int)b + sc;
                if (den > 0) {
                    const int num = 16 * (sa - sc) + den;
                    off = num / (2 * den);
                    if (num % (2 * den) < 0) --off;
                }
            }
            if (lane == 0) win[row + x] = b << 16 | rej << 15 | (uint32_t)(off + 8) << 8 | (uint32_t)best;
        }
        {  // the right pixels
            const int xr_top = x - a.d0 - (D - 1);
            if (xr_top >= c0 && xr_top < c1 && lane == top_lane) {
#pragma unroll
                for (int j = 0; j < KJ; ++j)
                    if (j == top_j) bestR[row + xr_top] = (uint8_t)(acc[j] & 255u);
            }
            if (x + 1 < x_end) {
                uint32_t fill[KJ];
#pragma unroll
                for (int j = 0; j < KJ; ++j) fill[j] = j > 0 ? (uint32_t)__builtin_amdgcn_readlane((int)acc[j > 0 ? j - 1 : 0], 63) : kStKeyInf;
#pragma unroll
                for (int j = 0; j < KJ; ++j) acc[j] = st_from_below(acc[j], fill[j]);
#pragma unroll
                for (int j = 0; j < KJ; ++j) s[j] = s_nxt[j];
            }
        }
    }
    // the incomplete right pixels of the last step (x = x_end - 1); the top candidate went out in the loop
#pragma unroll
    for (int j = 0; j < KJ; ++j) {
        const int e = 64 * j + lane, xr = x_end - 1 - a.d0 - e;
        if (e < D - 1 && xr >= c0 && xr < c1) bestR[row + xr] = (uint8_t)(acc[j] & 255u);
    }
}

// The rejections that need the other pixel's winner, and the outputs (include/o3dr.h step 6 (a), (c) and step 7).
__global__ __launch_bounds__(256) void k_stereo_finish(StereoArgs a)
{
    const int W = a.cols;
    const int64_t n = (int64_t)W * a.rows, i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t fi = (int64_t)blockIdx.y * n + i;
    const uint32_t w = a.win[fi];
    const int best = (int)(w & 255u), off = (int)((w >> 8) & 31u) - 8;
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W), xr = x - a.d0 - best;
    bool rej = ((w >> 15) & 1u) || xr < 0;
    if (!rej && a.lr >= 0) {
        const int br = a.bestR[(int64_t)blockIdx.y * n + (int64_t)y * W + xr];
        rej = abs(br - best) > a.lr;
    }
    if (a.disp) a.disp[fi] = rej ? (uint8_t)0 : (uint8_t)(a.d0 + best);
    if (a.q4) a.q4[fi] = rej ? (uint16_t)0 : (uint16_t)(16 * (a.d0 + best) + off);
    if (a.cost) a.cost[fi] = (uint16_t)(w >> 16);
}
