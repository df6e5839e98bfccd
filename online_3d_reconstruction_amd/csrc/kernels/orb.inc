// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// ORB features: grey pyramid, FAST-9/16 score + 5 x 5 box sums, candidates (non-maximum suppression, margin, Harris
// response) in row-major order, exact selection of the quota per (frame, level), orientation + steered BRIEF (contract:
// include/o3dr.h "ORB features"; DESIGN.md "ORB features").  Every value is an integer: nothing below depends on the
// launch geometry.  All stores are plain vector stores.
// =================================================================================================
constexpr int kOrbTileX = 64, kOrbTileY = 32;          // pixels per workgroup of the FAST pass (4 x 2 per lane)
constexpr int kOrbHalo = 3;                            // the ring's radius
constexpr int kOrbTilePitch = kOrbTileX + 2 * kOrbHalo + 2;  // 72 bytes
constexpr int kOrbTileRows = kOrbTileY + 2 * kOrbHalo;
constexpr int kOrbDescWaves = 4;                       // keypoints per workgroup of the describe pass
__device__ const short2 kOrbDir[64] = {O3DR_ORB_DIRECTIONS};
// the radius-3 ring, clockwise from 12 o'clock (y down)
__device__ const signed char kOrbRingX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
__device__ const signed char kOrbRingY[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};

__device__ __forceinline__ uint32_t orb_grey(uint32_t b, uint32_t g, uint32_t r) { return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14; }

// Level 0.  CH = 3: interleaved B G R, 4 pixels (12 bytes) per lane; CH = 1: grey, 16 pixels per lane.  A lane's pixels
// are consecutive in the level's row-major order; when they share a row and start on a 4-byte boundary of the source
// they are read as whole words.
template <int CH, int PX>
__global__ __launch_bounds__(256) void k_orb_level0(OrbArgs a)
{
    const int f = blockIdx.y, W = a.cols;
    const int64_t n = (int64_t)a.rows * W, i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * PX;
    if (i0 >= n) return;
    const uint8_t* src = a.img + (int64_t)f * a.fstride;
    uint8_t* dst = a.pyr + (int64_t)f * a.P + i0;
    const int y0 = (int)(i0 / W), x0 = (int)(i0 - (int64_t)y0 * W);
    alignas(16) uint8_t g[PX];
    const uint8_t* p0 = src + (int64_t)y0 * a.pitch + (int64_t)x0 * CH;
    constexpr bool kWide = PX * CH % 16 == 0;  // grey: one 16-byte load; B G R: three words
    if (x0 + PX <= W && (reinterpret_cast<uintptr_t>(p0) & (kWide ? 15 : 3)) == 0) {
        alignas(16) uint8_t raw[PX * CH];
        if (kWide) {
#pragma unroll
            for (int q = 0; q < PX * CH / 16; ++q) reinterpret_cast<uint4*>(raw)[q] = reinterpret_cast<const uint4*>(p0)[q];
        } else {
#pragma unroll
            for (int q = 0; q < PX * CH / 4; ++q) reinterpret_cast<uint32_t*>(raw)[q] = reinterpret_cast<const uint32_t*>(p0)[q];
        }
#pragma unroll
        for (int k = 0; k < PX; ++k) g[k] = CH == 3 ? (uint8_t)orb_grey(raw[3 * k], raw[3 * k + 1], raw[3 * k + 2]) : raw[k];
    } else {
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const int64_t i = i0 + k;
            g[k] = 0;
            if (i < n) {
                const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
                const uint8_t* p = src + (int64_t)y * a.pitch + (int64_t)x * CH;
                g[k] = CH == 3 ? (uint8_t)orb_grey(p[0], p[1], p[2]) : p[0];
            }
        }
    }
    if (i0 + PX <= n) {  // (frame and level bases are multiples of 256, i0 of PX)
        if (PX == 16)
            *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(g);
        else
            *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(g);
    } else {
        for (int k = 0; k < PX && i0 + k < n; ++k) dst[k] = g[k];
    }
}

// Level l from level l - 1: fixed-point bilinear resampling, 4 consecutive output pixels per lane.
__global__ __launch_bounds__(256) void k_orb_down(OrbArgs a, int l)
{
    const int f = blockIdx.y;
    const int W = a.lv[l].w, H = a.lv[l].h, Ws = a.lv[l - 1].w, Hs = a.lv[l - 1].h;
    const int64_t n = (int64_t)W * H, i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    const uint8_t* src = a.pyr + (int64_t)f * a.P + a.lv[l - 1].off;
    uint8_t* dst = a.pyr + (int64_t)f * a.P + a.lv[l].off + i0;
    const int64_t rx = ((int64_t)Ws << 16) / W, ry = ((int64_t)Hs << 16) / H;
    alignas(4) uint8_t g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = i0 + k < n ? i0 + k : n - 1;
        const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
        int64_t fx = ((int64_t)(2 * x + 1) * rx - 65536) >> 1, fy = ((int64_t)(2 * y + 1) * ry - 65536) >> 1;
        fx = fx < 0 ? 0 : fx;
        fy = fy < 0 ? 0 : fy;
        int xa = (int)(fx >> 16), ya = (int)(fy >> 16);
        xa = xa < Ws - 1 ? xa : Ws - 1;
        ya = ya < Hs - 1 ? ya : Hs - 1;
        const int xb = xa + 1 < Ws - 1 ? xa + 1 : Ws - 1, yb = ya + 1 < Hs - 1 ? ya + 1 : Hs - 1;
        const uint32_t wx = (uint32_t)(fx & 0xFFFF) >> 5, wy = (uint32_t)(fy & 0xFFFF) >> 5;
        const uint32_t p00 = src[(int64_t)ya * Ws + xa], p01 = src[(int64_t)ya * Ws + xb], p10 = src[(int64_t)yb * Ws + xa],
                       p11 = src[(int64_t)yb * Ws + xb];
        const uint32_t s = p00 * (2048u - wx) * (2048u - wy) + p01 * wx * (2048u - wy) + p10 * (2048u - wx) * wy + p11 * wx * wy;
        g[k] = (uint8_t)((s + (1u << 21)) >> 22);
    }
    if (i0 + 4 <= n)
        *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(g);
    else
        for (int k = 0; k < 4 && i0 + k < n; ++k) dst[k] = g[k];
}

// FAST-9/16 score of the centre c against its ring: the best arc of 9 contiguous ring pixels, brighter or darker
__device__ __forceinline__ int orb_fast_score(const uint8_t* t /* the centre inside the LDS tile */)
{
    const int c = t[0];
    int d[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) d[i] = (int)t[kOrbRingY[i] * kOrbTilePitch + kOrbRingX[i]] - c;
    int best = -255;
#pragma unroll
    for (int pol = 0; pol < 2; ++pol) {
        int m2[16], m4[16], m8[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) m2[i] = min(d[i], d[(i + 1) & 15]);
#pragma unroll
        for (int i = 0; i < 16; ++i) m4[i] = min(m2[i], m2[(i + 2) & 15]);
#pragma unroll
        for (int i = 0; i < 16; ++i) m8[i] = min(m4[i], m4[(i + 4) & 15]);
#pragma unroll
        for (int i = 0; i < 16; ++i) best = max(best, min(m8[i], d[(i + 8) & 15]));
#pragma unroll
        for (int i = 0; i < 16; ++i) d[i] = -d[i];
    }
    return best;
}

// One 64 x 32 tile of a level through LDS with the ring's halo: the u8 score map (0: no corner, and 0 within 3 pixels
// of the border) and the u16 5 x 5 box sums (0 within 2 pixels of the border).
__global__ __launch_bounds__(256) void k_orb_fast(OrbArgs a, int l, int tiles_x)
{
    __shared__ uint8_t tile[kOrbTileRows * kOrbTilePitch];
    __shared__ uint16_t hs[(kOrbTileY + 4) * kOrbTileX];  // horizontal 5-sums of rows -2 .. kOrbTileY + 1
    const int f = blockIdx.y, W = a.lv[l].w, H = a.lv[l].h, tid = threadIdx.x;
    const int ty0 = ((int)blockIdx.x / tiles_x) * kOrbTileY, tx0 = ((int)blockIdx.x % tiles_x) * kOrbTileX;
    const int64_t base = (int64_t)f * a.P + a.lv[l].off;
    const uint8_t* img = a.pyr + base;
    for (int i = tid; i < kOrbTileRows * (kOrbTileX + 2 * kOrbHalo); i += 256) {
        const int r = i / (kOrbTileX + 2 * kOrbHalo), cx = i - r * (kOrbTileX + 2 * kOrbHalo);
        const int y = ty0 + r - kOrbHalo, x = tx0 + cx - kOrbHalo;
        tile[r * kOrbTilePitch + cx] = (x >= 0 && x < W && y >= 0 && y < H) ? img[(int64_t)y * W + x] : (uint8_t)0;
    }
    __syncthreads();
    for (int i = tid; i < (kOrbTileY + 4) * kOrbTileX; i += 256) {
        const int r = i / kOrbTileX, cx = i - r * kOrbTileX;  // image row ty0 + r - 2, column tx0 + cx
        const uint8_t* t = tile + (r + kOrbHalo - 2) * kOrbTilePitch + cx + kOrbHalo;
        hs[i] = (uint16_t)((int)t[-2] + t[-1] + t[0] + t[1] + t[2]);
    }
    __syncthreads();
    const int lx = (tid & 15) * 4;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int ly = (tid >> 4) + half * 16, y = ty0 + ly, x = tx0 + lx;
        if (y >= H || x >= W) continue;
        alignas(4) uint8_t sc[4];
        alignas(8) uint16_t bx[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int xx = x + k;
            int s = 0;
            if (xx >= kOrbHalo && xx < W - kOrbHalo && y >= kOrbHalo && y < H - kOrbHalo) {
                s = orb_fast_score(tile + (ly + kOrbHalo) * kOrbTilePitch + lx + k + kOrbHalo);
                s = s > a.thr ? s : 0;
            }
            sc[k] = (uint8_t)s;
            int b = 0;
            if (xx >= 2 && xx < W - 2 && y >= 2 && y < H - 2) {
                const uint16_t* h = hs + ly * kOrbTileX + lx + k;  // row y - 2
                b = (int)h[0] + h[kOrbTileX] + h[2 * kOrbTileX] + h[3 * kOrbTileX] + h[4 * kOrbTileX];
            }
            bx[k] = (uint16_t)b;
        }
        const int64_t o = (int64_t)y * W + x;
        if (x + 4 <= W && (o & 3) == 0) {
            *reinterpret_cast<uint32_t*>(a.score + base + o) = *reinterpret_cast<const uint32_t*>(sc);
            *reinterpret_cast<uint2*>(a.box + base + o) = *reinterpret_cast<const uint2*>(bx);
        } else {
            for (int k = 0; k < 4 && x + k < W; ++k) {
                a.score[base + o + k] = sc[k];
                a.box[base + o + k] = bx[k];
            }
        }
    }
}

// the level a chunk of a frame belongs to
__device__ __forceinline__ int orb_chunk_level(const OrbArgs& a, int chunk)
{
    int l = 0;
#pragma unroll
    for (int k = 1; k < kOrbMaxLevels; ++k)
        if (k < a.n_levels && a.lv[k].chunks > 0 && chunk >= a.lv[k].chunk0) l = k;
    return l;
}

// R = 25 (a b - c^2) - (a + b)^2 over the 7 x 7 window of Sobel-like derivatives
__device__ __forceinline__ long long orb_harris(const uint8_t* img, int W, int x, int y)
{
    int sa = 0, sb = 0, sc = 0;
    for (int v = -3; v <= 3; ++v) {
        const uint8_t* r0 = img + (int64_t)(y + v - 1) * W + x;
        const uint8_t* r1 = r0 + W;
        const uint8_t* r2 = r1 + W;
#pragma unroll
        for (int u = -3; u <= 3; ++u) {
            const int ix = 2 * ((int)r1[u + 1] - r1[u - 1]) + ((int)r0[u + 1] - r0[u - 1]) + ((int)r2[u + 1] - r2[u - 1]);
            const int iy = 2 * ((int)r2[u] - r0[u]) + ((int)r2[u - 1] - r0[u - 1]) + ((int)r2[u + 1] - r0[u + 1]);
            sa += ix * ix;
            sb += iy * iy;
            sc += ix * iy;
        }
    }
    const long long A = sa, B = sb, C = sc;
    return 25 * (A * B - C * C) - (A + B) * (A + B);
}

// Candidates of one chunk of 1024 consecutive pixels (4 per lane): corners that beat all 8 neighbours strictly, inside
// the margin.  EMIT = false: the chunk's count.  EMIT = true (after k_orb_scan): (R, position) at the chunk's offset plus
// the candidate's rank inside the chunk - the level's candidates end up in row-major order.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_orb_candidates(OrbArgs a)
{
    __shared__ uint32_t lds[5];
    const int f = blockIdx.y, chunk = blockIdx.x, l = orb_chunk_level(a, chunk);
    const int W = a.lv[l].w, H = a.lv[l].h, e = a.edge;
    const int64_t base = (int64_t)f * a.P + a.lv[l].off, n = (int64_t)W * H;
    const uint8_t* sm = a.score + base;
    const int64_t i0 = (int64_t)(chunk - a.lv[l].chunk0) * kOrbChunk + threadIdx.x * 4;
    uint32_t mask = 0;
    // the lane's 4 scores as one word (level bases are multiples of 256 and the level is padded to one): mostly zero
    const uint32_t word = i0 < n ? *reinterpret_cast<const uint32_t*>(sm + i0) : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t i = i0 + k;
        const int s = (int)((word >> (8 * k)) & 255u);
        if (s == 0 || i >= n) continue;
        const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
        if (x < e || x >= W - e || y < e || y >= H - e) continue;
        const uint8_t* p = sm + i;
        const bool keep = p[-1] < s && p[1] < s && p[-W - 1] < s && p[-W] < s && p[-W + 1] < s && p[W - 1] < s && p[W] < s && p[W + 1] < s;
        if (keep) mask |= 1u << k;
    }
    uint32_t total;
    const uint32_t before = block_excl_scan_u32<4>((uint32_t)__popc(mask), lds, total);
    if (!EMIT) {
        if (threadIdx.x == 0) a.chunk_cnt[(int64_t)f * a.chunks_per_frame + chunk] = total;
        return;
    }
    if (mask == 0) return;
    int64_t slot = (int64_t)f * a.cands_per_frame + a.lv[l].cand0 + a.chunk_cnt[(int64_t)f * a.chunks_per_frame + chunk] + before;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!((mask >> k) & 1u)) continue;
        const int64_t i = i0 + k;
        const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
        a.cand_r[slot] = orb_harris(a.pyr + base, W, x, y);
        a.cand_pos[slot] = ((uint32_t)y << 16) | (uint32_t)x;
        ++slot;
    }
}

// exclusive scan of a (frame, level)'s chunk counts in place; the total is the segment's candidate count
__global__ __launch_bounds__(256) void k_orb_scan(OrbArgs a)
{
    __shared__ uint32_t lds[5];
    const int l = blockIdx.x, f = blockIdx.y;
    uint32_t* cnt = a.chunk_cnt + (int64_t)f * a.chunks_per_frame + a.lv[l].chunk0;
    const int nc = a.lv[l].chunks;
    uint32_t run = 0;
    for (int c0 = 0; c0 < nc; c0 += 256) {
        const int c = c0 + threadIdx.x;
        const uint32_t v = c < nc ? cnt[c] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan_u32<4>(v, lds, total);
        if (c < nc) cnt[c] = run + ex;
        run += total;
    }
    if (threadIdx.x == 0) a.seg_cand[f * a.n_levels + l] = run;
}

// order-preserving unsigned image of R
__device__ __forceinline__ unsigned long long orb_key(long long r) { return (unsigned long long)r ^ 0x8000000000000000ull; }

// One workgroup per (frame, level): the quota-th largest key by an 8-pass radix select over LDS histograms, then the
// kept candidates - key above the cut, or equal to it and among the first ties in row-major order - compacted in order to
// the front of the segment's slots.
__global__ __launch_bounds__(256) void k_orb_select(OrbArgs a)
{
    __shared__ uint32_t hist[256];
    __shared__ uint32_t lds[10];
    __shared__ unsigned long long s_prefix;
    __shared__ uint32_t s_want;
    const int l = blockIdx.x, f = blockIdx.y, seg = f * a.n_levels + l, tid = threadIdx.x;
    const uint32_t n = a.seg_cand[seg], quota = (uint32_t)a.lv[l].quota;
    if (n <= quota || quota == 0) {  // everything is kept, or (a level whose share of n_features rounds to 0) nothing is
        if (tid == 0) a.seg_sel[seg] = n <= quota ? n : 0u;
        return;
    }
    long long* R = a.cand_r + (int64_t)f * a.cands_per_frame + a.lv[l].cand0;
    uint32_t* P = a.cand_pos + (int64_t)f * a.cands_per_frame + a.lv[l].cand0;
    if (tid == 0) {
        s_prefix = 0;
        s_want = quota;  // the rank, counted from the largest, of the cut key among the keys that share the prefix
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        const unsigned long long prefix = s_prefix, himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
        for (uint32_t i = tid; i < n; i += 256) {
            const unsigned long long k = orb_key(R[i]);
            if ((k & himask) == prefix) atomicAdd(&hist[(uint32_t)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t want = s_want;
            int d = 255;
            while (d > 0 && hist[d] < want) want -= hist[d--];
            s_want = want;
            s_prefix = prefix | ((unsigned long long)d << shift);
        }
        __syncthreads();
    }
    const unsigned long long cut = s_prefix;
    const uint32_t ties_kept = s_want;  // >= 1: quota >= 1 here, and every pass leaves want >= 1
    uint32_t run_tie = 0, run_out = 0;
    for (uint32_t c0 = 0; c0 < n; c0 += 256) {
        const uint32_t i = c0 + tid;
        long long r = 0;
        uint32_t p = 0;
        unsigned long long k = 0;
        if (i < n) {
            r = R[i];
            p = P[i];
            k = orb_key(r);
        }
        const bool tie = i < n && k == cut;
        uint32_t total;
        const uint32_t tie_rank = run_tie + block_excl_scan_u32<4>(tie ? 1u : 0u, lds, total);
        run_tie += total;
        const bool keep = i < n && (k > cut || (tie && tie_rank < ties_kept));
        const uint32_t o = run_out + block_excl_scan_u32<4>(keep ? 1u : 0u, lds + 5, total);
        run_out += total;
        if (keep) {  // o <= i, and every read of this round happened before the barriers of the scans
            R[o] = r;
            P[o] = p;
        }
    }
    if (tid == 0) a.seg_sel[seg] = run_out;  // == quota
}

// the first output row of every (frame, level) of the group, the frames' offsets and the running total
__global__ __launch_bounds__(256) void k_orb_offsets(OrbArgs a)
{
    __shared__ uint32_t lds[5];
    const int n = a.frames * a.n_levels;
    long long run = *a.run_total;
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int i = c0 + threadIdx.x;
        const uint32_t v = i < n ? a.seg_sel[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan_u32<4>(v, lds, total);
        if (i < n) {
            a.seg_out[i] = run + ex;
            if (i % a.n_levels == a.n_levels - 1) a.offsets[a.f0 + i / a.n_levels + 1] = run + ex + v;
        }
        run += total;
    }
    if (threadIdx.x == 0) *a.run_total = run;  // (read by every lane before the first barrier above)
}

__device__ __forceinline__ int orb_wave_sum_i32(int v) { return (int)wave_sum_u32((uint32_t)v); }

// One wave per keypoint: the intensity centroid over the disc u^2 + v^2 <= 240, the direction bin from the 64 dot
// products (one per lane), the 256 steered tests on the box sums (4 per lane, 4 ballots) and the record.
__global__ __launch_bounds__(64 * kOrbDescWaves) void k_orb_describe(OrbArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * kOrbDescWaves + (threadIdx.x >> 6);
    if (w >= (int64_t)a.frames * a.n_features) return;  // wave-uniform, like every exit below
    const int f = (int)(w / a.n_features), r = (int)(w - (int64_t)f * a.n_features);
    int l = 0;
#pragma unroll
    for (int k = 1; k < kOrbMaxLevels; ++k)
        if (k < a.n_levels && r >= a.lv[k].qprefix) l = k;
    const int j = r - a.lv[l].qprefix, seg = f * a.n_levels + l;
    if (j >= a.lv[l].quota || (uint32_t)j >= a.seg_sel[seg]) return;
    const int64_t slot = (int64_t)f * a.cands_per_frame + a.lv[l].cand0 + j, out = a.seg_out[seg] + j;
    const uint32_t pos = a.cand_pos[slot];
    const int x = (int)(pos & 0xffffu), y = (int)(pos >> 16), W = a.lv[l].w, H = a.lv[l].h;
    const int64_t base = (int64_t)f * a.P + a.lv[l].off;
    const uint8_t* img = a.pyr + base + (int64_t)y * W + x;
    int m10 = 0, m01 = 0;
#pragma unroll 4
    for (int it = 0; it < 16; ++it) {  // the 31 x 31 square, 64 positions at a time
        const int q = it * 64 + lane;
        const int v = q / 31 - 15, u = q - (v + 15) * 31 - 15;
        if (q < 961 && u * u + v * v <= 240) {
            const int I = img[(int64_t)v * W + u];
            m10 += u * I;
            m01 += v * I;
        }
    }
    m10 = orb_wave_sum_i32(m10);
    m01 = orb_wave_sum_i32(m01);
    // the bin: the largest dot product, the lowest lane on a tie
    const long long dot = (long long)m10 * kOrbDir[lane].x + (long long)m01 * kOrbDir[lane].y;
    long long best = dot;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const int lo = __shfl_xor((int)(uint32_t)(unsigned long long)best, s, 64), hi = __shfl_xor((int)(best >> 32), s, 64);
        const long long other = (long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo);
        best = other > best ? other : best;
    }
    const int bin = (m10 == 0 && m01 == 0) ? 0 : (int)__builtin_ctzll(__ballot(dot == best));
    if (a.desc) {
        const uint16_t* box = a.box + base + (int64_t)y * W + x;
        const char4* pat = reinterpret_cast<const char4*>(a.pattern) + bin * 256;
        unsigned long long bits[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const char4 t = pat[q * 64 + lane];
            const int ax = (signed char)t.x, ay = (signed char)t.y, bx = (signed char)t.z, by = (signed char)t.w;
            const uint32_t sa = box[(int64_t)ay * W + ax], sb = box[(int64_t)by * W + bx];
            bits[q] = __ballot(sa < sb);
        }
        if (lane == 0) {
            uint4* d = reinterpret_cast<uint4*>(a.desc + out * 32);
            d[0] = make_uint4((uint32_t)bits[0], (uint32_t)(bits[0] >> 32), (uint32_t)bits[1], (uint32_t)(bits[1] >> 32));
            d[1] = make_uint4((uint32_t)bits[2], (uint32_t)(bits[2] >> 32), (uint32_t)bits[3], (uint32_t)(bits[3] >> 32));
        }
    }
    if (lane == 0) {
        const float fx = (float)(((double)x + 0.5) * (double)a.cols / (double)W - 0.5);
        const float fy = (float)(((double)y + 0.5) * (double)a.rows / (double)H - 0.5);
        if (a.kp_xy) *reinterpret_cast<float2*>(a.kp_xy + out * 2) = make_float2(fx, fy);
        if (a.kp) {
            const long long R = a.cand_r[slot];
            const float ang = (float)bin * 5.625f, size = (float)(31.0 * (double)a.cols / (double)W);
            uint4* d = reinterpret_cast<uint4*>(a.kp + out);
            d[0] = make_uint4(__float_as_uint(fx), __float_as_uint(fy), __float_as_uint(ang), __float_as_uint(size));
            d[1] = make_uint4((uint32_t)(unsigned long long)R, (uint32_t)((unsigned long long)R >> 32),
                              ((uint32_t)(uint16_t)y << 16) | (uint32_t)(uint16_t)x, (uint32_t)l | ((uint32_t)bin << 8));
        }
    }
}
