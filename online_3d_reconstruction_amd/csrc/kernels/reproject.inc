// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// K1 — fused reprojection + rigid transform (A1 + A2)
//
//   pose_functions.cpp:1110-1121: vec = Q*(x,y,d,1) in fp64 (rows evaluated left to right),
//       vec /= vec(3) as multiplication by 1./vec(3) (+0), (float) casts, colour R<<16|G<<8|B;
//   pose_functions.cpp:1358-1362 -> pcl::transformPointCloud, dense branch:
//       x' = ((m00*x + m01*y) + m02*z) + m03 in fp32, no fused multiply-add.
// =================================================================================================
struct Pix {
    float x, y, z;
    uint32_t rgba;
};

// Layout classes of the fused batch path.  The depth of a stereo point is quantised (one disparity level is ~0.2 m at
// 20 m), so 8 neighbouring pixels - one 128-byte line of 16-byte points - land on two or three depth sheets that are far
// apart in voxel order, and the per-voxel sums (k_centroid), which walk the frame in voxel order, fetched every line
// once per sheet.  The emit pass therefore writes the points of a tile (1024 consecutive candidates) class by class:
// class = slab of the point's grid cell along the world axis closest to the optical axis, modulo kSlabClasses.  All
// points of a voxel share the class and the reordering is stable, so the order of the points inside every voxel - the
// order the sums are taken in - is the pixel order it always was; only which points share a line changes.
__device__ __forceinline__ int slab_axis(const float* m)
{
    const float ax = fabsf(m[2]), ay = fabsf(m[6]), az = fabsf(m[10]);  // world components of the camera's z axis
    return (az >= ax && az >= ay) ? 2 : (ay >= ax ? 1 : 0);
}
__device__ __forceinline__ uint32_t slab_class(const Pix& p, int axis, float inv, int shift)
{
    const float c = axis == 2 ? p.z : (axis == 1 ? p.y : p.x);
    const int cell = (int)floorf(c * inv);
    return (uint32_t)(cell >> shift) & (uint32_t)(kSlabClasses - 1);
}

__device__ __forceinline__ Pix reproject_one(const double* __restrict__ Q, int x, int y, double d,
                                             uint32_t b, uint32_t g, uint32_t r, const float* m, bool xf)
{
    const double v0 = (double)x, v1 = (double)y;
    const double t0 = ((Q[0] * v0 + Q[1] * v1) + Q[2] * d) + Q[3];
    const double t1 = ((Q[4] * v0 + Q[5] * v1) + Q[6] * d) + Q[7];
    const double t2 = ((Q[8] * v0 + Q[9] * v1) + Q[10] * d) + Q[11];
    const double t3 = ((Q[12] * v0 + Q[13] * v1) + Q[14] * d) + Q[15];
    const double alpha = 1. / t3;
    const float X = (float)(t0 * alpha + 0.0);
    const float Y = (float)(t1 * alpha + 0.0);
    const float Z = (float)(t2 * alpha + 0.0);
    Pix p;
    if (xf) {
        p.x = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3];
        p.y = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7];
        p.z = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11];
    } else {
        p.x = X;
        p.y = Y;
        p.z = Z;
    }
    p.rgba = (r << 16) | (g << 8) | b;
    return p;
}

// disparity bytes of the (up to) 4 candidates of one lane; returns the validity mask
// disparity image element: CV_8UC1, or CV_64F with --use_segment_labels (pose_functions.cpp:1037,1102)
template <bool F64> struct DispT { using type = uint32_t; };
template <> struct DispT<true> { using type = double; };

// A1 + A2 of ONE pixel: the arithmetic every kernel that produces a point shares (k_reproject_emit and the
// bounding-box pass of the batch path).  lut_alpha / lut_z: the rectified-stereo table in LDS (nullptr: general 4x4 product).
template <bool F64>
__device__ __forceinline__ Pix reproject_px(const ReprojectArgs& a, const double* __restrict__ lut_alpha,
                                            const float* __restrict__ lut_z, const float* m, bool xf, int x, int y,
                                            typename DispT<F64>::type d, uint32_t cb, uint32_t cg, uint32_t cr)
{
    if constexpr (!F64) {
        if (lut_alpha) {
            // same arithmetic as reproject_one with the exact-zero terms of Q dropped (adding
            // +-0 and multiplying by the tabulated 1./w change no bit of the result)
            const double al = lut_alpha[d];
            const float X = (float)((a.Q[0] * (double)x + a.Q[3]) * al + 0.0);
            const float Y = (float)((a.Q[5] * (double)y + a.Q[7]) * al + 0.0);
            const float Z = lut_z[d];
            Pix p;
            if (xf) {
                p.x = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3];
                p.y = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7];
                p.z = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11];
            } else {
                p.x = X; p.y = Y; p.z = Z;
            }
            p.rgba = (cr << 16) | (cg << 8) | cb;
            return p;
        }
    }
    return reproject_one(a.Q, x, y, (double)d, cb, cg, cr, m, xf);
}

template <bool F64>
__device__ __forceinline__ uint32_t load_lane_disparities(const ReprojectArgs& a, const uint8_t* __restrict__ disp,
                                                          int c0, int n_cand, int& x0, int& y0,
                                                          typename DispT<F64>::type d[4])
{
    uint32_t valid = 0;
    if (c0 >= n_cand) return 0;
    if (!F64 && a.vec4) {  // 4 consecutive pixels of one row, 4-byte aligned
        const int ry = c0 / a.Nx, rx = c0 - ry * a.Nx;
        y0 = a.bb + ry;
        x0 = a.cs + rx;
        const uint32_t w = *reinterpret_cast<const uint32_t*>(disp + (int64_t)y0 * a.disp_pitch + x0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[k] = (typename DispT<F64>::type)((w >> (8 * k)) & 255u);
            if ((int32_t)((w >> (8 * k)) & 255u) > a.min_disp_u8) valid |= 1u << k;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + k;
            d[k] = 0;
            if (c < n_cand) {
                const int ry = c / a.Nx, rx = c - ry * a.Nx;
                const uint8_t* row = disp + (int64_t)(a.bb + ry * a.jump) * a.disp_pitch;
                const int x = a.cs + rx * a.jump;
                if (F64) {
                    d[k] = (typename DispT<F64>::type)reinterpret_cast<const double*>(row)[x];
                    if ((double)d[k] > a.min_disp) valid |= 1u << k;
                } else {
                    d[k] = (typename DispT<F64>::type)row[x];
                    if ((int32_t)row[x] > a.min_disp_u8) valid |= 1u << k;
                }
            }
        }
    }
    return valid;
}

// pass 1: valid candidates per 1024-candidate tile (reads 1 byte per candidate)
template <bool F64>
__global__ __launch_bounds__(kEmitThreads) void k_reproject_count(ReprojectArgs a, uint32_t* __restrict__ tile_cnt)
{
    __shared__ uint32_t lds[kEmitThreads / 64];
    const int f = blockIdx.y, tile = blockIdx.x;
    const uint8_t* disp = a.disp + (int64_t)f * a.disp_fstride;
    const int n_cand = a.Ny * a.Nx;
    const int c0 = tile * kEmitTile + threadIdx.x * kEmitPerLane;
    int x0 = 0, y0 = 0;
    typename DispT<F64>::type d[4];
    const uint32_t valid = load_lane_disparities<F64>(a, disp, c0, n_cand, x0, y0, d);
    const uint32_t s = wave_sum_u32(__popc(valid));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < kEmitThreads / 64; ++i) t += lds[i];
        tile_cnt[(int64_t)f * a.n_tiles + tile] = t;
    }
}

// pass 1 of the fused batch path: valid candidates per tile AND the tile's bounding box of the transformed points (no
// colour is read), so that PCL's grid geometry is known before the points are written and the emit pass can
// compute the voxel index on the spot.  Same arithmetic as k_reproject_emit, hence the same extreme values.
constexpr int kCountTiles = 4;  // tiles per workgroup of k_reproject_bbox_count
#ifndef O3DR_CBOX_TILES
#define O3DR_CBOX_TILES 8
#endif
constexpr int kCboxTiles = O3DR_CBOX_TILES;  // ... and of k_reproject_count_cbox (its reductions are per workgroup)
// only_if_overflow (the pass after k_reproject_count_cbox): frames whose CONSERVATIVE box tripped PCL's overflow guard get
// their exact box here (the guard must be decided on the box PCL would see); the counts exist already and are not touched.
template <bool F64>
__global__ __launch_bounds__(kEmitThreads) void k_reproject_bbox_count(ReprojectArgs a, uint32_t* __restrict__ tile_cnt,
                                                                       float* __restrict__ mm,
                                                                       const VoxelGeom* __restrict__ only_if_overflow)
{
    static_assert(kCountTiles % 2 == 0, "two 16-bit counts per word");
    if (only_if_overflow && only_if_overflow[blockIdx.y].overflow == 0u) return;
    __shared__ uint32_t lds[(kCountTiles / 2) * (kEmitThreads / 64)];
    __shared__ float mm_lds[6 * (kEmitThreads / 64)];
    __shared__ double lut_alpha[256];
    __shared__ float lut_z[256];
    if (a.lut) {
        lut_alpha[threadIdx.x] = a.lut[threadIdx.x].alpha;
        lut_z[threadIdx.x] = a.lut[threadIdx.x].z;
        __syncthreads();
    }
    // a workgroup takes kCountTiles consecutive tiles: one set of wave reductions and barriers for both (the counts
    // stay per tile; the box of both goes to the first tile's slot, the other slots get the neutral box)
    const int f = blockIdx.y;
    const uint8_t* disp = a.disp + (int64_t)f * a.disp_fstride;
    const int n_cand = a.Ny * a.Nx;
    float m[12];
    {
        const float* T = a.poses + 16 * (int64_t)f;  // (batch path: xf_mode 2)
#pragma unroll
        for (int i = 0; i < 12; ++i) m[i] = T[i];
    }
    // (the grid covers the frame's tile groups once, or - the pass behind the conservative box, where nearly every
    // workgroup returns above - is a few workgroups per frame that walk them)
    const int n_groups = (a.n_tiles + kCountTiles - 1) / kCountTiles;
#pragma unroll 1
    for (int tg = blockIdx.x; tg < n_groups; tg += gridDim.x) {
        const int tile0 = tg * kCountTiles;
        int x0[kCountTiles], y0[kCountTiles];
        typename DispT<F64>::type d[kCountTiles][4];
        uint32_t valid[kCountTiles];
#pragma unroll
        for (int t = 0; t < kCountTiles; ++t) {
            x0[t] = y0[t] = 0;
            valid[t] = load_lane_disparities<F64>(a, disp, (tile0 + t) * kEmitTile + (int)threadIdx.x * kEmitPerLane, n_cand, x0[t], y0[t], d[t]);
        }
        float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
        float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        uint32_t packed[kCountTiles / 2];  // the tiles' valid candidates of this lane, 16 bits per tile
#pragma unroll
        for (int j = 0; j < kCountTiles / 2; ++j) packed[j] = 0;
        bool any = false;
#pragma unroll
        for (int t = 0; t < kCountTiles; ++t) {
            const int c0 = (tile0 + t) * kEmitTile + (int)threadIdx.x * kEmitPerLane;
            packed[t / 2] += (uint32_t)__popc(valid[t]) << (16 * (t & 1));
            any = any || valid[t] != 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (valid[t] & (1u << k)) {
                    int x, y;
                    if (!F64 && a.vec4) {
                        x = x0[t] + k;
                        y = y0[t];
                    } else {
                        const int c = c0 + k;
                        const int ry = c / a.Nx, rx = c - ry * a.Nx;
                        y = a.bb + ry * a.jump;
                        x = a.cs + rx * a.jump;
                    }
                    const Pix p = reproject_px<F64>(a, a.lut ? lut_alpha : nullptr, lut_z, m, true, x, y, d[t][k], 0, 0, 0);
                    lo[0] = fminf(lo[0], p.x); hi[0] = fmaxf(hi[0], p.x);
                    lo[1] = fminf(lo[1], p.y); hi[1] = fmaxf(hi[1], p.y);
                    lo[2] = fminf(lo[2], p.z); hi[2] = fmaxf(hi[2], p.z);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kCountTiles / 2; ++j) {
            const uint32_t s = wave_sum_u32(packed[j]);
            if ((threadIdx.x & 63) == 0) lds[j * (kEmitThreads / 64) + (threadIdx.x >> 6)] = s;
        }
        block_minmax_store<kEmitThreads / 64>(lo, hi, any, mm_lds, mm + ((int64_t)f * a.mm_stride + tile0) * 6);
        if (!only_if_overflow && threadIdx.x < kCountTiles && tile0 + (int)threadIdx.x < a.n_tiles) {
            uint32_t t = 0;
#pragma unroll
            for (int i = 0; i < kEmitThreads / 64; ++i) t += lds[(threadIdx.x / 2) * (kEmitThreads / 64) + i];
            tile_cnt[(int64_t)f * a.n_tiles + tile0 + threadIdx.x] = (t >> (16 * (threadIdx.x & 1))) & 0xffffu;
        }
        if (threadIdx.x >= 6 && threadIdx.x < 6 * kCountTiles && tile0 + (int)threadIdx.x / 6 < a.n_tiles) {
            const int a6 = threadIdx.x % 6;
            mm[((int64_t)f * a.mm_stride + tile0 + threadIdx.x / 6) * 6 + a6] = a6 < 3 ? __builtin_inff() : -__builtin_inff();
        }
        __syncthreads();  // (the next round reuses the count words)
    }
}

// The same pass without the reprojection arithmetic (rectified-stereo Q, byte disparities): valid candidates per tile,
// and a CONSERVATIVE bounding box instead of the exact one.  The batch path needs a box before it writes points only to
// lay the voxel grid: ordering and occupancy do not depend on where the grid starts (indices are taken relative to
// min_b, and a larger box only makes them wider), so any box that CONTAINS every point serves - as long as PCL's overflow
// guard, which is decided on the exact box, cannot come out differently: a conservative box below the guard proves the
// exact one is below it; frames whose conservative box trips it get the exact pass (k_reproject_bbox_count above).
// Per wave (kCboxTiles pieces of 256 candidates, about a row apart): the ranges of x, y and disparity over the
// valid pixels; a world coordinate is, for fixed disparity, linear in x and y, and for fixed (x, y) a ratio of linear
// functions of the disparity (monotone), so over that box of (x, y, d) its extremes lie at the 8 corners.  Eight lanes
// evaluate the corners with the arithmetic of the emit pass; the box is widened by 2^-17 of the largest sum of
// magnitudes entering a coordinate, eight times what the fp32 / fp64 roundings of a pixel and a corner can differ from
// the exact values by (5 roundings of at most 2^-24 of that sum each).
// Which lane holds which pixels (kWide: the packed-load layout, ReprojectArgs::vec4).  A wave's share of a tile is 256
// consecutive candidates.  One dword per lane and tile makes every wave load a 256-byte request, and the pass ran at a
// quarter of the rate k_radix_hist reaches on a read-only stream.  With kWide, lane l takes piece l >> 3 of a round of 8
// tiles and 32 consecutive candidates of it, as two 16-byte loads from a 4-byte boundary; a 16-candidate group that
// crosses the end of a ROI row (or of the frame) falls back to its four dword loads - Nx is a multiple of 4 there, so a
// quad never crosses (and the launcher asks for Nx >= 32: a lane's run then crosses at most one row end).  The SET of pixels a wave covers is the same in both layouts, hence the same ranges, the same
// corners and margins, and the same box and counts bit for bit.  A tile's count: the sum over the 8 lanes of its piece.
// n_kp != nullptr: workgroup (0, f) also writes the neutral box of the keypoint slot (n_tiles) and n_kp[f] = 0 - what
// k_minmax_init does in front of the other paths (no keypoint pass runs in front of this one).
__device__ __forceinline__ void cbox_quad(uint32_t w, int x0, int y0, int32_t min_disp_u8, uint32_t& cnt, uint32_t& xmn,
                                          uint32_t& xmx, uint32_t& ymn, uint32_t& ymx, uint32_t& dmn, uint32_t& dmx)
{
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t b = (w >> (8 * k)) & 255u;
        if ((int32_t)b > min_disp_u8) {
            m |= 1u << k;
            dmn = u32_min(dmn, b); dmx = u32_max(dmx, b);
        }
    }
    if (m) {
        cnt += (uint32_t)__popc(m);
        xmn = u32_min(xmn, (uint32_t)(x0 + __ffs((int)m) - 1)); xmx = u32_max(xmx, (uint32_t)(x0 + 31 - __clz((int)m)));
        ymn = u32_min(ymn, (uint32_t)y0); ymx = u32_max(ymx, (uint32_t)y0);
    }
}
template <int kTiles, bool kWide>
__global__ __launch_bounds__(kEmitThreads) void k_reproject_count_cbox(ReprojectArgs a, uint32_t* __restrict__ tile_cnt,
                                                                       float* __restrict__ mm, uint32_t* __restrict__ n_kp)
{
    constexpr int kWaves = kEmitThreads / 64;
    static_assert(kTiles % 8 == 0, "a round of the wide layout is 8 tiles, one per 8 lanes");
    __shared__ uint32_t lds[kWide ? kTiles * kWaves : (kTiles / 2) * kWaves];
    __shared__ float mm_lds[6 * kWaves];
    const int f = blockIdx.y, tile0 = blockIdx.x * kTiles;
    const uint8_t* disp = a.disp + (int64_t)f * a.disp_fstride;
    const int n_cand = a.Ny * a.Nx;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (n_kp && blockIdx.x == 0) {
        if (threadIdx.x < 6)
            mm[((int64_t)f * a.mm_stride + a.n_tiles) * 6 + threadIdx.x] = threadIdx.x < 3 ? __builtin_inff() : -__builtin_inff();
        else if (threadIdx.x == 6)
            n_kp[f] = 0;
    }
    // the pose of the corner lanes depends on the frame alone: loaded here, not as a second round trip behind the reductions
    float m[12];
    {
        const float* T = a.poses + 16 * (int64_t)f;
#pragma unroll
        for (int i = 0; i < 12; ++i) m[i] = T[i];
    }
    uint32_t xmn = 0xffffffffu, xmx = 0u, ymn = 0xffffffffu, ymx = 0u, dmn = 0xffffffffu, dmx = 0u;
    if constexpr (kWide) {
        constexpr int kRounds = kTiles / 8;
        // (all loads first: 2 kRounds independent 16-byte requests in flight per lane; the dword loads of a group at a row
        // end go to registers of their own, so that no load waits for another one's destination)
        u32x4_a4_t q[kRounds][2];
        uint32_t e[kRounds][2][4];
        int lx[kRounds], ly[kRounds];  // the first of the lane's 32 candidates
        bool whole[kRounds][2];        // the group came as one 16-byte load
        const int x_end = a.cs + a.Nx;
        // pixel `step` candidates behind (x, y), step <= 32 <= Nx: at most one row end between them
        auto behind = [&](int x, int y, int step, int& qx, int& qy) {
            const bool wrap = x + step >= x_end;
            qx = x + step - (wrap ? a.Nx : 0);
            qy = y + (wrap ? 1 : 0);
        };
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int c = (tile0 + 8 * r + (lane >> 3)) * kEmitTile + w * 256 + (lane & 7) * 32;
            const int ry = c / a.Nx, rx = c - ry * a.Nx;
            lx[r] = a.cs + rx;
            ly[r] = a.bb + ry;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                int gx, gy;
                behind(lx[r], ly[r], 16 * h, gx, gy);
                whole[r][h] = c + 16 * h < n_cand && gx + 16 <= x_end;  // (the frame ends with a row)
                q[r][h] = u32x4_a4_t{0u, 0u, 0u, 0u};
                if (whole[r][h]) q[r][h] = *reinterpret_cast<const u32x4_a4_t*>(disp + (int64_t)gy * a.disp_pitch + gx);
            }
        }
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int c = (tile0 + 8 * r + (lane >> 3)) * kEmitTile + w * 256 + (lane & 7) * 32;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int j = 0; j < 4; ++j) e[r][h][j] = 0u;
                if (!whole[r][h]) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (c + 16 * h + 4 * j < n_cand) {
                            int qx, qy;
                            behind(lx[r], ly[r], 16 * h + 4 * j, qx, qy);
                            e[r][h][j] = *reinterpret_cast<const uint32_t*>(disp + (int64_t)qy * a.disp_pitch + qx);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kRounds; ++r) {
            const int c = (tile0 + 8 * r + (lane >> 3)) * kEmitTile + w * 256 + (lane & 7) * 32;
            uint32_t wd[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) wd[k] = whole[r][k >> 2] ? q[r][k >> 2][k & 3] : e[r][k >> 2][k & 3];
            // Dense frames: when all 32 candidates of every lane of the wave exist and are valid, their ranges are those of
            // all the bytes and of the run of pixels itself, and nothing is decided pixel by pixel.
            uint32_t bmn = 255u, bmx = 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t bt = (wd[k] >> (8 * i)) & 255u;
                    bmn = u32_min(bmn, bt); bmx = u32_max(bmx, bt);
                }
            }
            uint32_t cnt = 0;
            if (__all(c + 32 <= n_cand && (int32_t)bmn > a.min_disp_u8)) {
                cnt = 32;
                dmn = u32_min(dmn, bmn); dmx = u32_max(dmx, bmx);
                const bool wrap = lx[r] + 32 > x_end;  // the run goes on in the next row: both rows' ends are covered
                xmn = u32_min(xmn, (uint32_t)(wrap ? a.cs : lx[r])); xmx = u32_max(xmx, (uint32_t)(wrap ? x_end - 1 : lx[r] + 31));
                ymn = u32_min(ymn, (uint32_t)ly[r]); ymx = u32_max(ymx, (uint32_t)(ly[r] + (wrap ? 1 : 0)));
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (c + 4 * k < n_cand) {
                        int qx, qy;
                        behind(lx[r], ly[r], 4 * k, qx, qy);
                        cbox_quad(wd[k], qx, qy, a.min_disp_u8, cnt, xmn, xmx, ymn, ymx, dmn, dmx);
                    }
                }
            }
            // the piece's count: over its 8 lanes, which share a 16-lane row
            cnt += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cnt, 0x111, 0xf, 0xf, false);  // row_shr:1
            cnt += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cnt, 0x112, 0xf, 0xf, false);  // row_shr:2
            cnt += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cnt, 0x114, 0xf, 0xf, false);  // row_shr:4
            if ((lane & 7) == 7) lds[(8 * r + (lane >> 3)) * kWaves + w] = cnt;
        }
    } else {
        uint32_t packed[kTiles / 2];
#pragma unroll
        for (int j = 0; j < kTiles / 2; ++j) packed[j] = 0;
        // (all loads first: kTiles independent requests in flight per lane)
        int x0[kTiles], y0[kTiles];
        uint32_t d[kTiles][4], valid[kTiles];
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
            x0[t] = y0[t] = 0;
            valid[t] = load_lane_disparities<false>(a, disp, (tile0 + t) * kEmitTile + (int)threadIdx.x * kEmitPerLane, n_cand, x0[t], y0[t], d[t]);
        }
#pragma unroll
        for (int t = 0; t < kTiles; ++t) {
            const int c0 = (tile0 + t) * kEmitTile + (int)threadIdx.x * kEmitPerLane;
            packed[t / 2] += (uint32_t)__popc(valid[t]) << (16 * (t & 1));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (valid[t] & (1u << k)) {
                    int x, y;
                    if (a.vec4) {
                        x = x0[t] + k;
                        y = y0[t];
                    } else {
                        const int c = c0 + k;
                        const int ry = c / a.Nx, rx = c - ry * a.Nx;
                        y = a.bb + ry * a.jump;
                        x = a.cs + rx * a.jump;
                    }
                    xmn = u32_min(xmn, (uint32_t)x); xmx = u32_max(xmx, (uint32_t)x);
                    ymn = u32_min(ymn, (uint32_t)y); ymx = u32_max(ymx, (uint32_t)y);
                    dmn = u32_min(dmn, d[t][k]); dmx = u32_max(dmx, d[t][k]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kTiles / 2; ++j) {
            const uint32_t s = wave_sum_u32(packed[j]);
            if (lane == 0) lds[j * kWaves + w] = s;
        }
    }
    xmn = wave_min_u32(xmn); xmx = wave_max_u32(xmx);
    ymn = wave_min_u32(ymn); ymx = wave_max_u32(ymx);
    dmn = wave_min_u32(dmn); dmx = wave_max_u32(dmx);
    const bool any = dmn != 0xffffffffu;  // (uniform over the wave)
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    if (any && lane < 8) {
        const int x = (lane & 1) ? (int)xmx : (int)xmn, y = (lane & 2) ? (int)ymx : (int)ymn;
        const uint32_t d = (lane & 4) ? dmx : dmn;
        // the emit pass's arithmetic (reproject_px with the table), from the table in HBM
        const double al = a.lut[d].alpha;
        const float X = (float)((a.Q[0] * (double)x + a.Q[3]) * al + 0.0);
        const float Y = (float)((a.Q[5] * (double)y + a.Q[7]) * al + 0.0);
        const float Z = a.lut[d].z;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float p = ((m[4 * r] * X + m[4 * r + 1] * Y) + m[4 * r + 2] * Z) + m[4 * r + 3];
            const float mag = ((fabsf(m[4 * r] * X) + fabsf(m[4 * r + 1] * Y)) + fabsf(m[4 * r + 2] * Z)) + fabsf(m[4 * r + 3]);
            const float margin = mag * 7.62939453125e-06f;  // 2^-17
            lo[r] = p - margin;
            hi[r] = p + margin;
        }
    }
    block_minmax_store<kWaves>(lo, hi, any && lane < 8, mm_lds, mm + ((int64_t)f * a.mm_stride + tile0) * 6);
    if (threadIdx.x < kTiles && tile0 + (int)threadIdx.x < a.n_tiles) {
        uint32_t t = 0;
        if constexpr (kWide) {
#pragma unroll
            for (int i = 0; i < kWaves; ++i) t += lds[threadIdx.x * kWaves + i];
        } else {
#pragma unroll
            for (int i = 0; i < kWaves; ++i) t += lds[(threadIdx.x / 2) * kWaves + i];
            t = (t >> (16 * (threadIdx.x & 1))) & 0xffffu;
        }
        tile_cnt[(int64_t)f * a.n_tiles + tile0 + threadIdx.x] = t;
    }
    if (threadIdx.x >= 6 && threadIdx.x < 6 * kTiles && tile0 + (int)threadIdx.x / 6 < a.n_tiles) {
        const int a6 = threadIdx.x % 6;
        mm[((int64_t)f * a.mm_stride + tile0 + threadIdx.x / 6) * 6 + a6] = a6 < 3 ? __builtin_inff() : -__builtin_inff();
    }
}

// pass 2: recompute, transform, compact in row-major order, write 16-byte points coalesced
// KEYS (fused batch path: the grid geometry is already known, see k_reproject_bbox_count): the same pass also
// writes every point's voxel index for the sort, instead of a second kernel reading the 16-byte points back, and
// orders the tile's points by layout class (slab_class).  mm is not written then.
// A KEYS workgroup walks kEmitGroup consecutive tiles of one frame.  With `hist` it also counts the first radix pass's
// digits of the indices it writes: the first pass of such a frame sorts over CANDIDATE-ALIGNED tiles (sort tile t = the
// records of emit tiles [kEmitGroup t, kEmitGroup t + kEmitGroup), its scatter parts = the two halves of those emit
// tiles; see emit_part_range), so this workgroup is the only writer of sort tile blockIdx.x's histogram row and the
// counts leave as one 512-byte store - no global atomic, and k_radix_hist's pass over the indices is not needed.
// (Counted per emit tile into record-aligned sort tiles - one global atomic per non-empty (sort tile, digit), 19 M per
// 200-frame step - the counting cost this pass 0.2 ms and saved a 0.11 ms histogram pass.)
__device__ __forceinline__ void emit_digit_count(uint32_t* __restrict__ hw, bool ok, uint32_t dgt)
{
    // neighbouring records often share the digit: one add per wave then, else one LDS add per record
    const unsigned long long act = __ballot(ok);
    if (act == 0ull) return;
    const int first = __ffsll((long long)act) - 1;
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)dgt, first);
    if (__ballot(ok && dgt == d0) == act) {
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&hw[d0], (uint32_t)__popcll(act));
    } else if (ok) {
        atomicAdd(&hw[dgt], 1u);
    }
}
// KEYS: the tile loop keeps pose, geometry and Q live across tiles; left alone the allocator takes 85 VGPRs = 5 waves per
// SIMD, one workgroup per CU fewer than the 25.7 KB of LDS allow.  Asked for 6 it fits 79 (SGPR spills into lanes, no
// scratch).  The other instantiations (42-48 VGPRs, 8 waves) are not constrained by a minimum of 4.
template <bool F64, bool KEYS>
__global__ __launch_bounds__(kEmitThreads) __attribute__((amdgpu_waves_per_eu(KEYS ? 6 : 4)))
void k_reproject_emit(ReprojectArgs a, o3dr_point* __restrict__ out,
                                                                 const uint32_t* __restrict__ tile_off,
                                                                 const uint32_t* __restrict__ n_kp,
                                                                 float* __restrict__ mm,
                                                                 const VoxelGeom* __restrict__ geom, int64_t cap,
                                                                 uint32_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ hist,
                                                                 uint32_t* __restrict__ hist_part, int n_sort_tiles)
{
    constexpr int kGroup = KEYS ? kEmitGroup : 1;  // tiles per workgroup
    constexpr int kWaves = kEmitThreads / 64;
    __shared__ uint4 stage[kEmitTile];  // 16 KiB: the tile's points in output order
    __shared__ uint32_t key_stage[KEYS ? kEmitTile : 1];
    __shared__ uint32_t scan_lds[(kWaves + 1) * (KEYS ? kSlabClasses / 2 : 1)];
    __shared__ uint32_t cls_base[kSlabClasses + 1];
    __shared__ float mm_lds[6 * kWaves];
    __shared__ double lut_alpha[256];  // rectified-stereo Q: 1/w and Z depend on the disparity byte only
    __shared__ float lut_z[256];
    __shared__ uint32_t dcnt[KEYS ? kWaves * kMaxRadix : 1];  // digit counts of the workgroup's records, one table per wave
    if constexpr (KEYS) {
        // (the first count comes after the barriers of the first tile's scan)
        for (int i = threadIdx.x; i < kWaves * kMaxRadix; i += kEmitThreads) dcnt[i] = 0;
    }
    if (a.lut) {
        lut_alpha[threadIdx.x] = a.lut[threadIdx.x].alpha;
        lut_z[threadIdx.x] = a.lut[threadIdx.x].z;
        __syncthreads();
    }
    const int f = blockIdx.y;
    const uint8_t* disp = a.disp + (int64_t)f * a.disp_fstride;
    const uint8_t* bgr = a.bgr + (int64_t)f * a.bgr_fstride;
    const int n_cand = a.Ny * a.Nx;

    float m[12];
    const bool xf = a.xf_mode != 0;
    if (a.xf_mode == 2) {
        const float* T = a.poses + 16 * (int64_t)f;  // wave-uniform: scalar loads
#pragma unroll
        for (int i = 0; i < 12; ++i) m[i] = T[i];
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) m[i] = a.T[i];
    }
    VoxelGeom g;
    bool want_keys = false, part = false, count = false;
    int s_axis = 0;
    float s_inv = 0.f;
    uint32_t dmask = 0;
    if constexpr (KEYS) {
        g = geom[f];
        want_keys = !g.overflow && g.n != 0u && g.passes != 0u;
        count = want_keys && hist != nullptr;
        dmask = (uint32_t)geom_bins(g) - 1u;  // the digit k_radix_hist counts in pass 0
        // PCL's overflow guard returns the input as it is: pixel order, one class
        part = a.slab_shift >= 0 && !g.overflow;
        s_axis = slab_axis(m);
        s_inv = a.slab_inv[s_axis];
    }
    // this workgroup's sort tile (KEYS with hist): row of the frame's tile-major histograms
    const int64_t hrow = ((int64_t)f * n_sort_tiles + blockIdx.x) * kMaxRadix;

#pragma unroll 1
    for (int j = 0; j < kGroup; ++j) {
        const int tile = blockIdx.x * kGroup + j;
        if (tile >= a.n_tiles) break;
        if constexpr (KEYS) {
            if (j == kGroup / kScatParts && count) {  // the first scatter part's records are counted
                __syncthreads();
                if (threadIdx.x < kMaxRadix) {
                    uint32_t t = 0;
#pragma unroll
                    for (int ww = 0; ww < kWaves; ++ww) t += dcnt[ww * kMaxRadix + threadIdx.x];
                    hist_part[hrow + threadIdx.x] = t;
                }
                // (the counting goes on in the same tables, behind the barriers of this tile's scan)
            }
        }
        const int c0 = tile * kEmitTile + threadIdx.x * kEmitPerLane;
        int x0 = 0, y0 = 0;
        typename DispT<F64>::type d[4];
        const uint32_t valid = load_lane_disparities<F64>(a, disp, c0, n_cand, x0, y0, d);

        Pix p[4];
        float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
        float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
        uint32_t cls4 = 0;                        // the lane's classes, 4 bits per pixel
        uint32_t pc[kSlabClasses / 2];            // its points per class, two 16-bit fields per word
#pragma unroll
        for (int q = 0; q < kSlabClasses / 2; ++q) pc[q] = 0;
        if (valid) {
            uint32_t cb[4], cg[4], cr[4];
            if (!F64 && a.vec4) {  // 12 colour bytes of 4 pixels = 3 aligned dwords
                const uint32_t* q = reinterpret_cast<const uint32_t*>(bgr + (int64_t)y0 * a.bgr_pitch + 3 * (int64_t)x0);
                const uint32_t w0 = q[0], w1 = q[1], w2 = q[2];
                cb[0] = w0 & 255u;         cg[0] = (w0 >> 8) & 255u;  cr[0] = (w0 >> 16) & 255u;
                cb[1] = w0 >> 24;          cg[1] = w1 & 255u;         cr[1] = (w1 >> 8) & 255u;
                cb[2] = (w1 >> 16) & 255u; cg[2] = w1 >> 24;          cr[2] = w2 & 255u;
                cb[3] = (w2 >> 8) & 255u;  cg[3] = (w2 >> 16) & 255u; cr[3] = w2 >> 24;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (valid & (1u << k)) {
                    int x, y;
                    if (!F64 && a.vec4) {
                        x = x0 + k;
                        y = y0;
                    } else {
                        const int c = c0 + k;
                        const int ry = c / a.Nx, rx = c - ry * a.Nx;
                        y = a.bb + ry * a.jump;
                        x = a.cs + rx * a.jump;
                        const uint8_t* px = bgr + (int64_t)y * a.bgr_pitch + 3 * (int64_t)x;
                        cb[k] = px[0];
                        cg[k] = px[1];
                        cr[k] = px[2];
                    }
                    p[k] = reproject_px<F64>(a, a.lut ? lut_alpha : nullptr, lut_z, m, xf, x, y, d[k], cb[k], cg[k], cr[k]);
                    lo[0] = fminf(lo[0], p[k].x); hi[0] = fmaxf(hi[0], p[k].x);
                    lo[1] = fminf(lo[1], p[k].y); hi[1] = fmaxf(hi[1], p[k].y);
                    lo[2] = fminf(lo[2], p[k].z); hi[2] = fmaxf(hi[2], p[k].z);
                    if constexpr (KEYS) {
                        const uint32_t cls = part ? slab_class(p[k], s_axis, s_inv, a.slab_shift) : 0u;
                        cls4 |= cls << (4 * k);
#pragma unroll
                        for (int q = 0; q < kSlabClasses / 2; ++q)
                            if ((cls >> 1) == (uint32_t)q) pc[q] += 1u << (16u * (cls & 1u));
                    }
                }
            }
        }
        if constexpr (!KEYS) {
            uint32_t total;
            uint32_t pos = block_excl_scan_u32<kWaves>(__popc(valid), scan_lds, total);
            const uint32_t base = n_kp[f] + tile_off[(int64_t)f * a.n_tiles + tile];  // the tile's first point inside the frame's cloud
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (valid & (1u << k)) {
                    stage[pos] = make_uint4(__float_as_uint(p[k].x), __float_as_uint(p[k].y), __float_as_uint(p[k].z), p[k].rgba);
                    ++pos;
                }
            }
            __syncthreads();
            uint4* dst = reinterpret_cast<uint4*>(out + (int64_t)f * a.out_fstride + base);
            for (uint32_t i = threadIdx.x; i < total; i += kEmitThreads) dst[i] = stage[i];
            block_minmax_store<kWaves>(lo, hi, valid != 0, mm_lds, mm + ((int64_t)f * a.mm_stride + tile) * 6);
        } else {
            // the tile's points go out class by class (slab_class), pixel order inside a class
            // (the scan's barriers also end the previous tile's reads of the staging buffers)
            uint32_t tot[kSlabClasses / 2];
            block_excl_scan_multi_u32<kWaves, kSlabClasses / 2>(pc, scan_lds, tot);  // pc: places inside the classes
            if (threadIdx.x == 0) {
                uint32_t run = 0;
#pragma unroll
                for (int q = 0; q < kSlabClasses / 2; ++q) {
                    cls_base[2 * q] = run;
                    run += tot[q] & 0xffffu;
                    cls_base[2 * q + 1] = run;
                    run += tot[q] >> 16;
                }
                cls_base[kSlabClasses] = run;
            }
            __syncthreads();
            const uint32_t total = cls_base[kSlabClasses];
            const uint32_t base = n_kp[f] + tile_off[(int64_t)f * a.n_tiles + tile];  // the tile's first point inside the frame's cloud
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (valid & (1u << k)) {
                    const uint32_t cls = (cls4 >> (4 * k)) & 15u;
                    const uint32_t sh = 16u * (cls & 1u);
                    uint32_t pos = cls_base[cls];
#pragma unroll
                    for (int q = 0; q < kSlabClasses / 2; ++q) {
                        if ((cls >> 1) == (uint32_t)q) {
                            pos += (pc[q] >> sh) & 0xffffu;  // among the tile's points of the class
                            pc[q] += 1u << sh;
                        }
                    }
                    const uint4 v = make_uint4(__float_as_uint(p[k].x), __float_as_uint(p[k].y), __float_as_uint(p[k].z), p[k].rgba);
                    stage[pos] = v;
                    if (want_keys) key_stage[pos] = voxel_key_of(v, g, 0.f);
                }
            }
            __syncthreads();
            uint4* dst = reinterpret_cast<uint4*>(out + (int64_t)f * a.out_fstride + base);
            for (uint32_t i = threadIdx.x; i < total; i += kEmitThreads) dst[i] = stage[i];
            if (want_keys) {
                uint32_t* kd = keys + (int64_t)f * cap + base;
                uint32_t* hw = dcnt + (threadIdx.x >> 6) * kMaxRadix;
                for (uint32_t i0 = 0; i0 < total; i0 += kEmitThreads) {  // (uniform trips: the count votes over the wave)
                    const uint32_t i = i0 + threadIdx.x;
                    const bool ok = i < total;
                    const uint32_t key = ok ? key_stage[i] : 0u;
                    if (ok) kd[i] = key;
                    if (count) emit_digit_count(hw, ok, key & dmask);
                }
            }
        }
    }
    if constexpr (KEYS) {
        // the tile's row leaves in one piece: all kMaxRadix entries whatever the digit's width, zeros included (this
        // workgroup is the row's only writer, and k_scan_hist_tm's all_live reads every row of a frame that counts)
        if (count) {
            __syncthreads();
            if (threadIdx.x < kMaxRadix) {
                uint32_t t = 0;
#pragma unroll
                for (int ww = 0; ww < kWaves; ++ww) t += dcnt[ww * kMaxRadix + threadIdx.x];
                hist[hrow + threadIdx.x] = t;
            }
        }
    }
}

// one keypoint of the keypoint pass (pose_functions.cpp:1061-1090): truncation to int, the ROI, d > min_disparity, then
// reproject_one; false: rejected.  bgr == nullptr: colour 0 (o3dr_keypoints_3d without an image)
__device__ __forceinline__ bool keypoint_one(const ReprojectArgs& a, const uint8_t* disp, const uint8_t* bgr, const float* m, bool xf,
                                             float kx, float ky, Pix& p)
{
    const int x = (int)kx, y = (int)ky;
    if (!(x >= a.cs && x < a.cols - a.bb && y >= a.bb && y < a.rows - a.bb)) return false;
    const uint8_t* row = disp + (int64_t)y * a.disp_pitch;
    const double d = a.disp_f64 ? reinterpret_cast<const double*>(row)[x] : (double)row[x];
    if (!(d > a.min_disp)) return false;
    uint32_t b = 0, g = 0, r = 0;
    if (bgr) {
        const uint8_t* px = bgr + (int64_t)y * a.bgr_pitch + 3 * (int64_t)x;
        b = px[0], g = px[1], r = px[2];
    }
    p = reproject_one(a.Q, x, y, d, b, g, r, m, xf);
    return true;
}

// keypoint pass (pose_functions.cpp:1057-1091): one workgroup walks the keypoints in order
// one workgroup per frame; kp_off (optional) holds the frames' ranges in kp_xy, else all n_kp belong to frame 0
__global__ __launch_bounds__(256) void k_keypoint_pass(ReprojectArgs a, const float* __restrict__ kp_xy, int n_kp,
                                                       const int32_t* __restrict__ kp_off, o3dr_point* __restrict__ out,
                                                       uint32_t* __restrict__ n_kp_out, float* __restrict__ mm)
{
    __shared__ uint32_t scan_lds[256 / 64 + 1];
    __shared__ float mm_lds[6 * 4];
    const int f = blockIdx.x;
    if (kp_off) {
        kp_xy += 2 * (int64_t)kp_off[f];
        n_kp = kp_off[f + 1] - kp_off[f];
    }
    const uint8_t* disp = a.disp + (int64_t)f * a.disp_fstride;
    const uint8_t* bgr = a.bgr + (int64_t)f * a.bgr_fstride;
    out += (int64_t)f * a.out_fstride;
    float m[12];
    const bool xf = a.xf_mode != 0;
    for (int i = 0; i < 12; ++i) m[i] = (a.xf_mode == 2) ? a.poses[16 * (int64_t)f + i] : a.T[i];
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    bool any = false;
    uint32_t base = 0;
    for (int i0 = 0; i0 < n_kp; i0 += 256) {
        const int i = i0 + threadIdx.x;
        bool ok = false;
        Pix p;
        if (i < n_kp) ok = keypoint_one(a, disp, bgr, m, xf, kp_xy[2 * i], kp_xy[2 * i + 1], p);
        uint32_t total;
        const uint32_t pos = block_excl_scan_u32<4>(ok ? 1u : 0u, scan_lds, total);
        if (ok) {
            o3dr_point q;
            q.x = p.x; q.y = p.y; q.z = p.z; q.rgba = p.rgba;
            out[base + pos] = q;
            any = true;
            lo[0] = fminf(lo[0], p.x); hi[0] = fmaxf(hi[0], p.x);
            lo[1] = fminf(lo[1], p.y); hi[1] = fmaxf(hi[1], p.y);
            lo[2] = fminf(lo[2], p.z); hi[2] = fmaxf(hi[2], p.z);
        }
        base += total;
    }
    if (threadIdx.x == 0) n_kp_out[f] = base;
    block_minmax_store<4>(lo, hi, any, mm_lds, mm + ((int64_t)f * a.mm_stride + a.n_tiles) * 6);  // slot after the grid tiles
}

// A2 alone: pcl::transformPointCloud on an existing cloud (also the in-place re-transform of
// cloud_big, pose.cpp:353)
struct Mat34 {
    float m[12];
};
// the A2 arithmetic of one point; also the transform of the ICP queries (kernels/nn.inc), which must match it bit for bit
__device__ __forceinline__ void a2_apply(const float* __restrict__ m, float x, float y, float z, float& X, float& Y, float& Z)
{
    X = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    Y = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    Z = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}
__global__ __launch_bounds__(kPtThreads) void k_transform(const o3dr_point* __restrict__ in, int64_t n, Mat34 T,
                                                          o3dr_point* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kPtThreads + threadIdx.x;
    if (i >= n) return;
    const uint4 v = reinterpret_cast<const uint4*>(in)[i];
    const float x = __uint_as_float(v.x), y = __uint_as_float(v.y), z = __uint_as_float(v.z);
    float X, Y, Z;
    a2_apply(T.m, x, y, z, X, Y, Z);
    reinterpret_cast<uint4*>(out)[i] = make_uint4(__float_as_uint(X), __float_as_uint(Y), __float_as_uint(Z), v.w);
}
