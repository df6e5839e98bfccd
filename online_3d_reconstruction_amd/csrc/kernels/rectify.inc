// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Stereo rectification: the Q5 fixed-point undistort-rectify map of one camera, and the bilinear remap of a group of
// frames through one map (contract: include/o3dr.h "stereo rectification"; DESIGN.md "Stereo rectification").
//   k_rectify_maps   one thread per destination pixel, fp64: + - * / and floor in the contract's order.  The
//                    translation unit is built with -ffp-contract=off, so no multiply-add is fused; fp64 division is the
//                    correctly rounded one (no reciprocal approximation).  Runs once per camera: not hot.
//   k_rectify_remap  one thread per 4 horizontally adjacent destination pixels.  The 8 map words are loaded once (two
//                    16-byte loads where the address allows), the tap offsets, weights and inside flags derived from them
//                    stay in registers, and the thread then walks the group's frames: gather, blend, one dword store
//                    (channels = 1) or three (channels = 3) where the output address is 4-byte aligned.  All integer.
// All stores are plain vector stores.
// =================================================================================================

__global__ __launch_bounds__(256) void k_rectify_maps(RectMapArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)a.rows_out * a.cols_out;
    if (i >= n) return;
    const double u = (double)(int)(i % a.cols_out), v = (double)(int)(i / a.cols_out);
    const double X = (a.I[0] * u + a.I[1] * v) + a.I[2];
    const double Y = (a.I[3] * u + a.I[4] * v) + a.I[5];
    const double Wc = (a.I[6] * u + a.I[7] * v) + a.I[8];
    const double iw = 1.0 / Wc;
    const double x = X * iw, y = Y * iw;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * (x * y);
    const double k1 = a.k[0], k2 = a.k[1], p1 = a.k[2], p2 = a.k[3], k3 = a.k[4], k4 = a.k[5], k5 = a.k[6], k6 = a.k[7];
    const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
    const double kr = num / den;
    const double xd = (x * kr + p1 * xy2) + p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + p1 * (r2 + 2.0 * y2)) + p2 * xy2;
    const double mx = a.fx * xd + a.cx, my = a.fy * yd + a.cy;
    const double qx = floor(mx * 32.0 + 0.5), qy = floor(my * 32.0 + 0.5);
    // (a NaN fails every comparison)
    const bool in = qx >= -1048576.0 && qx < 1048576.0 && qy >= -1048576.0 && qy < 1048576.0;
    int2 q;
    q.x = in ? (int)qx : O3DR_RECTIFY_OUTSIDE;
    q.y = in ? (int)qy : O3DR_RECTIFY_OUTSIDE;
    a.map[2 * i] = q.x;
    a.map[2 * i + 1] = q.y;
}

// What one destination pixel keeps of its map entry for every frame: the byte offsets of its two tap rows and two tap
// columns inside a frame (clamped into the image, so that every address is one of the image's own), the four weights
// (zero where the tap is outside: `wout` then carries that weight to the border value) and the valid flag.
struct RectTaps {
    int64_t row0, row1;  // y0 * pitch, (y0 + 1) * pitch, clamped
    int32_t col0, col1;  // x0 * channels, (x0 + 1) * channels, clamped
    uint32_t w00, w01, w10, w11, wout;
    bool valid;
};
template <int CH>
__device__ __forceinline__ RectTaps rect_taps(int qx, int qy, int rows, int cols, int64_t pitch)
{
    const int x0 = qx >> 5, y0 = qy >> 5, ax = qx & 31, ay = qy & 31;
    const bool ix0 = x0 >= 0 && x0 < cols, ix1 = x0 + 1 >= 0 && x0 + 1 < cols;
    const bool iy0 = y0 >= 0 && y0 < rows, iy1 = y0 + 1 >= 0 && y0 + 1 < rows;
    const uint32_t w00 = (uint32_t)((32 - ax) * (32 - ay)), w01 = (uint32_t)(ax * (32 - ay));
    const uint32_t w10 = (uint32_t)((32 - ax) * ay), w11 = (uint32_t)(ax * ay);
    RectTaps t;
    t.row0 = (int64_t)min(max(y0, 0), rows - 1) * pitch;
    t.row1 = (int64_t)min(max(y0 + 1, 0), rows - 1) * pitch;
    t.col0 = min(max(x0, 0), cols - 1) * CH;
    t.col1 = min(max(x0 + 1, 0), cols - 1) * CH;
    t.w00 = ix0 && iy0 ? w00 : 0u;
    t.w01 = ix1 && iy0 ? w01 : 0u;
    t.w10 = ix0 && iy1 ? w10 : 0u;
    t.w11 = ix1 && iy1 ? w11 : 0u;
    t.wout = 1024u - (t.w00 + t.w01 + t.w10 + t.w11);  // the weight of the taps outside
    t.valid = t.wout == 0u;
    return t;
}
template <int CH>
__device__ __forceinline__ void rect_blend(const uint8_t* __restrict__ f, const RectTaps& t, uint32_t bias, uint32_t* o)
{
    const uint8_t *p00 = f + t.row0 + t.col0, *p01 = f + t.row0 + t.col1, *p10 = f + t.row1 + t.col0, *p11 = f + t.row1 + t.col1;
#pragma unroll
    for (int c = 0; c < CH; ++c)
        o[c] = (t.w00 * p00[c] + t.w01 * p01[c] + t.w10 * p10[c] + t.w11 * p11[c] + bias) >> 10;
}

template <int CH>
__global__ __launch_bounds__(256) void k_rectify_remap(RectArgs a, int quads_x)
{
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)a.rows_out * quads_x) return;
    const int y = (int)(q / quads_x), x = (int)(q % quads_x) * 4;
    const int n_px = min(4, a.cols_out - x);  // < 4: the row's tail
    const int64_t px0 = (int64_t)y * a.cols_out + x;
    const int32_t* mp = a.map + 2 * px0;
    int m[8];
    if (n_px == 4 && ((uintptr_t)mp & 15) == 0) {
        const int4 lo = *(const int4*)mp, hi = *(const int4*)(mp + 4);
        m[0] = lo.x, m[1] = lo.y, m[2] = lo.z, m[3] = lo.w, m[4] = hi.x, m[5] = hi.y, m[6] = hi.z, m[7] = hi.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool on = k < n_px;  // a pixel past the row's end: a sentinel, never stored
            m[2 * k] = on ? mp[2 * k] : O3DR_RECTIFY_OUTSIDE;
            m[2 * k + 1] = on ? mp[2 * k + 1] : O3DR_RECTIFY_OUTSIDE;
        }
    }
    RectTaps t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = rect_taps<CH>(m[2 * k], m[2 * k + 1], a.rows, a.cols, a.pitch);
    if (a.valid) {
        uint8_t* vp = a.valid + px0;
        if (n_px == 4 && ((uintptr_t)vp & 3) == 0) {
            *(uint32_t*)vp = (uint32_t)t[0].valid | (uint32_t)t[1].valid << 8 | (uint32_t)t[2].valid << 16 | (uint32_t)t[3].valid << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n_px) vp[k] = (uint8_t)t[k].valid;
        }
    }
    uint32_t bias[4];  // the border's share of the sum, and the rounding
#pragma unroll
    for (int k = 0; k < 4; ++k) bias[k] = t[k].wout * (uint32_t)a.border + 512u;

    const int64_t out_frame = (int64_t)a.rows_out * a.cols_out * CH;
    const uint8_t* __restrict__ src = a.src;
    uint8_t* __restrict__ op = a.out + px0 * CH;
    for (int f = 0; f < a.frames; ++f, src += a.fstride, op += out_frame) {
        uint32_t o[4 * CH];
#pragma unroll
        for (int k = 0; k < 4; ++k) rect_blend<CH>(src, t[k], bias[k], o + k * CH);
        if (n_px == 4 && ((uintptr_t)op & 3) == 0) {
#pragma unroll
            for (int w = 0; w < CH; ++w)
                ((uint32_t*)op)[w] = o[4 * w] | o[4 * w + 1] << 8 | o[4 * w + 2] << 16 | o[4 * w + 3] << 24;
        } else {
#pragma unroll
            for (int k = 0; k < 4 * CH; ++k)
                if (k < n_px * CH) op[k] = (uint8_t)o[k];
        }
    }
}
