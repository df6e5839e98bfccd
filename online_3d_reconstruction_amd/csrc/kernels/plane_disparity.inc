// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Plane-fitted disparity per segment label (--use_segment_labels; contract: include/o3dr.h, DESIGN.md
// "Plane-fitted disparity").  Three steps: exact integer sums per (frame, label), one fp64 fit per (frame, label), the
// f64 image.  Every sum is an integer add, so nothing below depends on the launch geometry or on arrival order.
// =================================================================================================
constexpr int kPdRun = 16;                     // consecutive pixels of one row a lane walks with its sums in registers
constexpr int kPdTileX = 128, kPdTileY = 32;   // pixels per workgroup: 8 lanes per row, 32 rows
constexpr int kPdSlots = 256;                  // labels a workgroup keeps in LDS (direct-mapped by label % 256)
constexpr uint32_t kPdNoLabel = 0xffffffffu;   // empty slot / a pixel whose label is out of range
constexpr int kPdEvalIter = 4;                 // pixel pairs per lane of the evaluate pass
static_assert(kPdTileX / kPdRun * kPdTileY == 256 && kPdSlots == 256, "one lane per run, one lane per slot");

// one lane's run: pixels of one row with one label (y is constant, so the y sums follow from these at the flush)
struct PdRun {
    uint32_t cnt, n, sx, sxx, sd, sxd, sdd;  // 16 pixels, x < 8192, d < 256: sxx < 2^30
};

// adds a run into the workgroup's slot for `lab`, or, when another label holds that slot, straight into the table
__device__ __forceinline__ void pd_flush(const PdRun& r, uint32_t lab, uint32_t y, uint32_t* tag, unsigned long long* sums,
                                         unsigned long long* table_f)
{
    if (lab == kPdNoLabel || r.cnt == 0) return;
    const unsigned long long Y = y;
    const unsigned long long v[kPdSums] = {r.n, r.sx,  r.n * Y,  r.sxx, r.sx * Y, r.n * Y * Y,
                                           r.sd, r.sxd, r.sd * Y, r.sdd, r.cnt};
    const uint32_t slot = lab % kPdSlots;
    const uint32_t prev = atomicCAS(&tag[slot], kPdNoLabel, lab);
    if (prev == kPdNoLabel || prev == lab) {
        unsigned long long* dst = sums + slot * kPdSums;
#pragma unroll
        for (int k = 0; k < kPdSums; ++k)
            if (v[k]) atomicAdd(dst + k, v[k]);
    } else {
        unsigned long long* dst = table_f + (size_t)lab * kPdSums;
#pragma unroll
        for (int k = 0; k < kPdSums; ++k)
            if (v[k]) atomicAdd(dst + k, v[k]);
    }
}

// LT: the label element (u8, u16, u32).  vec: every row of both images starts on a 16-byte boundary, so a full run is
// read with 16-byte loads.  thr: d participates iff (int)d > thr.  flag: bit 0 set when a label >= n_labels was seen.
template <typename LT>
__global__ __launch_bounds__(256) void k_pd_accumulate(const uint8_t* __restrict__ disp, int64_t dpitch, int64_t dfs,
                                                       const uint8_t* __restrict__ labels, int64_t lpitch, int64_t lfs, int rows,
                                                       int cols, uint32_t n_labels, int thr, int tiles_x, int vec,
                                                       unsigned long long* __restrict__ table, uint32_t* __restrict__ flag)
{
    __shared__ uint32_t tag[kPdSlots];
    __shared__ unsigned long long sums[kPdSlots * kPdSums];
    const int tid = threadIdx.x, f = blockIdx.y;
    tag[tid] = kPdNoLabel;
#pragma unroll
    for (int k = 0; k < kPdSums; ++k) sums[k * kPdSlots + tid] = 0;
    __syncthreads();
    const int ty = (int)blockIdx.x / tiles_x, tx = (int)blockIdx.x - ty * tiles_x;
    const int y = ty * kPdTileY + tid / (kPdTileX / kPdRun), x0 = tx * kPdTileX + (tid % (kPdTileX / kPdRun)) * kPdRun;
    unsigned long long* table_f = table + (size_t)f * n_labels * kPdSums;
    if (y < rows && x0 < cols) {
        const uint8_t* drow = disp + (int64_t)f * dfs + (int64_t)y * dpitch + x0;
        const LT* lrow = reinterpret_cast<const LT*>(labels + (int64_t)f * lfs + (int64_t)y * lpitch) + x0;
        const int m = cols - x0 < kPdRun ? cols - x0 : kPdRun;
        alignas(16) uint8_t dv[kPdRun];
        alignas(16) LT lv[kPdRun];
        if (vec && m == kPdRun) {
            *reinterpret_cast<uint4*>(dv) = *reinterpret_cast<const uint4*>(drow);
#pragma unroll
            for (int q = 0; q < (int)sizeof(LT); ++q)
                reinterpret_cast<uint4*>(lv)[q] = reinterpret_cast<const uint4*>(lrow)[q];
        } else {
#pragma unroll
            for (int i = 0; i < kPdRun; ++i) {
                dv[i] = i < m ? drow[i] : (uint8_t)0;
                lv[i] = i < m ? lrow[i] : (LT)0;
            }
        }
        PdRun r = {0, 0, 0, 0, 0, 0, 0};
        uint32_t cur = kPdNoLabel;
        bool bad = false;
#pragma unroll
        for (int i = 0; i < kPdRun; ++i) {
            if (i < m) {
                uint32_t lab = (uint32_t)lv[i];
                if (lab >= n_labels) {
                    bad = true;
                    lab = kPdNoLabel;
                }
                if (lab != cur) {
                    pd_flush(r, cur, (uint32_t)y, tag, sums, table_f);
                    r = PdRun{0, 0, 0, 0, 0, 0, 0};
                    cur = lab;
                }
                const uint32_t d = dv[i], x = (uint32_t)(x0 + i);
                r.cnt += 1;
                if ((int)d > thr) {
                    r.n += 1;
                    r.sx += x;
                    r.sxx += x * x;
                    r.sd += d;
                    r.sxd += x * d;
                    r.sdd += d * d;
                }
            }
        }
        pd_flush(r, cur, (uint32_t)y, tag, sums, table_f);
        if (bad) atomicOr(flag, 1u);
    }
    __syncthreads();
    const uint32_t lab = tag[tid];
    if (lab != kPdNoLabel) {
        unsigned long long* dst = table_f + (size_t)lab * kPdSums;
#pragma unroll
        for (int k = 0; k < kPdSums; ++k) {
            const unsigned long long v = sums[tid * kPdSums + k];
            if (v) atomicAdd(dst + k, v);
        }
    }
}

// the fit of include/o3dr.h step 3 and 4, operation by operation (the library is built with -ffp-contract=off)
__global__ __launch_bounds__(256) void k_pd_fit(const unsigned long long* __restrict__ table, int64_t n_rec, int min_pixels,
                                                double max_mse, o3dr_plane_disp_segment* __restrict__ rec)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rec) return;
    const unsigned long long* s = table + i * kPdSums;
    o3dr_plane_disp_segment r;
    r.a = r.b = r.c0 = r.mx = r.my = r.mse = 0.0;
    r.n_pixels = (uint32_t)s[10];
    r.n = (uint32_t)s[0];
    r.status = O3DR_PLANE_DISP_NONE;
    r.reserved = 0;
    if (s[0] != 0) {
        const double n = (double)s[0], Sx = (double)s[1], Sy = (double)s[2], Sxx = (double)s[3], Sxy = (double)s[4],
                     Syy = (double)s[5], Sd = (double)s[6], Sxd = (double)s[7], Syd = (double)s[8], Sdd = (double)s[9];
        const double mx = Sx / n, my = Sy / n, c0 = Sd / n;
        const double cxx = Sxx - Sx * mx, cxy = Sxy - Sx * my, cyy = Syy - Sy * my;
        const double cxd = Sxd - Sd * mx, cyd = Syd - Sd * my, cdd = Sdd - Sd * c0;
        const double det = cxx * cyy - cxy * cxy;
        const bool degenerate = det <= (O3DR_PLANE_DISP_TOL * cxx) * cyy;
        double a = 0.0, b = 0.0;
        r.status = O3DR_PLANE_DISP_MEAN;
        if (!((long long)s[0] < (long long)min_pixels) && !degenerate) {
            a = (cxd * cyy - cyd * cxy) / det;
            b = (cyd * cxx - cxd * cxy) / det;
            r.status = O3DR_PLANE_DISP_PLANE;
        }
        const double mse = ((cdd - a * cxd) - b * cyd) / n;
        if (max_mse > 0.0 && mse > max_mse) r.status = O3DR_PLANE_DISP_NONE;
        r.a = a;
        r.b = b;
        r.c0 = c0;
        r.mx = mx;
        r.my = my;
        r.mse = mse;
    }
    rec[i] = r;
}

// One lane writes pairs of consecutive pixels of a frame's dense f64 image with 16-byte stores: pair q covers the pixels
// 2q - lead and 2q - lead + 1, lead = 1 when the frame's first pixel sits 8 bytes past a 16-byte boundary.
template <typename LT>
__global__ __launch_bounds__(256) void k_pd_evaluate(const uint8_t* __restrict__ disp, int64_t dpitch, int64_t dfs,
                                                     const uint8_t* __restrict__ labels, int64_t lpitch, int64_t lfs, int rows,
                                                     int cols, uint32_t n_labels, int thr, int fill,
                                                     const o3dr_plane_disp_segment* __restrict__ rec, double* __restrict__ out)
{
    const int f = blockIdx.y;
    const int64_t npix = (int64_t)rows * cols;
    double* of = out + (int64_t)f * npix;
    const int64_t lead = (int64_t)((reinterpret_cast<uintptr_t>(of) >> 3) & 1);
    const uint8_t* df = disp + (int64_t)f * dfs;
    const uint8_t* lf = labels + (int64_t)f * lfs;
    const o3dr_plane_disp_segment* rf = rec + (int64_t)f * n_labels;
    uint32_t c_lab = kPdNoLabel;  // the coefficients of the label this lane saw last
    int c_status = O3DR_PLANE_DISP_NONE;
    double a = 0, b = 0, c0 = 0, mx = 0, my = 0;
    auto value = [&](int64_t p) -> double {
        const uint32_t y = (uint32_t)p / (uint32_t)cols, x = (uint32_t)p - y * (uint32_t)cols;
        const uint32_t d = df[(int64_t)y * dpitch + x];
        const uint32_t lab = (uint32_t) reinterpret_cast<const LT*>(lf + (int64_t)y * lpitch)[x];
        if (lab >= n_labels) return (double)d;
        if (lab != c_lab) {
            const o3dr_plane_disp_segment* r = rf + lab;
            c_lab = lab;
            c_status = r->status;
            a = r->a, b = r->b, c0 = r->c0, mx = r->mx, my = r->my;
        }
        if (c_status == O3DR_PLANE_DISP_NONE || (!fill && !((int)d > thr))) return (double)d;
        return (c0 + a * ((double)x - mx)) + b * ((double)y - my);
    };
    int64_t q = (int64_t)blockIdx.x * (256 * kPdEvalIter) + threadIdx.x;
#pragma unroll
    for (int it = 0; it < kPdEvalIter; ++it, q += 256) {
        const int64_t p0 = 2 * q - lead, p1 = p0 + 1;
        const bool ok0 = p0 >= 0 && p0 < npix, ok1 = p1 < npix;
        double v0 = 0, v1 = 0;
        if (ok0) v0 = value(p0);
        if (ok1) v1 = value(p1);
        if (ok0 && ok1)
            *reinterpret_cast<double2*>(of + p0) = make_double2(v0, v1);
        else if (ok0)
            of[p0] = v0;
        else if (ok1)
            of[p1] = v1;
    }
}
