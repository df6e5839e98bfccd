// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Rigid core: what every operator that fits a rigid transform to point pairs shares on the device (DESIGN.md "Rigid
// core").  The record, its solve (rigid_solve) and splitmix64 are in o3dr_rigid_solve.h, shared with the host.
//   A pair is used when both points are finite (pair_finite) and the caller's own gates pass.  A used pair adds the 16
//   moments about c0 (rigid_moments) or its squared residual at T (rigid_residual2); an unused one adds zeros.
//   THE REDUCTION TREE of every such sum: a run of 256 pairs = four waves; per field a wave butterfly (wave_sum_f64)
//   into rd[field][wave] (wave_fields), a barrier, then (w0 + w1) + (w2 + w3) (tree4).  The runs' partials are folded
//   either left to right by one lane per field (k_pose_chain, k_graph_moments) or by fold_partials (k_icp_fold,
//   k_rigid_fold).  draw3: the three local indices of a RANSAC hypothesis.
// =================================================================================================
constexpr int kRigidFoldThreads = 1024;  // fold_partials' workgroup

__device__ __forceinline__ bool pair_finite(const float4& s, const float4& t)
{
    return isfinite(s.x) && isfinite(s.y) && isfinite(s.z) && isfinite(t.x) && isfinite(t.y) && isfinite(t.z);
}

// v[RIGID_N .. kRigidFields) of one pair: count, a, b, a b^T with a = s - c0, b = t - c0 (all zero when not used)
__device__ __forceinline__ void rigid_moments(bool used, const float4& s, const float4& t, const double c0[3], double* v)
{
    const double ax = used ? (double)s.x - c0[0] : 0.0, ay = used ? (double)s.y - c0[1] : 0.0, az = used ? (double)s.z - c0[2] : 0.0;
    const double bx = used ? (double)t.x - c0[0] : 0.0, by = used ? (double)t.y - c0[1] : 0.0, bz = used ? (double)t.z - c0[2] : 0.0;
    v[RIGID_N] = used ? 1.0 : 0.0;
    v[RIGID_SA] = ax, v[RIGID_SA + 1] = ay, v[RIGID_SA + 2] = az;
    v[RIGID_SB] = bx, v[RIGID_SB + 1] = by, v[RIGID_SB + 2] = bz;
    v[RIGID_SAB] = ax * bx, v[RIGID_SAB + 1] = ax * by, v[RIGID_SAB + 2] = ax * bz;
    v[RIGID_SAB + 3] = ay * bx, v[RIGID_SAB + 4] = ay * by, v[RIGID_SAB + 5] = ay * bz;
    v[RIGID_SAB + 6] = az * bx, v[RIGID_SAB + 7] = az * by, v[RIGID_SAB + 8] = az * bz;
}

// |T s - t|^2 with T 3 x 4 row-major
__device__ __forceinline__ double rigid_residual2(const double* T, const float4& s, const float4& t)
{
    const double sx = s.x, sy = s.y, sz = s.z;
    const double ex = ((T[0] * sx + T[1] * sy) + T[2] * sz) + T[3] - (double)t.x;
    const double ey = ((T[4] * sx + T[5] * sy) + T[6] * sz) + T[7] - (double)t.y;
    const double ez = ((T[8] * sx + T[9] * sy) + T[10] * sz) + T[11] - (double)t.z;
    return (ex * ex + ey * ey) + ez * ez;
}

// the wave's sum of each of F fields -> rd[field][wv]; the caller's barrier follows
template <int F, int W>
__device__ __forceinline__ void wave_fields(const double* v, double (*rd)[W], int lane, int wv)
{
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const double x = wave_sum_f64(v[f]);
        if (lane == 0) rd[f][wv] = x;
    }
}
__device__ __forceinline__ double tree4(const double* w) { return (w[0] + w[1]) + (w[2] + w[3]); }

// a workgroup of kRigidFoldThreads folds row[0 .. n): thread t adds entries t, t + 1024, .. in order, a wave butterfly, one
// slot of red[16] per wave, the slots added in order.  The sum is thread 0's return value (0 in every other thread)
__device__ __forceinline__ double fold_partials(const double* row, uint32_t n, double* red)
{
    double s = 0.0;
    for (uint32_t b = threadIdx.x; b < n; b += kRigidFoldThreads) s += row[b];
    s = wave_sum_f64(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int j = 0; j < kRigidFoldThreads / kWave; ++j) t += red[j];
    return t;
}

// the three local indices (0 .. m-1) of hypothesis h of the stream S = splitmix64(seed ^ key)
__device__ __forceinline__ void draw3(uint64_t S, uint32_t h, uint32_t m, uint32_t loc[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint64_t r = splitmix64(S + 3ull * (uint64_t)h + (uint64_t)k);
        loc[k] = (uint32_t)(((r >> 32) * (uint64_t)m) >> 32);
    }
}
