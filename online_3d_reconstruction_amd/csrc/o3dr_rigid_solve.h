// libo3dr internal: the rigid fit's record, its Kabsch solve and the samplers' generator, stated once for host and device.
// A plain header: no HIP type or header, so it also compiles with a host C++17 compiler alone (tests/rigid_solve_main.cpp).
// Callers: o3dr_icp_align and o3dr_estimate_rigid_transform on the host, k_pose_chain on the device (rigid_solve);
// o3dr_orb_pattern on the host, the plane and rigid RANSACs on the device (splitmix64).  DESIGN.md "Rigid core".
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define O3DR_HD __host__ __device__
#else
#define O3DR_HD
#endif

namespace o3dr {

// "the 16 fp64 moments of o3dr_estimate_rigid_transform step 2", about a centre c0: a = src - c0, b = tgt - c0
enum : int {
    RIGID_N = 0,        // count of used pairs
    RIGID_SA = 1,       // sum a (3)
    RIGID_SB = 4,       // sum b (3)
    RIGID_SAB = 7,      // sum a b^T (9, row-major)
    kRigidFields = 16,
};

// the generator of every sampler (o3dr_segment_plane step 2, o3dr_ransac_rigid step 2, the ORB pattern)
O3DR_HD inline uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// one-sided Jacobi SVD of a 3x3 matrix: A = U diag(S) V^T, S descending (stable for equal norms: the insertion sort
// orders every tie pattern of three norms as std::sort does); U's first two columns (the third is not needed)
O3DR_HD inline void rigid_svd3(const double A_in[3][3], double U[3][3], double S[3], double V[3][3])
{
    double A[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) A[i][j] = A_in[i][j], V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int i = 0; i < 3; ++i) {
                    alpha += A[i][p] * A[i][p];
                    beta += A[i][q] * A[i][q];
                    gamma += A[i][p] * A[i][q];
                }
                if (!(fabs(gamma) > 1e-15 * sqrt(alpha * beta))) continue;
                rotated = true;
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int i = 0; i < 3; ++i) {
                    const double ap = A[i][p], aq = A[i][q];
                    A[i][p] = cs * ap - sn * aq;
                    A[i][q] = sn * ap + cs * aq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = cs * vp - sn * vq;
                    V[i][q] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
    int order[3] = {0, 1, 2};
    double nrm[3];
    for (int j = 0; j < 3; ++j) nrm[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
    for (int k = 1; k < 3; ++k)  // insertion sort, descending
        for (int m = k; m > 0 && nrm[order[m]] > nrm[order[m - 1]]; --m) {
            const int t = order[m];
            order[m] = order[m - 1];
            order[m - 1] = t;
        }
    double Vs[3][3];
    for (int k = 0; k < 3; ++k) {
        const int j = order[k];
        S[k] = nrm[j];
        for (int i = 0; i < 3; ++i) {
            Vs[i][k] = V[i][j];
            U[i][k] = nrm[j] > 0.0 ? A[i][j] / nrm[j] : 0.0;
        }
    }
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) V[i][k] = Vs[i][k];
}

// T (3 x 4, row-major) from a record of moments about c0: R = V diag(1, 1, d) U^T, t = mu_b - R mu_a
// (pcl::registration::TransformationEstimationSVD with the reflection corrected); false: cross-covariance of rank < 2
O3DR_HD inline bool rigid_solve(const double* rec, const double c0[3], double T[12])
{
    const double n = rec[RIGID_N];
    double ma[3], mb[3], H[3][3];
    for (int k = 0; k < 3; ++k) ma[k] = rec[RIGID_SA + k] / n, mb[k] = rec[RIGID_SB + k] / n;
    for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) H[j][k] = rec[RIGID_SAB + 3 * j + k] - n * ma[j] * mb[k];
    double U[3][3], S[3], V[3][3];
    rigid_svd3(H, U, S, V);
    if (!(S[0] > 0.0) || !isfinite(S[0]) || !(S[1] > 1e-12 * S[0])) return false;
    // U's third column as u1 x u2 (det U = +1): then d = det(V) gives the proper rotation
    U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
    U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
    U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    const double detV = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                        V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
    const double d[3] = {1.0, 1.0, detV < 0.0 ? -1.0 : 1.0};
    double R[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = V[i][0] * d[0] * U[j][0] + V[i][1] * d[1] * U[j][1] + V[i][2] * d[2] * U[j][2];
    for (int i = 0; i < 3; ++i) {
        double t = c0[i] + mb[i];
        for (int j = 0; j < 3; ++j) t -= R[i][j] * (c0[j] + ma[j]);
        for (int j = 0; j < 3; ++j) T[4 * i + j] = R[i][j];
        T[4 * i + 3] = t;
    }
    return isfinite(T[3]) && isfinite(T[7]) && isfinite(T[11]);
}

}  // namespace o3dr
