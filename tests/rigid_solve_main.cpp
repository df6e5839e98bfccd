// Stand-alone host program for online_3d_reconstruction_amd/csrc/o3dr_rigid_solve.h (tests/test_rigid_solve_host.py builds it
// with g++ and no HIP header).  It prints, for a fixed list of records, the record and c0 it passed to rigid_solve and the
// return value and T it got, every double as its 64 bits in hex; then it checks that the solve's insertion sort orders all
// 27 tie patterns of three norms as std::sort does with the same comparator.  tests/rigid_core_reference.py recomputes every
// printed T from the printed record.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>

#include "o3dr_rigid_solve.h"

using namespace o3dr;

static void hex(double v)
{
    uint64_t u;
    memcpy(&u, &v, 8);
    printf(" %016llx", (unsigned long long)u);
}

// the record of n pairs about c0, summed in index order (the order is this program's own: the test reads the record back)
static void moments(const double (*s)[3], const double (*t)[3], int n, const double c0[3], double rec[kRigidFields])
{
    for (int k = 0; k < kRigidFields; ++k) rec[k] = 0.0;
    for (int i = 0; i < n; ++i) {
        double a[3], b[3];
        for (int k = 0; k < 3; ++k) a[k] = s[i][k] - c0[k], b[k] = t[i][k] - c0[k];
        rec[RIGID_N] += 1.0;
        for (int k = 0; k < 3; ++k) rec[RIGID_SA + k] += a[k], rec[RIGID_SB + k] += b[k];
        for (int j = 0; j < 3; ++j)
            for (int k = 0; k < 3; ++k) rec[RIGID_SAB + 3 * j + k] += a[j] * b[k];
    }
}

static void run(const char* name, const double rec[kRigidFields], const double c0[3])
{
    double T[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const bool ok = rigid_solve(rec, c0, T);
    printf("case %s rec", name);
    for (int k = 0; k < kRigidFields; ++k) hex(rec[k]);
    for (int k = 0; k < 3; ++k) hex(c0[k]);
    printf(" ret %d T", ok ? 1 : 0);
    for (int k = 0; k < 12; ++k) hex(T[k]);
    printf("\n");
}

// out = R s + t
static void move(const double (*s)[3], int n, const double R[3][3], const double t[3], double (*out)[3])
{
    for (int i = 0; i < n; ++i)
        for (int r = 0; r < 3; ++r) out[i][r] = ((R[r][0] * s[i][0] + R[r][1] * s[i][1]) + R[r][2] * s[i][2]) + t[r];
}

static int order_check()
{
    int bad = 0;
    for (int p = 0; p < 27; ++p) {
        const double nrm[3] = {(double)(p % 3), (double)(p / 3 % 3), (double)(p / 9)};
        int ref[3] = {0, 1, 2}, order[3] = {0, 1, 2};
        std::sort(ref, ref + 3, [&](int a, int b) { return nrm[a] > nrm[b]; });
        for (int k = 1; k < 3; ++k)  // rigid_svd3's insertion sort
            for (int m = k; m > 0 && nrm[order[m]] > nrm[order[m - 1]]; --m) std::swap(order[m], order[m - 1]);
        // through the solve itself: A = diag(nrm) needs no rotation, so S and V's columns come out in the sort's order
        const double A[3][3] = {{nrm[0], 0.0, 0.0}, {0.0, nrm[1], 0.0}, {0.0, 0.0, nrm[2]}};
        double U[3][3], S[3], V[3][3];
        rigid_svd3(A, U, S, V);
        for (int k = 0; k < 3; ++k)
            if (order[k] != ref[k] || S[k] != nrm[ref[k]] || V[ref[k]][k] != 1.0) ++bad;
    }
    return bad;
}

int main()
{
    const double src[6][3] = {{0.25, -1.5, 2.0}, {1.75, 0.5, 3.25}, {-2.0, 1.0, 4.5}, {0.5, 2.25, 2.75}, {-1.25, -0.75, 5.0}, {3.0, 0.125, 3.5}};
    const double c = 0.8, s = 0.6;  // an exact rotation: 0.8^2 + 0.6^2 rounds to 1
    const double Rz[3][3] = {{c, -s, 0.0}, {s, c, 0.0}, {0.0, 0.0, 1.0}};
    const double Rg[3][3] = {{0.36, 0.48, -0.8}, {-0.8, 0.6, 0.0}, {0.48, 0.64, 0.6}};
    const double I[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    const double t1[3] = {0.5, -0.25, 0.125}, t0[3] = {0.0, 0.0, 0.0};
    double tgt[6][3], rec[kRigidFields];

    move(src, 6, Rg, t1, tgt);  // a generic motion
    moments(src, tgt, 6, tgt[0], rec);
    run("generic", rec, tgt[0]);
    double nan_rec[kRigidFields];  // the same record with one NaN moment
    memcpy(nan_rec, rec, sizeof rec);
    nan_rec[RIGID_SAB + 1] = std::numeric_limits<double>::quiet_NaN();
    run("nan_moment", nan_rec, tgt[0]);
    moments(src, tgt, 3, tgt[0], rec);  // n = 3
    run("n3", rec, tgt[0]);

    move(src, 6, I, t1, tgt);  // a pure translation
    moments(src, tgt, 6, tgt[0], rec);
    run("translation", rec, tgt[0]);

    // coplanar pairs (z = 0) mirrored inside their plane: the SVD's V has det < 0 and the third column is corrected
    const double flat[5][3] = {{1.0, 0.5, 0.0}, {-2.0, 1.5, 0.0}, {0.75, -1.25, 0.0}, {2.5, 2.0, 0.0}, {-0.5, -2.0, 0.0}};
    double mir[5][3];
    for (int i = 0; i < 5; ++i) mir[i][0] = -flat[i][0] + 0.5, mir[i][1] = flat[i][1] - 0.25, mir[i][2] = 0.125;
    moments(flat, mir, 5, mir[0], rec);
    run("coplanar_reflection", rec, mir[0]);

    const double line[4][3] = {{0.0, 0.0, 0.0}, {1.0, 2.0, 3.0}, {2.0, 4.0, 6.0}, {-1.5, -3.0, -4.5}};  // rank 1
    double lt[4][3];
    move(line, 4, Rz, t1, lt);
    moments(line, lt, 4, lt[0], rec);
    run("collinear_rank1", rec, lt[0]);

    const double same[3][3] = {{1.0, 2.0, 3.0}, {1.0, 2.0, 3.0}, {1.0, 2.0, 3.0}};  // rank 0
    moments(same, same, 3, same[0], rec);
    run("rank0", rec, same[0]);

    // axis pairs: H = diag(2, 2, 0.5) and diag(2, 2, 2) about the origin (equal column norms: the sort's ties)
    const double two[6][3] = {{1.0, 0.0, 0.0}, {-1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, -1.0, 0.0}, {0.0, 0.0, 0.5}, {0.0, 0.0, -0.5}};
    moments(two, two, 6, t0, rec);
    run("two_equal_singular", rec, t0);
    double twot[6][3];
    move(two, 6, Rz, t1, twot);
    moments(two, twot, 6, t0, rec);
    run("two_equal_singular_moved", rec, t0);
    const double three[6][3] = {{1.0, 0.0, 0.0}, {-1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, -1.0, 0.0}, {0.0, 0.0, 1.0}, {0.0, 0.0, -1.0}};
    moments(three, three, 6, t0, rec);
    run("three_equal_singular", rec, t0);
    double threet[6][3];
    move(three, 6, Rg, t1, threet);
    moments(three, threet, 6, t0, rec);
    run("three_equal_singular_moved", rec, t0);

    const int bad = order_check();
    printf("order check: %d of 27 patterns differ from std::sort\n", bad);
    printf("splitmix64 0 %016llx\n", (unsigned long long)splitmix64(0));
    return bad ? 1 : 0;
}
