// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Moving-least-squares smoothing and normals (o3dr_mls_smooth; DESIGN.md "MLS")
//   The cloud's search grid is the nearest-neighbour grid (launch_nn_grid: points in cell order with their original index
//   in .w, exact per-cell boxes, the cloud's box).  ONE LANE PER QUERY, queries taken in the grid's cell order (lane t:
//   grid.xyz[t], results to index .w), so the lanes of a wave share cells.  The neighbours come from the exact radius walk
//   over the window of the query's box (grid_radius_walk, util.inc: the clustering shares it).  Pass 1: k and the fp64
//   moments about the query; a fixed-sweep 3x3 Jacobi; pass 2 (polynomial fit): the weighted moments sum w u^a v^b (a + b <= 2 order) and sum w f u^a v^b; a
//   Cholesky solve and the epilogue.  Sums run over the window's cells row by row, points in cell order: no atomics
//   but the integer counters of the result.
// =================================================================================================
constexpr int kMlsThreads = 256;

struct MlsArgs {
    const o3dr_point* cloud;  // n points in the caller's order (colours are read here)
    uint32_t n;
    SearchGrid grid;          // the cloud's
    float r2;                 // (float)(r * r)
    double r, inv_h;          // search radius; 1 / sqr_gauss_param
    float pad_r;              // grid_pad_radius(r): half the side of the query's box
    o3dr_point* out;          // n (may be cloud)
    float* normals;           // 4 n (nx ny nz curvature) or nullptr
    uint32_t* nn_count;       // n or nullptr
    uint8_t* fit;             // n or nullptr
    unsigned long long* counters;  // n_none, n_plane, n_poly, max k
};

template <int O>
__global__ __launch_bounds__(kMlsThreads) void k_mls(MlsArgs a)
{
    const int64_t t = (int64_t)blockIdx.x * kMlsThreads + threadIdx.x;
    const bool valid = t < (int64_t)a.n;
    int kind = -1;
    uint32_t k = 0;
    if (valid) {
        const SorGeom g = *a.grid.geom;
        const float4 q = a.grid.xyz[t];
        const uint32_t idx = __float_as_uint(q.w);
        // pass 1: k and the moments about the query
        double s1[3] = {0.0, 0.0, 0.0}, s2[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        grid_radius_walk(a.grid, g, q, a.pad_r, a.r2, [&](const float4& p, float) {
            const double ex = (double)p.x - (double)q.x, ey = (double)p.y - (double)q.y, ez = (double)p.z - (double)q.z;
            ++k;
            s1[0] += ex, s1[1] += ey, s1[2] += ez;
            s2[0] += ex * ex, s2[1] += ex * ey, s2[2] += ex * ez;
            s2[3] += ey * ey, s2[4] += ey * ez, s2[5] += ez * ez;
        });
        const double inv_k = k ? 1.0 / (double)k : 0.0;
        const double mx = s1[0] * inv_k, my = s1[1] * inv_k, mz = s1[2] * inv_k;  // centroid - query
        double A[3][3], V[3][3];
        A[0][0] = s2[0] * inv_k - mx * mx, A[0][1] = s2[1] * inv_k - mx * my, A[0][2] = s2[2] * inv_k - mx * mz;
        A[1][1] = s2[3] * inv_k - my * my, A[1][2] = s2[4] * inv_k - my * mz, A[2][2] = s2[5] * inv_k - mz * mz;
        mls_jacobi3(A, V);
        // ascending eigenvalues (ties keep the lower column); selects, not indexing: V stays in registers
        const double d0 = A[0][0], d1 = A[1][1], d2 = A[2][2];
        int i0 = 0, i1 = 1, i2 = 2;
        auto ev = [&](int i) { return i == 0 ? d0 : (i == 1 ? d1 : d2); };
        if (ev(i1) < ev(i0)) { const int s = i0; i0 = i1; i1 = s; }
        if (ev(i2) < ev(i1)) { const int s = i1; i1 = i2; i2 = s; }
        if (ev(i1) < ev(i0)) { const int s = i0; i0 = i1; i1 = s; }
        const double l0 = ev(i0), l1 = ev(i1), l2 = ev(i2);
        const o3dr_point src = a.cloud[idx];  // read before the write below: in-place calls are safe
        o3dr_point o = src;
        float nrm[4] = {__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
        if (k < 3 || !(l1 > 1e-12 * l2)) {
            kind = O3DR_MLS_NONE;
        } else {
            double nx = i0 == 0 ? V[0][0] : (i0 == 1 ? V[0][1] : V[0][2]);
            double ny = i0 == 0 ? V[1][0] : (i0 == 1 ? V[1][1] : V[1][2]);
            double nz = i0 == 0 ? V[2][0] : (i0 == 1 ? V[2][1] : V[2][2]);
            const double nl = 1.0 / sqrt(nx * nx + ny * ny + nz * nz);
            nx *= nl, ny *= nl, nz *= nl;
            if (nz < 0.0 || (nz == 0.0 && (ny < 0.0 || (ny == 0.0 && nx < 0.0)))) nx = -nx, ny = -ny, nz = -nz;
            const double tr = l0 + l1 + l2;
            const double curv = tr != 0.0 ? l0 / tr : 0.0;
            // projection of the query onto the plane: m = p - (n . (p - c)) n, with p - c = -(mx, my, mz)
            const double dn = -(nx * mx + ny * my + nz * mz);
            const double px = (double)q.x - dn * nx, py = (double)q.y - dn * ny, pz = (double)q.z - dn * nz;
            double a0 = 0.0, au = 0.0, av = 0.0;
            kind = O3DR_MLS_PLANE;
            double ux = 0.0, uy = 0.0, uz = 0.0, vx = 0.0, vy = 0.0, vz = 0.0;
            if constexpr (O >= 1) {
                constexpr int nc = (O + 1) * (O + 2) / 2;
                constexpr int D = 2 * O, ns = (D + 1) * (D + 2) / 2;
                if (k >= (uint32_t)nc) {
                    // local frame
                    if (fabs(nz) <= 0.9) vx = -ny, vy = nx, vz = 0.0;
                    else vx = 0.0, vy = -nz, vz = ny;
                    const double vl = 1.0 / sqrt(vx * vx + vy * vy + vz * vz);
                    vx *= vl, vy *= vl, vz *= vl;
                    ux = ny * vz - nz * vy, uy = nz * vx - nx * vz, uz = nx * vy - ny * vx;
                    // pass 2: S[(a, b)] = sum w u^a v^b (a + b <= D), F[(a, b)] = sum w f u^a v^b (a + b <= O)
                    double S[ns], Fv[nc];
#pragma unroll
                    for (int m = 0; m < ns; ++m) S[m] = 0.0;
#pragma unroll
                    for (int m = 0; m < nc; ++m) Fv[m] = 0.0;
                    const double inv_r = 1.0 / a.r, inv_h = a.inv_h;
                    grid_radius_walk(a.grid, g, q, a.pad_r, a.r2, [&](const float4& p, float d) {
                        const double ex = (double)p.x - px, ey = (double)p.y - py, ez = (double)p.z - pz;
                        const double u = (ex * ux + ey * uy + ez * uz) * inv_r, v = (ex * vx + ey * vy + ez * vz) * inv_r;
                        const double f = ex * nx + ey * ny + ez * nz;
                        const double w = exp(-(double)d * inv_h);
                        double upow = w;
                        int m = 0, mf = 0;
#pragma unroll
                        for (int ea = 0; ea <= D; ++ea) {
                            double term = upow;
#pragma unroll
                            for (int eb = 0; eb <= D - ea; ++eb) {
                                S[m++] += term;
                                if (ea + eb <= O) Fv[mf++] += term * f;
                                term *= v;
                            }
                            upow *= u;
                        }
                    });
                    // the normal matrix M[i][j] = S[a_i + a_j, b_i + b_j] over the monomials u^a v^b (a outer, b inner)
                    int ma[nc], mb[nc];
                    {
                        int m = 0;
#pragma unroll
                        for (int ea = 0; ea <= O; ++ea)
#pragma unroll
                            for (int eb = 0; eb <= O - ea; ++eb) ma[m] = ea, mb[m] = eb, ++m;
                    }
                    auto sidx = [](int ea, int eb) { return ea * (D + 1) - ea * (ea - 1) / 2 + eb; };
                    double L[nc][nc], c[nc];
                    double dmax = 0.0;
#pragma unroll
                    for (int i = 0; i < nc; ++i) dmax = fmax(dmax, S[sidx(2 * ma[i], 2 * mb[i])]);
                    bool ok = true;
#pragma unroll
                    for (int i = 0; i < nc; ++i) {
#pragma unroll
                        for (int j = 0; j <= i; ++j) {
                            double s = S[sidx(ma[i] + ma[j], mb[i] + mb[j])];
#pragma unroll
                            for (int l = 0; l < j; ++l) s -= L[i][l] * L[j][l];
                            if (i == j) {
                                ok = ok && s > 1e-12 * dmax;
                                L[i][i] = sqrt(fmax(s, 0.0));
                            } else {
                                L[i][j] = L[j][j] > 0.0 ? s / L[j][j] : 0.0;
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < nc; ++i) {  // L y = F
                        double s = Fv[i];
#pragma unroll
                        for (int l = 0; l < i; ++l) s -= L[i][l] * c[l];
                        c[i] = s / L[i][i];
                    }
#pragma unroll
                    for (int i = nc - 1; i >= 0; --i) {  // L^T c = y
                        double s = c[i];
#pragma unroll
                        for (int l = i + 1; l < nc; ++l) s -= L[l][i] * c[l];
                        c[i] = s / L[i][i];
                    }
#pragma unroll
                    for (int i = 0; i < nc; ++i) ok = ok && isfinite(c[i]);
                    if (ok) {
                        kind = O3DR_MLS_POLY;
                        a0 = c[0], av = c[1] * inv_r, au = c[O + 1] * inv_r;
                    }
                }
            }
            double ox = px, oy = py, oz = pz, qnx = nx, qny = ny, qnz = nz;
            if (kind == O3DR_MLS_POLY) {
                ox += a0 * nx, oy += a0 * ny, oz += a0 * nz;
                qnx = nx - au * ux - av * vx, qny = ny - au * uy - av * vy, qnz = nz - au * uz - av * vz;
                const double ql = 1.0 / sqrt(qnx * qnx + qny * qny + qnz * qnz);
                qnx *= ql, qny *= ql, qnz *= ql;
            }
            o.x = (float)ox, o.y = (float)oy, o.z = (float)oz;
            nrm[0] = (float)qnx, nrm[1] = (float)qny, nrm[2] = (float)qnz, nrm[3] = (float)curv;
        }
        a.out[idx] = o;
        if (a.normals) reinterpret_cast<float4*>(a.normals)[idx] = make_float4(nrm[0], nrm[1], nrm[2], nrm[3]);
        if (a.nn_count) a.nn_count[idx] = k;
        if (a.fit) a.fit[idx] = (uint8_t)kind;
    }
    // the result's counters: per wave, then one integer atomic per wave and counter (order-independent)
    const unsigned long long none = __ballot(kind == O3DR_MLS_NONE), plane = __ballot(kind == O3DR_MLS_PLANE),
                             poly = __ballot(kind == O3DR_MLS_POLY);
    uint32_t km = k;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t x = __shfl_xor(km, o, 64);
        km = x > km ? x : km;
    }
    if ((threadIdx.x & 63) == 0 && (none | plane | poly)) {
        if (none) atomicAdd(&a.counters[0], (unsigned long long)__popcll(none));
        if (plane) atomicAdd(&a.counters[1], (unsigned long long)__popcll(plane));
        if (poly) atomicAdd(&a.counters[2], (unsigned long long)__popcll(poly));
        atomicMax(&a.counters[3], (unsigned long long)km);
    }
}
static_assert(kMlsThreads % kWave == 0, "the counters are folded per wave");
