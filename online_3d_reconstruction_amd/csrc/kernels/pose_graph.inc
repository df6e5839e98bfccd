// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Pose-graph refinement (o3dr_pose_graph_refine; contract: include/o3dr.h "pose graph", DESIGN.md "Pose-graph refinement")
//   k_graph_moments: ONE workgroup of kGraphRun threads per pair.  A step covers one run of 256 query rows: every thread
//   loads its row's correspondence in camera coordinates (used: pair_finite and the pair's gates), the 29 fields go through
//   wave_fields, the run is tree4 of its four waves (kernels/rigid_core.inc) and one lane per field folds the runs left to
//   right (the chain's partition).  The record keeps its own products: it is not the rigid record.  The pair's whole contribution
//   to the solve is that record: the iterations never touch a keypoint again.
//   k_graph_solve: ONE workgroup of kGraphThreads threads, vectors in global memory.  Per Gauss-Newton iteration one thread
//   per edge builds the edge's blocks, one thread per (frame, row) sums the gradient over the frame's adjacency, then
//   cg_iterations steps of block-Jacobi preconditioned CG (matvec: one thread per (frame, row) over the adjacency), then one
//   thread per frame retracts.  The diagonal blocks do not depend on the poses: they and their inverses are built once.
//   Nothing waits on another workgroup (there is none), every loop is bounded by a count from the arguments, and every
//   branch around a barrier is uniform (the scalars it tests come out of graph_sum, the same value in every thread).
// =================================================================================================
static_assert(kGraphRun == kChainRun && kGraphRun / kWave == 4, "the chain's partition");

__global__ __launch_bounds__(kGraphRun) void k_graph_moments(GraphMomArgs a)
{
    __shared__ double red[2][kGraphFields][kGraphRun / kWave];
    const uint32_t p = blockIdx.x;
    if (p >= a.n_pairs) return;  // (uniform)
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const MatchPair P = a.m.pairs[p];
    const bool ok = a.pair_ok[p] != 0;
    const uint32_t n_steps = (P.nq + kGraphRun - 1) / kGraphRun;
    double tot = 0.0;
    for (uint32_t st = 0; st < n_steps; ++st) {
        const uint32_t row = st * kGraphRun + tid;
        bool good = false, used = false;
        float4 sp = make_float4(0.f, 0.f, 0.f, 0.f), tp = sp;
        if (row < P.nq) {
            const MatchedRow m = matched_row(a.m, P, P.qbase, row, ok);  // (a rejected frame's pair: its good rows are still counted)
            good = m.good;
            if (m.hit) {
                sp = m.s, tp = m.t;
                used = pair_finite(sp, tp) && m.in;
            }
        }
        const double ax = used ? (double)sp.x : 0.0, ay = used ? (double)sp.y : 0.0, az = used ? (double)sp.z : 0.0;
        const double bx = used ? (double)tp.x : 0.0, by = used ? (double)tp.y : 0.0, bz = used ? (double)tp.z : 0.0;
        double v[kGraphFields];
        v[0] = used ? 1.0 : 0.0;
        v[1] = ax, v[2] = ay, v[3] = az;
        v[4] = bx, v[5] = by, v[6] = bz;
        v[7] = ax * ax, v[8] = ax * ay, v[9] = ax * az, v[10] = ay * ay, v[11] = ay * az, v[12] = az * az;
        v[13] = bx * bx, v[14] = bx * by, v[15] = bx * bz, v[16] = by * by, v[17] = by * bz, v[18] = bz * bz;
        v[19] = ax * bx, v[20] = ax * by, v[21] = ax * bz;
        v[22] = ay * bx, v[23] = ay * by, v[24] = ay * bz;
        v[25] = az * bx, v[26] = az * by, v[27] = az * bz;
        v[28] = good ? 1.0 : 0.0;
        double(*rd)[kGraphRun / kWave] = red[st & 1];
        wave_fields<kGraphFields>(v, rd, lane, wv);
        __syncthreads();  // (the other buffer is written next: its readers passed this barrier's predecessor)
        if (tid < (uint32_t)kGraphFields) tot += tree4(rd[tid]);
    }
    if (tid < (uint32_t)kGraphFields) a.mom[(uint64_t)p * kGraphFields + tid] = tot;
    if (tid == 0) a.counts[2 * (uint64_t)p + 1] = (uint32_t)tot;   // (counts are exact in fp64)
    if (tid == 28) a.counts[2 * (uint64_t)p] = (uint32_t)tot;
}

// ---- the solve ----------------------------------------------------------------------------------------------------------
// sum of x[k] y[k] (y == nullptr: of x[k]) over k < n, the same value in every thread: thread t takes k = t, t + 256, .. in
// ascending order, wave sums, then (w0 + w1) + (w2 + w3).  Two barriers: the second frees `red` for the next call.
__device__ double graph_sum(const double* x, const double* y, uint32_t n, double* red)
{
    double s = 0.0;
    for (uint32_t k = threadIdx.x; k < n; k += kGraphThreads) s += y ? x[k] * y[k] : x[k];
    wave_fields<1>(&s, reinterpret_cast<double(*)[kGraphThreads / kWave]>(red), threadIdx.x & 63, threadIdx.x >> 6);
    __syncthreads();
    const double r = tree4(red);
    __syncthreads();
    return r;
}

__device__ double graph_max_abs(const double* x, uint32_t n, double* red)
{
    double s = 0.0;
    for (uint32_t k = threadIdx.x; k < n; k += kGraphThreads) s = fmax(s, fabs(x[k]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s = fmax(s, __shfl_xor(s, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const double r = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return r;
}

// [x]x: hat(x) v = x cross v
__device__ __forceinline__ void graph_hat(const double x[3], double H[3][3])
{
    H[0][0] = 0.0, H[0][1] = -x[2], H[0][2] = x[1];
    H[1][0] = x[2], H[1][1] = 0.0, H[1][2] = -x[0];
    H[2][0] = -x[1], H[2][1] = x[0], H[2][2] = 0.0;
}

__device__ __forceinline__ void graph_mul3(const double A[3][3], const double B[3][3], double C[3][3])
{
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) C[r][c] = (A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c];
}

// entry (r, c) of a frame's diagonal block from one side of an edge: n, S = sum of the side's points, SS = their second
// moments (xx xy xz yy yz zz)
__device__ double graph_diag_entry(double n, const double* S, const double* SS, int r, int c)
{
    if (r < 3 && c < 3) return r == c ? n : 0.0;
    double h[3][3];
    graph_hat(S, h);
    if (r < 3) return -h[r][c - 3];
    if (c < 3) return h[r - 3][c];
    const int i = r - 3, j = c - 3;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const double ss = SS[lo == 0 ? hi : (lo == 1 ? 2 + hi : 5)];
    return i == j ? ((SS[0] + SS[3]) + SS[5]) - ss : -ss;
}

// one edge at the current poses: H_ij (6 x 6 row-major), g_i and g_j, the edge's energy
__device__ void graph_edge(const double* m, const double* Si, const double* Sj, double* Hij, double* g, double* E)
{
    const double n = m[0];
    const double* Sa = m + 1;
    const double* Sb = m + 4;
    double Sab[3][3], M[3][3], d[3], e[3], dt[3];
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) {
            Sab[p][q] = m[19 + 3 * p + q];
            M[p][q] = (Si[p] * Sj[q] + Si[3 + p] * Sj[3 + q]) + Si[6 + p] * Sj[6 + q];
        }
    for (int k = 0; k < 3; ++k) dt[k] = Si[9 + k] - Sj[9 + k];
    for (int p = 0; p < 3; ++p) {
        d[p] = (Si[p] * dt[0] + Si[3 + p] * dt[1]) + Si[6 + p] * dt[2];
        e[p] = (Sj[p] * dt[0] + Sj[3 + p] * dt[1]) + Sj[6 + p] * dt[2];
    }
    double MSb[3], MtSa[3];
    for (int p = 0; p < 3; ++p) {
        MSb[p] = (M[p][0] * Sb[0] + M[p][1] * Sb[1]) + M[p][2] * Sb[2];
        MtSa[p] = (M[0][p] * Sa[0] + M[1][p] * Sa[1]) + M[2][p] * Sa[2];
    }
    double msab = 0.0;
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) msab += M[p][q] * Sab[p][q];
    const double dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const double dSa = (d[0] * Sa[0] + d[1] * Sa[1]) + d[2] * Sa[2];
    const double dMSb = (d[0] * MSb[0] + d[1] * MSb[1]) + d[2] * MSb[2];
    const double trA = (m[7] + m[10]) + m[12], trB = (m[13] + m[16]) + m[18];
    *E = ((((trA + trB) + n * dd) + 2.0 * dSa) - 2.0 * msab) - 2.0 * dMSb;
    // blocks
    double hSa[3][3], hSb[3][3], B[3][3], Cb[3][3], W[3][3];
    graph_hat(Sa, hSa);
    graph_hat(Sb, hSb);
    graph_mul3(M, hSb, B);
    graph_mul3(hSa, M, Cb);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) W[r][c] = 0.0;
    for (int p = 0; p < 3; ++p)
        for (int q = 0; q < 3; ++q) {
            double ep[3] = {0.0, 0.0, 0.0}, eq[3] = {0.0, 0.0, 0.0}, hp[3][3], hq[3][3], t1[3][3], t2[3][3];
            ep[p] = 1.0, eq[q] = 1.0;
            graph_hat(ep, hp);
            graph_hat(eq, hq);
            graph_mul3(hp, M, t1);
            graph_mul3(t1, hq, t2);
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) W[r][c] += Sab[p][q] * t2[r][c];
        }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            Hij[6 * r + c] = -(n * M[r][c]);
            Hij[6 * r + 3 + c] = B[r][c];
            Hij[6 * (3 + r) + c] = -Cb[r][c];
            Hij[6 * (3 + r) + 3 + c] = W[r][c];
        }
    // gradient halves
    double Pm[3][3], Qm[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            Pm[r][c] = (Sab[r][0] * M[c][0] + Sab[r][1] * M[c][1]) + Sab[r][2] * M[c][2];
            Qm[r][c] = (Sab[0][r] * M[0][c] + Sab[1][r] * M[1][c]) + Sab[2][r] * M[2][c];
        }
    for (int k = 0; k < 3; ++k) {
        g[k] = (Sa[k] + n * d[k]) - MSb[k];
        g[6 + k] = -((MtSa[k] + n * e[k]) - Sb[k]);
    }
    g[3] = (Sa[1] * d[2] - Sa[2] * d[1]) - (Pm[1][2] - Pm[2][1]);
    g[4] = (Sa[2] * d[0] - Sa[0] * d[2]) - (Pm[2][0] - Pm[0][2]);
    g[5] = (Sa[0] * d[1] - Sa[1] * d[0]) - (Pm[0][1] - Pm[1][0]);
    g[9] = -((Qm[1][2] - Qm[2][1]) + (Sb[1] * e[2] - Sb[2] * e[1]));
    g[10] = -((Qm[2][0] - Qm[0][2]) + (Sb[2] * e[0] - Sb[0] * e[2]));
    g[11] = -((Qm[0][1] - Qm[1][0]) + (Sb[0] * e[1] - Sb[1] * e[0]));
}

// inverse of a symmetric 6 x 6 block by Cholesky (A = L L^T, inv = L^-T L^-1); false: not positive definite
__device__ bool graph_invert6(const double* A, double* inv)
{
    double L[6][6], Li[6][6];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = A[6 * i + j];
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            if (i == j) {
                if (!(s > 0.0) || !isfinite(s)) return false;
                L[i][i] = sqrt(s);
            } else {
                L[i][j] = s / L[j][j];
            }
        }
    for (int c = 0; c < 6; ++c)  // L^-1, column by column (forward substitution)
        for (int i = 0; i < 6; ++i) {
            if (i < c) {
                Li[i][c] = 0.0;
                continue;
            }
            double s = i == c ? 1.0 : 0.0;
            for (int k = c; k < i; ++k) s -= L[i][k] * Li[k][c];
            Li[i][c] = s / L[i][i];
        }
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) {
            double s = 0.0;
            for (int k = (i > j ? i : j); k < 6; ++k) s += Li[k][i] * Li[k][j];
            inv[6 * i + j] = s;
        }
    return true;
}

__global__ __launch_bounds__(kGraphThreads) void k_graph_solve(GraphArgs a)
{
    __shared__ double red[kGraphThreads / kWave];
    __shared__ uint32_t flags_s;
    const uint32_t tid = threadIdx.x;
    const uint32_t F = a.n_frames, E = a.n_edges, N = 6 * F;
    double* vr = a.vec;
    double* vx = a.vec + (uint64_t)N;
    double* vz = a.vec + 2 * (uint64_t)N;
    double* vp = a.vec + 3 * (uint64_t)N;
    double* vh = a.vec + 4 * (uint64_t)N;
    double* Minv = a.Hd + 36 * (uint64_t)F;
    if (tid == 0) flags_s = 0u;
    // the state: t, and R orthonormalised by rows
    for (uint32_t f = tid; f < F; f += kGraphThreads) {
        const float* m = a.poses_in + 16 * (uint64_t)f;
        double* S = a.state + 12 * (uint64_t)f;
        const double r1[3] = {(double)m[0], (double)m[1], (double)m[2]}, r2[3] = {(double)m[4], (double)m[5], (double)m[6]};
        const double n1 = sqrt((r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2]);
        const double e1[3] = {r1[0] / n1, r1[1] / n1, r1[2] / n1};
        const double pr = (r2[0] * e1[0] + r2[1] * e1[1]) + r2[2] * e1[2];
        const double u[3] = {r2[0] - pr * e1[0], r2[1] - pr * e1[1], r2[2] - pr * e1[2]};
        const double n2 = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
        const double e2[3] = {u[0] / n2, u[1] / n2, u[2] / n2};
        S[0] = e1[0], S[1] = e1[1], S[2] = e1[2];
        S[3] = e2[0], S[4] = e2[1], S[5] = e2[2];
        S[6] = e1[1] * e2[2] - e1[2] * e2[1];
        S[7] = e1[2] * e2[0] - e1[0] * e2[2];
        S[8] = e1[0] * e2[1] - e1[1] * e2[0];
        S[9] = (double)m[3], S[10] = (double)m[7], S[11] = (double)m[11];
    }
    // the diagonal blocks (they do not depend on the poses), summed over each frame's adjacency in pair order
    for (uint32_t c = tid; c < 36 * F; c += kGraphThreads) {
        const uint32_t f = c / 36, k = c - 36 * f;
        const int r = (int)(k / 6), q = (int)(k - 6 * (k / 6));
        const GraphFrameIn Fr = a.frames[f];
        double s = 0.0;
        if (Fr.role == (uint32_t)O3DR_REFINE_FREE) {
            for (uint32_t n = 0; n < Fr.n_adj; ++n) {
                const uint32_t es = a.adj[Fr.adj0 + n];
                const double* m = a.mom + (uint64_t)a.edges[es >> 1].pair * kGraphFields;
                s += (es & 1u) ? graph_diag_entry(m[0], m + 4, m + 13, r, q) : graph_diag_entry(m[0], m + 1, m + 7, r, q);
            }
            if (r == q && r < 3) s += a.prior_weight;
        }
        a.Hd[c] = s;
    }
    __syncthreads();
    for (uint32_t f = tid; f < F; f += kGraphThreads) {
        double* inv = Minv + 36 * (uint64_t)f;
        bool ok = false;
        if (a.frames[f].role == (uint32_t)O3DR_REFINE_FREE) {
            ok = graph_invert6(a.Hd + 36 * (uint64_t)f, inv);
            if (!ok) atomicOr(&flags_s, (uint32_t)O3DR_REFINE_FLAG_SINGULAR);
        }
        if (!ok)
            for (int k = 0; k < 36; ++k) inv[k] = 0.0;
    }
    __syncthreads();

    double energy_before = 0.0, grad_before = 0.0, energy = 0.0, grad = 0.0, last_step = 0.0;
    for (uint32_t it = 0; it <= a.gn_iterations; ++it) {
        // the edges at the current poses
        for (uint32_t e = tid; e < E; e += kGraphThreads) {
            const GraphEdgeIn Ed = a.edges[e];
            double en;
            graph_edge(a.mom + (uint64_t)Ed.pair * kGraphFields, a.state + 12 * (uint64_t)Ed.i, a.state + 12 * (uint64_t)Ed.j,
                       a.Hij + 36 * (uint64_t)e, a.ge + 12 * (uint64_t)e, &en);
            a.Ee[2 * (uint64_t)e + 1] = en;
            if (it == 0) a.Ee[2 * (uint64_t)e] = en;
        }
        __syncthreads();
        // r = -g per (frame, row), the prior's energy per frame in vh
        for (uint32_t c = tid; c < N; c += kGraphThreads) {
            const uint32_t f = c / 6, r = c - 6 * f;
            const GraphFrameIn Fr = a.frames[f];
            double g = 0.0, ep = 0.0;
            if (Fr.role == (uint32_t)O3DR_REFINE_FREE) {
                for (uint32_t n = 0; n < Fr.n_adj; ++n) {
                    const uint32_t es = a.adj[Fr.adj0 + n];
                    g += a.ge[12 * (uint64_t)(es >> 1) + 6 * (es & 1u) + r];
                }
                if (a.prior && a.prior_weight > 0.0) {
                    const double* S = a.state + 12 * (uint64_t)f;
                    const float* pm = a.prior + 16 * (uint64_t)f;
                    const double dt[3] = {S[9] - (double)pm[3], S[10] - (double)pm[7], S[11] - (double)pm[11]};
                    if (r < 3) g += a.prior_weight * ((S[r] * dt[0] + S[3 + r] * dt[1]) + S[6 + r] * dt[2]);
                    if (r == 0) ep = a.prior_weight * ((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]);
                }
            }
            vr[c] = -g;
            vx[c] = 0.0;
            vh[c] = ep;
        }
        __syncthreads();
        double esum = 0.0;
        for (uint32_t k = tid; k < E; k += kGraphThreads) esum += a.Ee[2 * (uint64_t)k + 1];  // (graph_sum's order, stride 2)
        esum = wave_sum_f64(esum);
        if ((tid & 63) == 0) red[tid >> 6] = esum;
        __syncthreads();
        esum = (red[0] + red[1]) + (red[2] + red[3]);
        __syncthreads();
        energy = esum + graph_sum(vh, nullptr, N, red);
        grad = sqrt(graph_sum(vr, vr, N, red));
        if (it == 0) energy_before = energy, grad_before = grad;
        if (it == a.gn_iterations) break;  // (uniform)
        // z = Minv r, p = z
        for (uint32_t c = tid; c < N; c += kGraphThreads) {
            const uint32_t f = c / 6, r = c - 6 * f;
            const double* mi = Minv + 36 * (uint64_t)f + 6 * r;
            const double* x = vr + 6 * (uint64_t)f;
            double s = 0.0;
            for (int k = 0; k < 6; ++k) s += mi[k] * x[k];
            vz[c] = s;
            vp[c] = s;
        }
        __syncthreads();
        double rz = graph_sum(vr, vz, N, red);
        for (uint32_t cg = 0; cg < a.cg_iterations; ++cg) {
            // H p
            for (uint32_t c = tid; c < N; c += kGraphThreads) {
                const uint32_t f = c / 6, r = c - 6 * f;
                const GraphFrameIn Fr = a.frames[f];
                double s = 0.0;
                if (Fr.role == (uint32_t)O3DR_REFINE_FREE) {
                    const double* hd = a.Hd + 36 * (uint64_t)f + 6 * r;
                    const double* x = vp + 6 * (uint64_t)f;
                    for (int k = 0; k < 6; ++k) s += hd[k] * x[k];
                    for (uint32_t n = 0; n < Fr.n_adj; ++n) {
                        const uint32_t es = a.adj[Fr.adj0 + n], e = es >> 1;
                        const GraphEdgeIn Ed = a.edges[e];
                        const double* h = a.Hij + 36 * (uint64_t)e;
                        if (es & 1u) {  // this frame is j: H_ij^T x_i
                            const double* y = vp + 6 * (uint64_t)Ed.i;
                            for (int k = 0; k < 6; ++k) s += h[6 * k + r] * y[k];
                        } else {
                            const double* y = vp + 6 * (uint64_t)Ed.j;
                            for (int k = 0; k < 6; ++k) s += h[6 * r + k] * y[k];
                        }
                    }
                }
                vh[c] = s;
            }
            __syncthreads();
            const double pHp = graph_sum(vp, vh, N, red);
            if (!(pHp > 0.0) || !isfinite(pHp) || !isfinite(rz)) {  // (uniform)
                if (tid == 0) flags_s |= (uint32_t)O3DR_REFINE_FLAG_CG_STOPPED;
                break;
            }
            const double alpha = rz / pHp;
            for (uint32_t c = tid; c < N; c += kGraphThreads) {
                vx[c] = vx[c] + alpha * vp[c];
                vr[c] = vr[c] - alpha * vh[c];
            }
            __syncthreads();
            for (uint32_t c = tid; c < N; c += kGraphThreads) {
                const uint32_t f = c / 6, r = c - 6 * f;
                const double* mi = Minv + 36 * (uint64_t)f + 6 * r;
                const double* x = vr + 6 * (uint64_t)f;
                double s = 0.0;
                for (int k = 0; k < 6; ++k) s += mi[k] * x[k];
                vz[c] = s;
            }
            __syncthreads();
            const double rz_new = graph_sum(vr, vz, N, red);
            const double beta = rz_new / rz;
            if (!isfinite(beta)) {  // (uniform)
                if (tid == 0) flags_s |= (uint32_t)O3DR_REFINE_FLAG_CG_STOPPED;
                break;
            }
            for (uint32_t c = tid; c < N; c += kGraphThreads) vp[c] = vz[c] + beta * vp[c];
            rz = rz_new;
            __syncthreads();
        }
        __syncthreads();
        last_step = graph_max_abs(vx, N, red);
        // retraction: t <- t + R v, R <- R C(w)
        for (uint32_t f = tid; f < F; f += kGraphThreads) {
            if (a.frames[f].role != (uint32_t)O3DR_REFINE_FREE) continue;
            double* S = a.state + 12 * (uint64_t)f;
            const double* x = vx + 6 * (uint64_t)f;
            double R[3][3], Cm[3][3], Rn[3][3];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) R[r][c] = S[3 * r + c];
            for (int r = 0; r < 3; ++r) S[9 + r] = S[9 + r] + ((R[r][0] * x[0] + R[r][1] * x[1]) + R[r][2] * x[2]);
            double qx = 0.5 * x[3], qy = 0.5 * x[4], qz = 0.5 * x[5];
            const double qn = sqrt(1.0 + ((qx * qx + qy * qy) + qz * qz));
            const double q0 = 1.0 / qn;
            qx = qx / qn, qy = qy / qn, qz = qz / qn;
            Cm[0][0] = 1.0 - 2.0 * (qy * qy + qz * qz), Cm[0][1] = 2.0 * (qx * qy - q0 * qz), Cm[0][2] = 2.0 * (qx * qz + q0 * qy);
            Cm[1][0] = 2.0 * (qx * qy + q0 * qz), Cm[1][1] = 1.0 - 2.0 * (qx * qx + qz * qz), Cm[1][2] = 2.0 * (qy * qz - q0 * qx);
            Cm[2][0] = 2.0 * (qx * qz - q0 * qy), Cm[2][1] = 2.0 * (qy * qz + q0 * qx), Cm[2][2] = 1.0 - 2.0 * (qx * qx + qy * qy);
            graph_mul3(R, Cm, Rn);
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) S[3 * r + c] = Rn[r][c];
        }
        __syncthreads();
    }
    __syncthreads();
    // outputs
    for (uint32_t f = tid; f < F; f += kGraphThreads) {
        const GraphFrameIn Fr = a.frames[f];
        const float* m = a.poses_in + 16 * (uint64_t)f;
        float* o = a.poses_out + 16 * (uint64_t)f;
        const double* S = a.state + 12 * (uint64_t)f;
        o3dr_refine_frame rec;
        rec.role = (int32_t)Fr.role;
        rec.degree = (int32_t)Fr.n_adj;
        if (Fr.role == (uint32_t)O3DR_REFINE_FREE) {
            for (int r = 0; r < 3; ++r) {
                for (int c = 0; c < 3; ++c) rec.T[4 * r + c] = S[3 * r + c];
                rec.T[4 * r + 3] = S[9 + r];
            }
            for (int k = 0; k < 12; ++k) o[k] = (float)rec.T[k];
            o[12] = o[13] = o[14] = 0.f;
            o[15] = 1.f;
        } else {
            for (int k = 0; k < 12; ++k) rec.T[k] = (double)m[k];
            const uint32_t* mi = reinterpret_cast<const uint32_t*>(m);
            uint32_t* oi = reinterpret_cast<uint32_t*>(o);
            for (int k = 0; k < 16; ++k) oi[k] = mi[k];  // (the input's bytes, NaN payloads included)
        }
        a.frames_out[f] = rec;
    }
    if (tid == 0) {
        o3dr_refine_result r = a.counts;
        r.energy_before = energy_before;
        r.energy_after = energy;
        r.grad_before = grad_before;
        r.grad_after = grad;
        r.last_step = last_step;
        r.flags = (int32_t)flags_s;
        *a.res = r;
    }
}
