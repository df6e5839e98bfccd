// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Pose chain (o3dr_pose_chain; contract: include/o3dr.h "pose chain", DESIGN.md "Pose chain")
//   k_pose_chain: ONE workgroup of kChainThreads threads walks the frames n_fixed .. n_frames - 1 in order.  Frame i's
//   correspondence slots are (pair, query row), pair-major in the static list's order: slot s is row s % nq of pair
//   s / nq (every pair of a frame has the frame as its query set).  Per frame:
//     0. the train frames' poses and "accepted" flags go to LDS (the same workgroup wrote them, a barrier ago);
//     1. pass A: every slot's `used` flag; n_good, n_used and the first used slot (integer LDS atomics);
//     2. pass B: the 16 moments of k_rigid_sums about c0 = the first used tgt, wave sums per wave, the run of 256 slots =
//        the tree of its four waves, the runs folded left to right by one lane per field;
//     3. lane 0: the Kabsch of icp_solve / svd3 (o3dr_api.hip), operation for operation;
//     4. pass C: the squared residuals at T over the same partition and fold;
//     5. lane 0 writes the record, the pose and the status; a barrier ends the frame.
//   Nothing waits on another workgroup (there is none), and every loop is bounded by a count from the arguments.
// =================================================================================================
constexpr int kChainWaves = kChainThreads / kWave;
constexpr int kChainRunWaves = kChainRun / kWave;      // waves per run of 256 slots
constexpr int kChainRuns = kChainThreads / kChainRun;  // runs per step of the workgroup
static_assert(kChainRun == kRigidPoints && kChainRunWaves == 4, "the partition of k_rigid_sums");
static_assert(kChainThreads >= 12 * kChainMaxPairs, "step 0: one lane per pose entry");

struct ChainSlot {
    bool good, used;  // good row of an accepted train frame; all of the contract's conditions (with the RANSAC byte, if any)
    float sx, sy, sz, tx, ty, tz;
};

// slot s of a frame: the row's record, src and the moved tgt
__device__ __forceinline__ ChainSlot chain_slot(const ChainArgs& a, const ChainFrameIn& F, uint32_t s, const float (*pose)[12],
                                                const uint32_t* accepted)
{
    ChainSlot o;
    o.good = o.used = false;
    o.sx = o.sy = o.sz = o.tx = o.ty = o.tz = 0.f;
    const uint32_t lp = s / F.nq, row = s - lp * F.nq;
    if (!accepted[lp]) return o;
    const MatchedRow m = matched_row(a.m, a.m.pairs[F.pair0 + lp], F.qbase, row);
    o.good = m.good;
    if (!m.hit) return o;
    const float4 sp = m.s, tp = m.t;
    float X, Y, Z;
    a2_apply(pose[lp], tp.x, tp.y, tp.z, X, Y, Z);
    o.sx = sp.x, o.sy = sp.y, o.sz = sp.z;
    o.tx = X, o.ty = Y, o.tz = Z;
    o.used = isfinite(sp.x) && isfinite(sp.y) && isfinite(sp.z) && isfinite(X) && isfinite(Y) && isfinite(Z);
    if (!m.in) o.used = false;  // (o3dr_pose_chain_robust: the pair's RANSAC mask)
    return o;
}

// svd3 of o3dr_api.hip on the device: one-sided Jacobi, S descending (stable for equal norms)
__device__ void chain_svd3(const double A_in[3][3], double U[3][3], double S[3], double V[3][3])
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

// icp_solve of o3dr_api.hip on the device: T (3 x 4, row-major) from the moments about c0; false: rank < 2
__device__ bool chain_solve(const double* rec, const double c0[3], double T[12])
{
    const double n = rec[0];
    double ma[3], mb[3], H[3][3];
    for (int k = 0; k < 3; ++k) ma[k] = rec[1 + k] / n, mb[k] = rec[4 + k] / n;
    for (int j = 0; j < 3; ++j)
        for (int k = 0; k < 3; ++k) H[j][k] = rec[7 + 3 * j + k] - n * ma[j] * mb[k];
    double U[3][3], S[3], V[3][3];
    chain_svd3(H, U, S, V);
    if (!(S[0] > 0.0) || !isfinite(S[0]) || !(S[1] > 1e-12 * S[0])) return false;
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

// the record, the pose and the status of frame i (one lane).  T == nullptr: the prior
__device__ void chain_write(const ChainArgs& a, uint32_t i, int32_t status, uint32_t n_pairs, uint32_t n_acc, uint32_t n_good,
                            uint32_t n_used, double rms, const double* T)
{
    o3dr_chain_frame r;
    r.status = status;
    r.n_pairs = (int32_t)n_pairs;
    r.n_pairs_accepted = (int32_t)n_acc;
    r.n_good = (int32_t)n_good;
    r.n_used = (int32_t)n_used;
    r.reserved = 0;
    r.rms = rms;
    float* pose = a.poses + 16 * (uint64_t)i;
    for (int k = 0; k < 12; ++k) {
        const float v = T ? (float)T[k] : a.prior[16 * (uint64_t)i + k];
        pose[k] = v;
        r.T[k] = T ? T[k] : (double)v;
    }
    pose[12] = pose[13] = pose[14] = 0.f;
    pose[15] = 1.f;
    if (!T)
        for (int k = 12; k < 16; ++k) pose[k] = a.prior[16 * (uint64_t)i + k];
    a.out[i] = r;
    a.status[i] = status;
}

__global__ __launch_bounds__(kChainThreads) void k_pose_chain(ChainArgs a)
{
    __shared__ float pose_s[kChainMaxPairs][12];
    __shared__ uint32_t acc_s[kChainMaxPairs];
    __shared__ uint32_t cnt_s[4];  // first used slot, n_good, n_used, accepted pairs
    __shared__ double red[2][kRigidFields][kChainWaves];
    __shared__ double mom_s[kRigidFields];
    __shared__ double T_s[12];
    __shared__ int32_t st_s;
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;

    for (uint32_t i = a.n_fixed; i < a.n_frames; ++i) {
        const ChainFrameIn F = a.frames[i];
        if (F.n_pairs == 0) {  // (uniform)
            if (tid == 0) chain_write(a, i, O3DR_CHAIN_ANCHOR, 0, 0, 0, 0, 0.0, nullptr);
            __syncthreads();
            continue;
        }
        // 0. train poses and flags
        if (tid < 4) cnt_s[tid] = tid == 0 ? 0xFFFFFFFFu : 0u;
        if (tid < F.n_pairs) acc_s[tid] = (uint32_t)a.status[a.pair_train[F.pair0 + tid]] <= (uint32_t)O3DR_CHAIN_MATCHED ? 1u : 0u;
        if (tid < 12 * F.n_pairs) {
            const uint32_t lp = tid / 12, k = tid - 12 * lp;
            pose_s[lp][k] = a.poses[16 * (uint64_t)a.pair_train[F.pair0 + lp] + k];
        }
        __syncthreads();
        const uint32_t n_slots = F.n_pairs * F.nq;
        const uint32_t n_steps = (n_slots + kChainThreads - 1) / kChainThreads;
        // 1. counts and the first used slot
        if (tid < F.n_pairs && acc_s[tid]) atomicAdd(&cnt_s[3], 1u);
        for (uint32_t st = 0; st < n_steps; ++st) {
            const uint32_t s = st * kChainThreads + tid;
            ChainSlot c;
            c.good = c.used = false;
            if (s < n_slots) c = chain_slot(a, F, s, pose_s, acc_s);
            const uint64_t bg = __ballot(c.good), bu = __ballot(c.used);
            if (lane == 0) {
                if (bg) atomicAdd(&cnt_s[1], (uint32_t)__builtin_popcountll(bg));
                if (bu) {
                    atomicAdd(&cnt_s[2], (uint32_t)__builtin_popcountll(bu));
                    atomicMin(&cnt_s[0], st * kChainThreads + (tid & ~63u) + (uint32_t)__builtin_ctzll(bu));
                }
            }
        }
        __syncthreads();
        const uint32_t first = cnt_s[0], n_good = cnt_s[1], n_used = cnt_s[2], n_acc = cnt_s[3];
        if (n_used < a.min_matches) {  // (uniform; min_matches >= 3, so `first` exists below)
            if (tid == 0) chain_write(a, i, O3DR_CHAIN_TOO_FEW, F.n_pairs, n_acc, n_good, n_used, 0.0, nullptr);
            __syncthreads();
            continue;
        }
        const ChainSlot cf = chain_slot(a, F, first, pose_s, acc_s);
        const double c0[3] = {(double)cf.tx, (double)cf.ty, (double)cf.tz};
        // 2. moments about c0
        double tot = 0.0;
        for (uint32_t st = 0; st < n_steps; ++st) {
            const uint32_t s = st * kChainThreads + tid;
            ChainSlot c;
            c.used = false;
            c.sx = c.sy = c.sz = c.tx = c.ty = c.tz = 0.f;
            if (s < n_slots) c = chain_slot(a, F, s, pose_s, acc_s);
            const bool used = c.used;
            const double ax = used ? (double)c.sx - c0[0] : 0.0, ay = used ? (double)c.sy - c0[1] : 0.0, az = used ? (double)c.sz - c0[2] : 0.0;
            const double bx = used ? (double)c.tx - c0[0] : 0.0, by = used ? (double)c.ty - c0[1] : 0.0, bz = used ? (double)c.tz - c0[2] : 0.0;
            double v[kRigidFields];
            v[0] = used ? 1.0 : 0.0;
            v[1] = ax, v[2] = ay, v[3] = az;
            v[4] = bx, v[5] = by, v[6] = bz;
            v[7] = ax * bx, v[8] = ax * by, v[9] = ax * bz;
            v[10] = ay * bx, v[11] = ay * by, v[12] = ay * bz;
            v[13] = az * bx, v[14] = az * by, v[15] = az * bz;
            double(*rd)[kChainWaves] = red[st & 1];
#pragma unroll
            for (int f = 0; f < kRigidFields; ++f) {
                const double x = wave_sum_f64(v[f]);
                if (lane == 0) rd[f][wv] = x;
            }
            __syncthreads();  // (the other buffer is written next: its readers passed this barrier's predecessor)
            if (tid < kRigidFields)
                for (int r = 0; r < kChainRuns; ++r) tot += (rd[tid][4 * r] + rd[tid][4 * r + 1]) + (rd[tid][4 * r + 2] + rd[tid][4 * r + 3]);
        }
        if (tid < kRigidFields) mom_s[tid] = tot;
        __syncthreads();
        // 3. the solve
        if (tid == 0) {
            double rec[kRigidFields], T[12];
            for (int k = 0; k < kRigidFields; ++k) rec[k] = mom_s[k];
            const bool ok = chain_solve(rec, c0, T);
            st_s = ok ? O3DR_CHAIN_MATCHED : O3DR_CHAIN_DEGENERATE;
            for (int k = 0; k < 12; ++k) T_s[k] = ok ? T[k] : 0.0;
        }
        __syncthreads();
        if (st_s == O3DR_CHAIN_DEGENERATE) {  // (uniform)
            if (tid == 0) chain_write(a, i, O3DR_CHAIN_DEGENERATE, F.n_pairs, n_acc, n_good, n_used, 0.0, nullptr);
            __syncthreads();
            continue;
        }
        // 4. residuals at T
        double T[12];
        for (int k = 0; k < 12; ++k) T[k] = T_s[k];
        double d2 = 0.0;
        for (uint32_t st = 0; st < n_steps; ++st) {
            const uint32_t s = st * kChainThreads + tid;
            ChainSlot c;
            c.used = false;
            c.sx = c.sy = c.sz = c.tx = c.ty = c.tz = 0.f;
            if (s < n_slots) c = chain_slot(a, F, s, pose_s, acc_s);
            const double sx = c.sx, sy = c.sy, sz = c.sz;
            const double ex = ((T[0] * sx + T[1] * sy) + T[2] * sz) + T[3] - (double)c.tx;
            const double ey = ((T[4] * sx + T[5] * sy) + T[6] * sz) + T[7] - (double)c.ty;
            const double ez = ((T[8] * sx + T[9] * sy) + T[10] * sz) + T[11] - (double)c.tz;
            const double x = wave_sum_f64(c.used ? (ex * ex + ey * ey) + ez * ez : 0.0);
            double(*rd)[kChainWaves] = red[st & 1];
            if (lane == 0) rd[0][wv] = x;
            __syncthreads();
            if (tid == 0)
                for (int r = 0; r < kChainRuns; ++r) d2 += (rd[0][4 * r] + rd[0][4 * r + 1]) + (rd[0][4 * r + 2] + rd[0][4 * r + 3]);
        }
        // 5. the record
        if (tid == 0) {
            const double rms = sqrt(d2 / (double)n_used);
            if (!(rms <= a.max_rms))
                chain_write(a, i, O3DR_CHAIN_RMS, F.n_pairs, n_acc, n_good, n_used, rms, nullptr);
            else
                chain_write(a, i, O3DR_CHAIN_MATCHED, F.n_pairs, n_acc, n_good, n_used, rms, T);
        }
        __syncthreads();
    }
}
