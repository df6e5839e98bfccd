// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Pose chain (o3dr_pose_chain; contract: include/o3dr.h "pose chain", DESIGN.md "Pose chain")
//   k_pose_chain: ONE workgroup of kChainThreads threads walks the frames n_fixed .. n_frames - 1 in order.  Frame i's
//   correspondence slots are (pair, query row), pair-major in the static list's order: slot s is row s % nq of pair
//   s / nq (every pair of a frame has the frame as its query set).  Per frame:
//     0. the train frames' poses and "accepted" flags go to LDS (the same workgroup wrote them, a barrier ago);
//     1. pass A: every slot's `used` flag; n_good, n_used and the first used slot (integer LDS atomics);
//     2. pass B: rigid_moments about c0 = the first used tgt, wave_fields per wave, the run of 256 slots = tree4 of its
//        four waves (kernels/rigid_core.inc), the runs folded left to right by one lane per field;
//     3. lane 0: rigid_solve (o3dr_rigid_solve.h), the function the host calls;
//     4. pass C: rigid_residual2 at T over the same partition and fold;
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
    float4 s, t;      // src, the moved tgt
};

// slot s of a frame: the row's record, src and the moved tgt (all clear past the frame's n_slots)
__device__ __forceinline__ ChainSlot chain_slot(const ChainArgs& a, const ChainFrameIn& F, uint32_t s, uint32_t n_slots,
                                                const float (*pose)[12], const uint32_t* accepted)
{
    ChainSlot o;
    o.good = o.used = false;
    o.s = o.t = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s >= n_slots) return o;
    const uint32_t lp = s / F.nq, row = s - lp * F.nq;
    if (!accepted[lp]) return o;
    const MatchedRow m = matched_row(a.m, a.m.pairs[F.pair0 + lp], F.qbase, row);
    o.good = m.good;
    if (!m.hit) return o;
    o.s = m.s;
    a2_apply(pose[lp], m.t.x, m.t.y, m.t.z, o.t.x, o.t.y, o.t.z);
    o.used = pair_finite(o.s, o.t);
    if (!m.in) o.used = false;  // (o3dr_pose_chain_robust: the pair's RANSAC mask)
    return o;
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
            const ChainSlot c = chain_slot(a, F, s, n_slots, pose_s, acc_s);
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
        const ChainSlot cf = chain_slot(a, F, first, n_slots, pose_s, acc_s);
        const double c0[3] = {(double)cf.t.x, (double)cf.t.y, (double)cf.t.z};
        // 2. moments about c0
        double tot = 0.0;
        for (uint32_t st = 0; st < n_steps; ++st) {
            const uint32_t s = st * kChainThreads + tid;
            const ChainSlot c = chain_slot(a, F, s, n_slots, pose_s, acc_s);
            double v[kRigidFields];
            rigid_moments(c.used, c.s, c.t, c0, v);
            double(*rd)[kChainWaves] = red[st & 1];
            wave_fields<kRigidFields>(v, rd, lane, wv);
            __syncthreads();  // (the other buffer is written next: its readers passed this barrier's predecessor)
            if (tid < kRigidFields)
                for (int r = 0; r < kChainRuns; ++r) tot += tree4(&rd[tid][kChainRunWaves * r]);
        }
        if (tid < kRigidFields) mom_s[tid] = tot;
        __syncthreads();
        // 3. the solve
        if (tid == 0) {
            double rec[kRigidFields], T[12];
            for (int k = 0; k < kRigidFields; ++k) rec[k] = mom_s[k];
            const bool ok = rigid_solve(rec, c0, T);
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
            const ChainSlot c = chain_slot(a, F, s, n_slots, pose_s, acc_s);
            const double r2 = rigid_residual2(T, c.s, c.t), x = c.used ? r2 : 0.0;
            double(*rd)[kChainWaves] = red[st & 1];
            wave_fields<1>(&x, rd, lane, wv);
            __syncthreads();
            if (tid == 0)
                for (int r = 0; r < kChainRuns; ++r) d2 += tree4(&rd[0][kChainRunWaves * r]);
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
