// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Three-point RANSAC for a rigid transform (o3dr_ransac_rigid, o3dr_pose_chain_robust; contract: include/o3dr.h
// "robust rigid fit", DESIGN.md "Robust fit")
//   k_ransac_rigid<kChain>: ONE workgroup of kRansacThreads threads per segment.  kChain == false: the segment is a run of
//   index-aligned src / tgt points with an optional mask; true: it is one pair of the chain's static list (src = the query
//   frame's keypoint, tgt = the train frame's best match, mask = the matcher's good byte), both in camera coordinates.
//     1. ordered compaction of the candidates (ballot + popcount prefix, the waves' counts through LDS): candidate rank r
//        below kRansacStage has its six coordinates and its position in LDS (SoA: a wave's lane-strided reads are
//        conflict-free), a rank above it only its position in the workspace list `over`, and is read through it;
//     2. the waves take the hypotheses round-robin (h = wave, wave + kRansacWaves, ..); every lane builds the same model
//        (the draws are uniform), the lanes stride over the candidates, the score is a sum of ballot popcounts: an exact
//        integer.  Each wave keeps its best (score, h) as one key (score << 32 | ~h): greatest score, then lowest h;
//     3. one LDS reduction over the waves' keys picks the winner;
//     4. every thread rebuilds the winner's model with the same operation sequence and the workgroup writes one byte per
//        position of the segment (each byte once: no ordering between stores is needed); lane 0 writes the record.
//   The finite test, the sampler (splitmix64, draw3) and the residual (rigid_residual2) are the rigid core's
//   (kernels/rigid_core.inc, o3dr_rigid_solve.h).
//   24 + 4 KiB of LDS per workgroup: five workgroups per CU fit in the 160 KiB, so a chain's ~1500 pairs cover the machine
//   in one to two rounds.  No float atomics, and every loop is bounded by a count from the arguments.
// =================================================================================================
constexpr int kRansacWaves = kRansacThreads / kWave;
static_assert(kRansacStage % kWave == 0, "a wave's 64 candidates are all staged or all read through the list");

// position i of the segment: its six coordinates; true: a candidate
template <bool kChain>
__device__ __forceinline__ bool ransac_load(const RansacArgs& a, const RansacSeg& S, const MatchPair& P, uint32_t i, float p[6])
{
    float4 s, t;
    if constexpr (kChain) {
        const MatchedRow m = matched_row(a.m, P, P.qbase, i);  // (S.start is P.rec0)
        if (!m.hit) return false;
        s = m.s, t = m.t;
    } else {
        if (a.mask && !a.mask[S.start + i]) return false;
        s = reinterpret_cast<const float4*>(a.src)[S.start + i];
        t = reinterpret_cast<const float4*>(a.tgt)[S.start + i];
    }
    p[0] = s.x, p[1] = s.y, p[2] = s.z, p[3] = t.x, p[4] = t.y, p[5] = t.z;
    return pair_finite(s, t);
}

// the candidate of rank r (< m): its coordinates and its position in the segment
template <bool kChain>
__device__ __forceinline__ uint32_t ransac_candidate(const RansacArgs& a, const RansacSeg& S, const MatchPair& P, uint32_t r,
                                                     const float (*pt_s)[kRansacStage], const uint32_t* pos_s, float p[6])
{
    if (r < (uint32_t)kRansacStage) {
#pragma unroll
        for (int k = 0; k < 6; ++k) p[k] = pt_s[k][r];
        return pos_s[r];
    }
    const uint32_t i = a.over[S.over0 + (r - kRansacStage)];
    (void)ransac_load<kChain>(a, S, P, i, p);
    return i;
}

// the orthonormal frame of one side's three points: e1 along p1 - p0, e3 along (p1 - p0) x (p2 - p0), e2 = e3 x e1, and the
// centroid; false: degenerate (|u x v|^2 <= 1e-12 |u|^2 |v|^2)
__device__ __forceinline__ bool ransac_frame(const double p0[3], const double p1[3], const double p2[3], double e[3][3], double c[3])
{
    const double ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
    const double vx = p2[0] - p0[0], vy = p2[1] - p0[1], vz = p2[2] - p0[2];
    const double wx = uy * vz - uz * vy, wy = uz * vx - ux * vz, wz = ux * vy - uy * vx;
    const double uu = (ux * ux + uy * uy) + uz * uz, vv = (vx * vx + vy * vy) + vz * vz, ww = (wx * wx + wy * wy) + wz * wz;
    for (int k = 0; k < 3; ++k) c[k] = ((p0[k] + p1[k]) + p2[k]) / 3.0;
    if (ww <= (1e-12 * uu) * vv) return false;
    const double lu = sqrt(uu), lw = sqrt(ww);
    e[0][0] = ux / lu, e[0][1] = uy / lu, e[0][2] = uz / lu;
    e[2][0] = wx / lw, e[2][1] = wy / lw, e[2][2] = wz / lw;
    e[1][0] = e[2][1] * e[0][2] - e[2][2] * e[0][1];
    e[1][1] = e[2][2] * e[0][0] - e[2][0] * e[0][2];
    e[1][2] = e[2][0] * e[0][1] - e[2][1] * e[0][0];
    return true;
}

// the model of three candidates (each p[6]: src, tgt): T 3 x 4 row-major; false: degenerate
__device__ __forceinline__ bool ransac_model(const float q[3][6], double T[12])
{
    double s[3][3], t[3][3];
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) s[k][j] = (double)q[k][j], t[k][j] = (double)q[k][3 + j];
    double es[3][3], et[3][3], cs[3], ct[3];
    const bool oks = ransac_frame(s[0], s[1], s[2], es, cs);
    const bool okt = ransac_frame(t[0], t[1], t[2], et, ct);
    if (!oks || !okt) return false;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[4 * i + j] = (et[0][i] * es[0][j] + et[1][i] * es[1][j]) + et[2][i] * es[2][j];
        T[4 * i + 3] = ct[i] - ((T[4 * i] * cs[0] + T[4 * i + 1] * cs[1]) + T[4 * i + 2] * cs[2]);
    }
    return true;
}

__device__ __forceinline__ bool ransac_inlier(const double T[12], const float p[6], double thr2)
{
    return rigid_residual2(T, make_float4(p[0], p[1], p[2], 0.f), make_float4(p[3], p[4], p[5], 0.f)) <= thr2;
}

// hypothesis h of a segment with m candidates: the three ranks, the model; false: degenerate
template <bool kChain>
__device__ __forceinline__ bool ransac_hypothesis(const RansacArgs& a, const RansacSeg& S, const MatchPair& P, uint64_t seed_s, uint32_t h,
                                                  uint32_t m, const float (*pt_s)[kRansacStage], const uint32_t* pos_s, double T[12],
                                                  uint32_t pos[3])
{
    uint32_t loc[3];
    float q[3][6];
    draw3(seed_s, h, m, loc);
#pragma unroll
    for (int k = 0; k < 3; ++k) pos[k] = ransac_candidate<kChain>(a, S, P, loc[k], pt_s, pos_s, q[k]);
    if (loc[0] == loc[1] || loc[0] == loc[2] || loc[1] == loc[2]) return false;
    return ransac_model(q, T);
}

template <bool kChain>
__global__ __launch_bounds__(kRansacThreads) void k_ransac_rigid(RansacArgs a)
{
    __shared__ float pt_s[6][kRansacStage];
    __shared__ uint32_t pos_s[kRansacStage];
    __shared__ uint32_t wcnt_s[kRansacWaves];
    __shared__ unsigned long long best_s[kRansacWaves];
    const uint32_t sg = blockIdx.x, tid = threadIdx.x;
    const uint32_t lane = tid & 63u, wv = tid >> 6;
    const RansacSeg S = a.seg[sg];
    MatchPair P;
    P.qbase = P.nq = P.tbase = P.nt = 0;
    if constexpr (kChain) P = a.m.pairs[sg];
    const uint32_t n_steps = (S.n + kRansacThreads - 1) / kRansacThreads;

    // 1. the candidates, in ascending position
    uint32_t m = 0;
    for (uint32_t st = 0; st < n_steps; ++st) {
        const uint32_t i = st * kRansacThreads + tid;
        float p[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const bool cand = i < S.n && ransac_load<kChain>(a, S, P, i, p);
        const unsigned long long bal = __ballot(cand);
        if (lane == 0) wcnt_s[wv] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < (uint32_t)kRansacWaves; ++w) {
            const uint32_t c = wcnt_s[w];
            before += w < wv ? c : 0u;
            total += c;
        }
        if (cand) {
            const uint32_t r = m + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
            if (r < (uint32_t)kRansacStage) {
#pragma unroll
                for (int k = 0; k < 6; ++k) pt_s[k][r] = p[k];
                pos_s[r] = i;
            } else {
                a.over[S.over0 + (r - kRansacStage)] = i;
            }
        }
        m += total;
        __syncthreads();  // (wcnt_s is rewritten by the next step; the staged candidates and the list are read below)
    }

    // 2. the hypotheses, round-robin over the waves
    const uint64_t seed_s = splitmix64(a.seed ^ S.key);
    unsigned long long best = 0ull;  // score << 32 | ~h; a score below 3 is no model
    if (m >= 3u) {
        for (uint32_t h = wv; h < a.iterations; h += kRansacWaves) {
            double T[12];
            uint32_t pos[3];
            uint32_t score = 0;
            if (ransac_hypothesis<kChain>(a, S, P, seed_s, h, m, pt_s, pos_s, T, pos)) {  // (uniform over the wave)
                for (uint32_t r0 = 0; r0 < m; r0 += kWave) {
                    const uint32_t r = r0 + lane;
                    float p[6];
                    bool in = false;
                    if (r < m) {
                        (void)ransac_candidate<kChain>(a, S, P, r, pt_s, pos_s, p);
                        in = ransac_inlier(T, p, a.thr2);
                    }
                    score += (uint32_t)__popcll(__ballot(in));
                }
            }
            const unsigned long long key = ((unsigned long long)score << 32) | (unsigned long long)(0xFFFFFFFFu - h);
            if (key > best) best = key;
        }
    }
    // 3. the winner: greatest score, then lowest h
    if (lane == 0) best_s[wv] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kRansacWaves; ++w) best = best_s[w] > best ? best_s[w] : best;
    const uint32_t score = (uint32_t)(best >> 32), hbest = 0xFFFFFFFFu - (uint32_t)best;
    const bool ok = score >= 3u;

    // 4. the mask and the record
    double T[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
    uint32_t pos[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    if (ok) (void)ransac_hypothesis<kChain>(a, S, P, seed_s, hbest, m, pt_s, pos_s, T, pos);
    for (uint32_t st = 0; st < n_steps; ++st) {
        const uint32_t i = st * kRansacThreads + tid;
        if (i >= S.n) break;
        float p[6];
        const bool in = ok && ransac_load<kChain>(a, S, P, i, p) && ransac_inlier(T, p, a.thr2);
        a.inlier[S.start + i] = in ? 1 : 0;
    }
    if (tid == 0) {
        o3dr_ransac_result r;
        for (int k = 0; k < 12; ++k) r.T[k] = T[k];
        r.n_candidates = (int32_t)m;
        r.n_inliers = ok ? (int32_t)score : 0;
        r.best_hypothesis = ok ? (int32_t)hbest : -1;
        for (int k = 0; k < 3; ++k) r.sample[k] = ok ? (int32_t)pos[k] : -1;
        r.status = ok ? O3DR_RANSAC_OK : m < 3u ? O3DR_RANSAC_TOO_FEW : O3DR_RANSAC_NO_MODEL;
        r.reserved = 0;
        a.res[sg] = r;
    }
}
