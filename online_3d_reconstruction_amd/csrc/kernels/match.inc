// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Feature matching (o3dr_match_knn2_hamming, o3dr_keypoints_3d, o3dr_estimate_rigid_transform; DESIGN.md "Feature matching")
//   k_match_scan: one WORK ITEM = one wave = (pair, 64 consecutive query rows, one chunk of chunk_rows consecutive train
//   rows).  A lane keeps its query row's 8 dwords in registers; the train rows are wave-uniform, so they come in as scalar
//   loads (a separate __restrict__ argument, uniform index).  Per train row: 8 xor + 8 accumulating bit counts, then a
//   branch-free top-2 update on a packed 32-bit key (d << 23 | row inside the chunk): min, max, min.  The wave writes its
//   two keys per query row as the chunk's partial.  Items run chunk-major inside a pair (the waves of a workgroup share
//   their train rows).
//   k_match_fold: one lane per record folds the pair's chunk partials in chunk order into (d, global row) keys.  The keys
//   are a total order, so the records do not depend on the chunk size.
//   k_keypoints_3d: one lane per keypoint, the keypoint pass's own per-keypoint body (keypoint_one, kernels/reproject.inc).
//   k_rigid_first / k_rigid_sums / k_rigid_fold: per-segment rigid_moments (or rigid_residual2) over runs of 256 points
//   from the segment's first point, wave_fields and tree4 per run, fold_partials per segment (kernels/rigid_core.inc);
//   the host solves each record with rigid_solve (o3dr_rigid_solve.h).
// =================================================================================================
constexpr int kMatchThreads = 256;          // four work items per workgroup
constexpr int kMatchKeyBits = 23;           // row-inside-chunk bits of a key (d <= 256 takes the upper 9)
constexpr uint32_t kMatchNone = 0xFFFFFFFFu;
constexpr int kMatchUnroll = 4;             // train rows per step of the hot loop
static_assert(kMatchThreads == 4 * kWave, "k_match_scan: four waves per workgroup");
static_assert((uint32_t)kMatchMaxChunk <= (1u << kMatchKeyBits), "the row inside a chunk must fit the key");

// the top-2 of packed keys (keys are distinct, b1 < b2)
__device__ __forceinline__ void match_top2(uint32_t key, uint32_t& b1, uint32_t& b2)
{
    const uint32_t hi = b1 > key ? b1 : key;
    b1 = b1 < key ? b1 : key;
    b2 = b2 < hi ? b2 : hi;
}

__device__ __forceinline__ uint32_t match_dist(const uint32_t q[8], const uint4 t0, const uint4 t1)
{
    uint32_t d = __builtin_popcount(q[0] ^ t0.x);
    d += __builtin_popcount(q[1] ^ t0.y);
    d += __builtin_popcount(q[2] ^ t0.z);
    d += __builtin_popcount(q[3] ^ t0.w);
    d += __builtin_popcount(q[4] ^ t1.x);
    d += __builtin_popcount(q[5] ^ t1.y);
    d += __builtin_popcount(q[6] ^ t1.z);
    d += __builtin_popcount(q[7] ^ t1.w);
    return d;
}

// the pair of a wave-uniform work item / record: the LAST pair whose first item (record) is <= it (pairs without items or
// records share their first one with the next pair and are skipped that way)
__device__ __forceinline__ uint32_t match_find_pair(const MatchPair* __restrict__ pairs, uint32_t n_pairs, uint64_t v, bool by_item)
{
    uint32_t lo = 0, hi = n_pairs - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        const uint64_t s = by_item ? pairs[mid].item0 : pairs[mid].rec0;
        if (s <= v)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kMatchThreads) void k_match_scan(MatchArgs a, const MatchPair* __restrict__ pairs,
                                                              const uint4* __restrict__ train, uint2* __restrict__ partial,
                                                              uint64_t item_off)
{
    const uint64_t w = item_off + (uint64_t)blockIdx.x * (kMatchThreads / kWave) +
                       (uint64_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w >= a.n_items) return;
    const int lane = threadIdx.x & 63;
    const uint32_t p = match_find_pair(pairs, a.n_pairs, w, true);
    const MatchPair P = pairs[p];
    const uint32_t local = (uint32_t)(w - P.item0);
    const uint32_t chunk = local / P.qwaves, qb = local - chunk * P.qwaves;
    const uint32_t row = qb * (uint32_t)kWave + (uint32_t)lane;
    const bool valid = row < P.nq;
    uint32_t q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (valid) {
        const uint4 v0 = a.desc[2 * ((uint64_t)P.qbase + row)], v1 = a.desc[2 * ((uint64_t)P.qbase + row) + 1];
        q[0] = v0.x, q[1] = v0.y, q[2] = v0.z, q[3] = v0.w;
        q[4] = v1.x, q[5] = v1.y, q[6] = v1.z, q[7] = v1.w;
    }
    const uint32_t j0 = chunk * a.chunk_rows;
    const uint32_t n = P.nt - j0 < a.chunk_rows ? P.nt - j0 : a.chunk_rows;
    const uint4* tp = train + 2 * ((uint64_t)P.tbase + j0);
    uint32_t b1 = kMatchNone, b2 = kMatchNone;
    uint32_t j = 0;
    for (; j + kMatchUnroll <= n; j += kMatchUnroll) {
        uint4 t[2 * kMatchUnroll];
#pragma unroll
        for (int u = 0; u < 2 * kMatchUnroll; ++u) t[u] = tp[2 * (uint64_t)j + u];
#pragma unroll
        for (int u = 0; u < kMatchUnroll; ++u) match_top2((match_dist(q, t[2 * u], t[2 * u + 1]) << kMatchKeyBits) | (j + u), b1, b2);
    }
    for (; j < n; ++j) match_top2((match_dist(q, tp[2 * (uint64_t)j], tp[2 * (uint64_t)j + 1]) << kMatchKeyBits) | j, b1, b2);
    if (valid) partial[P.part0 + (uint64_t)chunk * P.nq + row] = make_uint2(b1, b2);
}

__device__ __forceinline__ void match_top2_u64(uint64_t key, uint64_t& b1, uint64_t& b2)
{
    const uint64_t hi = b1 > key ? b1 : key;
    b1 = b1 < key ? b1 : key;
    b2 = b2 < hi ? b2 : hi;
}

__global__ __launch_bounds__(256) void k_match_fold(MatchArgs a, const MatchPair* __restrict__ pairs, const uint2* __restrict__ partial)
{
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < a.n_rec; r += (uint64_t)gridDim.x * 256) {
        const MatchPair P = pairs[match_find_pair(pairs, a.n_pairs, r, false)];
        const uint32_t i = (uint32_t)(r - P.rec0);
        uint64_t b1 = ~0ull, b2 = ~0ull;  // (d << 32) | global train row
        for (uint32_t c = 0; c < P.chunks; ++c) {
            const uint2 k = partial[P.part0 + (uint64_t)c * P.nq + i];
            const uint64_t base = (uint64_t)c * a.chunk_rows;
            const uint32_t mask = (1u << kMatchKeyBits) - 1u;
            if (k.x != kMatchNone) match_top2_u64(((uint64_t)(k.x >> kMatchKeyBits) << 32) | (base + (k.x & mask)), b1, b2);
            if (k.y != kMatchNone) match_top2_u64(((uint64_t)(k.y >> kMatchKeyBits) << 32) | (base + (k.y & mask)), b1, b2);
        }
        const bool h1 = b1 != ~0ull, h2 = b2 != ~0ull;
        const uint32_t d1 = h1 ? (uint32_t)(b1 >> 32) : kMatchNone, d2 = h2 ? (uint32_t)(b2 >> 32) : kMatchNone;
        a.rec[r] = make_uint4(h1 ? (uint32_t)b1 : kMatchNone, h2 ? (uint32_t)b2 : kMatchNone, d1, d2);
        if (a.good) a.good[r] = (h2 && d1 < a.max_distance && (float)d1 < a.ratio * (float)d2) ? 1 : 0;
    }
}

// ---- the one lookup of a matched row ----------------------------------------------------------------
// Query row `row` of pair P through what the matching pass left (MatchedPairs): the record r = P.rec0 + row, the good
// gate, the best train row ti and its gate ti < P.nt (a good row has both neighbours), the two keypoints as float4 and the
// RANSAC's byte.  chain_slot, ransac_load<true> and k_graph_moments read a row through it and add what is their own.
// qbase is the query set's first row: P.qbase, which the chain passes as its frame's ChainFrameIn::qbase (pose_chain fills
// both from the same offsets, so they are equal; with the pair's value k_pose_chain measured 2.5 % slower, DESIGN.md
// "Matched pairs").  The RANSAC's RansacSeg::start likewise repeats P.rec0.  points == false: only `good` is wanted.
struct MatchedRow {
    bool good;    // the matcher's byte
    bool hit;     // good and ti < nt: s and t are loaded
    bool in;      // the RANSAC kept the record (true without a filter)
    uint32_t ti;  // the train row inside its set
    float4 s, t;  // the query row's keypoint, the train row's
};
__device__ __forceinline__ MatchedRow matched_row(const MatchedPairs& M, const MatchPair& P, uint32_t qbase, uint32_t row, bool points = true)
{
    MatchedRow o;
    o.good = o.hit = false;
    o.in = true;
    o.ti = kMatchNone;
    o.s = o.t = make_float4(0.f, 0.f, 0.f, 0.f);
    const uint64_t r = P.rec0 + row;
    if (!M.good[r]) return o;
    o.good = true;
    if (!points) return o;
    o.ti = M.rec[r].x;
    if (o.ti >= P.nt) return o;
    o.hit = true;
    o.s = reinterpret_cast<const float4*>(M.kp3)[(uint64_t)qbase + row];
    o.t = reinterpret_cast<const float4*>(M.kp3)[(uint64_t)P.tbase + o.ti];
    if (M.inlier && !M.inlier[r]) o.in = false;
    return o;
}

// ---- index-aligned 3-D keypoints --------------------------------------------------------------------
// one lane per keypoint; kp_off: n_frames + 1 int32 entries (relative to the first keypoint)
__global__ __launch_bounds__(256) void k_keypoints_3d(ReprojectArgs a, const float* __restrict__ kp_xy, const int32_t* __restrict__ kp_off,
                                                      int n_frames, int n_kp, o3dr_point* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_kp) return;
    int lo = 0, hi = n_frames - 1;  // the last frame whose first keypoint is <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (kp_off[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    const int f = lo;
    float m[12];
    const bool xf = a.xf_mode != 0;
    for (int k = 0; k < 12; ++k) m[k] = xf ? a.poses[16 * (int64_t)f + k] : 0.f;
    const uint8_t* disp = a.disp + (int64_t)f * a.disp_fstride;
    const uint8_t* bgr = a.bgr ? a.bgr + (int64_t)f * a.bgr_fstride : nullptr;
    Pix p;
    uint4 v = make_uint4(0x7fc00000u, 0x7fc00000u, 0x7fc00000u, 0u);  // rejected: NaN x y z, rgba 0
    if (keypoint_one(a, disp, bgr, m, xf, kp_xy[2 * (int64_t)i], kp_xy[2 * (int64_t)i + 1], p))
        v = make_uint4(__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(p.z), p.rgba);
    reinterpret_cast<uint4*>(out)[i] = v;
}

// ---- batched rigid fit: per-segment fp64 moments ----------------------------------------------------
constexpr int kRigidThreads = kRigidPoints;  // points per workgroup = the fixed partition of the sums
static_assert(kRigidThreads == kNnThreads, "the partition of ICP step 5");

__device__ __forceinline__ bool rigid_used(const RigidArgs& a, uint64_t i, float4& s, float4& t)
{
    s = reinterpret_cast<const float4*>(a.src)[i];
    t = reinterpret_cast<const float4*>(a.tgt)[i];
    if (a.mask && !a.mask[i]) return false;
    return pair_finite(s, t);
}

// the segment of a workgroup: the last segment whose first workgroup is <= b
__device__ __forceinline__ uint32_t rigid_seg(const RigidArgs& a, uint32_t b)
{
    uint32_t lo = 0, hi = a.n_segs - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (a.seg[mid].block0 <= b)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// first used pair of every segment (first[s] starts at 0xFFFFFFFF): one integer atomic per wave
__global__ __launch_bounds__(kRigidThreads) void k_rigid_first(RigidArgs a)
{
    const uint32_t b = blockIdx.x;
    const uint32_t sid = rigid_seg(a, b);
    const RigidSeg S = a.seg[sid];
    const uint32_t k = (b - S.block0) * kRigidThreads + threadIdx.x;
    float4 s, t;
    const bool used = k < S.n && rigid_used(a, S.start + k, s, t);
    const uint64_t bal = __ballot(used);
    if ((threadIdx.x & 63) == 0 && bal)
        atomicMin(&a.first[sid], (b - S.block0) * kRigidThreads + (threadIdx.x & ~63u) + (uint32_t)__builtin_ctzll(bal));
}

// kResidual == false: the 16 moments about c0 (count, sum a, sum b, sum a b^T); true: the squared residual at the
// segment's T (one field).  Partials field-major: partial[k * n_blocks + b]
template <bool kResidual>
__global__ __launch_bounds__(kRigidThreads) void k_rigid_sums(RigidArgs a)
{
    constexpr int F = kResidual ? 1 : kRigidFields;
    __shared__ double red[F][kRigidThreads / kWave];
    const uint32_t b = blockIdx.x;
    const uint32_t sid = rigid_seg(a, b);
    const RigidSeg S = a.seg[sid];
    const uint32_t k = (b - S.block0) * kRigidThreads + threadIdx.x;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), t = s;
    const bool used = k < S.n && rigid_used(a, S.start + k, s, t);
    double v[F];
    if constexpr (kResidual) {
        const double r2 = rigid_residual2(a.T + 12 * (uint64_t)sid, s, t);
        v[0] = used ? r2 : 0.0;
    } else {
        const uint32_t f = a.first[sid];
        double c0[3] = {0.0, 0.0, 0.0};
        if (f != 0xFFFFFFFFu) {
            const float4 c = reinterpret_cast<const float4*>(a.tgt)[S.start + f];
            c0[0] = c.x, c0[1] = c.y, c0[2] = c.z;
        }
        rigid_moments(used, s, t, c0, v);
    }
    wave_fields<F>(v, red, threadIdx.x & 63, threadIdx.x >> 6);
    __syncthreads();
    if (threadIdx.x < F) {
        const int f = threadIdx.x;
        a.partial[(uint64_t)f * a.n_blocks + b] = tree4(red[f]);
    }
}

// one workgroup per (segment, field): the segment's partials through fold_partials -> rec[segment * n_fields + field];
// field 0's workgroup also writes the segment's c0 (3 doubles)
__global__ __launch_bounds__(kRigidFoldThreads) void k_rigid_fold(RigidArgs a, int n_fields)
{
    __shared__ double red[kRigidFoldThreads / kWave];
    const int k = blockIdx.y;
    const uint32_t sid = blockIdx.x;
    const RigidSeg S = a.seg[sid];
    const uint32_t nb = (S.n + kRigidThreads - 1) / kRigidThreads;
    const double t = fold_partials(a.partial + (uint64_t)k * a.n_blocks + S.block0, nb, red);
    if (threadIdx.x == 0) {
        a.rec[(uint64_t)sid * n_fields + k] = t;
        if (k == 0 && a.c0) {
            const uint32_t f = a.first[sid];
            double c[3] = {0.0, 0.0, 0.0};
            if (f != 0xFFFFFFFFu) {
                const float4 p = reinterpret_cast<const float4*>(a.tgt)[S.start + f];
                c[0] = p.x, c[1] = p.y, c[2] = p.z;
            }
            for (int j = 0; j < 3; ++j) a.c0[3 * (uint64_t)sid + j] = c[j];
        }
    }
}
