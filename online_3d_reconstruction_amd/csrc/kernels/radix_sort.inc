// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// K2b — stable LSD radix sort of (voxel index, point id).
//   PCL sorts with std::sort (order inside a voxel unspecified); the canonical order here is the
//   stable one: points of a voxel stay in ascending input order.  Each frame sorts only the bits its
//   index can take, in g.passes passes of g.bpp <= kMaxRadixBits bits (k_voxel_geom); pass p reads
//   buffer (p + buf0)&1 and writes the other.  A workgroup owns 8192 consecutive records, a wave 1024 of
//   them, a lane 16 consecutive ones; ranks come from per-lane LDS counters (k_radix_scatter_lane): no
//   cross-lane races, hence stable and deterministic.
// =================================================================================================
// Where a tile's digit count lives.  Digit-major rows ([digit][tile]: what the multi-workgroup scan walks) cost the
// histogram kernels one lone dword store per digit and array (~8 ns each: 0.25 ms per 200-frame step) and the scatter as
// many lone loads; tile-major rows ([tile][digit], `tm`) are one 512-byte store / load per workgroup, and the scan of a
// frame's row (k_scan_hist_tm: one workgroup, the row staged in LDS) walks them in digit-major order.
__device__ __forceinline__ int64_t hist_at(bool tm, int dgt, int tile, int n_tiles)
{
    return tm ? (int64_t)tile * kMaxRadix + dgt : (int64_t)dgt * n_tiles + tile;
}

__global__ __launch_bounds__(kSortThreads) void k_radix_hist(const uint32_t* __restrict__ keys0,
                                                             const uint32_t* __restrict__ keys1, int64_t cap,
                                                             const VoxelGeom* __restrict__ geom, int pass,
                                                             int n_tiles, uint32_t* __restrict__ hist,
                                                             uint32_t* __restrict__ hist_part, int tm)
{
    // private tables per wave AND per lane quarter (4 x 8 x 128 counters): an LDS add only collides
    // with the 15 other lanes of its quarter, and those spread over 128 bins
    constexpr int kSub = 4;
    __shared__ uint32_t h[kSub * kSortWaves * kMaxRadix];
    const int f = blockIdx.y, tile = blockIdx.x;  // (XCD-contiguous tile order costs this read-only kernel 10 %)
    const VoxelGeom g = geom[f];
    if (g.overflow || pass >= (int)g.passes) return;
    const uint32_t n = g.n;
    if ((int64_t)tile * kSortTile >= (int64_t)n) return;  // (a tile without records: the scans read its entries as zero)
    const int bins = geom_bins(g), shift = pass * (int)g.bpp;
    const uint32_t dmask = (uint32_t)bins - 1u;
    for (int i = threadIdx.x; i < kSub * kSortWaves * kMaxRadix; i += kSortThreads) h[i] = 0;
    __syncthreads();
    const uint32_t* src = (((pass + g.buf0) & 1) ? keys1 : keys0) + (int64_t)f * cap;
    const int64_t base = (int64_t)tile * kSortTile;
    uint32_t* hw = h + (((threadIdx.x >> 6) * kSub) + (threadIdx.x & (kSub - 1))) * kMaxRadix;
    if (base < n) {
        // a histogram does not care which lane sees which record: 16-byte loads, 4 per lane
        const bool vec = (((int64_t)f * cap) & 3) == 0;  // tile bases are multiples of 8192
        // (round r covers records [2048 r, 2048 r + 2048) of the tile: two rounds per scatter part)
        static_assert(kScatParts == 2 && kSortRounds / 4 == 4, "the first scatter part is rounds 0 and 1");
        uint4 v[kSortRounds / 4];
        bool whole[kSortRounds / 4];
#pragma unroll
        for (int r = 0; r < kSortRounds / 4; ++r) {
            const int64_t i = base + ((int64_t)r * kSortThreads + threadIdx.x) * 4;
            whole[r] = vec && i + 3 < n;
            if (whole[r]) v[r] = stream_load_u4(reinterpret_cast<const uint4*>(src + i));
        }
#pragma unroll
        for (int r = 0; r < kSortRounds / 4; ++r) {
            const int64_t i = base + ((int64_t)r * kSortThreads + threadIdx.x) * 4;
            if (r == kSortRounds / 8) {  // the first part is counted: its digit counts go to hist_part
                __syncthreads();
                for (int dgt = threadIdx.x; dgt < bins; dgt += kSortThreads) {
                    uint32_t t = 0;
#pragma unroll
                    for (int ww = 0; ww < kSub * kSortWaves; ++ww) t += h[ww * kMaxRadix + dgt];
                    hist_part[(int64_t)f * kMaxRadix * n_tiles + hist_at(tm != 0, dgt, tile, n_tiles)] = t;
                }
                __syncthreads();  // (the counting goes on in the same tables)
            }
            if (whole[r]) {
                atomicAdd(&hw[(v[r].x >> shift) & dmask], 1u);
                atomicAdd(&hw[(v[r].y >> shift) & dmask], 1u);
                atomicAdd(&hw[(v[r].z >> shift) & dmask], 1u);
                atomicAdd(&hw[(v[r].w >> shift) & dmask], 1u);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (i + k < n) atomicAdd(&hw[(src[i + k] >> shift) & dmask], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t* dst = hist + (int64_t)f * kMaxRadix * n_tiles;
    for (int dgt = threadIdx.x; dgt < bins; dgt += kSortThreads) {
        uint32_t t = 0;
#pragma unroll
        for (int ww = 0; ww < kSub * kSortWaves; ++ww) t += h[ww * kMaxRadix + dgt];
        dst[hist_at(tm != 0, dgt, tile, n_tiles)] = t;
    }
}

// PCL's index per point + k_radix_hist of pass 0 in one read of the points (clouds that arrive as points): one
// workgroup = one sort tile; the indices are written for the scatter, their lowest digit is counted on the way.
__global__ __launch_bounds__(kSortThreads) void k_voxel_keys_hist0(const o3dr_point* __restrict__ in, int64_t in_fstride,
                                                                   const VoxelGeom* __restrict__ geom, float z_offset,
                                                                   int64_t cap, uint32_t* __restrict__ keys, int n_tiles,
                                                                   uint32_t* __restrict__ hist, uint32_t* __restrict__ hist_part,
                                                                   const VoxelGeom* __restrict__ skip_grouped, int tm)
{
    constexpr int kSub = 4;
    __shared__ uint32_t h[kSub * kSortWaves * kMaxRadix];
    const int f = blockIdx.y, tile = blockIdx.x;
    const VoxelGeom g = geom[f];
    if (g.overflow || g.n == 0u || g.passes == 0u) return;  // (an empty frame has no sort: nothing reads its row)
    if (skip_grouped && skip_grouped[f].grouped != 0u) return;  // whole-cloud call that sorts group runs, not points
    const uint32_t n = g.n;
    const int64_t base = (int64_t)tile * kSortTile;
    if (base >= (int64_t)n) return;  // (a tile without records: the scans read its entries as zero)
    const int bins = geom_bins(g);
    const uint32_t dmask = (uint32_t)bins - 1u;
    for (int i = threadIdx.x; i < kSub * kSortWaves * kMaxRadix; i += kSortThreads) h[i] = 0;
    __syncthreads();
    const uint4* src = reinterpret_cast<const uint4*>(in + (int64_t)f * in_fstride);
    uint32_t* dst = keys + (int64_t)f * cap;
    uint32_t* hw = h + (((threadIdx.x >> 6) * kSub) + (threadIdx.x & (kSub - 1))) * kMaxRadix;
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
        const int64_t i = base + (int64_t)r * kSortThreads + threadIdx.x;
        if (r == kSortRounds / kScatParts) {  // the first scatter part of the tile is counted (k_radix_hist)
            __syncthreads();
            for (int dgt = threadIdx.x; dgt < bins; dgt += kSortThreads) {
                uint32_t t = 0;
#pragma unroll
                for (int ww = 0; ww < kSub * kSortWaves; ++ww) t += h[ww * kMaxRadix + dgt];
                hist_part[(int64_t)f * kMaxRadix * n_tiles + hist_at(tm != 0, dgt, tile, n_tiles)] = t;
            }
            __syncthreads();  // (the counting goes on in the same tables)
        }
        if (i < n) {
            const uint32_t key = voxel_key_of(src[i], g, z_offset);
            dst[i] = key;
            atomicAdd(&hw[key & dmask], 1u);
        }
    }
    __syncthreads();
    uint32_t* hd = hist + (int64_t)f * kMaxRadix * n_tiles;
    for (int dgt = threadIdx.x; dgt < bins; dgt += kSortThreads) {
        uint32_t t = 0;
#pragma unroll
        for (int ww = 0; ww < kSub * kSortWaves; ++ww) t += h[ww * kMaxRadix + dgt];
        hd[hist_at(tm != 0, dgt, tile, n_tiles)] = t;
    }
}

// Lane-counting stable scatter (classic, per-tile histogram offsets).  A lane owns 16
// CONSECUTIVE records, so input order = (lane, slot) order and ranking needs no cross-lane matching:
//   A. every lane adds 1 to its own 7-bit field of cnt[digit][lane/4] (four lanes share a dword) with a
//      returning LDS add: the old field is the record's rank among the lane's earlier records;
//   B. per digit row (one lane per row): running sum over the 16 dwords; each dword becomes
//      [31:21] = records of lower lane-quads, [20:0] = the records of the lanes below lane 1, 2, 3 of the quad
//      (prefixes of the four counts by two shift-adds: 6 VALU instructions per dword; unpacking bytes and repacking
//      5-bit counts took 14, 37 % of the kernel's instructions - and the kernel keeps the SIMDs' VALU ~60 % busy);
//   C. rank in wave = quad prefix + records of the lower lanes of the quad + own rank.
// ~300 VALU per 1024 records instead of ~1000 for wave-ballot matching, which PMC showed to be
// VALU-issue-bound (round 1).  Digits are at most 7 bits wide (kMaxRadix = 128).
constexpr int kCntStride = 17;  // dwords per digit row: 16 lane-quads + 1 pad (conflict-free row walks)
constexpr int kCntWords = kMaxRadix * kCntStride;  // per wave
constexpr int kRankWords = kScatWaves * kCntWords;
struct ScatterLds {
    __attribute__((aligned(16))) uint32_t smem[kRankWords > 2 * kScatTile ? kRankWords : 2 * kScatTile];  // rank counters, then keys | payloads staging
    uint32_t wave_tot[kScatWaves * kMaxRadix];  // per-wave digit totals -> exclusive wave prefixes
    uint32_t local_base[kMaxRadix];
    uint32_t delta[kMaxRadix];
    uint32_t scan_lds[kScatWaves + 1];
    // head flags from the last pass (ScatterJob::heads): digits seen in the look-back [0..3], digits that need it [4..7]
    uint32_t hmask[8];
    uint32_t lmin;  // ... and the low bits (below the pass's digit) of the part's first input record
};
struct ScatterJob {  // per launch, frame and workgroup
    const uint32_t *kin, *vin;
    uint32_t *kout, *vout;
    uint8_t* heads;          // last pass of a point sort: "this record starts a run", one byte per record at the record's
                             // output place, instead of kout (nothing else reads a point sort's sorted indices); else nullptr
    uint32_t low_mask;       // the index bits below this pass's digit
    const uint32_t* hist;    // the frame's scanned histogram rows
    const uint32_t* hist_part;  // ... and the digit counts of the first part of every tile
    int64_t begin, end;      // the records of this workgroup's part of its tile (at most kScatTile)
    uint32_t dmask;
    int shift, bins, pass, n_tiles;
    bool tm;                 // tile-major histogram rows (hist_at)
};

// Records of part `part` (of kScatParts) of sort tile `tile`.  Every pass but one cuts the frame's n records every
// kSortTile.  The first pass of a frame whose indices k_reproject_emit wrote AND counted (tile_off != nullptr: the
// scanned valid candidates per emit tile) cuts at candidate borders instead: sort tile t = the records of emit tiles
// [kEmitGroup t, kEmitGroup t + kEmitGroup), so that the workgroup that wrote them owned the tile's histogram row.  Such a
// part holds at most kScatTile records and may hold none; a stable sort does not care where its tiles are cut.
__device__ __forceinline__ void emit_part_range(const uint32_t* __restrict__ tile_off, int n_emit_tiles, int tile, int part,
                                                int64_t n, int64_t& begin, int64_t& end)
{
    if (tile_off) {
        constexpr int kPer = kEmitGroup / kScatParts;
        const int e0 = (tile * kScatParts + part) * kPer;
        begin = tile_off[e0];
        end = e0 + kPer < n_emit_tiles ? (int64_t)tile_off[e0 + kPer] : n;
    } else {
        begin = (int64_t)tile * kSortTile + (int64_t)part * kScatTile;
        end = begin + kScatTile < n ? begin + kScatTile : n;
    }
}

// the 16 consecutive records of this lane in part `part` of tile `tile` (+ this thread's scanned histogram entry): every
// global load of the workgroup is issued here, before any LDS work
__device__ __forceinline__ void scatter_load(const ScatterJob& J, int tile, int part, uint32_t (&key)[kSortRounds],
                                             uint32_t (&val)[kSortRounds], uint32_t& gstart, uint32_t& back)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t lbase = J.begin + (int64_t)w * kSortWaveItems + (int64_t)lane * kSortRounds;
    gstart = 0;
    back = 0;
    if (J.heads && w == kScatWaves - 1) {  // the 64 input records just before the part: first step of the look-back
        const int64_t j = J.begin - kWave + lane;
        if (j >= 0) back = J.kin[j];
    }
    if ((int)threadIdx.x < J.bins) {  // where this part's records of digit threadIdx.x go: after those of the parts before it
        gstart = J.hist[hist_at(J.tm, threadIdx.x, tile, J.n_tiles)];
        if (part != 0) gstart += J.hist_part[hist_at(J.tm, threadIdx.x, tile, J.n_tiles)];
    }
    // four-dword loads from wherever the part starts (a candidate-aligned part of a frame with invalid pixels starts on any
    // record; global_load_dwordx4 needs dword alignment only)
    if (lbase + kSortRounds <= J.end) {
#pragma unroll
        for (int q = 0; q < kSortRounds / 4; ++q) {
            const u32x4_a4_t k4 = *reinterpret_cast<const u32x4_a4_t*>(J.kin + lbase + 4 * q);
            key[4 * q] = k4.x; key[4 * q + 1] = k4.y; key[4 * q + 2] = k4.z; key[4 * q + 3] = k4.w;
        }
        if (J.pass != 0) {
#pragma unroll
            for (int q = 0; q < kSortRounds / 4; ++q) {
                const u32x4_a4_t v4 = *reinterpret_cast<const u32x4_a4_t*>(J.vin + lbase + 4 * q);
                val[4 * q] = v4.x; val[4 * q + 1] = v4.y; val[4 * q + 2] = v4.z; val[4 * q + 3] = v4.w;
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < kSortRounds; ++r) {
            const int64_t i = lbase + r;
            const bool ok = i < J.end;
            key[r] = ok ? J.kin[i] : 0xffffffffu;
            val[r] = (J.pass != 0 && ok) ? J.vin[i] : 0u;
        }
    }
    if (J.pass == 0) {  // the payload is the record's position in the input (point id, or group-run id)
#pragma unroll
        for (int r = 0; r < kSortRounds; ++r) val[r] = (uint32_t)(lbase + r);
    }
}

// Head flags from the last pass (J.heads != nullptr).  A record of the part starts a run of equal indices iff its
// predecessor in the OUTPUT differs.  Inside the part's sorted order that is the record before it, unless it is the part's first record of
// its digit v: then the predecessor is the last record with digit v among the input records before the part, if any.
// The input is sorted by the low bits (those below this pass's digit) and the part is a contiguous piece of it, so every
// record before the part has low bits <= Lmin, the low bits of the part's first record; the ones with low bits == Lmin
// are one contiguous block that ends just before the part.  So the record continues a run iff its low bits are Lmin and
// a record with digit v stands in that block.  One wave walks the block backwards, 64 records per step, ORing the digits
// it sees into a 128-bit mask, until the block ends, the frame starts, or every digit that the part's own records with
// low bits Lmin have is in the mask (a digit forces a long walk only across a gap in which it did not occur: at most
// 128 reads per record of a block, usually one 256-byte load per workgroup).  No waiting on other workgroups.
__device__ __forceinline__ void scatter_tile(const ScatterJob& J, ScatterLds& L, const uint32_t (&key)[kSortRounds],
                                             const uint32_t (&val)[kSortRounds], uint32_t gstart, uint32_t back)
{
    uint32_t* smem = L.smem;
    uint32_t* stage = L.smem;  // overlays the counters once every record knows its position
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t cnt = (uint32_t)(J.end - J.begin);
    const int64_t lbase = J.begin + (int64_t)w * kSortWaveItems + (int64_t)lane * kSortRounds;
    const int shift = J.shift, bins = J.bins;
    const uint32_t dmask = J.dmask;
    for (int i = threadIdx.x; i < kRankWords; i += kScatThreads) smem[i] = 0;
    if (J.heads) {
        if (threadIdx.x < 8) L.hmask[threadIdx.x] = 0;
        if (threadIdx.x == 0) L.lmin = key[0] & J.low_mask;  // (thread 0 holds the part's first record)
    }
    __syncthreads();
    const volatile uint32_t* hmask = L.hmask;
    const uint32_t lmin = J.heads ? L.lmin : 0u;

    // ---- A. own-lane ranks: four lanes share a dword, 7 bits each (a lane has at most 16 records of a digit)
    uint32_t* cw = smem + w * kCntWords;
    const int quad = lane >> 2, sub = lane & 3;
    const uint32_t fsh = 7u * (uint32_t)sub;
    uint32_t own[kSortRounds];
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
        own[r] = 0;
        if (lbase + r < J.end) {
            const uint32_t dgt = (key[r] >> shift) & dmask;
            const uint32_t old = atomicAdd(&cw[dgt * kCntStride + quad], 1u << fsh);
            own[r] = (old >> fsh) & 127u;
            // (the digits whose first record of the part may continue a run from before the part)
            if (J.heads && (key[r] & J.low_mask) == lmin && !((hmask[4 + (dgt >> 5)] >> (dgt & 31u)) & 1u))
                atomicOr(&L.hmask[4 + (dgt >> 5)], 1u << (dgt & 31u));
        }
    }
    __builtin_amdgcn_wave_barrier();
    // ---- B. per digit row (lanes 0..63 take rows lane and lane+64): the four counts of a dword become prefixes with
    // two shift-adds (7-bit fields: c0, c0+c1, c0+c1+c2 <= 48, total <= 64), the word keeps the three a lane can need
    // in [20:0] and the records of the lower lane-quads in [31:21]
#pragma unroll
    for (int h = 0; h < kMaxRadix / 64; ++h) {
        const int row = lane + 64 * h;
        if (row < bins) {
            uint32_t run = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t v = cw[row * kCntStride + j];
                const uint32_t t = v + (v << 7);
                const uint32_t t2 = t + (t << 14);
                cw[row * kCntStride + j] = (run << 21) | (t2 & 0x1fffffu);
                run += (t2 >> 21) & 127u;
            }
            L.wave_tot[w * kMaxRadix + row] = run;
        }
    }
    __syncthreads();
    if (J.heads && w == kScatWaves - 1) {  // the look-back (see above); `back` = input records [J.begin - 64, J.begin)
        int64_t j0 = J.begin - kWave;
        uint32_t kb = back;
        for (;;) {
            const bool in = j0 + lane >= 0 && (kb & J.low_mask) == lmin;
            if (in) {
                const uint32_t dgt = (kb >> shift) & dmask;
                atomicOr(&L.hmask[dgt >> 5], 1u << (dgt & 31u));
            }
            __builtin_amdgcn_wave_barrier();
            if (__ballot(in) != ~0ull || j0 <= 0) break;  // the block ends inside these 64, or they start the frame
            uint32_t miss = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) miss |= hmask[4 + q] & ~hmask[q];
            if (miss == 0u) break;
            j0 -= kWave;
            kb = j0 + lane >= 0 ? J.kin[j0 + lane] : 0u;
        }
    }

    // ---- 2. one digit per thread: wave prefixes, part total, local start, global delta
    uint32_t tot = 0;
    const int dg = threadIdx.x;
    if (dg < bins) {
#pragma unroll
        for (int ww = 0; ww < kScatWaves; ++ww) {
            const uint32_t t = L.wave_tot[ww * kMaxRadix + dg];
            L.wave_tot[ww * kMaxRadix + dg] = tot;
            tot += t;
        }
    }
    uint32_t tile_total;
    const uint32_t lb = block_excl_scan_u32<kScatWaves>(tot, L.scan_lds, tile_total);
    if (dg < bins) {
        L.local_base[dg] = lb;
        L.delta[dg] = gstart - lb;
    }
    __syncthreads();

    // ---- C. positions inside the part's sorted order
    uint32_t pos[kSortRounds];
    const uint32_t qsh = sub ? 7u * (uint32_t)(sub - 1) : 0u, qmk = sub ? 127u : 0u;  // where the lower lanes' records of the quad stand
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
        if (lbase + r < J.end) {
            const uint32_t dgt = (key[r] >> shift) & dmask;
            const uint32_t v = cw[dgt * kCntStride + quad];
            pos[r] = L.local_base[dgt] + L.wave_tot[w * kMaxRadix + dgt] + (v >> 21) + ((v >> qsh) & qmk) + own[r];
        }
    }
    __syncthreads();  // the staging buffers overlay the counters: everyone is done reading them
    // keys and payloads are staged together (2 x 16 KiB inside the counters' 34 KiB): one exchange instead of two
    uint32_t* stage_v = L.smem + kScatTile;
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
        if (lbase + r < J.end) {
            stage[pos[r]] = key[r];
            stage_v[pos[r]] = val[r];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSortRounds; ++r) {
        const uint32_t p = r * kScatThreads + threadIdx.x;
        if (p < cnt) {
            const uint32_t k = stage[p];
            const uint32_t dgt = (k >> shift) & dmask;
            const uint32_t d = p + L.delta[dgt];
            J.vout[d] = stage_v[p];
            if (J.heads) {
                // (consecutive lanes hold consecutive places of a digit run: byte stores to consecutive addresses)
                bool head;
                if (p != L.local_base[dgt])
                    head = k != stage[p - 1];
                else
                    head = !((k & J.low_mask) == lmin && ((hmask[dgt >> 5] >> (dgt & 31u)) & 1u));
                J.heads[d] = head ? 1 : 0;
            } else {
                J.kout[d] = k;
            }
        }
    }
}

// One workgroup of kScatWaves waves per PART of a tile (half of its 8192 records).  The histogram rows stay per tile;
// a part's records of a digit follow those of the parts before it (hist_part, counted by the histogram kernels).  Measured:
// the kernel is bound by its chain of LDS phases, not by bytes (48-bit records between the passes, 20 % fewer bytes,
// left it at 2.09 ms; profiles/r02_packed_records_experiment.json): four 4-wave workgroups per CU overlap those
// phases better than two 8-wave ones, while 4096-record histogram tiles would cost more in the histogram and scan
// kernels than the scatter gains.  (Two tiles per workgroup with the second tile's loads issued early: 4.2 ms against
// 2.8 - 137 VGPRs, one workgroup per CU.)
__global__ __launch_bounds__(kScatThreads) void k_radix_scatter_lane(uint32_t* __restrict__ keys0, uint32_t* __restrict__ vals0,
                                                                     uint32_t* __restrict__ keys1, uint32_t* __restrict__ vals1,
                                                                     int64_t cap, const VoxelGeom* __restrict__ geom, int pass,
                                                                     int n_tiles, const uint32_t* __restrict__ hist_scanned,
                                                                     const uint32_t* __restrict__ hist_part, int tm,
                                                                     const uint32_t* __restrict__ emit_tile_off,
                                                                     int n_emit_tiles, uint8_t* __restrict__ side,
                                                                     int64_t side_stride)
{
    __shared__ ScatterLds L;
    const int f = blockIdx.y;
    const VoxelGeom g = geom[f];
    if (g.overflow || pass >= (int)g.passes) return;
    // candidate-aligned tiles (emit_part_range): every part of the frame's emit tiles is an item, empty ones included
    const uint32_t* tile_off = emit_tile_off ? emit_tile_off + (int64_t)f * n_emit_tiles : nullptr;
    const int n_items = tile_off ? (n_emit_tiles + kEmitGroup / kScatParts - 1) / (kEmitGroup / kScatParts)
                                 : (int)(((int64_t)g.n + kScatTile - 1) / kScatTile);
    // XCD-contiguous order (gridDim.x is a multiple of 8): a part's 128 output runs (~128 bytes each, unaligned)
    // continue the runs of the part before it, and the lines they share are completed in one L2 instead of being
    // written back in pieces by two: 2.57 -> 2.06 ms per 200-frame step
    const int item = xcd_chunk_item(blockIdx.x, n_items);
    if (item < 0) return;
    const int tile = item / kScatParts, part = item % kScatParts;
    ScatterJob J;
    emit_part_range(tile_off, n_emit_tiles, tile, part, (int64_t)g.n, J.begin, J.end);
    if (J.begin >= J.end) return;
    const int par = (pass + (int)g.buf0) & 1;  // which of the two buffers this pass reads
    J.kin = (par ? keys1 : keys0) + (int64_t)f * cap;
    J.vin = (par ? vals1 : vals0) + (int64_t)f * cap;
    J.kout = (par ? keys0 : keys1) + (int64_t)f * cap;
    J.vout = (par ? vals0 : vals1) + (int64_t)f * cap;
    J.hist = hist_scanned + (int64_t)f * kMaxRadix * n_tiles;
    J.hist_part = hist_part + (int64_t)f * kMaxRadix * n_tiles;
    J.bins = geom_bins(g);
    J.dmask = (uint32_t)J.bins - 1u;
    J.shift = pass * (int)g.bpp;
    J.pass = pass;
    J.n_tiles = n_tiles;
    J.tm = tm != 0;
    // side (point sorts in launch_voxel_grid): the last pass leaves the run-head flag of every record, for k_run_heads (side_heads_tile)
    J.heads = (side && pass + 1 == (int)g.passes) ? side + (int64_t)f * side_stride : nullptr;
    J.low_mask = (1u << J.shift) - 1u;
    uint32_t key0[kSortRounds], val0[kSortRounds], g0, back;
    scatter_load(J, tile, part, key0, val0, g0, back);
    scatter_tile(J, L, key0, val0, g0, back);
}
