// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// Incremental merge (o3dr_finalize_incremental): the combined 2.5-D merge of cloud_big kept as running per-cell sums.
// The state is every occupied cell of the merged grid as an IncCell (CentroidPoint's seven raw fp32 sums + the count),
// the cells sorted by ABSOLUTE (layer, row, x), and one IncGroup per occupied absolute voxel group (util.inc:
// group_coord_of) with its 32-bit occupancy mask; off[g] = cells of the groups before g.  A call folds the points
// appended since the previous one:
//   1. the tail's group runs are sorted by group with the merge's own kernels (launch_inc_runs: the merge's
//      group_run_front, radix_pass and segment_runs), over a grid laid on the whole cloud's box: a group key relative to that box orders like the absolute coordinates;
//   2. k_inc_fold: one wave per tail group, lane = cell, k_centroid_groups' LDS counting sort and front-to-back adds,
//      but every lane starts from its cell's stored sums (zero for a new cell) and the sums are kept instead of divided;
//   3. the tail's groups and the state's are merged by rank (k_inc_place_*), the cells move to their new places
//      (k_inc_copy); k_inc_snapshot divides, with k_centroid_groups' epilogue.
// Every cell's sums therefore see exactly the additions o3dr_finalize performs, in the same order (cloud_big order).
// =================================================================================================
__device__ __forceinline__ bool inc_less(const IncGroup& a, const IncGroup& b)
{
    if (a.iz != b.iz) return a.iz < b.iz;
    if (a.iy != b.iy) return a.iy < b.iy;
    return a.bx < b.bx;
}
__device__ __forceinline__ bool inc_same(const IncGroup& a, const IncGroup& b) { return a.iz == b.iz && a.iy == b.iy && a.bx == b.bx; }
// groups of g[0, n) ordered before `key` (g is sorted)
__device__ __forceinline__ uint32_t inc_lower_bound(const IncGroup* __restrict__ g, uint32_t n, const IncGroup& key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (inc_less(g[mid], key))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Step 2.  The sorted tail (launch_inc_runs: seg_start / sorted run ids / run_start over the tail's points `in`) is
// folded into the state (old_g / old_off / old_cells, n_old groups): tail group v's 32 cells -> scratch[32 v ..] (all
// of them, empty ones with n = 0), its absolute coordinates and new mask -> tg[v], the state group it extends (or
// kIncNone) -> tmatch[v].  Guards as in k_centroid_groups: a record or point id outside its range sets
// O3DR_STATUS_INTERNAL in cc and is never dereferenced.
constexpr uint32_t kIncNone = 0xffffffffu;
__global__ __launch_bounds__(kGroupWaves * kWave) void k_inc_fold(
    const o3dr_point* __restrict__ in, const uint32_t* __restrict__ keys0, const uint32_t* __restrict__ keys1,
    const uint32_t* __restrict__ ids0, const uint32_t* __restrict__ ids1, const uint32_t* __restrict__ seg_start,
    const uint32_t* __restrict__ run_start, const VoxelGeom* __restrict__ geom_runs, const VoxelGeom* __restrict__ geom_pts,
    const uint32_t* __restrict__ n_vox, float z_offset, const IncGroup* __restrict__ old_g, const uint32_t* __restrict__ old_off,
    const IncCell* __restrict__ old_cells, uint32_t n_old, uint32_t n_old_cells, IncCell* __restrict__ scratch, uint32_t n_scratch,
    IncGroup* __restrict__ tg, uint32_t* __restrict__ tmatch, CloudCounters* __restrict__ cc)
{
    __shared__ GroupLds lds[kGroupWaves];
    const VoxelGeom g = geom_runs[0];
    const VoxelGeom gp = geom_pts[0];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (g.grouped == 0u || g.overflow || gp.overflow) {  // (the host ruled both out: a bookkeeping error)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(&cc->status, O3DR_STATUS_INTERNAL);
        return;
    }
    GroupLds& L = lds[w];
#pragma unroll
    for (int q = 0; q < kGroupChunks; ++q) L.mask[lane][q] = 0ull;
    if (lane < kGroupChunks) L.bnd[lane] = 0ull;
    __builtin_amdgcn_wave_barrier();
    const uint32_t nv = n_vox[0], n_rec = g.n, n_points = gp.n;
    const uint32_t* sk = sorted_buf(g, keys0, keys1);
    const uint32_t* rv = sorted_buf(g, ids0, ids1);
    const uint4* src = reinterpret_cast<const uint4*>(in);
    const int32_t bx0 = gp.min_b[0] >> kGroupBits;
    const uint32_t nbx = group_blocks_x(gp);
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    const unsigned long long starts_upto = (2ull << lane) - 2ull;  // positions 1 .. lane of a chunk
    bool bad = nv > n_scratch;
    for (uint32_t v = blockIdx.x * kGroupWaves + w; v < nv && v < n_scratch; v += gridDim.x * kGroupWaves) {
        const uint32_t jb = seg_start[v], je = seg_start[v + 1];
        IncGroup key;
        uint32_t match = kIncNone;
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        f32x2 s_xy = {0.f, 0.f}, s_rg = {0.f, 0.f}, s_ba = {0.f, 0.f};
        float sz = 0.f;
        uint32_t n_pts = 0;
        if (jb >= je || je > n_rec) {
            bad = true;
            key.bx = key.iy = key.iz = 0;
        } else {
            const uint32_t group_key = sk[jb];
            // the group's absolute coordinates (group_key_of inverted)
            const uint32_t rest = group_key / nbx;
            key.bx = (int32_t)(group_key - rest * nbx) + bx0;
            key.iy = (int32_t)(rest % (uint32_t)gp.div_b[1]) + gp.min_b[1];
            key.iz = (int32_t)(rest / (uint32_t)gp.div_b[1]) + gp.min_b[2];
            const uint32_t at = inc_lower_bound(old_g, n_old, key);
            if (at < n_old && inc_same(old_g[at], key)) match = at;
            // every cell lane starts from the sums the state holds for it
            if (match != kIncNone && lane < kGroupCells) {
                const uint32_t m = old_g[match].mask;
                if ((m >> lane) & 1u) {
                    const uint32_t ci = old_off[match] + (uint32_t)__popc(m & (uint32_t)lanes_below);
                    if (ci < n_old_cells) {
                        const IncCell o = old_cells[ci];
                        s_xy = f32x2{o.s[0], o.s[1]};
                        sz = o.s[2];
                        s_rg = f32x2{o.s[3], o.s[4]};
                        s_ba = f32x2{o.s[5], o.s[6]};
                        n_pts = o.n;
                    } else {
                        bad = true;
                    }
                }
            }
            // ---- from here to the end of the run loop: k_centroid_groups' fold, unchanged ----
            const uint32_t jlast = je - 1u;
            auto id_load = [&](uint32_t j0) { return rv[(j0 + lane < je) ? j0 + lane : jlast]; };
            uint32_t id_c = id_load(jb);
            bool id_ok = id_c < n_rec;
            uint32_t rb = run_start[id_ok ? id_c : 0u], re = run_start[(id_ok ? id_c : 0u) + 1u];
            uint32_t id_n = id_load(jb + kWave);
            for (uint32_t j0 = jb; j0 < je; j0 += kWave) {
                uint32_t first = 0, len = 0;
                if (j0 + lane < je) {
                    if (id_ok && rb < re && re <= n_points) {
                        first = rb;
                        len = re - rb;
                    } else {
                        bad = true;
                    }
                }
                id_ok = id_n < n_rec;
                rb = run_start[id_ok ? id_n : 0u];
                re = run_start[(id_ok ? id_n : 0u) + 1u];
                id_n = id_load(j0 + 2 * kWave);
                const uint32_t incl = wave_incl_scan_u32(len);
                const uint32_t pprev = incl - len;
                const uint32_t delta = first - pprev;
                const uint32_t total = __shfl(incl, 63, 64);
                auto step_load = [&](uint32_t k0, uint4 (&p)[kGroupChunks], uint32_t& okm) {
                    if (len != 0u && pprev > k0 && pprev < k0 + kGroupStep) {
                        const uint32_t r = pprev - k0;
                        atomicOr(&L.bnd[r >> 6], 1ull << (r & 63u));
                    }
                    __builtin_amdgcn_wave_barrier();
                    okm = 0;
#pragma unroll
                    for (int q = 0; q < kGroupChunks; ++q) {
                        const uint32_t kq = k0 + (uint32_t)(q * kWave);
                        const uint32_t rbase = (uint32_t)__popcll(__ballot(incl <= kq));
                        const uint32_t ri = rbase + (uint32_t)__popcll(L.bnd[q] & starts_upto);
                        const uint32_t spos = kq + (uint32_t)lane;
                        const uint32_t pidx = __shfl(delta, (int)(ri & 63u), 64) + spos;
                        const bool ok = spos < total && ri < (uint32_t)kWave && pidx < n_points;
                        p[q] = src[ok ? pidx : 0u];
                        okm |= ok ? (1u << q) : 0u;
                    }
                    __builtin_amdgcn_wave_barrier();
                    if (lane < kGroupChunks) L.bnd[lane] = 0ull;
                };
                uint4 p[kGroupChunks];
                uint32_t okm;
                step_load(0, p, okm);
                for (uint32_t k0 = 0; k0 < total; k0 += kGroupStep) {
                    uint4 pn[kGroupChunks];
                    uint32_t okn;
                    step_load(k0 + kGroupStep, pn, okn);
                    uint32_t cq[kGroupChunks];
#pragma unroll
                    for (int q = 0; q < kGroupChunks; ++q) {
                        cq[q] = 0;
                        if (okm & (1u << q)) {
                            uint32_t c;
                            const uint32_t gk = group_key_of(group_coord_of(p[q], gp.inv, z_offset, c), gp);
                            if (gk != group_key) c = 0xffffffffu;
                            if (c < (uint32_t)kGroupCells) {
                                cq[q] = c;
                                atomicOr(&L.mask[c][q], 1ull << lane);
                            } else {
                                bad = true;
                                okm &= ~(1u << q);
                            }
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
                    uint32_t cnt = 0, off;
                    {
                        uint32_t cc4[kGroupChunks];
#pragma unroll
                        for (int q = 0; q < kGroupChunks; ++q) {
                            cc4[q] = (uint32_t)__popcll(L.mask[lane][q]);
                            cnt += cc4[q];
                        }
                        off = wave_incl_scan_u32(cnt) - cnt;
                        uint32_t run = off;
#pragma unroll
                        for (int q = 0; q < kGroupChunks; ++q) {
                            L.pre[lane][q] = run;
                            run += cc4[q];
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int q = 0; q < kGroupChunks; ++q) {
                        if (okm & (1u << q)) {
                            const uint32_t pos = (L.pre[cq[q]][q] + (uint32_t)__popcll(L.mask[cq[q]][q] & lanes_below)) &
                                                 (uint32_t)(kGroupStep - 1);
                            L.sorted[pos] = make_uint4(p[q].x, p[q].y, __float_as_uint(__uint_as_float(p[q].z) + z_offset), p[q].w);
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int q = 0; q < kGroupChunks; ++q) L.mask[lane][q] = 0ull;
                    n_pts += cnt;
                    const uint32_t trips = wave_max_u32(cnt);
                    for (uint32_t t = 0; t < trips; t += 4) {
                        uint4 a4[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const uint4* at4 = (t + j < cnt) ? &L.sorted[(off + t) & (uint32_t)(kGroupStep - 1)] : &L.sorted[0];
                            a4[j] = at4[j];
                        }
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (t + j < cnt) {
                                const uint32_t c4 = a4[j].w;
                                s_xy += f32x2{__uint_as_float(a4[j].x), __uint_as_float(a4[j].y)};
                                sz += __uint_as_float(a4[j].z);
                                s_rg += f32x2{(float)((c4 >> 16) & 255u), (float)((c4 >> 8) & 255u)};
                                s_ba += f32x2{(float)(c4 & 255u), (float)(c4 >> 24)};
                            }
                        }
                    }
                    __builtin_amdgcn_wave_barrier();
#pragma unroll
                    for (int q = 0; q < kGroupChunks; ++q) p[q] = pn[q];
                    okm = okn;
                }
            }
        }
        // the group's 32 cells, sums kept (not divided)
        const unsigned long long occ = __ballot(lane < kGroupCells && n_pts > 0u);
        if (lane < kGroupCells) {
            IncCell r;
            r.s[0] = s_xy.x;
            r.s[1] = s_xy.y;
            r.s[2] = sz;
            r.s[3] = s_rg.x;
            r.s[4] = s_rg.y;
            r.s[5] = s_ba.x;
            r.s[6] = s_ba.y;
            r.n = n_pts;
            scratch[(int64_t)v * kGroupCells + lane] = r;
        }
        if (lane == 0) {
            key.mask = (uint32_t)occ;
            tg[v] = key;
            tmatch[v] = match;
        }
    }
    if (bad) atomicOr(&cc->status, O3DR_STATUS_INTERNAL);
}

// Step 3a.  flag[t] = 1 for the tail groups the state does not have yet (flag[nt] = 0: the scan's total is their number)
__global__ __launch_bounds__(256) void k_inc_new_flags(const uint32_t* __restrict__ tmatch, uint32_t nt, uint32_t* __restrict__ flag)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t < nt) flag[t] = tmatch[t] == kIncNone ? 1u : 0u;
    if (t == nt) flag[t] = 0u;
}
// Step 3b.  Merge by rank: state group i lands at i + (new tail groups ordered before it); new tail group t at
// (new tail groups before t) + (state groups ordered before it).  src[g]: where group g's cells come from - the state's
// group i (i), or the fold's scratch of tail group t (kIncScratch | t); cnt[g] = its cells (scanned into new_off next).
constexpr uint32_t kIncScratch = 0x80000000u;
__global__ __launch_bounds__(256) void k_inc_place_old(const IncGroup* __restrict__ old_g, uint32_t n_old, const IncGroup* __restrict__ tg,
                                                       const uint32_t* __restrict__ tmatch, uint32_t nt,
                                                       const uint32_t* __restrict__ new_excl, IncGroup* __restrict__ new_g,
                                                       uint32_t* __restrict__ src, uint32_t* __restrict__ cnt, uint32_t n_new,
                                                       CloudCounters* __restrict__ cc)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_old) return;
    IncGroup gi = old_g[i];
    const uint32_t lb = inc_lower_bound(tg, nt, gi);
    const uint32_t pos = i + new_excl[lb];
    uint32_t s = i;
    if (lb < nt && inc_same(tg[lb], gi)) {
        if (tmatch[lb] != i) {
            atomicOr(&cc->status, O3DR_STATUS_INTERNAL);
            return;
        }
        gi.mask = tg[lb].mask;
        s = kIncScratch | lb;
    }
    if (pos >= n_new) {
        atomicOr(&cc->status, O3DR_STATUS_INTERNAL);
        return;
    }
    new_g[pos] = gi;
    src[pos] = s;
    cnt[pos] = (uint32_t)__popc(gi.mask);
}
__global__ __launch_bounds__(256) void k_inc_place_new(const IncGroup* __restrict__ old_g, uint32_t n_old, const IncGroup* __restrict__ tg,
                                                       const uint32_t* __restrict__ tmatch, uint32_t nt,
                                                       const uint32_t* __restrict__ new_excl, IncGroup* __restrict__ new_g,
                                                       uint32_t* __restrict__ src, uint32_t* __restrict__ cnt, uint32_t n_new,
                                                       CloudCounters* __restrict__ cc)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= nt || tmatch[t] != kIncNone) return;
    const IncGroup gt = tg[t];
    const uint32_t pos = new_excl[t] + inc_lower_bound(old_g, n_old, gt);
    if (pos >= n_new) {
        atomicOr(&cc->status, O3DR_STATUS_INTERNAL);
        return;
    }
    new_g[pos] = gt;
    src[pos] = kIncScratch | t;
    cnt[pos] = (uint32_t)__popc(gt.mask);
}
// Step 3c.  The cells to their new places: one thread per (group, cell)
__global__ __launch_bounds__(256) void k_inc_copy(const IncGroup* __restrict__ new_g, const uint32_t* __restrict__ new_off,
                                                  const uint32_t* __restrict__ src, uint32_t n_new, const uint32_t* __restrict__ old_off,
                                                  const IncCell* __restrict__ old_cells, uint32_t n_old, uint32_t n_old_cells,
                                                  const IncCell* __restrict__ scratch, uint32_t nt, IncCell* __restrict__ cells,
                                                  uint32_t cells_cap, CloudCounters* __restrict__ cc)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint32_t gi = (uint32_t)(k >> kGroupBits), c = (uint32_t)(k & (kGroupCells - 1));
    if (gi >= n_new) return;
    const uint32_t m = new_g[gi].mask;
    if (!((m >> c) & 1u)) return;
    const uint32_t rank = (uint32_t)__popc(m & ((1u << c) - 1u));
    const uint32_t dst = new_off[gi] + rank, s = src[gi];
    bool ok = dst < cells_cap;
    IncCell r;
    if (s & kIncScratch) {
        const uint32_t t = s & ~kIncScratch;
        ok = ok && t < nt;
        if (ok) r = scratch[(int64_t)t * kGroupCells + c];
    } else {
        ok = ok && s < n_old && old_off[s] + rank < n_old_cells;
        if (ok) r = old_cells[old_off[s] + rank];  // (an untouched group keeps its mask)
    }
    if (ok)
        cells[dst] = r;
    else
        atomicOr(&cc->status, O3DR_STATUS_INTERNAL);
}

// Snapshot: cells with at least `need` points (min_points_per_voxel, at least 1) -> centroids, in cell order = ascending
// linear voxel index.  k_inc_keep_count: kept cells per group (need > 1 only; otherwise out_off = the state's off).
// One wave per group, lane = cell.
__global__ __launch_bounds__(256) void k_inc_keep_count(const IncGroup* __restrict__ grp, const uint32_t* __restrict__ off,
                                                        const IncCell* __restrict__ cells, uint32_t n_groups, uint32_t n_cells,
                                                        uint32_t need, uint32_t* __restrict__ keep_cnt)
{
    const uint32_t gi = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (gi >= n_groups) return;
    const uint32_t m = grp[gi].mask;
    bool keep = false;
    if (lane < (uint32_t)kGroupCells && ((m >> lane) & 1u)) {
        const uint32_t ci = off[gi] + (uint32_t)__popc(m & ((1u << lane) - 1u));
        keep = ci < n_cells && cells[ci].n >= need;
    }
    const unsigned long long km = __ballot(keep);
    if (lane == 0) keep_cnt[gi] = (uint32_t)__popcll(km);
}
__global__ __launch_bounds__(256) void k_inc_snapshot(const IncGroup* __restrict__ grp, const uint32_t* __restrict__ off,
                                                      const IncCell* __restrict__ cells, uint32_t n_groups, uint32_t n_cells,
                                                      uint32_t need, const uint32_t* __restrict__ out_off, float z_offset,
                                                      uint4* __restrict__ out, uint32_t out_cap, CloudCounters* __restrict__ cc)
{
    const uint32_t gi = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (gi >= n_groups) return;
    const uint32_t m = grp[gi].mask;
    IncCell r;
    bool keep = false;
    if (lane < (uint32_t)kGroupCells && ((m >> lane) & 1u)) {
        const uint32_t ci = off[gi] + (uint32_t)__popc(m & ((1u << lane) - 1u));
        if (ci < n_cells) {
            r = cells[ci];
            keep = r.n >= need;
        } else {
            atomicOr(&cc->status, O3DR_STATUS_INTERNAL);
        }
    }
    const unsigned long long km = __ballot(keep);
    if (!keep) return;
    const uint32_t o = out_off[gi] + (uint32_t)__popcll(km & ((1ull << lane) - 1ull));
    if (o >= out_cap) {
        atomicOr(&cc->status, O3DR_STATUS_INTERNAL);
        return;
    }
    // k_centroid_groups' epilogue: true fp32 division, truncated colours, z - z_offset in fp32
    const float nf = (float)r.n;
    const float cx = r.s[0] / nf, cy = r.s[1] / nf, cz = r.s[2] / nf - z_offset;
    const uint32_t rgba = ((uint32_t)(r.s[6] / nf) << 24) | ((uint32_t)(r.s[3] / nf) << 16) | ((uint32_t)(r.s[4] / nf) << 8) |
                          (uint32_t)(r.s[5] / nf);
    out[o] = make_uint4(__float_as_uint(cx), __float_as_uint(cy), __float_as_uint(cz), rgba);
}

// the tail's group-run heads from the flags cloud_big recorded while it grew (head_flag_place: byte i / 4, bit i % 4),
// shifted to start at point `first`, which is forced to be a head; one thread per output byte
__global__ __launch_bounds__(256) void k_inc_heads_shift(const uint8_t* __restrict__ rec, uint64_t first, uint64_t n,
                                                         uint8_t* __restrict__ out, uint64_t out_bytes)
{
    const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (b >= out_bytes) return;
    uint32_t v = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint64_t r = 4 * b + (uint64_t)q;
        if (r >= n) break;
        const uint64_t i = first + r;
        const uint32_t f = r == 0 ? 1u : ((uint32_t)rec[i >> 2] >> (uint32_t)(i & 3u)) & 1u;
        v |= f << q;
    }
    out[b] = (uint8_t)v;
}

// the state's bounding box extended by the tail's (both 6 floats: min xyz, max xyz); the result also goes to `mm6`
__global__ void k_inc_box_fold(float* __restrict__ box6, const float* __restrict__ tail6, float* __restrict__ mm6)
{
    const int a = threadIdx.x;
    if (a >= 6) return;
    const float v = a < 3 ? fminf(box6[a], tail6[a]) : fmaxf(box6[a], tail6[a]);
    box6[a] = v;
    mm6[a] = v;
}
