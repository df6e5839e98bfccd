// Part of libo3dr's single device translation unit: included by o3dr_kernels.hip inside namespace o3dr
// (kernels and their launchers must share a translation unit without relocatable device code).

// =================================================================================================
// K2c — runs of equal index -> one output point each
//   third/fourth pass of VoxelGrid::applyFilter + CentroidPoint<PointXYZRGB>
//   [PCL 1.8 common/impl/accumulators.hpp: fp32 sums, xyz / n, uint32_t(channel / n)]
// =================================================================================================

// Run heads per segment tile: one wave per tile, a lane takes 16 consecutive records; no LDS, no workgroup barrier.  Leaves
// the head flags (bit q of byte b = record 4 b + q of the tile starts a run; a lane's 16 flags are one dword, a tile's 256
// bytes are consecutive) and their number per tile.  Two sources, picked per frame by the one kernel (k_run_heads):

// ... of a sorted (or, buf_sel 0/1, any) index sequence: four 16-byte loads per lane, all issued before anything is
// compared, and the index just before them.  buf_sel < 0: the frame's sorted buffer; 0/1: that buffer as is
constexpr int kHeadWaves = 4;  // segment tiles per workgroup of k_run_heads
__device__ __forceinline__ uint32_t run_heads_tile(const uint32_t* __restrict__ k, int f, int64_t cap, int64_t n, int tile, int lane)
{
    const int64_t i0 = (int64_t)tile * kSegTile + lane * 16;
    uint32_t kk[16];
    if (((((int64_t)f * cap) & 3) == 0) && i0 + 15 < n) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 v = *reinterpret_cast<const uint4*>(k + i0 + 4 * q);
            kk[4 * q] = v.x; kk[4 * q + 1] = v.y; kk[4 * q + 2] = v.z; kk[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) kk[q] = (i0 + q < n) ? k[i0 + q] : 0u;
    }
    uint32_t prev = (uint32_t)wave_shr1_i32((int32_t)kk[15]);
    if (lane == 0) prev = (i0 > 0 && i0 < n) ? k[i0 - 1] : 0u;  // the tile before this one ends with it
    uint32_t bits = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int64_t i = i0 + q;
        if (i < n && (i == 0 || kk[q] != (q ? kk[q - 1] : prev))) bits |= 1u << ((q >> 2) * 8 + (q & 3));
    }
    return bits;
}
// ... of a frame whose last scatter pass decided them itself (scatter_tile, ScatterJob::heads) and left one byte per
// record, 1 = starts a run, instead of the sorted indices: the bytes packed into the flag layout, from one read of the
// byte array.  Frames that did not sort (PCL's overflow guard, no passes) have no such bytes and take the indices.
__device__ __forceinline__ uint32_t side_heads_tile(const uint8_t* __restrict__ sb, int64_t n, int tile, int lane)
{
    const int64_t i0 = (int64_t)tile * kSegTile + lane * 16;
    uint32_t w4[4] = {0u, 0u, 0u, 0u};
    if (i0 + 15 < n) {  // (the frame stride and i0 are multiples of 16)
        const uint4 v = stream_load_u4(reinterpret_cast<const uint4*>(sb + i0));
        w4[0] = v.x; w4[1] = v.y; w4[2] = v.z; w4[3] = v.w;
    } else {
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (i0 + q < n) w4[q >> 2] |= (uint32_t)(sb[i0 + q] & 1u) << ((q & 3) * 8);
    }
    uint32_t bits = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // four flag bytes -> the low nibble of flag byte q
        const uint32_t w = w4[q];
        bits |= ((w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u)) << (8 * q);
    }
    return bits;
}
// side != nullptr: the frames that sorted (passes != 0) left side bytes and are packed from them; the others compare indices
__global__ __launch_bounds__(kHeadWaves * kWave) void k_run_heads(const uint32_t* __restrict__ keys0, const uint32_t* __restrict__ keys1,
                                                                  int64_t cap, const VoxelGeom* __restrict__ geom, int n_tiles,
                                                                  uint32_t* __restrict__ seg_cnt, int buf_sel,
                                                                  uint8_t* __restrict__ head_bits, const uint8_t* __restrict__ side,
                                                                  int64_t side_stride)
{
    static_assert(kSegTile == 16 * kWave, "16 records per lane");
    const int f = blockIdx.y, lane = threadIdx.x & 63;
    const int tile = blockIdx.x * kHeadWaves + (threadIdx.x >> 6);
    const VoxelGeom g = geom[f];
    if (g.overflow || tile >= n_tiles) return;
    const int64_t n = g.n;
    uint32_t c = 0;
    if ((int64_t)tile * kSegTile < n) {
        uint32_t bits;
        if (side && g.passes != 0u)
            bits = side_heads_tile(side + (int64_t)f * side_stride, n, tile, lane);
        else
            bits = run_heads_tile((buf_sel < 0 ? sorted_buf(g, keys0, keys1) : (buf_sel ? keys1 : keys0)) + (int64_t)f * cap, f, cap, n,
                                  tile, lane);
        reinterpret_cast<uint32_t*>(head_bits + ((int64_t)f * n_tiles + tile) * 256)[lane] = bits;
        c = (uint32_t)__popc(bits);
    }
    c = wave_sum_u32(c);
    if (lane == 0) seg_cnt[(int64_t)f * n_tiles + tile] = c;
}

// head_bits: the flags k_run_heads / k_voxel_keys_heads left (bit q of byte b = record 4 b + q starts a run; a tile's 256
// bytes are consecutive).  One wave per segment tile, a lane takes 16 consecutive records (one dword of flags): the run
// numbers inside the tile come from a wave scan, no workgroup barrier.  head_keys_out + in_pts (forming group runs from
// the points of a cloud): the run's sort key = group key of its first point.
constexpr int kStartWaves = 4;  // segment tiles per workgroup of k_run_starts
__global__ __launch_bounds__(kStartWaves * kWave) void k_run_starts(
    const uint32_t* __restrict__ keys0, const uint32_t* __restrict__ keys1, int64_t cap, const VoxelGeom* __restrict__ geom,
    int n_tiles, const uint32_t* __restrict__ seg_off, const uint32_t* __restrict__ n_vox, uint32_t* __restrict__ seg_start,
    int buf_sel, uint32_t* __restrict__ head_keys_out, const VoxelGeom* __restrict__ mode, const o3dr_point* __restrict__ in_pts,
    float z_offset, const uint8_t* __restrict__ head_bits)
{
    static_assert(kSegTile == 16 * kWave, "16 records per lane");
    const int f = blockIdx.y, lane = threadIdx.x & 63;
    const int tile = blockIdx.x * kStartWaves + (threadIdx.x >> 6);
    const VoxelGeom g = geom[f];
    if (g.overflow) return;
    if (mode && mode[f].grouped == 0u) return;  // this cloud sorts its points, not group runs (k_run_geom)
    const uint32_t n = g.n;
    const int64_t base = (int64_t)tile * kSegTile;
    if (tile >= n_tiles || base >= n) return;
    uint32_t* ss = seg_start + (int64_t)f * (cap + 1);
    if (tile == 0 && lane == 0) ss[n_vox[f]] = n;  // sentinel: end of the last run
    uint32_t bits = reinterpret_cast<const uint32_t*>(head_bits + ((int64_t)f * n_tiles + tile) * 256)[lane];
    // the four flag bytes carry 4 flags each in their low nibbles; records past the end have no flags
    bits &= 0x0f0f0f0fu;
    if (base + lane * 16 + 16 > (int64_t)n) {
#pragma unroll
        for (int q = 0; q < 16; ++q)
            if (base + lane * 16 + q >= (int64_t)n) bits &= ~(1u << ((q >> 2) * 8 + (q & 3)));
    }
    const uint32_t cnt = (uint32_t)__popc(bits);
    const uint32_t incl = wave_incl_scan_u32(cnt);
    const uint32_t tile_runs = __shfl(incl, 63, 64);
    // the tile's run starts go through LDS in run order, so that the global stores are consecutive
    __shared__ uint32_t stage_all[kStartWaves][kSegTile];
    uint32_t* stage = stage_all[threadIdx.x >> 6];
    uint32_t pos = incl - cnt;
    const uint32_t i0 = (uint32_t)base + (uint32_t)lane * 16u;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        if (bits & (1u << ((q >> 2) * 8 + (q & 3)))) stage[pos++] = i0 + (uint32_t)q;
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t off = seg_off[(int64_t)f * n_tiles + tile];
    for (uint32_t j = lane; j < tile_runs; j += kWave) {
        const uint32_t i = stage[j];
        ss[off + j] = i;
        if (head_keys_out) {
            uint32_t cell;
            const GroupCoord gc = group_coord_of(reinterpret_cast<const uint4*>(in_pts)[i], g.inv, z_offset, cell);
            head_keys_out[(int64_t)f * cap + off + j] = group_key_of(gc, g);
        }
    }
}

// min_points_per_voxel > 1 (combined merge, pose_functions.cpp:1693): runs with fewer points are dropped
__global__ __launch_bounds__(256) void k_keep_count(const uint32_t* __restrict__ seg_start, int64_t cap,
                                                    const VoxelGeom* __restrict__ geom,
                                                    const uint32_t* __restrict__ n_vox, uint32_t min_points,
                                                    int n_tiles, uint32_t* __restrict__ seg_cnt)
{
    __shared__ uint32_t lds[4];
    const int f = blockIdx.y, tile = blockIdx.x;
    if (geom[f].overflow || geom[f].grouped != 0u) return;  // (grouped clouds filter inside k_centroid_groups)
    const uint32_t nv = n_vox[f];
    const uint32_t* ss = seg_start + (int64_t)f * (cap + 1);
    uint32_t c = 0;
    const int64_t base = (int64_t)tile * kSegTile;
    if (base < nv) {
        for (int j = 0; j < kSegTile / 256; ++j) {
            const int64_t o = base + j * 256 + threadIdx.x;
            if (o < nv) c += (ss[o + 1] - ss[o] >= min_points) ? 1u : 0u;
        }
    }
    c = wave_sum_u32(c);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) seg_cnt[(int64_t)f * n_tiles + tile] = lds[0] + lds[1] + lds[2] + lds[3];
}
__global__ __launch_bounds__(256) void k_keep_write(const uint32_t* __restrict__ seg_start, int64_t cap,
                                                    const VoxelGeom* __restrict__ geom,
                                                    const uint32_t* __restrict__ n_vox, uint32_t min_points,
                                                    int n_tiles, const uint32_t* __restrict__ seg_off,
                                                    uint32_t* __restrict__ keep_idx)
{
    __shared__ uint32_t scan_lds[5];
    const int f = blockIdx.y, tile = blockIdx.x;
    if (geom[f].overflow || geom[f].grouped != 0u) return;
    const uint32_t nv = n_vox[f];
    const int64_t base = (int64_t)tile * kSegTile;
    if (base >= nv) return;
    const uint32_t* ss = seg_start + (int64_t)f * (cap + 1);
    uint32_t* ki = keep_idx + (int64_t)f * cap;
    uint32_t off = seg_off[(int64_t)f * n_tiles + tile];
    for (int j = 0; j < kSegTile / 256; ++j) {
        const int64_t o = base + j * 256 + threadIdx.x;
        const bool keep = (o < nv) && (ss[o + 1] - ss[o] >= min_points);
        uint32_t total;
        const uint32_t pos = block_excl_scan_u32<4>(keep ? 1u : 0u, scan_lds, total);
        if (keep) ki[off + pos] = (uint32_t)o;
        off += total;
    }
}

// per-frame output counts -> absolute offsets; advances the cloud counter (one 256-thread workgroup,
// frames in chunks of 256; a batch's total stays far below 2^32 points)
__global__ __launch_bounds__(256) void k_frame_offsets(const VoxelGeom* __restrict__ geom, const uint32_t* __restrict__ n_vox,
                                                       const uint32_t* __restrict__ n_keep,
                                                       const uint32_t* __restrict__ n_grp, int frames, int passthrough,
                                                       uint32_t* __restrict__ n_out, uint64_t* __restrict__ out_off,
                                                       CloudCounters* __restrict__ cc, SortStats* __restrict__ stats,
                                                       const VoxelGeom* __restrict__ sort_geom, int side_heads)
{
    __shared__ uint32_t scan_lds[5];
    __shared__ unsigned long long acc[6];  // record-passes, points in, points out, status, records flagged by the last pass, records
    if (threadIdx.x < 6) acc[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = cc->count;
    uint64_t carry = 0;
    for (int f0 = 0; f0 < frames; f0 += 256) {
        const int f = f0 + threadIdx.x;
        uint32_t m = 0;
        if (f < frames) {
            const VoxelGeom g = geom[f];
            if (passthrough) {
                m = g.n;
            } else if (g.overflow) {
                m = g.n;
                atomicOr(&acc[3], (unsigned long long)O3DR_STATUS_VOXEL_OVERFLOW);
            } else {
                m = (n_grp && sort_geom[f].grouped) ? n_grp[f] : (n_keep ? n_keep[f] : n_vox[f]);
                atomicAdd(&acc[0], (unsigned long long)sort_geom[f].n * g.passes);  // records actually sorted
                atomicAdd(&acc[5], (unsigned long long)sort_geom[f].n);
                // (a point sort's last pass leaves run-head flags instead of the sorted indices: scatter_tile, side_heads_tile)
                if (side_heads && g.passes != 0u) atomicAdd(&acc[4], (unsigned long long)sort_geom[f].n);
                atomicAdd(&acc[1], (unsigned long long)g.n);
                atomicAdd(&acc[2], (unsigned long long)m);
            }
        }
        uint32_t total;
        const uint32_t excl = block_excl_scan_u32<4>(m, scan_lds, total);
        if (f < frames) {
            n_out[f] = m;
            out_off[f] = base + carry + excl;
        }
        carry += total;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        cc->count = base + carry;
        cc->status |= (uint32_t)acc[3];
        if (stats) {
            stats->sort_record_passes += acc[0];
            stats->voxel_points_in += acc[1];
            stats->voxel_points_out += acc[2];
            stats->sort_records += acc[5];
            stats->side_head_records += acc[4];
        }
    }
}

// test hook (o3dr_test_corrupt_next_gather): what a bookkeeping error upstream of the gathers would leave behind - one
// sorted payload of frame 0 pointing far outside the cloud
__global__ void k_test_corrupt_payload(uint32_t* __restrict__ vals0, uint32_t* __restrict__ vals1, const VoxelGeom* __restrict__ geom)
{
    const VoxelGeom g = geom[0];
    if (g.overflow || g.n == 0u) return;
    uint32_t* v = ((g.passes + g.buf0) & 1u) ? vals1 : vals0;
    v[g.n / 2u] = 0xfffffff0u;
}

// outputs [256 bx, 256 bx + 256) of frame f
__device__ __forceinline__ void centroid_block(int64_t bx, int f, const VoxelGeom& g, uint32_t n_o,
                                               const o3dr_point* __restrict__ in, int64_t in_fstride,
                                               const uint32_t* __restrict__ vals0, const uint32_t* __restrict__ vals1,
                                               int64_t cap, const uint32_t* __restrict__ seg_start,
                                               const uint32_t* __restrict__ keep_idx, const uint64_t* __restrict__ out_off,
                                               float z_offset, int passthrough, o3dr_point* __restrict__ out_base,
                                               float* __restrict__ out_mm, int nbx, CloudCounters* __restrict__ cc,
                                               const CloudHeads& ch)
{
    const int64_t o = bx * kPtThreads + threadIdx.x;
    const bool active = o < (int64_t)n_o;
    if (__ballot(active) == 0ull) return;  // whole wave idle (k_cloud_bbox_fold skips its slot by the same test)
    uint4 res = make_uint4(0, 0, 0, 0);
    if (active) {
        const uint4* src = reinterpret_cast<const uint4*>(in + (int64_t)f * in_fstride);
        if (passthrough) {
            res = src[o];
        } else if (g.overflow) {  // output = input; the caller's z += 500 / z -= 500 still happen around it
            res = src[o];
            res.z = __float_as_uint((__uint_as_float(res.z) + z_offset) - z_offset);
        } else {
            const uint32_t* ss = seg_start + (int64_t)f * (cap + 1);
            const uint32_t* pid = sorted_buf(g, vals0, vals1) + (int64_t)f * cap;
            const uint32_t v = keep_idx ? keep_idx[(int64_t)f * cap + o] : (uint32_t)o;
            uint32_t b = ss[v], e = ss[v + 1];
            // Guard of the gather: a record range or point id outside the frame can only come from a bookkeeping
            // error upstream; skip the load and raise O3DR_STATUS_INTERNAL (the ABI then returns O3DR_ERR_INTERNAL)
            // instead of faulting the process (include/o3dr.h: "negative code, never an abort").
            bool bad = b > e || e > g.n;
            if (bad) b = e = 0;
            float sx = 0.f, sy = 0.f, sz = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sa = 0.f;
            // the sums are strictly sequential (input order); the loads are not: 8 gathers in flight
            for (uint32_t li = b; li < e; li += 8) {
                uint32_t id[8];
                uint4 p[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    id[k] = (li + k < e) ? pid[li + k] : 0xffffffffu;
                    if (id[k] != 0xffffffffu && id[k] >= g.n) {
                        bad = true;
                        id[k] = 0xffffffffu;
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (id[k] != 0xffffffffu) p[k] = src[id[k]];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (id[k] != 0xffffffffu) {
                        sx += __uint_as_float(p[k].x);
                        sy += __uint_as_float(p[k].y);
                        sz += __uint_as_float(p[k].z) + z_offset;
                        sr += (float)((p[k].w >> 16) & 255u);
                        sg += (float)((p[k].w >> 8) & 255u);
                        sb += (float)(p[k].w & 255u);
                        sa += (float)(p[k].w >> 24);
                    }
                }
            }
            const float nf = (float)(e - b);
            const float cx = sx / nf, cy = sy / nf, cz = sz / nf - z_offset;
            const uint32_t rgba = ((uint32_t)(sa / nf) << 24) | ((uint32_t)(sr / nf) << 16) | ((uint32_t)(sg / nf) << 8) |
                                  (uint32_t)(sb / nf);
            res = make_uint4(__float_as_uint(cx), __float_as_uint(cy), __float_as_uint(cz), rgba);
            if (bad) atomicOr(&cc->status, O3DR_STATUS_INTERNAL);
        }
        reinterpret_cast<uint4*>(out_base + out_off[f])[o] = res;
    }
    if (ch.flags) {
        // cloud_big records where its group runs start (for the merge's grid: ch.inv, ch.z_offset) while it grows: a point
        // starts one iff its voxel group differs from its predecessor's.  Lane 0 has no predecessor here: every wave
        // leaves the groups of its first and last point, and k_cloud_heads_fix compares neighbouring waves.
        uint32_t cell;
        GroupCoord gc = {0, 0, 0};
        if (active) gc = group_coord_of(res, ch.inv, ch.z_offset, cell);
        GroupCoord prev;
        prev.bx = wave_shr1_i32(gc.bx);
        prev.iy = wave_shr1_i32(gc.iy);
        prev.iz = wave_shr1_i32(gc.iz);
        const int lane = threadIdx.x & 63;
        // the wave's 64 flags cover (parts of) five flag words: one atomic OR per word, not per head (raw pixel-order
        // clouds - dont_downsample, frames under PCL's overflow guard - start a run at nearly every point)
        const unsigned long long hm = __ballot(active && lane != 0 && group_differs(gc, prev));
        if (hm != 0ull && lane < 5) {
            const uint64_t g0 = out_off[f] + (uint64_t)(o - lane);  // the wave's first record
            const uint64_t word = (g0 >> 4) + (uint64_t)lane;
            const int shift = (int)((int64_t)(word << 4) - (int64_t)g0);  // -15 .. 64
            uint32_t f16 = 0;
            if (shift < 64) f16 = (uint32_t)((shift >= 0 ? (hm >> shift) : (hm << -shift)) & 0xffffull);
            const uint32_t bits = (f16 & 0xfu) | ((f16 & 0xf0u) << 4) | ((f16 & 0xf00u) << 8) | ((f16 & 0xf000u) << 12);
            if (bits) atomicOr(&ch.flags[word], bits);
        }
        // the groups of the wave's first and last output: one 24-byte store (lanes 0..5) instead of six dword stores
        int32_t* slot = ch.wave_gc + (((int64_t)f * nbx + bx) * (kPtThreads / 64) + (threadIdx.x >> 6)) * 6;
        const int last = 63 - __builtin_clzll(__ballot(active));  // (the wave has outputs: checked at the top)
        const int32_t f0 = __builtin_amdgcn_readlane(gc.bx, 0), f1 = __builtin_amdgcn_readlane(gc.iy, 0),
                      f2 = __builtin_amdgcn_readlane(gc.iz, 0);
        const int32_t l0 = __builtin_amdgcn_readlane(gc.bx, last), l1 = __builtin_amdgcn_readlane(gc.iy, last),
                      l2 = __builtin_amdgcn_readlane(gc.iz, last);
        if (lane < 6) slot[lane] = lane == 0 ? f0 : (lane == 1 ? f1 : (lane == 2 ? f2 : (lane == 3 ? l0 : (lane == 4 ? l1 : l2))));
    }
    if (out_mm) {  // bounding box of what this wave appended (folded into cloud_big's box by k_cloud_bbox_fold)
        float* slot = out_mm + (((int64_t)f * nbx + bx) * (kPtThreads / 64) + (threadIdx.x >> 6)) * 6;
        const float c3[3] = {__uint_as_float(res.x), __uint_as_float(res.y), __uint_as_float(res.z)};
        float mine = 0.f;  // lane a < 6 stores component a of the box: one 24-byte store
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float l = wave_min_f32(active ? c3[a] : __builtin_inff());
            const float h = wave_max_f32(active ? c3[a] : -__builtin_inff());
            if ((threadIdx.x & 63) == a) mine = l;
            if ((threadIdx.x & 63) == 3 + a) mine = h;
        }
        if ((threadIdx.x & 63) < 6) slot[threadIdx.x & 63] = mine;
    }
}

// kStride: the grid is smaller than the outputs need and workgroups loop (used where the kernel is launched only in
// case a cloud took the other sort variant, so that a launch that finds nothing to do costs a few thousand workgroups)
template <bool kStride>
__global__ __launch_bounds__(kPtThreads) void k_centroid(const o3dr_point* __restrict__ in, int64_t in_fstride,
                                                         const uint32_t* __restrict__ vals0,
                                                         const uint32_t* __restrict__ vals1, int64_t cap,
                                                         const uint32_t* __restrict__ seg_start,
                                                         const uint32_t* __restrict__ keep_idx,
                                                         const VoxelGeom* __restrict__ geom,
                                                         const uint32_t* __restrict__ n_out,
                                                         const uint64_t* __restrict__ out_off, float z_offset,
                                                         int passthrough, o3dr_point* __restrict__ out_base,
                                                         float* __restrict__ out_mm, int nbx, CloudCounters* __restrict__ cc,
                                                         CloudHeads ch)
{
    const int f = blockIdx.y;
    const VoxelGeom g = geom[f];
    // g.n == 0: nothing to write; grouped: k_centroid_groups / k_group_compact write it
    if (!passthrough && (g.n == 0 || g.grouped != 0u)) return;
    const uint32_t n_o = n_out[f];
    if (kStride) {
        for (int64_t bx = blockIdx.x; bx * kPtThreads < (int64_t)n_o; bx += gridDim.x)
            centroid_block(bx, f, g, n_o, in, in_fstride, vals0, vals1, cap, seg_start, keep_idx, out_off, z_offset,
                           passthrough, out_base, out_mm, nbx, cc, ch);
    } else {
        // XCD-contiguous block order (gridDim.x is a multiple of 8): neighbouring blocks gather from neighbouring lines
        const int bx = xcd_chunk_item(blockIdx.x, (int)(((int64_t)n_o + kPtThreads - 1) / kPtThreads));
        if (bx < 0) return;
        centroid_block(bx, f, g, n_o, in, in_fstride, vals0, vals1, cap, seg_start, keep_idx, out_off, z_offset,
                       passthrough, out_base, out_mm, nbx, cc, ch);
    }
}

// the head flags k_centroid could not decide: the first point of every wave against the last point of the wave before it
// (from the groups the waves left in wave_gc; a frame's first point always starts a run)
__global__ __launch_bounds__(256) void k_cloud_heads_fix(const uint32_t* __restrict__ n_out, const uint64_t* __restrict__ out_off,
                                                         int waves_per_frame, CloudHeads ch)
{
    const int f = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= waves_per_frame || j * kWave >= (int64_t)n_out[f]) return;
    bool head = j == 0;
    if (!head) {
        const int32_t* cur = ch.wave_gc + ((int64_t)f * waves_per_frame + j) * 6;
        head = cur[0] != cur[-3] || cur[1] != cur[-2] || cur[2] != cur[-1];
    }
    if (head) {
        uint64_t word;
        uint32_t bit;
        head_flag_place(out_off[f] + (uint64_t)j * kWave, word, bit);
        atomicOr(&ch.flags[word], 1u << bit);
    }
}

// running bounding box of cloud_big: fold the slots k_centroid wrote for a batch (only workgroups that had output)
__global__ __launch_bounds__(256) void k_cloud_bbox_fold(const float* __restrict__ slots, int nbx, int frames,
                                                         const uint32_t* __restrict__ n_out, float* __restrict__ partial)
{
    __shared__ float mm_lds[6 * 4];
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    const int64_t total = (int64_t)nbx * frames;  // nbx = wave slots per frame
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int f = (int)(i / nbx), bx = (int)(i - (int64_t)f * nbx);
        if ((int64_t)bx * 64 < (int64_t)n_out[f]) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = fminf(lo[a], slots[i * 6 + a]);
                hi[a] = fmaxf(hi[a], slots[i * 6 + 3 + a]);
            }
        }
    }
    block_minmax_store<4>(lo, hi, true, mm_lds, partial + (int64_t)blockIdx.x * 6);
}
__global__ __launch_bounds__(384) void k_cloud_bbox_merge(const float* __restrict__ partial, int n_partial, float* __restrict__ box6)
{
    const int a = threadIdx.x >> 6, lane = threadIdx.x & 63;  // one wave per component (min x,y,z, max x,y,z)
    float v = a < 3 ? __builtin_inff() : -__builtin_inff();
    for (int i = lane; i < n_partial; i += 64) v = a < 3 ? fminf(v, partial[i * 6 + a]) : fmaxf(v, partial[i * 6 + a]);
    v = a < 3 ? wave_min_f32(v) : wave_max_f32(v);
    if (lane == 0) box6[a] = a < 3 ? fminf(box6[a], v) : fmaxf(box6[a], v);
}

// =================================================================================================
// Grouped voxel grid (whole-cloud calls: the combined merge, o3dr_voxel_grid).
// Inputs of those calls are mostly concatenations of clouds that are already in voxel order, so consecutive points
// very often fall into neighbouring voxels.  A GROUP is kGroupCells = 64 consecutive linear voxel indices; a maximal
// block of consecutive points of one group is a GROUP RUN (a piece of one row of one frame's cloud: ~35 points in the
// 200-frame merge).  Sorting the runs by group (stable) instead of the points by voxel leaves ~35x fewer records, and
// k_centroid_groups then reads every group's points as contiguous blocks, in input order, one wave per group with
// lane = voxel: PCL's strictly sequential per-voxel sums, fed by coalesced loads instead of per-lane gathers.
// Results are bit-identical to the per-point path.
// =================================================================================================
__global__ void k_run_geom(const VoxelGeom* __restrict__ geom, const uint32_t* __restrict__ n_runs, int frames,
                           VoxelGeom* __restrict__ geom_runs, int force, int64_t slots)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= frames) return;
    VoxelGeom g = geom[f];
    // Grouped or per point?  Decided here, on the device; `grouped` is what everything downstream keys off.
    //  - every group needs kGroupCells result slots: no more groups can exist than runs, or than the grid has;
    //  - it pays when the runs average 1.25 points or more (o3dr_device.h, kGroupMinRunNum: measured down to raw pixel-order
    //    points, 1.6 per run); a cloud of isolated points has as many runs as points and nothing to gain.
    const uint32_t nr = n_runs[f];
    const uint64_t group_keys = (uint64_t)group_blocks_x(g) * (uint64_t)(uint32_t)g.div_b[1] * (uint64_t)(uint32_t)g.div_b[2];
    uint64_t max_groups = group_keys;
    if ((uint64_t)nr < max_groups) max_groups = nr;
    const bool fits = max_groups * kGroupCells <= (uint64_t)slots;
    const bool pays = (uint64_t)nr * kGroupMinRunNum <= (uint64_t)g.n * kGroupMinRunDen;
    if (g.overflow) {  // output = input (k_group_compact copies it)
        g.grouped = 1;
        g.n = 0;
    } else if (fits && (pays || force)) {
        g.grouped = 1;
        g.n = nr;
        g.buf0 = 1;  // the run keys are gathered into buffer 1
        sort_plan(g, group_keys);
    }
    geom_runs[f] = g;
}

// One wave per non-empty group v (ascending group key = ascending voxel index), lane = voxel of the group.
// The group's runs are taken in sorted (= input) order, 64 at a time; their points form one stream, read in steps of
// kGroupStep = 256 points with coalesced loads (4 chunks of 64: lane i of chunk q = point 64 q + i of the step).  A step
// is a small stable counting sort in LDS: every point sets its lane's bit in its voxel's mask of its chunk, the voxel
// lanes turn their four masks into counts and positions (one wave scan), every point is written to its place in
// (voxel, stream) order, and every voxel lane then adds its points front to back - the same strictly sequential fp32
// sums as k_centroid, but from consecutive LDS addresses.  Voxels with fewer than min_points points are dropped here
// (pose_functions.cpp:1693).  Results: the group's kept voxels, compacted, in slots[64 v ..]; their number in
// grp_cnt[v].  (frames == 1.)
constexpr int kGroupChunks = 4;
constexpr int kGroupStep = kGroupChunks * kWave;
struct GroupLds {
    uint4 sorted[kGroupStep];                      // the step's points in (voxel, stream) order: x, y, z + z_offset, rgba
    unsigned long long mask[kWave][kGroupChunks];  // per voxel and chunk: the lanes whose point falls into the voxel
    uint32_t pre[kWave][kGroupChunks];             // per voxel and chunk: place of the first of those points in `sorted`
    unsigned long long bnd[kGroupChunks];          // stream positions of the step at which a run starts
};
__global__ __launch_bounds__(kGroupWaves * kWave) void k_centroid_groups(
    const o3dr_point* __restrict__ in, const uint32_t* __restrict__ keys0, const uint32_t* __restrict__ keys1,
    const uint32_t* __restrict__ ids0, const uint32_t* __restrict__ ids1, const uint32_t* __restrict__ seg_start,
    const uint32_t* __restrict__ run_start, const VoxelGeom* __restrict__ geom_runs, const VoxelGeom* __restrict__ geom_pts,
    const uint32_t* __restrict__ n_vox, float z_offset, uint32_t min_points, uint4* __restrict__ slots, int64_t n_slots,
    uint32_t* __restrict__ grp_cnt, CloudCounters* __restrict__ cc)
{
    __shared__ GroupLds lds[kGroupWaves];
    const VoxelGeom g = geom_runs[0];
    if (g.grouped == 0u || g.overflow) return;
    const VoxelGeom gp = geom_pts[0];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    GroupLds& L = lds[w];
#pragma unroll
    for (int q = 0; q < kGroupChunks; ++q) L.mask[lane][q] = 0ull;
    if (lane < kGroupChunks) L.bnd[lane] = 0ull;
    __builtin_amdgcn_wave_barrier();
    const uint32_t nv = n_vox[0], n_rec = g.n, n_points = gp.n;
    const uint32_t* sk = sorted_buf(g, keys0, keys1);
    const uint32_t* rv = sorted_buf(g, ids0, ids1);
    const uint4* src = reinterpret_cast<const uint4*>(in);
    const uint32_t need = min_points > 1u ? min_points : 1u;
    // single z layer (the combined merge) and x/y extents below 2^24: the group key needs no z and a 24-bit multiply
    const bool flat = gp.div_b[2] == 1 && (uint32_t)gp.div_b[0] < (1u << 24) && (uint32_t)gp.div_b[1] < (1u << 24);
    const int32_t bx0 = gp.min_b[0] >> kGroupBits;
    const uint32_t nbx = group_blocks_x(gp);
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    const unsigned long long starts_upto = (2ull << lane) - 2ull;  // positions 1 .. lane of a chunk
    bool bad = false;
    for (uint32_t v = blockIdx.x * kGroupWaves + w; v < nv; v += gridDim.x * kGroupWaves) {
        uint32_t jb = seg_start[v], je = seg_start[v + 1];
        // guards of the gathers (see centroid_block): record ranges inside the run list, runs inside the cloud, voxels
        // inside the group, result slots inside the buffer
        if (jb >= je || je > n_rec || ((int64_t)v + 1) * kGroupCells > n_slots) {
            bad = true;
            if (lane == 0 && ((int64_t)v + 1) * kGroupCells <= n_slots) grp_cnt[v] = 0;
            continue;
        }
        const uint32_t group_key = sk[jb];
        // CentroidPoint's seven sums, paired for packed adds: (x, y), z, (r, g), (b, a)
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        f32x2 s_xy = {0.f, 0.f}, s_rg = {0.f, 0.f}, s_ba = {0.f, 0.f};
        float sz = 0.f;
        uint32_t n_pts = 0;
        // Lane r of a window holds run j0 + r.  Its record (first point, end) is loaded one window ahead and its id two
        // windows ahead, with unconditional loads from clamped addresses, so that neither load is waited for where it
        // is issued.  (n_rec >= 1 here; the run table has n_rec + 1 entries.)
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
            const uint32_t pprev = incl - len;  // stream position of this run's first point
            const uint32_t delta = first - pprev;  // point index - stream position, for the points of this run
            const uint32_t total = __shfl(incl, 63, 64);
            // the points at stream positions k0 + 64 q + lane: a position's run = the runs ending at or before the
            // chunk's first position, plus the runs that start after it up to the position itself
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
                    p[q] = src[ok ? pidx : 0u];  // (unconditional: the load is not waited for here)
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
                step_load(k0 + kGroupStep, pn, okn);  // in flight while this step is summed (past the end: nothing is ok)
                // 1. every point marks itself in its voxel's mask of its chunk
                uint32_t cq[kGroupChunks];
#pragma unroll
                for (int q = 0; q < kGroupChunks; ++q) {
                    cq[q] = 0;
                    if (okm & (1u << q)) {
                        uint32_t c, gk;
                        if (flat) {
                            const int32_t i0 = (int32_t)floorf(__uint_as_float(p[q].x) * gp.inv[0]);
                            const int32_t i1 = (int32_t)floorf(__uint_as_float(p[q].y) * gp.inv[1]) - gp.min_b[1];
                            c = (uint32_t)(i0 & (kGroupCells - 1));
                            gk = (uint32_t)((i0 >> kGroupBits) - bx0) + __umul24(nbx, (uint32_t)i1);
                        } else {
                            gk = group_key_of(group_coord_of(p[q], gp.inv, z_offset, c), gp);
                        }
                        if (gk != group_key) c = 0xffffffffu;  // (not a point of this group: a bookkeeping error upstream)
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
                // 2. voxel lanes: counts per chunk -> places of the voxel's points in (voxel, stream) order
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
                // 3. every point goes to its place, as the addends of CentroidPoint's seven sums
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
                // 4. voxel lanes: strictly sequential sums, the LDS reads of four points in flight
                n_pts += cnt;
                const uint32_t trips = wave_max_u32(cnt);
                for (uint32_t t = 0; t < trips; t += 4) {
                    uint4 a4[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        // (lanes with nothing left all read the same slot: one broadcast instead of 64 bank accesses)
                        const uint4* at = (t + j < cnt) ? &L.sorted[(off + t) & (uint32_t)(kGroupStep - 1)] : &L.sorted[0];
                        a4[j] = at[j];
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
                __builtin_amdgcn_wave_barrier();  // the next step overwrites `sorted`
#pragma unroll
                for (int q = 0; q < kGroupChunks; ++q) p[q] = pn[q];
                okm = okn;
            }
        }
        const bool keep = n_pts >= need;
        const unsigned long long km = __ballot(keep);
        if (keep) {
            const float nf = (float)n_pts;
            const float cx = s_xy.x / nf, cy = s_xy.y / nf, cz = sz / nf - z_offset;
            const uint32_t rgba = ((uint32_t)(s_ba.y / nf) << 24) | ((uint32_t)(s_rg.x / nf) << 16) | ((uint32_t)(s_rg.y / nf) << 8) |
                                  (uint32_t)(s_ba.x / nf);
            const uint32_t rank = (uint32_t)__popcll(km & lanes_below);
            slots[(int64_t)v * kGroupCells + rank] = make_uint4(__float_as_uint(cx), __float_as_uint(cy), __float_as_uint(cz), rgba);
        }
        if (lane == 0) grp_cnt[v] = (uint32_t)__popcll(km);
    }
    if (bad) atomicOr(&cc->status, O3DR_STATUS_INTERNAL);
}

// the groups' results, compacted per group in slots[64 v ..], to their places in the output (grp_off = exclusive scan
// of grp_cnt); a cloud under PCL's overflow guard is copied instead (the caller's z += 500 / z -= 500 still happen)
__global__ __launch_bounds__(256) void k_group_compact(const o3dr_point* __restrict__ in, const VoxelGeom* __restrict__ geom_runs,
                                                       const VoxelGeom* __restrict__ geom_pts, const uint32_t* __restrict__ n_vox,
                                                       const uint32_t* __restrict__ grp_off, const uint4* __restrict__ slots,
                                                       const uint64_t* __restrict__ out_off, float z_offset,
                                                       o3dr_point* __restrict__ out_base)
{
    const VoxelGeom g = geom_runs[0];
    if (g.grouped == 0u) return;
    uint4* dst = reinterpret_cast<uint4*>(out_base + out_off[0]);
    const int64_t step = (int64_t)gridDim.x * 256;
    if (g.overflow) {
        const uint4* src = reinterpret_cast<const uint4*>(in);
        const int64_t n = geom_pts[0].n;
        for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < n; o += step) {
            uint4 v = src[o];
            v.z = __float_as_uint((__uint_as_float(v.z) + z_offset) - z_offset);
            dst[o] = v;
        }
        return;
    }
    const int64_t total = (int64_t)n_vox[0] * kGroupCells;
    for (int64_t sidx = (int64_t)blockIdx.x * 256 + threadIdx.x; sidx < total; sidx += step) {
        const int64_t v = sidx >> kGroupBits;
        const uint32_t c = (uint32_t)(sidx & (kGroupCells - 1));
        const uint32_t o0 = grp_off[v], cnt = grp_off[v + 1] - o0;
        if (c < cnt) dst[o0 + c] = slots[sidx];
    }
}
