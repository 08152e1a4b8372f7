// vpt_volume_thickness.hip — local thickness on the device (vpt_distance_thickness and its _timed / _capped forms): per voxel the largest
// squared radius D(c) among the open balls { |v - c|^2 < D(c) } of a distance handle that hold the voxel.  The result is another
// vpt_distance handle (vpt_volume_distance.h), so within, channel, info, squared and destroy are the distance unit's.
// C-ABI and the contract: include/vpt.h; why the culls are exact, compiler figures and measurements: DESIGN.md "Local thickness".
//
// A gather per output tile, not a scatter per centre.  The volume is cut into tiles of 8 x 8 x 4 voxels; a wave owns an output tile, a lane
// a column of four voxels along z.  The tiles that hold a centre are listed in descending order of their largest D (sorted on the host, as
// the component list is); a wave walks that list from the top, 64 entries a step, one entry a lane, and runs over the centres of the tiles
// that pass two exact culls (value, reach: k_th_cover).  Everything is integer; a maximum has no order, so neither the walk's order nor the
// culls can change a bit of the result.  No workgroup waits for another and no wave for another wave: launch boundaries order the phases.
#include "vpt_volume_distance.h"

#define TH_TX 8
#define TH_TY 8
#define TH_TZ 4
#define TH_COUNT_SLOTS 64          // words the waves add their visit counts into (k_edt_x's reason: not ten thousand adds to one word)
#define TH_NO_VALUE_CULL 1u
#define TH_NO_REACH_CULL 2u

__device__ __forceinline__ uint32_t wave_min(uint32_t m) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = min(m, (uint32_t)__shfl_xor((int)m, o));
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)m);
}

// the lane's column of a tile at (x0, y0, z0): four values along z, 0 for a voxel outside the volume
__device__ __forceinline__ void th_column(const uint32_t *__restrict__ d2, int nx, int ny, int nz, int x0, int y0, int z0, int lane, uint32_t col[TH_TZ]) {
    const int x = x0 + (lane & 7), y = y0 + (lane >> 3);
    const bool inside = x < nx && y < ny;
#pragma unroll
    for (int k = 0; k < TH_TZ; k++) {
        const int z = z0 + k;
        col[k] = (inside && z < nz) ? d2[((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)x] : 0u;
    }
}

// ---------------------------------------------------------------------------------------------
// the largest D of every tile, k_th_tile_max
// ---------------------------------------------------------------------------------------------
// A wave a tile; tiles are numbered x fastest.
__global__ __launch_bounds__(256) void k_th_tile_max(const uint32_t *__restrict__ d2, uint32_t *__restrict__ tile_max, int nx, int ny, int nz, int tnx, int tny, size_t tiles) {
    const int lane = (int)threadIdx.x & 63;
    for (size_t tile = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); tile < tiles; tile += (size_t)gridDim.x * 4) {
        const int tx = (int)(tile % (size_t)tnx), ty = (int)(tile / (size_t)tnx % (size_t)tny), tz = (int)(tile / ((size_t)tnx * (size_t)tny));
        uint32_t col[TH_TZ];
        th_column(d2, nx, ny, nz, tx * TH_TX, ty * TH_TY, tz * TH_TZ, lane, col);
        uint32_t m = max(max(col[0], col[1]), max(col[2], col[3]));
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
        if (lane == 0) tile_max[tile] = m;
    }
}

// ---------------------------------------------------------------------------------------------
// the cover, k_th_cover
// ---------------------------------------------------------------------------------------------
// list[e] = (the largest D of a tile, its tile coordinates tx | ty << 10 | tz << 20), descending in the first.  Workgroup b (one wave) owns
// the output tile list[b]: its voxels start at t = D, and `low` is the least t among its voxels with D > 0 (it has one: it is listed).
//   Value cull: an entry with maxD <= low cannot raise any voxel, and neither can any entry behind it: the walk ends there.  `low` is taken
//   again after every tile the wave has run over, so the stop is as tight as it can be at tile granularity.
//   Reach cull: a ball of tile A holds a voxel of B only if the squared gap between the two boxes is below its D, so below maxD(A).  The
//   boxes are the full tiles (a tile cut by the volume's border lies inside its full box: the cull only gets weaker there), so the gap
//   per axis is max(0, 8 |dtx| - 7) resp. max(0, 4 |dtz| - 3).
// A step of the walk: lane l takes entry base + l, decides both culls for it, and a ballot hands the wave the entries to run over, in list
// order.  Running over A: every lane loads its column of A (256 values in 4 registers a lane), then for each of A's 64 (x, y) positions
// the lanes compute their squared distance to it in the plane once and for each of its four centres fetch D_c from the lane that holds it
// (a wave-uniform lane index: v_readlane, D_c lands in a scalar register).  A centre with D_c = 0 or D_c <= low is skipped by a scalar
// branch; for the others each of the lane's four voxels costs a compare and a conditional max: dxy2 < D_c - dz^2, dz wave-uniform.
// All quantities are below 2^26 in magnitude: plain 32-bit integer arithmetic is exact.
__global__ __launch_bounds__(64) void k_th_cover(const uint32_t *__restrict__ d2, uint32_t *__restrict__ out, const uint2 *__restrict__ list, uint32_t listed,
                                                int nx, int ny, int nz, uint32_t flags, unsigned long long *__restrict__ visited) {
    const int lane = (int)threadIdx.x;
    const bool value_cull = !(flags & TH_NO_VALUE_CULL), reach_cull = !(flags & TH_NO_REACH_CULL);
    const uint32_t own = list[blockIdx.x].y;
    const int btx = (int)(own & 1023u), bty = (int)((own >> 10) & 1023u), btz = (int)(own >> 20);
    const int bx0 = btx * TH_TX, by0 = bty * TH_TY, bz0 = btz * TH_TZ;
    uint32_t t[TH_TZ];
    th_column(d2, nx, ny, nz, bx0, by0, bz0, lane, t);
    bool live[TH_TZ];
#pragma unroll
    for (int k = 0; k < TH_TZ; k++) live[k] = t[k] != 0u;
    uint32_t low = 0u;
    if (value_cull) low = wave_min(min(min(live[0] ? t[0] : EDT_NONE, live[1] ? t[1] : EDT_NONE), min(live[2] ? t[2] : EDT_NONE, live[3] ? t[3] : EDT_NONE)));
    unsigned long long ran = 0ull;                               // (wave-uniform)
    for (uint32_t base = 0u; base < listed; base += 64u) {
        const uint32_t e = base + (uint32_t)lane;
        const uint2 a = e < listed ? list[e] : make_uint2(0u, 0u);            // maxD = 0: beyond the list, fails the value test below
        const int gx = max(0, TH_TX * abs((int)(a.y & 1023u) - btx) - (TH_TX - 1));
        const int gy = max(0, TH_TY * abs((int)((a.y >> 10) & 1023u) - bty) - (TH_TY - 1));
        const int gz = max(0, TH_TZ * abs((int)(a.y >> 20) - btz) - (TH_TZ - 1));
        const uint32_t gap = (uint32_t)(gx * gx + gy * gy + gz * gz);
        unsigned long long todo = __ballot(a.x > low && (!reach_cull || gap < a.x));
        while (todo) {
            const int j = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const uint32_t a_max = (uint32_t)__builtin_amdgcn_readlane((int)a.x, j), a_at = (uint32_t)__builtin_amdgcn_readlane((int)a.y, j);
            if (a_max <= low) break;                            // `low` has risen since the ballot: this entry and all behind it are out
            const int ax0 = (int)(a_at & 1023u) * TH_TX, ay0 = (int)((a_at >> 10) & 1023u) * TH_TY, az0 = (int)(a_at >> 20) * TH_TZ;
            uint32_t c[TH_TZ];
            th_column(d2, nx, ny, nz, ax0, ay0, az0, lane, c);
            const int rx = bx0 - ax0 + (lane & 7), ry = by0 - ay0 + (lane >> 3), rz = bz0 - az0;
#pragma unroll 1
            for (int i = 0; i < 64; i++) {
                const int dx = rx - (i & 7), dy = ry - (i >> 3);
                const int dxy2 = dx * dx + dy * dy;
#pragma unroll
                for (int k = 0; k < TH_TZ; k++) {
                    const uint32_t dc = (uint32_t)__builtin_amdgcn_readlane((int)c[k], i);
                    if (dc <= low) continue;                    // 0: not a centre; otherwise too small to raise anything here
#pragma unroll
                    for (int kk = 0; kk < TH_TZ; kk++) {
                        const int dz = rz + kk - k;
                        if (dxy2 < (int)dc - dz * dz) t[kk] = max(t[kk], dc);
                    }
                }
            }
            ran++;
            if (value_cull) low = wave_min(min(min(live[0] ? t[0] : EDT_NONE, live[1] ? t[1] : EDT_NONE), min(live[2] ? t[2] : EDT_NONE, live[3] ? t[3] : EDT_NONE)));
        }
        // the step's last entry is its smallest (0 beyond the list)
        if (value_cull && (uint32_t)__builtin_amdgcn_readlane((int)a.x, 63) <= low) break;
    }
    const int x = bx0 + (lane & 7), y = by0 + (lane >> 3);
    if (x < nx && y < ny) {
#pragma unroll
        for (int k = 0; k < TH_TZ; k++) {
            const int z = bz0 + k;
            if (z < nz) out[((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)x] = live[k] ? t[k] : 0u;
        }
    }
    if (lane == 0 && ran) atomicAdd(&visited[blockIdx.x % TH_COUNT_SLOTS], ran);
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// the body of the three entry points behind the argument checks; `d` is freed by the caller on failure.  ms, tiles, visited may be null.
static int thickness_build(vpt_distance *src, vpt_distance *d, uint32_t flags, double *ms, uint64_t *tiles, uint64_t *visited) {
    vpt_context *ctx = src->ctx;
    hipStream_t st = ctx->stream;
    d->ctx = ctx; d->nx = src->nx; d->ny = src->ny; d->nz = src->nz; d->format = src->format; d->filter = src->filter; d->norm16 = src->norm16;
    const size_t n = d->voxels(), texel_bytes = n * (size_t)(src->norm16 ? 2 : 1);
    HIP_TRY(d->texels.alloc(texel_bytes));
    HIP_TRY(d->values.alloc(n));
    HIP_TRY(hipMemcpyAsync(d->texels, src->texels, texel_bytes, hipMemcpyDeviceToDevice, st));
    d->info.seeds = src->info.seeds;
    if (src->info.seeds == 0) {                                 // D is NONE everywhere, and so is T2
        HIP_TRY(hipMemsetAsync(d->values, 0xFF, n * sizeof(uint32_t), st));
        HIP_TRY(hipStreamSynchronize(st));
        d->info.largest = 0u;
        return VPT_OK;
    }
    const int tnx = (d->nx + TH_TX - 1) / TH_TX, tny = (d->ny + TH_TY - 1) / TH_TY, tnz = (d->nz + TH_TZ - 1) / TH_TZ;      // <= 512, 512, 1024
    const size_t all = (size_t)tnx * (size_t)tny * (size_t)tnz;                                                              // <= 2^28
    DevBuf<uint32_t> tile_max, largest;                         // freed when the call returns: every path below drains the stream first
    DevBuf<uint2> list;
    DevBuf<unsigned long long> count;
    HIP_TRY(tile_max.alloc(all));
    HIP_TRY(largest.alloc(1));
    HIP_TRY(count.alloc(TH_COUNT_SLOTS));
    HIP_TRY(hipMemsetAsync(largest, 0, sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(count, 0, TH_COUNT_SLOTS * sizeof(unsigned long long), st));
    HIP_TRY(hipStreamSynchronize(st));                          // what is in front of the call is not its time
    double none[VPT_THICKNESS_PHASES] = {};
    if (!ms) ms = none;
    PhaseClock clock(st);
    // ---- tile maxima and their ordering; the voxels outside every listed tile have D = 0 = T2: the result starts as a copy of D
    const uint32_t *d2 = src->values.get();
    hipLaunchKernelGGL(k_th_tile_max, dim3(stream_grid(all, 4)), dim3(256), 0, st, d2, tile_max.get(), d->nx, d->ny, d->nz, tnx, tny, all);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(d->values, src->values, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
    std::vector<uint32_t> host_max(all);
    HIP_TRY(hipMemcpyAsync(host_max.data(), tile_max, all * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint64_t> keys;                                 // maxD descending, then the tile number ascending: one order whatever the sort does
    for (size_t tile = 0; tile < all; tile++)
        if (host_max[tile]) keys.push_back(((uint64_t)host_max[tile] << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)tile));
    std::sort(keys.begin(), keys.end(), [](uint64_t a, uint64_t b) { return a > b; });
    const size_t listed = keys.size();
    std::vector<uint2> host_list(listed);
    for (size_t e = 0; e < listed; e++) {
        const uint32_t tile = 0xFFFFFFFFu - (uint32_t)keys[e];
        const uint32_t tx = tile % (uint32_t)tnx, ty = tile / (uint32_t)tnx % (uint32_t)tny, tz = tile / ((uint32_t)tnx * (uint32_t)tny);
        host_list[e] = make_uint2((uint32_t)(keys[e] >> 32), tx | (ty << 10) | (tz << 20));
    }
    if (listed) {
        HIP_TRY(list.alloc(listed));
        HIP_TRY(hipMemcpyAsync(list, host_list.data(), listed * sizeof(uint2), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(clock.lap(&ms[0]));                                 // (host_list is no longer read)
    // ---- cover
    if (listed) {
        hipLaunchKernelGGL(k_th_cover, dim3((unsigned)listed), dim3(64), 0, st, d2, d->values.get(), (const uint2 *)list.get(), (uint32_t)listed, d->nx, d->ny, d->nz, flags,
                           count.get());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(clock.lap(&ms[1]));
    // ---- info
    unsigned long long host_count[TH_COUNT_SLOTS] = {}; uint32_t host_largest = 0;
    VPT_TRY(distance_largest(st, d->values.get(), n, largest.get()));
    HIP_TRY(hipMemcpyAsync(host_count, count, sizeof(host_count), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&host_largest, largest, sizeof(host_largest), hipMemcpyDeviceToHost, st));
    HIP_TRY(clock.lap(&ms[2]));
    d->info.largest = host_largest;
    if (tiles) *tiles = (uint64_t)listed;
    if (visited) { *visited = 0; for (int k = 0; k < TH_COUNT_SLOTS; k++) *visited += host_count[k]; }
    return VPT_OK;
}

static int thickness_create(vpt_distance *src, uint32_t flags, vpt_distance **out, double *ms, uint64_t *tiles, uint64_t *visited) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (ms) for (int i = 0; i < VPT_THICKNESS_PHASES; i++) ms[i] = 0.0;
    if (tiles) *tiles = 0;
    if (visited) *visited = 0;
    vpt_context *ctx = src->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<vpt_distance> d(new vpt_distance());
    const int rc = thickness_build(src, d.get(), flags, ms, tiles, visited);
    if (rc != VPT_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }      // the buffers are freed on return: nothing may still use them
    *out = d.release();
    return VPT_OK;
}

extern "C" int vpt_distance_thickness(vpt_distance *src, vpt_distance **out) { return thickness_create(src, 0u, out, nullptr, nullptr, nullptr); }

extern "C" int vpt_distance_thickness_timed(vpt_distance *src, vpt_distance **out, double *ms, uint64_t *tiles, uint64_t *visited) {
    if (!ms || !tiles || !visited) return fail(VPT_ERR_INVALID, "null argument");
    return thickness_create(src, 0u, out, ms, tiles, visited);
}

extern "C" int vpt_distance_thickness_capped(vpt_distance *src, int flags, vpt_distance **out, double *ms, uint64_t *visited) {
    if (flags & ~(int)(TH_NO_VALUE_CULL | TH_NO_REACH_CULL)) return fail(VPT_ERR_INVALID, "thickness flags %d: bit 0 (no value cull) and bit 1 (no reach cull) are taken", flags);
    return thickness_create(src, (uint32_t)flags, out, ms, nullptr, visited);
}
