// vpt_volume_reconstruct.hip — grey-level morphological reconstruction of a marker under a mask on the device (vpt_volume_reconstruct) and
// the geodesic operations that are one reconstruction each (vpt_volume_geodesic: fill holes, clear border, h-maxima, h-minima, dome,
// regional maxima and minima).  C-ABI and the contract: include/vpt.h; kernel forms, why the races are benign, compiler figures and
// measurements: DESIGN.md "Geodesic reconstruction".
//
// Three kernels: a streaming seed (r0 into the result's texels, the marker made in registers), the tile kernel (a 64 x 8 x 4 tile relaxed to
// convergence in LDS, launched again over the tiles whose surroundings rose) and a streaming epilogue.  Everything is unsigned integer
// min / max; no workgroup waits for another: launch boundaries order the phases, a texel is written by its tile's owner only, and the only
// atomic on global memory is the integer count of the tiles that worked.
//
// One domain: reconstruction by erosion is reconstruction by dilation of the complements, and the complement of a code c is c ^ M
// (M = 255 / 65535 has every bit set), so the kernels reconstruct by dilation on `code ^ flip`, flip = 0 or M, applied where a texel is
// loaded and where it is stored.  A neighbour outside the volume does not exist: it reads as 0, which max() ignores.
#include "vpt_internal.h"

#define RC_TX 64
#define RC_TY 8
#define RC_TZ 4
#define RC_VOX (RC_TX * RC_TY * RC_TZ)
#define RC_PX (RC_TX + 2)
#define RC_PY (RC_TY + 2)
#define RC_PZ (RC_TZ + 2)
#define RC_PAD (RC_PX * RC_PY * RC_PZ)
static_assert(RC_VOX == 2048, "eight voxels a thread");
// In-tile rounds: with the rim fixed, k rounds give every voxel the best path of at most k edges, and a simple path through the tile and
// its rim has at most RC_VOX edges; one more round sees that nothing changes.
#define RC_TILE_ROUNDS (RC_VOX + 1)

// words of the control block on the device (16 bytes, zeroed in front of every launch)
enum { RW_CHANGED = 0, RW_ACTIVE = 1, RW_WORDS = 4 };
// how the seed kernel makes the marker, in the flipped domain (K = mask ^ flip)
enum { SEED_MARKER = 0,     // min(marker ^ flip, K)
       SEED_BORDER = 1,     // K on the volume's six faces, 0 elsewhere
       SEED_SHIFT = 2 };    // max(K - h, 0)
// what the epilogue leaves, S the source code and R the reconstruction
enum { FIN_NONE = 0, FIN_SUB = 1 /* S - R */, FIN_ABOVE = 2 /* M where S > R */, FIN_BELOW = 3 /* M where S < R */ };

__device__ __forceinline__ void st_agent(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// is the offset (dx, dy, dz) != 0 a neighbour under CONN?
template <int CONN> __host__ __device__ constexpr bool is_neighbour(int dx, int dy, int dz) {
    const int m = (dx != 0) + (dy != 0) + (dz != 0);
    return m >= 1 && m <= (CONN == 6 ? 1 : CONN == 18 ? 2 : 3);
}
// Tile directions as bits: bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) is the neighbouring tile at (dx, dy, dz).  axis_dirs(a, v): the
// directions whose component along axis a is v; conn_dirs<CONN>(): those that are neighbour offsets under CONN.
__host__ __device__ constexpr uint32_t axis_dirs(int axis, int v) {
    uint32_t m = 0u;
    for (int b = 0; b < 27; b++) {
        const int d[3] = { b % 3 - 1, (b / 3) % 3 - 1, b / 9 - 1 };
        if (d[axis] == v) m |= 1u << b;
    }
    return m;
}
template <int CONN> __host__ __device__ constexpr uint32_t conn_dirs() {
    uint32_t m = 0u;
    for (int b = 0; b < 27; b++)
        if (is_neighbour<CONN>(b % 3 - 1, (b / 3) % 3 - 1, b / 9 - 1)) m |= 1u << b;
    return m;
}
// the tiles that hold a CONN-neighbour of the tile voxel (tx, ty, tz): a component may leave the tile only where the voxel lies on that face
template <int CONN> __device__ __forceinline__ uint32_t touched_tiles(int tx, int ty, int tz) {
    constexpr uint32_t X0 = axis_dirs(0, 0), XM = axis_dirs(0, -1), XP = axis_dirs(0, 1);
    constexpr uint32_t Y0 = axis_dirs(1, 0), YM = axis_dirs(1, -1), YP = axis_dirs(1, 1);
    constexpr uint32_t Z0 = axis_dirs(2, 0), ZM = axis_dirs(2, -1), ZP = axis_dirs(2, 1);
    constexpr uint32_t C = conn_dirs<CONN>();
    const uint32_t x = X0 | (tx == 0 ? XM : 0u) | (tx == RC_TX - 1 ? XP : 0u);
    const uint32_t y = Y0 | (ty == 0 ? YM : 0u) | (ty == RC_TY - 1 ? YP : 0u);
    const uint32_t z = Z0 | (tz == 0 ? ZM : 0u) | (tz == RC_TZ - 1 ? ZP : 0u);
    return x & y & z & C;
}

// ---------------------------------------------------------------------------------------------
// seed: k_recon_seed<T>
// ---------------------------------------------------------------------------------------------
// r0 = min(marker, mask) in the flipped domain, one voxel a lane and step; the marker is made in registers (SEED_*) and never stored.  A
// source of two channels is read through its stride: element i * stride + channel.  Bounds: i < n, so the loads end at element
// (n - 1) * stride + channel of a source of n * stride elements (channel < stride), the store at texel n - 1 of the result.
template <typename T>
__global__ __launch_bounds__(256) void k_recon_seed(const T *__restrict__ marker, uint32_t marker_stride, uint32_t marker_channel, const T *__restrict__ mask,
                                                   uint32_t mask_stride, uint32_t mask_channel, T *__restrict__ r, int nx, int ny, int nz, size_t n, int seed,
                                                   uint32_t h, uint32_t flip) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t K = (uint32_t)mask[i * mask_stride + mask_channel] ^ flip;
        uint32_t v;
        if (seed == SEED_MARKER) {
            v = min((uint32_t)marker[i * marker_stride + marker_channel] ^ flip, K);
        } else if (seed == SEED_SHIFT) {
            v = K > h ? K - h : 0u;
        } else {
            const int x = (int)(i % (size_t)nx); const size_t row = i / (size_t)nx; const int y = (int)(row % (size_t)ny), z = (int)(row / (size_t)ny);
            const bool face = x == 0 || x == nx - 1 || y == 0 || y == ny - 1 || z == 0 || z == nz - 1;
            v = face ? K : 0u;
        }
        r[i] = (T)(v ^ flip);
    }
}

// ---------------------------------------------------------------------------------------------
// tiles: k_recon_tiles<T, CONN>
// ---------------------------------------------------------------------------------------------
// A workgroup of 256 threads owns a RC_TX x RC_TY x RC_TZ tile, eight voxels a thread.  r and the mask are staged in LDS with a one-voxel
// rim: the rim of r holds the neighbouring tiles' texels as global memory has them now, 0 outside the volume, so the loop has no bounds
// tests; the rim of the mask is 0 and never read.  A round gives every tile voxel min(mask, max of itself and its CONN neighbours), in
// place: a neighbour read while its owner writes is the old or the new value, both of them values the iteration passes through, and a
// round in which no thread wrote has read settled values only, so it proves the fixed point for this rim.  The loop ends there, or after
// `rounds` rounds; a tile that was cut short flags itself for the next launch.
// What rose is stored (each texel by its owner only, a T-wide store).  A voxel of the tile's outer layer that rose sets the next launch's
// dirty flag of every existing tile that holds one of its CONN neighbours; whoever sets a flag raises words[RW_CHANGED].  A tile whose own
// flag is clear leaves after reading it.  Bounds: a tile voxel is read and written only where x < nx, y < ny, z < nz; a rim voxel is read
// only inside the volume; flags are written at tile indices inside the grid, which has one flag a tile.
template <typename T, int CONN>
__global__ __launch_bounds__(256) void k_recon_tiles(T *r, const T *__restrict__ mask, uint32_t mask_stride, uint32_t mask_channel, int nx, int ny, int nz,
                                                    uint32_t flip, int rounds, const uint32_t *__restrict__ dirty_now, uint32_t *__restrict__ dirty_next,
                                                    uint32_t *__restrict__ words) {
    __shared__ T s_r[RC_PAD], s_m[RC_PAD];
    __shared__ uint32_t s_dirs;
    const int tid = (int)threadIdx.x;
    const size_t tile = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (dirty_now && dirty_now[tile] == 0u) return;                 // (uniform) nothing around this tile rose in the last launch
    const int x0 = (int)blockIdx.x * RC_TX, y0 = (int)blockIdx.y * RC_TY, z0 = (int)blockIdx.z * RC_TZ;
    if (tid == 0) s_dirs = 0u;
    for (int i = tid; i < RC_PAD; i += 256) {
        const int px = i % RC_PX, py = (i / RC_PX) % RC_PY, pz = i / (RC_PX * RC_PY);
        const int x = x0 + px - 1, y = y0 + py - 1, z = z0 + pz - 1;
        uint32_t rv = 0u, mv = 0u;
        if (x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz) {
            const size_t g = ((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)x;
            rv = (uint32_t)r[g] ^ flip;
            if (px >= 1 && px <= RC_TX && py >= 1 && py <= RC_TY && pz >= 1 && pz <= RC_TZ) mv = (uint32_t)mask[g * mask_stride + mask_channel] ^ flip;
        }
        s_r[i] = (T)rv; s_m[i] = (T)mv;
    }
    __syncthreads();
    int at[8];                  // LDS index of this thread's voxel k, -1: outside the volume
    uint32_t first[8];          // what the voxel held when the launch began
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int j = tid + 256 * k, tx = j % RC_TX, ty = (j / RC_TX) % RC_TY, tz = j / (RC_TX * RC_TY);
        at[k] = -1; first[k] = 0u;
        if (x0 + tx < nx && y0 + ty < ny && z0 + tz < nz) {
            at[k] = ((tz + 1) * RC_PY + (ty + 1)) * RC_PX + (tx + 1);
            first[k] = s_r[at[k]];
        }
    }
    bool settled = false;
    for (int round = 0; round < rounds; round++) {
        bool changed = false;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int p = at[k];
            if (p < 0) continue;
            const uint32_t own = s_r[p], cap = s_m[p];
            if (own >= cap) continue;                              // at its mask: it cannot rise
            uint32_t m = own;
#pragma unroll
            for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++)
                        if (is_neighbour<CONN>(dx, dy, dz)) m = max(m, (uint32_t)s_r[p + (dz * RC_PY + dy) * RC_PX + dx]);
            m = min(m, cap);
            if (m > own) { s_r[p] = (T)m; changed = true; }
        }
        if (!__syncthreads_or(changed ? 1 : 0)) { settled = true; break; }       // (uniform: the barrier's result)
    }
    // ---- what rose goes back; which neighbouring tiles must look again
    uint32_t dirs = 0u;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int p = at[k];
        if (p < 0) continue;
        const uint32_t v = s_r[p];
        if (v == first[k]) continue;
        const int j = tid + 256 * k, tx = j % RC_TX, ty = (j / RC_TX) % RC_TY, tz = j / (RC_TX * RC_TY);
        r[((size_t)(z0 + tz) * (size_t)ny + (size_t)(y0 + ty)) * (size_t)nx + (size_t)(x0 + tx)] = (T)(v ^ flip);
        dirs |= touched_tiles<CONN>(tx, ty, tz);
    }
    if (dirs) atomicOr(&s_dirs, dirs);
    __syncthreads();
    bool flagged = false;
    if (tid < 27 && ((s_dirs >> tid) & 1u)) {
        const int bx = (int)blockIdx.x + tid % 3 - 1, by = (int)blockIdx.y + (tid / 3) % 3 - 1, bz = (int)blockIdx.z + tid / 9 - 1;
        if (bx >= 0 && bx < (int)gridDim.x && by >= 0 && by < (int)gridDim.y && bz >= 0 && bz < (int)gridDim.z) {
            dirty_next[((size_t)bz * gridDim.y + (size_t)by) * gridDim.x + (size_t)bx] = 1u;
            flagged = true;
        }
    }
    if (tid == 0 && !settled) { dirty_next[tile] = 1u; flagged = true; }       // cut short: this tile goes on in the next launch
    if (flagged) st_agent(&words[RW_CHANGED], 1u);
    if (tid == 0) atomicAdd(&words[RW_ACTIVE], 1u);                            // (measurements) tiles that did LDS work
}

// ---------------------------------------------------------------------------------------------
// epilogue: k_recon_finish<T>
// ---------------------------------------------------------------------------------------------
// In place over the result's texels: the subtraction of CLEAR_BORDER and DOME (R <= S there: reconstruction by dilation stays under its
// mask), the threshold of MAXIMA and MINIMA.  Bounds as k_recon_seed.
template <typename T>
__global__ __launch_bounds__(256) void k_recon_finish(const T *__restrict__ src, uint32_t src_stride, uint32_t src_channel, T *__restrict__ r, size_t n, int fin,
                                                     uint32_t M) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t S = (uint32_t)src[i * src_stride + src_channel], R = (uint32_t)r[i];
        r[i] = (T)(fin == FIN_SUB ? S - R : fin == FIN_ABOVE ? (S > R ? M : 0u) : (S < R ? M : 0u));
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static const char *const GEODESIC_OP_NAMES[] = { "FILL_HOLES", "CLEAR_BORDER", "HMAX", "HMIN", "DOME", "MAXIMA", "MINIMA" };

struct ReconPlan { int seed; uint32_t h; uint32_t flip; int fin; };
struct ReconProfile { double *ms; uint32_t *launches; uint64_t *tile_runs; };

// what every entry point asks of a source; `what`: "reconstruct" or "geodesic", `which`: "marker", "mask" or "src"
static int check_source(const char *what, const char *which, const vpt_volume *v, int channel) {
    if (v->format != VPT_FORMAT_R8 && v->format != VPT_FORMAT_RG8 && v->format != VPT_FORMAT_R16 && v->format != VPT_FORMAT_RG16)
        return fail(VPT_ERR_UNSUPPORTED, "%s: %s is an unsigned normalised volume (R8, RG8, R16, RG16; the window makes R8 / R16 of any scalar volume), not %s",
                    what, which, format_name(v->format));
    if (channel != 0 && channel != 1) return fail(VPT_ERR_INVALID, "%s: channel %d of %s: 0 or 1 are taken", what, channel, which);
    if (channel == 1 && v->channels != 2) return fail(VPT_ERR_INVALID, "%s: channel 1 of %s, which has one channel (%s)", what, which, format_name(v->format));
    return VPT_OK;
}
static int check_connectivity(int connectivity) {
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return fail(VPT_ERR_INVALID, "connectivity %d: 6, 18 or 26 are taken", connectivity);
    return VPT_OK;
}

template <typename T>
static void launch_tiles(int conn, dim3 grid, hipStream_t st, T *r, const T *mask, uint32_t ks, uint32_t kc, const vpt_volume *v, uint32_t flip, int rounds,
                         const uint32_t *now, uint32_t *next, uint32_t *words) {
    if (conn == 6) hipLaunchKernelGGL((k_recon_tiles<T, 6>), grid, dim3(256), 0, st, r, mask, ks, kc, v->nx, v->ny, v->nz, flip, rounds, now, next, words);
    else if (conn == 18) hipLaunchKernelGGL((k_recon_tiles<T, 18>), grid, dim3(256), 0, st, r, mask, ks, kc, v->nx, v->ny, v->nz, flip, rounds, now, next, words);
    else hipLaunchKernelGGL((k_recon_tiles<T, 26>), grid, dim3(256), 0, st, r, mask, ks, kc, v->nx, v->ny, v->nz, flip, rounds, now, next, words);
}

// seed, the launches of the tile kernel, epilogue: everything between the argument checks and volume_finish_derived.  `d` is the result,
// freed by the caller on failure.
template <typename T>
static int reconstruct_run(const vpt_volume *marker, int marker_channel, const vpt_volume *mask, int mask_channel, const ReconPlan &plan, int conn, int rounds,
                           vpt_volume *d, const ReconProfile &prof) {
    vpt_context *c = mask->ctx;
    hipStream_t st = c->stream;
    const size_t n = (size_t)mask->nx * (size_t)mask->ny * (size_t)mask->nz;
    const dim3 grid((unsigned)((mask->nx + RC_TX - 1) / RC_TX), (unsigned)((mask->ny + RC_TY - 1) / RC_TY), (unsigned)((mask->nz + RC_TZ - 1) / RC_TZ));
    const size_t tiles = (size_t)grid.x * grid.y * grid.z;
    DevBuf<uint32_t> words, flags;                                // freed when the call returns: every path below drains the stream first
    HIP_TRY(words.alloc(RW_WORDS));
    HIP_TRY(flags.alloc(2 * tiles));
    T *r = (T *)d->linear.get();
    const T *m = (const T *)marker->linear.get(), *k = (const T *)mask->linear.get();
    const uint32_t ms = (uint32_t)marker->channels, ks = (uint32_t)mask->channels;
    hipLaunchKernelGGL(k_recon_seed<T>, dim3(stream_grid(n)), dim3(256), 0, st, m, ms, (uint32_t)marker_channel, k, ks, (uint32_t)mask_channel, r, mask->nx, mask->ny,
                       mask->nz, n, plan.seed, plan.h, plan.flip);
    HIP_TRY(hipGetLastError());
    // The first launch takes every tile, a later one the tiles flagged by the one before it.  Every launch that sets a flag has raised a
    // texel (a flag is set by a tile in which a voxel rose, or which was cut short in a round that wrote), texels only rise and stay under
    // the mask, so the sum of r strictly rises from launch to launch and is bounded by the sum of the mask: the loop ends.
    uint32_t host_words[RW_WORDS] = {};
    for (uint32_t launch = 0; ; launch++) {
        const uint32_t *now = launch == 0 ? nullptr : flags.get() + (size_t)(launch & 1u) * tiles;
        uint32_t *next = flags.get() + (size_t)((launch + 1u) & 1u) * tiles;
        HIP_TRY(hipMemsetAsync(next, 0, tiles * sizeof(uint32_t), st));
        HIP_TRY(hipMemsetAsync(words, 0, RW_WORDS * sizeof(uint32_t), st));
        launch_tiles<T>(conn, grid, st, r, k, ks, (uint32_t)mask_channel, mask, plan.flip, rounds, now, next, words.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host_words, words, sizeof(host_words), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (prof.launches) (*prof.launches)++;
        if (prof.tile_runs) *prof.tile_runs += host_words[RW_ACTIVE];
        if (host_words[RW_CHANGED] == 0u) break;
    }
    if (plan.fin != FIN_NONE) {
        hipLaunchKernelGGL(k_recon_finish<T>, dim3(stream_grid(n)), dim3(256), 0, st, k, ks, (uint32_t)mask_channel, r, n, plan.fin, (uint32_t)(T)~(T)0);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(st));                             // `words` and `flags` go out of scope behind their last use
    return VPT_OK;
}

static int reconstruct(const char *what, vpt_volume *marker, int marker_channel, vpt_volume *mask, int mask_channel, const ReconPlan &plan, int conn, int rounds,
                       vpt_volume **out, const ReconProfile &prof) {
    const uint64_t n = (uint64_t)mask->nx * (uint64_t)mask->ny * (uint64_t)mask->nz;
    if (n > 0xFFFFFFFEull) return fail(VPT_ERR_UNSUPPORTED, "%s: %llu voxels exceed 2^32 - 2", what, (unsigned long long)n);
    if ((mask->ny + RC_TY - 1) / RC_TY > 65535 || (mask->nz + RC_TZ - 1) / RC_TZ > 65535) return fail(VPT_ERR_UNSUPPORTED, "%s: volume too large", what);
    vpt_context *c = mask->ctx;
    HIP_TRY(hipSetDevice(c->device));
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(c, mask->nx, mask->ny, mask->nz, mask->norm16 ? VPT_FORMAT_R16 : VPT_FORMAT_R8, false, &d));      // every texel is written by the seed
    PhaseClock clock(c->stream);
    if (prof.ms) {                                               // what is in front of the call is not its time
        const hipError_t e = clock.lap(prof.ms);
        if (e != hipSuccess) { vpt_volume_destroy(d); return fail(VPT_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); }
    }
    const int rc = mask->norm16 ? reconstruct_run<uint16_t>(marker, marker_channel, mask, mask_channel, plan, conn, rounds, d, prof)
                                : reconstruct_run<uint8_t>(marker, marker_channel, mask, mask_channel, plan, conn, rounds, d, prof);
    if (rc != VPT_OK) { (void)hipStreamSynchronize(c->stream); vpt_volume_destroy(d); return rc; }
    if (prof.ms) {
        const hipError_t e = clock.lap(prof.ms);
        if (e != hipSuccess) { vpt_volume_destroy(d); return fail(VPT_ERR_HIP, "%s: %s", what, hipGetErrorString(e)); }
    }
    return volume_finish_derived(c, marker->filter, d, out);
}

static int reconstruct_checked(vpt_volume *marker, int marker_channel, vpt_volume *mask, int mask_channel, int op, int connectivity, int rounds, vpt_volume **out,
                               const ReconProfile &prof) {
    if (!marker || !mask || !out) return fail(VPT_ERR_INVALID, "null argument");
    VPT_TRY(check_source("reconstruct", "marker", marker, marker_channel));
    VPT_TRY(check_source("reconstruct", "mask", mask, mask_channel));
    if (marker->ctx != mask->ctx) return fail(VPT_ERR_INVALID, "reconstruct: marker and mask belong to two contexts");
    if (marker->nx != mask->nx || marker->ny != mask->ny || marker->nz != mask->nz)
        return fail(VPT_ERR_INVALID, "reconstruct: marker is %dx%dx%d and mask is %dx%dx%d; vpt_volume_resample brings two grids together", marker->nx, marker->ny,
                    marker->nz, mask->nx, mask->ny, mask->nz);
    if (marker->norm16 != mask->norm16)
        return fail(VPT_ERR_UNSUPPORTED, "reconstruct: the channels of marker (%s) and mask (%s) differ in width (the window makes R8 / R16 of any scalar volume)",
                    format_name(marker->format), format_name(mask->format));
    if (op != VPT_RECONSTRUCT_DILATION && op != VPT_RECONSTRUCT_EROSION)
        return fail(VPT_ERR_INVALID, "reconstruct op %d: VPT_RECONSTRUCT_DILATION (0) or VPT_RECONSTRUCT_EROSION (1) are taken", op);
    VPT_TRY(check_connectivity(connectivity));
    const uint32_t M = mask->norm16 ? 65535u : 255u;
    const ReconPlan plan = { SEED_MARKER, 0u, op == VPT_RECONSTRUCT_EROSION ? M : 0u, FIN_NONE };
    return reconstruct("reconstruct", marker, marker_channel, mask, mask_channel, plan, connectivity, rounds, out, prof);
}

extern "C" int vpt_volume_reconstruct(vpt_volume *marker, int marker_channel, vpt_volume *mask, int mask_channel, int op, int connectivity, vpt_volume **out) {
    return reconstruct_checked(marker, marker_channel, mask, mask_channel, op, connectivity, RC_TILE_ROUNDS, out, ReconProfile{ nullptr, nullptr, nullptr });
}

extern "C" int vpt_volume_reconstruct_timed(vpt_volume *marker, int marker_channel, vpt_volume *mask, int mask_channel, int op, int connectivity, vpt_volume **out,
                                            double *ms, uint32_t *launches, uint64_t *tile_runs) {
    if (!ms || !launches) return fail(VPT_ERR_INVALID, "null argument");
    *ms = 0.0; *launches = 0u;
    if (tile_runs) *tile_runs = 0u;
    return reconstruct_checked(marker, marker_channel, mask, mask_channel, op, connectivity, RC_TILE_ROUNDS, out, ReconProfile{ ms, launches, tile_runs });
}

// (for tests) the cap is checked first: a refused cap touches neither the other arguments nor the device
extern "C" int vpt_volume_reconstruct_capped(vpt_volume *marker, int marker_channel, vpt_volume *mask, int mask_channel, int op, int connectivity, int tile_rounds,
                                             vpt_volume **out, double *ms, uint32_t *launches) {
    if (tile_rounds < 1) return fail(VPT_ERR_INVALID, "tile_rounds %d: a launch makes at least one round", tile_rounds);
    if (ms) *ms = 0.0;
    if (launches) *launches = 0u;
    return reconstruct_checked(marker, marker_channel, mask, mask_channel, op, connectivity, tile_rounds, out, ReconProfile{ ms, launches, nullptr });
}

static int geodesic(vpt_volume *src, int channel, int op, uint32_t h, int connectivity, vpt_volume **out, const ReconProfile &prof) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    VPT_TRY(check_source("geodesic", "src", src, channel));
    if (op < VPT_GEODESIC_FILL_HOLES || op > VPT_GEODESIC_MINIMA)
        return fail(VPT_ERR_INVALID, "geodesic op %d: VPT_GEODESIC_FILL_HOLES (0) .. VPT_GEODESIC_MINIMA (6) are taken", op);
    VPT_TRY(check_connectivity(connectivity));
    const uint32_t M = src->norm16 ? 65535u : 255u;
    const bool takes_h = op == VPT_GEODESIC_HMAX || op == VPT_GEODESIC_HMIN || op == VPT_GEODESIC_DOME;
    if (!takes_h && h != 0u) return fail(VPT_ERR_INVALID, "geodesic %s takes no h: %u is given, 0 is required", GEODESIC_OP_NAMES[op], h);
    if (h > M) return fail(VPT_ERR_INVALID, "geodesic %s h %u: the largest code of %s is %u", GEODESIC_OP_NAMES[op], h, format_name(src->format), M);
    ReconPlan plan = {};
    switch (op) {
        case VPT_GEODESIC_FILL_HOLES:   plan = ReconPlan{ SEED_BORDER, 0u, M, FIN_NONE }; break;
        case VPT_GEODESIC_CLEAR_BORDER: plan = ReconPlan{ SEED_BORDER, 0u, 0u, FIN_SUB }; break;
        case VPT_GEODESIC_HMAX:         plan = ReconPlan{ SEED_SHIFT, h, 0u, FIN_NONE }; break;
        case VPT_GEODESIC_HMIN:         plan = ReconPlan{ SEED_SHIFT, h, M, FIN_NONE }; break;
        case VPT_GEODESIC_DOME:         plan = ReconPlan{ SEED_SHIFT, h, 0u, FIN_SUB }; break;
        case VPT_GEODESIC_MAXIMA:       plan = ReconPlan{ SEED_SHIFT, 1u, 0u, FIN_ABOVE }; break;
        default:                        plan = ReconPlan{ SEED_SHIFT, 1u, M, FIN_BELOW }; break;
    }
    return reconstruct("geodesic", src, channel, src, channel, plan, connectivity, RC_TILE_ROUNDS, out, prof);
}

extern "C" int vpt_volume_geodesic(vpt_volume *src, int channel, int op, uint32_t h, int connectivity, vpt_volume **out) {
    return geodesic(src, channel, op, h, connectivity, out, ReconProfile{ nullptr, nullptr, nullptr });
}

extern "C" int vpt_volume_geodesic_timed(vpt_volume *src, int channel, int op, uint32_t h, int connectivity, vpt_volume **out, double *ms, uint32_t *launches,
                                         uint64_t *tile_runs) {
    if (!ms || !launches) return fail(VPT_ERR_INVALID, "null argument");
    *ms = 0.0; *launches = 0u;
    if (tile_runs) *tile_runs = 0u;
    return geodesic(src, channel, op, h, connectivity, out, ReconProfile{ ms, launches, tile_runs });
}
