// vpt_volume_skeleton.hip — curve skeleton and topological kernel of a value range of a volume by subfield thinning on the device
// (vpt_volume_skeleton and the vpt_skeleton_* family): one uint32 burn pass per voxel, the selection emitter (within), the closing census.
// C-ABI and the contract: include/vpt.h; why a sub-step is order-free, why the tile cull is exact, compiler figures and measurements:
// DESIGN.md "Skeleton".
//
// State as bit planes: X (the object), BORDER (the border voxels of X at the start of the pass) and MARK (the isthmus marks), one bit per
// voxel, 32 voxels along x a word, rows padded to whole tiles (2 words a tile).  The values array is touched once per voxel by the seed
// and once more by the store of the pass in which the voxel is deleted.  A pass is one launch of k_sk_border and eight of k_sk_step, one
// per subfield; no workgroup waits for another: launch boundaries order the sub-steps.  Within a launch a workgroup clears bits only in
// the words of its own tile, and the bits it clears are read by no other voxel's test in that launch (two voxels of one subfield are
// never 26-adjacent), so a neighbouring tile that stages such a word may see it before or after the clearing: it does not look at the bit.
#include "vpt_volume_skeleton.h"

#define SK_TX 64
#define SK_TY 8
#define SK_TZ 4
#define SK_MAX_AXIS 4096           // vpt_volume_distance's limit
#define SK_COUNT_SLOTS 64
#define SK_NO_CULL 1u
enum { SK_CHANGED = 0, SK_ACTIVE = 1, SK_WORDS = 2 };            // running sums over the passes; the host takes differences

// ---------------------------------------------------------------------------------------------
// the 3 x 3 x 3 neighbourhood as 27 bits: bit 9 (dz + 1) + 3 (dy + 1) + (dx + 1), the centre is bit 13
// ---------------------------------------------------------------------------------------------
constexpr uint32_t nb_mask(int kind) {      // 0: dx = -1, 1: dx = +1, 2: dy = -1, 3: dy = +1, 4: N18, 5: N6
    uint32_t m = 0u;
    for (int i = 0; i < 27; i++) {
        const int dx = i % 3 - 1, dy = i / 3 % 3 - 1, dz = i / 9 - 1;
        const int nonzero = (dx != 0) + (dy != 0) + (dz != 0);
        const bool in = kind == 0 ? dx == -1 : kind == 1 ? dx == 1 : kind == 2 ? dy == -1 : kind == 3 ? dy == 1 : kind == 4 ? (nonzero == 1 || nonzero == 2) : nonzero == 1;
        if (in) m |= 1u << i;
    }
    return m;
}
constexpr uint32_t NB_ALL = (1u << 27) - 1u, NB_CENTRE = 1u << 13;
constexpr uint32_t NB_X0 = nb_mask(0), NB_X2 = nb_mask(1), NB_Y0 = nb_mask(2), NB_Y2 = nb_mask(3), NB_18 = nb_mask(4), NB_6 = nb_mask(5);

// the set grown by one step along an axis, inside the cube: a shift by 1 / 3 / 9 moves a voxel to its x / y / z neighbour; what a shift
// carries into the next row or slab lands in the column or row that has no such neighbour and is masked off, and so is what leaves the
// 27 bits (the next dilation would shift it back in)
__device__ __forceinline__ uint32_t nb_grow_x(uint32_t s) { return ((s << 1) & (NB_ALL & ~NB_X0)) | ((s >> 1) & ~NB_X2); }
__device__ __forceinline__ uint32_t nb_grow_y(uint32_t s) { return ((s << 3) & (NB_ALL & ~NB_Y0)) | ((s >> 3) & ~NB_Y2); }
__device__ __forceinline__ uint32_t nb_grow_z(uint32_t s) { return ((s << 9) | (s >> 9)) & NB_ALL; }

// is `set` (non-empty, without the centre) one 26-connected component?  Flood from its lowest voxel: the 26-dilation is the three axis
// dilations composed.  A component of at most 26 voxels is reached in at most 25 steps.
__device__ __forceinline__ bool nb_one_component_26(uint32_t set) {
    uint32_t s = set & (0u - set);
    for (;;) {
        uint32_t t = s | nb_grow_x(s);
        t |= nb_grow_y(t);
        t |= nb_grow_z(t);
        t &= set;
        if (t == s) break;
        s = t;
    }
    return s == set;
}
// B(p) == 1: the background voxels of N6 are non-empty and all lie in one 6-connected component of N18 \ X
__device__ __forceinline__ bool nb_one_background_6(uint32_t obj) {
    const uint32_t bg = NB_18 & ~obj, faces = bg & NB_6;
    if (faces == 0u) return false;
    uint32_t s = faces & (0u - faces);
    for (;;) {
        const uint32_t t = (s | nb_grow_x(s) | nb_grow_y(s) | nb_grow_z(s)) & bg;
        if (t == s) break;
        s = t;
    }
    return (s & NB_6) == faces;
}

// ---------------------------------------------------------------------------------------------
// seed: threshold into the X plane, the values 0 / KEPT, the object's voxel count
// ---------------------------------------------------------------------------------------------
// A wave owns 64 voxels of a row: one ballot is two words of the plane.  Bits beyond nx stay 0.
template <typename T>
__global__ __launch_bounds__(256) void k_sk_seed(const T *__restrict__ src, uint32_t *__restrict__ values, uint32_t *__restrict__ plane, int nx, int tnx, size_t rows,
                                                uint32_t lo, uint32_t hi, unsigned long long *__restrict__ count) {
    const int lane = (int)threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (size_t)gridDim.x * 4, items = rows * (size_t)tnx;
    unsigned long long counted = 0ull;                           // (wave-uniform)
    for (size_t item = wave; item < items; item += waves) {
        const size_t row = item / (size_t)tnx; const int seg = (int)(item % (size_t)tnx);
        const int x = seg * 64 + lane;
        bool in = false;
        if (x < nx) {
            const uint32_t c = (uint32_t)src[row * (size_t)nx + (size_t)x];
            in = c >= lo && c <= hi;
            values[row * (size_t)nx + (size_t)x] = in ? VPT_THIN_KEPT : 0u;
        }
        const unsigned long long b = __ballot(in);
        if (lane < 2) plane[row * (size_t)(2 * tnx) + (size_t)(2 * seg + lane)] = (uint32_t)(b >> (32 * lane));
        counted += (unsigned long long)__popcll(b);
    }
    if (lane == 0 && counted) atomicAdd(&count[wave % SK_COUNT_SLOTS], counted);
}

// a word of a plane, 0 outside the volume
__device__ __forceinline__ uint32_t sk_word(const uint32_t *__restrict__ plane, int ny, int nz, int wpr, int z, int y, int wx) {
    if (z < 0 || z >= nz || y < 0 || y >= ny || wx < 0 || wx >= wpr) return 0u;
    return plane[((size_t)z * (size_t)ny + (size_t)y) * (size_t)wpr + (size_t)wx];
}

// ---------------------------------------------------------------------------------------------
// the start of a pass: which tiles take part, and their border voxels, k_sk_border
// ---------------------------------------------------------------------------------------------
// One wave a tile, a lane a word.  A tile takes part in this pass when it or one of its 26 neighbouring tiles changed a bit in the last
// pass (`prev`; DESIGN.md has the proof that nothing else can change), or when `all` is set (the first pass, or the cull switched off).
// The BORDER words of a tile that does not take part are those of the last pass: they would come out the same.  The tile's entry of the
// flag array that the NEXT pass's sub-steps will set is cleared here (`clear`: the third of three arrays, nobody reads or sets it now).
__global__ __launch_bounds__(64) void k_sk_border(const uint32_t *__restrict__ X, uint32_t *__restrict__ border, const uint32_t *__restrict__ prev, uint32_t *__restrict__ active,
                                                  uint32_t *__restrict__ clear, unsigned long long *__restrict__ words, int ny, int nz, int wpr, uint32_t all) {
    const int lane = (int)threadIdx.x;
    const int bx = (int)blockIdx.x, by = (int)blockIdx.y, bz = (int)blockIdx.z, gx = (int)gridDim.x, gy = (int)gridDim.y, gz = (int)gridDim.z;
    const size_t tile = ((size_t)bz * (size_t)gy + (size_t)by) * (size_t)gx + (size_t)bx;
    bool flag = all != 0u;
    if (!flag && lane < 27) {
        const int tx = bx + lane % 3 - 1, ty = by + lane / 3 % 3 - 1, tz = bz + lane / 9 - 1;
        if (tx >= 0 && tx < gx && ty >= 0 && ty < gy && tz >= 0 && tz < gz) flag = prev[((size_t)tz * (size_t)gy + (size_t)ty) * (size_t)gx + (size_t)tx] != 0u;
    }
    const bool takes_part = __ballot(flag) != 0ull;
    if (lane == 0) {
        active[tile] = takes_part ? 1u : 0u;
        clear[tile] = 0u;
        if (takes_part) atomicAdd(&words[SK_ACTIVE], 1ull);
    }
    if (!takes_part) return;
    const int z = bz * SK_TZ + (lane >> 4), y = by * SK_TY + ((lane >> 1) & 7), wx = bx * 2 + (lane & 1);
    if (y >= ny || z >= nz) return;
    const uint32_t c = sk_word(X, ny, nz, wpr, z, y, wx);
    const uint32_t xm = (c << 1) | (sk_word(X, ny, nz, wpr, z, y, wx - 1) >> 31), xp = (c >> 1) | (sk_word(X, ny, nz, wpr, z, y, wx + 1) << 31);
    const uint32_t inner = xm & xp & sk_word(X, ny, nz, wpr, z, y - 1, wx) & sk_word(X, ny, nz, wpr, z, y + 1, wx) & sk_word(X, ny, nz, wpr, z - 1, y, wx) &
                           sk_word(X, ny, nz, wpr, z + 1, y, wx);
    border[((size_t)z * (size_t)ny + (size_t)y) * (size_t)wpr + (size_t)wx] = c & ~inner;
}

// ---------------------------------------------------------------------------------------------
// one sub-step, k_sk_step
// ---------------------------------------------------------------------------------------------
// A workgroup owns a tile of 64 x 8 x 4 voxels and stages its X words with a rim of one row, one slab and one word: 6 x 10 x 4 words of
// LDS.  The voxels of subfield s in the tile are 32 x 4 x 2 = 256: one per thread.  A thread whose voxel is a candidate (in BORDER, in X,
// without a mark) queues it in LDS; then thread i takes the i-th queued voxel, so the topology test runs on full waves however sparse
// the candidates are.  The test gathers the 27 bits from LDS into one register and floods in registers (above).  A deletion clears the
// bit with an atomic-and on the tile's own word in memory (sixteen candidates share a word) and stores the pass into the values; a mark
// sets the bit in MARK the same way.  A tile that changed anything sets its flag and adds its count to words[SK_CHANGED].
__global__ __launch_bounds__(256) void k_sk_step(uint32_t *__restrict__ X, const uint32_t *__restrict__ border, uint32_t *__restrict__ mark, uint32_t *__restrict__ values,
                                                 const uint32_t *__restrict__ active, uint32_t *__restrict__ changed, unsigned long long *__restrict__ words,
                                                 int nx, int ny, int nz, int wpr, int s, int mode, uint32_t pass) {
    const int bx = (int)blockIdx.x, by = (int)blockIdx.y, bz = (int)blockIdx.z;
    const size_t tile = ((size_t)bz * (size_t)gridDim.y + (size_t)by) * (size_t)gridDim.x + (size_t)bx;
    if (active[tile] == 0u) return;                             // (uniform)
    __shared__ uint32_t rim[SK_TZ + 2][SK_TY + 2][4];
    __shared__ uint32_t queue[256];
    __shared__ uint32_t queued, did;
    const int tid = (int)threadIdx.x;
    const int x0 = bx * SK_TX, y0 = by * SK_TY, z0 = bz * SK_TZ;
    if (tid < (SK_TZ + 2) * (SK_TY + 2) * 4) {
        const int w = tid & 3, yy = (tid >> 2) % (SK_TY + 2), zz = (tid >> 2) / (SK_TY + 2);
        rim[zz][yy][w] = sk_word(X, ny, nz, wpr, z0 - 1 + zz, y0 - 1 + yy, bx * 2 - 1 + w);
    }
    if (tid == 0) { queued = 0u; did = 0u; }
    __syncthreads();
    {   // this thread's voxel of the subfield: is it a candidate?
        const int lx = 2 * (tid & 31) + (s & 1), ly = 2 * ((tid >> 5) & 3) + ((s >> 1) & 1), lz = 2 * (tid >> 7) + ((s >> 2) & 1);
        const int y = y0 + ly, z = z0 + lz;
        if (y < ny && z < nz) {
            const size_t at = ((size_t)z * (size_t)ny + (size_t)y) * (size_t)wpr + (size_t)(bx * 2 + (lx >> 5));
            uint32_t c = rim[lz + 1][ly + 1][1 + (lx >> 5)] & border[at];
            if (mode == VPT_THIN_ISTHMUS) c &= ~mark[at];
            if ((c >> (lx & 31)) & 1u) queue[atomicAdd(&queued, 1u)] = (uint32_t)(lx | (ly << 6) | (lz << 9));
        }
    }
    __syncthreads();
    if (tid < (int)queued) {
        const uint32_t q = queue[tid];
        const int lx = (int)(q & 63u), ly = (int)((q >> 6) & 7u), lz = (int)(q >> 9);
        // the 27 bits: per (dz, dy) the three bits lx - 1 .. lx + 1 of a row of four words whose bit 32 is the tile's voxel 0
        const int first = lx + 31, wi = first >> 5, sh = first & 31;
        uint32_t nb = 0u;
#pragma unroll
        for (int dz = 0; dz < 3; dz++) {
#pragma unroll
            for (int dy = 0; dy < 3; dy++) {
                const uint32_t *row = rim[lz + dz][ly + dy];
                const unsigned long long two = ((unsigned long long)row[wi + 1] << 32) | (unsigned long long)row[wi];
                nb |= ((uint32_t)(two >> sh) & 7u) << (9 * dz + 3 * dy);
            }
        }
        const uint32_t obj = nb & ~NB_CENTRE;
        bool kill = false, flag = false;
        if (obj != 0u && !(mode == VPT_THIN_ENDS && (obj & (obj - 1u)) == 0u)) {
            const bool one = nb_one_component_26(obj);
            if (!one) flag = mode == VPT_THIN_ISTHMUS;         // C(p) >= 2
            else kill = nb_one_background_6(obj);
        }
        if (kill || flag) {
            const int x = x0 + lx, y = y0 + ly, z = z0 + lz;
            const size_t at = ((size_t)z * (size_t)ny + (size_t)y) * (size_t)wpr + (size_t)(bx * 2 + (lx >> 5));
            if (kill) {
                atomicAnd(&X[at], ~(1u << (lx & 31)));
                values[((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)x] = pass;
            } else {
                atomicOr(&mark[at], 1u << (lx & 31));
            }
            atomicAdd(&did, 1u);
        }
    }
    __syncthreads();
    if (tid == 0 && did) { changed[tile] = 1u; atomicAdd(&words[SK_CHANGED], (unsigned long long)did); }
}

// ---------------------------------------------------------------------------------------------
// the closing census, k_sk_census
// ---------------------------------------------------------------------------------------------
// A thread a word of the final X plane; a word without a kept voxel (nearly all of them) costs one load.  Otherwise the nine rows around
// it come as three words each, folded into a 34-bit window whose bit j + 1 is voxel j of the word, and every kept voxel counts its kept
// 26-neighbours: 0, 1, 2, >= 3 go to four sums (isolated, ends, regular, junctions).
__global__ __launch_bounds__(256) void k_sk_census(const uint32_t *__restrict__ X, int ny, int nz, int wpr, size_t plane_words, unsigned long long *__restrict__ sums) {
    unsigned long long mine[4] = { 0ull, 0ull, 0ull, 0ull };
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < plane_words; i += (size_t)gridDim.x * 256) {
        uint32_t c = X[i];
        if (c == 0u) continue;
        const int wx = (int)(i % (size_t)wpr); const size_t r = i / (size_t)wpr; const int y = (int)(r % (size_t)ny), z = (int)(r / (size_t)ny);
        unsigned long long win[9];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const int zz = z + k / 3 - 1, yy = y + k % 3 - 1;
            win[k] = (unsigned long long)(sk_word(X, ny, nz, wpr, zz, yy, wx - 1) >> 31) | ((unsigned long long)sk_word(X, ny, nz, wpr, zz, yy, wx) << 1) |
                     ((unsigned long long)(sk_word(X, ny, nz, wpr, zz, yy, wx + 1) & 1u) << 33);
        }
        while (c) {
            const int b = __ffs((int)c) - 1;
            c &= c - 1u;
            int n = -1;                                         // the voxel itself is in its window
#pragma unroll
            for (int k = 0; k < 9; k++) n += __popc((uint32_t)(win[k] >> b) & 7u);
            mine[min(n, 3)]++;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        unsigned long long m = mine[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m += ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(m >> 32), o) << 32) | (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)m, o);
        if (((int)threadIdx.x & 63) == 0 && m) atomicAdd(&sums[k], m);
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// the body of vpt_volume_skeleton behind the argument checks; `k` is freed by the caller on failure
static int skeleton_build(vpt_skeleton *k, uint32_t lo, uint32_t hi, int mode, int passes, uint32_t flags) {
    hipStream_t st = k->ctx->stream;
    const int nx = k->nx, ny = k->ny, nz = k->nz;
    const int tnx = (nx + SK_TX - 1) / SK_TX, tny = (ny + SK_TY - 1) / SK_TY, tnz = (nz + SK_TZ - 1) / SK_TZ;      // <= 64, 512, 1024
    const int wpr = 2 * tnx;
    const size_t rows = (size_t)ny * (size_t)nz, plane_words = rows * (size_t)wpr, tiles = (size_t)tnx * (size_t)tny * (size_t)tnz;
    DevBuf<uint32_t> planes, tile_flags;                         // X, BORDER, MARK; active + three rounds of changed flags: freed when the call returns
    DevBuf<unsigned long long> words, count;                     // SK_WORDS running sums; the seed's slots, then the census' four sums
    HIP_TRY(planes.alloc(3 * plane_words));
    HIP_TRY(tile_flags.alloc(4 * tiles));
    HIP_TRY(words.alloc(SK_WORDS));
    HIP_TRY(count.alloc(SK_COUNT_SLOTS));
    uint32_t *X = planes.get(), *border = X + plane_words, *mark = border + plane_words;
    uint32_t *active = tile_flags.get(), *changed = active + tiles;
    HIP_TRY(hipMemsetAsync(mark, 0, plane_words * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(tile_flags, 0, 4 * tiles * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(words, 0, SK_WORDS * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(count, 0, SK_COUNT_SLOTS * sizeof(unsigned long long), st));
    HIP_TRY(hipStreamSynchronize(st));                          // what is in front of the call is not its time
    PhaseClock clock(st);
    // ---- seed
    unsigned long long host_count[SK_COUNT_SLOTS] = {};
    const dim3 seed_grid(stream_grid(rows * (size_t)tnx, 4));
    if (k->norm16) hipLaunchKernelGGL(k_sk_seed<uint16_t>, seed_grid, dim3(256), 0, st, (const uint16_t *)k->texels.get(), k->values.get(), X, nx, tnx, rows, lo, hi, count.get());
    else hipLaunchKernelGGL(k_sk_seed<uint8_t>, seed_grid, dim3(256), 0, st, (const uint8_t *)k->texels.get(), k->values.get(), X, nx, tnx, rows, lo, hi, count.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_count, count, sizeof(host_count), hipMemcpyDeviceToHost, st));
    HIP_TRY(clock.lap(&k->ms[0]));
    k->launches = 1;
    for (int i = 0; i < SK_COUNT_SLOTS; i++) k->info.object_voxels += host_count[i];
    k->info.converged = 1;
    if (k->info.object_voxels == 0) return VPT_OK;              // nothing to thin and nothing to count
    // ---- passes.  The sub-steps of pass p set changed[p % 3]; its border launch reads changed[(p - 1) % 3] and clears changed[(p + 1) % 3].
    const dim3 grid((unsigned)tnx, (unsigned)tny, (unsigned)tnz);
    unsigned long long host_words[SK_WORDS] = {}, before[SK_WORDS] = {};
    for (uint32_t pass = 1u; ; pass++) {
        const uint32_t all = (pass == 1u || (flags & SK_NO_CULL)) ? 1u : 0u;
        hipLaunchKernelGGL(k_sk_border, grid, dim3(64), 0, st, (const uint32_t *)X, border, (const uint32_t *)(changed + (size_t)((pass + 2u) % 3u) * tiles), active,
                           changed + (size_t)((pass + 1u) % 3u) * tiles, words.get(), ny, nz, wpr, all);
        HIP_TRY(hipGetLastError());
        HIP_TRY(clock.lap_add(&k->ms[1]));
        for (int s = 0; s < 8; s++) {
            hipLaunchKernelGGL(k_sk_step, grid, dim3(256), 0, st, X, (const uint32_t *)border, mark, k->values.get(), (const uint32_t *)active,
                               changed + (size_t)(pass % 3u) * tiles, words.get(), nx, ny, nz, wpr, s, mode, pass);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(host_words, words, sizeof(host_words), hipMemcpyDeviceToHost, st));
        HIP_TRY(clock.lap_add(&k->ms[2]));
        k->launches += 9;
        k->tile_visits += 8ull * (host_words[SK_ACTIVE] - before[SK_ACTIVE]);
        k->info.passes = pass;
        const bool idle = host_words[SK_CHANGED] == before[SK_CHANGED];
        k->info.converged = idle ? 1 : 0;
        if (idle || (passes > 0 && pass == (uint32_t)passes)) break;
        before[SK_CHANGED] = host_words[SK_CHANGED]; before[SK_ACTIVE] = host_words[SK_ACTIVE];
    }
    // ---- census
    unsigned long long sums[4] = {};
    HIP_TRY(hipMemsetAsync(count, 0, 4 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_sk_census, dim3(stream_grid(plane_words)), dim3(256), 0, st, (const uint32_t *)X, ny, nz, wpr, plane_words, count.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sums, count, sizeof(sums), hipMemcpyDeviceToHost, st));
    HIP_TRY(clock.lap(&k->ms[3]));                              // the planes and flags go out of scope behind their last use
    k->launches += 1;
    k->info.isolated = sums[0]; k->info.ends = sums[1]; k->info.regular = sums[2]; k->info.junctions = sums[3];
    k->info.kept_voxels = sums[0] + sums[1] + sums[2] + sums[3];
    return VPT_OK;
}

static int skeleton_create(vpt_volume *src, uint32_t lo, uint32_t hi, int mode, int passes, uint32_t flags, vpt_skeleton **out) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (src->format != VPT_FORMAT_R8 && src->format != VPT_FORMAT_R16)
        return fail(VPT_ERR_UNSUPPORTED, "skeletons are taken in one-channel unsigned normalised volumes (R8, R16; the window makes one of any scalar volume), not in %s",
                    format_name(src->format));
    const uint32_t M = src->norm16 ? 65535u : 255u;
    if (lo > hi) return fail(VPT_ERR_INVALID, "skeleton range [%u, %u]: lo exceeds hi", lo, hi);
    if (hi > M) return fail(VPT_ERR_INVALID, "skeleton range [%u, %u]: the largest code of %s is %u", lo, hi, format_name(src->format), M);
    if (mode != VPT_THIN_KERNEL && mode != VPT_THIN_ENDS && mode != VPT_THIN_ISTHMUS)
        return fail(VPT_ERR_INVALID, "mode %d: VPT_THIN_KERNEL (0), VPT_THIN_ENDS (1) or VPT_THIN_ISTHMUS (2) are taken", mode);
    if (passes < 0) return fail(VPT_ERR_INVALID, "passes %d: 0 (to the fixed point) or a positive cap are taken", passes);
    if (src->nx > SK_MAX_AXIS || src->ny > SK_MAX_AXIS || src->nz > SK_MAX_AXIS) return fail(VPT_ERR_UNSUPPORTED, "volume too large");
    vpt_context *ctx = src->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<vpt_skeleton> k(new vpt_skeleton());
    VPT_TRY(field_capture(k.get(), src));
    const int rc = skeleton_build(k.get(), lo, hi, mode, passes, flags);
    if (rc != VPT_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }      // the buffers are freed on return: nothing may still use them
    *out = k.release();
    return VPT_OK;
}

extern "C" int vpt_volume_skeleton(vpt_volume *src, uint32_t lo, uint32_t hi, int mode, int passes, vpt_skeleton **out) {
    return skeleton_create(src, lo, hi, mode, passes, 0u, out);
}

extern "C" int vpt_volume_skeleton_capped(vpt_volume *src, uint32_t lo, uint32_t hi, int mode, int passes, int flags, vpt_skeleton **out) {
    if (flags & ~(int)SK_NO_CULL) return fail(VPT_ERR_INVALID, "skeleton flags %d: bit 0 (no tile cull) is taken", flags);
    return skeleton_create(src, lo, hi, mode, passes, (uint32_t)flags, out);
}

extern "C" int vpt_skeleton_info(vpt_skeleton *k, struct vpt_skeleton_info *info) {
    if (!k || !info) return fail(VPT_ERR_INVALID, "null argument");
    *info = k->info;
    return VPT_OK;
}

extern "C" int vpt_skeleton_burn(vpt_skeleton *k, int x, int y, int z, int w, int h, int d, uint32_t *host_dst, size_t nbytes) {
    return field_read(k, x, y, z, w, h, d, host_dst, nbytes);
}

extern "C" int vpt_skeleton_within(vpt_skeleton *k, uint32_t k_lo, uint32_t k_hi, uint32_t fill, vpt_volume **out) {
    if (!k || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (k_lo > k_hi) return fail(VPT_ERR_INVALID, "burn passes %u .. %u: from exceeds to", k_lo, k_hi);
    return field_select(k, k_lo, k_hi, fill, out);
}

extern "C" int vpt_skeleton_profile(vpt_skeleton *k, double *ms, uint64_t *launches, uint64_t *tiles) {
    if (!k || !ms || !launches || !tiles) return fail(VPT_ERR_INVALID, "null argument");
    memcpy(ms, k->ms, sizeof(k->ms));
    *launches = k->launches; *tiles = k->tile_visits;
    return VPT_OK;
}

extern "C" int vpt_skeleton_destroy(vpt_skeleton *k) { return field_destroy(k); }
