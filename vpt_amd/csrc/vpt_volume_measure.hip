// vpt_volume_measure.hip — what a labelling is asked next, on the device: thirteen exact integer accumulators per component
// (vpt_components_measure: voxels, bounding box, index sums, range / sum / sum of squares of a measured channel, surface faces) and the
// volume that keeps a SET of ranks (vpt_components_keep_set).  C-ABI and the contract: include/vpt.h; kernel form, compiler figures and
// measurements: DESIGN.md "Measuring components".
//
// Everything is an integer sum, minimum or maximum: no float arithmetic, no workgroup waits for another, and the order in which the
// atomics arrive does not show in the result.
#include "vpt_volume_components.h"

// ---------------------------------------------------------------------------------------------
// the keyed reduction: k_measure<TV, STRIDE>
// ---------------------------------------------------------------------------------------------
// A workgroup of 256 threads owns a box of MS_BX x MS_BY x MS_BZ voxels; wave w takes the rows w, w + 4, ... of the box, 64 consecutive
// voxels of one row a step.  Runs of one rank along x are found as k_sizes finds them (__shfl_up, __ballot); a run's totals are closed
// forms of its two ends (count, sum of x, y count, z count) or come from a segmented scan towards the run's head (faces, value sum, sum of
// squares, value minimum and maximum: lane i adds lane i + o while that lane is in its run, o = 1 .. 32).  The head of a run whose rank is
// in the window adds the totals into the workgroup's LDS table, keyed by rank: open addressing over MS_SLOTS slots with linear probing, a
// slot claimed with one compare-and-swap on its key, then LDS integer atomics.  A head that finds no slot within MS_PROBES probes (the box
// holds more distinct ranks than the table takes) adds the same totals straight into the global record, so nothing is lost.  At the end
// every occupied slot goes to its global record: one global atomic per field.  One exception spares most of them: `sizes` holds the voxel
// count of every component of the window (the list's), and a slot (or a run without a slot) that has counted ALL of its component's voxels
// is that record's only contributor, so it writes the 88 bytes with plain stores over the initial record.  A small component lies within
// one box more often than not, and scattered 8-byte atomics were the whole time of a volume of them (DESIGN.md has the figures).
//
// Inside a box every 32-bit LDS word is wide enough: count <= 4096, index sums <= 4096 * 4095 < 2^24, value sum <= 4096 * 65535 < 2^28,
// faces <= 6 * 4096; only the sum of squares (<= 4096 * 65535^2 < 2^44) is a 64-bit word.  The global records are 64-bit sums whose
// bounds include/vpt.h states.
//
// Bounds of the loads: a lane with x >= nx reads nothing (rank 0); rows with y >= ny or z >= nz are skipped by the whole wave; a
// neighbour's rank is read only behind the test that the neighbour lies inside the volume; a rank r in the window has r - first - 1 < n,
// the length of the global table.
#define MS_BX 64
#define MS_BY 8
#define MS_BZ 8
#define MS_ROWS (MS_BY * MS_BZ)
#define MS_SLOTS 512
#define MS_PROBES 16
// the 32-bit words of a slot (the key and the 64-bit sum of squares have arrays of their own)
enum { F_COUNT = 0, F_MIN_X, F_MIN_Y, F_MIN_Z, F_MAX_X, F_MAX_Y, F_MAX_Z, F_VMIN, F_VMAX, F_SUM_X, F_SUM_Y, F_SUM_Z, F_VSUM, F_FACES, F_WORDS };
#define MS_LDS_BYTES (MS_SLOTS * (4 + 4 * F_WORDS + 8))
static_assert(MS_BX == 64, "a wave step is one row of the box");
static_assert((MS_SLOTS & (MS_SLOTS - 1)) == 0 && MS_PROBES <= MS_SLOTS, "the probe sequence wraps with a mask");
static_assert(sizeof(vpt_component_measure) == 88, "the global table is the caller's records");

// the totals of one run into the global record (the flush of a slot, and the path of a run that found no slot)
__device__ __forceinline__ void record_add(vpt_component_measure *rec, uint32_t count, uint32_t min_x, uint32_t min_y, uint32_t min_z, uint32_t max_x,
                                           uint32_t max_y, uint32_t max_z, uint32_t vmin, uint32_t vmax, unsigned long long sum_x,
                                           unsigned long long sum_y, unsigned long long sum_z, unsigned long long vsum, unsigned long long vsq,
                                           unsigned long long faces) {
    atomicAdd((unsigned long long *)&rec->voxels, (unsigned long long)count);
    atomicMin(&rec->min_x, min_x); atomicMin(&rec->min_y, min_y); atomicMin(&rec->min_z, min_z);
    atomicMax(&rec->max_x, max_x); atomicMax(&rec->max_y, max_y); atomicMax(&rec->max_z, max_z);
    atomicMin(&rec->value_min, vmin); atomicMax(&rec->value_max, vmax);
    atomicAdd((unsigned long long *)&rec->sum_x, sum_x); atomicAdd((unsigned long long *)&rec->sum_y, sum_y);
    atomicAdd((unsigned long long *)&rec->sum_z, sum_z);
    atomicAdd((unsigned long long *)&rec->value_sum, vsum); atomicAdd((unsigned long long *)&rec->value_sum_sq, vsq);
    atomicAdd((unsigned long long *)&rec->faces, faces);
}

// the same totals as the whole record: the caller has counted every voxel of the component, nobody else writes this record
__device__ __forceinline__ void record_store(vpt_component_measure *rec, uint32_t count, uint32_t min_x, uint32_t min_y, uint32_t min_z, uint32_t max_x,
                                             uint32_t max_y, uint32_t max_z, uint32_t vmin, uint32_t vmax, unsigned long long sum_x,
                                             unsigned long long sum_y, unsigned long long sum_z, unsigned long long vsum, unsigned long long vsq,
                                             unsigned long long faces) {
    vpt_component_measure r;
    r.voxels = count; r.min_x = min_x; r.min_y = min_y; r.min_z = min_z; r.max_x = max_x; r.max_y = max_y; r.max_z = max_z;
    r.value_min = vmin; r.value_max = vmax; r.sum_x = sum_x; r.sum_y = sum_y; r.sum_z = sum_z; r.value_sum = vsum; r.value_sum_sq = vsq; r.faces = faces;
    *rec = r;
}

// every record of the window before the pass: sums 0, minima at their largest value, maxima 0
__global__ __launch_bounds__(256) void k_measure_init(vpt_component_measure *__restrict__ table, uint32_t n) {
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < n; k += gridDim.x * 256u) {
        vpt_component_measure r = {};
        r.min_x = r.min_y = r.min_z = r.value_min = 0xFFFFFFFFu;
        table[k] = r;
    }
}

template <typename TV, int STRIDE>
__global__ __launch_bounds__(256) void k_measure(const uint32_t *__restrict__ L, const TV *__restrict__ values, int channel, int nx, int ny, int nz,
                                                uint32_t first, uint32_t n, const uint32_t *__restrict__ sizes,
                                                vpt_component_measure *__restrict__ table) {
    __shared__ uint32_t s_key[MS_SLOTS];
    __shared__ uint32_t s_word[F_WORDS][MS_SLOTS];
    __shared__ unsigned long long s_vsq[MS_SLOTS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int s = tid; s < MS_SLOTS; s += 256) {
        s_key[s] = 0u; s_vsq[s] = 0ull;
#pragma unroll
        for (int f = 0; f < F_WORDS; f++) s_word[f][s] = (f == F_MIN_X || f == F_MIN_Y || f == F_MIN_Z || f == F_VMIN) ? 0xFFFFFFFFu : 0u;
    }
    __syncthreads();
    const int x = (int)blockIdx.x * MS_BX + lane, y0 = (int)blockIdx.y * MS_BY, z0 = (int)blockIdx.z * MS_BZ;
    const size_t row = (size_t)nx, plane = (size_t)nx * (size_t)ny;
    for (int r = wave; r < MS_ROWS; r += 4) {
        const int y = y0 + r % MS_BY, z = z0 + r / MS_BY;
        if (y >= ny || z >= nz) continue;                           // (wave-uniform)
        const size_t i = (size_t)z * plane + (size_t)y * row + (size_t)x;
        const uint32_t l = x < nx ? L[i] : 0u;
        const uint32_t w = (l - first - 1u < n) ? l : 0u;           // the rank if it is in the window (rank 0 wraps to 2^32 - 1 - first >= n)
        if (__ballot(w != 0u) == 0ull) continue;
        const uint32_t left = __shfl_up(l, 1), right = __shfl_down(l, 1);
        uint32_t v = 0u, faces = 0u;
        if (w) {
            v = (uint32_t)values[i * STRIDE + (size_t)channel];
            faces = (x == 0 || (lane ? left : L[i - 1]) != l) + (x == nx - 1 || (lane != 63 ? right : L[i + 1]) != l)
                  + (y == 0 || L[i - row] != l) + (y == ny - 1 || L[i + row] != l) + (z == 0 || L[i - plane] != l) + (z == nz - 1 || L[i + plane] != l);
        }
        // runs of one windowed rank: `end` is the last lane of this lane's run
        const uint32_t before = __shfl_up(w, 1);
        const bool head = lane == 0 || w != before;
        const unsigned long long heads = __ballot(head);
        const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
        const int end = rest ? lane + __ffsll(rest) - 1 : 63;
        uint32_t vsum = v, vmin = v, vmax = v;
        unsigned long long vsq = (unsigned long long)v * v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t a = __shfl_down(vsum, o), b = __shfl_down(faces, o), c = __shfl_down(vmin, o), d = __shfl_down(vmax, o);
            const unsigned long long e = __shfl_down(vsq, o);
            if (lane + o <= end) { vsum += a; faces += b; vmin = min(vmin, c); vmax = max(vmax, d); vsq += e; }
        }
        if (!head || !w) continue;
        const uint32_t count = (uint32_t)(end - lane + 1), x0 = (uint32_t)x, x1 = (uint32_t)(x + end - lane);
        const uint32_t sum_x = (x0 + x1) * count / 2u;              // (x0 + x1) count is even: an odd x0 + x1 is an even count
        // ---- the slot of rank w
        int slot = -1;
        uint32_t s = (w * 2654435761u) >> 16;
        for (int probe = 0; probe < MS_PROBES; probe++, s++) {
            const uint32_t at = s & (MS_SLOTS - 1);
            const uint32_t old = atomicCAS(&s_key[at], 0u, w);
            if (old == 0u || old == w) { slot = (int)at; break; }
        }
        if (slot >= 0) {
            atomicAdd(&s_word[F_COUNT][slot], count);
            atomicMin(&s_word[F_MIN_X][slot], x0); atomicMin(&s_word[F_MIN_Y][slot], (uint32_t)y); atomicMin(&s_word[F_MIN_Z][slot], (uint32_t)z);
            atomicMax(&s_word[F_MAX_X][slot], x1); atomicMax(&s_word[F_MAX_Y][slot], (uint32_t)y); atomicMax(&s_word[F_MAX_Z][slot], (uint32_t)z);
            atomicMin(&s_word[F_VMIN][slot], vmin); atomicMax(&s_word[F_VMAX][slot], vmax);
            atomicAdd(&s_word[F_SUM_X][slot], sum_x); atomicAdd(&s_word[F_SUM_Y][slot], (uint32_t)y * count); atomicAdd(&s_word[F_SUM_Z][slot], (uint32_t)z * count);
            atomicAdd(&s_word[F_VSUM][slot], vsum); atomicAdd(&s_word[F_FACES][slot], faces);
            atomicAdd(&s_vsq[slot], vsq);
        } else if (count == sizes[w - first - 1u]) {               // the run is the whole component
            record_store(&table[w - first - 1u], count, x0, (uint32_t)y, (uint32_t)z, x1, (uint32_t)y, (uint32_t)z, vmin, vmax, sum_x,
                         (unsigned long long)y * count, (unsigned long long)z * count, vsum, vsq, faces);
        } else {
            record_add(&table[w - first - 1u], count, x0, (uint32_t)y, (uint32_t)z, x1, (uint32_t)y, (uint32_t)z, vmin, vmax, sum_x,
                       (unsigned long long)y * count, (unsigned long long)z * count, vsum, vsq, faces);
        }
    }
    __syncthreads();
    for (int s = tid; s < MS_SLOTS; s += 256) {
        const uint32_t key = s_key[s];
        if (key == 0u) continue;
        const uint32_t k = key - first - 1u;
        if (s_word[F_COUNT][s] == sizes[k])                         // the whole component lies in this box
            record_store(&table[k], s_word[F_COUNT][s], s_word[F_MIN_X][s], s_word[F_MIN_Y][s], s_word[F_MIN_Z][s], s_word[F_MAX_X][s],
                         s_word[F_MAX_Y][s], s_word[F_MAX_Z][s], s_word[F_VMIN][s], s_word[F_VMAX][s], s_word[F_SUM_X][s], s_word[F_SUM_Y][s],
                         s_word[F_SUM_Z][s], s_word[F_VSUM][s], s_vsq[s], s_word[F_FACES][s]);
        else
            record_add(&table[k], s_word[F_COUNT][s], s_word[F_MIN_X][s], s_word[F_MIN_Y][s], s_word[F_MIN_Z][s], s_word[F_MAX_X][s],
                       s_word[F_MAX_Y][s], s_word[F_MAX_Z][s], s_word[F_VMIN][s], s_word[F_VMAX][s], s_word[F_SUM_X][s], s_word[F_SUM_Y][s],
                       s_word[F_SUM_Z][s], s_word[F_VSUM][s], s_vsq[s], s_word[F_FACES][s]);
    }
}

// ---------------------------------------------------------------------------------------------
// the set emitter: k_select_set<T>
// ---------------------------------------------------------------------------------------------
// k_select's form (vpt_volume_field.hip) with the interval test replaced by bit `rank` of a bitset of listed + 1 bits: every rank is at
// most `listed`, so the word read is one of the listed / 32 + 1 the host uploads.
template <typename T>
__global__ __launch_bounds__(256) void k_select_set(const T *__restrict__ src, const uint32_t *__restrict__ ranks, const uint32_t *__restrict__ bits,
                                                   T *__restrict__ dst, size_t n, uint32_t fill) {
    typedef Four<T> F;
    const size_t quads = n / 4, stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t q = t0; q < quads; q += stride) {
        const typename F::in_t w = reinterpret_cast<const typename F::in_t *>(src)[q];
        const uint4 r = reinterpret_cast<const uint4 *>(ranks)[q];
        const uint32_t d[4] = { r.x, r.y, r.z, r.w };
        uint32_t v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = ((bits[d[i] >> 5] >> (d[i] & 31u)) & 1u) ? F::get(w, i) : fill;
        reinterpret_cast<typename F::in_t *>(dst)[q] = F::pack(v);
    }
    for (size_t i = quads * 4 + t0; i < n; i += stride) { const uint32_t d = ranks[i]; dst[i] = ((bits[d >> 5] >> (d & 31u)) & 1u) ? src[i] : (T)fill; }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
template <typename TV, int STRIDE>
static void launch_measure(const vpt_components *c, const void *values, int channel, uint32_t first, uint32_t n, const uint32_t *sizes,
                           vpt_component_measure *table) {
    const dim3 grid((unsigned)((c->nx + MS_BX - 1) / MS_BX), (unsigned)((c->ny + MS_BY - 1) / MS_BY), (unsigned)((c->nz + MS_BZ - 1) / MS_BZ));
    hipLaunchKernelGGL((k_measure<TV, STRIDE>), grid, dim3(256), 0, c->ctx->stream, (const uint32_t *)c->values.get(), (const TV *)values, channel,
                       c->nx, c->ny, c->nz, first, n, sizes, table);
}

static int measure(vpt_components *c, vpt_volume *values, int channel, uint64_t first, uint64_t n, struct vpt_component_measure *dst, double *ms) {
    if (!c || (!dst && n)) return fail(VPT_ERR_INVALID, "null argument");
    bool norm16 = c->norm16;
    int channels = 1;
    const void *texels = c->texels.get();
    if (values) {
        if (values->format != VPT_FORMAT_R8 && values->format != VPT_FORMAT_RG8 && values->format != VPT_FORMAT_R16 && values->format != VPT_FORMAT_RG16)
            return fail(VPT_ERR_UNSUPPORTED, "measure: values is an unsigned normalised volume (R8, RG8, R16, RG16; the window makes R8 / R16 of any scalar volume), not %s",
                        format_name(values->format));
        if (values->ctx != c->ctx) return fail(VPT_ERR_INVALID, "measure: the components and values belong to two contexts");
        if (values->nx != c->nx || values->ny != c->ny || values->nz != c->nz)
            return fail(VPT_ERR_INVALID, "measure: the components are %dx%dx%d and values is %dx%dx%d; vpt_volume_resample brings two grids together",
                        c->nx, c->ny, c->nz, values->nx, values->ny, values->nz);
        norm16 = values->norm16; channels = values->channels; texels = values->linear.get();
    }
    if (channel != 0 && channel != 1) return fail(VPT_ERR_INVALID, "measure: channel %d: 0 or 1 are taken", channel);
    if (channel == 1 && channels != 2)
        return fail(VPT_ERR_INVALID, "measure: channel 1 of values, which has one channel (%s)", format_name(values ? values->format : c->format));
    if (first > c->info.listed || n > c->info.listed - first)
        return fail(VPT_ERR_INVALID, "components %llu .. +%llu are not within the %llu listed", (unsigned long long)first, (unsigned long long)n, (unsigned long long)c->info.listed);
    if (n == 0) return VPT_OK;
    if ((c->ny + MS_BY - 1) / MS_BY > 65535 || (c->nz + MS_BZ - 1) / MS_BZ > 65535) return fail(VPT_ERR_UNSUPPORTED, "volume too large");
    vpt_context *ctx = c->ctx;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t first32 = (uint32_t)first, n32 = (uint32_t)n;       // listed <= 2^32 - 2
    DevBuf<vpt_component_measure> table;                                // freed when the call returns
    DevBuf<uint32_t> sizes;                                             // the voxel counts of the window's components, from the list
    HIP_TRY(table.alloc((size_t)n));
    HIP_TRY(sizes.alloc((size_t)n));
    std::vector<uint32_t> host_sizes((size_t)n);
    for (size_t k = 0; k < (size_t)n; k++) host_sizes[k] = c->list[(size_t)first + k].voxels;
    HIP_TRY(hipMemcpyAsync(sizes, host_sizes.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_measure_init, dim3(stream_grid((size_t)n)), dim3(256), 0, st, table.get(), n32);
    PhaseClock clock(st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && ms) e = clock.lap(ms);                       // what is in front of the pass is not its time
    if (e == hipSuccess) {
        if (norm16) { if (channels == 2) launch_measure<uint16_t, 2>(c, texels, channel, first32, n32, sizes.get(), table.get()); else launch_measure<uint16_t, 1>(c, texels, channel, first32, n32, sizes.get(), table.get()); }
        else { if (channels == 2) launch_measure<uint8_t, 2>(c, texels, channel, first32, n32, sizes.get(), table.get()); else launch_measure<uint8_t, 1>(c, texels, channel, first32, n32, sizes.get(), table.get()); }
        e = hipGetLastError();
    }
    if (e == hipSuccess && ms) e = clock.lap(ms);
    if (e == hipSuccess) e = hipMemcpyAsync(dst, table, (size_t)n * sizeof(vpt_component_measure), hipMemcpyDeviceToHost, st);
    const hipError_t drained = hipStreamSynchronize(st);                // `table`, `sizes` and `host_sizes` go out of scope behind their last use, whatever happened
    if (e == hipSuccess) e = drained;
    if (e != hipSuccess) return fail(VPT_ERR_HIP, "measure: %s", hipGetErrorString(e));
    return VPT_OK;
}

extern "C" int vpt_components_measure(vpt_components *c, vpt_volume *values, int channel, uint64_t first, uint64_t n, struct vpt_component_measure *dst) {
    return measure(c, values, channel, first, n, dst, nullptr);
}

extern "C" int vpt_components_measure_timed(vpt_components *c, vpt_volume *values, int channel, uint64_t first, uint64_t n,
                                            struct vpt_component_measure *dst, double *ms) {
    if (!ms) return fail(VPT_ERR_INVALID, "null argument");
    *ms = 0.0;
    return measure(c, values, channel, first, n, dst, ms);
}

extern "C" int vpt_components_keep_set(vpt_components *c, const uint64_t *ranks, uint64_t n, uint32_t fill, vpt_volume **out) {
    if (!c || !out || (!ranks && n)) return fail(VPT_ERR_INVALID, "null argument");
    const uint32_t M = c->norm16 ? 65535u : 255u;
    if (fill > M) return fail(VPT_ERR_INVALID, "fill %u: the largest code of %s is %u", fill, format_name(c->format), M);
    const uint64_t listed = c->info.listed;
    std::vector<uint32_t> bits((size_t)(listed / 32u + 1u), 0u);        // bit r: rank r is kept; bit 0 (background, dropped) stays clear
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t r = ranks[k];
        if (r == 0) return fail(VPT_ERR_INVALID, "rank 0 at position %llu of the set: ranks are 1-based", (unsigned long long)k);
        if (r <= listed) bits[(size_t)(r >> 5)] |= 1u << (r & 31u);     // ranks beyond the list select nothing
    }
    vpt_context *ctx = c->ctx;
    hipStream_t st = ctx->stream;
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<uint32_t> dbits;                                             // freed when the call returns
    HIP_TRY(dbits.alloc(bits.size()));
    HIP_TRY(hipMemcpyAsync(dbits, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    vpt_volume *d = nullptr;
    int rc = volume_create(ctx, c->nx, c->ny, c->nz, c->format, false, &d);      // every texel is written below
    if (rc == VPT_OK) {
        const size_t voxels = c->voxels();
        const dim3 grid(stream_grid(voxels / 4 + 1));
        if (c->norm16) hipLaunchKernelGGL(k_select_set<uint16_t>, grid, dim3(256), 0, st, (const uint16_t *)c->texels.get(), (const uint32_t *)c->values.get(), (const uint32_t *)dbits.get(), (uint16_t *)d->linear.get(), voxels, fill);
        else hipLaunchKernelGGL(k_select_set<uint8_t>, grid, dim3(256), 0, st, (const uint8_t *)c->texels.get(), (const uint32_t *)c->values.get(), (const uint32_t *)dbits.get(), d->linear.get(), voxels, fill);
        rc = volume_finish_derived(ctx, c->filter, d, out);
    }
    const hipError_t drained = hipStreamSynchronize(st);                // `bits` and `dbits` go out of scope behind their last use
    if (rc == VPT_OK && drained != hipSuccess) {
        vpt_volume_destroy(*out); *out = nullptr;
        return fail(VPT_ERR_HIP, "keep_set: %s", hipGetErrorString(drained));
    }
    return rc;
}
