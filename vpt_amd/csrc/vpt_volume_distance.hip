// vpt_volume_distance.hip — the exact squared Euclidean distance of every voxel to the nearest voxel of a value range of a volume (or of its
// complement) on the device (vpt_volume_distance and the vpt_distance_* family): one uint32 d2 per voxel, the two emitters (within, channel).
// C-ABI and the contract: include/vpt.h; kernel forms, compiler figures, the loop bounds and measurements: DESIGN.md "Distance transform".
//
// The transform is separable: g0 = 0 on the seeds and NONE elsewhere, then per axis, in the order x, y, z, out[i] = min over the finite
// g[j] of g[j] + (i - j)^2.  Everything is integer: positions are below 4096, so a d2 is at most 3 * 4095^2 < 2^26 and NONE = 2^32 - 1 never
// enters a sum.  No workgroup waits for another: launch boundaries order the phases.
#include "vpt_internal.h"
#include <chrono>
#include <memory>

#define EDT_NONE 0xFFFFFFFFu
#define EDT_MAX_AXIS 4096          // vpt_volume_create's limit: a row has at most 64 segments of 64 voxels, positions fit 16 bits

// ---------------------------------------------------------------------------------------------
// x: threshold and row pass, k_edt_x<T>
// ---------------------------------------------------------------------------------------------
// A wave owns a row.  First sweep: segment s = the voxels 64 s .. 64 s + 63; the wave ballots "is a seed" and lane s keeps segment s's
// ballot (a row has at most 64 segments), so the texels are read once.  Lane s then knows the first and the last seed of its segment, and
// a ballot of "segment s has a seed" tells every segment where the nearest seeded segment to its left and to its right is: an empty
// segment between two seeded ones is simply not in that ballot, the carry passes over it.  Second sweep: per segment the wave fetches the
// segment's ballot and the two carries from the lanes that hold them (wave-uniform lane indices), each lane finds the nearest set bit at or
// below and at or above itself with a masked clz / ctz, and stores dx^2 or NONE.  No LDS, no second read of anything.
// The same kernel counts the seeds: one 64-bit integer atomicAdd per wave, into one of EDT_COUNT_SLOTS words by the wave's number (the host
// adds them up): tens of thousands of adds to ONE word took longer than the rows themselves (DESIGN.md has the measurement).
#define EDT_COUNT_SLOTS 64
template <typename T>
__global__ __launch_bounds__(256) void k_edt_x(const T *__restrict__ src, uint32_t *__restrict__ g, int nx, size_t rows, uint32_t lo, uint32_t hi,
                                              uint32_t to_rest, unsigned long long *__restrict__ seeds) {
    const int lane = (int)threadIdx.x & 63;
    const int segments = (nx + 63) >> 6;                         // <= 64
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (size_t)gridDim.x * 4;
    unsigned long long counted = 0ull;                           // (wave-uniform)
    for (size_t row = wave; row < rows; row += waves) {
        const T *line = src + row * (size_t)nx;
        unsigned long long mine = 0ull;
        for (int s = 0; s < segments; s++) {
            const int x = (s << 6) + lane;
            bool seed = false;
            if (x < nx) { const uint32_t c = (uint32_t)line[x]; seed = ((c >= lo && c <= hi) ? 1u : 0u) != to_rest; }
            const unsigned long long b = __ballot(seed);
            if (lane == s) mine = b;
            counted += (unsigned long long)__popcll(b);
        }
        // of the segment this lane holds: the last and the first seed's position
        const int last = mine ? (lane << 6) + 63 - __clzll((long long)mine) : -1;
        const int first = mine ? (lane << 6) + __ffsll((long long)mine) - 1 : -1;
        const unsigned long long seeded = __ballot(mine != 0ull);
        uint32_t *out = g + row * (size_t)nx;
        for (int s = 0; s < segments; s++) {
            const unsigned long long b = ((unsigned long long)(uint32_t)__shfl((int)(mine >> 32), s) << 32) | (uint32_t)__shfl((int)(uint32_t)mine, s);
            const unsigned long long left = seeded & ((1ull << s) - 1ull), right = s == 63 ? 0ull : seeded & ~((2ull << s) - 1ull);
            const int carry_l = left ? __shfl(last, 63 - __clzll((long long)left)) : -1;          // the last seed in front of the segment
            const int carry_r = right ? __shfl(first, __ffsll((long long)right) - 1) : -1;        // the first seed behind it
            const int x = (s << 6) + lane;
            const unsigned long long at_or_below = b & ((2ull << lane) - 1ull);                   // (lane 63: 2 << 63 wraps to 0, the mask is all ones)
            const unsigned long long at_or_above = b & ~((1ull << lane) - 1ull);
            const int l = at_or_below ? (s << 6) + 63 - __clzll((long long)at_or_below) : carry_l;
            const int r = at_or_above ? (s << 6) + __ffsll((long long)at_or_above) - 1 : carry_r;
            uint32_t d = EDT_NONE;
            if (l >= 0) d = (uint32_t)((x - l) * (x - l));
            if (r >= 0) d = min(d, (uint32_t)((r - x) * (r - x)));
            if (x < nx) out[x] = d;
        }
    }
    if (lane == 0 && counted) atomicAdd(&seeds[wave % EDT_COUNT_SLOTS], counted);
}

// ---------------------------------------------------------------------------------------------
// y, then z: the lower envelope of parabolas, k_edt_line<AXIS>
// ---------------------------------------------------------------------------------------------
// Meijster's scans 3 and 4, one lane per line, the lanes along x: lane x owns the line (x, ., z) in the y pass and (x, y, .) in the z pass, so
// what a wave loads and stores at step j are consecutive dwords.  `in` is read only, `out` is another buffer: the envelope needs g at the
// positions on its stack until the backward scan has passed the stack entry, and that scan has by then overwritten positions above it.
// The stack lives in `stack`, laid out like the volume with the stack index in the place of the line's coordinate, so it is coalesced
// wherever the lanes' stacks are equally deep: one dword per entry, the parabola's position s in the low and its break point t (the first
// position at which it is the lowest) in the high 16 bits.  The top entry and g at its position are kept in registers.
// A position with g = NONE is never pushed, so every quantity is a sum of squares of numbers below 4096 and of finite g <= 2 * 4095^2: all
// below 2^31, plain 32-bit integer arithmetic is exact.
// Bounds.  Forward scan: each position is pushed at most once and popped at most once, so the pop loop runs at most `m` times per line in
// total and at most q + 1 <= m times per position; backward scan: one step per position.
__device__ __forceinline__ int edt_f(int x, int i, int gi) { return (x - i) * (x - i) + gi; }
// 1 + floor((u^2 - i^2 + gu - gi) / (2 (u - i))) for i < u: the first position at which u's parabola is strictly below i's.  The numerator
// may be negative (|.| < 2^26): C's division truncates, so the quotient is lowered by one when it was rounded up
__device__ __forceinline__ int edt_break(int i, int gi, int u, int gu) {
    const int num = u * u - i * i + gu - gi, den = 2 * (u - i);
    int q = num / den;
    if (num < 0 && q * den != num) q--;
    return q + 1;
}
template <int AXIS>       // 1: y, 2: z
__global__ __launch_bounds__(64) void k_edt_line(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t *__restrict__ stack, int nx, int ny, int nz) {
    const int m = AXIS == 1 ? ny : nz;
    const size_t step = AXIS == 1 ? (size_t)nx : (size_t)nx * (size_t)ny;
    const size_t lines = AXIS == 1 ? (size_t)nx * (size_t)nz : (size_t)nx * (size_t)ny;
    for (size_t line = (size_t)blockIdx.x * 64 + threadIdx.x; line < lines; line += (size_t)gridDim.x * 64) {
        // the line's voxel 0: y pass (x, 0, z) with line = z nx + x; z pass (x, y, 0) with line = y nx + x
        const size_t base = AXIS == 1 ? (line / (size_t)nx) * (size_t)nx * (size_t)ny + line % (size_t)nx : line;
        const uint32_t *gl = in + base;
        uint32_t *sl = stack + base;
        int q = -1, s_q = 0, t_q = 0, g_q = 0;                  // the stack's depth - 1 and its top entry
        uint32_t next = gl[0];
        for (int u = 0; u < m; u++) {
            const uint32_t gu = next;
            if (u + 1 < m) next = gl[(size_t)(u + 1) * step];
            if (gu == EDT_NONE) continue;
            while (q >= 0 && edt_f(t_q, s_q, g_q) > edt_f(t_q, u, (int)gu)) {       // u's parabola is lower where the top's begins: the top is hidden
                q--;
                if (q >= 0) {
                    const uint32_t e = sl[(size_t)q * step];
                    s_q = (int)(e & 0xFFFFu); t_q = (int)(e >> 16); g_q = (int)gl[(size_t)s_q * step];
                }
            }
            int w = 0;
            if (q >= 0) {
                w = edt_break(s_q, g_q, u, (int)gu);
                if (w >= m) continue;                            // u is never the lowest within the line
            }
            q++;
            s_q = u; t_q = w; g_q = (int)gu;
            sl[(size_t)q * step] = (uint32_t)u | ((uint32_t)w << 16);
        }
        uint32_t *ol = out + base;
        for (int u = m - 1; u >= 0; u--) {
            ol[(size_t)u * step] = q < 0 ? EDT_NONE : (uint32_t)edt_f(u, s_q, g_q);
            if (q >= 0 && u == t_q) {
                q--;
                if (q >= 0) {
                    const uint32_t e = sl[(size_t)q * step];
                    s_q = (int)(e & 0xFFFFu); t_q = (int)(e >> 16); g_q = (int)gl[(size_t)s_q * step];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the largest finite d2; emitters k_within<T>, k_channel<T>; read-back of a box of d2
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_largest(const uint32_t *__restrict__ d2, size_t n, uint32_t *__restrict__ largest) {
    uint32_t m = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t d = d2[i];
        if (d != EDT_NONE) m = max(m, d);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
    if (((int)threadIdx.x & 63) == 0 && m) atomicMax(largest, m);
}

// floor(sqrt(p)) for p < 2^53: the double square root is within one of it, the two steps make it exact
__device__ __forceinline__ uint32_t isqrt64(unsigned long long p) {
    unsigned long long r = (unsigned long long)sqrt((double)p);
    if (r * r > p) r--;
    if ((r + 1ull) * (r + 1ull) <= p) r++;
    return (uint32_t)r;
}

// Plain gathers over the linear storage, four voxels a thread (as k_keep / k_label of the components unit): the texels as one dword (uint8)
// or qword (uint16), d2 as one uint4, the result as one vector store; the last n % 4 voxels one by one.
template <typename T> struct Four;
template <> struct Four<uint8_t> {
    typedef uint32_t in_t; typedef uint2 pair_t;
    static __device__ __forceinline__ uint32_t get(in_t w, int i) { return (w >> (8 * i)) & 255u; }
    static __device__ __forceinline__ in_t pack(const uint32_t *v) { return v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24); }
    static __device__ __forceinline__ pair_t pack2(const uint32_t *v, const uint32_t *g) {
        return make_uint2(v[0] | (g[0] << 8) | (v[1] << 16) | (g[1] << 24), v[2] | (g[2] << 8) | (v[3] << 16) | (g[3] << 24));
    }
};
template <> struct Four<uint16_t> {
    typedef uint2 in_t; typedef uint4 pair_t;
    static __device__ __forceinline__ uint32_t get(in_t w, int i) { return ((i < 2 ? w.x : w.y) >> (16 * (i & 1))) & 65535u; }
    static __device__ __forceinline__ in_t pack(const uint32_t *v) { return make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16)); }
    static __device__ __forceinline__ pair_t pack2(const uint32_t *v, const uint32_t *g) {
        return make_uint4(v[0] | (g[0] << 16), v[1] | (g[1] << 16), v[2] | (g[2] << 16), v[3] | (g[3] << 16));
    }
};
template <typename T>
__global__ __launch_bounds__(256) void k_within(const T *__restrict__ src, const uint32_t *__restrict__ d2, T *__restrict__ dst, size_t n,
                                               uint32_t r2_lo, uint32_t r2_hi, uint32_t fill) {
    typedef Four<T> F;
    const size_t quads = n / 4, stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t q = t0; q < quads; q += stride) {
        const typename F::in_t w = reinterpret_cast<const typename F::in_t *>(src)[q];
        const uint4 r = reinterpret_cast<const uint4 *>(d2)[q];
        const uint32_t d[4] = { r.x, r.y, r.z, r.w };
        uint32_t v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = (d[i] >= r2_lo && d[i] <= r2_hi) ? F::get(w, i) : fill;
        reinterpret_cast<typename F::in_t *>(dst)[q] = F::pack(v);
    }
    for (size_t i = quads * 4 + t0; i < n; i += stride) { const uint32_t d = d2[i]; dst[i] = (d >= r2_lo && d <= r2_hi) ? src[i] : (T)fill; }
}
template <typename T>
__global__ __launch_bounds__(256) void k_channel(const T *__restrict__ src, const uint32_t *__restrict__ d2, T *__restrict__ dst, size_t n, uint32_t steps2) {
    typedef Four<T> F;
    constexpr uint32_t M = (1u << (8 * sizeof(T))) - 1u;
    const size_t quads = n / 4, stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t q = t0; q < quads; q += stride) {
        const typename F::in_t w = reinterpret_cast<const typename F::in_t *>(src)[q];
        const uint4 r = reinterpret_cast<const uint4 *>(d2)[q];
        const uint32_t d[4] = { r.x, r.y, r.z, r.w };
        uint32_t v[4], g[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { v[i] = F::get(w, i); g[i] = min(isqrt64((unsigned long long)steps2 * d[i]), M); }
        reinterpret_cast<typename F::pair_t *>(dst)[q] = F::pack2(v, g);
    }
    for (size_t i = quads * 4 + t0; i < n; i += stride) { dst[2 * i] = src[i]; dst[2 * i + 1] = (T)min(isqrt64((unsigned long long)steps2 * d2[i]), M); }
}
__global__ __launch_bounds__(256) void k_read_squared(const uint32_t *__restrict__ d2, int nx, int ny, uint32_t *__restrict__ blk, int x0, int y0, int z0,
                                                     int bw, int bh, size_t texels) {
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < texels; t += (size_t)gridDim.x * 256) {
        const int x = (int)(t % (size_t)bw); const size_t r = t / (size_t)bw; const int y = (int)(r % (size_t)bh), z = (int)(r / (size_t)bh);
        blk[t] = d2[((size_t)(z0 + z) * (size_t)ny + (size_t)(y0 + y)) * (size_t)nx + (size_t)(x0 + x)];
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
struct vpt_distance {
    vpt_context *ctx = nullptr;
    int nx = 0, ny = 0, nz = 0, format = 0, filter = VPT_FILTER_LINEAR;
    bool norm16 = false;
    DevBuf<uint8_t> texels;                 // the source's linear texels at the time of the call
    DevBuf<uint32_t> d2;                    // one squared distance per voxel
    struct vpt_distance_info info = {};
    double ms[VPT_DISTANCE_PHASES] = {};
    size_t voxels() const { return (size_t)nx * (size_t)ny * (size_t)nz; }
};

// grid of a grid-stride kernel over `items`, `per` of them a workgroup
static unsigned stream_grid(size_t items, size_t per = 256, size_t most = 8192) { return (unsigned)std::max<size_t>(1, std::min<size_t>((items + per - 1) / per, most)); }

// wall time of a phase, the stream drained at its end
static hipError_t lap(hipStream_t st, std::chrono::steady_clock::time_point *t0, double *ms) {
    const hipError_t e = hipStreamSynchronize(st);
    const auto t1 = std::chrono::steady_clock::now();
    *ms = std::chrono::duration<double, std::milli>(t1 - *t0).count();
    *t0 = t1;
    return e;
}

// the body of vpt_volume_distance behind the argument checks; `d` is freed by the caller on failure
static int distance_build(vpt_distance *d, uint32_t lo, uint32_t hi, int seeds) {
    const size_t n = d->voxels();
    hipStream_t st = d->ctx->stream;
    DevBuf<uint32_t> other, stack, largest;             // the y pass's output, the line passes' stacks: freed when the call returns
    DevBuf<unsigned long long> count;
    HIP_TRY(other.alloc(n));
    HIP_TRY(stack.alloc(n));
    HIP_TRY(largest.alloc(1));
    HIP_TRY(count.alloc(EDT_COUNT_SLOTS));
    HIP_TRY(hipMemsetAsync(largest, 0, sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(count, 0, EDT_COUNT_SLOTS * sizeof(unsigned long long), st));
    HIP_TRY(hipStreamSynchronize(st));
    auto t0 = std::chrono::steady_clock::now();
    // ---- x: the seeds and the row pass
    const size_t rows = (size_t)d->ny * (size_t)d->nz;
    const uint32_t to_rest = seeds == VPT_DISTANCE_TO_REST ? 1u : 0u;
    if (d->norm16) hipLaunchKernelGGL(k_edt_x<uint16_t>, dim3(stream_grid(rows, 4, 2048)), dim3(256), 0, st, (const uint16_t *)d->texels.get(), d->d2.get(), d->nx, rows, lo, hi, to_rest, count.get());
    else hipLaunchKernelGGL(k_edt_x<uint8_t>, dim3(stream_grid(rows, 4, 2048)), dim3(256), 0, st, (const uint8_t *)d->texels.get(), d->d2.get(), d->nx, rows, lo, hi, to_rest, count.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(lap(st, &t0, &d->ms[0]));
    // ---- y: d2 -> other
    hipLaunchKernelGGL(k_edt_line<1>, dim3(stream_grid((size_t)d->nx * (size_t)d->nz, 64)), dim3(64), 0, st, (const uint32_t *)d->d2.get(), other.get(), stack.get(), d->nx, d->ny, d->nz);
    HIP_TRY(hipGetLastError());
    HIP_TRY(lap(st, &t0, &d->ms[1]));
    // ---- z: other -> d2
    hipLaunchKernelGGL(k_edt_line<2>, dim3(stream_grid((size_t)d->nx * (size_t)d->ny, 64)), dim3(64), 0, st, (const uint32_t *)other.get(), d->d2.get(), stack.get(), d->nx, d->ny, d->nz);
    HIP_TRY(hipGetLastError());
    HIP_TRY(lap(st, &t0, &d->ms[2]));
    // ---- info
    unsigned long long host_count[EDT_COUNT_SLOTS] = {}; uint32_t host_largest = 0;
    hipLaunchKernelGGL(k_largest, dim3(stream_grid(n)), dim3(256), 0, st, (const uint32_t *)d->d2.get(), n, largest.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_count, count, sizeof(host_count), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&host_largest, largest, sizeof(host_largest), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));                  // `other`, `stack` and the two words go out of scope behind their last use
    d->info.seeds = 0; d->info.largest = host_largest;
    for (int k = 0; k < EDT_COUNT_SLOTS; k++) d->info.seeds += host_count[k];
    return VPT_OK;
}

extern "C" int vpt_volume_distance(vpt_volume *src, uint32_t lo, uint32_t hi, int seeds, vpt_distance **out) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (src->format != VPT_FORMAT_R8 && src->format != VPT_FORMAT_R16)
        return fail(VPT_ERR_UNSUPPORTED, "distances are taken in one-channel unsigned normalised volumes (R8, R16; the window makes one of any scalar volume), not in %s",
                    format_name(src->format));
    const uint32_t M = src->norm16 ? 65535u : 255u;
    if (lo > hi) return fail(VPT_ERR_INVALID, "distance range [%u, %u]: lo exceeds hi", lo, hi);
    if (hi > M) return fail(VPT_ERR_INVALID, "distance range [%u, %u]: the largest code of %s is %u", lo, hi, format_name(src->format), M);
    if (seeds != VPT_DISTANCE_TO_RANGE && seeds != VPT_DISTANCE_TO_REST)
        return fail(VPT_ERR_INVALID, "seeds %d: VPT_DISTANCE_TO_RANGE (0) or VPT_DISTANCE_TO_REST (1) are taken", seeds);
    if (src->nx > EDT_MAX_AXIS || src->ny > EDT_MAX_AXIS || src->nz > EDT_MAX_AXIS) return fail(VPT_ERR_UNSUPPORTED, "volume too large");
    vpt_context *ctx = src->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<vpt_distance> d(new vpt_distance());
    d->ctx = ctx; d->nx = src->nx; d->ny = src->ny; d->nz = src->nz; d->format = src->format; d->filter = src->filter; d->norm16 = src->norm16;
    const size_t n = d->voxels(), bytes = n * (size_t)src->vox_bytes;
    HIP_TRY(d->texels.alloc(bytes));
    HIP_TRY(d->d2.alloc(n));
    HIP_TRY(hipMemcpyAsync(d->texels, src->linear, bytes, hipMemcpyDeviceToDevice, ctx->stream));     // behind any upload into src
    const int rc = distance_build(d.get(), lo, hi, seeds);
    if (rc != VPT_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }      // the buffers are freed on return: nothing may still use them
    *out = d.release();
    return VPT_OK;
}

extern "C" int vpt_distance_info(vpt_distance *d, struct vpt_distance_info *info) {
    if (!d || !info) return fail(VPT_ERR_INVALID, "null argument");
    *info = d->info;
    return VPT_OK;
}

extern "C" int vpt_distance_squared(vpt_distance *c, int x, int y, int z, int w, int h, int d, uint32_t *host_dst, size_t nbytes) {
    if (!c || !host_dst) return fail(VPT_ERR_INVALID, "null argument");
    if (w < 1 || h < 1 || d < 1 || x < 0 || y < 0 || z < 0 || x + w > c->nx || y + h > c->ny || z + d > c->nz)
        return fail(VPT_ERR_INVALID, "block (%d,%d,%d)+(%d,%d,%d) outside volume %dx%dx%d", x, y, z, w, h, d, c->nx, c->ny, c->nz);
    const size_t texels = (size_t)w * h * d, need = texels * sizeof(uint32_t);
    if (nbytes < need) return fail(VPT_ERR_INVALID, "block buffer too short: %zu < %zu", nbytes, need);
    hipStream_t st = c->ctx->stream;
    HIP_TRY(hipSetDevice(c->ctx->device));
    if (x == 0 && y == 0 && w == c->nx && h == c->ny) {        // a run of whole z-slices is contiguous
        HIP_TRY(hipMemcpyAsync(host_dst, c->d2 + (size_t)z * c->nx * c->ny, need, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return VPT_OK;
    }
    DevBuf<uint32_t> block;
    HIP_TRY(block.alloc(texels));
    hipLaunchKernelGGL(k_read_squared, dim3(stream_grid(texels)), dim3(256), 0, st, (const uint32_t *)c->d2.get(), c->nx, c->ny, block.get(), x, y, z, w, h, texels);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_dst, block, need, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return VPT_OK;
}

// what volume_finish_derived reads of a derived volume's source: the context and the filter
static void source_stand_in(const vpt_distance *d, vpt_volume *v) { v->ctx = d->ctx; v->filter = d->filter; }

extern "C" int vpt_distance_within(vpt_distance *c, uint32_t r2_lo, uint32_t r2_hi, uint32_t fill, vpt_volume **out) {
    if (!c || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (r2_lo > r2_hi) return fail(VPT_ERR_INVALID, "squared distances %u .. %u: from exceeds to", r2_lo, r2_hi);
    const uint32_t M = c->norm16 ? 65535u : 255u;
    if (fill > M) return fail(VPT_ERR_INVALID, "fill %u: the largest code of %s is %u", fill, format_name(c->format), M);
    HIP_TRY(hipSetDevice(c->ctx->device));
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(c->ctx, c->nx, c->ny, c->nz, c->format, false, &d));      // every texel is written below
    const size_t n = c->voxels();
    const dim3 grid(stream_grid(n / 4 + 1));
    if (c->norm16) hipLaunchKernelGGL(k_within<uint16_t>, grid, dim3(256), 0, c->ctx->stream, (const uint16_t *)c->texels.get(), (const uint32_t *)c->d2.get(), (uint16_t *)d->linear.get(), n, r2_lo, r2_hi, fill);
    else hipLaunchKernelGGL(k_within<uint8_t>, grid, dim3(256), 0, c->ctx->stream, (const uint8_t *)c->texels.get(), (const uint32_t *)c->d2.get(), d->linear.get(), n, r2_lo, r2_hi, fill);
    vpt_volume source;
    source_stand_in(c, &source);
    return volume_finish_derived(&source, d, out);
}

extern "C" int vpt_distance_channel(vpt_distance *c, int steps, vpt_volume **out) {
    if (!c || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (steps < 1 || steps > 256) return fail(VPT_ERR_INVALID, "steps %d: 1 .. 256 rows of the transfer function per voxel of distance are taken", steps);
    HIP_TRY(hipSetDevice(c->ctx->device));
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(c->ctx, c->nx, c->ny, c->nz, c->norm16 ? VPT_FORMAT_RG16 : VPT_FORMAT_RG8, false, &d));      // every texel is written below
    const size_t n = c->voxels();
    const dim3 grid(stream_grid(n / 4 + 1));
    const uint32_t steps2 = (uint32_t)(steps * steps);
    if (c->norm16) hipLaunchKernelGGL(k_channel<uint16_t>, grid, dim3(256), 0, c->ctx->stream, (const uint16_t *)c->texels.get(), (const uint32_t *)c->d2.get(), (uint16_t *)d->linear.get(), n, steps2);
    else hipLaunchKernelGGL(k_channel<uint8_t>, grid, dim3(256), 0, c->ctx->stream, (const uint8_t *)c->texels.get(), (const uint32_t *)c->d2.get(), d->linear.get(), n, steps2);
    vpt_volume source;
    source_stand_in(c, &source);
    return volume_finish_derived(&source, d, out);
}

extern "C" int vpt_distance_profile(vpt_distance *d, double *ms) {
    if (!d || !ms) return fail(VPT_ERR_INVALID, "null argument");
    memcpy(ms, d->ms, sizeof(d->ms));
    return VPT_OK;
}

extern "C" int vpt_distance_destroy(vpt_distance *d) {
    if (!d) return fail(VPT_ERR_INVALID, "null argument");
    (void)hipSetDevice(d->ctx->device);
    (void)hipStreamSynchronize(d->ctx->stream);      // an emitter may still read the buffers
    delete d;
    return VPT_OK;
}
