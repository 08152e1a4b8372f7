// vpt_volume_distance.hip — the exact squared Euclidean distance of every voxel to the nearest voxel of a value range of a volume (or of its
// complement) on the device (vpt_volume_distance and the vpt_distance_* family): one uint32 d2 per voxel, the two emitters (within, channel).
// C-ABI and the contract: include/vpt.h; kernel forms, compiler figures, the loop bounds and measurements: DESIGN.md "Distance transform".
//
// The transform is separable: g0 = 0 on the seeds and NONE elsewhere, then per axis, in the order x, y, z, out[i] = min over the finite
// g[j] of g[j] + (i - j)^2.  Everything is integer: positions are below 4096, so a d2 is at most 3 * 4095^2 < 2^26 and NONE = 2^32 - 1 never
// enters a sum.  No workgroup waits for another: launch boundaries order the phases.
#include "vpt_volume_distance.h"

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
// the largest finite d2; the distance channel
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

// the distance channel's second value, before k_pair clamps it to the largest code: the distance in rows, `steps` a voxel (vpt_volume_field.h)
struct DistanceChannel {
    uint32_t steps2;
    __device__ __forceinline__ uint32_t operator()(uint32_t d2) const { return isqrt64((unsigned long long)steps2 * d2); }
};

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
int distance_largest(hipStream_t st, const uint32_t *d2, size_t n, uint32_t *largest) {
    hipLaunchKernelGGL(k_largest, dim3(stream_grid(n)), dim3(256), 0, st, d2, n, largest);
    HIP_TRY(hipGetLastError());
    return VPT_OK;
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
    PhaseClock clock(st);
    // ---- x: the seeds and the row pass
    const size_t rows = (size_t)d->ny * (size_t)d->nz;
    const uint32_t to_rest = seeds == VPT_DISTANCE_TO_REST ? 1u : 0u;
    if (d->norm16) hipLaunchKernelGGL(k_edt_x<uint16_t>, dim3(stream_grid(rows, 4, 2048)), dim3(256), 0, st, (const uint16_t *)d->texels.get(), d->values.get(), d->nx, rows, lo, hi, to_rest, count.get());
    else hipLaunchKernelGGL(k_edt_x<uint8_t>, dim3(stream_grid(rows, 4, 2048)), dim3(256), 0, st, (const uint8_t *)d->texels.get(), d->values.get(), d->nx, rows, lo, hi, to_rest, count.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.lap(&d->ms[0]));
    // ---- y: d2 -> other
    hipLaunchKernelGGL(k_edt_line<1>, dim3(stream_grid((size_t)d->nx * (size_t)d->nz, 64)), dim3(64), 0, st, (const uint32_t *)d->values.get(), other.get(), stack.get(), d->nx, d->ny, d->nz);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.lap(&d->ms[1]));
    // ---- z: other -> d2
    hipLaunchKernelGGL(k_edt_line<2>, dim3(stream_grid((size_t)d->nx * (size_t)d->ny, 64)), dim3(64), 0, st, (const uint32_t *)other.get(), d->values.get(), stack.get(), d->nx, d->ny, d->nz);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.lap(&d->ms[2]));
    // ---- info
    unsigned long long host_count[EDT_COUNT_SLOTS] = {}; uint32_t host_largest = 0;
    VPT_TRY(distance_largest(st, d->values.get(), n, largest.get()));
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
    VPT_TRY(field_capture(d.get(), src));
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
    return field_read(c, x, y, z, w, h, d, host_dst, nbytes);
}

extern "C" int vpt_distance_within(vpt_distance *c, uint32_t r2_lo, uint32_t r2_hi, uint32_t fill, vpt_volume **out) {
    if (!c || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (r2_lo > r2_hi) return fail(VPT_ERR_INVALID, "squared distances %u .. %u: from exceeds to", r2_lo, r2_hi);
    return field_select(c, r2_lo, r2_hi, fill, out);
}

extern "C" int vpt_distance_channel(vpt_distance *c, int steps, vpt_volume **out) {
    if (!c || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (steps < 1 || steps > 256) return fail(VPT_ERR_INVALID, "steps %d: 1 .. 256 rows of the transfer function per voxel of distance are taken", steps);
    return field_pair(c, DistanceChannel{ (uint32_t)(steps * steps) }, out);
}

extern "C" int vpt_distance_profile(vpt_distance *d, double *ms) {
    if (!d || !ms) return fail(VPT_ERR_INVALID, "null argument");
    memcpy(ms, d->ms, sizeof(d->ms));
    return VPT_OK;
}

extern "C" int vpt_distance_destroy(vpt_distance *d) { return field_destroy(d); }
