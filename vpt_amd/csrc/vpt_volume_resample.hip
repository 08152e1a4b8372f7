// vpt_volume_resample.hip — a volume resampled to any grid size on the device (vpt_volume_resample): NEAREST copies the texel whose cell
// holds the result texel's centre, FILTERED interpolates linearly along an axis that grows and averages areas along one that shrinks, in
// integers with one rounding.  C-ABI and the contract: include/vpt.h; kernel forms, compiler figures, the loop bounds and measurements:
// DESIGN.md "Resampling".
//
// FILTERED is separable and its sum is exact, so it is taken axis by axis with no rounding in between: the row pass k_resample_x leaves one
// uint32 partial sum per (result x, source y, source z) and channel, the plane pass k_resample_yz sums those over the y and z taps in 64-bit
// integers and divides once.  No workgroup waits for another: the launch boundary orders the passes.  No float arithmetic, no atomics.
#include "vpt_internal.h"

#define RS_MAX_AXIS 4096           // vpt_volume_create's limit: every product of two indices below fits 32 bits (8191 * 4096 < 2^25)
#define RS_LDS_DWORDS 4096         // 16 KiB: the longest source row, 4096 texels x 2 channels x 2 bytes

// ---------------------------------------------------------------------------------------------
// the taps of result index X along an axis of n source and N result texels
// ---------------------------------------------------------------------------------------------
// N >= n: linear interpolation at u = (X + 0.5) n / N - 0.5, clamped: num = (2 X + 1) n - N over D = 2 N; one tap of weight D at either
// end, else (i, D - f), (i + 1, f) with i = num div D, f = num mod D (f == 0: the second tap has no weight and is not read).  S = 2 N.
// N < n: the overlap of source cell j with result cell X in units where a source texel is N and a result texel n long,
// w_j = min((X + 1) n, (j + 1) N) - max(X n, j N) > 0 for j = (X n) div N .. ((X + 1) n - 1) div N.  S = n.
struct AxisTaps {
    int j0, j1;                    // the taps j0 .. j1, all inside 0 .. n - 1
    uint32_t w0, w1;               // a growing axis: the weights of j0 and of j1
    int n, N, X;
    __device__ __forceinline__ uint32_t weight(int j) const {
        if (N >= n) return j == j0 ? w0 : w1;
        return (uint32_t)(min((X + 1) * n, (j + 1) * N) - max(X * n, j * N));
    }
};
__device__ __forceinline__ AxisTaps axis_taps(int n, int N, int X) {
    AxisTaps t;
    t.n = n; t.N = N; t.X = X; t.w0 = 0u; t.w1 = 0u;
    if (N >= n) {
        const int D = 2 * N, num = (2 * X + 1) * n - N;
        if (num <= 0) { t.j0 = t.j1 = 0; t.w0 = (uint32_t)D; }
        else if (num >= (n - 1) * D) { t.j0 = t.j1 = n - 1; t.w0 = (uint32_t)D; }
        else {
            const int i = num / D, f = num - i * D;              // i <= n - 2
            t.j0 = i; t.j1 = f ? i + 1 : i; t.w0 = (uint32_t)(D - f); t.w1 = (uint32_t)f;
        }
    } else {
        t.j0 = (X * n) / N; t.j1 = ((X + 1) * n - 1) / N;        // j1 <= n - 1 since X + 1 <= N
    }
    return t;
}

// ---------------------------------------------------------------------------------------------
// row pass: k_resample_x<T, CH>
// ---------------------------------------------------------------------------------------------
// A workgroup stages `rows_per_group` consecutive source rows in LDS: they are one contiguous piece of the linear storage, copied as whole
// dwords from the dword that holds its first byte (the piece need not begin on a dword; the bytes in front of it belong to the row before
// and are inside the storage) up to the last dword that lies wholly inside the storage, and byte by byte behind that (the last piece of a
// volume whose size is no multiple of four).  Then the lanes run along the result's x over all staged rows, gather their taps from LDS and
// store one uint32 partial sum per result texel and channel, consecutive lanes consecutive dwords.  A partial is at most 65535 * 8192 < 2^29.
// Bounds: the copy loops run over the piece (<= 16 KiB + 3 bytes, the size of `tile`), the item loop over rows_per_group * N results, the
// tap loop over j0 .. j1 (at most n taps).
template <typename T, int CH>
__global__ __launch_bounds__(256) void k_resample_x(const T *__restrict__ src, uint32_t *__restrict__ part, int n, int N, uint32_t rows,
                                                   uint32_t rows_per_group, size_t total_bytes) {
    __shared__ uint32_t tile[RS_LDS_DWORDS + 1];
    const uint32_t r0 = blockIdx.x * rows_per_group;
    if (r0 >= rows) return;                                      // (the whole workgroup)
    const uint32_t nrows = min(rows_per_group, rows - r0);
    const size_t row_bytes = (size_t)n * CH * sizeof(T);
    const size_t b0 = (size_t)r0 * row_bytes, b1 = b0 + (size_t)nrows * row_bytes;      // the piece: bytes b0 .. b1 - 1 of the storage
    const size_t a0 = b0 & ~(size_t)3;
    const size_t d0 = a0 / 4, d1 = min((b1 + 3) / 4, total_bytes / 4);                  // d0 <= d1: a0 <= total_bytes, both whole dwords
    const uint32_t *src32 = reinterpret_cast<const uint32_t *>(src);
    for (size_t k = d0 + threadIdx.x; k < d1; k += 256) tile[k - d0] = src32[k];
    uint8_t *tile8 = reinterpret_cast<uint8_t *>(tile);
    const uint8_t *src8 = reinterpret_cast<const uint8_t *>(src);
    for (size_t p = max(d1 * 4, b0) + threadIdx.x; p < b1; p += 256) tile8[p - a0] = src8[p];      // at most 3 bytes
    __syncthreads();
    const T *staged = reinterpret_cast<const T *>(tile8 + (b0 - a0));                   // (uint16: row_bytes is even, so is b0 - a0)
    const uint32_t items = nrows * (uint32_t)N;                  // <= 16384 (the host's choice of rows_per_group) or N for one row
    for (uint32_t i = threadIdx.x; i < items; i += 256) {
        const uint32_t r = i / (uint32_t)N, X = i - r * (uint32_t)N;
        const AxisTaps a = axis_taps(n, N, (int)X);
        const T *row = staged + (size_t)r * (size_t)n * CH;
        uint32_t s[CH] = {};
        for (int j = a.j0; j <= a.j1; j++) {
            const uint32_t w = a.weight(j);
#pragma unroll
            for (int c = 0; c < CH; c++) s[c] += w * (uint32_t)row[j * CH + c];
        }
        const size_t o = (size_t)(r0 + r) * (size_t)N + X;
        if constexpr (CH == 2) reinterpret_cast<uint2 *>(part)[o] = make_uint2(s[0], s[1]);
        else part[o] = s[0];
    }
}

// ---------------------------------------------------------------------------------------------
// plane pass: k_resample_yz<T>
// ---------------------------------------------------------------------------------------------
// The partial sums are [nz][ny][cols] dwords, cols = result width x channels: both channels of a texel have the same weights, so the pass
// does not know channels.  Lanes run along the columns (what a wave loads at every tap and what it stores are consecutive dwords and
// texels), the four waves of a workgroup take four result rows; Y and Z, so every tap and weight, are wave-uniform.  Per z tap the y taps
// are summed (< 2^29 * 8192 = 2^42), then weighted by w_z (< 2^55); out = (2 sum + S) div (2 S), S = S_x S_y S_z <= 2^39.
// The division, x div d with x = 2 sum + S < 2^57 and the wave-uniform d = 2 S >= 16: the host gives m = floor(2^64 / d), the lane
// takes q = floor(x m / 2^64) (__umul64hi).  x / d - x m / 2^64 = x (2^64 / d - m) / 2^64 lies in [0, x / 2^64) and x < 2^64, so
// x m / 2^64 is in (x / d - 1, x / d] and q is floor(x / d) or one below it: one compare of the remainder x - q d with d makes it exact
// for every numerator (the compiler's 64-bit division was a quarter of the pass where an axis grows: DESIGN.md).
// Bounds: the tap loops run over j0 .. j1 of their axis (at most nz and ny steps); no other loop.
template <typename T>
__global__ __launch_bounds__(256) void k_resample_yz(const uint32_t *__restrict__ part, T *__restrict__ dst, int cols, int ny, int NY, int nz, int NZ,
                                                    unsigned long long S, unsigned long long reciprocal) {
    const int q = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63);
    const int Y = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6), Z = (int)blockIdx.z;
    if (q >= cols || Y >= NY) return;
    const AxisTaps ty = axis_taps(ny, NY, Y), tz = axis_taps(nz, NZ, Z);
    unsigned long long sum = 0ull;
    for (int z = tz.j0; z <= tz.j1; z++) {
        const uint32_t *plane = part + (size_t)z * (size_t)ny * (size_t)cols + (size_t)q;
        unsigned long long line = 0ull;
        for (int y = ty.j0; y <= ty.j1; y++) line += (unsigned long long)ty.weight(y) * (unsigned long long)plane[(size_t)y * (size_t)cols];
        sum += (unsigned long long)tz.weight(z) * line;
    }
    const unsigned long long x = 2ull * sum + S, d = 2ull * S;
    unsigned long long out = __umul64hi(x, reciprocal);
    if (x - out * d >= d) out++;
    dst[((size_t)Z * (size_t)NY + (size_t)Y) * (size_t)cols + (size_t)q] = (T)out;
}

// ---------------------------------------------------------------------------------------------
// NEAREST: k_resample_nearest<BYTES, PER>
// ---------------------------------------------------------------------------------------------
// A plain gather, the texel's bits copied: source index j = ((2 X + 1) n) div (2 N) per axis.  Lanes run along the result's x, Y and Z are
// the workgroup's; a lane gathers PER texels of BYTES bytes and stores them as one word.  PER > 1 (byte and 16-bit texels whose result
// row is a whole number of dwords, so every row begins on one): one dword store per lane.  No loop but the PER gathers.
template <int BYTES> struct TexelWord;
template <> struct TexelWord<1> { typedef uint8_t type; };
template <> struct TexelWord<2> { typedef uint16_t type; };
template <> struct TexelWord<4> { typedef uint32_t type; };
template <> struct TexelWord<8> { typedef uint2 type; };
template <int BYTES, int PER>
__global__ __launch_bounds__(256) void k_resample_nearest(const void *__restrict__ src, void *__restrict__ dst, int nx, int ny, int nz, int NX, int NY, int NZ) {
    typedef typename TexelWord<BYTES>::type texel_t;
    const int g = (int)blockIdx.x * 256 + (int)threadIdx.x, Y = (int)blockIdx.y, Z = (int)blockIdx.z;
    if (g * PER >= NX) return;                                   // (PER > 1: NX is a multiple of PER)
    const int jy = ((2 * Y + 1) * ny) / (2 * NY), jz = ((2 * Z + 1) * nz) / (2 * NZ);
    const texel_t *row = reinterpret_cast<const texel_t *>(src) + ((size_t)jz * (size_t)ny + (size_t)jy) * (size_t)nx;
    const size_t o = ((size_t)Z * (size_t)NY + (size_t)Y) * (size_t)NX;
    if constexpr (PER == 1) {
        reinterpret_cast<texel_t *>(dst)[o + (size_t)g] = row[((2 * g + 1) * nx) / (2 * NX)];
    } else {
        uint32_t w = 0u;
#pragma unroll
        for (int k = 0; k < PER; k++) {
            const int X = g * PER + k;
            w |= (uint32_t)row[((2 * X + 1) * nx) / (2 * NX)] << (8 * BYTES * k);
        }
        reinterpret_cast<uint32_t *>(dst)[(o * BYTES) / 4 + (size_t)g] = w;
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
template <int BYTES>
static void launch_nearest(const vpt_volume *src, vpt_volume *d) {
    constexpr int PER = BYTES < 4 ? 4 / BYTES : 1;
    hipStream_t st = src->ctx->stream;
    const void *s = (const void *)src->linear.get(); void *o = (void *)d->linear.get();
    if (PER > 1 && d->nx % PER == 0)
        hipLaunchKernelGGL((k_resample_nearest<BYTES, PER>), dim3((unsigned)((d->nx / PER + 255) / 256), (unsigned)d->ny, (unsigned)d->nz), dim3(256), 0, st,
                           s, o, src->nx, src->ny, src->nz, d->nx, d->ny, d->nz);
    else
        hipLaunchKernelGGL((k_resample_nearest<BYTES, 1>), dim3((unsigned)((d->nx + 255) / 256), (unsigned)d->ny, (unsigned)d->nz), dim3(256), 0, st,
                           s, o, src->nx, src->ny, src->nz, d->nx, d->ny, d->nz);
}

// the two passes of FILTERED, src -> part -> d; ms (or null): the passes' milliseconds, the stream drained after each
template <typename T, int CH>
static int launch_filtered(const vpt_volume *src, vpt_volume *d, uint32_t *part, double *ms) {
    hipStream_t st = src->ctx->stream;
    const size_t row_bytes = (size_t)src->nx * CH * sizeof(T);
    const uint32_t rows = (uint32_t)src->ny * (uint32_t)src->nz;
    // as many rows as 16 KiB of LDS hold, and no more than give a workgroup 16384 results (a short row of a wide result would be one group's work)
    const uint32_t per = (uint32_t)std::max<size_t>(1, std::min<size_t>((size_t)RS_LDS_DWORDS * 4 / row_bytes, (size_t)16384 / (size_t)d->nx));
    PhaseClock clock(st);
    if (ms) HIP_TRY(clock.lap(&ms[0]));                       // what is in front of the passes is not theirs
    hipLaunchKernelGGL((k_resample_x<T, CH>), dim3((rows + per - 1) / per), dim3(256), 0, st, (const T *)src->linear.get(), part, src->nx, d->nx, rows, per,
                       (size_t)rows * row_bytes);
    HIP_TRY(hipGetLastError());
    if (ms) HIP_TRY(clock.lap(&ms[0]));
    const unsigned long long S = (unsigned long long)(d->nx >= src->nx ? 2 * d->nx : src->nx) * (unsigned long long)(d->ny >= src->ny ? 2 * d->ny : src->ny) *
                                 (unsigned long long)(d->nz >= src->nz ? 2 * d->nz : src->nz);
    const unsigned long long reciprocal = (unsigned long long)((((unsigned __int128)1) << 64) / (unsigned __int128)(2ull * S));      // 2 S >= 16: below 2^64
    const int cols = d->nx * CH;
    hipLaunchKernelGGL((k_resample_yz<T>), dim3((unsigned)((cols + 63) / 64), (unsigned)((d->ny + 3) / 4), (unsigned)d->nz), dim3(256), 0, st,
                       (const uint32_t *)part, (T *)d->linear.get(), cols, src->ny, d->ny, src->nz, d->nz, S, reciprocal);
    HIP_TRY(hipGetLastError());
    if (ms) HIP_TRY(clock.lap(&ms[1]));
    return VPT_OK;
}

static int resample(vpt_volume *src, int width, int height, int depth, int mode, vpt_volume **out, double *ms) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (mode != VPT_RESAMPLE_NEAREST && mode != VPT_RESAMPLE_FILTERED)
        return fail(VPT_ERR_INVALID, "resample mode %d: VPT_RESAMPLE_NEAREST (0) or VPT_RESAMPLE_FILTERED (1) are taken", mode);
    if (width < 1 || height < 1 || depth < 1 || width > RS_MAX_AXIS || height > RS_MAX_AXIS || depth > RS_MAX_AXIS)
        return fail(VPT_ERR_INVALID, "resample size %dx%dx%d: every axis is in 1 .. %d", width, height, depth, RS_MAX_AXIS);
    const VolumeFormat *f = volume_format(src->format);
    if (!f || f->packed_bytes)
        return fail(VPT_ERR_UNSUPPORTED, "a volume is resampled in its own format, which a packed format's decoded storage does not have: %s", format_name(src->format));
    if (mode == VPT_RESAMPLE_FILTERED && (f->is_float || f->is_signed))
        return fail(VPT_ERR_UNSUPPORTED, "FILTERED resampling takes unsigned normalised volumes (R8, RG8, R16, RG16; the window makes one of any scalar volume), not %s; "
                    "NEAREST takes every unpacked format", format_name(src->format));
    vpt_context *c = src->ctx;
    HIP_TRY(hipSetDevice(c->device));
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(c, width, height, depth, src->format, false, &d));      // every texel is written below
    if (ms) ms[0] = ms[1] = 0.0;
    if (mode == VPT_RESAMPLE_NEAREST) {
        switch (src->vox_bytes) {
            case 1: launch_nearest<1>(src, d); break;
            case 2: launch_nearest<2>(src, d); break;
            case 4: launch_nearest<4>(src, d); break;
            default: launch_nearest<8>(src, d); break;
        }
        return volume_finish_derived(src->ctx, src->filter, d, out);
    }
    DevBuf<uint32_t> part;                                       // the row pass's partial sums: freed when the call returns
    hipError_t e = part.alloc((size_t)width * (size_t)src->ny * (size_t)src->nz * (size_t)src->channels);
    if (e != hipSuccess) { vpt_volume_destroy(d); return fail(VPT_ERR_HIP, "resampling workspace: %s", hipGetErrorString(e)); }
    int rc;
    if (src->norm16) rc = src->channels == 2 ? launch_filtered<uint16_t, 2>(src, d, part.get(), ms) : launch_filtered<uint16_t, 1>(src, d, part.get(), ms);
    else rc = src->channels == 2 ? launch_filtered<uint8_t, 2>(src, d, part.get(), ms) : launch_filtered<uint8_t, 1>(src, d, part.get(), ms);
    if (rc != VPT_OK) { (void)hipStreamSynchronize(c->stream); vpt_volume_destroy(d); return rc; }
    rc = volume_finish_derived(src->ctx, src->filter, d, out);
    (void)hipStreamSynchronize(c->stream);                       // the workspace is freed on return: its last reader has finished
    return rc;
}

extern "C" int vpt_volume_resample(vpt_volume *src, int width, int height, int depth, int mode, vpt_volume **out) {
    return resample(src, width, height, depth, mode, out, nullptr);
}

extern "C" int vpt_volume_resample_timed(vpt_volume *src, int width, int height, int depth, int mode, vpt_volume **out, double *ms) {
    if (!ms) return fail(VPT_ERR_INVALID, "null argument");
    return resample(src, width, height, depth, mode, out, ms);
}
