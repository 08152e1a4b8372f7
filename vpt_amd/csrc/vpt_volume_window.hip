// vpt_volume_window.hip — the value-range window of a one-channel volume on the device (vpt_volume_window) and the two queries one
// chooses a window with: smallest / largest code (vpt_volume_range) and the full-resolution histogram (vpt_volume_code_histogram).
// C-ABI and the two contracts: include/vpt.h; kernel forms, compiler figures and measurements: DESIGN.md "Value-range window".
#include "vpt_internal.h"

// source texel kinds: what `linear` holds for the five one-channel formats
enum { SRC_U8 = 0, SRC_U16 = 1, SRC_S8 = 2, SRC_S16 = 3, SRC_F32 = 4 };
template <int SRC> struct SrcTraits {
    static constexpr int BYTES = SRC == SRC_F32 ? 4 : (SRC == SRC_U16 || SRC == SRC_S16) ? 2 : 1;
    static constexpr bool SIGNED = SRC == SRC_S8 || SRC == SRC_S16;
    static constexpr int BITS = BYTES * 8;
    static constexpr uint32_t BIAS = SIGNED ? 1u << (BITS - 1) : 0u;         // bin = code + BIAS
};
// texel j of the dwords a lane loaded (integer sources: the code, SNORM's most negative code read as the one above it)
template <int SRC>
__device__ __forceinline__ int code_of(const uint32_t *w, int j) {
    if (SRC == SRC_U8) return (int)((w[j >> 2] >> (8 * (j & 3))) & 255u);
    if (SRC == SRC_S8) return max((int)(int8_t)(w[j >> 2] >> (8 * (j & 3))), -127);
    if (SRC == SRC_U16) return (int)((w[j >> 1] >> (16 * (j & 1))) & 65535u);
    return max((int)(int16_t)(w[j >> 1] >> (16 * (j & 1))), -32767);
}

// ---------------------------------------------------------------------------------------------
// the window: k_window<SRC, OUT, ALIGNED>
// ---------------------------------------------------------------------------------------------
// Integer contract, out = (2 n M + D) div (2 D) with n = c - lo clamped to [0, D] (n = 0 gives D div 2 D = 0 and n = D gives
// (2 D M + D) div 2 D = M: the clamp IS the two saturating branches).  The clamp is one integer median on the code (the host moves a
// window that lies wholly above or below every code next to the codes, so that lo and n fit 32 bits: window_params), and the division
// is exact without a division, a table or an integer multiply:
//   out = trunc(fl(fl(n k) + h)),  k = fl(M / D),  h = fl(0.5 + 1 / (4 D))          (doubles, host-computed, wave-uniform)
// With N = 2 n M + D = q E + s, E = 2 D, 0 <= s <= E - 1, the real number n M / D + 0.5 + 1 / (4 D) = (N + 0.5) / E = q + (s + 0.5) / E lies
// at least 0.5 / E >= 2^-34 inside (q, q + 1) (D <= 2^32).  The computed one differs from it by less than 2^-35: n M / D < 2^16, so k's
// rounding (2^-53 relative) moves the product by at most 2^-37, the product's own rounding by 2^-38, h's by 2^-53 and the sum's
// (below 2^17) by 2^-37.  So the truncation is q.  No contraction is needed or wanted (-ffp-contract=off like the rest).
// Per voxel: extract, median, subtract, convert, multiply, add, convert, pack — two double operations, no integer multiply.
struct WindowParams {
    double lo;       // float: lo
    double d;        // float: hi - lo
    double m;        // M
    double k, h;     // integer: fl(M / D), fl(0.5 + 1 / (4 D))
    int clo, chi;    // integer: the codes are clamped to [clo, chi] = [lo, hi] cut to int32
};
template <int SRC>
__device__ __forceinline__ uint32_t window_code(int c, const WindowParams &p) {
    const uint32_t n = (uint32_t)min(max(c, p.clo), p.chi) - (uint32_t)p.clo;      // c - lo in [0, D], < 2^32 (mod 2^32 arithmetic)
    return (uint32_t)((double)n * p.k + p.h);
}
// Float contract: t = ((double) v - lo) / (hi - lo); 0 if !(t > 0) (NaN, -inf), M if t >= 1, else floor(t M + 0.5): four double operations,
// the division IEEE (the compiler's correctly rounded expansion), and a floor.  Without branches: t cut to [0, 1] gives floor(M + 0.5) = M
// at the upper end, and the one select on !(t > 0) also takes NaN.
__device__ __forceinline__ uint32_t window_float(float v, const WindowParams &p) {
    const double t = ((double)v - p.lo) / p.d;
    const double tc = fmax(fmin(t, 1.0), 0.0);
    const uint32_t r = (uint32_t)floor(tc * p.m + 0.5);
    return t > 0.0 ? r : 0u;
}
// A lane takes 16 consecutive voxels per step: 16 * Bsrc bytes in (one, two or four 16-byte loads) and 16 or 32 bytes out (one or two
// 16-byte stores); R16 -> R8 is two loads per store.  The volume's linear storage is one array, so only its last n % 16 voxels are a
// tail, taken texel by texel (ALIGNED: there is none).  OUT = bytes per result texel.
template <int SRC, int OUT, bool ALIGNED>
__global__ __launch_bounds__(256) void k_window(const void *__restrict__ src, void *__restrict__ dst, size_t n, WindowParams p) {
    constexpr int BS = SrcTraits<SRC>::BYTES;
    const size_t groups = n / 16, stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t g = first; g < groups; g += stride) {
        uint32_t w[4 * BS];
#pragma unroll
        for (int k = 0; k < BS; k++) {
            const uint4 q = reinterpret_cast<const uint4 *>(src)[g * BS + k];
            w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w;
        }
        uint32_t o[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if constexpr (SRC == SRC_F32) o[j] = window_float(__uint_as_float(w[j]), p);
            else o[j] = window_code<SRC>(code_of<SRC>(w, j), p);
        }
        if (OUT == 1) {
            uint32_t d[4];
#pragma unroll
            for (int k = 0; k < 4; k++) d[k] = o[4 * k] | (o[4 * k + 1] << 8) | (o[4 * k + 2] << 16) | (o[4 * k + 3] << 24);
            reinterpret_cast<uint4 *>(dst)[g] = make_uint4(d[0], d[1], d[2], d[3]);
        } else {
            uint32_t d[8];
#pragma unroll
            for (int k = 0; k < 8; k++) d[k] = o[2 * k] | (o[2 * k + 1] << 16);
            reinterpret_cast<uint4 *>(dst)[g * 2] = make_uint4(d[0], d[1], d[2], d[3]);
            reinterpret_cast<uint4 *>(dst)[g * 2 + 1] = make_uint4(d[4], d[5], d[6], d[7]);
        }
    }
    if (!ALIGNED) {
        for (size_t i = groups * 16 + first; i < n; i += stride) {
            uint32_t o;
            if constexpr (SRC == SRC_F32) o = window_float(reinterpret_cast<const float *>(src)[i], p);
            else {
                uint32_t w1[1];
                if (BS == 1) w1[0] = reinterpret_cast<const uint8_t *>(src)[i];
                else w1[0] = reinterpret_cast<const uint16_t *>(src)[i];
                o = window_code<SRC>(code_of<SRC>(w1, 0), p);
            }
            if (OUT == 1) reinterpret_cast<uint8_t *>(dst)[i] = (uint8_t)o;
            else reinterpret_cast<uint16_t *>(dst)[i] = (uint16_t)o;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// smallest / largest texel: k_range<SRC>
// ---------------------------------------------------------------------------------------------
// out[0] = min, out[1] = max of an order-preserving unsigned encoding (the host sets them to 0xffffffff and 0: "no texel yet"):
//   integer sources: the bin, code + BIAS (SNORM's most negative code is clamped by the host: the clamp is monotone);
//   floats: the bits with the sign bit set (v >= 0) or all bits inverted (v < 0); NaN texels are skipped (min / max of a NaN
//   accumulator and a number is the number, so the accumulators start as NaN and stay NaN only while nothing else was seen).
// Integer texels are reduced two at a time as packed 16-bit lanes (bytes: the even and the odd bytes of a dword as two such pairs).
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
__device__ __forceinline__ uint32_t float_order(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
template <int SRC>
__global__ __launch_bounds__(256) void k_range(const void *__restrict__ src, size_t n, uint32_t *__restrict__ out) {
    typedef SrcTraits<SRC> S;
    constexpr int PER = 16 / S::BYTES;
    const size_t nvec = n / PER, stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t mn = 0xffffffffu, mx = 0u;
    if (SRC == SRC_F32) {
        float fmn = __uint_as_float(0x7fc00000u), fmx = fmn;
        for (size_t i = first; i < nvec; i += stride) {
            const uint4 q = reinterpret_cast<const uint4 *>(src)[i];
            const float f[4] = { __uint_as_float(q.x), __uint_as_float(q.y), __uint_as_float(q.z), __uint_as_float(q.w) };
#pragma unroll
            for (int j = 0; j < 4; j++) { fmn = fminf(fmn, f[j]); fmx = fmaxf(fmx, f[j]); }
        }
        for (size_t i = nvec * PER + first; i < n; i += stride) {
            const float f = reinterpret_cast<const float *>(src)[i];
            fmn = fminf(fmn, f); fmx = fmaxf(fmx, f);
        }
        if (fmn == fmn) { mn = float_order(fmn); mx = float_order(fmx); }
    } else {
        constexpr uint32_t FLIP = S::SIGNED ? (S::BYTES == 1 ? 0x80808080u : 0x80008000u) : 0u;
        uint32_t pmn = 0xffffffffu, pmx = 0u;
        for (size_t i = first; i < nvec; i += stride) {
            const uint4 q = reinterpret_cast<const uint4 *>(src)[i];
            const uint32_t d[4] = { q.x ^ FLIP, q.y ^ FLIP, q.z ^ FLIP, q.w ^ FLIP };
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (S::BYTES == 1) {
                    const uint32_t a = d[j] & 0x00ff00ffu, b = (d[j] >> 8) & 0x00ff00ffu;
                    pmn = pk_min(pk_min(pmn, a), b); pmx = pk_max(pk_max(pmx, a), b);
                } else { pmn = pk_min(pmn, d[j]); pmx = pk_max(pmx, d[j]); }
            }
        }
        mn = min(pmn & 65535u, pmn >> 16); mx = max(pmx & 65535u, pmx >> 16);
        for (size_t i = nvec * PER + first; i < n; i += stride) {
            const uint32_t c = (S::BYTES == 1 ? (uint32_t)reinterpret_cast<const uint8_t *>(src)[i] : (uint32_t)reinterpret_cast<const uint16_t *>(src)[i]) ^ S::BIAS;
            mn = min(mn, c); mx = max(mx, c);
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { mn = min(mn, (uint32_t)__shfl_xor((int)mn, s)); mx = max(mx, (uint32_t)__shfl_xor((int)mx, s)); }
    __shared__ uint32_t part[2][4];
    const int tid = (int)threadIdx.x;
    if ((tid & 63) == 0) { part[0][tid >> 6] = mn; part[1][tid >> 6] = mx; }
    __syncthreads();
    if (tid == 0) {
        mn = min(min(part[0][0], part[0][1]), min(part[0][2], part[0][3]));
        mx = max(max(part[1][0], part[1][1]), max(part[1][2], part[1][3]));
        if (mn <= mx) { atomicMin(&out[0], mn); atomicMax(&out[1], mx); }       // (a workgroup that saw no texel has mn > mx)
    }
}

// ---------------------------------------------------------------------------------------------
// counts per code: k_code_histogram<SRC>
// ---------------------------------------------------------------------------------------------
// Counts are integers: atomic adds in any order give the same bins.  bin = code + BIAS; SNORM's most negative code counts as the one
// above it (bin 1).  8-bit: 256 bins, one private LDS copy per wave, as k_histogram.  16-bit: 65 536 x 4 B does not fit LDS, so the
// CODE_SLAB bins from the volume's smallest code on (k_range's result, read from the device: no host round trip) are counted in LDS
// (32 KiB: five workgroups per CU) and the rest by global atomics — a 12-bit series in a 16-bit container, or Hounsfield units from
// -1024 up, is inside the slab as a whole.
#define CODE_SLAB 8192
template <int SRC>
__global__ __launch_bounds__(256) void k_code_histogram(const void *__restrict__ src, size_t n, uint32_t *__restrict__ bins, const uint32_t *__restrict__ range) {
    typedef SrcTraits<SRC> S;
    constexpr int PER = 16 / S::BYTES;
    const int tid = (int)threadIdx.x;
    const size_t nvec = n / PER, stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + tid;
    if (S::BYTES == 1) {
        __shared__ uint32_t h[4][256];
        const int wave = tid >> 6;
        for (int i = 0; i < 4; i++) h[i][tid] = 0u;
        __syncthreads();
        constexpr uint32_t FLIP = S::SIGNED ? 0x80808080u : 0u;
        for (size_t i = first; i < nvec; i += stride) {
            const uint4 q = reinterpret_cast<const uint4 *>(src)[i];
            const uint32_t d[4] = { q.x ^ FLIP, q.y ^ FLIP, q.z ^ FLIP, q.w ^ FLIP };
#pragma unroll
            for (int j = 0; j < 4; j++) {
#pragma unroll
                for (int b = 0; b < 4; b++) atomicAdd(&h[wave][(d[j] >> (8 * b)) & 255u], 1u);
            }
        }
        for (size_t i = nvec * PER + first; i < n; i += stride) atomicAdd(&h[wave][((uint32_t)reinterpret_cast<const uint8_t *>(src)[i] ^ FLIP) & 255u], 1u);
        __syncthreads();
        const uint32_t sum = h[0][tid] + h[1][tid] + h[2][tid] + h[3][tid];
        if (sum) atomicAdd(&bins[S::SIGNED && tid == 0 ? 1 : tid], sum);
    } else {
        __shared__ uint32_t h[CODE_SLAB];
        for (int i = tid; i < CODE_SLAB; i += 256) h[i] = 0u;
        __syncthreads();
        const uint32_t base = min(range[0], 65536u - (uint32_t)CODE_SLAB);      // (no texel: 0xffffffff, and nothing is counted)
        constexpr uint32_t FLIP = S::SIGNED ? 0x8000u : 0u;
        auto count = [&](uint32_t raw) {
            uint32_t bin = raw ^ FLIP;
            if (S::SIGNED) bin = max(bin, 1u);
            const uint32_t rel = bin - base;
            if (rel < (uint32_t)CODE_SLAB) atomicAdd(&h[rel], 1u);
            else atomicAdd(&bins[bin], 1u);
        };
        for (size_t i = first; i < nvec; i += stride) {
            const uint4 q = reinterpret_cast<const uint4 *>(src)[i];
            const uint32_t d[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
            for (int j = 0; j < 4; j++) { count(d[j] & 65535u); count(d[j] >> 16); }
        }
        for (size_t i = nvec * PER + first; i < n; i += stride) count((uint32_t)reinterpret_cast<const uint16_t *>(src)[i]);
        __syncthreads();
        for (int i = tid; i < CODE_SLAB; i += 256) { const uint32_t c = h[i]; if (c) atomicAdd(&bins[base + (uint32_t)i], c); }
    }
}

// ---------------------------------------------------------------------------------------------
// hosts
// ---------------------------------------------------------------------------------------------
// the texel kind of a one-channel source, or -1
static int source_kind(const vpt_volume *v) {                   // -1: not a one-channel volume
    const VolumeFormat *f = volume_format(v->format);
    if (!f || f->channels != 1) return -1;
    if (f->is_float) return SRC_F32;
    return f->bytes == 2 ? (f->is_signed ? SRC_S16 : SRC_U16) : (f->is_signed ? SRC_S8 : SRC_U8);
}
static inline size_t voxels(const vpt_volume *v) { return (size_t)v->nx * v->ny * v->nz; }

template <int SRC, int OUT>
static void launch_window_out(const vpt_volume *src, vpt_volume *dst, const WindowParams &p) {
    const size_t n = voxels(src);
    const dim3 grid(stream_grid(n / 16 + 1, 256, 2048));            // eight workgroups per CU, a stride loop beyond 2^23 voxels
    if (n % 16 == 0) hipLaunchKernelGGL((k_window<SRC, OUT, true>), grid, dim3(256), 0, src->ctx->stream, (const void *)src->linear, (void *)dst->linear, n, p);
    else hipLaunchKernelGGL((k_window<SRC, OUT, false>), grid, dim3(256), 0, src->ctx->stream, (const void *)src->linear, (void *)dst->linear, n, p);
}
template <int SRC>
static void launch_window(const vpt_volume *src, vpt_volume *dst, const WindowParams &p) {
    if (dst->norm16) launch_window_out<SRC, 2>(src, dst, p);
    else launch_window_out<SRC, 1>(src, dst, p);
}

extern "C" int vpt_volume_window(vpt_volume *src, double lo, double hi, int out_format, vpt_volume **out) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    const int kind = source_kind(src);
    if (kind < 0)
        return fail(VPT_ERR_UNSUPPORTED, "a window is taken from one-channel volumes (R8, R16, R8_SNORM, R16_SNORM, R32F), not from %s", format_name(src->format));
    if (out_format != VPT_FORMAT_R8 && out_format != VPT_FORMAT_R16)
        return fail(VPT_ERR_INVALID, "a windowed volume is R8 or R16, not %s", format_name(out_format));
    const double m = out_format == VPT_FORMAT_R16 ? 65535.0 : 255.0;
    WindowParams p = {};
    if (kind == SRC_F32) {
        const double d = hi - lo;
        if (!std::isfinite(lo) || !std::isfinite(hi) || !std::isfinite(d) || !(hi > lo))
            return fail(VPT_ERR_INVALID, "window [%g, %g] of an R32F volume: lo, hi and hi - lo must be finite and hi > lo", lo, hi);
        p.lo = lo; p.d = d; p.m = m;
    } else {
        const double lim = 2147483648.0;
        if (!(std::floor(lo) == lo && std::floor(hi) == hi && std::fabs(lo) <= lim && std::fabs(hi) <= lim && hi - lo >= 1.0))
            return fail(VPT_ERR_INVALID, "window [%g, %g] of an %s volume: lo and hi must be integers in [-2^31, 2^31] with hi - lo >= 1", lo, hi, format_name(src->format));
        // a window wholly above every code (all 0) or wholly below (all M) is replaced by one of width 1 next to the codes with the same
        // result; after that lo < 2^16 and hi > -2^15, so lo fits int32 and c - lo fits uint32
        if (lo >= 65536.0) { lo = 65536.0; hi = 65537.0; }
        else if (hi <= -32768.0) { lo = -32770.0; hi = -32769.0; }
        const double d = hi - lo;                                // exact: <= 2^32
        p.m = m; p.k = m / d; p.h = 0.5 + 1.0 / (4.0 * d);
        p.clo = (int)lo; p.chi = (int)std::min(hi, 2147483647.0);
    }
    vpt_context *c = src->ctx;
    HIP_TRY(hipSetDevice(c->device));
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(c, src->nx, src->ny, src->nz, out_format, false, &d));   // every texel is written below
    switch (kind) {
        case SRC_U8: launch_window<SRC_U8>(src, d, p); break;
        case SRC_U16: launch_window<SRC_U16>(src, d, p); break;
        case SRC_S8: launch_window<SRC_S8>(src, d, p); break;
        case SRC_S16: launch_window<SRC_S16>(src, d, p); break;
        default: launch_window<SRC_F32>(src, d, p); break;
    }
    return volume_finish_derived(src->ctx, src->filter, d, out);
}

// enqueues k_range of `v` into dev[0..1] (encoded min, max) on the context's stream
static hipError_t enqueue_range(const vpt_volume *v, int kind, uint32_t *dev) {
    hipStream_t st = v->ctx->stream;
    hipError_t e = hipMemsetAsync(dev, 0xff, 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(dev + 1, 0, 4, st);
    if (e != hipSuccess) return e;
    const size_t n = voxels(v);
    const dim3 grid(stream_grid(n * (size_t)v->vox_bytes / 16 + 1, 256, 2048));
    const void *s = (const void *)v->linear;
    switch (kind) {
        case SRC_U8: hipLaunchKernelGGL(k_range<SRC_U8>, grid, dim3(256), 0, st, s, n, dev); break;
        case SRC_U16: hipLaunchKernelGGL(k_range<SRC_U16>, grid, dim3(256), 0, st, s, n, dev); break;
        case SRC_S8: hipLaunchKernelGGL(k_range<SRC_S8>, grid, dim3(256), 0, st, s, n, dev); break;
        case SRC_S16: hipLaunchKernelGGL(k_range<SRC_S16>, grid, dim3(256), 0, st, s, n, dev); break;
        default: hipLaunchKernelGGL(k_range<SRC_F32>, grid, dim3(256), 0, st, s, n, dev); break;
    }
    return hipGetLastError();
}

extern "C" int vpt_volume_range(vpt_volume *v, double *lo, double *hi) {
    if (!v || !lo || !hi) return fail(VPT_ERR_INVALID, "null argument");
    const int kind = source_kind(v);
    if (kind < 0)
        return fail(VPT_ERR_UNSUPPORTED, "the range is taken from one-channel volumes (R8, R16, R8_SNORM, R16_SNORM, R32F), not from %s", format_name(v->format));
    vpt_context *c = v->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<uint32_t> dev;
    uint32_t host[2] = { 0u, 0u };
    HIP_TRY(dev.alloc(2));
    HIP_TRY(enqueue_range(v, kind, dev));
    HIP_TRY(hipMemcpyAsync(host, dev, sizeof(host), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (host[0] > host[1]) return fail(VPT_ERR_INVALID, "the %s volume holds no texel that is not NaN: it has no range", format_name(v->format));
    if (kind == SRC_F32) {
        float f[2];
        for (int i = 0; i < 2; i++) {
            const uint32_t u = host[i], bits = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
            memcpy(&f[i], &bits, 4);
        }
        *lo = (double)f[0]; *hi = (double)f[1];
    } else {
        const bool wide = kind == SRC_U16 || kind == SRC_S16, sgn = kind == SRC_S8 || kind == SRC_S16;
        const long bias = sgn ? (wide ? 32768 : 128) : 0, least = sgn ? -(bias - 1) : 0;
        *lo = (double)std::max((long)host[0] - bias, least);
        *hi = (double)std::max((long)host[1] - bias, least);
    }
    return VPT_OK;
}

extern "C" int vpt_volume_code_histogram(vpt_volume *v, uint32_t *bins, size_t nbins) {
    if (!v || !bins) return fail(VPT_ERR_INVALID, "null argument");
    const int kind = source_kind(v);
    if (kind < 0 || kind == SRC_F32)
        return fail(VPT_ERR_UNSUPPORTED, "codes are counted for R8, R16, R8_SNORM and R16_SNORM volumes, not for %s", format_name(v->format));
    const bool wide = kind == SRC_U16 || kind == SRC_S16;
    const size_t want = wide ? 65536 : 256;
    if (nbins != want) return fail(VPT_ERR_INVALID, "a code histogram of an %s volume has %zu bins, not %zu", format_name(v->format), want, nbins);
    if (voxels(v) > 0xFFFFFFFFull) return fail(VPT_ERR_UNSUPPORTED, "code histogram: %zu voxels exceed 2^32 - 1 (the bins are 32-bit)", voxels(v));
    vpt_context *c = v->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<uint32_t> buf;                                       // the bins, then k_range's two words
    HIP_TRY(buf.alloc(want + 2));
    uint32_t *dev = buf;
    HIP_TRY(hipMemsetAsync(dev, 0, want * sizeof(uint32_t), c->stream));
    if (wide) HIP_TRY(enqueue_range(v, kind, dev + want));
    const size_t n = voxels(v);
    const dim3 grid(stream_grid(n * (size_t)v->vox_bytes / 16 + 1, 256, wide ? 1280 : 2048));
    const void *s = (const void *)v->linear;
    switch (kind) {
        case SRC_U8: hipLaunchKernelGGL(k_code_histogram<SRC_U8>, grid, dim3(256), 0, c->stream, s, n, dev, (const uint32_t *)(dev + want)); break;
        case SRC_S8: hipLaunchKernelGGL(k_code_histogram<SRC_S8>, grid, dim3(256), 0, c->stream, s, n, dev, (const uint32_t *)(dev + want)); break;
        case SRC_U16: hipLaunchKernelGGL(k_code_histogram<SRC_U16>, grid, dim3(256), 0, c->stream, s, n, dev, (const uint32_t *)(dev + want)); break;
        default: hipLaunchKernelGGL(k_code_histogram<SRC_S16>, grid, dim3(256), 0, c->stream, s, n, dev, (const uint32_t *)(dev + want)); break;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(bins, dev, want * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VPT_OK;
}
