// vpt_volume_combine.hip — two volumes of one grid combined texel by texel into a third (vpt_volume_combine: mask, min, max, absolute
// difference, weighted blend, pair) or compared without making one (vpt_volume_compare: eight exact counts and sums), on the device.
// C-ABI and the contract: include/vpt.h; kernel forms, compiler figures and measurements: DESIGN.md "Combining two volumes".
//
// Everything is integer and elementwise over the linear index: no LDS, no workgroup waits for another, no float arithmetic, and the only
// atomics are the integer ones at the end of a wave of k_compare.
#include "vpt_internal.h"

// ---------------------------------------------------------------------------------------------
// the loads both kernels share
// ---------------------------------------------------------------------------------------------
// A lane takes a group of G = 16 / sizeof(TA) consecutive voxels (16 byte texels, 8 16-bit texels): a's texels are one 16-byte load, b's
// the G * STRIDE_B * sizeof(TB) bytes behind the same voxel index, 8 bytes (one uint2) or 16 .. 64 bytes (one to four uint4; more than two
// only where MASK or compare read a wider b than a).  A two-channel b is read whole and the channel taken with a shift.  Group g begins at
// byte 16 g of a and at byte 16 g * STRIDE_B * sizeof(TB) / sizeof(TA) of b: both are multiples of the load's size whatever nx is, and the
// storage begins on a 256-byte boundary.
template <typename TA, typename TB, int STRIDE_B> struct Group {
    static constexpr int G = 16 / (int)sizeof(TA);
    static constexpr int B_DWORDS = G * STRIDE_B * (int)sizeof(TB) / 4;       // 2, 4, 8 or 16
    uint32_t a[4], b[B_DWORDS];
    __device__ __forceinline__ void load(const TA *__restrict__ pa, const TB *__restrict__ pb, size_t g) {
        const uint4 w = reinterpret_cast<const uint4 *>(pa)[g];
        a[0] = w.x; a[1] = w.y; a[2] = w.z; a[3] = w.w;
        if constexpr (B_DWORDS == 2) {
            const uint2 v = reinterpret_cast<const uint2 *>(pb)[g];
            b[0] = v.x; b[1] = v.y;
        } else {
#pragma unroll
            for (int k = 0; k < B_DWORDS / 4; k++) {
                const uint4 v = reinterpret_cast<const uint4 *>(pb)[g * (B_DWORDS / 4) + k];
                b[4 * k] = v.x; b[4 * k + 1] = v.y; b[4 * k + 2] = v.z; b[4 * k + 3] = v.w;
            }
        }
    }
    // voxel i of the group (a compile-time index once the loops are unrolled): a's code, and the code of b's channel, which sits
    // `shift` = 8 * sizeof(TB) * b_channel bits up in b's texel
    __device__ __forceinline__ uint32_t code_a(int i) const {
        constexpr int PER = 4 / (int)sizeof(TA);
        return (a[i / PER] >> (8 * (int)sizeof(TA) * (i % PER))) & ((1u << (8 * sizeof(TA))) - 1u);
    }
    __device__ __forceinline__ uint32_t code_b(int i, uint32_t shift) const {
        constexpr int TEXEL = STRIDE_B * (int)sizeof(TB);                      // 1, 2 or 4 bytes
        constexpr int PER = 4 / TEXEL;
        const uint32_t texel = TEXEL == 4 ? b[i] : (b[i / PER] >> (8 * TEXEL * (i % PER)));
        return (texel >> shift) & ((1u << (8 * sizeof(TB))) - 1u);
    }
};

struct CombineArgs {
    uint32_t lo, hi, fill;         // MASK
    int32_t wa, wb, offset;        // BLEND
    uint32_t shift;                // of b's channel inside b's texel
};

// one result code.  BLEND: |wa A + wb B + 128| <= 2 * 4096 * 65535 + 128 < 2^30, so int32 is exact; >> of a negative int is the arithmetic
// shift (floor), and the offset (|.| <= 65535) keeps the sum far inside int32
template <int OP, uint32_t M>
__device__ __forceinline__ uint32_t combine_one(uint32_t A, uint32_t B, const CombineArgs &p) {
    if constexpr (OP == VPT_COMBINE_MASK) return (B >= p.lo && B <= p.hi) ? A : p.fill;
    else if constexpr (OP == VPT_COMBINE_MIN) return min(A, B);
    else if constexpr (OP == VPT_COMBINE_MAX) return max(A, B);
    else if constexpr (OP == VPT_COMBINE_ABSDIFF) return max(A, B) - min(A, B);
    else {
        const int32_t s = ((p.wa * (int32_t)A + p.wb * (int32_t)B + 128) >> 8) + p.offset;
        return (uint32_t)min(max(s, 0), (int32_t)M);
    }
}

// ---------------------------------------------------------------------------------------------
// k_combine<TA, TB, STRIDE_B, OP>
// ---------------------------------------------------------------------------------------------
// A grid-stride loop over the groups; the result of a group is one 16-byte store, the interleaved (A, B) texels of PAIR two.  The last
// n mod G voxels go one by one.  Bounds: g < groups = n div G, so the loads end at voxel groups * G - 1 < n of either source and the stores
// at the same voxel of the result (PAIR: texel 2 (groups * G) - 1 of 2 n); the tail runs over groups * G .. n - 1.
template <typename TA, typename TB, int STRIDE_B, int OP>
__global__ __launch_bounds__(256) void k_combine(const TA *__restrict__ a, const TB *__restrict__ b, TA *__restrict__ dst, size_t n, CombineArgs p) {
    typedef Group<TA, TB, STRIDE_B> Grp;
    constexpr int G = Grp::G, PER = 4 / (int)sizeof(TA), BITS = 8 * (int)sizeof(TA);
    constexpr uint32_t M = (1u << BITS) - 1u;
    const size_t groups = n / G, stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t g = t0; g < groups; g += stride) {
        Grp v;
        v.load(a, b, g);
        if constexpr (OP == VPT_COMBINE_PAIR) {
            uint32_t o[8] = {};
#pragma unroll
            for (int i = 0; i < G; i++) {                        // texel i is the codes 2 i and 2 i + 1 of the result
                const uint32_t A = v.code_a(i), B = v.code_b(i, p.shift);
                o[(2 * i) / PER] |= A << (BITS * ((2 * i) % PER));
                o[(2 * i + 1) / PER] |= B << (BITS * ((2 * i + 1) % PER));
            }
            reinterpret_cast<uint4 *>(dst)[2 * g] = make_uint4(o[0], o[1], o[2], o[3]);
            reinterpret_cast<uint4 *>(dst)[2 * g + 1] = make_uint4(o[4], o[5], o[6], o[7]);
        } else {
            uint32_t o[4] = {};
#pragma unroll
            for (int i = 0; i < G; i++) o[i / PER] |= combine_one<OP, M>(v.code_a(i), v.code_b(i, p.shift), p) << (BITS * (i % PER));
            reinterpret_cast<uint4 *>(dst)[g] = make_uint4(o[0], o[1], o[2], o[3]);
        }
    }
    for (size_t i = groups * G + t0; i < n; i += stride) {
        const uint32_t A = (uint32_t)a[i], B = (uint32_t)b[i * STRIDE_B + (p.shift ? 1 : 0)];
        if constexpr (OP == VPT_COMBINE_PAIR) { dst[2 * i] = (TA)A; dst[2 * i + 1] = (TA)B; }
        else dst[i] = (TA)combine_one<OP, M>(A, B, p);
    }
}

// ---------------------------------------------------------------------------------------------
// k_compare<TA, TB, STRIDE_B>
// ---------------------------------------------------------------------------------------------
// The same loads; every lane keeps its own 64-bit partial of each quantity.  No partial can overflow: a lane sees a subset of the volume's
// voxels, the entry point refuses more than 2^32 - 1 of them, and |A - B| <= 65535, so even the sum of squares over ALL voxels is at most
// (2^32 - 1) * 65535^2 < 2^64 (and that holds whatever stride the grid gives a lane).  The wave adds its lanes up with shuffles, and lane 0
// issues one integer atomic per quantity into one of CMP_SLOTS rows by the wave's number; the host adds the rows (one row serialised the
// waves: DESIGN.md "Distance transform").  Integer addition and maximum are associative, so the order of the atomics does not show.
#define CMP_SLOTS 64
#define CMP_WORDS 8                // differing, max |A - B|, sum |A - B|, sum (A - B)^2, in a, in b, in both, (unused)
struct CompareArgs { uint32_t lo_a, hi_a, lo_b, hi_b, shift; };
struct ComparePartial {
    unsigned long long differing = 0ull, largest = 0ull, sum_abs = 0ull, sum_sq = 0ull, in_a = 0ull, in_b = 0ull, both = 0ull;
    __device__ __forceinline__ void take(uint32_t A, uint32_t B, const CompareArgs &p) {
        const uint32_t d = max(A, B) - min(A, B);
        const bool ia = A >= p.lo_a && A <= p.hi_a, ib = B >= p.lo_b && B <= p.hi_b;
        differing += d ? 1ull : 0ull;
        largest = max(largest, (unsigned long long)d);
        sum_abs += d;
        sum_sq += (unsigned long long)d * d;
        in_a += ia ? 1ull : 0ull; in_b += ib ? 1ull : 0ull; both += (ia && ib) ? 1ull : 0ull;
    }
};
template <typename TA, typename TB, int STRIDE_B>
__global__ __launch_bounds__(256) void k_compare(const TA *__restrict__ a, const TB *__restrict__ b, size_t n, CompareArgs p, unsigned long long *__restrict__ slots) {
    typedef Group<TA, TB, STRIDE_B> Grp;
    constexpr int G = Grp::G;
    const size_t groups = n / G, stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    ComparePartial s;
    for (size_t g = t0; g < groups; g += stride) {
        Grp v;
        v.load(a, b, g);
#pragma unroll
        for (int i = 0; i < G; i++) s.take(v.code_a(i), v.code_b(i, p.shift), p);
    }
    for (size_t i = groups * G + t0; i < n; i += stride) s.take((uint32_t)a[i], (uint32_t)b[i * STRIDE_B + (p.shift ? 1 : 0)], p);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s.differing += __shfl_xor(s.differing, o); s.sum_abs += __shfl_xor(s.sum_abs, o); s.sum_sq += __shfl_xor(s.sum_sq, o);
        s.in_a += __shfl_xor(s.in_a, o); s.in_b += __shfl_xor(s.in_b, o); s.both += __shfl_xor(s.both, o);
        s.largest = max(s.largest, __shfl_xor(s.largest, o));
    }
    if ((threadIdx.x & 63) == 0) {
        const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        unsigned long long *row = slots + (wave % CMP_SLOTS) * CMP_WORDS;
        if (s.differing) { atomicAdd(&row[0], s.differing); atomicMax(&row[1], s.largest); atomicAdd(&row[2], s.sum_abs); atomicAdd(&row[3], s.sum_sq); }
        if (s.in_a) atomicAdd(&row[4], s.in_a);
        if (s.in_b) atomicAdd(&row[5], s.in_b);
        if (s.both) atomicAdd(&row[6], s.both);
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static const char *const COMBINE_OP_NAMES[] = { "MASK", "MIN", "MAX", "ABSDIFF", "BLEND", "PAIR" };

// what both entry points ask of their two volumes; `what`: "combine" or "compare"
static int check_pair(const char *what, const vpt_volume *a, const vpt_volume *b, int b_channel) {
    if (a->format != VPT_FORMAT_R8 && a->format != VPT_FORMAT_R16)
        return fail(VPT_ERR_UNSUPPORTED, "%s: a is a one-channel unsigned normalised volume (R8, R16; the window makes one of any scalar volume), not %s",
                    what, format_name(a->format));
    if (b->format != VPT_FORMAT_R8 && b->format != VPT_FORMAT_RG8 && b->format != VPT_FORMAT_R16 && b->format != VPT_FORMAT_RG16)
        return fail(VPT_ERR_UNSUPPORTED, "%s: b is an unsigned normalised volume (R8, RG8, R16, RG16; the window makes R8 / R16 of any scalar volume), not %s",
                    what, format_name(b->format));
    if (a->ctx != b->ctx) return fail(VPT_ERR_INVALID, "%s: a and b belong to two contexts", what);
    if (a->nx != b->nx || a->ny != b->ny || a->nz != b->nz)
        return fail(VPT_ERR_INVALID, "%s: a is %dx%dx%d and b is %dx%dx%d; vpt_volume_resample brings two grids together", what, a->nx, a->ny, a->nz,
                    b->nx, b->ny, b->nz);
    if (b_channel != 0 && b_channel != 1) return fail(VPT_ERR_INVALID, "%s: channel %d of b: 0 or 1 are taken", what, b_channel);
    if (b_channel == 1 && b->channels != 2) return fail(VPT_ERR_INVALID, "%s: channel 1 of b, which has one channel (%s)", what, format_name(b->format));
    return VPT_OK;
}

template <typename TA, typename TB, int STRIDE_B, int OP>
static void launch_combine(const vpt_volume *a, const vpt_volume *b, vpt_volume *d, const CombineArgs &p) {
    const size_t n = (size_t)a->nx * (size_t)a->ny * (size_t)a->nz;
    hipLaunchKernelGGL((k_combine<TA, TB, STRIDE_B, OP>), dim3(stream_grid(n / Group<TA, TB, STRIDE_B>::G + 1)), dim3(256), 0, a->ctx->stream,
                       (const TA *)a->linear.get(), (const TB *)b->linear.get(), (TA *)d->linear.get(), n, p);
}
// MASK reads a b of either width; every other op has TB = TA (the caller has checked)
template <typename TA, int STRIDE_B>
static void launch_op(int op, const vpt_volume *a, const vpt_volume *b, vpt_volume *d, const CombineArgs &p) {
    switch (op) {
        case VPT_COMBINE_MASK:
            if (b->norm16) launch_combine<TA, uint16_t, STRIDE_B, VPT_COMBINE_MASK>(a, b, d, p);
            else launch_combine<TA, uint8_t, STRIDE_B, VPT_COMBINE_MASK>(a, b, d, p);
            break;
        case VPT_COMBINE_MIN: launch_combine<TA, TA, STRIDE_B, VPT_COMBINE_MIN>(a, b, d, p); break;
        case VPT_COMBINE_MAX: launch_combine<TA, TA, STRIDE_B, VPT_COMBINE_MAX>(a, b, d, p); break;
        case VPT_COMBINE_ABSDIFF: launch_combine<TA, TA, STRIDE_B, VPT_COMBINE_ABSDIFF>(a, b, d, p); break;
        case VPT_COMBINE_BLEND: launch_combine<TA, TA, STRIDE_B, VPT_COMBINE_BLEND>(a, b, d, p); break;
        default: launch_combine<TA, TA, STRIDE_B, VPT_COMBINE_PAIR>(a, b, d, p); break;
    }
}

static int combine(vpt_volume *a, vpt_volume *b, const struct vpt_combine_params *p, vpt_volume **out, double *ms) {
    if (!a || !b || !p || !out) return fail(VPT_ERR_INVALID, "null argument");
    VPT_TRY(check_pair("combine", a, b, p->b_channel));
    if (p->op < VPT_COMBINE_MASK || p->op > VPT_COMBINE_PAIR)
        return fail(VPT_ERR_INVALID, "combine op %d: VPT_COMBINE_MASK (0) .. VPT_COMBINE_PAIR (5) are taken", p->op);
    const uint32_t M = a->norm16 ? 65535u : 255u, Mb = b->norm16 ? 65535u : 255u;
    if (p->op == VPT_COMBINE_MASK) {
        if (p->lo > p->hi) return fail(VPT_ERR_INVALID, "combine MASK range [%u, %u]: lo exceeds hi", p->lo, p->hi);
        if (p->hi > Mb) return fail(VPT_ERR_INVALID, "combine MASK range [%u, %u]: the largest code of %s is %u", p->lo, p->hi, format_name(b->format), Mb);
        if (p->fill > M) return fail(VPT_ERR_INVALID, "combine MASK fill %u: the largest code of %s is %u", p->fill, format_name(a->format), M);
    } else if (a->norm16 != b->norm16) {
        return fail(VPT_ERR_UNSUPPORTED, "combine %s: the channels of a (%s) and b (%s) differ in width; only MASK takes that (the window makes R8 / R16 of any scalar volume)",
                    COMBINE_OP_NAMES[p->op], format_name(a->format), format_name(b->format));
    }
    if (p->op == VPT_COMBINE_BLEND) {
        if (p->wa < -4096 || p->wa > 4096 || p->wb < -4096 || p->wb > 4096)
            return fail(VPT_ERR_INVALID, "combine BLEND weights %d, %d: each is in -4096 .. 4096 (1/256 units)", p->wa, p->wb);
        if (p->offset < -65535 || p->offset > 65535) return fail(VPT_ERR_INVALID, "combine BLEND offset %d: -65535 .. 65535 are taken", p->offset);
    }
    vpt_context *c = a->ctx;
    HIP_TRY(hipSetDevice(c->device));
    const int format = p->op != VPT_COMBINE_PAIR ? a->format : a->norm16 ? VPT_FORMAT_RG16 : VPT_FORMAT_RG8;
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(c, a->nx, a->ny, a->nz, format, false, &d));        // every texel is written below
    CombineArgs args = { p->lo, p->hi, p->fill, p->wa, p->wb, p->offset, p->b_channel ? (b->norm16 ? 16u : 8u) : 0u };
    PhaseClock clock(c->stream);
    if (ms) {                                                    // what is in front of the pass is not its time
        const hipError_t e = clock.lap(ms);
        if (e != hipSuccess) { vpt_volume_destroy(d); return fail(VPT_ERR_HIP, "combine: %s", hipGetErrorString(e)); }
    }
    if (a->norm16) { if (b->channels == 2) launch_op<uint16_t, 2>(p->op, a, b, d, args); else launch_op<uint16_t, 1>(p->op, a, b, d, args); }
    else { if (b->channels == 2) launch_op<uint8_t, 2>(p->op, a, b, d, args); else launch_op<uint8_t, 1>(p->op, a, b, d, args); }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && ms) e = clock.lap(ms);
    if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); vpt_volume_destroy(d); return fail(VPT_ERR_HIP, "combine: %s", hipGetErrorString(e)); }
    return volume_finish_derived(c, a->filter, d, out);
}

extern "C" int vpt_volume_combine(vpt_volume *a, vpt_volume *b, const struct vpt_combine_params *p, vpt_volume **out) {
    return combine(a, b, p, out, nullptr);
}

extern "C" int vpt_volume_combine_timed(vpt_volume *a, vpt_volume *b, const struct vpt_combine_params *p, vpt_volume **out, double *ms) {
    if (!ms) return fail(VPT_ERR_INVALID, "null argument");
    *ms = 0.0;
    return combine(a, b, p, out, ms);
}

template <typename TA, typename TB, int STRIDE_B>
static void launch_compare(const vpt_volume *a, const vpt_volume *b, const CompareArgs &p, unsigned long long *slots) {
    const size_t n = (size_t)a->nx * (size_t)a->ny * (size_t)a->nz;
    hipLaunchKernelGGL((k_compare<TA, TB, STRIDE_B>), dim3(stream_grid(n / Group<TA, TB, STRIDE_B>::G + 1)), dim3(256), 0, a->ctx->stream,
                       (const TA *)a->linear.get(), (const TB *)b->linear.get(), n, p, slots);
}
template <typename TA>
static void launch_compare_b(const vpt_volume *a, const vpt_volume *b, const CompareArgs &p, unsigned long long *slots) {
    if (b->norm16) { if (b->channels == 2) launch_compare<TA, uint16_t, 2>(a, b, p, slots); else launch_compare<TA, uint16_t, 1>(a, b, p, slots); }
    else { if (b->channels == 2) launch_compare<TA, uint8_t, 2>(a, b, p, slots); else launch_compare<TA, uint8_t, 1>(a, b, p, slots); }
}

extern "C" int vpt_volume_compare(vpt_volume *a, vpt_volume *b, int b_channel, uint32_t lo_a, uint32_t hi_a, uint32_t lo_b, uint32_t hi_b, uint64_t out[8]) {
    if (!a || !b || !out) return fail(VPT_ERR_INVALID, "null argument");
    VPT_TRY(check_pair("compare", a, b, b_channel));
    const size_t n = (size_t)a->nx * (size_t)a->ny * (size_t)a->nz;
    if (n > 0xFFFFFFFFull) return fail(VPT_ERR_UNSUPPORTED, "compare: %zu voxels exceed 2^32 - 1 (the sum of squared differences is 64-bit)", n);
    vpt_context *c = a->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<unsigned long long> slots;                            // freed when the call returns
    HIP_TRY(slots.alloc(CMP_SLOTS * CMP_WORDS));
    HIP_TRY(hipMemsetAsync(slots, 0, CMP_SLOTS * CMP_WORDS * sizeof(unsigned long long), c->stream));
    const CompareArgs args = { lo_a, hi_a, lo_b, hi_b, b_channel ? (b->norm16 ? 16u : 8u) : 0u };
    if (a->norm16) launch_compare_b<uint16_t>(a, b, args, slots.get()); else launch_compare_b<uint8_t>(a, b, args, slots.get());
    unsigned long long host[CMP_SLOTS * CMP_WORDS] = {};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host, slots, sizeof(host), hipMemcpyDeviceToHost, c->stream);
    const hipError_t drained = hipStreamSynchronize(c->stream);  // `slots` goes out of scope behind its last use, whatever happened
    if (e == hipSuccess) e = drained;
    if (e != hipSuccess) return fail(VPT_ERR_HIP, "compare: %s", hipGetErrorString(e));
    uint64_t sum[CMP_WORDS] = {};
    for (int s = 0; s < CMP_SLOTS; s++)
        for (int k = 0; k < CMP_WORDS; k++) sum[k] = k == 1 ? std::max<uint64_t>(sum[k], host[s * CMP_WORDS + k]) : sum[k] + host[s * CMP_WORDS + k];
    out[0] = (uint64_t)n;
    for (int k = 0; k < 7; k++) out[k + 1] = sum[k];
    return VPT_OK;
}
