// vpt_volume_pyramid.hip — a volume's next coarser level (vpt_volume_reduce: 2 x 2 x 2 cells averaged) and its binomial smoothing
// (vpt_volume_smooth: the separable (1, 2, 1)^3 / 64 kernel, 1 .. 8 passes) on the device.  C-ABI and the two contracts: include/vpt.h;
// kernel forms, compiler figures and measurements: DESIGN.md "Binomial smoothing and 2x reduction".
#include "vpt_internal.h"

// texel kinds of a stored channel: what `linear` holds for the ten formats the reduction takes
enum { K_U8 = 0, K_U16 = 1, K_S8 = 2, K_S16 = 3, K_F32 = 4 };
template <int KIND> struct KindTraits {
    static constexpr int BYTES = KIND == K_F32 ? 4 : (KIND == K_U16 || KIND == K_S16) ? 2 : 1;
};
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}

// ---------------------------------------------------------------------------------------------
// the reduction: k_reduce<KIND, CHANNELS, ALIGNED>
// ---------------------------------------------------------------------------------------------
// Integer contract, out = (sum of the eight codes + 4) >> 3 (arithmetic shift).  Signed codes are summed as u = c + 2^(B-1) (the stored
// bits with the sign bit flipped, the most negative code's 0 raised to 1: SNORM reads it as the one above it): the sum of the eight u is
// the sum of the codes + 8 * 2^(B-1), a multiple of 8 more, so (sum u + 4) >> 3 is the result + 2^(B-1) and flipping the sign bit back
// gives the result's bits.  Everything is unsigned from there on, and the bytes of a dword add as packed 16-bit lanes (8 * 255 < 2^16).
// Float contract, doubles: ((a000 + a100) + (a010 + a110)) + ((a001 + a101) + (a011 + a111)), times 0.125 (exact), rounded once to float.
//
// ALIGNED (the source row is a multiple of 32 bytes, so the result row is one of 16): a lane produces the 16 contiguous result bytes
// of one chunk from the 32 source bytes below them in each of the four rows (y0, z0), (y1, z0), (y0, z1), (y1, z1), y1 = min(2 Y + 1,
// ny - 1), z1 likewise — eight 16-byte loads, one 16-byte store; consecutive lanes take consecutive chunks of the result's storage, so
// a wave stores 1 KiB contiguously and loads 2 KiB contiguously from each row it touches.  One chunk per lane and no stride loop: the
// grid is the result.  Otherwise a lane produces one result texel from its eight clamped source texels.
// r[row][0 .. 7]: the 32 bytes of the four rows; o[0 .. 3]: the 16 result bytes
template <int KIND, int CH>
__device__ __forceinline__ void reduce_chunk(const uint32_t (&r)[4][8], uint32_t (&o)[4]) {
    if constexpr (KIND == K_F32) {
        if (CH == 1) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                double s[4];
#pragma unroll
                for (int j = 0; j < 4; j++) s[j] = (double)__uint_as_float(r[j][2 * k]) + (double)__uint_as_float(r[j][2 * k + 1]);
                o[k] = __float_as_uint((float)(((s[0] + s[1]) + (s[2] + s[3])) * 0.125));
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {                       // result dword k: texel k / 2, channel k % 2
                const int a = 4 * (k >> 1) + (k & 1);
                double s[4];
#pragma unroll
                for (int j = 0; j < 4; j++) s[j] = (double)__uint_as_float(r[j][a]) + (double)__uint_as_float(r[j][a + 2]);
                o[k] = __float_as_uint((float)(((s[0] + s[1]) + (s[2] + s[3])) * 0.125));
            }
        }
    } else if constexpr (KindTraits<KIND>::BYTES == 1) {
        constexpr uint32_t FLIP = KIND == K_S8 ? 0x80808080u : 0u;
        uint32_t e[8], d[8];                                    // sums over the four rows of the even and of the odd bytes, 16-bit lanes
#pragma unroll
        for (int i = 0; i < 8; i++) {
            e[i] = 0u; d[i] = 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t w = r[j][i] ^ FLIP;
                uint32_t ev = w & 0x00ff00ffu, od = (w >> 8) & 0x00ff00ffu;
                if (KIND == K_S8) { ev = pk_max_u16(ev, 0x00010001u); od = pk_max_u16(od, 0x00010001u); }
                e[i] += ev; d[i] += od;
            }
        }
        if (CH == 1) {                                          // bytes b0 b1 b2 b3: (b0 + b1, b2 + b3) = even + odd
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t a = ((e[2 * k] + d[2 * k] + 0x00040004u) >> 3) & 0x00ff00ffu, b = ((e[2 * k + 1] + d[2 * k + 1] + 0x00040004u) >> 3) & 0x00ff00ffu;
                o[k] = ((a & 255u) | ((a >> 8) & 0xff00u) | ((b & 255u) << 16) | ((b >> 16) << 24)) ^ FLIP;
            }
        } else {                                                // bytes r0 g0 r1 g1: r0 + r1 = the two lanes of even, g0 + g1 of odd
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint32_t t[2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const uint32_t rr = ((e[2 * k + h] & 65535u) + (e[2 * k + h] >> 16) + 4u) >> 3, gg = ((d[2 * k + h] & 65535u) + (d[2 * k + h] >> 16) + 4u) >> 3;
                    t[h] = rr | (gg << 8);
                }
                o[k] = (t[0] | (t[1] << 16)) ^ FLIP;
            }
        }
    } else {
        constexpr uint32_t FLIP = KIND == K_S16 ? 0x80008000u : 0u;
        uint32_t lo[8], hi[8];                                  // sums over the four rows of the low and of the high halves
#pragma unroll
        for (int i = 0; i < 8; i++) {
            lo[i] = 0u; hi[i] = 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t w = r[j][i] ^ FLIP;
                if (KIND == K_S16) w = pk_max_u16(w, 0x00010001u);
                lo[i] += w & 65535u; hi[i] += w >> 16;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t a, b;
            if (CH == 1) { a = (lo[2 * k] + hi[2 * k] + 4u) >> 3; b = (lo[2 * k + 1] + hi[2 * k + 1] + 4u) >> 3; }      // dword = texels t0 t1
            else { a = (lo[2 * k] + lo[2 * k + 1] + 4u) >> 3; b = (hi[2 * k] + hi[2 * k + 1] + 4u) >> 3; }             // dword = (r, g)
            o[k] = (a | (b << 16)) ^ FLIP;
        }
    }
}
// one stored channel as the contract sums it: u (integers) or the double (floats)
template <int KIND>
__device__ __forceinline__ auto channel_at(const void *src, size_t i) {
    if constexpr (KIND == K_F32) return (double)reinterpret_cast<const float *>(src)[i];
    else if constexpr (KIND == K_U8) return (uint32_t)reinterpret_cast<const uint8_t *>(src)[i];
    else if constexpr (KIND == K_S8) return max((uint32_t)reinterpret_cast<const uint8_t *>(src)[i] ^ 0x80u, 1u);
    else if constexpr (KIND == K_U16) return (uint32_t)reinterpret_cast<const uint16_t *>(src)[i];
    else return max((uint32_t)reinterpret_cast<const uint16_t *>(src)[i] ^ 0x8000u, 1u);
}
struct ReduceDims { int nx, ny, nz, NX, NY, NZ; uint32_t chunks_per_row; };

template <int KIND, int CH, bool ALIGNED>
__global__ __launch_bounds__(256) void k_reduce(const void *__restrict__ src, void *__restrict__ dst, ReduceDims p, size_t count) {
    const size_t g = (size_t)blockIdx.x * 256u + threadIdx.x;                  // chunk (ALIGNED) or result texel
    if (g >= count) return;
    if constexpr (ALIGNED) {
        const uint32_t g32 = (uint32_t)g;                                       // (the host refuses 2^32 chunks and more)
        const uint32_t row = g32 / p.chunks_per_row, cx = g32 - row * p.chunks_per_row;
        const uint32_t Z = row / (uint32_t)p.NY, Y = row - Z * (uint32_t)p.NY;
        const size_t y0 = 2u * Y, y1 = min(2u * Y + 1u, (uint32_t)p.ny - 1u), z0 = 2u * Z, z1 = min(2u * Z + 1u, (uint32_t)p.nz - 1u);
        const size_t vecs_per_row = (size_t)p.chunks_per_row * 2;               // 16-byte vectors in a source row
        const uint4 *s = reinterpret_cast<const uint4 *>(src);
        const size_t rows[4] = { z0 * (size_t)p.ny + y0, z0 * (size_t)p.ny + y1, z1 * (size_t)p.ny + y0, z1 * (size_t)p.ny + y1 };
        uint32_t r[4][8];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint4 a = s[rows[j] * vecs_per_row + 2 * (size_t)cx], b = s[rows[j] * vecs_per_row + 2 * (size_t)cx + 1];
            r[j][0] = a.x; r[j][1] = a.y; r[j][2] = a.z; r[j][3] = a.w; r[j][4] = b.x; r[j][5] = b.y; r[j][6] = b.z; r[j][7] = b.w;
        }
        uint32_t o[4];
        reduce_chunk<KIND, CH>(r, o);
        reinterpret_cast<uint4 *>(dst)[g] = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        const size_t X = g % (size_t)p.NX, t = g / (size_t)p.NX, Y = t % (size_t)p.NY, Z = t / (size_t)p.NY;
        const size_t xs[2] = { 2 * X, 2 * X + 1 < (size_t)p.nx ? 2 * X + 1 : 2 * X }, ys[2] = { 2 * Y, 2 * Y + 1 < (size_t)p.ny ? 2 * Y + 1 : 2 * Y },
                     zs[2] = { 2 * Z, 2 * Z + 1 < (size_t)p.nz ? 2 * Z + 1 : 2 * Z };
#pragma unroll
        for (int c = 0; c < CH; c++) {
            decltype(channel_at<KIND>(src, 0)) a[8];
#pragma unroll
            for (int k = 0; k < 8; k++) a[k] = channel_at<KIND>(src, ((zs[k >> 2] * (size_t)p.ny + ys[(k >> 1) & 1]) * (size_t)p.nx + xs[k & 1]) * CH + c);
            const size_t oi = g * CH + c;
            if constexpr (KIND == K_F32) {
                reinterpret_cast<float *>(dst)[oi] = (float)((((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) * 0.125);
            } else {
                const uint32_t m = (a[0] + a[1] + a[2] + a[3] + a[4] + a[5] + a[6] + a[7] + 4u) >> 3;
                if (KindTraits<KIND>::BYTES == 1) reinterpret_cast<uint8_t *>(dst)[oi] = (uint8_t)(m ^ (KIND == K_S8 ? 0x80u : 0u));
                else reinterpret_cast<uint16_t *>(dst)[oi] = (uint16_t)(m ^ (KIND == K_S16 ? 0x8000u : 0u));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// binomial smoothing: k_smooth<T, ALIGNED>
// ---------------------------------------------------------------------------------------------
// k_gradient's form (vpt_volume_ops.hip): a workgroup of 256 threads (32 lanes along x, 4 voxels each, by 8 rows) owns an SM_TX x SM_TY
// column and marches SM_TZ planes along z.  Per plane it stages the tile and its one-voxel halo in LDS (indices clamped per axis), two
// buffers and one barrier per plane, and every thread reduces the 3 x 6 texels around its four voxels to C = smooth_x(smooth_y v)
// (smooth = (1, 2, 1); C <= 16 * 65535).  C is kept for three planes in registers and the third axis is applied across them:
//   out(z) = (C(z-1) + 2 C(z) + C(z+1) + 32) >> 6                        (one rounding per pass; W <= 64 * 65535 < 2^32)
// ALIGNED (nx % 4 == 0): tile rows are loaded and results stored as one dword (uint8) or qword (uint16) per lane.
#define SM_TX 128
#define SM_TY 8
#define SM_TZ 32
#define SM_ROW (SM_TX + 8)          // LDS row: texel x0 - 1 at [3], the tile at [4 .. 4 + SM_TX), texel x0 + SM_TX at [4 + SM_TX]

template <typename T> struct Quad;
template <> struct Quad<uint8_t> {
    typedef uint32_t vec_t;
    static __device__ __forceinline__ uint32_t get(vec_t w, int i) { return (w >> (8 * i)) & 255u; }
    static __device__ __forceinline__ vec_t pack(const uint32_t *v) { return v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24); }
};
template <> struct Quad<uint16_t> {
    typedef uint2 vec_t;
    static __device__ __forceinline__ uint32_t get(vec_t w, int i) { return ((i < 2 ? w.x : w.y) >> (16 * (i & 1))) & 65535u; }
    static __device__ __forceinline__ vec_t pack(const uint32_t *v) { return make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16)); }
};

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(256) void k_smooth(const T *__restrict__ src, T *__restrict__ dst, int nx, int ny, int nz) {
    typedef Quad<T> Q;
    typedef typename Q::vec_t vec_t;
    __shared__ __align__(16) T tile[2][SM_TY + 2][SM_ROW];
    const int lx = (int)threadIdx.x & 31, ly = (int)threadIdx.x >> 5;
    const int x0 = (int)blockIdx.x * SM_TX, xs = x0 + lx * 4;
    const int by0 = (int)blockIdx.y * SM_TY, y = by0 + ly;
    const int z0 = (int)blockIdx.z * SM_TZ, z1 = min(z0 + SM_TZ, nz);
    const bool whole = ALIGNED && xs + 3 < nx;            // (ALIGNED: a group of four is inside the volume or outside it as a whole)

    uint32_t prev[4] = {}, cur[4] = {};
    for (int zz = z0 - 1; zz <= z1; zz++) {
        const int k = (zz - z0 + 1) & 1;
        // ---- stage plane clamp(zz): rows by0 - 1 .. by0 + SM_TY, clamped; row r of the tile by the threads of row r % SM_TY
        const size_t plane = (size_t)min(max(zz, 0), nz - 1) * (size_t)ny;
        for (int r = ly; r < SM_TY + 2; r += SM_TY) {
            const int yy = min(max(by0 - 1 + r, 0), ny - 1);
            const T *row = src + (plane + (size_t)yy) * (size_t)nx;
            T *t = &tile[k][r][4 + lx * 4];
            if (whole) *reinterpret_cast<vec_t *>(t) = *reinterpret_cast<const vec_t *>(row + xs);
            else {
#pragma unroll
                for (int i = 0; i < 4; i++) t[i] = row[min(xs + i, nx - 1)];
            }
            if (lx == 0) tile[k][r][3] = row[max(x0 - 1, 0)];
            if (lx == 31) tile[k][r][4 + SM_TX] = row[min(x0 + SM_TX, nx - 1)];
        }
        __syncthreads();      // (two buffers: the plane staged next was last read before this barrier)
        // ---- s[i] = smooth_y of texel column xs - 1 + i, then C = smooth_x of those
        uint32_t s[6] = {};
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const T *t = &tile[k][ly + j][4 + lx * 4];
            const vec_t w = *reinterpret_cast<const vec_t *>(t);
            const uint32_t m = j == 1 ? 2u : 1u;
            s[0] += m * (uint32_t)t[-1];
#pragma unroll
            for (int i = 0; i < 4; i++) s[1 + i] += m * Q::get(w, i);
            s[5] += m * (uint32_t)t[4];
        }
        uint32_t nxt[4];
#pragma unroll
        for (int i = 0; i < 4; i++) nxt[i] = s[i] + 2u * s[i + 1] + s[i + 2];
        // ---- plane z = zz - 1 is complete once its upper neighbour is known
        if (zz > z0 && y < ny && xs < nx) {
            uint32_t v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = (prev[i] + 2u * cur[i] + nxt[i] + 32u) >> 6;
            const size_t o = ((size_t)(zz - 1) * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)xs;
            if (whole) *reinterpret_cast<vec_t *>(dst + o) = Q::pack(v);
            else {
                for (int i = 0; i < 4 && xs + i < nx; i++) dst[o + i] = (T)v[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) { prev[i] = cur[i]; cur[i] = nxt[i]; }
    }
}

// ---------------------------------------------------------------------------------------------
// hosts
// ---------------------------------------------------------------------------------------------
template <int KIND, int CH>
static int launch_reduce(const vpt_volume *src, vpt_volume *dst) {
    ReduceDims p = { src->nx, src->ny, src->nz, dst->nx, dst->ny, dst->nz, 0u };
    const size_t row_bytes = (size_t)src->nx * (size_t)src->vox_bytes;
    hipStream_t st = src->ctx->stream;
    const void *s = (const void *)src->linear.get(); void *d = (void *)dst->linear.get();
    const bool aligned = row_bytes % 32 == 0;
    const size_t count = aligned ? row_bytes / 32 * (size_t)dst->ny * (size_t)dst->nz : (size_t)dst->nx * dst->ny * dst->nz;
    const size_t blocks = (count + 255) / 256;
    if ((aligned && count > 0xffffffffull) || blocks > 0x7fffffffull) return fail(VPT_ERR_UNSUPPORTED, "volume too large");
    if (aligned) {
        p.chunks_per_row = (uint32_t)(row_bytes / 32);
        hipLaunchKernelGGL((k_reduce<KIND, CH, true>), dim3((unsigned)blocks), dim3(256), 0, st, s, d, p, count);
    } else hipLaunchKernelGGL((k_reduce<KIND, CH, false>), dim3((unsigned)blocks), dim3(256), 0, st, s, d, p, count);
    return VPT_OK;
}
template <int KIND>
static int launch_reduce_channels(const vpt_volume *src, vpt_volume *dst) {
    return src->channels == 2 ? launch_reduce<KIND, 2>(src, dst) : launch_reduce<KIND, 1>(src, dst);
}

extern "C" int vpt_volume_reduce(vpt_volume *src, vpt_volume **out) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    const VolumeFormat *f = volume_format(src->format);
    if (!f || f->packed_bytes)
        return fail(VPT_ERR_UNSUPPORTED, "a volume is reduced in its own format, which a packed format's decoded storage does not have: %s", format_name(src->format));
    vpt_context *c = src->ctx;
    HIP_TRY(hipSetDevice(c->device));
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(c, (src->nx + 1) / 2, (src->ny + 1) / 2, (src->nz + 1) / 2, src->format, false, &d));   // every texel is written below
    int rc;
    if (f->is_float) rc = launch_reduce_channels<K_F32>(src, d);
    else if (f->bytes == 2) rc = f->is_signed ? launch_reduce_channels<K_S16>(src, d) : launch_reduce_channels<K_U16>(src, d);
    else rc = f->is_signed ? launch_reduce_channels<K_S8>(src, d) : launch_reduce_channels<K_U8>(src, d);
    if (rc != VPT_OK) { vpt_volume_destroy(d); return rc; }
    return volume_finish_derived(src->ctx, src->filter, d, out);
}

template <typename T>
static void launch_smooth(const vpt_volume *v, const T *s, T *d) {
    const dim3 grid((unsigned)((v->nx + SM_TX - 1) / SM_TX), (unsigned)((v->ny + SM_TY - 1) / SM_TY), (unsigned)((v->nz + SM_TZ - 1) / SM_TZ));
    if (v->nx % 4 == 0) hipLaunchKernelGGL((k_smooth<T, true>), grid, dim3(256), 0, v->ctx->stream, s, d, v->nx, v->ny, v->nz);
    else hipLaunchKernelGGL((k_smooth<T, false>), grid, dim3(256), 0, v->ctx->stream, s, d, v->nx, v->ny, v->nz);
}

extern "C" int vpt_volume_smooth(vpt_volume *src, int passes, vpt_volume **out) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (src->format != VPT_FORMAT_R8 && src->format != VPT_FORMAT_R16)
        return fail(VPT_ERR_UNSUPPORTED, "volumes are smoothed in front of the gradient, which is derived from one-channel unsigned normalised volumes (R8, R16), not from %s",
                    format_name(src->format));
    if (passes < 1 || passes > 8) return fail(VPT_ERR_INVALID, "%d smoothing passes: 1 to 8 are taken", passes);
    vpt_context *c = src->ctx;
    HIP_TRY(hipSetDevice(c->device));
    if ((src->ny + SM_TY - 1) / SM_TY > 65535 || (src->nz + SM_TZ - 1) / SM_TZ > 65535) return fail(VPT_ERR_UNSUPPORTED, "volume too large");
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(c, src->nx, src->ny, src->nz, src->format, false, &d));   // every texel is written by the last pass
    DevBuf<uint8_t> scratch;                                 // several passes go to and fro between the result's storage and this
    if (passes > 1) {
        hipError_t e = scratch.alloc((size_t)src->nx * src->ny * src->nz * (size_t)src->vox_bytes);
        if (e != hipSuccess) { vpt_volume_destroy(d); return fail(VPT_ERR_HIP, "smoothing scratch: %s", hipGetErrorString(e)); }
    }
    const uint8_t *from = src->linear.get();
    for (int i = 1; i <= passes; i++) {
        uint8_t *to = (passes - i) % 2 == 0 ? d->linear.get() : scratch.get();      // the last pass writes the result
        if (src->norm16) launch_smooth<uint16_t>(src, (const uint16_t *)from, (uint16_t *)to);
        else launch_smooth<uint8_t>(src, (const uint8_t *)from, (uint8_t *)to);
        from = to;
    }
    const int rc = volume_finish_derived(src->ctx, src->filter, d, out);
    if (passes > 1) (void)hipStreamSynchronize(c->stream);   // the scratch is freed on return: its last reader has finished
    return rc;
}
