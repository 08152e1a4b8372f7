// vpt_volume_ops.hip — volume operations on the device: the gradient-magnitude channel (vpt_volume_derive_gradient), texel read-back
// (vpt_volume_read_block) and value / value x gradient histograms (vpt_volume_histogram).  C-ABI and the integer contract of the
// gradient: include/vpt.h; kernel form and measurements: DESIGN.md "Gradient-magnitude channel".
#include "vpt_internal.h"

// ---------------------------------------------------------------------------------------------
// gradient magnitude: k_gradient<T, OP, ALIGNED>
// ---------------------------------------------------------------------------------------------
// A workgroup of 256 threads (32 lanes along x, 4 voxels each, by 8 rows) owns a GR_TX x GR_TY column of the volume and marches
// GR_TZ planes along z.  Per plane it stages the (GR_TX + 2) x (GR_TY + 2) texels of the plane's tile and one-voxel halo in LDS
// (indices clamped per axis: CLAMP_TO_EDGE), and every thread reduces the 3 x 6 texels around its four voxels to three in-plane
// quantities per voxel:
//   SOBEL:   A = smooth_y(diff_x v), B = smooth_x(diff_y v), C = smooth_x(smooth_y v)   (smooth = (1, 2, 1), diff = v(+1) - v(-1))
//   CENTRAL: A = diff_x v,           B = diff_y v,           C = v
// which are kept in registers for three planes; the third axis is applied across them:
//   SOBEL:   dx = A(z-1) + 2 A(z) + A(z+1), dy = B(z-1) + 2 B(z) + B(z+1), dz = C(z+1) - C(z-1)
//   CENTRAL: dx = A(z), dy = B(z), dz = C(z+1) - C(z-1)
// so the 3 x 3 x 3 Sobel costs the (1, 2, 1) sums once, not 3 x 18 taps.  Reads per source texel: (GR_TX + 2) / GR_TX x (GR_TY + 2) / GR_TY
// x (GR_TZ + 2) / GR_TZ = 1.016 x 1.25 x 1.0625 = 1.35 (the halo rows and planes are a neighbouring workgroup's tile: L2 traffic mostly).
// ALIGNED (nx % 4 == 0): the tile rows are loaded, and the interleaved (value, G) texels stored, as one dword (uint8) or qword
// (uint16) per lane and 8 / 16 bytes per lane, contiguous per half-wave along x; otherwise texel by texel.
#define GR_TX 128
#define GR_TY 8
#define GR_TZ 32
#define GR_ROW (GR_TX + 8)          // LDS row: texel x0 - 1 at [3], the tile at [4 .. 4 + GR_TX), texel x0 + GR_TX at [4 + GR_TX]

template <typename T> struct Texel4;
template <> struct Texel4<uint8_t> {
    typedef uint32_t in_t; typedef uint2 out_t;
    static __device__ __forceinline__ int get(in_t w, int i) { return (int)((w >> (8 * i)) & 255u); }
    static __device__ __forceinline__ in_t splat(uint32_t v) { return v * 0x01010101u; }
    static __device__ __forceinline__ out_t pack(in_t w, const uint32_t *g) {
        return make_uint2((w & 255u) | (g[0] << 8) | (((w >> 8) & 255u) << 16) | (g[1] << 24),
                          ((w >> 16) & 255u) | (g[2] << 8) | ((w >> 24) << 16) | (g[3] << 24));
    }
};
template <> struct Texel4<uint16_t> {
    typedef uint2 in_t; typedef uint4 out_t;
    static __device__ __forceinline__ int get(in_t w, int i) { return (int)(((i < 2 ? w.x : w.y) >> (16 * (i & 1))) & 65535u); }
    static __device__ __forceinline__ in_t splat(uint32_t v) { return make_uint2(v * 0x00010001u, v * 0x00010001u); }
    static __device__ __forceinline__ out_t pack(in_t w, const uint32_t *g) {
        return make_uint4((w.x & 65535u) | (g[0] << 16), (w.x >> 16) | (g[1] << 16), (w.y & 65535u) | (g[2] << 16), (w.y >> 16) | (g[3] << 16));
    }
};
// floor(sqrt(t)), exact: the float estimate is within one of it (t < 2^32: the conversion and the correctly rounded square root are each
// off by 2^-24 relative at most, 0.006 at the largest root), one integer step corrects it
__device__ __forceinline__ uint32_t isqrt32(uint32_t t) {
    uint32_t r = (uint32_t)sqrtf((float)t);
    if (r > 65535u) r = 65535u;
    if ((uint64_t)r * r > (uint64_t)t) r--;
    else if ((uint64_t)(r + 1u) * (r + 1u) <= (uint64_t)t) r++;
    return r;
}
struct GradPlane { int a[4], b[4], c[4]; };

template <typename T, int OP, bool ALIGNED>
__global__ __launch_bounds__(256) void k_gradient(const T *__restrict__ src, T *__restrict__ dst, int nx, int ny, int nz, unsigned long long q) {
    typedef Texel4<T> X;
    typedef typename X::in_t in_t;
    typedef typename X::out_t out_t;
    constexpr int B = (int)sizeof(T) * 8;
    constexpr int SHIFT = OP == VPT_GRADIENT_SOBEL ? 24 : 16;
    __shared__ __align__(16) T tile[2][GR_TY + 2][GR_ROW];
    const int lx = (int)threadIdx.x & 31, ly = (int)threadIdx.x >> 5;
    const int x0 = (int)blockIdx.x * GR_TX, xs = x0 + lx * 4;
    const int by0 = (int)blockIdx.y * GR_TY, y = by0 + ly;
    const int z0 = (int)blockIdx.z * GR_TZ, z1 = min(z0 + GR_TZ, nz);
    const bool whole = ALIGNED && xs + 3 < nx;            // (ALIGNED: a group of four is inside the volume or outside it as a whole)

    GradPlane prev = {}, cur = {};
    in_t vcur = X::splat(0u);
    for (int zz = z0 - 1; zz <= z1; zz++) {
        const int k = (zz - z0 + 1) & 1;
        // ---- stage plane clamp(zz): rows by0 - 1 .. by0 + GR_TY, clamped; row r of the tile by the threads of row r % GR_TY
        const size_t plane = (size_t)min(max(zz, 0), nz - 1) * (size_t)ny;
        for (int r = ly; r < GR_TY + 2; r += GR_TY) {
            const int yy = min(max(by0 - 1 + r, 0), ny - 1);
            const T *row = src + (plane + (size_t)yy) * (size_t)nx;
            T *t = &tile[k][r][4 + lx * 4];
            if (whole) *reinterpret_cast<in_t *>(t) = *reinterpret_cast<const in_t *>(row + xs);
            else {
#pragma unroll
                for (int i = 0; i < 4; i++) t[i] = row[min(xs + i, nx - 1)];
            }
            if (lx == 0) tile[k][r][3] = row[max(x0 - 1, 0)];
            if (lx == 31) tile[k][r][4 + GR_TX] = row[min(x0 + GR_TX, nx - 1)];
        }
        __syncthreads();      // (two buffers: the plane staged next was last read before this barrier)
        // ---- the in-plane quantities of this thread's four voxels: e[j][0..5] = texels xs - 1 .. xs + 4 of rows y - 1, y, y + 1
        int e[3][6];
        in_t own = X::splat(0u);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const T *t = &tile[k][ly + j][4 + lx * 4];
            const in_t w = *reinterpret_cast<const in_t *>(t);
            if (j == 1) own = w;
            e[j][0] = (int)t[-1];
#pragma unroll
            for (int i = 0; i < 4; i++) e[j][1 + i] = X::get(w, i);
            e[j][5] = (int)t[4];
        }
        GradPlane nxt;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            if (OP == VPT_GRADIENT_SOBEL) {
                const int s0 = e[0][i] + 2 * e[0][i + 1] + e[0][i + 2], s1 = e[1][i] + 2 * e[1][i + 1] + e[1][i + 2], s2 = e[2][i] + 2 * e[2][i + 1] + e[2][i + 2];
                nxt.a[i] = (e[0][i + 2] - e[0][i]) + 2 * (e[1][i + 2] - e[1][i]) + (e[2][i + 2] - e[2][i]);
                nxt.b[i] = s2 - s0;
                nxt.c[i] = s0 + 2 * s1 + s2;
            } else {
                nxt.a[i] = e[1][i + 2] - e[1][i];
                nxt.b[i] = e[2][i + 1] - e[0][i + 1];
                nxt.c[i] = e[1][i + 1];
            }
        }
        // ---- plane z = zz - 1 is complete once its upper neighbour is known
        if (zz > z0 && y < ny && xs < nx) {
            uint32_t g[4];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int dx = OP == VPT_GRADIENT_SOBEL ? prev.a[i] + 2 * cur.a[i] + nxt.a[i] : cur.a[i];
                const int dy = OP == VPT_GRADIENT_SOBEL ? prev.b[i] + 2 * cur.b[i] + nxt.b[i] : cur.b[i];
                const int dz = nxt.c[i] - prev.c[i];
                unsigned long long s;
                if (B == 8) s = (unsigned long long)(uint32_t)(dx * dx + dy * dy + dz * dz);          // <= 3 (16 * 255)^2 < 2^26
                else s = (unsigned long long)((long long)dx * dx) + (unsigned long long)((long long)dy * dy) + (unsigned long long)((long long)dz * dz);
                const unsigned long long tq = (s * q) >> SHIFT;                                         // < 2^64: include/vpt.h
                g[i] = (tq >> (2 * B)) != 0ull ? (1u << B) - 1u : isqrt32((uint32_t)tq);
            }
            const size_t o = (((size_t)(zz - 1) * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)xs) * 2;
            if (whole) *reinterpret_cast<out_t *>(dst + o) = X::pack(vcur, g);
            else {
                for (int i = 0; i < 4 && xs + i < nx; i++) { dst[o + 2 * i] = (T)X::get(vcur, i); dst[o + 2 * i + 1] = (T)g[i]; }
            }
        }
        prev = cur; cur = nxt; vcur = own;
    }
}

// ---------------------------------------------------------------------------------------------
// histograms
// ---------------------------------------------------------------------------------------------
// Counts are integers: atomic adds in any order give the same bins.  Smooth volumes put most voxels into few bins, so a workgroup counts
// in LDS and touches global memory once per non-empty bin at its end.
// One channel: 256 bins of the texel's top 8 bits, one private copy per wave.
template <typename T>
__global__ __launch_bounds__(256) void k_histogram(const T *__restrict__ v, size_t n, uint32_t *__restrict__ bins) {
    __shared__ uint32_t h[4][256];
    const int tid = (int)threadIdx.x, wave = tid >> 6;
    for (int i = 0; i < 4; i++) h[i][tid] = 0u;
    __syncthreads();
    constexpr int PER = 16 / (int)sizeof(T), SH = (int)sizeof(T) * 8 - 8;
    const size_t nvec = n / PER, stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + tid;
    for (size_t i = first; i < nvec; i += stride) {
        const uint4 w = reinterpret_cast<const uint4 *>(v)[i];
        const uint32_t d[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (sizeof(T) == 1) {
#pragma unroll
                for (int b = 0; b < 4; b++) atomicAdd(&h[wave][(d[j] >> (8 * b)) & 255u], 1u);
            } else {
                atomicAdd(&h[wave][(d[j] >> 8) & 255u], 1u);
                atomicAdd(&h[wave][d[j] >> 24], 1u);
            }
        }
    }
    for (size_t i = nvec * PER + first; i < n; i += stride) atomicAdd(&h[wave][(uint32_t)v[i] >> SH], 1u);
    __syncthreads();
    const uint32_t sum = h[0][tid] + h[1][tid] + h[2][tid] + h[3][tid];
    if (sum) atomicAdd(&bins[tid], sum);
}
// Two channels: bins[g * 256 + v] of both channels' top 8 bits.  The 256 KiB table does not fit LDS; the rows g < HIST_SLAB_ROWS, where a
// gradient channel has most of its voxels, are counted in an LDS slab (32 KiB: four workgroups per CU), the rest by global atomics.
#define HIST_SLAB_ROWS 32
template <typename T>
__global__ __launch_bounds__(256) void k_histogram_rg(const T *__restrict__ v, size_t nvox, uint32_t *__restrict__ bins) {
    __shared__ uint32_t h[HIST_SLAB_ROWS * 256];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < HIST_SLAB_ROWS * 256; i += 256) h[i] = 0u;
    __syncthreads();
    auto count = [&](uint32_t val, uint32_t g) {
        const uint32_t bin = g * 256u + val;
        if (g < (uint32_t)HIST_SLAB_ROWS) atomicAdd(&h[bin], 1u);
        else atomicAdd(&bins[bin], 1u);
    };
    constexpr int PER = 8 / (int)sizeof(T);                // voxels per 16-byte load
    const size_t nvec = nvox / PER, stride = (size_t)gridDim.x * blockDim.x, first = (size_t)blockIdx.x * blockDim.x + tid;
    for (size_t i = first; i < nvec; i += stride) {
        const uint4 w = reinterpret_cast<const uint4 *>(v)[i];
        const uint32_t d[4] = { w.x, w.y, w.z, w.w };
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (sizeof(T) == 1) { count(d[j] & 255u, (d[j] >> 8) & 255u); count((d[j] >> 16) & 255u, d[j] >> 24); }
            else count((d[j] >> 8) & 255u, d[j] >> 24);
        }
    }
    constexpr int SH = (int)sizeof(T) * 8 - 8;
    for (size_t i = nvec * PER + first; i < nvox; i += stride) count((uint32_t)v[2 * i] >> SH, (uint32_t)v[2 * i + 1] >> SH);
    __syncthreads();
    for (int i = tid; i < HIST_SLAB_ROWS * 256; i += 256) { const uint32_t c = h[i]; if (c) atomicAdd(&bins[i], c); }
}

// ---------------------------------------------------------------------------------------------
// read-back: the inverse of k_blit_block (a box of the linear storage, texel by texel, into a dense block)
// ---------------------------------------------------------------------------------------------
__global__ void k_read_block(const uint8_t *__restrict__ vol, int nx, int ny, uint8_t *__restrict__ blk, int x0, int y0, int z0, int bw, int bh, int bd, int ch) {
    const size_t n = (size_t)bw * bh * bd;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(t % bw); const size_t r = t / bw; const int y = (int)(r % bh); const int z = (int)(r / bh);
        const size_t s = (((size_t)(z0 + z) * ny + (y0 + y)) * nx + (x0 + x)) * ch;
        for (int c = 0; c < ch; c++) blk[t * ch + c] = vol[s + c];
    }
}

// ---------------------------------------------------------------------------------------------
// hosts
// ---------------------------------------------------------------------------------------------
template <typename T>
static void launch_gradient(const vpt_volume *src, vpt_volume *dst, int op, unsigned long long q) {
    const dim3 grid((unsigned)((src->nx + GR_TX - 1) / GR_TX), (unsigned)((src->ny + GR_TY - 1) / GR_TY), (unsigned)((src->nz + GR_TZ - 1) / GR_TZ));
    const T *s = (const T *)src->linear.get(); T *d = (T *)dst->linear.get();
    hipStream_t st = src->ctx->stream;
    const bool aligned = src->nx % 4 == 0;
    if (op == VPT_GRADIENT_SOBEL) {
        if (aligned) hipLaunchKernelGGL((k_gradient<T, VPT_GRADIENT_SOBEL, true>), grid, dim3(256), 0, st, s, d, src->nx, src->ny, src->nz, q);
        else hipLaunchKernelGGL((k_gradient<T, VPT_GRADIENT_SOBEL, false>), grid, dim3(256), 0, st, s, d, src->nx, src->ny, src->nz, q);
    } else {
        if (aligned) hipLaunchKernelGGL((k_gradient<T, VPT_GRADIENT_CENTRAL, true>), grid, dim3(256), 0, st, s, d, src->nx, src->ny, src->nz, q);
        else hipLaunchKernelGGL((k_gradient<T, VPT_GRADIENT_CENTRAL, false>), grid, dim3(256), 0, st, s, d, src->nx, src->ny, src->nz, q);
    }
}

extern "C" int vpt_volume_derive_gradient(vpt_volume *src, int op, float gain, vpt_volume **out) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (op != VPT_GRADIENT_CENTRAL && op != VPT_GRADIENT_SOBEL) return fail(VPT_ERR_INVALID, "unknown gradient operator %d", op);
    if (src->format != VPT_FORMAT_R8 && src->format != VPT_FORMAT_R16)
        return fail(VPT_ERR_UNSUPPORTED, "the gradient magnitude is derived from one-channel unsigned normalised volumes (R8, R16), not from %s",
                    format_name(src->format));
    const double qd = std::floor((double)gain * (double)gain * 16384.0 + 0.5);
    if (!(qd >= 1.0 && qd <= 4194304.0)) return fail(VPT_ERR_INVALID, "gradient gain %g: gain^2 * 16384 must round into [1, 4194304] (gains from 1/128 to 16)", (double)gain);
    vpt_context *c = src->ctx;
    HIP_TRY(hipSetDevice(c->device));
    if ((src->ny + GR_TY - 1) / GR_TY > 65535 || (src->nz + GR_TZ - 1) / GR_TZ > 65535) return fail(VPT_ERR_UNSUPPORTED, "volume too large");
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(c, src->nx, src->ny, src->nz, src->norm16 ? VPT_FORMAT_RG16 : VPT_FORMAT_RG8, false, &d));   // every texel is written below
    if (src->norm16) launch_gradient<uint16_t>(src, d, op, (unsigned long long)qd);
    else launch_gradient<uint8_t>(src, d, op, (unsigned long long)qd);
    return volume_finish_derived(src->ctx, src->filter, d, out);
}

extern "C" int vpt_volume_read_block(vpt_volume *v, int x, int y, int z, int w, int h, int d, void *host_dst, size_t nbytes) {
    if (!v || !host_dst) return fail(VPT_ERR_INVALID, "null argument");
    if (w < 1 || h < 1 || d < 1 || x < 0 || y < 0 || z < 0 || x + w > v->nx || y + h > v->ny || z + d > v->nz)
        return fail(VPT_ERR_INVALID, "block (%d,%d,%d)+(%d,%d,%d) outside volume %dx%dx%d", x, y, z, w, h, d, v->nx, v->ny, v->nz);
    const size_t texels = (size_t)w * h * d, need = texels * (size_t)v->vox_bytes;
    if (nbytes < need) return fail(VPT_ERR_INVALID, "block buffer too short: %zu < %zu", nbytes, need);
    vpt_context *c = v->ctx;
    HIP_TRY(hipSetDevice(c->device));
    if (x == 0 && y == 0 && w == v->nx && h == v->ny) {        // a run of whole z-slices is contiguous in the linear storage
        HIP_TRY(hipMemcpyAsync(host_dst, v->linear + (size_t)z * v->nx * v->ny * v->vox_bytes, need, hipMemcpyDeviceToHost, c->stream));
    } else {
        HIP_TRY(v->staging.reserve(need, c->stream));
        int grid = (int)((texels + 255) / 256); if (grid > 4096) grid = 4096;
        hipLaunchKernelGGL(k_read_block, dim3(grid), dim3(256), 0, c->stream, (const uint8_t *)v->linear.get(), v->nx, v->ny, v->staging, x, y, z, w, h, d, v->vox_bytes);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host_dst, v->staging, need, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VPT_OK;
}

extern "C" int vpt_volume_histogram(vpt_volume *v, uint32_t *bins, size_t nbins) {
    if (!v || !bins) return fail(VPT_ERR_INVALID, "null argument");
    const bool one = v->format == VPT_FORMAT_R8 || v->format == VPT_FORMAT_R16, two = v->format == VPT_FORMAT_RG8 || v->format == VPT_FORMAT_RG16;
    if (!one && !two) return fail(VPT_ERR_UNSUPPORTED, "histograms are counted for R8, R16, RG8 and RG16 volumes, not for %s", format_name(v->format));
    const size_t want = one ? 256 : 65536;
    if (nbins != want) return fail(VPT_ERR_INVALID, "a histogram of an %s volume has %zu bins, not %zu", format_name(v->format), want, nbins);
    const size_t nvox = (size_t)v->nx * v->ny * v->nz;
    if (nvox > 0xFFFFFFFFull) return fail(VPT_ERR_UNSUPPORTED, "histogram: %zu voxels exceed 2^32 - 1 (the bins are 32-bit)", nvox);
    vpt_context *c = v->ctx;
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<uint32_t> dev;
    HIP_TRY(dev.alloc(want));
    HIP_TRY(hipMemsetAsync(dev, 0, want * sizeof(uint32_t), c->stream));
    const size_t loads = nvox * (size_t)v->vox_bytes / 16 + 1;           // 16 bytes per thread and step
    unsigned grid = (unsigned)std::min<size_t>((loads + 255) / 256, one ? 2048 : 1024);
    if (one && v->norm16) hipLaunchKernelGGL(k_histogram<uint16_t>, dim3(grid), dim3(256), 0, c->stream, (const uint16_t *)v->linear.get(), nvox, dev.get());
    else if (one) hipLaunchKernelGGL(k_histogram<uint8_t>, dim3(grid), dim3(256), 0, c->stream, (const uint8_t *)v->linear.get(), nvox, dev.get());
    else if (v->norm16) hipLaunchKernelGGL(k_histogram_rg<uint16_t>, dim3(grid), dim3(256), 0, c->stream, (const uint16_t *)v->linear.get(), nvox, dev.get());
    else hipLaunchKernelGGL(k_histogram_rg<uint8_t>, dim3(grid), dim3(256), 0, c->stream, (const uint8_t *)v->linear.get(), nvox, dev.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(bins, dev, want * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VPT_OK;
}
