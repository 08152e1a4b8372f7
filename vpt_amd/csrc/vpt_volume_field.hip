// vpt_volume_field.hip — what the voxel fields share behind their builders (vpt_volume_field.h): the capture of the source, the read-back
// of a box of values, the select emitter and the destroy.  The callers (vpt_volume_components.hip, vpt_volume_distance.hip) check their own
// arguments; kernel forms and compiler figures: DESIGN.md "Connected components", "Distance transform".
#include "vpt_volume_field.h"

template <typename T>
__global__ __launch_bounds__(256) void k_select(const T *__restrict__ src, const uint32_t *__restrict__ values, T *__restrict__ dst, size_t n,
                                               uint32_t lo, uint32_t hi, uint32_t fill) {
    typedef Four<T> F;
    const size_t quads = n / 4, stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t q = t0; q < quads; q += stride) {
        const typename F::in_t w = reinterpret_cast<const typename F::in_t *>(src)[q];
        const uint4 r = reinterpret_cast<const uint4 *>(values)[q];
        const uint32_t d[4] = { r.x, r.y, r.z, r.w };
        uint32_t v[4];
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = (d[i] >= lo && d[i] <= hi) ? F::get(w, i) : fill;
        reinterpret_cast<typename F::in_t *>(dst)[q] = F::pack(v);
    }
    for (size_t i = quads * 4 + t0; i < n; i += stride) { const uint32_t d = values[i]; dst[i] = (d >= lo && d <= hi) ? src[i] : (T)fill; }
}
__global__ __launch_bounds__(256) void k_read_field(const uint32_t *__restrict__ values, int nx, int ny, uint32_t *__restrict__ blk, int x0, int y0, int z0,
                                                   int bw, int bh, size_t texels) {
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < texels; t += (size_t)gridDim.x * 256) {
        const int x = (int)(t % (size_t)bw); const size_t r = t / (size_t)bw; const int y = (int)(r % (size_t)bh), z = (int)(r / (size_t)bh);
        blk[t] = values[((size_t)(z0 + z) * (size_t)ny + (size_t)(y0 + y)) * (size_t)nx + (size_t)(x0 + x)];
    }
}

int field_describe(VoxelField *f, const vpt_volume *src, int format) {
    f->ctx = src->ctx; f->nx = src->nx; f->ny = src->ny; f->nz = src->nz; f->format = format; f->filter = src->filter; f->norm16 = src->norm16;
    const size_t n = f->voxels();
    HIP_TRY(f->texels.alloc(n * (size_t)(src->norm16 ? 2 : 1)));
    HIP_TRY(f->values.alloc(n));
    return VPT_OK;
}

int field_capture(VoxelField *f, const vpt_volume *src) {
    VPT_TRY(field_describe(f, src, src->format));
    const size_t bytes = f->voxels() * (size_t)src->vox_bytes;         // one channel: what field_describe allocated
    HIP_TRY(hipMemcpyAsync(f->texels, src->linear, bytes, hipMemcpyDeviceToDevice, f->ctx->stream));     // behind any upload into src
    return VPT_OK;
}

int field_read(VoxelField *f, int x, int y, int z, int w, int h, int d, uint32_t *host_dst, size_t nbytes) {
    if (!f || !host_dst) return fail(VPT_ERR_INVALID, "null argument");
    if (w < 1 || h < 1 || d < 1 || x < 0 || y < 0 || z < 0 || x + w > f->nx || y + h > f->ny || z + d > f->nz)
        return fail(VPT_ERR_INVALID, "block (%d,%d,%d)+(%d,%d,%d) outside volume %dx%dx%d", x, y, z, w, h, d, f->nx, f->ny, f->nz);
    const size_t texels = (size_t)w * h * d, need = texels * sizeof(uint32_t);
    if (nbytes < need) return fail(VPT_ERR_INVALID, "block buffer too short: %zu < %zu", nbytes, need);
    hipStream_t st = f->ctx->stream;
    HIP_TRY(hipSetDevice(f->ctx->device));
    if (x == 0 && y == 0 && w == f->nx && h == f->ny) {        // a run of whole z-slices is contiguous
        HIP_TRY(hipMemcpyAsync(host_dst, f->values + (size_t)z * f->nx * f->ny, need, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return VPT_OK;
    }
    DevBuf<uint32_t> block;
    HIP_TRY(block.alloc(texels));
    hipLaunchKernelGGL(k_read_field, dim3(stream_grid(texels)), dim3(256), 0, st, (const uint32_t *)f->values.get(), f->nx, f->ny, block.get(), x, y, z, w, h, texels);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_dst, block, need, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return VPT_OK;
}

int field_select(VoxelField *f, uint32_t lo, uint32_t hi, uint32_t fill, vpt_volume **out) {
    const uint32_t M = f->norm16 ? 65535u : 255u;
    if (fill > M) return fail(VPT_ERR_INVALID, "fill %u: the largest code of %s is %u", fill, format_name(f->format), M);
    HIP_TRY(hipSetDevice(f->ctx->device));
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(f->ctx, f->nx, f->ny, f->nz, f->format, false, &d));      // every texel is written below
    const size_t n = f->voxels();
    const dim3 grid(stream_grid(n / 4 + 1));
    if (f->norm16) hipLaunchKernelGGL(k_select<uint16_t>, grid, dim3(256), 0, f->ctx->stream, (const uint16_t *)f->texels.get(), (const uint32_t *)f->values.get(), (uint16_t *)d->linear.get(), n, lo, hi, fill);
    else hipLaunchKernelGGL(k_select<uint8_t>, grid, dim3(256), 0, f->ctx->stream, (const uint8_t *)f->texels.get(), (const uint32_t *)f->values.get(), d->linear.get(), n, lo, hi, fill);
    return volume_finish_derived(f->ctx, f->filter, d, out);
}

int field_destroy(VoxelField *f) {
    if (!f) return fail(VPT_ERR_INVALID, "null argument");
    (void)hipSetDevice(f->ctx->device);
    (void)hipStreamSynchronize(f->ctx->stream);      // an emitter may still read the buffers
    delete f;
    return VPT_OK;
}
