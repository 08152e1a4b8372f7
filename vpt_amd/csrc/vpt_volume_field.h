// vpt_volume_field.h — a voxel field: a snapshot of an R8 / R16 volume's linear texels plus one uint32 per voxel, and the four services every
// such pair offers (vpt_volume_field.hip): read a box of the values back, emit the volume that keeps the codes where lo <= value <= hi,
// emit the RG8 / RG16 volume (code, min(f(value), M)), destroy.  The units that build a field (vpt_volume_components.hip: the values are
// ranks; vpt_volume_distance.hip: squared distances) derive their handle from VoxelField and keep their builders, their argument checks and
// their info / list / profile payloads.  Kernel forms and compiler figures: DESIGN.md "Connected components", "Distance transform".
#pragma once
#include "vpt_internal.h"

struct VoxelField {
    vpt_context *ctx = nullptr;
    int nx = 0, ny = 0, nz = 0, format = 0, filter = VPT_FILTER_LINEAR;
    bool norm16 = false;
    DevBuf<uint8_t> texels;                 // the source's linear texels at the time of the call
    DevBuf<uint32_t> values;                // one value per voxel
    virtual ~VoxelField() = default;        // field_destroy deletes the unit's handle through this type
    size_t voxels() const { return (size_t)nx * (size_t)ny * (size_t)nz; }
};

// fills `f` from `src` but for the texels: context, dimensions, filter and channel width, `format` (R8 / R16: the snapshot's, one channel of
// src's width), and both buffers; the caller enqueues what fills the texels (vpt_volume_watershed.hip: one channel of a two-channel relief)
int field_describe(VoxelField *f, const vpt_volume *src, int format);
// fills `f` from the R8 / R16 volume `src` (the caller has checked it): dimensions, format and filter, both buffers, and the copy of src's
// texels on the context's stream, behind any upload into src
int field_capture(VoxelField *f, const vpt_volume *src);
// the values of the box (x, y, z) + (w, h, d) into host_dst
int field_read(VoxelField *f, int x, int y, int z, int w, int h, int d, uint32_t *host_dst, size_t nbytes);
// a new volume of the source's format: the source's code where lo <= value <= hi, `fill` elsewhere
int field_select(VoxelField *f, uint32_t lo, uint32_t hi, uint32_t fill, vpt_volume **out);
// waits for whatever still reads the buffers and deletes the handle
int field_destroy(VoxelField *f);

// ---------------------------------------------------------------------------------------------
// the emitters' texel access; the pair emitter k_pair<T, Map>
// ---------------------------------------------------------------------------------------------
// Plain gathers over the linear storage, four voxels a thread: the texels as one dword (uint8) or qword (uint16), the values as one uint4,
// the result as one vector store; the last n % 4 voxels one by one.  (Groups of four along the linear index are aligned whatever nx is.)
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
// (code, min(map(value), M)); Map: a device functor uint32 -> uint32, instantiated by the unit that owns it
template <typename T, typename Map>
__global__ __launch_bounds__(256) void k_pair(const T *__restrict__ src, const uint32_t *__restrict__ values, T *__restrict__ dst, size_t n, Map map) {
    typedef Four<T> F;
    constexpr uint32_t M = (1u << (8 * sizeof(T))) - 1u;
    const size_t quads = n / 4, stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t q = t0; q < quads; q += stride) {
        const typename F::in_t w = reinterpret_cast<const typename F::in_t *>(src)[q];
        const uint4 r = reinterpret_cast<const uint4 *>(values)[q];
        const uint32_t d[4] = { r.x, r.y, r.z, r.w };
        uint32_t v[4], g[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { v[i] = F::get(w, i); g[i] = min(map(d[i]), M); }
        reinterpret_cast<typename F::pair_t *>(dst)[q] = F::pack2(v, g);
    }
    for (size_t i = quads * 4 + t0; i < n; i += stride) { dst[2 * i] = src[i]; dst[2 * i + 1] = (T)min(map(values[i]), M); }
}

// a new RG8 / RG16 volume with the source's filter: (code, min(map(value), M))
template <typename Map>
static int field_pair(VoxelField *f, Map map, vpt_volume **out) {
    HIP_TRY(hipSetDevice(f->ctx->device));
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(f->ctx, f->nx, f->ny, f->nz, f->norm16 ? VPT_FORMAT_RG16 : VPT_FORMAT_RG8, false, &d));      // every texel is written below
    const size_t n = f->voxels();
    const dim3 grid(stream_grid(n / 4 + 1));
    if (f->norm16) hipLaunchKernelGGL((k_pair<uint16_t, Map>), grid, dim3(256), 0, f->ctx->stream, (const uint16_t *)f->texels.get(), (const uint32_t *)f->values.get(), (uint16_t *)d->linear.get(), n, map);
    else hipLaunchKernelGGL((k_pair<uint8_t, Map>), grid, dim3(256), 0, f->ctx->stream, (const uint8_t *)f->texels.get(), (const uint32_t *)f->values.get(), d->linear.get(), n, map);
    return volume_finish_derived(f->ctx, f->filter, d, out);
}
