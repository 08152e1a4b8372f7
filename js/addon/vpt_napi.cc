// vpt_napi.cc — thin N-API addon over the C-ABI of include/vpt.h (libvpt_hip.so).
//
// One JS function per C entry point, same argument order; handles are napi_external values; every non-zero return
// code becomes a thrown Error carrying vpt_last_error() (the reference only throws Error(msg)).  No logic lives here:
// the host-side mirror of the reference's classes is js/vpt/*.js.  Built with plain g++ against the system's
// node_api.h (N-API v8, Node >= 12) — see js/addon/Makefile.
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "vpt.h"

#define NAPI_OK(call) do { if ((call) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: " #call); return nullptr; } } while (0)

static napi_value throw_vpt(napi_env env) {
    napi_throw_error(env, nullptr, vpt_last_error());
    return nullptr;
}
#define VPT_CHECK(call) do { if ((call) != VPT_OK) return throw_vpt(env); } while (0)

static bool get_args(napi_env env, napi_callback_info info, size_t want, napi_value *argv) {
    size_t argc = want;
    if (napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr) != napi_ok || argc < want) {
        napi_throw_type_error(env, nullptr, "wrong number of arguments");
        return false;
    }
    return true;
}
static bool get_i32(napi_env env, napi_value v, int32_t *out) {
    if (napi_get_value_int32(env, v, out) != napi_ok) { napi_throw_type_error(env, nullptr, "expected a number"); return false; }
    return true;
}
template <typename T> static bool get_handle(napi_env env, napi_value v, T **out, bool allow_null = false) {
    napi_valuetype t;
    if (napi_typeof(env, v, &t) != napi_ok) return false;
    if (allow_null && (t == napi_null || t == napi_undefined)) { *out = nullptr; return true; }
    void *p = nullptr;
    if (t != napi_external || napi_get_value_external(env, v, &p) != napi_ok) {
        napi_throw_type_error(env, nullptr, "expected a native handle");
        return false;
    }
    *out = (T *)p;
    return true;
}
// any TypedArray / ArrayBuffer -> (pointer, byte length); null/undefined allowed when allow_null
static bool get_bytes(napi_env env, napi_value v, void **data, size_t *nbytes, bool allow_null = false) {
    napi_valuetype t;
    napi_typeof(env, v, &t);
    if (allow_null && (t == napi_null || t == napi_undefined)) { *data = nullptr; *nbytes = 0; return true; }
    bool is;
    if (napi_is_typedarray(env, v, &is) == napi_ok && is) {
        napi_typedarray_type ty; size_t len; napi_value ab; size_t off;
        if (napi_get_typedarray_info(env, v, &ty, &len, data, &ab, &off) != napi_ok) return false;
        static const size_t elem[] = { 1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 8 };
        *nbytes = len * elem[ty];
        return true;
    }
    if (napi_is_arraybuffer(env, v, &is) == napi_ok && is) return napi_get_arraybuffer_info(env, v, data, nbytes) == napi_ok;
    if (napi_is_dataview(env, v, &is) == napi_ok && is) {
        napi_value ab; size_t off;
        return napi_get_dataview_info(env, v, nbytes, data, &ab, &off) == napi_ok;
    }
    napi_throw_type_error(env, nullptr, "expected a TypedArray, DataView or ArrayBuffer");
    return false;
}
static bool get_uniforms(napi_env env, napi_value v, const vpt_uniforms **u, bool allow_null) {
    void *p; size_t n;
    if (!get_bytes(env, v, &p, &n, allow_null)) return false;
    if (p && n < sizeof(vpt_uniforms)) { napi_throw_range_error(env, nullptr, "uniform block is smaller than struct vpt_uniforms"); return false; }
    *u = (const vpt_uniforms *)p;
    return true;
}
// (handle, x, y, z, width, height, depth, bytes): what the box transfers of a volume and of a voxel field take
struct BoxArgs { void *handle; int32_t p[6]; void *data; size_t n; };
static bool get_box(napi_env env, napi_callback_info info, BoxArgs *b) {
    napi_value a[8];
    if (!get_args(env, info, 8, a) || !get_handle(env, a[0], &b->handle)) return false;
    for (int i = 0; i < 6; i++) if (!get_i32(env, a[1 + i], &b->p[i])) return false;
    return get_bytes(env, a[7], &b->data, &b->n);
}
static napi_value make_external(napi_env env, void *p) {
    napi_value v;
    NAPI_OK(napi_create_external(env, p, nullptr, nullptr, &v));     // explicit destroy() is the contract (AbstractRenderer.js:51-58)
    return v;
}
static napi_value undefined(napi_env env) { napi_value v; napi_get_undefined(env, &v); return v; }
static napi_value number(napi_env env, double d) { napi_value v; napi_create_double(env, d, &v); return v; }

// ---- context ------------------------------------------------------------------------------------------
static napi_value DeviceCount(napi_env env, napi_callback_info) {
    int n = 0;
    VPT_CHECK(vpt_device_count(&n));
    return number(env, n);
}
static napi_value ContextCreate(napi_env env, napi_callback_info info) {
    napi_value a[1]; int32_t dev;
    if (!get_args(env, info, 1, a) || !get_i32(env, a[0], &dev)) return nullptr;
    vpt_context *c = nullptr;
    VPT_CHECK(vpt_context_create(dev, &c));
    return make_external(env, c);
}
static napi_value ContextDestroy(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_context *c;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &c)) return nullptr;
    VPT_CHECK(vpt_context_destroy(c));
    return undefined(env);
}
static napi_value ContextSynchronize(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_context *c;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &c)) return nullptr;
    VPT_CHECK(vpt_context_synchronize(c));
    return undefined(env);
}
static napi_value Version(napi_env env, napi_callback_info) {
    napi_value v; napi_create_string_utf8(env, vpt_version(), NAPI_AUTO_LENGTH, &v); return v;
}

// ---- volume -------------------------------------------------------------------------------------------
static napi_value VolumeCreate(napi_env env, napi_callback_info info) {
    napi_value a[5]; vpt_context *c; int32_t w, h, d, f;
    if (!get_args(env, info, 5, a) || !get_handle(env, a[0], &c) || !get_i32(env, a[1], &w) || !get_i32(env, a[2], &h) ||
        !get_i32(env, a[3], &d) || !get_i32(env, a[4], &f)) return nullptr;
    vpt_volume *v = nullptr;
    VPT_CHECK(vpt_volume_create(c, w, h, d, f, &v));
    return make_external(env, v);
}
static napi_value VolumeUploadBlock(napi_env env, napi_callback_info info) {
    BoxArgs b;
    if (!get_box(env, info, &b)) return nullptr;
    VPT_CHECK(vpt_volume_upload_block((vpt_volume *)b.handle, b.p[0], b.p[1], b.p[2], b.p[3], b.p[4], b.p[5], b.data, b.n));
    return undefined(env);
}
static napi_value VolumeFinalize(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_volume *v;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &v)) return nullptr;
    VPT_CHECK(vpt_volume_finalize(v));
    return undefined(env);
}
static napi_value VolumeSetFilter(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_volume *v; int32_t f;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &v) || !get_i32(env, a[1], &f)) return nullptr;
    VPT_CHECK(vpt_volume_set_filter(v, f));
    return undefined(env);
}
static napi_value VolumeDestroy(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_volume *v;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &v)) return nullptr;
    VPT_CHECK(vpt_volume_destroy(v));
    return undefined(env);
}
static napi_value VolumeBrickedBytes(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_volume *v; uint64_t n = 0;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &v)) return nullptr;
    VPT_CHECK(vpt_volume_bricked_bytes(v, &n));
    return number(env, (double)n);
}
// volumeDeriveGradient(volume, op, gain) -> a new volume handle
static napi_value VolumeDeriveGradient(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_volume *v; int32_t op; double gain;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &v) || !get_i32(env, a[1], &op)) return nullptr;
    if (napi_get_value_double(env, a[2], &gain) != napi_ok) { napi_throw_type_error(env, nullptr, "expected a number"); return nullptr; }
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_volume_derive_gradient(v, op, (float)gain, &out));
    return make_external(env, out);
}
// volumeReadBlock(volume, x, y, z, width, height, depth, dst): the box's texels into dst (a TypedArray of the volume's texel type)
static napi_value VolumeReadBlock(napi_env env, napi_callback_info info) {
    BoxArgs b;
    if (!get_box(env, info, &b)) return nullptr;
    VPT_CHECK(vpt_volume_read_block((vpt_volume *)b.handle, b.p[0], b.p[1], b.p[2], b.p[3], b.p[4], b.p[5], b.data, b.n));
    return undefined(env);
}
// volumeHistogram(volume, bins): bins is a Uint32Array of 256 (one channel) or 65536 (two channels) counts
static napi_value VolumeHistogram(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_volume *v; void *data; size_t n;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &v) || !get_bytes(env, a[1], &data, &n)) return nullptr;
    VPT_CHECK(vpt_volume_histogram(v, (uint32_t *)data, n / sizeof(uint32_t)));
    return undefined(env);
}
// volumeWindow(volume, lo, hi, format) -> a new volume handle (format: VPT_FORMAT_R8 or VPT_FORMAT_R16)
static napi_value VolumeWindow(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_volume *v; double lo, hi; int32_t format;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &v)) return nullptr;
    if (napi_get_value_double(env, a[1], &lo) != napi_ok || napi_get_value_double(env, a[2], &hi) != napi_ok) {
        napi_throw_type_error(env, nullptr, "expected a number"); return nullptr;
    }
    if (!get_i32(env, a[3], &format)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_volume_window(v, lo, hi, format, &out));
    return make_external(env, out);
}
// volumeReduce(volume) -> a new volume handle: the next coarser level, ceil(n / 2) texels per axis
static napi_value VolumeReduce(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_volume *v;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &v)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_volume_reduce(v, &out));
    return make_external(env, out);
}
// volumeSmooth(volume, passes) -> a new volume handle: `passes` applications of the binomial 3 x 3 x 3 kernel
static napi_value VolumeSmooth(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_volume *v; int32_t passes;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &v) || !get_i32(env, a[1], &passes)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_volume_smooth(v, passes, &out));
    return make_external(env, out);
}
// volumeRank(volume, op, passes) -> a new volume handle: `passes` applications of the rank operator VPT_RANK_* over the 3 x 3 x 3 box
static napi_value VolumeRank(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_volume *v; int32_t op, passes;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &v) || !get_i32(env, a[1], &op) || !get_i32(env, a[2], &passes)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_volume_rank(v, op, passes, &out));
    return make_external(env, out);
}
// volumeResample(volume, width, height, depth, mode) -> a new volume handle: the volume on a grid of that size, mode VPT_RESAMPLE_*
static napi_value VolumeResample(napi_env env, napi_callback_info info) {
    napi_value a[5]; vpt_volume *v; int32_t w, h, d, mode;
    if (!get_args(env, info, 5, a) || !get_handle(env, a[0], &v) || !get_i32(env, a[1], &w) || !get_i32(env, a[2], &h) || !get_i32(env, a[3], &d) ||
        !get_i32(env, a[4], &mode)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_volume_resample(v, w, h, d, mode, &out));
    return make_external(env, out);
}
// ---- two volumes combined or compared -----------------------------------------------------------------
static bool get_u32(napi_env env, napi_value v, uint32_t *out);
// the ten arguments volumeCombine and volumeCombineTimed share: (a, b, op, channel, lo, hi, fill, wa, wb, offset)
static bool get_combine(napi_env env, napi_callback_info info, vpt_volume **va, vpt_volume **vb, struct vpt_combine_params *p) {
    napi_value a[10]; int32_t op, channel, wa, wb, offset;
    if (!get_args(env, info, 10, a) || !get_handle(env, a[0], va) || !get_handle(env, a[1], vb) || !get_i32(env, a[2], &op) || !get_i32(env, a[3], &channel) ||
        !get_u32(env, a[4], &p->lo) || !get_u32(env, a[5], &p->hi) || !get_u32(env, a[6], &p->fill) || !get_i32(env, a[7], &wa) || !get_i32(env, a[8], &wb) ||
        !get_i32(env, a[9], &offset)) return false;
    p->op = op; p->b_channel = channel; p->wa = wa; p->wb = wb; p->offset = offset;
    return true;
}
// volumeCombine(a, b, op, channel, lo, hi, fill, wa, wb, offset) -> a new volume handle: a and channel `channel` of b combined by VPT_COMBINE_*
static napi_value VolumeCombine(napi_env env, napi_callback_info info) {
    vpt_volume *va, *vb; struct vpt_combine_params p = {};
    if (!get_combine(env, info, &va, &vb, &p)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_volume_combine(va, vb, &p, &out));
    return make_external(env, out);
}
// volumeCombineTimed(the same) -> [a new volume handle, the milliseconds of the combining pass alone]
static napi_value VolumeCombineTimed(napi_env env, napi_callback_info info) {
    vpt_volume *va, *vb; struct vpt_combine_params p = {};
    if (!get_combine(env, info, &va, &vb, &p)) return nullptr;
    vpt_volume *out = nullptr; double ms = 0.0;
    VPT_CHECK(vpt_volume_combine_timed(va, vb, &p, &out, &ms));
    napi_value pair, e;
    napi_create_array_with_length(env, 2, &pair);
    napi_set_element(env, pair, 0, make_external(env, out));
    napi_create_double(env, ms, &e); napi_set_element(env, pair, 1, e);
    return pair;
}
// volumeCompare(a, b, channel, loA, hiA, loB, hiB) -> the eight 64-bit counts as sixteen numbers, (low, high) 32-bit halves: a count can
// pass 2^53, which the doubles componentsInfo returns its counts in do not hold exactly
static napi_value VolumeCompare(napi_env env, napi_callback_info info) {
    napi_value a[7]; vpt_volume *va, *vb; int32_t channel; uint32_t r[4];
    if (!get_args(env, info, 7, a) || !get_handle(env, a[0], &va) || !get_handle(env, a[1], &vb) || !get_i32(env, a[2], &channel) || !get_u32(env, a[3], &r[0]) ||
        !get_u32(env, a[4], &r[1]) || !get_u32(env, a[5], &r[2]) || !get_u32(env, a[6], &r[3])) return nullptr;
    uint64_t counts[8] = {};
    VPT_CHECK(vpt_volume_compare(va, vb, channel, r[0], r[1], r[2], r[3], counts));
    napi_value out, e;
    napi_create_array_with_length(env, 16, &out);
    for (int k = 0; k < 8; k++) {
        napi_create_double(env, (double)(uint32_t)(counts[k] & 0xFFFFFFFFull), &e); napi_set_element(env, out, 2 * k, e);
        napi_create_double(env, (double)(uint32_t)(counts[k] >> 32), &e); napi_set_element(env, out, 2 * k + 1, e);
    }
    return out;
}
// ---- morphological reconstruction and the geodesic operations ---------------------------------------------
// [a new volume handle, milliseconds, launches of the propagation kernel, tile runs] of the timed forms
static napi_value recon_profile(napi_env env, vpt_volume *out, double ms, uint32_t launches, uint64_t tile_runs) {
    napi_value r, e;
    napi_create_array_with_length(env, 4, &r);
    napi_set_element(env, r, 0, make_external(env, out));
    napi_create_double(env, ms, &e); napi_set_element(env, r, 1, e);
    napi_create_double(env, (double)launches, &e); napi_set_element(env, r, 2, e);
    napi_create_double(env, (double)tile_runs, &e); napi_set_element(env, r, 3, e);
    return r;
}
// volumeReconstruct(marker, markerChannel, mask, maskChannel, op, connectivity) -> a new volume handle: VPT_RECONSTRUCT_* of the marker under the mask
static napi_value VolumeReconstruct(napi_env env, napi_callback_info info) {
    napi_value a[6]; vpt_volume *m, *k; int32_t mc, kc, op, conn;
    if (!get_args(env, info, 6, a) || !get_handle(env, a[0], &m) || !get_i32(env, a[1], &mc) || !get_handle(env, a[2], &k) || !get_i32(env, a[3], &kc) ||
        !get_i32(env, a[4], &op) || !get_i32(env, a[5], &conn)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_volume_reconstruct(m, mc, k, kc, op, conn, &out));
    return make_external(env, out);
}
// volumeReconstructTimed(the same, tileRounds) -> [handle, ms, launches, tile runs]; tileRounds 0: the library's own round cap, otherwise
// vpt_volume_reconstruct_capped (no tile runs)
static napi_value VolumeReconstructTimed(napi_env env, napi_callback_info info) {
    napi_value a[7]; vpt_volume *m, *k; int32_t mc, kc, op, conn, rounds;
    if (!get_args(env, info, 7, a) || !get_handle(env, a[0], &m) || !get_i32(env, a[1], &mc) || !get_handle(env, a[2], &k) || !get_i32(env, a[3], &kc) ||
        !get_i32(env, a[4], &op) || !get_i32(env, a[5], &conn) || !get_i32(env, a[6], &rounds)) return nullptr;
    vpt_volume *out = nullptr; double ms = 0.0; uint32_t launches = 0; uint64_t runs = 0;
    if (rounds == 0) VPT_CHECK(vpt_volume_reconstruct_timed(m, mc, k, kc, op, conn, &out, &ms, &launches, &runs));
    else VPT_CHECK(vpt_volume_reconstruct_capped(m, mc, k, kc, op, conn, rounds, &out, &ms, &launches));
    return recon_profile(env, out, ms, launches, runs);
}
// volumeGeodesic(volume, channel, op, h, connectivity) -> a new volume handle: the geodesic operation VPT_GEODESIC_*
static napi_value VolumeGeodesic(napi_env env, napi_callback_info info) {
    napi_value a[5]; vpt_volume *v; int32_t channel, op, conn; uint32_t h;
    if (!get_args(env, info, 5, a) || !get_handle(env, a[0], &v) || !get_i32(env, a[1], &channel) || !get_i32(env, a[2], &op) || !get_u32(env, a[3], &h) ||
        !get_i32(env, a[4], &conn)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_volume_geodesic(v, channel, op, h, conn, &out));
    return make_external(env, out);
}
// volumeGeodesicTimed(the same) -> [handle, ms, launches, tile runs]
static napi_value VolumeGeodesicTimed(napi_env env, napi_callback_info info) {
    napi_value a[5]; vpt_volume *v; int32_t channel, op, conn; uint32_t h;
    if (!get_args(env, info, 5, a) || !get_handle(env, a[0], &v) || !get_i32(env, a[1], &channel) || !get_i32(env, a[2], &op) || !get_u32(env, a[3], &h) ||
        !get_i32(env, a[4], &conn)) return nullptr;
    vpt_volume *out = nullptr; double ms = 0.0; uint32_t launches = 0; uint64_t runs = 0;
    VPT_CHECK(vpt_volume_geodesic_timed(v, channel, op, h, conn, &out, &ms, &launches, &runs));
    return recon_profile(env, out, ms, launches, runs);
}
// volumeRange(volume) -> [lo, hi]: the smallest and the largest code or value
static napi_value VolumeRange(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_volume *v;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &v)) return nullptr;
    double lo = 0.0, hi = 0.0;
    VPT_CHECK(vpt_volume_range(v, &lo, &hi));
    napi_value out, e;
    napi_create_array_with_length(env, 2, &out);
    napi_create_double(env, lo, &e); napi_set_element(env, out, 0, e);
    napi_create_double(env, hi, &e); napi_set_element(env, out, 1, e);
    return out;
}
// volumeCodeHistogram(volume, bins): bins is a Uint32Array of 256 (8-bit codes) or 65536 (16-bit codes) counts
static napi_value VolumeCodeHistogram(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_volume *v; void *data; size_t n;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &v) || !get_bytes(env, a[1], &data, &n)) return nullptr;
    VPT_CHECK(vpt_volume_code_histogram(v, (uint32_t *)data, n / sizeof(uint32_t)));
    return undefined(env);
}

// ---- connected components -----------------------------------------------------------------------------
static bool get_u32(napi_env env, napi_value v, uint32_t *out) {
    double d;
    if (napi_get_value_double(env, v, &d) != napi_ok || !(d >= 0.0 && d <= 4294967295.0) || d != (double)(uint32_t)d) {
        napi_throw_type_error(env, nullptr, "expected an integer in 0 .. 2^32 - 1"); return false;
    }
    *out = (uint32_t)d;
    return true;
}
// a non-negative integer as a double; anything at or above 2^64 (Infinity included) is UINT64_MAX
static bool get_u64(napi_env env, napi_value v, uint64_t *out) {
    double d;
    if (napi_get_value_double(env, v, &d) != napi_ok || !(d >= 0.0)) { napi_throw_type_error(env, nullptr, "expected a non-negative number"); return false; }
    *out = d >= 18446744073709551616.0 ? UINT64_MAX : (uint64_t)d;
    return true;
}
// volumeComponents(volume, lo, hi, connectivity, minVoxels) -> a components handle
static napi_value VolumeComponents(napi_env env, napi_callback_info info) {
    napi_value a[5]; vpt_volume *v; uint32_t lo, hi, min_voxels; int32_t connectivity;
    if (!get_args(env, info, 5, a) || !get_handle(env, a[0], &v) || !get_u32(env, a[1], &lo) || !get_u32(env, a[2], &hi) ||
        !get_i32(env, a[3], &connectivity) || !get_u32(env, a[4], &min_voxels)) return nullptr;
    vpt_components *out = nullptr;
    VPT_CHECK(vpt_volume_components(v, lo, hi, connectivity, min_voxels, &out));
    return make_external(env, out);
}
// the eight arguments volumeWatershed and volumeWatershedTimed share: (relief, channel, texels | null, lo, hi, polarity, connectivity, minVoxels)
struct WatershedArgs { vpt_volume *relief, *texels; int32_t channel, polarity, connectivity; uint32_t lo, hi, min_voxels; };
static bool get_watershed(napi_env env, const napi_value *a, WatershedArgs *w) {
    return get_handle(env, a[0], &w->relief) && get_i32(env, a[1], &w->channel) && get_handle(env, a[2], &w->texels, true) && get_u32(env, a[3], &w->lo) &&
           get_u32(env, a[4], &w->hi) && get_i32(env, a[5], &w->polarity) && get_i32(env, a[6], &w->connectivity) && get_u32(env, a[7], &w->min_voxels);
}
// volumeWatershed(relief, channel, texels | null, lo, hi, polarity, connectivity, minVoxels) -> a components handle: the basins (VPT_WATERSHED_*)
static napi_value VolumeWatershed(napi_env env, napi_callback_info info) {
    napi_value a[8]; WatershedArgs w;
    if (!get_args(env, info, 8, a) || !get_watershed(env, a, &w)) return nullptr;
    vpt_components *out = nullptr;
    VPT_CHECK(vpt_volume_watershed(w.relief, w.channel, w.texels, w.lo, w.hi, w.polarity, w.connectivity, w.min_voxels, &out));
    return make_external(env, out);
}
// volumeWatershedTimed(the same, mergeSteps, flattenSteps, tileRounds) -> [handle, ms classify, ms plateau, ms links, plateau launches]; the
// three caps 0: the library's own, otherwise vpt_volume_watershed_capped
static napi_value VolumeWatershedTimed(napi_env env, napi_callback_info info) {
    napi_value a[11]; WatershedArgs w; int32_t merge_steps, flatten_steps, tile_rounds;
    if (!get_args(env, info, 11, a) || !get_watershed(env, a, &w) || !get_i32(env, a[8], &merge_steps) || !get_i32(env, a[9], &flatten_steps) ||
        !get_i32(env, a[10], &tile_rounds)) return nullptr;
    vpt_components *out = nullptr; double ms[VPT_WATERSHED_PHASES] = {}; uint32_t launches = 0;
    if (merge_steps == 0 && flatten_steps == 0 && tile_rounds == 0)
        VPT_CHECK(vpt_volume_watershed_timed(w.relief, w.channel, w.texels, w.lo, w.hi, w.polarity, w.connectivity, w.min_voxels, &out, ms, &launches));
    else
        VPT_CHECK(vpt_volume_watershed_capped(w.relief, w.channel, w.texels, w.lo, w.hi, w.polarity, w.connectivity, w.min_voxels, merge_steps, flatten_steps,
                                              tile_rounds, &out, ms, &launches));
    napi_value r, e;
    napi_create_array_with_length(env, 2 + VPT_WATERSHED_PHASES, &r);
    napi_set_element(env, r, 0, make_external(env, out));
    for (int k = 0; k < VPT_WATERSHED_PHASES; k++) { napi_create_double(env, ms[k], &e); napi_set_element(env, r, 1 + k, e); }
    napi_create_double(env, (double)launches, &e); napi_set_element(env, r, 1 + VPT_WATERSHED_PHASES, e);
    return r;
}
// componentsInfo(components) -> [listed, dropped, foregroundVoxels, listedVoxels]
static napi_value ComponentsInfo(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_components *c;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &c)) return nullptr;
    struct vpt_components_info i;
    VPT_CHECK(vpt_components_info(c, &i));
    const uint64_t f[4] = { i.listed, i.dropped, i.foreground_voxels, i.listed_voxels };
    napi_value out, e;
    napi_create_array_with_length(env, 4, &out);
    for (int k = 0; k < 4; k++) { napi_create_double(env, (double)f[k], &e); napi_set_element(env, out, k, e); }
    return out;
}
// componentsList(components, first, dst): dst is a Uint32Array of 4 n words, (rootX, rootY, rootZ, voxels) of components first .. first + n - 1
static napi_value ComponentsList(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_components *c; uint64_t first; void *data; size_t n;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &c) || !get_u64(env, a[1], &first) || !get_bytes(env, a[2], &data, &n)) return nullptr;
    VPT_CHECK(vpt_components_list(c, first, n / sizeof(struct vpt_component), (struct vpt_component *)data));
    return undefined(env);
}
// componentsRanks(components, x, y, z, width, height, depth, dst): the box's ranks into dst (a Uint32Array)
static napi_value ComponentsRanks(napi_env env, napi_callback_info info) {
    BoxArgs b;
    if (!get_box(env, info, &b)) return nullptr;
    VPT_CHECK(vpt_components_ranks((vpt_components *)b.handle, b.p[0], b.p[1], b.p[2], b.p[3], b.p[4], b.p[5], (uint32_t *)b.data, b.n));
    return undefined(env);
}
// componentsKeep(components, firstRank, lastRank, fill) -> a new volume handle
static napi_value ComponentsKeep(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_components *c; uint64_t first, last; uint32_t fill;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &c) || !get_u64(env, a[1], &first) || !get_u64(env, a[2], &last) || !get_u32(env, a[3], &fill)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_components_keep(c, first, last, fill, &out));
    return make_external(env, out);
}
// componentsLabel(components) -> a new volume handle
static napi_value ComponentsLabel(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_components *c;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &c)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_components_label(c, &out));
    return make_external(env, out);
}
// componentsMeasure(components, values | null, channel, first, dst): dst holds 88 n bytes (any TypedArray / ArrayBuffer), the records
// (struct vpt_component_measure) of components first .. first + n - 1; js/vpt/Volume.js reads the 64-bit fields out as BigInts
static bool get_measure(napi_env env, napi_callback_info info, size_t extra, napi_value *a, vpt_components **c, vpt_volume **values, int32_t *channel,
                        uint64_t *first, void **data, size_t *n) {
    return get_args(env, info, 5 + extra, a) && get_handle(env, a[0], c) && get_handle(env, a[1], values, true) && get_i32(env, a[2], channel) &&
           get_u64(env, a[3], first) && get_bytes(env, a[4], data, n);
}
static napi_value ComponentsMeasure(napi_env env, napi_callback_info info) {
    napi_value a[5]; vpt_components *c; vpt_volume *values; int32_t channel; uint64_t first; void *data; size_t n;
    if (!get_measure(env, info, 0, a, &c, &values, &channel, &first, &data, &n)) return nullptr;
    VPT_CHECK(vpt_components_measure(c, values, channel, first, n / sizeof(struct vpt_component_measure), (struct vpt_component_measure *)data));
    return undefined(env);
}
// componentsMeasureTimed(the same) -> the milliseconds of the measuring pass alone
static napi_value ComponentsMeasureTimed(napi_env env, napi_callback_info info) {
    napi_value a[5]; vpt_components *c; vpt_volume *values; int32_t channel; uint64_t first; void *data; size_t n;
    if (!get_measure(env, info, 0, a, &c, &values, &channel, &first, &data, &n)) return nullptr;
    double ms = 0.0;
    VPT_CHECK(vpt_components_measure_timed(c, values, channel, first, n / sizeof(struct vpt_component_measure), (struct vpt_component_measure *)data, &ms));
    return number(env, ms);
}
// componentsKeepSet(components, ranks, fill) -> a new volume handle; ranks is a BigUint64Array of 1-based ranks
static napi_value ComponentsKeepSet(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_components *c; void *data; size_t n; uint32_t fill;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &c) || !get_bytes(env, a[1], &data, &n) || !get_u32(env, a[2], &fill)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_components_keep_set(c, (const uint64_t *)data, n / sizeof(uint64_t), fill, &out));
    return make_external(env, out);
}
static napi_value ComponentsDestroy(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_components *c;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &c)) return nullptr;
    VPT_CHECK(vpt_components_destroy(c));
    return undefined(env);
}

// ---- distance transform -------------------------------------------------------------------------------
// volumeDistance(volume, lo, hi, seeds) -> a distance handle
static napi_value VolumeDistance(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_volume *v; uint32_t lo, hi; int32_t seeds;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &v) || !get_u32(env, a[1], &lo) || !get_u32(env, a[2], &hi) || !get_i32(env, a[3], &seeds)) return nullptr;
    vpt_distance *out = nullptr;
    VPT_CHECK(vpt_volume_distance(v, lo, hi, seeds, &out));
    return make_external(env, out);
}
// distanceInfo(distance) -> [seeds, largest]
static napi_value DistanceInfo(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_distance *d;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &d)) return nullptr;
    struct vpt_distance_info i;
    VPT_CHECK(vpt_distance_info(d, &i));
    napi_value out;
    napi_create_array_with_length(env, 2, &out);
    napi_set_element(env, out, 0, number(env, (double)i.seeds));
    napi_set_element(env, out, 1, number(env, (double)i.largest));
    return out;
}
// distanceSquared(distance, x, y, z, width, height, depth, dst): the box's squared distances into dst (a Uint32Array)
static napi_value DistanceSquared(napi_env env, napi_callback_info info) {
    BoxArgs b;
    if (!get_box(env, info, &b)) return nullptr;
    VPT_CHECK(vpt_distance_squared((vpt_distance *)b.handle, b.p[0], b.p[1], b.p[2], b.p[3], b.p[4], b.p[5], (uint32_t *)b.data, b.n));
    return undefined(env);
}
// distanceWithin(distance, r2Lo, r2Hi, fill) -> a new volume handle
static napi_value DistanceWithin(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_distance *d; uint32_t r2_lo, r2_hi, fill;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &d) || !get_u32(env, a[1], &r2_lo) || !get_u32(env, a[2], &r2_hi) || !get_u32(env, a[3], &fill)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_distance_within(d, r2_lo, r2_hi, fill, &out));
    return make_external(env, out);
}
// distanceChannel(distance, steps) -> a new volume handle
static napi_value DistanceChannel(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_distance *d; int32_t steps;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &d) || !get_i32(env, a[1], &steps)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_distance_channel(d, steps, &out));
    return make_external(env, out);
}
// distanceProfile(distance) -> [x, y, z] milliseconds
static napi_value DistanceProfile(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_distance *d;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &d)) return nullptr;
    double ms[VPT_DISTANCE_PHASES];
    VPT_CHECK(vpt_distance_profile(d, ms));
    napi_value out;
    napi_create_array_with_length(env, VPT_DISTANCE_PHASES, &out);
    for (int k = 0; k < VPT_DISTANCE_PHASES; k++) napi_set_element(env, out, k, number(env, ms[k]));
    return out;
}
// distanceThickness(distance) -> a distance handle: the local thickness
static napi_value DistanceThickness(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_distance *d;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &d)) return nullptr;
    vpt_distance *out = nullptr;
    VPT_CHECK(vpt_distance_thickness(d, &out));
    return make_external(env, out);
}
// distanceThicknessTimed(distance, flags) -> [handle, ms tiles, ms cover, ms info, tiles, visited]; flags < 0: vpt_distance_thickness_timed,
// otherwise vpt_distance_thickness_capped (tiles is then 0)
static napi_value DistanceThicknessTimed(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_distance *d; int32_t flags;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &d) || !get_i32(env, a[1], &flags)) return nullptr;
    vpt_distance *out = nullptr; double ms[VPT_THICKNESS_PHASES] = {}; uint64_t tiles = 0, visited = 0;
    if (flags < 0) VPT_CHECK(vpt_distance_thickness_timed(d, &out, ms, &tiles, &visited));
    else VPT_CHECK(vpt_distance_thickness_capped(d, flags, &out, ms, &visited));
    napi_value r;
    napi_create_array_with_length(env, 3 + VPT_THICKNESS_PHASES, &r);
    napi_set_element(env, r, 0, make_external(env, out));
    for (int k = 0; k < VPT_THICKNESS_PHASES; k++) napi_set_element(env, r, 1 + k, number(env, ms[k]));
    napi_set_element(env, r, 1 + VPT_THICKNESS_PHASES, number(env, (double)tiles));
    napi_set_element(env, r, 2 + VPT_THICKNESS_PHASES, number(env, (double)visited));
    return r;
}
// ---- skeleton -------------------------------------------------------------------------------------------
// volumeSkeleton(volume, lo, hi, mode, passes, flags) -> a skeleton handle; flags < 0: vpt_volume_skeleton, otherwise vpt_volume_skeleton_capped
static napi_value VolumeSkeleton(napi_env env, napi_callback_info info) {
    napi_value a[6]; vpt_volume *v; uint32_t lo, hi; int32_t mode, passes, flags;
    if (!get_args(env, info, 6, a) || !get_handle(env, a[0], &v) || !get_u32(env, a[1], &lo) || !get_u32(env, a[2], &hi) || !get_i32(env, a[3], &mode) ||
        !get_i32(env, a[4], &passes) || !get_i32(env, a[5], &flags)) return nullptr;
    vpt_skeleton *out = nullptr;
    if (flags < 0) VPT_CHECK(vpt_volume_skeleton(v, lo, hi, mode, passes, &out));
    else VPT_CHECK(vpt_volume_skeleton_capped(v, lo, hi, mode, passes, flags, &out));
    return make_external(env, out);
}
// skeletonInfo(skeleton) -> [object_voxels, kept_voxels, passes, converged, isolated, ends, regular, junctions]
static napi_value SkeletonInfo(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_skeleton *k;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &k)) return nullptr;
    struct vpt_skeleton_info i;
    VPT_CHECK(vpt_skeleton_info(k, &i));
    const uint64_t fields[8] = { i.object_voxels, i.kept_voxels, i.passes, i.converged, i.isolated, i.ends, i.regular, i.junctions };
    napi_value out;
    napi_create_array_with_length(env, 8, &out);
    for (int f = 0; f < 8; f++) napi_set_element(env, out, f, number(env, (double)fields[f]));
    return out;
}
// skeletonBurn(skeleton, x, y, z, width, height, depth, dst): the box's burn passes into dst (a Uint32Array)
static napi_value SkeletonBurn(napi_env env, napi_callback_info info) {
    BoxArgs b;
    if (!get_box(env, info, &b)) return nullptr;
    VPT_CHECK(vpt_skeleton_burn((vpt_skeleton *)b.handle, b.p[0], b.p[1], b.p[2], b.p[3], b.p[4], b.p[5], (uint32_t *)b.data, b.n));
    return undefined(env);
}
// skeletonWithin(skeleton, kLo, kHi, fill) -> a new volume handle
static napi_value SkeletonWithin(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_skeleton *k; uint32_t k_lo, k_hi, fill;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &k) || !get_u32(env, a[1], &k_lo) || !get_u32(env, a[2], &k_hi) || !get_u32(env, a[3], &fill)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_skeleton_within(k, k_lo, k_hi, fill, &out));
    return make_external(env, out);
}
// skeletonProfile(skeleton) -> [ms seed, ms border, ms steps, ms census, launches, tiles]
static napi_value SkeletonProfile(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_skeleton *k;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &k)) return nullptr;
    double ms[VPT_SKELETON_PHASES]; uint64_t launches = 0, tiles = 0;
    VPT_CHECK(vpt_skeleton_profile(k, ms, &launches, &tiles));
    napi_value out;
    napi_create_array_with_length(env, VPT_SKELETON_PHASES + 2, &out);
    for (int p = 0; p < VPT_SKELETON_PHASES; p++) napi_set_element(env, out, p, number(env, ms[p]));
    napi_set_element(env, out, VPT_SKELETON_PHASES, number(env, (double)launches));
    napi_set_element(env, out, VPT_SKELETON_PHASES + 1, number(env, (double)tiles));
    return out;
}
static napi_value SkeletonDestroy(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_skeleton *k;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &k)) return nullptr;
    VPT_CHECK(vpt_skeleton_destroy(k));
    return undefined(env);
}
// ---- graph ----------------------------------------------------------------------------------------------
// volumeGraph(volume, lo, hi) -> a graph handle
static napi_value VolumeGraph(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_volume *v; uint32_t lo, hi;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &v) || !get_u32(env, a[1], &lo) || !get_u32(env, a[2], &hi)) return nullptr;
    vpt_graph *out = nullptr;
    VPT_CHECK(vpt_volume_graph(v, lo, hi, &out));
    return make_external(env, out);
}
// skeletonGraph(skeleton) -> a graph handle
static napi_value SkeletonGraph(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_skeleton *k;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &k)) return nullptr;
    vpt_graph *out = nullptr;
    VPT_CHECK(vpt_skeleton_graph(k, &out));
    return make_external(env, out);
}
// graphInfo(graph) -> the fourteen fields of struct vpt_graph_info, in its order
static napi_value GraphInfo(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_graph *g;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &g)) return nullptr;
    struct vpt_graph_info i;
    VPT_CHECK(vpt_graph_info(g, &i));
    const uint64_t fields[14] = { i.kept_voxels, i.node_voxels, i.branches, i.nodes, i.isolated, i.segments, i.spurs, i.links, i.loops, i.cycles,
                                  i.steps_face, i.steps_edge, i.steps_corner, i.attachments };
    napi_value out;
    napi_create_array_with_length(env, 14, &out);
    for (int f = 0; f < 14; f++) napi_set_element(env, out, f, number(env, (double)fields[f]));
    return out;
}
// graphBranches(graph, first, dst): dst holds 64 n bytes, the records (struct vpt_graph_branch) of branches first .. first + n - 1;
// graphNodes(graph, first, dst): 16 n bytes (struct vpt_graph_node); js/vpt/Volume.js reads the fields out
static napi_value GraphBranches(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_graph *g; uint64_t first; void *data; size_t n;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &g) || !get_u64(env, a[1], &first) || !get_bytes(env, a[2], &data, &n)) return nullptr;
    VPT_CHECK(vpt_graph_branches(g, first, n / sizeof(struct vpt_graph_branch), (struct vpt_graph_branch *)data));
    return undefined(env);
}
static napi_value GraphNodes(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_graph *g; uint64_t first; void *data; size_t n;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &g) || !get_u64(env, a[1], &first) || !get_bytes(env, a[2], &data, &n)) return nullptr;
    VPT_CHECK(vpt_graph_nodes(g, first, n / sizeof(struct vpt_graph_node), (struct vpt_graph_node *)data));
    return undefined(env);
}
// graphComponents(graph, which) -> a components handle the caller owns; which 0: the branches, 1: the nodes
static napi_value GraphComponents(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_graph *g; int32_t which;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &g) || !get_i32(env, a[1], &which)) return nullptr;
    vpt_components *out = nullptr;
    if (which == 0) VPT_CHECK(vpt_graph_branch_components(g, &out));
    else VPT_CHECK(vpt_graph_node_components(g, &out));
    return make_external(env, out);
}
// graphClasses(graph) -> a new volume handle
static napi_value GraphClasses(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_graph *g;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &g)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_graph_classes(g, &out));
    return make_external(env, out);
}
// graphPrune(graph, length, wf, we, wc, flags, fill) -> a new volume handle; length: a BigUint64Array of one element (every 64-bit length)
static napi_value GraphPrune(napi_env env, napi_callback_info info) {
    napi_value a[7]; vpt_graph *g; void *data; size_t n; uint32_t wf, we, wc, flags, fill;
    if (!get_args(env, info, 7, a) || !get_handle(env, a[0], &g) || !get_bytes(env, a[1], &data, &n)) return nullptr;
    if (n != sizeof(uint64_t)) { napi_throw_type_error(env, nullptr, "expected a BigUint64Array of one element"); return nullptr; }
    if (!get_u32(env, a[2], &wf) || !get_u32(env, a[3], &we) || !get_u32(env, a[4], &wc) || !get_u32(env, a[5], &flags) || !get_u32(env, a[6], &fill)) return nullptr;
    vpt_volume *out = nullptr;
    VPT_CHECK(vpt_graph_prune(g, *(const uint64_t *)data, wf, we, wc, flags, fill, &out));
    return make_external(env, out);
}
// graphProfile(graph) -> [ms seed, ms classify, ms branches, ms nodes, ms links, ms host, launches]
static napi_value GraphProfile(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_graph *g;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &g)) return nullptr;
    double ms[VPT_GRAPH_PHASES]; uint64_t launches = 0;
    VPT_CHECK(vpt_graph_profile(g, ms, &launches));
    napi_value out;
    napi_create_array_with_length(env, VPT_GRAPH_PHASES + 1, &out);
    for (int p = 0; p < VPT_GRAPH_PHASES; p++) napi_set_element(env, out, p, number(env, ms[p]));
    napi_set_element(env, out, VPT_GRAPH_PHASES, number(env, (double)launches));
    return out;
}
static napi_value GraphDestroy(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_graph *g;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &g)) return nullptr;
    VPT_CHECK(vpt_graph_destroy(g));
    return undefined(env);
}
// ---- surface --------------------------------------------------------------------------------------------
// volumeSurface(volume, channel, level, scanWords) -> a surface handle; scanWords < 0: vpt_volume_surface, otherwise vpt_volume_surface_capped
static napi_value VolumeSurface(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_volume *v; int32_t channel, scan_words; uint32_t level;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &v) || !get_i32(env, a[1], &channel) || !get_u32(env, a[2], &level) || !get_i32(env, a[3], &scan_words)) return nullptr;
    vpt_surface *out = nullptr;
    if (scan_words < 0) VPT_CHECK(vpt_volume_surface(v, channel, level, &out));
    else VPT_CHECK(vpt_volume_surface_capped(v, channel, level, (uint32_t)scan_words, &out));
    return make_external(env, out);
}
// surfaceInfo(surface) -> [vertices, quads, cells, inside, crossings x, y, z, level, width, height, depth, channel]
static napi_value SurfaceInfo(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_surface *s;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &s)) return nullptr;
    struct vpt_surface_info i;
    VPT_CHECK(vpt_surface_info(s, &i));
    const double fields[12] = { (double)i.vertices, (double)i.quads, (double)i.cells, (double)i.inside, (double)i.crossings[0], (double)i.crossings[1],
                                (double)i.crossings[2], (double)i.level, (double)i.width, (double)i.height, (double)i.depth, (double)i.channel };
    napi_value out;
    napi_create_array_with_length(env, 12, &out);
    for (int f = 0; f < 12; f++) napi_set_element(env, out, f, number(env, fields[f]));
    return out;
}
// surfaceVertices(surface, first, dst) / surfaceQuads(surface, first, dst): dst is a Uint32Array of 3 n / 4 n words
static napi_value surface_page(napi_env env, napi_callback_info info, bool quads) {
    napi_value a[3]; vpt_surface *s; uint64_t first; void *data; size_t n;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &s) || !get_u64(env, a[1], &first) || !get_bytes(env, a[2], &data, &n)) return nullptr;
    if (quads) VPT_CHECK(vpt_surface_quads(s, first, n / 16, (uint32_t *)data, n));
    else VPT_CHECK(vpt_surface_vertices(s, first, n / 12, (uint32_t *)data, n));
    return undefined(env);
}
static napi_value SurfaceVertices(napi_env env, napi_callback_info info) { return surface_page(env, info, false); }
static napi_value SurfaceQuads(napi_env env, napi_callback_info info) { return surface_page(env, info, true); }
// surfaceProfile(surface) -> [ms inside, classify, scan, vertices, quads]
static napi_value SurfaceProfile(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_surface *s;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &s)) return nullptr;
    double ms[VPT_SURFACE_PHASES];
    VPT_CHECK(vpt_surface_profile(s, ms));
    napi_value out;
    napi_create_array_with_length(env, VPT_SURFACE_PHASES, &out);
    for (int p = 0; p < VPT_SURFACE_PHASES; p++) napi_set_element(env, out, p, number(env, ms[p]));
    return out;
}
static napi_value SurfaceDestroy(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_surface *s;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &s)) return nullptr;
    VPT_CHECK(vpt_surface_destroy(s));
    return undefined(env);
}
static napi_value DistanceDestroy(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_distance *d;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &d)) return nullptr;
    VPT_CHECK(vpt_distance_destroy(d));
    return undefined(env);
}

// ---- renderer -----------------------------------------------------------------------------------------
static napi_value RendererCreate(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_context *c; int32_t kind, w, h;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &c) || !get_i32(env, a[1], &kind) || !get_i32(env, a[2], &w) ||
        !get_i32(env, a[3], &h)) return nullptr;
    vpt_renderer *r = nullptr;
    VPT_CHECK(vpt_renderer_create(c, kind, w, h, &r));
    return make_external(env, r);
}
static napi_value RendererDestroy(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_renderer *r;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &r)) return nullptr;
    VPT_CHECK(vpt_renderer_destroy(r));
    return undefined(env);
}
static napi_value RendererSetShard(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_renderer *r; int32_t rank, world, rows;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &r) || !get_i32(env, a[1], &rank) || !get_i32(env, a[2], &world) ||
        !get_i32(env, a[3], &rows)) return nullptr;
    VPT_CHECK(vpt_renderer_set_shard(r, rank, world, rows));
    return undefined(env);
}
static napi_value RendererLocalRows(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_renderer *r; int rows = 0;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &r)) return nullptr;
    VPT_CHECK(vpt_renderer_local_rows(r, &rows));
    return number(env, rows);
}
static napi_value RendererGlobalRow(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_renderer *r; int32_t l; int g = 0;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &r) || !get_i32(env, a[1], &l)) return nullptr;
    VPT_CHECK(vpt_renderer_global_row(r, l, &g));
    return number(env, g);
}
static napi_value RendererSetVolume(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_renderer *r; vpt_volume *v;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &r) || !get_handle(env, a[1], &v, true)) return nullptr;
    VPT_CHECK(vpt_renderer_set_volume(r, v));
    return undefined(env);
}
static napi_value RendererSetImage(napi_env env, napi_callback_info info, bool tf) {
    napi_value a[4]; vpt_renderer *r; void *data; size_t n; int32_t w, h;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &r) || !get_bytes(env, a[1], &data, &n) || !get_i32(env, a[2], &w) ||
        !get_i32(env, a[3], &h)) return nullptr;
    if (w < 1 || h < 1 || n < (size_t)w * (size_t)h * 4) { napi_throw_range_error(env, nullptr, "image data shorter than width*height*4"); return nullptr; }
    if (tf) VPT_CHECK(vpt_renderer_set_transfer_function(r, (const uint8_t *)data, w, h));
    else VPT_CHECK(vpt_renderer_set_environment(r, (const uint8_t *)data, w, h));
    return undefined(env);
}
static napi_value RendererSetTransferFunction(napi_env env, napi_callback_info info) { return RendererSetImage(env, info, true); }
static napi_value RendererSetEnvironment(napi_env env, napi_callback_info info) { return RendererSetImage(env, info, false); }
// (r, data, width, height, format): HDR environment maps (VPT_ENV_*); data holds width * height texels of 4, 8 or 16 bytes
static napi_value RendererSetEnvironmentTexels(napi_env env, napi_callback_info info) {
    napi_value a[5]; vpt_renderer *r; void *data; size_t n; int32_t w, h, format;
    if (!get_args(env, info, 5, a) || !get_handle(env, a[0], &r) || !get_bytes(env, a[1], &data, &n) || !get_i32(env, a[2], &w) ||
        !get_i32(env, a[3], &h) || !get_i32(env, a[4], &format)) return nullptr;
    static const size_t texel_bytes[] = { 4, 8, 16, 4 };
    if (format >= VPT_ENV_RGBA8 && format <= VPT_ENV_RGBE8 && w >= 1 && h >= 1 && n < (size_t)w * (size_t)h * texel_bytes[format]) {
        char msg[96];
        snprintf(msg, sizeof msg, "environment data shorter than width*height*%zu bytes", texel_bytes[format]);
        napi_throw_range_error(env, nullptr, msg);
        return nullptr;
    }
    VPT_CHECK(vpt_renderer_set_environment_texels(r, data, w, h, format));   // (an unknown format or size: the library's error)
    return undefined(env);
}
static napi_value RendererResize(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_renderer *r; int32_t w, h;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &r) || !get_i32(env, a[1], &w) || !get_i32(env, a[2], &h)) return nullptr;
    VPT_CHECK(vpt_renderer_resize(r, w, h));
    return undefined(env);
}
typedef int (*pass_fn)(vpt_renderer *, const vpt_uniforms *);
static napi_value RendererPass(napi_env env, napi_callback_info info, pass_fn fn, bool allow_null) {
    napi_value a[2]; vpt_renderer *r; const vpt_uniforms *u;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &r) || !get_uniforms(env, a[1], &u, allow_null)) return nullptr;
    VPT_CHECK(fn(r, u));
    return undefined(env);
}
static napi_value RendererReset(napi_env env, napi_callback_info info) { return RendererPass(env, info, vpt_renderer_reset, true); }
static napi_value RendererGenerate(napi_env env, napi_callback_info info) { return RendererPass(env, info, vpt_renderer_generate, false); }
static napi_value RendererIntegrate(napi_env env, napi_callback_info info) { return RendererPass(env, info, vpt_renderer_integrate, false); }
static napi_value RendererRenderFrame(napi_env env, napi_callback_info info) { return RendererPass(env, info, vpt_renderer_render_frame, true); }
static napi_value RendererRender(napi_env env, napi_callback_info info) { return RendererPass(env, info, vpt_renderer_render, false); }
static napi_value RendererRead(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_renderer *r; int32_t which; void *dst; size_t n;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &r) || !get_i32(env, a[1], &which) || !get_bytes(env, a[2], &dst, &n)) return nullptr;
    VPT_CHECK(vpt_renderer_read(r, which, dst, n));
    return undefined(env);
}
static napi_value RendererReadFrameSlot(napi_env env, napi_callback_info info) {      // vpt_renderer_read_frame_slot (VPT_PLAY_FRAMES)
    napi_value a[3]; vpt_renderer *r; int32_t slot; void *dst; size_t n;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &r) || !get_i32(env, a[1], &slot) || !get_bytes(env, a[2], &dst, &n)) return nullptr;
    VPT_CHECK(vpt_renderer_read_frame_slot(r, slot, dst, n));
    return undefined(env);
}
static napi_value RendererSampleCount(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_renderer *r; uint64_t n = 0;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &r)) return nullptr;
    VPT_CHECK(vpt_renderer_sample_count(r, &n));
    return number(env, (double)n);
}
static napi_value RendererClearSampleCount(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_renderer *r;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &r)) return nullptr;
    VPT_CHECK(vpt_renderer_clear_sample_count(r));
    return undefined(env);
}
static napi_value RendererSetProfiling(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_renderer *r; int32_t on;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &r) || !get_i32(env, a[1], &on)) return nullptr;
    VPT_CHECK(vpt_renderer_set_profiling(r, on));
    return undefined(env);
}
static napi_value RendererProfile(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_renderer *r; double ms = 0; uint32_t n = 0;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &r)) return nullptr;
    VPT_CHECK(vpt_renderer_profile(r, &ms, &n));
    napi_value o; napi_create_object(env, &o);
    napi_set_named_property(env, o, "totalMs", number(env, ms));
    napi_set_named_property(env, o, "launches", number(env, n));
    return o;
}

static napi_value RendererSetOption(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_renderer *r; int32_t opt, val;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &r) || !get_i32(env, a[1], &opt) || !get_i32(env, a[2], &val)) return nullptr;
    VPT_CHECK(vpt_renderer_set_option(r, opt, val));
    return undefined(env);
}
// rendererSetLaoParams(handle, params: a 48-byte view laid out as struct vpt_lao_params)
static napi_value RendererSetLaoParams(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_renderer *r; void *p; size_t n;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &r) || !get_bytes(env, a[1], &p, &n)) return nullptr;
    if (n != sizeof(vpt_lao_params)) { napi_throw_range_error(env, nullptr, "LAO parameter block must be sizeof(struct vpt_lao_params) bytes"); return nullptr; }
    VPT_CHECK(vpt_renderer_set_lao_params(r, (const vpt_lao_params *)p));
    return undefined(env);
}
// rendererSetOcclusionSamples(handle, xy: Float32Array of 2 floats per sample) — DOSRenderer.js:103-140
static napi_value RendererSetOcclusionSamples(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_renderer *r; void *p; size_t n;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &r) || !get_bytes(env, a[1], &p, &n)) return nullptr;
    if (n % (2 * sizeof(float)) != 0) { napi_throw_range_error(env, nullptr, "occlusion samples are 2 floats each"); return nullptr; }
    VPT_CHECK(vpt_renderer_set_occlusion_samples(r, (const float *)p, (int)(n / (2 * sizeof(float)))));
    return undefined(env);
}
// rendererIntegrateSlices(handle, uniforms, slices: Float32Array of 3 floats per slice) — DOSRenderer.js:199-259
static napi_value RendererIntegrateSlices(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_renderer *r; const vpt_uniforms *u; void *p; size_t n;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &r) || !get_uniforms(env, a[1], &u, false) || !get_bytes(env, a[2], &p, &n)) return nullptr;
    if (n % (3 * sizeof(float)) != 0) { napi_throw_range_error(env, nullptr, "slices are 3 floats each"); return nullptr; }
    VPT_CHECK(vpt_renderer_integrate_slices(r, u, (const float *)p, (int)(n / (3 * sizeof(float)))));
    return undefined(env);
}
// rendererPlay(handle, baseUniforms, frameVars: Float32Array of 8 floats per frame, useGraph)
static bool get_frame_vars(napi_env env, napi_value v, const float **vars, int *count) {
    void *p; size_t n;
    if (!get_bytes(env, v, &p, &n)) return false;
    if (n == 0 || n % (8 * sizeof(float)) != 0) { napi_throw_range_error(env, nullptr, "frame variables are 8 floats per frame"); return false; }
    *vars = (const float *)p; *count = (int)(n / (8 * sizeof(float)));
    return true;
}
static napi_value RendererPlay(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_renderer *r; const vpt_uniforms *u; const float *vars; int count; int32_t graph;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &r) || !get_uniforms(env, a[1], &u, false) ||
        !get_frame_vars(env, a[2], &vars, &count) || !get_i32(env, a[3], &graph)) return nullptr;
    VPT_CHECK(vpt_renderer_play(r, u, vars, count, graph));
    return undefined(env);
}

// ---- tone mappers -------------------------------------------------------------------------------------
static napi_value TonemapperCreate(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_context *c; int32_t kind, w, h;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &c) || !get_i32(env, a[1], &kind) || !get_i32(env, a[2], &w) ||
        !get_i32(env, a[3], &h)) return nullptr;
    vpt_tonemapper *t = nullptr;
    VPT_CHECK(vpt_tonemapper_create(c, kind, w, h, &t));
    return make_external(env, t);
}
static napi_value TonemapperDestroy(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_tonemapper *t;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &t)) return nullptr;
    VPT_CHECK(vpt_tonemapper_destroy(t));
    return undefined(env);
}
static napi_value TonemapperResize(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_tonemapper *t; int32_t w, h;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &t) || !get_i32(env, a[1], &w) || !get_i32(env, a[2], &h)) return nullptr;
    VPT_CHECK(vpt_tonemapper_resize(t, w, h));
    return undefined(env);
}
static napi_value TonemapperSetSource(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_tonemapper *t; vpt_renderer *r;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &t) || !get_handle(env, a[1], &r, true)) return nullptr;
    VPT_CHECK(vpt_tonemapper_set_source(t, r));
    return undefined(env);
}
static napi_value TonemapperSetSourceImage(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_tonemapper *t; void *data; size_t n; int32_t w, rows;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &t) || !get_bytes(env, a[1], &data, &n) || !get_i32(env, a[2], &w) ||
        !get_i32(env, a[3], &rows)) return nullptr;
    if (w < 1 || rows < 1 || n < (size_t)w * (size_t)rows * 8) { napi_throw_range_error(env, nullptr, "image data shorter than width*rows*8"); return nullptr; }
    VPT_CHECK(vpt_tonemapper_set_source_image(t, data, w, rows));
    return undefined(env);
}
// tonemapperRender(handle, params: Float32Array(8) = low, mid, high, saturation, min, max, exposure, gamma)
static napi_value TonemapperRender(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_tonemapper *t; void *p; size_t n;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &t) || !get_bytes(env, a[1], &p, &n)) return nullptr;
    if (n < sizeof(vpt_tonemap_params)) { napi_throw_range_error(env, nullptr, "parameter block is smaller than struct vpt_tonemap_params"); return nullptr; }
    VPT_CHECK(vpt_tonemapper_render(t, (const vpt_tonemap_params *)p));
    return undefined(env);
}
static napi_value TonemapperSetOption(napi_env env, napi_callback_info info) {
    napi_value a[3]; vpt_tonemapper *t; int32_t opt, val;
    if (!get_args(env, info, 3, a) || !get_handle(env, a[0], &t) || !get_i32(env, a[1], &opt) || !get_i32(env, a[2], &val)) return nullptr;
    VPT_CHECK(vpt_tonemapper_set_option(t, opt, val));
    return undefined(env);
}
static napi_value TonemapperRows(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_tonemapper *t; int rows = 0;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &t)) return nullptr;
    VPT_CHECK(vpt_tonemapper_rows(t, &rows));
    return number(env, rows);
}
static napi_value TonemapperRead(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_tonemapper *t; void *dst; size_t n;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &t) || !get_bytes(env, a[1], &dst, &n)) return nullptr;
    VPT_CHECK(vpt_tonemapper_read(t, dst, n));
    return undefined(env);
}

// transferFunctionRasterize(ctx, bumps: Float32Array [count][8], width, height, unpremultiply, out: Uint8Array [height][width][4])
static napi_value TransferFunctionRasterize(napi_env env, napi_callback_info info) {
    napi_value a[6]; vpt_context *c; void *bumps, *dst; size_t nb, nd; int32_t w, h, unpre;
    if (!get_args(env, info, 6, a) || !get_handle(env, a[0], &c) || !get_bytes(env, a[1], &bumps, &nb) || !get_i32(env, a[2], &w) ||
        !get_i32(env, a[3], &h) || !get_i32(env, a[4], &unpre) || !get_bytes(env, a[5], &dst, &nd)) return nullptr;
    if (w < 1 || h < 1 || nd < (size_t)w * (size_t)h * 4) { napi_throw_range_error(env, nullptr, "the output holds width * height * 4 bytes"); return nullptr; }
    VPT_CHECK(vpt_transfer_function_rasterize(c, (const vpt_tf_bump *)bumps, (int)(nb / sizeof(vpt_tf_bump)), w, h, unpre, (uint8_t *)dst));
    return undefined(env);
}

// ---- multi-GPU frame gather ---------------------------------------------------------------------------
static napi_value GatherUniqueId(napi_env env, napi_callback_info info) {
    (void)info;
    void *data; napi_value ab;
    NAPI_OK(napi_create_arraybuffer(env, 128, &data, &ab));
    VPT_CHECK(vpt_gather_unique_id(data));
    return ab;
}
static napi_value GatherCreate(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_renderer *r; void *id; size_t n; int32_t rank, world;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &r) || !get_bytes(env, a[1], &id, &n) || !get_i32(env, a[2], &rank) ||
        !get_i32(env, a[3], &world)) return nullptr;
    if (n < 128) { napi_throw_range_error(env, nullptr, "the RCCL unique id is 128 bytes"); return nullptr; }
    vpt_gather *g = nullptr;
    VPT_CHECK(vpt_gather_create(r, id, rank, world, &g));
    return make_external(env, g);
}
static napi_value GatherDestroy(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_gather *g;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &g)) return nullptr;
    VPT_CHECK(vpt_gather_destroy(g));
    return undefined(env);
}
static napi_value GatherSetRoot(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_gather *g; int32_t root;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &g) || !get_i32(env, a[1], &root)) return nullptr;
    VPT_CHECK(vpt_gather_set_root(g, root));
    return undefined(env);
}
static napi_value GatherRender(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_gather *g; const vpt_uniforms *u;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &g) || !get_uniforms(env, a[1], &u, false)) return nullptr;
    VPT_CHECK(vpt_gather_render(g, u));
    return undefined(env);
}
static napi_value GatherPlay(napi_env env, napi_callback_info info) {
    napi_value a[4]; vpt_gather *g; const vpt_uniforms *u; const float *vars; int count; int32_t mode;
    if (!get_args(env, info, 4, a) || !get_handle(env, a[0], &g) || !get_uniforms(env, a[1], &u, false) ||
        !get_frame_vars(env, a[2], &vars, &count) || !get_i32(env, a[3], &mode)) return nullptr;
    VPT_CHECK(vpt_gather_play(g, u, vars, count, mode));
    return undefined(env);
}
static napi_value GatherSynchronize(napi_env env, napi_callback_info info) {
    napi_value a[1]; vpt_gather *g;
    if (!get_args(env, info, 1, a) || !get_handle(env, a[0], &g)) return nullptr;
    VPT_CHECK(vpt_gather_synchronize(g));
    return undefined(env);
}
static napi_value GatherReadFrame(napi_env env, napi_callback_info info) {
    napi_value a[2]; vpt_gather *g; void *dst; size_t n;
    if (!get_args(env, info, 2, a) || !get_handle(env, a[0], &g) || !get_bytes(env, a[1], &dst, &n)) return nullptr;
    VPT_CHECK(vpt_gather_read_frame(g, dst, n));
    return undefined(env);
}

#define EXPORT(name, fn) do { napi_value f; napi_create_function(env, name, NAPI_AUTO_LENGTH, fn, nullptr, &f); \
                              napi_set_named_property(env, exports, name, f); } while (0)
#define CONST(name) do { napi_set_named_property(env, exports, #name, number(env, name)); } while (0)

static napi_value Init(napi_env env, napi_value exports) {
    EXPORT("deviceCount", DeviceCount); EXPORT("contextCreate", ContextCreate); EXPORT("contextDestroy", ContextDestroy);
    EXPORT("contextSynchronize", ContextSynchronize); EXPORT("version", Version);
    EXPORT("volumeCreate", VolumeCreate); EXPORT("volumeUploadBlock", VolumeUploadBlock); EXPORT("volumeFinalize", VolumeFinalize);
    EXPORT("volumeSetFilter", VolumeSetFilter); EXPORT("volumeDestroy", VolumeDestroy); EXPORT("volumeBrickedBytes", VolumeBrickedBytes);
    EXPORT("volumeDeriveGradient", VolumeDeriveGradient); EXPORT("volumeReadBlock", VolumeReadBlock); EXPORT("volumeHistogram", VolumeHistogram);
    CONST(VPT_GRADIENT_CENTRAL); CONST(VPT_GRADIENT_SOBEL);
    EXPORT("volumeWindow", VolumeWindow); EXPORT("volumeRange", VolumeRange); EXPORT("volumeCodeHistogram", VolumeCodeHistogram);
    EXPORT("volumeReduce", VolumeReduce); EXPORT("volumeSmooth", VolumeSmooth); EXPORT("volumeRank", VolumeRank); EXPORT("volumeResample", VolumeResample);
    EXPORT("volumeCombine", VolumeCombine); EXPORT("volumeCombineTimed", VolumeCombineTimed); EXPORT("volumeCompare", VolumeCompare);
    EXPORT("volumeReconstruct", VolumeReconstruct); EXPORT("volumeReconstructTimed", VolumeReconstructTimed);
    EXPORT("volumeGeodesic", VolumeGeodesic); EXPORT("volumeGeodesicTimed", VolumeGeodesicTimed);
    EXPORT("volumeWatershed", VolumeWatershed); EXPORT("volumeWatershedTimed", VolumeWatershedTimed);
    EXPORT("volumeComponents", VolumeComponents); EXPORT("componentsInfo", ComponentsInfo); EXPORT("componentsList", ComponentsList);
    EXPORT("componentsRanks", ComponentsRanks); EXPORT("componentsKeep", ComponentsKeep); EXPORT("componentsLabel", ComponentsLabel);
    EXPORT("componentsMeasure", ComponentsMeasure); EXPORT("componentsMeasureTimed", ComponentsMeasureTimed); EXPORT("componentsKeepSet", ComponentsKeepSet);
    EXPORT("componentsDestroy", ComponentsDestroy);
    EXPORT("volumeDistance", VolumeDistance); EXPORT("distanceInfo", DistanceInfo); EXPORT("distanceSquared", DistanceSquared);
    EXPORT("distanceWithin", DistanceWithin); EXPORT("distanceChannel", DistanceChannel); EXPORT("distanceProfile", DistanceProfile);
    EXPORT("distanceDestroy", DistanceDestroy); EXPORT("distanceThickness", DistanceThickness); EXPORT("distanceThicknessTimed", DistanceThicknessTimed);
    EXPORT("volumeSkeleton", VolumeSkeleton); EXPORT("skeletonInfo", SkeletonInfo); EXPORT("skeletonBurn", SkeletonBurn); EXPORT("skeletonWithin", SkeletonWithin);
    EXPORT("skeletonProfile", SkeletonProfile); EXPORT("skeletonDestroy", SkeletonDestroy);
    EXPORT("volumeGraph", VolumeGraph); EXPORT("skeletonGraph", SkeletonGraph); EXPORT("graphInfo", GraphInfo); EXPORT("graphBranches", GraphBranches);
    EXPORT("graphNodes", GraphNodes); EXPORT("graphComponents", GraphComponents); EXPORT("graphClasses", GraphClasses); EXPORT("graphPrune", GraphPrune);
    EXPORT("graphProfile", GraphProfile); EXPORT("graphDestroy", GraphDestroy);
    EXPORT("volumeSurface", VolumeSurface); EXPORT("surfaceInfo", SurfaceInfo); EXPORT("surfaceVertices", SurfaceVertices); EXPORT("surfaceQuads", SurfaceQuads);
    EXPORT("surfaceProfile", SurfaceProfile); EXPORT("surfaceDestroy", SurfaceDestroy);
    EXPORT("rendererCreate", RendererCreate); EXPORT("rendererDestroy", RendererDestroy); EXPORT("rendererSetShard", RendererSetShard);
    EXPORT("rendererLocalRows", RendererLocalRows); EXPORT("rendererGlobalRow", RendererGlobalRow);
    EXPORT("rendererSetVolume", RendererSetVolume); EXPORT("rendererSetTransferFunction", RendererSetTransferFunction);
    EXPORT("rendererSetEnvironment", RendererSetEnvironment); EXPORT("rendererResize", RendererResize);
    EXPORT("rendererSetEnvironmentTexels", RendererSetEnvironmentTexels);
    CONST(VPT_ENV_RGBA8); CONST(VPT_ENV_RGBA16F); CONST(VPT_ENV_RGBA32F); CONST(VPT_ENV_RGBE8);
    EXPORT("rendererReset", RendererReset); EXPORT("rendererGenerate", RendererGenerate); EXPORT("rendererIntegrate", RendererIntegrate);
    EXPORT("rendererRenderFrame", RendererRenderFrame); EXPORT("rendererRender", RendererRender); EXPORT("rendererRead", RendererRead); EXPORT("rendererReadFrameSlot", RendererReadFrameSlot);
    EXPORT("rendererSampleCount", RendererSampleCount); EXPORT("rendererClearSampleCount", RendererClearSampleCount);
    EXPORT("rendererSetProfiling", RendererSetProfiling); EXPORT("rendererProfile", RendererProfile);
    EXPORT("rendererSetOption", RendererSetOption); EXPORT("rendererSetLaoParams", RendererSetLaoParams);
    EXPORT("rendererSetOcclusionSamples", RendererSetOcclusionSamples); EXPORT("rendererIntegrateSlices", RendererIntegrateSlices); EXPORT("rendererPlay", RendererPlay);
    EXPORT("tonemapperCreate", TonemapperCreate); EXPORT("tonemapperDestroy", TonemapperDestroy); EXPORT("tonemapperResize", TonemapperResize);
    EXPORT("tonemapperSetSource", TonemapperSetSource); EXPORT("tonemapperSetSourceImage", TonemapperSetSourceImage);
    EXPORT("tonemapperSetOption", TonemapperSetOption); CONST(VPT_TONEMAPPER_OPTION_TABLE); CONST(VPT_TONEMAPPER_OPTION_FUSE); CONST(VPT_TONEMAPPER_TABLE_NEVER);
    CONST(VPT_TONEMAPPER_TABLE_ALWAYS); CONST(VPT_TONEMAPPER_TABLE_AUTO);
    EXPORT("tonemapperRender", TonemapperRender); EXPORT("tonemapperRows", TonemapperRows); EXPORT("tonemapperRead", TonemapperRead);
    EXPORT("transferFunctionRasterize", TransferFunctionRasterize);
    CONST(VPT_TONEMAPPER_ARTISTIC); CONST(VPT_TONEMAPPER_RANGE); CONST(VPT_TONEMAPPER_REINHARD); CONST(VPT_TONEMAPPER_REINHARD2);
    CONST(VPT_TONEMAPPER_UNCHARTED2); CONST(VPT_TONEMAPPER_FILMIC); CONST(VPT_TONEMAPPER_UNREAL); CONST(VPT_TONEMAPPER_ACES);
    CONST(VPT_TONEMAPPER_LOTTES); CONST(VPT_TONEMAPPER_UCHIMURA);
    EXPORT("gatherUniqueId", GatherUniqueId); EXPORT("gatherCreate", GatherCreate); EXPORT("gatherDestroy", GatherDestroy);
    EXPORT("gatherSetRoot", GatherSetRoot); EXPORT("gatherRender", GatherRender); EXPORT("gatherPlay", GatherPlay); EXPORT("gatherSynchronize", GatherSynchronize);
    EXPORT("gatherReadFrame", GatherReadFrame);
    CONST(VPT_OPTION_MCS_PERSISTENT); CONST(VPT_OPTION_MCM_PERSISTENT); CONST(VPT_OPTION_FAST_MATH); CONST(VPT_OPTION_BOUNDARY_ATLAS); CONST(VPT_OPTION_SPLIT_STREAMS); CONST(VPT_OPTION_TILE_CLASSES); CONST(VPT_OPTION_VERIFY_TILE_CLASSES); CONST(VPT_OPTION_BUCKET_KERNEL); CONST(VPT_OPTION_COLUMN_RECORDS);
    CONST(VPT_PLAY_EAGER); CONST(VPT_PLAY_GRAPH); CONST(VPT_PLAY_FUSED); CONST(VPT_PLAY_FRAMES); CONST(VPT_FRAME_SLOTS);
    CONST(VPT_RENDERER_MIP); CONST(VPT_RENDERER_EAM); CONST(VPT_RENDERER_MCS); CONST(VPT_RENDERER_MCM);
    CONST(VPT_RENDERER_ISO); CONST(VPT_RENDERER_DEPTH); CONST(VPT_RENDERER_LAO); CONST(VPT_RENDERER_DOS); CONST(VPT_BUFFER_DOS_OCCLUSION);
    CONST(VPT_FILTER_NEAREST); CONST(VPT_FILTER_LINEAR); CONST(VPT_FILTER_QUASI_CUBIC); CONST(VPT_FORMAT_R8); CONST(VPT_FORMAT_RG8); CONST(VPT_FORMAT_R32F); CONST(VPT_FORMAT_RG32F);
    CONST(VPT_FORMAT_R8_SNORM); CONST(VPT_FORMAT_RG8_SNORM); CONST(VPT_FORMAT_RGB565); CONST(VPT_FORMAT_RGBA4); CONST(VPT_FORMAT_RGB5_A1);
    CONST(VPT_FORMAT_RGB10_A2); CONST(VPT_FORMAT_R11F_G11F_B10F); CONST(VPT_FORMAT_RGB9_E5);
    CONST(VPT_FORMAT_R16); CONST(VPT_FORMAT_RG16); CONST(VPT_FORMAT_R16_SNORM); CONST(VPT_FORMAT_RG16_SNORM);
    CONST(VPT_BUFFER_RENDER); CONST(VPT_BUFFER_FRAME); CONST(VPT_BUFFER_ACCUM);
    CONST(VPT_BUFFER_MCM_POSITION); CONST(VPT_BUFFER_MCM_DIRECTION); CONST(VPT_BUFFER_MCM_TRANSMITTANCE); CONST(VPT_BUFFER_MCM_RADIANCE);
    napi_set_named_property(env, exports, "UNIFORMS_BYTES", number(env, (double)sizeof(vpt_uniforms)));
    return exports;
}
NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
