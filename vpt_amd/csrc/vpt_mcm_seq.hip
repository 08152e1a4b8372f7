// vpt_mcm_seq.hip — MCM frame sequences in one launch (vpt_renderer_play with VPT_PLAY_FUSED / VPT_PLAY_FRAMES): k_mcm_multi and
// k_mcm_frames (vpt_kernels_mcm.h) keep the photon state in registers over the passes.  AbstractRenderer.js:60-70 called n times.
#include "vpt_mcm_select.h"
#include "vpt_kernels_mcm.h"

template <typename K>
static int launch_multi(K kernel, vpt_renderer *r, const PassArgs &a, uint32_t npasses) {
    size_t lds = lds_bytes(r);
    if (lds > 160 * 1024) return fail(VPT_ERR_UNSUPPORTED, "transfer function + volume tables need %zu B of LDS (> 160 KiB)", lds);
    if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, tile_grid(r), dim3(VPT_BLOCK), lds, r->ctx->stream, a, npasses);
    return VPT_OK;
}
template <typename K>
static int launch_frames(K kernel, vpt_renderer *r, const PassArgs &a, uint32_t npasses, uint2 *ring) {
    size_t lds = lds_bytes(r);
    if (lds > 160 * 1024) return fail(VPT_ERR_UNSUPPORTED, "transfer function + volume tables need %zu B of LDS (> 160 KiB)", lds);
    if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, tile_grid(r), dim3(VPT_BLOCK), lds, r->ctx->stream, a, npasses, ring, (uint32_t)((size_t)r->W * r->local_h));
    return VPT_OK;
}
int mcm_multi(vpt_renderer *r, const PassArgs &a, uint32_t npasses, uint2 *ring) {
    r->tm_valid = false;
    VPT_TRY(mcm_before_pass(r, a, nullptr));
    VPT_TRY(mcm_materialize(r));                      // a whole-image kernel: every tile's full photon state
    VPT_TRY(streams_deal(r, Deal{ DEAL_ROWS, 1 }));   // one stream: the side streams are joined first
    if (a.vol.records) {                              // column records: LINEAR one-channel byte volumes
        const int v = class_variant(r, a);
        VARIANT_CASES(ring ? launch_frames(k_mcm_frames<V>, r, a, npasses, ring) : launch_multi(k_mcm_multi<V>, r, a, npasses))
    }
#define MULTI_CASE(v, F) case v: return ring ? launch_frames(k_mcm_frames<v | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<v | F>, r, a, npasses);
#define MULTI_CASES(F) switch (variant_of(r)) { \
        case 0: return ring ? launch_frames(k_mcm_frames<0 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<0 | F>, r, a, npasses); \
        case 1: return ring ? launch_frames(k_mcm_frames<1 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<1 | F>, r, a, npasses); \
        case 2: return ring ? launch_frames(k_mcm_frames<2 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<2 | F>, r, a, npasses); \
        case 3: return ring ? launch_frames(k_mcm_frames<3 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<3 | F>, r, a, npasses); \
        case 8: return ring ? launch_frames(k_mcm_frames<8 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<8 | F>, r, a, npasses); \
        case 9: return ring ? launch_frames(k_mcm_frames<9 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<9 | F>, r, a, npasses); \
        case 10: return ring ? launch_frames(k_mcm_frames<10 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<10 | F>, r, a, npasses); \
        case 11: return ring ? launch_frames(k_mcm_frames<11 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<11 | F>, r, a, npasses); \
        case 32: return ring ? launch_frames(k_mcm_frames<32 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<32 | F>, r, a, npasses); \
        case 33: return ring ? launch_frames(k_mcm_frames<33 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<33 | F>, r, a, npasses); \
        case 34: return ring ? launch_frames(k_mcm_frames<34 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<34 | F>, r, a, npasses); \
        case 35: return ring ? launch_frames(k_mcm_frames<35 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<35 | F>, r, a, npasses); \
        case 40: return ring ? launch_frames(k_mcm_frames<40 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<40 | F>, r, a, npasses); \
        case 41: return ring ? launch_frames(k_mcm_frames<41 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<41 | F>, r, a, npasses); \
        case 42: return ring ? launch_frames(k_mcm_frames<42 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<42 | F>, r, a, npasses); \
        case 43: return ring ? launch_frames(k_mcm_frames<43 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<43 | F>, r, a, npasses); \
        case 128: return ring ? launch_frames(k_mcm_frames<128 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<128 | F>, r, a, npasses); \
        case 129: return ring ? launch_frames(k_mcm_frames<129 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<129 | F>, r, a, npasses); \
        case 130: return ring ? launch_frames(k_mcm_frames<130 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<130 | F>, r, a, npasses); \
        case 131: return ring ? launch_frames(k_mcm_frames<131 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<131 | F>, r, a, npasses); \
        case 136: return ring ? launch_frames(k_mcm_frames<136 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<136 | F>, r, a, npasses); \
        case 137: return ring ? launch_frames(k_mcm_frames<137 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<137 | F>, r, a, npasses); \
        case 138: return ring ? launch_frames(k_mcm_frames<138 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<138 | F>, r, a, npasses); \
        case 139: return ring ? launch_frames(k_mcm_frames<139 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<139 | F>, r, a, npasses); \
        case 256: return ring ? launch_frames(k_mcm_frames<256 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<256 | F>, r, a, npasses); \
        case 257: return ring ? launch_frames(k_mcm_frames<257 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<257 | F>, r, a, npasses); \
        case 264: return ring ? launch_frames(k_mcm_frames<264 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<264 | F>, r, a, npasses); \
        case 265: return ring ? launch_frames(k_mcm_frames<265 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<265 | F>, r, a, npasses); \
        case 288: return ring ? launch_frames(k_mcm_frames<288 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<288 | F>, r, a, npasses); \
        case 289: return ring ? launch_frames(k_mcm_frames<289 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<289 | F>, r, a, npasses); \
        case 296: return ring ? launch_frames(k_mcm_frames<296 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<296 | F>, r, a, npasses); \
        case 297: return ring ? launch_frames(k_mcm_frames<297 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<297 | F>, r, a, npasses); \
        case 384: return ring ? launch_frames(k_mcm_frames<384 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<384 | F>, r, a, npasses); \
        case 385: return ring ? launch_frames(k_mcm_frames<385 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<385 | F>, r, a, npasses); \
        case 392: return ring ? launch_frames(k_mcm_frames<392 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<392 | F>, r, a, npasses); \
        case 393: return ring ? launch_frames(k_mcm_frames<393 | F>, r, a, npasses, ring) : launch_multi(k_mcm_multi<393 | F>, r, a, npasses); \
        VPT_NORM16_VARIANTS(MULTI_CASE, F) \
        default: return fail(VPT_ERR_INVALID, "no frame-sequence kernel for variant %d", variant_of(r)); }
    if (r->fast_math) MULTI_CASES(VPT_V_FAST)
    MULTI_CASES(0)
#undef MULTI_CASES
#undef MULTI_CASE
}

