// vpt_mcm_seq.hip — MCM frame sequences in one launch (vpt_renderer_play with VPT_PLAY_FUSED / VPT_PLAY_FRAMES): k_mcm_multi and
// k_mcm_frames (vpt_kernels_mcm.h) keep the photon state in registers over the passes.  AbstractRenderer.js:60-70 called n times.
#include "vpt_mcm_select.h"
#include "vpt_kernels_mcm.h"

template <typename K>
static int launch_multi(K kernel, vpt_renderer *r, const PassArgs &a, uint32_t npasses) {
    const size_t lds = lds_bytes(r);
    VPT_TRY(lds_prepare((const void *)kernel, lds));
    hipLaunchKernelGGL(kernel, tile_grid(r), dim3(VPT_BLOCK), lds, r->ctx->stream, a, npasses);
    return VPT_OK;
}
template <typename K>
static int launch_frames(K kernel, vpt_renderer *r, const PassArgs &a, uint32_t npasses, uint2 *ring) {
    const size_t lds = lds_bytes(r);
    VPT_TRY(lds_prepare((const void *)kernel, lds));
    hipLaunchKernelGGL(kernel, tile_grid(r), dim3(VPT_BLOCK), lds, r->ctx->stream, a, npasses, ring, (uint32_t)((size_t)r->W * r->local_h));
    return VPT_OK;
}
int mcm_multi(vpt_renderer *r, const PassArgs &a, uint32_t npasses, uint2 *ring) {
    r->tm_valid = false;
    VPT_TRY(mcm_before_pass(r, a, nullptr));
    VPT_TRY(mcm_materialize(r));                      // a whole-image kernel: every tile's full photon state
    VPT_TRY(streams_deal(r, Deal{ DEAL_ROWS, 1 }));   // one stream: the side streams are joined first
    auto launch = [&](auto V) { return ring ? launch_frames(k_mcm_frames<V()>, r, a, npasses, ring) : launch_multi(k_mcm_multi<V()>, r, a, npasses); };
    auto none = [&] { return fail(VPT_ERR_INVALID, "no frame-sequence kernel for variant %d", variant_of(r)); };
    mcm_events_run(r, (uint64_t)a.steps * npasses);
    if (a.vol.records) return dispatch_variant<VPT_V_CLASS_BITS>(class_variant(r, a), launch, none);   // column records: LINEAR one-channel byte volumes
    if (r->fast_math) return dispatch_sampler_variant(variant_of(r), [&](auto V) { return launch(std::integral_constant<int, V() | VPT_V_FAST>{}); }, none);
    return dispatch_sampler_variant(variant_of(r), launch, none);
}
