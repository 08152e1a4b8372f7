// vpt_march.hip — the MIP, EAM and MCS renderers' passes (vpt_kernels_march.h) behind vpt_render.hip's entry points.
// MIPRenderer.js:69-100, EAMRenderer.js:88-153, MCSRenderer.js:74-140.
#include "vpt_internal.h"
#include "vpt_kernels_march.h"

// the tap form of each family, on top of the volume's variant v
// (dword-aligned 12-byte taps + v_alignbyte, VPT_V_ALIGNED, for MIP / EAM — re-measured in round 3 on the HIT tiles only, 256^3 1080p: EAM 63.7 us
// aligned against 72.3 unaligned on one stream, 52.1 / 63.3 on three; MIP 56.3 / 72.0, 45.1 / 64.1)
// (16-bit volumes with brick-code tables: the unaligned 16-byte loads — the realigned words cost EAM a wave per SIMD there, 68 against 63 VGPRs)
constexpr int eam_taps(int v) { return ((v & VPT_V_NORM16) && (v & VPT_V_WIDE)) ? 0 : VPT_V_ALIGNED; }
#ifndef VPT_MCS_TAPS
#define VPT_MCS_TAPS 0
#endif
constexpr int mcs_taps(int) { return VPT_MCS_TAPS; }
template <int MODE> static int launch_mip(vpt_renderer *r, const PassArgs &a) { return launch_variant(r, a, [](auto V) { return k_mip<MODE, V() | VPT_V_ALIGNED>; }); }
template <int MODE> static int launch_eam(vpt_renderer *r, const PassArgs &a) { return launch_variant(r, a, [](auto V) { return k_eam<MODE, V() | eam_taps(V())>; }); }
#define LAUNCH(kernel, r, a, lds) hipLaunchKernelGGL(kernel, tile_grid(r), dim3(VPT_BLOCK), (lds), (r)->ctx->stream, (a))

template <typename K>
static int launch_mcs_persist(K kernel, vpt_renderer *r, const PassArgs &a) {
    const size_t lds = lds_bytes(r);
    VPT_TRY(lds_prepare((const void *)kernel, lds));
    const size_t counter_bytes = (size_t)VPT_WORK_SHARDS * VPT_WORK_STRIDE * sizeof(uint32_t);
    if (!r->work_counter) HIP_TRY(r->work_counter.alloc(counter_bytes / sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(r->work_counter, 0, counter_bytes, r->ctx->stream));
    int ntx8 = (r->W + 7) / 8, nty8 = (r->local_h + 7) / 8, ntiles8 = ntx8 * nty8;
    int blocks = (ntiles8 + 3) / 4;
    if (blocks > 256 * 6) blocks = 256 * 6;           // persistent: every wave resident, tiles drawn from the counter
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(VPT_BLOCK), lds, r->ctx->stream, a, r->work_counter, ntx8, ntiles8);
    return VPT_OK;
}

int march_reset(vpt_renderer *r, const PassArgs &a) {
    switch (r->kind) {
        case VPT_RENDERER_MIP: LAUNCH(k_mip_reset, r, a, 0); break;
        case VPT_RENDERER_EAM: LAUNCH(k_eam_reset, r, a, 0); break;
        default: LAUNCH(k_mcs_reset, r, a, 0); break;
    }
    return VPT_OK;
}
template <int MODE> static int launch_mcs(vpt_renderer *r, const PassArgs &a) {
    if (r->mcs_persistent && persistent_volume(r->vol)) {       // (walks every tile; UNSIGNED_BYTE one-channel volumes, LINEAR or NEAREST)
        const int v = (r->vol->wide ? VPT_V_WIDE : 0) | (r->vol->filter == VPT_FILTER_NEAREST ? VPT_V_NEAREST : 0);
        return dispatch_variant<VPT_V_WIDE | VPT_V_NEAREST>(v, [&](auto V) { return launch_mcs_persist(k_mcs_persist<MODE, V()>, r, a); },
                                                            [&] { return fail(VPT_ERR_INVALID, "no persistent MCS kernel for variant %d", v); });
    }
    return launch_variant(r, a, [](auto V) { return k_mcs<MODE, V() | mcs_taps(V())>; });
}
int march_generate(vpt_renderer *r, const PassArgs &a) {                      // _generateFrame
    switch (r->kind) {
        case VPT_RENDERER_MIP: return launch_mip<0>(r, a);
        case VPT_RENDERER_EAM: return launch_eam<0>(r, a);
        default: return launch_mcs<0>(r, a);
    }
}
int march_integrate(vpt_renderer *r, const PassArgs &a) {                     // _integrateFrame
    switch (r->kind) {
        case VPT_RENDERER_MIP: LAUNCH(k_mip_integrate, r, a, 0); break;
        case VPT_RENDERER_EAM: LAUNCH(k_eam_integrate, r, a, 0); break;
        default: LAUNCH(k_mcs_integrate, r, a, 0); break;
    }
    return VPT_OK;
}
int march_render_frame(vpt_renderer *r, const PassArgs &a) {                  // _renderFrame
    switch (r->kind) {
        case VPT_RENDERER_MIP: LAUNCH(k_mip_render, r, a, 0); break;
        case VPT_RENDERER_EAM: LAUNCH(k_eam_render, r, a, 0); break;
        default: LAUNCH(k_mcs_render, r, a, 0); break;
    }
    return VPT_OK;
}
int march_fused(vpt_renderer *r, const PassArgs &a) {                         // render(): the three hooks in one launch
    switch (r->kind) {
        case VPT_RENDERER_MIP: return launch_mip<1>(r, a);
        case VPT_RENDERER_EAM: return launch_eam<1>(r, a);
        default: return launch_mcs<1>(r, a);
    }
}
