// vpt_mcm_hit.hip — the MCM integrate kernels (k_mcm_integrate, k_mcm_integrate_early: vpt_kernels_mcm.h) in a translation unit of
// their own: every volume format x wide tables x fast-math x column records, with and without the fused _renderFrame.  vpt_mcm.hip asks for
// one by variant.  MCMRenderer.glsl:116-172.
#include "vpt_mcm_select.h"
#include "vpt_kernels_mcm.h"

template <bool FUSE> static PassKernel hit_kernel(int v, bool early) {
    return dispatch_variant<VPT_V_CLASS_BITS>(v, [&](auto V) { return early ? (PassKernel)k_mcm_integrate_early<FUSE, V()> : (PassKernel)k_mcm_integrate<FUSE, V()>; },
                                              no_pass_kernel);
}
PassKernel mcm_hit_kernel(bool fuse, int v, bool early) { return fuse ? hit_kernel<true>(v, early) : hit_kernel<false>(v, early); }
template <bool FUSE> static PassKernel general_kernel(int v, bool fast) {
    return dispatch_sampler_variant(v, [&](auto V) { return fast ? (PassKernel)k_mcm_integrate<FUSE, V() | VPT_V_FAST> : (PassKernel)k_mcm_integrate<FUSE, V()>; },
                                    no_pass_kernel);
}
PassKernel mcm_general_kernel(bool fuse, int v, bool fast) { return fuse ? general_kernel<true>(v, fast) : general_kernel<false>(v, fast); }
// one pass over the whole image (no tile classes in force): the general kernel of the renderer's variant, split over the side streams
// like every sampling kernel (launch_sampling)
int mcm_general_pass(vpt_renderer *r, const PassArgs &a, bool fuse) {
    // (column records: LINEAR one-channel byte volume, variant_of is 0 or VPT_V_WIDE, and the kernel is the class variant's)
    const PassKernel k = a.vol.records ? mcm_hit_kernel(fuse, class_variant(r, a), false) : mcm_general_kernel(fuse, variant_of(r), r->fast_math != 0);
    if (!k) return fail(VPT_ERR_INVALID, "no sampling kernel for variant %d", variant_of(r));
    return launch_sampling(k, r, a);
}
