// vpt_mcm_select.h — what the MCM translation units (vpt_mcm.hip: tile classes, buckets; vpt_mcm_hit.hip: the integrate kernels;
// vpt_mcm_seq.hip: frame sequences in one launch) share on the host side: the sampler variant of a renderer's tile-class kernels and the
// lookup of an integrate kernel by variant (the switch from the run-time value to the template argument: vpt_variants.h).
#pragma once
#include "vpt_internal.h"

typedef void (*PassKernel)(PassArgs);
// the sampler variant of the tile-class kernels (LINEAR one-channel byte volumes): VPT_V_WIDE | VPT_V_FAST | VPT_V_REC
static inline int class_variant(const vpt_renderer *r, const PassArgs &a) {
    return (variant_of(r) & VPT_V_WIDE) | (r->fast_math ? VPT_V_FAST : 0) | (a.vol.records ? VPT_V_REC : 0);
}
#define VPT_V_CLASS_BITS (VPT_V_WIDE | VPT_V_FAST | VPT_V_REC)
static inline PassKernel no_pass_kernel() { return nullptr; }              // what a kernel lookup answers for a variant that has none
// vpt_mcm_hit.hip: the integrate kernels by variant (fuse: + _renderFrame); null: no such variant
PassKernel mcm_hit_kernel(bool fuse, int v, bool early);                   // v: class_variant(): k_mcm_integrate / k_mcm_integrate_early
PassKernel mcm_general_kernel(bool fuse, int v, bool fast);                // v: variant_of(): the general kernel k_mcm_integrate<fuse, v (| VPT_V_FAST)> of any volume format
int mcm_general_pass(vpt_renderer *r, const PassArgs &a, bool fuse);       // the whole image through the general kernel
