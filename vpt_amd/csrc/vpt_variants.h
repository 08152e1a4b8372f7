// vpt_variants.h — the variant bits V of the sampling kernels and the one switch from a run-time variant to a template argument.
// Nothing else: no HIP, no project header (tests/test_variants.py compiles it with the host compiler).  A new variant bit is added
// here — its definition, VPT_V_SAMPLER_BITS and sampler_variant_valid — and every launch site follows.
#pragma once
#include <type_traits>

// V: variant bits fixed at launch — bit 0 = 64-bit offset tables (WIDE), bit 1 = NEAREST filter.  No run-time branch
// inside the sampler: consecutive samples of a ray stay straight-line code, so their loads are issued together.
#define VPT_V_WIDE    1
#define VPT_V_NEAREST 2
#define VPT_V_ALIGNED 4   // fetch the two tap windows as dword-aligned 12-byte loads + v_alignbyte (texture-path bound kernels)
#define VPT_V_FAST    16  // MCM / MCS: hardware rcp / rsq / sqrt / log / sin / cos and shorter algebraic forms (no bit-exact CPU twin; VPT_OPTION_FAST_MATH)
#define VPT_V_F32     32  // FLOAT texels (R32F; R16F widened on upload): 5^3 floats in a 512-byte slot, no normalisation
#define VPT_V_RG      8   // two-channel (RG8) volume: texture(uVolume, p).rg has both channels, the transfer function is looked up in 2-D
#define VPT_V_REC     64  // in-cube samples from the column records instead of the bricks (one-channel byte volumes, LINEAR filter; MCM)
#define VPT_V_SNORM   128 // BYTE texels (R8_SNORM / RG8_SNORM): bricks as R8 / RG8, each tap decoded to fl32(c / 127) and filtered as R32F
#define VPT_V_QCUBIC  256 // quasi-cubic filter (VPT_FILTER_QUASI_CUBIC): the LINEAR cell and taps, smoothstep weights (qc_weight); never with NEAREST / REC
#define VPT_V_NORM16  512 // 16-bit normalised texels (R16 / RG16; | VPT_V_SNORM: R16_SNORM / RG16_SNORM): 5^3 words in a 256-byte slot (RG: the G
                          // brick 256 bytes behind), each tap decoded (norm16_decode) and filtered as R32F

// the sampler bits: (addressing, filter, channels, texels) of a volume, what variant_of() (vpt_internal.h) returns
#define VPT_V_SAMPLER_BITS (VPT_V_WIDE | VPT_V_NEAREST | VPT_V_RG | VPT_V_F32 | VPT_V_SNORM | VPT_V_QCUBIC | VPT_V_NORM16)
// ... and the combinations of them that exist: {32-bit, wide tables} x {LINEAR, NEAREST, QUASI_CUBIC} x {R, RG} x {u8, f32, s8, u16, s16} = 60.
// One filter at a time, and FLOAT texels are neither signed-normalised nor 16-bit.
constexpr bool sampler_variant_valid(int v) {
    return (v & ~VPT_V_SAMPLER_BITS) == 0 && !((v & VPT_V_NEAREST) && (v & VPT_V_QCUBIC)) && !((v & VPT_V_F32) && (v & (VPT_V_SNORM | VPT_V_NORM16)));
}
constexpr bool any_variant(int) { return true; }

// Run-time v -> compile-time V over the bit set BITS: returns f(std::integral_constant<int, v>{}) when v lies within BITS and VALID(v),
// else otherwise() — f is never called with another V than v, and no value falls through to some default kernel.  f is a generic callable
// (its results for every V convert to what otherwise() returns: a status, a kernel pointer).  Only the valid V are instantiated.
template <int BITS, bool (*VALID)(int) = any_variant, int V = 0, typename F, typename O>
auto dispatch_variant(int v, F &&f, O &&otherwise) -> decltype(otherwise()) {
    if constexpr (BITS != 0) {
        constexpr int B = BITS & -BITS;                   // the lowest bit not yet decided
        return (v & B) ? dispatch_variant<(BITS & ~B), VALID, (V | B)>(v, f, otherwise) : dispatch_variant<(BITS & ~B), VALID, V>(v, f, otherwise);
    } else if constexpr (VALID(V)) {
        if (v == V) return f(std::integral_constant<int, V>{});
        return otherwise();
    } else {
        return otherwise();
    }
}
// the 60 sampler variants
template <typename F, typename O>
auto dispatch_sampler_variant(int v, F &&f, O &&otherwise) -> decltype(otherwise()) {
    return dispatch_variant<VPT_V_SAMPLER_BITS, sampler_variant_valid>(v, f, otherwise);
}
