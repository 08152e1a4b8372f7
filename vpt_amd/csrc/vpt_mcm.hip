// vpt_mcm.hip — the MCM renderer's passes (vpt_kernels_mcm.h) behind vpt_render.hip's entry points: the tile classes (HIT | MISS kernels
// on two streams), the bucket kernels, reset / render / materialise.  The integrate kernels themselves are compiled in vpt_mcm_hit.hip, the
// frame sequences in one launch in vpt_mcm_seq.hip (three translation units: the build is parallel).  MCMRenderer.js:85-199.
#include "vpt_mcm_select.h"
#define VPT_MCM_PLAIN_KERNELS
#include "vpt_kernels_mcm.h"

// ---- MCM passes over the tile classes ---------------------------------------------------------------------------------
#ifdef VPT_EVENT_TIMING
#define VPT_TIMING_ARG(part, hit) do { if (hit) (part).violations = timing; else if (!check) (part).violations = timing_miss; } while (0)
#else
#define VPT_TIMING_ARG(part, hit) do { } while (0)
#endif
#ifdef VPT_EVENT_TIMING
// (VPT_EVENT_TIMING builds only) [0]: the HIT-tile kernel's wave slots, [1]: the MISS-tile kernels'; kept for the life of the process,
// hence bare pointers: never freed
static unsigned long long *g_timing[2] = { nullptr, nullptr };
static const size_t g_timing_waves[2] = { VPT_TIMING_WAVES, VPT_TIMING_MISS_WAVES };
static unsigned long long *timing_buffer(vpt_renderer *r, int which) {
    if (!g_timing[which]) {
        const size_t bytes = g_timing_waves[which] * 16 * sizeof(unsigned long long);
        if (hipMalloc(&g_timing[which], bytes) != hipSuccess) { g_timing[which] = nullptr; return nullptr; }
        hipMemsetAsync(g_timing[which], 0, bytes, r->ctx->stream);
        hipStreamSynchronize(r->ctx->stream);                  // (the MISS-tile kernel runs on a side stream)
    }
    return g_timing[which];
}
#endif
static bool mcm_classes_usable(const vpt_renderer *r, const PassArgs &a) {
    return r->cls.enabled && r->cls.valid && a.blur == 0.0f && memcmp(r->cls.mvp, a.mvp_inv.m, sizeof(r->cls.mvp)) == 0;
}
// the kernel side of it: the volume's boundary atlas (what k_mcm_miss samples; every format since round 4), no persistent-wave option
// (SNORM byte volumes: the general pass — no MISS-tile kernel form of their own; 16-bit volumes borrow the FLOAT one, launch_mcm_classes)
static bool mcm_classes_runnable(const vpt_renderer *r, const PassArgs &a) {
    return a.vol.atlas != nullptr && !r->mcm_persistent && !(r->vol->snorm && !r->vol->norm16);
}
// ... and of the bucket kernels (and of the HIT-tile kernel's early form): LINEAR one-channel byte volumes
static bool mcm_plain_volume(const vpt_renderer *r) { return (variant_of(r) & ~VPT_V_WIDE) == 0 && unsigned_r8(r->vol); }
// NEAREST / two-channel / float volumes: the MISS tiles through the one-phase sampler of k_mcm_miss (miss_sample_any); v: those three bits
template <bool FUSE> static PassKernel format_miss_kernel(int v, bool fast) {
    return dispatch_variant<VPT_V_NEAREST | VPT_V_RG | VPT_V_F32>(
        v, [&](auto F) { return fast ? (PassKernel)k_mcm_miss<FUSE, F() | VPT_V_FAST, false, true> : (PassKernel)k_mcm_miss<FUSE, F(), false, true>; }, no_pass_kernel);
}
// LINEAR one-channel byte volumes: the MISS-tile kernel of a form — the one list of what is instantiated.  Bit-exact arithmetic exists
// with LATE = true only (launch_mcm_classes: `late`); the settled forms have no FUSE parameter
template <bool FUSE> static PassKernel miss_kernel(int vf, MissForm form, bool fast, bool late, bool check) {
    if (vf) return format_miss_kernel<FUSE>(vf, fast);
    constexpr int Q = VPT_V_FAST; static_assert(MISS_PLAIN == 0 && MISS_PACKED == 1 && MISS_SETTLED == 2, "the rows' order");
    static const PassKernel kernels[3][6] = {                  // <arithmetic, CHECK, LATE>
        { k_mcm_miss<FUSE, Q, true, true>, k_mcm_miss<FUSE, Q, true, false>, k_mcm_miss<FUSE, 0, true, true>, k_mcm_miss<FUSE, Q, false, true>, k_mcm_miss<FUSE, Q, false, false>, k_mcm_miss<FUSE, 0, false, true> },
        { k_mcm_miss_packed<Q, true, true>, k_mcm_miss_packed<Q, true, false>, k_mcm_miss_packed<0, true, true>, k_mcm_miss_packed<Q, false, true>, k_mcm_miss_packed<Q, false, false>, k_mcm_miss_packed<0, false, true> },
        { k_mcm_miss_settled<Q, true, true>, k_mcm_miss_settled<Q, true, false>, k_mcm_miss_settled<0, true, true>, k_mcm_miss_settled<Q, false, true>, k_mcm_miss_settled<Q, false, false>, k_mcm_miss_settled<0, false, true> } };
    return kernels[form][(check ? 0 : 3) + (fast ? (late ? 0 : 1) : 2)];
}
// position / transmittance of the MISS tiles, as the last pass's arithmetic would have stored them
int mcm_materialize(vpt_renderer *r) {
    MissState &m = r->cls.miss;
    if (!m.stale()) return VPT_OK;
    VPT_TRY(join_side(r));
    HIP_TRY(hipSetDevice(r->ctx->device));
    PassArgs a;
    VPT_TRY(make_args(r, nullptr, false, &a));
    memcpy(a.mvp_inv.m, r->cls.mvp, sizeof(r->cls.mvp));
    mat4_sums(&a);
    a.pm.tile_list = r->cls.list + r->cls.n_hit; a.pm.list_n = r->cls.n_miss;
    if (r->cls.n_miss > 0) {
        const uint32_t words = m.words_fresh() ? 1u : 0u;      // the direction array first, from k_mcm_miss_packed's records
        if (m.stale_fast()) hipLaunchKernelGGL(k_mcm_materialize<true>, dim3((unsigned)r->cls.n_miss), dim3(VPT_BLOCK), 0, r->ctx->stream, a, m.pending(), words);
        else hipLaunchKernelGGL(k_mcm_materialize<false>, dim3((unsigned)r->cls.n_miss), dim3(VPT_BLOCK), 0, r->ctx->stream, a, m.pending(), words);
        HIP_TRY(hipGetLastError());
    }
    m.materialized();
    return VPT_OK;
}
int mcm_catch_up(vpt_renderer *r) { return r->cls.miss.owes() ? mcm_materialize(r) : VPT_OK; }
// (the MISS pixels' running mean moves again: the settled forms wait for a reset)
int mcm_environment_changed(vpt_renderer *r) { VPT_TRY(mcm_catch_up(r)); r->cls.miss.environment_changed(); return VPT_OK; }
// every form of pass runs its events of every pixel and says so here: the general, class and persistent passes (launch_mcm_pass), a
// bucket, a sequence in one launch (mcm_multi) and the replay of a cached graph (vpt_render.hip)
void mcm_events_run(vpt_renderer *r, uint64_t events) { r->cls.miss.events_run(events); }

// ---- the settled form of the MISS-tile pass (k_mcm_miss_settled) ---------------------------------------------------------------------
// Every event of a MISS pixel deposits the constant e of a 1x1 environment into the running mean r <- r + (e - r) / n, from r = 1 at the
// reset (k_mcm_reset).  The first deposit (n = 1, and 1 / 1 = 1 in both arithmetic variants) leaves fl(1 + fl(e - 1)): e itself for white,
// black and every e with 1 + (e - 1) == e — then e - r = 0 for good (settle_from_reset).  Any other e is approached to within a few units in
// the last place and the mean stops where the step |e - r| / n falls below half the spacing of the floats around r; all MISS pixels hold
// the same (r, n), so one of them read back between two passes decides it (settle_probe) for both variants: the bound below allows for a
// reciprocal that is off by an ulp and for a fused or an unfused multiply-add, and the step only shrinks as n grows.
static bool settle_env_usable(const vpt_renderer *r) {
    return r->env_w == 1 && r->env_h == 1 && std::isfinite(r->env_const.x) && std::isfinite(r->env_const.y) && std::isfinite(r->env_const.z);
}
static bool settle_from_reset(const vpt_renderer *r) {
    if (!settle_env_usable(r)) return false;
    const float e[3] = { r->env_const.x, r->env_const.y, r->env_const.z };
    for (int i = 0; i < 3; i++) {
        volatile float d = e[i] - 1.0f, r1 = 1.0f + d;
        if (!(r1 == e[i])) return false;
    }
    return true;
}
static bool settle_channel_final(float e, float rad, uint64_t n) {
    if (!std::isfinite(rad)) return false;
    if (e == rad) return true;
    if (!std::isnormal(rad)) return false;
    const double gap = std::min((double)std::nextafter(rad, INFINITY) - (double)rad, (double)rad - (double)std::nextafter(rad, -INFINITY));
    return std::fabs((double)e - (double)rad) * 1.001 / (double)(n + 1) < 0.49 * gap;
}
// reads [radiance, samples] of one MISS pixel back (a host wait: at most a few per reset, and only for an environment colour that
// settle_from_reset cannot decide)
static int settle_probe(vpt_renderer *r) {
    TileClasses &c = r->cls;
    const uint32_t *list = c.staging[c.stage_next ^ 1];          // the host copy of the lists on the device (classes_build)
    long long k = -1;
    for (int i = 0; list && i < c.n_miss && k < 0; i++) {
        const int tx = (int)(list[c.n_hit + i] & 0xffffu), ty = (int)(list[c.n_hit + i] >> 16), l = ty * VPT_TILE;
        const int lb = l / r->R, j = r->G == 1 ? l : (lb * r->G + r->g) * r->R + (l - lb * r->R);
        if (tx < r->tiles_x && l < r->local_h && j < r->H) k = ((long long)ty * r->tiles_x + tx) * VPT_BLOCK;   // the tile's first pixel (map_pixel)
    }
    if (k >= 0) {
        VPT_TRY(join_side(r));
        float4 v;
        HIP_TRY(hipMemcpyAsync(&v, r->st[3].get() + k, sizeof(v), hipMemcpyDeviceToHost, r->ctx->stream));
        HIP_TRY(hipStreamSynchronize(r->ctx->stream));
        const uint64_t n = c.miss.events();
        c.miss.probed(true, v.w >= 0.0f && (uint64_t)(v.w + 0.5f) == n,
                      settle_channel_final(r->env_const.x, v.x, n) && settle_channel_final(r->env_const.y, v.y, n) && settle_channel_final(r->env_const.z, v.z, n));
    } else c.miss.probed(false, false, false);
    return VPT_OK;
}
// an MCM reset with matrix u->mvp_inverse has just been enqueued
static int mcm_classify(vpt_renderer *r, const vpt_uniforms *u) {
    r->cls.valid = false; r->cls.miss.reset(settle_from_reset(r));   // the reset rewrote every array
    if (!r->cls.enabled || u->blur != 0.0f) return VPT_OK;
    return classes_build(r, u->mvp_inverse);
}

// profiling (inside a Timed pair only): starts on `s` the pair vpt_renderer_profile_side reads, around the first launch a pass puts
// on a side stream; returns the event to record on `s` behind that launch, or null
static hipEvent_t side_events_begin(vpt_renderer *r, hipStream_t s) {
    const EventPairs::Pair *pair = r->timed_now ? r->side_timing.take(1) : nullptr;
    if (!pair) return nullptr;
    hipEventRecord(pair->t0, s);
    return pair->t1;
}
// one MCM pass (integrate, or render() = integrate + renderFrame) as list launches: the HIT tiles through k_mcm_integrate on the
// context's stream, the MISS tiles through k_mcm_miss — with VPT_OPTION_SPLIT_STREAMS = K as K - 1 equal parts on the side streams,
// so that the latency-bound HIT tiles and the arithmetic-bound MISS tiles share the chip for the whole frame
template <bool FUSE>
static int launch_mcm_classes(vpt_renderer *r, const PassArgs &a) {
    const bool fast = r->fast_math != 0, check = r->cls.verify;
    PassKernel kh, km;
    // the HIT tiles: few enough to be resident at once at 5 waves per SIMD (a shard's share) -> the form with the early path end,
    // whose pass is one wave per SIMD walking a chain of dependent latencies; else the 7-waves form (VPT_HIT_KERNEL_FORM in the environment overrides)
    const bool plain = mcm_plain_volume(r);
    const bool early = plain && (r->hit_form == 2 || (r->hit_form == 0 && r->cls.n_hit <= 1280));
    // (another volume format: the HIT tiles through the general kernel of the volume's variant, from a tile list)
    if (plain) kh = mcm_hit_kernel(FUSE, class_variant(r, a), early);
    else kh = mcm_general_kernel(FUSE, variant_of(r), fast);
    // the MISS tiles: the sample consumed after the path end (its gather flies under that arithmetic) — whole frame 80.8 -> 79.3-79.7 us
    // fast-math, 96.1 -> 92.8 bit-exact, rank 3 of 8's share 18.4 -> 17.1 bit-exact but 15.8 -> 16.9 fast-math: there the sample is
    // consumed where the shader takes it
    const bool late = !(fast && early);
    // a quasi-cubic volume reuses the LINEAR MISS-tile kernel of its format: a MISS tile's sample is executed and discarded (mcm_events_miss),
    // so the filter cannot change what that kernel writes (tests/test_gpu_quasicubic.py: classes against the general pass, bit for bit)
    // A 16-bit volume's MISS tiles run the MISS-tile kernel of the FLOAT format of the same channels and filter (no k_mcm_miss of their own).
    // That kernel reads the volume through the boundary atlas alone (miss_sample_any -> sample_boundary_rg: no brick tables, no bricks),
    // and a 16-bit volume's atlas IS the float atlas of its decoded texels (float4 cells, v->atlas_dwords sized for them, vpt_volume_create):
    // every gather stays inside that allocation and reads what the R32F twin's would (tests/test_gpu_norm16.py: 1080p classes, atlas on / off).
    int vm = variant_of(r) & ~VPT_V_QCUBIC;
    if (vm & VPT_V_NORM16) vm = (vm & ~(VPT_V_NORM16 | VPT_V_SNORM)) | VPT_V_F32;
    const int vf = vm & ~VPT_V_WIDE;                           // a format with a MISS-tile kernel of its own: no settled forms
    if (!kh) return fail(VPT_ERR_INVALID, "no MCM tile-class kernels for variant %d", variant_of(r));
    // the form of the MISS part (MissState::plan) and what has to run in front of it
    TileClasses &c = r->cls;
    const MissPass pass = { FUSE, a.steps, !vf, c.n_miss, r->no_split, settle_env_usable(r), a.tm_table != nullptr, (const void *)a.render };
    MissPlan plan = c.miss.plan(pass);
    if (plan.probe_first) { VPT_TRY(settle_probe(r)); plan = c.miss.plan(pass, true); }
    if (plan.materialize_first || plan.catch_up_first) VPT_TRY(mcm_materialize(r));
    // (the packed form's records: every one is written by a pass before one reads it, miss_load_dir)
    if (plan.form == MISS_PACKED && !c.miss_words) HIP_TRY(c.miss_words.alloc(r->npix_padded));
    km = miss_kernel<FUSE>(vf, plan.form, fast, late, check);
    if (!km) return fail(VPT_ERR_INVALID, "no MCM tile-class kernels for variant %d", variant_of(r));   // (no vf is without one: never)
    const size_t lds_hit = lds_bytes(r), lds_miss = (size_t)r->tf_w * 2 * sizeof(float4);
    VPT_TRY(lds_prepare((const void *)kh, lds_hit));
    const int k = split_allowed(r) ? r->split : 1;
    struct Part { PassKernel kernel; const uint32_t *list; int n; size_t lds; };
    Part parts[VPT_MAX_SPLIT]; int np = 0;
    // (measured, 1080p headline frame, us per frame: HIT | MISS on two streams 81.0; HIT | MISS/2 | MISS/2 82.3-83.0; HIT/2 | HIT/2 | MISS
    // 82.7-84.1; four streams 93; one stream, HIT then MISS: 102.  Capping the HIT kernel's residency (dynamic LDS) to 2 / 3 / 4 / 5
    // workgroups per CU so that MISS waves always sit beside its waves: 99 / 91 / 83.4 / 82.2 against 81.6 uncapped — DESIGN.md section 5)
#ifdef VPT_EVENT_TIMING
    unsigned long long *const timing = timing_buffer(r, 0), *const timing_miss = timing_buffer(r, 1);
#endif
    // (a frame the volume fills — no MISS tile at all — was tried with the HIT list in k parts on the k streams: 143.9 -> 143.7 us, nothing)
    const int hit_parts = r->cls.n_hit > 0 ? 1 : 0;
    const int miss_parts = std::max(1, k - hit_parts);
    for (int i = 0; i < hit_parts; i++) {
        const int h0 = (int)((long long)r->cls.n_hit * i / hit_parts), h1 = (int)((long long)r->cls.n_hit * (i + 1) / hit_parts);
        if (h1 > h0) parts[np++] = Part{ kh, r->cls.list + h0, h1 - h0, lds_hit };
    }
    for (int i = 0; i < miss_parts; i++) {
        const int m0 = (int)((long long)r->cls.n_miss * i / miss_parts), m1 = (int)((long long)r->cls.n_miss * (i + 1) / miss_parts);
        if (m1 > m0) parts[np++] = Part{ km, r->cls.list + r->cls.n_hit + m0, m1 - m0, lds_miss };
    }
    VPT_TRY(streams_deal(r, Deal{ DEAL_LISTS, k == 1 ? 1 : std::max(np, 1) }));
    auto part_args = [&](int i) {
        PassArgs part = a;
        part.pm.tile_list = parts[i].list; part.pm.list_n = parts[i].n; part.miss_load_pos = c.miss.stale() ? 0u : 1u; part.violations = r->cls.violations;
        part.miss_verify = check ? 1u : 0u;
        part.miss_words = c.miss_words; part.miss_load_dir = c.miss.words_fresh() ? 0u : 1u;
        VPT_TIMING_ARG(part, i < hit_parts);
        return part;
    };
    if (k == 1) {
        // one stream: the launches follow each other; the dispatch's completion event (gather pipeline) rides on the last
        for (int i = 0; i < np; i++) {
            const PassArgs part = part_args(i);
            // profiling: the caller's pair (Timed) brackets both launches; the MISS-tile kernel gets the pair vpt_renderer_profile_side reads
            const hipEvent_t e1 = i >= hit_parts && i == np - 1 ? side_events_begin(r, r->ctx->stream) : nullptr;
            if (i + 1 == np) launch_range(parts[i].kernel, r, dim3((unsigned)parts[i].n), dim3(VPT_BLOCK), parts[i].lds, r->ctx->stream, part, 0);
            else hipLaunchKernelGGL(parts[i].kernel, dim3((unsigned)parts[i].n), dim3(VPT_BLOCK), parts[i].lds, r->ctx->stream, part);
            if (e1) hipEventRecord(e1, r->ctx->stream);
        }
    } else {
        // (the MISS-tile kernel is the longer of the two and goes first: its stream is the one a short sequence of frames waits for at the
        // end — blocks of 5 frames 87.5 -> 85.3 us per frame, of 20 frames 81.9 -> 81.1, long sequences the same)
        for (int i = np - 1; i >= 0; i--) {
            const PassArgs part = part_args(i);
            // profiling: the context's stream is bracketed by the caller (Timed); the first side launch gets a pair of its own
            const hipEvent_t e1 = i == 1 ? side_events_begin(r, range_stream(r, 1)) : nullptr;
            launch_range(parts[i].kernel, r, dim3((unsigned)parts[i].n), dim3(VPT_BLOCK), parts[i].lds, range_stream(r, i), part, i);
            if (e1) hipEventRecord(e1, range_stream(r, 1));
        }
    }
    c.miss.class_pass_done(plan.form, a.steps, fast, c.n_miss);
    return VPT_OK;
}

// VPT_OPTION_BUCKET_KERNEL: frames [0, count) of a bucket (frame f -> ring + f * slot_pixels texels) by one launch per tile class —
// k_mcm_bucket_hit on the context's stream, k_mcm_bucket_miss on the first side stream.  *ready = false: the preconditions of the tile
// classes do not hold (launch_mcm_pass) and the caller plays the frames one by one.
typedef void (*BucketKernel)(PassArgs, FrameSeeds, uint32_t, void *, uint32_t);
int mcm_bucket_ready(vpt_renderer *r, const PassArgs &a, bool *ready) {
    bool same = false;
    VPT_TRY(mcm_before_pass(r, a, &same));
    const bool two_streams = split_allowed(r);
    if (two_streams) VPT_TRY(ensure_split_streams(r));
    *ready = same && r->cls.enabled && mcm_classes_runnable(r, a) && mcm_plain_volume(r) && two_streams && !r->cls.verify;
    return VPT_OK;
}
template <bool DISPLAY> static BucketKernel bucket_hit_kernel(int v, bool early) {
    return dispatch_variant<VPT_V_CLASS_BITS>(
        v, [&](auto V) { return early ? (BucketKernel)k_mcm_bucket_hit<V(), true, DISPLAY> : (BucketKernel)k_mcm_bucket_hit<V(), false, DISPLAY>; },
        [] { return (BucketKernel)nullptr; });
}
template <bool DISPLAY>
static void bucket_kernels(int v, bool early, BucketKernel *kh, BucketKernel *km) {
    const bool fast = (v & VPT_V_FAST) != 0;
    *kh = bucket_hit_kernel<DISPLAY>(v, early);
    const bool late = !(fast && early);
    *km = fast ? (late ? (BucketKernel)k_mcm_bucket_miss<VPT_V_FAST, true, DISPLAY> : (BucketKernel)k_mcm_bucket_miss<VPT_V_FAST, false, DISPLAY>)
               : (BucketKernel)k_mcm_bucket_miss<0, true, DISPLAY>;
}
// display_table: null = RGBA16F slots; else the armed tone mapper's table — RGBA8 slots (slot_pixels counts texels either way)
int mcm_bucket(vpt_renderer *r, const PassArgs &a, const FrameVar *v, int count, void *ring, uint32_t slot_pixels, bool last_to_render_buffer,
               const uint8_t *display_table) {
    if (count < 1 || count > VPT_BUCKET_FRAMES) return fail(VPT_ERR_INVALID, "a bucket launch holds 1..%d frames", VPT_BUCKET_FRAMES);
    VPT_TRY(mcm_catch_up(r));                                  // k_mcm_bucket_miss counts on from the samples array
    const bool fast = r->fast_math != 0;
    // HIT tiles few enough to be resident at once at the kernel's four waves per SIMD: the form with the early path end (launch_mcm_classes)
    const bool early = r->hit_form == 2 || (r->hit_form == 0 && r->cls.n_hit <= 1024);
    BucketKernel kh, km;
    if (display_table) bucket_kernels<true>(class_variant(r, a), early, &kh, &km);
    else bucket_kernels<false>(class_variant(r, a), early, &kh, &km);
    if (!kh || !km) return fail(VPT_ERR_INVALID, "no MCM tile-class kernels for variant %d", variant_of(r));
    const size_t lds_hit = lds_bytes(r), lds_miss = (size_t)r->tf_w * 2 * sizeof(float4);
    VPT_TRY(lds_prepare((const void *)kh, lds_hit));
    VPT_TRY(streams_deal(r, Deal{ DEAL_LISTS, 2 }));
    FrameSeeds fs;
    for (int f = 0; f < VPT_BUCKET_FRAMES; f++) fs.seed[f] = f < count ? v[f].seed : 0.0f;
    PassArgs part = a;
    part.miss_load_pos = r->cls.miss.stale() ? 0u : 1u; part.violations = r->cls.violations; part.tm_table = display_table;
    if (!last_to_render_buffer) part.render = nullptr;
    if (r->cls.n_hit > 0) {
        part.pm.tile_list = r->cls.list; part.pm.list_n = r->cls.n_hit;
        hipLaunchKernelGGL(kh, dim3((unsigned)r->cls.n_hit), dim3(VPT_BLOCK), lds_hit, r->ctx->stream, part, fs, (uint32_t)count, ring, slot_pixels);
    }
    if (r->cls.n_miss > 0) {
        part.pm.tile_list = r->cls.list + r->cls.n_hit; part.pm.list_n = r->cls.n_miss;
        hipLaunchKernelGGL(km, dim3((unsigned)r->cls.n_miss), dim3(VPT_BLOCK), lds_miss, range_stream(r, 1), part, fs, (uint32_t)count, ring, slot_pixels);
    }
    r->cls.miss.bucket_done(fast, r->cls.n_miss);
    r->tm_valid = false;
    r->bucket_launches++;
    mcm_events_run(r, (uint64_t)a.steps * (uint64_t)count);
    return VPT_OK;
}

// persistent MCM: as many workgroups as are resident at once (occupancy query x CUs), never more than there are segments
template <typename K>
static int launch_mcm_persist(K kernel, vpt_renderer *r, const PassArgs &a) {
    const size_t lds = lds_bytes(r);
    VPT_TRY(lds_prepare((const void *)kernel, lds));
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, VPT_BLOCK, lds));
    if (per_cu < 1) per_cu = 1;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, r->ctx->device));
    int nseg = r->tiles_x * ((r->local_h + VPT_TILE - 1) / VPT_TILE) * 4;
    int blocks = per_cu * prop.multiProcessorCount;
    if (blocks > (nseg + 3) / 4) blocks = (nseg + 3) / 4;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(VPT_BLOCK), lds, r->ctx->stream, a, nseg);
    return VPT_OK;
}
#define LAUNCH_MCM_PERSIST(FUSE, r, a) do { \
    int v_ = ((r)->vol->wide ? VPT_V_WIDE : 0) | ((r)->vol->filter == VPT_FILTER_NEAREST ? VPT_V_NEAREST : 0); \
    switch (v_) { \
        case 0: VPT_TRY((r)->mcm_persistent == 2 ? launch_mcm_persist((k_mcm_persist<FUSE, 0, true>), (r), (a)) : launch_mcm_persist((k_mcm_persist<FUSE, 0, false>), (r), (a))); break; \
        case 1: VPT_TRY(launch_mcm_persist((k_mcm_persist<FUSE, 1, false>), (r), (a))); break; \
        case 2: VPT_TRY((r)->mcm_persistent == 2 ? launch_mcm_persist((k_mcm_persist<FUSE, 2, true>), (r), (a)) : launch_mcm_persist((k_mcm_persist<FUSE, 2, false>), (r), (a))); break; \
        default: VPT_TRY(launch_mcm_persist((k_mcm_persist<FUSE, 3, false>), (r), (a))); break; \
    } } while (0)

// MCM passes with a matrix (or a blur) other than the reset's: the photons of MISS tiles may now enter the cube — the classes are
// void until the next reset.  Whole-image kernels need the MISS tiles' position / transmittance arrays up to date first.
int mcm_before_pass(vpt_renderer *r, const PassArgs &a, bool *same_matrix) {
    const bool same = r->cls.valid && a.blur == 0.0f && memcmp(r->cls.mvp, a.mvp_inv.m, sizeof(r->cls.mvp)) == 0;
    if (r->cls.valid && !same) { VPT_TRY(mcm_materialize(r)); r->cls.valid = false; }
    if (same_matrix) *same_matrix = same;
    return VPT_OK;
}
template <bool FUSE>
static int launch_mcm_pass(vpt_renderer *r, const PassArgs &a) {
    bool same = false;
    VPT_TRY(mcm_before_pass(r, a, &same));
    // The two kernels of the classes pay on two streams (1080p headline frame 81 us against 99-106 for the general kernel; rank 3 of 8's
    // share 17.7 against 19.4) and lose when they have to follow each other on ONE stream (102; the share: 30.5 against 20.7): a pass
    // that must stay on the context's stream — no VPT_OPTION_SPLIT_STREAMS, a caller-owned render target without
    // vpt_renderer_play_into*, a sequence being captured — runs the general kernel.
    const bool two_streams = split_allowed(r);
    if (two_streams) VPT_TRY(ensure_split_streams(r));
    int rc;
    if (same && r->cls.enabled && mcm_classes_runnable(r, a) && (two_streams || r->cls.one_stream)) rc = launch_mcm_classes<FUSE>(r, a);
    else {
        VPT_TRY(mcm_materialize(r));
        if (r->mcm_persistent && persistent_volume(r->vol)) { LAUNCH_MCM_PERSIST(FUSE, r, a); rc = VPT_OK; }
        else rc = mcm_general_pass(r, a, FUSE);
    }
    if (rc == VPT_OK) mcm_events_run(r, a.steps);             // every form runs `steps` events of every pixel (launch_mcm_classes looks at the count before its pass)
    return rc;
}

// ---- what vpt_render.hip calls ------------------------------------------------------------------------------------------
#define LAUNCH(kernel, r, a, lds) hipLaunchKernelGGL(kernel, tile_grid(r), dim3(VPT_BLOCK), (lds), (r)->ctx->stream, (a))
int mcm_reset(vpt_renderer *r, const PassArgs &a, const vpt_uniforms *u) {
    LAUNCH(k_mcm_reset, r, a, 0);
    HIP_TRY(hipGetLastError());
    return mcm_classify(r, u);
}
int mcm_pass(vpt_renderer *r, const PassArgs &a, bool fuse_render) {
    return fuse_render ? launch_mcm_pass<true>(r, a) : launch_mcm_pass<false>(r, a);
}
int mcm_render_frame(vpt_renderer *r, const PassArgs &a) {
    // _renderFrame behind an integrate pass of the tile classes that is still on its two streams (render() hook by hook, AbstractRenderer.js:60-70):
    // the HIT tiles' texels by the context's stream, the MISS tiles' by the side stream — each behind its own class kernel, no join, so the
    // next pass's kernels overlap this one's as they do behind the fused call (1080p: 124 -> 104 us per frame hook by hook; fused 92)
    if (r->streams.busy() && r->streams.last == Deal{ DEAL_LISTS, 2 } && r->cls.valid && r->cls.n_hit > 0 && r->cls.n_miss > 0 &&
        !r->target_is_callers && !r->stop_events) {          // (the lists are those of the launch still in flight: a reset joins before it rebuilds them)
        PassArgs part = a;
        part.pm.tile_list = r->cls.list; part.pm.list_n = r->cls.n_hit;
        hipLaunchKernelGGL(k_mcm_render, dim3((unsigned)r->cls.n_hit), dim3(VPT_BLOCK), 0, r->ctx->stream, part);
        part.pm.tile_list = r->cls.list + r->cls.n_hit; part.pm.list_n = r->cls.n_miss;
        hipLaunchKernelGGL(k_mcm_render, dim3((unsigned)r->cls.n_miss), dim3(VPT_BLOCK), 0, range_stream(r, 1), part);
        return VPT_OK;
    }
    VPT_TRY(join_side(r));
    LAUNCH(k_mcm_render, r, a, 0);
    return VPT_OK;
}
#ifdef VPT_EVENT_TIMING
// instrumented builds only (tools/r04_event_timing.py, tools/miss_wave_life.py bind them by name): a class kernel's phase clocks summed over
// its waves since the last call, in 10 ns ticks.  The HIT-tile kernel — [0..4] per event: free path | cell + tables | load flight | blend +
// transfer function | decision + path end; [5] prologue, [6] epilogue, [7] one calibration mark per event, [8] waves.  The MISS-tile
// kernels — [0] the pass's events, [5] prologue up to the first event, [6] epilogue, [8] waves.
static int probe_timing(vpt_renderer *r, int which, uint64_t *out9) {
    if (!r || !out9 || !g_timing[which]) return fail(VPT_ERR_INVALID, "no timing buffer (run a classified pass first)");
    VPT_TRY(join_side(r));
    HIP_TRY(hipSetDevice(r->ctx->device));
    const size_t waves = g_timing_waves[which];
    std::vector<unsigned long long> host(waves * 16);
    HIP_TRY(hipMemcpyAsync(host.data(), g_timing[which], host.size() * 8, hipMemcpyDeviceToHost, r->ctx->stream));
    HIP_TRY(hipMemsetAsync(g_timing[which], 0, host.size() * 8, r->ctx->stream));
    HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    for (int k = 0; k < 9; k++) out9[k] = 0;
    for (size_t w = 0; w < waves; w++) for (int k = 0; k < 9; k++) out9[k] += host[w * 16 + k];
    // the LAST launch's timeline: when its waves started and ended, relative to the first wave's start (10 ns ticks): out9[9 ..] =
    // { waves, start p50, start p90, start max, end p10, end p50, end p90, end max }
    std::vector<unsigned long long> st, en;
    unsigned long long t0 = ~0ull;
    for (size_t w = 0; w < waves; w++) if (host[w * 16 + 8]) { st.push_back(host[w * 16 + 9]); en.push_back(host[w * 16 + 10]); t0 = std::min(t0, host[w * 16 + 9]); }
    for (int k = 9; k < 17; k++) out9[k] = 0;
    if (!st.empty()) {
        std::sort(st.begin(), st.end()); std::sort(en.begin(), en.end());
        const size_t n = st.size();
        out9[9] = n; out9[10] = st[n / 2] - t0; out9[11] = st[n * 9 / 10] - t0; out9[12] = st[n - 1] - t0;
        out9[13] = en[n / 10] - t0; out9[14] = en[n / 2] - t0; out9[15] = en[n * 9 / 10] - t0; out9[16] = en[n - 1] - t0;
    }
    return VPT_OK;
}
extern "C" VPT_API int vpt_probe_event_timing(vpt_renderer *r, uint64_t *out9) { return probe_timing(r, 0, out9); }
extern "C" VPT_API int vpt_probe_miss_timing(vpt_renderer *r, uint64_t *out9) { return probe_timing(r, 1, out9); }
#endif
