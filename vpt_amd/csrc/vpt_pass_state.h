// vpt_pass_state.h — what a renderer remembers between two passes about its tile classes, as plain host C++ (nothing of HIP is
// included: tests/test_pass_state.py compiles it with the host compiler alone and walks it).  Three types; their fields are private and
// every change of them is one of the named members below:
//   Destinations   a small set of render destinations
//   MarcherTrack   the accumulating ray marchers (MIP, EAM, ISO, MCS, Depth): which fused passes may launch the HIT tiles only
//   MissState      MCM: what the MISS tiles' passes owe their state arrays, and when their settled forms may run
// Device memory and HIP handles (the lists, their staging, miss_words) stay in TileClasses (vpt_internal.h).
#pragma once
#include <string.h>
#include "../../include/vpt.h"

// render destinations (the renderer's own buffer, a caller's target, the slots of a bucket or of the gather ring): a full set ignores
// what is added; a removal moves the last entry into the gap
#define VPT_COMPLETE_DESTS 40
class Destinations {
    const void *p_[VPT_COMPLETE_DESTS] = {}; int n_ = 0;
    int find(const void *p) const { for (int i = 0; i < n_; i++) if (p_[i] == p) return i; return -1; }
public:
    bool has(const void *p) const { return find(p) >= 0; }   int size() const { return n_; }   void clear() { n_ = 0; }
    void add(const void *p) { if (!has(p) && n_ < VPT_COMPLETE_DESTS) p_[n_++] = p; }
    void remove(const void *p) { const int i = find(p); if (i >= 0) p_[i] = p_[--n_]; }
    // every address in [lo, lo + bytes)
    void remove_range(const void *lo, size_t bytes) { for (int i = 0; i < n_;) if ((const char *)p_[i] >= (const char *)lo && (const char *)p_[i] < (const char *)lo + bytes) p_[i] = p_[--n_]; else i++; }
};

// The accumulating ray marchers (vpt_render.hip marcher_track has the reasoning).  Once one whole fused pass has run since the reset, and
// as long as every pass since the reset used ONE matrix, the tiles none of whose rays meet the cube hold final values: a fused pass into
// a destination that a WHOLE-image fused pass has written since the reset needs the HIT tiles only.
//   passes_, fused_passes_   generate / fused passes since the reset; mvp_: the matrix of the first of them
//   poisoned_       a pass since the reset used another matrix, or the environment was set (MCS: the fixed points of the ray-missing pixels
//                   move with it): nothing is skipped until the next reset
//   first_mix_one_  the first pass since the reset was a fused pass with mix == 1 (MCS, Depth: accumulator = frame exactly)
//   list_now_       the launch being enqueued covers the HIT tiles only
//   reset_seen_     a reset has run on the present buffers (zero-filled buffers are not a reset)
//   whole_          written by a whole-image fused pass since the reset: only there do the skipped tiles hold their final texels
class MarcherTrack {
    uint64_t passes_ = 0, fused_passes_ = 0; float mvp_[16] = {};
    bool poisoned_ = false, first_mix_one_ = false, list_now_ = false, reset_seen_ = false; Destinations whole_;
public:
    void reset() { passes_ = fused_passes_ = 0; poisoned_ = false; list_now_ = false; reset_seen_ = true; }
    void geometry_rebuilt() { passes_ = fused_passes_ = 0; reset_seen_ = false; whole_.clear(); }
    void environment_changed() { poisoned_ = true; }   bool list_now() const { return list_now_; }   void use_lists(bool on) { list_now_ = on; }
    bool has_destination(const void *p) const { return whole_.has(p); }   void forget_destinations(const void *lo, size_t bytes) { whole_.remove_range(lo, bytes); }
    // a generate (fused = false) or fused pass with matrix `mvp` into `dest` is about to be enqueued; true: it may launch the HIT tiles of
    // `mvp` only — the caller builds the lists and says use_lists(true) if they are there.  capturing: a graph would freeze the grid
    bool pass(int kind, const float *mvp, bool fused, float first_mix, bool enabled, bool capturing, bool env_opaque, const void *dest) {
        list_now_ = false;
        if (kind != VPT_RENDERER_MIP && kind != VPT_RENDERER_EAM && kind != VPT_RENDERER_ISO && kind != VPT_RENDERER_MCS && kind != VPT_RENDERER_DEPTH) return false;
        if (passes_ == 0) { whole_.clear(); memcpy(mvp_, mvp, sizeof(mvp_)); poisoned_ = false; first_mix_one_ = fused && first_mix == 1.0f; }
        else if (memcmp(mvp_, mvp, sizeof(mvp_)) != 0) poisoned_ = true;
        passes_++;
        // (MCS: the alpha channel's first step is fl(fl(e - 1) + 1) from the reset's 1, which is e itself only for e = 1: opaque environments)
        const bool fixed_point = kind == VPT_RENDERER_DEPTH ? first_mix_one_ : (kind == VPT_RENDERER_MCS ? (first_mix_one_ && env_opaque) : true);
        const bool lists = fused && enabled && !poisoned_ && !capturing && fused_passes_ >= 1 && fixed_point && reset_seen_ && whole_.has(dest);
        // a whole-image pass under the reset's matrix makes its destination whole (`lists`: dest is in the set already)
        if (fused) { fused_passes_++; if (!poisoned_) whole_.add(dest); }
        return lists;
    }
    // a frame of a cached graph's replay: a whole-image fused pass that did not come through pass()
    void replayed(int kind, const float *mvp, float mix, const void *dest) { (void)pass(kind, mvp, true, mix, false, true, false, dest); }
};

// MCM's MISS tiles (vpt_kernels.h "Tile classes", vpt_mcm.hip "settled").  While every pass uses the reset's matrix a MISS tile's photons
// never enter the cube and its passes run k_mcm_miss on 32 B of state, leaving the position / transmittance arrays behind (stale); once
// the MISS pixels' radiance is proven final (settle == 1) the settled forms run, which also leave samples uncounted (pending) and, the
// packed form, the direction array behind its jitter-word records (words_fresh).  pending > 0 or words_fresh imply stale, and while
// either holds (owes) nothing but the settled forms may run before k_mcm_materialize has: plan() says so, materialized() ends it.
enum MissForm { MISS_PLAIN = 0, MISS_PACKED = 1, MISS_SETTLED = 2 };   // k_mcm_miss, k_mcm_miss_packed, k_mcm_miss_settled (vpt_mcm.hip miss_kernel)
// a pass over the tile classes, as launch_mcm_classes sees it.  plain_kernel: the volume's format runs the plain MISS kernel (the others
// have no settled form); capturing: into a graph; env_usable: a finite 1 x 1 environment; table: a tone-map table rides on the fused store
struct MissPass { bool fuse; uint32_t steps; bool plain_kernel; int n_miss; bool capturing, env_usable, table; const void *dest; };
// probe_first: read a MISS pixel back, report it (probed) and plan again with probed = true — nothing else is set.  materialize_first:
// SETTLED reads the direction array, which the records are ahead of.  catch_up_first: PLAIN counts on from the samples array and reads it too
struct MissPlan { bool probe_first; MissForm form; bool materialize_first, catch_up_first; };
//   option_         VPT_OPTION_SETTLED_MISS: 0 off, 1 k_mcm_miss_settled, 2 k_mcm_miss_packed
//   stale_, stale_fast_   the position / transmittance arrays are behind; the pass that left them ran the fast variant
//   words_fresh_    the last pass was a packed one: the records are newer than the direction array
//   pending_        events the settled forms have run that the samples array does not show yet
//   events_         events of every pixel since the reset (= `samples` of a MISS pixel, pending included)
//   env_changed_    the environment was set since the reset: the MISS pixels' mean is on the move again until the next one
//   settle_, probes_   0: not known whether the MISS pixels' radiance is final, 1: proven, 2: given up until the next reset; read-backs spent on it
//   shown_          destinations all of whose MISS texels show the settled radiance; shown_events_: events_ behind the pass that last
//                   rebuilt it while settle_ == 0
//   settled_passes_ passes whose MISS tiles ran a settled form (vpt_renderer_settled_passes)
class MissState {
    int option_ = 2, settle_ = 0, probes_ = 0;
    bool stale_ = false, stale_fast_ = false, words_fresh_ = false, env_changed_ = false;
    uint32_t pending_ = 0; uint64_t events_ = 0, shown_events_ = 0, settled_passes_ = 0; Destinations shown_;
public:
    bool stale() const { return stale_; }                        bool stale_fast() const { return stale_fast_; }
    uint32_t pending() const { return pending_; }                bool words_fresh() const { return words_fresh_; }
    bool owes() const { return pending_ || words_fresh_; }       uint64_t events() const { return events_; }
    uint64_t settled_passes() const { return settled_passes_; }  bool has_destination(const void *p) const { return shown_.has(p); }
    void forget_destinations(const void *lo, size_t bytes) { shown_.remove_range(lo, bytes); }
    // a reset rewrote every array; settles_at_once: the first deposit already leaves the environment's colour (settle_from_reset)
    void reset(bool settles_at_once) { stale_ = words_fresh_ = env_changed_ = false; events_ = shown_events_ = 0; pending_ = 0; shown_.clear(); probes_ = 0; settle_ = settles_at_once ? 1 : 0; }
    void materialized() { stale_ = false; pending_ = 0; words_fresh_ = false; }   void geometry_rebuilt() { materialized(); shown_.clear(); }   // (new, zeroed arrays)
    void environment_changed() { env_changed_ = true; }          void set_option(int value) { option_ = value; }
    bool option_wants_catch_up(int value) const { return !value || (value != 2 && words_fresh_); }   // (1: k_mcm_miss_settled reads the direction array)
    // The settled form: the radiance of the MISS pixels is proven final, their samples stay countable in a float (2^24), and (a fused pass)
    // the destination already shows every MISS texel and no display table rides on the store; packed with VPT_OPTION_SETTLED_MISS = 2.
    MissPlan plan(const MissPass &p, bool probed = false) {
        const bool wanted = option_ && p.plain_kernel && p.n_miss > 0 && !env_changed_ && !p.capturing && p.env_usable && p.steps >= 1u && events_ >= 1 && events_ + p.steps < (1ull << 24);
        if (wanted && settle_ == 0 && pending_ == 0 && !probed) return MissPlan{ true, MISS_PLAIN, false, false };
        if (wanted && settle_ == 1 && (!p.fuse || (!p.table && shown_.has(p.dest))))
            return option_ == 2 ? MissPlan{ false, MISS_PACKED, false, false } : MissPlan{ false, MISS_SETTLED, words_fresh_, false };
        const bool shows = p.fuse && p.n_miss > 0 && p.steps >= 1u && settle_ != 2;   // this pass leaves every MISS texel of its destination behind
        if (shows && settle_ == 0) { shown_.clear(); shown_events_ = events_ + p.steps; }   // (a later proof covers the last pass's texels only)
        if (shows) shown_.add(p.dest);
        return MissPlan{ false, MISS_PLAIN, false, owes() };
    }
    // the outcome of the read-back plan() asked for: a pixel was there to read, its samples were events(), every channel has stopped moving
    void probed(bool found_pixel, bool counted, bool final) {
        probes_++;
        if (found_pixel && counted && final) { settle_ = 1; if (shown_events_ != events_) shown_.clear(); }   // (destinations written before the last pass show an earlier mean)
        else if (!found_pixel || probes_ >= 4) settle_ = 2;
    }
    void bucket_done(bool fast, int n_miss) { stale_ = n_miss > 0; stale_fast_ = fast; }   void events_run(uint64_t n) { events_ += n; }   // (every form of pass: vpt_mcm.hip mcm_events_run)
    void class_pass_done(MissForm form, uint32_t steps, bool fast, int n_miss) { bucket_done(fast, n_miss); words_fresh_ = form == MISS_PACKED; if (form != MISS_PLAIN) { pending_ += steps; settled_passes_++; } }
};
