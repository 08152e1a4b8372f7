// vpt_internal.h — what the translation units of libvpt_hip.so share: the objects behind the C-ABI handles (include/vpt.h), the
// error plumbing and the launch helpers.  Translation units (Makefile; built in parallel, linked into one library):
//   vpt_core.hip    context, volume (upload, re-layout), renderer life cycle, tile classification, options, read-back, probes
//   vpt_mcm.hip     the MCM passes (vpt_kernels_mcm.h): tile classes, bucket kernels, reset / render / materialise
//   vpt_mcm_hit.hip the MCM integrate kernels of every variant (k_mcm_integrate*), handed to vpt_mcm.hip by variant (vpt_mcm_select.h, vpt_variants.h)
//   vpt_mcm_seq.hip MCM frame sequences in one launch (k_mcm_multi, k_mcm_frames)
//   vpt_march.hip   MIP, EAM, MCS passes (vpt_kernels_march.h)
//   vpt_extra.hip   ISO, Depth, LAO, DOS passes (vpt_kernels_iso_depth.h)
//   vpt_render.hip  the renderer entry points: the four hooks, render(), frame sequences (vpt_renderer_play*)
//   vpt_post.hip    what follows a frame: tone mappers, the RCCL frame gather
//   vpt_volume_ops.hip  volume operations on the device: the gradient-magnitude channel, texel read-back, histograms
//   vpt_volume_window.hip  the value-range window (window / level) of a one-channel volume, its range and its code histogram
//   vpt_volume_pyramid.hip  the next coarser level of a volume (2 x 2 x 2 cells averaged) and its binomial smoothing
//   vpt_volume_rank.hip  the rank filters of a volume over the 3 x 3 x 3 box: median, erosion, dilation, opening and closing
//   vpt_volume_components.hip  the connected components of a value range: per-voxel ranks, the component list, keep and label volumes
//   vpt_volume_field.hip  what components and distances share (vpt_volume_field.h): a uint32 per voxel over a volume's texels, its read-back and emitters
//   vpt_volume_distance.hip  the exact squared Euclidean distance to a value range (or to its complement): per-voxel d2, within and channel volumes
//   vpt_volume_resample.hip  a volume resampled to any grid size: nearest texel, or linear interpolation / area average in integers
//   vpt_volume_combine.hip  two volumes of one grid combined texel by texel (mask, min, max, difference, blend, pair) or compared (exact counts and sums)
//   vpt_volume_measure.hip  what a labelling is asked next (vpt_volume_components.h): thirteen exact accumulators per component, the volume that keeps a set of ranks
//   vpt_volume_reconstruct.hip  grey-level morphological reconstruction of a marker under a mask and the geodesic operations made of it (fill holes, clear border, h-maxima / -minima, dome, regional maxima / minima)
//   vpt_volume_watershed.hip    the watershed of a relief by steepest descent on its lower completion: basins as a vpt_components handle (classify, plateau distance, links in and across tiles; the tail is the components')
//   vpt_volume_thickness.hip    local thickness, the largest inscribed ball: a vpt_distance handle (vpt_volume_distance.h) made of another one (tile maxima, the cover walk)
//   vpt_volume_skeleton.hip     curve skeleton and topological kernel by subfield thinning: burn passes as a voxel field (vpt_volume_skeleton.h; bit planes, border marking, eight sub-steps a pass under an exact tile cull, the census)
//   vpt_volume_surface.hip      the isosurface as a mesh by naive surface nets: a vpt_surface handle (inside plane, classify, prefix sums without a wait between workgroups, vertices and quads placed by offset + popcount)
//   vpt_volume_graph.hip        the graph of a voxel set (a skeleton): classes, branches and nodes as two labellings (vpt_volume_graph.h; bit plane, prefix-sum placed voxel list, links, prune and class emitters)
// vpt_variants.h (through vpt_device.h) holds the variant bits of the sampling kernels and the switch from a run-time variant to a template
// argument; launch_variant below is its use for a renderer's sampling pass.
// vpt_buffers.h holds DevBuf<T> / PinnedBuf<T>, the owners of device and pinned host memory: the objects below own their memory through such
// members and everything else in them has a default member initialiser, so `new` builds a valid object and `delete` frees all of it.
// vpt_handles.h holds their siblings for the other two resources: Event and Stream, the owners of a HIP event and of a HIP stream, and
// EventPairs, the pool of timing event pairs behind vpt_renderer_set_profiling.  The destroy functions leave everything idle and `delete`.
// vpt_pass_state.h holds what a renderer's passes remember about the tile classes between two calls (Destinations, MarcherTrack, MissState).
// Nothing device-side crosses a translation unit: a kernel is compiled by the unit that names it (the three MCM units share one header).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <hip/hip_ext.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/vpt.h"
#include "vpt_kernels.h"
#include "vpt_buffers.h"
#include "vpt_handles.h"
#include "vpt_pass_state.h"

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));     // vpt_core.hip; sets vpt_last_error()
char *vpt_error_buffer(void);                                                         // the calling thread's message (512 bytes)
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return fail(VPT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define VPT_TRY(expr) do { int r_ = (expr); if (r_ != VPT_OK) return r_; } while (0)

// ---------------------------------------------------------------------------------------------
// objects
// ---------------------------------------------------------------------------------------------
struct vpt_tonemapper;
struct vpt_context {
    int device = 0;
    hipStream_t stream = nullptr;                // the stream everything is enqueued on: `own`, or the caller's (vpt_context_create_on_stream)
    Stream own;
    std::vector<vpt_tonemapper *> tonemappers;   // live tone mappers: a destroyed renderer is unbound from them
    std::vector<struct vpt_renderer *> renderers; // live renderers: a destroyed volume is unbound from them
};

struct vpt_volume {
    vpt_context *ctx = nullptr;
    int nx = 0, ny = 0, nz = 0;
    int format = 0;            // the VPT_FORMAT_* the volume was created with
    int channels = 0;          // 1 = R8 / R32F, 2 = RG8 (interleaved)
    bool f32 = false;          // FLOAT texels (VPT_FORMAT_R32F): 4 bytes per voxel, 512-byte brick slots
    bool snorm = false;        // signed normalised texels (VPT_FORMAT_R8_SNORM / RG8_SNORM: stored like R8 / RG8; R16_SNORM / RG16_SNORM): VPT_V_SNORM
    bool norm16 = false;       // 16-bit normalised texels (VPT_FORMAT_R16 .. RG16_SNORM): 2 bytes per channel, 256-byte brick slots, VPT_V_NORM16
    int packed = 0;            // packed source format (VPT_FORMAT_RGB565 ..; 0: none): uploads are decoded into RG32F storage (f32, 2 channels)
    int packed_bytes = 0;      // bytes per packed source texel: 2 or 4
    int vox_bytes = 0;         // bytes per voxel of the linear storage: channels * (f32 ? 4 : norm16 ? 2 : 1)
    uint32_t slot_shift = 0, elem_shift = 0;   // log2 of a brick slot's bytes (two channels: both bricks) and of a stored channel's bytes (DevVolume)
    int filter = VPT_FILTER_LINEAR;            // Volume.js:53-54
    DevBuf<uint8_t> linear;    // nx*ny*nz*channels, the "texture storage" blocks are uploaded into
    DevBuf<uint8_t> bricks;    // apron bricks, Morton order
    size_t brick_bytes = 0;
    DevBuf<uint32_t> tab32;    // separable brick-offset tables TX | TY | TZ (vpt_device.h), 32-bit form
    DevBuf<uint32_t> tabc;     // brick Morton codes (always built; used when brick_bytes > 4 GiB, vpt_device.h cell_addr<WIDE>)
    bool wide = false;
    bool dirty = true;         // blocks uploaded since the last brickify
    bool any_upload = false;
    DevBuf<uint8_t> staging;   // blocks on their way in or out, grown on demand
    DevBuf<uint32_t> atlas;    // boundary atlas: the six outer voxel planes as 2 x 2-footprint cells (vpt_device.h sample_volume_boundary): one dword per cell
                               // and channel (byte volumes) or one float4 (float volumes; 16-bit volumes: the decoded texels); channel c's faces
                               // 6 * atlas_face cells behind c - 1's
    size_t atlas_dwords = 0;
    bool atlas_ok = true;      // float volumes: every texel is finite and < 1e37 (k_scan_finite at finalize): else the atlas is not used
    DevBuf<uint32_t> atlas_flag;
    uint32_t atlas_face = 0, atlas_shift = 0;   // dwords per face image (row pitch x rows), log2 of the row pitch
    // column records (vpt_device.h record_addr; one-channel byte volumes): built on the first MCM pass that wants them (volume_records)
    DevBuf<uint8_t> records; size_t rec_bytes = 0; bool rec_valid = false, rec_wide = false;
    DevBuf<uint32_t> rtab32, rtabc;     // RX | RY: byte offsets of the columns / their Z-order codes
};

// Tile classes (vpt_kernels.h, "Tile classes"): per reset the host sorts the 16x16 tiles into those none of whose camera rays
// can meet the cube (MISS) and the rest (HIT).  Three parts: the lists themselves with their options (here: device memory and HIP
// handles), and what the passes over them remember between two calls (vpt_pass_state.h, plain host C++ with private fields) — `track`
// for the accumulating ray marchers (marcher_track), `miss` for MCM's MISS tiles (vpt_mcm.hip).  A renderer is either MCM or a marcher:
// one of the two is always idle.
struct TileClasses {
    bool enabled = true, verify = false;   // VPT_OPTION_TILE_CLASSES (default on), VPT_OPTION_VERIFY_TILE_CLASSES
    bool one_stream = false;       // VPT_OPTION_TILE_CLASSES = 2: the MCM class kernels also where they must follow each other on one stream (each alone on the chip: measurements)
    bool valid = false;            // the lists describe `mvp` for the present geometry, and every pass since that reset used it
    float mvp[16] = {};
    DevBuf<uint32_t> list;         // device: n_hit HIT tiles, then n_miss MISS tiles, each tx | ty << 16
    int n_hit = 0, n_miss = 0;
    // what the lists on the device were built for: a reset with the same matrix and geometry (the interactive case: a transfer function or a
    // parameter changed, the camera did not) re-uses them — no classification, no upload (classes_build)
    bool built = false; float built_mvp[16] = {}; int built_geom[6] = {};
    // uploads go through two pinned staging buffers in turn, no host wait: staged[i] = the copy out of staging[i] has been enqueued and completes
    PinnedBuf<uint32_t> staging[2]; Event staged[2]; int stage_next = 0;
    DevBuf<unsigned long long> violations;
    // the packed form's records (k_mcm_miss_packed): the two jitter words of every MISS pixel's last reset, npix_padded of them in the state
    // arrays' tile order (allocated with the first packed pass); while miss.words_fresh() k_mcm_materialize rebuilds the direction array from them
    DevBuf<uint2> miss_words;
    MarcherTrack track; MissState miss;
    // what the library knows about the texels of this memory ends here: the caller may have used it in between
    void forget_destinations(const void *lo, size_t bytes = 1) { track.forget_destinations(lo, bytes); miss.forget_destinations(lo, bytes); }
};
// Split passes (VPT_OPTION_SPLIT_STREAMS = K): a sampling pass is dealt to up to K streams as tile-row ranges or parts of a tile list;
// range i runs on range_stream(r, i), the context's stream for i = 0 and a private side stream otherwise.  A pixel's pass depends on
// its own previous pass only, so the ranges never wait for each other: the launch gap, ramp and tail of one overlap the body of the
// others.  A Deal is how one launch maps the tiles to streams.  streams_deal(r, d), called before the launches, is the whole rule:
// the side streams are joined when they still hold a different deal's work (a tile's next pass must follow its last on one stream),
// and a deal of two or more ranges forks the side streams it uses behind the context's stream if that stream has enqueued anything
// since they last waited for it (dirty).  Every other entry point joins the side streams into the context's stream first (join_side).
enum { DEAL_ROWS = 0, DEAL_LISTS = 1 };
struct Deal {
    int layout = DEAL_ROWS;        // DEAL_ROWS: tile-row ranges; DEAL_LISTS: parts of the tile lists
    int ranges = 1;                // streams launched on
    bool operator==(const Deal &o) const { return layout == o.layout && ranges == o.ranges; }
    bool operator!=(const Deal &o) const { return !(*this == o); }
};
struct StreamSet {
    Stream side[VPT_MAX_SPLIT - 1];
    Event ev_fork, ev_join[VPT_MAX_SPLIT - 1];
    bool dirty = true;             // the context's stream has enqueued work the side streams have not waited for
    Deal last;                     // the deal of the last launch since the last join (a join resets it)
    bool busy() const { return last.ranges >= 2; }   // the side streams may hold work the context's stream has not joined
    void mark_dirty() { dirty = true; }
};

struct vpt_renderer {
    vpt_context *ctx = nullptr;
    int kind = 0;
    int W = 0, H = 0;
    int G = 1, g = 0, R = 8;
    int local_h = 0;
    int tiles_x = 0, tiles_y = 0, ntiles = 0;
    size_t npix_padded = 0;     // ntiles * 256
    uint64_t valid_pixels = 0;  // owned pixels inside the image
    vpt_volume *vol = nullptr;
    DevBuf<float4> tf; int tf_w = 0, tf_h = 0;
    DevBuf<float4> env; int env_w = 0, env_h = 0; float4 env_const = {}; bool env_opaque = false;   // env_opaque: every texel's alpha is 255
    DevBuf<uint8_t> frame, acc;
    DevBuf<float4> st[4];          // (MCM: 0 and 2 hold 12-byte texels, DOS: 2 and 3 hold floats — renderer_alloc_buffers)
    DevBuf<uint2> render;
    uint2 *render_target = nullptr;   // caller-owned redirect of the render buffer (or null)
    DevBuf<uint2> frame_ring; int ring_frames = 0;   // VPT_PLAY_FRAMES: VPT_FRAME_SLOTS frames of W x local_h RGBA16F (allocated on first use); frames of the last call
    DevBuf<float> ndc_x, ndc_y;    // pixel-centre NDC tables (W and H entries)
    DevBuf<FrameVar> frame_table; PinnedBuf<FrameVar> frame_staging;   // device ring of per-frame uniforms (+ the table of a captured sequence) + pinned staging
    uint64_t frames_played = 0;    // frames uploaded so far (monotonic): the ring's and the staging ring's cursor
    bool warmed = false;           // at least one eager fused render() has run (lazy allocations done)
    struct PlayGraph *play_graph = nullptr;  // cached hipGraph of a frame sequence
    DevBuf<uint32_t> work_counter; // tile counter of the persistent MCS kernel
    bool mcs_persistent = false;   // use k_mcs_persist (active-ray compaction) for the MCS generate pass: measured slower than k_mcs at every extinction tried
    LaoParams lao = { 1, 0.69f, 1, 0.05f, 1, 0.54f, 10, 0.19f, 1.0f, { 2.0f, 12.0f, 3.0f } };   // LAO renderer parameters (vpt_renderer_set_lao_params; defaults LAORenderer.js:17-108)
    DevBuf<float2> dos_samples; int dos_nsamples = 0;   // DOS: uOcclusionSamples (vpt_renderer_set_occlusion_samples)
    int dos_rect[4] = {}; bool dos_rect_valid = false;   // DOS: tile rectangle [x0, y0, x1, y1) of the previous integrate call (see dos_tile_rect)
    int dos_cur = 0;               // DOS: which of the occlusion buffers st[2|3] holds the latest slice (colour: st[0], in place)
    // VPT_OPTION_SPLIT_STREAMS = K: a sampling pass may be dealt to up to K streams (split_allowed, StreamSet)
    bool target_is_callers = false;   // render_target was set by vpt_renderer_set_render_target (not by the gather pipeline)
    bool no_split = false;         // set while a frame sequence is being captured into a hipGraph (one stream only)
    bool bucket_call = false;      // inside vpt_renderer_play_into*: the passes into the caller's bucket may use every stream, the call joins them before it returns
    const Event *stop_events = nullptr;  // gather pipeline: event i is attached to range i's launch (hipExtLaunchKernel stop event: the
    bool stop_used = false;        // dispatch packet's own completion signal, no barrier packet behind the kernel)
    int split = 1; bool split_auto = true;   // split_auto: the stream count is the library's default and follows the launch size (split_for)
    StreamSet streams;
    int boundary_atlas = 1;        // VPT_OPTION_BOUNDARY_ATLAS (default 1): MCM takes out-of-cube samples from the volume's boundary atlas
    int fast_math = 0;             // VPT_OPTION_FAST_MATH: MCM events with hardware rcp / rsq / log / sin / cos (k_mcm_integrate<.., V | VPT_V_FAST>)
    int mcm_persistent = 0;        // 0: k_mcm_integrate; 1: k_mcm_persist; 2: k_mcm_persist with next-segment prefetch // (persistent waves, state prefetch) for the MCM integrate pass
    TileClasses cls;               // MCM: HIT / MISS tile lists of the last reset's matrix (see classify_tiles)
    // tone mapping fused into the fused passes' frame store: the armed tone mapper (null: none), whether its output holds the tone-mapped
    // image of what the render buffer holds now, and the store's arguments (PassArgs.tm_*)
    struct vpt_tonemapper *tm_owner = nullptr; bool tm_valid = false; const uint8_t *tm_table = nullptr; uint32_t *tm_out = nullptr; int tm_mode = 0;
    uint64_t bucket_launches = 0;  // buckets of frames run by k_mcm_bucket_* so far (vpt_renderer_bucket_launches)
    bool bucket_kernel = false;    // VPT_OPTION_BUCKET_KERNEL: vpt_renderer_play_into runs a bucket's frames by one launch per tile class
    int hit_form = 0;              // VPT_HIT_KERNEL_FORM in the environment at creation (A/B and tests): 0 = by the number of HIT tiles, 1 = k_mcm_integrate, 2 = k_mcm_integrate_early
    int column_records = 2;        // VPT_OPTION_COLUMN_RECORDS: 0 = bricks, 1 = column records, 2 (default) = records where the bricks exceed VPT_RECORDS_AUTO_BYTES
    DevBuf<unsigned long long> samples;   // device counter (MIP/EAM/MCS)
    uint64_t samples_host = 0;     // analytic part (MCM)
    DevBuf<uint8_t> scratch;       // vpt_renderer_read: the de-tiled image, grown on demand
    bool profiling = false;
    int profile_every = 1; uint64_t profile_seq = 0;   // time every n-th launch of the dominant kernel
    EventPairs timing;             // the timed launches' event pairs; a pair's launches: 1, or the frames of a graph replay / a fused sequence
    // the same around the first launch a pass puts on a SIDE stream (tile classes: the MISS-tile kernel), for the passes `timing` samples
    EventPairs side_timing; bool timed_now = false;
};

struct vpt_tonemapper {
    vpt_context *ctx = nullptr;
    int kind = 0, W = 0, H = 0;
    vpt_renderer *source = nullptr;   // bound renderer (not owned), or null
    DevBuf<uint2> image; int image_w = 0, image_rows = 0;    // owned source texture (set_source_image), or null
    DevBuf<uint32_t> out;          // RGBA8 target, grown on demand
    int rows = 0;                  // rows of the last render
    int table_mode = VPT_TONEMAPPER_TABLE_AUTO;   // VPT_TONEMAPPER_TABLE_*
    DevBuf<uint8_t> table; bool table_valid = false; TonemapParams table_params = {};   // byte table of the current parameters (vpt_tonemap.h)
    bool fuse = true;              // VPT_TONEMAPPER_OPTION_FUSE (default on): arm the bound renderer's fused passes with this table and output
    TmFuse fuse_args = {}; bool fuse_args_valid = false;   // what the block behind the table holds (vpt_tonemap.h)
};

static const size_t COUNTER_BYTES = (size_t)VPT_COUNTER_SLOTS * VPT_COUNTER_STRIDE * sizeof(unsigned long long);

struct PlayGraph;

static inline size_t frame_elem(int kind) {
    switch (kind) {
        case VPT_RENDERER_MIP: return 1;
        case VPT_RENDERER_EAM: return 4;
        case VPT_RENDERER_MCS: return 16;
        case VPT_RENDERER_ISO: return 8;      // RGBA16F (ISORenderer.js:165-197)
        case VPT_RENDERER_DEPTH: return 4;    // R32F (DepthRenderer.js:165-189)
        case VPT_RENDERER_LAO: return 4;      // RGBA8 (LAORenderer.js:217-243)
        case VPT_RENDERER_DOS: return 0;      // colour RGBA32F (st[0]) + occlusion R32F double-buffered (st[2], st[3]), ROW-MAJOR (DOSRenderer.js:273-313)
        default: return 0;
    }
}

// ---------------------------------------------------------------------------------------------
// shared host functions (vpt_core.hip unless noted)
// ---------------------------------------------------------------------------------------------
int ensure_split_streams(vpt_renderer *r);          // creates the side streams r->split asks for, if they do not exist yet
int join_side(vpt_renderer *r);                     // the side streams' work happens-before everything enqueued on the context's stream from here on
int streams_deal(vpt_renderer *r, Deal d);          // before the launches of a deal: join and fork as the deal needs (StreamSet)
int make_args(vpt_renderer *r, const vpt_uniforms *u, bool need_volume, PassArgs *a);
int volume_create(vpt_context *c, int w, int h, int d, int format, bool zero_fill, vpt_volume **out);   // vpt_volume_create; zero_fill = false: the caller writes every texel
int volume_finish_derived(vpt_context *ctx, int filter, vpt_volume *d, vpt_volume **out);   // the shared tail of the derived volumes (gradient, window, reduce, smooth, rank, resample, combine, the voxel fields' emitters): finalize with the source's filter and hand out
int volume_records(vpt_volume *v);                  // builds the column records of a finalized one-channel byte volume if they are not current
hipError_t create_overlapping_stream(Stream *out, const vpt_renderer *r);   // overlaps r's context stream and side streams
bool invert_matrix(const float *m, double out[4][4]);               // column-major float matrix -> its inverse (double); false: singular
int classes_build(vpt_renderer *r, const float *mvp_inverse);       // tile lists of `mvp_inverse` on the device (classify_tiles)
void play_graph_free(PlayGraph *g);                                 // vpt_render.hip
void tonemappers_unbind(vpt_context *c, vpt_renderer *r);           // vpt_post.hip

// the renderer families behind the entry points of vpt_render.hip
int march_reset(vpt_renderer *r, const PassArgs &a);                // vpt_march.hip: MIP, EAM, MCS
int march_generate(vpt_renderer *r, const PassArgs &a);
int march_integrate(vpt_renderer *r, const PassArgs &a);
int march_render_frame(vpt_renderer *r, const PassArgs &a);
int march_fused(vpt_renderer *r, const PassArgs &a);
int extra_reset(vpt_renderer *r, const PassArgs &a);                // vpt_extra.hip: ISO, Depth, LAO, DOS
int extra_generate(vpt_renderer *r, const PassArgs &a);
int extra_integrate(vpt_renderer *r, const PassArgs &a);
int extra_render_frame(vpt_renderer *r, const PassArgs &a);
int extra_fused(vpt_renderer *r, const PassArgs &a);
void mat4_sums(PassArgs *a);                                        // vpt_core.hip: mvp_near / mvp_far of a->mvp_inv (make_args calls it)
int mcm_reset(vpt_renderer *r, const PassArgs &a, const vpt_uniforms *u);     // vpt_mcm.hip
int mcm_pass(vpt_renderer *r, const PassArgs &a, bool fuse_render);           // one integrate pass (tile classes where they are in force)
int mcm_render_frame(vpt_renderer *r, const PassArgs &a);
int mcm_multi(vpt_renderer *r, const PassArgs &a, uint32_t npasses, uint2 *ring);
int mcm_before_pass(vpt_renderer *r, const PassArgs &a, bool *same_matrix);
int mcm_materialize(vpt_renderer *r);
int mcm_catch_up(vpt_renderer *r);                                            // mcm_materialize if the settled forms left samples pending or the direction array behind
int mcm_environment_changed(vpt_renderer *r);                                 // the environment is about to be replaced
void mcm_events_run(vpt_renderer *r, uint64_t events);                        // every form of MCM pass counts its events here
int mcm_bucket_ready(vpt_renderer *r, const PassArgs &a, bool *ready);
int mcm_bucket(vpt_renderer *r, const PassArgs &a, const FrameVar *v, int count, void *ring, uint32_t slot_pixels, bool last_to_render_buffer,
               const uint8_t *display_table);
int launch_fused(vpt_renderer *r, const PassArgs &a);               // vpt_render.hip: the fused render() launch of the renderer's kind

struct BucketCall {              // scope of a vpt_renderer_play_into* call (vpt_renderer.bucket_call)
    vpt_renderer *r;
    explicit BucketCall(vpt_renderer *r_) : r(r_) { r->bucket_call = true; }
    ~BucketCall() { r->bucket_call = false; }
};
// frame sequences (vpt_render.hip)
int play_args(vpt_renderer *r, const vpt_uniforms *base, int count, PassArgs *a);
int play_upload_table(vpt_renderer *r, const float *vars, int count, bool graph, PassArgs *a);
int check_step(const vpt_uniforms *u);
static inline PassArgs frame_args(const PassArgs &a, const FrameVar &v) {      // eager frames carry their uniforms in the kernel arguments
    PassArgs f = a;
    f.seed = v.seed; f.offset = v.offset; f.mix = v.mix; f.light = f3{ v.lx, v.ly, v.lz };
    return f;
}

// what a VPT_FORMAT_* is, indexed by the format: the one place that knows (volume_create fills the vpt_volume fields from it)
struct VolumeFormat {
    const char *name;      // for messages
    int channels;          // of the storage: 1 or 2 (packed formats: their r and g)
    int bytes;             // per stored channel: 1, 2 (16-bit normalised) or 4 (FLOAT; packed formats are decoded into RG32F on upload)
    bool is_signed;        // signed normalised texels (VPT_V_SNORM)
    bool is_float;         // FLOAT storage (VPT_V_F32)
    int packed_bytes;      // bytes per packed source word (k_decode_packed), 0: not a packed format
};
static const VolumeFormat VOLUME_FORMATS[] = {
    { "R8", 1, 1, false, false, 0 },        { "RG8", 2, 1, false, false, 0 },            { "R32F", 1, 4, false, true, 0 },
    { "RG32F", 2, 4, false, true, 0 },      { "R8_SNORM", 1, 1, true, false, 0 },        { "RG8_SNORM", 2, 1, true, false, 0 },
    { "RGB565", 2, 4, false, true, 2 },     { "RGBA4", 2, 4, false, true, 2 },           { "RGB5_A1", 2, 4, false, true, 2 },
    { "RGB10_A2", 2, 4, false, true, 4 },   { "R11F_G11F_B10F", 2, 4, false, true, 4 },  { "RGB9_E5", 2, 4, false, true, 4 },
    { "R16", 1, 2, false, false, 0 },       { "RG16", 2, 2, false, false, 0 },           { "R16_SNORM", 1, 2, true, false, 0 },
    { "RG16_SNORM", 2, 2, true, false, 0 },
};
static_assert(sizeof(VOLUME_FORMATS) / sizeof(VOLUME_FORMATS[0]) == VPT_FORMAT_RG16_SNORM + 1, "one row per VPT_FORMAT_*");
static inline const VolumeFormat *volume_format(int format) {      // null: no such format
    return (format >= 0 && format <= VPT_FORMAT_RG16_SNORM) ? &VOLUME_FORMATS[format] : nullptr;
}
static inline const char *format_name(int format) { return volume_format(format) ? volume_format(format)->name : "?"; }
static inline bool is_march_kind(int k) { return k == VPT_RENDERER_MIP || k == VPT_RENDERER_EAM || k == VPT_RENDERER_MCS; }

// dynamic LDS of the sampling kernels: transfer-function pairs + the three brick-offset tables
static inline size_t lds_bytes(const vpt_renderer *r) {
    const vpt_volume *v = r->vol;
    return (size_t)r->tf_w * 2 * sizeof(float4) + (size_t)(v->nx + v->ny + v->nz) * 4;
}
// before a launch of `kernel` with `lds` bytes of dynamic LDS: more than a CU has cannot run, more than the default limit has to be asked for
static inline int lds_prepare(const void *kernel, size_t lds) {
    if (lds > 160 * 1024) return fail(VPT_ERR_UNSUPPORTED, "transfer function + volume tables need %zu B of LDS (> 160 KiB)", lds);
    if (lds > 64 * 1024) HIP_TRY(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return VPT_OK;
}
// grid of a grid-stride kernel over `items`, `per` of them a workgroup, `most` workgroups
static inline unsigned stream_grid(size_t items, size_t per = 256, size_t most = 8192) { return (unsigned)std::max<size_t>(1, std::min<size_t>((items + per - 1) / per, most)); }
// wall time of a phase, the stream drained at its end: lap() for a phase that runs once, lap_add() for one that comes round many times
struct PhaseClock {
    hipStream_t st; std::chrono::steady_clock::time_point t0;
    explicit PhaseClock(hipStream_t s) : st(s), t0(std::chrono::steady_clock::now()) {}
    hipError_t lap(double *ms) {
        const hipError_t e = hipStreamSynchronize(st);
        const auto t1 = std::chrono::steady_clock::now();
        *ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
        t0 = t1;
        return e;
    }
    hipError_t lap_add(double *ms) { double took; const hipError_t e = lap(&took); *ms += took; return e; }
};
static inline dim3 tile_grid(const vpt_renderer *r) { return dim3((unsigned)(r->tiles_x + 7) / 8u * 8u, (unsigned)r->tiles_y); }
// Ray-marching kernels (MIP, EAM, ISO, Depth, MCS) run as one-wave workgroups when 28 of their LDS images fit a CU: with
// the default camera only ~20 % of the tiles cross the cube, about one resident round of 4-wave workgroups, which the
// dispatcher cannot rebalance (measured: 3.3e11 samples/s against 5.7e11 when every tile crosses the cube).
static inline bool wave_blocks(const vpt_renderer *r) {
    return r->kind != VPT_RENDERER_MCM && r->kind != VPT_RENDERER_DOS && lds_bytes(r) * 28 <= 150 * 1024;
}
// may this pass be dealt to several streams?  (A frame rendered into caller memory — vpt_renderer_set_render_target — is consumed by work
// the caller enqueues on the context's stream right behind it: such passes stay on that stream unless the caller has taken the join upon
// itself (vpt_renderer_play_into*: one join per bucket of frames, at the end of the call).  The gather pipeline waits for every range itself.)
static inline bool split_allowed(const vpt_renderer *r) { return r->split >= 2 && !r->no_split && (!r->target_is_callers || r->bucket_call); }
static inline hipStream_t range_stream(const vpt_renderer *r, int i) { return i == 0 ? r->ctx->stream : r->streams.side[i - 1]; }
// one sampling launch; in the gather pipeline the range's "rendered" event rides on the dispatch itself
template <typename K>
static void launch_range(K kernel, vpt_renderer *r, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const PassArgs &a, int range) {
    if (r->stop_events) {
        hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, nullptr, r->stop_events[range].get(), 0, a);
        r->stop_used = true;
    } else {
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, a);
    }
}
// The streams a sampling launch of `tiles` tiles is dealt to.  The library's default counts (vpt_core.hip default_split) are those of a
// 1080p frame; a small frame is a handful of workgroups per stream and the fork / join edges cost more than the overlap returns — measured
// per renderer at 256^2 / 512^2 / 1024^2 (us per frame on 1 | 2 | 3 streams): EAM 39 | 46 | 49, 38 | 37 | 38, 48 (3); MIP 36 | 45 | 54,
// 40 | 34 | 38; MCS 9.8 | 12.0, 10.4 | 12.2, 14.9 | 13.8; ISO 38.8 | 43.6, 39.9 | 42.2, 45.7 | 42.4; Depth 41 | 46 | 43, 41 | 40 | 41.
// A count set through VPT_OPTION_SPLIT_STREAMS is taken as it is.
static inline int split_for(const vpt_renderer *r, int tiles) {
    int k = r->split;
    if (r->split_auto && k > 1) {
        const int per = (r->kind == VPT_RENDERER_MIP || r->kind == VPT_RENDERER_EAM || r->kind == VPT_RENDERER_DEPTH) ? 192 : (r->kind == VPT_RENDERER_LAO ? 32 : 384);
        k = std::min(k, std::max(1, tiles / per));
    }
    return k;
}
template <typename K>
static int launch_sampling(K kernel, vpt_renderer *r, const PassArgs &a) {
    const size_t lds = lds_bytes(r);
    VPT_TRY(lds_prepare((const void *)kernel, lds));
    // one-wave workgroups (the ray marchers when their LDS image is small): four times as many blocks along x, see map_pixel
    const bool wave = wave_blocks(r);
    const unsigned xmul = wave ? 4u : 1u;
    const dim3 block(wave ? 64u : (unsigned)VPT_BLOCK);
    const bool split = split_allowed(r);
    if (split) VPT_TRY(ensure_split_streams(r));
    if (r->cls.track.list_now()) {
        // the HIT tiles only (marcher_track): K equal parts of the list on the K streams
        const int k = split ? std::min(split_for(r, r->cls.n_hit), r->cls.n_hit) : 1;
        VPT_TRY(streams_deal(r, Deal{ DEAL_LISTS, k }));
        for (int i = 0; i < k; i++) {
            const int h0 = (int)((long long)r->cls.n_hit * i / k), h1 = (int)((long long)r->cls.n_hit * (i + 1) / k);
            PassArgs part = a;
            part.pm.tile_list = r->cls.list + h0; part.pm.list_n = h1 - h0;
            const unsigned blocks = wave ? (unsigned)((h1 - h0 + 7) / 8) * 32u : (unsigned)(h1 - h0);
            launch_range(kernel, r, dim3(blocks), block, lds, range_stream(r, i), part, i);
        }
        return VPT_OK;
    }
    const dim3 g = tile_grid(r);
    int k = split ? split_for(r, r->tiles_x * r->tiles_y) : 1;
    if (r->tiles_y < k) k = 1;
    VPT_TRY(streams_deal(r, Deal{ DEAL_ROWS, k }));
    for (int i = 0; i < k; i++) {                     // tile rows [g.y * i / k, g.y * (i + 1) / k)
        const unsigned y0 = g.y * i / k, y1 = g.y * (i + 1) / k;
        PassArgs part = a;
        part.pm.ty0 = (int)y0;
        launch_range(kernel, r, dim3(g.x * xmul, y1 - y0), block, lds, range_stream(r, i), part, i);
    }
    return VPT_OK;
}
// the instantiation for (addressing, filter, channels, texels): V = VPT_V_WIDE | VPT_V_NEAREST | VPT_V_RG | VPT_V_F32 | VPT_V_SNORM | VPT_V_QCUBIC |
// VPT_V_NORM16 bits
// MCM on a one-channel byte volume with the LINEAR filter: the in-cube samples come from the column records (VPT_OPTION_COLUMN_RECORDS).
// Measured (round 4, 1080p headline camera, us per frame bricks -> records): 512^3 80.0 -> 83.3, every tile HIT 143.9 -> 157.1, extinction 50
// 80.3 -> 92.9 — 256 MiB of bricks mostly live in the 256 MB Infinity Cache and a dense medium's short steps re-use brick lines, 512 MiB of
// records do neither —; 1024^3 (2 GiB of bricks, beyond every cache) 98.5 -> 96.6, HIT + MISS kernels alone 127.2 -> 122.0.  Hence AUTO.
#define VPT_RECORDS_AUTO_BYTES (512ull << 20)
static inline bool renderer_uses_records(const vpt_renderer *r) {
    const vpt_volume *v = r->vol;
    if (!(r->kind == VPT_RENDERER_MCM && v && v->channels == 1 && !v->f32 && !v->snorm && !v->norm16 && v->filter == VPT_FILTER_LINEAR && v->rtab32 != nullptr)) return false;
    return r->column_records == 1 || (r->column_records == 2 && v->brick_bytes > VPT_RECORDS_AUTO_BYTES);
}
static inline int variant_of(const vpt_renderer *r) {
    return ((r->vol->wide || (renderer_uses_records(r) && r->vol->rec_wide)) ? VPT_V_WIDE : 0) | (r->vol->filter == VPT_FILTER_NEAREST ? VPT_V_NEAREST : 0) | (r->vol->channels == 2 ? VPT_V_RG : 0) |
           (r->vol->f32 ? VPT_V_F32 : 0) | (r->vol->snorm ? VPT_V_SNORM : 0) | (r->vol->filter == VPT_FILTER_QUASI_CUBIC ? VPT_V_QCUBIC : 0) |
           (r->vol->norm16 ? VPT_V_NORM16 : 0);
}
// an UNSIGNED_BYTE one-channel volume: what the column records and the persistent forms take
static inline bool unsigned_r8(const vpt_volume *v) { return v->channels == 1 && !v->f32 && !v->snorm && !v->norm16; }
// ... with the LINEAR or NEAREST filter: the persistent forms (VPT_OPTION_*_PERSISTENT) have no quasi-cubic instantiation
static inline bool persistent_volume(const vpt_volume *v) { return unsigned_r8(v) && v->filter != VPT_FILTER_QUASI_CUBIC; }
// a renderer's sampling pass through the instantiation of its volume's variant: kernel_of(std::integral_constant<int, V>) names the kernel,
// adding what the kernel family wants on top of V (tap form, fast arithmetic)
template <typename KernelOf>
static int launch_variant(vpt_renderer *r, const PassArgs &a, KernelOf kernel_of) {
    const int v = variant_of(r);
    return dispatch_sampler_variant(v, [&](auto V) { return launch_sampling(kernel_of(V), r, a); },
                                    [&] { return fail(VPT_ERR_INVALID, "no sampling kernel for variant %d", v); });
}

// profiling: the pair of events for the launch about to be enqueued, or null — profiling is off, the launch is not the n-th
// (vpt_renderer_set_profiling(n)), or the pair could not be created: the launch then goes untimed
static inline EventPairs::Pair *profile_take(vpt_renderer *r, uint32_t launches) {
    if (!r->profiling || (r->profile_seq++ % (uint64_t)r->profile_every) != 0) return nullptr;
    return r->timing.take(launches);
}
struct Timed {   // HIP events around the dominant kernel (or around one graph replay of `launches` of them)
    vpt_renderer *r; const EventPairs::Pair *pair;
    Timed(vpt_renderer *r_, bool dominant, uint32_t launches = 1) : r(r_), pair(dominant ? profile_take(r_, launches) : nullptr) {
        if (!pair) return;
        hipEventRecord(pair->t0, r->ctx->stream);
        r->timed_now = true;
    }
    ~Timed() { if (pair) { hipEventRecord(pair->t1, r->ctx->stream); r->timed_now = false; } }
};
