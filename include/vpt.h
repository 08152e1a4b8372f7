/*
 * vpt.h — C-ABI of the MI355X-native renderer path (libvpt_hip.so).
 *
 * Drop-in boundary for the per-pixel generate / integrate / render / reset passes of the
 * MIP, EAM, MCS and MCM renderers of MOj0/vpt.  Every entry point cites the reference
 * interface (file:line under the reference tree) it replaces.  Plain pointers and sizes
 * only; no C++ or torch types.  All functions return VPT_OK (0) or a negative error code;
 * vpt_last_error() gives the message (the reference only throws Error(msg):
 * WebGL.js:14,28,180; Volume.js:40,103 — bindings convert non-zero into a thrown Error).
 *
 * Threading: like the reference (single JS thread, Ticker.js:5-8) a context is not
 * thread-safe.  Calls enqueue work on the context's HIP stream and return; only
 * vpt_context_synchronize, vpt_renderer_read* and vpt_renderer_sample_count block.
 *
 * Image convention: row 0 is the BOTTOM row (GL framebuffer origin), pixels are x-fastest.
 */
#ifndef VPT_H
#define VPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VPT_API __attribute__((visibility("default")))

#define VPT_OK               0
#define VPT_ERR_INVALID     -1   /* bad argument / bad state */
#define VPT_ERR_HIP         -2   /* HIP runtime error */
#define VPT_ERR_NO_VOLUME   -3   /* renderer has no (ready) volume: Volume.getTexture() == null, Volume.js:107-113 */
#define VPT_ERR_UNSUPPORTED -4

/* RendererFactory.js:10-23: all eight names ('mip' | 'iso' | 'eam' | 'lao' | 'mcs' | 'mcm' | 'dos' | 'depth') */
#define VPT_RENDERER_MIP 0
#define VPT_RENDERER_EAM 1
#define VPT_RENDERER_MCS 2
#define VPT_RENDERER_MCM 3
#define VPT_RENDERER_ISO   4   /* src/js/renderers/ISORenderer.js, src/glsl/renderers/ISORenderer.glsl */
#define VPT_RENDERER_DEPTH 5   /* src/js/renderers/DepthRenderer.js, src/glsl/renderers/DepthRenderer.glsl */
#define VPT_RENDERER_LAO   6   /* src/js/renderers/LAORenderer.js, src/glsl/renderers/LAORenderer.glsl */
#define VPT_RENDERER_DOS   7   /* src/js/renderers/DOSRenderer.js, src/glsl/renderers/DOSRenderer.glsl */

/* Volume.js:115-125 setFilter('linear' | 'nearest') */
#define VPT_FILTER_NEAREST 0
#define VPT_FILTER_LINEAR  1
#define VPT_FILTER_QUASI_CUBIC 2  /* setFilter('quasicubic'): the LINEAR cell and taps with smoothstep weights f' = (f * f) * (3 - 2 f) per axis
                                   * (src/glsl/mixins/quasiCubicSampling.glsl's formula): C1 where LINEAR is C0, one fetch per sample.  Every
                                   * renderer and format; not taken by column records or the persistent forms (VPT_OPTION_*_PERSISTENT) */

/* Volume formats (RAWReader.js:36-38: format RED, internalFormat R8, type UNSIGNED_BYTE) */
#define VPT_FORMAT_R8 0
#define VPT_FORMAT_R32F 2        /* format RED, internalFormat R32F (or R16F: widened exactly on upload), type FLOAT / HALF_FLOAT: the texel value
                                  * itself (not normalised), LINEAR-filtered like the byte formats (OES_texture_float_linear, RenderingContext.js:78);
                                  * blocks are uploaded as float32 */
#define VPT_FORMAT_RG8 1         /* format RG, internalFormat RG8, type UNSIGNED_BYTE: two interleaved channels, texture(uVolume, p).rg
                                  * has both and the transfer function is looked up in 2-D (MIPRenderer.glsl:45-49) */
#define VPT_FORMAT_RG32F 3       /* format RG, internalFormat RG32F (or RG16F widened on upload), type FLOAT / HALF_FLOAT: two interleaved float
                                  * channels (Volume.js:58-60 allocates whatever internalFormat the manifest names); blocks are uploaded as
                                  * interleaved float32 pairs */
#define VPT_FORMAT_R8_SNORM 4    /* format RED, internalFormat R8_SNORM, type BYTE: two's-complement bytes, texture(uVolume, p).r = max(c / 127, -1).
                                  * Stored as they are in one-byte bricks like R8 (same bricked_bytes); -128 is clamped to -127 once at
                                  * finalize; every tap is decoded to fl32(c / 127) and filtered in the R32F order: bit-identical to the R32F
                                  * volume of the decoded texels.  Blocks are uploaded as bytes.  Not taken by column records, the persistent
                                  * forms (VPT_OPTION_*_PERSISTENT) or the MCM tile classes: MCM runs its general pass on these volumes */
#define VPT_FORMAT_RG8_SNORM 5   /* format RG, internalFormat RG8_SNORM, type BYTE: two interleaved SNORM channels (as R8_SNORM; the RGB8_SNORM /
                                  * RGBA8_SNORM manifests' first two channels) */
/* Packed formats: blocks are uploaded as the packed words of their GL type (2 or 4 bytes per texel); the library decodes them on the device
 * (GL ES 3.0 rules) into (r, g) float pairs, and from then on the volume is an RG32F volume.  UNORM channels are fl32(c / (2^b - 1)). */
#define VPT_FORMAT_RGB565 6      /* format RGB, internalFormat RGB565, type UNSIGNED_SHORT_5_6_5: r = bits 15-11 / 31, g = bits 10-5 / 63 */
#define VPT_FORMAT_RGBA4 7       /* format RGBA, internalFormat RGBA4, type UNSIGNED_SHORT_4_4_4_4: r = bits 15-12 / 15, g = bits 11-8 / 15 */
#define VPT_FORMAT_RGB5_A1 8     /* format RGBA, internalFormat RGB5_A1, type UNSIGNED_SHORT_5_5_5_1: r = bits 15-11 / 31, g = bits 10-6 / 31 */
#define VPT_FORMAT_RGB10_A2 9    /* format RGBA, internalFormat RGB10_A2, type UNSIGNED_INT_2_10_10_10_REV: r = bits 9-0 / 1023, g = bits 19-10 / 1023 */
#define VPT_FORMAT_R11F_G11F_B10F 10  /* format RGB, internalFormat R11F_G11F_B10F, type UNSIGNED_INT_10F_11F_11F_REV: r = bits 10-0, g = bits 21-11
                                  * as unsigned 11-bit floats (5-bit exponent, 6-bit mantissa: exponent 0 denormal, 31 Inf / NaN).  A non-finite
                                  * texel switches the boundary atlas off, as for any float volume */
#define VPT_FORMAT_RGB9_E5 11    /* format RGB, internalFormat RGB9_E5, type UNSIGNED_INT_5_9_9_9_REV: r = bits 8-0, g = bits 17-9, shared
                                  * exponent e = bits 31-27: m * 2^(e - 24) */
/* 16-bit normalised formats (EXT_texture_norm16; opt-in on the hosts, as in WebGL).  Blocks are uploaded as little-endian uint16 (UNORM) or
 * int16 (SNORM), 2 bytes per channel, and the bricks keep 2 bytes per channel: vpt_volume_bricked_bytes is half that of R32F and twice that
 * of R8.  Every tap is decoded to the float an R32F volume of the decoded texels holds and filtered in the R32F order (NEAREST, LINEAR and
 * QUASI_CUBIC): bit-identical to that R32F / RG32F volume in every renderer.  Column records, the persistent forms (VPT_OPTION_*_PERSISTENT)
 * and VPT_OPTION_BUCKET_KERNEL are not taken, as for R32F: those options fall back to the general kernels.  The MCM tile classes are taken;
 * the boundary atlas holds the decoded texels as floats */
#define VPT_FORMAT_R16 12        /* format RED, internalFormat R16_EXT, type UNSIGNED_SHORT: texture(uVolume, p).r = fl32(c / 65535) */
#define VPT_FORMAT_RG16 13       /* format RG, internalFormat RG16_EXT, type UNSIGNED_SHORT: two interleaved UNORM channels (the RGB16_EXT /
                                  * RGBA16_EXT manifests' first two channels) */
#define VPT_FORMAT_R16_SNORM 14  /* format RED, internalFormat R16_SNORM_EXT, type SHORT: texture(uVolume, p).r = max(fl32(c / 32767), -1);
                                  * -32768 is clamped to -32767 once at finalize */
#define VPT_FORMAT_RG16_SNORM 15 /* format RG, internalFormat RG16_SNORM_EXT, type SHORT: two interleaved SNORM channels (RGB16 / RGBA16_SNORM_EXT:
                                  * the first two) */

/* Buffers readable through vpt_renderer_read (SingleBuffer.js / DoubleBuffer.js attachments) */
#define VPT_BUFFER_RENDER 0      /* RGBA16F, 8 B/pixel  (AbstractRenderer.js:142-155, getTexture() :114-116) */
#define VPT_BUFFER_FRAME  1      /* MIP R8 | EAM, LAO RGBA8 | MCS RGBA32F | ISO RGBA16F | Depth R32F  (_getFrameBufferSpec); none for MCM, DOS */
#define VPT_BUFFER_ACCUM  2      /* same formats; DOS: its RGBA32F colour attachment  (_getAccumulationBufferSpec, read side) */
#define VPT_BUFFER_MCM_POSITION      3   /* RGBA32F [pos.xyz, 0]            (MCMRenderer.js:214-263) */
#define VPT_BUFFER_MCM_DIRECTION     4   /* RGBA32F [dir.xyz, bounces]      */
#define VPT_BUFFER_MCM_TRANSMITTANCE 5   /* RGBA32F [transmittance.rgb, 0]  */
#define VPT_BUFFER_MCM_RADIANCE      6   /* RGBA32F [radiance.rgb, samples] */
#define VPT_BUFFER_DOS_OCCLUSION     7   /* R32F, the DOS renderer's second accumulation attachment (DOSRenderer.js:295-305);
                                            its colour attachment (RGBA32F) is VPT_BUFFER_ACCUM */

typedef struct vpt_context  vpt_context;
typedef struct vpt_volume   vpt_volume;
typedef struct vpt_renderer vpt_renderer;

/*
 * The uniforms the reference uploads before each draw (gl.uniform* calls in
 * MIPRenderer.js:82-97, EAMRenderer.js:99-116, MCSRenderer.js:88-117, MCMRenderer.js:91-106,155-175).
 * Values the reference draws with Math.random() (uOffset, uRandSeed, the MCS light direction)
 * are explicit inputs so a run is reproducible ("fixed-seed mode").
 * uInverseResolution is derived by the library from the renderer's size (fl32(1/W), fl32(1/H)).
 */
typedef struct vpt_uniforms {
    float    mvp_inverse[16];   /* uMvpInverseMatrix, column-major (gl-matrix layout) */
    float    rand_seed;         /* uRandSeed */
    float    offset;            /* uOffset            (MIP, EAM) */
    float    step_size;         /* uStepSize = 1/steps (MIP) or 1/slices (EAM, Depth); ISO: fl(1/float(uSteps)), the shader's own division */
    float    extinction;        /* uExtinction        (EAM, MCS, MCM, Depth) */
    float    anisotropy;        /* uAnisotropy        (MCM) */
    uint32_t max_bounces;       /* uMaxBounces        (MCM) */
    uint32_t steps;             /* uSteps             (MCM, ISO) */
    float    light_direction[3];/* uScatteringDirection (MCS) | uLight (ISO, model space, normalised: ISORenderer.js:152-166) */
    float    mix;               /* uMix (EAM, Depth: 1/frameNumber) | uInvFrameNumber (MCS) */
    float    blur;              /* uBlur              (MCM, always 0 in the reference: MCMRenderer.js:93,157) */
    float    isovalue;          /* uIsovalue          (ISO, ISORenderer.js:100) */
    float    gradient_step;     /* uGradientStep      (ISO, 0.005: ISORenderer.js:168) */
    float    threshold;         /* uThreshold         (Depth, DepthRenderer.js:112) */
    float    reserved;          /* keeps the block at 128 bytes */
} vpt_uniforms;

/* ---- context: replaces the WebGL2RenderingContext the reference passes as `gl` (RenderingContext.js:66-106) */
VPT_API int vpt_device_count(int *count);
VPT_API int vpt_context_create(int device_ordinal, vpt_context **out);
/* same, but work is enqueued on a caller-owned HIP stream (e.g. torch.cuda.current_stream().cuda_stream) so that
 * it orders with the caller's other work (RCCL collectives) without host synchronisation; the stream is not destroyed.
 *
 * Stream order (tests/test_gpu_stream_order.py asserts both lists on a caller's stream, behind a delay kernel).  Every entry point
 * takes effect in the order of the calls, after whatever the caller enqueued on the stream before the call and before whatever it
 * enqueues afterwards; device memory handed out (vpt_renderer_render_buffer_device, vpt_renderer_frame_ring_device,
 * vpt_tonemapper_output_device) or handed in (vpt_volume_upload_block_device, vpt_renderer_set_render_target, the vpt_renderer_play_into*
 * buckets) is read and written in that order.  A renderer's own render buffer behind split passes (VPT_OPTION_SPLIT_STREAMS) is
 * complete on the stream after vpt_renderer_join or any of the three *_device calls.
 *   Return WITHOUT a host wait (the work is only enqueued): vpt_volume_upload_block_device; vpt_volume_finalize of a volume that is not
 *   stored as floats; vpt_volume_set_filter; vpt_volume_reduce, vpt_volume_smooth and vpt_volume_rank with one pass, vpt_volume_combine,
 *   vpt_volume_window, vpt_volume_derive_gradient, vpt_volume_resample in its NEAREST mode; vpt_renderer_set_volume, vpt_renderer_reset
 *   (MCM: under the matrix of the last reset), vpt_renderer_render, vpt_renderer_play (VPT_PLAY_FUSED, VPT_PLAY_FRAMES),
 *   vpt_renderer_play_into, vpt_renderer_play_into_display, vpt_renderer_set_render_target, vpt_renderer_join,
 *   vpt_renderer_set_option once the side streams exist, the three *_device calls above, vpt_tonemapper_render.
 *   WAIT for the host (the stream is drained before they return): every upload from host memory (vpt_volume_upload_block,
 *   vpt_renderer_set_transfer_function, vpt_renderer_set_environment*, vpt_tonemapper_set_source_image), vpt_volume_finalize of a float
 *   volume (R32F, RG32F and the packed formats decoded into them: one scan for non-finite texels), vpt_volume_smooth / _rank with two
 *   or more passes, the filtered vpt_volume_resample, the voxel fields (vpt_volume_components, vpt_volume_distance and the volumes derived
 *   from them), every query and read-back, vpt_renderer_create, vpt_renderer_resize, every destroy, the first use of a lazily created object (the side
 *   streams of a renderer, a frame ring), vpt_context_synchronize. */
VPT_API int vpt_context_create_on_stream(int device_ordinal, void *hip_stream, vpt_context **out);
VPT_API int vpt_context_destroy(vpt_context *ctx);
VPT_API int vpt_context_synchronize(vpt_context *ctx);
VPT_API const char *vpt_last_error(void);
VPT_API const char *vpt_version(void);

/* ---- volume: Volume.js:31-78 (texStorage3D + texSubImage3D per placement), :115-125 (setFilter), :17-22 (destroy) */
VPT_API int vpt_volume_create(vpt_context *ctx, int width, int height, int depth, int format, vpt_volume **out);
VPT_API int vpt_volume_upload_block(vpt_volume *vol, int x, int y, int z, int width, int height, int depth,
                                    const void *host_data, size_t nbytes);
/* same, source already resident in HBM on this context's device (skips PCIe) */
VPT_API int vpt_volume_upload_block_device(vpt_volume *vol, int x, int y, int z, int width, int height, int depth,
                                           const void *device_data, size_t nbytes);
/* builds the bricked Z-order layout from the uploaded blocks; called implicitly by the first pass that needs it */
VPT_API int vpt_volume_finalize(vpt_volume *vol);
VPT_API int vpt_volume_set_filter(vpt_volume *vol, int filter);
VPT_API int vpt_volume_destroy(vpt_volume *vol);
/* force the > 4 GiB addressing variant (brick-code tables + computed in-brick offset; automatic when the bricked layout
 * exceeds 4 GiB); lets the wide kernel variants
 * be checked against the oracle on small volumes */
VPT_API int vpt_volume_set_wide_tables(vpt_volume *vol, int wide);
/* bytes of the bricked layout in HBM (for reporting) */
VPT_API int vpt_volume_bricked_bytes(vpt_volume *vol, uint64_t *nbytes);
/* ---- volume operations on the device (extension; DESIGN.md "Gradient-magnitude channel") */
/* The second channel of a 2-D transfer function, derived where the texels already are: a one-channel UNSIGNED NORMALISED volume
 * (VPT_FORMAT_R8, B = 8, or VPT_FORMAT_R16, B = 16) in, a new two-channel volume (RG8 / RG16) of the same size out; channel 0 is the source
 * texel, channel 1 the gradient magnitude G.  All in integers, v = the texel, indices clamped per axis (CLAMP_TO_EDGE):
 *   VPT_GRADIENT_CENTRAL: dx = v(x+1,y,z) - v(x-1,y,z), likewise dy, dz (doubled central differences); shift = 16
 *   VPT_GRADIENT_SOBEL:   dx = sum over a, b in {-1,0,1} of w(a) w(b) (v(x+1,y+a,z+b) - v(x-1,y+a,z+b)), w = (1, 2, 1), likewise dy, dz; shift = 24
 *   S = dx^2 + dy^2 + dz^2;  q = floor(gain^2 * 16384 + 0.5) (double, from the float gain);  T = (S * q) >> shift (64-bit unsigned);
 *   G = min(2^B - 1, floor(sqrt(T))), the exact integer square root.
 * With gain = 1 that is floor(|grad v|) in texel units per voxel for both operators.  Gains with q outside [1, 4194304] (gain outside
 * [1/128, 16]) and NaN: VPT_ERR_INVALID.  Float, SNORM, packed and two-channel sources: VPT_ERR_UNSUPPORTED. */
#define VPT_GRADIENT_CENTRAL 0
#define VPT_GRADIENT_SOBEL   1
/* a new, finalized RG8 / RG16 volume on src's context with src's filter, enqueued on the context's stream behind any upload into src;
 * src is not changed and may be destroyed afterwards.  The result is an ordinary volume (upload_block, set_filter, every renderer) */
VPT_API int vpt_volume_derive_gradient(vpt_volume *src, int op, float gain, vpt_volume **out);
/* texSubImage3D's inverse: the texels of a box, in the layout vpt_volume_upload_block takes them for this volume's format (packed
 * formats: the decoded RG32F texels the storage holds; SNORM: the most negative code reads as the one above it once the volume is
 * finalized); blocks until the copy has landed */
VPT_API int vpt_volume_read_block(vpt_volume *vol, int x, int y, int z, int width, int height, int depth, void *host_dst, size_t nbytes);
/* counts per bin, uint32: one-channel R8 / R16 volumes 256 bins of the value's top 8 bits (nbins = 256); RG8 / RG16 256 x 256 bins of
 * both channels' top 8 bits, bins[g * 256 + v] (nbins = 65536): what a 2-D transfer-function editor draws behind its bumps.  Other
 * formats: VPT_ERR_UNSUPPORTED.  A volume of more than 2^32 - 1 voxels: VPT_ERR_UNSUPPORTED, naming the count (the bins are 32-bit: one
 * that held the background of such a volume would wrap; vpt_volume_components refuses likewise).  Blocks. */
VPT_API int vpt_volume_histogram(vpt_volume *vol, uint32_t *bins, size_t nbins);
/* ---- value-range window (window / level) on the device (extension; DESIGN.md "Value-range window") */
/* Places a one-channel volume of any scalar format on the transfer function's [0, 1] axis: a new VPT_FORMAT_R8 (M = 255) or VPT_FORMAT_R16
 * (M = 65535) volume of the same size whose texel is 0 at or below `lo`, M at or above `hi` and linear in between.  Sources: R8, R16,
 * R8_SNORM, R16_SNORM, R32F (which includes R16F manifests, widened on upload); two-channel and packed sources: VPT_ERR_UNSUPPORTED,
 * naming the format.  out_format other than R8 / R16: VPT_ERR_INVALID.
 * The code c of a texel (integer sources) is the stored integer: 0 .. 2^B - 1 for R8 / R16; the two's-complement value for SNORM, the
 * most negative code read as the one above it (max(c, -(2^(B-1) - 1)): what finalize does once; these operations apply it themselves,
 * so their results do not depend on whether the source was finalized).  lo and hi are in code units.
 *   Integer contract (lo, hi integral, |lo|, |hi| <= 2^31, D = hi - lo >= 1; otherwise VPT_ERR_INVALID), in 64-bit integers, n = c - lo:
 *     out = 0 if n <= 0;  M if n >= D;  (2 n M + D) div (2 D) otherwise                (round half up)
 *   so R16 -> R16 with [0, 65535] and R8 -> R8 with [0, 255] are the identity, and the map is monotone.
 *   Float contract (R32F; lo, hi and hi - lo finite, hi > lo; otherwise VPT_ERR_INVALID), every operation one correctly rounded IEEE
 *   double operation, nothing fused:
 *     t = ((double) v - lo) / (hi - lo);   out = 0 if !(t > 0) (NaN and -inf included);  M if t >= 1;  else (uint) floor(t * M + 0.5)
 * vpt_amd.window_texels states both in numpy.
 * The result is a new, finalized volume on src's context with src's dimensions and filter, enqueued on the context's stream behind any
 * upload into src; src is not changed and may be destroyed afterwards.  The result is an ordinary volume (every renderer, set_filter,
 * upload_block, read_block, histogram, derive_gradient) */
VPT_API int vpt_volume_window(vpt_volume *src, double lo, double hi, int out_format, vpt_volume **out);
/* the smallest and the largest code (integer sources) or value (R32F: NaN texels ignored, infinities counted, -0 and +0 equal; a
 * volume without a texel that is not NaN: VPT_ERR_INVALID) of the same source formats.  Blocks. */
VPT_API int vpt_volume_range(vpt_volume *vol, double *lo, double *hi);
/* counts per code at full resolution, uint32: nbins = 2^B (256 or 65536), bin = code for R8 / R16, code + 2^(B-1) for R8_SNORM /
 * R16_SNORM.  R32F and every other format: VPT_ERR_UNSUPPORTED.  A volume of more than 2^32 - 1 voxels: VPT_ERR_UNSUPPORTED, naming the
 * count (the bins are 32-bit).  Blocks.  (vpt_volume_histogram counts the top 8 bits.) */
VPT_API int vpt_volume_code_histogram(vpt_volume *vol, uint32_t *bins, size_t nbins);

/* ---- the next coarser level and binomial smoothing on the device (extension; DESIGN.md "Binomial smoothing and 2x reduction") */
/* vpt_volume_reduce: a new volume in src's format with ceil(n / 2) texels per axis (an axis of 1 stays 1).  Result texel (X, Y, Z) is taken
 * per channel from the eight source texels at x in {2 X, min(2 X + 1, nx - 1)}, likewise y and z: indices are clamped, so on an odd axis the
 * last cell counts its last texel twice and no data is dropped.
 *   Integer formats (R8, RG8, R16, RG16, R8_SNORM, RG8_SNORM, R16_SNORM, RG16_SNORM): out = (sum of the eight codes + 4) >> 3 with an
 *   arithmetic shift: the floor of the mean, halves rounded up.  The code is the stored integer, for SNORM the most negative code read as
 *   the one above it (as for the window above; the result does not depend on whether the source was finalized).  32 bits hold every sum.
 *   Float formats (R32F, RG32F; R16F manifests are widened on upload): every texel is widened to double and the eight are added by IEEE
 *   double additions in this order: the two x-neighbours, then the two y-pairs, then the two z-halves,
 *     ((a000 + a100) + (a010 + a110)) + ((a001 + a101) + (a011 + a111)),                       a_xyz, nothing fused
 *   the sum is multiplied by 0.125 (exact) and rounded once to float.  Infinities follow IEEE; a cell that holds a NaN gives a NaN whose
 *   payload is not part of the contract.
 *   Packed formats (VPT_FORMAT_RGB565 .. VPT_FORMAT_RGB9_E5): VPT_ERR_UNSUPPORTED, naming the format.
 * The cube a volume occupies does not change: on an odd axis the reduced grid is therefore stretched by n / (2 ceil(n / 2)) along that axis.
 * vpt_volume_smooth: a new volume of src's size and format, `passes` (1 .. 8; otherwise VPT_ERR_INVALID) applications of the binomial
 * 3 x 3 x 3 kernel.  Sources: R8 and R16, the formats the gradient is derived from (smoothing is the step in front of it); every other format:
 * VPT_ERR_UNSUPPORTED, naming it.  One pass, in integers, v = the texel, indices clamped per axis (CLAMP_TO_EDGE), w = (1, 2, 1):
 *     W = sum over a, b, c in {-1, 0, 1} of w(a) w(b) w(c) v(x + a, y + b, z + c);   out = (W + 32) >> 6
 *   W <= 64 (2^B - 1) fits 32 bits and out never exceeds the source's largest texel: nothing saturates.  Each pass rounds once.
 * vpt_amd.reduce_texels and vpt_amd.smooth_texels state the contracts in numpy.
 * Both results are new, finalized volumes on src's context with src's filter, enqueued on the context's stream behind any upload into src;
 * src is not changed and may be destroyed afterwards.  The results are ordinary volumes (every renderer, set_filter, upload_block,
 * read_block, window, derive_gradient, and these two again) */
VPT_API int vpt_volume_reduce(vpt_volume *src, vpt_volume **out);
VPT_API int vpt_volume_smooth(vpt_volume *src, int passes, vpt_volume **out);

/* ---- median and grey-level morphology on the device (extension; DESIGN.md "Median and morphology") */
/* vpt_volume_rank: a new volume of src's size and format whose texels are rank statistics of the source's over the 3 x 3 x 3 box: the
 * edge-preserving denoiser (impulse noise is removed, not smeared) and the morphology in front of a gradient or an iso-surface.  Sources: R8
 * and R16, the formats the smoothing and the gradient take (the window makes one of any scalar volume); every other format:
 * VPT_ERR_UNSUPPORTED, naming it.  v = the texel code, indices clamped per axis (CLAMP_TO_EDGE); the neighbourhood N(x, y, z) is the 27
 * clamped taps v(x + a, y + b, z + c), a, b, c in {-1, 0, 1}, as a multiset: a clamped tap counts as often as it occurs.  One pass:
 *   VPT_RANK_MEDIAN: the 14th smallest of the 27 taps;   VPT_RANK_ERODE: the smallest;   VPT_RANK_DILATE: the largest.
 * All compares are unsigned on the whole code (R16 codes at or above 32768 are larger than those below).  `passes` p (1 .. 8; otherwise
 * VPT_ERR_INVALID): MEDIAN, ERODE and DILATE apply their pass p times; VPT_RANK_OPEN is p erosions, then p dilations; VPT_RANK_CLOSE p
 * dilations, then p erosions, inside one call (the result is finalized once).  Any other `op`: VPT_ERR_INVALID.
 *   So dilate(v) = M - erode(M - v) and median(v) = M - median(M - v), M = 2^B - 1; p erosions are the minimum over the clamped
 *   (2 p + 1)^3 box; erode <= median <= dilate and open <= v <= close; opening and closing are idempotent; a constant volume stays as it is.
 * vpt_amd.rank_texels states the contract in numpy.
 * The result is a new, finalized volume on src's context with src's filter, enqueued on the context's stream behind any upload into src;
 * src is not changed and may be destroyed afterwards.  The result is an ordinary volume (every renderer, set_filter, upload_block,
 * read_block, histogram, window, smooth, reduce, derive_gradient, and this again) */
#define VPT_RANK_MEDIAN 0
#define VPT_RANK_ERODE  1
#define VPT_RANK_DILATE 2
#define VPT_RANK_OPEN   3
#define VPT_RANK_CLOSE  4
VPT_API int vpt_volume_rank(vpt_volume *src, int op, int passes, vpt_volume **out);

/* ---- connected components of a value range on the device (extension; DESIGN.md "Connected components") */
/* The step behind an opening or closing: "keep the largest structure", "drop everything smaller than N voxels", "give each structure its own
 * row of the 2-D transfer function".  Sources: R8 and R16 (the window makes one of any scalar volume); every other format:
 * VPT_ERR_UNSUPPORTED, naming it.  Volumes of more than 2^32 - 2 voxels: VPT_ERR_UNSUPPORTED (labels and counts are 32-bit).
 *   Foreground: a voxel whose code c has lo <= c <= hi, compared as whole unsigned codes.  lo > hi, or hi above the format's largest code
 *   (255 / 65535): VPT_ERR_INVALID.
 *   Connectivity: 6 (voxels that share a face), 18 (a face or an edge) or 26 (a face, an edge or a corner); anything else VPT_ERR_INVALID.
 *   Nothing wraps and nothing is clamped: voxels outside the volume are background.  A component is a maximal connected set of foreground.
 *   Canonical order: a component's root is its voxel with the smallest linear index (z ny + y) nx + x.  Components of fewer than
 *   `min_voxels` voxels (min_voxels >= 1; 0: VPT_ERR_INVALID) are dropped; the others are listed by voxel count descending, then by root
 *   index ascending.  The rank of a voxel is the 1-based position of its component in that list (1 = the largest), and 0 for background
 *   and for the voxels of dropped components.  So no output depends on the order in which the device merges.
 * vpt_amd.components_texels, keep_texels and label_texels state the contract in numpy.
 * The handle owns a device copy of the source's texels and one uint32 rank per voxel: src is not changed and may be destroyed afterwards;
 * a viewer labels once and tries several selections.  vpt_volume_components blocks (the list is ordered on the host). */
typedef struct vpt_components vpt_components;
struct vpt_component       { uint32_t root_x, root_y, root_z, voxels; };
struct vpt_components_info { uint64_t listed, dropped, foreground_voxels, listed_voxels; };   /* components listed / dropped; voxels in range / in listed components */
VPT_API int vpt_volume_components(vpt_volume *src, uint32_t lo, uint32_t hi, int connectivity, uint32_t min_voxels, vpt_components **out);
VPT_API int vpt_components_info(vpt_components *c, struct vpt_components_info *info);
/* components first .. first + n - 1 of the canonical order (first is 0-based); a range not within `listed`: VPT_ERR_INVALID */
VPT_API int vpt_components_list(vpt_components *c, uint64_t first, uint64_t n, struct vpt_component *dst);
/* the ranks of a box of voxels, [d][h][w] uint32; the box and nbytes are checked as vpt_volume_read_block checks them.  Blocks. */
VPT_API int vpt_components_ranks(vpt_components *c, int x, int y, int z, int w, int h, int d, uint32_t *host_dst, size_t nbytes);
/* a new, finalized volume of the source's size, format and filter: the source code where first_rank <= rank <= last_rank, `fill` elsewhere.
 * 1 <= first_rank <= last_rank (last_rank may exceed `listed`) and fill <= the format's largest code; otherwise VPT_ERR_INVALID.
 * keep(1, 1, 0) is "the largest only"; keep(1, UINT64_MAX, 0) behind a min_voxels is island removal. */
VPT_API int vpt_components_keep(vpt_components *c, uint64_t first_rank, uint64_t last_rank, uint32_t fill, vpt_volume **out);
/* a new, finalized RG8 / RG16 volume with the source's filter: R the source code, G = min(rank, M), M = 255 / 65535, so a row of the 2-D
 * transfer function selects a structure; ranks beyond M share the last row (this saturation is part of the contract) */
VPT_API int vpt_components_label(vpt_components *c, vpt_volume **out);
/* Per-structure measurements (DESIGN.md "Measuring components"): dst[k] describes the component of rank first + 1 + k, k = 0 .. n - 1 (first
 * is 0-based, as in vpt_components_list); a range not within `listed`: VPT_ERR_INVALID; n = 0 checks the arguments and writes nothing (dst
 * may then be null).  Voxels whose rank lies outside the window contribute nothing.  The device table is n records and their n voxel counts (92 n bytes, freed when
 * the call returns): a caller with millions of components pages through them; a table that cannot be allocated: VPT_ERR_HIP, nothing is
 * leaked.
 *   Box and index sums: min / max of the voxel indices (inclusive), and their sums: the centroid is sum / voxels.  `voxels` is the list's.
 *   The root lies inside the box and root_z = min_z.
 *   Values: the whole unsigned codes of channel `channel` of `values` under the component's voxels: their min, max, sum and sum of squares.
 *   `values` null: the handle's own snapshot of the source's texels.  Otherwise an R8, RG8, R16 or RG16 volume (any other format:
 *   VPT_ERR_UNSUPPORTED, naming it) on the handle's context and of the handle's width, height and depth (otherwise VPT_ERR_INVALID, naming
 *   both sizes); its width is independent of the labelled source's, and it need not be finalized: the pass is enqueued on the context's
 *   stream behind any upload into it.  channel: 0, or 1 of a two-channel volume; anything else VPT_ERR_INVALID.  Typical use: label a
 *   smoothed, opened copy, then measure the original under those labels.
 *   faces: each voxel has 6 faces; a face counts when its neighbour lies outside the volume or has a different rank (rank 0, background
 *   and dropped components, is different): the surface in voxel faces, whatever connectivity the labelling used.
 *   faces = 6 voxels - 2 (face-adjacent pairs inside the component).
 *   No word can wrap: voxels <= 2^32 - 2 (the handle's limit), sum_x, sum_y, sum_z <= 4095 * 2^32, value_sum <= 65535 * 2^32,
 *   value_sum_sq <= 2^32 * 65535^2 < 2^64, faces <= 6 * 2^32.
 * Every field is an integer sum, minimum or maximum, so the result does not depend on the order the device works in: two runs give identical
 * bytes.  vpt_amd.measure_texels states the contract in numpy; vpt_amd.measure.derive gives centroid, mean, variance, extents and fill ratio.
 * The call blocks; the handle and `values` are not changed, and `values` may be destroyed afterwards. */
struct vpt_component_measure {
    uint64_t voxels;
    uint32_t min_x, min_y, min_z, max_x, max_y, max_z;   /* bounding box, inclusive */
    uint32_t value_min, value_max;                       /* whole unsigned codes of the measured channel */
    uint64_t sum_x, sum_y, sum_z;                        /* sums of voxel indices: centroid = sum / voxels */
    uint64_t value_sum, value_sum_sq;
    uint64_t faces;
};                                                       /* 88 bytes, no padding */
VPT_API int vpt_components_measure(vpt_components *c, vpt_volume *values, int channel, uint64_t first, uint64_t n, struct vpt_component_measure *dst);
/* (for measurements) the same, and the milliseconds of the measuring pass alone in *ms, the stream drained either side */
VPT_API int vpt_components_measure_timed(vpt_components *c, vpt_volume *values, int channel, uint64_t first, uint64_t n,
                                         struct vpt_component_measure *dst, double *ms);
/* a new, finalized volume of the source's size, format and filter: the source code where the voxel's rank is one of ranks[0 .. n - 1],
 * `fill` elsewhere.  Ranks are 1-based: a rank of 0 is VPT_ERR_INVALID; ranks above `listed` are ignored (as vpt_components_keep ignores a
 * last_rank beyond the list); duplicates are allowed; n = 0 gives a volume of `fill` (ranks may then be null).  fill above the format's
 * largest code: VPT_ERR_INVALID.  With the ranks a .. b the result equals vpt_components_keep(c, a, b, fill) byte for byte.
 * vpt_amd.keep_set_texels states it in numpy. */
VPT_API int vpt_components_keep_set(vpt_components *c, const uint64_t *ranks, uint64_t n, uint32_t fill, vpt_volume **out);
/* (for measurements) milliseconds of the phases of vpt_volume_components, ms[VPT_COMPONENTS_PHASES]: tile labelling, merge launches, flatten
 * launches, sizes, census + compaction, host sort, rank write; launches[2]: merge and flatten launches.  Either pointer may be null. */
#define VPT_COMPONENTS_PHASES 7
VPT_API int vpt_components_profile(vpt_components *c, double *ms, uint32_t *launches);
VPT_API int vpt_components_destroy(vpt_components *c);

/* ---- exact Euclidean distance transform of a value range on the device (extension; DESIGN.md "Distance transform") */
/* The step behind the structure has been isolated: "the tissue within r voxels of it" (a margin), "peel r voxels off it" (erosion by a
 * Euclidean ball of any radius), "colour by depth inside, or by distance from, it".  Sources: R8 and R16 (the window makes one of any scalar
 * volume); every other format: VPT_ERR_UNSUPPORTED, naming it.
 *   In range: a voxel whose code c has lo <= c <= hi, compared as whole unsigned codes.  lo > hi, or hi above the format's largest code M
 *   (255 / 65535): VPT_ERR_INVALID.
 *   Seeds: VPT_DISTANCE_TO_RANGE: the voxels in range (the result is the distance TO the structure, 0 on it); VPT_DISTANCE_TO_REST: the
 *   voxels not in range (the depth INSIDE the structure, 0 outside it); anything else VPT_ERR_INVALID.
 *   Distance: d2(v) = min over the seeds s of (vx - sx)^2 + (vy - sy)^2 + (vz - sz)^2, in voxel units, isotropic, uint32 (at most
 *   3 * 4095^2).  Nothing wraps and nothing is clamped: voxels outside the volume are neither seed nor non-seed, so the volume's border is
 *   NOT background for TO_REST.  Without any seed every d2 is VPT_DISTANCE_NONE.  The result is unique: only distances are given, never
 *   "which seed", so there is no tie to break.
 * vpt_amd.distance_squared_texels, within_texels and channel_texels state the contract in numpy.
 * The handle owns a device copy of the source's texels and one uint32 d2 per voxel: src is not changed and may be destroyed afterwards; a
 * viewer transforms once and tries several radii.  vpt_volume_distance blocks.  Two runs give identical bytes. */
#define VPT_DISTANCE_TO_RANGE 0
#define VPT_DISTANCE_TO_REST  1
#define VPT_DISTANCE_NONE 0xFFFFFFFFu
typedef struct vpt_distance vpt_distance;
struct vpt_distance_info { uint64_t seeds; uint32_t largest; };   /* the seeds; the largest finite d2, 0 when there is no seed */
VPT_API int vpt_volume_distance(vpt_volume *src, uint32_t lo, uint32_t hi, int seeds, vpt_distance **out);
VPT_API int vpt_distance_info(vpt_distance *dist, struct vpt_distance_info *info);
/* d2 of a box of voxels, [d][h][w] uint32; the box and nbytes are checked as vpt_components_ranks checks them.  Blocks. */
VPT_API int vpt_distance_squared(vpt_distance *dist, int x, int y, int z, int w, int h, int d, uint32_t *host_dst, size_t nbytes);
/* a new, finalized volume of the source's size, format and filter: the source code where r2_lo <= d2 <= r2_hi, `fill` elsewhere.
 * r2_lo > r2_hi, or fill above the format's largest code: VPT_ERR_INVALID.  VPT_DISTANCE_NONE is an ordinary value of d2 here: only
 * r2_hi = 0xFFFFFFFF selects it.  TO_RANGE and (0, r^2) is the margin of radius r; TO_REST and (r^2 + 1, 0xFFFFFFFF) the erosion by the ball. */
VPT_API int vpt_distance_within(vpt_distance *dist, uint32_t r2_lo, uint32_t r2_hi, uint32_t fill, vpt_volume **out);
/* a new, finalized RG8 / RG16 volume with the source's filter: R the source code, G = min(floor(steps sqrt(d2)), M) =
 * min(isqrt(steps^2 d2), M), isqrt the exact integer square root of the 64-bit product; steps (1 .. 256, otherwise VPT_ERR_INVALID) is
 * the rows of the 2-D transfer function per voxel of distance.  VPT_DISTANCE_NONE gives M; the saturation at M is part of the contract. */
VPT_API int vpt_distance_channel(vpt_distance *dist, int steps, vpt_volume **out);
/* (for measurements) milliseconds of the x, y and z passes of vpt_volume_distance, ms[VPT_DISTANCE_PHASES], the stream drained after each */
#define VPT_DISTANCE_PHASES 3
VPT_API int vpt_distance_profile(vpt_distance *dist, double *ms);
VPT_API int vpt_distance_destroy(vpt_distance *dist);

/* ---- local thickness: the largest inscribed ball, on the device (extension; DESIGN.md "Local thickness") */
/* The measurement behind the depth: at a voxel, the radius of the largest ball that fits inside the structure and contains the voxel
 * (trabecular thickness and spacing, vessel calibre, pore size; "colour the structure by how thick it is here", "keep the parts an
 * r-voxel ball fits into").  A voxel on the rim of a thick wall has depth 1 and thickness "the wall".
 *   Input: a vpt_distance handle `src` of either seed mode; D(c) is its squared distance at the voxel c.
 *   Centre: a voxel c with D(c) > 0.  Its ball: { v in the volume : |v - c|^2 < D(c) }: open, so it holds no seed; it may stick out of the
 *   volume, where no voxel exists (as in the distance transform, the border is not background).
 *   T2(v) = max { D(c) : v lies in the ball of c }, 0 when no ball holds v.  A maximum over integers: unique, whatever the order of work.
 *   In numpy:  T2 = zeros;  for c in argwhere(D > 0): T2[|grid - c|^2 < D[c]] = maximum(., D[c])       (vpt_amd.thickness_squared_texels
 *   states it by level sets; js/vpt/thickness.js in plain JS).
 *   It follows that T2(v) = 0 exactly where D(v) = 0; T2 >= D everywhere; max T2 = max D; { T2 >= t } is the union of the balls with
 *   D >= t.  With TO_REST the result is the thickness of the structure, with TO_RANGE that of its complement (pore size, separation).
 *   A src without any seed (info.seeds == 0) has D = VPT_DISTANCE_NONE everywhere: the result is VPT_DISTANCE_NONE everywhere (no kernel runs).
 * The result is an ordinary vpt_distance handle whose values are T2: vpt_distance_squared, _within, _channel, _info and _destroy work on it
 * unchanged; texel snapshot, format and filter are copied from src, device to device; info.seeds is src's, info.largest the largest finite
 * T2 (= src's).  within(r^2 + 1, 0xFFFFFFFF) is "the parts some inscribed ball of radius > r covers": the opening by Euclidean balls, at
 * every radius from one transform.  channel(steps) is (code, local radius in rows); steps = 2 gives the diameter in voxels; the pair
 * volume is a valid `values` argument of vpt_components_measure (mean and maximum thickness per structure).  vpt_distance_profile of the
 * result gives zeros.
 * The calls block.  src is not changed and may be destroyed afterwards.  Two runs give identical bytes.  Sizes: those vpt_volume_distance
 * takes.  A null argument, or unknown flag bits: VPT_ERR_INVALID.  A failed allocation: VPT_ERR_HIP, nothing is leaked. */
VPT_API int vpt_distance_thickness(vpt_distance *src, vpt_distance **out);
/* (for measurements) ms[VPT_THICKNESS_PHASES]: tile maxima and their ordering, the cover, info; the stream drained after each.  tiles: the
 * tiles that hold a centre (one workgroup each); visited: the centre tiles those workgroups ran over, summed. */
#define VPT_THICKNESS_PHASES 3      /* tile maxima + ordering, cover, info */
VPT_API int vpt_distance_thickness_timed(vpt_distance *src, vpt_distance **out, double *ms, uint64_t *tiles, uint64_t *visited);
/* (for tests) flags bit 0: no value cull, bit 1: no reach cull; the result is the contract's whatever the flags.  ms and visited may be null. */
VPT_API int vpt_distance_thickness_capped(vpt_distance *src, int flags, vpt_distance **out, double *ms, uint64_t *visited);

/* ---- curve skeleton and topological kernel by thinning, on the device (extension; DESIGN.md "Skeleton") */
/* The question behind "how thick": the centreline of vessels, airways, trabeculae, fibres and pore networks (how many branches, where they
 * meet, how thick along the centreline), and the homotopic erosion of any depth.  A subfield thinning: its result is a pure function of
 * the input, whatever the order of work.
 *   Input: an R8 or R16 volume `src`, a code range lo <= hi, a `mode`, a pass cap `passes`.  The object X is the set of voxels with
 *   lo <= code <= hi; everything else is background, and so is everything outside the volume (a voxel on a face of the volume has a
 *   background 6-neighbour).  Topology is (26, 6): the object is 26-connected, the background 6-connected.
 *   For a voxel p and the current X: N26(p) its 26 neighbours, N18(p) those with at most two non-zero offset components, N6(p) the six face
 *   neighbours; obj(p) = N26(p) ∩ X; C(p) = the number of 26-connected components of obj(p), adjacency taken inside N26(p), p excluded;
 *   B(p) = the number of 6-connected components of N18(p) \ X that contain a voxel of N6(p), adjacency taken inside N18(p).  p is simple
 *   iff C(p) == 1 && B(p) == 1 (Malandain-Bertrand).  Subfield of p = (x & 1) | (y & 1) << 1 | (z & 1) << 2.
 *   One pass k = 1, 2, ...:
 *     1. Border = the voxels of X that have a background 6-neighbour, taken from X as it is when the pass starts.
 *     2. For s = 0 .. 7 in this order, every p in Border ∩ X with subfield s is decided from the X at the start of the sub-step (they do
 *        not see each other: no two are 26-adjacent, so deciding them one by one in any order gives the same X):
 *          VPT_THIN_KERNEL:  delete p if it is simple.
 *          VPT_THIN_ENDS:    skip p if |obj(p)| == 1 (a curve end); otherwise delete p if it is simple.
 *          VPT_THIN_ISTHMUS: skip p if it carries the isthmus mark; otherwise, if C(p) >= 2, give p the mark (for good) and skip it;
 *                            otherwise delete p if it is simple.
 *     3. The run ends after the first pass that deletes nothing and marks nothing (converged = 1), and after pass `passes` when
 *        passes > 0 (converged says whether that pass was idle too).  passes == 0: to the fixed point.
 *   In numpy: vpt_amd.skeleton_burn_texels; in plain JS: js/vpt/skeleton.js.
 * The result is a voxel field like components and distances.  Its uint32 value per voxel is the burn pass: 0 for a voxel outside the
 * range, k for a voxel deleted in pass k, VPT_THIN_KEPT for a voxel that survived.  { value >= k } is the object after k - 1 passes: one run
 * serves a homotopic erosion of any depth.  An empty range runs no thinning kernel: passes 0, converged 1.  A single object voxel is not
 * simple (C = 0) and survives in every mode.
 * The calls block.  src is not changed and may be destroyed afterwards.  Two runs give identical bytes.  Formats other than R8 / R16:
 * VPT_ERR_UNSUPPORTED, naming the format.  Sizes: those vpt_volume_distance takes.  A null argument, lo > hi, hi beyond the format's largest
 * code, an unknown mode or passes < 0: VPT_ERR_INVALID.  A failed allocation: VPT_ERR_HIP, nothing is leaked. */
#define VPT_THIN_KERNEL  0
#define VPT_THIN_ENDS    1
#define VPT_THIN_ISTHMUS 2
#define VPT_THIN_KEPT 0xFFFFFFFFu
typedef struct vpt_skeleton vpt_skeleton;
/* passes: the passes run, the idle last one included; isolated, ends, regular, junctions: the kept voxels with 0, 1, 2 and >= 3 kept
 * 26-neighbours (they add up to kept_voxels) */
struct vpt_skeleton_info { uint64_t object_voxels, kept_voxels, passes, converged, isolated, ends, regular, junctions; };
VPT_API int vpt_volume_skeleton(vpt_volume *src, uint32_t lo, uint32_t hi, int mode, int passes, vpt_skeleton **out);
VPT_API int vpt_skeleton_info(vpt_skeleton *sk, struct vpt_skeleton_info *info);
/* the burn passes of a box of voxels, [d][h][w] uint32; the box and nbytes are checked as vpt_components_ranks checks them.  Blocks. */
VPT_API int vpt_skeleton_burn(vpt_skeleton *sk, int x, int y, int z, int w, int h, int d, uint32_t *host_dst, size_t nbytes);
/* a new, finalized volume of the source's size, format and filter: the source code where k_lo <= value <= k_hi, `fill` elsewhere.
 * k_lo <= k_hi and fill <= the format's largest code; otherwise VPT_ERR_INVALID.  within(VPT_THIN_KEPT, VPT_THIN_KEPT, 0) is the skeleton
 * as a volume: the renderers draw it, vpt_volume_combine cuts a thickness channel with it, vpt_volume_components labels its branches. */
VPT_API int vpt_skeleton_within(vpt_skeleton *sk, uint32_t k_lo, uint32_t k_hi, uint32_t fill, vpt_volume **out);
/* (for measurements) ms[VPT_SKELETON_PHASES]: seed, border marking, sub-steps, closing census, the stream drained after each (the passes'
 * times summed); launches: kernels launched; tiles: the tiles the sub-step launches worked on, summed */
#define VPT_SKELETON_PHASES 4
VPT_API int vpt_skeleton_profile(vpt_skeleton *sk, double *ms, uint64_t *launches, uint64_t *tiles);
/* (for tests) flags bit 0: no tile cull (every tile takes part in every pass); the result is the contract's whatever the flags */
VPT_API int vpt_volume_skeleton_capped(vpt_volume *src, uint32_t lo, uint32_t hi, int mode, int passes, int flags, vpt_skeleton **out);
VPT_API int vpt_skeleton_destroy(vpt_skeleton *sk);

/* ---- skeleton graph: branches, nodes, step counts and spur pruning, on the device (extension; DESIGN.md "Skeleton graph") */
/* What a centreline is for: how many branches there are, how long each is, where they meet and which are only spurs.  Every field is an
 * integer and the result is a pure function of the input, whatever the order of work.
 *   Input: a set K of voxels: the voxels of an R8 / R16 volume whose code lies in lo .. hi, compared as whole unsigned codes
 *   (vpt_volume_graph), or the kept voxels (burn == VPT_THIN_KEPT) of a skeleton (vpt_skeleton_graph).  Everything outside K, and everything
 *   outside the volume, is absent.  The contract holds for any set, thin or not.
 *   Classes: deg(p) = |N26(p) & K|; class(p) = 0 for p outside K, otherwise 1 + min(deg(p), 3): 1 isolated, 2 end, 3 regular, 4 junction.
 *   Branches: the 26-connected components of the voxels of class 1 .. 3.  Nodes: the 26-connected components of the voxels of class 4.
 *   Both are labelled in the components' canonical order (voxels descending, then root index ascending; ranks from 1).  A branch voxel has
 *   at most two neighbours in K, so a branch is one voxel, a simple path or a simple cycle.
 *   Branch record (struct vpt_graph_branch, 64 bytes, no padding), with linear index = (z height + y) width + x:
 *     voxels        the branch's voxels
 *     free_ends     its voxels of class 2
 *     attachments   the pairs (branch voxel, 26-adjacent node voxel)
 *     node_lo, _hi  the smallest and largest node rank over those pairs, 0 / 0 when there are none
 *     steps_face, steps_edge, steps_corner
 *                   the unordered 26-adjacent pairs inside the branch, plus the attachment pairs, by how many coordinates differ (1, 2, 3)
 *     tip_lo, _hi   the smallest and largest linear index among the branch's voxels with fewer than two neighbours in their own branch;
 *                   for a cycle both are its root (its smallest linear index)
 *     kind          from the other fields, the first line that applies:
 *                     VPT_GRAPH_SEGMENT   free_ends == 2
 *                     VPT_GRAPH_SPUR      free_ends == 1 && attachments == 1
 *                     VPT_GRAPH_LINK      attachments == 2 && node_lo != node_hi
 *                     VPT_GRAPH_LOOP      attachments == 2 && node_lo == node_hi
 *                     VPT_GRAPH_ISOLATED  voxels == 1            (free_ends == 0 && attachments == 0)
 *                     VPT_GRAPH_CYCLE     otherwise              (free_ends == 0 && attachments == 0 && voxels >= 3)
 *   It follows that free_ends + attachments is 0 or 2; that the steps add up to voxels - 1 + attachments for a path, to voxels for a cycle and
 *   to 0 for an isolated voxel; and that the nodes' degrees add up to the branches' attachments.
 *   Node record (struct vpt_graph_node): voxels; degree, the attachment pairs that name the node.
 *   In numpy: vpt_amd.graph.graph_texels (the authority); in plain JS: js/vpt/graph.js.
 * Length is derived on the host only: (steps_face + sqrt 2 steps_edge + sqrt 3 steps_corner) times a spacing.  It assumes cubic voxels
 * (vpt_volume_resample makes them).
 * vpt_volume_graph and vpt_skeleton_graph run on the context's stream behind any upload into src and they block, like
 * vpt_volume_components: the labelling reads counts back.  The source and the skeleton are not changed and may be destroyed afterwards.  Two
 * runs give identical bytes.  An empty K gives a graph of zero branches and nodes.  Formats other than R8 / R16: VPT_ERR_UNSUPPORTED, naming
 * the format.  More than 2^32 - 2 voxels, or more than 4096 along an axis: VPT_ERR_UNSUPPORTED.  A null argument, lo > hi, hi beyond the
 * format's largest code: VPT_ERR_INVALID.  A failed allocation: VPT_ERR_HIP, nothing is leaked. */
#define VPT_GRAPH_ISOLATED 0
#define VPT_GRAPH_SEGMENT  1
#define VPT_GRAPH_SPUR     2
#define VPT_GRAPH_LINK     3
#define VPT_GRAPH_LOOP     4
#define VPT_GRAPH_CYCLE    5
#define VPT_GRAPH_PRUNE_DEBRIS 1u
typedef struct vpt_graph vpt_graph;
struct vpt_graph_branch { uint32_t voxels, free_ends, attachments, kind, node_lo, node_hi; uint64_t steps_face, steps_edge, steps_corner, tip_lo, tip_hi; };
struct vpt_graph_node { uint64_t voxels, degree; };
/* kept_voxels = |K|; node_voxels: those of class 4; the six counts of kinds add up to branches; the step and attachment totals are over all
 * branches */
struct vpt_graph_info { uint64_t kept_voxels, node_voxels, branches, nodes, isolated, segments, spurs, links, loops, cycles,
                        steps_face, steps_edge, steps_corner, attachments; };
VPT_API int vpt_volume_graph(vpt_volume *src, uint32_t lo, uint32_t hi, vpt_graph **out);
VPT_API int vpt_skeleton_graph(vpt_skeleton *sk, vpt_graph **out);
VPT_API int vpt_graph_info(vpt_graph *g, struct vpt_graph_info *info);
/* the records of the branches / nodes of rank first + 1 .. first + n; a window not within the count: VPT_ERR_INVALID; n = 0 checks the
 * arguments and writes nothing (dst may then be null) */
VPT_API int vpt_graph_branches(vpt_graph *g, uint64_t first, uint64_t n, struct vpt_graph_branch *dst);
VPT_API int vpt_graph_nodes(vpt_graph *g, uint64_t first, uint64_t n, struct vpt_graph_node *dst);
/* the branches / the nodes as a new vpt_components handle that the caller owns (vpt_components_destroy) and that outlives the graph: ranks
 * are branch / node ranks, the texel snapshot is the source's codes (for vpt_skeleton_graph: the skeleton's own snapshot), so
 * vpt_components_keep, _keep_set, _label, _ranks, _list and _measure work on branches and nodes unchanged and speak in source codes:
 * measure(values = a thickness pair, channel 1) gives the mean and the largest radius per branch. */
VPT_API int vpt_graph_branch_components(vpt_graph *g, vpt_components **out);
VPT_API int vpt_graph_node_components(vpt_graph *g, vpt_components **out);
/* a new, finalized RG8 / RG16 volume with the source's filter: (code, class): a row of a 2-D transfer function colours ends and junctions */
VPT_API int vpt_graph_classes(vpt_graph *g, vpt_volume **out);
/* a new, finalized volume of the source's size, format and filter: the source code where the voxel is in K and its branch is not dropped,
 * `fill` elsewhere.  A branch is dropped when wf steps_face + we steps_edge + wc steps_corner <= length (64-bit arithmetic) and it is a SPUR,
 * or flag bit 0 (VPT_GRAPH_PRUNE_DEBRIS) is set and it is a SEGMENT or ISOLATED.  Node voxels always stay, so with flags = 0 the result has
 * as many 26-components as K.  One round: all spurs of a node go together (a Y whose three arms are all within `length` is reduced to its
 * node), and the result is not thinned again.  A weight above 65535, fill above the format's largest code, unknown flag bits, a null
 * argument: VPT_ERR_INVALID. */
VPT_API int vpt_graph_prune(vpt_graph *g, uint64_t length, uint32_t wf, uint32_t we, uint32_t wc, uint32_t flags, uint32_t fill, vpt_volume **out);
/* (for measurements) ms[VPT_GRAPH_PHASES]: seed, classify (counts, prefix sums, classes and the kept-voxel list), branch labelling, node
 * labelling, links, host ordering; the stream drained after each; launches: kernels of this unit launched (the labellings' are theirs) */
#define VPT_GRAPH_PHASES 6
VPT_API int vpt_graph_profile(vpt_graph *g, double *ms, uint64_t *launches);
VPT_API int vpt_graph_destroy(vpt_graph *g);

/* ---- isosurface mesh by naive surface nets, on the device (extension; DESIGN.md "Surface") */
/* What hands a structure's surface to everything else (printing, simulation, CAD, a mesh viewer), and a surface area better than a count
 * of voxel faces: one vertex per cell the surface crosses, one quad per grid edge it crosses.  No case table; vertices are shared and the
 * mesh is closed by construction.  The result is a pure function of the input in integers, in a fixed order.
 *   Input: a finalized R8, RG8, R16 or RG16 volume `src` (any other format: VPT_ERR_UNSUPPORTED, naming it); `channel` is 0, or 1 of a
 *   two-channel volume; 1 <= level <= M, where M is 255 or 65535 (otherwise VPT_ERR_INVALID).  The surface lies at code level - 1/2, so no
 *   grid point ever lies on it and there are no degenerate cases.
 *   Grid: voxel (x, y, z) is the grid point at those integer coordinates.  The grid is padded by one layer on every side: grid points run
 *   from -1 to W, H and D.  code(g) is the whole unsigned code of the channel inside the volume and 0 outside; inside(g) = code(g) >= level.
 *   A structure that touches the border is therefore closed there: outside the volume is background, as in the sibling units.
 *   Cells: cell c = (i, j, k), with -1 <= i <= W - 1 and likewise for j and k, has the eight corners c + o, o in {0, 1}^3, and twelve
 *   edges.  There are (W + 1)(H + 1)(D + 1) cells.
 *   Crossing: a grid edge (g, g + e_a) crosses when inside differs at its two ends.  Let a = code(g) and b = code(g + e_a).  Then
 *     n = |2 level - 1 - 2 a|,  d = 2 |b - a|,  t = (n 65536 + d / 2) div d   (in integers wide enough that nothing wraps: n 65536 < 2^34)
 *   t lies in 1 .. 65535.  The crossing point is g 65536 + t e_a, in fixed point of 1 / 65536 voxel.
 *   Vertex: a cell is active when at least one of its twelve edges crosses.  Let m be the number of its crossing edges and, per axis, s the
 *   sum over those edges of (crossing point - c 65536) (at most 12 * 65536).  Per axis the stored coordinate is
 *     q = (c_axis + 1) 65536 + (2 s + m) div (2 m),
 *   a uint32, at most (W + 1) 65536.  The position in voxel-index units is q / 65536 - 1.  Vertices are numbered in raster order of their
 *   cells: k slowest, then j, then i.
 *   Quads: take each crossing edge (g, a); let u = (a + 1) mod 3 and v = (a + 2) mod 3.  The quad's corners are the vertices of the cells
 *   g - e_u - e_v, g - e_v, g, g - e_u, in that order when inside(g), otherwise in the order [0, 3, 2, 1] of that list.  All four cells
 *   exist and are active (a crossing edge has an end inside the volume, so g's coordinates off the axis are real ones and g_a >= -1).
 *   Quads are numbered by g in raster order, then by axis x, y, z.  The triangles are (q0, q1, q2) and (q0, q2, q3); with this winding
 *   the right-hand normals point from the object to the background.
 *   Worked example: a 3 x 3 x 3 R8 volume of zeros with 255 at (1, 1, 1), level 128: every crossing has n = 255, d = 510, t = 32768; 8
 *   vertices and 6 quads; the vertex of cell (0, 0, 0) is (120149, 120149, 120149) (s = 163840, m = 3), that of cell (1, 1, 1) is
 *   (141995, 141995, 141995).
 *   In numpy: vpt_amd.surface.surface_texels (the authority); in plain JS: js/vpt/surface.js.
 * Limits: 2^32 or more vertices or quads: VPT_ERR_UNSUPPORTED, naming the count.  No code at or above the level: an empty surface; no emit
 * kernel runs and the reads of n = 0 succeed.  Two runs give identical bytes.
 * vpt_volume_surface runs on the context's stream behind any upload into src, and it blocks: it reads the two totals back before it
 * allocates the result, as vpt_volume_components does.  src is not changed and may be destroyed afterwards.  A null argument:
 * VPT_ERR_INVALID.  A failed allocation: VPT_ERR_HIP, nothing is leaked. */
typedef struct vpt_surface vpt_surface;
/* cells: (W + 1)(H + 1)(D + 1); inside: the voxels with code >= level; crossings[a]: the crossing edges along axis a (they add up to quads) */
struct vpt_surface_info { uint64_t vertices, quads, cells, inside; uint64_t crossings[3]; uint32_t level; int32_t width, height, depth, channel; };
VPT_API int vpt_volume_surface(vpt_volume *src, int channel, uint32_t level, vpt_surface **out);
/* (for tests) scan_words > 0: words per block of the prefix sums, so that a small volume crosses both levels of the scan; the result is
 * the contract's whatever the value */
VPT_API int vpt_volume_surface_capped(vpt_volume *src, int channel, uint32_t level, uint32_t scan_words, vpt_surface **out);
VPT_API int vpt_surface_info(vpt_surface *s, struct vpt_surface_info *info);
/* the vertices / quads first .. first + n - 1 as 3 n / 4 n uint32 words; a window not within the count: VPT_ERR_INVALID; n = 0 checks the
 * arguments and writes nothing (host_dst may then be null); nbytes below the window's bytes: VPT_ERR_INVALID.  Block. */
VPT_API int vpt_surface_vertices(vpt_surface *s, uint64_t first, uint64_t n, uint32_t *host_dst, size_t nbytes);
VPT_API int vpt_surface_quads(vpt_surface *s, uint64_t first, uint64_t n, uint32_t *host_dst, size_t nbytes);
/* the handle's buffers on the device (null for an empty surface), valid until destroy */
VPT_API int vpt_surface_device(vpt_surface *s, void **vertices, void **quads);
/* (for measurements) ms[VPT_SURFACE_PHASES]: the stream drained after each */
#define VPT_SURFACE_PHASES 5   /* inside plane, classify, prefix sums, emit vertices, emit quads */
VPT_API int vpt_surface_profile(vpt_surface *s, double *ms);
VPT_API int vpt_surface_destroy(vpt_surface *s);

/* ---- resampling to any grid size on the device (extension; DESIGN.md "Resampling") */
/* The step in front of everything that counts voxels (the rank filters' 3 x 3 x 3 box, components, distances "in voxel units"): a volume of
 * anisotropic voxels is brought to an isotropic grid, one that is too large or too coarse to a chosen size.  The result is a new, finalized
 * volume of width x height x depth texels (each 1 .. 4096; otherwise VPT_ERR_INVALID) in src's format, on src's context, with src's filter.
 * The cube the volume occupies does not change, only the grid inside it.  Any other `mode`: VPT_ERR_INVALID.  Below n is a source axis
 * length, N the matching result axis length, X a result index; every division is a floor division of non-negative integers.
 *   VPT_RESAMPLE_NEAREST: source index j = ((2 X + 1) n) div (2 N) per axis, the texel whose cell holds the centre of result texel X; the
 *   texel's bits are copied (NaN payloads included).  Every unpacked format, the ten vpt_volume_reduce takes; packed formats:
 *   VPT_ERR_UNSUPPORTED, naming the format.  The mode for label and mask volumes (vpt_components_label, vpt_distance_channel, any `fill`).
 *   VPT_RESAMPLE_FILTERED: R8, RG8, R16 and RG16, per channel, on whole unsigned codes; every other format: VPT_ERR_UNSUPPORTED, naming it.
 *   Each axis has non-negative integer tap weights with a constant sum S_axis, chosen by that axis alone:
 *     N >= n (the axis grows or stays): linear interpolation at the renderer's texel alignment, u = s n - 0.5 at s = (X + 0.5) / N, clamped
 *       to the edge.  num = (2 X + 1) n - N, D = 2 N.  num <= 0: one tap, index 0, weight D.  num >= (n - 1) D: one tap, index n - 1,
 *       weight D.  Otherwise i = num div D, f = num mod D and the taps are (i, D - f), (i + 1, f).  S_axis = 2 N.  N = n is the identity.
 *     N < n (the axis shrinks): the area average, nothing aliases and no source texel is dropped.  Source texel j has the weight
 *       w_j = min((X + 1) n, (j + 1) N) - max(X n, j N) for j = (X n) div N .. ((X + 1) n - 1) div N; every w_j is positive.  S_axis = n.
 *   With S = S_x S_y S_z and SUM = the sum over all taps of w_x w_y w_z code:   out = (2 SUM + S) div (2 S)
 *   one rounding, halves up, in 64-bit unsigned integers (S <= 8192^3 = 2^39, SUM <= 65535 S < 2^55, 2 SUM + S < 2^57).  The sum is exact,
 *   so the result does not depend on the order of the axes.  It lies within [min, max] of the source; a constant volume stays as it is;
 *   resampling the flipped volume gives the flipped result.  Halving every axis of a volume whose axes are all even equals
 *   vpt_volume_reduce byte for byte (weights N, N and (sum + 4) >> 3); on an odd axis the two differ: reduce clamps and counts the last
 *   texel twice, this averages areas.
 * vpt_amd.resample_texels states both modes in numpy; vpt_amd.isotropic_shape gives the size for cubic voxels from a spacing.
 * The result is enqueued on the context's stream behind any upload into src; src is not changed and may be destroyed afterwards.  The
 * result is an ordinary volume (every renderer, set_filter, upload_block, read_block, and every volume operation, this one included).
 * Two runs give identical bytes.  A result or a workspace (FILTERED: 4 bytes per channel of width x src height x src depth texels, freed
 * when the call returns) that cannot be allocated: VPT_ERR_HIP, nothing is leaked. */
#define VPT_RESAMPLE_NEAREST  0
#define VPT_RESAMPLE_FILTERED 1
VPT_API int vpt_volume_resample(vpt_volume *src, int width, int height, int depth, int mode, vpt_volume **out);
/* (for measurements) the same, and the milliseconds of the row pass and of the plane pass of FILTERED in ms[VPT_RESAMPLE_PHASES], the stream
 * drained after each (NEAREST: zeros) */
#define VPT_RESAMPLE_PHASES 2
VPT_API int vpt_volume_resample_timed(vpt_volume *src, int width, int height, int depth, int mode, vpt_volume **out, double *ms);

/* ---- two volumes combined or compared texel by texel on the device (extension; DESIGN.md "Combining two volumes") */
/* Every other volume operation takes one volume.  This one brings a second into the chain: a mask made on a filtered copy cuts the
 * original, a label file becomes the second channel, two acquisitions are subtracted, a volume meets its own derivative (unsharp masking).
 *   a: R8 or R16.  b: R8, RG8, R16 or RG16; b_channel (0, or 1 for a two-channel b; otherwise VPT_ERR_INVALID) names the channel of b that
 *   is read.  Every other format: VPT_ERR_UNSUPPORTED, naming it.  a and b belong to one context and have the same width, height and depth,
 *   otherwise VPT_ERR_INVALID (a size mismatch names both sizes; vpt_volume_resample brings two grids together).  a and b may be the same
 *   handle.  Below A and B are the whole unsigned codes of a texel of a and of the named channel of the same texel of b, M = 255 / 65535 the
 *   largest code of a's format and Mb that of b's.
 *   VPT_COMBINE_MASK: A where lo <= B <= hi, `fill` elsewhere; result in a's format.  b may be 8- or 16-bit whatever a is.  lo > hi,
 *     hi > Mb or fill > M: VPT_ERR_INVALID.
 *   VPT_COMBINE_MIN, _MAX, _ABSDIFF: min(A, B), max(A, B), |A - B|; a's format.
 *   VPT_COMBINE_BLEND: clamp(((wa A + wb B + 128) >> 8) + offset, 0, M); a's format.  wa and wb are in 1/256 units and lie in
 *     -4096 .. 4096, offset in -65535 .. 65535, otherwise VPT_ERR_INVALID.  >> is the arithmetic shift: the quotient is
 *     floor(x / 256 + 1 / 2), a half rounds up (-0.5 -> 0, -1.5 -> -1).  |wa A + wb B + 128| <= 2 * 4096 * 65535 + 128 < 2^31: 32-bit
 *     integers are exact.  (256, 256, 0) is the saturating sum, (256, -256, 0) the saturating difference, (128, 128, 0) the average
 *     (A + B + 1) >> 1, (-256, 0, M) the inversion, (512, -256, 0) with b = smooth(a) unsharp masking, (0, 256, 0) a channel of b alone.
 *   VPT_COMBINE_PAIR: (A, B) as an RG8 / RG16 volume.
 *   Any other op: VPT_ERR_INVALID.  Every op but MASK needs b's channel to be as wide as a's: VPT_ERR_UNSUPPORTED, naming both formats.
 *   Fields of the params an op does not name are not read.
 * vpt_amd.combine_texels states the ops in numpy, vpt_amd.compare_stats the counts below.
 * The result is a new, finalized volume on the sources' context with a's filter, enqueued on the context's stream behind any upload into
 * a or b (they need not be finalized); neither source is changed and both may be destroyed afterwards.  Every size vpt_volume_create
 * takes is taken.  Two runs give identical bytes. */
#define VPT_COMBINE_MASK    0
#define VPT_COMBINE_MIN     1
#define VPT_COMBINE_MAX     2
#define VPT_COMBINE_ABSDIFF 3
#define VPT_COMBINE_BLEND   4
#define VPT_COMBINE_PAIR    5
struct vpt_combine_params { int op; int b_channel; uint32_t lo, hi, fill; int32_t wa, wb, offset; };
VPT_API int vpt_volume_combine(vpt_volume *a, vpt_volume *b, const struct vpt_combine_params *p, vpt_volume **out);
/* (for measurements) the same, and in *ms the milliseconds of the combining pass alone, the stream drained in front of it and behind it
 * (the finalize of the result, which follows, costs more than the pass) */
VPT_API int vpt_volume_combine_timed(vpt_volume *a, vpt_volume *b, const struct vpt_combine_params *p, vpt_volume **out, double *ms);
/* a and b as above (mixed widths are taken), no volume is made: out = { voxels, differing (A != B), max |A - B|, sum |A - B|,
 * sum (A - B)^2, #(lo_a <= A <= hi_a), #(lo_b <= B <= hi_b), #(both) }, exact, on whole codes; a range with lo > hi counts nothing.
 * More than 2^32 - 1 voxels: VPT_ERR_UNSUPPORTED, naming the count; up to there sum (A - B)^2 <= (2^32 - 1) * 65535^2 < 2^64, so no word
 * of `out` can wrap.  Dice 2 both / (in_a + in_b), Jaccard, MSE and PSNR follow on the host.  Blocks.  Two runs give identical counts. */
VPT_API int vpt_volume_compare(vpt_volume *a, vpt_volume *b, int b_channel, uint32_t lo_a, uint32_t hi_a, uint32_t lo_b, uint32_t hi_b, uint64_t out[8]);

/* ---- grey-level morphological reconstruction and the geodesic operations on the device (extension; DESIGN.md "Geodesic reconstruction") */
/* The rank filters work over a fixed 3 x 3 x 3 box.  These propagate a value THROUGH a structure as far as it reaches: fill the cavities of
 * a structure, remove what touches the border, suppress maxima shallower than h, find the regional maxima of a distance channel (the seeds
 * that tell two touching structures apart).  All of them are one primitive, the reconstruction of a marker under a mask.
 *   Sources: R8, RG8, R16 and RG16 with a channel argument (0, or 1 of a two-channel volume; anything else VPT_ERR_INVALID); every other
 *   format: VPT_ERR_UNSUPPORTED, naming it.  marker and mask belong to one context and have the same width, height and depth, otherwise
 *   VPT_ERR_INVALID (a size mismatch names both sizes), and channels of the same width, otherwise VPT_ERR_UNSUPPORTED, naming both
 *   formats; they may be the same handle.  Connectivity c: 6, 18 or 26 as vpt_volume_components; anything else VPT_ERR_INVALID.  Nothing
 *   wraps and nothing is clamped: a neighbour outside the volume does not exist.  All compares are unsigned on whole codes; M = 255 / 65535.
 *   Reconstruction by dilation, R_d(marker, mask): r0 = min(marker, mask) (a marker above the mask is clamped, not refused),
 *     r_k+1(v) = min(mask(v), max(r_k(v), max over the c-neighbours u of v of r_k(u))), and the result is the first r_k with r_k+1 = r_k.
 *     Equivalently R(v) is the maximum, over all voxels s and all c-connected paths from s to v, of min(r0(s), min of the mask along the
 *     path): the result is unique, whatever order the device works in.
 *   Reconstruction by erosion: R_e(marker, mask) = M - R_d(M - marker, M - mask): r0 = max(marker, mask), min and max exchanged.
 *   vpt_volume_geodesic makes the marker on the device (it never exists as a volume).  h is 0 for the operations that take none and at
 *   most M, otherwise VPT_ERR_INVALID; any other op: VPT_ERR_INVALID.
 *     FILL_HOLES    R_e(m, src), m = src on the voxels of the volume's six faces, M elsewhere: every regional minimum not connected to
 *                   the border is raised to its rim; c is the connectivity of the path to the border
 *     CLEAR_BORDER  src - R_d(m, src), m = src on the six faces, 0 elsewhere
 *     HMAX          R_d(max(src - h, 0), src); h = 0 gives src
 *     HMIN          R_e(min(src + h, M), src)
 *     DOME          src - HMAX_h(src)
 *     MAXIMA        M where src > HMAX_1(src), 0 elsewhere: the plateaus without a higher c-neighbour.  A voxel of code 0 is never a
 *                   maximum; this is part of the contract
 *     MINIMA        M where src < HMIN_1(src), 0 elsewhere.  A voxel of code M is never a minimum
 * vpt_amd.reconstruct_texels and geodesic_texels state all of it in numpy.
 * The result is a new, finalized ONE-channel R8 / R16 volume of the sources' size and channel width on their context, with the filter of
 * marker / src: an ordinary volume for every renderer and every other volume operation.  The calls block (the host reads a word between
 * launches); the sources are not changed, need not be finalized and may be destroyed afterwards.  Two runs give identical bytes.  Volumes
 * of more than 2^32 - 2 voxels: VPT_ERR_UNSUPPORTED, like the components. */
#define VPT_RECONSTRUCT_DILATION 0
#define VPT_RECONSTRUCT_EROSION  1
#define VPT_GEODESIC_FILL_HOLES   0
#define VPT_GEODESIC_CLEAR_BORDER 1
#define VPT_GEODESIC_HMAX         2
#define VPT_GEODESIC_HMIN         3
#define VPT_GEODESIC_DOME         4
#define VPT_GEODESIC_MAXIMA       5
#define VPT_GEODESIC_MINIMA       6
VPT_API int vpt_volume_reconstruct(vpt_volume *marker, int marker_channel, vpt_volume *mask, int mask_channel, int op, int connectivity, vpt_volume **out);
VPT_API int vpt_volume_geodesic(vpt_volume *src, int channel, int op, uint32_t h, int connectivity, vpt_volume **out);
/* (for measurements) the same, and in *ms the milliseconds of the call up to the finalize of the result, the stream drained either side;
 * in *launches the launches of the propagation kernel and, unless it is null, in *tile_runs the tiles that did work, summed over them */
VPT_API int vpt_volume_reconstruct_timed(vpt_volume *marker, int marker_channel, vpt_volume *mask, int mask_channel, int op, int connectivity,
                                         vpt_volume **out, double *ms, uint32_t *launches, uint64_t *tile_runs);
VPT_API int vpt_volume_geodesic_timed(vpt_volume *src, int channel, int op, uint32_t h, int connectivity, vpt_volume **out, double *ms,
                                      uint32_t *launches, uint64_t *tile_runs);
/* (for tests) vpt_volume_reconstruct with the rounds a tile may make in LDS per launch given (the library's own: 2049, which no tile can
 * need); tile_rounds < 1: VPT_ERR_INVALID.  The result is the contract's whatever the cap; ms and launches as above, either may be null. */
VPT_API int vpt_volume_reconstruct_capped(vpt_volume *marker, int marker_channel, vpt_volume *mask, int mask_channel, int op, int connectivity,
                                          int tile_rounds, vpt_volume **out, double *ms, uint32_t *launches);

/* ---- watershed by steepest descent on a lower-completed relief on the device (extension; DESIGN.md "Watershed") */
/* The step behind the seeds: the regional maxima of a depth channel tell two touching structures apart, the watershed splits them.  The
 * result is an ordinary vpt_components handle whose components are the basins: info, list, ranks, keep, label, measure, keep_set and
 * destroy work on it unchanged.  Most watershed definitions depend on the order of flooding; here every step is a pure function of the
 * input, so no output depends on the order the device works in.
 *   Sources: `relief` is R8, RG8, R16 or RG16 with a `channel` argument read as vpt_volume_reconstruct reads one (0, or 1 of a two-channel
 *   volume; anything else VPT_ERR_INVALID); every other format: VPT_ERR_UNSUPPORTED, naming it.  M = 255 / 65535.  All compares are
 *   unsigned on whole codes.  Nothing wraps and nothing is clamped: a neighbour outside the volume does not exist.  Connectivity c: 6, 18
 *   or 26; anything else VPT_ERR_INVALID.  Volumes of more than 2^32 - 2 voxels: VPT_ERR_UNSUPPORTED, as for the components.
 *   Domain: D = { v : lo <= relief(v) <= hi }; lo > hi or hi > M: VPT_ERR_INVALID.  Only voxels of D are flooded and only voxels of D count
 *   as neighbours; everything else has rank 0.
 *   Polarity: VPT_WATERSHED_MINIMA floods from the minima, k(v) = relief(v); VPT_WATERSHED_MAXIMA from the maxima, k(v) = M - relief(v):
 *   the form for a depth channel.  Anything else: VPT_ERR_INVALID.
 *   Lower completion: d(v) = 0 if v has a c-neighbour u in D with k(u) < k(v); otherwise d(v) = 1 + min of d(u) over the c-neighbours u
 *   in D with k(u) = k(v); d(v) = infinity when no such chain reaches a voxel with d = 0.  So d is the geodesic step count, inside the
 *   level set, to the plateau's lower border, and the voxels with d = infinity are exactly the regional minima of k within D.  Two adjacent
 *   minimum voxels always have equal k.
 *   Descent: each voxel that is no minimum has one pointer p(v).  d(v) = 0: among the c-neighbours u in D with k(u) < k(v) the one of
 *   smallest k(u), then of smallest linear index (z ny + y) nx + x.  0 < d(v) < infinity: among the c-neighbours u in D with k(u) = k(v)
 *   and d(u) = d(v) - 1 the one of smallest linear index.  (k, d) falls lexicographically along p, so every walk ends on a minimum voxel.
 *   Basins: the connected components of the graph on D with the edges {v, p(v)}, and {u, v} for c-adjacent minimum voxels: a regional
 *   minimum together with every voxel whose walk ends in it.  There are no watershed-line voxels: every voxel of D belongs to exactly one
 *   basin.  Canonical order as vpt_volume_components: a basin's root is its smallest linear index; basins of fewer than `min_voxels` voxels
 *   (0: VPT_ERR_INVALID) are dropped, with rank 0; the others are ranked by voxel count descending, then by root ascending.
 *   info.foreground_voxels is |D|.
 *   The handle's texel snapshot (what keep, keep_set and label emit, and what measure reads without `values`): `texels` null: the chosen
 *   channel of the relief as a one-channel R8 / R16 snapshot.  Otherwise an R8 / R16 volume (any other format: VPT_ERR_UNSUPPORTED) of
 *   the relief's context, size and channel width (a mismatch: VPT_ERR_INVALID, naming both), whose filter the emitted volumes then carry:
 *   the emitters speak of the original volume, not of its depth.
 * vpt_amd.watershed_texels states the contract in numpy.  The calls block; the sources are not changed, need not be finalized and may be
 * destroyed afterwards.  Two runs give identical bytes. */
#define VPT_WATERSHED_MINIMA 0
#define VPT_WATERSHED_MAXIMA 1
VPT_API int vpt_volume_watershed(vpt_volume *relief, int channel, vpt_volume *texels, uint32_t lo, uint32_t hi, int polarity, int connectivity,
                                 uint32_t min_voxels, vpt_components **out);
/* (for measurements) the same, and ms[VPT_WATERSHED_PHASES]: the milliseconds of classify, the plateau launches and the links inside the
 * tiles (together they are phase 0 of vpt_components_profile, which has the common tail: merge, flatten, sizes, ...); *plateau_launches:
 * the launches of the plateau kernel.  Neither pointer may be null. */
#define VPT_WATERSHED_PHASES 3
VPT_API int vpt_volume_watershed_timed(vpt_volume *relief, int channel, vpt_volume *texels, uint32_t lo, uint32_t hi, int polarity, int connectivity,
                                       uint32_t min_voxels, vpt_components **out, double *ms, uint32_t *plateau_launches);
/* (for tests) vpt_volume_watershed with the caps given: merge_steps and flatten_steps as vpt_volume_components_capped, tile_rounds as
 * vpt_volume_reconstruct_capped (the rounds a tile of the plateau kernel may make in LDS per launch).  Caps below those siblings' minima
 * (3, 1, 1) are VPT_ERR_INVALID before any other check.  The result is the contract's whatever the caps; ms and plateau_launches as
 * above, either may be null. */
VPT_API int vpt_volume_watershed_capped(vpt_volume *relief, int channel, vpt_volume *texels, uint32_t lo, uint32_t hi, int polarity, int connectivity,
                                        uint32_t min_voxels, int merge_steps, int flatten_steps, int tile_rounds, vpt_components **out, double *ms,
                                        uint32_t *plateau_launches);

/* ---- renderer: AbstractRenderer.js:17-116 and the four subclasses */
/* new R(gl, volume, camera, environmentTexture, {resolution}) — AbstractRenderer.js:17-49; width != height is the
 * documented extension (uInverseResolution = (1/W, 1/H)).  Buffers are allocated as in _rebuildBuffers :78-92. */
VPT_API int vpt_renderer_create(vpt_context *ctx, int kind, int width, int height, vpt_renderer **out);
/* image-plane sharding (no reference counterpart): this renderer owns the row blocks b with b % world == rank,
 * rows_per_block rows each; all buffers then hold only the owned rows (vpt_renderer_local_rows). */
VPT_API int vpt_renderer_set_shard(vpt_renderer *r, int rank, int world, int rows_per_block);
VPT_API int vpt_renderer_local_rows(vpt_renderer *r, int *rows);
/* global row index of local row l (identity when unsharded); -1 for padding rows */
VPT_API int vpt_renderer_global_row(vpt_renderer *r, int local_row, int *global_row);
VPT_API int vpt_renderer_destroy(vpt_renderer *r);                                   /* destroy() :51-58 */
VPT_API int vpt_renderer_set_volume(vpt_renderer *r, vpt_volume *vol);               /* setVolume() :94-97 (caller resets) */
VPT_API int vpt_renderer_set_transfer_function(vpt_renderer *r, const uint8_t *rgba, int width, int height); /* :99-104 */
VPT_API int vpt_renderer_set_environment(vpt_renderer *r, const uint8_t *rgba, int width, int height);       /* RenderingContext.js:90-101,136-141 */
/* HDR environment maps (no reference counterpart: RenderingContext.js:95 leaves "HDRI & OpenEXR support" as a TODO).  The host texels
 * are copied raw to the device (4, 8 or 16 bytes per texel) and decoded there into the float4 table vpt_renderer_set_environment
 * fills, row 0 first (the image's top row, as an RGBA8 map).  The decode is exact:
 *   RGBA8    c / 255 per channel (correctly rounded; the same table as vpt_renderer_set_environment, bit for bit)
 *   RGBA16F  IEEE half -> float, subnormals, infinities and NaN payloads included
 *   RGBA32F  the bits as given
 *   RGBE8    Radiance shared exponent (r, g, b, e): each channel m * 2^(e - 136), exactly; e == 0 gives (0, 0, 0); alpha 1.  The
 *            convention of stb_image and three.js's RGBELoader (no +0.5 on the mantissa as in Ward's original).
 * Texel values are not validated (negative and non-finite floats are accepted, as GL accepts them).  The map is opaque for the MCS
 * fixed-point rule when every alpha is 1 (RGBA8 255, half 0x3C00, float 1.0f; RGBE always).  width and height in 1..16384;
 * a null pointer, an unknown format or another size: VPT_ERR_INVALID. */
#define VPT_ENV_RGBA8   0   /* what vpt_renderer_set_environment takes: c / 255 per channel */
#define VPT_ENV_RGBA16F 1   /* IEEE half, 8 B per texel */
#define VPT_ENV_RGBA32F 2   /* float, 16 B per texel */
#define VPT_ENV_RGBE8   3   /* Radiance shared-exponent bytes (r, g, b, e), 4 B per texel; alpha 1 */
VPT_API int vpt_renderer_set_environment_texels(vpt_renderer *r, const void *texels, int width, int height, int format);
/* The transfer-function widget's canvas as data (src/js/ui/TransferFunction/TransferFunction.js:110-121, src/glsl/TransferFunction.glsl:32-35):
 * `count` Gaussian bumps drawn in order into a cleared width x height RGBA8 target with gl.blendFunc(ONE, ONE_MINUS_SRC_ALPHA) —
 * src = color * exp(-|(position - uv) / size|^2) at the pixel centre uv, dst = src + dst * (1 - src.a), stored as UNORM8 after every
 * bump like the canvas's own 8-bit buffer — then handed over as texImage2D(canvas) hands it to setTransferFunction
 * (AbstractRenderer.js:99-104): texel row 0 = the canvas's TOP row (uv.y = 1 - 0.5 / height), and with `unpremultiply` != 0 the colour
 * divided by alpha again (what a browser does for a premultiplied WebGL canvas when UNPACK_PREMULTIPLY_ALPHA_WEBGL is false, the
 * reference's case; rounding to nearest).  Contract arithmetic (IEEE sqrt and division, the library's exp): one result on every host.
 * Parity unpinned: a browser's exp in `precision mediump` and its un-premultiplication are implementation-defined.
 * rgba_out: width * height * 4 bytes of HOST memory, the layout vpt_renderer_set_transfer_function takes. */
typedef struct vpt_tf_bump {
    float x, y;             /* position.x, position.y in [0, 1]^2 (y = 1: the top of the widget = the first texel row) */
    float sx, sy;           /* size.x, size.y */
    float r, g, b, a;       /* color */
} vpt_tf_bump;
VPT_API int vpt_transfer_function_rasterize(vpt_context *ctx, const vpt_tf_bump *bumps, int count, int width, int height,
                                            int unpremultiply, uint8_t *rgba_out);
VPT_API int vpt_renderer_resize(vpt_renderer *r, int width, int height);             /* setResolution() :106-112 (caller resets) */

/* the four hooks; integrate and reset include the DoubleBuffer swap (AbstractRenderer.js:60-76) */
VPT_API int vpt_renderer_reset(vpt_renderer *r, const vpt_uniforms *u);              /* reset(): _resetFrame + swap */
VPT_API int vpt_renderer_generate(vpt_renderer *r, const vpt_uniforms *u);           /* _generateFrame */
VPT_API int vpt_renderer_integrate(vpt_renderer *r, const vpt_uniforms *u);          /* _integrateFrame + swap */
VPT_API int vpt_renderer_render_frame(vpt_renderer *r, const vpt_uniforms *u);       /* _renderFrame */
/* render(): generate -> integrate -> swap -> renderFrame in ONE launch (same results as the three hooks) */
VPT_API int vpt_renderer_render(vpt_renderer *r, const vpt_uniforms *u);

/* Frame sequences: `count` consecutive render() passes enqueued by ONE call.  `base` holds the uniforms the frames
 * share; frame_vars holds count x 8 floats {rand_seed, offset, mix, 0, light.x, light.y, light.z, 0} — the uniforms
 * that change per frame.  mode VPT_PLAY_EAGER: count launches with the per-frame uniforms in their arguments.
 * VPT_PLAY_GRAPH: the launch sequence is captured once into a hipGraph and replayed (launch i takes its uniforms from entry i
 * of a device table that each call refills before the replay) — where that is the faster form: a captured sequence is whole-image kernels on one stream, so a
 * renderer whose passes run as tile lists and / or on several streams (the defaults) plays the sequence eagerly instead; set
 * VPT_OPTION_SPLIT_STREAMS 1 and VPT_OPTION_TILE_CLASSES 0 to get the graph.  VPT_PLAY_FUSED (MIP, EAM, MCS, MCM, ISO, Depth; MCM below 8 passes: played eagerly, the faster form there): ONE launch runs all `count` passes
 * of a pixel back to back with the photon state (MCM) or the accumulator (MIP, EAM, MCS, ISO, Depth) in registers — no
 * round trip through HBM between passes.  VPT_PLAY_FRAMES (MCM): VPT_PLAY_FUSED that still WRITES EVERY FRAME — pass f of the call
 * goes to slot f of the renderer's frame ring ([VPT_FRAME_SLOTS][local rows][width] RGBA16F, allocated on first use; count <=
 * VPT_FRAME_SLOTS): the images `count` render() calls would have shown one after the other, for a caller that displays or
 * records them later than it asks for them.  In every mode the buffers afterwards are identical to `count` calls of
 * vpt_renderer_render (the render buffer holds the last frame). */
#define VPT_PLAY_EAGER 0
#define VPT_PLAY_GRAPH 1
#define VPT_PLAY_FUSED 2
#define VPT_PLAY_FRAMES 3
#define VPT_FRAME_SLOTS 16
VPT_API int vpt_renderer_play(vpt_renderer *r, const vpt_uniforms *base, const float *frame_vars, int count, int mode);
/* frame `slot` of the last VPT_PLAY_FRAMES call ([local rows][width][4] RGBA16F), and the ring's device address (extensions: the
 * reference renders one frame per animation tick, AbstractRenderer.js:60-70, and has no frame sequences) */
/* (extension) `count` eager render() passes by one call, frame i written to caller-owned device memory at first_target + i * stride_bytes
 * (e.g. the slots of a bucket one collective will move); frame_vars as for vpt_renderer_play.  The same frames as `count` times
 * { vpt_renderer_set_render_target; vpt_renderer_render }, but the bucket's passes run on every stream of a split pass (MCM: the tile
 * classes' two kernels) and are joined ONCE, before the call returns: whatever the caller enqueues on the context's stream next sees all
 * `count` frames.  A later call with the same slots may skip texels that cannot have changed (see vpt_renderer_set_render_target). */
VPT_API int vpt_renderer_play_into(vpt_renderer *r, const vpt_uniforms *base, const float *frame_vars, int count, void *first_target, size_t stride_bytes);
VPT_API int vpt_renderer_read_frame_slot(vpt_renderer *r, int slot, void *host_dst, size_t nbytes);
VPT_API int vpt_renderer_frame_ring_device(vpt_renderer *r, void **device_ptr, size_t *slot_bytes);

/* read-back (the reference never reads back; it hands getTexture() to the tone mapper). Row-major, local rows. */
VPT_API int vpt_renderer_read(vpt_renderer *r, int buffer, void *host_dst, size_t nbytes);
/* device pointer of the row-major RGBA16F render buffer (for the RCCL frame gather) */
VPT_API int vpt_renderer_render_buffer_device(vpt_renderer *r, void **device_ptr, size_t *nbytes);
/* redirect _renderFrame output into caller-owned device memory (>= width*local_rows*8 bytes), e.g. the send buffer of
 * the frame gather; NULL restores the renderer's own render buffer (gl.bindFramebuffer analogue, SingleBuffer.js:28-32).  The first pass into a
 * target after this call writes every texel of it; later passes into the SAME target may skip texels whose value cannot have changed since
 * (the accumulating renderers' tiles that miss the volume): a caller that writes into the memory itself calls this function again */
VPT_API int vpt_renderer_set_render_target(vpt_renderer *r, void *device_ptr, size_t nbytes);
/* implementation switches (results are identical either way).  VPT_OPTION_MCS_PERSISTENT (default 0): run the MCS
 * generate pass as persistent waves with __ballot/__popcll active-ray compaction instead of one thread per pixel
 * (measured slower on MI355X at extinction 1..200 for 512^3 @ 1080p, DESIGN.md section 5: an option, never the default).  One-channel
 * byte volumes; other formats run the default kernels whatever the option says. */
#define VPT_OPTION_MCS_PERSISTENT 0
/* VPT_OPTION_MCM_PERSISTENT (default 0): 1 = run the MCM integrate pass as persistent waves walking several 8x8-pixel
 * segments (LDS tables staged once per workgroup), 2 = the same with the next segment's photon state prefetched under
 * the current segment's events.  Measured 4-8 % slower than one workgroup per tile (register pressure). */
#define VPT_OPTION_MCM_PERSISTENT 1
/* VPT_OPTION_FAST_MATH (default 0; MCM renderer): 1 = run the integrate pass with the arithmetic a GPU driver gives GLSL
 * (v_rcp_f32 / v_rsq_f32 / v_sqrt_f32 / v_log_f32 / v_sin_f32 / v_cos_f32, and algebraically equal shorter forms) instead of
 * the software routines of the bit-exact contract.  Same integer PCG stream, same decisions except within rounding error;
 * results are NOT bit-identical to the contract oracle: checked by first-event agreement and converged-image statistics
 * (tolerance in DESIGN.md section 3).  The persistent-wave option has no fast variant (it takes precedence when set). */
#define VPT_OPTION_FAST_MATH 2
/* VPT_OPTION_BOUNDARY_ATLAS (default 1; MCM renderer, LINEAR filter, one-channel volumes): the sample of an event whose position
 * lies outside the cube — taken at the clamped position and discarded by the shader (MCMRenderer.glsl:132-142) — is fetched from
 * the volume's boundary atlas (the six outer voxel planes, one dword per 2 x 2 footprint) instead of the bricks: the same
 * value bit for bit (a clamped cell has weight 0 along the clamped axis), one aligned 4-byte gather instead of two unaligned
 * 8-byte ones.  0 = always the bricks. */
#define VPT_OPTION_BOUNDARY_ATLAS 3
/* VPT_OPTION_SPLIT_STREAMS (every renderer but DOS; default since round 4: MCM 2 — the HIT | MISS kernels of the tile classes —, MIP / EAM /
 * Depth 3, ISO / MCS / LAO 2: the measured best forms at 1080p, so that a caller who sets nothing gets them (the default follows the launch size: a frame of a few hundred tiles
 * stays on one or two streams; a count set through the option is taken as it is); VPT_DEFAULT_SPLIT=1 in the environment restores 1
 * everywhere): K in 2 .. VPT_MAX_SPLIT = a pass is launched as K tile-row ranges (or K parts of a tile list), all but
 * the first on private side streams (created by the first pass that uses them).  A pixel's pass depends on its own previous pass only, so consecutive passes of the
 * ranges never wait for each other and the launch gap, ramp and tail of one range overlap the body of the others (HIP
 * streams in place of one longer launch).  Every other entry point (reads, reset, tone mapper, gather, synchronize ...) first
 * joins the side streams into the context's stream, so callers see the usual in-order semantics; while the render buffer is
 * redirected into caller memory (vpt_renderer_set_render_target, vpt_gather_*) passes stay on the context's stream, because the
 * caller's own work on that stream reads the frame; a frame sequence captured into a hipGraph (VPT_PLAY_GRAPH) stays on the capturing
 * stream.  Results identical. */
#define VPT_MAX_SPLIT 4
#define VPT_OPTION_SPLIT_STREAMS 4
/* (5: retired in round 4 — vpt_renderer_play_into* split their passes and join once per call by themselves) */
/* VPT_OPTION_TILE_CLASSES (default 1; MCM renderer, LINEAR filter, one-channel volumes with the boundary atlas; extension, no
 * reference counterpart): vpt_renderer_reset() sorts the 16x16 tiles into those none of whose camera rays (jitter included) can meet
 * the unit cube ("MISS") and the rest; while the passes keep the reset's uMvpInverseMatrix and blur == 0, a MISS tile's photon is
 * re-emitted and leaves again at every event (MCMRenderer.glsl:135-141 after resetPhoton :70-78), so its passes run a straight-line
 * kernel on 32 of the 56 state bytes per pixel.  Every buffer a caller can read is identical either way.
 * Value 2 (MCM; a measurement aid): the two class kernels also where a pass must stay on ONE stream, one after the other — each alone on the chip
 * (slower than the general kernel there, which is why 1 does not do it).
 * VPT_OPTION_VERIFY_TILE_CLASSES (default 0): the MISS-tile kernel also counts events that were inside the cube after all
 * (vpt_renderer_tile_classes' `violations`: must stay 0). */
#define VPT_OPTION_TILE_CLASSES 6
#define VPT_OPTION_VERIFY_TILE_CLASSES 7
/* (8: retired in round 4 — the library picks the HIT-tile kernel's form by the number of HIT tiles; VPT_HIT_KERNEL_FORM=1|2 in the environment
 * at renderer creation forces one for A/B measurements and tests) */
/* VPT_OPTION_BUCKET_KERNEL (default 0; MCM renderer; extension): vpt_renderer_play_into() runs up to 16 frames of its bucket by ONE launch
 * per tile class — the photon state stays in registers from the first frame to the last, launch gap, table staging and state traffic are
 * paid once per bucket instead of once per frame (what a rank's small share of a sharded frame mostly pays for) — where the tile classes
 * are in force (VPT_OPTION_TILE_CLASSES with VPT_OPTION_SPLIT_STREAMS >= 2: the defaults); elsewhere frame by
 * frame as without the option.  Every frame is rendered and written to its slot either way; results identical. */
#define VPT_OPTION_BUCKET_KERNEL 9
/* VPT_OPTION_COLUMN_RECORDS (default 2; MCM renderer, LINEAR filter, one-channel byte volumes; extension): 1 = the in-cube samples of the MCM
 * events are fetched from the volume's COLUMN RECORDS — a third layout of the same texels, built on the first MCM pass that wants it: one
 * dword per voxel holding the 2 x 2 x-y footprint of its cell, the records of a voxel column contiguous, so that the eight taps of a
 * trilinear sample are ONE dword-aligned 8-byte gather from one 64-byte sector instead of two byte-aligned windows of a 128-byte brick
 * line.  4 bytes per voxel of HBM.  Same taps, same lerps: results identical.  0 = the apron bricks, as the other renderers; 2 = records
 * where the bricks are beyond the Infinity Cache (> 512 MiB: measured 2-4 % faster there, 4-16 % slower on volumes that fit it). */
#define VPT_OPTION_COLUMN_RECORDS 10
/* VPT_OPTION_SETTLED_MISS (0 off, 1 the settled form, 2 its packed form; default 2; MCM renderer with the tile classes in force, LINEAR filter, one-channel byte volumes; extension): under a
 * 1x1 environment with finite colour every event of a MISS tile's pixel deposits the same constant, so its running mean stops moving within
 * the first events after a reset (at once for white or black; the library proves it for the colour at hand, with one 16-byte read-back where
 * it has to).  From then on the MISS-tile pass neither reads nor writes [radiance, samples] and stores no frame texel — 16 of the 32 state
 * bytes per pixel each way, no 8-byte texel; every event still runs, draw for draw, its sample executed — as long as the environment has
 * not been set since the reset, no display table rides on the fused store, the per-pixel sample count stays below 2^24 and (fused passes)
 * the destination has received every MISS texel once since the reset.  The samples owed are added before anything else reads them
 * (vpt_renderer_read, whole-image and bucket kernels, another matrix, an environment change, this option set to 0).  Every buffer a caller
 * can read is identical either way.  2: the pass also carries two 32-bit words of the random stream per pixel (the last reset's jitter
 * draws) instead of the 16-byte direction texel they determine, and the direction array of the MISS tiles is rebuilt from them before anything
 * else reads it; same preconditions, same buffers. */
#define VPT_OPTION_SETTLED_MISS 11
VPT_API int vpt_renderer_set_option(vpt_renderer *r, int option, int value);
/* (extension) how many buckets of frames vpt_renderer_play_into has run through the bucket kernels so far (VPT_OPTION_BUCKET_KERNEL) */
VPT_API int vpt_renderer_bucket_launches(vpt_renderer *r, uint64_t *launches);
/* (extension) how many passes so far ran their MISS tiles through the settled kernel (VPT_OPTION_SETTLED_MISS) */
VPT_API int vpt_renderer_settled_passes(vpt_renderer *r, uint64_t *passes);
/* (extension) tiles of each class under the last reset's matrix (all HIT when no classification is in force) and the
 * VPT_OPTION_VERIFY_TILE_CLASSES counter; any pointer may be null */
VPT_API int vpt_renderer_tile_classes(vpt_renderer *r, int *hit_tiles, int *miss_tiles, uint64_t *violations);
/* (extension, host only: touches no GPU) the classification itself for an image of width x height whose rows are sharded
 * (rank of world, rows_per_block): classes[ty * tiles_x + tx] = 1 where tile (tx, ty) of the rank's LOCAL rows is a MISS tile.
 * `classes` may be null to query the tile grid. */
VPT_API int vpt_classify_tiles(int width, int height, int rank, int world, int rows_per_block, const float *mvp_inverse,
                               uint8_t *classes, size_t nclasses, int *tiles_x, int *tiles_y);
/* (extension, no reference counterpart) Joins the side streams of a split pass (VPT_OPTION_SPLIT_STREAMS) into the context's stream: everything enqueued on that
 * stream afterwards sees every range of the passes enqueued so far.  A no-op when nothing is pending.  Every other entry point
 * that touches the renderer's buffers does this by itself. */
VPT_API int vpt_renderer_join(vpt_renderer *r);
/* the LAO renderer's own uniforms (gl.uniform* calls of LAORenderer.js:159-169; uStepSize and uExtinction travel in
 * vpt_uniforms); defaults are the reference's property defaults (LAORenderer.js:17-108) */
struct vpt_lao_params {
    int   local_ambient_occlusion;  /* uLocalAmbientOcclusion (true) */
    float lao_weight;               /* uLAOWeight (0.69) */
    int   num_lao_samples;          /* uNumLAOSamples (1) */
    float lao_step_size;            /* uLAOStepSize (0.05) */
    int   soft_shadows;             /* uSoftShadows (true) */
    float shadows_weight;           /* uShadowsWeight (0.54) */
    int   num_shadow_samples;       /* uNumShadowSamples (10) */
    float light_radius;             /* uLightRadious (0.19) */
    float light_coefficient;        /* uLightCoeficient (1.0) */
    float light_position[3];        /* uLightPosition (2, 12, 3) */
};
VPT_API int vpt_renderer_set_lao_params(vpt_renderer *r, const struct vpt_lao_params *p);
/* The DOS renderer (directional occlusion shading) sweeps the volume front to back, one view-aligned slice per
 * full-screen pass, each pass reading its neighbours' occlusion from the pass before (DOSRenderer.js:199-259):
 *   vpt_renderer_set_occlusion_samples  the RG32F texel row built by generateOcclusionSamples() (DOSRenderer.js:103-140),
 *                                       count x (x, y);
 *   vpt_renderer_integrate_slices       _integrateFrame(): `count` passes; pass s takes uOcclusionScale = slices[3s], slices[3s+1]
 *                                       and uDepth = slices[3s+2] (the `correction` vector of :243-252), uSliceDistance =
 *                                       u->step_size, uExtinction = u->extinction, uMvpInverseMatrix = u->mvp_inverse.
 * reset / render_frame / read work as for the other renderers (generate is the reference's empty hook); integrate, the
 * single-launch vpt_renderer_render, frame sequences and sharding are refused for this renderer. */
VPT_API int vpt_renderer_set_occlusion_samples(vpt_renderer *r, const float *xy, int count);
VPT_API int vpt_renderer_integrate_slices(vpt_renderer *r, const struct vpt_uniforms *u, const float *slices, int count);
/* volume samples executed since creation / last clear (SURVEY §8d metric) */
VPT_API int vpt_renderer_sample_count(vpt_renderer *r, uint64_t *count);
VPT_API int vpt_renderer_clear_sample_count(vpt_renderer *r);

/* per-launch HIP-event timing of the dominant kernel (generate for MIP/EAM/MCS, integrate for MCM) on the
 * context's stream; enable, run, then query: sum of durations in ms and number of timed launches.
 * enabled = 1 times every launch, enabled = n > 1 every n-th launch (the two event packets cost ~7 us per launch). */
VPT_API int vpt_renderer_set_profiling(vpt_renderer *r, int enabled);
VPT_API int vpt_renderer_profile(vpt_renderer *r, double *total_ms, uint32_t *launches);
/* the same for the first launch the sampled passes put on a side stream (a pass split by VPT_OPTION_SPLIT_STREAMS; with tile classes in
 * force that is the MISS-tile kernel, k_mcm_miss, while vpt_renderer_profile covers the HIT-tile kernel on the context's stream) */
VPT_API int vpt_renderer_profile_side(vpt_renderer *r, double *total_ms, uint32_t *launches);

/* ---- tone mappers (the classes of src/js/tonemappers/ and the shaders of src/glsl/tonemappers/).  One per-pixel pass:
 * RGBA16F render buffer of a renderer (AbstractToneMapper.setTexture, AbstractToneMapper.js:34-36) -> RGBA8
 * (AbstractToneMapper.js:66-79).  Source and target have the same resolution, as RenderingContext.js:184-187,223-227
 * keeps them, so the source is read texel for texel; a sharded renderer's source is its local rows. */
#define VPT_TONEMAPPER_ARTISTIC   0   /* ToneMapperFactory.js:13-24, in its order */
#define VPT_TONEMAPPER_RANGE      1
#define VPT_TONEMAPPER_REINHARD   2
#define VPT_TONEMAPPER_REINHARD2  3
#define VPT_TONEMAPPER_UNCHARTED2 4
#define VPT_TONEMAPPER_FILMIC     5
#define VPT_TONEMAPPER_UNREAL     6
#define VPT_TONEMAPPER_ACES       7
#define VPT_TONEMAPPER_LOTTES     8
#define VPT_TONEMAPPER_UCHIMURA   9
/* the gl.uniform1f values of the _renderFrame() hooks; a mapper reads only its own fields */
struct vpt_tonemap_params {
    float low, mid, high, saturation;   /* Artistic: ArtisticToneMapper.js:75-79 (defaults 0, 0.5, 1, 1) */
    float min, max;                     /* Range: RangeToneMapper.js:58-59 (0, 1) */
    float exposure;                     /* Reinhard ... Uchimura: ReinhardToneMapper.js:53 (1) */
    float gamma;                        /* all (2.2) */
};
typedef struct vpt_tonemapper vpt_tonemapper;
VPT_API int vpt_tonemapper_create(vpt_context *ctx, int kind, int width, int height, vpt_tonemapper **out);
VPT_API int vpt_tonemapper_destroy(vpt_tonemapper *t);
VPT_API int vpt_tonemapper_resize(vpt_tonemapper *t, int width, int height);           /* setResolution, :57-62 */
/* setTexture: the source is the renderer's render buffer (read at render time; NULL = the 1x1 white texture of
 * RenderingContext.js:176-181, i.e. every texel (1,1,1,1)) */
VPT_API int vpt_tonemapper_set_source(vpt_tonemapper *t, vpt_renderer *r);
/* setTexture with an image: [rows][width] RGBA16F copied from the host into a texture owned by the tone mapper */
VPT_API int vpt_tonemapper_set_source_image(vpt_tonemapper *t, const void *rgba16f, int width, int rows);
/* render(): one pass into the RGBA8 target */
VPT_API int vpt_tonemapper_render(vpt_tonemapper *t, const struct vpt_tonemap_params *p);
/* getTexture(): [rows][width] RGBA8 -> host (blocks); rows = the source's rows (the resolution's height when unsharded) */
VPT_API int vpt_tonemapper_read(vpt_tonemapper *t, void *dst, size_t nbytes);
/* (extension) vpt_renderer_play_into with the frames AS THE TONE MAPPER SHOWS THEM: frame i of `count` eager render() passes, tone-mapped to
 * RGBA8 by `t`, into caller-owned device memory at first_target + i * stride_bytes (stride >= width * local rows * 4) — half the bytes
 * of the RGBA16F frames for the collective that moves a bucket of them.  `t` must be armed on `r`: bound with vpt_tonemapper_set_source,
 * VPT_TONEMAPPER_OPTION_FUSE on, vpt_tonemapper_render called once with the parameters to show (its table form).  MCM with the tile
 * classes in force runs the bucket kernels (their frame store looks the texel up in the tone mapper's table; the renderer's own render
 * buffer is not written); otherwise frame by frame through the fused pass and a device copy of the tone mapper's output.  Texels
 * identical to vpt_tonemapper_render on the same frames.  Joins once, before it returns, as vpt_renderer_play_into does. */
VPT_API int vpt_renderer_play_into_display(vpt_renderer *r, vpt_tonemapper *t, const struct vpt_uniforms *base, const float *frame_vars, int count,
                                           void *first_target, size_t stride_bytes);
VPT_API int vpt_tonemapper_rows(vpt_tonemapper *t, int *rows);
VPT_API int vpt_tonemapper_output_device(vpt_tonemapper *t, void **ptr, size_t *nbytes);
/* Range and the eight curve mappers can run through a 65 536-entry byte table (every output byte depends on one
 * half-precision input): bit-identical output, byte gathers instead of log/exp/divisions.  AUTO (default) uses it for
 * images of >= 262 144 pixels or when the table of the current parameters already exists; Artistic does at
 * saturation 1 only (otherwise its channels are coupled). */
#define VPT_TONEMAPPER_OPTION_TABLE  0
#define VPT_TONEMAPPER_TABLE_NEVER   0
#define VPT_TONEMAPPER_TABLE_ALWAYS  1
#define VPT_TONEMAPPER_TABLE_AUTO    2
/* VPT_TONEMAPPER_OPTION_FUSE (default 1; extension): once vpt_tonemapper_render() has run in its table form on a bound renderer, that renderer's
 * fused render() passes write the tone-mapped RGBA8 texel (same table, same lookups: bit-identical) next to every RGBA16F texel they store, and
 * the following vpt_tonemapper_render() calls with unchanged parameters find their output ready and launch nothing — RenderingContext.render()
 * (RenderingContext.js:196-197: renderer.render(); toneMapper.render()) then costs one pass instead of two.  Any pass that writes the render
 * buffer another way (the separate hooks, frame sequences, a caller's render target), new parameters or a resize fall back to the separate pass. */
#define VPT_TONEMAPPER_OPTION_FUSE   1
VPT_API int vpt_tonemapper_set_option(vpt_tonemapper *t, int option, int value);

/* ---- multi-GPU frame gather (no reference counterpart).  One process per GPU; the image plane is sharded
 * with vpt_renderer_set_shard and every frame is all-gathered over RCCL/xGMI.  The pipeline lives below the C ABI so
 * that a frame costs the host two enqueues: kernel k+1 (context stream) overlaps the all_gather of frame k (own
 * communication stream), ordered by HIP events; send/receive buffers are double-buffered. */
typedef struct vpt_gather vpt_gather;
/* RCCL bootstrap: ONE rank obtains the 128-byte id and shares it with the others out of band (e.g. torch.distributed) */
VPT_API int vpt_gather_unique_id(void *id128);
/* collective: every rank of `world` calls it with the same id; the renderer must already be sharded (rank, world) */
VPT_API int vpt_gather_create(vpt_renderer *r, const void *id128, int rank, int world, vpt_gather **out);
VPT_API int vpt_gather_destroy(vpt_gather *g);
/* who receives the frames: root = -1 (default) every rank (RCCL all_gather); root = k only rank k, the display rank
 * (grouped ncclSend/ncclRecv: 1/world of the all_gather traffic).  Collective: every rank passes the same root. */
VPT_API int vpt_gather_set_root(vpt_gather *g, int root);
/* render() of the renderer into the next send buffer + asynchronous gather of it */
VPT_API int vpt_gather_render(vpt_gather *g, const vpt_uniforms *u);
/* `count` passes of the pipeline by one call (frame_vars as for vpt_renderer_play).  VPT_PLAY_EAGER: count frames, each
 * rendered and gathered; VPT_PLAY_FUSED (MCM): the count passes run in one launch and the resulting frame is gathered
 * once.  No graph mode — a captured graph holding RCCL collectives measured slower and unstable on this stack
 * (DESIGN.md section 7). */
VPT_API int vpt_gather_play(vpt_gather *g, const vpt_uniforms *base, const float *frame_vars, int count, int mode);
/* blocks until every enqueued frame has been rendered and gathered */
VPT_API int vpt_gather_synchronize(vpt_gather *g);
/* the most recently gathered frame, rows put back in order: [height][width] RGBA16F -> host (blocks) */
VPT_API int vpt_gather_read_frame(vpt_gather *g, void *host_dst, size_t nbytes);

/* ---- test probes: evaluate device-side building blocks on the GPU (tests/ compares with the oracle) */
#define VPT_PROBE_LOG     0   /* out[i] = log(in[i]) */
#define VPT_PROBE_SIN     1
#define VPT_PROBE_COS     2
#define VPT_PROBE_ASIN    3
#define VPT_PROBE_ATAN2   4   /* in = pairs (y, x) ; n outputs */
#define VPT_PROBE_PCG     5   /* bit patterns: out[i] = pcg(in[i]) */
#define VPT_PROBE_UNIFORM 6   /* bit pattern state in -> float uniform out */
#define VPT_PROBE_F16     7   /* out[i] (low 16 bits) = half(in[i]) */
#define VPT_PROBE_RCP     8   /* software reciprocal rcp_nr */
#define VPT_PROBE_RSQRT   9   /* software reciprocal square root rsqrt_nr */
#define VPT_PROBE_MIN     10  /* in = pairs (a, b) ; n outputs */
#define VPT_PROBE_MAX     11
#define VPT_PROBE_LOG_UNIFORM 12  /* log on the range of random_uniform */
#define VPT_PROBE_RCPZ    13  /* rcp_nrz: reciprocal with 1/(+-0) = +-inf */
#define VPT_PROBE_SQRT    14  /* sqrt_nr = x * rsqrt_nr(x) */
#define VPT_PROBE_EXP     15  /* the tone mappers' exp */
#define VPT_PROBE_POW     16  /* in = pairs (x, y): exp(y * log(x)) ; n outputs */
VPT_API int vpt_probe_math(vpt_context *ctx, int which, const float *in, float *out, size_t n);
/* samples texture(uVolume, p) -> transfer function at n positions (xyz triples); out = n RGBA float4 */
VPT_API int vpt_probe_sample(vpt_renderer *r, const float *xyz, float *rgba, size_t n);
/* the same through the volume's boundary atlas for positions outside the cube (what the MCM kernels execute for out-of-cube events; positions
 * inside go through the bricks): must equal vpt_probe_sample bit for bit in every volume format */
VPT_API int vpt_probe_sample_boundary(vpt_renderer *r, const float *xyz, float *rgba, size_t n);
/* the renderer's decoded environment table: width * height float4 texels, row 0 first, into rgba (room for n texels, n >= width * height) */
VPT_API int vpt_probe_environment_texels(vpt_renderer *r, float *rgba, size_t n);
/* The schedule of frame number `frame` of the gather pipeline as a pure host function (no GPU, no communicator needed): ring
 * buffer, event edges, render destination, RCCL operation.  vpt_gather_render / _play execute exactly this plan; exported so
 * that the multi-rank schedule can be checked without more than one GPU (tests/test_gather_schedule.py). */
#define VPT_GATHER_OP_NONE      0   /* one rank, rooted: nothing to exchange */
#define VPT_GATHER_OP_ALLGATHER 1   /* root -1: ncclAllGather(send[buffer] -> recv[buffer]) */
#define VPT_GATHER_OP_SEND      2   /* rooted, this rank is not the root: ncclSend(send[buffer]) to `peer` */
#define VPT_GATHER_OP_RECV      3   /* rooted, this rank is the root: `npeers` grouped ncclRecv into recv[buffer] (vpt_gather_plan_recv) */
typedef struct vpt_gather_step {
    int      ring;             /* buffers in the ring */
    int      buffer;           /* frame % ring */
    int      parity;           /* which half of the ring: (frame / (ring / 2)) & 1 */
    int      wait_gathered;    /* compute stream waits for gathered[parity] before the kernel (the half is re-entered) */
    int      record_gathered;  /* communication stream records gathered[parity] after this frame's exchange */
    int      rendered_event;   /* rendered[k]: kernel done -> the communication stream may start */
    int      in_place;         /* the kernel renders into recv[buffer] + render_offset (root of a rooted gather) instead of send[buffer] */
    int      op;               /* VPT_GATHER_OP_* */
    int      peer;             /* SEND: destination rank */
    int      npeers;           /* RECV: number of receives */
    uint64_t render_offset;    /* byte offset of the kernel's output inside recv[buffer] when in_place */
} vpt_gather_step;
VPT_API int vpt_gather_plan(uint64_t frame, int rank, int world, int root, uint64_t send_bytes, vpt_gather_step *out);
VPT_API int vpt_gather_plan_recv(const vpt_gather_step *step, int rank, int i, uint64_t send_bytes, int *peer, uint64_t *offset);
/* the row re-assembly of a gathered frame (k_assemble_rows, used by vpt_gather_read_frame) run on host data:
 * gathered = [world][local_rows][width] RGBA16F as the ranks' send buffers arrive, out = [height][width].  Lets a
 * one-GPU box check the multi-rank assembly against an unsharded frame. */
VPT_API int vpt_probe_assemble_rows(vpt_context *ctx, const void *gathered, int width, int height, int local_rows,
                                    int world, int rows_per_block, void *out);
/* measured HBM streaming-read rate: `iterations` grid-stride 16 B/lane reads of an nbytes scratch buffer (choose it far
 * larger than the 256 MB Infinity Cache); the second denominator SURVEY section 8d asks for next to the 8 TB/s peak */
VPT_API int vpt_probe_stream_read(vpt_context *ctx, size_t nbytes, int iterations, double *gb_per_s);
/* (for tests) vpt_volume_components with the two step caps given: the loads a unite of the merge and a voxel of the flatten may take in one
 * launch (vpt_volume_components passes 1024 and 64).  Small caps make the host's retry loops run on small volumes: the second and later
 * merge launches behind a unite that gave up, and the second and later flatten launches.  The result is the contract's whatever the caps.
 * Caps for which the loops' bounds do not hold, merge_steps < 3 or flatten_steps < 1, are VPT_ERR_INVALID, the message naming the smallest
 * value taken; they are checked before every other argument and before any device call. */
VPT_API int vpt_volume_components_capped(vpt_volume *src, uint32_t lo, uint32_t hi, int connectivity, uint32_t min_voxels, int merge_steps,
                                         int flatten_steps, vpt_components **out);

#ifdef __cplusplus
}
#endif
#endif /* VPT_H */
