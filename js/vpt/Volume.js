'use strict';
// src/js/Volume.js:3-127 on HIP device memory; fed by a reader (js/vpt/readers/readers.js).
const { EventTarget, CustomEvent } = require('./EventTarget.js');
const { native } = require('./native.js');

const R = require('./readers/readers.js');
const { checkConnectivity, checkRange, checkMinVoxels, checkKeep } = require('./components.js');
const { checkWindow, checkRankSet } = require('./measure.js');
const { checkSeeds, checkSteps, checkRadius, checkWithin, checkDistanceRange } = require('./distance.js');
const { checkResampleMode, checkResampleSize, isotropicShape } = require('./resample.js');
const { COMBINE_STATS, checkCombineOp, checkCombineChannel, checkCombineWeights, checkCombineMask, checkCompareRange, compareRatios } = require('./combine.js');
const { checkReconstructOp, checkGeodesicOp, checkGeodesicH, checkSourceChannel } = require('./reconstruct.js');
const { checkPolarity } = require('./watershed.js');
const { THIN_KEPT, SKELETON_INFO_FIELDS, checkThinMode, checkSkeletonRange, checkThinPasses, checkBurnWithin } = require('./skeleton.js');
const graphHost = require('./graph.js');
const surfaceHost = require('./surface.js');
const { RAWReader, GL_RED, GL_RG, GL_RGB, GL_RGBA, GL_UNSIGNED_BYTE, GL_FLOAT, GL_HALF_FLOAT, GL_BYTE } = R;

// [type, format, internalFormat, native format name, channels in the file, element kind] of the formats keyed on all three: SNORM bytes
// (RGB8_SNORM / RGBA8_SNORM keep their first two channels, as RGB8 / RGBA8 do) and the packed types (one word per texel, decoded on the device)
const SIZED = [
    [GL_BYTE, GL_RED, R.GL_R8_SNORM, 'VPT_FORMAT_R8_SNORM', 1, 'i8'],
    [GL_BYTE, GL_RG, R.GL_RG8_SNORM, 'VPT_FORMAT_RG8_SNORM', 2, 'i8'],
    [GL_BYTE, GL_RGB, R.GL_RGB8_SNORM, 'VPT_FORMAT_RG8_SNORM', 3, 'i8'],
    [GL_BYTE, GL_RGBA, R.GL_RGBA8_SNORM, 'VPT_FORMAT_RG8_SNORM', 4, 'i8'],
    [R.GL_UNSIGNED_SHORT_5_6_5, GL_RGB, R.GL_RGB565, 'VPT_FORMAT_RGB565', 1, 'packed'],
    [R.GL_UNSIGNED_SHORT_4_4_4_4, GL_RGBA, R.GL_RGBA4, 'VPT_FORMAT_RGBA4', 1, 'packed'],
    [R.GL_UNSIGNED_SHORT_5_5_5_1, GL_RGBA, R.GL_RGB5_A1, 'VPT_FORMAT_RGB5_A1', 1, 'packed'],
    [R.GL_UNSIGNED_INT_2_10_10_10_REV, GL_RGBA, R.GL_RGB10_A2, 'VPT_FORMAT_RGB10_A2', 1, 'packed'],
    [R.GL_UNSIGNED_INT_10F_11F_11F_REV, GL_RGB, R.GL_R11F_G11F_B10F, 'VPT_FORMAT_R11F_G11F_B10F', 1, 'packed'],
    [R.GL_UNSIGNED_INT_5_9_9_9_REV, GL_RGB, R.GL_RGB9_E5, 'VPT_FORMAT_RGB9_E5', 1, 'packed'],
];
// ... and those a context takes once it has enabled EXT_texture_norm16 (gl.getExtension): 16-bit channels uploaded as they are
const NORM16 = [
    [R.GL_UNSIGNED_SHORT, GL_RED, R.GL_R16_EXT, 'VPT_FORMAT_R16', 1, 'i16'],
    [R.GL_UNSIGNED_SHORT, GL_RG, R.GL_RG16_EXT, 'VPT_FORMAT_RG16', 2, 'i16'],
    [R.GL_UNSIGNED_SHORT, GL_RGB, R.GL_RGB16_EXT, 'VPT_FORMAT_RG16', 3, 'i16'],
    [R.GL_UNSIGNED_SHORT, GL_RGBA, R.GL_RGBA16_EXT, 'VPT_FORMAT_RG16', 4, 'i16'],
    [R.GL_SHORT, GL_RED, R.GL_R16_SNORM_EXT, 'VPT_FORMAT_R16_SNORM', 1, 'i16'],
    [R.GL_SHORT, GL_RG, R.GL_RG16_SNORM_EXT, 'VPT_FORMAT_RG16_SNORM', 2, 'i16'],
    [R.GL_SHORT, GL_RGB, R.GL_RGB16_SNORM_EXT, 'VPT_FORMAT_RG16_SNORM', 3, 'i16'],
    [R.GL_SHORT, GL_RGBA, R.GL_RGBA16_SNORM_EXT, 'VPT_FORMAT_RG16_SNORM', 4, 'i16'],
];

// IEEE half -> float (exact)
function halfToFloat(h) {
    const s = (h & 0x8000) ? -1 : 1, e = (h >> 10) & 31, m = h & 1023;
    if (e === 0) { return s * m * Math.pow(2, -24); }
    if (e === 31) { return m ? NaN : s * Infinity; }
    return s * (1 + m / 1024) * Math.pow(2, e - 15);
}

// (native format, channels in the file, element kind) for a manifest's (type, format, internalFormat): what a WebGL2 sampler3D can
// filter — UNSIGNED_BYTE and FLOAT / HALF_FLOAT with 1-4 channels (the shaders read .rg: further channels are dropped on upload), BYTE
// with an SNORM internal format, the packed types with the internal format each names (vpt_amd/volume.py device_format); on a context
// `gl` that has enabled EXT_texture_norm16, UNSIGNED_SHORT / SHORT with that extension's internal formats.  Anything else raises the
// reference's error (Volume.js:103).
function deviceFormat(N, modality, gl) {
    const t = modality.type, f = modality.format;
    if (t === GL_UNSIGNED_BYTE && (f === GL_RED || f === GL_RG || f === GL_RGB || f === GL_RGBA)) {
        const n = f === GL_RED ? 1 : (f === GL_RG ? 2 : (f === GL_RGB ? 3 : 4));
        return { fmt: n === 1 ? N.VPT_FORMAT_R8 : N.VPT_FORMAT_RG8, channels: n, kind: 'u8' };
    }
    if ((t === GL_FLOAT || t === GL_HALF_FLOAT) && (f === GL_RED || f === GL_RG || f === GL_RGB || f === GL_RGBA)) {
        const n = f === GL_RED ? 1 : (f === GL_RG ? 2 : (f === GL_RGB ? 3 : 4));
        return { fmt: n === 1 ? N.VPT_FORMAT_R32F : N.VPT_FORMAT_RG32F, channels: n, kind: t === GL_FLOAT ? 'f32' : 'f16' };
    }
    let sized = SIZED.find(e => e[0] === t && e[1] === f && e[2] === modality.internalFormat);
    if (!sized && gl && gl.extensionEnabled && gl.extensionEnabled('EXT_texture_norm16')) {
        sized = NORM16.find(e => e[0] === t && e[1] === f && e[2] === modality.internalFormat);
    }
    if (sized) { return { fmt: N[sized[3]], channels: sized[4], kind: sized[5] }; }
    throw new Error('Unknown volume datatype: ' + t);
}

// a block as the bytes vpt_volume_upload_block takes: (u)int8 or (u)int16 with at most two channels, float32, or packed words
function blockBytes(data, df) {
    const u8 = data instanceof Uint8Array ? data : new Uint8Array(data.buffer || data, data.byteOffset || 0, data.byteLength);
    if (df.kind === 'packed') { return u8; }                 // the words as they are
    if (df.kind === 'i16') {                                 // 16-bit channels: the first two of each texel, little-endian words as they are
        if (df.channels <= 2) { return u8; }
        const n = u8.length / (2 * df.channels), out = new Uint8Array(4 * n);
        for (let i = 0; i < n; i++) { for (let b = 0; b < 4; b++) { out[4 * i + b] = u8[2 * df.channels * i + b]; } }
        return out;
    }
    if (df.kind === 'u8' || df.kind === 'i8') {
        if (df.channels <= 2) { return u8; }
        const n = u8.length / df.channels, out = new Uint8Array(2 * n);
        for (let i = 0; i < n; i++) { out[2 * i] = u8[df.channels * i]; out[2 * i + 1] = u8[df.channels * i + 1]; }
        return out;
    }
    // float texels: float32 (half widened exactly), at most two channels (the shaders read .rg)
    let f;
    if (df.kind === 'f32') {
        f = new Float32Array(u8.buffer.slice(u8.byteOffset, u8.byteOffset + u8.byteLength));
    } else {
        const h = new Uint16Array(u8.buffer.slice(u8.byteOffset, u8.byteOffset + u8.byteLength));
        f = new Float32Array(h.length);
        for (let i = 0; i < h.length; i++) { f[i] = halfToFloat(h[i]); }
    }
    if (df.channels > 2) {
        const n = f.length / df.channels, out = new Float32Array(2 * n);
        for (let i = 0; i < n; i++) { out[2 * i] = f[df.channels * i]; out[2 * i + 1] = f[df.channels * i + 1]; }
        f = out;
    }
    return new Uint8Array(f.buffer);
}

// the VPT_FILTER_* code of a setFilter() name: 'linear', 'quasicubic' (smoothstep-weighted LINEAR cell, C1), anything else 'nearest' (:121)
function filterCode(N, filter) {
    if (filter === 'linear') { return N.VPT_FILTER_LINEAR; }
    if (filter === 'quasicubic') { return N.VPT_FILTER_QUASI_CUBIC; }
    return N.VPT_FILTER_NEAREST;
}

// the volume format behind a loaded modality, looked up like deviceFormat but with the 16-bit formats always known (a derived RG16 volume
// needs no extension), and the TypedArray of its texels: { fmt, channels (in the storage: 1 or 2), array }
function texelLayout(N, modality) {
    const m = modality;
    const sized = SIZED.find(e => e[0] === m.type && e[1] === m.format && e[2] === m.internalFormat) ||
                  NORM16.find(e => e[0] === m.type && e[1] === m.format && e[2] === m.internalFormat);
    const df = sized ? { fmt: N[sized[3]], channels: sized[4], kind: sized[5] } : deviceFormat(N, m, null);
    if (df.kind === 'packed') { return { fmt: df.fmt, channels: 2, array: Float32Array }; }      // the decoded RG32F texels
    const channels = Math.min(df.channels, 2);
    if (df.kind === 'f32' || df.kind === 'f16') { return { fmt: df.fmt, channels, array: Float32Array }; }
    if (df.kind === 'i16') { return { fmt: df.fmt, channels, array: m.type === R.GL_SHORT ? Int16Array : Uint16Array }; }
    return { fmt: df.fmt, channels, array: df.kind === 'i8' ? Int8Array : Uint8Array };
}

// VPT_GRADIENT_* of an operator name; q = floor(gain^2 16384 + 0.5) of the float32 gain must lie in [1, 4194304] (include/vpt.h)
function gradientArguments(N, operator, gain) {
    const op = operator === 'central' ? N.VPT_GRADIENT_CENTRAL : (operator === 'sobel' ? N.VPT_GRADIENT_SOBEL : null);
    if (op === null) { throw new Error(`unknown gradient operator '${operator}' ('central' or 'sobel')`); }
    const g = Math.fround(Number(gain)), q = Math.floor(g * g * 16384 + 0.5);
    if (!(q >= 1 && q <= 4194304)) { throw new Error(`gradient gain ${gain} outside [1/128, 16]`); }
    return { op, gain: g };
}

// 8 or 16 from a windowed volume's format name ('r8' | 'r16')
function windowFormatBits(format) {
    if (format === 'r8') { return 8; }
    if (format === 'r16') { return 16; }
    throw new Error(`a windowed volume is 'r8' or 'r16', not '${format}'`);
}

// (lo, hi) in code units from a full-resolution code histogram (256 or 65536 bins; signed: bin = code + 2^(B-1)): with N the sum of the bins
// and cum(k) the inclusive cumulative count, lo = the smallest code with cum >= max(1, ceil(N pLo / 100)), hi likewise for pHi, then
// hi = max(hi, lo + 1).  Integers only: a percentile is taken as the exact rational of its floating-point value (vpt_amd/window.py)
function percentileWindow(bins, pLo, pHi, signed) {
    if (bins.length !== 256 && bins.length !== 65536) { throw new Error('a code histogram has 256 or 65536 bins, not ' + bins.length); }
    if (!(pLo >= 0 && pLo <= pHi && pHi <= 100)) { throw new Error(`percentiles ${pLo}, ${pHi}: 0 <= pLo <= pHi <= 100`); }
    let total = 0;
    for (let i = 0; i < bins.length; i++) { total += bins[i]; }
    if (total === 0) { throw new Error('the histogram is empty'); }
    const need = p => {                                      // max(1, ceil(total * p / 100)), p = m / 2^k exactly
        let m = p, k = 0;
        while (!Number.isInteger(m)) { m *= 2; k++; }
        const num = BigInt(m) * BigInt(total), den = BigInt(100) * (BigInt(1) << BigInt(k));
        let q = num / den;
        if (q * den < num) { q += BigInt(1); }
        return Math.max(1, Number(q));
    };
    const code = p => {
        const want = need(p);
        let cum = 0;
        for (let i = 0; i < bins.length; i++) { cum += bins[i]; if (cum >= want) { return i - (signed ? bins.length / 2 : 0); } }
        return bins.length - 1 - (signed ? bins.length / 2 : 0);
    };
    const lo = code(pLo), hi = code(pHi);
    return [lo, Math.max(hi, lo + 1)];
}

class Volume extends EventTarget {

constructor(gl, reader, options) {
    super();
    this._gl = gl;
    this._reader = reader;
    this.metadata = null;
    this.ready = false;
    this.texture = null;
    this.modality = null;
}

destroy() {
    if (this.texture) { native().volumeDestroy(this.texture); this.texture = null; this.ready = false; }
}

async readMetadata() {
    if (!this.metadata) { this.metadata = await this._reader.readMetadata(); }
    return this.metadata;
}

async readModality(modalityName) {
    const N = native();
    this.ready = false;
    if (!this.metadata) { await this.readMetadata(); }
    const modality = this.metadata.modalities.find(m => m.name === modalityName);
    if (!modality) { throw new Error(`Modality '${modalityName}' does not exist`); }          // Volume.js:40
    this.modality = modality;
    if (this.texture) { N.volumeDestroy(this.texture); this.texture = null; }
    const df = deviceFormat(N, modality, this._gl);                                                       // Volume.js:58-60,84-105
    const { width, height, depth } = modality.dimensions;
    this.texture = N.volumeCreate(this._gl._h, width, height, depth, df.fmt);
    for (const { index, position } of modality.placements) {
        const data = await this._reader.readBlock(index);
        const d = this.metadata.blocks[index].dimensions;
        N.volumeUploadBlock(this.texture, position.x, position.y, position.z, d.width, d.height, d.depth, blockBytes(data, df));
        const progress = (index + 1) / modality.placements.length;
        this.dispatchEvent(new CustomEvent('progress', { detail: progress }));
    }
    N.volumeFinalize(this.texture);
    this.ready = true;
}

async load() { await this.readModality('default'); }

getTexture() { return this.ready ? this.texture : null; }

setFilter(filter) {
    if (!this.texture) { return; }
    const N = native();
    N.volumeSetFilter(this.texture, filterCode(N, filter));
}

// ---- extension: volume operations on the device (include/vpt.h; DESIGN.md "Gradient-magnitude channel") ----
nativeFormat() { return texelLayout(native(), this.modality).fmt; }

// texSubImage3D's inverse: the texels of a box, [depth][height][width]([2]) in a TypedArray of the volume's texel type
readBlock(x, y, z, width, height, depth) {
    const layout = texelLayout(native(), this.modality);
    const out = new layout.array(width * height * depth * layout.channels);
    native().volumeReadBlock(this.texture, x, y, z, width, height, depth, out);
    return out;
}

// Uint32Array counts: 256 bins of the value's top 8 bits (R8 / R16) or 256 x 256, bins[g * 256 + v] (RG8 / RG16)
histogram() {
    const layout = texelLayout(native(), this.modality);
    const bins = new Uint32Array(layout.channels === 2 ? 65536 : 256);
    native().volumeHistogram(this.texture, bins);
    return bins;
}

// a new, ready RG8 / RG16 volume with this volume's filter: channel 0 this (R8 / R16) volume's texels, channel 1 their gradient magnitude
// ({ operator: 'central' | 'sobel', gain }), derived on the device; this volume is not changed
deriveGradient(options) {
    options = options || {};
    const N = native();
    const a = gradientArguments(N, options.operator !== undefined ? options.operator : 'central', options.gain !== undefined ? options.gain : 1);
    const norm16 = this.nativeFormat() === N.VPT_FORMAT_R16;
    const out = new Volume(this._gl);
    out.texture = N.volumeDeriveGradient(this.texture, a.op, a.gain);
    const dimensions = Object.assign({}, this.modality.dimensions);
    out.modality = { name: this.modality.name || 'default', dimensions, transform: this.modality.transform, format: GL_RG,
        internalFormat: norm16 ? R.GL_RG16_EXT : R.GL_RG8, type: norm16 ? R.GL_UNSIGNED_SHORT : GL_UNSIGNED_BYTE,
        placements: [{ index: 0, position: { x: 0, y: 0, z: 0 } }] };
    out.metadata = { meta: Object.assign({}, (this.metadata || {}).meta), modalities: [out.modality],
        blocks: [{ url: null, format: 'raw', dimensions: Object.assign({}, dimensions) }] };
    out.ready = true;
    return out;
}

// ---- extension: the value-range window (include/vpt.h; DESIGN.md "Value-range window") ----
// a new, ready R8 / R16 volume with this volume's filter whose [0, 1] axis is the range [lo, hi] of this one-channel volume (code units for
// R8 / R16 / R8_SNORM / R16_SNORM, values for R32F): { lo, hi, format: 'r8' (default) | 'r16' }, derived on the device; this volume is not changed
window(options) {
    options = options || {};
    const N = native();
    const norm16 = windowFormatBits(options.format !== undefined ? options.format : 'r8') === 16;
    const out = new Volume(this._gl);
    out.texture = N.volumeWindow(this.texture, Number(options.lo), Number(options.hi), norm16 ? N.VPT_FORMAT_R16 : N.VPT_FORMAT_R8);
    const dimensions = Object.assign({}, this.modality.dimensions);
    out.modality = { name: this.modality.name || 'default', dimensions, transform: this.modality.transform, format: GL_RED,
        internalFormat: norm16 ? R.GL_R16_EXT : R.GL_R8, type: norm16 ? R.GL_UNSIGNED_SHORT : GL_UNSIGNED_BYTE,
        placements: [{ index: 0, position: { x: 0, y: 0, z: 0 } }] };
    out.metadata = { meta: Object.assign({}, (this.metadata || {}).meta), modalities: [out.modality],
        blocks: [{ url: null, format: 'raw', dimensions: Object.assign({}, dimensions) }] };
    out.ready = true;
    return out;
}

// [lo, hi]: the smallest and the largest code (R8 / R16 / R8_SNORM / R16_SNORM) or value (R32F, NaN texels ignored)
range() { return native().volumeRange(this.texture); }

// Uint32Array counts per code at full resolution: 256 (R8, R8_SNORM) or 65536 (R16, R16_SNORM) bins; bin = code, for SNORM code + 128 / + 32768
codeHistogram() {
    const N = native(), fmt = this.nativeFormat();
    const bins = new Uint32Array(fmt === N.VPT_FORMAT_R16 || fmt === N.VPT_FORMAT_R16_SNORM ? 65536 : 256);
    N.volumeCodeHistogram(this.texture, bins);
    return bins;
}

// [lo, hi] in code units: the pLo-th and pHi-th percentile codes of an integer volume (defaults 0.5 and 99.5)
percentileWindow(pLo, pHi) {
    const N = native(), fmt = this.nativeFormat();
    return percentileWindow(this.codeHistogram(), pLo !== undefined ? pLo : 0.5, pHi !== undefined ? pHi : 99.5,
        fmt === N.VPT_FORMAT_R8_SNORM || fmt === N.VPT_FORMAT_R16_SNORM);
}

// ---- extension: the next coarser level and binomial smoothing (include/vpt.h; DESIGN.md "Binomial smoothing and 2x reduction") ----
// the ready Volume around a derived native volume of this volume's format with the given dimensions
_sameFormat(texture, dimensions) {
    return derivedVolume(new Volume(this._gl), texture, this.modality, (this.metadata || {}).meta, dimensions);
}

// a new, ready volume in this volume's format and with its filter, `levels` (an integer >= 1, default 1) times reduced to ceil(n / 2) texels
// per axis, every texel the rounded mean of its 2 x 2 x 2 cell, derived on the device; stops early once every axis is 1; packed formats are
// refused; this volume is not changed
reduce(levels) {
    levels = checkLevels(levels !== undefined ? levels : 1);
    const N = native();
    let source = this, d = this.modality.dimensions;
    for (;;) {
        let texture;
        try { texture = N.volumeReduce(source.texture); } finally { if (source !== this) { source.destroy(); } }   // the level in between
        d = { width: (d.width + 1) >> 1, height: (d.height + 1) >> 1, depth: (d.depth + 1) >> 1 };
        source = this._sameFormat(texture, d);
        levels--;
        if (levels === 0 || Math.max(d.width, d.height, d.depth) === 1) { return source; }
    }
}

// a new, ready R8 / R16 volume of this (R8 / R16) volume's size and with its filter: `passes` (1 .. 8, default 1) applications of the binomial
// 3 x 3 x 3 kernel, derived on the device; this volume is not changed
smooth(passes) {
    passes = checkPasses(passes !== undefined ? passes : 1);
    return this._sameFormat(native().volumeSmooth(this.texture, passes), this.modality.dimensions);
}

// ---- extension: median and grey-level morphology (include/vpt.h; DESIGN.md "Median and morphology") ----
// a new, ready R8 / R16 volume of this (R8 / R16) volume's size and with its filter: `passes` (1 .. 8, default 1) applications of the rank
// operator `op` ('median' | 'erode' | 'dilate' | 'open' | 'close') over the clamped 3 x 3 x 3 box, derived on the device; this volume is not changed
rank(op, passes) {
    const code = rankOperatorCode(op);
    passes = checkRankPasses(passes !== undefined ? passes : 1);
    return this._sameFormat(native().volumeRank(this.texture, code, passes), this.modality.dimensions);
}
median(passes) { return this.rank('median', passes); }
erode(passes) { return this.rank('erode', passes); }
dilate(passes) { return this.rank('dilate', passes); }
open(passes) { return this.rank('open', passes); }
close(passes) { return this.rank('close', passes); }

// ---- extension: resampling to any grid size (include/vpt.h; DESIGN.md "Resampling") ----
// a new, ready volume in this volume's format and with its filter on a grid of width x height x depth texels (each 1 .. 4096) that fills the
// same cube: mode 'filtered' (default; R8, RG8, R16, RG16) interpolates linearly along an axis that grows and averages areas along one that
// shrinks, in integers with one rounding; 'nearest' (every unpacked format) copies the texel under each result texel's centre: the mode for
// labels and masks; derived on the device; this volume is not changed
resample(width, height, depth, mode) {
    const code = checkResampleMode(mode !== undefined ? mode : 'filtered');
    checkResampleSize(width, height, depth);
    return this._sameFormat(native().volumeResample(this.texture, width, height, depth, code), { width, height, depth });
}
// resample() to cubic voxels of edge `pitch` (default: the smallest spacing) from this volume's voxel spacing = [sx, sy, sz]
isotropic(spacing, pitch, mode) {
    const d = this.modality.dimensions, n = isotropicShape([d.width, d.height, d.depth], spacing, pitch);
    return this.resample(n[0], n[1], n[2], mode);
}

// ---- extension: two volumes combined or compared texel by texel (include/vpt.h; DESIGN.md "Combining two volumes") ----
// the arguments of native().volumeCombine behind combine(other, op, options), checked as combineTexels of combine.js checks them
_combineArguments(other, op, options) {
    options = options || {};
    const N = native(), code = checkCombineOp(op);
    if (!(other instanceof Volume) || !other.texture || !this.texture) { throw new Error('combine takes two ready volumes'); }
    const unknown = Object.keys(options).filter(k => ['channel', 'lo', 'hi', 'fill', 'wa', 'wb', 'offset'].indexOf(k) < 0);
    if (unknown.length) { throw new Error('combine takes channel, lo, hi, fill (mask) and wa, wb, offset (blend), not ' + unknown.sort().join(', ')); }
    const layout = texelLayout(N, other.modality);
    const channel = checkCombineChannel(options.channel !== undefined ? options.channel : 0, layout.channels);
    const largest = this.nativeFormat() === N.VPT_FORMAT_R16 || this.nativeFormat() === N.VPT_FORMAT_RG16 ? 65535 : 255;
    let mask = [0, 0, 0], blend = [0, 0, 0];
    if (op === 'mask') {
        const largestB = layout.array.BYTES_PER_ELEMENT === 2 ? 65535 : 255;
        mask = checkCombineMask(options.lo !== undefined ? options.lo : 0, options.hi !== undefined && options.hi !== null ? options.hi : largestB,
            options.fill !== undefined ? options.fill : 0, largestB, largest);
    } else if (op === 'blend') {
        blend = checkCombineWeights(options.wa !== undefined ? options.wa : 256, options.wb !== undefined ? options.wb : 0, options.offset);
    }
    return [this.texture, other.texture, code, channel, mask[0], mask[1], mask[2], blend[0], blend[1], blend[2]];
}
_combined(texture, op) {
    const out = this._sameFormat(texture, this.modality.dimensions);
    if (op === 'pair') {
        const norm16 = this.nativeFormat() === native().VPT_FORMAT_R16;
        Object.assign(out.modality, { format: GL_RG, internalFormat: norm16 ? R.GL_RG16_EXT : R.GL_RG8, type: norm16 ? R.GL_UNSIGNED_SHORT : GL_UNSIGNED_BYTE });
    }
    return out;
}
// a new, ready volume on this (R8 / R16) volume's context and with its filter: this volume's texels A combined with the texels B of channel
// options.channel (default 0) of `other` (R8, RG8, R16, RG16; same size; may be this volume) by `op`: 'mask' ({ lo, hi, fill }), 'min', 'max',
// 'absdiff', 'blend' ({ wa, wb, offset }) in this volume's format, or 'pair', the RG8 / RG16 volume (A, B); derived on the device; neither
// volume is changed
combine(other, op, options) {
    const a = this._combineArguments(other, op, options);
    return this._combined(native().volumeCombine.apply(null, a), op);
}
// (for measurements) [the volume combine() gives, the milliseconds of the combining pass alone, the stream drained around it]
combineTimed(other, op, options) {
    const a = this._combineArguments(other, op, options);
    const r = native().volumeCombineTimed.apply(null, a);
    return [this._combined(r[0], op), r[1]];
}
// this volume's codes where lo <= B <= hi, `fill` (default 0) elsewhere; `other` may be 8- or 16-bit whatever this volume is
mask(other, lo, hi, fill, channel) { return this.combine(other, 'mask', { lo, hi, fill: fill !== undefined ? fill : 0, channel: channel !== undefined ? channel : 0 }); }
minimum(other, channel) { return this.combine(other, 'min', { channel: channel !== undefined ? channel : 0 }); }
maximum(other, channel) { return this.combine(other, 'max', { channel: channel !== undefined ? channel : 0 }); }
absdiff(other, channel) { return this.combine(other, 'absdiff', { channel: channel !== undefined ? channel : 0 }); }
// clamp(((wa A + wb B + 128) >> 8) + offset, 0, M): weights in 1/256 units; (256, 256) adds, (256, -256) subtracts, (128, 128) averages,
// (-256, 0, M) inverts, (512, -256) against smooth() is unsharp masking
blend(other, wa, wb, offset, channel) { return this.combine(other, 'blend', { wa, wb, offset: offset !== undefined ? offset : 0, channel: channel !== undefined ? channel : 0 }); }
// the RG8 / RG16 volume (A, B): `other` becomes the second axis of the 2-D transfer function
pair(other, channel) { return this.combine(other, 'pair', { channel: channel !== undefined ? channel : 0 }); }
// { voxels, differing, maxAbs, sumAbs, sumSq, inA, inB, both }: exact BigInts (sumSq can pass 2^53) over this (R8 / R16) volume's codes A and
// the codes B of channel `channel` of `other` (mixed widths are taken), counted on the device; inA counts aRange[0] <= A <= aRange[1] (null:
// every code), inB likewise, both their intersection; plus dice, jaccard, mse, psnr as Numbers, null where a denominator is 0.  More than
// 2^32 - 1 voxels throw (VPT_ERR_UNSUPPORTED)
compare(other, aRange, bRange, channel) {
    const N = native();
    if (!(other instanceof Volume) || !other.texture || !this.texture) { throw new Error('compare takes two ready volumes'); }
    const layout = texelLayout(N, other.modality);
    channel = checkCombineChannel(channel !== undefined ? channel : 0, layout.channels);
    const largestA = this.nativeFormat() === N.VPT_FORMAT_R16 || this.nativeFormat() === N.VPT_FORMAT_RG16 ? 65535 : 255;
    const largestB = layout.array.BYTES_PER_ELEMENT === 2 ? 65535 : 255;
    const ra = checkCompareRange(aRange, largestA, 'aRange'), rb = checkCompareRange(bRange, largestB, 'bRange');
    const halves = N.volumeCompare(this.texture, other.texture, channel, ra[0], ra[1], rb[0], rb[1]);      // (low, high) 32-bit halves of the eight counts
    const stats = {};
    COMBINE_STATS.forEach((name, k) => { stats[name] = (BigInt(halves[2 * k + 1]) << 32n) | BigInt(halves[2 * k]); });
    return Object.assign(stats, compareRatios(stats, Math.max(largestA, largestB)));
}

// ---- extension: morphological reconstruction and the geodesic operations (include/vpt.h; DESIGN.md "Geodesic reconstruction") ----
// the ready one-channel R8 / R16 Volume around a native volume derived from this (R8, RG8, R16 or RG16) one
_oneChannel(texture) {
    const N = native(), norm16 = this.nativeFormat() === N.VPT_FORMAT_R16 || this.nativeFormat() === N.VPT_FORMAT_RG16;
    const modality = Object.assign({}, this.modality, { format: GL_RED, internalFormat: norm16 ? R.GL_R16_EXT : R.GL_R8,
        type: norm16 ? R.GL_UNSIGNED_SHORT : GL_UNSIGNED_BYTE });
    return derivedVolume(new Volume(this._gl), texture, modality, (this.metadata || {}).meta, this.modality.dimensions);
}
// the arguments of native().volumeReconstruct behind reconstruct(mask, options)
_reconstructArguments(mask, options) {
    options = options || {};
    const N = native(), code = checkReconstructOp(options.op !== undefined ? options.op : 'dilation');
    const connectivity = checkConnectivity(options.connectivity !== undefined ? options.connectivity : 6);
    if (!(mask instanceof Volume) || !mask.texture || !this.texture) { throw new Error('reconstruct takes two ready volumes'); }
    const unknown = Object.keys(options).filter(k => ['op', 'connectivity', 'channel', 'maskChannel', 'tileRounds'].indexOf(k) < 0);
    if (unknown.length) { throw new Error('reconstruct takes op, connectivity, channel and maskChannel, not ' + unknown.sort().join(', ')); }
    const channel = checkSourceChannel(options.channel !== undefined ? options.channel : 0, texelLayout(N, this.modality).channels);
    const maskChannel = checkSourceChannel(options.maskChannel !== undefined ? options.maskChannel : 0, texelLayout(N, mask.modality).channels);
    return [this.texture, channel, mask.texture, maskChannel, code, connectivity];
}
// a new, ready one-channel R8 / R16 volume on this volume's context and with its filter: the morphological reconstruction, by options.op
// 'dilation' (default) or 'erosion', of channel options.channel of this volume (the marker) under channel options.maskChannel of `mask` (R8,
// RG8, R16, RG16 either; same size and channel width; may be this volume) with options.connectivity 6 (default), 18 or 26, propagated on
// the device; neither volume is changed
reconstruct(mask, options) {
    return this._oneChannel(native().volumeReconstruct.apply(null, this._reconstructArguments(mask, options)));
}
// (for measurements) [the volume reconstruct() gives, { ms, launches, tileRuns }]: the milliseconds of the call up to the result's finalize,
// the stream drained either side, the launches of the propagation kernel and the tiles that worked, summed over them; options.tileRounds
// (for tests): the rounds a tile may make per launch (no tileRuns then)
reconstructTimed(mask, options) {
    const rounds = options && options.tileRounds !== undefined ? options.tileRounds : 0;
    if (!Number.isInteger(rounds) || (options && options.tileRounds !== undefined && rounds < 1)) { throw new Error('tileRounds is an integer >= 1'); }
    const r = native().volumeReconstructTimed.apply(null, this._reconstructArguments(mask, options).concat([rounds]));
    return [this._oneChannel(r[0]), { ms: r[1], launches: r[2], tileRuns: r[3] }];
}
_geodesicArguments(op, h, connectivity, channel) {
    const N = native(), code = checkGeodesicOp(op);
    connectivity = checkConnectivity(connectivity !== undefined ? connectivity : 6);
    if (!this.texture) { throw new Error('a geodesic operation takes a ready volume'); }
    const layout = texelLayout(N, this.modality);
    channel = checkSourceChannel(channel !== undefined ? channel : 0, layout.channels);
    h = checkGeodesicH(op, h !== undefined ? h : 0, layout.array.BYTES_PER_ELEMENT === 2 ? 65535 : 255);
    return [this.texture, channel, code, h, connectivity];
}
// a new, ready one-channel R8 / R16 volume on this (R8, RG8, R16 or RG16) volume's context and with its filter: the geodesic operation `op`
// ('fill_holes' | 'clear_border' | 'hmax' | 'hmin' | 'dome' | 'maxima' | 'minima'; h for 'hmax', 'hmin' and 'dome') of channel `channel`, on the
// device; this volume is not changed
geodesic(op, h, connectivity, channel) {
    return this._oneChannel(native().volumeGeodesic.apply(null, this._geodesicArguments(op, h, connectivity, channel)));
}
// (for measurements) [the volume geodesic() gives, { ms, launches, tileRuns }] as reconstructTimed()
geodesicTimed(op, h, connectivity, channel) {
    const r = native().volumeGeodesicTimed.apply(null, this._geodesicArguments(op, h, connectivity, channel));
    return [this._oneChannel(r[0]), { ms: r[1], launches: r[2], tileRuns: r[3] }];
}
// every regional minimum not connected to the volume's border raised to its rim
fillHoles(connectivity, channel) { return this.geodesic('fill_holes', 0, connectivity, channel); }
fillHolesTimed(connectivity, channel) { return this.geodesicTimed('fill_holes', 0, connectivity, channel); }
// what is connected to the volume's border removed, grey values kept
clearBorder(connectivity, channel) { return this.geodesic('clear_border', 0, connectivity, channel); }
clearBorderTimed(connectivity, channel) { return this.geodesicTimed('clear_border', 0, connectivity, channel); }
// maxima / minima shallower than h suppressed; dome: this - hmax(h)
hmax(h, connectivity, channel) { return this.geodesic('hmax', h, connectivity, channel); }
hmaxTimed(h, connectivity, channel) { return this.geodesicTimed('hmax', h, connectivity, channel); }
hmin(h, connectivity, channel) { return this.geodesic('hmin', h, connectivity, channel); }
hminTimed(h, connectivity, channel) { return this.geodesicTimed('hmin', h, connectivity, channel); }
dome(h, connectivity, channel) { return this.geodesic('dome', h, connectivity, channel); }
domeTimed(h, connectivity, channel) { return this.geodesicTimed('dome', h, connectivity, channel); }
// M on the plateaus without a higher (lower) neighbour, 0 elsewhere; a voxel of code 0 (M) is never a maximum (minimum)
regionalMaxima(connectivity, channel) { return this.geodesic('maxima', 0, connectivity, channel); }
regionalMaximaTimed(connectivity, channel) { return this.geodesicTimed('maxima', 0, connectivity, channel); }
regionalMinima(connectivity, channel) { return this.geodesic('minima', 0, connectivity, channel); }
regionalMinimaTimed(connectivity, channel) { return this.geodesicTimed('minima', 0, connectivity, channel); }

// ---- extension: watershed by steepest descent on a lower-completed relief (include/vpt.h; DESIGN.md "Watershed") ----
// the arguments of native().volumeWatershed behind watershed(lo, hi, options), and the volume the handle speaks of
_watershedArguments(lo, hi, options, timed) {
    options = options || {};
    const N = native();
    if (!this.texture) { throw new Error('a watershed takes a ready volume'); }
    const known = ['polarity', 'connectivity', 'minVoxels', 'channel', 'texels'].concat(timed ? ['caps'] : []);      // caps: the timed form's, for tests
    const unknown = Object.keys(options).filter(k => known.indexOf(k) < 0);
    if (unknown.length) { throw new Error('watershed takes polarity, connectivity, minVoxels, channel and texels, not ' + unknown.sort().join(', ')); }
    const layout = texelLayout(N, this.modality), norm16 = layout.array.BYTES_PER_ELEMENT === 2;
    const channel = checkSourceChannel(options.channel !== undefined ? options.channel : 0, layout.channels);
    checkRange(lo, hi, norm16 ? 65535 : 255);
    const polarity = checkPolarity(options.polarity !== undefined ? options.polarity : 'minima');
    const connectivity = checkConnectivity(options.connectivity !== undefined ? options.connectivity : 6);
    const minVoxels = checkMinVoxels(options.minVoxels !== undefined ? options.minVoxels : 1);
    const texels = options.texels !== undefined ? options.texels : null;
    if (texels !== null && (!(texels instanceof Volume) || !texels.texture)) { throw new Error('watershed takes a ready volume as texels'); }
    // the handle speaks of the volume whose texels it holds: `texels`, or the chosen channel of this one
    let source = texels !== null ? texels : this;
    if (texels === null && layout.channels === 2) {
        const modality = Object.assign({}, this.modality, { format: GL_RED, internalFormat: norm16 ? R.GL_R16_EXT : R.GL_R8,
            type: norm16 ? R.GL_UNSIGNED_SHORT : GL_UNSIGNED_BYTE });
        source = { _gl: this._gl, modality, metadata: this.metadata, nativeFormat: () => (norm16 ? N.VPT_FORMAT_R16 : N.VPT_FORMAT_R8) };
    }
    return { source, args: [this.texture, channel, texels !== null ? texels.texture : null, lo, hi, polarity, connectivity, minVoxels] };
}
// the basins of channel options.channel (0) of this (R8, RG8, R16 or RG16) volume, the relief, over the domain of the codes lo .. hi, as a
// Components object: the watershed by steepest descent on the lower completion, flooded from the options.polarity 'minima' (default) or
// 'maxima' (a depth channel), with options.connectivity 6 (default), 18 or 26, basins smaller than options.minVoxels (1) dropped, on the
// device (js/vpt/watershed.js states the contract).  options.texels (an R8 / R16 volume of this size and channel width; default: the relief's
// channel) is what keep, keepSet and label emit.  Neither volume is changed; both may be destroyed
watershed(lo, hi, options) {
    const w = this._watershedArguments(lo, hi, options, false);
    return new Components(w.source, native().volumeWatershed.apply(null, w.args));
}
// (for measurements) [the basins watershed() gives, { ms: { classify, plateau, links }, plateauLaunches }]; the common tail is the basins'
// profile().  options.caps (for tests): [mergeSteps, flattenSteps, tileRounds] of vpt_volume_watershed_capped
watershedTimed(lo, hi, options) {
    const w = this._watershedArguments(lo, hi, options, true), caps = options && options.caps !== undefined ? options.caps : [0, 0, 0];
    if (!Array.isArray(caps) || caps.length !== 3 || !caps.every(Number.isInteger)) { throw new Error('caps are [mergeSteps, flattenSteps, tileRounds]'); }
    const r = native().volumeWatershedTimed.apply(null, w.args.concat(caps));
    return [new Components(w.source, r[0]), { ms: { classify: r[1], plateau: r[2], links: r[3] }, plateauLaunches: r[4] }];
}
_split(lo, hi, options, timed) {
    options = options || {};
    const unknown = Object.keys(options).filter(k => ['h', 'steps', 'connectivity', 'minVoxels'].indexOf(k) < 0);
    if (unknown.length) { throw new Error('split takes h, steps, connectivity and minVoxels, not ' + unknown.sort().join(', ')); }
    const norm16 = this.nativeFormat() === native().VPT_FORMAT_R16;
    const h = options.h !== undefined ? options.h : 2, steps = options.steps !== undefined ? options.steps : 4;
    const connectivity = options.connectivity !== undefined ? options.connectivity : 26;
    const d = this.distance(lo, hi, 'rest');
    let depth, flattened;
    try { depth = d.channel(steps); } finally { d.destroy(); }
    try { flattened = depth.hmax(h, connectivity, 1); } finally { depth.destroy(); }
    try {
        const w = { polarity: 'maxima', connectivity, minVoxels: options.minVoxels !== undefined ? options.minVoxels : 1, texels: this };
        return timed ? flattened.watershedTimed(1, norm16 ? 65535 : 255, w) : flattened.watershed(1, norm16 ? 65535 : 255, w);
    } finally { flattened.destroy(); }
}
// the structures of the codes lo .. hi of this (R8 / R16) volume with touching ones split, as a Components object whose emitters speak of
// this volume: distance(lo, hi, 'rest') -> channel(steps) -> hmax(h, connectivity, 1) -> watershed(1, M, { polarity: 'maxima', connectivity,
// minVoxels, texels: this }), all on the device; options = { h: 2, steps: 4, connectivity: 26, minVoxels: 1 }.  The intermediates are destroyed
split(lo, hi, options) { return this._split(lo, hi, options, false); }
// (for measurements) [the basins split() gives, what watershedTimed() reports of its watershed step]
splitTimed(lo, hi, options) { return this._split(lo, hi, options, true); }

// ---- extension: connected components of a value range (include/vpt.h; DESIGN.md "Connected components") ----
// the connected components of the codes lo .. hi of this (R8 / R16) volume as a Components object, labelled on the device: connectivity 6
// (default), 18 or 26; minVoxels (default 1): smaller components are dropped.  The object owns what it needs; this volume is not changed
components(lo, hi, connectivity, minVoxels) {
    const N = native(), norm16 = this.nativeFormat() === N.VPT_FORMAT_R16;
    checkRange(lo, hi, norm16 ? 65535 : 255);
    connectivity = checkConnectivity(connectivity !== undefined ? connectivity : 6);
    minVoxels = checkMinVoxels(minVoxels !== undefined ? minVoxels : 1);
    return new Components(this, N.volumeComponents(this.texture, lo, hi, connectivity, minVoxels));
}
// only the n (default 1) largest components of the codes lo .. hi keep their codes; 0 elsewhere
keepLargest(lo, hi, n, connectivity) {
    const c = this.components(lo, hi, connectivity);
    try { return c.keep(1, n !== undefined ? n : 1); } finally { c.destroy(); }
}
// the components of the codes lo .. hi with at least minVoxels voxels keep their codes; 0 elsewhere
removeIslands(lo, hi, minVoxels, connectivity) {
    const c = this.components(lo, hi, connectivity, minVoxels);
    try { return c.keep(1, null); } finally { c.destroy(); }
}

// ---- extension: exact Euclidean distance transform of a value range (include/vpt.h; DESIGN.md "Distance transform") ----
// the squared Euclidean distance of every voxel of this (R8 / R16) volume to the nearest voxel whose code is (seeds 'range', the default) or
// is not (seeds 'rest') in lo .. hi, as a Distance object, transformed on the device.  The object owns what it needs; this volume is not changed
distance(lo, hi, seeds) {
    const N = native(), norm16 = this.nativeFormat() === N.VPT_FORMAT_R16;
    checkDistanceRange(lo, hi, norm16 ? 65535 : 255);
    return new Distance(this, N.volumeDistance(this.texture, lo, hi, checkSeeds(seeds !== undefined ? seeds : 'range')));
}
// the codes within `radius` voxels of the codes lo .. hi keep their codes; 0 elsewhere
margin(lo, hi, radius) {
    const r2 = checkRadius(radius), d = this.distance(lo, hi, 'range');
    try { return d.within(0, r2); } finally { d.destroy(); }
}
// the codes lo .. hi eroded by the Euclidean ball of `radius` voxels keep their codes; 0 elsewhere
core(lo, hi, radius) {
    const r2 = checkRadius(radius), d = this.distance(lo, hi, 'rest');
    try { return d.within(r2 + 1, null); } finally { d.destroy(); }
}

// ---- extension: local thickness, the largest inscribed ball (include/vpt.h; DESIGN.md "Local thickness") ----
_thickness(lo, hi, seeds, emit) {
    const d = this.distance(lo, hi, seeds);
    let t;
    try { t = d.thickness(); } finally { d.destroy(); }
    try { return emit(t); } finally { t.destroy(); }
}
// a new, ready RG8 / RG16 volume (code, local thickness): the second channel is, in `steps` (default 2: the diameter in voxels) rows a voxel,
// the radius of the largest ball that fits inside the structure of the codes lo .. hi (seeds 'rest', the default; 'range': inside its
// complement) and holds the voxel: distance -> thickness -> channel(steps) on the device.  A valid `values` of Components.measure
thickness(lo, hi, steps, seeds) {
    steps = checkSteps(steps !== undefined ? steps : 2);
    return this._thickness(lo, hi, seeds !== undefined ? seeds : 'rest', (t) => t.channel(steps));
}
// the codes lo .. hi opened by the Euclidean ball of `radius` voxels keep their codes (the parts some inscribed ball of a radius above
// `radius` covers); `fill` (default 0) elsewhere: the counterpart of core that gives the peeled rim back
openBall(lo, hi, radius, fill) {
    const r2 = checkRadius(radius);
    return this._thickness(lo, hi, 'rest', (t) => t.within(r2 + 1, null, fill));
}

// ---- extension: curve skeleton and topological kernel by thinning (include/vpt.h; DESIGN.md "Skeleton") ----
// the burn passes of thinning the codes lo .. hi of this (R8 / R16) volume, as a Skeleton object, thinned on the device: mode 'kernel'
// shrinks every structure to its topological kernel, 'ends' (the default) keeps curve ends (the centreline), 'isthmus' keeps the voxels that
// once held two parts together; passes caps the passes (default 0: to the fixed point).  The object owns what it needs; this volume is not
// changed.  flags (for tests): those of vpt_volume_skeleton_capped (1: no tile cull)
skeleton(lo, hi, mode, passes, flags) {
    const N = native(), norm16 = this.nativeFormat() === N.VPT_FORMAT_R16;
    checkSkeletonRange(lo, hi, norm16 ? 65535 : 255);
    const code = checkThinMode(mode !== undefined ? mode : 'ends');
    passes = checkThinPasses(passes !== undefined ? passes : 0);
    return new Skeleton(this, N.volumeSkeleton(this.texture, lo, hi, code, passes, flags !== undefined && flags !== null ? flags : -1));
}
// the voxels of the codes lo .. hi that survive the thinning (mode default 'ends') keep their codes; 0 elsewhere
// with prune (a length in the default step weights 10 / 14 / 17), up to pruneRounds (default 1) times: the skeleton's graph, its spurs within
// prune dropped (Graph.prune), the rest thinned again; a round that drops nothing ends it.  The pruned volume is filled with a code outside
// lo .. hi (0 when lo > 0, otherwise hi + 1), so a range that covers every code is refused with prune set
centreline(lo, hi, mode, prune, pruneRounds) {
    if (prune === undefined || prune === null) {
        const k = this.skeleton(lo, hi, mode);
        try { return k.volume(); } finally { k.destroy(); }
    }
    const norm16 = this.nativeFormat() === native().VPT_FORMAT_R16;
    checkSkeletonRange(lo, hi, norm16 ? 65535 : 255);
    pruneRounds = pruneRounds !== undefined && pruneRounds !== null ? pruneRounds : 1;
    if (!Number.isInteger(prune) || prune < 0) { throw new Error('prune is a non-negative integer, not ' + JSON.stringify(prune)); }
    if (!Number.isInteger(pruneRounds) || pruneRounds < 1 || pruneRounds > 65535) { throw new Error('pruneRounds is an integer in 1 .. 65535, not ' + JSON.stringify(pruneRounds)); }
    if (lo === 0 && hi >= (norm16 ? 65535 : 255)) { throw new Error(`centreline with prune: the range [${lo}, ${hi}] covers every code, none is left to fill with`); }
    const fill = lo > 0 ? 0 : hi + 1;
    let k = this.skeleton(lo, hi, mode);
    try {
        for (let round = 0; round < pruneRounds; round++) {
            const g = k.graph();
            let pruned;
            try {
                if (!graphHost.graphDropped(g.branchRecords(), prune).some(Boolean)) { break; }
                pruned = g.prune(prune, undefined, false, fill);
            } finally { g.destroy(); }
            let again;
            try { again = pruned.skeleton(lo, hi, mode); } finally { pruned.destroy(); }
            k.destroy();
            k = again;
        }
        return k.volume();
    } finally { k.destroy(); }
}

// ---- extension: the graph of a voxel set: branches, nodes, step counts, spur pruning (include/vpt.h; DESIGN.md "Skeleton graph") ----
// the graph of the voxels of the codes lo .. hi of this (R8 / R16) volume as a Graph object, built on the device (js/vpt/graph.js states the
// contract): meant for a thinned set (centreline), defined for any.  The object owns what it needs; this volume is not changed
graph(lo, hi) {
    const N = native(), norm16 = this.nativeFormat() === N.VPT_FORMAT_R16;
    graphHost.checkGraphRange(lo, hi, norm16 ? 65535 : 255);
    return new Graph(this, N.volumeGraph(this.texture, lo, hi));
}

// ---- extension: isosurface mesh by naive surface nets (include/vpt.h; DESIGN.md "Surface") ----
// the surface at code level - 1/2 of channel `channel` (default 0) of this (R8, RG8, R16 or RG16) volume as a Surface object: one vertex per
// cell the surface crosses, one quad per grid edge it crosses, extracted on the device (js/vpt/surface.js states the contract).  The
// object owns what it holds; this volume is not changed.  scanWords (for tests): the words per block of the prefix sums
surface(level, channel, scanWords) {
    const N = native(), layout = texelLayout(N, this.modality);
    const norm16 = [N.VPT_FORMAT_R16, N.VPT_FORMAT_RG16, N.VPT_FORMAT_R16_SNORM, N.VPT_FORMAT_RG16_SNORM].includes(layout.fmt);
    channel = surfaceHost.checkSurfaceChannel(channel !== undefined ? channel : 0, layout.channels);
    surfaceHost.checkSurfaceLevel(level, norm16 ? 65535 : 255);
    return new Surface(N.volumeSurface(this.texture, channel, level, scanWords !== undefined && scanWords !== null ? scanWords : -1));
}

}

// the ready Volume `out` around a derived native volume: `modality` with the given dimensions in one block, and a copy of `meta`
function derivedVolume(out, texture, modality, meta, dimensions) {
    out.texture = texture;
    out.modality = Object.assign({}, modality, { dimensions: Object.assign({}, dimensions),
        placements: [{ index: 0, position: { x: 0, y: 0, z: 0 } }] });
    out.metadata = { meta: Object.assign({}, meta), modalities: [out.modality],
        blocks: [{ url: null, format: 'raw', dimensions: Object.assign({}, dimensions) }] };
    out.ready = true;
    return out;
}

// What Distance and Components share: the native handle of one Uint32 per voxel over a snapshot of an R8 / R16 volume, the box read-back of
// those values and the description of the volumes derived from them.  `noun`: of the message thrown once destroyed; `destroy`, `read`: the
// names of the subclass's native functions.
class VoxelField {

constructor(source, handle, noun, destroy, read) {
    this._h = handle;
    this._noun = noun; this._destroy = destroy; this._read = read;
    this._gl = source._gl;
    this._norm16 = source.nativeFormat() === native().VPT_FORMAT_R16;
    this._dimensions = Object.assign({}, source.modality.dimensions);
    this._modality = Object.assign({}, source.modality);       // what a derived volume's description is made from (derivedVolume)
    this._meta = Object.assign({}, (source.metadata || {}).meta);
}

_handle() {
    if (!this._h) { throw new Error('the ' + this._noun + ' have been destroyed'); }
    return this._h;
}

destroy() {
    if (this._h) { native()[this._destroy](this._h); this._h = null; }
}

// Uint32Array [depth][height][width]: the values of a box of voxels (default: the whole volume)
_values(x, y, z, width, height, depth) {
    const d = this._dimensions;
    x = x || 0; y = y || 0; z = z || 0;
    width = width !== undefined ? width : d.width - x; height = height !== undefined ? height : d.height - y; depth = depth !== undefined ? depth : d.depth - z;
    const out = new Uint32Array(width * height * depth);
    native()[this._read](this._handle(), x, y, z, width, height, depth, out);
    return out;
}

// the ready Volume around a native volume derived from the field: of the source's format, or (pair) RG8 / RG16
_derived(texture, pair) {
    const out = derivedVolume(new Volume(this._gl), texture, this._modality, this._meta, this._dimensions);
    if (pair) {
        Object.assign(out.modality, { format: GL_RG, internalFormat: this._norm16 ? R.GL_RG16_EXT : R.GL_RG8,
            type: this._norm16 ? R.GL_UNSIGNED_SHORT : GL_UNSIGNED_BYTE });
    }
    return out;
}

}

// The burn passes of a thinning of a value range of a volume (Volume.skeleton): one Uint32 per voxel on the device, 0 outside the range, k for
// a voxel deleted in pass k, THIN_KEPT for a voxel that survived.  Thin once, select several times.  Outlives the volume it was made from;
// destroy() (or close()) frees the device memory.
class Skeleton extends VoxelField {

constructor(source, handle) { super(source, handle, 'burn passes', 'skeletonDestroy', 'skeletonBurn'); }

// { object_voxels, kept_voxels, passes, converged, isolated, ends, regular, junctions }: the last four count the kept voxels with 0, 1, 2
// and >= 3 kept 26-neighbours
get info() {
    const i = native().skeletonInfo(this._handle()), out = {};
    SKELETON_INFO_FIELDS.forEach((f, k) => { out[f] = i[k]; });
    return out;
}

// Uint32Array [depth][height][width]: the burn passes of a box of voxels (default: the whole volume)
burn(x, y, z, width, height, depth) { return this._values(x, y, z, width, height, depth); }

// a new, ready volume of the source's size, format and filter: the source's code where kLo <= burn pass <= kHi (defaults THIN_KEPT and
// 0xFFFFFFFF), `fill` (default 0) elsewhere; within(k) is the object after k - 1 passes
within(kLo, kHi, fill) {
    const k = checkBurnWithin(kLo !== undefined ? kLo : THIN_KEPT, kHi, fill !== undefined ? fill : 0, this._norm16 ? 65535 : 255);
    return this._derived(native().skeletonWithin(this._handle(), k[0], k[1], k[2]));
}

// the skeleton as a volume: within(THIN_KEPT, THIN_KEPT, 0)
volume() { return this.within(THIN_KEPT, THIN_KEPT, 0); }

// (for measurements) { ms: { seed, border, steps, census }, launches, tiles }
profile() {
    const r = native().skeletonProfile(this._handle());
    return { ms: { seed: r[0], border: r[1], steps: r[2], census: r[3] }, launches: r[4], tiles: r[5] };
}

// the graph of the kept voxels as a Graph object, built on the device; its emitters and its branches / nodes speak in the codes of this
// skeleton's source.  This object is not changed
graph() { return new Graph(fieldSource(this), native().skeletonGraph(this._handle())); }

close() { this.destroy(); }

}

// what VoxelField reads of its source, for a field made of another field: the description of that field's source
function fieldSource(field) {
    const N = native();
    return { _gl: field._gl, nativeFormat: () => (field._norm16 ? N.VPT_FORMAT_R16 : N.VPT_FORMAT_R8), modality: Object.assign({}, field._modality),
        metadata: { meta: Object.assign({}, field._meta) } };
}

// The graph of a set of voxels (Volume.graph, Skeleton.graph): the class of every voxel, the branches and the nodes as two labellings and one
// record per branch and node, on the device.  Build once; list, measure, prune and colour several times.  Outlives what it was made from;
// destroy() (or close()) frees the device memory (branches and nodes once taken are the caller's).
class Graph extends VoxelField {

constructor(source, handle) {
    super(source, handle, 'graph', 'graphDestroy', null);
    this._branches = null; this._nodes = null;
}

// { kept_voxels, node_voxels, branches, nodes, isolated, segments, spurs, links, loops, cycles, steps_face, steps_edge, steps_corner, attachments }
get info() {
    const i = native().graphInfo(this._handle()), out = {};
    graphHost.GRAPH_INFO_FIELDS.forEach((f, k) => { out[f] = i[k]; });
    return out;
}

// the branches / the nodes as a Components object (made at the first use; the caller destroys it): ranks are branch / node ranks, texels the
// source's codes, so measure, keepSet, keep and label work on them unchanged
get branches() {
    if (!this._branches) { this._branches = new Components(fieldSource(this), native().graphComponents(this._handle(), 0)); }
    return this._branches;
}
get nodes() {
    if (!this._nodes) { this._nodes = new Components(fieldSource(this), native().graphComponents(this._handle(), 1)); }
    return this._nodes;
}

_window(first, n, count, what) {
    first = first !== undefined && first !== null ? first : 0;
    n = n !== undefined && n !== null ? n : count - first;
    if (!Number.isInteger(first) || !Number.isInteger(n) || first < 0 || first > count || n < 0 || n > count - first) {
        throw new Error(`${what} ${JSON.stringify(first)} .. +${JSON.stringify(n)} are not within the ${count} of the graph`);
    }
    return [first, n];
}

// one record per branch of rank first + 1 .. first + n (default: all): { voxels, free_ends, attachments, kind, node_lo, node_hi, steps_face,
// steps_edge, steps_corner, tip_lo, tip_hi } as numbers (js/vpt/graph.js GRAPH_BRANCH_FIELDS; the 64-bit fields are exact below 2^53)
branchRecords(first, n) {
    const w = this._window(first, n, this.info.branches, 'branches'), bytes = new ArrayBuffer(64 * w[1]), view = new DataView(bytes), out = [];
    native().graphBranches(this._handle(), w[0], new Uint8Array(bytes));
    for (let k = 0; k < w[1]; k++) {
        const r = {};
        graphHost.GRAPH_BRANCH_FIELDS.forEach((f, j) => { r[f] = j < 6 ? view.getUint32(64 * k + 4 * j, true) : Number(view.getBigUint64(64 * k + 24 + 8 * (j - 6), true)); });
        out.push(r);
    }
    return out;
}
// one record per node: { voxels, degree }
nodeRecords(first, n) {
    const w = this._window(first, n, this.info.nodes, 'nodes'), bytes = new ArrayBuffer(16 * w[1]), view = new DataView(bytes), out = [];
    native().graphNodes(this._handle(), w[0], new Uint8Array(bytes));
    for (let k = 0; k < w[1]; k++) { out.push({ voxels: Number(view.getBigUint64(16 * k, true)), degree: Number(view.getBigUint64(16 * k + 8, true)) }); }
    return out;
}

// per branch: (steps_face + sqrt 2 steps_edge + sqrt 3 steps_corner) * spacing (default 1); assumes cubic voxels
lengths(spacing) { return graphHost.graphLengths(this.branchRecords(), spacing); }

// a new, ready RG8 / RG16 volume with the source's filter: (code, class): a row of a 2-D transfer function colours ends (2) and junctions (4)
classes() { return this._derived(native().graphClasses(this._handle()), true); }

// a new, ready volume of the source's size, format and filter: the source's code where the voxel is in the set and its branch is not
// dropped, fill (default 0) elsewhere.  A branch is dropped when weights (default [10, 14, 17]) . (steps_face, steps_edge, steps_corner) <=
// length (a number or a BigInt) and it is a spur, or (debris) a segment or an isolated voxel.  One round, not thinned again
prune(length, weights, debris, fill) {
    const p = graphHost.checkPrune(length, weights, debris ? graphHost.GRAPH_PRUNE_DEBRIS : 0, fill, this._norm16 ? 65535 : 255);
    return this._derived(native().graphPrune(this._handle(), BigUint64Array.of(p[0]), p[1][0], p[1][1], p[1][2], p[2], p[3]));
}

// (for measurements) { ms: { seed, classify, branches, nodes, links, host }, launches }
profile() {
    const r = native().graphProfile(this._handle());
    return { ms: { seed: r[0], classify: r[1], branches: r[2], nodes: r[3], links: r[4], host: r[5] }, launches: r[6] };
}

close() { this.destroy(); }

}

// The squared Euclidean distances to a value range of a volume, or to its complement (Volume.distance): one Uint32 per voxel on the device.
// Transform once, select several times.  Outlives the volume it was made from; destroy() frees the device memory.
class Distance extends VoxelField {

constructor(source, handle) { super(source, handle, 'distances', 'distanceDestroy', 'distanceSquared'); }

// { seeds, largest }: the number of seeds; the largest finite squared distance, 0 without a seed
get info() {
    const i = native().distanceInfo(this._handle());
    return { seeds: i[0], largest: i[1] };
}

// Uint32Array [depth][height][width]: the squared distances of a box of voxels (default: the whole volume); 0xFFFFFFFF: there is no seed
squared(x, y, z, width, height, depth) { return this._values(x, y, z, width, height, depth); }

// a new, ready volume of the source's size, format and filter: the source's code where r2Lo <= d2 <= r2Hi (defaults 0 and 0xFFFFFFFF),
// `fill` (default 0) elsewhere
within(r2Lo, r2Hi, fill) {
    const k = checkWithin(r2Lo !== undefined ? r2Lo : 0, r2Hi, fill !== undefined ? fill : 0, this._norm16 ? 65535 : 255);
    return this._derived(native().distanceWithin(this._handle(), k[0], k[1], k[2]));
}

// a new, ready RG8 / RG16 volume with the source's filter: (code, min(isqrt(steps^2 d2), M)): the second axis of a 2-D transfer function is
// the distance, `steps` (1 .. 256, default 1) rows a voxel
channel(steps) {
    steps = checkSteps(steps !== undefined ? steps : 1);
    return this._derived(native().distanceChannel(this._handle(), steps), true);
}

// a Distance around another native handle over the same snapshot
_sibling(handle) {
    const other = Object.assign(Object.create(Distance.prototype), this);
    other._dimensions = Object.assign({}, this._dimensions); other._modality = Object.assign({}, this._modality); other._meta = Object.assign({}, this._meta);
    other._h = handle;
    return other;
}

// the local thickness, as another Distance whose values are T2: per voxel the largest squared distance D(c) among the open balls
// { |v - c|^2 < D(c) } of these distances that hold the voxel, 0 where none does (thicknessSquaredTexels states it), on the device.
// within(r^2 + 1, null) of the result is the opening by the ball of radius r, channel(2) the local diameter.  This object is not changed
thickness() { return this._sibling(native().distanceThickness(this._handle())); }

// (for measurements) [what thickness gives, { ms: { tiles, cover, info }, tiles, visited }]; flags (for tests): those of
// vpt_distance_thickness_capped (1: no value cull, 2: no reach cull); tiles is then null
thicknessTimed(flags) {
    const r = native().distanceThicknessTimed(this._handle(), flags !== undefined && flags !== null ? flags : -1);
    return [this._sibling(r[0]), { ms: { tiles: r[1], cover: r[2], info: r[3] }, tiles: flags !== undefined && flags !== null ? null : r[4], visited: r[5] }];
}

// (for measurements) { x, y, z }: milliseconds of the three passes of the transform
profile() {
    const ms = native().distanceProfile(this._handle());
    return { x: ms[0], y: ms[1], z: ms[2] };
}

}

// The connected components of a value range of a volume (Volume.components): per-voxel ranks and the component list on the device.  Label
// once, select several times.  Outlives the volume it was made from; destroy() frees the device memory.
class Components extends VoxelField {

constructor(source, handle) { super(source, handle, 'components', 'componentsDestroy', 'componentsRanks'); }

// { listed, dropped, foregroundVoxels, listedVoxels }
get info() {
    const i = native().componentsInfo(this._handle());
    return { listed: i[0], dropped: i[1], foregroundVoxels: i[2], listedVoxels: i[3] };
}

// [[rootX, rootY, rootZ, voxels], ...] of the components first .. first + n - 1 of the canonical order (defaults: all)
list(first, n) {
    first = first !== undefined ? first : 0;
    if (n === undefined || n === null) { n = Math.max(this.info.listed - first, 0); }
    const words = new Uint32Array(4 * n), out = [];
    native().componentsList(this._handle(), first, words);
    for (let k = 0; k < n; k++) { out.push([words[4 * k], words[4 * k + 1], words[4 * k + 2], words[4 * k + 3]]); }
    return out;
}

// Uint32Array [depth][height][width]: the ranks of a box of voxels (default: the whole volume)
ranks(x, y, z, width, height, depth) { return this._values(x, y, z, width, height, depth); }

// a new, ready volume of the source's size, format and filter: the source's code where first <= rank <= last (defaults 1 and every rank),
// `fill` (default 0) elsewhere
keep(first, last, fill) {
    const k = checkKeep(first !== undefined ? first : 1, last, fill !== undefined ? fill : 0, this._norm16 ? 65535 : 255);
    return this._derived(native().componentsKeep(this._handle(), k[0], k[1], k[2]));
}

// a new, ready RG8 / RG16 volume with the source's filter: (code, min(rank, M)): the rows of a 2-D transfer function select the structures
label() { return this._derived(native().componentsLabel(this._handle()), true); }

// the arguments of the native measure calls and the buffer they fill: 88 bytes a record (struct vpt_component_measure)
_measureArgs(first, n, values, channel) {
    const w = checkWindow(first !== undefined ? first : 0, n, this.info.listed);
    if (values !== undefined && values !== null && !(values instanceof Volume && values.texture)) { throw new Error('measure takes a ready volume as values'); }
    channel = channel !== undefined ? channel : 0;
    if (!Number.isInteger(channel)) { throw new Error('channel is 0 or 1, not ' + JSON.stringify(channel)); }
    return [values ? values.texture : null, channel, w[0], new ArrayBuffer(88 * w[1])];
}
static _records(buffer) {
    const view = new DataView(buffer), out = [];
    for (let at = 0; at < buffer.byteLength; at += 88) {
        const u32 = k => view.getUint32(at + 8 + 4 * k, true), u64 = k => view.getBigUint64(at + 40 + 8 * k, true);
        out.push({ voxels: view.getBigUint64(at, true), minX: u32(0), minY: u32(1), minZ: u32(2), maxX: u32(3), maxY: u32(4), maxZ: u32(5), valueMin: u32(6),
                   valueMax: u32(7), sumX: u64(0), sumY: u64(1), sumZ: u64(2), valueSum: u64(3), valueSumSq: u64(4), faces: u64(5) });
    }
    return out;
}

// one record per component of rank first + 1 .. first + n (defaults: the whole list): { voxels, minX .. maxZ, valueMin, valueMax, sumX, sumY,
// sumZ, valueSum, valueSumSq, faces } counted on the device, the 64-bit fields as BigInts; `values` (an R8, RG8, R16 or RG16 volume of this
// size; default: the labelled texels) and `channel` choose what is measured under the components (measure.js: measureTexels states it,
// derive gives centroid, mean, variance, extents)
measure(first, n, values, channel) {
    const a = this._measureArgs(first, n, values, channel);
    native().componentsMeasure(this._handle(), a[0], a[1], a[2], a[3]);
    return Components._records(a[3]);
}

// (for measurements) [the records, the milliseconds of the measuring pass alone]
measureTimed(first, n, values, channel) {
    const a = this._measureArgs(first, n, values, channel);
    const ms = native().componentsMeasureTimed(this._handle(), a[0], a[1], a[2], a[3]);
    return [Components._records(a[3]), ms];
}

// a new, ready volume of the source's size, format and filter: the source's code where the voxel's rank is in `ranks` (an iterable of
// 1-based ranks, numbers or BigInts, duplicates and ranks beyond the list allowed; or booleans, one per listed component), `fill` elsewhere
keepSet(ranks, fill) {
    const set = checkRankSet(ranks, this.info.listed);
    const k = checkKeep(1, null, fill !== undefined ? fill : 0, this._norm16 ? 65535 : 255);
    return this._derived(native().componentsKeepSet(this._handle(), BigUint64Array.from(set, BigInt), k[2]));
}

}
// the number of smoothing passes (an integer in 1 .. 8) / of reductions (an integer >= 1); throws for anything else
function checkPasses(passes) {
    if (!Number.isInteger(passes) || passes < 1 || passes > 8) { throw new Error('smoothing passes are an integer in 1 .. 8, not ' + JSON.stringify(passes)); }
    return passes;
}
function checkLevels(levels) {
    if (!Number.isInteger(levels) || levels < 1) { throw new Error('reduction levels are an integer >= 1, not ' + JSON.stringify(levels)); }
    return levels;
}
// VPT_RANK_* of 'median' | 'erode' | 'dilate' | 'open' | 'close'; throws for anything else
const RANK_OPERATORS = ['median', 'erode', 'dilate', 'open', 'close'];
function rankOperatorCode(name) {
    const code = typeof name === 'string' ? RANK_OPERATORS.indexOf(name) : -1;
    if (code < 0) { throw new Error("a rank operator is 'median', 'erode', 'dilate', 'open' or 'close', not " + JSON.stringify(name)); }
    return code;
}
// the number of rank-filter passes (an integer in 1 .. 8); throws for anything else
function checkRankPasses(passes) {
    if (!Number.isInteger(passes) || passes < 1 || passes > 8) { throw new Error('rank-filter passes are an integer in 1 .. 8, not ' + JSON.stringify(passes)); }
    return passes;
}
// The surface of a volume at a level as a mesh (Volume.surface): Uint32 [V][3] vertices in fixed point of 1 / 65536 voxel and Uint32 [Q][4]
// quads on the device, in the contract's order.  Extract once, read, measure and write several times.  Outlives the volume it was made from;
// destroy() (or close()) frees the device memory.
class Surface {

constructor(handle) { this._h = handle; }

_handle() {
    if (!this._h) { throw new Error('the surface has been destroyed'); }
    return this._h;
}

destroy() {
    if (this._h) { native().surfaceDestroy(this._h); this._h = null; }
}

close() { this.destroy(); }

// { vertices, quads, cells, inside, crossings: [x, y, z], level, width, height, depth, channel }
get info() {
    const i = native().surfaceInfo(this._handle());
    return { vertices: i[0], quads: i[1], cells: i[2], inside: i[3], crossings: [i[4], i[5], i[6]], level: i[7], width: i[8], height: i[9], depth: i[10], channel: i[11] };
}

// Uint32Array [n][3]: the stored coordinates q (x, y, z) of the vertices first .. first + n - 1 (defaults: all)
vertices(first, n) {
    const w = surfaceHost.checkSurfaceWindow(first !== undefined ? first : 0, n, this.info.vertices, 'vertices'), out = new Uint32Array(3 * w[1]);
    native().surfaceVertices(this._handle(), w[0], out);
    return out;
}

// Uint32Array [n][4]: the vertex numbers of the quads first .. first + n - 1 (defaults: all)
quads(first, n) {
    const w = surfaceHost.checkSurfaceWindow(first !== undefined ? first : 0, n, this.info.quads, 'quads'), out = new Uint32Array(4 * w[1]);
    native().surfaceQuads(this._handle(), w[0], out);
    return out;
}

triangles() { return surfaceHost.surfaceTriangles(this.quads()); }
positions(spacing, origin) { return surfaceHost.surfacePositions(this.vertices(), spacing, origin); }
area(spacing) { return surfaceHost.surfaceArea(this.vertices(), this.quads(), spacing); }
volume(spacing) { return surfaceHost.surfaceVolume(this.vertices(), this.quads(), spacing); }
normals(spacing) { return surfaceHost.surfaceNormals(this.vertices(), this.quads(), spacing); }
writeStl(path, spacing, origin) { surfaceHost.writeStl(path, this.vertices(), this.quads(), spacing, origin); }
writePly(path, spacing, origin) { surfaceHost.writePly(path, this.vertices(), this.quads(), spacing, origin); }
writeObj(path, spacing, origin) { surfaceHost.writeObj(path, this.vertices(), this.quads(), spacing, origin); }

// (for measurements) { inside, classify, scan, vertices, quads } in milliseconds
get profile() {
    const r = native().surfaceProfile(this._handle());
    return { inside: r[0], classify: r[1], scan: r[2], vertices: r[3], quads: r[4] };
}

}

module.exports = { Volume, Components, Distance, Skeleton, Graph, Surface, RAWReader, filterCode, gradientArguments, windowFormatBits, percentileWindow, checkPasses, checkLevels, rankOperatorCode, checkRankPasses };
