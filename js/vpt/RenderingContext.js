'use strict';
// src/js/RenderingContext.js:20-229, headless: the caller of the renderer path (SURVEY section 8b "Caller to
// reproduce").  Same members and methods minus the browser parts (canvas, WebGL context loss, animators, recording):
// where the reference blits the tone mapper's texture to the canvas (:199-209), getFrame() reads it back.
//   new RenderingContext({ resolution, filter, device, rng })     resolution: number or { width, height }; filter: 'linear' (default),
//   'nearest' or 'quasicubic'; gradient: null (default), 'central' or 'sobel', gradientGain (default 1): a one-channel R8 / R16 volume gets its
//   gradient magnitude as second channel when it is loaded (Volume.deriveGradient); window: null (default), [lo, hi], 'range' or
//   { percentiles: [a, b] }, windowFormat: 'r8' (default) or 'r16': a one-channel volume is windowed when it is loaded, before the gradient
//   is derived (Volume.window); smooth: null (default) or passes 1 .. 8: an R8 / R16 volume is smoothed behind the window (Volume.smooth);
//   reduce: null (default), 0 or levels >= 1: the volume is reduced to half its resolution that many times behind the smoothing (Volume.reduce)
//   rank: null (default), 'median', 'erode', 'dilate', 'open' or 'close', rankPasses 1 .. 8 (default 1): an R8 / R16 volume gets that rank filter
//   over the 3 x 3 x 3 box behind the window and in front of the smoothing (Volume.rank)
//   components: null (default), { lo, hi, connectivity: 6, minVoxels: 1, mode: 'keep', keep: n | null } or { ..., mode: 'label' }: the connected
//   components of the codes lo .. hi of an R8 / R16 volume (Volume.components).  'keep' runs behind the rank filter and in front of the
//   smoothing: the n largest (null: all of at least minVoxels voxels) keep their codes, everything else becomes 0.  'label' runs where the
//   gradient runs, on the final scalar volume: the second channel is min(rank, M); it cannot be combined with `gradient`
//   distance: null (default), { lo, hi, seeds: 'range', mode: 'within', from: 0, to: null, fill: 0 } or { ..., mode: 'channel', steps: 1 }: the
//   exact squared Euclidean distance d2 of every voxel of an R8 / R16 volume to the codes lo .. hi (seeds 'range') or to the codes outside
//   them (seeds 'rest') (Volume.distance).  'within' runs behind `components` mode 'keep' and in front of the smoothing: the codes with
//   from <= d2 <= to (squared voxels; to null: no upper end) stay, everything else becomes `fill`.  'channel' runs where the gradient runs:
//   the second channel is min(isqrt(steps^2 d2), M); it cannot be combined with `gradient` or with `components` mode 'label'
//   thickness: null (default) or the keys of `distance`, with seeds 'rest' and steps 2 by default: the squared local thickness T2 (the largest
//   inscribed ball that holds the voxel; Distance.thickness) in the place of d2, applied where `distance` is and conflicting as it does:
//   'within' from r^2 + 1 is the opening by the ball of radius r, 'channel' with steps 2 the diameter in voxels.  Naming both throws.
//   skeleton: null (default) or { lo, hi, mode: 'kernel' | 'ends' (default) | 'isthmus', passes: 0, fill: 0 }: the volume is replaced by the
//   skeleton of the codes lo .. hi (Volume.skeleton): the voxels that survive the thinning keep their codes, everything else becomes
//   `fill`.  It is applied where `thickness` mode 'within' is; naming it together with `distance` or `thickness` mode 'within' throws.
//   resample: null (default), { size: [w, h, d] } or { spacing: [sx, sy, sz], pitch }, plus mode: 'filtered' (default) | 'nearest': the volume
//   is resampled to that grid, or to cubic voxels of edge `pitch` (default: the smallest spacing), behind the window and in front of the rank
//   filter, so rank, components and distance see the resampled grid (Volume.resample, Volume.isotropic); a volume whose format the mode does
//   not take is left as it is
//   combine: null (default) or { reader | volume, op, channel, lo, hi, fill, wa, wb, offset, resample: null | 'nearest' | 'filtered' }: an
//   R8 / R16 volume is combined with a second one when it is loaded (Volume.combine).  A `reader` is loaded into a second volume and
//   destroyed afterwards, a `volume` stays the caller's; with `resample` set and differing sizes the second volume is first resampled to the
//   primary's current grid in that mode.  The one-channel ops run behind `resample` and in front of `rank`; 'pair' runs where the gradient
//   runs, so it cannot be combined with `gradient`, `components` mode 'label' or `distance` mode 'channel'
//   geodesic: null (default) or { op: 'fill_holes' | 'clear_border' | 'hmax' | 'hmin' | 'dome' | 'maxima' | 'minima', h: 0, connectivity: 6 }: an
//   R8 / R16 volume gets that geodesic operation (Volume.geodesic) behind the rank filter and in front of `components` mode 'keep' and the
//   smoothing
//   split: null (default) or { lo, hi, h: 2, steps: 4, connectivity: 26, minVoxels: 1 }: the structures of the codes lo .. hi of an R8 / R16
//   volume with touching ones split by the watershed of their depth (Volume.split).  It runs where the gradient runs, on the final scalar
//   volume: the second channel is min(rank of the basin, M), so it cannot be combined with `gradient`, `components` mode 'label', `distance`
//   mode 'channel' or `combine` op 'pair'
const { EventTarget, CustomEvent } = require('./EventTarget.js');
const { Context } = require('./Context.js');
const { OrbitCameraAnimator } = require('./animators.js');
const { Node, Transform, PerspectiveCamera } = require('./scene.js');
const { Volume, gradientArguments, windowFormatBits, checkPasses, checkLevels, rankOperatorCode, checkRankPasses } = require('./Volume.js');
const { native } = require('./native.js');
const { checkConnectivity, checkRange, checkMinVoxels, checkKeep } = require('./components.js');
const { checkSeeds, checkSteps, checkWithin, checkDistanceRange } = require('./distance.js');
const { checkResampleMode, checkResampleSize, checkSpacing } = require('./resample.js');
const { checkCombineOp, checkCombineChannel, checkCombineWeights, checkCombineMask } = require('./combine.js');
const { checkGeodesicH } = require('./reconstruct.js');
const { checkSplit } = require('./watershed.js');
const { checkSkeleton, THIN_KEPT } = require('./skeleton.js');
const { RendererFactory } = require('./renderers/RendererFactory.js');
const { ToneMapperFactory } = require('./tonemappers/ToneMapperFactory.js');

class RenderingContext extends EventTarget {

constructor(options) {
    super();
    options = options || {};
    this.render = this.render.bind(this);
    this.gradient = options.gradient !== undefined ? options.gradient : null;
    this.gradientGain = options.gradientGain !== undefined && options.gradientGain !== null ? options.gradientGain : 1;
    if (this.gradient !== null) { gradientArguments(native(), this.gradient, this.gradientGain); }   // a bad option fails here, not at the first volume
    this.window = options.window !== undefined ? options.window : null;
    this.windowFormat = options.windowFormat !== undefined && options.windowFormat !== null ? options.windowFormat : 'r8';
    if (this.window !== null) { windowFormatBits(this.windowFormat); RenderingContext._windowSpec(this.window); }   // likewise
    this.smooth = options.smooth !== undefined ? options.smooth : null;
    this.reduce = options.reduce !== undefined ? options.reduce : null;
    if (this.smooth !== null) { checkPasses(this.smooth); }                          // likewise
    if (this.reduce !== null && this.reduce !== 0) { checkLevels(this.reduce); }
    this.rank = options.rank !== undefined ? options.rank : null;
    this.rankPasses = options.rankPasses !== undefined && options.rankPasses !== null ? options.rankPasses : 1;
    if (this.rank !== null) { rankOperatorCode(this.rank); }                         // likewise
    checkRankPasses(this.rankPasses);
    this.components = RenderingContext._componentsSpec(options.components);          // likewise
    if (this.components !== null && this.components.mode === 'label' && this.gradient !== null) {
        throw new Error("components mode 'label' and gradient both write the second channel: name one of them");
    }
    this.distance = RenderingContext._distanceSpec(options.distance);                // likewise
    if (this.distance !== null && this.distance.mode === 'channel') {
        if (this.gradient !== null) { throw new Error("distance mode 'channel' and gradient both write the second channel: name one of them"); }
        if (this.components !== null && this.components.mode === 'label') {
            throw new Error("distance mode 'channel' and components mode 'label' both write the second channel: name one of them");
        }
    }
    this.thickness = RenderingContext._distanceSpec(options.thickness, 'thickness'); // likewise
    if (this.thickness !== null) {
        if (this.distance !== null) { throw new Error('distance and thickness are two readings of one transform: name one of them'); }
        if (this.thickness.mode === 'channel') {
            if (this.gradient !== null) { throw new Error("thickness mode 'channel' and gradient both write the second channel: name one of them"); }
            if (this.components !== null && this.components.mode === 'label') {
                throw new Error("thickness mode 'channel' and components mode 'label' both write the second channel: name one of them");
            }
        }
    }
    this.skeleton = checkSkeleton(options.skeleton);                                 // likewise
    if (this.skeleton !== null) {
        if (this.distance !== null && this.distance.mode === 'within') {
            throw new Error("skeleton and distance mode 'within' both replace the volume by a selection of it: name one of them");
        }
        if (this.thickness !== null && this.thickness.mode === 'within') {
            throw new Error("skeleton and thickness mode 'within' both replace the volume by a selection of it: name one of them");
        }
    }
    this.resample = RenderingContext._resampleSpec(options.resample);                // likewise
    this.combine = RenderingContext._combineSpec(options.combine);                   // likewise
    if (this.combine !== null && this.combine.op === 'pair') {
        if (this.gradient !== null) { throw new Error("combine op 'pair' and gradient both write the second channel: name one of them"); }
        if (this.components !== null && this.components.mode === 'label') {
            throw new Error("combine op 'pair' and components mode 'label' both write the second channel: name one of them");
        }
        if (this.distance !== null && this.distance.mode === 'channel') {
            throw new Error("combine op 'pair' and distance mode 'channel' both write the second channel: name one of them");
        }
        if (this.thickness !== null && this.thickness.mode === 'channel') {
            throw new Error("combine op 'pair' and thickness mode 'channel' both write the second channel: name one of them");
        }
    }
    this.geodesic = RenderingContext._geodesicSpec(options.geodesic);                // likewise
    this.split = checkSplit(options.split);                                          // likewise
    if (this.split !== null) {
        if (this.gradient !== null) { throw new Error('split and gradient both write the second channel: name one of them'); }
        if (this.components !== null && this.components.mode === 'label') {
            throw new Error("split and components mode 'label' both write the second channel: name one of them");
        }
        if (this.distance !== null && this.distance.mode === 'channel') {
            throw new Error("split and distance mode 'channel' both write the second channel: name one of them");
        }
        if (this.thickness !== null && this.thickness.mode === 'channel') {
            throw new Error("split and thickness mode 'channel' both write the second channel: name one of them");
        }
        if (this.combine !== null && this.combine.op === 'pair') { throw new Error("split and combine op 'pair' both write the second channel: name one of them"); }
    }
    this.gl = new Context(options.device || 0);                                   // initGL(), :61-105
    this.environmentTexture = { data: new Uint8Array([255, 255, 255, 255]), width: 1, height: 1 };   // :90-101
    this._rng = options.rng;
    this._resolution = options.resolution !== undefined ? options.resolution : 512;   // :35
    this.filter = options.filter !== undefined ? options.filter : 'linear';           // :36
    this.camera = new Node();                                                         // :38-40
    this.camera.transform.localTranslation = [0, 0, 2];
    this.camera.components.push(new PerspectiveCamera(this.camera));
    this.camera.transform.addEventListener('change', () => {                          // :42-46
        if (this.renderer) { this.renderer.reset(); }
    });
    this.volume = new Volume(this.gl);                                                // :56
    this.volumeTransform = new Transform(new Node());                                 // :57
    this.renderer = null;
    this.toneMapper = null;
    this.cameraAnimator = new OrbitCameraAnimator(this.camera, null);                 // :54 (headless: no canvas to listen on)
    const size = this._size();
    this.resize(size[0], size[1]);
}

_size() {
    const r = this._resolution;
    return typeof r === 'number' ? [r, r] : [r.width, r.height];
}

destroy() {
    if (this.toneMapper) { this.toneMapper.destroy(); this.toneMapper = null; }
    if (this.renderer) { this.renderer.destroy(); this.renderer = null; }
    if (this.volume) { this.volume.destroy(); }
    this.gl.destroy();
}

resize(width, height) {                                                               // :117-121
    this.camera.getComponent(PerspectiveCamera).aspect = width / height;
}

async setVolume(reader) {                                                             // :123-133
    const old = this.volume;
    this.volume = new Volume(this.gl, reader);
    this.volume.addEventListener('progress', e => {
        this.dispatchEvent(new CustomEvent('progress', { detail: e.detail }));
    });
    await this.volume.load();
    this.volume.setFilter(this.filter);
    try {
        if (this.window !== null) {                                                    // the transfer function's x axis is [lo, hi]
            const source = this.volume, w = this._windowOf(source);
            this.volume = source.window({ lo: w[0], hi: w[1], format: this.windowFormat });
            source.destroy();
        }
        if (this.resample !== null && RenderingContext._resampleTakes(this.volume, this.resample.mode)) {
            const source = this.volume, spec = this.resample;
            this.volume = spec.size !== null ? source.resample(spec.size[0], spec.size[1], spec.size[2], spec.mode)
                : source.isotropic(spec.spacing, spec.pitch, spec.mode);
            source.destroy();
        }
        if (this.combine !== null && this.combine.op !== 'pair') { await this._combineWith(this.combine); }
        if (this.rank !== null) {
            const N = native(), fmt = this.volume.nativeFormat();
            if (fmt === N.VPT_FORMAT_R8 || fmt === N.VPT_FORMAT_R16) {                 // the formats the smoothing takes: any other volume as it is
                const source = this.volume;
                this.volume = source.rank(this.rank, this.rankPasses);
                source.destroy();
            }
        }
        if (this.geodesic !== null) {
            const N = native(), fmt = this.volume.nativeFormat();
            if (fmt === N.VPT_FORMAT_R8 || fmt === N.VPT_FORMAT_R16) {                 // any other volume as it is
                const source = this.volume, spec = this.geodesic;
                this.volume = source.geodesic(spec.op, Math.min(spec.h, fmt === N.VPT_FORMAT_R16 ? 65535 : 255), spec.connectivity);
                source.destroy();
            }
        }
        if (this.components !== null && this.components.mode === 'keep') { this._derive(found => found.keep(1, this.components.keep)); }
        if (this.distance !== null && this.distance.mode === 'within') {
            const spec = this.distance;
            this._deriveDistance(found => found.within(spec.from, spec.to, spec.fill));
        }
        if (this.thickness !== null && this.thickness.mode === 'within') {
            const spec = this.thickness;
            this._deriveDistance(found => found.within(spec.from, spec.to, spec.fill), true);
        }
        if (this.skeleton !== null) {
            const N = native(), fmt = this.volume.nativeFormat(), spec = this.skeleton;
            if (fmt === N.VPT_FORMAT_R8 || fmt === N.VPT_FORMAT_R16) {                 // any other volume as it is
                const source = this.volume, largest = fmt === N.VPT_FORMAT_R16 ? 65535 : 255;      // the range is open above
                const found = source.skeleton(spec.lo, Math.min(spec.hi, largest), spec.mode, spec.passes);
                try { this.volume = found.within(THIN_KEPT, THIN_KEPT, Math.min(spec.fill, largest)); } finally { found.destroy(); }
                source.destroy();
            }
        }
        if (this.smooth !== null) {
            const N = native(), fmt = this.volume.nativeFormat();
            if (fmt === N.VPT_FORMAT_R8 || fmt === N.VPT_FORMAT_R16) {                 // the formats the gradient takes: any other volume as it is
                const source = this.volume;
                this.volume = source.smooth(this.smooth);
                source.destroy();
            }
        }
        if (this.reduce) {
            const source = this.volume;
            this.volume = source.reduce(this.reduce);
            source.destroy();
        }
        if (this.gradient !== null) {
            const N = native(), fmt = this.volume.nativeFormat();
            if (fmt === N.VPT_FORMAT_R8 || fmt === N.VPT_FORMAT_R16) {                 // (value, gradient magnitude): the 2-D transfer function's axes
                const source = this.volume;
                this.volume = source.deriveGradient({ operator: this.gradient, gain: this.gradientGain });
                source.destroy();
            }
        }
        if (this.components !== null && this.components.mode === 'label') { this._derive(found => found.label()); }   // (value, rank)
        if (this.distance !== null && this.distance.mode === 'channel') { this._deriveDistance(found => found.channel(this.distance.steps)); }   // (value, distance)
        if (this.thickness !== null && this.thickness.mode === 'channel') { this._deriveDistance(found => found.channel(this.thickness.steps), true); }   // (value, local thickness)
        if (this.combine !== null && this.combine.op === 'pair') { await this._combineWith(this.combine); }                    // (value, the second volume)
        if (this.split !== null) {
            const N = native(), fmt = this.volume.nativeFormat();
            if (fmt === N.VPT_FORMAT_R8 || fmt === N.VPT_FORMAT_R16) {                 // (value, basin): any other volume as it is
                const source = this.volume, spec = this.split, largest = fmt === N.VPT_FORMAT_R16 ? 65535 : 255;      // hi and h are open above
                const found = source.split(spec.lo, Math.min(spec.hi, largest),
                    { h: Math.min(spec.h, largest), steps: spec.steps, connectivity: spec.connectivity, minVoxels: spec.minVoxels });
                try { this.volume = found.label(); } finally { found.destroy(); }
                source.destroy();
            }
        }
    } catch (e) {                                                                      // the context keeps the volume it had
        this.volume.destroy();
        this.volume = old;
        throw e;
    }
    if (this.renderer) { this.renderer.setVolume(this.volume); }
    if (old) { old.destroy(); }                                                        // device memory is not garbage-collected
}

// replaces this.volume (if it is R8 / R16: any other volume stays as it is) by what emit(components of the `components` option) returns
_derive(emit) {
    const N = native(), fmt = this.volume.nativeFormat(), spec = this.components;
    if (fmt !== N.VPT_FORMAT_R8 && fmt !== N.VPT_FORMAT_R16) { return; }
    const source = this.volume, largest = fmt === N.VPT_FORMAT_R16 ? 65535 : 255;      // the range is open above: hi may exceed an R8 volume's codes
    const found = source.components(spec.lo, Math.min(spec.hi, largest), spec.connectivity, spec.minVoxels);
    try { this.volume = emit(found); } finally { found.destroy(); }
    source.destroy();
}

// replaces this.volume (if it is R8 / R16: any other volume stays as it is) by what emit(distances of the `distance` option) returns, or
// (thickness) emit(local thickness of the `thickness` option)
_deriveDistance(emit, thickness) {
    const N = native(), fmt = this.volume.nativeFormat(), spec = thickness ? this.thickness : this.distance;
    if (fmt !== N.VPT_FORMAT_R8 && fmt !== N.VPT_FORMAT_R16) { return; }
    const source = this.volume, largest = fmt === N.VPT_FORMAT_R16 ? 65535 : 255;      // the range is open above: hi may exceed an R8 volume's codes
    let found = source.distance(spec.lo, Math.min(spec.hi, largest), spec.seeds);
    if (thickness) {
        const depth = found;
        try { found = depth.thickness(); } finally { depth.destroy(); }
    }
    try { this.volume = emit(found); } finally { found.destroy(); }
    source.destroy();
}

// replaces this.volume (if it is R8 / R16: any other volume stays as it is) by its combination with the second volume of the `combine` option
async _combineWith(spec) {
    const N = native(), fmt = this.volume.nativeFormat();
    if (fmt !== N.VPT_FORMAT_R8 && fmt !== N.VPT_FORMAT_R16) { return; }
    const source = this.volume;
    let second = spec.volume, owned = false;
    if (second === null) {
        second = new Volume(this.gl, spec.reader); owned = true;
        await second.load();
    }
    try {
        const d = source.modality.dimensions, o = second.modality.dimensions;
        if (spec.resample !== null && (d.width !== o.width || d.height !== o.height || d.depth !== o.depth)) {
            const fitted = second.resample(d.width, d.height, d.depth, spec.resample);
            if (owned) { second.destroy(); }
            second = fitted; owned = true;
        }
        this.volume = source.combine(second, spec.op, Object.assign({ channel: spec.channel }, spec.params));
    } finally {
        if (owned) { second.destroy(); }
    }
    source.destroy();
}

// the `combine` option with its defaults filled in, or null; throws for anything the contract does not take
static _combineSpec(spec) {
    if (spec === undefined || spec === null) { return null; }
    const known = ['reader', 'volume', 'op', 'channel', 'lo', 'hi', 'fill', 'wa', 'wb', 'offset', 'resample'];
    const given = k => spec[k] !== undefined && spec[k] !== null;
    if (typeof spec !== 'object' || Array.isArray(spec) || !('op' in spec) || !Object.keys(spec).every(k => known.includes(k)) || given('reader') === given('volume')) {
        throw new Error("combine is null or { reader | volume, op, channel, lo, hi, fill, wa, wb, offset, resample } with one of 'reader' and 'volume', not " +
            JSON.stringify(spec, (k, v) => (k === 'reader' || k === 'volume' ? String(v) : v)));
    }
    checkCombineOp(spec.op);
    if (given('volume') && !(spec.volume instanceof Volume)) { throw new Error("combine 'volume' is a Volume"); }
    const out = { reader: given('reader') ? spec.reader : null, volume: given('volume') ? spec.volume : null, op: spec.op,
        channel: checkCombineChannel(given('channel') ? spec.channel : 0, 2), params: {}, resample: null };
    if (given('resample')) { checkResampleMode(spec.resample); out.resample = spec.resample; }
    if (spec.op !== 'mask' && ['lo', 'hi', 'fill'].some(given)) { throw new Error("combine 'lo', 'hi' and 'fill' go with op 'mask'"); }
    if (spec.op !== 'blend' && ['wa', 'wb', 'offset'].some(given)) { throw new Error("combine 'wa', 'wb' and 'offset' go with op 'blend'"); }
    if (spec.op === 'mask') {
        const lo = given('lo') ? spec.lo : 0, fill = given('fill') ? spec.fill : 0;
        checkCombineMask(lo, given('hi') ? spec.hi : 65535, fill, 65535, 65535);
        out.params = { lo, hi: given('hi') ? spec.hi : null, fill };                  // hi null: the second volume's largest code
    } else if (spec.op === 'blend') {
        if (!given('wa') || !given('wb')) { throw new Error("combine op 'blend' needs 'wa' and 'wb'"); }
        const w = checkCombineWeights(spec.wa, spec.wb, given('offset') ? spec.offset : 0);
        out.params = { wa: w[0], wb: w[1], offset: w[2] };
    }
    return out;
}

// the `resample` option with its defaults filled in, or null; throws for anything the contract does not take
static _resampleSpec(spec) {
    if (spec === undefined || spec === null) { return null; }
    const known = ['size', 'spacing', 'pitch', 'mode'], given = k => spec[k] !== undefined && spec[k] !== null;
    if (typeof spec !== 'object' || Array.isArray(spec) || !Object.keys(spec).every(k => known.includes(k)) || ('size' in spec) === ('spacing' in spec)) {
        throw new Error("resample is null, { size: [w, h, d], mode } or { spacing: [sx, sy, sz], pitch, mode }, not " + JSON.stringify(spec));
    }
    const out = { size: null, spacing: null, pitch: null, mode: given('mode') ? spec.mode : 'filtered' };
    checkResampleMode(out.mode);
    if ('size' in spec) {
        if (given('pitch')) { throw new Error("resample 'pitch' goes with 'spacing'"); }
        if (!Array.isArray(spec.size) || spec.size.length !== 3) { throw new Error('resample size is [w, h, d], not ' + JSON.stringify(spec.size)); }
        out.size = checkResampleSize(spec.size[0], spec.size[1], spec.size[2]);
    } else {
        const k = checkSpacing(spec.spacing, spec.pitch);
        out.spacing = k[0]; out.pitch = k[1];
    }
    return out;
}

// does the mode take the volume's format?
static _resampleTakes(volume, mode) {
    const N = native(), fmt = volume.nativeFormat();
    if (mode === 'filtered') { return fmt === N.VPT_FORMAT_R8 || fmt === N.VPT_FORMAT_RG8 || fmt === N.VPT_FORMAT_R16 || fmt === N.VPT_FORMAT_RG16; }
    return !(fmt >= N.VPT_FORMAT_RGB565 && fmt <= N.VPT_FORMAT_RGB9_E5);
}

// the `distance` option (or, under its name, the `thickness` option: seeds 'rest' and steps 2 by default) with its defaults filled in, or
// null; throws for anything the contract does not take
static _distanceSpec(spec, name) {
    name = name || 'distance';
    const thickness = name === 'thickness';
    if (spec === undefined || spec === null) { return null; }
    const known = ['lo', 'hi', 'seeds', 'mode', 'from', 'to', 'fill', 'steps'], given = k => spec[k] !== undefined && spec[k] !== null;
    if (typeof spec !== 'object' || Array.isArray(spec) || !Object.keys(spec).every(k => known.includes(k)) || (spec.mode !== 'within' && spec.mode !== 'channel')) {
        throw new Error(name + " is null or { lo, hi, seeds, mode: 'within' | 'channel', from, to, fill, steps }, not " + JSON.stringify(spec));
    }
    checkDistanceRange(spec.lo, spec.hi, 65535);
    const out = { lo: spec.lo, hi: spec.hi, seeds: given('seeds') ? spec.seeds : (thickness ? 'rest' : 'range'), mode: spec.mode, from: 0, to: null, fill: 0,
        steps: thickness ? 2 : 1 };
    checkSeeds(out.seeds);
    if (spec.mode === 'within') {
        if (given('steps')) { throw new Error(name + " 'steps' goes with mode 'channel'"); }
        const k = checkWithin(given('from') ? spec.from : 0, spec.to, given('fill') ? spec.fill : 0, 65535);
        out.from = k[0]; out.to = k[1]; out.fill = k[2];
    } else {
        if (given('from') || given('to') || given('fill')) { throw new Error(name + " 'from', 'to' and 'fill' go with mode 'within'"); }
        out.steps = checkSteps(given('steps') ? spec.steps : out.steps);
    }
    return out;
}

// the `geodesic` option with its defaults filled in, or null; throws for anything the contract does not take
static _geodesicSpec(spec) {
    if (spec === undefined || spec === null) { return null; }
    if (typeof spec !== 'object' || Array.isArray(spec) || spec.op === undefined || Object.keys(spec).some(k => ['op', 'h', 'connectivity'].indexOf(k) < 0)) {
        throw new Error('geodesic is null or { op, h, connectivity }, not ' + JSON.stringify(spec));
    }
    const h = checkGeodesicH(spec.op, spec.h !== undefined && spec.h !== null ? spec.h : 0, 65535);      // h is open above: an R8 volume takes min(h, 255)
    return { op: spec.op, h, connectivity: checkConnectivity(spec.connectivity !== undefined && spec.connectivity !== null ? spec.connectivity : 6) };
}

// the `components` option with its defaults filled in, or null; throws for anything the contract does not take
static _componentsSpec(spec) {
    if (spec === undefined || spec === null) { return null; }
    const known = ['lo', 'hi', 'connectivity', 'minVoxels', 'mode', 'keep'];
    if (typeof spec !== 'object' || Array.isArray(spec) || !Object.keys(spec).every(k => known.includes(k)) || (spec.mode !== 'keep' && spec.mode !== 'label')) {
        throw new Error("components is null or { lo, hi, connectivity, minVoxels, mode: 'keep' | 'label', keep }, not " + JSON.stringify(spec));
    }
    checkRange(spec.lo, spec.hi, 65535);
    const out = { lo: spec.lo, hi: spec.hi, mode: spec.mode, keep: null,
        connectivity: checkConnectivity(spec.connectivity !== undefined && spec.connectivity !== null ? spec.connectivity : 6),
        minVoxels: checkMinVoxels(spec.minVoxels !== undefined && spec.minVoxels !== null ? spec.minVoxels : 1) };
    if (spec.keep !== undefined && spec.keep !== null) {
        if (spec.mode === 'label') { throw new Error("components 'keep' goes with mode 'keep'"); }
        out.keep = checkKeep(1, spec.keep, 0, 65535)[1];
    }
    return out;
}

// { kind: 'values', lo, hi } | { kind: 'range' } | { kind: 'percentiles', a, b } of a `window` option; throws for anything else
static _windowSpec(window) {
    if (window === 'range') { return { kind: 'range' }; }
    if (Array.isArray(window) && window.length === 2 && typeof window[0] === 'number' && typeof window[1] === 'number') {
        return { kind: 'values', lo: window[0], hi: window[1] };
    }
    if (window && typeof window === 'object' && !Array.isArray(window) && Object.keys(window).length === 1 &&
        Array.isArray(window.percentiles) && window.percentiles.length === 2) {
        const a = Number(window.percentiles[0]), b = Number(window.percentiles[1]);
        if (!(a >= 0 && a <= b && b <= 100)) { throw new Error(`window percentiles ${window.percentiles}: 0 <= a <= b <= 100`); }
        return { kind: 'percentiles', a, b };
    }
    throw new Error("window is null, [lo, hi], 'range' or { percentiles: [a, b] }, not " + JSON.stringify(window));
}

// [lo, hi] of the `window` option for this volume
_windowOf(volume) {
    const spec = RenderingContext._windowSpec(this.window);
    if (spec.kind === 'values') { return [spec.lo, spec.hi]; }
    if (spec.kind === 'percentiles') { return volume.percentileWindow(spec.a, spec.b); }
    const r = volume.range();
    if (volume.nativeFormat() !== native().VPT_FORMAT_R32F) { r[1] = Math.max(r[1], r[0] + 1); }
    return r;
}

setEnvironmentMap(image) {                                                            // :135-140 — { data: RGBA8 | HDR, width, height[, format] }
    this.environmentTexture = image;
    if (this.renderer) { this.renderer.setEnvironmentMap(image); }
}

setFilter(filter) {                                                                   // :142-150
    this.filter = filter;
    if (this.volume) {
        this.volume.setFilter(filter);
        if (this.renderer) { this.renderer.reset(); }
    }
}

chooseRenderer(renderer) {                                                            // :152-167
    if (this.renderer) { this.renderer.destroy(); }
    const rendererClass = RendererFactory(renderer);
    const options = { resolution: this._resolution, transform: this.volumeTransform };
    if (this._rng) { options.rng = this._rng; }
    this.renderer = new rendererClass(this.gl, this.volume, this.camera, this.environmentTexture, options);
    this.renderer.reset();
    if (this.toneMapper) { this.toneMapper.setTexture(this.renderer); }
    this.isTransformationDirty = true;
}

chooseToneMapper(toneMapper) {                                                        // :169-188
    if (this.toneMapper) { this.toneMapper.destroy(); }
    const toneMapperClass = ToneMapperFactory(toneMapper);
    this.toneMapper = new toneMapperClass(this.gl, this.renderer || null, { resolution: this._resolution });
}

render() {                                                                            // :190-210
    if (!this.renderer || !this.toneMapper) { return; }
    this.renderer.render();
    this.toneMapper.render();
}

// what the reference puts on the canvas: the tone mapper's RGBA8 image, read back
getFrame() { return this.toneMapper.getTexture(); }

// :259-305, headless and deterministic: for every frame time t = startTime + i / fps the camera animator is stepped, the
// renderer reset and `passes` render() calls made (the reference renders for `frameTime` seconds of wall clock), and the
// tone-mapped frame is written as directory/frameNNNN.png.  options: { directory, startTime, endTime, fps, passes }
recordAnimationToImageSequence(options) {
    const fs = require('fs'), path = require('path');
    const { encodePNG } = require('./png.js');
    options = options || {};
    if (!this.cameraAnimator || !this.renderer || !this.toneMapper) {
        throw new Error('recordAnimationToImageSequence needs a cameraAnimator, a renderer and a tone mapper');
    }
    const startTime = options.startTime || 0, endTime = options.endTime !== undefined ? options.endTime : 1;
    const fps = options.fps || 30, passes = options.passes || 16;
    const frames = Math.max(Math.ceil((endTime - startTime) * fps), 1);               // :261
    const timeStep = 1 / fps;
    fs.mkdirSync(options.directory, { recursive: true });
    const files = [];
    for (let i = 0; i < frames; i++) {
        const t = startTime + i * timeStep;                                           // :283
        this.cameraAnimator.update(t);
        this.renderer.reset();                                                        // :286
        for (let k = 0; k < passes; k++) { this.render(); }
        const file = path.join(options.directory, 'frame' + String(i).padStart(4, '0') + '.png');   // :291
        fs.writeFileSync(file, encodePNG(this.getFrame(), true));
        files.push(file);
        this.dispatchEvent(new CustomEvent('animationprogress', { detail: (i + 1) / frames }));     // :298-300
    }
    return files;
}

get resolution() { return this._resolution; }                                         // :212-214

set resolution(resolution) {                                                          // :216-229
    this._resolution = resolution;
    if (this.renderer) { this.renderer.setResolution(resolution); }
    if (this.toneMapper) {
        this.toneMapper.setResolution(resolution);
        if (this.renderer) { this.toneMapper.setTexture(this.renderer); }
    }
}

}
module.exports = { RenderingContext };
