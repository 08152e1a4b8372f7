'use strict';
// The watershed of a relief by steepest descent on its lower completion in plain JS: the contract of include/vpt.h ("watershed") restated
// for hosts without a device, the twin of vpt_amd/watershed.py.  texels: a Uint8Array / Uint16Array of [nz][ny][nx] codes, or interleaved
// [nz][ny][nx][2] with options.channels = 2 and options.channel naming the channel that is read.  M = 255 / 65535.
//   domain:   D = { v : lo <= relief(v) <= hi }; only voxels of D are flooded and count as neighbours, the rest has rank 0
//   polarity: 'minima': k = relief; 'maxima': k = M - relief (a depth channel)
//   lower completion: d(v) = 0 if v has a neighbour u in D with k(u) < k(v); otherwise 1 + min of d(u) over the neighbours u in D with
//             k(u) = k(v); infinity when no such chain reaches a voxel with d = 0: the regional minima of k within D
//   descent:  d(v) = 0: p(v) = the neighbour in D of smallest k below k(v), then of smallest linear index (z ny + y) nx + x;
//             0 < d(v) < infinity: the neighbour of the same k with d one less, of smallest linear index
//   basins:   a regional minimum together with every voxel whose walk along p ends in it; root = the basin's smallest linear index; basins of
//             fewer than minVoxels voxels are dropped, the others ranked by voxel count descending, then by root ascending
const { checkConnectivity, checkRange, checkMinVoxels } = require('./components.js');
const { checkGeodesicH, checkSourceChannel, geodesicTexels } = require('./reconstruct.js');
const { checkSteps, distanceSquaredTexels, channelTexels } = require('./distance.js');

const POLARITIES = ['minima', 'maxima'];                        // VPT_WATERSHED_*
const SPLIT_DEFAULTS = { h: 2, steps: 4, connectivity: 26, minVoxels: 1 };

// the code of 'minima' | 'maxima' (VPT_WATERSHED_*)
function checkPolarity(polarity) {
    const code = typeof polarity === 'string' ? POLARITIES.indexOf(polarity) : -1;
    if (code < 0) { throw new Error("watershed polarity is 'minima' or 'maxima', not " + JSON.stringify(polarity)); }
    return code;
}
// the `split` option of a rendering context with every key, or null: null | { lo, hi, h: 2, steps: 4, connectivity: 26, minVoxels: 1 }
function checkSplit(split, largest) {
    if (split === null || split === undefined) { return null; }
    largest = largest !== undefined ? largest : 65535;
    const known = ['lo', 'hi'].concat(Object.keys(SPLIT_DEFAULTS));
    if (typeof split !== 'object' || Array.isArray(split) || split.lo === undefined || split.hi === undefined || Object.keys(split).some(k => known.indexOf(k) < 0)) {
        throw new Error('split is null or { lo, hi, h: 2, steps: 4, connectivity: 26, minVoxels: 1 }, not ' + JSON.stringify(split));
    }
    const out = Object.assign({}, SPLIT_DEFAULTS);
    for (const k of Object.keys(split)) { if (split[k] !== undefined && split[k] !== null) { out[k] = split[k]; } }
    checkRange(out.lo, out.hi, largest);
    checkGeodesicH('hmax', out.h, largest);
    checkSteps(out.steps);
    checkConnectivity(out.connectivity);
    checkMinVoxels(out.minVoxels);
    return out;
}
function neighbourOffsets(connectivity) {
    const most = connectivity === 6 ? 1 : (connectivity === 18 ? 2 : 3), out = [];
    for (let dz = -1; dz <= 1; dz++) { for (let dy = -1; dy <= 1; dy++) { for (let dx = -1; dx <= 1; dx++) {
        const m = (dx !== 0) + (dy !== 0) + (dz !== 0);
        if (m >= 1 && m <= most) { out.push([dx, dy, dz]); }                      // in the order of the linear index
    } } }
    return out;
}

// { ranks: Uint32Array [nz][ny][nx], list: [[rootX, rootY, rootZ, voxels], ...] in canonical order, pointer: Float64Array (the linear index a
// voxel points to; its own on a minimum voxel, -1 outside D) }: dims = [nx, ny, nz], options = { polarity ('minima'), connectivity (6),
// minVoxels (1), channels, channel }
function watershedTexels(texels, dims, lo, hi, options) {
    options = options || {};
    const flip = checkPolarity(options.polarity !== undefined ? options.polarity : 'minima') === 1;
    const connectivity = checkConnectivity(options.connectivity !== undefined ? options.connectivity : 6);
    const minVoxels = checkMinVoxels(options.minVoxels !== undefined ? options.minVoxels : 1);
    if (!(texels instanceof Uint8Array) && !(texels instanceof Uint16Array)) { throw new Error('the relief is a Uint8Array or a Uint16Array'); }
    const M = texels instanceof Uint16Array ? 65535 : 255, [nx, ny, nz] = dims, n = nx * ny * nz;
    const channels = options.channels !== undefined ? options.channels : 1;
    if ((channels !== 1 && channels !== 2) || n < 1 || texels.length !== n * channels) { throw new Error('the relief is [nz][ny][nx] or [nz][ny][nx][2]'); }
    const channel = checkSourceChannel(options.channel !== undefined ? options.channel : 0, channels);
    checkRange(lo, hi, M);
    const offsets = neighbourOffsets(connectivity);
    const NONE = M + 1;                                          // the key of what is not in D: never below, never equal to, a voxel of D
    const k = new Int32Array(n);
    for (let i = 0; i < n; i++) { const c = texels[i * channels + channel]; k[i] = c >= lo && c <= hi ? (flip ? M - c : c) : NONE; }
    const around = (i, visit) => {                               // visit(j) for the neighbours of i in D, in index order
        const x = i % nx, y = Math.floor(i / nx) % ny, z = Math.floor(i / (nx * ny));
        for (const [dx, dy, dz] of offsets) {
            const xx = x + dx, yy = y + dy, zz = z + dz;
            if (xx < 0 || xx >= nx || yy < 0 || yy >= ny || zz < 0 || zz >= nz) { continue; }
            const j = (zz * ny + yy) * nx + xx;
            if (k[j] !== NONE) { visit(j); }
        }
    };
    // d by breadth-first search from the plateaus' lower borders, inside the level sets
    const d = new Float64Array(n).fill(Infinity);
    let queue = [];
    for (let i = 0; i < n; i++) {
        if (k[i] === NONE) { continue; }
        let lower = false;
        around(i, j => { if (k[j] < k[i]) { lower = true; } });
        if (lower) { d[i] = 0; queue.push(i); }
    }
    while (queue.length) {
        const next = [];
        for (const i of queue) { around(i, j => { if (k[j] === k[i] && d[j] === Infinity) { d[j] = d[i] + 1; next.push(j); } }); }
        queue = next;
    }
    const pointer = new Float64Array(n).fill(-1);
    for (let i = 0; i < n; i++) {
        if (k[i] === NONE) { continue; }
        let best = -1;
        if (d[i] === Infinity) { best = i; }
        else if (d[i] === 0) { let key = k[i]; around(i, j => { if (k[j] < key) { key = k[j]; best = j; } }); }
        else { around(i, j => { if (best < 0 && k[j] === k[i] && d[j] === d[i] - 1) { best = j; } }); }
        pointer[i] = best;
    }
    // the regional minima by flood fill, in index order: the seed of a minimum is its smallest voxel
    const region = new Float64Array(n).fill(-1), stack = [];
    for (let seed = 0; seed < n; seed++) {
        if (k[seed] === NONE || d[seed] !== Infinity || region[seed] >= 0) { continue; }
        region[seed] = seed; stack.push(seed);
        while (stack.length) { around(stack.pop(), j => { if (d[j] === Infinity && region[j] < 0) { region[j] = seed; stack.push(j); } }); }
    }
    // every voxel of D walks to its minimum; a basin is named by its smallest voxel
    const basin = new Float64Array(n).fill(-1), first = new Map(), sizes = new Map();
    for (let i = 0; i < n; i++) {
        if (k[i] === NONE) { continue; }
        let t = i;
        while (pointer[t] !== t) { t = pointer[t]; }
        const name = region[t];
        basin[i] = name;
        if (!first.has(name)) { first.set(name, i); sizes.set(name, 0); }       // voxels come in index order: the first is the root
        sizes.set(name, sizes.get(name) + 1);
    }
    const order = Array.from(first.keys()).filter(name => sizes.get(name) >= minVoxels);
    order.sort((p, q) => sizes.get(q) - sizes.get(p) || first.get(p) - first.get(q));
    const rankOf = new Map();
    order.forEach((name, position) => rankOf.set(name, position + 1));
    const ranks = new Uint32Array(n);
    for (let i = 0; i < n; i++) { if (basin[i] >= 0) { ranks[i] = rankOf.get(basin[i]) || 0; } }
    const list = order.map(name => { const r = first.get(name); return [r % nx, Math.floor(r / nx) % ny, Math.floor(r / (nx * ny)), sizes.get(name)]; });
    return { ranks, list, pointer };
}

// what Volume.split holds: distance to the rest -> channel(steps) -> hmax(h) of channel 1 -> watershed(1, M, 'maxima'); options = { h (2),
// steps (4), connectivity (26), minVoxels (1) }
function splitTexels(texels, dims, lo, hi, options) {
    const spec = checkSplit(Object.assign({ lo, hi }, options || {}), texels instanceof Uint16Array ? 65535 : 255);
    const [nx, ny, nz] = dims;
    const depth = channelTexels(texels, distanceSquaredTexels(texels, nx, ny, nz, lo, hi, 'rest'), spec.steps);
    const flattened = geodesicTexels(depth, dims, 'hmax', { h: spec.h, connectivity: spec.connectivity, channels: 2, channel: 1 });
    return watershedTexels(flattened, dims, 1, texels instanceof Uint16Array ? 65535 : 255,
        { polarity: 'maxima', connectivity: spec.connectivity, minVoxels: spec.minVoxels });
}

module.exports = { WATERSHED_POLARITIES: POLARITIES, checkPolarity, checkSplit, watershedTexels, splitTexels };
