'use strict';
// Grey-level morphological reconstruction of a marker under a mask, and the geodesic operations that are one reconstruction each, in plain
// JS: the contract of include/vpt.h ("morphological reconstruction and the geodesic operations") restated for hosts without a device, the
// twin of vpt_amd/reconstruct.py.  Texels are a Uint8Array or Uint16Array of [nz][ny][nx] texels with `channels` (1 or 2) interleaved
// channels of which `channel` is read; the result has one channel.  All compares are unsigned on whole codes, M = 255 / 65535.
// Connectivity c is 6, 18 or 26; a neighbour outside the volume does not exist.
//   dilation:  r0 = min(marker, mask);  r_k+1(v) = min(mask(v), max(r_k(v), max over the c-neighbours u of v of r_k(u)));  the result is
//              the first r_k with r_k+1 = r_k
//   erosion:   R_e(marker, mask) = M - R_d(M - marker, M - mask)
//   fill_holes    R_e(m, src), m = src on the voxels of the volume's six faces, M elsewhere
//   clear_border  src - R_d(m, src), m = src on the six faces, 0 elsewhere
//   hmax          R_d(max(src - h, 0), src);   hmin  R_e(min(src + h, M), src);   dome  src - hmax_h(src)
//   maxima        M where src > hmax_1(src), 0 elsewhere (a voxel of code 0 is never a maximum)
//   minima        M where src < hmin_1(src), 0 elsewhere (a voxel of code M is never a minimum)
const { checkConnectivity } = require('./components.js');

const RECONSTRUCT_OPS = ['dilation', 'erosion'];
const GEODESIC_OPS = ['fill_holes', 'clear_border', 'hmax', 'hmin', 'dome', 'maxima', 'minima'];
const TAKES_H = ['hmax', 'hmin', 'dome'];

// the code of 'dilation' | 'erosion' (VPT_RECONSTRUCT_*)
function checkReconstructOp(op) {
    const code = typeof op === 'string' ? RECONSTRUCT_OPS.indexOf(op) : -1;
    if (code < 0) { throw new Error("reconstruct op is 'dilation' or 'erosion', not " + JSON.stringify(op)); }
    return code;
}
// the code of 'fill_holes' | 'clear_border' | 'hmax' | 'hmin' | 'dome' | 'maxima' | 'minima' (VPT_GEODESIC_*)
function checkGeodesicOp(op) {
    const code = typeof op === 'string' ? GEODESIC_OPS.indexOf(op) : -1;
    if (code < 0) { throw new Error("geodesic op is 'fill_holes', 'clear_border', 'hmax', 'hmin', 'dome', 'maxima' or 'minima', not " + JSON.stringify(op)); }
    return code;
}
// h of the geodesic operation `op`: 0 .. largest for 'hmax', 'hmin' and 'dome', 0 for the others
function checkH(op, h, largest) {
    checkGeodesicOp(op);
    if (!Number.isInteger(h) || h < 0 || h > largest) { throw new Error(`geodesic h is an integer in 0 .. ${largest}, not ${JSON.stringify(h)}`); }
    if (TAKES_H.indexOf(op) < 0 && h !== 0) { throw new Error(`geodesic op '${op}' takes no h (0), not ${h}`); }
    return h;
}
// `channel` of a source of `channels` channels: 0, or 1 of a two-channel source
function checkSourceChannel(channel, channels) {
    if (channel !== 0 && channel !== 1) { throw new Error('channel is 0 or 1, not ' + JSON.stringify(channel)); }
    if (channel === 1 && channels !== 2) { throw new Error('channel 1 needs a two-channel volume'); }
    return channel;
}
function largestCode(texels, what) {
    if (texels instanceof Uint8Array) { return 255; }
    if (texels instanceof Uint16Array) { return 65535; }
    throw new Error(what + ' is a Uint8Array or a Uint16Array');
}
// the named channel of `texels` as an array of its own
function channelOf(texels, n, channels, channel, what) {
    channels = channels !== undefined ? channels : 1;
    if (channels !== 1 && channels !== 2) { throw new Error(what + ' has 1 or 2 channels, not ' + JSON.stringify(channels)); }
    if (texels.length !== n * channels) { throw new Error(`${what} has ${texels.length / channels} texels, not ${n}`); }
    channel = checkSourceChannel(channel !== undefined ? channel : 0, channels);
    const out = new texels.constructor(n);
    for (let i = 0; i < n; i++) { out[i] = texels[i * channels + channel]; }
    return out;
}
function neighbourOffsets(connectivity) {
    const most = connectivity === 6 ? 1 : (connectivity === 18 ? 2 : 3), out = [];
    for (let dz = -1; dz <= 1; dz++) { for (let dy = -1; dy <= 1; dy++) { for (let dx = -1; dx <= 1; dx++) {
        const m = (dx !== 0) + (dy !== 0) + (dz !== 0);
        if (m >= 1 && m <= most) { out.push([dx, dy, dz]); }
    } } }
    return out;
}
// R_d(marker, mask) (erosion: R_e) of two one-channel arrays of one type over the grid `dims` = [nx, ny, nz], the definition iterated to
// its fixed point
function reconstruct(marker, mask, dims, erosion, connectivity) {
    const [nx, ny, nz] = dims, n = nx * ny * nz, M = largestCode(mask, 'the mask'), flip = erosion ? M : 0;
    const offsets = neighbourOffsets(connectivity);
    let r = new mask.constructor(n);
    const k = new mask.constructor(n);
    for (let i = 0; i < n; i++) { k[i] = mask[i] ^ flip; r[i] = Math.min(marker[i] ^ flip, k[i]); }
    for (;;) {
        const next = new mask.constructor(n);
        let changed = false;
        for (let z = 0, i = 0; z < nz; z++) { for (let y = 0; y < ny; y++) { for (let x = 0; x < nx; x++, i++) {
            let m = r[i];
            if (m < k[i]) {
                for (const [dx, dy, dz] of offsets) {
                    const xx = x + dx, yy = y + dy, zz = z + dz;
                    if (xx >= 0 && xx < nx && yy >= 0 && yy < ny && zz >= 0 && zz < nz) { m = Math.max(m, r[(zz * ny + yy) * nx + xx]); }
                }
                m = Math.min(m, k[i]);
            }
            next[i] = m;
            if (m !== r[i]) { changed = true; }
        } } }
        if (!changed) { break; }
        r = next;
    }
    for (let i = 0; i < n; i++) { r[i] ^= flip; }
    return r;
}

// the texels vpt_volume_reconstruct gives: dims = [nx, ny, nz], options = { op ('dilation'), connectivity (6), channels, channel, maskChannels,
// maskChannel }
function reconstructTexels(marker, mask, dims, options) {
    options = options || {};
    const code = checkReconstructOp(options.op !== undefined ? options.op : 'dilation');
    const connectivity = checkConnectivity(options.connectivity !== undefined ? options.connectivity : 6);
    if (largestCode(marker, 'the marker') !== largestCode(mask, 'the mask')) { throw new Error('reconstruct needs volumes of one width'); }
    const n = dims[0] * dims[1] * dims[2];
    return reconstruct(channelOf(marker, n, options.channels, options.channel, 'the marker'),
        channelOf(mask, n, options.maskChannels, options.maskChannel, 'the mask'), dims, code === 1, connectivity);
}

// the texels vpt_volume_geodesic gives: dims = [nx, ny, nz], options = { h (0), connectivity (6), channels, channel }
function geodesicTexels(texels, dims, op, options) {
    options = options || {};
    checkGeodesicOp(op);
    const connectivity = checkConnectivity(options.connectivity !== undefined ? options.connectivity : 6);
    const M = largestCode(texels, 'the volume'), [nx, ny, nz] = dims, n = nx * ny * nz;
    const h = checkH(op, options.h !== undefined ? options.h : 0, M);
    const src = channelOf(texels, n, options.channels, options.channel, 'the volume');
    const marker = new src.constructor(n), out = new src.constructor(n);
    if (op === 'fill_holes' || op === 'clear_border') {
        for (let z = 0, i = 0; z < nz; z++) { for (let y = 0; y < ny; y++) { for (let x = 0; x < nx; x++, i++) {
            const face = x === 0 || x === nx - 1 || y === 0 || y === ny - 1 || z === 0 || z === nz - 1;
            marker[i] = face ? src[i] : (op === 'fill_holes' ? M : 0);
        } } }
        const r = reconstruct(marker, src, dims, op === 'fill_holes', connectivity);
        if (op === 'fill_holes') { return r; }
        for (let i = 0; i < n; i++) { out[i] = src[i] - r[i]; }
        return out;
    }
    const down = op === 'hmax' || op === 'dome' || op === 'maxima', step = op === 'maxima' || op === 'minima' ? 1 : h;
    for (let i = 0; i < n; i++) { marker[i] = down ? Math.max(src[i] - step, 0) : Math.min(src[i] + step, M); }
    const r = reconstruct(marker, src, dims, !down, connectivity);
    if (op === 'hmax' || op === 'hmin') { return r; }
    for (let i = 0; i < n; i++) { out[i] = op === 'dome' ? src[i] - r[i] : ((op === 'maxima' ? src[i] > r[i] : src[i] < r[i]) ? M : 0); }
    return out;
}

module.exports = { RECONSTRUCT_OPS, GEODESIC_OPS, checkReconstructOp, checkGeodesicOp, checkGeodesicH: checkH, checkSourceChannel, reconstructTexels,
    geodesicTexels };
