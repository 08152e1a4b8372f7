'use strict';
// A volume resampled to any grid size in plain JS: the contract of include/vpt.h ("resampling") restated for hosts without a device, the
// twin of vpt_amd/resample.py.  texels: a typed array of [nz][ny][nx] texels of `channels` (1 or 2) interleaved channels.  n is a source
// axis length, N the matching target length, X a result index; every division is a floor division of non-negative integers.
//   nearest:  source index j = ((2 X + 1) n) div (2 N) per axis; the texel's bytes are copied.  Uint8 / Uint16 / Int8 / Int16 / Float32 arrays.
//   filtered: Uint8Array and Uint16Array, per channel.  N >= n: linear interpolation, num = (2 X + 1) n - N, D = 2 N: num <= 0: (0, D);
//             num >= (n - 1) D: (n - 1, D); else i = num div D, f = num mod D: (i, D - f), (i + 1, f); S_axis = 2 N.  N < n: the area
//             average, w_j = min((X + 1) n, (j + 1) N) - max(X n, j N) for j = (X n) div N .. ((X + 1) n - 1) div N; S_axis = n.
//             out = (2 SUM + S) div (2 S), S = S_x S_y S_z, SUM the sum over all taps of w_x w_y w_z code: one rounding, halves up.
//             The sums along x and y stay below 2^42 and are Numbers; the last axis and the division are BigInt (2 SUM + S < 2^57).
const MODES = ['nearest', 'filtered'];
const MAX_AXIS = 4096;
const AXES = ['x', 'y', 'z'];

// the code of 'nearest' (0: VPT_RESAMPLE_NEAREST) or 'filtered' (1: VPT_RESAMPLE_FILTERED)
function checkMode(mode) {
    const code = typeof mode === 'string' ? MODES.indexOf(mode) : -1;
    if (code < 0) { throw new Error("resample mode is 'filtered' or 'nearest', not " + JSON.stringify(mode)); }
    return code;
}
// [width, height, depth] of a target grid: integers in 1 .. 4096
function checkSize(width, height, depth) {
    [width, height, depth].forEach((n, k) => {
        if (!Number.isInteger(n) || n < 1 || n > MAX_AXIS) {
            throw new Error(`resample size along ${AXES[k]} is an integer in 1 .. ${MAX_AXIS}, not ${JSON.stringify(n)}`);
        }
    });
    return [width, height, depth];
}
function positive(value, what) {
    if (typeof value !== 'number') { throw new Error(`${what} is a number, not ${JSON.stringify(value)}`); }
    if (!Number.isFinite(value) || !(value > 0)) { throw new Error(`${what} is finite and positive, not ${String(value)}`); }
    return value;
}
// [[sx, sy, sz], pitch]: three finite spacings > 0 and a finite pitch > 0 (null / undefined: the smallest spacing)
function checkSpacing(spacing, pitch) {
    if (!Array.isArray(spacing) || spacing.length !== 3) { throw new Error('spacing is [sx, sy, sz], not ' + JSON.stringify(spacing)); }
    spacing = spacing.map((s, k) => positive(s, 'the spacing along ' + AXES[k]));
    pitch = pitch === undefined || pitch === null ? Math.min(spacing[0], spacing[1], spacing[2]) : positive(pitch, 'pitch');
    return [spacing, pitch];
}
// [Nx, Ny, Nz]: the grid of cubic voxels of edge `pitch` (default: the smallest spacing) that fills the cube of a volume of size =
// [nx, ny, nz] voxels of spacing = [sx, sy, sz]: N = max(1, floor(n * s / pitch + 0.5)), IEEE doubles in this order
function isotropicShape(size, spacing, pitch) {
    if (!Array.isArray(size) || size.length !== 3) { throw new Error('size is [nx, ny, nz], not ' + JSON.stringify(size)); }
    size.forEach((n, k) => {
        if (!Number.isInteger(n) || n < 1 || n > MAX_AXIS) { throw new Error(`a volume has 1 .. ${MAX_AXIS} voxels along ${AXES[k]}, not ${JSON.stringify(n)}`); }
    });
    const checked = checkSpacing(spacing, pitch);
    return size.map((n, k) => {
        const cells = Math.floor(n * checked[0][k] / checked[1] + 0.5);
        if (!(cells <= MAX_AXIS)) { throw new Error(`the isotropic grid has ${cells} voxels along ${AXES[k]}: at most ${MAX_AXIS} are taken (choose a larger pitch)`); }
        return Math.max(1, cells);
    });
}
function checkAxis(n, N) {
    [n, N].forEach((v, k) => {
        if (!Number.isInteger(v) || v < 1 || v > MAX_AXIS) { throw new Error(`a ${k ? 'target' : 'source'} axis has 1 .. ${MAX_AXIS} texels, not ${JSON.stringify(v)}`); }
    });
}
// Int32Array [N]: the source index of every result index
function nearestIndex(n, N) {
    checkAxis(n, N);
    const out = new Int32Array(N);
    for (let X = 0; X < N; X++) { out[X] = Math.floor(((2 * X + 1) * n) / (2 * N)); }
    return out;
}
// { taps, S }: taps[X] = [[source index, weight], ...] with positive integer weights that sum to S
function axisTaps(n, N) {
    checkAxis(n, N);
    const taps = [];
    if (N >= n) {
        const D = 2 * N;
        for (let X = 0; X < N; X++) {
            const num = (2 * X + 1) * n - N;
            if (num <= 0) { taps.push([[0, D]]); }
            else if (num >= (n - 1) * D) { taps.push([[n - 1, D]]); }
            else {
                const i = Math.floor(num / D), f = num - i * D;
                taps.push(f ? [[i, D - f], [i + 1, f]] : [[i, D]]);
            }
        }
        return { taps, S: D };
    }
    for (let X = 0; X < N; X++) {
        const row = [];
        for (let j = Math.floor((X * n) / N); j <= Math.floor(((X + 1) * n - 1) / N); j++) {
            row.push([j, Math.min((X + 1) * n, (j + 1) * N) - Math.max(X * n, j * N)]);
        }
        taps.push(row);
    }
    return { taps, S: n };
}

function checked(texels, size, target, channels, filtered) {
    channels = channels !== undefined ? channels : 1;
    if (channels !== 1 && channels !== 2) { throw new Error('a volume has one or two channels'); }
    const ok = filtered ? [Uint8Array, Uint16Array] : [Uint8Array, Uint16Array, Int8Array, Int16Array, Float32Array];
    if (!ok.some(t => texels instanceof t)) {
        throw new Error((filtered ? 'filtered resampling takes a Uint8Array or a Uint16Array' : 'nearest resampling takes a Uint8Array, Uint16Array, Int8Array, Int16Array or Float32Array'));
    }
    if (!Array.isArray(size) || size.length !== 3 || !Array.isArray(target) || target.length !== 3) { throw new Error('sizes are [nx, ny, nz]'); }
    for (let k = 0; k < 3; k++) { checkAxis(size[k], target[k]); }
    checkSize(target[0], target[1], target[2]);
    if (texels.length !== size[0] * size[1] * size[2] * channels) { throw new Error('texels are [nz][ny][nx] of `channels` channels'); }
    return channels;
}

// the exact sums over all taps as BigInt64Array [NZ][NY][NX][channels], and S as a BigInt
function sums(texels, size, target, channels) {
    const [nx, ny, nz] = size, [NX, NY, NZ] = target;
    const tx = axisTaps(nx, NX), ty = axisTaps(ny, NY), tz = axisTaps(nz, NZ);
    const alongX = new Float64Array(nz * ny * NX * channels);
    for (let r = 0; r < nz * ny; r++) {
        for (let X = 0; X < NX; X++) {
            for (let c = 0; c < channels; c++) {
                let s = 0;
                for (const [j, w] of tx.taps[X]) { s += w * texels[(r * nx + j) * channels + c]; }
                alongX[(r * NX + X) * channels + c] = s;
            }
        }
    }
    const cols = NX * channels;
    const alongY = new Float64Array(nz * NY * cols);
    for (let z = 0; z < nz; z++) {
        for (let Y = 0; Y < NY; Y++) {
            for (let q = 0; q < cols; q++) {
                let s = 0;
                for (const [j, w] of ty.taps[Y]) { s += w * alongX[(z * ny + j) * cols + q]; }
                alongY[(z * NY + Y) * cols + q] = s;
            }
        }
    }
    const out = new BigInt64Array(NZ * NY * cols);
    for (let Z = 0; Z < NZ; Z++) {
        for (let p = 0; p < NY * cols; p++) {
            let s = 0n;
            for (const [j, w] of tz.taps[Z]) { s += BigInt(w) * BigInt(alongY[j * NY * cols + p]); }
            out[Z * NY * cols + p] = s;
        }
    }
    return { sums: out, S: BigInt(tx.S) * BigInt(ty.S) * BigInt(tz.S) };
}

// the texels on the grid target = [NX, NY, NZ], in the texels' type: what Volume.resample(NX, NY, NZ, mode) holds on the device
function resampleTexels(texels, size, target, mode, channels) {
    const code = checkMode(mode !== undefined ? mode : 'filtered');
    channels = checked(texels, size, target, channels, code === 1);
    const [nx, ny] = size, [NX, NY, NZ] = target;
    const out = new texels.constructor(NX * NY * NZ * channels);
    if (code === 0) {
        const ix = nearestIndex(size[0], NX), iy = nearestIndex(size[1], NY), iz = nearestIndex(size[2], NZ);
        const bytes = texels.BYTES_PER_ELEMENT * channels;
        const from = new Uint8Array(texels.buffer, texels.byteOffset, texels.byteLength), to = new Uint8Array(out.buffer);
        for (let Z = 0; Z < NZ; Z++) {
            for (let Y = 0; Y < NY; Y++) {
                for (let X = 0; X < NX; X++) {
                    const s = ((iz[Z] * ny + iy[Y]) * nx + ix[X]) * bytes, d = ((Z * NY + Y) * NX + X) * bytes;
                    for (let b = 0; b < bytes; b++) { to[d + b] = from[s + b]; }
                }
            }
        }
        return out;
    }
    const k = sums(texels, size, target, channels);
    for (let i = 0; i < out.length; i++) { out[i] = Number((2n * k.sums[i] + k.S) / (2n * k.S)); }
    return out;
}

// the number of result texels (per channel) of the filtered resampling whose exact value lies halfway between two codes
function countTies(texels, size, target, channels) {
    channels = checked(texels, size, target, channels, true);
    const k = sums(texels, size, target, channels);
    let ties = 0;
    for (let i = 0; i < k.sums.length; i++) { if ((2n * k.sums[i]) % (2n * k.S) === k.S) { ties++; } }
    return ties;
}

module.exports = { resampleTexels, isotropicShape, axisTaps, nearestIndex, countTies, checkResampleMode: checkMode, checkResampleSize: checkSize,
    checkSpacing, RESAMPLE_MAX_AXIS: MAX_AXIS };
