'use strict';
// node js/test/test_resample_host.js [TEXELS NX NY NZ BITS CHANNELS TX TY TZ] — no device: the argument checks of js/vpt/resample.js, the
// option validation of RenderingContext and the plain-JS twin against a brute force over every tap in BigInt.  With arguments, the twin of
// the texels in the file TEXELS on the grid TX x TY x TZ is printed as one JSON line (tests/test_resample_host.py compares it with the
// numpy statement).
const fs = require('fs');
const r = require('../vpt/resample.js');
const { RenderingContext } = require('../vpt/RenderingContext.js');

function throws(f, what, pattern) {
    let message = null;
    try { f(); } catch (e) { message = e.message; }
    if (message === null) { throw new Error(what + ' was accepted'); }
    if (pattern && !pattern.test(message)) { throw new Error(what + ': unexpected message ' + message); }
}
function equal(a, b, what) {
    if (a.length !== b.length) { throw new Error(what + ': wrong length'); }
    for (let i = 0; i < a.length; i++) { if (a[i] !== b[i]) { throw new Error(`${what}: element ${i} is ${a[i]}, expected ${b[i]}`); } }
}
// the taps of the contract, written out once more
function taps(n, N, X) {
    if (N >= n) {
        const D = 2 * N, num = (2 * X + 1) * n - N;
        if (num <= 0) { return [[0, D]]; }
        if (num >= (n - 1) * D) { return [[n - 1, D]]; }
        const i = Math.floor(num / D), f = num % D;
        return [[i, D - f], [i + 1, f]];
    }
    const out = [];
    for (let j = Math.floor(X * n / N); j <= Math.floor(((X + 1) * n - 1) / N); j++) { out.push([j, Math.min((X + 1) * n, (j + 1) * N) - Math.max(X * n, j * N)]); }
    return out;
}
function bruteForce(texels, size, target, channels) {
    const [nx, ny, nz] = size, [NX, NY, NZ] = target;
    const S = BigInt(NX >= nx ? 2 * NX : nx) * BigInt(NY >= ny ? 2 * NY : ny) * BigInt(NZ >= nz ? 2 * NZ : nz);
    const out = new texels.constructor(NX * NY * NZ * channels);
    for (let Z = 0; Z < NZ; Z++) { for (let Y = 0; Y < NY; Y++) { for (let X = 0; X < NX; X++) { for (let c = 0; c < channels; c++) {
        let sum = 0n;
        for (const [z, wz] of taps(nz, NZ, Z)) { for (const [y, wy] of taps(ny, NY, Y)) { for (const [x, wx] of taps(nx, NX, X)) {
            sum += BigInt(wz) * BigInt(wy) * BigInt(wx) * BigInt(texels[((z * ny + y) * nx + x) * channels + c]);
        } } }
        out[((Z * NY + Y) * NX + X) * channels + c] = Number((2n * sum + S) / (2n * S));
    } } } }
    return out;
}

// ---- the checks
if (r.checkResampleMode('nearest') !== 0 || r.checkResampleMode('filtered') !== 1) { throw new Error('mode codes'); }
for (const bad of [0, 1, 'linear', null, undefined, true]) { throws(() => r.checkResampleMode(bad), 'mode ' + JSON.stringify(bad), /resample mode is 'filtered' or 'nearest'/); }
equal(r.checkResampleSize(1, 4096, 7), [1, 4096, 7], 'size');
for (const [bad, axis] of [[[0, 1, 1], 'x'], [[1, 4097, 1], 'y'], [[1, 1, 1.5], 'z'], [[1, 1, '2'], 'z'], [[null, 1, 1], 'x'], [[1, true, 1], 'y'], [[-3, 1, 1], 'x']]) {
    throws(() => r.checkResampleSize(bad[0], bad[1], bad[2]), 'size ' + JSON.stringify(bad), new RegExp('along ' + axis));
}
equal(r.isotropicShape([512, 512, 200], [0.7, 0.7, 2.0]), [512, 512, 571], 'isotropic CT');
equal(r.isotropicShape([512, 512, 200], [0.7, 0.7, 2.0], 1.4), [256, 256, 286], 'pitch given');
equal(r.isotropicShape([3, 3, 3], [1, 1, 0.01], 1), [3, 3, 1], 'at least one voxel');
equal(r.isotropicShape([4096, 1, 1], [1, 1, 1]), [4096, 1, 1], 'the limit');
throws(() => r.isotropicShape([4097, 1, 1], [1, 1, 1]), 'a source of 4097', /along x/);
throws(() => r.isotropicShape([10, 10, 2049], [1, 1, 2]), 'a result of 4098', /along z/);
throws(() => r.isotropicShape([10, 241, 10], [1, 17, 1], 1), 'a result of 4097', /along y/);
for (const bad of [[0, 1, 1], [1, -1, 1], [1, 1, NaN], [Infinity, 1, 1], [1, '1', 1], [1, 1], null, 'abc']) {
    throws(() => r.isotropicShape([4, 4, 4], bad), 'spacing ' + JSON.stringify(bad), /spacing/);
}
for (const bad of [0, -1, NaN, Infinity, '1']) { throws(() => r.isotropicShape([4, 4, 4], [1, 1, 1], bad), 'pitch ' + JSON.stringify(bad), /pitch/); }
throws(() => r.resampleTexels(new Float32Array(8), [2, 2, 2], [2, 2, 2]), 'float texels, filtered');
throws(() => r.resampleTexels(new Int8Array(8), [2, 2, 2], [2, 2, 2], 'filtered'), 'signed texels, filtered');
throws(() => r.resampleTexels(new Uint8Array(7), [2, 2, 2], [2, 2, 2]), 'too few texels');
throws(() => r.resampleTexels(new Uint8Array(8), [2, 2, 2], [2, 2, 0]), 'a target of 0');
throws(() => r.resampleTexels(new Uint8Array(8), [2, 2, 2], [2, 2, 2], 'cubic'), 'an unknown mode');

// ---- the taps: positive weights that sum to S
for (let n = 1; n <= 24; n++) {
    for (let N = 1; N <= 24; N++) {
        const t = r.axisTaps(n, N), near = r.nearestIndex(n, N);
        if (t.S !== (N >= n ? 2 * N : n) || t.taps.length !== N) { throw new Error(`S of ${n} -> ${N}`); }
        for (let X = 0; X < N; X++) {
            let sum = 0;
            for (const [j, w] of t.taps[X]) { if (!(w > 0 && j >= 0 && j < n)) { throw new Error(`tap of ${n} -> ${N} at ${X}`); } sum += w; }
            if (sum !== t.S) { throw new Error(`weights of ${n} -> ${N} at ${X} sum to ${sum}`); }
            if (!(near[X] >= 0 && near[X] < n && (X === 0 || near[X] >= near[X - 1]))) { throw new Error(`nearest index of ${n} -> ${N} at ${X}`); }
        }
    }
}

// ---- the option
if (RenderingContext._resampleSpec(null) !== null || RenderingContext._resampleSpec(undefined) !== null) { throw new Error('no option'); }
let filled = RenderingContext._resampleSpec({ size: [3, 4, 5] });
if (JSON.stringify(filled) !== JSON.stringify({ size: [3, 4, 5], spacing: null, pitch: null, mode: 'filtered' })) { throw new Error('defaults: ' + JSON.stringify(filled)); }
filled = RenderingContext._resampleSpec({ spacing: [0.7, 0.7, 2], mode: 'nearest' });
if (JSON.stringify(filled) !== JSON.stringify({ size: null, spacing: [0.7, 0.7, 2], pitch: 0.7, mode: 'nearest' })) { throw new Error('spacing: ' + JSON.stringify(filled)); }
if (RenderingContext._resampleSpec({ spacing: [1, 1, 2], pitch: 0.5 }).pitch !== 0.5) { throw new Error('pitch'); }
for (const bad of ['filtered', [3, 4, 5], {}, { mode: 'nearest' }, { size: [3, 4, 5], spacing: [1, 1, 1] }, { size: [3, 4] }, { size: [0, 4, 5] }, { size: [3, 4, 4097] },
    { size: [3, 4, 5], pitch: 1 }, { size: [3, 4, 5], mode: 'linear' }, { spacing: [1, 1, 0] }, { spacing: [1, 1, NaN] }, { spacing: [1, 1] }, { spacing: [1, 1, 1], pitch: 0 },
    { spacing: [1, 1, 1], pitch: -2 }, { size: [3, 4, 5], factor: 2 }]) {
    throws(() => new RenderingContext({ resample: bad }), 'RenderingContext({ resample: ' + JSON.stringify(bad) + ' })');
}

// ---- the twin
let seed = 13579;
const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
let ties = 0;
for (const size of [[7, 6, 5], [1, 1, 1]]) {
    for (const target of [[7, 6, 5], [1, 1, 1], [5, 2, 3], [14, 12, 10], [7, 9, 2], [3, 4, 11]]) {
        for (const bits of [8, 16]) {
            for (const channels of [1, 2]) {
                const M = bits === 8 ? 255 : 65535, texels = new (bits === 8 ? Uint8Array : Uint16Array)(size[0] * size[1] * size[2] * channels);
                for (let i = 0; i < texels.length; i++) { texels[i] = rand() & M; }
                const what = `${size} -> ${target}, ${bits} bits, ${channels} channels`;
                equal(r.resampleTexels(texels, size, target, 'filtered', channels), bruteForce(texels, size, target, channels), what);
                ties += r.countTies(texels, size, target, channels);
                const near = r.resampleTexels(texels, size, target, 'nearest', channels);
                const ix = r.nearestIndex(size[0], target[0]), iy = r.nearestIndex(size[1], target[1]), iz = r.nearestIndex(size[2], target[2]);
                for (let i = 0; i < near.length; i++) {
                    const c = i % channels, X = Math.floor(i / channels) % target[0], Y = Math.floor(i / (channels * target[0])) % target[1], Z = Math.floor(i / (channels * target[0] * target[1]));
                    if (near[i] !== texels[((iz[Z] * size[1] + iy[Y]) * size[0] + ix[X]) * channels + c]) { throw new Error('nearest ' + what); }
                }
            }
        }
    }
}
if (ties < 1) { throw new Error('no exact halves among the cases: the rounding rule is not exercised'); }
// NaN payloads survive NEAREST
const f = new Float32Array(2); new Uint32Array(f.buffer).set([0x7FC12345, 0xFF800001]);
equal(new Uint32Array(r.resampleTexels(f, [2, 1, 1], [4, 1, 1], 'nearest').buffer), [0x7FC12345, 0x7FC12345, 0xFF800001, 0xFF800001], 'NaN payloads');

if (process.argv.length > 2) {
    const [path, nx, ny, nz, bits, channels, tx, ty, tz] = [process.argv[2]].concat(process.argv.slice(3).map(Number));
    const raw = fs.readFileSync(path);
    const texels = bits === 8 ? new Uint8Array(raw) : new Uint16Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length));
    console.log(JSON.stringify({ filtered: Array.from(r.resampleTexels(texels, [nx, ny, nz], [tx, ty, tz], 'filtered', channels)),
        nearest: Array.from(r.resampleTexels(texels, [nx, ny, nz], [tx, ty, tz], 'nearest', channels)), ties: r.countTies(texels, [nx, ny, nz], [tx, ty, tz], channels) }));
}
console.log('js resample host ok');
