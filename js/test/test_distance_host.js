'use strict';
// node js/test/test_distance_host.js [TEXELS NX NY NZ BITS LO HI] — no device: the argument checks of js/vpt/distance.js, the option
// validation of RenderingContext and the plain-JS twins against a brute force over every pair (voxel, seed).  With arguments, the twins of
// the texels in the file TEXELS are printed as one JSON line (tests/test_distance_host.py compares them with the numpy statement).
const fs = require('fs');
const d = require('../vpt/distance.js');
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
function bruteForce(texels, nx, ny, nz, lo, hi, rest) {
    const n = nx * ny * nz, out = new Uint32Array(n).fill(0xFFFFFFFF);
    for (let i = 0; i < n; i++) {
        const x = i % nx, y = Math.floor(i / nx) % ny, z = Math.floor(i / (nx * ny));
        for (let j = 0; j < n; j++) {
            if ((texels[j] >= lo && texels[j] <= hi) === rest) { continue; }
            const a = j % nx - x, b = Math.floor(j / nx) % ny - y, c = Math.floor(j / (nx * ny)) - z;
            out[i] = Math.min(out[i], a * a + b * b + c * c);
        }
    }
    return out;
}

// ---- the checks
if (d.checkSeeds('range') !== 0 || d.checkSeeds('rest') !== 1) { throw new Error('seed codes'); }
for (const bad of [0, 1, 'both', null, undefined, true]) { throws(() => d.checkSeeds(bad), 'seeds ' + JSON.stringify(bad), /seeds is 'range' or 'rest'/); }
if (d.checkSteps(1) !== 1 || d.checkSteps(256) !== 256) { throw new Error('steps'); }
for (const bad of [0, 257, -1, 1.5, '1', null, true]) { throws(() => d.checkSteps(bad), 'steps ' + JSON.stringify(bad), /steps/); }
if (d.checkRadius(0) !== 0 || d.checkRadius(2.5) !== 6 || d.checkRadius(Math.sqrt(2)) !== 2 || d.checkRadius(3) !== 9 || d.checkRadius(65535.9) !== 4294954188 || d.checkRadius(65536) !== 4294967294 || d.checkRadius(1e200) !== 4294967294) { throw new Error('radius'); }
for (const bad of [-1, NaN, Infinity, '2', null, true]) { throws(() => d.checkRadius(bad), 'radius ' + JSON.stringify(bad), /radius/); }
equal(d.checkWithin(0, null, 0, 255), [0, 0xFFFFFFFF, 0], 'within defaults');
for (const bad of [[2, 1, 0], [-1, 1, 0], [0, 0x100000000, 0], [0, 1, 256], [0, 1, -1], [0.5, 1, 0], [0, 1, null]]) {
    throws(() => d.checkWithin(bad[0], bad[1], bad[2], 255), 'within ' + JSON.stringify(bad));
}
for (const bad of [[2, 1], [0, 256], [-1, 5], [0.5, 1], [0, null]]) { throws(() => d.checkDistanceRange(bad[0], bad[1], 255), 'range ' + JSON.stringify(bad), /distance range/); }
throws(() => d.distanceSquaredTexels(new Float32Array(8), 2, 2, 2, 0, 1), 'float texels');
throws(() => d.distanceSquaredTexels(new Uint8Array(7), 2, 2, 2, 0, 1), 'too few texels');

// ---- the option
const good = { lo: 0, hi: 1, mode: 'within' };
if (RenderingContext._distanceSpec(null) !== null || RenderingContext._distanceSpec(undefined) !== null) { throw new Error('no option'); }
const filled = RenderingContext._distanceSpec(good);
if (JSON.stringify(filled) !== JSON.stringify({ lo: 0, hi: 1, seeds: 'range', mode: 'within', from: 0, to: 0xFFFFFFFF, fill: 0, steps: 1 })) { throw new Error('defaults: ' + JSON.stringify(filled)); }
if (RenderingContext._distanceSpec({ lo: 3, hi: 65535, seeds: 'rest', mode: 'channel', steps: 256 }).steps !== 256) { throw new Error('channel'); }
for (const bad of ['within', [0, 1], { lo: 0, hi: 1 }, { lo: 0, mode: 'within' }, Object.assign({}, good, { mode: 'margin' }), Object.assign({}, good, { lo: 2 }),
    Object.assign({}, good, { hi: 65536 }), Object.assign({}, good, { seeds: 'both' }), Object.assign({}, good, { from: 5, to: 4 }), Object.assign({}, good, { fill: 65536 }),
    Object.assign({}, good, { steps: 2 }), Object.assign({}, good, { mode: 'channel', steps: 0 }), Object.assign({}, good, { mode: 'channel', steps: 257 }),
    Object.assign({}, good, { mode: 'channel', fill: 1 }), Object.assign({}, good, { mode: 'channel', to: 9 }), Object.assign({}, good, { radius: 2 })]) {
    throws(() => new RenderingContext({ distance: bad }), 'RenderingContext({ distance: ' + JSON.stringify(bad) + ' })');
}
const channel = { lo: 0, hi: 1, mode: 'channel' };
throws(() => new RenderingContext({ distance: channel, gradient: 'sobel' }), 'channel with gradient', /second channel/);
throws(() => new RenderingContext({ distance: channel, components: { lo: 0, hi: 1, mode: 'label' } }), 'channel with label', /second channel/);

// ---- the twins
let seed = 24680;
const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
for (const [nx, ny, nz] of [[7, 5, 3], [1, 1, 1], [9, 1, 2], [1, 6, 1]]) {
    for (const bits of [8, 16]) {
        const M = bits === 8 ? 255 : 65535, texels = new (bits === 8 ? Uint8Array : Uint16Array)(nx * ny * nz);
        for (let i = 0; i < texels.length; i++) { texels[i] = rand() & M; }
        for (const [lo, hi] of [[0, M >> 3], [M >> 1, M], [0, M]]) {
            for (const seeds of ['range', 'rest']) {
                const d2 = d.distanceSquaredTexels(texels, nx, ny, nz, lo, hi, seeds);
                equal(d2, bruteForce(texels, nx, ny, nz, lo, hi, seeds === 'rest'), `d2 ${nx} x ${ny} x ${nz}, ${bits} bits, [${lo}, ${hi}], ${seeds}`);
            }
        }
    }
}
for (const p of [0, 1, 2, 3, 4, 8, 9, 4095 * 4095 * 65536 - 1, 4095 * 4095 * 65536, 4095 * 4095 * 65536 + 1, 0xFFFFFFFF * 65536]) {
    const r = d.isqrt(p);
    if (!(r * r <= p && (r + 1) * (r + 1) > p)) { throw new Error('isqrt(' + p + ') = ' + r); }
}
equal(d.channelTexels(new Uint8Array([7, 8, 9, 10]), new Uint32Array([0, 3, 4, 0xFFFFFFFF]), 2), [7, 0, 8, 3, 9, 4, 10, 255], 'channel');
equal(d.withinTexels(new Uint8Array([7, 8, 9, 10]), new Uint32Array([0, 3, 4, 0xFFFFFFFF]), 3, 4, 1), [1, 8, 9, 1], 'within');
equal(d.withinTexels(new Uint8Array([7, 8, 9, 10]), new Uint32Array([0, 3, 4, 0xFFFFFFFF]), 4), [0, 0, 9, 10], 'within to the end');

if (process.argv.length > 2) {
    const [path, nx, ny, nz, bits, lo, hi] = [process.argv[2]].concat(process.argv.slice(3).map(Number));
    const raw = fs.readFileSync(path);
    const texels = bits === 8 ? new Uint8Array(raw) : new Uint16Array(raw.buffer, raw.byteOffset, raw.length / 2);
    const out = {};
    for (const seeds of ['range', 'rest']) {
        const d2 = d.distanceSquaredTexels(texels, nx, ny, nz, lo, hi, seeds);
        out[seeds] = { d2: Array.from(d2), within: Array.from(d.withinTexels(texels, d2, 2, 9, 5)), channel: Array.from(d.channelTexels(texels, d2, 7)) };
    }
    console.log(JSON.stringify(out));
}
console.log('js distance host ok');
