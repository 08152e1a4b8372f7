'use strict';
// node js/test/test_thickness_host.js [TEXELS NX NY NZ BITS LO HI] — no device: the plain-JS statement of local thickness
// (js/vpt/thickness.js) against a loop over voxels and centres, the plates' closed form, no seed and all seeds, the `thickness` option of
// RenderingContext.  With arguments, T2 of the texels in the file TEXELS (BITS bits a voxel) for both seed modes is printed as one JSON line
// (tests/test_thickness_host.py compares it with the numpy statement).
const fs = require('fs');
const t = require('../vpt/thickness.js');
const d = require('../vpt/distance.js');
const { RenderingContext } = require('../vpt/RenderingContext.js');

function throws(f, what, pattern) {
    let message = null;
    try { f(); } catch (e) { message = e.message; }
    if (message === null) { throw new Error(what + ' was accepted'); }
    if (pattern && !pattern.test(message)) { throw new Error(what + ': unexpected message ' + message); }
}
function same(a, b, what) {
    if (a.length !== b.length) { throw new Error(what + ': wrong length'); }
    for (let i = 0; i < a.length; i++) { if (a[i] !== b[i]) { throw new Error(`${what}: element ${i} is ${a[i]}, expected ${b[i]}`); } }
}
// the contract read voxel by voxel: the largest D(c) over the centres c with |v - c|^2 < D(c)
function brute(d2, nx, ny, nz) {
    const out = new Uint32Array(d2.length);
    for (let v = 0; v < d2.length; v++) {
        const vx = v % nx, vy = Math.floor(v / nx) % ny, vz = Math.floor(v / (nx * ny));
        for (let c = 0; c < d2.length; c++) {
            const cx = c % nx, cy = Math.floor(c / nx) % ny, cz = Math.floor(c / (nx * ny));
            if (d2[c] > out[v] && (vx - cx) ** 2 + (vy - cy) ** 2 + (vz - cz) ** 2 < d2[c]) { out[v] = d2[c]; }
        }
    }
    return out;
}

// ---- random blobs, both seed modes
let seed = 2468;
const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
for (const [nx, ny, nz] of [[1, 1, 1], [9, 1, 1], [7, 5, 3], [11, 8, 6], [5, 13, 9]]) {
    const n = nx * ny * nz, a = new Uint8Array(n);
    for (let b = 0; b < 4; b++) {
        const cx = rand() % nx, cy = rand() % ny, cz = rand() % nz, r2 = (1 + rand() % 4) ** 2;
        for (let i = 0; i < n; i++) {
            if ((i % nx - cx) ** 2 + (Math.floor(i / nx) % ny - cy) ** 2 + (Math.floor(i / (nx * ny)) - cz) ** 2 <= r2) { a[i] = 200; }
        }
    }
    for (const seeds of ['rest', 'range']) {
        const d2 = d.distanceSquaredTexels(a, nx, ny, nz, 100, 255, seeds);
        if (d2[0] === d.DISTANCE_NONE) { continue; }
        const t2 = t.thicknessSquaredTexels(d2, nx, ny, nz);
        same(t2, brute(d2, nx, ny, nz), `${nx}x${ny}x${nz} ${seeds}`);
        let largestD = 0, largestT = 0;
        for (let i = 0; i < n; i++) {
            if (t2[i] < d2[i] || (t2[i] === 0) !== (d2[i] === 0)) { throw new Error('T2 >= D, and 0 exactly where D is 0'); }
            largestD = Math.max(largestD, d2[i]); largestT = Math.max(largestT, t2[i]);
        }
        if (largestD !== largestT) { throw new Error('max T2 = max D'); }
    }
}

// ---- plates: w voxels thick, spanning the volume: ceil(w / 2)^2 on the plate, 0 off it
for (const w of [1, 2, 5, 6]) {
    const nx = 7, ny = 9, nz = 8, a = new Uint8Array(nx * ny * nz), want = new Uint32Array(a.length);
    for (let i = 0; i < a.length; i++) {
        const y = Math.floor(i / nx) % ny;
        if (y >= 1 && y < 1 + w) { a[i] = 255; want[i] = Math.ceil(w / 2) ** 2; }
    }
    same(t.thicknessSquaredTexels(d.distanceSquaredTexels(a, nx, ny, nz, 1, 255, 'rest'), nx, ny, nz), want, 'plate ' + w);
    const pair = t.thicknessTexels(a, nx, ny, nz, 1, 255);                                // steps 2: the diameter, 2 ceil(w / 2)
    for (let i = 0; i < a.length; i++) { if (pair[2 * i] !== a[i] || pair[2 * i + 1] !== (a[i] ? 2 * Math.ceil(w / 2) : 0)) { throw new Error('plate ' + w + ': the pair'); } }
    const opened = t.openBallTexels(a, nx, ny, nz, 1, 255, Math.ceil(w / 2), 3);          // no ball of a radius above ceil(w / 2) fits
    if (!opened.every(c => c === 3)) { throw new Error('plate ' + w + ': opened by too large a ball'); }
    same(t.openBallTexels(a, nx, ny, nz, 1, 255, Math.ceil(w / 2) - 0.5), a, 'plate ' + w + ': opened by a ball that fits');
}

// ---- no seed, all seeds, refusals
const full = new Uint8Array(24).fill(9);
same(t.thicknessSquaredTexels(d.distanceSquaredTexels(full, 4, 3, 2, 1, 255, 'rest'), 4, 3, 2), new Uint32Array(24).fill(d.DISTANCE_NONE), 'no seed');
same(t.thicknessSquaredTexels(d.distanceSquaredTexels(full, 4, 3, 2, 1, 255, 'range'), 4, 3, 2), new Uint32Array(24), 'all seeds');
throws(() => t.thicknessSquaredTexels(new Uint32Array(5), 2, 2, 2), 'a wrong size', /squared distances/);
throws(() => t.thicknessSquaredTexels(new Float64Array(8), 2, 2, 2), 'floats', /squared distances/);
throws(() => t.thicknessSquaredTexels(new Uint32Array([1, 0, d.DISTANCE_NONE, 1]), 4, 1, 1), 'NONE among finite values', /NONE/);
throws(() => t.openBallTexels(full, 4, 3, 2, 1, 255, -1), 'a negative radius', /radius/);
throws(() => t.openBallTexels(full, 4, 3, 2, 1, 255, 1, 256), 'fill above M', /fill/);
throws(() => t.thicknessTexels(full, 4, 3, 2, 1, 255, 0), 'steps 0', /steps/);

// ---- the option: every refusal comes before the context opens a device
const ok = { lo: 100, hi: 255, mode: 'channel' };
for (const bad of ['thickness', {}, { lo: 1, hi: 2 }, { lo: 2, hi: 1, mode: 'within' }, { lo: 1, hi: 2, mode: 'both' }, { lo: 1, hi: 2, mode: 'within', steps: 2 },
    { lo: 1, hi: 2, mode: 'channel', from: 3 }, { lo: 1, hi: 2, mode: 'channel', steps: 0 }, { lo: 1, hi: 2, mode: 'within', seeds: 'all' },
    { lo: 1, hi: 2, mode: 'within', radius: 3 }, [1, 2]]) {
    throws(() => new RenderingContext({ thickness: bad }), 'thickness ' + JSON.stringify(bad));
}
throws(() => new RenderingContext({ thickness: ok, distance: { lo: 1, hi: 2, mode: 'within' } }), 'distance and thickness', /name one of them/);
for (const other of [{ gradient: 'central' }, { components: { lo: 1, hi: 2, mode: 'label' } }, { combine: { reader: {}, op: 'pair' } }, { split: { lo: 1, hi: 2 } }]) {
    throws(() => new RenderingContext(Object.assign({ thickness: ok }, other)), 'thickness channel with ' + JSON.stringify(other), /both write the second channel/);
}
const spec = RenderingContext._distanceSpec({ lo: 1, hi: 2, mode: 'channel' }, 'thickness');
if (spec.seeds !== 'rest' || spec.steps !== 2) { throw new Error('the defaults of the thickness option'); }

if (process.argv.length > 2) {
    const [path, nx, ny, nz, bits, lo, hi] = [process.argv[2]].concat(process.argv.slice(3, 9).map(Number));
    const bytes = fs.readFileSync(path);
    const texels = bits === 8 ? new Uint8Array(bytes.buffer, bytes.byteOffset, nx * ny * nz) : new Uint16Array(new Uint8Array(bytes).buffer, 0, nx * ny * nz);
    const out = {};
    for (const seeds of ['rest', 'range']) {
        out[seeds] = Array.from(t.thicknessSquaredTexels(d.distanceSquaredTexels(texels, nx, ny, nz, lo, hi, seeds), nx, ny, nz));
    }
    console.log(JSON.stringify(out));
}
console.log('js thickness host ok');
