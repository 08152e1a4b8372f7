'use strict';
// node js/test/test_skeleton_host.js [TEXELS NX NY NZ BITS LO HI] — no device: the plain-JS statement of the thinning contract
// (js/vpt/skeleton.js): neighbourhoods with known C and B, the order of the visits inside a sub-step, the shapes with known answers (a ball,
// a line, a single voxel, the empty range), the burn passes as the history of the erosion, refusals, the `skeleton` option of
// RenderingContext.  With arguments, the burn passes and the info of the texels in the file TEXELS (BITS bits a voxel) for the three modes,
// to the fixed point and capped at two passes, are printed as one JSON line (tests/test_skeleton_host.py compares it with the numpy statement).
const fs = require('fs');
const k = require('../vpt/skeleton.js');
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
function check(cond, what) { if (!cond) { throw new Error(what); } }
const MODES = ['kernel', 'ends', 'isthmus'];

// ---- neighbourhoods
const bit = (dx, dy, dz) => 1 << (9 * (dz + 1) + 3 * (dy + 1) + (dx + 1));
const full = (1 << 27) - 1 - (1 << 13);
const cb = (obj, c, b, what) => { const t = k.skeletonTopology(obj); check(t[0] === c && t[1] === b, `${what}: (C, B) = (${t}), expected (${c}, ${b})`); };
cb(0, 0, 1, 'an isolated voxel');
cb(full, 1, 0, 'an interior voxel');
cb(bit(1, 0, 0), 1, 1, 'a curve end');
cb(bit(1, 0, 0) | bit(-1, 0, 0), 2, 1, 'the middle of a line');
cb(full & ~bit(0, 0, 1), 1, 1, 'a voxel of a flat face');
cb(full & ~bit(0, 0, 1) & ~bit(0, 0, -1), 1, 2, 'a voxel of a sheet between two cavities');
cb(full & ~bit(0, 0, 1) & ~bit(1, 0, 0), 1, 2, 'two background faces apart');
cb(full & ~bit(0, 0, 1) & ~bit(1, 0, 0) & ~bit(1, 0, 1), 1, 1, 'two background faces joined through an edge');

// ---- random volumes: the order of the visits changes nothing; value >= k is the object after k - 1 passes
let seed = 1357;
const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
for (const [nx, ny, nz] of [[1, 1, 1], [9, 1, 1], [7, 5, 3], [12, 11, 9]]) {
    const a = new Uint8Array(nx * ny * nz);
    for (let i = 0; i < a.length; i++) { a[i] = rand() % 10 < 6 ? 100 + rand() % 100 : rand() % 100; }
    for (const mode of MODES) {
        const what = `${nx}x${ny}x${nz} ${mode}`;
        const one = k.skeletonBurnTexels(a, nx, ny, nz, 100, 255, mode), two = k.skeletonBurnTexels(a, nx, ny, nz, 100, 255, mode, 0, 'reversed');
        same(one.burn, two.burn, what + ': reversed order');
        check(JSON.stringify(one.info) === JSON.stringify(two.info), what + ': reversed order, info');
        check(one.info.converged === 1 && one.info.isolated + one.info.ends + one.info.regular + one.info.junctions === one.info.kept_voxels, what + ': info');
        for (let cap = 1; cap <= one.info.passes; cap++) {
            const capped = k.skeletonBurnTexels(a, nx, ny, nz, 100, 255, mode, cap);
            for (let i = 0; i < a.length; i++) {
                check((capped.burn[i] === k.THIN_KEPT) === (one.burn[i] >= cap + 1), `${what}: capped at ${cap}, voxel ${i}`);
            }
            check(capped.info.passes === cap && capped.info.converged === (cap === one.info.passes ? 1 : 0), `${what}: capped at ${cap}, info`);
        }
        same(k.skeletonTexels(a, nx, ny, nz, 100, 255, mode, 0, 7), k.burnWithinTexels(a, one.burn, k.THIN_KEPT, null, 7), what + ': skeletonTexels');
    }
}

// ---- shapes
{
    const n = 20, a = new Uint8Array(n * n * n);
    let voxels = 0;
    for (let z = 0, i = 0; z < n; z++) { for (let y = 0; y < n; y++) { for (let x = 0; x < n; x++, i++) {
        if ((x - 9.5) ** 2 + (y - 9.5) ** 2 + (z - 9.5) ** 2 <= 49) { a[i] = 200; voxels++; }
    } } }
    check(voxels === 1472, 'the ball has 1472 voxels');
    for (const mode of ['kernel', 'isthmus']) {
        const info = k.skeletonBurnTexels(a, n, n, n, 100, 255, mode).info;
        check(info.kept_voxels === 1 && info.passes === 8 && info.isolated === 1, 'the ball in ' + mode + ': ' + JSON.stringify(info));
    }
    const info = k.skeletonBurnTexels(a, n, n, n, 100, 255, 'ends').info;
    check(info.kept_voxels === 3 && info.ends === 2 && info.regular === 1, 'the ball in ends: ' + JSON.stringify(info));
    const line = new Uint8Array(n * n * n);
    for (let x = 3; x < 17; x++) { line[(7 * n + 11) * n + x] = 9; }
    const kept = k.skeletonBurnTexels(line, n, n, n, 9, 9, 'ends');
    check(kept.info.kept_voxels === 14 && kept.info.ends === 2 && kept.info.passes === 1, 'a line in ends: ' + JSON.stringify(kept.info));
    check(k.skeletonBurnTexels(line, n, n, n, 9, 9, 'kernel').info.kept_voxels === 1, 'a line in kernel');
}
for (const mode of MODES) {
    const one = k.skeletonBurnTexels(new Uint16Array([700]), 1, 1, 1, 700, 700, mode);
    check(one.burn[0] === k.THIN_KEPT && one.info.passes === 1 && one.info.isolated === 1 && one.info.kept_voxels === 1, 'a single voxel in ' + mode);
    const none = k.skeletonBurnTexels(new Uint8Array(24).fill(3), 4, 3, 2, 4, 9, mode, 5);
    check(none.burn.every(v => v === 0) && none.info.passes === 0 && none.info.converged === 1 && none.info.object_voxels === 0, 'the empty range in ' + mode);
}
check(k.skeletonBurnTexels(new Uint8Array(210).fill(9), 7, 6, 5, 9, 9, 'kernel').info.kept_voxels === 1, 'a volume that is all object');

// ---- refusals
const a = new Uint8Array(24).fill(9);
throws(() => k.skeletonBurnTexels(a, 4, 3, 2, 3, 2, 'ends'), 'lo above hi', /skeleton range/);
throws(() => k.skeletonBurnTexels(a, 4, 3, 2, 0, 256, 'ends'), 'hi above M', /skeleton range/);
throws(() => k.skeletonBurnTexels(a, 4, 3, 2, 1.5, 2, 'ends'), 'a fractional lo', /integer/);
throws(() => k.skeletonBurnTexels(a, 4, 3, 2, 1, 2, 'curve'), 'an unknown mode', /mode/);
throws(() => k.skeletonBurnTexels(a, 4, 3, 2, 1, 2, 1), 'a numeric mode', /mode/);
throws(() => k.skeletonBurnTexels(a, 4, 3, 2, 1, 2, 'ends', -1), 'negative passes', /passes/);
throws(() => k.skeletonBurnTexels(a, 4, 3, 2, 1, 2, 'ends', 0, 'random'), 'an unknown order', /order/);
throws(() => k.skeletonBurnTexels(a, 4, 3, 3, 1, 2, 'ends'), 'a wrong size', /texels/);
throws(() => k.skeletonBurnTexels(new Float32Array(24), 4, 3, 2, 1, 2, 'ends'), 'floats', /texels/);
throws(() => k.burnWithinTexels(a, new Uint32Array(24), 5, 4), 'from above to', /burn passes/);
throws(() => k.burnWithinTexels(a, new Uint32Array(24), 1, null, 256), 'fill above M', /fill/);
throws(() => k.burnWithinTexels(a, new Uint32Array(5)), 'a wrong burn size', /burn passes/);

// ---- the option: every refusal comes before the context opens a device
for (const bad of ['skeleton', {}, { lo: 1 }, { lo: 2, hi: 1 }, { lo: 1, hi: 2, mode: 'curve' }, { lo: 1, hi: 2, passes: -1 }, { lo: 1, hi: 2, passes: 1.5 },
    { lo: 1, hi: 2, fill: -1 }, { lo: 1, hi: 2, fill: 65536 }, { lo: 1, hi: 2, steps: 2 }, { lo: 1, hi: 65536 }, [1, 2]]) {
    throws(() => new RenderingContext({ skeleton: bad }), 'skeleton ' + JSON.stringify(bad));
}
for (const other of ['distance', 'thickness']) {
    const options = { skeleton: { lo: 100, hi: 255 } };
    options[other] = { lo: 1, hi: 2, mode: 'within' };
    throws(() => new RenderingContext(options), 'skeleton with ' + other, new RegExp("skeleton and " + other + " mode 'within' .*name one of them"));
}
check(JSON.stringify(k.checkSkeleton({ lo: 100, hi: 255 })) === JSON.stringify({ lo: 100, hi: 255, mode: 'ends', passes: 0, fill: 0 }), 'the defaults of the skeleton option');
check(k.checkSkeleton(null) === null && k.checkSkeleton(undefined) === null, 'no skeleton option');

if (process.argv.length > 2) {
    const [path, nx, ny, nz, bits, lo, hi] = [process.argv[2]].concat(process.argv.slice(3, 9).map(Number));
    const bytes = fs.readFileSync(path);
    const texels = bits === 8 ? new Uint8Array(bytes.buffer, bytes.byteOffset, nx * ny * nz) : new Uint16Array(new Uint8Array(bytes).buffer, 0, nx * ny * nz);
    const out = {};
    for (const mode of MODES) {
        for (const passes of [0, 2]) {
            const found = k.skeletonBurnTexels(texels, nx, ny, nz, lo, hi, mode, passes);
            out[mode + ' ' + passes] = { burn: Array.from(found.burn), info: found.info };
        }
    }
    console.log(JSON.stringify(out));
}
console.log('js skeleton host ok');
