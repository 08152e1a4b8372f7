'use strict';
// node js/test/test_combine_host.js [A B NX NY NZ BITS] — no device: the argument checks of js/vpt/combine.js, the option validation of
// RenderingContext and the plain-JS twin against the contract written out once more, texel by texel in BigInt.  With arguments, the twin of
// the texels in the files A (one channel) and B (two channels, BITS bits each) is printed as one JSON line (tests/test_combine_host.py
// compares it with the numpy statement).
const fs = require('fs');
const c = require('../vpt/combine.js');
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
function blends(M) {
    return [[256, 256, 0], [256, -256, 0], [256, -256, (M + 1) / 2], [128, 128, 0], [512, -256, 0], [-256, 0, M], [4096, 4096, -M], [-4096, -4096, M], [77, 151, 3], [0, 256, 0]];
}
// floor(x / 256 + 1 / 2) in BigInt, which has no shift to be wrong about
function blendOne(A, B, wa, wb, offset, M) {
    const x = BigInt(wa) * BigInt(A) + BigInt(wb) * BigInt(B) + 128n;
    let q = x / 256n;                                              // truncates
    if (x < 0n && q * 256n !== x) { q -= 1n; }
    const s = q + BigInt(offset);
    return Number(s < 0n ? 0n : s > BigInt(M) ? BigInt(M) : s);
}

// ---- the checks
equal(['mask', 'min', 'max', 'absdiff', 'blend', 'pair'].map(c.checkCombineOp), [0, 1, 2, 3, 4, 5], 'op codes');
for (const bad of ['mean', 0, null, undefined]) { throws(() => c.checkCombineOp(bad), 'op ' + JSON.stringify(bad), /combine op is/); }
for (const bad of [[4097, 0, 0], [0, -4097, 0], [1.5, 0, 0], [true, 0, 0], ['1', 0, 0], [0, 0, 65536], [0, 0, -65536], [0, 0, null]]) {
    throws(() => c.checkCombineWeights(bad[0], bad[1], bad[2]), 'weights ' + JSON.stringify(bad), /blend (weight|offset)/);
}
equal(c.checkCombineWeights(-4096, 4096, -65535), [-4096, 4096, -65535], 'the limits');
equal(c.checkCombineWeights(1, 2), [1, 2, 0], 'the default offset');
for (const bad of [[1, 1], [2, 2], [-1, 2], [true, 2], ['0', 2]]) { throws(() => c.checkCombineChannel(bad[0], bad[1]), 'channel ' + JSON.stringify(bad), /channel/); }
for (const bad of [{ lo: 3, hi: 2 }, { hi: 256 }, { fill: 256 }, { lo: -1 }, { fill: 1.5 }]) {
    throws(() => c.combineTexels(new Uint8Array(4), new Uint8Array(4), 'mask', bad), 'mask ' + JSON.stringify(bad), /mask/);
}
for (const op of ['min', 'max', 'absdiff', 'blend', 'pair']) { throws(() => c.combineTexels(new Uint8Array(4), new Uint16Array(4), op), op + ' of two widths', /one width/); }
throws(() => c.combineTexels(new Uint8Array(4), new Uint8Array(5), 'min'), 'two sizes', /size/);
throws(() => c.combineTexels(new Float32Array(4), new Uint8Array(4), 'min'), 'float texels');
throws(() => c.combineTexels(new Uint8Array(4), new Uint8Array(4), 'min', { channel: 1 }), 'channel 1 of one', /channel 1/);
for (const bad of [[3, 2], [0], 'ab', [0.5, 1], [-1, 4]]) { throws(() => c.compareStats(new Uint8Array(4), new Uint8Array(4), { aRange: bad }), 'range ' + JSON.stringify(bad), /aRange/); }
// -0.5 -> 0, -1.5 -> -1, the average of 1 and 2 is 2
if (((-128 + 128) >> 8) !== 0 || ((-384 + 128) >> 8) !== -1) { throw new Error('the shift'); }
if (c.combineTexels(new Uint8Array([1]), new Uint8Array([2]), 'blend', { wa: 128, wb: 128 })[0] !== 2) { throw new Error('the average of 1 and 2'); }

// ---- the option
if (RenderingContext._combineSpec(null) !== null || RenderingContext._combineSpec(undefined) !== null) { throw new Error('no option'); }
const reader = {};
let filled = RenderingContext._combineSpec({ reader, op: 'min' });
if (filled.reader !== reader || JSON.stringify(filled) !== JSON.stringify({ reader: {}, volume: null, op: 'min', channel: 0, params: {}, resample: null })) { throw new Error('defaults: ' + JSON.stringify(filled)); }
filled = RenderingContext._combineSpec({ reader, op: 'mask', lo: 1, hi: 300, fill: 9, channel: 1, resample: 'nearest' });
if (JSON.stringify(filled.params) !== JSON.stringify({ lo: 1, hi: 300, fill: 9 }) || filled.channel !== 1 || filled.resample !== 'nearest') { throw new Error('mask: ' + JSON.stringify(filled)); }
if (JSON.stringify(RenderingContext._combineSpec({ reader, op: 'mask' }).params) !== JSON.stringify({ lo: 0, hi: null, fill: 0 })) { throw new Error('mask defaults'); }
if (JSON.stringify(RenderingContext._combineSpec({ reader, op: 'blend', wa: 512, wb: -256 }).params) !== JSON.stringify({ wa: 512, wb: -256, offset: 0 })) { throw new Error('blend'); }
for (const bad of ['mask', {}, { op: 'min' }, { reader }, { reader, volume: reader, op: 'min' }, { volume: reader, op: 'min' }, { reader, op: 'mean' }, { reader, op: 'min', lo: 1 },
    { reader, op: 'mask', wa: 1 }, { reader, op: 'mask', lo: 5, hi: 4 }, { reader, op: 'mask', hi: 65536 }, { reader, op: 'mask', fill: -1 }, { reader, op: 'blend' },
    { reader, op: 'blend', wa: 4097, wb: 0 }, { reader, op: 'blend', wa: 1, wb: 1, offset: 70000 }, { reader, op: 'min', channel: 2 }, { reader, op: 'min', resample: 'cubic' },
    { reader, op: 'min', scale: 2 }]) {
    throws(() => new RenderingContext({ combine: bad }), 'RenderingContext({ combine: ' + JSON.stringify(bad) + ' })');
}
for (const other of [{ gradient: 'sobel' }, { components: { lo: 1, hi: 2, mode: 'label' } }, { distance: { lo: 1, hi: 2, mode: 'channel' } }]) {
    throws(() => new RenderingContext(Object.assign({ combine: { reader, op: 'pair' } }, other)), "'pair' with " + JSON.stringify(other), /second channel/);
}

// ---- the twin
let seed = 24680;
const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
for (const bits of [8, 16]) {
    const M = bits === 8 ? 255 : 65535, T = bits === 8 ? Uint8Array : Uint16Array;
    for (const n of [1, 35, 2415]) {
        for (const ties of [false, true]) {
            const codes = [0, 1, M - 1, M, 0x00FF & M, 0x0100 & M, 0x7FFF & M, 0x8000 & M, 0xFF00 & M];
            const a = new T(n), two = new T(2 * n), b = new T(n);
            for (let i = 0; i < n; i++) { a[i] = ties ? codes[rand() % codes.length] : rand() & M; b[i] = ties ? codes[rand() % codes.length] : rand() & M; two[2 * i] = a[i]; two[2 * i + 1] = b[i]; }
            const what = `${bits} bits, ${n} texels${ties ? ', ties' : ''}`;
            for (const [wa, wb, offset] of blends(M)) {
                const want = new T(n);
                for (let i = 0; i < n; i++) { want[i] = blendOne(a[i], b[i], wa, wb, offset, M); }
                equal(c.combineTexels(a, b, 'blend', { wa, wb, offset }), want, `blend ${wa} ${wb} ${offset}, ${what}`);
                equal(c.combineTexels(a, two, 'blend', { wa, wb, offset, channels: 2, channel: 1 }), want, `blend of channel 1, ${what}`);
            }
            const lo = M >> 2, hi = M - (M >> 2), mask = new T(n), mn = new T(n), mx = new T(n), ad = new T(n), pr = new T(2 * n);
            let sumSq = 0n, sumAbs = 0n, differing = 0n, inB = 0n;
            for (let i = 0; i < n; i++) {
                mask[i] = b[i] >= lo && b[i] <= hi ? a[i] : 7; mn[i] = a[i] < b[i] ? a[i] : b[i]; mx[i] = a[i] < b[i] ? b[i] : a[i]; ad[i] = mx[i] - mn[i]; pr[2 * i] = a[i]; pr[2 * i + 1] = b[i];
                sumSq += BigInt(ad[i]) * BigInt(ad[i]); sumAbs += BigInt(ad[i]); differing += ad[i] ? 1n : 0n; inB += b[i] >= lo && b[i] <= hi ? 1n : 0n;
            }
            equal(c.combineTexels(a, b, 'mask', { lo, hi, fill: 7 }), mask, 'mask, ' + what);
            equal(c.combineTexels(a, b, 'min'), mn, 'min, ' + what); equal(c.combineTexels(a, b, 'max'), mx, 'max, ' + what);
            equal(c.combineTexels(a, b, 'absdiff'), ad, 'absdiff, ' + what); equal(c.combineTexels(a, b, 'pair'), pr, 'pair, ' + what);
            equal(c.combineTexels(a, b, 'mask'), a, 'mask over every code, ' + what);
            equal(c.combineTexels(c.combineTexels(a, a, 'blend', { wa: -256, wb: 0, offset: M }), a, 'blend', { wa: -256, wb: 0, offset: M }), a, 'inversion twice, ' + what);
            const s = c.compareStats(a, two, { channels: 2, channel: 1, bRange: [lo, hi] });
            if (s.voxels !== BigInt(n) || s.sumSq !== sumSq || s.sumAbs !== sumAbs || s.differing !== differing || s.inB !== inB || s.inA !== BigInt(n) || s.both !== inB) { throw new Error('compare, ' + what); }
            if (s.mse !== Number(sumSq) / n && Math.abs(s.mse - Number(sumSq) / n) > 1e-9 * s.mse) { throw new Error('mse, ' + what); }
            if (s.dice !== 2 * Number(inB) / (n + Number(inB))) { throw new Error('dice, ' + what); }
        }
    }
}
// a mask of the other width
equal(c.combineTexels(new Uint8Array([5, 6]), new Uint16Array([300, 20]), 'mask', { lo: 256, hi: 65535, fill: 1 }), [5, 1], 'a 16-bit mask over bytes');
equal(c.combineTexels(new Uint16Array([500, 600]), new Uint8Array([3, 200]), 'mask', { lo: 100, hi: 255, fill: 65535 }), [65535, 600], 'a byte mask over 16 bits');
const none = c.compareStats(new Uint8Array(6), new Uint8Array(6), { aRange: [1, 255], bRange: [1, 255] });
if (none.dice !== null || none.jaccard !== null || none.psnr !== null || none.mse !== 0) { throw new Error('the null ratios'); }

if (process.argv.length > 2) {
    const [pa, pb] = process.argv.slice(2, 4), bits = Number(process.argv[7]);
    const read = (path) => { const raw = fs.readFileSync(path); return bits === 8 ? new Uint8Array(raw) : new Uint16Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length)); };
    const a = read(pa), two = read(pb), M = bits === 8 ? 255 : 65535, lo = M >> 2, hi = M - (M >> 2);
    const list = (op, options) => Array.from(c.combineTexels(a, two, op, Object.assign({ channels: 2, channel: 0 }, options)));
    const plain = (s) => { const o = {}; for (const k of Object.keys(s)) { o[k] = typeof s[k] === 'bigint' ? s[k].toString() : s[k]; } return o; };
    const stats = plain(c.compareStats(a, two, { channels: 2, channel: 0, aRange: [lo, hi], bRange: [lo, hi] }));
    const same = plain(c.compareStats(a, two, { channels: 2, channel: 1 }));
    console.log(JSON.stringify({ mask: list('mask', { lo, hi, fill: M - 1 }), min: list('min'), max: list('max'), absdiff: list('absdiff'), pair: list('pair'),
        absdiff1: list('absdiff', { channel: 1 }), blend: blends(M).map(([wa, wb, offset]) => list('blend', { wa, wb, offset })),
        compare: { voxels: stats.voxels, differing: stats.differing, max_abs: stats.maxAbs, sum_abs: stats.sumAbs, sum_sq: stats.sumSq, in_a: stats.inA, in_b: stats.inB,
            both: stats.both, dice: stats.dice, jaccard: stats.jaccard, mse: stats.mse, psnr: stats.psnr },
        compare_same: { differing: same.differing, mse: same.mse, psnr: same.psnr } }));
}
console.log('js combine host ok');
