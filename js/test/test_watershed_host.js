'use strict';
// node js/test/test_watershed_host.js [RELIEF NX NY NZ BITS] — no device: the argument checks of js/vpt/watershed.js, the `split` option of
// RenderingContext and the plain-JS twin on cases written down by hand.  With arguments, the twin of the two-channel texels in the file
// RELIEF (BITS bits a channel) is printed as one JSON line (tests/test_watershed_host.py compares it with the numpy statement).
const fs = require('fs');
const w = require('../vpt/watershed.js');
const { RenderingContext } = require('../vpt/RenderingContext.js');

function throws(f, what, pattern) {
    let message = null;
    try { f(); } catch (e) { message = e.message; }
    if (message === null) { throw new Error(what + ' was accepted'); }
    if (pattern && !pattern.test(message)) { throw new Error(what + ': unexpected message ' + message); }
}
function same(a, b, what) {
    if (JSON.stringify(Array.from(a)) !== JSON.stringify(Array.from(b))) { throw new Error(`${what}: ${JSON.stringify(Array.from(a))}, expected ${JSON.stringify(Array.from(b))}`); }
}

// ---- the checks
same(['minima', 'maxima'].map(w.checkPolarity), [0, 1], 'polarity codes');
for (const bad of ['both', 0, null, undefined]) { throws(() => w.checkPolarity(bad), 'polarity ' + JSON.stringify(bad), /polarity/); }
const u8 = (a) => new Uint8Array(a);
throws(() => w.watershedTexels(u8([1, 2]), [2, 1, 1], 3, 2), 'lo above hi', /range/);
throws(() => w.watershedTexels(u8([1, 2]), [2, 1, 1], 0, 256), 'hi above M', /range/);
throws(() => w.watershedTexels(u8([1, 2]), [2, 1, 1], 0, 255, { connectivity: 8 }), 'connectivity 8', /connectivity/);
throws(() => w.watershedTexels(u8([1, 2]), [2, 1, 1], 0, 255, { minVoxels: 0 }), 'minVoxels 0', /minVoxels/);
throws(() => w.watershedTexels(u8([1, 2]), [2, 1, 1], 0, 255, { channel: 1 }), 'channel 1 of one', /channel/);
throws(() => w.watershedTexels(u8([1, 2, 3]), [2, 1, 1], 0, 255), 'a wrong size', /relief/);
throws(() => w.watershedTexels(new Float32Array(2), [2, 1, 1], 0, 255), 'float texels', /relief/);

// ---- cases written down
// a row with two pits: the voxel between them (5) goes to the lower pit's side, 3 < 4; ties in size go by root
let r = w.watershedTexels(u8([9, 3, 5, 4, 8]), [5, 1, 1], 0, 255);
same(r.ranks, [1, 1, 1, 2, 2], 'two pits'); same(r.list, [[0, 0, 0, 3], [3, 0, 0, 2]], 'two pits, the list'); same(r.pointer, [1, 1, 1, 3, 3], 'two pits, the pointers');
// from the maxima the same row has three peaks, 9, 5 and 8: 3 climbs to 9, 4 to 8; equal sizes are ordered by root
r = w.watershedTexels(u8([9, 3, 5, 4, 8]), [5, 1, 1], 0, 255, { polarity: 'maxima' });
same(r.ranks, [1, 1, 3, 2, 2], 'three peaks'); same(r.list, [[0, 0, 0, 2], [3, 0, 0, 2], [2, 0, 0, 1]], 'three peaks, the list');
// a plateau between two pits is cut where the geodesic distances to its borders meet; the middle voxel goes to the smaller index
r = w.watershedTexels(u8([1, 7, 7, 7, 2]), [5, 1, 1], 0, 255);
same(r.ranks, [1, 1, 1, 2, 2], 'a plateau'); same(r.pointer, [0, 0, 1, 4, 4], 'a plateau, the pointers');
// the domain: a voxel outside D is no neighbour and has rank 0; minVoxels drops a basin
r = w.watershedTexels(u8([4, 0, 4, 5, 6]), [5, 1, 1], 1, 255);
same(r.ranks, [2, 0, 1, 1, 1], 'the domain'); same(r.pointer, [0, -1, 2, 2, 3], 'the domain, the pointers');
same(w.watershedTexels(u8([4, 0, 4, 5, 6]), [5, 1, 1], 1, 255, { minVoxels: 2 }).ranks, [0, 0, 1, 1, 1], 'minVoxels');
// a constant volume is one basin; two voxels that share a corner only
same(w.watershedTexels(new Uint16Array(6).fill(65535), [3, 2, 1], 0, 65535).list, [[0, 0, 0, 6]], 'constant');
const corner = u8([200, 0, 0, 0, 0, 0, 0, 200]);
same(w.watershedTexels(corner, [2, 2, 2], 1, 255, { connectivity: 26 }).list, [[0, 0, 0, 2]], 'a corner under 26');
same(w.watershedTexels(corner, [2, 2, 2], 1, 255, { connectivity: 18 }).list, [[0, 0, 0, 1], [1, 1, 1, 1]], 'a corner under 18');
// two channels
same(w.watershedTexels(u8([9, 1, 9, 2, 9, 1]), [3, 1, 1], 0, 255, { channels: 2, channel: 1 }).ranks, [1, 1, 2], 'channel 1');

// ---- the option
if (w.checkSplit(null) !== null || w.checkSplit(undefined) !== null) { throw new Error('no option'); }
same([JSON.stringify(w.checkSplit({ lo: 100, hi: 255 }))], [JSON.stringify({ h: 2, steps: 4, connectivity: 26, minVoxels: 1, lo: 100, hi: 255 })], 'defaults');
for (const bad of ['split', {}, { lo: 1 }, { lo: 2, hi: 1 }, { lo: 1, hi: 2, h: -1 }, { lo: 1, hi: 2, steps: 0 }, { lo: 1, hi: 2, connectivity: 7 },
    { lo: 1, hi: 2, minVoxels: 0 }, { lo: 1, hi: 2, depth: 3 }, [1, 2]]) {
    throws(() => new RenderingContext({ split: bad }), 'RenderingContext({ split: ' + JSON.stringify(bad) + ' })');
}
const ok = { lo: 100, hi: 255 };
throws(() => new RenderingContext({ split: ok, gradient: 'central' }), 'split with gradient', /split and .* both write the second channel/);
throws(() => new RenderingContext({ split: ok, components: { lo: 1, hi: 2, mode: 'label' } }), 'split with label', /split and .* both write the second channel/);
throws(() => new RenderingContext({ split: ok, distance: { lo: 1, hi: 2, mode: 'channel' } }), 'split with distance channel', /split and .* both write the second channel/);
throws(() => new RenderingContext({ split: ok, combine: { reader: {}, op: 'pair' } }), 'split with pair', /split and .* both write the second channel/);

if (process.argv.length > 2) {
    const path = process.argv[2], dims = process.argv.slice(3, 6).map(Number), bits = Number(process.argv[6]);
    const raw = fs.readFileSync(path);
    const two = bits === 8 ? new Uint8Array(raw) : new Uint16Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length));
    const M = bits === 8 ? 255 : 65535, out = {};
    for (const c of [6, 18, 26]) {
        for (const polarity of ['minima', 'maxima']) {
            for (const channel of [0, 1]) {
                const got = w.watershedTexels(two, dims, M >> 3, M - (M >> 4), { polarity, connectivity: c, minVoxels: 2, channels: 2, channel });
                out[`${polarity} ${c} ${channel}`] = { ranks: Array.from(got.ranks), list: got.list };
            }
        }
    }
    console.log(JSON.stringify(out));
}
console.log('js watershed host ok');
