'use strict';
// node js/test/test_reconstruct_host.js [MARKER MASK NX NY NZ BITS] — no device: the argument checks of js/vpt/reconstruct.js, the option
// validation of RenderingContext and the plain-JS twin on cases written down by hand.  With arguments, the twin of the texels in the files
// MARKER (two channels) and MASK (one channel, BITS bits each) is printed as one JSON line (tests/test_reconstruct_host.py compares it with
// the numpy statement).
const fs = require('fs');
const r = require('../vpt/reconstruct.js');
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

// ---- the checks
equal(['dilation', 'erosion'].map(r.checkReconstructOp), [0, 1], 'reconstruct op codes');
equal(['fill_holes', 'clear_border', 'hmax', 'hmin', 'dome', 'maxima', 'minima'].map(r.checkGeodesicOp), [0, 1, 2, 3, 4, 5, 6], 'geodesic op codes');
for (const bad of ['opening', 0, null, undefined]) {
    throws(() => r.checkReconstructOp(bad), 'op ' + JSON.stringify(bad), /reconstruct op is/);
    throws(() => r.checkGeodesicOp(bad), 'op ' + JSON.stringify(bad), /geodesic op is/);
}
for (const bad of [['hmax', 256], ['hmax', -1], ['hmax', 1.5], ['hmax', '1'], ['maxima', 1], ['fill_holes', 3], ['minima', 2], ['clear_border', 1]]) {
    throws(() => r.checkGeodesicH(bad[0], bad[1], 255), 'h ' + JSON.stringify(bad), /geodesic/);
}
if (r.checkGeodesicH('dome', 255, 255) !== 255 || r.checkGeodesicH('maxima', 0, 255) !== 0) { throw new Error('h'); }
for (const bad of [[1, 1], [2, 2], [-1, 2], [true, 2]]) { throws(() => r.checkSourceChannel(bad[0], bad[1]), 'channel ' + JSON.stringify(bad), /channel/); }
throws(() => r.reconstructTexels(new Uint8Array(4), new Uint16Array(4), [4, 1, 1]), 'two widths', /one width/);
throws(() => r.reconstructTexels(new Uint8Array(4), new Uint8Array(5), [4, 1, 1]), 'two sizes', /texels/);
throws(() => r.reconstructTexels(new Uint8Array(4), new Uint8Array(4), [4, 1, 1], { connectivity: 8 }), 'connectivity 8', /connectivity/);
throws(() => r.geodesicTexels(new Float32Array(4), [4, 1, 1], 'hmax'), 'float texels');

// ---- cases written down
const u8 = (a) => new Uint8Array(a);
// a row: the marker's 9 spreads under the mask until a voxel of 3 stops all but 3 of it
equal(r.reconstructTexels(u8([0, 9, 0, 0, 0, 0]), u8([5, 7, 8, 3, 6, 0]), [6, 1, 1]), [5, 7, 7, 3, 3, 0], 'a row by dilation');
equal(r.reconstructTexels(u8([255, 246, 255, 255, 255, 255]), u8([250, 248, 247, 252, 249, 255]), [6, 1, 1], { op: 'erosion' }),
    [250, 248, 248, 252, 252, 255], 'the complement by erosion');
// two voxels that share a corner only
const mask2 = u8([200, 0, 0, 0, 0, 0, 0, 200]), marker2 = u8([150, 0, 0, 0, 0, 0, 0, 0]);
equal(r.reconstructTexels(marker2, mask2, [2, 2, 2], { connectivity: 26 }), [150, 0, 0, 0, 0, 0, 0, 150], 'a corner under 26');
equal(r.reconstructTexels(marker2, mask2, [2, 2, 2], { connectivity: 18 }), [150, 0, 0, 0, 0, 0, 0, 0], 'a corner under 18');
// a 3 x 3 x 3 block around a pit: filled to the block; a pit on the border is not; what does not touch the border stays
const cube = (centre, face, corner) => { const a = new Uint8Array(27).fill(9); a[13] = centre; a[4] = face; a[0] = corner; return a; };
equal(r.geodesicTexels(cube(2, 9, 9), [3, 3, 3], 'fill_holes'), cube(9, 9, 9), 'fill_holes');
equal(r.geodesicTexels(cube(2, 3, 9), [3, 3, 3], 'fill_holes'), cube(3, 3, 9), 'a pit behind a lower pit on the border');
const lone = new Uint8Array(27); lone[13] = 7; lone[0] = 5;
const kept = new Uint8Array(27); kept[13] = 7;
equal(r.geodesicTexels(lone, [3, 3, 3], 'clear_border'), kept, 'clear_border under 6');
equal(r.geodesicTexels(lone, [3, 3, 3], 'clear_border', { connectivity: 26 }), new Uint8Array(27).fill(0).map((v, i) => i === 13 ? 2 : 0), 'clear_border under 26');
const hills = u8([0, 10, 4, 12, 0, 3, 0]);
equal(r.geodesicTexels(hills, [7, 1, 1], 'hmax', { h: 5 }), [0, 5, 4, 7, 0, 0, 0], 'hmax 5');
equal(r.geodesicTexels(hills, [7, 1, 1], 'hmax'), hills, 'hmax 0');
equal(r.geodesicTexels(hills, [7, 1, 1], 'dome', { h: 5 }), [0, 5, 0, 5, 0, 3, 0], 'dome 5');
equal(r.geodesicTexels(hills, [7, 1, 1], 'maxima'), [0, 255, 0, 255, 0, 255, 0], 'maxima');
equal(r.geodesicTexels(hills, [7, 1, 1], 'minima'), [255, 0, 255, 0, 255, 0, 255], 'minima');
equal(r.geodesicTexels(u8([0, 0, 0]), [3, 1, 1], 'maxima'), [0, 0, 0], 'a voxel of code 0 is never a maximum');
equal(r.geodesicTexels(u8([255, 255]), [2, 1, 1], 'minima'), [0, 0], 'a voxel of code M is never a minimum');
equal(r.geodesicTexels(u8([4, 4, 4]), [3, 1, 1], 'maxima'), [255, 255, 255], 'a constant volume is one plateau');
equal(r.geodesicTexels(new Uint16Array([0, 65535, 7]), [3, 1, 1], 'hmin', { h: 65535 }), [65535, 65535, 65535], 'hmin M');

// ---- the option
if (RenderingContext._geodesicSpec(null) !== null || RenderingContext._geodesicSpec(undefined) !== null) { throw new Error('no option'); }
if (JSON.stringify(RenderingContext._geodesicSpec({ op: 'fill_holes' })) !== JSON.stringify({ op: 'fill_holes', h: 0, connectivity: 6 })) { throw new Error('defaults'); }
if (JSON.stringify(RenderingContext._geodesicSpec({ op: 'hmax', h: 300, connectivity: 26 })) !== JSON.stringify({ op: 'hmax', h: 300, connectivity: 26 })) { throw new Error('hmax'); }
for (const bad of ['hmax', {}, { h: 3 }, { op: 'watershed' }, { op: 'hmax', h: -1 }, { op: 'hmax', h: 65536 }, { op: 'maxima', h: 1 }, { op: 'hmax', connectivity: 4 },
    { op: 'hmax', passes: 2 }, ['hmax']]) {
    throws(() => new RenderingContext({ geodesic: bad }), 'RenderingContext({ geodesic: ' + JSON.stringify(bad) + ' })');
}

if (process.argv.length > 2) {
    const [pm, pk] = process.argv.slice(2, 4), dims = process.argv.slice(4, 7).map(Number), bits = Number(process.argv[7]);
    const read = (path) => { const raw = fs.readFileSync(path); return bits === 8 ? new Uint8Array(raw) : new Uint16Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length)); };
    const two = read(pm), mask = read(pk), M = bits === 8 ? 255 : 65535, h = 37 * ((M / 255) | 0);
    const out = { reconstruct: {}, geodesic: {} };
    for (const c of [6, 18, 26]) {
        for (const op of ['dilation', 'erosion']) {
            for (const channel of [0, 1]) {
                out.reconstruct[`${op} ${c} ${channel}`] = Array.from(r.reconstructTexels(two, mask, dims, { op, connectivity: c, channels: 2, channel }));
            }
        }
        for (const op of r.GEODESIC_OPS) {
            const takes = op === 'hmax' || op === 'hmin' || op === 'dome';
            out.geodesic[`${op} ${c}`] = Array.from(r.geodesicTexels(mask, dims, op, { h: takes ? h : 0, connectivity: c }));
        }
    }
    console.log(JSON.stringify(out));
}
console.log('js reconstruct host ok');
