'use strict';
// node js/test/test_measure_host.js [CASE] — no device: the argument checks of js/vpt/measure.js and the plain-JS twin against the contract
// written out once more, voxel by voxel.  With a JSON case {shape, ranks, values, first, n, array, bits, selected, fill} the twin's records
// (64-bit fields as decimal strings, fields under the names of struct vpt_component_measure), its derive() and its keepSetTexels are
// printed as one JSON line (tests/test_measure_host.py compares them with the numpy statement).
const m = require('../vpt/measure.js');

function throws(f, what, pattern) {
    let message = null;
    try { f(); } catch (e) { message = e.message; }
    if (message === null) { throw new Error(what + ' was accepted'); }
    if (pattern && !pattern.test(message)) { throw new Error(what + ': unexpected message ' + message); }
}
const snake = name => name.replace(/[A-Z]/g, c => '_' + c.toLowerCase());

if (process.argv.length > 2) {
    const c = JSON.parse(process.argv[2]);
    const [nx, ny, nz] = c.shape;
    const records = m.measureTexels(Uint32Array.from(c.ranks), Uint16Array.from(c.values), nx, ny, nz, c.first, c.n);
    const array = (c.bits === 16 ? Uint16Array : Uint8Array).from(c.array);
    const plain = records.map(r => { const o = {}; for (const f of m.MEASURE_FIELDS) { o[snake(f)] = String(r[f]); } return o; });
    console.log(JSON.stringify({ records: plain, derived: m.derive(records), kept: Array.from(m.keepSetTexels(array, Uint32Array.from(c.ranks), c.selected, c.fill)) }));
    process.exit(0);
}

// ---- the checks
for (const bad of [[-1, 1], [0, 4], [4, 0], [3, 1], [0.5, 1], [0, -1], ['0', 1]]) { throws(() => m.checkWindow(bad[0], bad[1], 3), 'window ' + JSON.stringify(bad), /not within the 3 listed/); }
if (String(m.checkWindow(1, undefined, 3)) !== '1,2' || String(m.checkWindow(3, 0, 3)) !== '3,0') { throw new Error('the default window'); }
for (const bad of [[0], [1, 0], [-1], [1.5], ['1'], [0n]]) { throws(() => m.checkRankSet(bad), 'ranks ' + JSON.stringify(bad.map(String)), /1-based/); }
if (String(m.checkRankSet([3, 3, 2n, 1n << 40n])) !== '3,3,2,4294967295' || String(m.checkRankSet([true, false, true], 3)) !== '1,3') { throw new Error('the rank set'); }
throws(() => m.checkRankSet([true, false], 3), 'a short mask', /one entry per listed/);

// ---- a case small enough to write down: two bars and a single voxel in a 4 x 2 x 2 volume
//   z = 0:  1 1 0 2      z = 1:  1 0 0 2
//           0 0 0 2              3 0 0 0
const ranks = Uint32Array.from([1, 1, 0, 2, 0, 0, 0, 2, 1, 0, 0, 2, 3, 0, 0, 0]);
const values = Uint16Array.from([10, 20, 0, 65535, 0, 0, 0, 1, 30, 0, 0, 2, 7, 0, 0, 0]);
const got = m.measureTexels(ranks, values, 4, 2, 2);
const want = [
    { voxels: 3n, minX: 0, minY: 0, minZ: 0, maxX: 1, maxY: 0, maxZ: 1, valueMin: 10, valueMax: 30, sumX: 1n, sumY: 0n, sumZ: 1n, valueSum: 60n, valueSumSq: 1400n, faces: 14n },
    { voxels: 3n, minX: 3, minY: 0, minZ: 0, maxX: 3, maxY: 1, maxZ: 1, valueMin: 1, valueMax: 65535, sumX: 9n, sumY: 1n, sumZ: 1n, valueSum: 65538n, valueSumSq: 4294836230n, faces: 14n },
    { voxels: 1n, minX: 0, minY: 1, minZ: 1, maxX: 0, maxY: 1, maxZ: 1, valueMin: 7, valueMax: 7, sumX: 0n, sumY: 1n, sumZ: 1n, valueSum: 7n, valueSumSq: 49n, faces: 6n },
];
if (got.length !== 3) { throw new Error('three records'); }
got.forEach((r, k) => { for (const f of m.MEASURE_FIELDS) { if (r[f] !== want[k][f]) { throw new Error(`record ${k}, ${f}: ${r[f]}, expected ${want[k][f]}`); } } });
const slice = m.measureTexels(ranks, values, 4, 2, 2, 1, 1);
if (slice.length !== 1 || slice[0].valueSumSq !== want[1].valueSumSq || slice[0].faces !== 14n) { throw new Error('a window is a slice of the whole'); }
const d = m.derive(got);
if (d[0].centroidX !== 1 / 3 || d[0].mean !== 20 || d[0].variance !== 200 / 3 || d[0].extentX !== 2 || d[0].fill !== 3 / 4 || d[2].variance !== 0) { throw new Error('derive: ' + JSON.stringify(d[0])); }
// past 2^53: the ratio is still the nearest double
if (m.derive([{ voxels: 3000000007n, minX: 0, minY: 0, minZ: 0, maxX: 0, maxY: 0, maxZ: 0, sumX: 0n, sumY: 0n, sumZ: 0n, valueSum: 3000000007n * 65535n,
                valueSumSq: 3000000007n * 65535n * 65535n }])[0].variance !== 0) { throw new Error('a constant component has no variance'); }
throws(() => m.derive([{ voxels: 0n }]), 'an empty record', /no voxels/);

const texels = Uint8Array.from([9, 8, 7, 6, 5, 4, 3, 2, 1, 9, 8, 7, 6, 5, 4, 3]);
const kept = m.keepSetTexels(texels, ranks, [3, 1, 1, 77], 200);
const expected = Uint8Array.from([9, 8, 200, 200, 200, 200, 200, 200, 1, 200, 200, 200, 6, 200, 200, 200]);
kept.forEach((v, i) => { if (v !== expected[i]) { throw new Error(`keepSet: texel ${i} is ${v}`); } });
if (!m.keepSetTexels(texels, ranks, [], 5).every(v => v === 5)) { throw new Error('the empty set'); }
if (String(m.keepSetTexels(texels, ranks, [false, true, false])) !== String(m.keepSetTexels(texels, ranks, [2]))) { throw new Error('a mask'); }
throws(() => m.keepSetTexels(texels, ranks, [1], 256), 'fill 256', /largest code/);
throws(() => m.keepSetTexels(texels, ranks, [0]), 'rank 0', /1-based/);
console.log('js measure host: ok');
