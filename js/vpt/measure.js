'use strict';
// Per-component measurements of a labelling and the selection by a set of ranks in plain JS: the contract of include/vpt.h
// (vpt_components_measure, vpt_components_keep_set) restated for hosts without a device, the twin of vpt_amd/measure.py.
//   ranks: a Uint32Array of [nz][ny][nx] 1-based ranks (0: background and dropped components); values: a Uint8Array / Uint16Array of the
//   same length (its width is independent of the labelled texels')
//   record k: the component of rank first + 1 + k; voxels of other ranks contribute nothing
//   faces: a voxel's face counts when the neighbour across it lies outside the volume or has a different rank
// The 64-bit fields of a record are BigInts (as Volume.compare returns its counts), the 32-bit ones numbers.

const FIELDS = ['voxels', 'minX', 'minY', 'minZ', 'maxX', 'maxY', 'maxZ', 'valueMin', 'valueMax', 'sumX', 'sumY', 'sumZ', 'valueSum', 'valueSumSq', 'faces'];
const WIDE = new Set(['voxels', 'sumX', 'sumY', 'sumZ', 'valueSum', 'valueSumSq', 'faces']);

// [first, n]: integers with 0 <= first <= listed and 0 <= n <= listed - first (n null / undefined: to the end)
function checkWindow(first, n, listed) {
    if (!Number.isInteger(first) || first < 0 || first > listed) { throw new Error(`components ${JSON.stringify(first)} .. are not within the ${listed} listed`); }
    if (n === null || n === undefined) { n = listed - first; }
    if (!Number.isInteger(n) || n < 0 || n > listed - first) { throw new Error(`components ${first} .. +${JSON.stringify(n)} are not within the ${listed} listed`); }
    return [first, n];
}
// the ranks of a selection as an array of integers >= 1: an iterable of ranks (numbers or BigInts; duplicates and ranks beyond the list are
// allowed), or an array of booleans over the list (entry k selects rank k + 1)
function checkRankSet(selected, listed) {
    const a = Array.from(selected);
    if (a.length && a.every(v => typeof v === 'boolean')) {
        if (listed !== undefined && a.length !== listed) { throw new Error('a boolean selection has one entry per listed component'); }
        const out = [];
        a.forEach((v, k) => { if (v) { out.push(k + 1); } });
        return out;
    }
    return a.map(r => {
        if (typeof r === 'bigint') { if (r < 1n || r > 0xFFFFFFFFFFFFFFFFn) { throw new Error(`rank ${r}: ranks are 1-based`); } return r > 0xFFFFFFFFn ? 0xFFFFFFFF : Number(r); }
        if (!Number.isInteger(r) || r < 1) { throw new Error(`rank ${JSON.stringify(r)}: ranks are 1-based integers`); }
        return Math.min(r, 0xFFFFFFFF);                             // listed <= 2^32 - 2: such a rank selects nothing either way
    });
}

// the records of the components of rank first + 1 .. first + n (n undefined: to the largest rank present)
function measureTexels(ranks, values, nx, ny, nz, first, n) {
    const total = nx * ny * nz;
    if (!(ranks instanceof Uint32Array) || ranks.length !== total || total < 1) { throw new Error('ranks are a Uint32Array [nz][ny][nx]'); }
    if (!(values instanceof Uint8Array || values instanceof Uint16Array) || values.length !== total) { throw new Error('values are a Uint8Array or a Uint16Array of the ranks\' length'); }
    let listed = 0;
    for (let i = 0; i < total; i++) { if (ranks[i] > listed) { listed = ranks[i]; } }
    [first, n] = checkWindow(first !== undefined ? first : 0, n, listed);
    const out = [];
    for (let k = 0; k < n; k++) {
        out.push({ voxels: 0n, minX: 0xFFFFFFFF, minY: 0xFFFFFFFF, minZ: 0xFFFFFFFF, maxX: 0, maxY: 0, maxZ: 0, valueMin: 0xFFFFFFFF, valueMax: 0,
                   sumX: 0n, sumY: 0n, sumZ: 0n, valueSum: 0n, valueSumSq: 0n, faces: 0n });
    }
    for (let z = 0, i = 0; z < nz; z++) { for (let y = 0; y < ny; y++) { for (let x = 0; x < nx; x++, i++) {
        const r = ranks[i], k = r - first - 1;
        if (k < 0 || k >= n) { continue; }
        const o = out[k], v = values[i];
        let faces = 0;
        faces += (x === 0 || ranks[i - 1] !== r) + (x === nx - 1 || ranks[i + 1] !== r);
        faces += (y === 0 || ranks[i - nx] !== r) + (y === ny - 1 || ranks[i + nx] !== r);
        faces += (z === 0 || ranks[i - nx * ny] !== r) + (z === nz - 1 || ranks[i + nx * ny] !== r);
        o.voxels += 1n; o.sumX += BigInt(x); o.sumY += BigInt(y); o.sumZ += BigInt(z);
        o.valueSum += BigInt(v); o.valueSumSq += BigInt(v * v); o.faces += BigInt(faces);
        o.minX = Math.min(o.minX, x); o.minY = Math.min(o.minY, y); o.minZ = Math.min(o.minZ, z);
        o.maxX = Math.max(o.maxX, x); o.maxY = Math.max(o.maxY, y); o.maxZ = Math.max(o.maxZ, z);
        o.valueMin = Math.min(o.valueMin, v); o.valueMax = Math.max(o.valueMax, v);
    } } }
    return out;
}

// the codes where the voxel's rank is in `selected`, `fill` elsewhere, in the texels' type
function keepSetTexels(texels, ranks, selected, fill) {
    if (!(texels instanceof Uint8Array || texels instanceof Uint16Array)) { throw new Error('connected components take a Uint8Array or a Uint16Array'); }
    const largest = texels instanceof Uint8Array ? 255 : 65535;
    fill = fill !== undefined ? fill : 0;
    if (!Number.isInteger(fill) || fill < 0 || fill > largest) { throw new Error(`fill ${JSON.stringify(fill)}: the largest code is ${largest}`); }
    if (ranks.length !== texels.length) { throw new Error('ranks are one per voxel'); }
    const set = new Set(checkRankSet(selected));
    const out = new texels.constructor(texels.length);
    for (let i = 0; i < out.length; i++) { out[i] = set.has(ranks[i]) ? texels[i] : fill; }
    return out;
}

// num / den (BigInts, num >= 0, den > 0) as the nearest double: the quotient is taken to 55 or 56 bits with a sticky last bit, which the
// conversion then rounds once
function ratio(num, den) {
    if (num === 0n) { return 0; }
    const shift = 55 - (num.toString(2).length - den.toString(2).length);
    const a = shift >= 0 ? num << BigInt(shift) : num, b = shift >= 0 ? den : den << BigInt(-shift);
    let q = a / b;
    if (a % b !== 0n) { q |= 1n; }
    return Number(q) * Math.pow(2, -shift);
}

// per record: centroid (sum / voxels), mean, the population variance (n sumSq - sum^2) / n^2 with the numerator in integers before the one
// division, the box extents (max - min + 1) and the fill ratio voxels / box volume
function derive(records) {
    return records.map((r, k) => {
        const n = BigInt(r.voxels);
        if (n === 0n) { throw new Error(`record ${k} has no voxels`); }
        const s = BigInt(r.valueSum), s2 = BigInt(r.valueSumSq);
        const extentX = r.maxX - r.minX + 1, extentY = r.maxY - r.minY + 1, extentZ = r.maxZ - r.minZ + 1;
        return { centroidX: ratio(BigInt(r.sumX), n), centroidY: ratio(BigInt(r.sumY), n), centroidZ: ratio(BigInt(r.sumZ), n), mean: ratio(s, n),
                 variance: ratio(n * s2 - s * s, n * n), extentX, extentY, extentZ, fill: ratio(n, BigInt(extentX) * BigInt(extentY) * BigInt(extentZ)) };
    });
}

module.exports = { measureTexels, keepSetTexels, derive, checkWindow, checkRankSet, MEASURE_FIELDS: FIELDS, MEASURE_WIDE_FIELDS: WIDE };
