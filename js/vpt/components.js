'use strict';
// The connected components of a value range of a volume in plain JS: the contract of include/vpt.h ("connected components") restated for
// hosts without a device, the twin of vpt_amd/components.py.  texels: a Uint8Array / Uint16Array of [nz][ny][nx] codes.
//   foreground: lo <= code <= hi;  connectivity 6 (faces), 18 (faces and edges), 26 (faces, edges and corners); outside is background
//   root: the voxel of a component with the smallest linear index (z ny + y) nx + x
//   listed: the components of at least minVoxels voxels, by voxel count descending, then root ascending; rank: 1-based position, 0 elsewhere

function checkConnectivity(connectivity) {
    if (connectivity !== 6 && connectivity !== 18 && connectivity !== 26) { throw new Error('connectivity is 6, 18 or 26, not ' + JSON.stringify(connectivity)); }
    return connectivity;
}
function checkRange(lo, hi, largest) {
    if (!Number.isInteger(lo) || !Number.isInteger(hi) || !(0 <= lo && lo <= hi && hi <= largest)) {
        throw new Error(`component range [${JSON.stringify(lo)}, ${JSON.stringify(hi)}]: integers with 0 <= lo <= hi <= ${largest}`);
    }
    return [lo, hi];
}
function checkMinVoxels(minVoxels) {
    if (!Number.isInteger(minVoxels) || minVoxels < 1 || minVoxels > 0xFFFFFFFF) { throw new Error('minVoxels is an integer in 1 .. 2^32 - 1, not ' + JSON.stringify(minVoxels)); }
    return minVoxels;
}
// [first, last, fill]: 1 <= first <= last (last null / undefined: every rank; Infinity allowed), 0 <= fill <= largest
function checkKeep(first, last, fill, largest) {
    if (last === null || last === undefined) { last = Infinity; }
    if (!Number.isInteger(first) || !(Number.isInteger(last) || last === Infinity) || !(1 <= first && first <= last)) {
        throw new Error(`ranks ${JSON.stringify(first)} .. ${JSON.stringify(last)}: integers with 1 <= first <= last`);
    }
    if (!Number.isInteger(fill) || fill < 0 || fill > largest) { throw new Error(`fill ${JSON.stringify(fill)}: the largest code is ${largest}`); }
    return [first, last, fill];
}
function largestCode(texels) {
    if (texels instanceof Uint8Array) { return 255; }
    if (texels instanceof Uint16Array) { return 65535; }
    throw new Error('connected components take a Uint8Array or a Uint16Array');
}

// { ranks: Uint32Array [nz][ny][nx], list: [[rootX, rootY, rootZ, voxels], ...] in canonical order }
function componentsTexels(texels, nx, ny, nz, lo, hi, connectivity, minVoxels) {
    const largest = largestCode(texels);
    checkRange(lo, hi, largest);
    connectivity = checkConnectivity(connectivity !== undefined ? connectivity : 6);
    minVoxels = checkMinVoxels(minVoxels !== undefined ? minVoxels : 1);
    const n = nx * ny * nz;
    if (texels.length !== n || n < 1) { throw new Error('texels are [nz][ny][nx]'); }
    const most = connectivity === 6 ? 1 : connectivity === 18 ? 2 : 3;
    const offsets = [];
    for (let c = -1; c <= 1; c++) { for (let b = -1; b <= 1; b++) { for (let a = -1; a <= 1; a++) {
        const m = (a !== 0) + (b !== 0) + (c !== 0);
        if (m >= 1 && m <= most) { offsets.push([a, b, c]); }
    } } }
    // flood every component from its smallest voxel: voxels are visited in index order, so the seed of a component is its root
    const root = new Float64Array(n).fill(-1), stack = [], roots = [], sizes = [];
    for (let seed = 0; seed < n; seed++) {
        if (root[seed] >= 0 || texels[seed] < lo || texels[seed] > hi) { continue; }
        let size = 0;
        root[seed] = seed; stack.push(seed);
        while (stack.length) {
            const i = stack.pop(), x = i % nx, y = Math.floor(i / nx) % ny, z = Math.floor(i / (nx * ny));
            size++;
            for (const [a, b, c] of offsets) {
                const xx = x + a, yy = y + b, zz = z + c;
                if (xx < 0 || xx >= nx || yy < 0 || yy >= ny || zz < 0 || zz >= nz) { continue; }
                const j = (zz * ny + yy) * nx + xx;
                if (root[j] < 0 && texels[j] >= lo && texels[j] <= hi) { root[j] = seed; stack.push(j); }
            }
        }
        roots.push(seed); sizes.push(size);
    }
    const order = [];
    for (let k = 0; k < roots.length; k++) { if (sizes[k] >= minVoxels) { order.push(k); } }
    order.sort((p, q) => sizes[q] - sizes[p] || roots[p] - roots[q]);
    const rankOf = new Map();
    order.forEach((k, position) => rankOf.set(roots[k], position + 1));
    const ranks = new Uint32Array(n);
    for (let i = 0; i < n; i++) { if (root[i] >= 0) { ranks[i] = rankOf.get(root[i]) || 0; } }
    const list = order.map(k => [roots[k] % nx, Math.floor(roots[k] / nx) % ny, Math.floor(roots[k] / (nx * ny)), sizes[k]]);
    return { ranks, list };
}

// the codes where first <= rank <= last, `fill` elsewhere, in the texels' type
function keepTexels(texels, ranks, first, last, fill) {
    const k = checkKeep(first !== undefined ? first : 1, last, fill !== undefined ? fill : 0, largestCode(texels));
    if (ranks.length !== texels.length) { throw new Error('ranks are one per voxel'); }
    const out = new texels.constructor(texels.length);
    for (let i = 0; i < out.length; i++) { out[i] = ranks[i] >= k[0] && ranks[i] <= k[1] ? texels[i] : k[2]; }
    return out;
}

// interleaved (code, min(rank, M)) in the texels' type, M its largest code
function labelTexels(texels, ranks) {
    const M = largestCode(texels);
    if (ranks.length !== texels.length) { throw new Error('ranks are one per voxel'); }
    const out = new texels.constructor(2 * texels.length);
    for (let i = 0; i < texels.length; i++) { out[2 * i] = texels[i]; out[2 * i + 1] = Math.min(ranks[i], M); }
    return out;
}

module.exports = { componentsTexels, keepTexels, labelTexels, checkConnectivity, checkRange, checkMinVoxels, checkKeep };
