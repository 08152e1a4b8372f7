'use strict';
// The curve skeleton and the topological kernel of a value range of a volume by subfield thinning, in plain JS: the statement of the contract
// the device kernels (vpt_volume_skeleton and the vpt_skeleton_* family; include/vpt.h) are held to, for callers without a device.
// Uint8Array / Uint16Array texels, x fastest; the numpy statement (vpt_amd/skeleton.py) says the same and has the wording of the contract.
//
//   object X:  lo <= code <= hi; everything else, and everything outside the volume, is background; topology (26, 6)
//   obj(p):    the 26-neighbours of p in X;  C(p): the 26-components of obj(p);  B(p): the 6-components of N18(p) \ X that hold a face
//              neighbour of p;  simple: C == 1 and B == 1;  subfield: (x & 1) | (y & 1) << 1 | (z & 1) << 2
//   a pass:    Border = the voxels of X with a background face neighbour when the pass starts; for s = 0 .. 7 every voxel of Border still in X
//              with subfield s: 'kernel' deletes it if simple; 'ends' skips |obj| == 1, otherwise deletes it if simple; 'isthmus' skips a
//              marked voxel, marks and skips C >= 2, otherwise deletes it if simple
//   burn:      0 outside the range, k for a voxel deleted in pass k, THIN_KEPT for a voxel that survived

const THIN_KEPT = 0xFFFFFFFF;
const THIN_MODES = { kernel: 0, ends: 1, isthmus: 2 };
const SKELETON_INFO_FIELDS = ['object_voxels', 'kept_voxels', 'passes', 'converged', 'isolated', 'ends', 'regular', 'junctions'];

// the 3 x 3 x 3 neighbourhood as 27 bits: bit 9 (dz + 1) + 3 (dy + 1) + (dx + 1); the centre is bit 13
const OFFSETS = [];
for (let i = 0; i < 27; i++) { OFFSETS.push([i % 3 - 1, Math.floor(i / 3) % 3 - 1, Math.floor(i / 9) - 1]); }
const CENTRE = 1 << 13;
const nonzero = o => (o[0] !== 0) + (o[1] !== 0) + (o[2] !== 0);
let N18 = 0, N6 = 0;
OFFSETS.forEach((o, i) => { if (nonzero(o) === 1 || nonzero(o) === 2) { N18 |= 1 << i; } if (nonzero(o) === 1) { N6 |= 1 << i; } });
function adjacency(reach) {
    return OFFSETS.map((a) => {
        let m = 0;
        OFFSETS.forEach((b, j) => {
            const d = [Math.abs(a[0] - b[0]), Math.abs(a[1] - b[1]), Math.abs(a[2] - b[2])];
            if (j !== 13 && d[0] + d[1] + d[2] > 0 && Math.max(d[0], d[1], d[2]) <= 1 && d[0] + d[1] + d[2] <= reach) { m |= 1 << j; }
        });
        return m;
    });
}
const ADJ26 = adjacency(3), ADJ6 = adjacency(1);

// the connected components of a set of cube voxels: the voxels are added one by one, each joining the parts it touches
function parts(bits, adj) {
    let found = [];
    for (let i = 0; i < 27; i++) {
        if (!(bits & (1 << i))) { continue; }
        let joined = 1 << i;
        const rest = [];
        for (const part of found) { if (part & adj[i]) { joined |= part; } else { rest.push(part); } }
        rest.push(joined);
        found = rest;
    }
    return found;
}
// [C, B] of a voxel whose object neighbours are the bit set obj (27 bits, the centre bit clear)
function topology(obj) {
    return [parts(obj, ADJ26).length, parts(N18 & ~obj, ADJ6).filter(part => part & N6).length];
}

function whole(value, what) {
    if (typeof value !== 'number' || !Number.isInteger(value)) { throw new Error(what + ' is an integer, not ' + JSON.stringify(value)); }
    return value;
}
// the code of 'kernel' (0), 'ends' (1) or 'isthmus' (2); throws otherwise
function checkThinMode(mode) {
    if (typeof mode !== 'string' || !Object.prototype.hasOwnProperty.call(THIN_MODES, mode)) {
        throw new Error("mode is 'kernel', 'ends' or 'isthmus', not " + JSON.stringify(mode));
    }
    return THIN_MODES[mode];
}
function checkSkeletonRange(lo, hi, largest) {
    whole(lo, 'the lower end of a skeleton range'); whole(hi, 'the upper end of a skeleton range');
    if (!(0 <= lo && lo <= hi && hi <= largest)) { throw new Error(`skeleton range [${lo}, ${hi}]: 0 <= lo <= hi <= ${largest}`); }
}
// the pass cap: 0 (to the fixed point) or a positive integer below 2^31; throws otherwise
function checkThinPasses(passes) {
    whole(passes, 'passes');
    if (!(0 <= passes && passes < 2147483648)) { throw new Error('passes is 0 (to the fixed point) or a positive cap, not ' + passes); }
    return passes;
}
// [kLo, kHi, fill] of a selection of burn passes: 0 <= kLo <= kHi < 2^32 (kHi null / undefined: 0xFFFFFFFF), 0 <= fill <= largest
function checkBurnWithin(kLo, kHi, fill, largest) {
    whole(kLo, 'the first burn pass kept');
    kHi = kHi === undefined || kHi === null ? THIN_KEPT : whole(kHi, 'the last burn pass kept');
    whole(fill, 'fill');
    if (!(0 <= kLo && kLo <= kHi && kHi <= THIN_KEPT)) { throw new Error(`burn passes ${kLo} .. ${kHi}: 0 <= from <= to < 2^32 is required`); }
    if (!(0 <= fill && fill <= largest)) { throw new Error(`fill ${fill}: the largest code is ${largest}`); }
    return [kLo, kHi, fill];
}
function checkTexels(texels, nx, ny, nz) {
    if (!(texels instanceof Uint8Array || texels instanceof Uint16Array) || !(nx >= 1 && ny >= 1 && nz >= 1) || texels.length !== nx * ny * nz) {
        throw new Error('the skeleton takes Uint8Array or Uint16Array texels of width x height x depth voxels');
    }
    if (Math.max(nx, ny, nz) > 4096) { throw new Error('the skeleton takes at most 4096 voxels an axis'); }
    return texels instanceof Uint16Array ? 65535 : 255;
}

// { burn: Uint32Array, info } of thinning the codes lo .. hi in `mode` for at most `passes` passes (default 0: to the fixed point): what
// Volume.skeleton(...) holds on the device.  order (for tests): 'raster' (default) or 'reversed', the order of the visits inside a sub-step
function skeletonBurnTexels(texels, nx, ny, nz, lo, hi, mode, passes, order) {
    const largest = checkTexels(texels, nx, ny, nz);
    checkSkeletonRange(lo, hi, largest);
    const code = checkThinMode(mode);
    passes = checkThinPasses(passes !== undefined ? passes : 0);
    order = order !== undefined ? order : 'raster';
    if (order !== 'raster' && order !== 'reversed') { throw new Error("order is 'raster' or 'reversed', not " + JSON.stringify(order)); }
    const n = nx * ny * nz, px = nx + 2, py = ny + 2, plane = px * py;
    const X = new Uint8Array(px * py * (nz + 2));                 // the object with a background rim: [z + 1][y + 1][x + 1]
    const at = (x, y, z) => (z + 1) * plane + (y + 1) * px + (x + 1);
    const burn = new Uint32Array(n), marked = new Uint8Array(n);
    const info = {};
    for (const f of SKELETON_INFO_FIELDS) { info[f] = 0; }
    info.converged = 1;
    for (let z = 0, i = 0; z < nz; z++) { for (let y = 0; y < ny; y++) { for (let x = 0; x < nx; x++, i++) {
        if (texels[i] >= lo && texels[i] <= hi) { X[at(x, y, z)] = 1; burn[i] = THIN_KEPT; info.object_voxels++; }
    } } }
    if (info.object_voxels === 0) { return { burn: burn, info: info }; }
    for (let k = 1; ; k++) {
        const border = [[], [], [], [], [], [], [], []];              // per subfield, in raster order
        for (let z = 0, i = 0; z < nz; z++) { for (let y = 0; y < ny; y++) { for (let x = 0; x < nx; x++, i++) {
            const p = at(x, y, z);
            if (X[p] && !(X[p - 1] && X[p + 1] && X[p - px] && X[p + px] && X[p - plane] && X[p + plane])) { border[(x & 1) | ((y & 1) << 1) | ((z & 1) << 2)].push(i); }
        } } }
        let changed = 0;
        for (let s = 0; s < 8; s++) {
            const visits = order === 'reversed' ? border[s].slice().reverse() : border[s];
            for (const i of visits) {
                const x = i % nx, y = Math.floor(i / nx) % ny, z = Math.floor(i / (nx * ny)), p = at(x, y, z);
                let obj = 0;
                for (let b = 0; b < 27; b++) { if (b !== 13 && X[p + OFFSETS[b][0] + OFFSETS[b][1] * px + OFFSETS[b][2] * plane]) { obj |= 1 << b; } }
                if (code === 1 && obj !== 0 && (obj & (obj - 1)) === 0) { continue; }      // a curve end
                if (code === 2 && marked[i]) { continue; }
                const t = topology(obj);
                if (code === 2 && t[0] >= 2) { marked[i] = 1; changed++; }
                else if (t[0] === 1 && t[1] === 1) { X[p] = 0; burn[i] = k; changed++; }
            }
        }
        info.passes = k;
        info.converged = changed === 0 ? 1 : 0;
        if (changed === 0 || k === passes) { break; }
    }
    const counts = [0, 0, 0, 0];
    for (let z = 0, i = 0; z < nz; z++) { for (let y = 0; y < ny; y++) { for (let x = 0; x < nx; x++, i++) {
        const p = at(x, y, z);
        if (!X[p]) { continue; }
        let near = 0;
        for (let b = 0; b < 27; b++) { if (b !== 13) { near += X[p + OFFSETS[b][0] + OFFSETS[b][1] * px + OFFSETS[b][2] * plane]; } }
        counts[Math.min(near, 3)]++;
        info.kept_voxels++;
    } } }
    info.isolated = counts[0]; info.ends = counts[1]; info.regular = counts[2]; info.junctions = counts[3];
    return { burn: burn, info: info };
}

// the texels' codes where kLo <= burn <= kHi (defaults THIN_KEPT and 0xFFFFFFFF), `fill` (default 0) elsewhere: what Skeleton.within holds
function burnWithinTexels(texels, burn, kLo, kHi, fill) {
    if (!(texels instanceof Uint8Array || texels instanceof Uint16Array)) { throw new Error('the skeleton takes Uint8Array or Uint16Array texels'); }
    if (!(burn instanceof Uint32Array) || burn.length !== texels.length) { throw new Error('burn passes are one Uint32 per voxel of the texels'); }
    const k = checkBurnWithin(kLo !== undefined ? kLo : THIN_KEPT, kHi, fill !== undefined ? fill : 0, texels instanceof Uint16Array ? 65535 : 255);
    const out = new texels.constructor(texels.length);
    for (let i = 0; i < texels.length; i++) { out[i] = burn[i] >= k[0] && burn[i] <= k[1] ? texels[i] : k[2]; }
    return out;
}

// the codes of the voxels of lo .. hi that survive the thinning (mode default 'ends'), `fill` elsewhere: what Volume.centreline holds
function skeletonTexels(texels, nx, ny, nz, lo, hi, mode, passes, fill) {
    const found = skeletonBurnTexels(texels, nx, ny, nz, lo, hi, mode !== undefined ? mode : 'ends', passes);
    return burnWithinTexels(texels, found.burn, THIN_KEPT, THIN_KEPT, fill);
}

// the `skeleton` option of a RenderingContext with its defaults filled in: null, or { lo, hi, mode: 'ends', passes: 0, fill: 0 }; throws
// otherwise.  The range is open above (hi is cut to the volume's largest code when the option is applied)
function checkSkeleton(spec) {
    if (spec === undefined || spec === null) { return null; }
    const known = ['lo', 'hi', 'mode', 'passes', 'fill'], given = k => spec[k] !== undefined && spec[k] !== null;
    if (typeof spec !== 'object' || Array.isArray(spec) || !Object.keys(spec).every(k => known.includes(k)) || !given('lo') || !given('hi')) {
        throw new Error('skeleton is null or { lo, hi, mode, passes, fill }, not ' + JSON.stringify(spec));
    }
    checkSkeletonRange(spec.lo, spec.hi, 65535);
    const out = { lo: spec.lo, hi: spec.hi, mode: given('mode') ? spec.mode : 'ends', passes: checkThinPasses(given('passes') ? spec.passes : 0), fill: given('fill') ? spec.fill : 0 };
    checkThinMode(out.mode);
    whole(out.fill, 'fill');
    if (!(0 <= out.fill && out.fill <= 65535)) { throw new Error(`fill ${out.fill}: the largest code is 65535`); }
    return out;
}

module.exports = { THIN_KEPT, THIN_MODES, SKELETON_INFO_FIELDS, skeletonTopology: topology, checkThinMode, checkSkeletonRange, checkThinPasses, checkBurnWithin,
    skeletonBurnTexels, burnWithinTexels, skeletonTexels, checkSkeleton };
