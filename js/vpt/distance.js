'use strict';
// The exact squared Euclidean distance of every voxel to the nearest voxel of a value range of a volume (or of its complement) in plain JS:
// the contract of include/vpt.h ("distance transform") restated for hosts without a device, the twin of vpt_amd/distance.py.
// texels: a Uint8Array / Uint16Array of [nz][ny][nx] codes.
//   in range: lo <= code <= hi;  seeds 'range': the voxels in range, 'rest': the voxels not in range
//   d2: the minimum over the seeds of the squared offset, Uint32; nothing wraps, nothing is clamped: outside is neither seed nor non-seed;
//       NONE = 0xFFFFFFFF everywhere when there is no seed
const NONE = 0xFFFFFFFF;
const SEEDS = ['range', 'rest'];

// the code of 'range' (0: VPT_DISTANCE_TO_RANGE) or 'rest' (1: VPT_DISTANCE_TO_REST)
function checkSeeds(seeds) {
    const code = typeof seeds === 'string' ? SEEDS.indexOf(seeds) : -1;
    if (code < 0) { throw new Error("seeds is 'range' or 'rest', not " + JSON.stringify(seeds)); }
    return code;
}
function checkRange(lo, hi, largest) {
    if (!Number.isInteger(lo) || !Number.isInteger(hi) || !(0 <= lo && lo <= hi && hi <= largest)) {
        throw new Error(`distance range [${JSON.stringify(lo)}, ${JSON.stringify(hi)}]: integers with 0 <= lo <= hi <= ${largest}`);
    }
    return [lo, hi];
}
// the transfer-function rows per voxel of distance: an integer in 1 .. 256
function checkSteps(steps) {
    if (!Number.isInteger(steps) || steps < 1 || steps > 256) { throw new Error('steps is an integer in 1 .. 256, not ' + JSON.stringify(steps)); }
    return steps;
}
// floor(radius^2), taken in IEEE double, of a non-negative finite radius, at most 2^32 - 2 (the largest squared distance that is not NONE: a
// larger radius selects what that one selects)
function checkRadius(radius) {
    if (typeof radius !== 'number' || !Number.isFinite(radius) || radius < 0) {
        throw new Error('radius is finite and not negative, not ' + JSON.stringify(radius));
    }
    const square = radius * radius;
    return square >= NONE - 1 ? NONE - 1 : Math.floor(square);
}
// [r2Lo, r2Hi, fill]: integers with 0 <= r2Lo <= r2Hi < 2^32 (r2Hi null / undefined: 0xFFFFFFFF, NONE included), 0 <= fill <= largest
function checkWithin(r2Lo, r2Hi, fill, largest) {
    if (r2Hi === null || r2Hi === undefined) { r2Hi = NONE; }
    if (!Number.isInteger(r2Lo) || !Number.isInteger(r2Hi) || !(0 <= r2Lo && r2Lo <= r2Hi && r2Hi <= NONE)) {
        throw new Error(`squared distances ${JSON.stringify(r2Lo)} .. ${JSON.stringify(r2Hi)}: integers with 0 <= from <= to < 2^32`);
    }
    if (!Number.isInteger(fill) || fill < 0 || fill > largest) { throw new Error(`fill ${JSON.stringify(fill)}: the largest code is ${largest}`); }
    return [r2Lo, r2Hi, fill];
}
function largestCode(texels) {
    if (texels instanceof Uint8Array) { return 255; }
    if (texels instanceof Uint16Array) { return 65535; }
    throw new Error('the distance transform takes a Uint8Array or a Uint16Array');
}

// Uint32Array [nz][ny][nx]: d2 of every voxel.  Separable: per axis out[i] = min over the finite g[j] of g[j] + (i - j)^2
function distanceSquaredTexels(texels, nx, ny, nz, lo, hi, seeds) {
    checkRange(lo, hi, largestCode(texels));
    const rest = checkSeeds(seeds !== undefined ? seeds : 'range') === 1;
    const n = nx * ny * nz;
    if (texels.length !== n || n < 1) { throw new Error('texels are [nz][ny][nx]'); }
    let g = new Float64Array(n);
    for (let i = 0; i < n; i++) { g[i] = ((texels[i] >= lo && texels[i] <= hi) !== rest) ? 0 : Infinity; }
    const axes = [[nx, 1], [ny, nx], [nz, nx * ny]];           // length and stride of the lines of an axis
    for (const [m, step] of axes) {
        const out = new Float64Array(n);
        for (let base = 0; base < n; base++) {
            if (Math.floor(base / step) % m !== 0) { continue; }   // not a line's first voxel
            for (let i = 0; i < m; i++) {
                let best = Infinity;
                for (let j = 0; j < m; j++) { best = Math.min(best, g[base + j * step] + (i - j) * (i - j)); }
                out[base + i * step] = best;
            }
        }
        g = out;
    }
    const d2 = new Uint32Array(n);
    for (let i = 0; i < n; i++) { d2[i] = g[i] === Infinity ? NONE : g[i]; }
    return d2;
}

// the codes where r2Lo <= d2 <= r2Hi, `fill` elsewhere, in the texels' type
function withinTexels(texels, d2, r2Lo, r2Hi, fill) {
    const k = checkWithin(r2Lo !== undefined ? r2Lo : 0, r2Hi, fill !== undefined ? fill : 0, largestCode(texels));
    if (d2.length !== texels.length) { throw new Error('squared distances are one per voxel'); }
    const out = new texels.constructor(texels.length);
    for (let i = 0; i < out.length; i++) { out[i] = d2[i] >= k[0] && d2[i] <= k[1] ? texels[i] : k[2]; }
    return out;
}

// floor(sqrt(p)) for an integer 0 <= p < 2^53, exactly
function isqrt(p) {
    let r = Math.floor(Math.sqrt(p));
    if (r * r > p) { r--; }
    if ((r + 1) * (r + 1) <= p) { r++; }
    return r;
}

// interleaved (code, min(isqrt(steps^2 d2), M)) in the texels' type, M its largest code
function channelTexels(texels, d2, steps) {
    const M = largestCode(texels);
    steps = checkSteps(steps !== undefined ? steps : 1);
    if (d2.length !== texels.length) { throw new Error('squared distances are one per voxel'); }
    const out = new texels.constructor(2 * texels.length);
    for (let i = 0; i < texels.length; i++) { out[2 * i] = texels[i]; out[2 * i + 1] = Math.min(isqrt(steps * steps * d2[i]), M); }
    return out;
}

module.exports = { distanceSquaredTexels, withinTexels, channelTexels, isqrt, checkSeeds, checkSteps, checkRadius, checkWithin, checkDistanceRange: checkRange, DISTANCE_NONE: NONE };
