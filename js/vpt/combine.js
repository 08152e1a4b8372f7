'use strict';
// Two volumes of one grid combined texel by texel, or compared, in plain JS: the contract of include/vpt.h ("two volumes combined or
// compared") restated for hosts without a device, the twin of vpt_amd/combine.py.  a: a Uint8Array or Uint16Array of [nz][ny][nx] texels; b:
// one of `channels` (1 or 2) interleaved channels of which `channel` is read.  A and B are the whole unsigned codes, M = 255 / 65535 the
// largest code of a's type, Mb that of b's.
//   mask:    A where lo <= B <= hi, `fill` elsewhere.  b may be 8- or 16-bit whatever a is.  lo <= hi <= Mb, fill <= M.
//   min, max, absdiff:  min(A, B), max(A, B), |A - B|.
//   blend:   clamp(((wa A + wb B + 128) >> 8) + offset, 0, M): wa, wb in 1/256 units in -4096 .. 4096, offset in -65535 .. 65535.
//            |wa A + wb B + 128| < 2^31, so `| 0` and `>> 8` (the arithmetic shift: a half rounds up) are exact.
//   pair:    (A, B) interleaved, in a's type.
// Every op but mask needs b to have a's type.
const OPS = ['mask', 'min', 'max', 'absdiff', 'blend', 'pair'];
const MAX_WEIGHT = 4096;
const MAX_OFFSET = 65535;
const STATS = ['voxels', 'differing', 'maxAbs', 'sumAbs', 'sumSq', 'inA', 'inB', 'both'];

// the code of 'mask' | 'min' | 'max' | 'absdiff' | 'blend' | 'pair' (VPT_COMBINE_*)
function checkOp(op) {
    const code = typeof op === 'string' ? OPS.indexOf(op) : -1;
    if (code < 0) { throw new Error("combine op is 'mask', 'min', 'max', 'absdiff', 'blend' or 'pair', not " + JSON.stringify(op)); }
    return code;
}
// `channel` of a volume of `channels` channels: 0, or 1 for a two-channel volume
function checkChannel(channel, channels) {
    if (channel !== 0 && channel !== 1) { throw new Error('combine channel is 0 or 1, not ' + JSON.stringify(channel)); }
    if (channel === 1 && channels !== 2) { throw new Error('combine channel 1 needs a two-channel second volume'); }
    return channel;
}
// [wa, wb, offset] of a blend: the weights in -4096 .. 4096 (1/256 units), the offset in -65535 .. 65535
function checkWeights(wa, wb, offset) {
    offset = offset !== undefined ? offset : 0;
    [['wa', wa], ['wb', wb]].forEach(([name, w]) => {
        if (!Number.isInteger(w) || w < -MAX_WEIGHT || w > MAX_WEIGHT) {
            throw new Error(`blend weight ${name} is an integer in -${MAX_WEIGHT} .. ${MAX_WEIGHT} (1/256 units), not ${JSON.stringify(w)}`);
        }
    });
    if (!Number.isInteger(offset) || offset < -MAX_OFFSET || offset > MAX_OFFSET) {
        throw new Error(`blend offset is an integer in -${MAX_OFFSET} .. ${MAX_OFFSET}, not ${JSON.stringify(offset)}`);
    }
    return [wa, wb, offset];
}
// [lo, hi, fill] of a mask: 0 <= lo <= hi <= largestB and 0 <= fill <= largestA
function checkMask(lo, hi, fill, largestB, largestA) {
    if (!Number.isInteger(lo) || !Number.isInteger(hi) || !(lo >= 0 && lo <= hi && hi <= largestB)) {
        throw new Error(`mask range [${JSON.stringify(lo)}, ${JSON.stringify(hi)}]: integers with 0 <= lo <= hi <= ${largestB}`);
    }
    if (!Number.isInteger(fill) || fill < 0 || fill > largestA) { throw new Error(`mask fill is an integer in 0 .. ${largestA}, not ${JSON.stringify(fill)}`); }
    return [lo, hi, fill];
}
// [lo, hi] of a compare range (null / undefined: every code): integers in 0 .. 2^32 - 1 with lo <= hi
function checkCompareRange(range, largest, which) {
    if (range === undefined || range === null) { return [0, largest]; }
    if (!Array.isArray(range) || range.length !== 2 || !Number.isInteger(range[0]) || !Number.isInteger(range[1]) ||
        !(range[0] >= 0 && range[0] <= range[1] && range[1] <= 0xFFFFFFFF)) {
        throw new Error(`compare ${which} is null or [lo, hi], integers with 0 <= lo <= hi, not ${JSON.stringify(range)}`);
    }
    return [range[0], range[1]];
}
function largestCode(texels, what) {
    if (texels instanceof Uint8Array) { return 255; }
    if (texels instanceof Uint16Array) { return 65535; }
    throw new Error(what + ' is a Uint8Array or a Uint16Array');
}
function checkSources(a, b, channels, channel) {
    const M = largestCode(a, 'the first volume'), Mb = largestCode(b, 'the second volume');
    channels = channels !== undefined ? channels : 1;
    if (channels !== 1 && channels !== 2) { throw new Error('the second volume has 1 or 2 channels, not ' + JSON.stringify(channels)); }
    if (b.length !== a.length * channels) { throw new Error(`the volumes differ in size: ${a.length} and ${b.length / channels} texels`); }
    return [M, Mb, channels, checkChannel(channel !== undefined ? channel : 0, channels)];
}

// the texels vpt_volume_combine gives: options = { channels, channel, lo, hi, fill, wa, wb, offset } (hi undefined: b's largest code)
function combineTexels(a, b, op, options) {
    options = options || {};
    const code = checkOp(op);
    const [M, Mb, channels, channel] = checkSources(a, b, options.channels, options.channel);
    const n = a.length, B = (i) => b[i * channels + channel];
    if (op !== 'mask' && M !== Mb) { throw new Error(`combine op '${op}' needs volumes of one width; only 'mask' takes both`); }
    const out = new a.constructor(op === 'pair' ? 2 * n : n);
    if (op === 'mask') {
        const [lo, hi, fill] = checkMask(options.lo !== undefined ? options.lo : 0, options.hi !== undefined && options.hi !== null ? options.hi : Mb,
            options.fill !== undefined ? options.fill : 0, Mb, M);
        for (let i = 0; i < n; i++) { const v = B(i); out[i] = v >= lo && v <= hi ? a[i] : fill; }
    } else if (op === 'min') {
        for (let i = 0; i < n; i++) { out[i] = Math.min(a[i], B(i)); }
    } else if (op === 'max') {
        for (let i = 0; i < n; i++) { out[i] = Math.max(a[i], B(i)); }
    } else if (op === 'absdiff') {
        for (let i = 0; i < n; i++) { out[i] = Math.abs(a[i] - B(i)); }
    } else if (op === 'pair') {
        for (let i = 0; i < n; i++) { out[2 * i] = a[i]; out[2 * i + 1] = B(i); }
    } else {
        if (code !== 4) { throw new Error('unreachable'); }
        const [wa, wb, offset] = checkWeights(options.wa !== undefined ? options.wa : 256, options.wb !== undefined ? options.wb : 0, options.offset);
        for (let i = 0; i < n; i++) {
            const s = (((Math.imul(wa, a[i]) + Math.imul(wb, B(i)) + 128) | 0) >> 8) + offset;
            out[i] = Math.min(Math.max(s, 0), M);
        }
    }
    return out;
}

// num / den as the correctly rounded double (what Python's int / int gives): the quotient scaled by 2^128 has more than 64 bits, its last
// bit made sticky by a remainder; Number() rounds it once and the division by 2^128 is exact
function quotient(num, den) {
    const scaled = num << 128n;
    let q = scaled / den;
    if (q * den !== scaled) { q |= 1n; }
    return Number(q) / 2 ** 128;
}
// { dice, jaccard, mse, psnr } from the eight counts (Numbers or BigInts), in IEEE double; null where a denominator is 0 (psnr: where mse
// is 0).  largest: the peak of the PSNR, the largest code of the wider of the two volumes
function ratios(stats, largest) {
    const voxels = Number(stats.voxels), inA = Number(stats.inA), inB = Number(stats.inB), both = Number(stats.both);
    const union = inA + inB - both;
    const mse = voxels ? quotient(BigInt(stats.sumSq), BigInt(stats.voxels)) : null;
    return { dice: inA + inB ? 2 * both / (inA + inB) : null, jaccard: union ? both / union : null, mse,
        psnr: mse ? 10.0 * Math.log10(largest * largest / mse) : null };
}

// vpt_volume_compare's eight exact integers as BigInts (sumSq can pass 2^53) plus the ratios: options = { channels, channel, aRange, bRange }
function compareStats(a, b, options) {
    options = options || {};
    const [M, Mb, channels, channel] = checkSources(a, b, options.channels, options.channel);
    const [loA, hiA] = checkCompareRange(options.aRange, M, 'aRange'), [loB, hiB] = checkCompareRange(options.bRange, Mb, 'bRange');
    let differing = 0, maxAbs = 0, inA = 0, inB = 0, both = 0, sumAbs = 0n, sumSq = 0n;
    for (let i = 0; i < a.length; i++) {
        const A = a[i], B = b[i * channels + channel], d = Math.abs(A - B);
        const ia = A >= loA && A <= hiA, ib = B >= loB && B <= hiB;
        if (d) { differing++; sumAbs += BigInt(d); sumSq += BigInt(d * d); }        // d^2 <= 65535^2 < 2^53
        if (d > maxAbs) { maxAbs = d; }
        if (ia) { inA++; }
        if (ib) { inB++; }
        if (ia && ib) { both++; }
    }
    const stats = { voxels: BigInt(a.length), differing: BigInt(differing), maxAbs: BigInt(maxAbs), sumAbs, sumSq, inA: BigInt(inA), inB: BigInt(inB), both: BigInt(both) };
    return Object.assign(stats, ratios(stats, Math.max(M, Mb)));
}

module.exports = { COMBINE_OPS: OPS, COMBINE_STATS: STATS, checkCombineOp: checkOp, checkCombineChannel: checkChannel, checkCombineWeights: checkWeights,
    checkCombineMask: checkMask, checkCompareRange, combineTexels, compareStats, compareRatios: ratios };
