'use strict';
// node js/test/test_measure_gpu.js — GPU: the Node.js host's per-component measurements and set selection.  One (65, 9, 9) volume of
// uniform noise per width (one voxel past the measuring kernel's 64 x 8 x 8 box on every axis) and the 3-D checkerboard of the same shape
// (every voxel its own component: more distinct ranks in a box than its table has slots), labelled on the device (Volume.components):
// Components.measure (the whole list, a window, another volume of the other width as values, a two-channel volume) and Components.keepSet
// (a subset with duplicates and ranks beyond the list, a boolean mask, the empty set, an interval against keep) must equal the plain-JS
// twin of the contract (js/vpt/measure.js) over the ranks read back from the device.
const vpt = require('../vpt/index.js');

const NX = 65, NY = 9, NZ = 9;

function equal(a, b, what) {
    if (a.constructor !== b.constructor || a.length !== b.length) { throw new Error(what + ': wrong array'); }
    for (let i = 0; i < a.length; i++) { if (a[i] !== b[i]) { throw new Error(`${what}: texel ${i} is ${a[i]}, expected ${b[i]}`); } }
}
function sameRecords(got, want, what) {
    if (got.length !== want.length) { throw new Error(`${what}: ${got.length} records, expected ${want.length}`); }
    got.forEach((r, k) => { for (const f of vpt.MEASURE_FIELDS) {
        if (r[f] !== want[k][f]) { throw new Error(`${what}: record ${k}, ${f} is ${r[f]}, expected ${want[k][f]}`); }
    } });
}
function throws(f, what, pattern) {
    let message = null;
    try { f(); } catch (e) { message = e.message; }
    if (message === null) { throw new Error(what + ' was accepted'); }
    if (pattern && !pattern.test(message)) { throw new Error(what + ': unexpected message ' + message); }
}

async function main() {
    const ctx = new vpt.Context(0);
    if (!ctx.getExtension('EXT_texture_norm16')) { throw new Error('no EXT_texture_norm16'); }
    let seed = 97531;
    const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
    const n = NX * NY * NZ, whole = [0, 0, 0, NX, NY, NZ];
    const upload = async (texels, bits) => {
        const v = new vpt.Volume(ctx, new vpt.RAWReader(new Uint8Array(texels.buffer), { width: NX, height: NY, depth: NZ, bits: bits }));
        await v.load();
        return v;
    };
    const cases = [];
    for (const bits of [8, 16]) {
        const Ctor = bits === 8 ? Uint8Array : Uint16Array, M = bits === 8 ? 255 : 65535;
        const a = new Ctor(n);
        for (let i = 0; i < n; i++) { a[i] = rand() & M; }
        cases.push([`noise, ${bits} bits`, bits, a, 0, Math.round(0.30 * (M + 1)) - 1]);
    }
    const board = new Uint8Array(n);
    for (let z = 0, i = 0; z < NZ; z++) { for (let y = 0; y < NY; y++) { for (let x = 0; x < NX; x++, i++) { board[i] = (x + y + z) % 2 === 0 ? 200 : 0; } } }
    cases.push(['checkerboard', 8, board, 200, 255]);
    for (const [what, bits, a, lo, hi] of cases) {
        const Other = bits === 8 ? Uint16Array : Uint8Array, Mo = bits === 8 ? 65535 : 255;
        const o = new Other(n);
        for (let i = 0; i < n; i++) { o[i] = rand() & Mo; }
        const va = await upload(a, bits), vo = await upload(o, 24 - bits);
        const found = va.components(lo, hi, 6, 1);
        const ranks = found.ranks(), listed = found.info.listed;
        equal(ranks, vpt.componentsTexels(a, NX, NY, NZ, lo, hi, 6, 1).ranks, what + ': ranks');
        if (what === 'checkerboard' ? listed !== (n + 1) / 2 : listed < 64) { throw new Error(`${what}: degenerate input, ${listed} components`); }
        const all = found.measure();
        sameRecords(all, vpt.measureTexels(ranks, a, NX, NY, NZ, 0, listed), what);
        if (typeof all[0].voxels !== 'bigint' || typeof all[0].valueSumSq !== 'bigint' || typeof all[0].minX !== 'number') { throw new Error(what + ': field types'); }
        sameRecords(found.measure(3, 11), all.slice(3, 14), what + ': a window');
        sameRecords(found.measure(listed, 0), [], what + ': an empty window');
        sameRecords(found.measure(0, undefined, vo), vpt.measureTexels(ranks, o, NX, NY, NZ, 0, listed), what + ': values of the other width');
        const pair = va.pair(va);                                  // a two-channel volume made on the device: (a, a)
        sameRecords(found.measure(0, 5, pair, 1), all.slice(0, 5), what + ': channel 1 of a pair');
        pair.destroy();
        const timed = found.measureTimed(1, 4);
        sameRecords(timed[0], all.slice(1, 5), what + ': measureTimed');
        if (!(timed[1] > 0)) { throw new Error('measureTimed: no time'); }
        throws(() => found.measure(listed, 1), 'a window past the list', /not within/);
        throws(() => found.measure(0, 1, vo, 1), 'channel 1 of one', /channel 1/);
        const d = vpt.derive(all.slice(0, 3));
        if (!(d[0].fill > 0 && d[0].fill <= 1 && d[0].variance >= 0 && d[0].extentX >= 1)) { throw new Error(what + ': derive'); }
        // keepSet
        const chosen = [];
        for (let r = 2; r <= listed; r += 3) { chosen.push(r); }
        const mask = new Array(listed).fill(false);
        chosen.forEach(r => { mask[r - 1] = true; });
        const sets = [['a subset', chosen.concat(chosen.slice(0, 3), [listed + 5, 2 ** 40, BigInt(listed) + 9n]), 7], ['a mask', mask, 7], ['the empty set', [], 5]];
        for (const [name, selected, fill] of sets) {
            const kept = found.keepSet(selected, fill);
            if (!kept.ready || kept.nativeFormat() !== va.nativeFormat()) { throw new Error(`${what}, ${name}: wrong description`); }
            equal(kept.readBlock.apply(kept, whole), vpt.keepSetTexels(a, ranks, selected, fill), `${what}: keepSet, ${name}`);
            kept.destroy();
        }
        const interval = [];
        for (let r = 2; r <= Math.min(9, listed); r++) { interval.push(r); }
        const bySet = found.keepSet(interval, 1), byInterval = found.keep(2, Math.min(9, listed), 1);
        equal(bySet.readBlock.apply(bySet, whole), byInterval.readBlock.apply(byInterval, whole), what + ': an interval against keep');
        bySet.destroy(); byInterval.destroy();
        throws(() => found.keepSet([0]), 'rank 0', /1-based/);
        throws(() => found.keepSet([1], 65536), 'fill', /fill/);
        equal(va.readBlock.apply(va, whole), a, what + ': the source afterwards');
        found.destroy(); va.destroy(); vo.destroy();
        throws(() => found.measure(), 'a destroyed handle', /destroyed/);
    }
    ctx.destroy();
    console.log('js measure gpu ok');
}
main().catch(e => { console.error(e.stack || String(e)); process.exit(1); });
