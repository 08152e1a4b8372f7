'use strict';
// node js/test/test_watershed_gpu.js OUT — GPU: the Node.js host's watershed.  Three shapes (one voxel more than a 64 x 8 x 4 tile on every
// axis; three tiles on every axis; odd everywhere), uint8 and uint16, through Volume.watershed (both polarities, a two-channel relief, texels
// given), the timed and capped forms and Volume.split: the ranks and the list must equal the plain-JS twin of the contract
// (js/vpt/watershed.js).  Then RenderingContext({ split }) once: the source and the texels of what the context ends up with are written to
// OUT (tests/test_js_gpu_watershed.py compares them with the numpy chain).
const fs = require('fs');
const vpt = require('../vpt/index.js');
const { native } = require('../vpt/native.js');

const SHAPES = [[65, 9, 5], [130, 17, 9], [7, 5, 3]];
const NX = 28, NY = 16, NZ = 16;

function equal(a, b, what) {
    if (a.constructor !== b.constructor || a.length !== b.length) { throw new Error(what + ': wrong array'); }
    for (let i = 0; i < a.length; i++) { if (a[i] !== b[i]) { throw new Error(`${what}: element ${i} is ${a[i]}, expected ${b[i]}`); } }
}
function throws(f, what, pattern) {
    let message = null;
    try { f(); } catch (e) { message = e.message; }
    if (message === null) { throw new Error(what + ' was accepted'); }
    if (pattern && !pattern.test(message)) { throw new Error(what + ': unexpected message ' + message); }
}
// the handle against the twin's { ranks, list }; destroys the handle
function held(basins, want, what) {
    try {
        equal(basins.ranks(), want.ranks, what);
        if (JSON.stringify(basins.list()) !== JSON.stringify(want.list)) { throw new Error(what + ': the list differs'); }
        if (basins.info.listed !== want.list.length) { throw new Error(what + ': info.listed'); }
    } finally { basins.destroy(); }
}
// the worked example of the contract: two balls of radius 6 around x = 9 and x = secondX in a 28 x 16 x 16 grid, code 200
function twoBalls(secondX) {
    const v = new Uint8Array(NX * NY * NZ);
    for (let z = 0, i = 0; z < NZ; z++) { for (let y = 0; y < NY; y++) { for (let x = 0; x < NX; x++, i++) {
        const r = (y - 8) * (y - 8) + (z - 8) * (z - 8);
        if ((x - 9) * (x - 9) + r <= 36 || (x - secondX) * (x - secondX) + r <= 36) { v[i] = 200; }
    } } }
    return v;
}

async function main() {
    const outPath = process.argv[2];
    const N = native();
    const ctx = new vpt.Context(0);
    if (!ctx.getExtension('EXT_texture_norm16')) { throw new Error('no EXT_texture_norm16'); }
    let seed = 86421;
    const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
    const uploadTo = async (texels, bits, dims) => {
        const v = new vpt.Volume(ctx, new vpt.RAWReader(new Uint8Array(texels.buffer), { width: dims[0], height: dims[1], depth: dims[2], bits: bits }));
        await v.load();
        return v;
    };
    for (const dims of SHAPES) {
        const [nx, ny, nz] = dims, n = nx * ny * nz, whole = [0, 0, 0, nx, ny, nz];
        for (const bits of [8, 16]) {
            const Ctor = bits === 8 ? Uint8Array : Uint16Array, M = bits === 8 ? 255 : 65535, codes = [0, M >> 2, M >> 1, M - (M >> 2), M];
            const a = new Ctor(n), b = new Ctor(n);
            for (let i = 0; i < n; i++) { a[i] = rand() & M; b[i] = codes[rand() % codes.length]; }      // noise; five codes, so that plateaus occur
            const va = await uploadTo(a, bits, dims), vb = await uploadTo(b, bits, dims);
            const pair = vb.pair(va), two = pair.readBlock.apply(pair, whole);                            // (b, a), made on the device
            for (const connectivity of [6, 18, 26]) {
                for (const polarity of ['minima', 'maxima']) {
                    const what = `${polarity} under ${connectivity}, ${bits} bits, ${dims}`;
                    held(va.watershed(0, M, { polarity, connectivity }), vpt.watershedTexels(a, dims, 0, M, { polarity, connectivity }), what + ', noise');
                    held(vb.watershed(M >> 3, M, { polarity, connectivity, minVoxels: 2 }),
                        vpt.watershedTexels(b, dims, M >> 3, M, { polarity, connectivity, minVoxels: 2 }), what + ', plateaus');
                    for (const channel of [0, 1]) {
                        held(pair.watershed(0, M - (M >> 3), { polarity, connectivity, channel }),
                            vpt.watershedTexels(two, dims, 0, M - (M >> 3), { polarity, connectivity, channels: 2, channel }), what + ', channel ' + channel);
                    }
                }
            }
            // texels given: the emitters speak of the other volume; a channel of a two-channel relief is a one-channel snapshot
            const want = vpt.watershedTexels(two, dims, 0, M, { connectivity: 18, channels: 2, channel: 1 });
            let basins = pair.watershed(0, M, { connectivity: 18, channel: 1, texels: vb });
            let kept = basins.keep(1, 2, 7);
            equal(kept.readBlock.apply(kept, whole), vpt.keepTexels(b, want.ranks, 1, 2, 7), 'keep emits the codes of `texels`');
            kept.destroy(); basins.destroy();
            basins = pair.watershed(0, M, { connectivity: 18, channel: 1 });
            kept = basins.keep(1, 2, 7);
            if (kept.nativeFormat() !== va.nativeFormat()) { throw new Error('the snapshot has one channel'); }
            equal(kept.readBlock.apply(kept, whole), vpt.keepTexels(a, want.ranks, 1, 2, 7), 'keep emits the chosen channel');
            const labelled = basins.label();
            equal(labelled.readBlock.apply(labelled, whole), vpt.labelTexels(a, want.ranks), 'label');
            kept.destroy(); labelled.destroy(); basins.destroy();
            // the timed and capped forms
            const timed = vb.watershedTimed(0, M, { connectivity: 26 }), twin = vpt.watershedTexels(b, dims, 0, M, { connectivity: 26 });
            if (!(timed[1].ms.classify > 0) || !(timed[1].ms.links > 0) || !(timed[1].plateauLaunches >= 0)) { throw new Error('watershedTimed: ' + JSON.stringify(timed[1])); }
            held(timed[0], twin, 'watershedTimed');
            const capped = vb.watershedTimed(0, M, { connectivity: 26, caps: [3, 1, 1] });
            if (!(capped[1].plateauLaunches >= timed[1].plateauLaunches)) { throw new Error('capped: fewer plateau launches'); }
            held(capped[0], twin, 'the smallest caps');
            equal(va.readBlock.apply(va, whole), a, 'the relief afterwards'); equal(vb.readBlock.apply(vb, whole), b, 'the other volume afterwards');
            throws(() => va.watershed(0, M, { polarity: 'both' }), "polarity 'both'", /polarity/);
            throws(() => va.watershed(0, M, { connectivity: 8 }), 'connectivity 8', /connectivity/);
            throws(() => va.watershed(0, M, { channel: 1 }), 'channel 1 of a one-channel volume', /channel 1/);
            throws(() => va.watershed(0, M, { passes: 2 }), 'an unknown option', /passes/);
            throws(() => va.watershed(0, M, { caps: [3, 1, 1] }), 'caps outside the timed form', /caps/);
            throws(() => va.watershed(3, 2), 'lo above hi', /range/);
            throws(() => va.watershed(0, M, { minVoxels: 0 }), 'minVoxels 0', /minVoxels/);
            throws(() => va.watershed(0, M, { texels: {} }), 'texels that are no volume', /ready volume/);
            throws(() => va.watershedTimed(0, M, { caps: [2, 1, 1] }), 'the library: merge_steps 2', /merge_steps 2/);
            throws(() => va.watershedTimed(0, M, { caps: [3, 1, 0] }), 'the library: tile_rounds 0', /tile_rounds 0/);
            throws(() => N.volumeWatershed(va.texture, 0, null, 0, M, 2, 6, 1), 'the library: polarity 2', /polarity 2/);
            throws(() => va.watershed(0, M, { texels: pair }), 'the library: two-channel texels', /texels/);
            throws(() => va.split(1, M, { depth: 3 }), 'an unknown split option', /depth/);
            for (const vol of [pair, va, vb]) { vol.destroy(); }
        }
    }
    // the worked example, end to end on the device
    const dims = [NX, NY, NZ], balls = twoBalls(19), v = await uploadTo(balls, 8, dims);
    const wantSplit = vpt.splitTexels(balls, dims, 100, 255);
    if (JSON.stringify(wantSplit.list) !== JSON.stringify([[9, 8, 2, 924], [19, 8, 2, 887]])) { throw new Error('the twin: ' + JSON.stringify(wantSplit.list)); }
    const parts = v.split(100, 255);
    if (parts.info.foregroundVoxels !== 1811) { throw new Error('split: info ' + JSON.stringify(parts.info)); }
    const second = parts.keep(2, 2);
    equal(second.readBlock(0, 0, 0, NX, NY, NZ), vpt.keepTexels(balls, wantSplit.ranks, 2, 2, 0), 'split: keep emits the original codes');
    second.destroy();
    held(parts, wantSplit, 'split');
    const timedSplit = v.splitTimed(100, 255, { h: 4 });
    if (!(timedSplit[1].ms.links > 0)) { throw new Error('splitTimed: ' + JSON.stringify(timedSplit[1])); }
    held(timedSplit[0], vpt.splitTexels(balls, dims, 100, 255, { h: 4 }), 'splitTimed');
    const near = await uploadTo(twoBalls(17), 8, dims);
    for (const [h, sizes] of [[2, [887, 818]], [4, [1705]]]) {
        const p = near.split(100, 255, { h });
        if (JSON.stringify(p.list().map(b => b[3])) !== JSON.stringify(sizes)) { throw new Error(`the nearer pair, h ${h}: ${JSON.stringify(p.list())}`); }
        p.destroy();
    }
    near.destroy(); v.destroy();
    ctx.destroy();
    // the context path
    for (const bad of ['split', {}, { lo: 2, hi: 1 }, { lo: 1, hi: 2, connectivity: 7 }]) {
        throws(() => new vpt.RenderingContext({ split: bad }), 'RenderingContext({ split: ' + JSON.stringify(bad) + ' })');
    }
    throws(() => new vpt.RenderingContext({ split: { lo: 1, hi: 2 }, gradient: 'central' }), 'split with gradient', /second channel/);
    const rc = new vpt.RenderingContext({ resolution: { width: 72, height: 52 }, split: { lo: 100, hi: 300 } });      // hi is open above
    await rc.setVolume(new vpt.RAWReader(balls, { width: NX, height: NY, depth: NZ }));
    if (rc.volume.nativeFormat() !== N.VPT_FORMAT_RG8) { throw new Error('RenderingContext did not split'); }
    const tex = rc.volume.readBlock(0, 0, 0, NX, NY, NZ);
    rc.chooseRenderer('mip');
    rc.renderer.render();
    rc.destroy();
    fs.writeFileSync(outPath, Buffer.concat([Buffer.from(balls.buffer), Buffer.from(tex.buffer)]));
    console.log('js watershed gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
