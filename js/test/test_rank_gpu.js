'use strict';
// node js/test/test_rank_gpu.js OUT — GPU: the Node.js host's rank filters.  A (23, 19, 21) volume of uniform noise, uint8 and uint16,
// through Volume.rank('median', 2) and Volume.rank('close', 1) (and the conveniences): the texels read back (readBlock) must equal a
// plain-JS restatement of the contract of include/vpt.h.  Then RenderingContext({ window, rank, smooth, reduce, gradient }) once over a
// signed 16-bit RAW volume: the texels of what the context ends up with are written to OUT (tests/test_js_gpu_rank.py compares them with
// the numpy chain).
const fs = require('fs');
const vpt = require('../vpt/index.js');
const GL = require('../vpt/readers/readers.js');
const { native } = require('../vpt/native.js');

const NX = 21, NY = 19, NZ = 23;
const clamp = (i, n) => Math.min(Math.max(i, 0), n - 1);

// one pass: the 27 clamped taps of every texel, sorted as numbers; rank 13 is the median, 0 the erosion, 26 the dilation
function rankPass(v, nx, ny, nz, rank, Ctor) {
    const out = new Ctor(nx * ny * nz), taps = new Array(27);
    for (let z = 0; z < nz; z++) { for (let y = 0; y < ny; y++) { for (let x = 0; x < nx; x++) {
        let n = 0;
        for (let c = -1; c <= 1; c++) { for (let b = -1; b <= 1; b++) { for (let a = -1; a <= 1; a++) {
            taps[n++] = v[(clamp(z + c, nz) * ny + clamp(y + b, ny)) * nx + clamp(x + a, nx)];
        } } }
        taps.sort((p, q) => p - q);
        out[(z * ny + y) * nx + x] = taps[rank];
    } } }
    return out;
}
function rankTexels(v, nx, ny, nz, op, passes, Ctor) {
    const ranks = { median: [13], erode: [0], dilate: [26], open: [0, 26], close: [26, 0] }[op];
    let cur = v;
    for (const rank of ranks) { for (let p = 0; p < passes; p++) { cur = rankPass(cur, nx, ny, nz, rank, Ctor); } }
    return cur;
}
function equal(a, b, what) {
    if (a.constructor !== b.constructor || a.length !== b.length) { throw new Error(what + ': wrong array'); }
    for (let i = 0; i < a.length; i++) { if (a[i] !== b[i]) { throw new Error(`${what}: texel ${i} is ${a[i]}, expected ${b[i]}`); } }
}
function throws(f, what) {
    let threw = false;
    try { f(); } catch (e) { threw = true; }
    if (!threw) { throw new Error(what + ' was accepted'); }
}

async function main() {
    const outPath = process.argv[2];
    const N = native();
    const ctx = new vpt.Context(0);
    if (!ctx.getExtension('EXT_texture_norm16')) { throw new Error('no EXT_texture_norm16'); }
    let seed = 54321;
    const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
    for (const bits of [8, 16]) {
        const Ctor = bits === 8 ? Uint8Array : Uint16Array;
        const texels = new Ctor(NX * NY * NZ);
        for (let i = 0; i < texels.length; i++) { texels[i] = rand() & (bits === 8 ? 255 : 65535); }
        const v = new vpt.Volume(ctx, new vpt.RAWReader(new Uint8Array(texels.buffer), { width: NX, height: NY, depth: NZ, bits: bits }));
        await v.load();
        const m = v.rank('median', 2), c = v.rank('close'), e = v.erode(2);
        for (const d of [m, c, e]) {
            if (!d.ready || d.nativeFormat() !== v.nativeFormat() || d.modality.dimensions.width !== NX) { throw new Error('derived volumes change the format'); }
        }
        const got = m.readBlock(0, 0, 0, NX, NY, NZ);
        equal(got, rankTexels(texels, NX, NY, NZ, 'median', 2, Ctor), `rank('median', 2), ${bits} bits`);
        let changed = 0;
        for (let i = 0; i < got.length; i++) { if (got[i] !== texels[i]) { changed++; } }
        if (changed * 2 < got.length) { throw new Error("rank('median', 2) changes fewer than half of the texels"); }
        equal(c.readBlock(0, 0, 0, NX, NY, NZ), rankTexels(texels, NX, NY, NZ, 'close', 1, Ctor), `rank('close'), ${bits} bits`);
        equal(e.readBlock(0, 0, 0, NX, NY, NZ), rankTexels(texels, NX, NY, NZ, 'erode', 2, Ctor), `erode(2), ${bits} bits`);
        equal(v.readBlock(0, 0, 0, NX, NY, NZ), texels, 'the source afterwards');
        for (const name of ['median', 'erode', 'dilate', 'open', 'close']) {
            const a = v[name](), b = v.rank(name, 1);
            equal(a.readBlock(0, 0, 0, NX, NY, NZ), b.readBlock(0, 0, 0, NX, NY, NZ), name + '()');
            a.destroy(); b.destroy();
        }
        for (const bad of [0, 9, 1.5, '1', null, true]) { throws(() => v.rank('median', bad), "rank('median', " + JSON.stringify(bad) + ')'); }
        for (const bad of ['mean', 'Median', 0, null, undefined]) { throws(() => v.rank(bad, 1), 'rank(' + JSON.stringify(bad) + ')'); }
        const g = v.deriveGradient({ operator: 'central' });
        let named = '';
        try { g.rank('median', 1); } catch (err) { named = err.message; }     // a two-channel source: the library names the format
        if (!/RG(8|16)/.test(named)) { throw new Error('rank of a two-channel volume: ' + named); }
        for (const vol of [g, m, c, e, v]) { vol.destroy(); }
    }
    ctx.destroy();
    // the context path
    for (const bad of ['mean', 0, true]) { throws(() => new vpt.RenderingContext({ rank: bad }), 'RenderingContext({ rank: ' + JSON.stringify(bad) + ' })'); }
    for (const bad of [0, 9, 1.5, '1', true]) { throws(() => new vpt.RenderingContext({ rank: 'median', rankPasses: bad }), 'RenderingContext({ rankPasses: ' + JSON.stringify(bad) + ' })'); }
    const ct = new Int16Array(NX * NY * NZ);
    for (let i = 0; i < ct.length; i++) { ct[i] = (rand() % 4001) - 1000; }
    const rc = new vpt.RenderingContext({ resolution: { width: 72, height: 52 }, window: [-200, 400], windowFormat: 'r16', rank: 'median', rankPasses: 2,
        smooth: 1, reduce: 1, gradient: 'sobel', gradientGain: 2 });
    rc.gl.getExtension('EXT_texture_norm16');
    await rc.setVolume(new vpt.RAWReader(new Uint8Array(ct.buffer), { width: NX, height: NY, depth: NZ, bits: 16, signed: true }));
    if (rc.volume.nativeFormat() !== N.VPT_FORMAT_RG16 || rc.volume.modality.internalFormat !== GL.GL_RG16_EXT) { throw new Error('RenderingContext did not run the chain'); }
    const tex = rc.volume.readBlock(0, 0, 0, 11, 10, 12);
    rc.chooseRenderer('mip');
    rc.renderer.render();
    rc.destroy();
    fs.writeFileSync(outPath, Buffer.concat([Buffer.from(ct.buffer), Buffer.from(tex.buffer)]));
    console.log('js rank gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
