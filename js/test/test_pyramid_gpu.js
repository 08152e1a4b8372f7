'use strict';
// node js/test/test_pyramid_gpu.js OUT — GPU: the Node.js host's 2x reduction and binomial smoothing.  A (23, 19, 21) volume of uniform noise,
// uint8 and uint16, through Volume.reduce() and Volume.smooth(2): the texels read back (readBlock) must equal a plain-JS restatement of the
// two integer contracts of include/vpt.h.  Then RenderingContext({ window, smooth, reduce, gradient }) once over a signed 16-bit RAW volume:
// the texels of what the context ends up with are written to OUT (tests/test_js_gpu_pyramid.py compares them with the numpy chain).
const fs = require('fs');
const vpt = require('../vpt/index.js');
const GL = require('../vpt/readers/readers.js');
const { native } = require('../vpt/native.js');

const NX = 21, NY = 19, NZ = 23;
const clamp = (i, n) => Math.min(Math.max(i, 0), n - 1);

// out = (sum of the eight codes + 4) >> 3 over x in {2 X, min(2 X + 1, nx - 1)}, likewise y and z
function reduceTexels(v, nx, ny, nz, Ctor) {
    const rx = (nx + 1) >> 1, ry = (ny + 1) >> 1, rz = (nz + 1) >> 1, out = new Ctor(rx * ry * rz);
    for (let Z = 0; Z < rz; Z++) { for (let Y = 0; Y < ry; Y++) { for (let X = 0; X < rx; X++) {
        let s = 0;
        for (const z of [2 * Z, Math.min(2 * Z + 1, nz - 1)]) { for (const y of [2 * Y, Math.min(2 * Y + 1, ny - 1)]) {
            for (const x of [2 * X, Math.min(2 * X + 1, nx - 1)]) { s += v[(z * ny + y) * nx + x]; }
        } }
        out[(Z * ry + Y) * rx + X] = (s + 4) >> 3;
    } } }
    return out;
}
// one pass: W = sum of w(a) w(b) w(c) v(x + a, y + b, z + c), w = (1, 2, 1), indices clamped; out = (W + 32) >> 6
function smoothTexels(v, nx, ny, nz, passes, Ctor) {
    const w = [1, 2, 1];
    let cur = v;
    for (let p = 0; p < passes; p++) {
        const out = new Ctor(nx * ny * nz);
        for (let z = 0; z < nz; z++) { for (let y = 0; y < ny; y++) { for (let x = 0; x < nx; x++) {
            let W = 0;
            for (let c = -1; c <= 1; c++) { for (let b = -1; b <= 1; b++) { for (let a = -1; a <= 1; a++) {
                W += w[a + 1] * w[b + 1] * w[c + 1] * cur[(clamp(z + c, nz) * ny + clamp(y + b, ny)) * nx + clamp(x + a, nx)];
            } } }
            out[(z * ny + y) * nx + x] = (W + 32) >> 6;
        } } }
        cur = out;
    }
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
    let seed = 12345;
    const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
    for (const bits of [8, 16]) {
        const Ctor = bits === 8 ? Uint8Array : Uint16Array;
        const texels = new Ctor(NX * NY * NZ);
        for (let i = 0; i < texels.length; i++) { texels[i] = rand() & (bits === 8 ? 255 : 65535); }
        const bytes = new Uint8Array(texels.buffer);
        const v = new vpt.Volume(ctx, new vpt.RAWReader(bytes, { width: NX, height: NY, depth: NZ, bits: bits }));
        await v.load();
        const r = v.reduce(), s = v.smooth(2);
        if (!r.ready || r.nativeFormat() !== v.nativeFormat() || s.nativeFormat() !== v.nativeFormat()) { throw new Error('derived volumes change the format'); }
        const rd = r.modality.dimensions;
        if (rd.width !== 11 || rd.height !== 10 || rd.depth !== 12) { throw new Error('reduce: dimensions ' + JSON.stringify(rd)); }
        equal(r.readBlock(0, 0, 0, 11, 10, 12), reduceTexels(texels, NX, NY, NZ, Ctor), `reduce, ${bits} bits`);
        const want = smoothTexels(texels, NX, NY, NZ, 2, Ctor);
        const got = s.readBlock(0, 0, 0, NX, NY, NZ);
        equal(got, want, `smooth(2), ${bits} bits`);
        let changed = 0;
        for (let i = 0; i < got.length; i++) { if (got[i] !== texels[i]) { changed++; } }
        if (changed * 2 < got.length) { throw new Error('smooth(2) changes fewer than half of the texels'); }
        equal(v.readBlock(0, 0, 0, NX, NY, NZ), texels, 'the source afterwards');
        const top = v.reduce(10);                                 // stops once every axis is 1
        const td = top.modality.dimensions;
        if (td.width !== 1 || td.height !== 1 || td.depth !== 1) { throw new Error('reduce(10): dimensions ' + JSON.stringify(td)); }
        let level = texels, d = [NX, NY, NZ];
        while (Math.max(d[0], d[1], d[2]) > 1) { level = reduceTexels(level, d[0], d[1], d[2], Ctor); d = d.map(n => (n + 1) >> 1); }
        equal(top.readBlock(0, 0, 0, 1, 1, 1), level, `reduce(10), ${bits} bits`);
        for (const bad of [0, 9, 1.5, '1', null]) { throws(() => v.smooth(bad), 'smooth(' + JSON.stringify(bad) + ')'); }
        for (const bad of [0, -1, 1.5, '1', null]) { throws(() => v.reduce(bad), 'reduce(' + JSON.stringify(bad) + ')'); }
        const g = v.deriveGradient({ operator: 'central' });
        let named = '';
        try { g.smooth(1); } catch (e) { named = e.message; }     // a two-channel source: the library names the format
        if (!/RG(8|16)/.test(named)) { throw new Error('smooth of a two-channel volume: ' + named); }
        for (const vol of [g, top, r, s, v]) { vol.destroy(); }
    }
    ctx.destroy();
    // the context path
    for (const bad of [0, 9, 1.5, '1']) { throws(() => new vpt.RenderingContext({ smooth: bad }), 'RenderingContext({ smooth: ' + JSON.stringify(bad) + ' })'); }
    for (const bad of [-1, 1.5, '1']) { throws(() => new vpt.RenderingContext({ reduce: bad }), 'RenderingContext({ reduce: ' + JSON.stringify(bad) + ' })'); }
    const ct = new Int16Array(NX * NY * NZ);
    for (let i = 0; i < ct.length; i++) { ct[i] = (rand() % 4001) - 1000; }
    const rc = new vpt.RenderingContext({ resolution: { width: 72, height: 52 }, window: [-200, 400], windowFormat: 'r16', smooth: 2, reduce: 1,
        gradient: 'sobel', gradientGain: 2 });
    rc.gl.getExtension('EXT_texture_norm16');
    await rc.setVolume(new vpt.RAWReader(new Uint8Array(ct.buffer), { width: NX, height: NY, depth: NZ, bits: 16, signed: true }));
    if (rc.volume.nativeFormat() !== N.VPT_FORMAT_RG16 || rc.volume.modality.internalFormat !== GL.GL_RG16_EXT) { throw new Error('RenderingContext did not run the chain'); }
    const tex = rc.volume.readBlock(0, 0, 0, 11, 10, 12);
    rc.chooseRenderer('mip');
    rc.renderer.render();
    rc.destroy();
    fs.writeFileSync(outPath, Buffer.concat([Buffer.from(ct.buffer), Buffer.from(tex.buffer)]));
    console.log('js pyramid gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
