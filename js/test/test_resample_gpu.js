'use strict';
// node js/test/test_resample_gpu.js OUT — GPU: the Node.js host's resampling.  A (23, 19, 21) volume of uniform noise, uint8 and uint16,
// through Volume.resample (a shrink, a growth and the identity in one call; NEAREST) and Volume.isotropic: the texels read back (readBlock)
// must equal the plain-JS twin of the contract (js/vpt/resample.js).  Then RenderingContext({ window, resample, rank, smooth, gradient })
// once over a signed 16-bit RAW volume: the texels of what the context ends up with are written to OUT (tests/test_js_gpu_resample.py
// compares them with the numpy chain).
const fs = require('fs');
const vpt = require('../vpt/index.js');
const GL = require('../vpt/readers/readers.js');
const { native } = require('../vpt/native.js');

const NX = 21, NY = 19, NZ = 23;
const SPACING = [0.7, 0.7, 1.6];

function equal(a, b, what) {
    if (a.constructor !== b.constructor || a.length !== b.length) { throw new Error(what + ': wrong array'); }
    for (let i = 0; i < a.length; i++) { if (a[i] !== b[i]) { throw new Error(`${what}: texel ${i} is ${a[i]}, expected ${b[i]}`); } }
}
function throws(f, what, pattern) {
    let message = null;
    try { f(); } catch (e) { message = e.message; }
    if (message === null) { throw new Error(what + ' was accepted'); }
    if (pattern && !pattern.test(message)) { throw new Error(what + ': unexpected message ' + message); }
}

async function main() {
    const outPath = process.argv[2];
    const N = native();
    const ctx = new vpt.Context(0);
    if (!ctx.getExtension('EXT_texture_norm16')) { throw new Error('no EXT_texture_norm16'); }
    let seed = 97531;
    const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
    for (const bits of [8, 16]) {
        const Ctor = bits === 8 ? Uint8Array : Uint16Array;
        const texels = new Ctor(NX * NY * NZ);
        for (let i = 0; i < texels.length; i++) { texels[i] = rand() & (bits === 8 ? 255 : 65535); }
        const v = new vpt.Volume(ctx, new vpt.RAWReader(new Uint8Array(texels.buffer), { width: NX, height: NY, depth: NZ, bits: bits }));
        await v.load();
        const target = [21, 40, 9];                               // width, height, depth: identity, growth, shrink
        const f = v.resample(target[0], target[1], target[2]), n = v.resample(target[0], target[1], target[2], 'nearest'), iso = v.isotropic(SPACING);
        const shape = vpt.isotropicShape([NX, NY, NZ], SPACING);
        if (shape[0] !== 21 || shape[1] !== 19 || shape[2] !== 53) { throw new Error('isotropicShape: ' + shape); }
        for (const [d, size] of [[f, target], [n, target], [iso, shape]]) {
            const m = d.modality.dimensions;
            if (!d.ready || d.nativeFormat() !== v.nativeFormat() || m.width !== size[0] || m.height !== size[1] || m.depth !== size[2]) { throw new Error('derived volume: wrong description'); }
        }
        const got = f.readBlock(0, 0, 0, target[0], target[1], target[2]);
        equal(got, vpt.resampleTexels(texels, [NX, NY, NZ], target, 'filtered'), `resample(${target}), ${bits} bits`);
        equal(n.readBlock(0, 0, 0, target[0], target[1], target[2]), vpt.resampleTexels(texels, [NX, NY, NZ], target, 'nearest'), `resample(${target}, 'nearest'), ${bits} bits`);
        equal(iso.readBlock(0, 0, 0, shape[0], shape[1], shape[2]), vpt.resampleTexels(texels, [NX, NY, NZ], shape, 'filtered'), `isotropic(${SPACING}), ${bits} bits`);
        equal(v.readBlock(0, 0, 0, NX, NY, NZ), texels, 'the source afterwards');
        const same = v.resample(NX, NY, NZ);
        equal(same.readBlock(0, 0, 0, NX, NY, NZ), texels, 'the identity');
        for (const bad of [0, 4097, 1.5, '4', null, true]) { throws(() => v.resample(bad, 4, 4), 'resample(' + JSON.stringify(bad) + ', 4, 4)', /along x/); }
        for (const bad of ['linear', 0, null, true]) { throws(() => v.resample(4, 4, 4, bad), "resample(4, 4, 4, " + JSON.stringify(bad) + ')', /resample mode/); }
        throws(() => v.isotropic([1, 1, 0]), 'isotropic([1, 1, 0])', /spacing along z/);
        throws(() => v.isotropic([1, 1, 1], 0.001), 'isotropic(pitch 0.001)', /along x/);
        for (const vol of [same, f, n, iso, v]) { vol.destroy(); }
    }
    // a float volume: NEAREST takes it, FILTERED names the format
    const floats = new Float32Array(8).map((_, i) => i / 8);
    const fv = new vpt.Volume(ctx, new vpt.RAWReader(new Uint8Array(floats.buffer), { width: 2, height: 2, depth: 2, bits: 32 }));
    await fv.load();
    if (fv.nativeFormat() !== N.VPT_FORMAT_R32F) { throw new Error('not a float volume'); }
    throws(() => fv.resample(3, 3, 3), 'filtered resampling of a float volume', /R32F/);
    const grown = fv.resample(4, 2, 2, 'nearest');
    equal(grown.readBlock(0, 0, 0, 4, 2, 2), vpt.resampleTexels(floats, [2, 2, 2], [4, 2, 2], 'nearest'), 'nearest float texels');
    grown.destroy(); fv.destroy();
    ctx.destroy();
    // the context path
    for (const bad of ['filtered', { size: [0, 1, 1] }, { spacing: [1, 1] }, { size: [2, 2, 2], mode: 'linear' }]) {
        throws(() => new vpt.RenderingContext({ resample: bad }), 'RenderingContext({ resample: ' + JSON.stringify(bad) + ' })');
    }
    const ct = new Int16Array(NX * NY * NZ);
    for (let i = 0; i < ct.length; i++) { ct[i] = (rand() % 4001) - 1000; }
    const rc = new vpt.RenderingContext({ resolution: { width: 72, height: 52 }, window: [-200, 400], windowFormat: 'r16', resample: { spacing: SPACING },
        rank: 'median', smooth: 1, gradient: 'sobel', gradientGain: 2 });
    rc.gl.getExtension('EXT_texture_norm16');
    await rc.setVolume(new vpt.RAWReader(new Uint8Array(ct.buffer), { width: NX, height: NY, depth: NZ, bits: 16, signed: true }));
    if (rc.volume.nativeFormat() !== N.VPT_FORMAT_RG16 || rc.volume.modality.internalFormat !== GL.GL_RG16_EXT) { throw new Error('RenderingContext did not run the chain'); }
    const tex = rc.volume.readBlock(0, 0, 0, 21, 19, 53);
    rc.chooseRenderer('mip');
    rc.renderer.render();
    rc.destroy();
    fs.writeFileSync(outPath, Buffer.concat([Buffer.from(ct.buffer), Buffer.from(tex.buffer)]));
    console.log('js resample gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
