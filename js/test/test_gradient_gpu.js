'use strict';
// node js/test/test_gradient_gpu.js VOLUME TF OUT W H NX NY NZ TFW TFH — GPU: the Node.js host's gradient-magnitude channel.  Loads the R8
// volume in VOLUME (raw bytes, nx * ny * nz), derives the (value, gradient magnitude) volume with the Sobel operator at gain 4, and writes to
// OUT: the derived volume's texels (readBlock: whole, and a box that starts and ends mid-brick), its 256 x 256 histogram, and the RGBA16F
// render buffers of MIP and MCM under the RGBA8 transfer function in TF (tfw x tfh); then the same two frames through a RenderingContext
// with { gradient: 'sobel', gradientGain: 4 }.  tests/test_js_gpu_gradient.py does the same with the Python host and compares the bytes.
const fs = require('fs');
const vpt = require('../vpt/index.js');
const GL = require('../vpt/readers/readers.js');
const { native } = require('../vpt/native.js');

function goldenRng() { let k = 1; return () => { const v = (k * 0.61803398875) % 1; k++; return v; }; }

async function main() {
    const [volPath, tfPath, outPath, W, H, nx, ny, nz, tfw, tfh] = process.argv.slice(2).map((a, i) => (i < 3 ? a : Number(a)));
    const N = native();
    const bytes = new Uint8Array(fs.readFileSync(volPath)), tf = new Uint8Array(fs.readFileSync(tfPath));
    const reader = () => ({
        readMetadata: async () => ({
            meta: { version: 1 },
            modalities: [{ name: 'default', dimensions: { width: nx, height: ny, depth: nz }, format: GL.GL_RED, internalFormat: GL.GL_R8,
                type: GL.GL_UNSIGNED_BYTE, transform: { matrix: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1] },
                placements: [{ index: 0, position: { x: 0, y: 0, z: 0 } }] }],
            blocks: [{ url: '0', format: 'raw', dimensions: { width: nx, height: ny, depth: nz } }],
        }),
        readBlock: async () => bytes,
    });
    const ctx = new vpt.Context(0);
    const v = new vpt.Volume(ctx, reader());
    await v.load();
    const g = v.deriveGradient({ operator: 'sobel', gain: 4 });
    v.destroy();                                              // the derived volume stands alone
    if (!g.ready || g.nativeFormat() !== N.VPT_FORMAT_RG8 || g.modality.internalFormat !== GL.GL_RG8) { throw new Error('derived volume is not RG8'); }
    const out = [];
    const whole = g.readBlock(0, 0, 0, nx, ny, nz);
    if (!(whole instanceof Uint8Array) || whole.length !== 2 * nx * ny * nz) { throw new Error('readBlock: wrong array'); }
    out.push(Buffer.from(whole.buffer));
    out.push(Buffer.from(g.readBlock(1, 2, 3, 13, 9, 11).buffer));
    const hist = g.histogram();
    if (!(hist instanceof Uint32Array) || hist.length !== 65536) { throw new Error('histogram: wrong array'); }
    out.push(Buffer.from(hist.buffer));
    for (const bad of [{ operator: 'prewitt' }, { gain: 0 }, { gain: 17 }, { gain: NaN }]) {
        let threw = false;
        try { g.deriveGradient(bad); } catch (e) { threw = true; }
        if (!threw) { throw new Error('deriveGradient accepted ' + JSON.stringify(bad)); }
    }
    let named = '';
    try { g.deriveGradient({}); } catch (e) { named = e.message; }                 // a two-channel source: the library names the format
    if (!/RG8/.test(named)) { throw new Error('deriveGradient of an RG8 volume: ' + named); }
    for (const kind of ['mip', 'mcm']) {
        const r = new (vpt.RendererFactory(kind))(ctx, g, vpt.defaultCamera(W / H), null,
            { resolution: { width: W, height: H }, transform: new vpt.Transform(new vpt.Node()), rng: goldenRng() });
        r.reset();                                            // (as chooseRenderer does below: a reset draws from the rng)
        r.setTransferFunction({ data: tf, width: tfw, height: tfh });
        if (kind === 'mcm') { r.extinction = 40; }
        r.reset();
        for (let k = 0; k < 3; k++) { r.render(); }
        out.push(Buffer.from(r.read(N.VPT_BUFFER_RENDER, new Uint8Array(8 * W * H))));
        r.destroy();
    }
    g.destroy(); ctx.destroy();
    // the context path
    for (const kind of ['mip', 'mcm']) {
        const rc = new vpt.RenderingContext({ resolution: { width: W, height: H }, rng: goldenRng(), gradient: 'sobel', gradientGain: 4 });
        await rc.setVolume(reader());
        if (rc.volume.nativeFormat() !== N.VPT_FORMAT_RG8) { throw new Error('RenderingContext did not derive the channel'); }
        rc.chooseRenderer(kind);
        rc.renderer.setTransferFunction({ data: tf, width: tfw, height: tfh });
        if (kind === 'mcm') { rc.renderer.extinction = 40; }
        rc.renderer.reset();
        for (let k = 0; k < 3; k++) { rc.renderer.render(); }
        out.push(Buffer.from(rc.renderer.read(N.VPT_BUFFER_RENDER, new Uint8Array(8 * W * H))));
        rc.destroy();
    }
    fs.writeFileSync(outPath, Buffer.concat(out));
    console.log('js gradient gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
