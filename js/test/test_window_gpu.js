'use strict';
// node js/test/test_window_gpu.js VOLUME TF OUT W H NX NY NZ TFW TFH — GPU: the Node.js host's value-range window.  Loads the signed 16-bit
// volume in VOLUME (little-endian int16, nx * ny * nz samples) through RAWReader({ bits: 16, signed: true }) and writes to OUT: its range and
// its 2 / 98 percentile window (four float64), its 65536-bin code histogram, the texels of the volume windowed to [-200, 400] as R8 and as
// R16 (readBlock), and the RGBA16F render buffers of MIP and MCM over the R8 volume under the RGBA8 transfer function in TF (tfw x tfh);
// then the same two frames through a RenderingContext with { window: [-200, 400] }.  tests/test_js_gpu_window.py does the same with the
// Python host and compares the bytes.
const fs = require('fs');
const vpt = require('../vpt/index.js');
const GL = require('../vpt/readers/readers.js');
const { native } = require('../vpt/native.js');

function goldenRng() { let k = 1; return () => { const v = (k * 0.61803398875) % 1; k++; return v; }; }

async function main() {
    const [volPath, tfPath, outPath, W, H, nx, ny, nz, tfw, tfh] = process.argv.slice(2).map((a, i) => (i < 3 ? a : Number(a)));
    const N = native();
    const bytes = new Uint8Array(fs.readFileSync(volPath)), tf = new Uint8Array(fs.readFileSync(tfPath));
    const reader = () => new vpt.RAWReader(bytes, { width: nx, height: ny, depth: nz, bits: 16, signed: true });
    const ctx = new vpt.Context(0);
    if (!ctx.getExtension('EXT_texture_norm16')) { throw new Error('no EXT_texture_norm16'); }
    const v = new vpt.Volume(ctx, reader());
    await v.load();
    if (v.nativeFormat() !== N.VPT_FORMAT_R16_SNORM) { throw new Error('RAWReader({ bits: 16, signed }) did not give an R16_SNORM volume'); }
    const out = [];
    const range = v.range(), pw = v.percentileWindow(2, 98);
    out.push(Buffer.from(new Float64Array([range[0], range[1], pw[0], pw[1]]).buffer));
    const hist = v.codeHistogram();
    if (!(hist instanceof Uint32Array) || hist.length !== 65536) { throw new Error('codeHistogram: wrong array'); }
    out.push(Buffer.from(hist.buffer));
    const w8 = v.window({ lo: -200, hi: 400 }), w16 = v.window({ lo: -200, hi: 400, format: 'r16' });
    v.destroy();                                              // the windowed volumes stand alone
    if (!w8.ready || w8.nativeFormat() !== N.VPT_FORMAT_R8 || w8.modality.internalFormat !== GL.GL_R8) { throw new Error('windowed volume is not R8'); }
    if (w16.nativeFormat() !== N.VPT_FORMAT_R16 || w16.modality.internalFormat !== GL.GL_R16_EXT) { throw new Error('windowed volume is not R16'); }
    const t8 = w8.readBlock(0, 0, 0, nx, ny, nz), t16 = w16.readBlock(0, 0, 0, nx, ny, nz);
    if (!(t8 instanceof Uint8Array) || !(t16 instanceof Uint16Array)) { throw new Error('readBlock: wrong array'); }
    out.push(Buffer.from(t8.buffer)); out.push(Buffer.from(t16.buffer));
    const id = w8.window({ lo: 0, hi: 255 }).readBlock(0, 0, 0, nx, ny, nz);          // R8 -> R8 over [0, 255] is the identity
    for (let i = 0; i < id.length; i++) { if (id[i] !== t8[i]) { throw new Error('the identity window changed texel ' + i); } }
    for (const bad of [{ lo: 5, hi: 5 }, { lo: 0.5, hi: 3 }, { lo: 0, hi: 1, format: 'r32f' }, { lo: NaN, hi: 1 }]) {
        let threw = false;
        try { w8.window(bad); } catch (e) { threw = true; }
        if (!threw) { throw new Error('window accepted ' + JSON.stringify(bad)); }
    }
    w16.destroy();
    for (const kind of ['mip', 'mcm']) {
        const r = new (vpt.RendererFactory(kind))(ctx, w8, vpt.defaultCamera(W / H), null,
            { resolution: { width: W, height: H }, transform: new vpt.Transform(new vpt.Node()), rng: goldenRng() });
        r.reset();                                            // (as chooseRenderer does below: a reset draws from the rng)
        r.setTransferFunction({ data: tf, width: tfw, height: tfh });
        if (kind === 'mcm') { r.extinction = 40; }
        r.reset();
        for (let k = 0; k < 3; k++) { r.render(); }
        out.push(Buffer.from(r.read(N.VPT_BUFFER_RENDER, new Uint8Array(8 * W * H))));
        r.destroy();
    }
    const g = w8.deriveGradient({ operator: 'sobel', gain: 2 });
    let named = '';
    try { g.window({ lo: 0, hi: 1 }); } catch (e) { named = e.message; }            // a two-channel source: the library names the format
    if (!/RG8/.test(named)) { throw new Error('window of an RG8 volume: ' + named); }
    g.destroy(); w8.destroy(); ctx.destroy();
    // the context path
    for (const bad of ['auto', [1], { percentiles: [60, 40] }]) {
        let threw = false;
        try { new vpt.RenderingContext({ window: bad }); } catch (e) { threw = true; }
        if (!threw) { throw new Error('RenderingContext accepted window ' + JSON.stringify(bad)); }
    }
    for (const kind of ['mip', 'mcm']) {
        const rc = new vpt.RenderingContext({ resolution: { width: W, height: H }, rng: goldenRng(), window: [-200, 400] });
        rc.gl.getExtension('EXT_texture_norm16');
        await rc.setVolume(reader());
        if (rc.volume.nativeFormat() !== N.VPT_FORMAT_R8) { throw new Error('RenderingContext did not window the volume'); }
        rc.chooseRenderer(kind);
        rc.renderer.setTransferFunction({ data: tf, width: tfw, height: tfh });
        if (kind === 'mcm') { rc.renderer.extinction = 40; }
        rc.renderer.reset();
        for (let k = 0; k < 3; k++) { rc.renderer.render(); }
        out.push(Buffer.from(rc.renderer.read(N.VPT_BUFFER_RENDER, new Uint8Array(8 * W * H))));
        rc.destroy();
    }
    // 'range' and percentiles with the gradient behind them: the texels of what the context ends up with
    for (const window of ['range', { percentiles: [2, 98] }]) {
        const rc = new vpt.RenderingContext({ resolution: { width: W, height: H }, window: window, windowFormat: 'r16', gradient: 'central' });
        rc.gl.getExtension('EXT_texture_norm16');
        await rc.setVolume(reader());
        if (rc.volume.nativeFormat() !== N.VPT_FORMAT_RG16) { throw new Error('RenderingContext did not window and derive'); }
        out.push(Buffer.from(rc.volume.readBlock(0, 0, 0, nx, ny, nz).buffer));
        rc.destroy();
    }
    fs.writeFileSync(outPath, Buffer.concat(out));
    console.log('js window gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
