'use strict';
// node js/test/test_norm16_gpu.js VOLUME TF OUT W H NX NY NZ SIGNED — GPU: the Node.js host's 16-bit normalised volumes (EXT_texture_norm16).
// VOLUME holds nx * ny * nz little-endian uint16 (SIGNED = 0: R16_EXT / UNSIGNED_SHORT) or int16 (SIGNED = 1: R16_SNORM_EXT / SHORT) texels.
// Loading the manifest must raise the reference error until the context has called getExtension('EXT_texture_norm16'); then MIP, EAM and
// MCM frames (RGBA16F render buffers) go to OUT, and tests/test_js_gpu_norm16.py renders the same with the Python host and compares the bytes.
const assert = require('assert');
const fs = require('fs');
const vpt = require('../vpt/index.js');
const GL = require('../vpt/readers/readers.js');
const { native } = require('../vpt/native.js');

function goldenRng() { let k = 1; return () => { const v = (k * 0.61803398875) % 1; k++; return v; }; }

async function main() {
    const [volPath, tfPath, outPath, W, H, nx, ny, nz, signed] = process.argv.slice(2).map((a, i) => (i < 3 ? a : Number(a)));
    const N = native();
    const bytes = new Uint8Array(fs.readFileSync(volPath)), tf = new Uint8Array(fs.readFileSync(tfPath));
    const ctx = new vpt.Context(0);
    const cuts = [0, 7, 16, nz];                             // z slabs, the last ones mid-brick
    const plane = nx * ny * 2;
    const reader = {
        readMetadata: async () => ({
            meta: { version: 1 },
            modalities: [{ name: 'default', dimensions: { width: nx, height: ny, depth: nz }, format: GL.GL_RED,
                internalFormat: signed ? GL.GL_R16_SNORM_EXT : GL.GL_R16_EXT, type: signed ? GL.GL_SHORT : GL.GL_UNSIGNED_SHORT,
                transform: { matrix: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1] },
                placements: cuts.slice(0, -1).map((z, i) => ({ index: i, position: { x: 0, y: 0, z } })) }],
            blocks: cuts.slice(0, -1).map((z, i) => ({ url: String(i), format: 'raw', dimensions: { width: nx, height: ny, depth: cuts[i + 1] - z } })),
        }),
        readBlock: async i => bytes.subarray(cuts[i] * plane, cuts[i + 1] * plane),
    };
    let threw = false;
    try { await new vpt.Volume(ctx, reader).load(); } catch (e) { threw = /Unknown volume datatype/.test(e.message); }
    assert.ok(threw, '16-bit manifests raise the reference error without the extension');
    assert.strictEqual(ctx.getExtension('WEBGL_no_such_extension'), null);
    const ext = ctx.getExtension('EXT_texture_norm16');
    assert.ok(ext && ext.R16_EXT === 0x822A && ext.R16_SNORM_EXT === 0x8F98);
    assert.strictEqual(ctx.getExtension('EXT_texture_norm16'), ext);
    const other = new vpt.Context(0);                        // an enabled extension belongs to its context
    threw = false;
    try { await new vpt.Volume(other, reader).load(); } catch (e) { threw = /Unknown volume datatype/.test(e.message); }
    assert.ok(threw, 'another context has not enabled the extension');
    other.destroy();
    const v = new vpt.Volume(ctx, reader);
    await v.load();
    v.setFilter('linear');
    const out = [];
    for (const kind of ['mip', 'eam', 'mcm']) {
        const r = new (vpt.RendererFactory(kind))(ctx, v, vpt.defaultCamera(W / H), null,
            { resolution: { width: W, height: H }, transform: new vpt.Transform(new vpt.Node()), rng: goldenRng() });
        r.setTransferFunction({ data: tf, width: tf.length / 4, height: 1 });
        if (kind === 'mcm') { r.extinction = 40; }
        r.reset();
        for (let k = 0; k < 3; k++) { r.render(); }
        out.push(Buffer.from(r.read(N.VPT_BUFFER_RENDER, new Uint8Array(8 * W * H))));
        r.destroy();
    }
    fs.writeFileSync(outPath, Buffer.concat(out));
    v.destroy(); ctx.destroy();
    console.log('js norm16 gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
