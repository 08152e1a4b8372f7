'use strict';
// node js/test/test_quasicubic_gpu.js VOLUME TF OUT W H NX NY NZ — GPU: the Node.js host's quasi-cubic filter.  Renders the R8 volume in
// VOLUME (raw bytes, nx * ny * nz) with the RGBA8 transfer function in TF (w x 1) through MIP and MCM, setFilter('quasicubic'), and writes
// both RGBA16F render buffers to OUT; tests/test_js_gpu_quasicubic.py renders the same with the Python host and compares the bytes.
const fs = require('fs');
const vpt = require('../vpt/index.js');
const GL = require('../vpt/readers/readers.js');
const { native } = require('../vpt/native.js');

function goldenRng() { let k = 1; return () => { const v = (k * 0.61803398875) % 1; k++; return v; }; }

async function main() {
    const [volPath, tfPath, outPath, W, H, nx, ny, nz] = process.argv.slice(2).map((a, i) => (i < 3 ? a : Number(a)));
    const N = native();
    const bytes = new Uint8Array(fs.readFileSync(volPath)), tf = new Uint8Array(fs.readFileSync(tfPath));
    const ctx = new vpt.Context(0);
    const reader = {
        readMetadata: async () => ({
            meta: { version: 1 },
            modalities: [{ name: 'default', dimensions: { width: nx, height: ny, depth: nz }, format: GL.GL_RED, internalFormat: GL.GL_R8,
                type: GL.GL_UNSIGNED_BYTE, transform: { matrix: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1] },
                placements: [{ index: 0, position: { x: 0, y: 0, z: 0 } }] }],
            blocks: [{ url: '0', format: 'raw', dimensions: { width: nx, height: ny, depth: nz } }],
        }),
        readBlock: async () => bytes,
    };
    const v = new vpt.Volume(ctx, reader);
    await v.load();
    v.setFilter('quasicubic');
    const out = [];
    for (const kind of ['mip', 'mcm']) {
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
    console.log('js quasicubic gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
