'use strict';
// node js/test/test_envmap_gpu.js VOLUME TF HDR OUT W H NX NY NZ — GPU: the Node.js host's HDR environment maps.  VOLUME holds nx * ny * nz
// bytes (R8), TF an RGBA8 row, HDR a Radiance file read with readHDR and set as the environment of MCM and MCS renderers; their RGBA16F
// render buffers after three passes go to OUT, and tests/test_js_gpu_envmap.py renders the same with the Python host and compares the bytes.
// The addon refuses data shorter than the format's width * height texels, and the library an unknown format.
const assert = require('assert');
const fs = require('fs');
const vpt = require('../vpt/index.js');
const GL = require('../vpt/readers/readers.js');
const { native } = require('../vpt/native.js');

function goldenRng() { let k = 1; return () => { const v = (k * 0.61803398875) % 1; k++; return v; }; }

async function main() {
    const [volPath, tfPath, hdrPath, outPath, W, H, nx, ny, nz] = process.argv.slice(2).map((a, i) => (i < 4 ? a : Number(a)));
    const N = native();
    const bytes = new Uint8Array(fs.readFileSync(volPath)), tf = new Uint8Array(fs.readFileSync(tfPath));
    const env = vpt.readHDR(fs.readFileSync(hdrPath));
    assert.strictEqual(env.format, 'rgbe');
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
    v.setFilter('linear');
    const out = [];
    for (const kind of ['mcm', 'mcs']) {
        const r = new (vpt.RendererFactory(kind))(ctx, v, vpt.defaultCamera(W / H), env,
            { resolution: { width: W, height: H }, transform: new vpt.Transform(new vpt.Node()), rng: goldenRng() });
        r.setTransferFunction({ data: tf, width: tf.length / 4, height: 1 });
        r.extinction = kind === 'mcm' ? 40 : 9;
        r.reset();
        for (let k = 0; k < 3; k++) { r.render(); }
        out.push(Buffer.from(r.read(N.VPT_BUFFER_RENDER, new Uint8Array(8 * W * H))));
        if (kind === 'mcm') {
            const w = env.width, h = env.height;
            assert.throws(() => r.setEnvironmentMap({ data: env.data.subarray(0, 4 * w * h - 1), width: w, height: h, format: 'rgbe' }),
                e => e instanceof RangeError && /shorter than width\*height\*4/.test(e.message));
            assert.throws(() => r.setEnvironmentMap({ data: new Float32Array(4 * w * h - 1), width: w, height: h }),
                e => e instanceof RangeError && /shorter than width\*height\*16/.test(e.message));
            assert.throws(() => r.setEnvironmentMap({ data: new Uint16Array(4), width: 2, height: 1 }),
                e => e instanceof RangeError && /shorter than width\*height\*8/.test(e.message));
            assert.throws(() => N.rendererSetEnvironmentTexels(r._h, new Float32Array(4), 1, 1, 7), /unknown environment format 7/);
            assert.throws(() => r.setEnvironmentMap({ data: new Float32Array(4 * 16385), width: 1, height: 16385 }), /out of range/);
            assert.throws(() => r.setEnvironmentMap({ data: env.data, width: w, height: h, format: 'exr' }), TypeError);
        }
        r.destroy();
    }
    fs.writeFileSync(outPath, Buffer.concat(out));
    v.destroy(); ctx.destroy();
    console.log('js envmap gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
