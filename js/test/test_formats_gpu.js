'use strict';
// node js/test/test_formats_gpu.js — GPU: the Node.js host's volume formats beyond R8 / R32F.  An R8_SNORM manifest and a packed
// (RGB10_A2) manifest must render exactly like the R32F / RG32F manifest of their decoded texels.  Run by tests/test_js_gpu_formats.py.
const assert = require('assert');
const vpt = require('../vpt/index.js');
const GL = require('../vpt/readers/readers.js');
const { native } = require('../vpt/native.js');

function goldenRng() { let k = 1; return () => { const v = (k * 0.61803398875) % 1; k++; return v; }; }

async function main() {
    const N = native();
    const nx = 21, ny = 18, nz = 23, W = 72, H = 52, nv = nx * ny * nz;
    const ctx = new vpt.Context(0);
    const camera = vpt.defaultCamera(W / H);
    const transform = new vpt.Transform(new vpt.Node());
    // a manifest of one volume cut into z slabs (the last ones mid-brick) with the given (format, internalFormat, type)
    const mk = (bytes, format, internalFormat, type) => {
        const bpv = bytes.byteLength / nv, cuts = [0, 5, 14, nz];
        const rd = {
            readMetadata: async () => ({
                meta: { version: 1 },
                modalities: [{ name: 'default', dimensions: { width: nx, height: ny, depth: nz }, format, internalFormat, type,
                    transform: { matrix: [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1] },
                    placements: cuts.slice(0, -1).map((z, i) => ({ index: i, position: { x: 0, y: 0, z } })) }],
                blocks: cuts.slice(0, -1).map((z, i) => ({ url: String(i), format: 'raw', dimensions: { width: nx, height: ny, depth: cuts[i + 1] - z } })),
            }),
            readBlock: async i => new Uint8Array(bytes.buffer, cuts[i] * nx * ny * bpv, (cuts[i + 1] - cuts[i]) * nx * ny * bpv),
        };
        return new vpt.Volume(ctx, rd);
    };
    const render = async (v, kind) => {
        await v.load(); v.setFilter('linear');
        const r = new (vpt.RendererFactory(kind))(ctx, v, camera, null, { resolution: { width: W, height: H }, transform, rng: goldenRng() });
        r.reset(); r.render(); r.render();
        const out = Buffer.from(r.read(N.VPT_BUFFER_RENDER, new Uint8Array(8 * W * H)));
        r.destroy(); v.destroy();
        return out;
    };
    let seed = 12345;
    const rnd = () => { seed = (Math.imul(seed, 1103515245) + 12345) >>> 0; return seed; };

    // ---- R8_SNORM: every byte value, against the R32F volume of max(c / 127, -1) (float32 division, correctly rounded)
    {
        const s8 = new Int8Array(nv), f = new Float32Array(nv);
        for (let i = 0; i < nv; i++) {
            const c = i < 256 ? i - 128 : ((rnd() >>> 24) & 255) - 128;
            s8[i] = c; f[i] = Math.fround(Math.max(c, -127) / 127);
        }
        for (const kind of ['eam', 'mcm']) {
            const a = await render(mk(s8, GL.GL_RED, GL.GL_R8_SNORM, GL.GL_BYTE), kind);
            const b = await render(mk(f, GL.GL_RED, GL.GL_R32F, GL.GL_FLOAT), kind);
            assert.ok(a.equals(b), 'R8_SNORM renders like the R32F volume of its decoded texels (' + kind + ')');
        }
        let threw = false;
        try { await mk(s8, GL.GL_RED, 33322, GL.GL_BYTE).load(); } catch (e) { threw = /Unknown volume datatype/.test(e.message); }
        assert.ok(threw, 'BYTE with a non-SNORM internal format raises the reference error');
    }
    // ---- RGB10_A2 (UNSIGNED_INT_2_10_10_10_REV): r = bits 9-0 / 1023, g = bits 19-10 / 1023
    {
        const words = new Uint32Array(nv), rg = new Float32Array(2 * nv);
        for (let i = 0; i < nv; i++) {
            const w = rnd() >>> 0;
            words[i] = w; rg[2 * i] = Math.fround((w & 1023) / 1023); rg[2 * i + 1] = Math.fround(((w >>> 10) & 1023) / 1023);
        }
        const a = await render(mk(words, GL.GL_RGBA, GL.GL_RGB10_A2, GL.GL_UNSIGNED_INT_2_10_10_10_REV), 'mip');
        const b = await render(mk(rg, GL.GL_RG, 0x8230, GL.GL_FLOAT), 'mip');
        assert.ok(a.equals(b), 'RGB10_A2 renders like the RG32F volume of its decoded texels');
    }
    ctx.destroy();
    console.log('js formats gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
