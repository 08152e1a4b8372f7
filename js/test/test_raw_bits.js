'use strict';
// node js/test/test_raw_bits.js — CPU: RAWReader's `bits` (8, 16, 32) and `signed` options in the Node host: the manifest triple, the
// byte range of every slice, and that `bits: 8` and no `bits` give the metadata and blocks the reader always gave.  Run by
// tests/test_window_host.py.
const assert = require('assert');
const vpt = require('../vpt/index.js');
const GL = require('../vpt/readers/readers.js');

async function main() {
    const w = 5, h = 4, d = 3;
    const data = new Uint8Array(512);
    for (let i = 0; i < data.length; i++) { data[i] = i & 255; }
    const plain = new vpt.RAWReader(data, { width: w, height: h, depth: d });
    const plainMeta = await plain.readMetadata();
    assert.deepStrictEqual([plainMeta.modalities[0].format, plainMeta.modalities[0].internalFormat, plainMeta.modalities[0].type],
        [GL.GL_RED, GL.GL_R8, GL.GL_UNSIGNED_BYTE]);
    const cases = [
        [8, false, [GL.GL_RED, GL.GL_R8, GL.GL_UNSIGNED_BYTE], 1], [16, false, [GL.GL_RED, GL.GL_R16_EXT, GL.GL_UNSIGNED_SHORT], 2],
        [16, true, [GL.GL_RED, GL.GL_R16_SNORM_EXT, GL.GL_SHORT], 2], [32, false, [GL.GL_RED, GL.GL_R32F, GL.GL_FLOAT], 4],
    ];
    for (const [bits, signed, triple, size] of cases) {
        const r = new vpt.RAWReader(data, { width: w, height: h, depth: d, bits: bits, signed: signed });
        const md = await r.readMetadata();
        const m = md.modalities[0];
        assert.deepStrictEqual([m.format, m.internalFormat, m.type], triple);
        assert.deepStrictEqual(m.dimensions, { width: w, height: h, depth: d });
        assert.strictEqual(md.blocks.length, d); assert.strictEqual(m.placements.length, d);
        for (let i = 0; i < d; i++) {
            assert.deepStrictEqual(md.blocks[i].dimensions, { width: w, height: h, depth: 1 });
            const got = new Uint8Array(await r.readBlock(i));
            assert.deepStrictEqual(Array.from(got), Array.from(data.subarray(i * w * h * size, (i + 1) * w * h * size)));
        }
        if (bits === 8) {
            assert.deepStrictEqual(md, plainMeta);
            for (let i = 0; i < d; i++) {
                assert.deepStrictEqual(Array.from(new Uint8Array(await r.readBlock(i))), Array.from(new Uint8Array(await plain.readBlock(i))));
            }
        }
    }
    for (const bad of [{ bits: 12 }, { bits: 64 }, { bits: '16' }, { bits: 8, signed: true }, { bits: 32, signed: true }]) {
        assert.throws(() => new vpt.RAWReader(data, Object.assign({ width: w, height: h, depth: d }, bad)), /RAWReader/);
    }
    console.log('js raw bits ok');
}
main().catch(e => { console.error(e); process.exit(1); });
