'use strict';
// node js/test/test_distance_gpu.js OUT — GPU: the Node.js host's distance transform.  Uniform noise and a ball, uint8 and uint16, on a
// (23, 19, 21) volume through Volume.distance in both seed modes: the squared distances, the info and the texels of within() and channel(),
// and Volume.margin / Volume.core, must equal the plain-JS twins (js/vpt/distance.js).  Then RenderingContext({ window, distance: { mode:
// 'channel' } }) over a 16-bit RAW volume: the source texels and the texels the context ends up with are written to OUT
// (tests/test_js_gpu_distance.py compares them with the numpy chain).
const fs = require('fs');
const vpt = require('../vpt/index.js');
const GL = require('../vpt/readers/readers.js');
const { native } = require('../vpt/native.js');

function equal(a, b, what) {
    if (a.constructor !== b.constructor || a.length !== b.length) { throw new Error(what + ': wrong array'); }
    for (let i = 0; i < a.length; i++) { if (a[i] !== b[i]) { throw new Error(`${what}: element ${i} is ${a[i]}, expected ${b[i]}`); } }
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
    let seed = 13579;
    const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
    const NX = 23, NY = 19, NZ = 21, n = NX * NY * NZ;
    for (const bits of [8, 16]) {
        const Ctor = bits === 8 ? Uint8Array : Uint16Array, M = bits === 8 ? 255 : 65535;
        const texels = new Ctor(n);
        for (let i = 0; i < n; i++) {                                              // noise below M / 2, a ball of radius 6 at the code M
            const x = i % NX - 11, y = Math.floor(i / NX) % NY - 9, z = Math.floor(i / (NX * NY)) - 10;
            texels[i] = x * x + y * y + z * z <= 36 ? M : rand() & (M >> 1);
        }
        const v = new vpt.Volume(ctx, new vpt.RAWReader(new Uint8Array(texels.buffer), { width: NX, height: NY, depth: NZ, bits: bits }));
        await v.load();
        for (const [lo, hi, seeds] of [[0, M >> 6, 'range'], [M, M, 'range'], [M, M, 'rest'], [0, M >> 1, 'rest']]) {
            const what = `${bits} bits, [${lo}, ${hi}], ${seeds}`;
            const want = vpt.distanceSquaredTexels(texels, NX, NY, NZ, lo, hi, seeds);
            let largest = 0, count = 0;
            for (let i = 0; i < n; i++) { largest = Math.max(largest, want[i]); count += want[i] === 0 ? 1 : 0; }
            if (new Set(want).size < 8) { throw new Error(what + ': degenerate input'); }
            const d = v.distance(lo, hi, seeds);
            equal(d.squared(), want, what + ': squared');
            const info = d.info;
            if (info.seeds !== count || info.largest !== largest) { throw new Error(what + ': info ' + JSON.stringify(info)); }
            const all = d.within(), some = d.within(2, 9, 7), pair = d.channel(7);
            if (!all.ready || all.nativeFormat() !== v.nativeFormat() || pair.nativeFormat() !== (bits === 8 ? N.VPT_FORMAT_RG8 : N.VPT_FORMAT_RG16) ||
                pair.modality.internalFormat !== (bits === 8 ? GL.GL_RG8 : GL.GL_RG16_EXT)) { throw new Error(what + ': formats of the derived volumes'); }
            equal(all.readBlock(0, 0, 0, NX, NY, NZ), texels, what + ': within()');
            equal(some.readBlock(0, 0, 0, NX, NY, NZ), vpt.withinTexels(texels, want, 2, 9, 7), what + ': within(2, 9, 7)');
            equal(pair.readBlock(0, 0, 0, NX, NY, NZ), vpt.channelTexels(texels, want, 7), what + ': channel(7)');
            const p = d.profile();
            if (!(p.x >= 0 && p.y >= 0 && p.z >= 0)) { throw new Error(what + ': profile ' + JSON.stringify(p)); }
            throws(() => d.within(2, 1), 'within(2, 1)'); throws(() => d.within(0, 1, M + 1), 'within with a fill beyond the format');
            throws(() => d.channel(0), 'channel(0)'); throws(() => d.channel(257), 'channel(257)');
            for (const vol of [all, some, pair]) { vol.destroy(); }
            d.destroy();
            throws(() => d.squared(), 'squared distances of a destroyed handle');
        }
        const toBall = vpt.distanceSquaredTexels(texels, NX, NY, NZ, M, M, 'range'), inBall = vpt.distanceSquaredTexels(texels, NX, NY, NZ, M, M, 'rest');
        for (const radius of [0, 1.5, 3]) {
            const r2 = Math.floor(radius * radius), margin = v.margin(M, M, radius), core = v.core(M, M, radius);
            equal(margin.readBlock(0, 0, 0, NX, NY, NZ), vpt.withinTexels(texels, toBall, 0, r2, 0), `margin(${radius})`);
            equal(core.readBlock(0, 0, 0, NX, NY, NZ), vpt.withinTexels(texels, inBall, r2 + 1, null, 0), `core(${radius})`);
            margin.destroy(); core.destroy();
        }
        equal(v.readBlock(0, 0, 0, NX, NY, NZ), texels, 'the source afterwards');
        for (const bad of [[5, 4], [0, M + 1], [0, 1, 'both'], [0.5, 1]]) { throws(() => v.distance(...bad), 'distance(' + JSON.stringify(bad) + ')'); }
        throws(() => v.margin(0, 1, -1), 'margin with a negative radius'); throws(() => v.core(0, 1, NaN), 'core with NaN');
        const g = v.deriveGradient({ operator: 'central' });
        let named = '';
        try { g.distance(0, 1); } catch (err) { named = err.message; }          // a two-channel source: the library names the format
        if (!/RG(8|16)/.test(named)) { throw new Error('distance of a two-channel volume: ' + named); }
        g.destroy(); v.destroy();
    }
    ctx.destroy();
    // the context path: a signed 16-bit CT-like volume, windowed to R8, then (value, distance to the bright codes)
    const ct = new Int16Array(n);
    for (let i = 0; i < n; i++) { ct[i] = (rand() % 1400) - 600; }
    const rc = new vpt.RenderingContext({ resolution: { width: 72, height: 52 }, window: [-200, 400], distance: { lo: 250, hi: 254, mode: 'channel', steps: 64 } });
    rc.gl.getExtension('EXT_texture_norm16');
    await rc.setVolume(new vpt.RAWReader(new Uint8Array(ct.buffer), { width: NX, height: NY, depth: NZ, bits: 16, signed: true }));
    if (rc.volume.nativeFormat() !== N.VPT_FORMAT_RG8) { throw new Error('RenderingContext did not run the chain'); }
    const parts = [Buffer.from(ct.buffer), Buffer.from(rc.volume.readBlock(0, 0, 0, NX, NY, NZ).buffer)];
    rc.chooseRenderer('mip');
    rc.renderer.render();
    rc.destroy();
    fs.writeFileSync(outPath, Buffer.concat(parts));
    console.log('js distance gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
