'use strict';
// node js/test/test_reconstruct_gpu.js OUT — GPU: the Node.js host's reconstruction and geodesic operations.  Three shapes (one voxel more
// than a 64 x 8 x 4 tile on every axis; three tiles on every axis; odd everywhere), uint8 and uint16, through Volume.reconstruct (both ops,
// a two-channel marker), Volume.geodesic (all seven) and the timed and capped forms: the texels read back (readBlock) must equal the plain-JS
// twin of the contract (js/vpt/reconstruct.js).  Then RenderingContext({ rank, geodesic, smooth }) once: the source and the texels of what the
// context ends up with are written to OUT (tests/test_js_gpu_reconstruct.py compares them with the numpy chain).
const fs = require('fs');
const vpt = require('../vpt/index.js');
const { native } = require('../vpt/native.js');

const SHAPES = [[65, 9, 5], [130, 17, 9], [7, 5, 3]];
const NX = 37, NY = 22, NZ = 13;

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
    for (const dims of SHAPES) {
        const [nx, ny, nz] = dims, n = nx * ny * nz, whole = [0, 0, 0, nx, ny, nz];
        const upload = async (texels, bits) => {
            const v = new vpt.Volume(ctx, new vpt.RAWReader(new Uint8Array(texels.buffer), { width: nx, height: ny, depth: nz, bits: bits }));
            await v.load();
            return v;
        };
        for (const bits of [8, 16]) {
            const Ctor = bits === 8 ? Uint8Array : Uint16Array, M = bits === 8 ? 255 : 65535, codes = [0, M >> 2, M >> 1, M - (M >> 2), M];
            const a = new Ctor(n), b = new Ctor(n);
            for (let i = 0; i < n; i++) { a[i] = rand() & M; b[i] = codes[rand() % codes.length]; }      // noise; five codes, so that plateaus occur
            const va = await upload(a, bits), vb = await upload(b, bits);
            const pair = vb.pair(va), two = pair.readBlock.apply(pair, whole);                            // (b, a), made on the device
            for (const connectivity of [6, 18, 26]) {
                for (const op of ['dilation', 'erosion']) {
                    const what = `${op} under ${connectivity}, ${bits} bits, ${dims}`;
                    const d = va.reconstruct(vb, { op, connectivity });
                    if (!d.ready || d.nativeFormat() !== va.nativeFormat() || d.modality.dimensions.width !== nx) { throw new Error(what + ': wrong description'); }
                    equal(d.readBlock.apply(d, whole), vpt.reconstructTexels(a, b, dims, { op, connectivity }), what);
                    const c1 = pair.reconstruct(vb, { op, connectivity, channel: 1 });                  // the marker is channel 1 of a two-channel volume
                    if (c1.nativeFormat() !== va.nativeFormat()) { throw new Error(what + ': the result has one channel'); }
                    equal(c1.readBlock.apply(c1, whole), vpt.reconstructTexels(two, b, dims, { op, connectivity, channels: 2, channel: 1 }), what + ', channel 1');
                    d.destroy(); c1.destroy();
                }
                for (const op of vpt.GEODESIC_OPS) {
                    const h = op === 'hmax' || op === 'hmin' || op === 'dome' ? 41 * ((M / 255) | 0) : 0, what = `${op} ${h} under ${connectivity}, ${bits} bits, ${dims}`;
                    const d = vb.geodesic(op, h, connectivity);
                    equal(d.readBlock.apply(d, whole), vpt.geodesicTexels(b, dims, op, { h, connectivity }), what);
                    d.destroy();
                }
            }
            const g1 = pair.hmax(41 * ((M / 255) | 0), 26, 1);
            equal(g1.readBlock.apply(g1, whole), vpt.geodesicTexels(two, dims, 'hmax', { h: 41 * ((M / 255) | 0), connectivity: 26, channels: 2, channel: 1 }), 'hmax of channel 1');
            g1.destroy();
            const timed = va.reconstructTimed(vb, { connectivity: 18 });
            equal(timed[0].readBlock.apply(timed[0], whole), vpt.reconstructTexels(a, b, dims, { connectivity: 18 }), 'reconstructTimed');
            if (!(timed[1].ms > 0) || !(timed[1].launches >= 1) || !(timed[1].tileRuns >= 1)) { throw new Error('reconstructTimed: ' + JSON.stringify(timed[1])); }
            const capped = va.reconstructTimed(vb, { connectivity: 18, tileRounds: 1 });
            equal(capped[0].readBlock.apply(capped[0], whole), vpt.reconstructTexels(a, b, dims, { connectivity: 18 }), 'one round a launch');
            if (!(capped[1].launches >= timed[1].launches)) { throw new Error('one round a launch: fewer launches'); }
            const filled = vb.fillHolesTimed(6);
            equal(filled[0].readBlock.apply(filled[0], whole), vpt.geodesicTexels(b, dims, 'fill_holes'), 'fillHolesTimed');
            if (!(filled[1].launches >= 1)) { throw new Error('fillHolesTimed: ' + JSON.stringify(filled[1])); }
            timed[0].destroy(); capped[0].destroy(); filled[0].destroy();
            equal(va.readBlock.apply(va, whole), a, 'the marker afterwards'); equal(vb.readBlock.apply(vb, whole), b, 'the mask afterwards');
            throws(() => va.reconstruct(vb, { op: 'opening' }), "op 'opening'", /reconstruct op is/);
            throws(() => va.reconstruct(vb, { connectivity: 8 }), 'connectivity 8', /connectivity/);
            throws(() => va.reconstruct(vb, { channel: 1 }), 'channel 1 of a one-channel volume', /channel 1/);
            throws(() => va.reconstruct(vb, { passes: 2 }), 'an unknown option', /passes/);
            throws(() => va.reconstruct({}), 'no volume', /two ready volumes/);
            throws(() => va.reconstructTimed(vb, { tileRounds: 0 }), 'tileRounds 0', /tileRounds/);
            throws(() => va.geodesic('watershed'), "op 'watershed'", /geodesic op is/);
            throws(() => va.hmax(M + 1), 'h above M', /geodesic h/);
            throws(() => va.regionalMaxima(5), 'connectivity 5', /connectivity/);
            throws(() => N.volumeGeodesic(va.texture, 0, 5, 1, 6), 'the library: MAXIMA with h', /MAXIMA/);
            for (const vol of [pair, va, vb]) { vol.destroy(); }
        }
    }
    ctx.destroy();
    // the context path
    for (const bad of ['hmax', {}, { op: 'watershed' }, { op: 'maxima', h: 1 }, { op: 'hmax', connectivity: 4 }]) {
        throws(() => new vpt.RenderingContext({ geodesic: bad }), 'RenderingContext({ geodesic: ' + JSON.stringify(bad) + ' })');
    }
    const n = NX * NY * NZ, v = new Uint8Array(n);
    for (let i = 0; i < n; i++) { v[i] = rand() & 255; }
    const rc = new vpt.RenderingContext({ resolution: { width: 72, height: 52 }, rank: 'median', geodesic: { op: 'hmax', h: 40, connectivity: 18 }, smooth: 1 });
    await rc.setVolume(new vpt.RAWReader(v, { width: NX, height: NY, depth: NZ }));
    if (rc.volume.nativeFormat() !== N.VPT_FORMAT_R8) { throw new Error('RenderingContext did not run the chain'); }
    const tex = rc.volume.readBlock(0, 0, 0, NX, NY, NZ);
    rc.chooseRenderer('mip');
    rc.renderer.render();
    rc.destroy();
    fs.writeFileSync(outPath, Buffer.concat([Buffer.from(v.buffer), Buffer.from(tex.buffer)]));
    console.log('js reconstruct gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
