'use strict';
// node js/test/test_thickness_gpu.js OUT — GPU: the Node.js host's local thickness.  Random blobs in 9 x 13 x 21 (no tile of 8 x 8 x 4 divides
// it), both seed modes, and a ball of radius 18 in 96 x 40 x 24 that leaves the volume through its faces, uint8 and uint16, through
// Distance.thickness, its within and channel, the timed and flagged forms, Volume.thickness and Volume.openBall: every value must equal the
// plain-JS statement of the contract (js/vpt/thickness.js).  Then RenderingContext({ thickness }) once: the source and the texels of what
// the context ends up with are written to OUT (tests/test_js_gpu_thickness.py compares them with the numpy chain).
const fs = require('fs');
const vpt = require('../vpt/index.js');
const { native } = require('../vpt/native.js');

function equal(a, b, what) {
    if (a.constructor !== b.constructor || a.length !== b.length) { throw new Error(what + ': wrong array'); }
    for (let i = 0; i < a.length; i++) { if (a[i] !== b[i]) { throw new Error(`${what}: element ${i} is ${a[i]}, expected ${b[i]}`); } }
}
function throws(f, what, pattern) {
    let message = null;
    try { f(); } catch (e) { message = e.message; }
    if (message === null) { throw new Error(what + ' was accepted'); }
    if (pattern && !pattern.test(message)) { throw new Error(what + ': unexpected message ' + message); }
}

let seed = 97531;
const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
// structure: codes of the upper half; the rest: codes of the lower half
function texelsOf(mask, bits) {
    const M = bits === 8 ? 255 : 65535, half = (M >> 1) + 1, out = new (bits === 8 ? Uint8Array : Uint16Array)(mask.length);
    for (let i = 0; i < mask.length; i++) { out[i] = mask[i] ? half + rand() % half : rand() % half; }
    return out;
}
function balls(nx, ny, nz, list) {
    const mask = new Uint8Array(nx * ny * nz);
    for (let z = 0, i = 0; z < nz; z++) { for (let y = 0; y < ny; y++) { for (let x = 0; x < nx; x++, i++) {
        for (const [cx, cy, cz, r] of list) { if ((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r) { mask[i] = 1; } }
    } } }
    return mask;
}

async function main() {
    const outPath = process.argv[2];
    const N = native();
    const ctx = new vpt.Context(0);
    if (!ctx.getExtension('EXT_texture_norm16')) { throw new Error('no EXT_texture_norm16'); }
    const uploadTo = async (texels, bits, dims) => {
        const v = new vpt.Volume(ctx, new vpt.RAWReader(new Uint8Array(texels.buffer), { width: dims[0], height: dims[1], depth: dims[2], bits: bits }));
        await v.load();
        return v;
    };
    const blobs = [];
    for (let b = 0; b < 6; b++) { blobs.push([rand() % 9, rand() % 13, rand() % 21, 1 + (rand() % 40) / 10]); }
    const CASES = [
        { dims: [9, 13, 21], mask: balls(9, 13, 21, blobs), modes: ['rest', 'range'] },
        { dims: [96, 40, 24], mask: balls(96, 40, 24, [[17, 17, 10, 18]]), modes: ['rest'] },      // (the complement's balls are too many to paint one by one)
    ];
    for (const { dims, mask, modes } of CASES) {
        const [nx, ny, nz] = dims, whole = [0, 0, 0, nx, ny, nz];
        for (const bits of [8, 16]) {
            const M = bits === 8 ? 255 : 65535, lo = (M >> 1) + 1, a = texelsOf(mask, bits);
            const v = await uploadTo(a, bits, dims);
            for (const seeds of modes) {
                const what = `${dims} ${bits} bits ${seeds}`;
                const d2 = vpt.distanceSquaredTexels(a, nx, ny, nz, lo, M, seeds), t2 = vpt.thicknessSquaredTexels(d2, nx, ny, nz);
                const d = v.distance(lo, M, seeds);
                const t = d.thickness();
                equal(t.squared(), t2, what);
                equal(d.squared(), d2, what + ': the source afterwards');
                if (JSON.stringify(t.info) !== JSON.stringify(d.info)) { throw new Error(what + ': info ' + JSON.stringify(t.info)); }
                if (JSON.stringify(t.profile()) !== JSON.stringify({ x: 0, y: 0, z: 0 })) { throw new Error(what + ': profile'); }
                let out = t.within(17, null, 5);
                equal(out.readBlock.apply(out, whole), vpt.withinTexels(a, t2, 17, null, 5), what + ': within'); out.destroy();
                out = t.channel(2);
                equal(out.readBlock.apply(out, whole), vpt.channelTexels(a, t2, 2), what + ': channel'); out.destroy();
                t.destroy();
                const timed = d.thicknessTimed();
                if (!(timed[1].ms.cover > 0) || !(timed[1].tiles > 0) || !(timed[1].visited >= 0)) { throw new Error(what + ': thicknessTimed ' + JSON.stringify(timed[1])); }
                equal(timed[0].squared(), t2, what + ': timed'); timed[0].destroy();
                for (const flags of [0, 1, 2, 3]) {
                    const capped = d.thicknessTimed(flags);
                    if (capped[1].tiles !== null || capped[1].visited < timed[1].visited) { throw new Error(what + ': flags ' + flags + ' ' + JSON.stringify(capped[1])); }
                    equal(capped[0].squared(), t2, what + ': flags ' + flags); capped[0].destroy();
                }
                throws(() => d.thicknessTimed(4), 'the library: flags 4', /flags 4/);
                d.destroy();
                throws(() => d.thickness(), 'thickness of destroyed distances', /destroyed/);
                out = v.thickness(lo, M, 3, seeds);
                equal(out.readBlock.apply(out, whole), vpt.thicknessTexels(a, nx, ny, nz, lo, M, 3, seeds), what + ': Volume.thickness'); out.destroy();
            }
            let out = v.thickness(lo, M);
            equal(out.readBlock.apply(out, whole), vpt.thicknessTexels(a, nx, ny, nz, lo, M), 'Volume.thickness by default'); out.destroy();
            for (const [radius, fill] of [[0, 0], [1.5, 7], [3, 0]]) {
                out = v.openBall(lo, M, radius, fill);
                equal(out.readBlock.apply(out, whole), vpt.openBallTexels(a, nx, ny, nz, lo, M, radius, fill), `${dims} openBall ${radius}`); out.destroy();
            }
            throws(() => v.openBall(lo, M, -1), 'a negative radius', /radius/);
            throws(() => v.thickness(lo, M, 0), 'steps 0', /steps/);
            throws(() => v.thickness(lo, M, 2, 'all'), "seeds 'all'", /seeds/);
            equal(v.readBlock.apply(v, whole), a, 'the source afterwards');
            v.destroy();
        }
    }
    ctx.destroy();
    // the context path
    throws(() => new vpt.RenderingContext({ thickness: { lo: 1, hi: 2, mode: 'channel' }, gradient: 'central' }), 'thickness with gradient', /second channel/);
    const NX = 28, NY = 16, NZ = 16, two = texelsOf(balls(NX, NY, NZ, [[9, 8, 8, 6], [19, 8, 8, 4]]), 8);
    const rc = new vpt.RenderingContext({ resolution: { width: 72, height: 52 }, thickness: { lo: 128, hi: 300, mode: 'channel' } });      // hi is open above
    await rc.setVolume(new vpt.RAWReader(two, { width: NX, height: NY, depth: NZ }));
    if (rc.volume.nativeFormat() !== N.VPT_FORMAT_RG8) { throw new Error('RenderingContext did not derive the thickness'); }
    const tex = rc.volume.readBlock(0, 0, 0, NX, NY, NZ);
    rc.chooseRenderer('mip');
    rc.renderer.render();
    rc.destroy();
    fs.writeFileSync(outPath, Buffer.concat([Buffer.from(two.buffer), Buffer.from(tex.buffer)]));
    console.log('js thickness gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
