'use strict';
// node js/test/test_skeleton_gpu.js OUT — GPU: the Node.js host's thinning.  Noise of density 0.6 and a few overlapping balls in 70 x 19 x 11
// (two whole tiles of 64 x 8 x 4 and a partial one along every axis, across the 32-voxel word boundary), a row of 33, one voxel and the
// empty range, uint8 and uint16, the three modes, through Volume.skeleton, its info, burn, within, volume and profile, the pass cap, the
// form without the tile cull and Volume.centreline: every value must equal the plain-JS statement of the contract (js/vpt/skeleton.js).
// Then RenderingContext({ skeleton }) once: the source and the texels of what the context ends up with are written to OUT
// (tests/test_js_gpu_skeleton.py compares them with the numpy statement).
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
function sameInfo(got, want, what) {
    if (JSON.stringify(got) !== JSON.stringify(want)) { throw new Error(`${what}: info ${JSON.stringify(got)}, expected ${JSON.stringify(want)}`); }
}

let seed = 24680;
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
function noise(n, tenths) {
    const mask = new Uint8Array(n);
    for (let i = 0; i < n; i++) { mask[i] = rand() % 10 < tenths ? 1 : 0; }
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
    const CASES = [
        { dims: [70, 19, 11], mask: noise(70 * 19 * 11, 6) },
        { dims: [70, 19, 11], mask: balls(70, 19, 11, [[8, 9, 5, 6], [20, 9, 5, 8], [36, 6, 4, 5], [50, 12, 6, 7], [64, 9, 5, 5]]) },
        { dims: [33, 1, 1], mask: new Uint8Array(33).fill(1) },
        { dims: [1, 1, 1], mask: new Uint8Array(1).fill(1) },
    ];
    for (const { dims, mask } of CASES) {
        const [nx, ny, nz] = dims, whole = [0, 0, 0, nx, ny, nz];
        for (const bits of [8, 16]) {
            const M = bits === 8 ? 255 : 65535, lo = (M >> 1) + 1, hi = M - (M >> 4), a = texelsOf(mask, bits);      // the range leaves the top codes out
            const v = await uploadTo(a, bits, dims);
            for (const mode of ['kernel', 'ends', 'isthmus']) {
                const what = `${dims} ${bits} bits ${mode}`;
                const want = vpt.skeletonBurnTexels(a, nx, ny, nz, lo, hi, mode);
                const k = v.skeleton(lo, hi, mode);
                equal(k.burn(), want.burn, what);
                sameInfo(k.info, want.info, what);
                const profile = k.profile();
                if (profile.launches !== 2 + 9 * want.info.passes || !(profile.tiles > 0) || !(profile.ms.steps >= 0)) { throw new Error(what + ': profile ' + JSON.stringify(profile)); }
                let out = k.within(2, null, 5);
                equal(out.readBlock.apply(out, whole), vpt.burnWithinTexels(a, want.burn, 2, null, 5), what + ': within'); out.destroy();
                out = k.volume();
                equal(out.readBlock.apply(out, whole), vpt.skeletonTexels(a, nx, ny, nz, lo, hi, mode), what + ': volume'); out.destroy();
                throws(() => k.within(5, 4), 'from above to', /burn passes/);
                throws(() => k.within(1, null, M + 1), 'fill above M', /fill/);
                k.close();
                throws(() => k.burn(), 'burn of a destroyed skeleton', /destroyed/);
                const every = v.skeleton(lo, hi, mode, 0, 1);
                equal(every.burn(), want.burn, what + ': without the cull');
                if (every.profile().tiles < profile.tiles) { throw new Error(what + ': the cull adds tile visits'); }
                every.destroy();
                throws(() => v.skeleton(lo, hi, mode, 0, 2), 'the library: flags 2', /flags 2/);
                for (const passes of [1, 2, want.info.passes + 1]) {
                    const capped = vpt.skeletonBurnTexels(a, nx, ny, nz, lo, hi, mode, passes), kc = v.skeleton(lo, hi, mode, passes);
                    equal(kc.burn(), capped.burn, `${what}: capped at ${passes}`);
                    sameInfo(kc.info, capped.info, `${what}: capped at ${passes}`);
                    kc.destroy();
                }
            }
            const none = v.skeleton(0, 0, 'ends');                                  // no voxel has code 0 ... unless the draw says so
            sameInfo(none.info, vpt.skeletonBurnTexels(a, nx, ny, nz, 0, 0, 'ends').info, `${dims} ${bits} bits: the range [0, 0]`);
            none.destroy();
            let out = v.centreline(lo, hi);
            equal(out.readBlock.apply(out, whole), vpt.skeletonTexels(a, nx, ny, nz, lo, hi), `${dims} centreline by default`); out.destroy();
            throws(() => v.skeleton(hi, lo), 'lo above hi', /skeleton range/);
            throws(() => v.skeleton(lo, M + 1), 'hi above M', /skeleton range/);
            throws(() => v.skeleton(lo, hi, 'curve'), "mode 'curve'", /mode/);
            throws(() => v.skeleton(lo, hi, 'ends', -1), 'passes -1', /passes/);
            equal(v.readBlock.apply(v, whole), a, 'the source afterwards');
            v.destroy();
        }
    }
    ctx.destroy();
    // the context path
    throws(() => new vpt.RenderingContext({ skeleton: { lo: 1, hi: 2 }, thickness: { lo: 1, hi: 2, mode: 'within' } }), 'skeleton with thickness within', /name one of them/);
    const NX = 28, NY = 16, NZ = 16, two = texelsOf(balls(NX, NY, NZ, [[9, 8, 8, 6], [19, 8, 8, 4]]), 8);
    const rc = new vpt.RenderingContext({ resolution: { width: 72, height: 52 }, skeleton: { lo: 128, hi: 300, mode: 'ends', fill: 2 } });      // hi is open above
    await rc.setVolume(new vpt.RAWReader(two, { width: NX, height: NY, depth: NZ }));
    if (rc.volume.nativeFormat() !== N.VPT_FORMAT_R8) { throw new Error('RenderingContext did not keep the format'); }
    const tex = rc.volume.readBlock(0, 0, 0, NX, NY, NZ);
    rc.chooseRenderer('mip');
    rc.renderer.render();
    rc.destroy();
    fs.writeFileSync(outPath, Buffer.concat([Buffer.from(two.buffer), Buffer.from(tex.buffer)]));
    console.log('js skeleton gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
