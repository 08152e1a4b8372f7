'use strict';
// node js/test/test_components_gpu.js OUT — GPU: the Node.js host's connected components.  Uniform noise, uint8 and uint16, on a
// (23, 19, 21) volume and on one that passes the 64 x 8 x 4 labelling tile by one voxel on every axis, through Volume.components: the ranks,
// the list, the info and the texels of keep() and label() must equal the plain-JS twins (js/vpt/components.js).  Then
// RenderingContext({ components: { mode: 'keep' } }) and ({ mode: 'label' }) once each over an 8-bit RAW volume: the texels the context ends
// up with are written to OUT (tests/test_js_gpu_components.py compares them with the numpy statement).
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
    let seed = 97531;
    const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
    for (const [NX, NY, NZ] of [[23, 19, 21], [65, 9, 5]]) {
        for (const bits of [8, 16]) {
            const Ctor = bits === 8 ? Uint8Array : Uint16Array, M = bits === 8 ? 255 : 65535;
            const texels = new Ctor(NX * NY * NZ);
            for (let i = 0; i < texels.length; i++) { texels[i] = rand() & M; }
            const v = new vpt.Volume(ctx, new vpt.RAWReader(new Uint8Array(texels.buffer), { width: NX, height: NY, depth: NZ, bits: bits }));
            await v.load();
            for (const [connectivity, fraction, minVoxels] of [[6, 0.30, 1], [18, 0.13, 2], [26, 0.09, 1]]) {
                const lo = (M + 1) >> 2, hi = lo + Math.round(fraction * (M + 1)), what = `${NX} x ${NY} x ${NZ}, ${bits} bits, ${connectivity}`;
                const want = vpt.componentsTexels(texels, NX, NY, NZ, lo, hi, connectivity, minVoxels);
                if (want.list.length < 16) { throw new Error(what + ': degenerate input'); }
                const c = v.components(lo, hi, connectivity, minVoxels);
                equal(c.ranks(), want.ranks, what + ': ranks');
                if (JSON.stringify(c.list()) !== JSON.stringify(want.list)) { throw new Error(what + ': list'); }
                if (JSON.stringify(c.list(1, 2)) !== JSON.stringify(want.list.slice(1, 3))) { throw new Error(what + ': list(1, 2)'); }
                let voxels = 0;
                for (const e of want.list) { voxels += e[3]; }
                const info = c.info;
                if (info.listed !== want.list.length || info.listedVoxels !== voxels || info.foregroundVoxels < voxels) { throw new Error(what + ': info ' + JSON.stringify(info)); }
                const all = c.keep(), some = c.keep(2, 3, 7), pair = c.label();
                if (!all.ready || all.nativeFormat() !== v.nativeFormat() || pair.nativeFormat() !== (bits === 8 ? N.VPT_FORMAT_RG8 : N.VPT_FORMAT_RG16) ||
                    pair.modality.internalFormat !== (bits === 8 ? GL.GL_RG8 : GL.GL_RG16_EXT)) { throw new Error(what + ': formats of the derived volumes'); }
                equal(all.readBlock(0, 0, 0, NX, NY, NZ), vpt.keepTexels(texels, want.ranks), what + ': keep()');
                equal(some.readBlock(0, 0, 0, NX, NY, NZ), vpt.keepTexels(texels, want.ranks, 2, 3, 7), what + ': keep(2, 3, 7)');
                equal(pair.readBlock(0, 0, 0, NX, NY, NZ), vpt.labelTexels(texels, want.ranks), what + ': label()');
                throws(() => c.keep(0, 1), 'keep(0, 1)'); throws(() => c.keep(2, 1), 'keep(2, 1)'); throws(() => c.keep(1, 1, M + 1), 'keep with a fill beyond the format');
                throws(() => c.list(0, want.list.length + 1), 'a list beyond the end');
                for (const vol of [all, some, pair]) { vol.destroy(); }
                c.destroy();
                throws(() => c.ranks(), 'ranks of destroyed components');
            }
            const largest = v.keepLargest(0, M >> 2), want = vpt.componentsTexels(texels, NX, NY, NZ, 0, M >> 2, 6, 1);
            equal(largest.readBlock(0, 0, 0, NX, NY, NZ), vpt.keepTexels(texels, want.ranks, 1, 1, 0), 'keepLargest');
            const islands = v.removeIslands(0, M >> 2, 4, 18), want18 = vpt.componentsTexels(texels, NX, NY, NZ, 0, M >> 2, 18, 4);
            equal(islands.readBlock(0, 0, 0, NX, NY, NZ), vpt.keepTexels(texels, want18.ranks), 'removeIslands');
            equal(v.readBlock(0, 0, 0, NX, NY, NZ), texels, 'the source afterwards');
            for (const bad of [[5, 4], [0, M + 1], [0, 1, 8], [0, 1, 6, 0], [0.5, 1]]) { throws(() => v.components(...bad), 'components(' + JSON.stringify(bad) + ')'); }
            const g = v.deriveGradient({ operator: 'central' });
            let named = '';
            try { g.components(0, 1); } catch (err) { named = err.message; }      // a two-channel source: the library names the format
            if (!/RG(8|16)/.test(named)) { throw new Error('components of a two-channel volume: ' + named); }
            for (const vol of [g, largest, islands, v]) { vol.destroy(); }
        }
    }
    ctx.destroy();
    // the context path
    const good = { lo: 0, hi: 76, mode: 'keep' };
    for (const bad of ['keep', { lo: 0, hi: 1 }, Object.assign({}, good, { mode: 'drop' }), Object.assign({}, good, { lo: 77 }), Object.assign({}, good, { connectivity: 8 }),
        Object.assign({}, good, { minVoxels: 0 }), Object.assign({}, good, { keep: 0 }), Object.assign({}, good, { mode: 'label', keep: 1 })]) {
        throws(() => new vpt.RenderingContext({ components: bad }), 'RenderingContext({ components: ' + JSON.stringify(bad) + ' })');
    }
    throws(() => new vpt.RenderingContext({ gradient: 'sobel', components: Object.assign({}, good, { mode: 'label' }) }), 'gradient with mode label');
    const NX = 21, NY = 19, NZ = 23;
    const bytes = new Uint8Array(NX * NY * NZ);
    for (let i = 0; i < bytes.length; i++) { bytes[i] = rand() & 255; }
    const parts = [Buffer.from(bytes.buffer)];
    for (const components of [{ lo: 0, hi: 76, connectivity: 6, minVoxels: 2, mode: 'keep', keep: 3 }, { lo: 0, hi: 80, connectivity: 18, minVoxels: 2, mode: 'label' }]) {
        const rc = new vpt.RenderingContext({ resolution: { width: 72, height: 52 }, rank: 'median', components });
        await rc.setVolume(new vpt.RAWReader(bytes, { width: NX, height: NY, depth: NZ }));
        const two = components.mode === 'label';
        if (rc.volume.nativeFormat() !== (two ? N.VPT_FORMAT_RG8 : N.VPT_FORMAT_R8)) { throw new Error('RenderingContext did not run the chain'); }
        parts.push(Buffer.from(rc.volume.readBlock(0, 0, 0, NX, NY, NZ).buffer));
        rc.chooseRenderer('mip');
        rc.renderer.render();
        rc.destroy();
    }
    fs.writeFileSync(outPath, Buffer.concat(parts));
    console.log('js components gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
