'use strict';
// node js/test/test_combine_gpu.js OUT — GPU: the Node.js host's two-volume operations.  Two (23, 19, 21) volumes of uniform noise, uint8
// and uint16, through Volume.combine (every op, a two-channel second volume, a mask of the other width) and Volume.compare: the texels read
// back (readBlock) and the counts must equal the plain-JS twin of the contract (js/vpt/combine.js).  Then
// RenderingContext({ combine, rank, smooth }) once with a reader for the second volume on another grid: the two sources and the texels of
// what the context ends up with are written to OUT (tests/test_js_gpu_combine.py compares them with the numpy chain).
const fs = require('fs');
const vpt = require('../vpt/index.js');
const { native } = require('../vpt/native.js');

const NX = 21, NY = 19, NZ = 23;
const MX = 13, MY = 11, MZ = 9;

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
function sameStats(got, want, what) {
    for (const k of Object.keys(want)) { if (got[k] !== want[k]) { throw new Error(`${what}: ${k} is ${got[k]}, expected ${want[k]}`); } }
}

async function main() {
    const outPath = process.argv[2];
    const N = native();
    const ctx = new vpt.Context(0);
    if (!ctx.getExtension('EXT_texture_norm16')) { throw new Error('no EXT_texture_norm16'); }
    let seed = 86420;
    const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
    const n = NX * NY * NZ, whole = [0, 0, 0, NX, NY, NZ];
    const upload = async (texels, bits) => {
        const v = new vpt.Volume(ctx, new vpt.RAWReader(new Uint8Array(texels.buffer), { width: NX, height: NY, depth: NZ, bits: bits }));
        await v.load();
        return v;
    };
    for (const bits of [8, 16]) {
        const Ctor = bits === 8 ? Uint8Array : Uint16Array, Other = bits === 8 ? Uint16Array : Uint8Array, M = bits === 8 ? 255 : 65535, Mo = bits === 8 ? 65535 : 255;
        const a = new Ctor(n), b = new Ctor(n), o = new Other(n);
        for (let i = 0; i < n; i++) { a[i] = rand() & M; b[i] = rand() & M; o[i] = rand() & Mo; }
        const va = await upload(a, bits), vb = await upload(b, bits), vo = await upload(o, 24 - bits);
        const label = va.pair(vb);                                // a two-channel volume made on the device: (a, b)
        if (!label.ready || label.nativeFormat() !== (bits === 8 ? N.VPT_FORMAT_RG8 : N.VPT_FORMAT_RG16)) { throw new Error('pair: wrong description'); }
        const two = label.readBlock(0, 0, 0, NX, NY, NZ);
        equal(two, vpt.combineTexels(a, b, 'pair'), `pair, ${bits} bits`);
        const lo = M >> 2, hi = M - (M >> 2);
        const cases = [['mask', { lo, hi, fill: M - 1 }], ['min', {}], ['max', {}], ['absdiff', {}], ['blend', { wa: 256, wb: -256, offset: (M + 1) / 2 }],
            ['blend', { wa: 77, wb: 151, offset: 3 }], ['blend', { wa: -4096, wb: -4096, offset: M }], ['blend', { wa: 512, wb: -256, offset: 0 }]];
        for (const [op, options] of cases) {
            const what = `${op} ${JSON.stringify(options)}, ${bits} bits`;
            const d = va.combine(vb, op, options);
            if (!d.ready || d.nativeFormat() !== va.nativeFormat() || d.modality.dimensions.width !== NX) { throw new Error(what + ': wrong description'); }
            equal(d.readBlock.apply(d, whole), vpt.combineTexels(a, b, op, options), what);
            const c1 = va.combine(label, op, Object.assign({ channel: 1 }, options));
            equal(c1.readBlock.apply(c1, whole), vpt.combineTexels(a, two, op, Object.assign({ channels: 2, channel: 1 }, options)), what + ', channel 1');
            d.destroy(); c1.destroy();
        }
        const mixed = va.mask(vo, Mo >> 1, Mo, 5);
        equal(mixed.readBlock.apply(mixed, whole), vpt.combineTexels(a, o, 'mask', { lo: Mo >> 1, hi: Mo, fill: 5 }), `a mask of the other width, ${bits} bits`);
        mixed.destroy();
        const timed = va.combineTimed(vb, 'max');
        equal(timed[0].readBlock.apply(timed[0], whole), vpt.combineTexels(a, b, 'max'), 'combineTimed');
        if (!(timed[1] > 0)) { throw new Error('combineTimed: no time'); }
        timed[0].destroy();
        equal(va.readBlock.apply(va, whole), a, 'the first source afterwards'); equal(vb.readBlock.apply(vb, whole), b, 'the second source afterwards');
        sameStats(va.compare(vb, [lo, hi], [0, M >> 1]), vpt.compareStats(a, b, { aRange: [lo, hi], bRange: [0, M >> 1] }), `compare, ${bits} bits`);
        sameStats(va.compare(vo), vpt.compareStats(a, o), `compare, mixed widths, ${bits} bits`);
        sameStats(va.compare(label, [lo, hi], [lo, hi], 1), vpt.compareStats(a, two, { channels: 2, channel: 1, aRange: [lo, hi], bRange: [lo, hi] }), `compare, channel 1, ${bits} bits`);
        const same = va.compare(label);
        if (same.differing !== 0n || same.sumSq !== 0n || same.psnr !== null || same.dice !== 1 || typeof same.voxels !== 'bigint') { throw new Error('compare of identical texels'); }
        throws(() => va.combine(vb, 'mean'), "combine(vb, 'mean')", /combine op is/);
        throws(() => va.combine(vb, 'min', { channel: 1 }), 'channel 1 of a one-channel volume', /channel 1/);
        throws(() => va.blend(vb, 5000, 0), 'blend(5000, 0)', /blend weight wa/);
        throws(() => va.mask(vb, 3, 2), 'mask(3, 2)', /mask range/);
        throws(() => va.combine(vb, 'min', { scale: 2 }), 'an unknown option', /scale/);
        throws(() => va.combine({}, 'min'), 'no volume', /two ready volumes/);
        throws(() => va.minimum(vo), 'min of two widths', /R8.*R16|R16.*R8/);
        throws(() => label.minimum(va), 'a two-channel first volume', /RG(8|16)/);
        for (const vol of [label, va, vb, vo]) { vol.destroy(); }
    }
    ctx.destroy();
    // the context path
    for (const bad of ['mask', { op: 'min' }, { reader: {}, op: 'mean' }, { reader: {}, op: 'blend' }]) {
        throws(() => new vpt.RenderingContext({ combine: bad }), 'RenderingContext({ combine: ' + JSON.stringify(bad) + ' })');
    }
    throws(() => new vpt.RenderingContext({ gradient: 'sobel', combine: { reader: {}, op: 'pair' } }), "'pair' with gradient", /second channel/);
    const v = new Uint8Array(n), m = new Uint8Array(MX * MY * MZ);
    for (let i = 0; i < n; i++) { v[i] = rand() & 255; }
    for (let i = 0; i < m.length; i++) { m[i] = rand() & 255; }
    const second = new vpt.RAWReader(m, { width: MX, height: MY, depth: MZ });
    const rc = new vpt.RenderingContext({ resolution: { width: 72, height: 52 }, rank: 'median', smooth: 1,
        combine: { reader: second, op: 'mask', lo: 64, hi: 255, fill: 2, resample: 'nearest' } });
    await rc.setVolume(new vpt.RAWReader(v, { width: NX, height: NY, depth: NZ }));
    if (rc.volume.nativeFormat() !== N.VPT_FORMAT_R8) { throw new Error('RenderingContext did not run the chain'); }
    const tex = rc.volume.readBlock(0, 0, 0, NX, NY, NZ);
    rc.chooseRenderer('mip');
    rc.renderer.render();
    rc.destroy();
    fs.writeFileSync(outPath, Buffer.concat([Buffer.from(v.buffer), Buffer.from(m.buffer), Buffer.from(tex.buffer)]));
    console.log('js combine gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
