'use strict';
// node js/test/test_surface_gpu.js OUT — GPU: the Node.js host's surface.  Noise in 37 x 11 x 6 (the padded row crosses a word edge) at
// levels 1, 128 and 255, uint8 and uint16, both channels of a two-channel volume, a structure on the faces, one voxel, a full volume and
// the empty result, through Volume.surface, its info, vertices and quads (whole and paged), the capped scan, the mesh measures, the
// writers and profile: every value must equal the plain-JS statement of the contract (js/vpt/surface.js).  Then the texels of the first
// noise volume and its vertices and quads at level 128 are written to OUT (tests/test_js_gpu_surface.py compares them with the numpy
// statement).
const fs = require('fs');
const os = require('os');
const path = require('path');
const vpt = require('../vpt/index.js');

function equal(a, b, what) {
    if (a.constructor !== b.constructor || a.length !== b.length) { throw new Error(`${what}: wrong array (${a.length}, expected ${b.length})`); }
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
function noise(n, bits) {
    const out = new (bits === 8 ? Uint8Array : Uint16Array)(n);
    for (let i = 0; i < n; i++) { out[i] = rand() % (bits === 8 ? 256 : 65536); }
    return out;
}

async function main() {
    const outPath = process.argv[2];
    const ctx = new vpt.Context(0);
    if (!ctx.getExtension('EXT_texture_norm16')) { throw new Error('no EXT_texture_norm16'); }
    const uploadTo = async (texels, bits, dims) => {
        const v = new vpt.Volume(ctx, new vpt.RAWReader(new Uint8Array(texels.buffer), { width: dims[0], height: dims[1], depth: dims[2], bits: bits }));
        await v.load();
        return v;
    };
    const check = (vol, texels, dims, level, channel, channels, scanWords, what) => {
        const want = vpt.surfaceTexels(texels, dims[0], dims[1], dims[2], level, channel, channels);
        const s = vol.surface(level, channel, scanWords);
        if (JSON.stringify(s.info) !== JSON.stringify(want.info)) { throw new Error(`${what}: info ${JSON.stringify(s.info)}, expected ${JSON.stringify(want.info)}`); }
        equal(s.vertices(), want.vertices, what + ': vertices');
        equal(s.quads(), want.quads, what + ': quads');
        return [s, want];
    };
    const dims = [37, 11, 6], n = 37 * 11 * 6;
    let first = null, firstMesh = null;
    for (const bits of [8, 16]) {
        const M = bits === 8 ? 255 : 65535, texels = noise(n, bits);
        texels[100] = M;
        const vol = await uploadTo(texels, bits, dims);
        for (const level of [1, (M + 1) / 2, M]) {
            for (const scanWords of [undefined, 2]) {
                const [s, want] = check(vol, texels, dims, level, 0, 1, scanWords, `${bits} bits, level ${level}, scan ${scanWords}`);
                if (bits === 8 && level === 128 && scanWords === undefined) {
                    first = texels; firstMesh = want;
                    // paged reads tile the arrays; windows past the end are refused
                    const nv = want.info.vertices, nq = want.info.quads, pv = [], pq = [];
                    for (let at = 0; at < nv; at += 101) { pv.push(...s.vertices(at, Math.min(101, nv - at))); }
                    for (let at = 0; at < nq; at += 77) { pq.push(...s.quads(at, Math.min(77, nq - at))); }
                    equal(Uint32Array.from(pv), want.vertices, 'paged vertices'); equal(Uint32Array.from(pq), want.quads, 'paged quads');
                    if (s.vertices(nv).length !== 0 || s.quads(nq, 0).length !== 0) { throw new Error('the empty window at the end'); }
                    throws(() => s.vertices(nv + 1), 'vertices past the end', /not within/);
                    throws(() => s.quads(1, nq), 'quads past the end', /not within/);
                    // measures and writers go through the statement's functions on the device's arrays
                    if (s.area() !== vpt.surfaceArea(want.vertices, want.quads) || s.volume([1, 2, 3]) !== vpt.surfaceVolume(want.vertices, want.quads, [1, 2, 3])) { throw new Error('area / volume'); }
                    equal(s.triangles(), vpt.surfaceTriangles(want.quads), 'triangles');
                    equal(s.positions([2, 2, 2], [1, 0, 0]), vpt.surfacePositions(want.vertices, [2, 2, 2], [1, 0, 0]), 'positions');
                    equal(s.normals(), vpt.surfaceNormals(want.vertices, want.quads), 'normals');
                    const dir = fs.mkdtempSync(path.join(os.tmpdir(), 'vpt-surface-gpu-'));
                    for (const [name, mine, theirs] of [['stl', 'writeStl', vpt.writeStl], ['ply', 'writePly', vpt.writePly], ['obj', 'writeObj', vpt.writeObj]]) {
                        s[mine](path.join(dir, 'a.' + name), [1, 2, 3], [0, 0, 1]);
                        theirs(path.join(dir, 'b.' + name), want.vertices, want.quads, [1, 2, 3], [0, 0, 1]);
                        if (!fs.readFileSync(path.join(dir, 'a.' + name)).equals(fs.readFileSync(path.join(dir, 'b.' + name)))) { throw new Error(name + ' files differ'); }
                    }
                    for (const f of fs.readdirSync(dir)) { fs.unlinkSync(path.join(dir, f)); }
                    fs.rmdirSync(dir);
                    const p = s.profile;
                    for (const k of ['inside', 'classify', 'scan', 'vertices', 'quads']) { if (!(p[k] > 0)) { throw new Error('profile.' + k); } }
                }
                s.destroy();
                throws(() => s.vertices(), 'a destroyed surface', /destroyed/);
            }
        }
        throws(() => vol.surface(0), 'level 0', /1 <= level/);
        throws(() => vol.surface(M + 1), 'level M + 1', /1 <= level/);
        throws(() => vol.surface(1, 1), 'channel 1 of one channel', /one channel/);
        // the surface outlives its volume
        const s = vol.surface(7), want = vpt.surfaceTexels(texels, dims[0], dims[1], dims[2], 7);
        vol.destroy();
        equal(s.vertices(), want.vertices, 'after the volume is gone');
        s.close();
    }
    // small shapes: one voxel, a full volume, the empty result, a structure on all six faces
    {
        const one = Uint8Array.from([200]), v1 = await uploadTo(one, 8, [1, 1, 1]);
        check(v1, one, [1, 1, 1], 128, 0, 1, undefined, 'one voxel')[0].destroy();
        v1.destroy();
        const full = new Uint8Array(24).fill(255), v2 = await uploadTo(full, 8, [4, 3, 2]);
        const [s2, w2] = check(v2, full, [4, 3, 2], 1, 0, 1, undefined, 'a full volume');
        if (w2.info.vertices !== 54 || w2.info.quads !== 52) { throw new Error('a full 4 x 3 x 2 volume has 54 vertices and 52 quads'); }
        s2.destroy();
        const [s3] = check(v2, full, [4, 3, 2], 1, 0, 1, 1, 'a full volume, one word a scan block'); s3.destroy();
        v2.destroy();
        const flat = new Uint8Array(40 * 5 * 4).fill(9), v3 = await uploadTo(flat, 8, [40, 5, 4]);
        const [s4] = check(v3, flat, [40, 5, 4], 10, 0, 1, undefined, 'the empty result');
        if (s4.info.vertices !== 0 || s4.profile.vertices !== 0 || s4.profile.quads !== 0 || s4.triangles().length !== 0) { throw new Error('the empty result ran an emit kernel'); }
        s4.destroy(); v3.destroy();
        const d = [35, 10, 9], faces = new Uint8Array(35 * 10 * 9).fill(30);
        for (let z = 0, i = 0; z < 9; z++) { for (let y = 0; y < 10; y++) { for (let x = 0; x < 35; x++, i++) {
            const ax = Math.abs(x - 17) <= 1, ay = Math.abs(y - 5) <= 1, az = Math.abs(z - 4) <= 1;
            if ((ay && az) || (ax && az) || (ax && ay)) { faces[i] = 220; }
        } } }
        const v4 = await uploadTo(faces, 8, d);
        check(v4, faces, d, 128, 0, 1, 3, 'a structure on all six faces')[0].destroy();
        v4.destroy();
    }
    // both channels of a gradient-magnitude volume (RG8): the texels come back through readBlock
    {
        const base = noise(n, 8), vol = await uploadTo(base, 8, dims), rg = vol.deriveGradient({ operator: 'central', gain: 1 });
        const texels = rg.readBlock(0, 0, 0, dims[0], dims[1], dims[2]);
        for (const channel of [0, 1]) { check(rg, texels, dims, 60, channel, 2, undefined, 'RG8 channel ' + channel)[0].destroy(); }
        throws(() => rg.surface(60, 2), 'channel 2', /channel is 0 or 1/);
        rg.destroy(); vol.destroy();
    }
    const out = Buffer.concat([Buffer.from(first.buffer), Buffer.from(firstMesh.vertices.buffer), Buffer.from(firstMesh.quads.buffer)]);
    fs.writeFileSync(outPath, out);
    ctx.destroy();
    console.log('js surface gpu ok');
}
main().catch((e) => { console.error(e.stack || String(e)); process.exit(1); });
