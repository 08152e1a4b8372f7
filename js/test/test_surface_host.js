'use strict';
// node js/test/test_surface_host.js — no device: the plain-JS statement of the surface-nets contract (js/vpt/surface.js): the worked
// example to the digit, the arrays the numpy statement wrote for the small volumes of tests/golden/surface_cases.json, the range of t,
// what is asked of a mesh (closed, oriented, positive volume, triangles, positions), refusals, and the writers read back.
const fs = require('fs');
const os = require('os');
const path = require('path');
const s = require('../vpt/surface.js');

function throws(f, what, pattern) {
    let message = null;
    try { f(); } catch (e) { message = e.message; }
    if (message === null) { throw new Error(what + ' was accepted'); }
    if (pattern && !pattern.test(message)) { throw new Error(what + ': unexpected message ' + message); }
}
function same(a, b, what) {
    if (a.length !== b.length) { throw new Error(`${what}: length ${a.length}, expected ${b.length}`); }
    for (let i = 0; i < a.length; i++) { if (a[i] !== b[i]) { throw new Error(`${what}: element ${i} is ${a[i]}, expected ${b[i]}`); } }
}
function check(cond, what) { if (!cond) { throw new Error(what); } }

// ---- the worked example
{
    const t = new Uint8Array(27); t[13] = 255;
    const r = s.surfaceTexels(t, 3, 3, 3, 128);
    check(r.vertices instanceof Uint32Array && r.quads instanceof Uint32Array, 'typed arrays');
    check(r.info.vertices === 8 && r.info.quads === 6 && r.info.cells === 64 && r.info.inside === 1, 'worked example: counts');
    same(r.vertices.slice(0, 3), [120149, 120149, 120149], 'the vertex of cell (0, 0, 0)');
    same(r.vertices.slice(21), [141995, 141995, 141995], 'the vertex of cell (1, 1, 1)');
    same(r.info.crossings, [2, 2, 2], 'crossings');
    check(s.crossingT(0, 255, 128) === 32768, 't of the worked example');
}
// ---- t at the extreme levels
for (const M of [255, 65535]) {
    for (const level of [1, M]) {
        for (const a of [0, level - 1]) { for (const b of [level, M]) {
            for (const t of [s.crossingT(a, b, level), s.crossingT(b, a, level)]) { check(t >= 1 && t <= 65535, `t = ${t} at level ${level} of ${M}`); }
        } }
    }
}
check(s.crossingT(0, 65535, 1) === 1 && s.crossingT(0, 65535, 65535) === 65535, 'the extremes of t');

// ---- the shared arrays
const cases = JSON.parse(fs.readFileSync(path.join(__dirname, '..', '..', 'tests', 'golden', 'surface_cases.json'), 'utf8'));
check(cases.length >= 8, 'the fixture holds the cases');
for (const c of cases) {
    const texels = (c.bits === 8 ? Uint8Array : Uint16Array).from(c.texels);
    const r = s.surfaceTexels(texels, c.nx, c.ny, c.nz, c.level, c.channel, c.channels);
    same(r.vertices, c.vertices, c.name + ': vertices');
    same(r.quads, c.quads, c.name + ': quads');
    check(JSON.stringify(r.info) === JSON.stringify(c.info), `${c.name}: info ${JSON.stringify(r.info)}, expected ${JSON.stringify(c.info)}`);
    // closed and oriented: every directed edge occurs as often as its reverse
    const directed = new Map();
    for (let q = 0; q < r.quads.length; q += 4) { for (let k = 0; k < 4; k++) {
        const key = r.quads[q + k] + ' ' + r.quads[q + (k + 1) % 4];
        directed.set(key, (directed.get(key) || 0) + 1);
    } }
    for (const [key, n] of directed) { const [a, b] = key.split(' '); check(directed.get(b + ' ' + a) === n, `${c.name}: edge ${key} has no twin`); }
    if (c.name === 'soft ball') {
        const vol = s.surfaceVolume(r.vertices, r.quads), area = s.surfaceArea(r.vertices, r.quads);
        check(vol > 0 && area > 0, 'the soft ball encloses a volume');
        check(Math.abs(s.surfaceVolume(r.vertices, r.quads, [2, 3, 0.5]) / vol - 3) < 1e-12, 'spacing scales the volume');
        const n = s.surfaceNormals(r.vertices, r.quads), p = s.surfacePositions(r.vertices);
        for (let i = 0; i < n.length; i += 3) { check(n[i] * (p[i] - 4) + n[i + 1] * (p[i + 1] - 3.5) + n[i + 2] * (p[i + 2] - 3) > 0, 'a normal points inwards'); }
    }
}

// ---- triangles, positions, refusals
{
    const t = new Uint8Array(27); t[13] = 255;
    const r = s.surfaceTexels(t, 3, 3, 3, 128);
    const tri = s.surfaceTriangles(r.quads);
    same(tri.slice(0, 6), [r.quads[0], r.quads[1], r.quads[2], r.quads[0], r.quads[2], r.quads[3]], 'triangles');
    const p = s.surfacePositions(r.vertices, [2, 1, 0.5], [10, 0, -1]);
    check(p[0] === (120149 / 65536 - 1) * 2 + 10 && p[2] === (120149 / 65536 - 1) * 0.5 - 1, 'positions');
    throws(() => s.surfaceTexels(t, 3, 3, 3, 0), 'level 0', /1 <= level <= 255/);
    throws(() => s.surfaceTexels(t, 3, 3, 3, 256), 'level 256', /1 <= level <= 255/);
    throws(() => s.surfaceTexels(new Uint16Array(27), 3, 3, 3, 65536), 'level 65536', /1 <= level <= 65535/);
    throws(() => s.surfaceTexels(t, 3, 3, 3, 1.5), 'level 1.5', /integer/);
    throws(() => s.surfaceTexels(t, 3, 3, 3, 1, 1), 'channel 1 of one', /one channel/);
    throws(() => s.surfaceTexels(t, 3, 3, 3, 1, 2, 2), 'channel 2', /Uint8Array|channel is 0 or 1/);
    throws(() => s.surfaceTexels(new Float32Array(27), 3, 3, 3, 1), 'float texels', /Uint8Array or Uint16Array/);
    throws(() => s.surfaceTexels(t, 3, 3, 2, 1), 'wrong length', /Uint8Array or Uint16Array/);
    throws(() => s.surfacePositions(r.vertices, [1, 0, 1]), 'spacing 0', /positive/);
    throws(() => s.checkSurfaceWindow(9, null, 8, 'vertices'), 'window past the end', /not within/);
    same(s.checkSurfaceWindow(8, null, 8, 'vertices'), [8, 0], 'the empty window at the end');

    // ---- the writers, read back
    const dir = fs.mkdtempSync(path.join(os.tmpdir(), 'vpt-surface-'));
    const sp = [0.5, 0.25, 2], o = [-3, 1, 100], pos = s.surfacePositions(r.vertices, sp, o);
    s.writeStl(path.join(dir, 'a.stl'), r.vertices, r.quads, sp, o);
    s.writePly(path.join(dir, 'a.ply'), r.vertices, r.quads, sp, o);
    s.writeObj(path.join(dir, 'a.obj'), r.vertices, r.quads, sp, o);
    const stl = fs.readFileSync(path.join(dir, 'a.stl'));
    check(stl.length === 84 + 50 * 12 && stl.readUInt32LE(80) === 12, 'STL size');
    for (let k = 0; k < 12; k++) { for (let c = 0; c < 3; c++) { for (let a = 0; a < 3; a++) {
        check(stl.readFloatLE(84 + 50 * k + 12 + 12 * c + 4 * a) === Math.fround(pos[3 * tri[3 * k + c] + a]), 'STL corner');
    } } }
    const ply = fs.readFileSync(path.join(dir, 'a.ply')), end = ply.indexOf('end_header\n') + 11;
    check(ply.slice(0, end).toString('ascii').includes('element vertex 8\n') && ply.length === end + 12 * 8 + 17 * 6, 'PLY size');
    for (let i = 0; i < 24; i++) { check(ply.readFloatLE(end + 4 * i) === Math.fround(pos[i]), 'PLY vertex'); }
    for (let f = 0; f < 6; f++) {
        check(ply.readUInt8(end + 96 + 17 * f) === 4, 'PLY face size');
        for (let k = 0; k < 4; k++) { check(ply.readUInt32LE(end + 96 + 17 * f + 1 + 4 * k) === r.quads[4 * f + k], 'PLY face'); }
    }
    const obj = fs.readFileSync(path.join(dir, 'a.obj'), 'utf8').split('\n');
    const vs = obj.filter(l => l.startsWith('v ')).map(l => l.split(' ').slice(1).map(Number)), fsq = obj.filter(l => l.startsWith('f ')).map(l => l.split(' ').slice(1).map(Number));
    check(vs.length === 8 && fsq.length === 6, 'OBJ counts');
    vs.forEach((v, i) => same(v, pos.slice(3 * i, 3 * i + 3), 'OBJ vertex'));
    fsq.forEach((f, i) => same(f, Array.from(r.quads.slice(4 * i, 4 * i + 4)).map(x => x + 1), 'OBJ face'));
    for (const f of fs.readdirSync(dir)) { fs.unlinkSync(path.join(dir, f)); }
    fs.rmdirSync(dir);
}
console.log('js surface host ok');
