'use strict';
// The isosurface of a volume as a mesh by naive surface nets in plain JS: the contract of include/vpt.h (vpt_volume_surface) restated for
// hosts without a device, the twin of vpt_amd/surface.py, and what is asked of a mesh next (triangles, positions, area, volume, normals,
// the STL / PLY / OBJ writers).
//   texels: a Uint8Array / Uint16Array [nz][ny][nx]([channels]); 1 <= level <= M (255 or 65535); the surface lies at code level - 1/2
//   grid: voxel (x, y, z) is the grid point at those coordinates; the grid is padded by one layer on every side (-1 .. W, H, D); code(g)
//   is the whole unsigned code inside the volume and 0 outside; inside(g) = code(g) >= level
//   cells: c = (i, j, k), -1 <= i <= W - 1 (likewise j, k), with the corners c + o, o in {0, 1}^3, and twelve edges
//   crossing: an edge (g, g + e_a) crosses when inside differs at its ends; a = code(g), b = code(g + e_a), n = |2 level - 1 - 2 a|,
//   d = 2 |b - a|, t = (n 65536 + d / 2) div d; the crossing point is g 65536 + t e_a
//   vertex: a cell with m >= 1 crossing edges; per axis s = the sum of (crossing point - c 65536), q = (c_axis + 1) 65536 + (2 s + m) div (2 m);
//   the position is q / 65536 - 1; numbered in raster order of the cells (k slowest, then j, i)
//   quads: per crossing edge (g, a), u = (a + 1) mod 3, v = (a + 2) mod 3: the vertices of the cells g - e_u - e_v, g - e_v, g, g - e_u, in
//   that order when inside(g), otherwise [0, 3, 2, 1] of that list; numbered by g in raster order, then by axis x, y, z
// Every number stays below 2^53, so the doubles are exact integers.
const fs = require('fs');

const ONE = 65536;
const SURFACE_INFO_FIELDS = ['vertices', 'quads', 'cells', 'inside', 'crossings', 'level', 'width', 'height', 'depth', 'channel'];

function checkSurfaceChannel(channel, channels) {
    if (channel !== 0 && channel !== 1) { throw new Error(`channel is 0 or 1, not ${JSON.stringify(channel)}`); }
    if (channel >= channels) { throw new Error('channel 1 of a volume that has one channel'); }
    return channel;
}
function checkSurfaceLevel(level, largest) {
    if (!Number.isInteger(level)) { throw new Error(`the level of a surface is an integer, not ${JSON.stringify(level)}`); }
    if (level < 1 || level > largest) { throw new Error(`surface level ${level}: 1 <= level <= ${largest}`); }
    return level;
}
// [first, n]: integers with 0 <= first <= count and 0 <= n <= count - first (n null / undefined: to the end)
function checkSurfaceWindow(first, n, count, what) {
    if (!Number.isInteger(first) || first < 0 || first > count) { throw new Error(`${what} ${JSON.stringify(first)} .. are not within the ${count} of the surface`); }
    if (n === null || n === undefined) { n = count - first; }
    if (!Number.isInteger(n) || n < 0 || n > count - first) { throw new Error(`${what} ${first} .. +${JSON.stringify(n)} are not within the ${count} of the surface`); }
    return [first, n];
}

function crossingT(a, b, level) {
    const n = Math.abs(2 * level - 1 - 2 * a), d = 2 * Math.abs(b - a);
    return Math.floor((n * ONE + Math.floor(d / 2)) / d);
}

// { vertices: Uint32Array [V][3], quads: Uint32Array [Q][4], info } of the surface at `level` of channel `channel` (default 0) of
// `channels` (default 1) interleaved channels
function surfaceTexels(texels, nx, ny, nz, level, channel, channels) {
    channels = channels === undefined ? 1 : channels; channel = channel === undefined ? 0 : channel;
    if (!(texels instanceof Uint8Array || texels instanceof Uint16Array) || (channels !== 1 && channels !== 2) || ![nx, ny, nz].every(Number.isInteger) ||
        nx < 1 || ny < 1 || nz < 1 || texels.length !== nx * ny * nz * channels) {
        throw new Error('the surface takes a Uint8Array or Uint16Array [nz][ny][nx] or [nz][ny][nx][2]');
    }
    if (Math.max(nx, ny, nz) > 4096) { throw new Error('the surface takes at most 4096 voxels an axis'); }
    checkSurfaceChannel(channel, channels);
    checkSurfaceLevel(level, texels instanceof Uint8Array ? 255 : 65535);
    const dims = [nx, ny, nz];
    const code = (x, y, z) => (x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz) ? texels[((z * ny + y) * nx + x) * channels + channel] : 0;
    const cellAt = (i, j, k) => ((k + 1) * (ny + 1) + (j + 1)) * (nx + 1) + (i + 1);
    const number = new Int32Array((nx + 1) * (ny + 1) * (nz + 1)).fill(-1);
    const vertices = [], quads = [], crossings = [0, 0, 0];
    let inside = 0;
    for (let i = 0; i < nx * ny * nz; i++) { if (texels[i * channels + channel] >= level) { inside++; } }
    const c = [0, 0, 0], g = [0, 0, 0], s = [0, 0, 0];
    for (c[2] = -1; c[2] < nz; c[2]++) { for (c[1] = -1; c[1] < ny; c[1]++) { for (c[0] = -1; c[0] < nx; c[0]++) {
        let m = 0; s[0] = s[1] = s[2] = 0;
        for (let a = 0; a < 3; a++) {
            const u = (a + 1) % 3, v = (a + 2) % 3;
            for (let ou = 0; ou < 2; ou++) { for (let ov = 0; ov < 2; ov++) {
                g[0] = c[0]; g[1] = c[1]; g[2] = c[2]; g[u] += ou; g[v] += ov;
                const ca = code(g[0], g[1], g[2]);
                g[a] += 1;
                const cb = code(g[0], g[1], g[2]);
                if ((ca >= level) !== (cb >= level)) { m++; s[a] += crossingT(ca, cb, level); s[u] += ou * ONE; s[v] += ov * ONE; }
            } }
        }
        if (m) {
            number[cellAt(c[0], c[1], c[2])] = vertices.length / 3;
            for (let a = 0; a < 3; a++) { vertices.push((c[a] + 1) * ONE + Math.floor((2 * s[a] + m) / (2 * m))); }
        }
    } } }
    const h = [0, 0, 0];
    const at = (du, dv, u, v) => { h[0] = g[0]; h[1] = g[1]; h[2] = g[2]; h[u] -= du; h[v] -= dv; return number[cellAt(h[0], h[1], h[2])]; };
    for (g[2] = -1; g[2] <= nz; g[2]++) { for (g[1] = -1; g[1] <= ny; g[1]++) { for (g[0] = -1; g[0] <= nx; g[0]++) {
        const ca = code(g[0], g[1], g[2]);
        for (let a = 0; a < 3; a++) {
            if (g[a] + 1 > dims[a]) { continue; }
            g[a] += 1;
            const cb = code(g[0], g[1], g[2]);
            g[a] -= 1;
            if ((ca >= level) === (cb >= level)) { continue; }
            const u = (a + 1) % 3, v = (a + 2) % 3;
            const q0 = at(1, 1, u, v), q1 = at(0, 1, u, v), q2 = at(0, 0, u, v), q3 = at(1, 0, u, v);
            if (ca >= level) { quads.push(q0, q1, q2, q3); } else { quads.push(q0, q3, q2, q1); }
            crossings[a]++;
        }
    } } }
    const info = { vertices: vertices.length / 3, quads: quads.length / 4, cells: (nx + 1) * (ny + 1) * (nz + 1), inside, crossings, level,
        width: nx, height: ny, depth: nz, channel };
    return { vertices: Uint32Array.from(vertices), quads: Uint32Array.from(quads), info };
}

// ---- what is asked of a mesh ----
function triple(value, fallback, what) {
    const t = value === undefined || value === null ? fallback : Array.from(value);
    if (t.length !== 3 || !t.every(Number.isFinite)) { throw new Error(`${what} is three finite numbers (x, y, z), not ${JSON.stringify(value)}`); }
    return t;
}
// Uint32Array [2 Q][3]: the triangles (q0, q1, q2) and (q0, q2, q3) of every quad
function surfaceTriangles(quads) {
    const out = new Uint32Array(quads.length / 4 * 6);
    for (let q = 0; q < quads.length / 4; q++) {
        out.set([quads[4 * q], quads[4 * q + 1], quads[4 * q + 2], quads[4 * q], quads[4 * q + 2], quads[4 * q + 3]], 6 * q);
    }
    return out;
}
// Float64Array [V][3]: (q / 65536 - 1) * spacing + origin
function surfacePositions(vertices, spacing, origin) {
    const sp = triple(spacing, [1, 1, 1], 'spacing'), o = triple(origin, [0, 0, 0], 'origin');
    if (!sp.every(x => x > 0)) { throw new Error(`spacing is positive, not ${JSON.stringify(sp)}`); }
    const out = new Float64Array(vertices.length);
    for (let i = 0; i < vertices.length; i++) { out[i] = (vertices[i] / ONE - 1) * sp[i % 3] + o[i % 3]; }
    return out;
}
// f(a, b, c, corner indices) over the triangles, the corners as [x, y, z]
function eachTriangle(vertices, quads, spacing, origin, f) {
    const p = surfacePositions(vertices, spacing, origin), t = surfaceTriangles(quads);
    const corner = (i) => [p[3 * i], p[3 * i + 1], p[3 * i + 2]];
    for (let k = 0; k < t.length; k += 3) { f(corner(t[k]), corner(t[k + 1]), corner(t[k + 2]), [t[k], t[k + 1], t[k + 2]]); }
    return p;
}
const sub = (a, b) => [a[0] - b[0], a[1] - b[1], a[2] - b[2]];
const cross = (a, b) => [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]];
const dot = (a, b) => a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
function surfaceArea(vertices, quads, spacing) {
    let sum = 0;
    eachTriangle(vertices, quads, spacing, null, (a, b, c) => { const n = cross(sub(b, a), sub(c, a)); sum += 0.5 * Math.sqrt(dot(n, n)); });
    return sum;
}
function surfaceVolume(vertices, quads, spacing) {
    let sum = 0;
    eachTriangle(vertices, quads, spacing, null, (a, b, c) => { sum += dot(a, cross(b, c)); });
    return sum / 6;
}
// Float64Array [V][3]: per vertex the normalised sum of its triangles' normals, each weighted by the triangle's area
function surfaceNormals(vertices, quads, spacing) {
    const out = new Float64Array(vertices.length);
    eachTriangle(vertices, quads, spacing, null, (a, b, c, at) => {
        const n = cross(sub(b, a), sub(c, a));
        for (const i of at) { out[3 * i] += n[0]; out[3 * i + 1] += n[1]; out[3 * i + 2] += n[2]; }
    });
    for (let i = 0; i < out.length; i += 3) {
        const l = Math.sqrt(out[i] * out[i] + out[i + 1] * out[i + 1] + out[i + 2] * out[i + 2]) || 1;
        out[i] /= l; out[i + 1] /= l; out[i + 2] /= l;
    }
    return out;
}

// ---- writers ----
// binary STL: per triangle its unit normal and three corners as float32
function writeStl(path, vertices, quads, spacing, origin) {
    const count = quads.length / 4 * 2, buf = Buffer.alloc(84 + 50 * count, 0);
    buf.write('vpt surface'.padEnd(80, ' '), 0, 'ascii');
    buf.writeUInt32LE(count, 80);
    let at = 84;
    eachTriangle(vertices, quads, spacing, origin, (a, b, c) => {
        const n = cross(sub(b, a), sub(c, a)), l = Math.sqrt(dot(n, n)) || 1;
        for (const x of [n[0] / l, n[1] / l, n[2] / l].concat(a, b, c)) { buf.writeFloatLE(x, at); at += 4; }
        at += 2;
    });
    fs.writeFileSync(path, buf);
}
// binary little-endian PLY: float32 x y z per vertex, four uint32 indices per face
function writePly(path, vertices, quads, spacing, origin) {
    const p = surfacePositions(vertices, spacing, origin), nv = vertices.length / 3, nf = quads.length / 4;
    const header = Buffer.from(`ply\nformat binary_little_endian 1.0\ncomment vpt surface\nelement vertex ${nv}\nproperty float x\nproperty float y\n` +
        `property float z\nelement face ${nf}\nproperty list uchar uint vertex_indices\nend_header\n`, 'ascii');
    const body = Buffer.alloc(12 * nv + 17 * nf);
    let at = 0;
    for (let i = 0; i < p.length; i++) { body.writeFloatLE(p[i], at); at += 4; }
    for (let f = 0; f < nf; f++) {
        body.writeUInt8(4, at); at += 1;
        for (let k = 0; k < 4; k++) { body.writeUInt32LE(quads[4 * f + k], at); at += 4; }
    }
    fs.writeFileSync(path, Buffer.concat([header, body]));
}
// Wavefront OBJ: `v x y z` per vertex (the shortest decimals that give the double back), `f a b c d` per quad, 1-based
function writeObj(path, vertices, quads, spacing, origin) {
    const p = surfacePositions(vertices, spacing, origin), lines = ['# vpt surface'];
    for (let i = 0; i < p.length; i += 3) { lines.push(`v ${p[i]} ${p[i + 1]} ${p[i + 2]}`); }
    for (let f = 0; f < quads.length; f += 4) { lines.push(`f ${quads[f] + 1} ${quads[f + 1] + 1} ${quads[f + 2] + 1} ${quads[f + 3] + 1}`); }
    fs.writeFileSync(path, lines.join('\n') + '\n');
}

module.exports = { SURFACE_INFO_FIELDS, surfaceTexels, crossingT, checkSurfaceChannel, checkSurfaceLevel, checkSurfaceWindow, surfaceTriangles, surfacePositions,
    surfaceArea, surfaceVolume, surfaceNormals, writeStl, writePly, writeObj };
