'use strict';
// node js/test/test_graph_host.js [BITS LO HI (TEXELS NX NY NZ)...] — no device: the plain-JS statement of the graph contract (js/vpt/graph.js):
// shapes with known answers (a line, a Y, a ring, a block), the contract's identities and the order of the visits on random
// sets, pruning, refusals.  With arguments, the graph of the codes LO .. HI of every file TEXELS (BITS bits a voxel), two prunings, the
// class pair and the lengths are printed as one JSON line (tests/test_graph_host.py compares it with the numpy statement).
const fs = require('fs');
const g = require('../vpt/graph.js');
const { componentsTexels } = require('../vpt/components.js');
const K = g.GRAPH_KINDS;

function throws(f, what, pattern) {
    let message = null;
    try { f(); } catch (e) { message = e.message; }
    if (message === null) { throw new Error(what + ' was accepted'); }
    if (pattern && !pattern.test(message)) { throw new Error(what + ': unexpected message ' + message); }
}
function check(cond, what) { if (!cond) { throw new Error(what); } }
const row = r => g.GRAPH_BRANCH_FIELDS.map(f => r[f]);

// ---- shapes
{
    const n = 20, line = new Uint8Array(n * n * n);
    for (let x = 3; x < 17; x++) { line[(7 * n + 11) * n + x] = 9; }
    const found = g.graphTexels(line, n, n, n, 9, 9);
    check(found.info.branches === 1 && found.info.nodes === 0 && found.info.segments === 1, 'a line: ' + JSON.stringify(found.info));
    check(JSON.stringify(row(found.branches[0])) === JSON.stringify([14, 2, 0, K.SEGMENT, 0, 0, 13, 0, 0, (7 * n + 11) * n + 3, (7 * n + 11) * n + 16]), 'a line: its record');
    check(g.graphLengths(found.branches, 0.5)[0] === 6.5, 'a line: its length');
}
{
    // a Y in a plane: the node (4, 4), two arms down its diagonals and one straight up; the first voxels of the arms are not adjacent to one another
    const nx = 9, ny = 9, a = new Uint8Array(nx * ny);
    a[4 * nx + 4] = 1;
    for (let k = 1; k <= 3; k++) { a[(4 - k) * nx + 4 - k] = 1; a[(4 - k) * nx + 4 + k] = 1; a[(4 + k) * nx + 4] = 1; }
    const found = g.graphTexels(a, nx, ny, 1, 1, 1);
    check(found.info.nodes === 1 && found.nodes[0].degree === 3 && found.nodes[0].voxels === 1 && found.info.spurs === 3 && found.info.branches === 3, 'a Y: ' + JSON.stringify(found.info));
    check(found.branches.every(r => r.voxels === 3 && r.steps_face + r.steps_edge === 3 && r.free_ends === 1 && r.attachments === 1 && r.node_lo === 1 && r.node_hi === 1), 'a Y: its arms');
    check(found.info.steps_face === 3 && found.info.steps_edge === 6 && found.info.steps_corner === 0, 'a Y: its steps');
    const pruned = g.pruneTexels(a, found, 42);
    check(pruned.reduce((s, v) => s + v, 0) === 1 && pruned[4 * nx + 4] === 1, 'a Y within the length is reduced to its node');
    check(g.pruneTexels(a, found, 41).reduce((s, v) => s + v, 0) === 7, 'only the straight arm is within 41');
    check(g.pruneTexels(a, found, 29).reduce((s, v) => s + v, 0) === 10, 'a Y beyond the length stays');
}
{
    // a diamond ring: every voxel has its two diagonal neighbours
    const nx = 7, ny = 7, a = new Uint8Array(nx * ny);
    for (let y = 0; y < ny; y++) { for (let x = 0; x < nx; x++) { if (Math.abs(x - 3) + Math.abs(y - 3) === 3) { a[y * nx + x] = 1; } } }
    const found = g.graphTexels(a, nx, ny, 1, 1, 1);
    check(found.info.cycles === 1 && found.info.branches === 1 && found.info.nodes === 0, 'a ring: ' + JSON.stringify(found.info));
    const r = found.branches[0];
    check(r.voxels === 12 && r.steps_edge === 12 && r.steps_face === 0 && r.tip_lo === 3 && r.tip_hi === 3 && r.kind === K.CYCLE, 'a ring: its record');
}
{
    const a = new Uint8Array(5 * 5 * 3).fill(1);
    const found = g.graphTexels(a, 5, 5, 3, 1, 1);
    check(found.info.branches === 0 && found.info.nodes === 1 && found.nodes[0].voxels === 75 && found.nodes[0].degree === 0, 'a block is one node');
    const none = g.graphTexels(a, 5, 5, 3, 2, 9);
    check(none.info.kept_voxels === 0 && none.branches.length === 0 && none.nodes.length === 0, 'the empty set');
    const one = g.graphTexels(new Uint16Array([700]), 1, 1, 1, 700, 700);
    check(one.info.isolated === 1 && one.branches[0].kind === K.ISOLATED && one.branches[0].tip_lo === 0 && one.branches[0].tip_hi === 0, 'a single voxel');
}

// ---- random sets: the identities, the order of the visits, pruning keeps the components
let seed = 2468;
const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
const kinds = new Set();
for (const [nx, ny, nz, per] of [[12, 11, 9, 10], [70, 10, 6, 10], [70, 10, 6, 7], [13, 5, 1, 3]]) {
    const a = new Uint8Array(nx * ny * nz);
    for (let i = 0; i < a.length; i++) { a[i] = rand() % 100 < per ? 100 + rand() % 100 : rand() % 100; }
    const what = `${nx}x${ny}x${nz} ${per}%`;
    const one = g.graphTexels(a, nx, ny, nz, 100, 255), two = g.graphTexels(a, nx, ny, nz, 100, 255, 'reversed');
    check(JSON.stringify([one.info, one.branches, one.nodes]) === JSON.stringify([two.info, two.branches, two.nodes]), what + ': reversed order');
    let degrees = 0, attachments = 0;
    one.nodes.forEach((nd) => { degrees += nd.degree; });
    one.branches.forEach((r, k) => {
        const steps = r.steps_face + r.steps_edge + r.steps_corner;
        kinds.add(r.kind);
        attachments += r.attachments;
        check(r.free_ends + r.attachments === 0 || r.free_ends + r.attachments === 2, `${what}: branch ${k}: free ends + attachments`);
        check(steps === (r.kind === K.CYCLE ? r.voxels : r.kind === K.ISOLATED ? 0 : r.voxels - 1 + r.attachments), `${what}: branch ${k}: steps`);
        check(r.kind === g.graphKindOf(r.voxels, r.free_ends, r.attachments, r.node_lo, r.node_hi), `${what}: branch ${k}: kind`);
    });
    check(degrees === attachments && attachments === one.info.attachments, what + ': degrees and attachments');
    const before = componentsTexels(one.classes, nx, ny, nz, 1, 4, 26).list.length;
    for (const length of [0, 20, 45, 2 ** 40, (1n << 64n) - 1n]) {
        const out = g.pruneTexels(a, one, length, undefined, 0, 3), stays = out.map(v => (v !== 3 ? 1 : 0));
        check(componentsTexels(stays, nx, ny, nz, 1, 1, 26).list.length === before, `${what}: prune ${length} keeps the components`);
        if (length === 0) { check(stays.every((v, i) => v === (one.classes[i] ? 1 : 0)), what + ': prune 0 drops nothing'); }
    }
    const pair = g.classesTexels(a, one);
    check(pair.length === 2 * a.length && pair.every((v, i) => v === (i % 2 ? one.classes[i >> 1] : a[i >> 1])), what + ': the class pair');
}
check(kinds.size === 6, 'the random sets hold every kind: ' + JSON.stringify([...kinds]));

// ---- refusals
const a = new Uint8Array(24).fill(9), found = g.graphTexels(a, 4, 3, 2, 9, 9);
throws(() => g.graphTexels(a, 4, 3, 2, 3, 2), 'lo above hi', /graph range/);
throws(() => g.graphTexels(a, 4, 3, 2, 0, 256), 'hi above M', /graph range/);
throws(() => g.graphTexels(a, 4, 3, 2, 1.5, 2), 'a fractional lo', /graph range/);
throws(() => g.graphTexels(a, 4, 3, 3, 1, 2), 'a wrong size', /texels/);
throws(() => g.graphTexels(new Float32Array(24), 4, 3, 2, 1, 2), 'floats', /Uint8Array/);
throws(() => g.graphTexels(a, 4, 3, 2, 1, 2, 'random'), 'an unknown order', /order/);
throws(() => g.pruneTexels(a, found, -1), 'a negative length', /length/);
throws(() => g.pruneTexels(a, found, 1.5), 'a fractional length', /length/);
throws(() => g.pruneTexels(a, found, 1n << 64n), 'a length of 2^64', /length/);
throws(() => g.pruneTexels(a, found, 1, [1, 2]), 'two weights', /weights/);
throws(() => g.pruneTexels(a, found, 1, [1, 2, 65536]), 'a weight above 65535', /weights/);
throws(() => g.pruneTexels(a, found, 1, undefined, 2), 'an unknown flag', /flags/);
throws(() => g.pruneTexels(a, found, 1, undefined, 0, 256), 'fill above M', /fill/);
throws(() => g.pruneTexels(new Uint8Array(5), found, 1), 'other texels', /other texels/);

if (process.argv.length > 2) {
    const [bits, lo, hi] = process.argv.slice(2, 5).map(Number);
    const out = [];
    for (let k = 5; k + 3 < process.argv.length; k += 4) {
        const [nx, ny, nz] = process.argv.slice(k + 1, k + 4).map(Number);
        const bytes = fs.readFileSync(process.argv[k]);
        const texels = bits === 8 ? new Uint8Array(bytes.buffer, bytes.byteOffset, nx * ny * nz) : new Uint16Array(new Uint8Array(bytes).buffer, 0, nx * ny * nz);
        const graph = g.graphTexels(texels, nx, ny, nz, lo, hi);
        out.push({ info: graph.info, classes: Array.from(graph.classes), branch_ranks: Array.from(graph.branch_ranks), node_ranks: Array.from(graph.node_ranks),
            branches: graph.branches.map(row), nodes: graph.nodes.map(nd => [nd.voxels, nd.degree]),
            prune: Array.from(g.pruneTexels(texels, graph, 20, undefined, 0, 3)), debris: Array.from(g.pruneTexels(texels, graph, 30, [10, 14, 17], g.GRAPH_PRUNE_DEBRIS, 1)),
            pair: Array.from(g.classesTexels(texels, graph)), lengths: g.graphLengths(graph.branches, 0.5) });
    }
    console.log(JSON.stringify(out));
}
console.log('js graph host ok');
