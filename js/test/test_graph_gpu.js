'use strict';
// node js/test/test_graph_gpu.js OUT — GPU: the Node.js host's graph of a voxel set.  Sparse noise in 70 x 10 x 6 (across a tile of 64 x 8 x 4 and
// the 32-voxel word along every axis), a diagonal line and a Y through the corner (63, 7, 3) -> (64, 8, 4), one voxel and the empty set, uint8
// and uint16, through Volume.graph: info, branch and node records, the ranks of branches and nodes, keepSet on the branches, the class pair,
// prune and profile; and the skeleton of overlapping balls through Skeleton.graph and Volume.centreline(lo, hi, mode, prune): every value
// must equal the plain-JS statement of the contract (js/vpt/graph.js).  The texels of a pruned centreline are written to OUT
// (tests/test_js_gpu_graph.py compares them with the numpy statement).
const fs = require('fs');
const vpt = require('../vpt/index.js');

function equal(a, b, what) {
    if (a.constructor !== b.constructor || a.length !== b.length) { throw new Error(what + ': wrong array'); }
    for (let i = 0; i < a.length; i++) { if (a[i] !== b[i]) { throw new Error(`${what}: element ${i} is ${a[i]}, expected ${b[i]}`); } }
}
function same(got, want, what) {
    if (JSON.stringify(got) !== JSON.stringify(want)) { throw new Error(`${what}: ${JSON.stringify(got).slice(0, 400)}, expected ${JSON.stringify(want).slice(0, 400)}`); }
}
function throws(f, what, pattern) {
    let message = null;
    try { f(); } catch (e) { message = e.message; }
    if (message === null) { throw new Error(what + ' was accepted'); }
    if (pattern && !pattern.test(message)) { throw new Error(what + ': unexpected message ' + message); }
}

let seed = 97531;
const rand = () => { seed = (Math.imul(seed, 1664525) + 1013904223) >>> 0; return seed >>> 8; };
function texelsOf(mask, bits) {
    const M = bits === 8 ? 255 : 65535, half = (M >> 1) + 1, out = new (bits === 8 ? Uint8Array : Uint16Array)(mask.length);
    for (let i = 0; i < mask.length; i++) { out[i] = mask[i] ? half + rand() % half : rand() % half; }
    return out;
}
function noise(n, percent) {
    const mask = new Uint8Array(n);
    for (let i = 0; i < n; i++) { mask[i] = rand() % 100 < percent ? 1 : 0; }
    return mask;
}
function balls(nx, ny, nz, list) {
    const mask = new Uint8Array(nx * ny * nz);
    for (let z = 0, i = 0; z < nz; z++) { for (let y = 0; y < ny; y++) { for (let x = 0; x < nx; x++, i++) {
        for (const [cx, cy, cz, r] of list) { if ((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= r * r) { mask[i] = 1; } }
    } } }
    return mask;
}
const NX = 70, NY = 10, NZ = 6, at = (x, y, z) => (z * NY + y) * NX + x;
function diagonal() {
    const mask = new Uint8Array(NX * NY * NZ);
    for (let k = 0; k < 6; k++) { mask[at(60 + k, 4 + k, k)] = 1; }
    return mask;
}
function cornerWye() {
    const mask = new Uint8Array(NX * NY * NZ);
    mask[at(64, 8, 4)] = 1;
    for (let k = 1; k <= 3; k++) { mask[at(64 - k, 8 - k, 4 - k)] = 1; mask[at(64 + k, 8, 4)] = 1; mask[at(64 - k, 9, 5)] = 1; }
    return mask;
}

// everything a graph on the device says against the statement `want` over the texels `a`
function checkGraph(g, a, dims, want, what) {
    const whole = [0, 0, 0, dims[0], dims[1], dims[2]], M = a instanceof Uint8Array ? 255 : 65535;
    same(g.info, want.info, what + ': info');
    same(g.branchRecords(), want.branches, what + ': branch records');
    same(g.nodeRecords(), want.nodes, what + ': node records');
    equal(g.branches.ranks(), want.branch_ranks, what + ': branch ranks');
    equal(g.nodes.ranks(), want.node_ranks, what + ': node ranks');
    if (want.info.branches > 2) { same(g.branchRecords(1, want.info.branches - 2), want.branches.slice(1, -1), what + ': a window of the branches'); }
    same(g.lengths(0.5), vpt.graphLengths(want.branches, 0.5), what + ': lengths');
    let out = g.classes();
    equal(out.readBlock.apply(out, whole), vpt.classesTexels(a, want), what + ': classes'); out.destroy();
    for (const [length, weights, debris, fill] of [[0, undefined, false, 0], [20, [10, 14, 17], false, 3], [45, undefined, true, M], [(1n << 64n) - 1n, [65535, 65535, 65535], true, 7]]) {
        out = g.prune(length, weights, debris, fill);
        equal(out.readBlock.apply(out, whole), vpt.pruneTexels(a, want, length, weights, debris ? 1 : 0, fill), `${what}: prune ${length}`); out.destroy();
    }
    if (want.info.branches >= 2) {
        out = g.branches.keepSet([2, 1 + (want.info.branches >> 1)], 4);
        const keep = new Set([2, 1 + (want.info.branches >> 1)]);
        equal(out.readBlock.apply(out, whole), a.map((v, i) => (keep.has(want.branch_ranks[i]) ? v : 4)), what + ': keepSet on the branches'); out.destroy();
    }
    const profile = g.profile();
    if (profile.launches !== (want.info.kept_voxels === 0 ? 3 : want.info.branches === 0 ? 4 : 6) || !(profile.ms.links >= 0)) { throw new Error(what + ': profile ' + JSON.stringify(profile)); }
    throws(() => g.prune(-1), 'a negative length', /length/);
    throws(() => g.prune(1, [1, 2, 65536]), 'a weight above 65535', /weights/);
    throws(() => g.prune(1, undefined, false, M + 1), 'fill above M', /fill/);
    throws(() => g.branchRecords(want.info.branches + 1), 'a window beyond the branches', /not within/);
    g.branches.destroy(); g.nodes.destroy();
    g.close();
    throws(() => g.info, 'info of a destroyed graph', /destroyed/);
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
    const CASES = [
        { name: 'noise 10%', dims: [NX, NY, NZ], mask: noise(NX * NY * NZ, 10) },
        { name: 'noise 6%', dims: [NX, NY, NZ], mask: noise(NX * NY * NZ, 6) },
        { name: 'diagonal', dims: [NX, NY, NZ], mask: diagonal() },
        { name: 'corner wye', dims: [NX, NY, NZ], mask: cornerWye() },
        { name: 'voxel', dims: [1, 1, 1], mask: new Uint8Array(1).fill(1) },
        { name: 'nothing', dims: [33, 3, 2], mask: new Uint8Array(198) },
    ];
    const kinds = new Set();
    for (const { name, dims, mask } of CASES) {
        const [nx, ny, nz] = dims;
        for (const bits of [8, 16]) {
            const M = bits === 8 ? 255 : 65535, lo = (M >> 1) + 1, hi = M, a = texelsOf(mask, bits), what = `${name} ${bits} bits`;
            const want = vpt.graphTexels(a, nx, ny, nz, lo, hi);
            want.branches.forEach(r => kinds.add(r.kind));
            if (name === 'corner wye' && !(want.info.nodes === 1 && want.nodes[0].degree === 3 && want.info.spurs === 3)) { throw new Error('the corner wye is no Y: ' + JSON.stringify(want.info)); }
            if (name === 'diagonal' && !(want.info.segments === 1 && want.branches[0].steps_corner === 5)) { throw new Error('the diagonal is no line'); }
            const v = await uploadTo(a, bits, dims);
            checkGraph(v.graph(lo, hi), a, dims, want, what);
            throws(() => v.graph(hi, lo), 'lo above hi', /graph range/);
            throws(() => v.graph(lo, M + 1), 'hi above M', /graph range/);
            equal(v.readBlock(0, 0, 0, nx, ny, nz), a, 'the source afterwards');
            v.destroy();
        }
    }
    if (kinds.size !== 6) { throw new Error('the cases do not hold every kind: ' + JSON.stringify([...kinds])); }
    // a skeleton's graph, and the pruned centreline
    const BX = 70, BY = 19, BZ = 11, solid = texelsOf(balls(BX, BY, BZ, [[8, 9, 5, 6], [20, 9, 5, 8], [36, 6, 4, 5], [50, 12, 6, 7], [64, 9, 5, 5]]), 8);
    const v = await uploadTo(solid, 8, [BX, BY, BZ]);
    const burn = vpt.skeletonBurnTexels(solid, BX, BY, BZ, 128, 255, 'ends').burn, want = vpt.skeletonGraphTexels(burn, BX, BY, BZ);
    if (!(want.info.kept_voxels > 10 && want.info.branches > 0)) { throw new Error('degenerate skeleton: ' + JSON.stringify(want.info)); }
    const k = v.skeleton(128, 255, 'ends');
    checkGraph(k.graph(), solid, [BX, BY, BZ], want, 'the skeleton of the balls');
    k.destroy();
    let out = v.centreline(128, 255, 'ends');
    equal(out.readBlock(0, 0, 0, BX, BY, BZ), vpt.skeletonTexels(solid, BX, BY, BZ, 128, 255, 'ends'), 'centreline without prune'); out.destroy();
    throws(() => v.centreline(0, 255, 'ends', 20), 'a range that covers every code', /covers every code/);
    out = v.centreline(128, 255, 'ends', 30, 2);
    const pruned = out.readBlock(0, 0, 0, BX, BY, BZ);
    out.destroy(); v.destroy();
    ctx.destroy();
    fs.writeFileSync(outPath, Buffer.concat([Buffer.from(solid.buffer), Buffer.from(pruned.buffer)]));
    console.log('js graph gpu ok');
}
main().catch(e => { console.error(e); process.exit(1); });
