'use strict';
// The graph of a set of voxels (a thinned skeleton, or any set) in plain JS: the statement of the contract the device kernels
// (vpt_volume_graph, vpt_skeleton_graph and the vpt_graph_* family; include/vpt.h) are held to, for callers without a device.  Uint8Array /
// Uint16Array texels, x fastest; the numpy statement (vpt_amd/graph.py) says the same and has the wording of the contract.
//
//   K:        the voxels with lo <= code <= hi, or the kept voxels (burn == THIN_KEPT) of a skeleton; everything else is absent
//   class:    0 outside K, otherwise 1 + min(|N26(p) & K|, 3): 1 isolated, 2 end, 3 regular, 4 junction
//   branch:   a 26-component of the voxels of class 1 .. 3;  node: a 26-component of the voxels of class 4; canonical order, ranks from 1
//   record:   voxels, free_ends (class 2), attachments (pairs (branch voxel, adjacent node voxel)), kind, node_lo / node_hi (over those pairs,
//             0 / 0 without one), steps_face / _edge / _corner (pairs inside the branch plus attachment pairs, by the coordinates that
//             differ), tip_lo / tip_hi (linear indices of the voxels with fewer than two neighbours in the branch; the root for a cycle)
//   prune:    one round; a branch goes when wf steps_face + we steps_edge + wc steps_corner <= length and it is a SPUR, or (flag bit 0) a
//             SEGMENT or ISOLATED; node voxels always stay; all spurs of a node go together
// Lengths assume cubic voxels.
const { componentsTexels } = require('./components.js');
const { THIN_KEPT } = require('./skeleton.js');

const GRAPH_KINDS = { ISOLATED: 0, SEGMENT: 1, SPUR: 2, LINK: 3, LOOP: 4, CYCLE: 5 };
const GRAPH_PRUNE_DEBRIS = 1;
const GRAPH_DEFAULT_WEIGHTS = [10, 14, 17];
const GRAPH_INFO_FIELDS = ['kept_voxels', 'node_voxels', 'branches', 'nodes', 'isolated', 'segments', 'spurs', 'links', 'loops', 'cycles',
    'steps_face', 'steps_edge', 'steps_corner', 'attachments'];
const GRAPH_BRANCH_FIELDS = ['voxels', 'free_ends', 'attachments', 'kind', 'node_lo', 'node_hi', 'steps_face', 'steps_edge', 'steps_corner', 'tip_lo', 'tip_hi'];

function largestCode(texels) {
    if (texels instanceof Uint8Array) { return 255; }
    if (texels instanceof Uint16Array) { return 65535; }
    throw new Error('the graph takes Uint8Array or Uint16Array texels');
}
function checkGraphRange(lo, hi, largest) {
    if (!Number.isInteger(lo) || !Number.isInteger(hi) || !(0 <= lo && lo <= hi && hi <= largest)) {
        throw new Error(`graph range [${JSON.stringify(lo)}, ${JSON.stringify(hi)}]: integers with 0 <= lo <= hi <= ${largest}`);
    }
    return [lo, hi];
}
// [length (a BigInt), [wf, we, wc], flags, fill]; length: a non-negative integer number or BigInt below 2^64
function checkPrune(length, weights, flags, fill, largest) {
    if (typeof length === 'number' && Number.isInteger(length)) { length = BigInt(length); }
    if (typeof length !== 'bigint' || length < 0n || length >= (1n << 64n)) { throw new Error('prune length: an integer with 0 <= length < 2^64'); }
    weights = weights !== undefined && weights !== null ? weights : GRAPH_DEFAULT_WEIGHTS;
    if (!Array.isArray(weights) || weights.length !== 3 || !weights.every(w => Number.isInteger(w) && w >= 0 && w <= 65535)) {
        throw new Error('step weights are [face, edge, corner], each an integer in 0 .. 65535, not ' + JSON.stringify(weights));
    }
    flags = flags !== undefined && flags !== null ? flags : 0;
    if (!Number.isInteger(flags) || flags < 0 || (flags & ~GRAPH_PRUNE_DEBRIS)) { throw new Error(`prune flags ${JSON.stringify(flags)}: bit 0 (debris) is taken`); }
    fill = fill !== undefined && fill !== null ? fill : 0;
    if (!Number.isInteger(fill) || fill < 0 || fill > largest) { throw new Error(`fill ${JSON.stringify(fill)}: the largest code is ${largest}`); }
    return [length, weights, flags, fill];
}
function kindOf(voxels, freeEnds, attachments, nodeLo, nodeHi) {
    if (freeEnds === 2) { return GRAPH_KINDS.SEGMENT; }
    if (freeEnds === 1 && attachments === 1) { return GRAPH_KINDS.SPUR; }
    if (attachments === 2) { return nodeLo !== nodeHi ? GRAPH_KINDS.LINK : GRAPH_KINDS.LOOP; }
    return voxels === 1 ? GRAPH_KINDS.ISOLATED : GRAPH_KINDS.CYCLE;
}

// the graph of the voxels i with kept[i] != 0: { classes: Uint8Array, branch_ranks, node_ranks: Uint32Array, branches: [record], nodes:
// [{voxels, degree}], info }.  order (for tests): 'raster' or 'reversed', the order in which the branch voxels are visited.
function graphOf(kept, nx, ny, nz, order) {
    order = order !== undefined ? order : 'raster';
    if (order !== 'raster' && order !== 'reversed') { throw new Error("order is 'raster' or 'reversed', not " + JSON.stringify(order)); }
    const n = nx * ny * nz;
    if (kept.length !== n || n < 1) { throw new Error('the set is [nz][ny][nx]'); }
    if (Math.max(nx, ny, nz) > 4096 || n > 0xFFFFFFFE) { throw new Error('the graph takes at most 4096 voxels an axis and 2^32 - 2 voxels'); }
    const offsets = [];
    for (let c = -1; c <= 1; c++) { for (let b = -1; b <= 1; b++) { for (let a = -1; a <= 1; a++) { if (a || b || c) { offsets.push([a, b, c]); } } } }
    const classes = new Uint8Array(n);
    let keptVoxels = 0, nodeVoxels = 0;
    for (let i = 0; i < n; i++) {
        if (!kept[i]) { continue; }
        const x = i % nx, y = Math.floor(i / nx) % ny, z = Math.floor(i / (nx * ny));
        let deg = 0;
        for (const [a, b, c] of offsets) {
            const xx = x + a, yy = y + b, zz = z + c;
            if (xx >= 0 && xx < nx && yy >= 0 && yy < ny && zz >= 0 && zz < nz && kept[(zz * ny + yy) * nx + xx]) { deg++; }
        }
        classes[i] = 1 + Math.min(deg, 3);
        keptVoxels++;
        if (deg >= 3) { nodeVoxels++; }
    }
    const b = componentsTexels(classes, nx, ny, nz, 1, 3, 26), nd = componentsTexels(classes, nx, ny, nz, 4, 4, 26);
    const branches = b.list.map(() => ({ voxels: 0, free_ends: 0, attachments: 0, kind: 0, node_lo: 0xFFFFFFFF, node_hi: 0, steps_face: 0, steps_edge: 0,
        steps_corner: 0, tip_lo: Infinity, tip_hi: -1 }));
    const nodes = nd.list.map(c => ({ voxels: c[3], degree: 0 }));
    const steps = ['steps_face', 'steps_edge', 'steps_corner'];
    for (let v = 0; v < n; v++) {
        const i = order === 'raster' ? v : n - 1 - v;
        if (classes[i] < 1 || classes[i] > 3) { continue; }
        const x = i % nx, y = Math.floor(i / nx) % ny, z = Math.floor(i / (nx * ny));
        const r = branches[b.ranks[i] - 1];
        let own = 0;
        r.voxels++;
        if (classes[i] === 2) { r.free_ends++; }
        for (const [a, bb, c] of offsets) {
            const xx = x + a, yy = y + bb, zz = z + c;
            if (xx < 0 || xx >= nx || yy < 0 || yy >= ny || zz < 0 || zz >= nz) { continue; }
            const j = (zz * ny + yy) * nx + xx, cls = classes[j], differ = (a !== 0) + (bb !== 0) + (c !== 0);
            if (cls >= 1 && cls <= 3) {
                own++;
                if (j < i) { r[steps[differ - 1]]++; }
            } else if (cls === 4) {
                const rank = nd.ranks[j];
                r.attachments++;
                r[steps[differ - 1]]++;
                r.node_lo = Math.min(r.node_lo, rank); r.node_hi = Math.max(r.node_hi, rank);
                nodes[rank - 1].degree++;
            }
        }
        if (own < 2) { r.tip_lo = Math.min(r.tip_lo, i); r.tip_hi = Math.max(r.tip_hi, i); }
    }
    const info = {};
    for (const f of GRAPH_INFO_FIELDS) { info[f] = 0; }
    info.kept_voxels = keptVoxels; info.node_voxels = nodeVoxels; info.branches = branches.length; info.nodes = nodes.length;
    const counts = ['isolated', 'segments', 'spurs', 'links', 'loops', 'cycles'];
    branches.forEach((r, k) => {
        const c = b.list[k], root = (c[2] * ny + c[1]) * nx + c[0];
        if (r.node_lo === 0xFFFFFFFF) { r.node_lo = 0; }
        if (r.tip_hi < 0) { r.tip_lo = root; r.tip_hi = root; }
        r.kind = kindOf(r.voxels, r.free_ends, r.attachments, r.node_lo, r.node_hi);
        info[counts[r.kind]]++;
        info.steps_face += r.steps_face; info.steps_edge += r.steps_edge; info.steps_corner += r.steps_corner; info.attachments += r.attachments;
    });
    return { classes, branch_ranks: b.ranks, node_ranks: nd.ranks, branches, nodes, info };
}

// the graph of the codes lo .. hi of the texels
function graphTexels(texels, nx, ny, nz, lo, hi, order) {
    checkGraphRange(lo, hi, largestCode(texels));
    if (texels.length !== nx * ny * nz) { throw new Error('texels are [nz][ny][nx]'); }
    const kept = new Uint8Array(texels.length);
    for (let i = 0; i < kept.length; i++) { kept[i] = texels[i] >= lo && texels[i] <= hi ? 1 : 0; }
    return graphOf(kept, nx, ny, nz, order);
}
// the graph of the kept voxels of a skeleton's burn passes
function skeletonGraphTexels(burn, nx, ny, nz, order) {
    const kept = new Uint8Array(burn.length);
    for (let i = 0; i < kept.length; i++) { kept[i] = burn[i] === THIN_KEPT ? 1 : 0; }
    return graphOf(kept, nx, ny, nz, order);
}

// per branch record: does a pruning of `length` drop it?
function dropped(branches, length, weights, flags) {
    const p = checkPrune(length, weights, flags, 0, 0);
    const [wf, we, wc] = p[1].map(BigInt);
    return branches.map((r) => {
        const cost = (wf * BigInt(r.steps_face) + we * BigInt(r.steps_edge) + wc * BigInt(r.steps_corner)) & ((1n << 64n) - 1n);
        const sort = r.kind === GRAPH_KINDS.SPUR || ((p[2] & GRAPH_PRUNE_DEBRIS) !== 0 && (r.kind === GRAPH_KINDS.SEGMENT || r.kind === GRAPH_KINDS.ISOLATED));
        return sort && cost <= p[0];
    });
}
// the codes where the voxel is in the graph's set and its branch is not dropped, `fill` elsewhere, in the texels' type
function pruneTexels(texels, graph, length, weights, flags, fill) {
    const p = checkPrune(length, weights, flags, fill, largestCode(texels));
    if (graph.classes.length !== texels.length) { throw new Error('the graph is of other texels'); }
    const gone = dropped(graph.branches, p[0], p[1], p[2]);
    const out = new texels.constructor(texels.length);
    for (let i = 0; i < out.length; i++) {
        const c = graph.classes[i];
        out[i] = c !== 0 && !(c <= 3 && gone[graph.branch_ranks[i] - 1]) ? texels[i] : p[3];
    }
    return out;
}
// interleaved (code, class) in the texels' type
function classesTexels(texels, graph) {
    largestCode(texels);
    if (graph.classes.length !== texels.length) { throw new Error('the graph is of other texels'); }
    const out = new texels.constructor(2 * texels.length);
    for (let i = 0; i < texels.length; i++) { out[2 * i] = texels[i]; out[2 * i + 1] = graph.classes[i]; }
    return out;
}
// per branch record: (steps_face + sqrt 2 steps_edge + sqrt 3 steps_corner) * spacing
function graphLengths(branches, spacing) {
    spacing = spacing !== undefined ? spacing : 1.0;
    return branches.map(r => (r.steps_face + Math.SQRT2 * r.steps_edge + Math.sqrt(3.0) * r.steps_corner) * spacing);
}

module.exports = { GRAPH_KINDS, GRAPH_PRUNE_DEBRIS, GRAPH_DEFAULT_WEIGHTS, GRAPH_INFO_FIELDS, GRAPH_BRANCH_FIELDS, checkGraphRange, checkPrune, graphKindOf: kindOf,
    graphOf, graphTexels, skeletonGraphTexels, graphDropped: dropped, pruneTexels, classesTexels, graphLengths };
