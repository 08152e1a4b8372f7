'use strict';
// Local thickness, the largest inscribed ball, in plain JS: the contract of include/vpt.h ("local thickness") restated for hosts without a
// device, the twin of vpt_amd.thickness_squared_texels (vpt_amd/distance.py).
// d2: a Uint32Array of [nz][ny][nx] squared distances (distanceSquaredTexels).  A voxel c with d2(c) > 0 is a centre, its ball the voxels v
// of the array with |v - c|^2 < d2(c) (open: it holds no seed; what sticks out of the array does not exist), and T2(v) is the largest
// d2(c) among the balls that hold v, 0 when none does.  NONE everywhere (no seed) gives NONE everywhere.
// Stated as it reads: every centre paints its ball with its d2, a voxel keeps the largest.  (About R^3 voxels a centre: a statement, not
// the way to compute it; the device gathers per tile, DESIGN.md "Local thickness".)
const { distanceSquaredTexels, withinTexels, channelTexels, checkRadius, DISTANCE_NONE } = require('./distance.js');

function thicknessSquaredTexels(d2, nx, ny, nz) {
    const n = nx * ny * nz;
    if (!(d2 instanceof Uint32Array) || d2.length !== n || n < 1) { throw new Error('squared distances are a Uint32Array of [nz][ny][nx]'); }
    const out = new Uint32Array(n);
    let none = 0;
    for (let i = 0; i < n; i++) { if (d2[i] === DISTANCE_NONE) { none++; } }
    if (none === n) { return out.fill(DISTANCE_NONE); }
    if (none) { throw new Error('squared distances are finite everywhere, or NONE everywhere'); }
    for (let cz = 0, c = 0; cz < nz; cz++) {
        for (let cy = 0; cy < ny; cy++) {
            for (let cx = 0; cx < nx; cx++, c++) {
                const D = d2[c];
                if (D === 0) { continue; }
                const r = Math.ceil(Math.sqrt(D));                           // no offset of the ball reaches r on an axis
                for (let z = Math.max(cz - r, 0); z <= Math.min(cz + r, nz - 1); z++) {
                    for (let y = Math.max(cy - r, 0); y <= Math.min(cy + r, ny - 1); y++) {
                        const left = D - (z - cz) * (z - cz) - (y - cy) * (y - cy);
                        if (left <= 0) { continue; }
                        const row = (z * ny + y) * nx;
                        for (let x = Math.max(cx - r, 0); x <= Math.min(cx + r, nx - 1); x++) {
                            if ((x - cx) * (x - cx) < left && out[row + x] < D) { out[row + x] = D; }
                        }
                    }
                }
            }
        }
    }
    return out;
}

// interleaved (code, min(isqrt(steps^2 T2), M)) of the codes lo .. hi (seeds 'rest') or of their complement (seeds 'range'); steps 2: the
// diameter in voxels: what Volume.thickness holds
function thicknessTexels(texels, nx, ny, nz, lo, hi, steps, seeds) {
    const d2 = distanceSquaredTexels(texels, nx, ny, nz, lo, hi, seeds !== undefined ? seeds : 'rest');
    return channelTexels(texels, thicknessSquaredTexels(d2, nx, ny, nz), steps !== undefined ? steps : 2);
}

// the codes lo .. hi opened by the Euclidean ball of `radius` voxels, `fill` elsewhere: what Volume.openBall holds
function openBallTexels(texels, nx, ny, nz, lo, hi, radius, fill) {
    const r2 = checkRadius(radius);
    const d2 = distanceSquaredTexels(texels, nx, ny, nz, lo, hi, 'rest');
    return withinTexels(texels, thicknessSquaredTexels(d2, nx, ny, nz), r2 + 1, null, fill !== undefined ? fill : 0);
}

module.exports = { thicknessSquaredTexels, thicknessTexels, openBallTexels };
