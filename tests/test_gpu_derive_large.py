"""GPU: reconstruction and the geodesic operations, the watershed, local thickness, the skeleton, its graph and the surface on volumes of more than
2^31 (tier A) and more than 2^32 (tier B) voxels, where a linear index, a byte offset, a tile number or a counter kept in 32 bits goes wrong.

The method is that of tests/test_gpu_large_volumes.py: slabs of whole planes at z = 0, round the plane of linear voxel 2^31 (and 2^30 where
a four-byte value per voxel passes byte 2^32) and ending at z = nz - 1, background 0 elsewhere; every result is held byte for byte, no
tolerance appears.  The numpy statements of these operations iterate to a fixed point, recurse over level sets or visit voxels one by one,
so the slabs hold a few small solids with noise inside (large_volumes.solids) and the expected values come from the statement on a crop
round each solid; tests/test_large_volumes_host.py shows per operation, on a shape small enough to hold whole, that the crops give the
statement on the whole volume.  The surface of noise slabs comes from the statement on the twin.

Each test states its peak device memory as the sum of what it allocates (GiB; V: a volume = linear storage + bricks + boundary atlas,
large_volumes.volume_bytes; F: a voxel field = the texels' snapshot + one uint32 per voxel, large_volumes.field_bytes; n: the voxels) and
skips, with both figures, when less is free.  Nothing else may skip."""
import numpy as np
import pytest

import vpt_amd
from vpt_amd.surface import surface_texels

from large_volumes import (TIER_A, TIER_B, Layout, voxels, volume_bytes, field_bytes, sparse_volume, planes, differences, solids, on_crops,
                           watershed_on_crops, skeleton_on_crops, graph_on_crops, surface_on_crops, shift_twin_vertices, thickness_tiles)
from graph_cases import dropped, prune_texels
from test_gpu_large_volumes import DTYPE, require, tier, hold, background, refused

pytestmark = pytest.mark.gpu

THICK = 8                                                         # planes a slab of solids


def tiles_of(shape, tx, ty, tz):
    nx, ny, nz = shape
    return ((nx + tx - 1) // tx) * ((ny + ty - 1) // ty) * ((nz + tz - 1) // tz)


def solid_layout(shape, gap=2, four_bytes=False):
    """slabs of THICK planes on even planes; `four_bytes`: also one round voxel 2^30, where a uint32 per voxel passes byte 2^32"""
    return Layout(shape, THICK, gap, marks=(1 << 30, 1 << 31) if four_bytes else (1 << 31,), even=True)


def hold_field(read, blocks, lay, what, distinct=8):
    """the values of a voxel field in every slab equal `blocks`, as whole planes and as a box that is not; the planes between are 0"""
    nx, ny, _ = lay.shape
    for z0, want in zip(lay.starts, blocks):
        assert len(np.unique(want)) >= distinct, "degenerate input: %d distinct values expected in planes %d .. (%s)" % (len(np.unique(want)), z0, what)
        differences(read(0, 0, z0, nx, ny, lay.thick), want, "%s, planes %d .. %d" % (what, z0, z0 + lay.thick - 1))
        rows = np.nonzero(want.any(axis=(0, 2)))[0]
        x0, y0, w, h = 5, min(max(int(rows[len(rows) // 2]) - 3, 1), ny - 8), nx - 9, 7
        box = np.ascontiguousarray(want[:, y0:y0 + h, x0:x0 + w])
        assert box.any()
        differences(read(x0, y0, z0, w, h, lay.thick), box, "a box of %s, planes %d .. %d" % (what, z0, z0 + lay.thick - 1))
    for z in lay.between():
        assert not read(0, 0, z, nx, ny, 1).any(), "%s: plane %d between the slabs is not 0" % (what, z)


# ---- reconstruction and the geodesic operations -----------------------------------------------------------------------------------
@pytest.mark.timeout(180)
@pytest.mark.parametrize("kind,bits,connectivity", [('aligned', 8, 6), ('odd', 16, 26)])
def test_reconstruct_by_dilation_of_more_than_2_31_voxels(gpu_ctx, kind, bits, connectivity):
    """Tier A, marker and mask two sparse volumes with the same solids: the marker a tenth of another noise's voxels, so it rises along
    paths through the solids.  Peak: marker V + mask V + result V + the tile flags (2 x 4 bytes a tile of 64 x 8 x 4) = 3 x 10.6 = 31.9 GiB
    (R8), 3 x 21.4 = 64.2 GiB (R16)."""
    shape = TIER_A[kind]
    tier(shape, 1 << 31, 0xFFFFFFFE)
    require(3 * volume_bytes(shape, bits // 8) + 8 * tiles_of(shape, 64, 8, 4))
    dtype = DTYPE[bits]
    lay = solid_layout(shape)
    mask, crops = solids(lay, dtype, 201)
    other, _ = solids(lay, dtype, 211)
    marker = [np.where(np.random.default_rng(221 + i).random(b.shape) < 0.1, b, 0).astype(dtype) for i, b in enumerate(other)]
    pair = [np.ascontiguousarray(np.stack([a, b], axis=-1)) for a, b in zip(marker, mask)]
    want = on_crops(lay, pair, crops, lambda a: vpt_amd.reconstruct_texels(a, a, 'dilation', connectivity, 0, 1))
    assert sum(int((w != np.minimum(a, b)).sum()) for w, a, b in zip(want, marker, mask)) >= 100      # voxels that rise
    m, k = sparse_volume(gpu_ctx, lay, marker), None
    try:
        k = sparse_volume(gpu_ctx, lay, mask)
        out = m.reconstruct(k, 'dilation', connectivity)
    finally:
        m.destroy()
        if k is not None:
            k.destroy()
    try:
        hold(out, lay.twin(want), lay.windows(), "reconstruct by dilation R%d %s c%d" % (bits, kind, connectivity))
        background(out, lay.between(), 0, "reconstruct")
    finally:
        out.destroy()


@pytest.mark.timeout(300)
def test_fill_holes_of_more_than_2_31_voxels(gpu_ctx, capsys):
    """Tier A, R8, the erosion side: the result starts at 255 in all 2.7 G voxels behind the faces and the whole background falls to 0
    through the tile kernel's relaunches; the shell's cavity stays filled to its rim.  Peak: source V + result V + the tile flags = 21.2
    GiB.  One parametrisation: the device time is that of the background, not of the solids (printed: milliseconds and launches)."""
    shape = TIER_A['odd']
    tier(shape, 1 << 31, 0xFFFFFFFE)
    require(2 * volume_bytes(shape, 1) + 8 * tiles_of(shape, 64, 8, 4))
    lay = solid_layout(shape)
    blocks, crops = solids(lay, np.uint8, 231)
    want = on_crops(lay, blocks, crops, lambda a: vpt_amd.geodesic_texels(a, 'fill_holes', 0, 6))
    assert int((want[0] > blocks[0]).sum()) >= 27                 # the cavity
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        out, profile = src.fill_holes_timed(6)
    finally:
        src.destroy()
    with capsys.disabled():
        print("\nfill_holes of %d voxels: %.0f ms, %d launches, %d tile runs" % (voxels(shape), profile['ms'], profile['launches'], profile['tile_runs']))
    try:
        hold(out, lay.twin(want), lay.windows(), "fill_holes")
        background(out, lay.between() + [1 + THICK, shape[2] - THICK - 2], 0, "fill_holes")
    finally:
        out.destroy()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("kind,bits,channels,connectivity", [('aligned', 16, 1, 26), ('odd', 8, 2, 6)])
def test_dome_of_more_than_2_31_voxels(gpu_ctx, kind, bits, channels, connectivity):
    """Tier A: hmax by dilation, then the epilogue src - hmax (FIN_SUB) over all voxels.  The RG8 source is read through stride 2 at
    channel 1: the element index 2 i + 1 passes 2^32 at voxel 2^31.  Peak: source V (R16 21.4; RG8 21.2) + result V (21.4; 10.6) + the
    tile flags = 42.8 GiB (R16), 31.8 GiB (RG8)."""
    shape = TIER_A[kind]
    tier(shape, 1 << 31, 0xFFFFFFFE)
    require(volume_bytes(shape, bits // 8, channels) + volume_bytes(shape, bits // 8) + 8 * tiles_of(shape, 64, 8, 4))
    dtype, M = DTYPE[bits], (1 << bits) - 1
    channel = channels - 1
    lay = solid_layout(shape)
    blocks, crops = solids(lay, dtype, 241, channels)
    want = on_crops(lay, blocks, crops, lambda a: vpt_amd.geodesic_texels(a, 'dome', M // 8, connectivity, channel))
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        out = src.dome(M // 8, connectivity, channel)
    finally:
        src.destroy()
    try:
        hold(out, lay.twin(want), lay.windows(), "dome R%d x %d %s" % (bits, channels, kind))
        background(out, lay.between(), 0, "dome")
    finally:
        out.destroy()


# ---- the watershed ---------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(180)
@pytest.mark.parametrize("kind,bits,channels,polarity,connectivity", [('aligned', 16, 1, 'minima', 6), ('odd', 8, 2, 'maxima', 26)])
def test_watershed_of_more_than_2_31_voxels(gpu_ctx, kind, bits, channels, polarity, connectivity):
    """Tier A, the domain 1 .. M: the solids, whose noise gives hundreds of basins.  The RG8 relief is read through stride 2 at channel 1
    (the element index 2 i + 1 passes 2^32 at voxel 2^31) and the handle holds that channel.  Peak while flooding: relief V + handle F +
    directions n + plateau distances 4 n + the count array 4 n = 21.4 + 15.0 + 22.5 = 58.9 GiB (R16), 21.2 + 12.5 + 22.5 = 56.2 GiB (RG8);
    then handle + label volume (RG): 15.0 + 42.7 = 57.7 GiB (R16), 12.5 + 21.2 = 33.7 GiB (R8)."""
    shape = TIER_A[kind]
    n = tier(shape, 1 << 31, 0xFFFFFFFE)
    nx, ny, nz = shape
    item, channel = bits // 8, channels - 1
    require(max(volume_bytes(shape, item, channels) + field_bytes(shape, item) + 9 * n + 8 * tiles_of(shape, 64, 8, 4),
                field_bytes(shape, item) + volume_bytes(shape, item, 2)))
    dtype, M = DTYPE[bits], (1 << bits) - 1
    lay = solid_layout(shape, four_bytes=True)
    blocks, crops = solids(lay, dtype, 251, channels)
    codes = [np.ascontiguousarray(b[..., channel]) if channels == 2 else b for b in blocks]
    ranks, listed = watershed_on_crops(lay, blocks, crops, 1, M, polarity, connectivity, channel)
    far = [c for c in listed if (c[2] * ny + c[1]) * nx + c[0] > (1 << 31)]
    assert len(listed) >= 64 and len(far) >= 1 and len({c[2] for c in listed}) >= 4 and len({c[3] for c in listed}) >= 4
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        found = src.watershed(1, M, polarity, connectivity, channel=channel)
    finally:
        src.destroy()
    try:
        inside = int(sum((b >= 1).sum() for b in codes))
        assert found.info == {'listed': len(listed), 'dropped': 0, 'foreground_voxels': inside, 'listed_voxels': inside}
        assert found.list() == listed
        hold_field(found.ranks, ranks, lay, "ranks")
        twin = lay.twin(codes)
        twin_ranks = lay.twin(ranks)
        k = len(listed) // 2
        kept = found.keep(1, k)
        try:
            hold(kept, vpt_amd.keep_texels(twin, twin_ranks, 1, k), lay.windows(), "keep(1, %d)" % k)
            background(kept, lay.between(), 0, "keep")
        finally:
            kept.destroy()
        pair = found.label()
        try:
            hold(pair, vpt_amd.label_texels(twin, twin_ranks), lay.windows(), "label")
            background(pair, lay.between(), 0, "label")
        finally:
            pair.destroy()
    finally:
        found.destroy()


# ---- what 32-bit labels refuse ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_reconstruct_and_watershed_refuse_more_than_2_32_voxels(gpu_ctx):
    """Tier B: reconstruction keeps tile-local 32-bit voxel numbers, the watershed 32-bit labels and the graph 32-bit labels, list entries and
    counts; all say so.  Peak: one zero-filled R8 volume, 19.9 GiB."""
    shape = TIER_B['odd']
    n = tier(shape, 1 << 32)
    nx, ny, _ = shape
    require(volume_bytes(shape, 1))
    lay = Layout(shape, 1, 1)
    src = sparse_volume(gpu_ctx, lay, [np.zeros((1, ny, nx), np.uint8)] * 3)
    try:
        refused(lambda: src.reconstruct(src), "reconstruct", str(n), "2^32 - 2")
        refused(lambda: src.reconstruct(src, 'erosion', 26), "reconstruct", "2^32 - 2")
        for op in ('fill_holes', 'hmax', 'minima'):
            refused(lambda: src.geodesic(op, 1 if op == 'hmax' else 0), "geodesic", str(n), "2^32 - 2")
        refused(lambda: src.watershed(1, 255), "watershed", str(n), "2^32 - 2")
        refused(lambda: src.watershed(1, 255, 'maxima', 26), "watershed", "2^32 - 2")
        # the graph's labels, list entries and counts are 32-bit too (Skeleton.graph: test_skeleton_in_large_volumes, which has a skeleton)
        refused(lambda: src.graph(1, 255), "graph", str(n), "2^32 - 2")
        refused(lambda: src.graph(0, 0), "graph", "2^32 - 2")
    finally:
        src.destroy()


# ---- local thickness -------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(240)
@pytest.mark.parametrize("tier_name,kind,bits", [('B', 'odd', 8), ('A', 'aligned', 16)])
def test_thickness_in_large_volumes(gpu_ctx, tier_name, kind, bits):
    """distance(1, M, 'rest') -> thickness(): T2 of the solids; the tile count checks k_th_tile_max's numbering of the 17 M (tier B) tiles
    of 8 x 8 x 4.  The distance handle is destroyed before the emitters run.  Peak, tier B R8: source V 19.9 + the larger of (distance: F
    20.1 + 2 x 4 n = 52.3), (thickness: 2 F + 4 bytes a tile = 40.3) and (channel: F + RG8 V 39.8 = 59.9) = 79.8 GiB; tier A R16: 21.4 +
    max(15.0 + 20.0, 30.1, 15.0 + 42.7) = 79.1 GiB."""
    shape = (TIER_B if tier_name == 'B' else TIER_A)[kind]
    n = tier(shape, 1 << 32) if tier_name == 'B' else tier(shape, 1 << 31, 1 << 32)
    item = bits // 8
    F = field_bytes(shape, item)
    require(volume_bytes(shape, item) + max(F + 8 * n, 2 * F + 4 * tiles_of(shape, 8, 8, 4), F + volume_bytes(shape, item, 2)))
    dtype, M = DTYPE[bits], (1 << bits) - 1
    lay = solid_layout(shape, 4, four_bytes=tier_name == 'A')
    blocks, crops = solids(lay, dtype, 261)
    d2 = on_crops(lay, blocks, crops, lambda a: vpt_amd.distance_squared_texels(a, 1, M, 'rest'))
    t2 = on_crops(lay, blocks, crops, lambda a: vpt_amd.thickness_squared_texels(vpt_amd.distance_squared_texels(a, 1, M, 'rest')))
    largest = max(int(d.max()) for d in d2)
    assert largest < (lay.gap + 1) ** 2 and largest == max(int(t.max()) for t in t2)
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        found = src.distance(1, M, 'rest')
        try:
            hold_field(found.squared, d2, lay, "squared distances", distinct=8)
            t, profile = found.thickness_timed()
        finally:
            found.destroy()
        try:
            assert profile['tiles'] == thickness_tiles(lay, d2)
            assert t.info['largest'] == largest
            hold_field(t.squared, t2, lay, "T2", distinct=8)
        finally:
            t.destroy()
        out = src.thickness(1, M, 3)
    finally:
        src.destroy()
    try:
        want = on_crops(lay, blocks, crops, lambda a: vpt_amd.thickness_texels(a, 1, M, 3))
        hold(out, lay.twin(want), lay.windows(), "thickness(1, %d, 3)" % M)
        background(out, lay.between(), 0, "thickness")
    finally:
        out.destroy()


# ---- the skeleton ----------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(240)
@pytest.mark.parametrize("tier_name,kind,bits,mode", [('B', 'aligned', 8, 'ends'), ('A', 'odd', 16, 'kernel')])
def test_skeleton_in_large_volumes(gpu_ctx, tier_name, kind, bits, mode):
    """The slabs begin on even planes and a crop on an even voxel: the eight subfields of a pass are the parities of (x, y, z).  Peak
    while thinning: source V + handle F + three bit planes (3 x 4 bytes x 2 words a tile of 64 along x x ny x nz) + the tile flags (4 x 4
    bytes a tile of 64 x 8 x 4) = 19.9 + 20.0 + 1.6 = 41.5 GiB (tier B R8), 21.4 + 15.0 + 1.0 = 37.4 GiB (tier A R16); then handle + a
    volume like the source, less."""
    shape = (TIER_B if tier_name == 'B' else TIER_A)[kind]
    tier(shape, 1 << 32) if tier_name == 'B' else tier(shape, 1 << 31, 1 << 32)
    nx, ny, nz = shape
    item = bits // 8
    require(volume_bytes(shape, item) + field_bytes(shape, item) + 3 * 4 * 2 * ((nx + 63) // 64) * ny * nz + 16 * tiles_of(shape, 64, 8, 4))
    dtype, M = DTYPE[bits], (1 << bits) - 1
    lay = solid_layout(shape, four_bytes=tier_name == 'A')
    blocks, crops = solids(lay, dtype, 271)
    burn, info = skeleton_on_crops(lay, blocks, crops, 1, M, mode)
    assert info['passes'] >= 3 and info['converged'] == 1 and info['kept_voxels'] >= len(crops)
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        found = src.skeleton(1, M, mode)
    finally:
        src.destroy()
    try:
        assert found.info == info
        if tier_name == 'B':                                      # more than 2^32 - 2 voxels: the graph of this skeleton is refused
            refused(found.graph, "graph", str(voxels(shape)), "2^32 - 2")
        hold_field(found.burn, burn, lay, "burn passes", distinct=4)
        peeled = found.within(2, None)
        try:
            hold(peeled, lay.twin([vpt_amd.burn_within_texels(b, k, 2, None) for b, k in zip(blocks, burn)]), lay.windows(), "within(2)")
            background(peeled, lay.between(), 0, "within")
        finally:
            peeled.destroy()
        kept = found.volume()
        try:
            for z0, b, k in zip(lay.starts, blocks, burn):
                want = vpt_amd.burn_within_texels(b, k, found.KEPT, found.KEPT)
                assert want.any()
                differences(planes(kept, z0, z0 + THICK), want, "the skeleton, planes %d .. %d" % (z0, z0 + THICK - 1))
            background(kept, lay.between(), 0, "the skeleton")
        finally:
            kept.destroy()
    finally:
        found.destroy()


# ---- the graph -------------------------------------------------------------------------------------------------------------------
def hold_graph(g, want, fields, blocks, lay, prune, what):
    """a graph on the device against the crops' graphs put together: info and every record; the ranks as voxel fields; the class pair and
    one pruning in the slabs' planes; background between the slabs"""
    twin_codes = lay.twin(blocks)
    assert g.info == want.info, "%s: %r, expected %r" % (what, g.info, want.info)
    assert g.branch_records().tobytes() == want.branches.tobytes(), what + ": branch records"
    assert g.node_records().tobytes() == want.nodes.tobytes(), what + ": node records"
    for take, name in ((lambda: g.branches, 'branch_ranks'), (lambda: g.nodes, 'node_ranks')):
        handed = take()
        try:
            assert handed.info['listed'] == len(want.branches if name == 'branch_ranks' else want.nodes)
            hold_field(handed.ranks, fields[name], lay, "%s: %s" % (what, name), distinct=2)
        finally:
            handed.destroy()
    pair = g.classes()
    try:
        classes = lay.twin(fields['classes'])
        hold(pair, np.ascontiguousarray(np.stack([twin_codes, classes.astype(twin_codes.dtype)], axis=-1)), lay.windows(), what + ": classes")
        background(pair, lay.between(), 0, what + ": classes")
    finally:
        pair.destroy()
    length, debris, fill = prune
    gone = dropped(want.branches, length, flags=1 if debris else 0)
    assert 0 < int(gone.sum()) < len(gone), "%s: prune(%d) drops %d of %d branches" % (what, length, int(gone.sum()), len(gone))
    pruned = g.prune(length, debris=debris, fill=fill)
    try:
        expected = [prune_texels(b, c, r, want.branches, length, flags=1 if debris else 0, fill=fill) for b, c, r in zip(blocks, fields['classes'], fields['branch_ranks'])]
        assert any((e != np.where(c != 0, b, fill)).any() for e, b, c in zip(expected, blocks, fields['classes']))      # a dropped voxel in a slab
        twin = np.full(twin_codes.shape, fill, twin_codes.dtype)
        for t0, e in zip(lay.twin_starts, expected):
            twin[t0:t0 + lay.thick] = e
        hold(pruned, twin, lay.windows(), what + ": prune")
        background(pruned, lay.between(), fill, what + ": prune")
    finally:
        pruned.destroy()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind,bits", [('odd', 16), ('aligned', 8)])
def test_graph_of_more_than_2_31_voxels(gpu_ctx, kind, bits):
    """Tier A, the solids, two graphs: of the 'ends' skeleton (Skeleton.graph: the thinned bars, boxes and balls, one bar through voxel
    2^31) and of the upper eighth of the codes of the solids themselves (Volume.graph: specks and short chains of the noise, with nodes where
    they clump).  The list of kept voxels holds 32-bit linear indices, the tips travel through the wave's shuffles as 32-bit values, and the
    class field is labelled by the components' tile pass at 26-connectivity over more than 2^31 voxels.  Expected: the statement on the
    crops, put together (large_volumes.graph_on_crops; tests/test_large_volumes_host.py holds that to the statement on a whole volume).
    Peak, n voxels, V the source, F a voxel field: while the skeleton's graph is built V + F (the skeleton) + 2 F (the branches' and the
    nodes' labellings) + n (the class field) + the bit plane + 4 n (the components' count array, components_build) = 21.4 + 45.1 + 12.7 =
    79.2 GiB (R16), 10.6 + 37.5 + 12.7 = 60.8 GiB (R8); while it is read V + 2 F + n + a handed-out copy F or the class pair volume (the
    larger: RG) = 21.4 + 30.0 + 2.5 + 42.7 = 96.6 GiB (R16), 10.6 + 25.0 + 2.5 + 21.2 = 59.3 GiB (R8); the list is kilobytes.  The
    thinning that runs first, with V resident, stays below both (test_skeleton_in_large_volumes: V + F + three bit planes + the tile flags =
    37.4 GiB R16, 24.0 GiB R8); it is in the maximum all the same."""
    shape = TIER_A[kind]
    n = tier(shape, 1 << 31, 0xFFFFFFFE)
    nx, ny, nz = shape
    item = bits // 8
    V, F, plane = volume_bytes(shape, item), field_bytes(shape, item), 4 * 2 * ((nx + 63) // 64) * ny * nz
    require(max(V + F + 3 * plane + 16 * tiles_of(shape, 64, 8, 4), V + 3 * F + 5 * n + plane, V + 2 * F + n + max(F, volume_bytes(shape, item, 2))))
    dtype, M = DTYPE[bits], (1 << bits) - 1
    lay = solid_layout(shape, four_bytes=True)
    blocks, crops = solids(lay, dtype, 301)
    lo = M - M // 8
    burn, _ = skeleton_on_crops(lay, blocks, crops, 1, M, 'ends')
    cases = {'skeleton': [b == 0xFFFFFFFF for b in burn], 'range': [b >= lo for b in blocks]}
    stated = {}
    for what, kept in cases.items():
        want, fields = graph_on_crops(lay, kept, crops)
        # what makes the case say something, from the statement alone
        assert want.info['branches'] >= 8 and int(want.branches['tip_hi'].max()) >= 1 << 31, what
        last = fields['branch_ranks'][-1]
        assert last.any() and (fields['branch_ranks'][-2] != 0).any(), what                 # a branch in the last slab, and in the slab of voxel 2^31
        z, y, x = np.nonzero(last)
        assert int(((z + lay.starts[-1]) * ny + y).max()) * nx >= 1 << 31, what              # a listed branch voxel whose index needs 32 bits
        stated[what] = (want, fields)
    assert stated['range'][0].info['nodes'] >= 4 and stated['range'][0].info['links'] >= 1 and stated['range'][0].info['spurs'] >= 4
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        found = src.skeleton(1, M, 'ends')
        try:
            g = found.graph()
        finally:
            found.destroy()
        try:
            hold_graph(g, *stated['skeleton'], blocks, lay, (40, True, 5), "the skeleton's graph R%d %s" % (bits, kind))
        finally:
            g.destroy()
        g = src.graph(lo, M)
    finally:
        src.destroy()
    try:
        hold_graph(g, *stated['range'], blocks, lay, (20, False, 0), "the graph of %d .. %d R%d %s" % (lo, M, bits, kind))
    finally:
        g.destroy()


# ---- the surface -----------------------------------------------------------------------------------------------------------------
def surface_bytes(shape, scan_words=2048):
    """the scratch of vpt_volume_surface: the inside plane, four mask arrays and two count arrays of the cell words, the block sums"""
    nx, ny, nz = shape
    words = (ny + 1) * (nz + 1) * ((nx + 1 + 31) // 32)
    return 4 * (ny + 2) * (nz + 2) * ((nx + 2 + 31) // 32) + 24 * words + 8 * (2 * ((words + scan_words - 1) // scan_words) + 2), words


def same_mesh(s, vertices, quads, info, page=1 << 18):
    got = s.info
    assert got == info, "%r, expected %r" % (got, info)
    for read, want, what in ((s.vertices, vertices, 'vertices'), (s.quads, quads, 'quads')):
        for first in range(0, len(want), page):
            differences(read(first, min(page, len(want) - first)), want[first:first + page], "%s %d .." % (what, first))


@pytest.mark.timeout(240)
@pytest.mark.parametrize("tier_name,kind,bits,channels", [('B', 'aligned', 8, 1), ('B', 'odd', 8, 2), ('A', 'aligned', 16, 1)])
def test_surface_of_solids_in_large_volumes(gpu_ctx, tier_name, kind, bits, channels):
    """Vertices, quads and info of the solids' surface at half the code range; the RG8 volume is read at channel 1.  With the default
    SF_SCAN_WORDS = 2048 words a block a tier B volume has more than 65 535 scan blocks, the cap of the scan kernels' launches: 996 x 4097
    rows of 34 cell words = 138 740 808 words = 67 745 blocks ('aligned'), 1024 x 4097 x 33 = 138 445 824 words = 67 601 blocks ('odd').
    Peak: source V (R8 19.9, RG8 39.8, R16 21.4) + the inside plane 0.5 + six arrays of the cell words 3.1 (tier A: 0.3 + 2.0) = 23.5 / 43.4 /
    23.7 GiB; the mesh itself is kilobytes."""
    shape = (TIER_B if tier_name == 'B' else TIER_A)[kind]
    tier(shape, 1 << 32) if tier_name == 'B' else tier(shape, 1 << 31, 1 << 32)
    scratch, words = surface_bytes(shape)
    assert ((words + 2047) // 2048 > 65535) == (tier_name == 'B')
    require(volume_bytes(shape, bits // 8, channels) + scratch)
    dtype, M = DTYPE[bits], (1 << bits) - 1
    lay = solid_layout(shape)
    blocks, crops = solids(lay, dtype, 281, channels)
    vertices, quads, info = surface_on_crops(lay, blocks, crops, M // 2, channels - 1)
    assert len(vertices) >= 1000 and int(vertices[:, 2].max()) >> 16 == shape[2]
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        s = src.surface(M // 2, channels - 1)
    finally:
        src.destroy()
    try:
        same_mesh(s, vertices, quads, info)
    finally:
        s.destroy()


@pytest.mark.timeout(240)
def test_surface_of_noise_slabs_of_more_than_2_32_voxels(gpu_ctx):
    """Tier B, single planes of noise at a level in the top sixteenth of the codes: every slab holds 65 000 specks, more than 2^20
    vertices in all, so the offsets of the far slab are large and its cell words lie behind word 2^27.  The expected mesh is the
    statement's on the twin (7 planes), its vertices moved along z.  Peak: source V 19.9 + the inside plane 0.5 + six arrays of the cell
    words 3.1 + the mesh 0.06 = 23.6 GiB."""
    shape = TIER_B['odd']
    tier(shape, 1 << 32)
    scratch, words = surface_bytes(shape)
    assert words > 1 << 27
    require(volume_bytes(shape, 1) + scratch + (1 << 26))
    lay = Layout(shape, 1, 2)
    blocks = lay.noise(np.uint8, 291)
    info = {}
    vertices, quads = surface_texels(lay.twin(blocks), 241, info=info)
    vertices = shift_twin_vertices(lay, vertices)
    info.update(cells=(shape[0] + 1) * (shape[1] + 1) * (shape[2] + 1), depth=shape[2])
    assert len(vertices) >= 1 << 20 and 12 * len(vertices) + 16 * len(quads) < 1 << 26
    src = sparse_volume(gpu_ctx, lay, blocks)
    try:
        s = src.surface(241)
    finally:
        src.destroy()
    try:
        same_mesh(s, vertices, quads, info)
    finally:
        s.destroy()
