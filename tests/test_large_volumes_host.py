"""CPU: the method of tests/test_gpu_large_volumes.py on shapes small enough to hold whole.

The GPU tests never see a large volume's expected texels as a whole: they take them from the numpy statement applied to the twin, the
slabs stacked with background planes between them (tests/large_volumes.py).  That rests on one equivalence, shown here for every operation
those tests use, with the same slab layout on 11 x 9 x 40 voxels: the statement on the whole sparse volume, restricted to the planes the
GPU tests compare, equals the statement on the twin there; and the background planes they read are what they expect.  For the operations of
tests/test_gpu_derive_large.py, whose slabs hold a few small solids, the same on 75 x 61 x 44 voxels: the statement on a crop round each
solid, put together, equals the statement on the whole volume everywhere."""
import numpy as np
import pytest

import vpt_amd
from vpt_amd.resample import nearest_index

from large_volumes import (TIER_A, TIER_B, REACH, MARGIN, Layout, voxels, volume_bytes, distance_squared_within, slab_distances, counts, solids, crop_array,
                           on_crops, watershed_on_crops, skeleton_on_crops, graph_on_crops, surface_on_crops, shift_twin_vertices, thickness_tiles)

SHAPE = (11, 9, 40)                                               # nx, ny, nz
MARK = 11 * 9 * 21 + 5                                            # the linear voxel index the middle slab straddles
DTYPES = (np.uint8, np.uint16)


def layout(thick, gap, even=False, marks=(MARK,)):
    return Layout(SHAPE, thick, gap, marks=marks, even=even)


def same_in_windows(whole, twin, windows, what, distinct=8):
    for z_lo, z_hi, t_lo in windows:
        a, b = whole[z_lo:z_hi], twin[t_lo:t_lo + z_hi - z_lo]
        assert a.shape == b.shape and np.array_equal(a, b), "%s: planes %d .. %d" % (what, z_lo, z_hi - 1)
        assert len(np.unique(b)) >= distinct, "%s: %d distinct values in planes %d .. %d" % (what, len(np.unique(b)), z_lo, z_hi - 1)


def test_the_shapes_of_the_tiers():
    for shape in TIER_B.values():
        assert voxels(shape) > 1 << 32 and max(shape) <= 4096
    for shape in TIER_A.values():
        assert 1 << 31 < voxels(shape) < 0xFFFFFFFE and max(shape) <= 4096
    for tier in (TIER_A, TIER_B):
        assert tier['aligned'][0] % 32 == 0 and tier['odd'][0] % 2 == 1
    # the far slab of a tier B volume lies behind voxel 2^32, and the slab of a mark holds the mark with planes around it
    for shape in list(TIER_B.values()) + list(TIER_A.values()):
        nx, ny, nz = shape
        for thick in (1, 2, 3, 4):
            lay = Layout(shape, thick, 2, marks=(1 << 30, 1 << 31), even=thick % 2 == 0)
            assert lay.starts[0] == 0 and lay.starts[-1] + thick == nz and len(lay.starts) == 4
            if shape in TIER_B.values() and thick <= 3:
                assert lay.starts[-1] * nx * ny > 1 << 32
            for mark, z0 in zip((1 << 30, 1 << 31), lay.starts[1:]):
                assert z0 * nx * ny <= mark < (z0 + thick) * nx * ny
    # the footprint of a volume: linear storage, the bricks' Z-order span, the atlas (a 2048^3 R8 volume has 2^27 slots of 128 bytes)
    assert volume_bytes((2048, 2048, 2048), 1) == (1 << 33) + ((1 << 34) + 64) + 6 * 2048 * 2048 * 4


@pytest.mark.parametrize("dtype", DTYPES)
def test_window_and_histogram_counts(dtype):
    lay = layout(2, 1)
    blocks = lay.noise(dtype, 3)
    whole, twin = lay.whole(blocks), lay.twin(blocks)
    M = int(np.iinfo(dtype).max)
    for bits in (8, 16):
        same_in_windows(vpt_amd.window_texels(whole, -16, M - 50, bits), vpt_amd.window_texels(twin, -16, M - 50, bits), lay.windows(), 'window')
        floor = vpt_amd.window_texels(np.zeros((1, 1, 1), dtype), -16, M - 50, bits)[0, 0, 0]
        assert (vpt_amd.window_texels(whole, -16, M - 50, bits)[lay.between()] == floor).all()
    shift = 8 * dtype().itemsize - 8
    assert np.array_equal(counts(blocks, 256, shift, whole.size), np.bincount((whole.reshape(-1) >> shift).astype(np.int64), minlength=256))
    assert np.array_equal(counts(blocks, M + 1, 0, whole.size), np.bincount(whole.reshape(-1).astype(np.int64), minlength=M + 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_local_operations(dtype):
    cases = [('smooth 1', 1, lambda a: vpt_amd.smooth_texels(a, 1)), ('smooth 2', 2, lambda a: vpt_amd.smooth_texels(a, 2)),
             ('median', 1, lambda a: vpt_amd.rank_texels(a, 'median')), ('erode', 1, lambda a: vpt_amd.rank_texels(a, 'erode')),
             ('central', 1, lambda a: vpt_amd.gradient_magnitude(a, 'central', 1.0)), ('sobel', 1, lambda a: vpt_amd.gradient_magnitude(a, 'sobel', 1.0))]
    for what, halo, statement in cases:
        lay = layout(3, 2 * halo)
        blocks = lay.noise(dtype, 5)
        whole, twin = statement(lay.whole(blocks)), statement(lay.twin(blocks))
        same_in_windows(whole, twin, lay.windows(halo), what, distinct=2 if what == 'erode' else 8)
        assert not whole[lay.between(halo)].any(), what
        outside = np.ones(SHAPE[2], bool)
        for z_lo, z_hi, _ in lay.windows(halo):
            outside[z_lo:z_hi] = False
        assert not whole[outside].any(), "%s reaches beyond its halo" % what


@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce(dtype):
    lay = layout(4, 2, even=True)
    blocks = lay.noise(dtype, 7)
    assert all(z0 % 2 == 0 for z0 in lay.starts + lay.twin_starts)
    whole, twin = vpt_amd.reduce_texels(lay.whole(blocks)), vpt_amd.reduce_texels(lay.twin(blocks))
    same_in_windows(whole, twin, lay.halved(), 'reduce')
    assert not whole[[z // 2 for z in lay.between(2)]].any()


def test_resample():
    nx, ny, nz = SHAPE
    lay = layout(2, 1)
    blocks = lay.noise(np.uint8, 9)
    whole, twin = lay.whole(blocks), lay.twin(blocks)
    # nearest, nz kept: plane Z copies plane Z
    same_in_windows(vpt_amd.resample_texels(whole, (nz, 7, 13), 'nearest'), vpt_amd.resample_texels(twin, (twin.shape[0], 7, 13), 'nearest'), lay.windows(), 'nearest')
    # nearest, half of z: plane Z copies plane 2 Z + 1
    down = vpt_amd.resample_texels(whole, (nz // 2, ny // 3, nx // 3), 'nearest')
    jx, jy = nearest_index(nx, nx // 3), nearest_index(ny, ny // 3)
    hit = 0
    for z0, block in zip(lay.starts, blocks):
        for z in range(z0, z0 + lay.thick):
            if z % 2 == 1:
                assert np.array_equal(down[z // 2], block[z - z0][jy][:, jx])
                hit += 1
    assert hit == len(blocks) and np.array_equal(down[nz // 2 - 1], blocks[-1][-1][jy][:, jx])
    # filtered, nz kept, single planes: every plane is a 2-D resample of its own
    lay = layout(1, 0)
    blocks = lay.noise(np.uint8, 10)
    for w, h in ((5, 12), (14, 4)):
        whole = vpt_amd.resample_texels(lay.whole(blocks), (nz, h, w), 'filtered')
        twin = vpt_amd.resample_texels(lay.twin(blocks), (3, h, w), 'filtered')
        same_in_windows(whole, twin, lay.windows(), 'filtered in the plane')
        assert np.array_equal(whole[[z for z, _, _ in lay.windows()][-2:]], vpt_amd.resample_texels(lay.twin(blocks)[-2:], (2, h, w), 'filtered'))
        assert not whole[lay.between() + [1]].any()
    # filtered, a quarter of z: whole cells of four planes
    lay = layout(4, 4, even=True)
    p = MARK // (nx * ny)
    lay.starts = [0, p - p % 4, nz - 4]
    blocks = lay.noise(np.uint16, 11)
    whole = vpt_amd.resample_texels(lay.whole(blocks), (nz // 4, 4, 5), 'filtered')
    for z0, block in zip(lay.starts, blocks):
        assert np.array_equal(whole[z0 // 4:z0 // 4 + 1], vpt_amd.resample_texels(block, (1, 4, 5), 'filtered'))
    assert not whole[[z0 // 4 + 1 for z0 in lay.starts[:-1]] + [nz // 4 - 2]].any()


@pytest.mark.parametrize("connectivity", (6, 26))
@pytest.mark.parametrize("dtype", DTYPES)
def test_components(dtype, connectivity):
    nx, ny, nz = SHAPE
    M = int(np.iinfo(dtype).max)
    lo = M - (M + 1) // 8 + 1
    lay = layout(2, 1, marks=(11 * 9 * 9, MARK))
    blocks = lay.noise(dtype, 13)
    whole, twin = lay.whole(blocks), lay.twin(blocks)
    ranks, listed = vpt_amd.components_texels(whole, lo, M, connectivity)
    twin_ranks, twin_listed = vpt_amd.components_texels(twin, lo, M, connectivity)
    assert listed == [(x, y, lay.to_volume(z), v) for x, y, z, v in twin_listed]
    assert len(listed) >= 4 and len({c[2] for c in listed}) >= 2 and len({c[3] for c in listed}) >= 2
    same_in_windows(ranks, twin_ranks, lay.windows(), 'ranks', distinct=3)
    assert not ranks[lay.between()].any()
    k = len(listed) // 2
    same_in_windows(vpt_amd.keep_texels(whole, ranks, 1, k), vpt_amd.keep_texels(twin, twin_ranks, 1, k), lay.windows(), 'keep')
    same_in_windows(vpt_amd.label_texels(whole, ranks), vpt_amd.label_texels(twin, twin_ranks), lay.windows(), 'label')


@pytest.mark.parametrize("dtype", DTYPES)
def test_distances(dtype):
    nx, ny, nz = SHAPE
    M = int(np.iinfo(dtype).max)
    lo = M - (M + 1) // 16 + 1
    lay = layout(3, REACH + 1)
    blocks = lay.noise(dtype, 17)
    whole, twin = lay.whole(blocks), lay.twin(blocks)
    d2, largest = slab_distances(lay, blocks, lo, M)                  # asserts the conditions
    everywhere = vpt_amd.distance_squared_texels(whole, lo, M, 'range')
    in_twin = vpt_amd.distance_squared_texels(twin, lo, M, 'range')
    for (z_lo, z_hi, t_lo), want in zip(lay.windows(), d2):
        assert np.array_equal(everywhere[z_lo:z_hi], want) and np.array_equal(in_twin[t_lo:t_lo + lay.thick], want)
        assert len(np.unique(want)) >= 8
    assert largest == max(int(d.max()) for d in d2)
    # the plane midway between the last two slabs: bounded from below by the nearer slab's nearest plane
    a, b = lay.starts[-2] + lay.thick - 1, lay.starts[-1]
    z = (a + b) // 2
    assert int(everywhere[z].min()) >= min(z - a, b - z) ** 2
    half = largest // 2
    near = vpt_amd.within_texels(whole, everywhere, 1, half, 3)
    pair = vpt_amd.channel_texels(whole, everywhere, 16)
    for (z_lo, z_hi, _), block, want in zip(lay.windows(), blocks, d2):
        assert np.array_equal(near[z_lo:z_hi], vpt_amd.within_texels(block, want, 1, half, 3))
        assert np.array_equal(pair[z_lo:z_hi], vpt_amd.channel_texels(block, want, 16))
    assert (near[z] == 3).all()
    # seeds 'rest': the far slab with the background plane in front of it
    lay = layout(3, 4)
    blocks = lay.noise(dtype, 19)
    whole = lay.whole(blocks)
    cut = M - (M + 1) * 5 // 8 + 1
    everywhere = vpt_amd.distance_squared_texels(whole, cut, M, 'rest')
    padded = np.concatenate([np.zeros((1, ny, nx), dtype), blocks[-1]])
    want = distance_squared_within(padded < cut, 4)[1:]
    assert int(want.max()) <= 4 * 4 + 2 * 4 and np.array_equal(everywhere[nz - 3:], want)
    assert not everywhere[lay.between()].any()
    assert int((whole < cut).sum()) == whole.size - int(sum((b >= cut).sum() for b in blocks))      # the seeds, as the GPU test counts them


def test_the_windowed_distances_are_the_statement_where_they_are_small():
    rng = np.random.default_rng(23)
    for shape, density in (((5, 17, 19), 0.05), ((3, 30, 9), 0.02), ((1, 1, 40), 0.1)):
        seed = rng.random(shape) < density
        a = np.where(seed, 200, 0).astype(np.uint8)
        exact = vpt_amd.distance_squared_texels(a, 200, 200)
        for reach in (2, 4, 8):
            got = distance_squared_within(seed, reach)
            assert (got >= exact).all()
            small = got <= reach * reach + 2 * reach
            assert np.array_equal(got[small], exact[small]) and small.any()
            assert np.array_equal(got[exact <= reach * reach], exact[exact <= reach * reach])


# ---- solids: reconstruction, watershed, thickness, skeleton, surface ----------------------------------------------------------------
# The solids need 72 voxels along x (a bar across the word edge x = 64) and room for a mark's bar beside the other solids of its slab, so
# these run on 75 x 61 x 44 voxels; the mark is a voxel of plane 20, row 55.
SOLID_SHAPE = (75, 61, 44)
SOLID_MARK = (20 * 61 + 55) * 75 + 40


def solid_layout(gap=2):
    return Layout(SOLID_SHAPE, 8, gap, marks=(SOLID_MARK,), even=True)


def test_the_solids_lie_where_the_large_tests_need_them():
    for shape, marks in [(SOLID_SHAPE, (SOLID_MARK,))] + [(s, (1 << 31,)) for s in list(TIER_A.values()) + list(TIER_B.values())]:
        nx, ny, nz = shape
        lay = Layout(shape, 8, 2, marks=marks, even=True)
        blocks, crops = solids(lay, np.uint8, 1)
        assert blocks[0][0, 0, 0] and blocks[-1][-1, -1, -1]                                 # the corner x = y = z = 0 and the volume's last voxel
        m = marks[0]
        z = m // (nx * ny)
        (slab,) = [i for i, z0 in enumerate(lay.starts) if z0 <= z < z0 + 8]
        assert blocks[slab][z - lay.starts[slab], m // nx % ny, m % nx]                     # the mark's voxel
        first = blocks[0] > 0
        assert first[:, :, 31].any() and first[:, :, 32].any() and first[:, :, 63].any() and first[:, :, 64].any()      # word edges along x
        assert first[:, 7, 28:35].any() and first[:, 8, 28:35].any() and first[3, :, 28:35].any() and first[4, :, 28:35].any()      # tile edges y = 8, z = 4
        if voxels(shape) > 1 << 32:
            assert lay.starts[-1] * nx * ny > 1 << 32                                        # all of the last slab lies beyond voxel 2^32
        assert len({i for i, *_ in crops}) == 3 and all(o % 2 == 0 for c in crops for o in crop_array(lay, blocks, c)[1])
        inside = [np.zeros(b.shape, bool) for b in blocks]
        for i, y0, y1, x0, x1 in crops:
            inside[i][:, y0:y1, x0:x1] = True
        assert not any(b[~w].any() for b, w in zip(blocks, inside))                          # nothing lies outside the crops
        assert all(len(np.unique(b)) >= 8 for b in blocks)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reconstruction_on_crops(dtype):
    """By dilation (and the operations built on it: hmax, dome): a voxel rises only along paths inside the mask, and background (0) parts
    the solids and the slabs, so one background plane between two slabs is enough.  The erosion side (fill_holes): the background falls from
    the marker on the volume's faces; a crop's faces are faces of the volume or background that is connected to one, in the volume as in the
    crop (the first and the last slab touch the z faces in both, the others keep MARGIN background planes)."""
    M = int(np.iinfo(dtype).max)
    lay = solid_layout()
    mask, crops = solids(lay, dtype, 3)
    other, _ = solids(lay, dtype, 13)
    marker = [np.where(np.random.default_rng(23 + i).random(b.shape) < 0.1, b, 0).astype(dtype) for i, b in enumerate(other)]
    pair = [np.ascontiguousarray(np.stack([a, b], axis=-1)) for a, b in zip(marker, mask)]
    for connectivity in (6, 26):
        whole = vpt_amd.reconstruct_texels(lay.whole(marker), lay.whole(mask), 'dilation', connectivity)
        got = on_crops(lay, pair, crops, lambda a: vpt_amd.reconstruct_texels(a, a, 'dilation', connectivity, 0, 1))
        assert np.array_equal(whole, lay.whole(got)) and len(np.unique(whole)) >= 8
        assert (whole != np.minimum(lay.whole(marker), lay.whole(mask))).any()               # something rose
    for op, h, connectivity in (('fill_holes', 0, 6), ('fill_holes', 0, 26), ('dome', M // 8, 6), ('hmax', M // 8, 26), ('minima', 0, 6)):
        whole = vpt_amd.geodesic_texels(lay.whole(mask), op, h, connectivity)
        floor = M if op == 'minima' else 0                                                   # the background is one minimum: M everywhere on it
        got = on_crops(lay, mask, crops, lambda a: floor ^ vpt_amd.geodesic_texels(a, op, h, connectivity))
        assert np.array_equal(whole, floor ^ lay.whole(got)), op
        assert (whole[lay.between()] == floor).all()
        assert len(np.unique(whole)) >= (2 if op == 'minima' else 8)
        if op == 'fill_holes':
            assert (whole > lay.whole(mask)).sum() >= 27                                     # the shell's cavity
    # the second channel of a two-channel source
    both, crops2 = solids(lay, dtype, 5, channels=2)
    assert crops2 == crops
    whole = vpt_amd.geodesic_texels(lay.whole(both), 'hmax', M // 8, 6, 1)
    assert np.array_equal(whole, lay.whole(on_crops(lay, both, crops, lambda a: vpt_amd.geodesic_texels(a, 'hmax', M // 8, 6, 1))))
    assert not np.array_equal(whole, vpt_amd.geodesic_texels(lay.whole(both), 'hmax', M // 8, 6, 0))


@pytest.mark.parametrize("polarity,connectivity", [('minima', 6), ('maxima', 26)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_watershed_on_crops(dtype, polarity, connectivity):
    """lo >= 1: the background is outside the domain, no basin leaves its solid; one background plane parts the slabs."""
    M = int(np.iinfo(dtype).max)
    lay = solid_layout()
    blocks, crops = solids(lay, dtype, 7)
    ranks, listed = vpt_amd.watershed_texels(lay.whole(blocks), 1, M, polarity, connectivity)
    got, got_listed = watershed_on_crops(lay, blocks, crops, 1, M, polarity, connectivity)
    assert listed == got_listed and len(listed) >= 16 and len({c[3] for c in listed}) >= 3
    assert np.array_equal(ranks, lay.whole(got))


@pytest.mark.parametrize("dtype", DTYPES)
def test_thickness_on_crops(dtype):
    """seeds 'rest': D inside a solid is the distance to the nearest background voxel, which lies in the solid's box widened by one voxel,
    and the balls stay inside their solid.  (gap + 1)^2 exceeds the largest D."""
    M = int(np.iinfo(dtype).max)
    lay = solid_layout(4)
    blocks, crops = solids(lay, dtype, 9)
    d2 = vpt_amd.distance_squared_texels(lay.whole(blocks), 1, M, 'rest')
    got_d2 = on_crops(lay, blocks, crops, lambda a: vpt_amd.distance_squared_texels(a, 1, M, 'rest'))
    assert np.array_equal(d2, lay.whole(got_d2))
    assert int(d2.max()) < (lay.gap + 1) ** 2 and int(d2.max()) < (MARGIN + 1) ** 2 + 8
    t2 = vpt_amd.thickness_squared_texels(d2)
    got = on_crops(lay, blocks, crops, lambda a: vpt_amd.thickness_squared_texels(vpt_amd.distance_squared_texels(a, 1, M, 'rest')))
    assert np.array_equal(t2, lay.whole(got)) and len(np.unique(t2)) >= 8
    z, y, x = np.nonzero(d2)
    assert thickness_tiles(lay, got_d2) == len(set(zip(z // 4, y // 8, x // 8)))
    pair = on_crops(lay, blocks, crops, lambda a: vpt_amd.thickness_texels(a, 1, M, 3))
    assert np.array_equal(vpt_amd.thickness_texels(lay.whole(blocks), 1, M, 3), lay.whole(pair))


@pytest.mark.parametrize("mode", ['ends', 'kernel', 'isthmus'])
def test_skeleton_on_crops(mode):
    """gap >= 2 and even, and every crop's origin is even: the eight subfields of a pass are the parities of (x, y, z)."""
    lay = solid_layout()
    assert lay.gap >= 2 and lay.gap % 2 == 0 and all(z % 2 == 0 for z in lay.starts)
    blocks, crops = solids(lay, np.uint8, 11)
    burn, info = vpt_amd.skeleton_burn_texels(lay.whole(blocks), 1, 255, mode)
    got, got_info = skeleton_on_crops(lay, blocks, crops, 1, 255, mode)
    assert info == got_info and info['kept_voxels'] > 0 and info['passes'] >= 3
    assert np.array_equal(burn, lay.whole(got))
    # a crop moved by one voxel thins otherwise: the parities matter
    moved = np.zeros((8, 12, 14), np.uint8)
    moved[1:7, 3:9, 3:12] = 200
    moved[2:4, 2:5, 2:4] = 200
    assert not np.array_equal(vpt_amd.skeleton_burn_texels(moved, 1, 255, mode)[0][:, :, 1:],
                              vpt_amd.skeleton_burn_texels(np.roll(moved, -1, axis=2), 1, 255, mode)[0][:, :, :-1])


def test_graph_on_crops():
    """The graph of the 'ends' skeleton's kept set and of value ranges of the solids themselves: info, every record and every rank of the
    crops' graphs put together (graph_on_crops) are graph_of of the whole volume.  The range 1 .. M keeps every solid whole (nodes); a range
    of the upper codes leaves specks and short chains of the noise inside them (branches)."""
    from vpt_amd import graph as G
    lay = solid_layout()
    blocks, crops = solids(lay, np.uint8, 11)
    burn, _ = skeleton_on_crops(lay, blocks, crops, 1, 255, 'ends')
    sets = {'skeleton': [b == 0xFFFFFFFF for b in burn], '1 .. M': [b >= 1 for b in blocks], '224 .. M': [b >= 224 for b in blocks]}
    seen = {}
    for what, kept in sets.items():
        want = G.graph_of(lay.whole(kept))
        graph, fields = graph_on_crops(lay, kept, crops)
        assert graph.info == want['info'], what
        assert graph.branches.tobytes() == want['branches'].tobytes() and graph.nodes.tobytes() == want['nodes'].tobytes(), what
        for name, blocks_of in fields.items():
            assert np.array_equal(lay.whole(blocks_of), want[name]) and lay.whole(blocks_of).dtype == want[name].dtype, (what, name)
        seen[what] = want['info']
    assert seen['skeleton']['branches'] >= len(crops) // 2 and seen['skeleton']['kept_voxels'] > 0
    assert seen['1 .. M']['nodes'] >= len(crops) and seen['224 .. M']['branches'] >= 64 and seen['224 .. M']['links'] > 0 and seen['224 .. M']['spurs'] > 0


@pytest.mark.parametrize("dtype", DTYPES)
def test_surface_on_crops_and_on_the_twin(dtype):
    from vpt_amd.surface import surface_texels
    M = int(np.iinfo(dtype).max)
    lay = solid_layout()
    for channels, channel in ((1, 0), (2, 1)):
        blocks, crops = solids(lay, dtype, 15, channels)
        info = {}
        v, q = surface_texels(lay.whole(blocks), M // 2, channel, info=info)
        gv, gq, got_info = surface_on_crops(lay, blocks, crops, M // 2, channel)
        assert info == got_info and len(v) >= 1000
        assert np.array_equal(v, gv) and np.array_equal(q, gq)
    # noise slabs: the twin's vertices moved along z, the quads as they are (gap >= 2)
    for thick in (1, 2):
        lay = Layout(SOLID_SHAPE, thick, 2, marks=(SOLID_MARK,))
        blocks = lay.noise(dtype, 17)
        level = M - (M + 1) // 16 + 1
        info, twin_info = {}, {}
        v, q = surface_texels(lay.whole(blocks), level, info=info)
        tv, tq = surface_texels(lay.twin(blocks), level, info=twin_info)
        assert np.array_equal(v, shift_twin_vertices(lay, tv)) and np.array_equal(q, tq) and len(v) >= 1000
        assert {k: info[k] for k in ('vertices', 'quads', 'inside', 'crossings')} == {k: twin_info[k] for k in ('vertices', 'quads', 'inside', 'crossings')}
