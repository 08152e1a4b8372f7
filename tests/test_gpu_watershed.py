"""GPU: the watershed by steepest descent on a lower-completed relief (vpt_volume_watershed) on the device.

Every rank and the basin list are held, word for word, to vpt_amd.watershed_texels, the numpy statement of the contract
(tests/test_watershed_host.py holds that to a walk over Python integers).

The tile kernels' workgroup owns a tile of 64 x 8 x 4 voxels with a one-voxel rim; the plateau kernel is launched again over the tiles a
neighbour flagged.  The shapes are test_gpu_reconstruct's, the smallest at which that can go wrong: one voxel; a run shorter than a wave;
odd everywhere; exactly one tile; one voxel more on every axis; (130, 17, 9), three tiles on every axis, so face, edge and corner
neighbours all exist; and 4000 x 3 x 3, a long run of tiles on one axis."""
import ctypes as C

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.components import keep_texels, label_texels
from vpt_amd.measure import measure_texels, keep_set_texels
from vpt_amd.watershed import descent_texels, split_texels, watershed_texels

from test_gpu_pyramid import upload, whole
from reconstruct_cases import CONNECTIVITIES, DTYPES, largest, serpentine, two_balls, value_sets

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1), (5, 1, 1), (7, 5, 3), (64, 8, 4), (65, 9, 5), (130, 17, 9), (4000, 3, 3))
THREE_TILES = (130, 17, 9)
MIN_CAPS = (3, 1)                                                # merge_steps, flatten_steps: the smallest vpt_volume_components_capped takes


def held(basins, want, what):
    """the handle's ranks and list against the statement's (ranks, list); destroys the handle"""
    want_ranks, want_list = want
    try:
        got = basins.ranks()
        assert got.dtype == np.uint32 and got.shape == want_ranks.shape, what
        bad = np.argwhere(got != want_ranks)
        assert len(bad) == 0, "%d ranks differ (%s), first at %s: %d, expected %d" % (len(bad), what, bad[0], got[tuple(bad[0])], want_ranks[tuple(bad[0])])
        assert basins.list() == want_list, what
        info = basins.info
        assert info['listed'] == len(want_list) and info['listed_voxels'] == sum(b[3] for b in want_list), (what, info)
    finally:
        basins.destroy()


# ---- ranks and list ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_ranks_and_list_equal_the_statement(gpu_ctx, dtype, shape):
    M = largest(dtype)
    for name, _, relief in value_sets(dtype, shape, seed=41 + SHAPES.index(shape)):
        v = upload(gpu_ctx, relief)
        for c in CONNECTIVITIES:
            for polarity in ('minima', 'maxima'):
                for lo, hi in ((0, M), (M // 4, M) if polarity == 'minima' else (0, M - M // 4)):        # the whole range; codes cut off at one end
                    what = "%s %s %s, %d %s [%d, %d]" % (np.dtype(dtype).name, shape, name, c, polarity, lo, hi)
                    basins = v.watershed(lo, hi, polarity, c)
                    assert basins.info['foreground_voxels'] == np.count_nonzero((relief >= lo) & (relief <= hi)), what
                    held(basins, watershed_texels(relief, lo, hi, polarity, c), what)
        assert whole(v).tobytes() == relief.tobytes(), "the source changed"
        v.destroy()


# ---- a plateau across a tile corner and a tile edge --------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_plateau_that_touches_only_across_a_tile_corner_or_edge(gpu_ctx, dtype):
    """two voxels of code 200, (63, 7, 3) and ``second``, the first with a lower neighbour (62, 7, 3): d crosses to the second, and the
    second joins the first's basin, only where the two are neighbours: across a tile corner under 26, across a tile edge under 18 and 26"""
    for second, joined_under in (((64, 8, 4), (26,)), ((64, 8, 3), (18, 26))):
        nx, ny, nz = THREE_TILES
        relief = np.zeros((nz, ny, nx), dtype=dtype)
        relief[3, 7, 63] = relief[second[2], second[1], second[0]] = 200
        relief[3, 7, 62] = 100
        v = upload(gpu_ctx, relief)
        for c in CONNECTIVITIES:
            want = watershed_texels(relief, 1, largest(dtype), 'minima', c)
            assert [b[3] for b in want[1]] == ([3] if c in joined_under else [2, 1]), (second, c)
            d = descent_texels(relief, 1, largest(dtype), 'minima', c)[1]
            assert d[second[2], second[1], second[0]] == (1 if c in joined_under else -1), (second, c)
            held(v.watershed(1, largest(dtype), 'minima', c), want, "touching at %s under %d" % (second, c))
        v.destroy()


# ---- serpentines: the host's loops and the in-tile loop ------------------------------------------------------------------------------
def path_of(mask):
    """the voxels (z, y, x) of ``serpentine``'s path in order, from (0, 0, 0)"""
    _, ny, nx = mask.shape
    path = []
    for y in range(0, ny, 2):
        forward = (y // 2) % 2 == 0
        xs = range(nx) if forward else range(nx - 1, -1, -1)
        path.extend((0, y, x) for x in xs)
        if y + 2 < ny:
            path.append((0, y + 1, nx - 1 if forward else 0))
    assert len(path) == np.count_nonzero(mask) and all(mask[p] for p in path)
    return path


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_descending_serpentine_is_one_basin_whatever_the_caps(gpu_ctx, dtype):
    _, mask, length = serpentine((130, 17, 1), dtype)
    path = path_of(mask)
    relief = np.zeros_like(mask)
    for i, p in enumerate(path):
        relief[p] = 250 - i // 7                                  # falls by one every 7 voxels along the path; off the path: 0, outside D
    assert relief[path[-1]] >= 1
    M = largest(dtype)
    want = watershed_texels(relief, 1, M, 'minima', 6)
    assert want[1] == [(0, 0, 0, length)]
    _, d, pointer = descent_texels(relief, 1, M, 'minima', 6)
    index = lambda p: (p[0] * mask.shape[1] + p[1]) * mask.shape[2] + p[2]
    last_run = [p for p in path if relief[p] == relief[path[-1]]]               # the regional minimum: the path's last code
    assert len(last_run) == 1 + (length - 1) % 7 and all(d[p] == -1 and pointer[p] == index(p) for p in last_run)
    assert all(pointer[a] == index(b) for a, b in zip(path, path[1:len(path) - len(last_run) + 1])), "the pointer chain is the whole path down to the minimum"
    v = upload(gpu_ctx, relief)
    held(v.watershed(1, M, 'minima', 6), want, "descending serpentine")
    basins, profile = v.watershed_timed(1, M, 'minima', 6)
    print("descending serpentine: %r, merge and flatten launches %r" % (profile, basins.profile()[1:]))
    held(basins, want, "descending serpentine, timed")
    for tile_rounds in (1, 3):
        basins, profile = v.watershed_timed(1, M, 'minima', 6, _caps=MIN_CAPS + (tile_rounds,))
        merges, flattens = basins.profile()[1:]
        print("caps %r: %d plateau, %d merge, %d flatten launches" % (MIN_CAPS + (tile_rounds,), profile['plateau_launches'], merges, flattens))
        held(basins, want, "descending serpentine, caps %r" % (MIN_CAPS + (tile_rounds,),))
    v.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_plateau_serpentine_runs_d_against_the_tile_order(gpu_ctx, dtype):
    _, mask, length = serpentine((130, 17, 1), dtype)
    path = path_of(mask)
    relief = mask.copy()                                          # the whole path one code ...
    relief[path[-1]] = 199                                        # ... only its last voxel lower
    M = largest(dtype)
    want = watershed_texels(relief, 1, M, 'minima', 6)
    assert want[1] == [(0, 0, 0, length)]
    d = descent_texels(relief, 1, M, 'minima', 6)[1]
    assert d[path[0]] == length - 2 and d[path[-2]] == 0 and d[path[-1]] == -1
    v = upload(gpu_ctx, relief)
    basins, profile = v.watershed_timed(1, M, 'minima', 6)
    print("plateau serpentine: %r" % (profile,))
    assert profile['plateau_launches'] > 1 and all(ms >= 0.0 for ms in profile['ms'].values()) and profile['ms']['plateau'] > 0.0
    held(basins, want, "plateau serpentine")
    for tile_rounds in (1, 3):
        basins, capped = v.watershed_timed(1, M, 'minima', 6, _caps=MIN_CAPS + (tile_rounds,))
        assert capped['plateau_launches'] > profile['plateau_launches'], "a tile cut short goes on in the next launch"
        held(basins, want, "plateau serpentine, %d rounds a launch" % tile_rounds)
        held(v.watershed(1, M, 'minima', 6, _caps=MIN_CAPS + (tile_rounds,)), want, "plateau serpentine, capped and untimed")
    # from the maxima the complement is the same relief
    inverse = upload(gpu_ctx, np.where(mask != 0, M - relief.astype(np.int64), 0).astype(dtype))
    held(inverse.watershed(1, M, 'maxima', 6), want, "plateau serpentine from the maxima")
    inverse.destroy(); v.destroy()


# ---- other cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_a_checkerboard_has_a_basin_per_low_voxel(gpu_ctx):
    z, y, x = np.mgrid[0:5, 0:9, 0:65]
    relief = ((x + y + z) & 1).astype(np.uint8)
    want = watershed_texels(relief, 0, 255, 'minima', 6)
    assert len(want[1]) == np.count_nonzero(relief == 0) > relief.size // 2 - 1
    v = upload(gpu_ctx, relief)
    held(v.watershed(0, 255, 'minima', 6), want, "checkerboard")
    held(v.watershed(0, 255, 'minima', 6, min_voxels=3), watershed_texels(relief, 0, 255, 'minima', 6, 3), "checkerboard, min_voxels 3")
    v.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_constant_volume_is_one_basin_joined_across_every_tile_face(gpu_ctx, dtype):
    nx, ny, nz = THREE_TILES
    relief = np.full((nz, ny, nx), largest(dtype) // 3, dtype=dtype)
    v = upload(gpu_ctx, relief)
    for c in CONNECTIVITIES:
        for polarity in ('minima', 'maxima'):
            basins = v.watershed(0, largest(dtype), polarity, c)
            assert basins.list() == [(0, 0, 0, nx * ny * nz)] and basins.info['dropped'] == 0
            assert (basins.ranks() == 1).all()
            basins.destroy()
    v.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_two_channel_relief_texels_min_voxels_and_the_emitters(gpu_ctx, dtype):
    M = largest(dtype)
    (_, a, b), (_, p, q) = value_sets(dtype, (65, 9, 5), seed=53)[:2]
    two = np.stack([a, q], axis=-1)
    vtwo, vother = upload(gpu_ctx, two), upload(gpu_ctx, b)
    for channel in (0, 1):
        relief = two[..., channel]
        want = watershed_texels(two, M // 8, M, 'maxima', 18, 1, channel)
        assert np.array_equal(want[0], watershed_texels(relief, M // 8, M, 'maxima', 18)[0])
        basins = vtwo.watershed(M // 8, M, 'maxima', 18, channel=channel)
        # the snapshot is the chosen channel, one channel wide
        kept = basins.keep(1, 3, 7)
        assert kept.native_format()[0] == (N.FORMAT_R16 if dtype == np.uint16 else N.FORMAT_R8)
        assert np.array_equal(whole(kept), keep_texels(relief, want[0], 1, 3, 7))
        labelled = basins.label()
        assert np.array_equal(whole(labelled), label_texels(relief, want[0]))
        kept.destroy(); labelled.destroy()
        held(basins, want, "channel %d of a two-channel relief" % channel)
        # texels given: the emitters speak of the other volume; measure reads it without `values`
        basins = vtwo.watershed(M // 8, M, 'maxima', 18, 4, channel, texels=vother)
        want = watershed_texels(two, M // 8, M, 'maxima', 18, 4, channel)
        assert basins.info['dropped'] > 0 and basins.info['listed'] == len(want[1]) > 0
        for out, expect in ((basins.keep(2, None), keep_texels(b, want[0], 2, None)), (basins.keep_set([1, 3, 4], 9), keep_set_texels(b, want[0], [1, 3, 4], 9)),
                            (basins.label(), label_texels(b, want[0]))):
            assert np.array_equal(whole(out), expect)
            out.destroy()
        assert np.array_equal(basins.measure(), measure_texels(want[0], b))
        assert np.array_equal(basins.measure(values=vtwo, channel=1), measure_texels(want[0], two[..., 1]))
        held(basins, want, "channel %d, min_voxels 4, texels given" % channel)
    assert whole(vtwo).tobytes() == two.tobytes() and whole(vother).tobytes() == b.tobytes(), "a source changed"
    # the sources may be destroyed: the handle owns what it needs
    basins = vtwo.watershed(0, M, 'minima', 6, texels=vother)
    vtwo.destroy(); vother.destroy()
    kept = basins.keep(1, 1)
    assert np.array_equal(whole(kept), keep_texels(b, watershed_texels(a, 0, M, 'minima', 6)[0], 1, 1))
    kept.destroy(); basins.destroy()


@pytest.mark.timeout(120)
def test_measure_on_a_watershed_handle(gpu_ctx):
    _, _, relief = value_sets(np.uint8, THREE_TILES, seed=59)[1]
    v = upload(gpu_ctx, relief)
    for c in (6, 26):
        want = watershed_texels(relief, 60, 255, 'minima', c, 2)
        basins = v.watershed(60, 255, 'minima', c, 2)
        records = basins.measure()
        assert len(records) == len(want[1]) > 1 and np.array_equal(records, measure_texels(want[0], relief))
        assert [int(r) for r in records['voxels']] == [b[3] for b in want[1]]
        basins.destroy()
    v.destroy()


@pytest.mark.timeout(120)
def test_two_runs_give_identical_bytes(gpu_ctx):
    _, _, relief = value_sets(np.uint16, THREE_TILES, seed=61)[1]
    v = upload(gpu_ctx, relief)
    first, second = v.watershed(0, 65535, 'maxima', 26), v.watershed(0, 65535, 'maxima', 26)
    assert first.ranks().tobytes() == second.ranks().tobytes() and first.list() == second.list()
    first.destroy(); second.destroy(); v.destroy()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def refused(call, code, *names):
    with pytest.raises(vpt_amd.VptError) as e:
        call()
    assert e.value.code == code, str(e.value)
    for name in names:
        assert name in str(e.value), str(e.value)


@pytest.mark.timeout(120)
def test_every_refusal_of_the_contract(gpu_ctx):
    L = N.lib()
    a8 = upload(gpu_ctx, np.zeros((3, 4, 5), dtype=np.uint8))
    b8 = upload(gpu_ctx, np.zeros((3, 4, 6), dtype=np.uint8))
    rg8 = upload(gpu_ctx, np.zeros((3, 4, 5, 2), dtype=np.uint8))
    a16 = upload(gpu_ctx, np.zeros((3, 4, 5), dtype=np.uint16))
    f32 = upload(gpu_ctx, np.zeros((3, 4, 5), dtype=np.float32))
    s8 = upload(gpu_ctx, np.zeros((3, 4, 5), dtype=np.int8))
    other_ctx = vpt_amd.Context(0)
    elsewhere = upload(other_ctx, np.zeros((3, 4, 5), dtype=np.uint8))
    out = C.c_void_p()

    def ws(relief, channel=0, texels=None, lo=0, hi=255, polarity=0, c=6, min_voxels=1):
        return lambda: N.check(L.vpt_volume_watershed(relief.texture, channel, texels.texture if texels else None, lo, hi, polarity, c, min_voxels, C.byref(out)))

    def capped(merge_steps, flatten_steps, tile_rounds, relief=None):
        return lambda: N.check(L.vpt_volume_watershed_capped(relief.texture if relief else None, 0, None, 0, 255, 0, 6, 1, merge_steps, flatten_steps, tile_rounds,
                                                             C.byref(out), None, None))
    refused(ws(f32), N.ERR_UNSUPPORTED, 'relief', 'R32F')
    refused(ws(s8), N.ERR_UNSUPPORTED, 'relief', 'R8_SNORM')
    refused(ws(a8, 2), N.ERR_INVALID, 'channel 2')
    refused(ws(a8, -1), N.ERR_INVALID, 'channel -1')
    refused(ws(a8, 1), N.ERR_INVALID, 'channel 1', 'R8')
    refused(ws(a8, lo=3, hi=2), N.ERR_INVALID, '[3, 2]')
    refused(ws(a8, hi=256), N.ERR_INVALID, '256', '255')
    refused(ws(a16, hi=65536), N.ERR_INVALID, '65536', '65535')
    for polarity in (-1, 2):
        refused(ws(a8, polarity=polarity), N.ERR_INVALID, 'polarity %d' % polarity)
    for c in (0, 4, 8, 27):
        refused(ws(a8, c=c), N.ERR_INVALID, 'connectivity %d' % c)
    refused(ws(a8, min_voxels=0), N.ERR_INVALID, 'min_voxels 0')
    refused(ws(a8, texels=rg8), N.ERR_UNSUPPORTED, 'texels', 'RG8')
    refused(ws(a8, texels=f32), N.ERR_UNSUPPORTED, 'texels', 'R32F')
    refused(ws(a8, texels=elsewhere), N.ERR_INVALID, 'two contexts')
    refused(ws(a8, texels=b8), N.ERR_INVALID, '5x4x3', '6x4x3')
    refused(ws(a8, texels=a16), N.ERR_INVALID, 'R8', 'R16')
    refused(ws(rg8, 1, texels=a16), N.ERR_INVALID, 'RG8', 'R16')
    # the caps come first: a refused cap touches no other argument (the relief is null here)
    refused(capped(2, 1, 1), N.ERR_INVALID, 'merge_steps 2')
    refused(capped(3, 0, 1), N.ERR_INVALID, 'flatten_steps 0')
    for rounds in (0, -3):
        refused(capped(3, 1, rounds), N.ERR_INVALID, 'tile_rounds %d' % rounds)
    refused(capped(3, 1, 1), N.ERR_INVALID, 'null')
    refused(lambda: N.check(L.vpt_volume_watershed_timed(a8.texture, 0, None, 0, 255, 0, 6, 1, C.byref(out), None, None)), N.ERR_INVALID, 'null')
    assert not out.value, "a refused call hands nothing out"
    # the host checks refuse the same before the library is asked
    for call in (lambda: a8.watershed(0, 255, 'both'), lambda: a8.watershed(0, 255, connectivity=7), lambda: a8.watershed(0, 255, channel=1),
                 lambda: a8.watershed(3, 2), lambda: a8.watershed(0, 256), lambda: a8.watershed(0, 255, min_voxels=0), lambda: a8.watershed(0, 255, texels=3),
                 lambda: a8.split(3, 2), lambda: a8.split(1, 255, h=256), lambda: a8.split(1, 255, steps=0), lambda: a8.split(1, 255, connectivity=5)):
        with pytest.raises(ValueError):
            call()
    for v in (a8, b8, rg8, a16, f32, s8, elsewhere):
        v.destroy()
    other_ctx.destroy()


# ---- the worked example of the contract, end to end on the device -------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_split_of_two_overlapping_balls(gpu_ctx):
    a = two_balls(19)
    v = upload(gpu_ctx, a)
    basins = v.split(100, 255)
    assert basins.list() == [(9, 8, 2, 924), (19, 8, 2, 887)]
    assert basins.info == {'listed': 2, 'dropped': 0, 'foreground_voxels': 1811, 'listed_voxels': 1811}
    ranks = basins.ranks()
    assert set(np.unique(ranks[:, :, :15])) == {0, 1} and set(np.unique(ranks[:, :, 15:])) == {0, 2}, "cut between x = 14 and x = 15"
    want = split_texels(a, 100, 255)
    assert np.array_equal(ranks, want[0]) and basins.list() == want[1]
    # the emitters speak of the original volume, not of its depth
    second = basins.keep(2, 2)
    assert np.array_equal(whole(second), np.where(ranks == 2, a, 0)) and set(np.unique(whole(second))) == {0, 200}
    assert np.array_equal(basins.measure(), measure_texels(ranks, a))
    second.destroy(); basins.destroy()
    for h in (0, 1, 4, 8):
        basins, profile = v.split_timed(100, 255, h)
        assert basins.list() == [(9, 8, 2, 924), (19, 8, 2, 887)], h
        assert set(profile['ms']) == {'classify', 'plateau', 'links'}
        basins.destroy()
    assert whole(v).tobytes() == a.tobytes()
    v.destroy()
    # the nearer pair: the saddle survives hmax up to h = 2
    v = upload(gpu_ctx, two_balls(17))
    for h, sizes in ((0, [887, 818]), (1, [887, 818]), (2, [887, 818]), (4, [1705]), (8, [1705])):
        basins = v.split(100, 255, h)
        assert [b[3] for b in basins.list()] == sizes, h
        basins.destroy()
    v.destroy()
