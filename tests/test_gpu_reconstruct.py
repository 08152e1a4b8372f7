"""GPU: grey-level morphological reconstruction (vpt_volume_reconstruct) and the geodesic operations (vpt_volume_geodesic) on the device.

Every texel is held, byte for byte, to vpt_amd.reconstruct_texels / geodesic_texels, the numpy statements of the contract
(tests/test_reconstruct_host.py holds those to a best-first path search over Python integers).

The propagation kernel's workgroup owns a tile of 64 x 8 x 4 voxels with a one-voxel rim and is launched again over the tiles whose
surroundings rose.  The shapes are the smallest at which that can go wrong: one voxel; a run shorter than a wave; odd everywhere; exactly one
tile; one voxel more on every axis (a second, one-voxel-thick tile along each); (130, 17, 9), three tiles on every axis, so face, edge and
corner neighbours all exist; and 4000 x 3 x 3, a long run of tiles on one axis."""
import ctypes as C

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.reconstruct import reconstruct_texels, geodesic_texels
from vpt_amd.components import components_texels
from vpt_amd.distance import distance_squared_texels, channel_texels
from vpt_amd.synthetic import colour_tf

from test_gpu_volume_formats import render, same
from test_gpu_pyramid import upload, whole
from reconstruct_cases import CONNECTIVITIES, DTYPES, GEODESIC, largest, serpentine, touching, two_balls, value_sets

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1), (5, 1, 1), (7, 5, 3), (64, 8, 4), (65, 9, 5), (130, 17, 9), (4000, 3, 3))
THREE_TILES = (130, 17, 9)


def differences(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d texels differ (%s), first at %s: %d, expected %d" % (len(bad), what, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def taken(out):
    got = whole(out)
    out.destroy()
    return got


# ---- the texels themselves ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_texels_equal_the_contract(gpu_ctx, dtype, shape):
    for name, marker, mask in value_sets(dtype, shape, seed=11 + SHAPES.index(shape)):
        vm, vk = upload(gpu_ctx, marker), upload(gpu_ctx, mask)
        what = "%s %s %s" % (np.dtype(dtype).name, shape, name)
        for c in CONNECTIVITIES:
            for op in ('dilation', 'erosion'):
                differences(taken(vm.reconstruct(vk, op, c)), reconstruct_texels(marker, mask, op, c), "%s %d %s" % (op, c, what))
            for op, h in GEODESIC:
                h = h * (largest(dtype) // 255)
                differences(taken(vk.geodesic(op, h, c)), geodesic_texels(mask, op, h, c), "%s h %d, %d %s" % (op, h, c, what))
        assert whole(vm).tobytes() == marker.tobytes() and whole(vk).tobytes() == mask.tobytes(), "a source changed"
        vm.destroy(); vk.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_two_channel_sources_and_a_mixed_call(gpu_ctx, dtype):
    (_, a, b), (_, p, q) = value_sets(dtype, (65, 9, 5), seed=23)[:2]
    two_a, two_b = np.stack([a, p], axis=-1), np.stack([q, b], axis=-1)
    va, vb, vtwo_a, vtwo_b = upload(gpu_ctx, a), upload(gpu_ctx, b), upload(gpu_ctx, two_a), upload(gpu_ctx, two_b)
    for c in (6, 26):
        for ca in (0, 1):
            for cb in (0, 1):
                want = reconstruct_texels(two_a, two_b, 'dilation', c, ca, cb)
                out = vtwo_a.reconstruct(vtwo_b, 'dilation', c, ca, cb)
                assert out.native_format()[0] == (N.FORMAT_R16 if dtype == np.uint16 else N.FORMAT_R8), "the result has one channel"
                differences(taken(out), want, "channels %d, %d under %d" % (ca, cb, c))
            for op, h in GEODESIC:
                h = h * (largest(dtype) // 255)
                differences(taken(vtwo_a.geodesic(op, h, c, ca)), geodesic_texels(two_a, op, h, c, ca), "%s of channel %d under %d" % (op, ca, c))
        # the marker channel 1 of a two-channel volume, the mask a one-channel volume, and the other way round
        differences(taken(vtwo_a.reconstruct(vb, 'erosion', c, 1, 0)), reconstruct_texels(two_a, b, 'erosion', c, 1, 0), "mixed, marker RG")
        differences(taken(va.reconstruct(vtwo_b, 'dilation', c, 0, 1)), reconstruct_texels(a, two_b, 'dilation', c, 0, 1), "mixed, mask RG")
        differences(taken(va.reconstruct(va, 'dilation', c)), a, "a volume under itself")
    assert whole(vtwo_a).tobytes() == two_a.tobytes() and whole(vtwo_b).tobytes() == two_b.tobytes(), "a source changed"
    for v in (va, vb, vtwo_a, vtwo_b):
        v.destroy()


# ---- across tile corners and edges ----------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_structures_that_touch_only_across_a_tile_corner_or_edge(gpu_ctx, dtype):
    for second, joined_under in (((64, 8, 4), (26,)), ((64, 8, 3), (18, 26))):
        marker, mask = touching(THREE_TILES, dtype, second)
        vm, vk = upload(gpu_ctx, marker), upload(gpu_ctx, mask)
        for c in CONNECTIVITIES:
            got = taken(vm.reconstruct(vk, 'dilation', c))
            differences(got, reconstruct_texels(marker, mask, 'dilation', c), "touching at %s under %d" % (second, c))
            assert got[3, 7, 63] == 150 and got[second[2], second[1], second[0]] == (150 if c in joined_under else 0), (second, c)
            assert np.count_nonzero(got) == (2 if c in joined_under else 1)
        vm.destroy(); vk.destroy()


# ---- the host loop and the in-tile loop -------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_serpentine_across_tiles_takes_many_launches(gpu_ctx, dtype):
    marker, mask, _ = serpentine((130, 17, 1), dtype)
    want = reconstruct_texels(marker, mask, 'dilation', 6)
    assert want.tobytes() == mask.tobytes()
    vm, vk = upload(gpu_ctx, marker), upload(gpu_ctx, mask)
    out, profile = vm.reconstruct_timed(vk, 'dilation', 6)
    differences(taken(out), want, "serpentine")
    print("serpentine 130 x 17 x 1: %d launches, %d tile runs, %.3f ms" % (profile['launches'], profile['tile_runs'], profile['ms']))
    assert profile['launches'] > 2 and profile['ms'] > 0.0
    assert profile['launches'] <= profile['tile_runs'] < profile['launches'] * 9, "later launches take the dirty tiles only"
    # by erosion: the complement
    M = largest(dtype)
    out = upload(gpu_ctx, M - marker)
    inv = upload(gpu_ctx, M - mask)
    differences(taken(out.reconstruct(inv, 'erosion', 6)), M - want, "serpentine by erosion")
    for v in (vm, vk, out, inv):
        v.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_a_serpentine_inside_one_tile_whatever_the_round_cap(gpu_ctx, dtype):
    marker, mask, length = serpentine((64, 8, 4), dtype)
    vm, vk = upload(gpu_ctx, marker), upload(gpu_ctx, mask)
    out, profile = vm.reconstruct_timed(vk, 'dilation', 6)
    differences(taken(out), mask, "serpentine in a tile")
    assert profile['launches'] == 1, "one tile settles in LDS"
    for rounds in (1, 3):
        out, capped = vm.reconstruct_timed(vk, 'dilation', 6, _tile_rounds=rounds)
        differences(taken(out), mask, "serpentine in a tile, %d rounds a launch" % rounds)
        print("tile_rounds %d: %d launches for a path of %d voxels" % (rounds, capped['launches'], length))
        assert capped['launches'] > profile['launches']
    vm.destroy(); vk.destroy()


# ---- what the result is ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_two_runs_give_identical_bytes_and_the_result_is_an_ordinary_volume(gpu_ctx):
    _, marker, mask = value_sets(np.uint8, THREE_TILES, seed=31)[1]
    vm, vk = upload(gpu_ctx, marker), upload(gpu_ctx, mask)
    first, second = vm.reconstruct(vk, 'dilation', 18), vm.reconstruct(vk, 'dilation', 18)
    assert whole(first).tobytes() == whole(second).tobytes()
    again = first.hmax(30, 26)                                    # every volume operation takes it, this one included
    differences(taken(again), geodesic_texels(whole(first), 'hmax', 30, 26), "hmax of a reconstruction")
    opened = first.open()
    assert whole(opened).shape == mask.shape
    for v in (vm, vk, first, second, opened):
        v.destroy()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_result_renders_like_the_volume_uploaded_from_the_statement(gpu_ctx, dtype):
    z, y, x = np.mgrid[0:33, 0:40, 0:70]
    field = 90 + 60 * np.sin(x / 5.0) * np.cos(y / 4.0) + 50 * np.cos(z / 3.0) + 25 * np.sin((x + y + z) / 2.0)
    v = np.clip(field, 0, 255).astype(np.uint8)
    if dtype == np.uint16:
        v = v.astype(np.uint16) * 257
    h = 40 * (largest(dtype) // 255)
    tf = colour_tf(256)
    for filt in ('linear', 'nearest'):
        src = upload(gpu_ctx, v, filt)
        for op in ('hmax', 'fill_holes'):
            want = geodesic_texels(v, op, h if op == 'hmax' else 0, 26)
            assert len(np.unique(want)) >= 32 and want.tobytes() != v.tobytes(), "degenerate input"
            derived, twin = src.geodesic(op, h if op == 'hmax' else 0, 26), upload(gpu_ctx, want, filt)      # the result carries the source's filter
            for kind in ('mip', 'mcm'):
                fa = render(gpu_ctx, derived, kind, tf=tf)
                same(fa, render(gpu_ctx, twin, kind, tf=tf), '%s %s %s' % (op, kind, filt))
                pixels = np.ascontiguousarray(fa[-1]); pixels = pixels.reshape(-1, pixels.shape[-1])
                assert len(np.unique(pixels.view(np.uint16), axis=0)) >= 2, '%s: empty frame' % kind
            derived.destroy(); twin.destroy()
        src.destroy()


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
    a16 = upload(gpu_ctx, np.zeros((3, 4, 5), dtype=np.uint16))
    f32 = upload(gpu_ctx, np.zeros((3, 4, 5), dtype=np.float32))
    s8 = upload(gpu_ctx, np.zeros((3, 4, 5), dtype=np.int8))
    other_ctx = vpt_amd.Context(0)
    elsewhere = upload(other_ctx, np.zeros((3, 4, 5), dtype=np.uint8))
    out = C.c_void_p()
    rec = lambda m, mc, k, kc, op=0, c=6: (lambda: N.check(L.vpt_volume_reconstruct(m.texture, mc, k.texture, kc, op, c, C.byref(out))))
    geo = lambda s, ch, op, h=0, c=6: (lambda: N.check(L.vpt_volume_geodesic(s.texture, ch, op, h, c, C.byref(out))))
    refused(rec(f32, 0, a8, 0), N.ERR_UNSUPPORTED, 'marker', 'R32F')
    refused(rec(a8, 0, s8, 0), N.ERR_UNSUPPORTED, 'mask', 'R8_SNORM')
    refused(geo(f32, 0, 0), N.ERR_UNSUPPORTED, 'R32F')
    refused(rec(a8, 2, a8, 0), N.ERR_INVALID, 'channel 2')
    refused(rec(a8, 0, a8, 1), N.ERR_INVALID, 'channel 1', 'R8')
    refused(geo(a8, 1, 0), N.ERR_INVALID, 'channel 1')
    refused(geo(a8, -1, 0), N.ERR_INVALID, 'channel -1')
    refused(rec(a8, 0, elsewhere, 0), N.ERR_INVALID, 'two contexts')
    refused(rec(a8, 0, b8, 0), N.ERR_INVALID, '5x4x3', '6x4x3')
    refused(rec(a8, 0, a16, 0), N.ERR_UNSUPPORTED, 'R8', 'R16')
    refused(rec(a8, 0, a8, 0, op=2), N.ERR_INVALID, 'op 2')
    for c in (0, 4, 8, 27):
        refused(rec(a8, 0, a8, 0, c=c), N.ERR_INVALID, 'connectivity %d' % c)
        refused(geo(a8, 0, 0, c=c), N.ERR_INVALID, 'connectivity %d' % c)
    refused(geo(a8, 0, 7), N.ERR_INVALID, 'op 7')
    refused(geo(a8, 0, -1), N.ERR_INVALID, 'op -1')
    for op, name in ((0, 'FILL_HOLES'), (1, 'CLEAR_BORDER'), (5, 'MAXIMA'), (6, 'MINIMA')):
        refused(geo(a8, 0, op, h=1), N.ERR_INVALID, name)
    for op in (2, 3, 4):
        refused(geo(a8, 0, op, h=256), N.ERR_INVALID, '256', '255')
        refused(geo(a16, 0, op, h=65536), N.ERR_INVALID, '65536', '65535')
    for rounds in (0, -3):
        refused(lambda: N.check(L.vpt_volume_reconstruct_capped(a8.texture, 0, a8.texture, 0, 0, 6, rounds, C.byref(out), None, None)), N.ERR_INVALID,
                'tile_rounds %d' % rounds)
    assert not out.value, "a refused call hands nothing out"
    # the host checks refuse the same before the library is asked
    for call in (lambda: a8.reconstruct(a8, 'opening'), lambda: a8.reconstruct(a8, connectivity=7), lambda: a8.reconstruct(a8, channel=1),
                 lambda: a8.geodesic('watershed'), lambda: a8.hmax(256), lambda: a8.fill_holes(connectivity=5), lambda: a8.geodesic('maxima', 1),
                 lambda: a8.reconstruct(None)):
        with pytest.raises(ValueError):
            call()
    for v in (a8, b8, a16, f32, s8, elsewhere):
        v.destroy()
    other_ctx.destroy()


# ---- the worked example of the contract, end to end on the device -------------------------------------------------------------------
def seeds_on_the_device(ctx, second_x, h):
    """(components of the thresholded balls, components of the regional maxima of hmax_h of their depth channel), all on the device"""
    v = upload(ctx, two_balls(second_x))
    whole_structure = v.components(100, 255, 26)
    structures = whole_structure.info['listed']
    whole_structure.destroy()
    d = v.distance(100, 255, 'rest')
    depth = d.channel(steps=4)
    d.destroy()
    flattened = depth.hmax(h, 26, channel=1)
    maxima = flattened.regional_maxima(26)
    found = maxima.components(255, 255, 26)
    seeds = found.info['listed']
    found.destroy()
    for vol in (v, depth, flattened, maxima):
        vol.destroy()
    return structures, seeds


@pytest.mark.timeout(120)
def test_two_overlapping_balls_are_one_component_and_two_seeds(gpu_ctx):
    for h in (0, 1, 2, 4, 8):
        assert seeds_on_the_device(gpu_ctx, 19, h) == (1, 2), h
    for h, seeds in ((0, 2), (1, 2), (2, 2), (4, 1), (8, 1)):
        assert seeds_on_the_device(gpu_ctx, 17, h) == (1, seeds), h
    # and the device's texels are the statement's
    a = two_balls(19)
    depth = channel_texels(a, distance_squared_texels(a, 100, 255, 'rest'), 4)
    want = geodesic_texels(geodesic_texels(depth, 'hmax', 2, 26, 1), 'maxima', 0, 26)
    assert len(components_texels(want, 255, 255, 26)[1]) == 2
    v = upload(gpu_ctx, depth)
    flattened = v.hmax(2, 26, channel=1)
    differences(taken(flattened.regional_maxima(26)), want, "maxima of the depth channel")
    flattened.destroy(); v.destroy()
