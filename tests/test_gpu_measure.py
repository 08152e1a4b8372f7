"""GPU: per-component measurements of a labelling (vpt_components_measure) and the selection by a set of ranks
(vpt_components_keep_set) on the device.

The records are held, field for field, to vpt_amd.measure_texels and the kept volumes, byte for byte, to vpt_amd.keep_set_texels: the numpy
statements of the contract (tests/test_measure_host.py holds those to a loop in Python integers).  The ranks come from
vpt_amd.components_texels, which tests/test_gpu_components.py holds the device's labelling to.

The measuring kernel's workgroup owns a box of 64 x 8 x 8 voxels (MS_BX, MS_BY, MS_BZ in vpt_volume_measure.hip), a wave takes 64
consecutive voxels of a row, and the workgroup's LDS table has 512 slots (MS_SLOTS); the set emitter is a grid-stride loop over groups of
four voxels.  So the shapes that matter are one voxel past the box on every axis (two boxes an axis; with nx % 4 != 0 and == 0), one voxel
past two boxes (a box with neighbours on both sides, for the faces), a row longer than 128 voxels (a run that crosses two wave boundaries)
and a box that holds more distinct ranks than the table has slots (the 3-D checkerboard: half of the box's 4096 voxels)."""
import ctypes as C
import functools

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.measure import MEASURE_DTYPE

from test_gpu_components import noise, noise_range, differences, FRACTION
from test_gpu_volume_formats import render, same
from test_gpu_pyramid import upload, whole

pytestmark = pytest.mark.gpu

BOX = (64, 8, 8)                                                    # nx, ny, nz of a measuring box
SLOTS = 512                                                         # of a workgroup's table
BX, BY, BZ = BOX
NOISE = (23, 19, 21)
PLUS_ONE = (BX + 1, BY + 1, BZ + 1)                                 # nx % 4 != 0
PLUS_ONE_4 = (BX + 4, BY + 1, BZ + 1)                               # the same, nx % 4 == 0
TWO_BOXES = (2 * BX + 1, 2 * BY + 1, 2 * BZ + 1)
LONG_ROW = (3 * 64 + 7, 3, 2)                                       # a row of three waves and a rest
SHAPES = ((1, 1, 1), (7, 5, 1), (17, 1, 3), (1, 3, 17), NOISE, PLUS_ONE, PLUS_ONE_4, TWO_BOXES, LONG_ROW)
DTYPES = (np.uint8, np.uint16)


@functools.lru_cache(maxsize=None)
def labelled(dtype, shape, connectivity, seed, min_voxels=1):
    """(texels, ranks, list) of seeded noise: computed once, shared, never written to"""
    a = noise(dtype, shape, seed)
    lo, hi = noise_range(dtype, connectivity)
    ranks, listed = vpt_amd.components_texels(a, lo, hi, connectivity, min_voxels)
    for x in (a, ranks):
        x.setflags(write=False)
    return a, ranks, listed, lo, hi


def compare(got, want, what):
    assert got.dtype == want.dtype == MEASURE_DTYPE and got.shape == want.shape, what
    for name in MEASURE_DTYPE.names:
        bad = np.flatnonzero(got[name] != want[name])
        assert len(bad) == 0, "%s: %d records differ in %s, first %d: %d, expected %d" % (what, len(bad), name, bad[0], got[name][bad[0]], want[name][bad[0]])


def identities(records, listed, what):
    assert [int(v) for v in records['voxels']] == [c[3] for c in listed], what + ': voxels are the list\'s'
    roots = np.array([c[:3] for c in listed], np.int64).reshape(-1, 3)
    assert (records['min_x'] <= roots[:, 0]).all() and (roots[:, 0] <= records['max_x']).all() and (records['min_y'] <= roots[:, 1]).all() \
        and (roots[:, 1] <= records['max_y']).all() and (records['min_z'] == roots[:, 2]).all(), what + ': the root lies in the box, root_z = min_z'


def windows(listed):
    n = len(listed)
    return [(0, 1), (n - 1, 1), (n // 3, n // 2), (0, n), (n, 0), (1, 0)] if n else [(0, 0)]


def check(ctx, a, ranks, listed, lo, hi, connectivity, min_voxels=1, what=''):
    """labels `a` on the device, measures it under itself and holds the records and every window to the statement"""
    what = "%s %s %s c%d m%d" % (what, a.dtype.name, a.shape[::-1], connectivity, min_voxels)
    src = upload(ctx, a)
    found = src.components(lo, hi, connectivity, min_voxels)
    assert found.list() == listed, what + ': the labelling'
    want = vpt_amd.measure_texels(ranks, a, 0, len(listed))          # (n given: a rank the noise does not reach is still a window error)
    got = found.measure()
    compare(got, want, what)
    identities(got, listed, what)
    for first, n in windows(listed):
        compare(found.measure(first, n), want[first:first + n], what + ' window (%d, %d)' % (first, n))
    assert whole(src).tobytes() == a.tobytes(), what + ": the source's texels changed"
    found.destroy(); src.destroy()
    return got


# ---- noise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("connectivity", (6, 18, 26))
def test_noise_records_equal_the_statement(gpu_ctx, connectivity, dtype):
    for k, shape in enumerate(SHAPES):
        a, ranks, listed, lo, hi = labelled(dtype, shape, connectivity, 101 + k)
        check(gpu_ctx, a, ranks, listed, lo, hi, connectivity, what='noise')
        if shape in (PLUS_ONE, TWO_BOXES):
            assert len(listed) >= 64, "degenerate input: %d components" % len(listed)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES)
def test_dropped_components_lie_next_to_listed_ones(gpu_ctx, dtype):
    a, ranks, listed, lo, hi = labelled(dtype, PLUS_ONE, 6, 131, 3)
    everything = vpt_amd.components_texels(a, lo, hi, 6)[1]
    assert 8 <= len(listed) < len(everything) and listed[-1][3] >= 3
    # a dropped voxel (rank 0, foreground) across an edge from a listed one (across a face the two would be one component)
    fg = (a >= lo) & (a <= hi)
    assert ((ranks[:, 1:, 1:] > 0) & (ranks[:, :-1, :-1] == 0) & fg[:, :-1, :-1]).any(), "degenerate input: no dropped voxel beside a listed one"
    check(gpu_ctx, a, ranks, listed, lo, hi, 6, 3, what='min 3')


# ---- constructed cases -------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("shape", (PLUS_ONE, PLUS_ONE_4, TWO_BOXES))
def test_one_component_that_every_block_adds_to(gpu_ctx, shape):
    nx, ny, nz = shape
    for dtype, code in ((np.uint8, 9), (np.uint16, 65535)):
        a = np.full((nz, ny, nx), code, dtype)
        got = check(gpu_ctx, a, np.ones(a.shape, np.uint32), [(0, 0, 0, nx * ny * nz)], code, code, 6, what='all foreground')
        assert len(got) == 1 and int(got[0]['faces']) == 2 * (nx * ny + ny * nz + nx * nz)
        assert int(got[0]['value_sum_sq']) == nx * ny * nz * code * code and int(got[0]['sum_x']) == ny * nz * nx * (nx - 1) // 2


@pytest.mark.timeout(120)
def test_checkerboard_overflows_the_table(gpu_ctx):
    assert BX * BY * BZ // 2 > SLOTS, "a box of the checkerboard must hold more distinct ranks than the table has slots"
    nx, ny, nz = PLUS_ONE
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    board = np.where((x + y + z) % 2 == 0, 200, 0).astype(np.uint8)
    n = (nx * ny * nz + 1) // 2
    ranks = np.zeros(board.shape, np.uint32)
    ranks[board == 200] = np.arange(1, n + 1, dtype=np.uint32)        # singletons: size ties are listed by root, the linear index
    listed = [(int(c), int(b), int(a), 1) for a, b, c in zip(*np.nonzero(board == 200))]
    got = check(gpu_ctx, board, ranks, listed, 200, 255, 6, what='checkerboard')
    assert len(got) == n and (got['faces'] == 6).all() and (got['voxels'] == 1).all() and (got['value_sum'] == 200).all()
    assert (got['min_x'] == got['max_x']).all() and (got['sum_x'] == got['min_x']).all()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("shape", (PLUS_ONE, TWO_BOXES))
def test_alternate_rows_and_alternate_planes(gpu_ctx, shape):
    nx, ny, nz = shape
    rng = np.random.default_rng(137)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    for name, inside in (('rows', (y % 2 == 0) & (z % 2 == 0)), ('planes', z % 2 == 0)):
        a = np.where(inside, rng.integers(1, 65536, size=inside.shape), 0).astype(np.uint16)
        ranks, listed = vpt_amd.components_texels(a, 1, 65535, 6)
        assert len(listed) == (((ny + 1) // 2) * ((nz + 1) // 2) if name == 'rows' else (nz + 1) // 2)
        got = check(gpu_ctx, a, ranks, listed, 1, 65535, 6, what=name)
        if name == 'rows':
            assert (got['voxels'] == nx).all() and (got['faces'] == 4 * nx + 2).all() and (got['min_y'] == got['max_y']).all()
        else:
            assert (got['voxels'] == nx * ny).all() and (got['faces'] == 2 * nx * ny + 2 * nx + 2 * ny).all() and (got['min_z'] == got['max_z']).all()


# ---- the measured volume -----------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_values_of_either_width_and_two_channels(gpu_ctx):
    shape = PLUS_ONE
    nx, ny, nz = shape
    L = N.lib()
    for dtype in DTYPES:
        a, ranks, listed, lo, hi = labelled(dtype, shape, 6, 139)
        other = np.uint16 if dtype == np.uint8 else np.uint8
        src = upload(gpu_ctx, a)
        found = src.components(lo, hi, 6)
        src.destroy()                                              # the labelled source goes before anything is measured
        n = len(listed)
        compare(found.measure(values=None), vpt_amd.measure_texels(ranks, a, 0, n), 'values None')
        cases = [('the other width', noise(other, shape, 149), 0), ('all 0', np.zeros(a.shape, np.uint8), 0), ('all 65535', np.full(a.shape, 65535, np.uint16), 0)]
        rg16 = np.stack([noise(np.uint16, shape, 151), noise(np.uint16, shape, 157)], axis=-1)
        rg8 = np.stack([noise(np.uint8, shape, 163), noise(np.uint8, shape, 167)], axis=-1)
        cases += [('RG16 channel 1', rg16, 1), ('RG8 channel 0', rg8, 0), ('RG8 channel 1', rg8, 1), ('RG16 channel 0', rg16, 0)]
        for name, texels, channel in cases:
            vol = upload(gpu_ctx, texels)
            got = found.measure(values=vol, channel=channel)
            vol.destroy()                                          # right after the call
            plane = texels[..., channel] if texels.ndim == 4 else texels
            compare(got, vpt_amd.measure_texels(ranks, np.ascontiguousarray(plane), 0, n), name)
            if name == 'all 65535':
                assert (got['value_sum_sq'] == got['voxels'] * np.uint64(65535 * 65535)).all() and (got['value_min'] == 65535).all()
            if name == 'all 0':
                assert not got['value_sum'].any() and not got['value_max'].any() and not got['value_min'].any()
        # a volume that has not been finalized: the pass is enqueued behind the upload
        texels = noise(other, shape, 173)
        h = C.c_void_p()
        N.check(L.vpt_volume_create(gpu_ctx._h, nx, ny, nz, N.FORMAT_R16 if other == np.uint16 else N.FORMAT_R8, C.byref(h)))
        N.check(L.vpt_volume_upload_block(h, 0, 0, 0, nx, ny, nz, texels.ctypes.data_as(C.c_void_p), texels.nbytes))      # no vpt_volume_finalize
        got = np.zeros(n, MEASURE_DTYPE)
        N.check(L.vpt_components_measure(found._h, h, 0, 0, n, got.ctypes.data_as(C.POINTER(N.ComponentMeasure))))
        N.check(L.vpt_volume_destroy(h))
        compare(got, vpt_amd.measure_texels(ranks, texels, 0, n), 'not finalized')
        timed, ms = found.measure_timed(2, 5)
        compare(timed, vpt_amd.measure_texels(ranks, a, 2, 5), 'timed')
        assert ms > 0.0
        found.destroy()


@pytest.mark.timeout(120)
def test_two_runs_give_identical_bytes(gpu_ctx):
    a, ranks, listed, lo, hi = labelled(np.uint16, TWO_BOXES, 6, 179)
    src = upload(gpu_ctx, a)
    found = src.components(lo, hi, 6)
    first, second = found.measure(), found.measure()
    assert first.tobytes() == second.tobytes() == vpt_amd.measure_texels(ranks, a, 0, len(listed)).tobytes()
    chosen = list(range(2, len(listed), 3))
    one, two = found.keep_set(chosen, 3), found.keep_set(chosen, 3)
    assert whole(one).tobytes() == whole(two).tobytes()
    assert whole(src).tobytes() == a.tobytes() and found.ranks().tobytes() == ranks.tobytes()
    for thing in (one, two, found, src):
        thing.destroy()


# ---- errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_every_error_of_the_contract(gpu_ctx):
    L = N.lib()
    a = np.zeros((4, 4, 4), np.uint8); a[0, 0, 0] = a[3, 3, 3] = a[3, 3, 2] = 1
    src = upload(gpu_ctx, a)
    found = src.components(1, 1)                                    # two components: 2 voxels and 1
    assert found.list() == [(2, 3, 3, 2), (0, 0, 0, 1)]
    h = found._h
    buf = (N.ComponentMeasure * 4)()
    ms = C.c_double(0)

    def refused(code, words, *args):
        for rc in (L.vpt_components_measure(*args), L.vpt_components_measure_timed(*(args + (C.byref(ms),)))):
            assert rc == code, (args, L.vpt_last_error())
            for word in words:
                assert word.encode() in L.vpt_last_error(), (word, L.vpt_last_error())

    refused(N.ERR_INVALID, ("null",), None, None, 0, 0, 1, buf)
    refused(N.ERR_INVALID, ("null",), h, None, 0, 0, 1, None)           # dst null
    assert L.vpt_components_measure_timed(h, None, 0, 0, 1, buf, None) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    for first, n in ((0, 3), (1, 2), (2, 1), (3, 0), (1 << 63, 1 << 63), (0, 1 << 40)):
        refused(N.ERR_INVALID, ("not within the 2 listed",), h, None, 0, first, n, buf)
        with pytest.raises(ValueError):
            found.measure(first, n)
    assert L.vpt_components_measure(h, None, 0, 2, 0, buf) == N.OK and L.vpt_components_measure(h, None, 0, 1, 0, None) == N.OK      # as vpt_components_list
    for channel in (2, -1, 1):                                     # the snapshot has one channel
        refused(N.ERR_INVALID, ("channel",), h, None, channel, 0, 1, buf)
    for vol, name in ((upload(gpu_ctx, np.zeros((4, 4, 4), np.float32)), "R32F"), (upload(gpu_ctx, np.zeros((4, 4, 4), np.int8)), "R8_SNORM")):
        refused(N.ERR_UNSUPPORTED, (name,), h, vol.texture, 0, 0, 1, buf)
        with pytest.raises(vpt_amd.VptError, match=r"\b%s\b" % name) as e:
            found.measure(values=vol)
        assert e.value.code == N.ERR_UNSUPPORTED
        vol.destroy()
    other_size = upload(gpu_ctx, np.zeros((4, 5, 6), np.uint16))
    refused(N.ERR_INVALID, ("4x4x4", "6x5x4"), h, other_size.texture, 0, 0, 1, buf)
    other_size.destroy()
    one = upload(gpu_ctx, np.zeros((4, 4, 4), np.uint16))
    refused(N.ERR_INVALID, ("channel 1", "R16"), h, one.texture, 1, 0, 1, buf)
    refused(N.ERR_INVALID, ("channel 2",), h, one.texture, 2, 0, 1, buf)
    one.destroy()
    second = vpt_amd.Context(0)
    try:
        elsewhere = upload(second, np.zeros((4, 4, 4), np.uint8))
        refused(N.ERR_INVALID, ("context",), h, elsewhere.texture, 0, 0, 1, buf)
        elsewhere.destroy()
    finally:
        second.destroy()
    with pytest.raises(ValueError):
        found.measure(values=a)
    # keep_set
    out = C.c_void_p()
    ranks = (C.c_uint64 * 3)(1, 0, 2)
    assert L.vpt_components_keep_set(h, ranks, 3, 0, C.byref(out)) == N.ERR_INVALID and b"rank 0" in L.vpt_last_error()
    assert L.vpt_components_keep_set(h, ranks, 1, 256, C.byref(out)) == N.ERR_INVALID and b"fill 256" in L.vpt_last_error()
    assert L.vpt_components_keep_set(h, ranks, 1, 0, None) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    assert L.vpt_components_keep_set(None, ranks, 1, 0, C.byref(out)) == N.ERR_INVALID
    assert L.vpt_components_keep_set(h, None, 1, 0, C.byref(out)) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    for bad, fill in (([0], 0), ([1], 256), ([1], -1), ([1.5], 0), (np.ones(3, bool), 0)):
        with pytest.raises(ValueError):
            found.keep_set(bad, fill)
    found.destroy(); src.destroy()
    with pytest.raises(RuntimeError, match='destroyed'):
        found.measure()
    with pytest.raises(RuntimeError, match='destroyed'):
        found.keep_set([1])


# ---- keep_set ----------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", (NOISE, PLUS_ONE, PLUS_ONE_4))
def test_keep_set_equals_the_statement(gpu_ctx, shape, dtype):
    a, ranks, listed, lo, hi = labelled(dtype, shape, 6, 181)
    n = len(listed)
    M = int(np.iinfo(dtype).max)
    src = upload(gpu_ctx, a, 'nearest')
    found = src.components(lo, hi, 6)
    chosen = (np.random.default_rng(191).permutation(n)[:n // 3] + 1).tolist()
    mask = np.zeros(n, bool); mask[np.array(chosen) - 1] = True
    for name, selected, fill in (('a random subset', chosen, 0), ('the empty set', [], 5), ('ranks above the list', chosen[:4] + [n + 1, n + 77, 1 << 40], M),
                                 ('duplicates', chosen[:5] * 3, 1), ('a boolean mask', mask, 7), ('everything', np.ones(n, bool), 2)):
        out = found.keep_set(selected, fill)
        differences(whole(out), vpt_amd.keep_set_texels(a, ranks, selected, fill), name)
        assert out.ready and out.native_format() == src.native_format() and out.modality['dimensions'] == src.modality['dimensions']
        out.destroy()
    for first, last, fill in ((1, 1, 0), (2, 9, M), (n // 2, n, 3), (1, n, 0)):
        by_set, by_interval = found.keep_set(range(first, last + 1), fill), found.keep(first, last, fill)
        assert whole(by_set).tobytes() == whole(by_interval).tobytes(), ('an interval', first, last, fill)
        by_set.destroy(); by_interval.destroy()
    found.destroy(); src.destroy()


@pytest.mark.timeout(300)
def test_structures_off_the_border_measured_kept_and_rendered(gpu_ctx):
    """measure -> the ranks whose box touches no face of the volume -> keep_set: the volume is held to the statement, its MIP render to the
    render of the uploaded twin"""
    a, ranks, listed, lo, hi = labelled(np.uint8, NOISE, 6, 193)
    nx, ny, nz = NOISE
    src = upload(gpu_ctx, a)
    found = src.components(lo, hi, 6)
    r = found.measure()
    interior = (r['min_x'] > 0) & (r['min_y'] > 0) & (r['min_z'] > 0) & (r['max_x'] < nx - 1) & (r['max_y'] < ny - 1) & (r['max_z'] < nz - 1)
    assert 8 <= interior.sum() < len(listed), "degenerate input"
    kept = found.keep_set(interior)
    want = vpt_amd.keep_set_texels(a, ranks, interior)
    differences(whole(kept), want, 'interior structures')
    border = np.ones(a.shape, bool); border[1:-1, 1:-1, 1:-1] = False
    assert not want[border].any() and want.any()
    twin = upload(gpu_ctx, want)
    same(render(gpu_ctx, kept, 'mip'), render(gpu_ctx, twin, 'mip'), 'interior structures')
    for thing in (kept, twin, found, src):
        thing.destroy()
