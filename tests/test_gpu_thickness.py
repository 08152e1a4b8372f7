"""GPU: local thickness, the largest inscribed ball (vpt_distance_thickness) on the device.

Every T2 is held, byte for byte, to vpt_amd.thickness_squared_texels, the numpy statement of the contract (tests/test_thickness_host.py holds
that to a loop over the centres).

A wave owns an output tile of 8 x 8 x 4 voxels and walks the list of centre tiles 64 entries a step.  The shapes are the smallest at which
that can go wrong: one voxel; a row; 9 x 13 x 21 and 67 x 9 x 5, which no tile divides on any axis; a ball of radius 18 in 96 x 40 x 24 that
crosses many tiles (360 of them: several steps of the walk) and leaves the volume through its faces; two overlapping balls of unequal radii;
plates with the closed-form answer; no seed and all seeds."""
import ctypes as C
import functools

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.distance import NONE, channel_texels, distance_squared_texels, thickness_squared_texels, thickness_texels, open_ball_texels, within_texels
from vpt_amd.measure import measure_texels
from vpt_amd.watershed import split_texels

from test_gpu_pyramid import upload, whole

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.uint16)
SEEDS = ('rest', 'range')


def ball(shape, centre, radius):
    z, y, x = np.indices(shape)
    return (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= radius * radius


def blobs(shape, seed):
    """a few balls of radius 1 .. 5 at random centres, some cut by the border"""
    rng = np.random.default_rng(seed)
    mask = np.zeros(shape, bool)
    for _ in range(6):
        mask |= ball(shape, [rng.integers(0, n) for n in shape], rng.uniform(1.0, 5.0))
    return mask


def plate(shape, axis, first, w):
    mask = np.zeros(shape, bool)
    index = [slice(None)] * 3
    index[axis] = slice(first, first + w)
    mask[tuple(index)] = True
    return mask


def row():
    mask = np.zeros((1, 1, 37), bool)
    for first, n in ((0, 3), (5, 1), (8, 11), (22, 6), (30, 7)):
        mask[0, 0, first:first + n] = True
    return mask


# name -> the structure, [depth][height][width] bool
CASES = {
    'voxel': lambda: np.ones((1, 1, 1), bool),
    'row': row,
    '9x13x21': lambda: blobs((21, 13, 9), 3),
    '67x9x5': lambda: blobs((5, 9, 67), 4),
    'cut ball': lambda: ball((24, 40, 96), (10, 17, 17), 18),                            # leaves through x = 0, y = 0 and both z faces
    'two balls': lambda: ball((20, 30, 40), (9, 12, 12), 9) | ball((20, 30, 40), (11, 16, 24), 6),
    'plate 1': lambda: plate((11, 10, 12), 0, 4, 1),
    'plate 2': lambda: plate((11, 10, 12), 1, 3, 2),
    'plate 5': lambda: plate((11, 10, 12), 2, 6, 5),
    'plate 6': lambda: plate((11, 10, 12), 0, 2, 6),
    'no structure': lambda: np.zeros((21, 13, 9), bool),
    'all structure': lambda: np.ones((21, 13, 9), bool),
}
PLATES = {'plate 1': 1, 'plate 2': 2, 'plate 5': 5, 'plate 6': 6}
THREE = ('9x13x21', 'two balls', 'plate 5')


def window(dtype):
    M = int(np.iinfo(dtype).max)
    return M // 2 + 1, M


@functools.lru_cache(maxsize=None)
def texels(name, dtype):
    """the structure in codes of the upper half, the rest in codes of the lower half: the snapshot is not constant on either"""
    mask = CASES[name]()
    rng = np.random.default_rng(len(name))
    lo, hi = window(dtype)
    a = np.where(mask, rng.integers(lo, hi + 1, size=mask.shape), rng.integers(0, lo, size=mask.shape)).astype(dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def statement(name, seeds):
    """(D, T2) of a case: computed once, shared by every test, never written to"""
    lo, hi = window(np.uint8)
    d2 = distance_squared_texels(texels(name, np.uint8), lo, hi, seeds)
    t2 = thickness_squared_texels(d2)
    d2.setflags(write=False); t2.setflags(write=False)
    return d2, t2


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d values differ, first at [z, y, x] = %s: %d, expected %d" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def capped(d, flags):
    """(the thickness handle, visited) of vpt_distance_thickness_capped"""
    t, report = d.thickness_timed(_flags=flags)
    return t, report['visited']


# ---- the result, its info, the source afterwards -------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("seeds", SEEDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", list(CASES))
def test_thickness_equals_the_statement(gpu_ctx, name, dtype, seeds):
    a = texels(name, dtype)
    lo, hi = window(dtype)
    d2, t2 = statement(name, seeds)
    what = "%s %s %s" % (name, np.dtype(dtype).name, seeds)
    v = upload(gpu_ctx, a)
    d = v.distance(lo, hi, seeds)
    same(d.squared(), d2, what + ": the distances")
    t = d.thickness()
    try:
        same(t.squared(), t2, what)
        finite = t2[t2 != NONE]
        assert t.info == {'seeds': int(np.count_nonzero(d2 == 0)), 'largest': int(finite.max()) if finite.size else 0}, what
        assert t.info == d.info, what
        assert list(t.profile().values()) == [0.0, 0.0, 0.0], what
        same(d.squared(), d2, what + ": the source afterwards")
        # a box that starts and ends inside the volume
        dz, dy, dx = (n // 3 for n in a.shape)
        same(t.squared(dx, dy, dz, a.shape[2] - dx, a.shape[1] - dy, a.shape[0] - dz), np.ascontiguousarray(t2[dz:, dy:, dx:]), what + ": a box")
    finally:
        t.destroy(); d.destroy(); v.destroy()
    if name in PLATES and seeds == 'rest':
        mask = CASES[name]()
        half = (PLATES[name] + 1) // 2
        assert np.array_equal(t2, np.where(mask, half * half, 0)), what


# ---- the emitters ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("seeds", SEEDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", ('67x9x5', 'two balls', 'no structure'))
def test_within_and_channel_of_the_result(gpu_ctx, name, dtype, seeds):
    a = texels(name, dtype)
    lo, hi = window(dtype)
    _, t2 = statement(name, seeds)
    v = upload(gpu_ctx, a, 'nearest')
    d = v.distance(lo, hi, seeds)
    t = d.thickness()
    d.destroy(); v.destroy()                                     # the result owns what it needs
    try:
        for r2_lo, r2_hi, fill in ((0, None, 0), (10, None, 7), (17, 40, 0), (1, NONE - 1, 3), (NONE, None, 1)):
            out = t.within(r2_lo, r2_hi, fill)
            same(whole(out), within_texels(a, t2, r2_lo, r2_hi, fill), "%s within %r" % (name, (r2_lo, r2_hi, fill)))
            assert out.modality['internalFormat'] == v.modality['internalFormat']
            out.destroy()
        for steps in (1, 2, 256):
            out = t.channel(steps)
            same(whole(out), channel_texels(a, t2, steps), "%s channel %d" % (name, steps))
            out.destroy()
    finally:
        t.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_volume_thickness_and_open_ball(gpu_ctx, dtype):
    a = texels('two balls', dtype)
    lo, hi = window(dtype)
    v = upload(gpu_ctx, a)
    for steps, seeds in ((2, 'rest'), (3, 'range')):
        out = v.thickness(lo, hi, steps, seeds)
        same(whole(out), thickness_texels(a, lo, hi, steps, seeds), "thickness %d %s" % (steps, seeds))
        out.destroy()
    out = v.thickness(lo, hi)
    same(whole(out), thickness_texels(a, lo, hi), "thickness by default")
    out.destroy()
    for radius, fill in ((0, 0), (5.5, 0), (7, 9), (9, 0)):
        out = v.open_ball(lo, hi, radius, fill)
        want = open_ball_texels(a, lo, hi, radius, fill)
        same(whole(out), want, "open_ball %r" % (radius,))
        out.destroy()
    # the opening by the ball of radius 7 drops the smaller ball but for what the larger one covers, and keeps the larger one whole
    opened = open_ball_texels(a, lo, hi, 7) >= lo
    large, small = ball(a.shape, (9, 12, 12), 9), ball(a.shape, (11, 16, 24), 6)
    assert opened[large].all() and not opened[small & ~large].all() and not opened[~(large | small)].any()
    assert whole(v).tobytes() == a.tobytes(), "the source changed"
    v.destroy()


@pytest.mark.timeout(120)
def test_measure_takes_the_thickness_channel_as_values(gpu_ctx):
    a = texels('two balls', np.uint8)
    lo, hi = window(np.uint8)
    v = upload(gpu_ctx, a)
    basins = v.split(lo, hi)
    values = v.thickness(lo, hi, 2)
    try:
        ranks, listed = split_texels(a, lo, hi)
        assert len(listed) == 2
        want = measure_texels(ranks, thickness_texels(a, lo, hi, 2)[..., 1])
        got = basins.measure(values=values, channel=1)
        assert np.array_equal(got, want)
        # the larger ball's diameter in voxels, floor(2 sqrt(82)); the smaller one's basin holds voxels the larger ball covers
        assert [int(r) for r in got['value_max']] == [18, 18], got['value_max']
    finally:
        values.destroy(); basins.destroy(); v.destroy()


# ---- the culls change nothing; two runs; the source may go -----------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("seeds", SEEDS)
@pytest.mark.parametrize("name", THREE)
def test_the_culls_change_no_byte(gpu_ctx, name, seeds):
    a = texels(name, np.uint8)
    lo, hi = window(np.uint8)
    _, t2 = statement(name, seeds)
    v = upload(gpu_ctx, a)
    d = v.distance(lo, hi, seeds)
    visited = {}
    try:
        for flags in (0, 1, 2, 3):
            t, visited[flags] = capped(d, flags)
            got = t.squared()
            t.destroy()
            same(got, t2, "%s %s flags %d" % (name, seeds, flags))
        assert visited[0] <= visited[1] <= visited[3] and visited[0] <= visited[2] <= visited[3], visited
        # without either cull every listed tile runs over every listed tile
        t, report = d.thickness_timed()
        t.destroy()
        assert report['visited'] == visited[0] and visited[3] == report['tiles'] ** 2, (report, visited)
        assert all(ms >= 0.0 for ms in report['ms'].values()) and report['ms']['cover'] > 0.0, report
    finally:
        d.destroy(); v.destroy()


@pytest.mark.timeout(120)
def test_two_runs_give_identical_bytes_and_the_source_may_be_destroyed(gpu_ctx):
    a = texels('cut ball', np.uint16)
    lo, hi = window(np.uint16)
    v = upload(gpu_ctx, a)
    d = v.distance(lo, hi, 'rest')
    first, second = d.thickness(), d.thickness()
    d.destroy(); v.destroy()
    try:
        assert first.squared().tobytes() == second.squared().tobytes() == statement('cut ball', 'rest')[1].tobytes()
        again = first.thickness()                                # a thickness handle is a distance handle: its balls cover what they covered
        assert np.array_equal(again.squared() >= first.squared(), np.ones(a.shape, bool))
        again.destroy()
    finally:
        first.destroy(); second.destroy()


# ---- errors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_error_returns(gpu_ctx):
    lib = N.lib()
    a = texels('9x13x21', np.uint8)
    v = upload(gpu_ctx, a)
    d = v.distance(*window(np.uint8), 'rest')
    h, ms, tiles, visited = C.c_void_p(), (C.c_double * N.THICKNESS_PHASES)(), C.c_uint64(0), C.c_uint64(0)
    try:
        assert lib.vpt_distance_thickness(None, C.byref(h)) == N.ERR_INVALID
        assert lib.vpt_distance_thickness(d._handle(), None) == N.ERR_INVALID
        assert lib.vpt_distance_thickness_timed(d._handle(), C.byref(h), None, C.byref(tiles), C.byref(visited)) == N.ERR_INVALID
        assert lib.vpt_distance_thickness_timed(d._handle(), C.byref(h), ms, None, C.byref(visited)) == N.ERR_INVALID
        assert lib.vpt_distance_thickness_timed(d._handle(), C.byref(h), ms, C.byref(tiles), None) == N.ERR_INVALID
        assert lib.vpt_distance_thickness_timed(None, C.byref(h), ms, C.byref(tiles), C.byref(visited)) == N.ERR_INVALID
        for flags in (4, -1, 1 << 16):
            assert lib.vpt_distance_thickness_capped(d._handle(), flags, C.byref(h), None, None) == N.ERR_INVALID
            assert b'flags' in lib.vpt_last_error()
        assert lib.vpt_distance_thickness_capped(None, 0, C.byref(h), None, None) == N.ERR_INVALID
        assert not h.value
        # ms and visited may be null
        assert lib.vpt_distance_thickness_capped(d._handle(), 3, C.byref(h), None, None) == N.OK and h.value
        assert lib.vpt_distance_destroy(h) == N.OK
        with pytest.raises(ValueError):
            v.open_ball(*window(np.uint8), -1.0)
        with pytest.raises(ValueError):
            v.thickness(*window(np.uint8), 0)
        t = d.thickness()
        t.destroy()
        with pytest.raises(RuntimeError):
            t.thickness()
    finally:
        d.destroy(); v.destroy()
