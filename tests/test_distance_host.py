"""CPU: the distance transform on the host.  vpt_amd.distance_squared_texels / within_texels / channel_texels (numpy, the statement the
device kernels are held to by tests/test_gpu_distance.py) against a brute force over Python integers (every voxel against every seed),
against scipy.ndimage.distance_transform_edt where scipy is installed, the identities the contract of include/vpt.h implies, the argument
checks of both hosts (the Node ones through js/test/test_distance_host.js, without a device), the option validation of RenderingContext
and the C symbols without a device."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.distance import (NONE, channel_texels, check_radius, check_range, check_seeds, check_steps, check_within, core_texels,
                              distance_squared_texels, isqrt_texels, margin_texels, within_texels)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.uint8, np.uint16)
SEEDS = ('range', 'rest')
# nx, ny, nz: the shapes the formulation of the device's line passes was first checked on
SHAPES = ((23, 19, 21), (1, 1, 1), (65, 3, 2), (129, 2, 3), (1, 70, 1), (1, 1, 70), (7, 5, 1), (130, 9, 5))
DENSITIES = (0.003, 0.05, 0.5)


def noise(dtype, shape, seed):
    nx, ny, nz = shape
    M = int(np.iinfo(dtype).max)
    return np.random.default_rng(seed).integers(0, M + 1, size=(nz, ny, nx)).astype(dtype)


def code_range(dtype, density):
    """(lo, hi): `density` of all codes; for uint16 a range whose ends lie inside a byte and that straddles 0x7FFF / 0x8000"""
    if dtype == np.uint8:
        return 3, 3 + max(int(round(density * 256)) - 1, 0)
    width = max(int(round(density * 65536)), 3)
    lo = 0x8000 - width // 3
    return lo, lo + width - 1


def brute_force(a, lo, hi, seeds):
    """the contract in Python integers: d2 as nested lists"""
    d, h, w = a.shape
    v = a.tolist()
    rest = seeds == 'rest'
    where = [(z, y, x) for z in range(d) for y in range(h) for x in range(w) if (lo <= v[z][y][x] <= hi) != rest]
    return [[[min([(x - sx) ** 2 + (y - sy) ** 2 + (z - sz) ** 2 for sz, sy, sx in where], default=NONE) for x in range(w)] for y in range(h)]
            for z in range(d)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_statement_equals_a_brute_force_over_python_integers(dtype):
    M = int(np.iinfo(dtype).max)
    for n, shape in enumerate(((7, 5, 3), (1, 1, 1), (5, 1, 3), (1, 7, 1), (2, 2, 2))):
        a = noise(dtype, shape, seed=11 + n)
        for lo, hi in (code_range(dtype, 0.05), code_range(dtype, 0.5), (0, M), (0, 0) if dtype == np.uint16 else (1, 2)):
            for seeds in SEEDS:
                d2 = distance_squared_texels(a, lo, hi, seeds)
                assert d2.dtype == np.uint32 and d2.shape == a.shape
                assert d2.tolist() == brute_force(a, lo, hi, seeds), (dtype, shape, lo, hi, seeds)
    assert vpt_amd.distance_squared_texels is distance_squared_texels and vpt_amd.within_texels is within_texels
    assert vpt_amd.channel_texels is channel_texels and vpt_amd.check_seeds is check_seeds and vpt_amd.check_steps is check_steps
    assert vpt_amd.check_radius is check_radius


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seeds", SEEDS)
def test_the_statement_equals_scipys_transform(seeds, dtype):
    ndimage = pytest.importorskip("scipy.ndimage")
    M = int(np.iinfo(dtype).max)
    for n, shape in enumerate(SHAPES):
        a = noise(dtype, shape, seed=23 + n)
        for lo, hi in [code_range(dtype, density) for density in DENSITIES] + [(0, M)]:
            seed = ((a >= lo) & (a <= hi)) != (seeds == 'rest')
            d2 = distance_squared_texels(a, lo, hi, seeds)
            if not seed.any():
                assert (d2 == NONE).all(), (shape, lo, hi)
                continue
            want = np.rint(ndimage.distance_transform_edt(~seed) ** 2).astype(np.uint32)      # the distance to the nearest zero
            assert np.array_equal(d2, want), (dtype, shape, lo, hi, seeds)
    # every density was seen with seeds and, on the larger shapes, with distances beyond one voxel
    a = noise(dtype, SHAPES[0], seed=23)
    assert int(distance_squared_texels(a, *code_range(dtype, 0.003), 'range').max()) > 16


def blobs(shape, seed):
    """uint8 [nz][ny][nx]: the union of five balls of radius 3 .. 7 at code 200 over noise below 50"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 50, size=(nz, ny, nx)).astype(np.uint8)
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    for radius in (3, 4, 5, 6, 7):
        cx, cy, cz = (int(rng.integers(0, n)) for n in shape)
        a[(x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2 <= radius * radius] = 200
    return a


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_identities_the_contract_implies(dtype):
    M = int(np.iinfo(dtype).max)
    a = noise(dtype, (23, 19, 21), seed=31)
    lo, hi = code_range(dtype, 0.05)
    in_range = (a >= lo) & (a <= hi)
    to_range, to_rest = distance_squared_texels(a, lo, hi, 'range'), distance_squared_texels(a, lo, hi, 'rest')
    # TO_REST of a range is TO_RANGE of the complement mask
    mask = np.where(in_range, 0, 1).astype(dtype)
    assert np.array_equal(to_rest, distance_squared_texels(mask, 1, 1, 'range'))
    # 0 exactly on the seeds
    assert np.array_equal(to_range == 0, in_range) and np.array_equal(to_rest == 0, ~in_range)
    # flips and transposes commute with the transform
    for axis in (0, 1, 2):
        assert np.array_equal(distance_squared_texels(np.ascontiguousarray(np.flip(a, axis)), lo, hi), np.flip(to_range, axis))
    for axes in ((1, 0, 2), (2, 1, 0), (0, 2, 1), (1, 2, 0)):
        assert np.array_equal(distance_squared_texels(np.ascontiguousarray(a.transpose(axes)), lo, hi), to_range.transpose(axes))
    # within(0, 0) is the mask
    assert np.array_equal(within_texels(a, to_range, 0, 0), np.where(in_range, a, 0))
    assert np.array_equal(within_texels(a, to_range, 0, 0, M) != M, in_range & (a != M))
    assert np.array_equal(within_texels(a, to_range), a) and np.array_equal(within_texels(a, to_range, 1, None, 7), np.where(in_range, 7, a))
    # NONE is an ordinary value: only r2_hi = 0xFFFFFFFF selects it
    none = np.full(a.shape, NONE, np.uint32)
    assert (within_texels(a, none, 0, NONE - 1, 9) == 9).all() and np.array_equal(within_texels(a, none, NONE, NONE, 9), a)
    # core(r) is inside the structure is inside margin(r), and both are monotone in r
    b = blobs((33, 29, 31), seed=37).astype(dtype)
    structure = b == 200
    before_core, before_margin = structure, structure
    for radius in (0, 1, 1.5, 2, 3.2, 5):
        core, margin = core_texels(b, 200, 200, radius, 0) != 0, margin_texels(b, 200, 200, radius, 1) != 1
        margin |= (b == 1) & (distance_squared_texels(b, 200, 200) <= check_radius(radius))      # a kept code that equals the fill
        assert not (core & ~structure).any() and not (structure & ~margin).any(), radius
        assert not (core & ~before_core).any() and not (before_margin & ~margin).any(), radius
        before_core, before_margin = core, margin
    assert np.array_equal(core_texels(b, 200, 200, 0) != 0, structure) and before_core.any() and not before_margin.all()
    assert int(distance_squared_texels(b, 200, 200, 'rest').max()) >= 25, "degenerate input: no depth"


def test_the_channel_is_the_exact_integer_square_root():
    ks = [1, 2, 3, 255, 256, 257, 4094, 4095]
    values = sorted({v for k in ks for v in (k * k - 1, k * k, k * k + 1)} | {0, 2 * 4095 * 4095, 3 * 4095 * 4095, NONE - 1, NONE})
    d2 = np.array(values, np.uint32).reshape(1, 1, -1)
    for dtype in DTYPES:
        M = int(np.iinfo(dtype).max)
        a = np.arange(d2.size, dtype=dtype).reshape(d2.shape)
        for steps in (1, 2, 7, 255, 256):
            pair = channel_texels(a, d2, steps)
            assert pair.dtype == dtype and pair.shape == d2.shape + (2,) and np.array_equal(pair[..., 0], a)
            assert pair[0, 0, :, 1].tolist() == [min(math.isqrt(steps * steps * v), M) for v in values], (dtype, steps)
        assert channel_texels(a, d2)[0, 0, -1, 1] == M                # NONE gives M
    p = np.array([k * k + e for k in (1, 4095 * 256, (1 << 24) - 1, 1 << 24) for e in (-1, 0, 1)], np.uint64)
    assert isqrt_texels(p).tolist() == [math.isqrt(int(v)) for v in p]


def test_whole_code_compares():
    codes = np.array([0x00FF, 0x0100, 0x7FFF, 0x8000, 0xFF00], np.uint16)
    a = codes[np.random.default_rng(41).integers(0, 5, size=(6, 7, 8))]
    for lo, hi, inside in ((0x0100, 0x8000, (0x0100, 0x7FFF, 0x8000)), (0x00FF, 0x7FFF, (0x00FF, 0x0100, 0x7FFF)), (0x8000, 0xFFFF, (0x8000, 0xFF00))):
        assert np.array_equal(distance_squared_texels(a, lo, hi) == 0, np.isin(a, inside)), (lo, hi)
        assert np.array_equal(distance_squared_texels(a, lo, hi, 'rest') == 0, ~np.isin(a, inside)), (lo, hi)
    # nothing wraps: the last voxel of a row and the first of the next are neighbours in memory, not in the volume
    b = np.zeros((1, 2, 5), np.uint8)
    b[0, 0, 4] = 1
    assert distance_squared_texels(b, 1, 1)[0, 1].tolist() == [17, 10, 5, 2, 1]
    # the border is not background for 'rest'
    assert (distance_squared_texels(np.ones((3, 3, 3), np.uint8), 1, 1, 'rest') == NONE).all()


def test_arguments():
    a = np.zeros((2, 2, 2), np.uint8)
    assert check_seeds('range') == N.DISTANCE_TO_RANGE == 0 and check_seeds('rest') == N.DISTANCE_TO_REST == 1 and N.DISTANCE_NONE == NONE
    for bad in (0, 1, 'both', None, True, b'range'):
        with pytest.raises(ValueError, match='seeds'):
            check_seeds(bad)
        with pytest.raises(ValueError):
            distance_squared_texels(a, 0, 1, bad)
    for lo, hi in ((2, 1), (0, 256), (-1, 5), (0.0, 1), (0, None), (True, 1)):
        with pytest.raises(ValueError):
            distance_squared_texels(a, lo, hi)
    assert check_range(0, 65535, 65535) == (0, 65535)
    with pytest.raises(ValueError):
        distance_squared_texels(np.zeros((2, 2, 2), np.uint16), 0, 65536)
    assert check_steps(1) == 1 and check_steps(256) == 256 and check_steps(np.int32(7)) == 7
    for bad in (0, 257, -1, 1.5, '1', None, True):
        with pytest.raises(ValueError, match='steps'):
            check_steps(bad)
        with pytest.raises(ValueError):
            channel_texels(a, np.zeros((2, 2, 2), np.uint32), bad)
    assert [check_radius(r) for r in (0, 2.5, math.sqrt(2), 3, 65535.9, np.float32(1.5), 65536, 1e200)] == [0, 6, 2, 9, 4294954188, 2, NONE - 1, NONE - 1]
    for bad in (-1, float('nan'), float('inf'), '2', None, True):
        with pytest.raises(ValueError, match='radius'):
            check_radius(bad)
    d2 = np.zeros((2, 2, 2), np.uint32)
    assert check_within(0, None, 0, 255) == (0, NONE, 0)
    for r2_lo, r2_hi, fill in ((2, 1, 0), (-1, 1, 0), (0, 1 << 32, 0), (0, 1, 256), (0, 1, -1), (0.5, 1, 0), (0, 1, None)):
        with pytest.raises(ValueError):
            within_texels(a, d2, r2_lo, r2_hi, fill)
    for bad in (np.zeros((2, 2, 2), np.int8), np.zeros((2, 2, 2), np.float32), np.zeros((2, 2), np.uint8), np.zeros((2, 2, 2, 2), np.uint8),
                np.zeros((0, 2, 2), np.uint8)):
        with pytest.raises(ValueError):
            distance_squared_texels(bad, 0, 1)
        with pytest.raises(ValueError):
            channel_texels(bad, d2)
    for bad in (np.zeros((2, 2, 3), np.uint32), np.zeros((2, 2, 2), np.float32)):
        with pytest.raises(ValueError):
            within_texels(a, bad)
        with pytest.raises(ValueError):
            channel_texels(a, bad)


def test_rendering_context_refuses_bad_options_in_the_constructor():
    good = {'lo': 0, 'hi': 1, 'mode': 'within'}
    spec = vpt_amd.RenderingContext._distance_spec
    assert spec(None) is None
    assert spec(good) == {'lo': 0, 'hi': 1, 'seeds': 'range', 'mode': 'within', 'from': 0, 'to': NONE, 'fill': 0, 'steps': 1}
    assert spec(dict(good, seeds='rest', to=9, fill=3, **{'from': 4})) == {'lo': 0, 'hi': 1, 'seeds': 'rest', 'mode': 'within', 'from': 4, 'to': 9,
                                                                          'fill': 3, 'steps': 1}
    assert spec({'lo': 3, 'hi': 65535, 'mode': 'channel', 'steps': 256})['steps'] == 256
    for bad in ('within', [0, 1], {'lo': 0, 'hi': 1}, {'lo': 0, 'mode': 'within'}, dict(good, mode='margin'), dict(good, lo=2), dict(good, hi=65536),
                dict(good, seeds='both'), dict(good, to=4, **{'from': 5}), dict(good, fill=65536), dict(good, steps=2), dict(good, mode='channel', steps=0),
                dict(good, mode='channel', steps=257), dict(good, mode='channel', fill=1), dict(good, mode='channel', to=9), dict(good, radius=2)):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext({'distance': bad})
    channel = {'lo': 0, 'hi': 1, 'mode': 'channel'}
    with pytest.raises(ValueError, match='second channel'):
        vpt_amd.RenderingContext({'distance': channel, 'gradient': 'sobel'})
    with pytest.raises(ValueError, match='second channel'):
        vpt_amd.RenderingContext({'distance': channel, 'components': {'lo': 0, 'hi': 1, 'mode': 'label'}})


def test_symbols_resolve_and_null_handles_are_invalid_without_a_device():
    L = N.lib()
    names = ["vpt_volume_distance", "vpt_distance_info", "vpt_distance_squared", "vpt_distance_within", "vpt_distance_channel",
             "vpt_distance_profile", "vpt_distance_destroy"]
    for name in names:
        assert hasattr(L, name) and name in N.SYMBOLS, name
    out = C.c_void_p()
    assert L.vpt_volume_distance(None, 0, 1, 0, C.byref(out)) == N.ERR_INVALID
    assert b"null" in L.vpt_last_error()
    assert L.vpt_distance_info(None, C.byref(N.DistanceInfo())) == N.ERR_INVALID
    assert L.vpt_distance_squared(None, 0, 0, 0, 1, 1, 1, None, 0) == N.ERR_INVALID
    assert L.vpt_distance_within(None, 0, 1, 0, C.byref(out)) == N.ERR_INVALID
    assert L.vpt_distance_channel(None, 1, C.byref(out)) == N.ERR_INVALID
    assert L.vpt_distance_profile(None, (C.c_double * N.DISTANCE_PHASES)()) == N.ERR_INVALID
    assert L.vpt_distance_destroy(None) == N.ERR_INVALID
    assert C.sizeof(N.DistanceInfo) == 16 and N.DistanceInfo.largest.offset == 8


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
@pytest.mark.parametrize("dtype", DTYPES)
def test_node_checks_and_twins_equal_the_numpy_statement(tmp_path, dtype):
    nx, ny, nz = 13, 9, 11
    a = noise(dtype, (nx, ny, nz), seed=43)
    lo, hi = code_range(dtype, 0.05)
    (tmp_path / "texels.raw").write_bytes(a.astype(a.dtype.newbyteorder('<')).tobytes())
    res = subprocess.run(["node", os.path.join(ROOT, "js", "test", "test_distance_host.js"), str(tmp_path / "texels.raw"), str(nx), str(ny), str(nz),
                          str(a.dtype.itemsize * 8), str(lo), str(hi)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = res.stdout.decode().strip().splitlines()
    assert lines[-1] == 'js distance host ok'
    got = json.loads(lines[-2])
    for seeds in SEEDS:
        d2 = distance_squared_texels(a, lo, hi, seeds)
        assert len(np.unique(d2)) >= (8 if seeds == 'range' else 2), "degenerate input"
        assert got[seeds]['d2'] == d2.reshape(-1).tolist(), seeds
        assert got[seeds]['within'] == within_texels(a, d2, 2, 9, 5).reshape(-1).tolist(), seeds
        assert got[seeds]['channel'] == channel_texels(a, d2, 7).reshape(-1).tolist(), seeds
