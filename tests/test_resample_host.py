"""CPU: resampling on the host.  vpt_amd.resample_texels (numpy, the statement the device kernels are held to by
tests/test_gpu_resample.py) against a brute force in scalar Python loops over Python integers (every result texel summed over its taps
from the formulas of include/vpt.h, then one //), the consequences the contract implies, the taps, isotropic_shape, the argument checks of
both hosts (the Node ones through js/test/test_resample_host.js, without a device), the option validation of RenderingContext and the C
symbols without a device."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.resample import (axis_taps, check_mode, check_size, check_spacing, count_ties, isotropic_shape, nearest_index, resample_texels)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (np.uint8, np.uint16)
SOURCES = ((5, 6, 7), (1, 1, 1))                                  # depth, height, width
TARGETS = ((5, 6, 7), (1, 1, 1), (3, 2, 5), (10, 12, 14), (2, 9, 7), (11, 4, 3))


def noise(dtype, shape, seed, channels=1):
    M = int(np.iinfo(dtype).max)
    return np.random.default_rng(seed).integers(0, M + 1, size=tuple(shape) + ((2,) if channels == 2 else ())).astype(dtype)


def taps(n, N, X):
    """the taps of result index X as the contract writes them: [(source index, weight)], and S_axis"""
    if N >= n:
        num, D = (2 * X + 1) * n - N, 2 * N
        if num <= 0:
            return [(0, D)], D
        if num >= (n - 1) * D:
            return [(n - 1, D)], D
        i, f = num // D, num % D
        return [(i, D - f), (i + 1, f)], D
    return [(j, min((X + 1) * n, (j + 1) * N) - max(X * n, j * N)) for j in range((X * n) // N, ((X + 1) * n - 1) // N + 1)], n


def brute_force(a, shape):
    """the contract in Python integers: nested lists [Z][Y][X] (or [Z][Y][X][c])"""
    d, h, w = a.shape[:3]
    D, H, W = shape
    v = a.tolist()
    channels = a.shape[3] if a.ndim == 4 else 0
    out = []
    for Z in range(D):
        tz, sz = taps(d, D, Z)
        plane = []
        for Y in range(H):
            ty, sy = taps(h, H, Y)
            row = []
            for X in range(W):
                tx, sx = taps(w, W, X)
                S = sx * sy * sz
                texel = []
                for c in range(max(channels, 1)):
                    total = 0
                    for z, wz in tz:
                        for y, wy in ty:
                            for x, wx in tx:
                                total += wz * wy * wx * (v[z][y][x][c] if channels else v[z][y][x])
                    texel.append((2 * total + S) // (2 * S))
                row.append(texel if channels else texel[0])
            plane.append(row)
        out.append(plane)
    return out


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("dtype", DTYPES)
def test_the_statement_equals_a_brute_force_over_python_integers(dtype, channels):
    for n, source in enumerate(SOURCES):
        a = noise(dtype, source, seed=11 + n, channels=channels)
        for target in TARGETS:
            got = resample_texels(a, target)
            assert got.dtype == a.dtype and got.shape == tuple(target) + a.shape[3:]
            assert got.tolist() == brute_force(a, target), (dtype, channels, source, target)
            near = resample_texels(a, target, 'nearest')
            iz, iy, ix = (nearest_index(m, M) for m, M in zip(source, target))
            assert near.tolist() == [[[a[iz[Z], iy[Y], ix[X]].tolist() for X in range(target[2])] for Y in range(target[1])] for Z in range(target[0])]
    assert vpt_amd.resample_texels is resample_texels and vpt_amd.isotropic_shape is isotropic_shape and vpt_amd.count_ties is count_ties


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_consequences_the_contract_implies(dtype):
    M = int(np.iinfo(dtype).max)
    a = noise(dtype, (5, 6, 7), seed=17)
    # the identity
    assert np.array_equal(resample_texels(a, a.shape), a) and np.array_equal(resample_texels(a, a.shape, 'nearest'), a)
    # halving every axis of an all-even volume is the reduction, byte for byte; on an odd axis the two differ
    for shape in ((6, 8, 10), (2, 2, 2), (16, 16, 64)):
        for channels in (1, 2):
            b = noise(dtype, shape, seed=19, channels=channels)
            half = tuple(n // 2 for n in shape)
            assert resample_texels(b, half).tobytes() == vpt_amd.reduce_texels(b).tobytes(), (shape, channels)
    odd = noise(dtype, (5, 6, 7), seed=23)
    assert not np.array_equal(resample_texels(odd, (3, 3, 4)), vpt_amd.reduce_texels(odd))
    # within [min, max] of the source; a constant volume stays as it is
    for target in ((3, 2, 5), (10, 12, 14), (2, 9, 7), (11, 4, 3)):
        lowish = (noise(dtype, (5, 6, 7), seed=29) % 50 + 100).astype(dtype)
        out = resample_texels(lowish, target)
        assert int(lowish.min()) <= int(out.min()) and int(out.max()) <= int(lowish.max())
        for value in (0, 1, M // 2, M - 1, M):
            assert (resample_texels(np.full((5, 6, 7), value, dtype), target) == value).all(), (target, value)
        # the flip of the volume gives the flip of the result
        flipped = np.ascontiguousarray(a[::-1, ::-1, ::-1])
        assert np.array_equal(resample_texels(flipped, target), resample_texels(a, target)[::-1, ::-1, ::-1]), target
        for axis in (0, 1, 2):
            assert np.array_equal(resample_texels(np.ascontiguousarray(np.flip(a, axis)), target), np.flip(resample_texels(a, target), axis))
        # a transposed volume gives the transposed result: each axis is taken alone
        assert np.array_equal(resample_texels(np.ascontiguousarray(a.transpose(2, 0, 1)), (target[2], target[0], target[1])),
                              resample_texels(a, target).transpose(2, 0, 1))
    # exact halves occur: the rounding rule is exercised
    assert count_ties(noise(dtype, (6, 8, 10), seed=31), (3, 4, 5)) >= 1
    assert count_ties(noise(dtype, (5, 6, 7), seed=31), (10, 12, 14)) >= 1
    two = np.array([[[0, 1]]], dtype)
    assert count_ties(two, (1, 1, 1)) == 1 and resample_texels(two, (1, 1, 1)).tolist() == [[[1]]]                 # halves go up
    assert resample_texels(np.array([[[0, M]]], dtype), (1, 1, 4)).tolist() == [[[0, (2 * M + 4) // 8, (6 * M + 4) // 8, M]]]


def test_the_wide_divisor_fits_int64():
    """S = 2^34 and the largest code everywhere: 2 SUM + S = (2 * 65535 + 1) * 2^34 < 2^57"""
    a = np.full((2048, 2, 2048), 65535, np.uint16)
    assert (resample_texels(a, (1, 2048, 4)) == 65535).all()
    a[:1024] = 0
    assert (resample_texels(a, (1, 2048, 4)) == 32768).all()      # an exact half, rounded up
    assert count_ties(a, (1, 2048, 4)) == 2048 * 4


def test_taps_are_positive_and_sum_to_the_axis_sum():
    pairs = [(n, N) for n in range(1, 41) for N in range(1, 41)] + [(4096, 1), (1, 4096), (4095, 4096), (4096, 4095)]
    for n, N in pairs:
        rows, S = axis_taps(n, N)
        assert S == (2 * N if N >= n else n) and len(rows) == N
        covered = set()
        for X, row in enumerate(rows):
            assert all(w > 0 and 0 <= j < n for j, w in row) and sum(w for _, w in row) == S, (n, N, X)
            assert [j for j, _ in row] == list(range(row[0][0], row[0][0] + len(row)))
            want, _ = taps(n, N, X)
            assert row == [(j, w) for j, w in want if w], (n, N, X)
            covered.update(j for j, _ in row)
        if N < n:
            assert covered == set(range(n)), "a source texel is dropped"
            for j in range(n):                                    # every source texel's weights sum to N: the average is unbiased
                assert sum(w for row in rows for k, w in row if k == j) == N
        near = nearest_index(n, N)
        assert near.dtype == np.int64 and len(near) == N and near.min() >= 0 and near.max() <= n - 1 and (np.diff(near) >= 0).all()
        assert near.tolist() == [((2 * X + 1) * n) // (2 * N) for X in range(N)]
    assert [j for row in axis_taps(7, 7)[0] for j, _ in row] == list(range(7))


def test_isotropic_shape():
    assert isotropic_shape((512, 512, 200), (0.7, 0.7, 2.0)) == (512, 512, 571)
    assert isotropic_shape((512, 512, 200), (0.7, 0.7, 2.0), pitch=1.4) == (256, 256, 286)
    assert isotropic_shape((512, 512, 200), (0.7, 0.7, 2.0), 2.0) == (179, 179, 200)
    assert isotropic_shape((3, 3, 3), (1, 1, 0.01), 1) == (3, 3, 1)
    assert isotropic_shape((4096, 1, 1), (1, 1, 1)) == (4096, 1, 1)
    assert isotropic_shape([np.int32(8), 8, 8], [np.float32(0.5), 1, 2]) == (8, 16, 32)
    with pytest.raises(ValueError, match='along y'):
        isotropic_shape((10, 241, 10), (1, 17, 1), 1)             # 4097
    with pytest.raises(ValueError, match='along z'):
        isotropic_shape((10, 10, 2049), (1, 1, 2))
    with pytest.raises(ValueError, match='along x'):
        isotropic_shape((4097, 1, 1), (1, 1, 1))
    for bad in ((0, 1, 1), (1, -1, 1), (1, 1, float('nan')), (float('inf'), 1, 1), (1, '1', 1), (1, 1), None, 'abc', (True, 1, 1)):
        with pytest.raises(ValueError, match='spacing'):
            isotropic_shape((4, 4, 4), bad)
    for bad in (0, -1, float('nan'), float('inf'), '1', True):
        with pytest.raises(ValueError, match='pitch'):
            isotropic_shape((4, 4, 4), (1, 1, 1), bad)
    assert check_spacing([1, 2, 3]) == ((1.0, 2.0, 3.0), 1.0) and check_spacing((1, 2, 3), 0.5)[1] == 0.5


def test_arguments():
    a = np.zeros((2, 2, 2), np.uint8)
    assert check_mode('nearest') == N.RESAMPLE_NEAREST == 0 and check_mode('filtered') == N.RESAMPLE_FILTERED == 1
    for bad in (0, 1, 'linear', None, True, b'nearest'):
        with pytest.raises(ValueError, match='mode'):
            check_mode(bad)
        with pytest.raises(ValueError):
            resample_texels(a, (2, 2, 2), bad)
    assert check_size(1, 4096, np.int64(7)) == (1, 4096, 7)
    for bad, axis in (((0, 1, 1), 'x'), ((1, 4097, 1), 'y'), ((1, 1, 1.5), 'z'), ((1, 1, '2'), 'z'), ((None, 1, 1), 'x'), ((1, True, 1), 'y'), ((-3, 1, 1), 'x')):
        with pytest.raises(ValueError, match='along %s' % axis):
            check_size(*bad)
        with pytest.raises(ValueError):
            resample_texels(a, bad[::-1])
    for bad in (np.zeros((2, 2, 2), np.int8), np.zeros((2, 2, 2), np.float32), np.zeros((2, 2), np.uint8), np.zeros((2, 2, 2, 3), np.uint8),
                np.zeros((0, 2, 2), np.uint8), np.zeros((2, 2, 2), np.uint32)):
        with pytest.raises(ValueError):
            resample_texels(bad, (2, 2, 2))
        with pytest.raises(ValueError):
            count_ties(bad, (2, 2, 2))
    for ok in (np.zeros((2, 2, 2), np.int8), np.zeros((2, 2, 2, 2), np.int16), np.zeros((2, 2, 2), np.float32)):
        assert resample_texels(ok, (3, 1, 2), 'nearest').shape == (3, 1, 2) + ok.shape[3:]
    with pytest.raises(ValueError):
        resample_texels(np.zeros((2, 2, 2), np.float64), (2, 2, 2), 'nearest')
    with pytest.raises(ValueError):
        resample_texels(a, (2, 2))
    f = np.array([0x7FC12345, 0xFF800001], np.uint32).view(np.float32).reshape(1, 1, 2)
    assert resample_texels(f, (1, 1, 4), 'nearest').view(np.uint32).tolist() == [[[0x7FC12345, 0x7FC12345, 0xFF800001, 0xFF800001]]]


def test_rendering_context_refuses_bad_options_in_the_constructor():
    spec = vpt_amd.RenderingContext._resample_spec
    assert spec(None) is None
    assert spec({'size': [3, 4, 5]}) == {'size': (3, 4, 5), 'spacing': None, 'pitch': None, 'mode': 'filtered'}
    assert spec({'spacing': [0.7, 0.7, 2], 'mode': 'nearest'}) == {'size': None, 'spacing': (0.7, 0.7, 2.0), 'pitch': 0.7, 'mode': 'nearest'}
    assert spec({'spacing': (1, 1, 2), 'pitch': 0.5})['pitch'] == 0.5 and spec({'size': (3, 4, 5), 'pitch': None, 'mode': None})['mode'] == 'filtered'
    for bad in ('filtered', [3, 4, 5], {}, {'mode': 'nearest'}, {'size': [3, 4, 5], 'spacing': [1, 1, 1]}, {'size': [3, 4]}, {'size': [0, 4, 5]},
                {'size': [3, 4, 4097]}, {'size': [3, 4, 5], 'pitch': 1}, {'size': [3, 4, 5], 'mode': 'linear'}, {'spacing': [1, 1, 0]},
                {'spacing': [1, 1, float('nan')]}, {'spacing': [1, 1]}, {'spacing': [1, 1, 1], 'pitch': 0}, {'spacing': [1, 1, 1], 'pitch': -2},
                {'size': [3, 4, 5], 'factor': 2}):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext({'resample': bad})


def test_symbols_resolve_and_null_handles_are_invalid_without_a_device():
    L = N.lib()
    for name in ("vpt_volume_resample", "vpt_volume_resample_timed"):
        assert hasattr(L, name) and name in N.SYMBOLS, name
    out = C.c_void_p()
    assert L.vpt_volume_resample(None, 4, 4, 4, N.RESAMPLE_FILTERED, C.byref(out)) == N.ERR_INVALID
    assert b"null" in L.vpt_last_error()
    ms = (C.c_double * N.RESAMPLE_PHASES)()
    assert L.vpt_volume_resample_timed(None, 4, 4, 4, N.RESAMPLE_NEAREST, C.byref(out), ms) == N.ERR_INVALID
    header = open(os.path.join(ROOT, "include", "vpt.h")).read()
    assert "#define VPT_RESAMPLE_NEAREST  0" in header and "#define VPT_RESAMPLE_FILTERED 1" in header and "#define VPT_RESAMPLE_PHASES 2" in header


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
@pytest.mark.parametrize("dtype,channels", [(np.uint8, 1), (np.uint16, 2)])
def test_node_checks_and_twin_equal_the_numpy_statement(tmp_path, dtype, channels):
    nx, ny, nz = 13, 9, 11
    target = (7, 20, 9)                                           # depth, height, width: shrink, grow, shrink
    a = noise(dtype, (nz, ny, nx), seed=43, channels=channels)
    (tmp_path / "texels.raw").write_bytes(a.astype(a.dtype.newbyteorder('<')).tobytes())
    res = subprocess.run(["node", os.path.join(ROOT, "js", "test", "test_resample_host.js"), str(tmp_path / "texels.raw"), str(nx), str(ny), str(nz),
                          str(a.dtype.itemsize * 8), str(channels), str(target[2]), str(target[1]), str(target[0])],
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = res.stdout.decode().strip().splitlines()
    assert lines[-1] == 'js resample host ok'
    got = json.loads(lines[-2])
    want = resample_texels(a, target)
    assert len(np.unique(want)) >= 8, "degenerate input"
    assert got['filtered'] == want.reshape(-1).tolist()
    assert got['nearest'] == resample_texels(a, target, 'nearest').reshape(-1).tolist()
    assert got['ties'] == count_ties(a, target)
