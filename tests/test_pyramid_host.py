"""CPU: the 2x reduction and the binomial smoothing on the host.  vpt_amd.reduce_texels and vpt_amd.smooth_texels (numpy, the statements
the device kernels are held to by tests/test_gpu_pyramid.py) against scalar loops written here — Python integers with >> for the two
integer contracts, Python floats (IEEE doubles) with an explicit numpy.float32 rounding for the float contract —, the rounding ties, the
option validation of RenderingContext and the C symbols of the feature without a device."""
import ctypes as C
import math

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.pyramid import check_levels, check_passes, reduced_shape

INT_TYPES = (np.uint8, np.uint16, np.int8, np.int16)
SHAPES = ((1, 1, 1), (1, 5, 7), (3, 1, 17), (5, 6, 7))          # depth, height, width


def int_texels(dtype, shape, seed=3):
    """every code equally likely, the most negative one included"""
    info = np.iinfo(dtype)
    return np.random.default_rng(seed).integers(info.min, info.max + 1, size=shape).astype(dtype)


def float_texels(shape, seed=5, specials=True):
    """standard normal; `specials`: about 1 texel in 100 replaced by NaN, +inf or -inf"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape).astype(np.float32)
    if specials:
        pick = rng.random(shape)
        v[pick < 0.003] = np.nan; v[(pick >= 0.003) & (pick < 0.006)] = np.inf; v[(pick >= 0.006) & (pick < 0.009)] = -np.inf
    return v


def cells(shape):
    """(X, Y, Z) and the eight (x, y, z) taps of every result texel, in the contract's order: x fastest, then y, then z"""
    d, h, w = shape[:3]
    for Z in range((d + 1) // 2):
        for Y in range((h + 1) // 2):
            for X in range((w + 1) // 2):
                yield (X, Y, Z), [(x, y, z) for z in (2 * Z, min(2 * Z + 1, d - 1)) for y in (2 * Y, min(2 * Y + 1, h - 1)) for x in (2 * X, min(2 * X + 1, w - 1))]


def scalar_reduce_int(a):
    """the integer contract of include/vpt.h, texel by texel in Python integers; also the sums themselves"""
    least = -np.iinfo(a.dtype).max if a.dtype.kind == 'i' else 0
    four = a.reshape(a.shape[:3] + (-1,))
    out = np.zeros(reduced_shape(four.shape), a.dtype)
    sums = []
    for (X, Y, Z), taps in cells(a.shape):
        for c in range(four.shape[3]):
            s = sum(max(int(four[z, y, x, c]), least) for x, y, z in taps)
            sums.append(s)
            out[Z, Y, X, c] = (s + 4) >> 3
    return out.reshape(reduced_shape(a.shape)), sums


def scalar_reduce_float(a):
    """the float contract, texel by texel in Python floats (IEEE doubles, one rounding per addition), rounded once by numpy.float32"""
    four = a.reshape(a.shape[:3] + (-1,))
    out = np.zeros(reduced_shape(four.shape), np.float32)
    for (X, Y, Z), taps in cells(a.shape):
        for c in range(four.shape[3]):
            v = [float(four[z, y, x, c]) for x, y, z in taps]     # float32 -> double is exact
            s = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))
            with np.errstate(all='ignore'):
                out[Z, Y, X, c] = np.float32(s * 0.125)
    return out.reshape(reduced_shape(a.shape))


def scalar_smooth(a, passes):
    """the smoothing contract, texel by texel in Python integers: all 27 taps, one rounding per pass"""
    d, h, w = a.shape
    v = a.astype(object)
    wgt = (1, 2, 1)
    for _ in range(passes):
        nxt = np.zeros(a.shape, object)
        for z in range(d):
            for y in range(h):
                for x in range(w):
                    W = 0
                    for c in (-1, 0, 1):
                        for b in (-1, 0, 1):
                            for e in (-1, 0, 1):
                                W += wgt[c + 1] * wgt[b + 1] * wgt[e + 1] * int(v[min(max(z + c, 0), d - 1), min(max(y + b, 0), h - 1), min(max(x + e, 0), w - 1)])
                    nxt[z, y, x] = (W + 32) >> 6
        v = nxt
    return v.astype(a.dtype)


def same_floats(got, want):
    """bit for bit where the expectation is finite or infinite, NaN where it is NaN"""
    nan = np.isnan(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("dtype", INT_TYPES)
def test_integer_reduction_equals_the_scalar_loop(dtype, channels):
    ties = negative_ties = 0
    for shape in SHAPES:
        a = int_texels(dtype, shape + ((2,) if channels == 2 else ()))
        if dtype in (np.int8, np.int16):
            a.reshape(-1)[0] = np.iinfo(dtype).min                  # the most negative code is read as the one above it
        got = vpt_amd.reduce_texels(a)
        want, sums = scalar_reduce_int(a)
        assert got.dtype == a.dtype and got.shape == reduced_shape(a.shape)
        assert got.tolist() == want.tolist(), (dtype, shape)
        ties += sum(1 for s in sums if s % 8 == 4)
        negative_ties += sum(1 for s in sums if s % 8 == 4 and s < 0)
    assert ties >= 4, "no cell whose sum is 4 mod 8: the rounding ties are not exercised"
    if dtype in (np.int8, np.int16):
        assert negative_ties >= 2, "no negative rounding tie"
    # the ties themselves, by construction: a mean of k + 1/2 rounds up to k + 1, also below zero
    info = np.iinfo(dtype)
    for k in (info.min + 1, -3, -1, 0, 5, info.max - 1):
        if info.min < k + 1 <= info.max and k >= info.min + (1 if info.min < 0 else 0):
            cell = np.full((2, 2, 2), k, dtype); cell[0, 0, :] = k + 1; cell[1, 1, :] = k + 1      # four texels of k, four of k + 1
            assert vpt_amd.reduce_texels(cell).tolist() == [[[k + 1]]], (dtype, k)
    if info.min < 0:
        assert vpt_amd.reduce_texels(np.full((2, 2, 2), info.min, dtype)).tolist() == [[[info.min + 1]]]
    assert vpt_amd.reduce_texels(np.full((3, 3, 3), info.max, dtype)).tolist() == [[[info.max] * 2] * 2] * 2


@pytest.mark.parametrize("channels", [1, 2])
def test_float_reduction_equals_the_scalar_loop(channels):
    for shape in SHAPES + ((9, 10, 11),):
        a = float_texels(shape + ((2,) if channels == 2 else ()))
        if a.size >= 8:
            a.reshape(-1)[:3] = (np.nan, np.inf, -np.inf)
        assert same_floats(vpt_amd.reduce_texels(a), scalar_reduce_float(a)), shape
    # the order of the additions is part of the contract: 2^60 absorbs 1 unless the ones are added to each other first ...
    cell = np.array([[[2.0 ** 60, 1.0], [1.0, 1.0]], [[1.0, 1.0], [1.0, 1.0]]], np.float32)
    assert same_floats(vpt_amd.reduce_texels(cell), scalar_reduce_float(cell))
    # ... and the one rounding to float32 happens after the exact multiplication
    cell = np.array([[[1.0, 2.0 ** -24], [0.0, 0.0]], [[0.0, 0.0], [0.0, 0.0]]], np.float32)
    assert vpt_amd.reduce_texels(cell).tolist() == [[[float(np.float32((1.0 + 2.0 ** -24) * 0.125))]]]
    both = np.array([[[np.inf, -np.inf], [0.0, 0.0]], [[0.0, 0.0], [0.0, 0.0]]], np.float32)
    assert math.isnan(vpt_amd.reduce_texels(both)[0, 0, 0])
    big = np.full((2, 2, 2), 3.0e38, np.float32)                    # the sum is taken in doubles: no overflow on the way
    assert vpt_amd.reduce_texels(big).tolist() == [[[float(np.float32(3.0e38))]]]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_smoothing_equals_the_scalar_loop(dtype):
    for shape in SHAPES:
        a = int_texels(dtype, shape, seed=9)
        for passes in (1, 2):
            got = vpt_amd.smooth_texels(a, passes)
            assert got.dtype == a.dtype and got.shape == a.shape
            assert got.tolist() == scalar_smooth(a, passes).tolist(), (dtype, shape, passes)
    top = np.iinfo(dtype).max
    for value in (0, 1, 77, top):                                   # a constant volume stays that constant, at the largest texel too
        for passes in (1, 8):
            assert (vpt_amd.smooth_texels(np.full((4, 5, 6), value, dtype), passes) == value).all()
    impulse = np.zeros((21, 21, 21), dtype); impulse[10, 10, 10] = 255
    once = vpt_amd.smooth_texels(impulse, 1)
    assert once[10, 10, 10] == (8 * 255 + 32) >> 6 and once[9, 10, 10] == (4 * 255 + 32) >> 6 and once[9, 9, 9] == (255 + 32) >> 6
    assert vpt_amd.smooth_texels(impulse, 8)[10, 10, 10] > 0
    assert vpt_amd.smooth_texels is not None and vpt_amd.reduce_texels is not None


def test_arguments():
    assert check_passes(1) == 1 and check_passes(8) == 8 and check_levels(1) == 1 and check_levels(40) == 40
    for bad in (0, 9, -1, 1.0, '2', None, True):
        with pytest.raises(ValueError):
            check_passes(bad)
        with pytest.raises(ValueError):
            vpt_amd.smooth_texels(np.zeros((2, 2, 2), np.uint8), bad)
    for bad in (0, -1, 1.5, '1', None, True):
        with pytest.raises(ValueError):
            check_levels(bad)
    for bad in (np.zeros((2, 2, 2), np.int8), np.zeros((2, 2, 2), np.float32), np.zeros((2, 2, 2, 2), np.uint8), np.zeros((2, 2), np.uint8)):
        with pytest.raises(ValueError):
            vpt_amd.smooth_texels(bad)
    for bad in (np.zeros((2, 2, 2), np.float64), np.zeros((2, 2, 2), np.int32), np.zeros((2, 2, 2, 3), np.uint8), np.zeros((2, 2), np.uint8),
                np.zeros((0, 2, 2), np.uint8)):
        with pytest.raises(ValueError):
            vpt_amd.reduce_texels(bad)


def test_rendering_context_refuses_bad_options_in_the_constructor():
    for bad in (0, 9, -1, 1.5, '1', True):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext({'smooth': bad})
    for bad in (-1, 1.5, '1', True):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext({'reduce': bad})


def test_symbols_resolve_and_null_handles_are_invalid_without_a_device():
    L = N.lib()
    for name in ("vpt_volume_reduce", "vpt_volume_smooth"):
        assert hasattr(L, name) and name in N.SYMBOLS
    out = C.c_void_p()
    assert L.vpt_volume_reduce(None, C.byref(out)) == N.ERR_INVALID
    assert b"null" in L.vpt_last_error()
    assert L.vpt_volume_smooth(None, 1, C.byref(out)) == N.ERR_INVALID
    assert b"null" in L.vpt_last_error()
