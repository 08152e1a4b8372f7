"""CPU: the rank filters on the host.  vpt_amd.rank_texels (numpy, the statement the device kernels are held to by tests/test_gpu_rank.py)
against a restatement in Python integers written here — sorted(the 27 clamped taps)[13], min and max —, the properties the contract of
include/vpt.h implies, used as independent checks, the argument errors, the option validation of RenderingContext and the C symbol
without a device."""
import ctypes as C

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.rank import OPERATORS, check_passes, operator_code, rank_texels

from test_pyramid_host import int_texels

SHAPES = ((1, 1, 1), (1, 5, 7), (3, 1, 17), (17, 3, 1), (5, 6, 9))          # depth, height, width
NOISE = (21, 19, 23)
DTYPES = (np.uint8, np.uint16)


def scalar_pass(a, kind):
    """one pass of the contract, texel by texel in Python integers: all 27 clamped taps as a list (a clamped tap as often as it occurs)"""
    d, h, w = a.shape
    v = a.tolist()
    out = np.zeros(a.shape, a.dtype)
    for z in range(d):
        for y in range(h):
            for x in range(w):
                taps = [v[min(max(z + c, 0), d - 1)][min(max(y + b, 0), h - 1)][min(max(x + e, 0), w - 1)]
                        for c in (-1, 0, 1) for b in (-1, 0, 1) for e in (-1, 0, 1)]
                out[z, y, x] = sorted(taps)[13] if kind == 'median' else min(taps) if kind == 'erode' else max(taps)
    return out


def scalar_rank(a, op, passes):
    for kind in {'open': ('erode', 'dilate'), 'close': ('dilate', 'erode')}.get(op, (op,)):
        for _ in range(passes):
            a = scalar_pass(a, kind)
    return a


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPERATORS)
def test_rank_texels_equal_the_scalar_restatement(op, dtype):
    for shape in SHAPES:
        a = int_texels(dtype, shape, seed=21)
        for passes in (1, 2):
            got = rank_texels(a, op, passes)
            assert got.dtype == a.dtype and got.shape == a.shape
            assert got.tolist() == scalar_rank(a, op, passes).tolist(), (op, dtype, shape, passes)
    assert vpt_amd.rank_texels is rank_texels


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_properties_the_contract_implies(dtype):
    M = int(np.iinfo(dtype).max)
    v = int_texels(dtype, NOISE, seed=23)
    inv = (M - v.astype(np.int64)).astype(dtype)
    erode, median, dilate, opened, closed = (rank_texels(v, op) for op in OPERATORS[1:2] + OPERATORS[0:1] + OPERATORS[2:])
    # duality under v -> M - v
    assert np.array_equal(dilate, M - rank_texels(inv, 'erode')) and np.array_equal(erode, M - rank_texels(inv, 'dilate'))
    assert np.array_equal(median, M - rank_texels(inv, 'median'))
    assert np.array_equal(closed, M - rank_texels(inv, 'open'))
    # p erosions are the minimum over the clamped (2 p + 1)^3 box, p = 3
    p = 3
    pad = np.pad(v, p, mode='edge')
    d, h, w = v.shape
    box = np.stack([pad[c:c + d, b:b + h, a:a + w] for c in range(2 * p + 1) for b in range(2 * p + 1) for a in range(2 * p + 1)]).min(axis=0)
    assert np.array_equal(rank_texels(v, 'erode', p), box)
    # the order of the operators
    assert (erode <= median).all() and (median <= dilate).all() and (opened <= v).all() and (v <= closed).all()
    assert (erode < dilate).any()
    # opening and closing are idempotent; erosion and dilation form an adjunction: dilate(a) <= b exactly when a <= erode(b)
    for passes in (1, 2):
        o, c = rank_texels(v, 'open', passes), rank_texels(v, 'close', passes)
        assert np.array_equal(rank_texels(o, 'open', passes), o) and np.array_equal(rank_texels(c, 'close', passes), c)
    assert np.array_equal(rank_texels(rank_texels(erode, 'dilate'), 'erode'), erode)
    assert np.array_equal(rank_texels(rank_texels(dilate, 'erode'), 'dilate'), dilate)
    assert (rank_texels(erode, 'dilate') <= v).all() and (v <= rank_texels(dilate, 'erode')).all()
    # a constant volume is a fixed point of all five, also with axes of 1
    for value in (0, 1, 77, M):
        for shape in ((4, 5, 6), (1, 1, 1), (1, 3, 1)):
            for op in OPERATORS:
                assert (rank_texels(np.full(shape, value, dtype), op, 2) == value).all()


def test_unsigned_whole_code_compares_and_impulses():
    # 0x8000 is larger than 0x7fff (not a signed compare) and 0x0100 larger than 0x00ff (not a byte-wise one)
    a = np.array([[[0x7fff, 0x8000, 0x00ff, 0x0100, 0xff00]]], np.uint16)
    assert rank_texels(a, 'erode').tolist() == [[[0x7fff, 0x00ff, 0x00ff, 0x00ff, 0x0100]]]
    assert rank_texels(a, 'dilate').tolist() == [[[0x8000, 0x8000, 0x8000, 0xff00, 0xff00]]]
    assert rank_texels(a, 'median').tolist() == [[[0x7fff, 0x7fff, 0x0100, 0x0100, 0xff00]]]
    # a single impulse is removed by the median and by the opening, and spread over the box by the dilation
    for dtype in DTYPES:
        M = int(np.iinfo(dtype).max)
        v = np.full((7, 7, 7), 9, dtype); v[3, 3, 3] = M
        assert (rank_texels(v, 'median') == 9).all() and (rank_texels(v, 'open') == 9).all()
        assert int((rank_texels(v, 'dilate') == M).sum()) == 27 and np.array_equal(rank_texels(v, 'close'), v)


def test_arguments():
    a = np.zeros((2, 2, 2), np.uint8)
    assert [operator_code(name) for name in ('median', 'erode', 'dilate', 'open', 'close')] == [0, 1, 2, 3, 4]
    assert (N.RANK_MEDIAN, N.RANK_ERODE, N.RANK_DILATE, N.RANK_OPEN, N.RANK_CLOSE) == (0, 1, 2, 3, 4)
    assert check_passes(1) == 1 and check_passes(8) == 8
    for bad in ('mean', 'Median', '', None, 0, b'median'):
        with pytest.raises(ValueError):
            operator_code(bad)
        with pytest.raises(ValueError):
            rank_texels(a, bad)
    for bad in (0, 9, True, 1.5, -1, '1', None):
        with pytest.raises(ValueError, match='rank-filter passes'):
            check_passes(bad)
        with pytest.raises(ValueError):
            rank_texels(a, 'median', bad)
    for bad in (np.zeros((2, 2, 2), np.int8), np.zeros((2, 2, 2), np.float32), np.zeros((2, 2), np.uint8), np.zeros((2, 2, 2, 2), np.uint8),
                np.zeros((0, 2, 2), np.uint8)):
        with pytest.raises(ValueError):
            rank_texels(bad, 'median')


def test_rendering_context_refuses_bad_options_in_the_constructor():
    for bad in ('mean', 0, True, ['median']):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext({'rank': bad})
    for bad in (0, 9, -1, 1.5, '1', True):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext({'rank': 'median', 'rankPasses': bad})
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext({'rankPasses': bad})


def test_symbol_resolves_and_a_null_handle_is_invalid_without_a_device():
    L = N.lib()
    assert hasattr(L, "vpt_volume_rank") and "vpt_volume_rank" in N.SYMBOLS
    out = C.c_void_p()
    assert L.vpt_volume_rank(None, N.RANK_MEDIAN, 1, C.byref(out)) == N.ERR_INVALID
    assert b"null" in L.vpt_last_error()
