"""CPU: the gradient-magnitude contract on the host.  vpt_amd.gradient_magnitude (numpy, the statement the device kernel is held to by
tests/test_gpu_gradient.py) against a scalar Python-integer loop written here (math.isqrt, explicit index clamps), closed forms, the gain
range, and the C symbols of the feature without a device."""
import ctypes as C
import math

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd import readers as R
from vpt_amd.gradient import gain_factor, operator_code
from vpt_amd.volume import device_format

GAINS = (1 / 128, 0.5, 1, 3, 16)


def scalar_gradient(v, operator, gain):
    """the contract of include/vpt.h, voxel by voxel in Python integers"""
    d, h, w = v.shape
    bits = v.dtype.itemsize * 8
    g32 = float(np.float32(gain))
    q = math.floor(g32 * g32 * 16384.0 + 0.5)
    a = v.tolist()

    def at(x, y, z):
        return a[min(max(z, 0), d - 1)][min(max(y, 0), h - 1)][min(max(x, 0), w - 1)]

    out = np.zeros(v.shape, dtype=v.dtype)
    wgt = (1, 2, 1)
    for z in range(d):
        for y in range(h):
            for x in range(w):
                if operator == 'central':
                    dx = at(x + 1, y, z) - at(x - 1, y, z)
                    dy = at(x, y + 1, z) - at(x, y - 1, z)
                    dz = at(x, y, z + 1) - at(x, y, z - 1)
                    shift = 16
                else:
                    dx = dy = dz = 0
                    for i in (-1, 0, 1):
                        for j in (-1, 0, 1):
                            k = wgt[i + 1] * wgt[j + 1]
                            dx += k * (at(x + 1, y + i, z + j) - at(x - 1, y + i, z + j))
                            dy += k * (at(x + i, y + 1, z + j) - at(x + i, y - 1, z + j))
                            dz += k * (at(x + i, y + j, z + 1) - at(x + i, y + j, z - 1))
                    shift = 24
                s = dx * dx + dy * dy + dz * dz
                t = (s * q) >> shift
                assert s * q < 1 << 64
                out[z, y, x] = min((1 << bits) - 1, math.isqrt(t))
    return out


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("operator", ["central", "sobel"])
def test_numpy_statement_equals_the_scalar_loop(dtype, operator):
    rng = np.random.default_rng(11)
    top = np.iinfo(dtype).max
    smooth = (np.add.outer(np.add.outer(np.arange(6) * 7, np.arange(5) * 11), np.arange(9) * 5) * (top // 255)).astype(dtype)
    for v in (rng.integers(0, top + 1, size=(5, 6, 7)).astype(dtype), rng.integers(0, top + 1, size=(1, 4, 3)).astype(dtype), smooth):
        for gain in GAINS:
            got = vpt_amd.gradient_magnitude(v, operator, gain)
            assert got.dtype == dtype and got.shape == v.shape
            assert np.array_equal(got, scalar_gradient(v, operator, gain)), (operator, gain, v.shape)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("operator", ["central", "sobel"])
def test_closed_forms(dtype, operator):
    assert not vpt_amd.gradient_magnitude(np.full((4, 5, 6), 77, dtype), operator, 3).any()
    nx = 12
    for k in (1, 7, 23):                                   # k (nx - 1) <= 255
        ramp = np.broadcast_to((k * np.arange(nx)).astype(dtype), (5, 6, nx))
        for gain in (0.5, 1, 2, 3):                        # gain^2 16384 is an integer: q is exact
            g = vpt_amd.gradient_magnitude(ramp, operator, gain)
            assert (g[:, :, 1:-1] == math.floor(gain * k)).all(), (k, gain)
            assert (g[:, :, 0] == math.floor(gain * k / 2)).all() and (g[:, :, -1] == math.floor(gain * k / 2)).all(), (k, gain)
    # an axis of size 1 contributes nothing: the same ramp as a single row, a single slice and a single column
    row = (7 * np.arange(nx)).astype(dtype)
    for shape, axis in (((1, 1, nx), 2), ((1, nx, 1), 1), ((nx, 1, 1), 0)):
        g = vpt_amd.gradient_magnitude(row.reshape(shape), operator, 1).reshape(-1)
        assert (g[1:-1] == 7).all() and g[0] == 3 and g[-1] == 3, (shape, axis)
    assert not vpt_amd.gradient_magnitude(np.full((1, 1, 1), 200, dtype), operator, 16).any()


def test_sixteen_bit_worst_case_saturates_without_wrapping():
    v = np.zeros((4, 4, 6), np.uint16)
    v[:, :, 3:] = 65535
    g = vpt_amd.gradient_magnitude(v, 'sobel', 16)
    assert (g[:, :, 2:4] == 65535).all() and not g[:, :, 0].any() and not g[:, :, -1].any()
    assert np.array_equal(g, scalar_gradient(v, 'sobel', 16))
    v8 = (v >> 8).astype(np.uint8)
    assert (vpt_amd.gradient_magnitude(v8, 'sobel', 16)[:, :, 2:4] == 255).all()


def test_gain_range_and_operators():
    assert gain_factor(1 / 128) == 1 and gain_factor(16) == 4194304 and gain_factor(1) == 16384
    for bad in (0.0, 1 / 256, 16.01, -17.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            gain_factor(bad)
        with pytest.raises(ValueError):
            vpt_amd.gradient_magnitude(np.zeros((2, 2, 2), np.uint8), 'central', bad)
    assert operator_code('central') == N.GRADIENT_CENTRAL == 0 and operator_code('sobel') == N.GRADIENT_SOBEL == 1
    for bad in ('prewitt', 2, None, True):
        with pytest.raises(ValueError):
            operator_code(bad)
    for bad in (np.zeros((2, 2, 2), np.float32), np.zeros((2, 2, 2), np.int8), np.zeros((2, 2, 2, 2), np.uint8)):
        with pytest.raises(ValueError):
            vpt_amd.gradient_magnitude(bad)


def test_symbols_resolve_and_null_handles_are_invalid_without_a_device():
    L = N.lib()
    for name in ("vpt_volume_derive_gradient", "vpt_volume_read_block", "vpt_volume_histogram"):
        assert hasattr(L, name) and name in N.SYMBOLS
    out = C.c_void_p()
    assert L.vpt_volume_derive_gradient(None, N.GRADIENT_CENTRAL, 1.0, C.byref(out)) == N.ERR_INVALID
    assert b"null" in L.vpt_last_error()
    buf = (C.c_uint32 * 256)()
    assert L.vpt_volume_read_block(None, 0, 0, 0, 1, 1, 1, buf, 4) == N.ERR_INVALID
    assert L.vpt_volume_histogram(None, buf, 256) == N.ERR_INVALID


def test_manifest_handling_is_unchanged():
    """device_format of the triples the library took before still gives what it gave"""
    class Gl:
        def extension_enabled(self, name):
            return True
    m = lambda t, f, i=None: {'type': t, 'format': f, 'internalFormat': i}
    assert device_format(m(R.GL_UNSIGNED_BYTE, R.GL_RED, R.GL_R8)) == (N.FORMAT_R8, 1, np.uint8)
    assert device_format(m(R.GL_UNSIGNED_BYTE, R.GL_RG, R.GL_RG8)) == (N.FORMAT_RG8, 2, np.uint8)
    assert device_format(m(R.GL_UNSIGNED_BYTE, R.GL_RGBA, R.GL_RGBA8)) == (N.FORMAT_RG8, 4, np.uint8)
    assert device_format(m(R.GL_FLOAT, R.GL_RED, R.GL_R32F)) == (N.FORMAT_R32F, 1, np.float32)
    assert device_format(m(R.GL_HALF_FLOAT, R.GL_RG, 0x822F)) == (N.FORMAT_RG32F, 2, np.float16)
    assert device_format(m(R.GL_BYTE, R.GL_RED, R.GL_R8_SNORM)) == (N.FORMAT_R8_SNORM, 1, np.int8)
    assert device_format(m(R.GL_UNSIGNED_SHORT_5_6_5, R.GL_RGB, R.GL_RGB565)) == (N.FORMAT_RGB565, 1, np.uint16)
    assert device_format(m(R.GL_UNSIGNED_SHORT, R.GL_RED, R.GL_R16_EXT), Gl()) == (N.FORMAT_R16, 1, np.uint16)
    assert device_format(m(R.GL_UNSIGNED_SHORT, R.GL_RG, R.GL_RG16_EXT), Gl()) == (N.FORMAT_RG16, 2, np.uint16)
    with pytest.raises(RuntimeError, match="Unknown volume datatype"):
        device_format(m(R.GL_UNSIGNED_SHORT, R.GL_RED, R.GL_R16_EXT))
