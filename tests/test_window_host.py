"""CPU: the value-range window on the host.  vpt_amd.window_texels (numpy, the statement the device kernel is held to by
tests/test_gpu_window.py) against scalar loops written here — Python integers with // for the integer contract, Python floats (IEEE
doubles) for the float contract —, identity and monotonicity, vpt_amd.percentile_window against a sorted-array statement, RAWReader's
`bits` / `signed` options in both hosts, and the C symbols of the feature without a device."""
import ctypes as C
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd import readers as R
from vpt_amd.window import check_window, format_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_TYPES = (np.uint8, np.uint16, np.int8, np.int16)
# (generator of codes, window) per type whose texels fall strictly inside the window for the most part: the rounding branch
INSIDE = {np.uint8: ((0, 256), (20, 235)), np.uint16: ((0, 4096), (205, 3890)), np.int8: ((-128, 128), (-100, 100)),
          np.int16: ((-1000, 3001), (-900, 2800))}


def scalar_window_int(codes, signed_bits, lo, hi, M):
    """the integer contract of include/vpt.h, texel by texel in Python integers"""
    D = hi - lo
    out = []
    for c in codes:
        if signed_bits:
            c = max(c, -(2 ** (signed_bits - 1) - 1))
        n = c - lo
        out.append(0 if n <= 0 else M if n >= D else (2 * n * M + D) // (2 * D))
    return out


def scalar_window_float(values, lo, hi, M):
    """the float contract, texel by texel in Python floats (IEEE doubles, one rounding per operation)"""
    out = []
    for v in values:
        v = float(v)                                             # float32 -> double is exact
        if math.isnan(v):
            out.append(0); continue
        if math.isinf(v):
            out.append(M if v > 0 else 0); continue
        t = (v - lo) / (hi - lo)
        out.append(0 if not t > 0 else M if t >= 1 else int(math.floor(t * M + 0.5)))
    return out


def int_windows(dtype):
    info = np.iinfo(dtype)
    a, b = info.min, info.max
    return [(a, b), (0, 1), (-1, 0), (b - 1, b), (a, a + 1), (a + 1, a + 2), (5, 6), (b + 10, b + 500), (a - 500, a - 10),
            (-70000, 70000), (-2 ** 31, 2 ** 31), (-2 ** 31, -2 ** 31 + 1), (2 ** 31 - 1, 2 ** 31), (-2 ** 31, 0), (0, 2 ** 31),
            (-37, 91), (3, 250), INSIDE[dtype][1]]


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("dtype", INT_TYPES)
def test_integer_contract_equals_the_scalar_loop(dtype, bits):
    info = np.iinfo(dtype)
    M = (1 << bits) - 1
    every = np.arange(info.min, info.max + 1).astype(dtype)      # every code, the most negative one included
    rng = np.random.default_rng(5)
    for lo, hi in int_windows(dtype):
        got = vpt_amd.window_texels(every, lo, hi, bits)
        assert got.dtype == (np.uint8 if bits == 8 else np.uint16) and got.shape == every.shape
        want = scalar_window_int(every.tolist(), info.bits if info.min < 0 else 0, lo, hi, M)
        assert got.tolist() == want, (dtype, bits, lo, hi)
    for _ in range(40):                                          # random windows around the codes
        lo = int(rng.integers(info.min - 300, info.max + 300))
        hi = lo + int(rng.integers(1, 2 * (info.max - info.min)))
        got = vpt_amd.window_texels(every, lo, hi, bits)
        assert got.tolist() == scalar_window_int(every.tolist(), info.bits if info.min < 0 else 0, lo, hi, M), (dtype, bits, lo, hi)
    if info.min < 0:                                             # the most negative code reads as the one above it
        pair = vpt_amd.window_texels(np.array([info.min, info.min + 1], dtype), info.min, info.max, bits)
        assert pair[0] == pair[1]
        assert vpt_amd.window_texels(np.array([info.min], dtype), info.min, info.min + 1, bits)[0] == M


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("dtype", INT_TYPES)
def test_random_integer_texels_mostly_strictly_inside_the_window(dtype, bits):
    (a, b), (lo, hi) = INSIDE[dtype]
    M = (1 << bits) - 1
    v = np.random.default_rng(7).integers(a, b, size=(29, 30, 31)).astype(dtype)
    got = vpt_amd.window_texels(v, lo, hi, bits)
    inside = ((got > 0) & (got < M)).mean()
    assert inside >= 0.5, "degenerate case: %.3f of the texels strictly inside" % inside
    assert ((v.astype(np.int64) > lo) & (v.astype(np.int64) < hi)).mean() >= 0.5
    info = np.iinfo(dtype)
    assert got.reshape(-1).tolist() == scalar_window_int(v.reshape(-1).tolist(), info.bits if info.min < 0 else 0, lo, hi, M)
    if dtype == np.uint16 and bits == 8:
        assert len(np.unique(got)) == 256


def float_cases(lo, hi, M, seed=3):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, size=4000, dtype=np.uint64).astype(np.uint32).view(np.float32)       # random bit patterns
    special = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 3.4028235e38, -3.4028235e38,
                        lo, hi, np.nextafter(np.float32(lo), np.float32(np.inf)), np.nextafter(np.float32(hi), np.float32(-np.inf))], dtype=np.float32)
    k = np.arange(0, M, max(1, M // 997), dtype=np.float64)
    ties = (lo + (k + 0.5) * (hi - lo) / M).astype(np.float32)
    near = np.concatenate([np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf))])
    with np.errstate(over='ignore'):
        normal = (rng.standard_normal(4000) * (hi - lo) / 2 + (hi + lo) / 2).astype(np.float32)
    return np.concatenate([bits, special, ties, near, normal])


@pytest.mark.parametrize("bits", [8, 16])
def test_float_contract_equals_the_scalar_loop(bits):
    M = (1 << bits) - 1
    for lo, hi in ((-1.0, 1.0), (0.0, 1.0), (-1000.0, 3000.0), (0.1, 0.7), (-1e30, 1e30), (1e-40, 2e-40), (-3.0e38, 3.0e38 / 4), (5.0, 5.0 + 2 ** -40)):
        v = float_cases(lo, hi, M)
        got = vpt_amd.window_texels(v, lo, hi, bits)
        assert got.dtype == (np.uint8 if bits == 8 else np.uint16)
        assert got.tolist() == scalar_window_float(v.tolist(), lo, hi, M), (lo, hi, bits)
    v = np.array([np.nan, -np.inf, np.inf, -0.0, 0.0, 0.5, 1.0, 2.0], np.float32)
    assert vpt_amd.window_texels(v, 0.0, 1.0, bits).tolist() == [0, 0, M, 0, 0, (M + 1) // 2, M, M]


@pytest.mark.parametrize("bits", [8, 16])
def test_random_float_texels_mostly_strictly_inside_the_window(bits):
    M = (1 << bits) - 1
    v = np.random.default_rng(11).standard_normal((9, 10, 11)).astype(np.float32)
    got = vpt_amd.window_texels(v, -1.0, 1.0, bits)
    assert ((v > -1) & (v < 1)).mean() >= 0.5 and ((got > 0) & (got < M)).mean() >= 0.5
    assert got.reshape(-1).tolist() == scalar_window_float(v.reshape(-1).tolist(), -1.0, 1.0, M)
    assert len(np.unique(got)) >= 32


def test_identity_and_monotonicity():
    a16, a8 = np.arange(65536).astype(np.uint16), np.arange(256).astype(np.uint8)
    assert np.array_equal(vpt_amd.window_texels(a16, 0, 65535, 16), a16)
    assert np.array_equal(vpt_amd.window_texels(a8, 0, 255, 8), a8)
    rng = np.random.default_rng(13)
    for dtype in INT_TYPES:
        info = np.iinfo(dtype)
        every = np.arange(info.min, info.max + 1).astype(dtype)
        for _ in range(30):
            lo = int(rng.integers(info.min - 50, info.max))
            hi = lo + int(rng.integers(1, info.max - info.min + 100))
            for bits in (8, 16):
                out = vpt_amd.window_texels(every, lo, hi, bits).astype(np.int64)
                assert (np.diff(out) >= 0).all(), (dtype, lo, hi, bits)
    f = np.sort(np.random.default_rng(17).standard_normal(5000).astype(np.float32))
    for bits in (8, 16):
        assert (np.diff(vpt_amd.window_texels(f, -0.7, 1.3, bits).astype(np.int64)) >= 0).all()


def test_arguments():
    assert format_bits('r8') == 8 and format_bits('r16') == 16 and format_bits(16) == 16
    for bad in ('r32f', 12, None, True):
        with pytest.raises(ValueError):
            format_bits(bad)
    z = np.zeros(4, np.uint16)
    for lo, hi in ((5, 5), (6, 5), (0.5, 3), (0, 2.5), (-2 ** 31 - 1, 0), (0, 2 ** 31 + 1), (float('nan'), 1), (0, float('inf'))):
        with pytest.raises(ValueError):
            vpt_amd.window_texels(z, lo, hi)
    assert check_window(np.uint16, 2.0, 7.0) == (2, 7)          # integral floats are integers
    f = np.zeros(4, np.float32)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float('nan'), 1.0), (0.0, float('inf')), (-1.7e308, 1.7e308)):
        with pytest.raises(ValueError):
            vpt_amd.window_texels(f, lo, hi)
    for bad in (np.zeros(4, np.float64), np.zeros(4, np.int32), np.zeros(4, np.uint32)):
        with pytest.raises(ValueError):
            vpt_amd.window_texels(bad, 0, 1)


def test_percentile_window_equals_the_sorted_array_statement():
    rng = np.random.default_rng(19)
    cases = [(rng.integers(0, 4096, size=5000).astype(np.uint16), 65536, False), (rng.integers(-1000, 3001, size=3333).astype(np.int16), 65536, True),
             (rng.integers(0, 256, size=777).astype(np.uint8), 256, False), (rng.integers(-128, 128, size=1001).astype(np.int8), 256, True),
             (np.full(10, 42, np.uint8), 256, False), (np.array([7], np.uint16), 65536, False), (np.array([65535] * 3, np.uint16), 65536, False)]
    for codes, nbins, signed in cases:
        bias = nbins // 2 if signed else 0
        hist = np.bincount(codes.astype(np.int64) + bias, minlength=nbins).astype(np.uint32)
        s = sorted(codes.tolist())
        n = len(s)
        for p_lo, p_hi in ((0.5, 99.5), (0, 100), (1, 99), (25, 75), (50, 50), (0, 0), (100, 100), (0.1, 99.9), (33.3, 66.6)):
            from fractions import Fraction
            k_lo = max(1, math.ceil(Fraction(p_lo) * n / 100)); k_hi = max(1, math.ceil(Fraction(p_hi) * n / 100))
            lo = s[k_lo - 1]; hi = max(s[k_hi - 1], lo + 1)
            assert vpt_amd.percentile_window(hist, p_lo, p_hi, signed) == (lo, hi), (codes.dtype, p_lo, p_hi)
    with pytest.raises(ValueError):
        vpt_amd.percentile_window(np.zeros(256, np.uint32))
    with pytest.raises(ValueError):
        vpt_amd.percentile_window(np.ones(100, np.uint32))
    with pytest.raises(ValueError):
        vpt_amd.percentile_window(np.ones(256, np.uint32), 60, 40)


# ---- RAWReader: bits / signed ------------------------------------------------------------------------------------------------
RAW_DIMS = (5, 4, 3)                                             # width, height, depth


def raw_expectations():
    return {(8, False): (R.GL_RED, R.GL_R8, R.GL_UNSIGNED_BYTE, 1), (16, False): (R.GL_RED, R.GL_R16_EXT, R.GL_UNSIGNED_SHORT, 2),
            (16, True): (R.GL_RED, R.GL_R16_SNORM_EXT, R.GL_SHORT, 2), (32, False): (R.GL_RED, R.GL_R32F, R.GL_FLOAT, 4)}


def test_raw_reader_honours_bits_and_signed():
    w, h, d = RAW_DIMS
    data = bytes(range(256)) * 2                                 # 512 bytes >= 4 * 60
    plain = vpt_amd.RAWReader(data, {'width': w, 'height': h, 'depth': d})
    for (bits, signed), (fmt, ifmt, typ, size) in raw_expectations().items():
        r = vpt_amd.RAWReader(data, {'width': w, 'height': h, 'depth': d, 'bits': bits, 'signed': signed})
        md = r.readMetadata()
        m = md['modalities'][0]
        assert (m['format'], m['internalFormat'], m['type']) == (fmt, ifmt, typ), (bits, signed)
        assert m['dimensions'] == {'width': w, 'height': h, 'depth': d} and len(md['blocks']) == d == len(m['placements'])
        assert all(b['dimensions'] == {'width': w, 'height': h, 'depth': 1} for b in md['blocks'])
        for i in range(d):
            assert bytes(r.readBlock(i)) == data[i * w * h * size:(i + 1) * w * h * size], (bits, i)
        if bits == 8:                                            # bits: 8 and no bits: today's metadata and blocks
            assert md == plain.readMetadata() and 'bits' not in str(md)
            assert all(bytes(r.readBlock(i)) == bytes(plain.readBlock(i)) for i in range(d))
    m = plain.readMetadata()['modalities'][0]
    assert (m['format'], m['internalFormat'], m['type']) == (R.GL_RED, R.GL_R8, R.GL_UNSIGNED_BYTE)
    for bad in ({'bits': 12}, {'bits': 64}, {'bits': '16'}, {'bits': 8, 'signed': True}, {'bits': 32, 'signed': True}):
        with pytest.raises(RuntimeError):
            vpt_amd.RAWReader(data, dict({'width': w, 'height': h, 'depth': d}, **bad))
    # little-endian samples reach the volume's dtype as they are
    from vpt_amd.volume import device_format

    class Gl:
        def extension_enabled(self, name):
            return True
    samples = np.array([-1000, 3000, 0, 17], '<i2')
    r = vpt_amd.RAWReader(samples.tobytes(), {'width': 4, 'height': 1, 'depth': 1, 'bits': 16, 'signed': True})
    fmt, nch, dtype = device_format(r.readMetadata()['modalities'][0], Gl())
    assert (fmt, nch) == (N.FORMAT_R16_SNORM, 1) and np.frombuffer(bytes(r.readBlock(0)), dtype).tolist() == [-1000, 3000, 0, 17]
    assert struct.unpack('<4h', bytes(r.readBlock(0))) == (-1000, 3000, 0, 17)


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_raw_reader_honours_bits_and_signed():
    out = subprocess.run(["node", os.path.join(ROOT, "js", "test", "test_raw_bits.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and "js raw bits ok" in out.stdout.decode(), out.stdout.decode()


def test_symbols_resolve_and_null_handles_are_invalid_without_a_device():
    L = N.lib()
    for name in ("vpt_volume_window", "vpt_volume_range", "vpt_volume_code_histogram"):
        assert hasattr(L, name) and name in N.SYMBOLS
    out = C.c_void_p()
    assert L.vpt_volume_window(None, 0.0, 1.0, N.FORMAT_R8, C.byref(out)) == N.ERR_INVALID
    assert b"null" in L.vpt_last_error()
    lo, hi = C.c_double(), C.c_double()
    assert L.vpt_volume_range(None, C.byref(lo), C.byref(hi)) == N.ERR_INVALID
    buf = (C.c_uint32 * 256)()
    assert L.vpt_volume_code_histogram(None, buf, 256) == N.ERR_INVALID
    assert vpt_amd.window_texels is not None and vpt_amd.percentile_window is not None
