"""The value-range window (window / level) of a one-channel volume, on the host: the numpy statement of the two contracts the device
kernel (vpt_volume_window, include/vpt.h) is held to, for callers without a device and as the contracts' documentation.

The result is a uint8 (bits = 8, M = 255) or uint16 (bits = 16, M = 65535) array: 0 at or below ``lo``, M at or above ``hi``.

Integer arrays (uint8, uint16, int8, int16).  The code c is the stored integer, for the signed types with the most negative code
read as the one above it (SNORM: max(c, -(2^(B-1) - 1))).  ``lo``, ``hi`` integers, |lo|, |hi| <= 2^31, D = hi - lo >= 1, n = c - lo:

    out = 0 if n <= 0;  M if n >= D;  (2 n M + D) // (2 D) otherwise                    (round half up)

float32 arrays.  ``lo``, ``hi`` and ``hi - lo`` finite, hi > lo; every operation one IEEE double operation:

    t = (double(v) - lo) / (hi - lo);  out = 0 if not t > 0 (NaN, -inf);  M if t >= 1;  else floor(t * M + 0.5)"""
import math
from fractions import Fraction

import numpy as np

FORMATS = {'r8': 8, 'r16': 16}
_INTEGER = (np.uint8, np.uint16, np.int8, np.int16)


def format_bits(format):
    """8 or 16 from a result format name ('r8' | 'r16') or bit count"""
    if format in FORMATS:
        return FORMATS[format]
    if format in (8, 16) and not isinstance(format, bool):
        return int(format)
    raise ValueError("a windowed volume is 'r8' or 'r16', not %r" % (format,))


def check_window(dtype, lo, hi):
    """(lo, hi) as the contract takes them for texels of ``dtype`` (Python ints, or floats for float32); raises ValueError otherwise"""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        lo, hi = float(lo), float(hi)
        if not (math.isfinite(lo) and math.isfinite(hi) and math.isfinite(hi - lo) and hi > lo):
            raise ValueError('window [%r, %r] of float texels: lo, hi and hi - lo must be finite and hi > lo' % (lo, hi))
        return lo, hi
    if dtype.type not in _INTEGER:
        raise ValueError('a window is taken from uint8, uint16, int8, int16 or float32 texels, not %s' % dtype)
    if isinstance(lo, float) and not (math.isfinite(lo) and lo == math.floor(lo)) or isinstance(hi, float) and not (math.isfinite(hi) and hi == math.floor(hi)):
        raise ValueError('window [%r, %r] of integer texels: lo and hi must be integers' % (lo, hi))
    lo, hi = int(lo), int(hi)
    if abs(lo) > 2 ** 31 or abs(hi) > 2 ** 31 or hi - lo < 1:
        raise ValueError('window [%d, %d] of integer texels: lo and hi must lie in [-2^31, 2^31] with hi - lo >= 1' % (lo, hi))
    return lo, hi


def window_texels(array, lo, hi, bits=8):
    """The windowed texels of a uint8 / uint16 / int8 / int16 / float32 array of any shape, as uint8 (bits = 8) or uint16 (bits = 16):
    what ``Volume.window(lo, hi, format)`` holds on the device, byte for byte."""
    array = np.asarray(array)
    bits = format_bits(bits)
    lo, hi = check_window(array.dtype, lo, hi)
    M = (1 << bits) - 1
    out_dtype = np.uint8 if bits == 8 else np.uint16
    if array.dtype == np.float32:
        with np.errstate(all='ignore'):
            t = (array.astype(np.float64) - np.float64(lo)) / np.float64(hi - lo)
            inside = np.floor(np.minimum(np.maximum(t, 0.0), 1.0) * np.float64(M) + 0.5)      # the value is only used where 0 < t < 1
            inside = np.where(np.isnan(inside), 0.0, inside)
            out = np.where(~(t > 0), 0.0, np.where(t >= 1, np.float64(M), inside))
        return out.astype(out_dtype)
    c = array.astype(np.int64)
    if array.dtype.kind == 'i':
        c = np.maximum(c, -(np.iinfo(array.dtype).max))
    D = hi - lo
    n = np.clip(c - lo, 0, D)                                     # n = 0 and n = D give 0 and M by the formula itself
    return ((2 * n * M + D) // (2 * D)).astype(out_dtype)


def percentile_window(histogram, p_lo=0.5, p_hi=99.5, signed=False):
    """(lo, hi) in code units from a full-resolution code histogram (``Volume.code_histogram()``: 256 or 65536 bins; ``signed``: bin =
    code + 2^(B-1)).  With N = sum(bins) and cum(k) the inclusive cumulative count, lo = the smallest code with cum >= max(1, ceil(N p_lo / 100)),
    hi = the smallest code with cum >= max(1, ceil(N p_hi / 100)), then hi = max(hi, lo + 1).  Integers only (the percentiles are taken as the
    exact rationals of their floating-point values)."""
    bins = np.asarray(histogram).reshape(-1)
    if bins.size not in (256, 65536):
        raise ValueError('a code histogram has 256 or 65536 bins, not %d' % bins.size)
    if not (0 <= p_lo <= 100 and 0 <= p_hi <= 100 and p_lo <= p_hi):
        raise ValueError('percentiles %r, %r: 0 <= p_lo <= p_hi <= 100' % (p_lo, p_hi))
    cum = np.cumsum(bins.astype(np.int64))
    N = int(cum[-1])
    if N == 0:
        raise ValueError('the histogram is empty')
    bias = bins.size // 2 if signed else 0

    def code(p):
        need = max(1, math.ceil(Fraction(p) * N / 100))
        return int(np.searchsorted(cum, need, side='left')) - bias
    lo, hi = code(p_lo), code(p_hi)
    return lo, max(hi, lo + 1)
