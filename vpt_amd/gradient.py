"""The gradient-magnitude channel of a one-channel volume, on the host: the numpy statement of the contract the device kernel
(vpt_volume_derive_gradient, include/vpt.h) is held to, for callers without a device and as the contract's documentation.

All in integers.  v = the texel (uint8: B = 8, uint16: B = 16), indices clamped per axis (CLAMP_TO_EDGE):

  'central': dx = v(x+1,y,z) - v(x-1,y,z), likewise dy, dz (doubled central differences);            shift = 16
  'sobel':   dx = sum_{a,b in -1..1} w(a) w(b) (v(x+1,y+a,z+b) - v(x-1,y+a,z+b)), w = (1, 2, 1), ...;  shift = 24
  S = dx^2 + dy^2 + dz^2;  q = floor(gain^2 * 16384 + 0.5) from the float32 gain, 1 <= q <= 4194304 (gain 1/128 .. 16)
  T = (S * q) >> shift;  G = min(2^B - 1, floor(sqrt(T)))

With gain = 1, G = floor(|grad v|) in texel units per voxel for both operators."""
import math

import numpy as np

OPERATORS = {'central': 0, 'sobel': 1}


def operator_code(operator):
    """VPT_GRADIENT_* of an operator name ('central' | 'sobel') or code"""
    if operator in OPERATORS:
        return OPERATORS[operator]
    if operator in (0, 1) and not isinstance(operator, bool):
        return int(operator)
    raise ValueError("unknown gradient operator %r ('central' or 'sobel')" % (operator,))


def gain_factor(gain):
    """q = floor(gain^2 * 16384 + 0.5), in double from the gain rounded to float32 (what crosses the C ABI); raises outside [1, 4194304]"""
    g = float(np.float32(gain))
    q = math.floor(g * g * 16384.0 + 0.5) if math.isfinite(g) else 0
    if not 1 <= q <= 4194304:
        raise ValueError('gradient gain %r outside [1/128, 16]' % (gain,))
    return int(q)


def _isqrt(t):
    """floor(sqrt(t)) of a uint64 array, exact for t < 2^53: a float64 estimate and one integer correction each way"""
    r = np.sqrt(t.astype(np.float64)).astype(np.uint64)
    r = np.where(r * r > t, r - np.uint64(1), r)
    r1 = r + np.uint64(1)
    return np.where(r1 * r1 <= t, r1, r)


def gradient_magnitude(array, operator='central', gain=1.0):
    """G of a [depth][height][width] uint8 or uint16 array, in the array's dtype (the second channel
    ``Volume.derive_gradient(operator, gain)`` puts beside it on the device, byte for byte)."""
    array = np.asarray(array)
    if array.dtype not in (np.uint8, np.uint16) or array.ndim != 3:
        raise ValueError('the gradient magnitude is derived from a [depth][height][width] uint8 or uint16 array')
    op = operator_code(operator)
    q = gain_factor(gain)
    top = np.uint64(np.iinfo(array.dtype).max)
    p = np.pad(array.astype(np.int64), 1, mode='edge')                        # p[z+1, y+1, x+1] = v(x, y, z), clamped
    d, h, w = array.shape

    def sl(axis, o):                                                          # the volume shifted by o along one axis
        i = [slice(1, d + 1), slice(1, h + 1), slice(1, w + 1)]
        i[axis] = slice(1 + o, 1 + o + array.shape[axis])
        return tuple(i)

    if op == 0:
        diffs = [p[sl(ax, 1)] - p[sl(ax, -1)] for ax in range(3)]
        shift = 16
    else:
        def smooth(a, axis):                                                  # (1, 2, 1) along `axis` of a padded array (its ends are not used)
            out = 2 * a
            lo = [slice(None)] * 3; hi = [slice(None)] * 3; mid = [slice(None)] * 3
            lo[axis] = slice(0, -2); hi[axis] = slice(2, None); mid[axis] = slice(1, -1)
            out[tuple(mid)] += a[tuple(lo)] + a[tuple(hi)]
            return out
        diffs = []
        for ax in range(3):
            s = p
            for other in range(3):
                if other != ax:
                    s = smooth(s, other)
            diffs.append(s[sl(ax, 1)] - s[sl(ax, -1)])
        shift = 24
    S = sum((g * g).astype(np.uint64) for g in diffs)
    T = (S * np.uint64(q)) >> np.uint64(shift)
    return np.minimum(_isqrt(T), top).astype(array.dtype)
