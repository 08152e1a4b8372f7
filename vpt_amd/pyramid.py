"""A volume's next coarser level and its binomial smoothing, on the host: the numpy statement of the two contracts the device kernels
(vpt_volume_reduce, vpt_volume_smooth; include/vpt.h) are held to, for callers without a device and as the contracts' documentation.

Reduction.  A [depth][height][width] array, or [depth][height][width][2] for two channels, gives ceil(n / 2) texels per axis.  Result
texel (X, Y, Z) is taken per channel from the eight texels at x in {2 X, min(2 X + 1, nx - 1)}, likewise y and z (on an odd axis the last
cell counts its last texel twice):

  uint8, uint16, int8, int16:  out = (sum of the eight codes + 4) >> 3, an arithmetic shift (floor of the mean, halves rounded up); the
                               code is the stored integer, for the signed types the most negative one read as the one above it (SNORM)
  float32:                     doubles, ((a000 + a100) + (a010 + a110)) + ((a001 + a101) + (a011 + a111)) (a_xyz), times 0.125, rounded
                               once to float32

Smoothing.  uint8 and uint16 [depth][height][width] arrays, indices clamped per axis, w = (1, 2, 1):

  W = sum over a, b, c in {-1, 0, 1} of w(a) w(b) w(c) v(x + a, y + b, z + c);  out = (W + 32) >> 6;  p passes apply this p times"""
import numpy as np

_INTEGER = (np.uint8, np.uint16, np.int8, np.int16)
MAX_PASSES = 8


def check_passes(passes):
    """the number of smoothing passes, an integer in 1 .. 8; raises ValueError otherwise"""
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or not 1 <= passes <= MAX_PASSES:
        raise ValueError('smoothing passes are an integer in 1 .. %d, not %r' % (MAX_PASSES, passes))
    return int(passes)


def check_levels(levels):
    """the number of reductions, an integer >= 1; raises ValueError otherwise"""
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or levels < 1:
        raise ValueError('reduction levels are an integer >= 1, not %r' % (levels,))
    return int(levels)


def reduced_shape(shape):
    """ceil(n / 2) per spatial axis of a (depth, height, width[, 2]) shape"""
    return tuple((n + 1) // 2 for n in shape[:3]) + tuple(shape[3:])


def reduce_texels(array):
    """The next coarser level of a uint8 / uint16 / int8 / int16 / float32 [depth][height][width] or [depth][height][width][2] array, in
    the array's dtype: what ``Volume.reduce()`` holds on the device, byte for byte (NaN results: some NaN)."""
    array = np.asarray(array)
    if array.ndim not in (3, 4) or (array.ndim == 4 and array.shape[3] != 2) or 0 in array.shape:
        raise ValueError('a volume is reduced from a [depth][height][width] or [depth][height][width][2] array')
    if array.dtype != np.float32 and array.dtype.type not in _INTEGER:
        raise ValueError('a volume is reduced from uint8, uint16, int8, int16 or float32 texels, not %s' % array.dtype)
    d, h, w = array.shape[:3]

    def taps(n):                                                  # (2 X, min(2 X + 1, n - 1)) for X in 0 .. ceil(n / 2) - 1
        first = np.arange(0, n, 2)
        return first, np.minimum(first + 1, n - 1)
    zs, ys, xs = taps(d), taps(h), taps(w)

    def a(i, j, k):                                               # a_ijk: the texels at x tap i, y tap j, z tap k
        return wide[zs[k]][:, ys[j]][:, :, xs[i]]
    if array.dtype == np.float32:
        wide = array.astype(np.float64)
        with np.errstate(all='ignore'):
            s = ((a(0, 0, 0) + a(1, 0, 0)) + (a(0, 1, 0) + a(1, 1, 0))) + ((a(0, 0, 1) + a(1, 0, 1)) + (a(0, 1, 1) + a(1, 1, 1)))
            return (s * np.float64(0.125)).astype(np.float32)
    wide = array.astype(np.int64)
    if array.dtype.kind == 'i':
        wide = np.maximum(wide, -np.iinfo(array.dtype).max)
    s = sum(a(i, j, k) for k in (0, 1) for j in (0, 1) for i in (0, 1))
    return ((s + 4) >> 3).astype(array.dtype)


def smooth_texels(array, passes=1):
    """``passes`` applications of the binomial 3 x 3 x 3 kernel to a [depth][height][width] uint8 or uint16 array, in the array's dtype: what
    ``Volume.smooth(passes)`` holds on the device, byte for byte."""
    array = np.asarray(array)
    if array.dtype not in (np.uint8, np.uint16) or array.ndim != 3 or 0 in array.shape:
        raise ValueError('a [depth][height][width] uint8 or uint16 array is smoothed')
    v = array.astype(np.int64)
    for _ in range(check_passes(passes)):
        for axis in range(3):                                     # the sum is exact, so it is taken axis by axis; one rounding at the end
            p = np.pad(v, [(1, 1) if ax == axis else (0, 0) for ax in range(3)], mode='edge')
            n = v.shape[axis]
            cut = lambda o: tuple(slice(o, o + n) if ax == axis else slice(None) for ax in range(3))
            v = p[cut(0)] + 2 * p[cut(1)] + p[cut(2)]
        v = (v + 32) >> 6
    return v.astype(array.dtype)
