"""The rank filters of a volume over the 3 x 3 x 3 box, on the host: the numpy statement of the contract the device kernels (vpt_volume_rank;
include/vpt.h) are held to, for callers without a device and as the contract's documentation.

uint8 and uint16 [depth][height][width] arrays, v = the texel code, indices clamped per axis; the neighbourhood of a texel is the 27 clamped
taps v(x + a, y + b, z + c), a, b, c in {-1, 0, 1}, as a multiset (a clamped tap counts as often as it occurs).  One pass:

  'median':  the 14th smallest of the 27 taps;   'erode':  the smallest;   'dilate':  the largest      (unsigned compares of whole codes)

p passes apply the pass p times; 'open' is p erosions, then p dilations; 'close' p dilations, then p erosions."""
import numpy as np

from .pyramid import MAX_PASSES

OPERATORS = ('median', 'erode', 'dilate', 'open', 'close')          # index = VPT_RANK_* (include/vpt.h)


def operator_code(name):
    """VPT_RANK_* of 'median' | 'erode' | 'dilate' | 'open' | 'close'; raises ValueError otherwise"""
    if not isinstance(name, str) or name not in OPERATORS:
        raise ValueError("a rank operator is 'median', 'erode', 'dilate', 'open' or 'close', not %r" % (name,))
    return OPERATORS.index(name)


def check_passes(passes):
    """the number of rank-filter passes, an integer in 1 .. 8 (pyramid.check_passes' rule); raises ValueError otherwise"""
    if isinstance(passes, bool) or not isinstance(passes, (int, np.integer)) or not 1 <= passes <= MAX_PASSES:
        raise ValueError('rank-filter passes are an integer in 1 .. %d, not %r' % (MAX_PASSES, passes))
    return int(passes)


def _taps(v):
    """[27][depth][height][width]: the clamped taps of every texel"""
    p = np.pad(v, 1, mode='edge')
    d, h, w = v.shape
    return np.stack([p[c:c + d, b:b + h, a:a + w] for c in range(3) for b in range(3) for a in range(3)])


def _pass(v, kind):
    taps = _taps(v)
    if kind == 'erode':
        return taps.min(axis=0)
    if kind == 'dilate':
        return taps.max(axis=0)
    return np.partition(taps, 13, axis=0)[13]


def rank_texels(array, op, passes=1):
    """``passes`` applications of a rank operator over the clamped 3 x 3 x 3 box to a [depth][height][width] uint8 or uint16 array, in the
    array's dtype: what ``Volume.rank(op, passes)`` holds on the device, byte for byte."""
    array = np.asarray(array)
    if array.dtype not in (np.uint8, np.uint16) or array.ndim != 3 or 0 in array.shape:
        raise ValueError('the rank filters take a [depth][height][width] uint8 or uint16 array')
    name = OPERATORS[operator_code(op)]
    passes = check_passes(passes)
    sequence = {'open': ('erode', 'dilate'), 'close': ('dilate', 'erode')}.get(name, (name,))
    v = array
    for kind in sequence:
        for _ in range(passes):
            v = _pass(v, kind)
    return np.ascontiguousarray(v, dtype=array.dtype)
