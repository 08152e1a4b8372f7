"""Two volumes of one grid combined texel by texel, or compared, on the host: the numpy statement of the contract the device kernels
(vpt_volume_combine, vpt_volume_compare; include/vpt.h) are held to, for callers without a device and as the contract's documentation.

``a`` is a [depth][height][width] uint8 or uint16 array, ``b`` one of the same shape, or [depth][height][width][2] with ``channel`` naming
the channel that is read.  A and B are the whole unsigned codes, M = 255 / 65535 the largest code of a's type, Mb that of b's.

  mask:     A where lo <= B <= hi, ``fill`` elsewhere.  b may be 8- or 16-bit whatever a is.  lo <= hi <= Mb, fill <= M.
  min, max, absdiff:  min(A, B), max(A, B), |A - B|.
  blend:    clamp(((wa A + wb B + 128) >> 8) + offset, 0, M): wa, wb in 1/256 units in -4096 .. 4096, offset in -65535 .. 65535.  >> is the
            arithmetic shift: floor(x / 256 + 1 / 2), a half rounds up.  |wa A + wb B + 128| < 2^31.
  pair:     (A, B) as a [depth][height][width][2] array of a's type.
Every op but mask needs b to have a's type.

compare_stats gives the eight exact integers of vpt_volume_compare and the ratios a host derives from them in IEEE double."""
import math

import numpy as np

OPS = {'mask': 0, 'min': 1, 'max': 2, 'absdiff': 3, 'blend': 4, 'pair': 5}
MAX_WEIGHT = 4096
MAX_OFFSET = 65535
STATS = ('voxels', 'differing', 'max_abs', 'sum_abs', 'sum_sq', 'in_a', 'in_b', 'both')


def _integer(value):
    return isinstance(value, (int, np.integer)) and not isinstance(value, bool)


def check_op(op):
    """the code of 'mask' | 'min' | 'max' | 'absdiff' | 'blend' | 'pair' (VPT_COMBINE_*); raises ValueError otherwise"""
    if not isinstance(op, str) or op not in OPS:
        raise ValueError("combine op is 'mask', 'min', 'max', 'absdiff', 'blend' or 'pair', not %r" % (op,))
    return OPS[op]


def check_channel(channel, channels):
    """``channel`` of a volume of ``channels`` channels as an int: 0, or 1 for a two-channel volume; raises ValueError otherwise"""
    if not _integer(channel) or channel not in (0, 1):
        raise ValueError('combine channel is 0 or 1, not %r' % (channel,))
    if channel == 1 and channels != 2:
        raise ValueError('combine channel 1 needs a two-channel second volume')
    return int(channel)


def check_weights(wa, wb, offset=0):
    """(wa, wb, offset) of a blend as ints: the weights in -4096 .. 4096 (1/256 units), the offset in -65535 .. 65535; raises ValueError
    otherwise"""
    for name, w in (('wa', wa), ('wb', wb)):
        if not _integer(w) or not -MAX_WEIGHT <= w <= MAX_WEIGHT:
            raise ValueError('blend weight %s is an integer in -%d .. %d (1/256 units), not %r' % (name, MAX_WEIGHT, MAX_WEIGHT, w))
    if not _integer(offset) or not -MAX_OFFSET <= offset <= MAX_OFFSET:
        raise ValueError('blend offset is an integer in -%d .. %d, not %r' % (MAX_OFFSET, MAX_OFFSET, offset))
    return int(wa), int(wb), int(offset)


def check_mask(lo, hi, fill, largest_b, largest_a):
    """(lo, hi, fill) of a mask as ints: 0 <= lo <= hi <= ``largest_b`` and 0 <= fill <= ``largest_a``; raises ValueError otherwise"""
    if not _integer(lo) or not _integer(hi) or not 0 <= lo <= hi <= largest_b:
        raise ValueError('mask range [%r, %r]: integers with 0 <= lo <= hi <= %d' % (lo, hi, largest_b))
    if not _integer(fill) or not 0 <= fill <= largest_a:
        raise ValueError('mask fill is an integer in 0 .. %d, not %r' % (largest_a, fill))
    return int(lo), int(hi), int(fill)


def check_compare_range(rng, largest, which):
    """(lo, hi) of a compare range (None: every code) as ints in 0 .. 2^32 - 1 with lo <= hi; raises ValueError otherwise"""
    if rng is None:
        return 0, largest
    if isinstance(rng, (str, bytes)) or not hasattr(rng, '__len__') or len(rng) != 2 or not all(_integer(v) for v in rng) \
            or not 0 <= rng[0] <= rng[1] <= 0xFFFFFFFF:
        raise ValueError('compare %s is None or (lo, hi), integers with 0 <= lo <= hi, not %r' % (which, rng))
    return int(rng[0]), int(rng[1])


def _sources(a, b, channel):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim != 3:
        raise ValueError('the first volume is a [depth][height][width] uint8 or uint16 array')
    if b.dtype not in (np.uint8, np.uint16) or b.ndim not in (3, 4) or (b.ndim == 4 and b.shape[3] != 2):
        raise ValueError('the second volume is a [depth][height][width] or [depth][height][width][2] uint8 or uint16 array')
    if a.shape != b.shape[:3]:
        raise ValueError('the volumes differ in size: %r and %r' % (a.shape, b.shape[:3]))
    channel = check_channel(channel, 2 if b.ndim == 4 else 1)
    return a, (b[..., channel] if b.ndim == 4 else b)


def combine_texels(a, b, op, channel=0, lo=0, hi=None, fill=0, wa=256, wb=0, offset=0):
    """the texels vpt_volume_combine gives for the arrays ``a`` and ``b`` (module docstring); ``hi`` None: b's largest code"""
    code = check_op(op)
    a, b = _sources(a, b, channel)
    largest, largest_b = int(np.iinfo(a.dtype).max), int(np.iinfo(b.dtype).max)
    if op == 'mask':
        lo, hi, fill = check_mask(lo, largest_b if hi is None else hi, fill, largest_b, largest)
        return np.where((b >= lo) & (b <= hi), a, a.dtype.type(fill))
    if a.dtype != b.dtype:
        raise ValueError("combine op %r needs volumes of one width, not %s and %s; only 'mask' takes both" % (op, a.dtype, b.dtype))
    if op == 'min':
        return np.minimum(a, b)
    if op == 'max':
        return np.maximum(a, b)
    if op == 'absdiff':
        return np.maximum(a, b) - np.minimum(a, b)
    if op == 'pair':
        return np.stack([a, b], axis=-1)
    assert code == OPS['blend']
    wa, wb, offset = check_weights(wa, wb, offset)
    s = ((wa * a.astype(np.int64) + wb * b.astype(np.int64) + 128) >> 8) + offset      # numpy's >> of a signed integer is arithmetic
    return np.clip(s, 0, largest).astype(a.dtype)


def ratios(stats, largest):
    """{'dice', 'jaccard', 'mse', 'psnr'} from the eight integers, in IEEE double; None where a denominator is 0 (psnr: where mse is 0).
    ``largest``: the peak of the PSNR, the largest code of the wider of the two volumes"""
    voxels, in_a, in_b, both, sum_sq = (int(stats[k]) for k in ('voxels', 'in_a', 'in_b', 'both', 'sum_sq'))
    union = in_a + in_b - both
    mse = sum_sq / voxels if voxels else None
    return {'dice': 2 * both / (in_a + in_b) if in_a + in_b else None,
            'jaccard': both / union if union else None,
            'mse': mse,
            'psnr': 10.0 * math.log10(largest * largest / mse) if mse else None}


def compare_stats(a, b, a_range=None, b_range=None, channel=0):
    """the dict of vpt_volume_compare's eight exact integers (STATS) for the arrays ``a`` and ``b`` (mixed widths are taken), plus
    'dice' = 2 both / (in_a + in_b), 'jaccard' = both / (in_a + in_b - both), 'mse' = sum_sq / voxels and 'psnr' = 10 log10(peak^2 / mse)
    with the peak of the wider volume; a ratio whose denominator is 0 is None.  A range None takes every code."""
    a, b = _sources(a, b, channel)
    largest_a, largest_b = int(np.iinfo(a.dtype).max), int(np.iinfo(b.dtype).max)
    lo_a, hi_a = check_compare_range(a_range, largest_a, 'a_range')
    lo_b, hi_b = check_compare_range(b_range, largest_b, 'b_range')
    d = np.abs(a.astype(np.int64) - b.astype(np.int64))
    ia, ib = (a >= lo_a) & (a <= hi_a), (b >= lo_b) & (b <= hi_b)
    out = {'voxels': int(a.size), 'differing': int(np.count_nonzero(d)), 'max_abs': int(d.max()) if d.size else 0,
           'sum_abs': int(d.sum(dtype=np.uint64)), 'sum_sq': int((d.astype(np.uint64) ** 2).sum(dtype=np.uint64)),
           'in_a': int(np.count_nonzero(ia)), 'in_b': int(np.count_nonzero(ib)), 'both': int(np.count_nonzero(ia & ib))}
    out.update(ratios(out, max(largest_a, largest_b)))
    return out
