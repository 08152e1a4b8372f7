"""The exact squared Euclidean distance of every voxel to the nearest voxel of a value range of a volume (or of its complement), on the
host: the numpy statement of the contract the device kernels (vpt_volume_distance and the vpt_distance_* family; include/vpt.h) are held
to, for callers without a device and as the contract's documentation.

uint8 and uint16 [depth][height][width] arrays, c = the texel code.

  in range:  lo <= c <= hi, compared as whole unsigned codes
  seeds:     'range': the voxels in range (the distance TO the structure, 0 on it); 'rest': the voxels not in range (the depth INSIDE the
             structure, 0 outside it)
  d2:        of a voxel v: the minimum over the seeds s of (vx - sx)^2 + (vy - sy)^2 + (vz - sz)^2, uint32; nothing wraps, nothing is
             clamped: voxels outside the array are neither seed nor non-seed; NONE = 0xFFFFFFFF everywhere when there is no seed

within:   the code where r2_lo <= d2 <= r2_hi, `fill` elsewhere (NONE is an ordinary value of d2: only r2_hi = 0xFFFFFFFF selects it).
channel:  (code, min(isqrt(steps^2 d2), M)), isqrt the exact integer square root, M = 255 / 65535."""
import math

import numpy as np

NONE = 0xFFFFFFFF
SEEDS = {'range': 0, 'rest': 1}
_FAR = 1 << 40                                                  # beyond every sum of a finite d2 and a squared offset


def _whole(value, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s is an integer, not %r' % (what, value))
    return int(value)


def check_seeds(seeds):
    """the code of 'range' (0: VPT_DISTANCE_TO_RANGE) or 'rest' (1: VPT_DISTANCE_TO_REST); raises ValueError otherwise"""
    if not isinstance(seeds, str) or seeds not in SEEDS:
        raise ValueError("seeds is 'range' or 'rest', not %r" % (seeds,))
    return SEEDS[seeds]


def check_range(lo, hi, largest):
    """(lo, hi) of a distance range in code units: integers with 0 <= lo <= hi <= largest; raises ValueError otherwise"""
    lo, hi = _whole(lo, 'the lower end of a distance range'), _whole(hi, 'the upper end of a distance range')
    if not 0 <= lo <= hi <= largest:
        raise ValueError('distance range [%d, %d]: 0 <= lo <= hi <= %d' % (lo, hi, largest))
    return lo, hi


def check_steps(steps):
    """the transfer-function rows per voxel of distance, an integer in 1 .. 256; raises ValueError otherwise"""
    steps = _whole(steps, 'steps')
    if not 1 <= steps <= 256:
        raise ValueError('steps is in 1 .. 256, not %d' % steps)
    return steps


def check_radius(radius):
    """floor(radius^2), taken in IEEE double, of a non-negative finite radius, at most 2^32 - 2 (the largest squared distance that is not
    NONE: a larger radius selects what that one selects); raises ValueError otherwise"""
    if isinstance(radius, (bool, str)) or not isinstance(radius, (int, float, np.integer, np.floating)):
        raise ValueError('radius is a number, not %r' % (radius,))
    radius = float(radius)
    if not (math.isfinite(radius) and radius >= 0.0):
        raise ValueError('radius is finite and not negative, not %r' % (radius,))
    square = radius * radius
    return NONE - 1 if square >= float(NONE - 1) else int(math.floor(square))


def check_within(r2_lo, r2_hi, fill, largest):
    """(r2_lo, r2_hi, fill) of a selection: 0 <= r2_lo <= r2_hi < 2^32 (r2_hi None: 0xFFFFFFFF, NONE included), 0 <= fill <= largest;
    raises ValueError otherwise"""
    r2_lo = _whole(r2_lo, 'the smallest squared distance kept')
    r2_hi = NONE if r2_hi is None else _whole(r2_hi, 'the largest squared distance kept')
    fill = _whole(fill, 'fill')
    if not 0 <= r2_lo <= r2_hi <= NONE:
        raise ValueError('squared distances %d .. %d: 0 <= from <= to < 2^32 is required' % (r2_lo, r2_hi))
    if not 0 <= fill <= largest:
        raise ValueError('fill %d: the largest code is %d' % (fill, largest))
    return r2_lo, r2_hi, fill


def _texels(array):
    array = np.asarray(array)
    if array.dtype not in (np.uint8, np.uint16) or array.ndim != 3 or 0 in array.shape:
        raise ValueError('the distance transform takes a [depth][height][width] uint8 or uint16 array')
    return array


def _along(g, axis):
    """out[i] = min over j of g[j] + (i - j)^2 along `axis` (int64; _FAR and beyond: no seed on the line)"""
    g = np.moveaxis(g, axis, -1)
    shape = g.shape
    m = shape[-1]
    lines = g.reshape(-1, m)
    offsets = np.arange(m, dtype=np.int64)
    squares = (offsets[:, None] - offsets[None, :]) ** 2        # [i][j]
    out = np.empty_like(lines)
    chunk = max(1, (1 << 22) // (m * m))
    for first in range(0, len(lines), chunk):
        out[first:first + chunk] = (lines[first:first + chunk, None, :] + squares[None]).min(axis=-1)
    return np.moveaxis(out.reshape(shape), -1, axis)


def distance_squared_texels(array, lo, hi, seeds='range'):
    """uint32 [depth][height][width]: the squared distance of every voxel of a uint8 or uint16 array to the nearest voxel whose code is
    (seeds 'range') or is not (seeds 'rest') in lo .. hi; 0xFFFFFFFF everywhere without a seed: what ``Volume.distance(...)`` holds on the
    device."""
    array = _texels(array)
    lo, hi = check_range(lo, hi, int(np.iinfo(array.dtype).max))
    rest = check_seeds(seeds) == 1
    if max(array.shape) > 4096:
        raise ValueError('the distance transform takes at most 4096 voxels an axis')
    seed = ((array >= lo) & (array <= hi)) != rest
    g = np.where(seed, np.int64(0), np.int64(_FAR))
    for axis in (2, 1, 0):                                      # x, y, z: the order changes nothing, the minimum is over all seeds
        g = _along(g, axis)
    return np.ascontiguousarray(np.where(g >= _FAR, NONE, g), dtype=np.uint32)


def _squared(array, d2):
    d2 = np.asarray(d2)
    if d2.shape != array.shape or d2.dtype.kind not in 'ui':
        raise ValueError('squared distances are one unsigned integer per voxel of the array')
    return d2.astype(np.uint64)


def within_texels(array, d2, r2_lo=0, r2_hi=None, fill=0):
    """the array's codes where r2_lo <= d2 <= r2_hi (r2_hi None: 0xFFFFFFFF), ``fill`` elsewhere, in the array's dtype: what
    ``Distance.within(r2_lo, r2_hi, fill)`` holds on the device."""
    array = _texels(array)
    r2_lo, r2_hi, fill = check_within(r2_lo, r2_hi, fill, int(np.iinfo(array.dtype).max))
    d2 = _squared(array, d2)
    kept = (d2 >= np.uint64(r2_lo)) & (d2 <= np.uint64(r2_hi))
    return np.ascontiguousarray(np.where(kept, array, array.dtype.type(fill)), dtype=array.dtype)


def isqrt_texels(p):
    """floor(sqrt(p)) of a uint64 array with p < 2^53, exactly: the double square root is within one of it"""
    p = np.asarray(p, dtype=np.uint64)
    r = np.floor(np.sqrt(p.astype(np.float64))).astype(np.uint64)
    r = r - (r * r > p).astype(np.uint64)
    return r + ((r + np.uint64(1)) * (r + np.uint64(1)) <= p).astype(np.uint64)


def channel_texels(array, d2, steps=1):
    """[depth][height][width][2] in the array's dtype: (code, min(isqrt(steps^2 d2), M)), M the dtype's largest code: what
    ``Distance.channel(steps)`` holds on the device.  Distances beyond M / steps voxels, and NONE, share the last row of the 2-D transfer
    function."""
    array = _texels(array)
    steps = check_steps(steps)
    d2 = _squared(array, d2)
    if d2.size and int(d2.max()) > NONE:
        raise ValueError('squared distances are below 2^32')
    g = np.minimum(isqrt_texels(np.uint64(steps * steps) * d2), np.uint64(np.iinfo(array.dtype).max)).astype(array.dtype)
    return np.ascontiguousarray(np.stack([array, g], axis=-1))


_PAIRS = 1 << 21                                                # voxel-centre pairs looked at in one piece


def _covered(shape, centres, values, voxels):
    """of the voxels (flat indices): which lie in the open ball { |v - c|^2 < D_c } of one of the centres ([k][3] z, y, x; D_c = values):
    the distance to the set of centres, each lowered by its D_c, is below 0.  Only the box of the voxels, widened by the largest radius, is
    looked at: no ball from outside it reaches a voxel."""
    z, y, x = np.unravel_index(voxels, shape)
    reach = int(math.isqrt(int(values.max()))) + 1
    first = [max(int(a.min()) - reach, 0) for a in (z, y, x)]
    last = [min(int(a.max()) + reach + 1, m) for a, m in zip((z, y, x), shape)]
    inside = np.all((centres >= first) & (centres < last), axis=1)
    g = np.full([b - a for a, b in zip(first, last)], np.int64(_FAR))
    c = centres[inside] - first
    np.minimum.at(g, (c[:, 0], c[:, 1], c[:, 2]), -values[inside])
    for axis in (2, 1, 0):
        g = _along(g, axis)
    return g[z - first[0], y - first[1], x - first[2]] < 0


def _cover(shape, out, centres, values, voxels):
    """out[v] = the largest D_c among the balls that hold v, for the voxels (flat indices) that some ball holds; `values` is descending.
    Few pairs are looked at one by one.  Otherwise the centres are halved: a voxel that a ball of the upper half holds has its maximum
    there (every value of the lower half is no larger), every other voxel has it in the lower half or nowhere: the level sets
    { T2 >= t } = the union of the balls with D >= t, asked for the middle value first."""
    if not len(voxels) or not len(values):
        return
    if len(voxels) * len(values) <= _PAIRS or len(values) == 1:
        piece = max(1, _PAIRS // len(values))
        for first in range(0, len(voxels), piece):
            v = voxels[first:first + piece]
            at = np.stack(np.unravel_index(v, shape), axis=-1).astype(np.int64)
            held = ((at[:, None, :] - centres[None, :, :]) ** 2).sum(axis=-1) < values[None, :]
            out[v] = np.where(held, values[None, :], 0).max(axis=1)
        return
    half = len(values) // 2
    upper = _covered(shape, centres[:half], values[:half], voxels)
    _cover(shape, out, centres[:half], values[:half], voxels[upper])
    _cover(shape, out, centres[half:], values[half:], voxels[~upper])


def thickness_squared_texels(d2):
    """uint32 [depth][height][width]: the squared local thickness T2 of squared distances d2 (``distance_squared_texels``): a voxel c with
    d2(c) > 0 is a centre, its ball the voxels v of the array with |v - c|^2 < d2(c) (open: it holds no seed), and T2(v) is the largest
    d2(c) among the balls that hold v, 0 when none does: what ``Distance.thickness()`` holds on the device.  By level sets: for each
    distinct value t of d2, descending, the voxels not yet set take t where their squared distance to { d2 = t } is below t (``_cover``
    asks several levels at once).  NONE everywhere (no seed) gives NONE everywhere."""
    d2 = np.asarray(d2)
    if d2.ndim != 3 or 0 in d2.shape or d2.dtype.kind not in 'ui':
        raise ValueError('squared distances are a [depth][height][width] array of unsigned integers')
    d = d2.astype(np.int64)
    none = d == NONE
    if none.all():
        return np.full(d2.shape, NONE, np.uint32)
    if none.any() or int(d.min()) < 0 or int(d.max()) > NONE:
        raise ValueError('squared distances are finite everywhere, or NONE everywhere')
    out = np.zeros(d.size, np.int64)
    voxels = np.flatnonzero(d.ravel() > 0)
    values = d.ravel()[voxels]
    order = np.argsort(-values, kind='stable')
    centres = np.stack(np.unravel_index(voxels[order], d.shape), axis=-1).astype(np.int64)
    _cover(d.shape, out, centres, values[order], voxels)
    return np.ascontiguousarray(out.reshape(d.shape), dtype=np.uint32)


def thickness_texels(array, lo, hi, steps=2, seeds='rest'):
    """[depth][height][width][2] in the array's dtype: (code, min(isqrt(steps^2 T2), M)), T2 the squared local thickness of the codes
    lo .. hi (seeds 'rest') or of their complement (seeds 'range'); steps 2: the diameter in voxels: what
    ``Volume.thickness(lo, hi, steps, seeds)`` holds"""
    return channel_texels(array, thickness_squared_texels(distance_squared_texels(array, lo, hi, seeds)), steps)


def open_ball_texels(array, lo, hi, radius, fill=0):
    """the codes lo .. hi opened by the Euclidean ball of ``radius`` voxels: the codes that an inscribed ball of a radius above
    ``radius`` covers, ``fill`` elsewhere: what ``Volume.open_ball(lo, hi, radius)`` holds"""
    return within_texels(array, thickness_squared_texels(distance_squared_texels(array, lo, hi, 'rest')), check_radius(radius) + 1, None, fill)


def margin_texels(array, lo, hi, radius, fill=0):
    """the codes within ``radius`` voxels of the codes lo .. hi, ``fill`` elsewhere: what ``Volume.margin(lo, hi, radius)`` holds"""
    return within_texels(array, distance_squared_texels(array, lo, hi, 'range'), 0, check_radius(radius), fill)


def core_texels(array, lo, hi, radius, fill=0):
    """the codes lo .. hi eroded by the Euclidean ball of ``radius`` voxels: the codes deeper than ``radius`` inside the structure,
    ``fill`` elsewhere: what ``Volume.core(lo, hi, radius)`` holds"""
    return within_texels(array, distance_squared_texels(array, lo, hi, 'rest'), check_radius(radius) + 1, None, fill)
