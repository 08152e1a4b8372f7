"""Per-component measurements of a labelling and the selection by a set of ranks, on the host: the numpy statement of the contract the
device kernels (vpt_components_measure, vpt_components_keep_set; include/vpt.h) are held to, for callers without a device and as the
contract's documentation.

ranks: uint32 [depth][height][width], the 1-based rank of every voxel's component (0: background and dropped components), as
``components_texels`` gives them; values: an unsigned integer array of the same shape (its width is independent of the labelled array's).

  record k:      the component of rank first + 1 + k, k = 0 .. n - 1; voxels of other ranks contribute nothing
  box:           min / max of the voxel indices, inclusive;   sum_x, sum_y, sum_z: their sums (centroid = sum / voxels)
  values:        min, max, sum and sum of squares of the whole unsigned codes under the component
  faces:         a voxel's face counts when the neighbour across it lies outside the array or has a different rank

Every field is an exact integer.  The sum of squares of 16-bit codes can pass 2^63 (a component of 2^31 voxels and more) but not 2^64, so it
is summed in unsigned 64-bit words; ``derive`` multiplies such sums, which passes 2^64, and works in Python integers."""
import numpy as np

MEASURE_DTYPE = np.dtype([
    ('voxels', '<u8'),
    ('min_x', '<u4'), ('min_y', '<u4'), ('min_z', '<u4'), ('max_x', '<u4'), ('max_y', '<u4'), ('max_z', '<u4'),
    ('value_min', '<u4'), ('value_max', '<u4'),
    ('sum_x', '<u8'), ('sum_y', '<u8'), ('sum_z', '<u8'),
    ('value_sum', '<u8'), ('value_sum_sq', '<u8'),
    ('faces', '<u8'),
])
assert MEASURE_DTYPE.itemsize == 88            # struct vpt_component_measure (include/vpt.h): no padding


def _whole(value, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s is an integer, not %r' % (what, value))
    return int(value)


def check_window(first, n, listed):
    """(first, n) of a window of the component list: integers with 0 <= first <= listed and 0 <= n <= listed - first (n None: to the end);
    raises ValueError otherwise"""
    first = _whole(first, 'the first component measured')
    if not 0 <= first <= listed:
        raise ValueError('components %d .. are not within the %d listed' % (first, listed))
    n = listed - first if n is None else _whole(n, 'the number of components measured')
    if not 0 <= n <= listed - first:
        raise ValueError('components %d .. +%d are not within the %d listed' % (first, n, listed))
    return first, n


def check_rank_set(selected, listed=None):
    """the ranks of a selection as a list of Python integers: an iterable of 1-based ranks (duplicates and ranks beyond the list are
    allowed), or a boolean array over the list (entry k selects rank k + 1; its length is ``listed`` where that is given); raises
    ValueError for a rank below 1"""
    a = np.asarray(selected if isinstance(selected, np.ndarray) else list(selected))
    if a.dtype == np.bool_:
        if a.ndim != 1 or (listed is not None and len(a) != listed):
            raise ValueError('a boolean selection has one entry per listed component')
        return [int(k) + 1 for k in np.flatnonzero(a)]
    if a.size and a.dtype.kind not in 'ui' and not all(isinstance(r, (int, np.integer)) and not isinstance(r, bool) for r in a.reshape(-1).tolist()):
        raise ValueError('the selected ranks are integers')
    out = [int(r) for r in a.reshape(-1).tolist()]
    for r in out:
        if not 1 <= r <= 0xFFFFFFFFFFFFFFFF:
            raise ValueError('rank %d: ranks are 1-based' % r)
    return out


def _fields(ranks, values):
    ranks = np.asarray(ranks)
    if ranks.ndim != 3 or 0 in ranks.shape or ranks.dtype.kind not in 'ui':
        raise ValueError('ranks are one unsigned integer per voxel of a [depth][height][width] array')
    values = np.asarray(values)
    if values.shape != ranks.shape or values.dtype not in (np.uint8, np.uint16):
        raise ValueError('values are a uint8 or uint16 array of the ranks\' shape')
    return ranks.astype(np.int64), values


def measure_texels(ranks, values, first=0, n=None):
    """the records (MEASURE_DTYPE) of the components of rank first + 1 .. first + n of ``ranks`` (n None: to the largest rank present),
    ``values`` measured under them: what ``Components.measure(first, n, values)`` returns."""
    ranks, values = _fields(ranks, values)
    listed = int(ranks.max())
    first, n = check_window(first, n, listed)
    out = np.zeros(n, MEASURE_DTYPE)
    if n == 0:
        return out
    d, h, w = ranks.shape
    inside = (ranks > first) & (ranks <= first + n)
    key = (ranks[inside] - (first + 1)).astype(np.int64)
    z, y, x = (a.astype(np.int64) for a in np.nonzero(inside))
    v = values[inside].astype(np.int64)
    # faces: 6 per voxel less one for every neighbour of the same rank (outside the array: a rank no voxel has)
    p = np.pad(ranks, 1, constant_values=-1)
    same = np.zeros(ranks.shape, np.int64)
    for c, b, a in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
        same += p[1 + c:1 + c + d, 1 + b:1 + b + h, 1 + a:1 + a + w] == ranks
    faces = 6 - same[inside]

    out['voxels'] = np.bincount(key, minlength=n)
    # np.bincount sums weights in float64: exact only below 2^53, so the integer sums go through np.add.at on int64 / Python integers
    for name, q in (('sum_x', x), ('sum_y', y), ('sum_z', z), ('value_sum', v), ('faces', faces)):
        acc = np.zeros(n, np.int64)               # each is below 2^45 x 2^16: inside int64
        np.add.at(acc, key, q)
        out[name] = acc.astype(np.uint64)
    sq = np.zeros(n, np.uint64)                    # can pass 2^63 but not 2^64 (include/vpt.h): unsigned 64-bit words hold it exactly
    np.add.at(sq, key, (v * v).astype(np.uint64))
    out['value_sum_sq'] = sq
    for name, q in (('min_x', x), ('min_y', y), ('min_z', z), ('value_min', v)):
        acc = np.full(n, 0xFFFFFFFF, np.int64)
        np.minimum.at(acc, key, q)
        out[name] = acc.astype(np.uint32)
    for name, q in (('max_x', x), ('max_y', y), ('max_z', z), ('value_max', v)):
        acc = np.zeros(n, np.int64)
        np.maximum.at(acc, key, q)
        out[name] = acc.astype(np.uint32)
    return out


def keep_set_texels(array, ranks, selected, fill=0):
    """the array's codes where the voxel's rank is in ``selected`` (an iterable of 1-based ranks, or a boolean array over the list),
    ``fill`` elsewhere, in the array's dtype: what ``Components.keep_set(selected, fill)`` holds on the device."""
    from .components import _texels, _ranks, _whole as whole
    array = _texels(array)
    ranks = _ranks(array, ranks)
    listed = int(ranks.max())
    fill = whole(fill, 'fill')
    if not 0 <= fill <= int(np.iinfo(array.dtype).max):
        raise ValueError('fill %d: the largest code is %d' % (fill, int(np.iinfo(array.dtype).max)))
    table = np.zeros(listed + 1, bool)
    for r in check_rank_set(selected):
        if r <= listed:
            table[r] = True
    return np.ascontiguousarray(np.where(table[ranks.astype(np.int64)], array, array.dtype.type(fill)), dtype=array.dtype)


def derive(records):
    """per record of ``measure``: a structured float64 array of 'centroid_x', 'centroid_y', 'centroid_z' (sum / voxels), 'mean'
    (value_sum / voxels), 'variance' (the population variance (n sum_sq - sum^2) / n^2, the numerator taken in integers before the one
    division), the integer box extents 'extent_x', 'extent_y', 'extent_z' (max - min + 1) and 'fill' (voxels / box volume)."""
    records = np.asarray(records, MEASURE_DTYPE).reshape(-1)
    out = np.zeros(len(records), np.dtype([('centroid_x', 'f8'), ('centroid_y', 'f8'), ('centroid_z', 'f8'), ('mean', 'f8'), ('variance', 'f8'),
                                           ('extent_x', 'u4'), ('extent_y', 'u4'), ('extent_z', 'u4'), ('fill', 'f8')]))
    for k, r in enumerate(records):
        n = int(r['voxels'])
        if n == 0:
            raise ValueError('record %d has no voxels' % k)
        s, s2 = int(r['value_sum']), int(r['value_sum_sq'])
        ex, ey, ez = (int(r['max_' + a]) - int(r['min_' + a]) + 1 for a in 'xyz')
        out[k] = (int(r['sum_x']) / n, int(r['sum_y']) / n, int(r['sum_z']) / n, s / n, (n * s2 - s * s) / (n * n), ex, ey, ez, n / (ex * ey * ez))
    return out
