"""The watershed of a relief by steepest descent on its lower completion, on the host: the numpy statement of the contract the device
kernels (vpt_volume_watershed; include/vpt.h) are held to, for callers without a device and as the contract's documentation.

``array`` is a [depth][height][width] uint8 or uint16 array, or [depth][height][width][2] with a channel argument naming the channel that is
read.  All compares are unsigned on whole codes, M = 255 / 65535.  Connectivity c is 6, 18 or 26; a neighbour outside the volume does not
exist.  Every step is a pure function of the input, so no result depends on an order of flooding.

  domain:    D = { v : lo <= relief(v) <= hi }.  Only voxels of D are flooded and only voxels of D count as neighbours; the rest has rank 0.
  polarity:  'minima' floods from the minima, k(v) = relief(v); 'maxima' from the maxima, k(v) = M - relief(v) (a depth channel).
  lower completion:  d(v) = 0 if v has a c-neighbour u in D with k(u) < k(v); otherwise d(v) = 1 + min of d(u) over the c-neighbours u in
             D with k(u) = k(v); d(v) = infinity when no such chain reaches a voxel with d = 0.  d is the geodesic step count, inside the
             level set, to the plateau's lower border; the voxels with d = infinity are exactly the regional minima of k within D.
  descent:   a voxel that is no minimum has one pointer p(v).  d(v) = 0: among the c-neighbours u in D with k(u) < k(v) the one of smallest
             k(u), then of smallest linear index (z ny + y) nx + x.  0 < d(v) < infinity: among the c-neighbours u in D with k(u) = k(v) and
             d(u) = d(v) - 1 the one of smallest linear index.  (k, d) falls lexicographically along p: every walk ends on a minimum voxel.
  basins:    the connected components of the graph on D with the edges {v, p(v)} and {u, v} for c-adjacent minimum voxels: a regional
             minimum together with every voxel whose walk ends in it.  There are no watershed-line voxels.
  order:     the components' (vpt_amd.components): root = the basin's smallest linear index; basins of fewer than min_voxels voxels are
             dropped (rank 0), the others ranked by voxel count descending, then by root ascending.
The functions iterate the definition to its fixed point: plain, and as slow as the longest plateau path is long."""
import numpy as np

from .components import _roots, check_connectivity, check_min_voxels, check_range, neighbour_offsets
from .reconstruct import _channel

POLARITIES = {'minima': 0, 'maxima': 1}                                      # VPT_WATERSHED_*
SPLIT_DEFAULTS = {'h': 2, 'steps': 4, 'connectivity': 26, 'minVoxels': 1}


def check_polarity(polarity):
    """the code of 'minima' | 'maxima' (VPT_WATERSHED_*); raises ValueError otherwise"""
    if not isinstance(polarity, str) or polarity not in POLARITIES:
        raise ValueError("watershed polarity is 'minima' or 'maxima', not %r" % (polarity,))
    return POLARITIES[polarity]


def check_split(split, largest=65535):
    """the ``split`` option of a rendering context as a dict with every key, or None: None | {'lo', 'hi', 'h': 2, 'steps': 4,
    'connectivity': 26, 'minVoxels': 1}; raises ValueError otherwise"""
    from .distance import check_steps
    from .reconstruct import check_h
    if split is None:
        return None
    if not isinstance(split, dict) or 'lo' not in split or 'hi' not in split or set(split) - {'lo', 'hi'} - set(SPLIT_DEFAULTS):
        raise ValueError("split is None or {'lo', 'hi', 'h': 2, 'steps': 4, 'connectivity': 26, 'minVoxels': 1}, not %r" % (split,))
    out = dict(SPLIT_DEFAULTS, **split)
    out['lo'], out['hi'] = check_range(out['lo'], out['hi'], largest)
    out['h'] = check_h('hmax', out['h'], largest)
    out['steps'] = check_steps(out['steps'])
    out['connectivity'] = check_connectivity(out['connectivity'])
    out['minVoxels'] = check_min_voxels(out['minVoxels'])
    return out


def _shifted(padded, offset, shape):
    (dz, dy, dx), (d, h, w) = offset, shape
    return padded[1 + dz:1 + dz + d, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]


def descent_texels(array, lo, hi, polarity='minima', connectivity=6, channel=0):
    """(inside, d, p) of the contract, [depth][height][width] each: ``inside`` the domain D (bool); ``d`` the lower completion (int64; -1
    for infinity and outside D); ``p`` the linear index a voxel points to (int64; its own index on a minimum voxel, -1 outside D)"""
    relief = _channel(array, channel, 'the relief')
    if 0 in relief.shape:
        raise ValueError('the relief is empty')
    largest = int(np.iinfo(relief.dtype).max)
    lo, hi = check_range(lo, hi, largest)
    flip, offsets = check_polarity(polarity), neighbour_offsets(connectivity)
    if relief.size > 0xFFFFFFFE:
        raise ValueError('watershed: more than 2^32 - 2 voxels')
    shape, n = relief.shape, relief.size
    inside = (relief >= lo) & (relief <= hi)
    wide = relief.astype(np.int64)
    none = largest + 1                                           # the key of what is not in D: never lower than, never equal to, a voxel of D
    k = np.where(inside, largest - wide if flip else wide, none)
    kp = np.pad(k, 1, constant_values=none)
    far = n + 1                                                  # infinity: a chain has at most n - 1 steps
    lower = np.zeros(shape, dtype=bool)
    for o in offsets:
        lower |= _shifted(kp, o, shape) < k
    d = np.where(inside & lower, 0, far)
    while True:
        dp = np.pad(d, 1, constant_values=far)
        best = np.full(shape, far, dtype=np.int64)
        for o in offsets:
            best = np.minimum(best, np.where(_shifted(kp, o, shape) == k, _shifted(dp, o, shape), far))
        new = np.where(inside, np.minimum(d, np.minimum(best + 1, far)), far)
        if np.array_equal(new, d):
            break
        d = new
    # the pointers: offsets come in the order of the linear index, so the first that qualifies is the one of smallest index
    index = np.arange(n, dtype=np.int64).reshape(shape)
    ip = np.pad(index, 1, constant_values=-1)
    dp = np.pad(d, 1, constant_values=far)
    p = np.where(inside, index, -1)
    best_key = np.where(d == 0, k, -1)                          # d = 0: a neighbour must beat the best key so far, strictly
    taken = ~(inside & (d > 0) & (d < far))                     # 0 < d < infinity: the first neighbour one step nearer
    for o in offsets:
        ku, du, iu = _shifted(kp, o, shape), _shifted(dp, o, shape), _shifted(ip, o, shape)
        steeper = ku < best_key
        p = np.where(steeper, iu, p)
        best_key = np.where(steeper, ku, best_key)
        nearer = ~taken & (ku == k) & (du == d - 1)
        p = np.where(nearer, iu, p)
        taken |= nearer
    return inside, np.where(inside & (d < far), d, -1), p


def watershed_texels(array, lo, hi, polarity='minima', connectivity=6, min_voxels=1, channel=0):
    """(ranks, basins) of the relief ``array`` over the domain [lo, hi] (module docstring): ranks uint32 [depth][height][width], basins the
    list of (root_x, root_y, root_z, voxels) in canonical order: what ``Volume.watershed(...)`` holds on the device."""
    min_voxels = check_min_voxels(min_voxels)
    inside, d, p = descent_texels(array, lo, hi, polarity, connectivity, channel)
    dpt, h, w = inside.shape
    n = inside.size
    # every voxel follows its pointers to the minimum voxel its walk ends on
    end = np.where(inside, p, np.arange(n, dtype=np.int64).reshape(inside.shape)).reshape(-1)
    while True:
        up = end[end]
        if np.array_equal(up, end):
            break
        end = up
    # adjacent minimum voxels have equal k, so the regional minima are the plain c-components of the minimum voxels
    minimum = _roots(inside & (d < 0), connectivity).reshape(-1)
    basin = minimum[end]                                         # names a basin by the smallest index of its minimum
    flat = inside.reshape(-1)
    where = np.flatnonzero(flat)
    first = np.full(n + 1, n, dtype=np.int64)                   # the basin's smallest linear index: its root
    np.minimum.at(first, basin[where], where)
    label = np.where(flat, first[np.where(flat, basin, n)], n)
    roots, voxels = np.unique(label[where], return_counts=True)
    stay = voxels >= min_voxels
    roots, voxels = roots[stay], voxels[stay]
    order = np.lexsort((roots, -voxels))                        # voxels descending, then root ascending
    roots, voxels = roots[order], voxels[order]
    table = np.zeros(n + 1, np.uint32)
    table[roots] = np.arange(1, len(roots) + 1, dtype=np.uint32)
    ranks = np.ascontiguousarray(table[label].reshape(inside.shape), dtype=np.uint32)
    basins = [(int(r % w), int(r // w % h), int(r // (w * h)), int(v)) for r, v in zip(roots, voxels)]
    return ranks, basins


def split_texels(array, lo, hi, h=2, steps=4, connectivity=26, min_voxels=1):
    """(ranks, basins) of ``Volume.split``: the watershed, from the maxima, of the h-maxima-flattened depth channel of the codes lo .. hi
    of a one-channel array: distance to the rest -> channel(steps) -> hmax(h) -> watershed(1, M, 'maxima')"""
    from .distance import channel_texels, distance_squared_texels
    from .reconstruct import geodesic_texels
    array = np.asarray(array)
    depth = channel_texels(array, distance_squared_texels(array, lo, hi, 'rest'), steps)
    flattened = geodesic_texels(depth, 'hmax', h, connectivity, 1)
    return watershed_texels(flattened, 1, int(np.iinfo(array.dtype).max), 'maxima', connectivity, min_voxels)
