"""The connected components of a value range of a volume, on the host: the numpy statement of the contract the device kernels
(vpt_volume_components and the vpt_components_* family; include/vpt.h) are held to, for callers without a device and as the contract's
documentation.

uint8 and uint16 [depth][height][width] arrays, c = the texel code.

  foreground:    lo <= c <= hi, compared as whole unsigned codes
  connectivity:  6 (voxels that share a face), 18 (a face or an edge), 26 (a face, an edge or a corner); nothing wraps, nothing is clamped:
                 voxels outside the array are background
  root:          the voxel of a component with the smallest linear index (z ny + y) nx + x
  listed:        the components of at least min_voxels voxels, by voxel count descending, then by root index ascending
  rank:          of a voxel: the 1-based position of its component in that list; 0 for background and for the voxels of dropped components

keep:   the code where first <= rank <= last, `fill` elsewhere.      label:   (code, min(rank, M)), M = 255 / 65535."""
import numpy as np

CONNECTIVITIES = (6, 18, 26)


def check_connectivity(connectivity):
    """6, 18 or 26; raises ValueError otherwise"""
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or connectivity not in CONNECTIVITIES:
        raise ValueError('connectivity is 6, 18 or 26, not %r' % (connectivity,))
    return int(connectivity)


def _whole(value, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s is an integer, not %r' % (what, value))
    return int(value)


def check_range(lo, hi, largest):
    """(lo, hi) of a component range in code units: integers with 0 <= lo <= hi <= largest; raises ValueError otherwise"""
    lo, hi = _whole(lo, 'the lower end of a component range'), _whole(hi, 'the upper end of a component range')
    if not 0 <= lo <= hi <= largest:
        raise ValueError('component range [%d, %d]: 0 <= lo <= hi <= %d' % (lo, hi, largest))
    return lo, hi


def check_min_voxels(min_voxels):
    """the smallest listed component, an integer in 1 .. 2^32 - 1; raises ValueError otherwise"""
    min_voxels = _whole(min_voxels, 'min_voxels')
    if not 1 <= min_voxels <= 0xFFFFFFFF:
        raise ValueError('min_voxels is in 1 .. 2^32 - 1, not %d' % min_voxels)
    return min_voxels


def check_keep(first, last, fill, largest):
    """(first, last, fill) of a selection: 1 <= first <= last < 2^64 (last None: every rank), 0 <= fill <= largest; raises ValueError otherwise"""
    first = _whole(first, 'the first rank kept')
    last = 0xFFFFFFFFFFFFFFFF if last is None else _whole(last, 'the last rank kept')
    fill = _whole(fill, 'fill')
    if not 1 <= first <= last <= 0xFFFFFFFFFFFFFFFF:
        raise ValueError('ranks %d .. %d: 1 <= first <= last is required' % (first, last))
    if not 0 <= fill <= largest:
        raise ValueError('fill %d: the largest code is %d' % (fill, largest))
    return first, last, fill


def neighbour_offsets(connectivity):
    """the (dz, dy, dx) of a voxel's neighbours"""
    most = {6: 1, 18: 2, 26: 3}[check_connectivity(connectivity)]
    return [(c, b, a) for c in (-1, 0, 1) for b in (-1, 0, 1) for a in (-1, 0, 1) if 1 <= (a != 0) + (b != 0) + (c != 0) <= most]


def _texels(array):
    array = np.asarray(array)
    if array.dtype not in (np.uint8, np.uint16) or array.ndim != 3 or 0 in array.shape:
        raise ValueError('connected components take a [depth][height][width] uint8 or uint16 array')
    return array


def _roots(foreground, connectivity):
    """[depth][height][width] int64: the linear index of the root of every foreground voxel's component; the voxel count elsewhere"""
    d, h, w = foreground.shape
    n = foreground.size
    label = np.where(foreground, np.arange(n, dtype=np.int64).reshape(d, h, w), n)
    offsets = neighbour_offsets(connectivity)
    inside = np.flatnonzero(foreground)
    while True:
        # the smallest label around every voxel ...
        p = np.pad(label, 1, constant_values=n)
        m = label
        for c, b, a in offsets:
            m = np.minimum(m, p[1 + c:1 + c + d, 1 + b:1 + b + h, 1 + a:1 + a + w])
        # ... goes to the voxel its label names (labels name voxels of the same component), and every voxel follows the names to their end
        parent = np.arange(n + 1, dtype=np.int64)
        np.minimum.at(parent, label.reshape(-1)[inside], m.reshape(-1)[inside])
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        new = np.where(foreground, parent[label], n)
        if np.array_equal(new, label):
            return label
        label = new


def components_texels(array, lo, hi, connectivity=6, min_voxels=1):
    """(ranks, components) of the value range [lo, hi] of a [depth][height][width] uint8 or uint16 array: ranks uint32 [depth][height][width],
    components the list of (root_x, root_y, root_z, voxels) in canonical order: what ``Volume.components(...)`` holds on the device."""
    array = _texels(array)
    lo, hi = check_range(lo, hi, int(np.iinfo(array.dtype).max))
    connectivity, min_voxels = check_connectivity(connectivity), check_min_voxels(min_voxels)
    d, h, w = array.shape
    if array.size > 0xFFFFFFFE:
        raise ValueError('connected components: more than 2^32 - 2 voxels')
    foreground = (array >= lo) & (array <= hi)
    label = _roots(foreground, connectivity)
    roots, voxels = np.unique(label[foreground], return_counts=True)
    stay = voxels >= min_voxels
    roots, voxels = roots[stay], voxels[stay]
    order = np.lexsort((roots, -voxels))                      # voxels descending, then root ascending
    roots, voxels = roots[order], voxels[order]
    table = np.zeros(array.size + 1, np.uint32)
    table[roots] = np.arange(1, len(roots) + 1, dtype=np.uint32)
    ranks = np.ascontiguousarray(table[label], dtype=np.uint32)
    components = [(int(r % w), int(r // w % h), int(r // (w * h)), int(v)) for r, v in zip(roots, voxels)]
    return ranks, components


def _ranks(array, ranks):
    ranks = np.asarray(ranks)
    if ranks.shape != array.shape or ranks.dtype.kind not in 'ui':
        raise ValueError('ranks are one unsigned integer per voxel of the array')
    return ranks.astype(np.uint64)


def keep_texels(array, ranks, first=1, last=None, fill=0):
    """the array's codes where first <= rank <= last (last None: every rank), ``fill`` elsewhere, in the array's dtype: what
    ``Components.keep(first, last, fill)`` holds on the device."""
    array = _texels(array)
    first, last, fill = check_keep(first, last, fill, int(np.iinfo(array.dtype).max))
    ranks = _ranks(array, ranks)
    kept = (ranks >= np.uint64(first)) & (ranks <= np.uint64(last))
    return np.ascontiguousarray(np.where(kept, array, array.dtype.type(fill)), dtype=array.dtype)


def label_texels(array, ranks):
    """[depth][height][width][2] in the array's dtype: (code, min(rank, M)), M the dtype's largest code: what ``Components.label()`` holds on
    the device.  Ranks beyond M share the last row of the 2-D transfer function."""
    array = _texels(array)
    ranks = _ranks(array, ranks)
    g = np.minimum(ranks, np.uint64(np.iinfo(array.dtype).max)).astype(array.dtype)
    return np.ascontiguousarray(np.stack([array, g], axis=-1))
