"""The curve skeleton and the topological kernel of a value range of a volume by subfield thinning, on the host: the numpy statement of the
contract the device kernels (vpt_volume_skeleton and the vpt_skeleton_* family; include/vpt.h) are held to, for callers without a device
and as the contract's documentation.

uint8 and uint16 [depth][height][width] arrays, c = the texel code.

  object X:   lo <= c <= hi, compared as whole unsigned codes; everything else, and everything outside the array, is background
  topology:   (26, 6): the object is 26-connected, the background 6-connected
  obj(p):     the neighbours of p among its 26 that are in X
  C(p):       the number of 26-connected components of obj(p), adjacency inside N26(p), p excluded
  B(p):       the number of 6-connected components of N18(p) \\ X that hold a face neighbour of p, adjacency inside N18(p)
  simple:     C(p) == 1 and B(p) == 1
  subfield:   (x & 1) | (y & 1) << 1 | (z & 1) << 2

A pass k = 1, 2, ...: Border = the voxels of X with a background face neighbour, taken when the pass starts; then for s = 0 .. 7 every
voxel of Border still in X with subfield s is visited: 'kernel' deletes it if it is simple; 'ends' skips it if |obj| == 1 and otherwise
deletes it if it is simple; 'isthmus' skips a marked voxel, marks (for good) and skips one with C >= 2, and otherwise deletes it if it is
simple.  The voxels visited in a sub-step are never 26-adjacent, so the order of the visits changes nothing (``order`` lets a test say
so).  The run ends after the first pass that deletes and marks nothing, or after pass ``passes`` when that is positive.

burn:  uint32 per voxel: 0 outside the range, k for a voxel deleted in pass k, KEPT = 0xFFFFFFFF for a voxel that survived."""
import numpy as np

KEPT = 0xFFFFFFFF
MODES = {'kernel': 0, 'ends': 1, 'isthmus': 2}
INFO_FIELDS = ('object_voxels', 'kept_voxels', 'passes', 'converged', 'isolated', 'ends', 'regular', 'junctions')

# the 3 x 3 x 3 neighbourhood as 27 bits: bit 9 (dz + 1) + 3 (dy + 1) + (dx + 1); the centre is bit 13
_OFFSETS = [(i % 3 - 1, i // 3 % 3 - 1, i // 9 - 1) for i in range(27)]
_CENTRE = 1 << 13
_WEIGHTS = (1 << np.arange(27, dtype=np.int64))
_N18 = sum(1 << i for i, o in enumerate(_OFFSETS) if 1 <= sum(c != 0 for c in o) <= 2)
_N6 = sum(1 << i for i, o in enumerate(_OFFSETS) if sum(c != 0 for c in o) == 1)


def _adjacency(reach):
    """per bit, the bits of the cube (the centre left out) at most ``reach`` axis steps away with every offset difference within 1"""
    out = []
    for a in _OFFSETS:
        m = 0
        for j, b in enumerate(_OFFSETS):
            d = [abs(p - q) for p, q in zip(a, b)]
            if j != 13 and a != b and max(d) <= 1 and sum(d) <= reach:
                m |= 1 << j
        out.append(m)
    return out


_ADJ26, _ADJ6 = _adjacency(3), _adjacency(1)
_TOPOLOGY = {}


def _parts(bits, adjacency):
    """the connected components of a set of cube voxels, as a list of bit sets: the voxels are added one by one, each joining the parts
    it touches"""
    parts = []
    while bits:
        low = bits & -bits
        bits ^= low
        joined, near = low, adjacency[low.bit_length() - 1]
        rest = []
        for part in parts:
            if part & near:
                joined |= part
            else:
                rest.append(part)
        rest.append(joined)
        parts = rest
    return parts


def topology(obj):
    """(C, B) of a voxel whose object neighbours are the bit set ``obj`` (27 bits, the centre bit clear)"""
    found = _TOPOLOGY.get(obj)
    if found is None:
        c = len(_parts(obj, _ADJ26))
        b = sum(1 for part in _parts(_N18 & ~obj, _ADJ6) if part & _N6)
        found = (c, b)
        if len(_TOPOLOGY) < (1 << 20):
            _TOPOLOGY[obj] = found
    return found


def _whole(value, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s is an integer, not %r' % (what, value))
    return int(value)


def check_mode(mode):
    """the code of 'kernel' (0: VPT_THIN_KERNEL), 'ends' (1: VPT_THIN_ENDS) or 'isthmus' (2: VPT_THIN_ISTHMUS); raises ValueError otherwise"""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError("mode is 'kernel', 'ends' or 'isthmus', not %r" % (mode,))
    return MODES[mode]


def check_range(lo, hi, largest):
    """(lo, hi) of a skeleton range in code units: integers with 0 <= lo <= hi <= largest; raises ValueError otherwise"""
    lo, hi = _whole(lo, 'the lower end of a skeleton range'), _whole(hi, 'the upper end of a skeleton range')
    if not 0 <= lo <= hi <= largest:
        raise ValueError('skeleton range [%d, %d]: 0 <= lo <= hi <= %d' % (lo, hi, largest))
    return lo, hi


def check_passes(passes):
    """the pass cap: 0 (to the fixed point) or a positive integer below 2^31; raises ValueError otherwise"""
    passes = _whole(passes, 'passes')
    if not 0 <= passes < (1 << 31):
        raise ValueError('passes is 0 (to the fixed point) or a positive cap, not %d' % passes)
    return passes


def check_within(k_lo, k_hi, fill, largest):
    """(k_lo, k_hi, fill) of a selection of burn passes: 0 <= k_lo <= k_hi < 2^32 (k_hi None: 0xFFFFFFFF, the kept voxels included),
    0 <= fill <= largest; raises ValueError otherwise"""
    k_lo = _whole(k_lo, 'the first burn pass kept')
    k_hi = KEPT if k_hi is None else _whole(k_hi, 'the last burn pass kept')
    fill = _whole(fill, 'fill')
    if not 0 <= k_lo <= k_hi <= KEPT:
        raise ValueError('burn passes %d .. %d: 0 <= from <= to < 2^32 is required' % (k_lo, k_hi))
    if not 0 <= fill <= largest:
        raise ValueError('fill %d: the largest code is %d' % (fill, largest))
    return k_lo, k_hi, fill


def _texels(array):
    array = np.asarray(array)
    if array.dtype not in (np.uint8, np.uint16) or array.ndim != 3 or 0 in array.shape:
        raise ValueError('the skeleton takes a [depth][height][width] uint8 or uint16 array')
    if max(array.shape) > 4096:
        raise ValueError('the skeleton takes at most 4096 voxels an axis')
    return array


def _census(kept):
    """(isolated, ends, regular, junctions): the kept voxels with 0, 1, 2 and >= 3 kept 26-neighbours"""
    padded = np.pad(kept, 1).astype(np.int32)
    d, h, w = kept.shape
    near = -padded[1:-1, 1:-1, 1:-1]
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                near = near + padded[dz:dz + d, dy:dy + h, dx:dx + w]
    near = np.minimum(near[kept], 3)
    return tuple(int((near == k).sum()) for k in range(4))


def skeleton_burn_texels(array, lo, hi, mode, passes=0, order='raster', marks=None):
    """(uint32 [depth][height][width] burn passes, the info dict with INFO_FIELDS) of thinning the codes lo .. hi of a uint8 or uint16
    array in ``mode`` for at most ``passes`` passes (0: to the fixed point): what ``Volume.skeleton(...)`` holds on the device.
    ``order`` (for tests): 'raster' or 'reversed', the order in which the voxels of a sub-step are visited; each visit sees what the
    visits before it have deleted; ``marks``: a bool array of the array's shape that receives the isthmus marks."""
    array = _texels(array)
    lo, hi = check_range(lo, hi, int(np.iinfo(array.dtype).max))
    mode = check_mode(mode)
    passes = check_passes(passes)
    if order not in ('raster', 'reversed'):
        raise ValueError("order is 'raster' or 'reversed', not %r" % (order,))
    d, h, w = array.shape
    inside = (array >= lo) & (array <= hi)
    burn = np.where(inside, np.uint32(KEPT), np.uint32(0))
    info = dict.fromkeys(INFO_FIELDS, 0)
    info['object_voxels'] = int(inside.sum())
    info['converged'] = 1
    if info['object_voxels'] == 0:
        return burn, info
    X = np.pad(inside, 1)                                        # [z + 1][y + 1][x + 1]
    marked = np.zeros_like(inside) if marks is None else marks
    marked[...] = False
    k = 0
    while True:
        k += 1
        core = X[1:-1, 1:-1, 1:-1]
        border = core & ~(X[:-2, 1:-1, 1:-1] & X[2:, 1:-1, 1:-1] & X[1:-1, :-2, 1:-1] & X[1:-1, 2:, 1:-1] & X[1:-1, 1:-1, :-2] & X[1:-1, 1:-1, 2:])
        zs, ys, xs = np.nonzero(border)                          # raster order: x fastest
        subfield = (xs & 1) | ((ys & 1) << 1) | ((zs & 1) << 2)
        changed = 0
        for s in range(8):
            visits = np.flatnonzero(subfield == s)
            if order == 'reversed':
                visits = visits[::-1]
            for i in visits:
                z, y, x = int(zs[i]), int(ys[i]), int(xs[i])
                obj = int(X[z:z + 3, y:y + 3, x:x + 3].ravel().dot(_WEIGHTS)) & ~_CENTRE
                if mode == 1 and obj and obj & (obj - 1) == 0:
                    continue                                     # a curve end
                if mode == 2 and marked[z, y, x]:
                    continue
                c, b = topology(obj)
                if mode == 2 and c >= 2:
                    marked[z, y, x] = True
                    changed += 1
                elif c == 1 and b == 1:
                    X[z + 1, y + 1, x + 1] = False
                    burn[z, y, x] = k
                    changed += 1
        info['passes'] = k
        info['converged'] = 1 if changed == 0 else 0
        if changed == 0 or k == passes:
            break
    kept = np.ascontiguousarray(X[1:-1, 1:-1, 1:-1])
    info['isolated'], info['ends'], info['regular'], info['junctions'] = _census(kept)
    info['kept_voxels'] = int(kept.sum())
    return burn, info


def burn_within_texels(array, burn, k_lo=KEPT, k_hi=None, fill=0):
    """the array's codes where k_lo <= burn <= k_hi (k_hi None: 0xFFFFFFFF), ``fill`` elsewhere, in the array's dtype: what
    ``Skeleton.within(k_lo, k_hi, fill)`` holds on the device"""
    array = _texels(array)
    k_lo, k_hi, fill = check_within(k_lo, k_hi, fill, int(np.iinfo(array.dtype).max))
    burn = np.asarray(burn)
    if burn.shape != array.shape or burn.dtype.kind not in 'ui':
        raise ValueError('burn passes are one unsigned integer per voxel of the array')
    burn = burn.astype(np.uint64)
    chosen = (burn >= np.uint64(k_lo)) & (burn <= np.uint64(k_hi))
    return np.ascontiguousarray(np.where(chosen, array, array.dtype.type(fill)), dtype=array.dtype)


def skeleton_texels(array, lo, hi, mode='ends', passes=0, fill=0):
    """the codes of the voxels of lo .. hi that survive the thinning, ``fill`` elsewhere: what ``Volume.centreline(lo, hi, mode)`` and
    ``Skeleton.volume()`` hold"""
    burn, _ = skeleton_burn_texels(array, lo, hi, mode, passes)
    return burn_within_texels(array, burn, KEPT, KEPT, fill)


def check_skeleton(spec):
    """the `skeleton` option of a RenderingContext with its defaults filled in: None, or {'lo', 'hi', 'mode': 'ends', 'passes': 0,
    'fill': 0}; raises ValueError otherwise.  The range is open above (hi may exceed an R8 volume's codes: it is cut to the volume's
    largest code when the option is applied)."""
    if spec is None:
        return None
    if not isinstance(spec, dict):
        raise ValueError("skeleton is None or {'lo', 'hi', 'mode', 'passes', 'fill'}, not %r" % (spec,))
    unknown = sorted(set(spec) - {'lo', 'hi', 'mode', 'passes', 'fill'})
    if unknown:
        raise ValueError('skeleton: unknown keys %s' % ', '.join(unknown))
    if spec.get('lo') is None or spec.get('hi') is None:
        raise ValueError("skeleton needs 'lo' and 'hi'")
    lo, hi = check_range(spec['lo'], spec['hi'], 65535)
    mode = spec['mode'] if spec.get('mode') is not None else 'ends'
    check_mode(mode)
    passes = check_passes(spec['passes'] if spec.get('passes') is not None else 0)
    fill = _whole(spec['fill'] if spec.get('fill') is not None else 0, 'fill')
    if not 0 <= fill <= 65535:
        raise ValueError('fill %d: the largest code is 65535' % fill)
    return {'lo': lo, 'hi': hi, 'mode': mode, 'passes': passes, 'fill': fill}
