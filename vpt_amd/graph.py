"""The graph of a set of voxels (a thinned skeleton, or any set): its branches, its nodes, their lengths, and the pruning of spurs, on the
host: the numpy statement of the contract the device kernels (vpt_volume_graph, vpt_skeleton_graph and the vpt_graph_* family;
include/vpt.h) are held to, byte for byte, for callers without a device and as the contract's documentation.  Every field is an integer.

  K:         the voxels of a uint8 / uint16 [depth][height][width] array whose code lies in lo .. hi (whole unsigned codes), or the kept
             voxels (burn == KEPT) of a skeleton; everything else, and everything outside the array, is absent
  deg(p):    |N26(p) & K|
  class(p):  0 outside K, otherwise 1 + min(deg, 3): 1 isolated, 2 end, 3 regular, 4 junction
  branch:    a 26-connected component of the voxels of class 1 .. 3; node: a 26-connected component of the voxels of class 4; both in the
             components' canonical order (voxels descending, then root index ascending; ranks from 1)

A branch voxel has at most two neighbours in K, so a branch is one voxel, a simple path or a simple cycle.  Its record (BRANCH_DTYPE):

  voxels, free_ends (its voxels of class 2), attachments (the pairs (branch voxel, 26-adjacent node voxel)), node_lo / node_hi (the
  smallest and largest node rank over those pairs, 0 / 0 without one), steps_face / steps_edge / steps_corner (the unordered 26-adjacent
  pairs inside the branch plus the attachment pairs, by the number of coordinates that differ), tip_lo / tip_hi (the smallest and largest
  linear index among its voxels with fewer than two neighbours in the branch; the root for a cycle), kind (``kind_of``).

A node's record (NODE_DTYPE): voxels, degree (the attachment pairs that name it).  Lengths are derived on the host (``lengths``) and assume
cubic voxels (``Volume.isotropic`` makes them).

Pruning (``prune_texels``) is one round: a branch is dropped when wf steps_face + we steps_edge + wc steps_corner <= length and it is a
SPUR, or (flag bit 0, debris) a SEGMENT or an ISOLATED voxel; node voxels always stay.  All spurs of a node go together: a Y whose three
arms are all within ``length`` is reduced to its node."""
import numpy as np

from .components import components_texels, neighbour_offsets

KEPT = 0xFFFFFFFF
ISOLATED, SEGMENT, SPUR, LINK, LOOP, CYCLE = range(6)
KINDS = ('isolated', 'segment', 'spur', 'link', 'loop', 'cycle')
PRUNE_DEBRIS = 1
DEFAULT_WEIGHTS = (10, 14, 17)
INFO_FIELDS = ('kept_voxels', 'node_voxels', 'branches', 'nodes', 'isolated', 'segments', 'spurs', 'links', 'loops', 'cycles',
               'steps_face', 'steps_edge', 'steps_corner', 'attachments')
BRANCH_DTYPE = np.dtype([('voxels', '<u4'), ('free_ends', '<u4'), ('attachments', '<u4'), ('kind', '<u4'), ('node_lo', '<u4'), ('node_hi', '<u4'),
                         ('steps_face', '<u8'), ('steps_edge', '<u8'), ('steps_corner', '<u8'), ('tip_lo', '<u8'), ('tip_hi', '<u8')])
NODE_DTYPE = np.dtype([('voxels', '<u8'), ('degree', '<u8')])
assert BRANCH_DTYPE.itemsize == 64 and NODE_DTYPE.itemsize == 16


def _whole(value, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s is an integer, not %r' % (what, value))
    return int(value)


def check_range(lo, hi, largest):
    """(lo, hi) of a graph's range in code units: integers with 0 <= lo <= hi <= largest; raises ValueError otherwise"""
    lo, hi = _whole(lo, 'the lower end of a graph range'), _whole(hi, 'the upper end of a graph range')
    if not 0 <= lo <= hi <= largest:
        raise ValueError('graph range [%d, %d]: 0 <= lo <= hi <= %d' % (lo, hi, largest))
    return lo, hi


def check_prune(length, weights, flags, fill, largest):
    """(length, (wf, we, wc), flags, fill) of a pruning: 0 <= length < 2^64, each weight 0 .. 65535, flags 0 or PRUNE_DEBRIS,
    0 <= fill <= largest; raises ValueError otherwise"""
    length = _whole(length, 'the prune length')
    if not 0 <= length < (1 << 64):
        raise ValueError('prune length %d: 0 <= length < 2^64 is required' % length)
    try:
        weights = tuple(weights)
    except TypeError:
        raise ValueError('weights are (face, edge, corner), not %r' % (weights,))
    if len(weights) != 3:
        raise ValueError('weights are (face, edge, corner), not %r' % (weights,))
    weights = tuple(_whole(w, 'a step weight') for w in weights)
    if not all(0 <= w <= 65535 for w in weights):
        raise ValueError('step weights %r: each is 0 .. 65535' % (weights,))
    flags = _whole(flags, 'the prune flags')
    if flags & ~PRUNE_DEBRIS or flags < 0:
        raise ValueError('prune flags %d: bit 0 (debris) is taken' % flags)
    fill = _whole(fill, 'fill')
    if not 0 <= fill <= largest:
        raise ValueError('fill %d: the largest code is %d' % (fill, largest))
    return length, weights, flags, fill


def check_centreline_prune(lo, hi, prune, prune_rounds, largest):
    """(prune length, rounds, fill) of ``Volume.centreline(lo, hi, prune=..., prune_rounds=...)``: the fill is a code outside lo .. hi, 0
    when lo > 0 and otherwise hi + 1, so a range that covers every code is refused"""
    prune = _whole(prune, 'prune')
    prune_rounds = _whole(prune_rounds, 'prune_rounds')
    if not 0 <= prune < (1 << 64):
        raise ValueError('prune %d: 0 <= prune < 2^64 is required' % prune)
    if not 1 <= prune_rounds <= 65535:
        raise ValueError('prune_rounds %d: 1 .. 65535 are taken' % prune_rounds)
    if lo == 0 and hi >= largest:
        raise ValueError('centreline with prune: the range [%d, %d] covers every code, none is left to fill with' % (lo, hi))
    return prune, prune_rounds, (0 if lo > 0 else hi + 1)


def _texels(array):
    array = np.asarray(array)
    if array.dtype not in (np.uint8, np.uint16) or array.ndim != 3 or 0 in array.shape:
        raise ValueError('the graph takes a [depth][height][width] uint8 or uint16 array')
    if max(array.shape) > 4096:
        raise ValueError('the graph takes at most 4096 voxels an axis')
    if array.size > 0xFFFFFFFE:
        raise ValueError('the graph takes at most 2^32 - 2 voxels')
    return array


def kind_of(voxels, free_ends, attachments, node_lo, node_hi):
    """the kind of a branch from its other fields"""
    if free_ends == 2:
        return SEGMENT
    if free_ends == 1 and attachments == 1:
        return SPUR
    if attachments == 2:
        return LINK if node_lo != node_hi else LOOP
    return ISOLATED if voxels == 1 else CYCLE


def classes_of(kept):
    """uint8 per voxel: 0 outside the bool set ``kept``, otherwise 1 + min(kept 26-neighbours, 3)"""
    padded = np.pad(kept, 1).astype(np.int32)
    d, h, w = kept.shape
    near = -padded[1:-1, 1:-1, 1:-1]
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                near = near + padded[dz:dz + d, dy:dy + h, dx:dx + w]
    return np.where(kept, 1 + np.minimum(near, 3), 0).astype(np.uint8)


def graph_of(kept, order='raster'):
    """the graph of a bool [depth][height][width] set: a dict with 'classes' (uint8 per voxel), 'branch_ranks' and 'node_ranks' (uint32 per
    voxel), 'branches' (BRANCH_DTYPE, one record a branch), 'nodes' (NODE_DTYPE) and 'info' (INFO_FIELDS).  ``order`` (for tests):
    'raster' or 'reversed', the order in which the branch voxels are visited; every sum, minimum and maximum is of integers."""
    kept = np.asarray(kept)
    if kept.dtype != bool or kept.ndim != 3 or 0 in kept.shape:
        raise ValueError('the graph takes a [depth][height][width] bool set')
    if order not in ('raster', 'reversed'):
        raise ValueError("order is 'raster' or 'reversed', not %r" % (order,))
    d, h, w = kept.shape
    classes = classes_of(kept)
    branch_ranks, branch_list = components_texels(classes, 1, 3, 26)
    node_ranks, node_list = components_texels(classes, 4, 4, 26)
    branches = np.zeros(len(branch_list), BRANCH_DTYPE)
    nodes = np.zeros(len(node_list), NODE_DTYPE)
    nodes['voxels'] = [v for _, _, _, v in node_list]
    none = (1 << 64) - 1
    node_lo = [0xFFFFFFFF] * len(branch_list)
    tip_lo, tip_hi = [none] * len(branch_list), [-1] * len(branch_list)
    offsets = neighbour_offsets(26)
    visits = np.flatnonzero((classes >= 1) & (classes <= 3))
    if order == 'reversed':
        visits = visits[::-1]
    flat_classes, flat_branch, flat_node = classes.reshape(-1), branch_ranks.reshape(-1), node_ranks.reshape(-1)
    steps = ('steps_face', 'steps_edge', 'steps_corner')
    for i in visits:
        i = int(i)
        x, y, z = i % w, i // w % h, i // (w * h)
        b = branches[int(flat_branch[i]) - 1]
        own = 0                                                   # neighbours in the voxel's own branch
        b['voxels'] += 1
        b['free_ends'] += int(flat_classes[i] == 2)
        for dz, dy, dx in offsets:
            xx, yy, zz = x + dx, y + dy, z + dz
            if not (0 <= xx < w and 0 <= yy < h and 0 <= zz < d):
                continue
            j = (zz * h + yy) * w + xx
            c = int(flat_classes[j])
            differ = (dx != 0) + (dy != 0) + (dz != 0)
            if 1 <= c <= 3:                                       # adjacent branch voxels are of one branch
                own += 1
                if j < i:                                         # every pair once, at its voxel of larger index
                    b[steps[differ - 1]] += 1
            elif c == 4:
                r = int(flat_node[j])
                b['attachments'] += 1
                b[steps[differ - 1]] += 1
                k = int(flat_branch[i]) - 1
                node_lo[k] = min(node_lo[k], r)
                b['node_hi'] = max(int(b['node_hi']), r)
                nodes[r - 1]['degree'] += 1
        if own < 2:
            k = int(flat_branch[i]) - 1
            tip_lo[k], tip_hi[k] = min(tip_lo[k], i), max(tip_hi[k], i)
    for k, (rx, ry, rz, _) in enumerate(branch_list):
        b = branches[k]
        root = (rz * h + ry) * w + rx
        b['node_lo'] = 0 if node_lo[k] == 0xFFFFFFFF else node_lo[k]
        b['tip_lo'], b['tip_hi'] = (root, root) if tip_hi[k] < 0 else (tip_lo[k], tip_hi[k])
        b['kind'] = kind_of(int(b['voxels']), int(b['free_ends']), int(b['attachments']), int(b['node_lo']), int(b['node_hi']))
    info = dict.fromkeys(INFO_FIELDS, 0)
    info['kept_voxels'] = int(kept.sum())
    info['node_voxels'] = int((classes == 4).sum())
    info['branches'], info['nodes'] = len(branch_list), len(node_list)
    for name, kind in zip(('isolated', 'segments', 'spurs', 'links', 'loops', 'cycles'), range(6)):
        info[name] = int((branches['kind'] == kind).sum())
    for name in steps + ('attachments',):
        info[name] = int(branches[name].astype(np.uint64).sum())
    return {'classes': classes, 'branch_ranks': branch_ranks, 'node_ranks': node_ranks, 'branches': branches, 'nodes': nodes, 'info': info}


def graph_texels(array, lo, hi, order='raster'):
    """``graph_of`` of the voxels of a uint8 or uint16 array whose code lies in lo .. hi: what ``Volume.graph(lo, hi)`` holds on the device"""
    array = _texels(array)
    lo, hi = check_range(lo, hi, int(np.iinfo(array.dtype).max))
    return graph_of((array >= lo) & (array <= hi), order)


def skeleton_graph_texels(burn, order='raster'):
    """``graph_of`` of the kept voxels of a skeleton's burn passes: what ``Skeleton.graph()`` holds on the device"""
    burn = np.asarray(burn)
    if burn.ndim != 3 or burn.dtype.kind not in 'ui':
        raise ValueError('burn passes are one unsigned integer per voxel')
    return graph_of(burn.astype(np.uint64) == np.uint64(KEPT), order)


def dropped(branches, length, weights=DEFAULT_WEIGHTS, flags=0):
    """bool per branch record: does a pruning of ``length`` drop it?"""
    length, (wf, we, wc), flags, _ = check_prune(length, weights, flags, 0, 0)
    out = np.zeros(len(branches), bool)
    for k, b in enumerate(branches):
        cost = wf * int(b['steps_face']) + we * int(b['steps_edge']) + wc * int(b['steps_corner'])
        kind = int(b['kind'])
        out[k] = (cost & ((1 << 64) - 1)) <= length and (kind == SPUR or (bool(flags & PRUNE_DEBRIS) and kind in (SEGMENT, ISOLATED)))
    return out


def prune_texels(array, graph, length, weights=DEFAULT_WEIGHTS, flags=0, fill=0):
    """the array's codes where the voxel is in the graph's set and its branch is not dropped, ``fill`` elsewhere, in the array's dtype: what
    ``Graph.prune(length, weights, debris, fill)`` holds on the device.  ``graph``: what ``graph_texels`` gave for the array."""
    array = _texels(array)
    length, weights, flags, fill = check_prune(length, weights, flags, fill, int(np.iinfo(array.dtype).max))
    classes, ranks = graph['classes'], graph['branch_ranks']
    if classes.shape != array.shape:
        raise ValueError('the graph is of another array')
    gone = np.concatenate([[False], dropped(graph['branches'], length, weights, flags)])
    stays = (classes != 0) & ~gone[ranks]
    return np.ascontiguousarray(np.where(stays, array, array.dtype.type(fill)), dtype=array.dtype)


def classes_texels(array, graph):
    """[depth][height][width][2] in the array's dtype: (code, class): what ``Graph.classes()`` holds on the device; a row of a 2-D transfer
    function colours ends (2) and junctions (4)"""
    array = _texels(array)
    if graph['classes'].shape != array.shape:
        raise ValueError('the graph is of another array')
    return np.ascontiguousarray(np.stack([array, graph['classes'].astype(array.dtype)], axis=-1))


def lengths(records, spacing=1.0):
    """float64 per branch record: (steps_face + sqrt(2) steps_edge + sqrt(3) steps_corner) * spacing, the length of the branch between the
    centres of its end voxels (and of the node voxels it attaches to) for cubic voxels of edge ``spacing``"""
    records = np.asarray(records)
    return (records['steps_face'].astype(np.float64) + np.sqrt(2.0) * records['steps_edge'].astype(np.float64) +
            np.sqrt(3.0) * records['steps_corner'].astype(np.float64)) * float(spacing)


def centreline_texels(array, lo, hi, mode='ends', prune=None, prune_rounds=1):
    """what ``Volume.centreline(lo, hi, mode, prune, prune_rounds)`` holds: the skeleton; with ``prune``, up to ``prune_rounds`` times
    graph -> prune(prune) -> skeleton again, stopping early when a round drops nothing"""
    from .skeleton import skeleton_burn_texels, burn_within_texels
    array = _texels(array)
    lo, hi = check_range(lo, hi, int(np.iinfo(array.dtype).max))
    burn, _ = skeleton_burn_texels(array, lo, hi, mode)
    if prune is not None:
        prune, prune_rounds, fill = check_centreline_prune(lo, hi, prune, prune_rounds, int(np.iinfo(array.dtype).max))
        for _ in range(prune_rounds):
            graph = skeleton_graph_texels(burn)
            if not dropped(graph['branches'], prune).any():
                break
            array = prune_texels(array, graph, prune, fill=fill)
            burn, _ = skeleton_burn_texels(array, lo, hi, mode)
    return burn_within_texels(array, burn, KEPT, KEPT, 0)
