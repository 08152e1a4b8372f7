"""The graph of a volume whose content is made of small pieces, stated piece by piece, and the content of the graph tests at scale.
Importing this touches no device.

vpt_amd.graph.graph_of visits the kept voxels one by one and labels the whole array twice: seconds on 10^7 voxels.  A graph is local: a
voxel's class depends on its 26 neighbours, branches and nodes are 26-connected, and a record sums over a branch's voxels and their
neighbours.  So when no voxel of one piece is 26-adjacent to a voxel of another, the graph of the volume is the pieces' graphs side by
side; only three things speak of the volume as a whole and are translated here:

  ranks        global, in the components' canonical order: voxels descending, then the root's linear index in the volume ascending (a
               root is the voxel of smallest linear index; moving a piece keeps the order of its voxels, so a piece's roots stay roots)
  node_lo/hi   a piece's node ranks become the volume's
  tip_lo/hi    linear indices in the piece become linear indices in the volume (a cycle's root among them)

Every count of `info` is a sum over branches, nodes or voxels and adds up.  tests/test_graph_host.py and tests/test_large_volumes_host.py
show on volumes small enough to state whole that this equals vpt_amd.graph.graph_of, byte for byte."""
import numpy as np

from vpt_amd import graph as G


def _roots(ranks, count):
    """int64 [count]: the smallest linear index of every rank 1 .. count of a rank array"""
    flat = ranks.reshape(-1)
    at = np.flatnonzero(flat)
    out = np.full(count + 1, flat.size, np.int64)
    np.minimum.at(out, flat[at], at)
    assert count == 0 or int(out[1:].max()) < flat.size
    return out[1:]


def _moved(index, piece_shape, origin, shape):
    """linear indices in pieces of `piece_shape` ([k][3] or [3]) at `origin` ([k][3] or [3]) as linear indices of the volume `shape`"""
    index = np.asarray(index, np.int64)
    pd, ph, pw = (np.asarray(piece_shape, np.int64).T[i] for i in range(3))
    oz, oy, ox = (np.asarray(origin, np.int64).T[i] for i in range(3))
    x, y, z = index % pw, index // pw % ph, index // (pw * ph)
    return ((z + oz) * shape[1] + (y + oy)) * shape[2] + (x + ox)


class Assembled:
    """what `graph_on_pieces` gives: `info`, `branches` (BRANCH_DTYPE) and `nodes` (NODE_DTYPE) of the volume, and per piece k
    `origin[k]`, `local[k]` (the dict graph_of gave for the piece's motif, shared by every piece of that motif) and the tables
    `branch_table[k]`, `node_table[k]`: the volume's rank of a local rank (entry 0 is 0)"""

    def __init__(self, shape):
        self.shape = tuple(int(s) for s in shape)
        self.info, self.branches, self.nodes = None, None, None
        self.origin, self.local, self.branch_table, self.node_table = [], [], [], []

    def classes(self, k):
        return self.local[k]['classes']

    def branch_ranks(self, k):
        return self.branch_table[k][self.local[k]['branch_ranks']]

    def node_ranks(self, k):
        return self.node_table[k][self.local[k]['node_ranks']]

    def whole(self, field):
        """[depth][height][width] of the volume: 0 but for the pieces' `field` ('classes', 'branch_ranks', 'node_ranks')"""
        out = np.zeros(self.shape, np.uint8 if field == 'classes' else np.uint32)
        for k, (oz, oy, ox) in enumerate(self.origin):
            block = getattr(self, field)(k)
            d, h, w = block.shape
            out[oz:oz + d, oy:oy + h, ox:ox + w] = block
        return out

    def statement(self):
        """the dict vpt_amd.graph.graph_of would give for the whole volume"""
        return {'classes': self.whole('classes'), 'branch_ranks': self.whole('branch_ranks'), 'node_ranks': self.whole('node_ranks'),
                'branches': self.branches, 'nodes': self.nodes, 'info': self.info}


def graph_on_pieces(shape, pieces, low_faces=True):
    """The graph of the bool volume `shape` = (depth, height, width) that is empty but for `pieces`, [(origin (z, y, x), bool array)], as an
    `Assembled`.  Two pieces do not overlap, and every face of a piece that lies inside the volume is background; both are asserted.
    (`low_faces` False: only the last plane of a piece along every axis must be background.  Two boxes that do not overlap are apart along
    some axis; there the voxels of the lower one end two planes below the first of the upper one, so no two are 26-adjacent.  A tiling of
    one period needs no more.)  Pieces that share one array object are stated once."""
    shape = tuple(int(s) for s in shape)
    out = Assembled(shape)
    stated = {}
    for origin, kept in pieces:
        if id(kept) not in stated:
            assert kept.dtype == bool and kept.ndim == 3
            g = G.graph_of(kept)
            stated[id(kept)] = (kept, g, _roots(g['branch_ranks'], len(g['branches'])), _roots(g['node_ranks'], len(g['nodes'])),
                                [(bool(np.take(kept, 0, axis).any()), bool(np.take(kept, -1, axis).any())) for axis in range(3)])
        kept, g, _, _, faces = stated[id(kept)]
        for axis in range(3):
            lo, hi = int(origin[axis]), int(origin[axis]) + kept.shape[axis]
            assert 0 <= lo and hi <= shape[axis], "a piece at %r leaves the volume" % (origin,)
            assert not (faces[axis][1] and hi < shape[axis]), "the last plane along axis %d of the piece at %r is not background" % (axis, origin)
            assert not (low_faces and faces[axis][0] and lo > 0), "the first plane along axis %d of the piece at %r is not background" % (axis, origin)
        out.origin.append(tuple(int(o) for o in origin))
        out.local.append(g)
    # no two pieces overlap: two boxes do when their intervals meet along every axis
    boxes = np.array([o + l['classes'].shape for o, l in zip(out.origin, out.local)], np.int64).reshape(-1, 6)
    lo, hi = boxes[:, :3], boxes[:, :3] + boxes[:, 3:]
    for first in range(0, len(boxes), 256):
        meet = ((lo[first:first + 256, None, :] < hi[None, :, :]) & (lo[None, :, :] < hi[first:first + 256, None, :])).all(axis=2)
        meet[np.arange(len(meet)), first + np.arange(len(meet))] = False
        assert not meet.any(), "two pieces overlap"

    ids = [id(kept) for _, kept in pieces]

    def ranked(records_of, roots_of, dtype):
        """(the records of all pieces in the pieces' order, the volume's rank of each, the first record of every piece)"""
        counts = np.array([len(records_of(l)) for l in out.local], np.int64)
        first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        if first[-1] == 0:
            return np.zeros(0, dtype), np.zeros(0, np.uint32), first
        records = np.concatenate([records_of(l) for l in out.local])
        piece = np.repeat(np.arange(len(counts)), counts)
        roots = _moved(np.concatenate([roots_of(stated[id_]) for id_ in ids]), boxes[piece, 3:], boxes[piece, :3], shape)
        order = np.lexsort((roots, -records['voxels'].astype(np.int64)))
        rank = np.empty(len(records), np.uint32)
        rank[order] = np.arange(1, len(records) + 1, dtype=np.uint32)
        return records, rank, first

    nodes, node_rank, node_first = ranked(lambda l: l['nodes'], lambda s: s[3], G.NODE_DTYPE)
    branches, branch_rank, branch_first = ranked(lambda l: l['branches'], lambda s: s[2], G.BRANCH_DTYPE)
    for k in range(len(out.local)):
        out.branch_table.append(np.concatenate([np.zeros(1, np.uint32), branch_rank[branch_first[k]:branch_first[k + 1]]]))
        out.node_table.append(np.concatenate([np.zeros(1, np.uint32), node_rank[node_first[k]:node_first[k + 1]]]))
    if len(branches) == 0:
        out.branches = np.zeros(0, G.BRANCH_DTYPE)
    else:
        piece = np.repeat(np.arange(len(out.local)), np.diff(branch_first))
        for name in ('tip_lo', 'tip_hi'):
            branches[name] = _moved(branches[name], boxes[piece, 3:], boxes[piece, :3], shape).astype(np.uint64)
        padded = np.concatenate([node_rank, np.zeros(1, np.uint32)])      # a local rank of 0 reads the appended 0
        for name in ('node_lo', 'node_hi'):
            local = branches[name].astype(np.int64)
            branches[name] = padded[np.where(local > 0, node_first[piece] + local - 1, len(node_rank))]
        ordered = np.empty_like(branches)
        ordered[branch_rank.astype(np.int64) - 1] = branches
        out.branches = ordered
    if len(nodes) == 0:
        out.nodes = np.zeros(0, G.NODE_DTYPE)
    else:
        ordered = np.empty_like(nodes)
        ordered[node_rank.astype(np.int64) - 1] = nodes
        out.nodes = ordered
    out.info = {name: int(sum(l['info'][name] for l in out.local)) for name in G.INFO_FIELDS}
    return out


def dropped(branches, length, weights=G.DEFAULT_WEIGHTS, flags=0):
    """vpt_amd.graph.dropped without a Python loop over the records (2^21 of them in the dust tiling); tests/test_graph_host.py holds it to
    the original.  The cost wraps modulo 2^64 as there."""
    length, (wf, we, wc), flags, _ = G.check_prune(length, weights, flags, 0, 0)
    with np.errstate(over='ignore'):
        cost = np.uint64(wf) * branches['steps_face'] + np.uint64(we) * branches['steps_edge'] + np.uint64(wc) * branches['steps_corner']
    kind = branches['kind']
    sort = (kind == G.SPUR) | (bool(flags & G.PRUNE_DEBRIS) & ((kind == G.SEGMENT) | (kind == G.ISOLATED)))
    return sort & (cost <= np.uint64(length))


def prune_texels(array, classes, branch_ranks, branches, length, weights=G.DEFAULT_WEIGHTS, flags=0, fill=0):
    """vpt_amd.graph.prune_texels from the statement's parts, with the vectorised `dropped`"""
    gone = np.concatenate([[False], dropped(branches, length, weights, flags)])
    return np.ascontiguousarray(np.where((classes != 0) & ~gone[branch_ranks], array, array.dtype.type(fill)), dtype=array.dtype)


# ---- the list of kept voxels as k_gr_links sees it -----------------------------------------------------------------------------------
def wave_runs(statement):
    """The kept voxels in linear order, 64 a wave, the branch rank as key (0 for a node voxel), cut into runs of one key: per wave a list
    of (key, first lane, lanes).  This is what the links pass sums along a wave before it touches a record."""
    classes = statement['classes'].reshape(-1)
    at = np.flatnonzero(classes)
    keys = np.where(classes[at] <= 3, statement['branch_ranks'].reshape(-1)[at], 0).astype(np.int64)
    waves = []
    for base in range(0, len(keys), 64):
        k = keys[base:base + 64]
        heads = [0] + [i for i in range(1, len(k)) if k[i] != k[i - 1]]
        waves.append([(int(k[a]), a, b - a) for a, b in zip(heads, heads[1:] + [len(k)])])
    return waves


def wave_conditions(waves):
    """{condition: the waves that meet it} of what `wave_runs` gave:
      'full'       one run fills all 64 lanes
      'carried'    a run begins at a lane other than 0, reaches lane 63, and the next two waves begin with its key
      'apart'      at least three runs, two of them of one branch with a run of another branch (not node voxels) between them
      'over nodes' node voxels (key 0) alone separate two runs of one branch
      'last lane'  the last run is lane 63 alone"""
    met = {'full': [], 'carried': [], 'apart': [], 'over nodes': [], 'last lane': []}
    for w, runs in enumerate(waves):
        if len(runs) == 1 and runs[0][0] != 0 and runs[0][2] == 64:
            met['full'].append(w)
        key, lane, lanes = runs[-1]
        if key != 0 and lane > 0 and lane + lanes == 64 and lanes > 1 and w + 2 < len(waves) and waves[w + 1][0][0] == key and waves[w + 2][0][0] == key:
            met['carried'].append(w)
        if lane == 63 and lanes == 1 and key != 0:
            met['last lane'].append(w)
        for i in range(len(runs) - 2):
            if runs[i][0] != 0 and runs[i][0] == runs[i + 2][0]:
                met['over nodes' if runs[i + 1][0] == 0 else 'apart'].append(w)
    return met


# ---- content -----------------------------------------------------------------------------------------------------------------------
def padded(kept, margin=1):
    return np.pad(kept, margin)


def tiling(shape, motif, last=None):
    """[(origin, motif)] of every whole period of `motif` in `shape`, the same array object each; `last`: the piece of the period that
    ends at the volume's last voxel (of the motif's shape), so the end of every list is not a copy of its beginning"""
    d, h, w = motif.shape
    pieces = [((z, y, x), motif) for z in range(0, shape[0] - d + 1, d) for y in range(0, shape[1] - h + 1, h) for x in range(0, shape[2] - w + 1, w)]
    if last is not None:
        assert last.shape == motif.shape and all(s % m == 0 for s, m in zip(shape, motif.shape))
        pieces[-1] = (pieces[-1][0], last)
    return pieces


def set_of(shape, pieces):
    out = np.zeros(shape, bool)
    for (oz, oy, ox), kept in pieces:
        d, h, w = kept.shape
        out[oz:oz + d, oy:oy + h, ox:ox + w] = kept
    return out


def dust_motif():
    """[8][16][64]: voxels on even coordinates only, two apart: isolated voxels; four of the 32 rows hold two-voxel segments along x on a
    period of three instead.  980 branches in 8192 voxels; the last plane along every axis is background"""
    m = np.zeros((8, 16, 64), bool)
    m[::2, ::2, ::2] = True
    for z, y in ((0, 4), (2, 10), (4, 0), (6, 14)):
        m[z, y] = False
        m[z, y, 0:63:3] = True
        m[z, y, 1:63:3] = True
    return m


def wave_case():
    """[3][9][300], what `wave_runs` needs to show (tests/test_graph_host.py says which waves do):
      z 0, y 0   37 isolated voxels, then a line of 200 along x: a run that begins at lane 37, fills the next two waves and ends in a fourth
      z 0, y 2   25 isolated voxels: list positions 237 .. 261, so lane 63 of the fourth wave is a run of its own
      z 2        a ring in the xy plane with an isolated voxel inside it and a two-voxel tooth on its upper row: the tooth makes three voxels
                 of that row a node between two runs of the ring, which is one branch (a loop); the isolated voxel parts two more of them
      z 2        a comb: a spine along x with two-voxel teeth every fourth voxel: node voxels between one-voxel branches"""
    m = np.zeros((3, 9, 300), bool)
    m[0, 0, 0:74:2] = True
    m[0, 0, 75:275] = True
    m[0, 2, 0:50:2] = True
    L, R, a, b = 4, 16, 3, 8
    m[2, a, L + 1:R] = True
    m[2, b, L + 1:R] = True
    m[2, a + 1:b, L] = True
    m[2, a + 1:b, R] = True
    m[2, a + 2, L + 2] = True                                     # inside the ring
    m[2, a - 2:a, 10] = True                                      # the tooth
    m[2, 4, 40:121] = True                                        # the comb's spine
    m[2, 2:4, 42:120:4] = True
    return m
