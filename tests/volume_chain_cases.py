"""Fixed-seed chains of volume operations and what every step must give, from numpy and the vpt_amd statements alone (no device, no
_native): the cases of tests/test_gpu_volume_chain_fuzz.py; tests/test_volume_chain_cases.py holds the drawn set to its conditions.

``chain(seed)`` is a list of steps.  A step is a dict:

  op       the operation's name (a key of LEGAL; step 0 is always 'source')
  sub      the rank operator or the combine operation, None elsewhere: 'rank' and 'combine' are drawn, and counted, per sub-operation
  src      the index of the chain volume the step reads (volume k is the k-th one the chain made; the source is volume 0)
  out      the index of the volume the step makes; None for a scalar step and for upload_block, which changes volume ``src``
  kwargs   plain ints, floats, strings and small arrays: what the public method is called with ('b': ('volume', index) or ('fresh', texels))
  expect   the statement's result: the texels of volume ``out`` (upload_block: of volume ``src`` from then on), or the scalar result
  shape    (depth, height, width) of the volume the kernels of the step run over (resample: the target grid)
  format   the format of volume ``src``
  b_source for combine / compare, and the mask of a reconstruct and the values of a measure: where B comes from (B_SOURCES)
  facts    (steps of the later units) what the statements said of the step when it was drawn
  forced   (steps of the later units) None, or the value of the hook through which the step runs a second time

How a case is drawn.  Every sixteenth seed is one voxel.  The next PLANNED seeds take their shape from PLANS, which walks each kernel
family's tile extents (1, one below the tile, the tile, one above, two tiles plus one on every axis), and begin with that family's
operations: independent draws from the pools would need thousands of seeds to put 257 on the x axis of a volume that then happens to
be smoothed.  Every other seed draws each axis from the three pools (1 .. 9; 1 .. 80; EDGES) and its format by turns from FORMATS.
Steps: 3 .. 6; a step is upload_block with probability 0.25 (never first, last or twice in a row), a scalar with 0.25, a volume-producing operation otherwise, uniform among
the entries legal for the current format, the entries the chain has not used yet first; each seed also has three wishes, taken by turns
from the whole entry list, that go first where they are legal.  48 seeds did not reach every entry three times; the default 128 do.  A volume-producing step whose
expected texels are constant is drawn again, up to 8 times (constancy cascades: every later step would see a constant volume).

Seeds 0 .. 127 are drawn by these rules from the entries of the first units (OLD_ENTRIES) and are, chain for chain and byte for byte, what
they were before the later units (LATER: geodesic, reconstruct, watershed, split, keep_set, measure, thickness, skeleton) joined.

Seeds from LATER_SEEDS = 128 on are drawn by the later rules (``_draw_later_chain``).  A source is R8, R16, RG8 or RG16, one voxel every
sixteenth seed; the next len(LATER_PLANS) seeds take shape, first entries and style from LATER_PLANS (the tile extents of the later
kernel families, 31 / 32 / 33 for the words of the skeleton's bit planes, and the shapes the conditions name); the others draw their axes
as above under 20 000 voxels (every third: 40 000) and a style among noise, sphere, sparse and blobs (smoothed noise).  A step is
upload_block with probability 0.2, a scalar with 0.25, else volume-producing; three times in four it is an entry of the later units, else
one of the first; the first step makes a volume; wishes run over LATER_ENTRIES.  A thinning or thickness step is legal up to SLOW_VOXELS
voxels only (their statements take seconds beyond).  The mask of a reconstruct, the values of a measure and the ``texels`` of a watershed
are second volumes drawn as B is (fresh, earlier, self, a channel of a two-channel volume).  A chain must hold two steps of the later
units, one of which reads a volume a derive step made, else it is drawn again from the seed's next stream.  Every fourth seed (seed % 4
== 3) forces the slow paths: its steps of the families of FORCED carry 'forced', the hook's value, and run plainly and through the hook.
A later step carries 'facts': what the statements said of it when it was drawn (passes, basins, centre tiles ...), for the conditions.

Seeds from GRAPH_SEEDS = 224 on are drawn by the graph rules (``_draw_later_chain(graph=True)``, ``_draw_graph_step``): the later rules
with an R8 or R16 source of 200 .. GRAPH_VOXELS voxels (blobs, a sphere or sparse noise), GRAPH_PLANS for the first ten, wishes over
GRAPH_ENTRIES, and a step that is, three times in five, an entry of GRAPH: a centreline with pruning rounds, the pruning, the class pair
and the records of the graph of a value range or of a skeleton, and its branches and nodes as Components once the graph is gone.  A chain
must hold two such steps, one of which reads a derived volume.  The entries of GRAPH are in none of the lists above and every draw the
rules add stands behind ``if graph``: the chains of seeds 0 .. 223 are, byte for byte, what they were (pinned by digest in
tests/test_volume_chain_cases.py).

The later rules alone end at 224: the smallest multiple of 16 at which every condition of tests/test_volume_chain_cases.py held.  The last to
come are every (format, entry) pair (RG8 basins_label first occurs in 208 .. 223), a labelling with more than 512 ranks in one block
of the measuring kernel together with values from a derived pair's second channel (192 .. 207), and three steps of every forced hook
(reconstruct's: 192 .. 207)."""
import functools

import numpy as np

import vpt_amd
from vpt_amd.combine import combine_texels, compare_stats
from vpt_amd.components import components_texels, keep_texels, label_texels
from vpt_amd.distance import (distance_squared_texels, within_texels, channel_texels, thickness_squared_texels, thickness_texels, open_ball_texels,
                              check_radius)
from vpt_amd.gradient import gradient_magnitude
from vpt_amd.pyramid import reduce_texels, smooth_texels
from vpt_amd.measure import measure_texels, keep_set_texels
from vpt_amd.rank import rank_texels, OPERATORS as RANK_OPERATORS
from vpt_amd.reconstruct import geodesic_texels, reconstruct_texels, GEODESIC_OPS, RECONSTRUCT_OPS, TAKES_H
from vpt_amd.resample import resample_texels
from vpt_amd.skeleton import skeleton_burn_texels, burn_within_texels, skeleton_texels, KEPT, MODES as SKELETON_MODES
from vpt_amd.watershed import watershed_texels, split_texels
from vpt_amd.window import window_texels, percentile_window

CONSTANT = 20261019
DEFAULT_SEEDS = (0, 256)
LATER_SEEDS = 128                                      # the first seed drawn by the later rules (module docstring)
GRAPH_SEEDS = 224                                      # the first seed drawn by the graph rules (module docstring)
GRAPH_VOXELS = 6000                                    # the sources of those seeds: the graph statement visits kept voxels one by one
MAX_VOXELS = 100000
SLOW_VOXELS = 20000                                    # the thinning and thickness statements: seconds beyond (tests/test_gpu_thickness_fuzz.py's cap)
MAX_ROW_PASS = 400000                                  # resample: target width x source height x source depth (the row pass's workspace)
REDRAWS = 8

# name -> (numpy dtype, channels)
FORMATS = {'R8': (np.uint8, 1), 'R16': (np.uint16, 1), 'RG8': (np.uint8, 2), 'RG16': (np.uint16, 2), 'R8_SNORM': (np.int8, 1),
           'R16_SNORM': (np.int16, 1), 'R32F': (np.float32, 1), 'RG32F': (np.float32, 2)}
_U1 = ('R8', 'R16')
_ONE = ('R8', 'R16', 'R8_SNORM', 'R16_SNORM', 'R32F')
_INT1 = ('R8', 'R16', 'R8_SNORM', 'R16_SNORM')
_UNORM = ('R8', 'R16', 'RG8', 'RG16')
# operation -> the formats of the volume it is called on (the docstrings of vpt_amd/volume.py)
LEGAL = {
    'window': _ONE, 'derive_gradient': _U1, 'reduce': tuple(FORMATS), 'smooth': _U1, 'rank': _U1,
    'keep': _U1, 'label': _U1,                         # Volume.components(...) -> Components.keep / .label
    'within': _U1, 'channel': _U1,                     # Volume.distance(...) -> Distance.within / .channel
    'resample': tuple(FORMATS),                        # 'filtered': _UNORM only (RESAMPLE_FILTERED)
    'combine': _U1,                                    # B: _UNORM
    'upload_block': tuple(FORMATS),
    'range': _ONE, 'histogram': _UNORM, 'code_histogram': _INT1, 'percentile_window': _INT1, 'compare': _U1,
    'components_info': _U1, 'components_list': _U1, 'components_ranks': _U1, 'distance_info': _U1, 'distance_squared': _U1,
}
OLD_OPS = tuple(LEGAL)
# the later units: reconstruction, watershed, measurements, thickness, skeleton
LATER = {
    'geodesic': _UNORM, 'reconstruct': _UNORM,         # sub: the operation; the mask of a reconstruct: a B source of the marker's width
    'basins_keep': _UNORM, 'basins_label': _UNORM, 'basins_keep_set': _UNORM,      # Volume.watershed(...) -> Components.keep / .label / .keep_set
    'split_keep': _U1, 'split_label': _U1,             # Volume.split(...) -> Components.keep / .label
    'keep_set': _U1,                                   # Volume.components(...) -> Components.keep_set
    'thickness': _U1, 'open_ball': _U1,
    'thickness_within': _U1, 'thickness_channel': _U1,      # Volume.distance(...) -> Distance.thickness() -> .within / .channel
    'centreline': _U1, 'skeleton_within': _U1,         # sub of centreline: the mode; Volume.skeleton(...) -> Skeleton.within
    'basins_info': _UNORM, 'basins_list': _UNORM, 'basins_ranks': _UNORM, 'measure': _U1, 'basins_measure': _UNORM,
    'thickness_squared': _U1, 'thickness_info': _U1, 'skeleton_burn': _U1, 'skeleton_info': _U1,
}
LEGAL.update(LATER)
# the skeleton graph: the set is a value range of the volume (Volume.graph) or the kept voxels of its skeleton (Skeleton.graph)
GRAPH = {
    'centreline_prune': _U1,                           # Volume.centreline(lo, hi, mode, prune, prune_rounds)
    'graph_prune': _U1, 'graph_classes': _U1,          # Graph.prune(length, weights, debris, fill); Graph.classes(): the (code, class) pair
    'branches_keep_set': _U1, 'nodes_label': _U1,      # Graph.branches / .nodes, used after the graph has been destroyed
    'graph_info': _U1, 'graph_branches': _U1, 'graph_nodes': _U1,
}
LEGAL.update(GRAPH)
GRAPH_SCALAR_OPS = ('graph_info', 'graph_branches', 'graph_nodes')
RESAMPLE_FILTERED = _UNORM
COMBINE_OPS = ('mask', 'min', 'max', 'absdiff', 'blend', 'pair')
SCALAR_OPS = ('range', 'histogram', 'code_histogram', 'percentile_window', 'compare', 'components_info', 'components_list',
              'components_ranks', 'distance_info', 'distance_squared')
LATER_SCALAR_OPS = ('basins_info', 'basins_list', 'basins_ranks', 'measure', 'basins_measure', 'thickness_squared', 'thickness_info',
                    'skeleton_burn', 'skeleton_info')
B_SOURCES = ('fresh', 'earlier', 'self', 'rg_channel', 'other_width')
SUBS = {'rank': tuple(RANK_OPERATORS), 'combine': COMBINE_OPS, 'geodesic': tuple(GEODESIC_OPS), 'reconstruct': tuple(RECONSTRUCT_OPS),
        'centreline': tuple(SKELETON_MODES)}
# the hooks that force a unit's slow path (include/vpt.h "(for tests)"), by the step's family: the step runs plainly and forced
FORCED = {'skeleton': (1,), 'thickness': (1, 2, 3), 'reconstruct': (1,), 'watershed': ((3, 1, 1),)}
UNHOOKED = ('geodesic', 'split_keep', 'split_label')    # of those families, the public methods without a hook


def _entries(ops):
    out = []
    for op in ops:
        out += [(op, sub) for sub in SUBS.get(op, (None,))]
    return out


# the entries seeds 0 .. 127 are drawn from: those chains stay what they were before the later units joined
OLD_VOLUME_ENTRIES = _entries(op for op in OLD_OPS if op not in SCALAR_OPS and op != 'upload_block')
OLD_SCALAR_ENTRIES = _entries(SCALAR_OPS)
OLD_ENTRIES = OLD_VOLUME_ENTRIES + OLD_SCALAR_ENTRIES + [('upload_block', None)]
LATER_VOLUME_ENTRIES = _entries(op for op in LATER if op not in LATER_SCALAR_OPS)
LATER_SCALAR_ENTRIES = _entries(LATER_SCALAR_OPS)
LATER_ENTRIES = LATER_VOLUME_ENTRIES + LATER_SCALAR_ENTRIES
VOLUME_ENTRIES = OLD_VOLUME_ENTRIES + LATER_VOLUME_ENTRIES
SCALAR_ENTRIES = OLD_SCALAR_ENTRIES + LATER_SCALAR_ENTRIES
ENTRIES = OLD_ENTRIES + LATER_ENTRIES
# the entries of the graph rules: kept apart, so that the chains of seeds 0 .. 223 stay what they were (ENTRIES is what they are drawn from)
GRAPH_VOLUME_ENTRIES = [(op, None) for op in GRAPH if op not in GRAPH_SCALAR_OPS]
GRAPH_SCALAR_ENTRIES = [(op, None) for op in GRAPH_SCALAR_OPS]
GRAPH_ENTRIES = GRAPH_VOLUME_ENTRIES + GRAPH_SCALAR_ENTRIES

# kernel family -> the extents (x, y, z) of its tile; None: the kernel has no tile along that axis
TILES = {
    'gradient': (128, 8, 32),                          # GR_TX, GR_TY, GR_TZ (vpt_volume_ops.hip)
    'smooth': (128, 8, 32),                            # SM_TX, SM_TY, SM_TZ (vpt_volume_pyramid.hip)
    'rank': (128, 8, 32),                              # RK_TX, RK_TY, RK_TZ (vpt_volume_rank.hip)
    'components': (64, 8, 4),                          # CC_TX, CC_TY, CC_TZ (vpt_volume_components.hip)
    'distance': (64, None, None),                      # the 64-voxel row segments of k_edt_x (vpt_volume_distance.hip); y and z are marched whole
    'resample': (64, 4, None),                         # k_resample_yz: 64 columns x 4 rows of the TARGET grid a workgroup, one plane each
    'reconstruct': (64, 8, 4),                         # RC_TX, RC_TY, RC_TZ (vpt_volume_reconstruct.hip)
    'watershed': (64, 8, 4),                           # the plateau kernel's tile and the labelling's (vpt_volume_watershed.hip)
    'skeleton': (64, 8, 4),                            # SK_TX, SK_TY, SK_TZ; a word of a bit plane is 32 voxels of a row (vpt_volume_skeleton.hip)
    'measure': (64, 8, 8),                             # the block of one MS_SLOTS table (vpt_volume_measure.hip)
    'thickness': (8, 8, 4),                            # TH_TX, TH_TY, TH_TZ (vpt_volume_thickness.hip)
}
FAMILY = {'derive_gradient': 'gradient', 'smooth': 'smooth', 'rank': 'rank', 'keep': 'components', 'label': 'components',
          'components_info': 'components', 'components_list': 'components', 'components_ranks': 'components', 'within': 'distance',
          'channel': 'distance', 'distance_info': 'distance', 'distance_squared': 'distance', 'resample': 'resample',
          'geodesic': 'reconstruct', 'reconstruct': 'reconstruct', 'basins_keep': 'watershed', 'basins_label': 'watershed',
          'basins_keep_set': 'watershed', 'basins_info': 'watershed', 'basins_list': 'watershed', 'basins_ranks': 'watershed',
          'split_keep': 'watershed', 'split_label': 'watershed', 'keep_set': 'components', 'measure': 'measure', 'basins_measure': 'measure',
          'thickness': 'thickness', 'open_ball': 'thickness', 'thickness_within': 'thickness', 'thickness_channel': 'thickness',
          'thickness_squared': 'thickness', 'thickness_info': 'thickness', 'centreline': 'skeleton', 'skeleton_within': 'skeleton',
          'skeleton_burn': 'skeleton', 'skeleton_info': 'skeleton'}
FAMILY.update({op: 'graph' for op in GRAPH})
SLOW_FAMILIES = ('thickness', 'skeleton')              # at most SLOW_VOXELS voxels a step
# the kernels with a vector form and a texel-by-texel form, chosen by the row length: nx % 4 (gradient, smooth, rank: ALIGNED), the row's
# bytes % 32 (k_reduce); window and combine go by 16-byte groups of the whole volume
VECTOR_FAMILIES = ('gradient', 'smooth', 'rank')


def tile_extents(tile, word=None):
    """the extents an axis with this tile must be seen at; ``word``: the voxels of a machine word along the axis (the skeleton's bit
    planes along x: 32), seen at one below, at and one above it as well"""
    if tile is None:
        return (1,)
    return (1, tile - 1, tile, tile + 1, 2 * tile + 1) + ((word - 1, word, word + 1) if word else ())


WORD = {('skeleton', 'x'): 32}                         # (family, axis) -> the ``word`` of tile_extents


EDGES = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 132, 133, 255, 256, 257, 260)
EDGES_YZ = EDGES + (3, 4, 5, 7, 8, 9)


def _plans():
    """[(shape (depth, height, width), the entries the chain begins with)]: per tile geometry five shapes whose axes walk that
    geometry's extents, rotated against each other so that the largest extents never meet (the voxel cap)"""
    plans = []
    for families, begin in ((('gradient',), [('smooth', None), ('rank', 'median'), ('derive_gradient', None), ('rank', 'dilate')]),
                            (('components', 'distance'), [('keep', None), ('within', None), ('label', None), ('channel', None)])):
        tx, ty, tz = TILES[families[0]]
        xs, ys, zs = tile_extents(tx), tile_extents(ty), tile_extents(tz)
        for k in range(5):
            shape = (zs[(k + 2) % 5], ys[(k + 1) % 5], xs[k])
            assert shape[0] * shape[1] * shape[2] <= MAX_VOXELS
            plans.append((shape, begin, None))
    tx, ty, _ = TILES['resample']
    xs, ys = tile_extents(tx), tile_extents(ty)
    for k in range(5):                                            # the target grid walks the extents; the source is drawn
        plans.append((None, [('resample', None)], (None, ys[(k + 1) % 5], xs[k])))
    return plans


PLANS = _plans()
PLANNED = len(PLANS)


def _later_plans():
    """[(shape, the entries the chain begins with, the source's style)] of the seeds from LATER_SEEDS on: per tile geometry of the later
    units five shapes rotated as in ``_plans``, each beginning with one entry of every family of the geometry (so every family sees every
    extent), the skeleton's word extents, and the shapes the conditions of tests/test_volume_chain_cases.py name: 129 x 17 x 9, the
    largest a thinning or thickness step takes (153 thickness tiles, three skeleton tiles along x), 27^3 (a ball deeper than a
    thickness tile is wide) and two tiles of noise for the measuring table"""
    plans = []
    reconstruct = [('reconstruct', 'dilation'), ('geodesic', 'hmax'), ('reconstruct', 'erosion'), ('geodesic', 'fill_holes'), ('geodesic', 'dome')]
    watershed = [('basins_keep', None), ('basins_ranks', None), ('basins_keep_set', None), ('split_keep', None), ('basins_list', None)]
    skeleton = [('centreline', 'ends'), ('skeleton_within', None), ('centreline', 'kernel'), ('skeleton_burn', None), ('centreline', 'isthmus')]
    thickness = [('thickness', None), ('open_ball', None), ('thickness_within', None), ('thickness_channel', None), ('thickness_squared', None)]
    measure = [('basins_measure', None), ('measure', None)]

    def walk(family, begins, styles):
        tx, ty, tz = TILES[family]
        xs, ys, zs = tile_extents(tx), tile_extents(ty), tile_extents(tz)
        for k in range(5):
            shape = (zs[(k + 2) % 5], ys[(k + 1) % 5], xs[k])
            begin = [b[k % len(b)] for b in begins]
            plans.append((shape, begin[k % len(begin):] + begin[:k % len(begin)], styles[k % len(styles)]))

    walk('skeleton', (skeleton, reconstruct, watershed), ('blobs', 'noise', 'sphere'))
    for shape, k in (((5, 9, 31), 0), ((4, 7, 32), 2), ((9, 8, 33), 4)):             # the word of the skeleton's bit planes
        plans.append((shape, [skeleton[k], thickness[k], skeleton[1]], 'blobs'))
    walk('measure', (measure, measure[::-1], [('keep_set', None)] * 5), ('noise',))
    walk('thickness', (thickness, thickness[2:] + thickness[:2], [('thickness_info', None)] * 5), ('blobs', 'noise', 'sphere'))
    plans.append(((9, 17, 129), [('thickness_squared', None), ('skeleton_burn', None), ('basins_keep', None)], 'noise'))
    plans.append(((9, 17, 129), [('thickness', None), ('centreline', 'ends'), ('basins_measure', None)], 'blobs'))
    plans.append(((5, 17, 129), [('skeleton_within', None), ('thickness_channel', None), ('geodesic', 'maxima')], 'blobs'))
    plans.append(((27, 27, 27), [('thickness_within', None), ('open_ball', None), ('centreline', 'kernel')], 'sphere'))
    plans.append(((17, 17, 129), [('basins_label', None), ('basins_measure', None), ('measure', None)], 'noise'))
    for shape, _, _ in plans:
        assert shape[0] * shape[1] * shape[2] <= MAX_VOXELS
    return plans


LATER_PLANS = _later_plans()
# the seeds of the graph rules that are planned: every graph entry begins a chain on both widths, on shapes that cross a word of the
# bit plane (32), a 64-voxel segment and a labelling tile (64 x 8 x 4)
GRAPH_PLANS = [
    ((5, 9, 65), [('centreline_prune', None), ('graph_info', None), ('graph_prune', None)], 'blobs'),
    ((9, 17, 33), [('graph_prune', None), ('graph_classes', None), ('graph_branches', None)], 'sphere'),
    ((6, 10, 70), [('graph_classes', None), ('branches_keep_set', None), ('graph_nodes', None)], 'blobs'),
    ((9, 8, 66), [('branches_keep_set', None), ('nodes_label', None), ('graph_info', None)], 'blobs'),
    ((12, 14, 31), [('nodes_label', None), ('centreline_prune', None), ('graph_branches', None)], 'sphere'),
    ((5, 16, 64), [('graph_nodes', None), ('graph_prune', None), ('centreline_prune', None)], 'blobs'),
    ((7, 9, 96), [('graph_info', None), ('graph_classes', None), ('nodes_label', None)], 'blobs'),
    ((13, 13, 32), [('graph_branches', None), ('branches_keep_set', None), ('graph_prune', None)], 'sphere'),
    ((4, 11, 129), [('centreline_prune', None), ('graph_nodes', None), ('graph_classes', None)], 'blobs'),
    ((10, 12, 40), [('graph_prune', None), ('nodes_label', None), ('graph_info', None)], 'sphere'),
]


# ---- texels --------------------------------------------------------------------------------------------------------------------
def stored(a):
    """what a volume's storage holds once finalized: SNORM's most negative code reads as the one above it"""
    return np.maximum(a, -np.iinfo(a.dtype).max) if a.dtype.kind == 'i' else a


def _sphere(shape):
    d, h, w = shape
    z, y, x = (((np.arange(n) + 0.5) / n - 0.5) ** 2 for n in (d, h, w))
    return np.clip(1.0 - np.sqrt(z[:, None, None] + y[None, :, None] + x[None, None, :]) / 0.45, 0.0, 1.0)


def draw_texels(rng, fmt, shape, style=None, specials=False):
    """texels of ``fmt`` over ``shape``: 'noise' (uniform over every code), 'sphere' (a noisy sphere), 'sparse' (about 70 % background).
    Floats reach beyond [0, 1]; ``specials`` puts NaN, +-0 and +-inf into a float volume"""
    dtype, channels = FORMATS[fmt]
    full = tuple(shape) + ((2,) if channels == 2 else ())
    style = style or ('noise', 'sphere', 'sparse')[int(rng.integers(3))]
    if dtype == np.float32:
        if style == 'noise':
            v = rng.uniform(-0.5, 1.5, full)
        elif style == 'sphere':
            v = _sphere(shape).reshape(tuple(shape) + (1,) * (len(full) - 3)) * 1.3 - 0.1 + rng.normal(0, 0.08, full)
        else:
            v = np.where(rng.random(full) < 0.7, 0.0, rng.uniform(-0.25, 2.0, full))
        v = v.astype(np.float32)
        if specials:
            pick = rng.random(full)
            for k, special in enumerate((np.nan, np.inf, -np.inf, -0.0, 0.0)):
                v[(pick >= 0.004 * k) & (pick < 0.004 * (k + 1))] = special
            flat = v.reshape(-1)
            flat[:5] = (np.nan, np.inf, -np.inf, -0.0, 0.0)[:flat.size]
        return v
    info = np.iinfo(dtype)
    if style == 'noise':
        v = rng.integers(info.min, info.max + 1, size=full)
    elif style == 'sphere':
        base = _sphere(shape).reshape(tuple(shape) + (1,) * (len(full) - 3))
        v = info.min + base * (info.max - info.min) + rng.normal(0, 0.06 * (info.max - info.min), full)
    elif style == 'blobs':                                        # (asked for by name only) noise averaged over 3 x 3 x 3 boxes twice, over every code
        v = rng.random(full)
        for _ in range(2):
            p = np.pad(v, [(1, 1)] * 3 + [(0, 0)] * (len(full) - 3), mode='edge')
            v = sum(p[dz:dz + shape[0], dy:dy + shape[1], dx:dx + shape[2]] for dz in range(3) for dy in range(3) for dx in range(3)) / 27.0
        v = info.min + (v - v.min()) / max(float(v.max() - v.min()), 1e-9) * (info.max - info.min)
    else:
        background = 0 if info.min == 0 else int(info.min)        # SNORM: the most negative code, which storage reads as the one above it
        v = np.where(rng.random(full) < 0.7, background, rng.integers(info.min, info.max + 1, size=full))
    return np.clip(np.rint(v), info.min, info.max).astype(dtype)


def format_of(texels):
    for name, (dtype, channels) in FORMATS.items():
        if texels.dtype == dtype and channels == (2 if texels.ndim == 4 else 1):
            return name
    raise ValueError('no format for %s %r' % (texels.dtype, texels.shape))


def _axis(rng, edges):
    pool = int(rng.integers(3))
    if pool == 0:
        return int(rng.integers(1, 10))
    if pool == 1:
        return int(rng.integers(1, 81))
    return int(edges[int(rng.integers(len(edges)))])


def draw_shape(rng, fixed=(None, None, None), fits=lambda s: s[0] * s[1] * s[2] <= MAX_VOXELS):
    """(depth, height, width), every free axis from the three pools, drawn again while ``fits`` refuses it"""
    while True:
        shape = tuple(f if f is not None else _axis(rng, EDGES if k == 2 else EDGES_YZ) for k, f in enumerate(fixed))
        if fits(shape):
            return shape


def _box(rng, shape):
    """(x, y, z, w, h, d): one time in four 1 wide along an axis, one in four ending at the far corner"""
    d, h, w = shape
    size = [int(rng.integers(1, n + 1)) for n in (w, h, d)]
    kind = int(rng.integers(4))
    if kind == 0:
        size[int(rng.integers(3))] = 1
    start = [int(rng.integers(0, n - s + 1)) for n, s in zip((w, h, d), size)]
    if kind == 1:
        start = [n - s for n, s in zip((w, h, d), size)]
    return tuple(start) + tuple(size)


def _quantiles(rng, texels):
    """two codes (lo <= hi) at random quantiles of a one-channel integer volume"""
    flat = np.sort(texels.reshape(-1))
    a, b = sorted(int(flat[int(q * (flat.size - 1))]) for q in rng.random(2))
    return a, b


# ---- one chain -----------------------------------------------------------------------------------------------------------------
class _Chain:
    def __init__(self, seed):
        self.seed = seed
        self.rng = np.random.default_rng(CONSTANT + seed)
        self.steps = []
        self.texels = []                                          # the expected texels of every volume, as they are now
        self.used = set()
        self.fine = False                                         # (later plans) measure everything over a watershed of noise

    def add_volume(self, texels):
        self.texels.append(texels)
        return len(self.texels) - 1

    def one_channel_before(self, index):
        for k in range(index, -1, -1):
            if self.texels[k].ndim == 3:
                return k
        return None

    def same_grid(self, index, formats):
        shape = self.texels[index].shape[:3]
        return [k for k, t in enumerate(self.texels) if t.shape[:3] == shape and format_of(t) in formats]


def _field_args(c, texels):
    lo, hi = _quantiles(c.rng, texels)
    return lo, hi


def _draw_b(c, cur, a, op):
    """(kind, kwargs 'b', channel, B's texels) of a combine / compare of volume ``cur``"""
    rng = c.rng
    fmt = format_of(a)
    wide = fmt == 'R16'
    kind = B_SOURCES[int(rng.integers(len(B_SOURCES)))]
    if kind == 'other_width' and op not in ('mask', 'compare'):
        kind = 'fresh'
    if c.same_grid(cur, ('RG16' if wide else 'RG8',)) and rng.random() < 0.6:      # the chain made a two-channel volume of this grid: a label or gradient channel
        kind = 'rg_channel'
    elif op == 'compare' and len(c.same_grid(cur, _UNORM)) > 1 and rng.random() < 0.5:      # few chains hold a second volume of the grid
        kind = 'earlier'
    channel = 0
    if kind == 'self':
        return kind, ('volume', cur), 0, a
    if kind == 'earlier':
        found = [k for k in c.same_grid(cur, _UNORM if op == 'compare' else (fmt,)) if k != cur]      # compare takes mixed widths
        if found:
            k = found[int(rng.integers(len(found)))]
            return kind, ('volume', k), (int(rng.integers(2)) if c.texels[k].ndim == 4 else 0), c.texels[k]
        kind = 'fresh'
    if kind == 'rg_channel':
        channel = int(rng.integers(2))
        found = c.same_grid(cur, ('RG16' if wide else 'RG8',))
        if found:
            k = found[int(rng.integers(len(found)))]
            return kind, ('volume', k), channel, c.texels[k]
        b = draw_texels(rng, 'RG16' if wide else 'RG8', a.shape)
        return kind, ('fresh', b), channel, b
    if kind == 'other_width':
        found = c.same_grid(cur, ('R8', 'RG8') if wide else ('R16', 'RG16'))
        if found and rng.random() < 0.5:
            k = found[int(rng.integers(len(found)))]
            b = c.texels[k]
        else:
            k, b = None, draw_texels(rng, ('R8', 'RG8', 'R16', 'RG16')[(0 if wide else 2) + int(rng.integers(2))], a.shape)
        channel = int(rng.integers(2)) if b.ndim == 4 else 0
        return kind, (('volume', k) if k is not None else ('fresh', b)), channel, b
    b = draw_texels(rng, fmt, a.shape)
    return 'fresh', ('fresh', b), 0, b


def _code_range(rng, texels, channel=0):
    if rng.random() < 0.25:
        return None
    one = texels[..., channel] if texels.ndim == 4 else texels
    return _quantiles(rng, one)


def _draw_step(c, cur, entry):
    """a step dict of ``entry`` = (op, sub) on volume ``cur`` (without 'out'), and the texels of the volume it makes (None: none)"""
    rng, (op, sub) = c.rng, entry
    a = c.texels[cur]
    fmt = format_of(a)
    M = int(np.iinfo(a.dtype).max) if a.dtype.kind in 'ui' else None
    kw, made, expect, shape, b_source = {}, None, None, a.shape[:3], None
    if op == 'window':
        bits = (8, 16)[int(rng.integers(2))]
        if fmt == 'R32F':
            finite = np.sort(a[np.isfinite(a)].astype(np.float64))
            lo, hi = (sorted(float(finite[int(q * (finite.size - 1))]) for q in rng.random(2)) if finite.size else (0.0, 1.0))
            if not hi > lo:
                hi = lo + 0.5
        else:
            lo, hi = _quantiles(rng, a)
            hi = max(hi, lo + 1)
        kw = {'lo': lo, 'hi': hi, 'format': 'r%d' % bits}
        made = window_texels(a, lo, hi, bits)
    elif op == 'derive_gradient':
        kw = {'operator': ('central', 'sobel')[int(rng.integers(2))], 'gain': (0.5, 1.0, 4.0)[int(rng.integers(3))]}
        made = np.ascontiguousarray(np.stack([a, gradient_magnitude(a, **kw)], axis=-1))
    elif op == 'reduce':
        kw = {'levels': int(rng.integers(1, 3))}
        made = a
        for _ in range(kw['levels']):
            made = reduce_texels(made)
            if max(made.shape[:3]) == 1:
                break
    elif op == 'smooth':
        kw = {'passes': int(rng.integers(1, 4))}
        made = smooth_texels(a, kw['passes'])
    elif op == 'rank':
        kw = {'op': sub, 'passes': int(rng.integers(1, 3))}
        made = rank_texels(a, sub, kw['passes'])
    elif op in ('keep', 'label', 'components_info', 'components_list', 'components_ranks'):
        lo, hi = _field_args(c, a)
        kw = {'lo': lo, 'hi': hi, 'connectivity': (6, 18, 26)[int(rng.integers(3))], 'min_voxels': (1, 1, 2, 5, 40)[int(rng.integers(5))]}
        ranks, listed = components_texels(a, **kw)
        if op == 'keep':
            top = max(len(listed), 1)
            first = int(rng.integers(1, top + 1))
            last = None if rng.random() < 0.4 else int(rng.integers(first, top + 2))
            sel = {'first': first, 'last': last, 'fill': int(rng.integers(0, M + 1)) if rng.random() < 0.5 else 0}
            made = keep_texels(a, ranks, **sel)
            kw.update(sel)
        elif op == 'label':
            made = label_texels(a, ranks)
        elif op == 'components_info':
            foreground = int(np.count_nonzero((a >= lo) & (a <= hi)))
            every = listed if kw['min_voxels'] == 1 else components_texels(a, lo, hi, kw['connectivity'], 1)[1]
            expect = {'listed': len(listed), 'dropped': len(every) - len(listed), 'foreground_voxels': foreground,
                      'listed_voxels': int(sum(v for _, _, _, v in listed))}
        elif op == 'components_list':
            first = int(rng.integers(0, len(listed) + 1))
            n = None if rng.random() < 0.5 else int(rng.integers(0, len(listed) - first + 1))
            kw.update({'first': first, 'n': n})
            expect = listed[first:] if n is None else listed[first:first + n]
        else:
            x, y, z, w, h, d = _box(rng, a.shape[:3])
            kw.update({'box': (x, y, z, w, h, d)})
            expect = np.ascontiguousarray(ranks[z:z + d, y:y + h, x:x + w])
    elif op in ('within', 'channel', 'distance_info', 'distance_squared'):
        lo, hi = _field_args(c, a)
        kw = {'lo': lo, 'hi': hi, 'seeds': ('range', 'rest')[int(rng.integers(2))]}
        d2 = distance_squared_texels(a, **kw)
        finite = d2[d2 != 0xFFFFFFFF]
        largest = int(finite.max()) if finite.size else 0
        if op == 'within':
            r2_lo = int(rng.integers(0, largest + 1)) if rng.random() < 0.6 else 0
            r2_hi = None if rng.random() < 0.3 else int(rng.integers(r2_lo, largest + 2))
            sel = {'r2_lo': r2_lo, 'r2_hi': r2_hi, 'fill': int(rng.integers(0, M + 1)) if rng.random() < 0.5 else 0}
            made = within_texels(a, d2, **sel)
            kw.update(sel)
        elif op == 'channel':
            kw['steps'] = (1, 2, 7, 256)[int(rng.integers(4))]
            made = channel_texels(a, d2, kw['steps'])
        elif op == 'distance_info':
            seeds = int(np.count_nonzero(d2 == 0))
            expect = {'seeds': seeds, 'largest': largest}
        else:
            x, y, z, w, h, d = _box(rng, a.shape[:3])
            kw['box'] = (x, y, z, w, h, d)
            expect = np.ascontiguousarray(d2[z:z + d, y:y + h, x:x + w])
    elif op == 'resample':
        filtered = fmt in RESAMPLE_FILTERED and rng.random() < 0.6
        d0, h0, _ = a.shape[:3]
        fixed = sub if sub is not None else (None, None, None)    # (planned seeds: the target's height and width)
        shape = draw_shape(rng, fixed, lambda s: s[0] * s[1] * s[2] <= MAX_VOXELS and s[2] * h0 * d0 <= MAX_ROW_PASS)
        kw = {'width': shape[2], 'height': shape[1], 'depth': shape[0], 'mode': 'filtered' if filtered else 'nearest'}
        made = resample_texels(a, shape, kw['mode'])
    elif op == 'combine':
        b_source, b, channel, texels_b = _draw_b(c, cur, a, sub)
        kw = {'op': sub, 'b': b, 'channel': channel}
        if sub == 'mask':
            Mb = int(np.iinfo(texels_b.dtype).max)
            lo, hi = _quantiles(rng, texels_b[..., channel] if texels_b.ndim == 4 else texels_b)
            kw.update({'lo': lo, 'hi': min(hi, Mb), 'fill': int(rng.integers(0, M + 1)) if rng.random() < 0.5 else 0})
        elif sub == 'blend':
            wa, wb = ((256, 256), (256, -256), (128, 128), (-256, 0), (512, -256), (77, 151), (4096, -4096), (-3, 5))[int(rng.integers(8))]
            kw.update({'wa': wa, 'wb': wb, 'offset': (0, 0, M, 3, -7, M // 2)[int(rng.integers(6))]})
        made = combine_texels(a, texels_b, sub, **{k: v for k, v in kw.items() if k not in ('op', 'b')})
    elif op == 'upload_block':
        x, y, z, w, h, d = _box(rng, a.shape[:3])
        block = draw_texels(rng, fmt, (d, h, w), style='noise')
        if block.dtype.kind == 'i':                               # the most negative code reaches the storage only through finalize
            block = stored(block)
        kw = {'x': x, 'y': y, 'z': z, 'block': block}
        expect = a.copy()
        expect[z:z + d, y:y + h, x:x + w] = block
    elif op == 'range':
        if fmt == 'R32F':
            kept = a[~np.isnan(a)].astype(np.float64)
            expect = (float(kept.min()), float(kept.max())) if kept.size else None
        else:
            expect = (int(a.min()), int(a.max()))
    elif op == 'histogram':
        top = (a >> 8 if a.dtype == np.uint16 else a).astype(np.int64)
        if a.ndim == 4:
            expect = np.bincount((top[..., 1] * 256 + top[..., 0]).reshape(-1), minlength=65536).astype(np.uint32).reshape(256, 256)
        else:
            expect = np.bincount(top.reshape(-1), minlength=256).astype(np.uint32)
    elif op in ('code_histogram', 'percentile_window'):
        info = np.iinfo(a.dtype)
        bins = np.bincount(a.reshape(-1).astype(np.int64) - int(info.min), minlength=int(info.max) - int(info.min) + 1).astype(np.uint32)
        if op == 'code_histogram':
            expect = bins
        else:
            p_lo, p_hi = sorted(float(np.round(p, 2)) for p in rng.uniform(0, 100, 2))
            kw = {'p_lo': p_lo, 'p_hi': p_hi}
            expect = percentile_window(bins, p_lo, p_hi, signed=info.min < 0)
    elif op == 'compare':
        b_source, b, channel, texels_b = _draw_b(c, cur, a, 'compare')
        kw = {'b': b, 'channel': channel, 'a_range': _code_range(rng, a), 'b_range': _code_range(rng, texels_b, channel)}
        expect = compare_stats(a, texels_b, kw['a_range'], kw['b_range'], channel)
    else:
        raise ValueError(op)
    step = {'op': op, 'sub': sub if op in ('rank', 'combine') else None, 'src': cur, 'out': None, 'kwargs': kw,
            'expect': made if made is not None else expect, 'shape': tuple(shape), 'format': fmt, 'b_source': b_source}
    return step, made


# ---- the later units: geodesic, reconstruct, watershed, measure, thickness, skeleton -------------------------------------------------
def _channel_of(texels, channel):
    return texels[..., channel] if texels.ndim == 4 else texels


def _draw_other(c, cur, formats, kinds=B_SOURCES[:4]):
    """(kind, ('volume', index) | ('fresh', texels), channel, the texels) of a second volume on the grid of volume ``cur`` in one of
    ``formats``: the mask of a reconstruct, the values of a measure, the texels of a watershed.  A two-channel volume of the grid that
    the chain made (a thickness pair, a label or depth channel) is taken half of the times there is one."""
    rng = c.rng
    grid = c.texels[cur].shape[:3]
    kind = kinds[int(rng.integers(len(kinds)))]
    found = [k for k in c.same_grid(cur, formats) if k != cur]
    two = [k for k in c.same_grid(cur, formats) if c.texels[k].ndim == 4]
    if two and 'rg_channel' in kinds and rng.random() < 0.5:
        kind = 'rg_channel'
    if (kind == 'self' and format_of(c.texels[cur]) not in formats) or (kind == 'earlier' and not found):
        kind = 'fresh'
    if kind == 'self' or (kind == 'earlier') or (kind == 'rg_channel' and two):
        pool = [cur] if kind == 'self' else found if kind == 'earlier' else two
        k = pool[int(rng.integers(len(pool)))]
        b = c.texels[k]
        return kind, ('volume', k), (int(rng.integers(2)) if b.ndim == 4 else 0), b
    fmts = [f for f in formats if FORMATS[f][1] == 2] if kind == 'rg_channel' else list(formats)
    b = draw_texels(rng, fmts[int(rng.integers(len(fmts)))], grid)
    return kind, ('fresh', b), (int(rng.integers(2)) if b.ndim == 4 else 0), b


def _draw_selection(rng, listed):
    """the ``ranks`` of a keep_set: a boolean array over the list, or ranks with a duplicate and ranks beyond the list"""
    if rng.random() < 0.35:
        return rng.random(listed) < 0.5
    ranks = [int(r) for r in rng.integers(1, min(listed, 40) + 3, size=int(rng.integers(0, 25)))]
    if ranks:
        ranks += [ranks[0], listed + 1, (1 << 40) + 7]
    return tuple(ranks)


def _object_range(rng, one):
    """(lo, hi) of a structure to thin or to measure: most of the times everything from a quantile up (a solid: several passes, balls
    deeper than a voxel), else everything up to a quantile, else two quantiles"""
    M = int(np.iinfo(one.dtype).max)
    flat = np.sort(one.reshape(-1))
    roll = rng.random()
    if roll < 0.6:
        return max(int(flat[int(rng.uniform(0.2, 0.6) * (flat.size - 1))]), 1), M
    if roll < 0.75:
        return 0, min(int(flat[int(rng.uniform(0.4, 0.8) * (flat.size - 1))]), M - 1)
    return _quantiles(rng, one)


def _tiles_of(shape, tile):
    """int64 [depth][height][width]: the number of the (tx, ty, tz) tile every voxel lies in"""
    d, h, w = shape
    tx, ty, tz = tile
    z, y, x = np.arange(d) // tz, np.arange(h) // ty, np.arange(w) // tx
    return (z[:, None, None] * (int(y[-1]) + 1) + y[None, :, None]) * (int(x[-1]) + 1) + x[None, None, :]


def _rank_facts(ranks, listed):
    """what the conditions ask of a labelling: the number of structures listed, whether one has voxels in two tiles of the labelling
    kernels, the largest number of distinct ranks in one block of the measuring kernel"""
    top = int(ranks.max()) + 1
    inside = ranks > 0
    pairs = np.unique(_tiles_of(ranks.shape, TILES['watershed'])[inside] * top + ranks[inside].astype(np.int64))
    spans = bool(len(pairs) and np.bincount(pairs % top).max() > 1)
    pairs = np.unique(_tiles_of(ranks.shape, TILES['measure'])[inside] * top + ranks[inside].astype(np.int64))
    return {'listed': len(listed), 'spans_tiles': spans, 'block_ranks': int(np.bincount(pairs // top).max()) if len(pairs) else 0}


def _draw_later_step(c, cur, entry):
    """``_draw_step`` for the entries of the later units; the step carries 'facts', what tests/test_volume_chain_cases.py asks of it"""
    rng, (op, sub) = c.rng, entry
    a = c.texels[cur]
    fmt = format_of(a)
    M = int(np.iinfo(a.dtype).max)
    narrow = ('R8', 'RG8') if a.dtype == np.uint8 else ('R16', 'RG16')
    grid = a.shape[:3]
    kw, made, expect, b_source, facts = {}, None, None, None, {}
    fill = lambda: int(rng.integers(0, M + 1)) if rng.random() < 0.5 else 0
    connectivity = lambda: (6, 18, 26)[int(rng.integers(3))]
    if op == 'geodesic':
        channel = int(rng.integers(2)) if a.ndim == 4 else 0
        one = _channel_of(a, channel)
        h = 0
        if sub in TAKES_H:
            spread = int(one.max()) - int(one.min())
            roll = rng.random()
            h = 0 if roll < 0.2 else min(spread + 1 + int(rng.integers(3)), M) if roll < 0.4 else int(rng.integers(1, max(spread, 1) + 1))
        kw = {'op': sub, 'h': h, 'connectivity': connectivity(), 'channel': channel}
        made = geodesic_texels(a, sub, h, kw['connectivity'], channel)
        facts = {'h_above_range': sub in TAKES_H and h > int(one.max()) - int(one.min())}
    elif op == 'reconstruct':
        b_source, b, mask_channel, mask = _draw_other(c, cur, narrow, ('fresh',) * 4 + ('earlier',) * 2 + ('self', 'rg_channel'))
        channel = int(rng.integers(2)) if a.ndim == 4 else 0
        kw = {'b': b, 'op': sub, 'connectivity': connectivity(), 'channel': channel, 'mask_channel': mask_channel}
        made = reconstruct_texels(a, mask, sub, kw['connectivity'], channel, mask_channel)
        marker, under = _channel_of(a, channel), _channel_of(mask, mask_channel)
        facts = {'differs_from_both': bool((made != marker).any() and (made != under).any()),
                 'marker_not_under_mask': bool((marker < under).any() if sub == 'erosion' else (marker > under).any())}
    elif op.startswith('basins_'):
        channel = int(rng.integers(2)) if a.ndim == 4 else 0
        relief = _channel_of(a, channel)
        lo, hi = (0, M) if rng.random() < 0.5 else _quantiles(rng, relief)
        kw = {'lo': lo, 'hi': hi, 'polarity': ('minima', 'maxima')[int(rng.integers(2))], 'connectivity': connectivity(),
              'min_voxels': (1, 1, 2, 5, 40)[int(rng.integers(5))], 'channel': channel, 'texels': None}
        if c.fine and op == 'basins_measure':                     # every face-connected dip of the noise is a basin: hundreds a block
            channel, relief, lo, hi = 0, _channel_of(a, 0), 0, M
            kw.update({'lo': 0, 'hi': M, 'connectivity': 6, 'min_voxels': 1, 'channel': 0})
        emitted = relief
        if rng.random() < 0.35:                                   # what the emitters speak of: another volume of the relief's width
            _, kw['texels'], _, emitted = _draw_other(c, cur, narrow[:1], ('fresh', 'earlier'))
        ranks, listed = watershed_texels(a, lo, hi, kw['polarity'], kw['connectivity'], kw['min_voxels'], channel)
        facts = _rank_facts(ranks, listed)
        made, expect = _draw_selected(c, cur, op[len('basins_'):], kw, emitted, ranks, listed, facts,
                                      lambda: watershed_texels(a, lo, hi, kw['polarity'], kw['connectivity'], 1, channel)[1],
                                      int(np.count_nonzero((relief >= lo) & (relief <= hi))))
        b_source = kw.pop('b_source', None)
    elif op in ('split_keep', 'split_label'):
        lo, hi = _object_range(rng, a)
        kw = {'lo': lo, 'hi': hi, 'h': (0, 1, 2, 5)[int(rng.integers(4))], 'steps': (1, 2, 4)[int(rng.integers(3))], 'connectivity': connectivity(),
              'min_voxels': (1, 1, 2, 5)[int(rng.integers(4))]}
        ranks, listed = split_texels(a, **kw)
        facts = _rank_facts(ranks, listed)
        made, expect = _draw_selected(c, cur, op[len('split_'):], kw, a, ranks, listed, facts, None, None)
    elif op in ('keep_set', 'measure'):
        lo, hi = _field_args(c, a)
        kw = {'lo': lo, 'hi': hi, 'connectivity': connectivity(), 'min_voxels': (1, 1, 2, 5, 40)[int(rng.integers(5))]}
        ranks, listed = components_texels(a, **kw)
        facts = _rank_facts(ranks, listed)
        made, expect = _draw_selected(c, cur, op, kw, a, ranks, listed, facts, None, None)
        b_source = kw.pop('b_source', None)
    elif FAMILY[op] == 'thickness':
        lo, hi = _object_range(rng, a)
        seeds = 'rest' if op == 'open_ball' or rng.random() < 0.7 else 'range'      # open_ball is of the structure
        kw = {'lo': lo, 'hi': hi, 'seeds': seeds}
        d2 = distance_squared_texels(a, lo, hi, seeds)
        t2 = thickness_squared_texels(d2)
        centres = (d2 > 0) & (d2 != 0xFFFFFFFF)
        tiles = _tiles_of(grid, TILES['thickness'])
        facts = {'differs_from_distance': bool((t2 != d2).any()), 'centre_tiles': len(np.unique(tiles[centres])),
                 'largest_in_a_tile': int(d2[centres].max()) if centres.any() else 0}
        largest = int(t2[t2 != 0xFFFFFFFF].max()) if (t2 != 0xFFFFFFFF).any() else 0
        if op == 'thickness':
            kw['steps'] = int(rng.integers(1, 5))
            made = channel_texels(a, t2, kw['steps'])
            assert a.size > 4096 or made.tobytes() == thickness_texels(a, lo, hi, kw['steps'], seeds).tobytes()
        elif op == 'open_ball':
            kw = {'lo': lo, 'hi': hi, 'radius': float(np.round(rng.uniform(0, 1.2 * np.sqrt(largest) + 0.5), 2)), 'fill': fill()}
            made = within_texels(a, t2, check_radius(kw['radius']) + 1, None, kw['fill'])
            assert a.size > 4096 or made.tobytes() == open_ball_texels(a, **kw).tobytes()
        elif op == 'thickness_within':
            r2_lo = int(rng.integers(0, largest + 1)) if rng.random() < 0.6 else 0
            sel = {'r2_lo': r2_lo, 'r2_hi': None if rng.random() < 0.3 else int(rng.integers(r2_lo, largest + 2)), 'fill': fill()}
            made = within_texels(a, t2, **sel)
            kw.update(sel)
        elif op == 'thickness_channel':
            kw['steps'] = (1, 2, 7, 256)[int(rng.integers(4))]
            made = channel_texels(a, t2, kw['steps'])
        elif op == 'thickness_info':
            expect = {'seeds': int(np.count_nonzero(d2 == 0)), 'largest': largest}
        else:
            x, y, z, w, h, d = kw['box'] = _box(rng, grid)
            expect = np.ascontiguousarray(t2[z:z + d, y:y + h, x:x + w])
    elif FAMILY[op] == 'skeleton':
        lo, hi = _object_range(rng, a)
        mode = sub if op == 'centreline' else tuple(SKELETON_MODES)[int(rng.integers(3))]
        passes = 0 if op == 'centreline' or rng.random() < 0.5 else int(rng.integers(1, 5))
        kw = {'lo': lo, 'hi': hi, 'mode': mode}
        burn, info = skeleton_burn_texels(a, lo, hi, mode, passes)
        inside = (a >= lo) & (a <= hi)
        facts = dict(info, mode=mode, both_tiles=bool(grid[2] > 64 and inside[:, :, :64].any() and inside[:, :, 64:].any()))
        if op == 'centreline':
            made = burn_within_texels(a, burn, KEPT, KEPT, 0)
            assert a.size > 4096 or made.tobytes() == skeleton_texels(a, lo, hi, mode).tobytes()
        else:
            kw['passes'] = passes
            if op == 'skeleton_within':
                k_lo = KEPT if rng.random() < 0.3 else int(rng.integers(0, info['passes'] + 2))
                sel = {'k_lo': k_lo, 'k_hi': None if rng.random() < 0.5 else KEPT if k_lo == KEPT else int(rng.integers(k_lo, info['passes'] + 2)), 'fill': fill()}
                made = burn_within_texels(a, burn, **sel)
                kw.update(sel)
            elif op == 'skeleton_info':
                expect = info
            else:
                x, y, z, w, h, d = kw['box'] = _box(rng, grid)
                expect = np.ascontiguousarray(burn[z:z + d, y:y + h, x:x + w])
    else:
        raise ValueError(op)
    step = {'op': op, 'sub': sub, 'src': cur, 'out': None, 'kwargs': kw, 'expect': made if made is not None else expect, 'shape': tuple(grid),
            'format': fmt, 'b_source': b_source, 'facts': facts, 'forced': None}
    return step, made


def _draw_graph_step(c, cur, entry):
    """``_draw_step`` for the entries of the graph rules.  The set is the kept voxels of a skeleton of volume ``cur`` ('via': 'skeleton',
    three times in four) or a value range of it ('range'; a range from a quantile up of what a centreline step made is a thin set too).  A
    prune length is, four times in five, the median cost of the graph's spurs, so that it drops one and keeps one where their costs differ."""
    from vpt_amd import graph as G
    rng, (op, _) = c.rng, entry
    a = c.texels[cur]
    fmt = format_of(a)
    M = int(np.iinfo(a.dtype).max)
    grid = a.shape[:3]
    made, expect, facts = None, None, {}
    lo, hi = _object_range(rng, a)
    mode = tuple(SKELETON_MODES)[int(rng.integers(3))]
    if op == 'centreline_prune':
        if lo == 0 and hi >= M:
            hi = M - 1
        burn, _ = skeleton_burn_texels(a, lo, hi, mode)
        spurs = G.skeleton_graph_texels(burn)['branches']
        spurs = spurs[spurs['kind'] == G.SPUR]
        costs = np.sort(10 * spurs['steps_face'].astype(np.int64) + 14 * spurs['steps_edge'].astype(np.int64) + 17 * spurs['steps_corner'].astype(np.int64))
        prune = int(costs[len(costs) // 2]) if len(costs) and rng.random() < 0.8 else int(rng.integers(0, 60))
        kw = {'lo': lo, 'hi': hi, 'mode': mode, 'prune': prune, 'prune_rounds': (1, 3)[int(rng.integers(2))]}
        made = G.centreline_texels(a, lo, hi, mode, prune, kw['prune_rounds'])
        facts = {'spurs': int(len(costs)), 'differs_from_unpruned': bool((made != burn_within_texels(a, burn, KEPT, KEPT, 0)).any())}
    else:
        via = 'skeleton' if rng.random() < 0.75 else 'range'
        kw = {'via': via, 'lo': lo, 'hi': hi, 'mode': mode}
        g = G.skeleton_graph_texels(skeleton_burn_texels(a, lo, hi, mode)[0]) if via == 'skeleton' else G.graph_texels(a, lo, hi)
        facts = dict(g['info'], via=via)
        fill = int(rng.integers(0, M + 1)) if rng.random() < 0.5 else 0
        if op == 'graph_prune':
            b = g['branches']
            weights = G.DEFAULT_WEIGHTS if rng.random() < 0.6 else tuple(int(w) for w in rng.integers(0, 30, size=3))
            cost = weights[0] * b['steps_face'].astype(np.int64) + weights[1] * b['steps_edge'].astype(np.int64) + weights[2] * b['steps_corner'].astype(np.int64)
            spurs = np.sort(cost[b['kind'] == G.SPUR])
            length = int(spurs[(len(spurs) - 1) // 2]) if len(spurs) and rng.random() < 0.8 else int(rng.integers(0, 80))
            kw.update({'length': length, 'weights': weights, 'debris': bool(rng.random() < 0.4), 'fill': fill})
            made = G.prune_texels(a, g, length, weights, G.PRUNE_DEBRIS if kw['debris'] else 0, fill)
            facts.update(spur_dropped=bool(len(spurs) and spurs[0] <= length), spur_kept=bool(len(spurs) and spurs[-1] > length))
        elif op == 'graph_classes':
            made = G.classes_texels(a, g)
        elif op == 'branches_keep_set':
            kw.update({'ranks': _draw_selection(rng, len(g['branches'])), 'fill': fill})
            made = keep_set_texels(a, g['branch_ranks'], kw['ranks'], fill)
        elif op == 'nodes_label':
            made = label_texels(a, g['node_ranks'])
        elif op == 'graph_info':
            expect = g['info']
        elif op == 'graph_branches':
            n = len(g['branches'])
            first = int(rng.integers(0, n + 1))
            kw.update({'first': first, 'n': None if rng.random() < 0.5 else int(rng.integers(0, n - first + 1))})
            expect = g['branches'][first:] if kw['n'] is None else g['branches'][first:first + kw['n']]
        else:
            assert op == 'graph_nodes', op
            expect = g['nodes']
    step = {'op': op, 'sub': None, 'src': cur, 'out': None, 'kwargs': kw, 'expect': made if made is not None else expect, 'shape': tuple(grid),
            'format': fmt, 'b_source': None, 'facts': facts, 'forced': None}
    return step, made


def _draw_selected(c, cur, tail, kw, emitted, ranks, listed, facts, every, foreground):
    """(the texels made, the scalar expected) of ``tail`` (keep, label, keep_set, info, list, ranks, measure) of a labelling of volume
    ``cur`` whose emitters speak of ``emitted``; fills ``kw`` in"""
    rng = c.rng
    M = int(np.iinfo(emitted.dtype).max)
    fill = int(rng.integers(0, M + 1)) if rng.random() < 0.5 else 0
    if tail == 'keep':
        top = max(len(listed), 1)
        first = int(rng.integers(1, top + 1))
        sel = {'first': first, 'last': None if rng.random() < 0.4 else int(rng.integers(first, top + 2)), 'fill': fill}
        kw.update(sel)
        return keep_texels(emitted, ranks, **sel), None
    if tail == 'label':
        return label_texels(emitted, ranks), None
    if tail == 'keep_set':
        kw.update({'ranks': _draw_selection(rng, len(listed)), 'fill': fill})
        return keep_set_texels(emitted, ranks, kw['ranks'], fill), None
    if tail == 'info':
        dropped = 0 if kw['min_voxels'] == 1 else len(every()) - len(listed)
        return None, {'listed': len(listed), 'dropped': dropped, 'foreground_voxels': foreground, 'listed_voxels': int(sum(v for _, _, _, v in listed))}
    if tail == 'list':
        first = int(rng.integers(0, len(listed) + 1))
        n = None if rng.random() < 0.5 else int(rng.integers(0, len(listed) - first + 1))
        kw.update({'first': first, 'n': n})
        return None, listed[first:] if n is None else listed[first:first + n]
    if tail == 'ranks':
        x, y, z, w, h, d = kw['box'] = _box(rng, ranks.shape)
        return None, np.ascontiguousarray(ranks[z:z + d, y:y + h, x:x + w])
    assert tail == 'measure'
    first = int(rng.integers(0, len(listed) + 1)) if rng.random() < 0.5 else 0
    n = None if rng.random() < 0.5 else int(rng.integers(0, len(listed) - first + 1))
    if c.fine:                                                    # every rank of a block meets in the block's table
        first, n = 0, None
    values, kw['b'], kw['values_channel'] = emitted, None, 0
    if rng.random() < 0.7:
        kw['b_source'], kw['b'], kw['values_channel'], other = _draw_other(c, cur, _UNORM)
        values = _channel_of(other, kw['values_channel'])
        facts['values_of_a_derived_pair'] = bool(kw['b'][0] == 'volume' and kw['b'][1] > 0 and other.ndim == 4 and kw['values_channel'] == 1)
    kw.update({'first': first, 'n': n})
    return None, measure_texels(ranks, values, first, n)


def _constant(texels):
    flat = texels.reshape(-1)
    if flat.dtype.kind == 'f':
        flat = flat.view(np.uint32)
    return flat.size > 1 and not (flat != flat[0]).any()


def _legal(entry, fmt, texels):
    op = entry[0]
    if fmt not in LEGAL[op]:
        return False
    if op == 'range' and fmt == 'R32F' and np.isnan(texels).all():
        return False
    if FAMILY.get(op) in SLOW_FAMILIES and op in LATER and int(np.prod(texels.shape[:3])) > SLOW_VOXELS:
        return False
    if op in GRAPH and int(np.prod(texels.shape[:3])) > SLOW_VOXELS:
        return False
    return True


def _build_old(seed):
    c = _Chain(seed)
    rng = c.rng
    tiny = seed % 16 == 0
    rank = seed - seed // 16 - 1                                  # the seed's number among those that are not one voxel
    plan = PLANS[rank] if not tiny and rank < PLANNED else None
    free = rank - PLANNED
    if plan is not None:
        fmt = _U1[rank % 2]
    elif tiny:
        fmt = ('R8', 'R16_SNORM', 'R32F', 'RG16')[(seed // 16) % 4]
    else:
        fmt = (tuple(FORMATS) + _U1)[free % 10]
    if tiny:
        shape = (1, 1, 1)
    elif plan is not None and plan[0] is not None:
        shape = plan[0]
    elif plan is not None:                                        # a planned target: its row pass must fit whatever the source is
        shape = draw_shape(rng, fits=lambda s: s[0] * s[1] * s[2] <= MAX_VOXELS and plan[2][2] * s[1] * s[0] <= MAX_ROW_PASS)
    else:
        shape = draw_shape(rng)
    specials = FORMATS[fmt][0] == np.float32 and (free // 10) % 2 == 0
    source = draw_texels(rng, fmt, shape, specials=specials)
    cur = c.add_volume(stored(source))
    c.steps.append({'op': 'source', 'sub': None, 'src': None, 'out': 0, 'kwargs': {'format': fmt, 'texels': source}, 'expect': c.texels[0],
                    'shape': tuple(shape), 'format': fmt, 'b_source': None})
    begin = list(plan[1]) if plan is not None else []
    target = plan[2] if plan is not None else None
    wishes = [OLD_ENTRIES[(3 * seed + j) % len(OLD_ENTRIES)] for j in range(3)]
    count = max(int(rng.integers(3, 7)), min(len(begin), 4))
    for k in range(count):
        if begin and not _legal(begin[0], format_of(c.texels[cur]), c.texels[cur]):
            cur = c.one_channel_before(cur)
        texels = c.texels[cur]
        fmt = format_of(texels)
        for attempt in range(REDRAWS + 1):
            if begin and attempt == 0:
                entry = begin.pop(0)
            else:
                roll = rng.random()
                pool = [('upload_block', None)] if roll < 0.25 and 0 < k < count - 1 and c.steps[-1]['op'] != 'upload_block' else \
                    OLD_SCALAR_ENTRIES if roll < 0.50 else OLD_VOLUME_ENTRIES
                wished = [e for e in wishes if e not in c.used and _legal(e, fmt, texels)]
                legal = [e for e in pool if _legal(e, fmt, texels)]
                fresh = [e for e in legal if e not in c.used]
                if wished and attempt == 0 and rng.random() < 0.8:
                    entry = wished[0]
                elif fresh or legal:
                    entry = (fresh or legal)[int(rng.integers(len(fresh or legal)))]
                else:                                             # e.g. RG32F: no scalar takes it
                    legal = [e for e in OLD_VOLUME_ENTRIES if _legal(e, fmt, texels)]
                    entry = legal[int(rng.integers(len(legal)))]
            if entry[0] == 'resample' and target is not None:
                step, made = _draw_step(c, cur, ('resample', target))
                step['sub'] = None
            else:
                step, made = _draw_step(c, cur, entry)
            if made is None or texels.size == 1 or made.size == 1 or not _constant(made) or attempt == REDRAWS:
                break
        if entry[0] == 'resample':
            target = None
        c.used.add(entry)
        if made is not None:
            step['out'] = c.add_volume(made)
            cur = step['out']
        elif step['op'] == 'upload_block':
            c.texels[cur] = step['expect']
        c.steps.append(step)
        # after a two-channel result the chain goes on with it where an operation takes it, else with the last one-channel volume
        if c.texels[cur].ndim == 4 and c.one_channel_before(cur) is not None and rng.random() < 0.5:
            cur = c.one_channel_before(cur)
    return c.steps


def _reads_derived(step):
    return step['src'] > 0 or any(step['kwargs'].get(key) is not None and step['kwargs'][key][0] == 'volume' and step['kwargs'][key][1] > 0
                                  for key in ('b', 'texels'))


def _draw_later_chain(seed, attempt, graph=False):
    """a chain of the later rules; ``graph``: of the graph rules (module docstring).  Every draw the graph rules add stands behind
    ``if graph``, so the streams of seeds 128 .. 223 are what they were"""
    c = _Chain(seed)
    rng = c.rng = np.random.default_rng([CONSTANT + seed, attempt])
    n = seed - (GRAPH_SEEDS if graph else LATER_SEEDS)
    tiny = seed % 16 == 0
    rank = n - n // 16 - 1
    plans = GRAPH_PLANS if graph else LATER_PLANS
    plan = plans[rank] if not tiny and rank < len(plans) else None
    free = rank - len(plans)
    c.fine = plan is not None and plan[2] == 'noise' and ('basins_measure', None) in plan[1]
    if tiny:
        fmt, shape, style = _UNORM[(seed // 16) % 4], (1, 1, 1), None
    elif plan is not None:
        fmt, shape, style = _U1[rank % 2], plan[0], plan[2]
    elif graph:
        fmt = _U1[free % 2]
        shape = draw_shape(rng, fits=lambda s: 200 <= s[0] * s[1] * s[2] <= GRAPH_VOXELS)
        style = ('blobs', 'sphere', 'blobs', 'sparse')[int(rng.integers(4))]
    else:
        fmt = ('R8', 'RG8', 'R16', 'RG16', 'RG8', 'R16', 'RG16', 'R8')[free % 8]
        shape = draw_shape(rng, fits=lambda s: s[0] * s[1] * s[2] <= (2 if free % 3 == 2 else 1) * SLOW_VOXELS)
        style = ('noise', 'sphere', 'sparse', 'blobs')[int(rng.integers(4))]
    source = draw_texels(rng, fmt, shape, style=style)
    cur = c.add_volume(source)
    c.steps.append({'op': 'source', 'sub': None, 'src': None, 'out': 0, 'kwargs': {'format': fmt, 'texels': source}, 'expect': c.texels[0],
                    'shape': tuple(shape), 'format': fmt, 'b_source': None})
    begin = list(plan[1]) if plan is not None else []
    wished_of = GRAPH_ENTRIES if graph else LATER_ENTRIES
    wishes = [wished_of[(3 * n + j) % len(wished_of)] for j in range(3)]
    count = max(int(rng.integers(3, 7)), len(begin))
    forced = seed % 4 == 3
    for k in range(count):
        if begin and not _legal(begin[0], format_of(c.texels[cur]), c.texels[cur]):
            cur = c.one_channel_before(cur)
        texels = c.texels[cur]
        fmt = format_of(texels)
        planned = begin.pop(0) if begin else None
        for redraw in range(REDRAWS + 1):
            if planned is not None:                              # a planned entry is drawn again as itself: its family is to see this shape
                entry = planned
            else:
                roll, later = rng.random(), rng.random() < 0.75
                pool = [('upload_block', None)] if roll < 0.2 and 0 < k < count - 1 and c.steps[-1]['op'] != 'upload_block' else \
                    (LATER_SCALAR_ENTRIES if later else OLD_SCALAR_ENTRIES) if roll < 0.45 and k > 0 else \
                    (LATER_VOLUME_ENTRIES if later else OLD_VOLUME_ENTRIES)
                if graph and pool[0][0] != 'upload_block' and rng.random() < 0.6:
                    pool = GRAPH_SCALAR_ENTRIES if roll < 0.45 and k > 0 else GRAPH_VOLUME_ENTRIES
                wished = [e for e in wishes if e not in c.used and _legal(e, fmt, texels)]
                legal = [e for e in pool if _legal(e, fmt, texels)] or [e for e in LATER_VOLUME_ENTRIES if _legal(e, fmt, texels)]
                fresh = [e for e in legal if e not in c.used]
                if wished and redraw == 0 and rng.random() < 0.8:
                    entry = wished[0]
                else:
                    entry = (fresh or legal)[int(rng.integers(len(fresh or legal)))]
            step, made = (_draw_graph_step if entry[0] in GRAPH else _draw_later_step if entry[0] in LATER else _draw_step)(c, cur, entry)
            if made is None or texels.size == 1 or made.size == 1 or not _constant(made) or redraw == REDRAWS:
                break
        if forced and FAMILY.get(entry[0]) in FORCED and entry[0] in LATER and entry[0] not in UNHOOKED:
            hooks = FORCED[FAMILY[entry[0]]]
            step['forced'] = hooks[(seed // 4 + k) % len(hooks)]
        c.used.add(entry)
        if made is not None:
            step['out'] = c.add_volume(made)
            cur = step['out']
        elif step['op'] == 'upload_block':
            c.texels[cur] = step['expect']
        c.steps.append(step)
        if c.texels[cur].ndim == 4 and c.one_channel_before(cur) is not None and rng.random() < 0.5:
            cur = c.one_channel_before(cur)
    return c.steps


def _build_later(seed):
    """a chain of the later rules: at least two steps of the later units, one of which reads a volume that a derive step made; a draw
    that misses this is drawn again from the next stream of the seed"""
    for attempt in range(64):
        steps = _draw_later_chain(seed, attempt)
        later = [s for s in steps[1:] if s['op'] in LATER]
        if len(later) >= 2 and any(_reads_derived(s) for s in later):
            return steps
    raise AssertionError('seed %d: no chain of the later rules' % seed)


def _build_graph(seed):
    """a chain of the graph rules: at least two steps of the graph family, one of which reads a volume that a derive step made"""
    for attempt in range(64):
        steps = _draw_later_chain(seed, attempt, graph=True)
        mine = [s for s in steps[1:] if s['op'] in GRAPH]
        if len(mine) >= 2 and any(_reads_derived(s) for s in mine):
            return steps
    raise AssertionError('seed %d: no chain of the graph rules' % seed)


def _build(seed):
    return _build_old(seed) if seed < LATER_SEEDS else _build_later(seed) if seed < GRAPH_SEEDS else _build_graph(seed)


@functools.lru_cache(maxsize=None)
def chain(seed):
    """the steps of case ``seed`` (module docstring); computed once, shared and never changed"""
    steps = _build(int(seed))
    for step in steps:
        for value in [step['expect']] + list(step['kwargs'].values()):
            if isinstance(value, np.ndarray):
                value.setflags(write=False)
    return steps


def default_seeds():
    return range(*DEFAULT_SEEDS)


# ---- a chain as text -------------------------------------------------------------------------------------------------------------
def _text(value):
    if isinstance(value, np.ndarray):
        return '<%s %s>' % (value.dtype, 'x'.join(str(n) for n in value.shape))
    if isinstance(value, tuple) and len(value) == 2 and value[0] == 'fresh':
        return "('fresh', %s)" % _text(value[1])
    return repr(value)


def _later_text(op, kw, other, emitted):
    """the call of a step of the later units on its source, as text"""
    g = lambda *keys: ', '.join(_text(kw[k]) for k in keys)
    tails = {'keep': lambda: 'keep(%s)' % g('first', 'last', 'fill'), 'label': lambda: 'label()', 'keep_set': lambda: 'keep_set(%s)' % g('ranks', 'fill'),
             'info': lambda: 'info', 'list': lambda: 'list(%s)' % g('first', 'n'), 'ranks': lambda: 'ranks(*%r)' % (kw['box'],),
             'measure': lambda: 'measure(%s, %s, %d)' % (g('first', 'n'), other, kw['values_channel'])}
    if op == 'geodesic':
        return 'geodesic(%s)' % g('op', 'h', 'connectivity', 'channel')
    if op == 'reconstruct':
        return 'reconstruct(%s, %s)' % (other, g('op', 'connectivity', 'channel', 'mask_channel'))
    if op.startswith('basins_'):
        return 'watershed(%s, texels=%s).%s' % (g('lo', 'hi', 'polarity', 'connectivity', 'min_voxels', 'channel'), emitted, tails[op[7:]]())
    if op.startswith('split_'):
        return 'split(%s).%s' % (g('lo', 'hi', 'h', 'steps', 'connectivity', 'min_voxels'), tails[op[6:]]())
    if op in ('keep_set', 'measure'):
        return 'components(%s).%s' % (g('lo', 'hi', 'connectivity', 'min_voxels'), tails[op]())
    if op == 'thickness':
        return 'thickness(%s)' % g('lo', 'hi', 'steps', 'seeds')
    if op == 'open_ball':
        return 'open_ball(%s)' % g('lo', 'hi', 'radius', 'fill')
    if op.startswith('thickness_'):
        tail = {'within': lambda: 'within(%s)' % g('r2_lo', 'r2_hi', 'fill'), 'channel': lambda: 'channel(%s)' % g('steps'), 'info': lambda: 'info',
                'squared': lambda: 'squared(*%r)' % (kw['box'],)}[op[10:]]()
        return 'distance(%s).thickness().%s' % (g('lo', 'hi', 'seeds'), tail)
    if op == 'centreline':
        return 'centreline(%s)' % g('lo', 'hi', 'mode')
    tail = {'within': lambda: 'within(%s)' % g('k_lo', 'k_hi', 'fill'), 'info': lambda: 'info', 'burn': lambda: 'burn(*%r)' % (kw['box'],)}[op[9:]]()
    return 'skeleton(%s).%s' % (g('lo', 'hi', 'mode', 'passes'), tail)


def _graph_text(op, kw):
    """the call of a step of the graph rules on its source, as text"""
    if op == 'centreline_prune':
        return 'centreline(%d, %d, %r, prune=%d, prune_rounds=%d)' % (kw['lo'], kw['hi'], kw['mode'], kw['prune'], kw['prune_rounds'])
    made = 'skeleton(%d, %d, %r).graph()' % (kw['lo'], kw['hi'], kw['mode']) if kw['via'] == 'skeleton' else 'graph(%d, %d)' % (kw['lo'], kw['hi'])
    tail = {'graph_prune': lambda: 'prune(%r, %r, %r, %r)' % (kw['length'], kw['weights'], kw['debris'], kw['fill']), 'graph_classes': lambda: 'classes()',
            'branches_keep_set': lambda: 'branches.keep_set(%s, %r)    # the graph destroyed first' % (_text(kw['ranks']), kw['fill']),
            'nodes_label': lambda: 'nodes.label()    # the graph destroyed first', 'graph_info': lambda: 'info',
            'graph_branches': lambda: 'branch_records(%r, %r)' % (kw['first'], kw['n']), 'graph_nodes': lambda: 'node_records()'}[op]()
    return '%s.%s' % (made, tail)


def describe(seed):
    """the chain as lines for a Python session: ``steps = chain(seed)`` gives the arrays the lines name by step and keyword"""
    steps = chain(seed)
    lines = ['# volume chain seed %d: from volume_chain_cases import chain; steps = chain(%d); K = lambda i: steps[i]["kwargs"]' % (seed, seed)]
    for i, s in enumerate(steps):
        kw, src = s['kwargs'], 'v%s' % s['src']
        args = ', '.join('%s=%s' % (k, _text(v)) for k, v in kw.items() if k not in ('b', 'block', 'texels', 'box'))
        other, emitted = (None if kw.get(key) is None or s['op'] == 'source' else 'v%d' % kw[key][1] if kw[key][0] == 'volume' else
                          'upload(K(%d)["%s"][1])' % (i, key) for key in ('b', 'texels'))
        d, h, w = s['shape']
        if s['op'] == 'source':
            dtype, channels = FORMATS[kw['format']]
            flag = ', snorm=True' if dtype == np.int8 else ', norm16=True' if dtype in (np.uint16, np.int16) else ''
            call = 'v0 = Volume.from_array(ctx, K(0)["texels"]%s)    # %s, %d x %d x %d (w, h, d)' % (flag, kw['format'], w, h, d)
        elif s['op'] in ('keep', 'label', 'components_info', 'components_list', 'components_ranks'):
            made = '%s.components(%d, %d, %d, %d)' % (src, kw['lo'], kw['hi'], kw['connectivity'], kw['min_voxels'])
            tail = {'keep': 'keep(%r, %r, %r)' % (kw.get('first'), kw.get('last'), kw.get('fill')), 'label': 'label()', 'components_info': 'info',
                    'components_list': 'list(%r, %r)' % (kw.get('first'), kw.get('n')), 'components_ranks': 'ranks(*%r)' % (kw.get('box'),)}[s['op']]
            call = '%s.%s' % (made, tail)
        elif s['op'] in ('within', 'channel', 'distance_info', 'distance_squared'):
            made = '%s.distance(%d, %d, %r)' % (src, kw['lo'], kw['hi'], kw['seeds'])
            tail = {'within': 'within(%r, %r, %r)' % (kw.get('r2_lo'), kw.get('r2_hi'), kw.get('fill')), 'channel': 'channel(%r)' % kw.get('steps'),
                    'distance_info': 'info', 'distance_squared': 'squared(*%r)' % (kw.get('box'),)}[s['op']]
            call = '%s.%s' % (made, tail)
        elif s['op'] in GRAPH:
            call = '%s.%s' % (src, _graph_text(s['op'], kw))
        elif s['op'] in LATER:
            call = '%s.%s' % (src, _later_text(s['op'], kw, other, emitted))
            if s.get('forced') is not None:
                call += '    # and forced: %s' % {'skeleton': '_flags=%r', 'thickness': 'thickness_timed(_flags=%r)', 'reconstruct': 'reconstruct_timed(_tile_rounds=%r)',
                                                   'watershed': '_caps=%r'}[FAMILY[s['op']]] % (s['forced'],)
        elif s['op'] == 'combine':
            rest = ', '.join('%s=%r' % (k, v) for k, v in kw.items() if k not in ('b', 'op'))
            call = '%s.combine(%s, %r, %s)' % (src, other, kw['op'], rest)
        elif s['op'] == 'compare':
            call = '%s.compare(%s, %r, %r, %d)' % (src, other, kw['a_range'], kw['b_range'], kw['channel'])
        elif s['op'] == 'upload_block':
            call = '%s.upload_block(%d, %d, %d, K(%d)["block"])    # a %s box' % (src, kw['x'], kw['y'], kw['z'], i, 'x'.join(str(n) for n in kw['block'].shape[:3][::-1]))
        elif s['op'] == 'rank':
            call = '%s.rank(%r, %d)' % (src, kw['op'], kw['passes'])
        elif s['op'] == 'window':
            call = '%s.window(%r, %r, %r)' % (src, kw['lo'], kw['hi'], kw['format'])
        else:
            call = '%s.%s(%s)' % (src, s['op'], args)
        if s['out'] is not None and s['op'] != 'source':
            call = 'v%d = %s' % (s['out'], call)
        lines.append('%-100s # step %d%s' % (call, i, '' if s['op'] == 'source' else ', on %d x %d x %d %s' % (w, h, d, s['format'])))
    return '\n'.join(lines)
