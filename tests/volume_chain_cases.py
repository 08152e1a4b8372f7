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
  b_source for combine / compare: where B comes from (B_SOURCES)

How a case is drawn.  Every sixteenth seed is one voxel.  The next PLANNED seeds take their shape from PLANS, which walks each kernel
family's tile extents (1, one below the tile, the tile, one above, two tiles plus one on every axis), and begin with that family's
operations: independent draws from the pools would need thousands of seeds to put 257 on the x axis of a volume that then happens to
be smoothed.  Every other seed draws each axis from the three pools (1 .. 9; 1 .. 80; EDGES) and its format by turns from FORMATS.
Steps: 3 .. 6; a step is upload_block with probability 0.25 (never first, last or twice in a row), a scalar with 0.25, a volume-producing operation otherwise, uniform among
the entries legal for the current format, the entries the chain has not used yet first; each seed also has three wishes, taken by turns
from the whole entry list, that go first where they are legal.  48 seeds did not reach every entry three times; the default 128 do.  A volume-producing step whose
expected texels are constant is drawn again, up to 8 times (constancy cascades: every later step would see a constant volume)."""
import functools

import numpy as np

import vpt_amd
from vpt_amd.combine import combine_texels, compare_stats
from vpt_amd.components import components_texels, keep_texels, label_texels
from vpt_amd.distance import distance_squared_texels, within_texels, channel_texels
from vpt_amd.gradient import gradient_magnitude
from vpt_amd.pyramid import reduce_texels, smooth_texels
from vpt_amd.rank import rank_texels, OPERATORS as RANK_OPERATORS
from vpt_amd.resample import resample_texels
from vpt_amd.window import window_texels, percentile_window

CONSTANT = 20261019
DEFAULT_SEEDS = (0, 128)
MAX_VOXELS = 100000
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
RESAMPLE_FILTERED = _UNORM
COMBINE_OPS = ('mask', 'min', 'max', 'absdiff', 'blend', 'pair')
SCALAR_OPS = ('range', 'histogram', 'code_histogram', 'percentile_window', 'compare', 'components_info', 'components_list',
              'components_ranks', 'distance_info', 'distance_squared')
B_SOURCES = ('fresh', 'earlier', 'self', 'rg_channel', 'other_width')


def _entries(ops):
    out = []
    for op in ops:
        subs = RANK_OPERATORS if op == 'rank' else COMBINE_OPS if op == 'combine' else (None,)
        out += [(op, sub) for sub in subs]
    return out


VOLUME_ENTRIES = _entries(op for op in LEGAL if op not in SCALAR_OPS and op != 'upload_block')
SCALAR_ENTRIES = _entries(SCALAR_OPS)
ENTRIES = VOLUME_ENTRIES + SCALAR_ENTRIES + [('upload_block', None)]

# kernel family -> the extents (x, y, z) of its tile; None: the kernel has no tile along that axis
TILES = {
    'gradient': (128, 8, 32),                          # GR_TX, GR_TY, GR_TZ (vpt_volume_ops.hip)
    'smooth': (128, 8, 32),                            # SM_TX, SM_TY, SM_TZ (vpt_volume_pyramid.hip)
    'rank': (128, 8, 32),                              # RK_TX, RK_TY, RK_TZ (vpt_volume_rank.hip)
    'components': (64, 8, 4),                          # CC_TX, CC_TY, CC_TZ (vpt_volume_components.hip)
    'distance': (64, None, None),                      # the 64-voxel row segments of k_edt_x (vpt_volume_distance.hip); y and z are marched whole
    'resample': (64, 4, None),                         # k_resample_yz: 64 columns x 4 rows of the TARGET grid a workgroup, one plane each
}
FAMILY = {'derive_gradient': 'gradient', 'smooth': 'smooth', 'rank': 'rank', 'keep': 'components', 'label': 'components',
          'components_info': 'components', 'components_list': 'components', 'components_ranks': 'components', 'within': 'distance',
          'channel': 'distance', 'distance_info': 'distance', 'distance_squared': 'distance', 'resample': 'resample'}
# the kernels with a vector form and a texel-by-texel form, chosen by the row length: nx % 4 (gradient, smooth, rank: ALIGNED), the row's
# bytes % 32 (k_reduce); window and combine go by 16-byte groups of the whole volume
VECTOR_FAMILIES = ('gradient', 'smooth', 'rank')


def tile_extents(tile):
    """the extents an axis with this tile must be seen at"""
    return (1,) if tile is None else (1, tile - 1, tile, tile + 1, 2 * tile + 1)


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
    return True


def _build(seed):
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
    wishes = [ENTRIES[(3 * seed + j) % len(ENTRIES)] for j in range(3)]
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
                    SCALAR_ENTRIES if roll < 0.50 else VOLUME_ENTRIES
                wished = [e for e in wishes if e not in c.used and _legal(e, fmt, texels)]
                legal = [e for e in pool if _legal(e, fmt, texels)]
                fresh = [e for e in legal if e not in c.used]
                if wished and attempt == 0 and rng.random() < 0.8:
                    entry = wished[0]
                elif fresh or legal:
                    entry = (fresh or legal)[int(rng.integers(len(fresh or legal)))]
                else:                                             # e.g. RG32F: no scalar takes it
                    legal = [e for e in VOLUME_ENTRIES if _legal(e, fmt, texels)]
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


def describe(seed):
    """the chain as lines for a Python session: ``steps = chain(seed)`` gives the arrays the lines name by step and keyword"""
    steps = chain(seed)
    lines = ['# volume chain seed %d: from volume_chain_cases import chain; steps = chain(%d); K = lambda i: steps[i]["kwargs"]' % (seed, seed)]
    for i, s in enumerate(steps):
        kw, src = s['kwargs'], 'v%s' % s['src']
        args = ', '.join('%s=%s' % (k, _text(v)) for k, v in kw.items() if k not in ('b', 'block', 'texels', 'box'))
        if 'b' in kw:
            other = 'v%d' % kw['b'][1] if kw['b'][0] == 'volume' else 'upload(K(%d)["b"][1])' % i
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
