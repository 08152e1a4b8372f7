"""GPU: fixed-seed chains of volume operations (tests/volume_chain_cases.py) replayed through the public Volume, Components and Distance
methods; every volume a step makes is read back whole and must equal, byte for byte, what the numpy statements give for the same chain,
every scalar must be equal exactly.  tests/test_volume_chain_cases.py holds the drawn cases to the conditions that keep this test from
passing vacuously.

Even seeds destroy every volume once no later step reads it, before the result that was made from it is read back; odd seeds keep all
of them and read two earlier results again at the end.  Every case reads one random sub-box; every second case renders its last volume
and a volume uploaded from the expected texels with MIP and MCM, NEAREST and LINEAR, and the buffers must be bit-identical (a thickness
pair or a label volume through the 2-D transfer function).

Seeds 0 .. 127 are the chains of the first units, unchanged; seeds 128 .. 223 are drawn by the later rules of volume_chain_cases and put
geodesic operations, reconstructions, watersheds, splits, rank sets, measurements, thickness and thinning behind each other and behind the
first units.  Their field handles (basins, components, distances, thickness, skeleton) are made, used once and destroyed like the others.
A step that carries 'forced' runs twice, plainly and through the unit's test hook (skeleton _flags, thickness_timed _flags,
reconstruct_timed _tile_rounds, watershed _caps): the forced result must be the statement's and, byte for byte, the plain call's.
The slowest of the new seeds measured on an MI355X is seed 148 at 0.65 s (the 96 together: 6 s), most of it the statements on the CPU.

Seeds 224 .. 255 are drawn by the graph rules: centrelines with pruning rounds, the graph of a range or of a skeleton behind other steps,
its pruning, its class pair (which later two-channel steps and the 2-D transfer function take), its records, and its branches and nodes as
Components used after the graph has been destroyed.

VPT_VOLFUZZ_SEEDS=a:b widens the sweep."""
import os

import numpy as np
import pytest

import vpt_amd
from vpt_amd.distance import check_radius
from vpt_amd.scene import Transform, Node
from vpt_amd.synthetic import colour_tf, GoldenRatioRng

from conftest import orbit_camera
import volume_chain_cases as V
from test_gpu_volume_formats import BUFFERS, CLASSES

pytestmark = pytest.mark.gpu

_SEEDS = range(*[int(v) for v in os.environ.get("VPT_VOLFUZZ_SEEDS", "%d:%d" % V.DEFAULT_SEEDS).split(":")])


def upload(ctx, texels, filt='linear'):
    if texels.dtype == np.int8:
        return vpt_amd.Volume.from_array(ctx, texels, filt, snorm=True)
    return vpt_amd.Volume.from_array(ctx, texels, filt, norm16=texels.dtype in (np.uint16, np.int16))


def whole(vol):
    m = vol.modality['dimensions']
    return vol.read_block(0, 0, 0, m['width'], m['height'], m['depth'])


def bits(a):
    """the array as unsigned integers of its width, so that NaN texels compare by their bits ..."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def same_texels(got, want, what):
    """byte for byte; a NaN the statement computes (reduce of float texels) is any NaN"""
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s, expected %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    differ = bits(got) != bits(want)
    if want.dtype.kind == 'f':
        differ &= ~(np.isnan(got) & np.isnan(want))
    if differ.any():
        first = np.argwhere(differ)[0]
        z, y, x = (int(v) for v in first[:3])
        raise AssertionError("%s: %d bytes differ, first at (x, y, z) = (%d, %d, %d)%s: got %r, want %r" % (
            what, int(differ.sum()) * got.dtype.itemsize, x, y, z, ' channel %d' % first[3] if len(first) == 4 else '',
            got[tuple(first)], want[tuple(first)]))


def same_scalar(got, want, what):
    if isinstance(want, np.ndarray) and want.dtype.names:         # the records of a measure: every field of every record
        got = np.asarray(got)
        assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s, expected %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
        wrong = [(k, name, got[name][k], want[name][k]) for name in want.dtype.names for k in np.flatnonzero(got[name] != want[name])[:1]]
        assert not wrong, "%s: (record, field, got, want) %r" % (what, wrong[:6])
    elif isinstance(want, np.ndarray):
        got = np.asarray(got)
        assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64)), \
            "%s: %d values differ" % (what, int((got.astype(np.int64) != want.astype(np.int64)).sum()) if got.shape == want.shape else -1)
    elif isinstance(want, dict) and 'dice' in want:               # compare: the eight integers exactly, the ratios as the same doubles
        for key in want:
            assert got[key] == want[key] and type(got[key]) is type(want[key]), "%s: %s is %r, expected %r" % (what, key, got[key], want[key])
        assert set(got) == set(want), what
    else:
        assert got == want, "%s: %r, expected %r" % (what, got, want)


def render(ctx, vol, kind, filt, tf):
    w, h = 48, 40
    vol.setFilter(filt)
    r = CLASSES[kind](ctx, vol, orbit_camera(w / h), None, {'resolution': (w, h), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
    try:
        r.setTransferFunction(tf)
        if kind == 'mcm':
            r.extinction = 40
        r.reset()
        r.render()
        return [np.ascontiguousarray(r.read(b)) for b in BUFFERS.get(kind, [vpt_amd._native.BUFFER_RENDER, vpt_amd._native.BUFFER_FRAME,
                                                                            vpt_amd._native.BUFFER_ACCUM])] + [np.ascontiguousarray(r.getTexture())]
    finally:
        r.destroy()


class Replay:
    """the device side of one chain: volume k of the chain at vols[k] (None once destroyed), want[k] its expected texels as they are now"""

    def __init__(self, ctx, seed):
        self.ctx, self.seed, self.steps = ctx, seed, V.chain(seed)
        self.vols, self.want, self.extra = [], [], []
        self.destroys = seed % 2 == 0
        self.last_use = {}
        for i, s in enumerate(self.steps):
            others = [s['kwargs'].get(key) for key in ('b', 'texels')] if i else []
            for k in [s['src']] + [other[1] for other in others if other is not None and other[0] == 'volume']:
                if k is not None:
                    self.last_use[k] = i

    def what(self, i):
        return "%s\nstep %d (%s)" % (V.describe(self.seed), i, self.steps[i]['op'])

    def close(self):
        for vol in self.vols + self.extra:
            if vol is not None:
                vol.destroy()
        self.vols, self.extra = [], []

    def second(self, kw, key='b'):
        """(the Volume B of a combine / compare, the mask, values or texels of a later unit's step; whether this step made it)"""
        kind, value = kw[key]
        if kind == 'volume':
            return self.vols[value], False
        vol = upload(self.ctx, value)
        self.extra.append(vol)
        return vol, True

    def field(self, src, s):
        kw = s['kwargs']
        if V.FAMILY[s['op']] == 'components':
            return src.components(kw['lo'], kw['hi'], kw['connectivity'], kw['min_voxels'])
        return src.distance(kw['lo'], kw['hi'], kw['seeds'])

    @staticmethod
    def selected(f, tail, kw, values):
        """``tail`` of a Components object: (the new Volume or None, the scalar or None)"""
        if tail == 'keep':
            return f.keep(kw['first'], kw['last'], kw['fill']), None
        if tail == 'label':
            return f.label(), None
        if tail == 'keep_set':
            return f.keep_set(kw['ranks'], kw['fill']), None
        if tail == 'info':
            return None, f.info
        if tail == 'list':
            return None, f.list(kw['first'], kw['n'])
        if tail == 'ranks':
            return None, f.ranks(*kw['box'])
        return None, f.measure(kw['first'], kw['n'], values, kw['values_channel'])

    def later_once(self, s, hook, others):
        """a step of the later units, plainly (``hook`` None) or through the hook that forces the unit's slow path; every field handle
        is made, used once and destroyed"""
        op, kw, src = s['op'], s['kwargs'], self.vols[s['src']]
        family = V.FAMILY[op]
        if op == 'geodesic':
            return src.geodesic(kw['op'], kw['h'], kw['connectivity'], kw['channel']), None
        if op == 'reconstruct':
            args = (others['b'], kw['op'], kw['connectivity'], kw['channel'], kw['mask_channel'])
            return (src.reconstruct(*args) if hook is None else src.reconstruct_timed(*args, _tile_rounds=hook)[0]), None
        if op.startswith('basins_') or op.startswith('split_') or op in ('keep_set', 'measure'):
            if op.startswith('basins_'):
                f = src.watershed(kw['lo'], kw['hi'], kw['polarity'], kw['connectivity'], kw['min_voxels'], kw['channel'], texels=others.get('texels'), _caps=hook)
            elif op.startswith('split_'):
                f = src.split(kw['lo'], kw['hi'], kw['h'], kw['steps'], kw['connectivity'], kw['min_voxels'])
            else:
                f = src.components(kw['lo'], kw['hi'], kw['connectivity'], kw['min_voxels'])
            try:
                return self.selected(f, op.split('_', 1)[1] if op not in ('keep_set', 'measure') else op, kw, others.get('b'))
            finally:
                f.destroy()
        if family == 'thickness':
            if hook is None and op == 'thickness':
                return src.thickness(kw['lo'], kw['hi'], kw['steps'], kw['seeds']), None
            if hook is None and op == 'open_ball':
                return src.open_ball(kw['lo'], kw['hi'], kw['radius'], kw['fill']), None
            d = src.distance(kw['lo'], kw['hi'], kw.get('seeds', 'rest'))
            try:
                t = d.thickness() if hook is None else d.thickness_timed(_flags=hook)[0]
            finally:
                d.destroy()
            try:
                if op in ('thickness', 'thickness_channel'):
                    return t.channel(kw['steps']), None
                if op == 'open_ball':
                    return t.within(check_radius(kw['radius']) + 1, None, kw['fill']), None
                if op == 'thickness_within':
                    return t.within(kw['r2_lo'], kw['r2_hi'], kw['fill']), None
                return None, (t.info if op == 'thickness_info' else t.squared(*kw['box']))
            finally:
                t.destroy()
        assert family == 'skeleton', op
        if hook is None and op == 'centreline':
            return src.centreline(kw['lo'], kw['hi'], kw['mode']), None
        k = src.skeleton(kw['lo'], kw['hi'], kw['mode'], kw.get('passes', 0), _flags=hook)
        try:
            if op == 'centreline':
                return k.volume(), None
            if op == 'skeleton_within':
                return k.within(kw['k_lo'], kw['k_hi'], kw['fill']), None
            return None, (k.info if op == 'skeleton_info' else k.burn(*kw['box']))
        finally:
            k.destroy()

    def graph_step(self, s):
        """a step of the graph rules: the graph of a value range or of a skeleton (which is destroyed before the graph is used), used once
        and destroyed; the handed-out components are used after the graph is gone"""
        op, kw, src = s['op'], s['kwargs'], self.vols[s['src']]
        if op == 'centreline_prune':
            return src.centreline(kw['lo'], kw['hi'], kw['mode'], prune=kw['prune'], prune_rounds=kw['prune_rounds']), None
        if kw['via'] == 'skeleton':
            k = src.skeleton(kw['lo'], kw['hi'], kw['mode'])
            try:
                g = k.graph()
            finally:
                k.destroy()
        else:
            g = src.graph(kw['lo'], kw['hi'])
        handed = None
        try:
            if op == 'graph_prune':
                return g.prune(kw['length'], kw['weights'], kw['debris'], kw['fill']), None
            if op == 'graph_classes':
                return g.classes(), None
            if op == 'graph_info':
                return None, g.info
            if op == 'graph_branches':
                return None, g.branch_records(kw['first'], kw['n'])
            if op == 'graph_nodes':
                return None, g.node_records()
            handed = g.branches if op == 'branches_keep_set' else g.nodes
            g.destroy()
            return (handed.keep_set(kw['ranks'], kw['fill']) if op == 'branches_keep_set' else handed.label()), None
        finally:
            if handed is not None:
                handed.destroy()
            g.destroy()

    def later(self, i):
        """step i of the later units; where the case forces the slow path, again through the hook: the same bytes, the same scalar"""
        s = self.steps[i]
        others, mine = {}, []
        try:
            for key in ('b', 'texels'):
                if s['kwargs'].get(key) is not None:
                    others[key], made_here = self.second(s['kwargs'], key)
                    if made_here:
                        mine.append(others[key])
            made, scalar = self.later_once(s, None, others)
            if s['forced'] is not None:
                try:
                    again, scalar_again = self.later_once(s, s['forced'], others)
                    what = "%s, forced through %r" % (self.what(i), s['forced'])
                    if again is not None:
                        try:
                            same_texels(whole(again), s['expect'], what)
                            assert whole(again).tobytes() == whole(made).tobytes(), what
                        finally:
                            again.destroy()
                    else:
                        same_scalar(scalar_again, s['expect'], what)
                except BaseException:
                    if made is not None:
                        made.destroy()
                    raise
            return made, scalar
        finally:
            for vol in mine:
                self.extra.remove(vol)
                vol.destroy()

    def call(self, i):
        """run step i: (the new Volume or None, the scalar result or None)"""
        s = self.steps[i]
        op, kw, src = s['op'], s['kwargs'], self.vols[s['src']]
        if op == 'window':
            return src.window(kw['lo'], kw['hi'], kw['format']), None
        if op == 'derive_gradient':
            return src.derive_gradient(kw['operator'], kw['gain']), None
        if op == 'reduce':
            return src.reduce(kw['levels']), None
        if op == 'smooth':
            return src.smooth(kw['passes']), None
        if op == 'rank':
            return src.rank(kw['op'], kw['passes']), None
        if op == 'resample':
            return src.resample(kw['width'], kw['height'], kw['depth'], kw['mode']), None
        if op in V.GRAPH:
            return self.graph_step(s)
        if op in V.LATER:
            return self.later(i)
        if op in V.FAMILY and op != 'resample':                   # components and distances: made, used once, destroyed
            f = self.field(src, s)
            try:
                if op == 'keep':
                    return f.keep(kw['first'], kw['last'], kw['fill']), None
                if op == 'label':
                    return f.label(), None
                if op == 'within':
                    return f.within(kw['r2_lo'], kw['r2_hi'], kw['fill']), None
                if op == 'channel':
                    return f.channel(kw['steps']), None
                if op in ('components_info', 'distance_info'):
                    return None, f.info
                if op == 'components_list':
                    return None, f.list(kw['first'], kw['n'])
                return None, (f.ranks if op == 'components_ranks' else f.squared)(*kw['box'])
            finally:
                f.destroy()
        if op in ('combine', 'compare'):
            other, mine = self.second(kw)
            try:
                if op == 'combine':
                    params = {k: v for k, v in kw.items() if k not in ('op', 'b', 'channel')}
                    return src.combine(other, kw['op'], kw['channel'], **params), None
                return None, src.compare(other, kw['a_range'], kw['b_range'], kw['channel'])
            finally:
                if mine:
                    self.extra.remove(other)
                    other.destroy()
        if op == 'upload_block':
            src.upload_block(kw['x'], kw['y'], kw['z'], kw['block'])
            return None, None
        if op == 'range':
            return None, src.range()
        if op == 'histogram':
            return None, src.histogram()
        if op == 'code_histogram':
            return None, src.code_histogram()
        if op == 'percentile_window':
            return None, src.percentile_window(kw['p_lo'], kw['p_hi'])
        raise ValueError(op)

    def run(self):
        steps = self.steps
        source = steps[0]['kwargs']['texels']
        self.vols.append(upload(self.ctx, source))
        self.want.append(steps[0]['expect'])
        same_texels(whole(self.vols[0]), self.want[0], self.what(0))
        for i in range(1, len(steps)):
            s = steps[i]
            made, scalar = self.call(i)
            if made is not None:
                self.vols.append(made)
                self.want.append(s['expect'])
                assert len(self.vols) - 1 == s['out']
            if made is None and s['op'] == 'upload_block':
                self.want[s['src']] = s['expect']
                same_texels(whole(self.vols[s['src']]), s['expect'], self.what(i))
            elif made is None:
                same_scalar(scalar, s['expect'], self.what(i))
            if self.destroys:                                     # the sources go before the result is read
                for k, vol in enumerate(self.vols):
                    if vol is not None and k != len(self.vols) - 1 and self.last_use.get(k, 0) <= i:
                        vol.destroy()
                        self.vols[k] = None
            if made is not None:
                same_texels(whole(made), s['expect'], self.what(i))
        rng = np.random.default_rng(V.CONSTANT + 7919 * (self.seed + 1))
        alive = [k for k, vol in enumerate(self.vols) if vol is not None]
        if not self.destroys:                                     # later steps and upload_block on a source left earlier results alone
            for k in alive[:-1][-2:]:
                same_texels(whole(self.vols[k]), self.want[k], "%s\nvolume %d, read again at the end" % (V.describe(self.seed), k))
        last = alive[-1]
        x, y, z, w, h, d = V._box(rng, self.want[last].shape[:3])
        same_texels(self.vols[last].read_block(x, y, z, w, h, d), np.ascontiguousarray(self.want[last][z:z + d, y:y + h, x:x + w]),
                    "%s\nbox %r of volume %d" % (V.describe(self.seed), (x, y, z, w, h, d), last))
        if self.seed % 4 in (1, 2):                               # every second case, destroying and keeping ones alike
            twin = upload(self.ctx, self.want[last])
            self.extra.append(twin)
            tf = colour_tf(64, 16) if self.want[last].ndim == 4 else colour_tf(256)
            for kind in ('mip', 'mcm'):
                for filt in ('nearest', 'linear'):
                    a, b = render(self.ctx, self.vols[last], kind, filt, tf), render(self.ctx, twin, kind, filt, tf)
                    for n, (x, y) in enumerate(zip(a, b)):
                        assert x.shape == y.shape and x.tobytes() == y.tobytes(), \
                            "%s\n%s %s: buffer %d of the derived volume %d differs from the uploaded twin's" % (V.describe(self.seed), kind, filt, n, last)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("seed", _SEEDS)
def test_volume_chain_equals_its_numpy_statements(gpu_ctx, seed):
    replay = Replay(gpu_ctx, seed)
    try:
        replay.run()
    finally:
        replay.close()
