"""CPU: the numpy statement of the graph contract (vpt_amd.graph; include/vpt.h "skeleton graph"), held to known answers on the thinning
test's shapes and to the identities the contract promises, not to another implementation: a branch is one voxel, a simple path or a simple
cycle (asserted here, voxel by voxel, not assumed); free_ends + attachments is 0 or 2; the steps of a path, a cycle and an isolated voxel;
the nodes' degrees add up to the branches' attachments; the order of the visits changes nothing; pruning without the debris flag keeps
the count of 26-components.  The device and the JS statement are held to this statement byte for byte (tests/test_gpu_graph.py, the JS
twin below)."""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import vpt_amd
from vpt_amd import graph as G
from vpt_amd.components import components_texels, neighbour_offsets
from vpt_amd.skeleton import KEPT, skeleton_burn_texels

import graph_cases as GC
from test_skeleton_host import HI, LO, SHAPES, texels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANDOM_SHAPES = ((6, 10, 70), (9, 11, 12))
DENSITIES = (0.06, 0.10, 0.14)
SEEDS = (1, 2, 3, 4)


def random_set(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


RANDOM = {'random %dx%dx%d %.2f %d' % (shape + (density, seed)): functools.partial(random_set, shape, density, seed)
          for shape in RANDOM_SHAPES for density in DENSITIES for seed in SEEDS}


@functools.lru_cache(maxsize=None)
def kept_set(name):
    """the set of a case: the 'ends' skeleton of a shape's codes 100 .. 255, or a random set as it is"""
    if name in RANDOM:
        kept = RANDOM[name]()
    else:
        kept = skeleton_burn_texels(texels(SHAPES[name]()), LO, HI, 'ends')[0] == KEPT
    kept.setflags(write=False)
    return kept


CASES = list(SHAPES) + list(RANDOM)


@functools.lru_cache(maxsize=None)
def statement(name):
    """the graph of a case: computed once, shared, never written to"""
    g = G.graph_of(kept_set(name))
    for key in ('classes', 'branch_ranks', 'node_ranks', 'branches', 'nodes'):
        g[key].setflags(write=False)
    return g


def parts(mask):
    return len(components_texels(mask.astype(np.uint8), 1, 1, 26)[1])


def rows(records, *fields):
    return [tuple(int(r[f]) for f in fields) for r in records]


# ---- known answers ----------------------------------------------------------------------------------------------------------------
def test_a_line_is_one_segment():
    g = statement('line')
    assert g['info']['branches'] == 1 and g['info']['nodes'] == 0 and g['info']['segments'] == 1
    assert rows(g['branches'], 'voxels', 'free_ends', 'attachments', 'kind', 'steps_face', 'steps_edge', 'steps_corner') == [(14, 2, 0, G.SEGMENT, 13, 0, 0)]
    b = g['branches'][0]
    assert (int(b['tip_lo']), int(b['tip_hi'])) == ((7 * 20 + 11) * 20 + 3, (7 * 20 + 11) * 20 + 16) and (int(b['node_lo']), int(b['node_hi'])) == (0, 0)
    assert G.lengths(g['branches'], 0.5).tolist() == [6.5]


def test_a_wye_is_a_node_and_three_spurs():
    g = statement('wye')
    assert rows(g['nodes'], 'voxels', 'degree') == [(1, 3)]
    assert g['info']['branches'] == 3 and g['info']['spurs'] == 3
    assert all(r == (G.SPUR, 1, 1, 1, 1) for r in rows(g['branches'], 'kind', 'free_ends', 'attachments', 'node_lo', 'node_hi'))


def test_a_torus_is_three_links_and_three_one_voxel_spurs():
    g = statement('torus')
    assert g['info']['branches'] == 6 and rows(g['nodes'], 'voxels', 'degree') == [(1, 3)] * 3
    assert rows(g['branches'], 'kind', 'voxels', 'steps_face', 'steps_edge', 'steps_corner') == [
        (G.LINK, 16, 6, 11, 0), (G.LINK, 7, 6, 2, 0), (G.LINK, 7, 6, 2, 0), (G.SPUR, 1, 0, 1, 0), (G.SPUR, 1, 0, 1, 0), (G.SPUR, 1, 0, 1, 0)]
    assert sorted(rows(g['branches'][:3], 'node_lo', 'node_hi')) == [(1, 2), (1, 3), (2, 3)]      # the ring passes every node


def test_a_pruned_torus_thinned_again_is_one_cycle():
    a = texels(SHAPES['torus']())
    out = G.centreline_texels(a, LO, HI, 'ends', prune=20)
    g = G.graph_texels(out, LO, HI)
    assert g['info']['nodes'] == 0 and g['info']['kept_voxels'] == 33
    assert rows(g['branches'], 'kind', 'voxels', 'steps_face', 'steps_edge', 'steps_corner', 'free_ends', 'attachments') == [(G.CYCLE, 33, 18, 15, 0, 0, 0)]
    b = g['branches'][0]
    root = int(np.flatnonzero(g['classes'].reshape(-1))[0])
    assert int(b['tip_lo']) == int(b['tip_hi']) == root
    # without prune the convenience is the skeleton, and a second round finds nothing to drop
    assert np.array_equal(G.centreline_texels(a, LO, HI, 'ends'), vpt_amd.skeleton_texels(a, LO, HI, 'ends'))
    assert np.array_equal(G.centreline_texels(a, LO, HI, 'ends', prune=20, prune_rounds=3), out)


def test_a_hollow_ball_is_one_node():
    kept = skeleton_burn_texels(texels(SHAPES['hollow ball']()), LO, HI, 'kernel')[0] == KEPT     # the closed surface of tests/test_skeleton_host.py
    g = G.graph_of(kept)
    assert g['info']['branches'] == 0 and rows(g['nodes'], 'voxels', 'degree') == [(300, 0)] and g['info']['node_voxels'] == 300
    g = statement('hollow ball')                                  # in 'ends' too
    assert g['info']['branches'] == 0 and rows(g['nodes'], 'voxels', 'degree') == [(300, 0)]


# ---- identities -------------------------------------------------------------------------------------------------------------------
def test_the_random_sets_hold_every_kind():
    for seed in SEEDS:
        info = statement('random 6x10x70 0.10 %d' % seed)['info']
        assert all(info[k] > 0 for k in ('isolated', 'segments', 'spurs', 'links', 'loops', 'cycles')), (seed, info)


@pytest.mark.parametrize("name", CASES)
def test_the_identities_hold(name):
    kept = kept_set(name)
    g = statement(name)
    classes, branch_ranks, node_ranks, branches, nodes, info = (g[k] for k in ('classes', 'branch_ranks', 'node_ranks', 'branches', 'nodes', 'info'))
    d, h, w = kept.shape
    assert branches.dtype == G.BRANCH_DTYPE and nodes.dtype == G.NODE_DTYPE and tuple(info) == G.INFO_FIELDS
    assert np.array_equal(classes != 0, kept) and info['kept_voxels'] == int(kept.sum()) and info['node_voxels'] == int((classes == 4).sum())
    assert np.array_equal(branch_ranks != 0, (classes >= 1) & (classes <= 3)) and np.array_equal(node_ranks != 0, classes == 4)
    assert info['branches'] == len(branches) == int(branch_ranks.max()) and info['nodes'] == len(nodes) == int(node_ranks.max())
    # a branch voxel has at most two neighbours in the set, so at most two in its branch: one voxel, a simple path or a simple cycle
    padded = np.pad(branch_ranks, 1)
    own = np.zeros(kept.shape, np.int64)
    for c, b, a in neighbour_offsets(26):
        own += (padded[1 + c:1 + c + d, 1 + b:1 + b + h, 1 + a:1 + a + w] == branch_ranks) & (branch_ranks != 0)
    assert int(own.max(initial=0)) <= 2
    flat = np.arange(kept.size).reshape(kept.shape)
    for k, b in enumerate(branches):
        inside = branch_ranks == k + 1
        voxels, tips = int(inside.sum()), int((inside & (own < 2)).sum())
        assert voxels == int(b['voxels']) and tips in (0, 1, 2), k
        steps = int(b['steps_face']) + int(b['steps_edge']) + int(b['steps_corner'])
        free_ends, attachments, kind = int(b['free_ends']), int(b['attachments']), int(b['kind'])
        assert free_ends + attachments in (0, 2), k
        assert free_ends == int((inside & (classes == 2)).sum()), k
        if tips == 0:                                             # a cycle: every voxel has two neighbours in it
            assert voxels >= 3 and kind == G.CYCLE and steps == voxels and int(own[inside].sum()) == 2 * voxels, k
            assert int(b['tip_lo']) == int(b['tip_hi']) == int(flat[inside].min()), k
        elif voxels == 1:
            assert tips == 1 and int(b['tip_lo']) == int(b['tip_hi']) == int(flat[inside][0]), k
            assert steps == attachments and kind in ((G.ISOLATED,) if attachments == 0 else (G.SPUR, G.LINK, G.LOOP)), k
        else:                                                     # a path: two tips, every other voxel with two neighbours in it
            assert tips == 2 and int(own[inside].sum()) == 2 * (voxels - 1), k
            assert steps == voxels - 1 + attachments and kind not in (G.ISOLATED, G.CYCLE), k
            assert (int(b['tip_lo']), int(b['tip_hi'])) == (int(flat[inside & (own < 2)].min()), int(flat[inside & (own < 2)].max())), k
        assert kind == G.kind_of(voxels, free_ends, attachments, int(b['node_lo']), int(b['node_hi'])), k
        if kind == G.ISOLATED:
            assert (voxels, free_ends, attachments, steps) == (1, 0, 0, 0), k
        if kind == G.SPUR and voxels == 1:
            assert steps == 1, k                                  # a one-voxel spur has exactly one step: its attachment
        assert (attachments == 0) == (int(b['node_lo']) == 0) and 0 <= int(b['node_lo']) <= int(b['node_hi']) <= len(nodes), k
        assert (kind in (G.LINK, G.LOOP)) == (attachments == 2) and (kind == G.LOOP) <= (int(b['node_lo']) == int(b['node_hi'])), k
    assert int(nodes['degree'].sum()) == int(branches['attachments'].sum()) == info['attachments']
    assert [int(v) for v in nodes['voxels']] == [int((node_ranks == k + 1).sum()) for k in range(len(nodes))]
    assert sum(info[k] for k in ('isolated', 'segments', 'spurs', 'links', 'loops', 'cycles')) == info['branches']
    assert all(info[k] == int(branches[k].sum()) for k in ('steps_face', 'steps_edge', 'steps_corner'))
    # canonical order
    assert all(int(branches['voxels'][k]) >= int(branches['voxels'][k + 1]) for k in range(len(branches) - 1))


@pytest.mark.parametrize("name", CASES)
def test_the_order_of_the_visits_changes_nothing(name):
    g, other = statement(name), G.graph_of(kept_set(name), order='reversed')
    assert other['info'] == g['info']
    for key in ('classes', 'branch_ranks', 'node_ranks', 'branches', 'nodes'):
        assert other[key].tobytes() == g[key].tobytes(), key


# ---- pruning ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_pruning_keeps_the_components_and_drops_what_it_says(name):
    kept, g = kept_set(name), statement(name)
    a = texels(kept)
    before = parts(kept)
    for length in (0, 14, 20, 45, 1 << 40):
        out = G.prune_texels(a, g, length, fill=3)
        stays = out != 3
        assert np.array_equal(out[stays], a[stays]) and not (stays & ~kept).any()
        assert (stays & (g['classes'] == 4)).sum() == g['info']['node_voxels']          # node voxels always stay
        assert parts(stays) == before, length
        gone = G.dropped(g['branches'], length)
        assert np.array_equal(kept & ~stays, np.concatenate([[False], gone])[g['branch_ranks']])
        assert all(int(b['kind']) == G.SPUR for b in g['branches'][gone])
    # every spur has a step (a one-voxel spur exactly one), so a length of 0 drops nothing
    assert all(int(b['steps_face']) + int(b['steps_edge']) + int(b['steps_corner']) >= 1 for b in g['branches'] if int(b['kind']) == G.SPUR)
    assert np.array_equal(G.prune_texels(a, g, 0) != 0, kept)
    # debris: segments and isolated voxels go too
    out = G.prune_texels(a, g, 1 << 40, flags=G.PRUNE_DEBRIS, fill=3)
    kinds = np.concatenate([[-1], g['branches']['kind'].astype(np.int64)])[g['branch_ranks']]
    assert np.array_equal(out == 3, ~kept | np.isin(kinds, (G.SPUR, G.SEGMENT, G.ISOLATED)))
    # weights: a length in faces alone
    gone = G.dropped(g['branches'], 2, (1, 0, 0))
    assert [bool(x) for x in gone] == [int(b['kind']) == G.SPUR and int(b['steps_face']) <= 2 for b in g['branches']]


def test_a_wye_within_the_length_is_reduced_to_its_node():
    kept, g = kept_set('wye'), statement('wye')
    out = G.prune_texels(texels(kept), g, 1000)
    assert int((out != 0).sum()) == 1 and np.array_equal(out != 0, g['classes'] == 4)


def test_classes_texels_and_lengths():
    kept, g = kept_set('torus'), statement('torus')
    for dtype in (np.uint8, np.uint16):
        a = texels(kept, dtype)
        pair = G.classes_texels(a, g)
        assert pair.dtype == a.dtype and pair.shape == a.shape + (2,) and np.array_equal(pair[..., 0], a) and np.array_equal(pair[..., 1], g['classes'])
    b = g['branches']
    want = b['steps_face'] + np.sqrt(2.0) * b['steps_edge'] + np.sqrt(3.0) * b['steps_corner']
    assert np.array_equal(G.lengths(b), want) and np.array_equal(G.lengths(b, 0.25), want * 0.25)
    assert vpt_amd.graph_texels is G.graph_texels and vpt_amd.prune_texels is G.prune_texels and vpt_amd.classes_texels is G.classes_texels


def test_the_two_inputs_give_one_graph():
    a = texels(SHAPES['wye']())
    burn, _ = skeleton_burn_texels(a, LO, HI, 'ends')
    one, two = G.skeleton_graph_texels(burn), G.graph_texels(vpt_amd.skeleton_texels(a, LO, HI, 'ends'), LO, HI)
    assert one['info'] == two['info'] and one['branches'].tobytes() == two['branches'].tobytes() and one['nodes'].tobytes() == two['nodes'].tobytes()


# ---- arguments, the empty set -------------------------------------------------------------------------------------------------------
def test_the_argument_checks():
    a = texels(random_set((3, 4, 5), 0.3, 9))
    g = G.graph_texels(a, LO, HI)
    for call in (lambda: G.graph_texels(a, 3, 2), lambda: G.graph_texels(a, 0, 256), lambda: G.graph_texels(a, -1, 2), lambda: G.graph_texels(a, 1.5, 2),
                 lambda: G.graph_texels(a, True, 2), lambda: G.graph_texels(a.astype(np.float32), 1, 2), lambda: G.graph_texels(a[0], 1, 2),
                 lambda: G.graph_texels(np.zeros((0, 2, 2), np.uint8), 1, 2), lambda: G.graph_texels(np.zeros((1, 1, 4097), np.uint8), 1, 2),
                 lambda: G.graph_texels(a, 1, 2, order='random'), lambda: G.graph_of(a), lambda: G.skeleton_graph_texels(a.astype(np.float32)),
                 lambda: G.prune_texels(a, g, -1), lambda: G.prune_texels(a, g, 1.0), lambda: G.prune_texels(a, g, 1 << 64), lambda: G.prune_texels(a, g, 1, (1, 2)),
                 lambda: G.prune_texels(a, g, 1, (1, 2, 65536)), lambda: G.prune_texels(a, g, 1, (1, 2, -1)), lambda: G.prune_texels(a, g, 1, 5),
                 lambda: G.prune_texels(a, g, 1, flags=2), lambda: G.prune_texels(a, g, 1, fill=256), lambda: G.prune_texels(a, g, 1, fill=-1),
                 lambda: G.prune_texels(a[:2], g, 1), lambda: G.classes_texels(a[:2], g),
                 lambda: G.centreline_texels(a, 0, 255, 'ends', prune=5), lambda: G.centreline_texels(a, 1, 255, 'ends', prune=5, prune_rounds=0),
                 lambda: G.centreline_texels(a, 1, 255, 'ends', prune=-1), lambda: G.centreline_texels(a, 1, 255, 'ends', prune=2.5)):
        with pytest.raises(ValueError):
            call()
    assert G.check_centreline_prune(0, 254, 5, 1, 255) == (5, 1, 255) and G.check_centreline_prune(1, 255, 5, 2, 255) == (5, 2, 0)
    assert G.check_centreline_prune(0, 255, 5, 1, 65535) == (5, 1, 256)


def test_the_empty_set_and_a_single_voxel():
    a = texels(random_set((3, 4, 5), 0.3, 9))
    g = G.graph_texels(a, 99, 99)
    assert g['info'] == dict.fromkeys(G.INFO_FIELDS, 0) and len(g['branches']) == 0 and len(g['nodes']) == 0 and not g['classes'].any()
    assert np.array_equal(G.prune_texels(a, g, 5, fill=9), np.full(a.shape, 9, np.uint8))
    g = G.graph_texels(np.full((1, 1, 1), 7, np.uint8), 7, 7)
    assert rows(g['branches'], 'voxels', 'kind', 'tip_lo', 'tip_hi') == [(1, G.ISOLATED, 0, 0)] and g['info']['isolated'] == 1


# ---- content made of pieces (tests/graph_cases.py) ---------------------------------------------------------------------------------
def equals_whole(assembled, kept):
    """the assembled statement is graph_of of the whole set: info, every record, every rank, byte for byte"""
    want, got = G.graph_of(kept), assembled.statement()
    assert got['info'] == want['info']
    for key in ('classes', 'branch_ranks', 'node_ranks', 'branches', 'nodes'):
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and got[key].tobytes() == want[key].tobytes(), key
    return want


def motif(seed):
    return GC.padded(random_set((6, 10, 70), 0.10, seed))


def test_a_tiling_of_one_motif_assembles_to_the_statement_on_the_whole():
    shape = (16, 24, 144)                                         # 2 x 2 x 2 periods of [8][12][72]
    pieces = GC.tiling(shape, motif(1))
    assert len(pieces) == 8 and len({id(m) for _, m in pieces}) == 1
    want = equals_whole(GC.graph_on_pieces(shape, pieces), GC.set_of(shape, pieces))
    one = statement('random 6x10x70 0.10 1')['info']
    assert want['info'] == {k: 8 * v for k, v in one.items()} and one['nodes'] > 0 and one['cycles'] > 0
    # equal voxel counts in different pieces: ranked by the root's index in the volume, which no piece's own order knows
    assert len(set(want['branches']['voxels'].tolist())) < len(want['branches']) // 8


def test_a_tiling_of_two_motifs_and_an_odd_volume_assemble_to_the_statement_on_the_whole():
    shape = (17, 27, 149)                                         # the periods do not fill it
    a, b = motif(2), motif(3)
    pieces = [(o, b if i in (1, 2, 4, 7) else a) for i, (o, _) in enumerate(GC.tiling(shape, a))]
    assert len(pieces) == 8
    want = equals_whole(GC.graph_on_pieces(shape, pieces), GC.set_of(shape, pieces))
    # pieces of different content tie in voxel count, and a node of one piece and a node of another trade places in the order
    ranks = [GC.graph_on_pieces(shape, pieces).node_table[k][1:] for k in range(8)]
    assert all(len(r) > 0 for r in ranks) and any(int(ranks[k].min()) < int(ranks[0].max()) for k in range(1, 8))
    assert int(want['branches']['tip_hi'].max()) > 8 * 12 * 72 and int(want['branches']['node_hi'].max()) == want['info']['nodes']


def test_the_dust_tiling_needs_only_the_upper_faces():
    shape = (16, 32, 128)
    pieces = GC.tiling(shape, GC.dust_motif())
    want = equals_whole(GC.graph_on_pieces(shape, pieces, low_faces=False), GC.set_of(shape, pieces))
    assert want['info']['branches'] == 8 * 980 and want['info']['isolated'] == 8 * 896 and want['info']['segments'] == 8 * 84 and want['info']['nodes'] == 0
    with pytest.raises(AssertionError, match='first plane'):
        GC.graph_on_pieces(shape, pieces)
    with pytest.raises(AssertionError, match='overlap'):
        GC.graph_on_pieces(shape, pieces + [((4, 8, 32), pieces[0][1])], low_faces=False)
    with pytest.raises(AssertionError, match='last plane'):
        GC.graph_on_pieces(shape, [((0, 0, 0), np.ones((2, 2, 2), bool))])


@pytest.mark.parametrize("name", ['torus', 'random 6x10x70 0.10 1', 'random 9x11x12 0.14 2'])
def test_the_vectorised_pruning_is_the_statements(name):
    kept, g = kept_set(name), statement(name)
    a = texels(kept)
    for length, weights, flags in ((0, (10, 14, 17), 0), (20, (10, 14, 17), 0), (45, (10, 14, 17), 1), (2, (1, 0, 65535), 0), ((1 << 64) - 1, (65535,) * 3, 1)):
        assert np.array_equal(GC.dropped(g['branches'], length, weights, flags), G.dropped(g['branches'], length, weights, flags))
        assert np.array_equal(GC.prune_texels(a, g['classes'], g['branch_ranks'], g['branches'], length, weights, flags, 3), G.prune_texels(a, g, length, weights, flags, 3))
    big = np.zeros(2, G.BRANCH_DTYPE)                             # a cost that wraps modulo 2^64, as the device's does
    big['kind'], big['steps_face'] = G.SPUR, (1 << 63, 5)
    assert GC.dropped(big, 9, (2, 0, 0)).tolist() == G.dropped(big, 9, (2, 0, 0)).tolist() == [True, False]


def test_the_wave_case_holds_the_runs_it_is_for():
    g = G.graph_of(GC.wave_case())
    waves = GC.wave_runs(g)
    assert sum(lanes for runs in waves for _, _, lanes in runs) == g['info']['kept_voxels'] == 416
    met = GC.wave_conditions(waves)
    assert met['full'] == [1, 2] and met['carried'] == [0] and waves[0][-1] == (1, 37, 27) and met['last lane'] == [3]
    assert 4 in met['over nodes'] and 6 in met['apart']
    assert int(g['branches'][0]['voxels']) == 200 and int(g['branches'][1]['kind']) == G.LOOP and g['info']['isolated'] == 63


# ---- the JS statement -------------------------------------------------------------------------------------------------------------
JS_CASES = ['torus', 'wye', 'line', 'hollow ball'] + ['random 6x10x70 0.10 %d' % s for s in SEEDS] + ['random 9x11x12 0.14 1', 'random 9x11x12 0.06 2']


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
@pytest.mark.parametrize("dtype", (np.uint8, np.uint16), ids=lambda d: np.dtype(d).name)
def test_the_js_twin_equals_the_statement(tmp_path, dtype):
    M = int(np.iinfo(dtype).max)
    lo, hi = LO * (M // 255), M
    args = []
    for k, name in enumerate(JS_CASES):
        kept = kept_set(name)
        a = texels(kept, dtype)
        path = tmp_path / ("texels%d.raw" % k)
        path.write_bytes(a.astype(a.dtype.newbyteorder('<')).tobytes())
        args += [str(path), str(kept.shape[2]), str(kept.shape[1]), str(kept.shape[0])]
    res = subprocess.run(["node", os.path.join(ROOT, "js", "test", "test_graph_host.js"), str(np.dtype(dtype).itemsize * 8), str(lo), str(hi)] + args,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = res.stdout.decode().strip().splitlines()
    assert lines[-1] == 'js graph host ok'
    got = json.loads(lines[-2])
    assert len(got) == len(JS_CASES)
    for name, js in zip(JS_CASES, got):
        kept, g = kept_set(name), statement(name)
        a = texels(kept, dtype)
        assert js['info'] == g['info'], name
        assert js['classes'] == g['classes'].reshape(-1).tolist() and js['branch_ranks'] == g['branch_ranks'].reshape(-1).tolist(), name
        assert js['node_ranks'] == g['node_ranks'].reshape(-1).tolist(), name
        fields = list(G.BRANCH_DTYPE.names)
        assert js['branches'] == [[int(b[f]) for f in fields] for b in g['branches']], name
        assert js['nodes'] == [[int(n['voxels']), int(n['degree'])] for n in g['nodes']], name
        assert js['prune'] == G.prune_texels(a, g, 20, fill=3).reshape(-1).tolist(), name
        assert js['debris'] == G.prune_texels(a, g, 30, (10, 14, 17), G.PRUNE_DEBRIS, 1).reshape(-1).tolist(), name
        assert js['pair'] == G.classes_texels(a, g).reshape(-1).tolist(), name
        assert js['lengths'] == G.lengths(g['branches'], 0.5).tolist(), name
