"""GPU: the graph of a voxel set (vpt_volume_graph, vpt_skeleton_graph) on the device.

Info, every branch and node record, the branch and node ranks, the class pair volume and the pruned volumes are held, byte for byte, to
vpt_amd.graph, the numpy statement of the contract (tests/test_graph_host.py holds that to known answers and to the contract's identities).
No tolerance appears anywhere.

A labelling workgroup owns a tile of 64 x 8 x 4 voxels, a word of the bit plane holds 32 voxels along x.  The random sets of the host test
in [6][10][70] are the smallest that cross a tile and a word along every axis with a width that is no multiple of 32; the hand-built
diagonal line and the Y sit on the corner where eight tiles meet, (63, 7, 3) -> (64, 8, 4)."""
import ctypes as C
import functools

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd import graph as G
from vpt_amd.measure import keep_set_texels, measure_texels
from vpt_amd.skeleton import KEPT, skeleton_burn_texels, skeleton_texels

import graph_cases as GC
from test_gpu_pyramid import upload, whole
from test_graph_host import RANDOM
from test_skeleton_host import HI, LO, SHAPES
from test_skeleton_host import texels as host_texels

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.uint16)
CORNER = (6, 10, 70)                                              # [depth][height][width]


def diagonal():
    """a line along the space diagonal through (63, 7, 3) -> (64, 8, 4): every step crosses the word and, once, the tile along all axes"""
    mask = np.zeros(CORNER, bool)
    for k in range(6):
        mask[k, 4 + k, 60 + k] = True
    return mask


def corner_wye():
    """a Y whose node is the voxel (64, 8, 4): one arm down the diagonal into the tile below, one along x, one along -x a row and a slab on"""
    mask = np.zeros(CORNER, bool)
    mask[4, 8, 64] = True
    for k in (1, 2, 3):
        mask[4 - k, 8 - k, 64 - k] = True
        mask[4, 8, 64 + k] = True
        mask[5, 9, 64 - k] = True
    return mask


HAND = {'diagonal': diagonal, 'corner wye': corner_wye}
SETS = dict(RANDOM, **HAND)                                       # through Volume.graph(lo, hi)


def window(dtype):
    M = int(np.iinfo(dtype).max)
    return LO * (M // 255), M


@functools.lru_cache(maxsize=None)
def texels(name, dtype):
    """a case's texels: the shape (SHAPES) or the set itself (SETS) in codes of the range, the rest below it; in range at the same voxels in
    both widths, so one statement serves both"""
    mask = SHAPES[name]() if name in SHAPES else SETS[name]()
    a = host_texels(mask, dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def statement(name):
    """the graph of a case by the numpy statement: of the 'ends' skeleton of a shape, of a set as it is; computed once, never written to"""
    a = texels(name, np.uint8)
    if name in SHAPES:
        g = G.skeleton_graph_texels(skeleton_burn_texels(a, LO, HI, 'ends')[0])
    else:
        g = G.graph_texels(a, LO, HI)
    for key in ('classes', 'branch_ranks', 'node_ranks', 'branches', 'nodes'):
        g[key].setflags(write=False)
    return g


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d values differ, first at %s: %d, expected %d" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def check_graph(g, a, want, what):
    """everything a graph on the device says against the statement `want` over the texels `a`"""
    assert g.info == want['info'], what
    assert g.branch_records().tobytes() == want['branches'].tobytes(), what + ": branch records"
    assert g.node_records().tobytes() == want['nodes'].tobytes(), what + ": node records"
    same(g.branches.ranks(), want['branch_ranks'], what + ": branch ranks")
    same(g.nodes.ranks(), want['node_ranks'], what + ": node ranks")
    assert g.branches.info['listed'] == want['info']['branches'] and g.nodes.info['listed'] == want['info']['nodes'], what
    pair = g.classes()
    same(whole(pair), G.classes_texels(a, want), what + ": classes")
    pair.destroy()
    M = int(np.iinfo(a.dtype).max)
    for length, weights, debris, fill in ((0, (10, 14, 17), False, 0), (20, (10, 14, 17), False, 3), (45, (10, 14, 17), True, M), (2, (1, 0, 65535), False, 1),
                                          ((1 << 64) - 1, (65535, 65535, 65535), True, 7)):
        out = g.prune(length, weights, debris, fill)
        same(whole(out), G.prune_texels(a, want, length, weights, G.PRUNE_DEBRIS if debris else 0, fill), what + ": prune %r" % ((length, weights, debris, fill),))
        out.destroy()
    n = want['info']['branches']
    if n > 2:                                                     # a window of the lists
        assert g.branch_records(1, n - 2).tobytes() == want['branches'][1:n - 1].tobytes(), what
    assert np.array_equal(g.lengths(0.5), G.lengths(want['branches'], 0.5)), what
    ms, launches = g.profile()
    assert all(t >= 0.0 for t in ms.values()) and launches == (3 if want['info']['kept_voxels'] == 0 else 4 if n == 0 else 6), (what, launches)


# ---- the statement's cases are not empty ground ----------------------------------------------------------------------------------------
def test_the_cases_hold_what_they_are_for():
    for seed in (1, 2, 3, 4):
        info = statement('random 6x10x70 0.10 %d' % seed)['info']
        assert all(info[k] > 0 for k in ('isolated', 'segments', 'spurs', 'links', 'loops', 'cycles')), seed
    g = statement('diagonal')
    assert g['info']['branches'] == 1 and g['info']['segments'] == 1 and int(g['branches'][0]['steps_corner']) == 5 and g['classes'][3, 7, 63] == 3 and g['classes'][4, 8, 64] == 3
    g = statement('corner wye')
    assert g['classes'][4, 8, 64] == 4 and g['info']['nodes'] == 1 and int(g['nodes'][0]['degree']) == 3 and g['info']['spurs'] == 3 and g['info']['branches'] == 3
    for dtype in DTYPES:
        lo, hi = window(dtype)
        a = texels('torus', dtype)
        assert np.array_equal((a >= lo) & (a <= hi), SHAPES['torus']())


# ---- byte for byte against the statement ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", list(SHAPES))
def test_the_graph_of_a_skeleton_equals_the_statement(gpu_ctx, name, dtype):
    a = texels(name, dtype)
    lo, hi = window(dtype)
    want = statement(name)
    v = upload(gpu_ctx, a)
    k = v.skeleton(lo, hi, 'ends')
    g = k.graph()
    try:
        burn = k.burn()
        k.destroy(); v.destroy()                                  # the graph owns what it needs
        check_graph(g, a, want, "%s %s" % (name, np.dtype(dtype).name))
        assert np.array_equal(burn == KEPT, want['classes'] != 0)
    finally:
        for c in (g._branches, g._nodes):
            if c is not None:
                c.destroy()
        g.destroy(); k.destroy(); v.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", list(SETS))
def test_the_graph_of_a_range_equals_the_statement(gpu_ctx, name, dtype):
    a = texels(name, dtype)
    lo, hi = window(dtype)
    want = statement(name)
    v = upload(gpu_ctx, a)
    g = v.graph(lo, hi)
    try:
        assert whole(v).tobytes() == a.tobytes(), "the source changed"
        v.destroy()
        check_graph(g, a, want, "%s %s" % (name, np.dtype(dtype).name))
    finally:
        for c in (g._branches, g._nodes):
            if c is not None:
                c.destroy()
        g.close(); v.destroy()
    with pytest.raises(RuntimeError, match='destroyed'):
        g.info


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_both_entry_points_and_two_runs_give_the_same_bytes(gpu_ctx, dtype):
    a = texels('torus', dtype)
    lo, hi = window(dtype)
    v = upload(gpu_ctx, a)
    k = v.skeleton(lo, hi, 'ends')
    centre = k.volume()
    graphs = [k.graph(), k.graph(), centre.graph(lo, hi)]
    try:
        said = []
        for g in graphs:
            pair, pruned = g.classes(), g.prune(20, fill=2)
            said.append((g.info, g.branch_records().tobytes(), g.node_records().tobytes(), g.branches.ranks().tobytes(), g.nodes.ranks().tobytes(),
                         whole(pair).tobytes(), whole(pruned).tobytes()))
            pair.destroy(); pruned.destroy()
        assert said[0] == said[1], "two runs differ"
        # the kept set as a volume holds 0 outside the set where the skeleton's snapshot holds the source's codes: everything but the texels agrees
        assert said[0][:5] == said[2][:5], "the two entry points differ"
        assert said[0][0]['kept_voxels'] == 36
    finally:
        for g in graphs:
            for c in (g._branches, g._nodes):
                if c is not None:
                    c.destroy()
            g.destroy()
        centre.destroy(); k.destroy(); v.destroy()


# ---- branches and nodes are ordinary components ------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_branches_measure_and_keep_like_components(gpu_ctx, dtype):
    a = texels('torus', dtype)
    lo, hi = window(dtype)
    want = statement('torus')
    v = upload(gpu_ctx, a)
    thick = v.thickness(lo, hi)
    k = v.skeleton(lo, hi, 'ends')
    g = k.graph()
    branches, nodes = g.branches, g.nodes
    try:
        g.destroy()                                               # the components are the caller's and outlive the graph
        radius = np.ascontiguousarray(whole(thick)[..., 1])
        got = branches.measure(values=thick, channel=1)
        assert got.tobytes() == measure_texels(want['branch_ranks'], radius).tobytes() and len(got) == 6 and int(got['value_max'].max()) > 0
        assert branches.measure().tobytes() == measure_texels(want['branch_ranks'], a).tobytes()      # values None: the source's codes
        assert nodes.measure().tobytes() == measure_texels(want['node_ranks'], a).tobytes()
        for ranks, fill in (([1, 4], 0), ([2, 3, 6, 9], 5)):
            out = branches.keep_set(ranks, fill)
            same(whole(out), keep_set_texels(a, want['branch_ranks'], ranks, fill), "keep_set %r" % (ranks,))
            out.destroy()
        out = nodes.keep(1, 2)
        same(whole(out), vpt_amd.keep_texels(a, want['node_ranks'], 1, 2), "nodes.keep")
        out.destroy()
        out = branches.label()
        same(whole(out), vpt_amd.label_texels(a, want['branch_ranks']), "branches.label")
        out.destroy()
        assert branches.list() == vpt_amd.components_texels(want['classes'], 1, 3, 26)[1]
    finally:
        branches.destroy(); nodes.destroy(); g.destroy(); k.destroy(); thick.destroy(); v.destroy()


# ---- the convenience ---------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_centreline_with_and_without_prune(gpu_ctx, dtype):
    a = texels('torus', dtype)
    lo, hi = window(dtype)
    v = upload(gpu_ctx, a)
    try:
        out = v.centreline(lo, hi)
        same(whole(out), skeleton_texels(a, lo, hi), "centreline without prune")
        out.destroy()
        want = G.centreline_texels(a, lo, hi, 'ends', prune=20)
        ring = G.graph_texels(want, lo, hi)
        assert ring['info']['kept_voxels'] == 33 and ring['info']['cycles'] == 1 and ring['info']['branches'] == 1 and ring['info']['nodes'] == 0
        for rounds in (1, 3):
            out = v.centreline(lo, hi, prune=20, prune_rounds=rounds)
            same(whole(out), want, "centreline(prune=20, prune_rounds=%d)" % rounds)
            out.destroy()
        with pytest.raises(ValueError, match='covers every code'):
            v.centreline(0, int(np.iinfo(dtype).max), prune=20)
    finally:
        v.destroy()


# ---- the empty set, the error returns -------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_empty_set(gpu_ctx, dtype):
    M = int(np.iinfo(dtype).max)
    a = np.minimum(texels('random 9x11x12 0.10 1', dtype), dtype(M - 1))       # no voxel holds the largest code
    want = G.graph_texels(a, M, M)
    assert want['info']['kept_voxels'] == 0
    v = upload(gpu_ctx, a)
    g = v.graph(M, M)
    k = v.skeleton(M, M)
    h = k.graph()
    try:
        check_graph(g, a, want, "empty range")
        check_graph(h, a, want, "empty skeleton")
        assert len(g.branch_records()) == 0 and len(g.node_records()) == 0 and g.branches.list() == []
    finally:
        for x in (g, h):
            for c in (x._branches, x._nodes):
                if c is not None:
                    c.destroy()
            x.destroy()
        k.destroy(); v.destroy()


@pytest.mark.timeout(120)
def test_the_error_returns_name_what_was_wrong(gpu_ctx):
    L = N.lib()
    a = texels('corner wye', np.uint8)
    v = upload(gpu_ctx, a)
    pair = upload(gpu_ctx, np.ascontiguousarray(np.stack([a, a], axis=-1)))
    g = v.graph(LO, HI)
    h, out = C.c_void_p(), C.c_void_p()

    def refused(code, fragment, rc):
        assert rc == code and fragment in L.vpt_last_error().decode(), (rc, L.vpt_last_error())

    try:
        refused(N.ERR_INVALID, 'null', L.vpt_volume_graph(None, 1, 2, C.byref(h)))
        refused(N.ERR_INVALID, 'null', L.vpt_volume_graph(v.texture, 1, 2, None))
        refused(N.ERR_INVALID, 'null', L.vpt_skeleton_graph(None, C.byref(h)))
        refused(N.ERR_UNSUPPORTED, 'RG8', L.vpt_volume_graph(pair.texture, 1, 2, C.byref(h)))
        refused(N.ERR_INVALID, 'lo exceeds hi', L.vpt_volume_graph(v.texture, 3, 2, C.byref(h)))
        refused(N.ERR_INVALID, 'largest code', L.vpt_volume_graph(v.texture, 3, 256, C.byref(h)))
        assert not h.value
        refused(N.ERR_INVALID, 'null', L.vpt_graph_info(g._h, None))
        refused(N.ERR_INVALID, 'null', L.vpt_graph_info(None, C.byref(N.GraphInfo())))
        refused(N.ERR_INVALID, 'null', L.vpt_graph_branches(g._h, 0, 1, None))
        refused(N.ERR_INVALID, 'null', L.vpt_graph_nodes(g._h, 0, 1, None))
        assert L.vpt_graph_branches(g._h, 3, 0, None) == 0 and L.vpt_graph_nodes(g._h, 1, 0, None) == 0      # n = 0 checks the arguments only
        refused(N.ERR_INVALID, 'not within', L.vpt_graph_branches(g._h, 4, 0, None))
        refused(N.ERR_INVALID, 'not within', L.vpt_graph_branches(g._h, 2, 2, (N.GraphBranch * 2)()))
        refused(N.ERR_INVALID, 'not within', L.vpt_graph_nodes(g._h, 0, 2, (N.GraphNode * 2)()))
        refused(N.ERR_INVALID, 'null', L.vpt_graph_branch_components(g._h, None))
        refused(N.ERR_INVALID, 'null', L.vpt_graph_node_components(None, C.byref(h)))
        refused(N.ERR_INVALID, 'null', L.vpt_graph_classes(g._h, None))
        refused(N.ERR_INVALID, 'null', L.vpt_graph_prune(g._h, 1, 1, 1, 1, 0, 0, None))
        refused(N.ERR_INVALID, '65535', L.vpt_graph_prune(g._h, 1, 65536, 1, 1, 0, 0, C.byref(out)))
        refused(N.ERR_INVALID, '65535', L.vpt_graph_prune(g._h, 1, 1, 1, 65536, 0, 0, C.byref(out)))
        refused(N.ERR_INVALID, 'flags', L.vpt_graph_prune(g._h, 1, 1, 1, 1, 2, 0, C.byref(out)))
        refused(N.ERR_INVALID, 'largest code', L.vpt_graph_prune(g._h, 1, 1, 1, 1, 0, 256, C.byref(out)))
        refused(N.ERR_INVALID, 'null', L.vpt_graph_profile(g._h, None, None))
        refused(N.ERR_INVALID, 'null', L.vpt_graph_destroy(None))
        assert not out.value
        for bad in (lambda: v.graph(3, 2), lambda: v.graph(0, 256), lambda: g.prune(-1), lambda: g.prune(1, (1, 2)), lambda: g.prune(1, fill=256),
                    lambda: g.branch_records(4), lambda: g.node_records(0, 2)):
            with pytest.raises(ValueError):
                bad()
        with pytest.raises(vpt_amd.VptError, match='RG8'):
            pair.graph(1, 2)
    finally:
        g.destroy(); pair.destroy(); v.destroy()


# ---- at scale: every width, the axis limit, runs in a wave, many blocks, second trips -----------------------------------------------
# Each test asserts on the CPU, from the statement alone, the condition that makes it say something, then holds the device to the
# statement as above.  The device's layout, restated: a word of the bit plane holds 32 voxels along x, a row has wpr = 2 ceil(nx / 64)
# words, a scan block 256 words, a launch at most 8192 workgroups of 256 threads.
WIDTHS = (1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129)
GRID_CAP = 8192


def frozen(g):
    for key in ('classes', 'branch_ranks', 'node_ranks', 'branches', 'nodes'):
        g[key].setflags(write=False)
    return g


def graph_of_range(gpu_ctx, a):
    """Volume.graph over the window of `a`'s dtype; the source is destroyed at once: the graph owns what it needs"""
    lo, hi = window(a.dtype.type)
    v = upload(gpu_ctx, a)
    try:
        return v.graph(lo, hi)
    finally:
        v.destroy()


def release(g):
    for c in (g._branches, g._nodes):
        if c is not None:
            c.destroy()
    g.destroy()


@functools.lru_cache(maxsize=None)
def width_case(nx):
    """[3][5][nx] at density 0.15 and, at every x that is a multiple of 32 inside the volume, a kept pair across it along a row and one
    across it on a space diagonal: (the set, its statement)"""
    mask = np.random.default_rng(1000 + nx).random((3, 5, nx)) < 0.15
    for x in range(32, nx, 32):
        mask[0, 0, x - 1:x + 1] = True
        mask[1, 3, x - 1] = mask[2, 4, x] = True
    mask.setflags(write=False)
    return mask, frozen(G.graph_of(mask))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("nx", WIDTHS)
def test_every_width_round_a_word_and_a_segment(gpu_ctx, nx, dtype):
    """nx decides the segments a row (tnx), the words a row with their padding, whether gr_word(wx +- 1) leaves the row and whether the
    emitters have a tail (n % 4)."""
    mask, want = width_case(nx)
    kept = want['classes'] != 0
    assert {(3 * 5 * w) % 4 == 0 for w in WIDTHS} == {True, False} and kept.any()
    for x in range(32, nx, 32):                                   # both sides of every word edge, along a row and along a diagonal
        assert (kept[:, :, x - 1] & kept[:, :, x]).any(), x
        assert (kept[:-1, :-1, x - 1] & kept[1:, 1:, x]).any(), x
    g = graph_of_range(gpu_ctx, host_texels(mask, dtype))
    try:
        check_graph(g, host_texels(mask, dtype), want, "width %d %s" % (nx, np.dtype(dtype).name))
    finally:
        release(g)


LINES = {'x': ((2, 2, 4096), [(0, 0, slice(None))]), 'y': ((2, 4096, 2), [(0, slice(None), 0)]), 'z': ((4096, 2, 2), [(slice(None), 0, 0)]),
         'x twice': ((2, 3, 4096), [(0, 0, slice(None)), (0, 2, slice(None))]), 'y twice': ((2, 4096, 3), [(0, slice(None), 0), (0, slice(None), 2)]),
         'z twice': ((4096, 3, 2), [(slice(None), 0, 0), (slice(None), 2, 0)])}


@functools.lru_cache(maxsize=None)
def line_case(name):
    shape, lines = LINES[name]
    mask = np.zeros(shape, bool)
    for line in lines:
        mask[line] = True
    mask.setflags(write=False)
    return mask, frozen(G.graph_of(mask))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", list(LINES))
def test_a_line_as_long_as_an_axis_may_be(gpu_ctx, name, dtype):
    """4096 voxels along one axis, 2 along the others: one segment of 4095 face steps from the first voxel of the axis to the last.  A
    second line two voxels away needs three voxels across, so it has a case of its own: along y and z the list then alternates between the
    two branches voxel by voxel (runs of one lane), along x each line is 64 whole waves."""
    mask, want = line_case(name)
    lines = len(LINES[name][1])
    axis = 'zyx'.index(name[0])
    assert mask.shape[axis] == 4096 and want['info']['segments'] == want['info']['branches'] == lines and want['info']['nodes'] == 0
    flat = np.flatnonzero(mask.reshape(-1))
    for k, b in enumerate(want['branches']):
        assert (int(b['voxels']), int(b['steps_face']), int(b['steps_edge']), int(b['steps_corner']), int(b['free_ends'])) == (4096, 4095, 0, 0, 2)
        mine = np.flatnonzero((want['branch_ranks'] == k + 1).reshape(-1))
        assert (int(b['tip_lo']), int(b['tip_hi'])) == (int(mine[0]), int(mine[-1]))
    if lines == 2 and axis != 2:
        runs = [run for wave in GC.wave_runs(want) for run in wave]
        assert all(lanes == 1 for _, _, lanes in runs) and len(runs) == len(flat) == 8192
    g = graph_of_range(gpu_ctx, host_texels(mask, dtype))
    try:
        check_graph(g, host_texels(mask, dtype), want, "line %s %s" % (name, np.dtype(dtype).name))
    finally:
        release(g)


def test_no_volume_has_an_axis_of_4097_voxels(gpu_ctx):
    """vpt_volume_graph refuses more than 4096 voxels an axis (UNSUPPORTED, "at most 4096"), and so does the statement; a caller cannot get
    there: vpt_volume_create refuses such a volume first, and a skeleton is made of a volume."""
    with pytest.raises(ValueError, match='at most 4096'):
        G.graph_texels(np.zeros((1, 1, 4097), np.uint8), 1, 2)
    for shape in ((1, 1, 4097), (1, 4097, 1), (4097, 1, 1)):
        with pytest.raises(vpt_amd.VptError, match='out of range') as e:
            upload(gpu_ctx, np.zeros(shape, np.uint8))
        assert e.value.code == N.ERR_INVALID


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_runs_of_one_branch_along_a_wave(gpu_ctx, dtype):
    """k_gr_links sums a run of one key towards its first lane before it touches the record: graph_cases.wave_case holds a run over a whole
    wave, one that begins mid-wave and carries on through the next two, two runs of one branch parted by another branch and by node
    voxels, and a last run that is lane 63 alone."""
    mask = GC.wave_case()
    want = wave_statement()
    met = GC.wave_conditions(GC.wave_runs(want))
    assert all(met[k] for k in ('full', 'carried', 'apart', 'over nodes', 'last lane')), met
    assert want['info']['kept_voxels'] > 6 * 64 and want['info']['loops'] == 1 and want['info']['nodes'] > 0
    g = graph_of_range(gpu_ctx, host_texels(mask, dtype))
    try:
        check_graph(g, host_texels(mask, dtype), want, "runs in a wave %s" % np.dtype(dtype).name)
    finally:
        release(g)


@functools.lru_cache(maxsize=None)
def wave_statement():
    return frozen(G.graph_of(GC.wave_case()))


MANY = (127, 251, 65)                                             # [depth][height][width]


@functools.lru_cache(maxsize=None)
def many_blocks_case():
    """sparse noise and sixty small clumps in [127][251][65], three planes in the middle left empty: (the set, its statement)"""
    rng = np.random.default_rng(77)
    mask = rng.random(MANY) < 0.0016
    for _ in range(60):
        z, y, x = (int(rng.integers(0, n - 6)) for n in MANY)
        mask[z:z + 3, y:y + 4, x:x + 6] |= rng.random((3, 4, 6)) < 0.25
    mask[60:63] = False
    mask[-1, -1, -2:] = True                                      # the last block, which the run of one holds, is not empty
    mask.setflags(write=False)
    return mask, frozen(G.graph_of(mask))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_scan_of_many_blocks_places_the_list(gpu_ctx, dtype):
    """499 scan blocks: a thread of k_gr_scan_blocks owns a run of two, thread 249 a run of one, threads 250 .. 255 none; a voxel's place
    in the list, and so whether k_gr_links ever sees it, rests on the offset of its block."""
    mask, want = many_blocks_case()
    nz, ny, nx = MANY
    wpr = 2 * ((nx + 63) // 64)
    plane_words = nz * ny * wpr
    blocks = (plane_words + 255) // 256
    run = (blocks + 255) // 256
    assert plane_words > 65536 and blocks % 256 != 0 and run >= 2 and blocks % run != 0 and (blocks + run - 1) // run < 256
    z, y, x = np.nonzero(want['classes'])
    block = np.unique(((z * ny + y) * wpr + x // 32) // 256)
    assert len(np.unique(block // run)) >= 200 and int(block.max()) == blocks - 1
    empty = np.setdiff1d(np.arange(int(block.min()), int(block.max())), block)
    assert len(empty) >= 1                                        # an all-empty block between two that are not
    assert 3500 <= want['info']['kept_voxels'] <= 6000 and want['info']['nodes'] > 0 and want['info']['links'] > 0 and (nz * ny * nx) % 4 != 0
    g = graph_of_range(gpu_ctx, host_texels(mask, dtype))
    try:
        check_graph(g, host_texels(mask, dtype), want, "many blocks %s" % np.dtype(dtype).name)
    finally:
        release(g)


def texels_of_pieces(shape, pieces, dtype):
    """the pieces' sets in codes of the range, everything else below it; a motif's texels are made once"""
    made = {}
    a = np.zeros(shape, dtype)
    for (oz, oy, ox), kept in pieces:
        if id(kept) not in made:
            made[id(kept)] = host_texels(kept, dtype, seed=5 + len(made))
        d, h, w = kept.shape
        a[oz:oz + d, oy:oy + h, ox:ox + w] = made[id(kept)]
    return a


def pruned_shares(want, prunings):
    """per pruning whether the statement drops 'none', 'some' or 'all' of the branches"""
    gone = [int(GC.dropped(want['branches'], length, weights, G.PRUNE_DEBRIS if debris else 0).sum()) for length, weights, debris, _ in prunings]
    return ['none' if n == 0 else 'all' if n == len(want['branches']) else 'some' for n in gone]


def check_assembled(g, a, want, prunings, what):
    """`check_graph` against a statement put together from pieces (graph_cases.Assembled.statement), with the pruning stated without a
    Python loop over the records"""
    assert g.info == want['info'], what
    assert g.branch_records().tobytes() == want['branches'].tobytes(), what + ": branch records"
    assert g.node_records().tobytes() == want['nodes'].tobytes(), what + ": node records"
    for handed, name in ((g.branches, 'branch_ranks'), (g.nodes, 'node_ranks')):      # a copy of 4 bytes a voxel each: freed before the next
        try:
            same(handed.ranks(), want[name], "%s: %s" % (what, name))
        finally:
            handed.destroy()
    pair = g.classes()
    try:
        got = whole(pair)
    finally:
        pair.destroy()
    same(got[..., 0], a, what + ": classes, the codes")
    same(got[..., 1], want['classes'].astype(a.dtype), what + ": classes")
    del got
    for length, weights, debris, fill in prunings:
        flags = G.PRUNE_DEBRIS if debris else 0
        out = g.prune(length, weights, debris, fill)
        try:
            same(whole(out), GC.prune_texels(a, want['classes'], want['branch_ranks'], want['branches'], length, weights, flags, fill), what + ": prune %r" % ((length, weights, debris, fill),))
        finally:
            out.destroy()


@pytest.mark.timeout(300)
def test_the_second_trip_of_every_loop_over_voxels(gpu_ctx):
    """R16.  5400 copies of a padded random set that holds all six kinds, the last one another set: more than 2^21 kept voxels, so
    k_gr_links makes a second trip; k_gr_seed has more than 32 768 waves' worth of segments, the emitters more than 2^21 quads and the scan
    thousands of blocks.  The statement is put together from the two motifs (graph_cases.graph_on_pieces)."""
    first, last = GC.padded(RANDOM['random 6x10x70 0.10 1']()), GC.padded(RANDOM['random 6x10x70 0.10 2']())
    for seed in (1, 2):
        info = statement('random 6x10x70 0.10 %d' % seed)['info']
        assert all(info[k] > 0 for k in ('isolated', 'segments', 'spurs', 'links', 'loops', 'cycles'))
    shape = (8 * 54, 12 * 25, 72 * 4)
    nz, ny, nx = shape
    pieces = GC.tiling(shape, first, last)
    assert pieces[-1][1] is last and tuple(o + s for o, s in zip(pieces[-1][0], last.shape)) == shape and not np.array_equal(first, last)
    want = GC.graph_on_pieces(shape, pieces).statement()
    per_launch = GRID_CAP * 256
    assert want['info']['kept_voxels'] > per_launch                                          # k_gr_links
    assert ny * nz * ((nx + 63) // 64) > GRID_CAP * 4                                        # k_gr_seed: a wave an item
    assert nx * ny * nz // 4 > per_launch                                                    # k_gr_prune, k_gr_classes
    assert (ny * nz * 2 * ((nx + 63) // 64) + 255) // 256 > 16 * 256                         # k_gr_scan_blocks: runs of 17 and more
    assert want['info']['nodes'] > 0 and int(want['branches']['tip_hi'].max()) > nx * ny * (nz - 8)
    prunings = ((20, (10, 14, 17), False, 3), (30, (10, 14, 17), True, 65535))
    assert pruned_shares(want, prunings) == ['some', 'some']
    a = texels_of_pieces(shape, pieces, np.uint16)
    g = graph_of_range(gpu_ctx, a)
    try:
        check_assembled(g, a, want, prunings, "rich tiling")
    finally:
        release(g)


@pytest.mark.timeout(300)
def test_the_second_trip_of_the_loop_over_branches(gpu_ctx):
    """R8.  Isolated voxels on even coordinates and a few two-voxel segments, 2160 copies of [8][16][64]: more than 2^21 branches in 17.7 M
    voxels, so k_gr_init makes a second trip, every rank above 181 440 ties in voxel count and is ordered by its root, and the drop bitmap
    of a pruning has more than 65 536 words."""
    shape = (8 * 27, 16 * 20, 64 * 4)
    pieces = GC.tiling(shape, GC.dust_motif())
    want = GC.graph_on_pieces(shape, pieces, low_faces=False).statement()
    assert want['info']['branches'] > GRID_CAP * 256 and want['info']['branches'] // 32 + 1 > 65536
    assert want['info']['segments'] > 0 and want['info']['isolated'] > GRID_CAP * 256 - want['info']['segments']
    prunings = ((5, (10, 14, 17), True, 0), (9, (0, 14, 17), False, 9), (10, (10, 14, 17), True, 200))
    assert pruned_shares(want, prunings) == ['some', 'none', 'all']      # the isolated voxels; no spur to drop; the segments too
    a = texels_of_pieces(shape, pieces, np.uint8)
    g = graph_of_range(gpu_ctx, a)
    try:
        check_assembled(g, a, want, prunings, "dust tiling")
    finally:
        release(g)
