"""CPU: connected components on the host.  vpt_amd.components_texels / keep_texels / label_texels (numpy, the statement the device kernels
are held to by tests/test_gpu_components.py) against a restatement in Python integers written here — a breadth-first search, the list
sorted by (-voxels, root) —, against scipy.ndimage.label where scipy is installed (as partitions: scipy numbers components differently),
the properties the contract of include/vpt.h implies, the argument errors, the option validation of RenderingContext, the plain-JS twins
and the C symbols without a device."""
import ctypes as C
import json
import os
import shutil
import subprocess
from collections import deque

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.components import (check_connectivity, check_keep, check_min_voxels, check_range, components_texels, keep_texels, label_texels,
                                neighbour_offsets)

from test_pyramid_host import int_texels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1, 1), (1, 5, 7), (3, 1, 17), (17, 3, 1), (5, 6, 9), (12, 11, 12))          # depth, height, width
DTYPES = (np.uint8, np.uint16)
CONNECTIVITIES = (6, 18, 26)
FRACTION = {6: 0.30, 18: 0.13, 26: 0.09}                        # foreground below the percolation density: many components


def code_range(dtype, connectivity):
    M = int(np.iinfo(dtype).max)
    lo = (M + 1) // 3
    return lo, lo + int(FRACTION[connectivity] * (M + 1))


def search(a, lo, hi, connectivity, min_voxels=1):
    """the contract in Python integers: (ranks as nested lists, [(root_x, root_y, root_z, voxels)])"""
    d, h, w = a.shape
    v = a.tolist()
    steps = [(c, b, e) for c in (-1, 0, 1) for b in (-1, 0, 1) for e in (-1, 0, 1)
             if 1 <= abs(c) + abs(b) + abs(e) <= {6: 1, 18: 2, 26: 3}[connectivity]]
    seen = [[[False] * w for _ in range(h)] for _ in range(d)]
    found = []                                                   # (voxels, root index, members)
    for z in range(d):
        for y in range(h):
            for x in range(w):
                if seen[z][y][x] or not lo <= v[z][y][x] <= hi:
                    continue
                seen[z][y][x] = True
                members, queue = [], deque([(z, y, x)])
                while queue:
                    p = queue.popleft()
                    members.append(p)
                    for c, b, e in steps:
                        q = (p[0] + c, p[1] + b, p[2] + e)
                        if 0 <= q[0] < d and 0 <= q[1] < h and 0 <= q[2] < w and not seen[q[0]][q[1]][q[2]] and lo <= v[q[0]][q[1]][q[2]] <= hi:
                            seen[q[0]][q[1]][q[2]] = True
                            queue.append(q)
                root = min((p[0] * h + p[1]) * w + p[2] for p in members)
                found.append((len(members), root, members))
    listed = sorted((f for f in found if f[0] >= min_voxels), key=lambda f: (-f[0], f[1]))
    ranks = [[[0] * w for _ in range(h)] for _ in range(d)]
    for k, (_, _, members) in enumerate(listed):
        for z, y, x in members:
            ranks[z][y][x] = k + 1
    return ranks, [(r % w, r // w % h, r // (w * h), n) for n, r, _ in listed]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_components_texels_equal_the_search(connectivity, dtype):
    lo, hi = code_range(dtype, connectivity)
    for shape in SHAPES:
        a = int_texels(dtype, shape, seed=61)
        for min_voxels in (1, 3):
            ranks, listed = components_texels(a, lo, hi, connectivity, min_voxels)
            want_ranks, want_listed = search(a, lo, hi, connectivity, min_voxels)
            assert ranks.dtype == np.uint32 and ranks.shape == a.shape
            assert ranks.tolist() == want_ranks and listed == want_listed, (connectivity, dtype, shape, min_voxels)
    assert len(components_texels(int_texels(dtype, SHAPES[-1], seed=61), lo, hi, connectivity)[1]) >= 16, "degenerate input"
    assert vpt_amd.components_texels is components_texels and vpt_amd.keep_texels is keep_texels and vpt_amd.label_texels is label_texels


def same_partition(p, q):
    """two labellings of the same voxels split them alike: the pairs (label in p, label in q) are a bijection"""
    pairs = np.unique(np.stack([p.reshape(-1), q.reshape(-1)]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1] == len(np.unique(pairs[1]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_partitions_equal_scipys(dtype):
    ndimage = pytest.importorskip("scipy.ndimage")
    for connectivity, order in ((6, 1), (18, 2), (26, 3)):
        lo, hi = code_range(dtype, connectivity)
        for shape in ((21, 19, 23), (9, 17, 65)):
            a = int_texels(dtype, shape, seed=67)
            ranks, listed = components_texels(a, lo, hi, connectivity)
            labels, count = ndimage.label((a >= lo) & (a <= hi), structure=ndimage.generate_binary_structure(3, order))
            assert count == len(listed) >= 32 and ((labels == 0) == (ranks == 0)).all()
            assert same_partition(labels, ranks)
            assert sorted(np.bincount(labels.reshape(-1))[1:].tolist(), reverse=True) == [c[3] for c in listed]


def refines(fine, coarse):
    """every part of `fine` lies in one part of `coarse`"""
    pairs = np.unique(np.stack([fine.reshape(-1), coarse.reshape(-1)]), axis=1)
    return len(np.unique(pairs[0])) == pairs.shape[1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_properties_the_contract_implies(dtype):
    M = int(np.iinfo(dtype).max)
    a = int_texels(dtype, (21, 19, 23), seed=71)
    lo, hi = code_range(dtype, 18)
    foreground = (a >= lo) & (a <= hi)
    r6, l6 = components_texels(a, lo, hi, 6)
    r18, l18 = components_texels(a, lo, hi, 18)
    r26, l26 = components_texels(a, lo, hi, 26)
    # 6 refines 18 refines 26, and each strictly here
    assert refines(r6, r18) and refines(r18, r26) and len(l6) > len(l18) > len(l26) > 1
    for ranks, listed in ((r6, l6), (r18, l18), (r26, l26)):
        assert ((ranks != 0) == foreground).all() and sum(c[3] for c in listed) == int(foreground.sum())
        sizes = [c[3] for c in listed]
        assert sizes == sorted(sizes, reverse=True) and np.bincount(ranks.reshape(-1))[1:].tolist() == sizes
        # a root is its component's first voxel, and ties in size are ordered by root
        d, h, w = a.shape
        index = [(z * h + y) * w + x for x, y, z, _ in listed]
        first = {int(k): int(i) for i, k in reversed(list(zip(np.flatnonzero(ranks.reshape(-1)), ranks.reshape(-1)[np.flatnonzero(ranks.reshape(-1))])))}
        assert index == [first[k + 1] for k in range(len(listed))]
        ties = [(p, q) for p, q in zip(range(len(sizes) - 1), range(1, len(sizes))) if sizes[p] == sizes[q]]
        assert len(ties) >= 8 and all(index[p] < index[q] for p, q in ties)
        # keep(1, None) with min_voxels = 1 gives back the foreground and fills the rest
        assert np.array_equal(keep_texels(a, ranks, 1, None, 0), np.where(foreground, a, 0))
        assert np.array_equal(keep_texels(a, ranks, 1, None, M), np.where(foreground, a, M))
        assert np.array_equal(keep_texels(a, ranks, 2, 3, 7) != 7, ((ranks == 2) | (ranks == 3)) & (a != 7))
        assert (keep_texels(a, ranks, len(listed) + 1, None, 5) == 5).all()
    # dropped components read as background
    r, l = components_texels(a, lo, hi, 6, 3)
    assert l == [c for c in l6 if c[3] >= 3] and np.array_equal(r, np.where(r6 <= len(l), r6, 0))
    assert components_texels(a, lo, hi, 6, l6[0][3] + 1)[1] == [] and not components_texels(a, lo, hi, 6, l6[0][3] + 1)[0].any()
    # the label channel saturates at M
    pair = label_texels(a, r6)
    assert pair.dtype == a.dtype and pair.shape == a.shape + (2,) and np.array_equal(pair[..., 0], a)
    assert np.array_equal(pair[..., 1], np.minimum(r6, M))
    big = np.array([[[0, 1, M - 1, M, M + 1, 70000, 0xFFFFFFFF]]], np.uint32)
    assert label_texels(np.zeros((1, 1, 7), dtype), big)[0, 0, :, 1].tolist() == [0, 1, M - 1, M, M, M, M]
    if dtype == np.uint8:
        assert len(l6) > 255 and int(pair[..., 1].max()) == 255 and int((r6 > 255).sum()) > 0


def test_whole_code_compares():
    codes = np.array([0x00FF, 0x0100, 0x7FFF, 0x8000, 0xFF00], np.uint16)
    a = codes[np.random.default_rng(73).integers(0, 5, size=(6, 7, 8))]
    for lo, hi, inside in ((0x0100, 0x8000, (0x0100, 0x7FFF, 0x8000)),      # not byte-wise: 0x00FF is below, 0xFF00 above
                           (0x00FF, 0x7FFF, (0x00FF, 0x0100, 0x7FFF)),      # not signed: 0x8000 and 0xFF00 are above
                           (0x8000, 0xFFFF, (0x8000, 0xFF00)), (0x0101, 0x7FFE, ())):
        ranks, listed = components_texels(a, lo, hi, 26)
        assert ((ranks != 0) == np.isin(a, inside)).all(), (lo, hi)
        assert search(a, lo, hi, 26) == (ranks.tolist(), listed)
    line = codes.reshape(1, 1, 5)
    assert components_texels(line, 0x0100, 0x8000, 6)[1] == [(1, 0, 0, 3)]


def test_size_ties_are_ordered_by_root_and_edges_do_not_wrap():
    a = np.zeros((3, 4, 9), np.uint8)
    a[2, 3, 7:9] = 5; a[0, 0, 0:2] = 5; a[1, 2, 4] = 5; a[0, 3, 8] = 5; a[1, 0, 0] = 9      # two pairs, two singletons, one out of range
    ranks, listed = components_texels(a, 5, 5, 26)
    assert listed == [(0, 0, 0, 2), (7, 3, 2, 2), (8, 3, 0, 1), (4, 2, 1, 1)]
    assert ranks[2, 3, 8] == 2 and ranks[0, 3, 8] == 3 and ranks[1, 0, 0] == 0
    # the last voxel of a row and the first of the next are neighbours in memory, not in the volume
    b = np.zeros((2, 2, 4), np.uint8)
    b[0, 0, 3] = b[0, 1, 0] = b[1, 0, 0] = 1
    assert len(components_texels(b, 1, 1, 6)[1]) == 3 and len(components_texels(b, 1, 1, 26)[1]) == 2


def test_arguments():
    a = np.zeros((2, 2, 2), np.uint8)
    assert [check_connectivity(c) for c in (6, 18, 26)] == [6, 18, 26] and [len(neighbour_offsets(c)) for c in (6, 18, 26)] == [6, 18, 26]
    for bad in (0, 4, 8, 27, -6, 6.0, '6', None, True):
        with pytest.raises(ValueError, match='connectivity'):
            check_connectivity(bad)
        with pytest.raises(ValueError):
            components_texels(a, 0, 1, bad)
    for lo, hi in ((2, 1), (0, 256), (-1, 5), (0.0, 1), (0, None), (True, 1)):
        with pytest.raises(ValueError):
            components_texels(a, lo, hi)
    assert check_range(0, 65535, 65535) == (0, 65535) and check_min_voxels(1) == 1
    with pytest.raises(ValueError):
        components_texels(np.zeros((2, 2, 2), np.uint16), 0, 65536)
    for bad in (0, -1, 1.5, '1', None, True, 1 << 32):
        with pytest.raises(ValueError, match='min_voxels'):
            check_min_voxels(bad)
        with pytest.raises(ValueError):
            components_texels(a, 0, 1, 6, bad)
    ranks = np.zeros((2, 2, 2), np.uint32)
    assert check_keep(1, None, 0, 255) == (1, 0xFFFFFFFFFFFFFFFF, 0)
    for first, last, fill in ((0, 1, 0), (2, 1, 0), (1, 1, 256), (1, 1, -1), (1.0, 2, 0), (1, 2, None), (1, 1 << 64, 0)):
        with pytest.raises(ValueError):
            keep_texels(a, ranks, first, last, fill)
    for bad in (np.zeros((2, 2, 2), np.int8), np.zeros((2, 2, 2), np.float32), np.zeros((2, 2), np.uint8), np.zeros((2, 2, 2, 2), np.uint8),
                np.zeros((0, 2, 2), np.uint8)):
        with pytest.raises(ValueError):
            components_texels(bad, 0, 1)
        with pytest.raises(ValueError):
            label_texels(bad, ranks)
    for bad in (np.zeros((2, 2, 3), np.uint32), np.zeros((2, 2, 2), np.float32)):
        with pytest.raises(ValueError):
            keep_texels(a, bad)
        with pytest.raises(ValueError):
            label_texels(a, bad)


def test_rendering_context_refuses_bad_options_in_the_constructor():
    good = {'lo': 0, 'hi': 1, 'mode': 'keep'}
    spec = vpt_amd.RenderingContext._components_spec
    assert spec(None) is None
    assert spec(good) == {'lo': 0, 'hi': 1, 'mode': 'keep', 'connectivity': 6, 'minVoxels': 1, 'keep': None}
    assert spec(dict(good, mode='label', connectivity=26, minVoxels=9, hi=65535))['connectivity'] == 26
    assert spec(dict(good, keep=4))['keep'] == 4
    for bad in ('keep', [0, 1], {'lo': 0, 'hi': 1}, {'lo': 0, 'mode': 'keep'}, dict(good, mode='drop'), dict(good, lo=2), dict(good, hi=65536),
                dict(good, connectivity=8), dict(good, minVoxels=0), dict(good, keep=0), dict(good, keep=1.5), dict(good, mode='label', keep=2),
                dict(good, colour=True)):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext({'components': bad})
    with pytest.raises(ValueError, match='second channel'):
        vpt_amd.RenderingContext({'components': dict(good, mode='label'), 'gradient': 'sobel'})


def test_symbols_resolve_and_null_handles_are_invalid_without_a_device():
    L = N.lib()
    names = ["vpt_volume_components", "vpt_components_info", "vpt_components_list", "vpt_components_ranks", "vpt_components_keep",
             "vpt_components_label", "vpt_components_destroy"]
    for name in names:
        assert hasattr(L, name) and name in N.SYMBOLS, name
    out = C.c_void_p()
    assert L.vpt_volume_components(None, 0, 1, 6, 1, C.byref(out)) == N.ERR_INVALID
    assert b"null" in L.vpt_last_error()
    assert L.vpt_components_info(None, C.byref(N.ComponentsInfo())) == N.ERR_INVALID
    assert L.vpt_components_list(None, 0, 0, None) == N.ERR_INVALID
    assert L.vpt_components_ranks(None, 0, 0, 0, 1, 1, 1, None, 0) == N.ERR_INVALID
    assert L.vpt_components_keep(None, 1, 1, 0, C.byref(out)) == N.ERR_INVALID
    assert L.vpt_components_label(None, C.byref(out)) == N.ERR_INVALID
    assert L.vpt_components_destroy(None) == N.ERR_INVALID
    assert C.sizeof(N.Component) == 16 and C.sizeof(N.ComponentsInfo) == 32


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
@pytest.mark.parametrize("dtype", DTYPES)
def test_node_twins_equal_the_numpy_statement(tmp_path, dtype):
    d, h, w = 11, 9, 13
    a = int_texels(dtype, (d, h, w), seed=79)
    (tmp_path / "texels.raw").write_bytes(a.astype(a.dtype.newbyteorder('<')).tobytes())
    cases = []
    for connectivity in CONNECTIVITIES:
        lo, hi = code_range(dtype, connectivity)
        cases += [[lo, hi, connectivity, 1, 1, None, 0], [lo, hi, connectivity, 2, 2, 3, 9]]
    script = ("const fs = require('fs'), c = require(%s);"
              "const raw = fs.readFileSync(process.argv[1]), bits = %d, cases = %s;"
              "const texels = bits === 8 ? new Uint8Array(raw) : new Uint16Array(raw.buffer, raw.byteOffset, raw.length / 2);"
              "const out = cases.map(k => { const r = c.componentsTexels(texels, %d, %d, %d, k[0], k[1], k[2], k[3]);"
              "  return { ranks: Array.from(r.ranks), list: r.list, keep: Array.from(c.keepTexels(texels, r.ranks, k[4], k[5], k[6])),"
              "           label: Array.from(c.labelTexels(texels, r.ranks)) }; });"
              "let refused = 0;"
              "for (const f of [() => c.componentsTexels(texels, %d, %d, %d, 0, 1, 8, 1), () => c.componentsTexels(texels, %d, %d, %d, 2, 1, 6, 1),"
              "                 () => c.componentsTexels(texels, %d, %d, %d, 0, 1, 6, 0), () => c.keepTexels(texels, out[0].ranks, 0, 1, 0),"
              "                 () => c.keepTexels(texels, out[0].ranks, 1, 1, 70000)]) { try { f(); } catch (e) { refused++; } }"
              "console.log(JSON.stringify({ out, refused }));") % ((json.dumps(os.path.join(ROOT, "js", "vpt", "components.js")), a.dtype.itemsize * 8,
                                                                     json.dumps(cases)) + (w, h, d) * 4)
    res = subprocess.run(["node", "-e", script, str(tmp_path / "texels.raw")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    got = json.loads(res.stdout.decode())
    assert got['refused'] == 5
    for case, g in zip(cases, got['out']):
        lo, hi, connectivity, min_voxels, first, last, fill = case
        ranks, listed = components_texels(a, lo, hi, connectivity, min_voxels)
        assert len(listed) >= 8, "degenerate input"
        assert g['ranks'] == ranks.reshape(-1).tolist() and [tuple(c) for c in g['list']] == listed, case
        assert g['keep'] == keep_texels(a, ranks, first, last, fill).reshape(-1).tolist(), case
        assert g['label'] == label_texels(a, ranks).reshape(-1).tolist(), case
