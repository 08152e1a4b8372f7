"""CPU: the numpy statement of the watershed contract (vpt_amd.watershed; include/vpt.h) held to an independent walk over Python integers
(breadth-first search for the lower completion, the pointer followed from every voxel, nothing united), to the properties the contract
names, and to the figures of its worked example; the plain-JS twin (js/vpt/watershed.js, through js/test/test_watershed_host.js) held to the
numpy statement; and the `split` option of RenderingContext."""
from collections import deque
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from vpt_amd.components import components_texels, neighbour_offsets
from vpt_amd.distance import channel_texels, distance_squared_texels
from vpt_amd.reconstruct import geodesic_texels
from vpt_amd.watershed import check_polarity, check_split, descent_texels, split_texels, watershed_texels

from reconstruct_cases import CONNECTIVITIES, DTYPES, largest, two_balls, value_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def walk(a, lo, hi, polarity, connectivity, min_voxels=1):
    """(ranks, basins, pointer) by the contract's words, over Python integers: d by breadth-first search from the plateaus' lower borders,
    p by an explicit minimum over (k, index), the basin of a voxel by following p to a minimum voxel, the regional minima by flood fill"""
    dep, h, w = a.shape
    M = largest(a.dtype)
    n = dep * h * w
    code = [int(c) for c in a.reshape(-1)]
    inside = [lo <= c <= hi for c in code]
    k = [(M - c if polarity == 'maxima' else c) for c in code]
    offsets = neighbour_offsets(connectivity)

    def neighbours(i):
        x, y, z = i % w, i // w % h, i // (w * h)
        for dz, dy, dx in offsets:
            xx, yy, zz = x + dx, y + dy, z + dz
            if 0 <= xx < w and 0 <= yy < h and 0 <= zz < dep:
                j = (zz * h + yy) * w + xx
                if inside[j]:
                    yield j

    d = [None] * n
    queue = deque()
    for i in range(n):
        if inside[i] and any(k[j] < k[i] for j in neighbours(i)):
            d[i] = 0
            queue.append(i)
    while queue:
        i = queue.popleft()
        for j in neighbours(i):
            if k[j] == k[i] and d[j] is None:
                d[j] = d[i] + 1
                queue.append(j)
    pointer = [-1] * n
    for i in range(n):
        if not inside[i]:
            continue
        if d[i] is None:
            pointer[i] = i
        elif d[i] == 0:
            pointer[i] = min((k[j], j) for j in neighbours(i) if k[j] < k[i])[1]
        else:
            pointer[i] = min(j for j in neighbours(i) if k[j] == k[i] and d[j] == d[i] - 1)
    # the regional minima by flood fill, named by their smallest voxel
    region = [None] * n
    for i in range(n):
        if inside[i] and d[i] is None and region[i] is None:
            region[i] = i
            queue.append(i)
            while queue:
                u = queue.popleft()
                for j in neighbours(u):
                    if d[j] is None and region[j] is None:
                        assert k[j] == k[u], "two adjacent minimum voxels have equal k"
                        region[j] = i
                        queue.append(j)
    members = {}
    for i in range(n):
        if inside[i]:
            t, steps = i, 0
            while pointer[t] != t:
                nxt = pointer[t]
                assert (k[nxt], -1 if d[nxt] is None else d[nxt]) < (k[t], d[t]), "(k, d) falls along p"
                t, steps = nxt, steps + 1
                assert steps <= n
            members.setdefault(region[t], []).append(i)
    basins = sorted(((min(v), len(v)) for v in members.values() if len(v) >= min_voxels), key=lambda b: (-b[1], b[0]))
    rank_of_root = {root: r + 1 for r, (root, _) in enumerate(basins)}
    ranks = np.zeros(n, np.uint32)
    for v in members.values():
        r = rank_of_root.get(min(v), 0)
        for i in v:
            ranks[i] = r
    return ranks.reshape(a.shape), [(r % w, r // w % h, r // (w * h), c) for r, c in basins], np.array(pointer, dtype=np.int64).reshape(a.shape)


CASES = [(shape, dtype, seed) for shape in ((1, 1, 1), (5, 1, 1), (7, 5, 3), (12, 9, 5)) for dtype in DTYPES for seed in (3,)]


@pytest.mark.parametrize("shape,dtype,seed", CASES, ids=lambda v: str(getattr(v, '__name__', v)))
def test_the_statement_equals_the_walk(shape, dtype, seed):
    M = largest(dtype)
    for name, a, b in value_sets(dtype, shape, seed):
        for relief in (a, b):
            for c in CONNECTIVITIES:
                for polarity in ('minima', 'maxima'):
                    for lo, hi in ((0, M), (M // 4, M), (0, M - M // 4)):
                        for min_voxels in (1, 3):
                            want_ranks, want_list, want_p = walk(relief, lo, hi, polarity, c, min_voxels)
                            ranks, basins = watershed_texels(relief, lo, hi, polarity, c, min_voxels)
                            what = (name, shape, c, polarity, lo, hi, min_voxels)
                            assert ranks.dtype == np.uint32 and np.array_equal(ranks, want_ranks), what
                            assert basins == want_list, what
                            assert np.array_equal(descent_texels(relief, lo, hi, polarity, c)[2], want_p), what


def test_the_properties_of_the_contract():
    rng = np.random.default_rng(5)
    for dtype in DTYPES:
        M = largest(dtype)
        for name, a, _ in value_sets(dtype, (14, 9, 6), 17):
            for c in CONNECTIVITIES:
                lo, hi = M // 5, M - M // 7
                ranks, basins = watershed_texels(a, lo, hi, 'minima', c)
                inside, d, p = descent_texels(a, lo, hi, 'minima', c)
                # every voxel of D is ranked, nothing outside D is; the counts add up
                assert np.array_equal(ranks != 0, inside) and np.array_equal(inside, (a >= lo) & (a <= hi))
                assert sum(b[3] for b in basins) == np.count_nonzero(inside)
                # basin(v) = basin(p(v))
                flat = ranks.reshape(-1)
                where = np.flatnonzero(inside.reshape(-1))
                assert np.array_equal(flat[where], flat[p.reshape(-1)[where]])
                # the root is the basin's smallest voxel
                for r, (x, y, z, voxels) in enumerate(basins, 1):
                    members = np.flatnonzero(flat == r)
                    assert len(members) == voxels and members[0] == (z * a.shape[1] + y) * a.shape[2] + x
                # maxima of a = minima of M - a over [M - hi, M - lo]
                other = watershed_texels((M - a.astype(np.int64)).astype(dtype), M - hi, M - lo, 'maxima', c)
                assert np.array_equal(other[0], ranks) and other[1] == basins
                # as many basins as regional minima (D the whole volume, no minimum of code M; likewise maxima and code 0)
                inner = np.clip(a, 1, M - 1)
                if name != 'constant':
                    for polarity in ('minima', 'maxima'):
                        marks = geodesic_texels(inner, polarity, 0, c)
                        assert len(watershed_texels(inner, 0, M, polarity, c)[1]) == len(components_texels(marks, M, M, c)[1]) > 0, (name, c, polarity)
        # a constant volume is one basin, although MINIMA marks nothing
        flat_volume = np.full((3, 4, 5), M, dtype=dtype)
        assert not geodesic_texels(flat_volume, 'minima', 0, 6).any()
        assert watershed_texels(flat_volume, 0, M, 'minima', 6)[1] == [(0, 0, 0, 60)]
        # a strictly monotone run is one basin
        run = np.sort(rng.choice(M + 1, size=40, replace=False)).astype(dtype).reshape(1, 1, 40)
        for polarity in ('minima', 'maxima'):
            assert watershed_texels(run, 0, M, polarity, 6)[1] == [(0, 0, 0, 40)]
            assert watershed_texels(run[:, :, ::-1], 0, M, polarity, 26)[1] == [(0, 0, 0, 40)]


def worked_example(second_x, h):
    a = two_balls(second_x)
    depth = channel_texels(a, distance_squared_texels(a, 100, 255, 'rest'), 4)
    return a, geodesic_texels(depth, 'hmax', h, 26, 1)


@pytest.mark.parametrize("h", (0, 1, 2, 4, 8))
def test_the_worked_example_two_overlapping_balls(h):
    a, flattened = worked_example(19, h)
    ranks, basins = watershed_texels(flattened, 1, 255, 'maxima', 26)
    assert basins == [(9, 8, 2, 924), (19, 8, 2, 887)], basins
    assert np.count_nonzero(ranks) == 1811 == np.count_nonzero(a)
    assert set(np.unique(ranks[:, :, :15])) == {0, 1} and set(np.unique(ranks[:, :, 15:])) == {0, 2}, "cut between x = 14 and x = 15"
    assert split_texels(a, 100, 255, h)[1] == basins and np.array_equal(split_texels(a, 100, 255, h)[0], ranks)
    got = walk(flattened, 1, 255, 'maxima', 26)
    assert got[1] == [(9, 8, 2, 924), (19, 8, 2, 887)] and np.array_equal(got[0], ranks)
    # the nearer pair: two basins while the saddle survives hmax, one behind it
    a, flattened = worked_example(17, h)
    sizes = [b[3] for b in watershed_texels(flattened, 1, 255, 'maxima', 26)[1]]
    assert sizes == ([887, 818] if h <= 2 else [1705]), (h, sizes)
    assert [b[3] for b in walk(flattened, 1, 255, 'maxima', 26)[1]] == ([887, 818] if h <= 2 else [1705]), h


def test_the_argument_checks():
    a = np.zeros((2, 3, 4), np.uint8)
    assert check_polarity('minima') == 0 and check_polarity('maxima') == 1
    for call in (lambda: watershed_texels(a, 0, 255, 'both'), lambda: watershed_texels(a, 0, 255, 0), lambda: watershed_texels(a, 3, 2),
                 lambda: watershed_texels(a, 0, 256), lambda: watershed_texels(a, 0, 255, 'minima', 8), lambda: watershed_texels(a, 0, 255, 'minima', 6, 0),
                 lambda: watershed_texels(a, 0, 255, 'minima', 6, 1, 1), lambda: watershed_texels(a.astype(np.float32), 0, 255),
                 lambda: check_split({'lo': 1}), lambda: check_split({'lo': 1, 'hi': 2, 'depth': 3}), lambda: check_split({'lo': 2, 'hi': 1}),
                 lambda: check_split({'lo': 1, 'hi': 2, 'connectivity': 7}), lambda: check_split({'lo': 1, 'hi': 2, 'minVoxels': 0}), lambda: check_split(3)):
        with pytest.raises(ValueError):
            call()
    assert check_split(None) is None
    assert check_split({'lo': 100, 'hi': 255}) == {'lo': 100, 'hi': 255, 'h': 2, 'steps': 4, 'connectivity': 26, 'minVoxels': 1}
    two = np.zeros((2, 3, 4, 2), np.uint16)
    two[..., 1] = 7
    assert watershed_texels(two, 1, 65535, 'maxima', 18, 1, 1)[1] == [(0, 0, 0, 24)] and watershed_texels(two, 1, 65535)[1] == []


def test_the_split_option_is_validated_when_the_context_is_made():
    """every refusal comes before the context opens a device"""
    import vpt_amd
    ok = {'lo': 100, 'hi': 255}
    for bad in ('split', {}, {'lo': 1}, {'lo': 2, 'hi': 1}, {'lo': 1, 'hi': 2, 'h': -1}, {'lo': 1, 'hi': 2, 'steps': 0}, {'lo': 1, 'hi': 2, 'connectivity': 7},
                {'lo': 1, 'hi': 2, 'minVoxels': 0}, {'lo': 1, 'hi': 2, 'depth': 3}, [1, 2]):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext({'split': bad})
    for other in ({'gradient': 'central'}, {'components': {'lo': 1, 'hi': 2, 'mode': 'label'}}, {'distance': {'lo': 1, 'hi': 2, 'mode': 'channel'}},
                  {'combine': {'reader': object(), 'op': 'pair'}}):
        with pytest.raises(ValueError, match='split and .* both write the second channel'):
            vpt_amd.RenderingContext(dict(other, split=ok))


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_the_js_twin_equals_the_statement(tmp_path, dtype):
    nx, ny, nz = 11, 7, 4
    M = largest(dtype)
    (_, a, _), (_, _, b) = value_sets(dtype, (nx, ny, nz), 29)[:2]
    two = np.stack([a, b], axis=-1)
    (tmp_path / "relief.raw").write_bytes(two.astype(two.dtype.newbyteorder('<')).tobytes())
    res = subprocess.run(["node", os.path.join(ROOT, "js", "test", "test_watershed_host.js"), str(tmp_path / "relief.raw"), str(nx), str(ny), str(nz),
                          str(two.dtype.itemsize * 8)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = res.stdout.decode().strip().splitlines()
    assert lines[-1] == 'js watershed host ok'
    got = json.loads(lines[-2])
    for c in CONNECTIVITIES:
        for polarity in ('minima', 'maxima'):
            for channel in (0, 1):
                ranks, basins = watershed_texels(two, M >> 3, M - (M >> 4), polarity, c, 2, channel)
                mine = got['%s %d %d' % (polarity, c, channel)]
                assert mine['ranks'] == ranks.reshape(-1).tolist() and [tuple(b) for b in mine['list']] == basins, (polarity, c, channel)
