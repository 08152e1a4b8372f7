"""CPU: the numpy statement of the per-component measurements and of the selection by a set of ranks (vpt_amd.measure_texels,
keep_set_texels, derive; vpt_amd/measure.py), which the device kernels are held to (tests/test_gpu_measure.py).

The statement is held to a loop over the components in Python integers, on noise of every connectivity and both widths; the identities
of the contract (include/vpt.h) hold; `derive` is held to float64 numpy over the selected voxels; the plain-JS twin (js/vpt/measure.js)
gives the same records on the same seeded inputs; a set that is an interval selects what `keep_texels` selects; and a component's
records in a slab of a larger volume differ from those in the slab alone by the slab's offset only (the pattern
tests/test_large_volumes_host.py shows, which tests/test_gpu_measure_large.py relies on)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import vpt_amd
from vpt_amd.measure import MEASURE_DTYPE, check_rank_set, check_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRACTION = {6: 0.30, 18: 0.13, 26: 0.09}            # the foreground fractions of tests/test_gpu_components.py
SHAPE = (11, 9, 13)                                 # nx, ny, nz


def noise(dtype, shape, seed):
    nx, ny, nz = shape
    return np.random.default_rng(seed).integers(0, int(np.iinfo(dtype).max) + 1, size=(nz, ny, nx)).astype(dtype)


def labelled(dtype, connectivity, seed, shape=SHAPE, min_voxels=1):
    a = noise(dtype, shape, seed)
    hi = int(round(FRACTION[connectivity] * (int(np.iinfo(dtype).max) + 1))) - 1
    ranks, listed = vpt_amd.components_texels(a, 0, hi, connectivity, min_voxels)
    return a, ranks, listed


def by_hand(ranks, values, rank):
    """the record of one rank from its voxels, in Python integers"""
    zs, ys, xs = (c.tolist() for c in np.nonzero(ranks == rank))
    vs = [int(v) for v in values[ranks == rank].tolist()]
    d, h, w = ranks.shape
    faces = 0
    for z, y, x in zip(zs, ys, xs):
        for dz, dy, dx in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
            zz, yy, xx = z + dz, y + dy, x + dx
            if not (0 <= zz < d and 0 <= yy < h and 0 <= xx < w) or int(ranks[zz, yy, xx]) != rank:
                faces += 1
    return (len(vs), min(xs), min(ys), min(zs), max(xs), max(ys), max(zs), min(vs), max(vs), sum(xs), sum(ys), sum(zs), sum(vs),
            sum(v * v for v in vs), faces)


def test_the_record_is_the_c_struct():
    from vpt_amd import _native as N
    import ctypes as C
    assert MEASURE_DTYPE.itemsize == C.sizeof(N.ComponentMeasure) == 88
    for name, _ in N.ComponentMeasure._fields_:
        assert MEASURE_DTYPE.fields[name][1] == getattr(N.ComponentMeasure, name).offset, name
    assert [n for n, _ in N.ComponentMeasure._fields_] == list(MEASURE_DTYPE.names)


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16))
@pytest.mark.parametrize("connectivity", (6, 18, 26))
def test_statement_equals_a_loop_over_the_components(connectivity, dtype):
    a, ranks, listed = labelled(dtype, connectivity, seed=11 + connectivity)
    assert len(listed) >= 16
    other = noise(np.uint16 if dtype == np.uint8 else np.uint8, SHAPE, seed=5)      # the measured width is independent of the labelled one
    for values in (a, other):
        records = vpt_amd.measure_texels(ranks, values)
        assert records.dtype == MEASURE_DTYPE and len(records) == len(listed)
        for k in range(len(listed)):
            assert tuple(int(v) for v in records[k]) == by_hand(ranks, values, k + 1), (k, records[k])
        # windows are slices of the whole; voxels outside a window contribute nothing
        for first, n in ((0, 1), (len(listed) - 1, 1), (3, 7), (0, len(listed)), (len(listed), 0), (2, 0)):
            assert vpt_amd.measure_texels(ranks, values, first, n).tobytes() == records[first:first + n].tobytes(), (first, n)
        assert vpt_amd.measure_texels(ranks, values, 5).tobytes() == records[5:].tobytes()
    for first, n in ((len(listed) + 1, 0), (0, len(listed) + 1), (len(listed), 1), (-1, 1), (0, -1), (0.5, 1)):
        with pytest.raises(ValueError):
            vpt_amd.measure_texels(ranks, a, first, n)
        with pytest.raises(ValueError):
            check_window(first, n, len(listed))
    with pytest.raises(ValueError):
        vpt_amd.measure_texels(ranks, a[:-1])
    with pytest.raises(ValueError):
        vpt_amd.measure_texels(ranks, a.astype(np.float32))


@pytest.mark.parametrize("connectivity", (6, 26))
def test_identities_of_the_contract(connectivity):
    a, ranks, listed = labelled(np.uint8, connectivity, seed=23, min_voxels=2)
    records = vpt_amd.measure_texels(ranks, a)
    assert [int(v) for v in records['voxels']] == [c[3] for c in listed]
    for r, (rx, ry, rz, voxels) in zip(records, listed):
        assert r['min_x'] <= rx <= r['max_x'] and r['min_y'] <= ry <= r['max_y'] and rz == r['min_z'] <= r['max_z']
    # faces = 6 voxels - 2 (face-adjacent pairs inside the component), whatever connectivity the labelling used
    pairs = np.zeros(len(listed) + 1, np.int64)
    for axis in range(3):
        lo, hi = np.moveaxis(ranks, axis, 0)[:-1], np.moveaxis(ranks, axis, 0)[1:]
        np.add.at(pairs, lo[lo == hi].astype(np.int64), 1)
    assert (records['faces'].astype(np.int64) == 6 * records['voxels'].astype(np.int64) - 2 * pairs[1:]).all()
    # everything foreground: one record, the surface of the block
    nx, ny, nz = SHAPE
    one = vpt_amd.measure_texels(np.ones((nz, ny, nx), np.uint32), a)
    assert len(one) == 1 and int(one[0]['faces']) == 2 * (nx * ny + ny * nz + nx * nz) and int(one[0]['voxels']) == nx * ny * nz
    assert int(one[0]['value_sum']) == int(a.astype(np.int64).sum()) and (one[0]['max_x'], one[0]['max_y'], one[0]['max_z']) == (nx - 1, ny - 1, nz - 1)


def test_the_words_hold_the_bounds_of_the_contract():
    ranks = np.ones((2, 3, 5), np.uint32)
    values = np.full((2, 3, 5), 65535, np.uint16)
    assert int(vpt_amd.measure_texels(ranks, values)[0]['value_sum_sq']) == 30 * 65535 * 65535
    largest = (1 << 32) * 65535 * 65535                              # past 2^63, below 2^64: the record's unsigned word holds it
    assert 1 << 63 < largest < 1 << 64 and int(np.array([largest], dtype=np.uint64)[0]) == largest
    assert 4095 * (1 << 32) < 1 << 64 and 6 * (1 << 32) < 1 << 64


def test_derive_equals_float64_numpy_over_the_voxels():
    a, ranks, listed = labelled(np.uint16, 6, seed=31)
    values = noise(np.uint16, SHAPE, seed=37)
    records = vpt_amd.measure_texels(ranks, values)
    got = vpt_amd.derive(records)
    assert len(got) == len(listed)
    for k in range(len(listed)):
        z, y, x = np.nonzero(ranks == k + 1)
        v = values[ranks == k + 1].astype(np.float64)
        ex, ey, ez = x.max() - x.min() + 1, y.max() - y.min() + 1, z.max() - z.min() + 1
        assert (got[k]['extent_x'], got[k]['extent_y'], got[k]['extent_z']) == (ex, ey, ez)
        want = (x.mean(), y.mean(), z.mean(), v.mean(), v.var(), len(v) / float(ex * ey * ez))
        have = tuple(float(got[k][f]) for f in ('centroid_x', 'centroid_y', 'centroid_z', 'mean', 'variance', 'fill'))
        # one division of exact integers against numpy's summation in float64: a few ulps of the largest term (mean^2 for the variance)
        for h, w, scale in zip(have, want, (1, 1, 1, 1, max(v.mean() ** 2, 1.0), 1)):
            assert abs(h - w) <= 1e-12 * max(abs(w), scale), (k, have, want)
    assert (got['variance'] >= 0).all()
    # the integer numerator: a constant component has variance exactly 0 at codes where the float form n s2 / n^2 - mean^2 cancels badly
    rec = np.zeros(1, MEASURE_DTYPE)
    rec['voxels'], rec['value_sum'], rec['value_sum_sq'] = 3000000007, 3000000007 * 65535, 3000000007 * 65535 * 65535
    assert float(vpt_amd.derive(rec)[0]['variance']) == 0.0 and float(vpt_amd.derive(rec)[0]['mean']) == 65535.0
    with pytest.raises(ValueError):
        vpt_amd.derive(np.zeros(1, MEASURE_DTYPE))


@pytest.mark.parametrize("dtype", (np.uint8, np.uint16))
def test_keep_set_over_an_interval_equals_keep(dtype):
    a, ranks, listed = labelled(dtype, 6, seed=41)
    n = len(listed)
    M = int(np.iinfo(dtype).max)
    for first, last, fill in ((1, 1, 0), (2, 5, M), (3, n, 7), (n, n + 9, 1), (1, n, 0)):
        want = vpt_amd.keep_texels(a, ranks, first, last, fill)
        assert vpt_amd.keep_set_texels(a, ranks, range(first, last + 1), fill).tobytes() == want.tobytes(), (first, last, fill)
    rng = np.random.default_rng(43)
    chosen = rng.permutation(n)[:n // 3] + 1
    want = np.where(np.isin(ranks, chosen), a, dtype(9))
    assert vpt_amd.keep_set_texels(a, ranks, chosen.tolist() + chosen[:3].tolist() + [n + 4, 1 << 40], 9).tobytes() == want.tobytes()
    mask = np.zeros(n, bool); mask[chosen - 1] = True
    assert vpt_amd.keep_set_texels(a, ranks, mask, 9).tobytes() == want.tobytes()
    assert (vpt_amd.keep_set_texels(a, ranks, [], 5) == 5).all()
    for bad in ([0], [1, 0], [-1], [1.5], ['1']):
        with pytest.raises(ValueError):
            vpt_amd.keep_set_texels(a, ranks, bad)
    for fill in (-1, M + 1, 0.5):
        with pytest.raises(ValueError):
            vpt_amd.keep_set_texels(a, ranks, [1], fill)
    with pytest.raises(ValueError):
        check_rank_set(np.zeros(n + 1, bool), n)


def test_a_slab_of_a_larger_volume_measures_like_the_slab_alone():
    """components that lie within a slab z0 .. z0 + d - 1 of an otherwise empty volume: against the slab alone sum_z differs by
    voxels * z0, min_z and max_z by z0, and every other field is equal"""
    nx, ny, d, z0, nz = 9, 7, 5, 11, 23
    slab = noise(np.uint8, (nx, ny, d), seed=47)
    slab[0] = slab[-1] = 255                                          # nothing touches the slab's ends: no component leaves it
    big = np.full((nz, ny, nx), 255, np.uint8)
    big[z0:z0 + d] = slab
    r_small, l_small = vpt_amd.components_texels(slab, 0, 76, 6)
    r_big, l_big = vpt_amd.components_texels(big, 0, 76, 6)
    assert len(l_small) == len(l_big) >= 8
    small, large = vpt_amd.measure_texels(r_small, slab), vpt_amd.measure_texels(r_big, big)
    for name in MEASURE_DTYPE.names:
        offset = {'sum_z': small['voxels'] * np.uint64(z0), 'min_z': z0, 'max_z': z0}.get(name, 0)
        assert (large[name] == small[name] + offset).all(), name


def js_records(case):
    """the records js/vpt/measure.js gives for a seeded case (js/test/test_measure_host.js prints them as JSON, 64-bit fields as strings)"""
    out = subprocess.run(["node", os.path.join(ROOT, "js", "test", "test_measure_host.js"), json.dumps(case)], stdout=subprocess.PIPE, check=True,
                         timeout=120)
    return json.loads(out.stdout.decode())


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_the_js_twin_checks_its_arguments_and_a_case_written_down():
    res = subprocess.run(["node", os.path.join(ROOT, "js", "test", "test_measure_host.js")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert res.returncode == 0 and res.stdout.decode().strip().splitlines()[-1] == 'js measure host: ok', res.stdout.decode()[-2000:]


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_the_js_twin_gives_the_same_records():
    for dtype, connectivity in ((np.uint8, 6), (np.uint16, 26)):
        a, ranks, listed = labelled(dtype, connectivity, seed=53)
        values = noise(np.uint16, SHAPE, seed=59)
        records = vpt_amd.measure_texels(ranks, values, 2, len(listed) - 3)
        chosen = [1, 3, 3, len(listed), len(listed) + 7]
        got = js_records({'shape': list(SHAPE), 'ranks': ranks.reshape(-1).tolist(), 'values': values.reshape(-1).tolist(), 'first': 2,
                          'n': len(listed) - 3, 'array': a.reshape(-1).tolist(), 'bits': 8 * a.itemsize, 'selected': chosen, 'fill': 6})
        assert len(got['records']) == len(records)
        for g, r in zip(got['records'], records):
            assert {k: int(v) for k, v in g.items()} == {name: int(r[name]) for name in MEASURE_DTYPE.names}
        assert got['kept'] == vpt_amd.keep_set_texels(a, ranks, chosen, 6).reshape(-1).tolist()
        derived = vpt_amd.derive(records)
        for g, r in zip(got['derived'], derived):
            for js_name, name in (('centroidX', 'centroid_x'), ('centroidY', 'centroid_y'), ('centroidZ', 'centroid_z'), ('mean', 'mean'),
                                  ('variance', 'variance'), ('extentX', 'extent_x'), ('extentY', 'extent_y'), ('extentZ', 'extent_z'), ('fill', 'fill')):
                assert g[js_name] == float(r[name]), (js_name, g[js_name], r[name])      # the same exact integers through the same one division
