"""CPU: the numpy statement of local thickness (vpt_amd.thickness_squared_texels, thickness_texels, open_ball_texels) against a loop over
the centres that paints every ball; the invariants and the closed forms of the contract (include/vpt.h "local thickness"); the argument
checks; the `thickness` option of RenderingContext; the plain-JS twin (js/vpt/thickness.js) against the numpy statement."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import vpt_amd
from vpt_amd.distance import NONE, channel_texels, distance_squared_texels, open_ball_texels, thickness_squared_texels, thickness_texels, within_texels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = ('rest', 'range')


def painted(d2):
    """the contract as it reads: every centre paints its open ball with its D, a voxel keeps the largest"""
    d = d2.astype(np.int64)
    out = np.zeros_like(d)
    z, y, x = np.indices(d.shape)
    for c in np.argwhere(d > 0):
        D = d[tuple(c)]
        held = (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 < D
        out[held] = np.maximum(out[held], D)
    return out.astype(np.uint32)


def blobs(rng, shape):
    """a few balls at random centres, some cut by the border; code 200 inside, 0 .. 99 outside"""
    z, y, x = np.indices(shape)
    mask = np.zeros(shape, bool)
    for _ in range(int(rng.integers(1, 7))):
        c = [rng.integers(0, n) for n in shape]
        mask |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 <= rng.uniform(0.5, 6.0) ** 2
    return np.where(mask, 200, rng.integers(0, 100, size=shape)).astype(np.uint8)


def cases():
    rng = np.random.default_rng(77)
    shapes = [(19, 25, 18), (1, 1, 1), (1, 1, 23), (1, 9, 14), (7, 5, 3), (12, 3, 16), (4, 20, 9), (10, 10, 10), (2, 25, 2), (18, 6, 11)]
    return [blobs(rng, s) for s in shapes]


@pytest.mark.parametrize("seeds", SEEDS)
def test_the_statement_equals_the_painted_balls(seeds):
    checked = 0
    for a in cases():
        d2 = distance_squared_texels(a, 100, 255, seeds)
        if (d2 == NONE).all():
            continue
        got = thickness_squared_texels(d2)
        assert got.dtype == np.uint32 and got.shape == d2.shape
        assert np.array_equal(got, painted(d2)), (a.shape, seeds)
        checked += 1
    assert checked >= 8


def test_halving_the_centres_is_exercised(monkeypatch):
    """with room for few pairs at a time the statement asks several levels at once; the result is the same"""
    from vpt_amd import distance
    a = cases()[0]
    d2 = distance_squared_texels(a, 100, 255, 'range')
    want = painted(d2)
    calls = []
    covered = distance._covered
    monkeypatch.setattr(distance, '_covered', lambda *args: calls.append(1) or covered(*args))
    monkeypatch.setattr(distance, '_PAIRS', 1 << 10)
    assert np.array_equal(thickness_squared_texels(d2), want) and len(calls) > 10
    monkeypatch.setattr(distance, '_PAIRS', 1 << 40)
    del calls[:]
    assert np.array_equal(thickness_squared_texels(d2), want) and not calls


@pytest.mark.parametrize("seeds", SEEDS)
def test_the_invariants_of_the_contract(seeds):
    checked = 0
    for a in cases()[:6]:
        d2 = distance_squared_texels(a, 100, 255, seeds)
        if (d2 == NONE).all() or not d2.any():
            continue
        checked += 1
        t2 = thickness_squared_texels(d2)
        assert (t2 >= d2).all()
        assert np.array_equal(t2 == 0, d2 == 0)
        assert t2.max() == d2.max()
        z, y, x = np.indices(d2.shape)
        levels = np.unique(d2[d2 > 0])
        for t in {int(levels[0]), int(levels[len(levels) // 2]), int(levels[-1])}:
            union = np.zeros(d2.shape, bool)
            for c in np.argwhere(d2 >= max(t, 1)):
                union |= (z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2 < int(d2[tuple(c)])
            assert np.array_equal(t2 >= t, union), (a.shape, seeds, t)
        # flipping the input flips the result
        for axis in range(3):
            assert np.array_equal(thickness_squared_texels(np.flip(d2, axis)), np.flip(t2, axis))
        assert np.array_equal(thickness_squared_texels(d2.transpose(2, 0, 1)), t2.transpose(2, 0, 1))
    assert checked >= 4


@pytest.mark.parametrize("w", (1, 2, 5, 6))
def test_a_plate_is_as_thick_as_it_is(w):
    """a plate of w voxels that spans the volume: T2 = ceil(w / 2)^2 on every voxel of it, 0 off it"""
    half = (w + 1) // 2
    for axis, shape in ((0, (11, 6, 7)), (1, (5, 12, 4)), (2, (3, 8, 13))):
        a = np.zeros(shape, np.uint16)
        index = [slice(None)] * 3
        index[axis] = slice(2, 2 + w)
        a[tuple(index)] = 40000
        t2 = thickness_squared_texels(distance_squared_texels(a, 1, 65535, 'rest'))
        assert np.array_equal(t2, np.where(a > 0, half * half, 0)), (w, axis)
        pair = thickness_texels(a, 1, 65535)                       # steps 2: the diameter in voxels
        assert np.array_equal(pair[..., 0], a) and np.array_equal(pair[..., 1], np.where(a > 0, 2 * half, 0))
        assert np.array_equal(pair, channel_texels(a, t2, 2))
        assert np.array_equal(open_ball_texels(a, 1, 65535, half - 0.5), a)
        assert np.array_equal(open_ball_texels(a, 1, 65535, half, 7), np.full(shape, 7, np.uint16))


def test_no_seed_and_all_seeds():
    a = np.full((3, 4, 5), 9, np.uint8)
    none = distance_squared_texels(a, 1, 255, 'rest')
    assert (none == NONE).all()
    t2 = thickness_squared_texels(none)
    assert t2.dtype == np.uint32 and (t2 == NONE).all()
    assert np.array_equal(open_ball_texels(a, 1, 255, 1000.0), a)          # within(r2 + 1, None) selects NONE
    assert np.array_equal(thickness_texels(a, 1, 255)[..., 1], np.full(a.shape, 255))
    zero = thickness_squared_texels(distance_squared_texels(a, 1, 255, 'range'))
    assert zero.dtype == np.uint32 and not zero.any()


def test_the_argument_checks():
    a = np.zeros((2, 3, 4), np.uint8)
    a[0, 0, 0] = 200
    good = distance_squared_texels(a, 100, 255, 'rest')
    for bad in (good.reshape(-1), good.astype(np.float32), np.zeros((0, 3, 4), np.uint32), np.where(a > 0, NONE, 1).astype(np.uint32),
                good.astype(np.int64) - 5):
        with pytest.raises(ValueError):
            thickness_squared_texels(bad)
    assert np.array_equal(thickness_squared_texels(good.astype(np.int64)), thickness_squared_texels(good))
    for call in (lambda: open_ball_texels(a, 100, 255, -1.0), lambda: open_ball_texels(a, 100, 255, float('nan')), lambda: open_ball_texels(a, 100, 255, '3'),
                 lambda: open_ball_texels(a, 100, 255, True), lambda: open_ball_texels(a, 100, 255, 1, 256), lambda: open_ball_texels(a, 100, 255, 1, -1),
                 lambda: open_ball_texels(a, 100, 255, 1, 1.5), lambda: open_ball_texels(a, 3, 2, 1), lambda: open_ball_texels(a, 0, 256, 1),
                 lambda: open_ball_texels(a.astype(np.float32), 0, 1, 1), lambda: open_ball_texels(a[0], 0, 1, 1),
                 lambda: thickness_texels(a, 100, 255, 0), lambda: thickness_texels(a, 100, 255, 257), lambda: thickness_texels(a, 100, 255, 2, 'both')):
        with pytest.raises(ValueError):
            call()
    # a radius beyond every squared distance keeps nothing of a volume with a seed; radius 0 keeps the structure
    assert not open_ball_texels(a, 100, 255, 1e9).any()
    assert np.array_equal(open_ball_texels(a, 100, 255, 0), within_texels(a, good, 1, None))
    assert vpt_amd.thickness_squared_texels is thickness_squared_texels and vpt_amd.open_ball_texels is open_ball_texels


def test_the_thickness_option_is_validated_when_the_context_is_made():
    """every refusal comes before the context opens a device"""
    ok = {'lo': 100, 'hi': 255, 'mode': 'channel'}
    for bad in ('thickness', {}, {'lo': 1, 'hi': 2}, {'lo': 2, 'hi': 1, 'mode': 'within'}, {'lo': 1, 'hi': 2, 'mode': 'both'},
                {'lo': 1, 'hi': 2, 'mode': 'within', 'steps': 2}, {'lo': 1, 'hi': 2, 'mode': 'channel', 'from': 3}, {'lo': 1, 'hi': 2, 'mode': 'channel', 'fill': 1},
                {'lo': 1, 'hi': 2, 'mode': 'channel', 'steps': 0}, {'lo': 1, 'hi': 2, 'mode': 'within', 'seeds': 'all'},
                {'lo': 1, 'hi': 2, 'mode': 'within', 'from': 5, 'to': 4}, {'lo': 1, 'hi': 2, 'mode': 'within', 'radius': 3}, [1, 2]):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext({'thickness': bad})
    with pytest.raises(ValueError, match='thickness'):
        vpt_amd.RenderingContext({'thickness': {'lo': 1, 'hi': 2, 'mode': 'both'}})
    for mode in ('within', 'channel'):
        with pytest.raises(ValueError, match='distance and thickness'):
            vpt_amd.RenderingContext({'thickness': {'lo': 1, 'hi': 2, 'mode': mode}, 'distance': {'lo': 1, 'hi': 2, 'mode': 'within'}})
    for other in ({'gradient': 'central'}, {'components': {'lo': 1, 'hi': 2, 'mode': 'label'}}, {'combine': {'reader': object(), 'op': 'pair'}},
                  {'split': {'lo': 1, 'hi': 2}}):
        with pytest.raises(ValueError, match="thickness mode 'channel'.* both write the second channel|and thickness mode 'channel' both write"):
            vpt_amd.RenderingContext(dict(other, thickness=ok))
    spec = vpt_amd.RenderingContext._distance_spec
    assert spec(ok, 'thickness') == {'lo': 100, 'hi': 255, 'seeds': 'rest', 'mode': 'channel', 'from': 0, 'to': None, 'fill': 0, 'steps': 2}
    assert spec({'lo': 1, 'hi': 2, 'mode': 'within', 'from': 26}, 'thickness')['from'] == 26
    # the distance option reads as it did
    assert spec({'lo': 100, 'hi': 255, 'mode': 'channel'}) == {'lo': 100, 'hi': 255, 'seeds': 'range', 'mode': 'channel', 'from': 0, 'to': None, 'fill': 0, 'steps': 1}


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
@pytest.mark.parametrize("dtype", (np.uint8, np.uint16), ids=lambda d: np.dtype(d).name)
def test_the_js_twin_equals_the_statement(tmp_path, dtype):
    nz, ny, nx = 6, 9, 13
    rng = np.random.default_rng(31)
    M = int(np.iinfo(dtype).max)
    a = (blobs(rng, (nz, ny, nx)).astype(np.int64) * M // 255).astype(dtype)
    lo, hi = M // 2, M
    (tmp_path / "texels.raw").write_bytes(a.astype(a.dtype.newbyteorder('<')).tobytes())
    res = subprocess.run(["node", os.path.join(ROOT, "js", "test", "test_thickness_host.js"), str(tmp_path / "texels.raw"), str(nx), str(ny), str(nz),
                          str(a.dtype.itemsize * 8), str(lo), str(hi)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = res.stdout.decode().strip().splitlines()
    assert lines[-1] == 'js thickness host ok'
    got = json.loads(lines[-2])
    for seeds in SEEDS:
        want = thickness_squared_texels(distance_squared_texels(a, lo, hi, seeds))
        assert want.max() > 1 and got[seeds] == want.reshape(-1).tolist(), seeds
