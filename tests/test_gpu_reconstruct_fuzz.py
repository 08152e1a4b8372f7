"""GPU: fixed-seed draws of a reconstruction or a geodesic operation behind another volume operation (a rank filter, a window or a
combination, as tests/test_gpu_volume_chain_fuzz.py chains the others): shape up to 70 x 20 x 10 (two tiles along x, three along y and z),
format, connectivity, operation and h are drawn; every volume the chain makes is read back whole and must equal, byte for byte, what the
numpy statements give for the same chain.  No draw is skipped: draw() makes only calls the contract takes.

VPT_RECONFUZZ_SEEDS=a:b widens the sweep."""
import os

import numpy as np
import pytest

from vpt_amd.combine import combine_texels
from vpt_amd.rank import rank_texels
from vpt_amd.reconstruct import GEODESIC_OPS, TAKES_H, geodesic_texels, reconstruct_texels
from vpt_amd.window import window_texels

from test_gpu_pyramid import upload, whole

pytestmark = pytest.mark.gpu

_SEEDS = range(*[int(v) for v in os.environ.get("VPT_RECONFUZZ_SEEDS", "0:40").split(":")])
CONSTANT = 0x5EED


def texels(rng, shape, dtype, style):
    """'noise': every code; 'levels': a few codes, so that plateaus occur; 'blobs': smooth hills, so that maxima have depth"""
    M = int(np.iinfo(dtype).max)
    if style == 'noise':
        return rng.integers(0, M + 1, size=shape).astype(dtype)
    if style == 'levels':
        codes = np.sort(rng.integers(0, M + 1, size=4))
        return codes[rng.integers(0, 4, size=shape)].astype(dtype)
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
    f = np.zeros(shape)
    for _ in range(6):
        cx, cy, cz, s, a = rng.uniform(0, shape[2]), rng.uniform(0, shape[1]), rng.uniform(0, shape[0]), rng.uniform(1.5, 6.0), rng.uniform(0.3, 1.0)
        f += a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) / (2 * s * s))
    return np.clip(f / max(f.max(), 1e-9) * M + rng.integers(-2, 3, size=shape), 0, M).astype(dtype)


def draw(seed):
    """the chain of a seed: {'source', 'second', 'front': (name, kwargs), 'call': ('reconstruct' | 'geodesic', kwargs)}"""
    rng = np.random.default_rng(CONSTANT + 7919 * seed)
    def axis(most):                                               # 1 .. most; three times in four at least 3, so that the volume has an inside
        n = int(rng.integers(1, most + 1))
        return int(rng.integers(3, most + 1)) if n < 3 and rng.integers(0, 4) else n
    shape = (axis(10), axis(20), axis(70))                        # [depth][height][width]
    dtype = (np.uint8, np.uint16)[int(rng.integers(0, 2))]
    M = int(np.iinfo(dtype).max)
    styles = ('noise', 'levels', 'blobs')
    case = {'seed': seed, 'source': texels(rng, shape, dtype, styles[int(rng.integers(0, 3))]),
            'second': texels(rng, shape, dtype, styles[int(rng.integers(0, 3))])}
    front = ('rank', 'window', 'combine')[int(rng.integers(0, 3))]
    if front == 'rank':
        case['front'] = ('rank', {'op': ('median', 'erode', 'dilate', 'open', 'close')[int(rng.integers(0, 5))], 'passes': 1})
    elif front == 'window':
        lo = int(rng.integers(0, M // 2))
        case['front'] = ('window', {'lo': lo, 'hi': int(rng.integers(lo + 1, M + 1)), 'bits': (8, 16)[int(rng.integers(0, 2))]})
    else:
        case['front'] = ('combine', {'op': ('min', 'max', 'absdiff')[int(rng.integers(0, 3))]})
    connectivity = (6, 18, 26)[int(rng.integers(0, 3))]
    if rng.integers(0, 4) == 0:
        case['call'] = ('reconstruct', {'op': ('dilation', 'erosion')[int(rng.integers(0, 2))], 'connectivity': connectivity,
                                        'marker_first': bool(rng.integers(0, 2))})
    else:
        op = list(GEODESIC_OPS)[int(rng.integers(0, len(GEODESIC_OPS)))]
        case['call'] = ('geodesic', {'op': op, 'h_fraction': float(rng.uniform(0.0, 0.5)) if op in TAKES_H else 0.0, 'connectivity': connectivity})
    return case


def describe(case):
    return "seed %d: %s %s, %s %r, then %s %r" % (case['seed'], case['source'].dtype, case['source'].shape[::-1], case['front'][0], case['front'][1],
                                                  case['call'][0], case['call'][1])


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s\n%d texels differ, first at [z, y, x] = %s: %d, expected %d" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("seed", _SEEDS)
def test_a_drawn_chain_equals_its_numpy_statements(gpu_ctx, seed):
    case = draw(seed)
    what = describe(case)
    source, second = case['source'], case['second']
    vols = [upload(gpu_ctx, source), upload(gpu_ctx, second)]
    try:
        name, kw = case['front']
        if name == 'rank':
            front, want = vols[0].rank(kw['op'], kw['passes']), rank_texels(source, kw['op'], kw['passes'])
        elif name == 'window':
            front, want = vols[0].window(kw['lo'], kw['hi'], 'r%d' % kw['bits']), window_texels(source, kw['lo'], kw['hi'], kw['bits'])
        else:
            front, want = vols[0].combine(vols[1], kw['op']), combine_texels(source, second, kw['op'])
        vols.append(front)
        same(whole(front), want, what + "\nthe front step")
        M = int(np.iinfo(want.dtype).max)
        name, kw = case['call']
        if name == 'reconstruct':
            other = second if second.dtype == want.dtype else window_texels(second, 0, int(np.iinfo(second.dtype).max), 8 * want.dtype.itemsize)
            vols.append(upload(gpu_ctx, other))
            marker, mask = (want, other) if kw['marker_first'] else (other, want)
            vmarker, vmask = (front, vols[-1]) if kw['marker_first'] else (vols[-1], front)
            out, expect = vmarker.reconstruct(vmask, kw['op'], kw['connectivity']), reconstruct_texels(marker, mask, kw['op'], kw['connectivity'])
        else:
            h = int(kw['h_fraction'] * M)
            out, expect = front.geodesic(kw['op'], h, kw['connectivity']), geodesic_texels(want, kw['op'], h, kw['connectivity'])
        vols.append(out)
        same(whole(out), expect, what)
        same(whole(front), want, what + "\nthe source afterwards")
    finally:
        for v in vols:
            v.destroy()
