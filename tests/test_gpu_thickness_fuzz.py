"""GPU: fixed-seed draws of local thickness (vpt_distance_thickness) against vpt_amd.thickness_squared_texels, word for word.  The texels are
drawn as tests/test_gpu_volume_chain_fuzz.py draws its volumes (volume_chain_cases.draw_texels: noise, a noisy sphere, sparse); every axis
is in 1 .. 40 with at most 20 000 voxels a case; format, value range and seed mode are drawn.  The generator sets one voxel inside and one
outside the range, so every case has a seed and a centre and none is skipped.  Every tenth case runs with all four combinations of the two
culls switched off.

VPT_THICKFUZZ_SEEDS=a:b widens the sweep."""
import os

import numpy as np
import pytest

from vpt_amd.distance import distance_squared_texels, thickness_squared_texels

import volume_chain_cases as V
from test_gpu_pyramid import upload
from test_gpu_reconstruct_fuzz import same

pytestmark = pytest.mark.gpu

_SEEDS = range(*[int(v) for v in os.environ.get("VPT_THICKFUZZ_SEEDS", "0:40").split(":")])
CONSTANT = 0x7B1C
MAX_VOXELS = 20000


def draw(seed):
    rng = np.random.default_rng(CONSTANT + 7919 * seed)
    while True:
        shape = tuple(int(rng.integers(1, 41)) for _ in range(3))            # [depth][height][width]
        if 2 <= shape[0] * shape[1] * shape[2] <= MAX_VOXELS:
            break
    fmt = ('R8', 'R16')[int(rng.integers(2))]
    texels = V.draw_texels(rng, fmt, shape)
    M = int(np.iinfo(texels.dtype).max)
    lo = int(rng.integers(1, M))                                              # 1 .. M - 1
    hi = int(rng.integers(lo, M)) if rng.integers(2) else M - 1               # lo .. M - 1: 0 and M are outside the range
    flat = texels.reshape(-1)
    inside, outside = (int(i) for i in rng.choice(flat.size, size=2, replace=False))
    flat[inside], flat[outside] = lo, (0, M)[int(rng.integers(2))]
    return {'seed': seed, 'texels': texels, 'lo': lo, 'hi': hi, 'seeds': ('rest', 'range')[int(rng.integers(2))]}


def describe(case):
    return "seed %d: %s %s, [%d, %d] %s" % (case['seed'], case['texels'].dtype, case['texels'].shape[::-1], case['lo'], case['hi'], case['seeds'])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("seed", _SEEDS)
def test_a_drawn_thickness_equals_its_numpy_statement(gpu_ctx, seed):
    case = draw(seed)
    what = describe(case)
    a = case['texels']
    d2 = distance_squared_texels(a, case['lo'], case['hi'], case['seeds'])
    assert (d2 == 0).any() and (d2 > 0).any(), what
    want = thickness_squared_texels(d2)
    v = upload(gpu_ctx, a)
    d = v.distance(case['lo'], case['hi'], case['seeds'])
    try:
        same(d.squared(), d2, what + "\nthe distances")
        for flags in ((None, 0, 1, 2, 3) if seed % 10 == 0 else (None,)):
            t = d.thickness() if flags is None else d.thickness_timed(_flags=flags)[0]
            try:
                same(t.squared(), want, what + "\nflags %r" % (flags,))
                assert t.info == {'seeds': int(np.count_nonzero(d2 == 0)), 'largest': int(d2.max())}, what
            finally:
                t.destroy()
        same(d.squared(), d2, what + "\nthe source afterwards")
    finally:
        d.destroy(); v.destroy()
