"""GPU: the retry paths of vpt_volume_components, run on small volumes through vpt_volume_components_capped (include/vpt.h, "for tests"): a
unite that runs out of steps and gives up, the second and later merge launches behind it, the continuation of a unite behind a lost
atomicMin, and flatten launches that cannot confirm a root.  With the production caps (1024 and 64 steps) none of these runs below a
chain of more than a thousand tile components; with the smallest caps the bounds of the host's loops allow (3 and 1) they run on two tiles.

The caps change how often the host launches, never the result: every run is held through check() of tests/test_gpu_components.py to the
numpy statement of the contract, byte for byte, and a second run with the same caps to the same bytes.  The launch counts are asserted
only where one thread does all the uniting, so that no order of arrival can change them (components_model.corner_motifs has the trace,
tests/test_components_model.py replays it without a device); elsewhere they depend on the order and DESIGN.md reports what was seen."""
import ctypes as C

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N

from components_model import FLATTEN_STEPS, FLATTEN_STEPS_MIN, MERGE_STEPS, MERGE_STEPS_MIN, MOTIF_VOXELS, corner_motifs, flatten_launches
from test_gpu_components import (CONNECTIVITIES, DTYPES, PLUS_ONE, PLUS_ONE_4, TWO_TILES, TX, TY, TZ, box, check, noise, noise_range, serpentine,
                                 statement)
from test_gpu_pyramid import upload

pytestmark = pytest.mark.gpu

# (merge, flatten): both minima; each minimum beside the production value of the other; one in between
CAPS = ((MERGE_STEPS_MIN, FLATTEN_STEPS_MIN), (MERGE_STEPS_MIN, FLATTEN_STEPS), (MERGE_STEPS, FLATTEN_STEPS_MIN), (8, 3))


def twice(ctx, a, lo, hi, connectivity, caps, want, what):
    """check() with the caps, then a second run with the same caps held to the same bytes; (merge launches, flatten launches) of the second"""
    check(ctx, a, lo, hi, connectivity, what=what, caps=caps, want=want)
    src = upload(ctx, a)
    found = src.components(lo, hi, connectivity, _caps=caps)
    assert found.ranks().tobytes() == want[0].tobytes() and found.list() == want[1], "%s caps %r: the second run differs" % (what, caps)
    _, merges, flattens = found.profile()
    found.destroy(); src.destroy()
    assert merges >= 1 and merges <= flattens <= merges * (flatten_launches(FLATTEN_STEPS if caps is None else caps[1]) - 1), (what, caps, merges, flattens)
    return merges, flattens


def widened(a, lo, hi, dtype):
    """the uint8 case as it is, or the same foreground in 16 bits: every code times 257, the ends of the range with it"""
    return (a, lo, hi) if dtype == np.uint8 else (a.astype(np.uint16) * 257, lo * 257, hi * 257)


# ---- one thread unites: the launch counts are certain ---------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", (PLUS_ONE, TWO_TILES))
def test_a_unite_that_gives_up_is_made_again_by_the_next_merge_launch(gpu_ctx, shape, dtype):
    """The corner motif (components_model.corner_motifs: the trace is in its docstring), once on PLUS_ONE and at all eight corners of
    TWO_TILES, where eight unites give up in one launch.  6-connectivity: thread (x0, y0, z0) alone unites across tiles.
      merge cap 3:     its first unite hooks its root under the lone voxel below, its second needs a fourth step and gives up: 2 merge launches
      merge cap 1024:  1 merge launch
      flatten cap 1:   the voxel is two links from its root behind the merge launch and cannot confirm it in one step: at least 2 flatten
                       launches behind the first merge launch;  flatten cap 64: 1 flatten launch behind each merge launch"""
    motifs, count = corner_motifs(shape)
    assert count == (1 if shape == PLUS_ONE else 8)
    a, lo, hi = widened(motifs, 200, 200, dtype)
    want = statement(a, lo, hi, 6)
    assert len(want[1]) == count and all(c[3] == MOTIF_VOXELS for c in want[1])
    seen = {caps: twice(gpu_ctx, a, lo, hi, 6, caps, want, 'corner motif') for caps in CAPS + ((MERGE_STEPS, FLATTEN_STEPS), None)}
    print("corner motif %r %s: (merge, flatten) launches %r" % (shape, a.dtype.name, seen))
    assert seen[(3, 64)] == (2, 2), seen
    assert seen[(1024, 64)] == (1, 1) and seen[None] == (1, 1), seen             # None: vpt_volume_components itself
    assert seen[(1024, 1)][0] == 1 and seen[(1024, 1)][1] >= 2, seen             # one merge launch: every flatten launch is behind the first
    assert seen[(3, 1)][0] == 2 and seen[(3, 1)][1] >= 3, seen
    assert seen[(8, 3)] == (1, 1), seen                                        # 8 steps: the second unite confirms both roots; depth 2 <= 3


# ---- many threads unite: only the result is certain -----------------------------------------------------------------------------
def constructed(shape):
    """[(name, uint8 [nz][ny][nx], lo, hi)]: the inputs of test_constructed_cases whose components span tiles"""
    nx, ny, nz = shape
    cases = [('serpentine along ' + along, serpentine(shape, along), 200, 200) for along in ('x', 'z')]
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    cases.append(('checkerboard', np.where((x + y + z) % 2 == 0, 200, 0).astype(np.uint8), 200, 255))
    lo_x, lo_y, lo_z = (TX - 2, TX), (TY - 2, TY), (TZ - 2, TZ)
    hi_x, hi_y, hi_z = (TX, TX + 2), (TY, TY + 2), (TZ, TZ + 2)
    cases += [('edge along z', box(shape, lo_x, lo_y, lo_z) | box(shape, hi_x, hi_y, lo_z), 1, 255),
              ('edge along y', box(shape, lo_x, lo_y, lo_z) | box(shape, hi_x, lo_y, hi_z), 1, 255),
              ('edge along x', box(shape, lo_x, lo_y, lo_z) | box(shape, lo_x, hi_y, hi_z), 1, 255),
              ('edge along z, the other diagonal', box(shape, hi_x, lo_y, lo_z) | box(shape, lo_x, hi_y, lo_z), 1, 255),
              ('corner, main diagonal', box(shape, lo_x, lo_y, lo_z) | box(shape, hi_x, hi_y, hi_z), 1, 255),
              ('corner, another diagonal', box(shape, hi_x, lo_y, lo_z) | box(shape, lo_x, hi_y, hi_z), 1, 255)]
    a = box(shape, (0, 41), (2, 7), (0, 4))
    a[0, 2, 40:] = 200
    a[0, 0:3, nx - 1] = 200
    a[nz - 1, ny - 1, 0] = 200
    cases.append(('root in the last tile', a, 200, 200))
    return cases


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("shape", (PLUS_ONE, PLUS_ONE_4, TWO_TILES))
def test_reduced_caps_give_the_contract_on_chains_checkerboards_junctions_and_noise(gpu_ctx, shape, connectivity, dtype):
    """Which unite loses its atomicMin and goes on with the parent it displaced, and how deep a chain stands when a unite meets it, depends
    on the order of arrival: what is held is the result, under every pair of caps, and that a second run repeats it."""
    cases = [(name,) + widened(a, lo, hi, dtype) for name, a, lo, hi in constructed(shape)]
    cases.append(('noise', noise(dtype, shape, seed=91)) + noise_range(dtype, connectivity))
    most = {}
    for name, a, lo, hi in cases:
        want = statement(a, lo, hi, connectivity)
        if name.startswith('serpentine'):
            assert want[1] == [(0, 0, 0, int(((a >= lo) & (a <= hi)).sum()))]
        for caps in CAPS:
            seen = twice(gpu_ctx, a, lo, hi, connectivity, caps, want, name)
            most[caps] = tuple(max(m, s) for m, s in zip(most.get(caps, (0, 0)), seen))
    print("%r c%d %s: most (merge, flatten) launches %r" % (shape, connectivity, np.dtype(dtype).name, most))


# ---- what the entry refuses --------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_caps_below_the_minima_and_null_arguments_are_invalid(gpu_ctx):
    L = N.lib()
    out = C.c_void_p()
    vol = upload(gpu_ctx, np.zeros((4, 4, 4), np.uint8))
    for merge, flatten, text in ((MERGE_STEPS_MIN - 1, FLATTEN_STEPS, "merge_steps 2: at least 3"), (0, 1, "at least 3"), (-1024, 64, "at least 3"),
                                 (MERGE_STEPS, FLATTEN_STEPS_MIN - 1, "flatten_steps 0: at least 1"), (3, -64, "at least 1")):
        assert L.vpt_volume_components_capped(vol.texture, 0, 0, 6, 1, merge, flatten, C.byref(out)) == N.ERR_INVALID, (merge, flatten)
        assert text.encode() in L.vpt_last_error(), (merge, flatten, L.vpt_last_error())
        with pytest.raises(vpt_amd.VptError, match=text) as e:
            vol.components(0, 0, _caps=(merge, flatten))
        assert e.value.code == N.ERR_INVALID
    assert L.vpt_volume_components_capped(None, 0, 0, 6, 1, MERGE_STEPS_MIN, FLATTEN_STEPS_MIN, C.byref(out)) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    assert L.vpt_volume_components_capped(vol.texture, 0, 0, 6, 1, MERGE_STEPS_MIN, FLATTEN_STEPS_MIN, None) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    # the other arguments are checked as vpt_volume_components checks them
    for lo, hi, connectivity, min_voxels in ((5, 4, 6, 1), (0, 256, 6, 1), (0, 1, 8, 1), (0, 1, 6, 0)):
        assert L.vpt_volume_components_capped(vol.texture, lo, hi, connectivity, min_voxels, MERGE_STEPS_MIN, FLATTEN_STEPS_MIN, C.byref(out)) == N.ERR_INVALID
    found = vol.components(0, 0, _caps=(MERGE_STEPS_MIN, FLATTEN_STEPS_MIN))          # one tile: no merge launch at all
    assert found.list() == [(0, 0, 0, 64)] and found.profile()[1:] == (0, 0)
    found.destroy(); vol.destroy()
