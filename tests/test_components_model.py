"""CPU: the inputs of tests/test_gpu_components_retry.py do what that file says of them, shown on the sequential model of the merge and
flatten phases (tests/components_model.py) without a device; the launch limit of the flatten loop; and vpt_volume_components_capped's
refusal of caps below the minima, which comes before any other check and so needs no device either.

The model performs whole unites in a drawn order: a subset of the device's interleavings (components_model.py says what that means)."""
import ctypes as C

import numpy as np
import pytest

from vpt_amd import _native as N
from vpt_amd.components import components_texels

import components_model as M

NOISE = (23, 19, 21)                                                # nx, ny, nz as in tests/test_gpu_components.py: 1 x 3 x 6 tiles
PLUS_ONE = (M.TX + 1, M.TY + 1, M.TZ + 1)
TWO_TILES = (2 * M.TX + 1, 2 * M.TY + 1, 2 * M.TZ + 1)
ORDERS = 20
# (merge, flatten): both minima; each minimum beside the production value of the other; one in between
CAPS = ((M.MERGE_STEPS_MIN, M.FLATTEN_STEPS_MIN), (M.MERGE_STEPS_MIN, M.FLATTEN_STEPS), (M.MERGE_STEPS, M.FLATTEN_STEPS_MIN), (8, 3))


def test_the_pairs_of_a_thread_come_in_the_order_of_the_kernel():
    assert M.merge_offsets(6) == [(-1, 0, 0), (0, -1, 0), (0, 0, -1)]
    assert [len(M.merge_offsets(c)) for c in (6, 18, 26)] == [3, 9, 13]
    for c in (6, 18, 26):
        assert all((dz, dy, dx) < (0, 0, 0) for dz, dy, dx in M.merge_offsets(c))


def test_the_flatten_launch_limit():
    assert M.flatten_launches(M.FLATTEN_STEPS) == 7                 # what the constant was for 64 steps
    assert M.flatten_launches(1) == 34 and M.flatten_launches(2) == 22 and M.flatten_launches((1 << 31) - 1) == 3
    for cap in (1, 2, 3, 7, 63, 64, 65, 1000, 65535, 65536, (1 << 31) - 1):
        j = M.flatten_launches(cap) - 2
        depth = 1 << 32
        for _ in range(j):
            depth = -(-depth // (cap + 1))
        assert depth <= cap, cap                                    # launch j + 1 confirms every root within its steps
        assert j == 0 or -(-(1 << 32) // (cap + 1) ** (j - 1)) > cap, cap     # ... and j is the first such number


@pytest.mark.parametrize("shape", (PLUS_ONE, TWO_TILES))
def test_the_corner_motif_gives_up_once_at_merge_cap_3_and_raises_the_first_flatten_at_cap_1(shape):
    a, count = M.corner_motifs(shape)
    assert count == (1 if shape == PLUS_ONE else 8)
    fg = a == 200
    for connectivity in (6, 18, 26):
        want = M.contract_roots(fg, connectivity)
        assert len(set(want)) == count + 1
    want = M.contract_roots(fg, 6)
    threads = M.merge_threads(fg, 6)
    assert len(threads) == count and all(len(t) == 2 for t in threads), "one thread a motif makes its two unites"
    for seed in range(ORDERS):
        for (merge, flatten), flattens in (((3, 1), [2, 2]), ((3, 64), [1, 1]), ((1024, 1), [2]), ((1024, 64), [1]), ((8, 3), [1])):
            L, got = M.label(fg, 6, merge, flatten, np.random.default_rng(seed))
            assert L == want, (seed, merge, flatten)
            assert got == flattens, (seed, merge, flatten, got)


@pytest.mark.parametrize("connectivity", (6, 18, 26))
def test_the_model_ends_at_the_roots_of_the_contract_under_any_admissible_caps(connectivity):
    fraction = {6: 0.30, 18: 0.13, 26: 0.09}[connectivity]
    nx, ny, nz = NOISE
    inputs = [np.random.default_rng(97).random((nz, ny, nx)) < fraction]
    if connectivity == 6:
        inputs += [M.corner_motifs(shape)[0] == 200 for shape in (PLUS_ONE, TWO_TILES)]
    more_than_one_launch = 0
    for fg in inputs:
        want = M.contract_roots(fg, connectivity)
        for seed in range(ORDERS):
            for merge, flatten in CAPS:
                L, flattens = M.label(fg, connectivity, merge, flatten, np.random.default_rng(1000 * merge + seed))
                assert L == want, (fg.shape, seed, merge, flatten)
                more_than_one_launch += len(flattens) > 1
    assert more_than_one_launch, "no input made the model launch the merge twice"


def test_the_list_of_a_larger_min_voxels_is_the_head_of_the_whole_list():
    """what tests/test_gpu_components_wrap.py relies on to take the statement of an 8 M voxel volume once"""
    nx, ny, nz = NOISE
    a = np.random.default_rng(101).integers(0, 256, size=(nz, ny, nx)).astype(np.uint8)
    ranks, listed = components_texels(a, 0, 76, 6)
    for min_voxels in (1, 2, 5, listed[0][3], listed[0][3] + 1):
        got = M.at_least(ranks, listed, min_voxels)
        want = components_texels(a, 0, 76, 6, min_voxels)
        assert got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes() and got[1] == want[1], min_voxels


def test_caps_below_the_minima_are_refused_before_anything_else():
    L = N.lib()
    assert "vpt_volume_components_capped" in N.SYMBOLS and hasattr(L, "vpt_volume_components_capped")
    out = C.c_void_p()
    # no volume and no device: a refused cap is reported although src is null ...
    for merge, flatten, text in ((2, 64, b"merge_steps 2: at least 3"), (0, 64, b"at least 3"), (-1, 1, b"at least 3"), (1024, 0, b"flatten_steps 0: at least 1"),
                                 (3, -5, b"at least 1")):
        assert L.vpt_volume_components_capped(None, 0, 1, 6, 1, merge, flatten, C.byref(out)) == N.ERR_INVALID, (merge, flatten)
        assert text in L.vpt_last_error(), (merge, flatten, L.vpt_last_error())
    # ... and the minima themselves pass that check: the null arguments are what is refused
    for src_out in ((None, C.byref(out)), (None, None)):
        assert L.vpt_volume_components_capped(src_out[0], 0, 1, 6, 1, M.MERGE_STEPS_MIN, M.FLATTEN_STEPS_MIN, src_out[1]) == N.ERR_INVALID
        assert b"null" in L.vpt_last_error()
