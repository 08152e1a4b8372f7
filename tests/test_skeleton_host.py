"""CPU: the numpy statement of the thinning contract (vpt_amd.skeleton_burn_texels; include/vpt.h "curve skeleton"), held to what the
contract promises rather than to another implementation: the order of the visits inside a sub-step changes nothing; the kept set has the
object's components and the object's background components; thinning it again removes nothing; no kept border voxel could still go; the
burn passes are the history of the erosion.  The shapes have known answers.  The device and the JS statement are held to this statement
byte for byte (tests/test_gpu_skeleton.py, the JS twin below).

Two of these read differently in 'isthmus', by the contract's own wording: a marked voxel is skipped whatever has become of its
neighbourhood, so "no kept border voxel could still go" leaves the marked ones out, and the kept set is not a fixed point of a second run
that starts without the marks (the line below shows it by hand)."""
import functools
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import vpt_amd
from vpt_amd.components import components_texels
from vpt_amd.skeleton import (KEPT, INFO_FIELDS, MODES, burn_within_texels, check_skeleton, skeleton_burn_texels, skeleton_texels, topology, _CENTRE,
                              _WEIGHTS)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 20                                                            # the shapes' grid


def _grid():
    z, y, x = np.indices((G, G, G)).astype(np.float64)
    return z - 9.5, y - 9.5, x - 9.5


def ball():
    z, y, x = _grid()
    return x * x + y * y + z * z <= 49


def hollow_ball():
    z, y, x = _grid()
    r2 = x * x + y * y + z * z
    return (r2 <= 49) & (r2 > 16)


def torus():
    z, y, x = _grid()
    return (np.sqrt(x * x + y * y) - 6.0) ** 2 + z * z <= 4.0


def line():
    mask = np.zeros((G, G, G), bool)
    mask[7, 11, 3:17] = True
    return mask


def wye():
    """three cylinders of radius 2.5 and length 7 from the voxel (9, 9, 9), 120 degrees apart in the plane z = 9.  (The curve-end rule keeps
    a spur wherever a sub-step happens to leave a corner of a cylinder's cap standing, and which corners those are depends on the parity of
    the cap's position: the same Y one voxel further along x keeps five ends.  Pruning is not this contract's business; the Y stands where
    its three arms are the only ends.)"""
    z, y, x = (c - 9.0 for c in np.indices((G, G, G)).astype(np.float64))
    mask = np.zeros((G, G, G), bool)
    for k in range(3):
        ux, uy = np.cos(2 * np.pi * k / 3), np.sin(2 * np.pi * k / 3)
        s = x * ux + y * uy
        t = np.clip(s, 0.0, 7.0)
        mask |= ((x - t * ux) ** 2 + (y - t * uy) ** 2 + z * z <= 2.5 * 2.5) & (s <= 7.0)
    return mask


def noise(shape, seed, density=0.6):
    return np.random.default_rng(seed).random(shape) < density


SHAPES = {'ball': ball, 'hollow ball': hollow_ball, 'torus': torus, 'line': line, 'wye': wye}
RANDOM = {'noise %d' % seed: functools.partial(noise, (9, 11, 12), seed) for seed in (1, 2, 3, 4)}
CASES = dict(SHAPES, **RANDOM)
LO, HI = 100, 255


def texels(mask, dtype=np.uint8, seed=5):
    """the structure in codes of the upper part, the rest below it: the snapshot is not constant on either"""
    rng = np.random.default_rng(seed)
    M = int(np.iinfo(dtype).max)
    lo = LO * (M // 255)
    return np.where(mask, rng.integers(lo, M + 1, size=mask.shape), rng.integers(0, lo, size=mask.shape)).astype(dtype)


@functools.lru_cache(maxsize=None)
def statement(name, mode, passes=0):
    """(burn, info) of a case: computed once, shared, never written to"""
    burn, info = skeleton_burn_texels(texels(CASES[name]()), LO, HI, mode, passes)
    burn.setflags(write=False)
    return burn, info


def parts(mask, connectivity):
    return len(components_texels(mask.astype(np.uint8), 1, 1, connectivity)[1])


def background_parts(mask):
    return parts(~np.pad(mask, 1), 6)


def neighbourhood(padded, z, y, x):
    return int(padded[z:z + 3, y:y + 3, x:x + 3].ravel().dot(_WEIGHTS)) & ~_CENTRE


# ---- the neighbourhood test -------------------------------------------------------------------------------------------------------
def test_c_and_b_of_neighbourhoods_with_known_answers():
    bit = lambda dx, dy, dz: 1 << (9 * (dz + 1) + 3 * (dy + 1) + (dx + 1))
    full = (1 << 27) - 1 - _CENTRE
    assert topology(0) == (0, 1)                                  # an isolated voxel: no object part, one background
    assert topology(full) == (1, 0)                               # an interior voxel
    assert topology(bit(1, 0, 0)) == (1, 1)                       # a curve end is simple
    assert topology(bit(1, 0, 0) | bit(-1, 0, 0)) == (2, 1)       # the middle of a line
    assert topology(bit(1, 1, 1) | bit(-1, -1, -1)) == (2, 1)     # two opposite corners
    assert topology(full & ~bit(0, 0, 1)) == (1, 1)               # a voxel of a flat face
    assert topology(full & ~bit(0, 0, 1) & ~bit(0, 0, -1)) == (1, 2)   # a voxel of a one-voxel sheet between two cavities
    plane = sum(bit(dx, dy, 0) for dx in (-1, 0, 1) for dy in (-1, 0, 1)) - _CENTRE
    assert topology(plane) == (1, 2)                              # the middle of a plate keeps two sides apart
    assert topology(sum(bit(dx, dy, dz) for dx in (-1, 1) for dy in (-1, 1) for dz in (-1, 1))) == (8, 1)
    # a face neighbour in the background that no other background voxel of N18 touches is a part of its own
    assert topology(full & ~bit(0, 0, 1) & ~bit(1, 0, 0))[1] == 2
    assert topology(full & ~bit(0, 0, 1) & ~bit(1, 0, 0) & ~bit(1, 0, 1))[1] == 1


# ---- order independence -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_the_order_of_the_visits_changes_nothing(name, mode):
    burn, info = statement(name, mode)
    other, other_info = skeleton_burn_texels(texels(CASES[name]()), LO, HI, mode, order='reversed')
    assert other.tobytes() == burn.tobytes() and other_info == info


# ---- invariants -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_the_kept_set_has_the_objects_topology_and_is_a_fixed_point(name, mode):
    mask = CASES[name]()
    burn, info = statement(name, mode)
    kept = burn == KEPT
    assert burn.dtype == np.uint32 and tuple(info) == INFO_FIELDS
    assert np.array_equal(burn != 0, mask) and info['object_voxels'] == int(mask.sum()) and info['kept_voxels'] == int(kept.sum())
    last = int(burn[~kept].max())                                 # the last pass is the idle one; in 'isthmus' the one before it may only have marked
    assert info['converged'] == 1 and (last <= info['passes'] - 1 if mode == 'isthmus' else last == info['passes'] - 1)
    assert info['isolated'] + info['ends'] + info['regular'] + info['junctions'] == info['kept_voxels']
    assert parts(kept, 26) == parts(mask, 26), "object components"
    assert background_parts(kept) == background_parts(mask), "background components"
    # Thinning the kept set again deletes nothing and takes one idle pass.  Not in 'isthmus': the marks are state the kept set does not carry.
    # A straight line there loses an end voxel in sub-step 6 and the voxel behind it in sub-step 7, the rest is marked (C = 2); thinned
    # again, the unmarked line goes on losing its ends.  What the marks promise is the topology above.
    if mode != 'isthmus':
        again, again_info = skeleton_burn_texels(texels(kept), LO, HI, mode)
        assert np.array_equal(again == KEPT, kept) and again_info['passes'] == 1 and again_info['converged'] == 1
    # no kept border voxel is deletable under the mode's rule ('isthmus' skips a marked voxel whatever has become of it)
    padded = np.pad(kept, 1)
    marks = np.zeros(mask.shape, bool)
    assert skeleton_burn_texels(texels(mask), LO, HI, mode, marks=marks)[0].tobytes() == burn.tobytes()
    assert not marks[~kept].any() and (mode == 'isthmus' or not marks.any())
    for z, y, x in np.argwhere(kept):
        faces = padded[z, y + 1, x + 1] & padded[z + 2, y + 1, x + 1] & padded[z + 1, y, x + 1] & padded[z + 1, y + 2, x + 1] & padded[z + 1, y + 1, x] & padded[z + 1, y + 1, x + 2]
        if faces:
            continue
        obj = neighbourhood(padded, z, y, x)
        if (mode == 'ends' and bin(obj).count('1') == 1) or marks[z, y, x]:
            continue
        assert topology(obj) != (1, 1), (z, y, x)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ('ball', 'wye', 'noise 1'))
def test_the_burn_passes_are_the_history_of_the_erosion(name, mode):
    a = texels(CASES[name]())
    burn, info = statement(name, mode)
    assert info['passes'] >= 3
    for k in range(2, info['passes'] + 2):
        capped, capped_info = statement(name, mode, k - 1)
        assert np.array_equal(capped == KEPT, burn >= k), k
        assert np.array_equal(capped[capped != KEPT], burn[capped != KEPT]), k
        assert capped_info['passes'] == min(k - 1, info['passes']) and capped_info['converged'] == (1 if k - 1 >= info['passes'] else 0), k
        assert np.array_equal(burn_within_texels(a, burn, k, None), np.where(capped == KEPT, a, 0))


# ---- shapes -----------------------------------------------------------------------------------------------------------------------
def test_a_ball_thins_to_a_voxel_or_a_short_curve():
    assert int(ball().sum()) == 1472
    for mode in ('kernel', 'isthmus'):
        info = statement('ball', mode)[1]
        assert (info['kept_voxels'], info['isolated'], info['passes']) == (1, 1, 8), mode
    info = statement('ball', 'ends')[1]
    assert (info['kept_voxels'], info['ends'], info['regular'], info['junctions']) == (3, 2, 1, 0)


def test_a_hollow_ball_keeps_a_closed_surface_around_its_cavity():
    assert int(hollow_ball().sum()) == 1192
    burn, info = statement('hollow ball', 'kernel')
    kept = burn == KEPT
    assert parts(kept, 26) == 1 and background_parts(kept) == 2 and info['kept_voxels'] == 300


def test_a_torus_survives_as_a_closed_curve():
    burn, info = statement('torus', 'kernel')
    kept = burn == KEPT
    assert parts(kept, 26) == 1 and background_parts(kept) == 1
    assert info['kept_voxels'] >= 8 and info['regular'] == info['kept_voxels']           # every voxel of a closed curve has two neighbours


def test_a_line_keeps_its_ends_or_shrinks_to_a_voxel():
    burn, info = statement('line', 'ends')
    assert np.array_equal(burn == KEPT, line()) and (info['ends'], info['regular'], info['passes']) == (2, 12, 1)
    info = statement('line', 'kernel')[1]
    assert info['kept_voxels'] == 1 and info['isolated'] == 1


def test_a_wye_has_three_ends_and_a_junction():
    info = statement('wye', 'ends')[1]
    assert info['ends'] == 3 and info['junctions'] >= 1 and info['isolated'] == 0


# ---- arguments, the empty range, one voxel ----------------------------------------------------------------------------------------
def test_the_argument_checks():
    a = texels(noise((3, 4, 5), 9))
    for call in (lambda: skeleton_burn_texels(a, 3, 2, 'ends'), lambda: skeleton_burn_texels(a, 0, 256, 'ends'), lambda: skeleton_burn_texels(a, -1, 2, 'ends'),
                 lambda: skeleton_burn_texels(a, 1.5, 2, 'ends'), lambda: skeleton_burn_texels(a, True, 2, 'ends'), lambda: skeleton_burn_texels(a, 1, 2, 'curve'),
                 lambda: skeleton_burn_texels(a, 1, 2, 1), lambda: skeleton_burn_texels(a, 1, 2, 'ends', -1), lambda: skeleton_burn_texels(a, 1, 2, 'ends', 1.0),
                 lambda: skeleton_burn_texels(a, 1, 2, 'ends', 0, 'random'), lambda: skeleton_burn_texels(a.astype(np.float32), 1, 2, 'ends'),
                 lambda: skeleton_burn_texels(a[0], 1, 2, 'ends'), lambda: skeleton_burn_texels(np.zeros((0, 2, 2), np.uint8), 1, 2, 'ends'),
                 lambda: skeleton_burn_texels(np.zeros((1, 1, 4097), np.uint8), 1, 2, 'ends'),
                 lambda: burn_within_texels(a, np.zeros(a.shape, np.uint32), 5, 4), lambda: burn_within_texels(a, np.zeros(a.shape, np.uint32), 1, None, 256),
                 lambda: burn_within_texels(a, np.zeros((1, 1, 1), np.uint32)), lambda: burn_within_texels(a, np.zeros(a.shape, np.float32))):
        with pytest.raises(ValueError):
            call()
    assert skeleton_burn_texels(a.astype(np.uint16), 1, 65535, 'kernel')[1]['object_voxels'] > 0
    burn, _ = skeleton_burn_texels(a, LO, HI, 'ends')
    assert np.array_equal(skeleton_texels(a, LO, HI), burn_within_texels(a, burn)) and np.array_equal(skeleton_texels(a, LO, HI, fill=7), np.where(burn == KEPT, a, 7))
    assert vpt_amd.skeleton_burn_texels is skeleton_burn_texels and vpt_amd.skeleton_texels is skeleton_texels


@pytest.mark.parametrize("mode", list(MODES))
def test_the_empty_range_and_a_single_voxel(mode):
    a = texels(noise((3, 4, 5), 9))
    burn, info = skeleton_burn_texels(a, 99, 99, mode, 3)
    assert not burn.any() and info == dict(dict.fromkeys(INFO_FIELDS, 0), converged=1)
    burn, info = skeleton_burn_texels(np.full((1, 1, 1), 7, np.uint8), 7, 7, mode)
    assert burn.tolist() == [[[KEPT]]]
    assert info == {'object_voxels': 1, 'kept_voxels': 1, 'passes': 1, 'converged': 1, 'isolated': 1, 'ends': 0, 'regular': 0, 'junctions': 0}


def test_a_volume_that_is_all_object_reaches_one_voxel():
    burn, info = skeleton_burn_texels(np.full((5, 6, 7), 9, np.uint8), 9, 9, 'kernel')
    assert info['kept_voxels'] == 1 and info['object_voxels'] == 210


# ---- the RenderingContext option --------------------------------------------------------------------------------------------------
def test_the_skeleton_option_is_validated_when_the_context_is_made():
    """every refusal comes before the context opens a device"""
    for bad in ('skeleton', {}, {'lo': 1}, {'lo': 2, 'hi': 1}, {'lo': 1, 'hi': 2, 'mode': 'curve'}, {'lo': 1, 'hi': 2, 'mode': 1}, {'lo': 1, 'hi': 2, 'passes': -1},
                {'lo': 1, 'hi': 2, 'passes': 1.5}, {'lo': 1, 'hi': 2, 'fill': -1}, {'lo': 1, 'hi': 2, 'fill': 65536}, {'lo': 1, 'hi': 2, 'steps': 2},
                {'lo': 1, 'hi': 65536}, [1, 2]):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext({'skeleton': bad})
    with pytest.raises(ValueError, match='skeleton'):
        vpt_amd.RenderingContext({'skeleton': {'lo': 1, 'hi': 2, 'steps': 2}})
    ok = {'lo': 100, 'hi': 255}
    for other in ('distance', 'thickness'):
        with pytest.raises(ValueError, match="skeleton and %s mode 'within' .*name one of them" % other):
            vpt_amd.RenderingContext({'skeleton': ok, other: {'lo': 1, 'hi': 2, 'mode': 'within'}})
    assert check_skeleton(ok) == {'lo': 100, 'hi': 255, 'mode': 'ends', 'passes': 0, 'fill': 0}
    assert check_skeleton({'lo': 1, 'hi': 2, 'mode': 'isthmus', 'passes': 4, 'fill': 3}) == {'lo': 1, 'hi': 2, 'mode': 'isthmus', 'passes': 4, 'fill': 3}
    assert check_skeleton(None) is None


# ---- the JS statement -------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
@pytest.mark.parametrize("dtype", (np.uint8, np.uint16), ids=lambda d: np.dtype(d).name)
def test_the_js_twin_equals_the_statement(tmp_path, dtype):
    nz, ny, nx = 7, 9, 13
    M = int(np.iinfo(dtype).max)
    a = texels(noise((nz, ny, nx), 31, 0.65), dtype)
    lo, hi = LO * (M // 255), M - 1
    (tmp_path / "texels.raw").write_bytes(a.astype(a.dtype.newbyteorder('<')).tobytes())
    res = subprocess.run(["node", os.path.join(ROOT, "js", "test", "test_skeleton_host.js"), str(tmp_path / "texels.raw"), str(nx), str(ny), str(nz),
                          str(a.dtype.itemsize * 8), str(lo), str(hi)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = res.stdout.decode().strip().splitlines()
    assert lines[-1] == 'js skeleton host ok'
    got = json.loads(lines[-2])
    for mode in MODES:
        for passes in (0, 2):
            burn, info = skeleton_burn_texels(a, lo, hi, mode, passes)
            key = '%s %d' % (mode, passes)
            assert info['kept_voxels'] > 1 and got[key]['burn'] == burn.reshape(-1).tolist() and got[key]['info'] == info, key
