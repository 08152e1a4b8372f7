"""CPU: the numpy statement of morphological reconstruction and the geodesic operations (vpt_amd.reconstruct_texels, geodesic_texels) held to
a best-first path search over Python integers (the path statement of the contract), to scipy where it imports, and to the identities the
contract implies; the worked example of the contract (two overlapping balls: one component, two seeds); the plain-JS twin
(js/vpt/reconstruct.js, through js/test/test_reconstruct_host.js) held to the numpy statement; the `geodesic` option of RenderingContext; and
the C symbols without a device."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.reconstruct import (reconstruct_texels, geodesic_texels, check_geodesic_op, check_reconstruct_op, check_h, check_source_channel,
                                 RECONSTRUCT_OPS, GEODESIC_OPS)
from vpt_amd.components import components_texels
from vpt_amd.distance import distance_squared_texels, channel_texels

from reconstruct_cases import CONNECTIVITIES, DTYPES, best_paths, largest, serpentine, shells, touching, two_balls, value_sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (9, 6, 5)
IDS = dict(ids=lambda d: np.dtype(d).name)


# ---- the path statement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_the_fixed_point_is_the_best_path(dtype, connectivity):
    M = largest(dtype)
    for name, marker, mask in value_sets(dtype, SMALL, seed=3) + [('serpentine',) + serpentine((9, 7, 2), dtype)[:2]]:
        assert reconstruct_texels(marker, mask, 'dilation', connectivity).tobytes() == best_paths(marker, mask, connectivity).tobytes(), name
        # by erosion: the path statement of the complements
        want = M - best_paths(M - marker, M - mask, connectivity)
        assert reconstruct_texels(marker, mask, 'erosion', connectivity).tobytes() == want.astype(dtype).tobytes(), name


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_the_identities_of_the_contract(dtype, connectivity):
    M = largest(dtype)
    for name, marker, mask in value_sets(dtype, (13, 9, 6), seed=5):
        r = reconstruct_texels(marker, mask, 'dilation', connectivity)
        e = reconstruct_texels(marker, mask, 'erosion', connectivity)
        assert (r <= mask).all() and (r >= np.minimum(marker, mask)).all() and (e >= mask).all() and (e <= np.maximum(marker, mask)).all(), name
        assert (reconstruct_texels(M - marker, M - mask, 'erosion', connectivity) == M - r).all(), "duality, " + name
        assert (reconstruct_texels(r, mask, 'dilation', connectivity) == r).all() and (reconstruct_texels(e, mask, 'erosion', connectivity) == e).all(), "idempotence, " + name
        assert (reconstruct_texels(np.minimum(marker, mask), mask, 'dilation', connectivity) == r).all(), "a marker above the mask is clamped, " + name
        assert (reconstruct_texels(np.maximum(marker, mask), mask, 'erosion', connectivity) == e).all(), "a marker below the mask is clamped, " + name
        assert (geodesic_texels(mask, 'hmax', 0, connectivity) == mask).all() and (geodesic_texels(mask, 'hmin', 0, connectivity) == mask).all(), "h = 0, " + name
        h = 37 * (M // 255)
        hm = geodesic_texels(mask, 'hmax', h, connectivity)
        assert (hm <= mask).all() and (mask.astype(np.int64) - hm <= h).all()
        assert (geodesic_texels(mask, 'dome', h, connectivity) == mask - hm).all()
        assert (geodesic_texels(M - mask, 'hmin', h, connectivity) == M - hm).all(), "hmin is hmax of the complement, " + name
        assert (geodesic_texels(M - mask, 'minima', 0, connectivity) == geodesic_texels(mask, 'maxima', 0, connectivity)).all()
        filled = geodesic_texels(mask, 'fill_holes', 0, connectivity)
        assert (filled >= mask).all() and (geodesic_texels(filled, 'fill_holes', 0, connectivity) == filled).all()
        cleared = geodesic_texels(mask, 'clear_border', 0, connectivity)
        assert (cleared <= mask).all() and cleared[0].max() == 0 and cleared[:, :, -1].max() == 0, "the faces are connected to themselves"
    both = np.stack([marker, mask], axis=-1)
    assert (reconstruct_texels(both, both, 'dilation', connectivity, 0, 1) == r).all(), "channels of a two-channel array"
    assert (geodesic_texels(both, 'hmax', h, connectivity, 1) == hm).all()


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_the_edge_rules_of_maxima_and_minima(dtype):
    M = largest(dtype)
    a = np.zeros((3, 4, 5), dtype=dtype)
    assert geodesic_texels(a, 'maxima').max() == 0, "a voxel of code 0 is never a maximum"
    assert (geodesic_texels(a, 'minima') == M).all(), "a constant volume below M is one minimum"
    a[:] = M
    assert geodesic_texels(a, 'minima').max() == 0, "a voxel of code M is never a minimum"
    assert (geodesic_texels(a, 'maxima') == M).all()
    a[:] = 7
    a[1, 2, 2] = 8
    assert (geodesic_texels(a, 'maxima') == np.where(a == 8, M, 0)).all() and (geodesic_texels(a, 'minima') == np.where(a == 7, M, 0)).all()
    assert (geodesic_texels(a, 'hmax', M) == 0).all(), "h = M leaves nothing above 0"


@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_structures_that_touch_across_a_corner_or_an_edge(dtype):
    for second, joined_under in (((64, 8, 4), (26,)), ((64, 8, 3), (18, 26))):
        marker, mask = touching((66, 10, 6), dtype, second)
        for c in CONNECTIVITIES:
            r = reconstruct_texels(marker, mask, 'dilation', c)
            assert r[second[2], second[1], second[0]] == (150 if c in joined_under else 0) and r[3, 7, 63] == 150


# ---- scipy ------------------------------------------------------------------------------------------------------------------------
def structure(connectivity):
    from scipy import ndimage
    return ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_fill_holes_of_binary_volumes_equals_scipy(dtype, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    M = largest(dtype)
    rng = np.random.default_rng(17)
    noise = np.where(rng.random((9, 12, 14)) < 0.55, M, 0).astype(dtype)      # (has holes under 6 only: shells serve 18 and 26)
    cases = [noise, np.where(shells((15, 12, 9), dtype) > 0, M, 0).astype(dtype), np.where(shells((17, 15, 13), dtype, nested=True) > 0, M, 0).astype(dtype)]
    holes = 0
    for a in cases:
        # c is the connectivity of the path to the border, that is, of the background: scipy's structure is the background's too
        want = ndimage.binary_fill_holes(a > 0, structure=structure(connectivity))
        got = geodesic_texels(a, 'fill_holes', 0, connectivity)
        assert ((got > 0) == want).all() and set(np.unique(got)) <= {0, M}
        holes += int(np.count_nonzero(got != a))
    assert holes > 0, "degenerate input"


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_regional_maxima_are_the_plateaus_without_a_higher_neighbour(dtype, connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    M = largest(dtype)
    _, _, a = value_sets(dtype, (11, 9, 7), seed=29)[1]            # five codes: plateaus
    want = np.zeros(a.shape, dtype=bool)
    grown = ndimage.grey_dilation(a, footprint=structure(connectivity), mode='constant', cval=0)
    for value in np.unique(a):
        if value == 0:
            continue                                              # a voxel of code 0 is never a maximum
        labels, n = ndimage.label(a == value, structure=structure(connectivity))
        for k in range(1, n + 1):
            plateau = labels == k
            if grown[plateau].max() <= value:                     # no voxel of the plateau has a higher neighbour
                want |= plateau
    got = geodesic_texels(a, 'maxima', 0, connectivity)
    assert 0 < np.count_nonzero(want) < a.size and ((got == M) == want).all() and set(np.unique(got)) <= {0, M}
    assert (geodesic_texels(M - a, 'minima', 0, connectivity) == got).all()


# ---- the worked example of the contract ---------------------------------------------------------------------------------------------
def seeds(second_x, h):
    a = two_balls(second_x)
    assert len(components_texels(a, 100, 255, 26)[1]) == 1, "the threshold is one component"
    depth = channel_texels(a, distance_squared_texels(a, 100, 255, 'rest'), 4)
    maxima = geodesic_texels(geodesic_texels(depth, 'hmax', h, 26, 1), 'maxima', 0, 26)
    return len(components_texels(maxima, 255, 255, 26)[1])


def test_two_overlapping_balls_are_one_component_and_two_seeds():
    assert [seeds(19, h) for h in (0, 1, 2, 4, 8)] == [2, 2, 2, 2, 2]
    assert [seeds(17, h) for h in (0, 1, 2, 4, 8)] == [2, 2, 2, 1, 1]


# ---- the checks -------------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    assert [check_reconstruct_op(k) for k in ('dilation', 'erosion')] == [N.RECONSTRUCT_DILATION, N.RECONSTRUCT_EROSION] == list(RECONSTRUCT_OPS.values())
    assert [check_geodesic_op(k) for k in GEODESIC_OPS] == list(range(7)) and GEODESIC_OPS['minima'] == N.GEODESIC_MINIMA
    for bad in ('opening', 0, None):
        with pytest.raises(ValueError):
            check_reconstruct_op(bad)
        with pytest.raises(ValueError):
            check_geodesic_op(bad)
    for op, h in (('hmax', 256), ('hmax', -1), ('hmax', 1.5), ('hmax', True), ('maxima', 1), ('fill_holes', 2), ('clear_border', 1), ('minima', 1)):
        with pytest.raises(ValueError):
            check_h(op, h, 255)
    assert check_h('dome', 255, 255) == 255 and check_h('maxima', 0, 255) == 0
    for channel, channels in ((1, 1), (2, 2), (-1, 2), (True, 2)):
        with pytest.raises(ValueError):
            check_source_channel(channel, channels)
    a8, a16 = np.zeros((2, 3, 4), np.uint8), np.zeros((2, 3, 4), np.uint16)
    for call in (lambda: reconstruct_texels(a8, a16), lambda: reconstruct_texels(a8, a8[:1]), lambda: reconstruct_texels(a8, a8, connectivity=8),
                 lambda: reconstruct_texels(a8.astype(np.float32), a8), lambda: geodesic_texels(a8, 'hmax', 256), lambda: geodesic_texels(a8, 'maxima', 1),
                 lambda: geodesic_texels(a8, 'hmax', 1, channel=1), lambda: reconstruct_texels(a8, a8, 'closing')):
        with pytest.raises(ValueError):
            call()
    assert {'reconstruct_texels', 'geodesic_texels', 'RECONSTRUCT_OPS', 'GEODESIC_OPS'} <= set(vpt_amd.__all__)


def test_the_geodesic_option_is_validated_like_the_other_specs():
    spec = vpt_amd.RenderingContext._geodesic_spec
    assert spec(None) is None
    assert spec({'op': 'fill_holes'}) == {'op': 'fill_holes', 'h': 0, 'connectivity': 6}
    assert spec({'op': 'hmax', 'h': 300, 'connectivity': 26}) == {'op': 'hmax', 'h': 300, 'connectivity': 26}
    for bad in ('hmax', {}, {'h': 3}, {'op': 'watershed'}, {'op': 'hmax', 'h': -1}, {'op': 'hmax', 'h': 65536}, {'op': 'maxima', 'h': 1},
                {'op': 'hmax', 'connectivity': 4}, {'op': 'hmax', 'passes': 2}, ['hmax']):
        with pytest.raises(ValueError):
            spec(bad)


def test_the_library_refuses_null_arguments_and_a_bad_cap_without_a_device():
    L = N.lib()
    out = C.c_void_p()
    assert L.vpt_volume_reconstruct(None, 0, None, 0, 0, 6, C.byref(out)) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    assert L.vpt_volume_geodesic(None, 0, 0, 0, 6, C.byref(out)) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    assert L.vpt_volume_reconstruct_timed(None, 0, None, 0, 0, 6, C.byref(out), None, None, None) == N.ERR_INVALID
    assert L.vpt_volume_geodesic_timed(None, 0, 0, 0, 6, C.byref(out), None, None, None) == N.ERR_INVALID
    assert L.vpt_volume_reconstruct_capped(None, 0, None, 0, 0, 6, 0, C.byref(out), None, None) == N.ERR_INVALID and b"tile_rounds 0" in L.vpt_last_error()
    assert not out.value


# ---- the JS twin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
@pytest.mark.parametrize("dtype", DTYPES, **IDS)
def test_node_checks_and_twin_equal_the_numpy_statement(tmp_path, dtype):
    nx, ny, nz = 9, 6, 5
    M = largest(dtype)
    (_, a, mask), (_, b, _) = value_sets(dtype, (nx, ny, nz), seed=41)[:2]
    two = np.stack([a, b], axis=-1)
    little = lambda v: v.astype(v.dtype.newbyteorder('<')).tobytes()
    (tmp_path / "marker.raw").write_bytes(little(two)); (tmp_path / "mask.raw").write_bytes(little(mask))
    res = subprocess.run(["node", os.path.join(ROOT, "js", "test", "test_reconstruct_host.js"), str(tmp_path / "marker.raw"), str(tmp_path / "mask.raw"),
                          str(nx), str(ny), str(nz), str(a.dtype.itemsize * 8)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    lines = res.stdout.decode().strip().splitlines()
    assert lines[-1] == 'js reconstruct host ok'
    got = json.loads(lines[-2])
    for c in CONNECTIVITIES:
        for op in ('dilation', 'erosion'):
            for channel in (0, 1):
                assert got['reconstruct']['%s %d %d' % (op, c, channel)] == reconstruct_texels(two, mask, op, c, channel).reshape(-1).tolist(), (op, c, channel)
        for op in GEODESIC_OPS:
            h = 37 * (M // 255) if op in ('hmax', 'hmin', 'dome') else 0
            assert got['geodesic']['%s %d' % (op, c)] == geodesic_texels(mask, op, h, c).reshape(-1).tolist(), (op, c)
