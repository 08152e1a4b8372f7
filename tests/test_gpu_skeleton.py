"""GPU: curve skeleton and topological kernel by subfield thinning (vpt_volume_skeleton) on the device.

The whole burn field and every info field are held, byte for byte, to vpt_amd.skeleton_burn_texels, the numpy statement of the contract
(tests/test_skeleton_host.py holds that to what the contract promises), in all three modes.  No tolerance appears anywhere.

A workgroup owns a tile of 64 x 8 x 4 voxels, a word of the bit planes holds 32 voxels along x.  The shapes are the smallest at which that
can go wrong: 70 x 19 x 11 spans two whole tiles and a partial one along every axis and crosses the word boundary, filled with one blob
that crosses every seam and with noise of density 0.6; one voxel, a column, a row of 33 and a volume that is all object (the faces are its
only border); the ball, the hollow ball, the torus and the Y of the host test; a thick ball beside a thin line for the tile cull."""
import ctypes as C
import functools

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.combine import combine_texels
from vpt_amd.components import components_texels
from vpt_amd.distance import thickness_texels
from vpt_amd.skeleton import KEPT, MODES, burn_within_texels, skeleton_burn_texels, skeleton_texels

from test_gpu_pyramid import upload, whole
from test_skeleton_host import SHAPES, noise

pytestmark = pytest.mark.gpu

DTYPES = (np.uint8, np.uint16)
SEAMS = (11, 19, 70)                                              # [depth][height][width]


def ellipsoid(shape, centre, radii):
    z, y, x = np.indices(shape)
    return ((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 + ((x - centre[2]) / radii[2]) ** 2 <= 1.0


def blob():
    """one structure across every tile seam: an ellipsoid through the whole volume, a bar along each axis and a cavity"""
    mask = ellipsoid(SEAMS, (5, 9, 34), (4.6, 8.2, 33.0))
    mask[5, 9, :] = True; mask[:, 3, 40] = True; mask[2, :, 65] = True
    mask &= ~ellipsoid(SEAMS, (5, 9, 20), (2.0, 3.0, 5.0))
    return mask


def ball_and_line():
    """a thick ball and, tiles away from it, a thin line: the line's tiles have nothing to do after the first passes"""
    shape = (24, 40, 192)
    mask = ellipsoid(shape, (11, 19, 30), (9.0, 9.0, 9.0))
    mask[20, 36, 100:185] = True
    return mask


# name -> the structure, [depth][height][width] bool
CASES = {
    'blob': blob,
    'noise': functools.partial(noise, SEAMS, 17),
    'voxel': lambda: np.ones((1, 1, 1), bool),
    'column': lambda: np.ones((1, 40, 1), bool),
    'row 33': lambda: np.ones((1, 1, 33), bool),
    'all object': lambda: np.ones(SEAMS, bool),
    'nothing': lambda: np.zeros((5, 9, 33), bool),
    'ball and line': ball_and_line,
}
CASES.update(SHAPES)


def window(dtype):
    """the range: the upper half of the codes but for the very top of it, so the range cuts into the structure's codes"""
    M = int(np.iinfo(dtype).max)
    return M // 2 + 1, M - M // 16


@functools.lru_cache(maxsize=None)
def texels(name, dtype):
    """the structure in codes of the upper half (in 'blob' and 'noise' a sixteenth of them above the range: the range leaves voxels of the
    structure out), the rest in codes of the lower half.  The 16-bit array is in range exactly where the 8-bit one is: one statement
    serves both."""
    mask = CASES[name]()
    rng = np.random.default_rng(len(name))
    a = np.where(mask, rng.integers(128, 256, size=mask.shape), rng.integers(0, 128, size=mask.shape)).astype(np.uint8)
    if name not in ('blob', 'noise'):
        a = np.where(mask, np.minimum(a, 239), a).astype(np.uint8)          # only those two lose voxels to the range's upper end
    if dtype == np.uint16:
        a = (a.astype(np.uint16) << 8) | rng.integers(0, 256, size=mask.shape).astype(np.uint16)
        lo, hi = window(np.uint16)
        a = np.where((a >> 8) == 0xF0, np.minimum(a, hi), a).astype(np.uint16)                # 0xF0xx: in range up to hi = 0xF000
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def statement(name, mode, passes=0):
    """(burn, info) of a case: computed once on the 8-bit texels, shared by every test, never written to"""
    burn, info = skeleton_burn_texels(texels(name, np.uint8), *window(np.uint8), mode, passes)
    burn.setflags(write=False)
    return burn, info


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d values differ, first at [z, y, x] = %s: %d, expected %d" % (what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def test_the_two_widths_share_a_statement():
    for name in CASES:
        (lo8, hi8), (lo16, hi16) = window(np.uint8), window(np.uint16)
        a8, a16 = texels(name, np.uint8), texels(name, np.uint16)
        assert np.array_equal((a8 >= lo8) & (a8 <= hi8), (a16 >= lo16) & (a16 <= hi16)), name
    a = texels('noise', np.uint8)
    assert 0 < ((a >= 128) & (a > window(np.uint8)[1])).sum() < CASES['noise']().sum()       # the range leaves some of the structure out


# ---- the result, its info, the source afterwards -------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", list(CASES))
def test_burn_passes_and_info_equal_the_statement(gpu_ctx, name, dtype, mode):
    a = texels(name, dtype)
    lo, hi = window(dtype)
    burn, info = statement(name, mode)
    what = "%s %s %s" % (name, np.dtype(dtype).name, mode)
    v = upload(gpu_ctx, a)
    k = v.skeleton(lo, hi, mode)
    try:
        same(k.burn(), burn, what)
        assert k.info == info, what
        ms, launches, tiles = k.profile()
        assert launches == (1 if info['object_voxels'] == 0 else 2 + 9 * info['passes']), what
        assert all(t >= 0.0 for t in ms.values()) and (tiles > 0) == (info['object_voxels'] > 0), what
        assert whole(v).tobytes() == a.tobytes(), what + ": the source changed"
        dz, dy, dx = (n // 3 for n in a.shape)                    # a box that starts and ends inside the volume
        same(k.burn(dx, dy, dz, a.shape[2] - dx, a.shape[1] - dy, a.shape[0] - dz), np.ascontiguousarray(burn[dz:, dy:, dx:]), what + ": a box")
    finally:
        k.destroy(); v.destroy()
    if name in ('voxel', 'column', 'row 33', 'all object') and mode == 'kernel':
        assert info['kept_voxels'] == 1 and info['object_voxels'] == a.size, what


# ---- the pass cap --------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ('blob', 'noise', 'ball'))
def test_the_pass_cap_and_converged(gpu_ctx, name, mode):
    a = texels(name, np.uint8)
    lo, hi = window(np.uint8)
    full = statement(name, mode)[1]['passes']
    assert full >= 3
    v = upload(gpu_ctx, a)
    try:
        for passes in (1, 2, full + 1):
            burn, info = statement(name, mode, passes)
            k = v.skeleton(lo, hi, mode, passes)
            got, got_info = k.burn(), k.info
            k.destroy()
            same(got, burn, "%s %s capped at %d" % (name, mode, passes))
            assert got_info == info and info['passes'] == min(passes, full) and info['converged'] == (1 if passes > full else 0), (passes, got_info)
    finally:
        v.destroy()


# ---- the emitter -------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_within_volume_and_centreline(gpu_ctx, dtype):
    a = texels('blob', dtype)
    lo, hi = window(dtype)
    burn, info = statement('blob', 'ends')
    v = upload(gpu_ctx, a, 'nearest')
    k = v.skeleton(lo, hi)                                        # 'ends' by default
    v_format = v.modality['internalFormat']
    try:
        for k_lo, k_hi, fill in ((KEPT, None, 0), (1, None, 7), (2, 3, 0), (0, 0, 1), (3, KEPT - 1, 2)):
            out = k.within(k_lo, k_hi, fill)
            same(whole(out), burn_within_texels(a, burn, k_lo, k_hi, fill), "within %r" % ((k_lo, k_hi, fill),))
            assert out.modality['internalFormat'] == v_format
            out.destroy()
        out = k.volume()
        same(whole(out), skeleton_texels(a, lo, hi), "volume()")
        out.destroy()
        out = v.centreline(lo, hi, 'kernel')
        same(whole(out), skeleton_texels(a, lo, hi, 'kernel'), "centreline")
        out.destroy()
        v.destroy()                                               # the result owns what it needs
        out = k.within(info['passes'] - 1)
        same(whole(out), burn_within_texels(a, burn, info['passes'] - 1, None), "within after the source has gone")
        out.destroy()
    finally:
        k.close(); v.destroy()
    with pytest.raises(RuntimeError, match='destroyed'):
        k.burn()


# ---- the cull changes nothing, and does something; two runs ------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ('blob', 'noise', 'ball and line'))
def test_the_tile_cull_changes_no_byte(gpu_ctx, name, mode):
    a = texels(name, np.uint8)
    lo, hi = window(np.uint8)
    burn, info = statement(name, mode)
    v = upload(gpu_ctx, a)
    try:
        culled, every = v.skeleton(lo, hi, mode), v.skeleton(lo, hi, mode, _flags=1)
        got, got_every, visits, visits_every = culled.burn(), every.burn(), culled.profile()[2], every.profile()[2]
        assert culled.info == every.info == info
        culled.destroy(); every.destroy()
        same(got, burn, "%s %s" % (name, mode))
        assert got_every.tobytes() == got.tobytes()
        tiles = -(-a.shape[2] // 64) * -(-a.shape[1] // 8) * -(-a.shape[0] // 4)
        assert visits_every == 8 * tiles * info['passes'], (visits_every, tiles, info)
        assert visits <= visits_every
        if name == 'ball and line':                               # a condition: the cull has to do something
            assert info['passes'] >= 5 and visits < visits_every, (visits, visits_every)
    finally:
        v.destroy()


@pytest.mark.timeout(120)
def test_two_runs_give_identical_bytes(gpu_ctx):
    a = texels('noise', np.uint16)
    lo, hi = window(np.uint16)
    v = upload(gpu_ctx, a)
    first, second = v.skeleton(lo, hi, 'isthmus'), v.skeleton(lo, hi, 'isthmus')
    v.destroy()
    try:
        assert first.burn().tobytes() == second.burn().tobytes() == statement('noise', 'isthmus')[0].tobytes()
        assert first.info == second.info
    finally:
        first.destroy(); second.destroy()


# ---- composition ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_the_skeleton_cuts_a_thickness_channel_and_keeps_the_components(gpu_ctx):
    a = texels('blob', np.uint8)
    lo, hi = window(np.uint8)
    v = upload(gpu_ctx, a)
    centre = v.centreline(lo, hi)
    pair = v.thickness(lo, hi, 2)                                 # (code, local diameter)
    diameter = v.combine(pair, 'blend', 1, wa=0, wb=256)          # the second channel as a volume of its own
    along = diameter.mask(centre, lo, hi)                         # the diameter along the centreline, 0 elsewhere
    try:
        want_centre = skeleton_texels(a, lo, hi)
        want_diameter = combine_texels(a, thickness_texels(a, lo, hi, 2), 'blend', 1, wa=0, wb=256)
        want = combine_texels(want_diameter, want_centre, 'mask', lo=lo, hi=hi)
        same(whole(along), want, "the diameter along the centreline")
        assert len(np.unique(want)) >= 3, "degenerate input"
        # the branches can be labelled: the skeleton has the components of the range (26-connected)
        for name in ('blob', 'noise'):
            b = texels(name, np.uint8)
            vb = upload(gpu_ctx, b)
            kept = vb.centreline(lo, hi)
            found, source = kept.components(lo, hi, 26), vb.components(lo, hi, 26)
            try:
                assert found.info['listed'] == source.info['listed'] == len(components_texels(b, lo, hi, 26)[1]), name
                assert found.info['foreground_voxels'] == statement(name, 'ends')[1]['kept_voxels']
            finally:
                found.destroy(); source.destroy(); kept.destroy(); vb.destroy()
    finally:
        along.destroy(); diameter.destroy(); pair.destroy(); centre.destroy(); v.destroy()


@pytest.mark.timeout(120)
def test_python_rendering_context_applies_the_skeleton_option(gpu_ctx):
    from vpt_amd.readers import RAWReader
    a = texels('wye', np.uint8)
    d, h, w = a.shape
    for spec, want in (({'lo': 128, 'hi': 300}, skeleton_texels(a, 128, 255)),                                     # hi is open above
                       ({'lo': 128, 'hi': 239, 'mode': 'kernel', 'passes': 2, 'fill': 3}, skeleton_texels(a, 128, 239, 'kernel', 2, 3))):
        rc = vpt_amd.RenderingContext({'resolution': (72, 52), 'skeleton': spec})
        try:
            rc.setVolume(RAWReader(a, {'width': w, 'height': h, 'depth': d}))
            assert rc.volume.native_format()[0] == N.FORMAT_R8
            assert rc.volume.read_block(0, 0, 0, w, h, d).tobytes() == want.tobytes(), spec
            assert len(np.unique(want)) >= 3, "degenerate input"
        finally:
            rc.destroy()


# ---- errors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_error_returns(gpu_ctx):
    lib = N.lib()
    a = texels('wye', np.uint8)
    v = upload(gpu_ctx, a)
    pair = v.thickness(128, 255)
    k = v.skeleton(128, 255)
    h = C.c_void_p()
    out = np.zeros(a.shape, np.uint32)
    dst = out.ctypes.data_as(C.c_void_p)
    try:
        assert lib.vpt_volume_skeleton(None, 1, 2, 0, 0, C.byref(h)) == N.ERR_INVALID
        assert lib.vpt_volume_skeleton(v.texture, 1, 2, 0, 0, None) == N.ERR_INVALID
        assert lib.vpt_volume_skeleton(v.texture, 3, 2, 0, 0, C.byref(h)) == N.ERR_INVALID and b'lo exceeds hi' in lib.vpt_last_error()
        assert lib.vpt_volume_skeleton(v.texture, 1, 256, 0, 0, C.byref(h)) == N.ERR_INVALID and b'largest code' in lib.vpt_last_error()
        for mode in (-1, 3):
            assert lib.vpt_volume_skeleton(v.texture, 1, 2, mode, 0, C.byref(h)) == N.ERR_INVALID and b'mode' in lib.vpt_last_error()
        assert lib.vpt_volume_skeleton(v.texture, 1, 2, 0, -1, C.byref(h)) == N.ERR_INVALID and b'passes' in lib.vpt_last_error()
        assert lib.vpt_volume_skeleton(pair.texture, 1, 2, 0, 0, C.byref(h)) == N.ERR_UNSUPPORTED and b'RG8' in lib.vpt_last_error()
        for flags in (2, -1, 1 << 16):
            assert lib.vpt_volume_skeleton_capped(v.texture, 1, 2, 0, 0, flags, C.byref(h)) == N.ERR_INVALID and b'flags' in lib.vpt_last_error()
        assert not h.value
        info = N.SkeletonInfo()
        assert lib.vpt_skeleton_info(None, C.byref(info)) == N.ERR_INVALID and lib.vpt_skeleton_info(k._handle(), None) == N.ERR_INVALID
        ms, launches, tiles = (C.c_double * N.SKELETON_PHASES)(), C.c_uint64(0), C.c_uint64(0)
        assert lib.vpt_skeleton_profile(k._handle(), None, C.byref(launches), C.byref(tiles)) == N.ERR_INVALID
        assert lib.vpt_skeleton_profile(k._handle(), ms, None, C.byref(tiles)) == N.ERR_INVALID
        assert lib.vpt_skeleton_profile(k._handle(), ms, C.byref(launches), None) == N.ERR_INVALID
        assert lib.vpt_skeleton_destroy(None) == N.ERR_INVALID
        # bad boxes, as the siblings reject them
        d, hgt, w = a.shape
        for box in ((-1, 0, 0, 1, 1, 1), (0, 0, 0, w + 1, 1, 1), (0, 1, 0, w, hgt, d), (0, 0, 0, 0, 1, 1), (0, 0, d, 1, 1, 1)):
            assert lib.vpt_skeleton_burn(k._handle(), *box, dst, out.nbytes) == N.ERR_INVALID and b'outside volume' in lib.vpt_last_error(), box
        assert lib.vpt_skeleton_burn(k._handle(), 0, 0, 0, w, hgt, d, dst, out.nbytes - 1) == N.ERR_INVALID and b'too short' in lib.vpt_last_error()
        assert lib.vpt_skeleton_burn(k._handle(), 0, 0, 0, w, hgt, d, None, out.nbytes) == N.ERR_INVALID
        assert lib.vpt_skeleton_burn(None, 0, 0, 0, w, hgt, d, dst, out.nbytes) == N.ERR_INVALID
        # bad ranges and an oversized fill
        assert lib.vpt_skeleton_within(k._handle(), 5, 4, 0, C.byref(h)) == N.ERR_INVALID and b'from exceeds to' in lib.vpt_last_error()
        assert lib.vpt_skeleton_within(k._handle(), 1, 2, 256, C.byref(h)) == N.ERR_INVALID and b'fill 256' in lib.vpt_last_error()
        assert lib.vpt_skeleton_within(None, 1, 2, 0, C.byref(h)) == N.ERR_INVALID and lib.vpt_skeleton_within(k._handle(), 1, 2, 0, None) == N.ERR_INVALID
        assert not h.value
        for call in (lambda: v.skeleton(3, 2), lambda: v.skeleton(1, 256), lambda: v.skeleton(1, 2, 'curve'), lambda: v.skeleton(1, 2, 'ends', -1),
                     lambda: k.within(5, 4), lambda: k.within(1, None, 256), lambda: k.within(1.5)):
            with pytest.raises(ValueError):
                call()
        with pytest.raises(vpt_amd.VptError):
            pair.skeleton(1, 2)
    finally:
        k.destroy(); pair.destroy(); v.destroy()
