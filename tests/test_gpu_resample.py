"""GPU: a volume resampled to any grid size on the device (vpt_volume_resample).

The texels are held, byte for byte, to vpt_amd.resample_texels, the numpy statement of the contract (tests/test_resample_host.py holds that
to scalar Python loops over Python integers).  Parity chain to the oracle: volumes uploaded from the host are held to the CPU oracle by the
rest of the suite, so a derived volume must give byte-identical buffers to the volume uploaded from the numpy statement's texels.

Shapes are (depth, height, width).  The cases are the smallest at which each path of the kernels is taken: every clamp, the identity, a
halving (equal to vpt_volume_reduce), non-integer shrinking and growth, all three in one call, axes of one texel, rows longer than a wave
and no multiple of 64, the longest row (RG16: the 16 KiB of LDS a row may take), many workgroups along every axis of both passes, and the
divisor 2^34 that neither 32 bits nor a float reciprocal hold."""
import ctypes as C
import functools

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.loaders import BlobLoader
from vpt_amd.readers import BVPReader, RAWReader
from vpt_amd.resample import count_ties, isotropic_shape, resample_texels
from vpt_amd.synthetic import sphere_volume, colour_tf

from test_gpu_readers import make_bvp_typed
from test_gpu_volume_formats import render, same, PACKED
from test_pyramid_host import int_texels, float_texels, same_floats

pytestmark = pytest.mark.gpu

DIMS = (23, 19, 21)
HALVING = ((16, 16, 64), (8, 8, 32))
DOUBLING = ((7, 5, 4), (14, 10, 8))
FILTERED_CASES = (
    ((1, 1, 1), (1, 1, 1)), ((1, 1, 1), (3, 2, 5)),               # every clamp
    (DIMS, DIMS),                                                 # identity
    HALVING,                                                      # also equal to src.reduce()
    (DIMS, (7, 5, 4)),                                            # non-integer shrink, taps straddle cells
    ((7, 5, 4), DIMS),                                            # non-integer growth
    DOUBLING,                                                     # exact halves where the axis doubles
    (DIMS, (9, 40, 21)),                                          # shrink, grow and identity in one call
    ((1, 5, 7), (4, 1, 9)), ((3, 1, 17), (1, 6, 2)),              # an axis of 1, as source and as target
    ((2, 3, 133), (2, 3, 300)), ((2, 3, 300), (2, 3, 133)),       # rows longer than a wave, not a multiple of 64
    ((2, 2, 4096), (2, 2, 5)), ((2, 2, 5), (2, 2, 4096)),         # the longest row
    ((35, 11, 160), (20, 30, 333)),                               # many workgroups along every axis of both passes
)
NEAREST_CASES = ((DIMS, (7, 40, 21)), (DIMS, DIMS), ((2, 3, 133), (2, 3, 300)))


def upload(ctx, a, filt='linear'):
    if a.dtype == np.int8:
        return vpt_amd.Volume.from_array(ctx, a, filt, snorm=True)
    return vpt_amd.Volume.from_array(ctx, a, filt, norm16=a.dtype in (np.uint16, np.int16))


def whole(vol):
    m = vol.modality['dimensions']
    return vol.read_block(0, 0, 0, m['width'], m['height'], m['depth'])


def resampled(vol, shape, mode='filtered'):
    d, h, w = shape
    return vol.resample(w, h, d, mode)


@functools.lru_cache(maxsize=None)
def noise(dtype, shape, channels, seed=7):
    """uniform noise over every code; shared among the tests and left unchanged"""
    a = int_texels(dtype, tuple(shape) + ((2,) if channels == 2 else ()), seed)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected(dtype, source, target, channels):
    want = resample_texels(noise(dtype, source, channels), target)
    want.setflags(write=False)
    return want


def differences(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: %d of %d texels differ, first at %s: %d, expected %d" % (what, len(bad), want.size, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- FILTERED ----------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_filtered_texels_equal_the_contract(gpu_ctx, dtype, channels):
    for source, target in FILTERED_CASES:
        a = noise(dtype, source, channels)
        src = upload(gpu_ctx, a)
        out = resampled(src, target)
        got = whole(out)
        d, h, w = target
        assert out.modality['dimensions'] == {'width': w, 'height': h, 'depth': d} and out.ready
        assert out.native_format()[0] == src.native_format()[0]
        differences(got, expected(dtype, source, target, channels), '%s x%d %s -> %s' % (np.dtype(dtype).name, channels, source, target))
        if (source, target) == HALVING:
            reduced = src.reduce()
            assert whole(reduced).tobytes() == got.tobytes(), "halving an all-even volume differs from reduce()"
            reduced.destroy()
        if source == target:
            assert got.tobytes() == a.tobytes()
        assert whole(src).tobytes() == a.tobytes(), "the source's texels changed"
        again = resampled(src, target)
        assert whole(again).tobytes() == got.tobytes(), "two calls give different bytes"
        again.destroy(); out.destroy(); src.destroy()


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_the_inputs_contain_exact_halves(dtype):
    """a condition on the input (checked on the CPU as well): the rounding rule decides some texels of the halving and the doubling case"""
    for source, target in (HALVING, DOUBLING):
        for channels in (1, 2):
            assert count_ties(noise(dtype, source, channels), target) >= 1, (dtype, source, target, channels)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_wide_divisor(gpu_ctx, dtype):
    """S = 2048 * 4096 * 2048 = 2^34: 8 Mi source voxels, 8 Ki result voxels of 4096 taps each"""
    source, target = (2048, 2, 2048), (1, 2048, 4)
    a = noise(dtype, source, 1, seed=19)
    src = upload(gpu_ctx, a)
    out = resampled(src, target)
    got = whole(out)
    out.destroy(); src.destroy()
    want = resample_texels(a, target)
    assert len(np.unique(want)) >= 2, "degenerate input"          # (means of 2 Mi noise texels: they lie on both sides of a rounding boundary)
    differences(got, want, '%s wide divisor' % np.dtype(dtype).name)


# ---- NEAREST -----------------------------------------------------------------------------------------------------------------
def stored(a):
    """what the source's storage holds once finalized: SNORM's most negative code as the one above it"""
    return np.maximum(a, -np.iinfo(a.dtype).max) if a.dtype.kind == 'i' else a


@pytest.mark.timeout(300)
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int8, np.int16, np.float32])
def test_nearest_texels_are_copied_bits(gpu_ctx, dtype, channels):
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32}[np.dtype(dtype).itemsize]
    for source, target in NEAREST_CASES:
        shape = tuple(source) + ((2,) if channels == 2 else ())
        a = float_texels(shape, seed=23) if dtype == np.float32 else int_texels(dtype, shape, seed=23)
        if dtype == np.float32:
            a.reshape(-1).view(np.uint32)[:3] = (0x7FC12345, 0xFF800001, 0x80000000)      # NaN payloads, -0
            assert np.isnan(a).sum() >= 2 and np.isinf(a).sum() >= 1
        src = upload(gpu_ctx, a)
        out = resampled(src, target, 'nearest')
        got = whole(out)
        want = resample_texels(stored(a), target, 'nearest')
        assert got.dtype == want.dtype and got.shape == want.shape
        assert got.view(bits).tobytes() == want.view(bits).tobytes(), (dtype, channels, source, target)
        if source == target:
            assert got.view(bits).tobytes() == stored(a).view(bits).tobytes()
        assert whole(src).view(bits).tobytes() == stored(a).view(bits).tobytes(), "the source's texels changed"
        again = resampled(src, target, 'nearest')
        assert whole(again).view(bits).tobytes() == got.view(bits).tobytes(), "two calls give different bytes"
        again.destroy(); out.destroy(); src.destroy()


# ---- errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_unsupported_sources_and_bad_arguments(gpu_ctx):
    L = N.lib()
    words = np.random.default_rng(1).integers(0, 1 << 16, size=(4, 4, 4), dtype=np.uint64).astype(np.uint16)
    t, f, i, _ = PACKED[N.FORMAT_RGB565]
    packed = vpt_amd.Volume(gpu_ctx, BVPReader(BlobLoader(make_bvp_typed(words, f, i, t, ((), (), ()))))); packed.load()
    for mode in ('nearest', 'filtered'):
        with pytest.raises(vpt_amd.VptError, match=r"\bRGB565\b") as e:
            packed.resample(2, 2, 2, mode)
        assert e.value.code == N.ERR_UNSUPPORTED
    packed.destroy()
    for a, name in ((np.zeros((4, 4, 4), np.float32), "R32F"), (np.zeros((4, 4, 4), np.int8), "R8_SNORM"), (np.zeros((4, 4, 4, 2), np.int16), "RG16_SNORM")):
        vol = upload(gpu_ctx, a)
        with pytest.raises(vpt_amd.VptError, match=r"\b%s\b" % name) as e:
            vol.resample(2, 2, 2)
        assert e.value.code == N.ERR_UNSUPPORTED
        vol.resample(2, 2, 2, 'nearest').destroy()
        vol.destroy()
    vol = upload(gpu_ctx, np.zeros((4, 4, 4), np.uint8))
    out = C.c_void_p()
    for size in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (4097, 4, 4), (4, 4097, 4), (4, 4, 4097), (-1, 4, 4)):
        for mode in (N.RESAMPLE_NEAREST, N.RESAMPLE_FILTERED):
            assert L.vpt_volume_resample(vol.texture, size[0], size[1], size[2], mode, C.byref(out)) == N.ERR_INVALID, size
        with pytest.raises(ValueError):
            vol.resample(*size)
    for mode in (2, -1, 7):
        assert L.vpt_volume_resample(vol.texture, 4, 4, 4, mode, C.byref(out)) == N.ERR_INVALID
        assert b"mode" in L.vpt_last_error()
    with pytest.raises(ValueError, match='mode'):
        vol.resample(4, 4, 4, 'linear')
    assert L.vpt_volume_resample(vol.texture, 4, 4, 4, N.RESAMPLE_FILTERED, None) == N.ERR_INVALID
    assert L.vpt_volume_resample(None, 4, 4, 4, N.RESAMPLE_FILTERED, C.byref(out)) == N.ERR_INVALID
    vol.destroy()


# ---- parity chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype,channels,filt", [(np.uint8, 1, 'linear'), (np.uint16, 2, 'nearest')])
def test_derived_volumes_render_like_the_uploaded_texels(gpu_ctx, dtype, channels, filt):
    v = sphere_volume(0, noise=45.0, dims=DIMS)
    if dtype == np.uint16:
        v = v.astype(np.uint16) * 257
    if channels == 2:
        v = np.ascontiguousarray(np.stack([v, vpt_amd.gradient_magnitude(v, 'central', 2)], axis=-1))
    tf = colour_tf(256) if channels == 1 else colour_tf(64, 48)
    target = (17, 30, 26)
    want = resample_texels(v, target)
    assert len(np.unique(want)) >= 32, "degenerate input"
    src = upload(gpu_ctx, v, filt)
    derived = resampled(src, target)
    twin = upload(gpu_ctx, want, filt)                            # `derived` carries src's filter
    for kind in ('mip', 'mcm'):
        fa = render(gpu_ctx, derived, kind, tf=tf)
        same(fa, render(gpu_ctx, twin, kind, tf=tf), '%s %s' % (kind, filt))
        pixels = np.ascontiguousarray(fa[-1]); pixels = pixels.reshape(-1, pixels.shape[-1])
        assert len(np.unique(pixels.view(np.uint16), axis=0)) >= 2, '%s: empty frame' % kind
        assert fa[-1].tobytes() != render(gpu_ctx, src, kind, tf=tf)[-1].tobytes(), '%s: the operation changes nothing' % kind
    derived.destroy(); twin.destroy(); src.destroy()


# ---- the chain downstream ----------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_every_volume_operation_takes_the_result(gpu_ctx, dtype):
    from vpt_amd.distance import distance_squared_texels
    v = sphere_volume(0, noise=45.0, dims=DIMS)
    scale = 1
    if dtype == np.uint16:
        v, scale = v.astype(np.uint16) * 257, 257
    lo, hi = 110 * scale, 255 * scale
    src = upload(gpu_ctx, v)
    steps = [resampled(src, (23, 19, 60))]
    wants = [resample_texels(v, (23, 19, 60))]
    steps.append(steps[-1].rank('median'))
    wants.append(vpt_amd.rank_texels(wants[-1], 'median'))
    found = steps[-1].components(lo, hi)
    steps.append(found.keep(1, 2))
    found.destroy()
    wants.append(vpt_amd.keep_texels(wants[-1], vpt_amd.components_texels(wants[-1], lo, hi)[0], 1, 2))
    dist = steps[-1].distance(lo, hi)
    steps.append(dist.within(0, 9))
    dist.destroy()
    wants.append(vpt_amd.within_texels(wants[-1], distance_squared_texels(wants[-1], lo, hi), 0, 9))
    steps.append(steps[-1].smooth(1))
    wants.append(vpt_amd.smooth_texels(wants[-1], 1))
    last = steps[-1].derive_gradient('central')
    g = vpt_amd.gradient_magnitude(wants[-1], 'central')
    for name, vol, want in zip(('resample', 'rank', 'keep', 'within', 'smooth'), steps, wants):
        assert len(np.unique(want)) >= 8, "degenerate input at %s" % name
        differences(whole(vol), want, name)
    tex = whole(last)
    assert tex[..., 0].tobytes() == wants[-1].tobytes() and tex[..., 1].tobytes() == g.tobytes() and len(np.unique(g)) >= 8
    # the operation takes its own result, and a label volume in NEAREST
    back = resampled(steps[0], DIMS)
    differences(whole(back), resample_texels(wants[0], DIMS), 'resample of a resampled volume')
    grown = resampled(last, (30, 19, 21), 'nearest')
    assert whole(grown).tobytes() == resample_texels(tex, (30, 19, 21), 'nearest').tobytes()
    for vol in steps + [last, back, grown, src]:
        vol.destroy()


@pytest.mark.timeout(300)
def test_rendering_context_chain_equals_the_numpy_chain():
    d, h, w = DIMS
    v = (sphere_volume(0, noise=45.0, dims=DIMS).astype(np.int64) * 4000 // 255 - 1000).astype(np.int16)      # Hounsfield-like
    spacing = (0.7, 0.7, 1.6)
    rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'window': [-200, 400], 'windowFormat': 'r16', 'resample': {'spacing': spacing},
                                   'rank': 'median', 'smooth': 1, 'gradient': 'sobel', 'gradientGain': 2})
    try:
        assert rc.gl.getExtension('EXT_texture_norm16')
        rc.setVolume(RAWReader(v.astype('<i2').tobytes(), {'width': w, 'height': h, 'depth': d, 'bits': 16, 'signed': True}))
        assert rc.volume.native_format()[0] == N.FORMAT_RG16
        tex = whole(rc.volume)
        rc.chooseRenderer('eam'); rc.chooseToneMapper('artistic')
        rc.renderer.setTransferFunction(colour_tf(64, 48))
        rc.render()
        assert len(set(rc.getFrame().tobytes())) > 8
    finally:
        rc.destroy()
    nx, ny, nz = isotropic_shape((w, h, d), spacing)
    assert (nx, ny, nz) == (21, 19, 53)
    value = vpt_amd.window_texels(v, -200, 400, 16)
    value = resample_texels(value, (nz, ny, nx))
    value = vpt_amd.smooth_texels(vpt_amd.rank_texels(value, 'median'), 1)
    g = vpt_amd.gradient_magnitude(value, 'sobel', 2)
    assert len(np.unique(g)) >= 32
    assert tex.shape == (nz, ny, nx, 2) and tex[..., 0].tobytes() == value.tobytes() and tex[..., 1].tobytes() == g.tobytes()
    # 'size' and 'nearest'; a format the mode does not take is left as it is
    for options, want in (({'resample': {'size': [9, 40, 21]}}, v), ({'resample': {'size': [9, 40, 21], 'mode': 'nearest'}}, resample_texels(v, (21, 40, 9), 'nearest')),
                          ({'resample': None}, v)):
        rc = vpt_amd.RenderingContext(dict({'resolution': (72, 56)}, **options))
        try:
            rc.gl.getExtension('EXT_texture_norm16')
            rc.setVolume(RAWReader(v.astype('<i2').tobytes(), {'width': w, 'height': h, 'depth': d, 'bits': 16, 'signed': True}))
            assert rc.volume.native_format()[0] == N.FORMAT_R16_SNORM and whole(rc.volume).tobytes() == want.tobytes(), options
        finally:
            rc.destroy()
