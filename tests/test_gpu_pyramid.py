"""GPU: the next coarser level (vpt_volume_reduce) and the binomial smoothing (vpt_volume_smooth) derived on the device.

The texels are held, byte for byte, to vpt_amd.reduce_texels and vpt_amd.smooth_texels, the numpy statements of the contracts
(tests/test_pyramid_host.py holds those to scalar Python loops).  Parity chain to the oracle: volumes uploaded from the host are held to
the CPU oracle by the rest of the suite, so a derived volume must give byte-identical buffers to the volume uploaded from the numpy
statement's texels.

Neither kernel has a stride loop (k_reduce's grid is one lane per 16-byte chunk of the result, k_smooth's one workgroup per column
segment), so there is no wrap to exercise and the 10 M-voxel shape of the window tests is not used; MANY is the shape that takes more than
one workgroup along every axis of k_smooth's grid, and several of k_reduce's, instead."""
import ctypes as C

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.loaders import BlobLoader
from vpt_amd.readers import BVPReader, RAWReader
from vpt_amd.synthetic import sphere_volume, colour_tf

from test_gpu_readers import make_bvp_typed
from test_gpu_volume_formats import render, same, PACKED
from test_pyramid_host import INT_TYPES, int_texels, float_texels, same_floats

pytestmark = pytest.mark.gpu

DIMS = (23, 19, 21)                         # depth, height, width: every axis odd
# ... axes of one texel in every position; whole 16-byte vectors only (every dtype and channel count: 64 texels are 64 .. 512 bytes a row);
# one texel past a vector boundary
# ... one 32-byte vector pair a row at two bytes a texel and odd y and z: the vector form's clamps
SHAPES = (DIMS, (1, 1, 1), (1, 5, 7), (3, 1, 17), (17, 3, 1), (16, 16, 64), (4, 6, 33), (4, 6, 65), (3, 5, 16))
MANY = (35, 11, 160)                        # 160 = 5 x 32: the vector forms at every dtype; two smoothing tiles along x, y and z; odd y and z
MANY_ODD = (35, 11, 133)                    # the texel-by-texel forms over several workgroups


def upload(ctx, a, filt='linear'):
    if a.dtype == np.int8:
        return vpt_amd.Volume.from_array(ctx, a, filt, snorm=True)
    return vpt_amd.Volume.from_array(ctx, a, filt, norm16=a.dtype in (np.uint16, np.int16))


def whole(vol):
    m = vol.modality['dimensions']
    return vol.read_block(0, 0, 0, m['width'], m['height'], m['depth'])


def stored(a):
    """what the source's storage holds once finalized: SNORM's most negative code as the one above it"""
    return np.maximum(a, -np.iinfo(a.dtype).max) if a.dtype.kind == 'i' else a


def texels(dtype, dims, channels, seed=7):
    shape = tuple(dims) + ((2,) if channels == 2 else ())
    if dtype == np.float32:
        return float_texels(shape, seed)
    return int_texels(dtype, shape, seed)


def check_reduce(ctx, a):
    want = vpt_amd.reduce_texels(a)
    src = upload(ctx, a)
    out = src.reduce()
    got = whole(out)
    after = whole(src)
    src.destroy(); out.destroy()
    assert got.dtype == a.dtype and got.shape == want.shape, (got.shape, want.shape)
    if a.dtype == np.float32:
        if a.size >= 4096:
            finite = np.isfinite(want).mean()
            assert finite >= 0.9, "degenerate case: only %.3f of the result texels are finite" % finite
        assert same_floats(got, want), "%s %s: %d texels differ" % (a.dtype, a.shape, (got.view(np.uint32) != want.view(np.uint32)).sum())
        assert after.view(np.uint32).tobytes() == a.view(np.uint32).tobytes(), "the source's texels changed"
    else:
        bad = np.argwhere(got != want)
        assert len(bad) == 0, "%d texels differ (%s %s), first at %s: %d, expected %d" % (len(bad), a.dtype, a.shape, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
        assert after.tobytes() == stored(a).tobytes(), "the source's texels changed (%s)" % a.dtype


# ---- the texels themselves ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("dtype", INT_TYPES + (np.float32,))
def test_reduced_texels_equal_the_contract(gpu_ctx, dtype, channels):
    for dims in SHAPES + (MANY, MANY_ODD):
        a = texels(dtype, dims, channels)
        if a.dtype.kind == 'i' and a.size >= 8:
            a.reshape(-1)[:8] = np.iinfo(dtype).min               # a cell of the most negative code
        check_reduce(gpu_ctx, a)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_smoothed_texels_equal_the_contract(gpu_ctx, dtype):
    for dims in SHAPES + (MANY, MANY_ODD):
        a = int_texels(dtype, dims, seed=11)                      # uniform noise over every code
        src = upload(gpu_ctx, a)
        wants, cur = {}, a
        for passes in range(1, 9):                                # p passes are p applications of one pass
            cur = vpt_amd.smooth_texels(cur, 1)
            wants[passes] = cur
        assert wants[2].tobytes() == vpt_amd.smooth_texels(a, 2).tobytes()
        for passes in (1, 2, 8):
            want = wants[passes]
            out = src.smooth(passes)
            got = whole(out)
            out.destroy()
            assert got.dtype == a.dtype and got.shape == a.shape
            bad = np.argwhere(got != want)
            assert len(bad) == 0, "%d texels differ (%s %s, %d passes), first at z, y, x = %s: %d, expected %d" % (
                len(bad), a.dtype, a.shape, passes, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
            if a.size >= 64:
                assert (got != a).mean() >= 0.5, "the smoothing changes fewer than half of the texels"
        assert whole(src).tobytes() == a.tobytes(), "the source's texels changed"
        src.destroy()


@pytest.mark.timeout(120)
def test_levels(gpu_ctx):
    a = int_texels(np.uint16, (37, 50, 45), seed=13)
    src = upload(gpu_ctx, a)
    out = src.reduce(3)
    want = vpt_amd.reduce_texels(vpt_amd.reduce_texels(vpt_amd.reduce_texels(a)))
    assert want.shape == (5, 7, 6) and out.modality['dimensions'] == {'width': 6, 'height': 7, 'depth': 5}
    assert whole(out).tobytes() == want.tobytes()
    assert out.native_format()[0] == N.FORMAT_R16 and out.ready
    out.destroy(); src.destroy()
    b = int_texels(np.int8, (5, 6, 7), seed=17)
    src = upload(gpu_ctx, b)
    out = src.reduce(10)                                          # stops once every axis is 1
    assert out.modality['dimensions'] == {'width': 1, 'height': 1, 'depth': 1}
    want = b
    for _ in range(3):
        want = vpt_amd.reduce_texels(want)
    assert want.shape == (1, 1, 1) and whole(out).tobytes() == want.tobytes()
    one = out.reduce(2)                                           # a volume of one texel: a copy
    assert whole(one).tobytes() == want.tobytes()
    for vol in (one, out, src):
        vol.destroy()
    for bad in (0, -1, 1.5, '1', True):
        src = upload(gpu_ctx, b)
        with pytest.raises(ValueError):
            src.reduce(bad)
        src.destroy()


@pytest.mark.timeout(120)
def test_result_does_not_depend_on_the_source_being_finalized(gpu_ctx):
    """a source that was never finalized still holds SNORM's most negative code: the reduction reads it as the one above it itself"""
    L = N.lib()
    for dtype, fmt in ((np.int8, N.FORMAT_R8_SNORM), (np.int16, N.FORMAT_R16_SNORM)):
        info = np.iinfo(dtype)
        a = np.full((2, 4, 32), info.min, dtype)
        a[:, :, 5] = 3
        for w in (32, 31):                                        # the vector form and the texel form
            b = np.ascontiguousarray(a[:, :, :w])
            h, out = C.c_void_p(), C.c_void_p()
            N.check(L.vpt_volume_create(gpu_ctx._h, w, 4, 2, fmt, C.byref(h)))
            N.check(L.vpt_volume_upload_block(h, 0, 0, 0, w, 4, 2, b.ctypes.data_as(C.c_void_p), b.nbytes))
            N.check(L.vpt_volume_reduce(h, C.byref(out)))
            got = np.empty((1, 2, 16), dtype)
            N.check(L.vpt_volume_read_block(out, 0, 0, 0, 16, 2, 1, got.ctypes.data_as(C.c_void_p), got.nbytes))
            assert got.tobytes() == vpt_amd.reduce_texels(b).tobytes() and got[0, 0, 0] == info.min + 1
            L.vpt_volume_destroy(out); L.vpt_volume_destroy(h)


# ---- parity chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("filt", ['linear', 'quasicubic'])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_derived_volumes_render_like_the_uploaded_texels(gpu_ctx, dtype, filt):
    v = sphere_volume(0, noise=45.0, dims=DIMS)
    if dtype == np.uint16:
        v = (v.astype(np.uint16) * 257)
    tf = colour_tf(256)
    src = upload(gpu_ctx, v, filt)
    for derived, want in ((src.reduce(), vpt_amd.reduce_texels(v)), (src.smooth(2), vpt_amd.smooth_texels(v, 2))):
        assert len(np.unique(want)) >= 32, "degenerate input: %d distinct values" % len(np.unique(want))
        twin = upload(gpu_ctx, want, filt)                        # `derived` carries src's filter
        for kind in ('mip', 'mcm'):
            fa = render(gpu_ctx, derived, kind, tf=tf)
            same(fa, render(gpu_ctx, twin, kind, tf=tf), '%s %s %s' % (kind, filt, want.shape))
            pixels = np.ascontiguousarray(fa[-1]); pixels = pixels.reshape(-1, pixels.shape[-1])
            assert len(np.unique(pixels.view(np.uint16), axis=0)) >= 2, '%s: empty frame' % kind
            assert fa[-1].tobytes() != render(gpu_ctx, src, kind, tf=tf)[-1].tobytes(), '%s: the operation changes nothing' % kind
        derived.destroy(); twin.destroy()
    src.destroy()


@pytest.mark.timeout(300)
def test_rendering_context_chain_equals_the_numpy_chain(monkeypatch):
    d, h, w = DIMS
    v = (sphere_volume(0, noise=45.0, dims=DIMS).astype(np.int64) * 4000 // 255 - 1000).astype(np.int16)      # Hounsfield-like
    created, destroyed = [], []
    methods = {name: getattr(vpt_amd.Volume, name) for name in ('load', 'window', 'smooth', 'reduce', 'derive_gradient', 'destroy')}

    def tracked(name):
        def call(self, *args, **kwargs):
            out = methods[name](self, *args, **kwargs)
            made = self if name == 'load' else out
            created.append((name, made.texture.value))
            return out
        return call
    for name in ('load', 'window', 'smooth', 'reduce', 'derive_gradient'):
        monkeypatch.setattr(vpt_amd.Volume, name, tracked(name))

    def destroy(self):
        if self.texture:
            destroyed.append(self.texture.value)
        methods['destroy'](self)
    monkeypatch.setattr(vpt_amd.Volume, 'destroy', destroy)

    rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'window': [-200, 400], 'windowFormat': 'r16', 'smooth': 2, 'reduce': 1,
                                   'gradient': 'sobel', 'gradientGain': 2})
    try:
        assert rc.gl.getExtension('EXT_texture_norm16')
        rc.setVolume(RAWReader(v.astype('<i2').tobytes(), {'width': w, 'height': h, 'depth': d, 'bits': 16, 'signed': True}))
        assert rc.volume.native_format()[0] == N.FORMAT_RG16
        tex = whole(rc.volume)
        assert [name for name, _ in created] == ['load', 'window', 'smooth', 'reduce', 'derive_gradient']      # the order of the chain
        handles = [hnd for _, hnd in created]
        assert rc.volume.texture.value == handles[-1]
        assert destroyed == handles[:-1], "an intermediate volume stays alive"      # each source is destroyed once the next volume exists
        rc.chooseRenderer('eam'); rc.chooseToneMapper('artistic')
        rc.renderer.setTransferFunction(colour_tf(64, 48))
        rc.render()
        assert len(set(rc.getFrame().tobytes())) > 8
    finally:
        rc.destroy()
    wt = vpt_amd.window_texels(v, -200, 400, 16)
    value = vpt_amd.reduce_texels(vpt_amd.smooth_texels(wt, 2))
    g = vpt_amd.gradient_magnitude(value, 'sobel', 2)
    assert len(np.unique(g)) >= 32
    assert tex.shape == (12, 10, 11, 2) and tex[..., 0].tobytes() == value.tobytes() and tex[..., 1].tobytes() == g.tobytes()
    # the options absent, None or 0: the volume as it is; smooth leaves a volume that is not R8 / R16 alone, reduce takes it
    for options, fmt, want in (({}, N.FORMAT_R16_SNORM, v), ({'smooth': None, 'reduce': 0}, N.FORMAT_R16_SNORM, v),
                               ({'smooth': 3}, N.FORMAT_R16_SNORM, v), ({'smooth': 3, 'reduce': 2}, N.FORMAT_R16_SNORM, vpt_amd.reduce_texels(vpt_amd.reduce_texels(v)))):
        rc = vpt_amd.RenderingContext(dict({'resolution': (72, 56)}, **options))
        try:
            rc.gl.getExtension('EXT_texture_norm16')
            rc.setVolume(RAWReader(v.astype('<i2').tobytes(), {'width': w, 'height': h, 'depth': d, 'bits': 16, 'signed': True}))
            assert rc.volume.native_format()[0] == fmt and whole(rc.volume).tobytes() == want.tobytes(), options
        finally:
            rc.destroy()


# ---- errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_unsupported_sources_and_bad_arguments_raise(gpu_ctx):
    L = N.lib()
    words = np.random.default_rng(1).integers(0, 1 << 16, size=(4, 4, 4), dtype=np.uint64).astype(np.uint16)
    t, f, i, _ = PACKED[N.FORMAT_RGB565]
    packed = vpt_amd.Volume(gpu_ctx, BVPReader(BlobLoader(make_bvp_typed(words, f, i, t, ((), (), ()))))); packed.load()
    with pytest.raises(vpt_amd.VptError, match=r"\bRGB565\b") as e:
        packed.reduce()
    assert e.value.code == N.ERR_UNSUPPORTED
    sources = ((packed, "RGB565"), (upload(gpu_ctx, np.zeros((4, 4, 4), np.float32)), "R32F"), (upload(gpu_ctx, np.zeros((4, 4, 4), np.int8)), "R8_SNORM"),
               (upload(gpu_ctx, np.zeros((4, 4, 4), np.int16)), "R16_SNORM"), (upload(gpu_ctx, np.zeros((4, 4, 4, 2), np.uint8)), "RG8"),
               (upload(gpu_ctx, np.zeros((4, 4, 4, 2), np.uint16)), "RG16"))
    for vol, name in sources:
        with pytest.raises(vpt_amd.VptError, match=r"\b%s\b" % name) as e:
            vol.smooth(1)
        assert e.value.code == N.ERR_UNSUPPORTED
        vol.destroy()
    vol = upload(gpu_ctx, np.zeros((4, 4, 4), np.uint8))
    out = C.c_void_p()
    for passes in (0, 9, -1):
        assert L.vpt_volume_smooth(vol.texture, passes, C.byref(out)) == N.ERR_INVALID
        assert str(passes).encode() in L.vpt_last_error()
        with pytest.raises(ValueError):
            vol.smooth(passes)
    assert L.vpt_volume_smooth(vol.texture, 1, None) == N.ERR_INVALID and L.vpt_volume_reduce(vol.texture, None) == N.ERR_INVALID
    vol.destroy()
