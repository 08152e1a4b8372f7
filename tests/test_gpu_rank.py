"""GPU: the median, erosion, dilation, opening and closing of a volume derived on the device (vpt_volume_rank).

The texels are held, byte for byte, to vpt_amd.rank_texels, the numpy statement of the contract (tests/test_rank_host.py holds that to a
restatement in Python integers and to the properties the contract implies).  Parity chain to the oracle: volumes uploaded from the host are
held to the CPU oracle by the rest of the suite, so a derived volume must give byte-identical buffers to the volume uploaded from the numpy
statement's texels.

Both kernels march a 128 x 8 x 32 column per workgroup (RK_TX, RK_TY, RK_TZ in vpt_volume_rank.hip) and have no stride loop, so the largest
shapes are the two that pass that tile by one voxel on every axis: (129, 9, 33), texel by texel, and (132, 9, 33), whole vectors."""
import ctypes as C

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.loaders import BlobLoader
from vpt_amd.rank import OPERATORS
from vpt_amd.readers import BVPReader, RAWReader
from vpt_amd.synthetic import sphere_volume, colour_tf

from test_gpu_readers import make_bvp_typed
from test_gpu_volume_formats import render, same, PACKED
from test_gpu_pyramid import upload, whole

pytestmark = pytest.mark.gpu

TILE = (128, 8, 32)                                                 # nx, ny, nz of a workgroup's column
NOISE = (23, 19, 21)                                                # nx, ny, nz: every axis odd
SHAPES = (NOISE, (1, 1, 1), (7, 5, 1), (17, 1, 3), (1, 3, 17),      # ... axes of one texel in every position
          (TILE[0] + 1, TILE[1] + 1, TILE[2] + 1),                  # one voxel past the tile on every axis, nx % 4 != 0
          (TILE[0] + 4, TILE[1] + 1, TILE[2] + 1))                  # the same with nx % 4 == 0: the vector form
DTYPES = (np.uint8, np.uint16)


def value_sets(dtype, shape, seed):
    """(name, [nz][ny][nx] texels): (a) uniform noise over every code, (b) heavy ties from {0, 1, M - 1, M}, (c) (uint16) codes that tell
    whole-code unsigned compares from byte-wise or signed ones"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    M = int(np.iinfo(dtype).max)
    sets = [('noise', rng.integers(0, M + 1, size=(nz, ny, nx)).astype(dtype)),
            ('ties', np.array([0, 1, M - 1, M], dtype)[rng.integers(0, 4, size=(nz, ny, nx))])]
    if dtype == np.uint16:
        sets.append(('bytes', np.array([0x00FF, 0x0100, 0x7FFF, 0x8000, 0xFF00], dtype)[rng.integers(0, 5, size=(nz, ny, nx))]))
    return sets


def differences(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d texels differ (%s), first at z, y, x = %s: %d, expected %d" % (len(bad), what, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- the texels themselves ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("op", OPERATORS)
def test_rank_texels_equal_the_contract(gpu_ctx, op, dtype):
    for n, shape in enumerate(SHAPES):
        for name, a in value_sets(dtype, shape, seed=31 + n):
            src = upload(gpu_ctx, a)
            for passes in (1, 2) + ((8,) if shape == NOISE and name == 'noise' else ()):
                want = vpt_amd.rank_texels(a, op, passes)
                if shape == NOISE and name == 'noise' and passes <= 2:      # a result that merely copies its source cannot pass
                    assert len(np.unique(want)) >= 16 and (want != a).mean() >= 0.5, "degenerate input"
                out = getattr(src, op)(passes)
                got = whole(out)
                out.destroy()
                differences(got, want, "%s %s %s %s, %d passes" % (op, np.dtype(dtype).name, shape, name, passes))
            assert whole(src).tobytes() == a.tobytes(), "the source's texels changed"
            src.destroy()


@pytest.mark.timeout(120)
def test_the_result_outlives_its_source_and_the_conveniences_are_rank(gpu_ctx):
    nx, ny, nz = NOISE
    a = value_sets(np.uint16, NOISE, seed=41)[0][1]
    for op in OPERATORS:
        src = upload(gpu_ctx, a)
        out = src.rank(op, 2)
        src.destroy()                                             # before the read-back
        assert out.ready and out.native_format()[0] == N.FORMAT_R16 and out.modality['dimensions'] == {'width': nx, 'height': ny, 'depth': nz}
        differences(whole(out), vpt_amd.rank_texels(a, op, 2), op)
        again = out.rank(op)                                      # ... and this entry again
        differences(whole(again), vpt_amd.rank_texels(vpt_amd.rank_texels(a, op, 2), op), op + ' again')
        again.destroy(); out.destroy()


@pytest.mark.timeout(120)
def test_result_does_not_depend_on_the_source_being_finalized(gpu_ctx):
    L = N.lib()
    for dtype, fmt in ((np.uint8, N.FORMAT_R8), (np.uint16, N.FORMAT_R16)):
        for nx in (32, 31):                                       # the vector form and the texel form
            a = value_sets(dtype, (nx, 4, 3), seed=43)[0][1]
            for op in (N.RANK_MEDIAN, N.RANK_CLOSE):
                h, out = C.c_void_p(), C.c_void_p()
                N.check(L.vpt_volume_create(gpu_ctx._h, nx, 4, 3, fmt, C.byref(h)))
                N.check(L.vpt_volume_upload_block(h, 0, 0, 0, nx, 4, 3, a.ctypes.data_as(C.c_void_p), a.nbytes))
                N.check(L.vpt_volume_rank(h, op, 1, C.byref(out)))          # no vpt_volume_finalize(h)
                got = np.empty_like(a)
                N.check(L.vpt_volume_read_block(out, 0, 0, 0, nx, 4, 3, got.ctypes.data_as(C.c_void_p), got.nbytes))
                L.vpt_volume_destroy(out); L.vpt_volume_destroy(h)
                differences(got, vpt_amd.rank_texels(a, OPERATORS[op]), "%s %d" % (OPERATORS[op], nx))


# ---- an ordinary volume ------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES)
def test_rank_then_smooth_then_gradient_equals_the_numpy_chain(gpu_ctx, dtype):
    a = value_sets(dtype, NOISE, seed=47)[0][1]
    src = upload(gpu_ctx, a)
    ranked = src.median(1)
    smoothed = ranked.smooth(1)
    pair = smoothed.derive_gradient('sobel', 1)
    tex = whole(pair)
    hist = ranked.histogram()
    for vol in (pair, smoothed, ranked, src):
        vol.destroy()
    value = vpt_amd.smooth_texels(vpt_amd.rank_texels(a, 'median'), 1)
    g = vpt_amd.gradient_magnitude(value, 'sobel', 1)
    assert len(np.unique(g)) >= 16
    assert tex[..., 0].tobytes() == value.tobytes() and tex[..., 1].tobytes() == g.tobytes()
    top = vpt_amd.rank_texels(a, 'median') >> (8 if dtype == np.uint16 else 0)
    assert hist.tolist() == np.bincount(top.reshape(-1), minlength=256).tolist()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("filt", ['linear', 'quasicubic'])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_derived_volume_renders_like_the_uploaded_texels(gpu_ctx, dtype, filt):
    nx, ny, nz = NOISE
    v = sphere_volume(0, noise=45.0, dims=(nz, ny, nx))
    rng = np.random.default_rng(53)
    v[rng.random(v.shape) < 0.03] = 255                           # impulses for the median to remove
    if dtype == np.uint16:
        v = v.astype(np.uint16) * 257
    tf = colour_tf(256)
    src = upload(gpu_ctx, v, filt)
    derived, want = src.median(1), vpt_amd.rank_texels(v, 'median')
    assert len(np.unique(want)) >= 32, "degenerate input: %d distinct values" % len(np.unique(want))
    twin = upload(gpu_ctx, want, filt)                            # `derived` carries src's filter
    for kind in ('mip', 'mcm'):
        fa = render(gpu_ctx, derived, kind, tf=tf)
        same(fa, render(gpu_ctx, twin, kind, tf=tf), '%s %s' % (kind, filt))
        pixels = np.ascontiguousarray(fa[-1]); pixels = pixels.reshape(-1, pixels.shape[-1])
        assert len(np.unique(pixels.view(np.uint16), axis=0)) >= 2, '%s: empty frame' % kind
        assert fa[-1].tobytes() != render(gpu_ctx, src, kind, tf=tf)[-1].tobytes(), '%s: the operation changes nothing' % kind
    for vol in (derived, twin, src):
        vol.destroy()


@pytest.mark.timeout(300)
def test_rendering_context_chain_equals_the_numpy_chain(monkeypatch):
    nx, ny, nz = NOISE
    v = (sphere_volume(0, noise=45.0, dims=(nz, ny, nx)).astype(np.int64) * 4000 // 255 - 1000).astype(np.int16)      # Hounsfield-like
    raw = lambda a, bits, signed: RAWReader(a.tobytes(), {'width': nx, 'height': ny, 'depth': nz, 'bits': bits, 'signed': signed})
    created, destroyed = [], []
    methods = {name: getattr(vpt_amd.Volume, name) for name in ('load', 'window', 'rank', 'smooth', 'reduce', 'derive_gradient', 'destroy')}

    def tracked(name):
        def call(self, *args, **kwargs):
            out = methods[name](self, *args, **kwargs)
            created.append((name, (self if name == 'load' else out).texture.value))
            return out
        return call
    for name in ('load', 'window', 'rank', 'smooth', 'reduce', 'derive_gradient'):
        monkeypatch.setattr(vpt_amd.Volume, name, tracked(name))

    def destroy(self):
        if self.texture:
            destroyed.append(self.texture.value)
        methods['destroy'](self)
    monkeypatch.setattr(vpt_amd.Volume, 'destroy', destroy)

    rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'window': [-200, 400], 'windowFormat': 'r16', 'rank': 'median', 'rankPasses': 2,
                                   'smooth': 1, 'reduce': 1, 'gradient': 'sobel', 'gradientGain': 2})
    try:
        assert rc.gl.getExtension('EXT_texture_norm16')
        rc.setVolume(raw(v.astype('<i2'), 16, True))
        assert rc.volume.native_format()[0] == N.FORMAT_RG16
        tex = whole(rc.volume)
        assert [name for name, _ in created] == ['load', 'window', 'rank', 'smooth', 'reduce', 'derive_gradient']      # the order of the chain
        handles = [hnd for _, hnd in created]
        assert rc.volume.texture.value == handles[-1]
        assert destroyed == handles[:-1], "an intermediate volume stays alive"      # each source is destroyed once the next volume exists
    finally:
        rc.destroy()
    wt = vpt_amd.window_texels(v, -200, 400, 16)
    value = vpt_amd.reduce_texels(vpt_amd.smooth_texels(vpt_amd.rank_texels(wt, 'median', 2), 1))
    g = vpt_amd.gradient_magnitude(value, 'sobel', 2)
    assert len(np.unique(g)) >= 32
    assert tex[..., 0].tobytes() == value.tobytes() and tex[..., 1].tobytes() == g.tobytes()
    assert value.tobytes() != vpt_amd.reduce_texels(vpt_amd.smooth_texels(wt, 1)).tobytes(), "the median changes nothing"
    # a volume that is not R8 / R16 is left as it is: R32F with `rank` set and no window
    f = np.random.default_rng(59).standard_normal((nz, ny, nx)).astype(np.float32)
    rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'rank': 'erode'})
    try:
        rc.setVolume(raw(f.astype('<f4'), 32, False))
        assert rc.volume.native_format()[0] == N.FORMAT_R32F and whole(rc.volume).tobytes() == f.tobytes()
    finally:
        rc.destroy()


# ---- errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_unsupported_sources_and_bad_arguments_raise(gpu_ctx):
    L = N.lib()
    words = np.random.default_rng(1).integers(0, 1 << 16, size=(4, 4, 4), dtype=np.uint64).astype(np.uint16)
    t, f, i, _ = PACKED[N.FORMAT_RGB565]
    packed = vpt_amd.Volume(gpu_ctx, BVPReader(BlobLoader(make_bvp_typed(words, f, i, t, ((), (), ()))))); packed.load()
    sources = ((packed, "RGB565"), (upload(gpu_ctx, np.zeros((4, 4, 4), np.float32)), "R32F"), (upload(gpu_ctx, np.zeros((4, 4, 4), np.int8)), "R8_SNORM"),
               (upload(gpu_ctx, np.zeros((4, 4, 4, 2), np.uint8)), "RG8"))
    for vol, name in sources:
        for op in ('median', 'open'):
            with pytest.raises(vpt_amd.VptError, match=r"\b%s\b" % name) as e:
                vol.rank(op)
            assert e.value.code == N.ERR_UNSUPPORTED
        vol.destroy()
    vol = upload(gpu_ctx, np.zeros((4, 4, 4), np.uint8))
    out = C.c_void_p()
    for passes in (0, 9):
        assert L.vpt_volume_rank(vol.texture, N.RANK_MEDIAN, passes, C.byref(out)) == N.ERR_INVALID
        assert str(passes).encode() in L.vpt_last_error()
        with pytest.raises(ValueError):
            vol.rank('median', passes)
    for op in (5, -1):
        assert L.vpt_volume_rank(vol.texture, op, 1, C.byref(out)) == N.ERR_INVALID
        assert str(op).encode() in L.vpt_last_error()
    with pytest.raises(ValueError):
        vol.rank('mean')
    assert L.vpt_volume_rank(vol.texture, N.RANK_MEDIAN, 1, None) == N.ERR_INVALID
    vol.destroy()
    for options in ({'rank': 'mean'}, {'rank': 'median', 'rankPasses': 0}, {'rank': 'median', 'rankPasses': 9}, {'rankPasses': True}):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext(options)
