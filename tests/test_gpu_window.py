"""GPU: the value-range window derived on the device (vpt_volume_window), the range (vpt_volume_range) and the full-resolution code
histogram (vpt_volume_code_histogram).

The windowed texels are held, byte for byte, to vpt_amd.window_texels, the numpy statement of the two contracts (tests/test_window_host.py
holds that to scalar Python loops).  Parity chain to the oracle: R8 / R16 volumes uploaded from the host are held to the CPU oracle by the
rest of the suite, so a windowed volume must give byte-identical buffers to the volume uploaded from window_texels(...) in every renderer
and under every filter."""
import ctypes as C

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd import readers as R
from vpt_amd.loaders import BlobLoader
from vpt_amd.readers import BVPReader, RAWReader
from vpt_amd.synthetic import sphere_volume, colour_tf, GoldenRatioRng

from test_gpu_readers import make_bvp_typed
from test_gpu_volume_formats import render, same, CLASSES, PACKED
from test_window_host import INSIDE, INT_TYPES, int_windows, float_cases

pytestmark = pytest.mark.gpu

DIMS = (23, 19, 21)                         # depth, height, width: odd, nx % 4 != 0, 9177 voxels: a tail of 9 behind the 16-voxel groups
# ... a single slice; one voxel; a one-voxel axis in the middle; whole 16-voxel groups only (no tail)
SHAPES = (DIMS, (1, 5, 7), (1, 1, 1), (3, 1, 17), (17, 3, 1), (16, 16, 16))
WRAP = (160, 256, 256)                      # 10.5 M voxels: more than 2048 workgroups x 256 lanes x 16 voxels, the grid's stride loop wraps
FILTERS = ('linear', 'nearest', 'quasicubic')
TYPES = INT_TYPES + (np.float32,)
OUT_DTYPE = {8: np.uint8, 16: np.uint16}


def texels(dtype, dims, seed=7):
    """random texels of which most fall strictly inside the type's INSIDE window (floats: standard normal, window [-1, 1])"""
    rng = np.random.default_rng(seed)
    if dtype == np.float32:
        return rng.standard_normal(dims).astype(np.float32)
    a, b = INSIDE[dtype][0]
    return rng.integers(a, b, size=dims).astype(dtype)


def inside_window(dtype):
    return (-1.0, 1.0) if dtype == np.float32 else INSIDE[dtype][1]


def upload(ctx, a, filt='linear'):
    if a.dtype == np.int8:
        return vpt_amd.Volume.from_array(ctx, a, filt, snorm=True)
    return vpt_amd.Volume.from_array(ctx, a, filt, norm16=a.dtype in (np.uint16, np.int16))


def whole(vol, dims):
    d, h, w = dims
    return vol.read_block(0, 0, 0, w, h, d)


def stored(a):
    """what the source's storage holds once finalized: SNORM's most negative code as the one above it"""
    return np.maximum(a, -np.iinfo(a.dtype).max) if a.dtype.kind == 'i' else a


def check_window(ctx, a, lo, hi, bits, min_inside=0.0):
    want = vpt_amd.window_texels(a, lo, hi, bits)
    M = (1 << bits) - 1
    if min_inside:
        share = ((want > 0) & (want < M)).mean()
        assert share >= min_inside, "degenerate case: %.3f of the texels strictly inside the window" % share
    src = upload(ctx, a)
    out = src.window(lo, hi, 'r%d' % bits)
    got = whole(out, a.shape)
    after = whole(src, a.shape)
    src.destroy(); out.destroy()
    assert got.dtype == OUT_DTYPE[bits] and got.shape == a.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d texels differ (%s %s -> r%d, window [%r, %r]), first at z, y, x = %s: source %r gives %d, expected %d" % (
        len(bad), a.dtype, a.shape, bits, lo, hi, bad[0], a[tuple(bad[0])], got[tuple(bad[0])], want[tuple(bad[0])])
    assert after.tobytes() == stored(a).tobytes(), "the source's texels changed (%s)" % a.dtype


# ---- the texels themselves ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("dtype", TYPES)
def test_windowed_texels_equal_the_contract(gpu_ctx, dtype, bits):
    lo, hi = inside_window(dtype)
    for dims in SHAPES:
        check_window(gpu_ctx, texels(dtype, dims), lo, hi, bits, min_inside=0.5 if np.prod(dims) >= 64 else 0.0)
    check_window(gpu_ctx, texels(dtype, WRAP), lo, hi, bits, min_inside=0.5)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("dtype", INT_TYPES)
def test_integer_edge_windows_over_every_code(gpu_ctx, dtype, bits):
    info = np.iinfo(dtype)
    every = np.resize(np.arange(info.min, info.max + 1).astype(dtype), 5 * 33 * 399).reshape(5, 33, 399)      # every code, a tail of 11
    assert len(np.unique(every)) == info.max - info.min + 1
    for lo, hi in int_windows(dtype):
        check_window(gpu_ctx, every, lo, hi, bits)
    rng = np.random.default_rng(5)
    for _ in range(12):
        lo = int(rng.integers(info.min - 300, info.max + 300))
        check_window(gpu_ctx, every, lo, lo + int(rng.integers(1, 2 * (info.max - info.min))), bits)
    if dtype in (np.uint8, np.uint16) and info.bits == bits:      # the identity
        src = upload(gpu_ctx, every)
        out = src.window(0, info.max, 'r%d' % bits)
        assert whole(out, every.shape).tobytes() == every.tobytes()
        src.destroy(); out.destroy()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("bits", [8, 16])
def test_float_windows_specials_and_rounding_ties(gpu_ctx, bits):
    M = (1 << bits) - 1
    for lo, hi in ((-1.0, 1.0), (0.0, 1.0), (-1000.0, 3000.0), (0.1, 0.7), (-1e30, 1e30), (1e-40, 2e-40), (-3.0e38, 3.0e38 / 4), (5.0, 5.0 + 2 ** -40)):
        v = float_cases(lo, hi, M)
        v = np.resize(v, (v.size // 35 + 1) * 35).reshape(-1, 5, 7)
        assert np.isnan(v).any() and np.isinf(v).any()
        check_window(gpu_ctx, v, lo, hi, bits)


@pytest.mark.timeout(120)
def test_result_does_not_depend_on_the_source_being_finalized(gpu_ctx):
    """the operations read SNORM's most negative code as the one above it themselves: a source that was never finalized still holds it"""
    L = N.lib()
    for dtype, fmt in ((np.int8, N.FORMAT_R8_SNORM), (np.int16, N.FORMAT_R16_SNORM)):
        info = np.iinfo(dtype)
        a = np.full((3, 4, 5), info.min, dtype)
        a[1] = info.min + 1; a[2, 0, 0] = 5
        h = C.c_void_p()
        N.check(L.vpt_volume_create(gpu_ctx._h, 5, 4, 3, fmt, C.byref(h)))
        N.check(L.vpt_volume_upload_block(h, 0, 0, 0, 5, 4, 3, a.ctypes.data_as(C.c_void_p), a.nbytes))
        out = C.c_void_p()
        N.check(L.vpt_volume_window(h, float(info.min), float(info.min + 2), N.FORMAT_R8, C.byref(out)))
        got = np.empty(a.shape, np.uint8)
        N.check(L.vpt_volume_read_block(out, 0, 0, 0, 5, 4, 3, got.ctypes.data_as(C.c_void_p), got.nbytes))
        assert got.tobytes() == vpt_amd.window_texels(a, info.min, info.min + 2, 8).tobytes()
        assert got[0, 0, 0] == got[1, 0, 0] == 128 and got[2, 0, 0] == 255
        lo, hi = C.c_double(), C.c_double()
        N.check(L.vpt_volume_range(h, C.byref(lo), C.byref(hi)))
        assert (lo.value, hi.value) == (info.min + 1, 5)
        bins = np.zeros(1 << info.bits, np.uint32)
        N.check(L.vpt_volume_code_histogram(h, bins.ctypes.data_as(C.POINTER(C.c_uint32)), bins.size))
        want = np.bincount(np.maximum(a, -info.max).astype(np.int64).reshape(-1) - info.min, minlength=1 << info.bits)
        assert bins[0] == 0 and np.array_equal(bins, want)
        L.vpt_volume_destroy(out); L.vpt_volume_destroy(h)


@pytest.mark.timeout(60)
def test_windowed_volume_describes_itself(gpu_ctx):
    src = upload(gpu_ctx, texels(np.int16, DIMS), 'nearest')
    for bits in (8, 16):
        out = src.window(-200, 400, 'r%d' % bits)
        assert out.ready and out.getTexture() is not None
        m = out.modality
        assert m['dimensions'] == {'width': DIMS[2], 'height': DIMS[1], 'depth': DIMS[0]} and m['format'] == R.GL_RED
        assert (m['internalFormat'], m['type']) == ((R.GL_R8, R.GL_UNSIGNED_BYTE) if bits == 8 else (R.GL_R16_EXT, R.GL_UNSIGNED_SHORT))
        assert out.native_format()[0] == (N.FORMAT_R8 if bits == 8 else N.FORMAT_R16)
        assert out.bricked_bytes() * (2 if bits == 8 else 1) == src.bricked_bytes()
        assert out.histogram().sum() == np.prod(DIMS)               # an ordinary volume: the operations of its format take it
        out.destroy()
    src.destroy()


# ---- range and code histogram ------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_range_equals_numpy(gpu_ctx):
    for dtype in TYPES:
        for dims in (DIMS, (1, 1, 1), (16, 16, 16), (3, 1, 17)):
            a = texels(dtype, dims, seed=11)
            vol = upload(gpu_ctx, a)
            lo, hi = vol.range()
            vol.destroy()
            s = stored(a)
            assert (lo, hi) == (s.min(), s.max()), (dtype, dims)
            assert isinstance(lo, float if dtype == np.float32 else int)
    big = texels(np.uint16, WRAP, seed=13)
    big[77, 33, 11] = 60001; big[150, 200, 255] = 0
    vol = upload(gpu_ctx, big)
    assert vol.range() == (0, 60001)
    vol.destroy()
    for dtype in (np.int8, np.int16):                              # the most negative code alone, and beside others
        info = np.iinfo(dtype)
        a = np.full((2, 3, 4), info.min, dtype)
        vol = upload(gpu_ctx, a)
        assert vol.range() == (info.min + 1, info.min + 1)
        vol.destroy()
    f = np.array([np.nan, -0.0, 0.0, np.nan, -3.5, np.inf, 2.0, -np.inf] * 5, np.float32).reshape(2, 4, 5)
    vol = upload(gpu_ctx, f); assert vol.range() == (-np.inf, np.inf); vol.destroy()
    f = np.array([np.nan, -0.0, 0.0, -np.nan] * 6, np.float32).reshape(2, 3, 4)
    vol = upload(gpu_ctx, f); lo, hi = vol.range(); vol.destroy()
    assert lo == 0.0 and hi == 0.0                                 # by value: -0 = +0
    f = np.array([np.nan, 1e-45, -1e-45, 7.5], np.float32).reshape(1, 2, 2)
    vol = upload(gpu_ctx, f); assert vol.range() == (float(np.float32(-1e-45)), 7.5); vol.destroy()
    vol = upload(gpu_ctx, np.full((3, 3, 3), np.nan, np.float32))
    with pytest.raises(vpt_amd.VptError, match="NaN") as e:
        vol.range()
    assert e.value.code == N.ERR_INVALID
    vol.destroy()


def histogram_of(a):
    info = np.iinfo(a.dtype)
    return np.bincount(stored(a).astype(np.int64).reshape(-1) - info.min, minlength=info.max - info.min + 1).astype(np.uint32)


@pytest.mark.timeout(300)
def test_code_histograms_equal_numpy(gpu_ctx):
    rng = np.random.default_rng(17)
    dims = (37, 29, 43)
    cases = []
    for dtype in (np.uint8, np.int8):
        info = np.iinfo(dtype)
        cases.append(rng.integers(info.min, info.max + 1, size=dims).astype(dtype))
        cases.append((sphere_volume(0, noise=45.0, dims=dims).astype(np.int16) + info.min).astype(dtype))
    for dtype in (np.uint16, np.int16):
        info = np.iinfo(dtype)
        off = info.min
        band = lambda a, b: rng.integers(a, b, size=dims)
        two = band(100, 700); two[::2] = band(61000, 61900)[::2]
        cases += [(band(0, 4096) + off).astype(dtype),                       # a narrow band at the low end
                  (band(65536 - 3000, 65536) + off).astype(dtype),           # ... at the high end
                  (two + off).astype(dtype),                                 # two bands far apart: one of them is outside any slab
                  (band(0, 65536) + off).astype(dtype),                      # every code
                  (band(0, 65536).reshape(-1)[:4001].reshape(1, 1, 4001) + off).astype(dtype)]
    for a in cases:
        vol = upload(gpu_ctx, a)
        h = vol.code_histogram()
        vol.destroy()
        want = histogram_of(a)
        assert h.dtype == np.uint32 and h.shape == want.shape and int(h.sum()) == a.size, (a.dtype, a.shape)
        assert np.array_equal(h, want), (a.dtype, a.shape, np.argwhere(h != want)[:4].tolist())
    big = texels(np.uint16, WRAP, seed=19)
    vol = upload(gpu_ctx, big)
    assert np.array_equal(vol.code_histogram(), histogram_of(big))
    assert vol.percentile_window() == vpt_amd.percentile_window(histogram_of(big), 0.5, 99.5, False)
    vol.destroy()
    s = texels(np.int16, DIMS)
    vol = upload(gpu_ctx, s)
    assert vol.percentile_window(1, 99) == vpt_amd.percentile_window(histogram_of(s), 1, 99, True)
    srt = np.sort(s.reshape(-1))
    assert vol.percentile_window(0, 100) == (srt[0], srt[-1])
    vol.destroy()


# ---- parity chain ------------------------------------------------------------------------------------------------------------
def ct_volume(dims=DIMS):
    """int16 Hounsfield-like: the noisy sphere scaled to -1000 .. 3000"""
    v = sphere_volume(0, noise=45.0, dims=dims).astype(np.int64)
    return (v * 4000 // 255 - 1000).astype(np.int16)


def float_volume(dims=DIMS):
    v = sphere_volume(0, noise=45.0, dims=dims).astype(np.float32)
    return (v / np.float32(255.0) * np.float32(2.5) - np.float32(0.75)).astype(np.float32)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("case", ["ct", "float"])
@pytest.mark.parametrize("filt", FILTERS)
def test_windowed_volume_renders_like_the_uploaded_texels(gpu_ctx, filt, case):
    v, lo, hi, bits = (ct_volume(), -200, 400, 8) if case == "ct" else (float_volume(), -0.5, 1.5, 16)
    want = vpt_amd.window_texels(v, lo, hi, bits)
    assert len(np.unique(want)) >= 32, "degenerate input: %d distinct windowed values" % len(np.unique(want))
    tf = colour_tf(256)
    src = upload(gpu_ctx, v, filt)
    a = src.window(lo, hi, 'r%d' % bits)                          # carries src's filter
    b = upload(gpu_ctx, want, filt)
    for kind in CLASSES:
        fa = render(gpu_ctx, a, kind, tf=tf)
        same(fa, render(gpu_ctx, b, kind, tf=tf), '%s %s %s' % (kind, filt, case))
        # a non-empty frame: not every pixel is the same (an empty frame is the background everywhere).  Two passes of a Monte-Carlo
        # renderer over a 61 x 47 frame hold only a handful of distinct values beside the white environment, so the number of distinct
        # byte values says nothing there; MIP, which the pattern test measures that way, is held to it as well
        pixels = np.ascontiguousarray(fa[-1]); pixels = pixels.reshape(-1, pixels.shape[-1])
        assert len(np.unique(pixels.view(np.uint16), axis=0)) >= 2, '%s: empty frame' % kind
        if kind == 'mip':
            assert len(set(pixels.tobytes())) > 8, 'mip: empty frame'
    p = ((4,), {'frames': True})
    same(render(gpu_ctx, a, 'mcm', tf=tf, play=p), render(gpu_ctx, b, 'mcm', tf=tf, play=p), 'mcm frames %s %s' % (filt, case))
    for kind in ('eam', 'mcm'):                                    # the feature is visible: the source itself renders differently
        one, two = render(gpu_ctx, src, kind, tf=tf), render(gpu_ctx, a, kind, tf=tf)
        assert one[-1].tobytes() != two[-1].tobytes(), '%s: the window changes nothing' % kind
    for vol in (src, a, b):
        vol.destroy()


@pytest.mark.timeout(300)
def test_window_then_gradient_equals_the_numpy_chain(gpu_ctx):
    for v, lo, hi in ((ct_volume(), -200, 400), (float_volume(), -0.5, 1.5), (texels(np.int8, DIMS), -100, 100)):
        for bits in (8, 16):
            for operator in ('central', 'sobel'):
                src = upload(gpu_ctx, v)
                w = src.window(lo, hi, 'r%d' % bits)
                g = w.derive_gradient(operator, 2)
                got = whole(g, v.shape)
                for vol in (src, w, g):
                    vol.destroy()
                wt = vpt_amd.window_texels(v, lo, hi, bits)
                gm = vpt_amd.gradient_magnitude(wt, operator, 2)
                assert len(np.unique(gm)) >= 32
                assert got[..., 0].tobytes() == wt.tobytes() and got[..., 1].tobytes() == gm.tobytes(), (v.dtype, bits, operator)


@pytest.mark.timeout(300)
def test_source_and_windowed_volume_are_independent(gpu_ctx):
    v = ct_volume()
    tf = colour_tf(256)
    src = upload(gpu_ctx, v)
    before = {kind: render(gpu_ctx, src, kind, tf=tf) for kind in ('eam', 'mcm')}
    out = src.window(-200, 400)
    for kind in before:
        same(render(gpu_ctx, src, kind, tf=tf), before[kind], 'source after the window, %s' % kind)
    derived = {kind: render(gpu_ctx, out, kind, tf=tf) for kind in ('eam', 'mcm')}
    tex = whole(out, DIMS)
    src.upload_block(2, 3, 4, np.full((5, 6, 7), 3000, np.int16))
    assert whole(out, DIMS).tobytes() == tex.tobytes()
    src.destroy()
    for kind in derived:
        same(render(gpu_ctx, out, kind, tf=tf), derived[kind], 'windowed after source.destroy(), %s' % kind)
    # an ordinary R8 volume: a box uploaded into it is seen by the next pass
    box = np.random.default_rng(5).integers(0, 256, size=(9, 8, 10)).astype(np.uint8)
    out.upload_block(6, 5, 7, box)
    tex[7:16, 5:13, 6:16] = box
    assert whole(out, DIMS).tobytes() == tex.tobytes()
    twin = upload(gpu_ctx, tex)
    for kind in derived:
        same(render(gpu_ctx, out, kind, tf=tf), render(gpu_ctx, twin, kind, tf=tf), 'windowed after upload_block, %s' % kind)
    out.destroy(); twin.destroy()


@pytest.mark.timeout(120)
def test_renderer_bound_to_the_source_is_not_disturbed(gpu_ctx):
    from vpt_amd.scene import Transform, Node, default_camera
    v = sphere_volume(0, noise=45.0, dims=DIMS)
    tf = colour_tf(256)
    frames = []
    for window in (False, True):
        src = upload(gpu_ctx, v)
        r = vpt_amd.MCMRenderer(gpu_ctx, src, default_camera(61 / 47), None, {'resolution': (61, 47), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
        r.setTransferFunction(tf); r.extinction = 40; r.reset()
        r.render()
        out = src.window(30, 200) if window else None
        r.render()
        frames.append(r.getTexture())
        r.destroy(); src.destroy()
        if out:
            out.destroy()
    assert frames[0].tobytes() == frames[1].tobytes()


# ---- errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_unsupported_sources_and_bad_arguments_raise(gpu_ctx):
    rng = np.random.default_rng(1)
    words = rng.integers(0, 1 << 16, size=(4, 4, 4), dtype=np.uint64).astype(np.uint16)
    t, f, i, _ = PACKED[N.FORMAT_RGB565]
    packed = vpt_amd.Volume(gpu_ctx, BVPReader(BlobLoader(make_bvp_typed(words, f, i, t, ((), (), ()))))); packed.load()
    sources = ((upload(gpu_ctx, np.zeros((4, 4, 4, 2), np.uint8)), "RG8"), (upload(gpu_ctx, np.zeros((4, 4, 4, 2), np.float32)), "RG32F"),
               (vpt_amd.Volume.from_array(gpu_ctx, np.zeros((4, 4, 4, 2), np.int8), snorm=True), "RG8_SNORM"),
               (upload(gpu_ctx, np.zeros((4, 4, 4, 2), np.uint16)), "RG16"), (upload(gpu_ctx, np.zeros((4, 4, 4, 2), np.int16)), "RG16_SNORM"),
               (packed, "RGB565"))
    L = N.lib()
    for vol, name in sources:
        for call in (lambda: vol.window(0, 1), lambda: vol.range(), lambda: vol.code_histogram()):
            with pytest.raises(vpt_amd.VptError, match=r"\b%s\b" % name) as e:
                call()
            assert e.value.code == N.ERR_UNSUPPORTED
        vol.destroy()
    fvol = upload(gpu_ctx, np.zeros((4, 4, 4), np.float32))
    with pytest.raises(vpt_amd.VptError, match=r"\bR32F\b") as e:
        fvol.code_histogram()
    assert e.value.code == N.ERR_UNSUPPORTED
    h = C.c_void_p()
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (float('nan'), 1.0), (0.0, float('inf')), (-1.7e308, 1.7e308)):
        assert L.vpt_volume_window(fvol.texture, lo, hi, N.FORMAT_R8, C.byref(h)) == N.ERR_INVALID, (lo, hi)
        assert b"R32F" in L.vpt_last_error()
    fvol.destroy()
    vol = upload(gpu_ctx, np.zeros((4, 4, 4), np.uint16))
    for lo, hi in ((5.0, 5.0), (6.0, 5.0), (0.5, 3.0), (0.0, 2.5), (-2.0 ** 31 - 1, 0.0), (0.0, 2.0 ** 31 + 1), (float('nan'), 1.0), (0.0, float('inf'))):
        assert L.vpt_volume_window(vol.texture, lo, hi, N.FORMAT_R8, C.byref(h)) == N.ERR_INVALID, (lo, hi)
        assert b"R16" in L.vpt_last_error()
    for fmt in (N.FORMAT_RG8, N.FORMAT_R32F, N.FORMAT_R8_SNORM, N.FORMAT_R16_SNORM, N.FORMAT_RG16, -1, 99):
        assert L.vpt_volume_window(vol.texture, 0.0, 1.0, fmt, C.byref(h)) == N.ERR_INVALID, fmt
    with pytest.raises(ValueError):
        vol.window(0, 1, 'r32f')
    bins = np.zeros(256, np.uint32)
    assert L.vpt_volume_code_histogram(vol.texture, bins.ctypes.data_as(C.POINTER(C.c_uint32)), 256) == N.ERR_INVALID
    vol.destroy()
    vol = upload(gpu_ctx, np.zeros((4, 4, 4), np.uint8))
    bins = np.zeros(65536, np.uint32)
    assert L.vpt_volume_code_histogram(vol.texture, bins.ctypes.data_as(C.POINTER(C.c_uint32)), 65536) == N.ERR_INVALID
    vol.destroy()


# ---- context path ------------------------------------------------------------------------------------------------------------
def context_frames(options, reader, kind='eam', passes=3, norm16=True):
    opts = {'resolution': (72, 56), 'rng': GoldenRatioRng()}
    opts.update(options)
    rc = vpt_amd.RenderingContext(opts)
    if norm16:
        assert rc.gl.getExtension('EXT_texture_norm16')
    try:
        rc.resize(72, 56)
        rc.setVolume(reader)
        fmt = rc.volume.native_format()[0]
        tex = rc.volume.read_block(0, 0, 0, DIMS[2], DIMS[1], DIMS[0])
        rc.chooseRenderer(kind); rc.chooseToneMapper('artistic')
        rc.renderer.setTransferFunction(colour_tf(64, 48))
        if kind == 'mcm':
            rc.renderer.extinction = 40
        rc.renderer.reset()
        frames = []
        for _ in range(passes):
            rc.render()
            frames.append(rc.getFrame().copy())
    finally:
        rc.destroy()
    return fmt, tex, frames


def typed_reader(a):
    triple = {np.dtype(np.int16): (R.GL_RED, R.GL_R16_SNORM_EXT, R.GL_SHORT), np.dtype(np.uint16): (R.GL_RED, R.GL_R16_EXT, R.GL_UNSIGNED_SHORT),
              np.dtype(np.uint8): (R.GL_RED, R.GL_R8, R.GL_UNSIGNED_BYTE), np.dtype(np.float32): (R.GL_RED, R.GL_R32F, R.GL_FLOAT)}[a.dtype]
    return BVPReader(BlobLoader(make_bvp_typed(a, triple[0], triple[1], triple[2], ((9,), (11, 14), (7, 17)))))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", ["eam", "mcm"])
def test_rendering_context_windows_the_volume_when_asked(kind):
    d, h, w = DIMS
    v = ct_volume()
    raw16 = lambda: RAWReader(v.astype('<i2').tobytes(), {'width': w, 'height': h, 'depth': d, 'bits': 16, 'signed': True})   # a 16-bit .raw file, end to end
    hist = np.bincount(v.astype(np.int64).reshape(-1) + 32768, minlength=65536)
    spellings = (([-200, 400], (-200, 400)), ('range', (int(v.min()), int(v.max()))),
                 ({'percentiles': [2, 98]}, vpt_amd.percentile_window(hist, 2, 98, True)))
    for fmt_name, bits, native in (('r8', 8, N.FORMAT_R8), ('r16', 16, N.FORMAT_R16)):
        for window, (lo, hi) in spellings:
            want = vpt_amd.window_texels(v, lo, hi, bits)
            fmt, tex, frames = context_frames({'window': window, 'windowFormat': fmt_name}, raw16(), kind)
            assert fmt == native and tex.tobytes() == want.tobytes(), (window, fmt_name)
            fmt, _, by_hand = context_frames({}, typed_reader(want), kind)
            assert fmt == native
            same(frames, by_hand, 'context with window = %r against the uploaded texels' % (window,))
            if bits == 16:
                continue
            # ... and with the gradient behind it
            pair = np.ascontiguousarray(np.stack([want, vpt_amd.gradient_magnitude(want, 'sobel', 2)], axis=-1))
            fmt, tex, frames = context_frames({'window': window, 'gradient': 'sobel', 'gradientGain': 2}, raw16(), kind)
            assert fmt == N.FORMAT_RG8 and tex.tobytes() == pair.tobytes()
    # the option absent (or null): the volume as it is, and the gradient option leaves an SNORM volume alone
    fmt, tex, plain = context_frames({}, raw16(), kind)
    assert fmt == N.FORMAT_R16_SNORM and tex.tobytes() == v.tobytes()
    fmt, _, frames = context_frames({'window': None, 'gradient': 'sobel'}, raw16(), kind)
    assert fmt == N.FORMAT_R16_SNORM
    same(frames, plain, 'window = None')
    # a float volume: 'range', and the library's own error for a range that is not finite
    f = float_volume()
    fmt, tex, _ = context_frames({'window': 'range', 'windowFormat': 'r16'}, typed_reader(f), kind)
    assert fmt == N.FORMAT_R16 and tex.tobytes() == vpt_amd.window_texels(f, float(f.min()), float(f.max()), 16).tobytes()
    bad = f.copy(); bad[3, 4, 5] = np.inf
    with pytest.raises(vpt_amd.VptError) as e:
        context_frames({'window': 'range'}, typed_reader(bad), kind)
    assert e.value.code == N.ERR_INVALID
    with pytest.raises(vpt_amd.VptError) as e:
        context_frames({'window': 'range'}, typed_reader(np.full(DIMS, np.nan, np.float32)), kind)
    assert e.value.code == N.ERR_INVALID
    for bad in ('auto', [1], [1, 2, 3], {'percentile': [1, 2]}, {'percentiles': [60, 40]}, 5):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext({'window': bad})
    with pytest.raises(ValueError):
        vpt_amd.RenderingContext({'window': [0, 1], 'windowFormat': 'r32f'})
