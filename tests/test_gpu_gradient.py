"""GPU: the gradient-magnitude channel derived on the device (vpt_volume_derive_gradient), texel read-back (vpt_volume_read_block) and
histograms (vpt_volume_histogram).

The derived channel is held, byte for byte, to vpt_amd.gradient_magnitude, the numpy statement of the integer contract
(tests/test_gradient_host.py holds that to a scalar Python-integer loop).  Parity chain to the oracle: RG8 / RG16 volumes uploaded from the
host are held to the CPU oracle by the rest of the suite, so a derived volume must give byte-identical buffers to the volume uploaded from
np.stack([v, G], -1) in every renderer and under every filter."""
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
from test_volume_formats import decode_packed

pytestmark = pytest.mark.gpu

DIMS = (23, 19, 21)                         # depth, height, width: odd, no multiple of a brick or of any tile
# ... a single slice; a cube of whole bricks; larger than the gradient kernel's 128 x 8 x 32 tile on every axis, rows not dword-aligned;
# the same with dword-aligned rows that cross a tile
SHAPES = (DIMS, (1, 5, 7), (64, 64, 64), (35, 11, 131), (34, 10, 260))
OPERATORS = ('central', 'sobel')
FILTERS = ('linear', 'nearest', 'quasicubic')


def widen(v8, seed=7):
    """a uint16 field over the whole 16-bit range from a uint8 one"""
    return np.clip(v8.astype(np.int64) * 257 + np.random.default_rng(seed).integers(0, 257, size=v8.shape), 0, 65535).astype(np.uint16)


def sphere(dims, bits):
    v = sphere_volume(0, noise=45.0, dims=dims)
    return v if bits == 8 else widen(v)


def noise(dims, bits):
    return np.random.default_rng(7).integers(0, 1 << bits, size=dims).astype(np.uint8 if bits == 8 else np.uint16)


def upload(ctx, a, filt='linear'):
    return vpt_amd.Volume.from_array(ctx, a, filt, norm16=a.dtype == np.uint16)


def whole(vol, dims):
    d, h, w = dims
    return vol.read_block(0, 0, 0, w, h, d)


# ---- read-back ---------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_read_block_returns_what_was_uploaded(gpu_ctx):
    rng = np.random.default_rng(3)
    d, h, w = DIMS
    words = rng.integers(0, 1 << 16, size=DIMS, dtype=np.uint64).astype(np.uint16)
    t, f, i, _ = PACKED[N.FORMAT_RGB565]
    packed = vpt_amd.Volume(gpu_ctx, BVPReader(BlobLoader(make_bvp_typed(words, f, i, t, ((9,), (11, 14), (7, 17)))))); packed.load()
    texels = [rng.integers(0, 256, size=DIMS).astype(np.uint8), rng.integers(0, 256, size=DIMS + (2,)).astype(np.uint8),
              rng.standard_normal(DIMS).astype(np.float32), rng.integers(0, 65536, size=DIMS).astype(np.uint16)]
    volumes = [upload(gpu_ctx, a) for a in texels] + [packed]
    texels.append(decode_packed(words, N.FORMAT_RGB565))
    for vol, want in zip(volumes, texels):
        got = whole(vol, DIMS)
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
        # boxes that start and end mid-brick; a run of whole slices; one texel
        for x, y, z, bw, bh, bd in ((1, 2, 3, 13, 9, 11), (5, 0, 6, 16, h, 2), (0, 0, 9, w, h, 5), (w - 1, h - 1, d - 1, 1, 1, 1), (2, 3, 0, 3, 1, d)):
            got = vol.read_block(x, y, z, bw, bh, bd)
            assert got.tobytes() == np.ascontiguousarray(want[z:z + bd, y:y + bh, x:x + bw]).tobytes(), (want.dtype, x, y, z)
        with pytest.raises(vpt_amd.VptError, match="outside volume"):
            vol.read_block(1, 0, 0, w, h, d)
        vol.destroy()


# ---- the channel itself ------------------------------------------------------------------------------------------------------
def check_channel(ctx, v, operator, gain, want_distinct=32, clamp=False):
    want = vpt_amd.gradient_magnitude(v, operator, gain)
    top = np.iinfo(v.dtype).max
    if want_distinct:
        assert len(np.unique(want)) >= want_distinct, "degenerate input: %d distinct values" % len(np.unique(want))
    if clamp:
        share = (want == top).mean()
        assert 0.1 <= share <= 0.9, "degenerate clamp case: %.3f of the voxels at the maximum" % share
    src = upload(ctx, v)
    out = src.derive_gradient(operator, gain)
    got = whole(out, v.shape)
    src.destroy(); out.destroy()
    assert got.dtype == v.dtype and got.shape == v.shape + (2,)
    assert got[..., 0].tobytes() == v.tobytes(), "channel 0 is not the source (%s %s gain %s)" % (v.shape, operator, gain)
    bad = np.argwhere(got[..., 1] != want)
    assert len(bad) == 0, "%d voxels differ (%s %s %s gain %s), first at z, y, x = %s: %d, expected %d" % (
        len(bad), v.dtype, v.shape, operator, gain, bad[0], got[..., 1][tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("operator", OPERATORS)
def test_derived_channel_equals_the_contract(gpu_ctx, operator, bits):
    for dims in SHAPES:
        small = dims[0] == 1                                       # (35 voxels of a single slice cannot hold 32 distinct gradients)
        check_channel(gpu_ctx, sphere(dims, bits), operator, 4, want_distinct=0 if small else 32)
        check_channel(gpu_ctx, noise(dims, bits), operator, 1, want_distinct=0 if small else 32)
    for dims in SHAPES:                                            # the clamp: about half of the voxels at the maximum
        check_channel(gpu_ctx, noise(dims, bits), 'central', 3, want_distinct=0 if dims[0] == 1 else 32, clamp=dims[0] > 1)


@pytest.mark.timeout(120)
def test_extreme_gains_and_the_saturating_step(gpu_ctx):
    step = np.zeros((6, 9, 12), np.uint16); step[:, :, 6:] = 65535
    check_channel(gpu_ctx, step, 'sobel', 16, want_distinct=0)
    check_channel(gpu_ctx, (step >> 8).astype(np.uint8), 'sobel', 16, want_distinct=0)
    for bits in (8, 16):
        for operator in OPERATORS:
            for gain in (1 / 128, 0.5, 16):
                check_channel(gpu_ctx, noise(DIMS, bits), operator, gain, want_distinct=0)
                check_channel(gpu_ctx, sphere(DIMS, bits), operator, gain, want_distinct=0)


@pytest.mark.timeout(60)
def test_derived_volume_describes_itself(gpu_ctx):
    for bits in (8, 16):
        src = upload(gpu_ctx, sphere(DIMS, bits), 'nearest')
        out = src.derive_gradient('sobel', 2.0)
        assert out.ready and out.getTexture() is not None
        m = out.modality
        assert m['dimensions'] == {'width': DIMS[2], 'height': DIMS[1], 'depth': DIMS[0]} and m['format'] == R.GL_RG
        assert (m['internalFormat'], m['type']) == ((R.GL_RG8, R.GL_UNSIGNED_BYTE) if bits == 8 else (R.GL_RG16_EXT, R.GL_UNSIGNED_SHORT))
        assert out.native_format()[0] == (N.FORMAT_RG8 if bits == 8 else N.FORMAT_RG16)
        assert out.bricked_bytes() == 2 * src.bricked_bytes()
        src.destroy(); out.destroy()


# ---- parity chain ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(600)
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("filt", FILTERS)
def test_derived_volume_renders_like_the_uploaded_pair(gpu_ctx, filt, bits):
    v = sphere(DIMS, bits)
    tf = colour_tf(64, 48)
    for operator, gain in (('central', 4), ('sobel', 4)):
        src = upload(gpu_ctx, v, filt)
        a = src.derive_gradient(operator, gain)                   # carries src's filter
        pair = np.ascontiguousarray(np.stack([v, vpt_amd.gradient_magnitude(v, operator, gain)], axis=-1))
        b = upload(gpu_ctx, pair, filt)
        for kind in CLASSES:
            same(render(gpu_ctx, a, kind, tf=tf), render(gpu_ctx, b, kind, tf=tf), '%s %s %s %d' % (kind, filt, operator, bits))
        p = ((4,), {'frames': True})
        same(render(gpu_ctx, a, 'mcm', tf=tf, play=p), render(gpu_ctx, b, 'mcm', tf=tf, play=p), 'mcm frames %s %s %d' % (filt, operator, bits))
        if bits == 8:      # the feature is visible: the second channel moves the lookup off row 0 of the table
            for kind in ('eam', 'mcm'):
                one, two = render(gpu_ctx, src, kind, tf=tf), render(gpu_ctx, a, kind, tf=tf)
                assert one[-1].tobytes() != two[-1].tobytes(), '%s: the derived channel changes nothing' % kind
        for vol in (src, a, b):
            vol.destroy()


# ---- independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_source_and_derived_volume_are_independent(gpu_ctx):
    v = sphere(DIMS, 8)
    tf = colour_tf(64, 48)
    src = upload(gpu_ctx, v)
    before = {kind: render(gpu_ctx, src, kind, tf=tf) for kind in ('eam', 'mcm')}
    out = src.derive_gradient('sobel', 4)
    for kind in before:
        same(render(gpu_ctx, src, kind, tf=tf), before[kind], 'source after the derivation, %s' % kind)
    derived = {kind: render(gpu_ctx, out, kind, tf=tf) for kind in ('eam', 'mcm')}
    texels = whole(out, DIMS)
    # an upload into the source afterwards does not reach the derived volume
    src.upload_block(2, 3, 4, np.full((5, 6, 7), 200, np.uint8))
    assert whole(src, DIMS)[4:9, 3:9, 2:9].min() == 200
    assert whole(out, DIMS).tobytes() == texels.tobytes()
    for kind in derived:
        same(render(gpu_ctx, out, kind, tf=tf), derived[kind], 'derived after an upload into the source, %s' % kind)
    # ... nor does destroying the source
    src.destroy()
    for kind in derived:
        same(render(gpu_ctx, out, kind, tf=tf), derived[kind], 'derived after source.destroy(), %s' % kind)
    # the derived volume is an ordinary RG8 volume: a box uploaded into it is seen by the next pass
    box = np.random.default_rng(5).integers(0, 256, size=(9, 8, 10, 2)).astype(np.uint8)
    out.upload_block(6, 5, 7, box)
    texels[7:16, 5:13, 6:16] = box
    assert whole(out, DIMS).tobytes() == texels.tobytes()
    twin = upload(gpu_ctx, texels)
    for kind in derived:
        after = render(gpu_ctx, out, kind, tf=tf)
        same(after, render(gpu_ctx, twin, kind, tf=tf), 'derived after upload_block, %s' % kind)
        assert after[-1].tobytes() != derived[kind][-1].tobytes()
    out.destroy(); twin.destroy()


@pytest.mark.timeout(120)
def test_renderer_bound_to_the_source_is_not_disturbed(gpu_ctx):
    from vpt_amd.scene import Transform, Node, default_camera
    v = sphere(DIMS, 8)
    tf = colour_tf(64, 48)
    frames = []
    for derive in (False, True):
        src = upload(gpu_ctx, v)
        r = vpt_amd.MCMRenderer(gpu_ctx, src, default_camera(61 / 47), None, {'resolution': (61, 47), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
        r.setTransferFunction(tf); r.extinction = 40; r.reset()
        r.render()
        out = src.derive_gradient('central', 2) if derive else None
        r.render()
        frames.append(r.getTexture())
        r.destroy(); src.destroy()
        if out:
            out.destroy()
    assert frames[0].tobytes() == frames[1].tobytes()


# ---- histogram ---------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_histograms_equal_numpy(gpu_ctx):
    dims = (37, 29, 43)
    v8, v16 = sphere(dims, 8), sphere(dims, 16)
    n = v8.size
    for v, want in ((v8, np.bincount(v8.reshape(-1), minlength=256)), (v16, np.bincount((v16 >> 8).reshape(-1), minlength=256))):
        vol = upload(gpu_ctx, v)
        h = vol.histogram()
        assert h.dtype == np.uint32 and h.shape == (256,) and int(h.sum()) == n and np.array_equal(h, want)
        vol.destroy()

    def joint(pair):
        top = pair if pair.dtype == np.uint8 else pair >> 8
        want, _, _ = np.histogram2d(top[..., 1].reshape(-1), top[..., 0].reshape(-1), bins=[np.arange(257), np.arange(257)])
        return want.astype(np.uint32)

    src = upload(gpu_ctx, v8)
    derived = src.derive_gradient('sobel', 4)
    pair = whole(derived, dims)
    rng = np.random.default_rng(9)
    for vol, texels in ((derived, pair), (upload(gpu_ctx, rng.integers(0, 256, size=dims + (2,)).astype(np.uint8)), None),
                        (upload(gpu_ctx, rng.integers(0, 65536, size=(9, 10, 11, 2)).astype(np.uint16)), None)):
        if texels is None:
            texels = vol.read_block(0, 0, 0, vol.modality['dimensions']['width'], vol.modality['dimensions']['height'], vol.modality['dimensions']['depth'])
        h = vol.histogram()
        assert h.dtype == np.uint32 and h.shape == (256, 256) and int(h.sum()) == texels[..., 0].size
        assert np.array_equal(h, joint(texels))
        vol.destroy()
    assert pair[..., 1].max() >= 32, "the derived histogram must reach beyond the rows counted in LDS"
    src.destroy()
    f = upload(gpu_ctx, np.zeros((4, 4, 4), np.float32))
    with pytest.raises(vpt_amd.VptError, match="R32F"):
        f.histogram()
    f.destroy()


# ---- errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_unsupported_sources_and_bad_arguments_raise(gpu_ctx):
    rng = np.random.default_rng(1)
    words = rng.integers(0, 1 << 16, size=(4, 4, 4), dtype=np.uint64).astype(np.uint16)
    t, f, i, _ = PACKED[N.FORMAT_RGB565]
    packed = vpt_amd.Volume(gpu_ctx, BVPReader(BlobLoader(make_bvp_typed(words, f, i, t, ((), (), ()))))); packed.load()
    sources = ((upload(gpu_ctx, np.zeros((4, 4, 4), np.float32)), "R32F"), (upload(gpu_ctx, np.zeros((4, 4, 4, 2), np.uint8)), "RG8"),
               (vpt_amd.Volume.from_array(gpu_ctx, np.zeros((4, 4, 4), np.int8), snorm=True), "R8_SNORM"),
               (vpt_amd.Volume.from_array(gpu_ctx, np.zeros((4, 4, 4), np.int16), norm16=True), "R16_SNORM"),
               (upload(gpu_ctx, np.zeros((4, 4, 4, 2), np.uint16)), "RG16"), (packed, "RGB565"))
    for vol, name in sources:
        with pytest.raises(vpt_amd.VptError, match=r"\b%s\b" % name) as e:
            vol.derive_gradient('central', 1.0)
        assert e.value.code == N.ERR_UNSUPPORTED
        vol.destroy()
    vol = upload(gpu_ctx, np.zeros((4, 4, 4), np.uint8))
    for operator in ('prewitt', 2, None):
        with pytest.raises(ValueError):
            vol.derive_gradient(operator, 1.0)
    for gain in (0.0, 1 / 256, 16.5, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            vol.derive_gradient('central', gain)
    import ctypes as C
    h = C.c_void_p()
    L = N.lib()
    assert L.vpt_volume_derive_gradient(vol.texture, 2, 1.0, C.byref(h)) == N.ERR_INVALID
    for gain in (0.0, 16.5, float('nan')):
        assert L.vpt_volume_derive_gradient(vol.texture, 0, gain, C.byref(h)) == N.ERR_INVALID
    bins = np.zeros(100, np.uint32)
    assert L.vpt_volume_histogram(vol.texture, bins.ctypes.data_as(C.POINTER(C.c_uint32)), 100) == N.ERR_INVALID
    vol.destroy()


# ---- context path ------------------------------------------------------------------------------------------------------------
def context_frames(options, reader, kind='eam', passes=3):
    opts = {'resolution': (72, 56), 'rng': GoldenRatioRng()}
    opts.update(options)
    rc = vpt_amd.RenderingContext(opts)
    rc.resize(72, 56)
    rc.setVolume(reader)
    fmt = rc.volume.native_format()[0]
    rc.chooseRenderer(kind); rc.chooseToneMapper('artistic')
    rc.renderer.setTransferFunction(colour_tf(64, 48))
    if kind == 'mcm':
        rc.renderer.extinction = 40
    rc.renderer.reset()
    frames = []
    for _ in range(passes):
        rc.render()
        frames.append(rc.getFrame().copy())
    rc.destroy()
    return fmt, frames


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", ["eam", "mcm"])
def test_rendering_context_derives_the_channel_when_asked(kind):
    d, h, w = DIMS
    v = sphere(DIMS, 8)
    raw = lambda: RAWReader(v, {'width': w, 'height': h, 'depth': d})
    pair = np.ascontiguousarray(np.stack([v, vpt_amd.gradient_magnitude(v, 'sobel', 2)], axis=-1))
    by_hand = lambda: BVPReader(BlobLoader(make_bvp_typed(pair, R.GL_RG, R.GL_RG8, R.GL_UNSIGNED_BYTE, ((), (), ()))))
    fmt, derived = context_frames({'gradient': 'sobel', 'gradientGain': 2}, raw(), kind)
    assert fmt == N.FORMAT_RG8
    fmt, want = context_frames({}, by_hand(), kind)
    assert fmt == N.FORMAT_RG8
    same(derived, want, 'context with gradient = sobel against the hand-derived volume')
    # the option absent (or null): the one-channel volume as it is
    fmt, plain = context_frames({}, raw(), kind)
    assert fmt == N.FORMAT_R8
    same(context_frames({'gradient': None}, raw(), kind)[1], plain, 'gradient = None')
    assert plain[-1].tobytes() != derived[-1].tobytes()
    # a two-channel volume is used as it is, whatever the option says
    fmt, kept = context_frames({'gradient': 'central'}, by_hand(), kind)
    assert fmt == N.FORMAT_RG8
    same(kept, want, 'a two-channel volume under gradient = central')
    with pytest.raises(ValueError):
        vpt_amd.RenderingContext({'gradient': 'prewitt'})
