"""GPU: SNORM volumes (R8_SNORM / RG8_SNORM, one-byte bricks decoded per tap) and packed-texel volumes (decoded on upload into RG32F)
against the R32F / RG32F volume of their decoded texels, bit for bit: every buffer read() returns plus getTexture().  The R32F / RG32F
volumes are held to the oracle by the rest of the suite, so this equality is the parity chain (GL: convert, then filter)."""
import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd import readers as R
from vpt_amd.loaders import BlobLoader
from vpt_amd.readers import BVPReader
from vpt_amd.scene import Transform, Node, default_camera, mvp_inverse_matrix
from vpt_amd.synthetic import sphere_volume, colour_tf, GoldenRatioRng

from test_gpu_readers import make_bvp_typed
from test_volume_formats import snorm, decode_packed

pytestmark = pytest.mark.gpu

CLASSES = {'mip': vpt_amd.MIPRenderer, 'eam': vpt_amd.EAMRenderer, 'mcs': vpt_amd.MCSRenderer, 'mcm': vpt_amd.MCMRenderer,
           'iso': vpt_amd.ISORenderer, 'depth': vpt_amd.DepthRenderer, 'lao': vpt_amd.LAORenderer, 'dos': vpt_amd.DOSRenderer}
BUFFERS = {'mcm': [N.BUFFER_RENDER, N.BUFFER_MCM_POSITION, N.BUFFER_MCM_DIRECTION, N.BUFFER_MCM_TRANSMITTANCE, N.BUFFER_MCM_RADIANCE],
           'dos': [N.BUFFER_RENDER, N.BUFFER_ACCUM, N.BUFFER_DOS_OCCLUSION]}
DIMS = (23, 19, 21)                      # depth, height, width: odd, not a multiple of the 4^3 bricks
CUTS = ((9,), (11, 14), (7, 17))         # BVP block edges (x, y, z): blocks end mid-brick


def signed_volume(dims=DIMS, channels=1, seed=3):
    """int8 [d][h][w](/[2]): a noisy sphere shifted into [-128, 127] (every byte value occurs), the second channel random"""
    base = sphere_volume(0, noise=45.0, dims=dims).astype(np.int16) - 128
    flat = base.reshape(-1)
    flat[:256] = np.arange(-128, 128)
    s = base.astype(np.int8)
    if channels == 1:
        return s
    rng = np.random.default_rng(seed)
    out = rng.integers(-128, 128, size=dims + (channels,), dtype=np.int16).astype(np.int8)
    out[..., 0] = s
    return out


def render(ctx, gvol, kind, w=61, h=47, tf=None, options=(), play=None, passes=2):
    """reset + `passes` render() (or play(*play)) -> every buffer, getTexture() last"""
    r = CLASSES[kind](ctx, gvol, default_camera(w / h), None, {'resolution': (w, h), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
    if tf is not None:
        r.setTransferFunction(tf)
    for opt, val in options:
        r.set_option(opt, val)
    if kind == 'mcm':
        r.extinction = 40
    r.reset()
    if play is not None:
        r.play(*play[0], **play[1])
    else:
        for _ in range(passes):
            r.render()
    out = [r.read(b) for b in BUFFERS.get(kind, [N.BUFFER_RENDER, N.BUFFER_FRAME, N.BUFFER_ACCUM])] + [r.getTexture()]
    if play is not None and play[1].get('frames'):
        out += [r.read_frame_slot(k) for k in range(play[0][0])]
    r.destroy()
    return out


def same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s: buffer %d differs" % (what, i)


def twins(ctx, s, filt):
    """(SNORM volume, R32F / RG32F volume of the decoded texels) of an int8 array"""
    a = vpt_amd.Volume.from_array(ctx, s, filt, snorm=True)
    b = vpt_amd.Volume.from_array(ctx, snorm(s), filt)
    return a, b


@pytest.mark.timeout(120)
def test_snorm_probes_equal_the_r32f_probes(gpu_ctx):
    s = signed_volume()
    d, h, w = s.shape
    rng = np.random.default_rng(5)
    for filt in ('nearest', 'linear'):
        a, b = twins(gpu_ctx, s, filt)
        ra = vpt_amd.MIPRenderer(gpu_ctx, a, default_camera(1.0), None, {'resolution': (8, 8)})
        rb = vpt_amd.MIPRenderer(gpu_ctx, b, default_camera(1.0), None, {'resolution': (8, 8)})
        for r in (ra, rb):
            r.setTransferFunction(colour_tf(256))
        z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing='ij')
        centres = np.stack([(x + 0.5) / w, (y + 0.5) / h, (z + 0.5) / d], axis=-1).reshape(-1, 3).astype(np.float32)
        same([ra.probe_sample(centres)], [rb.probe_sample(centres)], 'texel centres, %s' % filt)
        inside = rng.uniform(0, 1, size=(20000, 3)).astype(np.float32)
        outside = rng.uniform(-0.4, 1.4, size=(20000, 3)).astype(np.float32)
        same([ra.probe_sample(inside), ra.probe_sample(outside)], [rb.probe_sample(inside), rb.probe_sample(outside)], 'random, %s' % filt)
        oob = outside[((outside > 1) | (outside < 0)).any(axis=1)]
        same([ra.probe_sample_boundary(oob)], [rb.probe_sample_boundary(oob)], 'boundary atlas, %s' % filt)
        same([ra.probe_sample_boundary(oob)], [ra.probe_sample(oob)], 'atlas = bricks, %s' % filt)
        ra.destroy(); rb.destroy(); a.destroy(); b.destroy()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("filt", ["linear", "nearest"])
def test_r8_snorm_renders_like_r32f_every_renderer(gpu_ctx, filt):
    s = signed_volume()
    a, b = twins(gpu_ctx, s, filt)
    tf = colour_tf(256)
    for kind in CLASSES:
        same(render(gpu_ctx, a, kind, tf=tf), render(gpu_ctx, b, kind, tf=tf), '%s %s' % (kind, filt))
    a.destroy(); b.destroy()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("nch", [2, 3, 4])
def test_multichannel_snorm_manifests_render_like_rg32f(gpu_ctx, nch):
    """RG8_SNORM, RGB8_SNORM, RGBA8_SNORM through a BVP with partial blocks (the shaders read .rg)"""
    s = signed_volume(channels=nch)
    fmt, ifmt = {2: (R.GL_RG, R.GL_RG8_SNORM), 3: (R.GL_RGB, R.GL_RGB8_SNORM), 4: (R.GL_RGBA, R.GL_RGBA8_SNORM)}[nch]
    tf = colour_tf(64, 48)
    for filt in ('linear', 'nearest'):
        a = vpt_amd.Volume(gpu_ctx, BVPReader(BlobLoader(make_bvp_typed(s, fmt, ifmt, R.GL_BYTE, CUTS)))); a.load(); a.setFilter(filt)
        b = vpt_amd.Volume.from_array(gpu_ctx, np.ascontiguousarray(snorm(s[..., :2])), filt)
        for kind in ('mip', 'eam', 'mcs', 'mcm'):
            same(render(gpu_ctx, a, kind, tf=tf), render(gpu_ctx, b, kind, tf=tf), 'RG%d SNORM %s %s' % (nch, kind, filt))
        a.destroy(); b.destroy()


@pytest.mark.timeout(300)
def test_snorm_fast_math_sequences_and_wide_tables(gpu_ctx):
    tf = colour_tf(256)
    s = signed_volume()
    for filt in ('linear', 'nearest'):
        a, b = twins(gpu_ctx, s, filt)
        o = [(N.OPTION_FAST_MATH, 1)]                 # (the MCM renderer's option; the other renderers have no fast variant)
        same(render(gpu_ctx, a, 'mcm', tf=tf, options=o), render(gpu_ctx, b, 'mcm', tf=tf, options=o), 'fast math mcm %s' % filt)
        for kind in ('mip', 'mcm'):
            p = ((4,), {'fused': True})
            same(render(gpu_ctx, a, kind, tf=tf, play=p), render(gpu_ctx, b, kind, tf=tf, play=p), 'play fused %s %s' % (kind, filt))
        p = ((4,), {'frames': True})
        same(render(gpu_ctx, a, 'mcm', tf=tf, play=p), render(gpu_ctx, b, 'mcm', tf=tf, play=p), 'frame sequence mcm %s' % filt)
        for v in (a, b):
            v.set_wide_tables(True)
        for kind in ('mip', 'mcm'):
            same(render(gpu_ctx, a, kind, tf=tf), render(gpu_ctx, b, kind, tf=tf), 'wide tables %s %s' % (kind, filt))
        a.destroy(); b.destroy()
    s2 = signed_volume(channels=2)
    a, b = twins(gpu_ctx, s2, 'linear')
    tf2 = colour_tf(64, 48)
    o = [(N.OPTION_FAST_MATH, 1)]
    same(render(gpu_ctx, a, 'mcm', tf=tf2, options=o), render(gpu_ctx, b, 'mcm', tf=tf2, options=o), 'RG fast math mcm')
    a.destroy(); b.destroy()


@pytest.mark.timeout(300)
def test_snorm_mcm_at_1080p_default_streams(gpu_ctx):
    s = signed_volume(dims=(45, 38, 51))
    a, b = twins(gpu_ctx, s, 'linear')
    tf = colour_tf(256)
    same(render(gpu_ctx, a, 'mcm', 1920, 1080, tf=tf), render(gpu_ctx, b, 'mcm', 1920, 1080, tf=tf), 'mcm 1080p')
    a.destroy(); b.destroy()


@pytest.mark.timeout(300)
def test_snorm_mip_against_the_oracle(gpu_ctx, oracle):
    s = signed_volume()
    a = vpt_amd.Volume.from_array(gpu_ctx, s, 'linear', snorm=True)
    w, h = 120, 90
    r = vpt_amd.MIPRenderer(gpu_ctx, a, default_camera(w / h), None, {'resolution': (w, h), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
    r.steps = 50
    r.reset()
    for _ in range(2):
        r.render()
    acc = r.read(N.BUFFER_ACCUM)
    r.destroy()
    m = mvp_inverse_matrix(default_camera(w / h), Transform(Node()))
    o = oracle.OracleRenderer('mip', oracle.OracleScene(np.ascontiguousarray(snorm(s)), 'linear'), w, h)
    o.reset(oracle.make_frame(w, h, m))
    g = GoldenRatioRng()
    for _ in range(2):
        o.render(oracle.make_frame(w, h, m, steps=50, offset=np.float32(g())))
    assert (acc.reshape(-1) == o.acc).all() and acc.max() > 0
    a.destroy()


@pytest.mark.timeout(60)
def test_snorm_storage_is_one_byte_per_channel(gpu_ctx):
    for dims in (DIMS, (64, 64, 64)):
        s1 = signed_volume(dims=dims)
        a = vpt_amd.Volume.from_array(gpu_ctx, s1, snorm=True)
        u = vpt_amd.Volume.from_array(gpu_ctx, s1.view(np.uint8))
        f = vpt_amd.Volume.from_array(gpu_ctx, snorm(s1))
        assert a.bricked_bytes() == u.bricked_bytes() and 4 * a.bricked_bytes() == f.bricked_bytes()
        s2 = signed_volume(dims=dims, channels=2)
        a2 = vpt_amd.Volume.from_array(gpu_ctx, s2, snorm=True)
        u2 = vpt_amd.Volume.from_array(gpu_ctx, s2.view(np.uint8))
        assert a2.bricked_bytes() == u2.bricked_bytes()
        for v in (a, u, f, a2, u2):
            v.destroy()


# ---- packed formats ----------------------------------------------------------------------------------------------------------
PACKED = {  # native format: (type, format, internalFormat, word dtype)
    N.FORMAT_RGB565: (R.GL_UNSIGNED_SHORT_5_6_5, R.GL_RGB, R.GL_RGB565, np.uint16),
    N.FORMAT_RGBA4: (R.GL_UNSIGNED_SHORT_4_4_4_4, R.GL_RGBA, R.GL_RGBA4, np.uint16),
    N.FORMAT_RGB5_A1: (R.GL_UNSIGNED_SHORT_5_5_5_1, R.GL_RGBA, R.GL_RGB5_A1, np.uint16),
    N.FORMAT_RGB10_A2: (R.GL_UNSIGNED_INT_2_10_10_10_REV, R.GL_RGBA, R.GL_RGB10_A2, np.uint32),
    N.FORMAT_R11F_G11F_B10F: (R.GL_UNSIGNED_INT_10F_11F_11F_REV, R.GL_RGB, R.GL_R11F_G11F_B10F, np.uint32),
    N.FORMAT_RGB9_E5: (R.GL_UNSIGNED_INT_5_9_9_9_REV, R.GL_RGB, R.GL_RGB9_E5, np.uint32),
}


def packed_volume(gl, words, fmt, filt):
    t, f, i, _ = PACKED[fmt]
    v = vpt_amd.Volume(gl, BVPReader(BlobLoader(make_bvp_typed(words, f, i, t, CUTS if words.shape == DIMS else ((), (), ())))))
    v.load(); v.setFilter(filt)
    return v


def words_of(fmt):
    if PACKED[fmt][3] == np.uint16:
        return np.arange(1 << 16, dtype=np.uint16).reshape(1, 256, 256)          # every 16-bit word
    rng = np.random.default_rng(fmt)
    w = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    uf11 = lambda e, m: (e << 6) | m
    edges = [0, 0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 1, 1 << 11, 1 << 22]
    if fmt == N.FORMAT_R11F_G11F_B10F:      # denormals, the largest finite, Inf, NaN in each channel
        for e, m in ((0, 1), (0, 63), (1, 0), (30, 63), (31, 0), (31, 1), (31, 63), (15, 0)):
            edges += [uf11(e, m), uf11(e, m) << 11, (uf11(e, m) << 11) | uf11(e, m), uf11(e, m) << 22]
    w[:len(edges)] = [e & 0xFFFFFFFF for e in edges]
    return w.reshape(64, 128, 128)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", sorted(PACKED))
def test_packed_nearest_probes_equal_the_numpy_decode(gpu_ctx, fmt):
    words = words_of(fmt)
    d, h, w = words.shape
    a = packed_volume(gpu_ctx, words, fmt, 'nearest')
    rg = decode_packed(words, fmt)
    b = vpt_amd.Volume.from_array(gpu_ctx, rg, 'nearest')
    ra = vpt_amd.MIPRenderer(gpu_ctx, a, default_camera(1.0), None, {'resolution': (8, 8)})
    rb = vpt_amd.MIPRenderer(gpu_ctx, b, default_camera(1.0), None, {'resolution': (8, 8)})
    tf = colour_tf(256, 256)
    ra.setTransferFunction(tf); rb.setTransferFunction(tf)
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing='ij')
    centres = np.stack([(x + 0.5) / w, (y + 0.5) / h, (z + 0.5) / d], axis=-1).reshape(-1, 3).astype(np.float32)
    pa, pb = ra.probe_sample(centres), rb.probe_sample(centres)
    assert np.array_equal(pa, pb, equal_nan=True), "NEAREST probes at texel centres"
    ra.destroy(); rb.destroy(); a.destroy(); b.destroy()


@pytest.mark.timeout(300)
@pytest.mark.parametrize("fmt", sorted(PACKED))
def test_packed_renders_like_rg32f(gpu_ctx, fmt):
    """MIP, EAM, MCM through a BVP with partial blocks, and through upload_block_device, against the RG32F volume of the decoded texels"""
    import torch
    rng = np.random.default_rng(100 + fmt)
    bits = 16 if PACKED[fmt][3] == np.uint16 else 32
    words = rng.integers(0, 1 << bits, size=DIMS, dtype=np.uint64).astype(PACKED[fmt][3])
    if fmt == N.FORMAT_R11F_G11F_B10F:      # finite texels of both ranges (exponents 0..16), so that the atlas stays on
        words = (words & ~np.uint32((31 << 6) | (31 << 17))) | (rng.integers(0, 17, size=DIMS).astype(np.uint32) << 6) | \
                (rng.integers(0, 17, size=DIMS).astype(np.uint32) << 17)
    if fmt == N.FORMAT_RGB9_E5:
        words = (words & np.uint32(0x07FFFFFF)) | (rng.integers(0, 25, size=DIMS).astype(np.uint32) << 27)
    rg = decode_packed(words, fmt)
    tf = colour_tf(64, 48)
    for filt in ('linear', 'nearest'):
        a = packed_volume(gpu_ctx, words, fmt, filt)
        b = vpt_amd.Volume.from_array(gpu_ctx, rg, filt)
        # the same volume uploaded from device memory, in three blocks with partial x-y extents
        d, h, w = DIMS
        t, f, i, _ = PACKED[fmt]
        dev = vpt_amd.Volume(gpu_ctx, BVPReader(BlobLoader(make_bvp_typed(np.zeros_like(words), f, i, t, ((), (), ()))))); dev.load(); dev.setFilter(filt)
        for (x0, x1), (y0, y1) in (((0, 9), (0, h)), ((9, w), (0, 11)), ((9, w), (11, h))):
            blk = torch.from_numpy(np.ascontiguousarray(words[:, y0:y1, x0:x1]).view(np.int16 if bits == 16 else np.int32)).cuda()
            torch.cuda.synchronize()
            dev.upload_block_device(x0, y0, 0, x1 - x0, y1 - y0, d, blk.data_ptr(), blk.numel() * blk.element_size())
            del blk
        for kind in ('mip', 'eam', 'mcm'):
            want = render(gpu_ctx, b, kind, tf=tf)
            same(render(gpu_ctx, a, kind, tf=tf), want, 'BVP %d %s %s' % (fmt, kind, filt))
            same(render(gpu_ctx, dev, kind, tf=tf), want, 'device upload %d %s %s' % (fmt, kind, filt))
        for v in (a, b, dev):
            v.destroy()


@pytest.mark.timeout(60)
def test_unfilterable_combinations_still_raise(gpu_ctx):
    vol = np.zeros((4, 4, 4), np.uint8)
    for t, f, i in ((R.GL_BYTE, R.GL_RED, 0x8231), (R.GL_BYTE, R.GL_RED, 33322), (R.GL_UNSIGNED_INT_2_10_10_10_REV, R.GL_RGBA, 0x906F),
                    (R.GL_UNSIGNED_SHORT_5_6_5, R.GL_RGBA, R.GL_RGB565), (0x84FA, 0x84F9, 0x88F0), (5124, R.GL_RED, 0x8235)):
        v = vpt_amd.Volume(gpu_ctx, BVPReader(BlobLoader(make_bvp_typed(vol, f, i, t, ((), (), ())))))
        with pytest.raises(RuntimeError, match="Unknown volume datatype"):
            v.load()
