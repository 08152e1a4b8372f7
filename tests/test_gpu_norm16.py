"""GPU: 16-bit normalised volumes (EXT_texture_norm16: R16, RG16, R16_SNORM, RG16_SNORM; sampler variant VPT_V_NORM16 = 512) against the
R32F / RG32F volume of their decoded texels, bit for bit: probes, every buffer of every renderer under every filter, the play modes, wide
tables, fast math, the MCM tile classes with and without the boundary atlas.  The R32F volumes are held to the oracle by the rest of the
suite (and here once more for MIP and MCM), so this equality is the parity chain (GL: convert each tap, then filter)."""
import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd import readers as R
from vpt_amd.loaders import BlobLoader
from vpt_amd.readers import BVPReader
from vpt_amd.scene import Transform, Node, default_camera, mvp_inverse_matrix
from vpt_amd.synthetic import sphere_volume, colour_tf, ramp_tf, GoldenRatioRng

from test_gpu_readers import make_bvp_typed
from test_gpu_volume_formats import render, same, CLASSES

pytestmark = pytest.mark.gpu

DIMS = (33, 47, 61)                      # depth, height, width: odd, not a multiple of the 4^3 bricks
CUTS = ((25,), (13, 30), (9, 20))        # BVP block edges (x, y, z): blocks end mid-brick
FILTERS = ('nearest', 'linear', 'quasicubic')
EXTREMES_U = (0, 1, 2, 32767, 32768, 65534, 65535)
EXTREMES_S = (-32768, -32767, -1, 0, 1, 32766, 32767)


def decode(c):
    """the R32F texels of a uint16 (UNORM: c / 65535) or int16 (SNORM: max(c / 32767, -1)) array, exactly (tests/test_norm16_host.py)"""
    c = np.asarray(c)
    if c.dtype == np.uint16:
        return (c.astype(np.float64) / 65535.0).astype(np.float32)
    return np.maximum(c.astype(np.float64) / 32767.0, -1.0).astype(np.float32)


def field(dims=DIMS, signed=False, channels=1, seed=7):
    """a noisy sphere spread over the whole 16-bit range (each extreme value occurs, in the first texels); a random second channel"""
    base = sphere_volume(0, noise=45.0, dims=dims).astype(np.int64) * 257 + np.random.default_rng(seed).integers(0, 257, size=dims)
    base = np.clip(base, 0, 65535)
    if signed:
        base = base - 32768
    out = base.astype(np.int16 if signed else np.uint16)
    flat = out.reshape(-1)
    ex = EXTREMES_S if signed else EXTREMES_U
    flat[:len(ex)] = ex
    flat[-len(ex):] = ex
    if channels == 1:
        return out
    rng = np.random.default_rng(seed + 1)
    lo, hi = (-32768, 32768) if signed else (0, 65536)
    multi = rng.integers(lo, hi, size=dims + (channels,)).astype(out.dtype)
    multi[..., 0] = out
    return multi


def twins(ctx, c, filt):
    """(16-bit volume, R32F / RG32F volume of the decoded texels)"""
    return vpt_amd.Volume.from_array(ctx, c, filt, norm16=True), vpt_amd.Volume.from_array(ctx, decode(c), filt)


def norm16_context():
    """a context of its own that has enabled EXT_texture_norm16 (the session's context must keep rejecting 16-bit manifests)"""
    ctx = vpt_amd.Context(0)
    assert ctx.getExtension('EXT_texture_norm16')
    return ctx


def probe_positions(dims, rng):
    d, h, w = dims
    z, y, x = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing='ij')
    centres = np.stack([(x + 0.5) / w, (y + 0.5) / h, (z + 0.5) / d], axis=-1).reshape(-1, 3).astype(np.float32)
    inside = rng.uniform(0, 1, size=(30000, 3)).astype(np.float32)
    # the faces, edges and corners of the cube and just inside / outside them (the apron of the last bricks)
    e = np.array([0.0, 1e-7, 0.5 / w, 1.0 / w, 0.5, 1 - 1.0 / w, 1 - 0.5 / w, 1 - 1e-7, 1.0], np.float32)
    edges = np.stack(np.meshgrid(e, e, e, indexing='ij'), axis=-1).reshape(-1, 3)
    outside = rng.uniform(-0.4, 1.4, size=(30000, 3)).astype(np.float32)
    return centres, np.concatenate([inside, edges]), outside


@pytest.mark.timeout(300)
@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("channels", [1, 2])
def test_probes_equal_the_r32f_probes(gpu_ctx, signed, channels):
    c = field(signed=signed, channels=channels)
    rng = np.random.default_rng(11)
    centres, inside, outside = probe_positions(DIMS, rng)
    tf = colour_tf(256) if channels == 1 else colour_tf(64, 48)
    for filt in FILTERS:
        a, b = twins(gpu_ctx, c, filt)
        ra = vpt_amd.MIPRenderer(gpu_ctx, a, default_camera(1.0), None, {'resolution': (8, 8)})
        rb = vpt_amd.MIPRenderer(gpu_ctx, b, default_camera(1.0), None, {'resolution': (8, 8)})
        for r in (ra, rb):
            r.setTransferFunction(tf)
        what = '%s%s %s' % ('SNORM ' if signed else '', channels, filt)
        same([ra.probe_sample(centres), ra.probe_sample(inside), ra.probe_sample(outside)],
             [rb.probe_sample(centres), rb.probe_sample(inside), rb.probe_sample(outside)], 'probes %s' % what)
        oob = outside[((outside > 1) | (outside < 0)).any(axis=1)]
        same([ra.probe_sample_boundary(oob)], [rb.probe_sample_boundary(oob)], 'boundary atlas %s' % what)
        same([ra.probe_sample_boundary(oob)], [ra.probe_sample(oob)], 'atlas = bricks %s' % what)
        if filt == 'nearest' and channels == 1:        # the extremes at texel centres: c = 0 .. 65535 / -32768 (reads -1) .. 32767
            got = ra.probe_sample(centres)
            assert np.array_equal(got, rb.probe_sample(centres))
        ra.destroy(); rb.destroy(); a.destroy(); b.destroy()


@pytest.mark.timeout(300)
def test_extreme_texels_read_as_their_decoded_values(gpu_ctx):
    """a ramp transfer function makes the probe's alpha the sample itself: the five extremes of the issue, NEAREST at texel centres"""
    for signed, vals, want in ((False, [0, 65535, 32767, 1, 65534], None), (True, [-32768, -32767, 32767, 0, -1], None)):
        c = np.array(vals * 13, dtype=np.int16 if signed else np.uint16)[:64].reshape(4, 4, 4)
        a, b = twins(gpu_ctx, c, 'nearest')
        ra = vpt_amd.MIPRenderer(gpu_ctx, a, default_camera(1.0), None, {'resolution': (8, 8)})
        rb = vpt_amd.MIPRenderer(gpu_ctx, b, default_camera(1.0), None, {'resolution': (8, 8)})
        for r in (ra, rb):
            r.setTransferFunction(ramp_tf(256))
        z, y, x = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing='ij')
        centres = np.stack([(x + 0.5) / 4, (y + 0.5) / 4, (z + 0.5) / 4], axis=-1).reshape(-1, 3).astype(np.float32)
        same([ra.probe_sample(centres)], [rb.probe_sample(centres)], 'extremes')
        if signed:
            assert decode(np.array([-32768], np.int16))[0] == -1.0 and decode(np.array([-32767], np.int16))[0] == -1.0
        ra.destroy(); rb.destroy(); a.destroy(); b.destroy()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("signed", [False, True])
def test_r16_renders_like_r32f_every_renderer(gpu_ctx, filt, signed):
    c = field(signed=signed)
    a, b = twins(gpu_ctx, c, filt)
    tf = colour_tf(256)
    for kind in CLASSES:
        same(render(gpu_ctx, a, kind, tf=tf, passes=3), render(gpu_ctx, b, kind, tf=tf, passes=3), '%s %s %s' % (kind, filt, signed))
    a.destroy(); b.destroy()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("signed", [False, True])
def test_rg16_renders_like_rg32f_with_a_2d_transfer_function(gpu_ctx, signed):
    c = field(dims=(21, 19, 23), signed=signed, channels=2)
    tf = colour_tf(64, 48)
    for filt in FILTERS:
        a, b = twins(gpu_ctx, c, filt)
        for kind in CLASSES:
            same(render(gpu_ctx, a, kind, tf=tf), render(gpu_ctx, b, kind, tf=tf), 'RG %s %s %s' % (kind, filt, signed))
        a.destroy(); b.destroy()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("nch", [1, 2, 3, 4])
@pytest.mark.parametrize("signed", [False, True])
def test_manifests_on_an_enabled_context_render_like_from_array(signed, nch):
    """BVP manifests with partial blocks (R16 .. RGBA16, _SNORM): the first two channels, as RGB8 / RGBA8; equal to from_array"""
    ctx = norm16_context()
    c = field(dims=(23, 19, 21), signed=signed, channels=nch)
    fmt = {1: R.GL_RED, 2: R.GL_RG, 3: R.GL_RGB, 4: R.GL_RGBA}[nch]
    ifmt = {1: R.GL_R16_EXT, 2: R.GL_RG16_EXT, 3: R.GL_RGB16_EXT, 4: R.GL_RGBA16_EXT}[nch] if not signed else \
        {1: R.GL_R16_SNORM_EXT, 2: R.GL_RG16_SNORM_EXT, 3: R.GL_RGB16_SNORM_EXT, 4: R.GL_RGBA16_SNORM_EXT}[nch]
    gltype = R.GL_SHORT if signed else R.GL_UNSIGNED_SHORT
    tf = colour_tf(256) if nch == 1 else colour_tf(64, 48)
    for filt in ('linear', 'nearest'):
        a = vpt_amd.Volume(ctx, BVPReader(BlobLoader(make_bvp_typed(c, fmt, ifmt, gltype, ((9,), (11, 14), (7, 17)))))); a.load(); a.setFilter(filt)
        b = vpt_amd.Volume.from_array(ctx, np.ascontiguousarray(c if nch == 1 else c[..., :2]), filt, norm16=True)
        f = vpt_amd.Volume.from_array(ctx, decode(c if nch == 1 else c[..., :2]), filt)
        for kind in ('mip', 'eam', 'mcs', 'mcm'):
            want = render(ctx, f, kind, tf=tf)
            same(render(ctx, a, kind, tf=tf), want, 'BVP %d %s %s' % (nch, kind, filt))
            same(render(ctx, b, kind, tf=tf), want, 'from_array %d %s %s' % (nch, kind, filt))
        for v in (a, b, f):
            v.destroy()
    ctx.destroy()


@pytest.mark.timeout(300)
def test_manifests_raise_without_the_extension(gpu_ctx):
    ctx = vpt_amd.Context(0)
    c = field(dims=(4, 4, 4))
    archive = make_bvp_typed(c, R.GL_RED, R.GL_R16_EXT, R.GL_UNSIGNED_SHORT, ((), (), ()))
    v = vpt_amd.Volume(ctx, BVPReader(BlobLoader(archive)))
    with pytest.raises(RuntimeError, match="Unknown volume datatype"):
        v.load()
    assert ctx.getExtension('EXT_texture_norm16')
    v = vpt_amd.Volume(ctx, BVPReader(BlobLoader(archive)))
    v.load()
    assert v.ready and v.bricked_bytes() > 0
    for t, f, i in ((R.GL_UNSIGNED_SHORT, R.GL_RED, 0x8234), (R.GL_SHORT, R.GL_RED, R.GL_R16_EXT), (R.GL_UNSIGNED_SHORT, R.GL_RG, R.GL_R16_EXT)):
        bad = vpt_amd.Volume(ctx, BVPReader(BlobLoader(make_bvp_typed(c, f, i, t, ((), (), ())))))
        with pytest.raises(RuntimeError, match="Unknown volume datatype"):
            bad.load()
    v.destroy()
    ctx.destroy()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("signed", [False, True])
def test_wide_tables_fast_math_and_play_modes(gpu_ctx, signed):
    import torch
    tf = colour_tf(256)
    c = field(dims=(21, 19, 23), signed=signed)
    for filt in FILTERS:
        a, b = twins(gpu_ctx, c, filt)
        o = [(N.OPTION_FAST_MATH, 1)]
        same(render(gpu_ctx, a, 'mcm', tf=tf, options=o), render(gpu_ctx, b, 'mcm', tf=tf, options=o), 'fast math %s' % filt)
        for kind in ('mip', 'eam', 'mcs', 'mcm'):
            for p in (((4,), {'use_graph': False}), ((4,), {'fused': True})):
                same(render(gpu_ctx, a, kind, tf=tf, play=p), render(gpu_ctx, b, kind, tf=tf, play=p), 'play %s %s %s' % (p[1], kind, filt))
        for o in ((), ((N.OPTION_FAST_MATH, 1),)):
            p = ((4,), {'frames': True})
            same(render(gpu_ctx, a, 'mcm', tf=tf, options=o, play=p), render(gpu_ctx, b, 'mcm', tf=tf, options=o, play=p), 'frames %s %s' % (o, filt))
        # play_into: four frames into caller-owned device memory
        w, h = 61, 47
        frames = []
        for v in (a, b):
            r = vpt_amd.MCMRenderer(gpu_ctx, v, default_camera(w / h), None, {'resolution': (w, h), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
            r.setTransferFunction(tf)
            r.reset()
            target = torch.zeros(4 * w * h * 4, dtype=torch.float16, device='cuda')
            torch.cuda.synchronize()
            r.play_into(4, target.data_ptr(), w * h * 8)
            gpu_ctx.synchronize()
            frames.append(target.cpu().numpy().copy())
            r.destroy()
        same([frames[0]], [frames[1]], 'play_into %s' % filt)
        for v in (a, b):
            v.set_wide_tables(True)
        for kind in CLASSES:
            same(render(gpu_ctx, a, kind, tf=tf), render(gpu_ctx, b, kind, tf=tf), 'wide tables %s %s' % (kind, filt))
        o = [(N.OPTION_FAST_MATH, 1)]
        same(render(gpu_ctx, a, 'mcm', tf=tf, options=o), render(gpu_ctx, b, 'mcm', tf=tf, options=o), 'wide fast math %s' % filt)
        a.destroy(); b.destroy()
    c2 = field(dims=(21, 19, 23), signed=signed, channels=2)
    a, b = twins(gpu_ctx, c2, 'linear')
    for v in (a, b):
        v.set_wide_tables(True)
    tf2 = colour_tf(64, 48)
    for kind in CLASSES:
        same(render(gpu_ctx, a, kind, tf=tf2), render(gpu_ctx, b, kind, tf=tf2), 'RG wide tables %s' % kind)
    a.destroy(); b.destroy()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("signed", [False, True])
def test_mcm_1080p_tile_classes_with_and_without_the_atlas(gpu_ctx, signed):
    """default streams and tile classes: the HIT tiles through the 16-bit general kernel, the MISS tiles through the FLOAT MISS-tile kernel
    on the float atlas of the decoded texels.  Equal to the general pass and to the R32F twin, atlas on and off, with the MISS-tile check"""
    c = field(dims=(45, 38, 51), signed=signed)
    tf = colour_tf(256)
    for filt in FILTERS:
        a, b = twins(gpu_ctx, c, filt)
        for extra in ((), ((N.OPTION_VERIFY_TILE_CLASSES, 1),), ((N.OPTION_FAST_MATH, 1),)):
            r = vpt_amd.MCMRenderer(gpu_ctx, a, default_camera(1920 / 1080), None,
                                    {'resolution': (1920, 1080), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
            r.setTransferFunction(tf)
            for opt, val in extra:
                r.set_option(opt, val)
            r.extinction = 40
            r.reset()
            for _ in range(4):
                r.render()
            classes_on = [r.read(k) for k in (N.BUFFER_RENDER, N.BUFFER_MCM_POSITION, N.BUFFER_MCM_DIRECTION,
                                              N.BUFFER_MCM_TRANSMITTANCE, N.BUFFER_MCM_RADIANCE)] + [r.getTexture()]
            hit, miss, violations = r.tile_classes()
            r.destroy()
            assert hit > 0 and miss > 0 and violations == 0, (hit, miss, violations)
            general = render(gpu_ctx, a, 'mcm', 1920, 1080, tf=tf, options=extra + ((N.OPTION_TILE_CLASSES, 0),), passes=4)
            no_atlas = render(gpu_ctx, a, 'mcm', 1920, 1080, tf=tf, options=extra + ((N.OPTION_BOUNDARY_ATLAS, 0),), passes=4)
            twin = render(gpu_ctx, b, 'mcm', 1920, 1080, tf=tf, options=extra, passes=4)
            same(classes_on, general, '1080p classes = general pass %s %s' % (filt, extra))
            same(classes_on, no_atlas, '1080p atlas on = off %s %s' % (filt, extra))
            same(classes_on, twin, '1080p = R32F %s %s' % (filt, extra))
        a.destroy(); b.destroy()


@pytest.mark.timeout(600)
def test_mip_and_mcm_against_the_oracle(gpu_ctx, oracle):
    c = field(dims=(32, 32, 32))
    a = vpt_amd.Volume.from_array(gpu_ctx, c, 'linear', norm16=True)
    w, h = 96, 64
    m = mvp_inverse_matrix(default_camera(w / h), Transform(Node()))
    r = vpt_amd.MIPRenderer(gpu_ctx, a, default_camera(w / h), None, {'resolution': (w, h), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
    r.steps = 50
    r.reset()
    for _ in range(2):
        r.render()
    acc = r.read(N.BUFFER_ACCUM)
    r.destroy()
    o = oracle.OracleRenderer('mip', oracle.OracleScene(decode(c), 'linear'), w, h)
    o.reset(oracle.make_frame(w, h, m))
    g = GoldenRatioRng()
    for _ in range(2):
        o.render(oracle.make_frame(w, h, m, steps=50, offset=np.float32(g())))
    assert (acc.reshape(-1) == o.acc).all() and acc.max() > 0
    # MCM (as smoke() does for R8): the image and the radiance state
    tf = ramp_tf(64)
    r = vpt_amd.MCMRenderer(gpu_ctx, a, default_camera(w / h), None, {'resolution': (w, h), 'transform': Transform(Node()), 'rng': GoldenRatioRng()})
    r.setTransferFunction(tf)
    r.extinction = 6
    r.reset()
    o = oracle.OracleRenderer('mcm', oracle.OracleScene(decode(c), 'linear', tf=tf), w, h)
    mm = r._matrix()
    o.reset(oracle.make_frame(w, h, mm, seed=np.float32(GoldenRatioRng()())))
    for _ in range(2):
        r.render()
        u = r._u
        o.render(oracle.make_frame(w, h, mm, seed=u.rand_seed, extinction=u.extinction, anisotropy=u.anisotropy,
                                   max_bounces=u.max_bounces, mcm_steps=u.steps))
    assert (r.getTexture().view(np.uint16) == o.image_f16().view(np.uint16)).all()
    assert (r.read(N.BUFFER_MCM_RADIANCE).view(np.uint32) == o.state[3].reshape(h, w, 4).view(np.uint32)).all()
    r.destroy(); a.destroy()


@pytest.mark.timeout(120)
def test_storage_is_two_bytes_per_channel(gpu_ctx):
    for dims in (DIMS, (64, 64, 64), (5, 3, 2)):
        for channels in (1, 2):
            u8 = np.zeros(dims + ((2,) if channels == 2 else ()), np.uint8)
            vols = [vpt_amd.Volume.from_array(gpu_ctx, u8.astype(np.uint16), norm16=True),
                    vpt_amd.Volume.from_array(gpu_ctx, u8.astype(np.int16), norm16=True),
                    vpt_amd.Volume.from_array(gpu_ctx, u8),
                    vpt_amd.Volume.from_array(gpu_ctx, u8.astype(np.float32))]
            n16, s16, n8, n32 = (v.bricked_bytes() for v in vols)
            assert n16 == s16 and 2 * n16 == n32 and n16 == 2 * n8, (dims, channels, n16, s16, n8, n32)
            for v in vols:
                v.destroy()


@pytest.mark.timeout(300)
def test_device_upload_from_a_torch_tensor(gpu_ctx):
    """upload_block_device from torch int16 / uint16 memory, in blocks with partial x-y extents, equals from_array"""
    import torch
    tf = colour_tf(256)
    for signed in (False, True):
        c = field(signed=signed)
        d, h, w = DIMS
        want = vpt_amd.Volume.from_array(gpu_ctx, c, 'linear', norm16=True)
        dev = vpt_amd.Volume.from_array(gpu_ctx, np.zeros_like(c), 'linear', norm16=True)
        for (x0, x1), (y0, y1) in (((0, 9), (0, h)), ((9, w), (0, 11)), ((9, w), (11, h))):
            blk = torch.from_numpy(np.ascontiguousarray(c[:, y0:y1, x0:x1]).view(np.int16)).cuda()
            torch.cuda.synchronize()
            dev.upload_block_device(x0, y0, 0, x1 - x0, y1 - y0, d, blk.data_ptr(), blk.numel() * blk.element_size())
            del blk
        host = vpt_amd.Volume.from_array(gpu_ctx, np.zeros_like(c), 'linear', norm16=True)
        host.upload_block(0, 0, 0, torch.from_numpy(c.view(np.int16)).numpy())
        for kind in ('mip', 'mcm'):
            ref = render(gpu_ctx, want, kind, tf=tf)
            same(render(gpu_ctx, dev, kind, tf=tf), ref, 'device upload %s %s' % (signed, kind))
            same(render(gpu_ctx, host, kind, tf=tf), ref, 'host upload %s %s' % (signed, kind))
        for v in (want, dev, host):
            v.destroy()
