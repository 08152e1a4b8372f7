"""GPU: two volumes combined texel by texel (vpt_volume_combine) and compared (vpt_volume_compare) on the device.

The texels are held, byte for byte, to vpt_amd.combine_texels and the counts to vpt_amd.compare_stats, the numpy statements of the contract
(tests/test_combine_host.py holds those to loops over Python integers).  Parity chain to the oracle: volumes uploaded from the host are
held to the CPU oracle by the rest of the suite, so a derived volume must give byte-identical buffers to the volume uploaded from the numpy
statement's texels.

Both kernels stream over the linear index: a lane takes a group of 16 / sizeof(a's texel) consecutive voxels (16 byte texels, 8 16-bit
texels; Group<>::G in vpt_volume_combine.hip), a workgroup has 256 lanes and stream_grid caps the grid at 8192 workgroups, so one trip of
the grid covers 16 x 256 x 8192 = 33 554 432 byte voxels.  LONG = 3345 x 3345 x 3 = 33 567 075 voxels is the smallest such shape with three
odd-ish axes above that: 790 lanes take a second trip through the stride loop for byte texels (every lane does for 16-bit texels), and
33 567 075 mod 16 = 3, so the volume ends on a partial group for either width.  The small shapes: (3,1,5) is 15 voxels, the tail loop alone
for either group size; (16,1,1) exactly one byte group and no tail (two 16-bit groups); the others are odd everywhere."""
import ctypes as C

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.combine import STATS, combine_texels, compare_stats
from vpt_amd.loaders import BlobLoader
from vpt_amd.readers import BVPReader, RAWReader
from vpt_amd.synthetic import sphere_volume, colour_tf

from test_gpu_readers import make_bvp_typed
from test_gpu_volume_formats import render, same, PACKED
from test_gpu_pyramid import upload, whole
from test_combine_host import blends, mask_range, value_sets, DTYPES, NOISE

pytestmark = pytest.mark.gpu

GROUP_BYTES, LANES, GRID_CAP = 16, 256, 8192
LONG = (3345, 3345, 3)
assert LONG[0] * LONG[1] * LONG[2] > GROUP_BYTES * LANES * GRID_CAP and (LONG[0] * LONG[1] * LONG[2]) % GROUP_BYTES == 3
SHAPES = ((1, 1, 1), (3, 1, 5), (16, 1, 1), (17, 1, 3), (7, 5, 1), NOISE)


def differences(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d texels differ (%s), first at %s: %d, expected %d" % (len(bad), what, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def other_width(b, dtype):
    """b's texels in the other width: bytes widened by 257, 16-bit codes cut to their high byte"""
    return (b.astype(np.uint16) * 257) if dtype == np.uint8 else (b >> 8).astype(np.uint8)


def calls(dtype):
    """[(op, params)] of one sweep: every op, every blend of the contract's table"""
    M = int(np.iinfo(dtype).max)
    lo, hi = mask_range(dtype)
    return ([('mask', {'lo': lo, 'hi': hi, 'fill': M - 1}), ('min', {}), ('max', {}), ('absdiff', {}), ('pair', {})] +
            [('blend', {'wa': wa, 'wb': wb, 'offset': offset}) for wa, wb, offset in blends(M)])


# ---- the texels themselves ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
def test_combined_texels_equal_the_contract(gpu_ctx, dtype):
    for n, shape in enumerate(SHAPES):
        for name, a, b in value_sets(dtype, shape, seed=5 + n):
            va, vb = upload(gpu_ctx, a), upload(gpu_ctx, b)
            two = np.stack([b, a], axis=-1)
            vtwo = upload(gpu_ctx, two)
            wide = other_width(b, dtype)
            vwide, vwide_two = upload(gpu_ctx, wide), upload(gpu_ctx, np.stack([wide, wide[::-1, ::-1, ::-1]], axis=-1))
            what = "%s %s %s" % (np.dtype(dtype).name, shape, name)
            for op, params in calls(dtype):
                want = combine_texels(a, b, op, **params)
                out = va.combine(vb, op, **params)
                differences(whole(out), want, "%s %s %s" % (op, params, what))
                out.destroy()
                for channel in (0, 1):                            # a two-channel b, read whole, the channel taken in registers
                    out = va.combine(vtwo, op, channel=channel, **params)
                    differences(whole(out), combine_texels(a, two, op, channel=channel, **params), "%s channel %d %s" % (op, channel, what))
                    out.destroy()
                out = va.combine(va, op, **params)                # a is b
                differences(whole(out), combine_texels(a, a, op, **params), "%s of a with itself %s" % (op, what))
                out.destroy()
            lo, hi = mask_range(wide.dtype)                       # a mask of the other width, one and two channels
            out = va.mask(vwide, lo, hi, fill=3)
            differences(whole(out), combine_texels(a, wide, 'mask', lo=lo, hi=hi, fill=3), "mixed mask %s" % what)
            out.destroy()
            out = va.mask(vwide_two, lo, hi, fill=3, channel=1)
            differences(whole(out), combine_texels(a, wide[::-1, ::-1, ::-1], 'mask', lo=lo, hi=hi, fill=3), "mixed mask, channel 1 %s" % what)
            out.destroy()
            assert whole(va).tobytes() == a.tobytes() and whole(vb).tobytes() == b.tobytes() and whole(vtwo).tobytes() == two.tobytes(), "a source changed"
            for vol in (va, vb, vtwo, vwide, vwide_two):
                vol.destroy()


@pytest.mark.timeout(300)
def test_a_second_trip_through_the_stride_loop_and_a_partial_last_group(gpu_ctx):
    nx, ny, nz = LONG
    rng = np.random.default_rng(61)
    a = rng.integers(0, 256, size=(nz, ny, nx), dtype=np.uint8)
    b = rng.integers(0, 256, size=(nz, ny, nx), dtype=np.uint8)
    va, vb = upload(gpu_ctx, a), upload(gpu_ctx, b)
    for op, params in (('mask', {'lo': 64, 'hi': 191, 'fill': 7}), ('blend', {'wa': 77, 'wb': 151, 'offset': 3}), ('pair', {})):
        out = va.combine(vb, op, **params)
        got = whole(out)
        out.destroy()
        assert got.tobytes() == combine_texels(a, b, op, **params).tobytes(), op
    want = compare_stats(a, b, (64, 191), (100, 255))
    got = va.compare(vb, (64, 191), (100, 255))
    assert got == want
    va.destroy(); vb.destroy()
    a16, b16 = a.astype(np.uint16) * 255 + b, b.astype(np.uint16) * 251 + a      # 16-bit texels: groups of 8
    va, vb = upload(gpu_ctx, a16), upload(gpu_ctx, b16)
    out = va.absdiff(vb)
    got = whole(out)
    out.destroy()
    assert got.tobytes() == combine_texels(a16, b16, 'absdiff').tobytes()
    assert va.compare(vb) == compare_stats(a16, b16)
    va.destroy(); vb.destroy()


@pytest.mark.timeout(120)
def test_the_result_outlives_its_sources_and_two_runs_give_identical_bytes(gpu_ctx):
    nx, ny, nz = NOISE
    for dtype, fmt, pair_fmt in ((np.uint8, N.FORMAT_R8, N.FORMAT_RG8), (np.uint16, N.FORMAT_R16, N.FORMAT_RG16)):
        _, a, b = value_sets(dtype, NOISE, seed=67)[0]
        for op, params in calls(dtype):
            va, vb = upload(gpu_ctx, a, 'nearest'), upload(gpu_ctx, b)
            first, second = va.combine(vb, op, **params), va.combine(vb, op, **params)
            va.destroy(); vb.destroy()                            # before the read-back
            assert first.ready and first.modality['dimensions'] == {'width': nx, 'height': ny, 'depth': nz}
            assert first.native_format()[0] == (pair_fmt if op == 'pair' else fmt)
            got = whole(first)
            differences(got, combine_texels(a, b, op, **params), op)
            assert whole(second).tobytes() == got.tobytes()
            if op != 'pair':
                again = first.combine(second, 'absdiff')          # an ordinary volume: this entry again
                assert not whole(again).any()
                again.destroy()
            first.destroy(); second.destroy()


@pytest.mark.timeout(120)
def test_conveniences_are_combine(gpu_ctx):
    _, a, b = value_sets(np.uint8, NOISE, seed=71)[0]
    va, vb = upload(gpu_ctx, a), upload(gpu_ctx, b)
    for out, want in ((va.mask(vb, 10, 200, 5), combine_texels(a, b, 'mask', lo=10, hi=200, fill=5)), (va.minimum(vb), np.minimum(a, b)),
                      (va.maximum(vb), np.maximum(a, b)), (va.absdiff(vb), combine_texels(a, b, 'absdiff')),
                      (va.blend(vb, 256, -256, 128), combine_texels(a, b, 'blend', wa=256, wb=-256, offset=128)), (va.pair(vb), np.stack([a, b], axis=-1))):
        differences(whole(out), want, 'convenience')
        out.destroy()
    out, ms = va.combine_timed(vb, 'blend', wa=128, wb=128)
    differences(whole(out), combine_texels(a, b, 'blend', wa=128, wb=128), 'timed')
    assert isinstance(ms, float) and ms > 0.0
    out.destroy()
    for bad in (lambda: va.combine(vb, 'mean'), lambda: va.combine(vb, 'min', channel=1), lambda: va.blend(vb, 5000, 0), lambda: va.mask(vb, 3, 2),
                lambda: va.mask(vb, 0, 256), lambda: va.combine(vb, 'min', scale=2), lambda: va.combine(a, 'min')):
        with pytest.raises(ValueError):
            bad()
    va.destroy(); vb.destroy()


@pytest.mark.timeout(120)
def test_result_does_not_depend_on_the_sources_being_finalized(gpu_ctx):
    L = N.lib()
    for dtype, fmt in ((np.uint8, N.FORMAT_R8), (np.uint16, N.FORMAT_R16)):
        for nx in (32, 31):
            _, a, b = value_sets(dtype, (nx, 4, 3), seed=73)[0]
            ha, hb, out = C.c_void_p(), C.c_void_p(), C.c_void_p()
            for h, texels in ((ha, a), (hb, b)):
                N.check(L.vpt_volume_create(gpu_ctx._h, nx, 4, 3, fmt, C.byref(h)))
                N.check(L.vpt_volume_upload_block(h, 0, 0, 0, nx, 4, 3, texels.ctypes.data_as(C.c_void_p), texels.nbytes))      # no vpt_volume_finalize
            p = N.CombineParams(op=N.COMBINE_BLEND, wa=256, wb=-256, offset=100)
            N.check(L.vpt_volume_combine(ha, hb, C.byref(p), C.byref(out)))
            got = np.empty_like(a)
            N.check(L.vpt_volume_read_block(out, 0, 0, 0, nx, 4, 3, got.ctypes.data_as(C.c_void_p), got.nbytes))
            counts = (C.c_uint64 * 8)()
            N.check(L.vpt_volume_compare(ha, hb, 0, 0, 100, 50, 200, counts))
            for h in (out, ha, hb):
                L.vpt_volume_destroy(h)
            differences(got, combine_texels(a, b, 'blend', wa=256, wb=-256, offset=100), "%s %d" % (np.dtype(dtype).name, nx))
            want = compare_stats(a, b, (0, 100), (50, 200))
            assert [int(v) for v in counts] == [want[k] for k in STATS]


# ---- an ordinary volume ------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pair_and_blend_render_like_the_uploaded_texels(gpu_ctx, dtype):
    nx, ny, nz = NOISE
    v = sphere_volume(0, noise=45.0, dims=(nz, ny, nx))
    w = sphere_volume(0, noise=20.0, seed=77, dims=(nz, ny, nx))[::-1].copy()
    if dtype == np.uint16:
        v, w = v.astype(np.uint16) * 257, w.astype(np.uint16) * 251
    tf1, tf2 = colour_tf(256), colour_tf(64, 16)
    for filt in ('linear', 'nearest'):
        va, vb = upload(gpu_ctx, v, filt), upload(gpu_ctx, w, 'quasicubic')      # the result carries a's filter
        for op, params, tf in (('pair', {}, tf2), ('blend', {'wa': 160, 'wb': -96, 'offset': 20}, tf1)):
            want = combine_texels(v, w, op, **params)
            assert len(np.unique(want)) >= 32, "degenerate input"
            derived, twin = va.combine(vb, op, **params), upload(gpu_ctx, want, filt)
            for kind in ('mip', 'mcm'):
                fa = render(gpu_ctx, derived, kind, tf=tf)
                same(fa, render(gpu_ctx, twin, kind, tf=tf), '%s %s %s' % (op, kind, filt))
                pixels = np.ascontiguousarray(fa[-1]); pixels = pixels.reshape(-1, pixels.shape[-1])
                assert len(np.unique(pixels.view(np.uint16), axis=0)) >= 2, '%s: empty frame' % kind
            derived.destroy(); twin.destroy()
        va.destroy(); vb.destroy()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES)
def test_compositions_equal_their_numpy_chains(gpu_ctx, dtype):
    nx, ny, nz = NOISE
    M = int(np.iinfo(dtype).max)
    v = sphere_volume(0, noise=45.0, dims=(nz, ny, nx))
    if dtype == np.uint16:
        v = v.astype(np.uint16) * 257
    src = upload(gpu_ctx, v)
    # unsharp masking: 2 v - smooth(v)
    smoothed = src.smooth(1)
    sharp = src.blend(smoothed, 512, -256)
    want = combine_texels(v, vpt_amd.smooth_texels(v, 1), 'blend', wa=512, wb=-256)
    assert (want != v).mean() > 0.2, "the operation changes nothing"
    differences(whole(sharp), want, 'unsharp')
    sharp.destroy(); smoothed.destroy()
    # segment on the filtered copy, cut the original
    lo, hi = M // 3, M
    opened = src.open(1)
    found = opened.components(lo, hi)
    label = found.label()
    cut = src.mask(label, 1, M, channel=1)
    filtered = vpt_amd.rank_texels(v, 'open')
    ranks = vpt_amd.components_texels(filtered, lo, hi)[0]
    labels = vpt_amd.label_texels(filtered, ranks)
    want = combine_texels(v, labels, 'mask', lo=1, hi=M, channel=1)
    assert 0.02 < (want != 0).mean() < 0.98 and (want != filtered)[want != 0].any(), "degenerate input"
    differences(whole(cut), want, 'cut the original')
    for vol in (cut, label, opened, src):
        vol.destroy()
    found.destroy()


@pytest.mark.timeout(300)
def test_rendering_context_chain_equals_the_numpy_chain():
    nx, ny, nz = NOISE
    size = (16, 14, 12)                                           # w, h, d of the primary's grid after `resample`
    v = sphere_volume(0, noise=45.0, dims=(nz, ny, nx))
    m = sphere_volume(0, noise=10.0, seed=81, dims=(9, 11, 13))   # the second volume lies on another grid
    raw = lambda a: RAWReader(a.tobytes(), {'width': a.shape[2], 'height': a.shape[1], 'depth': a.shape[0], 'bits': 8})
    rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'resample': {'size': list(size)}, 'rank': 'median', 'gradient': 'sobel',
                                   'combine': {'reader': raw(m), 'op': 'mask', 'lo': 90, 'hi': 255, 'fill': 1, 'resample': 'nearest'}})
    try:
        rc.setVolume(raw(v))
        assert rc.volume.native_format()[0] == N.FORMAT_RG8
        tex = whole(rc.volume)
        # a library error keeps the context's old volume: sizes differ and no `resample` is named
        kept = rc.volume.texture.value
        rc.combine = vpt_amd.RenderingContext._combine_spec({'reader': raw(m), 'op': 'min'})
        with pytest.raises(vpt_amd.VptError, match="16x14x12.*13x11x9") as e:
            rc.setVolume(raw(v))
        assert e.value.code == N.ERR_INVALID and rc.volume.texture.value == kept and whole(rc.volume).tobytes() == tex.tobytes()
    finally:
        rc.destroy()
    shape = (size[2], size[1], size[0])
    primary = vpt_amd.resample_texels(v, shape, 'filtered')
    second = vpt_amd.resample_texels(m, shape, 'nearest')
    masked = combine_texels(primary, second, 'mask', lo=90, hi=255, fill=1)
    assert 0.05 < (masked != primary).mean() < 0.95, "degenerate input"
    value = vpt_amd.rank_texels(masked, 'median')
    g = vpt_amd.gradient_magnitude(value, 'sobel', 1)
    assert tex[..., 0].tobytes() == value.tobytes() and tex[..., 1].tobytes() == g.tobytes()
    # 'pair' runs where the gradient runs; a caller's volume stays the caller's; a primary that is not R8 / R16 is left as it is
    ctx_rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'smooth': 1})
    try:
        theirs = upload(ctx_rc.gl, v[::-1].copy())
        ctx_rc.combine = vpt_amd.RenderingContext._combine_spec({'volume': theirs, 'op': 'pair'})
        ctx_rc.setVolume(raw(v))
        tex = whole(ctx_rc.volume)
        assert tex[..., 0].tobytes() == vpt_amd.smooth_texels(v, 1).tobytes() and tex[..., 1].tobytes() == v[::-1].tobytes()
        assert theirs.ready and whole(theirs).tobytes() == v[::-1].tobytes()
        f = np.random.default_rng(59).standard_normal((nz, ny, nx)).astype(np.float32)
        ctx_rc.setVolume(RAWReader(f.astype('<f4').tobytes(), {'width': nx, 'height': ny, 'depth': nz, 'bits': 32}))
        assert ctx_rc.volume.native_format()[0] == N.FORMAT_R32F and whole(ctx_rc.volume).tobytes() == f.tobytes()
        theirs.destroy()
    finally:
        ctx_rc.destroy()
    with pytest.raises(ValueError, match="second channel"):
        vpt_amd.RenderingContext({'gradient': 'central', 'combine': {'reader': raw(m), 'op': 'pair'}})


# ---- compare -----------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_compare_counts_equal_the_contract(gpu_ctx):
    for dtype in DTYPES:
        for n, shape in enumerate(SHAPES):
            for name, a, b in value_sets(dtype, shape, seed=83 + n):
                wide = other_width(b, dtype)
                va, vb, vwide, vtwo = upload(gpu_ctx, a), upload(gpu_ctx, b), upload(gpu_ctx, wide), upload(gpu_ctx, np.stack([a, b], axis=-1))
                ra, rb, rw = mask_range(dtype), (0, int(np.iinfo(dtype).max) // 2), mask_range(wide.dtype)
                what = "%s %s %s" % (np.dtype(dtype).name, shape, name)
                assert va.compare(vb, ra, rb) == compare_stats(a, b, ra, rb), what
                assert va.compare(vb) == compare_stats(a, b), what
                assert va.compare(vwide, ra, rw) == compare_stats(a, wide, ra, rw), "mixed widths " + what
                assert va.compare(vtwo, ra, rb, channel=1) == compare_stats(a, b, ra, rb), "channel 1 " + what
                got = va.compare(va, ra, ra)                      # identical volumes
                assert got == compare_stats(a, a, ra, ra) and got['differing'] == got['max_abs'] == got['sum_sq'] == 0 and got['psnr'] is None
                assert va.compare(vtwo, ra, ra, channel=0) == got
                assert va.compare(vb, ra, rb) == va.compare(vb, ra, rb), "two runs differ"
                for vol in (va, vb, vwide, vtwo):
                    vol.destroy()
    _, a, b = value_sets(np.uint16, NOISE, seed=89)[0]
    va, vb = upload(gpu_ctx, a), upload(gpu_ctx, b)
    got = va.compare(vb, (0x4000, 0xFFFF), (0x6000, 0xFFFF))
    assert got['sum_sq'] > 2 ** 40 and 0 < got['both'] < got['in_b'] < got['in_a'] < a.size and 0.0 < got['jaccard'] < got['dice'] < 1.0
    assert got['mse'] == got['sum_sq'] / a.size and got['dice'] == 2 * got['both'] / (got['in_a'] + got['in_b'])
    empty = va.compare(vb, (70000, 80000), (70000, 80000))       # ranges above every code: no denominator
    assert empty['in_a'] == empty['in_b'] == 0 and empty['dice'] is None and empty['jaccard'] is None
    va.destroy(); vb.destroy()


# ---- errors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_every_refusal_names_what_it_refuses(gpu_ctx):
    L = N.lib()
    words = np.random.default_rng(1).integers(0, 1 << 16, size=(4, 4, 4), dtype=np.uint64).astype(np.uint16)
    t, f, i, _ = PACKED[N.FORMAT_RGB565]
    packed = vpt_amd.Volume(gpu_ctx, BVPReader(BlobLoader(make_bvp_typed(words, f, i, t, ((), (), ()))))); packed.load()
    r8, r16 = upload(gpu_ctx, np.zeros((4, 4, 4), np.uint8)), upload(gpu_ctx, np.zeros((4, 4, 4), np.uint16))
    rg8 = upload(gpu_ctx, np.zeros((4, 4, 4, 2), np.uint8))
    out, counts = C.c_void_p(), (C.c_uint64 * 8)()

    def refused(a, b, code, names, **fields):
        p = N.CombineParams(**fields)
        assert L.vpt_volume_combine(a.texture, b.texture, C.byref(p), C.byref(out)) == code, (names, L.vpt_last_error())
        message = L.vpt_last_error().decode()
        for name in names:
            assert name in message, (name, message)

    def refused_by_both(a, b, code, names, b_channel=0):
        refused(a, b, code, names, op=N.COMBINE_MIN, b_channel=b_channel)
        assert L.vpt_volume_compare(a.texture, b.texture, b_channel, 0, 1, 0, 1, counts) == code
        message = L.vpt_last_error().decode()
        for name in names:
            assert name in message, (name, message)

    sources = ((packed, "RGB565"), (upload(gpu_ctx, np.zeros((4, 4, 4), np.float32)), "R32F"), (upload(gpu_ctx, np.zeros((4, 4, 4), np.int8)), "R8_SNORM"),
               (upload(gpu_ctx, np.zeros((4, 4, 4), np.int16)), "R16_SNORM"))
    for vol, name in sources:                                     # formats, as a and as b
        refused_by_both(vol, r8, N.ERR_UNSUPPORTED, (name, "window"))
        refused_by_both(r8, vol, N.ERR_UNSUPPORTED, (name, "window"))
        with pytest.raises(vpt_amd.VptError, match=r"\b%s\b" % name) as e:
            r8.minimum(vol)
        assert e.value.code == N.ERR_UNSUPPORTED
        vol.destroy()
    refused_by_both(rg8, r8, N.ERR_UNSUPPORTED, ("RG8",))          # a two-channel a
    for op in (N.COMBINE_MIN, N.COMBINE_MAX, N.COMBINE_ABSDIFF, N.COMBINE_BLEND, N.COMBINE_PAIR):      # widths differ: the mask alone takes that
        refused(r8, r16, N.ERR_UNSUPPORTED, ("R8", "R16", "MASK"), op=op)
        refused(r16, rg8, N.ERR_UNSUPPORTED, ("R16", "RG8"), op=op)
    other_size = upload(gpu_ctx, np.zeros((4, 5, 6), np.uint8))
    refused_by_both(r8, other_size, N.ERR_INVALID, ("4x4x4", "6x5x4", "resample"))
    other_size.destroy()
    second = vpt_amd.Context(0)
    try:
        elsewhere = upload(second, np.zeros((4, 4, 4), np.uint8))
        refused_by_both(r8, elsewhere, N.ERR_INVALID, ("context",))
        elsewhere.destroy()
    finally:
        second.destroy()
    for op in (-1, 6):
        refused(r8, r8, N.ERR_INVALID, (str(op),), op=op)
    for wa, wb in ((4097, 0), (0, -4097)):
        refused(r8, r8, N.ERR_INVALID, (str(wa), str(wb), "4096"), op=N.COMBINE_BLEND, wa=wa, wb=wb)
    for offset in (65536, -65536):
        refused(r8, r8, N.ERR_INVALID, (str(offset),), op=N.COMBINE_BLEND, wa=1, wb=1, offset=offset)
    refused(r8, r16, N.ERR_INVALID, ("fill 256", "255"), op=N.COMBINE_MASK, lo=0, hi=65535, fill=256)
    refused(r16, r8, N.ERR_INVALID, ("256", "255"), op=N.COMBINE_MASK, lo=0, hi=256, fill=65535)
    refused(r8, r8, N.ERR_INVALID, ("[9, 3]",), op=N.COMBINE_MASK, lo=9, hi=3)
    refused_by_both(r8, r8, N.ERR_INVALID, ("channel 1", "R8"), b_channel=1)
    refused_by_both(r8, rg8, N.ERR_INVALID, ("channel 2",), b_channel=2)
    p, ms = N.CombineParams(), C.c_double()
    for args in ((None, r8.texture, C.byref(p), C.byref(out)), (r8.texture, None, C.byref(p), C.byref(out)), (r8.texture, r8.texture, None, C.byref(out)),
                 (r8.texture, r8.texture, C.byref(p), None)):
        assert L.vpt_volume_combine(*args) == N.ERR_INVALID and b"null" in L.vpt_last_error()
        assert L.vpt_volume_combine_timed(*(args + (C.byref(ms),))) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    assert L.vpt_volume_combine_timed(r8.texture, r8.texture, C.byref(p), C.byref(out), None) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    for args in ((None, r8.texture, counts), (r8.texture, None, counts), (r8.texture, r8.texture, None)):
        assert L.vpt_volume_compare(args[0], args[1], 0, 0, 1, 0, 1, args[2]) == N.ERR_INVALID and b"null" in L.vpt_last_error()
    for vol in (r8, r16, rg8):
        vol.destroy()
