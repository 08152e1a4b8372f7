"""GPU: the exact squared Euclidean distance transform of a value range of a volume on the device (vpt_volume_distance and the
vpt_distance_* family).

Everything the handle gives (squared(), info, within, channel, and the source's texels unchanged) is held, byte for byte, to
vpt_amd.distance_squared_texels / within_texels / channel_texels, the numpy statement of the contract (tests/test_distance_host.py holds
that to a brute force in Python integers and to scipy).  Parity chain to the oracle: volumes uploaded from the host are held to the CPU
oracle by the rest of the suite, so a `channel` volume must give byte-identical buffers to the volume uploaded from the numpy statement's
texels.

The x pass works on segments of 64 voxels of a row and carries the nearest seed across segments; the y and z passes run one lane per line
with the lanes along x.  So the shapes that matter are a row of one voxel less than, exactly, and one voxel more than a segment, a row of
two segments and a voxel (a carry across a whole segment), one live lane (nx = 1), and the longest line the library admits (4096)."""
import ctypes as C

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.distance import NONE, check_radius
from vpt_amd.loaders import BlobLoader
from vpt_amd.readers import BVPReader, RAWReader
from vpt_amd.synthetic import colour_tf

from test_gpu_readers import make_bvp_typed
from test_gpu_volume_formats import render, same, PACKED
from test_gpu_pyramid import upload, whole
from test_distance_host import blobs, code_range, noise

pytestmark = pytest.mark.gpu

NOISE = (23, 19, 21)                                                # nx, ny, nz: every axis odd
SHAPES = (NOISE, (1, 1, 1), (7, 5, 1), (63, 3, 2), (64, 3, 2), (65, 3, 2), (129, 2, 3), (1, 70, 1), (1, 1, 70), (130, 9, 5))
BLOB_SHAPES = ((33, 29, 31), (65, 17, 9))
DTYPES = (np.uint8, np.uint16)
SEEDS = ('range', 'rest')
DENSITY = 0.03

_statements = {}


def statement(key, a, lo, hi, seeds):
    """the numpy statement's d2, computed once per input and left unchanged"""
    key = (key, a.dtype.name, a.shape, lo, hi, seeds)
    if key not in _statements:
        _statements[key] = vpt_amd.distance_squared_texels(a, lo, hi, seeds)
        _statements[key].setflags(write=False)
    return _statements[key]


def differences(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d values differ (%s), first at %s: %d, expected %d" % (len(bad), what, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def check(ctx, a, lo, hi, seeds, what, d2=None, steps=3):
    """transforms `a` on the device and holds everything the handle gives to the numpy statement; returns the statement's d2"""
    what = "%s %s %s [%d, %d] %s" % (what, a.dtype.name, a.shape[::-1], lo, hi, seeds)
    if d2 is None:
        d2 = vpt_amd.distance_squared_texels(a, lo, hi, seeds)
    finite = d2[d2 != NONE]
    src = upload(ctx, a)
    found = src.distance(lo, hi, seeds)
    differences(found.squared(), d2, what + ': squared')
    seed = ((a >= lo) & (a <= hi)) != (seeds == 'rest')
    assert found.info == {'seeds': int(seed.sum()), 'largest': int(finite.max()) if finite.size else 0}, what + ': info'
    half = max(int(finite.max()) // 2 if finite.size else 0, 1)
    near, pair = found.within(1, half, 3), found.channel(steps)
    differences(whole(near), vpt_amd.within_texels(a, d2, 1, half, 3), what + ': within')
    differences(whole(pair), vpt_amd.channel_texels(a, d2, steps), what + ': channel')
    assert whole(src).tobytes() == a.tobytes(), what + ": the source's texels changed"
    for thing in (near, pair, found, src):
        thing.destroy()
    return d2


def row_distances(a, lo, hi):
    """d2 of every voxel within its own row only: what the x pass alone gives"""
    nz, ny, nx = a.shape
    rows = [vpt_amd.distance_squared_texels(a[z, y].reshape(1, 1, nx), lo, hi) for z in range(nz) for y in range(ny)]
    return np.concatenate(rows).reshape(a.shape)


def blob_texels(dtype, shape, seed):
    """(texels, code): blobs at `code` over low noise, in the dtype"""
    b = blobs(shape, seed)
    return (b, 200) if dtype == np.uint8 else (b.astype(np.uint16) * 257, 200 * 257)


# ---- noise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("seeds", SEEDS)
def test_noise_equals_the_contract(gpu_ctx, seeds, dtype):
    lo, hi = code_range(dtype, DENSITY)
    for n, shape in enumerate(SHAPES):
        a = noise(dtype, shape, seed=101 + n)
        d2 = statement('noise', a, lo, hi, seeds)
        if shape == NOISE and seeds == 'range':                   # the reference alone passes these: an input that cannot tell a wrong pass is no test
            assert len(np.unique(d2[d2 != NONE])) >= 16, "degenerate input: %d distinct distances" % len(np.unique(d2))
            assert 2 * int((d2 < row_distances(a, lo, hi)).sum()) > d2.size, "degenerate input: the row pass decides the result"
        check(gpu_ctx, a, lo, hi, seeds, 'noise', d2)


# ---- blobs: a structure with depth -------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", BLOB_SHAPES)
def test_blobs_equal_the_contract_in_both_modes(gpu_ctx, shape, dtype):
    a, code = blob_texels(dtype, shape, seed=37)
    for seeds in SEEDS:
        d2 = statement('blobs', a, code, code, seeds)
        if seeds == 'rest':
            assert len(np.unique(d2[d2 != NONE])) >= 16, "degenerate input: %d distinct depths" % len(np.unique(d2))
        check(gpu_ctx, a, code, code, seeds, 'blobs', d2, steps=64)
        if dtype == np.uint8:
            g = vpt_amd.channel_texels(a, d2, 64)[..., 1]
            assert (g == 255).any() and ((g > 0) & (g < 255)).any(), "degenerate input: the channel does not saturate, or only saturates"


# ---- constructed cases -------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES)
def test_no_seed_every_seed_and_single_seeds(gpu_ctx, dtype):
    nx, ny, nz = NOISE
    M = int(np.iinfo(dtype).max)
    flat = np.full((nz, ny, nx), 9, dtype)
    for seeds, lo, hi in (('range', 10, M), ('rest', 9, 9)):
        d2 = check(gpu_ctx, flat, lo, hi, seeds, 'no seed')
        assert (d2 == NONE).all()
    for seeds, lo, hi in (('range', 9, 9), ('rest', 10, M)):
        d2 = check(gpu_ctx, flat, lo, hi, seeds, 'every voxel a seed')
        assert not d2.any()
    for cz in (0, nz - 1):
        for cy in (0, ny - 1):
            for cx in (0, nx - 1):
                a = np.zeros((nz, ny, nx), dtype)
                a[cz, cy, cx] = M
                d2 = check(gpu_ctx, a, M, M, 'range', 'one seed in the corner (%d, %d, %d)' % (cx, cy, cz))
                assert int(d2.max()) == (nx - 1) ** 2 + (ny - 1) ** 2 + (nz - 1) ** 2
                inverse = (M - a).astype(dtype)                  # the same seed as the only voxel out of range
                check(gpu_ctx, inverse, M, M, 'rest', 'one hole in the corner', d2)


@pytest.mark.timeout(120)
def test_a_carry_crosses_a_whole_segment(gpu_ctx):
    nx, ny, nz = 129, 2, 3
    a = np.zeros((nz, ny, nx), np.uint8)
    a[0, 0, 5] = a[0, 0, 60] = 7                                   # seeds in the first segment only; the query in the third is voxel 128
    a[1, 1, 63] = 7                                               # the last voxel of the first segment
    a[2, 0, 0] = 7
    for texels in (a, np.ascontiguousarray(a[:, :, ::-1])):      # ... and the mirror image: seeds in the last segment only
        d2 = check(gpu_ctx, texels, 7, 7, 'range', 'seeds in one segment')
        row = vpt_amd.distance_squared_texels(texels[0, 0].reshape(1, 1, nx), 7, 7)[0, 0]
        assert int(row.max()) == 68 * 68 and int(d2.max()) > 64 * 64 // 2
        check(gpu_ctx, texels, 0, 6, 'rest', 'seeds in one segment', d2)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("axis", ('x', 'y', 'z'))
def test_the_longest_line_and_the_exact_square_root(gpu_ctx, axis):
    n = 4096
    a = np.zeros((1, 2, n), np.uint16)                            # 4096 x 2 x 1, the only seed at (0, 0, 0)
    a[0, 0, 0] = 0x8000
    offsets = np.arange(n, dtype=np.uint32)
    d2 = np.stack([offsets * offsets, offsets * offsets + 1]).reshape(1, 2, n)      # what the statement gives (tests/test_distance_host.py: transposes commute)
    if axis == 'x':
        assert np.array_equal(statement('line', a, 0x8000, 0x8000, 'range'), d2)
    else:                                                         # the same volume turned: the long axis is y (4096 lines of ... one lane) or z
        turn = (0, 2, 1) if axis == 'y' else (2, 0, 1)
        a, d2 = np.ascontiguousarray(a.transpose(turn)), np.ascontiguousarray(d2.transpose(turn))
    src = upload(gpu_ctx, a)
    found = src.distance(0x8000, 0x8000)
    differences(found.squared(), d2, 'squared, the long axis is ' + axis)
    assert found.info == {'seeds': 1, 'largest': 4095 * 4095 + 1}
    for steps in (1, 7, 256):                                     # squares and non-squares up to 256^2 * (4095^2 + 1)
        pair = found.channel(steps)
        want = vpt_amd.channel_texels(a, d2, steps)
        assert (want[..., 1] == 65535).any() == (steps == 256) and len(np.unique(want[..., 1])) >= 256
        differences(whole(pair), want, 'channel(%d), the long axis is %s' % (steps, axis))
        pair.destroy()
    found.destroy(); src.destroy()


# ---- selections --------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("dtype", DTYPES)
def test_selections_margin_and_core(gpu_ctx, dtype):
    M = int(np.iinfo(dtype).max)
    a, code = blob_texels(dtype, BLOB_SHAPES[0], seed=37)
    src = upload(gpu_ctx, a)
    for seeds in SEEDS:
        d2 = statement('blobs', a, code, code, seeds)
        largest = int(d2.max())
        found = src.distance(code, code, seeds)
        for r2_lo, r2_hi, fill in ((largest + 1, largest + 5, 4), (0, None, 9), (0, NONE - 1, 9), (2, 9, M), (NONE, NONE, 1), (0, 0, 0), (5, 5, 0)):
            out = found.within(r2_lo, r2_hi, fill)
            want = vpt_amd.within_texels(a, d2, r2_lo, r2_hi, fill)
            differences(whole(out), want, "within(%r, %r, %r), %s" % (r2_lo, r2_hi, fill, seeds))
            out.destroy()
        assert (vpt_amd.within_texels(a, d2, largest + 1, largest + 5, 4) == 4).all() and np.array_equal(vpt_amd.within_texels(a, d2, 0, None, 9), a)
        sub = found.squared(3, 2, 1, 11, 7, 5)
        differences(sub, np.ascontiguousarray(d2[1:6, 2:9, 3:14]), 'a box of squared distances')
        found.destroy()
    for radius in (0, 1, 1.5, 2.9, 4, 1e6):                      # the last one: everything with a seed in reach; only what has no way out
        grown, peeled = src.margin(code, code, radius), src.core(code, code, radius)
        r2 = check_radius(radius)
        differences(whole(grown), vpt_amd.within_texels(a, statement('blobs', a, code, code, 'range'), 0, r2), 'margin(%r)' % radius)
        differences(whole(peeled), vpt_amd.within_texels(a, statement('blobs', a, code, code, 'rest'), r2 + 1, None), 'core(%r)' % radius)
        grown.destroy(); peeled.destroy()
    assert vpt_amd.within_texels(a, statement('blobs', a, code, code, 'rest'), 17, None).any(), "degenerate input: core(4) is empty"
    src.destroy()
    # NONE only: a volume without a seed
    flat = upload(gpu_ctx, np.full((5, 6, 7), 3, dtype))
    found = flat.distance(4, M)
    everything, nothing = found.within(NONE, NONE, 8), found.within(0, NONE - 1, 8)
    assert (whole(everything) == 3).all() and (whole(nothing) == 8).all() and found.info == {'seeds': 0, 'largest': 0}
    pair = found.channel(1)
    assert (whole(pair)[..., 1] == M).all()
    for thing in (everything, nothing, pair, found, flat):
        thing.destroy()


# ---- the handle --------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_the_handle_and_its_volumes_outlive_the_source_and_runs_repeat(gpu_ctx):
    nx, ny, nz = BLOB_SHAPES[1]
    a, code = blob_texels(np.uint16, BLOB_SHAPES[1], seed=37)
    d2 = statement('blobs', a, code, code, 'rest')
    src = upload(gpu_ctx, a, 'nearest')
    found = src.distance(code, code, 'rest')
    again = src.distance(code, code, 'rest')
    src.destroy()                                                 # before anything is read or derived
    kept, pair = found.within(2, None, 77), found.channel(16)
    assert found.squared().tobytes() == again.squared().tobytes() == d2.tobytes() and found.info == again.info
    assert set(found.profile()) == {'x', 'y', 'z'} and all(ms >= 0 for ms in found.profile().values())
    found.destroy(); again.destroy()                              # the derived volumes own their texels
    found.destroy()                                               # a second destroy does nothing
    with pytest.raises(RuntimeError, match='destroyed'):
        found.squared()
    assert kept.ready and kept.native_format()[0] == N.FORMAT_R16 and pair.native_format()[0] == N.FORMAT_RG16
    assert kept.modality['dimensions'] == pair.modality['dimensions'] == {'width': nx, 'height': ny, 'depth': nz}
    differences(whole(kept), vpt_amd.within_texels(a, d2, 2, None, 77), 'within')
    differences(whole(pair), vpt_amd.channel_texels(a, d2, 16), 'channel')
    grown = kept.margin(code, code, 2)                            # an ordinary volume: this entry again
    k = vpt_amd.within_texels(a, d2, 2, None, 77)
    differences(whole(grown), vpt_amd.within_texels(k, vpt_amd.distance_squared_texels(k, code, code), 0, 4), 'margin of the core')
    for vol in (grown, kept, pair):
        vol.destroy()


@pytest.mark.timeout(300)
def test_a_channel_volume_renders_like_the_uploaded_texels(gpu_ctx):
    a, code = blob_texels(np.uint8, BLOB_SHAPES[0], seed=37)
    d2 = statement('blobs', a, code, code, 'range')
    tf = colour_tf(64, 48)
    src = upload(gpu_ctx, a)
    found = src.distance(code, code)
    derived = found.channel(8)
    twin = upload(gpu_ctx, vpt_amd.channel_texels(a, d2, 8))
    plain = upload(gpu_ctx, np.stack([a, np.zeros_like(a)], axis=-1))
    fa = render(gpu_ctx, derived, 'mcm', tf=tf)
    same(fa, render(gpu_ctx, twin, 'mcm', tf=tf), 'channel volume')
    pixels = np.ascontiguousarray(fa[-1]); pixels = pixels.reshape(-1, pixels.shape[-1])
    assert len(np.unique(pixels.view(np.uint16), axis=0)) >= 2, 'empty frame'
    assert fa[-1].tobytes() != render(gpu_ctx, plain, 'mcm', tf=tf)[-1].tobytes(), 'the second channel changes nothing'
    for thing in (derived, twin, plain, found, src):
        thing.destroy()


@pytest.mark.timeout(300)
def test_rendering_context_modes_equal_the_chain_by_hand():
    nx, ny, nz = BLOB_SHAPES[0]
    a, code = blob_texels(np.uint8, BLOB_SHAPES[0], seed=37)
    raw = RAWReader(a.tobytes(), {'width': nx, 'height': ny, 'depth': nz, 'bits': 8})
    # 'within': behind components 'keep', in front of the smoothing
    rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'smooth': 1, 'components': {'lo': code, 'hi': code, 'mode': 'keep', 'keep': 2},
                                   'distance': {'lo': code, 'hi': 255, 'seeds': 'rest', 'mode': 'within', 'from': 5, 'fill': 1}})
    try:
        rc.setVolume(raw)
        tex = whole(rc.volume)
    finally:
        rc.destroy()
    ranks, listed = vpt_amd.components_texels(a, code, code, 6)
    assert len(listed) >= 2
    kept = vpt_amd.keep_texels(a, ranks, 1, 2)
    peeled = vpt_amd.within_texels(kept, vpt_amd.distance_squared_texels(kept, code, 255, 'rest'), 5, None, 1)
    assert (peeled == code).any() and ((peeled == 1) & (kept == code)).any(), "the selection changes nothing"
    assert tex.tobytes() == vpt_amd.smooth_texels(peeled, 1).tobytes()
    # 'channel': where the gradient runs, on the final scalar volume
    rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'smooth': 1, 'distance': {'lo': 100, 'hi': 65535, 'mode': 'channel', 'steps': 16}})
    try:
        rc.setVolume(raw)
        assert rc.volume.native_format()[0] == N.FORMAT_RG8
        tex = whole(rc.volume)
    finally:
        rc.destroy()
    value = vpt_amd.smooth_texels(a, 1)
    d2 = vpt_amd.distance_squared_texels(value, 100, 255)
    assert len(np.unique(d2)) >= 16
    assert tex.tobytes() == vpt_amd.channel_texels(value, d2, 16).tobytes()
    # a volume that is not R8 / R16 is left as it is
    f = np.random.default_rng(89).standard_normal((nz, ny, nx)).astype(np.float32)
    rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'distance': {'lo': 0, 'hi': 1, 'mode': 'channel'}})
    try:
        rc.setVolume(RAWReader(f.astype('<f4').tobytes(), {'width': nx, 'height': ny, 'depth': nz, 'bits': 32, 'signed': False}))
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
        with pytest.raises(vpt_amd.VptError, match=r"\b%s\b" % name) as e:
            vol.distance(0, 1)
        assert e.value.code == N.ERR_UNSUPPORTED and "the window makes one of any scalar volume" in str(e.value)
        vol.destroy()
    out = C.c_void_p()
    for dtype, M in ((np.uint8, 255), (np.uint16, 65535)):
        vol = upload(gpu_ctx, np.zeros((4, 4, 4), dtype))
        for lo, hi, seeds in ((5, 4, 0), (0, M + 1, 0), (0, 1, 2), (0, 1, -1)):
            assert L.vpt_volume_distance(vol.texture, lo, hi, seeds, C.byref(out)) == N.ERR_INVALID, (lo, hi, seeds)
        for lo, hi, seeds in ((5, 4, 'range'), (0, M + 1, 'range'), (0, 1, 'both'), (0, 1, 0)):
            with pytest.raises(ValueError):
                vol.distance(lo, hi, seeds)
        assert L.vpt_volume_distance(vol.texture, 0, 1, 0, None) == N.ERR_INVALID
        found = vol.distance(0, 0)                                # every voxel a seed
        assert found.info == {'seeds': 64, 'largest': 0}
        h = found._h
        for r2_lo, r2_hi, fill in ((2, 1, 0), (0, 1, M + 1)):
            assert L.vpt_distance_within(h, r2_lo, r2_hi, fill, C.byref(out)) == N.ERR_INVALID, (r2_lo, r2_hi, fill)
            with pytest.raises(ValueError):
                found.within(r2_lo, r2_hi, fill)
        for steps in (0, 257, -1):
            assert L.vpt_distance_channel(h, steps, C.byref(out)) == N.ERR_INVALID, steps
            with pytest.raises(ValueError):
                found.channel(steps)
        assert L.vpt_distance_within(h, 0, 1, 0, None) == N.ERR_INVALID and L.vpt_distance_channel(h, 1, None) == N.ERR_INVALID
        d2 = np.zeros(64, np.uint32)
        p = d2.ctypes.data_as(C.c_void_p)
        assert L.vpt_distance_squared(h, 0, 0, 0, 4, 4, 4, p, d2.nbytes - 1) == N.ERR_INVALID and b"too short" in L.vpt_last_error()
        assert L.vpt_distance_squared(h, 1, 0, 0, 4, 4, 4, p, d2.nbytes) == N.ERR_INVALID and b"outside" in L.vpt_last_error()
        assert L.vpt_distance_squared(h, 0, 0, 0, 4, 4, 0, p, d2.nbytes) == N.ERR_INVALID
        assert L.vpt_distance_squared(h, 0, 0, 0, 4, 4, 4, None, d2.nbytes) == N.ERR_INVALID
        assert L.vpt_distance_info(h, None) == N.ERR_INVALID and L.vpt_distance_profile(h, None) == N.ERR_INVALID
        for radius in (-1, float('nan'), float('inf')):
            with pytest.raises(ValueError):
                vol.margin(0, 0, radius)
            with pytest.raises(ValueError):
                vol.core(0, 0, radius)
        found.destroy(); vol.destroy()
    for options in ({'distance': 'within'}, {'distance': {'lo': 0, 'hi': 1}}, {'distance': {'lo': 2, 'hi': 1, 'mode': 'within'}},
                    {'distance': {'lo': 0, 'hi': 1, 'mode': 'margin'}}, {'distance': {'lo': 0, 'hi': 1, 'mode': 'within', 'seeds': 'both'}},
                    {'distance': {'lo': 0, 'hi': 1, 'mode': 'within', 'steps': 2}}, {'distance': {'lo': 0, 'hi': 1, 'mode': 'channel', 'steps': 0}},
                    {'distance': {'lo': 0, 'hi': 1, 'mode': 'channel'}, 'gradient': 'central'},
                    {'distance': {'lo': 0, 'hi': 1, 'mode': 'channel'}, 'components': {'lo': 0, 'hi': 1, 'mode': 'label'}}):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext(options)
