"""GPU: the connected components of a value range of a volume, labelled on the device (vpt_volume_components and the vpt_components_*
family).

The per-voxel ranks, the component list, the info and the texels of the `keep` and `label` volumes are held, byte for byte, to
vpt_amd.components_texels / keep_texels / label_texels, the numpy statement of the contract (tests/test_components_host.py holds that to a
breadth-first search in Python integers and to scipy).  Parity chain to the oracle: volumes uploaded from the host are held to the CPU
oracle by the rest of the suite, so a `label` volume must give byte-identical buffers to the volume uploaded from the numpy statement's
texels.

The labelling tile is 64 x 8 x 4 (CC_TX, CC_TY, CC_TZ in vpt_volume_components.hip); every other kernel is a grid-stride loop over the
linear index.  So the shapes that matter are one voxel past the tile on every axis (two tiles an axis, every face, edge and corner junction
once) and one voxel past two tiles (a tile with neighbours on both sides, a junction of eight whole tiles)."""
import ctypes as C

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.loaders import BlobLoader
from vpt_amd.readers import BVPReader, RAWReader
from vpt_amd.synthetic import colour_tf

from test_gpu_readers import make_bvp_typed
from test_gpu_volume_formats import render, same, PACKED
from test_gpu_pyramid import upload, whole

pytestmark = pytest.mark.gpu

TILE = (64, 8, 4)                                                   # nx, ny, nz of a labelling tile
TX, TY, TZ = TILE
NOISE = (23, 19, 21)                                                # nx, ny, nz: every axis odd
PLUS_ONE = (TX + 1, TY + 1, TZ + 1)                                 # nx % 4 != 0
PLUS_ONE_4 = (TX + 4, TY + 1, TZ + 1)                               # the same, nx % 4 == 0
TWO_TILES = (2 * TX + 1, 2 * TY + 1, 2 * TZ + 1)
SHAPES = (NOISE, (1, 1, 1), (7, 5, 1), (17, 1, 3), (1, 3, 17), PLUS_ONE, PLUS_ONE_4, TWO_TILES)
DTYPES = (np.uint8, np.uint16)
CONNECTIVITIES = (6, 18, 26)
# the foreground fraction of the noise: below the percolation density of the connectivity, or one giant component hides merge errors
FRACTION = {6: 0.30, 18: 0.13, 26: 0.09}


def noise(dtype, shape, seed):
    nx, ny, nz = shape
    M = int(np.iinfo(dtype).max)
    return np.random.default_rng(seed).integers(0, M + 1, size=(nz, ny, nx)).astype(dtype)


def noise_range(dtype, connectivity):
    """(lo, hi): FRACTION of all codes; for uint16 a range whose ends lie inside a byte and that straddles 0x7FFF / 0x8000"""
    if dtype == np.uint8:
        return 0, int(round(FRACTION[connectivity] * 256)) - 1
    width = int(round(FRACTION[connectivity] * 65536))
    lo = 0x8000 - width // 3
    return lo, lo + width - 1


def differences(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d values differ (%s), first at %s: %d, expected %d" % (len(bad), what, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def statement(a, lo, hi, connectivity, min_voxels=1):
    """(ranks, list, the number of components of any size) of the numpy statement"""
    ranks, listed = vpt_amd.components_texels(a, lo, hi, connectivity, min_voxels)
    return ranks, listed, len(listed if min_voxels == 1 else vpt_amd.components_texels(a, lo, hi, connectivity)[1])


def check(ctx, a, lo, hi, connectivity, min_voxels=1, what='', caps=None, want=None):
    """labels `a` on the device and holds everything the handle gives to the numpy statement; returns (ranks, list) of the statement.
    caps: (merge_steps, flatten_steps) of vpt_volume_components_capped; want: statement(a, lo, hi, connectivity, min_voxels), where several
    calls share it"""
    what = "%s %s %s [%d, %d] c%d m%d%s" % (what, a.dtype.name, a.shape[::-1], lo, hi, connectivity, min_voxels, '' if caps is None else ' caps %r' % (caps,))
    ranks, listed, everything = statement(a, lo, hi, connectivity, min_voxels) if want is None else want
    src = upload(ctx, a)
    found = src.components(lo, hi, connectivity, min_voxels, _caps=caps)
    differences(found.ranks(), ranks, what + ': ranks')
    assert found.list() == listed, what + ': list'
    assert found.info == {'listed': len(listed), 'dropped': everything - len(listed), 'foreground_voxels': int(((a >= lo) & (a <= hi)).sum()),
                          'listed_voxels': sum(c[3] for c in listed)}, what + ': info'
    kept, pair = found.keep(), found.label()
    differences(whole(kept), vpt_amd.keep_texels(a, ranks), what + ': keep')
    differences(whole(pair), vpt_amd.label_texels(a, ranks), what + ': label')
    assert whole(src).tobytes() == a.tobytes(), what + ": the source's texels changed"
    for thing in (kept, pair, found, src):
        thing.destroy()
    return ranks, listed


# ---- noise -------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_noise_equals_the_contract(gpu_ctx, connectivity, dtype):
    lo, hi = noise_range(dtype, connectivity)
    M = int(np.iinfo(dtype).max)
    for n, shape in enumerate(SHAPES):
        a = noise(dtype, shape, seed=61 + n)
        ranks, listed = check(gpu_ctx, a, lo, hi, connectivity, what='noise')
        if a.size >= NOISE[0] * NOISE[1] * NOISE[2]:              # an input whose components are few, or one, cannot tell a wrong merge
            sizes = [c[3] for c in listed]
            assert len(listed) >= 64, "degenerate input: %d components" % len(listed)
            assert len(set(sizes[:255])) < len(sizes[:255]), "degenerate input: no size tie"
            assert 2 * sizes[0] < sum(sizes), "degenerate input: one component holds half of the foreground"
            if dtype == np.uint8 and connectivity == 6:
                assert len(listed) > 255 and int(ranks.max()) > M, "degenerate input: G does not saturate"


@pytest.mark.timeout(300)
@pytest.mark.parametrize("dtype", DTYPES)
def test_min_voxels_selections_and_fill(gpu_ctx, dtype):
    a = noise(dtype, NOISE, seed=71)
    lo, hi = noise_range(dtype, 6)
    M = int(np.iinfo(dtype).max)
    _, listed = check(gpu_ctx, a, lo, hi, 6, 2, 'min 2')
    assert listed and listed[-1][3] >= 2
    ranks, none = check(gpu_ctx, a, lo, hi, 6, listed[0][3] + 1, 'min largest + 1')
    assert none == [] and not ranks.any()
    ranks, listed = vpt_amd.components_texels(a, lo, hi, 6)
    src = upload(gpu_ctx, a)
    found = src.components(lo, hi, 6)
    for first, last, fill in ((2, 3, 0), (1, 1, M), (3, None, 7), (len(listed), len(listed) + 5, 1), (len(listed) + 1, 1 << 40, 9), (1 << 33, None, 2)):
        out = found.keep(first, last, fill)
        want = vpt_amd.keep_texels(a, ranks, first, last, fill)
        differences(whole(out), want, "keep(%r, %r, %r)" % (first, last, fill))
        out.destroy()
    assert found.list(1, 2) == listed[1:3] and found.list(len(listed), 0) == []
    sub = found.ranks(3, 2, 1, 11, 7, 5)
    differences(sub, np.ascontiguousarray(ranks[1:6, 2:9, 3:14]), 'a box of ranks')
    # an empty selection of everything is all fill
    empty = src.components(lo, hi, 6, listed[0][3] + 1)
    out = empty.keep(1, None, 5)
    assert (whole(out) == 5).all()
    for thing in (out, empty, found, src):
        thing.destroy()


# ---- constructed cases -------------------------------------------------------------------------------------------------------
def serpentine(shape, along):
    """[nz][ny][nx] uint8, 200 on a one-voxel-wide path and 0 elsewhere: lines along axis `along` ('x' or 'z') on every second row and every
    second layer, joined at alternating ends, so the path runs the whole volume and crosses a tile face at every tile it meets"""
    nx, ny, nz = shape
    n0, n1, n2 = (nz, ny, nx) if along == 'x' else (nx, ny, nz)
    s = np.zeros((n0, n1, n2), np.uint8)
    end = 0
    for i0 in range(0, n0, 2):
        rows = list(range(0, n1, 2))
        if (i0 // 2) % 2:
            rows.reverse()
        for k, i1 in enumerate(rows):
            s[i0, i1, :] = 200
            end = n2 - 1 - end                                     # the line ends where the next one begins
            if k + 1 < len(rows):
                s[i0, (i1 + rows[k + 1]) // 2, end] = 200
        if i0 + 1 < n0:
            s[i0 + 1, rows[-1], end] = 200
    return np.ascontiguousarray(s if along == 'x' else s.transpose(2, 1, 0))


def box(shape, x, y, z):
    """uint8 [nz][ny][nx]: 200 in the box x[0] .. x[1] - 1 etc. (clipped to the volume), 0 elsewhere"""
    nx, ny, nz = shape
    a = np.zeros((nz, ny, nx), np.uint8)
    a[max(z[0], 0):z[1], max(y[0], 0):y[1], max(x[0], 0):x[1]] = 200
    return a


@pytest.mark.timeout(300)
@pytest.mark.parametrize("shape", (PLUS_ONE, PLUS_ONE_4, TWO_TILES))
def test_constructed_cases(gpu_ctx, shape):
    nx, ny, nz = shape
    # a serpentine is one component under every connectivity: the worst case of the merge
    for along in ('x', 'z'):
        s = serpentine(shape, along)
        for connectivity in CONNECTIVITIES:
            _, listed = check(gpu_ctx, s, 200, 200, connectivity, what='serpentine along ' + along)
            assert len(listed) == 1 and listed[0] == (0, 0, 0, int((s == 200).sum())), (along, connectivity, listed[:3])
    s16 = serpentine(shape, 'z').astype(np.uint16) * 257
    _, listed = check(gpu_ctx, s16, 0x8000, 0xFFFF, 6, what='serpentine, 16 bits')
    assert len(listed) == 1
    # a checkerboard: singletons through faces, one component through edges
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing='ij')
    board = np.where((x + y + z) % 2 == 0, 200, 0).astype(np.uint8)
    _, listed = check(gpu_ctx, board, 200, 255, 6, what='checkerboard')
    assert len(listed) == (nx * ny * nz + 1) // 2 and listed[0][3] == 1 and listed[:2] == [(0, 0, 0, 1), (2, 0, 0, 1)]
    for connectivity in (18, 26):
        _, listed = check(gpu_ctx, board, 200, 255, connectivity, what='checkerboard')
        assert len(listed) == 1
    # two blocks that touch only across a tile edge (each of the three directions an edge can run in), and only across the corner where
    # eight tiles meet
    lo_x, lo_y, lo_z = (TX - 2, TX), (TY - 2, TY), (TZ - 2, TZ)
    hi_x, hi_y, hi_z = (TX, TX + 2), (TY, TY + 2), (TZ, TZ + 2)
    edges = {'along z': box(shape, lo_x, lo_y, lo_z) | box(shape, hi_x, hi_y, lo_z),
             'along y': box(shape, lo_x, lo_y, lo_z) | box(shape, hi_x, lo_y, hi_z),
             'along x': box(shape, lo_x, lo_y, lo_z) | box(shape, lo_x, hi_y, hi_z),
             'along z, the other diagonal': box(shape, hi_x, lo_y, lo_z) | box(shape, lo_x, hi_y, lo_z)}
    for name, a in edges.items():
        for connectivity, count in ((6, 2), (18, 1), (26, 1)):
            _, listed = check(gpu_ctx, a, 1, 255, connectivity, what='edge ' + name)
            assert len(listed) == count, (name, connectivity, listed)
    corners = {'main diagonal': box(shape, lo_x, lo_y, lo_z) | box(shape, hi_x, hi_y, hi_z),
               'another diagonal': box(shape, hi_x, lo_y, lo_z) | box(shape, lo_x, hi_y, hi_z)}
    for name, a in corners.items():
        for connectivity, count in ((6, 2), (18, 2), (26, 1)):
            _, listed = check(gpu_ctx, a, 1, 255, connectivity, what='corner ' + name)
            assert len(listed) == count, (name, connectivity, listed)
    # everything and nothing
    _, listed = check(gpu_ctx, np.full((nz, ny, nx), 9, np.uint8), 9, 9, 6, what='all foreground')
    assert listed == [(0, 0, 0, nx * ny * nz)]
    _, listed = check(gpu_ctx, np.full((nz, ny, nx), 9, np.uint8), 10, 255, 26, what='all background')
    assert listed == []
    # most voxels in the first tile, the root (the smallest linear index) in the last tile along x
    a = box(shape, (0, 41), (2, 7), (0, 4))
    a[0, 2, 40:] = 200
    a[0, 0:3, nx - 1] = 200
    a[nz - 1, ny - 1, 0] = 200                                      # ... and a second component
    for connectivity in CONNECTIVITIES:
        _, listed = check(gpu_ctx, a, 200, 200, connectivity, what='root in the last tile')
        assert len(listed) == 2 and listed[0][:3] == (nx - 1, 0, 0) and listed[1] == (0, ny - 1, nz - 1, 1)


# ---- the handle --------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_the_handle_and_its_volumes_outlive_the_source_and_runs_repeat(gpu_ctx):
    nx, ny, nz = TWO_TILES
    a = noise(np.uint16, TWO_TILES, seed=73)
    lo, hi = noise_range(np.uint16, 6)
    ranks, listed = vpt_amd.components_texels(a, lo, hi, 6, 3)
    src = upload(gpu_ctx, a, 'nearest')
    found = src.components(lo, hi, 6, 3)
    again = src.components(lo, hi, 6, 3)
    src.destroy()                                                 # before anything is read or derived
    kept, pair = found.keep(1, 4, 77), found.label()
    assert found.ranks().tobytes() == again.ranks().tobytes() == ranks.tobytes() and found.list() == again.list() == listed
    found.destroy(); again.destroy()                              # the derived volumes own their texels
    found.destroy()                                               # a second destroy does nothing
    with pytest.raises(RuntimeError, match='destroyed'):
        found.ranks()
    assert kept.ready and kept.native_format()[0] == N.FORMAT_R16 and pair.native_format()[0] == N.FORMAT_RG16
    assert kept.modality['dimensions'] == pair.modality['dimensions'] == {'width': nx, 'height': ny, 'depth': nz}
    differences(whole(kept), vpt_amd.keep_texels(a, ranks, 1, 4, 77), 'keep')
    differences(whole(pair), vpt_amd.label_texels(a, ranks), 'label')
    smaller = kept.remove_islands(lo, hi, 5)                      # an ordinary volume: this entry again
    k_ranks = vpt_amd.components_texels(vpt_amd.keep_texels(a, ranks, 1, 4, 77), lo, hi, 6, 5)[0]
    differences(whole(smaller), vpt_amd.keep_texels(vpt_amd.keep_texels(a, ranks, 1, 4, 77), k_ranks), 'remove_islands')
    for vol in (smaller, kept, pair):
        vol.destroy()
    src = upload(gpu_ctx, a)
    largest = src.keep_largest(lo, hi, 2, 18)
    r18 = vpt_amd.components_texels(a, lo, hi, 18)[0]
    differences(whole(largest), vpt_amd.keep_texels(a, r18, 1, 2), 'keep_largest')
    largest.destroy(); src.destroy()


@pytest.mark.timeout(300)
def test_a_label_volume_renders_like_the_uploaded_texels(gpu_ctx):
    a = noise(np.uint8, NOISE, seed=79)
    ranks, listed = vpt_amd.components_texels(a, 0, 76, 6)
    assert len(listed) > 255
    tf = colour_tf(64, 48)
    src = upload(gpu_ctx, a)
    found = src.components(0, 76, 6)
    derived = found.label()
    twin = upload(gpu_ctx, vpt_amd.label_texels(a, ranks))
    plain = upload(gpu_ctx, np.stack([a, np.zeros_like(a)], axis=-1))
    fa = render(gpu_ctx, derived, 'mcm', tf=tf)
    same(fa, render(gpu_ctx, twin, 'mcm', tf=tf), 'label volume')
    pixels = np.ascontiguousarray(fa[-1]); pixels = pixels.reshape(-1, pixels.shape[-1])
    assert len(np.unique(pixels.view(np.uint16), axis=0)) >= 2, 'empty frame'
    assert fa[-1].tobytes() != render(gpu_ctx, plain, 'mcm', tf=tf)[-1].tobytes(), 'the second channel changes nothing'
    for thing in (derived, twin, plain, found, src):
        thing.destroy()


@pytest.mark.timeout(300)
def test_rendering_context_modes_equal_the_chain_by_hand():
    nx, ny, nz = NOISE
    a = noise(np.uint8, NOISE, seed=83)
    raw = RAWReader(a.tobytes(), {'width': nx, 'height': ny, 'depth': nz, 'bits': 8})
    spec = {'lo': 0, 'hi': 76, 'connectivity': 6, 'minVoxels': 2}
    # 'keep': behind the rank filter, in front of the smoothing
    rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'rank': 'median', 'smooth': 1, 'gradient': 'central',
                                   'components': dict(spec, mode='keep', keep=3)})
    try:
        rc.setVolume(raw)
        tex = whole(rc.volume)
    finally:
        rc.destroy()
    m = vpt_amd.rank_texels(a, 'median')
    ranks, listed = vpt_amd.components_texels(m, 0, 76, 6, 2)
    assert len(listed) > 3
    value = vpt_amd.smooth_texels(vpt_amd.keep_texels(m, ranks, 1, 3), 1)
    assert tex[..., 0].tobytes() == value.tobytes() and tex[..., 1].tobytes() == vpt_amd.gradient_magnitude(value, 'central', 1).tobytes()
    assert value.tobytes() != vpt_amd.smooth_texels(m, 1).tobytes(), "the selection changes nothing"
    # 'keep' without a number: island removal
    rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'components': dict(spec, mode='keep')})
    try:
        rc.setVolume(raw)
        tex = whole(rc.volume)
    finally:
        rc.destroy()
    ranks, _ = vpt_amd.components_texels(a, 0, 76, 6, 2)
    assert tex.tobytes() == vpt_amd.keep_texels(a, ranks).tobytes()
    # 'label': where the gradient runs, on the final scalar volume
    rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'smooth': 1, 'components': dict(spec, lo=100, hi=115, mode='label')})
    try:
        rc.setVolume(raw)
        assert rc.volume.native_format()[0] == N.FORMAT_RG8
        tex = whole(rc.volume)
    finally:
        rc.destroy()
    value = vpt_amd.smooth_texels(a, 1)
    ranks, listed = vpt_amd.components_texels(value, 100, 115, 6, 2)
    assert len(listed) >= 64
    assert tex.tobytes() == vpt_amd.label_texels(value, ranks).tobytes()
    with pytest.raises(ValueError):
        vpt_amd.RenderingContext({'gradient': 'sobel', 'components': dict(spec, mode='label')})
    # a volume that is not R8 / R16 is left as it is
    f = np.random.default_rng(89).standard_normal((nz, ny, nx)).astype(np.float32)
    rc = vpt_amd.RenderingContext({'resolution': (72, 56), 'components': dict(spec, mode='label')})
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
            vol.components(0, 1)
        assert e.value.code == N.ERR_UNSUPPORTED and "the window makes one of any scalar volume" in str(e.value)
        vol.destroy()
    out = C.c_void_p()
    for dtype, M in ((np.uint8, 255), (np.uint16, 65535)):
        vol = upload(gpu_ctx, np.zeros((4, 4, 4), dtype))
        for lo, hi, connectivity, min_voxels in ((5, 4, 6, 1), (0, M + 1, 6, 1), (0, 1, 4, 1), (0, 1, 0, 1), (0, 1, 27, 1), (0, 1, 6, 0)):
            assert L.vpt_volume_components(vol.texture, lo, hi, connectivity, min_voxels, C.byref(out)) == N.ERR_INVALID, (lo, hi, connectivity, min_voxels)
            with pytest.raises(ValueError):
                vol.components(lo, hi, connectivity, min_voxels)
        assert L.vpt_volume_components(vol.texture, 0, 1, 6, 1, None) == N.ERR_INVALID
        found = vol.components(0, 0)                              # one component of 64 voxels
        assert found.list() == [(0, 0, 0, 64)]
        h = found._h
        buf = (N.Component * 4)()
        for first, n in ((0, 2), (1, 1), (2, 0), (1 << 63, 1 << 63)):
            assert L.vpt_components_list(h, first, n, buf) == N.ERR_INVALID, (first, n)
        assert L.vpt_components_list(h, 1, 0, buf) == N.OK and L.vpt_components_list(h, 0, 1, None) == N.ERR_INVALID
        for first, last, fill in ((0, 1, 0), (2, 1, 0), (1, 1, M + 1)):
            assert L.vpt_components_keep(h, first, last, fill, C.byref(out)) == N.ERR_INVALID, (first, last, fill)
            with pytest.raises(ValueError):
                found.keep(first, last, fill)
        assert L.vpt_components_keep(h, 1, 1, 0, None) == N.ERR_INVALID and L.vpt_components_label(h, None) == N.ERR_INVALID
        ranks = np.zeros(64, np.uint32)
        p = ranks.ctypes.data_as(C.c_void_p)
        assert L.vpt_components_ranks(h, 0, 0, 0, 4, 4, 4, p, ranks.nbytes - 1) == N.ERR_INVALID and b"too short" in L.vpt_last_error()
        assert L.vpt_components_ranks(h, 1, 0, 0, 4, 4, 4, p, ranks.nbytes) == N.ERR_INVALID and b"outside" in L.vpt_last_error()
        assert L.vpt_components_ranks(h, 0, 0, 0, 4, 4, 0, p, ranks.nbytes) == N.ERR_INVALID
        assert L.vpt_components_ranks(h, 0, 0, 0, 4, 4, 4, None, ranks.nbytes) == N.ERR_INVALID
        assert L.vpt_components_info(h, None) == N.ERR_INVALID
        found.destroy(); vol.destroy()
    for options in ({'components': 'keep'}, {'components': {'lo': 0, 'hi': 1}}, {'components': {'lo': 2, 'hi': 1, 'mode': 'keep'}},
                    {'components': {'lo': 0, 'hi': 1, 'mode': 'drop'}}, {'components': {'lo': 0, 'hi': 1, 'mode': 'keep', 'connectivity': 8}},
                    {'components': {'lo': 0, 'hi': 1, 'mode': 'keep', 'minVoxels': 0}}, {'components': {'lo': 0, 'hi': 1, 'mode': 'keep', 'keep': 0}},
                    {'components': {'lo': 0, 'hi': 1, 'mode': 'label', 'keep': 2}}, {'components': {'lo': 0, 'hi': 1, 'mode': 'label'}, 'gradient': 'central'}):
        with pytest.raises(ValueError):
            vpt_amd.RenderingContext(options)
