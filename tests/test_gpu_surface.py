"""GPU: the isosurface mesh by naive surface nets (vpt_volume_surface) on the device.

Vertices, quads and every info field are held, byte for byte, to vpt_amd.surface.surface_texels, the numpy statement of the contract
(tests/test_surface_host.py holds that to what the contract promises).  No tolerance appears anywhere.

A word of the inside plane holds 32 grid points along x of a row padded to W + 2, a word of cells 32 of a row of W + 1; a workgroup of the
vertex kernel owns 256 words, of the quad kernel 128, a block of the prefix sums 2048 (or what _scan_words says).  The shapes are the
smallest at which that can go wrong: widths round the word edges with voxels in the first and the last column, structures on all six
faces, every cell active over 650 words with 2 and 3 words a scan block, the widest volume the library takes, and the three shapes at which
the grid-stride loops of k_sf_inside, of the scan kernels and of k_sf_classify make a second trip."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import vpt_amd
from vpt_amd import _native as N
from vpt_amd.surface import surface_texels

from test_gpu_pyramid import upload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check(ctx, array, level, channel=0, scan_words=None):
    """the device's surface of `array` equals the statement's; returns (vertices, quads)"""
    want_info = {}
    wv, wq = surface_texels(array, level, channel, info=want_info)
    vol = upload(ctx, array)
    s = vol.surface(level, channel, _scan_words=scan_words)
    vol.destroy()                                                 # the surface owns what it holds
    try:
        info = s.info
        assert info == want_info
        assert sum(info['crossings']) == info['quads']
        codes = array[..., channel] if array.ndim == 4 else array
        assert info['inside'] == int((codes >= level).sum())
        v, q = s.vertices(), s.quads()
        assert v.dtype == np.uint32 and q.dtype == np.uint32 and v.shape == wv.shape and q.shape == wq.shape
        assert np.array_equal(v, wv), 'vertices differ first at %s' % (np.argwhere(v != wv)[:1],)
        assert np.array_equal(q, wq), 'quads differ first at %s' % (np.argwhere(q != wq)[:1],)
    finally:
        s.destroy()
    return wv, wq


def noise(shape, dtype, seed):
    return np.random.default_rng(seed).integers(0, int(np.iinfo(dtype).max) + 1, shape, dtype=dtype)


def test_one_voxel(gpu_ctx):
    v, q = check(gpu_ctx, np.full((1, 1, 1), 200, np.uint8), 128)
    assert len(v) == 8 and len(q) == 6


def test_worked_example(gpu_ctx):
    a = np.zeros((3, 3, 3), np.uint8)
    a[1, 1, 1] = 255
    v, _ = check(gpu_ctx, a, 128)
    assert v[0].tolist() == [120149] * 3 and v[7].tolist() == [141995] * 3


@pytest.mark.parametrize('width', [30, 31, 32, 33, 62, 63, 64, 65])
def test_widths_round_the_word_edges(gpu_ctx, width):
    a = np.zeros((3, 5, width), np.uint8)
    a[:, :, 0] = 255; a[:, :, width - 1] = 255
    a[1, 2, :] = np.arange(width) * 7 % 256
    check(gpu_ctx, a, 100)


def test_structure_on_all_six_faces(gpu_ctx):
    z, y, x = np.indices((9, 10, 35))
    cross = (np.abs(y - 5) <= 1) & (np.abs(z - 4) <= 1) | (np.abs(x - 17) <= 1) & (np.abs(z - 4) <= 1) | (np.abs(x - 17) <= 1) & (np.abs(y - 5) <= 1)
    check(gpu_ctx, np.where(cross, 220, 30).astype(np.uint8), 128)


@pytest.mark.parametrize('level', [1, 128, 255])
def test_r8_noise(gpu_ctx, level):
    check(gpu_ctx, noise((6, 11, 37), np.uint8, 21), level)


@pytest.mark.parametrize('level', [1, 30000, 65535])
def test_r16_noise(gpu_ctx, level):
    a = noise((5, 7, 21), np.uint16, 22)
    a[2, 3, 10] = 65535
    a[0, 0, 0] = 0
    check(gpu_ctx, a, level)


@pytest.mark.parametrize('dtype, level', [(np.uint8, 77), (np.uint16, 40000)])
def test_second_channel(gpu_ctx, dtype, level):
    a = noise((4, 6, 34, 2), dtype, 23)
    check(gpu_ctx, a, level, 1)
    check(gpu_ctx, a, level, 0)


def test_full_volume(gpu_ctx):
    v, q = check(gpu_ctx, np.full((2, 3, 4), 255, np.uint8), 1)
    assert (len(v), len(q)) == (54, 52)


def test_empty_result(gpu_ctx):
    vol = upload(gpu_ctx, np.full((4, 5, 40), 9, np.uint8))
    s = vol.surface(10)
    info = s.info
    assert info['vertices'] == 0 and info['quads'] == 0 and info['inside'] == 0 and info['crossings'] == [0, 0, 0] and info['cells'] == 5 * 6 * 41
    assert s.vertices().shape == (0, 3) and s.quads().shape == (0, 4) and s.triangles().shape == (0, 3)
    p = s.profile
    assert p['inside'] > 0 and p['vertices'] == 0 and p['quads'] == 0
    assert s.device() == (None, None) and s.area() == 0.0
    s.destroy(); vol.destroy()


def checkerboard():
    z, y, x = np.indices((12, 24, 48))
    return np.where((x + y + z) % 2 == 0, 255, 0).astype(np.uint8)


@pytest.mark.parametrize('scan_words', [None, 2, 3])
def test_checkerboard_crosses_both_scan_levels(gpu_ctx, scan_words):
    """every cell of the 49 x 25 x 13 is active but four: a corner cell holds one voxel, and with even sizes four of the eight corner
    voxels of a checkerboard are 0 (15 925 - 4 = 15 921 vertices by the statement)"""
    v, _ = check(gpu_ctx, checkerboard(), 1, scan_words=scan_words)
    assert len(v) == 49 * 25 * 13 - 4 == 15921


def sprinkled(shape, seed, also):
    """uint8 noise below 128 with a seeded 1.5 % of the voxels, the eight corners and the voxels `also` raised to a seeded code of 128 and
    above: a surface at level 128 of many specks"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 128, shape, dtype=np.uint8)
    chosen = rng.random(shape) < 0.015
    for z in (0, shape[0] - 1):
        for y in (0, shape[1] - 1):
            for x in (0, shape[2] - 1):
                chosen[z, y, x] = True
    for at in also:
        chosen[at] = True
    a[chosen] = rng.integers(128, 256, int(chosen.sum()), dtype=np.uint8)
    return a


def cell_words(vertices, H, cwpr=1):
    """the word of the cell masks that holds each vertex's cell: ((k + 1) (H + 1) + j + 1) cwpr + (i + 1) div 32"""
    cell = vertices.astype(np.int64) >> 16
    return (cell[:, 2] * (H + 1) + cell[:, 1]) * cwpr + (cell[:, 0] >> 5)


def test_second_trip_of_the_inside_kernels_loop(gpu_ctx):
    """k_sf_inside: stream_grid(items, 4) launches at most 8 192 workgroups of 4 waves, and a wave takes the items wave, wave + 32 768, ...
    An item is 64 grid points of a padded row: W = 1 gives one word and one item a row, H = D = 180 gives (H + 2) (D + 2) = 182^2 = 33 124
    items, so the waves 0 .. 355 make a second trip.  It begins at item 32 768 = row 180 x 182 + 8: z = 179, y = 7; voxels are set there and
    in the row before it (y = 6), the last of the first trip."""
    H = D = 180
    assert (H + 2) * (D + 2) == 33124 > 8192 * 4 and divmod(8192 * 4, H + 2) == (D, 8)
    a = sprinkled((D, H, 1), 31, [(179, 6, 0), (179, 7, 0)])
    v, _ = check(gpu_ctx, a, 128)
    assert len(v) > 1000 and int(v[:, 2].max()) >> 16 == D and int(v[:, 2].min()) >> 16 == 0


def test_second_trip_of_the_scan_kernels_loops(gpu_ctx):
    """k_sf_block_sums, k_sf_scan_add: stream_grid(blocks, 1, 65 535) launches at most 65 535 workgroups, and one takes the blocks b,
    b + 65 535, ...  With _scan_words = 1 a block is a word; W = 1 gives one word a cell row, H = D = 256 gives (H + 1) (D + 1) = 257^2 =
    66 049 blocks, so the workgroups 0 .. 513 make a second trip, and a thread of k_sf_scan_blocks owns a run of per = ceil(66 049 / 256) =
    259 sums (never more than 2 before).  The second trip begins at word 65 535 = cell row 255 x 257 + 0: cells j = -1, k = 254, which the
    voxel y = 0, z = 254 makes active; word 65 534 is the cells j = 255, k = 253, of the voxel y = 255, z = 253."""
    H = D = 256
    words = (H + 1) * (D + 1)
    assert words == 66049 > 65535 and (words + 255) // 256 == 259 and divmod(65535, H + 1) == (255, 0)
    a = sprinkled((D, H, 1), 32, [(254, 0, 0), (253, 255, 0)])
    v, _ = check(gpu_ctx, a, 128, scan_words=1)
    w = cell_words(v, H)
    assert 65534 in w and 65535 in w and (w < 65534).any() and (w > 65535).any()


def test_second_trip_of_the_classify_kernels_loop(gpu_ctx):
    """k_sf_classify: stream_grid(words) launches at most 8 192 workgroups of 256 threads, and a thread takes the words w, w + 2 097 152,
    ...  W = 2 gives one word a cell row (W + 1 <= 32), H = D = 1448 gives (H + 1) (D + 1) = 1449^2 = 2 099 601 words, so the threads
    0 .. 2 448 make a second trip.  It begins at word 2 097 152 = cell row 1447 x 1449 + 449: cells j = 448, k = 1446, which the voxel
    y = 449, z = 1446 makes active; word 2 097 151 is the cells j = 447, of the voxel y = 447."""
    H = D = 1448
    words = (H + 1) * (D + 1)
    assert words == 2099601 > 8192 * 256 and divmod(8192 * 256, H + 1) == (1447, 449)
    a = sprinkled((D, H, 2), 33, [(1446, 449, 0), (1446, 447, 1)])
    v, _ = check(gpu_ctx, a, 128)
    w = cell_words(v, H)
    assert 2097151 in w and 2097152 in w and (w < 2097151).any() and (w > 2097152).any()


def test_widest_volume(gpu_ctx):
    a = np.zeros((2, 2, 4096), np.uint8)
    a[0, 0, 0] = 255; a[1, 1, 4095] = 200; a[0, 1, 2047:2050] = 99
    v, _ = check(gpu_ctx, a, 50)
    assert v[:, 0].max() > 4095 * 65536


def test_paged_reads_and_refused_windows(gpu_ctx):
    a = noise((5, 6, 33), np.uint8, 24)
    wv, wq = surface_texels(a, 128)
    vol = upload(gpu_ctx, a)
    s = vol.surface(128)
    for read, want, page in ((s.vertices, wv, 97), (s.quads, wq, 211)):
        parts = [read(first, min(page, len(want) - first)) for first in range(0, len(want), page)]
        assert np.array_equal(np.concatenate(parts), want)
        assert read(len(want), 0).shape[0] == 0 and read(len(want)).shape[0] == 0
        with pytest.raises(ValueError, match='not within'):
            read(len(want) + 1)
        with pytest.raises(ValueError, match='not within'):
            read(1, len(want))
    # the C-ABI refuses them itself
    L, buf = N.lib(), np.zeros(16, np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.vpt_surface_vertices(s._h, len(wv), 1, p, buf.nbytes) == N.ERR_INVALID and b'not within' in L.vpt_last_error()
    assert L.vpt_surface_quads(s._h, len(wq) + 1, 0, p, buf.nbytes) == N.ERR_INVALID
    assert L.vpt_surface_vertices(s._h, 0, 2, p, 23) == N.ERR_INVALID and b'too short' in L.vpt_last_error()
    assert L.vpt_surface_quads(s._h, 0, 1, None, 16) == N.ERR_INVALID
    assert L.vpt_surface_quads(s._h, 3, 0, None, 0) == N.OK
    assert L.vpt_surface_vertices(s._h, 1, 1, p, buf.nbytes) == N.OK and buf[:3].tolist() == wv[1].tolist() and not buf[3:].any()
    s.destroy(); vol.destroy()


def test_two_runs_identical_and_mesh_measures(gpu_ctx):
    z, y, x = np.indices((25, 25, 25)).astype(np.float64)
    ball = np.clip(np.rint(128 + 40 * (10 - np.sqrt((x - 12) ** 2 + (y - 12) ** 2 + (z - 12) ** 2))), 0, 255).astype(np.uint8)
    vol = upload(gpu_ctx, ball)
    a, b = vol.surface(128), vol.surface(128, _scan_words=5)
    assert a.vertices().tobytes() == b.vertices().tobytes() and a.quads().tobytes() == b.quads().tobytes()
    assert (a.info['vertices'], a.info['quads']) == (1904, 1902)
    wv, wq = surface_texels(ball, 128)
    from vpt_amd import surface as S
    assert a.area((1, 2, 3)) == S.area(wv, wq, (1, 2, 3)) and a.volume() == S.volume(wv, wq)
    assert np.array_equal(a.normals(), S.normals(wv, wq)) and np.array_equal(a.positions((2, 2, 2), (1, 0, 0)), S.positions(wv, (2, 2, 2), (1, 0, 0)))
    assert np.array_equal(a.triangles(), S.triangles(wq))
    assert set(a.profile) == {'inside', 'classify', 'scan', 'vertices', 'quads'} and all(ms > 0 for ms in a.profile.values())
    a.close(); b.close(); vol.destroy()
    with pytest.raises(RuntimeError, match='destroyed'):
        a.vertices()


def test_writers_from_the_device(gpu_ctx, tmp_path):
    from test_surface_host import read_obj, read_ply, read_stl
    a = noise((4, 5, 9), np.uint8, 25)
    wv, wq = surface_texels(a, 128)
    vol = upload(gpu_ctx, a)
    s = vol.surface(128)
    s.write_stl(str(tmp_path / 's.stl')); s.write_ply(str(tmp_path / 's.ply'), (1, 2, 3)); s.write_obj(str(tmp_path / 's.obj'))
    from vpt_amd import surface as S
    assert np.array_equal(read_stl(str(tmp_path / 's.stl'))[0][:, 1:, :], S.positions(wv)[S.triangles(wq)].astype(np.float32))
    p, _, faces = read_ply(str(tmp_path / 's.ply'))
    assert np.array_equal(p, S.positions(wv, (1, 2, 3)).astype(np.float32)) and np.array_equal(faces, wq)
    p, faces = read_obj(str(tmp_path / 's.obj'))
    assert np.array_equal(p, S.positions(wv)) and np.array_equal(faces, wq.astype(np.int64) + 1)
    s.destroy(); vol.destroy()


def test_argument_checks(gpu_ctx):
    L = N.lib()
    vol = upload(gpu_ctx, np.zeros((2, 2, 2), np.uint8))
    h = C.c_void_p()
    for level in (0, 256):
        assert L.vpt_volume_surface(vol.texture, 0, level, C.byref(h)) == N.ERR_INVALID and b'level' in L.vpt_last_error()
        with pytest.raises(ValueError, match='1 <= level <= 255'):
            vol.surface(level)
    for channel in (1, 2, -1):
        assert L.vpt_volume_surface(vol.texture, channel, 1, C.byref(h)) == N.ERR_INVALID and b'channel' in L.vpt_last_error()
    with pytest.raises(ValueError, match='channel 1 of a volume that has one channel'):
        vol.surface(1, 1)
    assert L.vpt_volume_surface(None, 0, 1, C.byref(h)) == N.ERR_INVALID and L.vpt_volume_surface(vol.texture, 0, 1, None) == N.ERR_INVALID
    assert L.vpt_volume_surface_capped(vol.texture, 0, 1, 0, C.byref(h)) == N.ERR_INVALID and b'scan_words' in L.vpt_last_error()
    vol.destroy()
    vol16 = upload(gpu_ctx, np.zeros((2, 2, 2), np.uint16))
    assert L.vpt_volume_surface(vol16.texture, 0, 65536, C.byref(h)) == N.ERR_INVALID
    vol16.destroy()
    for other in (np.zeros((2, 2, 2), np.float32), np.zeros((2, 2, 2), np.int8)):
        v = upload(gpu_ctx, other)
        assert L.vpt_volume_surface(v.texture, 0, 1, C.byref(h)) == N.ERR_UNSUPPORTED
        assert (b'R32F' if other.dtype == np.float32 else b'R8_SNORM') in L.vpt_last_error()
        v.destroy()
    assert L.vpt_surface_info(None, None) == N.ERR_INVALID and L.vpt_surface_destroy(None) == N.ERR_INVALID
    assert L.vpt_surface_profile(None, None) == N.ERR_INVALID and L.vpt_surface_device(None, None, None) == N.ERR_INVALID


def test_on_a_callers_stream_and_as_tensors():
    """a fresh process (torch's GPU state stays out of this one): upload_block_device enqueued on a caller's stream, then surface"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'surface_stream_worker.py')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=240)
    out = p.stdout.decode('utf-8', 'replace')
    assert p.returncode == 0 and 'PASS' in out, out
