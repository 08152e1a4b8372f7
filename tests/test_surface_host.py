"""CPU: the surface-nets statement (vpt_amd.surface.surface_texels): the worked example, the topology of the meshes it gives, the soft
ball's volume and area, the range of t, the argument checks, a plain-loop restatement of the contract, and the writers."""
import struct
from collections import Counter

import numpy as np
import pytest

from vpt_amd import surface as S
from vpt_amd.surface import surface_texels


# ---------------------------------------------------------------------------------------------
# the contract once more, in plain loops
# ---------------------------------------------------------------------------------------------
def crossing_t(a, b, level):
    n = abs(2 * level - 1 - 2 * a)
    d = 2 * abs(b - a)
    return (n * 65536 + d // 2) // d


def surface_loops(codes, level):
    D, H, W = codes.shape

    def code(g):
        x, y, z = g
        return int(codes[z, y, x]) if 0 <= x < W and 0 <= y < H and 0 <= z < D else 0

    def inside(g):
        return code(g) >= level

    def step(g, a, by=1):
        h = list(g)
        h[a] += by
        return tuple(h)

    number, vertices = {}, []
    for k in range(-1, D):
        for j in range(-1, H):
            for i in range(-1, W):
                c = (i, j, k)
                m, s = 0, [0, 0, 0]
                for a in range(3):
                    u, v = (a + 1) % 3, (a + 2) % 3
                    for ou in (0, 1):
                        for ov in (0, 1):
                            g = step(step(c, u, ou), v, ov)
                            h = step(g, a)
                            if inside(g) != inside(h):
                                point = [65536 * x for x in g]
                                point[a] += crossing_t(code(g), code(h), level)
                                m += 1
                                for axis in range(3):
                                    s[axis] += point[axis] - 65536 * c[axis]
                if m:
                    number[c] = len(vertices)
                    vertices.append([(c[axis] + 1) * 65536 + (2 * s[axis] + m) // (2 * m) for axis in range(3)])
    quads = []
    for z in range(-1, D + 1):
        for y in range(-1, H + 1):
            for x in range(-1, W + 1):
                g = (x, y, z)
                for a in range(3):
                    if g[a] + 1 > (W, H, D)[a] or inside(g) == inside(step(g, a)):
                        continue
                    u, v = (a + 1) % 3, (a + 2) % 3
                    four = [number[step(step(g, u, -1), v, -1)], number[step(g, v, -1)], number[g], number[step(g, u, -1)]]
                    quads.append(four if inside(g) else [four[0], four[3], four[2], four[1]])
    return np.array(vertices, np.uint32).reshape(-1, 3), np.array(quads, np.uint32).reshape(-1, 4)


# ---------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------
def grid(n):
    z, y, x = np.mgrid[:n, :n, :n].astype(np.float64)
    return x, y, z


def voxel13():
    a = np.zeros((13, 13, 13), np.uint8)
    a[6, 6, 6] = 255
    return a


def ball13():
    x, y, z = grid(13)
    return np.where((x - 6) ** 2 + (y - 6) ** 2 + (z - 6) ** 2 <= 4.5 ** 2, 255, 0).astype(np.uint8)


def torus13():
    x, y, z = grid(13)
    ring = np.sqrt((x - 6) ** 2 + (y - 6) ** 2) - 4.0
    return np.where(ring ** 2 + (z - 6) ** 2 <= 1.5 ** 2, 255, 0).astype(np.uint8)


def full13():
    return np.full((13, 13, 13), 200, np.uint8)


def corner_pair13():
    a = np.zeros((13, 13, 13), np.uint8)
    a[5, 5, 5] = a[6, 6, 6] = 255
    return a


def soft_ball():
    x, y, z = grid(25)
    r = np.sqrt((x - 12) ** 2 + (y - 12) ** 2 + (z - 12) ** 2)
    return np.clip(np.rint(128 + 40 * (10 - r)), 0, 255).astype(np.uint8)


def noise8():
    return np.random.default_rng(11).integers(0, 256, (5, 7, 9), dtype=np.uint8)


def noise16():
    return np.random.default_rng(12).integers(0, 65536, (4, 5, 6), dtype=np.uint16)


def edge_uses(quads):
    """(undirected edge -> quads that use it, directed edge -> times it occurs)"""
    undirected, directed = Counter(), Counter()
    for q in quads.tolist():
        for k in range(4):
            a, b = q[k], q[(k + 1) % 4]
            undirected[(min(a, b), max(a, b))] += 1
            directed[(a, b)] += 1
    return undirected, directed


def euler(vertices, quads):
    undirected, _ = edge_uses(quads)
    return len(vertices) - len(undirected) + len(quads)


def check_closed_oriented(vertices, quads):
    undirected, directed = edge_uses(quads)
    assert all(n % 2 == 0 for n in undirected.values())
    assert all(directed[(b, a)] == n for (a, b), n in directed.items())
    assert quads.max() < len(vertices)
    assert S.volume(vertices, quads) > 0
    return undirected


# ---------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------
def test_worked_example_to_the_digit():
    a = np.zeros((3, 3, 3), np.uint8)
    a[1, 1, 1] = 255
    info = {}
    v, q = surface_texels(a, 128, info=info)
    assert v.dtype == np.uint32 and q.dtype == np.uint32 and v.shape == (8, 3) and q.shape == (6, 4)
    assert v[0].tolist() == [120149, 120149, 120149] and v[7].tolist() == [141995, 141995, 141995]
    assert sorted(set(v.ravel().tolist())) == [120149, 141995]
    assert info == {'vertices': 8, 'quads': 6, 'cells': 64, 'inside': 1, 'crossings': [2, 2, 2], 'level': 128, 'width': 3, 'height': 3,
                    'depth': 3, 'channel': 0}
    # the first crossing in raster order of g is the z edge below the voxel: g = (1, 1, 0) is outside
    assert q[0].tolist() == [0, 2, 3, 1]
    assert crossing_t(0, 255, 128) == 32768


@pytest.mark.parametrize('shape, chi', [(voxel13, 2), (ball13, 2), (torus13, 0), (full13, 2)])
def test_manifold_shapes(shape, chi):
    v, q = surface_texels(shape(), 128)
    undirected = check_closed_oriented(v, q)
    assert set(undirected.values()) == {2}
    assert euler(v, q) == chi


def test_two_voxels_touching_at_a_corner():
    v, q = surface_texels(corner_pair13(), 128)
    undirected = check_closed_oriented(v, q)
    assert set(undirected.values()) == {2}
    assert len(q) == 12 and len(v) == 15              # the cell between them is shared: one vertex, not two


@pytest.mark.parametrize('make, level', [(noise8, 128), (noise16, 30000)])
def test_noise_stays_closed_and_oriented(make, level):
    v, q = surface_texels(make(), level)
    undirected = check_closed_oriented(v, q)
    assert 4 in set(undirected.values())


@pytest.mark.parametrize('make, levels', [(noise8, (1, 77, 128, 255)), (noise16, (1, 30000, 65535))])
def test_plain_loops_agree(make, levels):
    a = make()
    a.flat[3] = np.iinfo(a.dtype).max
    for level in levels:
        v, q = surface_texels(a, level)
        lv, lq = surface_loops(a, level)
        assert np.array_equal(v, lv) and np.array_equal(q, lq)


def test_soft_ball_volume_and_area():
    v, q = surface_texels(soft_ball(), 128)
    assert (len(v), len(q)) == (1904, 1902)
    check_closed_oriented(v, q)
    vol, ar = S.volume(v, q), S.area(v, q)
    print('soft ball: volume %.1f area %.1f' % (vol, ar))
    assert abs(vol / (4.0 / 3.0 * np.pi * 1000.0) - 1.0) < 0.015
    assert abs(ar / (4.0 * np.pi * 100.0) - 1.0) < 0.01
    # spacing scales them
    assert np.isclose(S.volume(v, q, (2, 3, 0.5)), 3.0 * vol) and np.isclose(S.area(v, q, (2, 2, 2)), 4.0 * ar)
    n = S.normals(v, q)
    centre = S.positions(v) - 12.0
    radial = centre / np.sqrt((centre ** 2).sum(axis=1, keepdims=True))
    assert ((n * radial).sum(axis=1) > 0.9).all()


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16])
def test_t_stays_in_range_at_the_extreme_levels(dtype):
    M = int(np.iinfo(dtype).max)
    for level in (1, M):
        seen = [crossing_t(a, b, level) for a in (0, level - 1) for b in (level, M)]
        seen += [crossing_t(b, a, level) for a in (0, level - 1) for b in (level, M)]
        assert min(seen) >= 1 and max(seen) <= 65535
    assert crossing_t(0, M, 1) == (1 if M == 65535 else 129) and crossing_t(0, M, M) == 65536 - crossing_t(0, M, 1)
    # and through the statement: a voxel of M beside zeros at both levels
    a = np.zeros((1, 1, 2), dtype)
    a[0, 0, 0] = M
    for level in (1, M):
        v, q = surface_texels(a, level)
        assert len(v) == 8 and len(q) == 6
        # at level 1 the surface hugs the voxel's neighbours, at level M the voxel itself: within the smallest t of a grid point
        far = np.abs(v.astype(np.int64) - 65536)
        assert far.max() <= (65536 if level == 1 else crossing_t(0, M, 1))


def test_nothing_reaches_the_level():
    info = {}
    v, q = surface_texels(np.full((3, 4, 5), 9, np.uint8), 10, info=info)
    assert v.shape == (0, 3) and q.shape == (0, 4) and v.dtype == np.uint32 and q.dtype == np.uint32
    assert info['vertices'] == 0 and info['quads'] == 0 and info['inside'] == 0 and info['cells'] == 4 * 5 * 6
    assert S.area(v, q) == 0.0 and S.volume(v, q) == 0.0 and S.triangles(q).shape == (0, 3)


def test_full_volume():
    info = {}
    v, q = surface_texels(np.full((2, 3, 4), 255, np.uint8), 1, info=info)
    assert (len(v), len(q)) == (54, 52)
    assert info['crossings'] == [2 * 3 * 2, 2 * 4 * 2, 2 * 4 * 3] and info['inside'] == 24
    undirected = check_closed_oriented(v, q)
    assert set(undirected.values()) == {2} and euler(v, q) == 2


def test_two_channels():
    rg = np.random.default_rng(5).integers(0, 256, (4, 5, 6, 2), dtype=np.uint8)
    for ch in (0, 1):
        v, q = surface_texels(rg, 100, ch)
        w, r = surface_texels(np.ascontiguousarray(rg[..., ch]), 100)
        assert np.array_equal(v, w) and np.array_equal(q, r)


def test_argument_checks():
    a = np.zeros((2, 2, 2), np.uint8)
    for level in (0, 256, -1):
        with pytest.raises(ValueError, match='1 <= level <= 255'):
            surface_texels(a, level)
    with pytest.raises(ValueError, match='1 <= level <= 65535'):
        surface_texels(a.astype(np.uint16), 65536)
    with pytest.raises(ValueError, match='is an integer'):
        surface_texels(a, 1.5)
    with pytest.raises(ValueError, match='is an integer'):
        surface_texels(a, True)
    with pytest.raises(ValueError, match='channel 1 of a volume that has one channel'):
        surface_texels(a, 1, 1)
    with pytest.raises(ValueError, match='channel is 0 or 1'):
        surface_texels(np.zeros((2, 2, 2, 2), np.uint8), 1, 2)
    for bad in (np.zeros((2, 2), np.uint8), np.zeros((2, 2, 2), np.float32), np.zeros((2, 2, 2, 3), np.uint8), np.zeros((0, 2, 2), np.uint8)):
        with pytest.raises(ValueError, match='uint8 or uint16 array'):
            surface_texels(bad, 1)
    v, q = surface_texels(voxel13(), 128)
    with pytest.raises(ValueError, match='spacing is positive'):
        S.positions(v, (1, 0, 1))
    with pytest.raises(ValueError, match='three finite numbers'):
        S.positions(v, (1, 1))
    with pytest.raises(ValueError, match=r'vertices \[V\]\[3\]'):
        S.area(v, q[:, :3])


def test_triangles_and_positions():
    v, q = surface_texels(voxel13(), 128)
    t = S.triangles(q)
    assert t.shape == (12, 3) and t[0].tolist() == q[0, [0, 1, 2]].tolist() and t[1].tolist() == q[0, [0, 2, 3]].tolist()
    p = S.positions(v, (2.0, 1.0, 0.5), (10.0, 0.0, -1.0))
    assert p.dtype == np.float64
    assert np.array_equal(p, (v.astype(np.float64) / 65536 - 1) * [2.0, 1.0, 0.5] + [10.0, 0.0, -1.0])
    # the vertices of a voxel of 255 among zeros lie a third and two thirds of the way round (6, 6, 6)
    assert np.allclose(np.abs(S.positions(v) - 6.0), 1.0 / 6.0, atol=1e-4)


# ---- the writers, read back ----
def read_stl(path):
    raw = open(path, 'rb').read()
    n, = struct.unpack_from('<I', raw, 80)
    assert len(raw) == 84 + 50 * n
    rec = np.frombuffer(raw, np.dtype([('f', '<f4', (12,)), ('attr', '<u2')]), offset=84)
    return rec['f'].reshape(n, 4, 3), rec['attr']


def read_ply(path):
    raw = open(path, 'rb').read()
    end = raw.index(b'end_header\n') + len(b'end_header\n')
    header = raw[:end].decode('ascii').split('\n')
    assert header[0] == 'ply' and header[1] == 'format binary_little_endian 1.0'
    nv = int([line for line in header if line.startswith('element vertex')][0].split()[-1])
    nf = int([line for line in header if line.startswith('element face')][0].split()[-1])
    p = np.frombuffer(raw, '<f4', 3 * nv, end).reshape(nv, 3)
    faces = np.frombuffer(raw, np.dtype([('n', 'u1'), ('v', '<u4', (4,))]), nf, end + 12 * nv)
    assert len(raw) == end + 12 * nv + 17 * nf
    return p, faces['n'], faces['v']


def read_obj(path):
    v, f = [], []
    for line in open(path):
        part = line.split()
        if part and part[0] == 'v':
            v.append([float(x) for x in part[1:]])
        elif part and part[0] == 'f':
            f.append([int(x) for x in part[1:]])
    return np.array(v, np.float64).reshape(-1, 3), np.array(f, np.int64).reshape(-1, 4)


def test_writers_round_trip(tmp_path):
    v, q = surface_texels(ball13(), 128)
    spacing, origin = (0.5, 0.25, 2.0), (-3.0, 1.0, 100.0)
    p = S.positions(v, spacing, origin)
    S.write_stl(str(tmp_path / 'a.stl'), v, q, spacing, origin)
    S.write_ply(str(tmp_path / 'a.ply'), v, q, spacing, origin)
    S.write_obj(str(tmp_path / 'a.obj'), v, q, spacing, origin)
    tri = S.triangles(q)
    facets, attr = read_stl(str(tmp_path / 'a.stl'))
    assert len(facets) == len(tri) and not attr.any()
    assert np.array_equal(facets[:, 1:, :], p[tri].astype(np.float32))
    a, b, c = (p[tri[:, k]] for k in range(3))
    n = np.cross(b - a, c - a)
    assert np.allclose(facets[:, 0, :], n / np.sqrt((n ** 2).sum(axis=1, keepdims=True)), atol=1e-6)
    pp, count, faces = read_ply(str(tmp_path / 'a.ply'))
    assert np.array_equal(pp, p.astype(np.float32)) and (count == 4).all() and np.array_equal(faces, q)
    op, of = read_obj(str(tmp_path / 'a.obj'))
    assert np.array_equal(op, p) and np.array_equal(of, q.astype(np.int64) + 1)
    # an empty surface writes valid files
    e = (np.zeros((0, 3), np.uint32), np.zeros((0, 4), np.uint32))
    S.write_stl(str(tmp_path / 'e.stl'), *e)
    S.write_ply(str(tmp_path / 'e.ply'), *e)
    S.write_obj(str(tmp_path / 'e.obj'), *e)
    assert len(read_stl(str(tmp_path / 'e.stl'))[0]) == 0 and len(read_ply(str(tmp_path / 'e.ply'))[0]) == 0
    assert len(read_obj(str(tmp_path / 'e.obj'))[0]) == 0


def test_64_cubed_takes_well_under_a_second():
    import time
    a = np.random.default_rng(3).integers(0, 256, (64, 64, 64), dtype=np.uint8)
    t0 = time.perf_counter()
    v, q = surface_texels(a, 128)
    took = time.perf_counter() - t0
    print('64^3 noise: %.3f s, %d vertices, %d quads' % (took, len(v), len(q)))
    assert len(v) > 250000
