"""The isosurface of a volume as a mesh by naive surface nets, on the host: the numpy statement of the contract the device kernels
(vpt_volume_surface and the vpt_surface_* family; include/vpt.h) are held to, for callers without a device and as the contract's
documentation; and what is asked of a mesh next (triangles, positions, area, volume, normals, the STL / PLY / OBJ writers).

uint8 and uint16 [depth][height][width] arrays (or [depth][height][width][2] with a ``channel``), 1 <= level <= M (255 or 65535).

  surface:   at code level - 1/2: no grid point ever lies on it, there are no degenerate cases
  grid:      voxel (x, y, z) is the grid point at those integer coordinates; the grid is padded by one layer on every side (-1 .. W, H, D);
             code(g) is the whole unsigned code inside the volume and 0 outside; inside(g) = code(g) >= level: a structure that touches
             the border is closed there
  cells:     cell c = (i, j, k), -1 <= i <= W - 1 (likewise j, k), has the eight corners c + o, o in {0, 1}^3, and twelve edges
  crossing:  a grid edge (g, g + e_a) crosses when inside differs at its ends.  With a = code(g), b = code(g + e_a):
             n = |2 level - 1 - 2 a|, d = 2 |b - a|, t = (n 65536 + d / 2) div d, 1 <= t <= 65535; the crossing point is
             g 65536 + t e_a, in fixed point of 1 / 65536 voxel
  vertex:    a cell is active when at least one of its edges crosses; m = the number of its crossing edges; per axis s = the sum over
             them of (crossing point - c 65536) and the stored coordinate q = (c_axis + 1) 65536 + (2 s + m) div (2 m), a uint32; the
             position in voxel-index units is q / 65536 - 1.  Vertices are numbered in raster order of their cells (k slowest, then j, i)
  quads:     per crossing edge (g, a), with u = (a + 1) mod 3 and v = (a + 2) mod 3: the vertices of the cells g - e_u - e_v, g - e_v, g,
             g - e_u, in that order when inside(g), in the order [0, 3, 2, 1] of that list otherwise; numbered by g in raster order, then
             by axis x, y, z.  The triangles are (q0, q1, q2) and (q0, q2, q3); the right-hand normals point from the object to the
             background

Everything is integers in a fixed order: two runs, the device, Python and Node give identical bytes."""
import struct

import numpy as np

ONE = 65536
INFO_FIELDS = ('vertices', 'quads', 'cells', 'inside', 'crossings', 'level', 'width', 'height', 'depth', 'channel')


def _whole(value, what):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise ValueError('%s is an integer, not %r' % (what, value))
    return int(value)


def check_channel(channel, channels):
    """the channel of a surface: 0, or 1 of a two-channel volume; raises ValueError otherwise"""
    channel = _whole(channel, 'channel')
    if channel not in (0, 1):
        raise ValueError('channel is 0 or 1, not %d' % channel)
    if channel >= channels:
        raise ValueError('channel 1 of a volume that has one channel')
    return channel


def check_level(level, largest):
    """the level of a surface in code units: an integer with 1 <= level <= largest; raises ValueError otherwise"""
    level = _whole(level, 'the level of a surface')
    if not 1 <= level <= largest:
        raise ValueError('surface level %d: 1 <= level <= %d' % (level, largest))
    return level


def check_window(first, n, count, what):
    """(first, n) of a window of the vertices or quads: integers with 0 <= first <= count and 0 <= n <= count - first (n None: to the
    end); raises ValueError otherwise"""
    first = _whole(first, 'the first of the %s read' % what)
    if not 0 <= first <= count:
        raise ValueError('%s %d .. are not within the %d of the surface' % (what, first, count))
    n = count - first if n is None else _whole(n, 'the number of %s read' % what)
    if not 0 <= n <= count - first:
        raise ValueError('%s %d .. +%d are not within the %d of the surface' % (what, first, n, count))
    return first, n


def _codes(array, channel):
    array = np.asarray(array)
    if array.dtype not in (np.uint8, np.uint16) or array.ndim not in (3, 4) or 0 in array.shape or (array.ndim == 4 and array.shape[3] != 2):
        raise ValueError('the surface takes a [depth][height][width] or [depth][height][width][2] uint8 or uint16 array')
    if max(array.shape[:3]) > 4096:
        raise ValueError('the surface takes at most 4096 voxels an axis')
    channel = check_channel(channel, 2 if array.ndim == 4 else 1)
    return (array[..., channel] if array.ndim == 4 else array), channel


def _box(a, axis, lo, n):
    """n entries of `a` along `axis` from `lo`"""
    index = [slice(None)] * 3
    index[axis] = slice(lo, lo + n)
    return a[tuple(index)]


def surface_texels(array, level, channel=0, info=None):
    """(vertices uint32 [V][3], quads uint32 [Q][4]) of the surface at ``level`` of channel ``channel`` of a uint8 or uint16 array: what
    ``Volume.surface(level, channel)`` holds on the device.  ``info``: a dict that receives INFO_FIELDS."""
    codes, channel = _codes(array, channel)
    level = check_level(level, int(np.iinfo(codes.dtype).max))
    D, H, W = codes.shape
    P = np.pad(codes.astype(np.int64), 1)                        # [z + 1][y + 1][x + 1]: the padded grid
    inside = P >= level
    cells = (D + 1, H + 1, W + 1)                                # [k + 1][j + 1][i + 1]
    # per numpy axis (0: z, 1: y, 2: x) the edges (g, g + e): do they cross, and where
    cross, t = [None] * 3, [None] * 3
    for ax in range(3):
        n = P.shape[ax] - 1
        a, b = _box(P, ax, 0, n), _box(P, ax, 1, n)
        cross[ax] = _box(inside, ax, 0, n) != _box(inside, ax, 1, n)
        den = np.where(cross[ax], 2 * np.abs(b - a), 1)
        t[ax] = np.where(cross[ax], (np.abs(2 * level - 1 - 2 * a) * ONE + den // 2) // den, 0)
    # per cell: m, and per axis s
    m = np.zeros(cells, np.int64)
    s = [np.zeros(cells, np.int64) for _ in range(3)]
    for ax in range(3):
        p, r = [o for o in range(3) if o != ax]
        for op in (0, 1):
            for orr in (0, 1):
                part = _box(_box(cross[ax], p, op, cells[p]), r, orr, cells[r])
                m += part
                s[ax] += _box(_box(t[ax], p, op, cells[p]), r, orr, cells[r])
                if op:
                    s[p] += part * ONE
                if orr:
                    s[r] += part * ONE
    active = m > 0
    ck, cj, ci = np.nonzero(active)                              # raster order: i fastest
    mm = m[active]
    q = [(c + 1) * ONE + (2 * sa[active] + mm) // (2 * mm) for c, sa in ((ci - 1, s[2]), (cj - 1, s[1]), (ck - 1, s[0]))]
    vertices = np.stack(q, axis=1).astype(np.uint32) if len(mm) else np.zeros((0, 3), np.uint32)
    number = np.cumsum(active.ravel()).reshape(cells) - 1        # the vertex of a cell, by the cell's array index
    # quads: per axis a (0: x, 1: y, 2: z) the crossing edges; g's padded index is the array index of cell g
    keys, rows = [], []
    for a in range(3):
        gz, gy, gx = np.nonzero(cross[2 - a])
        g = [gx, gy, gz]
        u, v = (a + 1) % 3, (a + 2) % 3

        def cell(du, dv):
            c = list(g)
            c[u] = c[u] - du
            c[v] = c[v] - dv
            return number[c[2], c[1], c[0]]
        c0, c1, c2, c3 = cell(1, 1), cell(0, 1), cell(0, 0), cell(1, 0)
        ins = inside[gz, gy, gx]
        rows.append(np.stack([c0, np.where(ins, c1, c3), c2, np.where(ins, c3, c1)], axis=1))
        keys.append(((gz * (H + 2) + gy) * (W + 2) + gx) * 3 + a)
    keys, rows = np.concatenate(keys), np.concatenate(rows)
    quads = rows[np.argsort(keys, kind='stable')].astype(np.uint32).reshape(-1, 4)
    if info is not None:
        info.update(vertices=len(vertices), quads=len(quads), cells=int(np.prod(cells)), inside=int(inside.sum()),
                    crossings=[int(cross[2 - a].sum()) for a in range(3)], level=level, width=W, height=H, depth=D, channel=channel)
    return vertices, quads


# ---- what is asked of a mesh ----
def _mesh(vertices, quads):
    vertices, quads = np.asarray(vertices), np.asarray(quads)
    if vertices.ndim != 2 or vertices.shape[1] != 3 or quads.ndim != 2 or quads.shape[1] != 4:
        raise ValueError('a surface is vertices [V][3] and quads [Q][4]')
    return vertices, quads


def _triple(value, what):
    out = np.asarray(value, np.float64)
    if out.shape != (3,) or not np.isfinite(out).all():
        raise ValueError('%s is three finite numbers (x, y, z), not %r' % (what, value))
    return out


def triangles(quads):
    """uint32 [2 Q][3]: the triangles (q0, q1, q2) and (q0, q2, q3) of every quad, in the quads' order"""
    quads = np.asarray(quads)
    return np.ascontiguousarray(quads[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3), dtype=np.uint32)


def positions(vertices, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """float64 [V][3]: (q / 65536 - 1) * spacing + origin, x y z"""
    spacing = _triple(spacing, 'spacing')
    if (spacing <= 0).any():
        raise ValueError('spacing is positive, not %r' % (tuple(spacing),))
    return (np.asarray(vertices).astype(np.float64) / ONE - 1.0) * spacing + _triple(origin, 'origin')


def _corners(vertices, quads, spacing):
    p = positions(vertices, spacing)
    tri = triangles(quads).astype(np.int64)
    return p, tri, p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]


def area(vertices, quads, spacing=(1, 1, 1)):
    """float64: the area of the triangles"""
    _, _, a, b, c = _corners(*_mesh(vertices, quads), spacing)
    return float(0.5 * np.sqrt((np.cross(b - a, c - a) ** 2).sum(axis=1)).sum())


def volume(vertices, quads, spacing=(1, 1, 1)):
    """float64: the volume the triangles enclose (positive: the normals point outwards)"""
    _, _, a, b, c = _corners(*_mesh(vertices, quads), spacing)
    return float((a * np.cross(b, c)).sum() / 6.0)


def normals(vertices, quads, spacing=(1, 1, 1)):
    """float64 [V][3]: per vertex the normalised sum of its triangles' normals, each weighted by the triangle's area"""
    p, tri, a, b, c = _corners(*_mesh(vertices, quads), spacing)
    n = np.cross(b - a, c - a)
    out = np.zeros_like(p)
    for k in range(3):
        np.add.at(out, tri[:, k], n)
    length = np.sqrt((out ** 2).sum(axis=1, keepdims=True))
    return out / np.where(length > 0, length, 1.0)


# ---- writers ----
def write_stl(path, vertices, quads, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """binary STL: per triangle its unit normal and three corners as float32"""
    vertices, quads = _mesh(vertices, quads)
    p = positions(vertices, spacing, origin)
    tri = triangles(quads).astype(np.int64)
    a, b, c = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    n = np.cross(b - a, c - a)
    length = np.sqrt((n ** 2).sum(axis=1, keepdims=True))
    n = n / np.where(length > 0, length, 1.0)
    rec = np.zeros(len(tri), np.dtype([('f', '<f4', (12,)), ('attr', '<u2')]))
    rec['f'] = np.concatenate([n, a, b, c], axis=1)
    with open(path, 'wb') as f:
        f.write(b'vpt surface'.ljust(80, b' '))
        f.write(struct.pack('<I', len(tri)))
        f.write(rec.tobytes())


def write_ply(path, vertices, quads, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """binary little-endian PLY: float32 x y z per vertex, four uint32 indices per face"""
    vertices, quads = _mesh(vertices, quads)
    p = positions(vertices, spacing, origin).astype('<f4')
    faces = np.zeros(len(quads), np.dtype([('n', 'u1'), ('v', '<u4', (4,))]))
    faces['n'] = 4
    faces['v'] = quads
    header = ('ply\nformat binary_little_endian 1.0\ncomment vpt surface\nelement vertex %d\nproperty float x\nproperty float y\n'
              'property float z\nelement face %d\nproperty list uchar uint vertex_indices\nend_header\n' % (len(p), len(quads)))
    with open(path, 'wb') as f:
        f.write(header.encode('ascii'))
        f.write(p.tobytes())
        f.write(faces.tobytes())


def write_obj(path, vertices, quads, spacing=(1, 1, 1), origin=(0, 0, 0)):
    """Wavefront OBJ: `v x y z` per vertex (the shortest decimals that give the float64 back), `f a b c d` per quad, 1-based"""
    vertices, quads = _mesh(vertices, quads)
    p = positions(vertices, spacing, origin)
    with open(path, 'w') as f:
        f.write('# vpt surface\n')
        f.write(''.join('v %r %r %r\n' % (float(x), float(y), float(z)) for x, y, z in p))
        f.write(''.join('f %d %d %d %d\n' % (a, b, c, d) for a, b, c, d in (np.asarray(quads).astype(np.int64) + 1)))
