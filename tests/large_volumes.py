"""Sparse volumes of more than 2^31 and more than 2^32 voxels, and the small twin their expected texels come from.

A reference that touches every voxel of a 4 Gi-voxel volume costs minutes of numpy, so the large volumes hold content only in a few thin
slabs of whole z-planes (seeded uniform noise over every code, another seed per slab: an index that wraps into another slab reads other
data) and are background 0 elsewhere:

    slab 0                at z = 0 (the clamped lower edge),
    one slab per `mark`   straddling the plane that holds that linear voxel index (2^31; 2^30 where four-byte values pass byte 2^32),
    the last slab         ending at z = nz - 1 (the clamped upper edge; beyond voxel 2^32 in a volume of more than 2^32 voxels).

The twin is the slabs stacked along z with `gap` background planes between them.  A local operation whose taps reach `halo` planes sees,
within `halo` planes of a slab, the same texels in the twin as in the large volume as long as gap >= 2 * halo, so the numpy statement on
the twin is the expected result there (tests/test_large_volumes_host.py shows that on small shapes for every operation the GPU tests use).

Where the statement is too slow for planes of noise (reconstruction, watershed, thickness, skeleton), a slab holds a few small solids
instead and the expected texels come from the statement on a crop round each (`solids` and what follows it).

`sparse_volume` builds the vpt_amd.Volume the way Volume._from_raw_array does, without a host array of the whole volume:
vpt_volume_create zero-fills on the device, one vpt_volume_upload_block per slab, vpt_volume_finalize."""
import ctypes as C

import numpy as np

# nx, ny, nz.  With at most 4096 texels an axis a volume above 2^32 voxels has planes above 2^20 voxels: nz = 4096 gives the cheapest slabs.
TIER_B = {'aligned': (1056, 995, 4096), 'odd': (1029, 1023, 4096)}      # > 2^32 voxels; nx % 32 == 0 (the vector forms) / odd nx
TIER_A = {'aligned': (832, 788, 4096), 'odd': (811, 809, 4096)}         # > 2^31 and < 2^32 voxels; the plane of voxel 2^31 lies well inside
GIB = float(1 << 30)


def voxels(shape):
    nx, ny, nz = shape
    return nx * ny * nz


class Layout:
    """Where the slabs lie in a volume of `shape` = (nx, ny, nz) and in its twin: `thick` planes a slab, `gap` background planes between
    two slabs of the twin; `even`: every slab begins on an even plane in both (2 x 2 x 2 cells)."""

    def __init__(self, shape, thick, gap, marks=(1 << 31,), even=False):
        nx, ny, nz = shape
        self.shape, self.thick, self.gap, self.marks = (nx, ny, nz), thick, gap, tuple(marks)
        plane = nx * ny
        starts = [0]
        for mark in marks:
            assert 0 <= mark < plane * nz
            z0 = mark // plane - thick // 2
            starts.append(z0 + z0 % 2 if even else z0)            # (thick >= 2: an even start one plane up still holds the mark's plane)
        starts.append(nz - thick)
        if even:
            assert thick % 2 == 0 and gap % 2 == 0 and nz % 2 == 0
        self.starts = sorted(starts)
        for a, b in zip(self.starts, self.starts[1:]):
            assert b - (a + thick) >= max(gap, 1), "the slabs %r of %d planes do not keep %d planes apart" % (self.starts, thick, gap)
        for mark in marks:                                        # each mark lies inside a slab, with a plane on either side where it has three
            assert any(z0 <= mark // plane < z0 + thick for z0 in self.starts)
        self.twin_starts = [i * (thick + gap) for i in range(len(self.starts))]
        self.twin_depth = self.twin_starts[-1] + thick

    def noise(self, dtype, seed, channels=1):
        """one block [thick][ny][nx] (two channels: [...][2]) of uniform noise over every code per slab, seeds seed, seed + 1, ..."""
        nx, ny, _ = self.shape
        size = (self.thick, ny, nx) + ((2,) if channels == 2 else ())
        return [np.random.default_rng(seed + i).integers(0, int(np.iinfo(dtype).max) + 1, size=size).astype(dtype) for i in range(len(self.starts))]

    def _stack(self, blocks, starts, depth):
        nx, ny, _ = self.shape
        out = np.zeros((depth, ny, nx) + blocks[0].shape[3:], blocks[0].dtype)
        for z0, block in zip(starts, blocks):
            out[z0:z0 + self.thick] = block
        return out

    def twin(self, blocks):
        return self._stack(blocks, self.twin_starts, self.twin_depth)

    def whole(self, blocks):
        """the sparse volume itself on the host: for small shapes only"""
        return self._stack(blocks, self.starts, self.shape[2])

    def windows(self, halo=0):
        """[(z_lo, z_hi, t_lo)]: per slab the planes z_lo .. z_hi - 1 of the volume within `halo` planes of it and the twin's plane of z_lo"""
        assert self.gap >= 2 * halo
        nz = self.shape[2]
        out = []
        for z0, t0 in zip(self.starts, self.twin_starts):
            lo, hi = max(z0 - halo, 0), min(z0 + self.thick + halo, nz)
            out.append((lo, hi, t0 - (z0 - lo)))
        return out

    def halved(self):
        """`windows` of the 2x reduction (an `even` layout): the result planes of the slabs' cells"""
        return [(z0 // 2, (z0 + self.thick) // 2, t0 // 2) for z0, t0 in zip(self.starts, self.twin_starts)]

    def between(self, halo=0):
        """background planes of the volume: the one behind each slab's halo and the one midway to the next slab"""
        out = []
        for a, b in zip(self.starts, self.starts[1:]):
            out += [a + self.thick + halo, (a + self.thick + b) // 2]
        return sorted(set(out))

    def to_volume(self, t):
        """the volume's plane of the twin's plane t, which lies in a slab"""
        for z0, t0 in zip(self.starts, self.twin_starts):
            if t0 <= t < t0 + self.thick:
                return z0 + (t - t0)
        raise ValueError('plane %d of the twin is background' % t)


# ---- squared distances of thin slabs ---------------------------------------------------------------------------------------------
FAR = 1 << 30                                                   # beyond every sum of a finite d2 and a squared offset; sums stay below 2^31


def _along(g, axis, reach):
    g = np.moveaxis(g, axis, 0)
    out = g.copy()
    for k in range(1, min(reach, g.shape[0] - 1) + 1):
        np.minimum(out[k:], g[:-k] + k * k, out=out[k:])
        np.minimum(out[:-k], g[k:] + k * k, out=out[:-k])
    return np.moveaxis(out, 0, axis)


def distance_squared_within(seed, reach):
    """uint32 like vpt_amd.distance_squared_texels(...) of the boolean array `seed`, from the seeds at most `reach` voxels away along every
    axis only: the minimum over a subset of the seeds, so never below the true value, and equal to it wherever the result is at most
    reach^2 + 2 reach (the nearest seed of such a voxel is within `reach` along every axis).  The caller asserts that."""
    g = np.where(seed, np.int32(0), np.int32(FAR))
    for axis in (2, 1, 0):
        g = np.minimum(_along(g, axis, reach), FAR)
    return np.where(g >= FAR, 0xFFFFFFFF, g).astype(np.uint32)


REACH = 8                                                         # voxels along an axis within which the slabs' reference looks for seeds


def slab_distances(lay, blocks, lo, hi):
    """per slab the squared distances to the codes lo .. hi of that slab alone, which are the volume's there when the largest of them is
    below the squared gap to the next slab (asserted); computed from the seeds within REACH voxels along every axis, which is exact while
    every value is at most REACH^2 + 2 REACH (asserted)"""
    out = [distance_squared_within((b >= lo) & (b <= hi), REACH) for b in blocks]
    largest = max(int(d.max()) for d in out)
    nearest = min(b - (a + lay.thick) for a, b in zip(lay.starts, lay.starts[1:])) + 1
    assert largest <= REACH * REACH + 2 * REACH and largest < nearest * nearest and largest < (lay.gap + 1) ** 2
    return out, largest


# ---- histograms of a sparse volume ----------------------------------------------------------------------------------------------
def counts(blocks, nbins, shift, n):
    want = np.zeros(nbins, np.int64)
    for b in blocks:
        want += np.bincount((b.reshape(-1) >> shift).astype(np.int64), minlength=nbins)
    want[0] += n - sum(b.size for b in blocks)
    return want


# ---- a few small solids a slab, and the statements on crops round them --------------------------------------------------------------
# Statements that iterate to a fixed point (reconstruction, the watershed's plateaus), recurse over level sets (thickness) or visit voxels
# one by one (thinning) cost minutes on planes of 10^6 noise voxels.  `solids` fills a slab with background but for a few small solids with
# seeded noise inside; the expected texels come from the statement on a crop round each solid: the solid's box widened by MARGIN background
# voxels in x and y (cut at the volume's faces, the origin lowered to an even voxel), the whole slab along z with MARGIN background planes
# beyond it where the volume has background there and none at the volume's own first and last plane.  A crop's face is therefore a face of
# the volume or background, its origin is even on every axis when the slab's first plane is (Layout(..., even=True)), and two crops of a
# slab are disjoint, so two solids lie at least 2 MARGIN voxels apart.  tests/test_large_volumes_host.py shows per operation that this is
# the statement on the whole volume.
MARGIN = 2


def _ball(r):
    z, y, x = np.indices((2 * r + 1,) * 3) - r
    return x * x + y * y + z * z <= r * r + 1


def _shell():
    """a cube of 7 voxels with walls of 2 round an enclosed cavity of 3: the thinning keeps a closed surface, fill_holes fills the cavity,
    the surface closes twice"""
    s = np.ones((7, 7, 7), bool)
    s[2:5, 2:5, 2:5] = False
    return s


def _box(d, h, w):
    return np.ones((d, h, w), bool)


def _balls():
    """eight balls x^2 + y^2 + z^2 <= c in a row along x, a voxel apart: the largest D, and so T2, of each is another number (2, 3, 4, 5,
    6, 8, 9, 10)"""
    z, y, x = np.indices((7, 7, 7)) - 3
    return np.concatenate([np.pad(x * x + y * y + z * z <= c, ((0, 0), (0, 0), (0, 1))) for c in (1, 2, 3, 4, 5, 6, 8, 9)], axis=2)[:, :, :-1]


def solids(lay, dtype, seed, channels=1):
    """(blocks, crops): one block [thick][ny][nx] (two channels: [...][2]) per slab, 0 but for a few solids whose voxels hold seeded noise
    over the upper three quarters of the codes (seeds seed, seed + 1, ... per slab), and the crops [(slab, y0, y1, x0, x1)].
      first slab:  a box in the corner x = 0, y = 0, z = 0; a shell across the word edge x = 32 and the tile edges y = 8, z = 4; a bar along
                   x across the word edge x = 64
      a mark's slab:  a bar along x that holds the mark's voxel; a ball, bars along y and z, a plate
      last slab:   a box that holds the volume's last voxel; a ball.  In a volume of more than 2^32 voxels all of it lies beyond voxel 2^32
      every slab:  a row of eight balls of growing radius (one crop), so the thickness takes many values"""
    nx, ny, nz = lay.shape
    T, M = lay.thick, int(np.iinfo(dtype).max)
    assert T >= 8 and T % 2 == 0 and lay.gap >= MARGIN and nx >= 72 and ny >= 60
    blocks, crops = [], []
    for i, z0 in enumerate(lay.starts):
        rng = np.random.default_rng(seed + i)
        marks = [m for m in lay.marks if z0 <= m // (nx * ny) < z0 + T]
        if i == 0:
            placed = [(_box(5, 4, 6), 0, 0, 0), (_shell(), 1, 5, 28), (_box(3, 3, 13), 2, 14, 58), (_balls(), 1, 22, 4)]
        elif i == len(lay.starts) - 1:
            placed = [(_box(4, 5, 6), T - 4, ny - 5, nx - 6), (_ball(3), 0, 3, 5), (_balls(), 0, 14, 4)]
        else:
            (m,) = marks
            zm, ym, xm = m // (nx * ny) - z0, m // nx % ny, m % nx
            at = (min(max(zm - 1, 0), T - 3), min(max(ym - 1, 0), ny - 3), min(max(xm - 6, 0), nx - 13))
            yb = 2 if ym >= ny // 2 else ny - 29                   # the other solids keep to the half of the plane without the mark
            placed = [(_box(3, 3, 13),) + at, (_ball(3), 0, yb, 10), (_box(3, 13, 3), 4, yb, 24), (_box(T, 3, 3), 0, yb + 2, 36), (_box(2, 9, 11), 3, yb + 1, 44),
                      (_balls(), 1, yb + 18, 4)]
            assert placed[0][0][zm - at[0], ym - at[1], xm - at[2]]
        block = np.zeros((T, ny, nx) + ((2,) if channels == 2 else ()), dtype)
        mine = []
        for solid, z, y, x in placed:
            d, h, w = solid.shape
            assert 0 <= z and z + d <= T and 0 <= y and y + h <= ny and 0 <= x and x + w <= nx
            block[z:z + d, y:y + h, x:x + w][solid] = rng.integers(M // 4 + 1, M + 1, size=(int(solid.sum()),) + block.shape[3:])
            y0, x0 = max(y - MARGIN, 0), max(x - MARGIN, 0)
            mine.append((i, y0 - y0 % 2, min(y + h + MARGIN, ny), x0 - x0 % 2, min(x + w + MARGIN, nx)))
        for _, y0, y1, x0, x1 in mine:                              # a crop's face inside the volume is background
            rim = [block[:, y, x0:x1] for y, inner in ((y0, y0 > 0), (y1 - 1, y1 < ny)) if inner] + [block[:, y0:y1, x] for x, inner in ((x0, x0 > 0), (x1 - 1, x1 < nx)) if inner]
            assert not any(r.any() for r in rim)
        for a in range(len(mine)):
            for b in range(a):
                (_, ay0, ay1, ax0, ax1), (_, by0, by1, bx0, bx1) = mine[a], mine[b]
                assert ay1 <= by0 or by1 <= ay0 or ax1 <= bx0 or bx1 <= ax0, "two crops of slab %d overlap" % i
        blocks.append(block)
        crops += mine
    return blocks, crops


def crop_array(lay, blocks, crop):
    """(the crop as an array, its origin (z, y, x) in the volume, the background planes in front of the slab's)"""
    i, y0, y1, x0, x1 = crop
    z0, T = lay.starts[i], lay.thick
    lo, hi = (MARGIN if z0 > 0 else 0), (MARGIN if z0 + T < lay.shape[2] else 0)
    inner = blocks[i][:, y0:y1, x0:x1]
    a = np.zeros((lo + T + hi,) + inner.shape[1:], inner.dtype)
    a[lo:lo + T] = inner
    return a, (z0 - lo, y0, x0), lo


def on_crops(lay, blocks, crops, statement):
    """per slab an array [thick][ny][nx](...) of what `statement` makes of every crop, 0 elsewhere; the statement's result on a crop's
    background planes beyond the slab must be 0 too"""
    out = None
    for crop in crops:
        i, y0, y1, x0, x1 = crop
        a, _, lo = crop_array(lay, blocks, crop)
        r = statement(a)
        if out is None:
            out = [np.zeros(b.shape[:3] + r.shape[3:], r.dtype) for b in blocks]
        assert not r[:lo].any() and not r[lo + lay.thick:].any()
        out[i][:, y0:y1, x0:x1] = r[lo:lo + lay.thick]
    return out


def watershed_on_crops(lay, blocks, crops, lo, hi, polarity, connectivity, channel=0):
    """(rank blocks, the basins as (x, y, z, voxels) of the volume) of vpt_amd.watershed_texels with lo >= 1: no basin leaves its solid, so
    the volume's basins are the crops' together, ranked by voxel count descending, then by the root's linear index in the volume"""
    import vpt_amd
    assert lo >= 1
    nx, ny, _ = lay.shape
    found, per = [], []
    for c, crop in enumerate(crops):
        a, (oz, oy, ox), _ = crop_array(lay, blocks, crop)
        ranks, basins = vpt_amd.watershed_texels(a, lo, hi, polarity, connectivity, 1, channel)
        per.append((ranks, np.zeros(len(basins) + 1, np.uint32)))
        found += [(-v, ((z + oz) * ny + y + oy) * nx + x + ox, c, k + 1) for k, (x, y, z, v) in enumerate(basins)]
    found.sort()
    for rank, (_, _, c, k) in enumerate(found):
        per[c][1][k] = rank + 1
    it = iter(per)

    def ranked(_):                                                # (on_crops takes the crops in their order)
        ranks, table = next(it)
        return table[ranks]
    return on_crops(lay, blocks, crops, ranked), [(root % nx, root // nx % ny, root // (nx * ny), -v) for v, root, _, _ in found]


def skeleton_on_crops(lay, blocks, crops, lo, hi, mode, passes=0):
    """(burn blocks, info) of vpt_amd.skeleton_burn_texels: a voxel's fate depends on its 26 neighbours and on the parities of its
    coordinates only, so the crops thin independently; the counts add up and the volume needs as many passes as the slowest crop"""
    import vpt_amd
    infos = []

    def statement(a):
        burn, info = vpt_amd.skeleton_burn_texels(a, lo, hi, mode, passes)
        infos.append(info)
        return burn
    for crop in crops:
        assert all(o % 2 == 0 for o in crop_array(lay, blocks, crop)[1]), "the parities of a crop are not the volume's"
    out = on_crops(lay, blocks, crops, statement)
    info = {name: sum(i[name] for i in infos) for name in infos[0]}
    info['passes'], info['converged'] = max(i['passes'] for i in infos), min(i['converged'] for i in infos)
    return out, info


def graph_on_crops(lay, kept, crops):
    """(the graph_cases.Assembled graph of the volume, {'classes', 'branch_ranks', 'node_ranks': blocks per slab}) of the bool blocks
    `kept`: a voxel's class and a branch's record depend on 26-neighbours only, a crop keeps background on every face inside the volume, so
    the crops' graphs side by side are the volume's; ranks, node ranks and tips are translated to the volume (graph_cases.graph_on_pieces)"""
    from graph_cases import graph_on_pieces
    nx, ny, nz = lay.shape
    pieces = []
    for crop in crops:
        a, origin, _ = crop_array(lay, kept, crop)
        pieces.append((origin, a))
    graph = graph_on_pieces((nz, ny, nx), pieces)
    fields = {}
    for name in ('classes', 'branch_ranks', 'node_ranks'):
        fields[name] = [np.zeros(b.shape[:3], np.uint8 if name == 'classes' else np.uint32) for b in kept]
        for k, crop in enumerate(crops):                          # piece k is crop k
            i, y0, y1, x0, x1 = crop
            lo = crop_array(lay, kept, crop)[2]
            r = getattr(graph, name)(k)
            assert not r[:lo].any() and not r[lo + lay.thick:].any()
            fields[name][i][:, y0:y1, x0:x1] = r[lo:lo + lay.thick]
    return graph, fields


def surface_on_crops(lay, blocks, crops, level, channel=0):
    """(vertices, quads, info) of vpt_amd.surface.surface_texels: a crop's mesh is the part of the volume's in its cells (the statement
    reads 0 outside a crop as outside the volume, and a crop keeps background round its solid).  Its vertices move by the crop's origin;
    the volume numbers vertices by their cells in raster order and quads by the grid point g of their edge in raster order, then by the
    axis.  The cell of a vertex is its stored coordinate div 65536 (the fraction is below 1: a cell's crossings are never all on its upper
    face); the third vertex of a quad is the one of cell g, and the first differs from it along the two axes that are not the edge's."""
    from vpt_amd.surface import ONE, surface_texels
    nx, ny, nz = lay.shape
    V, Q, base = [], [], 0
    info = {'vertices': 0, 'quads': 0, 'inside': 0, 'crossings': [0, 0, 0]}
    for crop in crops:
        a, (oz, oy, ox), _ = crop_array(lay, blocks, crop)
        mine = {}
        v, q = surface_texels(a, level, channel, info=mine)
        V.append(v.astype(np.int64) + np.array([ox, oy, oz], np.int64) * ONE)
        Q.append(q.astype(np.int64) + base)
        base += len(v)
        for name in ('vertices', 'quads', 'inside'):
            info[name] += mine[name]
        info['crossings'] = [s + t for s, t in zip(info['crossings'], mine['crossings'])]
    v, q = np.concatenate(V), np.concatenate(Q)
    cell = v // ONE
    key = (cell[:, 2] * (ny + 2) + cell[:, 1]) * (nx + 2) + cell[:, 0]
    order = np.argsort(key, kind='stable')
    assert len(np.unique(key)) == len(key)
    number = np.empty(len(v), np.int64)
    number[order] = np.arange(len(v))
    axis = np.argmin(cell[q[:, 2]] - cell[q[:, 0]], axis=1)
    assert ((cell[q[:, 2]] - cell[q[:, 0]]).sum(axis=1) == 2).all()
    quads = number[q][np.argsort(key[q[:, 2]] * 3 + axis, kind='stable')]
    info.update(cells=(nx + 1) * (ny + 1) * (nz + 1), level=level, width=nx, height=ny, depth=nz, channel=channel)
    return v[order].astype(np.uint32), quads.astype(np.uint32), info


def shift_twin_vertices(lay, vertices):
    """the vertices of a surface of the twin as the volume has them: 65536 (z_volume - z_twin) added to the z word of each slab's (the
    cells of a slab are its planes and the one in front: gap >= 2 keeps the slabs' cells apart); their order and the quads stay"""
    from vpt_amd.surface import ONE
    assert lay.gap >= 2
    out = vertices.astype(np.int64)
    k = out[:, 2] // ONE                                          # the cell's z + 1
    seen = np.zeros(len(out), bool)
    for z0, t0 in zip(lay.starts, lay.twin_starts):
        mine = (k >= t0) & (k <= t0 + lay.thick)
        assert not (seen & mine).any()
        out[mine, 2] += ONE * (z0 - t0)
        seen |= mine
    assert seen.all()
    return out.astype(np.uint32)


def thickness_tiles(lay, d2_blocks):
    """the 8 x 8 x 4 tiles of the volume that hold a voxel with D > 0"""
    total = 0
    for z0, d2 in zip(lay.starts, d2_blocks):
        z, y, x = np.nonzero(d2)
        total += len(np.unique((((z + z0) // 4) * 4096 + y // 8) * 4096 + x // 8))
    return total


# ---- device memory ---------------------------------------------------------------------------------------------------------------
def _zorder_slots(nb):
    """slots of the brick array of nb = bricks per axis (vpt_volume_create's Z-order with as many bits per axis as the axis needs)"""
    nbits = [max(int(n - 1).bit_length(), 0) for n in nb]
    pos, total = [[0] * 16 for _ in range(3)], 0
    for level in range(16):
        for ax in range(3):
            if level < nbits[ax]:
                pos[ax][level] = total
                total += 1
    code = 0
    for ax in range(3):
        for k in range(nbits[ax]):
            code |= (((nb[ax] - 1) >> k) & 1) << pos[ax][k]
    return code + 1


def volume_bytes(shape, itemsize, channels=1):
    """device bytes of one volume: linear storage + bricks + boundary atlas (vpt_volume_create)"""
    nx, ny, nz = shape
    linear = nx * ny * nz * itemsize * channels
    shift = 7 + {1: 0, 2: 1, 4: 2}[itemsize] + (1 if channels == 2 else 0)
    bricks = (_zorder_slots([(n + 3) // 4 for n in shape]) << shift) + 64
    pitch = 1
    while pitch < max(nx, ny):
        pitch *= 2
    atlas = 6 * pitch * max(ny, nz) * channels * (4 if itemsize > 1 else 1) * 4
    return linear + bricks + atlas


def field_bytes(shape, itemsize):
    """device bytes of a Components / Distance handle: the snapshot of the texels and one uint32 per voxel"""
    return voxels(shape) * (itemsize + 4)


# ---- the device volume -----------------------------------------------------------------------------------------------------------
def sparse_volume(ctx, layout, blocks, filter='linear'):
    """The ready vpt_amd.Volume (R8 / RG8 / R16 / RG16 by the blocks' dtype and channels) of layout.shape whose slabs hold `blocks` and
    whose other texels are 0; no host array of the whole volume exists."""
    import vpt_amd
    from vpt_amd import _native as N
    from vpt_amd import volume as V
    nx, ny, nz = layout.shape
    dtype, channels = blocks[0].dtype, 2 if blocks[0].ndim == 4 else 1
    fmt, gltype, glformat, internal = {
        ('uint8', 1): (N.FORMAT_R8, V.GL_UNSIGNED_BYTE, V.GL_RED, V.GL_R8), ('uint8', 2): (N.FORMAT_RG8, V.GL_UNSIGNED_BYTE, V.GL_RG, V.GL_RG8),
        ('uint16', 1): (N.FORMAT_R16, V.GL_UNSIGNED_SHORT, V.GL_RED, V.GL_R16_EXT), ('uint16', 2): (N.FORMAT_RG16, V.GL_UNSIGNED_SHORT, V.GL_RG, V.GL_RG16_EXT),
    }[(dtype.name, channels)]
    L = N.lib()
    handle = C.c_void_p()
    N.check(L.vpt_volume_create(ctx._h, nx, ny, nz, fmt, C.byref(handle)))                 # zero-filled on the device
    vol = vpt_amd.Volume(ctx)
    vol.texture = handle
    try:
        for z0, block in zip(layout.starts, blocks):
            block = np.ascontiguousarray(block)
            assert block.shape[:3] == (layout.thick, ny, nx)
            N.check(L.vpt_volume_upload_block(handle, 0, 0, z0, nx, ny, layout.thick, block.ctypes.data_as(C.c_void_p), block.nbytes))
        N.check(L.vpt_volume_finalize(handle))
    except Exception:
        vol.destroy()
        raise
    dims = {'width': nx, 'height': ny, 'depth': nz}
    vol.modality = {'name': 'default', 'dimensions': dims, 'transform': {'matrix': [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]},
                    'format': glformat, 'internalFormat': internal, 'type': gltype,
                    'placements': [{'index': 0, 'position': {'x': 0, 'y': 0, 'z': 0}}]}
    vol.metadata = {'meta': {'version': 1}, 'modalities': [vol.modality], 'blocks': [{'url': None, 'format': 'raw', 'dimensions': dict(dims)}]}
    vol.ready = True
    vol.setFilter(filter)
    return vol


def planes(vol, z_lo, z_hi):
    """whole planes z_lo .. z_hi - 1 of a volume (the contiguous copy)"""
    d = vol.modality['dimensions']
    return vol.read_block(0, 0, z_lo, d['width'], d['height'], z_hi - z_lo)


def differences(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, "%s: %s %s, expected %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d values differ (%s), first at %s: %s, expected %s" % (len(bad), what, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
