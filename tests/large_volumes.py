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
        self.shape, self.thick, self.gap = (nx, ny, nz), thick, gap
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
