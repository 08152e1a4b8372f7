"""Inputs the reconstruction tests share (tests/test_reconstruct_host.py, tests/test_gpu_reconstruct.py, tests/test_gpu_reconstruct_fuzz.py):
arrays are [depth][height][width], a voxel (x, y, z) is array[z, y, x].  The device's tile is 64 x 8 x 4 voxels."""
import heapq

import numpy as np

from vpt_amd.components import neighbour_offsets

TILE = (64, 8, 4)
DTYPES = (np.uint8, np.uint16)
CONNECTIVITIES = (6, 18, 26)
GEODESIC = (('fill_holes', 0), ('clear_border', 0), ('hmax', 0), ('hmax', 37), ('hmin', 29), ('dome', 41), ('maxima', 0), ('minima', 0))


def largest(dtype):
    return int(np.iinfo(dtype).max)


def scaled(a, dtype):
    """byte codes spread over the range of ``dtype`` (255 -> the largest code)"""
    return a.astype(np.uint8) if dtype == np.uint8 else (a.astype(np.uint16) * 257)


def value_sets(dtype, shape, seed):
    """[(name, marker, mask)] for a shape (x, y, z): independent noise over every code; noise over five codes, so that plateaus occur;
    a constant volume under a marker with one voxel above it"""
    nx, ny, nz = shape
    rng = np.random.default_rng(seed)
    M = largest(dtype)
    full = lambda: rng.integers(0, M + 1, size=(nz, ny, nx)).astype(dtype)
    codes = np.array([0, 60, 120, 200, 255])
    few = lambda: scaled(codes[rng.integers(0, len(codes), size=(nz, ny, nx))], dtype)
    constant = np.full((nz, ny, nx), M // 3, dtype=dtype)
    spike = np.zeros((nz, ny, nx), dtype=dtype)
    spike[nz // 2, ny // 2, nx // 2] = M
    return [('noise', full(), full()), ('plateaus', few(), few()), ('constant', spike, constant)]


def touching(shape, dtype, second):
    """(marker, mask): two voxels of code 200 in an empty mask, (63, 7, 3) and ``second``, the marker 150 on the first only: they are
    neighbours across a tile corner ((64, 8, 4): under 26 only) or across a tile edge ((64, 8, 3): under 18 and 26)"""
    nx, ny, nz = shape
    mask = np.zeros((nz, ny, nx), dtype=dtype)
    marker = np.zeros_like(mask)
    mask[3, 7, 63] = mask[second[2], second[1], second[0]] = 200
    marker[3, 7, 63] = 150
    return marker, mask


def serpentine(shape, dtype):
    """(marker, mask, voxels on the path): in the plane z = 0 every even row is a run of code 200 over the whole width, joined to the next
    even row by one voxel of the odd row between them, at alternating ends: one 6-connected path.  The marker is M on the path's first voxel
    (clamped to 200 by the mask), 0 elsewhere: the reconstruction is the mask, reached along the whole path."""
    nx, ny, nz = shape
    mask = np.zeros((nz, ny, nx), dtype=dtype)
    for y in range(0, ny, 2):
        mask[0, y, :] = 200
        if y + 2 < ny:
            mask[0, y + 1, nx - 1 if (y // 2) % 2 == 0 else 0] = 200
    marker = np.zeros_like(mask)
    marker[0, 0, 0] = largest(dtype)
    return marker, mask, int(np.count_nonzero(mask))


def shells(shape, dtype, nested=False):
    """a hollow box shell of code 200 one voxel inside the volume's border (closed under every connectivity), with a second shell inside
    its cavity when ``nested``; the cavities and the outside are 0"""
    nx, ny, nz = shape
    a = np.zeros((nz, ny, nx), dtype=dtype)

    def shell(m, code):
        a[m:nz - m, m:ny - m, m:nx - m] = code
        a[m + 1:nz - m - 1, m + 1:ny - m - 1, m + 1:nx - m - 1] = 0
    shell(1, 200)
    if nested:
        shell(3, 90)
    return a


def two_balls(second_x, dtype=np.uint8):
    """the worked example of the contract: a 28 x 16 x 16 grid with the balls (x - 9)^2 + (y - 8)^2 + (z - 8)^2 <= 36 and the same around
    x = ``second_x``, code 200"""
    z, y, x = np.mgrid[0:16, 0:16, 0:28]
    inside = ((x - 9) ** 2 + (y - 8) ** 2 + (z - 8) ** 2 <= 36) | ((x - second_x) ** 2 + (y - 8) ** 2 + (z - 8) ** 2 <= 36)
    return np.where(inside, 200, 0).astype(dtype)


def best_paths(marker, mask, connectivity):
    """reconstruction by dilation as the path statement, over Python integers: R(v) = max over the voxels s and the connected paths from s
    to v of min(r0(s), min of the mask along the path), found best first (a voxel is final when it leaves the heap: every later candidate
    is no higher)"""
    d, h, w = mask.shape
    r0 = [[[min(int(marker[z, y, x]), int(mask[z, y, x])) for x in range(w)] for y in range(h)] for z in range(d)]
    best = [[[-1] * w for _ in range(h)] for _ in range(d)]
    heap = [(-r0[z][y][x], z, y, x) for z in range(d) for y in range(h) for x in range(w)]
    heapq.heapify(heap)
    offsets = neighbour_offsets(connectivity)
    while heap:
        value, z, y, x = heapq.heappop(heap)
        value = -value
        if best[z][y][x] >= 0:
            continue
        best[z][y][x] = value
        for dz, dy, dx in offsets:
            zz, yy, xx = z + dz, y + dy, x + dx
            if 0 <= zz < d and 0 <= yy < h and 0 <= xx < w and best[zz][yy][xx] < 0:
                heapq.heappush(heap, (-min(value, int(mask[zz, yy, xx])), zz, yy, xx))
    return np.array(best, dtype=np.int64).astype(mask.dtype)
