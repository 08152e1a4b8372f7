"""A sequential model, in Python integers, of the merge and flatten phases of vpt_volume_components (vpt_amd/csrc/vpt_volume_components.hip)
with the two step caps of vpt_volume_components_capped, and the constructed input that makes a unite give up: shared by
tests/test_components_model.py (no device) and tests/test_gpu_components_retry.py.

The model restates find_root, unite, k_merge's choice of pairs, k_flatten and the host's two loops with their launch limits.  It performs
whole unites one after another, the threads' unites interleaved in a drawn order, and flattens voxel by voxel in a drawn order.  That is a
subset of what the device can do: there, loads and atomicMins of different unites interleave, and a unite can lose its atomicMin to
another.  So the model cannot show the device right; its job is to show that an input does what a GPU test says of it (this many merge
launches, a first flatten launch that raises the word) in every order the model can draw, before the input goes to a device."""
import numpy as np

from vpt_amd.components import components_texels

TILE = (64, 8, 4)                                                   # CC_TX, CC_TY, CC_TZ
TX, TY, TZ = TILE
MERGE_STEPS, FLATTEN_STEPS = 1024, 64                                # what vpt_volume_components passes
MERGE_STEPS_MIN, FLATTEN_STEPS_MIN = 3, 1                            # the smallest caps vpt_volume_components_capped takes
MOTIF_VOXELS = 5


def corner_motifs(shape):
    """(uint8 [nz][ny][nx] with 200 on the motifs and 0 elsewhere, the number of motifs): one motif at every (x0, y0, z0) of the volume
    with x0 one voxel into a tile and (y0, z0) on a tile corner that has a tile in front and a tile below.

    The motif: {(x0 - 1, y0, z0), (x0, y0, z0)}, the lone voxel (x0, y0, z0 - 1) in the tile below, and {(x0, y0 - 2, z0), (x0, y0 - 1, z0)}
    in the tile in front; one component of 5 voxels under every connectivity, no two motifs within two voxels of each other.  Under
    6-connectivity i = (x0, y0, z0) is the only voxel with a foreground neighbour of smaller index in another tile, so one thread makes
    both cross-tile unites and the order of arrival cannot change what happens.  With r = (x0 - 1, y0, z0) the root of i's tile component,
    l the lone voxel, f = (x0, y0 - 2, z0) the root of the neighbour g = (x0, y0 - 1, z0), and a merge cap of 3 steps:

      launch 1, unite(i, l):  L[i] names r (step 1), L[r] confirms r; L[l] confirms l; l < r: atomicMin hooks r under l.
                unite(i, g):  L[i] names r (step 1), L[r] names l (step 2), L[l] confirms l; L[g] names f (step 3): no step is left to
                              confirm f: the unite gives up and raises the word.  i -> r -> l: i is two links from its root.
      flatten:                cap 64: i, r name l, one launch.  cap 1: i reads L[r], reaches l and has no step left to confirm it: the
                              word is raised, and the second launch confirms l for every voxel: two launches.
      launch 2, unite(i, l):  both find l.   unite(i, g):  L[i] names l (step 1), confirmed; L[g] names f (step 2), L[f] confirms f
                              within the cap; l < f: f goes under l.  Nothing gives up: 2 merge launches.
      cap 1024: the second unite of launch 1 confirms f at its fourth load and hooks it: 1 merge launch; g -> f -> l is two links deep,
                so a flatten cap of 1 takes two launches behind it and a cap of 64 one."""
    nx, ny, nz = shape
    a = np.zeros((nz, ny, nx), np.uint8)
    count = 0
    for z0 in range(TZ, nz, TZ):
        for y0 in range(TY, ny, TY):
            for x0 in range(1, nx, TX):
                a[z0, y0, x0 - 1:x0 + 1] = 200
                a[z0 - 1, y0, x0] = 200
                a[z0, y0 - 2:y0, x0] = 200
                count += 1
    assert int((a == 200).sum()) == MOTIF_VOXELS * count
    return a, count


def at_least(ranks, listed, min_voxels):
    """(ranks, list) of the contract with `min_voxels`, from those with min_voxels = 1: the list is ordered by voxel count descending, so
    the components that stay are its head and keep their ranks; the voxels of the others get rank 0"""
    stay = [c for c in listed if c[3] >= min_voxels]
    assert stay == listed[:len(stay)]
    return np.where(ranks <= len(stay), ranks, 0).astype(np.uint32), stay


def merge_offsets(connectivity):
    """the (dz, dy, dx) to the neighbours of smaller linear index, in the order k_merge<CONN> visits them"""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dz, dy, dx) for dz in (-1, 0) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 1 <= (dx != 0) + (dy != 0) + (dz != 0) <= most and not (dz == 0 and (dy > 0 or (dy == 0 and dx > 0)))]


def flatten_launches(cap):
    """the limit of flatten launches behind one merge launch, as vpt_volume_components.hip derives it: a launch takes a depth d to at most
    ceil(d / (cap + 1)); behind j launches with ceil(2^32 / (cap + 1)^j) <= cap one more raises nothing; the limit is one more than that, j + 2"""
    j, p = 0, 1
    while -(-(1 << 32) // p) > cap:
        p *= cap + 1
        j += 1
    return j + 2


def contract_roots(foreground, connectivity):
    """list, one entry per voxel in linear order: the linear index + 1 of the root of the voxel's component by the contract, 0 for
    background: what L holds when the merge loop has ended"""
    d, h, w = foreground.shape
    ranks, listed = components_texels(foreground.astype(np.uint8), 1, 1, connectivity)
    table = np.zeros(len(listed) + 1, np.int64)
    for k, (x, y, z, _) in enumerate(listed):
        table[k + 1] = (z * h + y) * w + x + 1
    return table[ranks].reshape(-1).tolist()


def tile_labels(foreground, connectivity):
    """(L, tile components): what k_label_tiles leaves: every foreground voxel names the smallest voxel of its component WITHIN its tile"""
    d, h, w = foreground.shape
    L = np.zeros((d, h, w), np.int64)
    roots = 0
    for z0 in range(0, d, TZ):
        for y0 in range(0, h, TY):
            for x0 in range(0, w, TX):
                sub = foreground[z0:z0 + TZ, y0:y0 + TY, x0:x0 + TX]
                ranks, listed = components_texels(sub.astype(np.uint8), 1, 1, connectivity)
                table = np.zeros(len(listed) + 1, np.int64)
                for k, (x, y, z, _) in enumerate(listed):
                    table[k + 1] = ((z0 + z) * h + y0 + y) * w + x0 + x + 1
                L[z0:z0 + TZ, y0:y0 + TY, x0:x0 + TX] = table[ranks]
                roots += len(listed)
    return L.reshape(-1).tolist(), roots


def merge_threads(foreground, connectivity):
    """[[(i, j), ...], ...]: for every thread of k_merge that unites at all, its unites in the kernel's order"""
    d, h, w = foreground.shape
    offsets = merge_offsets(connectivity)
    threads = []
    for z, y, x in np.argwhere(foreground).tolist():
        fx, fy, fz = x % TX, y % TY, z % TZ
        if fx != 0 and fy != 0 and fz != 0 and fx != TX - 1 and fy != TY - 1:
            continue
        pairs = []
        for dz, dy, dx in offsets:
            xx, yy, zz = x + dx, y + dy, z + dz
            if xx < 0 or xx >= w or yy < 0 or yy >= h or zz < 0:
                continue
            if xx // TX == x // TX and yy // TY == y // TY and zz // TZ == z // TZ:
                continue
            if foreground[zz, yy, xx]:
                pairs.append(((z * h + y) * w + x, (zz * h + yy) * w + xx))
        if pairs:
            threads.append(pairs)
    return threads


def find_root(L, i, steps, cap):
    """(confirmed, voxel, steps)"""
    while steps < cap:
        p = L[i] - 1
        if p == i:
            return True, i, steps
        i = p
        steps += 1
    return False, i, steps


def unite(L, a, b, cap):
    """True when the unite gave up"""
    steps = 0
    for _ in range(cap):
        found, a, steps = find_root(L, a, steps, cap)
        if not found:
            return True
        found, b, steps = find_root(L, b, steps, cap)
        if not found:
            return True
        if a == b:
            return False
        if a < b:
            a, b = b, a
        old = L[a]
        L[a] = min(old, b + 1)                                      # atomicMin
        if old == a + 1:
            return False
        a = old - 1
    return True


def merge_launch(L, threads, cap, rng):
    """one k_merge launch, the threads' unites interleaved in a drawn order (each thread's own unites stay in order); True: the word is raised"""
    turns = rng.permutation(np.repeat(np.arange(len(threads)), [len(t) for t in threads])).tolist()
    at = [0] * len(threads)
    raised = False
    for t in turns:
        i, j = threads[t][at[t]]
        at[t] += 1
        raised = unite(L, i, j, cap) or raised
    return raised


def flatten_launch(L, voxels, cap, rng):
    """one k_flatten launch over the foreground voxels in a drawn order; True: the word is raised"""
    raised = False
    for i in rng.permutation(voxels).tolist():
        own = L[i]
        if own == i + 1:
            continue
        found, a, _ = find_root(L, own - 1, 0, cap)
        if a + 1 != own:
            L[i] = a + 1
        raised = raised or not found
    return raised


def label(foreground, connectivity, merge_steps, flatten_steps, rng):
    """(L, [flatten launches behind merge launch 1, behind merge launch 2, ...]): the host's loop of components_build over the model; the
    launch limits of the host are asserted"""
    assert merge_steps >= MERGE_STEPS_MIN and flatten_steps >= FLATTEN_STEPS_MIN
    d, h, w = foreground.shape
    L, tile_roots = tile_labels(foreground, connectivity)
    flattens = []
    if w <= TX and h <= TY and d <= TZ:
        return L, flattens
    threads = merge_threads(foreground, connectivity)
    voxels = np.flatnonzero(foreground.reshape(-1))
    while True:
        assert len(flattens) < tile_roots + 1, "the merge did not settle within %d launches" % (tile_roots + 1)
        gave_up = merge_launch(L, threads, merge_steps, rng)
        flattens.append(0)
        while True:
            assert flattens[-1] < flatten_launches(flatten_steps), "the labels were not flat after %d launches" % flattens[-1]
            flattens[-1] += 1
            if not flatten_launch(L, voxels, flatten_steps, rng):
                break
        if not gave_up:
            return L, flattens
