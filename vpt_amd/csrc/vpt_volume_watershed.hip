// vpt_volume_watershed.hip — the watershed of a relief by steepest descent on its lower completion (vpt_volume_watershed): the basins as an
// ordinary vpt_components handle.  C-ABI and the contract: include/vpt.h; kernel forms, why the races are benign, compiler figures and
// measurements: DESIGN.md "Watershed".
//
// Every step is a pure function of the input.  One uint32 per voxel, dist, holds the lower completion d; one byte per voxel, dirs, the
// pointer p as a direction code.  The passes: classify (d = 0 or unset), the plateau kernel (a 64 x 8 x 4 tile relaxed to convergence in
// LDS, launched again over the tiles a neighbour flagged), the links inside a tile (p, then min-label propagation across linked pairs only),
// the links across tiles (unite on L), and the components' own tail (vpt_volume_components.h: flatten, sizes, census, list, ranks).  No
// workgroup waits for another: launch boundaries order the phases.
//
// Keys.  A voxel's key is k(v) = code ^ flip (flip = 0, or M for the maxima: M - c = c ^ M) when lo <= code <= hi, and WS_OUT otherwise.
// WS_OUT is larger than every key of D, so "a neighbour in D with a smaller key" is one unsigned compare, and equal to none, so "a
// neighbour in D with the same key" is another (the voxel that asks is in D).  A neighbour outside the volume reads as WS_OUT: it does not
// exist.
#include "vpt_volume_components.h"

#define WS_OUT 0xFFFFFFFFu          // the key of a voxel that is not in D
#define WS_UNSET 0xFFFFFFFFu        // d: infinity (a chain has fewer than 2^32 - 2 steps)
#define WS_SELF 13                  // the direction code (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) of no offset: a minimum voxel
#define WS_NONE 255                 // the direction code of a voxel that is not in D
// In-tile rounds of the plateau kernel: with the rim fixed, r rounds give every voxel the best chain of at most r steps, and a simple
// chain through the tile has fewer than CC_VOX steps; one more round sees that nothing changes.
#define WS_TILE_ROUNDS (CC_VOX + 1)

enum { WW_CHANGED = 0, WW_WORDS = 4 };

// Tile directions as bits: bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1) is the neighbouring tile at (dx, dy, dz); the tiles that hold a
// CONN-neighbour of the tile voxel (tx, ty, tz): a chain may leave the tile only where the voxel lies on that face.
template <int CONN> __device__ __forceinline__ uint32_t touched_tiles(int tx, int ty, int tz) {
    uint32_t m = 0u;
#pragma unroll
    for (int dz = -1; dz <= 1; dz++)
#pragma unroll
        for (int dy = -1; dy <= 1; dy++)
#pragma unroll
            for (int dx = -1; dx <= 1; dx++) {
                if (!is_neighbour<CONN>(dx, dy, dz)) continue;
                const bool x = dx == 0 || (dx < 0 ? tx == 0 : tx == CC_TX - 1), y = dy == 0 || (dy < 0 ? ty == 0 : ty == CC_TY - 1);
                const bool z = dz == 0 || (dz < 0 ? tz == 0 : tz == CC_TZ - 1);
                if (x && y && z) m |= 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
            }
    return m;
}

// The keys of a tile and its one-voxel rim into LDS, and d likewise when `dist` is given.  Bounds: a voxel is read only inside the volume, at element
// g * stride + channel of a source of n * stride elements (channel < stride) and at word g of dist (n words).
template <typename T>
__device__ __forceinline__ void stage_tile(const T *__restrict__ src, uint32_t stride, uint32_t channel, const uint32_t *dist, int nx, int ny, int nz, int x0, int y0,
                                           int z0, uint32_t lo, uint32_t hi, uint32_t flip, uint32_t *s_key, uint32_t *s_d) {
    for (int i = (int)threadIdx.x; i < CC_PAD; i += 256) {
        const int px = i % CC_PX, py = (i / CC_PX) % CC_PY, pz = i / (CC_PX * CC_PY);
        const int x = x0 + px - 1, y = y0 + py - 1, z = z0 + pz - 1;
        uint32_t key = WS_OUT, d = WS_UNSET;
        if (x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz) {
            const size_t g = ((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)x;
            const uint32_t c = (uint32_t)src[g * stride + channel];
            if (c >= lo && c <= hi) {
                key = c ^ flip;
                if (dist) d = ld_agent(&dist[g]);
            }
        }
        s_key[i] = key;
        if (s_d) s_d[i] = d;
    }
}
// LDS index of this thread's voxel k (j = tid + 256 k), -1 outside the volume
__device__ __forceinline__ int tile_voxel(int j, int x0, int y0, int z0, int nx, int ny, int nz) {
    const int tx = j % CC_TX, ty = (j / CC_TX) % CC_TY, tz = j / (CC_TX * CC_TY);
    if (x0 + tx >= nx || y0 + ty >= ny || z0 + tz >= nz) return -1;
    return ((tz + 1) * CC_PY + (ty + 1)) * CC_PX + (tx + 1);
}
__device__ __forceinline__ size_t tile_global(int j, int x0, int y0, int z0, int nx, int ny) {
    const int tx = j % CC_TX, ty = (j / CC_TX) % CC_TY, tz = j / (CC_TX * CC_TY);
    return ((size_t)(z0 + tz) * (size_t)ny + (size_t)(y0 + ty)) * (size_t)nx + (size_t)(x0 + tx);
}

// ---------------------------------------------------------------------------------------------
// the snapshot of one channel: k_ws_channel<T>
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_ws_channel(const T *__restrict__ src, uint32_t stride, uint32_t channel, T *__restrict__ dst, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dst[i] = src[i * stride + channel];
}

// ---------------------------------------------------------------------------------------------
// classify: k_ws_classify<T, CONN>
// ---------------------------------------------------------------------------------------------
// A workgroup of 256 threads owns a tile, eight voxels a thread; the keys of the tile and its rim are staged in LDS.  A voxel of D with a
// neighbour of smaller key gets d = 0, every other voxel WS_UNSET.  A tile that holds an unset voxel of D flags itself for the first
// plateau launch (a tile without one has nothing to relax, now or later: d = 0 never changes).
template <typename T, int CONN>
__global__ __launch_bounds__(256) void k_ws_classify(const T *__restrict__ src, uint32_t stride, uint32_t channel, uint32_t *__restrict__ dist, int nx, int ny, int nz,
                                                    uint32_t lo, uint32_t hi, uint32_t flip, uint32_t *__restrict__ dirty, uint32_t *__restrict__ words) {
    __shared__ uint32_t s_key[CC_PAD];
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * CC_TX, y0 = (int)blockIdx.y * CC_TY, z0 = (int)blockIdx.z * CC_TZ;
    stage_tile<T>(src, stride, channel, nullptr, nx, ny, nz, x0, y0, z0, lo, hi, flip, s_key, nullptr);
    __syncthreads();
    bool unset = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int j = tid + 256 * k, p = tile_voxel(j, x0, y0, z0, nx, ny, nz);
        if (p < 0) continue;
        const uint32_t own = s_key[p];
        uint32_t m = own;
#pragma unroll
        for (int dz = -1; dz <= 1; dz++)
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++)
                    if (is_neighbour<CONN>(dx, dy, dz)) m = min(m, s_key[p + (dz * CC_PY + dy) * CC_PX + dx]);
        const bool border = m < own;                                // (own = WS_OUT has m <= own too: it is stored as unset below)
        dist[tile_global(j, x0, y0, z0, nx, ny)] = own != WS_OUT && border ? 0u : WS_UNSET;
        unset = unset || (own != WS_OUT && !border);
    }
    if (__syncthreads_or(unset ? 1 : 0) && tid == 0) {
        dirty[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = 1u;
        st_agent(&words[WW_CHANGED], 1u);
    }
}

// ---------------------------------------------------------------------------------------------
// plateau distance: k_ws_plateau<T, CONN>
// ---------------------------------------------------------------------------------------------
// d is the shortest path, with unit weights and inside the level set, to the plateau's lower border: the unique fixed point of
// d(v) = min(d(v), 1 + min over the same-key neighbours u of d(u)) from d = 0 on the border and unset elsewhere.  Every value ever stored
// is the length of a real chain (by induction over the stores), so d only falls and never passes the fixed point.
// The tile's keys and d are staged with a one-voxel rim: the rim of d holds the neighbouring tiles' words as global memory has them now.
// A round relaxes every tile voxel in place: a neighbour read while its owner writes is the old or the new value, both lengths of real
// chains, and a round in which no thread wrote has read settled values only, so it proves the fixed point for this rim.  The loop ends
// there, or after `rounds` rounds; a tile that was cut short flags itself for the next launch.
// What fell is stored (each word by its tile's owner only, one aligned 32-bit store).  A rim word read while its owner stores is the old
// or the new value; whoever stored it flags this tile for the next launch, which reads the new one.  A voxel of the tile's outer layer
// that fell sets the next launch's flag of every existing tile that holds one of its CONN neighbours; whoever sets a flag raises
// words[WW_CHANGED].  Bounds: a tile voxel is read and written only inside the volume; flags are written at tile indices inside the grid.
template <typename T, int CONN>
__global__ __launch_bounds__(256) void k_ws_plateau(const T *__restrict__ src, uint32_t stride, uint32_t channel, uint32_t *dist, int nx, int ny, int nz, uint32_t lo,
                                                   uint32_t hi, uint32_t flip, int rounds, const uint32_t *__restrict__ dirty_now, uint32_t *__restrict__ dirty_next,
                                                   uint32_t *__restrict__ words) {
    __shared__ uint32_t s_key[CC_PAD], s_d[CC_PAD];
    __shared__ uint32_t s_dirs;
    const int tid = (int)threadIdx.x;
    const size_t tile = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (dirty_now[tile] == 0u) return;                              // (uniform) nothing in or around this tile is waiting
    const int x0 = (int)blockIdx.x * CC_TX, y0 = (int)blockIdx.y * CC_TY, z0 = (int)blockIdx.z * CC_TZ;
    if (tid == 0) s_dirs = 0u;
    stage_tile<T>(src, stride, channel, dist, nx, ny, nz, x0, y0, z0, lo, hi, flip, s_key, s_d);
    __syncthreads();
    // (the loops over a thread's eight voxels are not unrolled: unrolled, the 26 compares of each voxel stay live side by side and the
    // kernel needs every register of a SIMD for two waves)
    bool settled = false;
    for (int round = 0; round < rounds; round++) {
        bool changed = false;
#pragma unroll 1
        for (int k = 0; k < 8; k++) {
            const int p = tile_voxel(tid + 256 * k, x0, y0, z0, nx, ny, nz);
            if (p < 0) continue;
            const uint32_t own = s_d[p], key = s_key[p];
            if (key == WS_OUT || own == 0u) continue;                // not in D, or on the border: it never changes
            uint32_t m = WS_UNSET;
#pragma unroll
            for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++)
                        if (is_neighbour<CONN>(dx, dy, dz)) {
                            const int q = p + (dz * CC_PY + dy) * CC_PX + dx;
                            if (s_key[q] == key) m = min(m, s_d[q]);
                        }
            if (m != WS_UNSET && m + 1u < own) { s_d[p] = m + 1u; changed = true; }
        }
        if (!__syncthreads_or(changed ? 1 : 0)) { settled = true; break; }       // (uniform: the barrier's result)
    }
    // ---- what fell goes back (global memory still has what the launch began with: only this workgroup writes the tile's words)
    uint32_t dirs = 0u;
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        const int j = tid + 256 * k, p = tile_voxel(j, x0, y0, z0, nx, ny, nz);
        if (p < 0 || s_key[p] == WS_OUT) continue;
        const uint32_t v = s_d[p];
        uint32_t *word = &dist[tile_global(j, x0, y0, z0, nx, ny)];
        if (v == ld_agent(word)) continue;
        st_agent(word, v);
        dirs |= touched_tiles<CONN>(j % CC_TX, (j / CC_TX) % CC_TY, j / (CC_TX * CC_TY));
    }
    if (dirs) atomicOr(&s_dirs, dirs);
    __syncthreads();
    bool flagged = false;
    if (tid < 27 && ((s_dirs >> tid) & 1u)) {
        const int bx = (int)blockIdx.x + tid % 3 - 1, by = (int)blockIdx.y + (tid / 3) % 3 - 1, bz = (int)blockIdx.z + tid / 9 - 1;
        if (bx >= 0 && bx < (int)gridDim.x && by >= 0 && by < (int)gridDim.y && bz >= 0 && bz < (int)gridDim.z) {
            dirty_next[((size_t)bz * gridDim.y + (size_t)by) * gridDim.x + (size_t)bx] = 1u;
            flagged = true;
        }
    }
    if (tid == 0 && !settled) { dirty_next[tile] = 1u; flagged = true; }       // cut short: this tile goes on in the next launch
    if (flagged) st_agent(&words[WW_CHANGED], 1u);
}

// ---------------------------------------------------------------------------------------------
// links inside a tile: k_ws_links<T, CONN>
// ---------------------------------------------------------------------------------------------
// Keys and the settled d are staged with their rim.  Every voxel of D computes its pointer as a direction code (offsets are visited in the
// order of the linear index, so the first that qualifies is the one of smallest index): d unset: WS_SELF, a minimum voxel; d = 0: the
// neighbour of smallest key, strictly below its own; otherwise the first neighbour of its key with d one less.  The code goes to LDS and
// to global memory (the merge reads it).  Then a voxel v is LINKED to its neighbour u in the tile when p(v) = u, p(u) = v, or both are
// minimum voxels of one key; the 26 links of a voxel are one mask, kept in the LDS word that held its d.  The labelling is k_label_tiles'
// (min-label propagation with pointer jumping over 16-bit LDS indices; the same bound, CC_VOX rounds), across linked pairs only: it leaves
// L flat within the tile, a voxel naming the smallest voxel of its tile component, and counts those roots for the bound of the host's
// merge loop.
template <typename T, int CONN>
__global__ __launch_bounds__(256) void k_ws_links(const T *__restrict__ src, uint32_t stride, uint32_t channel, const uint32_t *__restrict__ dist,
                                                 uint8_t *__restrict__ dirs, uint32_t *__restrict__ L, int nx, int ny, int nz, uint32_t lo, uint32_t hi, uint32_t flip,
                                                 uint32_t *__restrict__ words) {
    __shared__ uint32_t s_key[CC_PAD], s_d[CC_PAD];
    __shared__ uint16_t lab[CC_PAD];
    __shared__ uint8_t s_dir[CC_PAD];
    __shared__ uint32_t s_changed, s_roots;
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * CC_TX, y0 = (int)blockIdx.y * CC_TY, z0 = (int)blockIdx.z * CC_TZ;
    stage_tile<T>(src, stride, channel, dist, nx, ny, nz, x0, y0, z0, lo, hi, flip, s_key, s_d);
    for (int i = tid; i < CC_PAD; i += 256) { lab[i] = (uint16_t)CC_BG; s_dir[i] = (uint8_t)WS_NONE; }
    if (tid == 0) s_roots = 0u;
    __syncthreads();
    // (the loops over a thread's eight voxels are not unrolled: unrolled, the compiler keeps the 8 x 26 link tests as lane masks and spills)
    bool any = false;
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        const int j = tid + 256 * k, p = tile_voxel(j, x0, y0, z0, nx, ny, nz);
        if (p < 0) continue;
        const uint32_t key = s_key[p], d = s_d[p];
        uint32_t code = WS_NONE;
        if (key != WS_OUT) {
            code = WS_SELF;
            uint32_t best = key;
            bool found = false;
#pragma unroll
            for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++)
                        if (is_neighbour<CONN>(dx, dy, dz)) {
                            const int q = p + (dz * CC_PY + dy) * CC_PX + dx;
                            const uint32_t ku = s_key[q];
                            const uint32_t b = (uint32_t)((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
                            if (d == 0u) { if (ku < best) { best = ku; code = b; } }
                            else if (d != WS_UNSET && !found && ku == key && s_d[q] == d - 1u) { code = b; found = true; }
                        }
            lab[p] = (uint16_t)p;
            any = true;
        }
        s_dir[p] = (uint8_t)code;
        dirs[tile_global(j, x0, y0, z0, nx, ny)] = (uint8_t)code;
    }
    if (__syncthreads_or(any ? 1 : 0)) {
        // d has done its work: its words now hold the links, bit b: the neighbour at direction code b is linked to this voxel (it lies in
        // the tile: the rim has no label).  A thread writes the words of its own voxels only, and reads no other word of d from here on.
        uint32_t *s_links = s_d;
#pragma unroll 1
        for (int k = 0; k < 8; k++) {
            const int p = tile_voxel(tid + 256 * k, x0, y0, z0, nx, ny, nz);
            if (p < 0) continue;
            const uint32_t own = s_dir[p], key = s_key[p];
            uint32_t linked = 0u;
            if (own != WS_NONE) {
#pragma unroll
                for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                        for (int dx = -1; dx <= 1; dx++)
                            if (is_neighbour<CONN>(dx, dy, dz)) {
                                const int q = p + (dz * CC_PY + dy) * CC_PX + dx;
                                const uint32_t b = (uint32_t)((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
                                const uint32_t theirs = s_dir[q];
                                const bool in_tile = lab[q] != CC_BG;       // (lab is not written between the barrier above and the next)
                                const bool link = own == b || theirs == 26u - b || (own == WS_SELF && theirs == WS_SELF && s_key[q] == key);
                                linked |= in_tile && link ? 1u << b : 0u;
                            }
            }
            s_links[p] = linked;
        }
        for (int round = 0; round < CC_VOX; round++) {
            if (tid == 0) s_changed = 0u;
            __syncthreads();
            bool changed = false;
#pragma unroll 1
            for (int k = 0; k < 8; k++) {
                const int p = tile_voxel(tid + 256 * k, x0, y0, z0, nx, ny, nz);
                if (p < 0) continue;
                const uint32_t linked = s_links[p];
                if (linked == 0u) continue;                  // outside D, or a basin of its own within the tile
                const uint32_t own = lab[p];
                uint32_t m = own;
#pragma unroll
                for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                        for (int dx = -1; dx <= 1; dx++)
                            if (is_neighbour<CONN>(dx, dy, dz)) {
                                const uint32_t open = (linked >> ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1))) & 1u;      // no link: the label reads as CC_BG
                                m = min(m, (uint32_t)lab[p + (dz * CC_PY + dy) * CC_PX + dx] | (CC_BG & (open - 1u)));
                            }
                if (m < own) { lab[p] = (uint16_t)m; changed = true; }
            }
            if (changed) s_changed = 1u;
            __syncthreads();
            if (s_changed == 0u) break;                    // (uniform: every thread reads the word between the same two barriers)
#pragma unroll 1
            for (int k = 0; k < 8; k++) {
                const int p = tile_voxel(tid + 256 * k, x0, y0, z0, nx, ny, nz);
                if (p < 0 || s_links[p] == 0u) continue;
                const uint32_t own = lab[p];
                const uint32_t up = lab[lab[own]];         // labels name voxels of D in the tile, never the rim
                if (up < own) lab[p] = (uint16_t)up;
            }
            __syncthreads();
        }
    }
    // ---- the global form: linear index + 1 of the tile component's smallest voxel, 0 outside D
    uint32_t roots = 0u;
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        const int j = tid + 256 * k, p = tile_voxel(j, x0, y0, z0, nx, ny, nz);
        if (p < 0) continue;
        const int l = (int)lab[p];
        uint32_t g = 0u;
        if (l != (int)CC_BG) {
            const int lx = l % CC_PX - 1, ly = (l / CC_PX) % CC_PY - 1, lz = l / (CC_PX * CC_PY) - 1;
            g = (uint32_t)(((size_t)(z0 + lz) * (size_t)ny + (size_t)(y0 + ly)) * (size_t)nx + (size_t)(x0 + lx)) + 1u;
            roots += l == p ? 1u : 0u;
        }
        L[tile_global(j, x0, y0, z0, nx, ny)] = g;
    }
    if (roots) atomicAdd(&s_roots, roots);
    __syncthreads();
    if (tid == 0 && s_roots) atomicAdd(&words[W_TILE_ROOTS], s_roots);
}

// ---------------------------------------------------------------------------------------------
// links across tiles: k_ws_merge<T, CONN>
// ---------------------------------------------------------------------------------------------
// One thread a voxel.  A voxel whose pointer leaves its tile unites with the voxel it names; a minimum voxel unites with each minimum
// neighbour of its key and of smaller linear index that lies in another tile (every such pair once; the links inside a tile were joined by
// k_ws_links).  Two voxels of D with direction code WS_SELF and equal codes have equal keys.  Bounds: the pointer of a voxel names a voxel
// of D (k_ws_links found it inside the volume); the 13 offsets are tested against the volume.
template <typename T, int CONN>
__global__ __launch_bounds__(256) void k_ws_merge(const T *__restrict__ src, uint32_t stride, uint32_t channel, const uint8_t *__restrict__ dirs, uint32_t *__restrict__ L,
                                                 int nx, int ny, int nz, size_t n, int cap, uint32_t *__restrict__ words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t code = dirs[i];
        if (code == WS_NONE) continue;
        const int x = (int)(i % (size_t)nx); const size_t r = i / (size_t)nx; const int y = (int)(r % (size_t)ny), z = (int)(r / (size_t)ny);
        if (code != WS_SELF) {
            const int xx = x + (int)(code % 3u) - 1, yy = y + (int)((code / 3u) % 3u) - 1, zz = z + (int)(code / 9u) - 1;
            if (xx < 0 || xx >= nx || yy < 0 || yy >= ny || zz < 0 || zz >= nz) continue;           // (cannot be: see above)
            if (xx / CC_TX == x / CC_TX && yy / CC_TY == y / CC_TY && zz / CC_TZ == z / CC_TZ) continue;
            unite(L, (uint32_t)i, (uint32_t)(((size_t)zz * (size_t)ny + (size_t)yy) * (size_t)nx + (size_t)xx), cap, words);
            continue;
        }
        const int fx = x % CC_TX, fy = y % CC_TY, fz = z % CC_TZ;
        if (fx != 0 && fy != 0 && fz != 0 && fx != CC_TX - 1 && fy != CC_TY - 1) continue;      // no smaller neighbour outside the tile
        const T own = src[i * stride + channel];
#pragma unroll
        for (int dz = -1; dz <= 0; dz++)
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    if (!is_neighbour<CONN>(dx, dy, dz)) continue;
                    if (dz == 0 && (dy > 0 || (dy == 0 && dx > 0))) continue;        // the 13 offsets to a smaller index
                    const int xx = x + dx, yy = y + dy, zz = z + dz;
                    if (xx < 0 || xx >= nx || yy < 0 || yy >= ny || zz < 0) continue;
                    if (xx / CC_TX == x / CC_TX && yy / CC_TY == y / CC_TY && zz / CC_TZ == z / CC_TZ) continue;
                    const size_t j = ((size_t)zz * (size_t)ny + (size_t)yy) * (size_t)nx + (size_t)xx;
                    if (dirs[j] != WS_SELF || src[j * stride + channel] != own) continue;
                    unite(L, (uint32_t)i, (uint32_t)j, cap, words);
                }
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
struct WsPlan {
    const vpt_volume *relief; uint32_t channel, lo, hi, flip; int conn, tile_rounds;
    double *ms; uint32_t *plateau_launches;            // either may be null
};

#define WS_LAUNCH(KERNEL, T, grid, st, ...) do { \
    if (plan.conn == 6) hipLaunchKernelGGL((KERNEL<T, 6>), grid, dim3(256), 0, st, __VA_ARGS__); \
    else if (plan.conn == 18) hipLaunchKernelGGL((KERNEL<T, 18>), grid, dim3(256), 0, st, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<T, 26>), grid, dim3(256), 0, st, __VA_ARGS__); } while (0)

// classify, the plateau launches and the links inside a tile: the tile pass components_build asks for.  `dirs` stays for the merge.
template <typename T>
static int watershed_tiles(vpt_components *c, const WsPlan &plan, uint8_t *dirs, uint32_t *cc_words) {
    const vpt_volume *v = plan.relief;
    hipStream_t st = c->ctx->stream;
    const size_t n = c->voxels();
    const dim3 grid((unsigned)((c->nx + CC_TX - 1) / CC_TX), (unsigned)((c->ny + CC_TY - 1) / CC_TY), (unsigned)((c->nz + CC_TZ - 1) / CC_TZ));
    const size_t tiles = (size_t)grid.x * grid.y * grid.z;
    const T *src = (const T *)v->linear.get();
    const uint32_t stride = (uint32_t)v->channels;
    DevBuf<uint32_t> dist, words, flags;                         // freed when the pass returns: it drains the stream first
    HIP_TRY(dist.alloc(n));
    HIP_TRY(words.alloc(WW_WORDS));
    HIP_TRY(flags.alloc(2 * tiles));
    double none[VPT_WATERSHED_PHASES] = {};
    double *ms = plan.ms ? plan.ms : none;
    uint32_t host_words[WW_WORDS] = {};
    HIP_TRY(hipStreamSynchronize(st));                           // what is in front of the pass is not its time
    PhaseClock clock(st);
    // ---- classify; flags[0 .. tiles) are the first plateau launch's
    HIP_TRY(hipMemsetAsync(flags, 0, tiles * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(words, 0, WW_WORDS * sizeof(uint32_t), st));
    WS_LAUNCH(k_ws_classify, T, grid, st, src, stride, plan.channel, dist.get(), c->nx, c->ny, c->nz, plan.lo, plan.hi, plan.flip, flags.get(), words.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_words, words, sizeof(host_words), hipMemcpyDeviceToHost, st));
    HIP_TRY(clock.lap_add(&ms[0]));
    // ---- plateau distance.  A launch takes the tiles flagged by the one before it (the first: by classify).  Every launch that sets a
    // flag has lowered a word of d (a flag is set by a tile in which a voxel fell, or which was cut short in a round that wrote); d only
    // falls and each word is bounded below by its fixed point, so the loop ends.
    for (uint32_t launch = 0; host_words[WW_CHANGED] != 0u; launch++) {
        const uint32_t *now = flags.get() + (size_t)(launch & 1u) * tiles;
        uint32_t *next = flags.get() + (size_t)((launch + 1u) & 1u) * tiles;
        HIP_TRY(hipMemsetAsync(next, 0, tiles * sizeof(uint32_t), st));
        HIP_TRY(hipMemsetAsync(words, 0, WW_WORDS * sizeof(uint32_t), st));
        WS_LAUNCH(k_ws_plateau, T, grid, st, src, stride, plan.channel, dist.get(), c->nx, c->ny, c->nz, plan.lo, plan.hi, plan.flip, plan.tile_rounds, now, next,
                  words.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host_words, words, sizeof(host_words), hipMemcpyDeviceToHost, st));
        HIP_TRY(clock.lap_add(&ms[1]));
        if (plan.plateau_launches) (*plan.plateau_launches)++;
    }
    // ---- pointers and the links inside a tile
    WS_LAUNCH(k_ws_links, T, grid, st, src, stride, plan.channel, (const uint32_t *)dist.get(), dirs, c->values.get(), c->nx, c->ny, c->nz, plan.lo, plan.hi, plan.flip,
              cc_words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.lap_add(&ms[2]));
    return VPT_OK;
}

template <typename T>
static void watershed_merge(vpt_components *c, const WsPlan &plan, const uint8_t *dirs, int cap, uint32_t *words) {
    const vpt_volume *v = plan.relief;
    const size_t n = c->voxels();
    WS_LAUNCH(k_ws_merge, T, dim3(stream_grid(n)), c->ctx->stream, (const T *)v->linear.get(), (uint32_t)v->channels, plan.channel, dirs, c->values.get(), c->nx, c->ny,
              c->nz, n, cap, words);
}

// the handle's snapshot: `texels` (R8 / R16), or the chosen channel of the relief
static int watershed_capture(vpt_components *c, const vpt_volume *relief, uint32_t channel, const vpt_volume *texels) {
    if (texels) return field_capture(c, texels);
    if (relief->channels == 1) return field_capture(c, relief);
    VPT_TRY(field_describe(c, relief, relief->norm16 ? VPT_FORMAT_R16 : VPT_FORMAT_R8));
    const size_t n = c->voxels();
    hipStream_t st = c->ctx->stream;                             // behind any upload into the relief
    if (relief->norm16) hipLaunchKernelGGL(k_ws_channel<uint16_t>, dim3(stream_grid(n)), dim3(256), 0, st, (const uint16_t *)relief->linear.get(), 2u, channel, (uint16_t *)c->texels.get(), n);
    else hipLaunchKernelGGL(k_ws_channel<uint8_t>, dim3(stream_grid(n)), dim3(256), 0, st, (const uint8_t *)relief->linear.get(), 2u, channel, c->texels.get(), n);
    HIP_TRY(hipGetLastError());
    return VPT_OK;
}

static int watershed_create(vpt_volume *relief, int channel, vpt_volume *texels, uint32_t lo, uint32_t hi, int polarity, int connectivity, uint32_t min_voxels,
                            int merge_steps, int flatten_steps, int tile_rounds, vpt_components **out, double *ms, uint32_t *plateau_launches) {
    if (!relief || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (relief->format != VPT_FORMAT_R8 && relief->format != VPT_FORMAT_RG8 && relief->format != VPT_FORMAT_R16 && relief->format != VPT_FORMAT_RG16)
        return fail(VPT_ERR_UNSUPPORTED, "watershed: the relief is an unsigned normalised volume (R8, RG8, R16, RG16; the window makes R8 / R16 of any scalar volume), not %s",
                    format_name(relief->format));
    if (channel != 0 && channel != 1) return fail(VPT_ERR_INVALID, "watershed: channel %d of the relief: 0 or 1 are taken", channel);
    if (channel == 1 && relief->channels != 2) return fail(VPT_ERR_INVALID, "watershed: channel 1 of the relief, which has one channel (%s)", format_name(relief->format));
    const uint32_t M = relief->norm16 ? 65535u : 255u;
    if (lo > hi) return fail(VPT_ERR_INVALID, "watershed domain [%u, %u]: lo exceeds hi", lo, hi);
    if (hi > M) return fail(VPT_ERR_INVALID, "watershed domain [%u, %u]: the largest code of %s is %u", lo, hi, format_name(relief->format), M);
    if (polarity != VPT_WATERSHED_MINIMA && polarity != VPT_WATERSHED_MAXIMA)
        return fail(VPT_ERR_INVALID, "watershed polarity %d: VPT_WATERSHED_MINIMA (0) or VPT_WATERSHED_MAXIMA (1) are taken", polarity);
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return fail(VPT_ERR_INVALID, "connectivity %d: 6, 18 or 26 are taken", connectivity);
    if (min_voxels < 1u) return fail(VPT_ERR_INVALID, "min_voxels 0: a basin has at least one voxel");
    if (texels) {
        if (texels->format != VPT_FORMAT_R8 && texels->format != VPT_FORMAT_R16)
            return fail(VPT_ERR_UNSUPPORTED, "watershed: texels are a one-channel unsigned normalised volume (R8, R16), not %s", format_name(texels->format));
        if (texels->ctx != relief->ctx) return fail(VPT_ERR_INVALID, "watershed: relief and texels belong to two contexts");
        if (texels->nx != relief->nx || texels->ny != relief->ny || texels->nz != relief->nz)
            return fail(VPT_ERR_INVALID, "watershed: the relief is %dx%dx%d and texels are %dx%dx%d", relief->nx, relief->ny, relief->nz, texels->nx, texels->ny, texels->nz);
        if (texels->norm16 != relief->norm16)
            return fail(VPT_ERR_INVALID, "watershed: the channels of the relief (%s) and of texels (%s) differ in width", format_name(relief->format), format_name(texels->format));
    }
    const uint64_t n = (uint64_t)relief->nx * (uint64_t)relief->ny * (uint64_t)relief->nz;
    if (n > 0xFFFFFFFEull) return fail(VPT_ERR_UNSUPPORTED, "watershed: %llu voxels exceed 2^32 - 2 (labels and counts are 32-bit)", (unsigned long long)n);
    if ((relief->ny + CC_TY - 1) / CC_TY > 65535 || (relief->nz + CC_TZ - 1) / CC_TZ > 65535) return fail(VPT_ERR_UNSUPPORTED, "watershed: volume too large");
    vpt_context *ctx = relief->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<vpt_components> c(new vpt_components());
    VPT_TRY(watershed_capture(c.get(), relief, (uint32_t)channel, texels));
    DevBuf<uint8_t> dirs;                                        // freed on return: every path below drains the stream first
    HIP_TRY(dirs.alloc((size_t)n));
    vpt_components *h = c.get();
    uint8_t *d = dirs.get();
    const WsPlan plan = { relief, (uint32_t)channel, lo, hi, polarity == VPT_WATERSHED_MAXIMA ? M : 0u, connectivity, tile_rounds, ms, plateau_launches };
    const bool wide = relief->norm16;
    const ComponentsPasses passes = {
        "watershed",
        [=](uint32_t *words) { return wide ? watershed_tiles<uint16_t>(h, plan, d, words) : watershed_tiles<uint8_t>(h, plan, d, words); },
        [=](int cap, uint32_t *words) { if (wide) watershed_merge<uint16_t>(h, plan, d, cap, words); else watershed_merge<uint8_t>(h, plan, d, cap, words); } };
    const int rc = components_build(h, min_voxels, merge_steps, flatten_steps, passes);
    (void)hipStreamSynchronize(ctx->stream);                     // the buffers are freed on return: nothing may still use them
    if (rc != VPT_OK) return rc;
    *out = c.release();
    return VPT_OK;
}

extern "C" int vpt_volume_watershed(vpt_volume *relief, int channel, vpt_volume *texels, uint32_t lo, uint32_t hi, int polarity, int connectivity, uint32_t min_voxels,
                                    vpt_components **out) {
    return watershed_create(relief, channel, texels, lo, hi, polarity, connectivity, min_voxels, CC_MERGE_STEPS, CC_FLATTEN_STEPS, WS_TILE_ROUNDS, out, nullptr, nullptr);
}

extern "C" int vpt_volume_watershed_timed(vpt_volume *relief, int channel, vpt_volume *texels, uint32_t lo, uint32_t hi, int polarity, int connectivity,
                                          uint32_t min_voxels, vpt_components **out, double *ms, uint32_t *plateau_launches) {
    if (!ms || !plateau_launches) return fail(VPT_ERR_INVALID, "null argument");
    for (int i = 0; i < VPT_WATERSHED_PHASES; i++) ms[i] = 0.0;
    *plateau_launches = 0u;
    return watershed_create(relief, channel, texels, lo, hi, polarity, connectivity, min_voxels, CC_MERGE_STEPS, CC_FLATTEN_STEPS, WS_TILE_ROUNDS, out, ms, plateau_launches);
}

// (for tests) the caps are checked first: a refused cap touches neither the other arguments nor the device
extern "C" int vpt_volume_watershed_capped(vpt_volume *relief, int channel, vpt_volume *texels, uint32_t lo, uint32_t hi, int polarity, int connectivity,
                                           uint32_t min_voxels, int merge_steps, int flatten_steps, int tile_rounds, vpt_components **out, double *ms,
                                           uint32_t *plateau_launches) {
    VPT_TRY(components_check_caps(merge_steps, flatten_steps));
    if (tile_rounds < 1) return fail(VPT_ERR_INVALID, "tile_rounds %d: a launch makes at least one round", tile_rounds);
    if (ms) for (int i = 0; i < VPT_WATERSHED_PHASES; i++) ms[i] = 0.0;
    if (plateau_launches) *plateau_launches = 0u;
    return watershed_create(relief, channel, texels, lo, hi, polarity, connectivity, min_voxels, merge_steps, flatten_steps, tile_rounds, out, ms, plateau_launches);
}
