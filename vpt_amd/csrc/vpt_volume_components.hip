// vpt_volume_components.hip — the connected components of a value range of a volume on the device (vpt_volume_components and the
// vpt_components_* family): per-voxel ranks in the canonical order, the component list, and the two emitters (keep, label).  C-ABI and the
// contract: include/vpt.h; kernel forms, compiler figures, the loop bounds and measurements: DESIGN.md "Connected components".
//
// One uint32 per voxel, L, is first a parent array (L[i] = index of i's parent + 1, 0 = background; a root has L[i] = i + 1) and at the end
// the voxel's rank.  Every link ever written joins two voxels of one component and points to a smaller index, so parents only decrease and
// the root of a finished component is its smallest voxel whatever the order of arrival.  No workgroup waits for another: launch
// boundaries order the phases, and within the merge launch L is touched through device-scope integer atomics only.
#include "vpt_volume_components.h"

// ---------------------------------------------------------------------------------------------
// tile labelling: k_label_tiles<T, CONN>
// ---------------------------------------------------------------------------------------------
// A workgroup of 256 threads owns a CC_TX x CC_TY x CC_TZ tile, eight voxels a thread.  The tile's foreground is staged in LDS as one
// uint16 per voxel with a one-voxel background rim (no bounds tests in the loop): a foreground voxel starts with its own LDS index, which
// orders the tile's voxels as the linear index does.  Each round every voxel takes the smallest label among itself and its neighbours, then
// follows label -> label of the voxel it names twice (pointer jumping); a voxel's label is written by its owner only, and a value read
// while a neighbour's owner writes is the old or the new label, both labels of the same component.  A round without a change leaves every
// component with its smallest voxel's index.  Each changing round lowers a label, and a label moves at least one voxel per round along a
// shortest path, so CC_VOX rounds always suffice: that is the loop's bound.  (The tile's geometry, the control words and is_neighbour:
// vpt_volume_components.h, shared with the watershed's tile passes.)
template <typename T, int CONN>
__global__ __launch_bounds__(256) void k_label_tiles(const T *__restrict__ src, uint32_t *__restrict__ L, int nx, int ny, int nz, uint32_t lo, uint32_t hi,
                                                    uint32_t *__restrict__ words) {
    __shared__ uint16_t lab[CC_PAD];
    __shared__ uint32_t s_changed, s_roots;
    const int tid = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * CC_TX, y0 = (int)blockIdx.y * CC_TY, z0 = (int)blockIdx.z * CC_TZ;
    for (int i = tid; i < CC_PAD; i += 256) lab[i] = (uint16_t)CC_BG;
    if (tid == 0) s_roots = 0u;
    __syncthreads();
    int at[8];                  // LDS index of this thread's voxel k, -1: outside the volume
    bool any = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int j = tid + 256 * k, tx = j % CC_TX, ty = (j / CC_TX) % CC_TY, tz = j / (CC_TX * CC_TY);
        const int x = x0 + tx, y = y0 + ty, z = z0 + tz;
        at[k] = -1;
        if (x < nx && y < ny && z < nz) {
            const int p = ((tz + 1) * CC_PY + (ty + 1)) * CC_PX + (tx + 1);
            at[k] = p;
            const uint32_t c = (uint32_t)src[((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)x];
            if (c >= lo && c <= hi) { lab[p] = (uint16_t)p; any = true; }
        }
    }
    if (__syncthreads_or(any ? 1 : 0)) {
        for (int round = 0; round < CC_VOX; round++) {
            if (tid == 0) s_changed = 0u;
            __syncthreads();
            bool changed = false;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int p = at[k];
                if (p < 0) continue;
                const uint32_t own = lab[p];
                if (own == CC_BG) continue;
                uint32_t m = own;
#pragma unroll
                for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                        for (int dx = -1; dx <= 1; dx++)
                            if (is_neighbour<CONN>(dx, dy, dz)) m = min(m, (uint32_t)lab[p + (dz * CC_PY + dy) * CC_PX + dx]);     // the rim reads as CC_BG
                if (m < own) { lab[p] = (uint16_t)m; changed = true; }
            }
            if (changed) s_changed = 1u;
            __syncthreads();
            if (s_changed == 0u) break;                    // (uniform: every thread reads the word between the same two barriers)
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int p = at[k];
                if (p < 0) continue;
                const uint32_t own = lab[p];
                if (own == CC_BG) continue;
                const uint32_t up = lab[lab[own]];         // labels name foreground voxels of the same component, never the rim
                if (up < own) lab[p] = (uint16_t)up;
            }
            __syncthreads();
        }
    }
    // ---- the global form: linear index + 1 of the component's smallest voxel in the tile, 0 for background
    uint32_t roots = 0u;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int p = at[k];
        if (p < 0) continue;
        const int j = tid + 256 * k, tx = j % CC_TX, ty = (j / CC_TX) % CC_TY, tz = j / (CC_TX * CC_TY);
        const size_t i = ((size_t)(z0 + tz) * (size_t)ny + (size_t)(y0 + ty)) * (size_t)nx + (size_t)(x0 + tx);
        const uint32_t l = lab[p];
        uint32_t g = 0u;
        if (l != CC_BG) {
            const int lx = (int)l % CC_PX - 1, ly = ((int)l / CC_PX) % CC_PY - 1, lz = (int)l / (CC_PX * CC_PY) - 1;
            g = (uint32_t)(((size_t)(z0 + lz) * (size_t)ny + (size_t)(y0 + ly)) * (size_t)nx + (size_t)(x0 + lx)) + 1u;
            roots += l == (uint32_t)p ? 1u : 0u;
        }
        L[i] = g;
    }
    if (roots) atomicAdd(&s_roots, roots);
    __syncthreads();
    if (tid == 0 && s_roots) atomicAdd(&words[W_TILE_ROOTS], s_roots);      // the tile components: the bound of the host's merge loop
}

// ---------------------------------------------------------------------------------------------
// merging across tile faces: k_merge<CONN>; flatten: k_flatten
// ---------------------------------------------------------------------------------------------
// The label equivalence on L (find_root, unite): vpt_volume_components.h.
// One thread a voxel; a foreground voxel unites with each foreground neighbour of smaller linear index that lies in ANOTHER tile (every
// pair once; pairs inside a tile were joined by k_label_tiles).
template <int CONN>
__global__ __launch_bounds__(256) void k_merge(uint32_t *__restrict__ L, int nx, int ny, int nz, size_t n, int cap, uint32_t *__restrict__ words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % (size_t)nx); const size_t r = i / (size_t)nx; const int y = (int)(r % (size_t)ny), z = (int)(r / (size_t)ny);
        const int fx = x % CC_TX, fy = y % CC_TY, fz = z % CC_TZ;
        if (fx != 0 && fy != 0 && fz != 0 && fx != CC_TX - 1 && fy != CC_TY - 1) continue;      // no smaller neighbour outside the tile
        if (ld_agent(&L[i]) == 0u) continue;
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
                    if (ld_agent(&L[j]) == 0u) continue;
                    unite(L, (uint32_t)i, (uint32_t)j, cap, words);
                }
    }
}
// Every voxel takes the ancestor it reaches within `cap` loads.  Links written meanwhile by other threads name ancestors too, so a voxel at
// depth d ends at depth <= ceil(d / (cap + 1)) (flatten_launches has the argument); one that could not confirm a root raises W_CHANGED.
__global__ __launch_bounds__(256) void k_flatten(uint32_t *__restrict__ L, size_t n, int cap, uint32_t *__restrict__ words) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t own = ld_agent(&L[i]);
        if (own == 0u || own == (uint32_t)i + 1u) continue;
        uint32_t a = own - 1u;
        int steps = 0;
        const bool rooted = find_root(L, a, steps, cap);
        if (a + 1u != own) st_agent(&L[i], a + 1u);
        if (!rooted) st_agent(&words[W_CHANGED], 1u);
    }
}

// ---------------------------------------------------------------------------------------------
// sizes, census, compaction, the rank table
// ---------------------------------------------------------------------------------------------
// L is flat here: a voxel names its root.  A wave takes 64 consecutive voxels a step; runs of one root along x add once (integer atomicAdd:
// any order gives the same counts).
__global__ __launch_bounds__(256) void k_sizes(const uint32_t *__restrict__ L, size_t n, uint32_t *__restrict__ count) {
    const int lane = (int)threadIdx.x & 63;
    for (size_t base = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n; base += (size_t)gridDim.x * 256) {
        const size_t i = base + lane;
        const uint32_t l = i < n ? L[i] : 0u;
        const uint32_t before = __shfl_up(l, 1);
        const bool head = lane == 0 || l != before;
        const unsigned long long heads = __ballot(head);
        if (head && l) {
            const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
            atomicAdd(&count[l - 1u], (uint32_t)(rest ? __ffsll(rest) : 64 - lane));
        }
    }
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// components listed and dropped, voxels in range and in listed components: 64-bit integer sums, one atomicAdd per wave and quantity
__global__ __launch_bounds__(256) void k_census(const uint32_t *__restrict__ L, const uint32_t *__restrict__ count, size_t n, uint32_t min_voxels,
                                               unsigned long long *__restrict__ sums) {
    unsigned long long listed = 0, dropped = 0, fg = 0, lv = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t l = L[i];
        fg += l != 0u;
        if (l == (uint32_t)i + 1u) {
            const uint32_t c = count[i];
            if (c >= min_voxels) { listed++; lv += c; } else dropped++;
        }
    }
    listed = wave_sum(listed); dropped = wave_sum(dropped); fg = wave_sum(fg); lv = wave_sum(lv);
    if (((int)threadIdx.x & 63) == 0) {
        if (listed) atomicAdd(&sums[Q_LISTED], listed);
        if (dropped) atomicAdd(&sums[Q_DROPPED], dropped);
        if (fg) atomicAdd(&sums[Q_FOREGROUND], fg);
        if (lv) atomicAdd(&sums[Q_LISTED_VOXELS], lv);
    }
}
// the (root, voxels) pairs of the listed components, in the order the waves arrive: a wave reserves its slots with one atomicAdd
__global__ __launch_bounds__(256) void k_compact(const uint32_t *__restrict__ L, const uint32_t *__restrict__ count, size_t n, uint32_t min_voxels,
                                                uint2 *__restrict__ list, uint32_t capacity, uint32_t *__restrict__ words) {
    const int lane = (int)threadIdx.x & 63;
    for (size_t base = (size_t)blockIdx.x * 256 + (threadIdx.x & ~63u); base < n; base += (size_t)gridDim.x * 256) {
        const size_t i = base + lane;
        uint32_t c = 0u;
        if (i < n && L[i] == (uint32_t)i + 1u) c = count[i];
        const bool take = c != 0u && c >= min_voxels;
        const unsigned long long takes = __ballot(take);
        if (takes == 0ull) continue;
        uint32_t first = 0u;
        if (lane == 0) first = atomicAdd(&words[W_SLOT], (uint32_t)__popcll(takes));
        first = __shfl(first, 0);
        const uint32_t slot = first + (uint32_t)__popcll(takes & ((1ull << lane) - 1ull));
        if (take && slot < capacity) list[slot] = make_uint2((uint32_t)i, c);
    }
}
// table[root of the component of rank k] = k, from the list the host has put into canonical order (table: the zeroed count array)
__global__ __launch_bounds__(256) void k_rank_table(const uint2 *__restrict__ list, uint32_t listed, uint32_t *__restrict__ table) {
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < listed; k += gridDim.x * 256u) table[list[k].x] = k + 1u;
}
// L in place: a voxel's root becomes its rank
__global__ __launch_bounds__(256) void k_ranks(uint32_t *__restrict__ L, const uint32_t *__restrict__ table, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const uint32_t l = L[i];
        if (l) L[i] = table[l - 1u];
    }
}

// the label channel's second value, before k_pair clamps it to the largest code: the rank (vpt_volume_field.h)
struct RankChannel { __device__ __forceinline__ uint32_t operator()(uint32_t rank) const { return rank; } };

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// struct vpt_components: vpt_volume_components.h (vpt_volume_measure.hip reads the handle too)

// chase steps a unite / a voxel's flatten may take in one launch: CC_MERGE_STEPS and CC_FLATTEN_STEPS (vpt_volume_components.h) are what
// vpt_volume_components passes.
// The smallest caps for which the bounds of the host's loops (components_build) hold; vpt_volume_components_capped refuses smaller ones.
// Merge: on a flat forest a unite of two voxels that are not roots takes one step to the first root, confirms it, takes its second step to
// the other root and must still be below the cap to confirm that one: with fewer than 3 steps a launch without a hook could give up, and
// the argument that every launch which raises the word has hooked a root would not hold.
// Flatten: with one step a voxel ends at its grandparent or confirms its parent as the root, so depths at least halve and a flat forest
// raises nothing (flatten_launches below).
#define CC_MERGE_STEPS_MIN 3
#define CC_FLATTEN_STEPS_MIN 1
// Flatten launches the host makes at most behind one merge launch when a voxel may take `cap` steps; needing one more is an error.  A voxel at depth d starts at its
// parent (depth d - 1), and every load that does not confirm a root moves it at least one level up the forest as it was when the launch
// began (links written meanwhile by other threads name ancestors too).  So it confirms the root within d <= cap loads, and otherwise ends
// on a voxel that was at depth <= d - 1 - cap: by induction over the depth, a launch takes a depth d to at most ceil(d / (cap + 1)).  The
// forest is at most 2^32 deep (a link points to a smaller 32-bit index).  With j the first number of launches behind which
// ceil(2^32 / (cap + 1)^j) <= cap, launch j + 1 confirms every root within its steps and raises nothing; the limit is one more than
// that, j + 2.  64 steps: ceil(2^32 / 65^4) = 241, ceil(2^32 / 65^5) = 4, so j = 5 and the limit is 7; 1 step: j = 32, the limit is 34.
static int flatten_launches(int cap) {
    int j = 0;
    for (uint64_t p = 1; ((1ull << 32) + p - 1) / p > (uint64_t)cap; p *= (uint64_t)cap + 1u) j++;      // p < 2^32 (cap + 1) < 2^64
    return j + 2;
}

template <typename T>
static void launch_label_tiles(const vpt_components *c, const T *s, int conn, uint32_t lo, uint32_t hi, uint32_t *words) {
    const dim3 grid((unsigned)((c->nx + CC_TX - 1) / CC_TX), (unsigned)((c->ny + CC_TY - 1) / CC_TY), (unsigned)((c->nz + CC_TZ - 1) / CC_TZ));
    hipStream_t st = c->ctx->stream;
    if (conn == 6) hipLaunchKernelGGL((k_label_tiles<T, 6>), grid, dim3(256), 0, st, s, c->values.get(), c->nx, c->ny, c->nz, lo, hi, words);
    else if (conn == 18) hipLaunchKernelGGL((k_label_tiles<T, 18>), grid, dim3(256), 0, st, s, c->values.get(), c->nx, c->ny, c->nz, lo, hi, words);
    else hipLaunchKernelGGL((k_label_tiles<T, 26>), grid, dim3(256), 0, st, s, c->values.get(), c->nx, c->ny, c->nz, lo, hi, words);
}
void components_launch_merge(const vpt_components *c, int conn, int cap, uint32_t *words) {
    const size_t n = c->voxels();
    const dim3 grid(stream_grid(n));
    hipStream_t st = c->ctx->stream;
    if (conn == 6) hipLaunchKernelGGL(k_merge<6>, grid, dim3(256), 0, st, c->values.get(), c->nx, c->ny, c->nz, n, cap, words);
    else if (conn == 18) hipLaunchKernelGGL(k_merge<18>, grid, dim3(256), 0, st, c->values.get(), c->nx, c->ny, c->nz, n, cap, words);
    else hipLaunchKernelGGL(k_merge<26>, grid, dim3(256), 0, st, c->values.get(), c->nx, c->ny, c->nz, n, cap, words);
}

void components_launch_field_tiles(const vpt_components *c, const uint8_t *field, int conn, uint32_t lo, uint32_t hi, uint32_t *words) {
    launch_label_tiles<uint8_t>(c, field, conn, lo, hi, words);
}

// the body of vpt_volume_components and vpt_volume_watershed behind the argument checks (ComponentsPasses: vpt_volume_components.h); `c` is
// freed by the caller on failure
int components_build(vpt_components *c, uint32_t min_voxels, int merge_steps, int flatten_steps, const ComponentsPasses &passes) {
    const size_t n = c->voxels();
    hipStream_t st = c->ctx->stream;
    DevBuf<uint32_t> words, count;
    DevBuf<unsigned long long> sums;
    HIP_TRY(words.alloc(W_WORDS));
    HIP_TRY(sums.alloc(Q_WORDS));
    HIP_TRY(count.alloc(n));
    HIP_TRY(hipMemsetAsync(words, 0, W_WORDS * sizeof(uint32_t), st));
    HIP_TRY(hipMemsetAsync(sums, 0, Q_WORDS * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(count, 0, n * sizeof(uint32_t), st));
    HIP_TRY(hipStreamSynchronize(st));
    uint32_t host_words[W_WORDS] = {};
    PhaseClock clock(st);
    // ---- 1. tile labelling
    VPT_TRY(passes.tiles(words.get()));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_words, words, sizeof(host_words), hipMemcpyDeviceToHost, st));
    HIP_TRY(clock.lap_add(&c->ms[0]));
    // ---- 2., 3. merge and flatten until nothing gives up.
    // The bound of the loop.  Every merge launch begins with a flat forest (each voxel names its root: the flatten loop below ends that way,
    // and k_label_tiles leaves it so).  In a launch in which no hook succeeds the forest stays flat, every find ends within two loads and
    // every atomicMin meets a root, so no unite can give up: a merge launch that raises W_CHANGED has hooked at least one root under a
    // smaller one, for good (a root never becomes one again).  There are `tile_roots` roots when the loop begins (k_label_tiles counts
    // them), so at most tile_roots launches raise the word and launch tile_roots + 1 leaves it 0.  In practice the count is one launch per
    // merge_steps of chain that the tile components of one structure form (DESIGN.md has the measured counts).
    const int flatten_bound = flatten_launches(flatten_steps);
    const uint64_t merge_bound = (uint64_t)host_words[W_TILE_ROOTS] + 1u;
    const bool one_tile = c->nx <= CC_TX && c->ny <= CC_TY && c->nz <= CC_TZ;
    for (uint64_t round = 0; !one_tile; round++) {
        if (round == merge_bound) return fail(VPT_ERR_HIP, "%s: the merge did not settle within %llu launches", passes.what, (unsigned long long)merge_bound);
        HIP_TRY(hipMemsetAsync(words + W_CHANGED, 0, sizeof(uint32_t), st));
        passes.merge(merge_steps, words.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host_words, words, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(clock.lap_add(&c->ms[1]));
        c->launches[0]++;
        const bool merge_gave_up = host_words[W_CHANGED] != 0u;
        for (int f = 0; ; f++) {
            if (f == flatten_bound) return fail(VPT_ERR_HIP, "%s: the labels were not flat after %d launches", passes.what, flatten_bound);
            HIP_TRY(hipMemsetAsync(words + W_CHANGED, 0, sizeof(uint32_t), st));
            hipLaunchKernelGGL(k_flatten, dim3(stream_grid(n)), dim3(256), 0, st, c->values.get(), n, flatten_steps, words.get());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(host_words, words, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(clock.lap_add(&c->ms[2]));
            c->launches[1]++;
            if (host_words[W_CHANGED] == 0u) break;
        }
        if (!merge_gave_up) break;
    }
    // ---- 4. sizes
    hipLaunchKernelGGL(k_sizes, dim3(stream_grid(n)), dim3(256), 0, st, c->values.get(), n, count.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.lap_add(&c->ms[3]));
    // ---- 5. census, then the list of those that stay
    unsigned long long host_sums[Q_WORDS] = {};
    hipLaunchKernelGGL(k_census, dim3(stream_grid(n)), dim3(256), 0, st, c->values.get(), count.get(), n, min_voxels, sums.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_sums, sums, sizeof(host_sums), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    c->info.listed = host_sums[Q_LISTED]; c->info.dropped = host_sums[Q_DROPPED];
    c->info.foreground_voxels = host_sums[Q_FOREGROUND]; c->info.listed_voxels = host_sums[Q_LISTED_VOXELS];
    const uint32_t listed = (uint32_t)c->info.listed;                        // <= n < 2^32
    std::vector<uint2> pairs(listed);
    DevBuf<uint2> list;
    if (listed) {
        HIP_TRY(list.alloc(listed));
        hipLaunchKernelGGL(k_compact, dim3(stream_grid(n)), dim3(256), 0, st, c->values.get(), count.get(), n, min_voxels, list.get(), listed, words.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(pairs.data(), list, (size_t)listed * sizeof(uint2), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(clock.lap_add(&c->ms[4]));
    // ---- 6. the canonical order: voxels descending, then root ascending
    std::sort(pairs.begin(), pairs.end(), [](const uint2 &a, const uint2 &b) { return a.y != b.y ? a.y > b.y : a.x < b.x; });
    c->list.resize(listed);
    for (uint32_t k = 0; k < listed; k++) {
        const uint32_t i = pairs[k].x;
        c->list[k] = vpt_component{ i % (uint32_t)c->nx, (i / (uint32_t)c->nx) % (uint32_t)c->ny, i / ((uint32_t)c->nx * (uint32_t)c->ny), pairs[k].y };
    }
    HIP_TRY(clock.lap_add(&c->ms[5]));
    // ---- the rank table in the count array, then L in place
    HIP_TRY(hipMemsetAsync(count, 0, n * sizeof(uint32_t), st));
    if (listed) {
        HIP_TRY(hipMemcpyAsync(list, pairs.data(), (size_t)listed * sizeof(uint2), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_rank_table, dim3(stream_grid(listed)), dim3(256), 0, st, list.get(), listed, count.get());
    }
    hipLaunchKernelGGL(k_ranks, dim3(stream_grid(n)), dim3(256), 0, st, c->values.get(), count.get(), n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.lap_add(&c->ms[6]));          // `pairs`, `list` and `count` go out of scope behind their last use
    return VPT_OK;
}

// vpt_volume_components and vpt_volume_components_capped behind the check of the caps
static int components_create(vpt_volume *src, uint32_t lo, uint32_t hi, int connectivity, uint32_t min_voxels, int merge_steps, int flatten_steps,
                             vpt_components **out) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (src->format != VPT_FORMAT_R8 && src->format != VPT_FORMAT_R16)
        return fail(VPT_ERR_UNSUPPORTED, "connected components are taken of one-channel unsigned normalised volumes (R8, R16; the window makes one of any scalar volume), not of %s",
                    format_name(src->format));
    const uint32_t M = src->norm16 ? 65535u : 255u;
    if (lo > hi) return fail(VPT_ERR_INVALID, "component range [%u, %u]: lo exceeds hi", lo, hi);
    if (hi > M) return fail(VPT_ERR_INVALID, "component range [%u, %u]: the largest code of %s is %u", lo, hi, format_name(src->format), M);
    if (connectivity != 6 && connectivity != 18 && connectivity != 26) return fail(VPT_ERR_INVALID, "connectivity %d: 6, 18 or 26 are taken", connectivity);
    if (min_voxels < 1u) return fail(VPT_ERR_INVALID, "min_voxels 0: a component has at least one voxel");
    const uint64_t n = (uint64_t)src->nx * (uint64_t)src->ny * (uint64_t)src->nz;
    if (n > 0xFFFFFFFEull) return fail(VPT_ERR_UNSUPPORTED, "connected components: %llu voxels exceed 2^32 - 2 (labels and counts are 32-bit)", (unsigned long long)n);
    vpt_context *ctx = src->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    if ((src->ny + CC_TY - 1) / CC_TY > 65535 || (src->nz + CC_TZ - 1) / CC_TZ > 65535) return fail(VPT_ERR_UNSUPPORTED, "volume too large");
    std::unique_ptr<vpt_components> c(new vpt_components());
    VPT_TRY(field_capture(c.get(), src));
    vpt_components *h = c.get();
    const ComponentsPasses passes = {
        "connected components",
        [=](uint32_t *words) {
            if (h->norm16) launch_label_tiles<uint16_t>(h, (const uint16_t *)h->texels.get(), connectivity, lo, hi, words);
            else launch_label_tiles<uint8_t>(h, (const uint8_t *)h->texels.get(), connectivity, lo, hi, words);
            return (int)VPT_OK;
        },
        [=](int cap, uint32_t *words) { components_launch_merge(h, connectivity, cap, words); } };
    const int rc = components_build(h, min_voxels, merge_steps, flatten_steps, passes);
    if (rc != VPT_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }      // the buffers are freed on return: nothing may still use them
    *out = c.release();
    return VPT_OK;
}

int components_check_caps(int merge_steps, int flatten_steps) {
    if (merge_steps < CC_MERGE_STEPS_MIN)
        return fail(VPT_ERR_INVALID, "merge_steps %d: at least %d are needed for the merge loop's bound to hold", merge_steps, CC_MERGE_STEPS_MIN);
    if (flatten_steps < CC_FLATTEN_STEPS_MIN)
        return fail(VPT_ERR_INVALID, "flatten_steps %d: at least %d is needed for the flatten loop's bound to hold", flatten_steps, CC_FLATTEN_STEPS_MIN);
    return VPT_OK;
}

extern "C" int vpt_volume_components(vpt_volume *src, uint32_t lo, uint32_t hi, int connectivity, uint32_t min_voxels, vpt_components **out) {
    return components_create(src, lo, hi, connectivity, min_voxels, CC_MERGE_STEPS, CC_FLATTEN_STEPS, out);
}

// (for tests) the caps are checked first: a refused cap touches neither the other arguments nor the device
extern "C" int vpt_volume_components_capped(vpt_volume *src, uint32_t lo, uint32_t hi, int connectivity, uint32_t min_voxels, int merge_steps,
                                            int flatten_steps, vpt_components **out) {
    VPT_TRY(components_check_caps(merge_steps, flatten_steps));
    return components_create(src, lo, hi, connectivity, min_voxels, merge_steps, flatten_steps, out);
}

extern "C" int vpt_components_info(vpt_components *c, struct vpt_components_info *info) {
    if (!c || !info) return fail(VPT_ERR_INVALID, "null argument");
    *info = c->info;
    return VPT_OK;
}

extern "C" int vpt_components_list(vpt_components *c, uint64_t first, uint64_t n, struct vpt_component *dst) {
    if (!c || (!dst && n)) return fail(VPT_ERR_INVALID, "null argument");
    if (first > c->info.listed || n > c->info.listed - first)
        return fail(VPT_ERR_INVALID, "components %llu .. +%llu are not within the %llu listed", (unsigned long long)first, (unsigned long long)n, (unsigned long long)c->info.listed);
    if (n) memcpy(dst, c->list.data() + first, (size_t)n * sizeof(vpt_component));
    return VPT_OK;
}

extern "C" int vpt_components_ranks(vpt_components *c, int x, int y, int z, int w, int h, int d, uint32_t *host_dst, size_t nbytes) {
    return field_read(c, x, y, z, w, h, d, host_dst, nbytes);
}

extern "C" int vpt_components_keep(vpt_components *c, uint64_t first_rank, uint64_t last_rank, uint32_t fill, vpt_volume **out) {
    if (!c || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (first_rank < 1 || first_rank > last_rank)
        return fail(VPT_ERR_INVALID, "ranks %llu .. %llu: 1 <= first <= last is required", (unsigned long long)first_rank, (unsigned long long)last_rank);
    // ranks are 32-bit: a first rank beyond them keeps nothing (the empty range 1 .. 0), a last rank beyond them is their largest
    const uint32_t first = first_rank > 0xFFFFFFFFull ? 1u : (uint32_t)first_rank;
    const uint32_t last = first_rank > 0xFFFFFFFFull ? 0u : (uint32_t)std::min<uint64_t>(last_rank, 0xFFFFFFFFull);
    return field_select(c, first, last, fill, out);
}

extern "C" int vpt_components_label(vpt_components *c, vpt_volume **out) {
    if (!c || !out) return fail(VPT_ERR_INVALID, "null argument");
    return field_pair(c, RankChannel(), out);
}

extern "C" int vpt_components_profile(vpt_components *c, double *ms, uint32_t *launches) {
    if (!c) return fail(VPT_ERR_INVALID, "null argument");
    if (ms) memcpy(ms, c->ms, sizeof(c->ms));
    if (launches) memcpy(launches, c->launches, sizeof(c->launches));
    return VPT_OK;
}

extern "C" int vpt_components_destroy(vpt_components *c) { return field_destroy(c); }
