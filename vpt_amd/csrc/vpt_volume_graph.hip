// vpt_volume_graph.hip — the graph of a voxel set on the device (vpt_volume_graph, vpt_skeleton_graph and the vpt_graph_* family): the class of
// every voxel of the set, its branches and nodes as two labellings, one record per branch and node, and the two emitters (prune, classes).
// C-ABI and the contract: include/vpt.h; why a branch is a path or a cycle, compiler figures and measurements: DESIGN.md "Skeleton graph".
//
//   1. the set as a bit plane X, 32 voxels along x a word, rows padded to whole 64-voxel segments (the thinning unit's layout)   k_gr_seed
//   2. the kept voxels per block of 256 words, their exclusive prefix sums (one workgroup), then the class of every kept voxel and the
//      list of kept voxels in linear-index order, placed by offset + popcount                       k_gr_block_sums, k_gr_scan_blocks, k_gr_classify
//   3. classes 1 .. 3 and class 4 labelled at 26-connectivity by the components' tile pass, merge and tail (components_build)
//   4. one thread a listed branch voxel: its 26 neighbours' classes and ranks become the branch's record and the nodes' degrees; runs of one
//      branch along a wave are summed in registers before the atomics (integer add / min / max: any order gives the same bytes)    k_gr_links
//   5. the emitters, four voxels a thread (Four<T>)                                                    k_gr_prune, k_gr_classes
// No workgroup waits for another: launch boundaries order the phases.
#include "vpt_volume_graph.h"

#define GR_MAX_AXIS 4096            // the thinning unit's limit
#define GR_NONE32 0xFFFFFFFFu
#define GR_NONE64 0xFFFFFFFFFFFFFFFFull

// ---------------------------------------------------------------------------------------------
// seed: the set as a bit plane
// ---------------------------------------------------------------------------------------------
template <typename T> struct GrInRange {        // the codes lo .. hi of a volume's texels
    const T *src; uint32_t lo, hi;
    __device__ __forceinline__ bool operator()(size_t i) const { const uint32_t c = (uint32_t)src[i]; return c >= lo && c <= hi; }
};
struct GrKept {                                 // the kept voxels of a skeleton's burn passes
    const uint32_t *burn;
    __device__ __forceinline__ bool operator()(size_t i) const { return burn[i] == VPT_THIN_KEPT; }
};
// A wave owns 64 voxels of a row: one ballot is two words of the plane.  Bits beyond nx stay 0.
template <typename In>
__global__ __launch_bounds__(256) void k_gr_seed(In in, uint32_t *__restrict__ plane, int nx, int tnx, size_t rows) {
    const int lane = (int)threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (size_t)gridDim.x * 4, items = rows * (size_t)tnx;
    for (size_t item = wave; item < items; item += waves) {
        const size_t row = item / (size_t)tnx; const int seg = (int)(item % (size_t)tnx);
        const int x = seg * 64 + lane;
        const bool kept = x < nx && in(row * (size_t)nx + (size_t)x);
        const unsigned long long b = __ballot(kept);
        if (lane < 2) plane[row * (size_t)(2 * tnx) + (size_t)(2 * seg + lane)] = (uint32_t)(b >> (32 * lane));
    }
}

// a word of the plane, 0 outside the volume
__device__ __forceinline__ uint32_t gr_word(const uint32_t *__restrict__ plane, int ny, int nz, int wpr, int z, int y, int wx) {
    if (z < 0 || z >= nz || y < 0 || y >= ny || wx < 0 || wx >= wpr) return 0u;
    return plane[((size_t)z * (size_t)ny + (size_t)y) * (size_t)wpr + (size_t)wx];
}

// ---------------------------------------------------------------------------------------------
// where the kept voxels go in the list: counts per block of 256 words, their exclusive prefix sums
// ---------------------------------------------------------------------------------------------
// the inclusive scan of one value a thread over a workgroup of 256 (Hillis-Steele in LDS)
template <typename V>
__device__ __forceinline__ V gr_scan_256(V v, V *lds) {
    const int tid = (int)threadIdx.x;
    lds[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = 1; o < 256; o <<= 1) {
        const V t = tid >= o ? lds[tid - o] : (V)0;
        __syncthreads();
        lds[tid] += t;
        __syncthreads();
    }
    return lds[tid];
}
// sums[b]: the kept voxels of the words 256 b .. 256 b + 255
__global__ __launch_bounds__(256) void k_gr_block_sums(const uint32_t *__restrict__ X, size_t plane_words, uint32_t *__restrict__ sums) {
    __shared__ uint32_t part[4];
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t c = w < plane_words ? (uint32_t)__popc(X[w]) : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
    if (((int)threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) sums[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}
// one workgroup: the block sums become their exclusive prefix sums, *total the sum of all (< 2^32: a volume has at most 2^32 - 2 voxels).
// A thread owns a run of the sums.
__global__ __launch_bounds__(256) void k_gr_scan_blocks(uint32_t *__restrict__ sums, size_t blocks, unsigned long long *__restrict__ total) {
    __shared__ unsigned long long lds[256];
    const size_t run = (blocks + 255) / 256, b0 = (size_t)threadIdx.x * run, b1 = b0 + run < blocks ? b0 + run : blocks;
    unsigned long long mine = 0ull;
    for (size_t b = b0; b < b1; b++) mine += sums[b];
    const unsigned long long incl = gr_scan_256(mine, lds);
    unsigned long long at = incl - mine;
    for (size_t b = b0; b < b1; b++) { const uint32_t v = sums[b]; sums[b] = (uint32_t)at; at += v; }
    if (threadIdx.x == 255) *total = incl;
}

// ---------------------------------------------------------------------------------------------
// classes and the kept-voxel list, k_gr_classify
// ---------------------------------------------------------------------------------------------
// A thread a word of X; a word without a kept voxel (nearly all of them) costs its one load, and a block without one leaves after the
// vote.  Otherwise the nine rows around the word come as three words each, folded into a 34-bit window whose bit j + 1 is voxel j of the
// word, and every kept voxel counts its kept 26-neighbours.  The voxel's place in the list is the block's offset, plus the kept voxels of
// the block's words in front of this one (a scan in LDS), plus the kept voxels of this word below it: linear-index order, whatever the
// schedule.
__global__ __launch_bounds__(256) void k_gr_classify(const uint32_t *__restrict__ X, const uint32_t *__restrict__ offsets, uint8_t *__restrict__ classes,
                                                     uint32_t *__restrict__ list, int nx, int ny, int nz, int wpr, size_t plane_words) {
    __shared__ uint32_t lds[256];
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t c = w < plane_words ? X[w] : 0u;
    if (!__syncthreads_or(c != 0u ? 1 : 0)) return;             // (uniform)
    const uint32_t mine = (uint32_t)__popc(c);
    uint32_t at = offsets[blockIdx.x] + gr_scan_256(mine, lds) - mine;
    if (c == 0u) return;
    const int wx = (int)(w % (size_t)wpr); const size_t r = w / (size_t)wpr; const int y = (int)(r % (size_t)ny), z = (int)(r / (size_t)ny);
    unsigned long long win[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int zz = z + k / 3 - 1, yy = y + k % 3 - 1;
        win[k] = (unsigned long long)(gr_word(X, ny, nz, wpr, zz, yy, wx - 1) >> 31) | ((unsigned long long)gr_word(X, ny, nz, wpr, zz, yy, wx) << 1) |
                 ((unsigned long long)(gr_word(X, ny, nz, wpr, zz, yy, wx + 1) & 1u) << 33);
    }
    const size_t row = ((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)wx * 32;
    while (c) {
        const int b = __ffs((int)c) - 1;
        c &= c - 1u;
        int n = -1;                                             // the voxel itself is in its window
#pragma unroll
        for (int k = 0; k < 9; k++) n += __popc((uint32_t)(win[k] >> b) & 7u);
        const size_t i = row + (size_t)b;                       // wx 32 + b < nx: the seed leaves the bits beyond nx clear
        classes[i] = (uint8_t)(1 + min(n, 3));
        list[at++] = (uint32_t)i;
    }
}

// ---------------------------------------------------------------------------------------------
// links: the branch records and the nodes' degrees, k_gr_links
// ---------------------------------------------------------------------------------------------
// the records before the links pass: the identities of sum, min and max
__global__ __launch_bounds__(256) void k_gr_init(vpt_graph_branch *__restrict__ rec, uint32_t branches) {
    for (uint32_t k = blockIdx.x * 256u + threadIdx.x; k < branches; k += gridDim.x * 256u) {
        vpt_graph_branch b = {};
        b.node_lo = GR_NONE32; b.tip_lo = GR_NONE64;
        rec[k] = b;
    }
}
// A lane takes one listed voxel; a node voxel has nothing to add (its key is 0).  A branch voxel walks its 26 neighbours: a branch
// neighbour is of its own branch (adjacent branch voxels are connected) and the pair is counted at its voxel of larger index; a node
// neighbour is an attachment, which counts as a step, names a node rank and adds one to that node's degree (an atomic of its own: a branch
// voxel has at most two neighbours, and those of one node seldom sit in one wave).  The list is in linear-index order, so the voxels of a
// branch that runs along x sit in neighbouring lanes: a run of equal keys is summed towards its first lane (the counts packed in bytes:
// a lane adds at most 2 to each, a wave at most 128), and only that lane touches the record.
__global__ __launch_bounds__(256) void k_gr_links(const uint32_t *__restrict__ list, uint32_t kept, const uint8_t *__restrict__ classes, const uint32_t *__restrict__ brank,
                                                  const uint32_t *__restrict__ nrank, int nx, int ny, int nz, vpt_graph_branch *__restrict__ rec, uint32_t branches,
                                                  unsigned long long *__restrict__ degree, uint32_t nodes) {
    const int lane = (int)threadIdx.x & 63;
    for (uint32_t base = blockIdx.x * 256u + (threadIdx.x & ~63u); base < kept; base += gridDim.x * 256u) {      // (wave-uniform; graph_build keeps kept + the stride below 2^32)
        const uint32_t t = base + (uint32_t)lane;
        uint32_t key = 0u, counts = 0u, steps = 0u, nlo = GR_NONE32, nhi = 0u, tlo = GR_NONE32, thi = 0u;       // counts: voxels | free ends << 8 | attachments << 16
        if (t < kept) {
            const uint32_t i = list[t];
            const uint32_t cls = classes[i];
            if (cls >= 1u && cls <= 3u) {
                key = brank[i];
                const int x = (int)(i % (uint32_t)nx), y = (int)((i / (uint32_t)nx) % (uint32_t)ny), z = (int)(i / ((uint32_t)nx * (uint32_t)ny));
                counts = 1u | (cls == 2u ? 1u << 8 : 0u);
                int own = 0;
#pragma unroll
                for (int dz = -1; dz <= 1; dz++)
#pragma unroll
                    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                        for (int dx = -1; dx <= 1; dx++) {
                            if (dx == 0 && dy == 0 && dz == 0) continue;
                            const int xx = x + dx, yy = y + dy, zz = z + dz;
                            if (xx < 0 || xx >= nx || yy < 0 || yy >= ny || zz < 0 || zz >= nz) continue;
                            const uint32_t j = (uint32_t)(((size_t)zz * (size_t)ny + (size_t)yy) * (size_t)nx + (size_t)xx);
                            const uint32_t c = classes[j];
                            if (c == 0u) continue;
                            const uint32_t step = 1u << (8 * ((dx != 0) + (dy != 0) + (dz != 0) - 1));
                            if (c <= 3u) {
                                own++;
                                if (j < i) steps += step;
                            } else {
                                const uint32_t r = nrank[j];
                                counts += 1u << 16;
                                steps += step;
                                nlo = min(nlo, r); nhi = max(nhi, r);
                                if (r >= 1u && r <= nodes) atomicAdd(&degree[r - 1u], 1ull);
                            }
                        }
                if (own < 2) { tlo = i; thi = i + 1u; }           // thi: index + 1, 0: no tip
            }
        }
        // runs of one key
        const uint32_t before = (uint32_t)__shfl_up((int)key, 1);
        const bool head = lane == 0 || key != before;
        const unsigned long long heads = __ballot(head);
        const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);
        const int run_end = rest ? lane + __ffsll((long long)rest) - 1 : 63;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t a = (uint32_t)__shfl_down((int)counts, o), s = (uint32_t)__shfl_down((int)steps, o), l = (uint32_t)__shfl_down((int)nlo, o),
                           h = (uint32_t)__shfl_down((int)nhi, o), tl = (uint32_t)__shfl_down((int)tlo, o), th = (uint32_t)__shfl_down((int)thi, o);
            if (lane + o <= run_end) { counts += a; steps += s; nlo = min(nlo, l); nhi = max(nhi, h); tlo = min(tlo, tl); thi = max(thi, th); }
        }
        if (head && key >= 1u && key <= branches) {
            vpt_graph_branch *b = rec + (key - 1u);
            atomicAdd(&b->voxels, counts & 255u);
            if ((counts >> 8) & 255u) atomicAdd(&b->free_ends, (counts >> 8) & 255u);
            if (counts >> 16) {
                atomicAdd(&b->attachments, counts >> 16);
                atomicMin(&b->node_lo, nlo);
                atomicMax(&b->node_hi, nhi);
            }
            if (steps & 255u) atomicAdd((unsigned long long *)&b->steps_face, (unsigned long long)(steps & 255u));
            if ((steps >> 8) & 255u) atomicAdd((unsigned long long *)&b->steps_edge, (unsigned long long)((steps >> 8) & 255u));
            if (steps >> 16) atomicAdd((unsigned long long *)&b->steps_corner, (unsigned long long)(steps >> 16));
            if (thi) {
                atomicMin((unsigned long long *)&b->tip_lo, (unsigned long long)tlo);
                atomicMax((unsigned long long *)&b->tip_hi, (unsigned long long)(thi - 1u));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// the emitters: k_gr_prune, k_gr_classes
// ---------------------------------------------------------------------------------------------
// the source's code where the voxel is kept and its branch is not in the drop bitmap (bit rank - 1), `fill` elsewhere
template <typename T>
__global__ __launch_bounds__(256) void k_gr_prune(const T *__restrict__ src, const uint8_t *__restrict__ classes, const uint32_t *__restrict__ brank,
                                                  const uint32_t *__restrict__ drop, T *__restrict__ dst, size_t n, uint32_t fill) {
    typedef Four<T> F;
    const size_t quads = n / 4, stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t q = t0; q < quads; q += stride) {
        const uint32_t cw = reinterpret_cast<const uint32_t *>(classes)[q];
        uint32_t v[4] = { fill, fill, fill, fill };
        if (cw != 0u) {
            const typename F::in_t w = reinterpret_cast<const typename F::in_t *>(src)[q];
            const uint4 r4 = reinterpret_cast<const uint4 *>(brank)[q];
            const uint32_t r[4] = { r4.x, r4.y, r4.z, r4.w };
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t c = (cw >> (8 * i)) & 255u;
                const bool gone = c == 0u || (c <= 3u && r[i] != 0u && ((drop[(r[i] - 1u) >> 5] >> ((r[i] - 1u) & 31u)) & 1u));
                if (!gone) v[i] = F::get(w, i);
            }
        }
        reinterpret_cast<typename F::in_t *>(dst)[q] = F::pack(v);
    }
    for (size_t i = quads * 4 + t0; i < n; i += stride) {
        const uint32_t c = classes[i], r = brank[i];
        const bool gone = c == 0u || (c <= 3u && r != 0u && ((drop[(r - 1u) >> 5] >> ((r - 1u) & 31u)) & 1u));
        dst[i] = gone ? (T)fill : src[i];
    }
}
// (code, class)
template <typename T>
__global__ __launch_bounds__(256) void k_gr_classes(const T *__restrict__ src, const uint8_t *__restrict__ classes, T *__restrict__ dst, size_t n) {
    typedef Four<T> F;
    const size_t quads = n / 4, stride = (size_t)gridDim.x * 256, t0 = (size_t)blockIdx.x * 256 + threadIdx.x;
    for (size_t q = t0; q < quads; q += stride) {
        const typename F::in_t w = reinterpret_cast<const typename F::in_t *>(src)[q];
        const uint32_t cw = reinterpret_cast<const uint32_t *>(classes)[q];
        uint32_t v[4], g[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { v[i] = F::get(w, i); g[i] = (cw >> (8 * i)) & 255u; }
        reinterpret_cast<typename F::pair_t *>(dst)[q] = F::pack2(v, g);
    }
    for (size_t i = quads * 4 + t0; i < n; i += stride) { dst[2 * i] = src[i]; dst[2 * i + 1] = (T)classes[i]; }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static uint32_t graph_kind(const vpt_graph_branch &b) {
    if (b.free_ends == 2u) return VPT_GRAPH_SEGMENT;
    if (b.free_ends == 1u && b.attachments == 1u) return VPT_GRAPH_SPUR;
    if (b.attachments == 2u) return b.node_lo != b.node_hi ? VPT_GRAPH_LINK : VPT_GRAPH_LOOP;
    return b.voxels == 1u ? VPT_GRAPH_ISOLATED : VPT_GRAPH_CYCLE;
}

// one of the two labellings: the voxels of class lo .. hi, 26-connected, every component listed
static int graph_label(vpt_graph *g, vpt_components *c, uint32_t lo, uint32_t hi, const char *what) {
    const uint8_t *classes = g->classes.get();
    const ComponentsPasses passes = {
        what,
        [=](uint32_t *words) { components_launch_field_tiles(c, classes, 26, lo, hi, words); return (int)VPT_OK; },
        [=](int cap, uint32_t *words) { components_launch_merge(c, 26, cap, words); } };
    return components_build(c, 1u, CC_MERGE_STEPS, CC_FLATTEN_STEPS, passes);
}

// the body of vpt_volume_graph and vpt_skeleton_graph behind the argument checks: both labellings hold their texel snapshot, `seed` enqueues
// the launch that fills the plane; `g` is freed by the caller on failure
template <typename Seed>
static int graph_build(vpt_graph *g, Seed seed) {
    const vpt_components *f = g->branches.get();
    hipStream_t st = g->ctx->stream;
    const int nx = f->nx, ny = f->ny, nz = f->nz;
    const int tnx = (nx + 63) / 64, wpr = 2 * tnx;
    const size_t n = f->voxels(), rows = (size_t)ny * (size_t)nz, plane_words = rows * (size_t)wpr, blocks = (plane_words + 255) / 256;      // blocks <= 2^23
    DevBuf<uint32_t> X, offsets, list;
    DevBuf<unsigned long long> total;
    HIP_TRY(X.alloc(plane_words));
    HIP_TRY(offsets.alloc(blocks));
    HIP_TRY(total.alloc(1));
    HIP_TRY(g->classes.alloc((n + 3) / 4 * 4));
    HIP_TRY(hipMemsetAsync(g->classes, 0, (n + 3) / 4 * 4, st));
    HIP_TRY(hipStreamSynchronize(st));                          // what is in front of the call is not its time
    PhaseClock clock(st);
    // ---- 1. seed
    seed(X.get(), nx, tnx, rows, dim3(stream_grid(rows * (size_t)tnx, 4)));
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.lap(&g->ms[0]));
    // ---- 2. counts, prefix sums, classes and the list
    unsigned long long kept = 0ull;
    hipLaunchKernelGGL(k_gr_block_sums, dim3((unsigned)blocks), dim3(256), 0, st, (const uint32_t *)X.get(), plane_words, offsets.get());
    hipLaunchKernelGGL(k_gr_scan_blocks, dim3(1), dim3(256), 0, st, offsets.get(), blocks, total.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&kept, total, sizeof(kept), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    g->launches = 3;
    if (kept > n) return fail(VPT_ERR_HIP, "graph: %llu kept voxels counted in %zu", kept, n);
    if (kept) {
        HIP_TRY(list.alloc((size_t)kept));
        hipLaunchKernelGGL(k_gr_classify, dim3((unsigned)blocks), dim3(256), 0, st, (const uint32_t *)X.get(), (const uint32_t *)offsets.get(), g->classes.get(), list.get(),
                           nx, ny, nz, wpr, plane_words);
        HIP_TRY(hipGetLastError());
        g->launches++;
    }
    HIP_TRY(clock.lap(&g->ms[1]));
    // ---- 3. the two labellings (the dense route: each is a whole components run over the class field)
    VPT_TRY(graph_label(g, g->branches.get(), 1u, 3u, "graph branches"));
    HIP_TRY(clock.lap(&g->ms[2]));
    VPT_TRY(graph_label(g, g->nodes.get(), 4u, 4u, "graph nodes"));
    HIP_TRY(clock.lap(&g->ms[3]));
    // ---- 4. links
    const uint32_t branches = (uint32_t)g->branches->info.listed, nodes = (uint32_t)g->nodes->info.listed;
    g->branch.assign(branches, vpt_graph_branch{});
    g->node.assign(nodes, vpt_graph_node{});
    std::vector<unsigned long long> degree(nodes, 0ull);
    if (branches) {
        DevBuf<vpt_graph_branch> rec;
        DevBuf<unsigned long long> deg;
        HIP_TRY(rec.alloc(branches));
        HIP_TRY(deg.alloc(std::max<size_t>(nodes, 1)));
        HIP_TRY(hipMemsetAsync(deg, 0, std::max<size_t>(nodes, 1) * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(k_gr_init, dim3(stream_grid(branches)), dim3(256), 0, st, rec.get(), branches);
        // the wave-uniform loop of k_gr_links adds the grid's stride (at most 2^21) to a 32-bit index below `kept`
        if (kept > 0xFFFFFFFFull - (8192ull * 256ull)) return fail(VPT_ERR_UNSUPPORTED, "graph: %llu kept voxels", kept);
        hipLaunchKernelGGL(k_gr_links, dim3(stream_grid((size_t)kept)), dim3(256), 0, st, (const uint32_t *)list.get(), (uint32_t)kept, (const uint8_t *)g->classes.get(),
                           (const uint32_t *)g->branches->values.get(), (const uint32_t *)g->nodes->values.get(), nx, ny, nz, rec.get(), branches, deg.get(), nodes);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(g->branch.data(), rec, (size_t)branches * sizeof(vpt_graph_branch), hipMemcpyDeviceToHost, st));
        if (nodes) HIP_TRY(hipMemcpyAsync(degree.data(), deg, (size_t)nodes * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));                      // `rec` and `deg` go out of scope behind their last use
        g->launches += 2;
    }
    HIP_TRY(clock.lap(&g->ms[4]));
    // ---- 5. what the host derives: absent nodes and tips, kinds, totals
    struct vpt_graph_info &info = g->info;
    info.kept_voxels = kept; info.branches = branches; info.nodes = nodes;
    for (uint32_t k = 0; k < branches; k++) {
        vpt_graph_branch &b = g->branch[k];
        const vpt_component &c = g->branches->list[k];
        if (b.node_lo == GR_NONE32) b.node_lo = 0u;
        if (b.tip_lo == GR_NONE64) b.tip_lo = b.tip_hi = ((uint64_t)c.root_z * (uint64_t)ny + (uint64_t)c.root_y) * (uint64_t)nx + (uint64_t)c.root_x;      // a cycle: its root
        b.kind = graph_kind(b);
        switch (b.kind) {
            case VPT_GRAPH_ISOLATED: info.isolated++; break;
            case VPT_GRAPH_SEGMENT: info.segments++; break;
            case VPT_GRAPH_SPUR: info.spurs++; break;
            case VPT_GRAPH_LINK: info.links++; break;
            case VPT_GRAPH_LOOP: info.loops++; break;
            default: info.cycles++; break;
        }
        info.steps_face += b.steps_face; info.steps_edge += b.steps_edge; info.steps_corner += b.steps_corner; info.attachments += b.attachments;
    }
    for (uint32_t k = 0; k < nodes; k++) {
        g->node[k].voxels = g->nodes->list[k].voxels; g->node[k].degree = degree[k];
        info.node_voxels += g->node[k].voxels;
    }
    HIP_TRY(clock.lap(&g->ms[5]));
    return VPT_OK;
}

// a labelling handle with `like`'s geometry and a copy of `texels` (device; one channel of `like`'s width) enqueued on the stream
static int graph_snapshot(vpt_components *c, const VoxelField *like, const uint8_t *texels) {
    c->ctx = like->ctx; c->nx = like->nx; c->ny = like->ny; c->nz = like->nz; c->format = like->format; c->filter = like->filter; c->norm16 = like->norm16;
    const size_t n = c->voxels(), bytes = n * (size_t)(c->norm16 ? 2 : 1);
    HIP_TRY(c->texels.alloc(bytes));
    HIP_TRY(c->values.alloc(n));
    HIP_TRY(hipMemcpyAsync(c->texels, texels, bytes, hipMemcpyDeviceToDevice, c->ctx->stream));
    return VPT_OK;
}

static int graph_check_size(int nx, int ny, int nz) {
    const uint64_t n = (uint64_t)nx * (uint64_t)ny * (uint64_t)nz;
    if (n > 0xFFFFFFFEull) return fail(VPT_ERR_UNSUPPORTED, "graph: %llu voxels exceed 2^32 - 2 (labels and counts are 32-bit)", (unsigned long long)n);
    if (nx > GR_MAX_AXIS || ny > GR_MAX_AXIS || nz > GR_MAX_AXIS) return fail(VPT_ERR_UNSUPPORTED, "graph: volume too large (at most %d voxels an axis)", GR_MAX_AXIS);
    return VPT_OK;
}

extern "C" int vpt_volume_graph(vpt_volume *src, uint32_t lo, uint32_t hi, vpt_graph **out) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (src->format != VPT_FORMAT_R8 && src->format != VPT_FORMAT_R16)
        return fail(VPT_ERR_UNSUPPORTED, "graphs are taken of one-channel unsigned normalised volumes (R8, R16; the window makes one of any scalar volume), not of %s",
                    format_name(src->format));
    const uint32_t M = src->norm16 ? 65535u : 255u;
    if (lo > hi) return fail(VPT_ERR_INVALID, "graph range [%u, %u]: lo exceeds hi", lo, hi);
    if (hi > M) return fail(VPT_ERR_INVALID, "graph range [%u, %u]: the largest code of %s is %u", lo, hi, format_name(src->format), M);
    VPT_TRY(graph_check_size(src->nx, src->ny, src->nz));
    vpt_context *ctx = src->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<vpt_graph> g(new vpt_graph());
    g->ctx = ctx;
    g->branches.reset(new vpt_components());
    g->nodes.reset(new vpt_components());
    int rc = field_capture(g->branches.get(), src);             // the source's codes, behind any upload into src
    if (rc == VPT_OK) rc = graph_snapshot(g->nodes.get(), g->branches.get(), g->branches->texels.get());
    if (rc == VPT_OK) {
        const vpt_components *b = g->branches.get();
        hipStream_t st = ctx->stream;
        rc = graph_build(g.get(), [=](uint32_t *X, int nx, int tnx, size_t rows, dim3 grid) {
            GrInRange<uint16_t> wide; wide.src = (const uint16_t *)b->texels.get(); wide.lo = lo; wide.hi = hi;
            GrInRange<uint8_t> bytes; bytes.src = (const uint8_t *)b->texels.get(); bytes.lo = lo; bytes.hi = hi;
            if (b->norm16) hipLaunchKernelGGL(k_gr_seed<GrInRange<uint16_t>>, grid, dim3(256), 0, st, wide, X, nx, tnx, rows);
            else hipLaunchKernelGGL(k_gr_seed<GrInRange<uint8_t>>, grid, dim3(256), 0, st, bytes, X, nx, tnx, rows);
        });
    }
    if (rc != VPT_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }      // the buffers are freed on return: nothing may still use them
    *out = g.release();
    return VPT_OK;
}

extern "C" int vpt_skeleton_graph(vpt_skeleton *sk, vpt_graph **out) {
    if (!sk || !out) return fail(VPT_ERR_INVALID, "null argument");
    VPT_TRY(graph_check_size(sk->nx, sk->ny, sk->nz));
    vpt_context *ctx = sk->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<vpt_graph> g(new vpt_graph());
    g->ctx = ctx;
    g->branches.reset(new vpt_components());
    g->nodes.reset(new vpt_components());
    int rc = graph_snapshot(g->branches.get(), sk, sk->texels.get());      // the skeleton's own snapshot of its source
    if (rc == VPT_OK) rc = graph_snapshot(g->nodes.get(), sk, sk->texels.get());
    if (rc == VPT_OK) {
        const uint32_t *burn = sk->values.get();
        hipStream_t st = ctx->stream;
        rc = graph_build(g.get(), [=](uint32_t *X, int nx, int tnx, size_t rows, dim3 grid) {
            GrKept kept; kept.burn = burn;
            hipLaunchKernelGGL(k_gr_seed<GrKept>, grid, dim3(256), 0, st, kept, X, nx, tnx, rows);
        });
    }
    if (rc != VPT_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    *out = g.release();
    return VPT_OK;
}

extern "C" int vpt_graph_info(vpt_graph *g, struct vpt_graph_info *info) {
    if (!g || !info) return fail(VPT_ERR_INVALID, "null argument");
    *info = g->info;
    return VPT_OK;
}

extern "C" int vpt_graph_branches(vpt_graph *g, uint64_t first, uint64_t n, struct vpt_graph_branch *dst) {
    if (!g || (!dst && n)) return fail(VPT_ERR_INVALID, "null argument");
    if (first > g->info.branches || n > g->info.branches - first)
        return fail(VPT_ERR_INVALID, "branches %llu .. +%llu are not within the %llu of the graph", (unsigned long long)first, (unsigned long long)n, (unsigned long long)g->info.branches);
    if (n) memcpy(dst, g->branch.data() + first, (size_t)n * sizeof(vpt_graph_branch));
    return VPT_OK;
}

extern "C" int vpt_graph_nodes(vpt_graph *g, uint64_t first, uint64_t n, struct vpt_graph_node *dst) {
    if (!g || (!dst && n)) return fail(VPT_ERR_INVALID, "null argument");
    if (first > g->info.nodes || n > g->info.nodes - first)
        return fail(VPT_ERR_INVALID, "nodes %llu .. +%llu are not within the %llu of the graph", (unsigned long long)first, (unsigned long long)n, (unsigned long long)g->info.nodes);
    if (n) memcpy(dst, g->node.data() + first, (size_t)n * sizeof(vpt_graph_node));
    return VPT_OK;
}

// a copy of one of the graph's labellings that the caller owns
static int graph_hand_out(vpt_graph *g, const vpt_components *s, vpt_components **out) {
    HIP_TRY(hipSetDevice(g->ctx->device));
    std::unique_ptr<vpt_components> c(new vpt_components());
    int rc = graph_snapshot(c.get(), s, s->texels.get());
    if (rc == VPT_OK && hipMemcpyAsync(c->values, s->values, s->voxels() * sizeof(uint32_t), hipMemcpyDeviceToDevice, g->ctx->stream) != hipSuccess)
        rc = fail(VPT_ERR_HIP, "graph: the copy of the ranks failed");
    if (rc != VPT_OK) { (void)hipStreamSynchronize(g->ctx->stream); return rc; }
    c->list = s->list; c->info = s->info;
    memcpy(c->ms, s->ms, sizeof(c->ms)); memcpy(c->launches, s->launches, sizeof(c->launches));
    *out = c.release();
    return VPT_OK;
}

extern "C" int vpt_graph_branch_components(vpt_graph *g, vpt_components **out) {
    if (!g || !out) return fail(VPT_ERR_INVALID, "null argument");
    return graph_hand_out(g, g->branches.get(), out);
}

extern "C" int vpt_graph_node_components(vpt_graph *g, vpt_components **out) {
    if (!g || !out) return fail(VPT_ERR_INVALID, "null argument");
    return graph_hand_out(g, g->nodes.get(), out);
}

extern "C" int vpt_graph_classes(vpt_graph *g, vpt_volume **out) {
    if (!g || !out) return fail(VPT_ERR_INVALID, "null argument");
    const vpt_components *f = g->branches.get();
    HIP_TRY(hipSetDevice(g->ctx->device));
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(g->ctx, f->nx, f->ny, f->nz, f->norm16 ? VPT_FORMAT_RG16 : VPT_FORMAT_RG8, false, &d));      // every texel is written below
    const size_t n = f->voxels();
    const dim3 grid(stream_grid(n / 4 + 1));
    if (f->norm16) hipLaunchKernelGGL(k_gr_classes<uint16_t>, grid, dim3(256), 0, g->ctx->stream, (const uint16_t *)f->texels.get(), (const uint8_t *)g->classes.get(), (uint16_t *)d->linear.get(), n);
    else hipLaunchKernelGGL(k_gr_classes<uint8_t>, grid, dim3(256), 0, g->ctx->stream, (const uint8_t *)f->texels.get(), (const uint8_t *)g->classes.get(), d->linear.get(), n);
    return volume_finish_derived(g->ctx, f->filter, d, out);
}

extern "C" int vpt_graph_prune(vpt_graph *g, uint64_t length, uint32_t wf, uint32_t we, uint32_t wc, uint32_t flags, uint32_t fill, vpt_volume **out) {
    if (!g || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (wf > 65535u || we > 65535u || wc > 65535u) return fail(VPT_ERR_INVALID, "prune weights (%u, %u, %u): each is at most 65535", wf, we, wc);
    if (flags & ~VPT_GRAPH_PRUNE_DEBRIS) return fail(VPT_ERR_INVALID, "prune flags %u: bit 0 (debris) is taken", flags);
    const vpt_components *f = g->branches.get();
    const uint32_t M = f->norm16 ? 65535u : 255u;
    if (fill > M) return fail(VPT_ERR_INVALID, "fill %u: the largest code of %s is %u", fill, format_name(f->format), M);
    HIP_TRY(hipSetDevice(g->ctx->device));
    hipStream_t st = g->ctx->stream;
    // the drop bitmap, bit rank - 1
    const size_t words = g->branch.size() / 32 + 1;
    std::vector<uint32_t> bits(words, 0u);
    for (size_t k = 0; k < g->branch.size(); k++) {
        const vpt_graph_branch &b = g->branch[k];
        const uint64_t cost = (uint64_t)wf * b.steps_face + (uint64_t)we * b.steps_edge + (uint64_t)wc * b.steps_corner;
        const bool sort = b.kind == VPT_GRAPH_SPUR || ((flags & VPT_GRAPH_PRUNE_DEBRIS) && (b.kind == VPT_GRAPH_SEGMENT || b.kind == VPT_GRAPH_ISOLATED));
        if (sort && cost <= length) bits[k >> 5] |= 1u << (k & 31);
    }
    DevBuf<uint32_t> drop;
    HIP_TRY(drop.alloc(words));
    HIP_TRY(hipMemcpyAsync(drop, bits.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(g->ctx, f->nx, f->ny, f->nz, f->format, false, &d));      // every texel is written below
    const size_t n = f->voxels();
    const dim3 grid(stream_grid(n / 4 + 1));
    if (f->norm16) hipLaunchKernelGGL(k_gr_prune<uint16_t>, grid, dim3(256), 0, st, (const uint16_t *)f->texels.get(), (const uint8_t *)g->classes.get(), (const uint32_t *)f->values.get(),
                                      (const uint32_t *)drop.get(), (uint16_t *)d->linear.get(), n, fill);
    else hipLaunchKernelGGL(k_gr_prune<uint8_t>, grid, dim3(256), 0, st, (const uint8_t *)f->texels.get(), (const uint8_t *)g->classes.get(), (const uint32_t *)f->values.get(),
                            (const uint32_t *)drop.get(), d->linear.get(), n, fill);
    const int rc = volume_finish_derived(g->ctx, f->filter, d, out);
    (void)hipStreamSynchronize(st);                             // the bitmap is freed on return
    return rc;
}

extern "C" int vpt_graph_profile(vpt_graph *g, double *ms, uint64_t *launches) {
    if (!g || !ms || !launches) return fail(VPT_ERR_INVALID, "null argument");
    memcpy(ms, g->ms, sizeof(g->ms));
    *launches = g->launches;
    return VPT_OK;
}

extern "C" int vpt_graph_destroy(vpt_graph *g) {
    if (!g) return fail(VPT_ERR_INVALID, "null argument");
    (void)hipSetDevice(g->ctx->device);
    (void)hipStreamSynchronize(g->ctx->stream);      // an emitter or a copy may still read the buffers
    delete g;
    return VPT_OK;
}
