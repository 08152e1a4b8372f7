// vpt_volume_surface.hip — the isosurface of a volume as a mesh by naive surface nets on the device (vpt_volume_surface and the
// vpt_surface_* family): one vertex per cell the surface crosses, one quad per grid edge it crosses, all in integers and in a fixed order.
// C-ABI and the contract: include/vpt.h; why the order is deterministic, compiler figures and measurements: DESIGN.md "Surface".
//
// Five phases, each its own launches on the context's stream; no workgroup waits for another:
//   1. the inside plane: one bit per point of the padded grid (-1 .. W, H, D), 32 along x a word, the padding bits 0          k_sf_inside
//   2. classify: a lane a word of 32 cells: the active mask, the three owned-edge masks (a cell owns the edges that leave its
//      corner 0 along +x, +y, +z), and two counts a word: active cells, owned crossings                                        k_sf_classify
//   3. exclusive prefix sums of both count arrays over the words in raster order, reduce-then-scan: sums of blocks of words,
//      a scan of those sums by one workgroup per array, then the scan inside every block      k_sf_block_sums, k_sf_scan_blocks, k_sf_scan_add
//   4. vertices: an active cell reads its eight codes, forms q and stores it at offset[word] + popcount(active & below(bit))   k_sf_vertices
//   5. quads: an owned crossing finds its four cells' numbers the same way and stores its uint4                                k_sf_quads
// No atomic decides an address: a vertex's and a quad's place is a prefix sum plus a popcount, so the order is the contract's.  The emit
// kernels compact their work into an LDS queue first (where the surface is thin a workgroup's words hold few set bits), so that full
// waves do the divisions and the gathers, as k_sk_step does; the place in the queue is anybody's, the place in the result is not.
#include "vpt_internal.h"

#define SF_COUNT_SLOTS 64
#define SF_SCAN_WORDS 2048u         // words a block of the prefix sums (vpt_volume_surface_capped: any other)
#define SF_V_WORDS 256              // words a workgroup of k_sf_vertices: at most 8192 queued cells
#define SF_Q_WORDS 128              // words a workgroup of k_sf_quads: at most 12288 queued crossings
enum { SF_INSIDE = 0, SF_CROSS = 1, SF_TALLIES = 4 };             // per slot: inside voxels, crossings along x, y, z

struct vpt_surface {
    vpt_context *ctx = nullptr;
    struct vpt_surface_info info = {};
    DevBuf<uint32_t> vertices, quads;          // 3 words a vertex, 4 a quad
    double ms[VPT_SURFACE_PHASES] = {};
};

// the grid of a call.  Array indices are coordinates + 1: point (x, y, z) is bit x + 1 of plane row (y + 1, z + 1), cell (i, j, k) is bit
// i + 1 of cell row (j + 1, k + 1), and the corner 0 of a cell is the point with the cell's indices.
struct SfGrid {
    int W, H, D;
    int wpr, cwpr;                 // words a row: of the W + 2 grid points, of the W + 1 cells (cwpr <= wpr).  An axis is at most 4096, so the
                                   // plane's wave items (4098^2 rows of 65) and the cell words (4097^2 rows of 129) stay below 2^32: 32-bit divisions
    int stride, channel;           // the texel of voxel v is src[v * stride + channel]
};

// ---------------------------------------------------------------------------------------------
// 1. the inside plane
// ---------------------------------------------------------------------------------------------
// A wave owns 64 grid points of a padded row: one ballot is two words of the plane.  Rows y = -1, H and z = -1, D, the points x = -1 and
// x >= W come out 0.
template <typename T>
__global__ __launch_bounds__(256) void k_sf_inside(const T *__restrict__ src, uint32_t *__restrict__ plane, SfGrid g, int segs, size_t rows, uint32_t level,
                                                  unsigned long long *__restrict__ tally) {
    const int lane = (int)threadIdx.x & 63;
    const size_t wave = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (size_t)gridDim.x * 4, items = rows * (size_t)segs;
    unsigned long long counted = 0ull;                           // (wave-uniform)
    for (size_t item = wave; item < items; item += waves) {
        const uint32_t row = (uint32_t)item / (uint32_t)segs; const int seg = (int)((uint32_t)item % (uint32_t)segs);      // (items < 2^32: SfGrid)
        const int x = seg * 64 + lane - 1, y = (int)(row % (uint32_t)(g.H + 2)) - 1, z = (int)(row / (uint32_t)(g.H + 2)) - 1;
        bool in = false;
        if (x >= 0 && x < g.W && y >= 0 && y < g.H && z >= 0 && z < g.D)
            in = (uint32_t)src[(((size_t)z * (size_t)g.H + (size_t)y) * (size_t)g.W + (size_t)x) * (size_t)g.stride + (size_t)g.channel] >= level;
        const unsigned long long b = __ballot(in);
        if (lane < 2 && 2 * seg + lane < g.wpr) plane[row * (size_t)g.wpr + (size_t)(2 * seg + lane)] = (uint32_t)(b >> (32 * lane));
        counted += (unsigned long long)__popcll(b);
    }
    if (lane == 0 && counted) atomicAdd(&tally[(wave % SF_COUNT_SLOTS) * SF_TALLIES + SF_INSIDE], counted);
}

// ---------------------------------------------------------------------------------------------
// 2. classify
// ---------------------------------------------------------------------------------------------
// A thread a word of 32 cells.  Per bounding row (cj + oy, ck + oz) the plane's word is the corners ox = 0 of the 32 cells, and the word
// shifted down by one with the next word's bit 0 carried in is their corners ox = 1.  active = some corner inside and not all of them; an
// owned edge crosses when corner 0 and the corner one step along the axis differ.  masks: four arrays of `words` (active, x, y, z);
// counts: two (active cells, owned crossings).  The crossings per axis go to the tally: they decide no address.
__global__ __launch_bounds__(256) void k_sf_classify(const uint32_t *__restrict__ plane, uint32_t *__restrict__ masks, uint32_t *__restrict__ counts, SfGrid g, size_t words,
                                                    unsigned long long *__restrict__ tally) {
    uint32_t crossed[3] = { 0u, 0u, 0u };                        // at most 32 a word and 2^20 words a thread
    for (size_t w = (size_t)blockIdx.x * 256 + threadIdx.x; w < words; w += (size_t)gridDim.x * 256) {
        const uint32_t r = (uint32_t)w / (uint32_t)g.cwpr; const int wx = (int)((uint32_t)w % (uint32_t)g.cwpr);             // (words < 2^32: SfGrid)
        const size_t cj = r % (uint32_t)(g.H + 1), ck = r / (uint32_t)(g.H + 1);
        uint32_t any = 0u, all = ~0u, a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {                            // oy = k & 1, oz = k >> 1
            const uint32_t *row = plane + ((ck + (size_t)(k >> 1)) * (size_t)(g.H + 2) + cj + (size_t)(k & 1)) * (size_t)g.wpr;
            a[k] = row[wx];
            b[k] = (a[k] >> 1) | ((wx + 1 < g.wpr ? row[wx + 1] : 0u) << 31);
            any |= a[k] | b[k]; all &= a[k] & b[k];
        }
        const int cells = min(32, g.W + 1 - 32 * wx);
        const uint32_t valid = cells == 32 ? ~0u : (1u << cells) - 1u;
        const uint32_t active = any & ~all & valid, ex = (a[0] ^ b[0]) & valid, ey = (a[0] ^ a[1]) & valid, ez = (a[0] ^ a[2]) & valid;
        masks[w] = active; masks[words + w] = ex; masks[2 * words + w] = ey; masks[3 * words + w] = ez;
        counts[w] = (uint32_t)__popc(active);
        counts[words + w] = (uint32_t)(__popc(ex) + __popc(ey) + __popc(ez));
        crossed[0] += (uint32_t)__popc(ex); crossed[1] += (uint32_t)__popc(ey); crossed[2] += (uint32_t)__popc(ez);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        uint32_t m = crossed[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) m += (uint32_t)__shfl_xor((int)m, o);
        if (((int)threadIdx.x & 63) == 0 && m) atomicAdd(&tally[((blockIdx.x * 4 + (threadIdx.x >> 6)) % SF_COUNT_SLOTS) * SF_TALLIES + SF_CROSS + k], (unsigned long long)m);
    }
}

// ---------------------------------------------------------------------------------------------
// 3. the prefix sums
// ---------------------------------------------------------------------------------------------
// the exclusive scan of one value a thread over a workgroup of 256 (Hillis-Steele in LDS); *total: the sum of all
template <typename V>
__device__ __forceinline__ V sf_scan_256(V v, V *lds, V *total) {
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
    const V inclusive = lds[tid];
    *total = lds[255];
    __syncthreads();                                             // the next call writes lds again
    return inclusive - v;
}

// sums[y * blocks + b] = the sum of block b (per_block words) of count array y = blockIdx.y
__global__ __launch_bounds__(256) void k_sf_block_sums(const uint32_t *__restrict__ counts, size_t words, uint32_t per_block, unsigned long long *__restrict__ sums, size_t blocks) {
    __shared__ unsigned long long red[256];
    const int tid = (int)threadIdx.x;
    const uint32_t *c = counts + (size_t)blockIdx.y * words;
    for (size_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const size_t lo = b * (size_t)per_block, hi = min(lo + (size_t)per_block, words);
        unsigned long long mine = 0ull;
        for (size_t i = lo + (size_t)tid; i < hi; i += 256) mine += (unsigned long long)c[i];
        red[tid] = mine;
        __syncthreads();
#pragma unroll
        for (int o = 128; o >= 1; o >>= 1) {
            if (tid < o) red[tid] += red[tid + o];
            __syncthreads();
        }
        if (tid == 0) sums[(size_t)blockIdx.y * blocks + b] = red[0];
        __syncthreads();
    }
}

// one workgroup per count array: its block sums become their exclusive scan, totals[y] the sum of all.  A thread owns a run of the sums.
__global__ __launch_bounds__(256) void k_sf_scan_blocks(unsigned long long *__restrict__ sums, size_t blocks, unsigned long long *__restrict__ totals) {
    __shared__ unsigned long long lds[256];
    unsigned long long *s = sums + (size_t)blockIdx.x * blocks;
    const size_t per = (blocks + 255) / 256, lo = min((size_t)threadIdx.x * per, blocks), hi = min(lo + per, blocks);
    unsigned long long mine = 0ull, total;
    for (size_t i = lo; i < hi; i++) mine += s[i];
    unsigned long long run = sf_scan_256(mine, lds, &total);
    for (size_t i = lo; i < hi; i++) { const unsigned long long v = s[i]; s[i] = run; run += v; }
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// every count becomes its offset: the scan inside block b, 256 words a round with the carry, plus the block's scanned sum (the totals are
// below 2^32 or the host gives up before anything reads an offset)
__global__ __launch_bounds__(256) void k_sf_scan_add(uint32_t *__restrict__ counts, size_t words, uint32_t per_block, const unsigned long long *__restrict__ sums, size_t blocks) {
    __shared__ uint32_t lds[256];
    uint32_t *c = counts + (size_t)blockIdx.y * words;
    for (size_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const size_t lo = b * (size_t)per_block, hi = min(lo + (size_t)per_block, words);
        uint32_t carry = (uint32_t)sums[(size_t)blockIdx.y * blocks + b];
        for (size_t base = lo; base < hi; base += 256) {        // (uniform)
            const size_t i = base + threadIdx.x;
            const uint32_t v = i < hi ? c[i] : 0u;
            uint32_t total;
            const uint32_t before = sf_scan_256(v, lds, &total);
            if (i < hi) c[i] = carry + before;
            carry += total;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 4. vertices
// ---------------------------------------------------------------------------------------------
// t of a crossing edge with the codes a, b at its ends: (n 65536 + d / 2) div d with n = |2 level - 1 - 2 a|, d = 2 |b - a|.  Bytes: n 65536
// < 2^25.  16 bits: n 65536 < 2^34, so the division goes in two steps of 32 bits: n 256 = q1 d + r1, and then
// n 65536 + d / 2 = 256 q1 d + (256 r1 + d / 2), whose second part is below 2^26.
template <typename T>
__device__ __forceinline__ uint32_t sf_t(uint32_t a, uint32_t b, uint32_t level) {
    const uint32_t l2 = 2u * level - 1u, n = l2 > 2u * a ? l2 - 2u * a : 2u * a - l2, d = 2u * (a > b ? a - b : b - a);
    if (sizeof(T) == 1) return (n * 65536u + d / 2u) / d;
    const uint32_t x = n * 256u, q1 = x / d, r1 = x - q1 * d;
    return q1 * 256u + (r1 * 256u + d / 2u) / d;
}

// the number of the vertex of cell (ci, cj, ck): the offset of its word plus the active cells below it in the word
__device__ __forceinline__ uint32_t sf_vertex_of(const uint32_t *__restrict__ active, const uint32_t *__restrict__ voff, const SfGrid &g, int ci, int cj, int ck) {
    ci = max(ci, 0); cj = max(cj, 0); ck = max(ck, 0);          // (never below 0 by the contract: no read outside the arrays whatever the masks hold)
    const size_t w = ((size_t)ck * (size_t)(g.H + 1) + (size_t)cj) * (size_t)g.cwpr + (size_t)(ci >> 5);
    return voff[w] + (uint32_t)__popc(active[w] & ((1u << (ci & 31)) - 1u));
}

// A workgroup owns SF_V_WORDS words.  A thread queues the set bits of its word (one LDS atomic a word reserves the run); then thread i
// takes the i-th, i + 256-th ... queued cell: its eight codes (0 outside the volume), the twelve edges, q per axis, three stores.
template <typename T>
__global__ __launch_bounds__(256) void k_sf_vertices(const T *__restrict__ src, const uint32_t *__restrict__ active, const uint32_t *__restrict__ voff, uint32_t *__restrict__ vertices,
                                                    SfGrid g, size_t words, uint32_t level) {
    __shared__ uint16_t queue[SF_V_WORDS * 32];
    __shared__ uint32_t queued;
    const int tid = (int)threadIdx.x;
    const size_t first = (size_t)blockIdx.x * SF_V_WORDS;
    if (tid == 0) queued = 0u;
    __syncthreads();
    {
        uint32_t a = first + (size_t)tid < words ? active[first + (size_t)tid] : 0u;
        if (a) {
            uint32_t slot = atomicAdd(&queued, (uint32_t)__popc(a));
            while (a) { queue[slot++] = (uint16_t)((tid << 5) | (__ffs((int)a) - 1)); a &= a - 1u; }
        }
    }
    __syncthreads();
    const uint32_t n = queued;
    for (uint32_t e = (uint32_t)tid; e < n; e += 256u) {
        const uint32_t item = queue[e];
        const size_t w = first + (size_t)(item >> 5);
        const int bit = (int)(item & 31u);
        const uint32_t r = (uint32_t)w / (uint32_t)g.cwpr;
        const int ci = (int)((uint32_t)w % (uint32_t)g.cwpr) * 32 + bit, cj = (int)(r % (uint32_t)(g.H + 1)), ck = (int)(r / (uint32_t)(g.H + 1));
        uint32_t c[8];
#pragma unroll
        for (int o = 0; o < 8; o++) {
            const int x = ci - 1 + (o & 1), y = cj - 1 + ((o >> 1) & 1), z = ck - 1 + (o >> 2);
            c[o] = (x >= 0 && x < g.W && y >= 0 && y < g.H && z >= 0 && z < g.D)
                 ? (uint32_t)src[(((size_t)z * (size_t)g.H + (size_t)y) * (size_t)g.W + (size_t)x) * (size_t)g.stride + (size_t)g.channel] : 0u;
        }
        uint32_t m = 0u, s[3] = { 0u, 0u, 0u };
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
#pragma unroll
            for (int k = 0; k < 4; k++) {                        // the four edges along ax: offsets k & 1 along p, k >> 1 along q
                const int p = (ax + 1) % 3, q = (ax + 2) % 3, o = ((k & 1) << p) | ((k >> 1) << q);
                const uint32_t ca = c[o], cb = c[o | (1 << ax)];
                if ((ca >= level) != (cb >= level)) {
                    m++;
                    s[ax] += sf_t<T>(ca, cb, level); s[p] += (uint32_t)(k & 1) * 65536u; s[q] += (uint32_t)(k >> 1) * 65536u;
                }
            }
        }
        const size_t at = 3 * (size_t)(voff[w] + (uint32_t)__popc(active[w] & ((1u << bit) - 1u)));
        vertices[at] = (uint32_t)ci * 65536u + (2u * s[0] + m) / (2u * m);
        vertices[at + 1] = (uint32_t)cj * 65536u + (2u * s[1] + m) / (2u * m);
        vertices[at + 2] = (uint32_t)ck * 65536u + (2u * s[2] + m) / (2u * m);
    }
}

// ---------------------------------------------------------------------------------------------
// 5. quads
// ---------------------------------------------------------------------------------------------
// A workgroup owns SF_Q_WORDS words; its first SF_Q_WORDS threads queue their word's owned crossings as (word, bit, axis).  A queued
// crossing (g, a) is quad offset[word] + the crossings of the cells below g in the word + those of g along lower axes; its corners are the
// vertices of the cells g - e_u - e_v, g - e_v, g, g - e_u (all exist and are active: a crossing edge has an end inside the volume, so g's
// indices off the axis are at least 1), turned round when g is outside.
__global__ __launch_bounds__(256) void k_sf_quads(const uint32_t *__restrict__ plane, const uint32_t *__restrict__ masks, const uint32_t *__restrict__ voff, const uint32_t *__restrict__ qoff,
                                                 uint4 *__restrict__ quads, SfGrid g, size_t words) {
    __shared__ uint16_t queue[SF_Q_WORDS * 96];
    __shared__ uint32_t queued;
    const int tid = (int)threadIdx.x;
    const size_t first = (size_t)blockIdx.x * SF_Q_WORDS;
    if (tid == 0) queued = 0u;
    __syncthreads();
    if (tid < SF_Q_WORDS && first + (size_t)tid < words) {
        const size_t w = first + (size_t)tid;
        const uint32_t ex = masks[words + w], ey = masks[2 * words + w], ez = masks[3 * words + w];
        uint32_t any = ex | ey | ez;
        if (any) {
            uint32_t slot = atomicAdd(&queued, (uint32_t)(__popc(ex) + __popc(ey) + __popc(ez)));
            while (any) {
                const int bit = __ffs((int)any) - 1;
                any &= any - 1u;
                if ((ex >> bit) & 1u) queue[slot++] = (uint16_t)((tid << 7) | (bit << 2) | 0);
                if ((ey >> bit) & 1u) queue[slot++] = (uint16_t)((tid << 7) | (bit << 2) | 1);
                if ((ez >> bit) & 1u) queue[slot++] = (uint16_t)((tid << 7) | (bit << 2) | 2);
            }
        }
    }
    __syncthreads();
    const uint32_t n = queued;
    const uint32_t *active = masks;
    for (uint32_t e = (uint32_t)tid; e < n; e += 256u) {
        const uint32_t item = queue[e];
        const size_t w = first + (size_t)(item >> 7);
        const int bit = (int)((item >> 2) & 31u), a = (int)(item & 3u);
        const uint32_t ex = masks[words + w], ey = masks[2 * words + w], ez = masks[3 * words + w], below = (1u << bit) - 1u;
        const size_t at = (size_t)(qoff[w] + (uint32_t)(__popc(ex & below) + __popc(ey & below) + __popc(ez & below)) + (a > 0 ? (ex >> bit) & 1u : 0u) + (a > 1 ? (ey >> bit) & 1u : 0u));
        const uint32_t r = (uint32_t)w / (uint32_t)g.cwpr;
        const int ci = (int)((uint32_t)w % (uint32_t)g.cwpr) * 32 + bit, cj = (int)(r % (uint32_t)(g.H + 1)), ck = (int)(r / (uint32_t)(g.H + 1));
        // a = 0: u = y, v = z; a = 1: u = z, v = x; a = 2: u = x, v = y
        const int ux = a == 2, uy = a == 0, uz = a == 1, vx = a == 1, vy = a == 2, vz = a == 0;
        const uint32_t c0 = sf_vertex_of(active, voff, g, ci - ux - vx, cj - uy - vy, ck - uz - vz), c1 = sf_vertex_of(active, voff, g, ci - vx, cj - vy, ck - vz),
                       c2 = voff[w] + (uint32_t)__popc(active[w] & below), c3 = sf_vertex_of(active, voff, g, ci - ux, cj - uy, ck - uz);
        const bool in = (plane[((size_t)ck * (size_t)(g.H + 2) + (size_t)cj) * (size_t)g.wpr + (size_t)(ci >> 5)] >> (ci & 31)) & 1u;
        quads[at] = in ? make_uint4(c0, c1, c2, c3) : make_uint4(c0, c3, c2, c1);
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
// the body of vpt_volume_surface behind the argument checks; `s` is freed by the caller on failure
static int surface_build(vpt_surface *s, const vpt_volume *src, int channel, uint32_t level, uint32_t scan_words) {
    hipStream_t st = s->ctx->stream;
    SfGrid g;
    g.W = src->nx; g.H = src->ny; g.D = src->nz;
    g.wpr = (g.W + 2 + 31) / 32; g.cwpr = (g.W + 1 + 31) / 32;
    g.stride = src->channels; g.channel = channel;
    const int segs = (g.wpr + 1) / 2;
    const size_t rows = (size_t)(g.H + 2) * (size_t)(g.D + 2), plane_words = rows * (size_t)g.wpr;
    const size_t words = (size_t)(g.H + 1) * (size_t)(g.D + 1) * (size_t)g.cwpr, blocks = (words + scan_words - 1) / scan_words;
    s->info.cells = (uint64_t)(g.W + 1) * (uint64_t)(g.H + 1) * (uint64_t)(g.D + 1);
    s->info.level = level; s->info.width = g.W; s->info.height = g.H; s->info.depth = g.D; s->info.channel = channel;
    DevBuf<uint32_t> plane, masks, counts;                       // freed when the call returns
    DevBuf<unsigned long long> sums, tally;                      // 2 * blocks block sums + the two totals; SF_COUNT_SLOTS * SF_TALLIES
    HIP_TRY(plane.alloc(plane_words));
    HIP_TRY(masks.alloc(4 * words));
    HIP_TRY(counts.alloc(2 * words));
    HIP_TRY(sums.alloc(2 * blocks + 2));
    HIP_TRY(tally.alloc(SF_COUNT_SLOTS * SF_TALLIES));
    HIP_TRY(hipMemsetAsync(tally, 0, SF_COUNT_SLOTS * SF_TALLIES * sizeof(unsigned long long), st));
    HIP_TRY(hipStreamSynchronize(st));                          // what is in front of the call (an upload into src) is not its time
    PhaseClock clock(st);
    unsigned long long host_tally[SF_COUNT_SLOTS * SF_TALLIES] = {};
    // ---- the inside plane
    const dim3 inside_grid(stream_grid(rows * (size_t)segs, 4));
    if (src->norm16) hipLaunchKernelGGL(k_sf_inside<uint16_t>, inside_grid, dim3(256), 0, st, (const uint16_t *)src->linear.get(), plane.get(), g, segs, rows, level, tally.get());
    else hipLaunchKernelGGL(k_sf_inside<uint8_t>, inside_grid, dim3(256), 0, st, (const uint8_t *)src->linear.get(), plane.get(), g, segs, rows, level, tally.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_tally, tally, sizeof(host_tally), hipMemcpyDeviceToHost, st));
    HIP_TRY(clock.lap(&s->ms[0]));
    for (int i = 0; i < SF_COUNT_SLOTS; i++) s->info.inside += host_tally[i * SF_TALLIES + SF_INSIDE];
    if (s->info.inside == 0) return VPT_OK;                      // an empty surface: nothing to classify, nothing to emit
    // ---- classify
    hipLaunchKernelGGL(k_sf_classify, dim3(stream_grid(words)), dim3(256), 0, st, (const uint32_t *)plane.get(), masks.get(), counts.get(), g, words, tally.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.lap(&s->ms[1]));
    // ---- prefix sums: the counts become the offsets in place
    const dim3 scan_grid(stream_grid(blocks, 1, 65535), 2);
    unsigned long long totals[2] = {};
    hipLaunchKernelGGL(k_sf_block_sums, scan_grid, dim3(256), 0, st, (const uint32_t *)counts.get(), words, scan_words, sums.get(), blocks);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sf_scan_blocks, dim3(2), dim3(256), 0, st, sums.get(), blocks, sums.get() + 2 * blocks);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sf_scan_add, scan_grid, dim3(256), 0, st, counts.get(), words, scan_words, (const unsigned long long *)sums.get(), blocks);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(totals, sums.get() + 2 * blocks, sizeof(totals), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(host_tally, tally, sizeof(host_tally), hipMemcpyDeviceToHost, st));
    HIP_TRY(clock.lap(&s->ms[2]));
    for (int i = 0; i < SF_COUNT_SLOTS; i++)
        for (int a = 0; a < 3; a++) s->info.crossings[a] += host_tally[i * SF_TALLIES + SF_CROSS + a];
    if (totals[0] >> 32) return fail(VPT_ERR_UNSUPPORTED, "the surface has %llu vertices: 2^32 or more are not taken", totals[0]);
    if (totals[1] >> 32) return fail(VPT_ERR_UNSUPPORTED, "the surface has %llu quads: 2^32 or more are not taken", totals[1]);
    s->info.vertices = totals[0]; s->info.quads = totals[1];
    if (totals[0] == 0) return VPT_OK;
    // ---- emit
    HIP_TRY(s->vertices.alloc(3 * (size_t)totals[0]));
    HIP_TRY(s->quads.alloc(4 * (size_t)totals[1]));
    clock = PhaseClock(st);                                      // the allocations are in no phase
    const uint32_t *active = masks.get(), *voff = counts.get(), *qoff = counts.get() + words;
    const dim3 v_grid((unsigned)((words + SF_V_WORDS - 1) / SF_V_WORDS)), q_grid((unsigned)((words + SF_Q_WORDS - 1) / SF_Q_WORDS));
    if (src->norm16) hipLaunchKernelGGL(k_sf_vertices<uint16_t>, v_grid, dim3(256), 0, st, (const uint16_t *)src->linear.get(), active, voff, s->vertices.get(), g, words, level);
    else hipLaunchKernelGGL(k_sf_vertices<uint8_t>, v_grid, dim3(256), 0, st, (const uint8_t *)src->linear.get(), active, voff, s->vertices.get(), g, words, level);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.lap(&s->ms[3]));
    hipLaunchKernelGGL(k_sf_quads, q_grid, dim3(256), 0, st, (const uint32_t *)plane.get(), (const uint32_t *)masks.get(), voff, qoff, (uint4 *)s->quads.get(), g, words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.lap(&s->ms[4]));                               // the scratch goes out of scope behind its last use
    return VPT_OK;
}

static int surface_create(vpt_volume *src, int channel, uint32_t level, uint32_t scan_words, vpt_surface **out) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (src->format != VPT_FORMAT_R8 && src->format != VPT_FORMAT_RG8 && src->format != VPT_FORMAT_R16 && src->format != VPT_FORMAT_RG16)
        return fail(VPT_ERR_UNSUPPORTED, "surfaces are taken of unsigned normalised volumes (R8, RG8, R16, RG16; the window makes R8 / R16 of any scalar volume), not of %s",
                    format_name(src->format));
    if (channel != 0 && channel != 1) return fail(VPT_ERR_INVALID, "surface: channel %d: 0 or 1 are taken", channel);
    if (channel >= src->channels) return fail(VPT_ERR_INVALID, "surface: channel 1 of a volume that has one channel (%s)", format_name(src->format));
    const uint32_t M = src->norm16 ? 65535u : 255u;
    if (level < 1u || level > M) return fail(VPT_ERR_INVALID, "surface level %u: 1 <= level <= %u (the largest code of %s) is required", level, M, format_name(src->format));
    vpt_context *ctx = src->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    std::unique_ptr<vpt_surface> s(new vpt_surface());
    s->ctx = ctx;
    const int rc = surface_build(s.get(), src, channel, level, scan_words);
    if (rc != VPT_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }      // the buffers are freed on return: nothing may still use them
    *out = s.release();
    return VPT_OK;
}

extern "C" int vpt_volume_surface(vpt_volume *src, int channel, uint32_t level, vpt_surface **out) {
    return surface_create(src, channel, level, SF_SCAN_WORDS, out);
}

extern "C" int vpt_volume_surface_capped(vpt_volume *src, int channel, uint32_t level, uint32_t scan_words, vpt_surface **out) {
    if (scan_words == 0u) return fail(VPT_ERR_INVALID, "surface: scan_words 0: a positive number of words per block of the prefix sums is taken");
    return surface_create(src, channel, level, scan_words, out);
}

extern "C" int vpt_surface_info(vpt_surface *s, struct vpt_surface_info *info) {
    if (!s || !info) return fail(VPT_ERR_INVALID, "null argument");
    *info = s->info;
    return VPT_OK;
}

// `per` words of each of the items first .. first + n - 1 of `buf` (which holds `have` items) into host_dst
static int surface_page(vpt_surface *s, const uint32_t *buf, uint64_t have, const char *what, size_t per, uint64_t first, uint64_t n, uint32_t *host_dst, size_t nbytes) {
    if (!host_dst && n) return fail(VPT_ERR_INVALID, "null argument");
    if (first > have || n > have - first)
        return fail(VPT_ERR_INVALID, "%s %llu .. +%llu are not within the %llu of the surface", what, (unsigned long long)first, (unsigned long long)n, (unsigned long long)have);
    const size_t need = (size_t)n * per * sizeof(uint32_t);
    if (nbytes < need) return fail(VPT_ERR_INVALID, "%s buffer too short: %zu < %zu", what, nbytes, need);
    if (n == 0) return VPT_OK;
    HIP_TRY(hipSetDevice(s->ctx->device));
    HIP_TRY(hipMemcpyAsync(host_dst, buf + (size_t)first * per, need, hipMemcpyDeviceToHost, s->ctx->stream));
    HIP_TRY(hipStreamSynchronize(s->ctx->stream));
    return VPT_OK;
}

extern "C" int vpt_surface_vertices(vpt_surface *s, uint64_t first, uint64_t n, uint32_t *host_dst, size_t nbytes) {
    if (!s) return fail(VPT_ERR_INVALID, "null argument");
    return surface_page(s, s->vertices.get(), s->info.vertices, "vertices", 3, first, n, host_dst, nbytes);
}

extern "C" int vpt_surface_quads(vpt_surface *s, uint64_t first, uint64_t n, uint32_t *host_dst, size_t nbytes) {
    if (!s) return fail(VPT_ERR_INVALID, "null argument");
    return surface_page(s, s->quads.get(), s->info.quads, "quads", 4, first, n, host_dst, nbytes);
}

extern "C" int vpt_surface_device(vpt_surface *s, void **vertices, void **quads) {
    if (!s || !vertices || !quads) return fail(VPT_ERR_INVALID, "null argument");
    *vertices = s->vertices.get(); *quads = s->quads.get();
    return VPT_OK;
}

extern "C" int vpt_surface_profile(vpt_surface *s, double *ms) {
    if (!s || !ms) return fail(VPT_ERR_INVALID, "null argument");
    memcpy(ms, s->ms, sizeof(s->ms));
    return VPT_OK;
}

extern "C" int vpt_surface_destroy(vpt_surface *s) {
    if (!s) return fail(VPT_ERR_INVALID, "null argument");
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);      // a caller's work on the stream may still read the buffers
    delete s;
    return VPT_OK;
}
