// vpt_volume_rank.hip — the rank filters of a volume over the clamped 3 x 3 x 3 box on the device (vpt_volume_rank): the median, grey-level
// erosion (the smallest tap) and dilation (the largest), and opening / closing built from the two.  C-ABI and the contract: include/vpt.h;
// kernel forms, compiler figures and measurements: DESIGN.md "Median and morphology".
#include "vpt_internal.h"

// ---------------------------------------------------------------------------------------------
// the column both kernels march: k_smooth's (vpt_volume_pyramid.hip)
// ---------------------------------------------------------------------------------------------
// A workgroup of 256 threads (32 lanes along x, 4 voxels each, by 8 rows) owns an RK_TX x RK_TY column and marches RK_TZ planes along z.
// Per plane it stages the tile and its one-voxel halo in LDS (indices clamped per axis), two buffers and one barrier per plane.
// ALIGNED (nx % 4 == 0): tile rows are loaded and results stored as one dword (uint8) or qword (uint16) per lane.
#define RK_TX 128
#define RK_TY 8
#define RK_TZ 32
#define RK_ROW (RK_TX + 8)          // LDS row: texel x0 - 1 at [3], the tile at [4 .. 4 + RK_TX), texel x0 + RK_TX at [4 + RK_TX]

template <typename T> struct Quad;
template <> struct Quad<uint8_t> {
    typedef uint32_t vec_t;
    static __device__ __forceinline__ uint32_t get(vec_t w, int i) { return (w >> (8 * i)) & 255u; }
    static __device__ __forceinline__ vec_t pack(const uint32_t *v) { return v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24); }
};
template <> struct Quad<uint16_t> {
    typedef uint2 vec_t;
    static __device__ __forceinline__ uint32_t get(vec_t w, int i) { return ((i < 2 ? w.x : w.y) >> (16 * (i & 1))) & 65535u; }
    static __device__ __forceinline__ vec_t pack(const uint32_t *v) { return make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16)); }
};

// stages plane clamp(zz) of the column into tile[RK_TY + 2][RK_ROW]: rows by0 - 1 .. by0 + RK_TY, clamped; row r by the threads of row r % RK_TY
template <typename T, bool ALIGNED>
__device__ __forceinline__ void stage_plane(T (*tile)[RK_ROW], const T *__restrict__ src, int zz, int nx, int ny, int nz, int x0, int by0, int lx, int ly) {
    typedef typename Quad<T>::vec_t vec_t;
    const int xs = x0 + lx * 4;
    const bool whole = ALIGNED && xs + 3 < nx;            // (ALIGNED: a group of four is inside the volume or outside it as a whole)
    const size_t plane = (size_t)min(max(zz, 0), nz - 1) * (size_t)ny;
    for (int r = ly; r < RK_TY + 2; r += RK_TY) {
        const int yy = min(max(by0 - 1 + r, 0), ny - 1);
        const T *row = src + (plane + (size_t)yy) * (size_t)nx;
        T *t = &tile[r][4 + lx * 4];
        if (whole) *reinterpret_cast<vec_t *>(t) = *reinterpret_cast<const vec_t *>(row + xs);
        else {
#pragma unroll
            for (int i = 0; i < 4; i++) t[i] = row[min(xs + i, nx - 1)];
        }
        if (lx == 0) tile[r][3] = row[max(x0 - 1, 0)];
        if (lx == 31) tile[r][4 + RK_TX] = row[min(x0 + RK_TX, nx - 1)];
    }
}
// the four voxels (xs .. xs + 3, y, z) of a thread
template <typename T, bool ALIGNED>
__device__ __forceinline__ void store_quad(T *__restrict__ dst, const uint32_t (&v)[4], int xs, int y, int z, int nx, int ny) {
    const size_t o = ((size_t)z * (size_t)ny + (size_t)y) * (size_t)nx + (size_t)xs;
    if (ALIGNED && xs + 3 < nx) *reinterpret_cast<typename Quad<T>::vec_t *>(dst + o) = Quad<T>::pack(v);
    else {
        for (int i = 0; i < 4 && xs + i < nx; i++) dst[o + i] = (T)v[i];
    }
}

// ---------------------------------------------------------------------------------------------
// erosion and dilation: k_rank_extreme<T, MAX, ALIGNED>
// ---------------------------------------------------------------------------------------------
// The smallest (largest) of a box is taken axis by axis.  Per plane a thread reduces the 3 x 6 texels around its four voxels to
// E = ext_x(ext_y v), keeps E for three planes in registers and emits out(z) = ext(E(z-1), E(z), E(z+1)).  All compares are unsigned on
// the whole code, widened to 32 bits.
template <bool MAX> __device__ __forceinline__ uint32_t ext(uint32_t a, uint32_t b) { return MAX ? max(a, b) : min(a, b); }

template <typename T, bool MAX, bool ALIGNED>
__global__ __launch_bounds__(256) void k_rank_extreme(const T *__restrict__ src, T *__restrict__ dst, int nx, int ny, int nz) {
    typedef Quad<T> Q;
    typedef typename Q::vec_t vec_t;
    __shared__ __align__(16) T tile[2][RK_TY + 2][RK_ROW];
    const int lx = (int)threadIdx.x & 31, ly = (int)threadIdx.x >> 5;
    const int x0 = (int)blockIdx.x * RK_TX, xs = x0 + lx * 4;
    const int by0 = (int)blockIdx.y * RK_TY, y = by0 + ly;
    const int z0 = (int)blockIdx.z * RK_TZ, z1 = min(z0 + RK_TZ, nz);

    uint32_t prev[4] = {}, cur[4] = {};
    for (int zz = z0 - 1; zz <= z1; zz++) {
        const int k = (zz - z0 + 1) & 1;
        stage_plane<T, ALIGNED>(tile[k], src, zz, nx, ny, nz, x0, by0, lx, ly);
        __syncthreads();      // (two buffers: the plane staged next was last read before this barrier)
        // ---- s[i] = ext_y of texel column xs - 1 + i, then E = ext_x of those
        uint32_t s[6];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const T *t = &tile[k][ly + j][4 + lx * 4];
            const vec_t w = *reinterpret_cast<const vec_t *>(t);
            uint32_t c[6];
            c[0] = (uint32_t)t[-1];
#pragma unroll
            for (int i = 0; i < 4; i++) c[1 + i] = Q::get(w, i);
            c[5] = (uint32_t)t[4];
#pragma unroll
            for (int i = 0; i < 6; i++) s[i] = j == 0 ? c[i] : ext<MAX>(s[i], c[i]);
        }
        uint32_t nxt[4];
#pragma unroll
        for (int i = 0; i < 4; i++) nxt[i] = ext<MAX>(ext<MAX>(s[i], s[i + 1]), s[i + 2]);
        // ---- plane z = zz - 1 is complete once its upper neighbour is known
        if (zz > z0 && y < ny && xs < nx) {
            uint32_t v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = ext<MAX>(ext<MAX>(prev[i], cur[i]), nxt[i]);
            store_quad<T, ALIGNED>(dst, v, xs, y, zz - 1, nx, ny);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) { prev[i] = cur[i]; cur[i] = nxt[i]; }
    }
}

// ---------------------------------------------------------------------------------------------
// the median: k_median<T, ALIGNED>
// ---------------------------------------------------------------------------------------------
// The median is not separable: the 27 taps of three planes meet in one selection.  What is shared is the order along y: per plane a thread
// sorts the three y-taps of each of its six texel columns xs - 1 .. xs + 4 once, and three voxels along x and three planes along z use that
// sorted triple.  All of it runs in packed 16-bit lanes for both texel widths (a uint8 code widened to 16 bits compares as it did), two
// voxels an instruction: columns are paired as P[j] = (column j, column j + 1), j = 0 .. 4, so the voxel pair (xs, xs + 1) selects from
// P[0], P[1], P[2] and the pair (xs + 2, xs + 3) from P[2], P[3], P[4], lane by lane.  The P[j] of the last three planes stay in registers
// (3 planes x 5 pairs x 3 sorted values), as k_smooth keeps C.
// Selection of the 14th of 27, exact ("forgetful selection"): of any 15 candidates the smallest has 14 above it and the largest 14 below,
// so neither is the median of the 27; both are dropped and the next tap admitted, 12 times, and the median of the last three is the result.
// Dropping takes 3 n / 2 - 2 compare-exchanges at n candidates: 150 for n = 15 .. 4, and 4 operations for the last three; with the 18 of
// the y-sorts a plane (shared by four voxels) that is 150 + 2 + 4.5 = 156.5 packed compare-exchanges per voxel pair, 78 per voxel.
typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
__device__ __forceinline__ void pk_sort2(uint32_t &a, uint32_t &b) { const uint32_t lo = pk_min(a, b); b = pk_max(a, b); a = lo; }

// the 14th smallest of t[0 .. 26], lane by lane
__device__ __forceinline__ uint32_t pk_median27(const uint32_t (&t)[27]) {
    uint32_t a[15];
#pragma unroll
    for (int i = 0; i < 15; i++) a[i] = t[i];
#pragma unroll
    for (int n = 15; n >= 4; n--) {
        // the smallest of a[0 .. n) to a[0], the largest to a[n - 1]: pairs first, then the smallest of the lower and the largest of the upper half
        const int half = (n + 1) / 2;
#pragma unroll
        for (int i = 0; i < n / 2; i++) pk_sort2(a[i], a[n - 1 - i]);
#pragma unroll
        for (int i = 1; i < half; i++) pk_sort2(a[0], a[i]);
#pragma unroll
        for (int i = n - half; i < n - 1; i++) pk_sort2(a[i], a[n - 1]);
        a[0] = t[27 - (n - 3)];         // n = 15 admits t[15], n = 4 admits t[26]; a[n - 1] is forgotten
    }
    return pk_max(pk_min(a[0], a[1]), pk_min(pk_max(a[0], a[1]), a[2]));
}

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(256) void k_median(const T *__restrict__ src, T *__restrict__ dst, int nx, int ny, int nz) {
    typedef Quad<T> Q;
    typedef typename Q::vec_t vec_t;
    __shared__ __align__(16) T tile[2][RK_TY + 2][RK_ROW];
    const int lx = (int)threadIdx.x & 31, ly = (int)threadIdx.x >> 5;
    const int x0 = (int)blockIdx.x * RK_TX, xs = x0 + lx * 4;
    const int by0 = (int)blockIdx.y * RK_TY, y = by0 + ly;
    const int z0 = (int)blockIdx.z * RK_TZ, z1 = min(z0 + RK_TZ, nz);

    uint32_t prev[15] = {}, cur[15] = {};                 // [3 j + rank]: the sorted y-triples of the column pairs P[j] of the last two planes
    for (int zz = z0 - 1; zz <= z1; zz++) {
        const int k = (zz - z0 + 1) & 1;
        stage_plane<T, ALIGNED>(tile[k], src, zz, nx, ny, nz, x0, by0, lx, ly);
        __syncthreads();      // (two buffers: the plane staged next was last read before this barrier)
        // ---- rows as the pairs (c0, c1), (c2, c3), (c4, c5) of the six columns, sorted along y
        uint32_t s[3][3];                                 // [pair][row], then [pair][rank]
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const T *t = &tile[k][ly + j][4 + lx * 4];
            const vec_t w = *reinterpret_cast<const vec_t *>(t);
            s[0][j] = (uint32_t)t[-1] | (Q::get(w, 0) << 16);
            s[1][j] = Q::get(w, 1) | (Q::get(w, 2) << 16);
            s[2][j] = Q::get(w, 3) | ((uint32_t)t[4] << 16);
        }
#pragma unroll
        for (int i = 0; i < 3; i++) { pk_sort2(s[i][0], s[i][1]); pk_sort2(s[i][1], s[i][2]); pk_sort2(s[i][0], s[i][1]); }
        uint32_t nxt[15];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            nxt[0 + r] = s[0][r];
            nxt[3 + r] = (s[0][r] >> 16) | (s[1][r] << 16);     // (c1, c2): the ranks hold lane by lane, so the lanes regroup freely
            nxt[6 + r] = s[1][r];
            nxt[9 + r] = (s[1][r] >> 16) | (s[2][r] << 16);     // (c3, c4)
            nxt[12 + r] = s[2][r];
        }
        // ---- plane z = zz - 1 is complete once its upper neighbour is known
        if (zz > z0 && y < ny && xs < nx) {
            uint32_t v[4];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                uint32_t taps[27];
#pragma unroll
                for (int i = 0; i < 9; i++) { taps[i] = prev[6 * h + i]; taps[9 + i] = cur[6 * h + i]; taps[18 + i] = nxt[6 * h + i]; }
                const uint32_t m = pk_median27(taps);
                v[2 * h] = m & 65535u; v[2 * h + 1] = m >> 16;
            }
            store_quad<T, ALIGNED>(dst, v, xs, y, zz - 1, nx, ny);
        }
#pragma unroll
        for (int i = 0; i < 15; i++) { prev[i] = cur[i]; cur[i] = nxt[i]; }
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
enum { PASS_MEDIAN = 0, PASS_MIN = 1, PASS_MAX = 2 };

template <typename T, bool ALIGNED>
static void launch_pass_as(const vpt_volume *v, int pass, const T *s, T *d) {
    const dim3 grid((unsigned)((v->nx + RK_TX - 1) / RK_TX), (unsigned)((v->ny + RK_TY - 1) / RK_TY), (unsigned)((v->nz + RK_TZ - 1) / RK_TZ));
    hipStream_t st = v->ctx->stream;
    if (pass == PASS_MEDIAN) hipLaunchKernelGGL((k_median<T, ALIGNED>), grid, dim3(256), 0, st, s, d, v->nx, v->ny, v->nz);
    else if (pass == PASS_MIN) hipLaunchKernelGGL((k_rank_extreme<T, false, ALIGNED>), grid, dim3(256), 0, st, s, d, v->nx, v->ny, v->nz);
    else hipLaunchKernelGGL((k_rank_extreme<T, true, ALIGNED>), grid, dim3(256), 0, st, s, d, v->nx, v->ny, v->nz);
}
template <typename T>
static void launch_pass(const vpt_volume *v, int pass, const T *s, T *d) {
    if (v->nx % 4 == 0) launch_pass_as<T, true>(v, pass, s, d);
    else launch_pass_as<T, false>(v, pass, s, d);
}

extern "C" int vpt_volume_rank(vpt_volume *src, int op, int passes, vpt_volume **out) {
    if (!src || !out) return fail(VPT_ERR_INVALID, "null argument");
    if (src->format != VPT_FORMAT_R8 && src->format != VPT_FORMAT_R16)
        return fail(VPT_ERR_UNSUPPORTED, "the median, erosion and dilation are taken of one-channel unsigned normalised volumes (R8, R16; the window makes one of any scalar volume), not of %s",
                    format_name(src->format));
    if (op < VPT_RANK_MEDIAN || op > VPT_RANK_CLOSE) return fail(VPT_ERR_INVALID, "%d is no rank operator (VPT_RANK_MEDIAN .. VPT_RANK_CLOSE)", op);
    if (passes < 1 || passes > 8) return fail(VPT_ERR_INVALID, "%d rank-filter passes: 1 to 8 are taken", passes);
    vpt_context *c = src->ctx;
    HIP_TRY(hipSetDevice(c->device));
    if ((src->ny + RK_TY - 1) / RK_TY > 65535 || (src->nz + RK_TZ - 1) / RK_TZ > 65535) return fail(VPT_ERR_UNSUPPORTED, "volume too large");
    // the launches of the call: p of one kind, or p of the first kind and then p of the second (opening: min, max; closing: max, min)
    const int first = op == VPT_RANK_MEDIAN ? PASS_MEDIAN : (op == VPT_RANK_ERODE || op == VPT_RANK_OPEN) ? PASS_MIN : PASS_MAX;
    const int second = op == VPT_RANK_OPEN ? PASS_MAX : PASS_MIN;
    const int launches = (op == VPT_RANK_OPEN || op == VPT_RANK_CLOSE) ? 2 * passes : passes;
    vpt_volume *d = nullptr;
    VPT_TRY(volume_create(c, src->nx, src->ny, src->nz, src->format, false, &d));   // every texel is written by the last launch
    DevBuf<uint8_t> scratch;                                 // several launches go to and fro between the result's storage and this
    if (launches > 1) {
        hipError_t e = scratch.alloc((size_t)src->nx * src->ny * src->nz * (size_t)src->vox_bytes);
        if (e != hipSuccess) { vpt_volume_destroy(d); return fail(VPT_ERR_HIP, "rank-filter scratch: %s", hipGetErrorString(e)); }
    }
    const uint8_t *from = src->linear.get();
    for (int i = 1; i <= launches; i++) {
        uint8_t *to = (launches - i) % 2 == 0 ? d->linear.get() : scratch.get();    // the last launch writes the result
        const int pass = i <= passes ? first : second;
        if (src->norm16) launch_pass<uint16_t>(src, pass, (const uint16_t *)from, (uint16_t *)to);
        else launch_pass<uint8_t>(src, pass, (const uint8_t *)from, (uint8_t *)to);
        from = to;
    }
    const int rc = volume_finish_derived(src->ctx, src->filter, d, out);       // finalized once, after the last launch
    if (launches > 1) (void)hipStreamSynchronize(c->stream); // the scratch is freed on return: its last reader has finished
    return rc;
}
