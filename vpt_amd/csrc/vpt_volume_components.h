// vpt_volume_components.h — the object behind a vpt_components handle, for the units that work on it: vpt_volume_components.hip builds it
// from a value range (labelling, list, ranks), vpt_volume_watershed.hip builds it from a relief (basins) and vpt_volume_measure.hip reads it
// (per-component measurements, selection by a set of ranks).  The two builders share the tile's geometry, the label equivalence on L
// (find_root, unite) and the host's loop behind the tile pass (components_build), which lives in vpt_volume_components.hip.
#pragma once
#include <functional>
#include "vpt_volume_field.h"

struct vpt_components : VoxelField {       // the values are L: at the end one rank per voxel
    std::vector<vpt_component> list;        // canonical order
    struct vpt_components_info info = {};
    double ms[VPT_COMPONENTS_PHASES] = {};
    uint32_t launches[2] = {};
};

// ---------------------------------------------------------------------------------------------
// the tile, the control block, the label equivalence
// ---------------------------------------------------------------------------------------------
#define CC_TX 64
#define CC_TY 8
#define CC_TZ 4
#define CC_VOX (CC_TX * CC_TY * CC_TZ)
#define CC_PX (CC_TX + 2)
#define CC_PY (CC_TY + 2)
#define CC_PZ (CC_TZ + 2)
#define CC_PAD (CC_PX * CC_PY * CC_PZ)
#define CC_BG 0xFFFFu
static_assert(CC_VOX == 2048 && CC_PAD < 0xFFFF, "eight voxels a thread; LDS indices fit 16 bits");

// words of the control block on the device
enum { W_CHANGED = 0, W_TILE_ROOTS = 1, W_SLOT = 2, W_WORDS = 4 };
enum { Q_LISTED = 0, Q_DROPPED = 1, Q_FOREGROUND = 2, Q_LISTED_VOXELS = 3, Q_WORDS = 4 };

__device__ __forceinline__ uint32_t ld_agent(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(uint32_t *p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// is the offset (dx, dy, dz) != 0 a neighbour under CONN?
template <int CONN> __device__ __forceinline__ constexpr bool is_neighbour(int dx, int dy, int dz) {
    const int m = (dx != 0) + (dy != 0) + (dz != 0);
    return m >= 1 && m <= (CONN == 6 ? 1 : CONN == 18 ? 2 : 3);
}

// Label equivalence on L.  find follows parents to a root, at most `cap` loads for a whole unite; unite hooks the larger of two roots under
// the smaller with atomicMin.  If the word was no longer a root's (another thread hooked it in between), the atomicMin has at worst
// replaced that thread's link a -> p by a -> b with b < p, so the unite goes on with (p, b): nothing that was joined before the launch is
// ever parted (only words found to be roots IN this launch are written, and those held no link when it began).  A unite that runs out of
// steps gives up and raises W_CHANGED; the host flattens and launches again.
__device__ __forceinline__ bool find_root(const uint32_t *L, uint32_t &i, int &steps, int cap) {
    for (; steps < cap; steps++) {
        const uint32_t p = ld_agent(&L[i]) - 1u;
        if (p == i) return true;
        i = p;
    }
    return false;
}
__device__ __forceinline__ void unite(uint32_t *L, uint32_t a, uint32_t b, int cap, uint32_t *words) {
    int steps = 0;
    for (int tries = 0; tries < cap; tries++) {
        if (!find_root(L, a, steps, cap) || !find_root(L, b, steps, cap)) break;
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }                   // a > b: a goes under b
        const uint32_t old = __hip_atomic_fetch_min(&L[a], b + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a + 1u) return;                                          // a was a root still: hooked
        a = old - 1u;                                                       // the parent a had: it belongs with b too
    }
    st_agent(&words[W_CHANGED], 1u);
}

// ---------------------------------------------------------------------------------------------
// the host's loop (vpt_volume_components.hip)
// ---------------------------------------------------------------------------------------------
// What a builder brings: `tiles` enqueues its tile pass on the context's stream (any number of launches; it may block) and leaves L flat
// within every tile (a voxel names the smallest voxel of its tile component, + 1; 0: not labelled) with those tile roots counted in
// words[W_TILE_ROOTS]; `merge` enqueues one launch that unites across tiles, a unite taking at most `cap` loads and raising
// words[W_CHANGED] when it gives up.  `what` names the operation in messages.
struct ComponentsPasses {
    const char *what;
    std::function<int(uint32_t *words)> tiles;
    std::function<void(int cap, uint32_t *words)> merge;
};
// tile pass, merge and flatten until nothing gives up, sizes, census, list, ranks: fills c->values, c->list, c->info, c->ms, c->launches
int components_build(vpt_components *c, uint32_t min_voxels, int merge_steps, int flatten_steps, const ComponentsPasses &passes);
// the passes of a value range, for a builder whose foreground is a range lo .. hi of a one-byte field of its own rather than of the
// handle's texels (vpt_volume_graph.hip: the class field): the tile pass over `field`, and the merge across tiles (it reads L alone)
void components_launch_field_tiles(const vpt_components *c, const uint8_t *field, int conn, uint32_t lo, uint32_t hi, uint32_t *words);
void components_launch_merge(const vpt_components *c, int conn, int cap, uint32_t *words);
// the caps of a _capped entry point against the smallest for which the bounds of components_build's loops hold
int components_check_caps(int merge_steps, int flatten_steps);
// the chase steps the entry points without caps pass
#define CC_MERGE_STEPS 1024
#define CC_FLATTEN_STEPS 64
