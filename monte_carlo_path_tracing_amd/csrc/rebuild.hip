// Device side of mcpt_scene_rebuild and mcpt_scene_tree_cost (include/mcpt.h): a new 4-wide tree over
// the facets a device state holds, built on the device from its current tri_v, beside the tree the traversals read.
//
// Kernels, all on one stream (kernel boundaries are the only synchronisation between blocks, as in refit.hip):
//   k_rb_bounds / k_rb_bounds_final  the box of the facet centroids: per-block partials, then one wave (min and max
//                                    do not depend on the order);
//   k_rb_morton                      one 63-bit Morton code per facet (21 bits per axis) and the facet ids;
//   rocPRIM radix_sort_pairs         the stable sort of (code, facet): position in the sorted order = leaf slot;
//   per level, top-down:
//     k_rb_split                     one thread per node of the level: the node's range of the sorted order cut into
//                                    up to four sub-ranges, and how many of them become nodes;
//     rocPRIM exclusive_scan         numbers those nodes in order (no atomics: breadth-first by construction);
//     k_rb_emit                      writes the BvhNode4 / BvhNode4Q (children, counts, empty boxes), the ranges of
//                                    the next level's nodes and their traversal-stack depth;
//   k_rb_leaves                      leaf_v, the facet -> slot map and every slot's dirty byte;
//   refit_levels_enqueue             refit.hip's k_refit_level over all levels, deepest first: every fp32 box with
//                                    the build's margin and every quantised node by the one rule there is.
// The host reads three words back after each level (the size of the next one, the stack need so far, the error
// flags): at most kRebuildMaxLevels small round trips per rebuild, and the host needs level_first anyway.
//
// Depth: a node on level l (root 0) may own at most leaf_max * 4^(kRebuildMaxLevels - l) facets; a cut is moved
// towards the median whenever a side would not fit what the remaining levels can hold, so level 14's children are all
// leaves for every input (also for any number of coincident triangles, whose codes are all equal).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstring>  // before rocprim.hpp
#include <vector>

#include <rocprim/rocprim.hpp>

#include "mcpt.h"
#include "mcpt_internal.h"

namespace mcpt {

namespace {

#define RB_HIP_OK(x)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MCPT_E_DEVICE;                                                              \
        }                                                                                      \
    } while (0)

constexpr int kRbBlock = 256;
constexpr int kRbMaxPartials = 1024;

// lane l takes lane l + off: the same tree every run
__device__ inline double wave_min(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
    return v;
}
__device__ inline double wave_max(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    return v;
}

// the centre of the facet's box on each axis, in double (exact: a sum of two floats halved); a hidden facet
// (mcpt_scene_set_visible; hidden may be null) is its first vertex, where its collapsed slot sits
__device__ inline void facet_centroid(const float4* __restrict__ tri_v, const uint8_t* __restrict__ hidden, int f, double c[3]) {
    const float4 a = tri_v[3 * (size_t)f];
    const bool hid = hidden && hidden[f];
    const float4 b = hid ? a : tri_v[3 * (size_t)f + 1], d = hid ? a : tri_v[3 * (size_t)f + 2];
    c[0] = 0.5 * ((double)fminf(fminf(a.x, b.x), d.x) + (double)fmaxf(fmaxf(a.x, b.x), d.x));
    c[1] = 0.5 * ((double)fminf(fminf(a.y, b.y), d.y) + (double)fmaxf(fmaxf(a.y, b.y), d.y));
    c[2] = 0.5 * ((double)fminf(fminf(a.z, b.z), d.z) + (double)fmaxf(fmaxf(a.z, b.z), d.z));
}

// part: six arrays of nb doubles (lo x y z, hi x y z)
__global__ __launch_bounds__(kRbBlock) void k_rb_bounds(const float4* __restrict__ tri_v, const uint8_t* __restrict__ hidden, int F, int nb,
                                                        double* __restrict__ part) {
    __shared__ double s[6][kRbBlock / 64];
    double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    for (int f = blockIdx.x * kRbBlock + threadIdx.x; f < F; f += nb * kRbBlock) {
        double c[3];
        facet_centroid(tri_v, hidden, f, c);
#pragma unroll
        for (int a = 0; a < 3; a++) lo[a] = fmin(lo[a], c[a]), hi[a] = fmax(hi[a], c[a]);
    }
    const int wave = threadIdx.x / 64;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double l = wave_min(lo[a]), h = wave_max(hi[a]);
        if ((threadIdx.x & 63) == 0) s[a][wave] = l, s[3 + a][wave] = h;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        double v = s[threadIdx.x][0];
        for (int w = 1; w < kRbBlock / 64; w++) v = threadIdx.x < 3 ? fmin(v, s[threadIdx.x][w]) : fmax(v, s[threadIdx.x][w]);
        part[(size_t)threadIdx.x * nb + blockIdx.x] = v;
    }
}

// one wave: bounds[0..2] = lo, bounds[3..5] = hi
__global__ __launch_bounds__(64) void k_rb_bounds_final(const double* __restrict__ part, int nb, double* __restrict__ bounds) {
    for (int a = 0; a < 6; a++) {
        double v = a < 3 ? DBL_MAX : -DBL_MAX;
        for (int b = threadIdx.x; b < nb; b += 64) v = a < 3 ? fmin(v, part[(size_t)a * nb + b]) : fmax(v, part[(size_t)a * nb + b]);
        v = a < 3 ? wave_min(v) : wave_max(v);
        if (threadIdx.x == 0) bounds[a] = v;
    }
}

// 21 bits -> every third bit of 63
__device__ inline uint64_t spread3(uint64_t x) {
    x &= 0x1fffffull;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__global__ __launch_bounds__(kRbBlock) void k_rb_morton(const float4* __restrict__ tri_v, const uint8_t* __restrict__ hidden, int F,
                                                        const double* __restrict__ bounds,
                                                        uint64_t* __restrict__ keys, int32_t* __restrict__ vals) {
    const int f = blockIdx.x * kRbBlock + threadIdx.x;
    if (f >= F) return;
    double c[3];
    facet_centroid(tri_v, hidden, f, c);
    uint64_t q[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double lo = bounds[a], ext = bounds[3 + a] - lo;
        double g = ext > 0 ? (c[a] - lo) / ext * 2097152.0 : 0.0;
        g = fmin(fmax(g, 0.0), 2097151.0);
        q[a] = (uint64_t)g;
    }
    keys[f] = spread3(q[0]) << 2 | spread3(q[1]) << 1 | spread3(q[2]);
    vals[f] = f;
}

// where the sorted range [b, e) (e - b >= 2) is cut: at the first key with the highest differing bit set, at the
// median where all keys are equal; then moved towards the median until neither side holds more than `side_cap`
__device__ inline int cut_range(const uint64_t* __restrict__ keys, int b, int e, int64_t side_cap) {
    const int n = e - b;
    const uint64_t kb = keys[b], ke = keys[e - 1];
    int m;
    if (kb == ke) {
        m = b + n / 2;
    } else {
        const int bit = 63 - __clzll((long long)(kb ^ ke));
        int lo = b + 1, hi = e - 1;  // keys[b] has the bit clear, keys[e - 1] has it set
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if ((keys[mid] >> bit) & 1ull) hi = mid;
            else lo = mid + 1;
        }
        m = lo;
    }
    const int64_t lmin = max((int64_t)1, (int64_t)n - side_cap), lmax = min((int64_t)n - 1, side_cap);
    const int64_t left = min(max((int64_t)(m - b), lmin), lmax);
    return b + (int)left;
}

// cuts[i] = (x1, x2, x3, children): child k of node n0 + i owns [x_k, x_{k+1}) with x_0 = the range's begin and
// x_children = its end.  child_cap: the most facets a node of the next level may own (leaf_max on the last level)
__global__ __launch_bounds__(kRbBlock) void k_rb_split(const uint64_t* __restrict__ keys, const int32_t* __restrict__ node_b,
                                                       const int32_t* __restrict__ node_e, int n0, int n, int leaf_max,
                                                       int64_t child_cap, int4* __restrict__ cuts, int32_t* __restrict__ cnt) {
    const int i = blockIdx.x * kRbBlock + threadIdx.x;
    if (i >= n) return;
    const int b = node_b[n0 + i], e = node_e[n0 + i];
    int x1 = e, x2 = e, x3 = e, nc = 1;  // a range of at most leaf_max facets (the root's only): one leaf child
    if (e - b > leaf_max) {
        const int m = cut_range(keys, b, e, 2 * child_cap);
        const bool sl = m - b > leaf_max, sr = e - m > leaf_max;
        const int cl = sl ? cut_range(keys, b, m, child_cap) : m, cr = sr ? cut_range(keys, m, e, child_cap) : e;
        if (sl) x1 = cl, x2 = m, x3 = cr;
        else x1 = m, x2 = cr;
        nc = 2 + sl + sr;
    }
    // trailing sub-ranges of a node with fewer than four children are empty
    cuts[i] = make_int4(x1, x2, x3, nc);
    cnt[i] = (x1 - b > leaf_max) + (x2 - x1 > leaf_max) + (x3 - x2 > leaf_max) + (e - x3 > leaf_max);
}

struct EmitOut {
    BvhNode4* bvh4;
    BvhNode4Q* bvh4q;
    int32_t *node_b, *node_e, *above;
    int32_t* words;  // [0] stack need (max), [1] error flags (or), [2] nodes of the next level
    int32_t cap_nodes;
};

__global__ __launch_bounds__(kRbBlock) void k_rb_emit(EmitOut o, const int4* __restrict__ cuts, const int32_t* __restrict__ off,
                                                      int n0, int n, int leaf_max) {
    const int i = blockIdx.x * kRbBlock + threadIdx.x;
    int here = 0;
    if (i < n) {
        const int ni = n0 + i;
        const int4 c = cuts[i];
        const int x[5] = {o.node_b[ni], c.x, c.y, c.z, o.node_e[ni]};
        const int nc = c.w;
        here = o.above[ni] + max(nc - 1, 0);
        int ch[4] = {kBvh4Empty, kBvh4Empty, kBvh4Empty, kBvh4Empty}, ct[4] = {0, 0, 0, 0};
        int next = n0 + n + off[i], bad = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k >= nc) continue;
            const int s = x[k], t = x[k + 1], sz = t - s;
            if (sz < 1) {
                bad |= 1;
            } else if (sz <= leaf_max) {
                if (sz >= (1 << kBvh4LeafBits) || s >= (1 << (31 - kBvh4LeafBits))) bad |= 2;
                ch[k] = ~((s << kBvh4LeafBits) | sz);
                ct[k] = sz;
            } else if (next >= o.cap_nodes) {
                bad |= 4;
            } else {
                ch[k] = next;
                o.node_b[next] = s;
                o.node_e[next] = t;
                o.above[next] = here;
                next++;
            }
        }
        if (bad) atomicOr(o.words + 1, bad);  // only a refused build gets here
        if (i == n - 1) o.words[2] = next - (n0 + n);
        float4* nd = reinterpret_cast<float4*>(o.bvh4 + ni);
        const float4 elo = make_float4(FLT_MAX, FLT_MAX, FLT_MAX, FLT_MAX), ehi = make_float4(-FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX);
        const float4 chf = make_float4(__int_as_float(ch[0]), __int_as_float(ch[1]), __int_as_float(ch[2]), __int_as_float(ch[3]));
#pragma unroll
        for (int a = 0; a < 3; a++) nd[a] = elo, nd[3 + a] = ehi;
        nd[6] = chf;
        nd[7] = make_float4(__int_as_float(ct[0]), __int_as_float(ct[1]), __int_as_float(ct[2]), __int_as_float(ct[3]));
        float4* qn = reinterpret_cast<float4*>(o.bvh4q + ni);  // planes by the refit; pad and child here
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        qn[0] = z, qn[1] = z, qn[2] = z;
        qn[3] = chf;
    }
    for (int d = 32; d >= 1; d >>= 1) here = max(here, __shfl_xor(here, d));
    if ((threadIdx.x & 63) == 0 && here > 0) atomicMax(o.words, here);  // an integer max: any order
}

__global__ __launch_bounds__(kRbBlock) void k_rb_root(int32_t* node_b, int32_t* node_e, int32_t* above, int F) {
    if (blockIdx.x == 0 && threadIdx.x == 0) node_b[0] = 0, node_e[0] = F, above[0] = 0;
}

// slot s holds facet vals[s]; a hidden facet's slot is collapsed to its first vertex (k_visibility_scatter's form)
__global__ __launch_bounds__(kRbBlock) void k_rb_leaves(const float4* __restrict__ tri_v, const uint8_t* __restrict__ hidden,
                                                        const int32_t* __restrict__ vals, int F,
                                                        float4* __restrict__ leaf_v, int32_t* __restrict__ slot_start,
                                                        int32_t* __restrict__ slot_list, uint8_t* __restrict__ slot_dirty) {
    const int s = blockIdx.x * kRbBlock + threadIdx.x;
    if (s >= F) return;
    const int f = vals[s];
    float4 v0 = tri_v[3 * (size_t)f];
    const bool hid = hidden && hidden[f];
    const float4 v1 = hid ? v0 : tri_v[3 * (size_t)f + 1], v2 = hid ? v0 : tri_v[3 * (size_t)f + 2];
    v0.w = __int_as_float(f);
    leaf_v[3 * (size_t)s] = v0;
    leaf_v[3 * (size_t)s + 1] = make_float4(v1.x, v1.y, v1.z, 0.f);
    leaf_v[3 * (size_t)s + 2] = make_float4(v2.x, v2.y, v2.z, 0.f);
    slot_list[f] = s;
    slot_dirty[s] = 1;
    slot_start[s] = s;
    if (s == F - 1) slot_start[F] = F;
}

// ---- mcpt_scene_tree_cost ----
__device__ inline double slot_area(const BvhNode4& n, int k) {
    const double dx = (double)n.hi[0][k] - (double)n.lo[0][k], dy = (double)n.hi[1][k] - (double)n.lo[1][k],
                 dz = (double)n.hi[2][k] - (double)n.lo[2][k];
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}
__device__ inline double root_area(const BvhNode4& r) {
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    bool any = false;
    for (int k = 0; k < 4; k++)
        if (r.child[k] != kBvh4Empty) {
            any = true;
            for (int a = 0; a < 3; a++) lo[a] = fminf(lo[a], r.lo[a][k]), hi[a] = fmaxf(hi[a], r.hi[a][k]);
        }
    if (!any) return 0.0;
    const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1], dz = (double)hi[2] - (double)lo[2];
    return 2.0 * (dx * dy + dy * dz + dz * dx);
}

// block b sums nodes [b * chunk, (b + 1) * chunk) into part[b]: lanes in a fixed tree, waves in index order
__global__ __launch_bounds__(kRbBlock) void k_tree_cost(const BvhNode4* __restrict__ nodes, int n, int chunk, double* __restrict__ part) {
    __shared__ double s[kRbBlock / 64];
    const double a0 = root_area(nodes[0]);
    const int p0 = blockIdx.x * chunk, p1 = min(n, p0 + chunk);
    double sum = 0.0;
    if (a0 > 0.0)
        for (int p = p0 + threadIdx.x; p < p1; p += kRbBlock) {
            const BvhNode4& nd = nodes[p];
            for (int k = 0; k < 4; k++)
                if (nd.child[k] != kBvh4Empty) sum += slot_area(nd, k) / a0 * (double)(nd.child[k] < 0 ? nd.count[k] : 1);
        }
    for (int off = 32; off >= 1; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x / 64] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kRbBlock / 64; w++) sum += s[w];
        part[blockIdx.x] = sum;
    }
}
__global__ __launch_bounds__(64) void k_tree_cost_final(const double* __restrict__ part, int nb, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < nb; b++) s += part[b];
    *out = s;
}

template <class T>
int rb_alloc(std::vector<void*>& owned, size_t count, T** out) {
    void* p = nullptr;
    RB_HIP_OK(hipMalloc(&p, std::max<size_t>(count * sizeof(T), 256)));
    owned.push_back(p);
    *out = static_cast<T*>(p);
    return MCPT_OK;
}

}  // namespace

struct RebuildWork {
    int32_t F = 0;
    std::vector<void*> owned;
    uint64_t *keys0 = nullptr, *keys1 = nullptr;
    int32_t *vals0 = nullptr, *vals1 = nullptr;
    int32_t *node_b = nullptr, *node_e = nullptr, *above = nullptr, *cnt = nullptr, *off = nullptr, *words = nullptr;
    int4* cuts = nullptr;
    double* part = nullptr;  // 6 * kRbMaxPartials partials, then the six bounds
    void* temp = nullptr;
    size_t temp_bytes = 0;
};

void rebuild_work_destroy(RebuildWork* w) {
    if (!w) return;
    for (void* p : w->owned) (void)hipFree(p);
    delete w;
}

int rebuild_work_create(int32_t F, RebuildWork** out) {
    if (F < 1 || F >= (1 << (31 - kBvh4LeafBits))) {
        set_error("mcpt_scene_rebuild: %d facets do not fit the traversal's leaf code", F);
        return MCPT_E_SCENE;
    }
    RebuildWork* w = new RebuildWork;
    w->F = F;
    const size_t n = (size_t)F;
    int rc;
    if ((rc = rb_alloc(w->owned, n, &w->keys0)) || (rc = rb_alloc(w->owned, n, &w->keys1)) || (rc = rb_alloc(w->owned, n, &w->vals0)) ||
        (rc = rb_alloc(w->owned, n, &w->vals1)) || (rc = rb_alloc(w->owned, n, &w->node_b)) || (rc = rb_alloc(w->owned, n, &w->node_e)) ||
        (rc = rb_alloc(w->owned, n, &w->above)) || (rc = rb_alloc(w->owned, n, &w->cnt)) || (rc = rb_alloc(w->owned, n, &w->off)) ||
        (rc = rb_alloc(w->owned, 16, &w->words)) || (rc = rb_alloc(w->owned, n, &w->cuts)) ||
        (rc = rb_alloc(w->owned, 6 * (size_t)kRbMaxPartials + 8, &w->part))) {
        rebuild_work_destroy(w);
        return rc;
    }
    size_t sort_bytes = 0, scan_bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_bytes, w->keys0, w->keys1, w->vals0, w->vals1, n, 0, 63, (hipStream_t) nullptr);
    if (e == hipSuccess)
        e = rocprim::exclusive_scan(nullptr, scan_bytes, w->cnt, w->off, (int32_t)0, n, rocprim::plus<int32_t>(), (hipStream_t) nullptr);
    if (e != hipSuccess) {
        set_error("mcpt_scene_rebuild: rocPRIM temporary-storage query failed: %s", hipGetErrorString(e));
        rebuild_work_destroy(w);
        return MCPT_E_DEVICE;
    }
    w->temp_bytes = std::max(sort_bytes, scan_bytes);
    unsigned char* t = nullptr;
    if ((rc = rb_alloc(w->owned, w->temp_bytes, &t))) {
        rebuild_work_destroy(w);
        return rc;
    }
    w->temp = t;
    *out = w;
    return MCPT_OK;
}

int rebuild_build(RebuildWork* w, RefitDev* out, int leaf_max, int stack_cap, double margin, void* stream,
                  std::vector<int32_t>* level_first, int32_t* stack_need) {
    const int F = w->F;
    if (out->F != F || out->nslots != F || leaf_max < 1 || leaf_max >= (1 << kBvh4LeafBits)) {
        set_error("rebuild: buffers or leaf size do not match the device state");
        return MCPT_E_INVALID;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float4* tri_v = reinterpret_cast<const float4*>(out->tri_v);
    const int fblocks = (F + kRbBlock - 1) / kRbBlock, nb = std::min(fblocks, kRbMaxPartials);
    double* bounds = w->part + 6 * (size_t)kRbMaxPartials;
    hipLaunchKernelGGL(k_rb_bounds, dim3(nb), dim3(kRbBlock), 0, st, tri_v, out->hidden, F, nb, w->part);
    hipLaunchKernelGGL(k_rb_bounds_final, dim3(1), dim3(64), 0, st, w->part, nb, bounds);
    hipLaunchKernelGGL(k_rb_morton, dim3(fblocks), dim3(kRbBlock), 0, st, tri_v, out->hidden, F, bounds, w->keys0, w->vals0);
    RB_HIP_OK(hipGetLastError());
    size_t tb = w->temp_bytes;
    RB_HIP_OK(rocprim::radix_sort_pairs(w->temp, tb, w->keys0, w->keys1, w->vals0, w->vals1, (size_t)F, 0, 63, st));
    RB_HIP_OK(hipMemsetAsync(w->words, 0, 16 * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_rb_root, dim3(1), dim3(kRbBlock), 0, st, w->node_b, w->node_e, w->above, F);
    // the most facets a node of level l + 1 may own: leaf_max * 4^(kRebuildMaxLevels - 1 - l), saturated
    auto child_cap = [&](int l) {
        int64_t c = leaf_max;
        for (int k = 0; k < kRebuildMaxLevels - 1 - l && c < ((int64_t)1 << 40); k++) c *= 4;
        return c;
    };
    if ((int64_t)F > 4 * child_cap(0)) {
        set_error("mcpt_scene_rebuild: %d facets do not fit %d levels of %d-facet leaves", F, kRebuildMaxLevels, leaf_max);
        return MCPT_E_SCENE;
    }
    const EmitOut eo{out->bvh4, out->bvh4q, w->node_b, w->node_e, w->above, w->words, F};
    std::vector<int32_t> lf{0, 1};
    int32_t hw[3] = {0, 0, 0};
    for (int l = 0;; l++) {
        const int n0 = lf[l], n = lf[l + 1] - n0, blocks = (n + kRbBlock - 1) / kRbBlock;
        hipLaunchKernelGGL(k_rb_split, dim3(blocks), dim3(kRbBlock), 0, st, w->keys1, w->node_b, w->node_e, n0, n, leaf_max,
                           child_cap(l), w->cuts, w->cnt);
        RB_HIP_OK(hipGetLastError());
        tb = w->temp_bytes;
        RB_HIP_OK(rocprim::exclusive_scan(w->temp, tb, w->cnt, w->off, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), st));
        hipLaunchKernelGGL(k_rb_emit, dim3(blocks), dim3(kRbBlock), 0, st, eo, w->cuts, w->off, n0, n, leaf_max);
        RB_HIP_OK(hipGetLastError());
        RB_HIP_OK(hipMemcpyAsync(hw, w->words, sizeof hw, hipMemcpyDeviceToHost, st));
        RB_HIP_OK(hipStreamSynchronize(st));
        if (hw[1] || hw[2] < 0 || (int64_t)lf.back() + hw[2] > F || (hw[2] > 0 && l + 1 >= kRebuildMaxLevels)) {
            set_error("mcpt_scene_rebuild: the new tree failed its checks on level %d (flags %d, %d nodes follow %d)", l, hw[1],
                      hw[2], lf.back());
            return MCPT_E_SCENE;
        }
        if (hw[2] == 0) break;
        lf.push_back(lf.back() + hw[2]);
    }
    // no traversal may ever see a tree that could drop a push
    if (hw[0] > stack_cap) {
        set_error("mcpt_scene_rebuild: the new tree needs %d traversal stack entries, more than the %d the kernels hold", hw[0],
                  stack_cap);
        return MCPT_E_SCENE;
    }
    out->nnodes = lf.back();
    hipLaunchKernelGGL(k_rb_leaves, dim3(fblocks), dim3(kRbBlock), 0, st, tri_v, out->hidden, w->vals1, F,
                       reinterpret_cast<float4*>(out->leaf_v),
                       const_cast<int32_t*>(out->slot_start), const_cast<int32_t*>(out->slot_list), out->slot_dirty);
    RB_HIP_OK(hipGetLastError());
    RB_HIP_OK(hipMemsetAsync(out->node_dirty, 0, (size_t)out->nnodes, st));
    int rc;
    if ((rc = refit_levels_enqueue(*out, lf.data(), (int)lf.size() - 1, margin, stream))) return rc;
    *level_first = std::move(lf);
    *stack_need = hw[0];
    return MCPT_OK;
}

int tree_cost_enqueue(const BvhNode4* nodes, int32_t nnodes, double* words, void* stream, double** result) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nnodes < 1) {
        RB_HIP_OK(hipMemsetAsync(words, 0, sizeof(double), st));
        *result = words;
        return MCPT_OK;
    }
    int chunk = (nnodes + kRbMaxPartials - 1) / kRbMaxPartials;
    chunk = (chunk + kRbBlock - 1) / kRbBlock * kRbBlock;
    const int nb = (nnodes + chunk - 1) / chunk;
    hipLaunchKernelGGL(k_tree_cost, dim3(nb), dim3(kRbBlock), 0, st, nodes, nnodes, chunk, words);
    hipLaunchKernelGGL(k_tree_cost_final, dim3(1), dim3(64), 0, st, words, nb, words + nb);
    RB_HIP_OK(hipGetLastError());
    *result = words + nb;
    return MCPT_OK;
}

}  // namespace mcpt
