// Device side of mcpt_scene_update (include/mcpt.h): new vertices are written into the facet and
// leaf arrays of a device state, and the boxes of its 4-wide tree -- the fp32 nodes of trace4_ww and the 64-byte
// quantised nodes of k_rays_persistent -- are refit bottom-up.  The topology stays, so no traversal kernel changes.
//
// Kernels, all on one stream:
//   k_refit_validate  (device form only) counts non-finite values and positions outside the arena;
//   k_transform_range (mcpt_scene_transform, §4.21) an affine map of a facet range of the rest pose into the staging
//                     arrays, counting the same offenders; the host reads the count before the scatter is enqueued;
//   k_refit_scatter   one thread per facet of the range: tri_v, tri_n, every leaf slot of the facet, its dirty byte;
//   k_visibility_scatter (mcpt_scene_set_visible, §4.28) one thread per facet of the range: its mask byte and, from
//                     tri_v, every leaf slot collapsed to the first vertex or restored, its dirty byte;
//   k_refit_level     one launch per tree level, deepest first, one thread per node: a leaf child with a dirty slot
//                     gets the union of the full bounds of all its triangles, enlarged by the build's margin; an
//                     inner child whose node is dirty gets the union of that node's slot boxes; a node with a
//                     recomputed slot is marked dirty and requantised by the same thread;
//   two memsets       clear the dirty bytes.
// A level reads only what the launch before it wrote (the level below) and writes only its own nodes: kernel
// boundaries on the stream are the only synchronisation, and no block waits on another.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "mcpt.h"
#include "mcpt_internal.h"

namespace mcpt {

namespace {

#define REFIT_HIP_OK(x)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MCPT_E_DEVICE;                                                              \
        }                                                                                      \
    } while (0)

constexpr int kRefitBlock = 256;

struct Arena {
    double lo[3], hi[3];
};

// std::nextafter(x, +-FLT_MAX) for a finite x (Builder::to_float_box's outward ulp)
__device__ inline float next_up(float x) {
    if (x == 0.0f) return __uint_as_float(1u);
    const unsigned b = __float_as_uint(x);
    return __uint_as_float(x > 0.0f ? b + 1u : b - 1u);
}
__device__ inline float next_down(float x) { return -next_up(-x); }

__device__ inline float comp(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ inline int comp(const int4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }
__device__ inline void set_comp(float4& v, int k, float x) {
    if (k == 0) v.x = x;
    if (k == 1) v.y = x;
    if (k == 2) v.z = x;
    if (k == 3) v.w = x;
}

// i indexes the count * 9 floats of the range: axis i % 3 of some vertex
__global__ __launch_bounds__(kRefitBlock) void k_refit_validate(int64_t n, const float* __restrict__ pos,
                                                                const float* __restrict__ nrm, Arena ar, unsigned* bad) {
    const int64_t i = (int64_t)blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= n) return;
    const int a = (int)(i % 3);
    const float p = pos[i];
    bool b = !isfinite(p) || (double)p < ar.lo[a] || (double)p > ar.hi[a];
    if (nrm) b = b || !isfinite(nrm[i]);
    if (b) atomicAdd(bad, 1u);  // only a refused call gets here
}

// The block's facets go through LDS so that the input is read with consecutive lanes on consecutive dwords; a
// thread then takes its facet's 9 floats at stride 9 (odd: no bank conflict) and stores float4s.
__global__ __launch_bounds__(kRefitBlock) void k_refit_scatter(RefitDev r, int first, int count, const float* __restrict__ pos,
                                                               const float* __restrict__ nrm) {
    __shared__ float sp[9 * kRefitBlock];
    const int base = blockIdx.x * kRefitBlock;
    const int nb = min(kRefitBlock, count - base);
    const size_t off = 9 * (size_t)base;
    for (int i = threadIdx.x; i < 9 * nb; i += kRefitBlock) sp[i] = pos[off + i];
    if (nrm) {
        float* out = r.tri_n + 9 * (size_t)(first + base);
        for (int i = threadIdx.x; i < 9 * nb; i += kRefitBlock) out[i] = nrm[off + i];
    }
    __syncthreads();
    if ((int)threadIdx.x >= nb) return;
    const int f = first + base + (int)threadIdx.x;
    const float* p = sp + 9 * threadIdx.x;
    float4 v0 = make_float4(p[0], p[1], p[2], 0.0f);
    const float4 v1 = make_float4(p[3], p[4], p[5], 0.0f), v2 = make_float4(p[6], p[7], p[8], 0.0f);
    float4* tv = reinterpret_cast<float4*>(r.tri_v) + 3 * (size_t)f;
    tv[0] = v0;
    tv[1] = v1;
    tv[2] = v2;
    // a hidden facet (mcpt_scene_set_visible) keeps its new values in tri_v; its slots hold the new v0 three times
    const bool hid = r.hidden && r.hidden[f];
    const float4 s1 = hid ? v0 : v1, s2 = hid ? v0 : v2;
    v0.w = __int_as_float(f);  // the facet id bits of the slot's first vertex
    for (int q = r.slot_start[f]; q < r.slot_start[f + 1]; q++) {
        const int s = r.slot_list[q];
        float4* lv = reinterpret_cast<float4*>(r.leaf_v) + 3 * (size_t)s;
        lv[0] = v0;
        lv[1] = s1;
        lv[2] = s2;
        r.slot_dirty[s] = 1;
    }
}

// mcpt_scene_set_visible (include/mcpt.h): one thread per facet of the range, from tri_v (three
// consecutive float4 per lane).  A facet whose byte already says `hide` is left alone.  A hidden facet's slots hold its
// first vertex three times (both triangle tests reject a zero determinant exactly), a visible one's its vertices; the
// facet id bits stay in the first .w.  k_refit_level then shrinks or regrows the boxes from the slots as they are.
__global__ __launch_bounds__(kRefitBlock) void k_visibility_scatter(RefitDev r, int first, int count, int hide) {
    const int i = blockIdx.x * kRefitBlock + (int)threadIdx.x;
    if (i >= count) return;
    const int f = first + i;
    if ((r.hidden[f] != 0) == (hide != 0)) return;
    r.hidden[f] = hide ? 1 : 0;
    const float4* tv = reinterpret_cast<const float4*>(r.tri_v) + 3 * (size_t)f;
    float4 v0 = tv[0];
    float4 v1 = tv[1], v2 = tv[2];
    v0.w = 0.0f, v1.w = 0.0f, v2.w = 0.0f;
    if (hide) v1 = v0, v2 = v0;
    v0.w = __int_as_float(f);
    for (int q = r.slot_start[f]; q < r.slot_start[f + 1]; q++) {
        const int s = r.slot_list[q];
        float4* lv = reinterpret_cast<float4*>(r.leaf_v) + 3 * (size_t)s;
        lv[0] = v0;
        lv[1] = v1;
        lv[2] = v2;
        r.slot_dirty[s] = 1;
    }
}

// mcpt_scene_transform (include/mcpt.h): 168 bytes passed by value, so the matrices sit in SGPRs
struct TransformArgs {
    double m[12], n[9];
};

// One thread per facet of the range.  The rest vertices are three float4 per lane (consecutive lanes, consecutive
// 48-byte records); the rest normals and both outputs (count * 9 floats each, the layout k_refit_scatter reads) go
// through one LDS buffer at stride 9 (odd: no bank conflict) so that every global access has consecutive lanes on
// consecutive dwords.  The 18 dot products are the header's rule: fp64, no contraction, the written order.  Offending
// values (k_refit_validate's terms) are counted with one integer atomic per wave that has any; nothing else is shared
// between blocks, and nothing of the scene is written.
__global__ __launch_bounds__(kRefitBlock) void k_transform_range(const float* __restrict__ rest_v, const float* __restrict__ rest_n,
                                                                 int first, int count, TransformArgs t, Arena ar,
                                                                 float* __restrict__ out_pos, float* __restrict__ out_nrm,
                                                                 unsigned* bad) {
    __shared__ float sp[9 * kRefitBlock];
    const int base = blockIdx.x * kRefitBlock;
    const int nb = min(kRefitBlock, count - base);
    const size_t off = 9 * (size_t)base;
    const bool live = (int)threadIdx.x < nb;
    float* mine = sp + 9 * threadIdx.x;
    unsigned nbad = 0;
    {
        const float* in = rest_n + 9 * (size_t)(first + base);
        for (int i = threadIdx.x; i < 9 * nb; i += kRefitBlock) sp[i] = in[i];
    }
    __syncthreads();
    if (live) {
        float o[9];
#pragma unroll
        for (int v = 0; v < 3; v++) {
            const double x = mine[3 * v], y = mine[3 * v + 1], z = mine[3 * v + 2];
#pragma unroll
            for (int r = 0; r < 3; r++) {
                o[3 * v + r] = (float)((t.n[3 * r] * x + t.n[3 * r + 1] * y) + t.n[3 * r + 2] * z);
                nbad += !isfinite(o[3 * v + r]);
            }
        }
#pragma unroll
        for (int i = 0; i < 9; i++) mine[i] = o[i];  // the thread's own nine words
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 9 * nb; i += kRefitBlock) out_nrm[off + i] = sp[i];
    __syncthreads();
    if (live) {
        const float4* rv = reinterpret_cast<const float4*>(rest_v) + 3 * (size_t)(first + base + (int)threadIdx.x);
#pragma unroll
        for (int v = 0; v < 3; v++) {
            const float4 p = rv[v];
            const double x = p.x, y = p.y, z = p.z;
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const float q = (float)(((t.m[4 * r] * x + t.m[4 * r + 1] * y) + t.m[4 * r + 2] * z) + t.m[4 * r + 3]);
                nbad += !isfinite(q) || (double)q < ar.lo[r] || (double)q > ar.hi[r];
                mine[3 * v + r] = q;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 9 * nb; i += kRefitBlock) out_pos[off + i] = sp[i];
    // every lane of the block is still here: the ballot sees whole waves; only a refused call goes further
    if (__ballot(nbad != 0) == 0) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) nbad += __shfl_xor(nbad, d);
    if ((threadIdx.x & 63) == 0) atomicAdd(bad, nbad);
}

// quantize_bvh4's rule for one axis of one node: org = the used children's minimum, then the smallest power-of-two
// scale for which every byte plane decodes outward by the traversal's exact fmaf (node_tplanes in render.hip)
__device__ inline void requantise_axis(const float4& lo, const float4& hi, const bool (&used)[4], float* org, unsigned* bexp,
                                       unsigned* qlo_out, unsigned* qhi_out) {
    float olo = FLT_MAX, ohi = -FLT_MAX;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (used[k]) {
            olo = fminf(olo, comp(lo, k));
            ohi = fmaxf(ohi, comp(hi, k));
        }
    if (olo > ohi) olo = ohi = 0.0f;
    const double ext = (double)ohi - (double)olo;
    // ilogb is floor(log2): never above the host's ceil(log2) start, so the first scale that passes is the same
    int b = ext > 0 ? max(1, min(254, ilogb(ext / 255.0) + 127 - 1)) : 1;
    unsigned qlo = 0, qhi = 0;
    for (;; b++) {
        if (b > 254) b = 254;
        const float sc = __uint_as_float((unsigned)b << 23);
        const double scale = (double)sc;
        bool ok = fmaf(255.0f, sc, olo) >= ohi || b == 254;
        qlo = qhi = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (!ok) continue;
            if (!used[k]) {
                qlo |= 255u << (8 * k);  // empty slot: lo > hi
                continue;
            }
            const float nlo = comp(lo, k), nhi = comp(hi, k);
            int ql = (int)fmin(fmax(floor(((double)nlo - (double)olo) / scale), 0.0), 255.0);
            while (ql > 0 && fmaf((float)ql, sc, olo) > nlo) ql--;
            int qh = (int)fmin(fmax(ceil(((double)nhi - (double)olo) / scale), 0.0), 255.0);
            while (qh < 255 && fmaf((float)qh, sc, olo) < nhi) qh++;
            if (fmaf((float)ql, sc, olo) > nlo || fmaf((float)qh, sc, olo) < nhi) {
                ok = false;  // needs a coarser scale
            } else {
                qlo |= (unsigned)ql << (8 * k);
                qhi |= (unsigned)qh << (8 * k);
            }
        }
        if (ok || b == 254) break;
    }
    *org = olo;
    *bexp = (unsigned)b;
    *qlo_out = qlo;
    *qhi_out = qhi;
}

__global__ __launch_bounds__(kRefitBlock) void k_refit_level(RefitDev r, int n0, int n1, double margin) {
    const int ni = n0 + (int)(blockIdx.x * kRefitBlock + threadIdx.x);
    const bool valid = ni < n1;
    BvhNode4* nd = r.bvh4 + (valid ? ni : n0);
    const int4 ch = *reinterpret_cast<const int4*>(nd->child);
    const float4* leafv = reinterpret_cast<const float4*>(r.leaf_v);
    bool dirty[4];
    float blo[4][3], bhi[4][3];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = comp(ch, k);
        dirty[k] = false;
#pragma unroll
        for (int a = 0; a < 3; a++) blo[k][a] = FLT_MAX, bhi[k][a] = -FLT_MAX;
        if (!valid || c == kBvh4Empty) continue;
        if (c < 0) {
            const int code = ~c, s0 = code >> kBvh4LeafBits, cnt = code & ((1 << kBvh4LeafBits) - 1);
            bool any = false;
            for (int j = 0; j < cnt; j++) any = any || r.slot_dirty[s0 + j] != 0;
            if (!any) continue;
            float l[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, h[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
            for (int j = 0; j < 3 * cnt; j++) {
                const float4 p = leafv[3 * (size_t)s0 + j];
                l[0] = fminf(l[0], p.x), l[1] = fminf(l[1], p.y), l[2] = fminf(l[2], p.z);
                h[0] = fmaxf(h[0], p.x), h[1] = fmaxf(h[1], p.y), h[2] = fmaxf(h[2], p.z);
            }
#pragma unroll
            for (int a = 0; a < 3; a++) {  // Builder::to_float_box
                blo[k][a] = next_down((float)((double)l[a] - margin));
                bhi[k][a] = next_up((float)((double)h[a] + margin));
            }
            dirty[k] = true;
        } else if (r.node_dirty[c]) {
            // unused slots hold (FLT_MAX, -FLT_MAX): neutral in the union
            const BvhNode4* cn = r.bvh4 + c;
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const float4 L = *reinterpret_cast<const float4*>(cn->lo[a]);
                const float4 H = *reinterpret_cast<const float4*>(cn->hi[a]);
                blo[k][a] = fminf(fminf(L.x, L.y), fminf(L.z, L.w));
                bhi[k][a] = fmaxf(fmaxf(H.x, H.y), fmaxf(H.z, H.w));
            }
            dirty[k] = true;
        }
    }
    const bool changed = dirty[0] || dirty[1] || dirty[2] || dirty[3];
    const unsigned long long m = __ballot(changed);
    if (m == 0) return;
    if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(r.counters + 1, (unsigned)__popcll(m));
    if (!changed) return;
    float4 lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = *reinterpret_cast<const float4*>(nd->lo[a]);
        hi[a] = *reinterpret_cast<const float4*>(nd->hi[a]);
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (dirty[k]) {
                set_comp(lo[a], k, blo[k][a]);
                set_comp(hi[a], k, bhi[k][a]);
            }
        *reinterpret_cast<float4*>(nd->lo[a]) = lo[a];
        *reinterpret_cast<float4*>(nd->hi[a]) = hi[a];
    }
    r.node_dirty[ni] = 1;
    bool used[4];
#pragma unroll
    for (int k = 0; k < 4; k++) used[k] = comp(ch, k) != kBvh4Empty && comp(lo[0], k) <= comp(hi[0], k);
    float org[3];
    unsigned ex = 0, q[6];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        unsigned b;
        requantise_axis(lo[a], hi[a], used, &org[a], &b, &q[2 * a], &q[2 * a + 1]);
        ex |= b << (8 * a);
    }
    BvhNode4Q* qn = r.bvh4q + ni;  // org + ex, q[0..3], q[4..5]; pad and child stay
    *reinterpret_cast<float4*>(qn->org) = make_float4(org[0], org[1], org[2], __uint_as_float(ex));
    *reinterpret_cast<uint4*>(qn->q) = make_uint4(q[0], q[1], q[2], q[3]);
    *reinterpret_cast<uint2*>(qn->q + 4) = make_uint2(q[4], q[5]);
}

}  // namespace

int refit_validate_enqueue(const RefitDev& r, int32_t count, const float* dpos, const float* dnrm, const double lo[3],
                           const double hi[3], void* stream) {
    Arena ar;
    for (int a = 0; a < 3; a++) ar.lo[a] = lo[a], ar.hi[a] = hi[a];
    hipStream_t st = static_cast<hipStream_t>(stream);
    REFIT_HIP_OK(hipMemsetAsync(r.counters, 0, sizeof(unsigned), st));
    const int64_t n = 9 * (int64_t)count;
    hipLaunchKernelGGL(k_refit_validate, dim3((unsigned)((n + kRefitBlock - 1) / kRefitBlock)), dim3(kRefitBlock), 0, st, n, dpos,
                       dnrm, ar, r.counters);
    REFIT_HIP_OK(hipGetLastError());
    return MCPT_OK;
}

int transform_enqueue(const RefitDev& r, const float* rest_v, const float* rest_n, int32_t first, int32_t count,
                      const double m[12], const double n[9], const double lo[3], const double hi[3], float* out_pos,
                      float* out_nrm, void* stream) {
    if (first < 0 || count < 1 || (int64_t)first + count > r.F || !rest_v || !rest_n || !out_pos || !out_nrm) {
        set_error("transform: range or buffers do not match the device state");
        return MCPT_E_INVALID;
    }
    TransformArgs t;
    Arena ar;
    for (int i = 0; i < 12; i++) t.m[i] = m[i];
    for (int i = 0; i < 9; i++) t.n[i] = n[i];
    for (int a = 0; a < 3; a++) ar.lo[a] = lo[a], ar.hi[a] = hi[a];
    hipStream_t st = static_cast<hipStream_t>(stream);
    REFIT_HIP_OK(hipMemsetAsync(r.counters, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_transform_range, dim3((count + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, rest_v, rest_n,
                       first, count, t, ar, out_pos, out_nrm, r.counters);
    REFIT_HIP_OK(hipGetLastError());
    return MCPT_OK;
}

int refit_enqueue(const RefitDev& r, const int32_t* level_first, int nlevels, int32_t first, int32_t count, const float* dpos,
                  const float* dnrm, double margin, void* stream) {
    if (first < 0 || count < 1 || (int64_t)first + count > r.F || nlevels < 1 || level_first[0] != 0 ||
        level_first[nlevels] != r.nnodes) {
        set_error("refit: range or levels do not match the device state");
        return MCPT_E_INVALID;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_refit_scatter, dim3((count + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, r, first, count,
                       dpos, dnrm);
    return refit_levels_enqueue(r, level_first, nlevels, margin, stream);
}

int visibility_enqueue(const RefitDev& r, const int32_t* level_first, int nlevels, int32_t first, int32_t count, int32_t visible,
                       double margin, void* stream) {
    if (first < 0 || count < 1 || (int64_t)first + count > r.F || !r.hidden) {
        set_error("visibility: range or mask do not match the device state");
        return MCPT_E_INVALID;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_visibility_scatter, dim3((count + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, r, first, count,
                       visible ? 0 : 1);
    return refit_levels_enqueue(r, level_first, nlevels, margin, stream);
}

int refit_levels_enqueue(const RefitDev& r, const int32_t* level_first, int nlevels, double margin, void* stream) {
    if (nlevels < 1 || level_first[0] != 0 || level_first[nlevels] != r.nnodes) {
        set_error("refit: levels do not match the device state");
        return MCPT_E_INVALID;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    REFIT_HIP_OK(hipMemsetAsync(r.counters + 1, 0, sizeof(unsigned), st));
    for (int l = nlevels - 1; l >= 0; l--) {
        const int n0 = level_first[l], n1 = level_first[l + 1];
        if (n1 <= n0) continue;
        hipLaunchKernelGGL(k_refit_level, dim3((n1 - n0 + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, r, n0, n1,
                           margin);
    }
    REFIT_HIP_OK(hipGetLastError());
    REFIT_HIP_OK(hipMemsetAsync(r.slot_dirty, 0, (size_t)r.nslots, st));
    REFIT_HIP_OK(hipMemsetAsync(r.node_dirty, 0, (size_t)r.nnodes, st));
    return MCPT_OK;
}

}  // namespace mcpt
