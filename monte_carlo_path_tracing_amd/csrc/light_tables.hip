// Device side of a light move (mcpt_scene_set_lights_movable, include/mcpt.h): after refit.hip's
// scatter has written the new vertices and normals of a facet range into tri_v / tri_n, everything the light prep and
// the area sampling read of the range's light triangles is derived again on the device, by the host formulas of
// get_device_state (render.hip), unique_normal_of_facet and light_triangle_area (scene_io.cpp) restated operation for
// operation: fp64 + - * / and sqrt round as the host's and the file is built without contraction, so every table comes
// out bit for bit as a fresh device state's.
//
// Kernels, all on one stream:
//   k_light_validate     (before anything is modified) one thread per facet of the range, on the staged positions:
//                        counts the light triangles whose fp64 (b - a) x (c - a) has a zero or non-finite length;
//   k_light_records      one thread per facet of the range, light facets only: lt_v, lt_n, lt_pk, lt_d, lt_w, lt_f, its
//                        half of lt_pair, l_area; marks the light's chunk and group dirty;
//   k_light_chunks       one wave per dirty 64-light chunk, one lane per light: chunk_sph, chunk_sk and the chunk's
//                        scratch row (unrounded S, K, lo, hi); every reduction is a min or a max;
//   k_light_globals      one block over the rows: light_bound and the band constants into a small struct;
//   k_light_area_cum     one wave per dirty group: the running fp64 sum of l_area in table order, added serially
//                        (the order is part of the rule), staged through LDS in 64-entry tiles;
//   k_light_leaf_scatter one thread per facet of the range: the facet's slots of the light-only tree's leaf array
//                        from tri_v, and their dirty bytes (refit.hip's k_refit_level does the rest).
// No block waits on another; kernel boundaries on the stream are the only synchronisation.
//
// A re-light (mcpt_scene_set_light_radiance) reuses k_light_chunks and k_light_globals after its own
//   k_light_radiance_validate (device form, before anything is modified) one thread per component: negative or not finite;
//   k_light_radiance     one thread per light of the range: light_rad, light_sum, the radiance words of lt_n / lt_w /
//                        lt_f, a group's grp_sum at its first light; marks the chunk (and that group) dirty;
//   k_light_group_cum    one thread: the running fp64 sum of grp_sum in group order.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>

#include "mcpt.h"
#include "mcpt_internal.h"

namespace mcpt {

namespace {

#define LT_HIP_OK(x)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MCPT_E_DEVICE;                                                              \
        }                                                                                      \
    } while (0)

constexpr int kLtBlock = 256;
constexpr double kEps = 1e-8;  // MCPT_EPS (device_math.h): the threshold folded into LightPair::d

__device__ inline double norm3(const double* a) { return sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }
// scene_io.cpp's dot: r = 0; r += a0 b0; r += a1 b1; r += a2 b2
__device__ inline double dot3(const double* a, const double* b) {
    double r = 0;
    r += a[0] * b[0];
    r += a[1] * b[1];
    r += a[2] * b[2];
    return r;
}
__device__ inline void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// pos: the staged range (count * 9 floats); light: tri_light of the range's first facet on
__global__ __launch_bounds__(kLtBlock) void k_light_validate(int count, const float* __restrict__ pos,
                                                             const int32_t* __restrict__ light, unsigned* bad) {
    const int i = (int)(blockIdx.x * kLtBlock + threadIdx.x);
    if (i >= count || light[i] < 0) return;
    const float* p = pos + 9 * (size_t)i;
    double ba[3], ca[3], n[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        ba[q] = (double)p[3 + q] - (double)p[q];
        ca[q] = (double)p[6 + q] - (double)p[q];
    }
    cross3(ba, ca, n);
    const double l = norm3(n);
    if (!(l > 0) || !isfinite(l)) atomicAdd(bad, 1u);  // only a refused call gets here
}

__global__ __launch_bounds__(kLtBlock) void k_light_records(LightTabDev t, int first, int count) {
    const int i = (int)(blockIdx.x * kLtBlock + threadIdx.x);
    if (i >= count) return;
    const int f = first + i;
    const int l = t.tri_light[f];
    if (l < 0) return;
    const float4* tv = reinterpret_cast<const float4*>(t.tri_v) + 3 * (size_t)f;
    const float4 va = tv[0], vb = tv[1], vc = tv[2];
    const float* tn = t.tri_n + 9 * (size_t)f;
    // unique_normal_of_facet
    const double a[3] = {va.x, va.y, va.z}, b[3] = {vb.x, vb.y, vb.z}, c[3] = {vc.x, vc.y, vc.z};
    double nv[3][3], ba[3], ca[3], n[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double tt[3] = {tn[3 * k], tn[3 * k + 1], tn[3 * k + 2]};
        const double len = norm3(tt);
#pragma unroll
        for (int q = 0; q < 3; q++) nv[k][q] = tt[q] / len;
    }
#pragma unroll
    for (int q = 0; q < 3; q++) {
        ba[q] = b[q] - a[q];
        ca[q] = c[q] - a[q];
    }
    cross3(ba, ca, n);
    const double len = norm3(n);
    double un[3], nr[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        un[q] = n[q] / len;
        nr[q] = un[q] * -1;
    }
    const double w = dot3(un, nv[0]) + dot3(un, nv[1]) + dot3(un, nv[2]);
    const double wr = dot3(nr, nv[0]) + dot3(nr, nv[1]) + dot3(nr, nv[2]);
    if (!(w > wr)) {
#pragma unroll
        for (int q = 0; q < 3; q++) un[q] = nr[q];
    }
    const double lsum = t.light_sum[l];
    const float unf[3] = {(float)un[0], (float)un[1], (float)un[2]};
    // lt_v, lt_n, lt_pk, lt_d
    float4* lv = reinterpret_cast<float4*>(t.lt_v) + 3 * (size_t)l;
    lv[0] = make_float4(va.x, va.y, va.z, unf[0]);
    lv[1] = make_float4(vb.x, vb.y, vb.z, unf[1]);
    lv[2] = make_float4(vc.x, vc.y, vc.z, unf[2]);
    reinterpret_cast<double4*>(t.lt_n)[l] = make_double4(un[0], un[1], un[2], lsum);
    float4* pk = reinterpret_cast<float4*>(t.lt_pk) + 3 * (size_t)l;
    pk[0] = make_float4(va.x, vb.x, vc.x, unf[0]);
    pk[1] = make_float4(va.y, vb.y, vc.y, unf[1]);
    pk[2] = make_float4(va.z, vb.z, vc.z, unf[2]);
    const double nd = un[0] * va.x + un[1] * va.y + un[2] * va.z;
    t.lt_d[l] = (float)nd;
    // lt_w: p0, p1, p2 in fp64, then 2 sum
    double2* lw = reinterpret_cast<double2*>(t.lt_w) + 5 * (size_t)l;
    lw[0] = make_double2(va.x, va.y);
    lw[1] = make_double2(va.z, vb.x);
    lw[2] = make_double2(vb.y, vb.z);
    lw[3] = make_double2(vc.x, vc.y);
    lw[4] = make_double2(vc.z, 2.0 * lsum);
    // lt_f: the edges formed in fp64 and rounded once
    const float e1[3] = {(float)((double)vb.x - va.x), (float)((double)vb.y - va.y), (float)((double)vb.z - va.z)};
    const float e2[3] = {(float)((double)vc.x - va.x), (float)((double)vc.y - va.y), (float)((double)vc.z - va.z)};
    float4* lf = reinterpret_cast<float4*>(t.lt_f) + 4 * (size_t)l;
    lf[0] = make_float4(va.x, va.y, va.z, e1[0]);
    lf[1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
    lf[2] = make_float4(e2[2], (float)(2.0 * lsum), 0, 0);
    // the light's half of its 128-byte pair record (32 floats: nl[3] pairs, d pair, p[9] pairs, padding); the other
    // half's floats are another thread's or nobody's
    float* P = t.lt_pair + 32 * (size_t)(l >> 1);
    const int h = l & 1;
    P[h] = unf[0];
    P[2 + h] = unf[1];
    P[4 + h] = unf[2];
    P[6 + h] = (float)(nd + kEps);
    const float4 vv[3] = {va, vb, vc};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        P[8 + 2 * (3 * k) + h] = vv[k].x;
        P[8 + 2 * (3 * k + 1) + h] = vv[k].y;
        P[8 + 2 * (3 * k + 2) + h] = vv[k].z;
    }
    // light_triangle_area: n = (b - a) x (c - a), n = n * (1 / |n|), 0.5 * ((b - a) x (c - a)) . n
    {
        const double inv = 1.0 / len;
        const double m[3] = {n[0] * inv, n[1] * inv, n[2] * inv};
        double d = 0;
        d += n[0] * m[0];
        d += n[1] * m[1];
        d += n[2] * m[2];
        t.l_area[l] = 0.5 * d;
    }
    t.chunk_dirty[l >> 6] = 1;
    t.group_dirty[t.light_group[l]] = 1;
}

__device__ inline double wave_min(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d));
    return v;
}
__device__ inline double wave_max(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d));
    return v;
}

// one 64-thread block (one wave) per chunk; all != 0: every chunk (the state's first light move fills every row)
__global__ __launch_bounds__(64) void k_light_chunks(LightTabDev t, int all) {
    const int c = (int)blockIdx.x;
    if (!all && !t.chunk_dirty[c]) return;
    const int lane = (int)threadIdx.x;
    const int l = 64 * c + lane;
    const bool live = l < t.NL;
    float4 v[3] = {make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0), make_float4(0, 0, 0, 0)};
    if (live) {
        const float4* lv = reinterpret_cast<const float4*>(t.lt_v) + 3 * (size_t)l;
        v[0] = lv[0], v[1] = lv[1], v[2] = lv[2];
    }
    double lo[3], hi[3], ctr[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double mn = 1e300, mx = -1e300;
        if (live) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double p = a == 0 ? v[k].x : a == 1 ? v[k].y : v[k].z;
                mn = fmin(mn, p);
                mx = fmax(mx, p);
            }
        }
        lo[a] = wave_min(mn);
        hi[a] = wave_max(mx);
        // the centre as stored (float)
        ctr[a] = (double)(float)(0.5 * (lo[a] + hi[a]));
    }
    double R = 0, S = 0, K = 0;
    if (live) {
        const double ls = t.light_sum[l];
        double lmin = 1e300;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float4 p = v[k], q = v[(k + 1) % 3];
            const double dx = (double)p.x - ctr[0], dy = (double)p.y - ctr[1], dz = (double)p.z - ctr[2];
            R = fmax(R, sqrt(dx * dx + dy * dy + dz * dz));
            const double ex = (double)q.x - p.x, ey = (double)q.y - p.y, ez = (double)q.z - p.z;
            lmin = fmin(lmin, sqrt(ex * ex + ey * ey + ez * ez));
        }
        S = ls;
        K = lmin > 0 ? ls / lmin : 1e30;
    }
    R = wave_max(R);
    S = wave_max(S);
    K = wave_max(K);
    if (lane == 0) {
        reinterpret_cast<float4*>(t.chunk_sph)[c] =
            make_float4((float)ctr[0], (float)ctr[1], (float)ctr[2], (float)(R * (1 + 1e-6) + 1e-6));
        reinterpret_cast<float2*>(t.chunk_sk)[c] = make_float2((float)(S * (1 + 1e-6)), (float)fmin(K * (1 + 1e-6), 1e30));
        double* row = t.chunk_row + kLightRowWords * (size_t)c;
        row[0] = S;
        row[1] = K;
#pragma unroll
        for (int a = 0; a < 3; a++) row[2 + a] = lo[a], row[5 + a] = hi[a];
        if (!all) atomicAdd(t.counters + 2, 1u);
    }
}

__device__ inline double block_max(double v, double* sh) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
}

// one block: the scene-wide constants from the chunk rows and spheres, as get_device_state computes them
__global__ __launch_bounds__(kLtBlock) void k_light_globals(LightTabDev t) {
    __shared__ double sh[4];
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, smax = 0, kmax = 0;
    for (int c = (int)threadIdx.x; c < t.nchunks; c += kLtBlock) {
        const double* row = t.chunk_row + kLightRowWords * (size_t)c;
        smax = fmax(smax, row[0]);
        kmax = fmax(kmax, row[1]);
#pragma unroll
        for (int a = 0; a < 3; a++) lo[a] = fmin(lo[a], row[2 + a]), hi[a] = fmax(hi[a], row[5 + a]);
    }
    double ctr[3], bound = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = -block_max(-lo[a], sh);
        hi[a] = block_max(hi[a], sh);
        ctr[a] = 0.5 * (lo[a] + hi[a]);
        bound = fmax(bound, fmax(fabs(lo[a]), fabs(hi[a])));  // max |coordinate|: the vertices are floats, so this is one
    }
    smax = block_max(smax, sh);
    kmax = block_max(kmax, sh);
    double Rs = 0;
    for (int c = (int)threadIdx.x; c < t.nchunks; c += kLtBlock) {  // the scene sphere contains every chunk sphere
        const float4 s = reinterpret_cast<const float4*>(t.chunk_sph)[c];
        const double dx = s.x - ctr[0], dy = s.y - ctr[1], dz = s.z - ctr[2];
        Rs = fmax(Rs, sqrt(dx * dx + dy * dy + dz * dz) + s.w);
    }
    Rs = block_max(Rs, sh);
    if (threadIdx.x == 0) {
        LightGlobals g;
        for (int a = 0; a < 3; a++) g.band_ctr[a] = ctr[a];
        g.band_R = Rs * (1 + 1e-6) + 1e-6;
        g.band_S = smax * (1 + 1e-6);
        g.band_K = fmin(kmax * (1 + 1e-6), 1e30);
        g.light_bound = (float)bound;
        g.pad = 0;
        *t.globals = g;
    }
}

// one 64-thread block (one wave) per group
__global__ __launch_bounds__(64) void k_light_area_cum(LightTabDev t) {
    __shared__ double tile[64];
    const int g = (int)blockIdx.x;
    if (!t.group_dirty[g]) return;
    const int start = t.grp_range[2 * g], n = t.grp_range[2 * g + 1];
    const int lane = (int)threadIdx.x;
    double run = 0;  // lane 0's
    for (int base = 0; base < n; base += 64) {
        const int m = min(64, n - base);
        if (lane < m) tile[lane] = t.l_area[start + base + lane];
        __syncthreads();
        if (lane == 0)
            for (int j = 0; j < m; j++) {
                run += tile[j];
                tile[j] = run;
            }
        __syncthreads();
        if (lane < m) t.l_area_cum[start + base + lane] = tile[lane];
        __syncthreads();
    }
    if (lane == 0) atomicAdd(t.counters + 3, 1u);
}

__global__ __launch_bounds__(kLtBlock) void k_light_leaf_scatter(RefitDev r, int first, int count, const int32_t* __restrict__ tri_light) {
    const int i = (int)(blockIdx.x * kLtBlock + threadIdx.x);
    if (i >= count) return;
    const int f = first + i;
    if (tri_light[f] < 0) return;
    const float4* tv = reinterpret_cast<const float4*>(r.tri_v) + 3 * (size_t)f;
    float4 v0 = tv[0];
    const float4 v1 = tv[1], v2 = tv[2];
    v0.w = __int_as_float(f);  // the facet id bits of the slot's first vertex
    for (int q = r.slot_start[f]; q < r.slot_start[f + 1]; q++) {
        const int s = r.slot_list[q];
        float4* lv = reinterpret_cast<float4*>(r.leaf_v) + 3 * (size_t)s;
        lv[0] = v0;
        lv[1] = make_float4(v1.x, v1.y, v1.z, 0.0f);
        lv[2] = make_float4(v2.x, v2.y, v2.z, 0.0f);
        r.slot_dirty[s] = 1;
    }
}

// ---- a re-light (mcpt_scene_set_light_radiance) ----

// one thread per value of the staged radiances: negative or not finite (a NaN fails v >= 0)
__global__ __launch_bounds__(kLtBlock) void k_light_radiance_validate(int64_t n, const double* __restrict__ rgb, unsigned* bad) {
    const int64_t i = (int64_t)blockIdx.x * kLtBlock + threadIdx.x;
    if (i >= n) return;
    const double v = rgb[i];
    if (!(v >= 0) || !isfinite(v)) atomicAdd(bad, 1u);  // only a refused call gets here
}

// one thread per light of the range: everything mcpt_scene_create derives from the radiance of ONE light, by its
// formulas (the sum is (r + g) + b).  The chunk's (S, K) and the constants follow in k_light_chunks / k_light_globals,
// grp_cum in k_light_group_cum.  Geometry words, pair records, padding and sentinel records are not touched.
__global__ __launch_bounds__(kLtBlock) void k_light_radiance(LightTabDev t, int first, int count, const double* __restrict__ rgb) {
    const int i = (int)(blockIdx.x * kLtBlock + threadIdx.x);
    if (i >= count) return;
    const int l = first + i;
    const double r = rgb[3 * (size_t)i], g = rgb[3 * (size_t)i + 1], b = rgb[3 * (size_t)i + 2];
    const double lsum = r + g + b;
    t.light_rad[3 * (size_t)l] = r;
    t.light_rad[3 * (size_t)l + 1] = g;
    t.light_rad[3 * (size_t)l + 2] = b;
    t.light_sum[l] = lsum;
    t.lt_n[4 * (size_t)l + 3] = lsum;                          // double4 .w
    t.lt_w[2 * (5 * (size_t)l + 4) + 1] = 2.0 * lsum;          // double2 [5l + 4].y
    t.lt_f[4 * (4 * (size_t)l + 2) + 1] = (float)(2.0 * lsum);  // float4 [4l + 2].y
    t.chunk_dirty[l >> 6] = 1;
    const int grp = t.light_group[l];
    if (t.grp_range[2 * grp] == l) {  // a group's sum is its first light's, as create takes it
        t.grp_sum[grp] = lsum;
        t.group_dirty[grp] = 1;
    }
}

// grp_cum: the running fp64 sum of grp_sum in group order, added serially by one thread (the order is part of the
// rule, as for k_light_area_cum; a scene has a handful of groups)
__global__ __launch_bounds__(64) void k_light_group_cum(LightTabDev t) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double run = 0;
    for (int g = 0; g < t.ngroups; g++) {
        run += t.grp_sum[g];
        t.grp_cum[g] = run;
    }
}

}  // namespace

int light_radiance_validate_enqueue(int64_t n, const double* drgb, unsigned* bad, void* stream) {
    if (n < 1 || !drgb || !bad) {
        set_error("light tables: bad validation arguments");
        return MCPT_E_INVALID;
    }
    hipLaunchKernelGGL(k_light_radiance_validate, dim3((unsigned)((n + kLtBlock - 1) / kLtBlock)), dim3(kLtBlock), 0,
                       static_cast<hipStream_t>(stream), n, drgb, bad);
    LT_HIP_OK(hipGetLastError());
    return MCPT_OK;
}

int light_radiance_enqueue(const LightTabDev& t, int32_t first, int32_t count, const double* drgb, bool groups, void* stream) {
    if (first < 0 || count < 1 || (int64_t)first + count > t.NL || t.nchunks != (t.NL + 63) / 64 || t.ngroups < 1 || !drgb ||
        !t.light_rad || !t.grp_sum || !t.grp_cum) {
        set_error("light tables: range or tables do not match the device state");
        return MCPT_E_INVALID;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_light_radiance, dim3((count + kLtBlock - 1) / kLtBlock), dim3(kLtBlock), 0, st, t, first, count, drgb);
    hipLaunchKernelGGL(k_light_chunks, dim3(t.nchunks), dim3(64), 0, st, t, 0);
    hipLaunchKernelGGL(k_light_globals, dim3(1), dim3(kLtBlock), 0, st, t);
    if (groups) hipLaunchKernelGGL(k_light_group_cum, dim3(1), dim3(64), 0, st, t);
    LT_HIP_OK(hipGetLastError());
    LT_HIP_OK(hipMemsetAsync(t.chunk_dirty, 0, (size_t)t.nchunks, st));
    LT_HIP_OK(hipMemsetAsync(t.group_dirty, 0, (size_t)t.ngroups, st));
    return MCPT_OK;
}

int light_validate_enqueue(int32_t count, const float* dpos, const int32_t* tri_light_of_range, unsigned* bad, void* stream) {
    if (count < 1 || !dpos || !tri_light_of_range || !bad) {
        set_error("light tables: bad validation arguments");
        return MCPT_E_INVALID;
    }
    hipLaunchKernelGGL(k_light_validate, dim3((count + kLtBlock - 1) / kLtBlock), dim3(kLtBlock), 0, static_cast<hipStream_t>(stream),
                       count, dpos, tri_light_of_range, bad);
    LT_HIP_OK(hipGetLastError());
    return MCPT_OK;
}

int light_chunks_all_enqueue(const LightTabDev& t, void* stream) {
    if (t.NL < 1 || t.nchunks != (t.NL + 63) / 64) {
        set_error("light tables: the chunk count does not match the light table");
        return MCPT_E_INVALID;
    }
    hipLaunchKernelGGL(k_light_chunks, dim3(t.nchunks), dim3(64), 0, static_cast<hipStream_t>(stream), t, 1);
    LT_HIP_OK(hipGetLastError());
    return MCPT_OK;
}

int light_area_cum_enqueue(const LightTabDev& t, void* stream) {
    if (t.ngroups < 1) return MCPT_OK;
    hipLaunchKernelGGL(k_light_area_cum, dim3(t.ngroups), dim3(64), 0, static_cast<hipStream_t>(stream), t);
    LT_HIP_OK(hipGetLastError());
    return MCPT_OK;
}

int light_tables_enqueue(const LightTabDev& t, const RefitDev& lr, const int32_t* level_first, int nlevels, int32_t first,
                         int32_t count, double margin, void* stream) {
    if (first < 0 || count < 1 || (int64_t)first + count > t.F || t.NL < 1 || t.nchunks != (t.NL + 63) / 64 || t.ngroups < 1 ||
        lr.F != t.F) {
        set_error("light tables: range or tables do not match the device state");
        return MCPT_E_INVALID;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((count + kLtBlock - 1) / kLtBlock), block(kLtBlock);
    LT_HIP_OK(hipMemsetAsync(t.counters + 2, 0, 2 * sizeof(unsigned), st));
    hipLaunchKernelGGL(k_light_records, grid, block, 0, st, t, first, count);
    hipLaunchKernelGGL(k_light_chunks, dim3(t.nchunks), dim3(64), 0, st, t, 0);
    hipLaunchKernelGGL(k_light_globals, dim3(1), block, 0, st, t);
    hipLaunchKernelGGL(k_light_area_cum, dim3(t.ngroups), dim3(64), 0, st, t);
    hipLaunchKernelGGL(k_light_leaf_scatter, grid, block, 0, st, lr, first, count, t.tri_light);
    LT_HIP_OK(hipGetLastError());
    LT_HIP_OK(hipMemsetAsync(t.chunk_dirty, 0, (size_t)t.nchunks, st));
    LT_HIP_OK(hipMemsetAsync(t.group_dirty, 0, (size_t)t.ngroups, st));
    return refit_levels_enqueue(lr, level_first, nlevels, margin, stream);
}

}  // namespace mcpt
