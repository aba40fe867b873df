// What the a-trous filter (denoise.hip) and the temporal accumulation (temporal.hip) share: the block shape,
// the guides' parameter block, the centre pixel's registers, geo(p, q) and the spatial variance estimate V_0
// of include/mcpt.h (device code, fp64 with -ffp-contract=off), and the host helpers around a launch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "mcpt.h"
#include "mcpt_internal.h"

namespace mcpt_dn {

constexpr int kBx = 64, kBy = 4;  // a wave = 64 consecutive x of one row

struct DnParams {
    int W, H;
    double sigma_color, sigma_normal, sigma_plane, sigma_albedo;
    const double *albedo, *normal, *position, *depth;  // the guides
};

__device__ constexpr double h5(int d) {  // h(d), d in [-2, 2]
    return d == 0 ? 3.0 / 8 : (d == 1 || d == -1) ? 1.0 / 4 : 1.0 / 16;
}

struct Centre {  // the centre pixel's guides, in registers for all 25 taps
    bool hit;
    double N[3], X[3], rho[3], plane;  // plane = sigma_plane * depth_p
};

__device__ inline Centre centre_of(const DnParams& P, size_t p) {
    Centre c;
    const double depth = P.depth[p];
    c.hit = depth > 0;
    for (int k = 0; k < 3; k++) c.N[k] = P.normal[3 * p + k], c.X[k] = P.position[3 * p + k], c.rho[k] = P.albedo[3 * p + k];
    c.plane = P.sigma_plane * depth;
    return c;
}

// geo(p, q): 0 when exactly one of them hits (no pow, no exp), 1 when both miss, else w_n w_x w_a
__device__ inline double geo_of(const DnParams& P, const Centre& c, double depth_q, const double* Nq, const double* Xq,
                                const double* Rq) {
    const bool hq = depth_q > 0;
    if (hq != c.hit) return 0.0;
    if (!hq) return 1.0;
    const double nn = c.N[0] * Nq[0] + c.N[1] * Nq[1] + c.N[2] * Nq[2];
    const double pd = c.N[0] * (Xq[0] - c.X[0]) + c.N[1] * (Xq[1] - c.X[1]) + c.N[2] * (Xq[2] - c.X[2]);
    const double a0 = c.rho[0] - Rq[0], a1 = c.rho[1] - Rq[1], a2 = c.rho[2] - Rq[2];
    const double wn = pow(fmax(0.0, nn), P.sigma_normal);
    const double wx = exp(-fabs(pd) / c.plane);
    const double wa = exp(-(a0 * a0 + a1 * a1 + a2 * a2) / (P.sigma_albedo * P.sigma_albedo));
    return wn * wx * wa;
}
__device__ inline double geo(const DnParams& P, const Centre& c, size_t q) {
    return geo_of(P, c, P.depth[q], P.normal + 3 * q, P.position + 3 * q, P.albedo + 3 * q);
}

__device__ inline double lum(const double* C, size_t q) { return (C[3 * q] + C[3 * q + 1] + C[3 * q + 2]) / 3.0; }

// V_0(p) = sum u (l(q) - m)^2 / sum u over the clipped 5x5 at step 1, u = h h geo, m = sum u l / sum u
__device__ inline double spatial_v0(const DnParams& P, const double* C, int x, int y) {
    const Centre c = centre_of(P, (size_t)y * P.W + x);
    double u[25], l[25], su = 0.0, sl = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++)
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int k = 5 * (dy + 2) + dx + 2, qx = x + dx, qy = y + dy;
            u[k] = 0.0, l[k] = 0.0;
            if (qx < 0 || qx >= P.W || qy < 0 || qy >= P.H) continue;
            const size_t q = (size_t)qy * P.W + qx;
            const double g = geo(P, c, q);
            if (g == 0.0) continue;
            u[k] = h5(dy) * h5(dx) * g;
            l[k] = lum(C, q);
            su += u[k];
            sl += u[k] * l[k];
        }
    const double m = sl / su;
    double sv = 0.0;
#pragma unroll
    for (int k = 0; k < 25; k++) sv += u[k] * ((l[k] - m) * (l[k] - m));
    return sv / su;
}

// ---- host side: what both entry points need around their launches ----

#define DN_HIP_OK(x)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (x);                                                                         \
        if (e_ != hipSuccess) {                                                                      \
            mcpt::set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MCPT_E_DEVICE;                                                                    \
        }                                                                                            \
    } while (0)

inline int check_device_array(const void* p, int device, const char* name) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        mcpt::set_error("%s is not device memory (unknown to the HIP runtime)", name);
        return MCPT_E_INVALID;
    }
    if (a.type != hipMemoryTypeDevice || a.device != device) {
        mcpt::set_error("%s is not device memory of device %d (memory type %d, device %d)", name, device, (int)a.type, a.device);
        return MCPT_E_INVALID;
    }
    return MCPT_OK;
}

struct Scratch {  // one device allocation and two events, released on every return path
    double* p = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int restore = -1;  // the device that was current before the call
    ~Scratch() {
        if (p) (void)hipFree(p);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        if (restore >= 0) (void)hipSetDevice(restore);
    }
};

inline int select_device(int device, Scratch& S, int* used) {
    int cur = 0;
    DN_HIP_OK(hipGetDevice(&cur));
    *used = device < 0 ? cur : device;
    if (*used != cur) {
        int nd = 0;
        DN_HIP_OK(hipGetDeviceCount(&nd));
        if (*used >= nd) {
            mcpt::set_error("device %d: no such device (%d visible)", *used, nd);
            return MCPT_E_INVALID;
        }
        DN_HIP_OK(hipSetDevice(*used));
        S.restore = cur;
    }
    return MCPT_OK;
}

}  // namespace mcpt_dn
