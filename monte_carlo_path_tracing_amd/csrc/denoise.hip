// Variance-guided edge-avoiding a-trous filter for gfx950 (mcpt_denoise, include/mcpt.h states the rule in
// full) and the host helper mcpt_variance_from_noise.  No counterpart in the reference.
//
//   k_spatial_variance  lane per pixel : V_0 when the caller supplies none (two passes over the clipped 5x5)
//   k_atrous            lane per pixel : one iteration at step s (25 taps, fully unrolled, h as constants)
//
// Everything is fp64, with exp / pow / sqrt from the device library and -ffp-contract=off, so a numpy
// restatement of the rule reproduces the output to rounding (tests/test_denoise.py).  A block is 64 x 4
// pixels: a wave covers 64 consecutive x of one row, so every tap's loads are consecutive across the wave.
// The centre pixel's guides stay in registers; a tap whose hit / miss state differs from the centre's is
// skipped before its pow and exps.  Colour and variance ping-pong between two library buffers; the last
// iteration writes the caller's outputs.  All reads are direct global loads: at 800 x 600 the guides (10
// doubles per pixel) and colour + variance (4) are 54 MB and stay in L2 / Infinity Cache
// (profiles/denoise_benches.txt holds the A/B against the layouts that were tried).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "mcpt.h"
#include "mcpt_internal.h"

using mcpt::set_error;

namespace {

#define DN_HIP_OK(x)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MCPT_E_DEVICE;                                                              \
        }                                                                                      \
    } while (0)

constexpr int kBx = 64, kBy = 4;  // a wave = 64 consecutive x of one row
constexpr double kEps = 1e-10;

struct DnParams {
    int W, H;
    double sigma_color, sigma_normal, sigma_plane, sigma_albedo;
    const double *albedo, *normal, *position, *depth;  // the guides
};

__device__ constexpr double h5(int d) {  // h(d), d in [-2, 2]
    return d == 0 ? 3.0 / 8 : (d == 1 || d == -1) ? 1.0 / 4 : 1.0 / 16;
}
__device__ constexpr double g3(int d) { return d == 0 ? 1.0 / 2 : 1.0 / 4; }

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
__global__ __launch_bounds__(kBx* kBy) void k_spatial_variance(DnParams P, const double* C, double* V) {
    const int x = blockIdx.x * kBx + threadIdx.x, y = blockIdx.y * kBy + threadIdx.y;
    if (x >= P.W || y >= P.H) return;
    const size_t p = (size_t)y * P.W + x;
    const Centre c = centre_of(P, p);
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
    V[p] = sv / su;
}

// one iteration at step s: (Cin, Vin) -> (Cout, Vout)
__global__ __launch_bounds__(kBx* kBy) void k_atrous(DnParams P, const double* Cin, const double* Vin, double* Cout,
                                                     double* Vout, int s) {
    const int x = blockIdx.x * kBx + threadIdx.x, y = blockIdx.y * kBy + threadIdx.y;
    if (x >= P.W || y >= P.H) return;
    const size_t p = (size_t)y * P.W + x;
    const Centre c = centre_of(P, p);
    const double lp = lum(Cin, p);
    double gv = 0.0, gw = 0.0;  // Vg: the clipped, renormalised 3x3 Gaussian of Vin
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int qx = x + dx, qy = y + dy;
            if (qx < 0 || qx >= P.W || qy < 0 || qy >= P.H) continue;
            const double g = g3(dy) * g3(dx);
            gv += g * Vin[(size_t)qy * P.W + qx];
            gw += g;
        }
    const double sigma = P.sigma_color * sqrt(fmax(gv / gw, 0.0)) + kEps;
    double sw = 0.0, sv = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++)
#pragma unroll
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + s * dx, qy = y + s * dy;
            if (qx < 0 || qx >= P.W || qy < 0 || qy >= P.H) continue;
            const size_t q = (size_t)qy * P.W + qx;
            const double g = geo(P, c, q);
            if (g == 0.0) continue;
            const double q0 = Cin[3 * q], q1 = Cin[3 * q + 1], q2 = Cin[3 * q + 2];
            const double lq = (q0 + q1 + q2) / 3.0;
            const double w = h5(dy) * h5(dx) * g * exp(-fabs(lp - lq) / sigma);
            s0 += w * q0;
            s1 += w * q1;
            s2 += w * q2;
            sv += w * w * Vin[q];
            sw += w;
        }
    Cout[3 * p] = s0 / sw;
    Cout[3 * p + 1] = s1 / sw;
    Cout[3 * p + 2] = s2 / sw;
    Vout[p] = sv / (sw * sw);
}

// every check a call makes before it touches a device
int check_call(const mcpt_denoise_opts* o, int W, int H, const double* color, const double* variance,
               const mcpt_aov_buffers* g, const double* out, const double* out_variance) {
    if (!o) {
        set_error("null mcpt_denoise_opts");
        return MCPT_E_INVALID;
    }
    if (o->struct_size != sizeof(mcpt_denoise_opts)) {
        set_error("mcpt_denoise_opts.struct_size is %u, this library expects %zu (use mcpt_denoise_opts_init / the "
                  "mcpt.h of MCPT_VERSION %d)", o->struct_size, sizeof(mcpt_denoise_opts), MCPT_VERSION);
        return MCPT_E_INVALID;
    }
    if (o->iterations < 1 || o->iterations > 8) {
        set_error("invalid denoise options: iterations %d is outside 1..8", o->iterations);
        return MCPT_E_INVALID;
    }
    const struct {
        const char* name;
        double v;
    } sig[] = {{"sigma_color", o->sigma_color}, {"sigma_normal", o->sigma_normal}, {"sigma_plane", o->sigma_plane},
               {"sigma_albedo", o->sigma_albedo}};
    for (const auto& s : sig)
        if (!std::isfinite(s.v) || !(s.v > 0)) {
            set_error("invalid denoise options: %s %g must be finite and > 0", s.name, s.v);
            return MCPT_E_INVALID;
        }
    if (W < 1 || H < 1 || (long long)W * H > (1ll << 28)) {
        set_error("invalid frame size: width %d, height %d", W, H);
        return MCPT_E_INVALID;
    }
    if (!color || !out) {
        set_error("null argument: %s", !color ? "color" : "out");
        return MCPT_E_INVALID;
    }
    if (!g || !g->albedo || !g->normal || !g->position || !g->depth) {
        set_error("null argument: guides (%s); all four guide arrays are required",
                  !g ? "the struct" : !g->albedo ? "albedo" : !g->normal ? "normal" : !g->position ? "position" : "depth");
        return MCPT_E_INVALID;
    }
    // an output overlapping an input would be read by neighbouring pixels after it is written
    const size_t npx = (size_t)W * H;
    const struct {
        const char* name;
        const double* p;
        size_t n;
    } ins[] = {{"color", color, 3 * npx},         {"variance", variance, npx},        {"guides.albedo", g->albedo, 3 * npx},
               {"guides.normal", g->normal, 3 * npx}, {"guides.position", g->position, 3 * npx}, {"guides.depth", g->depth, npx}},
      outs[] = {{"out", out, 3 * npx}, {"out_variance", out_variance, npx}};
    for (const auto& w : outs)
        for (const auto& r : ins)
            if (w.p && r.p && (uintptr_t)w.p < (uintptr_t)(r.p + r.n) && (uintptr_t)r.p < (uintptr_t)(w.p + w.n)) {
                set_error("%s is aliasing %s: the filter cannot run in place", w.name, r.name);
                return MCPT_E_INVALID;
            }
    if (out_variance && (uintptr_t)out < (uintptr_t)(out_variance + npx) && (uintptr_t)out_variance < (uintptr_t)(out + 3 * npx)) {
        set_error("out is aliasing out_variance");
        return MCPT_E_INVALID;
    }
    return MCPT_OK;
}

int check_device_array(const void* p, int device, const char* name) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        set_error("%s is not device memory (unknown to the HIP runtime)", name);
        return MCPT_E_INVALID;
    }
    if (a.type != hipMemoryTypeDevice || a.device != device) {
        set_error("%s is not device memory of device %d (memory type %d, device %d)", name, device, (int)a.type, a.device);
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

int select_device(int device, Scratch& S, int* used) {
    int cur = 0;
    DN_HIP_OK(hipGetDevice(&cur));
    *used = device < 0 ? cur : device;
    if (*used != cur) {
        int nd = 0;
        DN_HIP_OK(hipGetDeviceCount(&nd));
        if (*used >= nd) {
            set_error("device %d: no such device (%d visible)", *used, nd);
            return MCPT_E_INVALID;
        }
        DN_HIP_OK(hipSetDevice(*used));
        S.restore = cur;
    }
    return MCPT_OK;
}

// the filter over device arrays; tmp holds 8 npx doubles (two colour + variance buffers)
int run_filter(const mcpt_denoise_opts* o, int W, int H, const double* dC, const double* dV, const mcpt_aov_buffers* g,
               double* dOut, double* dOutV, double* tmp, Scratch& S, double* seconds) {
    const size_t npx = (size_t)W * H;
    double* bufC[2] = {tmp, tmp + 3 * npx};
    double* bufV[2] = {tmp + 6 * npx, tmp + 7 * npx};
    const DnParams P{W, H, o->sigma_color, o->sigma_normal, o->sigma_plane, o->sigma_albedo, g->albedo, g->normal, g->position, g->depth};
    const dim3 grid((W + kBx - 1) / kBx, (H + kBy - 1) / kBy), block(kBx, kBy);
    const int K = o->iterations;
    DN_HIP_OK(hipEventCreate(&S.e0));
    DN_HIP_OK(hipEventCreate(&S.e1));
    DN_HIP_OK(hipEventRecord(S.e0, nullptr));
    const double *srcC = dC, *srcV = dV;
    if (!srcV) {  // iteration 0 writes buffer 0, so the estimate goes to buffer 1
        hipLaunchKernelGGL(k_spatial_variance, grid, block, 0, nullptr, P, dC, bufV[1]);
        DN_HIP_OK(hipGetLastError());
        srcV = bufV[1];
    }
    for (int i = 0; i < K; i++) {
        const bool last = i == K - 1;
        double* dstC = last ? dOut : bufC[i & 1];
        double* dstV = last && dOutV ? dOutV : bufV[i & 1];
        hipLaunchKernelGGL(k_atrous, grid, block, 0, nullptr, P, srcC, srcV, dstC, dstV, 1 << i);
        DN_HIP_OK(hipGetLastError());
        srcC = dstC, srcV = dstV;
    }
    DN_HIP_OK(hipEventRecord(S.e1, nullptr));
    DN_HIP_OK(hipEventSynchronize(S.e1));
    float ms = 0;
    DN_HIP_OK(hipEventElapsedTime(&ms, S.e0, S.e1));
    if (seconds) *seconds = ms * 1e-3;
    return MCPT_OK;
}

}  // namespace

extern "C" {

void mcpt_denoise_opts_init(mcpt_denoise_opts* o) {
    if (!o) return;
    std::memset((void*)o, 0, sizeof *o);
    o->struct_size = sizeof *o;
    o->iterations = 5;
    o->sigma_color = 4.0;
    o->sigma_normal = 128.0;
    o->sigma_plane = 0.01;
    o->sigma_albedo = 0.1;
    o->device = -1;
}

int mcpt_denoise_device(const mcpt_denoise_opts* o, int32_t W, int32_t H, const double* dC, const double* dV,
                        const mcpt_aov_buffers* g, double* dOut, double* dOutV, double* seconds) {
    int rc;
    if ((rc = check_call(o, W, H, dC, dV, g, dOut, dOutV))) return rc;
    Scratch S;
    int device;
    if ((rc = select_device(o->device, S, &device))) return rc;
    if ((rc = check_device_array(dC, device, "dev_color")) || (dV && (rc = check_device_array(dV, device, "dev_variance"))) ||
        (rc = check_device_array(g->albedo, device, "dev_guides.albedo")) ||
        (rc = check_device_array(g->normal, device, "dev_guides.normal")) ||
        (rc = check_device_array(g->position, device, "dev_guides.position")) ||
        (rc = check_device_array(g->depth, device, "dev_guides.depth")) || (rc = check_device_array(dOut, device, "dev_out")) ||
        (dOutV && (rc = check_device_array(dOutV, device, "dev_out_variance"))))
        return rc;
    const size_t npx = (size_t)W * H;
    DN_HIP_OK(hipMalloc(&S.p, 8 * npx * sizeof(double)));
    // the caller's arrays may still be written by work on other streams (e.g. torch's)
    DN_HIP_OK(hipDeviceSynchronize());
    return run_filter(o, W, H, dC, dV, g, dOut, dOutV, S.p, S, seconds);
}

int mcpt_denoise(const mcpt_denoise_opts* o, int32_t W, int32_t H, const double* color, const double* variance,
                 const mcpt_aov_buffers* g, double* out, double* out_variance, double* seconds) {
    int rc;
    if ((rc = check_call(o, W, H, color, variance, g, out, out_variance))) return rc;
    Scratch S;
    int device;
    if ((rc = select_device(o->device, S, &device))) return rc;
    const size_t npx = (size_t)W * H, B = sizeof(double);
    // colour 3, variance 1, guides 3 + 3 + 3 + 1, out 3, out variance 1, then the filter's 8
    DN_HIP_OK(hipMalloc(&S.p, 26 * npx * B));
    double* dC = S.p;
    double* dV = dC + 3 * npx;
    const mcpt_aov_buffers dg{dV + npx, dV + 4 * npx, dV + 7 * npx, dV + 10 * npx};
    double* dOut = dg.depth + npx;
    double* dOutV = dOut + 3 * npx;
    DN_HIP_OK(hipMemcpy(dC, color, 3 * npx * B, hipMemcpyHostToDevice));
    if (variance) DN_HIP_OK(hipMemcpy(dV, variance, npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dg.albedo, g->albedo, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dg.normal, g->normal, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dg.position, g->position, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dg.depth, g->depth, npx * B, hipMemcpyHostToDevice));
    if ((rc = run_filter(o, W, H, dC, variance ? dV : nullptr, &dg, dOut, dOutV, dOutV + npx, S, seconds))) return rc;
    DN_HIP_OK(hipMemcpy(out, dOut, 3 * npx * B, hipMemcpyDeviceToHost));
    if (out_variance) DN_HIP_OK(hipMemcpy(out_variance, dOutV, npx * B, hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_variance_from_noise(int32_t W, int32_t H, const double* rgb, const double* noise, double* variance) {
    if (W < 1 || H < 1 || !rgb || !noise || !variance) {
        set_error("mcpt_variance_from_noise: null argument or invalid frame size (width %d, height %d)", W, H);
        return MCPT_E_INVALID;
    }
    const size_t npx = (size_t)W * H;
    for (size_t p = 0; p < npx; p++) {
        const double s = rgb[3 * p] + rgb[3 * p + 1] + rgb[3 * p + 2];
        const double d = s > 0 ? noise[p] * std::sqrt(s) / 3.0 : 0.0;
        variance[p] = d * d;
    }
    return MCPT_OK;
}

}  // extern "C"
