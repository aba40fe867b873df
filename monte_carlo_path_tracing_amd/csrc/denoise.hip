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

#include "denoise_common.h"
#include "mcpt.h"
#include "mcpt_internal.h"

using mcpt::set_error;
using namespace mcpt_dn;

namespace {

constexpr double kEps = 1e-10;

__device__ constexpr double g3(int d) { return d == 0 ? 1.0 / 2 : 1.0 / 4; }

// V_0 where the caller supplies no variance: spatial_v0 of denoise_common.h (temporal.hip runs the same estimate)
__global__ __launch_bounds__(kBx* kBy) void k_spatial_variance(DnParams P, const double* C, double* V) {
    const int x = blockIdx.x * kBx + threadIdx.x, y = blockIdx.y * kBy + threadIdx.y;
    if (x >= P.W || y >= P.H) return;
    V[(size_t)y * P.W + x] = spatial_v0(P, C, x, y);
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

// the option struct's checks; mcpt::denoise_check_opts is this function
int check_opts(const mcpt_denoise_opts* o) {
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
    return MCPT_OK;
}

// every check a call makes before it touches a device
int check_call(const mcpt_denoise_opts* o, int W, int H, const double* color, const double* variance,
               const mcpt_aov_buffers* g, const double* out, const double* out_variance) {
    int orc;
    if ((orc = check_opts(o))) return orc;
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

// the filter over device arrays, enqueued on the null stream; tmp holds 8 npx doubles (two colour + variance buffers)
int enqueue_filter(const mcpt_denoise_opts* o, int W, int H, const double* dC, const double* dV, const mcpt_aov_buffers* g,
                   double* dOut, double* dOutV, double* tmp) {
    const size_t npx = (size_t)W * H;
    double* bufC[2] = {tmp, tmp + 3 * npx};
    double* bufV[2] = {tmp + 6 * npx, tmp + 7 * npx};
    const DnParams P{W, H, o->sigma_color, o->sigma_normal, o->sigma_plane, o->sigma_albedo, g->albedo, g->normal, g->position, g->depth};
    const dim3 grid((W + kBx - 1) / kBx, (H + kBy - 1) / kBy), block(kBx, kBy);
    const int K = o->iterations;
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
    return MCPT_OK;
}

// the same, timed with two events and waited for
int run_filter(const mcpt_denoise_opts* o, int W, int H, const double* dC, const double* dV, const mcpt_aov_buffers* g,
               double* dOut, double* dOutV, double* tmp, Scratch& S, double* seconds) {
    int rc;
    DN_HIP_OK(hipEventCreate(&S.e0));
    DN_HIP_OK(hipEventCreate(&S.e1));
    DN_HIP_OK(hipEventRecord(S.e0, nullptr));
    if ((rc = enqueue_filter(o, W, H, dC, dV, g, dOut, dOutV, tmp))) return rc;
    DN_HIP_OK(hipEventRecord(S.e1, nullptr));
    DN_HIP_OK(hipEventSynchronize(S.e1));
    float ms = 0;
    DN_HIP_OK(hipEventElapsedTime(&ms, S.e0, S.e1));
    if (seconds) *seconds = ms * 1e-3;
    return MCPT_OK;
}

}  // namespace

// mcpt_internal.h: the filter for a caller that owns every buffer (sequence.hip)
namespace mcpt {

int denoise_check_opts(const mcpt_denoise_opts* o) { return check_opts(o); }

int denoise_enqueue(const mcpt_denoise_opts* o, int32_t W, int32_t H, const double* dC, const double* dV,
                    const mcpt_aov_buffers* g, double* dOut, double* dOutV, double* tmp) {
    int rc;
    if ((rc = check_call(o, W, H, dC, dV, g, dOut, dOutV))) return rc;
    if (!tmp) {
        set_error("null argument: the filter's scratch");
        return MCPT_E_INVALID;
    }
    return enqueue_filter(o, W, H, dC, dV, g, dOut, dOutV, tmp);
}

}  // namespace mcpt

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
