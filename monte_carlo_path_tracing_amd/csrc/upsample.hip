// Guided (joint bilateral) upsampling for gfx950 (mcpt_upsample, include/mcpt.h states the rule in full; Kopf et al.
// 2007, "Joint Bilateral Upsampling") and the host helper mcpt_camera_scaled.  No counterpart in the reference.
//
//   k_upsample  lane per full-size pixel : the four low-size taps around the pixel's source point, each weighed by
//                                          its bilinear weight times geo(p, q) of the a-trous filter (centre: the
//                                          full-size guides at p, tap: the low-size guides at q); the containing low
//                                          pixel where the weights sum to less than min_weight, and those pixels
//                                          counted
//
// Everything is fp64 with -ffp-contract=off, so a numpy restatement of the rule reproduces the output to rounding
// (tests/test_upsample.py).  A block is 64 x 4 full-size pixels as in denoise.hip: a wave is 64 consecutive x of one
// row, so the centre's loads and the store are consecutive across the wave.  The taps are direct global loads: the
// lanes of a wave share them (at factor 2 a wave's row touches about 34 low pixels, each read by two to four lanes),
// so they come out of the vector L1 / L2.  A variant that staged the block's 34 x 4 low pixels in LDS was measured
// against this one and lost at factor 2 (profiles/upsample_benches.txt).  The fallback count is an integer:
// a wave counts its lanes with a ballot and issues one 64-bit integer atomic, so the count is exact and no
// floating-point atomic is involved.
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

struct UpLow {  // the low-size frame: colour and guides
    int w, h, f;
    double min_weight;
    const double *color, *albedo, *normal, *position, *depth;
};

// P: the full-size guides (P.W x P.H = f w x f h) and the sigmas
__global__ __launch_bounds__(kBx* kBy) void k_upsample(DnParams P, UpLow L, double* __restrict__ out,
                                                       unsigned long long* __restrict__ fallbacks) {
    const int j = blockIdx.x * kBx + threadIdx.x, i = blockIdx.y * kBy + threadIdx.y;
    const bool inside = j < P.W && i < P.H;
    bool fell = false;
    if (inside) {
        const size_t p = (size_t)i * P.W + j;
        const Centre c = centre_of(P, p);
        const double half = (L.f - 1) / 2.0;
        const double y = ((double)i - half) / (double)L.f, x = ((double)j - half) / (double)L.f;
        const double yf = floor(y), xf = floor(x);
        const int i0 = (int)yf, j0 = (int)xf;
        const double fy = y - yf, fx = x - xf;
        double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int di = 0; di < 2; di++)
#pragma unroll
            for (int dj = 0; dj < 2; dj++) {
                const int qi = i0 + di, qj = j0 + dj;
                if (qi < 0 || qi >= L.h || qj < 0 || qj >= L.w) continue;
                const size_t q = (size_t)qi * L.w + qj;
                const double b = (di ? fy : 1.0 - fy) * (dj ? fx : 1.0 - fx);
                const double w = b * geo_of(P, c, L.depth[q], L.normal + 3 * q, L.position + 3 * q, L.albedo + 3 * q);
                s0 += w * L.color[3 * q];
                s1 += w * L.color[3 * q + 1];
                s2 += w * L.color[3 * q + 2];
                sw += w;
            }
        double o0, o1, o2;
        if (sw >= L.min_weight) {
            o0 = s0 / sw, o1 = s1 / sw, o2 = s2 / sw;
        } else {  // the low pixel that contains p
            const size_t q = (size_t)(i / L.f) * L.w + j / L.f;
            o0 = L.color[3 * q], o1 = L.color[3 * q + 1], o2 = L.color[3 * q + 2];
            fell = true;
        }
        out[3 * p] = o0;
        out[3 * p + 1] = o1;
        out[3 * p + 2] = o2;
    }
    // no lane has left: the ballot sees the whole wave (threadIdx.x = the lane)
    const unsigned long long m = __ballot(fell);
    if (threadIdx.x == 0 && m) atomicAdd(fallbacks, (unsigned long long)__popcll(m));
}

bool sigma_ok(double v) { return std::isfinite(v) && v > 0; }

int check_opts(const mcpt_upsample_opts* o) {
    if (!o) {
        set_error("null mcpt_upsample_opts");
        return MCPT_E_INVALID;
    }
    if (o->struct_size != sizeof(mcpt_upsample_opts)) {
        set_error("mcpt_upsample_opts.struct_size is %u, this library expects %zu (use mcpt_upsample_opts_init / the "
                  "mcpt.h of MCPT_VERSION %d)", o->struct_size, sizeof(mcpt_upsample_opts), MCPT_VERSION);
        return MCPT_E_INVALID;
    }
    if (o->factor < 2 || o->factor > 4) {
        set_error("invalid upsample options: factor %d is outside 2..4", o->factor);
        return MCPT_E_INVALID;
    }
    const struct {
        const char* name;
        double v;
    } sig[] = {{"sigma_normal", o->sigma_normal}, {"sigma_plane", o->sigma_plane}, {"sigma_albedo", o->sigma_albedo}};
    for (const auto& s : sig)
        if (!sigma_ok(s.v)) {
            set_error("invalid upsample options: %s %g must be finite and > 0", s.name, s.v);
            return MCPT_E_INVALID;
        }
    if (!std::isfinite(o->min_weight) || !(o->min_weight > 0) || !(o->min_weight <= 1)) {
        set_error("invalid upsample options: min_weight %g must lie in (0, 1]", o->min_weight);
        return MCPT_E_INVALID;
    }
    return MCPT_OK;
}

int check_guides(const mcpt_aov_buffers* g, const char* name) {
    if (!g || !g->albedo || !g->normal || !g->position || !g->depth) {
        set_error("null argument: %s (%s); all four guide arrays are required", name,
                  !g ? "the struct" : !g->albedo ? "albedo" : !g->normal ? "normal" : !g->position ? "position" : "depth");
        return MCPT_E_INVALID;
    }
    return MCPT_OK;
}

// every check a call makes before it touches a device; w, h: the low size
int check_call(const mcpt_upsample_opts* o, int w, int h, const double* color, const mcpt_aov_buffers* g,
               const mcpt_aov_buffers* G, const double* out) {
    int rc;
    if ((rc = check_opts(o))) return rc;
    const long long f = o->factor;
    if (w < 1 || h < 1 || (long long)w * h * f * f > (1ll << 28)) {
        set_error("invalid frame size: width %d, height %d at factor %d (the full frame may hold 2^28 pixels)", w, h, o->factor);
        return MCPT_E_INVALID;
    }
    if (!color || !out) {
        set_error("null argument: %s", !color ? "color" : "out");
        return MCPT_E_INVALID;
    }
    if ((rc = check_guides(g, "guides")) || (rc = check_guides(G, "full_guides"))) return rc;
    const size_t npx = (size_t)w * h, NPX = npx * (size_t)(f * f);
    const struct {
        const char* name;
        const double* p;
        size_t n;
    } ins[] = {{"color", color, 3 * npx},
               {"guides.albedo", g->albedo, 3 * npx},
               {"guides.normal", g->normal, 3 * npx},
               {"guides.position", g->position, 3 * npx},
               {"guides.depth", g->depth, npx},
               {"full_guides.albedo", G->albedo, 3 * NPX},
               {"full_guides.normal", G->normal, 3 * NPX},
               {"full_guides.position", G->position, 3 * NPX},
               {"full_guides.depth", G->depth, NPX}};
    for (const auto& r : ins)
        if ((uintptr_t)out < (uintptr_t)(r.p + r.n) && (uintptr_t)r.p < (uintptr_t)(out + 3 * NPX)) {
            set_error("out is aliasing %s: neighbouring pixels read it after it is written", r.name);
            return MCPT_E_INVALID;
        }
    return MCPT_OK;
}

// zeroes the count and launches the kernel on the null stream
int enqueue(const mcpt_upsample_opts* o, int w, int h, const double* dC, const mcpt_aov_buffers* g, const mcpt_aov_buffers* G,
            double* dOut, unsigned long long* dCount) {
    const int f = o->factor, W = w * f, H = h * f;
    const DnParams P{W, H, 0.0, o->sigma_normal, o->sigma_plane, o->sigma_albedo, G->albedo, G->normal, G->position, G->depth};
    const UpLow L{w, h, f, o->min_weight, dC, g->albedo, g->normal, g->position, g->depth};
    DN_HIP_OK(hipMemsetAsync(dCount, 0, sizeof *dCount, nullptr));
    const dim3 grid((W + kBx - 1) / kBx, (H + kBy - 1) / kBy), block(kBx, kBy);
    hipLaunchKernelGGL(k_upsample, grid, block, 0, nullptr, P, L, dOut, dCount);
    DN_HIP_OK(hipGetLastError());
    return MCPT_OK;
}

// the same, timed with two events and waited for; the count comes back
int run(const mcpt_upsample_opts* o, int w, int h, const double* dC, const mcpt_aov_buffers* g, const mcpt_aov_buffers* G,
        double* dOut, unsigned long long* dCount, Scratch& S, uint64_t* count, double* seconds) {
    int rc;
    DN_HIP_OK(hipEventCreate(&S.e0));
    DN_HIP_OK(hipEventCreate(&S.e1));
    DN_HIP_OK(hipEventRecord(S.e0, nullptr));
    if ((rc = enqueue(o, w, h, dC, g, G, dOut, dCount))) return rc;
    DN_HIP_OK(hipEventRecord(S.e1, nullptr));
    DN_HIP_OK(hipEventSynchronize(S.e1));
    float ms = 0;
    DN_HIP_OK(hipEventElapsedTime(&ms, S.e0, S.e1));
    if (seconds) *seconds = ms * 1e-3;
    unsigned long long n = 0;
    DN_HIP_OK(hipMemcpy(&n, dCount, sizeof n, hipMemcpyDeviceToHost));
    if (count) *count = n;
    return MCPT_OK;
}

}  // namespace

// mcpt_internal.h: the upsampling for a caller that owns every buffer (sequence.hip)
namespace mcpt {

int upsample_check_opts(const mcpt_upsample_opts* o) { return check_opts(o); }

int upsample_enqueue(const mcpt_upsample_opts* o, int32_t w, int32_t h, const double* dC, const mcpt_aov_buffers* g,
                     const mcpt_aov_buffers* G, double* dOut, unsigned long long* dCount) {
    int rc;
    if ((rc = check_call(o, w, h, dC, g, G, dOut))) return rc;
    if (!dCount) {
        set_error("null argument: the fallback counter");
        return MCPT_E_INVALID;
    }
    return enqueue(o, w, h, dC, g, G, dOut, dCount);
}

}  // namespace mcpt

extern "C" {

void mcpt_upsample_opts_init(mcpt_upsample_opts* o) {
    if (!o) return;
    std::memset((void*)o, 0, sizeof *o);
    o->struct_size = sizeof *o;
    o->factor = 2;
    o->sigma_normal = 128.0;
    o->sigma_plane = 0.01;
    o->sigma_albedo = 0.1;
    o->min_weight = 1e-4;
    o->device = -1;
}

int mcpt_upsample_device(const mcpt_upsample_opts* o, int32_t w, int32_t h, const double* dC, const mcpt_aov_buffers* g,
                         const mcpt_aov_buffers* G, double* dOut, uint64_t* count, double* seconds) {
    int rc;
    if ((rc = check_call(o, w, h, dC, g, G, dOut))) return rc;
    Scratch S;
    int device;
    if ((rc = select_device(o->device, S, &device))) return rc;
    if ((rc = check_device_array(dC, device, "dev_color")) || (rc = check_device_array(g->albedo, device, "dev_guides.albedo")) ||
        (rc = check_device_array(g->normal, device, "dev_guides.normal")) ||
        (rc = check_device_array(g->position, device, "dev_guides.position")) ||
        (rc = check_device_array(g->depth, device, "dev_guides.depth")) ||
        (rc = check_device_array(G->albedo, device, "dev_full_guides.albedo")) ||
        (rc = check_device_array(G->normal, device, "dev_full_guides.normal")) ||
        (rc = check_device_array(G->position, device, "dev_full_guides.position")) ||
        (rc = check_device_array(G->depth, device, "dev_full_guides.depth")) || (rc = check_device_array(dOut, device, "dev_out")))
        return rc;
    DN_HIP_OK(hipMalloc(&S.p, sizeof(unsigned long long)));
    // the caller's arrays may still be written by work on other streams (e.g. torch's)
    DN_HIP_OK(hipDeviceSynchronize());
    return run(o, w, h, dC, g, G, dOut, (unsigned long long*)S.p, S, count, seconds);
}

int mcpt_upsample(const mcpt_upsample_opts* o, int32_t w, int32_t h, const double* color, const mcpt_aov_buffers* g,
                  const mcpt_aov_buffers* G, double* out, uint64_t* count, double* seconds) {
    int rc;
    if ((rc = check_call(o, w, h, color, g, G, out))) return rc;
    Scratch S;
    int device;
    if ((rc = select_device(o->device, S, &device))) return rc;
    const size_t npx = (size_t)w * h, NPX = npx * o->factor * o->factor, B = sizeof(double);
    // the count's word, then low: colour 3, guides 3 + 3 + 3 + 1; full: guides 3 + 3 + 3 + 1, out 3
    DN_HIP_OK(hipMalloc(&S.p, (1 + 13 * npx + 13 * NPX) * B));
    double* dC = S.p + 1;
    const mcpt_aov_buffers dg{dC + 3 * npx, dC + 6 * npx, dC + 9 * npx, dC + 12 * npx};
    double* F = dC + 13 * npx;
    const mcpt_aov_buffers dG{F, F + 3 * NPX, F + 6 * NPX, F + 9 * NPX};
    double* dOut = F + 10 * NPX;
    DN_HIP_OK(hipMemcpy(dC, color, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dg.albedo, g->albedo, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dg.normal, g->normal, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dg.position, g->position, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dg.depth, g->depth, npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dG.albedo, G->albedo, 3 * NPX * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dG.normal, G->normal, 3 * NPX * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dG.position, G->position, 3 * NPX * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dG.depth, G->depth, NPX * B, hipMemcpyHostToDevice));
    if ((rc = run(o, w, h, dC, &dg, &dG, dOut, (unsigned long long*)S.p, S, count, seconds))) return rc;
    DN_HIP_OK(hipMemcpy(out, dOut, 3 * NPX * B, hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_camera_scaled(const mcpt_camera* in, int32_t factor, mcpt_camera* out) {
    if (!in || !out) {
        set_error("mcpt_camera_scaled: null argument: %s", !in ? "in" : "out");
        return MCPT_E_INVALID;
    }
    if (factor < 1 || in->width < 1 || in->height < 1 || (long long)in->width * factor > INT32_MAX ||
        (long long)in->height * factor > INT32_MAX) {
        set_error("mcpt_camera_scaled: factor %d must be >= 1 and the camera's width %d and height %d >= 1, their products "
                  "within 32 bits", factor, in->width, in->height);
        return MCPT_E_INVALID;
    }
    mcpt_camera r = *in;
    r.width = in->width * factor;
    r.height = in->height * factor;
    *out = r;
    return MCPT_OK;
}

}  // extern "C"
