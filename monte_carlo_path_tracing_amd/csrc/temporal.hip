// Temporal accumulation for gfx950 (mcpt_temporal_accumulate, include/mcpt.h states the rule in full) and the
// host helper mcpt_camera_orbit.  No counterpart in the reference.
//
//   k_temporal_accumulate  lane per pixel : reproject, gather the four taps of the previous history, blend,
//                                           and the temporal variance where the history is long enough
//   k_temporal_spatial     lane per pixel : V_0 of the a-trous filter on the blended colour, only in lanes whose
//                                           history is short (the others leave at once)
//
// Everything is fp64 with -ffp-contract=off, so a numpy restatement of the rule reproduces the output to
// rounding (tests/test_temporal.py).  A block is 64 x 4 pixels as in denoise.hip: the centre's loads and the
// stores are consecutive across a wave; the four gathers follow the reprojection, which keeps neighbours
// together under a camera move.  The centre's guides stay in registers for the four taps.  Plain loads and
// stores only: no atomics, no LDS.  Per pixel the first kernel reads 10 doubles of its own (colour, normal,
// position, depth), up to 4 x 14 of the previous frame (depth, moments, normal, position, colour; neighbouring
// lanes share them in cache) and writes 8: about 0.5 KB.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "cam_frame.h"
#include "denoise_common.h"
#include "mcpt.h"
#include "mcpt_internal.h"

using mcpt::set_error;
using namespace mcpt_dn;

namespace {

struct TpParams {
    int W, H;
    bool has_prev;
    double E[3], U[3], V[3], Nc[3], S;  // the previous camera's frame, S = wlen / pixellen
    double alpha, max_history, normal_min, plane_max, min_weight, var_n;  // var_n = variance_min_history - 0.5
    const double *C, *N, *X, *depth;        // the current frame
    const double *pN, *pX, *pdepth, *pC, *pM;  // the previous state
    double *outC, *outM, *outV;
};

__device__ inline bool temporal_variance_applies(const TpParams& P, double n, double g) { return n > P.var_n && g < 1.0; }

__global__ __launch_bounds__(kBx* kBy) void k_temporal_accumulate(TpParams P) {
    const int x = blockIdx.x * kBx + threadIdx.x, y = blockIdx.y * kBy + threadIdx.y;
    if (x >= P.W || y >= P.H) return;
    const size_t p = (size_t)y * P.W + x;
    const double c0 = P.C[3 * p], c1 = P.C[3 * p + 1], c2 = P.C[3 * p + 2];
    const double l = (c0 + c1 + c2) / 3.0;
    const double depth = P.depth[p];
    double wsum = 0.0, h0 = 0.0, h1 = 0.0, h2 = 0.0, m1 = 0.0, m2 = 0.0, hn = 0.0, hg = 0.0;
    bool source = false;
    if (P.has_prev && depth > 0) {
        const double N0 = P.N[3 * p], N1 = P.N[3 * p + 1], N2 = P.N[3 * p + 2];
        const double X0 = P.X[3 * p], X1 = P.X[3 * p + 1], X2 = P.X[3 * p + 2];
        const double d0 = X0 - P.E[0], d1 = X1 - P.E[1], d2 = X2 - P.E[2];
        const double a = d0 * P.U[0] + d1 * P.U[1] + d2 * P.U[2];
        const double b = d0 * P.V[0] + d1 * P.V[1] + d2 * P.V[2];
        const double c = d0 * P.Nc[0] + d1 * P.Nc[1] + d2 * P.Nc[2];
        if (c > 0) {
            const double ys = (P.H - 1) / 2.0 - P.S * a / c, xs = (P.W - 1) / 2.0 + P.S * b / c;
            if (ys > -1 && ys < P.H && xs > -1 && xs < P.W) {  // in double: only now is the conversion to int safe
                source = true;
                const double fi = floor(ys), fj = floor(xs);
                const int i0 = (int)fi, j0 = (int)fj;
                const double fy = ys - fi, fx = xs - fj;
                const double plane = P.plane_max * depth;
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int di = t >> 1, dj = t & 1, qi = i0 + di, qj = j0 + dj;
                    if (qi < 0 || qi >= P.H || qj < 0 || qj >= P.W) continue;
                    const size_t q = (size_t)qi * P.W + qj;
                    if (!(P.pdepth[q] > 0) || !(P.pM[4 * q + 2] > 0)) continue;
                    const double nn = N0 * P.pN[3 * q] + N1 * P.pN[3 * q + 1] + N2 * P.pN[3 * q + 2];
                    if (!(nn >= P.normal_min)) continue;
                    const double pd = N0 * (P.pX[3 * q] - X0) + N1 * (P.pX[3 * q + 1] - X1) + N2 * (P.pX[3 * q + 2] - X2);
                    if (!(fabs(pd) <= plane)) continue;
                    const double bq = (di ? fy : 1.0 - fy) * (dj ? fx : 1.0 - fx);
                    wsum += bq;
                    h0 += bq * P.pC[3 * q];
                    h1 += bq * P.pC[3 * q + 1];
                    h2 += bq * P.pC[3 * q + 2];
                    m1 += bq * P.pM[4 * q];
                    m2 += bq * P.pM[4 * q + 1];
                    hn += bq * P.pM[4 * q + 2];
                    hg += bq * P.pM[4 * q + 3];
                }
            }
        }
    }
    double o0 = c0, o1 = c1, o2 = c2, om1 = l, om2 = l * l, on = 1.0, og = 1.0;
    if (source && wsum >= P.min_weight) {
        on = fmin(hn / wsum + 1.0, P.max_history);
        const double A = fmax(P.alpha, 1.0 / on), B = 1.0 - A;
        o0 = B * (h0 / wsum) + A * c0;
        o1 = B * (h1 / wsum) + A * c1;
        o2 = B * (h2 / wsum) + A * c2;
        om1 = B * (m1 / wsum) + A * l;
        om2 = B * (m2 / wsum) + A * (l * l);
        og = B * B * (hg / wsum) + A * A;
    }
    P.outC[3 * p] = o0, P.outC[3 * p + 1] = o1, P.outC[3 * p + 2] = o2;
    P.outM[4 * p] = om1, P.outM[4 * p + 1] = om2, P.outM[4 * p + 2] = on, P.outM[4 * p + 3] = og;
    if (P.outV && temporal_variance_applies(P, on, og)) P.outV[p] = fmax(0.0, om2 - om1 * om1) * og / (1.0 - og);
}

// the pixels k_temporal_accumulate left without a variance: V_0 of the blended colour (D's guides are the current ones)
__global__ __launch_bounds__(kBx* kBy) void k_temporal_spatial(TpParams P, DnParams D) {
    const int x = blockIdx.x * kBx + threadIdx.x, y = blockIdx.y * kBy + threadIdx.y;
    if (x >= P.W || y >= P.H) return;
    const size_t p = (size_t)y * P.W + x;
    if (temporal_variance_applies(P, P.outM[4 * p + 2], P.outM[4 * p + 3])) return;
    P.outV[p] = spatial_v0(D, P.outC, x, y);
}

struct Range {
    const char* name;
    const double* p;
    size_t n;
};
bool overlap(const Range& a, const Range& b) {
    return a.p && b.p && (uintptr_t)a.p < (uintptr_t)(b.p + b.n) && (uintptr_t)b.p < (uintptr_t)(a.p + a.n);
}

// every check a call makes before it touches a device; *has_prev: the previous state is given
int check_call(const mcpt_temporal_opts* o, const mcpt_camera* pc, int W, int H, const double* color, const mcpt_aov_buffers* g,
               const mcpt_aov_buffers* pg, const double* pcol, const double* pmom, const double* out, const double* outm,
               const double* outv, bool* has_prev) {
    if (!o) {
        set_error("null mcpt_temporal_opts");
        return MCPT_E_INVALID;
    }
    if (o->struct_size != sizeof(mcpt_temporal_opts)) {
        set_error("mcpt_temporal_opts.struct_size is %u, this library expects %zu (use mcpt_temporal_opts_init / the "
                  "mcpt.h of MCPT_VERSION %d)", o->struct_size, sizeof(mcpt_temporal_opts), MCPT_VERSION);
        return MCPT_E_INVALID;
    }
    if (!(o->alpha > 0 && o->alpha <= 1)) {
        set_error("invalid temporal options: alpha %g is outside (0, 1]", o->alpha);
        return MCPT_E_INVALID;
    }
    if (o->max_history < 1) {
        set_error("invalid temporal options: max_history %d must be >= 1", o->max_history);
        return MCPT_E_INVALID;
    }
    if (!std::isfinite(o->normal_min)) {
        set_error("invalid temporal options: normal_min %g must be finite", o->normal_min);
        return MCPT_E_INVALID;
    }
    if (!(o->min_weight > 0 && o->min_weight <= 1)) {
        set_error("invalid temporal options: min_weight %g is outside (0, 1]", o->min_weight);
        return MCPT_E_INVALID;
    }
    if (o->variance_min_history < 2) {
        set_error("invalid temporal options: variance_min_history %d must be >= 2", o->variance_min_history);
        return MCPT_E_INVALID;
    }
    const struct {
        const char* name;
        double v;
    } pos[] = {{"plane_max", o->plane_max}, {"sigma_normal", o->sigma_normal}, {"sigma_plane", o->sigma_plane},
               {"sigma_albedo", o->sigma_albedo}};
    for (const auto& s : pos)
        if (!std::isfinite(s.v) || !(s.v > 0)) {
            set_error("invalid temporal options: %s %g must be finite and > 0", s.name, s.v);
            return MCPT_E_INVALID;
        }
    if (W < 1 || H < 1 || (long long)W * H > (1ll << 28)) {
        set_error("invalid frame size: width %d, height %d", W, H);
        return MCPT_E_INVALID;
    }
    if (!color || !out || !outm) {
        set_error("null argument: %s", !color ? "color" : !out ? "out_color" : "out_moments");
        return MCPT_E_INVALID;
    }
    if (!g || !g->albedo || !g->normal || !g->position || !g->depth) {
        set_error("null argument: guides (%s); all four guide arrays are required",
                  !g ? "the struct" : !g->albedo ? "albedo" : !g->normal ? "normal" : !g->position ? "position" : "depth");
        return MCPT_E_INVALID;
    }
    const int given = (pc != nullptr) + (pg != nullptr) + (pcol != nullptr) + (pmom != nullptr);
    *has_prev = given == 4;
    if (given != 0 && given != 4) {
        set_error("partial previous state: %s is NULL while %s is given (pass prev_cam, prev_guides, prev_color and "
                  "prev_moments, or none of them)", !pc ? "prev_cam" : !pg ? "prev_guides" : !pcol ? "prev_color" : "prev_moments",
                  pc ? "prev_cam" : pg ? "prev_guides" : pcol ? "prev_color" : "prev_moments");
        return MCPT_E_INVALID;
    }
    if (*has_prev) {
        if (!pg->normal || !pg->position || !pg->depth) {
            set_error("partial previous state: prev_guides.%s is NULL (normal, position and depth are required)",
                      !pg->normal ? "normal" : !pg->position ? "position" : "depth");
            return MCPT_E_INVALID;
        }
        if (pc->width != W || pc->height != H) {
            set_error("prev_cam is %d x %d, the frame is width %d, height %d: the history cannot change size", pc->width,
                      pc->height, W, H);
            return MCPT_E_INVALID;
        }
    }
    // an output overlapping an input would be read by other pixels after it is written
    const size_t npx = (size_t)W * H;
    const Range ins[] = {{"color", color, 3 * npx},
                         {"guides.albedo", g->albedo, 3 * npx},
                         {"guides.normal", g->normal, 3 * npx},
                         {"guides.position", g->position, 3 * npx},
                         {"guides.depth", g->depth, npx},
                         {"prev_guides.normal", *has_prev ? pg->normal : nullptr, 3 * npx},
                         {"prev_guides.position", *has_prev ? pg->position : nullptr, 3 * npx},
                         {"prev_guides.depth", *has_prev ? pg->depth : nullptr, npx},
                         {"prev_color", pcol, 3 * npx},
                         {"prev_moments", pmom, 4 * npx}},
                outs[] = {{"out_color", out, 3 * npx}, {"out_moments", outm, 4 * npx}, {"out_variance", outv, npx}};
    for (const auto& w : outs)
        for (const auto& r : ins)
            if (overlap(w, r)) {
                set_error("%s is aliasing %s: the accumulation cannot run in place (swap two sets of history buffers)",
                          w.name, r.name);
                return MCPT_E_INVALID;
            }
    for (int a = 0; a < 3; a++)
        for (int b = a + 1; b < 3; b++)
            if (overlap(outs[a], outs[b])) {
                set_error("%s is aliasing %s", outs[a].name, outs[b].name);
                return MCPT_E_INVALID;
            }
    return MCPT_OK;
}

// both kernels over device arrays
int run_accumulate(const mcpt_temporal_opts* o, const mcpt_camera* pc, int W, int H, const double* dC, const mcpt_aov_buffers* g,
                   const mcpt_aov_buffers* pg, const double* dpC, const double* dpM, double* dOut, double* dOutM,
                   double* dOutV, Scratch& S, double* seconds) {
    TpParams P{};
    P.W = W, P.H = H;
    P.has_prev = pc != nullptr;
    if (pc) {
        const mcpt::CamFrame f = mcpt::cam_setup(*pc);
        const mcpt::d3 v[4] = {f.eye, f.U, f.V, f.N};
        double* dst[4] = {P.E, P.U, P.V, P.Nc};
        for (int k = 0; k < 4; k++) dst[k][0] = v[k].x, dst[k][1] = v[k].y, dst[k][2] = v[k].z;
        P.S = f.wlen / f.pixellen;
        P.pN = pg->normal, P.pX = pg->position, P.pdepth = pg->depth, P.pC = dpC, P.pM = dpM;
    }
    P.alpha = o->alpha, P.max_history = o->max_history, P.normal_min = o->normal_min, P.plane_max = o->plane_max;
    P.min_weight = o->min_weight, P.var_n = o->variance_min_history - 0.5;
    P.C = dC, P.N = g->normal, P.X = g->position, P.depth = g->depth;
    P.outC = dOut, P.outM = dOutM, P.outV = dOutV;
    const DnParams D{W, H, 0.0, o->sigma_normal, o->sigma_plane, o->sigma_albedo, g->albedo, g->normal, g->position, g->depth};
    const dim3 grid((W + kBx - 1) / kBx, (H + kBy - 1) / kBy), block(kBx, kBy);
    DN_HIP_OK(hipEventCreate(&S.e0));
    DN_HIP_OK(hipEventCreate(&S.e1));
    DN_HIP_OK(hipEventRecord(S.e0, nullptr));
    hipLaunchKernelGGL(k_temporal_accumulate, grid, block, 0, nullptr, P);
    DN_HIP_OK(hipGetLastError());
    if (dOutV) {
        hipLaunchKernelGGL(k_temporal_spatial, grid, block, 0, nullptr, P, D);
        DN_HIP_OK(hipGetLastError());
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

void mcpt_temporal_opts_init(mcpt_temporal_opts* o) {
    if (!o) return;
    std::memset((void*)o, 0, sizeof *o);
    o->struct_size = sizeof *o;
    o->max_history = 64;
    o->variance_min_history = 4;
    o->device = -1;
    o->alpha = 0.1;
    o->normal_min = 0.9;
    o->plane_max = 0.02;
    o->min_weight = 0.01;
    o->sigma_normal = 128.0;
    o->sigma_plane = 0.01;
    o->sigma_albedo = 0.1;
}

int mcpt_temporal_accumulate_device(const mcpt_temporal_opts* o, const mcpt_camera* pc, int32_t W, int32_t H, const double* dC,
                                    const mcpt_aov_buffers* g, const mcpt_aov_buffers* pg, const double* dpC, const double* dpM,
                                    double* dOut, double* dOutM, double* dOutV, double* seconds) {
    int rc;
    bool has_prev = false;
    if ((rc = check_call(o, pc, W, H, dC, g, pg, dpC, dpM, dOut, dOutM, dOutV, &has_prev))) return rc;
    Scratch S;
    int device;
    if ((rc = select_device(o->device, S, &device))) return rc;
    if ((rc = check_device_array(dC, device, "dev_color")) || (rc = check_device_array(g->albedo, device, "dev_guides.albedo")) ||
        (rc = check_device_array(g->normal, device, "dev_guides.normal")) ||
        (rc = check_device_array(g->position, device, "dev_guides.position")) ||
        (rc = check_device_array(g->depth, device, "dev_guides.depth")) || (rc = check_device_array(dOut, device, "dev_out_color")) ||
        (rc = check_device_array(dOutM, device, "dev_out_moments")) ||
        (dOutV && (rc = check_device_array(dOutV, device, "dev_out_variance"))))
        return rc;
    if (has_prev && ((rc = check_device_array(pg->normal, device, "dev_prev_guides.normal")) ||
                     (rc = check_device_array(pg->position, device, "dev_prev_guides.position")) ||
                     (rc = check_device_array(pg->depth, device, "dev_prev_guides.depth")) ||
                     (rc = check_device_array(dpC, device, "dev_prev_color")) ||
                     (rc = check_device_array(dpM, device, "dev_prev_moments"))))
        return rc;
    // the caller's arrays may still be written by work on other streams (e.g. torch's)
    DN_HIP_OK(hipDeviceSynchronize());
    return run_accumulate(o, has_prev ? pc : nullptr, W, H, dC, g, pg, dpC, dpM, dOut, dOutM, dOutV, S, seconds);
}

int mcpt_temporal_accumulate(const mcpt_temporal_opts* o, const mcpt_camera* pc, int32_t W, int32_t H, const double* color,
                             const mcpt_aov_buffers* g, const mcpt_aov_buffers* pg, const double* pcol, const double* pmom,
                             double* out, double* outm, double* outv, double* seconds) {
    int rc;
    bool has_prev = false;
    if ((rc = check_call(o, pc, W, H, color, g, pg, pcol, pmom, out, outm, outv, &has_prev))) return rc;
    Scratch S;
    int device;
    if ((rc = select_device(o->device, S, &device))) return rc;
    const size_t npx = (size_t)W * H, B = sizeof(double);
    // colour 3, guides 3 + 3 + 3 + 1, out colour 3, moments 4, variance 1, then the previous state 3 + 3 + 1 + 3 + 4
    DN_HIP_OK(hipMalloc(&S.p, (has_prev ? 35 : 21) * npx * B));
    double* dC = S.p;
    const mcpt_aov_buffers dg{dC + 3 * npx, dC + 6 * npx, dC + 9 * npx, dC + 12 * npx};
    double* dOut = dC + 13 * npx;
    double* dOutM = dOut + 3 * npx;
    double* dOutV = dOutM + 4 * npx;
    double* prev = has_prev ? dOutV + npx : nullptr;  // only then does the allocation reach that far
    const mcpt_aov_buffers dpg{nullptr, prev, prev ? prev + 3 * npx : nullptr, prev ? prev + 6 * npx : nullptr};
    double* dpC = prev ? prev + 7 * npx : nullptr;
    double* dpM = prev ? dpC + 3 * npx : nullptr;
    DN_HIP_OK(hipMemcpy(dC, color, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dg.albedo, g->albedo, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dg.normal, g->normal, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dg.position, g->position, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dg.depth, g->depth, npx * B, hipMemcpyHostToDevice));
    if (has_prev) {
        DN_HIP_OK(hipMemcpy(dpg.normal, pg->normal, 3 * npx * B, hipMemcpyHostToDevice));
        DN_HIP_OK(hipMemcpy(dpg.position, pg->position, 3 * npx * B, hipMemcpyHostToDevice));
        DN_HIP_OK(hipMemcpy(dpg.depth, pg->depth, npx * B, hipMemcpyHostToDevice));
        DN_HIP_OK(hipMemcpy(dpC, pcol, 3 * npx * B, hipMemcpyHostToDevice));
        DN_HIP_OK(hipMemcpy(dpM, pmom, 4 * npx * B, hipMemcpyHostToDevice));
    }
    if ((rc = run_accumulate(o, has_prev ? pc : nullptr, W, H, dC, &dg, &dpg, dpC, dpM, dOut, dOutM, outv ? dOutV : nullptr, S,
                             seconds)))
        return rc;
    DN_HIP_OK(hipMemcpy(out, dOut, 3 * npx * B, hipMemcpyDeviceToHost));
    DN_HIP_OK(hipMemcpy(outm, dOutM, 4 * npx * B, hipMemcpyDeviceToHost));
    if (outv) DN_HIP_OK(hipMemcpy(outv, dOutV, npx * B, hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_camera_orbit(const mcpt_camera* in, double degrees, mcpt_camera* out) {
    if (!in || !out) {
        set_error("mcpt_camera_orbit: null argument: %s", !in ? "in" : "out");
        return MCPT_E_INVALID;
    }
    const double ul = std::sqrt(in->up[0] * in->up[0] + in->up[1] * in->up[1] + in->up[2] * in->up[2]);
    if (!std::isfinite(degrees) || !std::isfinite(ul) || !(ul > 0)) {
        set_error("mcpt_camera_orbit: degrees %g must be finite and up must have a finite length > 0 (it is %g)", degrees, ul);
        return MCPT_E_INVALID;
    }
    const double t = degrees * 3.14159265358979323846 / 180.0, s = std::sin(t), c1 = 1.0 - std::cos(t);
    const double k[3] = {in->up[0] / ul, in->up[1] / ul, in->up[2] / ul};
    const double v[3] = {in->eye[0] - in->lookat[0], in->eye[1] - in->lookat[1], in->eye[2] - in->lookat[2]};
    const double kv = k[0] * v[0] + k[1] * v[1] + k[2] * v[2];
    const double kxv[3] = {k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0]};
    mcpt_camera r = *in;
    for (int a = 0; a < 3; a++) r.eye[a] = in->eye[a] + (kxv[a] * s - (v[a] - k[a] * kv) * c1);
    *out = r;
    return MCPT_OK;
}

}  // extern "C"
