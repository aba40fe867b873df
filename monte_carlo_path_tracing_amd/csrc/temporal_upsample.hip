// Temporal upsampling for gfx950 (mcpt_temporal_upsample, include/mcpt.h states the rule in full) and the host helper
// mcpt_upsample_phase.  No counterpart in the reference.
//
//   k_temporal_upsample  lane per full-size pixel : reproject and gather the four taps of the previous full-size
//                                                   history (mcpt_temporal_accumulate's steps), then one of four cases:
//                                                   a traced pixel blends its sample of the low frame or starts a
//                                                   history, an untraced one carries its history over unblended or is
//                                                   filled from the four nearest traced samples, weighed by geo(p, q')
//                                                   over the full-size guides; the temporal variance where the history
//                                                   is long enough; the filled and the fallback pixels counted
//   k_temporal_spatial   (temporal.hip, through temporal_spatial_enqueue) V_0 for the pixels left without a variance
//
// Everything is fp64 with -ffp-contract=off, so a numpy restatement of the rule reproduces the output to rounding
// (tests/test_temporal_upsample.py).  A block is 64 x 4 full-size pixels as in temporal.hip and upsample.hip: a wave is
// 64 consecutive x of one row, so the centre's loads and the stores are consecutive across the wave.  Every lane does
// the reprojection gather first; the fill runs only in the lanes without history, which after the first f^2 frames are
// disocclusions and frame borders.  The traced lanes are every f-th of a wave in every f-th row, and their loads of the
// low frame are consecutive.  Plain loads and stores only, no LDS; the two counts are integers: a wave counts its lanes
// with a ballot and issues one 64-bit integer atomic per count, so they are exact.  Per pixel the kernel reads 7 doubles
// of its own guides, up to 4 x 14 of the previous frame (neighbouring lanes share them in cache), 3 of the low frame in
// one lane of f^2 and writes 8; a filled pixel reads up to 4 x 10 guides and 4 x 3 colours more: about 0.6 KB.
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

struct TuParams {
    int w, h, f, a, b;  // the low frame, the factor and the phase; the full size is in the guides' DnParams
    bool has_prev;
    double E[3], U[3], V[3], Nc[3], S;  // the previous full-size camera's frame, S = wlen / pixellen
    double alpha, max_history, normal_min, plane_max, min_weight, var_n;  // the accumulation's; var_n = variance_min_history - 0.5
    double fill_min_weight;                                              // the fill's (mcpt_upsample_opts.min_weight)
    const double* C;                           // the low colour
    const double *pN, *pX, *pdepth, *pC, *pM;  // the previous state
    double *outC, *outM, *outV;
};

// G: the full-size guides with the FILL's sigmas (geo of the fill); counts: filled, fallback
__global__ __launch_bounds__(kBx* kBy) void k_temporal_upsample(TuParams P, DnParams G, unsigned long long* __restrict__ counts) {
    const int x = blockIdx.x * kBx + threadIdx.x, y = blockIdx.y * kBy + threadIdx.y;
    const bool inside = x < G.W && y < G.H;
    bool filled = false, fell = false;
    if (inside) {
        const size_t p = (size_t)y * G.W + x;
        const bool traced = y % P.f == P.a && x % P.f == P.b;
        double c0 = 0.0, c1 = 0.0, c2 = 0.0;
        if (traced) {
            const size_t q = (size_t)(y / P.f) * P.w + x / P.f;
            c0 = P.C[3 * q], c1 = P.C[3 * q + 1], c2 = P.C[3 * q + 2];
        }
        const double l = (c0 + c1 + c2) / 3.0;
        // mcpt_temporal_accumulate's source, taps and history (k_temporal_accumulate), at the full size
        const double depth = G.depth[p];
        double wsum = 0.0, h0 = 0.0, h1 = 0.0, h2 = 0.0, m1 = 0.0, m2 = 0.0, hn = 0.0, hg = 0.0;
        bool source = false;
        if (P.has_prev && depth > 0) {
            const double N0 = G.normal[3 * p], N1 = G.normal[3 * p + 1], N2 = G.normal[3 * p + 2];
            const double X0 = G.position[3 * p], X1 = G.position[3 * p + 1], X2 = G.position[3 * p + 2];
            const double d0 = X0 - P.E[0], d1 = X1 - P.E[1], d2 = X2 - P.E[2];
            const double a = d0 * P.U[0] + d1 * P.U[1] + d2 * P.U[2];
            const double b = d0 * P.V[0] + d1 * P.V[1] + d2 * P.V[2];
            const double c = d0 * P.Nc[0] + d1 * P.Nc[1] + d2 * P.Nc[2];
            if (c > 0) {
                const double ys = (G.H - 1) / 2.0 - P.S * a / c, xs = (G.W - 1) / 2.0 + P.S * b / c;
                if (ys > -1 && ys < G.H && xs > -1 && xs < G.W) {  // in double: only now is the conversion to int safe
                    source = true;
                    const double fi = floor(ys), fj = floor(xs);
                    const int i0 = (int)fi, j0 = (int)fj;
                    const double fy = ys - fi, fx = xs - fj;
                    const double plane = P.plane_max * depth;
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const int di = t >> 1, dj = t & 1, qi = i0 + di, qj = j0 + dj;
                        if (qi < 0 || qi >= G.H || qj < 0 || qj >= G.W) continue;
                        const size_t q = (size_t)qi * G.W + qj;
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
        const bool history = source && wsum >= P.min_weight;
        double o0 = c0, o1 = c1, o2 = c2, om1 = l, om2 = l * l, on = 1.0, og = 1.0;  // traced, without history
        if (traced && history) {  // the blend
            on = fmin(hn / wsum + 1.0, P.max_history);
            const double A = fmax(P.alpha, 1.0 / on), B = 1.0 - A;
            o0 = B * (h0 / wsum) + A * c0;
            o1 = B * (h1 / wsum) + A * c1;
            o2 = B * (h2 / wsum) + A * c2;
            om1 = B * (m1 / wsum) + A * l;
            om2 = B * (m2 / wsum) + A * (l * l);
            og = B * B * (hg / wsum) + A * A;
        } else if (!traced && history) {  // carried over: nothing is blended, n is not incremented
            o0 = h0 / wsum, o1 = h1 / wsum, o2 = h2 / wsum;
            om1 = m1 / wsum, om2 = m2 / wsum, on = hn / wsum, og = hg / wsum;
        } else if (!traced) {  // the fill: the four traced samples around p, weighed over the full-size guides
            filled = true;
            const Centre ctr = centre_of(G, p);
            const double ys = ((double)y - (double)P.a) / (double)P.f, xs = ((double)x - (double)P.b) / (double)P.f;
            const double yf = floor(ys), xf = floor(xs);
            const int i0 = (int)yf, j0 = (int)xf;
            const double fy = ys - yf, fx = xs - xf;
            double sw = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int di = 0; di < 2; di++)
#pragma unroll
                for (int dj = 0; dj < 2; dj++) {
                    const int qi = i0 + di, qj = j0 + dj;
                    if (qi < 0 || qi >= P.h || qj < 0 || qj >= P.w) continue;
                    const size_t q = (size_t)qi * P.w + qj;
                    const size_t qf = (size_t)(P.f * qi + P.a) * G.W + (P.f * qj + P.b);  // the pixel q was traced through
                    const double bq = (di ? fy : 1.0 - fy) * (dj ? fx : 1.0 - fx);
                    const double wq = bq * geo(G, ctr, qf);
                    s0 += wq * P.C[3 * q];
                    s1 += wq * P.C[3 * q + 1];
                    s2 += wq * P.C[3 * q + 2];
                    sw += wq;
                }
            if (sw >= P.fill_min_weight) {
                o0 = s0 / sw, o1 = s1 / sw, o2 = s2 / sw;
            } else {  // the nearest traced pixel
                const int qi = min(max((int)floor(ys + 0.5), 0), P.h - 1), qj = min(max((int)floor(xs + 0.5), 0), P.w - 1);
                const size_t q = (size_t)qi * P.w + qj;
                o0 = P.C[3 * q], o1 = P.C[3 * q + 1], o2 = P.C[3 * q + 2];
                fell = true;
            }
            om1 = (o0 + o1 + o2) / 3.0;
            om2 = om1 * om1;
            on = 0.0;  // nobody's sample: shown, never a history
        }
        P.outC[3 * p] = o0, P.outC[3 * p + 1] = o1, P.outC[3 * p + 2] = o2;
        P.outM[4 * p] = om1, P.outM[4 * p + 1] = om2, P.outM[4 * p + 2] = on, P.outM[4 * p + 3] = og;
        if (P.outV && on > P.var_n && og < 1.0) P.outV[p] = fmax(0.0, om2 - om1 * om1) * og / (1.0 - og);
    }
    // no lane has left: the ballots see the whole wave (threadIdx.x = the lane)
    const unsigned long long mf = __ballot(filled), mb = __ballot(fell);
    if (threadIdx.x == 0) {
        if (mf) atomicAdd(counts, (unsigned long long)__popcll(mf));
        if (mb) atomicAdd(counts + 1, (unsigned long long)__popcll(mb));
    }
}

struct Range {
    const char* name;
    const double* p;
    size_t n;
};
bool overlap(const Range& a, const Range& b) {
    return a.p && b.p && (uintptr_t)a.p < (uintptr_t)(b.p + b.n) && (uintptr_t)b.p < (uintptr_t)(a.p + a.n);
}

// every check a call makes before it touches a device; w, h: the low size; *has_prev: the previous state is given
int check_call(const mcpt_temporal_opts* tp, const mcpt_upsample_opts* up, int a, int b, const mcpt_camera* pc, int w, int h,
               const double* color, const mcpt_aov_buffers* G, const mcpt_aov_buffers* pG, const double* pcol, const double* pmom,
               const double* out, const double* outm, const double* outv, bool* has_prev) {
    int rc;
    if ((rc = mcpt::temporal_check_opts(tp, nullptr, false)) || (rc = mcpt::upsample_check_opts(up))) return rc;
    const long long f = up->factor;
    if (a < 0 || a >= f || b < 0 || b >= f) {
        set_error("invalid phase (%d, %d): both must lie in [0, factor = %d)", a, b, up->factor);
        return MCPT_E_INVALID;
    }
    if (w < 1 || h < 1 || (long long)w * h * f * f > (1ll << 28)) {
        set_error("invalid frame size: width %d, height %d at factor %d (the full frame may hold 2^28 pixels)", w, h, up->factor);
        return MCPT_E_INVALID;
    }
    if (!color || !out || !outm) {
        set_error("null argument: %s", !color ? "color" : !out ? "out_color" : "out_moments");
        return MCPT_E_INVALID;
    }
    if (!G || !G->albedo || !G->normal || !G->position || !G->depth) {
        set_error("null argument: full_guides (%s); all four guide arrays are required",
                  !G ? "the struct" : !G->albedo ? "albedo" : !G->normal ? "normal" : !G->position ? "position" : "depth");
        return MCPT_E_INVALID;
    }
    const int given = (pc != nullptr) + (pG != nullptr) + (pcol != nullptr) + (pmom != nullptr);
    *has_prev = given == 4;
    if (given != 0 && given != 4) {
        set_error("partial previous state: %s is NULL while %s is given (pass prev_full_cam, prev_full_guides, prev_color and "
                  "prev_moments, or none of them)",
                  !pc ? "prev_full_cam" : !pG ? "prev_full_guides" : !pcol ? "prev_color" : "prev_moments",
                  pc ? "prev_full_cam" : pG ? "prev_full_guides" : pcol ? "prev_color" : "prev_moments");
        return MCPT_E_INVALID;
    }
    const int W = (int)(w * f), H = (int)(h * f);
    if (*has_prev) {
        if (!pG->normal || !pG->position || !pG->depth) {
            set_error("partial previous state: prev_full_guides.%s is NULL (normal, position and depth are required)",
                      !pG->normal ? "normal" : !pG->position ? "position" : "depth");
            return MCPT_E_INVALID;
        }
        if (pc->width != W || pc->height != H) {
            set_error("prev_full_cam is %d x %d, the full frame is width %d, height %d (factor %d times the low %d x %d): the "
                      "history lives at the full size", pc->width, pc->height, W, H, up->factor, w, h);
            return MCPT_E_INVALID;
        }
    }
    const size_t npx = (size_t)w * h, NPX = (size_t)W * H;
    const Range ins[] = {{"color", color, 3 * npx},
                         {"full_guides.albedo", G->albedo, 3 * NPX},
                         {"full_guides.normal", G->normal, 3 * NPX},
                         {"full_guides.position", G->position, 3 * NPX},
                         {"full_guides.depth", G->depth, NPX},
                         {"prev_full_guides.normal", *has_prev ? pG->normal : nullptr, 3 * NPX},
                         {"prev_full_guides.position", *has_prev ? pG->position : nullptr, 3 * NPX},
                         {"prev_full_guides.depth", *has_prev ? pG->depth : nullptr, NPX},
                         {"prev_color", pcol, 3 * NPX},
                         {"prev_moments", pmom, 4 * NPX}},
                outs[] = {{"out_color", out, 3 * NPX}, {"out_moments", outm, 4 * NPX}, {"out_variance", outv, NPX}};  // NULL: overlaps nothing
    for (const auto& o : outs)
        for (const auto& r : ins)
            if (overlap(o, r)) {
                set_error("%s is aliasing %s: other pixels read it after it is written (swap two sets of history buffers)", o.name,
                          r.name);
                return MCPT_E_INVALID;
            }
    for (int i = 0; i < 3; i++)
        for (int j = i + 1; j < 3; j++)
            if (overlap(outs[i], outs[j])) {
                set_error("%s is aliasing %s", outs[i].name, outs[j].name);
                return MCPT_E_INVALID;
            }
    return MCPT_OK;
}

// zeroes the counts and launches the kernels on the null stream; pc == nullptr: no previous state
int enqueue(const mcpt_temporal_opts* tp, const mcpt_upsample_opts* up, int a, int b, const mcpt_camera* pc, int w, int h,
            const double* dC, const mcpt_aov_buffers* G, const mcpt_aov_buffers* pG, const double* dpC, const double* dpM,
            double* dOut, double* dOutM, double* dOutV, unsigned long long* dCounts) {
    const int f = up->factor, W = w * f, H = h * f;
    TuParams P{};
    P.w = w, P.h = h, P.f = f, P.a = a, P.b = b;
    P.has_prev = pc != nullptr;
    if (pc) {
        const mcpt::CamFrame cf = mcpt::cam_setup(*pc);
        const mcpt::d3 v[4] = {cf.eye, cf.U, cf.V, cf.N};
        double* dst[4] = {P.E, P.U, P.V, P.Nc};
        for (int k = 0; k < 4; k++) dst[k][0] = v[k].x, dst[k][1] = v[k].y, dst[k][2] = v[k].z;
        P.S = cf.wlen / cf.pixellen;
        P.pN = pG->normal, P.pX = pG->position, P.pdepth = pG->depth, P.pC = dpC, P.pM = dpM;
    }
    P.alpha = tp->alpha, P.max_history = tp->max_history, P.normal_min = tp->normal_min, P.plane_max = tp->plane_max;
    P.min_weight = tp->min_weight, P.var_n = tp->variance_min_history - 0.5;
    P.fill_min_weight = up->min_weight;
    P.C = dC;
    P.outC = dOut, P.outM = dOutM, P.outV = dOutV;
    const DnParams D{W, H, 0.0, up->sigma_normal, up->sigma_plane, up->sigma_albedo, G->albedo, G->normal, G->position, G->depth};
    DN_HIP_OK(hipMemsetAsync(dCounts, 0, 2 * sizeof *dCounts, nullptr));
    const dim3 grid((W + kBx - 1) / kBx, (H + kBy - 1) / kBy), block(kBx, kBy);
    hipLaunchKernelGGL(k_temporal_upsample, grid, block, 0, nullptr, P, D, dCounts);
    DN_HIP_OK(hipGetLastError());
    if (dOutV) return mcpt::temporal_spatial_enqueue(tp, W, H, G, dOut, dOutM, dOutV);
    return MCPT_OK;
}

// the same, timed with two events and waited for; the counts come back
int run(const mcpt_temporal_opts* tp, const mcpt_upsample_opts* up, int a, int b, const mcpt_camera* pc, int w, int h,
        const double* dC, const mcpt_aov_buffers* G, const mcpt_aov_buffers* pG, const double* dpC, const double* dpM, double* dOut,
        double* dOutM, double* dOutV, unsigned long long* dCounts, Scratch& S, uint64_t* filled, uint64_t* fallback,
        double* seconds) {
    int rc;
    DN_HIP_OK(hipEventCreate(&S.e0));
    DN_HIP_OK(hipEventCreate(&S.e1));
    DN_HIP_OK(hipEventRecord(S.e0, nullptr));
    if ((rc = enqueue(tp, up, a, b, pc, w, h, dC, G, pG, dpC, dpM, dOut, dOutM, dOutV, dCounts))) return rc;
    DN_HIP_OK(hipEventRecord(S.e1, nullptr));
    DN_HIP_OK(hipEventSynchronize(S.e1));
    float ms = 0;
    DN_HIP_OK(hipEventElapsedTime(&ms, S.e0, S.e1));
    if (seconds) *seconds = ms * 1e-3;
    unsigned long long n[2] = {0, 0};
    DN_HIP_OK(hipMemcpy(n, dCounts, sizeof n, hipMemcpyDeviceToHost));
    if (filled) *filled = n[0];
    if (fallback) *fallback = n[1];
    return MCPT_OK;
}

}  // namespace

// mcpt_internal.h: the temporal upsampling for a caller that owns every buffer (sequence.hip)
namespace mcpt {

int temporal_upsample_enqueue(const mcpt_temporal_opts* tp, const mcpt_upsample_opts* up, int32_t a, int32_t b,
                              const mcpt_camera* pc, int32_t w, int32_t h, const double* dC, const mcpt_aov_buffers* G,
                              const mcpt_aov_buffers* pG, const double* dpC, const double* dpM, double* dOut, double* dOutM,
                              double* dOutV, unsigned long long* dCounts) {
    int rc;
    bool has_prev = false;
    if ((rc = check_call(tp, up, a, b, pc, w, h, dC, G, pG, dpC, dpM, dOut, dOutM, dOutV, &has_prev))) return rc;
    if (!dCounts) {
        set_error("null argument: the filled and fallback counters");
        return MCPT_E_INVALID;
    }
    return enqueue(tp, up, a, b, has_prev ? pc : nullptr, w, h, dC, G, pG, dpC, dpM, dOut, dOutM, dOutV, dCounts);
}

}  // namespace mcpt

extern "C" {

int mcpt_upsample_phase(int32_t factor, uint64_t frame_index, int32_t* a, int32_t* b) {
    if (!a || !b) {
        set_error("mcpt_upsample_phase: null argument: %s", !a ? "a" : "b");
        return MCPT_E_INVALID;
    }
    if (factor < 2 || factor > 4) {
        set_error("mcpt_upsample_phase: factor %d is outside 2..4", factor);
        return MCPT_E_INVALID;
    }
    const int k = (int)(frame_index % (uint64_t)(factor * factor));
    *a = k % factor;
    *b = (*a + k / factor) % factor;
    return MCPT_OK;
}

int mcpt_temporal_upsample_device(const mcpt_temporal_opts* tp, const mcpt_upsample_opts* up, int32_t a, int32_t b,
                                  const mcpt_camera* pc, int32_t w, int32_t h, const double* dC, const mcpt_aov_buffers* G,
                                  const mcpt_aov_buffers* pG, const double* dpC, const double* dpM, double* dOut, double* dOutM,
                                  double* dOutV, uint64_t* filled, uint64_t* fallback, double* seconds) {
    int rc;
    bool has_prev = false;
    if ((rc = check_call(tp, up, a, b, pc, w, h, dC, G, pG, dpC, dpM, dOut, dOutM, dOutV, &has_prev))) return rc;
    Scratch S;
    int device;
    if ((rc = select_device(tp->device, S, &device))) return rc;
    if ((rc = check_device_array(dC, device, "dev_color")) || (rc = check_device_array(G->albedo, device, "dev_full_guides.albedo")) ||
        (rc = check_device_array(G->normal, device, "dev_full_guides.normal")) ||
        (rc = check_device_array(G->position, device, "dev_full_guides.position")) ||
        (rc = check_device_array(G->depth, device, "dev_full_guides.depth")) ||
        (rc = check_device_array(dOut, device, "dev_out_color")) || (rc = check_device_array(dOutM, device, "dev_out_moments")) ||
        (dOutV && (rc = check_device_array(dOutV, device, "dev_out_variance"))))
        return rc;
    if (has_prev && ((rc = check_device_array(pG->normal, device, "dev_prev_full_guides.normal")) ||
                     (rc = check_device_array(pG->position, device, "dev_prev_full_guides.position")) ||
                     (rc = check_device_array(pG->depth, device, "dev_prev_full_guides.depth")) ||
                     (rc = check_device_array(dpC, device, "dev_prev_color")) ||
                     (rc = check_device_array(dpM, device, "dev_prev_moments"))))
        return rc;
    DN_HIP_OK(hipMalloc(&S.p, 2 * sizeof(unsigned long long)));
    // the caller's arrays may still be written by work on other streams (e.g. torch's)
    DN_HIP_OK(hipDeviceSynchronize());
    return run(tp, up, a, b, has_prev ? pc : nullptr, w, h, dC, G, pG, dpC, dpM, dOut, dOutM, dOutV, (unsigned long long*)S.p, S,
               filled, fallback, seconds);
}

int mcpt_temporal_upsample(const mcpt_temporal_opts* tp, const mcpt_upsample_opts* up, int32_t a, int32_t b,
                           const mcpt_camera* pc, int32_t w, int32_t h, const double* color, const mcpt_aov_buffers* G,
                           const mcpt_aov_buffers* pG, const double* pcol, const double* pmom, double* out, double* outm,
                           double* outv, uint64_t* filled, uint64_t* fallback, double* seconds) {
    int rc;
    bool has_prev = false;
    if ((rc = check_call(tp, up, a, b, pc, w, h, color, G, pG, pcol, pmom, out, outm, outv, &has_prev))) return rc;
    Scratch S;
    int device;
    if ((rc = select_device(tp->device, S, &device))) return rc;
    const size_t npx = (size_t)w * h, NPX = npx * up->factor * up->factor, B = sizeof(double);
    // the counts' two words, the low colour 3; full size: guides 3 + 3 + 3 + 1, out colour 3, moments 4, variance 1, then
    // the previous state 3 + 3 + 1 + 3 + 4
    DN_HIP_OK(hipMalloc(&S.p, (2 + 3 * npx + (has_prev ? 32 : 18) * NPX) * B));
    double* dC = S.p + 2;
    double* F = dC + 3 * npx;
    const mcpt_aov_buffers dG{F, F + 3 * NPX, F + 6 * NPX, F + 9 * NPX};
    double* dOut = F + 10 * NPX;
    double* dOutM = dOut + 3 * NPX;
    double* dOutV = dOutM + 4 * NPX;
    double* prev = has_prev ? dOutV + NPX : nullptr;  // only then does the allocation reach that far
    const mcpt_aov_buffers dpG{nullptr, prev, prev ? prev + 3 * NPX : nullptr, prev ? prev + 6 * NPX : nullptr};
    double* dpC = prev ? prev + 7 * NPX : nullptr;
    double* dpM = prev ? dpC + 3 * NPX : nullptr;
    DN_HIP_OK(hipMemcpy(dC, color, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dG.albedo, G->albedo, 3 * NPX * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dG.normal, G->normal, 3 * NPX * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dG.position, G->position, 3 * NPX * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dG.depth, G->depth, NPX * B, hipMemcpyHostToDevice));
    if (has_prev) {
        DN_HIP_OK(hipMemcpy(dpG.normal, pG->normal, 3 * NPX * B, hipMemcpyHostToDevice));
        DN_HIP_OK(hipMemcpy(dpG.position, pG->position, 3 * NPX * B, hipMemcpyHostToDevice));
        DN_HIP_OK(hipMemcpy(dpG.depth, pG->depth, NPX * B, hipMemcpyHostToDevice));
        DN_HIP_OK(hipMemcpy(dpC, pcol, 3 * NPX * B, hipMemcpyHostToDevice));
        DN_HIP_OK(hipMemcpy(dpM, pmom, 4 * NPX * B, hipMemcpyHostToDevice));
    }
    if ((rc = run(tp, up, a, b, has_prev ? pc : nullptr, w, h, dC, &dG, &dpG, dpC, dpM, dOut, dOutM, outv ? dOutV : nullptr,
                  (unsigned long long*)S.p, S, filled, fallback, seconds)))
        return rc;
    DN_HIP_OK(hipMemcpy(out, dOut, 3 * NPX * B, hipMemcpyDeviceToHost));
    DN_HIP_OK(hipMemcpy(outm, dOutM, 4 * NPX * B, hipMemcpyDeviceToHost));
    if (outv) DN_HIP_OK(hipMemcpy(outv, dOutV, NPX * B, hipMemcpyDeviceToHost));
    return MCPT_OK;
}

}  // extern "C"
