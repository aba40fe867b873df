// Temporal accumulation for gfx950 (mcpt_temporal_accumulate, mcpt_temporal_accumulate_clamped,
// mcpt_temporal_accumulate_motion and mcpt_temporal_accumulate_antilag, include/mcpt.h states the rules in full) and the
// host helper mcpt_camera_orbit.  No counterpart in the reference.
//
//   k_temporal_accumulate  lane per pixel : reproject, gather the four taps of the previous history, blend,
//                                           and the temporal variance where the history is long enough; the
//                                           <true, *> instantiations (the clamped call) gather and blend the fast
//                                           history with the same taps and leaves the variance to the clamp
//   k_temporal_clamp       lane per pixel : (the clamped call) mean and standard deviation of the fast history over
//                                           the hit taps of the clipped window (an LDS tile), two passes; clamps
//                                           the blended colour in place, corrects the moments, writes the shift
//                                           and the temporal variance; lanes without history leave early
//   k_temporal_spatial     lane per pixel : V_0 of the a-trous filter on the blended colour, only in lanes whose
//                                           history is short (the others leave at once)
//
// The <*, true> instantiations (mcpt_temporal_accumulate_motion) take the reprojected point and the normal of the tap tests
// from the motion AOVs (the surface point's previous position and normal) instead of the current guides: three
// substitutions, two more pointers in TpParams, 6 doubles more read per pixel; everything else is the same code.
//
// The <*, *, true> instantiations (mcpt_temporal_accumulate_antilag) read one double more per pixel with a history -- the
// Lambda of the stratum its source falls in (temporal_gradient.hip writes that map) -- and raise the blend weights by
// it: one pointer and two ints more in TpParams.  The <*, *, false> instantiations are the code they were (DESIGN.md
// 4.25 compares their resource usage).
//
// Everything is fp64 with -ffp-contract=off, so a numpy restatement of the rule reproduces the output to
// rounding (tests/test_temporal.py).  A block is 64 x 4 pixels as in denoise.hip: the centre's loads and the
// stores are consecutive across a wave; the four gathers follow the reprojection, which keeps neighbours
// together under a camera move.  The centre's guides stay in registers for the four taps.  Plain loads and
// stores only: no atomics, and no LDS outside k_temporal_clamp.  Per pixel the first kernel reads 10 doubles of
// its own (colour, normal, position, depth), up to 4 x 14 of the previous frame (depth, moments, normal, position,
// colour; neighbouring lanes share them in cache) and writes 8: about 0.5 KB (the clamped call: 4 x 3 more read
// and 4 more written).
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
    // the clamped call only
    int radius;
    double alpha_fast, sigma;
    const double* pF;
    double *outF, *outS;  // outS: k_temporal_accumulate<true> leaves "has a history" (1 or 0), k_temporal_clamp the shift
    // the motion call only: the previous position and normal of every pixel's surface point
    const double *mX, *mN;
    // the anti-lag call only: the hs x ws map of Lambda, its stratum and its row length
    const double* lam;
    int stratum, lam_ws;
};

__device__ inline bool temporal_variance_applies(const TpParams& P, double n, double g) { return n > P.var_n && g < 1.0; }

template <bool FAST, bool MOTION, bool ANTILAG>
__global__ __launch_bounds__(kBx* kBy) void k_temporal_accumulate(TpParams P) {
    const int x = blockIdx.x * kBx + threadIdx.x, y = blockIdx.y * kBy + threadIdx.y;
    if (x >= P.W || y >= P.H) return;
    const size_t p = (size_t)y * P.W + x;
    const double c0 = P.C[3 * p], c1 = P.C[3 * p + 1], c2 = P.C[3 * p + 2];
    const double l = (c0 + c1 + c2) / 3.0;
    const double depth = P.depth[p];
    double wsum = 0.0, h0 = 0.0, h1 = 0.0, h2 = 0.0, m1 = 0.0, m2 = 0.0, hn = 0.0, hg = 0.0;
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;  // FAST: the fast history's gather
    bool source = false;
    double lam = 0.0;  // ANTILAG: the source stratum's Lambda, clamped to [0, 1]
    if (P.has_prev && depth > 0) {
        // MOTION: the source and the taps' normal and plane tests take the point where it was a frame ago
        const double* pn = MOTION ? P.mN : P.N;
        const double* px = MOTION ? P.mX : P.X;
        const double N0 = pn[3 * p], N1 = pn[3 * p + 1], N2 = pn[3 * p + 2];
        const double X0 = px[3 * p], X1 = px[3 * p + 1], X2 = px[3 * p + 2];
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
                if (ANTILAG) {  // the stratum of the nearest previous pixel
                    const int li = min(max((int)floor(ys + 0.5), 0), P.H - 1), lj = min(max((int)floor(xs + 0.5), 0), P.W - 1);
                    const double L = P.lam[(size_t)(li / P.stratum) * P.lam_ws + lj / P.stratum];
                    lam = L > 0 ? (L < 1 ? L : 1.0) : 0.0;
                }
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
                    if (FAST) {
                        f0 += bq * P.pF[3 * q];
                        f1 += bq * P.pF[3 * q + 1];
                        f2 += bq * P.pF[3 * q + 2];
                    }
                }
            }
        }
    }
    double o0 = c0, o1 = c1, o2 = c2, om1 = l, om2 = l * l, on = 1.0, og = 1.0;
    const bool history = source && wsum >= P.min_weight;
    double nb = 1.0;  // the history length the blend weights are taken from (ANTILAG: on is then n_out)
    if (history) {
        nb = on = fmin(hn / wsum + 1.0, P.max_history);
        double A = fmax(P.alpha, 1.0 / on);
        if (ANTILAG) {
            A = A + lam * (1.0 - A);
            on = (1.0 - lam) * nb + lam;
        }
        const double B = 1.0 - A;
        o0 = B * (h0 / wsum) + A * c0;
        o1 = B * (h1 / wsum) + A * c1;
        o2 = B * (h2 / wsum) + A * c2;
        om1 = B * (m1 / wsum) + A * l;
        om2 = B * (m2 / wsum) + A * (l * l);
        og = B * B * (hg / wsum) + A * A;
    }
    P.outC[3 * p] = o0, P.outC[3 * p + 1] = o1, P.outC[3 * p + 2] = o2;
    P.outM[4 * p] = om1, P.outM[4 * p + 1] = om2, P.outM[4 * p + 2] = on, P.outM[4 * p + 3] = og;
    if (FAST) {  // the variance waits for the clamped colour and the corrected moments (k_temporal_clamp)
        double F0 = c0, F1 = c1, F2 = c2;
        if (history) {
            double A = fmax(P.alpha_fast, 1.0 / nb);
            if (ANTILAG) A = A + lam * (1.0 - A);
            const double B = 1.0 - A;
            F0 = B * (f0 / wsum) + A * c0;
            F1 = B * (f1 / wsum) + A * c1;
            F2 = B * (f2 / wsum) + A * c2;
        }
        P.outF[3 * p] = F0, P.outF[3 * p + 1] = F1, P.outF[3 * p + 2] = F2;
        P.outS[p] = history ? 1.0 : 0.0;
        return;
    }
    if (P.outV && temporal_variance_applies(P, on, og)) P.outV[p] = fmax(0.0, om2 - om1 * om1) * og / (1.0 - og);
}

// The clamp of the clamped call, in place on outC / outM after k_temporal_accumulate<true>: neighbours are read from
// outF and depth only, which no lane of this kernel writes.  The block first copies its (64 + 2 r) x (4 + 2 r) window
// of outF and depth into LDS: four planes (F.r, F.g, F.b, depth), so consecutive lanes read consecutive doubles;
// 22 KB at the largest radius, which leaves seven blocks to a CU.  Pixels outside the frame enter as misses.  On
// the MI355X the tile beat direct global reads of the window.  Each tap is read twice (mean, then
// deviations) instead of held in up to 3 * 49 registers.
constexpr int kClampRmax = 3, kTw = kBx + 2 * kClampRmax, kTh = kBy + 2 * kClampRmax, kPlane = kTw * kTh;

__global__ __launch_bounds__(kBx* kBy) void k_temporal_clamp(TpParams P) {
    __shared__ double tile[4 * kPlane];
    const int x = blockIdx.x * kBx + threadIdx.x, y = blockIdx.y * kBy + threadIdx.y;
    const int bx0 = blockIdx.x * kBx - P.radius, by0 = blockIdx.y * kBy - P.radius;
    const int tw = kBx + 2 * P.radius, th = kBy + 2 * P.radius;
    for (int t = threadIdx.y * kBx + threadIdx.x; t < tw * th; t += kBx * kBy) {
        const int ty = t / tw, tx = t - ty * tw, gx = bx0 + tx, gy = by0 + ty;
        double d = 0.0, a0 = 0.0, a1 = 0.0, a2 = 0.0;
        if (gx >= 0 && gx < P.W && gy >= 0 && gy < P.H) {
            const size_t q = (size_t)gy * P.W + gx;
            d = P.depth[q], a0 = P.outF[3 * q], a1 = P.outF[3 * q + 1], a2 = P.outF[3 * q + 2];
        }
        const int e = ty * kTw + tx;
        tile[e] = a0, tile[kPlane + e] = a1, tile[2 * kPlane + e] = a2, tile[3 * kPlane + e] = d;
    }
    __syncthreads();
    if (x >= P.W || y >= P.H) return;
    const size_t p = (size_t)y * P.W + x;
    if (P.outS[p] == 0.0) return;  // no history: colour, moments and a shift of 0 are already in place
    const int y0 = max(y - P.radius, 0) - by0, y1 = min(y + P.radius, P.H - 1) - by0;  // the clipped window, in the tile
    const int x0 = max(x - P.radius, 0) - bx0, x1 = min(x + P.radius, P.W - 1) - bx0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, cnt = 0.0;
    for (int ty = y0; ty <= y1; ty++)
        for (int tx = x0; tx <= x1; tx++) {
            const int e = ty * kTw + tx;
            if (!(tile[3 * kPlane + e] > 0)) continue;
            cnt += 1.0;
            s0 += tile[e], s1 += tile[kPlane + e], s2 += tile[2 * kPlane + e];
        }
    const double mu0 = s0 / cnt, mu1 = s1 / cnt, mu2 = s2 / cnt;  // cnt >= 1: p itself is a hit
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;
    for (int ty = y0; ty <= y1; ty++)
        for (int tx = x0; tx <= x1; tx++) {
            const int e = ty * kTw + tx;
            if (!(tile[3 * kPlane + e] > 0)) continue;
            const double e0 = tile[e] - mu0, e1 = tile[kPlane + e] - mu1, e2 = tile[2 * kPlane + e] - mu2;
            v0 += e0 * e0, v1 += e1 * e1, v2 += e2 * e2;
        }
    const double w0 = P.sigma * sqrt(v0 / cnt), w1 = P.sigma * sqrt(v1 / cnt), w2 = P.sigma * sqrt(v2 / cnt);
    const double S0 = P.outC[3 * p], S1 = P.outC[3 * p + 1], S2 = P.outC[3 * p + 2];
    const double o0 = fmin(fmax(S0, mu0 - w0), mu0 + w0);
    const double o1 = fmin(fmax(S1, mu1 - w1), mu1 + w1);
    const double o2 = fmin(fmax(S2, mu2 - w2), mu2 + w2);
    const double shift = (o0 + o1 + o2) / 3.0 - (S0 + S1 + S2) / 3.0;
    const double m1 = P.outM[4 * p], om1 = m1 + shift, om2 = P.outM[4 * p + 1] + (om1 * om1 - m1 * m1);
    const double on = P.outM[4 * p + 2], og = P.outM[4 * p + 3];
    P.outC[3 * p] = o0, P.outC[3 * p + 1] = o1, P.outC[3 * p + 2] = o2;
    P.outM[4 * p] = om1, P.outM[4 * p + 1] = om2;
    P.outS[p] = shift;
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

// the clamped call's extra arguments (clamp == nullptr: the plain call, the other three are NULL)
struct ClampArgs {
    const mcpt_temporal_clamp_opts* clamp;
    const double* pfast;
    double *outf, *outs;
};

// the anti-lag call's extra arguments (g == nullptr: every other call)
struct AntilagArgs {
    const mcpt_gradient_opts* g;
    const double* lam;
};

// the option structs' checks (c is looked at only when clamped); mcpt::temporal_check_opts is this function
int check_opts(const mcpt_temporal_opts* o, const mcpt_temporal_clamp_opts* c, bool clamped) {
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
    if (clamped) {
        if (!c) {
            set_error("null mcpt_temporal_clamp_opts (clamp)");
            return MCPT_E_INVALID;
        }
        if (c->struct_size != sizeof(mcpt_temporal_clamp_opts)) {
            set_error("mcpt_temporal_clamp_opts.struct_size is %u, this library expects %zu (use "
                      "mcpt_temporal_clamp_opts_init / the mcpt.h of MCPT_VERSION %d)", c->struct_size,
                      sizeof(mcpt_temporal_clamp_opts), MCPT_VERSION);
            return MCPT_E_INVALID;
        }
        if (c->radius < 1 || c->radius > 3) {
            set_error("invalid clamp options: radius %d is outside 1..3", c->radius);
            return MCPT_E_INVALID;
        }
        if (!(c->alpha_fast > 0 && c->alpha_fast <= 1)) {
            set_error("invalid clamp options: alpha_fast %g is outside (0, 1]", c->alpha_fast);
            return MCPT_E_INVALID;
        }
        if (!std::isfinite(c->sigma) || !(c->sigma >= 0)) {
            set_error("invalid clamp options: sigma %g must be finite and >= 0", c->sigma);
            return MCPT_E_INVALID;
        }
    }
    return MCPT_OK;
}

// every check a call makes before it touches a device; *has_prev: the previous state is given
int check_call(const mcpt_temporal_opts* o, const mcpt_camera* pc, int W, int H, const double* color, const mcpt_aov_buffers* g,
               const mcpt_aov_buffers* pg, const double* pcol, const double* pmom, const double* out, const double* outm,
               const double* outv, bool* has_prev, bool clamped = false, const ClampArgs& ca = ClampArgs{},
               bool with_motion = false, const mcpt_motion_buffers* mo = nullptr, bool antilag = false,
               const AntilagArgs& al = AntilagArgs{}) {
    int orc;
    if ((orc = check_opts(o, ca.clamp, clamped))) return orc;
    if (antilag) {
        if (!al.g || !al.lam) {
            set_error("null argument: %s", !al.g ? "gradient" : "lambda");
            return MCPT_E_INVALID;
        }
        if ((orc = mcpt::gradient_check_opts(al.g))) return orc;
    }
    if (W < 1 || H < 1 || (long long)W * H > (1ll << 28)) {
        set_error("invalid frame size: width %d, height %d", W, H);
        return MCPT_E_INVALID;
    }
    if (!color || !out || !outm) {
        set_error("null argument: %s", !color ? "color" : !out ? "out_color" : "out_moments");
        return MCPT_E_INVALID;
    }
    if (clamped && !ca.outf) {
        set_error("null argument: out_fast");
        return MCPT_E_INVALID;
    }
    if (!g || !g->albedo || !g->normal || !g->position || !g->depth) {
        set_error("null argument: guides (%s); all four guide arrays are required",
                  !g ? "the struct" : !g->albedo ? "albedo" : !g->normal ? "normal" : !g->position ? "position" : "depth");
        return MCPT_E_INVALID;
    }
    if (with_motion && (!mo || !mo->prev_position || !mo->prev_normal)) {
        set_error("null argument: motion (%s); both motion arrays are required",
                  !mo ? "the struct" : !mo->prev_position ? "prev_position" : "prev_normal");
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
    if (clamped && *has_prev != (ca.pfast != nullptr)) {
        set_error("partial previous state: prev_fast is %s (the fast history belongs to the previous state: pass it with "
                  "prev_cam, prev_guides, prev_color and prev_moments, or none of them)",
                  ca.pfast ? "given while the rest of the previous state is NULL" : "NULL while the rest of the previous state is given");
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
    const size_t nlam = antilag ? (size_t)((H + al.g->stratum - 1) / al.g->stratum) * ((W + al.g->stratum - 1) / al.g->stratum) : 0;
    const Range ins[] = {{"color", color, 3 * npx},
                         {"guides.albedo", g->albedo, 3 * npx},
                         {"guides.normal", g->normal, 3 * npx},
                         {"guides.position", g->position, 3 * npx},
                         {"guides.depth", g->depth, npx},
                         {"prev_guides.normal", *has_prev ? pg->normal : nullptr, 3 * npx},
                         {"prev_guides.position", *has_prev ? pg->position : nullptr, 3 * npx},
                         {"prev_guides.depth", *has_prev ? pg->depth : nullptr, npx},
                         {"prev_color", pcol, 3 * npx},
                         {"prev_moments", pmom, 4 * npx},
                         {"prev_fast", ca.pfast, 3 * npx},
                         {"motion.prev_position", with_motion ? mo->prev_position : nullptr, 3 * npx},
                         {"motion.prev_normal", with_motion ? mo->prev_normal : nullptr, 3 * npx},
                         {"lambda", antilag ? al.lam : nullptr, nlam}},
                outs[] = {{"out_color", out, 3 * npx}, {"out_moments", outm, 4 * npx}, {"out_variance", outv, npx},
                          {"out_fast", ca.outf, 3 * npx}, {"out_shift", ca.outs, npx}};  // NULL: overlaps nothing
    for (const auto& w : outs)
        for (const auto& r : ins)
            if (overlap(w, r)) {
                set_error("%s is aliasing %s: the accumulation cannot run in place (swap two sets of history buffers)",
                          w.name, r.name);
                return MCPT_E_INVALID;
            }
    for (int a = 0; a < 5; a++)
        for (int b = a + 1; b < 5; b++)
            if (overlap(outs[a], outs[b])) {
                set_error("%s is aliasing %s", outs[a].name, outs[b].name);
                return MCPT_E_INVALID;
            }
    return MCPT_OK;
}

// the kernels over device arrays, enqueued on the null stream; ca (the clamped call): its device arrays, outs never NULL;
// mo (the motion call): its two device arrays
int enqueue_accumulate(const mcpt_temporal_opts* o, const mcpt_camera* pc, int W, int H, const double* dC, const mcpt_aov_buffers* g,
                       const mcpt_aov_buffers* pg, const double* dpC, const double* dpM, double* dOut, double* dOutM,
                       double* dOutV, const ClampArgs* ca, const mcpt_motion_buffers* mo = nullptr, const AntilagArgs* al = nullptr) {
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
    if (ca) {
        P.radius = ca->clamp->radius, P.alpha_fast = ca->clamp->alpha_fast, P.sigma = ca->clamp->sigma;
        P.pF = ca->pfast, P.outF = ca->outf, P.outS = ca->outs;
    }
    const DnParams D{W, H, 0.0, o->sigma_normal, o->sigma_plane, o->sigma_albedo, g->albedo, g->normal, g->position, g->depth};
    const dim3 grid((W + kBx - 1) / kBx, (H + kBy - 1) / kBy), block(kBx, kBy);
    if (mo) P.mX = mo->prev_position, P.mN = mo->prev_normal;
    if (al) P.lam = al->lam, P.stratum = al->g->stratum, P.lam_ws = (W + al->g->stratum - 1) / al->g->stratum;
    if (ca) {
        if (al) {
            if (mo) hipLaunchKernelGGL((k_temporal_accumulate<true, true, true>), grid, block, 0, nullptr, P);
            else hipLaunchKernelGGL((k_temporal_accumulate<true, false, true>), grid, block, 0, nullptr, P);
        } else {
            if (mo) hipLaunchKernelGGL((k_temporal_accumulate<true, true, false>), grid, block, 0, nullptr, P);
            else hipLaunchKernelGGL((k_temporal_accumulate<true, false, false>), grid, block, 0, nullptr, P);
        }
        DN_HIP_OK(hipGetLastError());
        if (P.has_prev) hipLaunchKernelGGL(k_temporal_clamp, grid, block, 0, nullptr, P);  // else no pixel has a history
    } else if (al) {
        if (mo) hipLaunchKernelGGL((k_temporal_accumulate<false, true, true>), grid, block, 0, nullptr, P);
        else hipLaunchKernelGGL((k_temporal_accumulate<false, false, true>), grid, block, 0, nullptr, P);
    } else {
        if (mo) hipLaunchKernelGGL((k_temporal_accumulate<false, true, false>), grid, block, 0, nullptr, P);
        else hipLaunchKernelGGL((k_temporal_accumulate<false, false, false>), grid, block, 0, nullptr, P);
    }
    DN_HIP_OK(hipGetLastError());
    if (dOutV) {
        hipLaunchKernelGGL(k_temporal_spatial, grid, block, 0, nullptr, P, D);
        DN_HIP_OK(hipGetLastError());
    }
    return MCPT_OK;
}

// the same, timed with two events and waited for
int run_accumulate(const mcpt_temporal_opts* o, const mcpt_camera* pc, int W, int H, const double* dC, const mcpt_aov_buffers* g,
                   const mcpt_aov_buffers* pg, const double* dpC, const double* dpM, double* dOut, double* dOutM,
                   double* dOutV, Scratch& S, double* seconds, const ClampArgs* ca = nullptr, const mcpt_motion_buffers* mo = nullptr,
                   const AntilagArgs* al = nullptr) {
    int rc;
    DN_HIP_OK(hipEventCreate(&S.e0));
    DN_HIP_OK(hipEventCreate(&S.e1));
    DN_HIP_OK(hipEventRecord(S.e0, nullptr));
    if ((rc = enqueue_accumulate(o, pc, W, H, dC, g, pg, dpC, dpM, dOut, dOutM, dOutV, ca, mo, al))) return rc;
    DN_HIP_OK(hipEventRecord(S.e1, nullptr));
    DN_HIP_OK(hipEventSynchronize(S.e1));
    float ms = 0;
    DN_HIP_OK(hipEventElapsedTime(&ms, S.e0, S.e1));
    if (seconds) *seconds = ms * 1e-3;
    return MCPT_OK;
}

}  // namespace

// mcpt_internal.h: the accumulation for a caller that owns every buffer (sequence.hip)
namespace mcpt {

int temporal_check_opts(const mcpt_temporal_opts* o, const mcpt_temporal_clamp_opts* clamp, bool clamped) {
    return check_opts(o, clamp, clamped);
}

int temporal_enqueue(const mcpt_temporal_opts* o, const mcpt_camera* pc, int32_t W, int32_t H, const double* dC,
                     const mcpt_aov_buffers* g, const mcpt_aov_buffers* pg, const double* dpC, const double* dpM, double* dOut,
                     double* dOutM, double* dOutV, const TemporalClampIo* io, const mcpt_motion_buffers* motion,
                     const TemporalAntilagIo* antilag) {
    int rc;
    bool has_prev = false;
    const ClampArgs ca = io ? ClampArgs{io->clamp, io->prev_fast, io->out_fast, io->out_shift} : ClampArgs{};
    const AntilagArgs al = antilag ? AntilagArgs{antilag->gradient, antilag->lambda} : AntilagArgs{};
    if ((rc = check_call(o, pc, W, H, dC, g, pg, dpC, dpM, dOut, dOutM, dOutV, &has_prev, io != nullptr, ca, motion != nullptr, motion,
                         antilag != nullptr, al)))
        return rc;
    if (io && !io->out_shift) {  // the kernels pass "has a history" through it: the caller's scratch
        set_error("null argument: out_shift (required by the caller-owned form)");
        return MCPT_E_INVALID;
    }
    return enqueue_accumulate(o, has_prev ? pc : nullptr, W, H, dC, g, pg, dpC, dpM, dOut, dOutM, dOutV, io ? &ca : nullptr, motion,
                              antilag ? &al : nullptr);
}

int temporal_spatial_enqueue(const mcpt_temporal_opts* o, int32_t W, int32_t H, const mcpt_aov_buffers* g, const double* dOutC,
                             const double* dOutM, double* dOutV) {
    TpParams P{};  // what k_temporal_spatial reads of it
    P.W = W, P.H = H;
    P.var_n = o->variance_min_history - 0.5;
    P.outC = const_cast<double*>(dOutC), P.outM = const_cast<double*>(dOutM), P.outV = dOutV;
    const DnParams D{W, H, 0.0, o->sigma_normal, o->sigma_plane, o->sigma_albedo, g->albedo, g->normal, g->position, g->depth};
    const dim3 grid((W + kBx - 1) / kBx, (H + kBy - 1) / kBy), block(kBx, kBy);
    hipLaunchKernelGGL(k_temporal_spatial, grid, block, 0, nullptr, P, D);
    DN_HIP_OK(hipGetLastError());
    return MCPT_OK;
}

}  // namespace mcpt

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

// the device forms; ca: the clamped call's arguments, nullptr for the plain call; with_motion: the motion call, mo its arrays
static int accumulate_device(const mcpt_temporal_opts* o, const mcpt_camera* pc, int32_t W, int32_t H, const double* dC,
                             const mcpt_aov_buffers* g, const mcpt_aov_buffers* pg, const double* dpC, const double* dpM,
                             double* dOut, double* dOutM, double* dOutV, double* seconds, const ClampArgs* ca,
                             bool with_motion = false, const mcpt_motion_buffers* mo = nullptr, const AntilagArgs* al = nullptr) {
    int rc;
    bool has_prev = false;
    if ((rc = check_call(o, pc, W, H, dC, g, pg, dpC, dpM, dOut, dOutM, dOutV, &has_prev, ca != nullptr, ca ? *ca : ClampArgs{},
                         with_motion, mo, al != nullptr, al ? *al : AntilagArgs{})))
        return rc;
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
    if (with_motion && ((rc = check_device_array(mo->prev_position, device, "dev_motion.prev_position")) ||
                        (rc = check_device_array(mo->prev_normal, device, "dev_motion.prev_normal"))))
        return rc;
    if (al && (rc = check_device_array(al->lam, device, "dev_lambda"))) return rc;
    ClampArgs dca{};
    if (ca) {
        if ((rc = check_device_array(ca->outf, device, "dev_out_fast")) ||
            (ca->outs && (rc = check_device_array(ca->outs, device, "dev_out_shift"))) ||
            (has_prev && (rc = check_device_array(ca->pfast, device, "dev_prev_fast"))))
            return rc;
        dca = *ca;
        if (!dca.outs) {  // the kernels pass "has a history" through it
            DN_HIP_OK(hipMalloc(&S.p, (size_t)W * H * sizeof(double)));
            dca.outs = S.p;
        }
    }
    // the caller's arrays may still be written by work on other streams (e.g. torch's)
    DN_HIP_OK(hipDeviceSynchronize());
    return run_accumulate(o, has_prev ? pc : nullptr, W, H, dC, g, pg, dpC, dpM, dOut, dOutM, dOutV, S, seconds, ca ? &dca : nullptr,
                          with_motion ? mo : nullptr, al);
}

// the host forms
static int accumulate_host(const mcpt_temporal_opts* o, const mcpt_camera* pc, int32_t W, int32_t H, const double* color,
                           const mcpt_aov_buffers* g, const mcpt_aov_buffers* pg, const double* pcol, const double* pmom,
                           double* out, double* outm, double* outv, double* seconds, const ClampArgs* ca,
                           bool with_motion = false, const mcpt_motion_buffers* mo = nullptr, const AntilagArgs* al = nullptr) {
    int rc;
    bool has_prev = false;
    if ((rc = check_call(o, pc, W, H, color, g, pg, pcol, pmom, out, outm, outv, &has_prev, ca != nullptr, ca ? *ca : ClampArgs{},
                         with_motion, mo, al != nullptr, al ? *al : AntilagArgs{})))
        return rc;
    Scratch S;
    int device;
    if ((rc = select_device(o->device, S, &device))) return rc;
    const size_t npx = (size_t)W * H, B = sizeof(double);
    // colour 3, guides 3 + 3 + 3 + 1, out colour 3, moments 4, variance 1, then the previous state 3 + 3 + 1 + 3 + 4,
    // then the clamped call's fast history 3, shift 1 and previous fast history 3, then the motion call's two maps 3 + 3,
    // then the anti-lag call's Lambda (hs * ws)
    const size_t nlam = al ? (size_t)((H + al->g->stratum - 1) / al->g->stratum) * ((W + al->g->stratum - 1) / al->g->stratum) : 0;
    const size_t nfix = ((has_prev ? 35 : 21) + (ca ? 7 : 0) + (with_motion ? 6 : 0)) * npx;
    DN_HIP_OK(hipMalloc(&S.p, (nfix + nlam) * B));
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
    ClampArgs dca{};
    if (ca) {
        dca.clamp = ca->clamp;
        dca.outf = S.p + (has_prev ? 35 : 21) * npx, dca.outs = dca.outf + 3 * npx;
        if (has_prev) {
            double* dpF = dca.outs + npx;
            DN_HIP_OK(hipMemcpy(dpF, ca->pfast, 3 * npx * B, hipMemcpyHostToDevice));
            dca.pfast = dpF;
        }
    }
    mcpt_motion_buffers dmo{};
    if (with_motion) {
        dmo.prev_position = S.p + ((has_prev ? 35 : 21) + (ca ? 7 : 0)) * npx, dmo.prev_normal = dmo.prev_position + 3 * npx;
        DN_HIP_OK(hipMemcpy(dmo.prev_position, mo->prev_position, 3 * npx * B, hipMemcpyHostToDevice));
        DN_HIP_OK(hipMemcpy(dmo.prev_normal, mo->prev_normal, 3 * npx * B, hipMemcpyHostToDevice));
    }
    AntilagArgs dal{};
    if (al) {
        dal.g = al->g, dal.lam = S.p + nfix;
        DN_HIP_OK(hipMemcpy(S.p + nfix, al->lam, nlam * B, hipMemcpyHostToDevice));
    }
    if ((rc = run_accumulate(o, has_prev ? pc : nullptr, W, H, dC, &dg, &dpg, dpC, dpM, dOut, dOutM, outv ? dOutV : nullptr, S,
                             seconds, ca ? &dca : nullptr, with_motion ? &dmo : nullptr, al ? &dal : nullptr)))
        return rc;
    if (ca) {
        DN_HIP_OK(hipMemcpy(ca->outf, dca.outf, 3 * npx * B, hipMemcpyDeviceToHost));
        if (ca->outs) DN_HIP_OK(hipMemcpy(ca->outs, dca.outs, npx * B, hipMemcpyDeviceToHost));
    }
    DN_HIP_OK(hipMemcpy(out, dOut, 3 * npx * B, hipMemcpyDeviceToHost));
    DN_HIP_OK(hipMemcpy(outm, dOutM, 4 * npx * B, hipMemcpyDeviceToHost));
    if (outv) DN_HIP_OK(hipMemcpy(outv, dOutV, npx * B, hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_temporal_accumulate_device(const mcpt_temporal_opts* o, const mcpt_camera* pc, int32_t W, int32_t H, const double* dC,
                                    const mcpt_aov_buffers* g, const mcpt_aov_buffers* pg, const double* dpC, const double* dpM,
                                    double* dOut, double* dOutM, double* dOutV, double* seconds) {
    return accumulate_device(o, pc, W, H, dC, g, pg, dpC, dpM, dOut, dOutM, dOutV, seconds, nullptr);
}

int mcpt_temporal_accumulate(const mcpt_temporal_opts* o, const mcpt_camera* pc, int32_t W, int32_t H, const double* color,
                             const mcpt_aov_buffers* g, const mcpt_aov_buffers* pg, const double* pcol, const double* pmom,
                             double* out, double* outm, double* outv, double* seconds) {
    return accumulate_host(o, pc, W, H, color, g, pg, pcol, pmom, out, outm, outv, seconds, nullptr);
}

void mcpt_temporal_clamp_opts_init(mcpt_temporal_clamp_opts* c) {
    if (!c) return;
    std::memset((void*)c, 0, sizeof *c);
    c->struct_size = sizeof *c;
    c->radius = 2;
    c->alpha_fast = 0.5;
    c->sigma = 2.0;
}

int mcpt_temporal_accumulate_clamped_device(const mcpt_temporal_opts* o, const mcpt_temporal_clamp_opts* clamp, const mcpt_camera* pc,
                                            int32_t W, int32_t H, const double* dC, const mcpt_aov_buffers* g,
                                            const mcpt_aov_buffers* pg, const double* dpC, const double* dpM, const double* dpF,
                                            double* dOut, double* dOutM, double* dOutF, double* dOutV, double* dOutS,
                                            double* seconds) {
    const ClampArgs ca{clamp, dpF, dOutF, dOutS};
    return accumulate_device(o, pc, W, H, dC, g, pg, dpC, dpM, dOut, dOutM, dOutV, seconds, &ca);
}

int mcpt_temporal_accumulate_clamped(const mcpt_temporal_opts* o, const mcpt_temporal_clamp_opts* clamp, const mcpt_camera* pc,
                                     int32_t W, int32_t H, const double* color, const mcpt_aov_buffers* g,
                                     const mcpt_aov_buffers* pg, const double* pcol, const double* pmom, const double* pfast,
                                     double* out, double* outm, double* outf, double* outv, double* outs, double* seconds) {
    const ClampArgs ca{clamp, pfast, outf, outs};
    return accumulate_host(o, pc, W, H, color, g, pg, pcol, pmom, out, outm, outv, seconds, &ca);
}

// the motion call: clamp == NULL is the plain rule, whose fast-history and shift arguments must then be NULL
static int motion_clamp_args(const mcpt_temporal_clamp_opts* clamp, const double* pfast, double* outf, double* outs) {
    if (!clamp && (pfast || outf || outs)) {
        set_error("%s is given without clamp: prev_fast, out_fast and out_shift belong to the clamped rule (pass clamp, or "
                  "leave them NULL)", pfast ? "prev_fast" : outf ? "out_fast" : "out_shift");
        return MCPT_E_INVALID;
    }
    return MCPT_OK;
}

int mcpt_temporal_accumulate_motion_device(const mcpt_temporal_opts* o, const mcpt_temporal_clamp_opts* clamp, const mcpt_camera* pc,
                                           int32_t W, int32_t H, const double* dC, const mcpt_aov_buffers* g,
                                           const mcpt_motion_buffers* mo, const mcpt_aov_buffers* pg, const double* dpC,
                                           const double* dpM, const double* dpF, double* dOut, double* dOutM, double* dOutF,
                                           double* dOutS, double* dOutV, double* seconds) {
    int rc;
    if ((rc = motion_clamp_args(clamp, dpF, dOutF, dOutS))) return rc;
    const ClampArgs ca{clamp, dpF, dOutF, dOutS};
    return accumulate_device(o, pc, W, H, dC, g, pg, dpC, dpM, dOut, dOutM, dOutV, seconds, clamp ? &ca : nullptr, true, mo);
}

int mcpt_temporal_accumulate_motion(const mcpt_temporal_opts* o, const mcpt_temporal_clamp_opts* clamp, const mcpt_camera* pc,
                                    int32_t W, int32_t H, const double* color, const mcpt_aov_buffers* g,
                                    const mcpt_motion_buffers* mo, const mcpt_aov_buffers* pg, const double* pcol,
                                    const double* pmom, const double* pfast, double* out, double* outm, double* outf,
                                    double* outs, double* outv, double* seconds) {
    int rc;
    if ((rc = motion_clamp_args(clamp, pfast, outf, outs))) return rc;
    const ClampArgs ca{clamp, pfast, outf, outs};
    return accumulate_host(o, pc, W, H, color, g, pg, pcol, pmom, out, outm, outv, seconds, clamp ? &ca : nullptr, true, mo);
}

// the anti-lag call: the motion call's arguments (motion may be NULL) and the Lambda map
int mcpt_temporal_accumulate_antilag_device(const mcpt_temporal_opts* o, const mcpt_temporal_clamp_opts* clamp, const mcpt_camera* pc,
                                            int32_t W, int32_t H, const double* dC, const mcpt_aov_buffers* g,
                                            const mcpt_motion_buffers* mo, const mcpt_aov_buffers* pg, const double* dpC,
                                            const double* dpM, const double* dpF, double* dOut, double* dOutM, double* dOutF,
                                            double* dOutS, double* dOutV, double* seconds, const mcpt_gradient_opts* gradient,
                                            const double* dLambda) {
    int rc;
    if ((rc = motion_clamp_args(clamp, dpF, dOutF, dOutS))) return rc;
    const ClampArgs ca{clamp, dpF, dOutF, dOutS};
    const AntilagArgs al{gradient, dLambda};
    return accumulate_device(o, pc, W, H, dC, g, pg, dpC, dpM, dOut, dOutM, dOutV, seconds, clamp ? &ca : nullptr, mo != nullptr, mo,
                             &al);
}

int mcpt_temporal_accumulate_antilag(const mcpt_temporal_opts* o, const mcpt_temporal_clamp_opts* clamp, const mcpt_camera* pc,
                                     int32_t W, int32_t H, const double* color, const mcpt_aov_buffers* g,
                                     const mcpt_motion_buffers* mo, const mcpt_aov_buffers* pg, const double* pcol,
                                     const double* pmom, const double* pfast, double* out, double* outm, double* outf,
                                     double* outs, double* outv, double* seconds, const mcpt_gradient_opts* gradient,
                                     const double* lambda) {
    int rc;
    if ((rc = motion_clamp_args(clamp, pfast, outf, outs))) return rc;
    const ClampArgs ca{clamp, pfast, outf, outs};
    const AntilagArgs al{gradient, lambda};
    return accumulate_host(o, pc, W, H, color, g, pg, pcol, pmom, out, outm, outv, seconds, clamp ? &ca : nullptr, mo != nullptr, mo,
                           &al);
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
