// The temporal gradient of the anti-lag for gfx950 (mcpt_gradient_opts, mcpt_gradient_phase, mcpt_temporal_gradient and
// its _device form; include/mcpt.h states the rule in full) and the reduction a frame sequence prints about it.  No
// counterpart in the reference.
//
//   k_temporal_gradient  lane per stratum : num and den of the up to (2 r + 1)^2 neighbouring strata's sample pixels
//                                           (6 doubles each), summed rows top to bottom and columns left to right,
//                                           then Lambda
//   k_lambda_stats       block per chunk  : the sum and the maximum of Lambda, per-block partials
//   k_lambda_final       one lane         : adds the partials in index order
//
// Everything is fp64 with -ffp-contract=off, so a numpy restatement of the rule reproduces the output to rounding
// (tests/test_antilag_cpu.py).  A block is 64 x 4 strata as in temporal.hip: a wave takes 64 consecutive strata of a
// row, whose sample pixels lie s pixels apart (3 s doubles), so at s = 3 a wave's loads of one tap touch 72-byte
// strides -- every second 64-byte line; the window's other taps reuse the neighbours' lines from cache.  Plain loads
// and stores only: no atomics, no LDS (the window is at most 49 taps of a map 1 / s^2 the frame's size: at 800 x 600
// and s = 3 the kernel is 53 k lanes).  The reduction is sequence.hip's k_frame_stats in shape: thread t of a block
// takes the chunk's values t, t + 256, ... in order, the wave adds its lanes by a shuffle tree (a fixed order), lane 0
// of wave 0 adds the four waves in wave order through LDS.  The maximum does not depend on the order; the sum's order is
// fixed.
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

struct GrParams {
    int W, H, ws, hs, s, a, b, r;
    double scale;
    const double *prev, *regrad;
    double* lam;
};

__global__ __launch_bounds__(kBx* kBy) void k_temporal_gradient(GrParams P) {
    const int J = blockIdx.x * kBx + threadIdx.x, I = blockIdx.y * kBy + threadIdx.y;
    if (J >= P.ws || I >= P.hs) return;
    double Num = 0.0, Den = 0.0;
    for (int di = -P.r; di <= P.r; di++) {
        const int II = I + di;
        if (II < 0 || II >= P.hs) continue;
        const int qi = P.s * II + P.a;
        if (qi >= P.H) continue;  // the sample pixel lies below the frame: num = den = 0
        for (int dj = -P.r; dj <= P.r; dj++) {
            const int JJ = J + dj;
            if (JJ < 0 || JJ >= P.ws) continue;
            const int qj = P.s * JJ + P.b;
            if (qj >= P.W) continue;
            const size_t q = 3 * ((size_t)qi * P.W + qj);
            const double g0 = P.regrad[q], g1 = P.regrad[q + 1], g2 = P.regrad[q + 2];
            const double p0 = P.prev[q], p1 = P.prev[q + 1], p2 = P.prev[q + 2];
            const double num = fabs(g0 - p0) + fabs(g1 - p1) + fabs(g2 - p2);
            const double den = fmax(g0, p0) + fmax(g1, p1) + fmax(g2, p2);
            Num += num;
            Den += den;
        }
    }
    double L = 0.0;
    if (Den > 0) {
        const double x = P.scale * Num / Den;
        L = x < 1 ? x : 1.0;
    }
    P.lam[(size_t)I * P.ws + J] = L;
}

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_lambda_stats(const double* __restrict__ lam, size_t n, size_t chunk,
                                                         double* __restrict__ psum, double* __restrict__ pmax) {
    __shared__ double ssum[kBlock / 64], smax[kBlock / 64];
    const size_t p0 = (size_t)blockIdx.x * chunk, p1 = p0 + chunk < n ? p0 + chunk : n;
    double sum = 0.0, mx = 0.0;  // Lambda >= 0
    for (size_t p = p0 + threadIdx.x; p < p1; p += kBlock) {
        const double v = lam[p];
        sum += v;
        mx = fmax(mx, v);
    }
    for (int off = 32; off >= 1; off >>= 1) {  // lane l takes lane l + off: the same tree every run
        sum += __shfl_down(sum, off, 64);
        mx = fmax(mx, __shfl_down(mx, off, 64));
    }
    const int wave = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) ssum[wave] = sum, smax[wave] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; w++) sum += ssum[w], mx = fmax(mx, smax[w]);
        psum[blockIdx.x] = sum, pmax[blockIdx.x] = mx;
    }
}

__global__ __launch_bounds__(64) void k_lambda_final(const double* __restrict__ psum, const double* __restrict__ pmax, int nb,
                                                     double n, double* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double sum = 0.0, mx = 0.0;
    for (int b = 0; b < nb; b++) sum += psum[b], mx = fmax(mx, pmax[b]);
    out[0] = sum / n, out[1] = mx;
}

// the reduction's shape, as sequence.hip's: at most kMaxPartials blocks, each over a chunk that is a multiple of the block
constexpr size_t kMaxPartials = 1024, kMinChunk = 4 * kBlock;
struct StatsShape {
    size_t chunk;
    int nb;
};
StatsShape stats_shape(size_t n) {
    size_t chunk = (n + kMaxPartials - 1) / kMaxPartials;
    chunk = (chunk + kBlock - 1) / kBlock * kBlock;
    if (chunk < kMinChunk) chunk = kMinChunk;
    return StatsShape{chunk, (int)((n + chunk - 1) / chunk)};
}

struct Range {
    const char* name;
    const double* p;
    size_t n;
};
bool overlap(const Range& a, const Range& b) {
    return (uintptr_t)a.p < (uintptr_t)(b.p + b.n) && (uintptr_t)b.p < (uintptr_t)(a.p + a.n);
}

// every check of mcpt_temporal_gradient[_device] that needs no device
int check_call(const mcpt_gradient_opts* o, int W, int H, int a, int b, const double* prev, const double* regrad, const double* lam) {
    int rc;
    if ((rc = mcpt::gradient_check_opts(o))) return rc;
    if (a < 0 || a >= o->stratum || b < 0 || b >= o->stratum) {
        set_error("mcpt_temporal_gradient: invalid phase (%d, %d): both must lie in [0, stratum = %d)", a, b, o->stratum);
        return MCPT_E_INVALID;
    }
    if (W < 1 || H < 1 || (long long)W * H > (1ll << 28)) {
        set_error("mcpt_temporal_gradient: invalid frame size: width %d, height %d", W, H);
        return MCPT_E_INVALID;
    }
    if (!prev || !regrad || !lam) {
        set_error("mcpt_temporal_gradient: null argument: %s", !prev ? "prev_raw" : !regrad ? "regrad" : "out_lambda");
        return MCPT_E_INVALID;
    }
    const size_t npx = (size_t)W * H, s = o->stratum;
    const Range out{"out_lambda", lam, ((H + s - 1) / s) * ((W + s - 1) / s)}, ins[] = {{"prev_raw", prev, 3 * npx}, {"regrad", regrad, 3 * npx}};
    for (const auto& r : ins)
        if (overlap(out, r)) {
            set_error("mcpt_temporal_gradient: out_lambda is aliasing %s", r.name);
            return MCPT_E_INVALID;
        }
    return MCPT_OK;
}

int enqueue_gradient(const mcpt_gradient_opts* o, int W, int H, int a, int b, const double* dPrev, const double* dRegrad, double* dLam) {
    GrParams P{};
    P.W = W, P.H = H, P.s = o->stratum, P.a = a, P.b = b, P.r = o->radius;
    P.ws = (W + P.s - 1) / P.s, P.hs = (H + P.s - 1) / P.s;
    P.scale = o->scale;
    P.prev = dPrev, P.regrad = dRegrad, P.lam = dLam;
    const dim3 grid((P.ws + kBx - 1) / kBx, (P.hs + kBy - 1) / kBy), block(kBx, kBy);
    hipLaunchKernelGGL(k_temporal_gradient, grid, block, 0, nullptr, P);
    DN_HIP_OK(hipGetLastError());
    return MCPT_OK;
}

// the kernel, timed with two events and waited for
int run_gradient(const mcpt_gradient_opts* o, int W, int H, int a, int b, const double* dPrev, const double* dRegrad, double* dLam,
                 Scratch& S, double* seconds) {
    int rc;
    DN_HIP_OK(hipEventCreate(&S.e0));
    DN_HIP_OK(hipEventCreate(&S.e1));
    DN_HIP_OK(hipEventRecord(S.e0, nullptr));
    if ((rc = enqueue_gradient(o, W, H, a, b, dPrev, dRegrad, dLam))) return rc;
    DN_HIP_OK(hipEventRecord(S.e1, nullptr));
    DN_HIP_OK(hipEventSynchronize(S.e1));
    float ms = 0;
    DN_HIP_OK(hipEventElapsedTime(&ms, S.e0, S.e1));
    if (seconds) *seconds = ms * 1e-3;
    return MCPT_OK;
}

}  // namespace

namespace mcpt {

int gradient_check_opts(const mcpt_gradient_opts* o) {
    if (!o) {
        set_error("null mcpt_gradient_opts");
        return MCPT_E_INVALID;
    }
    if (o->struct_size != sizeof(mcpt_gradient_opts)) {
        set_error("mcpt_gradient_opts.struct_size is %u, this library expects %zu (use mcpt_gradient_opts_init / the "
                  "mcpt.h of MCPT_VERSION %d)", o->struct_size, sizeof(mcpt_gradient_opts), MCPT_VERSION);
        return MCPT_E_INVALID;
    }
    if (o->stratum < 1 || o->stratum > 8) {
        set_error("invalid gradient options: stratum %d is outside 1..8", o->stratum);
        return MCPT_E_INVALID;
    }
    if (o->radius < 0 || o->radius > 3) {
        set_error("invalid gradient options: radius %d is outside 0..3", o->radius);
        return MCPT_E_INVALID;
    }
    if (!std::isfinite(o->scale) || !(o->scale > 0)) {
        set_error("invalid gradient options: scale %g must be finite and > 0", o->scale);
        return MCPT_E_INVALID;
    }
    return MCPT_OK;
}

int temporal_gradient_enqueue(const mcpt_gradient_opts* o, int32_t W, int32_t H, int32_t a, int32_t b, const double* dPrev,
                              const double* dRegrad, double* dLambda) {
    int rc;
    if ((rc = check_call(o, W, H, a, b, dPrev, dRegrad, dLambda))) return rc;
    return enqueue_gradient(o, W, H, a, b, dPrev, dRegrad, dLambda);
}

// stats_shape(n).nb is not monotone in n (the chunk is rounded up to the block), so the scratch is sized by its bound
size_t lambda_stats_words() { return 2 + 2 * kMaxPartials; }

int lambda_stats_enqueue(const double* dLambda, size_t n, double* words) {
    const StatsShape sh = stats_shape(n);
    if (n < 1 || (size_t)sh.nb > kMaxPartials) {  // chunk >= n / kMaxPartials, so this cannot happen: the scratch's bound
        set_error("lambda statistics: %zu values give %d partials, the scratch holds %zu", n, sh.nb, kMaxPartials);
        return MCPT_E_INVALID;
    }
    double *psum = words + 2, *pmax = psum + sh.nb;
    hipLaunchKernelGGL(k_lambda_stats, dim3(sh.nb), dim3(kBlock), 0, nullptr, dLambda, n, sh.chunk, psum, pmax);
    DN_HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(k_lambda_final, dim3(1), dim3(64), 0, nullptr, psum, pmax, sh.nb, (double)n, words);
    DN_HIP_OK(hipGetLastError());
    return MCPT_OK;
}

}  // namespace mcpt

extern "C" {

void mcpt_gradient_opts_init(mcpt_gradient_opts* o) {
    if (!o) return;
    std::memset((void*)o, 0, sizeof *o);
    o->struct_size = sizeof *o;
    o->stratum = 3;
    o->radius = 1;
    o->device = -1;
    o->scale = 1.0;
}

int mcpt_gradient_phase(int32_t s, uint64_t frame_index, int32_t* a, int32_t* b) {
    if (!a || !b) {
        set_error("mcpt_gradient_phase: null argument: %s", !a ? "a" : "b");
        return MCPT_E_INVALID;
    }
    if (s < 1 || s > 8) {
        set_error("mcpt_gradient_phase: stratum %d is outside 1..8", s);
        return MCPT_E_INVALID;
    }
    const int k = (int)(frame_index % (uint64_t)(s * s));
    *a = k % s;
    *b = (*a + k / s) % s;
    return MCPT_OK;
}

int mcpt_temporal_gradient_device(const mcpt_gradient_opts* o, int32_t W, int32_t H, int32_t a, int32_t b, const double* dPrev,
                                  const double* dRegrad, double* dLambda, double* seconds) {
    int rc;
    if ((rc = check_call(o, W, H, a, b, dPrev, dRegrad, dLambda))) return rc;
    Scratch S;
    int device;
    if ((rc = select_device(o->device, S, &device))) return rc;
    if ((rc = check_device_array(dPrev, device, "dev_prev_raw")) || (rc = check_device_array(dRegrad, device, "dev_regrad")) ||
        (rc = check_device_array(dLambda, device, "dev_out_lambda")))
        return rc;
    // the caller's arrays may still be written by work on other streams (e.g. torch's)
    DN_HIP_OK(hipDeviceSynchronize());
    return run_gradient(o, W, H, a, b, dPrev, dRegrad, dLambda, S, seconds);
}

int mcpt_temporal_gradient(const mcpt_gradient_opts* o, int32_t W, int32_t H, int32_t a, int32_t b, const double* prev,
                           const double* regrad, double* lambda, double* seconds) {
    int rc;
    if ((rc = check_call(o, W, H, a, b, prev, regrad, lambda))) return rc;
    Scratch S;
    int device;
    if ((rc = select_device(o->device, S, &device))) return rc;
    const size_t npx = (size_t)W * H, s = o->stratum, nl = ((H + s - 1) / s) * ((W + s - 1) / s), B = sizeof(double);
    DN_HIP_OK(hipMalloc(&S.p, (6 * npx + nl) * B));
    double *dPrev = S.p, *dRegrad = dPrev + 3 * npx, *dLam = dRegrad + 3 * npx;
    DN_HIP_OK(hipMemcpy(dPrev, prev, 3 * npx * B, hipMemcpyHostToDevice));
    DN_HIP_OK(hipMemcpy(dRegrad, regrad, 3 * npx * B, hipMemcpyHostToDevice));
    if ((rc = run_gradient(o, W, H, a, b, dPrev, dRegrad, dLam, S, seconds))) return rc;
    DN_HIP_OK(hipMemcpy(lambda, dLam, nl * B, hipMemcpyDeviceToHost));
    return MCPT_OK;
}

}  // extern "C"
