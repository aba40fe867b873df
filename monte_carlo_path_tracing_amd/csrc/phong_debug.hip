// mcpt_debug_phong (include/mcpt_debug.h): the Phong functions of device_math.h on caller-chosen inputs, with the
// template arguments the render kernels instantiate them with -- variant 0 the MIS / shade() kernels' forms, variant 1
// the BRDF-only kernels'.  One thread per record; nothing but device_math.h's inline functions is called, and the file
// is built by the same rule as render.hip (-ffp-contract=off), so the arithmetic is the kernels'.  tests/test_phong.py.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_math.h"
#include "mcpt.h"
#include "mcpt_debug.h"
#include "mcpt_internal.h"

namespace mcpt {

namespace {

#define PHONG_HIP_OK(x)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            if (d_in) (void)hipFree(d_in);                                                     \
            if (d_out) (void)hipFree(d_out);                                                   \
            return MCPT_E_DEVICE;                                                              \
        }                                                                                      \
    } while (0)

constexpr int kPhongBlock = 256;
constexpr int kPhongIn = 19, kPhongOut = 8;

template <bool kBrdfOnly>
__global__ void __launch_bounds__(kPhongBlock) k_debug_phong(int32_t n, const double* __restrict__ in,
                                                             double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kPhongBlock + threadIdx.x;
    if (i >= n) return;
    const double* r = in + i * kPhongIn;
    const d3 N = mk3(r[0], r[1], r[2]), wi = mk3(r[3], r[4], r[5]), wr = mk3(r[6], r[7], r[8]);
    const d3 kd = mk3(r[9], r[10], r[11]), ks = mk3(r[12], r[13], r[14]);
    const double sh = r[15], u0 = r[16], k1 = r[17], k2 = r[18];
    const d3 b = kBrdfOnly ? brdf_phong<false, true>(N, wi, wr, kd, ks, sh) : brdf_phong<true, false>(N, wi, wr, kd, ks, sh);
    const double p = phong_pdf(N, wi, wr, kd, ks, sh);
    double sp = 0;
    const d3 dir = sample_phong<kBrdfOnly>(N, wr, kd, ks, sh, u0, k1, k2, &sp);
    double* o = out + i * kPhongOut;
    o[0] = b.x;
    o[1] = b.y;
    o[2] = b.z;
    o[3] = p;
    o[4] = dir.x;
    o[5] = dir.y;
    o[6] = dir.z;
    o[7] = sp;
}

}  // namespace

}  // namespace mcpt

extern "C" int mcpt_debug_phong(int32_t n, int32_t variant, const double* in19, double* out8) {
    using namespace mcpt;
    if (n < 0 || (variant != 0 && variant != 1) || !in19 || !out8) {
        set_error("mcpt_debug_phong: n >= 0, variant 0 or 1 and non-null arrays expected");
        return MCPT_E_INVALID;
    }
    if (n == 0) return MCPT_OK;
    double *d_in = nullptr, *d_out = nullptr;
    const size_t in_bytes = (size_t)n * kPhongIn * sizeof(double), out_bytes = (size_t)n * kPhongOut * sizeof(double);
    PHONG_HIP_OK(hipMalloc((void**)&d_in, in_bytes));
    PHONG_HIP_OK(hipMalloc((void**)&d_out, out_bytes));
    PHONG_HIP_OK(hipMemcpy(d_in, in19, in_bytes, hipMemcpyHostToDevice));
    const unsigned blocks = (unsigned)(((int64_t)n + kPhongBlock - 1) / kPhongBlock);
    if (variant == 0) k_debug_phong<false><<<blocks, kPhongBlock>>>(n, d_in, d_out);
    else k_debug_phong<true><<<blocks, kPhongBlock>>>(n, d_in, d_out);
    PHONG_HIP_OK(hipGetLastError());
    PHONG_HIP_OK(hipMemcpy(out8, d_out, out_bytes, hipMemcpyDeviceToHost));
    PHONG_HIP_OK(hipDeviceSynchronize());
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return MCPT_OK;
}
