// The device-resident frame sequence for gfx950 (mcpt_sequence, mcpt_tone_map_device, mcpt_frame_stats_device;
// include/mcpt.h states the contract).  No counterpart in the reference, whose main() renders one frame.
//
//   k_tone_map<4>   lane per four values : the tone map of image.cpp over device memory, one 32-bit store of four
//                                          levels per lane (the output is then 4-byte aligned); the tail of the
//                                          frame (3 W H mod 4 values) is written byte by byte
//   k_tone_map<1>   lane per value       : the same for an output that is not 4-byte aligned
//   k_frame_stats   block per chunk      : the history statistics of a frame, per-block partials
//   k_stats_final   one lane             : adds the partials in index order
//
// The handle composes the existing device forms: mcpt_render_device and mcpt_render_aovs_device as they are (they
// run on the scene's stream and wait for it), then temporal_enqueue, the statistics, denoise_enqueue
// (mcpt_internal.h) and the tone map on the null stream, separated by the handle's events, and one synchronisation.
// Everything a frame touches is allocated in mcpt_sequence_create: one device allocation, cut into the buffers
// below, and 40 pinned bytes for the statistics and the upsampling's fallback count.  A sequence created by
// mcpt_sequence_create_upsampled adds three stages between the filter and the tone map: the AOVs of the scaled camera
// (mcpt_render_aovs_device again, into the full-size guides), upsample_enqueue (mcpt_internal.h) and the tone map of the
// full-size frame; everything before them is the plain sequence's code on the plain sequence's buffers.  A sequence
// created by mcpt_sequence_create_temporal_upsampled has a frame function of its own (frame_temporal_upsampled): the
// phase rays (camera_phase_rays_enqueue), mcpt_render_rays_device into the low raw frame, the full-size AOVs,
// temporal_upsample_enqueue and from there the plain frame's stages on full-size buffers.
//
// With mcpt_sequence_set_motion a plain sequence's frame adds one stage after the AOVs: motion_aovs_enqueue
// (mcpt_internal.h: k_motion_aovs on the primary-hit tables the AOVs just built) into two maps allocated at the first
// set_motion(on), and temporal_enqueue takes them (mcpt_temporal_accumulate_motion's rule).
//
// With mcpt_sequence_set_antilag a plain sequence's frame adds the gradient pass BEFORE its render (so the frame's AOVs
// and motion AOVs still see the primary-hit tables of the frame's own camera): gradient_rays_enqueue of the previous
// camera, mcpt_render_rays_device with the previous seed, temporal_gradient_enqueue against the raw frame the previous
// frame kept and lambda_stats_enqueue (mcpt_internal.h); temporal_enqueue then takes Lambda
// (mcpt_temporal_accumulate_antilag's rule) and the frame ends by keeping its raw frame (a device-to-device copy).  The
// buffers are an allocation of their own, made at the first switch-on.
//
// The tone map's loads are plain: lane k reads values 4 k .. 4 k + 3 (32 consecutive bytes, a wave 2 KB), stores
// are one dword per lane.  pow is the device library's; -ffp-contract=off as everywhere.  The statistics read the
// moments' n (every fourth double) and the shift once: thread t of a block takes the chunk's pixels t, t + 256, ...
// in order, the wave adds its lanes by a shuffle tree (a fixed order), lane 0 of wave 0 adds the four waves in wave
// order through LDS.  Counts are integers, so only the sum of n depends on the order, and that order is fixed.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "denoise_common.h"
#include "mcpt.h"
#include "mcpt_internal.h"
#include "scene_state.h"  // DevBuf: the anti-lag allocation is counted by mcpt_debug_device_bytes_live

using mcpt::set_error;
using mcpt_dn::check_device_array;
using mcpt_dn::Scratch;
using mcpt_dn::select_device;

namespace {

constexpr int kBlock = 256;

__device__ inline uint32_t tone_level(double v, double A, double gamma) {
    const double r = A * pow(v, gamma);
    const double x = floor(r * 255 + 0.5);
    if (!(x >= -2147483648.0 && x < 2147483648.0)) return 0u;  // the reference's out-of-range conversion: INT_MIN, hence 0
    return (uint32_t)fmin(fmax(x, 0.0), 255.0);
}

template <int VPT>
__global__ __launch_bounds__(kBlock) void k_tone_map(const double* __restrict__ rgb, size_t n, double A, double gamma,
                                                     uint8_t* __restrict__ out) {
    const size_t base = ((size_t)blockIdx.x * kBlock + threadIdx.x) * VPT;
    if (base >= n) return;
    if (VPT == 4 && base + 4 <= n) {
        const uint32_t l0 = tone_level(rgb[base], A, gamma), l1 = tone_level(rgb[base + 1], A, gamma);
        const uint32_t l2 = tone_level(rgb[base + 2], A, gamma), l3 = tone_level(rgb[base + 3], A, gamma);
        *reinterpret_cast<uint32_t*>(out + base) = l0 | (l1 << 8) | (l2 << 16) | (l3 << 24);
        return;
    }
    for (size_t k = base; k < n && k < base + VPT; k++) out[k] = (uint8_t)tone_level(rgb[k], A, gamma);
}

struct StatsOut {  // 32 bytes: what a frame sends to the host
    unsigned long long kept, moved;
    double nsum;
    unsigned long long pad;
};

// partials: kept[nb], moved[nb] (counts), nsum[nb] (doubles), as three arrays of 8-byte words
__global__ __launch_bounds__(kBlock) void k_frame_stats(const double* __restrict__ moments, const double* __restrict__ shift,
                                                        size_t npx, size_t chunk, unsigned long long* __restrict__ pkept,
                                                        unsigned long long* __restrict__ pmoved, double* __restrict__ pnsum) {
    __shared__ unsigned long long skept[kBlock / 64], smoved[kBlock / 64];
    __shared__ double snsum[kBlock / 64];
    const size_t p0 = (size_t)blockIdx.x * chunk, p1 = p0 + chunk < npx ? p0 + chunk : npx;
    unsigned long long kept = 0, moved = 0;
    double nsum = 0.0;
    for (size_t p = p0 + threadIdx.x; p < p1; p += kBlock) {
        const double n = moments[4 * p + 2];
        kept += n > 1.5;
        if (n > 0) nsum += n;
        if (shift) moved += shift[p] != 0.0;
    }
    for (int off = 32; off >= 1; off >>= 1) {  // lane l takes lane l + off: the same tree every run
        kept += __shfl_down(kept, off, 64);
        moved += __shfl_down(moved, off, 64);
        nsum += __shfl_down(nsum, off, 64);
    }
    const int wave = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0) skept[wave] = kept, smoved[wave] = moved, snsum[wave] = nsum;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; w++) kept += skept[w], moved += smoved[w], nsum += snsum[w];
        pkept[blockIdx.x] = kept, pmoved[blockIdx.x] = moved, pnsum[blockIdx.x] = nsum;
    }
}

__global__ __launch_bounds__(64) void k_stats_final(const unsigned long long* __restrict__ pkept,
                                                    const unsigned long long* __restrict__ pmoved,
                                                    const double* __restrict__ pnsum, int nb, StatsOut* __restrict__ out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    StatsOut s{0, 0, 0.0, 0};
    for (int b = 0; b < nb; b++) s.kept += pkept[b], s.moved += pmoved[b], s.nsum += pnsum[b];
    *out = s;
}

// the reduction's shape for a frame of npx pixels: at most kMaxPartials blocks, each over a chunk that is a multiple
// of the block (so the final pass stays short and its rounding small: DESIGN.md 4.15)
constexpr size_t kMaxPartials = 1024, kMinChunk = 4 * kBlock;
struct StatsShape {
    size_t chunk;
    int nb;
};
StatsShape stats_shape(size_t npx) {
    size_t chunk = (npx + kMaxPartials - 1) / kMaxPartials;
    chunk = (chunk + kBlock - 1) / kBlock * kBlock;
    if (chunk < kMinChunk) chunk = kMinChunk;
    return StatsShape{chunk, (int)((npx + chunk - 1) / chunk)};
}
size_t stats_words(size_t npx) { return 3 * (size_t)stats_shape(npx).nb + sizeof(StatsOut) / 8; }  // partials + the result

// both kernels on the null stream; words: stats_words(npx) 8-byte words of device scratch, the result in its last four
int enqueue_stats(const double* dM, const double* dS, size_t npx, void* words, StatsOut** result) {
    const StatsShape sh = stats_shape(npx);
    unsigned long long* pkept = (unsigned long long*)words;
    unsigned long long* pmoved = pkept + sh.nb;
    double* pnsum = (double*)(pmoved + sh.nb);
    StatsOut* res = (StatsOut*)(pnsum + sh.nb);
    hipLaunchKernelGGL(k_frame_stats, dim3(sh.nb), dim3(kBlock), 0, nullptr, dM, dS, npx, sh.chunk, pkept, pmoved, pnsum);
    DN_HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(k_stats_final, dim3(1), dim3(64), 0, nullptr, pkept, pmoved, pnsum, sh.nb, res);
    DN_HIP_OK(hipGetLastError());
    *result = res;
    return MCPT_OK;
}

int check_tone(double maxr, double gamma, const char* maxname, const char* gname) {
    if (!std::isfinite(maxr) || !(maxr > 0)) {
        set_error("invalid tone map: %s %g must be finite and > 0", maxname, maxr);
        return MCPT_E_INVALID;
    }
    if (!std::isfinite(gamma) || !(gamma > 0)) {
        set_error("invalid tone map: %s %g must be finite and > 0", gname, gamma);
        return MCPT_E_INVALID;
    }
    return MCPT_OK;
}

int enqueue_tone_map(const double* dRgb, size_t n, double maxr, double gamma, uint8_t* dOut) {
    const double A = std::pow(maxr, -gamma);
    if (((uintptr_t)dOut & 3) == 0) {
        const size_t lanes = (n + 3) / 4;
        hipLaunchKernelGGL(k_tone_map<4>, dim3((unsigned)((lanes + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr, dRgb, n, A,
                           gamma, dOut);
    } else {
        hipLaunchKernelGGL(k_tone_map<1>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr, dRgb, n, A, gamma,
                           dOut);
    }
    DN_HIP_OK(hipGetLastError());
    return MCPT_OK;
}

bool frame_size_ok(long long W, long long H) { return W >= 1 && H >= 1 && W * H <= (1ll << 28); }

}  // namespace

struct mcpt_sequence {
    mcpt_scene* scene = nullptr;
    mcpt_render_opts base{};  // spp = the sequence's; the seed is set per frame
    mcpt_sequence_opts opts{};
    mcpt_temporal_opts tp{};
    mcpt_temporal_clamp_opts tc{};
    mcpt_denoise_opts dn{};
    mcpt_upsample_opts up{};
    int factor = 0;   // 0: no upsampling; else the shown frame is factor times the render's along each axis
    size_t NPX = 0;   // the shown frame's pixels (npx without upsampling)
    int device = -1;  // the ordinal, resolved in create
    size_t npx = 0;
    // one device allocation: raw, two sets, variance, shift, filtered, the filter's scratch, the statistics' words, rgb8
    double* mem = nullptr;
    double* raw = nullptr;
    struct Set {
        mcpt_aov_buffers g{};
        double *color = nullptr, *moments = nullptr, *fast = nullptr;
        mcpt_camera cam{};
    } set[2];
    double *variance = nullptr, *shift = nullptr, *filtered = nullptr, *tmp = nullptr;
    void* stats_words = nullptr;
    mcpt_aov_buffers full{};      // upsampling: the guides of the scaled camera
    double* upsampled = nullptr;  // and the shown full-size colour
    unsigned long long* fallbacks = nullptr;
    // temporal upsampling (mcpt_sequence_create_temporal_upsampled): raw is the low frame, the two sets, variance,
    // filtered, the scratch and the statistics are full size, `full` and `upsampled` are unused
    bool tu = false;
    double *ray_o = nullptr, *ray_d = nullptr;  // the phase rays, npx * 3 each
    unsigned long long* tu_counts = nullptr;    // filled, fallback
    int phase_a = 0, phase_b = 0;               // the last frame's (mcpt_sequence_temporal_upsample_info)
    double rays_seconds = 0, filled_share = 0;
    uint8_t* rgb8 = nullptr;
    StatsOut* host_stats = nullptr;  // pinned; one more word behind it: the fallback count (tu: two more, its filled and fallback)
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double guide_seconds = 0, upsample_seconds = 0, fallback_share = 0;  // the last frame's (mcpt_sequence_upsample_info)
    int cur = 0;            // the set the next frame writes
    bool has_prev = false;  // set[cur ^ 1] holds a history
    bool has_last = false;  // set[cur ^ 1] and the shared buffers hold the last frame
    uint64_t frame_index = 0;
    // object motion (mcpt_sequence_set_motion): the two motion AOVs, an allocation of their own made at the first
    // set_motion(on); motion: the next frame runs with it; last_motion: the last frame did
    bool motion = false, last_motion = false;
    double* motion_mem = nullptr;
    mcpt_motion_buffers mo{};
    hipEvent_t ev_motion = nullptr;  // between the AOVs and the motion AOVs
    double motion_seconds = 0;
    // anti-lag (mcpt_sequence_set_antilag): the gradient rays, the gradient raw frame, the kept raw frame, Lambda (sized
    // for stratum 1) and the reduction's words, an allocation of their own made at the first switch-on; antilag: the
    // next frame runs with it; last_antilag: the last frame did, last_ran: and its gradient pass ran
    bool antilag = false, last_antilag = false, last_ran = false;
    mcpt_gradient_opts go{}, last_go{};
    mcpt::DevBuf al_mem;
    double *al_ray_o = nullptr, *al_ray_d = nullptr, *al_raw = nullptr, *al_kept = nullptr, *al_lambda = nullptr, *al_words = nullptr;
    double* al_host = nullptr;  // pinned: Lambda's mean and maximum
    hipEvent_t ev_al[4] = {nullptr, nullptr, nullptr, nullptr};  // the ray kernel, then (after the trace) gradient + reduction
    bool kept_valid = false;  // al_kept holds the raw frame of set[cur ^ 1], rendered with kept_seed
    uint64_t kept_seed = 0;
    int al_a = 0, al_b = 0;
    double al_trace_seconds = 0, al_kernel_seconds = 0, al_mean = 0, al_max = 0;
};

namespace {

void release(mcpt_sequence* s) {
    if (!s) return;
    if (s->mem || s->host_stats || s->ev[0] || s->motion_mem || s->ev_motion || s->al_mem.p || s->al_host || s->ev_al[0]) {
        int cur = 0;
        const bool sw = hipGetDevice(&cur) == hipSuccess && cur != s->device && hipSetDevice(s->device) == hipSuccess;
        if (s->mem) (void)hipFree(s->mem);
        if (s->motion_mem) (void)hipFree(s->motion_mem);
        if (s->ev_motion) (void)hipEventDestroy(s->ev_motion);
        (void)s->al_mem.release();
        if (s->al_host) (void)hipHostFree(s->al_host);
        for (hipEvent_t e : s->ev_al)
            if (e) (void)hipEventDestroy(e);
        if (s->host_stats) (void)hipHostFree(s->host_stats);
        for (hipEvent_t e : s->ev)
            if (e) (void)hipEventDestroy(e);
        if (sw) (void)hipSetDevice(cur);
    }
    delete s;
}

// what `what` names in the last frame: *bytes its size; dev: the device pointer
int locate(mcpt_sequence* s, int32_t what, bool allow_rgb8, const void** dev, size_t* bytes) {
    if (!s) {
        set_error("null mcpt_sequence");
        return MCPT_E_INVALID;
    }
    const mcpt_sequence::Set& L = s->set[s->cur ^ 1];
    const size_t d = sizeof(double), n = s->tu ? s->NPX : s->npx;  // temporal upsampling: all but RAW are full size
    const void* p = nullptr;
    size_t b = 0;
    if (s->tu && (what == MCPT_SEQ_FAST || what == MCPT_SEQ_SHIFT || what == MCPT_SEQ_UPSAMPLED)) {
        set_error("%s: a temporally upsampled sequence has no such buffer (its full-size frame is MCPT_SEQ_ACCUMULATED or "
                  "MCPT_SEQ_FILTERED; the history clamp is not available)",
                  what == MCPT_SEQ_FAST ? "MCPT_SEQ_FAST" : what == MCPT_SEQ_SHIFT ? "MCPT_SEQ_SHIFT" : "MCPT_SEQ_UPSAMPLED");
        return MCPT_E_INVALID;
    }
    switch (what) {
        case MCPT_SEQ_RAW: p = s->raw, b = 3 * s->npx * d; break;
        case MCPT_SEQ_ACCUMULATED: p = L.color, b = 3 * n * d; break;
        case MCPT_SEQ_MOMENTS: p = L.moments, b = 4 * n * d; break;
        case MCPT_SEQ_VARIANCE: p = s->variance, b = n * d; break;
        case MCPT_SEQ_FILTERED:
            if (!s->opts.denoise) {
                set_error("MCPT_SEQ_FILTERED: the sequence was created without denoise");
                return MCPT_E_INVALID;
            }
            p = s->filtered, b = 3 * n * d;
            break;
        case MCPT_SEQ_FAST:
        case MCPT_SEQ_SHIFT:
            if (!s->opts.clamp) {
                set_error("%s: the sequence was created without clamp", what == MCPT_SEQ_FAST ? "MCPT_SEQ_FAST" : "MCPT_SEQ_SHIFT");
                return MCPT_E_INVALID;
            }
            if (what == MCPT_SEQ_FAST) p = L.fast, b = 3 * n * d;
            else p = s->shift, b = n * d;
            break;
        case MCPT_SEQ_PREV_POSITION:
        case MCPT_SEQ_PREV_NORMAL:
            if (!s->motion || (s->has_last && !s->last_motion)) {
                set_error("%s: %s", what == MCPT_SEQ_PREV_POSITION ? "MCPT_SEQ_PREV_POSITION" : "MCPT_SEQ_PREV_NORMAL",
                          !s->motion ? "motion is off for this sequence (mcpt_sequence_set_motion)"
                                     : "the last frame ran before motion was switched on");
                return MCPT_E_INVALID;
            }
            p = what == MCPT_SEQ_PREV_POSITION ? s->mo.prev_position : s->mo.prev_normal, b = 3 * n * d;
            break;
        case MCPT_SEQ_GRADIENT_LAMBDA:
        case MCPT_SEQ_GRADIENT_RAW: {
            const char* name = what == MCPT_SEQ_GRADIENT_LAMBDA ? "MCPT_SEQ_GRADIENT_LAMBDA" : "MCPT_SEQ_GRADIENT_RAW";
            if (!s->antilag || (s->has_last && !s->last_antilag)) {
                set_error("%s: %s", name, !s->antilag ? "anti-lag is off for this sequence (mcpt_sequence_set_antilag)"
                                                      : "the last frame ran before anti-lag was switched on");
                return MCPT_E_INVALID;
            }
            if (what == MCPT_SEQ_GRADIENT_RAW && s->has_last && !s->last_ran) {
                set_error("%s: the last frame's gradient pass did not run (no history, or the previous frame kept no raw frame)", name);
                return MCPT_E_INVALID;
            }
            if (what == MCPT_SEQ_GRADIENT_RAW) p = s->al_raw, b = 3 * n * d;
            else {
                const size_t st = s->last_go.stratum > 0 ? s->last_go.stratum : 1;
                p = s->al_lambda, b = ((s->opts.height + st - 1) / st) * ((s->opts.width + st - 1) / st) * d;
            }
            break;
        }
        case MCPT_SEQ_RGB8:
            if (allow_rgb8) {
                p = s->rgb8, b = 3 * s->NPX;
                break;
            }
            [[fallthrough]];
        case MCPT_SEQ_UPSAMPLED:
            if (what == MCPT_SEQ_UPSAMPLED && s->factor) {
                p = s->upsampled, b = 3 * s->NPX * d;
                break;
            }
            [[fallthrough]];
        default:
            set_error("unknown buffer selector %d%s", what,
                      what == MCPT_SEQ_RGB8 ? " (MCPT_SEQ_RGB8 is not an array of doubles: use mcpt_sequence_device_buffer, or "
                                              "the frame's out_rgb8)"
                      : what == MCPT_SEQ_UPSAMPLED ? " for this sequence (MCPT_SEQ_UPSAMPLED: the sequence was created "
                                                     "without upsampling; use mcpt_sequence_create_upsampled)" : "");
            return MCPT_E_INVALID;
    }
    if (!s->has_last) {
        set_error("the sequence holds no frame (none since create, reset or a failed frame)");
        return MCPT_E_INVALID;
    }
    *dev = p, *bytes = b;
    return MCPT_OK;
}

}  // namespace

extern "C" {

int mcpt_tone_map_device(const double* dRgb, int32_t W, int32_t H, double maxr, double gamma, uint8_t* dOut, int32_t dev) {
    if (!dRgb || !dOut) {
        set_error("mcpt_tone_map_device: null argument: %s", !dRgb ? "dev_rgb" : "dev_rgb8");
        return MCPT_E_INVALID;
    }
    if (!frame_size_ok(W, H)) {
        set_error("mcpt_tone_map_device: invalid frame size: width %d, height %d", W, H);
        return MCPT_E_INVALID;
    }
    int rc;
    if ((rc = check_tone(maxr, gamma, "max_radiance", "gamma"))) return rc;
    Scratch S;
    int device;
    if ((rc = select_device(dev, S, &device))) return rc;
    if ((rc = check_device_array(dRgb, device, "dev_rgb")) || (rc = check_device_array(dOut, device, "dev_rgb8"))) return rc;
    // the caller's arrays may still be written by work on other streams (e.g. torch's)
    DN_HIP_OK(hipDeviceSynchronize());
    if ((rc = enqueue_tone_map(dRgb, 3 * (size_t)W * H, maxr, gamma, dOut))) return rc;
    DN_HIP_OK(hipStreamSynchronize(nullptr));
    return MCPT_OK;
}

int mcpt_frame_stats_device(const double* dM, const double* dS, int32_t W, int32_t H, int32_t dev, uint64_t* kept,
                            double* history_sum, uint64_t* moved) {
    if (!dM) {
        set_error("mcpt_frame_stats_device: null argument: dev_moments");
        return MCPT_E_INVALID;
    }
    if (!frame_size_ok(W, H)) {
        set_error("mcpt_frame_stats_device: invalid frame size: width %d, height %d", W, H);
        return MCPT_E_INVALID;
    }
    int rc;
    Scratch S;
    int device;
    if ((rc = select_device(dev, S, &device))) return rc;
    if ((rc = check_device_array(dM, device, "dev_moments")) || (dS && (rc = check_device_array(dS, device, "dev_shift")))) return rc;
    const size_t npx = (size_t)W * H;
    DN_HIP_OK(hipMalloc(&S.p, stats_words(npx) * 8));
    DN_HIP_OK(hipDeviceSynchronize());
    StatsOut* res = nullptr;
    if ((rc = enqueue_stats(dM, dS, npx, S.p, &res))) return rc;
    StatsOut h{};
    DN_HIP_OK(hipMemcpy(&h, res, sizeof h, hipMemcpyDeviceToHost));
    if (kept) *kept = h.kept;
    if (history_sum) *history_sum = h.nsum;
    if (moved) *moved = h.moved;
    return MCPT_OK;
}

void mcpt_sequence_opts_init(mcpt_sequence_opts* o) {
    if (!o) return;
    std::memset((void*)o, 0, sizeof *o);
    o->struct_size = sizeof *o;
    o->info_size = sizeof(mcpt_sequence_info);
    o->spp = 1;
    o->denoise = 1;
    o->tone_max = 380.0;  // main.cpp:583
    o->tone_gamma = 0.25;
}

// the three constructors; up == nullptr: mcpt_sequence_create; tu: mcpt_sequence_create_temporal_upsampled
static int sequence_create(mcpt_scene* scene, const mcpt_render_opts* base, const mcpt_sequence_opts* o,
                           const mcpt_temporal_opts* tp, const mcpt_temporal_clamp_opts* tc, const mcpt_denoise_opts* dn,
                           const mcpt_upsample_opts* up, mcpt_sequence** out, bool tu = false) {
    if (!scene || !base || !o || !out) {
        set_error("mcpt_sequence_create: null argument: %s", !scene ? "scene" : !base ? "base" : !o ? "opts" : "out");
        return MCPT_E_INVALID;
    }
    *out = nullptr;
    if (o->struct_size != sizeof(mcpt_sequence_opts)) {
        set_error("mcpt_sequence_opts.struct_size is %u, this library expects %zu (use mcpt_sequence_opts_init / the "
                  "mcpt.h of MCPT_VERSION %d)", o->struct_size, sizeof(mcpt_sequence_opts), MCPT_VERSION);
        return MCPT_E_INVALID;
    }
    if (base->struct_size != sizeof(mcpt_render_opts)) {
        set_error("mcpt_render_opts.struct_size is %u, this library expects %zu (use mcpt_render_opts_init / the "
                  "mcpt.h of MCPT_VERSION %d)", base->struct_size, sizeof(mcpt_render_opts), MCPT_VERSION);
        return MCPT_E_INVALID;
    }
    if (base->num_devices != 0 || base->devices || base->comm) {
        set_error("a frame sequence is single-device: a device list or a communicator is not supported");
        return MCPT_E_INVALID;
    }
    mcpt_render_opts def;
    mcpt_render_opts_init(&def);
    if (base->spp != def.spp || base->sample_begin != 0 || base->sample_end != 0) {
        set_error("frame sequence: spp, sample_begin and sample_end of the base options must be left at their defaults "
                  "(spp %d, range [%d,%d)); the samples of a frame come from mcpt_sequence_opts.spp", base->spp,
                  base->sample_begin, base->sample_end);
        return MCPT_E_INVALID;
    }
    if ((base->mode != MCPT_MODE_MIS && base->mode != MCPT_MODE_BRDF && base->mode != MCPT_MODE_SHADE &&
         base->mode != MCPT_MODE_SHADE_AREA) || (base->accel != MCPT_ACCEL_BVH && base->accel != MCPT_ACCEL_GRID)) {
        set_error("invalid render options (mode %d, accel %d)", base->mode, base->accel);
        return MCPT_E_INVALID;
    }
    if ((base->flags & MCPT_RENDER_PIXEL_JITTER) && base->accel == MCPT_ACCEL_GRID) {
        set_error("MCPT_RENDER_PIXEL_JITTER is not supported with MCPT_ACCEL_GRID (the jittered roots are traced over the BVH)");
        return MCPT_E_INVALID;
    }
    if (tu && base->accel == MCPT_ACCEL_GRID) {
        set_error("temporal upsampling: MCPT_ACCEL_GRID is not supported (the phase rays are traced by mcpt_render_rays, over the BVH)");
        return MCPT_E_INVALID;
    }
    if (tu && (base->flags & MCPT_RENDER_PIXEL_JITTER)) {
        set_error("temporal upsampling: MCPT_RENDER_PIXEL_JITTER is not supported (the phase rays go through the full-size "
                  "pixels' centres; mcpt_render_rays refuses the flag)");
        return MCPT_E_INVALID;
    }
    if (tu && o->clamp != 0) {
        set_error("temporal upsampling: mcpt_sequence_opts.clamp must be 0 (the history clamp is not defined for this rule)");
        return MCPT_E_INVALID;
    }
    if (o->spp < 1) {
        set_error("invalid sequence options: spp %d must be >= 1", o->spp);
        return MCPT_E_INVALID;
    }
    if (!frame_size_ok(o->width, o->height)) {
        set_error("invalid frame size: width %d, height %d", o->width, o->height);
        return MCPT_E_INVALID;
    }
    if ((o->denoise != 0 && o->denoise != 1) || (o->clamp != 0 && o->clamp != 1)) {
        set_error("invalid sequence options: denoise %d and clamp %d must be 0 or 1", o->denoise, o->clamp);
        return MCPT_E_INVALID;
    }
    int rc;
    if ((rc = check_tone(o->tone_max, o->tone_gamma, "tone_max", "tone_gamma"))) return rc;
    if ((rc = mcpt::temporal_check_opts(tp, tc, o->clamp != 0))) return rc;
    if (o->denoise && (rc = mcpt::denoise_check_opts(dn))) return rc;
    if (up) {
        if ((rc = mcpt::upsample_check_opts(up))) return rc;
        if (!frame_size_ok(o->width * (long long)up->factor, o->height * (long long)up->factor)) {
            set_error("invalid frame size: width %d, height %d at upsample factor %d (the full frame may hold 2^28 pixels)",
                      o->width, o->height, up->factor);
            return MCPT_E_INVALID;
        }
    }

    mcpt_sequence* s = new (std::nothrow) mcpt_sequence;
    if (!s) {
        set_error("out of host memory");
        return MCPT_E_DEVICE;
    }
    struct Guard {  // releases the half-built handle on every failing return
        mcpt_sequence* s;
        ~Guard() { release(s); }
    } guard{s};
    s->scene = scene;
    s->base = *base;
    s->base.spp = o->spp;
    s->opts = *o;
    s->tp = *tp;
    if (o->clamp) s->tc = *tc;
    if (o->denoise) s->dn = *dn;
    if (up) s->up = *up, s->factor = up->factor;
    const size_t npx = s->npx = (size_t)o->width * o->height;
    const size_t NPX = s->NPX = up ? npx * up->factor * up->factor : npx;
    Scratch S;  // restores the caller's device
    if ((rc = select_device(base->device, S, &s->device))) return rc;
    s->base.device = s->tp.device = s->dn.device = s->device;
    if (tu) {  // the low raw frame and its rays; everything else at the full size
        s->tu = true;
        const size_t words = 9 * npx + (2 * 17 + 1 + (o->denoise ? 3 + 8 : 0)) * NPX + stats_words(NPX) + 2;
        DN_HIP_OK(hipMalloc(&s->mem, words * 8 + 3 * NPX));
        double* q = s->mem;
        s->raw = q, s->ray_o = q + 3 * npx, s->ray_d = q + 6 * npx;
        q += 9 * npx;
        auto take = [&](size_t k) {
            double* r = q;
            q += k * NPX;
            return r;
        };
        for (auto& t : s->set) {
            t.g.albedo = take(3), t.g.normal = take(3), t.g.position = take(3), t.g.depth = take(1);
            t.color = take(3), t.moments = take(4);
        }
        s->variance = take(1);
        if (o->denoise) s->filtered = take(3), s->tmp = take(8);
        s->stats_words = q;
        q += stats_words(NPX);
        s->tu_counts = (unsigned long long*)q;
        s->rgb8 = (uint8_t*)(s->mem + words);  // after whole 8-byte words: 8-byte aligned
        DN_HIP_OK(hipHostMalloc((void**)&s->host_stats, sizeof(StatsOut) + 3 * sizeof(unsigned long long)));
        for (auto& e : s->ev) DN_HIP_OK(hipEventCreate(&e));
        guard.s = nullptr;
        *out = s;
        return MCPT_OK;
    }
    const size_t per_set = 10 + 3 + 4 + (o->clamp ? 3 : 0);
    const size_t doubles = 3 + 2 * per_set + 1 + (o->clamp ? 1 : 0) + (o->denoise ? 3 + 8 : 0);
    const size_t words = doubles * npx + stats_words(npx) + (up ? 13 * NPX + 1 : 0);
    DN_HIP_OK(hipMalloc(&s->mem, words * 8 + 3 * NPX));
    double* q = s->mem;
    auto take = [&](size_t k) {
        double* r = q;
        q += k * npx;
        return r;
    };
    s->raw = take(3);
    for (auto& t : s->set) {
        t.g.albedo = take(3), t.g.normal = take(3), t.g.position = take(3), t.g.depth = take(1);
        t.color = take(3), t.moments = take(4);
        if (o->clamp) t.fast = take(3);
    }
    s->variance = take(1);
    if (o->clamp) s->shift = take(1);
    if (o->denoise) s->filtered = take(3), s->tmp = take(8);
    s->stats_words = q;
    if (up) {
        q += stats_words(npx);
        s->fallbacks = (unsigned long long*)q++;
        s->full.albedo = q, s->full.normal = q + 3 * NPX, s->full.position = q + 6 * NPX, s->full.depth = q + 9 * NPX;
        s->upsampled = q + 10 * NPX;
    }
    s->rgb8 = (uint8_t*)(s->mem + words);  // after whole 8-byte words: 8-byte aligned
    DN_HIP_OK(hipHostMalloc((void**)&s->host_stats, sizeof(StatsOut) + sizeof(unsigned long long)));
    for (auto& e : s->ev) DN_HIP_OK(hipEventCreate(&e));
    guard.s = nullptr;
    *out = s;
    return MCPT_OK;
}

int mcpt_sequence_create(mcpt_scene* scene, const mcpt_render_opts* base, const mcpt_sequence_opts* o,
                         const mcpt_temporal_opts* tp, const mcpt_temporal_clamp_opts* tc, const mcpt_denoise_opts* dn,
                         mcpt_sequence** out) {
    return sequence_create(scene, base, o, tp, tc, dn, nullptr, out);
}

int mcpt_sequence_create_upsampled(mcpt_scene* scene, const mcpt_render_opts* base, const mcpt_sequence_opts* o,
                                   const mcpt_temporal_opts* tp, const mcpt_temporal_clamp_opts* tc,
                                   const mcpt_denoise_opts* dn, const mcpt_upsample_opts* up, mcpt_sequence** out) {
    if (!up) {
        if (out) *out = nullptr;
        set_error("mcpt_sequence_create_upsampled: null argument: upsample");
        return MCPT_E_INVALID;
    }
    return sequence_create(scene, base, o, tp, tc, dn, up, out);
}

int mcpt_sequence_upsample_info(mcpt_sequence* s, double* guide_seconds, double* upsample_seconds, double* fallback_share) {
    if (!s) {
        set_error("null mcpt_sequence");
        return MCPT_E_INVALID;
    }
    if (!s->factor || s->tu) {
        set_error("mcpt_sequence_upsample_info: the sequence %s", s->tu ? "upsamples temporally (use "
                  "mcpt_sequence_temporal_upsample_info)" : "was created without upsampling");
        return MCPT_E_INVALID;
    }
    if (!s->has_last) {
        set_error("the sequence holds no frame (none since create, reset or a failed frame)");
        return MCPT_E_INVALID;
    }
    if (guide_seconds) *guide_seconds = s->guide_seconds;
    if (upsample_seconds) *upsample_seconds = s->upsample_seconds;
    if (fallback_share) *fallback_share = s->fallback_share;
    return MCPT_OK;
}

int mcpt_sequence_create_temporal_upsampled(mcpt_scene* scene, const mcpt_render_opts* base, const mcpt_sequence_opts* o,
                                            const mcpt_temporal_opts* tp, const mcpt_denoise_opts* dn,
                                            const mcpt_upsample_opts* up, mcpt_sequence** out) {
    if (!up) {
        if (out) *out = nullptr;
        set_error("mcpt_sequence_create_temporal_upsampled: null argument: upsample");
        return MCPT_E_INVALID;
    }
    return sequence_create(scene, base, o, tp, nullptr, dn, up, out, true);
}

int mcpt_sequence_temporal_upsample_info(mcpt_sequence* s, int32_t* a, int32_t* b, double* rays_seconds, double* filled_share,
                                         double* fallback_share) {
    if (!s) {
        set_error("null mcpt_sequence");
        return MCPT_E_INVALID;
    }
    if (!s->tu) {
        set_error("mcpt_sequence_temporal_upsample_info: the sequence was created without temporal upsampling");
        return MCPT_E_INVALID;
    }
    if (!s->has_last) {
        set_error("the sequence holds no frame (none since create, reset or a failed frame)");
        return MCPT_E_INVALID;
    }
    if (a) *a = s->phase_a;
    if (b) *b = s->phase_b;
    if (rays_seconds) *rays_seconds = s->rays_seconds;
    if (filled_share) *filled_share = s->filled_share;
    if (fallback_share) *fallback_share = s->fallback_share;
    return MCPT_OK;
}

// a frame of a temporally upsampled sequence (the arguments are checked): ev[5] .. ev[6] the phase rays, then the traced
// rays, ev[0] .. ev[4] as in a plain frame with every stage at the full size
static int frame_temporal_upsampled(mcpt_sequence* s, const mcpt_camera* cam, uint64_t seed, uint8_t* out_rgb8,
                                    mcpt_sequence_info* info, mcpt_stats* stats) {
    const int w = s->opts.width, h = s->opts.height, f = s->factor, W = w * f, H = h * f;
    const size_t npx = s->npx, NPX = s->NPX;
    mcpt_sequence::Set &C = s->set[s->cur], &P = s->set[s->cur ^ 1];
    int rc, device;
    Scratch S;  // restores the caller's device
    if ((rc = select_device(s->device, S, &device))) return rc;
    int32_t pa = 0, pb = 0;
    mcpt_camera fullcam;
    if ((rc = mcpt_upsample_phase(f, s->frame_index, &pa, &pb)) || (rc = mcpt_camera_scaled(cam, f, &fullcam))) return rc;
    s->has_last = false;  // the shared buffers are about to be overwritten
    DN_HIP_OK(hipEventRecord(s->ev[5], nullptr));
    if ((rc = mcpt::camera_phase_rays_enqueue(&fullcam, f, pa, pb, s->ray_o, s->ray_d))) return rc;
    DN_HIP_OK(hipEventRecord(s->ev[6], nullptr));
    DN_HIP_OK(hipMemsetAsync(s->raw, 0, 3 * npx * sizeof(double), nullptr));
    mcpt_render_opts ro = s->base;
    ro.seed = seed;
    mcpt_stats st{};
    mcpt_render_opts rs = ro;  // the library's own stats struct, whatever the caller's size
    rs.stats_size = sizeof st;
    if ((rc = mcpt_render_rays_device(s->scene, &rs, (int32_t)npx, s->ray_o, s->ray_d, s->raw, &st))) return rc;
    DN_HIP_OK(hipSetDevice(device));
    DN_HIP_OK(hipEventRecord(s->ev[0], nullptr));
    if ((rc = mcpt_render_aovs_device(s->scene, &fullcam, &ro, &C.g))) return rc;
    DN_HIP_OK(hipSetDevice(device));
    DN_HIP_OK(hipEventRecord(s->ev[1], nullptr));
    const bool hp = s->has_prev;
    if ((rc = mcpt::temporal_upsample_enqueue(&s->tp, &s->up, pa, pb, hp ? &P.cam : nullptr, w, h, s->raw, &C.g, hp ? &P.g : nullptr,
                                              hp ? P.color : nullptr, hp ? P.moments : nullptr, C.color, C.moments, s->variance,
                                              s->tu_counts)))
        return rc;
    StatsOut* dres = nullptr;
    if ((rc = enqueue_stats(C.moments, nullptr, NPX, s->stats_words, &dres))) return rc;
    DN_HIP_OK(hipEventRecord(s->ev[2], nullptr));
    const double* shown = C.color;
    if (s->opts.denoise) {
        if ((rc = mcpt::denoise_enqueue(&s->dn, W, H, C.color, s->variance, &C.g, s->filtered, nullptr, s->tmp))) return rc;
        shown = s->filtered;
    }
    DN_HIP_OK(hipEventRecord(s->ev[3], nullptr));
    if ((rc = enqueue_tone_map(shown, 3 * NPX, s->opts.tone_max, s->opts.tone_gamma, s->rgb8))) return rc;
    DN_HIP_OK(hipEventRecord(s->ev[4], nullptr));
    unsigned long long* hcounts = (unsigned long long*)(s->host_stats + 1) + 1;
    DN_HIP_OK(hipMemcpyAsync(s->host_stats, dres, sizeof(StatsOut), hipMemcpyDeviceToHost, nullptr));
    DN_HIP_OK(hipMemcpyAsync(hcounts, s->tu_counts, 2 * sizeof *hcounts, hipMemcpyDeviceToHost, nullptr));
    if (out_rgb8) DN_HIP_OK(hipMemcpyAsync(out_rgb8, s->rgb8, 3 * NPX, hipMemcpyDeviceToHost, nullptr));
    DN_HIP_OK(hipStreamSynchronize(nullptr));
    float ms[5] = {0, 0, 0, 0, 0};
    for (int k = 0; k < 4; k++) DN_HIP_OK(hipEventElapsedTime(&ms[k], s->ev[k], s->ev[k + 1]));
    DN_HIP_OK(hipEventElapsedTime(&ms[4], s->ev[5], s->ev[6]));
    s->phase_a = pa, s->phase_b = pb;
    s->rays_seconds = ms[4] * 1e-3;
    s->filled_share = (double)hcounts[0] / (double)NPX;
    s->fallback_share = (double)hcounts[1] / (double)NPX;
    mcpt_sequence_info fi{};
    fi.render_seconds = st.seconds;
    fi.aov_seconds = ms[0] * 1e-3, fi.temporal_seconds = ms[1] * 1e-3;
    fi.denoise_seconds = s->opts.denoise ? ms[2] * 1e-3 : 0.0, fi.tonemap_seconds = ms[3] * 1e-3;
    fi.kept = (double)s->host_stats->kept / (double)NPX;
    fi.mean_history = s->host_stats->nsum / (double)NPX;
    fi.frame_index = s->frame_index;
    if (info) std::memcpy((void*)info, &fi, s->opts.info_size < sizeof fi ? s->opts.info_size : sizeof fi);
    if (stats) std::memcpy((void*)stats, &st, s->base.stats_size < sizeof st ? s->base.stats_size : sizeof st);
    C.cam = fullcam;
    s->cur ^= 1;
    s->has_prev = s->has_last = true;
    s->frame_index++;
    return MCPT_OK;
}

int mcpt_sequence_frame(mcpt_sequence* s, const mcpt_camera* cam, uint64_t seed, uint8_t* out_rgb8, mcpt_sequence_info* info,
                        mcpt_stats* stats) {
    if (!s || !cam) {
        set_error("mcpt_sequence_frame: null argument: %s", !s ? "seq" : "cam");
        return MCPT_E_INVALID;
    }
    if (cam->width != s->opts.width || cam->height != s->opts.height) {
        set_error("the camera is %d x %d, the sequence was created for width %d, height %d", cam->width, cam->height,
                  s->opts.width, s->opts.height);
        return MCPT_E_INVALID;
    }
    if (!(cam->dist_scale > 0)) {
        set_error("invalid camera");
        return MCPT_E_INVALID;
    }
    if (s->tu) return frame_temporal_upsampled(s, cam, seed, out_rgb8, info, stats);
    const int W = s->opts.width, H = s->opts.height;
    const size_t npx = s->npx;
    mcpt_sequence::Set &C = s->set[s->cur], &P = s->set[s->cur ^ 1];
    int rc, device;
    Scratch S;  // restores the caller's device
    if ((rc = select_device(s->device, S, &device))) return rc;
    s->has_last = false;  // the shared buffers are about to be overwritten
    const bool antilag = s->antilag;
    const mcpt_gradient_opts go = s->go;
    bool ran = false;
    int32_t pa = 0, pb = 0;
    mcpt_stats gst{};
    if (antilag) {
        const size_t gs = go.stratum, nlam = ((H + gs - 1) / gs) * ((W + gs - 1) / gs);
        if ((rc = mcpt_gradient_phase(go.stratum, s->frame_index, &pa, &pb))) return rc;
        if (s->has_prev && s->kept_valid) {  // the previous frame's samples again, in the scene as it is now
            DN_HIP_OK(hipEventRecord(s->ev_al[0], nullptr));
            if ((rc = mcpt::gradient_rays_enqueue(&P.cam, go.stratum, pa, pb, s->al_ray_o, s->al_ray_d))) return rc;
            DN_HIP_OK(hipEventRecord(s->ev_al[1], nullptr));
            DN_HIP_OK(hipMemsetAsync(s->al_raw, 0, 3 * npx * sizeof(double), nullptr));
            mcpt_render_opts gr = s->base;
            gr.seed = s->kept_seed;
            gr.stats_size = sizeof gst;
            if ((rc = mcpt_render_rays_device(s->scene, &gr, (int32_t)npx, s->al_ray_o, s->al_ray_d, s->al_raw, &gst))) return rc;
            DN_HIP_OK(hipSetDevice(device));
            DN_HIP_OK(hipEventRecord(s->ev_al[2], nullptr));
            if ((rc = mcpt::temporal_gradient_enqueue(&go, W, H, pa, pb, s->al_kept, s->al_raw, s->al_lambda))) return rc;
            ran = true;
        } else {
            DN_HIP_OK(hipMemsetAsync(s->al_lambda, 0, nlam * sizeof(double), nullptr));
            DN_HIP_OK(hipEventRecord(s->ev_al[2], nullptr));
        }
        if ((rc = mcpt::lambda_stats_enqueue(s->al_lambda, nlam, s->al_words))) return rc;
        DN_HIP_OK(hipEventRecord(s->ev_al[3], nullptr));
    }
    DN_HIP_OK(hipMemsetAsync(s->raw, 0, 3 * npx * sizeof(double), nullptr));
    mcpt_render_opts ro = s->base;
    ro.seed = seed;
    mcpt_stats st{};
    mcpt_render_opts rs = ro;  // the library's own stats struct, whatever the caller's size
    rs.stats_size = sizeof st;
    if ((rc = mcpt_render_device(s->scene, cam, &rs, s->raw, &st))) return rc;
    DN_HIP_OK(hipSetDevice(device));
    DN_HIP_OK(hipEventRecord(s->ev[0], nullptr));
    if ((rc = mcpt_render_aovs_device(s->scene, cam, &ro, &C.g))) return rc;
    DN_HIP_OK(hipSetDevice(device));
    const bool motion = s->motion;
    if (motion) {  // ev[0] .. ev_motion the AOVs, ev_motion .. ev[1] the motion AOVs, on the tables the AOVs just built
        DN_HIP_OK(hipEventRecord(s->ev_motion, nullptr));
        if ((rc = mcpt::motion_aovs_enqueue(s->scene, device, W, H, &s->mo))) return rc;
        DN_HIP_OK(hipSetDevice(device));
    }
    DN_HIP_OK(hipEventRecord(s->ev[1], nullptr));
    const mcpt::TemporalClampIo io{&s->tc, s->has_prev ? P.fast : nullptr, C.fast, s->shift};
    const bool hp = s->has_prev;
    const mcpt::TemporalAntilagIo al{&go, s->al_lambda};
    if ((rc = mcpt::temporal_enqueue(&s->tp, hp ? &P.cam : nullptr, W, H, s->raw, &C.g, hp ? &P.g : nullptr, hp ? P.color : nullptr,
                                     hp ? P.moments : nullptr, C.color, C.moments, s->variance, s->opts.clamp ? &io : nullptr,
                                     motion ? &s->mo : nullptr, antilag ? &al : nullptr)))
        return rc;
    StatsOut* dres = nullptr;
    if ((rc = enqueue_stats(C.moments, s->shift, npx, s->stats_words, &dres))) return rc;
    DN_HIP_OK(hipEventRecord(s->ev[2], nullptr));
    const double* shown = C.color;
    if (s->opts.denoise) {
        if ((rc = mcpt::denoise_enqueue(&s->dn, W, H, C.color, s->variance, &C.g, s->filtered, nullptr, s->tmp))) return rc;
        shown = s->filtered;
    }
    DN_HIP_OK(hipEventRecord(s->ev[3], nullptr));
    unsigned long long* hfall = (unsigned long long*)(s->host_stats + 1);
    if (s->factor) {  // the full-size guides, then the shown low frame onto them: ev[3] .. ev[5] .. ev[6], the tone map ends at ev[4]
        mcpt_camera fullcam;
        if ((rc = mcpt_camera_scaled(cam, s->factor, &fullcam))) return rc;
        if ((rc = mcpt_render_aovs_device(s->scene, &fullcam, &ro, &s->full))) return rc;
        DN_HIP_OK(hipSetDevice(device));
        DN_HIP_OK(hipEventRecord(s->ev[5], nullptr));
        if ((rc = mcpt::upsample_enqueue(&s->up, W, H, shown, &C.g, &s->full, s->upsampled, s->fallbacks))) return rc;
        shown = s->upsampled;
        DN_HIP_OK(hipEventRecord(s->ev[6], nullptr));
    }
    if ((rc = enqueue_tone_map(shown, 3 * s->NPX, s->opts.tone_max, s->opts.tone_gamma, s->rgb8))) return rc;
    DN_HIP_OK(hipEventRecord(s->ev[4], nullptr));
    DN_HIP_OK(hipMemcpyAsync(s->host_stats, dres, sizeof(StatsOut), hipMemcpyDeviceToHost, nullptr));
    if (s->factor) DN_HIP_OK(hipMemcpyAsync(hfall, s->fallbacks, sizeof *hfall, hipMemcpyDeviceToHost, nullptr));
    if (out_rgb8) DN_HIP_OK(hipMemcpyAsync(out_rgb8, s->rgb8, 3 * s->NPX, hipMemcpyDeviceToHost, nullptr));
    if (antilag) {  // the next frame's gradient pass compares against this frame's raw render
        s->kept_valid = false;
        DN_HIP_OK(hipMemcpyAsync(s->al_kept, s->raw, 3 * npx * sizeof(double), hipMemcpyDeviceToDevice, nullptr));
        DN_HIP_OK(hipMemcpyAsync(s->al_host, s->al_words, 2 * sizeof(double), hipMemcpyDeviceToHost, nullptr));
    }
    DN_HIP_OK(hipStreamSynchronize(nullptr));
    float ms[4] = {0, 0, 0, 0};
    for (int k = 0; k < 3; k++) DN_HIP_OK(hipEventElapsedTime(&ms[k], s->ev[k], s->ev[k + 1]));
    DN_HIP_OK(hipEventElapsedTime(&ms[3], s->ev[s->factor ? 6 : 3], s->ev[4]));
    if (motion) {
        float mm = 0;
        DN_HIP_OK(hipEventElapsedTime(&ms[0], s->ev[0], s->ev_motion));
        DN_HIP_OK(hipEventElapsedTime(&mm, s->ev_motion, s->ev[1]));
        s->motion_seconds = mm * 1e-3;
    }
    s->last_motion = motion;
    if (antilag) {
        float k0 = 0, k1 = 0;
        if (ran) DN_HIP_OK(hipEventElapsedTime(&k0, s->ev_al[0], s->ev_al[1]));
        DN_HIP_OK(hipEventElapsedTime(&k1, s->ev_al[2], s->ev_al[3]));
        s->al_a = pa, s->al_b = pb;
        s->al_trace_seconds = ran ? gst.seconds : 0.0;
        s->al_kernel_seconds = (k0 + k1) * 1e-3;  // without the pass: the reduction alone
        s->al_mean = s->al_host[0], s->al_max = s->al_host[1];
        s->kept_seed = seed;
        s->last_go = go;
    }
    s->kept_valid = antilag;
    s->last_antilag = antilag, s->last_ran = ran;
    if (s->factor) {
        float g = 0, u = 0;
        DN_HIP_OK(hipEventElapsedTime(&g, s->ev[3], s->ev[5]));
        DN_HIP_OK(hipEventElapsedTime(&u, s->ev[5], s->ev[6]));
        s->guide_seconds = g * 1e-3, s->upsample_seconds = u * 1e-3;
        s->fallback_share = (double)*hfall / (double)s->NPX;
    }
    mcpt_sequence_info fi{};
    fi.render_seconds = st.seconds;
    fi.aov_seconds = ms[0] * 1e-3, fi.temporal_seconds = ms[1] * 1e-3;
    fi.denoise_seconds = s->opts.denoise ? ms[2] * 1e-3 : 0.0, fi.tonemap_seconds = ms[3] * 1e-3;
    fi.kept = (double)s->host_stats->kept / (double)npx;
    fi.mean_history = s->host_stats->nsum / (double)npx;
    fi.clamped = (double)s->host_stats->moved / (double)npx;
    fi.frame_index = s->frame_index;
    if (info) std::memcpy((void*)info, &fi, s->opts.info_size < sizeof fi ? s->opts.info_size : sizeof fi);
    if (stats) std::memcpy((void*)stats, &st, s->base.stats_size < sizeof st ? s->base.stats_size : sizeof st);
    C.cam = *cam;
    s->cur ^= 1;
    s->has_prev = s->has_last = true;
    s->frame_index++;
    return MCPT_OK;
}

int mcpt_sequence_set_motion(mcpt_sequence* s, int32_t on) {
    if (!s) {
        set_error("null mcpt_sequence");
        return MCPT_E_INVALID;
    }
    if (s->factor || s->tu) {
        set_error("mcpt_sequence_set_motion: object motion is not supported in a sequence created by %s (use mcpt_sequence_create)",
                  s->tu ? "mcpt_sequence_create_temporal_upsampled" : "mcpt_sequence_create_upsampled");
        return MCPT_E_INVALID;
    }
    if (on && !s->motion_mem) {
        int device;
        Scratch S;  // restores the caller's device
        int rc;
        if ((rc = select_device(s->device, S, &device))) return rc;
        if (!s->ev_motion) DN_HIP_OK(hipEventCreate(&s->ev_motion));
        DN_HIP_OK(hipMalloc(&s->motion_mem, 6 * s->npx * sizeof(double)));
        s->mo.prev_position = s->motion_mem, s->mo.prev_normal = s->motion_mem + 3 * s->npx;
    }
    s->motion = on != 0;
    return MCPT_OK;
}

int mcpt_sequence_set_antilag(mcpt_sequence* s, const mcpt_gradient_opts* g) {
    if (!s) {
        set_error("null mcpt_sequence");
        return MCPT_E_INVALID;
    }
    if (s->factor || s->tu) {
        set_error("mcpt_sequence_set_antilag: anti-lag is not supported in a sequence created by %s (use mcpt_sequence_create)",
                  s->tu ? "mcpt_sequence_create_temporal_upsampled" : "mcpt_sequence_create_upsampled");
        return MCPT_E_INVALID;
    }
    if (!g) {
        s->antilag = false;
        return MCPT_OK;
    }
    if ((s->base.flags & MCPT_RENDER_PIXEL_JITTER) || s->base.accel == MCPT_ACCEL_GRID) {
        set_error("mcpt_sequence_set_antilag: %s is not supported (the gradient samples are traced by mcpt_render_rays, which "
                  "refuses it)", (s->base.flags & MCPT_RENDER_PIXEL_JITTER) ? "MCPT_RENDER_PIXEL_JITTER" : "MCPT_ACCEL_GRID");
        return MCPT_E_INVALID;
    }
    int rc;
    if ((rc = mcpt::gradient_check_opts(g))) return rc;
    if (!s->al_mem.p) {
        int device;
        Scratch S;  // restores the caller's device
        if ((rc = select_device(s->device, S, &device))) return rc;
        for (auto& e : s->ev_al)
            if (!e) DN_HIP_OK(hipEventCreate(&e));
        if (!s->al_host) DN_HIP_OK(hipHostMalloc((void**)&s->al_host, 2 * sizeof(double)));
        const size_t npx = s->npx;
        if ((rc = mcpt::ensure(s->al_mem, (13 * npx + mcpt::lambda_stats_words()) * sizeof(double)))) return rc;
        double* q = (double*)s->al_mem.p;
        s->al_ray_o = q, s->al_ray_d = q + 3 * npx, s->al_raw = q + 6 * npx, s->al_kept = q + 9 * npx, s->al_lambda = q + 12 * npx;
        s->al_words = q + 13 * npx;
    }
    if (!s->antilag) s->kept_valid = false;  // frames since the switch-off kept nothing
    s->go = *g;
    s->go.device = s->device;
    s->antilag = true;
    return MCPT_OK;
}

int mcpt_sequence_antilag_info(mcpt_sequence* s, int32_t* ran, int32_t* a, int32_t* b, double* trace_seconds, double* kernel_seconds,
                               double* lambda_mean, double* lambda_max) {
    if (!s) {
        set_error("null mcpt_sequence");
        return MCPT_E_INVALID;
    }
    if (!s->has_last) {
        set_error("the sequence holds no frame (none since create, reset or a failed frame)");
        return MCPT_E_INVALID;
    }
    if (!s->last_antilag) {
        set_error("mcpt_sequence_antilag_info: the last frame ran without anti-lag (mcpt_sequence_set_antilag)");
        return MCPT_E_INVALID;
    }
    if (ran) *ran = s->last_ran ? 1 : 0;
    if (a) *a = s->al_a;
    if (b) *b = s->al_b;
    if (trace_seconds) *trace_seconds = s->al_trace_seconds;
    if (kernel_seconds) *kernel_seconds = s->al_kernel_seconds;
    if (lambda_mean) *lambda_mean = s->al_mean;
    if (lambda_max) *lambda_max = s->al_max;
    return MCPT_OK;
}

int mcpt_sequence_motion_info(mcpt_sequence* s, double* motion_seconds) {
    if (!s) {
        set_error("null mcpt_sequence");
        return MCPT_E_INVALID;
    }
    if (!s->has_last) {
        set_error("the sequence holds no frame (none since create, reset or a failed frame)");
        return MCPT_E_INVALID;
    }
    if (!s->last_motion) {
        set_error("mcpt_sequence_motion_info: the last frame ran without motion (mcpt_sequence_set_motion)");
        return MCPT_E_INVALID;
    }
    if (motion_seconds) *motion_seconds = s->motion_seconds;
    return MCPT_OK;
}

int mcpt_sequence_read(mcpt_sequence* s, int32_t what, double* host_out) {
    const void* p = nullptr;
    size_t bytes = 0;
    int rc;
    if ((rc = locate(s, what, false, &p, &bytes))) return rc;
    if (!host_out) {
        set_error("mcpt_sequence_read: null argument: host_out");
        return MCPT_E_INVALID;
    }
    DN_HIP_OK(hipMemcpy(host_out, p, bytes, hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_sequence_device_buffer(mcpt_sequence* s, int32_t what, const void** dev_ptr) {
    const void* p = nullptr;
    size_t bytes = 0;
    int rc;
    if ((rc = locate(s, what, true, &p, &bytes))) return rc;
    if (!dev_ptr) {
        set_error("mcpt_sequence_device_buffer: null argument: dev_ptr");
        return MCPT_E_INVALID;
    }
    *dev_ptr = p;
    return MCPT_OK;
}

int mcpt_sequence_reset(mcpt_sequence* s) {
    if (!s) {
        set_error("null mcpt_sequence");
        return MCPT_E_INVALID;
    }
    s->has_prev = s->has_last = false;
    s->kept_valid = false;
    s->frame_index = 0;
    return MCPT_OK;
}

void mcpt_sequence_destroy(mcpt_sequence* s) { release(s); }

}  // extern "C"
