// The scene handle and its per-device state, shared by the translation units that work on them: render.hip (the
// renderer, which creates the states), scene_edit.hip (update, transform, pose / rest save, host sync, rebuild) and
// tree_debug.hip (the host-side tree checks).  Private to the library: the loaders' and kernels' interface is
// mcpt_internal.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "mcpt.h"
#include "mcpt_internal.h"

// two consecutive light triangles (2q, 2q+1) for the lane-per-node cull, every field as an (A, B)
// float pair so that one v_pk_fma_f32 with a scalar operand serves both lights: nl = unique normal,
// d = float(nl . p0 + 1e-8) (the threshold folded in), p[3k+i] = coordinate i of vertex k.  Padding
// lights (index >= N_L) have nl = 0, d = 1e30 (light-side culled).  128 B = two s_load_dwordx16.
struct LightPair {
    float2 nl[3];
    float2 d;      // nl . p0 + 1e-8 of both lights
    float2 p[9];
    float pad[6];
};

struct DScene {
    int F, NL;
    const float4* tri_v;      // F*3, original facet order
    const float* tri_n;       // F*9 vertex normals
    const int* tri_mat;       // F
    const int* tri_light;     // F -> light index or -1
    const float* mtl;         // M*7
    const double* light_rad;  // NL*3
    const double* light_sum;  // NL
    const int* light_facet;   // NL
    const float4* lt_v;       // NL*3 light vertices (reference order); .w = float(unique normal)
    float light_bound;        // max |coordinate| over light vertices
    const double4* lt_n;      // NL: unique normal xyz, w = RadianceRGB::sum()
    const float4* lt_pk;      // NL*3: (p0.x, p1.x, p2.x, nl.x), (.. .y), (.. .z) -- packed cheap stages
    const float* lt_d;        // NL: float(nl . p0)
    const double2* lt_w;      // NL*5: p0, p1, p2 (fp64), 2 RadianceRGB::sum()
    const float4* lt_f;       // NL*4: fp32 records of MCPT_RENDER_PRECISION_FP32 (LightF32: p0, p1, p2 with the
                              // area normal in .w, then 2 RadianceRGB::sum() as fp64 bits)
    const struct LightPair* lt_pair;  // 32*nchunks light pairs for k_prep_cull_lanes (scalar loads)
    // exact-pick band: per 64-light chunk a bounding sphere (centre, radius) of its
    // vertices and (max sum L, max sum L / shortest edge) of its lights; the same over the whole table
    const float4* chunk_sph;  // nchunks
    const float2* chunk_sk;   // nchunks
    double band_ctr[3], band_R, band_S, band_K;
    const float4* leaf_v;     // per leaf slot: 3 float4 (w of the first = facet id bits)
    const mcpt::BvhNode4* bvh4;     // 4-wide collapse of bvh (same leaves), breadth-first node order
    const mcpt::BvhNode4* lbvh4;
    const mcpt::BvhNode4Q* bvh4q;   // the same trees as 64-B compressed nodes (k_rays_persistent)
    const mcpt::BvhNode4Q* lbvh4q;
    int nbvh4, nlbvh4;        // node counts
    const float4* lleaf_v;
    // 8-wide compressed trees (BvhNode8Q, k_rays_cw8) and their triangle slots (3 float4 each, w of the
    // first = facet id bits; unused slots are never read); null when a tree does not fit the 24-bit base
    const mcpt::BvhNode8Q* bvh8;
    const mcpt::BvhNode8Q* lbvh8;
    const float4* tri8_v;
    const float4* ltri8_v;
    // select_a_point_from_lights (MCPT_MODE_SHADE_AREA): the lightsRadiance map in name order --
    // RadianceRGB::sum() per light and its running sum, the light-table run of its triangles -- and
    // the triangles' areas (Mylight.cpp:66-69) with their running sum within their light
    int ngroups;
    const double* grp_sum;
    const double* grp_cum;
    const int2* grp_range;    // (first light-table index, count)
    const double* l_area;
    const double* l_area_cum;
    // reference uniform grid (MCPT_ACCEL_GRID; null until mcpt_scene_meshing / a grid render)
    const int* g_start;       // CSR cell -> facets
    const int* g_tri;
    double g_mn[3], g_inv_d;
    int g_lim[3], g_gd[3];
};

constexpr int kStack = 48;
constexpr int kLeafBits = mcpt::kBvh4LeafBits;  // (5) leaf code ~((first slot << kLeafBits) | count)
// the sentinel records behind the padded light tables (lt_w and lt_f have nl_pad + kSentinelPad records)
constexpr int kSentinelPad = 64;

#define HIP_OK(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            set_error("%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MCPT_E_DEVICE;                                                              \
        }                                                                                      \
    } while (0)

namespace mcpt {

// bytes held by live DevBufs on all devices (mcpt_debug_device_bytes_live): adjusted by DevBuf's grow and release only
extern std::atomic<int64_t> g_device_bytes_live;

// a device allocation that frees itself: move-only (a move assignment hands the old allocation to the source, which
// frees it when it goes), grown by ensure() alone
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p), std::swap(bytes, o.bytes);
        return *this;
    }
    ~DevBuf() { (void)release(); }
    hipError_t release() {
        g_device_bytes_live -= (int64_t)bytes;
        void* q = std::exchange(p, nullptr);
        bytes = 0;
        return q ? hipFree(q) : hipSuccess;
    }
};

// one tree of a device state as refit.hip's kernels take it, with the first node of every level (DeviceState::refit)
struct TreeRefit {
    RefitDev dev{};
    std::vector<int32_t> level_first;
    bool ready = false;
};

struct DeviceState {
    int device = -1;
    DScene d{};
    std::vector<DevBuf> allocs;
    hipStream_t stream = nullptr;
    // reusable work buffers
    DevBuf hit_f, hit_tbg, root_pnw, root_kind, fb, rank_fb, stats, work, qa[14], qb[14], qs[14], aux[9], sl[13], cache_bt, cache_lst, cache_info, cache_w, masks;
    DevBuf cull_keys, cull_order, cull_count;  // the cull's node order (CullOrder)
    DevBuf exact, exact_scr, slack;  // exact pick: list, k_prep_exact's scratch, per-node slack
    DevBuf lit_slot, lit_pool;        // exact pick: roots' literal sums per pixel (RootLit)
    DevBuf sc_cum, sc_wsum, sc_last;  // small-table root-point cache (SmallCache)
    DevBuf pick_tab, pick_wsum;       // the root pick table of a run's window (PickTable)
    // adaptive sampling: half sums A / B, active lists and state bytes (ping-pong), per-block survivor counts
    // (+ the total), the library's own count / noise maps
    DevBuf ad_acc[2], ad_list[2], ad_state[2], ad_blk, ad_count, ad_noise;
    int ad_last_list = -1, ad_last_n = 0;  // the last active list built (mcpt_debug_adaptive_active)
    DevBuf aov;  // mcpt_render_aovs: the four maps of a host call (10 doubles per pixel)
    DevBuf ray_o, ray_d;  // mcpt_render_rays: a host call's origins and directions
    DevBuf ray_i;         // mcpt_render_rays_indexed: a host call's ids
    int spill_cap = 0;  // nodes the spill stack qs holds (grown on demand)
    bool bvh8_tried = false;  // ensure_bvh8 ran on this device
    DevBuf g_start, g_tri;  // the scene's uniform grid (MCPT_ACCEL_GRID), version grid_version
    int grid_version = 0;
    // mcpt_scene_update on this device: what refit.hip's kernels need beside the scene's own arrays (built at the
    // device state's first update: the facet -> leaf-slot map, the dirty bytes, the counters and the first node of
    // every level of the breadth-first 4-wide tree) and the staging copies of a host call's arrays
    TreeRefit refit;
    DevBuf up_pos, up_nrm;
    // mcpt_scene_set_visible: the state's copy of host.hidden (F bytes), allocated with the refit state
    // of a handle that has a mask or at the state's first visibility call; refit.dev.hidden points at it from then on
    DevBuf hidden;
    // a light move on this device, built at the state's first one: the light tables' pointers for
    // light_tables.hip, a second TreeRefit over the light-only tree (lbvh4, lbvh4q, lleaf_v; tri_v / tri_n shared with
    // `refit`) with its own slot map, dirty bytes, counters and levels, a pinned copy of the by-value constants and
    // the events around the light stage
    // A re-light needs the tables' half of that alone -- ltab with the chunk rows, the dirty bytes, the
    // constants' struct, the counters, the pinned copy and the events (ltab_ready) -- and never the light-only tree's;
    // up_rad stages a host call's radiances.
    LightTabDev ltab{};
    bool ltab_ready = false;
    DevBuf up_rad;
    TreeRefit lrefit;
    LightGlobals* pinned_globals = nullptr;
    hipEvent_t evl0 = nullptr, evl1 = nullptr;
    // mcpt_scene_rebuild on this device: the leaf slots of the main tree the state holds (the host
    // tree's until the first rebuild, F after it); the builder's scratch; two sets of tree arrays sized for F nodes and
    // F slots, built into in turn (the tree in use is never the one being written); the identity slot_start, the
    // counters and the cost reduction's words, shared by both sets.  All allocated at the first rebuild (the words at
    // the first mcpt_scene_tree_cost) and reused.
    size_t nslots = 0;
    RebuildWork* rb_work = nullptr;
    struct RebuildSet {
        DevBuf bvh4, bvh4q, leaf_v, slot_list, slot_dirty, node_dirty;
    } rb_set[2];
    DevBuf rb_slot_start, rb_counters, cost_words;
    int rb_next = 0;
    // mcpt_scene_pose_save: the previous pose's copies of d.tri_v / d.tri_n (null until the first save or, for a state
    // created after it, from the host copy: the previous pose is then the current one)
    DevBuf prev_v, prev_n;
    // mcpt_scene_rest_save: the rest pose's copies of d.tri_v / d.tri_n, the source of every mcpt_scene_transform
    DevBuf rest_v, rest_n;
    unsigned* pinned_count = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, evp0 = nullptr, evp1 = nullptr, evr0 = nullptr, evr1 = nullptr;

    // on its own device: the stream, the events, the pinned blocks and the rebuild's scratch; the buffers free themselves
    ~DeviceState() {
        if (device >= 0) (void)hipSetDevice(device);
        rebuild_work_destroy(rb_work);
        if (pinned_count) (void)hipHostFree(pinned_count);
        if (pinned_globals) (void)hipHostFree(pinned_globals);
        if (stream) (void)hipStreamDestroy(stream);
        for (hipEvent_t e : {ev0, ev1, evp0, evp1, evr0, evr1, evl0, evl1})
            if (e) (void)hipEventDestroy(e);
    }
};

// the facet -> leaf-slot map of a binary tree and its refit index, built at the tree's first update or transform
struct SlotMap {
    BvhRefitIndex ix;
    std::vector<int32_t> start, list;
};

}  // namespace mcpt

struct mcpt_scene {
    mcpt::HostScene host;
    mcpt::Bvh bvh, lbvh;
    mcpt::Bvh8 bvh8, lbvh8;  // 8-wide compressed trees of bvh / lbvh (k_rays_cw8), built on first use (ensure_bvh8)
    bool bvh8_built = false;
    std::mutex bvh8_mu;
    mcpt::Grid grid;       // Myobj::cal_scene_boundingbox(eye) + meshing(n0) (mcpt_scene_meshing)
    int grid_version = 0;  // bumped by every rebuild; devices re-upload on mismatch
    std::vector<std::unique_ptr<mcpt::DeviceState>> devs;
    std::mutex devs_mu;             // devs (render_multi creates device states on its worker threads)
    std::vector<int> comm_devices;  // distinct devices of the cached ncclCommInitAll communicators
    std::vector<void*> comms;
    std::mutex mu;
    // mcpt_scene_update: the build's bounding box, largest axis extent and box margin (box_margin of that box: it
    // covers every position of the arena) stay the scene's for good; `updated` once a call succeeded (the 8-wide trees are then stale and refused); the refit
    // index of `bvh` and the facet -> leaf-slot map, both built at the first update
    double build_lo[3] = {0, 0, 0}, build_hi[3] = {0, 0, 0}, build_ext = 0, margin = 0;
    bool updated = false;
    mcpt::SlotMap slots;
    // mcpt_scene_set_visible: how many bytes of host.hidden are set
    int32_t hidden_count = 0;
    // mcpt_scene_set_lights_movable: the switch, the numbers of the last successful update / transform
    // call, and the same index and slot map for `lbvh`, built at the first light move
    bool lights_movable = false;
    mcpt_light_update_stats light_stats{};
    mcpt::SlotMap lslots;
    // mcpt_scene_rebuild: nodes and leaf slots of the first rebuilt state's main tree (0: never rebuilt), for
    // mcpt_scene_accel_bytes
    uint64_t rebuilt_nodes = 0, rebuilt_slots = 0;
    // mcpt_scene_pose_save: host.pos / host.nrm as they were at the last save (empty until the first one)
    bool pose_saved = false;
    std::vector<float> prev_pos, prev_nrm;
    // mcpt_scene_rest_save / mcpt_scene_transform: the rest pose (host.pos / host.nrm at the save);
    // the facet ranges of host.pos / host.nrm / host.unique_n / bvh that are behind the devices, and whether prev_pos /
    // prev_nrm are (a pose_save while ranges were pending); host_sync brings all of it up to date from the first
    // device state.  host_mu guards pending and prev_stale and the sync itself: every read or write of the two takes it
    // (transform, pose_save, host_pending, host_sync), so render_multi's workers, which create device states and so
    // sync without holding `mu`, see a consistent list.  It does NOT order a render against a concurrent transform of
    // the same handle: as for an update, one render or update at a time per handle is the caller's rule (`mu`)
    bool rest_saved = false;
    std::vector<float> rest_pos, rest_nrm;
    mcpt::PendingRanges pending;
    bool prev_stale = false;
    std::mutex host_mu;
};

namespace mcpt {

// puts the thread back on the device it was on when a function that visits device states returns, on every path
struct DeviceRestore {
    int device = -1;
    ~DeviceRestore() {
        if (device >= 0) (void)hipSetDevice(device);
    }
};

// ---- render.hip ----
int ensure(DevBuf& b, size_t bytes);  // at least `bytes` (the contents are lost when it grows)
// the device's scene state, created on first use; makes `device` (< 0: the current one) current
int get_device_state(mcpt_scene* sc, int device, DeviceState** out);
int check_device_buffer(const void* p, int device, const char* name = "dev_out_rgb");
int prep_chunks(int NL);
void ensure_bvh8_host(mcpt_scene* sc);
int bvh8_refused(const mcpt_scene* sc);
int hidden_refused(const mcpt_scene* sc, const char* what);  // the grid modes while facets are hidden (§4.28)
extern std::atomic<int> g_rebuild_leaf_max;

// a host array as a buffer of its own that D owns, even if the copy fails
template <class T>
int upload(DeviceState& D, const std::vector<T>& v, const T** out) {
    DevBuf b;
    if (int rc = ensure(b, v.size() * sizeof(T))) return rc;
    void* p = b.p;
    D.allocs.push_back(std::move(b));
    if (!v.empty()) HIP_OK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = static_cast<const T*>(p);
    return MCPT_OK;
}
template <class T>
int upload(DeviceState& D, const std::vector<T>& v, T** out) {  // the same for an array the kernels write
    return upload(D, v, const_cast<const T**>(out));
}

// ---- scene_edit.hip ----
std::vector<DeviceState*> device_states(mcpt_scene* sc);
int host_sync(mcpt_scene* sc);
void ensure_slot_map(mcpt_scene* sc, bool light_tree);
int ensure_refit_state(mcpt_scene* sc, DeviceState& D);
int ensure_hidden_state(mcpt_scene* sc, DeviceState& D);
int ensure_light_tables(mcpt_scene* sc, DeviceState& D);
int ensure_light_state(mcpt_scene* sc, DeviceState& D);

}  // namespace mcpt
