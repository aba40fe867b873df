/* mcpt.h -- C ABI of libmcpt_hip.so, the MI355X (gfx950) path tracer.
 *
 * Drop-in boundary for the reference's per-pixel radiance loop (luotong96/Monte_Carlo_Path_Tracing).
 * The reference has no plugin/FFI seam: its loop is inlined in main() (main.cpp:547-588) and
 * calls `veach.closet_ray_intersect(eye, dir, triangle(-1,-1))` then
 * `shade_with_mis` / `shade_with_brdf` on the globals `Myobj veach` / `Mylight lights`
 * (main.cpp:23-24).  Each entry point below names the reference interface it replaces.
 *
 * Conventions: every function returns 0 (MCPT_OK) or a negative MCPT_E_* code; no exception
 * crosses the ABI (the reference instead exit(1)s on load errors, Myobj.cpp:15-20,
 * Mylight.cpp:16-20, and throws std::out_of_range on a bad material, main.cpp:425);
 * mcpt_last_error() returns a thread-local message.  Callers own host buffers; the library owns
 * device memory.  One render at a time per scene handle.  Results are deterministic for a fixed
 * (seed, spp, width, height) independent of how the sample range is split across calls / GPUs,
 * up to fp64 summation order.
 */
#ifndef MCPT_H
#define MCPT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCPT_VERSION 20300 /* 2.3.0: adaptive sampling (mcpt_adaptive_opts, mcpt_render_adaptive and its _device
                               * form); no existing struct changes; added since under the same number (additions
                               * only: bind them when present): primary-hit AOVs (mcpt_aov_buffers,
                               * mcpt_render_aovs and its _device form) and the variance-guided a-trous denoiser
                               * (mcpt_denoise_opts, mcpt_denoise and its _device form, mcpt_variance_from_noise);
                               * temporal accumulation (mcpt_temporal_opts, mcpt_temporal_accumulate and its
                               * _device form, mcpt_camera_orbit); its history clamping
                               * (mcpt_temporal_clamp_opts, mcpt_temporal_accumulate_clamped and its _device form);
                               * the device-resident frame sequence (mcpt_sequence, mcpt_sequence_opts,
                               * mcpt_sequence_info, the mcpt_sequence_* functions, mcpt_tone_map_device and
                               * mcpt_frame_stats_device); radiance along caller-supplied rays and pixel jitter
                               * (mcpt_render_rays and its _device form, mcpt_camera_rays, the flag
                               * MCPT_RENDER_PIXEL_JITTER); guided upsampling (mcpt_upsample_opts, mcpt_upsample and its
                               * _device form, mcpt_camera_scaled, mcpt_sequence_create_upsampled,
                               * mcpt_sequence_upsample_info, the selector MCPT_SEQ_UPSAMPLED); in-place geometry
                               * updates with a device-side BVH refit (mcpt_update_stats, mcpt_scene_update and its
                               * _device form); object motion for the temporal accumulation (mcpt_scene_pose_save,
                               * mcpt_motion_buffers, mcpt_render_motion_aovs and its _device form,
                               * mcpt_temporal_accumulate_motion and its _device form, mcpt_sequence_set_motion,
                               * mcpt_sequence_motion_info, the selectors MCPT_SEQ_PREV_POSITION and
                               * MCPT_SEQ_PREV_NORMAL); on-device transforms of facet ranges with a lazily synced
                               * host copy (mcpt_scene_rest_save, mcpt_scene_transform, mcpt_scene_host_pending,
                               * mcpt_scene_host_sync, mcpt_transform_rotation); an on-device rebuild of the main tree
                               * (mcpt_rebuild_stats, mcpt_scene_rebuild, mcpt_scene_tree_cost); movable light
                               * triangles (mcpt_scene_set_lights_movable, mcpt_scene_lights_movable,
                               * mcpt_light_update_stats, mcpt_scene_light_update_info); in-place re-lighting
                               * (mcpt_relight_stats, mcpt_scene_set_light_radiance and its _device form,
                               * mcpt_scene_set_materials, mcpt_scene_light_groups); anti-lag by temporal gradients
                               * (mcpt_gradient_opts, mcpt_gradient_phase, mcpt_gradient_rays and its _device form,
                               * mcpt_temporal_gradient and its _device form, mcpt_temporal_accumulate_antilag and its
                               * _device form, mcpt_sequence_set_antilag, mcpt_sequence_antilag_info, the selectors
                               * MCPT_SEQ_GRADIENT_LAMBDA and MCPT_SEQ_GRADIENT_RAW);
                               * mcpt_stats gains pick_table_roots (appended, guarded by stats_size: stats ABI 2.3);
                               * 2.2.0: mcpt_stats gains comm_init_seconds, device_setup_seconds and
                               * device_seconds[MCPT_STATS_MAX_DEVICES] (appended): where a multi-device call's
                               * time went; mcpt_render_opts gains stats_size (appended: a caller built against
                               * an older header is refused by struct_size instead of having its smaller
                               * mcpt_stats overrun);
                               * 2.1.0: mcpt_stats gains prep_exact_nodes, cache_build_seconds and prep_band_nodes
                               * (appended);
                               * 2.0.0: mcpt_render_opts carries struct_size (checked first), a device list
                               * and a multi-process communicator; debug entry points moved to mcpt_debug.h */

enum {
    MCPT_OK = 0,
    MCPT_E_INVALID = -1,  /* bad argument */
    MCPT_E_IO = -2,       /* file not found / parse error */
    MCPT_E_SCENE = -3,    /* scene violates the reference's assumptions (e.g. facet without material) */
    MCPT_E_DEVICE = -4,   /* HIP error */
    MCPT_E_OVERFLOW = -5, /* reserved (since 2.0 a generation larger than the queue is processed in slices) */
    MCPT_E_CANCELLED = -6, /* the progress callback asked to stop */
};

/* shade_with_mis main.cpp:402 / shade_with_brdf :348 / shade :269 (the one main() calls, :575) with
 * the spherical-triangle light sampler (main.cpp:297) / shade with the uniform-area light sampler
 * select_a_point_from_lights (Mylight.cpp:102-160, the alternative commented out at main.cpp:296:
 * a light by radiance, a triangle by area, a uniform point; no O(N_L) light prep) */
enum { MCPT_MODE_MIS = 0, MCPT_MODE_BRDF = 1, MCPT_MODE_SHADE = 2, MCPT_MODE_SHADE_AREA = 3 };

/* closest-hit acceleration: the BVH (default; the true closest hit) or the reference's own uniform
 * grid with its in-cell acceptance rule (Myobj.cpp:78-162, 334-622), crack included -- hit for hit
 * the reference's traversal, for parity studies (much slower). */
enum { MCPT_ACCEL_BVH = 0, MCPT_ACCEL_GRID = 1 };
/* mcpt_closest_hit flags */
enum { MCPT_HIT_LIGHT_ONLY = 1, MCPT_HIT_GRID = 2 };

typedef struct mcpt_scene mcpt_scene;

/* Flattened scene (host pointers, copied by mcpt_scene_create).  Facets in the reference's
 * (shape, face) order; light table in Mylight::lightsTriangles order (material name, then facet,
 * Mylight.cpp:88). */
typedef struct {
    int32_t nfacets, nmaterials, nlights;
    const float* positions;      /* nfacets*9: v0 v1 v2 (tinyobj real_t = float) */
    const float* normals;        /* nfacets*9: vertex normals */
    const int32_t* material_id;  /* nfacets */
    const float* materials;      /* nmaterials*7: Kd[3] Ks[3] Ns */
    const int32_t* light_facet;  /* nlights: facet of each light triangle */
    const double* light_radiance; /* nlights*3: radiance of its <light> material */
    const int32_t* light_group;  /* optional, nlights: index of its <light> (ascending; the lights of
                                  * select_a_point_from_lights, Mylight.cpp:102-160); NULL = each run of
                                  * equal radiance is one light */
} mcpt_scene_desc;

/* Camera of main.cpp:507-510,547-564 generalised to width x height:
 * pixellen = tan(fovy/360)*|w|/(height/2) (the reference's /360 quirk kept), eye pulled back by
 * dist_scale (2 in the reference). */
typedef struct {
    double eye[3], lookat[3], up[3];
    double fovy;
    double dist_scale;
    int32_t width, height;
} mcpt_camera;

/* progress callback (replaces the reference's per-row progress / EasyX display, main.cpp:539-592):
 * called on the rendering host thread after every wavefront generation with the camera samples
 * dispatched so far and the call's total; return nonzero to cancel the render (MCPT_E_CANCELLED,
 * the framebuffer then holds a partial sum). */
typedef int (*mcpt_progress_fn)(void* user, uint64_t samples_dispatched, uint64_t samples_total);

/* Multi-process communicator (one process per GPU, e.g. torchrun): rank 0 creates an id with
 * mcpt_comm_unique_id, the caller broadcasts its MCPT_COMM_ID_BYTES bytes (any channel), every rank
 * calls mcpt_comm_init_rank (RCCL ncclCommInitRank on `device`; collective over all ranks).  The
 * library owns the RCCL communicator. */
typedef struct mcpt_comm mcpt_comm;
#define MCPT_COMM_ID_BYTES 128

typedef struct {
    uint32_t struct_size;   /* sizeof(mcpt_render_opts) of the caller's header (mcpt_render_opts_init sets
                             * it); checked before any other field -- a mismatch is MCPT_E_INVALID */
    int32_t spp;            /* samples per pixel of the whole frame (the 1/spp weight) */
    int32_t sample_begin;   /* render global sample indices [sample_begin, sample_end) */
    int32_t sample_end;     /*   (0,0 = all); with devices / comm this is the JOB's range, split below */
    int32_t mode;           /* MCPT_MODE_MIS / MCPT_MODE_BRDF / MCPT_MODE_SHADE */
    uint64_t seed;          /* counter-RNG seed (reference default 20240430 in bench/tests) */
    int32_t samples_per_launch; /* wavefront working set: the node queue is refilled with camera samples
                                 * up to samples_per_launch x width x height nodes per generation
                                 * (0 = auto: 48 Mi nodes, at most the call's camera samples and at
                                 * most half the free HBM) */
    int32_t queue_factor;   /* wavefront queue capacity = factor * batch roots (0 = 2); a generation with
                             * more nodes than the children buffer can take is processed in slices, the
                             * rest parked on a spill stack in HBM (never an overflow error) */
    int32_t device;         /* HIP device ordinal (-1 = current); ignored when num_devices > 0 */
    int32_t accel;          /* MCPT_ACCEL_BVH / MCPT_ACCEL_GRID (grid over the scene and this camera's
                             * eye with n0 = 100000, main.cpp:501-504; rebuilt when the eye changes) */
    mcpt_progress_fn progress; /* optional (NULL = none); with several devices it is called from the
                                * devices' worker threads, serialised by the library */
    void* progress_user;
    int32_t flags;          /* MCPT_RENDER_* bits (0 = defaults) */
    /* One process, several GPUs: num_devices > 0 splits [sample_begin, sample_end)
     * into num_devices contiguous, balanced shards, shard k rendered on devices[k] (a device may be
     * listed more than once: its shards run one after another into that device's buffer), one host
     * thread and stream per distinct device, no exchange while rendering; then ONE RCCL
     * ncclReduce(sum) over the distinct devices (ncclCommInitAll, cached per scene handle) into the
     * root devices[0].  mcpt_render: the result lands in out_rgb; mcpt_render_device: dev_out_rgb
     * lives on devices[0].  The image equals the single-device render up to fp64 summation order. */
    int32_t num_devices;
    const int32_t* devices;
    /* One process per GPU: this process renders rank's share of [sample_begin, sample_end) on the
     * communicator's device and the call ends with ONE ncclReduce(sum, root rank 0): the whole job's
     * sum is ADDED to rank 0's buffer; other ranks' buffers are left unchanged (their shard goes
     * through a library buffer).  Every rank must make the same call.  Exclusive with devices.
     * Failures: a rank whose render fails (out of memory, its own cancel, ...) still joins the reduce with
     * a failure flag, so rank 0 returns MCPT_E_DEVICE "k of N ranks failed" and nobody blocks.  The one
     * exception is a rank that cannot take part in the reduce at all -- it cannot allocate its
     * (W*H*3 + 1)-double reduce buffer (done first, before any other allocation of the call, and kept
     * for later calls of the same frame size) or its device can no longer enqueue work: it aborts the
     * communicator and returns, and under RCCL its peers then block in ncclReduce (RCCL has no way to
     * release them from one rank).  Leave that buffer's room free on every device. */
    mcpt_comm* comm;
    uint32_t stats_size;    /* sizeof(mcpt_stats) of the caller's header (mcpt_render_opts_init sets it): the
                             * library writes at most this many bytes of the stats (0: none) */
} mcpt_render_opts;
/* mcpt_render_opts.flags: skip the light-side cull statistic in the hot loop of the split light cull;
 * mcpt_stats.light_evals_culled_backface then reads 0 and _culled_plane holds both cheap-stage culls
 * (every prep variant reports it that way).  Images and all other statistics are unchanged. */
enum { MCPT_RENDER_NO_BACKFACE_STATS = 1 };
/* mcpt_render_opts.flags: shade_with_mis evaluates the BRDF branch's light pdf with the node's OWN
 * light prep instead of the reference's stale sampler state (main.cpp:443 vs :487: the state the
 * last prep inside the light branch's recursion left, Mylight.cpp:484-493).  The default follows
 * the reference; this flag is the "fixed" estimator (4.6e-3 relative L2 from the reference's on the
 * Veach stand-in, profiles/stale_pdf_delta.json). */
enum { MCPT_RENDER_FRESH_PDF = 2 };
/* mcpt_render_opts.flags: precision of the light prep's full stage (SURVEY.md §8(b) FP32_STABLE,
 * opt-in).  Default (flag clear) = FP64_LIGHT: the reference's fp64, required for parity.  With the
 * flag, the spherical-triangle weights (Mylight.cpp:360-413) are evaluated two lights per lane in
 * packed fp32 by a cancellation-free Van Oosterom-Strackee form (p - x1 with x1 split hi + lo, the
 * triple product against a precomputed area normal) and summed in fp64: weights within ~1e-6 of the
 * fp64 ones, rendered frames within the 1e-3 relative L2 tolerance of the fp64 render; the edge-length
 * and vertex-angle culls below 1e-8 rad reduce to "sA > 0".  Applies to scenes with more than 64
 * light triangles (the split prep); cheap culls, pick, sampling, pdf and shading stay fp64. */
enum { MCPT_RENDER_PRECISION_FP32 = 4 };

/* mcpt_render_opts.flags: anti-aliasing (opt-in; no counterpart in the reference, whose samples all go through the
 * pixel's centre, main.cpp:563-564).  Sample k of pixel p = i * width + j shoots its camera ray through
 * (i + dy, j + dx) instead of (i, j): dy = u(key, 0) - 0.5 and dx = u(key, 1) - 0.5 with key the counter RNG's key of
 * (seed, pixel p, sample k, node 0) -- a stream no shading node uses (node ids start at 1) -- so every sample lies in
 * its pixel's square and the frame is the scene under a box pixel filter.  The direction is the camera's formula
 * (main.cpp:563-564) at the fractional coordinates; mcpt_camera_rays returns these rays.  Everything after the primary
 * hit is unchanged, a sample's ray depends on (seed, p, k) only, so sample ranges, device lists and communicators
 * split a jittered frame as they split a plain one.  The primary hit is traced per sample and no root shares a light
 * prep: mcpt_stats.prep_cached_nodes and prep_cache_points are 0 and the render is slower (README.md gives the
 * measured cost).  Accepted by mcpt_render, mcpt_render_device and (through base->flags) mcpt_sequence_create;
 * MCPT_E_INVALID before any device work together with MCPT_ACCEL_GRID and in mcpt_render_adaptive[_device] and
 * mcpt_render_rays[_device].  mcpt_render_aovs ignores it like every other flag: the AOVs stay at the pixel centres. */
enum { MCPT_RENDER_PIXEL_JITTER = 8 };

/* zero-fills *opts and sets struct_size, stats_size, device = -1, seed = 20240430, spp = 10 (main.cpp:567),
 * mode = MCPT_MODE_MIS */
void mcpt_render_opts_init(mcpt_render_opts* opts);

#define MCPT_STATS_MAX_DEVICES 16
typedef struct {
    double seconds;         /* device time of the render (HIP events) */
    uint64_t camera_samples;
    uint64_t shading_nodes; /* nodes that passed entry + RR (prep nodes in MIS) */
    uint64_t light_evals_survived; /* light triangles surviving the cull chain (MIS prep) */
    uint64_t rays;          /* extension rays traced */
    uint64_t light_rays;    /* light-only rays traced (MIS light pdf) */
    uint64_t generations;   /* wavefront generations launched */
    double prep_seconds;    /* device time inside the light-prep kernel (HIP events, its stream) */
    uint64_t prep_launches;
    uint64_t light_evals_total;           /* prep_full_nodes x light triangles (MIS, shade) */
    uint64_t light_evals_culled_backface; /* culled by the light-side test (Mylight.cpp:340-345) */
    uint64_t light_evals_culled_plane;    /* culled by the tangent-plane test (Mylight.cpp:347-357) */
    uint64_t light_evals_candidates;      /* passed both; evaluated in full (Mylight.cpp:360-413) */
    uint64_t prep_full_nodes;   /* prep nodes that ran the O(N_L) stages (incl. root-cache builds) */
    uint64_t prep_cached_nodes; /* root nodes served by the per-pixel root-point cache (pick only) */
    uint64_t prep_cache_points; /* root points whose prep built the cache (included in prep_full_nodes) */
    uint64_t spilled_nodes; /* nodes parked on the spill stack (generations larger than the queue) */
    double reduce_seconds;  /* the RCCL reduce of a multi-device / multi-rank call (0 otherwise) */
    int32_t devices_used;   /* distinct devices (or 1 per rank) that rendered */
    double trace_seconds;   /* device time in the traversal kernel (k_mis_rays; BRDF-only: k_extend_brdf) */
    uint64_t trace_launches;
    uint64_t node_visits;   /* BVH node visits and ray/triangle tests of that kernel -- counted only when */
    uint64_t tri_tests;     /* the render sets MCPT_DEBUG_COUNT_TRAVERSAL (mcpt_debug.h), else 0 */
    uint64_t prep_exact_nodes; /* light preps whose pick lay within the rounding band of a cumulative-weight
                                * boundary and were redone with the reference's literal formulas and
                                * summation order (Mylight.cpp:335-438), so the pick is the reference's.
                                * The band's constants are calibrated, not a proven bound (DESIGN.md
                                * §4.3.3: tools/prep_error_study.py on the stand-in, tools/band_margin_study.py
                                * on the stress scenes: margins x2.1 (slivers, 32 seeds) to x111, x10 on the
                                * stand-in; tests/test_band_margin.py) */
    double cache_build_seconds; /* device time building the per-pixel root-point cache (in prep_seconds) */
    uint64_t prep_band_nodes;   /* light preps whose slack the whole-table band bound could not clear and
                                 * that took the per-chunk band test (prep_exact_nodes of them failed it) */
    /* ABI 2.2: where a multi-device / multi-rank call's time went */
    double comm_init_seconds;    /* device list: wall time of ncclCommInitAll in THIS call (first call over a
                                  * device set; 0 when the cached communicator is reused).  Created on the
                                  * calling thread before any device work starts.  0 for single-device and
                                  * mcpt_comm calls (mcpt_comm_init_rank is the caller's) */
    double device_setup_seconds; /* device list: max over devices of the worker's setup wall time (device state:
                                  * scene upload + BVH on first use; framebuffer) */
    double device_seconds[MCPT_STATS_MAX_DEVICES]; /* per rank of the call's communicator (distinct devices
                                  * in order of first appearance; entries beyond 16 not recorded): wall time of
                                  * its shards, setup and reduce excluded -- max/min is the load imbalance.
                                  * Single device / mcpt_comm rank: [0] = this call's render time */
    /* ABI 2.3 (appended; a caller with a smaller stats_size gets the prefix) */
    uint64_t pick_table_roots;   /* cached roots (of prep_cached_nodes) whose pick came from the per-run root pick
                                  * table instead of a search of the pixel's cached row */
} mcpt_stats;
/* With several devices, `seconds` is the wall time of the whole call (setup + shards + reduce; comm init
 * excluded), counts are summed over devices and prep_seconds is summed device time. */

int mcpt_version(void);
const char* mcpt_last_error(void);

/* Myobj::read + Mylight::read + gather_light_triangles (Myobj.cpp:10-28, Mylight.cpp:11-100):
 * OBJ/MTL via the tinyobjloader-compatible reader, <light mtlname radiance> via the XML reader. */
int mcpt_scene_load(const char* obj_path, const char* xml_path, mcpt_scene** out);
/* flattened-array form of the same (the reference's data after loading) */
int mcpt_scene_create(const mcpt_scene_desc* desc, mcpt_scene** out);
void mcpt_scene_destroy(mcpt_scene* scene);
int mcpt_scene_counts(const mcpt_scene* scene, int32_t* nfacets, int32_t* nmaterials, int32_t* nlights);
/* device bytes of the acceleration structures the traversal reads (both BVHs' 4-wide nodes and leaf
 * triangles; the reference's counterpart is its uniform grid, Myobj.cpp:110-162) */
int mcpt_scene_accel_bytes(const mcpt_scene* scene, uint64_t* bytes);
/* host copies of the loaded, flattened scene (any pointer may be NULL): the reference's data
 * after Myobj::read / gather_light_triangles, plus Myobj::get_unique_normal_of_facet (Myobj.cpp:680) */
int mcpt_scene_arrays(const mcpt_scene* scene, float* positions, float* normals, int32_t* material_id,
                      float* materials, int32_t* light_facet, double* light_radiance, double* unique_normals);
/* the XML's <camera> block (README.md:339-343; ignored by the reference main.cpp:507-510) */
int mcpt_scene_camera(const mcpt_scene* scene, mcpt_camera* cam);

/* In-place geometry update: facets [first, first + count) get new vertex positions (and, unless `normals` is
 * NULL, new vertex normals); no reference interface corresponds (the reference loads one static scene).
 *
 * The rule: after a successful call the scene behaves as one made by mcpt_scene_create from the new arrays would,
 * for every entry point that takes the handle -- mcpt_closest_hit and mcpt_primary_hits return the same facet and
 * (t, beta, gamma) bit for bit (closest hits are a total order on (t, facet), so they do not depend on how tight the
 * refit boxes are), renders are equal up to the order of the framebuffer's fp64 atomics, and mcpt_scene_arrays returns
 * the new positions and normals with the unique normals of the updated facets recomputed as at load time.  The topology
 * of the BVH stays: on the host the binary tree's boxes are refit, and on every device the scene already lives on the
 * facet and leaf arrays are rewritten and the 4-wide tree's boxes (fp32 and 64-byte quantised nodes) are refit by
 * kernels, level by level; no rebuild, no light-table upload, no new buffers.  The call takes the scene's lock (one
 * render or update at a time per handle); with a communicator every rank must make the same update call.
 *
 * The arena: the scene keeps the bounding box and the box margin of its build; positions must stay inside that box
 * grown by its largest axis extent `ext` on every side.  The margin is 1e-5 * ext + 1e-6 + 3 * 2^-24 * C, C the largest
 * |coordinate| of the ARENA (not of the positions at build time): the last term covers the rounding of the traversals'
 * fp32 slab arithmetic, which grows with the coordinates and not with the extent.  The rule for
 * edited scenes follows: a refit (update, transform, moved lights) and a rebuild use the build's margin unchanged, and
 * it is valid for every position they can be given, because a position outside the arena is refused.  To move a scene
 * farther than its arena, create it at the new place.
 *
 * Refused with MCPT_E_INVALID and a message, before anything on the host or on any device is modified: a NULL scene
 * or NULL positions; count < 1, first < 0 or first + count > nfacets; a stats struct_size mismatch; a facet of the
 * range that is a light triangle (lights cannot move unless mcpt_scene_set_lights_movable, below, switched them to
 * movable for this handle: the first such facet is named); a non-finite position or normal;
 * a position outside the arena; in the device form a pointer that is not device memory on `device`.
 *
 * An update invalidates the host grid (the next MCPT_ACCEL_GRID render or mcpt_scene_meshing call rebuilds it from the
 * new positions; MCPT_HIT_GRID queries need a new mcpt_scene_meshing call) and the opt-in 8-wide debug trees (refused
 * for the handle from its first update on, include/mcpt_debug.h).  Not covered: light triangles (unless switched to movable), topology or
 * facet count changes.  A refit tree degrades as geometry moves far: mcpt_scene_tree_cost measures it and mcpt_scene_rebuild
 * (below) replaces it.  The temporal accumulation follows moved geometry through the scene's previous pose
 * (mcpt_scene_pose_save below, mcpt_temporal_accumulate_motion). */
typedef struct {
    uint32_t struct_size;       /* sizeof(mcpt_update_stats) of the caller's header (mcpt_update_stats_init sets it) */
    int32_t facets;             /* count of the call */
    int64_t leaf_slots;         /* leaf slots rewritten (a facet with spatial-split references has several) */
    int64_t nodes_refit;        /* 4-wide nodes with at least one slot box recomputed, per device state; the first one's */
    int32_t levels;             /* tree levels launched */
    int32_t device_states;      /* device states brought up to date (0: none existed yet) */
    double device_seconds;      /* HIP events around the kernels of the first device state (0 if none) */
} mcpt_update_stats;
void mcpt_update_stats_init(mcpt_update_stats* stats);
/* host arrays: positions count*9 (v0 v1 v2 per facet), normals count*9 or NULL (keep); stats may be NULL */
int mcpt_scene_update(mcpt_scene* scene, int32_t first, int32_t count, const float* positions, const float* normals,
                      mcpt_update_stats* stats);
/* the same from device memory on `device` (-1 = current): the value checks run in a kernel that counts offending
 * values, and the host reads that count back before any modifying kernel is enqueued; the host copy of the scene is
 * brought up to date by a device-to-host copy of the range */
int mcpt_scene_update_device(mcpt_scene* scene, int32_t device, int32_t first, int32_t count, const float* dev_positions,
                             const float* dev_normals, mcpt_update_stats* stats);
/* The previous pose of a scene: the vertex positions and normals of every facet as they were at the last
 * mcpt_scene_pose_save.  The call records the current ones -- on the host copy and, device to device on the state's
 * stream (no host round trip), on every device state the scene has; a device state created later takes its previous
 * pose from the host copy.  Storage is allocated at the first call; until then the previous pose IS the current pose
 * (the same arrays, no copy).  mcpt_scene_update[_device] never touches the previous pose, so a frame loop is
 * pose_save, updates, frame: mcpt_render_motion_aovs then tells where every visible surface point was a frame ago.
 * Takes the scene's lock.  MCPT_E_INVALID for a NULL scene. */
int mcpt_scene_pose_save(mcpt_scene* scene);

/* On-device transforms of facet ranges: "this object is now rotated by M", evaluated where the vertices live
 * (DESIGN.md §4.21).  No reference interface corresponds.
 *
 * mcpt_scene_rest_save records the current positions and normals of every facet as the scene's REST pose: on the host
 * copy, and device to device on every device state (layout of tri_v / tri_n, as pose_save's prev_v / prev_n); a later
 * device state takes it from the host copy.  Brings the host copy up to date first (see mcpt_scene_host_sync).
 * MCPT_E_INVALID: NULL scene.
 *
 * mcpt_scene_transform: facets [first, first + count) := m applied to their REST pose.  m: 3x4 row-major doubles;
 * normal_m: 3x3 row-major doubles for the vertex normals, NULL = the linear part of m.  stats as mcpt_scene_update's
 * (may be NULL); device_seconds covers the transform kernel, the read-back of its count word and the refit.
 *
 * The rule, in fp64 with no contraction (the library is built with -ffp-contract=off on host and device), so that a
 * caller can restate it bit for bit: for a rest vertex (x, y, z), floats widened to double, and row r of m,
 *     out_r = (float)(((m[4r] * x + m[4r+1] * y) + m[4r+2] * z) + m[4r+3])      (round to nearest even)
 * and for a rest vertex normal (nx, ny, nz) and row r of n = normal_m
 *     out_r = (float)((n[3r] * nx + n[3r+1] * ny) + n[3r+2] * nz)
 * which is not normalised (the AOVs normalise at interpolation).  The identity reproduces the rest pose value for value
 * (a -0 becomes +0).  The source is always the rest pose, never the current one, so a frame loop does not drift.
 *
 * After a successful call mcpt_scene_update's rule holds word for word: the scene behaves as mcpt_scene_create of the
 * arrays the rule produces -- hits bit for bit, renders up to the order of the fp64 atomics, mcpt_scene_arrays returns
 * those arrays with the unique normals of the range recomputed as at load time.  The grid and the 8-wide debug trees
 * are invalidated as by an update.
 *
 * Refused with MCPT_E_INVALID and a message, before anything on the host or on any device is modified: a NULL scene or
 * m; count < 1, first < 0 or first + count > nfacets; a stats struct_size mismatch; a light triangle in the range (the
 * first one is named); a non-finite entry of m or normal_m; no rest pose saved yet; a transformed position or normal
 * that is non-finite after the conversion to float; a transformed position outside the arena (mcpt_scene_update's).
 *
 * The host copy is synced lazily.  While the scene has no device state the call computes the new arrays on the host by
 * the rule and is an ordinary mcpt_scene_update of them.  Once a device state exists nothing is computed on the host:
 * every device state evaluates the rule in a kernel from its own rest copy, counts the offending values (read back
 * before any modifying kernel is enqueued), and refits as for an update; the host copy (positions, normals, unique
 * normals, the binary tree) only gets the range recorded as BEHIND.  Everything that reads the host copy brings it up
 * to date first -- mcpt_scene_arrays, a device state on a new device, the grid (mcpt_scene_meshing, MCPT_ACCEL_GRID
 * renders), the mcpt_debug_bvh4_* walks, mcpt_scene_update[_device] (their host refit needs every triangle of a
 * touched leaf) and mcpt_scene_rest_save -- by copying the ranges back from the first device state and running an
 * update's host half over them, so a synced host copy equals an eagerly updated one.  mcpt_scene_pose_save does NOT
 * sync: while ranges are behind it makes its device-to-device copies only, and the host's previous pose follows at the
 * next sync (from the device copy, which changes only at a pose_save).  A frame loop pose_save, transform, frame
 * therefore never waits for the host. */
int mcpt_scene_rest_save(mcpt_scene* scene);
int mcpt_scene_transform(mcpt_scene* scene, int32_t first, int32_t count, const double m[12], const double normal_m[9],
                         mcpt_update_stats* stats);
/* *facets = how many facets of the host copy are behind the devices (0: in sync) */
int mcpt_scene_host_pending(const mcpt_scene* scene, int64_t* facets);
/* brings the host copy up to date now (a no-op when nothing is pending) */
int mcpt_scene_host_sync(mcpt_scene* scene);
/* host helper, Rodrigues as mcpt_camera_orbit: rotation by `degrees` about the axis through `pivot` along axis/|axis|,
 * then + translate (NULL = 0), as a 3x4 matrix.  0 degrees gives the identity's linear part exactly.
 * MCPT_E_INVALID: NULL pointer, non-finite input, axis of length 0. */
int mcpt_transform_rotation(const double axis[3], double degrees, const double pivot[3], const double translate[3],
                            double m[12]);

/* On-device rebuild of the main tree.  Updates and transforms keep the topology of the tree the scene
 * was created with, so the tree gets worse the further geometry moves.  No reference interface corresponds.
 *
 * mcpt_scene_rebuild: on every device state the scene has, the main 4-wide tree -- fp32 nodes, quantised nodes, leaf
 * triangles and the refit's state -- is replaced by one built on that device from its current facet array: Morton order
 * of the facet centroids (63-bit codes, a stable radix sort), a top-down build with one launch per level, numbered
 * breadth-first by scans, one leaf slot per facet, at most 15 node levels for EVERY input (so at most 45 traversal
 * stack entries, fewer than the kernels hold: many coincident triangles give a balanced tree), boxes and quantised
 * nodes by the refit's own kernel.  The tree is a pure function of the positions: the same arrays give the same tree
 * bit for bit.  After a successful call mcpt_scene_update's rule holds word for word: the scene behaves as
 * mcpt_scene_create of the current arrays would -- hits bit for bit, renders up to the order of the fp64 atomics.
 *
 * Untouched: the light-only tree and every light table; the facet arrays, the previous pose and the rest pose; the
 * host copy, including the host's binary tree, which keeps its topology (it is still a valid refit tree, and a device
 * state created later is made from it).  The call does not sync the host: mcpt_scene_host_pending is the same before
 * and after, so a loop of transform, rebuild, frame never waits for the host copy.  It takes the scene's lock and marks
 * the handle as updated: the 8-wide debug trees are refused afterwards.  With a communicator every rank must make the
 * same call.  Later updates and transforms refit the new tree.
 *
 * With no device state the call returns MCPT_OK with device_states = 0 and changes nothing.  MCPT_E_INVALID, before any
 * work: a NULL scene, a stats struct_size mismatch.  The new tree is built beside the one in use and checked (its
 * indices, its traversal-stack need, its leaf codes) before the state's pointers change: should a check fail, that
 * state keeps its old tree and the call returns MCPT_E_SCENE.  Buffers for the build are allocated at a state's first
 * rebuild (two sets of tree arrays for nfacets nodes and slots, used in turn) and reused by every later one.
 *
 * mcpt_scene_tree_cost: the surface-area cost of the fp32 4-wide tree `device` (-1 = current) holds, a quality number a
 * caller can base a rebuild policy on.  With A(box) = 2 (dx dy + dy dz + dz dx) of the float planes widened to double
 * and A0 = A(union of the root's used slots), cost = sum over nodes and used slots k of A(slot k) / A0 * (the slot's
 * triangle count if it is a leaf, else 1); 0 when A0 == 0.  A used slot is one whose child is not the empty marker.
 * Reduced on the device in a fixed order (per-block partials, then index order; no floating-point atomics), so two
 * calls return the same bits.  Creates the device state if needed.  MCPT_E_INVALID: NULL scene or cost. */
typedef struct {
    uint32_t struct_size;    /* sizeof(mcpt_rebuild_stats) of the caller's header (mcpt_rebuild_stats_init sets it) */
    int32_t facets;          /* the scene's facets */
    int32_t nodes, levels;   /* of the new 4-wide tree (the first device state's) */
    int32_t stack_need;      /* the most traversal stack entries the new tree can need */
    int32_t device_states;   /* states rebuilt (0: none existed) */
    double cost_before, cost_after; /* mcpt_scene_tree_cost of the first state */
    double device_seconds;   /* HIP events around the first state's build */
} mcpt_rebuild_stats;
void mcpt_rebuild_stats_init(mcpt_rebuild_stats* stats);
int mcpt_scene_rebuild(mcpt_scene* scene, mcpt_rebuild_stats* stats);
int mcpt_scene_tree_cost(mcpt_scene* scene, int32_t device, double* cost);

/* Movable light triangles.  A per-handle switch, default 0.  While on, mcpt_scene_update[_device] and
 * mcpt_scene_transform accept ranges that contain light triangles; everything else about those calls is unchanged.
 * mcpt_scene_update's rule then holds word for word with light facets included: after a successful call the scene
 * behaves as mcpt_scene_create of the new arrays would -- mcpt_closest_hit (with and without MCPT_HIT_LIGHT_ONLY) and
 * mcpt_primary_hits bit for bit, mcpt_light_prep's weights_sum, count and pick bit for bit, renders in every mode up to
 * the order of the fp64 atomics, mcpt_scene_arrays with the new positions and normals and unique normals recomputed as
 * at load time.  The light table's order, radiances, groups and light_facet do not change, nor do the facet count and
 * which facets are lights: only the geometry does.  On every device state the light tables (vertices, normals, the
 * packed and fp32 records, the pair records, the chunk spheres and (S, K), the band constants, the areas and their
 * running sums) are derived again on the device from the scattered vertices, by the load-time formulas, and the
 * light-only tree is refit in place with the main scene's box margin; the host copy follows as for any facet
 * (at once for mcpt_scene_update, at the next sync for a transform on a scene with device states).
 *
 * Additional refusal while on (MCPT_E_INVALID, before anything on the host or on any device is modified): a light
 * triangle whose new vertices a, b, c give |(b - a) x (c - a)| == 0 or non-finite in fp64 (its unique normal would not
 * be finite).  mcpt_scene_update names the first such facet; the device form and mcpt_scene_transform count the
 * offenders into the same word as the other value checks.  The arena is the scene's, unchanged.  Switching off later
 * only restores the refusals.  Light facets are ordinary rows of the previous pose, so mcpt_scene_pose_save and the
 * motion AOVs follow a directly visible light; the shading that changes under a moved light is the anti-lag's case
 * (mcpt_temporal_accumulate_antilag).  mcpt_scene_rebuild still leaves the light-only tree alone: it keeps its build
 * topology and is only refit.
 *
 * mcpt_scene_set_lights_movable takes the scene's lock; with a communicator every rank must make the same call.
 * MCPT_E_INVALID: a NULL scene (or a NULL `on` of the getter).
 * mcpt_scene_light_update_info: the numbers of the LAST successful update / transform call on this handle (all zero
 * before the first, and `lights` 0 for a call whose range held no light).  MCPT_E_INVALID: NULL scene or out, a
 * struct_size mismatch. */
int mcpt_scene_set_lights_movable(mcpt_scene* scene, int32_t on);
int mcpt_scene_lights_movable(const mcpt_scene* scene, int32_t* on);
typedef struct {
    uint32_t struct_size;      /* sizeof(mcpt_light_update_stats) of the caller's header (the _init sets it) */
    int32_t lights;            /* light triangles in the last update / transform call's range (0: none) */
    int32_t chunks;            /* 64-light chunks whose sphere and (S, K) were recomputed */
    int32_t groups;            /* <light> groups whose running area sums were recomputed */
    int64_t light_nodes_refit; /* nodes of the light-only 4-wide tree with a recomputed slot box (first state) */
    int32_t light_levels;
    double device_seconds;     /* HIP events around the light stage of the first device state (in addition to
                                * mcpt_update_stats.device_seconds, which keeps its meaning) */
} mcpt_light_update_stats;
void mcpt_light_update_stats_init(mcpt_light_update_stats* stats);
int mcpt_scene_light_update_info(const mcpt_scene* scene, mcpt_light_update_stats* out);

/* In-place re-lighting: new radiances for a range of the light table, new rows of the material table.
 * No reference interface corresponds.  The rule is mcpt_scene_update's: after a successful call the scene behaves as
 * mcpt_scene_create of the new arrays WITH THE SCENE'S CURRENT LIGHT GROUPING PASSED AS light_group would -- every light
 * table byte for byte, mcpt_light_prep bit for bit, renders in every mode up to the order of the fp64 atomics,
 * mcpt_scene_arrays with the new radiances and materials -- on the host copy and on every device the scene lives on.
 * The grouping is part of the rule because mcpt_scene_create without light_group infers the groups from runs of equal
 * radiance: a re-light never regroups, even when two neighbouring groups end up with equal radiances.  Unchanged too:
 * the light table's order, light_facet, which facets are lights, the facet, material and group counts, material_id,
 * every tree and all geometry.  The calls work whether mcpt_scene_set_lights_movable is on or off, take the scene's
 * lock (one render or edit at a time per handle), and with a communicator every rank must make the same call.
 *
 * mcpt_scene_set_light_radiance: lights [first_light, first_light + count) of the light table get the radiances rgb
 * (count * 3 doubles).  As mcpt_scene_create forms them: a light's sum is (r + g) + b in fp64, a group's sum is the sum
 * of its FIRST light, and the groups' running sum is added in group order.  On every device state the rows of the
 * radiance and sum tables, the radiance words of the light records, the (S, K) of the 64-light chunks of the range,
 * the band constants and the groups' sums are derived again by kernels on the state's stream, which is synchronised
 * once at the end of the call; neither refit state is needed or built.  A zero radiance is allowed and switches the light off.
 * mcpt_scene_set_light_radiance_device: the same from count * 3 doubles of device memory on `device` (< 0: the current
 * one); the values are checked by a kernel that counts the offenders, read back before any modifying kernel is
 * enqueued; the host copy follows inside the call by one device-to-host copy (nothing is left pending).
 * mcpt_scene_set_materials: rows [first_material, first_material + count) of the material table get mtl (count * 7
 * floats: Kd[3] Ks[3] Ns), on the host copy and by one asynchronous copy on each device state's stream.
 * mcpt_scene_light_groups: group[l] = the index of light l's group (nlights entries, ascending): exactly what
 * mcpt_scene_desc.light_group takes, so a caller can build the fresh scene of the rule.
 *
 * count == 0 succeeds and does nothing.  Refused with MCPT_E_INVALID and a message that names the first offender,
 * before anything on the host or on any device is modified: a NULL scene; count < 0, a first index < 0 or a range that
 * ends behind the table; a NULL array with count > 0; a stats struct_size mismatch; a radiance component or a Kd / Ks /
 * Ns value that is negative or not finite (the device form reports how many); in the device form a pointer that is not
 * device memory on `device`.
 *
 * Not covered: reassigning facets to materials, turning a facet into a light or back, changing the light, material or
 * group counts, the lights of the opt-in 8-wide debug trees, and the history of a surface whose shading changed (the
 * anti-lag's case, mcpt_temporal_accumulate_antilag, as for a moved light). */
typedef struct {
    uint32_t struct_size;   /* sizeof(mcpt_relight_stats) of the caller's header (mcpt_relight_stats_init sets it) */
    int32_t lights;         /* lights given a radiance (count of a radiance call, else 0) */
    int32_t chunks;         /* 64-light chunks of the range: their (S, K) were recomputed */
    int32_t groups;         /* groups whose first light is in the range: their sum was rewritten */
    int32_t materials;      /* material rows written (count of mcpt_scene_set_materials, else 0) */
    int32_t device_states;  /* device states brought up to date (0: none existed yet) */
    double device_seconds;  /* HIP events around the stage on the first device state (0 if none) */
} mcpt_relight_stats;
void mcpt_relight_stats_init(mcpt_relight_stats* stats);
int mcpt_scene_set_light_radiance(mcpt_scene* scene, int32_t first_light, int32_t count, const double* rgb,
                                  mcpt_relight_stats* stats);
int mcpt_scene_set_light_radiance_device(mcpt_scene* scene, int32_t device, int32_t first_light, int32_t count,
                                         const void* dev_rgb, mcpt_relight_stats* stats);
int mcpt_scene_set_materials(mcpt_scene* scene, int32_t first_material, int32_t count, const float* mtl,
                             mcpt_relight_stats* stats);
int mcpt_scene_light_groups(const mcpt_scene* scene, int32_t* group);

/* Facet visibility: ranges of facets hidden and shown again in place.  No reference interface
 * corresponds.  The rule: after a successful call the scene traces and renders as mcpt_scene_create of the current
 * arrays WITHOUT the hidden facets would, with that scene's facet ids mapped back through the monotone old -> new index
 * map -- mcpt_closest_hit and mcpt_primary_hits bit for bit, renders in every mode up to the order of the fp64 atomics.
 *
 * mcpt_scene_set_visible: facets [first, first + count) become invisible (visible == 0) or visible again (any other
 * value).  No ray of any call hits a hidden facet -- camera rays, extension rays, the MIS light-visibility rays,
 * mcpt_closest_hit, mcpt_primary_hits, the AOV and motion-AOV calls, mcpt_render_rays*, the adaptive render and every
 * sequence -- so it occludes nothing and is never shaded.  Everything else about it stays: its index, mcpt_scene_counts,
 * mcpt_scene_arrays and its material.  mcpt_scene_update[_device], mcpt_scene_transform, mcpt_scene_pose_save,
 * mcpt_scene_rest_save and mcpt_scene_host_sync accept hidden facets and store their new values, which appear when the
 * facet is shown.  Hiding a hidden facet or showing a visible one is accepted and does nothing to that facet.
 *
 * How: the facet arrays, the ids, the slot map and every tree's topology stay.  A hidden facet's leaf slots hold its own
 * first vertex three times, which both triangle tests reject exactly (a zero determinant), and the boxes on its path are
 * refit around those points; showing scatters the facet array's vertices back and refits again.  The host copy comes
 * first (a per-facet byte and the host tree's boxes: a device state created later honours the mask), then every device
 * state the handle has, each by one scatter kernel and the refit's per-level kernels on the state's stream, which is
 * synchronised once.  Like mcpt_scene_update the call takes the scene's lock, syncs the host copy first if ranges are
 * pending, and its first success marks the handle as updated (the 8-wide debug trees are refused afterwards).
 * mcpt_scene_rebuild keeps every facet: a hidden one is placed at its point with collapsed slots.  `stats` (may be
 * NULL) is filled as an update fills it.  With a communicator every rank must make the same call.
 *
 * Refused with MCPT_E_INVALID before anything is modified: a NULL scene; count <= 0 or a range outside the scene; a
 * stats struct_size mismatch; a range that contains a light triangle, with or without mcpt_scene_set_lights_movable (the
 * first one is named: hiding a light would change every light table; mcpt_scene_set_light_radiance with zeros switches
 * a light off).  While any facet is hidden, MCPT_ACCEL_GRID, MCPT_HIT_GRID and mcpt_scene_meshing are refused with
 * MCPT_E_INVALID: the reference grid's in-cell rule depends on the scene's box, so a grid without the facets would not
 * be the reference's.
 *
 * mcpt_scene_visibility: visible[f] = 1 / 0 for every facet (nfacets bytes, may be NULL) and the number of hidden
 * facets (may be NULL).  MCPT_E_INVALID: a NULL scene.
 *
 * Not covered: hiding lights; visibility per ray type (camera-only, shadow-only); a rebuild that drops hidden facets
 * from the tree; changing the facet count; consistency across the ranks of a communicator. */
int mcpt_scene_set_visible(mcpt_scene* scene, int32_t first, int32_t count, int32_t visible, mcpt_update_stats* stats);
int mcpt_scene_visibility(const mcpt_scene* scene, uint8_t* visible, int32_t* hidden);

/* main.cpp:547-588: render samples [sample_begin, sample_end) of an spp-sample frame and ADD
 * sum_k L_k * (1/spp) into out_rgb (caller-owned host buffer, height*width*3 doubles, row 0 =
 * top image row).  Devices: opts->device, or opts->devices / opts->comm (see mcpt_render_opts). */
int mcpt_render(mcpt_scene* scene, const mcpt_camera* cam, const mcpt_render_opts* opts, double* out_rgb,
                mcpt_stats* stats);
/* same, accumulating into a DEVICE buffer (height*width*3 doubles on opts->device, devices[0] or the
 * comm's device), without any host round trip.  The buffer must be coarse-grained device memory
 * (hipMalloc, or the torch caching allocator): the framebuffer is updated with hardware fp64
 * atomics, which do not work on fine-grained / managed (hipMallocManaged, hipHostMalloc) memory --
 * such buffers are rejected with MCPT_E_INVALID. */
int mcpt_render_device(mcpt_scene* scene, const mcpt_camera* cam, const mcpt_render_opts* opts,
                       double* dev_out_rgb, mcpt_stats* stats);

/* Radiance along caller-supplied rays (no counterpart in the reference, whose only rays are its camera's): ray r
 * starts at origin[3r..] and runs along dir[3r..] (n*3 doubles each), both used as given -- dir is NOT normalised and
 * the first node's outgoing direction is -dir, so pass unit directions for the reference's shading.  The call ADDS
 * sum_k L_k / spp over the samples k in [sample_begin, sample_end) of ray r into out_rgb[3r..] (n*3 doubles), as
 * mcpt_render does per pixel; sample k of ray r draws the counter-RNG numbers of (seed, pixel = r, sample = k), so
 * the rays of an n-pixel frame give that frame's image.  A ray with a non-finite component or a zero direction is a
 * miss (adds nothing).  opts supplies spp, the sample range, mode, seed, device, flags, samples_per_launch,
 * queue_factor and progress.  The closest hit is traced per sample over the BVH and every root takes the full light
 * prep (prep_cached_nodes = prep_cache_points = 0); stats->camera_samples = n * (sample_end - sample_begin).
 * MCPT_E_INVALID before any device work: n < 1, a NULL array, a device list or a communicator, MCPT_ACCEL_GRID,
 * MCPT_RENDER_PIXEL_JITTER and everything mcpt_render refuses in opts. */
int mcpt_render_rays(mcpt_scene* scene, const mcpt_render_opts* opts, int32_t n, const double* origin, const double* dir,
                     double* out_rgb, mcpt_stats* stats);
/* same with the three arrays in DEVICE memory (coarse-grained, on opts->device; see mcpt_render_device) */
int mcpt_render_rays_device(mcpt_scene* scene, const mcpt_render_opts* opts, int32_t n, const double* dev_origin,
                            const double* dev_dir, double* dev_out_rgb, mcpt_stats* stats);
/* The same radiance for a sparse set of a frame's pixels: ray r carries an explicit pixel id index[r].
 * origin and dir are n*3 doubles read densely, index holds n ids, out_rgb is out_n*3 doubles.  Ray r ADDS
 * sum_k L_k / spp into out_rgb[3*index[r]..], and sample k of ray r draws the counter-RNG numbers of (seed,
 * pixel = index[r], sample = k): the n rays of a frame's pixels index[0..n) give those pixels of mcpt_render_rays over
 * the whole frame, at the cost of n rays.  Nothing else in out_rgb is written.  Duplicate ids are allowed: each entry
 * adds the same samples again.  A broken ray is a miss as above.  stats->camera_samples = n * (sample_end -
 * sample_begin).  MCPT_E_INVALID before any device work: everything mcpt_render_rays refuses, a NULL index, out_n < 1
 * or out_n > 2^28, and an id outside [0, out_n) (the message names the first such entry). */
int mcpt_render_rays_indexed(mcpt_scene* scene, const mcpt_render_opts* opts, int32_t n, const int32_t* index,
                             const double* origin, const double* dir, int32_t out_n, double* out_rgb, mcpt_stats* stats);
/* same with the four arrays in DEVICE memory (coarse-grained, on opts->device; see mcpt_render_device).  The ids cannot
 * be read before the run: the root kernel bound-checks every id before it forms an address from it, a ray whose id lies
 * outside [0, out_n) traces nothing and adds nothing, and the call then returns MCPT_E_INVALID AFTER the run, with a
 * message that says so -- the valid rays' sums have been added, nothing outside the out_n slots has been touched, and
 * *stats is not written. */
int mcpt_render_rays_indexed_device(mcpt_scene* scene, const mcpt_render_opts* opts, int32_t n, const int32_t* dev_index,
                                    const double* dev_origin, const double* dev_dir, int32_t out_n, double* dev_out_rgb,
                                    mcpt_stats* stats);
/* The camera's height*width rays for sample index `sample`, row 0 = top image row, to host arrays (height*width*3
 * doubles each): origin = the pulled-back eye, dir = the unit direction through the pixel's centre (jitter = 0;
 * `seed` and `sample` are then unused) or through MCPT_RENDER_PIXEL_JITTER's offset for (seed, pixel, sample)
 * (jitter = 1).  Computed on `device` (-1 = current) by the function the render's root kernel calls, so these are
 * the render's rays bit for bit: mcpt_render_rays over them reproduces mcpt_render.  MCPT_E_INVALID before any device
 * work: a NULL pointer, an invalid camera, sample < 0, jitter outside 0 and 1. */
int mcpt_camera_rays(const mcpt_camera* cam, uint64_t seed, int32_t sample, int32_t jitter, int32_t device,
                     double* origin, double* dir);

/* Adaptive sampling (no counterpart in the reference, which gives every pixel the same spp, main.cpp:567):
 * the frame is rendered in passes, each active pixel's noise is estimated after every pass, and pixels at or
 * below the threshold stop being sampled.  Sample k of a pixel draws the counter-RNG numbers of a plain
 * render's sample k, so the result can be reproduced from plain renders.
 *   passes   pass 0 renders global sample indices [0, min_spp) of every pixel, each later pass the next
 *            pass_spp indices of the active pixels only; the last pass is cut at max_spp.  A pass [a, b) is
 *            split at h = a + (b - a) / 2 (integer division): samples [a, h) are summed into A, samples
 *            [h, b) into B (raw fp64 sums).
 *   noise    after a pass, for each pixel active in it, with n its sample count: I = (A + B) / n,
 *            Ah = 2 A / n, num = sum_c |I_c - Ah_c|, e = num / sqrt(sum_c I_c) if num > 0, else 0 (Dammertz
 *            et al. 2010, "A Hierarchical Automatic Stopping Condition for Monte Carlo Global Illumination",
 *            with the half buffer taken from the first half of each pass).
 *   active   U = active and e > threshold; next active = active and dilate(U, radius), the dilation over
 *            the (2 radius + 1)^2 square clipped at the frame's border.  A pixel that leaves never returns.
 *            The passes end when no pixel is active or the count reaches max_spp.
 * Single device only: a device list or a communicator is refused, and so is MCPT_RENDER_PIXEL_JITTER. */
typedef struct {
    uint32_t struct_size; /* sizeof(mcpt_adaptive_opts) of the caller's header; a mismatch is MCPT_E_INVALID */
    int32_t min_spp;      /* samples of pass 0: even, >= 2 */
    int32_t pass_spp;     /* samples of each later pass: even, >= 2 */
    int32_t max_spp;      /* the cap: >= min_spp */
    double threshold;     /* tau >= 0: a pixel with e <= tau has converged */
    int32_t radius;       /* 0..4: an unconverged pixel keeps its neighbours within this distance active */
} mcpt_adaptive_opts;
/* zero-fills *opts and sets struct_size, min_spp = 16, pass_spp = 16, max_spp = 1024, threshold = 0.05,
 * radius = 1 (a pixel whose first samples are all black has e = 0; its neighbours keep it sampled) */
void mcpt_adaptive_opts_init(mcpt_adaptive_opts* opts);
/* Renders adaptively and ADDS (A + B) / count per pixel into out_rgb (as mcpt_render adds its weighted sum);
 * count (int32 per pixel: samples taken) and noise (double per pixel: the last e computed for it) are
 * overwritten; either may be NULL.  `base` supplies mode, seed, device, accel, flags, progress,
 * samples_per_launch and queue_factor; its spp, sample_begin and sample_end must be left as
 * mcpt_render_opts_init set them, and num_devices / comm must be unset (MCPT_E_INVALID otherwise).
 * stats: summed over the passes; camera_samples is the sum of the count map, prep_cache_points is counted
 * once (the root-point cache is built once per call). */
int mcpt_render_adaptive(mcpt_scene* scene, const mcpt_camera* cam, const mcpt_render_opts* base,
                         const mcpt_adaptive_opts* adaptive, double* out_rgb, int32_t* count, double* noise,
                         mcpt_stats* stats);
/* same with the three maps in DEVICE memory (coarse-grained, on base->device; see mcpt_render_device) */
int mcpt_render_adaptive_device(mcpt_scene* scene, const mcpt_camera* cam, const mcpt_render_opts* base,
                                const mcpt_adaptive_opts* adaptive, double* dev_out_rgb, int32_t* dev_count,
                                double* dev_noise, mcpt_stats* stats);

/* Primary-hit feature buffers (AOVs; no counterpart in the reference): what the first hit of every pixel's
 * camera ray looks like, for filters that must not blur across geometry.  Row 0 = top image row.  For a pixel
 * whose primary ray hits facet f at (beta, gamma), exactly as mcpt_primary_hits reports it:
 *   position  height*width*3: the interpolated hit point (main.cpp:406)
 *   normal    height*width*3: the normalised interpolation of f's vertex normals (main.cpp:407); NOT flipped
 *             for a back face
 *   depth     height*width:   the Euclidean distance from the primary ray's origin (the pulled-back eye) to
 *             position
 *   albedo    height*width*3: Kd + Ks of f's material per channel (the floats widened to double, then added)
 * A miss writes 0 to all four; depth == 0 is the miss marker (a hit has depth > 0).  Any pointer may be NULL. */
typedef struct {
    double *albedo, *normal, *position, *depth;
} mcpt_aov_buffers;
/* Fills the host arrays of *out.  opts supplies device and accel only (every other field is ignored); a
 * device list or a communicator is MCPT_E_INVALID.  Runs the per-call setup of a render (primary hits, root
 * table) and one kernel that writes the maps; no sample is traced. */
int mcpt_render_aovs(mcpt_scene* scene, const mcpt_camera* cam, const mcpt_render_opts* opts,
                     const mcpt_aov_buffers* out);
/* same with the arrays in DEVICE memory (coarse-grained, on opts->device; see mcpt_render_device) */
int mcpt_render_aovs_device(mcpt_scene* scene, const mcpt_camera* cam, const mcpt_render_opts* opts,
                            const mcpt_aov_buffers* dev_out);
/* Motion AOVs: where the surface point a pixel shows was in the scene's PREVIOUS pose (mcpt_scene_pose_save).  For a
 * pixel whose primary ray hits facet f at (beta, gamma) in the CURRENT pose, exactly as mcpt_primary_hits reports it:
 *   prev_position  height*width*3: the interpolation of position above with the previous pose's vertices of f
 *   prev_normal    height*width*3: the normalised interpolation of the previous pose's vertex normals of f
 * -- the function that gives position and normal, on the other arrays; before any mcpt_scene_pose_save both maps equal
 * mcpt_render_aovs' position and normal bit for bit.  A miss writes 0.  Either pointer may be NULL. */
typedef struct {
    double *prev_position, *prev_normal;
} mcpt_motion_buffers;
/* As mcpt_render_aovs: the same arguments, refusals and per-call setup (primary hits, root table), then one kernel
 * that reads the primary hits and writes the two maps. */
int mcpt_render_motion_aovs(mcpt_scene* scene, const mcpt_camera* cam, const mcpt_render_opts* opts,
                            const mcpt_motion_buffers* out);
/* same with the arrays in DEVICE memory (coarse-grained, on opts->device; see mcpt_render_device) */
int mcpt_render_motion_aovs_device(mcpt_scene* scene, const mcpt_camera* cam, const mcpt_render_opts* opts,
                                   const mcpt_motion_buffers* dev_out);

/* Variance-guided edge-avoiding a-trous wavelet filter (Dammertz et al. 2010, "Edge-Avoiding A-Trous Wavelet
 * Transform for fast Global Illumination Filtering", with the luminance edge-stopping function scaled by the
 * local standard deviation as in Schied et al. 2017, "Spatiotemporal Variance-Guided Filtering"), on one
 * frame, in fp64 throughout.  Inputs: the colour C_0 (height*width*3), an optional per-pixel variance V_0 of
 * the pixel's mean luminance (height*width) and the four guides of an mcpt_aov_buffers: N normal, X position,
 * rho albedo and depth.  With hit(p) = depth_p > 0, h = (1/16, 1/4, 3/8, 1/4, 1/16) indexed by d + 2 and
 * eps = 1e-10, iteration i = 0 .. iterations - 1 with step s = 2^i computes for every pixel p
 *   l(p)     = (C_i(p).r + C_i(p).g + C_i(p).b) / 3
 *   Vg(p)    = the 3x3 Gaussian (1/4, 1/2, 1/4)^2 of V_i around p; taps outside the frame are dropped and the
 *              remaining weights renormalised (sum of weight * V_i over the sum of the weights)
 *   sigma(p) = sigma_color * sqrt(max(Vg(p), 0)) + eps
 *   taps     q = p + s * (dx, dy) for dx, dy in [-2, 2]; taps outside the frame are skipped
 *   geo(p,q) = w_n * w_x * w_a when both p and q hit, 1 when both miss, 0 when exactly one hits, with
 *              w_n = max(0, N_p . N_q)^sigma_normal
 *              w_x = exp(-|N_p . (X_q - X_p)| / (sigma_plane * depth_p))
 *              w_a = exp(-|rho_p - rho_q|^2 / sigma_albedo^2)
 *   w        = h(dx) * h(dy) * geo(p, q) * exp(-|l(p) - l(q)| / sigma(p))
 *   C_{i+1}(p) = sum_q w C_i(q) / sum_q w
 *   V_{i+1}(p) = sum_q w^2 V_i(q) / (sum_q w)^2          (the centre tap, w = 9/64, keeps sum_q w > 0)
 * The results are out = C_K and out_variance = V_K, K = iterations; both are overwritten, not added to.
 * When variance is NULL, V_0 is a two-pass spatial estimate over the clipped 5x5 window at step 1:
 *   u(q) = h(dx) * h(dy) * geo(p, q),  m = sum_q u l(q) / sum_q u,  V_0(p) = sum_q u (l(q) - m)^2 / sum_q u
 * (the one-pass form m2 - m1^2 cancels, and the square root that follows amplifies its error).
 * The filter is normalised, hence biased: it trades variance for blur, smears highlights far brighter than
 * their surroundings when their variance is large, and without a supplied variance it treats an emitter's
 * edge as noise.  Single device. */
typedef struct {
    uint32_t struct_size;  /* sizeof(mcpt_denoise_opts) of the caller's header; a mismatch is MCPT_E_INVALID */
    int32_t iterations;    /* 1..8, default 5: iteration i uses step 2^i */
    double sigma_color;    /* default 4: luminance edge-stopping, in standard deviations */
    double sigma_normal;   /* default 128: exponent of the normal weight */
    double sigma_plane;    /* default 0.01: distance from p's tangent plane, relative to depth_p */
    double sigma_albedo;   /* default 0.1: albedo distance (RGB Euclidean) */
    int32_t device;        /* HIP device ordinal (-1 = current) */
} mcpt_denoise_opts;
/* zero-fills *opts and sets struct_size and the defaults above (device = -1) */
void mcpt_denoise_opts_init(mcpt_denoise_opts* opts);
/* Host arrays in, host arrays out.  guides: all four arrays are required.  variance (height*width) may be
 * NULL (the spatial estimate), out_variance (height*width) and device_seconds (device time of the filter's
 * kernels, HIP events) may be NULL.  Refused with MCPT_E_INVALID before any device work: a struct_size
 * mismatch, iterations outside 1..8, a sigma that is not finite or not > 0, width or height < 1, a NULL
 * colour, output or guide array, out (or out_variance) aliasing an input array. */
int mcpt_denoise(const mcpt_denoise_opts* opts, int32_t width, int32_t height, const double* color,
                 const double* variance, const mcpt_aov_buffers* guides, double* out, double* out_variance,
                 double* device_seconds);
/* same with every array in DEVICE memory on opts->device (device_seconds stays a host pointer) */
int mcpt_denoise_device(const mcpt_denoise_opts* opts, int32_t width, int32_t height, const double* dev_color,
                        const double* dev_variance, const mcpt_aov_buffers* dev_guides, double* dev_out,
                        double* dev_out_variance, double* device_seconds);
/* Host helper: the adaptive render's outputs (image I = rgb, noise e) as V_0 = (e * sqrt(sum_c I_c) / 3)^2 per
 * pixel (0 where sum_c I_c <= 0): the squared mean absolute channel difference between I and the rescaled
 * first half buffer Ah (e sqrt(sum I) = sum_c |I_c - Ah_c|), a one-sample estimate of the variance of the
 * pixel's mean luminance.  rgb height*width*3, noise and variance height*width. */
int mcpt_variance_from_noise(int32_t width, int32_t height, const double* rgb, const double* noise, double* variance);

/* Temporal accumulation: the other half of Schied et al. 2017 (SVGF).  The scene is static, so the world position
 * of a pixel's primary hit is projected into the PREVIOUS frame's camera, the previous frame's accumulated colour
 * and luminance moments are gathered there (bilinear, every tap's geometry checked), blended with the current
 * frame, and a per-pixel variance of the accumulated luminance comes out for mcpt_denoise.  fp64 throughout.
 * Inputs for a frame of width w, height h: the current colour C (h*w*3), the current guides (N normal, X position,
 * depth; albedo is read by the spatial estimate only) and, optionally, the previous state: its camera cam', its
 * guides N', X', depth' (its albedo is ignored), its colour history Hc' (h*w*3) and its moments Hm' (h*w*4,
 * interleaved (m1, m2, n, g)).
 *   frame    of cam', as the renderer builds it (main.cpp:507-510): wv = lookat - eye, the pulled-back eye
 *            E = eye - wv * (dist_scale - 1), Nc = wv / |wv|, V = (Nc x up) / |Nc x up|, U = (V x Nc) / |V x Nc|,
 *            S = wlen / pixellen with wlen = |wv * dist_scale| and pixellen = tan(fovy / 360) * wlen / (h / 2)
 * For each pixel p = (i, j) (row, column), with l = (C.r + C.g + C.b) / 3:
 *   source   when depth_p > 0: d = X_p - E, a = d . U, b = d . V, c = d . Nc; when also c > 0:
 *            y = (h - 1) / 2 - S * a / c, x = (w - 1) / 2 + S * b / c (the inverse of the camera ray's direction).
 *            p has NO source when depth_p == 0, or c <= 0, or !(y > -1 && y < h && x > -1 && x < w)
 *   taps     i0 = floor(y), j0 = floor(x), fy = y - i0, fx = x - j0; q = (i0 + di, j0 + dj) for (di, dj) = (0, 0),
 *            (0, 1), (1, 0), (1, 1) in this order, with b_q = (di ? fy : 1 - fy) * (dj ? fx : 1 - fx).  A tap is
 *            valid when it lies inside the frame, depth'_q > 0, n'_q > 0, N_p . N'_q >= normal_min and
 *            |N_p . (X'_q - X_p)| <= plane_max * depth_p (a surface point keeps its world position, so the
 *            plane distance is taken in world space)
 *   history  Wsum = sum of b_q over the valid taps; p has history when it has a source and Wsum >= min_weight;
 *            then (Hc, m1', m2', n', g') = (sum of b_q * the tap's values) / Wsum, n' and g' as doubles
 *   blend    with history: n = min(n' + 1, max_history), A = max(alpha, 1 / n), out_color = (1 - A) Hc + A C,
 *            m1 = (1 - A) m1' + A l, m2 = (1 - A) m2' + A l^2, g = (1 - A)^2 g' + A^2;
 *            without (and whenever no previous state is given): out_color = C, (m1, m2, n, g) = (l, l^2, 1, 1).
 *            g is the sum of the squared blend weights: one frame's variance times g is the variance of the
 *            blended value (g = 1 / n while the blend is an arithmetic mean)
 *   variance when n > variance_min_history - 0.5 and g < 1: V = max(0, m2 - m1^2) * g / (1 - g), the empirical
 *            per-frame luminance variance with the small-sample correction, scaled to the accumulated value;
 *            otherwise V is the spatial estimate V_0 of mcpt_denoise above, word for word (u-weighted, two passes
 *            over the clipped 5x5 at step 1), of out_color with the current guides and this call's sigma_normal,
 *            sigma_plane and sigma_albedo.  The - 0.5 keeps the decision away from the integers n takes in a
 *            static sequence; g < 1 fails only for alpha = 1, where nothing is accumulated.
 * out_color (h*w*3), out_moments (h*w*4) and out_variance (h*w, optional) are overwritten.  The history is the
 * caller's: feed out_color / out_moments of one call as prev_color / prev_moments of the next (two sets of buffers,
 * swapped; an output may not alias an input).  The filtered colour is NOT fed back, miss pixels keep no history,
 * and the reprojection follows the camera only: geometry moved by mcpt_scene_update is followed by
 * mcpt_temporal_accumulate_motion below (changed shading on static surfaces, a moving shadow, is what the clamped
 * form is for).  Single device. */
typedef struct {
    uint32_t struct_size;  /* sizeof(mcpt_temporal_opts) of the caller's header; a mismatch is MCPT_E_INVALID */
    int32_t max_history;   /* default 64, >= 1: the cap of the history length n */
    int32_t variance_min_history; /* default 4, >= 2: with a shorter history the variance is the spatial estimate */
    int32_t device;        /* HIP device ordinal (-1 = current) */
    double alpha;          /* default 0.1, in (0, 1]: the smallest weight of the current frame */
    double normal_min;     /* default 0.9, finite: a tap needs N_p . N'_q >= normal_min */
    double plane_max;      /* default 0.02, finite and > 0: and lies within plane_max * depth_p of p's tangent plane */
    double min_weight;     /* default 0.01, in (0, 1]: the least bilinear weight of the valid taps */
    double sigma_normal;   /* default 128 */
    double sigma_plane;    /* default 0.01    the spatial estimate's geo(p, q), as in mcpt_denoise_opts */
    double sigma_albedo;   /* default 0.1 */
} mcpt_temporal_opts;
/* zero-fills *opts and sets struct_size and the defaults above (device = -1) */
void mcpt_temporal_opts_init(mcpt_temporal_opts* opts);
/* Host arrays in, host arrays out.  guides: all four arrays are required.  The previous state -- prev_cam,
 * prev_guides (normal, position and depth required), prev_color, prev_moments -- is given whole or not at all
 * (all NULL: every pixel starts a history); prev_cam's width and height must equal width and height.
 * out_variance and device_seconds (device time of the kernels, HIP events) may be NULL.  Refused with
 * MCPT_E_INVALID before any device work: a struct_size mismatch, an option outside the range above (sigmas:
 * finite and > 0), width or height < 1, a NULL required array, a partial previous state, a previous camera of
 * another size, an output aliasing an input or another output. */
int mcpt_temporal_accumulate(const mcpt_temporal_opts* opts, const mcpt_camera* prev_cam, int32_t width, int32_t height,
                             const double* color, const mcpt_aov_buffers* guides, const mcpt_aov_buffers* prev_guides,
                             const double* prev_color, const double* prev_moments, double* out_color,
                             double* out_moments, double* out_variance, double* device_seconds);
/* same with every array in DEVICE memory on opts->device (prev_cam and device_seconds stay host pointers) */
int mcpt_temporal_accumulate_device(const mcpt_temporal_opts* opts, const mcpt_camera* prev_cam, int32_t width,
                                    int32_t height, const double* dev_color, const mcpt_aov_buffers* dev_guides,
                                    const mcpt_aov_buffers* dev_prev_guides, const double* dev_prev_color,
                                    const double* dev_prev_moments, double* dev_out_color, double* dev_out_moments,
                                    double* dev_out_variance, double* device_seconds);

/* Temporal accumulation with history clamping (opt-in; mcpt_temporal_accumulate above is unchanged).  The long
 * history ghosts view-dependent shading once the camera moves: the reprojected surface point is the same, its
 * radiance towards the new camera is not.  The remedy of the SVGF descendants (variance clipping against a fast
 * history, as in ReLAX): keep a second history Hf that forgets within a few frames, and clamp the long one per pixel
 * and channel to mean +- sigma * standard deviation of the fast history over a small window.  The state gains the
 * fast history (h*w*3): prev_fast in, out_fast out.
 * Everything of mcpt_temporal_accumulate's rule up to and including `blend` is unchanged; call its results S (the
 * colour) and (m1, m2, n, g).  Then, for each pixel p:
 *   fast     gathered from prev_fast with the same taps, validity tests, b_q and Wsum as Hc; with history:
 *            A_f = max(alpha_fast, 1 / n) with the same n, F = (1 - A_f) Hf + A_f C; without: F = C.  out_fast = F:
 *            what mcpt_temporal_accumulate returns as colour for alpha = alpha_fast, prev_color = prev_fast and
 *            the same prev_moments, bit for bit
 *   box      only when p has history (which implies depth_p > 0): over the taps q of the clipped
 *            (2 radius + 1)^2 window around p with depth_q > 0 (the current depth), rows top to bottom, columns
 *            left to right, k of them, per channel c: mu_c = (sum of F_q,c) / k, then
 *            sd_c = sqrt((sum of (F_q,c - mu_c)^2) / k), lo_c = mu_c - sigma * sd_c, hi_c = mu_c + sigma * sd_c.
 *            Two passes, not sum x^2 - (sum x)^2 / k, for the reason given for V_0 above
 *   clamp    out_color_c = min(max(S_c, lo_c), hi_c).  With l_S = (S.r + S.g + S.b) / 3 and l_out the same of
 *            out_color: shift = l_out - l_S, m1 <- m1 + shift, m2 <- m2 + (m1_new^2 - m1_old^2) (the central moment
 *            m2 - m1^2 is kept), n and g unchanged.  Without history: out_color = C, moments (l, l^2, 1, 1), shift 0
 *   variance as in mcpt_temporal_accumulate, from the clamped out_color and the corrected moments: the temporal
 *            formula where it applies, otherwise V_0 of the clamped out_color
 * out_shift (h*w, optional) is the shift per pixel, 0 where nothing moved: a continuous quantity, so two
 * implementations can be compared without a discrete "was clamped" decision.  sigma = 0 replaces the history by the
 * window's mean; a large sigma clamps nothing except where the window's deviation is 0 (a single hit tap).  The
 * clamped colour is the history of the next call, and so is out_fast.  It costs accuracy where there is nothing to
 * fix: on a static camera the box cuts into the long history's converged values. */
typedef struct {
    uint32_t struct_size; /* sizeof(mcpt_temporal_clamp_opts) of the caller's header; a mismatch is MCPT_E_INVALID */
    int32_t radius;       /* default 2, 1..3: the (2 radius + 1)^2 window of the fast history */
    double alpha_fast;    /* default 0.5, in (0, 1]: the smallest weight of the current frame in the fast history */
    double sigma;         /* default 2, finite and >= 0: the box is mean +- sigma * standard deviation, per channel */
} mcpt_temporal_clamp_opts;
/* zero-fills *clamp and sets struct_size and the defaults above */
void mcpt_temporal_clamp_opts_init(mcpt_temporal_clamp_opts* clamp);
/* As mcpt_temporal_accumulate, with prev_fast (part of the previous state: given with it or not at all), out_fast
 * (required) and out_shift (may be NULL).  Refused with MCPT_E_INVALID before any device work: everything
 * mcpt_temporal_accumulate refuses, a NULL clamp, a clamp struct_size mismatch, a radius, alpha_fast or sigma outside
 * the ranges above, a NULL out_fast, a previous state without prev_fast or prev_fast alone, out_fast or out_shift
 * aliasing an input or another output (and an output aliasing prev_fast). */
int mcpt_temporal_accumulate_clamped(const mcpt_temporal_opts* opts, const mcpt_temporal_clamp_opts* clamp,
                                     const mcpt_camera* prev_cam, int32_t width, int32_t height, const double* color,
                                     const mcpt_aov_buffers* guides, const mcpt_aov_buffers* prev_guides,
                                     const double* prev_color, const double* prev_moments, const double* prev_fast,
                                     double* out_color, double* out_moments, double* out_fast, double* out_variance,
                                     double* out_shift, double* device_seconds);
/* same with every array in DEVICE memory on opts->device (opts, clamp, prev_cam and device_seconds stay host pointers) */
int mcpt_temporal_accumulate_clamped_device(const mcpt_temporal_opts* opts, const mcpt_temporal_clamp_opts* clamp,
                                            const mcpt_camera* prev_cam, int32_t width, int32_t height,
                                            const double* dev_color, const mcpt_aov_buffers* dev_guides,
                                            const mcpt_aov_buffers* dev_prev_guides, const double* dev_prev_color,
                                            const double* dev_prev_moments, const double* dev_prev_fast,
                                            double* dev_out_color, double* dev_out_moments, double* dev_out_fast,
                                            double* dev_out_variance, double* dev_out_shift, double* device_seconds);

/* Temporal accumulation with object motion (opt-in; the two forms above are unchanged).  Between the previous frame
 * and this one geometry may have moved in place (mcpt_scene_update after mcpt_scene_pose_save): the surface point
 * pixel p shows now lay elsewhere, and was oriented otherwise, when the previous frame's history was written.  The
 * motion AOVs of this frame (mcpt_render_motion_aovs) say where: Xm = prev_position, Nm = prev_normal.  The rule is
 * mcpt_temporal_accumulate's -- mcpt_temporal_accumulate_clamped's when clamp is not NULL -- word for word, with
 * exactly three substitutions:
 *   source   d = Xm_p - E (the previous position is what the previous camera saw)
 *   taps     a tap needs Nm_p . N'_q >= normal_min
 *            and |Nm_p . (X'_q - Xm_p)| <= plane_max * depth_p; depth_p stays the CURRENT depth
 * Everything else reads the current guides: depth_p > 0 decides whether p has a source at all, `blend`, the moments,
 * the fast history and the box of the clamp, and the spatial estimate of the variance.  With Xm = X and Nm = N (a
 * scene that did not move) the outputs are those of the plain or clamped call bit for bit.  What it does not do: no
 * screen-space motion vectors come out, lights do not move, and shading that changes on a static surface is the
 * anti-lag's job (mcpt_temporal_accumulate_antilag below) or, without it, the clamp's.
 * Host arrays in, host arrays out; the arguments are those of the two forms above.  motion: both arrays are required.
 * clamp == NULL selects the plain rule; prev_fast, out_fast and out_shift must then be NULL.  With clamp, prev_fast
 * belongs to the previous state, out_fast is required and out_shift may be NULL.  Refused with MCPT_E_INVALID before
 * any device work: everything the plain call (clamp == NULL) or the clamped call refuses, a NULL motion struct or
 * array, an output aliasing a motion array, a fast-history or shift argument without clamp. */
int mcpt_temporal_accumulate_motion(const mcpt_temporal_opts* opts, const mcpt_temporal_clamp_opts* clamp,
                                    const mcpt_camera* prev_cam, int32_t width, int32_t height, const double* color,
                                    const mcpt_aov_buffers* guides, const mcpt_motion_buffers* motion,
                                    const mcpt_aov_buffers* prev_guides, const double* prev_color,
                                    const double* prev_moments, const double* prev_fast, double* out_color,
                                    double* out_moments, double* out_fast, double* out_shift, double* out_variance,
                                    double* device_seconds);
/* same with every array in DEVICE memory on opts->device (opts, clamp, prev_cam and device_seconds stay host pointers) */
int mcpt_temporal_accumulate_motion_device(const mcpt_temporal_opts* opts, const mcpt_temporal_clamp_opts* clamp,
                                           const mcpt_camera* prev_cam, int32_t width, int32_t height,
                                           const double* dev_color, const mcpt_aov_buffers* dev_guides,
                                           const mcpt_motion_buffers* dev_motion, const mcpt_aov_buffers* dev_prev_guides,
                                           const double* dev_prev_color, const double* dev_prev_moments,
                                           const double* dev_prev_fast, double* dev_out_color, double* dev_out_moments,
                                           double* dev_out_fast, double* dev_out_shift, double* dev_out_variance,
                                           double* device_seconds);

/* Anti-lag by temporal gradients (Schied et al. 2018, "Gradient Estimation for Temporally Stable Real-Time Path
 * Tracing"; opt-in, no counterpart in the reference; every form above is unchanged).  The accumulation reprojects
 * geometry, but radiance that changed on a surface that did not move -- a dimmed light, a moved lamp's shadow, a
 * re-tinted wall -- is blended at alpha for about 1 / alpha frames.  The remedy: a sparse subset of the PREVIOUS frame's
 * samples is traced again, with the previous camera and the previous seed, in the CURRENT scene.  The counter RNG is
 * keyed by (seed, pixel, sample), so the two radiances differ only by what changed in the scene: their difference is a
 * noise-free measure of that change, and the blend weight is raised where it is large.
 *   options  mcpt_gradient_opts: the stratum s (one gradient sample per s x s block of the previous frame's pixels), the
 *            radius r (a window of (2 r + 1)^2 strata) and a scale on the ratio
 *   phase    (a, b) with 0 <= a, b < s picks the sample pixel (s I + a, s J + b) of stratum (I, J).  The phase of frame
 *            k (mcpt_gradient_phase) is mcpt_upsample_phase's rule for s in 1..8: k' = k mod s^2, a = k' mod s,
 *            b = (a + k' div s) mod s -- a bijection onto the s^2 phases
 *   rays     mcpt_gradient_rays(cam, s, a, b): height*width rays.  Every origin is the pulled-back eye.  The direction of
 *            pixel (i, j) is mcpt_camera_rays(cam, jitter = 0)'s direction bit for bit (the same device function) when
 *            i mod s == a and j mod s == b; every other direction is (0, 0, 0), which mcpt_render_rays treats as a miss
 *            that traces nothing.  mcpt_render_rays over these arrays with seed S therefore adds, at index p of a
 *            selected pixel, the radiance mcpt_render(cam, seed S) gives pixel p, and nothing anywhere else
 *   gradient mcpt_temporal_gradient: prev_raw is the previous frame's raw render, regrad the radiance along the gradient
 *            rays (both h*w*3); out_lambda is hs*ws with hs = (h + s - 1) / s, ws = (w + s - 1) / s (integer division),
 *            overwritten.  For stratum (I, J) with sample pixel q = (s I + a, s J + b): if q lies inside the frame,
 *            num(I, J) = sum over c of |regrad_c(q) - prev_raw_c(q)| and den(I, J) = sum over c of
 *            fmax(regrad_c(q), prev_raw_c(q)), c = r, g, b in this order starting from the first term; otherwise both
 *            are 0.  Num and Den are the sums of num and den over the strata (I + di, J + dj) with |di|, |dj| <= r that
 *            lie inside the grid, rows top to bottom and columns left to right, starting from 0.
 *            Lambda(I, J) = 0 when !(Den > 0); otherwise x = scale * Num / Den and Lambda = x < 1 ? x : 1, so a NaN
 *            gives 1.  fp64, with no contraction
 *   accumulation  mcpt_temporal_accumulate_antilag: mcpt_temporal_accumulate_motion's rule word for word (with motion ==
 *            NULL the current guides are used, which is the plain or the clamped rule), with these substitutions for a
 *            pixel that has history:
 *            lookup        qi = min(max((int)floor(ys + 0.5), 0), h - 1) and qj likewise from xs and w, (ys, xs) the
 *                          `source` step's coordinates; L = lambda[(qi / s) * ws + qj / s] (integer divisions);
 *                          l = L > 0 ? (L < 1 ? L : 1) : 0
 *            blend         n = min(n' + 1, max_history), A0 = max(alpha, 1 / n), A = A0 + l * (1 - A0); colour, m1, m2
 *                          and g are blended with this A exactly as before (g = (1 - A)^2 g' + A^2); the stored
 *                          history length is n_out = (1 - l) * n + l
 *            fast history  Af0 = max(alpha_fast, 1 / n) with the same n (not n_out), Af = Af0 + l * (1 - Af0)
 *            Everything else -- the box, the shift, the variance with n_out and g, the spatial estimate -- is unchanged.
 *            With lambda == 0 everywhere every output equals the plain, clamped or motion call's BIT FOR BIT:
 *            A0 + 0 * (1 - A0) = A0 and 1 * n + 0 = n.
 * What the gradient sees: a change of radiance along the previous camera's own rays -- re-lit lights, edited materials,
 * moved lights, moved occluders and moved geometry.  What it does not see: view-dependent change from camera motion
 * (the rays are the previous camera's); that stays the clamp's job.  The samples are not forward-projected and the
 * gradient is not filtered beyond the window sum.  Single device. */
typedef struct {
    uint32_t struct_size; /* sizeof(mcpt_gradient_opts) of the caller's header; a mismatch is MCPT_E_INVALID */
    int32_t stratum;      /* default 3, 1..8: one gradient sample per stratum x stratum block of pixels */
    int32_t radius;       /* default 1, 0..3: Num and Den are summed over (2 radius + 1)^2 strata */
    int32_t device;       /* HIP device ordinal (-1 = current) */
    double scale;         /* default 1, finite and > 0: multiplier on Num / Den */
} mcpt_gradient_opts;
/* zero-fills *opts and sets struct_size and the defaults above (device = -1) */
void mcpt_gradient_opts_init(mcpt_gradient_opts* opts);
/* Host helper: the phase of frame `frame_index` at `stratum` (1..8).  MCPT_E_INVALID for a NULL pointer or a stratum
 * outside 1..8. */
int mcpt_gradient_phase(int32_t stratum, uint64_t frame_index, int32_t* a, int32_t* b);
/* The gradient rays of `cam` (see `rays` above) to host arrays, height*width*3 doubles each, computed on `device`
 * (-1 = current).  MCPT_E_INVALID before any device work: a NULL pointer, an invalid camera, a frame of more than 2^28
 * pixels, a stratum outside 1..8, a phase outside [0, stratum). */
int mcpt_gradient_rays(const mcpt_camera* cam, int32_t stratum, int32_t a, int32_t b, int32_t device, double* origin,
                       double* dir);
/* same with origin and dir in DEVICE memory on `device` */
int mcpt_gradient_rays_device(const mcpt_camera* cam, int32_t stratum, int32_t a, int32_t b, int32_t device,
                              double* dev_origin, double* dev_dir);
/* Host helper, no device work: the selected pixels of phase (a, b) in a width x height frame, as a list.  With
 * hs' = a < height ? (height - a + stratum - 1) / stratum : 0 and ws' likewise from b and width (integer division),
 * *count = hs' * ws' -- which may be 0, as for a 2 x 2 frame at stratum 3 with phase (2, 2) -- and entry r = I * ws' + J
 * is pixel (stratum I + a) * width + stratum J + b: strictly increasing.  index may be NULL (the count only), else it
 * takes *count entries.  MCPT_E_INVALID: a NULL count, width or height < 1 or a frame of more than 2^28 pixels, a
 * stratum outside 1..8, a phase outside [0, stratum). */
int mcpt_gradient_index(int32_t width, int32_t height, int32_t stratum, int32_t a, int32_t b, int32_t* count, int32_t* index);
/* The gradient rays of the selected pixels alone, for mcpt_render_rays_indexed: mcpt_gradient_index's count entries of
 * the index (count int32), the pulled-back eye as origin and the pixel's direction (count*3 doubles each) -- the rays
 * mcpt_gradient_rays gives the selected pixels, bit for bit (the same device function).  With count == 0 the call
 * succeeds and writes nothing.  The checks are mcpt_gradient_rays' own, and a NULL index. */
int mcpt_gradient_rays_indexed(const mcpt_camera* cam, int32_t stratum, int32_t a, int32_t b, int32_t device, int32_t* index,
                               double* origin, double* dir);
/* same with the three arrays in DEVICE memory on `device` */
int mcpt_gradient_rays_indexed_device(const mcpt_camera* cam, int32_t stratum, int32_t a, int32_t b, int32_t device,
                                      int32_t* dev_index, double* dev_origin, double* dev_dir);
/* Host arrays in, host array out (see `gradient` above).  device_seconds (device time of the kernel, HIP events) may be
 * NULL.  Refused with MCPT_E_INVALID before any device work: a NULL opts, a struct_size mismatch, a stratum, radius or
 * scale out of range, a phase outside [0, stratum), width or height < 1 or a frame of more than 2^28 pixels, a NULL
 * array, out_lambda aliasing an input. */
int mcpt_temporal_gradient(const mcpt_gradient_opts* opts, int32_t width, int32_t height, int32_t a, int32_t b,
                           const double* prev_raw, const double* regrad, double* out_lambda, double* device_seconds);
/* same with the three arrays in DEVICE memory on opts->device */
int mcpt_temporal_gradient_device(const mcpt_gradient_opts* opts, int32_t width, int32_t height, int32_t a, int32_t b,
                                  const double* dev_prev_raw, const double* dev_regrad, double* dev_out_lambda,
                                  double* device_seconds);
/* Host arrays in, host arrays out; the arguments are mcpt_temporal_accumulate_motion's plus gradient (read for its
 * stratum only, but checked whole) and lambda (the hs*ws map of mcpt_temporal_gradient at that stratum).  motion may be
 * NULL (the current guides are then used); clamp may be NULL as in the motion call.  Refused with MCPT_E_INVALID before
 * any device work: everything the motion call refuses (a NULL motion struct excepted), a NULL gradient or lambda, a
 * struct_size mismatch, a stratum, radius or scale out of range, an output aliasing lambda. */
int mcpt_temporal_accumulate_antilag(const mcpt_temporal_opts* opts, const mcpt_temporal_clamp_opts* clamp,
                                     const mcpt_camera* prev_cam, int32_t width, int32_t height, const double* color,
                                     const mcpt_aov_buffers* guides, const mcpt_motion_buffers* motion,
                                     const mcpt_aov_buffers* prev_guides, const double* prev_color,
                                     const double* prev_moments, const double* prev_fast, double* out_color,
                                     double* out_moments, double* out_fast, double* out_shift, double* out_variance,
                                     double* device_seconds, const mcpt_gradient_opts* gradient, const double* lambda);
/* same with every array in DEVICE memory on opts->device (the option structs, prev_cam and device_seconds stay host
 * pointers) */
int mcpt_temporal_accumulate_antilag_device(const mcpt_temporal_opts* opts, const mcpt_temporal_clamp_opts* clamp,
                                            const mcpt_camera* prev_cam, int32_t width, int32_t height,
                                            const double* dev_color, const mcpt_aov_buffers* dev_guides,
                                            const mcpt_motion_buffers* dev_motion, const mcpt_aov_buffers* dev_prev_guides,
                                            const double* dev_prev_color, const double* dev_prev_moments,
                                            const double* dev_prev_fast, double* dev_out_color, double* dev_out_moments,
                                            double* dev_out_fast, double* dev_out_shift, double* dev_out_variance,
                                            double* device_seconds, const mcpt_gradient_opts* gradient,
                                            const double* dev_lambda);

/* Guided upsampling (joint bilateral upsampling, Kopf et al. 2007; no counterpart in the reference): trace at 1 / f of
 * the shown size and reconstruct the full-size frame from the low-size radiance and full-size guides.  A camera's
 * extent does not depend on its pixel count (pixellen = tan(fovy/360) |w| / (height / 2) and a row's offset is
 * pixellen (i - (H - 1) / 2)), so the camera with f times the rows and columns (mcpt_camera_scaled) covers the same
 * image plane: low-size pixel I spans the full-size rows f I .. f I + f - 1, its centre at full-size row
 * f I + (f - 1) / 2.  Inputs: the low-size colour C (h*w*3), the low-size guides g (normal N, position X, albedo rho,
 * depth) at h x w, the full-size guides G at (f h) x (f w), the integer factor f.  All arithmetic is fp64, with no
 * contraction.  For each full-size pixel p = (i, j):
 *   source   y = (i - (f - 1) / 2.0) / f, x = (j - (f - 1) / 2.0) / f; i0 = floor(y), j0 = floor(x), fy = y - i0,
 *            fx = x - j0
 *   taps     q = (i0 + di, j0 + dj) for (di, dj) = (0, 0), (0, 1), (1, 0), (1, 1) in this order; taps outside the low
 *            frame are skipped; b_q = (di ? fy : 1 - fy) * (dj ? fx : 1 - fx)
 *   weight   w_q = b_q * geo(p, q), geo the denoiser's (mcpt_denoise above) with the centre taken from G at p (so the
 *            plane term uses sigma_plane * depth_p of G) and the tap from g at q: w_n w_x w_a when both hit, 1 when
 *            both miss, 0 when exactly one hits
 *   result   Wsum = sum of w_q; if Wsum >= min_weight, out(p) = (sum of w_q C(q)) / Wsum; otherwise the fallback
 *            out(p) = C(i / f, j / f) (integer division: the low pixel that contains p), and p counts as a fallback
 *            pixel
 * out ((f h)*(f w)*3) is overwritten, not added to.  The fallback count is an integer reduced with integer atomics:
 * exact, and the same on every run.  The albedo is not demodulated, the variance is not upsampled, f is an integer and
 * nothing is searched beyond the four taps.  Single device. */
typedef struct {
    uint32_t struct_size;  /* sizeof(mcpt_upsample_opts) of the caller's header; a mismatch is MCPT_E_INVALID */
    int32_t factor;        /* default 2, 2..4: the full frame is factor times the low one along each axis */
    double sigma_normal;   /* default 128 */
    double sigma_plane;    /* default 0.01    geo(p, q), as in mcpt_denoise_opts */
    double sigma_albedo;   /* default 0.1 */
    double min_weight;     /* default 1e-4, finite and in (0, 1]: below this sum of weights a pixel takes the fallback */
    int32_t device;        /* HIP device ordinal (-1 = current) */
} mcpt_upsample_opts;
/* zero-fills *opts and sets struct_size and the defaults above (device = -1) */
void mcpt_upsample_opts_init(mcpt_upsample_opts* opts);
/* Host arrays in, host arrays out.  width and height are the LOW size; color and guides hold height*width pixels,
 * full_guides and out (factor*height)*(factor*width).  All four arrays of both guide sets are required.
 * fallback_count (the number of fallback pixels) and device_seconds (device time of the kernel, HIP events) may be
 * NULL.  Refused with MCPT_E_INVALID before any device work: a struct_size mismatch, factor outside 2..4, a sigma that
 * is not finite or not > 0, a min_weight that is not finite or outside (0, 1], width or height < 1 or a full frame of
 * more than 2^28 pixels, a NULL colour or output array, a NULL array in either guide set, out aliasing an input. */
int mcpt_upsample(const mcpt_upsample_opts* opts, int32_t width, int32_t height, const double* color,
                  const mcpt_aov_buffers* guides, const mcpt_aov_buffers* full_guides, double* out,
                  uint64_t* fallback_count, double* device_seconds);
/* same with every array in DEVICE memory on opts->device (fallback_count and device_seconds stay host pointers) */
int mcpt_upsample_device(const mcpt_upsample_opts* opts, int32_t width, int32_t height, const double* dev_color,
                         const mcpt_aov_buffers* dev_guides, const mcpt_aov_buffers* dev_full_guides, double* dev_out,
                         uint64_t* fallback_count, double* device_seconds);
/* Host helper: *out = *in with width * factor and height * factor -- the one definition of "the full-size camera of a
 * low-size camera".  MCPT_E_INVALID for a NULL pointer, factor < 1, a width or height < 1 or a product beyond 32 bits.
 * in and out may be the same struct. */
int mcpt_camera_scaled(const mcpt_camera* in, int32_t factor, mcpt_camera* out);

/* Temporal upsampling (no counterpart in the reference): instead of tracing a low-size camera and guessing the pixels
 * in between (mcpt_upsample), every frame traces a different 1 / f^2 subset of the FULL-size camera's pixels -- those
 * with row mod f == a and column mod f == b, the frame's phase (a, b) -- and accumulates them in a full-size history,
 * so that a static or slowly moving camera converges to a full-resolution image at the tracing cost of a low one.
 * Inputs: the factor f (mcpt_upsample_opts.factor, 2..4), the phase (a, b) with 0 <= a, b < f, the low size w x h (the
 * full size is W = f w, H = f h), the low colour C (h*w*3) where C(I, J) is the radiance of FULL-size pixel
 * (f I + a, f J + b) through that pixel's centre (mcpt_camera_phase_rays gives those rays), this frame's full-size
 * guides G and, optionally, the previous state AT FULL SIZE: its full-size camera, its guides G', its colour Hc'
 * (H*W*3) and its moments Hm' (H*W*4, interleaved (m1, m2, n, g)).  All arithmetic is fp64, with no contraction.  For
 * each full-size pixel p = (i, j):
 *   traced   p is traced when i mod f == a and j mod f == b; then c = C(i / f, j / f) (integer division) and
 *            l = (c.r + c.g + c.b) / 3
 *   history  mcpt_temporal_accumulate's `source`, `taps` and `history` steps word for word, at W x H with G, G' and the
 *            previous camera (a tap with n'_q == 0 is invalid, as there): "p has history" and, if so,
 *            (Hc, m1', m2', n', g')
 *   traced, with history     mcpt_temporal_accumulate's `blend` with C = c
 *   traced, without history  out = c, moments (l, l^2, 1, 1)
 *   untraced, with history   out = Hc, moments (m1', m2', n', g'): nothing is blended and n is not incremented
 *   untraced, without history (the fill)
 *            source   y = (i - a) / f, x = (j - b) / f (as doubles); i0 = floor(y), j0 = floor(x), fy = y - i0,
 *                     fx = x - j0
 *            taps     the low pixels q = (i0 + di, j0 + dj) for (di, dj) = (0, 0), (0, 1), (1, 0), (1, 1) in this order;
 *                     taps outside the low frame are skipped; b_q = (di ? fy : 1 - fy) * (dj ? fx : 1 - fx)
 *            weight   w_q = b_q * geo(p, q'), geo the denoiser's with mcpt_upsample_opts' sigmas, the centre G at p, the
 *                     tap G at q' = (f q_i + a, f q_j + b), the full-size pixel q was traced through (no low-size
 *                     guides exist in this mode)
 *            result   Wsum = sum of w_q; if Wsum >= mcpt_upsample_opts.min_weight, out = (sum of w_q C(q)) / Wsum;
 *                     otherwise the fallback out = C(I*, J*) with I* = clamp(floor(y + 0.5), 0, h - 1) and J* likewise
 *                     from x and w (the nearest traced pixel), and p counts as a fallback pixel
 *            moments  (l_out, l_out^2, 0, 1): n = 0 marks a value that is nobody's sample.  It is shown, but it never
 *                     serves as history (its tap is invalid in the next frame)
 *   variance as in mcpt_temporal_accumulate, from out and the moments: the temporal formula where
 *            n > variance_min_history - 0.5 and g < 1, otherwise the spatial estimate V_0 of out with G and
 *            mcpt_temporal_opts' sigmas
 *   counts   filled = the pixels in the fill case, fallback = those of them that took the fallback; integers reduced
 *            with integer atomics, exact and the same on every run
 * The phase of frame k (mcpt_upsample_phase): k' = k mod f^2, a = k' mod f, b = (a + k' div f) mod f -- a bijection onto
 * the f^2 phases, for f = 2: (0,0), (1,1), (0,1), (1,0).  A pixel is traced every f^2-th frame, so its history forgets
 * over f^2 / alpha frames, not 1 / alpha.  The history is not clamped, samples and guides are not jittered, f is an
 * integer.  Single device. */
/* Host helper: the phase of frame `frame_index` at `factor` (2..4).  MCPT_E_INVALID for a NULL pointer or a factor
 * outside 2..4. */
int mcpt_upsample_phase(int32_t factor, uint64_t frame_index, int32_t* a, int32_t* b);
/* The (height / factor) * (width / factor) rays of full_cam's pixels (factor I + a, factor J + b), row-major in (I, J):
 * origin and dir n*3 each (host arrays), computed on `device` (-1 = current) by the function the render's root kernel
 * calls, so they are mcpt_camera_rays(full_cam)'s rays at those pixels bit for bit.  MCPT_E_INVALID before any device
 * work: a NULL pointer, an invalid camera, a factor outside 2..4, a width or height that factor does not divide, a
 * phase outside [0, factor). */
int mcpt_camera_phase_rays(const mcpt_camera* full_cam, int32_t factor, int32_t a, int32_t b, int32_t device,
                           double* origin, double* dir);
/* same with origin and dir in DEVICE memory on `device` */
int mcpt_camera_phase_rays_device(const mcpt_camera* full_cam, int32_t factor, int32_t a, int32_t b, int32_t device,
                                  double* dev_origin, double* dev_dir);
/* Host arrays in, host arrays out.  width and height are the LOW size: color holds height*width pixels, every other
 * array (factor*height)*(factor*width).  full_guides: all four arrays are required.  The previous state --
 * prev_full_cam, prev_full_guides (normal, position and depth required), prev_color, prev_moments -- is given whole or
 * not at all; prev_full_cam must be (factor*width) x (factor*height).  out_color, out_moments and out_variance
 * (optional) are overwritten.  filled_count, fallback_count and device_seconds (device time of the kernels, HIP events)
 * may be NULL.  temporal->device selects the device (upsample->device is ignored).  Refused with MCPT_E_INVALID before
 * any device work: everything mcpt_temporal_accumulate and mcpt_upsample refuse (a struct_size mismatch or an option out
 * of range in either struct, a NULL required array, a partial previous state, a previous camera of another size, an
 * output aliasing an input or another output, width or height < 1 or a full frame of more than 2^28 pixels) and a
 * phase outside [0, factor). */
int mcpt_temporal_upsample(const mcpt_temporal_opts* temporal, const mcpt_upsample_opts* upsample, int32_t a, int32_t b,
                           const mcpt_camera* prev_full_cam, int32_t width, int32_t height, const double* color,
                           const mcpt_aov_buffers* full_guides, const mcpt_aov_buffers* prev_full_guides,
                           const double* prev_color, const double* prev_moments, double* out_color, double* out_moments,
                           double* out_variance, uint64_t* filled_count, uint64_t* fallback_count, double* device_seconds);
/* same with every array in DEVICE memory on temporal->device (the options, prev_full_cam, the counts and device_seconds
 * stay host pointers) */
int mcpt_temporal_upsample_device(const mcpt_temporal_opts* temporal, const mcpt_upsample_opts* upsample, int32_t a,
                                  int32_t b, const mcpt_camera* prev_full_cam, int32_t width, int32_t height,
                                  const double* dev_color, const mcpt_aov_buffers* dev_full_guides,
                                  const mcpt_aov_buffers* dev_prev_full_guides, const double* dev_prev_color,
                                  const double* dev_prev_moments, double* dev_out_color, double* dev_out_moments,
                                  double* dev_out_variance, uint64_t* filled_count, uint64_t* fallback_count,
                                  double* device_seconds);

/* Host helper: *out = *in with eye rotated by `degrees` about the axis through lookat along k = up / |up|
 * (Rodrigues, right-handed): with v = eye - lookat, t = degrees * pi / 180 and vp = v - k (k . v),
 * eye' = eye + (k x v) sin t - vp (1 - cos t); 0 degrees returns eye bit for bit.  MCPT_E_INVALID for a NULL
 * pointer, a degrees that is not finite or an up of length 0.  in and out may be the same struct. */
int mcpt_camera_orbit(const mcpt_camera* in, double degrees, mcpt_camera* out);

/* Myobj::cal_scene_boundingbox(eye) + Myobj::meshing(n0) (Myobj.cpp:78-162): build the scene's
 * uniform grid (box of every vertex and `eye`; cell edge = largest extent / n0^(1/3)) for
 * MCPT_HIT_GRID queries.  Renders with MCPT_ACCEL_GRID build their own for their camera. */
int mcpt_scene_meshing(mcpt_scene* scene, const double eye[3], int32_t n0);
/* the current grid: box_and_cell = (xmin, xmax, ymin, ymax, zmin, zmax, cell edge), cells per axis */
int mcpt_scene_grid_info(const mcpt_scene* scene, double* box_and_cell, int32_t* cells);

/* Myobj::closet_ray_intersect (Myobj.cpp:334) / closet_ray_intersect_light_triangle (:476) for a
 * batch of n rays (host arrays): ro/rd n*3, exclude n (origin facet, -1 none) ->
 * facet (or -1) and t, beta, gamma (n*3).  flags: MCPT_HIT_LIGHT_ONLY (the light-only query),
 * MCPT_HIT_GRID (the reference's grid of mcpt_scene_meshing instead of the BVH). */
int mcpt_closest_hit(mcpt_scene* scene, int32_t n, const double* ro, const double* rd, const int32_t* exclude,
                     int32_t flags, int32_t* facet, double* tbg);
/* Mylight::prepared_for_lights_spherical_triangle_sampling (Mylight.cpp:322) at n shading points
 * (x1, normal) -> weights_sum, survivor count, and the FACET of the light triangle picked by the
 * counter-RNG rule for uniform u[k] (first survivor with cumulative weight >= u*weights_sum;
 * -1 if empty or weights_sum < 1e-8). */
int mcpt_light_prep(mcpt_scene* scene, int32_t n, const double* x1, const double* normal, const double* u,
                    double* weights_sum, int32_t* count, int32_t* pick);
/* primary-hit map of main.cpp:563-572 for a camera: facet (or -1), t, beta, gamma per pixel */
int mcpt_primary_hits(mcpt_scene* scene, const mcpt_camera* cam, int32_t* facet, double* tbg);

/* RadianceRGB::tone_mapping (RadianceRGB.cpp:51-67) of an HDR frame + the EasyX saveimage BMP
 * layout (32-bpp BI_RGB, bottom-up) of main.cpp:583-596 */
int mcpt_tone_map(const double* rgb, int32_t width, int32_t height, double max_radiance, double gamma,
                  uint8_t* out_rgb8);
int mcpt_write_bmp(const char* path, const uint8_t* rgb8, int32_t width, int32_t height);
/* mcpt_tone_map over DEVICE memory on `device` (-1 = current): dev_rgb height*width*3 doubles, dev_rgb8 as many
 * bytes.  The same rule value by value: A = pow(max_radiance, -gamma) on the host, r = A * pow(v, gamma) and
 * x = floor(r * 255 + 0.5) on the device; the level is 0 when !(x >= -2^31 && x < 2^31) (NaN, infinities and huge
 * values: the reference's x86 out-of-range conversion), else x clamped to 0..255.  The device's pow is not the
 * host's, so a value whose 255 r + 0.5 lies within 1e-9 * max(1, |255 r + 0.5|) of an integer may come out one
 * level off mcpt_tone_map's; every other value is the same byte.  Refused with MCPT_E_INVALID before any device
 * work: a NULL pointer, width or height < 1, a max_radiance or gamma that is not finite or not > 0. */
int mcpt_tone_map_device(const double* dev_rgb, int32_t width, int32_t height, double max_radiance, double gamma,
                         uint8_t* dev_rgb8, int32_t device);

/* What a frame sequence prints about its history, reduced on the device: over the moments (height*width*4, (m1, m2,
 * n, g) of mcpt_temporal_accumulate) *kept = the pixels with n > 1.5 and *history_sum = the sum of n over the pixels
 * with n > 0; over the optional shift map (height*width, mcpt_temporal_accumulate_clamped's) *moved = the pixels with
 * shift != 0 (0 when dev_shift is NULL).  Any output may be NULL.  Deterministic: per-block partial sums in a fixed
 * lane and wave order, then one pass over the partials in index order -- no floating-point atomics, so two runs
 * give the same bits and the counts are exact.  MCPT_E_INVALID before any device work for a NULL dev_moments or a
 * width or height < 1. */
int mcpt_frame_stats_device(const double* dev_moments, const double* dev_shift, int32_t width, int32_t height,
                            int32_t device, uint64_t* kept, double* history_sum, uint64_t* moved);

/* A frame sequence resident on one device: render, AOVs, temporal accumulation, statistics, filter and tone map of
 * every frame run on buffers the handle allocated once in mcpt_sequence_create; per frame only the 8-bit image (when
 * asked for) and a few dozen bytes of statistics cross to the host.  The stages are the existing device forms
 * (mcpt_render_device, mcpt_render_aovs_device, the rules of mcpt_temporal_accumulate[_clamped] and mcpt_denoise)
 * and mcpt_tone_map_device, so every buffer holds what those calls would have produced from the same inputs.  The
 * history is the unfiltered accumulated colour; the filtered colour is not fed back.  One device, no adaptive
 * sampling.  The scene must outlive the handle; one call at a time per handle. */
typedef struct mcpt_sequence mcpt_sequence;
typedef struct {
    uint32_t struct_size; /* sizeof(mcpt_sequence_opts) of the caller's header; a mismatch is MCPT_E_INVALID */
    int32_t width, height;
    int32_t spp;          /* samples per pixel of every frame, >= 1 */
    int32_t denoise;      /* 0: show the accumulated colour; 1: filter it (mcpt_denoise's rule) */
    int32_t clamp;        /* 0: mcpt_temporal_accumulate's rule; 1: mcpt_temporal_accumulate_clamped's */
    double tone_max, tone_gamma; /* defaults 380, 0.25 (main.cpp:583): finite and > 0 */
    uint32_t info_size;   /* sizeof(mcpt_sequence_info) of the caller's header (mcpt_sequence_opts_init sets it): a
                           * frame writes at most this many bytes of its info */
} mcpt_sequence_opts;
/* zero-fills *opts and sets struct_size, info_size, spp = 1, denoise = 1, clamp = 0 and the tone map's defaults;
 * width and height are the caller's to set */
void mcpt_sequence_opts_init(mcpt_sequence_opts* opts);
/* `base` supplies mode, device, accel, flags, samples_per_launch, queue_factor and progress, as for
 * mcpt_render_adaptive: its spp, sample_begin and sample_end must be left as mcpt_render_opts_init set them (the
 * samples come from opts->spp, the seed from each frame) and a device list or a communicator is refused.  temporal
 * is required; clamp is required when opts->clamp, denoise when opts->denoise (otherwise they are ignored); the
 * device fields of the stage options are ignored, base->device is the sequence's.  Refused with MCPT_E_INVALID
 * before any device work: a NULL argument, a struct_size mismatch of any struct, the conditions above, spp < 1,
 * width or height < 1, a tone_max or tone_gamma that is not finite or not > 0, a mode or accel that does not exist
 * and everything the stage option structs' own calls refuse.  Allocates every buffer of a frame (MCPT_E_DEVICE when
 * that fails). */
int mcpt_sequence_create(mcpt_scene* scene, const mcpt_render_opts* base, const mcpt_sequence_opts* opts,
                         const mcpt_temporal_opts* temporal, const mcpt_temporal_clamp_opts* clamp,
                         const mcpt_denoise_opts* denoise, mcpt_sequence** out);
typedef struct {
    /* device time (HIP events).  render: mcpt_stats.seconds of the frame's render; aov: the window of
     * mcpt_render_aovs_device; temporal: the accumulation's kernels and the statistics reduction; denoise: the
     * filter's kernels (0 without denoise); tonemap: the tone map's kernel */
    double render_seconds, aov_seconds, temporal_seconds, denoise_seconds, tonemap_seconds;
    double kept;          /* share of the pixels with a history length n > 1.5 */
    double mean_history;  /* (sum of n over the pixels with n > 0) / (width * height) */
    double clamped;       /* share of the pixels the clamp moved (shift != 0); 0 without clamp */
    uint64_t frame_index; /* frames since create or the last reset, this one not counted: 0 starts every history */
} mcpt_sequence_info;
/* One frame: zero the raw buffer, render [0, spp) with `seed` into it, write the AOVs, accumulate onto the previous
 * frame's state (none on the first frame and after a reset), reduce the statistics, filter (if denoise), tone-map
 * the shown frame (the filtered colour if denoise, else the accumulated one) and, when out_rgb8 is not NULL, copy
 * its height*width*3 bytes to the host; then the two sets of history buffers swap.  The stages after the AOVs go to
 * the null stream and the frame ends with one synchronisation.  info and stats (the render's; base->stats_size
 * bytes) may be NULL.  MCPT_E_INVALID before any device work: a NULL handle or camera, an invalid camera, a camera
 * whose width or height is not the handle's.  A failed frame leaves the history as it was (the buffers of the last
 * frame are then no longer readable until the next frame succeeds). */
int mcpt_sequence_frame(mcpt_sequence* seq, const mcpt_camera* cam, uint64_t seed, uint8_t* out_rgb8,
                        mcpt_sequence_info* info, mcpt_stats* stats);
/* the last frame's buffers: RAW the render (h*w*3), ACCUMULATED (h*w*3), MOMENTS (h*w*4), VARIANCE (h*w), FILTERED
 * (h*w*3; with denoise), FAST (h*w*3) and SHIFT (h*w) (with clamp), RGB8 (h*w*3 bytes; mcpt_sequence_device_buffer
 * only) */
enum { MCPT_SEQ_RAW = 0, MCPT_SEQ_ACCUMULATED = 1, MCPT_SEQ_MOMENTS = 2, MCPT_SEQ_VARIANCE = 3, MCPT_SEQ_FILTERED = 4,
       MCPT_SEQ_FAST = 5, MCPT_SEQ_SHIFT = 6, MCPT_SEQ_RGB8 = 7 };
/* a sequence created by mcpt_sequence_create_upsampled only: UPSAMPLED the shown full-size frame ((f h)*(f w)*3
 * doubles); its RGB8 is that frame's (f h)*(f w)*3 bytes.  Refused (an unknown selector) by any other sequence */
enum { MCPT_SEQ_UPSAMPLED = 8 };
/* copies one of them to the host.  MCPT_E_INVALID: a NULL argument, an unknown selector (RGB8 included), FAST or
 * SHIFT without clamp, FILTERED without denoise, no frame since create / reset / a failed frame */
int mcpt_sequence_read(mcpt_sequence* seq, int32_t what, double* host_out);
/* the device pointer of one of them (on the sequence's device), valid until the next frame, reset or destroy; the
 * same refusals, RGB8 allowed */
int mcpt_sequence_device_buffer(mcpt_sequence* seq, int32_t what, const void** dev_ptr);
/* the next frame starts every history (as the first frame did); the buffers stay allocated */
int mcpt_sequence_reset(mcpt_sequence* seq);
void mcpt_sequence_destroy(mcpt_sequence* seq);
/* A sequence that renders at opts->width x opts->height and shows factor times that (mcpt_upsample's rule;
 * mcpt_sequence_create and mcpt_sequence_opts are unchanged).  upsample is required (its device field is ignored);
 * everything mcpt_sequence_create and mcpt_upsample refuse is refused here, the full frame's size included.  Every
 * buffer is still allocated once, here: the full-size guides, the upsampled colour and the full-size 8-bit frame too.
 * mcpt_sequence_frame still takes the render-size camera.  A frame runs render, AOVs, accumulation, statistics and
 * filter at the render size exactly as a plain sequence does (those buffers hold the same bits), then the AOVs of
 * mcpt_camera_scaled(cam, factor) into the full-size guides, mcpt_upsample's kernel on the shown low frame (the
 * filtered colour if denoise, else the accumulated one), the tone map of the full-size frame and the copy: out_rgb8 is
 * then (f h)*(f w)*3 bytes.  MCPT_RENDER_PIXEL_JITTER moves the samples, not the guides, as in a plain sequence. */
int mcpt_sequence_create_upsampled(mcpt_scene* scene, const mcpt_render_opts* base, const mcpt_sequence_opts* opts,
                                   const mcpt_temporal_opts* temporal, const mcpt_temporal_clamp_opts* clamp,
                                   const mcpt_denoise_opts* denoise, const mcpt_upsample_opts* upsample,
                                   mcpt_sequence** out);
/* the last frame's new stages (HIP events): guide_seconds the window of the full-size mcpt_render_aovs_device,
 * upsample_seconds the upsampling kernel; fallback_share = fallback pixels / full-size pixels.  Any output may be
 * NULL.  MCPT_E_INVALID: a NULL handle, a sequence created without upsampling, no frame since create / reset / a
 * failed frame.  (mcpt_sequence_info is not extended; its tonemap_seconds is the full-size tone map's.) */
int mcpt_sequence_upsample_info(mcpt_sequence* seq, double* guide_seconds, double* upsample_seconds,
                                double* fallback_share);
/* A sequence that traces opts->width x opts->height rays a frame and accumulates them at factor times that size
 * (mcpt_temporal_upsample's rule; the other constructors are unchanged).  mcpt_sequence_frame still takes the
 * render-size camera.  A frame takes its phase from frame_index (mcpt_upsample_phase), writes the phase rays of
 * mcpt_camera_scaled(cam, factor), zeroes the low raw buffer, traces the rays (mcpt_render_rays_device: n = w h, the
 * frame's seed, ray r draws the random numbers of pixel r), renders the full-size AOVs, runs mcpt_temporal_upsample's
 * kernels onto the previous full-size state, reduces the statistics over the full-size moments, filters at full size (if
 * denoise), tone-maps the full-size frame and copies its (f h)*(f w)*3 bytes out; then the history buffers swap.  Every
 * buffer is allocated here.  Selectors: RAW is h*w*3 (the traced samples, row-major in (I, J)); ACCUMULATED, MOMENTS,
 * VARIANCE, FILTERED and RGB8 are full size; FAST, SHIFT and UPSAMPLED are refused.  mcpt_sequence_info's kept and
 * mean_history are over the full-size pixels, its render_seconds the traced rays', its aov_seconds the full-size
 * guides'.  Refused with MCPT_E_INVALID: everything mcpt_sequence_create_upsampled refuses, opts->clamp (the history
 * clamp is not defined for this rule), MCPT_RENDER_PIXEL_JITTER and MCPT_ACCEL_GRID in base (mcpt_render_rays refuses
 * them).  The traced rays share no root-point cache (see mcpt_render_rays): the mode is for few-spp sequences. */
int mcpt_sequence_create_temporal_upsampled(mcpt_scene* scene, const mcpt_render_opts* base, const mcpt_sequence_opts* opts,
                                            const mcpt_temporal_opts* temporal, const mcpt_denoise_opts* denoise,
                                            const mcpt_upsample_opts* upsample, mcpt_sequence** out);
/* the last frame's phase (a, b), rays_seconds the phase-ray kernel's device time (HIP events), filled_share = fill pixels
 * / full-size pixels and fallback_share = fallback pixels / full-size pixels.  Any output may be NULL.
 * MCPT_E_INVALID: a NULL handle, a sequence not created by mcpt_sequence_create_temporal_upsampled, no frame since create
 * / reset / a failed frame. */
int mcpt_sequence_temporal_upsample_info(mcpt_sequence* seq, int32_t* a, int32_t* b, double* rays_seconds,
                                         double* filled_share, double* fallback_share);
/* Object motion in a sequence created by mcpt_sequence_create: on != 0 makes every frame from the next one on run the
 * motion AOVs (mcpt_render_motion_aovs' kernel, on the primary-hit tables the frame's AOVs just built: no second
 * primary trace) after the AOVs and accumulate by mcpt_temporal_accumulate_motion's rule, plain or clamped as the
 * sequence was created; 0 returns to the rule it was created with.  The two maps are allocated at the first call
 * with on != 0.  The caller saves the pose (mcpt_scene_pose_save, then the updates, then the frame); the sequence
 * never does.  MCPT_E_INVALID: a NULL handle, a sequence created by mcpt_sequence_create_upsampled or
 * mcpt_sequence_create_temporal_upsampled (motion there is not supported). */
int mcpt_sequence_set_motion(mcpt_sequence* seq, int32_t on);
/* the last frame's motion stage (HIP events around the motion AOVs; mcpt_sequence_info.aov_seconds does not include
 * it).  MCPT_E_INVALID: a NULL handle, a last frame that ran without motion, no frame since create / reset / a failed
 * frame.  motion_seconds may be NULL. */
int mcpt_sequence_motion_info(mcpt_sequence* seq, double* motion_seconds);
/* the last frame's motion AOVs (h*w*3 each), for mcpt_sequence_read and mcpt_sequence_device_buffer; refused while
 * motion is off (and until a frame has run with it) */
enum { MCPT_SEQ_PREV_POSITION = 9, MCPT_SEQ_PREV_NORMAL = 10 };
/* Anti-lag in a sequence created by mcpt_sequence_create: gradient != NULL makes every frame from the next one on keep
 * its raw frame and its seed (a device-to-device copy), and -- when a history exists and the previous frame kept its raw
 * frame -- run the gradient pass before its render: the phase from frame_index (mcpt_gradient_phase), mcpt_gradient_rays
 * of the PREVIOUS camera, mcpt_render_rays_device over them (the sequence's mode, spp and flags, n = width * height, the
 * PREVIOUS seed) into a zeroed buffer, mcpt_temporal_gradient's kernel against the kept raw frame and a deterministic
 * reduction of Lambda's mean and maximum (per-block partials in a fixed order, then index order; no floating-point
 * atomics).  The frame then accumulates by mcpt_temporal_accumulate_antilag's rule, with motion when that is on and
 * with the clamp when the sequence was created with it.  When the pass does not run (the first frame, the first frame
 * after a reset or after the switch) Lambda is zero-filled and the frame is the plain rule's bit for bit.  NULL switches
 * it off: the frames are then those of a sequence that never had it.  The buffers (two ray arrays, the gradient raw
 * frame, the kept raw frame, a Lambda map of one double a pixel -- enough for stratum 1 -- and the reduction's words,
 * whose number does not depend on the frame or the stratum) are an allocation of their own, made at the first
 * switch-on.  mcpt_sequence_info and the stats argument of a frame describe the main render only.
 * mcpt_sequence_reset drops the kept raw frame.  MCPT_E_INVALID: a NULL handle, a sequence created by
 * mcpt_sequence_create_upsampled or mcpt_sequence_create_temporal_upsampled, a base with MCPT_RENDER_PIXEL_JITTER or
 * MCPT_ACCEL_GRID (mcpt_render_rays refuses both), invalid options (mcpt_temporal_gradient's checks; the device field is
 * ignored). */
int mcpt_sequence_set_antilag(mcpt_sequence* seq, const mcpt_gradient_opts* gradient);
/* the last frame's anti-lag stage: *ran 1 when the gradient pass ran, else 0; the phase (a, b); trace_seconds the
 * gradient render's mcpt_stats.seconds (0 when it did not run); kernel_seconds the ray, gradient and reduction kernels
 * alone (HIP events; the buffers' zero fills are outside them; when the pass did not run: the reduction); Lambda's
 * mean and maximum over the hs*ws strata.  Any output may be NULL.  MCPT_E_INVALID: a NULL handle, a last frame that
 * ran without anti-lag, no frame since create / reset / a failed frame. */
int mcpt_sequence_antilag_info(mcpt_sequence* seq, int32_t* ran, int32_t* a, int32_t* b, double* trace_seconds,
                               double* kernel_seconds, double* lambda_mean, double* lambda_max);
/* the last frame's Lambda (hs*ws doubles at the stratum it ran with) and, only when the gradient pass ran, the radiance
 * along the gradient rays (h*w*3; 0 off the selected pixels); refused while anti-lag is off (and until a frame has run
 * with it) */
enum { MCPT_SEQ_GRADIENT_LAMBDA = 11, MCPT_SEQ_GRADIENT_RAW = 12 };

/* Multi-process communicator (see mcpt_comm above): ncclGetUniqueId / ncclCommInitRank /
 * ncclCommDestroy.  device -1 = the current device. */
int mcpt_comm_unique_id(uint8_t id[MCPT_COMM_ID_BYTES]);
int mcpt_comm_init_rank(int32_t nranks, int32_t rank, const uint8_t id[MCPT_COMM_ID_BYTES], int32_t device,
                        mcpt_comm** out);
void mcpt_comm_destroy(mcpt_comm* comm);

#ifdef __cplusplus
}
#endif
#endif
