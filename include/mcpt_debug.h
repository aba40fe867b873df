/* mcpt_debug.h -- diagnostics and A/B switches of libmcpt_hip.so.  NOT part of the drop-in boundary
 * (include/mcpt.h): kernel-variant timing and render switches used by tools/ for same-box A/B
 * experiments.  No reference interface corresponds to these. */
#ifndef MCPT_DEBUG_H
#define MCPT_DEBUG_H
#include "mcpt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mcpt_render_opts.flags bits for A/B experiments (the library accepts them; images are unchanged):
 * MCPT_DEBUG_SPLIT_BRDF runs BRDF-only renders as gen / rays / combine kernels instead of the fused
 * k_extend_brdf; MCPT_DEBUG_NO_ROOT_CACHE disables the per-pixel root-point light-prep cache. */
enum {
    MCPT_DEBUG_SPLIT_BRDF = 1 << 16,
    MCPT_DEBUG_NO_ROOT_CACHE = 1 << 17,
    MCPT_DEBUG_COUNT_TRAVERSAL = 1 << 18,
    MCPT_DEBUG_SHARD_RANKS = 1 << 19,
    MCPT_DEBUG_RAYS_PERSIST = 1 << 20,
    MCPT_DEBUG_RAYS_CW8 = 1 << 21,
    MCPT_DEBUG_FUSED_CULL = 1 << 22,
    MCPT_DEBUG_NO_EXACT_DEFER = 1 << 23,
    MCPT_DEBUG_NO_PICK_TABLE = 1 << 24,
    MCPT_DEBUG_REEVAL_PICK = 1 << 25
};
/* MCPT_DEBUG_REEVAL_PICK: k_prep_pk2 keeps no batch weights in LDS, so every node's pick evaluates the 64 candidates of
 * its picked batch again (the only form before the stash).  By default the weights of a node's first batches stay in the
 * idle tail of the wave's candidate-list region and a whole picked batch among them is read back; sums, picks, margins
 * and frames are the same either way (tests/test_prep_stash_pick.py). */
/* MCPT_DEBUG_NO_PICK_TABLE: cached roots search their pixel's cached row in every generation (k_prep_pick_g)
 * instead of looking their pick up in the run's root pick table (k_root_pick_table + k_pick_lookup; sums, picks,
 * exact-list membership and frames are the same either way). */
/* MCPT_DEBUG_NO_EXACT_DEFER: k_prep_exact recomputes a root's literal sums even when another wave of the same
 * launch is computing its pixel's, instead of deferring the root to the follow-up launch that only searches the
 * stored sums (the default since round 6; picks and sums are the same either way). */
/* MCPT_DEBUG_FUSED_CULL: the MIS children's light prep runs its cheap stages inside k_prep_pk2, one wave per
 * node (prep variant 8, chunks below the node's tangent plane skipped), instead of k_prep_cull_lanes' lane per
 * node writing candidate words that k_prep_pk2 reads back (variant 17). */
/* MCPT_DEBUG_RAYS_PERSIST: the MIS / shade ray sets of every scene go through the persistent refilling
 * traversal (by default only trees beyond an XCD's L2 do; smaller ones take k_mis_rays, one ray per thread).
 * MCPT_DEBUG_RAYS_CW8: the persistent traversal walks the 8-wide compressed trees (k_rays_cw8) instead of the
 * 4-wide ones (k_rays_persistent).  mcpt_closest_hit flag MCPT_DEBUG_HIT_CW8: trace the batch through the
 * 8-wide trees (one ray per thread, k_rays_cw8's traversal). */
enum { MCPT_DEBUG_HIT_CW8 = 1 << 8 };
/* MCPT_DEBUG_COUNT_TRAVERSAL runs the traversal kernel's counting instance, which fills
 * mcpt_stats.node_visits / tri_tests (the events of the traversal roofline; slower, for untimed
 * replays).
 * MCPT_DEBUG_SHARD_RANKS (device lists, mcpt_render_opts.devices): every list entry becomes its own rank
 * of the ncclCommInitAll communicator, a repeated device included (normally repeated devices are merged
 * into one rank).  Real RCCL refuses a device twice; with mcpt_debug_set_collective_lib pointing at the
 * test collective (tests/collshim) it runs the multi-rank group reduce on a one-GPU box. */

/* Test infrastructure: load the NCCL-API collective library at `path` instead of librccl.so.1.  Must
 * be called before the first communicator of the process (mcpt_comm_unique_id / _init_rank or a device
 * list render), else MCPT_E_INVALID.  tests/collshim/libmcpt_collshim.so implements the entry points the
 * library binds (ncclGetUniqueId, ncclCommInitRank, ncclCommInitAll, ncclReduce, ncclGroupStart/End,
 * ncclCommDestroy, ncclCommAbort, ncclGetErrorString) over host shared memory, so 2-8 processes can
 * share one GPU -- the multi-rank protocol of mcpt_render_opts.comm then runs in CI as it does over
 * xGMI.  Not part of the drop-in boundary. */
int mcpt_debug_set_collective_lib(const char* path);

/* diagnostics: run the light-prep kernel variant `variant` `iters` times on the n points and report
 * the mean device time per launch; outputs like those of mcpt_light_prep, pick = facet.  Variants: -1 auto
 * (9 if N_L <= 64, else 17, else 0 when the candidate list does not fit in LDS); 0 k_prep (per-wave
 * LDS candidate queue, any N_L); 8 k_prep_pk2 (packed-fp32 cheap stages, stored LDS candidate list,
 * branch-free fp64 batches, lane-parallel batch search in one kernel); 9 k_prep_lane (lane per
 * node, small light sets); 17 k_prep_cull_lanes (lane per node, light table in scalar registers)
 * + k_prep_pk2's fp64 phase (the renderer's form: the cull's lanes take the nodes bucketed by their
 * tangent-plane chunk classes and skip the work a class decides, k_cull_classify); 18 variant 17 without
 * that order and without the chunk classes (its candidate words must be identical); 19 variant 17 with
 * MCPT_DEBUG_REEVAL_PICK (every pick re-evaluates its batch; sums and picks must be identical).  Other values:
 * MCPT_E_DEVICE (invalid value). */
int mcpt_debug_prep_bench(mcpt_scene* scene, int32_t n, const double* x1, const double* normal, const double* u,
                          int32_t variant, int32_t iters, double* ms_per_launch, double* weights_sum, int32_t* pick);
/* diagnostics: how the n nodes of the last mcpt_debug_prep_bench call (process-wide; its untimed first launch) got
 * their picks in k_prep_pk2: *from_stash nodes read the picked batch's weights back from LDS, *reevaluated nodes
 * evaluated the batch again (a batch beyond the stashed ones, a partial last batch, or variant 19).  Nodes without a
 * pick (weights_sum below 1e-8) count in neither; variants that do not run k_prep_pk2 report 0, 0. */
int mcpt_debug_prep_pick_counts(int64_t* from_stash, int64_t* reevaluated);

/* diagnostics: mcpt_light_prep with every point through the exact fallback alone (k_prep_exact: the
 * reference's literal cull chain and weights, Mylight.cpp:335-413, summed in index order, and the
 * counter-RNG pick over those sums) -- the arithmetic the renderer uses for picks inside the
 * ambiguity band.  Scenes with more than 64 light triangles (else MCPT_E_INVALID). */
int mcpt_debug_light_prep_exact(mcpt_scene* scene, int32_t n, const double* x1, const double* normal, const double* u,
                                double* weights_sum, int32_t* count, int32_t* pick);

/* diagnostics: the reference's literal cull chain (Mylight.cpp:335-413, light_tri_stage) for every light
 * at one point, 20 doubles per light: stage (0 survives, 1/2 cheap culls, 3 full-stage cull), A, B, C
 * (after the orientation swap), a, b, c, alpha, beta, gamma, alpha+beta+gamma-pi, w (-1 if culled),
 * alpha's acos argument, B.C.  For checking the GPU's fp64 sqrt / division / acos against the host's. */
int mcpt_debug_light_literal(mcpt_scene* scene, const double x1[3], const double normal[3], double* out20);

/* diagnostics (host only, no GPU): the traversal's fp32 triangle pre-test (tri_filter in render.hip)
 * on n (triangle, ray) pairs -- tri: 9 floats per triangle (a, b, c), ro / rd: 3 doubles per ray,
 * tlim: the traversal's current limit per pair (FLT_MAX: none).  verdict: 0 the reference's fp64 test
 * (Myobj.cpp:165-192) surely rejects, or the hit lies surely beyond tlim; 2 it surely accepts, with
 * tup >= its t; 1 undecided.  Lets a CPU test check the bound's soundness against the fp64 test. */
int mcpt_debug_tri_filter(int32_t n, const float* tri, const double* ro, const double* rd, const float* tlim,
                          int32_t* verdict, float* tup);

/* diagnostics (host only): checks the 8-wide compressed tree of the scene (light_only: the light-only tree)
 * against its binary tree.  out[6] = nodes reached, triangles reached, facets of the binary tree,
 * facets reached more than once, errors (bad indices, or a triangle vertex outside the decoded box of a slot
 * on its path), depth. */
int mcpt_debug_bvh8_check(mcpt_scene* scene, int32_t light_only, int64_t out[6]);
// The 4-wide tree of every traversal kernel (collapse_bvh4) and its quantized form (quantize_bvh4), walked on
// the host: out = {nodes, facets reached, facets in the binary tree, facets reached twice, errors (a vertex
// outside an ancestor slot's box, a quantized slot box not containing its fp32 box, a bad index), depth}.
int mcpt_debug_bvh4_check(mcpt_scene* scene, int32_t light_only, int64_t out[6]);
// The same walk over what `device` (-1 = current) holds of the scene's main tree: its 4-wide nodes (leaf codes
// unpacked), quantized nodes and leaf slots are downloaded and walked against the host positions; vertices of a leaf
// slot or of the device's facet array that differ from the host positions count as errors too.  The check of the
// device-side refit (mcpt_scene_update, include/mcpt.h).  A hidden facet (mcpt_scene_set_visible) is walked, here and
// in mcpt_debug_bvh4_check, as the collapsed triangle its leaf slots hold -- its first vertex three times: a hidden
// facet's slot that holds a real triangle and a visible facet's slot that is collapsed both count as errors, while the
// device's facet array is compared with the stored values.  Unchanged when nothing is hidden.
int mcpt_debug_bvh4_check_device(mcpt_scene* scene, int32_t device, int64_t out[6]);
// Downloads that tree: counts = {nodes, leaf slots}; nodes (128 B each), qnodes (64 B each) and leaf_facets (the
// facet of every slot) may each be NULL, else they hold at least cap_nodes / cap_slots entries (a smaller capacity
// than the tree has is MCPT_E_INVALID).  Lets a test compare the nodes before and after an update.
int mcpt_debug_bvh4_download(mcpt_scene* scene, int32_t device, int64_t counts[2], void* nodes, void* qnodes,
                             int32_t* leaf_facets, int64_t cap_nodes, int64_t cap_slots);
// The trees mcpt_debug_bvh4_check walks, handed out: the host's 4-wide tree (collapse_bvh4 of the binary tree, or of
// the light-only one) and its quantised form (quantize_bvh4), in mcpt_debug_bvh4_download's layout and with its
// capacity rules.  Needs no device.  Lets a CPU test model the traversals' box tests on the very boxes a device gets.
int mcpt_debug_bvh4_host(mcpt_scene* scene, int32_t light_only, int64_t counts[2], void* nodes, void* qnodes,
                         int32_t* leaf_facets, int64_t cap_nodes, int64_t cap_slots);
// mcpt_debug_bvh4_check_device's walk over the LIGHT-ONLY tree `device` holds (its nodes, quantized nodes and leaf
// slots against the host positions; a leaf slot's vertices that differ from the host's count as errors).  The check of
// the light tree's device-side refit (mcpt_scene_set_lights_movable, include/mcpt.h).
int mcpt_debug_bvh4_check_device_light(mcpt_scene* scene, int32_t device, int64_t out[6]);
// Downloads one light table of the state `device` (-1 = current) holds, as raw bytes: which = "lt_v", "lt_n", "lt_pk",
// "lt_d", "lt_w", "lt_f", "lt_pair", "chunk_sph", "chunk_sk", "l_area", "l_area_cum" (each in the size the state
// allocated, padding and sentinel records included), the tables a re-light writes beside those (mcpt_scene_set_light_radiance,
// mcpt_scene_set_materials): "light_rad", "light_sum", "grp_sum", "grp_cum", "mtl", or "globals" (light_bound and the band constants the state passes
// to its kernels by value: 6 doubles band_ctr[3], band_R, band_S, band_K, then the float light_bound and 4 zero
// bytes).  *bytes = the table's size; out may be NULL (size query), else cap >= *bytes or MCPT_E_INVALID.  Creates the
// device state if needed.  Lets a test compare an updated state against a fresh one byte for byte.
int mcpt_debug_light_tables(mcpt_scene* scene, int32_t device, const char* which, void* out, int64_t cap, int64_t* bytes);
// k_light_area_cum alone over every group of the state `device` holds, `reps` times between two HIP events (the
// running sums are rewritten with the same values); *seconds = the time of one run.  tools/light_update_bench.py.
int mcpt_debug_light_area_cum_bench(mcpt_scene* scene, int32_t device, int32_t reps, double* seconds);
/* After a scene's first mcpt_scene_update the 8-wide trees are stale: MCPT_DEBUG_RAYS_CW8, MCPT_DEBUG_HIT_CW8 and
 * mcpt_debug_bvh8_check are refused for that handle (MCPT_E_INVALID). */

/* diagnostics: the last active-pixel list the scene's most recent adaptive render built on `device` (-1 = current)
 * -- the pixels sampled by its last pass, or the list built after pass 0 when max_spp = min_spp + pass_spp.
 * *n = its length (0: no list was built); up to `cap` pixel indices are copied to `pixels`. */
int mcpt_debug_adaptive_active(mcpt_scene* scene, int32_t device, int32_t* pixels, int32_t cap, int32_t* n);

/* The root pick table's rules, process-wide (0: the library's default): min_samples, the fewest samples per pixel
 * of a run at which the table is built; window_samples, a cap on the samples one table covers (rounded down to whole
 * root groups), so that a small run rolls over several windows.  For tests and the min_samples A/B. */
int mcpt_debug_set_pick_table(int32_t min_samples, int32_t window_samples);

/* mcpt_scene_rebuild's leaf size, process-wide: the most facets of a leaf child, 1..4 (0: the library's default, 2).
 * For the leaf-size measurement of tools/rebuild_bench.py; every value gives a valid tree.  MCPT_E_INVALID otherwise. */
int mcpt_debug_set_rebuild_leaf_max(int32_t leaf_max);

/* diagnostics: the light pick of every root of a render call with these options (scene, camera, seed, mode, sample
 * range, flags), without tracing anything: pick, weights_sum and ambiguous are [width * height][samples] arrays.  The
 * picks come from the path the render's run would take -- the root pick table and its lookup, or with
 * MCPT_DEBUG_NO_PICK_TABLE (or below min_samples) the pick kernel over the cached rows, driven by the run's root
 * queue.  pick: the light index, -1 without one; ambiguous: 1 for a root the exact pick redoes.  A sample that
 * terminates at entry (Russian roulette) and every sample of a pixel without a cached root carry the sentinel
 * pick -2, weights_sum 0, ambiguous 0.  MCPT_E_INVALID when the call has no root-point cache. */
int mcpt_debug_root_picks(mcpt_scene* scene, const mcpt_camera* cam, const mcpt_render_opts* opts, int32_t* pick,
                          double* weights_sum, int32_t* ambiguous);

/* diagnostics: the Phong functions of csrc/device_math.h on n caller-chosen records, one thread per record, with the
 * template arguments the render kernels use.  A record is 19 doubles in -- n[3] wi[3] wr[3] kd[3] ks[3] sh u0 k1 k2
 * -- and 8 doubles out -- brdf[3] pdf dir[3] sample_pdf: brdf_phong(n, wi, wr, kd, ks, sh), phong_pdf of the same
 * arguments, and sample_phong(n, wr, kd, ks, sh, u0, k1, k2) with its pdf.  variant 0: the MIS / shade() kernels'
 * forms (brdf_phong<true, false>, sample_phong<false>); variant 1: the BRDF-only kernels' (brdf_phong<false, true>,
 * sample_phong<true>); phong_pdf is the same function in both.  Needs no scene; runs on the current device (a
 * host-to-device copy, one launch, a device-to-host copy, a synchronize).  n == 0 does nothing; n < 0, another
 * variant or a NULL array is MCPT_E_INVALID.  tests/test_phong.py compares the outputs with the oracle's and with a
 * high-precision evaluation. */
int mcpt_debug_phong(int32_t n, int32_t variant, const double* in19, double* out8);

/* diagnostics: the bytes of device memory the library's self-owning buffers hold at this moment, process-wide and over
 * all devices -- every scene's uploaded arrays and work buffers, counted where a buffer is allocated and where it is
 * freed.  0 in a process that never made a device state; back to its earlier value once the scenes made since are
 * destroyed (tests/test_device_memory.py).  Needs no device. */
int64_t mcpt_debug_device_bytes_live(void);

#ifdef __cplusplus
}
#endif
#endif
