// Host-side scene representation shared by the loaders, the BVH builder and the HIP renderer.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "mcpt.h"

namespace mcpt {

// Flattened scene: facets in the reference's (shape, face) order, the light table in
// Mylight::lightsTriangles order (Mylight.cpp:88: material name, then facet).
struct HostScene {
    int F = 0, M = 0, NL = 0;
    std::vector<float> pos;         // F*9  v0 v1 v2
    std::vector<float> nrm;         // F*9  vertex normals
    std::vector<int32_t> mat;       // F
    std::vector<float> mtl;         // M*7  Kd Ks Ns
    std::vector<std::string> mtl_names;
    std::vector<int32_t> light_facet;   // NL
    std::vector<double> light_rad;      // NL*3
    std::vector<double> light_sum;      // NL  RadianceRGB::sum()
    std::vector<int32_t> light_of;      // F -> light index or -1
    std::vector<double> unique_n;       // F*3  Myobj::get_unique_normal_of_facet
    std::vector<double> light_area;     // NL   lightTriangle::area (Mylight.cpp:66-69)
    // Mylight::lightsRadiance in map order (every XML light, also one without triangles):
    // RadianceRGB::sum() and the run [start, start + count) of its triangles in the light table
    std::vector<double> group_rsum;
    std::vector<int32_t> group_start, group_count;
    bool has_cam = false;
    mcpt_camera cam{};
    // mcpt_scene_set_visible: F bytes, 1 = hidden; empty until the handle's first call
    std::vector<uint8_t> hidden;
    bool is_hidden(int f) const { return !hidden.empty() && hidden[static_cast<size_t>(f)] != 0; }
};

// scene_io.cpp
bool load_obj_mtl(const std::string& obj_path, HostScene& s, std::string& err);
struct LightDef {
    std::string name;
    double rgb[3];
};
bool load_light_xml(const std::string& xml_path, HostScene& s, std::vector<LightDef>& lights, std::string& err);
// gather_light_triangles + unique normals (Mylight.cpp:32-100, Myobj.cpp:680-709)
bool finalize_scene(HostScene& s, std::vector<LightDef> lights, std::string& err);
double light_triangle_area(const HostScene& s, int f);  // Mylight.cpp:66-69

// bvh.cpp -- binary BVH over a facet subset, flattened for the GPU.
struct BvhNode {       // 64 B: both children's boxes in one node (one fetch per visit)
    float lo[2][3];    // child 0/1 AABB min
    float hi[2][3];    // child 0/1 AABB max
    int32_t child[2];  // >= 0: inner node index; < 0: leaf, ~child = first leaf slot
    int32_t count[2];  // leaf triangle count (0 for inner children)
};
struct Bvh {
    std::vector<BvhNode> nodes;
    std::vector<int32_t> leaf_facets;  // facet ids in leaf order
};
Bvh build_bvh(const HostScene& s, const std::vector<int32_t>& facets, int max_leaf);

// The margin every box of a tree over facets inside [lo, hi] is enlarged by: 1e-5 of the largest
// axis extent `ext` + 1e-6, plus kBoxMarginUlps * 2^-24 * C for the traversals' fp32 slab arithmetic, whose absolute
// error grows with the size of the coordinates and not with the scene's extent.  C bounds |coordinate| over the arena
// of mcpt_scene_update ([lo - ext, hi + ext]), so the one value holds for every position an update, a transform, a
// refit or a rebuild can put into the tree.  The only place the formula lives: both host builders, the scene's refit
// margin (host and k_refit_level) and the rebuild use it.
constexpr double kBoxMarginUlps = 3.0;
double box_margin(const double lo[3], const double hi[3]);

// 4-wide node (128 B, two cache lines): the four children's boxes as per-axis float4s, so a
// node visit is 8 dwordx4 loads and four independent slab tests.  Children as in BvhNode;
// unused slots hold kBvh4Empty.
constexpr int32_t kBvh4Empty = 0x7fffffff;
struct BvhNode4 {
    float lo[3][4];    // lo[axis][child]
    float hi[3][4];
    int32_t child[4];  // >= 0: inner node; < 0: leaf ~first slot; kBvh4Empty: no child
    int32_t count[4];
};
// compressed 4-wide node (64 B, half a cache line): per axis the children's union minimum `org` and
// a power-of-two scale 2^(ex_a - 127); each child plane is a byte q with plane = fma(q, scale, org)
// in fp32, rounded outward at build time against that exact fp32 expression, so every decoded box
// contains its BvhNode4 box (conservative: the traversal only prunes with it).  Loaded as four
// dwordx4: (org, ex), (q lo.x, hi.x, lo.y, hi.y), (q lo.z, hi.z, -, -), children.
struct BvhNode4Q {
    float org[3];
    uint32_t ex;       // byte a: biased fp32 exponent of axis a's scale
    uint32_t q[6];     // q[2a] lo planes, q[2a + 1] hi planes of axis a; byte k = child k
    uint32_t pad[2];
    int32_t child[4];  // as BvhNode4 (leaf codes already packed)
};
static_assert(sizeof(BvhNode4Q) == 64, "BvhNode4Q must be 64 B");
std::vector<BvhNode4Q> quantize_bvh4(const std::vector<BvhNode4>& in);

// collapses a binary BVH into a 4-wide one (greedy: expand the largest-area inner child until
// four children); leaves and leaf slots are shared with the binary tree
std::vector<BvhNode4> collapse_bvh4(const Bvh& b);

// 8-wide compressed node (128 B, one cache line) for the wide traversal (k_rays_cw8), after Ylitie, Karras &
// Laine's compressed wide BVH (HPG 2017), adapted: the same conservative byte planes as BvhNode4Q for eight
// children, children ordered by OCTANT -- slot s holds the child whose centre lies on the negative side of
// the node centre along axis a iff bit a of s is set (greedy assignment) -- so that a ray visits hit
// children in (slot XOR its octant code) order, near to far, with no sort; inner child s at node base + s
// (eight node slots reserved per node with inner children: a stack entry is (base << 8 | hit bits), no
// child code needs loading) and each leaf child's <= 2 triangles at fixed triangle slots (a triangle
// group is a base and a 16-bit mask).  Binary leaves with more than two triangles are split (by index
// halves) before the collapse.
struct BvhNode8Q {
    float org[3];
    uint32_t ex;           // bytes 0-2: biased fp32 exponent of axis a's scale; byte 3: imask (slots of inner children)
    uint32_t qlo[3][2];    // qlo[a][h]: byte k = lo plane of child 4 h + k on axis a (plane = fma(q, 2^(e - 127), org))
    uint32_t qhi[3][2];
    int32_t base_inner;    // inner child of slot s: node base_inner + s
    int32_t base_tri;      // triangle j (0, 1) of leaf child s: triangle slot base_tri + 2 s + j
    uint32_t tvalid;       // bit 2 s + j: that triangle slot holds a triangle
    uint32_t pad[13];
};
static_assert(sizeof(BvhNode8Q) == 128, "BvhNode8Q must be 128 B");
struct Bvh8 {
    std::vector<BvhNode8Q> nodes;      // node 0 = root
    std::vector<int32_t> tri_facets;   // facet of each triangle slot (-1: unused)
    int depth = 0;                     // levels of nodes (the 8-wide traversal stack holds at most one entry per level)
};
// the 8-wide tree of a binary BVH built by build_bvh over the same facets (boxes conservative: every decoded
// child box contains the fp32 box the binary tree holds for it, or its triangles' for a split leaf)
Bvh8 build_bvh8(const HostScene& s, const Bvh& b);

// leaf children of the device's 4-wide nodes are packed as ~((first leaf slot << kBvh4LeafBits) | count)
constexpr int kBvh4LeafBits = 5;

// bvh.cpp -- refit of a binary BVH after mcpt_scene_update moved facets: topology and leaf slots stay, only boxes
// change.  The index is built once per tree (at its first update).
struct BvhRefitIndex {
    std::vector<int32_t> parent;      // node -> 2 * parent node + slot (-1: the root)
    std::vector<int32_t> slot_owner;  // leaf slot -> 2 * node + slot of the leaf that holds it
};
BvhRefitIndex make_bvh_refit_index(const Bvh& b);
// Builder::to_float_box's arithmetic: the margin applied in double, rounded to float, then one ulp outward
void box_with_margin(const double lo[3], const double hi[3], double margin, float* flo, float* fhi);
// every leaf holding one of `slots` gets the union of the FULL bounds of all its triangles (from s.pos), enlarged by
// `margin`; every ancestor slot the union of its child node's two slot boxes.  Boxes off those paths are untouched.
// A hidden facet (s.hidden, mcpt_scene_set_visible) counts as its first vertex alone.
void refit_bvh(Bvh& b, const BvhRefitIndex& ix, const HostScene& s, const std::vector<int32_t>& slots, double margin);

// scene_io.cpp -- Myobj::get_unique_normal_of_facet (Myobj.cpp:680-709) of facet f into s.unique_n
void unique_normal_of_facet(HostScene& s, int f);

// host_mirror.cpp -- the host side of mcpt_scene_transform (no HIP in it: the sanitizer driver runs it)
// mcpt_scene_transform's rule (include/mcpt.h) for `count` facets: rest arrays -> pos / nrm (count * 9 floats each)
void transform_facets(const float* rest_pos, const float* rest_nrm, size_t count, const double m[12], const double n[9],
                      float* pos, float* nrm);
// the facet ranges whose host copy is behind the devices: sorted, disjoint, non-touching [first, end) pairs; beyond
// kPendingMax entries the list collapses to its hull
constexpr size_t kPendingMax = 48;
struct PendingRanges {
    std::vector<std::pair<int32_t, int32_t>> r;
    void add(int32_t first, int32_t count);
    int64_t facets() const;
};
// the CSR facet -> leaf-slot map of a tree over facets [0, F)
void make_facet_slot_map(const Bvh& b, int F, std::vector<int32_t>& slot_start, std::vector<int32_t>& slot_list);
// the host half of an update once s.pos / s.nrm of the ranges are current: their unique normals, then one refit_bvh
// over their slots; returns the number of slots
int64_t host_refresh_ranges(HostScene& s, Bvh& b, const BvhRefitIndex& ix, const std::vector<int32_t>& slot_start,
                            const std::vector<int32_t>& slot_list, const PendingRanges& ranges, double margin);

// the same for the light triangles of the ranges (a light move): their light_area, then one refit_bvh
// of the light-only tree `lb` over their slots (slot map and index of `lb`); returns the number of light triangles
int64_t host_refresh_lights(HostScene& s, Bvh& lb, const BvhRefitIndex& ix, const std::vector<int32_t>& slot_start,
                            const std::vector<int32_t>& slot_list, const PendingRanges& ranges, double margin);
// the first light triangle of pos (count facets from `first`, 9 floats each) whose fp64 (b - a) x (c - a) has a zero
// or non-finite length, or -1
int first_degenerate_light(const HostScene& s, int32_t first, int32_t count, const float* pos);

// refit.hip -- the device side of mcpt_scene_update: the device pointers of one device state's main tree (owned by
// scene_state.h's DeviceState) and the kernels that rewrite them.  Both functions only enqueue on `stream` (a
// hipStream_t) of the current device.
struct RefitDev {
    float* tri_v;               // F * 3 float4
    float* tri_n;               // F * 9
    float* leaf_v;              // nslots * 3 float4 (w of the first = facet id bits)
    BvhNode4* bvh4;             // breadth-first, leaf codes packed
    BvhNode4Q* bvh4q;
    const int32_t* slot_start;  // F + 1: CSR facet -> leaf slots
    const int32_t* slot_list;
    uint8_t* slot_dirty;        // nslots
    uint8_t* node_dirty;        // nnodes
    unsigned* counters;         // [0] offending values (refit_validate_enqueue), [1] nodes refit
    int32_t F, nslots, nnodes;
    uint8_t* hidden;            // F bytes, 1 = hidden (mcpt_scene_set_visible); null until the state's first mask
};
// counts into r.counters[0] the non-finite values of dpos / dnrm (count * 9 floats each, dnrm may be null) and the
// positions outside [lo, hi]
int refit_validate_enqueue(const RefitDev& r, int32_t count, const float* dpos, const float* dnrm, const double lo[3],
                           const double hi[3], void* stream);
// scatter of facets [first, first + count), one refit launch per level (level l = nodes [level_first[l],
// level_first[l + 1]), deepest first), then the dirty bytes cleared
int refit_enqueue(const RefitDev& r, const int32_t* level_first, int nlevels, int32_t first, int32_t count, const float* dpos,
                  const float* dnrm, double margin, void* stream);
// mcpt_scene_transform on one device state: clears r.counters[0], then k_transform_range writes the rule's image of
// facets [first, first + count) of the rest pose (rest_v: F * 3 float4, rest_n: F * 9) into out_pos / out_nrm
// (count * 9 floats each) and counts the offending values (refit_validate_enqueue's terms) into r.counters[0];
// nothing of the scene is modified
int transform_enqueue(const RefitDev& r, const float* rest_v, const float* rest_n, int32_t first, int32_t count,
                      const double m[12], const double n[9], const double lo[3], const double hi[3], float* out_pos,
                      float* out_nrm, void* stream);

// k_refit_level alone over every level, deepest first, on the dirty bytes the state holds (r.counters[1] cleared
// first, the dirty bytes after): the tail of refit_enqueue, and how a rebuilt tree gets its boxes
int refit_levels_enqueue(const RefitDev& r, const int32_t* level_first, int nlevels, double margin, void* stream);

// mcpt_scene_set_visible on one device state (r.hidden must be set): k_visibility_scatter gives facets
// [first, first + count) their mask byte and, from tri_v, every leaf slot its collapsed (v0, v0, v0) or full form with
// the dirty byte; then refit_levels_enqueue
int visibility_enqueue(const RefitDev& r, const int32_t* level_first, int nlevels, int32_t first, int32_t count, int32_t visible,
                       double margin, void* stream);

// light_tables.hip -- the device side of a light move (mcpt_scene_set_lights_movable): the device
// pointers of one device state's light tables (owned by scene_state.h's DeviceState; the layouts are get_device_state's)
// and the kernels that derive them again from tri_v / tri_n.  Every function only enqueues on `stream`.
constexpr int kLightRowWords = 8;  // a chunk's scratch row: unrounded S, K, lo[3], hi[3]
struct LightGlobals {              // the light constants DScene holds by value
    double band_ctr[3], band_R, band_S, band_K;
    float light_bound, pad;
};
struct LightTabDev {
    const float* tri_v;          // F * 3 float4
    const float* tri_n;          // F * 9
    const int32_t* tri_light;    // F -> light or -1
    double* light_rad;           // NL * 3 (written by a re-light only)
    double* light_sum;           // NL
    const int32_t* light_group;  // NL -> group
    const int32_t* grp_range;    // ngroups * (first light, count)
    float* lt_v;                 // NL * 3 float4
    double* lt_n;                // NL double4
    float* lt_pk;                // NL * 3 float4
    float* lt_d;                 // NL
    double* lt_w;                // NL * 5 double2
    float* lt_f;                 // NL * 4 float4
    float* lt_pair;              // 32 floats per light pair
    double* l_area;              // NL
    double* l_area_cum;          // NL
    double* grp_sum;             // ngroups (a re-light)
    double* grp_cum;             // ngroups (a re-light)
    float* chunk_sph;            // nchunks float4
    float* chunk_sk;             // nchunks float2
    double* chunk_row;           // nchunks * kLightRowWords
    uint8_t* chunk_dirty;        // nchunks
    uint8_t* group_dirty;        // ngroups
    LightGlobals* globals;
    unsigned* counters;          // the tables' own 16 words: [2] chunks recomputed, [3] groups recomputed
    int32_t F, NL, nchunks, ngroups;
};
// adds to *bad the light triangles of the staged range (dpos: count * 9 floats; tri_light_of_range: count entries)
// whose (b - a) x (c - a) has a zero or non-finite fp64 length; *bad is not cleared
int light_validate_enqueue(int32_t count, const float* dpos, const int32_t* tri_light_of_range, unsigned* bad, void* stream);
// every chunk's sphere, (S, K) and scratch row from the tables as they are (a state's first light move)
int light_chunks_all_enqueue(const LightTabDev& t, void* stream);
// the records of the light facets of [first, first + count) from tri_v / tri_n (already scattered), their chunks, the
// constants, the dirty groups' area sums, then the light-only tree `lr`: its leaf slots of those facets and
// refit_levels_enqueue with `margin`
int light_tables_enqueue(const LightTabDev& t, const RefitDev& lr, const int32_t* level_first, int nlevels, int32_t first,
                         int32_t count, double margin, void* stream);
// k_light_area_cum alone over the groups whose dirty byte is set (tools/light_update_bench.py times it)
int light_area_cum_enqueue(const LightTabDev& t, void* stream);
// a re-light (mcpt_scene_set_light_radiance).  light_radiance_validate_enqueue adds to *bad the values
// of drgb (n doubles) that are negative or not finite; *bad is not cleared.  light_radiance_enqueue gives lights
// [first, first + count) the radiances drgb (count * 3 doubles of device memory): their rows of light_rad / light_sum,
// the radiance words of lt_n / lt_w / lt_f and the grp_sum of every group whose first light is in the range, then the
// dirty chunks' (S, K) and rows, the constants, grp_cum when `groups` (a group's first light is in the range), and
// the dirty bytes cleared.  No geometry field and no tree is touched.
int light_radiance_validate_enqueue(int64_t n, const double* drgb, unsigned* bad, void* stream);
int light_radiance_enqueue(const LightTabDev& t, int32_t first, int32_t count, const double* drgb, bool groups, void* stream);

// rebuild.hip -- the device side of mcpt_scene_rebuild and mcpt_scene_tree_cost
constexpr int kRebuildMaxLevels = 15;  // node levels of a rebuilt tree, for every input
constexpr int kRebuildLeafMax = 2;     // facets per leaf child (chosen by measurement, §4.22)
// the builder's scratch for a state of F facets (Morton codes, the sorted order, per-node ranges, rocPRIM's temporary
// storage): allocated on the current device at a state's first rebuild, reused by every later one
struct RebuildWork;
int rebuild_work_create(int32_t F, RebuildWork** out);
void rebuild_work_destroy(RebuildWork* w);
// builds a tree over out->tri_v's F facets into out's OTHER arrays (bvh4, bvh4q: F nodes; leaf_v, slot_list,
// slot_dirty: F slots; slot_start: F + 1; node_dirty: F; counters) on `stream`, boxes by refit_levels_enqueue, and
// waits for the topology (not for the boxes).  Sets out->nnodes, the first node of every level and the tree's
// bvh4_stack_need (computed top-down on the device); MCPT_E_SCENE if the tree fails its checks or needs more than
// stack_cap entries -- nothing but `out`'s arrays and the scratch has been written then
int rebuild_build(RebuildWork* w, RefitDev* out, int leaf_max, int stack_cap, double margin, void* stream,
                  std::vector<int32_t>* level_first, int32_t* stack_need);
// the SAH cost of mcpt_scene_tree_cost of a device's 4-wide nodes: per-block partials, then index order.  words:
// kTreeCostWords doubles of device scratch; *result points at the cost inside them once `stream` has run
constexpr size_t kTreeCostWords = 1025;
int tree_cost_enqueue(const BvhNode4* nodes, int32_t nnodes, double* words, void* stream, double** result);

// grid.cpp -- the reference's uniform grid (Myobj.cpp:78-162) for the MCPT_ACCEL_GRID mode
struct Grid {
    bool ok = false;
    double eye[3] = {0, 0, 0};  // camera point the bounding box was built with
    int n0 = 0;
    double mn[3], mx[3];        // bounding box of every vertex and the eye
    double d = 0, inv_d = 0;    // cell edge and its reciprocal
    int lim[3], gd[3];          // last cell index per axis; cells per axis (lim + 1)
    std::vector<int32_t> cell_start;  // CSR over cells (x-major, then y, then z)
    std::vector<int32_t> cell_tri;    // facets per cell, ascending facet id
};
Grid build_grid(const HostScene& s, const double eye[3], int n0);

void set_error(const char* fmt, ...);

// temporal.hip / denoise.hip -- the accumulation and the filter for a caller that owns every buffer, scratch
// included (the frame sequence, sequence.hip).  Not exported.  Both make every check of their public device forms
// that needs no device, then only enqueue their kernels on the null stream of the CURRENT device: no allocation,
// no pointer query, no event and no synchronisation.  The public functions run the same kernels on the same
// arguments, so the results are theirs bit for bit.
struct TemporalClampIo {  // the clamped rule's extra arguments
    const mcpt_temporal_clamp_opts* clamp;
    const double* prev_fast;  // part of the previous state
    double* out_fast;
    double* out_shift;  // required here: the kernels pass "has a history" through it (the public form's scratch)
};
struct TemporalAntilagIo {  // the anti-lag rule's extra arguments
    const mcpt_gradient_opts* gradient;
    const double* lambda;  // hs * ws at gradient->stratum
};
int temporal_check_opts(const mcpt_temporal_opts* o, const mcpt_temporal_clamp_opts* clamp, bool clamped);
// io == nullptr: mcpt_temporal_accumulate's rule, else mcpt_temporal_accumulate_clamped's; motion != nullptr: either
// in mcpt_temporal_accumulate_motion's form (both arrays required); antilag != nullptr: any of them in
// mcpt_temporal_accumulate_antilag's form
int temporal_enqueue(const mcpt_temporal_opts* o, const mcpt_camera* prev_cam, int32_t W, int32_t H, const double* dC,
                     const mcpt_aov_buffers* g, const mcpt_aov_buffers* pg, const double* dpC, const double* dpM, double* dOut,
                     double* dOutM, double* dOutV, const TemporalClampIo* io, const mcpt_motion_buffers* motion = nullptr,
                     const TemporalAntilagIo* antilag = nullptr);

// temporal_gradient.hip -- the temporal gradient in the same form.  gradient_check_opts: mcpt_gradient_opts' checks.
// temporal_gradient_enqueue: every check of mcpt_temporal_gradient_device that needs no device, then its kernel on the
// null stream.  lambda_stats_enqueue: the mean and the maximum of n values of Lambda -- per-block partials in a fixed
// lane and wave order, then one pass over the partials in index order -- into words[0] (mean) and words[1] (max);
// words: lambda_stats_words() doubles of device scratch, enough for every n (the number of partials is bounded, and
// not monotone in n).
int gradient_check_opts(const mcpt_gradient_opts* o);
int temporal_gradient_enqueue(const mcpt_gradient_opts* o, int32_t W, int32_t H, int32_t a, int32_t b, const double* dPrev,
                              const double* dRegrad, double* dLambda);
size_t lambda_stats_words();
int lambda_stats_enqueue(const double* dLambda, size_t n, double* words);
int denoise_check_opts(const mcpt_denoise_opts* o);
// tmp: 8 * W * H doubles of scratch (two colour + variance buffers)
int denoise_enqueue(const mcpt_denoise_opts* o, int32_t W, int32_t H, const double* dC, const double* dV,
                    const mcpt_aov_buffers* g, double* dOut, double* dOutV, double* tmp);

// upsample.hip -- the guided upsampling in the same form: every check of mcpt_upsample_device that needs no device,
// then the count's memset and the kernel on the null stream.  dCount: one 64-bit word of device memory.
int upsample_check_opts(const mcpt_upsample_opts* o);
int upsample_enqueue(const mcpt_upsample_opts* o, int32_t w, int32_t h, const double* dC, const mcpt_aov_buffers* g,
                     const mcpt_aov_buffers* G, double* dOut, unsigned long long* dCount);

// temporal.hip -- k_temporal_spatial alone, for temporal_upsample.hip: V_0 of dOutC with the guides g and o's sigmas
// into dOutV wherever the moments dOutM fail the temporal variance's condition; no check, the null stream
int temporal_spatial_enqueue(const mcpt_temporal_opts* o, int32_t W, int32_t H, const mcpt_aov_buffers* g, const double* dOutC,
                             const double* dOutM, double* dOutV);

// temporal_upsample.hip -- the temporal upsampling in the same form: every check of mcpt_temporal_upsample_device that
// needs no device, then the counts' memset and the kernels on the null stream.  dCounts: two 64-bit words of device
// memory (filled, fallback).
int temporal_upsample_enqueue(const mcpt_temporal_opts* tp, const mcpt_upsample_opts* up, int32_t a, int32_t b,
                              const mcpt_camera* prev_full_cam, int32_t w, int32_t h, const double* dC, const mcpt_aov_buffers* G,
                              const mcpt_aov_buffers* pG, const double* dpC, const double* dpM, double* dOut, double* dOutM,
                              double* dOutV, unsigned long long* dCounts);

// render.hip -- mcpt_camera_phase_rays_device's checks that need no device, then its kernel on the null stream of the
// current device
int camera_phase_rays_enqueue(const mcpt_camera* full_cam, int32_t factor, int32_t a, int32_t b, double* dOrigin, double* dDir);
// the same for mcpt_gradient_rays_device
int gradient_rays_enqueue(const mcpt_camera* cam, int32_t stratum, int32_t a, int32_t b, double* dOrigin, double* dDir);
// the same for mcpt_gradient_rays_indexed_device; *count gets the number of entries, and with 0 entries
// nothing is launched
int gradient_rays_indexed_enqueue(const mcpt_camera* cam, int32_t stratum, int32_t a, int32_t b, int32_t* dIndex, double* dOrigin,
                                  double* dDir, int32_t* count);

// render.hip -- k_motion_aovs alone, on the primary-hit tables the scene's state on `device` holds from its last
// mcpt_render_aovs[_device] call, which must have been for a W x H camera (the frame sequence calls it right after the
// frame's AOVs, so no second primary trace is made).  Takes the scene's lock, launches on the state's stream and waits
// for it.  dev_out: device pointers on `device`, either may be null; no pointer query.
int motion_aovs_enqueue(mcpt_scene* scene, int32_t device, int32_t W, int32_t H, const mcpt_motion_buffers* dev_out);

}  // namespace mcpt
