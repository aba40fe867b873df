// Host-side checks and downloads of the scene's trees and light tables (include/mcpt_debug.h): the 4-wide trees on
// the host and as a device holds them, the 8-wide trees, the light tables of a device state.  No kernel of the
// renderer is launched here.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <vector>

#include "mcpt_debug.h"
#include "scene_state.h"  // with mcpt.h, mcpt_internal.h and the HIP runtime

using namespace mcpt;

extern "C" {

// host-only check of an 8-wide tree (include/mcpt_debug.h): every facet of the binary tree is reached exactly
// once, and every reached triangle's vertices lie inside the decoded box of every slot on its path (the
// traversal prunes with those boxes, so this is what keeps its hits the binary tree's)
// references beyond the first of each facet in a binary tree's leaf list (spatial splits repeat facets)
static int64_t dup_refs(const Bvh& b) {
    std::vector<int32_t> f(b.leaf_facets);
    std::sort(f.begin(), f.end());
    return (int64_t)(f.size() - (std::unique(f.begin(), f.end()) - f.begin()));
}
// A facet may sit in several leaves (spatial splits, each reference with its triangle clipped to one side):
// then its references' regions (the intersection of the slot boxes on each one's path) must together cover
// the triangle -- checked at the vertices, edge points and interior points; a facet with one reference
// needs all three vertices inside every box on its path.
struct RefRegion {
    int32_t f;
    float lo[3], hi[3];
};
static int64_t check_coverage(const std::vector<float>& pos, std::vector<RefRegion>& refs) {
    std::sort(refs.begin(), refs.end(), [](const RefRegion& x, const RefRegion& y) { return x.f < y.f; });
    int64_t bad = 0;
    static const double kW[][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {.5, .5, 0}, {0, .5, .5}, {.5, 0, .5}, {1. / 3, 1. / 3, 1. / 3},
                                   {.8, .1, .1}, {.1, .8, .1}, {.1, .1, .8}, {.25, .75, 0}, {.75, .25, 0}, {0, .25, .75},
                                   {0, .75, .25}, {.25, 0, .75}, {.75, 0, .25}};
    for (size_t i = 0; i < refs.size();) {
        size_t j = i;
        while (j < refs.size() && refs[j].f == refs[i].f) j++;
        const float* v = &pos[9 * (size_t)refs[i].f];
        const int npts = j - i == 1 ? 3 : (int)(sizeof(kW) / sizeof(kW[0]));
        for (int w = 0; w < npts; w++) {
            float x[3];
            for (int a = 0; a < 3; a++)
                x[a] = j - i == 1 ? v[3 * w + a] : (float)(kW[w][0] * v[a] + kW[w][1] * v[3 + a] + kW[w][2] * v[6 + a]);
            bool in = false;
            for (size_t r = i; r < j && !in; r++)
                in = x[0] >= refs[r].lo[0] && x[0] <= refs[r].hi[0] && x[1] >= refs[r].lo[1] && x[1] <= refs[r].hi[1] &&
                     x[2] >= refs[r].lo[2] && x[2] <= refs[r].hi[2];
            if (!in) bad++;
        }
        i = j;
    }
    return bad;
}
// the 4-wide tree every traversal kernel reads (collapse_bvh4 of the binary tree) and its quantized form
// (quantize_bvh4), walked on the host: every facet of the binary tree reached, each reference's triangle
// covered by the slot boxes on its path (check_coverage), and every quantized slot box containing its fp32
// box (the conservative rounding the persistent traversal relies on)
// the walk itself, over any copy of a tree: nodes with unpacked leaf children (~first slot, count), their quantized
// forms, the facet of every leaf slot and the positions (9 floats per facet) the triangles are checked with
static void bvh4_walk(const std::vector<BvhNode4>& b4, const std::vector<BvhNode4Q>& q4, const std::vector<int32_t>& leaf_facets,
                      const std::vector<float>& pos, int64_t* out) {
    const int F = (int)(pos.size() / 9);
    int64_t nodes = 0, tris = 0, dup = 0, bad = 0, maxd = 0;
    std::vector<int> seen(F, 0);
    std::vector<RefRegion> refs;
    RefRegion cur{0, {-FLT_MAX, -FLT_MAX, -FLT_MAX}, {FLT_MAX, FLT_MAX, FLT_MAX}};
    std::function<void(int32_t, int)> walk = [&](int32_t ni, int depth) {
        if (ni < 0 || (size_t)ni >= b4.size()) {
            bad++;
            return;
        }
        nodes++;
        maxd = std::max<int64_t>(maxd, depth);
        const BvhNode4& n = b4[ni];
        const BvhNode4Q& q = q4[ni];
        for (int k = 0; k < 4; k++) {
            if (n.child[k] == kBvh4Empty || (n.child[k] < 0 && n.count[k] == 0)) continue;
            const RefRegion saved = cur;
            for (int a = 0; a < 3; a++) {
                cur.lo[a] = std::max(cur.lo[a], n.lo[a][k]), cur.hi[a] = std::min(cur.hi[a], n.hi[a][k]);
                const uint32_t bits = ((q.ex >> (8 * a)) & 0xffu) << 23;
                float sc_;
                std::memcpy(&sc_, &bits, 4);
                const float ql = std::fmaf((float)((q.q[2 * a] >> (8 * k)) & 0xffu), sc_, q.org[a]);
                const float qh = std::fmaf((float)((q.q[2 * a + 1] >> (8 * k)) & 0xffu), sc_, q.org[a]);
                if (!(ql <= n.lo[a][k] && qh >= n.hi[a][k])) bad++;
            }
            if (n.child[k] >= 0) {
                walk(n.child[k], depth + 1);
            } else {
                const int32_t first = ~n.child[k];
                for (int32_t j = first; j < first + n.count[k]; j++) {
                    if (j < 0 || (size_t)j >= leaf_facets.size() || leaf_facets[j] < 0 || leaf_facets[j] >= F) {
                        bad++;
                        continue;
                    }
                    const int f = leaf_facets[j];
                    tris++;
                    if (seen[f]++) dup++;
                    cur.f = f;
                    refs.push_back(cur);
                }
            }
            cur = saved;
        }
    };
    if (!b4.empty()) walk(0, 1);
    bad += check_coverage(pos, refs);
    std::vector<int32_t> distinct(leaf_facets);
    std::sort(distinct.begin(), distinct.end());
    out[0] = nodes;
    out[1] = tris - dup;  // distinct facets reached
    out[2] = (int64_t)(std::unique(distinct.begin(), distinct.end()) - distinct.begin());
    out[3] = dup;
    out[4] = bad;
    out[5] = maxd;
}
// the positions the trees are checked against: the host's, with a hidden facet (mcpt_scene_set_visible, DESIGN.md
// §4.28) as the collapsed triangle its leaf slots hold -- its first vertex three times; the host's own when none is
static std::vector<float> slot_positions(const HostScene& hs) {
    std::vector<float> pos(hs.pos);
    for (int f = 0; f < hs.F; f++)
        if (hs.is_hidden(f))
            for (int k = 1; k < 3; k++) std::copy_n(&hs.pos[9 * (size_t)f], 3, &pos[9 * (size_t)f + 3 * k]);
    return pos;
}
int mcpt_debug_bvh4_check(mcpt_scene* sc, int32_t light_only, int64_t* out) {
    if (!sc || !out) {
        set_error("invalid argument");
        return MCPT_E_INVALID;
    }
    std::lock_guard<std::mutex> lk(sc->mu);
    if (int rs = host_sync(sc)) return rs;
    const Bvh& bb = light_only ? sc->lbvh : sc->bvh;
    const std::vector<BvhNode4> b4 = collapse_bvh4(bb);
    bvh4_walk(b4, quantize_bvh4(b4), bb.leaf_facets, slot_positions(sc->host), out);
    return MCPT_OK;
}

// what `device` holds of the main tree: nodes with their leaf codes unpacked, quantized nodes, the facet and the
// vertices of every leaf slot, the facet array's vertices
struct DeviceTree {
    std::vector<BvhNode4> b4;
    std::vector<BvhNode4Q> q4;
    std::vector<float4> leaf_v, tri_v;
    std::vector<int32_t> leaf_facets;
};
static int download_tree(mcpt_scene* sc, int32_t device, bool vertices, DeviceTree* t, bool light_only = false) {
    DeviceState* D;
    int rc;
    if ((rc = host_sync(sc))) return rc;  // the device check compares against host.pos
    if ((rc = get_device_state(sc, device, &D))) return rc;
    HIP_OK(hipDeviceSynchronize());
    const DScene& d = D->d;
    const size_t nslots = light_only ? sc->lbvh.leaf_facets.size() : D->nslots;
    const int nn = light_only ? d.nlbvh4 : d.nbvh4;
    t->b4.resize(nn);
    t->q4.resize(nn);
    t->leaf_v.resize(3 * nslots);
    HIP_OK(hipMemcpy(t->b4.data(), light_only ? d.lbvh4 : d.bvh4, t->b4.size() * sizeof(BvhNode4), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(t->q4.data(), light_only ? d.lbvh4q : d.bvh4q, t->q4.size() * sizeof(BvhNode4Q), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(t->leaf_v.data(), light_only ? d.lleaf_v : d.leaf_v, t->leaf_v.size() * sizeof(float4), hipMemcpyDeviceToHost));
    if (vertices) {
        t->tri_v.resize(3 * (size_t)d.F);
        HIP_OK(hipMemcpy(t->tri_v.data(), d.tri_v, t->tri_v.size() * sizeof(float4), hipMemcpyDeviceToHost));
    }
    for (BvhNode4& n : t->b4)
        for (int k = 0; k < 4; k++)
            if (n.child[k] < 0) n.child[k] = ~(~n.child[k] >> kLeafBits);  // pack_leaf_codes kept count[k]
    t->leaf_facets.resize(nslots);
    for (size_t q = 0; q < nslots; q++) std::memcpy(&t->leaf_facets[q], &t->leaf_v[3 * q].w, 4);
    return MCPT_OK;
}
static int bvh4_check_device(mcpt_scene* sc, int32_t device, bool light_only, int64_t* out);
int mcpt_debug_bvh4_check_device(mcpt_scene* sc, int32_t device, int64_t* out) { return bvh4_check_device(sc, device, false, out); }
int mcpt_debug_bvh4_check_device_light(mcpt_scene* sc, int32_t device, int64_t* out) { return bvh4_check_device(sc, device, true, out); }
static int bvh4_check_device(mcpt_scene* sc, int32_t device, bool light_only, int64_t* out) {
    if (!sc || !out) {
        set_error("invalid argument");
        return MCPT_E_INVALID;
    }
    std::lock_guard<std::mutex> lk(sc->mu);
    DeviceTree t;
    int rc;
    if ((rc = download_tree(sc, device, true, &t, light_only))) return rc;
    // a hidden facet's slot must hold its collapsed form and a visible facet's its triangle: either way round is an error
    const std::vector<float> pos = slot_positions(sc->host);
    bvh4_walk(t.b4, t.q4, t.leaf_facets, pos, out);
    // the device's own copies of the vertices against the host's: the slots against the slot form, the facet array
    // against the stored values (a hidden facet keeps them)
    auto differs = [&](const float4* v, const std::vector<float>& p, int f) {
        int64_t n = 0;
        for (int k = 0; k < 3; k++) n += std::memcmp(&v[k].x, &p[9 * (size_t)f + 3 * k], 12) != 0;
        return n;
    };
    for (size_t q = 0; q < t.leaf_facets.size(); q++)
        if (t.leaf_facets[q] >= 0 && t.leaf_facets[q] < sc->host.F) out[4] += differs(&t.leaf_v[3 * q], pos, t.leaf_facets[q]);
    for (int f = 0; f < sc->host.F; f++) out[4] += differs(&t.tri_v[3 * (size_t)f], sc->host.pos, f);
    return MCPT_OK;
}
int mcpt_debug_light_tables(mcpt_scene* sc, int32_t device, const char* which, void* out, int64_t cap, int64_t* bytes) {
    if (!sc || !which || !bytes) {
        set_error("mcpt_debug_light_tables: invalid argument");
        return MCPT_E_INVALID;
    }
    std::lock_guard<std::mutex> lk(sc->mu);
    DeviceState* D;
    int rc;
    if ((rc = get_device_state(sc, device, &D))) return rc;
    HIP_OK(hipDeviceSynchronize());
    const DScene& d = D->d;
    // the sizes get_device_state allocated
    const size_t NL = (size_t)std::max(d.NL, 1), nch = (size_t)prep_chunks(d.NL), nl_pad = 256 * ((nch + 3) / 4);
    const std::string w = which;
    const void* src = nullptr;
    size_t n = 0;
    LightGlobals g{};
    if (w == "lt_v") src = d.lt_v, n = 3 * NL * sizeof(float4);
    else if (w == "lt_n") src = d.lt_n, n = NL * sizeof(double4);
    else if (w == "lt_pk") src = d.lt_pk, n = 3 * nl_pad * sizeof(float4);
    else if (w == "lt_d") src = d.lt_d, n = nl_pad * sizeof(float);
    else if (w == "lt_w") src = d.lt_w, n = 5 * (nl_pad + kSentinelPad) * sizeof(double2);
    else if (w == "lt_f") src = d.lt_f, n = 4 * (nl_pad + kSentinelPad) * sizeof(float4);
    else if (w == "lt_pair") src = d.lt_pair, n = 32 * nch * sizeof(LightPair);
    else if (w == "chunk_sph") src = d.chunk_sph, n = nch * sizeof(float4);
    else if (w == "chunk_sk") src = d.chunk_sk, n = nch * sizeof(float2);
    else if (w == "l_area") src = d.l_area, n = (size_t)d.NL * sizeof(double);
    else if (w == "l_area_cum") src = d.l_area_cum, n = (size_t)d.NL * sizeof(double);
    else if (w == "light_rad") src = d.light_rad, n = 3 * (size_t)d.NL * sizeof(double);
    else if (w == "light_sum") src = d.light_sum, n = (size_t)d.NL * sizeof(double);
    else if (w == "grp_sum") src = d.grp_sum, n = (size_t)d.ngroups * sizeof(double);
    else if (w == "grp_cum") src = d.grp_cum, n = (size_t)d.ngroups * sizeof(double);
    else if (w == "mtl") src = d.mtl, n = 7 * (size_t)sc->host.M * sizeof(float);
    else if (w == "globals") {
        for (int a = 0; a < 3; a++) g.band_ctr[a] = d.band_ctr[a];
        g.band_R = d.band_R, g.band_S = d.band_S, g.band_K = d.band_K, g.light_bound = d.light_bound;
        n = sizeof g;
    } else {
        set_error("mcpt_debug_light_tables: no table named '%s'", which);
        return MCPT_E_INVALID;
    }
    *bytes = (int64_t)n;
    if (!out) return MCPT_OK;
    if (cap < (int64_t)n) {
        set_error("mcpt_debug_light_tables: '%s' has %zu bytes, more than the buffer's %lld", which, n, (long long)cap);
        return MCPT_E_INVALID;
    }
    if (src) {
        if (n) HIP_OK(hipMemcpy(out, src, n, hipMemcpyDeviceToHost));
    } else {
        std::memcpy(out, &g, n);
    }
    return MCPT_OK;
}

int mcpt_debug_light_area_cum_bench(mcpt_scene* sc, int32_t device, int32_t reps, double* seconds) {
    if (!sc || !seconds || reps < 1) {
        set_error("mcpt_debug_light_area_cum_bench: invalid argument");
        return MCPT_E_INVALID;
    }
    std::lock_guard<std::mutex> lk(sc->mu);
    DeviceState* D;
    int rc;
    if ((rc = get_device_state(sc, device, &D))) return rc;
    if (sc->host.NL < 1) {
        set_error("mcpt_debug_light_area_cum_bench: the scene has no lights");
        return MCPT_E_INVALID;
    }
    ensure_slot_map(sc, false);
    if ((rc = ensure_refit_state(sc, *D)) || (rc = ensure_light_state(sc, *D))) return rc;
    HIP_OK(hipDeviceSynchronize());
    for (int k = -1; k < reps; k++) {  // one warm-up run
        HIP_OK(hipMemsetAsync(D->ltab.group_dirty, 1, (size_t)D->ltab.ngroups, D->stream));
        if (k == 0) HIP_OK(hipEventRecord(D->evl0, D->stream));
        if ((rc = light_area_cum_enqueue(D->ltab, D->stream))) return rc;
    }
    HIP_OK(hipEventRecord(D->evl1, D->stream));
    HIP_OK(hipMemsetAsync(D->ltab.group_dirty, 0, (size_t)D->ltab.ngroups, D->stream));
    HIP_OK(hipStreamSynchronize(D->stream));
    float ms = 0;
    HIP_OK(hipEventElapsedTime(&ms, D->evl0, D->evl1));
    *seconds = 1e-3 * ms / reps;
    return MCPT_OK;
}

int mcpt_debug_bvh4_download(mcpt_scene* sc, int32_t device, int64_t* counts, void* nodes, void* qnodes, int32_t* leaf_facets,
                             int64_t cap_nodes, int64_t cap_slots) {
    if (!sc || !counts) {
        set_error("invalid argument");
        return MCPT_E_INVALID;
    }
    std::lock_guard<std::mutex> lk(sc->mu);
    DeviceTree t;
    int rc;
    if ((rc = download_tree(sc, device, false, &t))) return rc;
    counts[0] = (int64_t)t.b4.size();
    counts[1] = (int64_t)t.leaf_facets.size();
    if (((nodes || qnodes) && cap_nodes < counts[0]) || (leaf_facets && cap_slots < counts[1])) {
        set_error("mcpt_debug_bvh4_download: the tree has %lld nodes and %lld leaf slots, more than the buffers hold",
                  (long long)counts[0], (long long)counts[1]);
        return MCPT_E_INVALID;
    }
    if (nodes) std::memcpy(nodes, t.b4.data(), t.b4.size() * sizeof(BvhNode4));
    if (qnodes) std::memcpy(qnodes, t.q4.data(), t.q4.size() * sizeof(BvhNode4Q));
    if (leaf_facets) std::copy(t.leaf_facets.begin(), t.leaf_facets.end(), leaf_facets);
    return MCPT_OK;
}

int mcpt_debug_bvh4_host(mcpt_scene* sc, int32_t light_only, int64_t* counts, void* nodes, void* qnodes, int32_t* leaf_facets,
                         int64_t cap_nodes, int64_t cap_slots) {
    if (!sc || !counts) {
        set_error("invalid argument");
        return MCPT_E_INVALID;
    }
    std::lock_guard<std::mutex> lk(sc->mu);
    if (int rs = host_sync(sc)) return rs;
    const Bvh& bb = light_only ? sc->lbvh : sc->bvh;
    const std::vector<BvhNode4> b4 = collapse_bvh4(bb);
    counts[0] = (int64_t)b4.size();
    counts[1] = (int64_t)bb.leaf_facets.size();
    if (((nodes || qnodes) && cap_nodes < counts[0]) || (leaf_facets && cap_slots < counts[1])) {
        set_error("mcpt_debug_bvh4_host: the tree has %lld nodes and %lld leaf slots, more than the buffers hold",
                  (long long)counts[0], (long long)counts[1]);
        return MCPT_E_INVALID;
    }
    if (nodes) std::memcpy(nodes, b4.data(), b4.size() * sizeof(BvhNode4));
    if (qnodes) {
        const std::vector<BvhNode4Q> q4 = quantize_bvh4(b4);
        std::memcpy(qnodes, q4.data(), q4.size() * sizeof(BvhNode4Q));
    }
    if (leaf_facets) std::copy(bb.leaf_facets.begin(), bb.leaf_facets.end(), leaf_facets);
    return MCPT_OK;
}

int mcpt_debug_bvh8_check(mcpt_scene* sc, int32_t light_only, int64_t* out) {
    if (!sc || !out) {
        set_error("invalid argument");
        return MCPT_E_INVALID;
    }
    std::lock_guard<std::mutex> lk(sc->mu);
    if (int rc = bvh8_refused(sc)) return rc;
    ensure_bvh8_host(sc);
    const Bvh8& b = light_only ? sc->lbvh8 : sc->bvh8;
    const Bvh& bb = light_only ? sc->lbvh : sc->bvh;
    const HostScene& hs = sc->host;
    int64_t nodes = 0, tris = 0, dup = 0, bad = 0, maxd = 0;
    std::vector<int> seen(hs.F, 0);
    struct Box {
        float lo[3], hi[3];
    };
    std::vector<Box> path;
    std::vector<RefRegion> refs;
    auto decode = [](const BvhNode8Q& n, int a, int k, bool hi) {
        const uint32_t w = hi ? n.qhi[a][k >> 2] : n.qlo[a][k >> 2];
        const uint32_t bits = ((n.ex >> (8 * a)) & 0xffu) << 23;
        float sc_;
        std::memcpy(&sc_, &bits, 4);
        return std::fmaf((float)((w >> (8 * (k & 3))) & 0xffu), sc_, n.org[a]);
    };
    std::function<void(int32_t, int)> walk = [&](int32_t ni, int depth) {
        if (ni < 0 || (size_t)ni >= b.nodes.size()) {
            bad++;
            return;
        }
        nodes++;
        maxd = std::max<int64_t>(maxd, depth);
        const BvhNode8Q& n = b.nodes[ni];
        const uint32_t imask = n.ex >> 24;
        for (int k = 0; k < 8; k++) {
            Box bx;
            for (int a = 0; a < 3; a++) bx.lo[a] = decode(n, a, k, false), bx.hi[a] = decode(n, a, k, true);
            path.push_back(bx);
            if (imask & (1u << k)) {
                walk(n.base_inner + k, depth + 1);
            } else {
                for (int j = 0; j < 2; j++) {
                    if (!(n.tvalid & (1u << (2 * k + j)))) continue;
                    const int64_t q = (int64_t)n.base_tri + 2 * k + j;
                    if (q < 0 || (size_t)q >= b.tri_facets.size() || b.tri_facets[q] < 0 || b.tri_facets[q] >= hs.F) {
                        bad++;
                        continue;
                    }
                    const int f = b.tri_facets[q];
                    tris++;
                    if (seen[f]++) dup++;
                    RefRegion r{f, {-FLT_MAX, -FLT_MAX, -FLT_MAX}, {FLT_MAX, FLT_MAX, FLT_MAX}};
                    for (const Box& p : path)
                        for (int a = 0; a < 3; a++) r.lo[a] = std::max(r.lo[a], p.lo[a]), r.hi[a] = std::min(r.hi[a], p.hi[a]);
                    refs.push_back(r);
                }
            }
            path.pop_back();
        }
    };
    if (!b.nodes.empty()) walk(0, 1);
    bad += check_coverage(hs.pos, refs);
    out[0] = nodes;
    out[1] = tris - dup;  // distinct facets reached
    out[2] = (int64_t)bb.leaf_facets.size() - dup_refs(bb);
    out[3] = dup;
    out[4] = bad;
    out[5] = maxd;
    return MCPT_OK;
}

}  // extern "C"
