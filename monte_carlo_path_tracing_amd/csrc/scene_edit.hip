// Scene editing: everything that changes a loaded scene's geometry in place and keeps the host copy, the device
// states and their trees in step -- mcpt_scene_update[_device], movable lights, mcpt_scene_pose_save / _rest_save,
// mcpt_scene_transform with the lazily synced host copy, mcpt_scene_rebuild and mcpt_scene_tree_cost, the facet
// visibility of mcpt_scene_set_visible -- and what its
// lights and surfaces look like: mcpt_scene_set_light_radiance[_device], mcpt_scene_set_materials (include/mcpt.h).
// Host code only: the kernels are refit.hip's, light_tables.hip's and rebuild.hip's.  Locks are taken in the order
// mu, host_mu, devs_mu; every function that visits device states leaves the caller's device current (DeviceRestore).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "scene_state.h"  // with mcpt.h, mcpt_internal.h and the HIP runtime

using namespace mcpt;

// the facet -> leaf-slot map and the binary tree's refit index of the main or the light-only tree, built at the
// handle's first update or transform (the light-only tree's: at its first light move)
void mcpt::ensure_slot_map(mcpt_scene* sc, bool light_tree) {
    SlotMap& m = light_tree ? sc->lslots : sc->slots;
    if (!m.start.empty()) return;
    const Bvh& b = light_tree ? sc->lbvh : sc->bvh;
    make_facet_slot_map(b, sc->host.F, m.start, m.list);
    m.ix = make_bvh_refit_index(b);
}
static bool range_has_light(const mcpt_scene* sc, int32_t first, int32_t end) {
    for (int f = first; f < end; f++)
        if (sc->host.light_of[f] >= 0) return true;
    return false;
}

std::vector<DeviceState*> mcpt::device_states(mcpt_scene* sc) {
    std::vector<DeviceState*> devs;
    std::lock_guard<std::mutex> lk(sc->devs_mu);
    for (auto& D : sc->devs) devs.push_back(D.get());
    return devs;
}

// mcpt_scene_host_sync: the host copy brought up to date from the first device state (every state holds the same
// arrays) -- the pending ranges of tri_v / tri_n into host.pos / host.nrm, then update_apply's host half over them,
// and the previous pose as a whole if a pose_save left it stale.  Every reader of host.pos, host.nrm, host.unique_n,
// the binary tree's boxes, prev_pos or prev_nrm calls this first; a no-op when nothing is pending.
int mcpt::host_sync(mcpt_scene* sc) {
    std::lock_guard<std::mutex> lk(sc->host_mu);
    if (sc->pending.r.empty() && !sc->prev_stale) return MCPT_OK;
    const std::vector<DeviceState*> devs = device_states(sc);
    DeviceState* D = devs.empty() ? nullptr : devs.front();
    if (!D) {
        set_error("the host copy is behind the devices but the scene has no device state");
        return MCPT_E_DEVICE;
    }
    DeviceRestore back;
    HIP_OK(hipGetDevice(&back.device));
    HIP_OK(hipSetDevice(D->device));
    HostScene& hs = sc->host;
    // every copy lands in a buffer of its own first: a copy that fails leaves the host copy as it was, still pending
    std::vector<std::vector<float4>> dv(sc->pending.r.size());
    std::vector<std::vector<float>> dn(sc->pending.r.size());
    for (size_t i = 0; i < sc->pending.r.size(); i++) {
        const size_t f0 = (size_t)sc->pending.r[i].first, n = (size_t)sc->pending.r[i].second - f0;
        dv[i].resize(3 * n);
        dn[i].resize(9 * n);
        HIP_OK(hipMemcpy(dv[i].data(), D->d.tri_v + 3 * f0, 3 * n * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(dn[i].data(), D->d.tri_n + 9 * f0, 9 * n * sizeof(float), hipMemcpyDeviceToHost));
    }
    std::vector<float4> pv;
    std::vector<float> pn;
    if (sc->prev_stale && hs.F > 0) {  // the device copies change only at a pose_save: they are still that pose
        pv.resize(3 * (size_t)hs.F);
        pn.resize(hs.nrm.size());
        HIP_OK(hipMemcpy(pv.data(), D->prev_v.p, pv.size() * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(pn.data(), D->prev_n.p, pn.size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    auto unpack = [](const std::vector<float4>& v, float* out) {
        for (size_t i = 0; i < v.size(); i++) out[3 * i] = v[i].x, out[3 * i + 1] = v[i].y, out[3 * i + 2] = v[i].z;
    };
    for (size_t i = 0; i < sc->pending.r.size(); i++) {
        const size_t f0 = (size_t)sc->pending.r[i].first;
        unpack(dv[i], hs.pos.data() + 9 * f0);
        std::copy(dn[i].begin(), dn[i].end(), hs.nrm.begin() + 9 * f0);
    }
    if (!sc->pending.r.empty()) {
        ensure_slot_map(sc, false);
        host_refresh_ranges(hs, sc->bvh, sc->slots.ix, sc->slots.start, sc->slots.list, sc->pending, sc->margin);
        bool lights = false;  // a transform moved light triangles (mcpt_scene_set_lights_movable): areas, light-only tree
        for (const auto& p : sc->pending.r) lights = lights || range_has_light(sc, p.first, p.second);
        if (lights) {
            ensure_slot_map(sc, true);
            host_refresh_lights(hs, sc->lbvh, sc->lslots.ix, sc->lslots.start, sc->lslots.list, sc->pending, sc->margin);
        }
        sc->grid.ok = false;  // as update_apply: rebuilt from the new positions by the next grid-mode call
    }
    if (sc->prev_stale) {
        sc->prev_pos.resize(hs.pos.size());
        unpack(pv, sc->prev_pos.data());
        sc->prev_nrm = std::move(pn);
    }
    sc->pending.r.clear();
    sc->prev_stale = false;
    return MCPT_OK;
}
// the refusal of a NULL scene or, where a call has another required pointer (arg_name), of that
static int refuse_null(const char* who, const void* sc, const void* arg = nullptr, const char* arg_name = nullptr) {
    if (sc && (arg || !arg_name)) return MCPT_OK;
    set_error("%s: NULL %s", who, !sc ? "scene" : arg_name);
    return MCPT_E_INVALID;
}
// the three stats structs (mcpt_update_stats, mcpt_light_update_stats, mcpt_rebuild_stats): zeroed with their size
// filled in, and the refusal of a caller's struct of another size (null: nothing to check)
template <class S>
static void stats_init(S* st) {
    if (!st) return;
    std::memset((void*)st, 0, sizeof *st);
    st->struct_size = sizeof *st;
}
template <class S>
static int check_struct_size(const S* st, const char* name) {
    if (!st || st->struct_size == sizeof(S)) return MCPT_OK;
    set_error("%s.struct_size %u does not match this library's %zu (header / library version mismatch)", name, st->struct_size,
              sizeof(S));
    return MCPT_E_INVALID;
}

// ---- mcpt_scene_update (include/mcpt.h; the kernels are refit.hip's) ----

// every refusal that needs neither the values nor a device
// `data`: the call's required pointer argument and its name in the message
static int update_check_args(const mcpt_scene* sc, int32_t first, int32_t count, const void* data, const mcpt_update_stats* stats,
                             const char* who = "mcpt_scene_update", const char* data_name = "positions") {
    if (int rn = refuse_null(who, sc, data, data_name)) return rn;
    if (count < 1 || first < 0 || (int64_t)first + count > sc->host.F) {
        set_error("%s: facets [%d, %lld) are not a non-empty range of the scene's %d facets", who, first,
                  (long long)first + count, sc->host.F);
        return MCPT_E_INVALID;
    }
    return check_struct_size(stats, "mcpt_update_stats");
}
static int update_check_lights(const mcpt_scene* sc, int32_t first, int32_t count, const char* who = "mcpt_scene_update") {
    if (sc->lights_movable) return MCPT_OK;  // mcpt_scene_set_lights_movable: light facets move as any other
    for (int f = first; f < first + count; f++)
        if (sc->host.light_of[f] >= 0) {
            set_error("%s: facet %d is a light triangle (light %d); lights cannot move", who, f, sc->host.light_of[f]);
            return MCPT_E_INVALID;
        }
    return MCPT_OK;
}
// the arena: the build's box grown by its largest axis extent on every side
static void update_arena(const mcpt_scene* sc, double lo[3], double hi[3]) {
    for (int a = 0; a < 3; a++) lo[a] = sc->build_lo[a] - sc->build_ext, hi[a] = sc->build_hi[a] + sc->build_ext;
}
static int update_check_values(const mcpt_scene* sc, int32_t first, int32_t count, const float* pos, const float* nrm,
                               const char* who = "mcpt_scene_update") {
    double lo[3], hi[3];
    update_arena(sc, lo, hi);
    for (size_t i = 0; i < 9 * (size_t)count; i++) {
        const int f = first + (int)(i / 9), a = (int)(i % 3);
        if (!std::isfinite(pos[i]) || (nrm && !std::isfinite(nrm[i]))) {
            set_error("%s: facet %d has a non-finite %s", who, f, std::isfinite(pos[i]) ? "normal" : "position");
            return MCPT_E_INVALID;
        }
        if (pos[i] < lo[a] || pos[i] > hi[a]) {
            set_error("%s: facet %d has a position outside the arena (axis %d: %g not in [%g, %g], the "
                      "build's box grown by its largest extent)", who, f, a, (double)pos[i], lo[a], hi[a]);
            return MCPT_E_INVALID;
        }
    }
    return MCPT_OK;
}

// the first node of every level of a breadth-first 4-wide tree (nodes with packed leaf codes); false if the tree is
// not in that order or an index is out of range
static bool bvh4_levels(const std::vector<BvhNode4>& b4, size_t nslots, std::vector<int32_t>* levels) {
    const int32_t nn = (int32_t)b4.size();
    std::vector<int32_t> lf{0, 1};
    bool ok = !b4.empty();
    while (ok) {
        const int32_t n0 = lf[lf.size() - 2], n1 = lf.back();
        int64_t next = n1;  // breadth-first order: the inner children of a level are the next level, in order
        for (int32_t n = n0; n < n1 && ok; n++)
            for (int k = 0; k < 4; k++) {
                const int32_t c = b4[n].child[k];
                if (c == kBvh4Empty) continue;
                if (c >= 0) {
                    ok = ok && c == next++ && c < nn;
                } else {
                    const int64_t s0 = ~c >> kLeafBits, cnt = ~c & ((1 << kLeafBits) - 1);
                    ok = ok && s0 + cnt <= (int64_t)nslots;
                }
            }
        if (next == n1) break;
        ok = ok && next <= nn;
        lf.push_back((int32_t)next);
    }
    if (!ok || lf.back() != nn) return false;
    *levels = std::move(lf);
    return true;
}
// what refit.hip's kernels need of one 4-wide tree of D (the current device), built once: the tree's indices are
// checked here, so the kernels need no bounds tests; then the CSR facet -> leaf-slot map `m`, the dirty bytes and the
// counters are uploaded and the first node of every level is kept.  `tree` names the tree in the refusal.
static int build_tree_refit(DeviceState& D, TreeRefit& t, const BvhNode4* nodes, const BvhNode4Q* qnodes, int nnodes,
                            const float4* leaf_v, size_t nslots, const SlotMap& m, const char* tree) {
    std::vector<BvhNode4> b4(nnodes);
    HIP_OK(hipMemcpy(b4.data(), nodes, b4.size() * sizeof(BvhNode4), hipMemcpyDeviceToHost));
    std::vector<int32_t> lf;
    if (!bvh4_levels(b4, nslots, &lf)) {
        set_error("mcpt_scene_update: device %d's %s4-wide tree is not in breadth-first order", D.device, tree);
        return MCPT_E_SCENE;
    }
    RefitDev& r = t.dev;
    r.F = D.d.F;
    r.nslots = (int32_t)nslots;
    r.nnodes = nnodes;
    r.tri_v = const_cast<float*>(reinterpret_cast<const float*>(D.d.tri_v));
    r.tri_n = const_cast<float*>(D.d.tri_n);
    r.leaf_v = const_cast<float*>(reinterpret_cast<const float*>(leaf_v));
    r.bvh4 = const_cast<BvhNode4*>(nodes);
    r.bvh4q = const_cast<BvhNode4Q*>(qnodes);
    int rc;
    if ((rc = upload(D, m.start, &r.slot_start)) || (rc = upload(D, m.list, &r.slot_list))) return rc;
    const std::vector<uint8_t> zs(std::max<size_t>(nslots, 1), 0), zn(std::max<size_t>(b4.size(), 1), 0);
    const std::vector<unsigned> zc(16, 0);
    if ((rc = upload(D, zs, &r.slot_dirty)) || (rc = upload(D, zn, &r.node_dirty)) || (rc = upload(D, zc, &r.counters))) return rc;
    t.level_first = std::move(lf);
    return MCPT_OK;
}
// a device state's first update or transform: the main tree's (the scene's slot map exists: ensure_slot_map)
int mcpt::ensure_refit_state(mcpt_scene* sc, DeviceState& D) {
    if (D.refit.ready) return MCPT_OK;
    if (int rc = build_tree_refit(D, D.refit, D.d.bvh4, D.d.bvh4q, D.d.nbvh4, D.d.leaf_v, D.nslots, sc->slots, "")) return rc;
    D.refit.ready = true;
    return ensure_hidden_state(sc, D);
}
// the state's copy of the handle's visibility mask, made from the host's bytes as they are -- a
// state's slots were written under exactly that mask, by get_device_state or by the calls since -- and handed to the
// refit state if there is one.  Nothing to do for a handle that never hid a facet: the pointer stays null.
int mcpt::ensure_hidden_state(mcpt_scene* sc, DeviceState& D) {
    const std::vector<uint8_t>& h = sc->host.hidden;
    if (h.empty()) return MCPT_OK;
    if (!D.hidden.p) {
        if (int rc = ensure(D.hidden, h.size())) return rc;
        HIP_OK(hipMemcpy(D.hidden.p, h.data(), h.size(), hipMemcpyHostToDevice));
    }
    if (D.refit.ready) D.refit.dev.hidden = (uint8_t*)D.hidden.p;
    return MCPT_OK;
}

// the tables' half of what a device state's first light move builds, and all a re-light needs: the
// light tables' pointers, the light -> group map, the chunk rows (filled here from the tables as they are), the dirty
// bytes, the counters and the small struct of constants.  Needs neither refit state.  The current device is D's.
int mcpt::ensure_light_tables(mcpt_scene* sc, DeviceState& D) {
    if (D.ltab_ready) return MCPT_OK;
    const DScene& d = D.d;
    const HostScene& hs = sc->host;
    if (hs.NL < 1) {
        set_error("the scene has no lights");
        return MCPT_E_INVALID;
    }
    int rc;
    const int nch = prep_chunks(hs.NL), ng = d.ngroups;
    std::vector<int32_t> lgroup(hs.NL, 0);
    for (int g = 0; g < ng; g++)
        for (int l = hs.group_start[g]; l < hs.group_start[g] + hs.group_count[g]; l++) lgroup[l] = g;
    const std::vector<uint8_t> zch(nch, 0), zg(std::max(ng, 1), 0);
    const std::vector<double> zrow(kLightRowWords * (size_t)nch, 0.0);
    const std::vector<LightGlobals> zglob(1);
    const std::vector<unsigned> zc(16, 0);
    LightTabDev& t = D.ltab;
    if ((rc = upload(D, zch, &t.chunk_dirty)) || (rc = upload(D, zg, &t.group_dirty)) || (rc = upload(D, zrow, &t.chunk_row)) ||
        (rc = upload(D, zglob, &t.globals)) || (rc = upload(D, lgroup, &t.light_group)) || (rc = upload(D, zc, &t.counters)))
        return rc;
    t.tri_v = reinterpret_cast<const float*>(d.tri_v);
    t.tri_n = d.tri_n;
    t.tri_light = d.tri_light;
    t.light_rad = const_cast<double*>(d.light_rad);
    t.light_sum = const_cast<double*>(d.light_sum);
    t.grp_sum = const_cast<double*>(d.grp_sum);
    t.grp_cum = const_cast<double*>(d.grp_cum);
    t.grp_range = reinterpret_cast<const int32_t*>(d.grp_range);
    t.lt_v = const_cast<float*>(reinterpret_cast<const float*>(d.lt_v));
    t.lt_n = const_cast<double*>(reinterpret_cast<const double*>(d.lt_n));
    t.lt_pk = const_cast<float*>(reinterpret_cast<const float*>(d.lt_pk));
    t.lt_d = const_cast<float*>(d.lt_d);
    t.lt_w = const_cast<double*>(reinterpret_cast<const double*>(d.lt_w));
    t.lt_f = const_cast<float*>(reinterpret_cast<const float*>(d.lt_f));
    t.lt_pair = const_cast<float*>(reinterpret_cast<const float*>(d.lt_pair));
    t.l_area = const_cast<double*>(d.l_area);
    t.l_area_cum = const_cast<double*>(d.l_area_cum);
    t.chunk_sph = const_cast<float*>(reinterpret_cast<const float*>(d.chunk_sph));
    t.chunk_sk = const_cast<float*>(reinterpret_cast<const float*>(d.chunk_sk));
    t.F = d.F;
    t.NL = hs.NL;
    t.nchunks = nch;
    t.ngroups = ng;
    if (!D.pinned_globals) HIP_OK(hipHostMalloc(&D.pinned_globals, sizeof(LightGlobals)));
    if (!D.evl0) HIP_OK(hipEventCreate(&D.evl0));
    if (!D.evl1) HIP_OK(hipEventCreate(&D.evl1));
    // every chunk's row from the tables as they are: a later move recomputes only its own chunks
    if ((rc = light_chunks_all_enqueue(t, D.stream))) return rc;
    HIP_OK(hipStreamSynchronize(D.stream));
    D.ltab_ready = true;
    return MCPT_OK;
}

// what a device state's first light move builds (after ensure_refit_state): build_tree_refit's state for the
// light-only tree, then the tables' half above.  The current device is D's.
int mcpt::ensure_light_state(mcpt_scene* sc, DeviceState& D) {
    if (D.lrefit.ready) return MCPT_OK;
    const DScene& d = D.d;
    ensure_slot_map(sc, true);
    int rc;  // a scene without lights has no light-only tree to refit: refused as a tree of no nodes
    if ((rc = build_tree_refit(D, D.lrefit, d.lbvh4, d.lbvh4q, sc->host.NL < 1 ? 0 : d.nlbvh4, d.lleaf_v, sc->lbvh.leaf_facets.size(),
                               sc->lslots, "light-only ")) ||
        (rc = ensure_light_tables(sc, D)))
        return rc;
    D.lrefit.ready = true;
    return MCPT_OK;
}

extern "C" {

void mcpt_update_stats_init(mcpt_update_stats* st) { stats_init(st); }

// the light stage of an update or transform on one state, after refit_enqueue's scatter on the same stream; the
// constants land in the state's pinned copy by the time the stream is synchronised
static int light_stage_enqueue(mcpt_scene* sc, DeviceState& D, int32_t first, int32_t count) {
    HIP_OK(hipEventRecord(D.evl0, D.stream));
    if (int rc = light_tables_enqueue(D.ltab, D.lrefit.dev, D.lrefit.level_first.data(), (int)D.lrefit.level_first.size() - 1, first, count,
                                      sc->margin, D.stream))
        return rc;
    HIP_OK(hipEventRecord(D.evl1, D.stream));
    HIP_OK(hipMemcpyAsync(D.pinned_globals, D.ltab.globals, sizeof(LightGlobals), hipMemcpyDeviceToHost, D.stream));
    return MCPT_OK;
}
// after that synchronisation: the state's by-value constants patched; lst != null: the first state's numbers
static int light_stage_finish(DeviceState& D, mcpt_light_update_stats* lst) {
    const LightGlobals& g = *D.pinned_globals;
    for (int a = 0; a < 3; a++) D.d.band_ctr[a] = g.band_ctr[a];
    D.d.band_R = g.band_R;
    D.d.band_S = g.band_S;
    D.d.band_K = g.band_K;
    D.d.light_bound = g.light_bound;
    if (lst) {
        float ms = 0;
        unsigned c[4] = {0, 0, 0, 0};
        HIP_OK(hipEventElapsedTime(&ms, D.evl0, D.evl1));
        HIP_OK(hipMemcpy(c, D.lrefit.dev.counters, 2 * sizeof(unsigned), hipMemcpyDeviceToHost));  // [1]: the tree's
        HIP_OK(hipMemcpy(c + 2, D.ltab.counters + 2, 2 * sizeof(unsigned), hipMemcpyDeviceToHost));  // [2], [3]: the tables'
        lst->device_seconds = 1e-3 * ms;
        lst->light_nodes_refit = c[1];
        lst->chunks = (int32_t)c[2];
        lst->groups = (int32_t)c[3];
        lst->light_levels = (int32_t)D.lrefit.level_first.size() - 1;
    }
    return MCPT_OK;
}
// the numbers of a call with `lights` light triangles in its range, before any device state has added its own:
// chunks and groups counted on the host (a scene with device states takes the first state's counters instead)
static mcpt_light_update_stats light_stats_host(const mcpt_scene* sc, int32_t first, int32_t count) {
    mcpt_light_update_stats st;
    mcpt_light_update_stats_init(&st);
    const HostScene& hs = sc->host;
    std::vector<uint8_t> ch(prep_chunks(hs.NL), 0), gr(std::max<size_t>(hs.group_start.size(), 1), 0);
    for (int f = first; f < first + count; f++) {
        const int l = hs.light_of[f];
        if (l < 0) continue;
        st.lights++;
        ch[l >> 6] = 1;
        // the last group that starts at or before l (groups without triangles share a start with their successor)
        const auto g = std::upper_bound(hs.group_start.begin(), hs.group_start.end(), l) - hs.group_start.begin();
        if (g > 0) gr[(size_t)g - 1] = 1;
    }
    for (uint8_t b : ch) st.chunks += b;
    for (uint8_t b : gr) st.groups += b;
    return st;
}

// one state of an update or transform once ev0 is recorded on its stream and its staging arrays hold the range (the
// current device is D's): the refit up to ev1, the light stage, the synchronisation, the state's constants and, from
// the first state of the call, the call's numbers
static int refit_state(mcpt_scene* sc, DeviceState& D, int32_t first, int32_t count, const float* sp, const float* sn,
                       mcpt_update_stats& st, mcpt_light_update_stats& lst) {
    int rc;
    if ((rc = refit_enqueue(D.refit.dev, D.refit.level_first.data(), (int)D.refit.level_first.size() - 1, first, count, sp, sn, sc->margin,
                            D.stream)))
        return rc;
    HIP_OK(hipEventRecord(D.ev1, D.stream));
    if (lst.lights && (rc = light_stage_enqueue(sc, D, first, count))) return rc;
    HIP_OK(hipStreamSynchronize(D.stream));
    if (lst.lights && (rc = light_stage_finish(D, st.device_states == 0 ? &lst : nullptr))) return rc;
    if (st.device_states++ == 0) {
        float ms = 0;
        unsigned n = 0;
        HIP_OK(hipEventElapsedTime(&ms, D.ev0, D.ev1));
        HIP_OK(hipMemcpy(&n, D.refit.dev.counters + 1, sizeof n, hipMemcpyDeviceToHost));
        st.device_seconds = 1e-3 * ms;
        st.nodes_refit = n;
        st.levels = (int32_t)D.refit.level_first.size() - 1;
    }
    return MCPT_OK;
}

// the call after its refusals: the host scene first (it stays the truth for device states made later, for the grid
// and for the debug checks), then every device state the scene has.  src_device >= 0: dpos / dnrm are device memory
// there and that device's state reads them directly; every other state gets a staging copy of the host arrays.
static int update_apply(mcpt_scene* sc, int32_t first, int32_t count, const float* pos, const float* nrm, int src_device,
                        const float* dpos, const float* dnrm, mcpt_update_stats* stats) {
    HostScene& hs = sc->host;
    ensure_slot_map(sc, false);  // first update of the handle: the facet -> leaf-slot map and the binary tree's index
    std::copy(pos, pos + 9 * (size_t)count, hs.pos.begin() + 9 * (size_t)first);
    if (nrm) std::copy(nrm, nrm + 9 * (size_t)count, hs.nrm.begin() + 9 * (size_t)first);
    for (int f = first; f < first + count; f++) unique_normal_of_facet(hs, f);
    const std::vector<int32_t> slots(sc->slots.list.begin() + sc->slots.start[first], sc->slots.list.begin() + sc->slots.start[first + count]);
    refit_bvh(sc->bvh, sc->slots.ix, hs, slots, sc->margin);
    // light triangles in the range (mcpt_scene_set_lights_movable): their areas and the light-only tree's boxes
    mcpt_light_update_stats lst = light_stats_host(sc, first, count);
    if (lst.lights) {
        ensure_slot_map(sc, true);
        PendingRanges one;
        one.add(first, count);
        host_refresh_lights(hs, sc->lbvh, sc->lslots.ix, sc->lslots.start, sc->lslots.list, one, sc->margin);
    }
    sc->grid.ok = false;  // rebuilt from the new positions by the next grid-mode call
    sc->updated = true;   // the 8-wide trees are stale from here on (bvh8_refused)
    mcpt_update_stats st;
    mcpt_update_stats_init(&st);
    st.facets = count;
    st.leaf_slots = (int64_t)slots.size();
    const std::vector<DeviceState*> devs = device_states(sc);
    DeviceRestore back;
    if (!devs.empty()) HIP_OK(hipGetDevice(&back.device));
    for (DeviceState* D : devs) {
        HIP_OK(hipSetDevice(D->device));
        int rc;
        if ((rc = ensure_refit_state(sc, *D)) || (lst.lights && (rc = ensure_light_state(sc, *D)))) return rc;
        const float *sp = dpos, *sn = dnrm;
        if (D->device != src_device) {
            if ((rc = ensure(D->up_pos, 36ull * count)) || (nrm && (rc = ensure(D->up_nrm, 36ull * count)))) return rc;
            HIP_OK(hipMemcpy(D->up_pos.p, pos, 36ull * count, hipMemcpyHostToDevice));
            if (nrm) HIP_OK(hipMemcpy(D->up_nrm.p, nrm, 36ull * count, hipMemcpyHostToDevice));
            sp = (const float*)D->up_pos.p;
            sn = nrm ? (const float*)D->up_nrm.p : nullptr;
        }
        // work of other streams (the caller's, a frame sequence's) that still reads or writes these arrays
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipEventRecord(D->ev0, D->stream));
        if ((rc = refit_state(sc, *D, first, count, sp, sn, st, lst))) return rc;
    }
    sc->light_stats = lst;
    if (stats) *stats = st;
    return MCPT_OK;
}

// the switch's extra refusal on host arrays: the first degenerate light triangle of the range is named
static int update_check_light_values(const mcpt_scene* sc, int32_t first, int32_t count, const float* pos,
                                     const char* who = "mcpt_scene_update") {
    if (!sc->lights_movable) return MCPT_OK;
    const int f = first_degenerate_light(sc->host, first, count, pos);
    if (f < 0) return MCPT_OK;
    set_error("%s: light triangle %d (light %d) would be degenerate: |(b - a) x (c - a)| is zero or not finite, so it "
              "has no unique normal", who, f, sc->host.light_of[f]);
    return MCPT_E_INVALID;
}

int mcpt_scene_update(mcpt_scene* sc, int32_t first, int32_t count, const float* pos, const float* nrm, mcpt_update_stats* stats) {
    int rc;
    if ((rc = update_check_args(sc, first, count, pos, stats))) return rc;
    std::lock_guard<std::mutex> lk(sc->mu);
    if ((rc = update_check_lights(sc, first, count)) || (rc = update_check_values(sc, first, count, pos, nrm)) ||
        (rc = update_check_light_values(sc, first, count, pos)))
        return rc;
    if ((rc = host_sync(sc))) return rc;  // the host refit reads every triangle of a touched leaf
    return update_apply(sc, first, count, pos, nrm, -1, nullptr, nullptr, stats);
}

// mcpt_scene_update_device's value checks on `device` (current): the offenders of the range counted into one word
// on the device -- non-finite values, positions outside the arena and, with `lights`, light triangles that would be
// degenerate (against the range's rows of light_of) -- and read back before anything is modified
static int update_device_count_bad(const mcpt_scene* sc, int32_t first, int32_t count, const float* dpos, const float* dnrm, bool lights,
                                   unsigned* bad) {
    int rc;
    DevBuf word, lof;
    if ((rc = ensure(word, 64))) return rc;
    RefitDev v{};
    v.counters = (unsigned*)word.p;
    double lo[3], hi[3];
    update_arena(sc, lo, hi);
    if ((rc = refit_validate_enqueue(v, count, dpos, dnrm, lo, hi, nullptr))) return rc;
    if (lights) {
        if ((rc = ensure(lof, 4ull * count))) return rc;
        HIP_OK(hipMemcpy(lof.p, sc->host.light_of.data() + first, 4ull * count, hipMemcpyHostToDevice));
        if ((rc = light_validate_enqueue(count, dpos, (const int32_t*)lof.p, v.counters, nullptr))) return rc;
    }
    HIP_OK(hipMemcpy(bad, word.p, sizeof *bad, hipMemcpyDeviceToHost));
    return MCPT_OK;
}

int mcpt_scene_update_device(mcpt_scene* sc, int32_t device, int32_t first, int32_t count, const float* dpos, const float* dnrm,
                             mcpt_update_stats* stats) {
    int rc;
    if ((rc = update_check_args(sc, first, count, dpos, stats))) return rc;
    std::lock_guard<std::mutex> lk(sc->mu);
    if ((rc = update_check_lights(sc, first, count))) return rc;
    if ((rc = host_sync(sc))) return rc;  // as mcpt_scene_update
    DeviceRestore back;
    HIP_OK(hipGetDevice(&back.device));
    if (device < 0) device = back.device;
    if ((rc = check_device_buffer(dpos, device, "dev_positions")) || (dnrm && (rc = check_device_buffer(dnrm, device, "dev_normals"))))
        return rc;
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipDeviceSynchronize());  // the caller's streams may still be writing the arrays
    const bool lights = sc->lights_movable && range_has_light(sc, first, first + count);
    unsigned bad = 0;
    if ((rc = update_device_count_bad(sc, first, count, dpos, dnrm, lights, &bad))) return rc;
    if (bad) {
        set_error("mcpt_scene_update_device: %u values of the range are non-finite or positions outside the arena (the "
                  "build's box grown by its largest extent)%s", bad, lights ? ", or light triangles that would be degenerate" : "");
        return MCPT_E_INVALID;
    }
    std::vector<float> hp(9 * (size_t)count), hn(dnrm ? 9 * (size_t)count : 0);
    HIP_OK(hipMemcpy(hp.data(), dpos, 36ull * count, hipMemcpyDeviceToHost));
    if (dnrm) HIP_OK(hipMemcpy(hn.data(), dnrm, 36ull * count, hipMemcpyDeviceToHost));
    HIP_OK(hipSetDevice(back.device));
    return update_apply(sc, first, count, hp.data(), dnrm ? hn.data() : nullptr, device, dpos, dnrm, stats);
}

// ---- movable light triangles (include/mcpt.h; the kernels are light_tables.hip's) ----
int mcpt_scene_set_lights_movable(mcpt_scene* sc, int32_t on) {
    if (int rn = refuse_null("mcpt_scene_set_lights_movable", sc)) return rn;
    std::lock_guard<std::mutex> lk(sc->mu);
    sc->lights_movable = on != 0;
    return MCPT_OK;
}
int mcpt_scene_lights_movable(const mcpt_scene* sc, int32_t* on) {
    if (int rn = refuse_null("mcpt_scene_lights_movable", sc, on, "on")) return rn;
    mcpt_scene* w = const_cast<mcpt_scene*>(sc);
    std::lock_guard<std::mutex> lk(w->mu);
    *on = sc->lights_movable ? 1 : 0;
    return MCPT_OK;
}
void mcpt_light_update_stats_init(mcpt_light_update_stats* st) { stats_init(st); }
int mcpt_scene_light_update_info(const mcpt_scene* sc, mcpt_light_update_stats* out) {
    if (int rn = refuse_null("mcpt_scene_light_update_info", sc, out, "out")) return rn;
    if (int rc = check_struct_size(out, "mcpt_light_update_stats")) return rc;
    mcpt_scene* w = const_cast<mcpt_scene*>(sc);
    std::lock_guard<std::mutex> lk(w->mu);
    *out = sc->light_stats;
    out->struct_size = sizeof *out;
    return MCPT_OK;
}

// ---- in-place re-lighting (include/mcpt.h; the kernels are light_tables.hip's) ----
void mcpt_relight_stats_init(mcpt_relight_stats* st) { stats_init(st); }

// the refusals of the three setters that need no values: `n` rows of `what`, and the call's array
static int relight_check_args(const char* who, const mcpt_scene* sc, int32_t first, int32_t count, int32_t n, const char* what,
                              const void* data, const char* data_name, const mcpt_relight_stats* stats) {
    if (int rn = refuse_null(who, sc)) return rn;
    if (count < 0 || first < 0 || (int64_t)first + count > n) {
        set_error("%s: %s [%d, %lld) are not a range of the scene's %d", who, what, first, (long long)first + count, n);
        return MCPT_E_INVALID;
    }
    if (count > 0 && !data) {
        set_error("%s: NULL %s", who, data_name);
        return MCPT_E_INVALID;
    }
    return check_struct_size(stats, "mcpt_relight_stats");
}
static bool relight_value_ok(double v) { return v >= 0 && std::isfinite(v); }

// a state's events for a stage that needs no light tables (mcpt_scene_set_materials on a scene without lights)
static int ensure_light_events(DeviceState& D) {
    if (!D.evl0) HIP_OK(hipEventCreate(&D.evl0));
    if (!D.evl1) HIP_OK(hipEventCreate(&D.evl1));
    return MCPT_OK;
}

// mcpt_scene_set_light_radiance after its refusals: the host copy first (it stays the truth for device states made
// later), then every device state.  src_device >= 0: drgb is device memory there and that device's state reads it
// directly; every other state gets a staging copy of rgb.
static int relight_apply(mcpt_scene* sc, int32_t first, int32_t count, const double* rgb, int src_device, const double* drgb,
                         mcpt_relight_stats* stats) {
    HostScene& hs = sc->host;
    mcpt_relight_stats st;
    mcpt_relight_stats_init(&st);
    st.lights = count;
    st.chunks = (first + count - 1) / 64 - first / 64 + 1;
    std::copy(rgb, rgb + 3 * (size_t)count, hs.light_rad.begin() + 3 * (size_t)first);
    for (int l = first; l < first + count; l++) hs.light_sum[l] = hs.light_rad[3 * (size_t)l] + hs.light_rad[3 * (size_t)l + 1] + hs.light_rad[3 * (size_t)l + 2];
    for (size_t g = 0; g < hs.group_start.size(); g++)  // a group without triangles keeps the sum it was loaded with
        if (hs.group_count[g] > 0 && hs.group_start[g] >= first && hs.group_start[g] < first + count) {
            hs.group_rsum[g] = hs.light_sum[hs.group_start[g]];
            st.groups++;
        }
    const std::vector<DeviceState*> devs = device_states(sc);
    DeviceRestore back;
    if (!devs.empty()) HIP_OK(hipGetDevice(&back.device));
    for (DeviceState* D : devs) {
        HIP_OK(hipSetDevice(D->device));
        int rc;
        if ((rc = ensure_light_tables(sc, *D))) return rc;
        const double* src = drgb;
        if (D->device != src_device) {
            if ((rc = ensure(D->up_rad, 24ull * count))) return rc;
            HIP_OK(hipMemcpy(D->up_rad.p, rgb, 24ull * count, hipMemcpyHostToDevice));
            src = (const double*)D->up_rad.p;
        }
        // work of other streams (the caller's, a frame sequence's) that still reads these tables
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipEventRecord(D->evl0, D->stream));
        if ((rc = light_radiance_enqueue(D->ltab, first, count, src, st.groups > 0, D->stream))) return rc;
        HIP_OK(hipEventRecord(D->evl1, D->stream));
        HIP_OK(hipMemcpyAsync(D->pinned_globals, D->ltab.globals, sizeof(LightGlobals), hipMemcpyDeviceToHost, D->stream));
        HIP_OK(hipStreamSynchronize(D->stream));
        if ((rc = light_stage_finish(*D, nullptr))) return rc;  // the state's by-value constants: band_S, band_K
        if (st.device_states++ == 0) {
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, D->evl0, D->evl1));
            st.device_seconds = 1e-3 * ms;
        }
    }
    if (stats) *stats = st;
    return MCPT_OK;
}

int mcpt_scene_set_light_radiance(mcpt_scene* sc, int32_t first, int32_t count, const double* rgb, mcpt_relight_stats* stats) {
    static const char* who = "mcpt_scene_set_light_radiance";
    if (int rc = relight_check_args(who, sc, first, count, sc ? sc->host.NL : 0, "lights", rgb, "rgb", stats)) return rc;
    std::lock_guard<std::mutex> lk(sc->mu);
    for (size_t i = 0; i < 3 * (size_t)count; i++)
        if (!relight_value_ok(rgb[i])) {
            set_error("%s: light %d has a negative or non-finite radiance (component %d: %g)", who, first + (int)(i / 3), (int)(i % 3), rgb[i]);
            return MCPT_E_INVALID;
        }
    if (count == 0) {
        stats_init(stats);
        return MCPT_OK;
    }
    return relight_apply(sc, first, count, rgb, -1, nullptr, stats);
}

int mcpt_scene_set_light_radiance_device(mcpt_scene* sc, int32_t device, int32_t first, int32_t count, const void* drgb,
                                         mcpt_relight_stats* stats) {
    static const char* who = "mcpt_scene_set_light_radiance_device";
    int rc;
    if ((rc = relight_check_args(who, sc, first, count, sc ? sc->host.NL : 0, "lights", drgb, "dev_rgb", stats))) return rc;
    std::lock_guard<std::mutex> lk(sc->mu);
    if (count == 0) {
        stats_init(stats);
        return MCPT_OK;
    }
    DeviceRestore back;
    HIP_OK(hipGetDevice(&back.device));
    if (device < 0) device = back.device;
    if ((rc = check_device_buffer(drgb, device, "dev_rgb"))) return rc;
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipDeviceSynchronize());  // the caller's streams may still be writing the array
    // the offenders counted into one word before anything is modified, as mcpt_scene_update_device counts its own
    DevBuf word;
    unsigned bad = 0;
    if ((rc = ensure(word, 64))) return rc;
    HIP_OK(hipMemset(word.p, 0, sizeof(unsigned)));
    if ((rc = light_radiance_validate_enqueue(3 * (int64_t)count, (const double*)drgb, (unsigned*)word.p, nullptr))) return rc;
    HIP_OK(hipMemcpy(&bad, word.p, sizeof bad, hipMemcpyDeviceToHost));
    if (bad) {
        set_error("%s: %u radiance components of lights [%d, %d) are negative or not finite", who, bad, first, first + count);
        return MCPT_E_INVALID;
    }
    std::vector<double> h(3 * (size_t)count);  // the host copy follows by this one copy of the range
    HIP_OK(hipMemcpy(h.data(), drgb, 24ull * count, hipMemcpyDeviceToHost));
    HIP_OK(hipSetDevice(back.device));
    return relight_apply(sc, first, count, h.data(), device, (const double*)drgb, stats);
}

int mcpt_scene_set_materials(mcpt_scene* sc, int32_t first, int32_t count, const float* mtl, mcpt_relight_stats* stats) {
    static const char* who = "mcpt_scene_set_materials";
    if (int rc = relight_check_args(who, sc, first, count, sc ? sc->host.M : 0, "materials", mtl, "mtl", stats)) return rc;
    std::lock_guard<std::mutex> lk(sc->mu);
    for (size_t i = 0; i < 7 * (size_t)count; i++)
        if (!relight_value_ok(mtl[i])) {
            const int c = (int)(i % 7);
            set_error("%s: material %d has a negative or non-finite %s (%g)", who, first + (int)(i / 7), c < 3 ? "Kd" : c < 6 ? "Ks" : "Ns",
                      (double)mtl[i]);
            return MCPT_E_INVALID;
        }
    mcpt_relight_stats st;
    mcpt_relight_stats_init(&st);
    if (count > 0) {
        HostScene& hs = sc->host;
        st.materials = count;
        std::copy(mtl, mtl + 7 * (size_t)count, hs.mtl.begin() + 7 * (size_t)first);
        const std::vector<DeviceState*> devs = device_states(sc);
        DeviceRestore back;
        if (!devs.empty()) HIP_OK(hipGetDevice(&back.device));
        for (DeviceState* D : devs) {
            HIP_OK(hipSetDevice(D->device));
            if (int rc = ensure_light_events(*D)) return rc;
            HIP_OK(hipDeviceSynchronize());  // work of other streams that still reads the table
            HIP_OK(hipEventRecord(D->evl0, D->stream));
            // from the host copy, which outlives the copy (the stream is synchronised below)
            HIP_OK(hipMemcpyAsync(const_cast<float*>(D->d.mtl) + 7 * (size_t)first, hs.mtl.data() + 7 * (size_t)first, 28ull * count,
                                  hipMemcpyHostToDevice, D->stream));
            HIP_OK(hipEventRecord(D->evl1, D->stream));
            HIP_OK(hipStreamSynchronize(D->stream));
            if (st.device_states++ == 0) {
                float ms = 0;
                HIP_OK(hipEventElapsedTime(&ms, D->evl0, D->evl1));
                st.device_seconds = 1e-3 * ms;
            }
        }
    }
    if (stats) *stats = st;
    return MCPT_OK;
}

int mcpt_scene_light_groups(const mcpt_scene* sc, int32_t* group) {
    if (int rn = refuse_null("mcpt_scene_light_groups", sc, group, "group")) return rn;
    mcpt_scene* w = const_cast<mcpt_scene*>(sc);
    std::lock_guard<std::mutex> lk(w->mu);
    const HostScene& hs = sc->host;
    for (size_t g = 0; g < hs.group_start.size(); g++)
        for (int l = hs.group_start[g]; l < hs.group_start[g] + hs.group_count[g]; l++) group[l] = (int32_t)g;
    return MCPT_OK;
}

// ---- mcpt_scene_pose_save (include/mcpt.h) ----
// the device half of mcpt_scene_pose_save and mcpt_scene_rest_save: every state's d.tri_v / d.tri_n copied into the two
// buffers of the state the call names
static int save_on_devices(mcpt_scene* sc, DevBuf DeviceState::*dst_v, DevBuf DeviceState::*dst_n) {
    const std::vector<DeviceState*> devs = device_states(sc);
    if (devs.empty()) return MCPT_OK;
    DeviceRestore back;
    HIP_OK(hipGetDevice(&back.device));
    for (DeviceState* D : devs) {
        HIP_OK(hipSetDevice(D->device));
        DevBuf &v = D->*dst_v, &n = D->*dst_n;
        const size_t vb = 3 * (size_t)std::max(D->d.F, 1) * sizeof(float4), nb = 9 * (size_t)D->d.F * sizeof(float);
        int rc;
        if ((rc = ensure(v, vb)) || (rc = ensure(n, std::max<size_t>(nb, 4)))) return rc;
        // device to device on the state's stream: ordered after the refits (mcpt_scene_update) and before the motion
        // AOVs, which run there too
        HIP_OK(hipMemcpyAsync(v.p, D->d.tri_v, vb, hipMemcpyDeviceToDevice, D->stream));
        if (nb) HIP_OK(hipMemcpyAsync(n.p, D->d.tri_n, nb, hipMemcpyDeviceToDevice, D->stream));
        HIP_OK(hipStreamSynchronize(D->stream));
    }
    return MCPT_OK;
}
int mcpt_scene_pose_save(mcpt_scene* sc) {
    if (int rn = refuse_null("mcpt_scene_pose_save", sc)) return rn;
    std::lock_guard<std::mutex> lk(sc->mu);
    if (std::lock_guard<std::mutex> hl(sc->host_mu); sc->pending.r.empty()) {
        sc->prev_pos = sc->host.pos;
        sc->prev_nrm = sc->host.nrm;
        sc->prev_stale = false;
    } else {
        // the host copy is behind the devices (mcpt_scene_transform) and a frame loop must not pay for a sync here:
        // the device copies below are the pose, and host_sync refreshes prev_pos / prev_nrm from the first state's
        sc->prev_stale = true;
    }
    sc->pose_saved = true;
    return save_on_devices(sc, &DeviceState::prev_v, &DeviceState::prev_n);
}

// ---- mcpt_scene_rest_save, mcpt_scene_transform and the lazily synced host copy (include/mcpt.h, DESIGN.md §4.21;
// the kernel is refit.hip's, the host arithmetic and the pending ranges host_mirror.cpp's) ----
int mcpt_scene_rest_save(mcpt_scene* sc) {
    if (int rn = refuse_null("mcpt_scene_rest_save", sc)) return rn;
    std::lock_guard<std::mutex> lk(sc->mu);
    int rc;
    if ((rc = host_sync(sc))) return rc;
    sc->rest_pos = sc->host.pos;
    sc->rest_nrm = sc->host.nrm;
    sc->rest_saved = true;
    return save_on_devices(sc, &DeviceState::rest_v, &DeviceState::rest_n);
}

// the call after the refusals that need no values, on a scene with device states: every state transforms the range
// from its own rest copy into its staging arrays and counts the offenders; the counts are read back before anything
// is modified; then refit_enqueue as for an update.  The host copy only gets the range marked as behind.
static int transform_on_devices(mcpt_scene* sc, const std::vector<DeviceState*>& devs, int32_t first, int32_t count,
                                const double m[12], const double n[9], mcpt_update_stats* stats) {
    ensure_slot_map(sc, false);
    mcpt_update_stats st;
    mcpt_update_stats_init(&st);
    st.facets = count;
    st.leaf_slots = (int64_t)sc->slots.start[first + count] - sc->slots.start[first];
    mcpt_light_update_stats lst = light_stats_host(sc, first, count);
    double lo[3], hi[3];
    update_arena(sc, lo, hi);
    int rc;
    DeviceRestore back;
    HIP_OK(hipGetDevice(&back.device));
    std::vector<unsigned> bad(devs.size(), 0);
    for (size_t i = 0; i < devs.size(); i++) {
        DeviceState* D = devs[i];
        HIP_OK(hipSetDevice(D->device));
        if ((rc = ensure_refit_state(sc, *D)) || (rc = ensure(D->up_pos, 36ull * count)) || (rc = ensure(D->up_nrm, 36ull * count)) ||
            (lst.lights && (rc = ensure_light_state(sc, *D))))
            return rc;
        if (!D->rest_v.p || !D->rest_n.p) {
            set_error("mcpt_scene_transform: device %d holds no rest pose", D->device);
            return MCPT_E_DEVICE;
        }
        // work of other streams (the caller's, a frame sequence's) that still reads or writes these arrays
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipEventRecord(D->ev0, D->stream));
        if ((rc = transform_enqueue(D->refit.dev, (const float*)D->rest_v.p, (const float*)D->rest_n.p, first, count, m, n, lo, hi,
                                    (float*)D->up_pos.p, (float*)D->up_nrm.p, D->stream)))
            return rc;
        // degenerate light triangles of the staged range count into the same word
        if (lst.lights && (rc = light_validate_enqueue(count, (const float*)D->up_pos.p, D->d.tri_light + first, D->refit.dev.counters, D->stream)))
            return rc;
        HIP_OK(hipMemcpyAsync(&bad[i], D->refit.dev.counters, sizeof(unsigned), hipMemcpyDeviceToHost, D->stream));
    }
    unsigned nbad = 0;
    for (size_t i = 0; i < devs.size(); i++) {
        HIP_OK(hipSetDevice(devs[i]->device));
        HIP_OK(hipStreamSynchronize(devs[i]->stream));
        nbad = std::max(nbad, bad[i]);
    }
    if (nbad) {  // only the staging arrays were written
        set_error("mcpt_scene_transform: %u transformed values of facets [%d, %d) are non-finite or positions outside the "
                  "arena (the build's box grown by its largest extent)%s", nbad, first, first + count,
                  lst.lights ? ", or light triangles that would be degenerate" : "");
        return MCPT_E_INVALID;
    }
    // the devices are modified from here on, so the marks come first: should a launch below fail, the host copy is
    // still known to be behind (host.pos / host.nrm / host.unique_n and the binary tree follow at the next host_sync)
    {
        std::lock_guard<std::mutex> hl(sc->host_mu);
        sc->pending.add(first, count);
    }
    sc->grid.ok = false;  // stale from here on, as after an update
    sc->updated = true;   // the 8-wide trees are stale from here on (bvh8_refused)
    for (DeviceState* D : devs) {
        HIP_OK(hipSetDevice(D->device));
        if ((rc = refit_state(sc, *D, first, count, (const float*)D->up_pos.p, (const float*)D->up_nrm.p, st, lst))) return rc;
    }
    sc->light_stats = lst;
    if (stats) *stats = st;
    return MCPT_OK;
}

int mcpt_scene_transform(mcpt_scene* sc, int32_t first, int32_t count, const double m[12], const double normal_m[9],
                         mcpt_update_stats* stats) {
    static const char* who = "mcpt_scene_transform";
    int rc;
    if ((rc = update_check_args(sc, first, count, m, stats, who, "m"))) return rc;
    std::lock_guard<std::mutex> lk(sc->mu);
    if ((rc = update_check_lights(sc, first, count, who))) return rc;
    double n[9];
    for (int i = 0; i < 12; i++)
        if (!std::isfinite(m[i])) {
            set_error("%s: m[%d] is not finite", who, i);
            return MCPT_E_INVALID;
        }
    for (int i = 0; i < 9; i++) {
        n[i] = normal_m ? normal_m[i] : m[4 * (i / 3) + i % 3];
        if (!std::isfinite(n[i])) {
            set_error("%s: normal_m[%d] is not finite", who, i);
            return MCPT_E_INVALID;
        }
    }
    if (!sc->rest_saved) {
        set_error("%s: the scene has no rest pose yet (call mcpt_scene_rest_save first)", who);
        return MCPT_E_INVALID;
    }
    const std::vector<DeviceState*> devs = device_states(sc);
    if (!devs.empty()) return transform_on_devices(sc, devs, first, count, m, n, stats);
    // no device state yet: the rule on the host, then an ordinary update (nothing is left pending)
    std::vector<float> pos(9 * (size_t)count), nrm(9 * (size_t)count);
    transform_facets(sc->rest_pos.data() + 9 * (size_t)first, sc->rest_nrm.data() + 9 * (size_t)first, (size_t)count, m, n, pos.data(),
                     nrm.data());
    if ((rc = update_check_values(sc, first, count, pos.data(), nrm.data(), who)) ||
        (rc = update_check_light_values(sc, first, count, pos.data(), who)))
        return rc;
    return update_apply(sc, first, count, pos.data(), nrm.data(), -1, nullptr, nullptr, stats);
}

int mcpt_scene_host_pending(const mcpt_scene* sc, int64_t* facets) {
    if (int rn = refuse_null("mcpt_scene_host_pending", sc, facets, "facets")) return rn;
    mcpt_scene* w = const_cast<mcpt_scene*>(sc);
    std::lock_guard<std::mutex> lk(w->mu);
    std::lock_guard<std::mutex> hl(w->host_mu);
    *facets = sc->pending.facets();
    return MCPT_OK;
}

int mcpt_scene_host_sync(mcpt_scene* sc) {
    if (int rn = refuse_null("mcpt_scene_host_sync", sc)) return rn;
    std::lock_guard<std::mutex> lk(sc->mu);
    return host_sync(sc);
}

// ---- mcpt_scene_set_visible and mcpt_scene_visibility (include/mcpt.h; the kernel is refit.hip's) ----
int mcpt_scene_set_visible(mcpt_scene* sc, int32_t first, int32_t count, int32_t visible, mcpt_update_stats* stats) {
    static const char* who = "mcpt_scene_set_visible";
    int rc;
    if ((rc = refuse_null(who, sc))) return rc;
    if (count < 1 || first < 0 || (int64_t)first + count > sc->host.F) {
        set_error("%s: facets [%d, %lld) are not a non-empty range of the scene's %d facets", who, first, (long long)first + count,
                  sc->host.F);
        return MCPT_E_INVALID;
    }
    if ((rc = check_struct_size(stats, "mcpt_update_stats"))) return rc;
    std::lock_guard<std::mutex> lk(sc->mu);
    HostScene& hs = sc->host;
    for (int f = first; f < first + count; f++)
        if (hs.light_of[f] >= 0) {
            set_error("%s: facet %d is a light triangle (light %d); lights cannot be hidden (mcpt_scene_set_light_radiance "
                      "with zeros switches one off)", who, f, hs.light_of[f]);
            return MCPT_E_INVALID;
        }
    if ((rc = host_sync(sc))) return rc;  // the host refit reads every triangle of a touched leaf
    ensure_slot_map(sc, false);
    if (hs.hidden.empty()) hs.hidden.assign((size_t)hs.F, 0);
    // every state's mask and refit state while the host's bytes are still the ones its slots were written under
    const std::vector<DeviceState*> devs = device_states(sc);
    DeviceRestore back;
    if (!devs.empty()) HIP_OK(hipGetDevice(&back.device));
    for (DeviceState* D : devs) {
        HIP_OK(hipSetDevice(D->device));
        if ((rc = ensure_refit_state(sc, *D)) || (rc = ensure_hidden_state(sc, *D))) return rc;
    }
    // the host copy first: it stays the truth for device states made later and for the debug checks
    const uint8_t hide = visible ? 0 : 1;
    for (int f = first; f < first + count; f++) {
        sc->hidden_count += (int32_t)hide - (int32_t)hs.hidden[f];
        hs.hidden[f] = hide;
    }
    const std::vector<int32_t> slots(sc->slots.list.begin() + sc->slots.start[first], sc->slots.list.begin() + sc->slots.start[first + count]);
    refit_bvh(sc->bvh, sc->slots.ix, hs, slots, sc->margin);
    sc->grid.ok = false;  // refused while anything is hidden, rebuilt by the next grid-mode call after that
    sc->updated = true;   // the 8-wide trees are stale from here on (bvh8_refused)
    mcpt_update_stats st;
    mcpt_update_stats_init(&st);
    st.facets = count;
    st.leaf_slots = (int64_t)slots.size();
    for (DeviceState* D : devs) {
        HIP_OK(hipSetDevice(D->device));
        // work of other streams (the caller's, a frame sequence's) that still reads these arrays
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipEventRecord(D->ev0, D->stream));
        if ((rc = visibility_enqueue(D->refit.dev, D->refit.level_first.data(), (int)D->refit.level_first.size() - 1, first, count, visible,
                                     sc->margin, D->stream)))
            return rc;
        HIP_OK(hipEventRecord(D->ev1, D->stream));
        HIP_OK(hipStreamSynchronize(D->stream));
        if (st.device_states++ == 0) {
            float ms = 0;
            unsigned n = 0;
            HIP_OK(hipEventElapsedTime(&ms, D->ev0, D->ev1));
            HIP_OK(hipMemcpy(&n, D->refit.dev.counters + 1, sizeof n, hipMemcpyDeviceToHost));
            st.device_seconds = 1e-3 * ms;
            st.nodes_refit = n;
            st.levels = (int32_t)D->refit.level_first.size() - 1;
        }
    }
    if (stats) *stats = st;
    return MCPT_OK;
}

int mcpt_scene_visibility(const mcpt_scene* sc, uint8_t* visible, int32_t* hidden) {
    if (int rn = refuse_null("mcpt_scene_visibility", sc)) return rn;
    mcpt_scene* w = const_cast<mcpt_scene*>(sc);
    std::lock_guard<std::mutex> lk(w->mu);
    if (visible)
        for (int f = 0; f < sc->host.F; f++) visible[f] = sc->host.is_hidden(f) ? 0 : 1;
    if (hidden) *hidden = sc->hidden_count;
    return MCPT_OK;
}

// ---- mcpt_scene_rebuild and mcpt_scene_tree_cost (include/mcpt.h; the kernels are rebuild.hip's) ----
void mcpt_rebuild_stats_init(mcpt_rebuild_stats* st) { stats_init(st); }

// the cost of the main tree `D` holds, on its stream (the current device is D's)
static int tree_cost_of(DeviceState& D, double* cost) {
    int rc;
    if ((rc = ensure(D.cost_words, kTreeCostWords * sizeof(double)))) return rc;
    double* res = nullptr;
    if ((rc = tree_cost_enqueue(D.d.bvh4, D.d.nbvh4, (double*)D.cost_words.p, D.stream, &res))) return rc;
    HIP_OK(hipMemcpyAsync(cost, res, sizeof(double), hipMemcpyDeviceToHost, D.stream));
    HIP_OK(hipStreamSynchronize(D.stream));
    return MCPT_OK;
}

// one device state (the current device is D's): the new tree is built into the set of arrays the state is not using,
// checked, and only then do the state's pointers change -- together
static int rebuild_state(mcpt_scene* sc, DeviceState& D, mcpt_rebuild_stats* st) {
    const size_t F = (size_t)D.d.F;
    int rc;
    if (!D.rb_work && (rc = rebuild_work_create(D.d.F, &D.rb_work))) return rc;
    for (DeviceState::RebuildSet& B : D.rb_set)  // both sets at the first rebuild: nothing grows from call to call
        if ((rc = ensure(B.bvh4, F * sizeof(BvhNode4))) || (rc = ensure(B.bvh4q, F * sizeof(BvhNode4Q))) ||
            (rc = ensure(B.leaf_v, 3 * F * sizeof(float4))) || (rc = ensure(B.slot_list, F * sizeof(int32_t))) ||
            (rc = ensure(B.slot_dirty, F)) || (rc = ensure(B.node_dirty, F)))
            return rc;
    if ((rc = ensure(D.rb_slot_start, (F + 1) * sizeof(int32_t))) || (rc = ensure(D.rb_counters, 16 * sizeof(unsigned)))) return rc;
    DeviceState::RebuildSet& S = D.rb_set[D.rb_next];
    RefitDev r{};
    r.F = r.nslots = D.d.F;
    r.tri_v = const_cast<float*>(reinterpret_cast<const float*>(D.d.tri_v));
    r.tri_n = const_cast<float*>(D.d.tri_n);
    r.leaf_v = (float*)S.leaf_v.p;
    r.bvh4 = (BvhNode4*)S.bvh4.p;
    r.bvh4q = (BvhNode4Q*)S.bvh4q.p;
    r.slot_start = (const int32_t*)D.rb_slot_start.p;
    r.slot_list = (const int32_t*)S.slot_list.p;
    r.slot_dirty = (uint8_t*)S.slot_dirty.p;
    r.node_dirty = (uint8_t*)S.node_dirty.p;
    r.counters = (unsigned*)D.rb_counters.p;
    // hidden facets stay in the tree, at their points with collapsed slots; both sets carry the mask
    if ((rc = ensure_hidden_state(sc, D))) return rc;
    r.hidden = (uint8_t*)D.hidden.p;
    // work of other streams (the caller's, a frame sequence's) that still reads the arrays of the set built two
    // rebuilds ago, or writes tri_v
    HIP_OK(hipDeviceSynchronize());
    if (st && (rc = tree_cost_of(D, &st->cost_before))) return rc;
    std::vector<int32_t> lf;
    int32_t need = 0;
    HIP_OK(hipEventRecord(D.ev0, D.stream));
    const int leaf_max = g_rebuild_leaf_max.load() ? g_rebuild_leaf_max.load() : kRebuildLeafMax;
    if ((rc = rebuild_build(D.rb_work, &r, leaf_max, kStack, sc->margin, D.stream, &lf, &need))) {
        (void)hipStreamSynchronize(D.stream);
        return rc;
    }
    HIP_OK(hipEventRecord(D.ev1, D.stream));
    HIP_OK(hipStreamSynchronize(D.stream));
    D.d.bvh4 = r.bvh4;
    D.d.bvh4q = r.bvh4q;
    D.d.leaf_v = reinterpret_cast<const float4*>(r.leaf_v);
    D.d.nbvh4 = r.nnodes;
    D.nslots = F;
    D.refit.dev = r;
    D.refit.level_first = std::move(lf);
    D.refit.ready = true;
    D.rb_next ^= 1;
    if (st) {
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, D.ev0, D.ev1));
        st->device_seconds = 1e-3 * ms;
        st->nodes = r.nnodes;
        st->levels = (int32_t)D.refit.level_first.size() - 1;
        st->stack_need = need;
        if ((rc = tree_cost_of(D, &st->cost_after))) return rc;
        sc->rebuilt_nodes = (uint64_t)r.nnodes;
        sc->rebuilt_slots = F;
    }
    return MCPT_OK;
}

int mcpt_scene_rebuild(mcpt_scene* sc, mcpt_rebuild_stats* stats) {
    if (int rn = refuse_null("mcpt_scene_rebuild", sc)) return rn;
    if (int rc = check_struct_size(stats, "mcpt_rebuild_stats")) return rc;
    std::lock_guard<std::mutex> lk(sc->mu);
    mcpt_rebuild_stats st;
    mcpt_rebuild_stats_init(&st);
    st.facets = sc->host.F;
    const std::vector<DeviceState*> devs = device_states(sc);
    if (!devs.empty() && sc->host.F > 0) {
        DeviceRestore back;
        HIP_OK(hipGetDevice(&back.device));
        for (DeviceState* D : devs) {
            HIP_OK(hipSetDevice(D->device));
            if (int rc = rebuild_state(sc, *D, st.device_states == 0 ? &st : nullptr)) return rc;
            st.device_states++;
            sc->updated = true;  // the 8-wide trees keep the host tree's topology: refused from here on (bvh8_refused)
        }
    }
    if (stats) *stats = st;
    return MCPT_OK;
}

int mcpt_scene_tree_cost(mcpt_scene* sc, int32_t device, double* cost) {
    if (int rn = refuse_null("mcpt_scene_tree_cost", sc, cost, "cost")) return rn;
    std::lock_guard<std::mutex> lk(sc->mu);
    DeviceRestore back;
    HIP_OK(hipGetDevice(&back.device));
    DeviceState* D;
    int rc;
    if ((rc = get_device_state(sc, device, &D))) return rc;
    return tree_cost_of(*D, cost);
}

}  // extern "C"
