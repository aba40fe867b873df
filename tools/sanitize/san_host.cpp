// Sanitizer driver (host code only, no GPU): built with -fsanitize=address,undefined by
// `make -C monte_carlo_path_tracing_amd/csrc sanitize` together with the library's host sources
// (scene_io.cpp, bvh.cpp, grid.cpp, image.cpp, host_mirror.cpp) and the oracle (oracle/mcpt_oracle.c).
//
// For every (obj, xml) pair on the command line it runs what mcpt_scene_load does on the host --
// Myobj::read / Mylight::read / gather_light_triangles (scene_io.cpp, the reference's Myobj.cpp:10-28,
// Mylight.cpp:11-100) -- then the BVH build, 4-wide collapse and quantisation (bvh.cpp), the
// reference's uniform grid (grid.cpp, Myobj.cpp:78-162), the tone map and BMP writer (image.cpp),
// and the same file through the oracle's loader plus a few oracle queries and a tiny render.  A
// malformed file must come back as an error, never as a sanitizer report.
//
//   san_host OUT_DIR obj1 xml1 [obj2 xml2 ...]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "mcpt_internal.h"

extern "C" {
#include "mcpt_oracle.h"
}

using namespace mcpt;

static int run_library(const char* obj, const char* xml, const std::string& out_dir, int idx) {
    HostScene hs;
    std::vector<LightDef> lights;
    std::string err;
    if (!load_obj_mtl(obj, hs, err) || !load_light_xml(xml, hs, lights, err)) return 1;
    if (!finalize_scene(hs, lights, err)) return 2;
    std::vector<int32_t> all(hs.F), lt(hs.light_facet);
    for (int f = 0; f < hs.F; f++) all[f] = f;
    for (int leaf : {1, 2, 8}) {
        const Bvh b = build_bvh(hs, all, leaf), lb = build_bvh(hs, lt, leaf);
        const std::vector<BvhNode4> b4 = collapse_bvh4(b), lb4 = collapse_bvh4(lb);
        const std::vector<BvhNode4Q> q = quantize_bvh4(b4), lq = quantize_bvh4(lb4);
        if (q.size() != b4.size() || lq.size() != lb4.size()) return 3;
        // the 8-wide trees (leaf 8: binary leaves of up to 8 triangles, split by build_bvh8): every reference of
        // the binary tree once (a facet split spatially -- this build makes spatial splits in every tree -- has
        // several references)
        for (const Bvh* bb : {&b, &lb}) {
            const Bvh8 b8 = build_bvh8(hs, *bb);
            std::vector<int> seen(hs.F, 0), want(hs.F, 0);
            for (int32_t f : bb->leaf_facets)
                if (f >= 0 && f < hs.F) want[f]++;
            size_t used = 0;
            for (int32_t f : b8.tri_facets)
                if (f >= 0) {
                    if (f >= hs.F || ++seen[f] > want[f]) return 6;
                    used++;
                }
            if (used != bb->leaf_facets.size() || b8.nodes.empty()) return 6;
        }
        // mcpt_scene_update's host half: move the slots of three facets (few slots: the sorted list and the heap),
        // then every slot (marks and the sweep), refit the binary tree each time; it must still collapse and quantise
        if (hs.F > 0) {
            Bvh rb = b;
            HostScene moved = hs;
            const BvhRefitIndex ix = make_bvh_refit_index(rb);
            for (int pass = 0; pass < 2; pass++) {
                std::vector<int32_t> slots;
                for (size_t q = 0; q < rb.leaf_facets.size(); q++) {
                    const int f = rb.leaf_facets[q];
                    if (pass == 1 || f == 0 || f == hs.F - 1 || f == hs.F / 2) slots.push_back((int32_t)q);
                }
                for (int32_t q : slots) {
                    const int f = rb.leaf_facets[q];
                    for (int c = 0; c < 9; c++) moved.pos[9 * (size_t)f + c] += 0.25f;
                    unique_normal_of_facet(moved, f);
                }
                refit_bvh(rb, ix, moved, slots, 1e-5);
                const std::vector<BvhNode4> r4 = collapse_bvh4(rb);
                if (quantize_bvh4(r4).size() != r4.size()) return 7;
            }
            // mcpt_scene_transform's host side (host_mirror.cpp): overlapping, touching and many scattered ranges
            // merged into the pending list (past kPendingMax it collapses to the hull), every pending facet rotated
            // from the rest pose by the rule, then the host half of the sync over the list
            PendingRanges pend;
            std::vector<uint8_t> marked(hs.F, 0);  // what was added, kept independently of the list
            auto add = [&](int32_t a, int32_t c) {
                pend.add(a, c);
                for (int32_t g = a; g < a + c; g++) marked[g] = 1;
            };
            for (int32_t s : {0, hs.F / 2, hs.F - 1, 1, hs.F / 2 + 1, hs.F / 3}) add(s, std::min<int32_t>(2, hs.F - s));
            for (int32_t f = 0; f < hs.F && f < 3 * (int32_t)kPendingMax; f += 3) add(f, 1);
            int64_t covered = 0, want = 0;
            const bool hull = pend.r.size() == 1;  // a collapsed list covers more than was added, never less
            for (size_t i = 0; i < pend.r.size(); i++) {
                if (pend.r[i].first < 0 || pend.r[i].second > hs.F || pend.r[i].first >= pend.r[i].second) return 8;
                if (i && pend.r[i - 1].second >= pend.r[i].first) return 8;  // sorted, disjoint, not touching
                covered += pend.r[i].second - pend.r[i].first;
            }
            for (int32_t g = 0; g < hs.F; g++) {
                bool in = false;
                for (const auto& p : pend.r) in = in || (g >= p.first && g < p.second);
                if (marked[g] && !in) return 8;
                if (!hull && in && !marked[g]) return 8;
                want += marked[g];
            }
            if (pend.r.size() > kPendingMax || covered != pend.facets() || covered < want) return 8;
            double m[12];
            const double axis[3] = {0.3, 1.0, -0.2}, pivot[3] = {0.5, 0.25, -1.0}, shift[3] = {0.125, 0.0, -0.25};
            if (mcpt_transform_rotation(axis, 33.0, pivot, shift, m) != MCPT_OK) return 8;
            const double n[9] = {m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]};
            HostScene turned = hs;
            for (const auto& p : pend.r)
                transform_facets(hs.pos.data() + 9 * (size_t)p.first, hs.nrm.data() + 9 * (size_t)p.first, (size_t)(p.second - p.first),
                                 m, n, turned.pos.data() + 9 * (size_t)p.first, turned.nrm.data() + 9 * (size_t)p.first);
            Bvh tb = b;
            std::vector<int32_t> slot_start, slot_list;
            make_facet_slot_map(tb, hs.F, slot_start, slot_list);
            if (host_refresh_ranges(turned, tb, ix, slot_start, slot_list, pend, 1e-5) < covered) return 8;
            const std::vector<BvhNode4> t4 = collapse_bvh4(tb);
            if (quantize_bvh4(t4).size() != t4.size()) return 8;
            if (hs.NL > 0) {  // the light half of such a move: the areas and the light-only tree's refit
                Bvh ltree = lb;
                const BvhRefitIndex lix = make_bvh_refit_index(ltree);
                std::vector<int32_t> lstart, llist;
                make_facet_slot_map(ltree, hs.F, lstart, llist);
                int64_t nl = 0;
                for (const auto& p : pend.r)
                    for (int32_t g = p.first; g < p.second; g++) nl += turned.light_of[g] >= 0;
                if (host_refresh_lights(turned, ltree, lix, lstart, llist, pend, 1e-5) != nl) return 8;
                const int bad = first_degenerate_light(turned, 0, hs.F, turned.pos.data());
                if (bad >= hs.F || (bad >= 0 && turned.light_of[bad] < 0)) return 8;
                const std::vector<BvhNode4> l4 = collapse_bvh4(ltree);
                if (quantize_bvh4(l4).size() != l4.size()) return 8;
            }
        }
    }
    const double eye[3] = {hs.has_cam ? hs.cam.eye[0] : 0.0, hs.has_cam ? hs.cam.eye[1] : 0.0,
                           hs.has_cam ? hs.cam.eye[2] : 0.0};
    if (std::isfinite(eye[0]) && std::isfinite(eye[1]) && std::isfinite(eye[2])) {
        const Grid g = build_grid(hs, eye, 1000);
        (void)g;
    }
    const int W = 7, H = 5;
    std::vector<double> hdr(3 * W * H);
    for (size_t k = 0; k < hdr.size(); k++) hdr[k] = (k % 5 == 0) ? NAN : (k % 7 == 0 ? -1.0 : 0.37 * k);
    std::vector<uint8_t> rgb8(3 * W * H);
    if (mcpt_tone_map(hdr.data(), W, H, 380.0, 0.25, rgb8.data())) return 4;
    const std::string bmp = out_dir + "/san_" + std::to_string(idx) + ".bmp";
    if (mcpt_write_bmp(bmp.c_str(), rgb8.data(), W, H)) return 5;
    std::remove(bmp.c_str());
    return 0;
}

static int run_oracle(const char* obj, const char* xml) {
    orc_scene* s = orc_scene_load(obj, xml);
    if (!s) return 1;
    int F = 0, M = 0, NL = 0;
    orc_scene_counts(s, &F, &M, &NL);
    const double eye[3] = {28.2792, 5.2, 1.23612e-06};
    orc_grid_build(s, eye, 1000);
    double tbg[3];
    for (int k = 0; k < 16; k++) {
        const double ro[3] = {0.1 * k, 1.0, -0.5 * k}, rd[3] = {0.6, -0.48, 0.64};
        (void)orc_closest_hit(s, ro, rd, -1, tbg);
        (void)orc_closest_light_hit(s, ro, rd, -1, tbg);
        const double x1[3] = {0.3 * k, 0.01, 0.2 * k}, n[3] = {0, 1, 0};
        int cnt = 0;
        std::vector<int> idx(NL + 1);
        std::vector<double> w(NL + 1);
        (void)orc_light_prep(s, x1, n, &cnt, idx.data(), w.data());
        double o6[6];
        orc_light_sample_u(s, x1, n, 0.37, 0.5, 0.5, o6);
    }
    if (F > 0 && F < 200000) {  // a tiny counter-RNG render of every integrator
        orc_camera cam;
        std::memset(&cam, 0, sizeof cam);
        if (orc_scene_camera(s, &cam) != 0) {
            const double e[3] = {28.2792, 5.2, 1.23612e-06}, l[3] = {0, 2.8, 0}, u[3] = {0, 1, 0};
            std::memcpy(cam.eye, e, sizeof e);
            std::memcpy(cam.lookat, l, sizeof l);
            std::memcpy(cam.up, u, sizeof u);
            cam.fovy = 20.1143;
            cam.dist_scale = 2.0;
        }
        cam.width = 8;
        cam.height = 6;
        std::vector<double> img(3 * 8 * 6);
        uint64_t stats[4];
        for (int mode = 0; mode < 4; mode++)
            (void)orc_render(s, &cam, mode, 20240430ull, 2, 0, 2, 1, 0, 1, img.data(), stats);
    }
    orc_scene_free(s);
    return 0;
}

// PendingRanges::add on lists that do not depend on any scene: merges of overlapping and touching ranges in any
// order, and the collapse to the hull once more than kPendingMax disjoint ranges are held
static bool check_pending_ranges() {
    using R = std::vector<std::pair<int32_t, int32_t>>;
    PendingRanges p;
    p.add(5, 3);
    p.add(8, 2);  // touches [5, 8)
    if (p.r != R{{5, 10}}) return false;
    p.add(0, 2);
    p.add(20, 4);
    p.add(12, 1);
    if (p.r != R{{0, 2}, {5, 10}, {12, 13}, {20, 24}} || p.facets() != 12) return false;
    p.add(7, 0);  // an empty range is ignored
    p.add(1, 12);  // overlaps the first, swallows the second, touches the third
    if (p.r != R{{0, 13}, {20, 24}} || p.facets() != 17) return false;
    PendingRanges q;
    const int32_t n = (int32_t)kPendingMax;
    for (int32_t i = n - 1; i >= 0; i--) q.add(100 + 10 * i, 1);  // descending: every insertion is at the front
    if (q.r.size() != kPendingMax || q.facets() != n || q.r.front() != std::make_pair(100, 101)) return false;
    q.add(3, 2);  // one more disjoint range: the hull
    if (q.r != R{{3, 100 + 10 * (n - 1) + 1}}) return false;
    q.add(2000, 1);  // and the list grows again from there
    return q.r == R{{3, 100 + 10 * (n - 1) + 1}, {2000, 2001}};
}

int main(int argc, char** argv) {
    if (argc < 4 || (argc - 2) % 2) {
        std::fprintf(stderr, "usage: %s OUT_DIR obj xml [obj xml ...]\n", argv[0]);
        return 2;
    }
    if (!check_pending_ranges()) {
        std::fprintf(stderr, "san_host: PendingRanges::add gives a wrong list\n");
        return 1;
    }
    const std::string out_dir = argv[1];
    int loaded = 0, rejected = 0, oloaded = 0, orejected = 0;
    for (int a = 2; a + 1 < argc; a += 2) {
        const int r = run_library(argv[a], argv[a + 1], out_dir, a);
        (r == 0 ? loaded : rejected)++;
        const int ro = run_oracle(argv[a], argv[a + 1]);
        (ro == 0 ? oloaded : orejected)++;
    }
    std::printf("san_host: %d scene pairs; library loaded %d rejected %d; oracle loaded %d rejected %d; no sanitizer report\n",
                (argc - 2) / 2, loaded, rejected, oloaded, orejected);
    return 0;
}
