// Host side of mcpt_scene_transform (include/mcpt.h), free of HIP so that the sanitizer driver
// (tools/sanitize/san_host.cpp) runs it: the transform rule on host arrays, the list of facet ranges whose host copy
// is behind the devices, the host half of an update over such ranges, and mcpt_transform_rotation.
#include <algorithm>
#include <cmath>

#include "mcpt_internal.h"

namespace mcpt {

// the rule of include/mcpt.h: fp64, no contraction (the tree is built with -ffp-contract=off), in this order
void transform_facets(const float* rest_pos, const float* rest_nrm, size_t count, const double m[12], const double n[9],
                      float* pos, float* nrm) {
    for (size_t v = 0; v < 3 * count; v++) {
        const double x = rest_pos[3 * v], y = rest_pos[3 * v + 1], z = rest_pos[3 * v + 2];
        const double nx = rest_nrm[3 * v], ny = rest_nrm[3 * v + 1], nz = rest_nrm[3 * v + 2];
        for (int r = 0; r < 3; r++) {
            pos[3 * v + r] = static_cast<float>(((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3]);
            nrm[3 * v + r] = static_cast<float>((n[3 * r] * nx + n[3 * r + 1] * ny) + n[3 * r + 2] * nz);
        }
    }
}

void PendingRanges::add(int32_t first, int32_t count) {
    if (count < 1) return;
    int32_t lo = first, hi = first + count;
    // every range that overlaps or touches [lo, hi) is absorbed; the list stays sorted and disjoint
    auto a = std::lower_bound(r.begin(), r.end(), lo, [](const std::pair<int32_t, int32_t>& p, int32_t x) { return p.second < x; });
    auto b = a;
    while (b != r.end() && b->first <= hi) {
        lo = std::min(lo, b->first);
        hi = std::max(hi, b->second);
        ++b;
    }
    a = r.erase(a, b);
    r.insert(a, {lo, hi});
    if (r.size() > kPendingMax) r.assign(1, {r.front().first, r.back().second});  // the hull
}

int64_t PendingRanges::facets() const {
    int64_t n = 0;
    for (const auto& p : r) n += p.second - p.first;
    return n;
}

void make_facet_slot_map(const Bvh& b, int F, std::vector<int32_t>& slot_start, std::vector<int32_t>& slot_list) {
    const std::vector<int32_t>& lfac = b.leaf_facets;
    slot_start.assign(static_cast<size_t>(F) + 1, 0);
    for (int32_t f : lfac) slot_start[f + 1]++;
    for (int f = 0; f < F; f++) slot_start[f + 1] += slot_start[f];
    slot_list.resize(lfac.size());
    std::vector<int32_t> at(slot_start.begin(), slot_start.end() - 1);
    for (size_t q = 0; q < lfac.size(); q++) slot_list[at[lfac[q]]++] = static_cast<int32_t>(q);
}

int64_t host_refresh_ranges(HostScene& s, Bvh& b, const BvhRefitIndex& ix, const std::vector<int32_t>& slot_start,
                            const std::vector<int32_t>& slot_list, const PendingRanges& ranges, double margin) {
    std::vector<int32_t> slots;
    for (const auto& p : ranges.r) {
        for (int f = p.first; f < p.second; f++) unique_normal_of_facet(s, f);
        slots.insert(slots.end(), slot_list.begin() + slot_start[p.first], slot_list.begin() + slot_start[p.second]);
    }
    if (!slots.empty()) refit_bvh(b, ix, s, slots, margin);
    return static_cast<int64_t>(slots.size());
}

int64_t host_refresh_lights(HostScene& s, Bvh& lb, const BvhRefitIndex& ix, const std::vector<int32_t>& slot_start,
                            const std::vector<int32_t>& slot_list, const PendingRanges& ranges, double margin) {
    std::vector<int32_t> slots;
    int64_t lights = 0;
    for (const auto& p : ranges.r) {
        for (int f = p.first; f < p.second; f++)
            if (s.light_of[f] >= 0) {
                s.light_area[s.light_of[f]] = light_triangle_area(s, f);
                lights++;
            }
        slots.insert(slots.end(), slot_list.begin() + slot_start[p.first], slot_list.begin() + slot_start[p.second]);
    }
    if (!slots.empty()) refit_bvh(lb, ix, s, slots, margin);
    return lights;
}

int first_degenerate_light(const HostScene& s, int32_t first, int32_t count, const float* pos) {
    for (int32_t i = 0; i < count; i++) {
        if (s.light_of[first + i] < 0) continue;
        const float* p = pos + 9 * static_cast<size_t>(i);
        double ba[3], ca[3];
        for (int q = 0; q < 3; q++) {
            ba[q] = static_cast<double>(p[3 + q]) - static_cast<double>(p[q]);
            ca[q] = static_cast<double>(p[6 + q]) - static_cast<double>(p[q]);
        }
        const double n[3] = {ba[1] * ca[2] - ba[2] * ca[1], ba[2] * ca[0] - ba[0] * ca[2], ba[0] * ca[1] - ba[1] * ca[0]};
        const double l = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (!(l > 0) || !std::isfinite(l)) return first + i;
    }
    return -1;
}

}  // namespace mcpt

extern "C" int mcpt_transform_rotation(const double axis[3], double degrees, const double pivot[3], const double translate[3],
                                       double m[12]) {
    using mcpt::set_error;
    if (!axis || !pivot || !m) {
        set_error("mcpt_transform_rotation: NULL %s", !axis ? "axis" : !pivot ? "pivot" : "m");
        return MCPT_E_INVALID;
    }
    bool fin = std::isfinite(degrees);
    for (int a = 0; a < 3; a++) fin = fin && std::isfinite(axis[a]) && std::isfinite(pivot[a]) && (!translate || std::isfinite(translate[a]));
    const double al = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    if (!fin || !std::isfinite(al) || !(al > 0)) {
        set_error("mcpt_transform_rotation: degrees, axis, pivot and translate must be finite and the axis must have a "
                  "finite length > 0 (it is %g)", al);
        return MCPT_E_INVALID;
    }
    const double t = degrees * 3.14159265358979323846 / 180.0, s = std::sin(t), c = std::cos(t), c1 = 1.0 - c;
    const double k[3] = {axis[0] / al, axis[1] / al, axis[2] / al};
    // Rodrigues: R = c I + (1 - c) k k^T + s [k]x; "+ 0.0" turns a -0 of the 0-degree case into +0
    const double cross[3][3] = {{0, -k[2], k[1]}, {k[2], 0, -k[0]}, {-k[1], k[0], 0}};
    for (int r = 0; r < 3; r++) {
        for (int q = 0; q < 3; q++) m[4 * r + q] = ((r == q ? c : 0.0) + (c1 * k[r] * k[q] + s * cross[r][q])) + 0.0;
        const double rp = (m[4 * r] * pivot[0] + m[4 * r + 1] * pivot[1]) + m[4 * r + 2] * pivot[2];
        m[4 * r + 3] = (pivot[r] - rp) + (translate ? translate[r] : 0.0);
    }
    return MCPT_OK;
}
