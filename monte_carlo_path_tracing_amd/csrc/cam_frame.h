// The camera frame of main.cpp:507-510,547-553, shared by the renderer (render.hip) and the temporal
// reprojection (temporal.hip), which inverts cam_dir with it.
#pragma once
#include <cmath>

#include "device_math.h"
#include "mcpt.h"

namespace mcpt {

struct CamFrame {
    d3 eye, U, V, N;
    double wlen, pixellen;
    int W, H;
};

// camera of main.cpp:507-510,547-553 (host, fp64, same operation order as the oracle)
static CamFrame cam_setup(const mcpt_camera& c) {
    auto sub3 = [](d3 a, d3 b) { return d3{a.x - b.x, a.y - b.y, a.z - b.z}; };
    auto mul3 = [](d3 a, double s) { return d3{a.x * s, a.y * s, a.z * s}; };
    auto nrm = [](d3 a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); };
    auto unit = [&](d3 a) {
        double l = nrm(a);
        return d3{a.x / l, a.y / l, a.z / l};
    };
    auto cr = [](d3 a, d3 b) { return d3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; };
    CamFrame f;
    d3 start{c.eye[0], c.eye[1], c.eye[2]};
    d3 w = sub3(d3{c.lookat[0], c.lookat[1], c.lookat[2]}, start);
    start = sub3(start, mul3(w, c.dist_scale - 1));
    w = mul3(w, c.dist_scale);
    f.eye = start;
    f.wlen = nrm(w);
    f.pixellen = std::tan(c.fovy / 360) * nrm(w) / (c.height / 2.0);
    f.N = unit(w);
    f.V = unit(cr(f.N, d3{c.up[0], c.up[1], c.up[2]}));
    f.U = unit(cr(f.V, f.N));
    f.W = c.width;
    f.H = c.height;
    return f;
}

}  // namespace mcpt
