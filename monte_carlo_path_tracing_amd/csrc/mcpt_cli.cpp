// mcpt_render -- the reference's render driver (main.cpp:497-600) as a host C++ program over the
// C ABI: load the scene (Myobj::read / Mylight::read, main.cpp:500-504), set the camera
// (main.cpp:507-510, eye pulled back 2x by default), render(scene, camera, spp, mode), tone-map
// (380, 0.25; main.cpp:583) and save the BMP (main.cpp:596).  Unlike the reference, size, spp,
// integrator and output path are flags instead of edits to main.cpp.
//
//   mcpt_render --scene scenes/veach-mis/veach-mis [--width 1280 --height 720] [--spp 10]
//               [--mode mis|brdf|shade|shade-area] [--seed 20240430] [--out test.bmp] [--hdr out.pfm] [--progress]
//               [--grid] [--devices 0,1,2,3,4,5,6,7] [--precision fp64|fp32] [--jitter]
//   --jitter anti-aliases (MCPT_RENDER_PIXEL_JITTER): every sample's camera ray goes through its own point of the
//   pixel's square instead of the centre (a box pixel filter); slower, the primary hit is traced per sample.  Works
//   with --frames, --orbit, --denoise, --history-clamp, --device-sequence and --devices; not with --adaptive or --grid.
//               [--adaptive TAU [--min-spp N] [--pass-spp N] [--radius R] [--count-out count.bmp]]
//   --adaptive TAU renders adaptively (mcpt_render_adaptive): passes of --pass-spp samples after the first
//   --min-spp (default 16 each), a pixel stops once its noise estimate is at most TAU and so are its
//   neighbours' within --radius (default 1); --spp is the cap.  Prints the mean spp and the share of pixels at
//   the cap; --count-out writes the per-pixel sample count as a grey BMP (white = the cap).  One device.
//               [--denoise [--denoise-iterations K] [--denoise-sigma-color S]] [--aov-out PREFIX]
//   --denoise filters the frame with the variance-guided a-trous filter (mcpt_denoise) guided by the primary-hit
//   AOVs (mcpt_render_aovs); --out and --hdr then carry the denoised frame.  With --adaptive the variance comes
//   from the adaptive render's noise map (mcpt_variance_from_noise), else from the filter's spatial estimate.
//   --aov-out PREFIX writes PREFIX_albedo.pfm, PREFIX_normal.pfm (PF) and PREFIX_depth.pfm (Pf).
//               [--frames N --orbit DEG [--temporal-alpha A] [--history-clamp K [--clamp-radius R] [--clamp-alpha-fast A]]]
//   --frames N renders a sequence with temporal accumulation (mcpt_temporal_accumulate): frame k uses the camera
//   orbited by k * DEG degrees about the up axis through lookat (mcpt_camera_orbit) and seed + k (with the counter
//   RNG the same seed would repeat the same noise), and is accumulated onto the reprojected history of frame k - 1.
//   With --denoise the accumulated colour and its temporal variance feed mcpt_denoise; the unfiltered accumulated
//   colour stays the history.  --out, --hdr and --aov-out gain _%04d (the frame) before the extension; one line per
//   frame reports the share of pixels that kept their history.  Not with --adaptive.
//   --history-clamp K accumulates with mcpt_temporal_accumulate_clamped: the history is clamped to mean +- K standard
//   deviations of a fast history (weight of the current frame >= A, default 0.5) over the (2 R + 1)^2 window (default
//   R = 2), which removes the ghosts of view-dependent shading at larger steps and costs a little on a static camera;
//   the frame's line then ends with the share of pixels the clamp moved.
//               [--device-sequence]
//   --device-sequence (with --frames) runs the same sequence through mcpt_sequence: every stage, the tone map
//   included, works on device buffers allocated once, and per frame only the 8-bit image (and the HDR frame, when
//   --hdr asks for it) comes back.  The files and the lines printed are those of the default path.  One device; not
//   with --aov-out (the handle does not hand out the guides).
//               [--upsample F]
//   --upsample F (2..4) traces at 1 / F of the size asked for and reconstructs the full-size frame by guided upsampling
//   (mcpt_upsample): --width and --height are the shown size and must be divisible by F; the render, the AOVs, the
//   accumulation and the filter run at size / F, then the AOVs of the full-size camera (mcpt_camera_scaled) guide the
//   upsampling, and --out and --hdr carry the full-size frame.  Works for a single frame, with --frames and with
//   --frames --device-sequence (mcpt_sequence_create_upsampled); not with --adaptive, --grid or --aov-out.
//               [--temporal-upsample]
//   --temporal-upsample (with --frames N --device-sequence --upsample F) traces, every frame, a different 1 / F^2 subset
//   of the full-size pixels and accumulates them in a full-size history (mcpt_sequence_create_temporal_upsampled): the
//   same files and lines as the --upsample arm, the "upsampled" line carrying the frame's phase and the share of the
//   pixels that were filled in.  Not with --history-clamp, --jitter, --grid or --adaptive.
//               [--hide FIRST:COUNT[:FRAME]] [--show FIRST:COUNT[:FRAME]]
//   --hide and --show (repeatable, with or without --frames and --device-sequence) make facets [FIRST, FIRST + COUNT)
//   invisible or visible again in place (mcpt_scene_set_visible) before the frame with the 0-based index FRAME (default
//   0), in command-line order, and print a "hid" / "showed" line with the call's statistics.  A range with a light
//   triangle is refused with the library's message.  Not with --grid.
//               [--move FIRST:COUNT:DX,DY,DZ]
//   --move (with --frames N, with or without --device-sequence) animates facets [FIRST, FIRST + COUNT): before frame
//   k >= 1 they are set to float(double(original) + k * (DX, DY, DZ)) by mcpt_scene_update (the BVH is refit in place, no
//   rebuild), and the frame prints a "moved" line with the update's statistics.  A range with a light triangle, or a
//   step that leaves the scene's arena, ends the run with the library's message.
//               [--rotate FIRST:COUNT:AX,AY,AZ:DEG:PX,PY,PZ]
//   --rotate (with --frames N, with or without --device-sequence; not with --move) turns facets [FIRST, FIRST + COUNT):
//   the scene's rest pose is saved once before frame 0 (mcpt_scene_rest_save), and before frame k >= 1 the range is set
//   to the rest pose rotated by k * DEG degrees about the axis (AX, AY, AZ) through (PX, PY, PZ) by mcpt_scene_transform
//   (evaluated on the device; the host copy is not touched during the loop); the frame prints a "rotated" line.
//               [--lights-movable]
//   --lights-movable (with --frames N and --move or --rotate) switches the scene's light triangles to movable before
//   frame 0 (mcpt_scene_set_lights_movable), so a range with light triangles is moved like any other: the light tables
//   and the light-only tree follow on the device.
//               [--rebuild RATIO]
//   --rebuild (with --frames N and --move or --rotate) watches the tree the moves degrade: after each frame's move the
//   tree's cost is read (mcpt_scene_tree_cost), and once it exceeds RATIO (finite, > 1) times the cost at the last build
//   or rebuild the main tree is rebuilt on the device (mcpt_scene_rebuild) and the frame prints a "rebuilt" line.
//               [--motion]
//   --motion (with --frames N, with or without --device-sequence; meant for --move and --rotate) lets the history follow the moved
//   facets: before each frame's move the scene's pose is saved (mcpt_scene_pose_save), the frame renders the motion AOVs
//   (mcpt_render_motion_aovs) and accumulates with mcpt_temporal_accumulate_motion (mcpt_sequence_set_motion in the device
//   sequence), so a moved surface keeps its history instead of restarting it every frame.  Not with --upsample.
//               [--antilag] [--antilag-stratum S]
//   --antilag (with --frames N, with or without --device-sequence; meant for --dim, --tint, --move and --rotate) drops
//   history that an edit of the scene made stale: every frame from the second on traces one sample pixel per S x S
//   block (S = 3, or --antilag-stratum S in 1..8) of the previous frame again, with that frame's camera and seed in the
//   scene as it is now (mcpt_gradient_rays, mcpt_render_rays), turns the difference into Lambda (mcpt_temporal_gradient)
//   and accumulates with mcpt_temporal_accumulate_antilag (mcpt_sequence_set_antilag in the device sequence); the frame
//   prints an "anti-lag" line.  Not with --jitter, --grid or --upsample.
//               [--dim GROUP:FACTOR]... [--tint MATERIAL:R,G,B]...
//   --dim and --tint (with --frames N, with or without --device-sequence, with --move / --rotate or alone) re-light the
//   scene in place: before frame k >= 1 the radiance of every light of GROUP (mcpt_scene_light_groups) is multiplied by
//   FACTOR once more (mcpt_scene_set_light_radiance; 0 switches the group off), and before frame 1 row MATERIAL of the
//   material table gets Kd = (R, G, B) (mcpt_scene_set_materials).  Each prints a "dimmed" / "tinted" line.
//   --devices renders on several GPUs of this node: the sample range is split into one contiguous shard
//   per listed device, rendered concurrently, and summed by ONE RCCL reduce into the first device
//   (mcpt_render_opts.devices; the reference itself is single-threaded, README.md:418).
//   --grid traverses the reference's uniform grid (Myobj.cpp:78-162, n0 = 100000) instead of the BVH.
//   --precision fp32 selects the opt-in FP32_STABLE light prep (MCPT_RENDER_PRECISION_FP32); fp64 (the
//   reference's, default) otherwise.
//   --progress prints the share of camera samples dispatched (the reference prints per-row progress
//   and updates its EasyX window, main.cpp:539-592) through mcpt_render_opts.progress.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mcpt.h"

namespace {

int print_progress(void* user, uint64_t done, uint64_t total) {
    int* last = static_cast<int*>(user);
    const int pct = total ? (int)(100 * done / total) : 100;
    if (pct / 10 != *last / 10) {
        std::fprintf(stderr, "\rrendering: %3d%% of %llu camera samples dispatched", pct, (unsigned long long)total);
        if (pct == 100) std::fprintf(stderr, "\n");
        *last = pct;
    }
    return 0;
}

// render(scene, camera, spp, mode): main.cpp:547-588 lifted into a function.
int render(mcpt_scene* scene, const mcpt_camera& cam, int spp, int mode, uint64_t seed, bool progress, bool grid, int flags,
           const std::vector<int32_t>& devices, std::vector<double>& hdr, mcpt_stats* st) {
    hdr.assign(3ull * cam.width * cam.height, 0.0);
    mcpt_render_opts o;
    mcpt_render_opts_init(&o);
    o.spp = spp;
    o.mode = mode;
    o.seed = seed;
    o.accel = grid ? MCPT_ACCEL_GRID : MCPT_ACCEL_BVH;
    o.flags = flags;
    if (!devices.empty()) {  // one process, several GPUs: shards + one RCCL reduce
        o.num_devices = (int32_t)devices.size();
        o.devices = devices.data();
    }
    int last = -10;
    if (progress) {
        o.progress = print_progress;
        o.progress_user = &last;
    }
    return mcpt_render(scene, &cam, &o, hdr.data(), st);
}

// the adaptive form of render(): --spp is the cap; the count map comes back too
int render_adaptive(mcpt_scene* scene, const mcpt_camera& cam, const mcpt_adaptive_opts& ad, int mode, uint64_t seed,
                    bool progress, bool grid, int flags, std::vector<double>& hdr, std::vector<int32_t>& count,
                    std::vector<double>& noise, mcpt_stats* st) {
    hdr.assign(3ull * cam.width * cam.height, 0.0);
    count.assign((size_t)cam.width * cam.height, 0);
    noise.assign((size_t)cam.width * cam.height, 0.0);
    mcpt_render_opts o;
    mcpt_render_opts_init(&o);
    o.mode = mode;
    o.seed = seed;
    o.accel = grid ? MCPT_ACCEL_GRID : MCPT_ACCEL_BVH;
    o.flags = flags;
    int last = -10;
    if (progress) {
        o.progress = print_progress;
        o.progress_user = &last;
    }
    return mcpt_render_adaptive(scene, &cam, &o, &ad, hdr.data(), count.data(), noise.data(), st);
}

// channels: 3 (PF) or 1 (Pf)
bool write_pfm(const char* path, const std::vector<double>& hdr, int W, int H, int channels = 3) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    std::fprintf(f, "%s\n%d %d\n-1.0\n", channels == 3 ? "PF" : "Pf", W, H);
    std::vector<float> row((size_t)channels * W);
    for (int i = H - 1; i >= 0; i--) {  // PFM is bottom-up
        for (int k = 0; k < channels * W; k++) row[k] = static_cast<float>(hdr[(size_t)channels * i * W + k]);
        std::fwrite(row.data(), sizeof(float), row.size(), f);
    }
    std::fclose(f);
    return true;
}

// "out.bmp", 7 -> "out_0007.bmp" (no extension: appended)
std::string frame_path(const std::string& path, int k) {
    char tag[16];
    std::snprintf(tag, sizeof tag, "_%04d", k);
    const size_t dot = path.rfind('.'), slash = path.find_last_of('/');
    if (dot == std::string::npos || (slash != std::string::npos && dot < slash)) return path + tag;
    return path.substr(0, dot) + tag + path.substr(dot);
}

// --move FIRST:COUNT:DX,DY,DZ: before frame k >= 1 facets [first, first + count) are set to
// float(double(original) + k * d) through mcpt_scene_update, from the original arrays so that nothing drifts
struct Mover {
    int32_t first = 0, count = 0;
    double d[3] = {0, 0, 0};
    std::vector<float> original, moved;
    bool parse(const char* arg) {
        char tail = 0;
        return std::sscanf(arg, "%d:%d:%lf,%lf,%lf%c", &first, &count, &d[0], &d[1], &d[2], &tail) == 5 && first >= 0 && count >= 1 &&
               std::isfinite(d[0]) && std::isfinite(d[1]) && std::isfinite(d[2]);
    }
    // the range against the scene (a light facet in it is the library's refusal, at the first update)
    int bind(mcpt_scene* scene) {
        int32_t nf = 0;
        mcpt_scene_counts(scene, &nf, nullptr, nullptr);
        if ((int64_t)first + count > nf) {
            std::fprintf(stderr, "--move: facets [%d, %lld) are not in the scene's %d\n", first, (long long)first + count, nf);
            return 2;
        }
        std::vector<float> all(9 * (size_t)nf);
        mcpt_scene_arrays(scene, all.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        original.assign(all.begin() + 9 * (size_t)first, all.begin() + 9 * ((size_t)first + count));
        moved.resize(original.size());
        return 0;
    }
    int apply(mcpt_scene* scene, int k) {
        if (k < 1) return 0;
        for (size_t i = 0; i < original.size(); i++) moved[i] = (float)((double)original[i] + k * d[i % 3]);
        mcpt_update_stats us;
        mcpt_update_stats_init(&us);
        if (mcpt_scene_update(scene, first, count, moved.data(), nullptr, &us) != MCPT_OK) {
            std::fprintf(stderr, "--move failed: %s\n", mcpt_last_error());
            return 1;
        }
        std::printf("  moved facets [%d, %d) by %d x (%g, %g, %g): %lld leaf slots, %lld nodes refit on %d levels, %.3f ms device\n",
                    first, first + count, k, d[0], d[1], d[2], (long long)us.leaf_slots, (long long)us.nodes_refit, us.levels,
                    us.device_seconds * 1e3);
        return 0;
    }
};

// --hide FIRST:COUNT[:FRAME] and --show FIRST:COUNT[:FRAME] (repeatable): before the frame with that 0-based index
// (default 0, so it also works without --frames) facets [first, first + count) are hidden or shown again in place
// (mcpt_scene_set_visible), in the order of the command line
struct Visibility {
    struct Edit {
        int32_t first, count, frame, visible;
    };
    std::vector<Edit> edits;
    bool parse(const char* arg, bool visible) {
        Edit e{0, 0, 0, visible ? 1 : 0};
        char tail = 0;
        const int n = std::sscanf(arg, "%d:%d%c", &e.first, &e.count, &tail);
        if (n == 3 && std::sscanf(arg, "%d:%d:%d%c", &e.first, &e.count, &e.frame, &tail) != 3) return false;
        if (n < 2 || e.first < 0 || e.count < 1 || e.frame < 0) return false;
        edits.push_back(e);
        return true;
    }
    int apply(mcpt_scene* scene, int k) const {
        for (const Edit& e : edits) {
            if (e.frame != k) continue;
            mcpt_update_stats us;
            mcpt_update_stats_init(&us);
            if (mcpt_scene_set_visible(scene, e.first, e.count, e.visible, &us) != MCPT_OK) {
                std::fprintf(stderr, "--%s failed: %s\n", e.visible ? "show" : "hide", mcpt_last_error());
                return 1;
            }
            std::printf("  %s facets [%d, %d): %lld leaf slots, %lld nodes refit on %d levels, %.3f ms device\n",
                        e.visible ? "showed" : "hid", e.first, e.first + e.count, (long long)us.leaf_slots, (long long)us.nodes_refit,
                        us.levels, us.device_seconds * 1e3);
        }
        return 0;
    }
};

// --rotate FIRST:COUNT:AX,AY,AZ:DEG:PX,PY,PZ: the scene's rest pose is saved once before frame 0; before frame k >= 1
// facets [first, first + count) are set to the rest pose rotated by k * DEG degrees about the axis through the pivot
// (mcpt_transform_rotation, mcpt_scene_transform: evaluated on the device, always from the rest pose)
struct Rotator {
    int32_t first = 0, count = 0;
    double axis[3] = {0, 0, 0}, deg = 0, pivot[3] = {0, 0, 0};
    bool parse(const char* arg) {
        char tail = 0;
        if (std::sscanf(arg, "%d:%d:%lf,%lf,%lf:%lf:%lf,%lf,%lf%c", &first, &count, &axis[0], &axis[1], &axis[2], &deg, &pivot[0],
                        &pivot[1], &pivot[2], &tail) != 9)
            return false;
        double m[12];
        return first >= 0 && count >= 1 && mcpt_transform_rotation(axis, deg, pivot, nullptr, m) == MCPT_OK;
    }
    int bind(mcpt_scene* scene) {
        int32_t nf = 0;
        mcpt_scene_counts(scene, &nf, nullptr, nullptr);
        if ((int64_t)first + count > nf) {
            std::fprintf(stderr, "--rotate: facets [%d, %lld) are not in the scene's %d\n", first, (long long)first + count, nf);
            return 2;
        }
        if (mcpt_scene_rest_save(scene) != MCPT_OK) {
            std::fprintf(stderr, "--rotate failed: %s\n", mcpt_last_error());
            return 1;
        }
        return 0;
    }
    int apply(mcpt_scene* scene, int k) {
        if (k < 1) return 0;
        double m[12];
        mcpt_update_stats us;
        mcpt_update_stats_init(&us);
        if (mcpt_transform_rotation(axis, k * deg, pivot, nullptr, m) != MCPT_OK ||
            mcpt_scene_transform(scene, first, count, m, nullptr, &us) != MCPT_OK) {
            std::fprintf(stderr, "--rotate failed: %s\n", mcpt_last_error());
            return 1;
        }
        std::printf("  rotated facets [%d, %d) by %g deg: %lld leaf slots, %lld nodes refit on %d levels, %.3f ms device\n", first,
                    first + count, k * deg, (long long)us.leaf_slots, (long long)us.nodes_refit, us.levels, us.device_seconds * 1e3);
        return 0;
    }
};

// --rebuild RATIO (with --frames N and --move or --rotate): after each frame's move the main tree's cost is read
// (mcpt_scene_tree_cost); once it exceeds RATIO x the cost at the last build or rebuild, the tree is rebuilt on the
// device (mcpt_scene_rebuild) and one line says so
struct Rebuilder {
    double ratio = 0, base = 0;
    bool have_base = false;
    bool parse(const char* arg) {
        char* e = nullptr;
        ratio = std::strtod(arg, &e);
        return e != arg && *e == 0 && std::isfinite(ratio) && ratio > 1.0;
    }
    int apply(mcpt_scene* scene, int k) {
        double cost = 0;
        if (mcpt_scene_tree_cost(scene, -1, &cost) != MCPT_OK) {
            std::fprintf(stderr, "--rebuild failed: %s\n", mcpt_last_error());
            return 1;
        }
        if (!have_base) {
            base = cost, have_base = true;
            return 0;
        }
        if (!(cost > ratio * base)) return 0;
        mcpt_rebuild_stats rs;
        mcpt_rebuild_stats_init(&rs);
        if (mcpt_scene_rebuild(scene, &rs) != MCPT_OK) {
            std::fprintf(stderr, "--rebuild failed: %s\n", mcpt_last_error());
            return 1;
        }
        std::printf("  rebuilt the tree before frame %d: cost %.4g > %g x %.4g, now %.4g; %d nodes on %d levels, stack need %d, %.3f ms "
                    "device\n", k, rs.cost_before, ratio, base, rs.cost_after, rs.nodes, rs.levels, rs.stack_need,
                    rs.device_seconds * 1e3);
        base = rs.cost_after;
        return 0;
    }
};

// --dim GROUP:FACTOR (repeatable) and --tint MATERIAL:R,G,B (repeatable), with --frames N: before frame k >= 1 every light
// of GROUP (an index of mcpt_scene_light_groups) gets its radiance multiplied by FACTOR once more, each step an fp64
// multiply of the previous value (mcpt_scene_set_light_radiance); before frame 1 row MATERIAL of the material table
// gets Kd = (R, G, B) (mcpt_scene_set_materials).  Nothing is rebuilt and no geometry moves.
struct Relighter {
    struct Dim {
        int32_t group;
        double factor;
        int32_t l0 = 0, l1 = 0;  // the group's run of the light table
    };
    struct Tint {
        int32_t material;
        float kd[3];
    };
    std::vector<Dim> dims;
    std::vector<Tint> tints;
    std::vector<double> rad;  // the light table's radiances as the steps so far left them
    bool parse_dim(const char* arg) {
        Dim d{};
        char tail = 0;
        if (std::sscanf(arg, "%d:%lf%c", &d.group, &d.factor, &tail) != 2 || d.group < 0 || !std::isfinite(d.factor) || d.factor < 0) return false;
        dims.push_back(d);
        return true;
    }
    bool parse_tint(const char* arg) {
        Tint t{};
        char tail = 0;
        if (std::sscanf(arg, "%d:%f,%f,%f%c", &t.material, &t.kd[0], &t.kd[1], &t.kd[2], &tail) != 4 || t.material < 0) return false;
        for (float v : t.kd)
            if (!std::isfinite(v) || v < 0) return false;
        tints.push_back(t);
        return true;
    }
    // the groups and rows against the scene
    int bind(mcpt_scene* scene) {
        int32_t nm = 0, nl = 0;
        mcpt_scene_counts(scene, nullptr, &nm, &nl);
        std::vector<int32_t> group(nl > 0 ? nl : 1, -1);
        rad.assign(3 * (size_t)(nl > 0 ? nl : 1), 0.0);
        if (nl > 0) {
            mcpt_scene_light_groups(scene, group.data());
            mcpt_scene_arrays(scene, nullptr, nullptr, nullptr, nullptr, nullptr, rad.data(), nullptr);
        }
        for (Dim& d : dims) {
            d.l0 = d.l1 = 0;
            for (int32_t l = 0; l < nl; l++)
                if (group[l] == d.group) {
                    if (d.l1 == d.l0) d.l0 = l;
                    d.l1 = l + 1;
                }
            if (d.l1 == d.l0) {
                std::fprintf(stderr, "--dim: the scene has no light group %d (its %d light triangles are in groups 0..%d)\n", d.group, nl,
                             nl > 0 ? group[nl - 1] : -1);
                return 2;
            }
        }
        for (const Tint& t : tints)
            if (t.material >= nm) {
                std::fprintf(stderr, "--tint: material %d is not one of the scene's %d\n", t.material, nm);
                return 2;
            }
        return 0;
    }
    int apply(mcpt_scene* scene, int k) {
        if (k < 1) return 0;
        mcpt_relight_stats rs;
        mcpt_relight_stats_init(&rs);
        for (const Dim& d : dims) {
            for (size_t i = 3 * (size_t)d.l0; i < 3 * (size_t)d.l1; i++) rad[i] *= d.factor;
            if (mcpt_scene_set_light_radiance(scene, d.l0, d.l1 - d.l0, rad.data() + 3 * (size_t)d.l0, &rs) != MCPT_OK) {
                std::fprintf(stderr, "--dim failed: %s\n", mcpt_last_error());
                return 1;
            }
            std::printf("  dimmed light group %d by %g (step %d): %d lights in %d chunks, %.3f ms device\n", d.group, d.factor, k, rs.lights,
                        rs.chunks, rs.device_seconds * 1e3);
        }
        if (k == 1 && !tints.empty()) {
            int32_t nm = 0;
            mcpt_scene_counts(scene, nullptr, &nm, nullptr);
            std::vector<float> mtl(7 * (size_t)nm);
            mcpt_scene_arrays(scene, nullptr, nullptr, nullptr, mtl.data(), nullptr, nullptr, nullptr);
            for (const Tint& t : tints) {
                float* row = mtl.data() + 7 * (size_t)t.material;
                std::memcpy(row, t.kd, sizeof t.kd);
                if (mcpt_scene_set_materials(scene, t.material, 1, row, &rs) != MCPT_OK) {
                    std::fprintf(stderr, "--tint failed: %s\n", mcpt_last_error());
                    return 1;
                }
                std::printf("  tinted material %d: Kd = (%g, %g, %g), %.3f ms device\n", t.material, t.kd[0], t.kd[1], t.kd[2],
                            rs.device_seconds * 1e3);
            }
        }
        return 0;
    }
};

struct SequenceArgs {
    int frames, spp, mode, flags;
    double orbit;
    uint64_t seed;
    bool progress, grid, denoise;
    std::string out, hdr_out, aov_out;
    Mover* move;  // --move, or null
    bool motion;  // --motion
    Rotator* rotate;  // --rotate, or null
    Rebuilder* rebuild;  // --rebuild, or null
    Relighter* relight;  // --dim / --tint, or null
    int antilag;  // --antilag: the stratum, or 0
    const Visibility* vis;  // --hide / --show, or null
};

void print_antilag(int stratum, int a, int b, double mean, double mx, double trace_seconds) {
    std::printf("  anti-lag: stratum %d, phase (%d, %d), Lambda mean %.4f, max %.4f, %.3f ms gradient render\n", stratum, a, b, mean, mx,
                trace_seconds * 1e3);
}

// --frames: render, accumulate (and filter) frame after frame; the history ping-pongs between two sets of buffers
// the full-size guides of `cam` scaled by up.factor, then mcpt_upsample of the low frame `low` into `full`; prints the
// stage's line
int upsample_frame(mcpt_scene* scene, const mcpt_camera& cam, const mcpt_upsample_opts& up, const std::vector<double>& low,
                   const mcpt_aov_buffers& aov, std::vector<double>& full) {
    mcpt_camera fc;
    if (mcpt_camera_scaled(&cam, up.factor, &fc) != MCPT_OK) {
        std::fprintf(stderr, "%s\n", mcpt_last_error());
        return 1;
    }
    const size_t NPX = (size_t)fc.width * fc.height;
    std::vector<double> albedo(3 * NPX), normal(3 * NPX), position(3 * NPX), depth(NPX);
    const mcpt_aov_buffers faov{albedo.data(), normal.data(), position.data(), depth.data()};
    mcpt_render_opts ao;
    mcpt_render_opts_init(&ao);
    if (mcpt_render_aovs(scene, &fc, &ao, &faov) != MCPT_OK) {
        std::fprintf(stderr, "AOV render failed: %s\n", mcpt_last_error());
        return 1;
    }
    full.assign(3 * NPX, 0.0);
    uint64_t fell = 0;
    double usec = 0;
    if (mcpt_upsample(&up, cam.width, cam.height, low.data(), &aov, &faov, full.data(), &fell, &usec) != MCPT_OK) {
        std::fprintf(stderr, "upsampling failed: %s\n", mcpt_last_error());
        return 1;
    }
    std::printf("  upsampled: factor %d to %dx%d, %.2f%% of the pixels took the fallback, %.3f ms device\n", up.factor, fc.width,
                fc.height, 100.0 * (double)fell / (double)NPX, usec * 1e3);
    return 0;
}

int render_sequence(mcpt_scene* scene, const mcpt_camera& cam0, const SequenceArgs& a, const std::vector<int32_t>& devices,
                    const mcpt_temporal_opts& tp, const mcpt_temporal_clamp_opts* clamp, const mcpt_denoise_opts& dn,
                    const mcpt_upsample_opts* up) {
    const int W = cam0.width, H = cam0.height;
    const int SW = up ? W * up->factor : W, SH = up ? H * up->factor : H;  // the shown size
    const size_t npx = (size_t)W * H;
    struct Frame {
        mcpt_camera cam;
        std::vector<double> albedo, normal, position, depth, color, moments, fast;
    } fr[2];
    for (auto& f : fr) {
        f.albedo.resize(3 * npx), f.normal.resize(3 * npx), f.position.resize(3 * npx), f.depth.resize(npx);
        f.color.resize(3 * npx), f.moments.resize(4 * npx);
        if (clamp) f.fast.resize(3 * npx);
    }
    std::vector<double> hdr, variance(npx), filtered(3 * npx), shift(clamp ? npx : 0), upsampled;
    std::vector<double> prev_position(a.motion ? 3 * npx : 0), prev_normal(a.motion ? 3 * npx : 0);
    // --antilag: the previous frame's raw render, the gradient rays and their radiance, Lambda
    mcpt_gradient_opts go;
    mcpt_gradient_opts_init(&go);
    if (a.antilag) go.stratum = a.antilag;
    const size_t nlam = a.antilag ? (size_t)((H + go.stratum - 1) / go.stratum) * ((W + go.stratum - 1) / go.stratum) : 0;
    std::vector<double> prev_raw, ray_o(a.antilag ? 3 * npx : 0), ray_d(a.antilag ? 3 * npx : 0), regrad, lambda(nlam);
    for (int k = 0; k < a.frames; k++) {
        Frame &cur = fr[k & 1], &prev = fr[(k & 1) ^ 1];
        if (a.motion && mcpt_scene_pose_save(scene) != MCPT_OK) {
            std::fprintf(stderr, "--motion failed: %s\n", mcpt_last_error());
            return 1;
        }
        if (a.vis && a.vis->apply(scene, k)) return 1;
        if (a.move && a.move->apply(scene, k)) return 1;
        if (a.rotate && a.rotate->apply(scene, k)) return 1;
        if (a.rebuild && a.rebuild->apply(scene, k)) return 1;
        if (a.relight && a.relight->apply(scene, k)) return 1;
        if (mcpt_camera_orbit(&cam0, k * a.orbit, &cur.cam) != MCPT_OK) {
            std::fprintf(stderr, "%s\n", mcpt_last_error());
            return 1;
        }
        if (a.antilag) {  // the previous frame's samples again, in the scene as it is now
            std::fill(lambda.begin(), lambda.end(), 0.0);
            if (k) {
                int32_t pa = 0, pb = 0;
                mcpt_render_opts gr;
                mcpt_render_opts_init(&gr);
                gr.spp = a.spp, gr.mode = a.mode, gr.seed = a.seed + k - 1, gr.flags = a.flags;
                mcpt_stats gst{};
                regrad.assign(3 * npx, 0.0);
                if (mcpt_gradient_phase(go.stratum, (uint64_t)k, &pa, &pb) != MCPT_OK ||
                    mcpt_gradient_rays(&prev.cam, go.stratum, pa, pb, -1, ray_o.data(), ray_d.data()) != MCPT_OK ||
                    mcpt_render_rays(scene, &gr, (int32_t)npx, ray_o.data(), ray_d.data(), regrad.data(), &gst) != MCPT_OK ||
                    mcpt_temporal_gradient(&go, W, H, pa, pb, prev_raw.data(), regrad.data(), lambda.data(), nullptr) != MCPT_OK) {
                    std::fprintf(stderr, "anti-lag gradient failed: %s\n", mcpt_last_error());
                    return 1;
                }
                double sum = 0, mx = 0;
                for (double v : lambda) sum += v, mx = v > mx ? v : mx;
                print_antilag(go.stratum, pa, pb, sum / (double)nlam, mx, gst.seconds);
            }
        }
        mcpt_stats st{};
        if (render(scene, cur.cam, a.spp, a.mode, a.seed + k, a.progress, a.grid, a.flags, devices, hdr, &st) != MCPT_OK) {
            std::fprintf(stderr, "render failed: %s\n", mcpt_last_error());
            return 1;
        }
        if (a.antilag) prev_raw = hdr;
        const mcpt_aov_buffers aov{cur.albedo.data(), cur.normal.data(), cur.position.data(), cur.depth.data()};
        const mcpt_aov_buffers paov{prev.albedo.data(), prev.normal.data(), prev.position.data(), prev.depth.data()};
        mcpt_render_opts ao;
        mcpt_render_opts_init(&ao);
        ao.accel = a.grid ? MCPT_ACCEL_GRID : MCPT_ACCEL_BVH;
        if (mcpt_render_aovs(scene, &cur.cam, &ao, &aov) != MCPT_OK) {
            std::fprintf(stderr, "AOV render failed: %s\n", mcpt_last_error());
            return 1;
        }
        const mcpt_motion_buffers mo{prev_position.data(), prev_normal.data()};
        if (a.motion && mcpt_render_motion_aovs(scene, &cur.cam, &ao, &mo) != MCPT_OK) {
            std::fprintf(stderr, "motion AOV render failed: %s\n", mcpt_last_error());
            return 1;
        }
        double tsec = 0;
        const int rc = a.antilag ? mcpt_temporal_accumulate_antilag(&tp, clamp, k ? &prev.cam : nullptr, W, H, hdr.data(), &aov,
                                                                    a.motion ? &mo : nullptr, k ? &paov : nullptr,
                                                                    k ? prev.color.data() : nullptr, k ? prev.moments.data() : nullptr,
                                                                    clamp && k ? prev.fast.data() : nullptr, cur.color.data(),
                                                                    cur.moments.data(), clamp ? cur.fast.data() : nullptr,
                                                                    clamp ? shift.data() : nullptr, variance.data(), &tsec, &go,
                                                                    lambda.data())
                       : a.motion ? mcpt_temporal_accumulate_motion(&tp, clamp, k ? &prev.cam : nullptr, W, H, hdr.data(), &aov, &mo,
                                                                  k ? &paov : nullptr, k ? prev.color.data() : nullptr,
                                                                  k ? prev.moments.data() : nullptr,
                                                                  clamp && k ? prev.fast.data() : nullptr, cur.color.data(),
                                                                  cur.moments.data(), clamp ? cur.fast.data() : nullptr,
                                                                  clamp ? shift.data() : nullptr, variance.data(), &tsec)
                       : clamp ? mcpt_temporal_accumulate_clamped(&tp, clamp, k ? &prev.cam : nullptr, W, H, hdr.data(), &aov,
                                                                k ? &paov : nullptr, k ? prev.color.data() : nullptr,
                                                                k ? prev.moments.data() : nullptr, k ? prev.fast.data() : nullptr,
                                                                cur.color.data(), cur.moments.data(), cur.fast.data(),
                                                                variance.data(), shift.data(), &tsec)
                             : mcpt_temporal_accumulate(&tp, k ? &prev.cam : nullptr, W, H, hdr.data(), &aov, k ? &paov : nullptr,
                                                        k ? prev.color.data() : nullptr, k ? prev.moments.data() : nullptr,
                                                        cur.color.data(), cur.moments.data(), variance.data(), &tsec);
        if (rc != MCPT_OK) {
            std::fprintf(stderr, "temporal accumulation failed: %s\n", mcpt_last_error());
            return 1;
        }
        size_t kept = 0;
        double nsum = 0;
        for (size_t p = 0; p < npx; p++) kept += cur.moments[4 * p + 2] > 1.5, nsum += cur.moments[4 * p + 2];
        std::printf("frame %d: orbit %g deg, seed %llu, %.3f s render, %.3f ms accumulate, %.1f%% of the pixels kept their "
                    "history (mean length %.2f)", k, k * a.orbit, (unsigned long long)(a.seed + k), st.seconds, tsec * 1e3,
                    100.0 * kept / npx, nsum / npx);
        if (clamp) {
            size_t moved = 0;
            for (size_t p = 0; p < npx; p++) moved += shift[p] != 0;
            std::printf(", the clamp moved %.1f%% of the pixels", 100.0 * moved / npx);
        }
        std::printf("\n");
        const std::vector<double>* shown = &cur.color;
        if (a.denoise) {
            double dsec = 0;
            if (mcpt_denoise(&dn, W, H, cur.color.data(), variance.data(), &aov, filtered.data(), nullptr, &dsec) != MCPT_OK) {
                std::fprintf(stderr, "denoise failed: %s\n", mcpt_last_error());
                return 1;
            }
            std::printf("  denoised: %d iterations, sigma_color %g, variance from the temporal moments, %.3f ms device\n",
                        dn.iterations, dn.sigma_color, dsec * 1e3);
            shown = &filtered;
        }
        if (!a.aov_out.empty()) {
            const std::string pre = frame_path(a.aov_out, k);
            if (!(write_pfm((pre + "_albedo.pfm").c_str(), cur.albedo, W, H) && write_pfm((pre + "_normal.pfm").c_str(), cur.normal, W, H) &&
                  write_pfm((pre + "_depth.pfm").c_str(), cur.depth, W, H, 1))) {
                std::fprintf(stderr, "cannot write %s_{albedo,normal,depth}.pfm\n", pre.c_str());
                return 1;
            }
        }
        if (up) {
            if (upsample_frame(scene, cur.cam, *up, *shown, aov, upsampled)) return 1;
            shown = &upsampled;
        }
        std::vector<uint8_t> rgb8(shown->size());
        mcpt_tone_map(shown->data(), SW, SH, 380.0, 0.25, rgb8.data());  // main.cpp:583
        if (mcpt_write_bmp(frame_path(a.out, k).c_str(), rgb8.data(), SW, SH) != MCPT_OK) {
            std::fprintf(stderr, "%s\n", mcpt_last_error());
            return 1;
        }
        if (!a.hdr_out.empty() && !write_pfm(frame_path(a.hdr_out, k).c_str(), *shown, SW, SH)) {
            std::fprintf(stderr, "cannot write %s\n", frame_path(a.hdr_out, k).c_str());
            return 1;
        }
    }
    return 0;
}

// --frames --device-sequence: the same sequence through mcpt_sequence; the lines and files of render_sequence
int render_sequence_device(mcpt_scene* scene, const mcpt_camera& cam0, const SequenceArgs& a, const mcpt_temporal_opts& tp,
                           const mcpt_temporal_clamp_opts* clamp, const mcpt_denoise_opts& dn, const mcpt_upsample_opts* up,
                           bool temporal_upsample) {
    const int W = up ? cam0.width * up->factor : cam0.width, H = up ? cam0.height * up->factor : cam0.height;  // the shown size
    const size_t npx = (size_t)W * H;
    mcpt_render_opts base;
    mcpt_render_opts_init(&base);
    base.mode = a.mode;
    base.accel = a.grid ? MCPT_ACCEL_GRID : MCPT_ACCEL_BVH;
    base.flags = a.flags;
    int last = -10;
    if (a.progress) {
        base.progress = print_progress;
        base.progress_user = &last;
    }
    mcpt_sequence_opts so;
    mcpt_sequence_opts_init(&so);
    so.width = cam0.width, so.height = cam0.height, so.spp = a.spp;
    so.denoise = a.denoise, so.clamp = clamp != nullptr;
    mcpt_sequence* seq = nullptr;
    if ((temporal_upsample ? mcpt_sequence_create_temporal_upsampled(scene, &base, &so, &tp, a.denoise ? &dn : nullptr, up, &seq)
         : up              ? mcpt_sequence_create_upsampled(scene, &base, &so, &tp, clamp, a.denoise ? &dn : nullptr, up, &seq)
                           : mcpt_sequence_create(scene, &base, &so, &tp, clamp, a.denoise ? &dn : nullptr, &seq)) != MCPT_OK) {
        std::fprintf(stderr, "sequence setup failed: %s\n", mcpt_last_error());
        return 1;
    }
    if (a.motion && mcpt_sequence_set_motion(seq, 1) != MCPT_OK) {
        std::fprintf(stderr, "sequence setup failed: %s\n", mcpt_last_error());
        mcpt_sequence_destroy(seq);
        return 1;
    }
    mcpt_gradient_opts go;
    mcpt_gradient_opts_init(&go);
    if (a.antilag) go.stratum = a.antilag;
    if (a.antilag && mcpt_sequence_set_antilag(seq, &go) != MCPT_OK) {
        std::fprintf(stderr, "sequence setup failed: %s\n", mcpt_last_error());
        mcpt_sequence_destroy(seq);
        return 1;
    }
    std::vector<uint8_t> rgb8(3 * npx);
    std::vector<double> shown;
    int rc = 0;
    for (int k = 0; k < a.frames && !rc; k++) {
        mcpt_camera cam;
        mcpt_sequence_info fi{};
        last = -10;
        if (a.motion && mcpt_scene_pose_save(scene) != MCPT_OK) {
            std::fprintf(stderr, "--motion failed: %s\n", mcpt_last_error());
            rc = 1;
            break;
        }
        if ((a.vis && a.vis->apply(scene, k)) || (a.move && a.move->apply(scene, k)) || (a.rotate && a.rotate->apply(scene, k)) ||
            (a.rebuild && a.rebuild->apply(scene, k)) || (a.relight && a.relight->apply(scene, k))) {
            rc = 1;
            break;
        }
        if (mcpt_camera_orbit(&cam0, k * a.orbit, &cam) != MCPT_OK ||
            mcpt_sequence_frame(seq, &cam, a.seed + k, rgb8.data(), &fi, nullptr) != MCPT_OK) {
            std::fprintf(stderr, "frame %d failed: %s\n", k, mcpt_last_error());
            rc = 1;
            break;
        }
        if (a.antilag) {
            int32_t ran = 0, pa = 0, pb = 0;
            double tsec = 0, mean = 0, mx = 0;
            if (mcpt_sequence_antilag_info(seq, &ran, &pa, &pb, &tsec, nullptr, &mean, &mx) != MCPT_OK) {
                std::fprintf(stderr, "%s\n", mcpt_last_error());
                rc = 1;
                break;
            }
            if (ran) print_antilag(go.stratum, pa, pb, mean, mx, tsec);
        }
        std::printf("frame %d: orbit %g deg, seed %llu, %.3f s render, %.3f ms accumulate, %.1f%% of the pixels kept their "
                    "history (mean length %.2f)", k, k * a.orbit, (unsigned long long)(a.seed + k), fi.render_seconds,
                    fi.temporal_seconds * 1e3, 100.0 * fi.kept, fi.mean_history);
        if (clamp) std::printf(", the clamp moved %.1f%% of the pixels", 100.0 * fi.clamped);
        std::printf("\n");
        if (a.denoise)
            std::printf("  denoised: %d iterations, sigma_color %g, variance from the temporal moments, %.3f ms device\n",
                        dn.iterations, dn.sigma_color, fi.denoise_seconds * 1e3);
        if (temporal_upsample) {
            int32_t pa = 0, pb = 0;
            double rsec = 0, filled = 0, share = 0;
            if (mcpt_sequence_temporal_upsample_info(seq, &pa, &pb, &rsec, &filled, &share) != MCPT_OK) {
                std::fprintf(stderr, "%s\n", mcpt_last_error());
                rc = 1;
                break;
            }
            std::printf("  upsampled: factor %d to %dx%d, %.2f%% of the pixels took the fallback, %.3f ms phase rays; phase (%d, %d), "
                        "%.2f%% of the pixels filled\n", up->factor, W, H, 100.0 * share, rsec * 1e3, pa, pb, 100.0 * filled);
        } else if (up) {
            double usec = 0, share = 0;
            if (mcpt_sequence_upsample_info(seq, nullptr, &usec, &share) != MCPT_OK) {
                std::fprintf(stderr, "%s\n", mcpt_last_error());
                rc = 1;
                break;
            }
            std::printf("  upsampled: factor %d to %dx%d, %.2f%% of the pixels took the fallback, %.3f ms device\n", up->factor, W, H,
                        100.0 * share, usec * 1e3);
        }
        if (mcpt_write_bmp(frame_path(a.out, k).c_str(), rgb8.data(), W, H) != MCPT_OK) {
            std::fprintf(stderr, "%s\n", mcpt_last_error());
            rc = 1;
        }
        if (!rc && !a.hdr_out.empty()) {
            shown.resize(3 * npx);
            if (mcpt_sequence_read(seq, up && !temporal_upsample ? MCPT_SEQ_UPSAMPLED : a.denoise ? MCPT_SEQ_FILTERED : MCPT_SEQ_ACCUMULATED,
                                   shown.data()) != MCPT_OK) {
                std::fprintf(stderr, "%s\n", mcpt_last_error());
                rc = 1;
            } else if (!write_pfm(frame_path(a.hdr_out, k).c_str(), shown, W, H)) {
                std::fprintf(stderr, "cannot write %s\n", frame_path(a.hdr_out, k).c_str());
                rc = 1;
            }
        }
    }
    mcpt_sequence_destroy(seq);
    return rc;
}

}  // namespace

int main(int argc, char** argv) {
    std::string scene_base = "scenes/veach-mis/veach-mis", out = "test.bmp", hdr_out;
    int W = 1280, H = 720, spp = 10, mode = MCPT_MODE_MIS;
    double dist_scale = 2.0;
    uint64_t seed = 20240430;
    bool xml_cam = false, progress = false, grid = false;
    int flags = 0;
    std::vector<int32_t> devices;
    bool adaptive = false;
    mcpt_adaptive_opts ad;
    mcpt_adaptive_opts_init(&ad);
    std::string count_out, aov_out;
    bool denoise = false;
    mcpt_denoise_opts dn;
    mcpt_denoise_opts_init(&dn);
    int frames = 0;
    double orbit = 0.0;
    bool sequence_flag = false;  // --orbit, --temporal-alpha or a clamp option seen
    mcpt_temporal_opts tp;
    mcpt_temporal_opts_init(&tp);
    bool history_clamp = false, clamp_flag = false;  // --history-clamp seen; --clamp-radius or --clamp-alpha-fast seen
    bool device_sequence = false;
    mcpt_temporal_clamp_opts tc;
    mcpt_temporal_clamp_opts_init(&tc);
    bool upsample = false, temporal_upsample = false;
    mcpt_upsample_opts up;
    mcpt_upsample_opts_init(&up);
    bool move_flag = false, motion_flag = false, rotate_flag = false, lights_movable_flag = false;
    bool antilag_flag = false, antilag_stratum_flag = false;
    int antilag_stratum = 3;
    Mover mover;
    Rotator rotator;
    bool rebuild_flag = false;
    Rebuilder rebuilder;
    Relighter relighter;
    Visibility visibility;
    for (int a = 1; a < argc; a++) {
        auto next = [&]() -> const char* {
            if (a + 1 >= argc) {
                std::fprintf(stderr, "missing value for %s\n", argv[a]);
                std::exit(2);
            }
            return argv[++a];
        };
        if (!std::strcmp(argv[a], "--scene")) scene_base = next();
        else if (!std::strcmp(argv[a], "--width")) W = std::atoi(next());
        else if (!std::strcmp(argv[a], "--height")) H = std::atoi(next());
        else if (!std::strcmp(argv[a], "--spp")) spp = std::atoi(next());
        else if (!std::strcmp(argv[a], "--mode")) {
            const char* m = next();
            if (!std::strcmp(m, "mis")) mode = MCPT_MODE_MIS;
            else if (!std::strcmp(m, "brdf")) mode = MCPT_MODE_BRDF;
            else if (!std::strcmp(m, "shade")) mode = MCPT_MODE_SHADE;
            else if (!std::strcmp(m, "shade-area")) mode = MCPT_MODE_SHADE_AREA;
            else {
                std::fprintf(stderr, "unknown --mode %s (mis, brdf, shade, shade-area)\n", m);
                return 2;
            }
        }
        else if (!std::strcmp(argv[a], "--seed")) seed = std::strtoull(next(), nullptr, 10);
        else if (!std::strcmp(argv[a], "--out")) out = next();
        else if (!std::strcmp(argv[a], "--hdr")) hdr_out = next();
        else if (!std::strcmp(argv[a], "--dist-scale")) dist_scale = std::atof(next());
        else if (!std::strcmp(argv[a], "--xml-camera")) xml_cam = true;
        else if (!std::strcmp(argv[a], "--progress")) progress = true;
        else if (!std::strcmp(argv[a], "--grid")) grid = true;
        else if (!std::strcmp(argv[a], "--jitter")) flags |= MCPT_RENDER_PIXEL_JITTER;
        else if (!std::strcmp(argv[a], "--precision")) {
            const char* v = next();
            if (!std::strcmp(v, "fp32")) flags |= MCPT_RENDER_PRECISION_FP32;
            else if (std::strcmp(v, "fp64")) {
                std::fprintf(stderr, "--precision: fp64 or fp32, not %s\n", v);
                return 2;
            }
        }
        else if (!std::strcmp(argv[a], "--adaptive")) {
            adaptive = true;
            ad.threshold = std::atof(next());
        }
        else if (!std::strcmp(argv[a], "--min-spp")) ad.min_spp = std::atoi(next());
        else if (!std::strcmp(argv[a], "--pass-spp")) ad.pass_spp = std::atoi(next());
        else if (!std::strcmp(argv[a], "--radius")) ad.radius = std::atoi(next());
        else if (!std::strcmp(argv[a], "--count-out")) count_out = next();
        else if (!std::strcmp(argv[a], "--denoise")) denoise = true;
        else if (!std::strcmp(argv[a], "--denoise-iterations")) dn.iterations = std::atoi(next());
        else if (!std::strcmp(argv[a], "--denoise-sigma-color")) dn.sigma_color = std::atof(next());
        else if (!std::strcmp(argv[a], "--aov-out")) aov_out = next();
        else if (!std::strcmp(argv[a], "--frames")) {
            frames = std::atoi(next());
            if (frames < 1) {
                std::fprintf(stderr, "--frames needs a count >= 1\n");
                return 2;
            }
        }
        else if (!std::strcmp(argv[a], "--orbit")) orbit = std::atof(next()), sequence_flag = true;
        else if (!std::strcmp(argv[a], "--temporal-alpha")) tp.alpha = std::atof(next()), sequence_flag = true;
        else if (!std::strcmp(argv[a], "--history-clamp")) tc.sigma = std::atof(next()), history_clamp = sequence_flag = true;
        else if (!std::strcmp(argv[a], "--clamp-radius")) tc.radius = std::atoi(next()), clamp_flag = sequence_flag = true;
        else if (!std::strcmp(argv[a], "--clamp-alpha-fast")) tc.alpha_fast = std::atof(next()), clamp_flag = sequence_flag = true;
        else if (!std::strcmp(argv[a], "--device-sequence")) device_sequence = true;
        else if (!std::strcmp(argv[a], "--upsample")) up.factor = std::atoi(next()), upsample = true;
        else if (!std::strcmp(argv[a], "--temporal-upsample")) temporal_upsample = true;
        else if (!std::strcmp(argv[a], "--move")) {
            if (!mover.parse(next())) {
                std::fprintf(stderr, "--move needs FIRST:COUNT:DX,DY,DZ (a facet range and a finite step per frame), not %s\n", argv[a]);
                return 2;
            }
            move_flag = true;
        }
        else if (!std::strcmp(argv[a], "--rotate")) {
            if (!rotator.parse(next())) {
                std::fprintf(stderr, "--rotate needs FIRST:COUNT:AX,AY,AZ:DEG:PX,PY,PZ (a facet range, an axis of length > 0, finite "
                                     "degrees per frame and a pivot), not %s\n", argv[a]);
                return 2;
            }
            rotate_flag = true;
        }
        else if (!std::strcmp(argv[a], "--rebuild")) {
            if (!rebuilder.parse(next())) {
                std::fprintf(stderr, "--rebuild needs RATIO, a finite number > 1 (rebuild once the tree's cost exceeds RATIO x the "
                                     "cost at the last build), not %s\n", argv[a]);
                return 2;
            }
            rebuild_flag = true;
        }
        else if (!std::strcmp(argv[a], "--dim")) {
            if (!relighter.parse_dim(next())) {
                std::fprintf(stderr, "--dim needs GROUP:FACTOR (a light group and a finite factor >= 0 per frame), not %s\n", argv[a]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[a], "--tint")) {
            if (!relighter.parse_tint(next())) {
                std::fprintf(stderr, "--tint needs MATERIAL:R,G,B (a row of the material table and a finite Kd >= 0), not %s\n", argv[a]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[a], "--hide") || !std::strcmp(argv[a], "--show")) {
            const char* opt = argv[a];
            if (!visibility.parse(next(), !std::strcmp(opt, "--show"))) {
                std::fprintf(stderr, "%s needs FIRST:COUNT[:FRAME] (a facet range and the 0-based frame it takes effect before), not %s\n",
                             opt, argv[a]);
                return 2;
            }
        }
        else if (!std::strcmp(argv[a], "--motion")) motion_flag = true;
        else if (!std::strcmp(argv[a], "--antilag")) antilag_flag = true;
        else if (!std::strcmp(argv[a], "--antilag-stratum")) antilag_stratum = std::atoi(next()), antilag_stratum_flag = true;
        else if (!std::strcmp(argv[a], "--lights-movable")) lights_movable_flag = true;
        else if (!std::strcmp(argv[a], "--devices")) {
            for (const char* p = next(); *p;) {
                char* e = nullptr;
                devices.push_back((int32_t)std::strtol(p, &e, 10));
                if (e == p) {
                    std::fprintf(stderr, "bad --devices list\n");
                    return 2;
                }
                p = *e == ',' ? e + 1 : e;
            }
        }
        else {
            std::fprintf(stderr, "unknown option %s\n", argv[a]);
            return 2;
        }
    }
    if (flags & MCPT_RENDER_PIXEL_JITTER) {  // refused before anything is loaded
        if (adaptive) {
            std::fprintf(stderr, "--jitter needs plain renders; drop --adaptive\n");
            return 2;
        }
        if (grid) {
            std::fprintf(stderr, "--jitter traces its camera rays over the BVH; drop --grid\n");
            return 2;
        }
    }
    if (!visibility.edits.empty()) {  // refused before anything is loaded
        if (grid) {
            std::fprintf(stderr, "--hide and --show are not supported with --grid: the reference grid's in-cell rule depends on the "
                                 "scene's box, so a grid without the hidden facets would not be the reference's; drop --grid\n");
            return 2;
        }
        for (const Visibility::Edit& e : visibility.edits)
            if (e.frame >= std::max(frames, 1)) {
                std::fprintf(stderr, "--%s %d:%d:%d: frame %d is not one of the run's %d (0-based)\n", e.visible ? "show" : "hide", e.first,
                             e.count, e.frame, e.frame, std::max(frames, 1));
                return 2;
            }
    }
    if (move_flag && frames == 0) {  // refused before anything is loaded
        std::fprintf(stderr, "--move moves facets between the frames of a sequence; add --frames N\n");
        return 2;
    }
    if (rotate_flag && (frames == 0 || move_flag)) {  // refused before anything is loaded
        std::fprintf(stderr, "--rotate %s\n", frames == 0 ? "rotates facets between the frames of a sequence; add --frames N"
                                                          : "and --move both rewrite their facets from an original pose; give one of them");
        return 2;
    }
    if (rebuild_flag && (frames == 0 || !(move_flag || rotate_flag))) {  // refused before anything is loaded
        std::fprintf(stderr, "--rebuild rebuilds the tree that moves between the frames of a sequence degrade; add %s\n",
                     frames == 0 ? "--frames N" : "--move or --rotate");
        return 2;
    }
    if (lights_movable_flag && (frames == 0 || !(move_flag || rotate_flag))) {  // refused before anything is loaded
        std::fprintf(stderr, "--lights-movable lets the moves between the frames of a sequence take light triangles along; add %s\n",
                     frames == 0 ? "--frames N" : "--move or --rotate");
        return 2;
    }
    const bool relight_flag = !relighter.dims.empty() || !relighter.tints.empty();
    if (relight_flag && frames == 0) {  // refused before anything is loaded
        std::fprintf(stderr, "--dim and --tint re-light the scene between the frames of a sequence; add --frames N\n");
        return 2;
    }
    if (motion_flag && (frames == 0 || upsample)) {  // refused before anything is loaded
        std::fprintf(stderr, "--motion %s\n", frames == 0 ? "follows moved facets through the history of a sequence; add --frames N"
                                                          : "is not supported with upsampling; drop --upsample");
        return 2;
    }
    if (antilag_stratum_flag && !antilag_flag) {  // refused before anything is loaded
        std::fprintf(stderr, "--antilag-stratum sets the stratum of --antilag; add --antilag\n");
        return 2;
    }
    if (antilag_flag) {  // refused before anything is loaded
        const char* why = frames == 0 ? "drops stale history in a sequence; add --frames N"
                          : antilag_stratum < 1 || antilag_stratum > 8 ? "needs an --antilag-stratum in 1..8"
                          : (flags & MCPT_RENDER_PIXEL_JITTER) ? "traces its gradient samples through the pixels' centres; drop --jitter"
                          : grid     ? "traces its gradient samples over the BVH; drop --grid"
                          : upsample ? "is not supported with upsampling; drop --upsample"
                                     : nullptr;
        if (why) {
            std::fprintf(stderr, "--antilag %s\n", why);
            return 2;
        }
    }
    if (temporal_upsample) {  // refused before anything is loaded
        const char* why = !upsample          ? "accumulates at --upsample F times the traced size; add --upsample F"
                          : !device_sequence ? "runs in the device-resident sequence; add --frames N --device-sequence"
                          : history_clamp    ? "has no history clamp; drop --history-clamp"
                          : (flags & MCPT_RENDER_PIXEL_JITTER) ? "traces through the full-size pixels' centres; drop --jitter"
                          : grid             ? "traces its rays over the BVH; drop --grid"
                          : adaptive         ? "accumulates plain samples; drop --adaptive"
                                             : nullptr;
        if (why) {
            std::fprintf(stderr, "--temporal-upsample %s\n", why);
            return 2;
        }
    }
    if (upsample) {  // refused before anything is loaded
        if (up.factor < 2 || up.factor > 4) {
            std::fprintf(stderr, "--upsample needs a factor in 2..4, not %d\n", up.factor);
            return 2;
        }
        if (adaptive) {
            std::fprintf(stderr, "--upsample reconstructs plain renders; drop --adaptive\n");
            return 2;
        }
        if (grid) {
            std::fprintf(stderr, "--upsample takes its guides over the BVH; drop --grid\n");
            return 2;
        }
        if (!aov_out.empty()) {
            std::fprintf(stderr, "--upsample has guides at two sizes; drop --aov-out\n");
            return 2;
        }
        if (W < 1 || H < 1 || W % up.factor || H % up.factor) {
            std::fprintf(stderr, "--upsample %d: --width %d and --height %d are the shown size and must be divisible by %d\n",
                         up.factor, W, H, up.factor);
            return 2;
        }
    }
    if (device_sequence) {  // refused before anything is loaded
        if (frames == 0) {
            std::fprintf(stderr, "--device-sequence needs --frames\n");
            return 2;
        }
        if (adaptive) {
            std::fprintf(stderr, "--device-sequence runs plain renders; drop --adaptive\n");
            return 2;
        }
        if (!aov_out.empty()) {
            std::fprintf(stderr, "--device-sequence keeps the guides on the device; drop --aov-out\n");
            return 2;
        }
        if (!devices.empty()) {
            std::fprintf(stderr, "--device-sequence runs on one device; drop --devices\n");
            return 2;
        }
    }
    mcpt_scene* scene = nullptr;
    if (mcpt_scene_load((scene_base + ".obj").c_str(), (scene_base + ".xml").c_str(), &scene) != MCPT_OK) {
        std::fprintf(stderr, "scene load failed: %s\n", mcpt_last_error());
        return 1;
    }
    int32_t nf, nm, nl;
    mcpt_scene_counts(scene, &nf, &nm, &nl);
    std::printf("facets %d, materials %d, light triangles %d\n", nf, nm, nl);
    mcpt_camera cam{};
    if (!xml_cam || mcpt_scene_camera(scene, &cam) != MCPT_OK) {  // main.cpp:507-510
        const double eye[3] = {28.2792, 5.2, 1.23612e-06}, look[3] = {0.0, 2.8, 0.0}, up[3] = {0, 1, 0};
        std::memcpy(cam.eye, eye, sizeof eye);
        std::memcpy(cam.lookat, look, sizeof look);
        std::memcpy(cam.up, up, sizeof up);
        cam.fovy = 20.1143;
    }
    cam.dist_scale = dist_scale;
    const int SW = W, SH = H;  // the shown size; W x H from here on is the render's
    if (upsample) W /= up.factor, H /= up.factor;
    cam.width = W;
    cam.height = H;
    std::vector<double> hdr;
    mcpt_stats st{};
    std::vector<int32_t> count;
    std::vector<double> noise;
    if (adaptive && !devices.empty()) {
        std::fprintf(stderr, "--adaptive renders on one device; drop --devices\n");
        return 2;
    }
    if (!adaptive && !count_out.empty()) {
        std::fprintf(stderr, "--count-out needs --adaptive\n");
        return 2;
    }
    if (sequence_flag && frames == 0) {
        std::fprintf(stderr, "--orbit, --temporal-alpha and --history-clamp need --frames\n");
        return 2;
    }
    if (frames > 0) {
        if (adaptive) {
            std::fprintf(stderr, "--frames accumulates plain renders; drop --adaptive\n");
            return 2;
        }
        if (lights_movable_flag && mcpt_scene_set_lights_movable(scene, 1) != MCPT_OK) {
            std::fprintf(stderr, "--lights-movable failed: %s\n", mcpt_last_error());
            return 1;
        }
        if (move_flag) {
            if (const int rc = mover.bind(scene)) return rc;
        }
        if (rotate_flag) {
            if (const int rc = rotator.bind(scene)) return rc;
        }
        if (relight_flag) {
            if (const int rc = relighter.bind(scene)) return rc;
        }
        const SequenceArgs sa{frames, spp, mode, flags, orbit, seed, progress, grid, denoise, out, hdr_out, aov_out,
                              move_flag ? &mover : nullptr, motion_flag, rotate_flag ? &rotator : nullptr,
                              rebuild_flag ? &rebuilder : nullptr, relight_flag ? &relighter : nullptr,
                              antilag_flag ? antilag_stratum : 0, visibility.edits.empty() ? nullptr : &visibility};
        if (clamp_flag && !history_clamp) {
            std::fprintf(stderr, "--clamp-radius and --clamp-alpha-fast need --history-clamp\n");
            return 2;
        }
        const mcpt_upsample_opts* upp = upsample ? &up : nullptr;
        const int rc = device_sequence ? render_sequence_device(scene, cam, sa, tp, history_clamp ? &tc : nullptr, dn, upp, temporal_upsample)
                                       : render_sequence(scene, cam, sa, devices, tp, history_clamp ? &tc : nullptr, dn, upp);
        mcpt_scene_destroy(scene);
        return rc;
    }
    if (visibility.apply(scene, 0)) return 1;
    ad.max_spp = spp;
    const auto t0 = std::chrono::steady_clock::now();
    if ((adaptive ? render_adaptive(scene, cam, ad, mode, seed, progress, grid, flags, hdr, count, noise, &st)
                  : render(scene, cam, spp, mode, seed, progress, grid, flags, devices, hdr, &st)) != MCPT_OK) {
        std::fprintf(stderr, "render failed: %s\n", mcpt_last_error());
        return 1;
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("%dx%d @ %d spp (%s): %.3f s wall, %.3f s device, %.2f Msamples/s on %d device(s)\n", W, H, spp,
                mode == MCPT_MODE_MIS ? "MIS" : mode == MCPT_MODE_BRDF ? "BRDF" : mode == MCPT_MODE_SHADE ? "shade" : "shade-area",
                sec, st.seconds,
                st.camera_samples / st.seconds * 1e-6, st.devices_used);
    if (st.devices_used > 1) {  // where a multi-device call's time went
        std::printf("  comm init %.3f s, device setup %.3f s (max), reduce %.4f s; per device:", st.comm_init_seconds,
                    st.device_setup_seconds, st.reduce_seconds);
        for (int u = 0; u < st.devices_used && u < MCPT_STATS_MAX_DEVICES; u++) std::printf(" %.3f", st.device_seconds[u]);
        std::printf(" s\n");
    }
    if (adaptive) {
        size_t capped = 0;
        for (int32_t c : count) capped += c >= spp;
        std::printf("  adaptive (threshold %g, min %d, pass %d, radius %d): mean %.2f spp of at most %d, %.1f%% of the pixels "
                    "at the cap\n", ad.threshold, ad.min_spp, ad.pass_spp, ad.radius, (double)st.camera_samples / count.size(),
                    spp, 100.0 * capped / count.size());
        if (!count_out.empty()) {  // grey: 255 = the cap
            std::vector<uint8_t> grey(3 * count.size());
            for (size_t k = 0; k < count.size(); k++)
                grey[3 * k] = grey[3 * k + 1] = grey[3 * k + 2] = (uint8_t)(255ll * count[k] / spp);
            if (mcpt_write_bmp(count_out.c_str(), grey.data(), W, H) != MCPT_OK) {
                std::fprintf(stderr, "%s\n", mcpt_last_error());
                return 1;
            }
        }
    }
    if (denoise || !aov_out.empty() || upsample) {
        const size_t npx = (size_t)W * H;
        std::vector<double> albedo(3 * npx), normal(3 * npx), position(3 * npx), depth(npx);
        const mcpt_aov_buffers aov{albedo.data(), normal.data(), position.data(), depth.data()};
        mcpt_render_opts ao;
        mcpt_render_opts_init(&ao);
        ao.accel = grid ? MCPT_ACCEL_GRID : MCPT_ACCEL_BVH;
        if (mcpt_render_aovs(scene, &cam, &ao, &aov) != MCPT_OK) {
            std::fprintf(stderr, "AOV render failed: %s\n", mcpt_last_error());
            return 1;
        }
        if (!aov_out.empty() && !(write_pfm((aov_out + "_albedo.pfm").c_str(), albedo, W, H) &&
                                  write_pfm((aov_out + "_normal.pfm").c_str(), normal, W, H) &&
                                  write_pfm((aov_out + "_depth.pfm").c_str(), depth, W, H, 1))) {
            std::fprintf(stderr, "cannot write %s_{albedo,normal,depth}.pfm\n", aov_out.c_str());
            return 1;
        }
        if (denoise) {
            // adaptive: the noise map as the variance of the pixel's mean luminance; else the spatial estimate
            std::vector<double> variance, filtered(3 * npx);
            if (adaptive) {
                variance.resize(npx);
                mcpt_variance_from_noise(W, H, hdr.data(), noise.data(), variance.data());
            }
            double dsec = 0;
            if (mcpt_denoise(&dn, W, H, hdr.data(), adaptive ? variance.data() : nullptr, &aov, filtered.data(), nullptr,
                             &dsec) != MCPT_OK) {
                std::fprintf(stderr, "denoise failed: %s\n", mcpt_last_error());
                return 1;
            }
            hdr.swap(filtered);
            std::printf("  denoised: %d iterations, sigma_color %g, variance from %s, %.3f ms device\n", dn.iterations,
                        dn.sigma_color, adaptive ? "the adaptive noise map" : "the spatial estimate", dsec * 1e3);
        }
        if (upsample) {
            std::vector<double> full;
            if (upsample_frame(scene, cam, up, hdr, aov, full)) return 1;
            hdr.swap(full);
        }
    }
    std::vector<uint8_t> rgb8(hdr.size());
    mcpt_tone_map(hdr.data(), SW, SH, 380.0, 0.25, rgb8.data());  // main.cpp:583
    if (mcpt_write_bmp(out.c_str(), rgb8.data(), SW, SH) != MCPT_OK) {
        std::fprintf(stderr, "%s\n", mcpt_last_error());
        return 1;
    }
    if (!hdr_out.empty() && !write_pfm(hdr_out.c_str(), hdr, SW, SH)) {
        std::fprintf(stderr, "cannot write %s\n", hdr_out.c_str());
        return 1;
    }
    mcpt_scene_destroy(scene);
    return 0;
}
