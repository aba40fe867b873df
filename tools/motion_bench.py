#!/usr/bin/env python3
"""What object motion in the temporal accumulation costs and buys (profiles/motion_benches.txt).

One MI355X, one process, the arms taking turns repetition by repetition after one warm-up round; medians are what
README.md and DESIGN.md 4.20 quote:
  motion_aovs   the motion stage of a frame sequence at 800x600 (mcpt_sequence_motion_info: HIP events around
                k_motion_aovs, its launch and its stream synchronisation included) beside the AOV stage's window
  accumulate    mcpt_temporal_accumulate_motion_device against mcpt_temporal_accumulate_device (plain) and
                mcpt_temporal_accumulate_clamped_device (clamped) at 800x600, device seconds (HIP events around the
                kernels), on the guides and history of two rendered frames 1.5 degrees apart; the motion arrays are
                the current position and normal (the work does not depend on their values)
  pose_save     Scene.pose_save on Cornell + 1 M random triangles with one device state: wall time (the call ends in a
                stream synchronisation); the first call, which allocates, is reported apart
  sequence      eight 4-spp 800x600 frames, plate 2 of the Veach stand-in (facets [36, 48)) moved 0.5 along its top
                normal per frame, seen from above (tests/test_motion_cpu.py's camera), FrameSequence with denoise,
                motion on against motion off: wall time per frame (pose save, update and frame) and the relative MSE
                of the shown frame over the plate's pixels (and over the rest) against an independent 1024-spp frame
                of the last pose; once in MIS and once BRDF-only (no light sampling: a noisier frame)
  bench         with --parent-lib PATH (a libmcpt_hip.so built from the parent commit): bench.py --gpus 1 --steps 3
                --warmup 1 with this tree's library and with the parent's, taking turns, three runs each
Prints one JSON line; --append adds it to profiles/motion_benches.txt.

  python tools/motion_bench.py [--parent-lib PATH] [--append]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import monte_carlo_path_tracing_amd as mcpt  # noqa: E402

W, H, SPP, SEED = 800, 600, 4, mcpt.DEFAULT_SEED
PLATE = (36, 48)
KEYS = ("albedo", "normal", "position", "depth")
VEACH = os.path.join(ROOT, "scenes", "veach-mis", "veach-mis")
med = statistics.median


def cornell(triangles):
    d = os.path.join(tempfile.gettempdir(), "mcpt_cornell_%d_20240430" % triangles)
    obj, xml = d + "/cornell-random.obj", d + "/cornell-random.xml"
    if not (os.path.exists(obj) and os.path.exists(xml)):
        subprocess.run([sys.executable, os.path.join(ROOT, "scenes", "gen_cornell_random.py"), "--triangles", str(triangles),
                        "--seed", "20240430", d], check=True, capture_output=True)
    return obj, xml


def fresh(arr):
    return mcpt.Scene.create(arr["positions"], arr["normals"], arr["material_id"], arr["materials"], arr["light_facet"],
                             arr["light_radiance"])


def plate_camera():
    c = mcpt.Camera()
    c.eye[:], c.lookat[:], c.up[:] = (10.0, 14.0, 0.0), (-0.5, 2.85, 0.0), (0.0, 1.0, 0.0)
    c.fovy, c.dist_scale, c.width, c.height = 60.0, 1.0, W, H
    return c


def plate_pose(arr, k):
    n = arr["unique_normal"][PLATE[0]:PLATE[1]]
    step = 0.5 * n[np.argmax(n[:, 1])]
    return (arr["positions"][PLATE[0]:PLATE[1]].astype(np.float64) + np.tile(k * step, 3)).astype(np.float32)


def rel_mse(a, ref, mask):
    d = (a - ref)[mask]
    return float(np.mean((d * d).sum(-1) / ((ref[mask] * ref[mask]).sum(-1) + 1e-2)))


def bench_motion_aovs(reps):
    scene = mcpt.Scene.load(VEACH + ".obj", VEACH + ".xml")
    seq = mcpt.FrameSequence(scene, W, H, 1, denoise=False, motion=True)
    ms, aov = [], []
    for rep in range(reps + 1):
        scene.pose_save()
        seq.frame(mcpt.camera_orbit(mcpt.Camera.reference(W, H), 0.3 * rep), SEED + rep, readback=False)
        if rep:
            ms.append(seq.motion_info() * 1e3), aov.append(seq.info.aov_seconds * 1e3)
    seq.close()
    return {"motion_stage_ms": ms, "median_motion_stage_ms": med(ms), "median_aov_stage_ms": med(aov)}


def bench_accumulate(reps):
    import torch
    scene = mcpt.Scene.load(VEACH + ".obj", VEACH + ".xml")
    cams = [mcpt.camera_orbit(mcpt.Camera.reference(W, H), 1.5 * k) for k in range(2)]
    imgs = [mcpt.render(scene, c, SPP, seed=SEED + k)[0] for k, c in enumerate(cams)]
    aovs = [mcpt.render_aovs(scene, c) for c in cams]
    c0, m0, f0, _, _, _ = mcpt.temporal_accumulate_clamped(imgs[0], aovs[0])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptrs = lambda d: {k: a.data_ptr() for k, a in d.items()}
    g0, g1 = ({k: t(a[k]) for k in KEYS} for a in aovs)
    mo = {"prev_position": t(aovs[1]["position"]), "prev_normal": t(aovs[1]["normal"])}
    img, dc0, dm0, df0 = t(imgs[1]), t(c0), t(m0), t(f0)
    f64 = dict(dtype=torch.float64, device="cuda")
    o, m, f, v, s = (torch.zeros(sh, **f64) for sh in ((H, W, 3), (H, W, 4), (H, W, 3), (H, W), (H, W)))
    prev = (cams[0], ptrs(g0), dc0.data_ptr(), dm0.data_ptr())
    prevc = prev + (df0.data_ptr(),)
    torch.cuda.synchronize()
    arms = {
        "plain": lambda: mcpt.temporal_accumulate_device(W, H, img.data_ptr(), ptrs(g1), o.data_ptr(), m.data_ptr(), v.data_ptr(), prev=prev),
        "plain_motion": lambda: mcpt.temporal_accumulate_motion_device(W, H, img.data_ptr(), ptrs(g1), ptrs(mo), o.data_ptr(), m.data_ptr(),
                                                                       None, v.data_ptr(), None, prev=prev),
        "clamped": lambda: mcpt.temporal_accumulate_clamped_device(W, H, img.data_ptr(), ptrs(g1), o.data_ptr(), m.data_ptr(), f.data_ptr(),
                                                                   v.data_ptr(), s.data_ptr(), prev=prevc, clamp=True),
        "clamped_motion": lambda: mcpt.temporal_accumulate_motion_device(W, H, img.data_ptr(), ptrs(g1), ptrs(mo), o.data_ptr(), m.data_ptr(),
                                                                         f.data_ptr(), v.data_ptr(), s.data_ptr(), prev=prevc, clamp=True),
    }
    ms = {k: [] for k in arms}
    for rep in range(reps + 1):
        for k, fn in arms.items():
            sec = fn()
            if rep:
                ms[k].append(sec * 1e3)
    out = {k + "_ms": v for k, v in ms.items()}
    out.update({"median_" + k + "_ms": med(v) for k, v in ms.items()})
    out["plain_motion_over_plain"] = med(ms["plain_motion"]) / med(ms["plain"])
    out["clamped_motion_over_clamped"] = med(ms["clamped_motion"]) / med(ms["clamped"])
    return out


def bench_pose_save(triangles, reps):
    obj, xml = cornell(triangles)
    scene = mcpt.Scene.load(obj, xml)
    mcpt.primary_hits(scene, mcpt.Camera.reference(8, 6))  # one device state
    ms = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        scene.pose_save()
        ms.append((time.perf_counter() - t0) * 1e3)
    n = scene.nfacets
    scene.close()
    return {"facets": n, "first_call_ms": ms[0], "wall_ms": ms[1:], "median_wall_ms": med(ms[1:]),
            "bytes_copied": n * (3 * 16 + 9 * 4) * 2}  # device to device (read + written) beside the host copy


def bench_sequence(frames, reps, ref_spp, mode):
    arr = mcpt.Scene.load(VEACH + ".obj", VEACH + ".xml").arrays()
    cam = plate_camera()
    last = dict(arr, positions=arr["positions"].copy())
    last["positions"][PLATE[0]:PLATE[1]] = plate_pose(arr, frames - 1)
    ref_scene = fresh(last)
    ref = mcpt.render(ref_scene, cam, ref_spp, mode=mode, seed=SEED + 1000)[0]
    f, _ = mcpt.primary_hits(ref_scene, cam)
    plate = ((f >= PLATE[0]) & (f < PLATE[1])).reshape(H, W)
    arms = {False: {"frame_wall_ms": [], "plate_rel_mse": None}, True: {"frame_wall_ms": [], "plate_rel_mse": None}}
    for rep in range(reps + 1):
        for motion, res in arms.items():
            scene = fresh(arr)
            seq = mcpt.FrameSequence(scene, W, H, SPP, mode=mode, denoise=True, motion=motion)
            walls = []
            for k in range(frames):
                t0 = time.perf_counter()
                if motion:
                    scene.pose_save()
                if k:
                    scene.update(PLATE[0], plate_pose(arr, k))
                seq.frame(cam, SEED + k)
                walls.append((time.perf_counter() - t0) * 1e3)
            shown, n = seq.read("filtered"), seq.read("moments")[..., 2]
            seq.close()
            scene.close()
            if rep:
                res["frame_wall_ms"].append(med(walls[1:]))
                res.update(plate_rel_mse=rel_mse(shown, ref, plate), rest_rel_mse=rel_mse(shown, ref, ~plate),
                           plate_mean_history=float(n[plate].mean()))
    for res in arms.values():
        res["median_frame_wall_ms"] = med(res["frame_wall_ms"])
    return {"mode": mode, "frames": frames, "spp": SPP, "reference_spp": ref_spp, "plate_pixels": int(plate.sum()), "motion_off": arms[False],
            "motion_on": arms[True], "plate_rel_mse_off_over_on": arms[False]["plate_rel_mse"] / arms[True]["plate_rel_mse"]}


def bench_headline(parent_lib, runs):
    arms = {"this": None, "parent": parent_lib}
    vals = {k: [] for k in arms}
    for _ in range(runs):
        for k, lib in arms.items():
            env = dict(os.environ)
            if lib:
                env["MCPT_LIB_PATH"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], env=env,
                               capture_output=True, text=True, check=True)
            vals[k].append(json.loads(r.stdout.strip().splitlines()[-1])["value"])
    return {"msamples_per_s": vals, "median_this": med(vals["this"]), "median_parent": med(vals["parent"]),
            "this_over_parent": med(vals["this"]) / med(vals["parent"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--parent-lib", default="", help="libmcpt_hip.so of the parent commit: adds the bench.py comparison")
    ap.add_argument("--parts", default="motion_aovs,accumulate,pose_save,sequence,sequence_brdf",
                    help="comma-separated: which measurements to run")
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/motion_benches.txt")
    a = ap.parse_args()
    res = {"label": a.label, "size": "%dx%d" % (W, H), "reps": a.reps}
    parts = a.parts.split(",")
    if "motion_aovs" in parts:
        res["motion_aovs"] = bench_motion_aovs(a.reps)
    if "accumulate" in parts:
        res["accumulate"] = bench_accumulate(a.reps)
    if "pose_save" in parts:
        res["pose_save"] = bench_pose_save(a.triangles, a.reps)
    if "sequence" in parts:
        res["sequence"] = bench_sequence(a.frames, 2, a.reference_spp, "mis")
    if "sequence_brdf" in parts:
        res["sequence_brdf"] = bench_sequence(a.frames, 2, a.reference_spp, "brdf")
    if a.parent_lib:
        res["bench"] = bench_headline(a.parent_lib, 3)
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "motion_benches.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
