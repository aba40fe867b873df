#!/usr/bin/env python3
"""What anti-lag by temporal gradients costs and buys (profiles/antilag_benches.txt).

One MI355X, one process, 800x600 at 4 spp, MIS, the Veach stand-in, three FrameSequence arms taking turns frame by
frame: anti-lag off, stratum 3 and stratum 2 (radius 1); medians are what README.md and DESIGN.md 4.25 quote:
  cost      eight frames after a warm-up frame along a 0.3 degree orbit, denoise on: wall time per frame (the whole
            mcpt_sequence_frame call, no read-back), the main render's device seconds, and of the gradient pass
            trace_seconds (the gradient render's mcpt_stats.seconds) and kernel_seconds (the ray, gradient and
            reduction kernels, HIP events); the overhead is each arm's median wall time over the off arm's, beside
            the 1 / stratum^2 share of the frame's samples the pass traces
  error     a static reference camera, six frames, then the big light's group dimmed to a tenth
            (Scene.set_group_radiance) and three more: the relative L2 of the raw and the accumulated frame against
            an independent 1024-spp frame (seed 777) of the dimmed scene, for each arm, with Lambda's mean and maximum
  bench     with --parent-lib PATH (a libmcpt_hip.so built from the parent commit): bench.py --gpus 1 --steps 3
            --warmup 1 --no-cpu with this tree's library and with the parent's, taking turns, three runs each
Prints one JSON line; --append adds it to profiles/antilag_benches.txt.

  python tools/antilag_bench.py [--parent-lib PATH] [--append]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import monte_carlo_path_tracing_amd as mcpt  # noqa: E402

W, H, SPP, SEED = 800, 600, 4, mcpt.DEFAULT_SEED
VEACH = os.path.join(ROOT, "scenes", "veach-mis", "veach-mis")
ARMS = {"off": None, "stratum3": dict(stratum=3, radius=1), "stratum2": dict(stratum=2, radius=1)}
med = statistics.median


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def bench_cost(frames):
    scene = mcpt.Scene.load(VEACH + ".obj", VEACH + ".xml")
    seqs = {k: mcpt.FrameSequence(scene, W, H, SPP, mode="mis", denoise=True, antilag=v) for k, v in ARMS.items()}
    out = {k: dict(frame_wall_ms=[], render_ms=[], trace_ms=[], kernel_ms=[], lambda_max=[]) for k in ARMS}
    for k in range(frames + 1):  # frame 0 warms up (and has no gradient pass)
        cam = mcpt.camera_orbit(mcpt.Camera.reference(W, H), 0.3 * k)
        for name, seq in seqs.items():
            t0 = time.perf_counter()
            seq.frame(cam, SEED + k, readback=False)
            wall = time.perf_counter() - t0
            if k == 0:
                continue
            r = out[name]
            r["frame_wall_ms"].append(1e3 * wall)
            r["render_ms"].append(1e3 * seq.info.render_seconds)
            if ARMS[name] is not None:
                info = seq.antilag_info()
                assert info["ran"]
                r["trace_ms"].append(1e3 * info["trace_seconds"])
                r["kernel_ms"].append(1e3 * info["kernel_seconds"])
                r["lambda_max"].append(info["lambda_max"])
    for seq in seqs.values():
        seq.close()
    for name, r in out.items():
        for key in ("frame_wall_ms", "render_ms", "trace_ms", "kernel_ms"):
            if r[key]:
                r["median_" + key] = med(r[key])
    off = out["off"]["median_frame_wall_ms"]
    for name, v in ARMS.items():
        if v is not None:
            out[name]["wall_over_off"] = out[name]["median_frame_wall_ms"] / off
            out[name]["trace_over_render"] = out[name]["median_trace_ms"] / out[name]["median_render_ms"]
            out[name]["sample_share"] = 1.0 / v["stratum"] ** 2
    return out


def bench_error(before, after, ref_spp):
    cam = mcpt.Camera.reference(W, H)
    res, ref = {}, None
    for name, v in ARMS.items():
        scene = mcpt.Scene.load(VEACH + ".obj", VEACH + ".xml")
        big = int(scene.light_groups()[np.flatnonzero(np.all(scene.arrays()["light_radiance"] == 10.0, -1))[0]])
        seq = mcpt.FrameSequence(scene, W, H, SPP, mode="mis", denoise=False, antilag=v)
        rows = []
        for k in range(before + after):
            if k == before:
                scene.set_group_radiance(big, (1.0, 1.0, 1.0))
                if ref is None:
                    ref = mcpt.render(scene, cam, ref_spp, mode="mis", seed=777)[0]
            seq.frame(cam, SEED + k, readback=False)
            if k >= before:
                row = dict(frame=k, raw=rel_l2(seq.read("raw"), ref), accumulated=rel_l2(seq.read("accumulated"), ref))
                if v is not None:
                    info = seq.antilag_info()
                    row.update(lambda_mean=info["lambda_mean"], lambda_max=info["lambda_max"])
                rows.append(row)
        seq.close()
        res[name] = rows
    return {"frames_before": before, "reference_spp": ref_spp, "arms": res}


def bench_headline(parent_lib, runs):
    arms = {"this": None, "parent": parent_lib}
    vals = {k: [] for k in arms}
    for _ in range(runs):
        for k, lib in arms.items():
            env = dict(os.environ)
            if lib:
                env["MCPT_LIB_PATH"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu"],
                               env=env, capture_output=True, text=True, check=True, timeout=300)
            vals[k].append(json.loads(r.stdout.strip().splitlines()[-1])["value"])
    spread = {k: (max(v) - min(v)) / med(v) for k, v in vals.items()}
    return {"msamples_per_s": vals, "median_this": med(vals["this"]), "median_parent": med(vals["parent"]),
            "this_over_parent": med(vals["this"]) / med(vals["parent"]), "spread": spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reference-spp", type=int, default=1024)
    ap.add_argument("--parent-lib", default="", help="libmcpt_hip.so of the parent commit: adds the bench.py comparison")
    ap.add_argument("--parts", default="cost,error", help="comma-separated: which measurements to run")
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/antilag_benches.txt")
    a = ap.parse_args()
    res = {"label": a.label, "size": "%dx%d" % (W, H), "spp": SPP}
    parts = a.parts.split(",")
    if "cost" in parts:
        res["cost"] = bench_cost(a.frames)
    if "error" in parts:
        res["error"] = bench_error(6, 3, a.reference_spp)
    if a.parent_lib:
        res["bench"] = bench_headline(a.parent_lib, 3)
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "antilag_benches.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
