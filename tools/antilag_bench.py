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
  indexed   (--parts indexed, needs --parent-lib; profiles/antilag_indexed_benches.txt) the gradient pass over the
            indexed ray call against the parent's full-size call: the package is loaded twice in this
            process, once per library, and the two take turns frame by frame at strata 3 and 2 (wall per frame,
            trace_seconds, kernel_seconds; medians of eight frames after a warm-up, and this tree's over the parent's);
            then, with this tree's library alone, render_rays_indexed_device over a phase's count rays against
            render_rays_device over the frame's full-size gradient rays (zero directions off the selection), taking
            turns, the calls' mcpt_stats.seconds and wall time
Prints one JSON line; --append adds it to profiles/antilag_benches.txt (indexed: profiles/antilag_indexed_benches.txt).

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


def load_package(name, lib_path):
    """a second copy of the package under `name`, bound to the library at lib_path (LIB_PATH is read at import)"""
    import importlib.util
    pkg = os.path.join(ROOT, "monte_carlo_path_tracing_amd")
    old = os.environ.get("MCPT_LIB_PATH")
    os.environ["MCPT_LIB_PATH"] = os.path.abspath(lib_path)
    try:
        spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mod.lib()
    finally:
        if old is None:
            del os.environ["MCPT_LIB_PATH"]
        else:
            os.environ["MCPT_LIB_PATH"] = old
    return mod


def bench_indexed(parent_lib, frames):
    import torch
    libs = {"parent": load_package("mcpt_parent", parent_lib), "this": mcpt}
    arms = {k: v for k, v in ARMS.items() if v is not None}
    seqs, scenes = {}, {}
    for lname, m in libs.items():
        scenes[lname] = m.Scene.load(VEACH + ".obj", VEACH + ".xml")
        for aname, v in arms.items():
            seqs[lname, aname] = m.FrameSequence(scenes[lname], W, H, SPP, mode="mis", denoise=True, antilag=v)
    rows = {k: dict(frame_wall_ms=[], trace_ms=[], kernel_ms=[]) for k in seqs}
    for k in range(frames + 1):  # frame 0 warms up (and has no gradient pass)
        for (lname, aname), seq in seqs.items():
            cam = libs[lname].camera_orbit(libs[lname].Camera.reference(W, H), 0.3 * k)
            t0 = time.perf_counter()
            seq.frame(cam, SEED + k, readback=False)
            wall = time.perf_counter() - t0
            if k == 0:
                continue
            info = seq.antilag_info()
            assert info["ran"]
            rows[lname, aname]["frame_wall_ms"].append(1e3 * wall)
            rows[lname, aname]["trace_ms"].append(1e3 * info["trace_seconds"])
            rows[lname, aname]["kernel_ms"].append(1e3 * info["kernel_seconds"])
    for seq in seqs.values():
        seq.close()
    out = {"sequence": {}, "call": {}}
    for aname in arms:
        r = {}
        for lname in libs:
            r[lname] = {"median_" + key: med(v) for key, v in rows[lname, aname].items()}
            r[lname].update(rows[lname, aname])
        for key in ("frame_wall_ms", "trace_ms", "kernel_ms"):
            r["this_over_parent_" + key] = r["this"]["median_" + key] / r["parent"]["median_" + key]
        out["sequence"][aname] = r
    # the two calls alone, this tree's library
    scene, cam = scenes["this"], mcpt.Camera.reference(W, H)
    for aname, v in arms.items():
        s = v["stratum"]
        idx, o, d = mcpt.gradient_rays_indexed(cam, s, 1, 1)
        fo, fd = mcpt.gradient_rays(cam, s, 1, 1)
        t = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (idx, o, d, fo, fd)]
        fb = torch.zeros(3 * W * H, dtype=torch.float64, device="cuda")
        res = dict(full_ms=[], indexed_ms=[], full_wall_ms=[], indexed_wall_ms=[], n=int(len(idx)), full_n=W * H)
        for k in range(frames + 1):
            fb.zero_()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st_f = mcpt.render_rays_device(scene, W * H, t[3].data_ptr(), t[4].data_ptr(), SPP, fb.data_ptr(), seed=SEED)
            t1 = time.perf_counter()
            fb.zero_()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            st_i = mcpt.render_rays_indexed_device(scene, len(idx), t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), W * H, SPP,
                                                   fb.data_ptr(), seed=SEED)
            t3 = time.perf_counter()
            if k:
                res["full_ms"].append(1e3 * st_f.seconds), res["indexed_ms"].append(1e3 * st_i.seconds)
                res["full_wall_ms"].append(1e3 * (t1 - t0)), res["indexed_wall_ms"].append(1e3 * (t3 - t2))
        res["median_full_ms"], res["median_indexed_ms"] = med(res["full_ms"]), med(res["indexed_ms"])
        res["indexed_over_full"] = res["median_indexed_ms"] / res["median_full_ms"]
        res["indexed_over_full_wall"] = med(res["indexed_wall_ms"]) / med(res["full_wall_ms"])
        out["call"][aname] = res
    return out


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
    ap.add_argument("--parts", default="cost,error", help="comma-separated: cost, error, indexed; nobench leaves bench.py out")
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/antilag_benches.txt")
    a = ap.parse_args()
    res = {"label": a.label, "size": "%dx%d" % (W, H), "spp": SPP}
    parts = a.parts.split(",")
    if "cost" in parts:
        res["cost"] = bench_cost(a.frames)
    if "error" in parts:
        res["error"] = bench_error(6, 3, a.reference_spp)
    if "indexed" in parts:
        if not a.parent_lib:
            ap.error("--parts indexed needs --parent-lib")
        res["indexed"] = bench_indexed(a.parent_lib, a.frames)
    if a.parent_lib and "nobench" not in parts:
        res["bench"] = bench_headline(a.parent_lib, 3)
    line = json.dumps(res)
    print(line)
    if a.append:
        name = "antilag_indexed_benches.txt" if "indexed" in parts else "antilag_benches.txt"
        with open(os.path.join(ROOT, "profiles", name), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
