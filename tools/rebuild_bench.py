#!/usr/bin/env python3
"""What a degraded refit tree costs and what mcpt_scene_rebuild gives back (profiles/rebuild_benches.txt).

Cornell + 1 M random triangles (scenes/gen_cornell_random.py, the C5 scene), one MI355X, one process, the arms taking
turns round by round after one warm-up round; medians of --reps rounds are what README.md and DESIGN.md 4.22 quote.
  rebuild      Scene.rebuild of the untouched scene: wall time (time.perf_counter around the call, which ends in a stream
               synchronisation) and mcpt_rebuild_stats.device_seconds (HIP events around the build), against what a
               caller had to do before: Scene.create of the same arrays (host SAH build) plus the first call's device
               setup (an 8x6 primary_hits), wall time
  traversal    the case of DESIGN.md 4.19: a tenth of the triangles translated by a quarter of the extent; the device
               time (mcpt_stats.seconds) of a 4-spp 800x600 MIS frame on the refit tree, on the rebuilt tree and on a
               fresh SAH tree of the same arrays; Scene.tree_cost of the three; the frames must agree under the suite's
               tight gates
  leaf_max     the same frame on trees rebuilt with leaves of at most 1, 2, 3 and 4 facets
               (mcpt_debug_set_rebuild_leaf_max): frame time, tree cost, nodes, build time
  headline     (--parent-lib) bench.py --gpus 1 --steps 3 --warmup 1 with this tree's library and the parent's, taking
               turns: no headline code changes, so the two must lie inside the run-to-run spread
Prints one JSON line; --append adds it to profiles/rebuild_benches.txt.

  python tools/rebuild_bench.py [--parts rebuild,traversal,leaf_max,headline] [--parent-lib PATH] [--append]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import monte_carlo_path_tracing_amd as mcpt  # noqa: E402
from update_bench import cornell, fresh, longest_non_light_run, translated  # noqa: E402

med = statistics.median


def bench_rebuild(arr, reps):
    cam_small = mcpt.Camera.reference(8, 6)
    scene = fresh(arr)
    mcpt.primary_hits(scene, cam_small)
    runs, create = [], []
    st = None
    for rep in range(reps + 1):  # rep 0 warms up (code objects, the builder's buffers)
        t0 = time.perf_counter()
        other = fresh(arr)
        t1 = time.perf_counter()
        mcpt.primary_hits(other, cam_small)
        t2 = time.perf_counter()
        other.close()
        scene.tree_cost()  # untimed: the release of the other arm's device memory is not the rebuild's to pay
        t3 = time.perf_counter()
        st = scene.rebuild()
        w = time.perf_counter() - t3
        if rep:
            runs.append({"wall_ms": w * 1e3, "device_ms": st["device_seconds"] * 1e3})
            create.append({"create_ms": (t1 - t0) * 1e3, "device_setup_ms": (t2 - t1) * 1e3, "wall_ms": (t2 - t0) * 1e3})
    scene.close()
    res = {"rebuild": runs, "create": create, "stats": {k: st[k] for k in ("facets", "nodes", "levels", "stack_need")},
           "median_rebuild_wall_ms": med(r["wall_ms"] for r in runs), "median_rebuild_device_ms": med(r["device_ms"] for r in runs),
           "median_create_wall_ms": med(r["wall_ms"] for r in create)}
    res["create_over_rebuild_wall"] = res["median_create_wall_ms"] / res["median_rebuild_wall_ms"]
    return res


def moved_case(arr):
    p = arr["positions"].astype(np.float64).reshape(-1, 3)
    ext = float((p.max(axis=0) - p.min(axis=0)).max())
    r0, r1 = longest_non_light_run(arr)
    n = (r1 - r0) // 10
    first = r0 + (r1 - r0 - n) // 2
    new = translated(arr["positions"][first:first + n], (ext / 4.0, 0.0, 0.0))
    arr2 = dict(arr, positions=arr["positions"].copy())
    arr2["positions"][first:first + n] = new
    return first, n, new, arr2


def on_refit_tree(arr, first, new):
    s = fresh(arr)
    mcpt.primary_hits(s, mcpt.Camera.reference(8, 6))
    s.update(first, new)
    return s


def frame_ms(scene, cam):
    img, st = mcpt.render(scene, cam, 4, seed=mcpt.DEFAULT_SEED)
    return img, st.seconds * 1e3


def bench_traversal(arr, reps):
    first, n, new, arr2 = moved_case(arr)
    cam = mcpt.Camera.reference(800, 600)
    scenes = {"refit": on_refit_tree(arr, first, new), "rebuilt": on_refit_tree(arr, first, new), "fresh": fresh(arr2)}
    rst = scenes["rebuilt"].rebuild()
    times = {k: [] for k in scenes}
    imgs = {}
    for rep in range(reps + 1):
        for k, s in scenes.items():
            imgs[k], ms = frame_ms(s, cam)
            if rep:
                times[k].append(ms)
    l2 = {k: float(np.linalg.norm(imgs[k] - imgs["fresh"]) / np.linalg.norm(imgs["fresh"])) for k in ("refit", "rebuilt")}
    assert max(l2.values()) <= 1e-8, l2
    res = {"moved_facets": n, "rebuild": rst, "frame_device_ms": times, "frame_rel_l2_vs_fresh": l2,
           "tree_cost": {k: s.tree_cost() for k, s in scenes.items()},
           "median_frame_ms": {k: med(v) for k, v in times.items()}}
    res["refit_over_rebuilt"] = res["median_frame_ms"]["refit"] / res["median_frame_ms"]["rebuilt"]
    res["rebuilt_over_fresh"] = res["median_frame_ms"]["rebuilt"] / res["median_frame_ms"]["fresh"]
    for s in scenes.values():
        s.close()
    return res


def bench_leaf_max(arr, reps):
    first, n, new, _ = moved_case(arr)
    cam = mcpt.Camera.reference(800, 600)
    scene = on_refit_tree(arr, first, new)
    arms = {k: {"frame_ms": [], "build_ms": []} for k in (1, 2, 3, 4)}
    for rep in range(reps + 1):
        for k, a in arms.items():
            mcpt.debug_set_rebuild_leaf_max(k)
            st = scene.rebuild()
            _, ms = frame_ms(scene, cam)
            if rep:
                a["frame_ms"].append(ms), a["build_ms"].append(st["device_seconds"] * 1e3)
                a.update(nodes=st["nodes"], levels=st["levels"], stack_need=st["stack_need"], tree_cost=st["cost_after"])
    mcpt.debug_set_rebuild_leaf_max(0)
    scene.close()
    for a in arms.values():
        a["median_frame_ms"], a["median_build_ms"] = med(a["frame_ms"]), med(a["build_ms"])
    return {str(k): a for k, a in arms.items()}


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
    ap.add_argument("--parts", default="rebuild,traversal,leaf_max", help="comma-separated: which measurements to run")
    ap.add_argument("--parent-lib", default="", help="libmcpt_hip.so of the parent commit, for the headline part")
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/rebuild_benches.txt")
    a = ap.parse_args()
    parts = a.parts.split(",")
    res = {"label": a.label, "reps": a.reps}
    if set(parts) & {"rebuild", "traversal", "leaf_max"}:
        obj, xml = cornell(a.triangles)
        arr = mcpt.Scene.load(obj, xml).arrays()
        res["scene"] = "cornell + %d triangles: %d facets" % (a.triangles, len(arr["positions"]))
        if "rebuild" in parts:
            res["rebuild"] = bench_rebuild(arr, a.reps)
        if "traversal" in parts:
            res["traversal"] = bench_traversal(arr, a.reps)
        if "leaf_max" in parts:
            res["leaf_max"] = bench_leaf_max(arr, a.reps)
    if "headline" in parts:
        if not a.parent_lib:
            ap.error("the headline part needs --parent-lib")
        res["headline"] = bench_headline(a.parent_lib, a.reps)
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "rebuild_benches.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
