#!/usr/bin/env python3
"""What re-lighting a scene in place costs, against making the scene again (profiles/relight_benches.txt).

One MI355X, one process, the arms taking turns repetition by repetition after one warm-up round; medians of --reps
rounds.  The edits alternate between a dimmed table and the original one.
  radiance cases   one light group of the Veach stand-in, all of its 3 012 lights, all 5 200 lights of
                   tests/scenegen.sphere_mix:
    set_radiance         Scene.set_light_radiance of the precomputed radiances
    set_radiance_device  Scene.set_light_radiance_device of the same radiances held in a torch tensor on the device
    create               Scene.create of the same arrays (with the grouping) plus the first call's device setup (an
                         8 x 6 primary_hits)
  material cases   one row and all rows of the stand-in's material table: set_materials against the same create
For each: wall time (time.perf_counter around the call, which ends in a stream synchronisation) and the call's
mcpt_relight_stats.device_seconds (HIP events around the stage on the state's stream).  Prints one JSON line; --append
adds it to profiles/relight_benches.txt.

  python tools/relight_bench.py [--append]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import monte_carlo_path_tracing_amd as mcpt  # noqa: E402


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def create(arr, groups, cam):
    s = mcpt.Scene.create(arr["positions"], arr["normals"], arr["material_id"], arr["materials"], arr["light_facet"],
                          arr["light_radiance"], light_group=groups)
    mcpt.primary_hits(s, cam)
    return s


def run_case(a, arr, cam, arms_of):
    """arms_of(scene, rep) -> {arm: call}; "create" returns a scene, every other arm the stats dict"""
    scene = create(arr, None, cam)
    groups = scene.light_groups()
    arms = {}
    for rep in range(a.reps + 1):  # rep 0 warms up (code objects, the chunk rows, allocations)
        for arm, call in arms_of(scene, groups, rep).items():
            w, st = timed(call)
            v = arms.setdefault(arm, {"wall_ms": [], "device_ms": []})
            if arm == "create":
                st.close()
            elif rep:
                v["device_ms"].append(st["device_seconds"] * 1e3)
                v["stats"] = {k: st[k] for k in ("lights", "chunks", "groups", "materials", "device_states")}
            if rep:
                v["wall_ms"].append(w)
    for v in arms.values():
        for s in ("wall", "device"):
            if v[s + "_ms"]:
                v["median_%s_ms" % s] = statistics.median(v[s + "_ms"])
    scene.close()
    return arms


def main():
    import torch
    import scenegen

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/relight_benches.txt")
    a = ap.parse_args()
    scene_dir = os.path.join(ROOT, "scenes", "veach-mis")
    veach = mcpt.Scene.load(os.path.join(scene_dir, "veach-mis.obj"), os.path.join(scene_dir, "veach-mis.xml")).arrays()
    obj, xml = scenegen.sphere_mix(tempfile.mkdtemp())
    mix = mcpt.Scene.load(obj, xml).arrays()
    cut = np.flatnonzero((np.diff(veach["light_radiance"], axis=0) != 0).any(axis=1)) + 1  # the groups: runs of equal radiance
    cam = mcpt.Camera.reference(8, 6)
    res = {"label": a.label, "reps": a.reps, "cases": {}}
    radiance_cases = {"veach_one_group": (veach, int(cut[0]), int(cut[1]) - int(cut[0])), "veach_all_3012": (veach, 0, 3012),
                      "sphere_mix_all_5200": (mix, 0, 5200)}
    for name, (arr, first, n) in radiance_cases.items():
        r0 = arr["light_radiance"][first:first + n].copy()
        tables = [r0 * 0.5, r0]
        dev = [torch.from_numpy(t).cuda() for t in tables]

        def arms_of(scene, groups, rep, arr=arr, first=first, n=n, tables=tables, dev=dev):
            whole = {k: v.copy() for k, v in arr.items()}
            whole["light_radiance"][first:first + n] = tables[rep % 2]
            return {"set_radiance": lambda: scene.set_light_radiance(first, tables[rep % 2]),
                    "set_radiance_device": lambda: scene.set_light_radiance_device(first, n, dev[rep % 2].data_ptr()),
                    "create": lambda: create(whole, groups, cam)}

        arms = run_case(a, arr, cam, arms_of)
        res["cases"][name] = {"facets": len(arr["positions"]), "lights": [first, first + n], "arms": arms,
                              "create_over_set_wall": arms["create"]["median_wall_ms"] / arms["set_radiance"]["median_wall_ms"]}
        note("%s done" % name)
    M = len(veach["materials"])
    for name, (first, n) in {"veach_one_material": (0, 1), "veach_all_materials": (0, M)}.items():
        m0 = veach["materials"][first:first + n].copy()
        half = m0.copy()
        half[:, :6] *= 0.5
        tables = [half, m0]

        def arms_of(scene, groups, rep, first=first, n=n, tables=tables):
            whole = {k: v.copy() for k, v in veach.items()}
            whole["materials"][first:first + n] = tables[rep % 2]
            return {"set_materials": lambda: scene.set_materials(first, tables[rep % 2]), "create": lambda: create(whole, groups, cam)}

        arms = run_case(a, veach, cam, arms_of)
        res["cases"][name] = {"facets": len(veach["positions"]), "materials": [first, first + n], "arms": arms,
                              "create_over_set_wall": arms["create"]["median_wall_ms"] / arms["set_materials"]["median_wall_ms"]}
        note("%s done" % name)
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "relight_benches.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
