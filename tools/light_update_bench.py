#!/usr/bin/env python3
"""What moving light triangles in place costs, against making the scene again (profiles/light_update_benches.txt).

One MI355X, one process, the arms taking turns repetition by repetition after one warm-up round; medians of --reps
rounds.  Cases: one light group of the Veach stand-in, all of its 3 012 lights, and all 5 200 lights of
tests/scenegen.sphere_mix, moved back and forth between a small translation and the original pose.
  update          Scene.update of the precomputed arrays
  update_device   Scene.update_device of the same arrays held in torch tensors on the device
  transform       Scene.transform of the translation's matrix (the host copy is synced outside the timer)
  create          Scene.create of the same arrays plus the first call's device setup (an 8 x 6 primary_hits)
For each: wall time (time.perf_counter around the call, which ends in a stream synchronisation), the call's
mcpt_update_stats.device_seconds (scatter and main-tree refit) and the light stage's own device time
(mcpt_light_update_stats.device_seconds).  Per scene also the area-sum kernel alone over every group
(mcpt_debug_light_area_cum_bench).  Prints one JSON line; --append adds it to profiles/light_update_benches.txt.

  python tools/light_update_bench.py [--append]
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


def fresh(arr):
    return mcpt.Scene.create(arr["positions"], arr["normals"], arr["material_id"], arr["materials"], arr["light_facet"],
                             arr["light_radiance"])


def translated(pos, d):
    return (pos.astype(np.float64) + np.tile(np.asarray(d, np.float64), 3)).astype(np.float32)


def light_span(arr, l0, l1):
    """the facet range of lights [l0, l1), which must be contiguous facets"""
    f = arr["light_facet"][l0:l1]
    assert np.array_equal(f, np.arange(f[0], f[0] + len(f)))
    return int(f[0]), len(f)


def main():
    import torch
    import scenegen

    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/light_update_benches.txt")
    a = ap.parse_args()
    scene_dir = os.path.join(ROOT, "scenes", "veach-mis")
    veach = mcpt.Scene.load(os.path.join(scene_dir, "veach-mis.obj"), os.path.join(scene_dir, "veach-mis.xml")).arrays()
    obj, xml = scenegen.sphere_mix(tempfile.mkdtemp())
    mix = mcpt.Scene.load(obj, xml).arrays()
    rad = veach["light_radiance"]
    cut = np.flatnonzero((np.diff(rad, axis=0) != 0).any(axis=1)) + 1  # the groups: runs of equal radiance
    lf_sorted = np.sort(veach["light_facet"])
    assert np.array_equal(lf_sorted, np.arange(lf_sorted[0], lf_sorted[0] + 3012))
    mf = np.sort(mix["light_facet"])
    cases = {"veach_one_group": (veach, light_span(veach, int(cut[0]), int(cut[1]))),
             "veach_all_3012": (veach, (int(lf_sorted[0]), 3012)),
             "sphere_mix_all_5200": (mix, (int(mf[0]), 5200))}
    cam_small = mcpt.Camera.reference(8, 6)
    step = (0.05, 0.1, -0.05)
    m = np.hstack([np.eye(3), np.asarray(step, np.float64).reshape(3, 1)])
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    res = {"label": a.label, "reps": a.reps, "cases": {}}
    for name, (arr, (first, n)) in cases.items():
        scene = fresh(arr)
        mcpt.primary_hits(scene, cam_small)
        scene.set_lights_movable()
        scene.rest_save()
        p0, q = arr["positions"][first:first + n], arr["normals"][first:first + n]
        poses = [(m, translated(p0, step)), (ident, p0.copy())]
        dev = [(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()) for _, p in poses]
        arms = {arm: {"wall_ms": [], "device_ms": [], "light_stage_ms": []} for arm in ("update", "update_device", "transform", "create")}
        for rep in range(a.reps + 1):  # rep 0 warms up (code objects, the refit and light states, allocations)
            mat, p = poses[rep % 2]
            tp, tq = dev[rep % 2]
            whole = {k: v.copy() for k, v in arr.items()}
            whole["positions"][first:first + n] = p

            def create():
                s = fresh(whole)
                mcpt.primary_hits(s, cam_small)
                return s

            calls = {"update": lambda: scene.update(first, p, q),
                     "update_device": lambda: scene.update_device(first, n, tp.data_ptr(), tq.data_ptr()),
                     "transform": lambda: scene.transform(first, n, mat),
                     "create": create}
            for arm, call in calls.items():
                w, st = timed(call)
                if arm == "create":
                    st.close()
                    dev_ms = light_ms = None
                else:
                    info = scene.light_update_info()
                    assert info["lights"] == n
                    dev_ms, light_ms = st["device_seconds"] * 1e3, info["device_seconds"] * 1e3
                    scene.host_sync()
                if rep:
                    v = arms[arm]
                    v["wall_ms"].append(w)
                    if dev_ms is not None:
                        v["device_ms"].append(dev_ms), v["light_stage_ms"].append(light_ms)
                        v["info"] = {k: info[k] for k in ("lights", "chunks", "groups", "light_nodes_refit", "light_levels")}
            note("%s: round %d done" % (name, rep))
        for v in arms.values():
            for s in ("wall", "device", "light_stage"):
                if v[s + "_ms"]:
                    v["median_%s_ms" % s] = statistics.median(v[s + "_ms"])
        got = scene.arrays()["positions"][first:first + n]
        assert np.array_equal(got, poses[a.reps % 2][1])
        entry = {"facets": len(arr["positions"]), "range": [first, first + n], "arms": arms,
                 "create_over_update_wall": arms["create"]["median_wall_ms"] / arms["update"]["median_wall_ms"],
                 "area_cum_kernel_ms_all_groups": mcpt.debug_light_area_cum_bench(scene, reps=20) * 1e3}
        res["cases"][name] = entry
        scene.close()
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "light_update_benches.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
