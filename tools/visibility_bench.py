#!/usr/bin/env python3
"""What hiding and showing facets in place costs, and what the dead slots cost a frame (profiles/visibility_benches.txt).

Cornell + 1 M random triangles (scenes/gen_cornell_random.py, the C5 scene), one MI355X, one process, the arms taking
turns repetition by repetition after one warm-up round; medians of --reps rounds.
  call      hide and show of 1 facet, 1 000 facets and every non-light facet (one call per non-light run): wall time
            (time.perf_counter around the calls, each of which ends in a stream synchronisation) and the calls'
            mcpt_update_stats.device_seconds (HIP events around the scatter and the refit on the state's stream), against
            Scene.create of the remaining arrays plus the first call's device setup (an 8 x 6 primary_hits)
  frame     all random triangles (the longest non-light run) hidden, one 4-spp 800 x 600 MIS frame (device seconds of the
            render's stats) three ways: on the tree hidden in place, after rebuild(), and on a fresh scene of the
            remaining arrays -- the price of keeping dead slots in the tree
  headline  (--parent-lib) bench.py --gpus 1 --steps 3 --warmup 1 with this tree's library and the parent's, taking
            turns: no render kernel changes, so the two must lie inside the run-to-run spread
Prints one JSON line; --append adds it to profiles/visibility_benches.txt.

  python tools/visibility_bench.py [--parts call,frame,headline] [--parent-lib PATH] [--append]
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
from update_bench import cornell, fresh, longest_non_light_run  # noqa: E402

med = statistics.median


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def non_light_runs(arr):
    light = np.zeros(len(arr["positions"]), bool)
    light[arr["light_facet"]] = True
    edge = np.flatnonzero(np.diff(np.concatenate([[True], light, [True]]).astype(np.int8)))
    return [(int(a), int(b)) for a, b in zip(edge[0::2], edge[1::2])]


def without(arr, ranges):
    """the arrays without the facets of `ranges`: rows dropped, light_facet through the old -> new index map"""
    keep = np.ones(len(arr["positions"]), bool)
    for a, b in ranges:
        keep[a:b] = False
    new_of_old = np.cumsum(keep) - 1
    out = dict(arr)
    for k in ("positions", "normals", "material_id"):
        out[k] = np.ascontiguousarray(arr[k][keep])
    out["light_facet"] = new_of_old[arr["light_facet"]].astype(np.int32)
    return out


def create(arr, cam):
    s = fresh(arr)
    mcpt.primary_hits(s, cam)
    return s


def bench_call(arr, reps):
    cam = mcpt.Camera.reference(8, 6)
    a, b = longest_non_light_run(arr)
    cases = {"1": [(a + (b - a) // 2, a + (b - a) // 2 + 1)], "1000": [(a + (b - a) // 2, a + (b - a) // 2 + 1000)],
             "all_non_light": non_light_runs(arr)}
    scene = create(arr, cam)
    out = {}
    for name, ranges in cases.items():
        rest = without(arr, ranges)
        arms = {k: {"wall_ms": [], "device_ms": []} for k in ("hide", "show", "create")}

        def edit(visible):
            sts = [scene.set_visible(f0, f1 - f0, visible) for f0, f1 in ranges]
            return sum(s["device_seconds"] for s in sts) * 1e3, sts

        for rep in range(reps + 1):  # rep 0 warms up (code objects, the refit state, the mask, allocations)
            for arm in ("hide", "show", "create"):
                if arm == "create":
                    w, s = timed(lambda: create(rest, cam))
                    s.close()
                    mcpt.primary_hits(scene, cam)  # untimed: the next round's hide does not wait for this arm's teardown
                    dev = None
                else:
                    w, (dev, sts) = timed(lambda: edit(arm == "show"))
                    arms[arm]["stats"] = {k: sum(s[k] for s in sts) for k in ("facets", "leaf_slots", "nodes_refit")}
                    arms[arm]["stats"]["levels"] = sts[0]["levels"]
                if rep:
                    arms[arm]["wall_ms"].append(w)
                    if dev is not None:
                        arms[arm]["device_ms"].append(dev)
        for v in arms.values():
            v["median_wall_ms"] = med(v["wall_ms"])
            if v["device_ms"]:
                v["median_device_ms"] = med(v["device_ms"])
        out[name] = {"ranges": len(ranges), "facets": int(sum(f1 - f0 for f0, f1 in ranges)), "arms": arms,
                     "create_over_hide_wall": arms["create"]["median_wall_ms"] / arms["hide"]["median_wall_ms"]}
        note("call %s done" % name)
    scene.close()
    return out


def bench_frame(arr, reps):
    cam = mcpt.Camera.reference(800, 600)
    a, b = longest_non_light_run(arr)
    scenes = {"in_place": fresh(arr), "rebuilt": fresh(arr), "fresh_without": fresh(without(arr, [(a, b)]))}
    info = {}
    for k in ("in_place", "rebuilt"):
        mcpt.primary_hits(scenes[k], mcpt.Camera.reference(8, 6))
        info[k + "_cost_before"] = scenes[k].tree_cost()
        scenes[k].hide(a, b - a)
    info["rebuild"] = scenes["rebuilt"].rebuild()
    for k, s in scenes.items():
        info[k + "_cost"] = s.tree_cost()
    ms = {k: [] for k in scenes}
    for rep in range(reps + 1):
        for k, s in scenes.items():
            _, st = mcpt.render(s, cam, 4, mode="mis", seed=20240430 + rep)
            if rep:
                ms[k].append(st.seconds * 1e3)
    for s in scenes.values():
        s.close()
    res = {"hidden": [a, b], "frame_ms": ms, **{"median_%s_ms" % k: med(v) for k, v in ms.items()}, **info}
    res["in_place_over_fresh"] = res["median_in_place_ms"] / res["median_fresh_without_ms"]
    res["rebuilt_over_fresh"] = res["median_rebuilt_ms"] / res["median_fresh_without_ms"]
    return res


def bench_headline(parent_lib, runs):
    arms = {"this": None, "parent": parent_lib}
    vals = {k: [] for k in arms}
    for _ in range(runs):
        for k, lib in arms.items():
            env = dict(os.environ)
            if lib:
                env["MCPT_LIB_PATH"] = os.path.abspath(lib)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], env=env,
                               capture_output=True, text=True, check=True, timeout=600)
            vals[k].append(json.loads(r.stdout.strip().splitlines()[-1])["value"])
    spread = {k: (max(v) - min(v)) / med(v) for k, v in vals.items()}
    return {"msamples_per_s": vals, "median_this": med(vals["this"]), "median_parent": med(vals["parent"]),
            "this_over_parent": med(vals["this"]) / med(vals["parent"]), "spread": spread}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="call,frame", help="comma-separated: call, frame, headline")
    ap.add_argument("--parent-lib", default="", help="libmcpt_hip.so of the parent commit, for the headline part")
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/visibility_benches.txt")
    a = ap.parse_args()
    parts = a.parts.split(",")
    res = {"label": a.label, "reps": a.reps}
    if "call" in parts or "frame" in parts:
        obj, xml = cornell(a.triangles)
        arr = mcpt.Scene.load(obj, xml).arrays()
        res["scene"] = "cornell + %d triangles: %d facets" % (a.triangles, len(arr["positions"]))
        if "call" in parts:
            res["call"] = bench_call(arr, a.reps)
        if "frame" in parts:
            res["frame"] = bench_frame(arr, a.reps)
            note("frame done")
    if "headline" in parts:
        if not a.parent_lib:
            ap.error("the headline part needs --parent-lib")
        res["headline"] = bench_headline(a.parent_lib, a.reps)
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "visibility_benches.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
