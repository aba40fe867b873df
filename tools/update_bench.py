#!/usr/bin/env python3
"""What moving geometry costs: mcpt_scene_update against making a new scene (profiles/update_benches.txt).

Cornell + 1 M random triangles (scenes/gen_cornell_random.py, the C5 scene), one MI355X, one process, the arms taking
turns repetition by repetition after one warm-up round:
  update 1 / 1 000 / all   Scene.update of one facet, of 1 000 facets and of the whole longest run of non-light facets
                           (translated back and forth by a hundredth of the extent): wall time (time.perf_counter
                           around the call, which ends in a stream synchronisation) and mcpt_update_stats.device_seconds
                           (HIP events around the scatter, the per-level refit launches and the clears)
  rebuild                  what a caller has to do without the update: Scene.create of the same arrays (host SAH build)
                           plus the first call's device setup (an 8x6 primary_hits: collapse, renumbering, quantisation,
                           every upload); wall time
Then the traversal cost of a refit tree: a tenth of the triangles translated by a quarter of the extent, and the device
time (mcpt_stats.seconds) of a 4-spp 800x600 MIS frame on the refit scene against a fresh scene of the same arrays,
again taking turns; the frames must agree under the suite's tight gates.
Medians are what README.md and DESIGN.md 4.19 quote.  Prints one JSON line; --append adds it to
profiles/update_benches.txt.

  python tools/update_bench.py [--append]
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


def longest_non_light_run(arr):
    light = np.zeros(len(arr["positions"]), bool)
    light[arr["light_facet"]] = True
    edge = np.flatnonzero(np.diff(np.concatenate([[True], light, [True]]).astype(np.int8)))
    return max(zip(edge[0::2].tolist(), edge[1::2].tolist()), key=lambda r: r[1] - r[0])


def translated(pos, d):
    return (pos.astype(np.float64) + np.tile(np.asarray(d, np.float64), 3)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/update_benches.txt")
    a = ap.parse_args()
    obj, xml = cornell(a.triangles)
    arr = mcpt.Scene.load(obj, xml).arrays()
    p = arr["positions"].astype(np.float64).reshape(-1, 3)
    ext = float((p.max(axis=0) - p.min(axis=0)).max())
    r0, r1 = longest_non_light_run(arr)
    sizes = {"1": 1, "1000": min(1000, r1 - r0), "all": r1 - r0}
    cam_small = mcpt.Camera.reference(8, 6)
    scene = fresh(arr)
    mcpt.primary_hits(scene, cam_small)
    step = ext / 100.0
    arms = {k: {"wall_ms": [], "device_ms": [], "stats": None} for k in sizes}
    rebuild = []
    for rep in range(a.reps + 1):  # rep 0 warms up (code objects, the refit state of the device, allocations)
        for k, n in sizes.items():
            first = r0 + (r1 - r0 - n) // 2
            new = translated(arr["positions"][first:first + n], (step if rep % 2 == 0 else 0.0, 0.0, 0.0))
            t0 = time.perf_counter()
            st = scene.update(first, new)
            w = time.perf_counter() - t0
            if rep:
                arms[k]["wall_ms"].append(w * 1e3), arms[k]["device_ms"].append(st["device_seconds"] * 1e3)
                arms[k]["stats"] = {q: st[q] for q in ("facets", "leaf_slots", "nodes_refit", "levels")}
        t0 = time.perf_counter()
        other = fresh(arr)
        t1 = time.perf_counter()
        mcpt.primary_hits(other, cam_small)
        t2 = time.perf_counter()
        other.close()
        if rep:
            rebuild.append({"create_ms": (t1 - t0) * 1e3, "device_setup_ms": (t2 - t1) * 1e3, "wall_ms": (t2 - t0) * 1e3})
    for v in arms.values():
        v["median_wall_ms"], v["median_device_ms"] = statistics.median(v["wall_ms"]), statistics.median(v["device_ms"])
    res = {"label": a.label, "scene": "cornell + %d triangles: %d facets, non-light run [%d, %d)" % (a.triangles, len(p) // 3, r0, r1),
           "reps": a.reps, "update": arms,
           "rebuild": {"runs": rebuild, "median_wall_ms": statistics.median(r["wall_ms"] for r in rebuild),
                       "median_create_ms": statistics.median(r["create_ms"] for r in rebuild)}}
    res["rebuild_over_full_update_wall"] = res["rebuild"]["median_wall_ms"] / arms["all"]["median_wall_ms"]
    scene.close()
    # traversal cost of a refit tree against a rebuilt one
    n = (r1 - r0) // 10
    first = r0 + (r1 - r0 - n) // 2
    new = translated(arr["positions"][first:first + n], (ext / 4.0, 0.0, 0.0))
    refit = fresh(arr)
    cam = mcpt.Camera.reference(800, 600)
    mcpt.primary_hits(refit, cam_small)
    res["traversal"] = {"moved_facets": n, "update": refit.update(first, new)}
    arr2 = dict(arr, positions=arr["positions"].copy())
    arr2["positions"][first:first + n] = new
    rebuilt = fresh(arr2)
    tr, tb = [], []
    for rep in range(3 + 1):
        ir, sr = mcpt.render(refit, cam, 4, seed=mcpt.DEFAULT_SEED)
        ib, sb = mcpt.render(rebuilt, cam, 4, seed=mcpt.DEFAULT_SEED)
        if rep:
            tr.append(sr.seconds * 1e3), tb.append(sb.seconds * 1e3)
    l2 = float(np.linalg.norm(ir - ib) / np.linalg.norm(ib))
    assert l2 <= 1e-8, l2
    res["traversal"].update({"refit_frame_device_ms": tr, "rebuilt_frame_device_ms": tb, "frame_rel_l2": l2,
                             "refit_over_rebuilt": statistics.median(tr) / statistics.median(tb)})
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "update_benches.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
