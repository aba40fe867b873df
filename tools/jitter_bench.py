#!/usr/bin/env python3
"""What MCPT_RENDER_PIXEL_JITTER costs (profiles/jitter_benches.txt).

Veach-MIS 800x600: the 1024-spp MIS frame, the 1024-spp BRDF-only frame and the 4-spp MIS frame of
tools/sequence_bench.py, each rendered three ways in one process, the arms taking turns:
  plain     the default path: roots from the per-pixel tables, root-point cache
  no_cache  plain with MCPT_DEBUG_NO_ROOT_CACHE: every root takes the full light prep -- what losing the cache costs
            (no cache to lose in BRDF-only, which has no light prep: that arm shows the run-to-run spread there)
  jitter    MCPT_RENDER_PIXEL_JITTER: no cache either, and the primary hit traced per sample by k_roots_rays
Per arm: Msamples/s and mcpt_stats.seconds (device time, HIP events) as medians over --repeat timed calls after one
warm-up call, every call's seconds, and the share of the plain rate the arm keeps.
Prints one JSON line; --append adds it to profiles/jitter_benches.txt.

  python tools/jitter_bench.py [--append]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import monte_carlo_path_tracing_amd as mcpt  # noqa: E402

ARMS = (("plain", 0), ("no_cache", mcpt.DEBUG_NO_ROOT_CACHE), ("jitter", mcpt.RENDER_PIXEL_JITTER))


def workload(scene, cam, spp, mode, repeat):
    calls = {name: [] for name, _ in ARMS}
    for name, flags in ARMS:  # warm-up: code objects, the scene's device state, allocations
        mcpt.render(scene, cam, spp, mode=mode, flags=flags)
    for _ in range(repeat):
        for name, flags in ARMS:
            calls[name].append(mcpt.render(scene, cam, spp, mode=mode, flags=flags)[1])
    out = {}
    for name, _ in ARMS:
        sec = [st.seconds for st in calls[name]]
        rate = [st.camera_samples / st.seconds * 1e-6 for st in calls[name]]
        out[name] = {"median_seconds": statistics.median(sec), "median_msamples_per_s": statistics.median(rate),
                     "all_seconds": sec, "prep_cached_nodes": int(calls[name][0].prep_cached_nodes),
                     "generations": int(calls[name][0].generations)}
    for name in ("no_cache", "jitter"):
        out[name]["share_of_plain_rate"] = out[name]["median_msamples_per_s"] / out["plain"]["median_msamples_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--frame-spp", type=int, default=4, help="the short frame of tools/sequence_bench.py")
    ap.add_argument("--repeat", type=int, default=3, help="timed calls per arm")
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/jitter_benches.txt")
    a = ap.parse_args()
    d = os.path.join(ROOT, "scenes", "veach-mis")
    scene = mcpt.Scene.load(os.path.join(d, "veach-mis.obj"), os.path.join(d, "veach-mis.xml"))
    cam = mcpt.Camera.reference(a.width, a.height)
    res = {"label": a.label, "frame": "%dx%d" % (a.width, a.height),
           "mis_%dspp" % a.spp: workload(scene, cam, a.spp, "mis", a.repeat),
           "brdf_%dspp" % a.spp: workload(scene, cam, a.spp, "brdf", a.repeat),
           "mis_%dspp" % a.frame_spp: workload(scene, cam, a.frame_spp, "mis", max(a.repeat, 5))}
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "jitter_benches.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
