#!/usr/bin/env python3
"""What a frame of a short sequence costs around its render: the host pipeline against the device-resident handle
(profiles/sequence_benches.txt).

Veach-MIS 800x600, --frames frames of --spp samples along an orbit of --orbit degrees a frame (frame k at seed + k),
filtered, once with plain accumulation and once with history clamping.  Two arms, in one process, frame by frame one
after the other:
  host    render + render_aovs + TemporalAccumulator.push + denoise + tone_map: every stage's host form, so the frame
          and its guides come back, the history goes up and comes back, the filter's inputs go up again, and the tone
          map runs on one host core
  handle  FrameSequence.frame (mcpt_sequence): the same kernels on buffers allocated once, the 8-bit frame comes back
Per arm: the wall time of every frame (time.perf_counter around calls that end in a device synchronisation), the
render's device time (mcpt_stats.seconds, HIP events), "non-render" = wall - render device time, and its share of
the wall time; per frame of the handle also the stage device times of mcpt_sequence_info.  One warm-up frame per arm
(code objects, the scene's device state, allocations) precedes the timed frames, after which both histories start
over; the medians over the timed frames are what README.md and DESIGN.md 4.15 quote.  The two arms' 8-bit frames are
compared (they differ where an independent render's summation order moves a value across a level).
Prints one JSON line; --append adds it to profiles/sequence_benches.txt.

  python tools/sequence_bench.py [--append]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import monte_carlo_path_tracing_amd as mcpt  # noqa: E402

SEED = mcpt.DEFAULT_SEED
STAGES = ("render_seconds", "aov_seconds", "temporal_seconds", "denoise_seconds", "tonemap_seconds")


def host_frame(scene, acc, cam, spp, seed):
    """one frame through the host forms -> (rgb8, wall seconds, render device seconds)"""
    t0 = time.perf_counter()
    img, st = mcpt.render(scene, cam, spp, seed=seed)
    aov = mcpt.render_aovs(scene, cam)
    out, var = acc.push(cam, img, aov)
    shown = mcpt.denoise(out, aov, variance=var)[0]
    rgb8 = mcpt.tone_map(shown)
    return rgb8, time.perf_counter() - t0, st.seconds


def handle_frame(seq, cam, seed):
    t0 = time.perf_counter()
    rgb8 = seq.frame(cam, seed)
    return rgb8, time.perf_counter() - t0, seq.info.render_seconds


def summary(wall, render):
    non = [w - r for w, r in zip(wall, render)]
    ms = lambda v: [x * 1e3 for x in v]
    return {"wall_ms": ms(wall), "render_device_ms": ms(render), "non_render_ms": ms(non),
            "median_wall_ms": statistics.median(ms(wall)), "median_non_render_ms": statistics.median(ms(non)),
            "median_non_render_share": statistics.median([n / w for n, w in zip(non, wall)])}


def run(scene, a, clamp):
    cam0 = mcpt.Camera.reference(a.width, a.height)
    seq = mcpt.FrameSequence(scene, a.width, a.height, a.spp, denoise=True, clamp=True if clamp else None)
    # warm-up: one frame per arm, then both histories start over
    host_frame(scene, mcpt.TemporalAccumulator(clamp=True if clamp else None), cam0, a.spp, SEED)
    handle_frame(seq, cam0, SEED)
    seq.reset()
    acc = mcpt.TemporalAccumulator(clamp=True if clamp else None)
    hw, hr, sw, sr, stages, differ = [], [], [], [], [], []
    for k in range(a.frames):
        cam = mcpt.camera_orbit(cam0, k * a.orbit)
        h8, w, r = host_frame(scene, acc, cam, a.spp, SEED + k)
        hw.append(w), hr.append(r)
        s8, w, r = handle_frame(seq, cam, SEED + k)
        sw.append(w), sr.append(r)
        stages.append({k2[:-8] + "_ms": getattr(seq.info, k2) * 1e3 for k2 in STAGES})
        d = np.abs(h8.astype(int) - s8.astype(int))
        differ.append({"values": int((d != 0).sum()), "largest": int(d.max())})
        assert abs(seq.info.kept - acc.kept) < 1e-3, (seq.info.kept, acc.kept)
    seq.close()
    host, handle = summary(hw, hr), summary(sw, sr)
    return {"host": host, "handle": handle, "handle_stage_device_ms": stages,
            "median_stage_device_ms": {k: statistics.median(s[k] for s in stages) for k in stages[0]},
            "non_render_host_over_handle": host["median_non_render_ms"] / handle["median_non_render_ms"],
            "rgb8_values_that_differ": differ}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--orbit", type=float, default=0.05, help="degrees per frame")
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/sequence_benches.txt")
    a = ap.parse_args()
    d = os.path.join(ROOT, "scenes", "veach-mis")
    scene = mcpt.Scene.load(os.path.join(d, "veach-mis.obj"), os.path.join(d, "veach-mis.xml"))
    res = {"label": a.label,
           "frame": "%dx%d mis, %d frames of %d spp, orbit %g deg/frame, denoise" % (a.width, a.height, a.frames, a.spp, a.orbit),
           "plain": run(scene, a, False), "clamp": run(scene, a, True)}
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "sequence_benches.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
