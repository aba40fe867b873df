#!/usr/bin/env python3
"""What guided upsampling buys per frame of a short sequence (profiles/upsample_benches.txt).

Veach-MIS, --frames frames along an orbit of --orbit degrees a frame (frame k at seed + k), filtered, shown at
--width x --height.  Three arms, each a FrameSequence, in one process, frame by frame one after the other:
  native        the shown size at --spp samples
  upsampled     1 / --factor of the shown size at --spp samples, upsampled (FrameSequence(..., upsample=factor))
  upsampled_eq  the same at --spp * factor^2 samples: the sample count of `native`
Per arm: the wall time of every frame (time.perf_counter around a call that ends in a device synchronisation), the
stage device times of mcpt_sequence_info, for the upsampled arms also those of mcpt_sequence_upsample_info and the
fallback share, and the last shown frame against ONE independent --ref-spp frame of the shown size at another seed:
the tone-mapped relative L2 and the relative MSE of tests/test_denoise.py.  One warm-up frame per arm (code objects,
the scene's device state, allocations) precedes the timed frames, after which the histories start over; the medians
over the timed frames are what README.md and DESIGN.md 4.17 quote.
The kernel alone: mcpt_upsample_device --kernel-runs times on device copies of the last frame's inputs, the median of
its device seconds (HIP events around the count's memset and the kernel), and the share of the algorithmic traffic
rate it reaches: (13 doubles per low pixel + 10 + 3 per full pixel) / time over the 6.29 TB/s a copy kernel measures
on this part.
Prints one JSON line; --append adds it to profiles/upsample_benches.txt.

  python tools/upsample_bench.py [--append]
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
COPY_RATE = 6.29e12  # bytes per second: the measured float4 copy of an MI355X


def tm(x):
    return np.minimum(np.maximum(x, 0.0) / 380.0, 1.0) ** 0.25


def tm_l2(a, ref):
    return float(np.linalg.norm(tm(a) - tm(ref)) / np.linalg.norm(tm(ref)))


def rel_mse(a, ref):
    d = a - ref
    return float(np.mean((d * d).sum(-1) / ((ref * ref).sum(-1) + 1e-2)))


def traffic_bytes(w, h, f):
    return 8 * (13 * w * h + 13 * f * f * w * h)


def kernel_alone(scene, cam, color, f, runs):
    import torch
    g, G = mcpt.render_aovs(scene, cam), mcpt.render_aovs(scene, mcpt.camera_scaled(cam, f))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dc, dg, dG = t(color), {k: t(a) for k, a in g.items()}, {k: t(a) for k, a in G.items()}
    h, w = color.shape[:2]
    out = torch.zeros((f * h, f * w, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda d: {k: a.data_ptr() for k, a in d.items()}
    secs = [mcpt.upsample_device(w, h, dc.data_ptr(), ptr(dg), ptr(dG), out.data_ptr(), factor=f)[1] for _ in range(runs + 2)][2:]
    med = statistics.median(secs)
    b = traffic_bytes(w, h, f)
    return {"runs": runs, "device_ms": [s * 1e3 for s in secs], "median_device_ms": med * 1e3, "algorithmic_bytes": b,
            "bytes_per_second": b / med, "share_of_copy_rate": b / med / COPY_RATE}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=800, help="the shown size")
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--orbit", type=float, default=0.05, help="degrees per frame")
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--kernel-runs", type=int, default=20)
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/upsample_benches.txt")
    a = ap.parse_args()
    f = a.factor
    assert a.width % f == 0 and a.height % f == 0
    w, h = a.width // f, a.height // f
    d = os.path.join(ROOT, "scenes", "veach-mis")
    scene = mcpt.Scene.load(os.path.join(d, "veach-mis.obj"), os.path.join(d, "veach-mis.xml"))
    full0, low0 = mcpt.Camera.reference(a.width, a.height), mcpt.Camera.reference(w, h)
    arms = {"native": (mcpt.FrameSequence(scene, a.width, a.height, a.spp, denoise=True), full0, a.spp),
            "upsampled": (mcpt.FrameSequence(scene, w, h, a.spp, denoise=True, upsample=f), low0, a.spp),
            "upsampled_eq": (mcpt.FrameSequence(scene, w, h, a.spp * f * f, denoise=True, upsample=f), low0, a.spp * f * f)}
    for seq, cam0, _ in arms.values():  # warm-up: one frame per arm, then the histories start over
        seq.frame(cam0, SEED)
        seq.reset()
    rec = {n: {"spp": spp, "wall_ms": [], "stage_device_ms": [], "upsample_stage_ms": [], "fallback_share": []}
           for n, (_, _, spp) in arms.items()}
    for k in range(a.frames):
        for n, (seq, cam0, _) in arms.items():
            cam = mcpt.camera_orbit(cam0, k * a.orbit)
            t0 = time.perf_counter()
            seq.frame(cam, SEED + k)
            rec[n]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            rec[n]["stage_device_ms"].append({s[:-8] + "_ms": getattr(seq.info, s) * 1e3 for s in STAGES})
            if seq.factor > 1:
                u = seq.upsample_info()
                rec[n]["upsample_stage_ms"].append({"guide_ms": u["guide_seconds"] * 1e3, "upsample_ms": u["upsample_seconds"] * 1e3})
                rec[n]["fallback_share"].append(u["fallback_share"])
    last = mcpt.camera_orbit(full0, (a.frames - 1) * a.orbit)
    ref, _ = mcpt.render(scene, last, a.ref_spp, seed=SEED + 1000)
    for n, (seq, _, _) in arms.items():
        r = rec[n]
        shown = seq.read("upsampled" if seq.factor > 1 else "filtered")
        r["median_wall_ms"] = statistics.median(r["wall_ms"])
        r["median_stage_device_ms"] = {s: statistics.median(x[s] for x in r["stage_device_ms"]) for s in r["stage_device_ms"][0]}
        if seq.factor > 1:
            r["median_upsample_stage_ms"] = {s: statistics.median(x[s] for x in r["upsample_stage_ms"]) for s in ("guide_ms", "upsample_ms")}
            r["median_fallback_share"] = statistics.median(r["fallback_share"])
        r["tone_mapped_rel_l2"], r["rel_mse"] = tm_l2(shown, ref), rel_mse(shown, ref)
    low_last = mcpt.camera_orbit(low0, (a.frames - 1) * a.orbit)
    kern = kernel_alone(scene, low_last, arms["upsampled"][0].read("filtered"), f, a.kernel_runs)
    for seq, _, _ in arms.values():
        seq.close()
    res = {"label": a.label,
           "frame": "%dx%d shown, mis, %d frames, orbit %g deg/frame, denoise, factor %d, reference %d spp" %
                    (a.width, a.height, a.frames, a.orbit, f, a.ref_spp),
           "arms": rec, "wall_native_over_upsampled": rec["native"]["median_wall_ms"] / rec["upsampled"]["median_wall_ms"],
           "wall_native_over_upsampled_eq": rec["native"]["median_wall_ms"] / rec["upsampled_eq"]["median_wall_ms"],
           "kernel": kern}
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "upsample_benches.txt"), "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
