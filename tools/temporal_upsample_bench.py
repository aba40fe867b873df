#!/usr/bin/env python3
"""What temporal upsampling buys over guided upsampling in a short sequence (profiles/temporal_upsample_benches.txt).

Veach-MIS, filtered, shown at --width x --height, two runs: --frames frames along an orbit of --orbit degrees a frame
and --static-frames frames of a static camera (frame k at seed + k).  Four arms, each a FrameSequence, in one process,
frame by frame one after the other:
  native        the shown size at --spp samples
  upsampled     1 / --factor of the shown size at --spp samples, guided upsampling (FrameSequence(..., upsample=factor))
  temporal      as many rays through the full-size pixels of the frame's phase, accumulated at the shown size
                (FrameSequence(..., upsample=factor, temporal_upsample=True))
  temporal_eq   the same at --spp * factor^2 samples: the sample count of `native`
Per arm and run: the wall time of every frame (time.perf_counter around a call that ends in a device synchronisation),
the stage device times of mcpt_sequence_info (for the temporal arms render is the traced rays, aov the full-size guides,
temporal the new kernels and the statistics, denoise the full-size filter), for the upsampled arm those of
mcpt_sequence_upsample_info, for the temporal arms the phase-ray kernel's time and the filled and fallback shares, and the
last shown frame against ONE independent --ref-spp frame of the shown size at another seed: the tone-mapped relative L2
and the relative MSE of tests/test_denoise.py.  One warm-up frame per arm precedes the timed frames of each run, after
which the histories start over; README.md and DESIGN.md 4.18 quote the medians over the timed frames.
The kernels alone, at the shown size, --kernel-runs times each, taking turns in one process on device copies of the last
static frame's state: mcpt_temporal_upsample_device (its device seconds: the counts' memset, k_temporal_upsample and
k_temporal_spatial) against mcpt_temporal_accumulate_device of a full-size colour on the same guides and history.
Prints one JSON line; --append adds it to profiles/temporal_upsample_benches.txt.

  python tools/temporal_upsample_bench.py [--append]
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


def tm(x):
    return np.minimum(np.maximum(x, 0.0) / 380.0, 1.0) ** 0.25


def tm_l2(a, ref):
    return float(np.linalg.norm(tm(a) - tm(ref)) / np.linalg.norm(tm(ref)))


def rel_mse(a, ref):
    d = a - ref
    return float(np.mean((d * d).sum(-1) / ((ref * ref).sum(-1) + 1e-2)))


def med(rows, keys):
    return {k: statistics.median(r[k] for r in rows) for k in keys}


def run(scene, arms, full0, frames, orbit, ref_spp):
    """one run of every arm, frame by frame in turn -> the record per arm"""
    for seq, cam0, _ in arms.values():  # warm-up: one frame per arm, then the histories start over
        seq.reset()
        seq.frame(cam0, SEED)
        seq.reset()
    rec = {n: {"spp": spp, "wall_ms": [], "stage_device_ms": [], "extra": []} for n, (_, _, spp) in arms.items()}
    for k in range(frames):
        for n, (seq, cam0, _) in arms.items():
            cam = mcpt.camera_orbit(cam0, k * orbit)
            t0 = time.perf_counter()
            seq.frame(cam, SEED + k, readback=True)
            rec[n]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            rec[n]["stage_device_ms"].append({s[:-8] + "_ms": getattr(seq.info, s) * 1e3 for s in STAGES})
            if seq.temporal_upsample:
                u = seq.temporal_upsample_info()
                rec[n]["extra"].append({"rays_ms": u["rays_seconds"] * 1e3, "filled_share": u["filled_share"],
                                        "fallback_share": u["fallback_share"]})
            elif seq.factor > 1:
                u = seq.upsample_info()
                rec[n]["extra"].append({"guide_ms": u["guide_seconds"] * 1e3, "upsample_ms": u["upsample_seconds"] * 1e3,
                                        "fallback_share": u["fallback_share"]})
    ref, _ = mcpt.render(scene, mcpt.camera_orbit(full0, (frames - 1) * orbit), ref_spp, seed=SEED + 1000)
    for n, (seq, _, _) in arms.items():
        r = rec[n]
        shown = seq.read("filtered" if seq.temporal_upsample or seq.factor == 1 else "upsampled")
        r["median_wall_ms"] = statistics.median(r["wall_ms"])
        r["median_stage_device_ms"] = med(r["stage_device_ms"], r["stage_device_ms"][0])
        if r["extra"]:
            r["median_extra"] = med(r["extra"], r["extra"][0])
        r["tone_mapped_rel_l2"], r["rel_mse"] = tm_l2(shown, ref), rel_mse(shown, ref)
    return rec


def kernels_alone(scene, seq, low_cam, f, runs):
    """mcpt_temporal_upsample_device against mcpt_temporal_accumulate_device at the full size, taking turns"""
    import torch
    full = mcpt.camera_scaled(low_cam, f)
    G = mcpt.render_aovs(scene, full)
    raw, acc, mom = seq.read("raw"), seq.read("accumulated"), seq.read("moments")
    h, w = raw.shape[:2]
    H, W = f * h, f * w
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dG, dpG = {k: t(a) for k, a in G.items()}, {k: t(a) for k, a in G.items()}
    # the sequence's own history (n <= frames / f^2: every pixel's variance is still the spatial estimate in both calls'
    # outputs or, for the accumulation, one step from the temporal formula) and a long one (n = 16, g = 1 / 16: the
    # temporal formula everywhere, k_temporal_spatial leaves at once)
    long_mom = mom.copy()
    long_mom[..., 2], long_mom[..., 3] = np.where(mom[..., 2] > 0, 16.0, 0.0), 1.0 / 16
    draw, dfull, dacc = t(raw), t(np.repeat(np.repeat(raw, f, 0), f, 1)), t(acc)
    oc, om, ov = (torch.zeros((H, W, k), dtype=torch.float64, device="cuda") for k in (3, 4, 1))
    ptr = lambda d: {k: a.data_ptr() for k, a in d.items()}
    ms = lambda s: [x * 1e3 for x in s[2:]]
    res = {"size": "%dx%d" % (W, H), "runs": runs, "largest_n_of_the_sequence_history": float(mom[..., 2].max())}
    for name, m in (("sequence_history", mom), ("long_history", long_mom)):
        dmom = t(m)
        torch.cuda.synchronize()
        prev = (full, ptr(dpG), dacc.data_ptr(), dmom.data_ptr())
        tu, ta = [], []
        for k in range(runs + 2):
            a, b = mcpt.upsample_phase(f, k)
            tu.append(mcpt.temporal_upsample_device(w, h, draw.data_ptr(), ptr(dG), a, b, oc.data_ptr(), om.data_ptr(), ov.data_ptr(),
                                                    prev=prev, factor=f)[2])
            ta.append(mcpt.temporal_accumulate_device(W, H, dfull.data_ptr(), ptr(dG), oc.data_ptr(), om.data_ptr(), ov.data_ptr(),
                                                      prev=prev))
        res[name] = {"temporal_upsample_ms": ms(tu), "temporal_accumulate_ms": ms(ta),
                     "median_temporal_upsample_ms": statistics.median(ms(tu)),
                     "median_temporal_accumulate_ms": statistics.median(ms(ta))}
    # without a previous state every untraced pixel runs the fill and every pixel the spatial estimate, in both calls
    tu = [mcpt.temporal_upsample_device(w, h, draw.data_ptr(), ptr(dG), 0, 0, oc.data_ptr(), om.data_ptr(), ov.data_ptr(),
                                        factor=f)[2] for _ in range(runs + 2)]
    ta = [mcpt.temporal_accumulate_device(W, H, dfull.data_ptr(), ptr(dG), oc.data_ptr(), om.data_ptr(), ov.data_ptr())
          for _ in range(runs + 2)]
    res["first_frame"] = {"median_temporal_upsample_ms": statistics.median(ms(tu)), "median_temporal_accumulate_ms": statistics.median(ms(ta))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=800, help="the shown size")
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--frames", type=int, default=8, help="of the orbit run")
    ap.add_argument("--static-frames", type=int, default=12)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--orbit", type=float, default=0.05, help="degrees per frame")
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--kernel-runs", type=int, default=20)
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/temporal_upsample_benches.txt")
    a = ap.parse_args()
    f = a.factor
    assert a.width % f == 0 and a.height % f == 0
    w, h = a.width // f, a.height // f
    d = os.path.join(ROOT, "scenes", "veach-mis")
    scene = mcpt.Scene.load(os.path.join(d, "veach-mis.obj"), os.path.join(d, "veach-mis.xml"))
    full0, low0 = mcpt.Camera.reference(a.width, a.height), mcpt.Camera.reference(w, h)
    arms = {"native": (mcpt.FrameSequence(scene, a.width, a.height, a.spp, denoise=True), full0, a.spp),
            "upsampled": (mcpt.FrameSequence(scene, w, h, a.spp, denoise=True, upsample=f), low0, a.spp),
            "temporal": (mcpt.FrameSequence(scene, w, h, a.spp, denoise=True, upsample=f, temporal_upsample=True), low0, a.spp),
            "temporal_eq": (mcpt.FrameSequence(scene, w, h, a.spp * f * f, denoise=True, upsample=f, temporal_upsample=True), low0,
                            a.spp * f * f)}
    orbit = run(scene, arms, full0, a.frames, a.orbit, a.ref_spp)
    static = run(scene, arms, full0, a.static_frames, 0.0, a.ref_spp)
    kern = kernels_alone(scene, arms["temporal"][0], low0, f, a.kernel_runs)
    for seq, _, _ in arms.values():
        seq.close()
    res = {"label": a.label,
           "frame": "%dx%d shown, mis, denoise, factor %d, reference %d spp; orbit: %d frames at %g deg/frame; static: %d frames" %
                    (a.width, a.height, f, a.ref_spp, a.frames, a.orbit, a.static_frames),
           "orbit": orbit, "static": static, "kernels": kern}
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "temporal_upsample_benches.txt"), "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
