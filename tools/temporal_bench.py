#!/usr/bin/env python3
"""Cost and effect of the temporal accumulation on a low-sample orbit (profiles/temporal_benches.txt).

Veach-MIS 800x600: renders --frames frames of --spp samples along an orbit of --orbit degrees a frame (frame k
at seed + k), accumulates them (mcpt_temporal_accumulate through TemporalAccumulator) and compares, against an
independent --ref-spp frame at the last camera (seed + 100), the raw last frame, the denoised last frame (spatial
variance), the accumulated frame and the accumulated + denoised frame (temporal variance): tone-mapped relative
L2 and relative MSE.  Times one accumulate call (device seconds of its kernels, HIP events; median, fastest and
all of --repeat calls after a warm-up) in two states -- the second frame of a sequence, where every history is
short and the spatial estimate runs in every lane, and the last frame, where it runs only in the pixels that
lost their history -- next to one a-trous iteration (mcpt_denoise with a supplied variance, iterations = 1: one
k_atrous launch) on the same frame, and the bytes the accumulate kernel moves per pixel, counted from the rule:
requested = own 10 doubles + 4 taps x 14 + 8 written (3 colour, 4 moments, 1 variance), unique = the same with
each previous pixel counted once.
History clamping (mcpt_temporal_accumulate_clamped, TemporalAccumulator(clamp=True)): the same three states of the
clamped call are timed beside the plain one ("clamped_*"; the difference is the fast history's gather and
k_temporal_clamp), the main sequence gains its clamped rows, and "quality_by_orbit" renders the sequence again at each
step of --orbits (degrees a frame) and reports the accumulated and the clamped frame, unfiltered and denoised, against
that sequence's own reference.
Prints one JSON line; --append adds it to profiles/temporal_benches.txt.

  python tools/temporal_bench.py [--repeat 9 --append]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import monte_carlo_path_tracing_amd as mcpt  # noqa: E402

SEED = mcpt.DEFAULT_SEED


def tm(x):
    return np.minimum(np.maximum(x, 0.0) / 380.0, 1.0) ** 0.25


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def rel_mse(a, ref):
    d = a - ref
    return float(np.mean((d * d).sum(-1) / ((ref * ref).sum(-1) + 1e-2)))


def metrics(a, ref):
    return {"tone_mapped_rel_l2": rel_l2(tm(a), tm(ref)), "rel_mse": rel_mse(a, ref)}


def timed(fn, repeat):
    fn()  # warm-up: code object load, allocations
    t = [fn() * 1e3 for _ in range(repeat)]
    return {"median_ms": statistics.median(t), "fastest_ms": min(t), "all_ms": t}


def sequence(scene, cam0, a, orbit):
    """the frames of one orbit through the plain and the clamped accumulator -> what main() reports of them"""
    acc, cl = mcpt.TemporalAccumulator(), mcpt.TemporalAccumulator(clamp=True)
    states, cstates, kept, moved, render_s = [], [], [], [], []
    for k in range(a.frames):
        cam = mcpt.camera_orbit(cam0, k * orbit)
        img, st = mcpt.render(scene, cam, a.spp, seed=SEED + k)
        aov = mcpt.render_aovs(scene, cam)
        states.append((img, aov, acc.state))
        cstates.append((img, aov, cl.state))
        out, var = acc.push(cam, img, aov)
        cout, cvar = cl.push(cam, img, aov)
        kept.append(acc.kept)
        moved.append(cl.clamped)
        render_s.append(st.seconds)
    ref, _ = mcpt.render(scene, cam, a.ref_spp, seed=SEED + 100)
    rows = {"raw_last_frame": metrics(img, ref),
            "denoised_last_frame": metrics(mcpt.denoise(img, aov)[0], ref),
            "accumulated": metrics(out, ref),
            "accumulated_denoised": metrics(mcpt.denoise(out, aov, variance=var)[0], ref),
            "clamped": metrics(cout, ref),
            "clamped_denoised": metrics(mcpt.denoise(cout, aov, variance=cvar)[0], ref),
            "pixels_moved_by_the_clamp": moved}
    return dict(states=states, cstates=cstates, kept=kept, render_s=render_s, rows=rows, acc=acc, out=out, var=var, aov=aov)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--orbit", type=float, default=0.3, help="degrees per frame")
    ap.add_argument("--orbits", default="0.012,0.05,0.3", help="steps of the quality rows with and without the clamp")
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--repeat", type=int, default=9, help="timed calls of each kind")
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/temporal_benches.txt")
    a = ap.parse_args()
    d = os.path.join(ROOT, "scenes", "veach-mis")
    scene = mcpt.Scene.load(os.path.join(d, "veach-mis.obj"), os.path.join(d, "veach-mis.xml"))
    cam0 = mcpt.Camera.reference(a.width, a.height)
    mcpt.render(scene, cam0, 16)  # warm-up: device state, buffers
    q = sequence(scene, cam0, a, a.orbit)
    states, cstates, kept, render_s, acc, out, var, aov = (q[k] for k in ("states", "cstates", "kept", "render_s", "acc", "out", "var", "aov"))
    npx = a.width * a.height
    call = lambda s: (lambda: mcpt.temporal_accumulate(s[0], s[1], s[2])[3])
    ccall = lambda s: (lambda: mcpt.temporal_accumulate_clamped(s[0], s[1], s[2])[5])
    res = {
        "label": a.label,
        "frame": "%dx%d mis, %d frames of %d spp, orbit %g deg/frame" % (a.width, a.height, a.frames, a.spp, a.orbit),
        "accumulate_second_frame": timed(call(states[1]), a.repeat),
        "accumulate_last_frame": timed(call(states[-1]), a.repeat),
        "accumulate_first_frame_no_history": timed(call(states[0]), a.repeat),
        "clamped_second_frame": timed(ccall(cstates[1]), a.repeat),
        "clamped_last_frame": timed(ccall(cstates[-1]), a.repeat),
        "clamped_first_frame_no_history": timed(ccall(cstates[0]), a.repeat),
        "atrous_one_iteration": timed(lambda: mcpt.denoise(out, aov, variance=var, iterations=1)[2], a.repeat),
        "bytes_per_pixel": {"requested": 8 * (10 + 4 * 14 + 8), "unique": 8 * (10 + 14 + 8)},
        "render_device_seconds_per_frame": render_s,
        "pixels_with_history": kept,
        "mean_history_length_last_frame": float(acc.moments[..., 2].mean()),
        "ref_spp": a.ref_spp,
        **q["rows"],
        "quality_by_orbit": {o: sequence(scene, cam0, a, float(o))["rows"] for o in a.orbits.split(",") if o},
    }
    t = res["accumulate_last_frame"]["median_ms"] * 1e-3
    res["accumulate_last_frame_GBps"] = {k: v * npx / t * 1e-9 for k, v in res["bytes_per_pixel"].items()}
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "temporal_benches.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
