#!/usr/bin/env python3
"""Cost and effect of the a-trous denoiser on the adaptive frame (profiles/denoise_benches.txt).

Veach-MIS 800x600 at the README's adaptive configuration (cap 1024, 64 per pass, tau 0.05, radius 1): renders
the plain frame at the cap (the reference image), the adaptive frame, the AOVs, and filters the adaptive frame
with the variance from its noise map.  Prints one JSON line with the denoiser's device ms (fastest and all of
--repeat calls; also with the spatial variance estimate), the adaptive and plain device seconds, and
tone-mapped relative L2, relative MSE and linear relative L2 of the raw and of the denoised adaptive frame
against the plain one, the same against a plain frame at seed + 1 (independent of the adaptive frame's samples),
and the 4-spp frame raw and denoised against that independent frame.  --append adds the line to profiles/denoise_benches.txt.

  python tools/denoise_bench.py [--iterations 5 --repeat 5 --append]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import monte_carlo_path_tracing_amd as mcpt  # noqa: E402


def tm(x):
    return np.minimum(np.maximum(x, 0.0) / 380.0, 1.0) ** 0.25


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def rel_mse(a, ref):
    d = a - ref
    return float(np.mean((d * d).sum(-1) / ((ref * ref).sum(-1) + 1e-2)))


def metrics(a, ref):
    return {"tone_mapped_rel_l2": rel_l2(tm(a), tm(ref)), "rel_mse": rel_mse(a, ref), "linear_rel_l2": rel_l2(a, ref),
            "mean_energy_ratio": float(a.mean() / ref.mean())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--min-spp", type=int, default=64)
    ap.add_argument("--pass-spp", type=int, default=64)
    ap.add_argument("--radius", type=int, default=1)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5, help="timed denoiser calls of each kind (the fastest is reported)")
    ap.add_argument("--label", default="", help="free text stored with the line (e.g. the kernel variant of an A/B build)")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/denoise_benches.txt")
    a = ap.parse_args()
    d = os.path.join(ROOT, "scenes", "veach-mis")
    scene = mcpt.Scene.load(os.path.join(d, "veach-mis.obj"), os.path.join(d, "veach-mis.xml"))
    cam = mcpt.Camera.reference(a.width, a.height)
    mcpt.render(scene, cam, 16)  # warm-up: device state, buffers
    plain, pst = mcpt.render(scene, cam, a.max_spp)
    adapt = [mcpt.render_adaptive(scene, cam, a.max_spp, a.threshold, min_spp=a.min_spp, pass_spp=a.pass_spp,
                                  radius=a.radius) for _ in range(2)]
    img, count, noise, st = min(adapt, key=lambda r: r[3].seconds)
    aov = mcpt.render_aovs(scene, cam)
    var = mcpt.variance_from_noise(img, noise)
    mcpt.denoise(img, aov, variance=var, iterations=a.iterations)  # warm-up: code object load
    runs = [mcpt.denoise(img, aov, variance=var, iterations=a.iterations) for _ in range(a.repeat)]
    spatial = [mcpt.denoise(img, aov, iterations=a.iterations) for _ in range(a.repeat)]
    out = runs[0][0]
    res = {
        "label": a.label,
        "frame": "%dx%d mis" % (a.width, a.height),
        "adaptive": {"max_spp": a.max_spp, "min_spp": a.min_spp, "pass_spp": a.pass_spp, "radius": a.radius,
                     "threshold": a.threshold},
        "iterations": a.iterations,
        "denoise_device_ms": min(r[2] for r in runs) * 1e3,
        "denoise_device_ms_all": [r[2] * 1e3 for r in runs],
        "denoise_spatial_variance_device_ms": min(r[2] for r in spatial) * 1e3,
        "adaptive_device_seconds": st.seconds,
        "adaptive_mean_spp": float(count.mean()),
        "plain_device_seconds": pst.seconds,
        "raw_vs_plain": metrics(img, plain),
        "denoised_vs_plain": metrics(out, plain),
        "denoised_spatial_variance_vs_plain": metrics(spatial[0][0], plain),
    }
    # the plain frame shares its first samples with the adaptive one (a pixel at the cap is the same number in
    # both), which flatters the raw frame; a plain frame at another seed is independent of both
    other, _ = mcpt.render(scene, cam, a.max_spp, seed=mcpt.DEFAULT_SEED + 1)
    res["raw_vs_plain_other_seed"] = metrics(img, other)
    res["denoised_vs_plain_other_seed"] = metrics(out, other)
    # and the low-sample case the filter is for: 4 spp of the same frame
    lo, _, lo_noise, _ = mcpt.render_adaptive(scene, cam, 4, a.threshold, min_spp=4, pass_spp=4, radius=a.radius)
    lo_out, _, lo_sec = mcpt.denoise(lo, aov, variance=mcpt.variance_from_noise(lo, lo_noise), iterations=a.iterations)
    res["spp4_raw_vs_plain_other_seed"] = metrics(lo, other)
    res["spp4_denoised_vs_plain_other_seed"] = metrics(lo_out, other)
    res["spp4_denoise_device_ms"] = lo_sec * 1e3
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "denoise_benches.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
