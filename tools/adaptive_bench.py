#!/usr/bin/env python3
"""Cost of adaptive sampling against the plain render it replaces (profiles/adaptive_benches.txt).

Veach-MIS 800x600, MIS: a plain render at --max-spp, then render_adaptive with the same cap; prints one JSON
line with the adaptive call's total samples, device seconds and Msamples/s, the plain render's, the time ratio
and the relative L2 between the two images.  With a library built with -DMCPT_ADAPTIVE_DIAG=1 (through
MCPT_LIB_PATH) the library's "adaptive diag:" lines on stderr give the wavefront runs, their drain time and the
time in the adaptive kernels of each call, in call order.

  python tools/adaptive_bench.py [--max-spp 1024 --min-spp 64 --pass-spp 64 --radius 1 --threshold 0.05]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import monte_carlo_path_tracing_amd as mcpt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--min-spp", type=int, default=64)
    ap.add_argument("--pass-spp", type=int, default=64)
    ap.add_argument("--radius", type=int, default=1)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--mode", default="mis")
    ap.add_argument("--repeat", type=int, default=2, help="timed calls of each kind (the fastest is reported)")
    a = ap.parse_args()
    d = os.path.join(ROOT, "scenes", "veach-mis")
    scene = mcpt.Scene.load(os.path.join(d, "veach-mis.obj"), os.path.join(d, "veach-mis.xml"))
    cam = mcpt.Camera.reference(a.width, a.height)
    mcpt.render(scene, cam, 16, mode=a.mode)  # warm-up: device state, buffers
    plain = [mcpt.render(scene, cam, a.max_spp, mode=a.mode) for _ in range(a.repeat)]
    adapt = [mcpt.render_adaptive(scene, cam, a.max_spp, a.threshold, min_spp=a.min_spp, pass_spp=a.pass_spp,
                                  radius=a.radius, mode=a.mode) for _ in range(a.repeat)]
    pimg, pst = min(plain, key=lambda r: r[1].seconds)
    img, count, noise, st = min(adapt, key=lambda r: r[3].seconds)
    res = {
        "frame": "%dx%d %s" % (a.width, a.height, a.mode),
        "adaptive": {"max_spp": a.max_spp, "min_spp": a.min_spp, "pass_spp": a.pass_spp, "radius": a.radius,
                     "threshold": a.threshold},
        "adaptive_samples": int(st.camera_samples),
        "adaptive_mean_spp": float(count.mean()),
        "adaptive_pixels_at_cap": float((count >= a.max_spp).mean()),
        "adaptive_device_seconds": st.seconds,
        "adaptive_msamples_per_s": st.camera_samples / st.seconds * 1e-6,
        "adaptive_generations": int(st.generations),
        "plain_samples": int(pst.camera_samples),
        "plain_device_seconds": pst.seconds,
        "plain_msamples_per_s": pst.camera_samples / pst.seconds * 1e-6,
        "plain_generations": int(pst.generations),
        "time_ratio_adaptive_over_plain": st.seconds / pst.seconds,
        "sample_ratio_adaptive_over_plain": st.camera_samples / pst.camera_samples,
        "rel_l2_adaptive_vs_plain": float(np.linalg.norm(img - pimg) / np.linalg.norm(pimg)),
        "all_seconds": {"plain": [r[1].seconds for r in plain], "adaptive": [r[3].seconds for r in adapt]},
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
