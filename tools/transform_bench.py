#!/usr/bin/env python3
"""What keeping the host out of a geometry update is worth: mcpt_scene_transform against mcpt_scene_update
(profiles/transform_benches.txt).

Cornell + 1 M random triangles (scenes/gen_cornell_random.py, the C5 scene), one MI355X, one process, the arms taking
turns repetition by repetition after one warm-up round.  Ranges: 1, 1 000 and all facets of the longest non-light run,
turned back and forth between a small rotation about the range's centroid and the identity.
  update          Scene.update of the precomputed arrays (the numpy restatement of the rule, outside the timer)
  update_device   Scene.update_device of the same arrays held in torch tensors on the device
  transform       Scene.transform of the matrix
For each: wall time (time.perf_counter around the call, which ends in a stream synchronisation), the call's
mcpt_update_stats.device_seconds, and, separately, the wall time of one Scene.host_sync right after it (a no-op after
the update arms, whose host copy is current; after transform it is the deferred host half).  The transform arm also
times the same call once more at once (repeat_wall_ms): in the turn-taking the device has idled through the previous
arm's host work, in a frame loop it has not.
Then a frame loop: eight 4-spp frames of a FrameSequence(motion=True) with a tenth of the run rotating a little more
every frame -- pose_save, move, frame -- the move by Scene.update of precomputed arrays against Scene.transform, wall
per frame (frames 1..7); and the transform arm once more with a host_sync every frame, which gives the gain back.
Medians are what README.md and DESIGN.md 4.21 quote.  Prints one JSON line; --append adds it to
profiles/transform_benches.txt.

  python tools/transform_bench.py [--append]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import monte_carlo_path_tracing_amd as mcpt  # noqa: E402
from update_bench import cornell, fresh, longest_non_light_run  # noqa: E402


def restate(pos, nrm, m):
    """the rule of include/mcpt.h in numpy (tests/test_transform_cpu.py)"""
    m = np.asarray(m, np.float64).reshape(3, 4)
    x, y, z = pos.astype(np.float64).reshape(-1, 3).T
    nx, ny, nz = nrm.astype(np.float64).reshape(-1, 3).T
    p = np.stack([((m[r, 0] * x + m[r, 1] * y) + m[r, 2] * z) + m[r, 3] for r in range(3)], axis=1).astype(np.float32)
    q = np.stack([(m[r, 0] * nx + m[r, 1] * ny) + m[r, 2] * nz for r in range(3)], axis=1).astype(np.float32)
    return p.reshape(-1, 9), q.reshape(-1, 9)


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--triangles", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="", help="free text stored with the line")
    ap.add_argument("--append", action="store_true", help="append the line to profiles/transform_benches.txt")
    a = ap.parse_args()
    obj, xml = cornell(a.triangles)
    arr = mcpt.Scene.load(obj, xml).arrays()
    note("scene loaded")
    r0, r1 = longest_non_light_run(arr)
    sizes = {"1": 1, "1000": min(1000, r1 - r0), "all": r1 - r0}
    cam_small = mcpt.Camera.reference(8, 6)
    scene = fresh(arr)
    scene.rest_save()
    mcpt.primary_hits(scene, cam_small)
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    cases = {}
    for k, n in sizes.items():
        first = r0 + (r1 - r0 - n) // 2
        rest_p, rest_n = arr["positions"][first:first + n], arr["normals"][first:first + n]
        m = mcpt.transform_rotation((0.2, 1.0, 0.1), 3.0, rest_p.astype(np.float64).reshape(-1, 3).mean(axis=0))
        poses = [(m,) + restate(rest_p, rest_n, m), (ident,) + restate(rest_p, rest_n, ident)]
        dev = [(torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()) for _, p, q in poses]
        cases[k] = (first, n, poses, dev)
    arms = {k: {arm: {"wall_ms": [], "device_ms": [], "host_sync_ms": []} for arm in ("update", "update_device", "transform")}
            for k in sizes}
    for rep in range(a.reps + 1):  # rep 0 warms up (code objects, the refit state of the device, allocations)
        for k, (first, n, poses, dev) in cases.items():
            m, p, q = poses[rep % 2]
            tp, tq = dev[rep % 2]
            calls = {"update": lambda: scene.update(first, p, q),
                     "update_device": lambda: scene.update_device(first, n, tp.data_ptr(), tq.data_ptr()),
                     "transform": lambda: scene.transform(first, n, m)}
            for arm, call in calls.items():
                w, st = timed(call)
                # the same call again at once: the device has not idled through another arm's host work
                again = timed(call)[0] if arm == "transform" else None
                pending = scene.host_pending()
                ws, _ = timed(scene.host_sync)
                assert (pending == n) == (arm == "transform") and scene.host_pending() == 0
                if rep:
                    v = arms[k][arm]
                    v["wall_ms"].append(w), v["device_ms"].append(st["device_seconds"] * 1e3), v["host_sync_ms"].append(ws)
                    v["stats"] = {s: st[s] for s in ("facets", "leaf_slots", "nodes_refit", "levels")}
                    if again is not None:
                        v.setdefault("repeat_wall_ms", []).append(again)
        note("round %d done" % rep)
    for per in arms.values():
        for v in per.values():
            for s in ("wall", "device", "host_sync"):
                v["median_%s_ms" % s] = statistics.median(v[s + "_ms"])
            if "repeat_wall_ms" in v:
                v["median_repeat_wall_ms"] = statistics.median(v["repeat_wall_ms"])
    # all three arms must have left the same scene behind
    want = {kk: vv.copy() for kk, vv in arr.items()}
    for first, n, poses, _ in cases.values():
        want["positions"][first:first + n], want["normals"][first:first + n] = poses[a.reps % 2][1:]
    got = scene.arrays()
    assert np.array_equal(got["positions"], want["positions"]) and np.array_equal(got["normals"], want["normals"])
    res = {"label": a.label, "scene": "cornell + %d triangles: %d facets, non-light run [%d, %d)" % (a.triangles, len(arr["positions"]), r0, r1),
           "reps": a.reps, "ranges": arms}
    t, u = arms["all"]["transform"], arms["all"]["update"]
    res["all_update_over_transform_wall"] = u["median_wall_ms"] / t["median_wall_ms"]
    res["all_transform_plus_sync_ms"] = t["median_wall_ms"] + t["median_host_sync_ms"]
    # the frame loop: a tenth of the run turning a little more every frame
    n = (r1 - r0) // 10
    first = r0 + (r1 - r0 - n) // 2
    rest_p, rest_n = arr["positions"][first:first + n], arr["normals"][first:first + n]
    pivot = rest_p.astype(np.float64).reshape(-1, 3).mean(axis=0)
    frames = 8
    mats = [mcpt.transform_rotation((0.2, 1.0, 0.1), 2.0 * f, pivot) for f in range(frames)]
    pre = [restate(rest_p, rest_n, m) for m in mats]
    cam = mcpt.Camera.reference(800, 600)
    seq = mcpt.FrameSequence(scene, 800, 600, 4, denoise=False, motion=True)
    loops = {"update": lambda f: scene.update(first, *pre[f]), "transform": lambda f: scene.transform(first, n, mats[f])}

    def sync_too(f):
        scene.transform(first, n, mats[f])
        scene.host_sync()

    loops["transform_sync_every_frame"] = sync_too
    loop_res = {arm: {"frame_wall_ms": [], "move_wall_ms": []} for arm in loops}
    for rnd in range(2):  # round 0 warms up
        for arm, move in loops.items():
            scene.host_sync()
            seq.reset()
            for f in range(frames):
                t0 = time.perf_counter()
                scene.pose_save()
                t1 = time.perf_counter()
                if f:
                    move(f)
                t2 = time.perf_counter()
                seq.frame(cam, mcpt.DEFAULT_SEED + f, readback=False)
                t3 = time.perf_counter()
                if rnd and f:
                    loop_res[arm]["frame_wall_ms"].append((t3 - t0) * 1e3), loop_res[arm]["move_wall_ms"].append((t2 - t1) * 1e3)
            if arm == "transform":
                assert scene.host_pending() == n  # seven frames and the host was never touched
        note("loop round %d done" % rnd)
    for v in loop_res.values():
        v["median_frame_wall_ms"], v["median_move_wall_ms"] = statistics.median(v["frame_wall_ms"]), statistics.median(v["move_wall_ms"])
    res["frame_loop"] = {"moved_facets": n, "frames": frames, "size": "800x600 at 4 spp, motion on, no filter", "arms": loop_res}
    seq.close()
    scene.close()
    line = json.dumps(res)
    print(line)
    if a.append:
        with open(os.path.join(ROOT, "profiles", "transform_benches.txt"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
