"""Object motion in the temporal accumulation without a GPU (mcpt_scene_pose_save, mcpt_render_motion_aovs,
mcpt_temporal_accumulate_motion, mcpt_sequence_set_motion; include/mcpt.h states the rule): the ABI, every refusal of
the new entry points, the host half of the pose save, the CLI's usage errors -- and the inputs of the GPU tests
(tests/test_motion.py), pinned here with the numpy emulator alone.

The motion emulator is test_temporal's `emulate_temporal` (test_temporal_clamp's `emulate_clamped` with a clamp) called
with guides whose position and normal are replaced by the motion arrays; depth stays the current one, and the spatial
estimate of the variance is recomputed from the CURRENT guides, as the rule says.

Two kinds of input:
  * motion_case(ww, hh, move): test_temporal's analytic scene (floor, wall, slab) ray cast at ww x hh from two cameras
    4 degrees apart, a random current colour and previous history (analytic_inputs' recipe; at 37 x 29 its arrays
    themselves), and synthetic motion arrays: the slab's pixels get a rigid motion -- a translation in the slab's plane
    and a rotation of the normal by 8 degrees about y (N . N' = 0.990, inside normal_min = 0.9; the plane test then
    reads |sin 8 (z' - z)|).  KEEP is a translation of a few hundredths of a pixel, under which the slab keeps its
    history; LOSE one of (0, 0.5, 0.8), which sends a band along the slab's silhouette to the wall and floor behind.
  * plate_frames(orbit): the Veach stand-in seen from motion_camera() (above plate 2, facets [36, 48), so that its top
    face fills a third of a 32 x 24 frame), six poses of the plate, each STEP = 0.5 along the top face's normal further:
    0.5 > plane_max * depth = 0.02 * 17 at the far end, so the plain rule's plane test fails on the plate in every
    frame.  Guides from pyoracle's hits in an OBJ rewritten for each pose, motion arrays in numpy from (facet, beta,
    gamma) and the previous pose's vertices."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE_OBJ, SCENE_XML
import monte_carlo_path_tracing_amd as mcpt
from oracle import pyoracle as po
from test_denoise import aovs_from_hits, lum, spatial_variance, synthetic
from test_scene_update_cpu import fresh, translated
from test_temporal import (AORBIT, DEFAULTS, LOW, analytic_camera, analytic_inputs, dilate, emulate_temporal, ray_cast,
                           taps_touch)
from test_temporal_clamp import CLAMP, emulate_clamped

CLI = os.path.join(ROOT, "monte_carlo_path_tracing_amd", "mcpt_render")
SCENE_BASE = os.path.splitext(str(SCENE_OBJ))[0]
KEYS = ("albedo", "normal", "position", "depth")
NEW_SYMBOLS = ("mcpt_scene_pose_save", "mcpt_render_motion_aovs", "mcpt_render_motion_aovs_device",
               "mcpt_temporal_accumulate_motion", "mcpt_temporal_accumulate_motion_device", "mcpt_sequence_set_motion",
               "mcpt_sequence_motion_info")
PLATE = (36, 48)  # the second plate of the stand-in; its non-light facets are [0, 72)
W, H, FRAMES, SPP = 32, 24, 6, 2
STEP_LENGTH = 0.5  # per frame, along the plate's top normal
ORBIT = 1.5
SIZES = [(1, 1), (5, 3), (2, 70), (32, 24), (37, 29)]  # the edges of the 64 x 4 block, several blocks, analytic_inputs' own
KEEP, LOSE = (0.0, 0.02, -0.05), (0.0, 0.5, 0.8)  # translations in the slab's plane x = 0
ROTATION = 8.0  # degrees about y, of the slab's previous normal
SLAB_ALBEDO = (0.3, 0.5, 0.7)


# ---- the rule in numpy ----

def emulate_motion(color, g, motion, prev=None, clamp=None, **opts):
    """emulate_temporal's (clamp None) or emulate_clamped's outputs for the motion form of the rule"""
    gm = dict(g, position=np.asarray(motion["prev_position"], np.float64), normal=np.asarray(motion["prev_normal"], np.float64))
    o = dict(DEFAULTS, **opts)
    v0 = lambda out: spatial_variance(out, g, o["sigma_normal"], o["sigma_plane"], o["sigma_albedo"])
    if clamp is None:
        out, mom, var, info = emulate_temporal(color, gm, prev, **opts)
        return out, mom, np.where(info["temporal"], var, v0(out)), info
    out, mom, fast, var, shift, info = emulate_clamped(color, gm, prev, None if clamp is True else clamp, **opts)
    return out, mom, fast, np.where(info["temporal"], var, v0(out)), shift, info


# ---- inputs: the analytic frames with synthetic motion ----

_cpu = {}


def motion_case(ww, hh, move):
    """((cam0, g0, pcol, pmom, pfast), g1, color, motion, slab): the previous state, the current guides and colour, the
    motion arrays for the translation `move` and the mask of the slab's pixels"""
    if (ww, hh) not in _cpu:
        if (ww, hh) == (37, 29):
            cam0, g0, pcol, pmom, cam1, g1, color = analytic_inputs()
            rng = np.random.default_rng(13)
        else:
            rng = np.random.default_rng(1000 * ww + hh)
            cam0 = analytic_camera()
            cam0.width, cam0.height = ww, hh
            cam1 = mcpt.camera_orbit(cam0, AORBIT)
            g0, g1 = ray_cast(cam0), ray_cast(cam1)
            color, pcol = rng.uniform(0.0, 2.0, (hh, ww, 3)), rng.uniform(0.0, 2.0, (hh, ww, 3))
            m1 = lum(pcol)
            n = rng.integers(1, 65, (hh, ww)).astype(np.float64)
            pick = rng.uniform(size=(hh, ww))
            n[pick < 0.1], n[pick > 0.85] = 0.0, 64.0
            var = rng.uniform(0.0, 0.3, (hh, ww))
            var[rng.uniform(size=(hh, ww)) < 0.2] = 0.0
            pmom = np.stack([m1, m1 * m1 + var, n, 1.0 / np.maximum(n, 1.0)], -1)
        pfast = pcol + rng.uniform(-3.0, 3.0, pcol.shape)
        _cpu[ww, hh] = ((cam0, g0, pcol, pmom, pfast), g1, color)
    prev, g1, color = _cpu[ww, hh]
    slab = (g1["depth"] > 0) & np.all(g1["albedo"] == np.array(SLAB_ALBEDO), -1)
    t = np.deg2rad(ROTATION)
    mo = dict(prev_position=np.where(slab[..., None], g1["position"] - np.array(move), g1["position"]),
              prev_normal=np.where(slab[..., None], np.array([np.cos(t), 0.0, np.sin(t)]), g1["normal"]))
    return prev, g1, color, mo, slab


# ---- inputs: the moving plate of the Veach stand-in ----

def motion_camera(width=W, height=H):
    """above plate 2, looking down its top face's normal: the face spans the width and 10 to 12 of the 24 rows of a 32 x 24 frame
    (the renderer's half field of view is tan(fovy / 360))"""
    c = mcpt.Camera()
    c.eye[:] = (10.0, 14.0, 0.0)
    c.lookat[:] = (-0.5, 2.85, 0.0)
    c.up[:] = (0.0, 1.0, 0.0)
    c.fovy, c.dist_scale, c.width, c.height = 60.0, 1.0, width, height
    return c


def veach_arrays():
    if "veach" not in _cpu:
        _cpu["veach"] = mcpt.Scene.load(SCENE_OBJ, SCENE_XML).arrays()
    return _cpu["veach"]


def plate_step(arr):
    """STEP_LENGTH along the unique normal of the plate's top face (the one that points up most)"""
    n = arr["unique_normal"][PLATE[0]:PLATE[1]]
    return tuple(float(v) for v in STEP_LENGTH * n[np.argmax(n[:, 1])])


def plate_pose(arr, k):
    """the plate's positions in frame k: float(double(original) + k * step), the CLI's --move arithmetic"""
    return translated(arr["positions"][PLATE[0]:PLATE[1]], k * np.array(plate_step(arr)))


def posed(arr, k):
    out = dict(arr)
    out["positions"] = arr["positions"].copy()
    out["positions"][PLATE[0]:PLATE[1]] = plate_pose(arr, k)
    return out


def write_posed_obj(folder, arr, k):
    """the stand-in's OBJ with plate 2's vertices at pose k (its MTL and XML beside it) -> (obj, xml)"""
    lines = open(SCENE_OBJ).read().splitlines()
    vline = [i for i, ln in enumerate(lines) if ln.startswith("v ")]
    start = lines.index("o plate2")
    faces = [i for i in range(start + 1, len(lines)) if lines[i].startswith("f ")][:PLATE[1] - PLATE[0]]
    new = plate_pose(arr, k).reshape(-1, 3, 3)
    for fi, i in enumerate(faces):
        for c, tok in enumerate(lines[i].split()[1:]):
            lines[vline[int(tok.split("/")[0]) - 1]] = "v %.9g %.9g %.9g" % tuple(new[fi, c])
    os.makedirs(folder, exist_ok=True)
    obj = os.path.join(folder, "veach-mis.obj")
    with open(obj, "w") as f:
        f.write("\n".join(lines) + "\n")
    for ext in (".mtl", ".xml"):
        shutil.copy(SCENE_BASE + ext, os.path.join(folder, "veach-mis" + ext))
    return obj, os.path.join(folder, "veach-mis.xml")


def motion_from_hits(f, tbg, arr_prev, hh, ww):
    """the motion AOVs in numpy: node_point over the previous pose's arrays (aovs_from_hits' position and normal)"""
    a = aovs_from_hits(f, tbg, arr_prev, np.zeros(3), hh, ww)
    return dict(prev_position=a["position"], prev_normal=a["normal"])


def plate_frames(orbit, tmp):
    """per frame k of the six: (camera, colour, guides, motion arrays, plate mask), guides from pyoracle's hits in the
    OBJ of pose k, the colour random (a history's length does not depend on it)"""
    if ("plate", orbit) not in _cpu:
        arr = veach_arrays()
        rng = np.random.default_rng(17)
        frames = []
        for k in range(FRAMES):
            obj, xml = write_posed_obj(os.path.join(str(tmp), "pose%d" % k), arr, k)
            osc = po.Scene(obj, xml)
            v = osc.facets()[0]
            cur, before = posed(arr, k), posed(arr, max(k - 1, 0))
            assert np.array_equal(v[:, :9].astype(np.float32), cur["positions"])  # the rewritten OBJ is pose k
            cam = mcpt.camera_orbit(motion_camera(), k * orbit)
            ocam = po.Camera.from_buffer_copy(cam)
            eye, _ = po.camera_ray(ocam, 0, 0)
            osc.build_grid(eye)
            f, tbg = np.zeros(W * H, np.int32), np.zeros((W * H, 3))
            for p in range(W * H):
                f[p], tbg[p] = osc.closest_hit(eye, po.camera_ray(ocam, p // W, p % W)[1])
            g = aovs_from_hits(f, tbg, cur, eye, H, W)
            on_plate = ((f >= PLATE[0]) & (f < PLATE[1])).reshape(H, W)
            frames.append((cam, rng.uniform(0.0, 2.0, (H, W, 3)), g, motion_from_hits(f, tbg, before, H, W), on_plate))
        _cpu["plate", orbit] = frames
    return _cpu["plate", orbit]


def considered(masks):
    """the pixels at least 2 px inside the silhouette of every mask given (the plate's in the last two frames: a hit on
    the plate in consecutive frames)"""
    out = np.ones_like(masks[0])
    for m in masks:
        out &= ~dilate(~m, 2)
    return out


def history_lengths(frames, with_motion):
    """n of the last frame of the emulator's chain, and the share of pixels a low margin tainted on the way"""
    prev, tainted = None, None
    for cam, img, g, mo, _ in frames:
        c, m, v, info = emulate_motion(img, g, mo, prev) if with_motion else emulate_temporal(img, g, prev, **DEFAULTS)
        low = info["margin"] < LOW
        tainted = low if tainted is None else low | taps_touch(tainted, info)
        prev = (cam, g, c, m)
    return m[..., 2], tainted


# ---- the tests ----

def test_motion_symbols_are_exported():
    hdr = (ROOT / "include" / "mcpt.h").read_text()
    declared = set(re.findall(r"\b(mcpt_[a-z_0-9]+)\s*\(", hdr))
    L = mcpt.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in mcpt.EXPORTS and hasattr(L, name), name
    for name in ("MotionBuffers", "render_motion_aovs", "render_motion_aovs_device", "temporal_accumulate_motion",
                 "temporal_accumulate_motion_device"):
        assert name in mcpt.__all__ and hasattr(mcpt, name), name
    assert hasattr(mcpt.Scene, "pose_save") and hasattr(mcpt.FrameSequence, "motion_info")
    assert re.search(r"MCPT_SEQ_PREV_POSITION = 9, MCPT_SEQ_PREV_NORMAL = 10", hdr)
    assert mcpt.SEQ_MOTION_BUFFERS == {"prev_position": (9, (3,)), "prev_normal": (10, (3,))}
    assert L.mcpt_version() == mcpt.MCPT_VERSION == 20300


def test_motion_buffers_layout_matches_header(tmp_path):
    py = mcpt.MotionBuffers
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mcpt.h"', "int main(void) {",
           'printf("sizeof %zu\\n", sizeof(mcpt_motion_buffers));']
    for f, _ in py._fields_:
        src.append('printf("%s %%zu\\n", offsetof(mcpt_motion_buffers, %s));' % (f, f))
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(py)
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset, f


def test_pose_save_then_update_returns_the_new_arrays():
    """the host half: the previous pose is a copy, so an update after the save shows in mcpt_scene_arrays as always"""
    arr = veach_arrays()
    scene = fresh(arr)
    scene.pose_save()
    assert all(np.array_equal(scene.arrays()[k], arr[k]) for k in arr)
    new, nrm = plate_pose(arr, 3), -arr["normals"][PLATE[0]:PLATE[1]]
    scene.update(PLATE[0], new, nrm)
    scene.pose_save()
    scene.update(PLATE[0], plate_pose(arr, 4))
    got = scene.arrays()
    want = posed(arr, 4)
    want["normals"] = arr["normals"].copy()
    want["normals"][PLATE[0]:PLATE[1]] = nrm
    assert np.array_equal(got["positions"], want["positions"]) and np.array_equal(got["normals"], want["normals"])
    assert mcpt.lib().mcpt_scene_pose_save(None) == -1 and "NULL scene" in mcpt.lib().mcpt_last_error().decode()


def _accumulate(clamped=False, null=(), alias=None, extra=(), opts=None, clamp_opts=None, width=6, height=4, prev_size=None):
    """mcpt_temporal_accumulate_motion on a 6 x 4 frame with the given changes to a valid call -> (rc, message)"""
    color, _, g = synthetic(6, 4)
    o = mcpt.TemporalOpts()
    mcpt.lib().mcpt_temporal_opts_init(C.byref(o))
    for k, v in (opts or {}).items():
        setattr(o, k, v)
    c = mcpt.TemporalClampOpts()
    mcpt.lib().mcpt_temporal_clamp_opts_init(C.byref(c))
    for k, v in (clamp_opts or {}).items():
        setattr(c, k, v)
    cam = mcpt.Camera.reference(*(prev_size or (6, 4)))
    ins = dict(color=color, prev_color=np.ones((4, 6, 3)), prev_moments=np.ones((4, 6, 4)), prev_fast=np.ones((4, 6, 3)),
               prev_position=g["position"].copy(), prev_normal=g["normal"].copy())
    outs = dict(out_color=np.full((4, 6, 3), 7.0), out_moments=np.full((4, 6, 4), 7.0), out_fast=np.full((4, 6, 3), 7.0),
                out_shift=np.full((4, 6), 7.0), out_variance=np.full((4, 6), 7.0))
    ptr = {k: a.ctypes.data for k, a in {**ins, **outs}.items()}
    if not clamped:
        for k in ("prev_fast", "out_fast", "out_shift"):
            ptr[k] = None
    for k in extra:  # a clamped rule's argument given to the plain rule
        ptr[k] = {**ins, **outs}[k].ctypes.data
    if alias:
        ptr[alias[0]] = ptr[alias[1]] if alias[1] in ptr else g[alias[1]].ctypes.data
    for k in null:
        if k in ptr:
            ptr[k] = None
    b = mcpt.AovBuffers(*[None if k in null else g[k].ctypes.data for k in KEYS])
    pb = mcpt.AovBuffers(*[None if "pg_" + k in null else g[k].ctypes.data for k in KEYS])  # pg_*: a field of prev_guides
    mb = mcpt.MotionBuffers(ptr["prev_position"], ptr["prev_normal"])
    rc = mcpt.lib().mcpt_temporal_accumulate_motion(
        C.byref(o), C.byref(c) if clamped else None, None if "prev_cam" in null else C.byref(cam), width, height, ptr["color"],
        None if "guides" in null else C.byref(b), None if "motion" in null else C.byref(mb),
        None if "prev_guides" in null else C.byref(pb), ptr["prev_color"], ptr["prev_moments"], ptr["prev_fast"], ptr["out_color"],
        ptr["out_moments"], ptr["out_fast"], ptr["out_shift"], ptr["out_variance"], None)
    for a in outs.values():
        assert np.all(a == 7.0)
    return rc, mcpt.lib().mcpt_last_error().decode()


NAN, INF = float("nan"), float("inf")
PLAIN_REFUSALS = [
    (dict(opts={"struct_size": 8}), "struct_size"),
    *[(dict(opts={"alpha": v}), "alpha") for v in (0.0, 1.5, NAN)],
    (dict(opts={"max_history": 0}), "max_history"),
    (dict(opts={"normal_min": NAN}), "normal_min"),
    *[(dict(opts={"min_weight": v}), "min_weight") for v in (0.0, 1.5)],
    (dict(opts={"variance_min_history": 1}), "variance_min_history"),
    *[(dict(opts={s: v}), s) for s in ("plane_max", "sigma_normal", "sigma_plane", "sigma_albedo") for v in (0.0, INF)],
    (dict(width=0), "width"),
    (dict(height=0), "height"),
    *[(dict(null=(k,)), k) for k in ("color", "out_color", "out_moments", "guides", *KEYS)],
    *[(dict(null=(k,)), k) for k in ("prev_cam", "prev_guides", "prev_color", "prev_moments")],
    *[(dict(null=("pg_" + k,)), "prev_guides." + k) for k in ("normal", "position", "depth")],
    (dict(null=("prev_cam", "prev_guides", "prev_color")), "partial previous state"),
    (dict(prev_size=(6, 5)), "prev_cam"),
    *[(dict(alias=a), "aliasing") for a in (("out_color", "color"), ("out_color", "prev_color"), ("out_moments", "prev_moments"),
                                            ("out_variance", "depth"), ("out_color", "normal"), ("out_variance", "out_moments"))],
    # the motion arrays: required, and no output may alias them
    (dict(null=("motion",)), "motion (the struct)"),
    (dict(null=("prev_position",)), "motion (prev_position)"),
    (dict(null=("prev_normal",)), "motion (prev_normal)"),
    *[(dict(alias=(w, r)), "aliasing motion." + r) for w in ("out_color", "out_variance") for r in ("prev_position", "prev_normal")],
]
CLAMPED_REFUSALS = [
    (dict(clamp_opts={"struct_size": 8}), "mcpt_temporal_clamp_opts.struct_size"),
    *[(dict(clamp_opts={"radius": v}), "radius") for v in (0, 4)],
    *[(dict(clamp_opts={"alpha_fast": v}), "alpha_fast") for v in (0.0, 1.5)],
    *[(dict(clamp_opts={"sigma": v}), "sigma") for v in (-1.0, NAN)],
    (dict(null=("out_fast",)), "out_fast"),
    (dict(null=("prev_fast",)), "prev_fast"),
    (dict(null=("prev_cam", "prev_guides", "prev_color", "prev_moments")), "prev_fast"),
    *[(dict(alias=a), "aliasing") for a in (("out_fast", "prev_fast"), ("out_shift", "depth"), ("out_color", "prev_fast"),
                                            ("out_fast", "prev_position"), ("out_shift", "prev_normal"))],
]


@pytest.mark.parametrize("kw,word", PLAIN_REFUSALS + [(dict(kw, clamped=True), word) for kw, word in PLAIN_REFUSALS + CLAMPED_REFUSALS] + [
    (dict(extra=(k,)), k + " is given without clamp") for k in ("prev_fast", "out_fast", "out_shift")])
def test_invalid_motion_accumulate_calls_are_refused(kw, word):
    """MCPT_E_INVALID with a message naming the argument, before any device work; the outputs stay untouched"""
    rc, msg = _accumulate(**kw)
    assert rc == -1, (rc, msg)
    assert word in msg, msg


@pytest.mark.parametrize("clamped", [False, True])
def test_valid_motion_accumulate_calls_pass_the_argument_checks(clamped):
    """the call then goes on to the device: no such device, after every argument check (also of the device form)"""
    rc, msg = _accumulate(clamped=clamped, opts={"device": 1 << 20})
    assert rc != 0 and "device" in msg and "null" not in msg and "aliasing" not in msg, (rc, msg)
    rc, msg = _accumulate(clamped=clamped, opts={"device": 1 << 20}, null=("prev_cam", "prev_guides", "prev_color", "prev_moments", "prev_fast"))
    assert rc != 0 and "device" in msg and "partial" not in msg, (rc, msg)


def test_invalid_motion_aov_calls_are_refused():
    """mcpt_render_motion_aovs' refusals are mcpt_render_aovs', message for message"""
    L = mcpt.lib()
    scene = fresh(veach_arrays())
    cam, o = mcpt.Camera.reference(6, 4), mcpt._aov_opts(None, "bvh")
    a = np.zeros((4, 6, 3))
    mb, ab = mcpt.MotionBuffers(a.ctypes.data, a.ctypes.data), mcpt.AovBuffers(None, a.ctypes.data, a.ctypes.data, None)
    devs = (C.c_int32 * 2)(0, 0)

    def both(change, word):
        for fn, fa, b in ((L.mcpt_render_motion_aovs, L.mcpt_render_aovs, (mb, ab)), (L.mcpt_render_motion_aovs_device,
                                                                                    L.mcpt_render_aovs_device, (mb, ab))):
            msgs = []
            for f, buf in ((fn, b[0]), (fa, b[1])):
                c2, o2 = mcpt.Camera.from_buffer_copy(cam), mcpt.RenderOpts.from_buffer_copy(o)
                args = dict(scene=scene.h, cam=C.byref(c2), opts=C.byref(o2), out=C.byref(buf))
                change(args, c2, o2)
                assert f(args["scene"], args["cam"], args["opts"], args["out"]) == -1
                msgs.append(L.mcpt_last_error().decode())
            assert word in msgs[0] and msgs[0].replace("mcpt_render_motion_aovs", "mcpt_render_aovs") == msgs[1], msgs

    both(lambda a, c, o: a.update(scene=None), "null argument")
    both(lambda a, c, o: a.update(opts=None), "null argument")
    both(lambda a, c, o: a.update(out=None), "null argument")
    both(lambda a, c, o: setattr(o, "struct_size", 8), "struct_size")
    both(lambda a, c, o: (setattr(o, "num_devices", 2), setattr(o, "devices", C.cast(devs, C.POINTER(C.c_int32)))), "single-device")
    both(lambda a, c, o: setattr(o, "accel", 7), "accel")
    both(lambda a, c, o: setattr(c, "width", 0), "camera")
    both(lambda a, c, o: setattr(c, "dist_scale", 0.0), "camera")
    both(lambda a, c, o: a.update(cam=None), "camera")
    assert np.all(a == 0)


def test_calls_without_a_sequence_are_refused():
    L = mcpt.lib()
    s = C.c_double()
    assert L.mcpt_sequence_set_motion(None, 1) == -1 and "null mcpt_sequence" in L.mcpt_last_error().decode()
    assert L.mcpt_sequence_motion_info(None, C.byref(s)) == -1 and "null mcpt_sequence" in L.mcpt_last_error().decode()


@pytest.mark.parametrize("args,word", [
    (["--motion"], "--frames"),
    (["--denoise", "--motion"], "--frames"),
    (["--frames", "2", "--motion", "--upsample", "2"], "--upsample"),
    (["--frames", "2", "--device-sequence", "--motion", "--upsample", "2", "--temporal-upsample"], "--upsample"),
])
def test_cli_motion_usage_errors(args, word):
    """refused before anything is loaded or any device is touched"""
    r = subprocess.run([CLI, "--scene", SCENE_BASE, "--width", "16", "--height", "12", "--spp", "1", *args],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--motion" in r.stderr and word in r.stderr, (r.returncode, r.stderr)


@pytest.mark.parametrize("ww,hh", SIZES)
def test_motion_emulator_with_the_current_guides_is_the_plain_emulator(ww, hh):
    prev, g1, color, _, _ = motion_case(ww, hh, KEEP)
    same = dict(prev_position=g1["position"], prev_normal=g1["normal"])
    for a, b in zip(emulate_motion(color, g1, same, prev[:4], **DEFAULTS)[:3], emulate_temporal(color, g1, prev[:4], **DEFAULTS)[:3]):
        assert np.array_equal(a, b)
    for a, b in zip(emulate_motion(color, g1, same, prev, clamp=CLAMP, **DEFAULTS)[:5], emulate_clamped(color, g1, prev, CLAMP, **DEFAULTS)[:5]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("ww,hh", SIZES)
def test_motion_cases_keep_within_the_cap_and_take_both_branches(ww, hh):
    """the inputs of test_motion.py's emulator comparison: at most 1 % of the pixels under check_outputs' margin; at the
    two large sizes the slab keeps its history under KEEP, loses a silhouette band of it under LOSE, and the motion
    form differs from the plain one"""
    hist = {}
    for name, move in (("keep", KEEP), ("lose", LOSE)):
        prev, g1, color, mo, slab = motion_case(ww, hh, move)
        out, mom, var, info = emulate_motion(color, g1, mo, prev[:4], **DEFAULTS)
        assert (info["margin"] < LOW).mean() <= 0.01
        assert (emulate_motion(color, g1, mo, prev, clamp=CLAMP, **DEFAULTS)[5]["margin"] < LOW).mean() <= 0.01
        assert np.isfinite(out).all() and np.isfinite(mom).all() and np.isfinite(var).all()
        hist[name] = info["history"]
        plain = emulate_temporal(color, g1, prev[:4], **DEFAULTS)
        if ww * hh >= 32 * 24:
            assert not np.array_equal(plain[1][..., 2], mom[..., 2])
    print("%d x %d: slab %d pixels, with history %d (keep), %d (lose)" % (ww, hh, slab.sum(), hist["keep"][slab].sum(), hist["lose"][slab].sum()))
    assert slab.any()
    if ww * hh >= 32 * 24:
        assert hist["keep"][slab].mean() >= 0.8
        lost = slab & hist["keep"] & ~hist["lose"]
        assert lost.sum() >= 5 and (slab & hist["lose"]).sum() >= 5


@pytest.mark.parametrize("orbit", [0.0, ORBIT], ids=["static", "orbit"])
def test_the_step_loses_the_plain_history_on_the_plate(orbit, tmp_path_factory):
    """the emulator alone on pyoracle's hits: what test_motion.py's history test asserts of the GPU"""
    frames = plate_frames(orbit, tmp_path_factory.getbasetemp() / "motion_poses")
    px = considered([f[4] for f in frames][-2:])
    n_plain, _ = history_lengths(frames, False)
    n_motion, tainted = history_lengths(frames, True)
    print("orbit %g: %d pixels considered; plain n in [%g, %g], motion n in [%g, %g]; tainted %d"
          % (orbit, px.sum(), n_plain[px].min(), n_plain[px].max(), n_motion[px].min(), n_motion[px].max(), tainted.sum()))
    assert px.sum() >= 40
    assert tainted.mean() <= 0.01
    if orbit == 0.0:
        assert np.all(n_plain[px] == 1) and np.all(n_motion[px] >= 5)
    else:
        assert (n_motion[px] > n_plain[px]).mean() >= 0.9
