"""Object motion in the temporal accumulation on the GPU (mcpt_scene_pose_save, mcpt_render_motion_aovs,
mcpt_temporal_accumulate_motion, mcpt_sequence_set_motion; include/mcpt.h).  Run on the MI355X box:
`pytest -m gpu`.  The inputs, the motion emulator and the CPU-side checks of both are tests/test_motion_cpu.py's.

  * the motion AOVs against node_point in numpy over the previous pose's arrays, from mcpt_primary_hits' (facet, beta,
    gamma), under the tight gates of conftest.py; bit for bit the AOVs' position and normal while the pose is unsaved
  * the accumulation against the emulator through test_temporal's check_outputs (test_temporal_clamp's check_clamped),
    plain and clamped, on the analytic frames with a rigid motion of the slab that keeps its history and one that
    loses a band of it
  * with motion arrays equal to the current guides: mcpt_temporal_accumulate[_clamped]'s outputs bit for bit
  * a plate moved 0.5 along its normal every frame keeps a history of 6 frames with motion and none without
  * the frame sequence with motion against the host pipeline, and the CLI's two paths against each other"""
import re
import subprocess

import numpy as np
import pytest

from conftest import TIGHT_L2, TIGHT_PX
import monte_carlo_path_tracing_amd as mcpt
from test_denoise import max_px_rel, read_pfm, rel_l2
from test_motion_cpu import (CLI, FRAMES, H, KEEP, LOSE, ORBIT, PLATE, SCENE_BASE, SIZES, SPP, W, considered, emulate_motion,
                             motion_camera, motion_case, motion_from_hits, plate_pose, veach_arrays)
from test_scene_update import STEP
from test_scene_update_cpu import fresh, translated
from test_sequence import read_bmp
from test_temporal import DEFAULTS, check_outputs
from test_temporal_clamp import CLAMP, check_clamped

pytestmark = pytest.mark.gpu
SEED = 20240430


def assert_tight(got, want, what):
    l2, px = rel_l2(got, want), max_px_rel(got, want)
    print("%s: rel L2 %.3e, max pixel %.3e" % (what, l2, px))
    assert l2 <= TIGHT_L2 and px <= TIGHT_PX, (what, l2, px)


# ---- 1. the motion AOVs ----

@pytest.mark.parametrize("ww,hh", [(32, 24), (33, 8), (1, 1)])
def test_motion_aovs(ww, hh):
    import torch
    arr = veach_arrays()
    scene, cam = fresh(arr), motion_camera(ww, hh)
    # no pose saved: the previous pose is the current one
    aov, mo = mcpt.render_aovs(scene, cam), mcpt.render_motion_aovs(scene, cam)
    assert np.array_equal(mo["prev_position"], aov["position"]) and np.array_equal(mo["prev_normal"], aov["normal"])
    assert (aov["depth"] > 0).any()
    # saved, then moved: node_point over the OLD arrays at the NEW hits
    new, nrm = translated(arr["positions"][PLATE[0]:PLATE[1]], STEP), -arr["normals"][PLATE[0]:PLATE[1]]
    scene.pose_save()
    scene.update(PLATE[0], new, nrm)
    mo = mcpt.render_motion_aovs(scene, cam)
    f, tbg = mcpt.primary_hits(scene, cam)
    want = motion_from_hits(f, tbg, arr, hh, ww)
    assert_tight(mo["prev_position"], want["prev_position"], "prev_position")
    assert_tight(mo["prev_normal"], want["prev_normal"], "prev_normal")
    on_plate = ((f >= PLATE[0]) & (f < PLATE[1])).reshape(hh, ww)
    aov = mcpt.render_aovs(scene, cam)
    if ww * hh > 1:
        assert on_plate.any() and (~on_plate & (aov["depth"] > 0)).any()
    assert np.allclose((aov["position"] - mo["prev_position"])[on_plate], STEP, rtol=0, atol=1e-5)  # float32 vertices of a few units
    assert np.allclose((aov["normal"] + mo["prev_normal"])[on_plate], 0.0, rtol=0, atol=1e-6)  # the update flipped the normals
    rest = ~on_plate
    assert np.array_equal(aov["position"][rest], mo["prev_position"][rest]) and np.array_equal(aov["normal"][rest], mo["prev_normal"][rest])
    # the device form, either pointer alone too
    dp, dn = (torch.full((hh, ww, 3), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    mcpt.render_motion_aovs_device(scene, cam, dp.data_ptr(), dn.data_ptr())
    assert np.array_equal(dp.cpu().numpy(), mo["prev_position"]) and np.array_equal(dn.cpu().numpy(), mo["prev_normal"])
    dn.fill_(7.0)
    torch.cuda.synchronize()
    mcpt.render_motion_aovs_device(scene, cam, None, dn.data_ptr())
    assert np.array_equal(dn.cpu().numpy(), mo["prev_normal"])
    with pytest.raises(mcpt.MCPTError, match="dev_out.prev_position"):
        mcpt.render_motion_aovs_device(scene, cam, mo["prev_position"].ctypes.data, dn.data_ptr())
    # a device state first created after the save and the update takes the previous pose from the host copy
    late = fresh(arr)
    late.pose_save()
    late.update(PLATE[0], new, nrm)
    mo2 = mcpt.render_motion_aovs(late, cam)
    assert np.array_equal(mo2["prev_position"], mo["prev_position"]) and np.array_equal(mo2["prev_normal"], mo["prev_normal"])
    # a second save without an update: the identity again
    scene.pose_save()
    mo = mcpt.render_motion_aovs(scene, cam)
    assert np.array_equal(mo["prev_position"], aov["position"]) and np.array_equal(mo["prev_normal"], aov["normal"])


# ---- 2. the accumulation against the emulator ----

@pytest.mark.parametrize("move", [KEEP, LOSE], ids=["keep", "lose"])
@pytest.mark.parametrize("clamped", [False, True], ids=["plain", "clamped"])
@pytest.mark.parametrize("ww,hh", SIZES)
def test_motion_accumulate_vs_emulator(ww, hh, clamped, move):
    prev, g1, color, mo, slab = motion_case(ww, hh, move)
    if not clamped:
        want = emulate_motion(color, g1, mo, prev[:4], **DEFAULTS)
        out, mom, var, sec = mcpt.temporal_accumulate_motion(color, g1, mo, prev[:4])
        check_outputs((out, mom, var), want)
        info = want[3]
    else:
        want = emulate_motion(color, g1, mo, prev, clamp=CLAMP, **DEFAULTS)
        out, mom, fast, var, shift, sec = mcpt.temporal_accumulate_motion(color, g1, mo, prev, clamp=True)
        check_clamped((out, mom, fast, var, shift), want, CLAMP["radius"])
        info = want[5]
    assert sec > 0
    print("slab: %d pixels, %d with history" % (slab.sum(), info["history"][slab].sum()))
    # without a previous state the motion arrays are not read
    out0, mom0, var0, _ = mcpt.temporal_accumulate_motion(color, g1, mo)
    ref0 = mcpt.temporal_accumulate(color, g1)
    assert np.array_equal(out0, ref0[0]) and np.array_equal(mom0, ref0[1]) and np.array_equal(var0, ref0[2])


# ---- 3. static identity ----

def test_motion_with_the_current_guides_is_the_plain_call_bit_for_bit():
    import torch
    scene = mcpt.Scene.load(SCENE_BASE + ".obj", SCENE_BASE + ".xml")
    cams = [mcpt.camera_orbit(mcpt.Camera.reference(W, H), k * ORBIT) for k in range(2)]
    imgs = [mcpt.render(scene, c, SPP, mode="mis", seed=SEED + k)[0] for k, c in enumerate(cams)]
    aovs = [mcpt.render_aovs(scene, c) for c in cams]
    same = dict(prev_position=aovs[1]["position"], prev_normal=aovs[1]["normal"])
    rendered = mcpt.render_motion_aovs(scene, cams[1])  # no pose saved
    assert np.array_equal(rendered["prev_position"], same["prev_position"]) and np.array_equal(rendered["prev_normal"], same["prev_normal"])
    c0, m0, _, _ = mcpt.temporal_accumulate(imgs[0], aovs[0])
    prev = (cams[0], aovs[0], c0, m0)
    want = mcpt.temporal_accumulate(imgs[1], aovs[1], prev)[:3]
    got = mcpt.temporal_accumulate_motion(imgs[1], aovs[1], same, prev)[:3]
    assert (want[1][..., 2] > 1.5).mean() > 0.5  # the orbit keeps most histories
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    c0, m0, f0, _, _, _ = mcpt.temporal_accumulate_clamped(imgs[0], aovs[0])
    prev = (cams[0], aovs[0], c0, m0, f0)
    want = mcpt.temporal_accumulate_clamped(imgs[1], aovs[1], prev)[:5]
    got = mcpt.temporal_accumulate_motion(imgs[1], aovs[1], same, prev, clamp=True)[:5]
    assert (want[4] != 0).any()  # the clamp moved something
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # the device form equals the host form
    t = lambda a: torch.from_numpy(np.array(a)).cuda()
    keys = ("albedo", "normal", "position", "depth")
    dg0, dg1 = ({k: t(a[k]) for k in keys} for a in aovs)
    dmo = {k: t(v) for k, v in same.items()}
    dimg, dc0, dm0, df0 = t(imgs[1]), t(c0), t(m0), t(f0)
    f64 = dict(dtype=torch.float64, device="cuda")
    do, dm, df, dv, ds = (torch.zeros(s, **f64) for s in ((H, W, 3), (H, W, 4), (H, W, 3), (H, W), (H, W)))
    torch.cuda.synchronize()
    ptrs = lambda d: {k: a.data_ptr() for k, a in d.items()}
    sec = mcpt.temporal_accumulate_motion_device(W, H, dimg.data_ptr(), ptrs(dg1), ptrs(dmo), do.data_ptr(), dm.data_ptr(), df.data_ptr(),
                                                 dv.data_ptr(), ds.data_ptr(), clamp=True,
                                                 prev=(cams[0], ptrs(dg0), dc0.data_ptr(), dm0.data_ptr(), df0.data_ptr()))
    assert sec > 0
    for a, b in zip((do, dm, df, dv, ds), got):
        assert np.array_equal(a.cpu().numpy(), b)


# ---- 4. history follows the object ----

_gpu = {}


def gpu_plate_sequence(orbit):
    """six 2-spp frames of the plate moved STEP_LENGTH along its normal per frame, pushed through a plain and a motion
    accumulator -> (n of the last frame, plain and motion; the plate's mask per frame)"""
    if orbit not in _gpu:
        arr = veach_arrays()
        scene = fresh(arr)
        plain, motion, masks = mcpt.TemporalAccumulator(), mcpt.TemporalAccumulator(), []
        for k in range(FRAMES):
            scene.pose_save()
            if k:
                scene.update(PLATE[0], plate_pose(arr, k))
            cam = mcpt.camera_orbit(motion_camera(), k * orbit)
            img = mcpt.render(scene, cam, SPP, mode="mis", seed=SEED + k)[0]
            aov, mo = mcpt.render_aovs(scene, cam), mcpt.render_motion_aovs(scene, cam)
            plain.push(cam, img, aov)
            motion.push(cam, img, aov, motion=mo)
            f, _ = mcpt.primary_hits(scene, cam)
            masks.append(((f >= PLATE[0]) & (f < PLATE[1])).reshape(H, W))
        _gpu[orbit] = (plain.moments[..., 2], motion.moments[..., 2], masks)
    return _gpu[orbit]


def test_history_follows_the_moved_plate():
    """Fails without motion vectors: the plate is 0.5 further along its normal every frame, more than plane_max * depth =
    0.02 * 17, so the plain rule's plane test fails on it in every frame."""
    n_plain, n_motion, masks = gpu_plate_sequence(0.0)
    px = considered(masks[-2:])
    print("%d pixels at least 2 px inside the plate in the last two frames; plain n in [%g, %g], motion n in [%g, %g]"
          % (px.sum(), n_plain[px].min(), n_plain[px].max(), n_motion[px].min(), n_motion[px].max()))
    assert px.sum() >= 40
    assert np.all(n_motion[px] >= 5)
    assert np.all(n_plain[px] == 1)
    # 2 px and more away from the plate in every frame both arms carry the same history
    far = considered([~np.logical_or.reduce(masks)])
    assert far.any() and np.array_equal(n_plain[far], n_motion[far])


def test_history_follows_the_moved_plate_under_an_orbit():
    n_plain, n_motion, masks = gpu_plate_sequence(ORBIT)
    px = considered(masks[-2:])
    better = (n_motion[px] > n_plain[px]).mean()
    print("%d pixels considered, the motion arm's history is longer on %.1f %% of them" % (px.sum(), 100.0 * better))
    assert px.sum() >= 40 and better >= 0.9


# ---- 5. the sequence ----

@pytest.mark.parametrize("clamp", [False, True], ids=["plain", "clamp"])
def test_sequence_with_motion_vs_host_pipeline(clamp):
    arr = veach_arrays()
    scene = fresh(arr)
    seq = mcpt.FrameSequence(scene, W, H, SPP, mode="mis", denoise=False, clamp=True if clamp else None, motion=True)
    with pytest.raises(mcpt.MCPTError, match="holds no frame"):
        seq.motion_info()
    acc = mcpt.TemporalAccumulator(clamp=True if clamp else None)
    kept = []
    for k in range(4):
        scene.pose_save()  # the caller's: the sequence never saves the pose
        if k:
            scene.update(PLATE[0], plate_pose(arr, k))
        cam = mcpt.camera_orbit(motion_camera(), k * ORBIT)
        seq.frame(cam, SEED + k)
        got = {n: seq.read(n) for n in ["raw", "accumulated", "moments", "variance", "prev_position", "prev_normal"] + (["fast", "shift"] if clamp else [])}
        assert seq.motion_info() > 0 and 0.0 < seq.info.aov_seconds < 10.0
        img = mcpt.render(scene, cam, SPP, mode="mis", seed=SEED + k)[0]
        assert_tight(got["raw"], img, "frame %d raw" % k)
        aov, mo = mcpt.render_aovs(scene, cam), mcpt.render_motion_aovs(scene, cam)
        assert_tight(got["prev_position"], mo["prev_position"], "frame %d prev_position" % k)
        assert_tight(got["prev_normal"], mo["prev_normal"], "frame %d prev_normal" % k)
        c, v = acc.push(cam, got["raw"], aov, motion=mo)  # the same kernels on the same inputs
        assert_tight(got["accumulated"], c, "frame %d accumulated" % k)
        assert np.allclose(got["moments"], acc.moments, rtol=1e-6, atol=0) and np.allclose(got["variance"], v, rtol=1e-6, atol=1e-300)
        if clamp:
            assert_tight(got["fast"], acc.fast, "frame %d fast" % k)
            assert np.allclose(got["shift"], acc.shift, rtol=1e-6, atol=1e-300)
        f, _ = mcpt.primary_hits(scene, cam)
        on_plate = ((f >= PLATE[0]) & (f < PLATE[1])).reshape(H, W)
        kept.append((got["moments"][..., 2] > 1.5)[on_plate].mean())
    print("share of the plate's pixels with a history, per frame:", kept)
    assert kept[0] == 0 and min(kept[1:]) > 0.5
    # switched off: the selectors and the info are refused, the next frame restarts the plate
    seq.set_motion(False)
    with pytest.raises(mcpt.MCPTError, match="motion is off"):
        seq.read("prev_position")
    with pytest.raises(mcpt.MCPTError, match="motion is off"):
        seq.device_buffer("prev_normal")
    scene.update(PLATE[0], plate_pose(arr, 4))
    seq.frame(mcpt.camera_orbit(motion_camera(), 4 * ORBIT), SEED + 4)
    with pytest.raises(mcpt.MCPTError, match="without motion"):
        seq.motion_info()
    f, _ = mcpt.primary_hits(scene, mcpt.camera_orbit(motion_camera(), 4 * ORBIT))
    inside = considered([((f >= PLATE[0]) & (f < PLATE[1])).reshape(H, W)])
    assert inside.any() and np.all(seq.read("moments")[..., 2][inside] == 1)
    seq.close()


def test_upsampled_sequences_refuse_motion():
    scene = mcpt.Scene.load(SCENE_BASE + ".obj", SCENE_BASE + ".xml")
    for kw, name in ((dict(upsample=2), "mcpt_sequence_create_upsampled"),
                     (dict(upsample=2, temporal_upsample=True), "mcpt_sequence_create_temporal_upsampled")):
        with pytest.raises(mcpt.MCPTError, match="not supported in a sequence created by %s" % name):
            mcpt.FrameSequence(scene, 16, 12, 1, denoise=False, motion=True, **kw)
        seq = mcpt.FrameSequence(scene, 16, 12, 1, denoise=False, **kw)
        with pytest.raises(mcpt.MCPTError, match="not supported"):
            seq.set_motion(True)
        with pytest.raises(mcpt.MCPTError):
            seq.set_motion(False)
        seq.close()


def test_motion_on_a_scene_that_never_moved_shows_the_same_frames():
    scene = mcpt.Scene.load(SCENE_BASE + ".obj", SCENE_BASE + ".xml")
    shown = {}
    for motion in (False, True):
        seq = mcpt.FrameSequence(scene, W, H, SPP, mode="mis", denoise=True, clamp=True, motion=motion)
        shown[motion] = []
        for k in range(3):
            if motion and k == 2:
                scene.pose_save()  # a save without an update changes nothing
            shown[motion].append(seq.frame(mcpt.camera_orbit(mcpt.Camera.reference(W, H), k * ORBIT), SEED + k))
        seq.close()
    for a, b in zip(shown[False], shown[True]):
        assert np.array_equal(a, b)
    assert not np.array_equal(shown[True][0], shown[True][2])


# ---- 6. the CLI ----

def test_cli_motion_on_both_paths(tmp_path):
    def run(tag, *extra):
        r = subprocess.run([CLI, "--scene", SCENE_BASE, "--out", str(tmp_path / (tag + ".bmp")), "--hdr", str(tmp_path / (tag + ".pfm")),
                            "--width", str(W), "--height", str(H), "--spp", str(SPP), "--frames", "3", "--move", "36:12:0.6,1.4,0",
                            *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        kept = [float(re.search(r"([0-9.]+)% of the pixels kept", ln).group(1)) for ln in r.stdout.splitlines() if ln.startswith("frame ")]
        assert len(kept) == 3 and r.stdout.count("moved facets [36, 48)") == 2, r.stdout
        return kept, [str(tmp_path / ("%s_%04d" % (tag, k))) for k in range(3)]

    k_host, host = run("host", "--motion")
    k_dev, dev = run("dev", "--motion", "--device-sequence")
    _, off = run("off")
    assert k_host == k_dev
    # from this camera the plate shows mostly its front face, in whose plane the move nearly lies: without motion its
    # pixels pass the plane test and gather another surface point's history, with motion their own
    assert np.allclose(read_pfm(host[0] + ".pfm"), read_pfm(off[0] + ".pfm"), rtol=1e-6, atol=1e-30)
    assert rel_l2(read_pfm(host[2] + ".pfm"), read_pfm(off[2] + ".pfm")) > 1e-4
    for a, b in zip(host, dev):
        # both runs rendered anew: equal up to the framebuffer's summation order, far below float32 and a grey level
        assert np.allclose(read_pfm(a + ".pfm"), read_pfm(b + ".pfm"), rtol=1e-6, atol=1e-30)
        x, y = read_bmp(a + ".bmp").astype(int), read_bmp(b + ".bmp").astype(int)
        assert np.abs(x - y).max() <= 1 and (x != y).mean() <= 1e-3
