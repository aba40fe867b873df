"""Anti-lag by temporal gradients on the GPU (mcpt_gradient_rays, mcpt_temporal_gradient,
mcpt_temporal_accumulate_antilag, mcpt_sequence_set_antilag; include/mcpt.h).  Run on the MI355X box:
`pytest -m gpu`.  The emulators, the inputs and the CPU-side checks of both are tests/test_antilag_cpu.py's.

  * the gradient rays against camera_rays, bit for bit, and exact zeros off the selected pixels
  * the gradient against emulate_gradient: the same fp64 operations in the same order, so 1e-14 absolute
  * the accumulation against emulate_antilag through test_temporal's check_outputs (test_temporal_clamp's
    check_clamped): plain, clamped and both motion forms
  * with Lambda == 0 the plain, clamped and motion calls' outputs bit for bit, host and device forms
  * rendered: an unedited scene gives Lambda at the renders' own run-to-run noise, a scene whose every radiance was
    doubled Lambda = 1 / 2
  * the frame sequence with anti-lag against the host pipeline across a re-light and a moved plate, its switching and
    refusals, the dimmed-light scenario's error, and the CLI's two paths against each other"""
import gc
import re
import subprocess

import numpy as np
import pytest

from conftest import TIGHT_L2, TIGHT_PX
import monte_carlo_path_tracing_amd as mcpt
from test_antilag_cpu import (CLI, QDIM, QEDIT, QFRAMES, QH, QREF_SEED, QREF_SPP, QSPP, QW, SCENE_BASE, SEED, emulate_antilag,
                              emulate_gradient, gradient_inputs, grid_shape, random_lambda, rel_l2 as q_rel_l2, run_scenario)
from test_denoise import max_px_rel, read_pfm, rel_l2
from test_motion_cpu import KEEP, LOSE, PLATE, SIZES, motion_camera, motion_case, plate_pose, veach_arrays
from test_scene_update_cpu import fresh
from test_sequence import read_bmp
from test_temporal import DEFAULTS, analytic_inputs, check_outputs
from test_temporal_clamp import CLAMP, check_clamped

pytestmark = pytest.mark.gpu
W, H, SPP = 16, 12, 4
KEYS = ("albedo", "normal", "position", "depth")


def assert_tight(got, want, what):
    l2, px = rel_l2(got, want), max_px_rel(got, want)
    print("%s: rel L2 %.3e, max pixel %.3e" % (what, l2, px))
    assert l2 <= TIGHT_L2 and px <= TIGHT_PX, (what, l2, px)


def selected(hh, ww, s, a, b):
    sel = np.zeros((hh, ww), bool)
    sel[a::s, b::s] = True
    return sel


def big_light_group(scene, arr):
    """the group of light_big: the lights of radiance 10"""
    return int(scene.light_groups()[np.flatnonzero(np.all(arr["light_radiance"] == 10.0, -1))[0]])


# ---- 1. the gradient rays ----

@pytest.mark.parametrize("ww,hh", [(16, 12), (1, 1), (5, 3), (65, 3)])
def test_gradient_rays_are_the_camera_rays_at_the_selected_pixels(ww, hh):
    cam = mcpt.camera_orbit(mcpt.Camera.reference(ww, hh), 3.0)
    o, d = mcpt.camera_rays(cam, jitter=False)
    assert np.all(np.abs(np.linalg.norm(d, axis=1) - 1.0) < 1e-12)
    for s in (1, 2, 3):
        for a in range(s):
            for b in range(s):
                go, gd = mcpt.gradient_rays(cam, s, a, b)
                sel = selected(hh, ww, s, a, b).reshape(-1)
                assert np.array_equal(go, o)
                assert np.array_equal(gd[sel], d[sel]) and np.all(gd[~sel] == 0.0)


def test_gradient_rays_device_form_writes_its_arrays_only():
    import torch
    cam = mcpt.Camera.reference(65, 3)
    n, pad = 65 * 3 * 3, 64
    bo, bd = (torch.full((n + 2 * pad,), 7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    torch.cuda.synchronize()
    assert mcpt.lib().mcpt_gradient_rays_device(cam, 3, 1, 2, -1, bo.data_ptr() + 8 * pad, bd.data_ptr() + 8 * pad) == 0
    go, gd = mcpt.gradient_rays(cam, 3, 1, 2)
    ho, hd = bo.cpu().numpy(), bd.cpu().numpy()
    assert np.array_equal(ho[pad:-pad].reshape(-1, 3), go) and np.array_equal(hd[pad:-pad].reshape(-1, 3), gd)
    for h in (ho, hd):
        assert np.all(h[:pad] == 7.0) and np.all(h[-pad:] == 7.0)
    rc = mcpt.lib().mcpt_gradient_rays_device(cam, 3, 1, 2, -1, go.ctypes.data, bd.data_ptr())
    assert rc == -1 and "dev_origin" in mcpt.lib().mcpt_last_error().decode()


# ---- 2. the gradient against the emulator ----

@pytest.mark.parametrize("ww,hh", [(1, 1), (5, 3), (2, 70), (65, 5), (32, 24)])
def test_temporal_gradient_vs_emulator(ww, hh):
    prev, re_ = gradient_inputs(hh, ww, 7 * ww + hh)
    worst = 0.0
    for s in (1, 2, 3, 8):
        for r in (0, 1, 3):
            for a, b in {(0, 0), (s - 1, s - 1), (s // 2, 0), (0, s - 1)}:
                for scale in (1.0, 2.5):
                    want, den = emulate_gradient(prev, re_, a, b, s, r, scale)
                    got, sec = mcpt.temporal_gradient(prev, re_, a, b, stratum=s, radius=r, scale=scale)
                    assert got.shape == want.shape == grid_shape(hh, ww, s) and sec > 0
                    worst = max(worst, float(np.abs(got - want).max()))
                    assert np.all(got[den == 0] == 0.0) and np.all((got >= 0) & (got <= 1))
    print("%d x %d: max |Lambda - emulator| %.3e" % (ww, hh, worst))
    assert worst <= 1e-14


def test_temporal_gradient_device_form_equals_host_form():
    import torch
    ww, hh, s, pad = 65, 5, 3, 64
    prev, re_ = gradient_inputs(hh, ww, 3)
    want, _ = mcpt.temporal_gradient(prev, re_, 2, 1, stratum=s, radius=1)
    dp, dr = torch.from_numpy(prev).cuda(), torch.from_numpy(re_).cuda()
    buf = torch.full((want.size + 2 * pad,), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    g = mcpt._gradient_opts(s, 1)
    sec = mcpt.C.c_double()
    rc = mcpt.lib().mcpt_temporal_gradient_device(g, ww, hh, 2, 1, dp.data_ptr(), dr.data_ptr(), buf.data_ptr() + 8 * pad, sec)
    assert rc == 0 and sec.value > 0, mcpt.lib().mcpt_last_error()
    h = buf.cpu().numpy()
    assert np.array_equal(h[pad:-pad].reshape(want.shape), want) and np.all(h[:pad] == 7.0) and np.all(h[-pad:] == 7.0)
    assert np.array_equal(dp.cpu().numpy(), prev) and np.array_equal(dr.cpu().numpy(), re_)
    rc = mcpt.lib().mcpt_temporal_gradient_device(g, ww, hh, 2, 1, prev.ctypes.data, dr.data_ptr(), buf.data_ptr(), None)
    assert rc == -1 and "dev_prev_raw" in mcpt.lib().mcpt_last_error().decode()


# ---- 3. the accumulation against the emulator ----

@pytest.mark.parametrize("move", [KEEP, LOSE], ids=["keep", "lose"])
@pytest.mark.parametrize("variant", ["plain", "clamped", "motion", "motion-clamped"])
@pytest.mark.parametrize("ww,hh", SIZES)
def test_antilag_accumulate_vs_emulator(ww, hh, variant, move):
    """SIZES' (37, 29) is test_temporal.analytic_inputs' own arrays (motion_case)"""
    prev, g1, color, mo, _ = motion_case(ww, hh, move)
    if (ww, hh) == (37, 29):
        assert color is analytic_inputs()[6]
    clamped, motion = "clamped" in variant, mo if "motion" in variant else None
    for s in (1, 3):
        lam = random_lambda(hh, ww, s, 100 * ww + hh + s)
        if not clamped:
            want = emulate_antilag(color, g1, lam, s, prev[:4], motion=motion, **DEFAULTS)
            out, mom, var, sec = mcpt.temporal_accumulate_antilag(color, g1, lam, prev[:4], motion=motion, stratum=s)
            check_outputs((out, mom, var), want)
        else:
            want = emulate_antilag(color, g1, lam, s, prev, motion=motion, clamp=CLAMP, **DEFAULTS)
            out, mom, fast, var, shift, sec = mcpt.temporal_accumulate_antilag(color, g1, lam, prev, motion=motion, clamp=True, stratum=s)
            check_clamped((out, mom, fast, var, shift), want, CLAMP["radius"])
        assert sec > 0
    # without a previous state Lambda is not read
    out0, mom0, var0, _ = mcpt.temporal_accumulate_antilag(color, g1, lam, stratum=s)
    ref0 = mcpt.temporal_accumulate(color, g1)
    assert np.array_equal(out0, ref0[0]) and np.array_equal(mom0, ref0[1]) and np.array_equal(var0, ref0[2])


# ---- 4. Lambda == 0 is the existing calls, and the device forms ----

def test_antilag_with_a_zero_lambda_is_the_existing_calls_bit_for_bit():
    import torch
    ww, hh = 37, 29
    prev, g1, color, mo, _ = motion_case(ww, hh, LOSE)
    t = lambda a: torch.from_numpy(np.array(a)).cuda()
    ptrs = lambda d: {k: a.data_ptr() for k, a in d.items()}
    dg0, dg1, dmo = {k: t(prev[1][k]) for k in KEYS}, {k: t(g1[k]) for k in KEYS}, {k: t(v) for k, v in mo.items()}
    dimg, dc0, dm0, df0 = t(color), t(prev[2]), t(prev[3]), t(prev[4])
    f64 = dict(dtype=torch.float64, device="cuda")
    pad = 64
    for s in (1, 3, 8):
        zero = np.zeros(grid_shape(hh, ww, s))
        dlam = t(zero)
        for motion in (None, mo):
            # plain
            want = (mcpt.temporal_accumulate(color, g1, prev[:4]) if motion is None else mcpt.temporal_accumulate_motion(color, g1, mo, prev[:4]))[:3]
            got = mcpt.temporal_accumulate_antilag(color, g1, zero, prev[:4], motion=motion, stratum=s)[:3]
            assert (want[1][..., 2] > 1.5).mean() > 0.3
            for a, b in zip(got, want):
                assert np.array_equal(a, b)
            # clamped
            wantc = (mcpt.temporal_accumulate_clamped(color, g1, prev) if motion is None
                     else mcpt.temporal_accumulate_motion(color, g1, mo, prev, clamp=True))[:5]
            gotc = mcpt.temporal_accumulate_antilag(color, g1, zero, prev, motion=motion, clamp=True, stratum=s)[:5]
            assert (wantc[4] != 0).any()
            for a, b in zip(gotc, wantc):
                assert np.array_equal(a, b)
            # the device form: the same bits, and nothing outside its arrays
            sizes = [hh * ww * 3, hh * ww * 4, hh * ww * 3, hh * ww, hh * ww]  # colour, moments, fast, variance, shift
            bufs = [torch.full((n + 2 * pad,), 7.0, **f64) for n in sizes]
            torch.cuda.synchronize()
            p = [b.data_ptr() + 8 * pad for b in bufs]
            sec = mcpt.temporal_accumulate_antilag_device(
                ww, hh, dimg.data_ptr(), ptrs(dg1), dlam.data_ptr(), p[0], p[1], p[2], p[3], p[4], clamp=True, stratum=s,
                motion_ptrs=None if motion is None else ptrs(dmo), prev=(prev[0], ptrs(dg0), dc0.data_ptr(), dm0.data_ptr(), df0.data_ptr()))
            assert sec > 0
            for b, n, w in zip(bufs, sizes, (wantc[0], wantc[1], wantc[2], wantc[3], wantc[4])):
                h = b.cpu().numpy()
                assert np.array_equal(h[pad:-pad], w.reshape(-1)) and np.all(h[:pad] == 7.0) and np.all(h[-pad:] == 7.0)
            bufs = [torch.full((n + 2 * pad,), 7.0, **f64) for n in sizes]
            torch.cuda.synchronize()
            p = [b.data_ptr() + 8 * pad for b in bufs]
            mcpt.temporal_accumulate_antilag_device(ww, hh, dimg.data_ptr(), ptrs(dg1), dlam.data_ptr(), p[0], p[1], None, p[3], None, stratum=s,
                                                    motion_ptrs=None if motion is None else ptrs(dmo),
                                                    prev=(prev[0], ptrs(dg0), dc0.data_ptr(), dm0.data_ptr()))
            for b, w in zip((bufs[0], bufs[1], bufs[3]), want):
                assert np.array_equal(b.cpu().numpy()[pad:-pad], w.reshape(-1))
            assert np.all(bufs[2].cpu().numpy() == 7.0) and np.all(bufs[4].cpu().numpy() == 7.0)


def test_antilag_device_form_equals_host_form_with_a_random_lambda():
    import torch
    ww, hh, s = 37, 29, 3
    prev, g1, color, mo, _ = motion_case(ww, hh, KEEP)
    lam = random_lambda(hh, ww, s, 5)
    want = mcpt.temporal_accumulate_antilag(color, g1, lam, prev, motion=mo, clamp=True, stratum=s)[:5]
    plain = mcpt.temporal_accumulate_motion(color, g1, mo, prev, clamp=True)[:5]
    assert not np.array_equal(want[0], plain[0]) and not np.array_equal(want[1][..., 2], plain[1][..., 2])
    t = lambda a: torch.from_numpy(np.array(a)).cuda()
    ptrs = lambda d: {k: a.data_ptr() for k, a in d.items()}
    dg0, dg1, dmo = {k: t(prev[1][k]) for k in KEYS}, {k: t(g1[k]) for k in KEYS}, {k: t(v) for k, v in mo.items()}
    dimg, dc0, dm0, df0, dlam = t(color), t(prev[2]), t(prev[3]), t(prev[4]), t(lam)
    f64 = dict(dtype=torch.float64, device="cuda")
    do, dm, df, dv, ds = (torch.zeros(sh, **f64) for sh in ((hh, ww, 3), (hh, ww, 4), (hh, ww, 3), (hh, ww), (hh, ww)))
    torch.cuda.synchronize()
    mcpt.temporal_accumulate_antilag_device(ww, hh, dimg.data_ptr(), ptrs(dg1), dlam.data_ptr(), do.data_ptr(), dm.data_ptr(), df.data_ptr(),
                                            dv.data_ptr(), ds.data_ptr(), clamp=True, stratum=s, motion_ptrs=ptrs(dmo),
                                            prev=(prev[0], ptrs(dg0), dc0.data_ptr(), dm0.data_ptr(), df0.data_ptr()))
    for a, b in zip((do, dm, df, dv, ds), want):
        assert np.array_equal(a.cpu().numpy(), b)
    assert np.array_equal(dlam.cpu().numpy(), lam)
    with pytest.raises(mcpt.MCPTError, match="dev_lambda"):
        mcpt.temporal_accumulate_antilag_device(ww, hh, dimg.data_ptr(), ptrs(dg1), lam.ctypes.data, do.data_ptr(), dm.data_ptr(), stratum=s)


# ---- 5. rendered ----

@pytest.mark.parametrize("mode", ["mis", "brdf"])
def test_rendered_gradient_is_zero_unedited_and_a_half_after_doubling(mode):
    """The gradient compares render with render_rays, which tests/test_rays.py gates at TIGHT_PX per pixel (||d|| <=
    TIGHT_PX ||c||); sum_c |d_c| <= sqrt 3 ||d|| and sum_c max_c >= ||c||_inf >= ||c|| / sqrt 3, so a stratum's ratio -- and
    a window's, a ratio of sums -- is at most 3 TIGHT_PX.  A scale of every radiance by 2 is exact through the whole
    chain (test_doubling_every_radiance_doubles_the_frame), so regrad = 2 prev up to the same noise and
    Lambda = |2 c - c| / max(2 c, c) = 1 / 2."""
    arr = veach_arrays()
    scene, cam = fresh(arr), mcpt.Camera.reference(W, H)
    prev_raw = mcpt.render(scene, cam, SPP, mode=mode, seed=SEED)[0]
    assert (prev_raw.sum(-1) > 0).sum() >= 10  # BRDF sampling at 4 spp finds a light from few pixels
    for doubled in (False, True):
        if doubled:
            scene.set_light_radiance(0, 2.0 * arr["light_radiance"])
        for s, r in ((3, 1), (1, 0), (2, 3)):
            a, b = mcpt.gradient_phase(s, 4)
            o, d = mcpt.gradient_rays(cam, s, a, b)
            regrad = mcpt.render_rays(scene, o, d, SPP, mode=mode, seed=SEED)[0].reshape(H, W, 3)
            assert np.all(regrad[~selected(H, W, s, a, b)] == 0.0)
            lam, _ = mcpt.temporal_gradient(prev_raw, regrad, a, b, stratum=s, radius=r)
            _, den = emulate_gradient(prev_raw, regrad, a, b, s, r)
            assert (den > 0).any()
            if not doubled:
                print("%s, stratum %d radius %d: max Lambda %.3e" % (mode, s, r, lam.max()))
                assert lam.max() <= 3 * TIGHT_PX
            else:
                dev = np.abs(lam - 0.5)[den > 0].max()
                print("%s doubled, stratum %d radius %d: max |Lambda - 1/2| %.3e" % (mode, s, r, dev))
                assert dev <= 1e-5 and np.all(lam[den == 0] == 0.0)


# ---- 6. the sequence ----

@pytest.mark.parametrize("clamp", [False, True], ids=["plain", "clamp"])
def test_sequence_with_antilag_vs_host_pipeline(clamp):
    """eight frames with motion on, a dimmed light group before frame 4 and a moved plate before frame 6.  The sequence's
    stages are the host calls' kernels: fed the sequence's own raw frames they give its Lambda and its accumulated frame
    bit for bit or within the tight gates; fed independent renders, Lambda agrees within 6 TIGHT_PX: with e = TIGHT_PX
    each of the two frames is within e ||c|| per pixel, and a sample pixel's den = sum_c max(g_c, p_c) >= max(||g||, ||p||)
    (non-negative radiance), so Num moves by at most sum_c (|dg_c| + |dp_c|) <= sqrt 3 e (||g|| + ||p||) <= 2 sqrt 3 e den and
    Den by at most sum_c max(|dg_c|, |dp_c|) <= sqrt 3 e den; Lambda = Num / Den <= 1 then moves by at most
    (2 sqrt 3 + sqrt 3) e = 5.2 e to first order."""
    arr = veach_arrays()
    scene = fresh(arr)
    s = 3
    seq = mcpt.FrameSequence(scene, W, H, SPP, mode="mis", denoise=False, clamp=True if clamp else None, motion=True, antilag=True)
    with pytest.raises(mcpt.MCPTError, match="holds no frame"):
        seq.antilag_info()
    acc = mcpt.TemporalAccumulator(clamp=True if clamp else None)
    group = big_light_group(scene, arr)
    prev_raw = prev_cam = prev_img = None
    peaks = []
    for k in range(8):
        scene.pose_save()
        if k == 4:
            scene.set_group_radiance(group, (1.0, 1.0, 1.0))
        if k == 6:
            scene.update(PLATE[0], plate_pose(arr, 1))
        cam = mcpt.camera_orbit(motion_camera(W, H), 0.5 * k)
        seq.frame(cam, SEED + k)
        names = ["raw", "accumulated", "moments", "variance", "gradient_lambda"] + (["fast", "shift"] if clamp else [])
        got = {n: seq.read(n) for n in names}
        info = seq.antilag_info()
        assert info["ran"] == (k > 0) and info["phase"] == mcpt.gradient_phase(s, k)
        assert all(np.isfinite(info[t]) and 0 <= info[t] < 10.0 for t in ("trace_seconds", "kernel_seconds"))
        assert got["gradient_lambda"].shape == grid_shape(H, W, s)
        assert info["lambda_max"] == got["gradient_lambda"].max() and abs(info["lambda_mean"] - got["gradient_lambda"].mean()) <= 1e-12
        img = mcpt.render(scene, cam, SPP, mode="mis", seed=SEED + k)[0]
        assert_tight(got["raw"], img, "frame %d raw" % k)
        aov, mo = mcpt.render_aovs(scene, cam), mcpt.render_motion_aovs(scene, cam)
        if k == 0:
            assert np.all(got["gradient_lambda"] == 0.0)
            with pytest.raises(mcpt.MCPTError, match="did not run"):
                seq.read("gradient_raw")
            assert info["trace_seconds"] == 0.0
        else:
            a, b = info["phase"]
            sel = selected(H, W, s, a, b)
            graw = seq.read("gradient_raw")
            # the previous camera and seed in the current scene: the whole frame's render at the selected pixels
            again = mcpt.render(scene, prev_cam, SPP, mode="mis", seed=SEED + k - 1)[0]
            assert np.all(graw[~sel] == 0.0)
            assert_tight(graw, np.where(sel[..., None], again, 0.0), "frame %d gradient_raw" % k)
            o, d = mcpt.gradient_rays(prev_cam, s, a, b)
            rr = mcpt.render_rays(scene, o, d, SPP, mode="mis", seed=SEED + k - 1)[0].reshape(H, W, 3)
            assert_tight(graw, rr, "frame %d gradient_raw vs render_rays" % k)
            lam_own, _ = mcpt.temporal_gradient(prev_raw, graw, a, b, stratum=s)
            assert np.array_equal(got["gradient_lambda"], lam_own)  # the same kernel on the same inputs
            lam_host, _ = mcpt.temporal_gradient(prev_img, rr, a, b, stratum=s)
            dl = np.abs(got["gradient_lambda"] - lam_host).max()
            print("frame %d: Lambda max %.4f, |Lambda - host pipeline's| %.3e" % (k, got["gradient_lambda"].max(), dl))
            assert dl <= 6 * TIGHT_PX
            assert info["trace_seconds"] > 0
        peaks.append(float(got["gradient_lambda"].max()))
        c, v = acc.push(cam, got["raw"], aov, motion=mo, lam=got["gradient_lambda"], stratum=s)
        assert_tight(got["accumulated"], c, "frame %d accumulated" % k)
        assert np.allclose(got["moments"], acc.moments, rtol=1e-6, atol=0) and np.allclose(got["variance"], v, rtol=1e-6, atol=1e-300)
        if clamp:
            assert_tight(got["fast"], acc.fast, "frame %d fast" % k)
            assert np.allclose(got["shift"], acc.shift, rtol=1e-6, atol=1e-300)
        prev_raw, prev_cam, prev_img = got["raw"], cam, img
    print("Lambda's maximum per frame:", peaks)
    quiet = [peaks[k] for k in (1, 2, 3, 5, 7)]
    # the edits show three orders above the noise (how far above depends on the view; the quality test measures that)
    assert max(quiet) <= 3 * TIGHT_PX and peaks[4] > 1e-3 and peaks[6] > 1e-3
    seq.close()


def test_antilag_drops_the_stale_history_on_the_gpu():
    """the dimmed-light scenario of tests/test_antilag_cpu.py with the GPU's renders: the first frame after the edit is
    more than twice as close to the dimmed scene's reference as the plain accumulation"""
    arr = veach_arrays()
    scene, cam = fresh(arr), mcpt.Camera.reference(QW, QH)
    group = big_light_group(scene, arr)
    guides = mcpt.render_aovs(scene, cam)
    state = {"dimmed": False}

    def at(k):
        if k >= QEDIT and not state["dimmed"]:
            scene.set_group_radiance(group, (10.0 * QDIM,) * 3)
            state["dimmed"] = True

    def render(k):
        at(k)
        return mcpt.render(scene, cam, QSPP, mode="mis", seed=SEED + k)[0]

    def again(k):
        at(k)
        a, b = mcpt.gradient_phase(3, k)
        o, d = mcpt.gradient_rays(cam, 3, a, b)
        return mcpt.render_rays(scene, o, d, QSPP, mode="mis", seed=SEED + k - 1)[0].reshape(QH, QW, 3)

    frames = run_scenario(render, again, guides)  # it renders frame k before it asks for frame k - 1's samples again
    ref = mcpt.render(scene, cam, QREF_SPP, mode="mis", seed=QREF_SEED)[0]
    for k in range(QEDIT, QFRAMES):
        raw, plain, anti, lam = frames[k]
        print("frame %d: raw %.3f, plain %.3f, anti-lag %.3f; Lambda max %.3e"
              % (k, q_rel_l2(raw, ref), q_rel_l2(plain, ref), q_rel_l2(anti, ref), lam.max()))
    for k in range(QFRAMES):
        if k != QEDIT:
            assert frames[k][3].max() <= 3 * TIGHT_PX
    e_plain, e_anti = q_rel_l2(frames[QEDIT][1], ref), q_rel_l2(frames[QEDIT][2], ref)
    assert e_anti < e_plain / 2, (e_anti, e_plain)


def test_antilag_switching_and_refusals():
    scene = mcpt.Scene.load(SCENE_BASE + ".obj", SCENE_BASE + ".xml")
    cams = [mcpt.camera_orbit(mcpt.Camera.reference(W, H), 0.5 * k) for k in range(6)]
    never = mcpt.FrameSequence(scene, W, H, SPP, mode="mis", denoise=True, clamp=True)
    shown = [never.frame(c, SEED + k) for k, c in enumerate(cams)]
    never.close()
    seq = mcpt.FrameSequence(scene, W, H, SPP, mode="mis", denoise=True, clamp=True)
    for name in ("gradient_lambda", "gradient_raw"):
        with pytest.raises(mcpt.MCPTError, match="anti-lag is off"):
            seq.read(name)
    got = [seq.frame(cams[0], SEED)]
    with pytest.raises(mcpt.MCPTError, match="without anti-lag"):
        seq.antilag_info()
    seq.set_antilag(dict(stratum=2, radius=0))
    with pytest.raises(mcpt.MCPTError, match="before anti-lag was switched on"):
        seq.read("gradient_lambda")
    got.append(seq.frame(cams[1], SEED + 1))  # the first frame after the switch: nothing was kept, the plain rule
    assert seq.antilag_info()["ran"] is False and np.all(seq.read("gradient_lambda") == 0.0)
    assert seq.read("gradient_lambda").shape == grid_shape(H, W, 2)
    got.append(seq.frame(cams[2], SEED + 2))
    info = seq.antilag_info()
    assert info["ran"] is True and info["phase"] == mcpt.gradient_phase(2, 2) and info["lambda_max"] <= 3 * TIGHT_PX
    assert seq.read("gradient_raw").shape == (H, W, 3)
    seq.set_antilag(dict(stratum=3))  # the last frame's map keeps the shape of the stratum it ran with
    assert seq.read("gradient_lambda").shape == grid_shape(H, W, 2)
    seq.reset()  # drops the kept frame with the history
    seq.frame(cams[2], SEED + 2)
    assert seq.antilag_info()["ran"] is False and seq.info.frame_index == 0
    seq.set_antilag(None)
    with pytest.raises(mcpt.MCPTError, match="anti-lag is off"):
        seq.device_buffer("gradient_lambda")
    seq.close()
    # an unedited scene: Lambda is the renders' run-to-run noise, far below a grey level, and off again the frames are
    # those of a sequence that never had it
    for a, b in zip(got, shown):
        assert np.abs(a.astype(int) - b.astype(int)).max() <= 1
    seq = mcpt.FrameSequence(scene, W, H, SPP, mode="mis", denoise=False, clamp=True, antilag=True)
    plain = mcpt.FrameSequence(scene, W, H, SPP, mode="mis", denoise=False, clamp=True)
    for k in range(5):
        if k == 2:
            seq.set_antilag(False)
        if k == 4:
            seq.set_antilag(True)  # on again: the frame before kept nothing
        seq.frame(cams[k], SEED + k, readback=False)
        plain.frame(cams[k], SEED + k, readback=False)
        if k >= 2:
            for name in ("accumulated", "fast"):
                assert_tight(seq.read(name), plain.read(name), "frame %d %s" % (k, name))
            assert np.allclose(seq.read("moments"), plain.read("moments"), rtol=1e-6, atol=0)
            if k < 4:
                with pytest.raises(mcpt.MCPTError):
                    seq.antilag_info()
            else:
                assert seq.antilag_info()["ran"] is False
    seq.close(), plain.close()
    # refusals
    for kw, name in ((dict(upsample=2), "mcpt_sequence_create_upsampled"),
                     (dict(upsample=2, temporal_upsample=True), "mcpt_sequence_create_temporal_upsampled")):
        with pytest.raises(mcpt.MCPTError, match="not supported in a sequence created by %s" % name):
            mcpt.FrameSequence(scene, 16, 12, 1, denoise=False, antilag=True, **kw)
    with pytest.raises(mcpt.MCPTError, match="MCPT_RENDER_PIXEL_JITTER"):
        mcpt.FrameSequence(scene, 16, 12, 1, denoise=False, antilag=True, flags=mcpt.RENDER_PIXEL_JITTER)
    with pytest.raises(mcpt.MCPTError, match="MCPT_ACCEL_GRID"):
        mcpt.FrameSequence(scene, 16, 12, 1, denoise=False, antilag=True, accel="grid")
    seq = mcpt.FrameSequence(scene, 16, 12, 1, denoise=False)
    for bad, word in ((dict(stratum=9), "stratum"), (dict(radius=4), "radius"), (dict(scale=0.0), "scale")):
        with pytest.raises(mcpt.MCPTError, match=word):
            seq.set_antilag(bad)
    with pytest.raises(TypeError, match="unknown antilag option"):
        seq.set_antilag(dict(strata=2))
    seq.close()


def test_close_frees_what_the_switch_allocated():
    gc.collect()
    scene = mcpt.Scene.load(SCENE_BASE + ".obj", SCENE_BASE + ".xml")
    seq = mcpt.FrameSequence(scene, W, H, 1, denoise=False)
    seq.frame(mcpt.Camera.reference(W, H), SEED)
    before = mcpt.debug_device_bytes_live()
    seq.set_antilag(True)
    during = mcpt.debug_device_bytes_live()
    assert during - before >= 13 * W * H * 8
    seq.set_antilag(False)
    seq.set_antilag(True)  # allocated once
    assert mcpt.debug_device_bytes_live() == during
    seq.frame(mcpt.Camera.reference(W, H), SEED + 1)
    seq.frame(mcpt.Camera.reference(W, H), SEED + 2)
    assert seq.antilag_info()["ran"] is True
    grown = mcpt.debug_device_bytes_live()  # the scene's own work buffers of render_rays
    seq.close()
    assert grown - mcpt.debug_device_bytes_live() == during - before


# ---- 7. the CLI ----

def test_cli_antilag_on_both_paths(tmp_path):
    def run(tag, *extra):
        r = subprocess.run([CLI, "--scene", SCENE_BASE, "--out", str(tmp_path / (tag + ".bmp")), "--hdr", str(tmp_path / (tag + ".pfm")),
                            "--width", str(QW), "--height", str(QH), "--spp", str(SPP), "--frames", "3",
                            *extra], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        peaks = [float(m.group(1)) for m in re.finditer(r"anti-lag: stratum 2, phase \(\d, \d\), Lambda mean [0-9.]+, max ([0-9.]+)", r.stdout)]
        return peaks, [str(tmp_path / ("%s_%04d" % (tag, k))) for k in range(3)], r.stdout

    # --dim 0:0.1 multiplies the group's radiance by 0.1 before every frame k >= 1: every frame's gradient sees an edit
    edit = ("--dim", "%d:0.1" % 0, "--antilag", "--antilag-stratum", "2")
    p_host, host, out = run("host", *edit)
    p_dev, dev, _ = run("dev", *edit, "--device-sequence")
    # the printed maxima (four decimals) of two runs that rendered anew
    assert len(p_host) == len(p_dev) == 2 and np.allclose(p_host, p_dev, rtol=0, atol=2e-4) and min(p_host) > 0.3, out
    # the stale history is dropped: a frame after the edit is nearer to a tenth of the frame before than to that frame
    f0, f1 = read_pfm(host[0] + ".pfm"), read_pfm(host[1] + ".pfm")
    assert f1.sum() < 0.6 * f0.sum()
    for a, b in zip(host, dev):
        # both runs rendered anew: equal up to the framebuffer's summation order, far below float32 and a grey level
        assert np.allclose(read_pfm(a + ".pfm"), read_pfm(b + ".pfm"), rtol=1e-6, atol=1e-30)
        x, y = read_bmp(a + ".bmp").astype(int), read_bmp(b + ".bmp").astype(int)
        assert np.abs(x - y).max() <= 1 and (x != y).mean() <= 1e-3
