"""History clamping (mcpt_temporal_accumulate_clamped; include/mcpt.h states the rule): the GPU against
`emulate_clamped`, a numpy restatement built on test_temporal's `emulate_temporal` (the fast history IS that
emulator run with alpha = alpha_fast on prev_fast; then the box over the hit taps of the clipped window, the clamp
and the moment correction), fed identical host arrays; plus the ABI checks and the emulator's quality on the
oracle's frames, which need no GPU.

The clamp adds no discrete decision: min / max are continuous, and which taps count is decided by the miss marker
depth = 0, which is exact.  So the left-out pixels are test_temporal's (emulator margin < 1e-9), widened by the
window's radius because a pixel's box reads the fast history of its neighbours; the inputs below leave none out.

Gates: check_outputs of test_temporal on colour, moments and variance; TIGHT_L2 / TIGHT_PX on the fast colour; the
shift at 1e-6 relative to max(|shift|, the largest fast-history channel value in the pixel's window): the shift is a
difference of quantities of that size, so its rounding is about 1e-16 of it
(test_clamp_gates_keep_margin_over_rounding).

Quality (eight 4-spp frames against 256 spp at the last camera, seed + 100), the emulator on the oracle's frames
where this file was written, tone-mapped relative L2 / relative MSE:
  1.5 deg a frame: raw 0.323 / 0.081, accumulated 0.237 / 0.177, clamped 0.207 / 0.063,
                   accumulated + denoised 0.234 / 0.035, clamped + denoised 0.227 / 0.032
  0.5 deg a frame: raw 0.312 / 0.089, accumulated 0.151 / 0.123, clamped 0.146 / 0.040,
                   accumulated + denoised 0.178 / 0.026, clamped + denoised 0.183 / 0.026
The clamp restores "accumulated beats the raw frame" in relative MSE, which is what is asserted (clamped < raw and
clamped < accumulated, at both steps; margins of 22 % and 55 % against the raw frame).  After the filter the clamp
gains little at 1.5 degrees and nothing at 0.5, where the tone-mapped L2 gets worse (0.178 -> 0.183); nothing about
the filtered frames is asserted.  The clamp moves 12 to 30 of the 768 pixels a frame."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE_OBJ, SCENE_XML, TIGHT_L2, TIGHT_PX
import monte_carlo_path_tracing_amd as mcpt
from oracle import pyoracle as po
from test_denoise import emulate, lum, max_px_rel, read_pfm, rel_l2, rel_mse, synthetic, spatial_variance, tm_l2
from test_temporal import (DEFAULTS, FRAMES, H, KEYS, LOW, ORBIT, SEED, SPP, W, analytic_inputs, check_outputs,
                           emulate_temporal, oracle_sequence, taps_touch)

CLAMP = dict(radius=2, alpha_fast=0.5, sigma=2.0)
MID_ORBIT = 0.5  # degrees a frame: the smallest step at which the unclamped history is worse than the raw frame
# at sigma 2 the analytic frames' wide fast history moves few pixels (none at radius 3): every radius also runs at 0.5
CLAMP_CASES = [{}, dict(radius=1), dict(radius=3), dict(sigma=0.5), dict(sigma=0.0), dict(radius=1, sigma=0.5),
               dict(radius=3, sigma=0.5)]
CLAMP_IDS = ["defaults", "radius1", "radius3", "sigma0.5", "sigma0", "radius1-sigma0.5", "radius3-sigma0.5"]
NEW_SYMBOLS = ("mcpt_temporal_clamp_opts_init", "mcpt_temporal_accumulate_clamped", "mcpt_temporal_accumulate_clamped_device")
SHIFT_GATE = 1e-6


# ---- the rule of include/mcpt.h in numpy ----

def emulate_clamped(color, g, prev=None, clamp=None, **opts):
    """(out_color, out_moments, out_fast, out_variance, out_shift, info) of the rule; prev = (camera, guides, colour,
    moments, fast) or None.  info: emulate_temporal's, plus per pixel `fastmax` (the largest |fast| in the window),
    `sd_positive` (a positive deviation in every channel), `clipped` (the window leaves the frame) and `misses` (it
    holds miss taps); the last three are False without history"""
    cl = dict(CLAMP, **(clamp or {}))
    r, sigma = cl["radius"], cl["sigma"]
    color = np.asarray(color, dtype=np.float64)
    hh, ww = color.shape[:2]
    S, mom, _, info = emulate_temporal(color, g, None if prev is None else prev[:4], **opts)
    if prev is None:
        F = color.copy()
    else:
        F = emulate_temporal(color, g, (prev[0], prev[1], prev[4], prev[3]), **dict(opts, alpha=cl["alpha_fast"]))[0]
    hist, hit = info["history"], g["depth"] > 0
    cnt, s = np.zeros((hh, ww)), np.zeros((hh, ww, 3))
    fastmax, taps = np.zeros((hh, ww)), np.zeros((hh, ww))
    offs = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]  # rows top to bottom, columns left to right
    ii, jj = np.mgrid[0:hh, 0:ww]

    def tap(dy, dx):
        qi, qj = ii + dy, jj + dx
        inside = (qi >= 0) & (qi < hh) & (qj >= 0) & (qj < ww)
        qi, qj = np.clip(qi, 0, hh - 1), np.clip(qj, 0, ww - 1)
        return inside, inside & hit[qi, qj], F[qi, qj]

    for dy, dx in offs:
        inside, ok, Fq = tap(dy, dx)
        cnt = cnt + ok
        s = s + np.where(ok[..., None], Fq, 0.0)
        taps = taps + inside
        fastmax = np.maximum(fastmax, np.where(ok, np.abs(Fq).max(-1), 0.0))
    k = np.where(hist, cnt, 1.0)[..., None]
    mu = s / k
    v = np.zeros((hh, ww, 3))
    for dy, dx in offs:
        _, ok, Fq = tap(dy, dx)
        e = Fq - mu
        v = v + np.where(ok[..., None], e * e, 0.0)
    sd = np.sqrt(v / k)
    wd = sigma * sd
    out = np.where(hist[..., None], np.minimum(np.maximum(S, mu - wd), mu + wd), S)
    shift = np.where(hist, lum(out) - lum(S), 0.0)
    m1 = mom[..., 0]
    m1n = m1 + shift
    m2n = mom[..., 1] + (m1n * m1n - m1 * m1)
    mom = np.stack([m1n, m2n, mom[..., 2], mom[..., 3]], -1)
    gg, temporal = mom[..., 3], info["temporal"]
    vt = np.maximum(0.0, m2n - m1n * m1n) * gg / np.where(temporal, 1.0 - gg, 1.0)
    o = dict(DEFAULTS, **opts)
    var = np.where(temporal, vt, spatial_variance(out, g, o["sigma_normal"], o["sigma_plane"], o["sigma_albedo"]))
    info = dict(info, fastmax=fastmax, sd_positive=hist & (sd > 0).all(-1), clipped=hist & (taps < (2 * r + 1) ** 2),
                misses=hist & (cnt < taps))
    return out, mom, F, var, shift, info


def widen(mask, r):
    """the pixels within r of a pixel of mask (test_temporal's dilate needs a frame wider than r)"""
    hh, ww = mask.shape
    out = mask.copy()
    for i, j in zip(*np.nonzero(mask)):
        out[max(i - r, 0):i + r + 1, max(j - r, 0):j + r + 1] = True
    return out


def shift_error(got, want, fastmax):
    """the shift's error on its gate's scale, per pixel"""
    scale = np.maximum(np.abs(want), fastmax)
    d = np.abs(got - want)
    return np.where(scale > 0, d / np.where(scale > 0, scale, 1.0), np.where(d > 0, np.inf, 0.0))


def check_clamped(got, want, radius, skip=None):
    """(colour, moments, fast, variance, shift) of the GPU against the emulator's (with its info).  Left out: the
    emulator's low-margin pixels and `skip`, widened by the window's radius.  Returns the pixels left out."""
    gc, gm, gf, gv, gs = got
    wc, wm, wf, wv, ws, info = want
    low = info["margin"] < LOW
    if skip is not None:
        low = low | skip
    out = widen(low, radius)
    check_outputs((gc, gm, gv), (wc, wm, wv, info), skip=out)
    keep = ~out
    assert np.isfinite(gf).all() and np.isfinite(gs).all()
    # the fast history of a low-margin pixel itself differs, its neighbours' does not
    l2, px = rel_l2(gf[~low], wf[~low]), max_px_rel(gf[~low], wf[~low])
    rs = float(shift_error(gs, ws, info["fastmax"])[keep].max()) if keep.any() else 0.0
    print("fast colour rel L2 %.3e, max pixel %.3e; shift max rel %.3e; shift != 0 in %d of %d pixels with history"
          % (l2, px, rs, (ws != 0).sum(), info["history"].sum()))
    assert l2 <= TIGHT_L2 and px <= TIGHT_PX
    assert rs <= SHIFT_GATE
    assert np.all(gs[keep & ~info["history"]] == 0)
    return out


def emulate_clamped_sequence(frames, clamp=None, **opts):
    """the emulator chained over (camera, colour, guides) frames -> per frame (colour, moments, fast, variance, shift,
    info, tainted); a tainted pixel taints the pixels whose taps touch it a frame later and its window at once"""
    r = dict(CLAMP, **(clamp or {}))["radius"]
    prev, tainted, outs = None, None, []
    for cam, img, g in frames:
        c, m, f, v, s, info = emulate_clamped(img, g, prev, clamp, **opts)
        low = info["margin"] < LOW
        tainted = widen(low if tainted is None else low | taps_touch(tainted, info), r)
        outs.append((c, m, f, v, s, info, tainted))
        prev = (cam, g, c, m, f)
    return outs


# ---- inputs ----

_cpu = {}


def analytic_clamp_inputs():
    """test_temporal's analytic frames (37 x 29, 4 degree orbit, the slab occluder) with a previous fast history that
    differs from the long one by noise wide enough for a box of half a standard deviation to leave pixels alone"""
    if "a" not in _cpu:
        cam0, g0, pcol, pmom, cam1, g1, color = analytic_inputs()
        rng = np.random.default_rng(12)
        pfast = pcol + rng.uniform(-3.0, 3.0, pcol.shape)
        pfast.setflags(write=False)
        _cpu["a"] = ((cam0, g0, pcol, pmom, pfast), g1, color)
    return _cpu["a"]


def oracle_quality(orbit):
    """test_temporal's oracle frames along `orbit` degrees a frame and the oracle's 256-spp frame at the last camera
    (seed + 100)"""
    if orbit not in _cpu:
        frames, _ = oracle_sequence(orbit)
        osc = po.Scene(SCENE_OBJ, SCENE_XML)
        ocam = po.Camera.from_buffer_copy(frames[-1][0])
        eye, _ = po.camera_ray(ocam, 0, 0)
        osc.build_grid(eye)
        _cpu[orbit] = (frames, osc.render(ocam, po.MODE_MIS, SEED + 100, 256, nthreads=4)[0])
    return _cpu[orbit]


def quality_numbers(img, acc, clamped, dn_acc, dn_clamped, ref):
    """tone-mapped relative L2 / relative MSE of the five frames, printed; returns the relative MSEs"""
    m = [(tm_l2(x, ref), rel_mse(x, ref)) for x in (img, acc, clamped, dn_acc, dn_clamped)]
    print("tone-mapped rel L2 / relative MSE: raw %.3f / %.3f, accumulated %.3f / %.3f, clamped %.3f / %.3f, "
          "accumulated + denoised %.3f / %.3f, clamped + denoised %.3f / %.3f" % tuple(v for p in m for v in p))
    return [p[1] for p in m]


@pytest.fixture(scope="module")
def scene():
    return mcpt.Scene.load(SCENE_OBJ, SCENE_XML)


_gpu = {}


def gpu_sequence(scene, orbit):
    """the GPU's eight 4-spp frames along the orbit with their AOVs, the outputs of TemporalAccumulator(clamp=True) and
    of the plain accumulator for each, and the 256-spp frame at the last camera, once"""
    if orbit not in _gpu:
        acc, plain = mcpt.TemporalAccumulator(clamp=True), mcpt.TemporalAccumulator()
        assert plain.clamp is None
        frames, outs, unclamped = [], [], []
        for k in range(FRAMES):
            cam = mcpt.camera_orbit(mcpt.Camera.reference(W, H), k * orbit)
            img, _ = mcpt.render(scene, cam, SPP, mode="mis", seed=SEED + k)
            aov = mcpt.render_aovs(scene, cam)
            c, v = acc.push(cam, img, aov)
            assert acc.clamped == float((acc.shift != 0).mean())
            frames.append((cam, img, aov))
            outs.append((c, acc.moments, acc.fast, v, acc.shift))
            unclamped.append(plain.push(cam, img, aov))
        ref = mcpt.render(scene, cam, 256, mode="mis", seed=SEED + 100)[0]
        _gpu[orbit] = (frames, outs, unclamped, ref)
    return _gpu[orbit]


# ---- GPU ----

@pytest.mark.gpu
@pytest.mark.parametrize("clamp", CLAMP_CASES, ids=CLAMP_IDS)
def test_clamped_vs_emulator_on_analytic_frames(clamp):
    prev, g1, color = analytic_clamp_inputs()
    want = emulate_clamped(color, g1, prev, clamp, **DEFAULTS)
    got = mcpt.temporal_accumulate_clamped(color, g1, prev, clamp or None)
    left = check_clamped(got[:5], want, dict(CLAMP, **clamp)["radius"])
    assert not left.any()  # test_analytic_clamp_inputs_meet_the_conditions: no decision is close
    assert got[5] > 0
    if clamp.get("sigma") == 0.0:  # the history is replaced by the window's mean: every pixel with history moves
        assert (want[4][want[5]["history"]] != 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ww,hh", [(1, 1), (5, 3), (2, 70)])
def test_clamped_vs_emulator_on_tiny_frames(ww, hh):
    """radius 3: every window is clipped on at least two sides (test_temporal's tiny frames and their camera)"""
    rng = np.random.default_rng(ww * 100 + hh)
    color, _, g = synthetic(ww, hh, seed=ww * 100 + hh)
    clamp = dict(radius=3)
    check_clamped(mcpt.temporal_accumulate_clamped(color, g, None, clamp)[:5], emulate_clamped(color, g, None, clamp, **DEFAULTS), 3)
    cam = mcpt.Camera()
    cam.eye[:] = (0.05 * ww + 0.03, 0.05 * hh + 0.02, -2.0)
    cam.lookat[:] = (0.05 * ww, 0.05 * hh, 2.0)
    cam.up[:] = (0.0, -1.0, 0.0)
    cam.fovy, cam.dist_scale, cam.width, cam.height = 360.0 * np.arctan(0.0125 * hh), 1.0, ww, hh
    pcol = rng.uniform(0.0, 2.0, (hh, ww, 3))
    n = rng.integers(0, 6, (hh, ww)).astype(np.float64)
    m1 = lum(pcol)
    pmom = np.stack([m1, m1 * m1 + rng.uniform(0.0, 0.2, (hh, ww)), n, 1.0 / np.maximum(n, 1.0)], -1)
    prev = (cam, g, pcol, pmom, rng.uniform(0.0, 2.0, (hh, ww, 3)))
    want = emulate_clamped(color, g, prev, clamp, **DEFAULTS)
    check_clamped(mcpt.temporal_accumulate_clamped(color, g, prev, clamp)[:5], want, 3)
    if ww * hh > 1:
        assert want[5]["history"].any() and want[5]["clipped"][want[5]["history"]].all()


@pytest.mark.gpu
def test_clamped_accumulator_vs_emulator_on_a_rendered_orbit(scene):
    """1.5 degrees a frame through TemporalAccumulator(clamp=True): every output of every frame"""
    frames, outs, _, _ = gpu_sequence(scene, ORBIT)
    want = emulate_clamped_sequence(frames, **DEFAULTS)
    for k in range(FRAMES):
        print("frame %d" % k)
        check_clamped(outs[k], want[k][:6], 0, skip=want[k][6])  # the taint is already widened
    assert all((w[4] != 0).any() for w in want[1:])
    assert not (want[0][4] != 0).any()


@pytest.mark.gpu
def test_clamp_invariants():
    prev, g1, color = analytic_clamp_inputs()
    cam0, g0, pcol, pmom, pfast = prev
    # the fast history is the plain accumulation of prev_fast with alpha = alpha_fast, bit for bit
    out, mom, fast, var, shift, _ = mcpt.temporal_accumulate_clamped(color, g1, prev)
    assert np.array_equal(fast, mcpt.temporal_accumulate(color, g1, (cam0, g0, pfast, pmom), alpha=CLAMP["alpha_fast"])[0])
    assert (shift != 0).any()
    # a box too wide to clamp anything returns the plain accumulation, bit for bit, except where the window's
    # deviation is 0 in some channel (lo = hi = mean).  On these frames that is no pixel at all: every pixel with
    # history has at least two hit taps with different values in its window.
    c0, m0, v0, _ = mcpt.temporal_accumulate(color, g1, prev[:4])
    c1, m1, f1, v1, s1, _ = mcpt.temporal_accumulate_clamped(color, g1, prev, dict(sigma=1e30))
    info = emulate_clamped(color, g1, prev, dict(sigma=1e30), **DEFAULTS)[5]
    excluded = info["history"] & ~info["sd_positive"]
    print("pixels whose window has a zero deviation: %d" % excluded.sum())
    assert excluded.sum() == 0
    assert np.array_equal(c1, c0) and np.array_equal(m1, m0) and np.array_equal(v1, v0) and np.all(s1 == 0)
    assert np.array_equal(f1, fast)
    # no previous state: nothing to clamp
    out, mom, fast, var, shift, _ = mcpt.temporal_accumulate_clamped(color, g1)
    c0, m0, v0, _ = mcpt.temporal_accumulate(color, g1)
    assert np.all(shift == 0) and np.array_equal(fast, color) and np.array_equal(out, color)
    assert np.array_equal(mom, m0) and np.array_equal(var, v0)


@pytest.mark.gpu
def test_clamped_device_form_equals_host_form(scene):
    import torch
    frames, outs, _, _ = gpu_sequence(scene, ORBIT)
    (cam0, _, aov0), (cam1, img1, aov1) = frames[0], frames[1]
    c0, m0, f0, _, _ = outs[0]
    t = lambda a: torch.from_numpy(np.array(a)).cuda()
    dimg, dc0, dm0, df0 = t(img1), t(c0), t(m0), t(f0)
    dg0, dg1 = {k: t(aov0[k]) for k in KEYS}, {k: t(aov1[k]) for k in KEYS}
    f64 = dict(dtype=torch.float64, device="cuda")
    do, dm, df = torch.zeros((H, W, 3), **f64), torch.zeros((H, W, 4), **f64), torch.zeros((H, W, 3), **f64)
    dv, ds = torch.zeros((H, W), **f64), torch.zeros((H, W), **f64)
    prev = (cam0, {k: a.data_ptr() for k, a in dg0.items()}, dc0.data_ptr(), dm0.data_ptr(), df0.data_ptr())
    ptrs = {k: a.data_ptr() for k, a in dg1.items()}
    torch.cuda.synchronize()
    sec = mcpt.temporal_accumulate_clamped_device(W, H, dimg.data_ptr(), ptrs, do.data_ptr(), dm.data_ptr(), df.data_ptr(),
                                                  dv.data_ptr(), ds.data_ptr(), prev=prev)
    assert sec > 0
    for d, h in zip((do, dm, df, dv, ds), outs[1]):
        assert np.array_equal(d.cpu().numpy(), h)
    # neither variance nor shift; no previous state
    do2, dm2, df2 = torch.zeros_like(do), torch.zeros_like(dm), torch.zeros_like(df)
    torch.cuda.synchronize()
    mcpt.temporal_accumulate_clamped_device(W, H, dimg.data_ptr(), ptrs, do2.data_ptr(), dm2.data_ptr(), df2.data_ptr(), prev=prev)
    assert np.array_equal(do2.cpu().numpy(), outs[1][0]) and np.array_equal(dm2.cpu().numpy(), outs[1][1])
    assert np.array_equal(df2.cpu().numpy(), outs[1][2])
    torch.cuda.synchronize()
    mcpt.temporal_accumulate_clamped_device(W, H, dimg.data_ptr(), ptrs, do2.data_ptr(), dm2.data_ptr(), df2.data_ptr())
    assert np.array_equal(do2.cpu().numpy(), img1) and np.array_equal(df2.cpu().numpy(), img1)


@pytest.mark.gpu
def test_cli_history_clamp(scene, tmp_path):
    cli = os.path.join(ROOT, "monte_carlo_path_tracing_amd", "mcpt_render")
    bmp, pfm = str(tmp_path / "out.bmp"), str(tmp_path / "out.pfm")
    r = subprocess.run([cli, "--scene", os.path.splitext(str(SCENE_OBJ))[0], "--width", str(W), "--height", str(H),
                        "--frames", "3", "--orbit", str(ORBIT), "--spp", str(SPP), "--history-clamp", "2", "--hdr", pfm,
                        "--out", bmp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("frame ")]
    assert len(lines) == 3 and all("kept their history" in ln and "the clamp moved" in ln for ln in lines), r.stdout
    frames, outs, unclamped, _ = gpu_sequence(scene, ORBIT)
    assert "the clamp moved 0.0% of the pixels" in lines[0]
    assert "the clamp moved %.1f%% of the pixels" % (100.0 * (outs[2][4] != 0).mean()) in lines[2]
    got = read_pfm(str(tmp_path / "out_0002.pfm"))
    assert np.allclose(got, outs[2][0].astype(np.float32), rtol=1e-6, atol=1e-30)
    assert not np.allclose(got, unclamped[2][0].astype(np.float32), rtol=1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("orbit", [ORBIT, MID_ORBIT])
def test_clamped_frame_beats_the_raw_and_the_unclamped_frame(scene, orbit):
    """The orderings test_clamp_emulator_on_the_oracle_orbits shows on the oracle's frames, and no others: in relative
    MSE the clamped accumulated frame is below the raw last frame and below the unclamped accumulated frame."""
    frames, outs, unclamped, ref = gpu_sequence(scene, orbit)
    _, img, aov = frames[-1]
    acc, var = unclamped[-1]
    clamped, var_c = outs[-1][0], outs[-1][3]
    dn_acc, dn_clamped = mcpt.denoise(acc, aov, variance=var)[0], mcpt.denoise(clamped, aov, variance=var_c)[0]
    raw, plain, cl, _, _ = quality_numbers(img, acc, clamped, dn_acc, dn_clamped, ref)
    assert cl < raw
    assert cl < plain


# ---- CPU ----

def test_analytic_clamp_inputs_meet_the_conditions():
    """what the analytic frames must offer at sigma 0.5: between 10 % and 90 % of the pixels with history move, in both
    directions, some windows are clipped by the border and some contain miss taps; no pixel is left out"""
    prev, g1, color = analytic_clamp_inputs()
    assert rel_l2(prev[4], prev[2]) >= 0.1  # the fast history is not the long one
    for clamp in CLAMP_CASES:
        c, m, f, v, s, info = emulate_clamped(color, g1, prev, clamp, **DEFAULTS)
        hist = info["history"]
        moved = (s != 0) & hist
        print("%s: shift != 0 in %d of %d pixels with history, %d up, %d down; clipped windows %d, with misses %d"
              % (clamp, moved.sum(), hist.sum(), (s > 0).sum(), (s < 0).sum(), info["clipped"].sum(), info["misses"].sum()))
        assert not (info["margin"] < LOW).any()
        assert all(np.isfinite(a).all() for a in (c, m, f, v, s))
        assert not (s[~hist] != 0).any()
        assert info["clipped"].any() and info["misses"].any() and (hist & ~info["clipped"] & ~info["misses"]).any()
        if clamp.get("sigma") == 0.5:  # at every radius
            assert 0.1 * hist.sum() <= moved.sum() <= 0.9 * hist.sum()
            assert (s > 0).any() and (s < 0).any()
        # the central moment survives the correction (to rounding of m2)
        S, m0, _, _ = emulate_temporal(color, g1, prev[:4], **DEFAULTS)
        assert np.abs((m[..., 1] - m[..., 0] ** 2) - (m0[..., 1] - m0[..., 0] ** 2)).max() <= 1e-12 * m[..., 1].max()


@pytest.mark.parametrize("orbit", [ORBIT, MID_ORBIT])
def test_clamp_emulator_on_the_oracle_orbits(orbit):
    """The restatement on the oracle's eight 4-spp frames at 1.5 and 0.5 degrees a frame: finite outputs, the 1 % cap,
    the clamp moves at least one pixel and at most half of those with history in every frame after the first, and the
    orderings the GPU test asserts (the module's docstring has the numbers)."""
    frames, ref = oracle_quality(orbit)
    seq = emulate_clamped_sequence(frames, **DEFAULTS)
    for k, (c, m, f, v, s, info, tainted) in enumerate(seq):
        assert tainted.mean() <= 0.01
        assert all(np.isfinite(a).all() for a in (c, m, f, v, s))
        moved = (s != 0).sum()
        print("frame %d: the clamp moved %d of %d pixels with history" % (k, moved, info["history"].sum()))
        assert (moved == 0) if k == 0 else (1 <= moved <= 0.5 * info["history"].sum())
    prev = None
    for cam, img, g in frames:
        c, m, v, _ = emulate_temporal(img, g, prev, **DEFAULTS)
        prev = (cam, g, c, m)
    _, img, g = frames[-1]
    clamped, var_c = seq[-1][0], seq[-1][3]
    raw, plain, cl, _, _ = quality_numbers(img, c, clamped, emulate(c, v, g)[0], emulate(clamped, var_c, g)[0], ref)
    assert cl < raw
    assert cl < plain


def test_clamp_gates_keep_margin_over_rounding():
    """Every input perturbed by 1e-15 relative (n' = 0 and the miss marker stay), on the analytic frames with every clamp
    setting: where this test was written the fast colour moved by 1.1e-14 L2 and 6.7e-13 per pixel, the shift by
    1.1e-14 on its gate's scale, against gates of 1e-8 / 1e-6 and 1e-6: six orders and more; a thousandth of each gate
    is asserted."""
    rng = np.random.default_rng(5)
    nz = lambda a: np.asarray(a) * (1.0 + 1e-15 * rng.uniform(-1.0, 1.0, np.shape(a)))
    nzg = lambda g: {k: nz(v) for k, v in g.items()}
    (cam0, g0, pcol, pmom, pfast), g1, color = analytic_clamp_inputs()
    worst = np.zeros(3)
    for clamp in CLAMP_CASES:
        pm = nz(pmom)
        pm[..., 2] = pmom[..., 2]
        a = emulate_clamped(color, g1, (cam0, g0, pcol, pmom, pfast), clamp, **DEFAULTS)
        b = emulate_clamped(nz(color), nzg(g1), (cam0, nzg(g0), nz(pcol), pm, nz(pfast)), clamp, **DEFAULTS)
        worst = np.maximum(worst, [rel_l2(b[2], a[2]), max_px_rel(b[2], a[2]), shift_error(b[4], a[4], a[5]["fastmax"]).max()])
    print("fast colour L2 %.2e, per pixel %.2e; shift on its scale %.2e" % tuple(worst))
    assert worst[0] <= 1e-3 * TIGHT_L2 and worst[1] <= 1e-3 * TIGHT_PX
    assert worst[2] <= 1e-3 * SHIFT_GATE


def test_clamp_symbols_are_exported():
    hdr = (ROOT / "include" / "mcpt.h").read_text()
    declared = set(re.findall(r"\b(mcpt_[a-z_0-9]+)\s*\(", hdr))
    L = mcpt.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in mcpt.EXPORTS and hasattr(L, name), name
    for name in ("TemporalClampOpts", "temporal_accumulate_clamped", "temporal_accumulate_clamped_device"):
        assert name in mcpt.__all__ and hasattr(mcpt, name), name
    assert L.mcpt_version() == mcpt.MCPT_VERSION == 20300
    acc = mcpt.TemporalAccumulator()
    assert acc.clamp is None and acc.clamped == 0.0
    assert mcpt.TemporalAccumulator(clamp=dict(sigma=1.5), alpha=0.2).clamp == dict(sigma=1.5)
    with pytest.raises(TypeError):
        mcpt.temporal_accumulate_clamped(np.zeros((2, 2, 3)), {k: np.zeros((2, 2) if k == "depth" else (2, 2, 3)) for k in KEYS},
                                         clamp=dict(k=2))


def test_clamp_opts_layout_matches_header(tmp_path):
    py = mcpt.TemporalClampOpts
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mcpt.h"', "int main(void) {",
           'printf("sizeof %zu\\n", sizeof(mcpt_temporal_clamp_opts));']
    for f, _ in py._fields_:
        src.append('printf("%s %%zu\\n", offsetof(mcpt_temporal_clamp_opts, %s));' % (f, f))
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(py)
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset, f
    c = py()
    mcpt.lib().mcpt_temporal_clamp_opts_init(C.byref(c))
    assert c.struct_size == C.sizeof(py)
    assert {k: getattr(c, k) for k in CLAMP} == CLAMP


def _call(opts=None, clamp=None, width=6, height=4, null=(), alias=None, no_prev=False):
    """mcpt_temporal_accumulate_clamped on a 6x4 frame with the given changes to a valid call -> (rc, message)"""
    color, _, g = synthetic(6, 4)
    o, c = mcpt.TemporalOpts(), mcpt.TemporalClampOpts()
    mcpt.lib().mcpt_temporal_opts_init(C.byref(o))
    mcpt.lib().mcpt_temporal_clamp_opts_init(C.byref(c))
    for k, v in (opts or {}).items():
        setattr(o, k, v)
    for k, v in (clamp or {}).items():
        setattr(c, k, v)
    cam = mcpt.Camera.reference(6, 4)
    ins = dict(color=color, prev_color=np.ones((4, 6, 3)), prev_moments=np.ones((4, 6, 4)), prev_fast=np.ones((4, 6, 3)))
    outs = dict(out_color=np.full((4, 6, 3), 7.0), out_moments=np.full((4, 6, 4), 7.0), out_fast=np.full((4, 6, 3), 7.0),
                out_variance=np.full((4, 6), 7.0), out_shift=np.full((4, 6), 7.0))
    b = mcpt.AovBuffers(*[g[k].ctypes.data for k in KEYS])
    pb = mcpt.AovBuffers(*[g[k].ctypes.data for k in KEYS])
    ptr = {k: a.ctypes.data for k, a in {**ins, **outs}.items()}
    if alias:
        ptr[alias[0]] = ptr[alias[1]] if alias[1] in ptr else g[alias[1]].ctypes.data
    if no_prev:
        null = tuple(null) + ("prev_cam", "prev_guides", "prev_color", "prev_moments")
    for k in null:
        if k in ptr:
            ptr[k] = None
    rc = mcpt.lib().mcpt_temporal_accumulate_clamped(
        C.byref(o), None if "clamp" in null else C.byref(c), None if "prev_cam" in null else C.byref(cam), width, height,
        ptr["color"], C.byref(b), None if "prev_guides" in null else C.byref(pb), ptr["prev_color"], ptr["prev_moments"],
        ptr["prev_fast"], ptr["out_color"], ptr["out_moments"], ptr["out_fast"], ptr["out_variance"], ptr["out_shift"], None)
    for a in outs.values():
        assert np.all(a == 7.0)
    return rc, mcpt.lib().mcpt_last_error().decode()


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("kw,word", [
    (dict(clamp={"struct_size": 8}), "mcpt_temporal_clamp_opts.struct_size"),
    *[(dict(clamp={"radius": v}), "radius") for v in (0, 4, -1)],
    *[(dict(clamp={"alpha_fast": v}), "alpha_fast") for v in (0.0, -0.1, 1.5, NAN)],
    *[(dict(clamp={"sigma": v}), "sigma") for v in (-1.0, NAN, INF)],
    (dict(null=("clamp",)), "clamp"),
    (dict(null=("out_fast",)), "out_fast"),
    (dict(null=("prev_fast",)), "prev_fast"),
    (dict(no_prev=True), "prev_fast"),
    *[(dict(alias=a), "aliasing") for a in (("out_fast", "color"), ("out_fast", "prev_fast"), ("out_fast", "prev_color"),
                                            ("out_fast", "out_color"), ("out_shift", "depth"), ("out_shift", "out_variance"),
                                            ("out_shift", "out_fast"), ("out_shift", "prev_moments"), ("out_color", "prev_fast"),
                                            ("out_moments", "prev_fast"))],
    # and what mcpt_temporal_accumulate refuses
    (dict(opts={"struct_size": 8}), "mcpt_temporal_opts.struct_size"),
    (dict(opts={"alpha": 0.0}), "alpha"),
    (dict(width=0), "width"),
    (dict(null=("color",)), "color"),
    (dict(null=("out_color",)), "out_color"),
    (dict(null=("prev_cam",)), "prev_cam"),
    (dict(null=("prev_moments",)), "prev_moments"),
    (dict(alias=("out_color", "color")), "aliasing"),
])
def test_invalid_clamped_calls_are_refused(kw, word):
    """MCPT_E_INVALID with a message naming the argument, before any device work (this test needs no GPU); the
    outputs stay untouched"""
    rc, msg = _call(**kw)
    assert rc == -1, (rc, msg)
    assert word in msg, msg


def test_valid_clamped_calls_pass_the_argument_checks():
    """the valid call of _call, with and without a previous state and the optional outputs, ends at the device"""
    for kw in (dict(), dict(no_prev=True, null=("prev_fast",)), dict(null=("out_shift", "out_variance"))):
        rc, msg = _call(opts={"device": 1 << 20}, **kw)  # no such device: the call ends there, after every argument check
        assert rc != 0 and not any(w in msg for w in ("null", "partial", "aliasing", "invalid", "struct_size")), (rc, msg)
