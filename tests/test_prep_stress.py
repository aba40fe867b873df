"""The light prep at its cull thresholds and away from the origin, on the MI355X: `pytest -m gpu`.
The scenes of scenegen.prep_stress at the six places and sizes of stresscases.CASES; inputs, oracle results and the
long-double reference come from tests/prepcases.py, and tests/test_prep_stress_cpu.py checks their power without a GPU.

1. Threshold decisions.  At both points of every threshold pair (fp64-adjacent shading points astride the light-side
   or the tangent-plane test's 1e-8; the value is far inside the packed-fp32 cull's error, so every one of them takes
   the fp64 fallback, which must round as the reference does): counts and picks the oracle's, from mcpt_light_prep,
   from every prep variant and from the exact fallback alone.
2. Away from the origin.  1 000 points on both sides of every facet: counts and picks exact, weights_sum within 1e-3.
3. Accuracy.  Variant 17's weights_sum against the long-double reference, no worse than twice the oracle's.
4. Frames.  `hard` at 32 x 24 x 8 MIS against the oracle, in fp64 and with MCPT_RENDER_PRECISION_FP32."""
import functools

import numpy as np
import pytest

import monte_carlo_path_tracing_amd as mcpt
from conftest import NORTH_STAR_TOL, TIGHT_L2, TIGHT_PX
from oracle import pyoracle as po
import prepcases as pc

pytestmark = pytest.mark.gpu
CASES = list(pc.CASES)
TOL = 1e-3  # weights_sum against the oracle: tests/test_exact_pick_stress.py's


def bits(x):
    return np.ascontiguousarray(x).view(np.int64)


def rel(a, b):
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


def jumps(ws, ows, plane):
    """the plane pairs' weights_sum steps (hi - lo) and the oracle's"""
    k = np.flatnonzero(plane)
    return ws[2 * k + 1] - ws[2 * k], ows[2 * k + 1] - ows[2 * k]


def assert_jump(ws, ows, plane, what):
    got, want = jumps(ws, ows, plane)
    assert (want > 0).all()
    assert (got > 0).all() and (np.abs(got - want) <= TOL * want).all(), (what, got, want)


@pytest.mark.parametrize("case", CASES)
def test_threshold_decisions_plain(case):
    s = pc.scene(case, "plain")
    X, N, u, plane = pc.pair_points(case, "plain")
    ows, ocnt, opick, _ = pc.pair_reference(case, "plain")
    seen = ocnt > 0
    ws, cnt, pick = mcpt.light_prep(s, X, N, u)
    print("%s / plain: %d points; light_prep counts equal %d, picks equal %d" % (case, len(X), (cnt == ocnt).sum(), (pick == opick).sum()))
    assert np.array_equal(cnt, ocnt), (np.flatnonzero(cnt != ocnt), cnt[cnt != ocnt], ocnt[cnt != ocnt])
    assert np.array_equal(pick, opick), np.flatnonzero(pick != opick)
    assert rel(ws, ows)[seen].max() <= TOL and (ws[~seen] == 0).all()
    assert_jump(ws, ows, plane, "light_prep")
    _, w17, p17 = mcpt.debug_prep_bench(s, X, N, u, variant=17, iters=1)
    for v in (18, 8):  # the same candidates in the same order, so the same bits
        _, wv, pv = mcpt.debug_prep_bench(s, X, N, u, variant=v, iters=1)
        assert np.array_equal(bits(wv), bits(w17)), (v, np.flatnonzero(wv != w17), wv[wv != w17], w17[wv != w17])
        assert np.array_equal(pv, p17), v
    assert (w17[~seen] == 0).all()
    assert_jump(w17, ows, plane, "variant 17")
    _, w0, p0 = mcpt.debug_prep_bench(s, X, N, u, variant=0, iters=1)
    assert np.array_equal(p0, p17)
    assert rel(w0, ows)[seen].max() <= TOL and (w0[~seen] == 0).all()
    assert_jump(w0, ows, plane, "variant 0")
    we, ce, pe = mcpt.debug_light_prep_exact(s, X, N, u)
    assert np.array_equal(ce, ocnt) and np.array_equal(pe, opick)
    assert_jump(we, ows, plane, "exact")


@pytest.mark.parametrize("case", CASES)
def test_threshold_decisions_few(case):
    s = pc.scene(case, "few")
    assert s.nlights <= 64
    X, N, u, plane = pc.pair_points(case, "few")
    ows, ocnt, opick, _ = pc.pair_reference(case, "few")
    seen = ocnt > 0
    ws, cnt, pick = mcpt.light_prep(s, X, N, u)
    print("%s / few: %d points; light_prep counts equal %d, picks equal %d" % (case, len(X), (cnt == ocnt).sum(), (pick == opick).sum()))
    assert np.array_equal(cnt, ocnt), (np.flatnonzero(cnt != ocnt), cnt[cnt != ocnt], ocnt[cnt != ocnt])
    assert np.array_equal(pick, opick), np.flatnonzero(pick != opick)
    assert_jump(ws, ows, plane, "light_prep")
    _, w9, p9 = mcpt.debug_prep_bench(s, X, N, u, variant=9, iters=1)
    assert np.array_equal(p9[seen], opick[seen]), np.flatnonzero(p9 != opick)
    assert rel(w9, ows)[seen].max() <= TOL and (w9[~seen] == 0).all()
    assert_jump(w9, ows, plane, "variant 9")


@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("case", CASES)
def test_light_prep_away_from_the_origin(case, kind):
    s = pc.scene(case, kind)
    X, N, u = pc.points(case, kind)
    ows, ocnt, opick, _ = pc.reference(case, kind)
    ws, cnt, pick = mcpt.light_prep(s, X, N, u)
    lit = ocnt > 0
    r = rel(ws, ows)
    print("%s / %s: N_L %d, %d of %d points see lights; counts equal %d, picks equal %d; weights_sum max rel diff %.2e" % (
        case, kind, s.nlights, lit.sum(), len(X), (cnt == ocnt).sum(), (pick == opick).sum(), r[lit].max()))
    assert lit.sum() >= 200
    assert np.array_equal(cnt, ocnt), (np.flatnonzero(cnt != ocnt)[:10], cnt[cnt != ocnt][:10], ocnt[cnt != ocnt][:10])
    assert np.array_equal(pick, opick), np.flatnonzero(pick != opick)[:10]
    assert r[lit].max() <= TOL
    if kind != "few":
        _, w17, p17 = mcpt.debug_prep_bench(s, X, N, u, variant=17, iters=1)
        _, w18, p18 = mcpt.debug_prep_bench(s, X, N, u, variant=18, iters=1)
        assert (w17 > 0).sum() >= 200
        assert np.array_equal(bits(w17), bits(w18)) and np.array_equal(p17, p18)


@pytest.mark.parametrize("case", CASES)
def test_weights_sum_accuracy(case):
    """variant 17's weights_sum (the Van Oosterom-Strackee form in fp64) and the oracle's (the reference's literal
    alpha + beta + gamma - pi) against the long-double reference on the accuracy points: E_gpu <= 2 E_ref.  Both take
    p - x1 in fp64, which dominates far from the origin; the table is in DESIGN.md 3.6."""
    X, N, u = pc.points(case, "plain")
    ows = pc.reference(case, "plain")[0]
    _, acc, hp = pc.accuracy(case)
    _, w17, _ = mcpt.debug_prep_bench(pc.scene(case, "plain"), X, N, u, variant=17, iters=1)
    LD = np.longdouble
    e_gpu = float((np.abs(w17[acc].astype(LD) - hp[acc]) / hp[acc]).max())
    e_ref = float((np.abs(ows[acc].astype(LD) - hp[acc]) / hp[acc]).max())
    print("%s: %d accuracy points; E_gpu %.3e, E_ref %.3e" % (case, acc.sum(), e_gpu, e_ref))
    assert acc.sum() >= 160
    assert e_gpu <= 2 * e_ref


# ---- frames ----
W, H, SPP = 32, 24, 8


def rel_l2(g, c):
    return float(np.linalg.norm(g - c) / max(np.linalg.norm(c), 1e-300))


def px_rel(g, c):
    d = np.linalg.norm((g - c).reshape(-1, 3), axis=1)
    n = np.linalg.norm(c.reshape(-1, 3), axis=1)
    return np.where(n > 0, d / np.maximum(n, 1e-300), np.where(d > 0, np.inf, 0.0))


@functools.lru_cache(maxsize=None)
def oracle_frame(case):
    osc = pc.oracle(case, "hard")
    oc = osc.camera()
    oc.width, oc.height = W, H
    e, _ = po.camera_ray(oc, 0, 0)
    osc.build_grid(e)
    ref, _ = osc.render(oc, po.MODE_MIS, pc.SEED, SPP, nthreads=16)
    ref.setflags(write=False)
    return ref


def camera(case):
    cam = pc.scene(case, "hard").camera()
    cam.width, cam.height = W, H
    return cam


@pytest.mark.parametrize("case", CASES)
def test_mis_frame_vs_oracle(case):
    ref = oracle_frame(case)
    img, st = mcpt.render(pc.scene(case, "hard"), camera(case), SPP, mode="mis", seed=pc.SEED)
    l2, mx = rel_l2(img, ref), float(px_rel(img, ref).max())
    print("%s hard %dx%dx%d MIS: rel L2 %.3e, max per-pixel %.3e; %d shading nodes, %d band tests, %d exact preps" % (
        case, W, H, SPP, l2, mx, st.shading_nodes, st.prep_band_nodes, st.prep_exact_nodes))
    assert np.isfinite(img).all() and np.isfinite(ref).all() and (ref.reshape(-1, 3).sum(axis=1) > 0).mean() > 0.5
    assert l2 <= NORTH_STAR_TOL and mx <= NORTH_STAR_TOL, (l2, mx)
    assert l2 <= TIGHT_L2 and mx <= TIGHT_PX, (l2, mx)
    if case == "origin":
        assert st.prep_exact_nodes > 0  # the exact fallback runs


@pytest.mark.parametrize("case", CASES)
def test_fp32_frame_vs_oracle(case):
    """MCPT_RENDER_PRECISION_FP32 under the rule of test_gpu_parity.test_precision_fp32_vs_oracle: frame relative L2
    <= 1e-3, at most 1 % of the pixels beyond 1e-3 and none beyond 0.5"""
    ref = oracle_frame(case)
    img, _ = mcpt.render(pc.scene(case, "hard"), camera(case), SPP, mode="mis", seed=pc.SEED, flags=mcpt.RENDER_PRECISION_FP32)
    l2, px = rel_l2(img, ref), px_rel(img, ref)
    print("%s hard %dx%dx%d MIS fp32 prep: rel L2 %.3e, max per-pixel %.3e, pixels > 1e-3: %.4f" % (
        case, W, H, SPP, l2, px.max(), (px > 1e-3).mean()))
    assert np.isfinite(img).all() and (img >= 0).all()
    assert l2 <= NORTH_STAR_TOL
    assert (px > 1e-3).mean() <= 0.01 and px.max() <= 0.5
