"""The light-prep stress inputs and their high-precision reference, without a GPU (the GPU half is
tests/test_prep_stress.py; the shared pieces are tests/prepcases.py).  Conditions on the generators, judged by the
oracle alone -- inputs that a subtly wrong kernel cannot pass:

1. Threshold pairs (prepcases.pairs): on `plain` and `few` at every place and size, at least 8 pairs of fp64-adjacent
   shading points astride the tangent-plane test's 1e-8 and at least 8 astride the light-side test's, the oracle's
   survivor sets different on the two sides; the plane pairs change the count by exactly one light.
2. The shading points (prepcases.points): at least 200 of the 1 000 see lights in every scene; on `plain` the chunks of
   64 lights lie above, below and across the points' tangent planes, and at least 80 % of the lit points are accuracy
   points (prepcases.accuracy).
3. The long-double reference of the weights (prepcases.sigma_w_hp) against mpmath at 50 digits."""
import numpy as np
import pytest

import prepcases as pc
import scenegen

CASES = list(pc.CASES)


@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("case", CASES)
def test_scene_layout(case, kind):
    """the kind's lights, every one of them, at the case's place and size; the camera moved with the scene"""
    off, scale = pc.CASES[case]
    osc, L = pc.oracle(case, kind), pc.lights(case, kind)
    assert osc.nlights == scenegen.PREP_NLIGHTS[kind] == len(L["P"])
    assert (osc.nlights <= 64) == (kind == "few")
    v = osc.facets()[0][:12, :9].astype(np.float64).reshape(-1, 3)  # the floor: the file's first box
    lo = scale * (np.asarray(off) + (-4.0, -0.2, -4.0))  # the floor's lowest corner
    assert np.allclose(v.min(axis=0), lo, rtol=1e-6, atol=1e-6 * scale)
    panel = L["P"][L["lsum"] == 6.0].reshape(-1, 3)
    assert np.allclose(panel.max(axis=0) - panel.min(axis=0), scale * np.array([3.0, 0.3, 3.0]), rtol=1e-2)
    cam = osc.camera()
    assert np.allclose(list(cam.eye), scale * (np.asarray(off) + scenegen.CAM[0]), rtol=1e-9, atol=1e-9 * scale)
    assert np.allclose(list(cam.lookat), scale * (np.asarray(off) + scenegen.CAM[1]), rtol=1e-9, atol=1e-9 * scale)


def ulps_apart(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("kind", ["plain", "few"])
@pytest.mark.parametrize("case", CASES)
def test_threshold_pairs(case, kind):
    ps = pc.pairs(case, kind)
    _, cnt, pick, surv = pc.pair_reference(case, kind)
    plane = [k for k, p in enumerate(ps) if p["test"] == "plane"]
    side = [k for k, p in enumerate(ps) if p["test"] == "side"]
    assert len(plane) >= 8 and len(side) >= 8, (len(plane), len(side))
    for k, p in enumerate(ps):
        assert not np.array_equal(p["x_lo"], p["x_hi"])
        assert ulps_apart(p["x_lo"], p["x_hi"]).max() <= 1.0  # the last bits only
        lo, hi = set(surv[2 * k].tolist()), set(surv[2 * k + 1].tolist())
        assert lo != hi and p["light"] in lo ^ hi
        if p["test"] == "plane":  # the peeking vertex belongs to one light: exactly that light appears
            assert hi - lo == {p["light"]} and not lo - hi and cnt[2 * k + 1] == cnt[2 * k] + 1
    # the plane pairs vary the normal and the vertex that peeks; the side pairs the light
    assert len({p["light"] for p in (ps[k] for k in plane)}) >= 2
    assert len({tuple(ps[k]["n"]) for k in plane}) >= 4
    assert len({ps[k]["light"] for k in side}) >= 8
    print("%s / %s: %d plane pairs, %d side pairs; lights flipping per side pair: %s" % (
        case, kind, len(plane), len(side), [len(set(surv[2 * k].tolist()) ^ set(surv[2 * k + 1].tolist())) for k in side]))


@pytest.mark.parametrize("case", CASES)
def test_power_of_the_points(case):
    for kind in pc.KINDS:
        _, cnt, _, _ = pc.reference(case, kind)
        assert (np.asarray(cnt) > 0).sum() >= 200, (kind, (np.asarray(cnt) > 0).sum())
    # chunk classes on `plain`: every (point, chunk of 64 lights) by the signs of n . (p - x1) over the chunk's vertices
    L = pc.lights(case, "plain")
    X, N, _ = pc.points(case, "plain")
    t = np.einsum("lkc,nc->nlk", L["P"], N) - np.einsum("nc,nc->n", X, N)[:, None, None]  # (points, lights, 3)
    nch = (len(L["P"]) + 63) // 64
    above = below = across = 0
    for c in range(nch):
        tc = t[:, 64 * c:64 * (c + 1)].reshape(len(X), -1)
        a, b = (tc > 0).all(axis=1), (tc < 0).all(axis=1)
        above, below, across = above + a.sum(), below + b.sum(), across + (~a & ~b).sum()
    print("%s: (point, chunk) classes above %d, below %d, across %d" % (case, above, below, across))
    assert nch == 10 and min(above, below, across) >= 300
    lit, acc, _ = pc.accuracy(case)
    print("%s: %d lit points, %d accuracy points" % (case, lit.sum(), acc.sum()))
    assert lit.sum() >= 200 and acc.sum() >= 0.8 * lit.sum()


def _to_mp(x):
    import mpmath as mp
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - np.longdouble(hi)))  # a long double is the sum of two doubles, exactly


@pytest.mark.parametrize("case,kind", [("offset-1e3", "plain"), ("origin", "plain"), ("large", "few")])
def test_long_double_reference_vs_mpmath(case, kind):
    """sigma_w_hp against the same formulas in mpmath at 50 digits, on the first 20 lit points x all lights.

    Measured (x87 long double, 64-bit significand), worst over the three scenes:
      weights_sum, relative                        1.3e-19
      one weight, error relative to weights_sum    7.7e-21
      one weight, relative to itself               1.2e-16
    The last is not the format's 1e-19: it is a light seen at grazing incidence (its plane 6e-4 units from the point),
    where a . (e1 x e2) cancels three digits -- the triangle's own conditioning, and a weight of 4e-6 of the sum.  Every
    weight seen from more than 0.1 units off its plane: 8.2e-19.  The asserted bounds are 4 x the measured values; what
    tests/test_prep_stress.py uses is the sum."""
    import mpmath as mp
    L = pc.lights(case, kind)
    X, N, _ = pc.points(case, kind)
    _, cnt, _, _ = pc.reference(case, kind)
    lit = np.flatnonzero(np.asarray(cnt) > 0)[:20]
    assert len(lit) == 20
    e_sum = e_w = e_rel = e_far = 0.0
    with mp.workdps(50):
        for k in lit:
            s, w, tmp, _, cand = pc.sigma_w_hp(L, X[k], N[k])
            m = pc.sigma_w_mp(L, X[k], N[k])
            total = sum(m)
            assert total > 0
            for i in range(len(w)):
                assert (w[i] > 0) == (m[i] > 0) and (m[i] > 0) <= bool(cand[i])
                if m[i] > 0:
                    d = abs(_to_mp(w[i]) - m[i])
                    e_w, e_rel = max(e_w, float(d / total)), max(e_rel, float(d / m[i]))
                    if tmp[i] > 0.1 * pc.CASES[case][1]:
                        e_far = max(e_far, float(d / m[i]))
            e_sum = max(e_sum, float(abs(_to_mp(s) - total) / total))
    print("%s / %s: long double vs mpmath: weights_sum %.2e, a weight over the sum %.2e, a weight %.2e, off grazing %.2e" % (
        case, kind, e_sum, e_w, e_rel, e_far))
    assert e_sum <= 5.2e-19 and e_w <= 3.1e-20 and e_rel <= 4.7e-16 and e_far <= 3.3e-18
