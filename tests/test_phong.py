"""device_math.h's brdf_phong, phong_pdf and sample_phong, run one record per thread through mcpt_debug_phong with the
template arguments the render kernels use (variant 0: the MIS / shade() kernels, variant 1: the BRDF-only kernels),
against the oracle on every record of tests/phonggen.py (~40 000) and against a 240-bit mpmath evaluation on its
stratified subset (3 564).  The error model, its units (2^-53 * cond) and the oracle's own constants K_ref are those
of tests/test_phong_cpu.py; the kernels are granted 4 K_ref (the device's pow, acos and sincos are other ~1-ulp
implementations of what glibc gives the oracle, feeding the same amplification), variant 1 with its header's own terms
added to cond (2 |sh log2 c| for exp2(y log2 x), |log2 k1| / (sh + 1) doubled).

Measured on an MI355X (largest normalised error per output over the subset; bound 4 K_ref):

    output               oracle (K_ref)   variant 0   variant 1   bound
    brdf (3 channels)    1.84 (2)         1.839       1.839       8
    pdf                  0.86 (1)         0.853       0.853       4
    sampled direction    1.24 (2)         1.236       1.000       8
    sample pdf           1.40 (2)         1.393       1.385       8

Variant 0 equals the oracle bit for bit on 31 330 of the 39 960 records and has its pattern of zeros, NaNs and signs
on all of them.  Per material class the largest variant-0 errors lie between 0.14 (specular, Ns = 0) and 1.84
(Ks = (0.3, 0, 0.2), Ns = 50) for brdf, 0.14-0.85 for pdf, 0.60-1.24 for the direction and 0.28-1.39 (Ns = 1e6) for
the sample pdf; variant 1's between 0.14-1.84, 0.14-0.85, 0.28-1.00 and 0.28-1.39 (its cond carries the header's own
terms).  Variant 1 differs from variant 0 by at most 0.028 of the summed bounds in brdf (Ns = 0.5 and -0.5: exp2 / log2),
0.067 in the direction and 0.053 in the sample pdf; phong_pdf is bit-identical between the two.  Ns = 2e6, beyond
phong_pow_bounded, and Ns = -0.5 stay inside the same bounds as every other class: no shortcut exceeded its model.
"""
import ctypes as C

import numpy as np
import pytest

import monte_carlo_path_tracing_amd as mcpt
import phonggen as pg

pytestmark = pytest.mark.gpu
FACTOR = 4.0  # the kernels' margin over K_ref


@pytest.fixture(scope="module")
def data():
    rec, cls = pg.generate()
    dec = pg.decisions(rec)
    return rec, cls, dec, pg.oracle_outputs(rec)


@pytest.fixture(scope="module")
def dev(data):
    rec = data[0]
    return [mcpt.debug_phong(rec, v) for v in (0, 1)]


@pytest.fixture(scope="module")
def refs(data):
    """the high-precision reference of every subset record, computed once: (index, ref, conds of variant 0 and 1)"""
    rec, cls, dec, orc = data
    out = []
    for i in pg.subset(rec, cls):
        ref = pg.mp_reference(rec, dec, i)
        out.append((i, ref, (pg.conds(ref, 0), pg.conds(ref, 1))))
    return out


def _zeroed(out):
    """values the error model counts as zero (at most ABS_MAX: underflowed products) as zeros"""
    return np.where(np.abs(out) <= pg.ABS_MAX, 0.0, out)


def _mismatch(cls, bad):
    i = np.nonzero(bad)[0]
    return [(int(j), cls["mat"][j], cls["geo"][j], cls["wi"][j], cls["u0"][j], cls["k1"][j], cls["k2"][j]) for j in i[:5]]


def test_entry_validation():
    assert mcpt.debug_phong(np.zeros((0, 19)), 0).shape == (0, 8)  # n == 0: nothing to do
    one = np.zeros((1, 19))
    for variant in (-1, 2):
        with pytest.raises(mcpt.MCPTError):
            mcpt.debug_phong(one, variant)
    L = mcpt.lib()
    assert L.mcpt_debug_phong(-1, 0, one.reshape(-1), np.zeros(8)) == -1  # MCPT_E_INVALID
    raw = C.CFUNCTYPE(C.c_int, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p)(("mcpt_debug_phong", L))
    out = np.zeros(8)
    assert raw(1, 0, None, out.ctypes.data) == -1 and raw(1, 0, one.ctypes.data, None) == -1  # a null array


@pytest.mark.parametrize("variant", [0, 1])
def test_patterns_equal_the_oracles(data, dev, variant):
    """zeros, NaNs, infinities and signs of all 8 outputs on every record: c > 0, ct < 0, cs < 0, p0 >= u0, the frame
    switch and the side of the surface the sampled direction lies on are decided on dot products evaluated in the
    oracle's order with contraction off, so none may differ (black materials: the oracle's NaN pattern).

    Variant 1's direction is the one exception, and not a decision: sincospi(2 k2) is exactly 0 or +-1 at the quarter
    turns, where the oracle's sincos(2 pi k2) of the rounded 2 pi leaves 1.2e-16, so a component that vanishes in exact
    arithmetic is 0 in the kernel and +-1e-16 in the oracle (1 529 records on an MI355X, every one of them at most
    1.84e-16 on both sides).  There a component of at most 2^-50 on both sides -- below the smallest direction bound of
    any record, 4 K_ref 2^-53 * 4 -- counts as zero; so does dot(dir, n) for the side of the surface (16 records: k1 in
    {0, 2^-53} with k2 = 0.5 puts the direction into the tangent plane, exactly in the kernel and to -1e-16 in the
    oracle; the sample's weight carries that dot product as a factor).  Variant 0 is compared strictly."""
    rec, cls, dec, orc = data
    g = dev[variant]
    pg_, po_ = pg.pattern(_zeroed(g)), pg.pattern(_zeroed(orc))
    if variant == 1:
        tiny_g, tiny_o = np.abs(g[:, 4:7]) <= pg.C_SLACK, np.abs(orc[:, 4:7]) <= pg.C_SLACK
        print("variant 1: %d records with a direction component of the other sign or zero, all below 2^-50: %s" % (
            int((pg_ != po_).any(1).sum()), bool((tiny_g & tiny_o)[pg_[:, 4:7] != po_[:, 4:7]].all())))
        pg_[:, 4:7][tiny_g & tiny_o] = 0
        po_[:, 4:7][tiny_g & tiny_o] = 0
    bad = (pg_ != po_).any(1)
    assert not bad.any(), (int(bad.sum()), _mismatch(cls, bad))
    n = rec[:, :3]
    with np.errstate(all="ignore"):
        dg, do = pg.dot(g[:, 4:7], n), pg.dot(orc[:, 4:7], n)
    below_g, below_o = dg < 0, do < 0
    bad = below_g != below_o
    if variant == 1:
        print("variant 1: %d directions on the other side of the surface, largest |dot| %.3g" % (
            int(bad.sum()), float(np.max(np.maximum(np.abs(dg), np.abs(do))[bad], initial=0.0))))
        bad &= ~((np.abs(dg) <= pg.C_SLACK) & (np.abs(do) <= pg.C_SLACK))
    print("variant %d: %d of %d sampled directions below the surface" % (variant, int(below_o.sum()), len(rec)))
    assert not bad.any(), (int(bad.sum()), _mismatch(cls, bad))
    black = cls["mat"] == "black/Ns50"
    assert black.sum() >= 1000 and np.array_equal(np.isnan(g[black]), np.isnan(orc[black]))
    assert np.isnan(orc[black][:, 3]).all() and np.isnan(orc[black][:, 7]).all()


@pytest.mark.parametrize("variant", [0, 1])
def test_zero_specular_is_bit_identical(data, dev, variant):
    """ks == 0 (the skip-zero claim, Ns = 2e6 beyond phong_pow_bounded included): brdf and pdf are the oracle's bits, in
    the kernels that skip the pow and in those that multiply it by zero"""
    rec, cls, dec, orc = data
    g = dev[variant]
    sel = (rec[:, 12:15] == 0).all(1) & (rec[:, 9:12] != 0).any(1)
    assert sel.sum() >= 7000 and (rec[sel, 15] == 2e6).sum() >= 1000
    bad = (np.ascontiguousarray(g[:, :4]).view(np.uint64) != np.ascontiguousarray(orc[:, :4]).view(np.uint64)).any(1) & sel
    assert not bad.any(), (int(bad.sum()), _mismatch(cls, bad))


def _per_class(cls, rows, key="mat"):
    """largest normalised error per class and output: {class: {output: value}}"""
    table = {}
    for i, ne in rows:
        t = table.setdefault(cls[key][i], {k: 0.0 for k in pg.OUTPUTS})
        for k in pg.OUTPUTS:
            t[k] = max(t[k], ne[k])
    return table


@pytest.mark.parametrize("variant", [0, 1])
def test_against_mpmath(data, dev, refs, variant):
    """every subset record within 4 K_ref * 2^-53 * cond of the high-precision reference, per output; the measured
    maxima per material class are printed.  A class beyond its bound is a finding about that kernel's shortcut."""
    rec, cls, dec, orc = data
    g = dev[variant]
    rows = [(i, pg.normalised_errors(g[i], ref, cnd[variant])) for i, ref, cnd in refs]
    table = _per_class(cls, rows)
    print("variant %d: largest error per material class in units of 2^-53 cond (brdf pdf dir spdf)" % variant)
    for mat, t in table.items():
        print("  %-18s %s" % (mat, " ".join("%8.3f" % t[k] for k in pg.OUTPUTS)))
    worst = {k: max(t[k] for t in table.values()) for k in pg.OUTPUTS}
    print("variant %d: overall %s; bound %s" % (variant, " ".join("%s %.3f" % (k, worst[k]) for k in pg.OUTPUTS),
                                                " ".join("%g" % (FACTOR * pg.K_REF[k]) for k in pg.OUTPUTS)))
    for k in pg.OUTPUTS:
        bad = [(i, ne[k]) for i, ne in rows if not ne[k] <= FACTOR * pg.K_REF[k]]
        assert not bad, (k, len(bad), [(i, e, cls["mat"][i], cls["geo"][i], cls["wi"][i], cls["u0"][i], cls["k1"][i],
                                        cls["k2"][i]) for i, e in bad[:5]])


def test_variant1_against_variant0(data, dev, refs):
    """the BRDF-only kernels' forms against the MIS kernels': on the subset every output differs by at most the sum of
    the two bounds; on every record the lobe choice and the cosine lobe's pdf agree (the sample pdf to the sum of the
    two variants' bounds, evaluated in fp64)"""
    rec, cls, dec, orc = data
    g0, g1 = dev
    k = {o: FACTOR * pg.K_REF[o] for o in pg.OUTPUTS}
    rows = []
    for i, ref, cnd in refs:
        t0, t1 = pg.abs_tolerances(ref, cnd[0], k), pg.abs_tolerances(ref, cnd[1], k)
        with np.errstate(all="ignore"):
            d = np.abs(g1[i] - g0[i])
            d = np.where(np.isnan(g0[i]) & np.isnan(g1[i]) | (g0[i] == g1[i]), 0.0, d)  # equal NaNs and infinities
            d = np.where(np.isnan(d), np.inf, d)
            ddir = float(np.sqrt((d[4:7] ** 2).sum()))
        tol = {o: np.add(t0[o], t1[o]) for o in pg.OUTPUTS}
        frac = {"brdf": float(np.max(np.where(d[:3] == 0, 0.0, d[:3] / tol["brdf"]))), "pdf": 0.0 if d[3] == 0 else d[3] / tol["pdf"],
                "dir": 0.0 if ddir == 0 else ddir / tol["dir"], "spdf": 0.0 if d[7] == 0 else d[7] / tol["spdf"]}
        rows.append((i, frac))
    table = _per_class(cls, rows)
    print("variant 1 - variant 0: largest difference per material class as a fraction of the summed bounds (brdf pdf dir spdf)")
    for mat, t in table.items():
        print("  %-18s %s" % (mat, " ".join("%8.4f" % t[o] for o in pg.OUTPUTS)))
    for o in pg.OUTPUTS:
        bad = [(i, f[o]) for i, f in rows if not f[o] <= 1.0]
        assert not bad, (o, len(bad), [(i, e, cls["mat"][i], cls["geo"][i], cls["wi"][i], cls["k1"][i]) for i, e in bad[:5]])
    # every record: phong_pdf is the same function in both variants, and the sample pdf shows the lobe choice
    assert np.array_equal(g0[:, 3], g1[:, 3], equal_nan=True)
    k1 = rec[:, 17]
    u = 2.0 ** -53
    with np.errstate(all="ignore"):
        lg = np.where(k1 == 0, 1075.0, np.abs(np.log2(k1)))
        cond = np.where(dec["ind"] == 0, 3 + 2 * np.sqrt(k1) / np.maximum(np.sqrt(1 - k1), 2.0 ** -30), 2 + 1.5 * lg)
        tol = 2 * FACTOR * pg.K_REF["spdf"] * u * cond * np.abs(g0[:, 7]) + pg.ABS_MAX
        d = np.abs(g1[:, 7] - g0[:, 7])
        d = np.where(np.isnan(g0[:, 7]) & np.isnan(g1[:, 7]) | (g0[:, 7] == g1[:, 7]), 0.0, d)
        bad = ~(d <= np.where(np.isnan(tol), 0.0, tol))  # a NaN pdf (black) must be NaN in both
    for lobe in (0, 1):
        sel = (dec["ind"] == lobe) & (d > 0)
        print("all records, lobe %d: sample pdf differs on %d, largest fraction of the bound %.4f" % (
            lobe, int(sel.sum()), float(np.max(d[sel] / tol[sel])) if sel.any() else 0.0))
    assert not bad.any(), (int(bad.sum()), _mismatch(cls, bad))
