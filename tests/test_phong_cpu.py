"""The Phong functions' test inputs and tolerances, checked without a GPU: the oracle's brdf_phong, phong_pdf and
sample_phong against a 240-bit mpmath evaluation of BRDF.cpp's formulas on the records of tests/phonggen.py, and the
conditions that keep the GPU test (tests/test_phong.py) honest.  Nothing here reads the code under test: it pins the
constants the GPU test takes its margin from.

K_ref, the oracle's largest error per output in units of 2^-53 * cond (phonggen.conds) over the 3 564 records of
phonggen.subset, rounded up to a power of two:

    output                      measured   K_ref
    brdf (3 channels)           1.84       2
    pdf                         0.86       1
    sampled direction           1.24       2
    sample pdf                  1.40       2

The condition numbers start from cond = 4 + 4 sh / c (lobes), 1 + (c / st)(1 + |log2 k1| / (sh + 1)) (direction) and
2 + |log2 k1| (specular sample pdf) and were refined where a class needed it; each change is written down at
phonggen.conds and phonggen.normalised_errors:
  * a frame term 4 st / |axis x e| for the specular lobe's direction (without it the oracle itself reads 1 800 on
    the records whose mirror axis is one frame switch away from e_x);
  * a lobe whose dot product is below 2^-40 is compared as an interval over c +- 2^-50 (sh / c has no meaning for a c
    of a few ulps, and Ns = -0.5 turns c = 0 into an infinity);
  * the brdf and pdf outputs are sums, so their denominators add the sum itself and, for the pdf, the diffuse part's
    own cancelling dot product;
  * an absolute 1e-280 is granted everywhere (a product that underflows to a denormal or to zero).
"""
import numpy as np
import pytest

import phonggen as pg


@pytest.fixture(scope="module")
def data():
    rec, cls = pg.generate()
    dec = pg.decisions(rec)
    return rec, cls, dec, pg.oracle_outputs(rec)


def test_records_are_float32_materials_and_unit_vectors(data):
    rec, cls, dec, orc = data
    assert 38000 <= rec.shape[0] <= 42000
    mats = rec[:, 9:16]
    assert np.array_equal(mats, mats.astype(np.float32).astype(np.float64))
    for k in range(3):
        assert np.abs(np.linalg.norm(rec[:, 3 * k:3 * k + 3], axis=1) - 1).max() <= 4e-16
    assert ((rec[:, 16:19] >= 0) & (rec[:, 16:19] < 1)).all()
    assert set(cls["geo"]) == set(pg.GEO) and set(cls["wi"]) == set(pg.WI)
    rec2, _ = pg.generate()
    assert np.array_equal(rec, rec2)  # deterministic


def test_decisions_are_the_oracles(data):
    """phonggen.decisions repeats the oracle's arithmetic: every decision that shows in the oracle's outputs agrees"""
    rec, cls, dec, orc = data
    ks, kd = rec[:, 12:15], rec[:, 9:12]
    nonblack = (kd.sum(1) + ks.sum(1)) > 0
    spec = orc[:, :3] - kd * (1.0 / np.pi)
    # where the specular term shows: no diffuse part to be absorbed in, and Ns <= 0.5, so that no c > 0 underflows
    shown = (ks[:, 0] > 0) & (kd.sum(1) == 0) & (rec[:, 15] <= 0.5)
    assert shown.sum() >= 2000 and (~dec["c_pos"][shown]).sum() >= 100
    assert np.array_equal(spec[shown, 0] > 0, dec["c_pos"][shown])
    p0 = dec["p0"]
    lobe0 = dec["ind"] == 0
    with np.errstate(all="ignore"):
        assert np.array_equal(orc[lobe0 & nonblack, 7] <= p0[lobe0 & nonblack] / np.pi * (1 + 1e-15), np.ones((lobe0 & nonblack).sum(), bool))
    # the frame switch: the sampled direction of the other frame differs in the azimuth's origin; checked through the
    # degenerate frame: an axis of exactly -e_x takes the e_x frame and gives the reference's NaN direction
    neg_ex = (dec["axis"][:, 0] == -1.0) & (dec["axis"][:, 1] == 0) & (dec["axis"][:, 2] == 0)
    assert neg_ex.sum() >= 50 and np.array_equal(np.isnan(orc[:, 4]), neg_ex)


def test_coverage_conditions(data):
    rec, cls, dec, orc = data
    lb, lp = pg.lobe_estimates(rec, dec)
    cells = pg.reachable_cells(rec, cls)
    assert len(cells) == 2 * len(set(cls["mat"])) - 7 - 1  # no specular lobe for the 7 diffuse classes, no cosine lobe for black
    for mat, lobe in cells:
        cell = (cls["mat"] == mat) & (dec["ind"] == lobe)
        assert cell.sum() >= 200, (mat, lobe, cell.sum())
        for l in (lb, lp):
            rel = cell & (l >= pg.LOBE_MIN)
            assert rel.sum() >= 0.25 * cell.sum(), (mat, lobe, rel.sum(), cell.sum())
            smp = cell & (cls["wi"] == "sampled_spec")
            under = smp & (l < pg.LOBE_MIN)
            assert smp.sum() >= 40 and under.sum() <= 0.05 * smp.sum(), (mat, lobe, under.sum(), smp.sum())
    for lobe in (0, 1):
        for side in (True, False):
            assert ((dec["ind"] == lobe) & (dec["frame_ex"] == side)).sum() >= 50
    for key, names in (("u0", pg.U0), ("k1", pg.K1), ("k2", pg.K2)):
        for name in names:
            assert (cls[key] == name).sum() >= 50, (key, name)
    k1 = rec[:, 17]
    for k in range(20, 54):
        assert (k1 == 1 - 2.0 ** -k).sum() >= 50, k
    p0 = dec["p0"]
    assert ((rec[:, 16] == p0) & (p0 > 0) & (p0 < 1)).sum() >= 50  # u0 == p0 exactly, inside (0, 1)
    # the subset is stratified over the cells and small enough for the high-precision comparison
    sub = pg.subset(rec, cls)
    assert len(sub) <= 4000
    for mat, lobe in cells:
        assert ((cls["mat"][sub] == mat) & (dec["ind"][sub] == lobe)).sum() >= 40, (mat, lobe)


def test_oracle_against_mpmath_pins_k_ref(data):
    """the oracle's normalised errors stay within K_REF, and K_REF is the measured maximum rounded up to a power of
    two (see the module docstring) -- no record of the subset is skipped: NaNs and infinities are compared as such"""
    rec, cls, dec, orc = data
    sub = pg.subset(rec, cls)
    worst = {k: (0.0, None) for k in pg.OUTPUTS}
    nrel = 0
    for i in sub:
        ref = pg.mp_reference(rec, dec, i)
        ne = pg.normalised_errors(orc[i], ref, pg.conds(ref, 0))
        nrel += ne["relative"]
        for k in pg.OUTPUTS:
            if ne[k] > worst[k][0]:
                worst[k] = (ne[k], (cls["mat"][i], cls["geo"][i], cls["wi"][i], cls["u0"][i], cls["k1"][i], cls["k2"][i]))
    for k in pg.OUTPUTS:
        print("oracle %-5s max %.3f of 2^-53 cond at %s (K_ref %g)" % (k, worst[k][0], worst[k][1], pg.K_REF[k]))
    assert nrel >= 0.25 * len(sub)
    for k in pg.OUTPUTS:
        assert pg.K_REF[k] / 2 < worst[k][0] <= pg.K_REF[k], (k, worst[k])
