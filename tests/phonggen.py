"""Deterministic inputs for the Phong function tests (tests/test_phong_cpu.py, tests/test_phong.py), a
high-precision reference of the same functions and the error model both tests share.

A record is 19 doubles -- n[3] wi[3] wr[3] kd[3] ks[3] sh u0 k1 k2 (mcpt_debug_phong, include/mcpt_debug.h) -- and
carries four class names: its material, its (n, wr) geometry, how wi was chosen and which end points its uniforms sit
on.  The renderer holds materials as float, so kd, ks and sh are float32 values widened to double; directions are fp64
unit vectors as the kernels produce them.

Classes
  material   5 mixes x Ns in {0, 0.5, 1, 50, 5000, 1e6, 2e6}, plus Ns = -0.5 and black (function level only)
  geometry   random; n = +-e_x, +-e_y, +-e_z; the mirror axis of wr exactly e_x; the mirror axis, or n, at
             1 - axis.x = 1e-9, 0.9e-8, 1.1e-8, 1e-7 (both sides of the frame switch at MCPT_EPS); wr grazing
             (dot(wr, n) ~ 1e-9); wr below the surface
  wi         drawn by the oracle's sampler with the specular lobe forced (Kd = 0 for the draw, so that a 1e6 lobe is
             met where it does not underflow) or the cosine lobe forced, each with uniforms of its own; uniform over
             the hemisphere; perpendicular to n (an exactly zero product for the axis normals, a rounded one
             elsewhere); below the surface; the mirror direction; one ulp either side
             of perpendicular to the mirror axis
  uniforms   u0 in {0, p0, nextafter(p0, -+) (kept inside [0, 1 - 2^-53], the range of a uniform), random, 1 - 2^-53};
             k1 in {0, 2^-53, 0.5, random, 1 - 2^-k for k = 20..53}; k2 in {0, 0.25, 0.5, 0.75, random, 1 - 2^-53}

The discrete decisions (c > 0, ct < 0, cs < 0, p0 >= u0, the frame switch) are recomputed here in numpy with the oracle's
operation order (every numpy fp64 operation rounds once, as the oracle's do with contraction off), so that the
high-precision reference takes the oracle's branch.
"""
import numpy as np

EPS = 1e-8
U = 2.0 ** -53
ONE_M = 1.0 - U  # the largest uniform
NS_VALUES = (0.0, 0.5, 1.0, 50.0, 5000.0, 1e6, 2e6)
F32 = np.float32
MIXES = {  # name: (kd, ks)
    "diffuse": ((0.5, 0.5, 0.5), (0.0, 0.0, 0.0)),
    "specular": ((0.0, 0.0, 0.0), (0.5, 0.5, 0.5)),
    "plates": ((0.07, 0.09, 0.13), (0.1, 0.2, 0.3)),
    "kszero": ((0.2, 0.2, 0.2), (0.3, 0.0, 0.2)),
    "tinykd": ((1e-6, 1e-6, 1e-6), (0.5, 0.5, 0.5)),
}
PER_MATERIAL = 1080
GEO = ("random", "n_axis", "mirror_ex", "mirror_near_ex", "n_near_ex", "grazing", "wr_below")
GEO_P = (0.30, 0.12, 0.10, 0.16, 0.12, 0.10, 0.10)
WI = ("sampled_spec", "sampled_cos", "uniform", "perp_n", "below", "mirror", "perp_mirror")
WI_P = (0.35, 0.10, 0.15, 0.08, 0.08, 0.10, 0.14)
U0 = ("zero", "p0", "p0_minus", "p0_plus", "random", "one_m")
U0_P = (0.10, 0.10, 0.10, 0.10, 0.50, 0.10)
K1 = ("zero", "ulp", "half", "random", "near_one")
K1_P = (0.08, 0.08, 0.08, 0.50, 0.26)
K2 = ("zero", "quarter", "half", "three_quarter", "random", "one_m")
K2_P = (0.08, 0.08, 0.08, 0.08, 0.60, 0.08)
NEAR = (1e-9, 0.9e-8, 1.1e-8, 1e-7)


def material_classes():
    """name -> (kd[3], ks[3], sh), all float32 values as doubles"""
    out = {}
    for mix, (kd, ks) in MIXES.items():
        for ns in NS_VALUES:
            out["%s/Ns%g" % (mix, ns)] = (kd, ks, ns)
    out["plates/Ns-0.5"] = MIXES["plates"] + (-0.5,)
    out["black/Ns50"] = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 50.0)
    return {k: (np.array(kd, F32).astype(np.float64), np.array(ks, F32).astype(np.float64), float(F32(sh)))
            for k, (kd, ks, sh) in out.items()}


# ---- the oracle's fp64 arithmetic in numpy (mcpt_oracle.c vdot, vnormalized, vcross: one rounding per operation) ----
def dot(a, b):
    s = 0.0 + a[..., 0] * b[..., 0]
    s = s + a[..., 1] * b[..., 1]
    return s + a[..., 2] * b[..., 2]


def normalized(a):
    l = np.sqrt(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1] + a[..., 2] * a[..., 2])
    return a / l[..., None]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def mirror(w, n):
    """-w + 2 n dot(w, n), the reflection both brdf_phong (of wi) and phong_pdf / sample_phong (of wr) build"""
    return w * -1 + n * (2 * dot(w, n))[..., None]


def decisions(rec):
    """The oracle's discrete decisions for (N, 19) records, and the fp64 values they are taken on."""
    n, wi, wr, kd, ks = (rec[:, 3 * k:3 * k + 3] for k in range(5))
    u0 = rec[:, 16]
    one = np.ones(3)
    with np.errstate(all="ignore"):
        d, s = dot(kd, one) / 3, dot(ks, one) / 3
        tot = (0.0 + d) + s
        p0 = d / tot
        ind = np.where(p0 >= u0, 0, 1)
        c = dot(wr, mirror(wi, n))
        ct = dot(wi, n)
        R = normalized(mirror(wr, n))
        cs = dot(wi, R)
        axis = np.where((ind == 0)[:, None], n, R)
        frame_ex = np.abs(dot(axis, np.array([1.0, 0.0, 0.0])) - 1) > EPS
    return dict(p0=p0, ind=ind, c=c, c_pos=c > 0, ct=ct, ct_neg=ct < 0, cs=cs, cs_neg=cs < 0, axis=axis, frame_ex=frame_ex)


def lobe_estimates(rec, dec):
    """fp64 estimates of the scalar lobe values (sh + 1) c^sh / (2 pi) of brdf_phong and phong_pdf (NaN where the branch
    is not taken) -- for counting which records sit in the underflow range, not for comparing"""
    sh = rec[:, 15]
    with np.errstate(all="ignore"):
        lb = np.where(dec["c_pos"], (sh + 1) * np.power(np.abs(dec["c"]), sh) / (2 * np.pi), np.nan)
        lp = np.where(~dec["cs_neg"], (sh + 1) * np.power(np.abs(dec["cs"]), sh) / (2 * np.pi), np.nan)
    return lb, lp


# ---- the generator ---------------------------------------------------------------------------------------------------
def _unit(rng, m):
    v = rng.standard_normal((m, 3))
    return normalized(v)


def _tangent(rng, a):
    """a unit vector perpendicular (up to rounding) to every row of a"""
    t = cross(a, _unit(rng, a.shape[0]))
    return normalized(t)


def _above(rng, n, lo=0.05):
    """random unit vectors with dot(., n) in [lo, 1]"""
    m = n.shape[0]
    z = lo + (1 - lo) * rng.random(m)
    t = _tangent(rng, n)
    return normalized(n * z[:, None] + t * np.sqrt(1 - z * z)[:, None])


def _near_ex(rng, m):
    """unit vectors with 1 - x = one of NEAR (cycled), random azimuth"""
    delta = np.array(NEAR)[np.arange(m) % len(NEAR)]
    x = 1 - delta
    r = np.sqrt(1 - x * x)
    az = 2 * np.pi * rng.random(m)
    return normalized(np.stack([x, r * np.cos(az), r * np.sin(az)], -1))


def _reflect_to(rng, axis):
    """(n, wr) whose mirror axis normalized(-wr + 2 n dot(wr, n)) is `axis` up to rounding, at a random incidence"""
    n = _above(rng, axis, 0.2)
    wr = normalized(mirror(axis, n))
    return n, wr


def _choose(rng, names, p, m):
    return np.array(names)[rng.choice(len(names), size=m, p=np.array(p) / np.sum(p))]


def generate(seed=20240430, per_material=PER_MATERIAL):
    """(records (N, 19) float64, classes: dict of (N,) string arrays "mat", "geo", "wi", "u0", "k1", "k2")"""
    from oracle import pyoracle as po

    rng = np.random.default_rng(seed)
    recs, cls = [], {k: [] for k in ("mat", "geo", "wi", "u0", "k1", "k2")}
    ex = np.array([1.0, 0.0, 0.0])
    axes6 = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0], [0, 0, 1.0], [0, 0, -1.0]])
    for mat, (kd, ks, sh) in material_classes().items():
        m = per_material
        geo = _choose(rng, GEO, GEO_P, m)
        wic = _choose(rng, WI, WI_P, m)
        u0c, k1c, k2c = _choose(rng, U0, U0_P, m), _choose(rng, K1, K1_P, m), _choose(rng, K2, K2_P, m)
        # geometry: every class is generated for all rows and selected, which keeps the stream of random numbers
        # independent of the class counts
        n = _unit(rng, m)
        wr = _above(rng, n)
        sel = geo == "n_axis"
        n_ax = axes6[rng.integers(0, 6, m)]
        wr_ax = _above(rng, n_ax)
        n[sel], wr[sel] = n_ax[sel], wr_ax[sel]
        # the mirror axis exactly e_x: normal incidence on n = e_x, and wr = e_y on the rounded (1, 1, 0) / sqrt 2,
        # whose reflection normalises to x = 1 exactly (asserted below)
        sel = geo == "mirror_ex"
        alt = (np.arange(m) % 2 == 1)[:, None]
        s2 = np.sqrt(0.5)
        n_me = np.where(alt, np.array([s2, s2, 0.0]), ex)
        wr_me = np.where(alt, np.array([0.0, 1.0, 0.0]), ex)
        n[sel], wr[sel] = n_me[sel], wr_me[sel]
        assert (normalized(mirror(wr_me, n_me))[:, 0] == 1.0).all()
        sel = geo == "mirror_near_ex"
        n_ne, wr_ne = _reflect_to(rng, _near_ex(rng, m))
        n[sel], wr[sel] = n_ne[sel], wr_ne[sel]
        sel = geo == "n_near_ex"
        n_nn = _near_ex(rng, m)
        wr_nn = _above(rng, n_nn)
        n[sel], wr[sel] = n_nn[sel], wr_nn[sel]
        sel = geo == "grazing"
        wr_g = normalized(_tangent(rng, n) + n * 1e-9)
        wr[sel] = wr_g[sel]
        sel = geo == "wr_below"
        wr_b = _above(rng, -n)
        wr[sel] = wr_b[sel]
        # uniforms
        p0 = float(decisions(np.concatenate([n[:1], n[:1], wr[:1], kd[None], ks[None], np.zeros((1, 4))], 1))["p0"][0])
        p0c = min(max(p0, 0.0), ONE_M) if p0 == p0 else 0.5
        rnd = rng.random((m, 3)) * (1 - 2 * U) + U  # random uniforms inside (0, 1)
        u0 = np.select([u0c == "zero", u0c == "p0", u0c == "p0_minus", u0c == "p0_plus", u0c == "one_m"],
                       [0.0, p0c, max(np.nextafter(p0c, -1.0), 0.0), min(np.nextafter(p0c, 2.0), ONE_M), ONE_M], rnd[:, 0])
        kk = rng.integers(20, 54, m)
        k1 = np.select([k1c == "zero", k1c == "ulp", k1c == "half", k1c == "near_one"], [0.0, U, 0.5, 1 - 2.0 ** -kk],
                       rnd[:, 1])
        k2 = np.select([k2c == "zero", k2c == "quarter", k2c == "half", k2c == "three_quarter", k2c == "one_m"],
                       [0.0, 0.25, 0.5, 0.75, ONE_M], rnd[:, 2])
        # wi
        R = normalized(mirror(wr, n))
        wi = _above(rng, n, 0.0)  # "uniform": dot(wi, n) uniform in [0, 1] is uniform over the hemisphere
        su = rng.random((m, 2)) * (1 - 2 * U) + U
        kd0 = np.zeros(3)
        ks1 = np.full(3, 0.5)
        for i in np.nonzero((wic == "sampled_spec") | (wic == "sampled_cos"))[0]:
            if wic[i] == "sampled_spec":
                w = po.sample_phong_u(n[i], wr[i], kd0, ks1, sh, ONE_M, su[i, 0], su[i, 1])[:3]
            else:
                w = po.sample_phong_u(n[i], wr[i], ks1, kd0, sh, 0.0, su[i, 0], su[i, 1])[:3]
            if not np.isnan(w).any():  # an axis of exactly -e_x has no frame (NaN): such a ray never reaches a BRDF
                wi[i] = w
        sel = wic == "perp_n"
        wi_p = _tangent(rng, n)
        wi[sel] = wi_p[sel]
        axis_sel = sel & (np.abs(n).max(1) == 1.0)  # an axis normal: make the product exactly zero
        wi[axis_sel] = np.where(np.abs(n[axis_sel]) == 1.0, 0.0, wi[axis_sel])
        wi[axis_sel] = normalized(wi[axis_sel])
        sel = wic == "below"
        wi_b = _above(rng, -n, 0.0)
        wi[sel] = wi_b[sel]
        sel = wic == "mirror"
        wi[sel] = R[sel]
        sel = wic == "perp_mirror"
        wi_pm = _tangent(rng, R)
        step = np.where(rng.random(m) < 0.5, 1.0, -1.0)
        big = np.argmax(np.abs(wi_pm * R), 1)  # one ulp on the component that moves dot(wi, R) most
        rows = np.arange(m)
        wi_pm[rows, big] = np.nextafter(wi_pm[rows, big], step * np.sign(R[rows, big]) * np.inf)
        wi[sel] = wi_pm[sel]
        rec = np.concatenate([n, wi, wr, np.broadcast_to(kd, (m, 3)), np.broadcast_to(ks, (m, 3)),
                              np.full((m, 1), sh), u0[:, None], k1[:, None], k2[:, None]], 1)
        recs.append(rec)
        for k, v in (("mat", np.full(m, mat)), ("geo", geo), ("wi", wic), ("u0", u0c), ("k1", k1c), ("k2", k2c)):
            cls[k].append(v)
    return np.ascontiguousarray(np.concatenate(recs)), {k: np.concatenate(v) for k, v in cls.items()}


def subset(rec, cls, per_cell=54, seed=7):
    """Indices of the records that get the high-precision comparison: up to per_cell of every (material, lobe) cell,
    taken round-robin over the cell's (geometry, wi) classes so that each is met -- at most 4 000 in all."""
    ind = decisions(rec)["ind"]
    rng = np.random.default_rng(seed)
    pick = []
    for mat in dict.fromkeys(cls["mat"]):
        for lobe in (0, 1):
            idx = np.nonzero((cls["mat"] == mat) & (ind == lobe))[0]
            if not len(idx):
                continue
            groups = {}
            for i in rng.permutation(idx):
                groups.setdefault((cls["geo"][i], cls["wi"][i]), []).append(i)
            order = []
            queues = list(groups.values())
            while queues and len(order) < per_cell:
                for q in queues:
                    order.append(q.pop())
                queues = [q for q in queues if q]
            pick += order[:per_cell]
    out = np.array(sorted(pick))
    assert len(out) <= 4000
    return out


def oracle_outputs(rec):
    """(N, 8) brdf[3] pdf dir[3] sample_pdf of the oracle, one call per function and record"""
    from oracle import pyoracle as po

    out = np.zeros((rec.shape[0], 8))
    with np.errstate(all="ignore"):
        for i, r in enumerate(rec):
            n, wi, wr, kd, ks = (np.ascontiguousarray(r[3 * k:3 * k + 3]) for k in range(5))
            out[i, :3] = po.brdf_phong(n, wi, wr, kd, ks, r[15])
            out[i, 3] = po.phong_pdf(n, wi, wr, kd, ks, r[15])
            out[i, 4:] = po.sample_phong_u(n, wr, kd, ks, r[15], r[16], r[17], r[18])
    return out


def pattern(out):
    """zeros, NaNs, infinities and signs of the outputs: 0 zero, 1 / -1 the sign of a finite value, 2 / -2 of an
    infinity, 3 NaN (the sign of a zero is not part of the pattern: -0 + x and +0 + x are the same sum)"""
    p = np.sign(out)
    p = np.where(np.isinf(out), 2 * p, p)
    return np.where(np.isnan(out), 3, p).astype(np.int8)


# ---- the high-precision reference and the error model ----------------------------------------------------------------
def _pow0(mp, x, y):
    """x^y for x >= 0 with pow()'s conventions at x = 0"""
    if x == 0:
        return mp.mpf(1) if y == 0 else (mp.mpf(0) if y > 0 else mp.inf)
    return mp.power(x, y)


def mp_reference(rec, dec, i, prec=240):
    """BRDF.cpp's formulas at record i's fp64 inputs in `prec`-bit arithmetic, on the oracle's branches (dec =
    decisions(rec)).  Returns a dict: out (8 mpf, NaN where the formula is 0 / 0), spec_brdf[3] / spec_pdf (the specular
    parts of brdf and pdf), lobe (the scalar lobe value (sh + 1) c^sh / (2 pi) of each, None where its branch is not
    taken) and the quantities the condition numbers use."""
    import mpmath as mp

    mp.mp.prec = prec
    f = lambda x: mp.mpf(float(x))  # noqa: E731
    r = rec[i]
    n, wi, wr, kd, ks = ([f(x) for x in r[3 * k:3 * k + 3]] for k in range(5))
    sh, k1, k2 = f(r[15]), f(r[17]), f(r[18])
    vdot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]  # noqa: E731

    def vnorm(a):  # 0 / 0 = NaN, as in the reference (its frame for an axis of exactly -e_x: axis x e_x = 0)
        l = mp.sqrt(vdot(a, a))
        return [mp.nan] * 3 if l == 0 or mp.isnan(l) else [x / l for x in a]

    vcross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]  # noqa: E731
    vmirror = lambda w, m: [-w[k] + 2 * m[k] * vdot(w, m) for k in range(3)]  # noqa: E731
    nan = mp.nan
    d, s = (kd[0] + kd[1] + kd[2]) / 3, (ks[0] + ks[1] + ks[2]) / 3
    black = d + s == 0
    p0, p1 = (nan, nan) if black else (d / (d + s), s / (d + s))
    res = {}
    # brdf_phong
    c = vdot(wr, vmirror(wi, n))
    lobe_b = None
    if dec["c_pos"][i]:
        lobe_b = (sh + 1) * _pow0(mp, abs(c), sh) / (2 * mp.pi)
    spec_b = [ks[k] * lobe_b if lobe_b is not None else mp.mpf(0) for k in range(3)]
    brdf = [kd[k] / mp.pi + spec_b[k] for k in range(3)]
    # phong_pdf
    ct = vdot(wi, n)
    R = vnorm(vmirror(wr, n))
    cs = vdot(wi, R)
    lobe_p = None
    if not dec["cs_neg"][i]:
        lobe_p = (sh + 1) / (2 * mp.pi) * _pow0(mp, abs(cs), sh)
    if black:
        pdf, spec_p, diff_p = nan, nan, nan
    else:
        diff_p = mp.mpf(0) if dec["ct_neg"][i] else p0 * ct / mp.pi
        spec_p = mp.mpf(0) if lobe_p is None else (p1 * lobe_p if p1 != 0 else mp.mpf(0))  # a zero weight is the skip's case
        pdf = diff_p + spec_p
    # sample_phong
    ind = int(dec["ind"][i])
    if ind == 0:
        x = 1 - 2 * k1
        theta = mp.acos(x) / 2
        axis = n
        carg = x
    else:
        carg = _pow0(mp, k1, 1 / (sh + 1))
        theta = mp.acos(carg)
        axis = R
    st, ctheta = mp.sin(theta), mp.cos(theta)
    if ind == 0:
        spdf = p0 * ctheta / mp.pi if not black else nan
    else:
        spdf = p1 * (sh + 1) / (2 * mp.pi) * _pow0(mp, k1, sh / (sh + 1)) if not black else nan
    phi = 2 * mp.pi * k2
    e = [mp.mpf(1), mp.mpf(0), mp.mpf(0)] if dec["frame_ex"][i] else [mp.mpf(0), mp.mpf(1), mp.mpf(0)]
    ae = vcross(axis, e)
    nx = vnorm(ae)
    ny = vnorm(vcross(axis, nx))
    loc = [st * mp.cos(phi), st * mp.sin(phi), ctheta]
    dirv = vnorm([nx[k] * loc[0] + ny[k] * loc[1] + axis[k] * loc[2] for k in range(3)])
    res["out"] = brdf + [pdf] + dirv + [spdf]
    res.update(spec_brdf=spec_b, spec_pdf=spec_p, diff_pdf=diff_p, lobe_brdf=lobe_b, lobe_pdf=lobe_p, c=c, cs=cs, ct=ct,
               sum_abs_ct=sum(abs(wi[k] * n[k]) for k in range(3)), ind=ind, st=st, carg=carg, k1=k1, sh=sh, black=black,
               pd=p0, frame_r=mp.sqrt(vdot(ae, ae)), weights=(ks, p1))
    return res


# The oracle's own largest normalised errors over subset(generate()), rounded up to a power of two and pinned by
# tests/test_phong_cpu.py (measured 1.84, 0.86, 1.24, 1.40); the GPU test grants the kernels 4 K_REF
K_REF = {"brdf": 2.0, "pdf": 1.0, "dir": 2.0, "spdf": 2.0}
OUTPUTS = ("brdf", "pdf", "dir", "spdf")


def reachable_cells(rec, cls):
    """the (material, lobe) cells a uniform u0 in [0, 1 - 2^-53] can reach: the cosine lobe needs p0 >= 0 (not NaN: a
    black material's weights are 0 / 0), the specular lobe p0 < 1 - 2^-53 (a diffuse-only material never picks it)"""
    p0 = decisions(rec)["p0"]
    cells = []
    for mat in dict.fromkeys(cls["mat"]):
        p = p0[np.argmax(cls["mat"] == mat)]
        cells += [(mat, 0)] if p >= 0 else []
        cells += [(mat, 1)] if not p >= ONE_M else []
    return cells


LOBE_MIN = 1e-290  # a lobe value below this is compared absolutely
ABS_MAX = 1e-280
C_LINEAR = 2.0 ** -40  # below this |c| the lobe is compared as an interval, not by the linear condition number
C_SLACK = 2.0 ** -50  # the absolute error granted to a dot product of unit vectors there (8 * 2^-53)


def _lg(mp, k1):
    return mp.mpf(1075) if k1 == 0 else abs(mp.log(k1, 2))


def conds(ref, variant=0):
    """The condition numbers of the four outputs for one record: the error of an output in units of 2^-53 that an
    evaluation with a few correctly rounded steps may show.  variant 1 adds the BRDF-only kernels' documented terms
    (device_math.h): 2 |sh log2 c| for the exp2 / log2 lobe, and the pow's |log2 k1| / (sh + 1) doubled.

    brdf, pdf   spec * (4 + 4 |sh| / c) + total: the dot product's rounding is amplified by sh / c in c^sh; the sum with
                the diffuse part rounds once more (`total`); the pdf's diffuse part carries its own dot product,
                pd (sum |wi_k n_k| + |ct|) / pi (ct cancels for wi perpendicular to n).  Absolute, in the output's units.
    dir         specular lobe: 4 + (c / max(st, 2^-30)) (1 + |log2 k1| / (sh + 1)): theta = acos(c) moves by dc / st,
                and c = k1^(1/(sh+1)) carries the pow's and the exponent's rounding.  Cosine lobe, by analogy:
                4 + |x| / max(sin 2 theta, 2^-30) with x = 1 - 2 k1 (theta = acos(x) / 2, sin 2 theta = sqrt(1 - x^2)).
                The constant 4 (1 for a frame without rounding) is the frame: two normalisations, two cross products
                and the final normalisation of a unit vector, about an ulp each.  The specular lobe adds 4 st / r, r =
                |axis x e| the length of the frame's first cross product: the mirror axis is a computed unit vector with
                a few 2^-53 of absolute error, which turns nx by that error over r -- r is 4.5e-5 one frame switch
                (1 - axis.x = 1e-9) away from e_x, where the oracle's own directions are off by up to 2 000 * 2^-53.
                The cosine lobe's axis is the input n itself and has no such term.
    sample_pdf  specular lobe: 2 + |log2 k1| (pow(k1, sh / (sh + 1))); cosine lobe: 3 + 2 st / max(ct, 2^-30), the
                chain's angle error (pi / 2 ulps of acos, halved, plus sincos) seen through cos theta.  Relative."""
    import mpmath as mp

    sh = ref["sh"]
    out = ref["out"]

    def spec_cond(c, lobe, fast):
        if lobe is None:
            return mp.mpf(4)
        ac = max(abs(c), mp.mpf(10) ** -300)
        k = 4 + 4 * abs(sh) / ac
        if fast:
            k += 2 * abs(sh * mp.log(ac, 2))
        return k

    cb = spec_cond(ref["c"], ref["lobe_brdf"], variant == 1)  # phong_pdf keeps pow in every kernel
    d_brdf = [cb * abs(ref["spec_brdf"][k]) + abs(out[k]) for k in range(3)]
    if ref["black"]:
        d_pdf = mp.nan
    else:
        d_pdf = (spec_cond(ref["cs"], ref["lobe_pdf"], False) * abs(ref["spec_pdf"]) + abs(out[3]) +
                 2 * ref["pd"] * (ref["sum_abs_ct"] + abs(ref["ct"])) / mp.pi)
    st, k1 = ref["st"], ref["k1"]
    floor = mp.mpf(2) ** -30
    vf = 2 if variant == 1 else 1
    if ref["ind"] == 1:
        d_dir = 4 + abs(ref["carg"]) / max(st, floor) * (1 + vf * _lg(mp, k1) / abs(sh + 1)) + 4 * st / max(ref["frame_r"], floor)
        d_spdf = 2 + vf * _lg(mp, k1)
    else:
        x = ref["carg"]
        d_dir = 4 + abs(x) / max(mp.sqrt(max(1 - x * x, 0)), floor)
        ctheta = mp.sqrt((1 + x) / 2)
        d_spdf = 3 + 2 * st / max(ctheta, floor)
    return d_brdf, d_pdf, d_dir, d_spdf


def normalised_errors(got, ref, cnd):
    """The errors of one record's 8 outputs `got` (float64) against ref = mp_reference(...) in units of 2^-53 * cond
    (cnd = conds(ref, variant)): dict brdf, pdf, dir, spdf, plus `relative` (the brdf / pdf lobes were both compared
    relatively) and `underflow`.  A lobe value below LOBE_MIN is not compared relatively: the output's specular part
    must then be at most ABS_MAX in absolute value.  A NaN or an infinity where the reference has none, or the other
    way round, is an infinite error: nothing is skipped."""
    import mpmath as mp

    out = ref["out"]
    d_brdf, d_pdf, d_dir, d_spdf = cnd
    u = mp.mpf(2) ** -53
    inf = float("inf")

    def special(g, e):
        """None if both finite; else 0 / inf for a matching / mismatching NaN or infinity"""
        gn, en = bool(np.isnan(g)), bool(mp.isnan(e))
        gi, ei = bool(np.isinf(g)), bool(mp.isinf(e))
        if not (gn or en or gi or ei):
            return None
        return 0.0 if (gn == en and gi == ei and (not gi or (g > 0) == (e > 0))) else inf

    def term(g, e, d, lobe, diff, c, w):
        if lobe is not None and abs(c) < C_LINEAR:
            # a dot product within a few ulps of zero has no relative accuracy and sh / c no meaning: the specular
            # part may be anything the lobe takes for a c within C_SLACK of the exact one (infinite for sh < 0 at c = 0)
            sh = ref["sh"]
            v = [(sh + 1) * _pow0(mp, max(abs(c) + sgn * C_SLACK, 0), sh) / (2 * mp.pi) * w for sgn in (-1, 1)]
            lo, hi = diff + min(v), diff + max(v)
            if np.isnan(g) or mp.isnan(lo) or mp.isnan(hi):
                return (0.0 if np.isnan(g) and (mp.isnan(lo) or mp.isnan(hi)) else inf), False
            gm = mp.inf if np.isinf(g) else mp.mpf(float(g))
            out_by = max(lo - gm, gm - hi, 0)
            scale = u * 4 * (abs(diff) + (min(v) if mp.isinf(max(v)) else max(v))) + ABS_MAX
            return (0.0 if out_by == 0 else float(out_by / scale)), False
        sp = special(g, e)
        if sp is not None:
            return sp, False
        if lobe is not None and lobe < LOBE_MIN:  # underflow: the specular part absolutely
            err = max(abs(mp.mpf(float(g)) - diff) - ABS_MAX, 0)
            return (0.0 if err == 0 else (float(err / (u * d)) if d > 0 else inf)), True
        err = max(abs(mp.mpf(float(g)) - e) - ABS_MAX, 0)  # ABS_MAX: products that underflow to denormals or zero
        if err == 0:
            return 0.0, False
        return (float(err / (u * d)) if d > 0 else inf), False

    res = {}
    eb, under = 0.0, False
    for k in range(3):
        diff = out[k] - ref["spec_brdf"][k]
        e, un = term(got[k], out[k], d_brdf[k], ref["lobe_brdf"], diff, ref["c"], ref["weights"][0][k])
        eb, under = max(eb, e), under or un
    res["brdf"] = eb
    e, un = term(got[3], out[3], d_pdf, ref["lobe_pdf"], ref["diff_pdf"], ref["cs"], ref["weights"][1])
    res["pdf"], under = e, under or un
    res["underflow"] = under
    res["relative"] = (ref["lobe_brdf"] is not None and ref["lobe_brdf"] >= LOBE_MIN and ref["lobe_pdf"] is not None and
                       ref["lobe_pdf"] >= LOBE_MIN and abs(ref["c"]) >= C_LINEAR and abs(ref["cs"]) >= C_LINEAR)
    if any(mp.isnan(x) for x in out[4:7]):
        res["dir"] = 0.0 if all(np.isnan(got[4:7])) else inf
    elif any(np.isnan(got[4:7])) or any(np.isinf(got[4:7])):
        res["dir"] = inf
    else:
        dist = mp.sqrt(sum((mp.mpf(float(got[4 + k])) - out[4 + k]) ** 2 for k in range(3)))
        res["dir"] = float(dist / (u * d_dir))
    sp = special(got[7], out[7])
    if sp is not None:
        res["spdf"] = sp
    else:
        err = max(abs(mp.mpf(float(got[7])) - out[7]) - ABS_MAX, 0)
        res["spdf"] = 0.0 if err == 0 else (float(err / (u * d_spdf * abs(out[7]))) if out[7] != 0 else inf)
    return res


def abs_tolerances(ref, cnd, k):
    """What normalised_errors <= k (a dict per output) means in absolute terms for one record: brdf[3], pdf, dir
    (Euclidean) and spdf as floats, infinite where an interval comparison has no upper end -- the terms two evaluations
    of the same record may differ by (tests/test_phong.py compares the two kernel variants with the sum of their two)."""
    import mpmath as mp

    out = ref["out"]
    d_brdf, d_pdf, d_dir, d_spdf = cnd
    u = mp.mpf(2) ** -53

    def fl(x):
        return float("inf") if mp.isnan(x) or mp.isinf(x) else float(x)

    def term(d, lobe, diff, c, w, kk):
        if lobe is not None and abs(c) < C_LINEAR:
            sh = ref["sh"]
            v = [(sh + 1) * _pow0(mp, max(abs(c) + sgn * C_SLACK, 0), sh) / (2 * mp.pi) * w for sgn in (-1, 1)]
            if any(mp.isinf(x) or mp.isnan(x) for x in v):
                return float("inf")
            return fl(max(v) - min(v) + kk * (u * 4 * (abs(diff) + max(v)) + ABS_MAX))
        return fl(kk * u * d + 2 * ABS_MAX)

    res = {"brdf": [term(d_brdf[j], ref["lobe_brdf"], out[j] - ref["spec_brdf"][j], ref["c"], ref["weights"][0][j], k["brdf"])
                    for j in range(3)]}
    res["pdf"] = term(d_pdf, ref["lobe_pdf"], ref["diff_pdf"], ref["cs"], ref["weights"][1], k["pdf"])
    res["dir"] = fl(k["dir"] * u * d_dir)
    res["spdf"] = fl(k["spdf"] * u * d_spdf * abs(out[7]) + ABS_MAX)
    return res
