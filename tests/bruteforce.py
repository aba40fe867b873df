"""The plain reference of the traversal tests: the closest hit over ALL facets by the reference's fp64 Cramer rule
(Myobj.cpp:165-192), in tri_hit's operation order (render.hip: det3 as ((0 + c0 z0) + c1 z1) + c2 z2 of the cross
product's components, no contraction), ties to the lowest facet id.  No tree, no pruning, no fp32: what every traversal
kernel must reproduce bit for bit.  A helper module, imported by the tests."""
import numpy as np

EPS = 1e-8  # MCPT_EPS


def _cross(x, y):
    return (x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1], x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2],
            x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0])


def _det(x, y, z):
    c0, c1, c2 = _cross(x, y)
    return ((0 + c0 * z[..., 0]) + c1 * z[..., 1]) + c2 * z[..., 2]


def accept_all(arrays, ro, rd):
    """(ok, t, beta, gamma), each rays x facets: tri_hit's verdict and values for every (ray, facet) pair"""
    P = arrays["positions"].astype(np.float64).reshape(-1, 3, 3)
    a, ab, ac = P[:, 0], P[:, 0] - P[:, 1], P[:, 0] - P[:, 2]
    ro, rd = np.asarray(ro, np.float64).reshape(-1, 1, 3), np.asarray(rd, np.float64).reshape(-1, 1, 3)
    ar = a[None] - ro
    with np.errstate(all="ignore"):
        dA = _det(ab[None], ac[None], rd)
        be, ga, t = _det(ar, ac[None], rd) / dA, _det(ab[None], ar, rd) / dA, _det(ab[None], ac[None], ar) / dA
        ok = (np.abs(dA) >= EPS) & ~((be < 0) | (ga < 0) | (be + ga > 1) | (t < 0) | (np.abs(t) < EPS))
    return ok, t, be, ga


def brute_force(arrays, ro, rd, exclude=None, light_only=False, chunk=256):
    """(facet, t, beta, gamma) of the closest accepted facet per ray; facet -1 (and zeros) where nothing is hit.
    exclude: a facet id per ray that is skipped (-1: none); light_only: only light facets count."""
    ro, rd = np.asarray(ro, np.float64).reshape(-1, 3), np.asarray(rd, np.float64).reshape(-1, 3)
    n, F = len(ro), len(arrays["positions"])
    ex = np.full(n, -1) if exclude is None else np.asarray(exclude).astype(np.int64)
    # the facets that count, in ascending order (the same values per pair whether or not the others are evaluated)
    ids = np.unique(np.asarray(arrays["light_facet"], np.int64)) if light_only else np.arange(F)
    sub = {"positions": arrays["positions"][ids]}
    col = np.full(F + 1, -1)
    col[ids] = np.arange(len(ids))
    exc = col[ex]  # ex == -1 reads the spare last entry: -1
    facet, out = np.full(n, -1, np.int32), np.zeros((n, 3))
    for s in range(0, n if len(ids) else 0, chunk):
        e = slice(s, min(s + chunk, n))
        ok, t, be, ga = accept_all(sub, ro[e], rd[e])
        rows = np.arange(ok.shape[0])
        has = exc[e] >= 0
        ok[rows[has], exc[e][has]] = False
        best = np.argmin(np.where(ok, t, np.inf), axis=1)  # the first minimum: ties to the lowest facet id
        hit = ok[rows, best]
        facet[e] = np.where(hit, ids[best], -1)
        for k, v in enumerate((t, be, ga)):
            out[e, k] = np.where(hit, v[rows, best], 0.0)
    return facet, out[:, 0], out[:, 1], out[:, 2]
