"""The traversal stress inputs and the boxes' margin, without a GPU (the GPU half is tests/test_traversal_stress.py).

1. Power of the inputs: the stress scene (scenegen.ray_stress) at every place and size, and every ray family
   (scenegen.stress_rays), judged by the fp64 brute force alone -- enough accepted rays, enough misses, enough hits on
   an edge, enough ties between coincident facets.  Conditions on the generator, not measurements of the library.

2. A host model of the box tests.  For every brute-force hit, every box on the path from the root to a leaf slot of
   the winning facet must pass the traversals' slab tests, or the kernel cannot find the hit.  The boxes are the
   library's own (mcpt_debug_bvh4_host: collapse_bvh4 and quantize_bvh4 of the host tree, the nodes a device gets);
   the slab expressions are restated here in numpy float32, fmaf as an fp64 product and sum rounded once to float32:
   trace4_ww's fma(plane, inv, -(float)ro * inv) on the fp32 nodes and node_tplanes' fma(byte, scale * inv,
   fma(org, inv, -(float)ro * inv)) on the quantised ones, each with tlimit = FLT_MAX and with the winner's own
   tlimit = (float)t * 1.0001f + 1e-5f.  THIS IS A MODEL, NOT THE KERNEL: a necessary condition, evaluated on the
   host; the kernels themselves are compared with the brute force on the GPU.

   With the margin 1e-5 * extent + 1e-6 alone (the library before the coordinate term, same scenes and rays) the model
   loses hits once the coordinates are large against the extent -- hits with a failing box on every path, fp32 form
   (FLT_MAX / own t) and quantised form (FLT_MAX / own t):
       offset-1e3  aimed      2 / 5 and 0 / 0 of 3 146 hits      offset-1e4  aimed    0 / 2 and 0 / 2 of 3 132
       offset-1e3  secondary  0 / 2 and 0 / 2 of 2 656           offset-1e4  scaled   0 / 1 and 0 / 1 of 2 963
       offset-1e3  scaled     0 / 2 and 0 / 0 of 2 973
   and none at the origin, at offset 1e2 or in the small and large scenes.  The margin's coordinate term
    removes every loss."""
import numpy as np
import pytest

import monte_carlo_path_tracing_amd as mcpt
import scenegen
import stresscases as sc

FLT_MAX = np.float32(np.finfo(np.float32).max)
f32 = np.float32


@pytest.mark.parametrize("case", list(sc.CASES))
def test_scene_layout(case):
    """the loader keeps the file's facet order and every facet, the zero-area ones included; the box has the case's
    extent and place; the only lights are the light quad"""
    s, arr, R = sc.scene(case), sc.arrays_of(case), scenegen.stress_ranges()
    off, scale = sc.CASES[case]
    assert s.nfacets == R["light"][1] == sum(n for _, n in scenegen.STRESS_GROUPS)
    assert sorted(int(f) for f in arr["light_facet"]) == list(range(*R["light"]))
    P = arr["positions"].astype(np.float64).reshape(-1, 3, 3)
    lo, hi = P.reshape(-1, 3).min(axis=0), P.reshape(-1, 3).max(axis=0)
    assert np.allclose(lo, scale * np.asarray(off), rtol=1e-6, atol=1e-6 * scale)
    assert np.allclose(hi - lo, scale, rtol=1e-3)
    area2 = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
    d0, d1 = R["degenerate"]
    # collinear: zero up to the float32 rounding of the vertices, edge (< 0.1 extents) times a unit in the last place
    assert (area2[d0:d1] <= 0.1 * scale * np.spacing(np.abs(arr["positions"]).max())).all()
    assert (area2[d0 + 4:d1] == 0).all()                 # a repeated vertex: exactly zero
    c0, c1 = R["coincident"]
    assert np.array_equal(np.sort(P[c0:c1:2].reshape(-1, 3, 3), axis=1), np.sort(P[c0 + 1:c1:2].reshape(-1, 3, 3), axis=1))
    r = mcpt.debug_bvh4_check(s)
    assert r["errors"] == 0 and r["tris"] == r["facets"] == s.nfacets, r


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("case", list(sc.CASES))
def test_power_of_the_inputs(case, family):
    ro, rd, ex = sc.rays(case, family)
    f, t, be, ga = sc.reference(case, family)
    assert len(ro) == scenegen.STRESS_RAYS == 4096 + 37 and np.isnan(rd[-1]).all() and f[-1] == -1
    hit = f >= 0
    edge = hit & (np.minimum(np.minimum(be, ga), 1.0 - be - ga) <= 1e-9)
    nties = sc.ties(case, family)
    print("%s / %s: %d accepted, %d miss, %d on an edge, %d ties" % (case, family, hit.sum(), (~hit).sum(), edge.sum(), nties))
    assert hit.sum() >= 1000 and (~hit).sum() >= 500 and edge.sum() >= 200 and nties >= 20
    if family == "axis":
        assert ((rd[:-1] == 0).sum(axis=1) >= 1).all() and np.signbit(rd[:-1][rd[:-1] == 0]).any()
        R = scenegen.stress_ranges()
        V = sc.arrays_of(case)["positions"][R["lattice"][0]:R["coincident"][0] + 32].astype(np.float64).reshape(-1, 3)
        for a in range(3):  # every origin coordinate is the coordinate of a lattice vertex
            assert np.isin(ro[:-1, a], V[:, a]).all()
    if family == "scaled":
        n = np.linalg.norm(rd[:-1], axis=1)
        assert np.allclose(n[:len(n) // 2], 1e-3) and np.allclose(n[len(ro) // 2:], 1e3)


# ---- the host model of the box tests ----
def fma32(a, b, c):
    """fmaf(a, b, c) of float32 arrays: the product is exact in fp64, the sum rounds once there, then once to float32"""
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def slot_paths(nodes):
    """for every leaf slot the (node, child) pairs from its leaf up to the root, padded: pn, pk [slots, depth] and
    their validity"""
    parent, owner = {}, {}
    child, count = nodes["child"], nodes["count"]
    for n in range(len(nodes)):
        for k in range(4):
            c = int(child[n, k])
            if c == mcpt.BVH4_EMPTY:
                continue
            if c >= 0:
                parent[c] = (n, k)
            else:
                for s in range(~c, ~c + int(count[n, k])):
                    owner[s] = (n, k)
    paths = []
    for s in range(max(owner) + 1):
        p, at = [], owner[s]
        while True:
            p.append(at)
            if at[0] == 0:
                break
            at = parent[at[0]]
        paths.append(p)
    depth = max(len(p) for p in paths)
    pn, pk = np.zeros((len(paths), depth), np.int64), np.zeros((len(paths), depth), np.int64)
    valid = np.zeros((len(paths), depth), bool)
    for s, p in enumerate(paths):
        pn[s, :len(p)], pk[s, :len(p)], valid[s, :len(p)] = [x[0] for x in p], [x[1] for x in p], True
    return pn, pk, valid


def ray_frame(ro, rd):
    """inv and (float)ro * inv as every traversal computes them"""
    f = rd.astype(np.float32)
    f = np.where(np.abs(f) < f32(1e-30), np.copysign(f32(1e-30), f), f).astype(np.float32)
    inv = (f32(1.0) / f).astype(np.float32)
    return inv, (ro.astype(np.float32) * inv).astype(np.float32)


def slabs_fp32(nodes, pn, pk, inv, oi, tlimit):
    """trace4_ww's test of the boxes (pn, pk) [rays, depth]"""
    lo, hi = nodes["lo"][pn, :, pk], nodes["hi"][pn, :, pk]  # [rays, depth, axis]
    a, b = fma32(lo, inv[:, None], -oi[:, None]), fma32(hi, inv[:, None], -oi[:, None])
    tn, tf = np.minimum(a, b), np.maximum(a, b)
    t0 = np.maximum(np.maximum(tn[..., 0], tn[..., 1]), np.maximum(tn[..., 2], f32(0)))
    t1 = np.minimum(np.minimum(tf[..., 0], tf[..., 1]), np.minimum(tf[..., 2], tlimit[:, None]))
    with np.errstate(over="ignore"):
        return t0 <= (t1 * f32(1.00001)).astype(np.float32) + f32(1e-6)


def slabs_quantised(qnodes, pn, pk, inv, oi, tlimit):
    """node_tplanes' planes and k_rays_persistent's test of the boxes (pn, pk) [rays, depth]"""
    org = qnodes["org"][pn]  # [rays, depth, axis]
    ex = qnodes["ex"][pn]
    q = qnodes["q"][pn]
    sh = (8 * pk).astype(np.uint32)
    tn, tf = [], []
    for a in range(3):
        scale = (((ex >> np.uint32(8 * a)) & np.uint32(0xff)) << np.uint32(23)).astype(np.uint32).view(np.float32)
        with np.errstate(over="ignore"):
            m = (scale * inv[:, None, a]).astype(np.float32)
        b = fma32(org[..., a], inv[:, None, a], -oi[:, None, a])
        ql = ((q[..., 2 * a] >> sh) & np.uint32(0xff)).astype(np.float32)
        qh = ((q[..., 2 * a + 1] >> sh) & np.uint32(0xff)).astype(np.float32)
        neg = (inv[:, None, a] < 0)
        tn.append(fma32(np.where(neg, qh, ql), m, b))
        tf.append(fma32(np.where(neg, ql, qh), m, b))
    t0 = np.maximum(np.maximum(tn[0], tn[1]), np.maximum(tn[2], f32(0)))
    t1 = np.minimum(np.minimum(tf[0], tf[1]), np.minimum(tf[2], tlimit[:, None]))
    return t0 <= fma32(t1, f32(1.00001), f32(1e-6))


def lost_hits(case, family, tree):
    """per (form, limit): the brute-force hits no leaf slot of whose facet has a path of passing boxes"""
    nodes, qnodes, leaf_facets, pn, pk, valid = tree
    ro, rd, _ = sc.rays(case, family)
    f, t, _, _ = sc.reference(case, family)
    hit = np.flatnonzero(f >= 0)
    inv, oi = ray_frame(ro[hit], rd[hit])
    assert np.isfinite(inv).all() and np.isfinite(oi).all()
    with np.errstate(over="ignore"):
        own = (t[hit].astype(np.float32) * f32(1.0001)).astype(np.float32) + f32(1e-5)
    limits = {"FLT_MAX": np.full(len(hit), FLT_MAX), "own t": own}
    order = np.argsort(leaf_facets, kind="stable")
    first = np.searchsorted(leaf_facets[order], f[hit], "left")
    nslots = np.searchsorted(leaf_facets[order], f[hit], "right") - first
    assert (nslots >= 1).all()
    out = {}
    for form, test in (("fp32", lambda n, k, lim: slabs_fp32(nodes, n, k, inv, oi, lim)),
                       ("quantised", lambda n, k, lim: slabs_quantised(qnodes, n, k, inv, oi, lim))):
        for name, lim in limits.items():
            found = np.zeros(len(hit), bool)
            for j in range(int(nslots.max())):  # a facet with spatial-split references has several slots
                s = order[np.minimum(first + j, len(order) - 1)]
                ok = (test(pn[s], pk[s], lim) | ~valid[s]).all(axis=1)
                found |= ok & (j < nslots)
            out[form, name] = int((~found).sum())
    return out, len(hit)


@pytest.fixture(scope="module")
def trees():
    cache = {}

    def get(case):
        if case not in cache:
            nodes, qnodes, lf = mcpt.debug_bvh4_host(sc.scene(case))
            cache[case] = (nodes, qnodes, lf) + slot_paths(nodes)
        return cache[case]
    return get


def test_host_tree_is_the_checked_tree():
    """mcpt_debug_bvh4_host hands out the tree mcpt_debug_bvh4_check walks: its node count, every facet in a slot"""
    s = sc.scene("origin")
    nodes, qnodes, lf = mcpt.debug_bvh4_host(s)
    r = mcpt.debug_bvh4_check(s)
    assert len(nodes) == len(qnodes) == r["nodes"] and len(lf) == r["tris"] + r["duplicates"]
    assert np.array_equal(np.unique(lf), np.arange(s.nfacets))
    assert np.array_equal(nodes["child"] == mcpt.BVH4_EMPTY, qnodes["child"] == mcpt.BVH4_EMPTY)
    ln, lq, llf = mcpt.debug_bvh4_host(s, light_only=True)
    assert len(ln) == mcpt.debug_bvh4_check(s, True)["nodes"] and sorted(llf) == sorted(s.arrays()["light_facet"])


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("case", list(sc.CASES))
def test_every_box_on_the_winning_path_passes_the_model(trees, case, family):
    """A MODEL of the kernels' box tests, not the kernels (see the module's docstring): necessary for the hit"""
    lost, nhit = lost_hits(case, family, trees(case))
    print("%s / %s: %d hits; lost %s" % (case, family, nhit, lost))
    assert all(v == 0 for v in lost.values()), (nhit, lost)
