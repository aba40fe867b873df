"""Every traversal kernel against the fp64 brute force (tests/bruteforce.py), away from the Veach stand-in and away
from the origin: the stress cluster of scenegen.ray_stress at six places and sizes (stresscases.CASES) under five ray
families (scenegen.stress_rays) -- rays at vertices and edges, the renderer's own secondary rays, directions with
exact zeros from origins on box planes, far origins, directions that are not unit length, a NaN direction.  Facets
equal, (t, beta, gamma) bit for bit: the 4-wide fp32 tree (mcpt_closest_hit, mcpt_primary_hits), the 8-wide compressed
tree (wide=True), trees refit and rebuilt on the device after a transform, and -- through renders, the only way to
reach it -- the byte-quantised persistent traversal.  Run on the MI355X box: `pytest -m gpu`.

The inputs' power and a host model of the box tests are tests/test_traversal_stress_cpu.py.

The edited scenes: a transform must stay inside the arena (the build's box grown by its extent, include/mcpt.h), so a
scene cannot be built at the origin and moved 1e2 extents; that transform is refused, which is asserted.  The edit
routes therefore build the scene 0.9 extents (on every axis) away from the case's place and translate it there: the
device refits, or refits and rebuilds, at the case's coordinates."""
import numpy as np
import pytest

import monte_carlo_path_tracing_amd as mcpt
from bruteforce import brute_force
from conftest import NORTH_STAR_TOL, TIGHT_L2, TIGHT_PX
from oracle import pyoracle as po
import scenegen
import stresscases as sc
from test_scene_update_cpu import fresh

pytestmark = pytest.mark.gpu
SEED = 20240430
OFFSET_CASES = ["offset-1e2", "offset-1e3", "offset-1e4"]
SHIFT = (-0.9, 0.9, -0.9)  # where the edit routes build their scene, in extents from the case's place
OMODE = {"mis": po.MODE_MIS, "brdf": po.MODE_BRDF, "shade_area": po.MODE_SHADE_AREA}


def assert_hits(got, want, what):
    f, tbg = got
    wf, wt, wb, wg = want
    hit = wf >= 0
    print("%s: %d of %d rays hit" % (what, hit.sum(), len(wf)))
    assert np.array_equal(f, wf), (what, np.flatnonzero(f != wf)[:10], f[f != wf][:10], wf[f != wf][:10])
    assert np.array_equal(tbg[hit], np.stack([wt, wb, wg], axis=1)[hit]), what  # bit for bit


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("case", list(sc.CASES))
def test_closest_hit_equals_brute_force(case, family):
    """the one-ray-per-thread traversals: trace4_ww over the fp32 nodes and trace_cw8 over the 8-wide compressed
    nodes, over all facets and over the lights only"""
    scene = sc.scene(case)
    ro, rd, ex = sc.rays(case, family)
    for light_only in (False, True):
        want = sc.reference(case, family, light_only)
        for wide in (False, True):
            assert_hits(mcpt.closest_hit(scene, ro, rd, ex, light_only, wide=wide), want,
                        "%s / %s, light_only=%s, wide=%s" % (case, family, light_only, wide))


@pytest.mark.parametrize("case", list(sc.CASES))
def test_primary_hits_equal_brute_force(case):
    """mcpt_primary_hits of the scene's own camera (48 x 36, looking at the cluster) against the brute force over the
    rays mcpt_camera_rays gives for it"""
    scene = sc.scene(case)
    cam = scene.camera()
    cam.width, cam.height = 48, 36
    o, d = mcpt.camera_rays(cam)
    want = brute_force(sc.arrays_of(case), o, d)
    assert (want[0] >= 0).sum() > 300 and len(np.unique(want[0])) > 50  # the camera does see the cluster
    assert_hits(mcpt.primary_hits(scene, cam), want, "%s, primary hits" % case)


# ---- scenes that reach their place by an edit ----
_edited = {}


def edited(case, route):
    """(scene, its arrays, a fresh scene of those arrays): built SHIFT away, translated to the case's place on the
    device (lights included), and for route "rebuild" rebuilt there"""
    if (case, route) not in _edited:
        _, scale = sc.CASES[case]
        scene = mcpt.Scene.load(*sc.files(case, SHIFT))
        scene.set_lights_movable()
        scene.rest_save()
        mcpt.primary_hits(scene, mcpt.Camera.reference(8, 6))  # the device state exists before the transform
        m = np.hstack([np.eye(3), -scale * np.asarray(SHIFT)[:, None]])
        st = scene.transform(0, scene.nfacets, m)
        assert st["device_states"] == 1 and st["nodes_refit"] >= 1, st
        if route == "rebuild":
            rb = scene.rebuild()
            assert rb["device_states"] == 1, rb
        r = mcpt.debug_bvh4_check_device(scene)
        assert r["errors"] == 0 and r["tris"] == r["facets"] == scene.nfacets, r
        with pytest.raises(mcpt.MCPTError, match="8-wide"):  # stale after an update: refused, not traced
            mcpt.closest_hit(scene, np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]]), wide=True)
        arr = scene.arrays()
        lo = arr["positions"].reshape(-1, 3).min(axis=0)
        want = scale * np.asarray(sc.CASES[case][0])
        assert np.allclose(lo, want, rtol=1e-6, atol=1e-3 * scale), (lo, want)  # it is at the case's place
        _edited[case, route] = (scene, arr, fresh(arr))
    return _edited[case, route]


def test_a_translation_beyond_the_arena_is_refused():
    scene = mcpt.Scene.load(*sc.files("origin"))
    scene.set_lights_movable()
    scene.rest_save()
    m = np.hstack([np.eye(3), np.array([[1e2], [-5e1], [2.5e1]])])
    with pytest.raises(mcpt.MCPTError, match="outside the arena"):
        scene.transform(0, scene.nfacets, m)


@pytest.mark.parametrize("family", sc.FAMILIES)
@pytest.mark.parametrize("route", ["refit", "rebuild"])
@pytest.mark.parametrize("case", OFFSET_CASES)
def test_edited_scene_equals_brute_force_and_a_fresh_scene(case, route, family):
    scene, arr, again = edited(case, route)
    ro, rd, ex = scenegen.stress_rays(arr, family)
    for light_only in (False, True):
        want = brute_force(arr, ro, rd, ex, light_only)
        assert_hits(mcpt.closest_hit(scene, ro, rd, ex, light_only), want, "%s by %s / %s, light_only=%s" % (case, route, family, light_only))
        assert_hits(mcpt.closest_hit(again, ro, rd, ex, light_only), want, "%s fresh / %s, light_only=%s" % (case, family, light_only))


# ---- the quantised persistent traversal, through renders ----
def rel_l2(g, c):
    return float(np.linalg.norm(g - c) / max(np.linalg.norm(c), 1e-300))


def max_px_rel(g, c):
    d = np.linalg.norm((g - c).reshape(-1, 3), axis=1)
    n = np.linalg.norm(c.reshape(-1, 3), axis=1)
    return float(np.max(np.where(n > 0, d / np.maximum(n, 1e-300), np.where(d > 0, np.inf, 0.0))))


def gate(g, c, what):
    err, mx = rel_l2(g, c), max_px_rel(g, c)
    print("%s: rel L2 %.3e, max per-pixel %.3e" % (what, err, mx))
    assert np.isfinite(g).all() and (g >= 0).all()
    assert err <= NORTH_STAR_TOL and mx <= NORTH_STAR_TOL, (what, err, mx)
    assert err <= TIGHT_L2 and mx <= TIGHT_PX, (what, err, mx)


@pytest.fixture(scope="module")
def oracle_1e3():
    """the oracle's scene of the offset-1e3 file, its camera (16 x 12) and its grid"""
    o = po.Scene(*sc.files("offset-1e3"))
    c = o.camera()
    assert (c.width, c.height) == (16, 12)
    e, _ = po.camera_ray(c, 0, 0)
    o.build_grid(e)
    return o, c


@pytest.mark.parametrize("mode", ["mis", "shade_area"])
def test_persistent_traversals_render_the_oracle_frame(oracle_1e3, mode):
    """render_rays along the camera's own rays, 16 x 12 at 4 spp, 1e3 extents from the origin: k_mis_rays (default),
    k_rays_persistent over the byte-quantised 4-wide nodes and k_rays_cw8 over the 8-wide ones give one frame, the
    oracle's"""
    o, c = oracle_1e3
    scene = sc.scene("offset-1e3")
    cam = scene.camera()
    org, d = mcpt.camera_rays(cam)
    ref, _ = o.render(c, OMODE[mode], SEED, 4, nthreads=8)
    assert np.isfinite(ref).all() and (ref.reshape(-1, 3).sum(axis=1) > 0).mean() > 0.15  # lit and in view
    frames = {}
    for name, flags in (("default", 0), ("persistent", mcpt.DEBUG_RAYS_PERSIST), ("persistent cw8", mcpt.DEBUG_RAYS_PERSIST | mcpt.DEBUG_RAYS_CW8)):
        g, st = mcpt.render_rays(scene, org, d, 4, mode=mode, seed=SEED, flags=flags)
        frames[name] = g.reshape(cam.height, cam.width, 3)
        gate(frames[name], ref, "%s, %s vs the oracle" % (mode, name))
    for name in ("persistent", "persistent cw8"):
        gate(frames[name], frames["default"], "%s, %s vs default" % (mode, name))


def test_brdf_render_equals_the_oracle_frame(oracle_1e3):
    """mcpt_render in brdf mode (k_extend_brdf's traversal) at the same place"""
    o, c = oracle_1e3
    scene = sc.scene("offset-1e3")
    g, _ = mcpt.render(scene, scene.camera(), 32, mode="brdf", seed=SEED)
    ref, _ = o.render(c, OMODE["brdf"], SEED, 32, nthreads=8)
    assert (ref.reshape(-1, 3).sum(axis=1) > 0).mean() > 0.05
    gate(g, ref, "brdf vs the oracle")
