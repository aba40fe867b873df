"""mcpt_scene_set_visible without a GPU (include/mcpt.h): no device state exists, so only the host half
runs -- the ABI, the mask's round trip, every refusal, the host tree as mcpt_debug_bvh4_check sees it, and the property
the feature rests on: the traversal's fp32 triangle pre-test rejects a triangle collapsed to one vertex for every ray.
The device half is tests/test_visibility.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE_OBJ, SCENE_XML
import monte_carlo_path_tracing_amd as mcpt
from test_scene_update_cpu import check_tree, fresh, non_light_runs, translated

CLI = os.path.join(ROOT, "monte_carlo_path_tracing_amd", "mcpt_render")
SCENE_BASE = os.path.splitext(str(SCENE_OBJ))[0]
PLATE = (36, 48)


@pytest.fixture(scope="module")
def veach_arrays():
    return mcpt.Scene.load(SCENE_OBJ, SCENE_XML).arrays()


def test_abi_of_the_visibility_calls():
    hdr = (ROOT / "include" / "mcpt.h").read_text()
    for name in ("mcpt_scene_set_visible", "mcpt_scene_visibility"):
        assert name in mcpt.EXPORTS and re.search(r"\b%s\s*\(" % name, hdr) and hasattr(mcpt.lib(), name)
    assert int(re.search(r"#define MCPT_VERSION (\d+)", hdr).group(1)) == 20300 == mcpt.lib().mcpt_version()


def test_host_only_round_trip_arrays_and_tree(veach_arrays):
    scene = fresh(veach_arrays)
    before = scene.arrays()
    F = scene.nfacets
    assert scene.hidden_count() == 0 and scene.visible().all() and scene.visible().shape == (F,)
    st = scene.hide(PLATE[0], PLATE[1] - PLATE[0])
    assert st["device_states"] == 0 and st["facets"] == 12 and st["leaf_slots"] >= 12 and st["device_seconds"] == 0.0, st
    want = np.ones(F, bool)
    want[PLATE[0]:PLATE[1]] = False
    assert scene.hidden_count() == 12 and np.array_equal(scene.visible(), want)
    check_tree(scene)
    # hiding a hidden facet and showing a visible one are accepted and change nothing about them
    scene.hide(PLATE[0] + 4, 20)
    want[PLATE[0] + 4:PLATE[0] + 24] = False
    assert scene.hidden_count() == 24 and np.array_equal(scene.visible(), want)
    scene.show(0, PLATE[0] + 2)
    want[:PLATE[0] + 2] = True
    assert scene.hidden_count() == 22 and np.array_equal(scene.visible(), want)
    check_tree(scene)
    # an update of hidden facets stores the values; the tree stays consistent with the collapsed points
    new = translated(before["positions"][PLATE[0]:PLATE[1]], (0.7, 0.9, 0.3))
    scene.update(PLATE[0], new)
    check_tree(scene)
    assert np.array_equal(scene.arrays()["positions"][PLATE[0]:PLATE[1]], new)
    assert scene.hidden_count() == 22
    scene.update(PLATE[0], before["positions"][PLATE[0]:PLATE[1]])
    scene.show(0, 72)
    assert scene.hidden_count() == 0 and scene.visible().all()
    check_tree(scene)
    after = scene.arrays()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert scene.nfacets == F
    with pytest.raises(mcpt.MCPTError, match="8-wide"):  # the first success marked the handle as updated
        mcpt.debug_bvh8_check(scene)


def test_arrays_are_byte_equal_while_hidden(veach_arrays):
    scene = fresh(veach_arrays)
    before = scene.arrays()
    scene.hide(12, 36)
    after = scene.arrays()
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    assert (scene.nfacets, scene.nmaterials, scene.nlights) == (len(before["positions"]), len(before["materials"]),
                                                               len(before["light_facet"]))


def test_every_refusal_leaves_the_scene_unchanged(veach_arrays):
    scene = fresh(veach_arrays)
    before = scene.arrays()
    (a, b), = non_light_runs(before)[:1]
    assert (a, b) == (0, 72)
    L = mcpt.lib()

    def refused(rc, *words):
        assert rc == -1
        msg = L.mcpt_last_error().decode()
        for w in words:
            assert w in msg, msg

    refused(L.mcpt_scene_set_visible(None, 0, 1, 0, None), "NULL scene")
    refused(L.mcpt_scene_visibility(None, None, None), "NULL scene")
    for first, count in ((0, 0), (0, -3), (-1, 2), (scene.nfacets - 1, 2), (scene.nfacets, 1), (0, 2 ** 31 - 1)):
        for vis in (0, 1):
            refused(L.mcpt_scene_set_visible(scene.h, first, count, vis, None), "range")
    st = mcpt.UpdateStats()
    L.mcpt_update_stats_init(C.byref(st))
    st.struct_size -= 8
    refused(L.mcpt_scene_set_visible(scene.h, 0, 2, 0, C.byref(st)), "struct_size")
    # a range that runs into the light triangles: the first one is named, with and without movable lights, and for show too
    for movable in (False, True):
        scene.set_lights_movable(movable)
        for call in (scene.hide, scene.show):
            with pytest.raises(mcpt.MCPTError, match=r"facet %d is a light triangle" % b):
                call(b - 2, 4)
            with pytest.raises(mcpt.MCPTError, match=r"facet %d is a light triangle .*cannot be hidden" % (b + 5)):
                call(b + 5, 1)
    scene.set_lights_movable(False)
    assert scene.hidden_count() == 0 and scene.visible().all()
    after = scene.arrays()
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert mcpt.debug_bvh8_check(scene)["errors"] == 0  # no call succeeded: the 8-wide trees are not refused
    scene.meshing((0.0, 2.0, 15.0), 1000)  # nothing is hidden: the grid is allowed
    # while something is hidden the grid is refused, and allowed again once everything is shown
    scene.hide(3, 1)
    with pytest.raises(mcpt.MCPTError, match="mcpt_scene_meshing is refused while facets are hidden"):
        scene.meshing((0.0, 2.0, 15.0), 1000)
    scene.show(3, 1)
    scene.meshing((0.0, 2.0, 15.0), 1000)


def test_a_collapsed_triangle_is_rejected_by_the_filter_for_every_ray(veach_arrays):
    """What the feature rests on: tri_filter gets ab = ac = 0 for a slot that holds one vertex three times, so its
    verdict is 0 (the fp64 test surely rejects: its determinant is exactly 0) -- through the point, 1e-15 beside it,
    starting on it, and along an axis."""
    rng = np.random.default_rng(28)
    P = veach_arrays["positions"].reshape(-1, 3)
    n = 200000
    v = P[rng.integers(0, len(P), n)].astype(np.float32)
    tri = np.concatenate([v, v, v], axis=1)
    vd = v.astype(np.float64)
    lo, hi = P.min(axis=0).astype(np.float64), P.max(axis=0).astype(np.float64)
    ro = lo + rng.random((n, 3)) * (hi - lo)
    kind = np.arange(n) % 4
    target = vd.copy()
    beside = kind == 1
    target[beside] *= 1.0 + rng.choice([1e-15, -1e-15], (beside.sum(), 1))
    rd = target - ro
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    on = kind == 2  # starting on the point, in a random direction
    ro[on] = vd[on]
    d = rng.normal(size=(on.sum(), 3))
    rd[on] = d / np.linalg.norm(d, axis=1, keepdims=True)
    ax = kind == 3  # axis-parallel, through the point
    axis = rng.integers(0, 3, ax.sum())
    rd[ax] = np.eye(3)[axis] * rng.choice([1.0, -1.0], (ax.sum(), 1))
    ro[ax] = vd[ax] - rd[ax] * rng.uniform(0.1, 20.0, (ax.sum(), 1))
    verdict, _ = mcpt.debug_tri_filter(tri, ro, rd)
    assert verdict.shape == (n,) and not verdict.any(), np.bincount(verdict)


@pytest.mark.parametrize("args,word", [(["--hide", "36"], "FIRST:COUNT"), (["--hide", "36:0"], "FIRST:COUNT"),
                                       (["--show", "36:12:"], "FIRST:COUNT"), (["--hide", "36:12:x"], "FIRST:COUNT"),
                                       (["--hide", "36:12:-1"], "FIRST:COUNT"),
                                       (["--hide", "36:12", "--grid"], "not supported with --grid"),
                                       (["--show", "36:12:1"], "frame 1 is not one of the run's 1"),
                                       (["--frames", "2", "--hide", "36:12:2"], "frame 2 is not one of the run's 2")])
def test_cli_visibility_usage_errors(args, word):
    r = subprocess.run([CLI, "--scene", SCENE_BASE, "--width", "8", "--height", "6", "--spp", "1", *args], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr, (r.returncode, r.stderr)
