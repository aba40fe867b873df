"""Movable light triangles on the GPU (mcpt_scene_set_lights_movable, include/mcpt.h): after a light
move the scene behaves as a fresh mcpt_scene_create of the new arrays -- every light table of the device state byte for
byte (mcpt_debug_light_tables), hits and the light prep bit for bit, frames up to the order of the framebuffer's fp64
atomics -- and both refit trees pass the host walk.  Run on the MI355X box: `pytest -m gpu`.

Scenes: light panels of 32 and 66 lights (one chunk; a second chunk of two lights), the Veach stand-in (3 012 lights in
several groups: a whole group, and a sub-range that starts at an odd light index with an odd count, so pair records
are shared with unmoved lights and chunks are partly dirty) and scenegen.sphere_mix (5 200 lights, more than 4 096)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE_OBJ, SCENE_XML, TIGHT_L2, TIGHT_PX
import monte_carlo_path_tracing_amd as mcpt
import scenegen
from test_gpu_parity import max_px_rel, rel_l2
from test_light_update_cpu import group_facets, light_groups
from test_scene_update import read_pfm
from test_scene_update_cpu import fresh, translated
from test_transform_cpu import with_transform

pytestmark = pytest.mark.gpu
SEED = 20240430
W, H, SPP = 16, 12, 3
CLI = os.path.join(ROOT, "monte_carlo_path_tracing_amd", "mcpt_render")
SCENE_BASE = os.path.splitext(str(SCENE_OBJ))[0]
MODES = ("mis", "brdf", "shade", "shade_area")


def sized(cam, w, h):
    c = mcpt.Camera.from_buffer_copy(cam)
    c.width, c.height = w, h
    return c


def with_range(arr, first, new, nrm=None):
    out = {k: v.copy() for k, v in arr.items()}
    out["positions"][first:first + len(new)] = new
    if nrm is not None:
        out["normals"][first:first + len(new)] = nrm
    return out


def lights_of_range(arr, a, b):
    """the light indices of the light facets in [a, b)"""
    lf = arr["light_facet"]
    return np.flatnonzero((lf >= a) & (lf < b))


def dirty_counts(arr, a, b):
    """(lights, distinct 64-light chunks, distinct groups) of the facet range, computed from the arrays"""
    ls = lights_of_range(arr, a, b)
    grp = np.zeros(len(arr["light_facet"]), np.int64)
    for g, (l0, l1) in enumerate(light_groups(arr)):
        grp[l0:l1] = g
    return len(ls), len(np.unique(ls // 64)), len(np.unique(grp[ls]))


class Case:
    """one scene and one light move: the arrays, the moved facet range and its new positions, a camera"""

    def __init__(self, arr, cam, rng_, step):
        self.arr, self.cam, (self.a, self.b) = arr, cam, rng_
        self.new = translated(arr["positions"][self.a:self.b], step)
        self.want = with_range(arr, self.a, self.new)

    def moved(self):
        """a scene that lived on the device before its lights moved"""
        s = fresh(self.arr)
        mcpt.primary_hits(s, sized(self.cam, 8, 6))
        s.set_lights_movable()
        s.update(self.a, self.new)
        return s


def load_case(tmp_path_factory, name):
    if name.startswith("panel"):
        nx, nz = (4, 4) if name == "panel32" else (3, 11)
        obj, xml = scenegen.light_panel(str(tmp_path_factory.mktemp(name)), nx=nx, nz=nz)
    elif name == "sphmix":
        obj, xml = scenegen.sphere_mix(str(tmp_path_factory.mktemp(name)))
    else:
        obj, xml = SCENE_OBJ, SCENE_XML
    loaded = mcpt.Scene.load(obj, xml)
    arr = loaded.arrays()
    cam = mcpt.Camera.reference(W, H) if name.startswith("veach") else loaded.camera()
    groups = light_groups(arr)
    if name == "panel32":
        assert len(arr["light_facet"]) == 32
        return Case(arr, cam, group_facets(arr, 0), (0.3, -0.4, 0.2))
    if name == "panel66":
        assert len(arr["light_facet"]) == 66  # the second chunk holds two lights
        return Case(arr, cam, group_facets(arr, 0), (-0.25, 0.3, 0.4))
    if name == "veach_group":
        assert len(arr["light_facet"]) == 3012 and len(groups) >= 3
        return Case(arr, cam, group_facets(arr, 1), (0.5, 1.25, -0.75))
    if name == "veach_odd":
        a, b = group_facets(arr, 2)
        l0 = groups[2][0]
        first = a + (1 - l0 % 2)  # the facet of the group's first odd light index
        count = 131
        assert first + count < b
        c = Case(arr, cam, (first, first + count), (-0.4, 0.8, 0.6))
        ls = lights_of_range(arr, first, first + count)
        # an odd first light index and an odd count: both end pair records are shared with unmoved lights, and the
        # range neither starts nor ends on a chunk boundary
        assert ls[0] % 2 == 1 and len(ls) % 2 == 1 and ls[0] % 64 != 0 and (ls[-1] + 1) % 64 != 0
        return c
    assert name == "sphmix" and len(arr["light_facet"]) == 5200 and len(groups) == 4
    ext = []
    for g in range(4):
        a, b = group_facets(arr, g)
        p = arr["positions"][a:b].reshape(-1, 3)
        ext.append((p.max(axis=0) - p.min(axis=0)).max())
    return Case(arr, cam, group_facets(arr, int(np.argmin(ext))), (0.6, 0.5, 0.9))  # the smallest sphere


CASES = ("panel32", "panel66", "veach_group", "veach_odd", "sphmix")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """every case with its moved scene and the fresh scene of the same arrays (shared, never modified by a test)"""
    out = {}

    def get(name):
        if name not in out:
            c = load_case(tmp_path_factory, name)
            c.scene, c.ref = c.moved(), fresh(c.want)
            out[name] = c
        return out[name]

    return get


def assert_tables_equal(got_scene, want_scene):
    got, want = mcpt.debug_light_tables(got_scene), mcpt.debug_light_tables(want_scene)
    for k in mcpt.LIGHT_TABLES:
        assert got[k].shape == want[k].shape and got[k].size > 0, k
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, "%s: %d bytes differ, the first at %d" % (k, bad.size, bad[0])


def check_trees(scene):
    r = mcpt.debug_bvh4_check_device(scene)
    assert r["errors"] == 0 and r["tris"] == r["facets"] == scene.nfacets, r
    r = mcpt.debug_bvh4_check_device_light(scene)
    assert r["errors"] == 0 and r["tris"] == r["facets"] == scene.nlights, r


def assert_tight(got, want, what):
    l2, px = rel_l2(got, want), max_px_rel(got, want)
    print("%s: rel L2 %.3e, max pixel %.3e" % (what, l2, px))
    assert l2 <= TIGHT_L2 and px <= TIGHT_PX, (what, l2, px)


def edge_and_vertex_rays(arr, a, b, n=3000, seed=7):
    """test_scene_update's rays: aimed at vertices, edge points and +-ulp targets, a third of them at facets [a, b)"""
    P = arr["positions"].astype(np.float64).reshape(-1, 3, 3)
    rng = np.random.default_rng(seed)
    tri = rng.integers(0, len(P), n)
    tri[::3] = rng.integers(a, b, len(tri[::3]))
    kind = rng.integers(0, 3, n)
    w = rng.random((n, 3))
    w[kind == 0] = np.eye(3)[rng.integers(0, 3, (kind == 0).sum())]
    e = rng.integers(0, 3, n)
    w[(kind == 1), e[kind == 1]] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    target = np.einsum("nk,nkc->nc", w, P[tri])
    target *= 1.0 + rng.choice([0.0, 1e-15, -1e-15, 1e-12, -1e-12], (n, 1))
    lo, hi = P.reshape(-1, 3).min(axis=0), P.reshape(-1, 3).max(axis=0)
    ro = lo + rng.random((n, 3)) * (hi - lo)
    near = rng.random(n) < 0.3
    ro[near] = target[near] + rng.normal(0, 0.05, (near.sum(), 3))
    rd = target - ro
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    ex = np.where(rng.random(n) < 0.2, tri, -1).astype(np.int32)
    return ro, rd, ex


def prep_points(arr, n=2000, seed=11):
    P = arr["positions"].astype(np.float64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    lo, hi = P.min(axis=0), P.max(axis=0)
    x1 = lo + rng.random((n, 3)) * (hi - lo)
    nn = rng.normal(size=(n, 3))
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    return x1, nn, rng.random(n)


@pytest.mark.parametrize("name", CASES)
def test_tables_trees_hits_and_prep_equal_a_fresh_scene(cases, name):
    c = cases(name)
    scene, ref = c.scene, c.ref
    nl, nch, ng = dirty_counts(c.arr, c.a, c.b)
    assert_tables_equal(scene, ref)
    check_trees(scene)
    ro, rd, ex = edge_and_vertex_rays(c.want, c.a, c.b)
    for light_only in (True, False):
        f, tbg = mcpt.closest_hit(scene, ro, rd, ex, light_only=light_only)
        f2, tbg2 = mcpt.closest_hit(ref, ro, rd, ex, light_only=light_only)
        assert np.array_equal(f, f2) and np.array_equal(tbg, tbg2), light_only
        on = (f >= c.a) & (f < c.b)
        print("%s light_only=%s: %d/%d rays hit, %d of them the moved lights" % (name, light_only, (f >= 0).sum(), len(f), on.sum()))
        assert on.sum() > 100
    x1, nn, u = prep_points(c.want)
    got, want = mcpt.light_prep(scene, x1, nn, u), mcpt.light_prep(ref, x1, nn, u)
    for g, w_, what in zip(got, want, ("weights_sum", "count", "pick")):
        assert np.array_equal(g, w_), what
    assert (got[1] > 0).sum() > 100  # the points do see lights
    cam = sized(c.cam, 32, 24)
    for g, w_ in zip(mcpt.primary_hits(scene, cam), mcpt.primary_hits(ref, cam)):
        assert np.array_equal(g, w_)
    # the host copy followed: arrays and both binary trees
    a, b = scene.arrays(), ref.arrays()
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    for light_only in (False, True):
        assert mcpt.debug_bvh4_check(scene, light_only=light_only)["errors"] == 0


@pytest.mark.parametrize("name", CASES)
def test_light_update_info_numbers(cases, name):
    c = cases(name)
    info = c.scene.light_update_info()
    nl, nch, ng = dirty_counts(c.arr, c.a, c.b)
    assert info["lights"] == nl and info["chunks"] == nch and info["groups"] == ng, (info, nl, nch, ng)
    assert info["light_nodes_refit"] >= 1 and info["light_levels"] >= 1 and info["device_seconds"] > 0, info


@pytest.mark.parametrize("name", CASES)
def test_frames_equal_a_fresh_scene(cases, name):
    c = cases(name)
    cam = sized(c.cam, W, H)
    runs = [(m, 0) for m in MODES]
    if name == "veach_group":
        runs += [("mis", mcpt.RENDER_PRECISION_FP32), ("mis", mcpt.RENDER_FRESH_PDF)]
    for mode, flags in runs:
        got = mcpt.render(c.scene, cam, SPP, mode=mode, seed=SEED, flags=flags)[0]
        want = mcpt.render(c.ref, cam, SPP, mode=mode, seed=SEED, flags=flags)[0]
        assert_tight(got, want, "%s moved vs fresh, %s flags %d" % (name, mode, flags))
        assert np.isfinite(got).all() and got.max() > 0


def test_the_move_shows_in_the_frame(cases):
    c = cases("veach_group")
    cam = sized(c.cam, W, H)
    got = mcpt.render(c.scene, cam, SPP, mode="mis", seed=SEED)[0]
    untouched = mcpt.render(fresh(c.arr), cam, SPP, mode="mis", seed=SEED)[0]
    assert rel_l2(got, untouched) > 1e3 * TIGHT_L2


@pytest.mark.parametrize("name", ["panel66", "veach_odd"])
def test_move_and_move_back_gives_the_original_tables(cases, name):
    c = cases(name)
    s = c.moved()
    s.update(c.a, c.arr["positions"][c.a:c.b])
    assert_tables_equal(s, fresh(c.arr))
    check_trees(s)


def test_two_moves_in_a_row(cases):
    c = cases("veach_group")
    s = c.moved()
    a2, b2 = group_facets(c.arr, 0)
    new2 = translated(c.arr["positions"][a2:b2], (-0.3, 0.9, 0.4))
    s.update(a2, new2)
    third = translated(c.new[5:70], (0.2, 0.1, -0.3))  # part of the first range again
    s.update(c.a + 5, third)
    want = with_range(with_range(c.want, a2, new2), c.a + 5, third)
    ref = fresh(want)
    assert_tables_equal(s, ref)
    check_trees(s)
    cam = sized(c.cam, 32, 24)
    for g, w_ in zip(mcpt.primary_hits(s, cam), mcpt.primary_hits(ref, cam)):
        assert np.array_equal(g, w_)


def test_a_device_state_made_after_a_host_only_move(cases):
    """no device state exists at the move: the host half alone (areas, unique normals, the light-only binary tree)
    is what the state is later made from"""
    c = cases("veach_odd")
    s = fresh(c.arr)
    s.set_lights_movable()
    st = s.update(c.a, c.new)
    assert st["device_states"] == 0
    assert_tables_equal(s, c.ref)
    check_trees(s)
    ro, rd, ex = edge_and_vertex_rays(c.want, c.a, c.b, n=1000)
    f, tbg = mcpt.closest_hit(s, ro, rd, ex, light_only=True)
    f2, tbg2 = mcpt.closest_hit(c.ref, ro, rd, ex, light_only=True)
    assert np.array_equal(f, f2) and np.array_equal(tbg, tbg2)


def test_device_form_equals_host_form(cases):
    import torch
    c = cases("veach_odd")
    dev = fresh(c.arr)
    cam = sized(c.cam, 32, 24)
    mcpt.primary_hits(dev, cam)
    dev.set_lights_movable()
    nrm = -c.arr["normals"][c.a:c.b]
    tp, tn = torch.from_numpy(c.new).cuda(), torch.from_numpy(nrm).cuda()
    st = dev.update_device(c.a, len(c.new), tp.data_ptr(), tn.data_ptr())
    assert st["device_states"] == 1
    host = fresh(c.arr)
    mcpt.primary_hits(host, cam)
    host.set_lights_movable()
    host.update(c.a, c.new, nrm)
    assert_tables_equal(dev, host)
    assert_tables_equal(dev, fresh(with_range(c.arr, c.a, c.new, nrm)))
    check_trees(dev)
    a, b = dev.arrays(), host.arrays()
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert dev.light_update_info()["lights"] == host.light_update_info()["lights"] == len(c.new)


def test_rest_save_and_a_rotation_of_a_light_group(cases):
    c = cases("veach_group")
    s = fresh(c.arr)
    cam = sized(c.cam, 32, 24)
    mcpt.primary_hits(s, cam)
    s.set_lights_movable()
    s.rest_save()
    pivot = c.arr["positions"][c.a:c.b].astype(np.float64).reshape(-1, 3).mean(axis=0)
    m = mcpt.transform_rotation((0.2, 1.0, -0.3), 40.0, pivot, (0.3, 0.5, -0.2))
    st = s.transform(c.a, c.b - c.a, m)
    assert st["device_states"] == 1
    pending = s.host_pending()
    assert pending == c.b - c.a  # the host copy is only marked
    want = with_transform(c.arr, (c.a, c.b), m)  # the header's rule restated in numpy
    ref = fresh(want)
    assert_tables_equal(s, ref)
    for g, w_ in zip(mcpt.primary_hits(s, cam), mcpt.primary_hits(ref, cam)):
        assert np.array_equal(g, w_)
    x1, nn, u = prep_points(want, n=500)
    for g, w_ in zip(mcpt.light_prep(s, x1, nn, u), mcpt.light_prep(ref, x1, nn, u)):
        assert np.array_equal(g, w_)
    info = s.light_update_info()
    assert info["lights"] == c.b - c.a and info["groups"] == 1
    assert s.host_pending() == pending  # none of that synced the host
    s.host_sync()
    assert s.host_pending() == 0
    a, b = s.arrays(), ref.arrays()
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    check_trees(s)
    for light_only in (False, True):
        assert mcpt.debug_bvh4_check(s, light_only=light_only)["errors"] == 0


def test_degenerate_lights_are_refused_and_nothing_changes(cases):
    import torch
    c = cases("panel66")
    s = fresh(c.arr)
    cam = sized(c.cam, 32, 24)
    before = mcpt.primary_hits(s, cam)
    tables = mcpt.debug_light_tables(s)
    s.set_lights_movable()
    bad = c.new.copy()
    bad[7, 6:9] = bad[7, 0:3]  # one light collapses to a segment
    with pytest.raises(mcpt.MCPTError, match="light triangles that would be degenerate"):
        s.update_device(c.a, len(bad), torch.from_numpy(bad).cuda().data_ptr())
    with pytest.raises(mcpt.MCPTError, match=r"light triangle %d \(light 7\) would be degenerate" % (c.a + 7)):
        s.update(c.a, bad)
    s.rest_save()
    with pytest.raises(mcpt.MCPTError, match="light triangles that would be degenerate"):
        s.transform(c.a, c.b - c.a, np.zeros((3, 4)))  # the whole panel onto the origin
    assert s.host_pending() == 0 and s.light_update_info()["lights"] == 0
    after = mcpt.primary_hits(s, cam)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    now = mcpt.debug_light_tables(s)
    for k in tables:
        assert np.array_equal(tables[k], now[k]), k
    assert np.array_equal(s.arrays()["positions"], c.arr["positions"])


def test_without_the_switch_a_refusal_leaves_the_hits_alone(cases):
    c = cases("panel32")
    s = fresh(c.arr)
    cam = sized(c.cam, 32, 24)
    before = mcpt.primary_hits(s, cam)
    with pytest.raises(mcpt.MCPTError, match=r"facet %d is a light triangle" % c.a):
        s.update(c.a, c.new)
    after = mcpt.primary_hits(s, cam)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_frame_sequence_frame_after_a_light_move(cases):
    """whatever a render call derives from the light tables is derived again by the next one: a sequence that rendered
    before the move gives, after it, the 8-bit frame a sequence on a fresh scene gives"""
    c = cases("veach_group")
    cam = sized(c.cam, W, H)
    s = fresh(c.arr)
    s.set_lights_movable()
    seq = mcpt.FrameSequence(s, W, H, SPP, denoise=False)
    seq.frame(cam, SEED)
    s.update(c.a, c.new)
    seq.reset()
    got = seq.frame(cam, SEED + 1)
    raw = seq.read("raw")
    seq.close()
    ref_seq = mcpt.FrameSequence(c.ref, W, H, SPP, denoise=False)
    want = ref_seq.frame(cam, SEED + 1)
    raw_want = ref_seq.read("raw")
    ref_seq.close()
    assert_tight(raw, raw_want, "sequence frame after a light move")
    assert np.array_equal(got, want)


def test_cli_move_with_lights_movable(tmp_path, cases):
    c = cases("veach_group")
    spec = "%d:%d:0.5,1.25,-0.75" % (c.a, c.b - c.a)

    def run(tag, *args):
        pfm = str(tmp_path / (tag + ".pfm"))
        r = subprocess.run([CLI, "--scene", SCENE_BASE, "--out", str(tmp_path / (tag + ".bmp")), "--hdr", pfm, "--width", "32",
                            "--height", "24", "--spp", "2", "--frames", "2", *args], capture_output=True, text=True, timeout=120)
        return r, [str(tmp_path / ("%s_%04d.pfm" % (tag, k))) for k in range(2)]

    refused, _ = run("refused", "--move", spec)
    assert refused.returncode != 0 and "is a light triangle" in refused.stderr, refused.stderr
    still, fs = run("still")
    moved, fm = run("moved", "--move", spec, "--lights-movable")
    assert still.returncode == 0 and moved.returncode == 0, (still.stderr, moved.stderr)
    assert "moved facets [%d, %d)" % (c.a, c.b) in moved.stdout
    assert rel_l2(read_pfm(fm[0]), read_pfm(fs[0])) <= 1e-7
    assert rel_l2(read_pfm(fm[1]), read_pfm(fs[1])) > 1e-3
