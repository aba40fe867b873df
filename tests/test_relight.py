"""In-place re-lighting on the GPU (mcpt_scene_set_light_radiance, mcpt_scene_set_materials; include/mcpt.h, DESIGN.md
§4.24): after an edit the scene behaves as a fresh mcpt_scene_create of the edited arrays WITH THE SCENE'S GROUPING
PASSED EXPLICITLY -- every table of RELIGHT_TABLES byte for byte (mcpt_debug_light_tables), the light prep bit for bit,
frames up to the order of the framebuffer's fp64 atomics.  Run on the MI355X box: `pytest -m gpu`.

Scenes (test_light_update's): light panels of 32 and 66 lights (one chunk and one group; a second chunk of two lights),
the Veach stand-in (3 012 lights, 5 groups) and scenegen.sphere_mix (5 200 lights, more than 4 096, 4 groups).  Every
edited scene has been on the device before the edit.  Frames are 16 x 12 at 3 spp."""
import gc
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE_OBJ, SCENE_XML
import monte_carlo_path_tracing_amd as mcpt
import scenegen
from test_gpu_parity import rel_l2
from test_light_update import (H, MODES, SEED, SPP, W, assert_tight, check_trees, edge_and_vertex_rays, prep_points, sized,
                               with_range)
from test_light_update_cpu import group_facets, light_groups
from test_relight_cpu import fresh_grouped, group_index, with_materials, with_radiance
from test_scene_update import read_pfm
from test_scene_update_cpu import fresh, translated

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "monte_carlo_path_tracing_amd", "mcpt_render")
SCENE_BASE = os.path.splitext(str(SCENE_OBJ))[0]


def on_device(arr, cam):
    """a scene that lives on the device (inferred groups: the runs of equal radiance of the ORIGINAL arrays)"""
    s = fresh(arr)
    mcpt.primary_hits(s, sized(cam, 8, 6))
    return s


def assert_tables_equal(got_scene, want_scene, tables=None):
    tables = mcpt.RELIGHT_TABLES if tables is None else tables
    got, want = mcpt.debug_light_tables(got_scene, tables), mcpt.debug_light_tables(want_scene, tables)
    for k in tables:
        assert got[k].shape == want[k].shape and got[k].size > 0, k
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, "%s: %d bytes differ, the first at %d" % (k, bad.size, bad[0])


def band(scene):
    """(band_S, band_K) the state passes to its kernels"""
    g = mcpt.debug_light_tables(scene, "globals")
    return tuple(np.frombuffer(g.tobytes()[:48], np.float64)[4:6])


def expected_counts(gi, first, n):
    """(lights, chunks, groups) of a radiance call from the arrays: the 64-light chunks of the range, and the groups
    whose first light is in it"""
    ls = np.arange(first, first + n)
    starts = np.flatnonzero(np.diff(np.concatenate([[-1], gi])) != 0)
    return n, len(np.unique(ls // 64)), int(np.isin(starts, ls).sum())


class Case:
    """one scene and its radiance edits [(first light, n x 3 radiances)], applied in order"""

    def __init__(self, arr, cam, edits):
        self.arr, self.cam, self.edits = arr, cam, [(int(f), np.asarray(r, np.float64).reshape(-1, 3)) for f, r in edits]
        self.gi = group_index(arr)
        self.want = arr
        for f, r in self.edits:
            self.want = with_radiance(self.want, f, r)

    def edited(self):
        s = on_device(self.arr, self.cam)
        self.stats = [s.set_light_radiance(f, r) for f, r in self.edits]
        return s


def load_arrays(tmp_path_factory, name):
    if name.startswith("panel"):
        nx, nz = (4, 4) if name == "panel32" else (3, 11)
        obj, xml = scenegen.light_panel(str(tmp_path_factory.mktemp(name)), nx=nx, nz=nz)
    elif name == "sphmix":
        obj, xml = scenegen.sphere_mix(str(tmp_path_factory.mktemp(name)))
    else:
        obj, xml = SCENE_OBJ, SCENE_XML
    loaded = mcpt.Scene.load(obj, xml)
    return loaded.arrays(), (mcpt.Camera.reference(W, H) if name == "veach" else loaded.camera())


def make_case(scenes, name):
    rng = np.random.default_rng(3)
    if name == "panel32_group":  # one chunk, one group, all of it
        arr, cam = scenes("panel32")
        assert len(arr["light_radiance"]) == 32
        return Case(arr, cam, [(0, np.tile((5.0, 3.0, 1.0), (32, 1)))])
    if name == "panel66_tail":  # an odd first index and an odd count across the chunk boundary; the group's first light stays
        arr, cam = scenes("panel66")
        assert len(arr["light_radiance"]) == 66
        return Case(arr, cam, [(63, rng.random((3, 3)) * 4.0)])
    if name == "veach_group":  # a whole group
        arr, cam = scenes("veach")
        l0, l1 = light_groups(arr)[1]
        return Case(arr, cam, [(l0, np.tile((7.0, 5.0, 3.0), (l1 - l0, 1)))])
    if name == "veach_odd":
        # an odd first light and an odd count inside group 2, starting and ending inside chunks, all dimmer than the
        # group was: the partly dirty chunks keep S, K maxima that come from untouched lights, the whole ones fall
        arr, cam = scenes("veach")
        l0, l1 = light_groups(arr)[2]
        first, n = l0 + (1 - l0 % 2), 131
        assert first % 2 == 1 and first % 64 != 0 and (first + n) % 64 != 0 and first + n < l1 and first > l0
        assert (first + n - 1) // 64 - first // 64 >= 2  # at least one chunk wholly inside
        return Case(arr, cam, [(first, arr["light_radiance"][first:first + n] * rng.uniform(0.1, 0.5, (n, 3)))])
    if name == "veach_brightest":
        # one light made by far the brightest of the scene, then dimmed below its chunk's others: its chunk's S and
        # band_S must come down again
        arr, cam = scenes("veach")
        return Case(arr, cam, [(1000, [(4000.0, 4000.0, 4000.0)]), (1000, [(0.125, 0.25, 0.125)])])
    arr, cam = scenes("sphmix")
    groups = light_groups(arr)
    assert len(arr["light_radiance"]) == 5200 and len(groups) == 4
    if name == "sphmix_zero":  # one group switched off while the others stay lit
        l0, l1 = groups[2]
        return Case(arr, cam, [(l0, np.zeros((l1 - l0, 3)))])
    assert name == "sphmix_equal"  # two neighbouring groups given one radiance: they must not merge
    (a0, a1), (b0, b1) = groups[0], groups[1]
    assert a1 == b0
    return Case(arr, cam, [(a0, np.tile((5.0, 5.0, 5.0), (a1 - a0, 1))), (b0, np.tile((5.0, 5.0, 5.0), (b1 - b0, 1)))])


CASES = ("panel32_group", "panel66_tail", "veach_group", "veach_odd", "veach_brightest", "sphmix_zero", "sphmix_equal")


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    out = {}

    def get(name):
        if name not in out:
            out[name] = load_arrays(tmp_path_factory, name)
        return out[name]

    return get


@pytest.fixture(scope="module")
def cases(scenes):
    """every case with its edited scene and the fresh scene of the rule (shared, never modified by a test)"""
    out = {}

    def get(name):
        if name not in out:
            c = make_case(scenes, name)
            c.scene, c.ref = c.edited(), fresh_grouped(c.want, c.gi)
            out[name] = c
        return out[name]

    return get


@pytest.fixture(scope="module")
def veach_frames(scenes):
    """the untouched stand-in's frames in the four modes"""
    arr, cam = scenes("veach")
    s = fresh(arr)
    return {m: mcpt.render(s, sized(cam, W, H), SPP, mode=m, seed=SEED)[0] for m in MODES}


@pytest.mark.parametrize("name", CASES)
def test_tables_prep_and_arrays_equal_a_fresh_scene(cases, name):
    c = cases(name)
    assert np.array_equal(c.scene.light_groups(), c.gi) and np.array_equal(c.ref.light_groups(), c.gi)
    assert_tables_equal(c.scene, c.ref)
    x1, nn, u = prep_points(c.want)
    got, want = mcpt.light_prep(c.scene, x1, nn, u), mcpt.light_prep(c.ref, x1, nn, u)
    for g, w_, what in zip(got, want, ("weights_sum", "count", "pick")):
        assert np.array_equal(g, w_), what
    assert (got[1] > 0).sum() > 100  # the points do see lights
    a, b = c.scene.arrays(), c.ref.arrays()
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a["light_radiance"], c.want["light_radiance"])


@pytest.mark.parametrize("name", CASES)
def test_stats_are_the_counts_of_the_arrays(cases, name):
    c = cases(name)
    for (first, rad), st in zip(c.edits, c.stats):
        nl, nch, ng = expected_counts(c.gi, first, len(rad))
        assert (st["lights"], st["chunks"], st["groups"], st["materials"], st["device_states"]) == (nl, nch, ng, 0, 1), st
        assert st["device_seconds"] > 0, st
        print("%s: %d lights, %d chunks, %d groups: %.3f ms device" % (name, nl, nch, ng, st["device_seconds"] * 1e3))


def test_the_inferred_grouping_would_differ(cases):
    """why the rule names the grouping: the radiances alone give other groups than the scene keeps"""
    for name in ("panel66_tail", "sphmix_equal"):
        c = cases(name)
        inferred = fresh(c.want)
        assert not np.array_equal(inferred.light_groups(), c.gi)
        assert mcpt.debug_light_tables(inferred, "grp_sum").shape != mcpt.debug_light_tables(c.scene, "grp_sum").shape


def test_band_constants_fall_when_the_brightest_light_is_dimmed(cases, scenes):
    c = cases("veach_brightest")
    arr, cam = scenes("veach")
    s = on_device(arr, cam)
    s0, k0 = band(s)
    s.set_light_radiance(*c.edits[0])
    s1, k1 = band(s)
    sk1 = np.frombuffer(mcpt.debug_light_tables(s, "chunk_sk").tobytes(), np.float32).reshape(-1, 2)[1000 // 64]
    s.set_light_radiance(*c.edits[1])
    s2, k2 = band(s)
    sk2 = np.frombuffer(mcpt.debug_light_tables(s, "chunk_sk").tobytes(), np.float32).reshape(-1, 2)[1000 // 64]
    print("band_S %.6g -> %.6g -> %.6g, band_K %.6g -> %.6g -> %.6g" % (s0, s1, s2, k0, k1, k2))
    # S comes back to the value the group's other lights give.  The scene's K (sum / shortest edge) is held by a light
    # with a far shorter edge, so band_K need not move; the chunk's own K, below, must
    assert s1 == 12000.0 * (1 + 1e-6) and s1 > s0 and s2 == s0 and k1 >= k0 and k2 == k0
    assert sk2[0] < sk1[0] and sk2[1] < sk1[1]
    assert_tables_equal(s, c.ref)


@pytest.mark.parametrize("name", ["panel32_group", "veach_odd"])
def test_hits_are_unchanged_by_a_relight(cases, name):
    c = cases(name)
    untouched = fresh(c.arr)
    lf = np.sort(c.arr["light_facet"])
    ro, rd, ex = edge_and_vertex_rays(c.arr, int(lf[0]), int(lf[-1]) + 1)
    for light_only in (True, False):
        f, tbg = mcpt.closest_hit(c.scene, ro, rd, ex, light_only=light_only)
        f2, tbg2 = mcpt.closest_hit(untouched, ro, rd, ex, light_only=light_only)
        assert np.array_equal(f, f2) and np.array_equal(tbg, tbg2), light_only
        assert (f >= 0).sum() > 100
    check_trees(c.scene)


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
        assert_tight(got, want, "%s re-lit vs fresh, %s flags %d" % (name, mode, flags))
        assert np.isfinite(got).all() and got.max() > 0


def test_the_relight_shows_in_the_frame(cases, veach_frames):
    c = cases("veach_group")
    got = mcpt.render(c.scene, sized(c.cam, W, H), SPP, mode="mis", seed=SEED)[0]
    assert rel_l2(got, veach_frames["mis"]) > 1e-3


def test_doubling_every_radiance_doubles_the_frame(scenes, veach_frames):
    """a scale by a power of two is exact through the whole chain and leaves the pick's ratios alone"""
    arr, cam = scenes("veach")
    s = on_device(arr, cam)
    s.set_light_radiance(0, 2.0 * arr["light_radiance"])
    for mode in MODES:
        got = mcpt.render(s, sized(cam, W, H), SPP, mode=mode, seed=SEED)[0]
        assert_tight(got, 2.0 * veach_frames[mode], "doubled radiances, %s" % mode)


@pytest.mark.parametrize("rows", ["one", "all"])
def test_materials_equal_a_fresh_scene(scenes, rows):
    arr, cam = scenes("veach")
    M = len(arr["materials"])
    assert M >= 3
    rng = np.random.default_rng(9)
    if rows == "one":
        first, new = 1, np.array([[0.0, 0.0, 0.0, 0.4, 0.0, 0.3, 25.0]], np.float32)  # Kd = 0 and a zero Ks channel
    else:
        first, new = 0, np.concatenate([rng.random((M, 6)) * 0.45, rng.uniform(1.0, 80.0, (M, 1))], axis=1).astype(np.float32)
        new[0, :3] = 0.0  # a row with Kd = 0
        new[2, 4] = 0.0   # and one with a zero Ks channel
    s = on_device(arr, cam)
    before = mcpt.render(s, sized(cam, W, H), SPP, mode="mis", seed=SEED)[0]
    st = s.set_materials(first, new)
    assert (st["lights"], st["chunks"], st["groups"], st["materials"], st["device_states"]) == (0, 0, 0, len(new), 1), st
    want = with_materials(arr, first, new)
    ref = fresh_grouped(want, group_index(arr))
    assert_tables_equal(s, ref)
    assert np.array_equal(s.arrays()["materials"], want["materials"])
    for mode in MODES:
        got = mcpt.render(s, sized(cam, W, H), SPP, mode=mode, seed=SEED)[0]
        assert_tight(got, mcpt.render(ref, sized(cam, W, H), SPP, mode=mode, seed=SEED)[0], "%s rows of materials, %s" % (rows, mode))
        if mode == "mis":
            assert rel_l2(got, before) > 1e-3  # the edit shows


@pytest.mark.parametrize("name", ["panel66_tail", "veach_odd", "sphmix_zero"])
def test_edit_and_edit_back_gives_the_original_tables(cases, name):
    c = cases(name)
    s = c.edited()
    for first, rad in reversed(c.edits):
        s.set_light_radiance(first, c.arr["light_radiance"][first:first + len(rad)])
    assert_tables_equal(s, fresh(c.arr))


def test_two_edits_in_a_row_equal_the_combined_edit(cases):
    c = cases("veach_odd")
    (first, rad), = c.edits
    l0, l1 = light_groups(c.arr)[1]
    whole = np.tile((3.0, 1.0, 2.0), (l1 - l0, 1))
    again = rad[20:81] * 3.0  # part of the first range again
    two = c.edited()
    two.set_light_radiance(l0, whole)
    two.set_light_radiance(first + 20, again)
    want = with_radiance(with_radiance(c.want, l0, whole), first + 20, again)
    # the combined edit: one call over the span of all three
    a, b = min(l0, first), max(l1, first + len(rad))
    one = on_device(c.arr, c.cam)
    one.set_light_radiance(a, want["light_radiance"][a:b])
    assert_tables_equal(two, one)
    assert_tables_equal(two, fresh_grouped(want, c.gi))


def test_device_form_equals_host_form(cases):
    import torch
    c = cases("veach_odd")
    (first, rad), = c.edits
    dev = on_device(c.arr, c.cam)
    t = torch.from_numpy(rad.copy()).cuda()
    st = dev.set_light_radiance_device(first, len(rad), t.data_ptr())
    assert (st["lights"], st["device_states"]) == (len(rad), 1) and st["chunks"] == c.stats[0]["chunks"], st
    assert_tables_equal(dev, c.scene)
    assert_tables_equal(dev, c.ref)
    a, b = dev.arrays(), c.scene.arrays()
    for k in b:
        assert np.array_equal(a[k], b[k]), k
    assert dev.host_pending() == 0


@pytest.mark.parametrize("value", [-1.0, float("nan"), float("inf")])
def test_device_form_refuses_a_bad_value_and_changes_nothing(cases, value):
    import torch
    c = cases("veach_odd")
    (first, rad), = c.edits
    s = on_device(c.arr, c.cam)
    tables = mcpt.debug_light_tables(s, mcpt.RELIGHT_TABLES)
    bad = rad.copy()
    bad[57, 1] = value
    with pytest.raises(mcpt.MCPTError, match=r"1 radiance components of lights \[%d, %d\) are negative or not finite" % (first, first + len(rad))):
        s.set_light_radiance_device(first, len(bad), torch.from_numpy(bad).cuda().data_ptr())
    host = np.zeros((4, 3))
    with pytest.raises(mcpt.MCPTError, match="dev_rgb"):  # host memory is not device memory
        s.set_light_radiance_device(first, 4, host.ctypes.data)
    now = mcpt.debug_light_tables(s, mcpt.RELIGHT_TABLES)
    for k in tables:
        assert np.array_equal(tables[k], now[k]), k
    a = s.arrays()
    for k, v in c.arr.items():
        assert a[k].tobytes() == v.tobytes(), k


def test_a_device_state_made_after_a_host_only_relight(cases, scenes):
    c = cases("sphmix_equal")
    s = fresh(c.arr)
    for first, rad in c.edits:
        assert s.set_light_radiance(first, rad)["device_states"] == 0
    mtl = c.arr["materials"].copy()
    mtl[0, :3] = (0.1, 0.6, 0.2)
    assert s.set_materials(0, mtl[:1])["device_states"] == 0
    ref = fresh_grouped(with_materials(c.want, 0, mtl[:1]), c.gi)
    assert_tables_equal(s, ref)
    cam = sized(c.cam, W, H)
    assert_tight(mcpt.render(s, cam, SPP, mode="shade_area", seed=SEED)[0], mcpt.render(ref, cam, SPP, mode="shade_area", seed=SEED)[0],
                 "state made after a host-only re-light")


@pytest.mark.parametrize("order", ["move_then_relight", "relight_then_move"])
def test_together_with_a_light_move(scenes, order):
    arr, cam = scenes("veach")
    gi = group_index(arr)
    a, b = group_facets(arr, 1)
    l0, l1 = light_groups(arr)[1]
    new = translated(arr["positions"][a:b], (0.5, 1.25, -0.75))
    rad = np.tile((6.0, 2.0, 9.0), (l1 - l0, 1))
    s = on_device(arr, cam)
    s.set_lights_movable()
    if order == "move_then_relight":
        s.update(a, new)
        s.set_light_radiance(l0, rad)
    else:
        s.set_light_radiance(l0, rad)
        s.update(a, new)
    want = with_radiance(with_range(arr, a, new), l0, rad)
    ref = fresh_grouped(want, gi)
    assert_tables_equal(s, ref)
    check_trees(s)
    x1, nn, u = prep_points(want, n=500)
    for g, w_ in zip(mcpt.light_prep(s, x1, nn, u), mcpt.light_prep(ref, x1, nn, u)):
        assert np.array_equal(g, w_)
    assert_tight(mcpt.render(s, sized(cam, W, H), SPP, mode="mis", seed=SEED)[0],
                 mcpt.render(ref, sized(cam, W, H), SPP, mode="mis", seed=SEED)[0], order)
    x = s.arrays()
    for k, v in ref.arrays().items():
        assert np.array_equal(x[k], v), k


def test_a_relight_without_a_move_builds_no_refit_state(cases):
    """a re-lit scene refuses nothing a moved one would: the switch stays off and a later first move still works"""
    c = cases("veach_group")
    s = c.edited()
    assert s.lights_movable is False and s.light_update_info()["lights"] == 0
    a, b = group_facets(c.arr, 1)
    with pytest.raises(mcpt.MCPTError, match="is a light triangle"):
        s.update(a, c.arr["positions"][a:b])
    assert_tables_equal(s, c.ref)


def test_rebuild_after_a_relight_leaves_the_tables_alone(cases):
    c = cases("veach_odd")
    s = c.edited()
    st = s.rebuild()
    assert st["device_states"] == 1
    assert_tables_equal(s, c.ref)
    cam = sized(c.cam, W, H)
    assert_tight(mcpt.render(s, cam, SPP, mode="mis", seed=SEED)[0], mcpt.render(c.ref, cam, SPP, mode="mis", seed=SEED)[0],
                 "rebuild after a re-light")


def test_frame_sequence_frame_after_a_relight_and_a_material_edit(cases):
    """whatever a render call derives from the light or material tables is derived again by the next one"""
    c = cases("veach_group")
    cam = sized(c.cam, W, H)
    mtl = c.arr["materials"].copy()
    mtl[0] = (0.1, 0.5, 0.2, 0.3, 0.0, 0.1, 30.0)
    s = fresh(c.arr)
    seq = mcpt.FrameSequence(s, W, H, SPP, denoise=False)
    seq.frame(cam, SEED)
    for first, rad in c.edits:
        s.set_light_radiance(first, rad)
    s.set_materials(0, mtl[:1])
    seq.reset()
    got = seq.frame(cam, SEED + 1)
    raw = seq.read("raw")
    seq.close()
    ref = fresh_grouped(with_materials(c.want, 0, mtl[:1]), c.gi)
    ref_seq = mcpt.FrameSequence(ref, W, H, SPP, denoise=False)
    want = ref_seq.frame(cam, SEED + 1)
    raw_want = ref_seq.read("raw")
    ref_seq.close()
    assert_tight(raw, raw_want, "sequence frame after a re-light")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("extra", [[], ["--device-sequence"]], ids=["host-sequence", "device-sequence"])
def test_cli_dim_and_tint(tmp_path, extra):
    """frames 0 .. 2 of the CLI against a Python sequence with the same edits; the PFM is float32 (6e-8)"""
    frames, w, h, spp = 3, 32, 24, 2
    pfm = str(tmp_path / "relit.pfm")
    r = subprocess.run([CLI, "--scene", SCENE_BASE, "--out", str(tmp_path / "relit.bmp"), "--hdr", pfm, "--width", str(w), "--height", str(h),
                        "--spp", str(spp), "--frames", str(frames), "--dim", "4:0.5", "--dim", "3:1.5", "--tint", "0:0.1,0.6,0.2", *extra],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("dimmed light group 4 by 0.5") == 2 and r.stdout.count("dimmed light group 3 by 1.5") == 2
    assert r.stdout.count("tinted material 0") == 1
    s = mcpt.Scene.load(SCENE_OBJ, SCENE_XML)
    arr, gi = s.arrays(), s.light_groups()
    rad = arr["light_radiance"].copy()
    cam = mcpt.Camera.reference(w, h)
    seq = mcpt.FrameSequence(s, w, h, spp, denoise=False)
    shown = []
    for k in range(frames):
        if k >= 1:
            for g, factor in ((4, 0.5), (3, 1.5)):
                rad[gi == g] *= factor
                s.set_group_radiance(g, rad[gi == g][0])
        if k == 1:
            row = arr["materials"][0].copy()
            row[:3] = (0.1, 0.6, 0.2)
            s.set_materials(0, row)
        seq.frame(cam, SEED + k)
        shown.append(seq.read("accumulated"))
    seq.close()
    assert np.array_equal(s.arrays()["light_radiance"], rad)
    for k in range(frames):
        got = read_pfm(str(tmp_path / ("relit_%04d.pfm" % k)))
        err = rel_l2(got, shown[k])
        print("frame %d: rel L2 %.3e against the Python sequence" % (k, err))
        assert err <= 1e-6, (k, err)
    assert rel_l2(shown[1], shown[0]) > 1e-3


def test_close_frees_what_a_relight_allocated(scenes):
    import torch
    arr, cam = scenes("veach")
    gc.collect()
    b0 = mcpt.debug_device_bytes_live()
    s = on_device(arr, cam)
    s.set_light_radiance(5, arr["light_radiance"][5:200] * 0.5)
    s.set_light_radiance_device(0, 7, torch.ones(7, 3, dtype=torch.float64).cuda().data_ptr())
    s.set_materials(0, arr["materials"][:2])
    assert mcpt.debug_device_bytes_live() > b0
    s.close()
    assert mcpt.debug_device_bytes_live() == b0
