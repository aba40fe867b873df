"""The host driver's integer statistics, pinned per driver branch (GPU).

For a fixed seed every count below follows from the seed alone: which generations the wavefront loop makes, how
many prep / trace launches it issues, how many nodes it shades, caches and spills, how many rays it shoots.  One tiny
frame per branch of the driver (render_on_device) is rendered and its counters are compared, exactly, with
tests/golden/driver_counters.json -- recorded from the driver before it was broken up into a plan, bound buffers and
a wavefront run, after three recordings had agreed on every field kept.  Every case sets samples_per_launch, so the
working set (and with it the generation structure) does not depend on the free device memory.  Where the CPU oracle
counts the same thing (a plain camera render's extension rays, light-only rays and, with a light prep, its prep
nodes), the count is held to the oracle too.

Left out of the recording: the spill case's generations, trace_launches, prep_launches and spilled_nodes.  Which
children a full generation parks on the spill stack depends on the order in which the workgroups appended them, so
the later generations' sizes (not their sum) differ from run to run: three recordings gave 857 / 872 / 874
generations and 3087 / 3146 / 3162 spilled nodes.  That case asserts spilled_nodes > 0 instead.
"""
import json

import pytest

import monte_carlo_path_tracing_amd as mcpt
from conftest import GOLDEN, SCENE_OBJ, SCENE_XML, cornell_scene
from oracle import pyoracle as po
import scenegen

SEED = 20240430
GOLDEN_FILE = GOLDEN / "driver_counters.json"

# the counts that follow from the seed alone (no time, no device count)
FIELDS = ["camera_samples", "rays", "light_rays", "shading_nodes", "generations", "trace_launches", "prep_launches",
          "prep_full_nodes", "prep_cached_nodes", "prep_cache_points", "spilled_nodes", "light_evals_total",
          "light_evals_culled_backface", "light_evals_culled_plane", "light_evals_candidates", "light_evals_survived",
          "prep_exact_nodes", "prep_band_nodes"]
MUST_HAVE = FIELDS[:4]

# name -> (scene, W, H, spp, mode, render keywords); samples_per_launch is set in every case
CASES = {
    "mis_stale": ("veach", 32, 24, 4, "mis", dict(samples_per_launch=2)),
    "mis_fresh_pdf": ("veach", 16, 12, 4, "mis", dict(samples_per_launch=2, flags=mcpt.RENDER_FRESH_PDF)),
    "shade": ("veach", 16, 12, 4, "shade", dict(samples_per_launch=2)),
    "shade_area": ("veach", 16, 12, 4, "shade_area", dict(samples_per_launch=2)),
    "brdf": ("veach", 16, 12, 8, "brdf", dict(samples_per_launch=3)),
    "split_brdf": ("veach", 16, 12, 8, "brdf", dict(samples_per_launch=3, flags=mcpt.DEBUG_SPLIT_BRDF)),
    "no_root_cache": ("veach", 16, 12, 4, "mis", dict(samples_per_launch=2, flags=mcpt.DEBUG_NO_ROOT_CACHE)),
    "fp32": ("veach", 16, 12, 4, "mis", dict(samples_per_launch=2, flags=mcpt.RENDER_PRECISION_FP32)),
    "cornell_small_table": ("cornell", 16, 12, 4, "mis", dict(samples_per_launch=2)),
    "spill": ("room", 8, 6, 2, "mis", dict(samples_per_launch=1, queue_factor=1)),
    "adaptive": ("veach", 32, 24, 12, "mis", dict(samples_per_launch=2)),
    "rays": ("veach", 13, 7, 4, "mis", dict(samples_per_launch=2)),
    "jitter": ("veach", 16, 12, 4, "mis", dict(samples_per_launch=2, flags=mcpt.RENDER_PIXEL_JITTER)),
}
# plain camera renders with the oracle's own sampling (fp64 picks): its extension rays (stats[2]) and light-only
# rays (stats[3]) are the render's, and its light-prep nodes (stats[1]) the shading nodes of the modes that prep
ORACLE_CASES = ["mis_stale", "mis_fresh_pdf", "shade", "shade_area", "brdf", "split_brdf", "no_root_cache",
                "cornell_small_table", "spill"]
OMODE = {"mis": po.MODE_MIS, "shade": po.MODE_SHADE, "shade_area": po.MODE_SHADE_AREA, "brdf": po.MODE_BRDF}

_scenes = {}
_stats = {}


def _paths(which, tmp):
    if which == "veach":
        return SCENE_OBJ, SCENE_XML
    if which == "cornell":
        return cornell_scene(300)
    return scenegen.occluded_room(str(tmp))


def _scene(which, tmp):
    if which not in _scenes:
        obj, xml = _paths(which, tmp)
        _scenes[which] = (mcpt.Scene.load(obj, xml), obj, xml)
    return _scenes[which]


def _camera(which, scene, W, H):
    if which == "veach":
        return mcpt.Camera.reference(W, H)
    cam = scene.camera()
    cam.width, cam.height = W, H
    return cam


def measure(name, tmp):
    """the case's counters as {field: int} (rendered once per session)"""
    if name in _stats:
        return _stats[name]
    which, W, H, spp, mode, kw = CASES[name]
    scene = _scene(which, tmp)[0]
    cam = _camera(which, scene, W, H)
    if name == "adaptive":
        st = mcpt.render_adaptive(scene, cam, spp, 0.1, min_spp=4, pass_spp=4, radius=1, mode=mode, seed=SEED, **kw)[3]
    elif name == "rays":
        o, d = mcpt.camera_rays(cam)
        st = mcpt.render_rays(scene, o, d, spp, mode=mode, seed=SEED, **kw)[1]
    else:
        st = mcpt.render(scene, cam, spp, mode=mode, seed=SEED, **kw)[1]
    _stats[name] = {f: int(getattr(st, f)) for f in FIELDS}
    return _stats[name]


def test_golden_file_covers_every_case():
    gold = json.loads(GOLDEN_FILE.read_text())
    assert sorted(gold) == sorted(CASES)
    for name, row in gold.items():
        assert set(MUST_HAVE) <= set(row) <= set(FIELDS), name
        assert all(isinstance(v, int) for v in row.values()), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_driver_counters_match_the_recording(tmp_path_factory, name):
    gold = json.loads(GOLDEN_FILE.read_text())[name]
    got = measure(name, tmp_path_factory.getbasetemp())
    print(name, got)
    assert {f: got[f] for f in gold} == gold
    if name == "spill":
        assert got["spilled_nodes"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ORACLE_CASES)
def test_counts_match_the_oracle(tmp_path_factory, name):
    tmp = tmp_path_factory.getbasetemp()
    which, W, H, spp, mode, _ = CASES[name]
    got = measure(name, tmp)
    _, obj, xml = _scene(which, tmp)
    o = po.Scene(obj, xml)
    c = po.reference_camera(W, H) if which == "veach" else o.camera()
    c.width, c.height = W, H
    e, _ = po.camera_ray(c, 0, 0)
    o.build_grid(e)
    _, ost = o.render(c, OMODE[mode], SEED, spp, nthreads=8)
    print(name, "oracle", [int(v) for v in ost])
    assert got["camera_samples"] == W * H * spp
    assert (got["rays"], got["light_rays"]) == (int(ost[2]), int(ost[3]))
    if mode in ("mis", "shade"):
        assert got["shading_nodes"] == int(ost[1])
