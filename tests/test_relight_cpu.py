"""In-place re-lighting (mcpt_scene_set_light_radiance, mcpt_scene_set_materials, mcpt_scene_light_groups; include/mcpt.h,
DESIGN.md §4.24) without a GPU: no device state exists, so only the host half runs -- the ABI, the groups, the edited
host arrays, every refusal, the no-ops and the CLI's usage errors.  The device half is tests/test_relight.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE_OBJ, SCENE_XML
import monte_carlo_path_tracing_amd as mcpt
from test_light_update_cpu import assert_arrays_equal, check_trees, light_groups
from test_scene_update_cpu import fresh

CLI = os.path.join(ROOT, "monte_carlo_path_tracing_amd", "mcpt_render")
SCENE_BASE = os.path.splitext(str(SCENE_OBJ))[0]
NEW = ("mcpt_relight_stats_init", "mcpt_scene_set_light_radiance", "mcpt_scene_set_light_radiance_device",
       "mcpt_scene_set_materials", "mcpt_scene_light_groups")
NEW_TABLES = ("light_rad", "light_sum", "grp_sum", "grp_cum", "mtl")


def fresh_grouped(arr, groups):
    """the fresh scene of the rule: mcpt_scene_create of the arrays with the grouping passed explicitly"""
    return mcpt.Scene.create(arr["positions"], arr["normals"], arr["material_id"], arr["materials"], arr["light_facet"],
                             arr["light_radiance"], light_group=groups)


def with_radiance(arr, first, rad):
    out = {k: v.copy() for k, v in arr.items()}
    rad = np.asarray(rad, np.float64).reshape(-1, 3)
    out["light_radiance"][first:first + len(rad)] = rad
    return out


def with_materials(arr, first, mtl):
    out = {k: v.copy() for k, v in arr.items()}
    mtl = np.asarray(mtl, np.float32).reshape(-1, 7)
    out["materials"][first:first + len(mtl)] = mtl
    return out


def group_index(arr):
    """the group index of every light from the runs of equal radiance"""
    g = np.zeros(len(arr["light_radiance"]), np.int32)
    for k, (l0, l1) in enumerate(light_groups(arr)):
        g[l0:l1] = k
    return g


@pytest.fixture(scope="module")
def veach_arrays():
    return mcpt.Scene.load(SCENE_OBJ, SCENE_XML).arrays()


def test_abi_of_the_relight(tmp_path):
    hdr = (ROOT / "include" / "mcpt.h").read_text()
    for name in NEW:
        assert name in mcpt.EXPORTS and re.search(r"\b%s\s*\(" % name, hdr) and hasattr(mcpt.lib(), name), name
    assert int(re.search(r"#define MCPT_VERSION (\d+)", hdr).group(1)) == 20300 == mcpt.lib().mcpt_version() == mcpt.MCPT_VERSION
    assert mcpt.RELIGHT_TABLES == mcpt.LIGHT_TABLES + NEW_TABLES and "RelightStats" in mcpt.__all__
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "mcpt.h"', "int main(void) {",
           'printf("sizeof %zu\\n", sizeof(mcpt_relight_stats));']
    for f, _ in mcpt.RelightStats._fields_:
        src.append('printf("%s %%zu\\n", offsetof(mcpt_relight_stats, %s));' % (f, f))
    src.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(tmp_path / "layout.c"), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(mcpt.RelightStats) == 32
    for f, _ in mcpt.RelightStats._fields_:
        assert int(got[f]) == getattr(mcpt.RelightStats, f).offset, f
    assert [f for f, _ in mcpt.RelightStats._fields_] == ["struct_size", "lights", "chunks", "groups", "materials", "device_states",
                                                          "device_seconds"]
    st = mcpt.RelightStats()
    st.lights = 7
    mcpt.lib().mcpt_relight_stats_init(C.byref(st))
    assert st.struct_size == 32 and st.lights == 0


def test_light_groups_of_the_stand_in_and_of_an_explicit_grouping(veach_arrays):
    loaded = mcpt.Scene.load(SCENE_OBJ, SCENE_XML)
    want = group_index(veach_arrays)
    assert want.max() >= 2 and len(want) == 3012
    assert np.array_equal(loaded.light_groups(), want) and loaded.light_groups().dtype == np.int32
    assert np.array_equal(fresh(veach_arrays).light_groups(), want)
    # an explicit grouping that the radiances would not give: the first group cut in two
    cut = want.copy()
    cut[400:] += 1
    assert np.array_equal(fresh_grouped(veach_arrays, cut).light_groups(), cut)
    # four equal radiances, two groups
    tri = np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]] * 4, np.float32) + np.arange(4, dtype=np.float32)[:, None]
    nrm = np.tile(np.array([0, 0, 1] * 3, np.float32), (4, 1))
    s = mcpt.Scene.create(tri, nrm, [0] * 4, [[0.5] * 6 + [1.0]], [0, 1, 2, 3], [[1, 1, 1]] * 4, light_group=[0, 0, 1, 1])
    assert np.array_equal(s.light_groups(), [0, 0, 1, 1])


def test_host_only_edits_equal_the_edited_arrays(veach_arrays):
    groups = light_groups(veach_arrays)
    gi = group_index(veach_arrays)
    s = fresh(veach_arrays)
    l0, l1 = groups[1]
    rng = np.random.default_rng(5)
    sub = rng.random((131, 3)) * 9.0
    st = s.set_light_radiance(l0 + 1, sub)
    assert st == dict(lights=131, chunks=(l0 + 131) // 64 - (l0 + 1) // 64 + 1, groups=0, materials=0, device_states=0,
                      device_seconds=0.0), st
    want = with_radiance(veach_arrays, l0 + 1, sub)
    # groups 2 and 3 end up with one radiance: neighbours, equal, and still two groups
    same = (6.5, 6.5, 6.5)
    for g in (2, 3):
        st = s.set_group_radiance(g, same)
        assert st["lights"] == groups[g][1] - groups[g][0] and st["groups"] == 1, st
        want = with_radiance(want, groups[g][0], np.tile(same, (groups[g][1] - groups[g][0], 1)))
    mtl = veach_arrays["materials"].copy()
    mtl[1] = (0.0, 0.0, 0.0, 0.25, 0.0, 0.75, 40.0)
    st = s.set_materials(1, mtl[1:3])
    assert st == dict(lights=0, chunks=0, groups=0, materials=2, device_states=0, device_seconds=0.0), st
    want = with_materials(want, 1, mtl[1:3])
    assert_arrays_equal(s.arrays(), want)
    assert np.array_equal(s.light_groups(), gi)
    # the radiances alone would give another grouping: groups 2 and 3 merged, the sub-range a group per light
    inferred = light_groups(want)
    assert (groups[2][0], groups[3][1]) in inferred and not np.array_equal(fresh(want).light_groups(), gi)
    ref = fresh_grouped(want, gi)
    assert_arrays_equal(s.arrays(), ref.arrays())
    assert np.array_equal(ref.light_groups(), gi)
    check_trees(s)


def refusal_cases(arr):
    """(what, call on a scene, words of the message): one entry per refusal of the header"""
    NL, M = len(arr["light_radiance"]), len(arr["materials"])
    rad, mtl = np.ones((2, 3)), np.array([[0.5] * 6 + [10.0]] * 2, np.float32)

    def bad_rad(c, v):
        r = np.ones((3, 3))
        r[1, c] = v
        return r

    def bad_mtl(c, v):
        m = np.array([[0.5] * 6 + [10.0]] * 3, np.float32)
        m[2, c] = v
        return m

    raw = mcpt.lib()
    return [
        ("lights: first < 0", lambda s: s.set_light_radiance(-1, rad), "lights [-1, 1) are not a range of the scene's %d" % NL),
        ("lights: past the table", lambda s: s.set_light_radiance(NL - 1, rad), "lights [%d, %d) are not a range" % (NL - 1, NL + 1)),
        ("lights: count < 0", lambda s: mcpt._check(raw.mcpt_scene_set_light_radiance(s.h, 0, -1, rad.ctypes.data_as(C.c_void_p), None)),
         "lights [0, -1) are not a range"),
        ("lights: NULL array", lambda s: mcpt._check(raw.mcpt_scene_set_light_radiance(s.h, 0, 2, None, None)), "NULL rgb"),
        ("lights: negative", lambda s: s.set_light_radiance(10, bad_rad(2, -1e-300)), "light 11 has a negative or non-finite radiance (component 2"),
        ("lights: NaN", lambda s: s.set_light_radiance(10, bad_rad(0, np.nan)), "light 11 has a negative or non-finite radiance (component 0"),
        ("lights: inf", lambda s: s.set_light_radiance(10, bad_rad(1, np.inf)), "light 11 has a negative or non-finite radiance (component 1"),
        ("materials: first < 0", lambda s: s.set_materials(-2, mtl), "materials [-2, 0) are not a range of the scene's %d" % M),
        ("materials: past the table", lambda s: s.set_materials(M - 1, mtl), "materials [%d, %d) are not a range" % (M - 1, M + 1)),
        ("materials: count < 0", lambda s: mcpt._check(raw.mcpt_scene_set_materials(s.h, 0, -3, mtl.ctypes.data_as(C.c_void_p), None)),
         "materials [0, -3) are not a range"),
        ("materials: NULL array", lambda s: mcpt._check(raw.mcpt_scene_set_materials(s.h, 0, 1, None, None)), "NULL mtl"),
        ("materials: negative Kd", lambda s: s.set_materials(0, bad_mtl(1, -0.5)), "material 2 has a negative or non-finite Kd"),
        ("materials: NaN Ks", lambda s: s.set_materials(0, bad_mtl(4, np.nan)), "material 2 has a negative or non-finite Ks"),
        ("materials: inf Ns", lambda s: s.set_materials(0, bad_mtl(6, np.inf)), "material 2 has a negative or non-finite Ns"),
        ("materials: negative Ns", lambda s: s.set_materials(0, bad_mtl(6, -1.0)), "material 2 has a negative or non-finite Ns"),
        ("device form: past the table", lambda s: s.set_light_radiance_device(NL, 1, 64), "lights [%d, %d) are not a range" % (NL, NL + 1)),
        ("device form: NULL array", lambda s: mcpt._check(raw.mcpt_scene_set_light_radiance_device(s.h, -1, 0, 1, None, None)), "NULL dev_rgb"),
    ]


N_REFUSALS = 17


@pytest.mark.parametrize("k", range(N_REFUSALS))
def test_refusals_change_nothing(veach_arrays, k):
    cases = refusal_cases(veach_arrays)
    assert len(cases) == N_REFUSALS
    what, call, words = cases[k]
    s = fresh(veach_arrays)
    with pytest.raises(mcpt.MCPTError, match=re.escape(words)) as e:
        call(s)
    assert "mcpt error -1" in str(e.value), what
    got = s.arrays()
    for key, v in veach_arrays.items():
        assert got[key].tobytes() == v.tobytes(), (what, key)
    assert np.array_equal(s.light_groups(), group_index(veach_arrays))


def test_null_scene_and_stats_size_are_refused(veach_arrays):
    L = mcpt.lib()
    s = fresh(veach_arrays)
    one = np.ones(3)
    for rc in (L.mcpt_scene_set_light_radiance(None, 0, 1, one.ctypes.data_as(C.c_void_p), None),
               L.mcpt_scene_set_light_radiance_device(None, -1, 0, 1, C.c_void_p(64), None),
               L.mcpt_scene_set_materials(None, 0, 0, None, None), L.mcpt_scene_light_groups(None, np.zeros(1, np.int32))):
        assert rc == -1 and "NULL scene" in L.mcpt_last_error().decode()
    st = mcpt.RelightStats()
    L.mcpt_relight_stats_init(C.byref(st))
    st.struct_size -= 8
    assert L.mcpt_scene_set_light_radiance(s.h, 0, 1, one.ctypes.data_as(C.c_void_p), C.byref(st)) == -1
    assert "mcpt_relight_stats.struct_size" in L.mcpt_last_error().decode()
    assert_arrays_equal(s.arrays(), veach_arrays)


def test_a_count_of_zero_succeeds_and_changes_nothing(veach_arrays):
    L = mcpt.lib()
    s = fresh(veach_arrays)
    zero = dict(lights=0, chunks=0, groups=0, materials=0, device_states=0, device_seconds=0.0)
    NL, M = s.nlights, s.nmaterials
    assert s.set_light_radiance(5, np.zeros((0, 3))) == zero
    assert s.set_light_radiance(NL, np.zeros((0, 3))) == zero  # an empty range at the table's end is a range
    assert s.set_materials(M, np.zeros((0, 7), np.float32)) == zero
    assert s.set_light_radiance_device(3, 0, 0) == zero
    assert L.mcpt_scene_set_light_radiance(s.h, 0, 0, None, None) == 0 and L.mcpt_scene_set_materials(s.h, 0, 0, None, None) == 0
    got = s.arrays()
    for key, v in veach_arrays.items():
        assert got[key].tobytes() == v.tobytes(), key


def test_a_zero_radiance_is_allowed(veach_arrays):
    s = fresh(veach_arrays)
    l0, l1 = light_groups(veach_arrays)[0]
    s.set_group_radiance(0, (0.0, 0.0, 0.0))
    assert not s.arrays()["light_radiance"][l0:l1].any() and s.arrays()["light_radiance"][l1:].all()
    with pytest.raises(mcpt.MCPTError, match="no lights in group 99"):
        s.set_group_radiance(99, (1, 1, 1))


@pytest.mark.parametrize("args,word", [
    (["--dim", "0:0.5"], "--frames N"),
    (["--tint", "0:0.5,0.5,0.5"], "--frames N"),
    (["--frames", "2", "--dim", "0"], "GROUP:FACTOR"),
    (["--frames", "2", "--dim", "0:0.5x"], "GROUP:FACTOR"),
    (["--frames", "2", "--dim", "-1:0.5"], "GROUP:FACTOR"),
    (["--frames", "2", "--dim", "0:-0.5"], "GROUP:FACTOR"),
    (["--frames", "2", "--dim", "0:nan"], "GROUP:FACTOR"),
    (["--frames", "2", "--dim"], "missing value"),
    (["--frames", "2", "--tint", "0:0.5,0.5"], "MATERIAL:R,G,B"),
    (["--frames", "2", "--tint", "0:0.5,0.5,-1"], "MATERIAL:R,G,B"),
    (["--frames", "2", "--tint", "0:0.5,0.5,inf"], "MATERIAL:R,G,B"),
    (["--frames", "2", "--tint", "-1:0.5,0.5,0.5"], "MATERIAL:R,G,B"),
    (["--frames", "2", "--dim", "99:0.5"], "no light group 99"),
    (["--frames", "2", "--tint", "99:0.5,0.5,0.5"], "material 99 is not one of the scene's"),
])
def test_cli_relight_usage_errors(args, word):
    """refused before any device is touched (an unknown group or row: once the scene is loaded)"""
    r = subprocess.run([CLI, "--scene", SCENE_BASE, "--width", "16", "--height", "12", "--spp", "1", *args],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr, (r.returncode, r.stderr)
