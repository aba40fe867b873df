"""The root pick table: one pixel-major pass per window of a run's samples computes every cached
root's light pick (k_root_pick_table) and the generations look their fresh roots up (k_pick_lookup), instead of
searching the pixel's cached row root by root (k_prep_pick_g, kept behind MCPT_DEBUG_NO_PICK_TABLE and for the
cases the table does not cover).  Both paths call the same device functions, so picks, sums and exact-list
membership must be EQUAL -- and frames equal up to the order of the fp64 atomic adds.

Frames are small (<= 33 x 25: no multiple of a pixel tile of 16) and the table is engaged at small sample counts
through mcpt_debug_set_pick_table(min_samples=2); window_samples=16 makes a 70-sample run roll over five windows,
the last one partial."""
import numpy as np
import pytest

import monte_carlo_path_tracing_amd as mcpt
import scenegen
from conftest import SCENE_OBJ, SCENE_XML, cornell_scene

pytestmark = pytest.mark.gpu
SEED = 20240430
OFF = mcpt.DEBUG_NO_PICK_TABLE
L2, PX = 1e-12, 1e-10  # "equal up to fp64 atomic order" (test_deferred_duplicate_roots_change_nothing)


def rel_l2(g, c):
    return float(np.linalg.norm(g - c) / max(np.linalg.norm(c), 1e-300))


def max_px_rel(g, c):
    d = np.linalg.norm((g - c).reshape(-1, 3), axis=1)
    n = np.linalg.norm(c.reshape(-1, 3), axis=1)
    return float(np.max(np.where(n > 0, d / np.maximum(n, 1e-300), np.where(d > 0, np.inf, 0.0))))


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    d = tmp_path_factory.mktemp("picktab")
    out = {"veach": mcpt.Scene.load(SCENE_OBJ, SCENE_XML)}
    for name, (make, _) in scenegen.STRESS.items():
        out[name] = mcpt.Scene.load(*make(str(d / name)))
    return out


@pytest.fixture
def table_on():
    """the table from 2 samples per pixel on; set_window(n) caps its window"""
    mcpt.debug_set_pick_table(2, 0)
    try:
        yield lambda window: mcpt.debug_set_pick_table(2, window)
    finally:
        mcpt.debug_set_pick_table(0, 0)


def cam_of(scene, w, h):
    cam = scene.camera()
    cam.width, cam.height = w, h
    return cam


def picks_both(scene, cam, rng_, mode="mis"):
    a = mcpt.debug_root_picks(scene, cam, rng_[1], rng_, mode=mode, seed=SEED)
    b = mcpt.debug_root_picks(scene, cam, rng_[1], rng_, mode=mode, seed=SEED, flags=OFF)
    return a, b


def assert_picks_equal(a, b, what):
    (pa, wa, fa), (pb, wb, fb) = a, b
    live = pb != -2
    print("%s: %d of %d roots survive, %d without a pick, %d ambiguous" % (
        what, live.sum(), live.size, (pb == -1).sum(), fb.sum()))
    assert live.sum() > live.size // 4  # the scene is seen and RR keeps ~0.6
    assert np.array_equal(pa, pb), np.argwhere(pa != pb)[:10]
    assert np.array_equal(fa, fb), np.argwhere(fa != fb)[:10]
    assert np.array_equal(wa.view(np.uint64), wb.view(np.uint64)), np.argwhere(wa != wb)[:10]


@pytest.mark.parametrize("window", [0, 16])
@pytest.mark.parametrize("rng_", [(0, 70), (6, 76)])
def test_pick_identity_veach(scenes, table_on, rng_, window):
    table_on(window)
    cam = cam_of(scenes["veach"], 33, 25)
    a, b = picks_both(scenes["veach"], cam, rng_)
    assert_picks_equal(a, b, "veach 33x25 samples %s window %d" % (rng_, window))
    assert (b[0] >= 0).sum() > 1000 and len(np.unique(b[0][b[0] >= 0])) > 100


@pytest.mark.parametrize("name", ["slivers", "sphmix", "tinyfar"])
def test_pick_identity_stress(scenes, table_on, name):
    cam = cam_of(scenes[name], 32, 24)
    a, b = picks_both(scenes[name], cam, (0, 64))
    assert_picks_equal(a, b, "%s 32x24x64" % name)
    if name == "tinyfar":  # the band always covers the pick: every surviving root is redone exactly
        assert np.array_equal(a[2] == 1, a[0] != -2)


COUNTS = ["shading_nodes", "rays", "light_rays", "prep_cached_nodes", "prep_exact_nodes", "prep_band_nodes"]


def assert_render_equal(scene, cam, spp, mode="mis"):
    a, sa = mcpt.render(scene, cam, spp, mode=mode, seed=SEED)
    b, sb = mcpt.render(scene, cam, spp, mode=mode, seed=SEED, flags=OFF)
    l2, px = rel_l2(a, b), max_px_rel(a, b)
    print("%dx%dx%d %s: table roots %d of %d cached, rel L2 %.2e, max per-pixel %.2e" % (
        cam.width, cam.height, spp, mode, sa.pick_table_roots, sa.prep_cached_nodes, l2, px))
    for k in COUNTS:
        assert getattr(sa, k) == getattr(sb, k), k
    assert sb.pick_table_roots == 0
    assert l2 < L2 and px < PX
    return sa


@pytest.mark.parametrize("case", ["veach", "veach-window16", "veach-shade", "tinyfar"])
def test_render_identity(scenes, table_on, case):
    name, _, variant = case.partition("-")
    if variant == "window16":
        table_on(16)
    cam = cam_of(scenes[name], *((33, 25) if name == "veach" else (32, 24)))
    st = assert_render_equal(scenes[name], cam, 64, mode="shade" if variant == "shade" else "mis")
    assert st.pick_table_roots == st.prep_cached_nodes > 0


def test_fallback_light_counts(scenes, table_on):
    """beyond 4096 lights (dense: 14 160, no root cache at all) and at <= 64 (the small-table pick)"""
    st = assert_render_equal(scenes["dense"], cam_of(scenes["dense"], 32, 24), 8)
    assert st.pick_table_roots == 0
    small = mcpt.Scene.load(*cornell_scene(300))
    assert small.nlights <= 64
    st = assert_render_equal(small, cam_of(small, 32, 24), 16)
    assert st.pick_table_roots == 0 and st.prep_cached_nodes > 0


def test_fallback_below_min_samples(scenes):
    """the default min_samples is far above 8 samples per pixel; with it lowered to 8 the same render engages"""
    cam = cam_of(scenes["veach"], 33, 25)
    st = assert_render_equal(scenes["veach"], cam, 8)
    assert st.pick_table_roots == 0 and st.prep_cached_nodes > 0
    mcpt.debug_set_pick_table(8, 0)
    try:
        assert assert_render_equal(scenes["veach"], cam, 8).pick_table_roots == st.prep_cached_nodes
        assert assert_render_equal(scenes["veach"], cam, 7).pick_table_roots == 0
    finally:
        mcpt.debug_set_pick_table(0, 0)


def test_fallback_adaptive_later_passes(scenes, table_on):
    """pass 0 (the whole frame) takes the table, the later passes' active-pixel runs do not: the call's table roots
    are those of samples [0, 16) alone"""
    s, cam = scenes["veach"], cam_of(scenes["veach"], 33, 25)
    kw = dict(min_spp=16, pass_spp=16, mode="mis", seed=SEED)
    a, ca, _, sa = mcpt.render_adaptive(s, cam, 48, 1e-9, **kw)
    b, cb, _, sb = mcpt.render_adaptive(s, cam, 48, 1e-9, flags=OFF, **kw)
    _, s16 = mcpt.render(s, cam, 16, mode="mis", seed=SEED)
    print("adaptive: %d table roots of %d cached; plain 16 spp: %d" % (
        sa.pick_table_roots, sa.prep_cached_nodes, s16.pick_table_roots))
    assert ca.max() > 16 and np.array_equal(ca, cb)
    assert sa.pick_table_roots == s16.pick_table_roots == s16.prep_cached_nodes < sa.prep_cached_nodes
    assert sb.pick_table_roots == 0
    for k in COUNTS:
        assert getattr(sa, k) == getattr(sb, k), k
    assert rel_l2(a, b) < L2 and max_px_rel(a, b) < PX
