"""mcpt_scene_rebuild and mcpt_scene_tree_cost on the GPU (include/mcpt.h): after a rebuild the scene
behaves as a fresh mcpt_scene_create of the current arrays -- hits bit for bit (against a fresh scene and against the
fp64 brute force), frames up to the order of the framebuffer's fp64 atomics -- the device's new tree passes the host walk
(mcpt_debug_bvh4_check_device), is breadth-first, at most 15 levels deep and a pure function of the positions, and later
updates and transforms refit it.  Run on the MI355X box: `pytest -m gpu`."""
import numpy as np
import pytest

from conftest import SCENE_OBJ, SCENE_XML
import monte_carlo_path_tracing_amd as mcpt
import scenegen
from test_gpu_parity import brute_force_hits
from test_scene_update import (PLATE, SEED, SPP, H, W, assert_tight, check_device, dirty_nodes, moved_plate, read_pfm, rows,
                               run_cli, with_range)
from test_scene_update_cpu import fresh, translated
from test_transform_cpu import assert_arrays_equal, plate_move, with_transform

pytestmark = pytest.mark.gpu
MAX_LEVELS, STACK = 15, 48  # the builder's depth bound and the traversal kernels' stack entries
PLATE_B = (48, 60)
# V_rebuilt / V_fresh measured on the needles case below; the test allows 1.5 x that
NEEDLES_VISITS_RATIO = 1.318  # 144 301 / 109 481


@pytest.fixture(scope="module")
def veach():
    return mcpt.Scene.load(SCENE_OBJ, SCENE_XML).arrays()


@pytest.fixture(scope="module")
def needles(tmp_path_factory):
    obj, xml = scenegen.needles(str(tmp_path_factory.mktemp("needles")))
    return mcpt.Scene.load(obj, xml).arrays()


def edge_rays(arr, n, seed, focus=None):
    """test_scene_update's rays: aimed at vertices, edge points and interior points of random triangles, some targets
    off by a few ulps, a fifth excluding their own triangle; a third aimed at the facets [focus[0], focus[1])"""
    P = arr["positions"].astype(np.float64).reshape(-1, 3, 3)
    rng = np.random.default_rng(seed)
    tri = rng.integers(0, len(P), n)
    if focus is not None:
        tri[::3] = rng.integers(focus[0], focus[1], len(tri[::3]))
    kind = rng.integers(0, 3, n)
    w = rng.random((n, 3))
    w[kind == 0] = np.eye(3)[rng.integers(0, 3, (kind == 0).sum())]  # a vertex
    e = rng.integers(0, 3, n)
    w[(kind == 1), e[kind == 1]] = 0.0  # a point on an edge
    w /= w.sum(axis=1, keepdims=True)
    target = np.einsum("nk,nkc->nc", w, P[tri])
    target *= 1.0 + rng.choice([0.0, 1e-15, -1e-15, 1e-12, -1e-12], (n, 1))
    lo, hi = P.reshape(-1, 3).min(axis=0), P.reshape(-1, 3).max(axis=0)
    ro = lo - 0.5 + rng.random((n, 3)) * (hi - lo + 1.0)
    near = rng.random(n) < 0.3
    ro[near] = target[near] + rng.normal(0, 0.05, (near.sum(), 3))
    rd = target - ro
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    ex = np.where(rng.random(n) < 0.2, tri, -1).astype(np.int32)
    return ro, rd, ex


def assert_hits_equal_brute_force(scene, arr, ro, rd, ex):
    f, tbg = mcpt.closest_hit(scene, ro, rd, ex)
    bf = brute_force_hits(arr, np.concatenate([ro, rd, ex[:, None]], axis=1), False)
    assert np.array_equal(f, bf), np.flatnonzero(f != bf)[:8]
    return f, tbg


def level_starts(nodes):
    """the first node of every level, asserting the layout the LDS top levels and the refit rely on: every level is a
    contiguous run, and the inner children of a level are exactly the next one, in order"""
    child = nodes["child"]
    lf = [0, 1]
    while True:
        c = child[lf[-2]:lf[-1]].reshape(-1)
        inner = c[(c >= 0) & (c != mcpt.BVH4_EMPTY)]
        assert np.array_equal(inner, np.arange(lf[-1], lf[-1] + len(inner))), len(lf)
        if len(inner) == 0:
            break
        lf.append(lf[-1] + len(inner))
    assert lf[-1] == len(nodes)
    return lf


def stack_need(nodes):
    """bvh4_stack_need in numpy: the most entries a traversal can hold, sum over a root-to-node path of (children - 1)"""
    child = nodes["child"]
    used = (child != mcpt.BVH4_EMPTY).sum(axis=1)
    above = np.zeros(len(nodes), np.int64)
    here = np.zeros(len(nodes), np.int64)
    for n in range(len(nodes)):  # breadth-first: parents first
        here[n] = above[n] + max(int(used[n]) - 1, 0)
        for c in child[n]:
            if c >= 0 and c != mcpt.BVH4_EMPTY:
                above[c] = here[n]
    return int(here.max())


def tree_cost_numpy(nodes):
    """the header's formula from the downloaded fp32 nodes"""
    lo, hi = nodes["lo"].astype(np.float64), nodes["hi"].astype(np.float64)  # [node, axis, slot]
    used = nodes["child"] != mcpt.BVH4_EMPTY
    if not used[0].any():
        return 0.0
    rl, rh = lo[0][:, used[0]].min(axis=1), hi[0][:, used[0]].max(axis=1)
    d0 = rh - rl
    a0 = 2.0 * (d0[0] * d0[1] + d0[1] * d0[2] + d0[2] * d0[0])
    if a0 == 0.0:
        return 0.0
    d = hi - lo
    area = 2.0 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0])
    weight = np.where(nodes["child"] < 0, nodes["count"], 1).astype(np.float64)
    return float((area[used] / a0 * weight[used]).sum())


def check_rebuilt(scene, st, nfacets):
    """the stats of a rebuild against what the device holds afterwards"""
    r = check_device(scene, nfacets)
    nodes, qn, lf = mcpt.debug_bvh4_download(scene)
    assert r["duplicates"] == 0 and sorted(lf.tolist()) == list(range(nfacets))  # one leaf slot per facet
    starts = level_starts(nodes)
    assert r["depth"] == len(starts) - 1 == st["levels"] <= MAX_LEVELS, (r, st)
    assert st["nodes"] == len(nodes) == r["nodes"] and st["facets"] == nfacets and st["device_states"] == 1, st
    assert st["stack_need"] == stack_need(nodes) <= 3 * MAX_LEVELS < STACK, (st, stack_need(nodes))
    leaf = (nodes["child"] < 0)
    # the quantised nodes keep the traversal's packed leaf codes ~((first slot << 5) | count)
    packed = np.where(leaf, ~((~nodes["child"] << 5) | nodes["count"]), nodes["child"])
    assert np.array_equal(packed, qn["child"]) and not qn["pad"].any()
    assert (nodes["count"][leaf] >= 1).all() and (nodes["count"][~leaf] == 0).all()
    assert st["device_seconds"] > 0
    return nodes, qn, lf


def test_untouched_scene(veach):
    cam = mcpt.Camera.reference(32, 24)
    scene, ref = fresh(veach), fresh(veach)
    f0, t0 = mcpt.primary_hits(scene, cam)
    st = scene.rebuild()
    check_rebuilt(scene, st, scene.nfacets)
    assert st["cost_before"] > 0 and st["cost_after"] > 0
    f1, t1 = mcpt.primary_hits(scene, cam)
    f2, t2 = mcpt.primary_hits(ref, cam)
    assert np.array_equal(f1, f2) and np.array_equal(t1, t2) and np.array_equal(f0, f1) and np.array_equal(t0, t1)
    ro, rd, ex = edge_rays(veach, 3000, 7)
    f, tbg = assert_hits_equal_brute_force(scene, veach, ro, rd, ex)
    fr, tr = mcpt.closest_hit(ref, ro, rd, ex)
    assert np.array_equal(f, fr) and np.array_equal(tbg, tr)
    assert (f >= 0).sum() > 1000
    with pytest.raises(mcpt.MCPTError, match="8-wide"):  # the 8-wide trees keep the old topology: refused
        mcpt.closest_hit(scene, ro[:4], rd[:4], ex[:4], wide=True)


def soup(nf, seed):
    """nf random triangles in a unit box, no lights"""
    rng = np.random.default_rng(seed)
    a = rng.random((nf, 1, 3))
    tri = (a + rng.normal(0, 0.15, (nf, 3, 3))).astype(np.float32).reshape(nf, 9)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (nf, 3))
    return dict(positions=tri, normals=nrm, material_id=np.zeros(nf, np.int32),
                materials=np.array([[0.5, 0.5, 0.5, 0, 0, 0, 1]], np.float32), light_facet=np.zeros(0, np.int32),
                light_radiance=np.zeros((0, 3)))


@pytest.mark.parametrize("nf", [1, 2, 3, 63, 64, 65, 257, 1025])
def test_wave_and_block_edges(nf):
    arr = soup(nf, 100 + nf)
    scene = fresh(arr)
    ro, rd, ex = edge_rays(arr, 300, nf)
    before = mcpt.closest_hit(scene, ro, rd, ex)  # the device state exists
    st = scene.rebuild()
    nodes, _, _ = check_rebuilt(scene, st, nf)
    f, tbg = assert_hits_equal_brute_force(scene, arr, ro, rd, ex)
    assert np.array_equal(f, before[0]) and np.array_equal(tbg, before[1])
    assert (f >= 0).sum() > 50  # (a ray that excludes its own triangle of a one-triangle soup misses)
    if nf == 1:
        assert len(nodes) == 1 and st["levels"] == 1 and st["stack_need"] == 0


def test_coincident_triangles():
    """64 exactly coincident triangles (equal Morton codes: median splits) and 8 others: a balanced tree, where the
    host's SAH builder can only stop at its depth cap.  The depth: a range that holds the cluster and some of the
    others is cut between two different codes, so each of a level's two cuts takes at least one of the 8 others away
    from the cluster's side -- at most 4 levels until the cluster is alone -- and 64 equal codes take 3 levels of median
    cuts (64, 16, 4, then leaves of two)."""
    arr = soup(72, 5)
    arr["positions"][:64] = arr["positions"][0]
    scene = fresh(arr)
    ro, rd, ex = edge_rays(arr, 300, 11, focus=(0, 64))
    mcpt.closest_hit(scene, ro, rd, ex)
    st = scene.rebuild()
    check_rebuilt(scene, st, 72)
    assert st["levels"] <= 7, st
    f, _ = assert_hits_equal_brute_force(scene, arr, ro, rd, ex)
    assert ((f >= 0) & (f < 64)).sum() > 50


def tree_bytes(scene):
    return [rows(x) if x.dtype.names else x for x in mcpt.debug_bvh4_download(scene)]


def test_determinism(veach):
    new = moved_plate(veach)
    arr = with_range(veach, PLATE[0], new)
    scene = fresh(veach)
    mcpt.primary_hits(scene, mcpt.Camera.reference(8, 6))
    scene.update(PLATE[0], new)
    scene.rebuild()
    first = tree_bytes(scene)
    scene.rebuild()  # into the other set of arrays
    second = tree_bytes(scene)
    scene.rebuild()  # and back into the first
    third = tree_bytes(scene)
    other = fresh(arr)
    mcpt.primary_hits(other, mcpt.Camera.reference(8, 6))
    other.rebuild()
    for name, t in (("second", second), ("third", third), ("fresh scene", tree_bytes(other))):
        for x, y in zip(first, t):
            assert np.array_equal(x, y), name


def test_updates_refit_the_new_tree(veach):
    cam = mcpt.Camera.reference(32, 24)
    scene = fresh(veach)
    mcpt.primary_hits(scene, cam)
    new = moved_plate(veach)
    scene.update(PLATE[0], new)
    st = scene.rebuild()
    n0, q0, lf0 = check_rebuilt(scene, st, scene.nfacets)
    new_b = moved_plate(veach, PLATE_B, (-0.3, 0.5, 0.4))
    u1 = scene.update(PLATE_B[0], new_b)
    n1, q1, lf1 = mcpt.debug_bvh4_download(scene)
    moved = np.zeros(scene.nfacets, bool)
    moved[PLATE_B[0]:PLATE_B[1]] = True
    dirty = dirty_nodes(n0, lf0, moved)  # in the NEW topology
    assert np.array_equal(lf0, lf1) and np.array_equal(n0["child"], n1["child"]) and np.array_equal(q0["child"], q1["child"])
    assert u1["nodes_refit"] == dirty.sum() and u1["levels"] == st["levels"] and u1["device_states"] == 1, (u1, dirty.sum())
    assert np.array_equal(rows(n0)[~dirty], rows(n1)[~dirty]) and np.array_equal(rows(q0)[~dirty], rows(q1)[~dirty])
    assert (rows(n0)[dirty] != rows(n1)[dirty]).any()
    newer = translated(new, (0.2, -0.1, 0.3))
    u2 = scene.update(PLATE[0], newer)
    moved[:] = False
    moved[PLATE[0]:PLATE[1]] = True
    assert u2["nodes_refit"] == dirty_nodes(n0, lf0, moved).sum()
    arr = with_range(with_range(veach, PLATE[0], newer), PLATE_B[0], new_b)
    check_device(scene, scene.nfacets)
    assert_arrays_equal(scene.arrays(), fresh(arr).arrays())
    f1, t1 = mcpt.primary_hits(scene, cam)
    f2, t2 = mcpt.primary_hits(fresh(arr), cam)
    assert np.array_equal(f1, f2) and np.array_equal(t1, t2)
    ro, rd, ex = edge_rays(arr, 600, 3, focus=PLATE)
    assert_hits_equal_brute_force(scene, arr, ro, rd, ex)


def test_transforms_and_the_lazy_host_copy(veach):
    cam = mcpt.Camera.reference(32, 24)
    scene = fresh(veach)
    scene.rest_save()
    mcpt.primary_hits(scene, cam)
    a, b = PLATE
    scene.transform(a, b - a, plate_move(veach, 20.0))
    pending = scene.host_pending()
    assert pending == b - a
    st = scene.rebuild()
    assert scene.host_pending() == pending  # the rebuild neither read nor synced the host copy
    m = plate_move(veach, 50.0)
    t = scene.transform(a, b - a, m)
    assert t["levels"] == st["levels"] and t["device_states"] == 1 and scene.host_pending() == pending
    want = with_transform(veach, PLATE, m)
    f1, t1 = mcpt.primary_hits(scene, cam)  # still no sync
    assert scene.host_pending() == pending
    f2, t2 = mcpt.primary_hits(fresh(want), cam)
    assert np.array_equal(f1, f2) and np.array_equal(t1, t2)
    assert_arrays_equal(scene.arrays(), fresh(want).arrays())  # the header's rule; this read syncs
    assert scene.host_pending() == 0
    check_device(scene, scene.nfacets)


def test_previous_pose_is_untouched(veach):
    cam = mcpt.Camera.reference(W, H)
    new = moved_plate(veach)
    out = []
    for rebuild in (False, True):
        scene = fresh(veach)
        mcpt.primary_hits(scene, cam)
        scene.pose_save()
        scene.update(PLATE[0], new)
        if rebuild:
            scene.rebuild()
        out.append(mcpt.render_motion_aovs(scene, cam))
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
    aov = mcpt.render_aovs(fresh(with_range(veach, PLATE[0], new)), cam)
    assert not np.array_equal(out[1]["prev_position"], aov["position"])  # the plate is in view: the pose does differ


@pytest.mark.parametrize("mode", ["mis", "brdf", "shade", "shade_area"])
def test_frames_equal_a_fresh_scene(veach, mode):
    cam = mcpt.Camera.reference(W, H)
    scene = fresh(veach)
    mcpt.render(scene, cam, 1, mode=mode, seed=SEED)
    new = moved_plate(veach)
    scene.update(PLATE[0], new)
    scene.rebuild()
    got = mcpt.render(scene, cam, SPP, mode=mode, seed=SEED)[0]
    want = mcpt.render(fresh(with_range(veach, PLATE[0], new)), cam, SPP, mode=mode, seed=SEED)[0]
    assert_tight(got, want, "rebuilt vs fresh, %s" % mode)


def test_frame_sequence_sees_a_rebuild_between_frames(veach):
    scene = fresh(veach)
    cam = mcpt.Camera.reference(W, H)
    seq = mcpt.FrameSequence(scene, W, H, SPP, denoise=False)
    seq.frame(cam, SEED)
    new = moved_plate(veach)
    scene.update(PLATE[0], new)
    scene.rebuild()
    seq.frame(cam, SEED + 1)
    raw = seq.read("raw")
    seq.close()
    want = mcpt.render(fresh(with_range(veach, PLATE[0], new)), cam, SPP, mode="mis", seed=SEED + 1)[0]
    assert_tight(raw, want, "sequence frame after a rebuild")


def test_tree_cost_is_the_header_formula_and_reproducible(veach):
    scene = fresh(veach)
    c0 = scene.tree_cost()  # creates the device state
    assert c0 == scene.tree_cost() and c0 > 0
    want = tree_cost_numpy(mcpt.debug_bvh4_download(scene)[0])
    assert abs(c0 - want) <= 1e-12 * want, (c0, want)
    scene.update(PLATE[0], moved_plate(veach))
    c1 = scene.tree_cost()
    want = tree_cost_numpy(mcpt.debug_bvh4_download(scene)[0])
    assert abs(c1 - want) <= 1e-12 * want and c1 != c0, (c1, want, c0)
    st = scene.rebuild()
    c2 = scene.tree_cost(device=0)
    want = tree_cost_numpy(mcpt.debug_bvh4_download(scene)[0])
    assert abs(c2 - want) <= 1e-12 * want, (c2, want)
    assert st["cost_before"] == c1 and st["cost_after"] == c2 == scene.tree_cost()


def count_frame(scene, cam):
    img, s = mcpt.render(scene, cam, 2, mode="brdf", seed=SEED, flags=mcpt.DEBUG_COUNT_TRAVERSAL)
    return img, int(s.node_visits) + int(s.tri_tests)


def test_quality_on_the_needles(needles):
    """every tenth needle (7 000 scattered ones) moved by a quarter of the extent: the refit tree, the rebuilt tree and
    a fresh SAH tree of the same arrays.  Measured on the MI355X: V_rebuilt / V_fresh =
    NEEDLES_VISITS_RATIO; the counts have no run-to-run noise, the factor 1.5 leaves room for builder tuning."""
    cam = mcpt.Camera.reference(32, 24)
    nf = len(needles["positions"])
    first = nf - 70000
    idx = np.arange(first, nf, 10)
    assert len(idx) == 7000
    pos = needles["positions"].copy()
    pos[idx] = translated(pos[idx], (2.5, 0.0, 0.0))  # a quarter of the 10-unit box, inside the arena
    arr = dict(needles, positions=pos)
    scene = fresh(needles)
    mcpt.primary_hits(scene, cam)
    c_start = scene.tree_cost()
    scene.update(first, pos[first:])  # one call over the needles: the unmoved ones get their own positions again
    c_refit = scene.tree_cost()
    img_refit, v_refit = count_frame(scene, cam)
    st = scene.rebuild()
    check_rebuilt(scene, st, nf)
    c_rebuilt = scene.tree_cost()
    img_rebuilt, v_rebuilt = count_frame(scene, cam)
    ref = fresh(arr)
    c_fresh = ref.tree_cost()
    img_fresh, v_fresh = count_frame(ref, cam)
    print("needles: cost start %.2f refit %.2f rebuilt %.2f fresh %.2f; visits + tests refit %d rebuilt %d fresh %d "
          "(rebuilt / fresh %.4f, refit / rebuilt %.3f); %d nodes on %d levels, stack need %d, %.3f ms device"
          % (c_start, c_refit, c_rebuilt, c_fresh, v_refit, v_rebuilt, v_fresh, v_rebuilt / v_fresh, v_refit / v_rebuilt,
             st["nodes"], st["levels"], st["stack_need"], st["device_seconds"] * 1e3))
    assert st["cost_before"] == c_refit and st["cost_after"] == c_rebuilt
    assert c_refit > c_start
    assert c_rebuilt < c_refit and v_rebuilt < v_refit  # the point of the feature
    assert v_rebuilt <= 1.5 * NEEDLES_VISITS_RATIO * v_fresh
    assert_tight(img_rebuilt, img_fresh, "needles, rebuilt vs fresh")
    assert_tight(img_refit, img_fresh, "needles, refit vs fresh")
    f1, t1 = mcpt.primary_hits(scene, cam)
    f2, t2 = mcpt.primary_hits(ref, cam)
    assert np.array_equal(f1, f2) and np.array_equal(t1, t2)


def test_cli_rebuild(tmp_path):
    # a move far enough to raise the stand-in's tree cost by 1.6 % (its 3 012 light triangles do not move)
    plain, fp = run_cli(tmp_path, "plain", "--move", "36:12:5,5,3")
    reb, fr = run_cli(tmp_path, "rebuilt", "--move", "36:12:5,5,3", "--rebuild", "1.01")
    assert plain.returncode == 0 and reb.returncode == 0, (plain.stderr, reb.stderr)
    assert "rebuilt the tree before frame 1" in reb.stdout and "rebuilt the tree" not in plain.stdout, reb.stdout
    for k, (a, b) in enumerate(zip(fp, fr)):
        # the PFM is float32 of renders that differ by the order of the fp64 atomics (1e-16 relative): a value changes
        # only where that crosses a float32 rounding boundary
        assert_tight(read_pfm(b), read_pfm(a), "CLI frame %d, with and without --rebuild" % k)
