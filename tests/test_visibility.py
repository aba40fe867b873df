"""mcpt_scene_set_visible on the GPU (include/mcpt.h).  The yardstick everywhere is a fresh
Scene.create of the arrays WITHOUT the hidden facets (rows dropped, light_facet and every exclude id mapped through the
monotone old -> new index map, returned ids mapped back) and the fp64 brute force of tests/bruteforce.py over the visible
facets: never the code under test.  The map is monotone, so "ties to the lower facet id" is preserved, and the frames'
RNG does not see facet ids.  The host half is tests/test_visibility_cpu.py.

The Veach stand-in has 72 non-light facets; the plate [36, 48) covers 128 of the 768 pixels at 32 x 24 (fp64 brute force
on the CPU)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE_OBJ, SCENE_XML, TIGHT_L2, TIGHT_PX
import monte_carlo_path_tracing_amd as mcpt
import scenegen
from bruteforce import brute_force
from test_gpu_parity import max_px_rel, rel_l2
from test_scene_update_cpu import fresh, non_light_runs, translated

pytestmark = pytest.mark.gpu
SEED = 20240430
W, H, SPP = 16, 12, 3
PLATE = (36, 48)
NP = PLATE[1] - PLATE[0]
STEP = (0.7, 0.9, 0.3)
MODES = ("mis", "brdf", "shade", "shade_area")
CLI = os.path.join(ROOT, "monte_carlo_path_tracing_amd", "mcpt_render")
SCENE_BASE = os.path.splitext(str(SCENE_OBJ))[0]


@pytest.fixture(scope="module")
def veach():
    return mcpt.Scene.load(SCENE_OBJ, SCENE_XML).arrays()


class Without:
    """the arrays without the facets of the bool mask `hidden`, and the index maps between the two numberings"""

    def __init__(self, arr, hidden):
        keep = ~hidden
        self.new_of_old = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
        self.old_of_new = np.flatnonzero(keep).astype(np.int32)
        self.arr = {k: v.copy() for k, v in arr.items()}
        for k in ("positions", "normals", "material_id"):
            self.arr[k] = arr[k][keep]
        if "unique_normal" in arr:
            self.arr["unique_normal"] = arr["unique_normal"][keep]
        self.arr["light_facet"] = self.new_of_old[arr["light_facet"]]
        assert (self.arr["light_facet"] >= 0).all()

    def exclude(self, ex):
        ex = np.asarray(ex, np.int32)
        return np.where(ex >= 0, self.new_of_old[np.maximum(ex, 0)], -1).astype(np.int32)

    def back(self, f):
        f = np.asarray(f)
        return np.where(f >= 0, self.old_of_new[np.maximum(f, 0)], -1).astype(np.int32)

    def scene(self):
        return fresh(self.arr)

    def closest_hit(self, ro, rd, ex, scene=None):
        f, tbg = mcpt.closest_hit(scene or self.scene(), ro, rd, self.exclude(ex))
        return self.back(f), tbg

    def primary_hits(self, cam):
        f, tbg = mcpt.primary_hits(self.scene(), cam)
        return self.back(f), tbg

    def brute_force(self, ro, rd, ex):
        return self.back(brute_force(self.arr, ro, rd, self.exclude(ex))[0])


def mask(arr, *ranges):
    m = np.zeros(len(arr["positions"]), bool)
    for a, b in ranges:
        m[a:b] = True
    return m


def with_range(arr, first, new):
    out = {k: v.copy() for k, v in arr.items()}
    out["positions"][first:first + len(new)] = new
    return out


@pytest.fixture(scope="module")
def no_plate(veach):
    return Without(veach, mask(veach, PLATE))


@pytest.fixture(scope="module")
def no_plate_hits(no_plate):
    return no_plate.primary_hits(mcpt.Camera.reference(32, 24))


@pytest.fixture(scope="module")
def full_hits(veach):
    return mcpt.primary_hits(fresh(veach), mcpt.Camera.reference(32, 24))


def check_device(scene):
    r = mcpt.debug_bvh4_check_device(scene)
    assert r["errors"] == 0 and r["tris"] == r["facets"] == scene.nfacets, r
    return r


def assert_tight(got, want, what):
    l2, px = rel_l2(got, want), max_px_rel(got, want)
    print("%s: rel L2 %.3e, max pixel %.3e" % (what, l2, px))
    assert l2 <= TIGHT_L2 and px <= TIGHT_PX, (what, l2, px)


def assert_hits(got, want):
    assert np.array_equal(got[0], want[0])
    hit = want[0] >= 0
    assert np.array_equal(got[1][hit], want[1][hit])


def vertex_rays(arr, aim, n=3000, seed=7):
    """test_closest_hit_at_the_arena_limit's rays: vertices, edge points and +-ulp targets from far and near origins,
    a third of them aimed at the facets [aim[0], aim[1]), a fifth excluding their target"""
    P = arr["positions"].astype(np.float64).reshape(-1, 3, 3)
    rng = np.random.default_rng(seed)
    tri = rng.integers(0, len(P), n)
    tri[::3] = rng.integers(aim[0], aim[1], len(tri[::3]))
    kind = rng.integers(0, 3, n)
    w = rng.random((n, 3))
    w[kind == 0] = np.eye(3)[rng.integers(0, 3, (kind == 0).sum())]  # a vertex
    e = rng.integers(0, 3, n)
    w[(kind == 1), e[kind == 1]] = 0.0  # a point on an edge
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
    return ro, rd, ex, tri


def test_primary_hits_equal_a_fresh_scene_without_the_plate(veach, no_plate_hits, full_hits):
    cam = mcpt.Camera.reference(32, 24)
    scene = fresh(veach)
    f0, t0 = mcpt.primary_hits(scene, cam)  # the device state exists before the call
    assert np.array_equal(f0, full_hits[0])
    st = scene.hide(PLATE[0], NP)
    assert st["device_states"] == 1 and st["facets"] == NP and st["leaf_slots"] >= NP and st["nodes_refit"] >= 1, st
    assert st["levels"] >= 2 and st["device_seconds"] > 0, st
    got = mcpt.primary_hits(scene, cam)
    assert_hits(got, no_plate_hits)
    changed = got[0] != f0
    on_plate = (f0 >= PLATE[0]) & (f0 < PLATE[1])
    print("%d pixels changed, %d showed the plate" % (changed.sum(), on_plate.sum()))
    assert changed.sum() == 128 and np.array_equal(changed, on_plate)
    assert not ((got[0] >= PLATE[0]) & (got[0] < PLATE[1])).any()
    check_device(scene)
    assert scene.hidden_count() == NP and scene.nfacets == len(veach["positions"])


def test_closest_hit_equals_the_fresh_scene_and_the_brute_force(veach, no_plate):
    scene = fresh(veach)
    mcpt.primary_hits(scene, mcpt.Camera.reference(8, 6))
    scene.hide(PLATE[0], NP)
    ro, rd, ex, tri = vertex_rays(veach, PLATE)
    f, tbg = mcpt.closest_hit(scene, ro, rd, ex)
    f2, tbg2 = no_plate.closest_hit(ro, rd, ex)
    assert_hits((f, tbg), (f2, tbg2))
    assert np.array_equal(f, no_plate.brute_force(ro, rd, ex))
    assert not ((f >= PLATE[0]) & (f < PLATE[1])).any()
    aimed = (tri >= PLATE[0]) & (tri < PLATE[1])
    behind = aimed & (f >= 0)
    print("%d/%d rays hit, %d of the %d aimed at the hidden plate hit something behind it" % ((f >= 0).sum(), len(f), behind.sum(),
                                                                                              aimed.sum()))
    assert behind.sum() > 100


@pytest.fixture(scope="module")
def untouched_frames(veach):
    scene = fresh(veach)
    cam = mcpt.Camera.reference(W, H)
    return {m: mcpt.render(scene, cam, SPP, mode=m, seed=SEED)[0] for m in MODES}


@pytest.mark.parametrize("mode", MODES)
def test_frames_equal_a_fresh_scene_without_the_plate(veach, no_plate, untouched_frames, mode):
    cam = mcpt.Camera.reference(W, H)
    scene = fresh(veach)
    mcpt.render(scene, cam, 1, mode=mode, seed=SEED)
    scene.hide(PLATE[0], NP)
    got = mcpt.render(scene, cam, SPP, mode=mode, seed=SEED)[0]
    want = mcpt.render(no_plate.scene(), cam, SPP, mode=mode, seed=SEED)[0]
    assert_tight(got, want, "hidden vs fresh without, %s" % mode)
    d = rel_l2(got, untouched_frames[mode])
    print("distance from the untouched frame: %.3e" % d)
    assert d > 1e3 * TIGHT_L2


def rows(a):
    return a.view(np.uint8).reshape(len(a), -1)


def test_hide_then_show_is_the_untouched_scene_and_the_same_refit(veach, full_hits):
    cam = mcpt.Camera.reference(32, 24)
    scene, moved = fresh(veach), fresh(veach)
    for s in (scene, moved):
        mcpt.primary_hits(s, cam)
    scene.hide(PLATE[0], NP)
    st = scene.show(PLATE[0], NP)
    su = moved.update(PLATE[0], veach["positions"][PLATE[0]:PLATE[1]])  # the same refit over the same slots
    for k in ("facets", "leaf_slots", "nodes_refit", "levels", "device_states"):
        assert st[k] == su[k], (k, st, su)
    assert_hits(mcpt.primary_hits(scene, cam), full_hits)
    a, b = mcpt.debug_bvh4_download(scene), mcpt.debug_bvh4_download(moved)
    assert np.array_equal(rows(a[0]), rows(b[0])) and np.array_equal(rows(a[1]), rows(b[1])) and np.array_equal(a[2], b[2])
    check_device(scene)
    assert scene.hidden_count() == 0
    for m in ("mis",):
        got = mcpt.render(scene, mcpt.Camera.reference(W, H), SPP, mode=m, seed=SEED)[0]
        assert_tight(got, mcpt.render(fresh(veach), mcpt.Camera.reference(W, H), SPP, mode=m, seed=SEED)[0], "shown again, %s" % m)


def test_update_while_hidden(veach, no_plate_hits):
    cam = mcpt.Camera.reference(32, 24)
    scene = fresh(veach)
    mcpt.primary_hits(scene, cam)
    scene.hide(PLATE[0], NP)
    new = translated(veach["positions"][PLATE[0]:PLATE[1]], STEP)
    scene.update(PLATE[0], new)
    check_device(scene)
    assert_hits(mcpt.primary_hits(scene, cam), no_plate_hits)  # wherever the hidden plate is, the scene without it
    assert np.array_equal(scene.arrays()["positions"][PLATE[0]:PLATE[1]], new)
    scene.show(PLATE[0], NP)
    check_device(scene)
    want = mcpt.primary_hits(fresh(with_range(veach, PLATE[0], new)), cam)
    assert_hits(mcpt.primary_hits(scene, cam), want)
    assert not np.array_equal(want[0], no_plate_hits[0])


def test_transform_while_hidden(veach, no_plate_hits):
    cam = mcpt.Camera.reference(32, 24)
    scene = fresh(veach)
    mcpt.primary_hits(scene, cam)
    scene.rest_save()
    scene.hide(PLATE[0], NP)
    m = np.concatenate([np.eye(3), np.asarray(STEP, np.float64)[:, None]], axis=1)
    st = scene.transform(PLATE[0], NP, m)
    assert st["device_states"] == 1 and scene.host_pending() == NP
    assert_hits(mcpt.primary_hits(scene, cam), no_plate_hits)
    check_device(scene)  # syncs the host copy: the host tree takes the hidden facets as their points
    scene.show(PLATE[0], NP)
    check_device(scene)
    new = scene.arrays()["positions"][PLATE[0]:PLATE[1]]
    assert not np.array_equal(new, veach["positions"][PLATE[0]:PLATE[1]])
    want = mcpt.primary_hits(fresh(with_range(veach, PLATE[0], new)), cam)
    assert_hits(mcpt.primary_hits(scene, cam), want)
    assert not np.array_equal(want[0], no_plate_hits[0])


def test_rebuild_while_hidden_and_show_after_it(veach, no_plate, no_plate_hits, full_hits):
    cam, fcam = mcpt.Camera.reference(32, 24), mcpt.Camera.reference(W, H)
    scene = fresh(veach)
    mcpt.primary_hits(scene, cam)
    scene.hide(PLATE[0], NP)
    st = scene.rebuild()
    assert st["device_states"] == 1 and st["facets"] == scene.nfacets, st
    check_device(scene)
    assert_hits(mcpt.primary_hits(scene, cam), no_plate_hits)
    got = mcpt.render(scene, fcam, SPP, mode="mis", seed=SEED)[0]
    assert_tight(got, mcpt.render(no_plate.scene(), fcam, SPP, mode="mis", seed=SEED)[0], "rebuilt while hidden, mis")
    scene.show(PLATE[0], NP)
    check_device(scene)
    assert_hits(mcpt.primary_hits(scene, cam), full_hits)
    got = mcpt.render(scene, fcam, SPP, mode="mis", seed=SEED)[0]
    assert_tight(got, mcpt.render(fresh(veach), fcam, SPP, mode="mis", seed=SEED)[0], "shown after the rebuild, mis")
    # and a rebuild after that sees an ordinary scene
    scene.rebuild()
    check_device(scene)
    assert_hits(mcpt.primary_hits(scene, cam), full_hits)


def test_a_device_state_created_after_the_call_honours_the_mask(veach, no_plate_hits):
    cam = mcpt.Camera.reference(32, 24)
    scene, live = fresh(veach), fresh(veach)
    st = scene.hide(PLATE[0], NP)  # before the handle's first device call
    assert st["device_states"] == 0
    got = mcpt.primary_hits(scene, cam)
    assert_hits(got, no_plate_hits)
    assert not ((got[0] >= PLATE[0]) & (got[0] < PLATE[1])).any()
    check_device(scene)
    # its slots and boxes are those of a state that was edited in place
    mcpt.primary_hits(live, cam)
    live.hide(PLATE[0], NP)
    a, b = mcpt.debug_bvh4_download(scene), mcpt.debug_bvh4_download(live)
    assert np.array_equal(rows(a[0]), rows(b[0])) and np.array_equal(rows(a[1]), rows(b[1])) and np.array_equal(a[2], b[2])
    # and it follows later calls: an update while hidden, then show
    new = translated(veach["positions"][PLATE[0]:PLATE[1]], STEP)
    scene.update(PLATE[0], new)
    assert_hits(mcpt.primary_hits(scene, cam), no_plate_hits)
    scene.show(PLATE[0], NP)
    check_device(scene)
    assert_hits(mcpt.primary_hits(scene, cam), mcpt.primary_hits(fresh(with_range(veach, PLATE[0], new)), cam))


def test_needles_spatial_splits_whole_leaves_and_subtrees(tmp_path_factory):
    obj, xml = scenegen.needles(str(tmp_path_factory.mktemp("needles")))
    arr = mcpt.Scene.load(obj, xml).arrays()
    F = len(arr["positions"])
    assert F > 70000 and non_light_runs(arr) == [(0, F)]  # 70 000 needles and the floor, no lights
    scene = fresh(arr)
    r0 = check_device(scene)
    assert r0["duplicates"] > 0  # spatial splits: facets with several slots
    rng = np.random.default_rng(9)
    ranges = [(int(a), int(a + c)) for a, c in zip(rng.integers(0, F // 2 - 300, 40), rng.integers(1, 301, 40))]
    ranges.append((F // 2, F))  # one contiguous half: whole leaves and whole subtrees
    slots = 0
    for a, b in ranges:
        slots += scene.hide(a, b - a)["leaf_slots"]
    hidden = mask(arr, *ranges)
    assert slots > hidden.sum() and scene.hidden_count() == hidden.sum() and np.array_equal(scene.visible(), ~hidden)
    check_device(scene)
    wo = Without(arr, hidden)
    # 2 000 rays aimed at hidden and visible needles alike
    P = arr["positions"].astype(np.float64).reshape(-1, 3, 3)
    n = 2000
    tri = np.where(np.arange(n) % 2 == 0, rng.choice(np.flatnonzero(hidden), n), rng.choice(np.flatnonzero(~hidden), n))
    w = rng.random((n, 3))
    w /= w.sum(axis=1, keepdims=True)
    target = np.einsum("nk,nkc->nc", w, P[tri])
    ro = rng.uniform(-5.0, 5.0, (n, 3))
    rd = target - ro
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    ex = np.where(rng.random(n) < 0.2, tri, -1).astype(np.int32)
    f, _ = mcpt.closest_hit(scene, ro, rd, ex)
    bf = wo.brute_force(ro, rd, ex)
    assert np.array_equal(f, bf)
    assert not hidden[f[f >= 0]].any()
    print("%d/%d rays hit; %d facets hidden over %d slots" % ((f >= 0).sum(), n, hidden.sum(), slots))
    assert (f >= 0).sum() > n // 4


def test_tree_cost_does_not_grow(veach):
    scene = fresh(veach)
    before = scene.tree_cost()
    scene.hide(PLATE[0], NP)
    after = scene.tree_cost()
    print("tree cost %.6f -> %.6f" % (before, after))
    assert after <= before  # every box is a subset of its old self


def sequence_frames(veach):
    """FrameSequence (16 x 12, 2 spp, static camera, 4 frames, no filter), the plate hidden between frames 2 and 3"""
    scene = fresh(veach)
    cam = mcpt.Camera.reference(W, H)
    seq = mcpt.FrameSequence(scene, W, H, 2, denoise=False)
    frames = []
    for k in range(4):
        if k == 2:
            scene.hide(PLATE[0], NP)
        rgb8 = seq.frame(cam, SEED + k)
        frames.append(dict(rgb8=rgb8, raw=seq.read("raw"), accumulated=seq.read("accumulated")))
    seq.close()
    return frames


@pytest.fixture(scope="module")
def seq_frames(veach):
    return sequence_frames(veach)


def test_sequence_sees_the_call_between_frames(veach, no_plate, seq_frames):
    cam = mcpt.Camera.reference(W, H)
    full, without = fresh(veach), no_plate.scene()
    assert_tight(seq_frames[2]["raw"], mcpt.render(without, cam, 2, mode="mis", seed=SEED + 2)[0], "raw frame 3")
    assert rel_l2(seq_frames[2]["raw"], mcpt.render(full, cam, 2, mode="mis", seed=SEED + 2)[0]) > 1e3 * TIGHT_L2
    acc = mcpt.TemporalAccumulator()
    for k in range(4):
        s = full if k < 2 else without
        c, _ = acc.push(cam, mcpt.render(s, cam, 2, mode="mis", seed=SEED + k)[0], mcpt.render_aovs(s, cam))
        if k >= 2:
            assert_tight(seq_frames[k]["accumulated"], c, "accumulated frame %d" % (k + 1))


def read_bmp(path):
    """the 32-bpp bottom-up B G R 0 layout of mcpt_write_bmp -> H x W x 3 uint8, row 0 on top"""
    raw = open(path, "rb").read()
    ww, hh = int.from_bytes(raw[18:22], "little"), int.from_bytes(raw[22:26], "little")
    px = np.frombuffer(raw, np.uint8, offset=int.from_bytes(raw[10:14], "little")).reshape(hh, ww, 4)
    return px[::-1, :, 2::-1].copy()


def cli(tmp_path, tag, *args):
    return subprocess.run([CLI, "--scene", SCENE_BASE, "--out", str(tmp_path / (tag + ".bmp")), "--width", str(W), "--height", str(H),
                           "--spp", "2", "--seed", str(SEED), *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("extra", [[], ["--device-sequence"]], ids=["host-sequence", "device-sequence"])
def test_cli_hide_writes_the_sequence_of_the_python_api(tmp_path, seq_frames, extra):
    from test_sequence import undecided
    r = cli(tmp_path, "hid", "--frames", "4", "--hide", "36:12:2", *extra)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("hid facets [36, 48)") == 1, r.stdout
    differ = 0
    for k in range(4):
        got = read_bmp(str(tmp_path / ("hid_%04d.bmp" % k)))
        # rendered anew: the frames are the sequence's up to the summation order, which moves a level only where the
        # tone map's t sits on an integer
        d = got.astype(int) - seq_frames[k]["rgb8"].astype(int)
        assert (np.abs(d) <= undecided(seq_frames[k]["accumulated"])).all(), k
        differ += (d != 0).sum()
    print("%d of %d bytes differ" % (differ, 4 * got.size))


def test_cli_hide_with_the_grid_flag_is_refused(tmp_path):
    r = cli(tmp_path, "grid", "--frames", "2", "--hide", "36:12:1", "--grid")
    assert r.returncode != 0 and "--hide and --show are not supported with --grid" in r.stderr, r.stderr
    # a single frame: hidden before frame 0, the default
    one = cli(tmp_path, "one", "--hide", "36:12", "--hdr", str(tmp_path / "one.pfm"))
    assert one.returncode == 0 and "hid facets [36, 48)" in one.stdout, (one.stdout, one.stderr)


def test_refusals_on_a_live_state_change_nothing(veach, no_plate_hits):
    cam = mcpt.Camera.reference(32, 24)
    scene = fresh(veach)
    mcpt.primary_hits(scene, cam)
    scene.hide(PLATE[0], NP)
    ro, rd, ex, _ = vertex_rays(veach, PLATE, n=64)

    def unchanged():
        assert_hits(mcpt.primary_hits(scene, cam), no_plate_hits)
        assert scene.hidden_count() == NP

    with pytest.raises(mcpt.MCPTError, match="facet 72 is a light triangle"):
        scene.hide(60, 13)
    unchanged()
    with pytest.raises(mcpt.MCPTError, match="facet 72 is a light triangle"):
        scene.show(PLATE[0], 72 - PLATE[0] + 1)
    unchanged()
    with pytest.raises(mcpt.MCPTError, match="refused while facets are hidden"):
        mcpt.render(scene, mcpt.Camera.reference(W, H), 1, mode="mis", seed=SEED, accel="grid")
    unchanged()
    with pytest.raises(mcpt.MCPTError, match="refused while facets are hidden"):
        scene.meshing((0.0, 2.0, 15.0), 1000)
    with pytest.raises(mcpt.MCPTError, match="refused while facets are hidden"):
        mcpt.closest_hit(scene, ro, rd, ex, grid=True)
    unchanged()
    with pytest.raises(mcpt.MCPTError, match="8-wide"):
        mcpt.closest_hit(scene, ro, rd, ex, wide=True)
    unchanged()
    check_device(scene)
    # once everything is shown again the grid modes are back
    scene.show(PLATE[0], NP)
    g = mcpt.render(scene, mcpt.Camera.reference(W, H), SPP, mode="mis", seed=SEED, accel="grid")[0]
    assert_tight(g, mcpt.render(scene, mcpt.Camera.reference(W, H), SPP, mode="mis", seed=SEED)[0], "grid vs BVH once shown")
