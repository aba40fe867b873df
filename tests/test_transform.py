"""mcpt_scene_transform on the GPU (include/mcpt.h): once a device state exists the rule runs in
k_transform_range and the host copy only follows on demand.  Everything is compared with a fresh mcpt_scene_create of
the numpy restatement of the rule (tests/test_transform_cpu.py) -- hits bit for bit, frames up to the order of the
framebuffer's fp64 atomics -- and the device's refit tree passes the host walk.  Run on the MI355X box: `pytest -m gpu`.

Not testable on one GPU, reviewed from the code: a device state created on a second device while ranges are pending."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SCENE_OBJ, SCENE_XML
import monte_carlo_path_tracing_amd as mcpt
import scenegen
from test_gpu_parity import brute_force_hits
from test_scene_update import assert_tight, check_device, dirty_nodes, moved_plate, rows, with_range
from test_scene_update_cpu import arena, float_at_most, fresh
from test_transform_cpu import IDENTITY, PLATE, assert_arrays_equal, centroid, plate_move, restate, with_transform

pytestmark = pytest.mark.gpu
SEED = 20240430
W, H, SPP = 16, 12, 3
PLATE_B = (48, 60)     # the third plate, for the update of a disjoint range
PLATE_FAR = (60, 72)   # the fourth, for the move to the arena's limit
CLI = os.path.join(ROOT, "monte_carlo_path_tracing_amd", "mcpt_render")
SCENE_BASE = os.path.splitext(str(SCENE_OBJ))[0]


@pytest.fixture(scope="module")
def veach():
    return mcpt.Scene.load(SCENE_OBJ, SCENE_XML).arrays()


@pytest.fixture(scope="module")
def needles(tmp_path_factory):
    obj, xml = scenegen.needles(str(tmp_path_factory.mktemp("needles")))
    return mcpt.Scene.load(obj, xml).arrays()


def on_device(arr, cam=None):
    """a fresh scene with its rest pose saved and a device state"""
    scene = fresh(arr)
    scene.rest_save()
    mcpt.primary_hits(scene, cam or mcpt.Camera.reference(8, 6))
    return scene


def test_primary_hits_equal_a_fresh_scene(veach):
    cam = mcpt.Camera.reference(32, 24)
    scene = fresh(veach)
    scene.rest_save()
    f0, t0 = mcpt.primary_hits(scene, cam)  # the device state exists before the transform
    m = plate_move(veach)
    st = scene.transform(PLATE[0], PLATE[1] - PLATE[0], m)
    assert st["device_states"] == 1 and st["nodes_refit"] >= 1 and st["levels"] >= 2 and st["device_seconds"] > 0, st
    assert st["facets"] == 12 and st["leaf_slots"] == 12
    assert scene.host_pending() == 12
    f1, t1 = mcpt.primary_hits(scene, cam)
    f2, t2 = mcpt.primary_hits(fresh(with_transform(veach, PLATE, m)), cam)
    assert np.array_equal(f1, f2) and np.array_equal(t1, t2)
    assert not np.array_equal(f0, f1)  # the plate is in view: the transform did change the map
    assert scene.host_pending() == 12  # a trace reads nothing of the host copy
    check_device(scene, scene.nfacets)  # compares the device's vertices with the host's: this syncs
    assert scene.host_pending() == 0
    assert_arrays_equal(scene.arrays(), fresh(with_transform(veach, PLATE, m)).arrays())
    with pytest.raises(mcpt.MCPTError, match="8-wide"):  # refused at the transform itself, not at the sync
        mcpt.closest_hit(scene, np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]]), wide=True)


def test_closest_hit_at_the_arena_limit_vs_fresh_scene_and_brute_force(veach):
    """test_scene_update's edge / vertex / +-ulp rays after the plate was rotated and pushed to the arena's far corner"""
    scene = on_device(veach)
    a, b = PLATE_FAR
    rot = mcpt.transform_rotation((0.2, 1.0, -0.3), 40.0, centroid(veach, PLATE_FAR))
    _, hi = arena(veach)
    top = float_at_most(hi)
    turned = restate(veach["positions"][a:b], veach["normals"][a:b], rot)[0].astype(np.float64).reshape(-1, 3)
    # four float32 steps inside the limit: the sum's double rounding and the conversion can each move the result by one
    m = rot.copy()
    m[:, 3] += (top.astype(np.float64) - 4 * np.spacing(top).astype(np.float64)) - turned.max(axis=0)
    arr = with_transform(veach, PLATE_FAR, m)
    new = arr["positions"][a:b].reshape(-1, 3)
    assert (new.max(axis=0).astype(np.float64) <= hi).all() and (new.max(axis=0) >= top - 8 * np.spacing(top)).all()
    scene.transform(a, b - a, m)
    P = arr["positions"].astype(np.float64).reshape(-1, 3, 3)
    rng = np.random.default_rng(7)
    n = 3000
    tri = rng.integers(0, len(P), n)
    tri[::3] = rng.integers(a, b, len(tri[::3]))
    kind = rng.integers(0, 3, n)
    w = rng.random((n, 3))
    w[kind == 0] = np.eye(3)[rng.integers(0, 3, (kind == 0).sum())]  # a vertex
    e = rng.integers(0, 3, n)
    w[(kind == 1), e[kind == 1]] = 0.0  # a point on an edge
    w /= w.sum(axis=1, keepdims=True)
    target = np.einsum("nk,nkc->nc", w, P[tri])
    target *= 1.0 + rng.choice([0.0, 1e-15, -1e-15, 1e-12, -1e-12], (n, 1))
    lo, hi_ = P.reshape(-1, 3).min(axis=0), P.reshape(-1, 3).max(axis=0)
    ro = lo + rng.random((n, 3)) * (hi_ - lo)
    near = rng.random(n) < 0.3
    ro[near] = target[near] + rng.normal(0, 0.05, (near.sum(), 3))
    rd = target - ro
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    ex = np.where(rng.random(n) < 0.2, tri, -1).astype(np.int32)
    f, tbg = mcpt.closest_hit(scene, ro, rd, ex)
    f2, tbg2 = mcpt.closest_hit(fresh(arr), ro, rd, ex)
    assert np.array_equal(f, f2) and np.array_equal(tbg, tbg2)
    bf = brute_force_hits(arr, np.concatenate([ro, rd, ex[:, None]], axis=1), False)
    assert np.array_equal(f, bf)
    on_plate = (f >= a) & (f < b)
    print("%d/%d rays hit, %d of them the transformed plate" % ((f >= 0).sum(), n, on_plate.sum()))
    assert on_plate.sum() > 100
    assert scene.host_pending() == 12
    check_device(scene, scene.nfacets)


@pytest.mark.parametrize("first,count", [(40, 1), (36, 12), (5, 63), (3, 65), (0, 72)], ids=["1", "12", "63", "65", "all-non-light"])
def test_ranges_on_the_stand_in(veach, first, count):
    """errors == 0 on the device tree; nodes off the dirty paths bit-identical; nodes_refit as Scene.update's"""
    scene = fresh(veach)
    scene.rest_save()
    n0, q0, lf = mcpt.debug_bvh4_download(scene)
    rng_ = (first, first + count)
    m = mcpt.transform_rotation((0.1, 1.0, 0.4), 12.0, centroid(veach, rng_), (-0.4, 0.6, 0.8))
    st = scene.transform(first, count, m)
    assert scene.host_pending() == count
    check_device(scene, scene.nfacets)
    n1, q1, lf1 = mcpt.debug_bvh4_download(scene)
    moved = np.zeros(scene.nfacets, bool)
    moved[first:first + count] = True
    dirty = dirty_nodes(n0, lf, moved)
    assert np.array_equal(lf, lf1) and np.array_equal(n0["child"], n1["child"]) and np.array_equal(q0["child"], q1["child"])
    assert np.array_equal(rows(n0)[~dirty], rows(n1)[~dirty]) and np.array_equal(rows(q0)[~dirty], rows(q1)[~dirty])
    assert (rows(n0)[dirty] != rows(n1)[dirty]).any()
    other = fresh(veach)
    mcpt.debug_bvh4_download(other)
    want = with_transform(veach, rng_, m)
    su = other.update(first, want["positions"][first:first + count], want["normals"][first:first + count])
    assert st["nodes_refit"] == su["nodes_refit"] == dirty.sum() and st["leaf_slots"] == su["leaf_slots"] == count, (st, su)
    assert st["levels"] == su["levels"] and st["facets"] == count
    for x, y in zip((n1, q1, lf1), mcpt.debug_bvh4_download(other)):  # and the refit trees are the same bits
        assert np.array_equal(rows(x) if x.dtype.names else x, rows(y) if y.dtype.names else y)


@pytest.mark.parametrize("count", [257, 1000])
def test_needles_spatial_split_tree(needles, count):
    """a range that crosses the 256-thread block, facets with several leaf slots"""
    cam = mcpt.Camera.reference(32, 24)
    scene = on_device(needles, cam)
    first = 30000
    rng_ = (first, first + count)
    m = mcpt.transform_rotation((1.0, 0.5, -0.25), 50.0, centroid(needles, rng_), (0.1, 0.0, -0.1))
    st = scene.transform(first, count, m)
    assert st["leaf_slots"] > count and st["levels"] >= 6 and scene.host_pending() == count, st
    want = with_transform(needles, rng_, m)
    f1, t1 = mcpt.primary_hits(scene, cam)
    f2, t2 = mcpt.primary_hits(fresh(want), cam)
    assert np.array_equal(f1, f2) and np.array_equal(t1, t2)
    r = check_device(scene, scene.nfacets)
    assert r["duplicates"] > 0
    got = scene.arrays()
    assert np.array_equal(got["positions"], want["positions"]) and np.array_equal(got["normals"], want["normals"])


def test_many_scattered_ranges_collapse_to_their_hull(needles):
    """the pending list holds at most 48 ranges: the 49th disjoint one turns it into the hull, which a sync then copies
    back whole -- facets in the gaps included, unchanged"""
    scene = on_device(needles)
    want = needles
    first, stride = 30000, 3
    for i in range(50):
        f = first + stride * i
        m = mcpt.transform_rotation((0.0, 1.0, 0.0), 5.0 + i, centroid(needles, (f, f + 1)))
        scene.transform(f, 1, m)
        want = with_transform(want, (f, f + 1), m, rest=needles)
        # 48 singles; the 49th makes the hull [first, first + 3 * 48 + 1); the 50th is a single beside it again
        expect = i + 1 if i < 48 else stride * 48 + 1 + (i - 48)
        assert scene.host_pending() == expect, (i, scene.host_pending())
    scene.transform(first + 1, 1, IDENTITY)  # inside the hull: nothing new is pending
    assert scene.host_pending() == stride * 48 + 2
    got = scene.arrays()
    assert scene.host_pending() == 0
    assert np.array_equal(got["positions"], want["positions"]) and np.array_equal(got["normals"], want["normals"])
    assert np.array_equal(got["unique_normal"], fresh(want).arrays()["unique_normal"])
    check_device(scene, scene.nfacets)


@pytest.mark.parametrize("mode", ["mis", "brdf", "shade"])
def test_frames_equal_a_fresh_scene(veach, mode):
    cam = mcpt.Camera.reference(W, H)
    scene = fresh(veach)
    scene.rest_save()
    still = mcpt.render(scene, cam, SPP, mode=mode, seed=SEED)[0]
    m = plate_move(veach)
    scene.transform(PLATE[0], PLATE[1] - PLATE[0], m)
    got = mcpt.render(scene, cam, SPP, mode=mode, seed=SEED)[0]
    want = mcpt.render(fresh(with_transform(veach, PLATE, m)), cam, SPP, mode=mode, seed=SEED)[0]
    assert_tight(got, want, "transformed vs fresh, %s" % mode)
    assert not np.array_equal(got, still)  # and the plate's new pose shows
    assert scene.host_pending() == 12  # a render reads nothing of the host copy


def test_transform_and_update_of_disjoint_ranges_in_either_order(veach):
    cam = mcpt.Camera.reference(32, 24)
    m = plate_move(veach)
    new_b = moved_plate(veach, PLATE_B, (-0.3, 0.5, 0.4))
    want = with_range(with_transform(veach, PLATE, m), PLATE_B[0], new_b)
    ref = fresh(want)
    fr, tr = mcpt.primary_hits(ref, cam)
    one, two = on_device(veach, cam), on_device(veach, cam)
    one.transform(PLATE[0], 12, m)
    assert one.host_pending() == 12
    one.update(PLATE_B[0], new_b)  # the update's host refit needs a current host copy: it syncs first
    assert one.host_pending() == 0
    two.update(PLATE_B[0], new_b)
    two.transform(PLATE[0], 12, m)
    assert two.host_pending() == 12
    for s in (one, two):
        f, t = mcpt.primary_hits(s, cam)
        assert np.array_equal(f, fr) and np.array_equal(t, tr)
        assert_arrays_equal(s.arrays(), ref.arrays())
        check_device(s, s.nfacets)
        assert mcpt.debug_bvh4_check(s)["errors"] == 0
    # rest_save after an update makes the updated pose the rest: the identity on plate B keeps its updated pose, and
    # a transform of it starts there
    one.rest_save()
    one.transform(PLATE_B[0], 12, IDENTITY)
    assert_arrays_equal(one.arrays(), ref.arrays())
    mb = mcpt.transform_rotation((0, 1, 0), 20.0, centroid(want, PLATE_B))
    one.transform(PLATE_B[0], 12, mb)
    again = fresh(with_transform(want, PLATE_B, mb))
    f, t = mcpt.primary_hits(one, cam)
    f2, t2 = mcpt.primary_hits(again, cam)
    assert np.array_equal(f, f2) and np.array_equal(t, t2)
    assert_arrays_equal(one.arrays(), again.arrays())


def test_refused_transforms_change_nothing(veach):
    cam = mcpt.Camera.reference(32, 24)
    scene = on_device(veach, cam)
    m = plate_move(veach)
    scene.transform(PLATE[0], 12, m)
    before = mcpt.primary_hits(scene, cam)
    assert scene.host_pending() == 12
    with pytest.raises(mcpt.MCPTError, match="outside the arena"):  # the plate scaled by 100 about the origin
        scene.transform(PLATE[0], 12, IDENTITY * 100.0, np.eye(3))
    with pytest.raises(mcpt.MCPTError, match="non-finite"):
        scene.transform(PLATE[0], 12, IDENTITY * 1e39, np.eye(3))
    with pytest.raises(mcpt.MCPTError, match="non-finite"):
        scene.transform(PLATE[0], 12, IDENTITY, np.eye(3) * 1e39)
    with pytest.raises(mcpt.MCPTError, match="facet 72 is a light triangle"):
        scene.transform(70, 4, m)
    late = fresh(veach)
    mcpt.primary_hits(late, cam)
    with pytest.raises(mcpt.MCPTError, match="no rest pose"):
        late.transform(PLATE[0], 12, m)
    after = mcpt.primary_hits(scene, cam)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert scene.host_pending() == 12
    check_device(scene, scene.nfacets)
    assert_arrays_equal(scene.arrays(), fresh(with_transform(veach, PLATE, m)).arrays())


def test_sequence_with_motion_never_syncs_the_host(veach):
    """pose_save + transform per frame against pose_save + Scene.update of the restated arrays, the same seeds"""
    cam = mcpt.Camera.reference(16, 12)
    a, b = PLATE
    arms = []
    for _ in range(2):
        scene = fresh(veach)
        scene.rest_save()
        arms.append((scene, mcpt.FrameSequence(scene, 16, 12, 1, denoise=False, motion=True)))
    (st, sq_t), (su, sq_u) = arms
    for k in range(4):
        m = plate_move(veach, 10.0 * k)
        new = with_transform(veach, PLATE, m)
        st.pose_save()
        su.pose_save()
        if k:
            st.transform(a, b - a, m)
            su.update(a, new["positions"][a:b], new["normals"][a:b])
        sq_t.frame(cam, SEED + k)
        sq_u.frame(cam, SEED + k)
        for name in ("accumulated", "moments", "prev_position"):
            assert np.array_equal(sq_t.read(name), sq_u.read(name)), (k, name)
    assert st.host_pending() > 0  # three frames of pose_save + transform and nothing synced
    st.host_sync()
    assert st.host_pending() == 0
    assert_arrays_equal(st.arrays(), su.arrays())
    # the host's previous pose followed too: a state made from the host copy now would get frame 2's pose
    mo_t, mo_u = mcpt.render_motion_aovs(st, cam), mcpt.render_motion_aovs(su, cam)
    assert np.array_equal(mo_t["prev_position"], mo_u["prev_position"])
    sq_t.close()
    sq_u.close()


def run_cli(tmp_path, tag, pivot, *args):
    out = str(tmp_path / (tag + ".bmp"))
    r = subprocess.run([CLI, "--scene", SCENE_BASE, "--out", out, "--width", "32", "--height", "24", "--spp", "2", "--frames", "3",
                        "--rotate", "36:12:0.3,1,0.2:15:%r,%r,%r" % tuple(float(x) for x in pivot), *args],
                       capture_output=True, text=True, timeout=120)
    return r, [str(tmp_path / ("%s_%04d.bmp" % (tag, k))) for k in range(3)]


def test_cli_rotate_host_and_device_sequence_write_the_same_frames(tmp_path, veach):
    pivot = centroid(veach, PLATE)
    host, fh = run_cli(tmp_path, "host", pivot)
    dev, fd = run_cli(tmp_path, "dev", pivot, "--device-sequence")
    assert host.returncode == 0 and dev.returncode == 0, (host.stderr, dev.stderr)
    for r in (host, dev):
        assert r.stdout.count("rotated facets [36, 48)") == 2, r.stdout
    frames = [(open(x, "rb").read(), open(y, "rb").read()) for x, y in zip(fh, fd)]
    for k, (x, y) in enumerate(frames):
        assert x == y, k
    assert frames[0][0] != frames[1][0] != frames[2][0]
