"""k_prep_pk2's pick from stashed batch weights (DESIGN.md §4.3 "Pick").

The batch loop keeps the weights of a node's first m batches in the idle tail of the wave's candidate-list region
(LDS) and the pick reads a whole picked batch below m back instead of evaluating its 64 candidates again; a batch
beyond the stash, or a partial last batch, is evaluated again as before.  MCPT_DEBUG_REEVAL_PICK (prep variant 19)
forces the re-evaluation for every node.  Both forms must give the same weights_sum, pick and margin bit for bit:
  * points: the stand-in and the stress scenes, ~300 shading points each with 66 values of u (0, 1 - 2^-53 and
    (k + 0.5) / 64), so every batch of every point is picked by some u -- variant 17 against variant 19;
    the light panel (7 200 lights, up to 113 batches) and sphmix take the nb > 64 / N_L > 4096 forms, `dense`
    (14 160 lights) the LDS-queue prep that has no stash at all;
  * edge shapes: synthetic light strips that give a floor point exactly 0, 1, 63, 64, 65, 255, 256, 257 candidates,
    a strip with candidates the full stage culls, and one whose weights_sum stays below 1e-8;
  * frames: 64x48, 32 spp MIS with and without the flag -- identical bytes, identical exact-pick statistics (the
    margins feed the exact-pick lists, so a margin that moved shows here); rendered one sample per call, because a
    call of several samples per pixel is not reproducible to the byte even against itself, and once more as a single
    call, equal up to the order of the framebuffer's adds.
"""
import numpy as np
import pytest

import monte_carlo_path_tracing_amd as mcpt
from oracle import pyoracle as po
import scenegen
from conftest import SCENE_OBJ, SCENE_XML
from test_exact_pick_stress import surface_points

pytestmark = pytest.mark.gpu
SEED = 20240430
NPOINTS = 300
U66 = np.concatenate([[0.0, 1.0 - 2.0 ** -53], (np.arange(64) + 0.5) / 64.0])
gv = scenegen.gv


def with_u_grid(X, N):
    """every point with each of the 66 values of u"""
    return np.repeat(X, len(U66), axis=0), np.repeat(N, len(U66), axis=0), np.tile(U66, len(X))


def both_forms(scene, X, N, u):
    """variant 17 and the forced re-evaluation (19): (weights_sum, pick) of each and their served counts"""
    _, wa, pa = mcpt.debug_prep_bench(scene, X, N, u, variant=17, iters=1)
    ca = mcpt.debug_prep_pick_counts()
    _, wb, pb = mcpt.debug_prep_bench(scene, X, N, u, variant=19, iters=1)
    cb = mcpt.debug_prep_pick_counts()
    return (wa, pa, ca), (wb, pb, cb)


def assert_same(a, b, what):
    (wa, pa, ca), (wb, pb, cb) = a, b
    print("%s: %d nodes, %d with a pick; stash %d / re-evaluated %d; forced form %d / %d" % (
        what, len(wa), (pb >= 0).sum(), ca[0], ca[1], cb[0], cb[1]))
    assert np.array_equal(wa.view(np.uint64), wb.view(np.uint64)), np.nonzero(wa != wb)[0][:10]
    assert np.array_equal(pa, pb), np.nonzero(pa != pb)[0][:10]
    assert cb[0] == 0  # the forced form never reads the stash
    assert ca[0] + ca[1] == cb[1]  # the same nodes have a picked batch


@pytest.fixture(scope="module")
def scene_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("stash")
    out = {"veach": (SCENE_OBJ, SCENE_XML), "panel": scenegen.light_panel(str(d / "panel"))}
    for name in ("slivers", "tinyfar", "soup", "sphmix", "dense"):
        out[name] = scenegen.STRESS[name][0](str(d / name))
    return out


@pytest.mark.parametrize("name", ["veach", "slivers", "tinyfar", "soup", "sphmix", "panel", "dense"])
def test_pick_identity_points(scene_files, name):
    obj, xml = scene_files[name]
    s = mcpt.Scene.load(obj, xml)
    X, N, _ = surface_points(po.Scene(obj, xml), NPOINTS)
    a, b = both_forms(s, *with_u_grid(X, N))
    assert_same(a, b, name)
    assert (b[1] >= 0).sum() >= 66 * 20  # the points see lights
    if name == "veach":  # both ways of serving a pick occur, often
        assert a[2][0] >= 1000 and a[2][1] >= 1000, a[2]
    if name == "panel":  # more than 64 batches at some point: every light of the panel faces the floor
        ws, cnt, _ = mcpt.light_prep(s, X, N, np.full(len(X), 0.5))
        assert cnt.max() > 4096, cnt.max()
    if name == "dense":  # k_prep: no k_prep_pk2, nothing to count
        assert a[2] == (0, 0)


N_AWAY = 1400  # lights the cheap stages cull: 22+ chunks of list region, room for every strip's batches in the stash


def strip_scene(outdir, k_down, tiny=0, radiance=(2.0, 2.0, 2.0), size=0.02, y=2.5):
    """k_down light triangles facing the floor in a strip at height y (triangle legs `size`), `tiny` more of them
    400-2000 units up with 1e-6 legs (edges below 1e-8 rad: the full stage's edge-length cull) inserted after the
    tenth, and N_AWAY triangles facing away from the floor (the light-side stage culls them): the table has more
    than 64 lights whatever k_down is, and its list region (one 128-B slot per chunk) leaves the stash at least as
    many rows as a strip has batches ((nchunks - nb) / 4 >= nb for nb <= 5).  A floor point below the strip has
    exactly k_down + tiny candidates."""
    obj, mtls = gv.Obj(), []
    scenegen._floor(obj, mtls)
    nd, nu = obj.normal((0.0, -1.0, 0.0)), obj.normal((0.0, 1.0, 0.0))
    down = []
    for i in range(k_down):
        x, z = -0.5 + size * (i % 40), -0.2 + size * (i // 40)
        a, b, c = obj.vert((x, y, z)), obj.vert((x + size, y, z)), obj.vert((x + size, y, z + size))
        down.append(((a, nd), (b, nd), (c, nd)))  # (b - a) x (c - a) = -y
    for j in range(tiny):
        h, e = 400.0 * (j + 1), 1e-6
        a, b, c = obj.vert((0.1 * j, h, 0.0)), obj.vert((0.1 * j + e, h, 0.0)), obj.vert((0.1 * j + e, h, e))
        down.insert(min(10, len(down)), ((a, nd), (b, nd), (c, nd)))
    up = []
    for i in range(N_AWAY):
        x, z = -0.5 + 0.02 * (i % 50), 0.5 + 0.02 * (i // 50)
        a, b, c = obj.vert((x, 3.0, z)), obj.vert((x + 0.02, 3.0, z + 0.02)), obj.vert((x + 0.02, 3.0, z))
        up.append(((a, nu), (b, nu), (c, nu)))  # (b - a) x (c - a) = +y
    obj.groups.append(("strip", "strip", down + up))
    mtls.append(("strip", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0))
    return scenegen._write(outdir, "strip", obj, mtls, [("strip", radiance)], scenegen.CAM)


FLOOR_X = np.array([[0.0, 0.0, 0.0], [-0.3, 0.0, 0.4], [0.7, 0.0, -0.6], [1.5, 0.0, 1.5]])
FLOOR_N = np.tile([0.0, 1.0, 0.0], (len(FLOOR_X), 1))


def oracle_prep(obj, xml):
    osc = po.Scene(obj, xml)
    ws, cnt = np.zeros(len(FLOOR_X)), np.zeros(len(FLOOR_X), np.int32)
    for k in range(len(FLOOR_X)):
        w, idx, _ = osc.light_prep(FLOOR_X[k], FLOOR_N[k])
        ws[k], cnt[k] = w, len(idx)
    return ws, cnt


@pytest.mark.parametrize("ncand", [0, 1, 63, 64, 65, 255, 256, 257])
def test_edge_candidate_counts(tmp_path, ncand):
    obj, xml = strip_scene(str(tmp_path), ncand)
    s = mcpt.Scene.load(obj, xml)
    assert s.nlights == ncand + N_AWAY
    a, b = both_forms(s, *with_u_grid(FLOOR_X, FLOOR_N))
    assert_same(a, b, "strip of %d" % ncand)
    # the CPU reference: every strip triangle survives at every floor point, the others never do
    ows, ocnt = oracle_prep(obj, xml)
    ws, cnt, _ = mcpt.light_prep(s, FLOOR_X, FLOOR_N, np.full(len(FLOOR_X), 0.5))
    assert np.array_equal(ocnt, np.full(len(FLOOR_X), ncand)) and np.array_equal(cnt, ocnt)
    assert np.allclose(ws, ows, rtol=1e-3, atol=0)
    assert np.allclose(a[0], np.repeat(ows, len(U66)), rtol=1e-3, atol=0)  # the reference's own rounding noise
    picked = a[1].reshape(len(FLOOR_X), len(U66))
    if ncand == 0:
        assert (picked == -1).all() and a[2] == (0, 0)
    else:
        assert (picked >= 0).all()
        assert len(np.unique(picked[0])) >= min(ncand, 32)  # near-equal weights: u's grid spreads over the strip
        # whole batches come from the stash, a partial last batch is evaluated again
        assert (a[2][0] > 0) == (ncand >= 64) and (a[2][1] > 0) == (ncand % 64 != 0)


def test_edge_full_stage_cull_in_picked_batch(tmp_path):
    """five candidates of the first batch are culled by the full stage only (edges below 1e-8 rad)"""
    obj, xml = strip_scene(str(tmp_path), 123, tiny=5)
    s = mcpt.Scene.load(obj, xml)
    a, b = both_forms(s, *with_u_grid(FLOOR_X, FLOOR_N))
    assert_same(a, b, "strip of 123 + 5 tiny")
    _, ocnt = oracle_prep(obj, xml)
    _, cnt, _ = mcpt.light_prep(s, FLOOR_X, FLOOR_N, np.full(len(FLOOR_X), 0.5))
    print("survivors of 128 candidates:", cnt, "reference:", ocnt)
    assert np.array_equal(cnt, ocnt) and (cnt < 128).all() and (cnt >= 123).all()
    assert a[2][0] > 0  # two whole batches, the culled lanes in the first: read back with their cull marks
    assert (a[1] >= 0).all()


def test_edge_sum_below_eps(tmp_path):
    obj, xml = strip_scene(str(tmp_path), 100, radiance=(1e-6, 1e-6, 1e-6), size=0.005)
    s = mcpt.Scene.load(obj, xml)
    a, b = both_forms(s, *with_u_grid(FLOOR_X, FLOOR_N))
    assert_same(a, b, "dim strip")
    assert (a[0] > 0).all() and (a[0] < 1e-8).all() and (a[1] == -1).all()
    assert a[2] == (0, 0)  # no pick, nothing served


SPP = 32
COUNTS = ["shading_nodes", "prep_exact_nodes", "prep_band_nodes"]


def frame_by_samples(scene, cam, flags):
    """the 64x48, SPP-sample MIS frame rendered one camera sample per call (sample_range (k, k + 1) of SPP): the frame
    of every sample, their sum in sample order, and the summed statistics.  A pixel then receives at most one add per
    call, so a call's frame does not depend on the order of the framebuffer's fp64 atomic adds and is reproducible to
    the byte; a call of several samples per pixel is not (below)."""
    per, tot = [], {k: 0 for k in COUNTS}
    for k in range(SPP):
        img, st = mcpt.render(scene, cam, SPP, mode="mis", seed=SEED, sample_range=(k, k + 1), flags=flags)
        per.append(img)
        for c in COUNTS:
            tot[c] += getattr(st, c)
    frame = np.zeros_like(per[0])
    for img in per:
        frame += img
    return per, frame, tot


@pytest.mark.parametrize("name", ["veach", "soup"])
def test_frames_identical(scene_files, name):
    """64x48, 32 spp MIS with the stash and with the forced re-evaluation, same seed: framebuffers identical as bytes
    and equal exact-pick statistics (the margins feed the exact-pick lists, so a margin that moved shows here).

    The frame is rendered sample by sample (frame_by_samples).  One call of 32 samples per pixel cannot be compared
    as bytes with anything, itself included: its pixels are sums of up to 33 fp64 atomic adds whose order varies from
    run to run -- measured on MI355X, four renders of the SAME 64x48x32 call differ from one another in 4 068 - 4 209
    of the 9 216 doubles (relative L2 1.4e-16 - 1.7e-16), with the parent commit's library as with this one
    (profiles/prep_stash_ab.txt).  Every per-sample frame is compared as bytes, then their sum in sample order."""
    obj, xml = scene_files[name]
    s = mcpt.Scene.load(obj, xml)
    cam = s.camera()
    cam.width, cam.height = 64, 48
    pa, a, sa = frame_by_samples(s, cam, 0)
    pb, b, sb = frame_by_samples(s, cam, mcpt.DEBUG_REEVAL_PICK)
    pc, _, _ = frame_by_samples(s, cam, 0)
    same = [x.tobytes() == y.tobytes() for x, y in zip(pa, pb)]
    again = [x.tobytes() == y.tobytes() for x, y in zip(pa, pc)]
    print("%s 64x48x%d MIS by samples: %d of %d per-sample frames identical between the forms, %d of %d between two "
          "runs of one form; %s / %s" % (name, SPP, sum(same), SPP, sum(again), SPP, sa, sb))
    assert sa == sb and sa["shading_nodes"] > 0 and sa["prep_exact_nodes"] > 0
    assert all(again), "a one-sample call is not reproducible"
    assert all(same), np.nonzero(~np.array(same))[0]
    assert a.tobytes() == b.tobytes() and a.sum() > 0


@pytest.mark.parametrize("name", ["veach", "soup"])
def test_frames_single_call(scene_files, name):
    """The same frame as ONE call of 32 samples per pixel (the root-point cache and the root pick table engage only
    there): equal statistics, and every value equal up to the order of its adds.  A pixel component is a sum of at
    most 33 non-negative terms (32 root splats and a primary emitter hit), so two orders of the same terms differ by
    at most 2 (33 - 1) 2^-53 of the sum -- the standard bound of recursive summation; the test allows 64 * 2^-53."""
    obj, xml = scene_files[name]
    s = mcpt.Scene.load(obj, xml)
    cam = s.camera()
    cam.width, cam.height = 64, 48
    a, sa = mcpt.render(s, cam, SPP, mode="mis", seed=SEED)
    b, sb = mcpt.render(s, cam, SPP, mode="mis", seed=SEED, flags=mcpt.DEBUG_REEVAL_PICK)
    rel = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    print("%s 64x48x%d MIS, one call: largest relative difference of a value %.3e; exact preps %d / %d, band tests "
          "%d / %d" % (name, SPP, rel.max(), sa.prep_exact_nodes, sb.prep_exact_nodes, sa.prep_band_nodes, sb.prep_band_nodes))
    for c in COUNTS + ["prep_cached_nodes"]:
        assert getattr(sa, c) == getattr(sb, c), c
    assert sa.prep_cached_nodes > 0 and (a >= 0).all()
    assert rel.max() <= 64 * 2.0 ** -53
