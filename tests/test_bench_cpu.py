"""bench.py's CPU-side contract (no GPU): the CPU baseline's two legs (the oracle on ONE
core, the reference's loop main.cpp:557-588 being single-threaded per README.md:418, beside the host's
thread share at full spp), the launcher check of --gpus and --dump-outputs' file forms; and, on the GPU, what
a plain run does and dumps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_cpu_baseline_single_thread_leg():
    out, img, spp = bench.cpu_baseline("veach", 80, 60, "mis", 20240430, 8, 5.0, 0.5)
    assert out["cores"] == 1 and out["kind"] == "port" and out["value"] == out["single_thread_value"] > 0
    assert out["multi_thread_value"] > 0 and out["multi_thread_cores"] >= 1 and spp == out["multi_thread_spp"]
    assert 1 <= out["single_thread_spp"] <= 8 and out["subset_pixels"] == len(range(7, 60, 20)) * len(range(7, 80, 20))
    assert out["reference_equivalent_value"] == out["value"] / out["oracle_over_reference_cross_host"]
    assert img.shape == (60, 80, 3) and img[7::20, 7::20].sum() > 0


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: a frame within the size limit is written whole as float64; a larger one as the same
    seeded pixel sample every time, within the limit, with the pixels' indices beside it."""
    fb = np.random.default_rng(1).random((30, 40, 3))
    bench.dump_outputs(str(tmp_path / "a"), fb, 7)
    a = np.load(tmp_path / "a" / "framebuffer.npy")
    assert a.dtype == np.float64 and np.array_equal(a, fb) and os.listdir(tmp_path / "a") == ["framebuffer.npy"]
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 3200)  # 100 sampled pixels of the 1200
    for d in "bc":
        bench.dump_outputs(str(tmp_path / d), fb, 7)
    b, ib = np.load(tmp_path / "b" / "framebuffer.npy"), np.load(tmp_path / "b" / "framebuffer_pixels.npy")
    assert b.shape == (100, 3) and ib.shape == (100,) and b.nbytes + ib.nbytes <= 3200
    assert len(set(ib.tolist())) == 100 and np.array_equal(b, fb.reshape(-1, 3)[ib.astype(int)])
    assert np.array_equal(ib, np.load(tmp_path / "c" / "framebuffer_pixels.npy"))
    assert np.array_equal(b, np.load(tmp_path / "c" / "framebuffer.npy"))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_its_frame(tmp_path):
    """A plain `bench.py --gpus 1 --steps N --warmup W` runs no replay and no CPU baseline (those fields are
    null), times N steps, and with --dump-outputs writes the frame its N steps accumulated: the render of
    the same N x S samples in one call, up to the fp64 accumulation order (1e-12, as tests/test_gpu_parity.py
    bounds it)."""
    import monte_carlo_path_tracing_amd as mcpt
    from conftest import SCENE_OBJ, SCENE_XML
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--spp-per-step", "2", "--width", "80", "--height", "60", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{\"metric\"")][-1])
    assert line["steps"] == 3 and line["samples"] == 80 * 60 * 3 * 2 and line["value"] > 0
    elapsed = line["samples"] / line["value"] / 1e6  # seconds; the line rounds ms_per_step to 1 us, value to 1e-4
    assert abs(line["ms_per_step"] * 3 / 1e3 - elapsed) <= 5e-3 * elapsed
    assert line["cpu_baseline"] is None and line["l2_vs_cpu"] is None and line["roofline_trace"] is None
    assert "cpu baseline" not in r.stderr
    fb = np.load(d / "framebuffer.npy")
    assert fb.dtype == np.float64 and fb.shape == (60, 80, 3) and os.listdir(d) == ["framebuffer.npy"]
    ref, _ = mcpt.render(mcpt.Scene.load(SCENE_OBJ, SCENE_XML), mcpt.Camera.reference(80, 60), 6, mode="mis", seed=20240430)
    assert np.linalg.norm(fb - ref) / np.linalg.norm(ref) <= 1e-12


def test_bench_gpus_must_match_launcher():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "4", "--no-cpu"], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode != 0 and "--gpus 4" in r.stderr
