"""Device buffers own their memory (csrc/scene_state.h: DevBuf, ~DeviceState): mcpt_scene_destroy frees everything a
scene's device states hold, whichever entry points allocated it.  mcpt_debug_device_bytes_live counts the bytes held by
live buffers, so a scene that is loaded, used and destroyed leaves the counter where it was.

The failed-upload path of ensure_bvh8 and the device restore on error paths need a device error to be reached; they are
not provoked here (the guard trims the state's allocations, the restore is a destructor)."""
import gc
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, SCENE_OBJ, SCENE_XML
import monte_carlo_path_tracing_amd as mcpt

SEED = 20240430
FACET = 36  # a facet of the stand-in's second plate: no light triangle
SHIFT = np.array([[1, 0, 0, 0], [0, 1, 0, 0.01], [0, 0, 1, 0]], np.float64)

CPU_CYCLE = """
import sys
sys.path.insert(0, %r)
import numpy as np
import monte_carlo_path_tracing_amd as mcpt
assert mcpt.debug_device_bytes_live() == 0
s = mcpt.Scene.load(%r, %r)
pos = s.arrays()["positions"][%d:%d + 1]
s.update(%d, pos + np.float32(0.01))
s.rest_save()
s.transform(%d, 1, np.array(%r))
s.pose_save()
s.rebuild()
assert mcpt.debug_device_bytes_live() == 0
s.close()
print("live", mcpt.debug_device_bytes_live())
"""


def test_device_bytes_live_symbol_is_exported():
    hdr = (ROOT / "include" / "mcpt_debug.h").read_text()
    name = "mcpt_debug_device_bytes_live"
    assert re.search(r"\bint64_t\s+%s\s*\(\s*void\s*\)" % name, hdr)
    assert name in mcpt.DEBUG_EXPORTS and hasattr(mcpt.lib(), name) and hasattr(mcpt, "debug_device_bytes_live")


def test_no_device_state_no_bytes():
    """a process of its own: it never makes a device state, so a load / update / transform / destroy cycle on the
    stand-in runs the host halves alone and the counter stays 0"""
    src = CPU_CYCLE % (str(ROOT), str(SCENE_OBJ), str(SCENE_XML), FACET, FACET, FACET, FACET, SHIFT.tolist())
    out = subprocess.run([sys.executable, "-c", src], check=True, capture_output=True, text=True, cwd=str(ROOT)).stdout
    assert out.split()[-2:] == ["live", "0"], out


def used_scene():
    """the stand-in after the calls whose buffers the hand-kept free list missed or could miss: the root pick table, a
    host render_rays call, rest / pose copies, the staging arrays of a transform and a rebuild's tree sets"""
    s = mcpt.Scene.load(SCENE_OBJ, SCENE_XML)
    cam = s.camera()
    cam.width, cam.height = 33, 25
    mcpt.debug_set_pick_table(2, 0)
    try:
        _, st = mcpt.render(s, cam, 8, mode="mis", seed=SEED)
    finally:
        mcpt.debug_set_pick_table(0, 0)
    assert st.pick_table_roots > 0
    o, d = mcpt.camera_rays(cam)
    rad, _ = mcpt.render_rays(s, o[:64], d[:64], 1, mode="mis", seed=SEED)
    assert rad.shape == (64, 3) and np.isfinite(rad).all()
    s.rest_save()
    s.transform(FACET, 1, SHIFT)
    s.pose_save()
    s.rebuild()
    return s


@pytest.mark.gpu
def test_destroy_frees_every_buffer():
    gc.collect()  # scenes other tests dropped go now, not between the two readings
    b0 = mcpt.debug_device_bytes_live()
    for cycle in range(2):
        s = used_scene()
        held = mcpt.debug_device_bytes_live()
        print("cycle %d: %d bytes before, %d with the scene" % (cycle, b0, held))
        assert held > b0
        s.close()
        assert mcpt.debug_device_bytes_live() == b0


@pytest.mark.gpu
def test_destroy_frees_the_8_wide_trees():
    gc.collect()
    b0 = mcpt.debug_device_bytes_live()
    s = mcpt.Scene.load(SCENE_OBJ, SCENE_XML)
    cam = s.camera()
    cam.width, cam.height = 32, 24
    plain, _ = mcpt.render(s, cam, 8, mode="mis", seed=SEED)
    with_4 = mcpt.debug_device_bytes_live()
    img, _ = mcpt.render(s, cam, 8, mode="mis", seed=SEED, flags=mcpt.DEBUG_RAYS_PERSIST | mcpt.DEBUG_RAYS_CW8)
    assert np.isfinite(plain).all() and np.isfinite(img).all()
    assert mcpt.debug_device_bytes_live() > with_4 > b0  # the 8-wide trees were uploaded
    s.close()
    assert mcpt.debug_device_bytes_live() == b0
