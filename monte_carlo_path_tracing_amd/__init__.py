"""MI355X-native Monte Carlo path tracer -- host-side mirror of the reference's render interface.

The reference (luotong96/Monte_Carlo_Path_Tracing) renders in `main()` (main.cpp:497-600):
load `Myobj veach` / `Mylight lights` (main.cpp:23-24, 500-504), set the camera (main.cpp:507-510),
trace one pixel-centre ray per pixel and average `spp` calls of `shade_with_mis` /
`shade_with_brdf` (main.cpp:557-588), tone-map (main.cpp:583) and save `test.bmp` (main.cpp:596).

Here the same steps are `Scene.load`, `Camera.reference`, `render(scene, camera, spp, mode)`,
`tone_map` and `write_bmp`, all backed by the C ABI of `libmcpt_hip.so` (include/mcpt.h), whose
hot path is hand-written HIP for gfx950.  There is no CPU fallback: every call fails loudly when
the native library (or, for rendering, a GPU) is missing.
"""
import ctypes as C
import os

import numpy as np

__all__ = ["Scene", "Camera", "Comm", "render", "render_device", "render_rays", "render_rays_device", "camera_rays", "RENDER_PIXEL_JITTER",
           "render_rays_indexed", "render_rays_indexed_device", "gradient_index", "gradient_rays_indexed",
           "render_adaptive", "render_adaptive_device", "closest_hit", "light_prep", "primary_hits",
           "AovBuffers", "DenoiseOpts", "render_aovs", "render_aovs_device", "denoise", "denoise_device", "variance_from_noise",
           "TemporalOpts", "TemporalAccumulator", "temporal_accumulate", "temporal_accumulate_device", "camera_orbit",
           "TemporalClampOpts", "temporal_accumulate_clamped", "temporal_accumulate_clamped_device",
           "SequenceOpts", "SequenceInfo", "FrameSequence", "tone_map_device", "frame_stats_device",
           "UpsampleOpts", "upsample", "upsample_device", "camera_scaled",
           "upsample_phase", "camera_phase_rays", "temporal_upsample", "temporal_upsample_device",
           "MotionBuffers", "render_motion_aovs", "render_motion_aovs_device", "temporal_accumulate_motion",
           "temporal_accumulate_motion_device", "transform_rotation", "RelightStats",
           "GradientOpts", "gradient_phase", "gradient_rays", "temporal_gradient", "temporal_accumulate_antilag",
           "temporal_accumulate_antilag_device", "SEQ_ANTILAG_BUFFERS",
           "tone_map", "write_bmp", "MODE_MIS", "MODE_BRDF", "MODE_SHADE", "MODE_SHADE_AREA", "ACCEL_BVH", "ACCEL_GRID", "Stats", "MCPTError", "LIB_PATH", "lib"]

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCPT_LIB_PATH") or os.path.join(HERE, "libmcpt_hip.so")  # override: A/B of two builds
MODE_MIS, MODE_BRDF, MODE_SHADE = 0, 1, 2  # shade_with_mis / shade_with_brdf / shade (main.cpp:402/348/269)
MODE_SHADE_AREA = 3  # shade with select_a_point_from_lights (Mylight.cpp:102-160; main.cpp:296)
MODES = {"mis": MODE_MIS, "brdf": MODE_BRDF, "shade": MODE_SHADE, "shade_area": MODE_SHADE_AREA}
ACCEL_BVH, ACCEL_GRID = 0, 1  # mcpt_render_opts.accel: BVH, or the reference's uniform grid (Myobj.cpp:78-162)
HIT_LIGHT_ONLY, HIT_GRID = 1, 2  # mcpt_closest_hit flags
DEFAULT_SEED = 20240430
MCPT_VERSION = 20300  # include/mcpt.h MCPT_VERSION this mirror is written against
COMM_ID_BYTES = 128  # MCPT_COMM_ID_BYTES
STATS_MAX_DEVICES = 16  # MCPT_STATS_MAX_DEVICES


class MCPTError(RuntimeError):
    pass


class Camera(C.Structure):
    """mcpt_camera: main.cpp:507-510,547-564 generalised to width x height."""
    _fields_ = [("eye", C.c_double * 3), ("lookat", C.c_double * 3), ("up", C.c_double * 3),
                ("fovy", C.c_double), ("dist_scale", C.c_double), ("width", C.c_int32), ("height", C.c_int32)]

    @classmethod
    def reference(cls, width=1280, height=720, dist_scale=2.0):
        """The hard-coded Veach camera of main.cpp:507-510 (eye pulled back 2x)."""
        c = cls()
        c.eye[:] = (28.2792, 5.2, 1.23612e-06)
        c.lookat[:] = (0.0, 2.8, 0.0)
        c.up[:] = (0.0, 1.0, 0.0)
        c.fovy = 20.1143
        c.dist_scale = dist_scale
        c.width, c.height = int(width), int(height)
        return c


class RenderOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("spp", C.c_int32), ("sample_begin", C.c_int32),
                ("sample_end", C.c_int32), ("mode", C.c_int32),
                ("seed", C.c_uint64), ("samples_per_launch", C.c_int32), ("queue_factor", C.c_int32),
                ("device", C.c_int32), ("accel", C.c_int32), ("progress", C.c_void_p),
                ("progress_user", C.c_void_p), ("flags", C.c_int32), ("num_devices", C.c_int32),
                ("devices", C.POINTER(C.c_int32)), ("comm", C.c_void_p), ("stats_size", C.c_uint32)]
RENDER_NO_BACKFACE_STATS = 1  # mcpt_render_opts.flags (include/mcpt.h)
RENDER_FRESH_PDF = 2  # shade_with_mis: the node's own light pdf instead of the reference's stale one
RENDER_PRECISION_FP32 = 4  # opt-in FP32_STABLE light prep (packed-fp32 weights, fp64 sums); default FP64_LIGHT
RENDER_PIXEL_JITTER = 8  # opt-in anti-aliasing: every sample's camera ray through its own sub-pixel offset (box filter)
DEBUG_SPLIT_BRDF, DEBUG_NO_ROOT_CACHE, DEBUG_COUNT_TRAVERSAL = 1 << 16, 1 << 17, 1 << 18  # include/mcpt_debug.h
DEBUG_SHARD_RANKS = 1 << 19  # device lists: every entry its own communicator rank (tests/collshim)
DEBUG_RAYS_PERSIST = 1 << 20  # MIS / shade ray sets through the persistent refilling traversal on every scene
DEBUG_RAYS_CW8 = 1 << 21  # the persistent traversal walks the 8-wide compressed trees (k_rays_cw8)
DEBUG_FUSED_CULL = 1 << 22  # MIS children's prep: cheap stages inside k_prep_pk2 (variant 8) instead of k_prep_cull_lanes
DEBUG_NO_EXACT_DEFER = 1 << 23  # k_prep_exact recomputes same-launch duplicate roots instead of deferring them
DEBUG_NO_PICK_TABLE = 1 << 24  # cached roots search their pixel's cached row (k_prep_pick_g) instead of the root pick table
DEBUG_REEVAL_PICK = 1 << 25  # k_prep_pk2 stashes no batch weights: every pick evaluates its picked batch again
DEBUG_HIT_CW8 = 1 << 8  # mcpt_closest_hit: trace through the 8-wide trees


class AdaptiveOpts(C.Structure):
    """mcpt_adaptive_opts: the adaptive stopping rule's parameters (include/mcpt.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("min_spp", C.c_int32), ("pass_spp", C.c_int32), ("max_spp", C.c_int32),
                ("threshold", C.c_double), ("radius", C.c_int32)]


class AovBuffers(C.Structure):
    """mcpt_aov_buffers: the four primary-hit maps (include/mcpt.h); any pointer may be NULL where allowed."""
    _fields_ = [("albedo", C.c_void_p), ("normal", C.c_void_p), ("position", C.c_void_p), ("depth", C.c_void_p)]


class MotionBuffers(C.Structure):
    """mcpt_motion_buffers: the two motion AOVs (include/mcpt.h)."""
    _fields_ = [("prev_position", C.c_void_p), ("prev_normal", C.c_void_p)]


class DenoiseOpts(C.Structure):
    """mcpt_denoise_opts: the a-trous filter's parameters (include/mcpt.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32), ("sigma_color", C.c_double),
                ("sigma_normal", C.c_double), ("sigma_plane", C.c_double), ("sigma_albedo", C.c_double),
                ("device", C.c_int32)]


class TemporalOpts(C.Structure):
    """mcpt_temporal_opts: the temporal accumulation's parameters (include/mcpt.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("max_history", C.c_int32), ("variance_min_history", C.c_int32),
                ("device", C.c_int32), ("alpha", C.c_double), ("normal_min", C.c_double), ("plane_max", C.c_double),
                ("min_weight", C.c_double), ("sigma_normal", C.c_double), ("sigma_plane", C.c_double),
                ("sigma_albedo", C.c_double)]


class TemporalClampOpts(C.Structure):
    """mcpt_temporal_clamp_opts: the history clamp's parameters (include/mcpt.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("radius", C.c_int32), ("alpha_fast", C.c_double), ("sigma", C.c_double)]


class GradientOpts(C.Structure):
    """mcpt_gradient_opts: the temporal gradient's parameters (include/mcpt.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("stratum", C.c_int32), ("radius", C.c_int32), ("device", C.c_int32),
                ("scale", C.c_double)]


class UpsampleOpts(C.Structure):
    """mcpt_upsample_opts: the guided upsampling's parameters (include/mcpt.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("factor", C.c_int32), ("sigma_normal", C.c_double),
                ("sigma_plane", C.c_double), ("sigma_albedo", C.c_double), ("min_weight", C.c_double),
                ("device", C.c_int32)]


class SequenceOpts(C.Structure):
    """mcpt_sequence_opts: what a device-resident frame sequence is created with (include/mcpt.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("spp", C.c_int32),
                ("denoise", C.c_int32), ("clamp", C.c_int32), ("tone_max", C.c_double), ("tone_gamma", C.c_double),
                ("info_size", C.c_uint32)]


class SequenceInfo(C.Structure):
    """mcpt_sequence_info: the stage device times and the history statistics of one frame (include/mcpt.h)."""
    _fields_ = [("render_seconds", C.c_double), ("aov_seconds", C.c_double), ("temporal_seconds", C.c_double),
                ("denoise_seconds", C.c_double), ("tonemap_seconds", C.c_double), ("kept", C.c_double),
                ("mean_history", C.c_double), ("clamped", C.c_double), ("frame_index", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# mcpt_sequence_read / _device_buffer selectors: name -> (MCPT_SEQ_*, trailing shape)
SEQ_BUFFERS = {"raw": (0, (3,)), "accumulated": (1, (3,)), "moments": (2, (4,)), "variance": (3, ()), "filtered": (4, (3,)),
               "fast": (5, (3,)), "shift": (6, ()), "rgb8": (7, (3,)), "upsampled": (8, (3,))}
# and of a sequence with motion: MCPT_SEQ_PREV_POSITION, MCPT_SEQ_PREV_NORMAL
SEQ_MOTION_BUFFERS = {"prev_position": (9, (3,)), "prev_normal": (10, (3,))}
# and of a sequence with anti-lag: MCPT_SEQ_GRADIENT_LAMBDA (hs x ws at the stratum), MCPT_SEQ_GRADIENT_RAW
SEQ_ANTILAG_BUFFERS = {"gradient_lambda": (11, ()), "gradient_raw": (12, (3,))}


PROGRESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64)


class Stats(C.Structure):
    _fields_ = [("seconds", C.c_double), ("camera_samples", C.c_uint64), ("shading_nodes", C.c_uint64),
                ("light_evals_survived", C.c_uint64), ("rays", C.c_uint64), ("light_rays", C.c_uint64),
                ("generations", C.c_uint64), ("prep_seconds", C.c_double), ("prep_launches", C.c_uint64),
                ("light_evals_total", C.c_uint64), ("light_evals_culled_backface", C.c_uint64),
                ("light_evals_culled_plane", C.c_uint64), ("light_evals_candidates", C.c_uint64),
                ("prep_full_nodes", C.c_uint64), ("prep_cached_nodes", C.c_uint64), ("prep_cache_points", C.c_uint64),
                ("spilled_nodes", C.c_uint64), ("reduce_seconds", C.c_double), ("devices_used", C.c_int32),
                ("trace_seconds", C.c_double), ("trace_launches", C.c_uint64), ("node_visits", C.c_uint64),
                ("tri_tests", C.c_uint64), ("prep_exact_nodes", C.c_uint64), ("cache_build_seconds", C.c_double),
                ("prep_band_nodes", C.c_uint64), ("comm_init_seconds", C.c_double),
                ("device_setup_seconds", C.c_double), ("device_seconds", C.c_double * STATS_MAX_DEVICES),
                ("pick_table_roots", C.c_uint64)]

    def as_dict(self):
        """scalar fields (summable); device_seconds is in per_device_seconds()"""
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "device_seconds"}

    def per_device_seconds(self):
        """device_seconds[:devices_used]: each rank's shard wall time (setup and reduce excluded)"""
        return [float(v) for v in self.device_seconds[:max(1, min(self.devices_used, STATS_MAX_DEVICES))]]


_lib = None

# every symbol include/mcpt.h declares (tests check the .so exports them all)
class SceneDesc(C.Structure):
    """mcpt_scene_desc (include/mcpt.h)"""
    _fields_ = [("nfacets", C.c_int32), ("nmaterials", C.c_int32), ("nlights", C.c_int32), ("positions", C.c_void_p),
                ("normals", C.c_void_p), ("material_id", C.c_void_p), ("materials", C.c_void_p), ("light_facet", C.c_void_p),
                ("light_radiance", C.c_void_p), ("light_group", C.c_void_p)]


class UpdateStats(C.Structure):
    """mcpt_update_stats (include/mcpt.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("facets", C.c_int32), ("leaf_slots", C.c_int64), ("nodes_refit", C.c_int64),
                ("levels", C.c_int32), ("device_states", C.c_int32), ("device_seconds", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class RebuildStats(C.Structure):
    """mcpt_rebuild_stats (include/mcpt.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("facets", C.c_int32), ("nodes", C.c_int32), ("levels", C.c_int32),
                ("stack_need", C.c_int32), ("device_states", C.c_int32), ("cost_before", C.c_double),
                ("cost_after", C.c_double), ("device_seconds", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class LightUpdateStats(C.Structure):
    """mcpt_light_update_stats (include/mcpt.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("lights", C.c_int32), ("chunks", C.c_int32), ("groups", C.c_int32),
                ("light_nodes_refit", C.c_int64), ("light_levels", C.c_int32), ("device_seconds", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


class RelightStats(C.Structure):
    """mcpt_relight_stats (include/mcpt.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("lights", C.c_int32), ("chunks", C.c_int32), ("groups", C.c_int32),
                ("materials", C.c_int32), ("device_states", C.c_int32), ("device_seconds", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "struct_size"}


# mcpt_debug_bvh4_download's node layouts (BvhNode4 / BvhNode4Q of the library; leaf children as ~first slot, count)
BVH4_NODE = np.dtype([("lo", np.float32, (3, 4)), ("hi", np.float32, (3, 4)), ("child", np.int32, 4), ("count", np.int32, 4)])
BVH4_QNODE = np.dtype([("org", np.float32, 3), ("ex", np.uint32), ("q", np.uint32, 6), ("pad", np.uint32, 2), ("child", np.int32, 4)])
BVH4_EMPTY = 0x7fffffff

EXPORTS = ["mcpt_version", "mcpt_last_error", "mcpt_scene_load", "mcpt_scene_create", "mcpt_scene_destroy",
           "mcpt_scene_counts", "mcpt_scene_accel_bytes", "mcpt_scene_arrays", "mcpt_scene_camera", "mcpt_scene_meshing", "mcpt_scene_grid_info",
           "mcpt_render_opts_init", "mcpt_render", "mcpt_render_device",
           "mcpt_render_rays", "mcpt_render_rays_device", "mcpt_camera_rays",
           "mcpt_render_rays_indexed", "mcpt_render_rays_indexed_device", "mcpt_gradient_index", "mcpt_gradient_rays_indexed",
           "mcpt_gradient_rays_indexed_device",
           "mcpt_adaptive_opts_init", "mcpt_render_adaptive", "mcpt_render_adaptive_device",
           "mcpt_render_aovs", "mcpt_render_aovs_device", "mcpt_denoise_opts_init", "mcpt_denoise", "mcpt_denoise_device",
           "mcpt_variance_from_noise", "mcpt_temporal_opts_init", "mcpt_temporal_accumulate",
           "mcpt_temporal_accumulate_device", "mcpt_temporal_clamp_opts_init", "mcpt_temporal_accumulate_clamped",
           "mcpt_temporal_accumulate_clamped_device", "mcpt_camera_orbit", "mcpt_closest_hit", "mcpt_light_prep", "mcpt_primary_hits", "mcpt_tone_map",
           "mcpt_write_bmp", "mcpt_comm_unique_id", "mcpt_comm_init_rank", "mcpt_comm_destroy",
           "mcpt_tone_map_device", "mcpt_frame_stats_device", "mcpt_sequence_opts_init", "mcpt_sequence_create",
           "mcpt_sequence_frame", "mcpt_sequence_read", "mcpt_sequence_device_buffer", "mcpt_sequence_reset",
           "mcpt_sequence_destroy", "mcpt_upsample_opts_init", "mcpt_upsample", "mcpt_upsample_device",
           "mcpt_camera_scaled", "mcpt_sequence_create_upsampled", "mcpt_sequence_upsample_info",
           "mcpt_upsample_phase", "mcpt_camera_phase_rays", "mcpt_camera_phase_rays_device", "mcpt_temporal_upsample",
           "mcpt_temporal_upsample_device", "mcpt_sequence_create_temporal_upsampled", "mcpt_sequence_temporal_upsample_info",
           "mcpt_update_stats_init", "mcpt_scene_update", "mcpt_scene_update_device",
           "mcpt_scene_pose_save", "mcpt_render_motion_aovs", "mcpt_render_motion_aovs_device",
           "mcpt_temporal_accumulate_motion", "mcpt_temporal_accumulate_motion_device", "mcpt_sequence_set_motion",
           "mcpt_sequence_motion_info",
           "mcpt_scene_rest_save", "mcpt_scene_transform", "mcpt_scene_host_pending", "mcpt_scene_host_sync",
           "mcpt_transform_rotation",
           "mcpt_rebuild_stats_init", "mcpt_scene_rebuild", "mcpt_scene_tree_cost",
           "mcpt_scene_set_lights_movable", "mcpt_scene_lights_movable", "mcpt_light_update_stats_init",
           "mcpt_scene_light_update_info",
           "mcpt_relight_stats_init", "mcpt_scene_set_light_radiance", "mcpt_scene_set_light_radiance_device",
           "mcpt_scene_set_materials", "mcpt_scene_light_groups",
           "mcpt_scene_set_visible", "mcpt_scene_visibility",
           "mcpt_gradient_opts_init", "mcpt_gradient_phase", "mcpt_gradient_rays", "mcpt_gradient_rays_device",
           "mcpt_temporal_gradient", "mcpt_temporal_gradient_device", "mcpt_temporal_accumulate_antilag",
           "mcpt_temporal_accumulate_antilag_device", "mcpt_sequence_set_antilag", "mcpt_sequence_antilag_info"]
DEBUG_EXPORTS = ["mcpt_debug_bvh4_check_device_light", "mcpt_debug_light_tables", "mcpt_debug_light_area_cum_bench","mcpt_debug_prep_bench", "mcpt_debug_tri_filter", "mcpt_debug_light_prep_exact", "mcpt_debug_light_literal",
                 "mcpt_debug_set_collective_lib", "mcpt_debug_bvh8_check", "mcpt_debug_bvh4_check",
                 "mcpt_debug_adaptive_active", "mcpt_debug_bvh4_check_device", "mcpt_debug_bvh4_download",
                 "mcpt_debug_set_pick_table", "mcpt_debug_root_picks", "mcpt_debug_set_rebuild_leaf_max",
                 "mcpt_debug_phong", "mcpt_debug_device_bytes_live", "mcpt_debug_prep_pick_counts",
                 "mcpt_debug_bvh4_host"]  # include/mcpt_debug.h


def lib():
    """The native library; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MCPTError("libmcpt_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "or `make -C monte_carlo_path_tracing_amd/csrc`")
        # One HIP runtime per process: torch wheels bundle their own libamdhip64.so.7 /
        # libhsa-runtime64.so.1 (same sonames as /opt/rocm's).  Loading torch first makes this
        # library bind to torch's runtime, so device pointers and streams are shared; loading
        # /opt/rocm's runtime first would leave torch without a usable GPU.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        P, I, D = C.c_void_p, C.c_int32, C.c_double
        dp = np.ctypeslib.ndpointer(np.float64, flags="C")
        fp = np.ctypeslib.ndpointer(np.float32, flags="C")
        ip = np.ctypeslib.ndpointer(np.int32, flags="C")
        u8 = np.ctypeslib.ndpointer(np.uint8, flags="C")
        L.mcpt_version.restype = C.c_int
        L.mcpt_last_error.restype = C.c_char_p
        L.mcpt_scene_load.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(P)]
        L.mcpt_scene_create.argtypes = [P, C.POINTER(P)]
        L.mcpt_scene_destroy.argtypes = [P]
        L.mcpt_scene_destroy.restype = None
        L.mcpt_scene_counts.argtypes = [P, C.POINTER(I), C.POINTER(I), C.POINTER(I)]
        L.mcpt_scene_accel_bytes.argtypes = [P, C.POINTER(C.c_uint64)]
        L.mcpt_scene_arrays.argtypes = [P, fp, fp, ip, fp, ip, dp, dp]
        L.mcpt_scene_camera.argtypes = [P, C.POINTER(Camera)]
        L.mcpt_scene_meshing.argtypes = [P, dp, I]
        L.mcpt_scene_grid_info.argtypes = [P, dp, ip]
        L.mcpt_render_opts_init.argtypes = [C.POINTER(RenderOpts)]
        L.mcpt_render_opts_init.restype = None
        L.mcpt_render.argtypes = [P, C.POINTER(Camera), C.POINTER(RenderOpts), dp, C.POINTER(Stats)]
        L.mcpt_render_device.argtypes = [P, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_void_p, C.POINTER(Stats)]
        if hasattr(L, "mcpt_render_adaptive"):  # ABI 2.3 (an older build timed through MCPT_LIB_PATH lacks it)
            L.mcpt_adaptive_opts_init.argtypes = [C.POINTER(AdaptiveOpts)]
            L.mcpt_adaptive_opts_init.restype = None
            L.mcpt_render_adaptive.argtypes = [P, C.POINTER(Camera), C.POINTER(RenderOpts), C.POINTER(AdaptiveOpts), dp,
                                               C.c_void_p, C.c_void_p, C.POINTER(Stats)]
            L.mcpt_render_adaptive_device.argtypes = [P, C.POINTER(Camera), C.POINTER(RenderOpts),
                                                      C.POINTER(AdaptiveOpts), C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.POINTER(Stats)]
        if hasattr(L, "mcpt_denoise"):  # added under ABI 2.3 (an older build timed through MCPT_LIB_PATH lacks them)
            L.mcpt_render_aovs.argtypes = [P, C.POINTER(Camera), C.POINTER(RenderOpts), C.POINTER(AovBuffers)]
            L.mcpt_render_aovs_device.argtypes = L.mcpt_render_aovs.argtypes
            L.mcpt_denoise_opts_init.argtypes = [C.POINTER(DenoiseOpts)]
            L.mcpt_denoise_opts_init.restype = None
            L.mcpt_denoise.argtypes = [C.POINTER(DenoiseOpts), I, I, P, P, C.POINTER(AovBuffers), P, P, C.POINTER(D)]
            L.mcpt_denoise_device.argtypes = L.mcpt_denoise.argtypes
            L.mcpt_variance_from_noise.argtypes = [I, I, dp, dp, dp]
        if hasattr(L, "mcpt_temporal_accumulate"):  # added under ABI 2.3 as well
            L.mcpt_temporal_opts_init.argtypes = [C.POINTER(TemporalOpts)]
            L.mcpt_temporal_opts_init.restype = None
            L.mcpt_temporal_accumulate.argtypes = [C.POINTER(TemporalOpts), C.POINTER(Camera), I, I, P, C.POINTER(AovBuffers),
                                                   C.POINTER(AovBuffers), P, P, P, P, P, C.POINTER(D)]
            L.mcpt_temporal_accumulate_device.argtypes = L.mcpt_temporal_accumulate.argtypes
            L.mcpt_camera_orbit.argtypes = [C.POINTER(Camera), D, C.POINTER(Camera)]
        if hasattr(L, "mcpt_temporal_accumulate_clamped"):  # and so is the history clamp
            L.mcpt_temporal_clamp_opts_init.argtypes = [C.POINTER(TemporalClampOpts)]
            L.mcpt_temporal_clamp_opts_init.restype = None
            L.mcpt_temporal_accumulate_clamped.argtypes = [C.POINTER(TemporalOpts), C.POINTER(TemporalClampOpts), C.POINTER(Camera),
                                                           I, I, P, C.POINTER(AovBuffers), C.POINTER(AovBuffers), P, P, P, P, P,
                                                           P, P, P, C.POINTER(D)]
            L.mcpt_temporal_accumulate_clamped_device.argtypes = L.mcpt_temporal_accumulate_clamped.argtypes
        if hasattr(L, "mcpt_sequence_create"):  # and the device-resident frame sequence
            L.mcpt_tone_map_device.argtypes = [P, I, I, D, D, P, I]
            L.mcpt_frame_stats_device.argtypes = [P, P, I, I, I, C.POINTER(C.c_uint64), C.POINTER(D), C.POINTER(C.c_uint64)]
            L.mcpt_sequence_opts_init.argtypes = [C.POINTER(SequenceOpts)]
            L.mcpt_sequence_opts_init.restype = None
            L.mcpt_sequence_create.argtypes = [P, C.POINTER(RenderOpts), C.POINTER(SequenceOpts), C.POINTER(TemporalOpts),
                                               C.POINTER(TemporalClampOpts), C.POINTER(DenoiseOpts), C.POINTER(P)]
            L.mcpt_sequence_frame.argtypes = [P, C.POINTER(Camera), C.c_uint64, P, C.POINTER(SequenceInfo), C.POINTER(Stats)]
            L.mcpt_sequence_read.argtypes = [P, I, P]
            L.mcpt_sequence_device_buffer.argtypes = [P, I, C.POINTER(P)]
            L.mcpt_sequence_reset.argtypes = [P]
            L.mcpt_sequence_destroy.argtypes = [P]
            L.mcpt_sequence_destroy.restype = None
        if hasattr(L, "mcpt_upsample"):  # and the guided upsampling
            L.mcpt_upsample_opts_init.argtypes = [C.POINTER(UpsampleOpts)]
            L.mcpt_upsample_opts_init.restype = None
            L.mcpt_upsample.argtypes = [C.POINTER(UpsampleOpts), I, I, P, C.POINTER(AovBuffers), C.POINTER(AovBuffers), P,
                                        C.POINTER(C.c_uint64), C.POINTER(D)]
            L.mcpt_upsample_device.argtypes = L.mcpt_upsample.argtypes
            L.mcpt_camera_scaled.argtypes = [C.POINTER(Camera), I, C.POINTER(Camera)]
            L.mcpt_sequence_create_upsampled.argtypes = [P, C.POINTER(RenderOpts), C.POINTER(SequenceOpts), C.POINTER(TemporalOpts),
                                                         C.POINTER(TemporalClampOpts), C.POINTER(DenoiseOpts),
                                                         C.POINTER(UpsampleOpts), C.POINTER(P)]
            L.mcpt_sequence_upsample_info.argtypes = [P, C.POINTER(D), C.POINTER(D), C.POINTER(D)]
        if hasattr(L, "mcpt_temporal_upsample"):  # and the temporal upsampling
            L.mcpt_upsample_phase.argtypes = [I, C.c_uint64, C.POINTER(I), C.POINTER(I)]
            L.mcpt_camera_phase_rays.argtypes = [C.POINTER(Camera), I, I, I, I, P, P]
            L.mcpt_camera_phase_rays_device.argtypes = L.mcpt_camera_phase_rays.argtypes
            L.mcpt_temporal_upsample.argtypes = [C.POINTER(TemporalOpts), C.POINTER(UpsampleOpts), I, I, C.POINTER(Camera), I, I, P,
                                                 C.POINTER(AovBuffers), C.POINTER(AovBuffers), P, P, P, P, P,
                                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(D)]
            L.mcpt_temporal_upsample_device.argtypes = L.mcpt_temporal_upsample.argtypes
            L.mcpt_sequence_create_temporal_upsampled.argtypes = [P, C.POINTER(RenderOpts), C.POINTER(SequenceOpts),
                                                                  C.POINTER(TemporalOpts), C.POINTER(DenoiseOpts),
                                                                  C.POINTER(UpsampleOpts), C.POINTER(P)]
            L.mcpt_sequence_temporal_upsample_info.argtypes = [P, C.POINTER(I), C.POINTER(I), C.POINTER(D), C.POINTER(D),
                                                               C.POINTER(D)]
        if hasattr(L, "mcpt_render_rays"):  # and the radiance along caller-supplied rays
            L.mcpt_render_rays.argtypes = [P, C.POINTER(RenderOpts), I, P, P, P, C.POINTER(Stats)]
            L.mcpt_render_rays_device.argtypes = L.mcpt_render_rays.argtypes
            L.mcpt_camera_rays.argtypes = [C.POINTER(Camera), C.c_uint64, I, I, I, P, P]
        if hasattr(L, "mcpt_render_rays_indexed"):  # and along rays that carry their pixel ids
            L.mcpt_render_rays_indexed.argtypes = [P, C.POINTER(RenderOpts), I, P, P, P, I, P, C.POINTER(Stats)]
            L.mcpt_render_rays_indexed_device.argtypes = L.mcpt_render_rays_indexed.argtypes
            L.mcpt_gradient_index.argtypes = [I, I, I, I, I, C.POINTER(I), P]
            L.mcpt_gradient_rays_indexed.argtypes = [C.POINTER(Camera), I, I, I, I, P, P, P]
            L.mcpt_gradient_rays_indexed_device.argtypes = L.mcpt_gradient_rays_indexed.argtypes
        if hasattr(L, "mcpt_scene_update"):  # and the in-place geometry updates
            L.mcpt_update_stats_init.argtypes = [C.POINTER(UpdateStats)]
            L.mcpt_update_stats_init.restype = None
            L.mcpt_scene_update.argtypes = [P, I, I, P, P, C.POINTER(UpdateStats)]
            L.mcpt_scene_update_device.argtypes = [P, I, I, I, P, P, C.POINTER(UpdateStats)]
        if hasattr(L, "mcpt_scene_pose_save"):  # and the object motion of the temporal accumulation
            L.mcpt_scene_pose_save.argtypes = [P]
            L.mcpt_render_motion_aovs.argtypes = [P, C.POINTER(Camera), C.POINTER(RenderOpts), C.POINTER(MotionBuffers)]
            L.mcpt_render_motion_aovs_device.argtypes = L.mcpt_render_motion_aovs.argtypes
            L.mcpt_temporal_accumulate_motion.argtypes = [C.POINTER(TemporalOpts), C.POINTER(TemporalClampOpts), C.POINTER(Camera), I, I,
                                                          P, C.POINTER(AovBuffers), C.POINTER(MotionBuffers), C.POINTER(AovBuffers),
                                                          P, P, P, P, P, P, P, P, C.POINTER(D)]
            L.mcpt_temporal_accumulate_motion_device.argtypes = L.mcpt_temporal_accumulate_motion.argtypes
            L.mcpt_sequence_set_motion.argtypes = [P, I]
            L.mcpt_sequence_motion_info.argtypes = [P, C.POINTER(D)]
        if hasattr(L, "mcpt_scene_transform"):  # and the on-device transforms with the lazily synced host copy
            L.mcpt_scene_rest_save.argtypes = [P]
            L.mcpt_scene_transform.argtypes = [P, I, I, P, P, C.POINTER(UpdateStats)]
            L.mcpt_scene_host_pending.argtypes = [P, C.POINTER(C.c_int64)]
            L.mcpt_scene_host_sync.argtypes = [P]
            L.mcpt_transform_rotation.argtypes = [P, D, P, P, P]
        if hasattr(L, "mcpt_scene_rebuild"):  # and the on-device rebuild of the main tree
            L.mcpt_rebuild_stats_init.argtypes = [C.POINTER(RebuildStats)]
            L.mcpt_rebuild_stats_init.restype = None
            L.mcpt_scene_rebuild.argtypes = [P, C.POINTER(RebuildStats)]
            L.mcpt_scene_tree_cost.argtypes = [P, I, C.POINTER(D)]
        if hasattr(L, "mcpt_scene_set_lights_movable"):  # and the movable light triangles
            L.mcpt_scene_set_lights_movable.argtypes = [P, I]
            L.mcpt_scene_lights_movable.argtypes = [P, C.POINTER(I)]
            L.mcpt_light_update_stats_init.argtypes = [C.POINTER(LightUpdateStats)]
            L.mcpt_light_update_stats_init.restype = None
            L.mcpt_scene_light_update_info.argtypes = [P, C.POINTER(LightUpdateStats)]
        if hasattr(L, "mcpt_scene_set_light_radiance"):  # and the in-place re-lighting
            L.mcpt_relight_stats_init.argtypes = [C.POINTER(RelightStats)]
            L.mcpt_relight_stats_init.restype = None
            L.mcpt_scene_set_light_radiance.argtypes = [P, I, I, P, C.POINTER(RelightStats)]
            L.mcpt_scene_set_light_radiance_device.argtypes = [P, I, I, I, P, C.POINTER(RelightStats)]
            L.mcpt_scene_set_materials.argtypes = [P, I, I, P, C.POINTER(RelightStats)]
            L.mcpt_scene_light_groups.argtypes = [P, ip]
        if hasattr(L, "mcpt_scene_set_visible"):  # and the facet visibility
            L.mcpt_scene_set_visible.argtypes = [P, I, I, I, C.POINTER(UpdateStats)]
            L.mcpt_scene_visibility.argtypes = [P, P, C.POINTER(C.c_int32)]
        if hasattr(L, "mcpt_temporal_gradient"):  # and the anti-lag by temporal gradients
            L.mcpt_gradient_opts_init.argtypes = [C.POINTER(GradientOpts)]
            L.mcpt_gradient_opts_init.restype = None
            L.mcpt_gradient_phase.argtypes = [I, C.c_uint64, C.POINTER(I), C.POINTER(I)]
            L.mcpt_gradient_rays.argtypes = [C.POINTER(Camera), I, I, I, I, P, P]
            L.mcpt_gradient_rays_device.argtypes = L.mcpt_gradient_rays.argtypes
            L.mcpt_temporal_gradient.argtypes = [C.POINTER(GradientOpts), I, I, I, I, P, P, P, C.POINTER(D)]
            L.mcpt_temporal_gradient_device.argtypes = L.mcpt_temporal_gradient.argtypes
            L.mcpt_temporal_accumulate_antilag.argtypes = L.mcpt_temporal_accumulate_motion.argtypes + [C.POINTER(GradientOpts), P]
            L.mcpt_temporal_accumulate_antilag_device.argtypes = L.mcpt_temporal_accumulate_antilag.argtypes
            L.mcpt_sequence_set_antilag.argtypes = [P, C.POINTER(GradientOpts)]
            L.mcpt_sequence_antilag_info.argtypes = [P, C.POINTER(I), C.POINTER(I), C.POINTER(I), C.POINTER(D), C.POINTER(D),
                                                     C.POINTER(D), C.POINTER(D)]
        L.mcpt_closest_hit.argtypes = [P, I, dp, dp, ip, I, ip, dp]
        L.mcpt_light_prep.argtypes = [P, I, dp, dp, dp, dp, ip, ip]
        L.mcpt_primary_hits.argtypes = [P, C.POINTER(Camera), ip, dp]
        # debug entry points (include/mcpt_debug.h): bound when present, so an older build can still
        # be timed against this one through MCPT_LIB_PATH (tools/ab_run.sh)
        dbg = {"mcpt_debug_prep_bench": [P, I, dp, dp, dp, I, I, C.POINTER(C.c_double), dp, ip],
               "mcpt_debug_tri_filter": [I, fp, dp, dp, fp, ip, fp],
               "mcpt_debug_light_prep_exact": [P, I, dp, dp, dp, dp, ip, ip],
               "mcpt_debug_light_literal": [P, dp, dp, dp],
               "mcpt_debug_set_collective_lib": [C.c_char_p],
               "mcpt_debug_bvh8_check": [P, I, np.ctypeslib.ndpointer(np.int64, flags="C")],
               "mcpt_debug_bvh4_check": [P, I, np.ctypeslib.ndpointer(np.int64, flags="C")],
               "mcpt_debug_adaptive_active": [P, I, ip, I, C.POINTER(I)],
               "mcpt_debug_bvh4_check_device": [P, I, np.ctypeslib.ndpointer(np.int64, flags="C")],
               "mcpt_debug_set_pick_table": [I, I],
               "mcpt_debug_set_rebuild_leaf_max": [I],
               "mcpt_debug_root_picks": [P, C.POINTER(Camera), C.POINTER(RenderOpts), ip, dp, ip],
               "mcpt_debug_bvh4_download": [P, I, np.ctypeslib.ndpointer(np.int64, flags="C"), P, P, P, C.c_int64, C.c_int64],
               "mcpt_debug_bvh4_host": [P, I, np.ctypeslib.ndpointer(np.int64, flags="C"), P, P, P, C.c_int64, C.c_int64],
               "mcpt_debug_bvh4_check_device_light": [P, I, np.ctypeslib.ndpointer(np.int64, flags="C")],
               "mcpt_debug_light_tables": [P, I, C.c_char_p, P, C.c_int64, C.POINTER(C.c_int64)],
               "mcpt_debug_light_area_cum_bench": [P, I, I, C.POINTER(D)],
               "mcpt_debug_phong": [I, I, dp, dp], "mcpt_debug_device_bytes_live": [],
               "mcpt_debug_prep_pick_counts": [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]}
        for name, argt in dbg.items():
            if hasattr(L, name):
                getattr(L, name).argtypes = argt
        if hasattr(L, "mcpt_debug_device_bytes_live"):
            L.mcpt_debug_device_bytes_live.restype = C.c_int64
        L.mcpt_tone_map.argtypes = [dp, I, I, D, D, u8]
        L.mcpt_write_bmp.argtypes = [C.c_char_p, u8, I, I]
        L.mcpt_comm_unique_id.argtypes = [C.c_char_p]
        L.mcpt_comm_init_rank.argtypes = [I, I, C.c_char_p, I, C.POINTER(P)]
        L.mcpt_comm_destroy.argtypes = [P]
        L.mcpt_comm_destroy.restype = None
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise MCPTError("mcpt error %d: %s" % (rc, lib().mcpt_last_error().decode()))


def _d(x, shape=None):
    a = np.ascontiguousarray(x, dtype=np.float64)
    return a if shape is None else a.reshape(shape)


class Scene:
    """Myobj + Mylight: an OBJ/MTL scene and its <light mtlname radiance> XML (main.cpp:500-504)."""

    def __init__(self, handle):
        self.h = handle
        # bound now: at interpreter shutdown the module's globals (lib) may already be gone when __del__ runs
        self._destroy = lib().mcpt_scene_destroy
        f, m, n = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().mcpt_scene_counts(self.h, C.byref(f), C.byref(m), C.byref(n)))
        self.nfacets, self.nmaterials, self.nlights = f.value, m.value, n.value

    @classmethod
    def load(cls, obj_path, xml_path):
        h = C.c_void_p()
        _check(lib().mcpt_scene_load(os.fsencode(obj_path), os.fsencode(xml_path), C.byref(h)))
        return cls(h)

    @classmethod
    def create(cls, positions, normals, material_id, materials, light_facet, light_radiance, light_group=None):
        """mcpt_scene_create: the flattened-array form (the arrays of Scene.arrays(); the library copies them).
        light_group: optional ascending index of each light triangle's <light>."""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 9)
        nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 9)
        mat = np.ascontiguousarray(material_id, np.int32).reshape(-1)
        mtl = np.ascontiguousarray(materials, np.float32).reshape(-1, 7)
        lf = np.ascontiguousarray(light_facet, np.int32).reshape(-1)
        lr = np.ascontiguousarray(light_radiance, np.float64).reshape(-1, 3)
        lg = None if light_group is None else np.ascontiguousarray(light_group, np.int32).reshape(-1)
        if nrm.shape != pos.shape or mat.shape[0] != pos.shape[0] or lr.shape[0] != lf.shape[0] or \
                (lg is not None and lg.shape[0] != lf.shape[0]):
            raise MCPTError("Scene.create: array shapes do not match")
        ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        d = SceneDesc(pos.shape[0], mtl.shape[0], lf.shape[0], ptr(pos), ptr(nrm), ptr(mat), ptr(mtl), ptr(lf), ptr(lr), ptr(lg))
        h = C.c_void_p()
        _check(lib().mcpt_scene_create(C.byref(d), C.byref(h)))
        return cls(h)

    def close(self):
        if getattr(self, "h", None):
            self._destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def update(self, first, positions, normals=None):
        """mcpt_scene_update: facets [first, first + len(positions)) get new vertex positions (n x 9 floats) and,
        unless normals is None, new vertex normals; the BVH is refit in place on the host and on every device the
        scene lives on.  Light triangles cannot move unless set_lights_movable() switched them to movable.  Returns the call's mcpt_update_stats as a dict."""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 9)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 9)
        if nrm is not None and nrm.shape != pos.shape:
            raise MCPTError("Scene.update: normals must match positions")
        st = UpdateStats()
        lib().mcpt_update_stats_init(C.byref(st))
        _check(lib().mcpt_scene_update(self.h, int(first), pos.shape[0], pos.ctypes.data_as(C.c_void_p),
                                       None if nrm is None else nrm.ctypes.data_as(C.c_void_p), C.byref(st)))
        return st.as_dict()

    def update_device(self, first, count, positions_ptr, normals_ptr=None, device=None):
        """mcpt_scene_update_device: the same from device memory (count x 9 floats each) on `device`."""
        st = UpdateStats()
        lib().mcpt_update_stats_init(C.byref(st))
        _check(lib().mcpt_scene_update_device(self.h, -1 if device is None else int(device), int(first), int(count),
                                              C.c_void_p(positions_ptr), C.c_void_p(normals_ptr) if normals_ptr else None,
                                              C.byref(st)))
        return st.as_dict()

    def set_lights_movable(self, on=True):
        """mcpt_scene_set_lights_movable: while on, update(), update_device() and transform() accept ranges that
        contain light triangles; the light tables and the light-only tree follow on every device, and the scene
        behaves as Scene.create of the new arrays would.  Off (the default) restores the refusals."""
        _check(lib().mcpt_scene_set_lights_movable(self.h, 1 if on else 0))

    @property
    def lights_movable(self):
        """mcpt_scene_lights_movable: the switch"""
        on = C.c_int32(0)
        _check(lib().mcpt_scene_lights_movable(self.h, C.byref(on)))
        return bool(on.value)

    def light_update_info(self):
        """mcpt_scene_light_update_info: the light stage's numbers of the last successful update / transform call as a
        dict (lights, chunks, groups, light_nodes_refit, light_levels, device_seconds)."""
        st = LightUpdateStats()
        lib().mcpt_light_update_stats_init(C.byref(st))
        _check(lib().mcpt_scene_light_update_info(self.h, C.byref(st)))
        return st.as_dict()

    def _relight(self, call, *args):
        st = RelightStats()
        lib().mcpt_relight_stats_init(C.byref(st))
        _check(call(self.h, *args, C.byref(st)))
        return st.as_dict()

    def set_light_radiance(self, first_light, radiance):
        """mcpt_scene_set_light_radiance: lights [first_light, first_light + n) of the light table get the radiances
        `radiance` (n x 3), on the host copy and on every device the scene lives on; the scene then behaves as
        Scene.create of the new arrays with light_group=self.light_groups() would (a re-light never regroups).  Zero
        switches a light off.  Returns the call's mcpt_relight_stats as a dict."""
        rgb = _d(radiance).reshape(-1, 3)
        return self._relight(lib().mcpt_scene_set_light_radiance, int(first_light), rgb.shape[0], rgb.ctypes.data_as(C.c_void_p))

    def set_light_radiance_device(self, first_light, count, ptr, device=None):
        """mcpt_scene_set_light_radiance_device: the same from count x 3 doubles of device memory on `device`."""
        return self._relight(lib().mcpt_scene_set_light_radiance_device, -1 if device is None else int(device), int(first_light),
                             int(count), C.c_void_p(ptr))

    def set_group_radiance(self, g, rgb):
        """every light of group g (an index of light_groups()) set to the one colour rgb"""
        ls = np.flatnonzero(self.light_groups() == int(g))
        if ls.size == 0:
            raise MCPTError("Scene.set_group_radiance: the scene has no lights in group %d" % int(g))
        return self.set_light_radiance(int(ls[0]), np.tile(_d(rgb, (1, 3)), (ls.size, 1)))

    def set_materials(self, first, materials):
        """mcpt_scene_set_materials: rows [first, first + n) of the material table get `materials` (n x 7: Kd[3] Ks[3]
        Ns), on the host copy and on every device the scene lives on.  Returns the call's mcpt_relight_stats as a dict."""
        mtl = np.ascontiguousarray(materials, np.float32).reshape(-1, 7)
        return self._relight(lib().mcpt_scene_set_materials, int(first), mtl.shape[0], mtl.ctypes.data_as(C.c_void_p))

    def light_groups(self):
        """mcpt_scene_light_groups: the group index of every light (ascending): what Scene.create's light_group takes"""
        g = np.zeros(max(self.nlights, 1), np.int32)
        _check(lib().mcpt_scene_light_groups(self.h, g))
        return g[:self.nlights]

    def pose_save(self):
        """mcpt_scene_pose_save: the current vertex positions and normals become the scene's previous pose, on the host
        copy and (device to device) on every device the scene lives on; update() never touches it.  A frame loop is
        pose_save, update, frame: render_motion_aovs then tells where each visible surface point was a frame ago."""
        _check(lib().mcpt_scene_pose_save(self.h))

    def rest_save(self):
        """mcpt_scene_rest_save: the current vertex positions and normals become the scene's rest pose, the source of
        every transform(); on the host copy and (device to device) on every device the scene lives on."""
        _check(lib().mcpt_scene_rest_save(self.h))

    def transform(self, first, count, m, normal_m=None):
        """mcpt_scene_transform: facets [first, first + count) := m (anything that reshapes to 3 x 4) applied to their
        rest pose, normal_m (3 x 3, None = the linear part of m) to their vertex normals, by the header's fp64 rule.
        Once the scene lives on a device the arithmetic runs there and the host copy only follows on demand
        (host_pending, host_sync; arrays() and every other reader sync by themselves).  Returns the stats dict of
        update()."""
        mm = _d(m).reshape(12)
        nm = None if normal_m is None else _d(normal_m).reshape(9)
        st = UpdateStats()
        lib().mcpt_update_stats_init(C.byref(st))
        _check(lib().mcpt_scene_transform(self.h, int(first), int(count), mm.ctypes.data_as(C.c_void_p),
                                          None if nm is None else nm.ctypes.data_as(C.c_void_p), C.byref(st)))
        return st.as_dict()

    def host_pending(self):
        """mcpt_scene_host_pending: how many facets of the host copy are behind the devices (0: in sync)"""
        n = C.c_int64(0)
        _check(lib().mcpt_scene_host_pending(self.h, C.byref(n)))
        return int(n.value)

    def host_sync(self):
        """mcpt_scene_host_sync: brings the host copy up to date now (a no-op when nothing is pending)"""
        _check(lib().mcpt_scene_host_sync(self.h))

    def rebuild(self):
        """mcpt_scene_rebuild: on every device the scene lives on, the main 4-wide tree is replaced by one built there
        from the current positions (the refit of update() and transform() keeps the topology, so the tree degrades as
        geometry moves far).  The host copy is neither read nor synced.  Returns the call's mcpt_rebuild_stats as a
        dict; device_states is 0, and nothing changed, while the scene lives on no device."""
        st = RebuildStats()
        lib().mcpt_rebuild_stats_init(C.byref(st))
        _check(lib().mcpt_scene_rebuild(self.h, C.byref(st)))
        return st.as_dict()

    def tree_cost(self, device=None):
        """mcpt_scene_tree_cost: the surface-area cost of the 4-wide tree `device` holds (the header's formula), the
        number a rebuild policy can watch: it grows as the refit tree degrades and drops at a rebuild."""
        c = C.c_double(0.0)
        _check(lib().mcpt_scene_tree_cost(self.h, -1 if device is None else int(device), C.byref(c)))
        return float(c.value)

    def set_visible(self, first, count, visible=True):
        """mcpt_scene_set_visible: facets [first, first + count) become invisible (visible=False) or visible again, on
        the host copy and on every device the scene lives on.  No ray of any call hits a hidden facet; its index, its
        rows of arrays() and its material stay, and update() / transform() of a hidden facet store values that appear
        when it is shown.  Light triangles cannot be hidden; the grid modes are refused while anything is.  Returns
        the stats dict of update()."""
        st = UpdateStats()
        lib().mcpt_update_stats_init(C.byref(st))
        _check(lib().mcpt_scene_set_visible(self.h, int(first), int(count), 1 if visible else 0, C.byref(st)))
        return st.as_dict()

    def hide(self, first, count):
        """set_visible(first, count, False)"""
        return self.set_visible(first, count, False)

    def show(self, first, count):
        """set_visible(first, count, True)"""
        return self.set_visible(first, count, True)

    def visible(self):
        """mcpt_scene_visibility: a bool per facet, False where it is hidden"""
        v = np.zeros(max(self.nfacets, 1), np.uint8)
        _check(lib().mcpt_scene_visibility(self.h, v.ctypes.data_as(C.c_void_p), None))
        return v[:self.nfacets].astype(bool)

    def hidden_count(self):
        """mcpt_scene_visibility: how many facets are hidden"""
        n = C.c_int32(0)
        _check(lib().mcpt_scene_visibility(self.h, None, C.byref(n)))
        return int(n.value)

    def arrays(self):
        F, M, NL = self.nfacets, self.nmaterials, self.nlights
        pos, nrm = np.zeros((F, 9), np.float32), np.zeros((F, 9), np.float32)
        mat, mtl = np.zeros(F, np.int32), np.zeros((M, 7), np.float32)
        lf, lr, un = np.zeros(max(NL, 1), np.int32), np.zeros((max(NL, 1), 3)), np.zeros((F, 3))
        _check(lib().mcpt_scene_arrays(self.h, pos, nrm, mat, mtl, lf, lr, un))
        return dict(positions=pos, normals=nrm, material_id=mat, materials=mtl, light_facet=lf[:NL],
                    light_radiance=lr[:NL], unique_normal=un)

    def meshing(self, eye, n0=100000):
        """Myobj::cal_scene_boundingbox(eye) + Myobj::meshing(n0) (Myobj.cpp:78-162): the reference's
        uniform grid, for closest_hit(..., grid=True)."""
        _check(lib().mcpt_scene_meshing(self.h, _d(eye, (3,)), int(n0)))

    def grid_info(self):
        """((xmin, xmax, ymin, ymax, zmin, zmax, cell edge), cells per axis) of the current grid"""
        box, cells = np.zeros(7), np.zeros(3, np.int32)
        _check(lib().mcpt_scene_grid_info(self.h, box, cells))
        return box, cells

    def accel_bytes(self):
        """device bytes of the BVHs the traversal reads (mcpt_scene_accel_bytes)"""
        b = C.c_uint64()
        _check(lib().mcpt_scene_accel_bytes(self.h, C.byref(b)))
        return b.value

    def camera(self):
        c = Camera()
        _check(lib().mcpt_scene_camera(self.h, C.byref(c)))
        return c


class Comm:
    """mcpt_comm: this process's rank of a multi-process RCCL communicator owned by the library
    (one process per GPU).  Rank 0 calls Comm.unique_id(); the caller broadcasts the bytes (e.g.
    torch.distributed.broadcast_object_list); every rank then constructs Comm(nranks, rank, id, device).
    Renders with comm=... render this rank's share of the job's sample range and end with ONE
    ncclReduce(sum) into rank 0's buffer."""

    def __init__(self, nranks, rank, uid, device=-1):
        if len(uid) != COMM_ID_BYTES:
            raise ValueError("comm id must be %d bytes" % COMM_ID_BYTES)
        h = C.c_void_p()
        self._destroy = lib().mcpt_comm_destroy
        _check(lib().mcpt_comm_init_rank(int(nranks), int(rank), bytes(uid), int(device), C.byref(h)))
        self.h, self.nranks, self.rank = h, int(nranks), int(rank)

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _check(lib().mcpt_comm_unique_id(buf))
        return buf.raw

    def close(self):
        if getattr(self, "h", None):
            self._destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def set_collective_lib(path):
    """Test infrastructure (include/mcpt_debug.h): use the NCCL-API library at `path` (the host-memory
    collective tests/collshim/libmcpt_collshim.so) instead of RCCL for this process's communicators, so
    several ranks can share one GPU.  Must precede the first Comm / device-list render."""
    _check(lib().mcpt_debug_set_collective_lib(os.fsencode(path)))


def _opts(spp, mode, seed, sample_range, device, samples_per_launch, queue_factor, progress=None, accel="bvh",
          flags=0, devices=None, comm=None):
    """progress(done, total) -> truthy to cancel; the ctypes thunk is kept on the returned struct.
    devices: list of device ordinals (one process, several GPUs); comm: a Comm (one process per GPU)."""
    o = RenderOpts()
    lib().mcpt_render_opts_init(C.byref(o))
    o.flags = int(flags)
    if devices is not None:
        o._devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        o.num_devices = len(devices)
        o.devices = C.cast(o._devs, C.POINTER(C.c_int32))
    if comm is not None:
        o.comm = comm.h
    a = {"bvh": ACCEL_BVH, "grid": ACCEL_GRID}.get(accel, -1) if isinstance(accel, str) else int(accel)
    if a not in (ACCEL_BVH, ACCEL_GRID):
        raise ValueError("accel must be 'bvh' or 'grid'")
    o.accel = a
    if progress is not None:
        o._thunk = PROGRESS_FN(lambda _u, done, total: 1 if progress(int(done), int(total)) else 0)
        o.progress = C.cast(o._thunk, C.c_void_p)
    o.spp = int(spp)
    o.sample_begin = o.sample_end = 0
    m = MODES.get(mode, -1) if isinstance(mode, str) else int(mode)
    if m not in MODES.values():
        raise ValueError("mode must be one of %s" % sorted(MODES))
    o.mode = m
    o.seed = int(seed)
    if sample_range is not None:
        o.sample_begin, o.sample_end = int(sample_range[0]), int(sample_range[1])
    o.device = -1 if device is None else int(device)
    o.samples_per_launch = int(samples_per_launch or 0)
    o.queue_factor = int(queue_factor or 0)
    return o


def render(scene, camera, spp, mode="mis", seed=DEFAULT_SEED, sample_range=None, out=None, device=None,
           samples_per_launch=0, queue_factor=0, progress=None, accel="bvh", devices=None, comm=None, flags=0):
    """render(scene, camera, spp, mode) -- main.cpp:547-588.  Returns (H x W x 3 fp64 radiance, Stats).

    Adds sum_k L_k / spp over samples k in `sample_range` (default all) into `out` (zeros if None).
    progress(samples_dispatched, samples_total), called after every wavefront generation, replaces
    the reference's per-row progress output; a truthy return cancels (MCPTError, partial sum).
    accel="grid" traces every ray through the reference's uniform grid (Myobj.cpp:78-162) instead of
    the BVH: hit-for-hit the reference's traversal, crack included.
    devices=[d0, d1, ...] shards the sample range over several GPUs of this process (one thread and
    stream each; a device may repeat) and sums them with one RCCL reduce; comm=Comm(...) renders this
    rank's share and reduces to rank 0 (see mcpt_render_opts in include/mcpt.h)."""
    if out is None:
        out = np.zeros((camera.height, camera.width, 3))
    assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (camera.height, camera.width, 3)
    st = Stats()
    o = _opts(spp, mode, seed, sample_range, device, samples_per_launch, queue_factor, progress, accel, flags,
              devices, comm)
    _check(lib().mcpt_render(scene.h, C.byref(camera), C.byref(o), out.reshape(-1), C.byref(st)))
    return out, st


def render_device(scene, camera, spp, dev_ptr, mode="mis", seed=DEFAULT_SEED, sample_range=None, device=None,
                  samples_per_launch=0, queue_factor=0, progress=None, accel="bvh", flags=0, devices=None, comm=None):
    """Accumulate into a device buffer of H*W*3 doubles (e.g. a torch.float64 CUDA tensor's data_ptr()).
    flags: RENDER_NO_BACKFACE_STATS skips the light-side cull statistic (mcpt_render_opts.flags)."""
    st = Stats()
    o = _opts(spp, mode, seed, sample_range, device, samples_per_launch, queue_factor, progress, accel, flags,
              devices, comm)
    _check(lib().mcpt_render_device(scene.h, C.byref(camera), C.byref(o), C.c_void_p(int(dev_ptr)), C.byref(st)))
    return st


def render_rays(scene, origin, dir, spp, mode="mis", seed=DEFAULT_SEED, sample_range=None, out=None, device=None,
                samples_per_launch=0, queue_factor=0, progress=None, flags=0):
    """Radiance along caller-supplied rays (mcpt_render_rays, include/mcpt.h): origin and dir are n x 3, used as given
    (dir is not normalised).  Returns (n x 3 fp64 radiance, Stats): sum_k L_k / spp over the samples k in
    `sample_range` (default all) ADDED into `out` (zeros if None); sample k of ray r draws the random numbers of
    (seed, pixel r, sample k).  The seam for other camera models: camera_rays gives this renderer's own rays.
    Single device, BVH only."""
    origin, dir = _d(origin, (-1, 3)), _d(dir, (-1, 3))
    n = origin.shape[0]
    assert dir.shape == (n, 3)
    if out is None:
        out = np.zeros((n, 3))
    assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (n, 3)
    st = Stats()
    o = _opts(spp, mode, seed, sample_range, device, samples_per_launch, queue_factor, progress, "bvh", flags)
    _check(lib().mcpt_render_rays(scene.h, C.byref(o), n, origin.ctypes.data, dir.ctypes.data, out.ctypes.data, C.byref(st)))
    return out, st


def render_rays_device(scene, n, origin_ptr, dir_ptr, spp, dev_ptr, mode="mis", seed=DEFAULT_SEED, sample_range=None,
                       device=None, samples_per_launch=0, queue_factor=0, progress=None, flags=0):
    """render_rays over device buffers of n*3 doubles each (e.g. torch.float64 CUDA tensors' data_ptr()): the
    radiance is accumulated into dev_ptr.  Returns the Stats."""
    st = Stats()
    o = _opts(spp, mode, seed, sample_range, device, samples_per_launch, queue_factor, progress, "bvh", flags)
    opt = lambda p: None if p is None else C.c_void_p(int(p))
    _check(lib().mcpt_render_rays_device(scene.h, C.byref(o), int(n), opt(origin_ptr), opt(dir_ptr), opt(dev_ptr), C.byref(st)))
    return st


def render_rays_indexed(scene, index, origin, dir, out_n, spp, mode="mis", seed=DEFAULT_SEED, sample_range=None, out=None,
                        device=None, samples_per_launch=0, queue_factor=0, progress=None, flags=0):
    """mcpt_render_rays_indexed (include/mcpt.h): render_rays for a sparse set of a frame's pixels.  index holds n pixel
    ids in [0, out_n), origin and dir are n x 3.  Returns (out_n x 3 fp64 radiance, Stats): ray r's sum is ADDED into
    row index[r] of `out` (zeros if None) and nothing else is written; sample k of ray r draws the random numbers of
    (seed, pixel index[r], sample k).  Duplicate ids add the same samples again.  Single device, BVH only."""
    index = np.ascontiguousarray(index, dtype=np.int32).reshape(-1)
    origin, dir = _d(origin, (-1, 3)), _d(dir, (-1, 3))
    n = index.shape[0]
    assert origin.shape == (n, 3) and dir.shape == (n, 3)
    if out is None:
        out = np.zeros((max(int(out_n), 0), 3))
    assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (max(int(out_n), 0), 3)
    st = Stats()
    o = _opts(spp, mode, seed, sample_range, device, samples_per_launch, queue_factor, progress, "bvh", flags)
    _check(lib().mcpt_render_rays_indexed(scene.h, C.byref(o), n, index.ctypes.data, origin.ctypes.data, dir.ctypes.data,
                                          int(out_n), out.ctypes.data, C.byref(st)))
    return out, st


def render_rays_indexed_device(scene, n, index_ptr, origin_ptr, dir_ptr, out_n, spp, dev_ptr, mode="mis", seed=DEFAULT_SEED,
                               sample_range=None, device=None, samples_per_launch=0, queue_factor=0, progress=None, flags=0):
    """render_rays_indexed over device buffers (n int32 ids, n*3 doubles each of origins and directions, out_n*3 doubles
    at dev_ptr, e.g. torch CUDA tensors' data_ptr()): the radiance is accumulated into dev_ptr.  An id outside
    [0, out_n) is found by the kernel: that ray adds nothing and the call raises after the run.  Returns the Stats."""
    st = Stats()
    o = _opts(spp, mode, seed, sample_range, device, samples_per_launch, queue_factor, progress, "bvh", flags)
    opt = lambda p: None if p is None else C.c_void_p(int(p))
    _check(lib().mcpt_render_rays_indexed_device(scene.h, C.byref(o), int(n), opt(index_ptr), opt(origin_ptr), opt(dir_ptr),
                                                 int(out_n), opt(dev_ptr), C.byref(st)))
    return st


def camera_rays(camera, seed=DEFAULT_SEED, sample=0, jitter=False, device=None):
    """mcpt_camera_rays: the camera's rays for sample index `sample` as (origin, dir), H*W x 3 each in pixel order:
    through the pixel centres, or (jitter=True) the rays a render with RENDER_PIXEL_JITTER shoots for (seed, sample) --
    computed on the device by the function the render itself calls."""
    n = camera.width * camera.height
    origin, dir = np.zeros((n, 3)), np.zeros((n, 3))
    _check(lib().mcpt_camera_rays(C.byref(camera), int(seed), int(sample), int(jitter), -1 if device is None else int(device),
                                  origin.ctypes.data, dir.ctypes.data))
    return origin, dir


def _adaptive_opts(max_spp, threshold, min_spp, pass_spp, radius):
    a = AdaptiveOpts()
    lib().mcpt_adaptive_opts_init(C.byref(a))
    a.max_spp, a.threshold, a.radius = int(max_spp), float(threshold), int(radius)
    if min_spp is not None:
        a.min_spp = int(min_spp)
    if pass_spp is not None:
        a.pass_spp = int(pass_spp)
    return a


def _adaptive_base(mode, seed, device, samples_per_launch, queue_factor, progress, accel, flags):
    o = _opts(0, mode, seed, None, device, samples_per_launch, queue_factor, progress, accel, flags)
    d = RenderOpts()
    lib().mcpt_render_opts_init(C.byref(d))
    o.spp = d.spp  # left at its default: the sample counts come from the adaptive options
    return o


def render_adaptive(scene, camera, max_spp, threshold, min_spp=None, pass_spp=None, radius=1, mode="mis",
                    seed=DEFAULT_SEED, out=None, device=None, samples_per_launch=0, queue_factor=0, progress=None,
                    accel="bvh", flags=0):
    """Adaptive sampling (mcpt_render_adaptive, include/mcpt.h): render in passes of pass_spp samples after
    the first min_spp (library defaults: 16 each), estimate each active pixel's noise e after every pass and
    stop sampling the pixels with e <= threshold whose neighbours within `radius` have converged too; no pixel
    takes more than max_spp.  Returns (image, count, noise, Stats): the H x W x 3 mean radiance ADDED into
    `out` (zeros if None), the int32 H x W samples taken and the H x W last noise estimate.  Single device."""
    if out is None:
        out = np.zeros((camera.height, camera.width, 3))
    assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape == (camera.height, camera.width, 3)
    count = np.zeros((camera.height, camera.width), np.int32)
    noise = np.zeros((camera.height, camera.width))
    st = Stats()
    o = _adaptive_base(mode, seed, device, samples_per_launch, queue_factor, progress, accel, flags)
    a = _adaptive_opts(max_spp, threshold, min_spp, pass_spp, radius)
    _check(lib().mcpt_render_adaptive(scene.h, C.byref(camera), C.byref(o), C.byref(a), out.reshape(-1),
                                      count.ctypes.data_as(C.c_void_p), noise.ctypes.data_as(C.c_void_p), C.byref(st)))
    return out, count, noise, st


def render_adaptive_device(scene, camera, max_spp, threshold, dev_ptr, count_ptr=None, noise_ptr=None, min_spp=None,
                           pass_spp=None, radius=1, mode="mis", seed=DEFAULT_SEED, device=None, samples_per_launch=0,
                           queue_factor=0, progress=None, accel="bvh", flags=0):
    """render_adaptive into device buffers (e.g. torch CUDA tensors' data_ptr()): dev_ptr H*W*3 float64
    (added into), count_ptr H*W int32 and noise_ptr H*W float64 (overwritten; either may be None)."""
    st = Stats()
    o = _adaptive_base(mode, seed, device, samples_per_launch, queue_factor, progress, accel, flags)
    a = _adaptive_opts(max_spp, threshold, min_spp, pass_spp, radius)
    _check(lib().mcpt_render_adaptive_device(
        scene.h, C.byref(camera), C.byref(o), C.byref(a), C.c_void_p(int(dev_ptr)),
        None if count_ptr is None else C.c_void_p(int(count_ptr)),
        None if noise_ptr is None else C.c_void_p(int(noise_ptr)), C.byref(st)))
    return st


def _aov_opts(device, accel, flags=0):
    return _opts(1, "mis", DEFAULT_SEED, None, device, 0, 0, accel=accel, flags=flags)


def render_aovs(scene, camera, device=None, accel="bvh", flags=0):
    """Primary-hit feature buffers (mcpt_render_aovs, include/mcpt.h): dict of albedo (Kd + Ks), normal (shading
    normal, not flipped), position (H x W x 3 each) and depth (H x W, distance from the pulled-back eye; 0 marks a
    miss, whose other maps are 0 too).  flags are ignored by the library (RENDER_PIXEL_JITTER too: the AOVs stay at
    the pixel centres); the keyword only lets a caller hand over a render's options unchanged."""
    H, W = camera.height, camera.width
    a = dict(albedo=np.zeros((H, W, 3)), normal=np.zeros((H, W, 3)), position=np.zeros((H, W, 3)), depth=np.zeros((H, W)))
    b = AovBuffers(*[a[k].ctypes.data for k in ("albedo", "normal", "position", "depth")])
    o = _aov_opts(device, accel, flags)
    _check(lib().mcpt_render_aovs(scene.h, C.byref(camera), C.byref(o), C.byref(b)))
    return a


def render_aovs_device(scene, camera, albedo_ptr=None, normal_ptr=None, position_ptr=None, depth_ptr=None, device=None,
                       accel="bvh"):
    """render_aovs into device buffers (e.g. torch CUDA float64 tensors' data_ptr()): H*W*3 doubles each, depth
    H*W; any may be None."""
    b = AovBuffers(*[None if p is None else int(p) for p in (albedo_ptr, normal_ptr, position_ptr, depth_ptr)])
    o = _aov_opts(device, accel)
    _check(lib().mcpt_render_aovs_device(scene.h, C.byref(camera), C.byref(o), C.byref(b)))


def render_motion_aovs(scene, camera, device=None, accel="bvh", flags=0):
    """Motion AOVs (mcpt_render_motion_aovs, include/mcpt.h): dict of prev_position and prev_normal (H x W x 3 each) --
    render_aovs' position and normal of every pixel's primary hit, evaluated over the scene's previous pose
    (Scene.pose_save); equal to them until the first pose_save, 0 at a miss."""
    H, W = camera.height, camera.width
    a = dict(prev_position=np.zeros((H, W, 3)), prev_normal=np.zeros((H, W, 3)))
    b = MotionBuffers(a["prev_position"].ctypes.data, a["prev_normal"].ctypes.data)
    o = _aov_opts(device, accel, flags)
    _check(lib().mcpt_render_motion_aovs(scene.h, C.byref(camera), C.byref(o), C.byref(b)))
    return a


def render_motion_aovs_device(scene, camera, prev_position_ptr=None, prev_normal_ptr=None, device=None, accel="bvh"):
    """render_motion_aovs into device buffers (e.g. torch CUDA float64 tensors' data_ptr()): H*W*3 doubles each; either
    may be None."""
    b = MotionBuffers(*[None if p is None else int(p) for p in (prev_position_ptr, prev_normal_ptr)])
    o = _aov_opts(device, accel)
    _check(lib().mcpt_render_motion_aovs_device(scene.h, C.byref(camera), C.byref(o), C.byref(b)))


def _denoise_opts(iterations, sigma_color, sigma_normal, sigma_plane, sigma_albedo, device):
    o = DenoiseOpts()
    lib().mcpt_denoise_opts_init(C.byref(o))
    for k, v in (("sigma_color", sigma_color), ("sigma_normal", sigma_normal), ("sigma_plane", sigma_plane),
                 ("sigma_albedo", sigma_albedo)):
        if v is not None:
            setattr(o, k, float(v))
    if iterations is not None:
        o.iterations = int(iterations)
    o.device = -1 if device is None else int(device)
    return o


def denoise(color, aovs, variance=None, iterations=None, sigma_color=None, sigma_normal=None, sigma_plane=None,
            sigma_albedo=None, device=None):
    """Variance-guided a-trous filter (mcpt_denoise; include/mcpt.h states the rule).  color H x W x 3, aovs the
    dict of render_aovs (all four maps), variance H x W (of the pixel's mean luminance, e.g. variance_from_noise)
    or None for the filter's own spatial estimate; None parameters take the library defaults (5 iterations,
    sigmas 4 / 128 / 0.01 / 0.1).  Returns (out, out_variance, device seconds)."""
    color = _d(color)
    H, W = color.shape[:2]
    assert color.shape == (H, W, 3)
    g = {k: _d(aovs[k], (H, W) if k == "depth" else (H, W, 3)) for k in ("albedo", "normal", "position", "depth")}
    b = AovBuffers(*[g[k].ctypes.data for k in ("albedo", "normal", "position", "depth")])
    var = None if variance is None else _d(variance, (H, W))
    out, out_var, sec = np.zeros((H, W, 3)), np.zeros((H, W)), C.c_double()
    o = _denoise_opts(iterations, sigma_color, sigma_normal, sigma_plane, sigma_albedo, device)
    _check(lib().mcpt_denoise(C.byref(o), W, H, color.ctypes.data, None if var is None else var.ctypes.data, C.byref(b),
                              out.ctypes.data, out_var.ctypes.data, C.byref(sec)))
    return out, out_var, sec.value


def denoise_device(width, height, color_ptr, aov_ptrs, out_ptr, variance_ptr=None, out_variance_ptr=None, iterations=None,
                   sigma_color=None, sigma_normal=None, sigma_plane=None, sigma_albedo=None, device=None):
    """denoise over device buffers (e.g. torch CUDA float64 tensors' data_ptr()): aov_ptrs is a dict of the four
    guides' pointers; variance_ptr and out_variance_ptr may be None.  Returns the device seconds."""
    b = AovBuffers(*[int(aov_ptrs[k]) for k in ("albedo", "normal", "position", "depth")])
    sec = C.c_double()
    o = _denoise_opts(iterations, sigma_color, sigma_normal, sigma_plane, sigma_albedo, device)
    _check(lib().mcpt_denoise_device(
        C.byref(o), int(width), int(height), C.c_void_p(int(color_ptr)),
        None if variance_ptr is None else C.c_void_p(int(variance_ptr)), C.byref(b), C.c_void_p(int(out_ptr)),
        None if out_variance_ptr is None else C.c_void_p(int(out_variance_ptr)), C.byref(sec)))
    return sec.value


def variance_from_noise(img, noise):
    """mcpt_variance_from_noise: render_adaptive's image and noise map as the variance of each pixel's mean
    luminance, V = (e sqrt(sum_c I_c) / 3)^2 -- the denoiser's `variance` input."""
    img = _d(img)
    H, W = img.shape[:2]
    var = np.zeros((H, W))
    _check(lib().mcpt_variance_from_noise(W, H, img.reshape(-1), _d(noise, (H, W)).reshape(-1), var.reshape(-1)))
    return var


def camera_orbit(camera, degrees):
    """mcpt_camera_orbit: a copy of `camera` with its eye rotated by `degrees` about the axis through lookat along
    up (the CLI's --orbit builds its cameras with the same function, so both are bit-identical)."""
    out = Camera()
    _check(lib().mcpt_camera_orbit(C.byref(camera), float(degrees), C.byref(out)))
    return out


def transform_rotation(axis, degrees, pivot, translate=None):
    """mcpt_transform_rotation: the (3, 4) float64 matrix of a rotation by `degrees` about the axis through `pivot`
    along `axis`, then + translate; for Scene.transform."""
    m = np.zeros((3, 4))
    ax, pv = _d(axis, (3,)), _d(pivot, (3,))
    tr = None if translate is None else _d(translate, (3,))
    _check(lib().mcpt_transform_rotation(ax.ctypes.data_as(C.c_void_p), float(degrees), pv.ctypes.data_as(C.c_void_p),
                                         None if tr is None else tr.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p)))
    return m


def camera_scaled(camera, factor):
    """mcpt_camera_scaled: a copy of `camera` with factor times the width and height -- the full-size camera of a
    low-size one (the same image plane: low pixel I spans the full-size rows factor I .. factor I + factor - 1)."""
    out = Camera()
    _check(lib().mcpt_camera_scaled(C.byref(camera), int(factor), C.byref(out)))
    return out


UPSAMPLE_OPTS = ("factor", "sigma_normal", "sigma_plane", "sigma_albedo", "min_weight")


def _upsample_opts(factor, sigma_normal, sigma_plane, sigma_albedo, min_weight, device):
    o = UpsampleOpts()
    lib().mcpt_upsample_opts_init(C.byref(o))
    if factor is not None:
        o.factor = int(factor)
    for k, v in (("sigma_normal", sigma_normal), ("sigma_plane", sigma_plane), ("sigma_albedo", sigma_albedo),
                 ("min_weight", min_weight)):
        if v is not None:
            setattr(o, k, float(v))
    o.device = -1 if device is None else int(device)
    return o


def upsample(color, aovs, full_aovs, factor=2, sigma_normal=None, sigma_plane=None, sigma_albedo=None, min_weight=None,
             device=None):
    """Guided upsampling (mcpt_upsample; include/mcpt.h states the rule): color h x w x 3 and aovs (the dict of
    render_aovs) at the low size, full_aovs the guides of camera_scaled(camera, factor) at (factor h) x (factor w).
    None parameters take the library defaults (sigmas 128 / 0.01 / 0.1, min_weight 1e-4).  Returns (the full-size
    frame, the number of pixels that took the fallback)."""
    color = _d(color)
    h, w = color.shape[:2]
    assert color.shape == (h, w, 3)
    f = int(factor)
    keys = ("albedo", "normal", "position", "depth")
    g = {k: _d(aovs[k], (h, w) if k == "depth" else (h, w, 3)) for k in keys}
    G = {k: _d(full_aovs[k], (f * h, f * w) if k == "depth" else (f * h, f * w, 3)) for k in keys}
    b, B = AovBuffers(*[g[k].ctypes.data for k in keys]), AovBuffers(*[G[k].ctypes.data for k in keys])
    out, n = np.zeros((f * h, f * w, 3)), C.c_uint64()
    o = _upsample_opts(f, sigma_normal, sigma_plane, sigma_albedo, min_weight, device)
    _check(lib().mcpt_upsample(C.byref(o), w, h, color.ctypes.data, C.byref(b), C.byref(B), out.ctypes.data, C.byref(n), None))
    return out, n.value


def upsample_device(width, height, color_ptr, aov_ptrs, full_aov_ptrs, out_ptr, factor=2, sigma_normal=None, sigma_plane=None,
                    sigma_albedo=None, min_weight=None, device=None):
    """upsample over device buffers (e.g. torch CUDA float64 tensors' data_ptr()): width and height are the low size,
    aov_ptrs and full_aov_ptrs dicts of the four guides' pointers at the low and the full size.  Returns (the
    fallback count, the device seconds)."""
    keys = ("albedo", "normal", "position", "depth")
    b, B = AovBuffers(*[int(aov_ptrs[k]) for k in keys]), AovBuffers(*[int(full_aov_ptrs[k]) for k in keys])
    n, sec = C.c_uint64(), C.c_double()
    o = _upsample_opts(factor, sigma_normal, sigma_plane, sigma_albedo, min_weight, device)
    _check(lib().mcpt_upsample_device(C.byref(o), int(width), int(height), C.c_void_p(int(color_ptr)), C.byref(b), C.byref(B),
                                      C.c_void_p(int(out_ptr)), C.byref(n), C.byref(sec)))
    return n.value, sec.value


def upsample_phase(factor, frame_index):
    """mcpt_upsample_phase: the phase (a, b) of frame `frame_index` of a temporally upsampled sequence at `factor`:
    k = frame_index mod factor^2, a = k mod factor, b = (a + k div factor) mod factor."""
    a, b = C.c_int32(), C.c_int32()
    _check(lib().mcpt_upsample_phase(int(factor), int(frame_index), C.byref(a), C.byref(b)))
    return a.value, b.value


def camera_phase_rays(full_camera, factor, a, b, device=None):
    """mcpt_camera_phase_rays: the rays of full_camera's pixels (factor I + a, factor J + b) as (origin, dir),
    (H / factor) * (W / factor) x 3 each, row-major in (I, J): camera_rays(full_camera)'s rays at those pixels bit for
    bit -- what a temporally upsampled frame of phase (a, b) traces."""
    n = (full_camera.width // int(factor)) * (full_camera.height // int(factor)) if int(factor) > 0 else 0
    origin, dir = np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 3))
    _check(lib().mcpt_camera_phase_rays(C.byref(full_camera), int(factor), int(a), int(b), -1 if device is None else int(device),
                                        origin.ctypes.data, dir.ctypes.data))
    return origin[:n], dir[:n]


def _fill_opts(factor, fill):
    """the UpsampleOpts of a temporal upsampling: the factor and the fill's dict"""
    u = dict(fill or {}, factor=factor)
    unknown = set(u) - set(UPSAMPLE_OPTS)
    if unknown:
        raise TypeError("unknown fill option %r (one of %s)" % (sorted(unknown)[0], ", ".join(UPSAMPLE_OPTS[1:])))
    return _upsample_opts(*[u.get(k) for k in UPSAMPLE_OPTS], None)


def temporal_upsample(color, full_aovs, a, b, prev=None, factor=2, fill=None, **opts):
    """Temporal upsampling (mcpt_temporal_upsample; include/mcpt.h states the rule).  color h x w x 3 holds the radiance
    of the full-size pixels (factor I + a, factor J + b) (render_rays over camera_phase_rays), full_aovs the guides of the
    full-size camera at (factor h) x (factor w); prev is None or the previous FULL-SIZE state (camera, aovs, colour,
    moments): the full-size Camera and guides of the previous frame and the colour and moments this function returned for
    it.  fill: None or a dict of the fill's sigma_normal, sigma_plane, sigma_albedo and min_weight (UpsampleOpts; they
    share their names with the accumulation's); opts: the fields of TemporalOpts, as for temporal_accumulate.  Returns (colour, moments (m1, m2, n, g), variance -- all full size --, the
    number of filled pixels, the number of them that took the fallback, the device seconds)."""
    color = _d(color)
    h, w = color.shape[:2]
    assert color.shape == (h, w, 3)
    f = int(factor)
    H, W = f * h, f * w
    keys = ("albedo", "normal", "position", "depth")
    g = {k: _d(full_aovs[k], (H, W) if k == "depth" else (H, W, 3)) for k in keys}
    B = AovBuffers(*[g[k].ctypes.data for k in keys])
    pc = pb = pcol = pmom = None
    if prev is not None:
        pcam, paov, pcol, pmom = prev
        pg = {k: _d(paov[k], (H, W) if k == "depth" else (H, W, 3)) for k in keys[1:]}
        pb = AovBuffers(None, *[pg[k].ctypes.data for k in keys[1:]])
        pcol, pmom = _d(pcol, (H, W, 3)), _d(pmom, (H, W, 4))
        pc = C.byref(pcam)
    out, mom, var = np.zeros((H, W, 3)), np.zeros((H, W, 4)), np.zeros((H, W))
    filled, fell, sec = C.c_uint64(), C.c_uint64(), C.c_double()
    o, u = _temporal_opts(opts), _fill_opts(f, fill)
    _check(lib().mcpt_temporal_upsample(
        C.byref(o), C.byref(u), int(a), int(b), pc, w, h, color.ctypes.data, C.byref(B), None if pb is None else C.byref(pb),
        None if pcol is None else pcol.ctypes.data, None if pmom is None else pmom.ctypes.data, out.ctypes.data,
        mom.ctypes.data, var.ctypes.data, C.byref(filled), C.byref(fell), C.byref(sec)))
    return out, mom, var, filled.value, fell.value, sec.value


def temporal_upsample_device(width, height, color_ptr, full_aov_ptrs, a, b, out_color_ptr, out_moments_ptr,
                             out_variance_ptr=None, prev=None, factor=2, fill=None, **opts):
    """temporal_upsample over device buffers (e.g. torch CUDA float64 tensors' data_ptr()): width and height are the low
    size, full_aov_ptrs a dict of the four full-size guides' pointers; prev is None or (full-size camera, dict of the
    previous normal / position / depth pointers, previous colour pointer, previous moments pointer); out_variance_ptr
    may be None.  Returns (filled count, fallback count, device seconds)."""
    B = AovBuffers(*[int(full_aov_ptrs[k]) for k in ("albedo", "normal", "position", "depth")])
    pc = pb = pcol = pmom = None
    if prev is not None:
        pcam, paov, pcol, pmom = prev
        pb = AovBuffers(None, *[int(paov[k]) for k in ("normal", "position", "depth")])
        pc, pcol, pmom = C.byref(pcam), C.c_void_p(int(pcol)), C.c_void_p(int(pmom))
    filled, fell, sec = C.c_uint64(), C.c_uint64(), C.c_double()
    o, u = _temporal_opts(opts), _fill_opts(factor, fill)
    _check(lib().mcpt_temporal_upsample_device(
        C.byref(o), C.byref(u), int(a), int(b), pc, int(width), int(height), C.c_void_p(int(color_ptr)), C.byref(B),
        None if pb is None else C.byref(pb), pcol, pmom, C.c_void_p(int(out_color_ptr)), C.c_void_p(int(out_moments_ptr)),
        None if out_variance_ptr is None else C.c_void_p(int(out_variance_ptr)), C.byref(filled), C.byref(fell), C.byref(sec)))
    return filled.value, fell.value, sec.value


TEMPORAL_OPTS = ("alpha", "max_history", "normal_min", "plane_max", "min_weight", "variance_min_history", "sigma_normal",
                 "sigma_plane", "sigma_albedo", "device")


def _temporal_opts(opts):
    o = TemporalOpts()
    lib().mcpt_temporal_opts_init(C.byref(o))
    for k, v in opts.items():
        if k not in TEMPORAL_OPTS:
            raise TypeError("unknown temporal option %r (one of %s)" % (k, ", ".join(TEMPORAL_OPTS)))
        if v is not None:
            setattr(o, k, type(getattr(o, k))(v))
    return o


def temporal_accumulate(color, aovs, prev=None, **opts):
    """Temporal accumulation (mcpt_temporal_accumulate; include/mcpt.h states the rule).  color H x W x 3 and aovs
    (the dict of render_aovs) are the current frame; prev is None (every pixel starts a history) or the previous
    state (camera, aovs, colour, moments): that frame's Camera and guides and the colour and moments this function
    returned for it.  opts: the fields of TemporalOpts (alpha, max_history, normal_min, plane_max, min_weight,
    variance_min_history, sigma_normal, sigma_plane, sigma_albedo, device); None or absent = the library default.
    Returns (colour H x W x 3, moments H x W x 4 of (m1, m2, n, g), variance H x W of the accumulated luminance --
    the `variance` input of denoise -- and the device seconds)."""
    color = _d(color)
    H, W = color.shape[:2]
    assert color.shape == (H, W, 3)
    keys = ("albedo", "normal", "position", "depth")
    g = {k: _d(aovs[k], (H, W) if k == "depth" else (H, W, 3)) for k in keys}
    b = AovBuffers(*[g[k].ctypes.data for k in keys])
    pc = pb = pcol = pmom = None
    if prev is not None:
        pcam, paov, pcol, pmom = prev
        pg = {k: _d(paov[k], (H, W) if k == "depth" else (H, W, 3)) for k in keys[1:]}
        pb = AovBuffers(None, *[pg[k].ctypes.data for k in keys[1:]])
        pcol, pmom = _d(pcol, (H, W, 3)), _d(pmom, (H, W, 4))
        pc = C.byref(pcam)
    out, mom, var, sec = np.zeros((H, W, 3)), np.zeros((H, W, 4)), np.zeros((H, W)), C.c_double()
    o = _temporal_opts(opts)
    _check(lib().mcpt_temporal_accumulate(
        C.byref(o), pc, W, H, color.ctypes.data, C.byref(b), None if pb is None else C.byref(pb),
        None if pcol is None else pcol.ctypes.data, None if pmom is None else pmom.ctypes.data, out.ctypes.data,
        mom.ctypes.data, var.ctypes.data, C.byref(sec)))
    return out, mom, var, sec.value


def temporal_accumulate_device(width, height, color_ptr, aov_ptrs, out_color_ptr, out_moments_ptr, out_variance_ptr=None,
                               prev=None, **opts):
    """temporal_accumulate over device buffers (e.g. torch CUDA float64 tensors' data_ptr()): aov_ptrs is a dict of
    the four guides' pointers; prev is None or (camera, dict of the previous normal / position / depth pointers,
    previous colour pointer, previous moments pointer); out_variance_ptr may be None.  Returns the device seconds."""
    b = AovBuffers(*[int(aov_ptrs[k]) for k in ("albedo", "normal", "position", "depth")])
    pc = pb = pcol = pmom = None
    if prev is not None:
        pcam, paov, pcol, pmom = prev
        pb = AovBuffers(None, *[int(paov[k]) for k in ("normal", "position", "depth")])
        pc, pcol, pmom = C.byref(pcam), C.c_void_p(int(pcol)), C.c_void_p(int(pmom))
    sec = C.c_double()
    o = _temporal_opts(opts)
    _check(lib().mcpt_temporal_accumulate_device(
        C.byref(o), pc, int(width), int(height), C.c_void_p(int(color_ptr)), C.byref(b), None if pb is None else C.byref(pb),
        pcol, pmom, C.c_void_p(int(out_color_ptr)), C.c_void_p(int(out_moments_ptr)),
        None if out_variance_ptr is None else C.c_void_p(int(out_variance_ptr)), C.byref(sec)))
    return sec.value


CLAMP_OPTS = ("radius", "alpha_fast", "sigma")


def _clamp_opts(clamp):
    """clamp: None or True (the library defaults) or a dict of radius / alpha_fast / sigma"""
    c = TemporalClampOpts()
    lib().mcpt_temporal_clamp_opts_init(C.byref(c))
    for k, v in ({} if clamp is None or clamp is True else dict(clamp)).items():
        if k not in CLAMP_OPTS:
            raise TypeError("unknown clamp option %r (one of %s)" % (k, ", ".join(CLAMP_OPTS)))
        if v is not None:
            setattr(c, k, type(getattr(c, k))(v))
    return c


def temporal_accumulate_clamped(color, aovs, prev=None, clamp=None, **opts):
    """temporal_accumulate with history clamping (mcpt_temporal_accumulate_clamped; include/mcpt.h states the rule).
    prev is None or (camera, aovs, colour, moments, fast): the previous frame's Camera and guides and the colour,
    moments and fast history this function returned for it.  clamp: None or True for the library defaults, or a dict
    of radius, alpha_fast, sigma.  opts as temporal_accumulate.  Returns (colour H x W x 3, moments H x W x 4, fast
    history H x W x 3, variance H x W, shift H x W -- how far the clamp moved each pixel's luminance, 0 where it did
    not -- and the device seconds)."""
    color = _d(color)
    H, W = color.shape[:2]
    assert color.shape == (H, W, 3)
    keys = ("albedo", "normal", "position", "depth")
    g = {k: _d(aovs[k], (H, W) if k == "depth" else (H, W, 3)) for k in keys}
    b = AovBuffers(*[g[k].ctypes.data for k in keys])
    pc = pb = pcol = pmom = pfast = None
    if prev is not None:
        pcam, paov, pcol, pmom, pfast = prev
        pg = {k: _d(paov[k], (H, W) if k == "depth" else (H, W, 3)) for k in keys[1:]}
        pb = AovBuffers(None, *[pg[k].ctypes.data for k in keys[1:]])
        pcol, pmom, pfast = _d(pcol, (H, W, 3)), _d(pmom, (H, W, 4)), _d(pfast, (H, W, 3))
        pc = C.byref(pcam)
    out, mom, fast, var, shift = np.zeros((H, W, 3)), np.zeros((H, W, 4)), np.zeros((H, W, 3)), np.zeros((H, W)), np.zeros((H, W))
    sec = C.c_double()
    o, c = _temporal_opts(opts), _clamp_opts(clamp)
    ptr = lambda a: None if a is None else a.ctypes.data
    _check(lib().mcpt_temporal_accumulate_clamped(
        C.byref(o), C.byref(c), pc, W, H, color.ctypes.data, C.byref(b), None if pb is None else C.byref(pb), ptr(pcol),
        ptr(pmom), ptr(pfast), out.ctypes.data, mom.ctypes.data, fast.ctypes.data, var.ctypes.data, shift.ctypes.data,
        C.byref(sec)))
    return out, mom, fast, var, shift, sec.value


def temporal_accumulate_clamped_device(width, height, color_ptr, aov_ptrs, out_color_ptr, out_moments_ptr, out_fast_ptr,
                                       out_variance_ptr=None, out_shift_ptr=None, prev=None, clamp=None, **opts):
    """temporal_accumulate_clamped over device buffers, as temporal_accumulate_device: prev is None or (camera, dict of
    the previous normal / position / depth pointers, previous colour, moments and fast-history pointers);
    out_variance_ptr and out_shift_ptr may be None.  Returns the device seconds."""
    b = AovBuffers(*[int(aov_ptrs[k]) for k in ("albedo", "normal", "position", "depth")])
    pc = pb = pcol = pmom = pfast = None
    if prev is not None:
        pcam, paov, pcol, pmom, pfast = prev
        pb = AovBuffers(None, *[int(paov[k]) for k in ("normal", "position", "depth")])
        pc, pcol, pmom, pfast = C.byref(pcam), C.c_void_p(int(pcol)), C.c_void_p(int(pmom)), C.c_void_p(int(pfast))
    sec = C.c_double()
    o, c = _temporal_opts(opts), _clamp_opts(clamp)
    opt = lambda p: None if p is None else C.c_void_p(int(p))
    _check(lib().mcpt_temporal_accumulate_clamped_device(
        C.byref(o), C.byref(c), pc, int(width), int(height), C.c_void_p(int(color_ptr)), C.byref(b),
        None if pb is None else C.byref(pb), pcol, pmom, pfast, C.c_void_p(int(out_color_ptr)),
        C.c_void_p(int(out_moments_ptr)), C.c_void_p(int(out_fast_ptr)), opt(out_variance_ptr), opt(out_shift_ptr),
        C.byref(sec)))
    return sec.value


def temporal_accumulate_motion(color, aovs, motion, prev=None, clamp=None, **opts):
    """Temporal accumulation with object motion (mcpt_temporal_accumulate_motion; include/mcpt.h states the rule): as
    temporal_accumulate (clamp=None) or temporal_accumulate_clamped (clamp=True or a dict), with the reprojected point and
    the normal of the taps' tests taken from `motion`, the dict of render_motion_aovs (prev_position, prev_normal).
    prev and the return value are those of the form chosen: (colour, moments, variance, seconds) without clamp,
    (colour, moments, fast, variance, shift, seconds) with it."""
    color = _d(color)
    H, W = color.shape[:2]
    assert color.shape == (H, W, 3)
    keys = ("albedo", "normal", "position", "depth")
    g = {k: _d(aovs[k], (H, W) if k == "depth" else (H, W, 3)) for k in keys}
    b = AovBuffers(*[g[k].ctypes.data for k in keys])
    mo = {k: _d(motion[k], (H, W, 3)) for k in ("prev_position", "prev_normal")}
    mb = MotionBuffers(mo["prev_position"].ctypes.data, mo["prev_normal"].ctypes.data)
    pc = pb = pcol = pmom = pfast = None
    if prev is not None:
        pcam, paov, pcol, pmom = prev[:4]
        pg = {k: _d(paov[k], (H, W) if k == "depth" else (H, W, 3)) for k in keys[1:]}
        pb = AovBuffers(None, *[pg[k].ctypes.data for k in keys[1:]])
        pcol, pmom = _d(pcol, (H, W, 3)), _d(pmom, (H, W, 4))
        if clamp is not None:
            pfast = _d(prev[4], (H, W, 3))
        pc = C.byref(pcam)
    out, mom, var, sec = np.zeros((H, W, 3)), np.zeros((H, W, 4)), np.zeros((H, W)), C.c_double()
    fast, shift = (np.zeros((H, W, 3)), np.zeros((H, W))) if clamp is not None else (None, None)
    o = _temporal_opts(opts)
    c = _clamp_opts(clamp) if clamp is not None else None
    ptr = lambda a: None if a is None else a.ctypes.data
    _check(lib().mcpt_temporal_accumulate_motion(
        C.byref(o), None if c is None else C.byref(c), pc, W, H, color.ctypes.data, C.byref(b), C.byref(mb),
        None if pb is None else C.byref(pb), ptr(pcol), ptr(pmom), ptr(pfast), out.ctypes.data, mom.ctypes.data, ptr(fast),
        ptr(shift), var.ctypes.data, C.byref(sec)))
    if clamp is None:
        return out, mom, var, sec.value
    return out, mom, fast, var, shift, sec.value


def temporal_accumulate_motion_device(width, height, color_ptr, aov_ptrs, motion_ptrs, out_color_ptr, out_moments_ptr,
                                      out_fast_ptr=None, out_variance_ptr=None, out_shift_ptr=None, prev=None, clamp=None,
                                      **opts):
    """temporal_accumulate_motion over device buffers: motion_ptrs is a dict of the prev_position and prev_normal
    pointers; prev is None or (camera, dict of the previous normal / position / depth pointers, previous colour and
    moments pointers[, previous fast-history pointer with clamp]); out_fast_ptr is required with clamp and, like
    out_shift_ptr, must be None without.  Returns the device seconds."""
    b = AovBuffers(*[int(aov_ptrs[k]) for k in ("albedo", "normal", "position", "depth")])
    mb = MotionBuffers(int(motion_ptrs["prev_position"]), int(motion_ptrs["prev_normal"]))
    opt = lambda p: None if p is None else C.c_void_p(int(p))
    pc = pb = pcol = pmom = pfast = None
    if prev is not None:
        pcam, paov, pcol, pmom = prev[:4]
        pb = AovBuffers(None, *[int(paov[k]) for k in ("normal", "position", "depth")])
        pc, pcol, pmom = C.byref(pcam), opt(pcol), opt(pmom)
        if clamp is not None:
            pfast = opt(prev[4])
    sec = C.c_double()
    o = _temporal_opts(opts)
    c = _clamp_opts(clamp) if clamp is not None else None
    _check(lib().mcpt_temporal_accumulate_motion_device(
        C.byref(o), None if c is None else C.byref(c), pc, int(width), int(height), opt(color_ptr), C.byref(b), C.byref(mb),
        None if pb is None else C.byref(pb), pcol, pmom, pfast, opt(out_color_ptr), opt(out_moments_ptr), opt(out_fast_ptr),
        opt(out_shift_ptr), opt(out_variance_ptr), C.byref(sec)))
    return sec.value


GRADIENT_OPTS = ("stratum", "radius", "scale", "device")


def _gradient_opts(stratum=None, radius=None, scale=None, device=None):
    g = GradientOpts()
    lib().mcpt_gradient_opts_init(C.byref(g))
    for k, v in (("stratum", stratum), ("radius", radius), ("scale", scale), ("device", device)):
        if v is not None:
            setattr(g, k, type(getattr(g, k))(v))
    return g


def gradient_phase(stratum, frame_index):
    """mcpt_gradient_phase: the phase (a, b) of frame `frame_index` at `stratum` (1..8), upsample_phase's rule:
    k = frame_index mod stratum^2, a = k mod stratum, b = (a + k div stratum) mod stratum."""
    a, b = C.c_int32(), C.c_int32()
    _check(lib().mcpt_gradient_phase(int(stratum), int(frame_index), C.byref(a), C.byref(b)))
    return a.value, b.value


def gradient_rays(camera, stratum, a, b, device=None):
    """mcpt_gradient_rays: (origin, dir), H*W x 3 each in pixel order: camera_rays(camera)'s rays at the pixels (i, j)
    with i mod stratum == a and j mod stratum == b bit for bit, a zero direction (a miss for render_rays) everywhere else
    -- what an anti-lag gradient pass traces, with the previous frame's camera and seed."""
    n = max(camera.width * camera.height, 1)
    origin, dir = np.zeros((n, 3)), np.zeros((n, 3))
    _check(lib().mcpt_gradient_rays(C.byref(camera), int(stratum), int(a), int(b), -1 if device is None else int(device),
                                    origin.ctypes.data, dir.ctypes.data))
    return origin, dir


def gradient_index(width, height, stratum, a, b):
    """mcpt_gradient_index: the pixels (i, j) of a width x height frame with i mod stratum == a and j mod stratum == b as
    an increasing int32 list of pixel ids i * width + j (possibly empty).  No device work."""
    n = C.c_int32()
    _check(lib().mcpt_gradient_index(int(width), int(height), int(stratum), int(a), int(b), C.byref(n), None))
    index = np.zeros(max(n.value, 1), dtype=np.int32)
    _check(lib().mcpt_gradient_index(int(width), int(height), int(stratum), int(a), int(b), C.byref(n), index.ctypes.data))
    return index[:n.value]


def gradient_rays_indexed(camera, stratum, a, b, device=None):
    """mcpt_gradient_rays_indexed: (index, origin, dir) of the selected pixels alone -- gradient_index's ids and
    gradient_rays' rays at them bit for bit, count and count x 3 -- what render_rays_indexed takes."""
    n = len(gradient_index(camera.width, camera.height, stratum, a, b))
    index, origin, dir = np.zeros(max(n, 1), dtype=np.int32), np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 3))
    _check(lib().mcpt_gradient_rays_indexed(C.byref(camera), int(stratum), int(a), int(b), -1 if device is None else int(device),
                                            index.ctypes.data, origin.ctypes.data, dir.ctypes.data))
    return index[:n], origin[:n], dir[:n]


def temporal_gradient(prev_raw, regrad, a, b, stratum=3, radius=1, scale=1.0, device=None):
    """mcpt_temporal_gradient (include/mcpt.h states the rule): prev_raw H x W x 3 is the previous frame's raw render,
    regrad H x W x 3 the radiance along gradient_rays of the previous camera with the previous seed in the current scene
    (0 off the selected pixels).  Returns (Lambda, ceil(H / stratum) x ceil(W / stratum), in [0, 1]; the device seconds)."""
    prev_raw, regrad = _d(prev_raw), _d(regrad)
    H, W = prev_raw.shape[:2]
    assert prev_raw.shape == (H, W, 3) and regrad.shape == (H, W, 3)
    g = _gradient_opts(stratum, radius, scale, device)
    s = max(int(g.stratum), 1)
    lam, sec = np.zeros(((H + s - 1) // s, (W + s - 1) // s)), C.c_double()
    _check(lib().mcpt_temporal_gradient(C.byref(g), W, H, int(a), int(b), prev_raw.ctypes.data, regrad.ctypes.data,
                                        lam.ctypes.data, C.byref(sec)))
    return lam, sec.value


def temporal_accumulate_antilag(color, aovs, lam, prev=None, motion=None, clamp=None, stratum=3, **opts):
    """Temporal accumulation with anti-lag (mcpt_temporal_accumulate_antilag; include/mcpt.h states the rule): as
    temporal_accumulate (clamp=None) or temporal_accumulate_clamped, with motion (the dict of render_motion_aovs) as
    temporal_accumulate_motion, and the blend weights raised by `lam`, the map temporal_gradient returned at `stratum`.
    prev and the return value are those of the form chosen.  With lam == 0 the outputs are that form's bit for bit."""
    color = _d(color)
    H, W = color.shape[:2]
    assert color.shape == (H, W, 3)
    keys = ("albedo", "normal", "position", "depth")
    g = {k: _d(aovs[k], (H, W) if k == "depth" else (H, W, 3)) for k in keys}
    b = AovBuffers(*[g[k].ctypes.data for k in keys])
    mb = None
    if motion is not None:
        mo = {k: _d(motion[k], (H, W, 3)) for k in ("prev_position", "prev_normal")}
        mb = MotionBuffers(mo["prev_position"].ctypes.data, mo["prev_normal"].ctypes.data)
    go = _gradient_opts(stratum)
    s = max(int(go.stratum), 1)
    lam = _d(lam, ((H + s - 1) // s, (W + s - 1) // s))
    pc = pb = pcol = pmom = pfast = None
    if prev is not None:
        pcam, paov, pcol, pmom = prev[:4]
        pg = {k: _d(paov[k], (H, W) if k == "depth" else (H, W, 3)) for k in keys[1:]}
        pb = AovBuffers(None, *[pg[k].ctypes.data for k in keys[1:]])
        pcol, pmom = _d(pcol, (H, W, 3)), _d(pmom, (H, W, 4))
        if clamp is not None:
            pfast = _d(prev[4], (H, W, 3))
        pc = C.byref(pcam)
    out, mom, var, sec = np.zeros((H, W, 3)), np.zeros((H, W, 4)), np.zeros((H, W)), C.c_double()
    fast, shift = (np.zeros((H, W, 3)), np.zeros((H, W))) if clamp is not None else (None, None)
    o = _temporal_opts(opts)
    c = _clamp_opts(clamp) if clamp is not None else None
    ptr = lambda a: None if a is None else a.ctypes.data
    _check(lib().mcpt_temporal_accumulate_antilag(
        C.byref(o), None if c is None else C.byref(c), pc, W, H, color.ctypes.data, C.byref(b), None if mb is None else C.byref(mb),
        None if pb is None else C.byref(pb), ptr(pcol), ptr(pmom), ptr(pfast), out.ctypes.data, mom.ctypes.data, ptr(fast),
        ptr(shift), var.ctypes.data, C.byref(sec), C.byref(go), lam.ctypes.data))
    if clamp is None:
        return out, mom, var, sec.value
    return out, mom, fast, var, shift, sec.value


def temporal_accumulate_antilag_device(width, height, color_ptr, aov_ptrs, lambda_ptr, out_color_ptr, out_moments_ptr,
                                       out_fast_ptr=None, out_variance_ptr=None, out_shift_ptr=None, prev=None, motion_ptrs=None,
                                       clamp=None, stratum=3, **opts):
    """temporal_accumulate_antilag over device buffers, as temporal_accumulate_motion_device: lambda_ptr the device
    pointer of the Lambda map at `stratum`; motion_ptrs None or a dict of the prev_position and prev_normal pointers.
    Returns the device seconds."""
    b = AovBuffers(*[int(aov_ptrs[k]) for k in ("albedo", "normal", "position", "depth")])
    mb = None if motion_ptrs is None else MotionBuffers(int(motion_ptrs["prev_position"]), int(motion_ptrs["prev_normal"]))
    opt = lambda p: None if p is None else C.c_void_p(int(p))
    pc = pb = pcol = pmom = pfast = None
    if prev is not None:
        pcam, paov, pcol, pmom = prev[:4]
        pb = AovBuffers(None, *[int(paov[k]) for k in ("normal", "position", "depth")])
        pc, pcol, pmom = C.byref(pcam), opt(pcol), opt(pmom)
        if clamp is not None:
            pfast = opt(prev[4])
    sec = C.c_double()
    o, go = _temporal_opts(opts), _gradient_opts(stratum)
    c = _clamp_opts(clamp) if clamp is not None else None
    _check(lib().mcpt_temporal_accumulate_antilag_device(
        C.byref(o), None if c is None else C.byref(c), pc, int(width), int(height), opt(color_ptr), C.byref(b),
        None if mb is None else C.byref(mb), None if pb is None else C.byref(pb), pcol, pmom, pfast, opt(out_color_ptr),
        opt(out_moments_ptr), opt(out_fast_ptr), opt(out_shift_ptr), opt(out_variance_ptr), C.byref(sec), C.byref(go),
        opt(lambda_ptr)))
    return sec.value


class TemporalAccumulator:
    """The history of a frame sequence over a static scene: push(camera, color, aovs) accumulates one frame onto
    what the earlier pushes left and returns (accumulated colour, variance of its luminance); the unfiltered
    accumulated colour is the history (denoise the returned frame, not the history).  opts as temporal_accumulate.
    After a push: `moments` (H x W x 4), `seconds` (device time) and `kept` (share of pixels that kept a history).
    clamp: None (the default: plain accumulation), True or a dict of radius / alpha_fast / sigma for history clamping
    (temporal_accumulate_clamped); then a push also leaves `fast` (the fast history), `shift` and `clamped`, the share
    of pixels with shift != 0.  push(..., motion=render_motion_aovs(scene, camera)) follows geometry moved by
    Scene.update since the last Scene.pose_save (temporal_accumulate_motion).  push(..., lam=Lambda, stratum=s) raises
    the blend weights by the temporal gradient's map (temporal_accumulate_antilag), with or without motion and clamp."""

    def __init__(self, clamp=None, **opts):
        if clamp is False:
            clamp = None
        self.clamp, self.opts = clamp, opts
        self.reset()

    def reset(self):
        self.state, self.moments, self.seconds, self.kept = None, None, 0.0, 0.0
        self.fast, self.shift, self.clamped = None, None, 0.0

    def push(self, camera, color, aovs, motion=None, lam=None, stratum=3):
        cam = Camera.from_buffer_copy(camera)
        keep = {k: np.array(aovs[k], dtype=np.float64) for k in ("albedo", "normal", "position", "depth")}
        if lam is not None:
            r = temporal_accumulate_antilag(color, keep, lam, self.state, motion, self.clamp, stratum, **self.opts)
            if self.clamp is None:
                out, mom, var, self.seconds = r
                self.state = (cam, keep, out, mom)
            else:
                out, mom, self.fast, var, self.shift, self.seconds = r
                self.state = (cam, keep, out, mom, self.fast)
                self.clamped = float((self.shift != 0).mean())
        elif self.clamp is None:
            if motion is None:
                out, mom, var, self.seconds = temporal_accumulate(color, keep, self.state, **self.opts)
            else:
                out, mom, var, self.seconds = temporal_accumulate_motion(color, keep, motion, self.state, **self.opts)
            self.state = (cam, keep, out, mom)
        else:
            if motion is None:
                out, mom, self.fast, var, self.shift, self.seconds = temporal_accumulate_clamped(color, keep, self.state, self.clamp,
                                                                                                 **self.opts)
            else:
                out, mom, self.fast, var, self.shift, self.seconds = temporal_accumulate_motion(color, keep, motion, self.state,
                                                                                                self.clamp, **self.opts)
            self.state = (cam, keep, out, mom, self.fast)
            self.clamped = float((self.shift != 0).mean())
        self.moments = mom
        self.kept = float((mom[..., 2] > 1.5).mean())
        return out, var


DENOISE_OPTS = ("iterations", "sigma_color", "sigma_normal", "sigma_plane", "sigma_albedo")


class FrameSequence:
    """A frame sequence resident on one device (mcpt_sequence; include/mcpt.h states the contract): every frame is
    rendered, accumulated onto the reprojected history, filtered (denoise=True) and tone-mapped on buffers allocated
    once here, and only the 8-bit frame and a few statistics come back.  The same kernels as render / render_aovs /
    TemporalAccumulator / denoise ran on the same inputs, so read() returns what that host pipeline computes.
    clamp: None or False (plain accumulation), True or a dict of radius / alpha_fast / sigma (history clamping).
    denoise: False, True (the filter's defaults) or a dict of iterations / sigma_color / sigma_normal / sigma_plane /
    sigma_albedo.  temporal_opts: the fields of TemporalOpts, as for temporal_accumulate (device excepted).
    upsample: None (the default), a factor F in 2..4 or a dict of factor / sigma_normal / sigma_plane / sigma_albedo /
    min_weight: width x height stays the render's size, the shown frame (frame()'s return, read("upsampled"),
    device_buffer("rgb8")) is F times that along each axis, reconstructed by upsample()'s rule from the shown low frame
    and the guides of camera_scaled(camera, F); upsample_info() then gives the new stages' times.
    temporal_upsample=True (with upsample=F; no clamp, jitter or grid): every frame traces width x height rays through a
    different 1 / F^2 subset of the full-size pixels (upsample_phase) and accumulates them in a full-size history
    (temporal_upsample()'s rule): read("raw") is H x W x 3, accumulated / moments / variance / filtered are full size,
    "upsampled", "fast" and "shift" are refused, and temporal_upsample_info() gives the phase and the fill's shares.
    motion=True (not with upsample): every frame also runs the motion AOVs and accumulates by
    temporal_accumulate_motion's rule, following geometry moved by Scene.update since the caller's last Scene.pose_save
    (the sequence never saves the pose); read("prev_position") / read("prev_normal") and motion_info() then work, and
    set_motion() switches it from the next frame on.
    antilag=True or a dict of stratum / radius / scale (not with upsample, jitter or grid): every frame keeps its raw
    frame and seed, the next one traces a 1 / stratum^2 subset of those samples again in the scene as it then is
    (gradient_rays, render_rays with the kept seed), turns the difference into Lambda (temporal_gradient) and accumulates
    by temporal_accumulate_antilag's rule, so that history made stale by an edit of the scene is dropped at once;
    read("gradient_lambda") / read("gradient_raw") and antilag_info() then work, and set_antilag() switches it from the
    next frame on.
    After a frame: `info` (SequenceInfo: stage device times, kept, mean_history, clamped) and `stats` (the render's)."""

    def __init__(self, scene, width, height, spp, mode="mis", denoise=True, clamp=None, device=None, accel="bvh", flags=0,
                 tone_max=None, tone_gamma=None, upsample=None, temporal_upsample=False, motion=False, antilag=None,
                 **temporal_opts):
        self.h = None
        self._destroy = lib().mcpt_sequence_destroy
        if clamp is False:
            clamp = None
        base = _adaptive_base(mode, DEFAULT_SEED, device, 0, 0, None, accel, flags)
        o = SequenceOpts()
        lib().mcpt_sequence_opts_init(C.byref(o))
        o.width, o.height, o.spp = int(width), int(height), int(spp)
        o.denoise, o.clamp = int(bool(denoise)), int(clamp is not None)
        if tone_max is not None:
            o.tone_max = float(tone_max)
        if tone_gamma is not None:
            o.tone_gamma = float(tone_gamma)
        tp = _temporal_opts(temporal_opts)
        tc = _clamp_opts(clamp) if clamp is not None else None
        dn = None
        if denoise:
            d = denoise if isinstance(denoise, dict) else {}
            unknown = set(d) - set(DENOISE_OPTS)
            if unknown:
                raise TypeError("unknown denoise option %r (one of %s)" % (sorted(unknown)[0], ", ".join(DENOISE_OPTS)))
            dn = _denoise_opts(*[d.get(k) for k in DENOISE_OPTS], device)
        h = C.c_void_p()
        self.factor, self.temporal_upsample = 1, bool(temporal_upsample)
        if temporal_upsample and (upsample is None or upsample is False):
            raise ValueError("temporal_upsample=True needs upsample=F (the factor)")
        if upsample is None or upsample is False:
            _check(lib().mcpt_sequence_create(scene.h, C.byref(base), C.byref(o), C.byref(tp), None if tc is None else C.byref(tc),
                                              None if dn is None else C.byref(dn), C.byref(h)))
        else:
            u = dict(upsample) if isinstance(upsample, dict) else {"factor": upsample}
            unknown = set(u) - set(UPSAMPLE_OPTS)
            if unknown:
                raise TypeError("unknown upsample option %r (one of %s)" % (sorted(unknown)[0], ", ".join(UPSAMPLE_OPTS)))
            up = _upsample_opts(*[u.get(k) for k in UPSAMPLE_OPTS], device)
            if temporal_upsample:
                _check(lib().mcpt_sequence_create_temporal_upsampled(scene.h, C.byref(base), C.byref(o), C.byref(tp),
                                                                     None if dn is None else C.byref(dn), C.byref(up), C.byref(h)))
            else:
                _check(lib().mcpt_sequence_create_upsampled(scene.h, C.byref(base), C.byref(o), C.byref(tp),
                                                            None if tc is None else C.byref(tc),
                                                            None if dn is None else C.byref(dn), C.byref(up), C.byref(h)))
            self.factor = up.factor
        self.h, self.scene = h, scene  # the scene must outlive the handle
        self.width, self.height, self.spp, self.denoise, self.clamp = o.width, o.height, o.spp, bool(denoise), clamp
        self.info, self.stats = None, None
        self.motion = False
        self.antilag = None
        if motion:
            self.set_motion(True)
        if antilag is not None and antilag is not False:
            self.set_antilag(antilag)

    def set_antilag(self, antilag):
        """mcpt_sequence_set_antilag: from the next frame on, run the gradient pass and accumulate by the anti-lag rule
        (True for the defaults, or a dict of stratum / radius / scale), or not (None or False); refused by an upsampled
        sequence and with jitter or the grid."""
        if antilag is None or antilag is False:
            _check(lib().mcpt_sequence_set_antilag(self.h, None))
            self.antilag = None
            return
        d = {} if antilag is True else dict(antilag)
        unknown = set(d) - set(GRADIENT_OPTS[:3])
        if unknown:
            raise TypeError("unknown antilag option %r (one of %s)" % (sorted(unknown)[0], ", ".join(GRADIENT_OPTS[:3])))
        g = _gradient_opts(d.get("stratum"), d.get("radius"), d.get("scale"))
        _check(lib().mcpt_sequence_set_antilag(self.h, C.byref(g)))
        self.antilag = g

    def antilag_info(self):
        """mcpt_sequence_antilag_info of the last frame: dict of ran (the gradient pass ran), phase (a, b), trace_seconds
        (the gradient render), kernel_seconds (the ray, gradient and reduction kernels), lambda_mean and lambda_max;
        antilag only."""
        r, a, b = C.c_int32(), C.c_int32(), C.c_int32()
        t, k, m, x = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        _check(lib().mcpt_sequence_antilag_info(self.h, C.byref(r), C.byref(a), C.byref(b), C.byref(t), C.byref(k), C.byref(m),
                                                C.byref(x)))
        return dict(ran=bool(r.value), phase=(a.value, b.value), trace_seconds=t.value, kernel_seconds=k.value,
                    lambda_mean=m.value, lambda_max=x.value)

    def set_motion(self, on):
        """mcpt_sequence_set_motion: from the next frame on, accumulate with (True) or without (False) object motion;
        refused by an upsampled sequence."""
        _check(lib().mcpt_sequence_set_motion(self.h, int(bool(on))))
        self.motion = bool(on)

    def motion_info(self):
        """mcpt_sequence_motion_info of the last frame: the device seconds of the motion AOVs; motion=True only."""
        s = C.c_double()
        _check(lib().mcpt_sequence_motion_info(self.h, C.byref(s)))
        return s.value

    def frame(self, camera, seed=DEFAULT_SEED, readback=True):
        """One frame with `camera` (of the sequence's size) and `seed`; returns the tone-mapped H x W x 3 uint8 frame
        (with upsample=F: F H x F W x 3), or None with readback=False (the frame then stays on the device:
        device_buffer("rgb8"))."""
        out = np.zeros((self.factor * self.height, self.factor * self.width, 3), np.uint8) if readback else None
        info, st = SequenceInfo(), Stats()
        _check(lib().mcpt_sequence_frame(self.h, C.byref(camera), int(seed), None if out is None else out.ctypes.data,
                                         C.byref(info), C.byref(st)))
        self.info, self.stats = info, st
        self._lambda_stratum = int(self.antilag.stratum) if self.antilag is not None else 0  # what gradient_lambda is sized by
        return out

    def read(self, name):
        """The last frame's buffer `name` as a float64 array: raw, accumulated, filtered, fast (H x W x 3), moments
        (H x W x 4), variance, shift (H x W); with upsample=F also upsampled (F H x F W x 3); with motion=True also
        prev_position and prev_normal (H x W x 3); with antilag also gradient_lambda (ceil(H / s) x ceil(W / s)) and,
        when the gradient pass ran, gradient_raw (H x W x 3)."""
        what, tail = SEQ_BUFFERS.get(name, SEQ_MOTION_BUFFERS.get(name, SEQ_ANTILAG_BUFFERS.get(name, (-1, ()))))
        f = self.factor if name == "upsampled" or (self.temporal_upsample and name != "raw") else 1
        out = np.zeros((f * self.height, f * self.width) + tail)
        if name == "gradient_lambda":  # at the stratum the last frame ran with, whatever set_antilag set since
            s = max(getattr(self, "_lambda_stratum", 0), 1)
            out = np.zeros(((self.height + s - 1) // s, (self.width + s - 1) // s))
        _check(lib().mcpt_sequence_read(self.h, what, out.ctypes.data))
        return out

    def device_buffer(self, name):
        """The device pointer (int) of the last frame's buffer `name` (read()'s names and rgb8), valid until the next
        frame, reset or close."""
        p = C.c_void_p()
        what = SEQ_BUFFERS.get(name, SEQ_MOTION_BUFFERS.get(name, SEQ_ANTILAG_BUFFERS.get(name, (-1, ()))))[0]
        _check(lib().mcpt_sequence_device_buffer(self.h, what, C.byref(p)))
        return p.value

    def upsample_info(self):
        """mcpt_sequence_upsample_info of the last frame: dict of guide_seconds (the full-size AOVs), upsample_seconds
        (the upsampling kernel) and fallback_share (fallback pixels / full-size pixels); upsample=F only."""
        g, u, s = C.c_double(), C.c_double(), C.c_double()
        _check(lib().mcpt_sequence_upsample_info(self.h, C.byref(g), C.byref(u), C.byref(s)))
        return dict(guide_seconds=g.value, upsample_seconds=u.value, fallback_share=s.value)

    def temporal_upsample_info(self):
        """mcpt_sequence_temporal_upsample_info of the last frame: dict of phase (a, b), rays_seconds (the phase-ray
        kernel), filled_share and fallback_share (fill and fallback pixels / full-size pixels); temporal_upsample=True
        only."""
        a, b, r, s, t = C.c_int32(), C.c_int32(), C.c_double(), C.c_double(), C.c_double()
        _check(lib().mcpt_sequence_temporal_upsample_info(self.h, C.byref(a), C.byref(b), C.byref(r), C.byref(s), C.byref(t)))
        return dict(phase=(a.value, b.value), rays_seconds=r.value, filled_share=s.value, fallback_share=t.value)

    def reset(self):
        """The next frame starts every history."""
        _check(lib().mcpt_sequence_reset(self.h))

    def close(self):
        if getattr(self, "h", None):
            self._destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()


def tone_map_device(ptr, width, height, out_ptr, max_radiance=380.0, gamma=0.25, device=None):
    """mcpt_tone_map_device: tone_map over device memory -- ptr H*W*3 float64, out_ptr H*W*3 uint8 (e.g. torch CUDA
    tensors' data_ptr()).  A value whose 255 r + 0.5 is within 1e-9 relative of an integer may differ from tone_map by
    one level (the device's pow is not the host's)."""
    _check(lib().mcpt_tone_map_device(None if ptr is None else C.c_void_p(int(ptr)), int(width), int(height),
                                      float(max_radiance), float(gamma), None if out_ptr is None else C.c_void_p(int(out_ptr)),
                                      -1 if device is None else int(device)))


def frame_stats_device(moments_ptr, width, height, shift_ptr=None, device=None):
    """mcpt_frame_stats_device over device memory: moments_ptr H*W*4 float64, shift_ptr H*W float64 or None.  Returns
    (pixels with n > 1.5, sum of n over the pixels with n > 0, pixels with shift != 0), reduced in a fixed order."""
    kept, moved, nsum = C.c_uint64(), C.c_uint64(), C.c_double()
    _check(lib().mcpt_frame_stats_device(None if moments_ptr is None else C.c_void_p(int(moments_ptr)),
                                         None if shift_ptr is None else C.c_void_p(int(shift_ptr)), int(width), int(height),
                                         -1 if device is None else int(device), C.byref(kept), C.byref(nsum), C.byref(moved)))
    return kept.value, nsum.value, moved.value


def debug_adaptive_active(scene, device=-1):
    """Diagnostics: the last active-pixel list the scene's most recent adaptive render built
    (include/mcpt_debug.h), as an int32 array of pixel indices."""
    n = C.c_int32()
    _check(lib().mcpt_debug_adaptive_active(scene.h, int(device), np.zeros(1, np.int32), 0, C.byref(n)))
    px = np.zeros(max(n.value, 1), np.int32)
    _check(lib().mcpt_debug_adaptive_active(scene.h, int(device), px, n.value, C.byref(n)))
    return px[:n.value]


def debug_set_pick_table(min_samples=0, window_samples=0):
    """mcpt_debug_set_pick_table (include/mcpt_debug.h): process-wide overrides of the root pick table's rules,
    0 = the library's default."""
    _check(lib().mcpt_debug_set_pick_table(int(min_samples), int(window_samples)))


def debug_device_bytes_live():
    """mcpt_debug_device_bytes_live (include/mcpt_debug.h): the bytes of device memory the library's buffers hold now,
    over all scenes and devices; back to its earlier value once the scenes made since are destroyed."""
    return int(lib().mcpt_debug_device_bytes_live())


def debug_set_rebuild_leaf_max(leaf_max=0):
    """mcpt_debug_set_rebuild_leaf_max (include/mcpt_debug.h): the most facets of a leaf child of Scene.rebuild's trees,
    1..4, process-wide; 0 = the library's default."""
    _check(lib().mcpt_debug_set_rebuild_leaf_max(int(leaf_max)))


def debug_root_picks(scene, camera, spp, sample_range, mode="mis", seed=DEFAULT_SEED, flags=0, device=None):
    """mcpt_debug_root_picks (include/mcpt_debug.h): (pick, weights_sum, ambiguous), each [pixels][samples of
    sample_range], of the roots a render with these options would queue; pick -2 marks a sample that terminates at
    entry or a pixel without a cached root."""
    o = _opts(spp, mode, seed, sample_range, device, 0, 0, flags=flags)
    n = (camera.width * camera.height, int(sample_range[1]) - int(sample_range[0]))
    pick, wsum, amb = np.zeros(n, np.int32), np.zeros(n), np.zeros(n, np.int32)
    _check(lib().mcpt_debug_root_picks(scene.h, C.byref(camera), C.byref(o), pick.reshape(-1), wsum.reshape(-1),
                                       amb.reshape(-1)))
    return pick, wsum, amb


def closest_hit(scene, ro, rd, exclude=None, light_only=False, grid=False, wide=False):
    """Myobj::closet_ray_intersect (Myobj.cpp:334) / ..._light_triangle (:476) for a batch of rays.
    grid=True traverses the reference's uniform grid of Scene.meshing (crack included), else the BVH;
    wide=True (diagnostics) the 8-wide compressed BVH of the persistent traversal (k_rays_cw8)."""
    ro, rd = _d(ro, (-1, 3)), _d(rd, (-1, 3))
    n = ro.shape[0]
    ex = np.full(n, -1, np.int32) if exclude is None else np.ascontiguousarray(exclude, np.int32)
    f, tbg = np.zeros(n, np.int32), np.zeros((n, 3))
    flags = (HIT_LIGHT_ONLY if light_only else 0) | (HIT_GRID if grid else 0) | (DEBUG_HIT_CW8 if wide else 0)
    _check(lib().mcpt_closest_hit(scene.h, n, ro, rd, ex, flags, f, tbg))
    return f, tbg


def light_prep(scene, x1, normal, u):
    """Mylight::prepared_for_lights_spherical_triangle_sampling at n points + the inverse-CDF pick."""
    x1, normal, u = _d(x1, (-1, 3)), _d(normal, (-1, 3)), _d(u, (-1,))
    n = x1.shape[0]
    ws, cnt, pick = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
    _check(lib().mcpt_light_prep(scene.h, n, x1, normal, u, ws, cnt, pick))
    return ws, cnt, pick


def debug_light_prep_exact(scene, x1, normal, u):
    """Diagnostics: light_prep with every point through the exact fallback alone (the reference's
    literal cull chain and weights, summed in index order; include/mcpt_debug.h)."""
    x1, normal, u = _d(x1, (-1, 3)), _d(normal, (-1, 3)), _d(u, (-1,))
    n = x1.shape[0]
    ws, cnt, pick = np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32)
    _check(lib().mcpt_debug_light_prep_exact(scene.h, n, x1, normal, u, ws, cnt, pick))
    return ws, cnt, pick


def debug_light_literal(scene, x1, normal):
    """Diagnostics: the literal cull chain's intermediates for every light at one point (N_L x 20)."""
    out = np.zeros((scene.nlights, 20))
    _check(lib().mcpt_debug_light_literal(scene.h, _d(x1, (3,)), _d(normal, (3,)), out.reshape(-1)))
    return out


def debug_bvh8_check(scene, light_only=False):
    """Diagnostics (host only): the 8-wide tree against its binary tree (include/mcpt_debug.h).  Returns dict
    nodes, tris, facets, duplicates, errors, depth."""
    out = np.zeros(6, np.int64)
    _check(lib().mcpt_debug_bvh8_check(scene.h, 1 if light_only else 0, out))
    return dict(zip(("nodes", "tris", "facets", "duplicates", "errors", "depth"), (int(v) for v in out)))


def debug_bvh4_check(scene, light_only=False):
    """Diagnostics (host only): the 4-wide tree every traversal reads and its quantized form against the
    binary tree (include/mcpt_debug.h).  Returns dict nodes, tris, facets, duplicates, errors, depth."""
    out = np.zeros(6, np.int64)
    _check(lib().mcpt_debug_bvh4_check(scene.h, 1 if light_only else 0, out))
    return dict(zip(("nodes", "tris", "facets", "duplicates", "errors", "depth"), (int(v) for v in out)))


def debug_bvh4_check_device(scene, device=-1):
    """Diagnostics: debug_bvh4_check's walk over what `device` holds of the main tree (nodes, quantized nodes, leaf
    slots), plus the device's vertices against the host positions (include/mcpt_debug.h).  Same dict."""
    out = np.zeros(6, np.int64)
    _check(lib().mcpt_debug_bvh4_check_device(scene.h, int(device), out))
    return dict(zip(("nodes", "tris", "facets", "duplicates", "errors", "depth"), (int(v) for v in out)))


def debug_bvh4_check_device_light(scene, device=-1):
    """Diagnostics: debug_bvh4_check_device's walk over the light-only tree `device` holds (include/mcpt_debug.h)."""
    out = np.zeros(6, np.int64)
    _check(lib().mcpt_debug_bvh4_check_device_light(scene.h, int(device), out))
    return dict(zip(("nodes", "tris", "facets", "duplicates", "errors", "depth"), (int(v) for v in out)))


LIGHT_TABLES = ("lt_v", "lt_n", "lt_pk", "lt_d", "lt_w", "lt_f", "lt_pair", "chunk_sph", "chunk_sk", "l_area", "l_area_cum",
                "globals")
# and what a re-light writes beside them (Scene.set_light_radiance, Scene.set_materials)
RELIGHT_TABLES = LIGHT_TABLES + ("light_rad", "light_sum", "grp_sum", "grp_cum", "mtl")


def debug_light_tables(scene, which=None, device=-1):
    """Diagnostics: one light table of the state `device` holds as raw bytes (np.uint8), or with which=None a dict of
    all of LIGHT_TABLES (include/mcpt_debug.h); a tuple of names (RELIGHT_TABLES) gives a dict of those.  "globals": band_ctr[3], band_R, band_S, band_K (float64), then
    light_bound (float32) and 4 zero bytes."""
    if which is None:
        return {w: debug_light_tables(scene, w, device) for w in LIGHT_TABLES}
    if isinstance(which, (tuple, list)):
        return {w: debug_light_tables(scene, w, device) for w in which}
    n = C.c_int64(0)
    _check(lib().mcpt_debug_light_tables(scene.h, int(device), which.encode(), None, 0, C.byref(n)))
    out = np.zeros(max(int(n.value), 1), np.uint8)
    _check(lib().mcpt_debug_light_tables(scene.h, int(device), which.encode(), out.ctypes.data_as(C.c_void_p), out.shape[0],
                                         C.byref(n)))
    return out[:int(n.value)]


def debug_light_area_cum_bench(scene, reps=20, device=-1):
    """Diagnostics: seconds of one run of the area-sum kernel over every group (include/mcpt_debug.h)."""
    s = C.c_double(0.0)
    _check(lib().mcpt_debug_light_area_cum_bench(scene.h, int(device), int(reps), C.byref(s)))
    return float(s.value)


def debug_bvh4_download(scene, device=-1):
    """Diagnostics: the device's main 4-wide tree as (nodes [BVH4_NODE], quantized nodes [BVH4_QNODE], facet of every
    leaf slot); leaf children read ~first slot with their count in "count" (include/mcpt_debug.h)."""
    counts = np.zeros(2, np.int64)
    _check(lib().mcpt_debug_bvh4_download(scene.h, int(device), counts, None, None, None, 0, 0))
    nodes, qn = np.zeros(int(counts[0]), BVH4_NODE), np.zeros(int(counts[0]), BVH4_QNODE)
    lf = np.zeros(max(int(counts[1]), 1), np.int32)
    _check(lib().mcpt_debug_bvh4_download(scene.h, int(device), counts, nodes.ctypes.data_as(C.c_void_p),
                                          qn.ctypes.data_as(C.c_void_p), lf.ctypes.data_as(C.c_void_p), nodes.shape[0],
                                          lf.shape[0]))
    return nodes, qn, lf[:int(counts[1])]


def debug_bvh4_host(scene, light_only=False):
    """Diagnostics (host only, no GPU): the 4-wide tree debug_bvh4_check walks and its quantised form, in
    debug_bvh4_download's layout: (nodes [BVH4_NODE], quantized nodes [BVH4_QNODE], facet of every leaf slot)."""
    counts = np.zeros(2, np.int64)
    lo = 1 if light_only else 0
    _check(lib().mcpt_debug_bvh4_host(scene.h, lo, counts, None, None, None, 0, 0))
    nodes, qn = np.zeros(int(counts[0]), BVH4_NODE), np.zeros(int(counts[0]), BVH4_QNODE)
    lf = np.zeros(max(int(counts[1]), 1), np.int32)
    _check(lib().mcpt_debug_bvh4_host(scene.h, lo, counts, nodes.ctypes.data_as(C.c_void_p), qn.ctypes.data_as(C.c_void_p),
                                      lf.ctypes.data_as(C.c_void_p), nodes.shape[0], lf.shape[0]))
    return nodes, qn, lf[:int(counts[1])]


def debug_tri_filter(tri, ro, rd, tlim=None):
    """Diagnostics (host only): the traversal's fp32 triangle pre-test on (triangle, ray) pairs.
    Returns (verdict, tup): 0 = the fp64 test surely rejects (or the hit is surely beyond tlim),
    2 = it surely accepts with t <= tup, 1 = undecided (include/mcpt_debug.h)."""
    tri = np.ascontiguousarray(tri, np.float32).reshape(-1, 9)
    n = tri.shape[0]
    ro, rd = _d(ro, (-1, 3)), _d(rd, (-1, 3))
    tl = np.full(n, np.finfo(np.float32).max, np.float32) if tlim is None else np.ascontiguousarray(tlim, np.float32)
    verdict, tup = np.zeros(n, np.int32), np.zeros(n, np.float32)
    _check(lib().mcpt_debug_tri_filter(n, tri, ro, rd, tl, verdict, tup))
    return verdict, tup


def debug_phong(records, variant):
    """Diagnostics: device_math.h's brdf_phong, phong_pdf and sample_phong on (n, 19) records -- n[3] wi[3] wr[3] kd[3]
    ks[3] sh u0 k1 k2 -- as the MIS / shade() kernels instantiate them (variant 0) or the BRDF-only kernels (variant 1).
    Returns an (n, 8) array: brdf[3] pdf dir[3] sample_pdf (include/mcpt_debug.h)."""
    rec = _d(records, (-1, 19))
    out = np.zeros((rec.shape[0], 8))
    _check(lib().mcpt_debug_phong(rec.shape[0], int(variant), rec.reshape(-1), out.reshape(-1)))
    return out


def debug_prep_bench(scene, x1, normal, u, variant=-1, iters=5):
    """Diagnostics: mean ms per launch of a light-prep kernel variant (see include/mcpt.h)."""
    x1, normal, u = _d(x1, (-1, 3)), _d(normal, (-1, 3)), _d(u, (-1,))
    n = x1.shape[0]
    ms, ws, pick = C.c_double(), np.zeros(n), np.zeros(n, np.int32)
    _check(lib().mcpt_debug_prep_bench(scene.h, n, x1, normal, u, int(variant), int(iters), C.byref(ms), ws, pick))
    return ms.value, ws, pick


def debug_prep_pick_counts():
    """Diagnostics: (nodes whose pick read the stashed batch weights, nodes that re-evaluated their picked batch) of the
    last debug_prep_bench call (include/mcpt_debug.h)."""
    a, b = C.c_int64(), C.c_int64()
    _check(lib().mcpt_debug_prep_pick_counts(C.byref(a), C.byref(b)))
    return a.value, b.value


def primary_hits(scene, camera):
    n = camera.width * camera.height
    f, tbg = np.zeros(n, np.int32), np.zeros((n, 3))
    _check(lib().mcpt_primary_hits(scene.h, C.byref(camera), f, tbg))
    return f, tbg


def tone_map(hdr, max_radiance=380.0, gamma=0.25):
    """RadianceRGB::tone_mapping(380, 0.25) of main.cpp:583 over a whole H x W x 3 frame."""
    hdr = np.ascontiguousarray(hdr, np.float64)
    H, W = hdr.shape[:2]
    out = np.zeros((H, W, 3), np.uint8)
    _check(lib().mcpt_tone_map(hdr.reshape(-1), W, H, max_radiance, gamma, out.reshape(-1)))
    return out


def write_bmp(path, rgb8):
    """The 32-bpp bottom-up BMP layout of the reference's test.bmp (main.cpp:596)."""
    rgb8 = np.ascontiguousarray(rgb8, np.uint8)
    H, W = rgb8.shape[:2]
    _check(lib().mcpt_write_bmp(os.fsencode(path), rgb8.reshape(-1), W, H))
