"""ctypes view of the C ABI (include/ptgpu.h, include/pthost.h).

The product is the C/HIP code under ``csrc/`` and ``host/``; this module only
mirrors the structs and loads the shared libraries so that tests, bench.py and
__graft_entry__ can call through the same C ABI a Rust host would bind
(INTEGRATION.md).  The directory name contains a hyphen, so it is imported as
``path_tracer_amd`` through ``__graft_entry__.load_package()``.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
ROOT = PKG_DIR.parent

PT_OK = 0
PT_ERR_INVALID, PT_ERR_IO, PT_ERR_PARSE, PT_ERR_DEVICE, PT_ERR_NUMERIC, PT_ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -6
PT_MODEL_MESH, PT_MODEL_SPHERE = 0, 1
PT_LIGHT_POINT, PT_LIGHT_DIRECTIONAL = 0, 1
PT_TONEMAP_REINHARD, PT_TONEMAP_FILMIC, PT_TONEMAP_ACES = 0, 1, 2
PT_FLAG_TIMING, PT_FLAG_COUNTERS, PT_FLAG_NO_GRIDS, PT_FLAG_MEGAKERNEL = 1, 2, 4, 8
TONEMAPS = {"REINHARD": 0, "FILMIC": 1, "ACES": 2}
DEBUG_PLANES = ("normal", "albedo", "opacity", "metalness", "roughness", "emissive", "ior")


class Texture(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("width", C.c_uint32), ("height", C.c_uint32),
                ("channels", C.c_uint32), ("_pad", C.c_uint32)]


class Material(C.Structure):
    _fields_ = [("albedo", C.c_float * 3), ("emissive", C.c_float * 3), ("opacity", C.c_float),
                ("metalness", C.c_float), ("roughness", C.c_float), ("ior", C.c_float),
                ("tex_albedo", C.c_int32), ("tex_emissive", C.c_int32), ("tex_opacity", C.c_int32),
                ("tex_metalness", C.c_int32), ("tex_roughness", C.c_int32), ("tex_normal", C.c_int32)]


class Model(C.Structure):
    _fields_ = [("kind", C.c_int32), ("material", C.c_int32), ("tri_first", C.c_uint32),
                ("tri_count", C.c_uint32), ("center", C.c_float * 3), ("radius", C.c_float)]


class Light(C.Structure):
    _fields_ = [("kind", C.c_int32), ("vec", C.c_float * 3), ("color", C.c_float * 3), ("size", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("transform", C.c_float * 16), ("fov", C.c_float), ("zfar", C.c_float), ("znear", C.c_float)]


class MaterialEdit(C.Structure):
    """pth_material_edit: one material's factors in a keyframe (fields: the PTH_MAT_* bits of what is given)."""
    _fields_ = [("index", C.c_uint32), ("fields", C.c_uint32), ("albedo", C.c_float * 3), ("emissive", C.c_float * 3),
                ("opacity", C.c_float), ("metalness", C.c_float), ("roughness", C.c_float), ("ior", C.c_float)]


class Keyframe(C.Structure):
    """pth_keyframe: one frame of a keyframe file (pth_keyframes_load)."""
    _fields_ = [("has_camera", C.c_uint32), ("camera", Camera), ("has_lights", C.c_uint32), ("n_lights", C.c_uint32),
                ("lights", C.POINTER(Light)), ("n_materials", C.c_uint32), ("_pad", C.c_uint32),
                ("materials", C.POINTER(MaterialEdit))]


PTH_MAT_ALBEDO, PTH_MAT_EMISSIVE, PTH_MAT_OPACITY, PTH_MAT_METALNESS, PTH_MAT_ROUGHNESS, PTH_MAT_IOR = 1, 2, 4, 8, 16, 32


class SceneDesc(C.Structure):
    _fields_ = [("n_models", C.c_uint32), ("n_materials", C.c_uint32), ("n_textures", C.c_uint32),
                ("n_lights", C.c_uint32), ("n_triangles", C.c_uint64), ("n_texel_bytes", C.c_uint64),
                ("models", C.POINTER(Model)), ("materials", C.POINTER(Material)),
                ("textures", C.POINTER(Texture)), ("lights", C.POINTER(Light)),
                ("triangles", C.POINTER(C.c_float)), ("texels", C.POINTER(C.c_uint8)),
                ("camera", Camera), ("background", C.c_float * 3), ("_pad", C.c_uint32)]


class Profile(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("samples", C.c_uint32),
                ("bounces", C.c_uint32), ("brdf", C.c_int32), ("tonemap", C.c_int32)]

    @classmethod
    def make(cls, width=1920, height=1080, samples=64, bounces=4, tonemap="FILMIC"):
        return cls(width, height, samples, bounces, 0, TONEMAPS[tonemap] if isinstance(tonemap, str) else tonemap)


PROGRESS_FN = C.CFUNCTYPE(None, C.c_uint32, C.c_uint32, C.c_void_p)
PREVIEW_FN = C.CFUNCTYPE(None, C.POINTER(C.c_uint8), C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p)


class Opts(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("device", C.c_int32), ("shard_rank", C.c_uint32),
                ("shard_count", C.c_uint32), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32),
                ("sample_batch", C.c_uint32), ("_pad", C.c_uint32), ("progress", PROGRESS_FN),
                ("progress_user", C.c_void_p), ("preview", PREVIEW_FN), ("preview_user", C.c_void_p)]

    @classmethod
    def make(cls, flags=0, device=-1, shard_rank=0, shard_count=1, tile_w=0, tile_h=0, sample_batch=0, preview=None):
        o = cls(flags, device, shard_rank, shard_count, tile_w, tile_h, sample_batch, 0,
                C.cast(None, PROGRESS_FN), None, C.cast(None, PREVIEW_FN), None)
        if preview is not None:
            o._keep = PREVIEW_FN(preview)  # keep the trampoline alive with the struct
            o.preview = o._keep
        return o


PT_GUIDE_FLOATS = 8
PT_AOV_FLOATS, PT_AOV_FIRST_ENTRY, PT_AOV_CENTRE = 16, 1, 2
PT_DENOISE_NO_DEMODULATE = 1
PT_DENOISE_STAGES = 10


class DenoiseParams(C.Structure):
    """pt_denoise_params: the a-trous filter's settings (include/ptgpu.h)."""
    _fields_ = [("iterations", C.c_uint32), ("flags", C.c_uint32), ("normal_power_log2", C.c_uint32),
                ("tonemap", C.c_int32), ("sigma_color", C.c_float), ("sigma_depth", C.c_float)]

    @classmethod
    def default(cls, **changes):
        """pt_denoise_params_default, with fields replaced by keyword."""
        return cls._from(gpu_lib().pt_denoise_params_default, changes)

    @classmethod
    def default_var(cls, **changes):
        """pt_denoise_var_params_default (the variance-guided filter's settings), with fields replaced by keyword."""
        return cls._from(gpu_lib().pt_denoise_var_params_default, changes)

    @classmethod
    def _from(cls, fill, changes):
        p = cls()
        fill(C.byref(p))
        for k, v in changes.items():
            if k not in dict(cls._fields_):
                raise TypeError(f"pt_denoise_params has no field {k!r}")
            setattr(p, k, TONEMAPS[v] if k == "tonemap" and isinstance(v, str) else v)
        return p


PT_LIGHTMIX_MAX_LIGHTS = 16


class LightMixInfo(C.Structure):
    _fields_ = [("n_lights", C.c_uint32), ("samples", C.c_uint32), ("n_local", C.c_uint64), ("device_bytes", C.c_uint64),
                ("unit", C.c_float * PT_LIGHTMIX_MAX_LIGHTS)]


PT_FILM_MAX_SAMPLES = 1 << 24
PT_FILM_DEFAULT_LUM_FLOOR = 0.01


class FilmInfo(C.Structure):
    """pt_film_info."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("passes", C.c_uint32), ("last_pass_samples", C.c_uint32),
                ("n_local", C.c_uint64), ("samples", C.c_uint64), ("device_bytes", C.c_uint64)]


class FilmNoise(C.Structure):
    """pt_film_noise_stats: what pt_film_noise makes of the film's moments."""
    _fields_ = [("mean_error", C.c_double), ("max_block_error", C.c_double), ("fraction_over", C.c_double),
                ("samples", C.c_uint64), ("n_blocks", C.c_uint32), ("converged", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


FILM_PASS_FN = C.CFUNCTYPE(None, C.POINTER(FilmInfo), C.POINTER(FilmNoise), C.c_void_p)


class FilmTileStats(C.Structure):
    """pt_film_tile_stats: what pt_film_tile_noise makes of the film's moments and counts."""
    _fields_ = [("mean_error", C.c_double), ("max_tile_error", C.c_double), ("samples", C.c_uint64),
                ("pixel_samples", C.c_uint64), ("n_tiles", C.c_uint32), ("over_tiles", C.c_uint32),
                ("active_tiles", C.c_uint32), ("converged", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class FilmAdaptiveInfo(C.Structure):
    """pt_film_adaptive_info."""
    _fields_ = [("uniform", C.c_uint32), ("tile_w", C.c_uint32), ("tile_h", C.c_uint32), ("tiles_x", C.c_uint32),
                ("tiles_y", C.c_uint32), ("n_tiles", C.c_uint32), ("tile_passes", C.c_uint32), ("last_pass_tiles", C.c_uint32),
                ("min_samples", C.c_uint64), ("max_samples", C.c_uint64), ("pixel_samples", C.c_uint64),
                ("device_bytes", C.c_uint64)]


class FilmAdaptiveParams(C.Structure):
    """pt_film_adaptive_params."""
    _fields_ = [("target", C.c_double), ("max_samples", C.c_uint64), ("lum_floor", C.c_float),
                ("first_pass_samples", C.c_uint32), ("uniform_samples", C.c_uint32), ("dilate", C.c_uint32)]

    @classmethod
    def default(cls, **changes):
        """pt_film_adaptive_params_default, with fields replaced by keyword."""
        p = cls()
        gpu_lib().pt_film_adaptive_params_default(C.byref(p))
        for k, v in changes.items():
            if k not in dict(cls._fields_):
                raise TypeError(f"pt_film_adaptive_params has no field {k!r}")
            setattr(p, k, v)
        return p


class FilmFilteredParams(C.Structure):
    """pt_film_filtered_params: the adaptive loop's settings and the variance filter's."""
    _fields_ = [("adaptive", FilmAdaptiveParams), ("filter", DenoiseParams)]

    @classmethod
    def default(cls, filter=None, **changes):
        """pt_film_filtered_params_default; keywords replace fields of .adaptive, `filter` (a DenoiseParams) replaces .filter."""
        p = cls()
        gpu_lib().pt_film_filtered_params_default(C.byref(p))
        for k, v in changes.items():
            if k not in dict(FilmAdaptiveParams._fields_):
                raise TypeError(f"pt_film_adaptive_params has no field {k!r}")
            setattr(p.adaptive, k, v)
        if filter is not None:
            p.filter = filter
        return p


class FilmWindowInfo(C.Structure):
    """pt_film_window_info."""
    _fields_ = [("windowed", C.c_uint32), ("enumeration", C.c_uint32), ("windows", C.c_uint32), ("tile_windows", C.c_uint32)]


class FilmWindowParams(C.Structure):
    """pt_film_window_params."""
    _fields_ = [("target", C.c_double), ("lum_floor", C.c_float), ("window_samples", C.c_uint32), ("adaptive", C.c_uint32),
                ("uniform_samples", C.c_uint32), ("dilate", C.c_uint32)]

    @classmethod
    def default(cls, **changes):
        """pt_film_window_params_default, with fields replaced by keyword."""
        p = cls()
        gpu_lib().pt_film_window_params_default(C.byref(p))
        for k, v in changes.items():
            if k not in dict(cls._fields_):
                raise TypeError(f"pt_film_window_params has no field {k!r}")
            setattr(p, k, v)
        return p


class FilmShardInfo(C.Structure):
    """pt_film_shard_info."""
    _fields_ = [("shard", C.c_uint32), ("rank", C.c_uint32), ("count", C.c_uint32), ("n_tiles", C.c_uint32),
                ("own_tiles", C.c_uint32), ("_pad", C.c_uint32), ("n_pixels", C.c_uint64)]


# pt_film_exchange_fn: int (float* tile_sum, float* tile_max, uint32_t n_tiles, void* user)
FILM_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_void_p)


class HistoryParams(C.Structure):
    """pt_history_params: the reprojection tests, the cap and the window rotation of a History (include/ptgpu.h)."""
    _fields_ = [("normal_cos", C.c_float), ("plane_tol", C.c_float), ("max_samples", C.c_uint32), ("rotate", C.c_uint32)]

    @classmethod
    def default(cls, **changes):
        """pt_history_params_default, with fields replaced by keyword."""
        p = cls()
        gpu_lib().pt_history_params_default(C.byref(p))
        for k, v in changes.items():
            if k not in dict(cls._fields_):
                raise TypeError(f"pt_history_params has no field {k!r}")
            setattr(p, k, v)
        return p


class HistoryInfo(C.Structure):
    """pt_history_info."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("frames", C.c_uint32), ("last_samples", C.c_uint32),
                ("min_count", C.c_uint32), ("max_count", C.c_uint32), ("device_bytes", C.c_uint64), ("params", HistoryParams)]


class HistoryView(C.Structure):
    """pt_history_view: the constants of one camera for the history's image size (M row-major)."""
    _fields_ = [("c3", C.c_float * 3), ("M", C.c_float * 9), ("tx", C.c_float), ("ty", C.c_float)]


class Hit(C.Structure):
    _fields_ = [("prim", C.c_int32), ("flags", C.c_int32), ("dist", C.c_float), ("u", C.c_float),
                ("v", C.c_float)]


class Timing(C.Structure):
    _fields_ = [("launches", C.c_uint32), ("integrate_ms", C.c_float), ("postprocess_ms", C.c_float),
                ("total_ms", C.c_float), ("generate_ms", C.c_float), ("trace_ms", C.c_float),
                ("shade_ms", C.c_float), ("shadow_ms", C.c_float), ("accumulate_ms", C.c_float),
                ("stage_launches", C.c_uint32), ("bounce0_launches", C.c_uint32), ("bounce0_ms", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "segments", "shadow_rays", "nodes_visited",
                                          "tris_tested", "shaded_hits", "rng_draws", "restarts",
                                          "max_nodes_per_cast", "casts_over_1k_nodes", "trace_nodes", "trace_tris",
                                          "shadow_skipped", "bounce0_hits", "bounce0_shadow_rays", "bounce0_tris",
                                          "grid_tris", "bounce0_cam_tris", "deferred_casts", "exact_casts", "masked_casts", "bounce0_masked")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class SceneInfo(C.Structure):
    _fields_ = [("n_prims", C.c_uint64), ("n_kd_nodes", C.c_uint64), ("n_kd_leaves", C.c_uint64),
                ("n_leaf_refs", C.c_uint64), ("kd_depth", C.c_uint32), ("has_translucent", C.c_uint32),
                ("kd_build_seconds", C.c_float), ("upload_seconds", C.c_float), ("device_bytes", C.c_uint64),
                ("cam_grid_res", C.c_uint32), ("light_grids", C.c_uint32), ("grid_refs", C.c_uint64),
                ("grid_build_seconds", C.c_float), ("escape_build_seconds", C.c_float), ("escape_prims", C.c_uint32),
                ("escape_clear_fraction", C.c_float), ("queue_bytes", C.c_uint64), ("queue_chunk_items", C.c_uint32),
                ("frame_planned", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class KdNode(C.Structure):
    _fields_ = [("w0", C.c_uint32), ("w1", C.c_uint32)]


class KdTree(C.Structure):
    _fields_ = [("n_nodes", C.c_uint64), ("n_refs", C.c_uint64), ("n_leaves", C.c_uint64),
                ("depth", C.c_uint32), ("_pad", C.c_uint32), ("bounds_min", C.c_float * 3),
                ("bounds_max", C.c_float * 3), ("nodes", C.POINTER(KdNode)), ("refs", C.POINTER(C.c_uint32)),
                ("build_seconds", C.c_double), ("expected_nodes", C.c_double), ("expected_tests", C.c_double)]


class GridRef(C.Structure):
    _fields_ = [("prim", C.c_uint32), ("mindist", C.c_float)]


class OriginGridC(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("res", C.c_uint32), ("n_cells", C.c_uint64), ("n_refs", C.c_uint64),
                ("n_global", C.c_uint32), ("enabled", C.c_uint32), ("max_cell_refs", C.c_uint32),
                ("ray_offset", C.c_float), ("cell_off", C.POINTER(C.c_uint32)), ("refs", C.POINTER(GridRef)),
                ("build_seconds", C.c_double), ("kind", C.c_uint32), ("axis_u", C.c_float * 3),
                ("axis_v", C.c_float * 3), ("axis_w", C.c_float * 3), ("u0", C.c_float), ("v0", C.c_float),
                ("cells_per_unit", C.c_float)]


class OracleStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("samples", "segments", "shadow_rays", "shaded_hits", "rng_draws",
                                          "max_draws_per_sample", "numeric_errors")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


_host = None
_gpu = None

# Every symbol include/pthost.h declares (tests check they are all exported).
HOST_SYMBOLS = ["pth_scene_load_isf", "pth_scene_free", "pth_scene_desc", "pth_scene_generate_ps5",
                "pth_scene_save_isf", "pth_convert_gltf", "pth_profile_load", "pth_profile_parse", "pth_png_read",
                "pth_png_decode", "pth_png_write_rgb8", "pth_free", "pth_prim_count", "pth_kd_build",
                "pth_kd_free", "pth_origin_grid_build", "pth_ortho_grid_build", "pth_origin_grid_auto_resolution", "pth_origin_grid_free",
                "pth_last_error", "pth_scene_set_camera", "pth_camera_path_load", "pth_camera_path_free",
                "pth_scene_set_lights", "pth_scene_set_materials", "pth_keyframes_load", "pth_keyframes_free", "pth_keyframe_apply",
                "pth_lights_differ_in_color_only"]
# Every symbol include/ptgpu.h declares.
GPU_SYMBOLS = ["pt_scene_create", "pt_scene_destroy", "pt_scene_set_camera", "pt_scene_set_lights", "pt_scene_set_materials", "pt_prep_create", "pt_prep_destroy", "pt_scene_create_from_prep",
               "pt_comm_unique_id", "pt_comm_create", "pt_comm_create_all", "pt_comm_destroy", "pt_gather_tiles", "pt_render_gathered", "pt_local_pixel_count", "pt_local_pixel_map",
               "pt_render", "pt_render_device", "pt_debug_render", "pt_assemble_tiles", "pt_get_timing", "pt_get_counters",
               "pt_scene_get_info", "pt_get_cull_stats", "pt_get_rng_cache_stats", "pt_get_hit_cache_stats", "pt_get_vis_cache_stats", "pt_get_hit1_cache_stats", "pt_get_hit1_fused_stats", "pt_get_cont_cache_stats", "pt_get_cont_escape_stats", "pt_get_b0_lean_stats", "pt_get_b1_lean_stats", "pt_scene_cont_states_copy", "pt_get_hit2_cache_stats", "pt_get_vis1_cache_stats", "pt_get_bounce1_fused_stats", "pt_get_bounce_hits_cache_stats", "pt_get_bounce_vis_cache_stats", "pt_get_bounce_fused_stats", "pt_kernel_occupancy", "pt_scene_escape_copy", "pt_escape_query", "pt_scene_grid_header", "pt_scene_grid_copy", "pt_trace_rays", "pt_trace_rays_wavefront",
               "pt_trace_rays_all", "pt_intersect_triangles",
               "pt_rng_words", "pt_eval_math", "pt_measure_copy_bandwidth", "pt_measure_gather_rate", "pt_last_error",
               "pt_version", "pt_render_guides", "pt_render_guides_device", "pt_denoise_params_default", "pt_denoise_scratch_bytes",
               "pt_denoise", "pt_denoise_device", "pt_render_denoised", "pt_denoise_stage_times",
               "pt_render_moments", "pt_render_moments_device", "pt_render_samples", "pt_denoise_var_params_default",
               "pt_denoise_var_scratch_bytes", "pt_denoise_var", "pt_denoise_var_device", "pt_render_denoised_var",
               "pt_denoise_var_stage_times",
               "pt_lightmix_capture", "pt_lightmix_create_from_planes", "pt_lightmix_destroy", "pt_lightmix_get_info",
               "pt_lightmix_basis", "pt_lightmix_apply", "pt_lightmix_apply_device",
               "pt_film_create", "pt_film_create_from_planes", "pt_film_destroy", "pt_film_reset", "pt_film_get_info",
               "pt_film_read", "pt_film_planes_device", "pt_film_add_pass", "pt_film_add_planes", "pt_film_noise", "pt_film_resolve",
               "pt_film_resolve_device", "pt_film_render_until", "pt_film_kernel_times",
               "pt_tiles_pixel_count", "pt_tiles_pixel_map", "pt_render_tiles", "pt_render_tiles_device",
               "pt_film_add_tile_pass", "pt_film_add_tile_planes", "pt_film_read_counts", "pt_film_tile_noise",
               "pt_film_get_adaptive_info", "pt_film_render_until_adaptive", "pt_film_adaptive_params_default",
               "pt_film_adaptive_kernel_times",
               "pt_film_filtered_params_default", "pt_film_denoise_scratch_bytes", "pt_film_denoise_device", "pt_film_denoise",
               "pt_film_tile_reduce_device", "pt_film_filtered_noise", "pt_film_render_until_filtered",
               "pt_film_denoise_kernel_times",
               "pt_render_window", "pt_render_window_device", "pt_film_create_windowed", "pt_film_add_window",
               "pt_film_add_tile_window", "pt_film_get_window_info", "pt_film_window_params_default",
               "pt_film_render_until_windowed", "pt_film_window_kernel_times",
               "pt_film_create_shard", "pt_film_get_shard_info", "pt_film_shard_tile_noise", "pt_film_tile_stats_from_sums",
               "pt_film_select_tiles", "pt_film_render_until_adaptive_sharded", "pt_film_render_until_windowed_sharded",
               "pt_film_exchange_comm", "pt_film_assemble",
               "pt_render_aov", "pt_render_aov_device", "pt_render_aov_samples", "pt_aov_guides", "pt_aov_guides_device",
               "pt_render_denoised_aov",
               "pt_history_params_default", "pt_history_create", "pt_history_destroy", "pt_history_reset", "pt_history_get_info",
               "pt_history_get_view", "pt_history_advance", "pt_history_advance_device", "pt_history_add_frame", "pt_history_read",
               "pt_history_resolve", "pt_history_resolve_device", "pt_history_denoise", "pt_history_denoise_device",
               "pt_history_kernel_times"]


def host_lib():
    """libpthost.so: loader, profile, PNG, generator, KD builder (no HIP)."""
    global _host
    if _host is None:
        path = PKG_DIR / "libpthost.so"
        if not path.exists():
            raise PtError(-2, f"{path} is missing: run `make host` (or __graft_entry__.build())")
        L = C.CDLL(str(path))
        L.pth_scene_load_isf.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.pth_scene_free.argtypes = [C.c_void_p]
        L.pth_scene_free.restype = None
        L.pth_scene_desc.argtypes = [C.c_void_p]
        L.pth_scene_desc.restype = C.POINTER(SceneDesc)
        L.pth_scene_generate_ps5.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_void_p)]
        L.pth_scene_save_isf.argtypes = [C.c_void_p, C.c_char_p]
        L.pth_convert_gltf.argtypes = [C.c_char_p, C.c_char_p]
        L.pth_profile_load.argtypes = [C.c_char_p, C.POINTER(Profile)]
        L.pth_profile_parse.argtypes = [C.c_char_p, C.POINTER(Profile)]
        L.pth_png_read.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                   C.POINTER(C.POINTER(C.c_uint8))]
        L.pth_png_decode.argtypes = [C.c_char_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32), C.POINTER(C.POINTER(C.c_uint8))]
        L.pth_png_write_rgb8.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p]
        L.pth_free.argtypes = [C.c_void_p]
        L.pth_free.restype = None
        L.pth_prim_count.argtypes = [C.POINTER(SceneDesc)]
        L.pth_prim_count.restype = C.c_uint64
        L.pth_kd_build.argtypes = [C.POINTER(SceneDesc), C.POINTER(KdTree)]
        L.pth_kd_free.argtypes = [C.POINTER(KdTree)]
        L.pth_kd_free.restype = None
        L.pth_origin_grid_build.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_float), C.c_uint32, C.c_float,
                                            C.c_float, C.POINTER(OriginGridC)]
        L.pth_ortho_grid_build.argtypes = [C.POINTER(SceneDesc), C.POINTER(C.c_float), C.c_uint32, C.POINTER(OriginGridC)]
        L.pth_origin_grid_free.argtypes = [C.POINTER(OriginGridC)]
        L.pth_origin_grid_free.restype = None
        L.pth_last_error.restype = C.c_char_p
        L.pth_scene_set_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
        L.pth_camera_path_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(Camera)), C.POINTER(C.c_uint32)]
        L.pth_camera_path_free.argtypes = [C.POINTER(Camera)]
        L.pth_camera_path_free.restype = None
        L.pth_scene_set_lights.argtypes = [C.c_void_p, C.POINTER(Light), C.c_uint32]
        L.pth_scene_set_materials.argtypes = [C.c_void_p, C.POINTER(Material), C.c_uint32]
        L.pth_keyframes_load.argtypes = [C.c_char_p, C.POINTER(C.POINTER(Keyframe)), C.POINTER(C.c_uint32)]
        L.pth_keyframes_free.argtypes = [C.POINTER(Keyframe)]
        L.pth_keyframes_free.restype = None
        L.pth_keyframe_apply.argtypes = [C.c_void_p, C.POINTER(Keyframe)]
        L.pth_lights_differ_in_color_only.argtypes = [C.POINTER(Light), C.c_uint32, C.POINTER(Light), C.c_uint32]
        _host = L
    return _host


def gpu_lib():
    """libptgpu.so: the HIP integrator behind the C ABI.  Fails loudly when missing."""
    global _gpu
    if _gpu is None:
        path = Path(os.environ.get("PT_GPU_LIB", PKG_DIR / "libptgpu.so"))  # override: A/B builds only
        if not path.exists():
            raise PtError(-4, f"{path} is missing: the HIP extension was not built "
                              "(run `make gpu` or __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(str(path))
        vp = C.c_void_p
        L.pt_scene_create.argtypes = [C.POINTER(SceneDesc), C.c_int, C.POINTER(vp)]
        L.pt_scene_destroy.argtypes = [vp]
        L.pt_scene_destroy.restype = None
        L.pt_prep_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(vp)]
        L.pt_prep_destroy.argtypes = [vp]
        L.pt_prep_destroy.restype = None
        L.pt_scene_create_from_prep.argtypes = [vp, C.c_int, C.POINTER(vp)]
        L.pt_scene_set_camera.argtypes = [vp, C.POINTER(Camera)]
        L.pt_scene_set_lights.argtypes = [vp, C.POINTER(Light), C.c_uint32]
        L.pt_scene_set_materials.argtypes = [vp, C.POINTER(Material), C.c_uint32]
        L.pt_comm_unique_id.argtypes = [vp]
        L.pt_comm_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
        L.pt_comm_create_all.argtypes = [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]
        L.pt_comm_destroy.argtypes = [vp]
        L.pt_comm_destroy.restype = None
        L.pt_gather_tiles.argtypes = [vp, C.POINTER(Profile), C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, vp, vp, vp, vp]
        L.pt_render_gathered.argtypes = [vp, vp, C.POINTER(Profile), C.POINTER(Opts), C.c_uint64, vp]
        L.pt_local_pixel_count.argtypes = [C.POINTER(Profile), C.POINTER(Opts)]
        L.pt_local_pixel_count.restype = C.c_uint64
        L.pt_local_pixel_map.argtypes = [C.POINTER(Profile), C.POINTER(Opts), vp]
        L.pt_render.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), vp, vp]
        L.pt_render_device.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), vp, vp, vp]
        L.pt_assemble_tiles.argtypes = [C.POINTER(Profile), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                        C.c_uint32, vp, vp, vp]
        L.pt_debug_render.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.POINTER(C.c_int)]
        L.pt_get_timing.argtypes = [vp, C.POINTER(Timing)]
        L.pt_get_counters.argtypes = [vp, C.POINTER(Counters)]
        L.pt_scene_get_info.argtypes = [vp, C.POINTER(SceneInfo)]
        L.pt_trace_rays.argtypes = [vp, vp, C.c_uint64, vp]
        L.pt_trace_rays_wavefront.argtypes = [vp, vp, vp, C.c_uint64, C.c_uint32, vp]
        L.pt_scene_grid_header.argtypes = [vp, C.c_uint32, vp]
        L.pt_scene_escape_copy.argtypes = [vp, vp, C.c_uint64]
        if hasattr(L, "pt_escape_query"):
            L.pt_escape_query.argtypes = [vp, vp, vp, C.c_uint64, vp]
        L.pt_get_cull_stats.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        if hasattr(L, "pt_get_rng_cache_stats"):   # (an A/B library of an earlier commit, PT_GPU_LIB, has none)
            L.pt_get_rng_cache_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
        if hasattr(L, "pt_get_hit_cache_stats"):
            L.pt_get_hit_cache_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 5
        if hasattr(L, "pt_get_vis_cache_stats"):
            L.pt_get_vis_cache_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
        if hasattr(L, "pt_get_hit1_cache_stats"):
            L.pt_get_hit1_cache_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 7
        if hasattr(L, "pt_get_hit1_fused_stats"):
            L.pt_get_hit1_fused_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
        if hasattr(L, "pt_get_cont_cache_stats"):
            L.pt_get_cont_cache_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 7
        if hasattr(L, "pt_get_b0_lean_stats"):
            L.pt_get_b0_lean_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 3
            L.pt_get_b0_lean_stats.restype = C.c_int
        if hasattr(L, "pt_get_b1_lean_stats"):
            L.pt_get_b1_lean_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
            L.pt_get_b1_lean_stats.restype = C.c_int
        if hasattr(L, "pt_get_cont_escape_stats"):
            L.pt_get_cont_escape_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
            L.pt_scene_cont_states_copy.argtypes = [vp, vp, C.c_uint64]
        if hasattr(L, "pt_get_hit2_cache_stats"):
            L.pt_get_hit2_cache_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 7
        if hasattr(L, "pt_get_vis1_cache_stats"):
            L.pt_get_vis1_cache_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
        if hasattr(L, "pt_get_bounce1_fused_stats"):
            L.pt_get_bounce1_fused_stats.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 6
        for name, n in (("pt_get_bounce_hits_cache_stats", 7), ("pt_get_bounce_vis_cache_stats", 4), ("pt_get_bounce_fused_stats", 6)):
            if hasattr(L, name):
                getattr(L, name).argtypes = [vp, C.c_uint32] + [C.POINTER(C.c_uint64)] * n
        if hasattr(L, "pt_kernel_occupancy"):
            L.pt_kernel_occupancy.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int)]
        L.pt_scene_grid_copy.argtypes = [vp, C.c_uint32, vp, vp]
        L.pt_trace_rays_all.argtypes = [vp, vp, C.c_uint64, C.c_uint32, vp, vp]
        L.pt_intersect_triangles.argtypes = [C.c_int, vp, vp, C.c_uint64, vp]
        L.pt_rng_words.argtypes = [C.c_int, vp, C.c_uint64, C.c_uint32, vp]
        L.pt_eval_math.argtypes = [C.c_int, C.c_int, vp, C.c_uint64, vp]
        L.pt_measure_copy_bandwidth.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]
        L.pt_measure_gather_rate.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_double)]
        dp = C.POINTER(DenoiseParams)
        L.pt_render_guides.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
        L.pt_render_guides_device.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp]
        L.pt_denoise_params_default.argtypes = [dp]
        L.pt_denoise_params_default.restype = None
        L.pt_denoise_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]
        L.pt_denoise_scratch_bytes.restype = C.c_uint64
        L.pt_denoise.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, dp, vp, vp, vp, vp]
        L.pt_denoise_device.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, dp, vp, vp, vp, vp, vp, vp]
        L.pt_render_denoised.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), dp, vp, vp]
        L.pt_denoise_stage_times.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, dp, vp, vp, vp, vp, vp, vp]
        L.pt_render_moments.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), vp, vp, vp]
        L.pt_render_moments_device.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), vp, vp, vp, vp]
        L.pt_render_samples.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), vp]
        L.pt_denoise_var_params_default.argtypes = [dp]
        L.pt_denoise_var_params_default.restype = None
        L.pt_denoise_var_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]
        L.pt_denoise_var_scratch_bytes.restype = C.c_uint64
        L.pt_denoise_var.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, dp, vp, vp, vp, vp, vp]
        L.pt_denoise_var_device.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, dp, vp, vp, vp, vp, vp, vp, vp]
        L.pt_render_denoised_var.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), dp, vp, vp]
        L.pt_denoise_var_stage_times.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, dp, vp, vp, vp, vp, vp, vp, vp]
        if hasattr(L, "pt_render_aov"):   # (an A/B library of an earlier commit has no AOV pass)
            L.pt_render_aov.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), C.c_uint32, vp]
            L.pt_render_aov_device.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), C.c_uint32, vp, vp]
            L.pt_render_aov_samples.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), C.c_uint32, vp]
            L.pt_aov_guides.argtypes = [C.c_int, C.c_uint64, C.c_uint32, vp, vp]
            L.pt_aov_guides_device.argtypes = [C.c_int, C.c_uint64, C.c_uint32, vp, vp, vp]
            L.pt_render_denoised_aov.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), dp, C.c_int, C.c_uint32, vp, vp]
        if hasattr(L, "pt_lightmix_capture"):   # (an A/B library of an earlier commit has no light mixer)
            L.pt_lightmix_capture.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), C.POINTER(vp)]
            L.pt_lightmix_create_from_planes.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, vp, vp, C.POINTER(vp)]
            L.pt_lightmix_destroy.argtypes = [vp]
            L.pt_lightmix_destroy.restype = None
            L.pt_lightmix_get_info.argtypes = [vp, C.POINTER(LightMixInfo)]
            L.pt_lightmix_basis.argtypes = [vp, C.c_uint32, vp]
            L.pt_lightmix_apply.argtypes = [vp, vp, C.c_int, vp, vp]
            L.pt_lightmix_apply_device.argtypes = [vp, vp, C.c_int, vp, vp, vp]
        if hasattr(L, "pt_film_create"):   # (an A/B library of an earlier commit has no film)
            L.pt_film_create.argtypes = [C.c_int, C.POINTER(Profile), C.POINTER(Opts), C.POINTER(vp)]
            L.pt_film_create_from_planes.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, vp, vp, C.POINTER(vp)]
            L.pt_film_destroy.argtypes = [vp]
            L.pt_film_destroy.restype = None
            L.pt_film_reset.argtypes = [vp]
            L.pt_film_get_info.argtypes = [vp, C.POINTER(FilmInfo)]
            L.pt_film_read.argtypes = [vp, vp, vp]
            L.pt_film_planes_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
            L.pt_film_add_pass.argtypes = [vp, vp, C.c_uint32]
            L.pt_film_add_planes.argtypes = [vp, C.c_uint32, vp, vp]
            L.pt_film_noise.argtypes = [vp, C.c_float, C.c_double, C.POINTER(FilmNoise), vp, vp, vp]
            L.pt_film_resolve.argtypes = [vp, C.c_int, vp, vp]
            L.pt_film_resolve_device.argtypes = [vp, C.c_int, vp, vp, vp]
            L.pt_film_render_until.argtypes = [vp, vp, C.c_uint32, C.c_uint64, C.c_float, C.c_double, FILM_PASS_FN, vp,
                                               C.POINTER(FilmNoise)]
            L.pt_film_kernel_times.argtypes = [vp, C.c_float, C.c_int, C.c_uint32, vp, vp]
        if hasattr(L, "pt_render_tiles"):   # (an A/B library of an earlier commit has no tile-list frames, no adaptive film)
            L.pt_tiles_pixel_count.argtypes = [C.POINTER(Profile), C.POINTER(Opts), vp, C.c_uint32]
            L.pt_tiles_pixel_count.restype = C.c_uint64
            L.pt_tiles_pixel_map.argtypes = [C.POINTER(Profile), C.POINTER(Opts), vp, C.c_uint32, vp]
            L.pt_render_tiles.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), vp, C.c_uint32, vp, vp, vp]
            L.pt_render_tiles_device.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), vp, C.c_uint32, vp, vp, vp, vp]
            L.pt_film_add_tile_pass.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32]
            L.pt_film_add_tile_planes.argtypes = [vp, C.c_uint32, vp, C.c_uint32, vp, vp]
            L.pt_film_read_counts.argtypes = [vp, vp]
            L.pt_film_tile_noise.argtypes = [vp, C.c_float, C.c_double, C.POINTER(FilmTileStats), vp, vp, vp]
            L.pt_film_get_adaptive_info.argtypes = [vp, C.POINTER(FilmAdaptiveInfo)]
            L.pt_film_render_until_adaptive.argtypes = [vp, vp, C.POINTER(FilmAdaptiveParams), FILM_PASS_FN, vp,
                                                        C.POINTER(FilmTileStats)]
            L.pt_film_adaptive_params_default.argtypes = [C.POINTER(FilmAdaptiveParams)]
            L.pt_film_adaptive_params_default.restype = None
            L.pt_film_adaptive_kernel_times.argtypes = [vp, C.c_float, C.c_int, C.c_uint32, vp, vp, vp]
        if hasattr(L, "pt_film_denoise"):   # (an A/B library of an earlier commit has no film filter)
            L.pt_film_filtered_params_default.argtypes = [C.POINTER(FilmFilteredParams)]
            L.pt_film_filtered_params_default.restype = None
            L.pt_film_denoise_scratch_bytes.argtypes = [vp]
            L.pt_film_denoise_scratch_bytes.restype = C.c_uint64
            L.pt_film_denoise_device.argtypes = [vp, C.c_int, dp, C.c_float, vp, vp, vp, vp, vp, vp]
            L.pt_film_denoise.argtypes = [vp, vp, C.c_int, dp, C.c_float, vp, vp, vp]
            L.pt_film_tile_reduce_device.argtypes = [vp, vp, vp, vp, vp]
            L.pt_film_filtered_noise.argtypes = [vp, vp, dp, C.c_float, C.c_double, C.POINTER(FilmTileStats), vp, vp, vp]
            L.pt_film_render_until_filtered.argtypes = [vp, vp, C.POINTER(FilmFilteredParams), FILM_PASS_FN, vp,
                                                        C.POINTER(FilmTileStats)]
            L.pt_film_denoise_kernel_times.argtypes = [vp, vp, dp, C.c_float, C.c_uint32, vp, vp, vp, vp]
        if hasattr(L, "pt_render_window"):   # (an A/B library of an earlier commit has no windows)
            L.pt_render_window.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, vp, vp]
            L.pt_render_window_device.argtypes = [vp, C.POINTER(Profile), C.POINTER(Opts), C.c_uint32, C.c_uint32, vp, C.c_uint32,
                                                  vp, vp, vp, vp]
            L.pt_film_create_windowed.argtypes = [C.c_int, C.POINTER(Profile), C.POINTER(Opts), C.POINTER(vp)]
            L.pt_film_add_window.argtypes = [vp, vp, C.c_uint32]
            L.pt_film_add_tile_window.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32]
            L.pt_film_get_window_info.argtypes = [vp, C.POINTER(FilmWindowInfo)]
            L.pt_film_window_params_default.argtypes = [C.POINTER(FilmWindowParams)]
            L.pt_film_window_params_default.restype = None
            L.pt_film_render_until_windowed.argtypes = [vp, vp, C.POINTER(FilmWindowParams), FILM_PASS_FN, vp,
                                                        C.POINTER(FilmTileStats)]
            L.pt_film_window_kernel_times.argtypes = [vp, C.c_uint32, vp, vp]
        if hasattr(L, "pt_film_create_shard"):   # (an A/B library of an earlier commit has no shard films)
            L.pt_film_create_shard.argtypes = [C.c_int, C.POINTER(Profile), C.POINTER(Opts), C.c_uint32, C.POINTER(vp)]
            L.pt_film_get_shard_info.argtypes = [vp, C.POINTER(FilmShardInfo)]
            L.pt_film_shard_tile_noise.argtypes = [vp, C.c_float, vp, vp, vp]
            L.pt_film_tile_stats_from_sums.argtypes = [vp, vp, C.c_double, C.POINTER(FilmTileStats)]
            L.pt_film_select_tiles.argtypes = [vp, vp, C.c_double, C.c_uint32, vp, C.POINTER(C.c_uint32)]
            L.pt_film_render_until_adaptive_sharded.argtypes = [vp, vp, C.POINTER(FilmAdaptiveParams), FILM_EXCHANGE_FN, vp,
                                                                FILM_PASS_FN, vp, C.POINTER(FilmTileStats)]
            L.pt_film_render_until_windowed_sharded.argtypes = [vp, vp, C.POINTER(FilmWindowParams), FILM_EXCHANGE_FN, vp,
                                                                FILM_PASS_FN, vp, C.POINTER(FilmTileStats)]
            L.pt_film_exchange_comm.argtypes = [vp, vp, C.c_uint32, vp]
            L.pt_film_assemble.argtypes = [vp, C.POINTER(vp), C.c_uint32]
        if hasattr(L, "pt_history_create"):   # (an A/B library of an earlier commit has no histories)
            L.pt_history_params_default.argtypes = [C.POINTER(HistoryParams)]
            L.pt_history_params_default.restype = None
            L.pt_history_create.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(HistoryParams), C.POINTER(vp)]
            L.pt_history_destroy.argtypes = [vp]
            L.pt_history_destroy.restype = None
            L.pt_history_reset.argtypes = [vp]
            L.pt_history_get_info.argtypes = [vp, C.POINTER(HistoryInfo)]
            L.pt_history_get_view.argtypes = [vp, C.c_int, C.POINTER(HistoryView)]
            L.pt_history_advance.argtypes = [vp, C.POINTER(Camera), C.c_uint32, vp, vp, vp, vp]
            L.pt_history_advance_device.argtypes = [vp, C.POINTER(Camera), C.c_uint32, vp, vp, vp, vp, vp]
            L.pt_history_add_frame.argtypes = [vp, vp, C.POINTER(Profile), C.POINTER(Opts), C.c_uint32]
            L.pt_history_read.argtypes = [vp, vp, vp, vp, vp, vp, vp]
            L.pt_history_resolve.argtypes = [vp, C.c_int, vp, vp]
            L.pt_history_resolve_device.argtypes = [vp, C.c_int, vp, vp, vp]
            L.pt_history_denoise.argtypes = [vp, C.c_int, C.POINTER(DenoiseParams), C.c_float, vp, vp]
            L.pt_history_denoise_device.argtypes = [vp, C.c_int, C.POINTER(DenoiseParams), C.c_float, vp, vp, vp]
            L.pt_history_kernel_times.argtypes = [vp, C.c_uint32, vp]
        L.pt_last_error.restype = C.c_char_p
        L.pt_version.restype = C.c_char_p
        _gpu = L
    return _gpu


def kernel_occupancy(which, device=0):
    """Workgroups of the fused bounce-0 kernel per compute unit (0: the variant computing its ChaCha words, 1: the cached one,
    2 / 3: the cached one storing / loading the camera hits, 4 / 5: the loading one with the shadow-visibility cache, for
    point lights / with a directional light, 6: the one that loads the bounce-0 continuation as well)."""
    n = C.c_int()
    check_gpu(gpu_lib().pt_kernel_occupancy(device, which, C.byref(n)))
    return n.value


def check_host(rc):
    if rc != PT_OK:
        raise PtError(rc, host_lib().pth_last_error().decode(errors="replace"))


def check_gpu(rc):
    if rc != PT_OK:
        raise PtError(rc, gpu_lib().pt_last_error().decode(errors="replace"))


def make_camera(camera):
    """A Camera from a Camera (copied) or a dict in ISF form ({"transform": 4 columns of 4, "fov", "zfar", "znear"}, the
    numbers narrowed to f32 as the ISF loader does).  None is passed on as a null pointer (the C ABI rejects it)."""
    if camera is None:
        return None
    if isinstance(camera, Camera):
        c = Camera()
        C.memmove(C.byref(c), C.byref(camera), C.sizeof(Camera))
        return c
    cols = camera["transform"]
    if len(cols) != 4 or any(len(col) != 4 for col in cols):
        raise ValueError("camera transform: 4 columns of 4 numbers expected")
    return Camera((C.c_float * 16)(*[float(v) for col in cols for v in col]), float(camera["fov"]),
                  float(camera["zfar"]), float(camera["znear"]))


def camera_to_dict(camera):
    """The ISF form of a Camera (f32 values as Python floats: they round-trip exactly)."""
    t = list(camera.transform)
    return {"transform": [t[4 * k:4 * k + 4] for k in range(4)], "fov": camera.fov, "zfar": camera.zfar,
            "znear": camera.znear}


def load_camera_path(path):
    """`--camera-path` file (pth_camera_path_load): a JSON array of ISF camera objects -> list of Camera."""
    ptr = C.POINTER(Camera)()
    n = C.c_uint32(0)
    check_host(host_lib().pth_camera_path_load(os.fsencode(str(path)), C.byref(ptr), C.byref(n)))
    try:
        return [make_camera(ptr[i]) for i in range(n.value)]
    finally:
        host_lib().pth_camera_path_free(ptr)


def _table(cls, items, n):
    """(array, count) for a C table of `cls` from a list of structures (copied); items None: a null pointer with count n or 0."""
    if items is None:
        return None, (0 if n is None else n)
    items = list(items)
    arr = (cls * max(1, len(items)))()
    for i, it in enumerate(items):
        C.memmove(C.byref(arr, i * C.sizeof(cls)), C.byref(it), C.sizeof(cls))
    return arr, (len(items) if n is None else n)


class Keyframes:
    """A keyframe file (pth_keyframes_load, `render --keyframes`): a list of Keyframe structures, valid while this object
    lives.  Apply frame i with HostScene.apply_keyframe / GpuScene.apply_keyframe."""

    def __init__(self, path):
        self._ptr = C.POINTER(Keyframe)()
        n = C.c_uint32(0)
        check_host(host_lib().pth_keyframes_load(os.fsencode(str(path)), C.byref(self._ptr), C.byref(n)))
        self._n = n.value

    def __len__(self):
        return self._n

    def __getitem__(self, i):
        if not 0 <= i < self._n:
            raise IndexError(i)
        return self._ptr[i]

    def __iter__(self):
        return (self[i] for i in range(self._n))

    @staticmethod
    def lights(frame):
        """The lights a frame sets (copies), or None if it keeps them."""
        return [_copy(Light, frame.lights[i]) for i in range(frame.n_lights)] if frame.has_lights else None

    @staticmethod
    def material_edits(frame):
        return [_copy(MaterialEdit, frame.materials[i]) for i in range(frame.n_materials)]

    def close(self):
        if self._ptr:
            host_lib().pth_keyframes_free(self._ptr)
            self._ptr = C.POINTER(Keyframe)()
            self._n = 0

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _copy(cls, s):
    c = cls()
    C.memmove(C.byref(c), C.byref(s), C.sizeof(cls))
    return c


def load_keyframes(path):
    """`--keyframes` file (pth_keyframes_load) -> Keyframes."""
    return Keyframes(path)


class HostScene:
    """Owned pth_scene handle (ISF file or generated)."""

    def __init__(self, handle):
        self.handle = handle
        self.desc = host_lib().pth_scene_desc(handle)

    @classmethod
    def load_isf(cls, path):
        h = C.c_void_p()
        check_host(host_lib().pth_scene_load_isf(os.fsencode(str(path)), C.byref(h)))
        return cls(h)

    @classmethod
    def generate_ps5(cls, target_tris, seed=0, flags=0):
        h = C.c_void_p()
        check_host(host_lib().pth_scene_generate_ps5(target_tris, seed, flags, C.byref(h)))
        return cls(h)

    def save_isf(self, directory):
        check_host(host_lib().pth_scene_save_isf(self.handle, os.fsencode(str(directory))))

    @property
    def n_triangles(self):
        return int(self.desc.contents.n_triangles)

    @property
    def camera(self):
        """A copy of the scene's camera."""
        return make_camera(self.desc.contents.camera)

    def set_camera(self, camera):
        """pth_scene_set_camera: camera is a Camera or a dict in ISF form."""
        c = make_camera(camera)
        check_host(host_lib().pth_scene_set_camera(self.handle, C.byref(c) if c is not None else None))

    @property
    def lights(self):
        """Copies of the scene's lights."""
        d = self.desc.contents
        return [_copy(Light, d.lights[i]) for i in range(d.n_lights)]

    @property
    def materials(self):
        """Copies of the scene's materials (pt_scene_desc.materials: in an ISF scene material i is model i's)."""
        d = self.desc.contents
        return [_copy(Material, d.materials[i]) for i in range(d.n_materials)]

    def set_lights(self, lights, n=None):
        """pth_scene_set_lights: lights is a list of Light (all of them); None passes a null pointer (with count n)."""
        arr, cnt = _table(Light, lights, n)
        check_host(host_lib().pth_scene_set_lights(self.handle, arr, cnt))

    def set_materials(self, materials, n=None):
        """pth_scene_set_materials: the whole material table, a list of Material; None passes a null pointer."""
        arr, cnt = _table(Material, materials, n)
        check_host(host_lib().pth_scene_set_materials(self.handle, arr, cnt))

    def apply_keyframe(self, frame):
        """pth_keyframe_apply: one Keyframe of a Keyframes (camera, lights, materials, in that order)."""
        check_host(host_lib().pth_keyframe_apply(self.handle, C.byref(frame)))

    @property
    def n_prims(self):
        return int(host_lib().pth_prim_count(self.desc))

    @property
    def n_lights(self):
        return int(self.desc.contents.n_lights)

    def close(self):
        if self.handle:
            host_lib().pth_scene_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OriginGrid:
    """pth_origin_grid (host/origin_grid.cpp): cube map of primitive lists around one point, with the cell lookup
    restated in numpy f32 exactly as the device computes it (csrc/pt_grid.h og_cell)."""

    def __init__(self, host_scene, origin=None, res=0, ray_offset=0.0, max_dir_len=1.001, direction=None):
        """origin: cube-map grid around a point; direction: orthographic grid for rays of that direction."""
        import numpy as np
        self.c = OriginGridC()
        if direction is not None:
            dvec = (C.c_float * 3)(*[float(v) for v in direction])
            check_host(host_lib().pth_ortho_grid_build(host_scene.desc, dvec, res, C.byref(self.c)))
        else:
            o = (C.c_float * 3)(*[float(v) for v in origin])
            check_host(host_lib().pth_origin_grid_build(host_scene.desc, o, res, ray_offset, max_dir_len, C.byref(self.c)))
        self.enabled = bool(self.c.enabled)
        self.res, self.n_global, self.n_refs = int(self.c.res), int(self.c.n_global), int(self.c.n_refs)
        if self.enabled:
            self.cell_off = np.ctypeslib.as_array(self.c.cell_off, (int(self.c.n_cells) + 1,))
            raw = np.ctypeslib.as_array(C.cast(self.c.refs, C.POINTER(C.c_uint32)), (max(1, self.n_refs) * 2,))
            self.ref_prim = raw[0::2]
            self.ref_mindist = raw[1::2].view(np.float32)

    @classmethod
    def from_device(cls, gpu_scene, which):
        """The grid the DEVICE built for a scene (csrc/pt_grid_build.h): which = 0 camera, 1 + i light i."""
        import numpy as np
        self = cls.__new__(cls)
        self.c = OriginGridC()
        self._owned = False
        check_gpu(gpu_scene.lib.pt_scene_grid_header(gpu_scene.handle, which, C.byref(self.c)))
        self.enabled = bool(self.c.enabled)
        self.res, self.n_global, self.n_refs = int(self.c.res), int(self.c.n_global), int(self.c.n_refs)
        if self.enabled:
            self.cell_off = np.zeros(int(self.c.n_cells) + 1, np.uint32)
            raw = np.zeros(max(1, self.n_refs) * 2, np.uint32)
            check_gpu(gpu_scene.lib.pt_scene_grid_copy(gpu_scene.handle, which, self.cell_off.ctypes.data, raw.ctypes.data))
            self.ref_prim = raw[0::2]
            self.ref_mindist = raw[1::2].view(np.float32)
        return self

    def cells(self, w):
        """Cell index of every direction w [n, 3] - orthographic grids: of every ray ORIGIN w - in the f32 arithmetic
        of the device (csrc/pt_grid.h og_cell / og_cell_ortho)."""
        import numpy as np
        w = np.ascontiguousarray(w, np.float32).reshape(-1, 3)
        if self.c.kind == 1:
            au, av = np.array(list(self.c.axis_u), np.float32), np.array(list(self.c.axis_v), np.float32)
            dot = lambda a: ((w[:, 0] * a[0] + w[:, 1] * a[1]).astype(np.float32) + w[:, 2] * a[2]).astype(np.float32)
            with np.errstate(all="ignore"):
                fu = ((dot(au) - np.float32(self.c.u0)) * np.float32(self.c.cells_per_unit)).astype(np.float32)
                fv = ((dot(av) - np.float32(self.c.v0)) * np.float32(self.c.cells_per_unit)).astype(np.float32)
            top = np.float32(self.res - 1)
            iu = np.nan_to_num(np.where(fu >= 0, np.minimum(np.floor(fu), top), 0)).astype(np.int64)
            iv = np.nan_to_num(np.where(fv >= 0, np.minimum(np.floor(fv), top), 0)).astype(np.int64)
            return iv * self.res + iu
        a = np.abs(w)
        axis = np.where((a[:, 0] >= a[:, 1]) & (a[:, 0] >= a[:, 2]), 0, np.where(a[:, 1] >= a[:, 2], 1, 2))
        idx = np.arange(len(w))
        wa, wb, wc = w[idx, axis], w[idx, (axis + 1) % 3], w[idx, (axis + 2) % 3]
        with np.errstate(all="ignore"):
            inv = np.float32(1.0) / np.abs(wa)
            half = np.float32(0.5 * self.res)
            fu = (wb * inv + np.float32(1.0)) * half
            fv = (wc * inv + np.float32(1.0)) * half
        top = np.float32(self.res - 1)
        iu = np.where(fu >= 0, np.minimum(np.floor(fu), top), 0)   # NaN -> 0, like the device's clamp
        iv = np.where(fv >= 0, np.minimum(np.floor(fv), top), 0)
        iu = np.nan_to_num(iu).astype(np.int64)
        iv = np.nan_to_num(iv).astype(np.int64)
        face = 2 * axis + (wa < 0)
        return (face * self.res + iv) * self.res + iu

    def depth(self, p):
        """Orthographic grids: depth of the points p along the rays' direction, as the device computes it."""
        import numpy as np
        p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
        a = np.array(list(self.c.axis_w), np.float32)
        return ((p[:, 0] * a[0] + p[:, 1] * a[1]).astype(np.float32) + p[:, 2] * a[2]).astype(np.float32)

    def candidates(self, cell):
        """(primitive words, mindist) of one cell, the global block in front."""
        import numpy as np
        b, e = int(self.cell_off[cell]), int(self.cell_off[cell + 1])
        sel = np.r_[0:self.n_global, b:e]
        return self.ref_prim[sel], self.ref_mindist[sel]

    def close(self):
        if getattr(self, "_owned", True):
            host_lib().pth_origin_grid_free(C.byref(self.c))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def convert_gltf(input_path, output_dir):
    """`path-tracer convert`: glTF 2.0 -> output_dir/scene.isf + textures (src/scene/gltf.rs:146-265)."""
    check_host(host_lib().pth_convert_gltf(os.fsencode(str(input_path)), os.fsencode(str(output_dir))))


def load_profile(path=None, text=None):
    p = Profile()
    if text is not None:
        check_host(host_lib().pth_profile_parse(text.encode(), C.byref(p)))
    else:
        check_host(host_lib().pth_profile_load(os.fsencode(str(path)) if path else None, C.byref(p)))
    return p


class Prep:
    """pt_prep: the host half of pt_scene_create (KD-tree, origin grids), built once for several devices."""

    def __init__(self, host_scene: HostScene):
        self.handle = C.c_void_p()
        self._host = host_scene
        check_gpu(gpu_lib().pt_prep_create(host_scene.desc, C.byref(self.handle)))

    def close(self):
        if self.handle:
            gpu_lib().pt_prep_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """pt_comm: RCCL communicator of the tile gather (one process per GPU: unique id from rank 0)."""

    def __init__(self, unique_id: bytes, rank, size, device):
        self.handle = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        check_gpu(gpu_lib().pt_comm_create(buf, rank, size, device, C.byref(self.handle)))
        self.rank, self.size = rank, size

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        check_gpu(gpu_lib().pt_comm_unique_id(buf))
        return bytes(buf)

    def gather_tiles(self, profile, tile_w, tile_h, slice_pixels, elem_bytes, d_local, d_gathered, d_image, stream=0):
        check_gpu(gpu_lib().pt_gather_tiles(self.handle, C.byref(profile), tile_w, tile_h, slice_pixels, elem_bytes,
                                            d_local, d_gathered, d_image, stream))

    def close(self):
        if self.handle:
            gpu_lib().pt_comm_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GpuScene:
    """Device-resident scene (pt_scene_create / pt_scene_destroy)."""

    def __init__(self, host_scene: HostScene, device=0, prep=None):
        self.lib = gpu_lib()
        self.handle = C.c_void_p()
        self._host = host_scene
        if prep is not None:   # host work (KD-tree, origin grids) done once by Prep, uploaded here
            check_gpu(self.lib.pt_scene_create_from_prep(prep.handle, device, C.byref(self.handle)))
        else:
            check_gpu(self.lib.pt_scene_create(host_scene.desc, device, C.byref(self.handle)))

    def info(self):
        i = SceneInfo()
        check_gpu(self.lib.pt_scene_get_info(self.handle, C.byref(i)))
        return i

    def set_camera(self, camera):
        """pt_scene_set_camera: camera is a Camera or a dict in ISF form; None raises PtError (PT_ERR_INVALID)."""
        c = make_camera(camera)
        check_gpu(self.lib.pt_scene_set_camera(self.handle, C.byref(c) if c is not None else None))

    def set_lights(self, lights, n=None):
        """pt_scene_set_lights: lights is a list of Light (all of them; [] removes every light); None passes a null pointer
        with count n (PT_ERR_INVALID for n > 0)."""
        arr, cnt = _table(Light, lights, n)
        check_gpu(self.lib.pt_scene_set_lights(self.handle, arr, cnt))

    def set_materials(self, materials, n=None):
        """pt_scene_set_materials: the whole material table (as many as the scene was made with), a list of Material."""
        arr, cnt = _table(Material, materials, n)
        check_gpu(self.lib.pt_scene_set_materials(self.handle, arr, cnt))

    def apply_keyframe(self, frame, host_scene):
        """What `render --keyframes` does for a frame after the first: host_scene (the description this scene renders) takes
        the frame, then this scene takes its camera, lights and materials - those the frame names."""
        host_scene.apply_keyframe(frame)
        if frame.has_camera:
            self.set_camera(host_scene.camera)
        if frame.has_lights:
            self.set_lights(host_scene.lights)
        if frame.n_materials:
            self.set_materials(host_scene.materials)

    def render(self, profile, opts=None):
        """Host-buffer render: returns (rgb8 [n,3] uint8, accum [n,3] float32)."""
        import numpy as np
        opts = opts or Opts.make()
        n = int(self.lib.pt_local_pixel_count(C.byref(profile), C.byref(opts)))
        rgb = np.empty((n, 3), np.uint8)
        acc = np.empty((n, 3), np.float32)
        check_gpu(self.lib.pt_render(self.handle, C.byref(profile), C.byref(opts), rgb.ctypes.data, acc.ctypes.data))
        return rgb, acc

    def render_device(self, profile, opts, d_rgb8, d_accum, stream=0):
        check_gpu(self.lib.pt_render_device(self.handle, C.byref(profile), C.byref(opts), d_rgb8, d_accum, stream))

    def debug_render(self, width, height):
        """--debug-textures planes: dict name -> [H*W, 3] uint8, or {} when nothing was hit."""
        import numpy as np
        planes = np.zeros((7, width * height, 3), np.uint8)
        any_hit = C.c_int(0)
        check_gpu(self.lib.pt_debug_render(self.handle, width, height, planes.ctypes.data, C.byref(any_hit)))
        if not any_hit.value:
            return {}
        return dict(zip(DEBUG_PLANES, planes))

    def render_guides(self, width, height):
        """pt_render_guides: [H*W, 8] float32 - normal3, depth, albedo3, primitive index as int32 bits (view(np.int32))."""
        import numpy as np
        g = np.empty((width * height, PT_GUIDE_FLOATS), np.float32)
        check_gpu(self.lib.pt_render_guides(self.handle, width, height, g.ctypes.data))
        return g

    def render_guides_device(self, width, height, d_guides, stream=0):
        check_gpu(self.lib.pt_render_guides_device(self.handle, width, height, d_guides, stream))

    def render_denoised(self, profile, params, opts=None):
        """pt_render_denoised: (rgb8 [H*W, 3] uint8, color [H*W, 3] float32 mean radiance) of the filtered frame."""
        import numpy as np
        n = profile.width * profile.height
        rgb = np.empty((n, 3), np.uint8)
        col = np.empty((n, 3), np.float32)
        check_gpu(self.lib.pt_render_denoised(self.handle, C.byref(profile), C.byref(opts) if opts is not None else None,
                                              C.byref(params) if params is not None else None, rgb.ctypes.data, col.ctypes.data))
        return rgb, col

    def render_moments(self, profile, opts=None):
        """pt_render_moments: (rgb8 [n, 3] uint8, accum [n, 3] float32, moments [n, 2] float32 = sum and sum of squares of
        the samples' luminance)."""
        import numpy as np
        opts = opts or Opts.make()
        n = int(self.lib.pt_local_pixel_count(C.byref(profile), C.byref(opts)))
        rgb = np.empty((n, 3), np.uint8)
        acc = np.empty((n, 3), np.float32)
        mom = np.empty((n, 2), np.float32)
        check_gpu(self.lib.pt_render_moments(self.handle, C.byref(profile), C.byref(opts), rgb.ctypes.data, acc.ctypes.data,
                                             mom.ctypes.data))
        return rgb, acc, mom

    def render_moments_device(self, profile, opts, d_rgb8, d_accum, d_moments, stream=0):
        check_gpu(self.lib.pt_render_moments_device(self.handle, C.byref(profile), C.byref(opts), d_rgb8, d_accum, d_moments, stream))

    def render_tiles(self, profile, tiles, opts=None, want_moments=True):
        """pt_render_tiles: (rgb8 [n, 3] uint8, accum [n, 3] float32, moments [n, 2] float32 or None) of the listed tiles
        (global tile numbers, strictly ascending), packed in list order - tiles_pixel_map gives every packed pixel's
        global index."""
        import numpy as np
        opts = opts or Opts.make()
        t = _tile_list(tiles)
        n = int(self.lib.pt_tiles_pixel_count(C.byref(profile), C.byref(opts), t.ctypes.data, len(t)))
        rgb = np.empty((n, 3), np.uint8)
        acc = np.empty((n, 3), np.float32)
        mom = np.empty((n, 2), np.float32) if want_moments else None
        check_gpu(self.lib.pt_render_tiles(self.handle, C.byref(profile), C.byref(opts), t.ctypes.data, len(t), rgb.ctypes.data,
                                           acc.ctypes.data, mom.ctypes.data if want_moments else None))
        return rgb, acc, mom

    def render_tiles_device(self, profile, opts, tiles, d_rgb8, d_accum, d_moments, stream=0):
        """pt_render_tiles_device: device pointers (any may be 0 / None, not all)."""
        t = _tile_list(tiles)
        check_gpu(self.lib.pt_render_tiles_device(self.handle, C.byref(profile), C.byref(opts), t.ctypes.data, len(t),
                                                  d_rgb8 or None, d_accum or None, d_moments or None, stream))

    def render_window(self, profile, s0, s1, accum=None, moments=None, opts=None, tiles=None, want_moments=True):
        """pt_render_window: the samples [s0, s1) of the frame (profile, opts), continuing the sums in accum [n, 3] and
        moments [n, 2] (float32; ignored and may be None when s0 == 0).  tiles: a tile list (packed layout of render_tiles),
        None the whole frame.  Returns (rgb8, accum, moments or None) - new arrays, the arguments are not written."""
        import numpy as np
        opts = opts or Opts.make()
        t = _tile_list(tiles) if tiles is not None else None
        if t is not None:
            n = int(self.lib.pt_tiles_pixel_count(C.byref(profile), C.byref(opts), t.ctypes.data, len(t)))
        else:
            n = int(self.lib.pt_local_pixel_count(C.byref(profile), C.byref(opts)))
        rgb = np.empty((n, 3), np.uint8)
        acc = np.zeros((n, 3), np.float32) if accum is None else np.array(accum, np.float32, order="C")
        mom = None
        if want_moments:
            mom = np.zeros((n, 2), np.float32) if moments is None else np.array(moments, np.float32, order="C")
        if acc.shape != (n, 3) or (mom is not None and mom.shape != (n, 2)):
            raise PtError(PT_ERR_INVALID, "render_window: accum must be [n, 3] and moments [n, 2]")
        check_gpu(self.lib.pt_render_window(self.handle, C.byref(profile), C.byref(opts), s0, s1,
                                            t.ctypes.data if t is not None else None, len(t) if t is not None else 0,
                                            rgb.ctypes.data, acc.ctypes.data, mom.ctypes.data if mom is not None else None))
        return rgb, acc, mom

    def render_window_device(self, profile, opts, s0, s1, d_rgb8, d_accum, d_moments, tiles=None, stream=0):
        """pt_render_window_device: device pointers (d_rgb8 and d_moments may be 0 / None); d_accum and d_moments are in-out."""
        t = _tile_list(tiles) if tiles is not None else None
        check_gpu(self.lib.pt_render_window_device(self.handle, C.byref(profile), C.byref(opts), s0, s1,
                                                   t.ctypes.data if t is not None else None, len(t) if t is not None else 0,
                                                   d_rgb8 or None, d_accum or None, d_moments or None, stream))

    tiles_pixel_count = staticmethod(lambda profile, tiles, opts=None: tiles_pixel_count(profile, tiles, opts))
    tiles_pixel_map = staticmethod(lambda profile, tiles, opts=None: tiles_pixel_map(profile, tiles, opts))

    def render_samples(self, profile, opts=None):
        """pt_render_samples (test hook): [samples, n, 3] float32, the radiance of every sample of every packed pixel."""
        import numpy as np
        opts = opts or Opts.make()
        n = int(self.lib.pt_local_pixel_count(C.byref(profile), C.byref(opts)))
        if profile.samples * n * 12 > 256 << 20:
            raise PtError(PT_ERR_INVALID, "render_samples: the sample planes would exceed 256 MiB")
        out = np.empty((profile.samples, n, 3), np.float32)
        check_gpu(self.lib.pt_render_samples(self.handle, C.byref(profile), C.byref(opts), out.ctypes.data))
        return out

    def render_denoised_var(self, profile, params, opts=None):
        """pt_render_denoised_var: (rgb8 [H*W, 3] uint8, color [H*W, 3] float32 mean radiance) of the frame filtered with
        its own per-pixel variance."""
        import numpy as np
        n = profile.width * profile.height
        rgb = np.empty((n, 3), np.uint8)
        col = np.empty((n, 3), np.float32)
        check_gpu(self.lib.pt_render_denoised_var(self.handle, C.byref(profile), C.byref(opts) if opts is not None else None,
                                                  C.byref(params) if params is not None else None, rgb.ctypes.data, col.ctypes.data))
        return rgb, col

    def render_aov(self, profile, opts=None, aov_flags=0):
        """pt_render_aov: [n, 16] float32 pixel records (include/ptgpu.h) in the packed local order of render();
        [:, 14].view(np.int32) is the primitive of the first covered sample."""
        import numpy as np
        opts = opts or Opts.make()
        n = int(self.lib.pt_local_pixel_count(C.byref(profile), C.byref(opts)))
        out = np.empty((n, PT_AOV_FLOATS), np.float32)
        check_gpu(self.lib.pt_render_aov(self.handle, C.byref(profile), C.byref(opts), aov_flags, out.ctypes.data))
        return out

    def render_aov_device(self, profile, opts, d_aov, aov_flags=0, stream=0):
        check_gpu(self.lib.pt_render_aov_device(self.handle, C.byref(profile), C.byref(opts) if opts is not None else None,
                                                aov_flags, d_aov, stream))

    def render_aov_samples(self, profile, opts=None, aov_flags=0):
        """pt_render_aov_samples (test hook): [samples, n, 16] float32, the record of every sample of every packed pixel."""
        import numpy as np
        opts = opts or Opts.make()
        n = int(self.lib.pt_local_pixel_count(C.byref(profile), C.byref(opts)))
        if profile.samples * n * 64 > 256 << 20:
            raise PtError(PT_ERR_INVALID, "render_aov_samples: the sample planes would exceed 256 MiB")
        out = np.empty((profile.samples, n, PT_AOV_FLOATS), np.float32)
        check_gpu(self.lib.pt_render_aov_samples(self.handle, C.byref(profile), C.byref(opts), aov_flags, out.ctypes.data))
        return out

    def render_denoised_aov(self, profile, params, variance=False, opts=None, aov_flags=0):
        """pt_render_denoised_aov: render_denoised (variance: render_denoised_var) steered by the guides of the frame's own
        samples (render_aov + aov_guides) instead of the pixel-centre guides."""
        import numpy as np
        n = profile.width * profile.height
        rgb = np.empty((n, 3), np.uint8)
        col = np.empty((n, 3), np.float32)
        check_gpu(self.lib.pt_render_denoised_aov(self.handle, C.byref(profile), C.byref(opts) if opts is not None else None,
                                                  C.byref(params) if params is not None else None, 1 if variance else 0,
                                                  aov_flags, rgb.ctypes.data, col.ctypes.data))
        return rgb, col

    def lightmix_capture(self, profile, opts=None):
        """pt_lightmix_capture: the light-mixer planes of this scene's view for (profile, opts), as a LightMix."""
        handle = C.c_void_p()
        check_gpu(self.lib.pt_lightmix_capture(self.handle, C.byref(profile), C.byref(opts) if opts is not None else None,
                                               C.byref(handle)))
        return LightMix(handle)

    def timing(self):
        t = Timing()
        check_gpu(self.lib.pt_get_timing(self.handle, C.byref(t)))
        return t

    def cull_stats(self):
        """(8x8 pixel blocks, blocks the camera-grid cull found empty) of the last frame; (0, 0): no cull ran."""
        n, e = C.c_uint32(), C.c_uint32()
        check_gpu(self.lib.pt_get_cull_stats(self.handle, C.byref(n), C.byref(e)))
        return n.value, e.value

    def _cache_stats(self, getter, n):
        """The n uint64 values one of the frame caches' getters writes."""
        v = [C.c_uint64() for _ in range(n)]
        check_gpu(getter(self.handle, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def rng_cache_stats(self):
        """The scene's cache of ChaCha words: (device bytes, work items of the keyed enumeration, items cached, fill launches)."""
        return self._cache_stats(self.lib.pt_get_rng_cache_stats, 4)

    def hit_cache_stats(self):
        """The scene's cache of camera hits: (device bytes, work items of the keyed view, items cached, storing launches,
        loading launches)."""
        return self._cache_stats(self.lib.pt_get_hit_cache_stats, 5)

    def vis_cache_stats(self):
        """The scene's cache of bounce-0 shadow visibility: (device bytes, work items of the keyed view and lights, times the
        plane was zeroed, launches of the variant that reads and fills it)."""
        return self._cache_stats(self.lib.pt_get_vis_cache_stats, 4)

    def hit1_cache_stats(self):
        """The scene's cache of bounce-1 hits: (device bytes, work items of the keyed view and materials, items cached so far,
        times the plane was zeroed, storing launches, loading launches, casts the loading launches had no record for).
        Waits for the device."""
        return self._cache_stats(self.lib.pt_get_hit1_cache_stats, 7)

    def hit1_fused_stats(self):
        """The bounce-0 launches that read the cache of bounce-1 hits themselves: (launches, bounce-1 records written with a
        known hit or miss, records elided - the ray is known to miss and the path's colour was final -, records written for
        items without a cached hit).  PT_HIT1_FUSED=0 switches them off.  Waits for the device."""
        return self._cache_stats(self.lib.pt_get_hit1_fused_stats, 4)

    def cont_cache_stats(self):
        """The scene's cache of bounce-0 continuations - the sampled direction and the throughput of the bounce-1 ray: (device
        bytes, work items of the keyed view and materials, items cached, times the planes were zeroed, storing launches,
        loading launches, hit lanes of loading launches that found no record - always 0).  PT_CONT_CACHE=0 switches it off,
        PT_CONT_CACHE_GIB (default 8) is its budget.  Waits for the device."""
        return self._cache_stats(self.lib.pt_get_cont_cache_stats, 7)

    def cont_escape_stats(self):
        """The escape answers in the continuation records (PT_CONT_ESCAPE): (launches that refilled records stored before the
        scene's masks existed, items they went over, loading launches told that the records have answers, lanes of such
        launches that ran the escape test themselves - 0 once the records are refilled).  Waits for the device."""
        return self._cache_stats(self.lib.pt_get_cont_escape_stats, 4)

    def b0_lean_stats(self):
        """The lean variant of the loading bounce-0 launch (PT_B0_LEAN): (lean launches, general launches, frames in which a
        lean launch met a lane it has no code for - always 0).  A configuration goes lean after a planned frame in which every
        bounce-0 launch loaded all its caches and no lane cast, lacked a record or wrote a shadow record; any scene edit,
        re-keyed cache or new masks put it back on the general variant until a frame has been counted clean again."""
        return self._cache_stats(self.lib.pt_get_b0_lean_stats, 3)

    def b1_lean_stats(self):
        """The lean variant of the fused shade pass of bounces 1 and 2 (PT_B1_LEAN): (lean launches at bounce 1, lean launches
        at bounce 2, general fused launches at those bounces, queue entries the lean launches handed to the list pass behind
        them).  A bounce goes lean after a planned frame that sent fewer than 1/64 of that bounce's shaded records to the
        shadow queue; what a lean launch cannot shade the list pass shades, so results never depend on it.  Waits for the
        device."""
        return self._cache_stats(self.lib.pt_get_b1_lean_stats, 4)

    def cont_states(self, count=None):
        """The state words of the first `count` cached continuation records (default: all of them) as a uint32 array: bit 0
        written, bit 1 the record carries the escape test's answer, bit 2 that answer.  Waits for the device."""
        import numpy as np
        n = int(self.cont_cache_stats()[2]) if count is None else int(count)
        out = np.zeros(n, dtype=np.uint32)
        check_gpu(self.lib.pt_scene_cont_states_copy(self.handle, out.ctypes.data_as(C.c_void_p), C.c_uint64(n)))
        return out

    def hit2_cache_stats(self):
        """The scene's cache of bounce-2 hits: the fields of hit1_cache_stats.  Waits for the device."""
        return self._cache_stats(self.lib.pt_get_hit2_cache_stats, 7)

    def vis1_cache_stats(self):
        """The scene's cache of bounce-1 shadow visibility: (device bytes, work items of the keyed view, materials and lights,
        times the plane was zeroed, launches of the shadow kernel that reads and fills it)."""
        return self._cache_stats(self.lib.pt_get_vis1_cache_stats, 4)

    def bounce1_fused_stats(self):
        """The bounce-1 shade launches that read the bounce-1 shadow visibility (and the bounce-2 hits) themselves: (chunks that
        took the kernel, records whose lights it added itself, records it left to the shadow queue, bounce-2 records written
        with a known hit, survivors that got no bounce-2 record - final colour, next cast known to miss -, records written
        for items without a cached hit).  PT_VIS1_FUSED=0 / PT_HIT2_FUSED=0 switch the steps off.  Waits for the device."""
        return self._cache_stats(self.lib.pt_get_bounce1_fused_stats, 6)

    def _bounce_stats(self, getter, bounce, n):
        return self._cache_stats(lambda handle, *out: getter(handle, C.c_uint32(bounce), *out), n)

    def bounce_hits_cache_stats(self, bounce):
        """The scene's cache of the hits of `bounce` (1-5): the fields of hit1_cache_stats.  Bounces 3-5 are switched as a group,
        PT_TAIL_HIT_CACHE=0 / PT_TAIL_HIT_CACHE_GIB (per plane).  Waits for the device."""
        return self._bounce_stats(self.lib.pt_get_bounce_hits_cache_stats, bounce, 7)

    def bounce_vis_cache_stats(self, bounce):
        """The scene's cache of the shadow visibility of `bounce` (1-4): the fields of vis1_cache_stats.  Bounces 2-4 are
        switched as a group, PT_TAIL_VIS_CACHE=0 / PT_TAIL_VIS_CACHE_GIB (per plane)."""
        return self._bounce_stats(self.lib.pt_get_bounce_vis_cache_stats, bounce, 4)

    def bounce_fused_stats(self, bounce):
        """The shade launches of `bounce` (1-4) that read that bounce's shadow visibility themselves: the fields of
        bounce1_fused_stats (the last three are bounce 1's alone).  Bounces 2-4: PT_TAIL_VIS_FUSED=0 switches them off.
        Waits for the device."""
        return self._bounce_stats(self.lib.pt_get_bounce_fused_stats, bounce, 6)

    def counters(self):
        c = Counters()
        check_gpu(self.lib.pt_get_counters(self.handle, C.byref(c)))
        return c

    def trace(self, rays):
        import numpy as np
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros(len(rays), dtype=HIT_DTYPE)
        check_gpu(self.lib.pt_trace_rays(self.handle, rays.ctypes.data, len(rays), out.ctypes.data))
        return out

    def escape_masks(self):
        """(normals [n, 3] (0: no mask), v0 [n, 3], bits [n, 6, 64] bool: True = 'may hit') as the device built them."""
        import numpy as np
        n = int(self.info().n_prims)
        raw = np.zeros((n, 20), np.uint32)
        check_gpu(self.lib.pt_scene_escape_copy(self.handle, raw.ctypes.data, raw.nbytes))
        f = raw.view(np.float32)
        normals, v0 = f[:, 0:3].copy(), np.stack([f[:, 3], f[:, 4], f[:, 5]], axis=1)
        words = raw[:, 8:20].reshape(n, 6, 2)
        bits = ((words[:, :, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(n, 6, 64)
        return normals, v0, bits

    def escape_query(self, prims, rays):
        """bool [n]: does the mask of prims[i] prove that rays[i] (origin3, direction3) hits nothing - the kernels' own lookup
        (escape_proves_miss) run on the device, the height check of the origin included."""
        import numpy as np
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        prims = np.ascontiguousarray(prims, np.uint32).reshape(-1)
        if len(prims) != len(rays):
            raise ValueError("escape_query: one primitive per ray")
        out = np.zeros(len(rays), np.uint8)
        check_gpu(self.lib.pt_escape_query(self.handle, prims.ctypes.data, rays.ctypes.data, len(rays), out.ctypes.data))
        return out.astype(bool)

    def trace_wavefront(self, rays, start_prims=None, mode=0):
        """Closest hits through k_wf_trace itself (mode bit 0: entry lists from start_prims, bit 1: k_wf_trace_wide)."""
        import numpy as np
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros(len(rays), dtype=HIT_DTYPE)
        sp = None if start_prims is None else np.ascontiguousarray(start_prims, np.uint32)
        check_gpu(self.lib.pt_trace_rays_wavefront(self.handle, rays.ctypes.data, None if sp is None else sp.ctypes.data,
                                                   len(rays), mode, out.ctypes.data))
        return out

    def trace_all(self, rays, max_hits=8):
        import numpy as np
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((len(rays), max_hits), dtype=HIT_DTYPE)
        counts = np.zeros(len(rays), np.uint32)
        check_gpu(self.lib.pt_trace_rays_all(self.handle, rays.ctypes.data, len(rays), max_hits,
                                             out.ctypes.data, counts.ctypes.data))
        return out, counts

    def close(self):
        if self.handle:
            self.lib.pt_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


try:
    import numpy as _np
    HIT_DTYPE = _np.dtype([("prim", "<i4"), ("flags", "<i4"), ("dist", "<f4"), ("u", "<f4"), ("v", "<f4")])
except Exception:  # pragma: no cover
    HIT_DTYPE = None


class LightMix:
    """The planes of one captured view (pt_lightmix): E and one difference plane per light.  Owns device memory; outlives the
    scene it was captured from."""

    def __init__(self, handle):
        self.lib = gpu_lib()
        self.handle = handle

    @classmethod
    def from_planes(cls, planes, unit, samples, device=0):
        """pt_lightmix_create_from_planes: planes [n_lights + 1, n_local, 3] float32 (E, then D_l), unit [n_lights]."""
        import numpy as np
        planes = np.ascontiguousarray(planes, np.float32)
        unit = np.ascontiguousarray(unit, np.float32).reshape(-1)
        if planes.ndim != 3 or planes.shape[2] != 3 or planes.shape[0] != len(unit) + 1:
            raise PtError(PT_ERR_INVALID, "LightMix.from_planes: planes must be [n_lights + 1, n_local, 3] for n_lights units")
        handle = C.c_void_p()
        check_gpu(gpu_lib().pt_lightmix_create_from_planes(device, len(unit), samples, planes.shape[1], unit.ctypes.data,
                                                           planes.ctypes.data, C.byref(handle)))
        return cls(handle)

    @property
    def info(self):
        i = LightMixInfo()
        check_gpu(self.lib.pt_lightmix_get_info(self.handle, C.byref(i)))
        return i

    def basis(self, i):
        """Plane i (0: E, 1 + l: D_l) as [n_local, 3] float32."""
        import numpy as np
        out = np.empty((self.info.n_local, 3), np.float32)
        check_gpu(self.lib.pt_lightmix_basis(self.handle, i, out.ctypes.data))
        return out

    @staticmethod
    def _colors(colors):
        import numpy as np
        return np.ascontiguousarray(colors, np.float32).reshape(-1, 3)

    def apply(self, colors, tonemap=None, want_accum=False):
        """pt_lightmix_apply: rgb8 [n_local, 3] uint8 of the view with light colours `colors` [n_lights, 3] (tonemap: a name or
        number, default FILMIC); with want_accum (rgb8, accum [n_local, 3] float32)."""
        import numpy as np
        c = self._colors(colors)
        tm = TONEMAPS["FILMIC"] if tonemap is None else TONEMAPS.get(tonemap, tonemap)
        n = self.info.n_local
        rgb = np.empty((n, 3), np.uint8)
        acc = np.empty((n, 3), np.float32) if want_accum else None
        check_gpu(self.lib.pt_lightmix_apply(self.handle, c.ctypes.data, tm, rgb.ctypes.data, acc.ctypes.data if want_accum else None))
        return (rgb, acc) if want_accum else rgb

    def apply_device(self, colors, tonemap, d_rgb8, d_accum, stream=0):
        """pt_lightmix_apply_device: device pointers (either may be 0 / None), asynchronous on `stream`."""
        c = self._colors(colors)
        tm = TONEMAPS["FILMIC"] if tonemap is None else TONEMAPS.get(tonemap, tonemap)
        check_gpu(self.lib.pt_lightmix_apply_device(self.handle, c.ctypes.data, tm, d_rgb8 or None, d_accum or None, stream))

    def close(self):
        if self.handle:
            self.lib.pt_lightmix_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Film:
    """pt_film: the sum of several whole frames of one view (accum and luminance moments) and the noise figure of its
    moments.  Every pass has at least twice the samples of the pass before it (include/ptgpu.h).  Owns device memory."""

    def __init__(self, profile, opts=None, device=0):
        self.lib = gpu_lib()
        self.handle = C.c_void_p()
        self.tonemap = profile.tonemap if profile is not None else TONEMAPS["FILMIC"]
        check_gpu(self.lib.pt_film_create(device, C.byref(profile) if profile is not None else None,
                                          C.byref(opts) if opts is not None else None, C.byref(self.handle)))

    @classmethod
    def from_planes(cls, accum, moments, samples, last_pass_samples=None, device=0):
        """pt_film_create_from_planes: accum [n_local, 3] and moments [n_local, 2] float32, `samples` their total."""
        import numpy as np
        accum = np.ascontiguousarray(accum, np.float32)
        moments = np.ascontiguousarray(moments, np.float32)
        if accum.ndim != 2 or accum.shape[1] != 3 or moments.shape != (accum.shape[0], 2):
            raise PtError(PT_ERR_INVALID, "Film.from_planes: accum must be [n_local, 3] and moments [n_local, 2]")
        self = cls.__new__(cls)
        self.lib = gpu_lib()
        self.handle = C.c_void_p()
        self.tonemap = TONEMAPS["FILMIC"]
        check_gpu(self.lib.pt_film_create_from_planes(device, accum.shape[0], samples,
                                                      samples if last_pass_samples is None else last_pass_samples,
                                                      accum.ctypes.data, moments.ctypes.data, C.byref(self.handle)))
        return self

    @property
    def info(self):
        i = FilmInfo()
        check_gpu(self.lib.pt_film_get_info(self.handle, C.byref(i)))
        return i

    def add_pass(self, scene, samples):
        """pt_film_add_pass: one more frame of `samples` samples (at least twice the last pass's) of a GpuScene."""
        check_gpu(self.lib.pt_film_add_pass(self.handle, scene.handle, samples))

    def add_planes(self, accum, moments, samples):
        """pt_film_add_planes: a pass rendered elsewhere (pt_render_moments' accum [n_local, 3] and moments [n_local, 2])."""
        import numpy as np
        accum = np.ascontiguousarray(accum, np.float32)
        moments = np.ascontiguousarray(moments, np.float32)
        n = int(self.info.n_local)
        if accum.shape != (n, 3) or moments.shape != (n, 2):
            raise PtError(PT_ERR_INVALID, "Film.add_planes: accum must be [n_local, 3] and moments [n_local, 2]")
        check_gpu(self.lib.pt_film_add_planes(self.handle, samples, accum.ctypes.data, moments.ctypes.data))

    def render_until(self, scene, first, max_samples, target, lum_floor=PT_FILM_DEFAULT_LUM_FLOOR, on_pass=None):
        """pt_film_render_until: passes of first, 2 * first, ... samples until the mean error is <= target or the next pass
        would take the total above max_samples; on_pass(FilmInfo, FilmNoise) after every pass (copies).  Returns the last
        FilmNoise."""
        out = FilmNoise()
        failure = []

        def trampoline(info, noise, _user):
            try:
                on_pass(_copy(FilmInfo, info.contents), _copy(FilmNoise, noise.contents))
            except BaseException as e:   # (an exception cannot cross the C frames: raised after the call)
                failure.append(e)
        cb = FILM_PASS_FN(trampoline) if on_pass is not None else C.cast(None, FILM_PASS_FN)
        check_gpu(self.lib.pt_film_render_until(self.handle, scene.handle, first, max_samples, lum_floor, target, cb, None,
                                                C.byref(out)))
        if failure:
            raise failure[0]
        return out

    def noise(self, target, lum_floor=PT_FILM_DEFAULT_LUM_FLOOR, want_planes=False):
        """pt_film_noise: FilmNoise; with want_planes (FilmNoise, err [n_local], block_sum [n_blocks], block_max [n_blocks])."""
        import numpy as np
        out = FilmNoise()
        if not want_planes:
            check_gpu(self.lib.pt_film_noise(self.handle, lum_floor, target, C.byref(out), None, None, None))
            return out
        n = int(self.info.n_local)
        nb = (n + 255) // 256
        err, bsum, bmax = np.empty(n, np.float32), np.empty(nb, np.float32), np.empty(nb, np.float32)
        check_gpu(self.lib.pt_film_noise(self.handle, lum_floor, target, C.byref(out), err.ctypes.data, bsum.ctypes.data,
                                         bmax.ctypes.data))
        return out, err, bsum, bmax

    def read(self):
        """pt_film_read: (accum [n_local, 3], moments [n_local, 2]) float32."""
        import numpy as np
        n = int(self.info.n_local)
        acc, mom = np.empty((n, 3), np.float32), np.empty((n, 2), np.float32)
        check_gpu(self.lib.pt_film_read(self.handle, acc.ctypes.data, mom.ctypes.data))
        return acc, mom

    def _tonemap(self, tonemap):
        return self.tonemap if tonemap is None else TONEMAPS.get(tonemap, tonemap)

    def resolve(self, tonemap=None, want_color=False):
        """pt_film_resolve: rgb8 [n_local, 3] uint8 (tonemap: a name or number, default the profile's - FILMIC for a film from
        planes); with want_color (rgb8, color [n_local, 3] float32 = accum / samples)."""
        import numpy as np
        n = int(self.info.n_local)
        rgb = np.empty((n, 3), np.uint8)
        col = np.empty((n, 3), np.float32) if want_color else None
        check_gpu(self.lib.pt_film_resolve(self.handle, self._tonemap(tonemap), rgb.ctypes.data,
                                           col.ctypes.data if want_color else None))
        return (rgb, col) if want_color else rgb

    def resolve_device(self, tonemap, d_rgb8, d_color, stream=0):
        """pt_film_resolve_device: device pointers (either may be 0 / None), asynchronous on `stream`."""
        check_gpu(self.lib.pt_film_resolve_device(self.handle, self._tonemap(tonemap), d_rgb8 or None, d_color or None, stream))

    def planes_device(self):
        """pt_film_planes_device: the device addresses (accum, moments) of the film's planes."""
        a, m = C.c_void_p(), C.c_void_p()
        check_gpu(self.lib.pt_film_planes_device(self.handle, C.byref(a), C.byref(m)))
        return a.value, m.value

    def kernel_times(self, lum_floor=PT_FILM_DEFAULT_LUM_FLOOR, with_err=False, reps=20):
        """pt_film_kernel_times: (ms of k_film_merge [reps], ms of k_film_noise [reps])."""
        import numpy as np
        a, b = np.zeros(reps, np.float32), np.zeros(reps, np.float32)
        check_gpu(self.lib.pt_film_kernel_times(self.handle, lum_floor, int(with_err), reps, a.ctypes.data, b.ctypes.data))
        return a, b

    def reset(self):
        check_gpu(self.lib.pt_film_reset(self.handle))

    # ---- the adaptive film
    def add_tile_pass(self, scene, samples, tiles):
        """pt_film_add_tile_pass: a pass of `samples` samples over the listed tiles (global numbers, strictly ascending)."""
        t = _tile_list(tiles)
        check_gpu(self.lib.pt_film_add_tile_pass(self.handle, scene.handle, samples, t.ctypes.data, len(t)))

    def add_tile_planes(self, accum, moments, samples, tiles):
        """pt_film_add_tile_planes: a tile pass rendered elsewhere (GpuScene.render_tiles' packed accum and moments)."""
        import numpy as np
        t = _tile_list(tiles)
        accum = np.ascontiguousarray(accum, np.float32)
        moments = np.ascontiguousarray(moments, np.float32)
        if accum.ndim != 2 or accum.shape[1] != 3 or moments.shape != (accum.shape[0], 2):
            raise PtError(PT_ERR_INVALID, "Film.add_tile_planes: accum must be [n, 3] and moments [n, 2]")
        check_gpu(self.lib.pt_film_add_tile_planes(self.handle, samples, t.ctypes.data, len(t), accum.ctypes.data,
                                                   moments.ctypes.data))

    def read_counts(self):
        """pt_film_read_counts: every pixel's sample count [n_local] uint32."""
        import numpy as np
        counts = np.empty(int(self.info.n_local), np.uint32)
        check_gpu(self.lib.pt_film_read_counts(self.handle, counts.ctypes.data))
        return counts

    @property
    def adaptive_info(self):
        i = FilmAdaptiveInfo()
        check_gpu(self.lib.pt_film_get_adaptive_info(self.handle, C.byref(i)))
        return i

    def tile_noise(self, target, lum_floor=PT_FILM_DEFAULT_LUM_FLOOR, want_planes=False):
        """pt_film_tile_noise: FilmTileStats; with want_planes (FilmTileStats, err [n_local], tile_sum [n_tiles],
        tile_max [n_tiles])."""
        import numpy as np
        out = FilmTileStats()
        if not want_planes:
            check_gpu(self.lib.pt_film_tile_noise(self.handle, lum_floor, target, C.byref(out), None, None, None))
            return out
        n, nt = int(self.info.n_local), int(self.adaptive_info.n_tiles)
        err, tsum, tmax = np.empty(n, np.float32), np.empty(nt, np.float32), np.empty(nt, np.float32)
        check_gpu(self.lib.pt_film_tile_noise(self.handle, lum_floor, target, C.byref(out), err.ctypes.data, tsum.ctypes.data,
                                              tmax.ctypes.data))
        return out, err, tsum, tmax

    def render_until_adaptive(self, scene, params, on_pass=None):
        """pt_film_render_until_adaptive: doubling passes, the later ones over the tiles that are still above the target;
        on_pass(FilmInfo, FilmNoise) after every pass (copies).  Returns the last FilmTileStats."""
        out = FilmTileStats()
        failure = []

        def trampoline(info, noise, _user):
            try:
                on_pass(_copy(FilmInfo, info.contents), _copy(FilmNoise, noise.contents))
            except BaseException as e:   # (an exception cannot cross the C frames: raised after the call)
                failure.append(e)
        cb = FILM_PASS_FN(trampoline) if on_pass is not None else C.cast(None, FILM_PASS_FN)
        check_gpu(self.lib.pt_film_render_until_adaptive(self.handle, scene.handle, C.byref(params), cb, None, C.byref(out)))
        if failure:
            raise failure[0]
        return out

    def adaptive_kernel_times(self, lum_floor=PT_FILM_DEFAULT_LUM_FLOOR, tonemap=None, reps=20):
        """pt_film_adaptive_kernel_times: ms of (k_film_merge_tiles, k_film_tile_noise, k_film_post_counts), [reps] each."""
        import numpy as np
        a, b, c = (np.zeros(reps, np.float32) for _ in range(3))
        check_gpu(self.lib.pt_film_adaptive_kernel_times(self.handle, lum_floor, self._tonemap(tonemap), reps, a.ctypes.data,
                                                         b.ctypes.data, c.ctypes.data))
        return a, b, c

    # ---- windowed films
    @classmethod
    def windowed(cls, profile, opts=None, device=0):
        """pt_film_create_windowed: a film whose passes are windows of ONE enumeration of profile.samples samples."""
        self = cls.__new__(cls)
        self.lib = gpu_lib()
        self.handle = C.c_void_p()
        self.tonemap = profile.tonemap if profile is not None else TONEMAPS["FILMIC"]
        check_gpu(self.lib.pt_film_create_windowed(device, C.byref(profile) if profile is not None else None,
                                                   C.byref(opts) if opts is not None else None, C.byref(self.handle)))
        return self

    def add_window(self, scene, samples):
        """pt_film_add_window: the next `samples` samples of the enumeration, for every pixel."""
        check_gpu(self.lib.pt_film_add_window(self.handle, scene.handle, samples))

    def add_tile_window(self, scene, samples, tiles):
        """pt_film_add_tile_window: the next `samples` samples of every listed tile, each from its own count."""
        t = _tile_list(tiles)
        check_gpu(self.lib.pt_film_add_tile_window(self.handle, scene.handle, samples, t.ctypes.data, len(t)))

    @property
    def window_info(self):
        i = FilmWindowInfo()
        check_gpu(self.lib.pt_film_get_window_info(self.handle, C.byref(i)))
        return i

    def render_until_windowed(self, scene, params, on_pass=None):
        """pt_film_render_until_windowed: windows of params.window_samples samples until no tile is above the target or the
        active tiles hold the whole enumeration; on_pass(FilmInfo, FilmNoise) after every window (copies).  Returns the last
        FilmTileStats."""
        out = FilmTileStats()
        failure = []

        def trampoline(info, noise, _user):
            try:
                on_pass(_copy(FilmInfo, info.contents), _copy(FilmNoise, noise.contents))
            except BaseException as e:   # (an exception cannot cross the C frames: raised after the call)
                failure.append(e)
        cb = FILM_PASS_FN(trampoline) if on_pass is not None else C.cast(None, FILM_PASS_FN)
        check_gpu(self.lib.pt_film_render_until_windowed(self.handle, scene.handle, C.byref(params), cb, None, C.byref(out)))
        if failure:
            raise failure[0]
        return out

    def window_kernel_times(self, reps=20):
        """pt_film_window_kernel_times: ms of (k_film_gather_tiles, k_film_scatter_tiles) over every tile, [reps] each."""
        import numpy as np
        a, b = np.zeros(reps, np.float32), np.zeros(reps, np.float32)
        check_gpu(self.lib.pt_film_window_kernel_times(self.handle, reps, a.ctypes.data, b.ctypes.data))
        return a, b

    # ---- sharded films
    @classmethod
    def shard(cls, profile, opts, windowed=False, device=0):
        """pt_film_create_shard: the part of rank opts.shard_rank of a film that opts.shard_count ranks hold together
        (windowed: a window film of profile.samples)."""
        self = cls.__new__(cls)
        self.lib = gpu_lib()
        self.handle = C.c_void_p()
        self.tonemap = profile.tonemap if profile is not None else TONEMAPS["FILMIC"]
        check_gpu(self.lib.pt_film_create_shard(device, C.byref(profile) if profile is not None else None,
                                                C.byref(opts) if opts is not None else None, int(windowed), C.byref(self.handle)))
        return self

    @property
    def shard_info(self):
        i = FilmShardInfo()
        check_gpu(self.lib.pt_film_get_shard_info(self.handle, C.byref(i)))
        return i

    def shard_tile_noise(self, lum_floor=PT_FILM_DEFAULT_LUM_FLOOR, want_err=False):
        """pt_film_shard_tile_noise: (tile_sum [n_tiles], tile_max [n_tiles]) of the image's tiles, 0 for other ranks' tiles;
        with want_err (tile_sum, tile_max, err [n_local] in packed local order)."""
        import numpy as np
        nt = int(self.shard_info.n_tiles)
        tsum, tmax = np.empty(nt, np.float32), np.empty(nt, np.float32)
        err = np.empty(int(self.info.n_local), np.float32) if want_err else None
        check_gpu(self.lib.pt_film_shard_tile_noise(self.handle, lum_floor, tsum.ctypes.data, tmax.ctypes.data,
                                                    err.ctypes.data if want_err else None))
        return (tsum, tmax, err) if want_err else (tsum, tmax)

    def tile_stats_from_sums(self, tile_sum, target):
        """pt_film_tile_stats_from_sums: FilmTileStats of a complete tile_sum array [n_tiles]."""
        import numpy as np
        tile_sum = np.ascontiguousarray(tile_sum, np.float32)
        if tile_sum.shape != (int(self.shard_info.n_tiles),):
            raise PtError(PT_ERR_INVALID, "Film.tile_stats_from_sums: tile_sum must be [n_tiles]")
        out = FilmTileStats()
        check_gpu(self.lib.pt_film_tile_stats_from_sums(self.handle, tile_sum.ctypes.data, target, C.byref(out)))
        return out

    def select_tiles(self, tile_sum, target, dilate=1):
        """pt_film_select_tiles: the tiles above the target (dilate: and their 8 neighbours), ascending, uint32."""
        import numpy as np
        tile_sum = np.ascontiguousarray(tile_sum, np.float32)
        nt = int(self.shard_info.n_tiles)
        if tile_sum.shape != (nt,):
            raise PtError(PT_ERR_INVALID, "Film.select_tiles: tile_sum must be [n_tiles]")
        tiles, n = np.empty(nt, np.uint32), C.c_uint32()
        check_gpu(self.lib.pt_film_select_tiles(self.handle, tile_sum.ctypes.data, target, dilate, tiles.ctypes.data, C.byref(n)))
        return tiles[:n.value].copy()

    def _render_until_sharded(self, fn, scene, params, exchange, on_pass):
        import numpy as np
        out = FilmTileStats()
        failure = []

        def trampoline(info, noise, _user):
            try:
                on_pass(_copy(FilmInfo, info.contents), _copy(FilmNoise, noise.contents))
            except BaseException as e:   # (an exception cannot cross the C frames: raised after the call)
                failure.append(e)

        def exchange_trampoline(tile_sum, tile_max, n_tiles, _user):
            try:   # the callback works on the two arrays in place; its return value is the C callback's (None: 0)
                rc = exchange(np.ctypeslib.as_array(tile_sum, (n_tiles,)), np.ctypeslib.as_array(tile_max, (n_tiles,)))
                return int(rc or 0)
            except BaseException as e:
                failure.append(e)
                return -1
        if isinstance(exchange, tuple):   # (a C callback and its user pointer, e.g. (lib.pt_film_exchange_comm, comm.handle))
            ex, ex_user = C.cast(exchange[0], FILM_EXCHANGE_FN), exchange[1]
        else:
            ex = FILM_EXCHANGE_FN(exchange_trampoline) if exchange is not None else C.cast(None, FILM_EXCHANGE_FN)
            ex_user = None
        cb = FILM_PASS_FN(trampoline) if on_pass is not None else C.cast(None, FILM_PASS_FN)
        rc = fn(self.handle, scene.handle, C.byref(params), ex, ex_user, cb, None, C.byref(out))
        if failure:
            raise failure[0]
        check_gpu(rc)
        return out

    def render_until_adaptive_sharded(self, scene, params, exchange=None, on_pass=None):
        """pt_film_render_until_adaptive_sharded on a shard film.  exchange(tile_sum, tile_max): a blocking collective over
        the ranks that combines the two float32 arrays in place and returns 0 (or None), non-zero to end the loop with
        PT_ERR_DEVICE; or a tuple (C function, user pointer); None: one rank.  Returns the last FilmTileStats."""
        return self._render_until_sharded(self.lib.pt_film_render_until_adaptive_sharded, scene, params, exchange, on_pass)

    def render_until_windowed_sharded(self, scene, params, exchange=None, on_pass=None):
        """pt_film_render_until_windowed_sharded on a windowed shard film; the arguments of render_until_adaptive_sharded."""
        return self._render_until_sharded(self.lib.pt_film_render_until_windowed_sharded, scene, params, exchange, on_pass)

    def assemble(self, shards):
        """pt_film_assemble: this empty unsharded film becomes the whole film of the shard films `shards` (every rank once)."""
        handles = (C.c_void_p * len(shards))(*[f.handle for f in shards])
        check_gpu(self.lib.pt_film_assemble(self.handle, handles, len(shards)))

    # ---- the film filter
    def denoise_scratch_bytes(self):
        return int(self.lib.pt_film_denoise_scratch_bytes(self.handle))

    def denoise(self, scene, params, variance=True, lum_floor=PT_FILM_DEFAULT_LUM_FLOOR, want_ferr=False):
        """pt_film_denoise: the a-trous filter (variance-guided, or plain) on the film's planes with guides rendered from a
        GpuScene; (color [n_local, 3] float32, rgb8 [n_local, 3] uint8), with want_ferr (variance only) also ferr [n_local]."""
        import numpy as np
        n = int(self.info.n_local)
        col, rgb = np.empty((n, 3), np.float32), np.empty((n, 3), np.uint8)
        ferr = np.empty(n, np.float32) if want_ferr else None
        check_gpu(self.lib.pt_film_denoise(self.handle, scene.handle, int(variance), C.byref(params), lum_floor, rgb.ctypes.data,
                                           col.ctypes.data, ferr.ctypes.data if want_ferr else None))
        return (col, rgb, ferr) if want_ferr else (col, rgb)

    def denoise_device(self, params, variance, d_guides, d_color, d_rgb8, d_ferr, d_scratch, lum_floor=PT_FILM_DEFAULT_LUM_FLOOR,
                       stream=0):
        """pt_film_denoise_device: device pointers (outputs may be 0 / None, not all), asynchronous on `stream`."""
        check_gpu(self.lib.pt_film_denoise_device(self.handle, int(variance), C.byref(params), lum_floor, d_guides, d_color or None,
                                                  d_rgb8 or None, d_ferr or None, d_scratch or None, stream))

    def tile_reduce_device(self, d_err, d_tile_sum, d_tile_max, stream=0):
        """pt_film_tile_reduce_device: the tile sums and maxima of an error plane on the device."""
        check_gpu(self.lib.pt_film_tile_reduce_device(self.handle, d_err, d_tile_sum, d_tile_max, stream))

    def filtered_noise(self, scene, params, target, lum_floor=PT_FILM_DEFAULT_LUM_FLOOR, want_planes=False):
        """pt_film_filtered_noise: FilmTileStats of the filtered image's error; with want_planes (FilmTileStats,
        ferr [n_local], tile_sum [n_tiles], tile_max [n_tiles])."""
        import numpy as np
        out = FilmTileStats()
        if not want_planes:
            check_gpu(self.lib.pt_film_filtered_noise(self.handle, scene.handle, C.byref(params), lum_floor, target, C.byref(out),
                                                      None, None, None))
            return out
        n, nt = int(self.info.n_local), int(self.adaptive_info.n_tiles)
        ferr, tsum, tmax = np.empty(n, np.float32), np.empty(nt, np.float32), np.empty(nt, np.float32)
        check_gpu(self.lib.pt_film_filtered_noise(self.handle, scene.handle, C.byref(params), lum_floor, target, C.byref(out),
                                                  ferr.ctypes.data, tsum.ctypes.data, tmax.ctypes.data))
        return out, ferr, tsum, tmax

    def render_until_filtered(self, scene, params, on_pass=None):
        """pt_film_render_until_filtered: render_until_adaptive with the tiles selected by the error of the filtered image
        (params: FilmFilteredParams); on_pass(FilmInfo, FilmNoise) after every pass.  Returns the last FilmTileStats."""
        out = FilmTileStats()
        failure = []

        def trampoline(info, noise, _user):
            try:
                on_pass(_copy(FilmInfo, info.contents), _copy(FilmNoise, noise.contents))
            except BaseException as e:   # (an exception cannot cross the C frames: raised after the call)
                failure.append(e)
        cb = FILM_PASS_FN(trampoline) if on_pass is not None else C.cast(None, FILM_PASS_FN)
        check_gpu(self.lib.pt_film_render_until_filtered(self.handle, scene.handle, C.byref(params), cb, None, C.byref(out)))
        if failure:
            raise failure[0]
        return out

    def denoise_kernel_times(self, scene, params, lum_floor=PT_FILM_DEFAULT_LUM_FLOOR, reps=20):
        """pt_film_denoise_kernel_times: ms of (prep, all passes, finish + ferr, tile reduce), [reps] each."""
        import numpy as np
        t = [np.zeros(reps, np.float32) for _ in range(4)]
        check_gpu(self.lib.pt_film_denoise_kernel_times(self.handle, scene.handle, C.byref(params), lum_floor, reps,
                                                        *(a.ctypes.data for a in t)))
        return tuple(t)

    def close(self):
        if self.handle:
            self.lib.pt_film_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class History:
    """pt_history: the sample sums of a camera path's frames, carried from view to view by projecting every pixel's AOV
    surface point into the previous camera (include/ptgpu.h).  For a static scene; owns device memory."""

    def __init__(self, width, height, params=None, device=0):
        self.lib = gpu_lib()
        self.handle = C.c_void_p()
        self.width, self.height = int(width), int(height)
        params = HistoryParams.default() if params is None else params
        check_gpu(self.lib.pt_history_create(device, width, height, C.byref(params), C.byref(self.handle)))

    @property
    def info(self):
        i = HistoryInfo()
        check_gpu(self.lib.pt_history_get_info(self.handle, C.byref(i)))
        return i

    def view(self, which):
        """pt_history_get_view: the HistoryView of the previous (0) or the current (1) camera."""
        v = HistoryView()
        check_gpu(self.lib.pt_history_get_view(self.handle, which, C.byref(v)))
        return v

    def reset(self):
        check_gpu(self.lib.pt_history_reset(self.handle))

    def advance(self, camera, samples, accum, moments, aov, want_map=False):
        """pt_history_advance: a frame of `samples` samples rendered from `camera` (GpuScene.render_moments' accum [n, 3] and
        moments [n, 2], GpuScene.render_aov's records [n, 16]) joins the history; with want_map the int32 map [n]."""
        import numpy as np
        n = self.width * self.height
        accum = np.ascontiguousarray(accum, np.float32)
        moments = np.ascontiguousarray(moments, np.float32)
        aov = np.ascontiguousarray(aov, np.float32)
        if accum.size != n * 3 or moments.size != n * 2 or aov.size != n * PT_AOV_FLOATS:
            raise PtError(PT_ERR_INVALID, "History.advance: accum must be [n, 3], moments [n, 2] and aov [n, 16]")
        cam = make_camera(camera)
        hmap = np.empty(n, np.int32) if want_map else None
        check_gpu(self.lib.pt_history_advance(self.handle, C.byref(cam) if cam is not None else None, samples, accum.ctypes.data,
                                              moments.ctypes.data, aov.ctypes.data, hmap.ctypes.data if want_map else None))
        return hmap

    def advance_device(self, camera, samples, d_accum, d_moments, d_aov, d_map=None, stream=0):
        """pt_history_advance_device: device pointers (d_map may be 0 / None), asynchronous on `stream`."""
        cam = make_camera(camera)
        check_gpu(self.lib.pt_history_advance_device(self.handle, C.byref(cam) if cam is not None else None, samples, d_accum,
                                                     d_moments, d_aov, d_map or None, stream))

    def add_frame(self, scene, profile, frame_index, opts=None):
        """pt_history_add_frame: render the GpuScene's current view (profile.samples samples, the window frame_index % rotate
        of the longer enumeration) with its AOV records and advance."""
        check_gpu(self.lib.pt_history_add_frame(self.handle, scene.handle, C.byref(profile),
                                                C.byref(opts) if opts is not None else None, frame_index))

    def read(self):
        """pt_history_read: (accum [n, 3], moments [n, 2], counts [n] uint32, surf [n, 8], guides [n, 8])."""
        import numpy as np
        n = self.width * self.height
        acc, mom, cnt = np.empty((n, 3), np.float32), np.empty((n, 2), np.float32), np.empty(n, np.uint32)
        surf, guides = np.empty((n, 8), np.float32), np.empty((n, PT_GUIDE_FLOATS), np.float32)
        check_gpu(self.lib.pt_history_read(self.handle, acc.ctypes.data, mom.ctypes.data, cnt.ctypes.data, surf.ctypes.data,
                                           guides.ctypes.data, None))
        return acc, mom, cnt, surf, guides

    def read_map(self):
        """The int32 map [n] of the last add_frame (include/ptgpu.h: a source pixel, or -1 .. -6)."""
        import numpy as np
        hmap = np.empty(self.width * self.height, np.int32)
        check_gpu(self.lib.pt_history_read(self.handle, None, None, None, None, None, hmap.ctypes.data))
        return hmap

    def resolve(self, tonemap="FILMIC"):
        """pt_history_resolve: (rgb8 [n, 3] uint8, color [n, 3] float32 = accum / count)."""
        import numpy as np
        n = self.width * self.height
        rgb, col = np.empty((n, 3), np.uint8), np.empty((n, 3), np.float32)
        check_gpu(self.lib.pt_history_resolve(self.handle, TONEMAPS.get(tonemap, tonemap), rgb.ctypes.data, col.ctypes.data))
        return rgb, col

    def resolve_device(self, tonemap, d_rgb8, d_color, stream=0):
        """pt_history_resolve_device: device pointers (either may be 0 / None), asynchronous on `stream`."""
        check_gpu(self.lib.pt_history_resolve_device(self.handle, TONEMAPS.get(tonemap, tonemap), d_rgb8 or None, d_color or None,
                                                     stream))

    def denoise(self, params, variance=True, lum_floor=PT_FILM_DEFAULT_LUM_FLOOR):
        """pt_history_denoise: the film filter on the history's planes, counts and guides; (color [n, 3], rgb8 [n, 3])."""
        import numpy as np
        n = self.width * self.height
        col, rgb = np.empty((n, 3), np.float32), np.empty((n, 3), np.uint8)
        check_gpu(self.lib.pt_history_denoise(self.handle, int(variance), C.byref(params) if params is not None else None,
                                              lum_floor, rgb.ctypes.data, col.ctypes.data))
        return col, rgb

    def denoise_device(self, params, variance, d_rgb8, d_color, lum_floor=PT_FILM_DEFAULT_LUM_FLOOR, stream=0):
        """pt_history_denoise_device: device pointers (either may be 0 / None), asynchronous on `stream`."""
        check_gpu(self.lib.pt_history_denoise_device(self.handle, int(variance), C.byref(params), lum_floor, d_rgb8 or None,
                                                     d_color or None, stream))

    def kernel_times(self, reps=20):
        """pt_history_kernel_times: ms of k_hist_advance, [reps]."""
        import numpy as np
        t = np.zeros(reps, np.float32)
        check_gpu(self.lib.pt_history_kernel_times(self.handle, reps, t.ctypes.data))
        return t

    def close(self):
        if self.handle:
            self.lib.pt_history_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def denoise(width, height, samples, params, accum, guides, device=0):
    """pt_denoise on host arrays: accum [H*W, 3] float32 SUM of samples, guides [H*W, 8] float32 (GpuScene.render_guides);
    returns (color [H*W, 3] float32 mean radiance, rgb8 [H*W, 3] uint8)."""
    import numpy as np
    n = width * height
    accum = np.ascontiguousarray(accum, np.float32)
    guides = np.ascontiguousarray(guides, np.float32)
    if accum.size != n * 3 or guides.size != n * PT_GUIDE_FLOATS:
        raise ValueError("denoise: accum must hold width*height*3 and guides width*height*8 floats")
    col = np.empty((n, 3), np.float32)
    rgb = np.empty((n, 3), np.uint8)
    check_gpu(gpu_lib().pt_denoise(device, width, height, samples, C.byref(params) if params is not None else None,
                                   accum.ctypes.data, guides.ctypes.data, col.ctypes.data, rgb.ctypes.data))
    return col, rgb


def denoise_scratch_bytes(width, height):
    return int(gpu_lib().pt_denoise_scratch_bytes(width, height))


def denoise_var(width, height, samples, params, accum, moments, guides, device=0):
    """pt_denoise_var on host arrays: denoise() plus moments [H*W, 2] float32 (GpuScene.render_moments); returns
    (color [H*W, 3] float32 mean radiance, rgb8 [H*W, 3] uint8)."""
    import numpy as np
    n = width * height
    accum = np.ascontiguousarray(accum, np.float32)
    moments = np.ascontiguousarray(moments, np.float32)
    guides = np.ascontiguousarray(guides, np.float32)
    if accum.size != n * 3 or moments.size != n * 2 or guides.size != n * PT_GUIDE_FLOATS:
        raise ValueError("denoise_var: accum must hold width*height*3, moments width*height*2 and guides width*height*8 floats")
    col = np.empty((n, 3), np.float32)
    rgb = np.empty((n, 3), np.uint8)
    check_gpu(gpu_lib().pt_denoise_var(device, width, height, samples, C.byref(params) if params is not None else None,
                                       accum.ctypes.data, moments.ctypes.data, guides.ctypes.data, col.ctypes.data,
                                       rgb.ctypes.data))
    return col, rgb


def aov_guides(samples, aov, device=0):
    """pt_aov_guides on host arrays: aov [n, 16] float32 pixel records of a frame of `samples` samples (GpuScene.render_aov);
    returns guides [n, 8] float32 in the layout of GpuScene.render_guides."""
    import numpy as np
    aov = np.ascontiguousarray(aov, np.float32)
    if aov.size == 0 or aov.size % PT_AOV_FLOATS:
        raise ValueError("aov_guides: aov must hold n * 16 floats")
    n = aov.size // PT_AOV_FLOATS
    guides = np.empty((n, PT_GUIDE_FLOATS), np.float32)
    check_gpu(gpu_lib().pt_aov_guides(device, n, samples, aov.ctypes.data, guides.ctypes.data))
    return guides


def denoise_var_scratch_bytes(width, height):
    return int(gpu_lib().pt_denoise_var_scratch_bytes(width, height))


def _tile_list(tiles):
    import numpy as np
    return np.ascontiguousarray(tiles, np.uint32).reshape(-1)


def tiles_pixel_count(profile, tiles, opts=None):
    """pt_tiles_pixel_count: packed pixels of a tile list (0: a list or options that are refused)."""
    opts = opts or Opts.make()
    t = _tile_list(tiles)
    return int(gpu_lib().pt_tiles_pixel_count(C.byref(profile), C.byref(opts), t.ctypes.data, len(t)))


def tiles_pixel_map(profile, tiles, opts=None):
    """pt_tiles_pixel_map: the global pixel index of every packed pixel of a tile list (no GPU needed)."""
    import numpy as np
    opts = opts or Opts.make()
    t = _tile_list(tiles)
    lib = gpu_lib()
    out = np.empty(int(lib.pt_tiles_pixel_count(C.byref(profile), C.byref(opts), t.ctypes.data, len(t))), np.uint32)
    check_gpu(lib.pt_tiles_pixel_map(C.byref(profile), C.byref(opts), t.ctypes.data, len(t), out.ctypes.data))
    return out


def local_pixel_map(profile, opts):
    import numpy as np
    lib = gpu_lib()
    n = int(lib.pt_local_pixel_count(C.byref(profile), C.byref(opts)))
    out = np.empty(n, np.uint32)
    check_gpu(lib.pt_local_pixel_map(C.byref(profile), C.byref(opts), out.ctypes.data))
    return out


def measure_copy_bandwidth(device=0, nbytes=1 << 30, reps=5):
    """GB/s (read + write) of a plain device copy kernel: the achievable-HBM yardstick."""
    out = C.c_double(0.0)
    check_gpu(gpu_lib().pt_measure_copy_bandwidth(device, nbytes, reps, C.byref(out)))
    return out.value


def measure_gather_rate(device=0, table_bytes=32 << 20, bytes_per_load=8, loads_per_lane=512):
    """1e9 scattered lane-loads per second (the KD walk's access pattern): the ceiling the traversal kernels see."""
    out = C.c_double(0.0)
    check_gpu(gpu_lib().pt_measure_gather_rate(device, table_bytes, bytes_per_load, loads_per_lane, C.byref(out)))
    return out.value
