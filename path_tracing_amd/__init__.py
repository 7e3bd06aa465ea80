"""path_tracing_amd -- MI355X-native unidirectional path-tracing hot path.

Python front-end of the C ABI in include/hpt.h (libhpt.so: hand-written HIP kernels for
gfx950 + host BVH build).  Mirrors the reference's launch-and-accumulate helper API
(reference include/pt_cu_helper.h:5-6, src/pt_cu_helper.cpp:12-77):

    Scene(lights, spheres, triangles)      ~ move_data_to_cuda_pt (upload once)
    Scene.render_pt(cam, W, H, depth, spp) ~ run_cuda_pt / pt_render_wrapper

There is no CPU fallback: if libhpt.so is missing or no HIP device is visible, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import layouts, scene_io  # noqa: F401
from .layouts import CAMERA, LIGHT, SPHERE, TRIANGLE

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libhpt.so")

FLAG_BRUTE_FORCE = 1
FLAG_COUNT_WORK = 2
FLAG_OUTPUT_SUM = 4
FLAG_TIME_KERNELS = 8
FLAG_RUSSIAN_ROULETTE = 16
FLAG_SINGLE_PIPELINE = 32
FLAG_NO_HOST_WAIT = 64
DENOISE_DEMODULATE = 1
DENOISE_TIME = 2
ACCUM_MOMENTS = 1
DISPLAY_BGR = 1
DISPLAY_FLIP_Y = 2
HISTORY_MOMENTS = 1


class HptError(RuntimeError):
    pass


class Params(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("sample_offset", C.c_int32), ("max_delta", C.c_int32),
                ("rank", C.c_int32), ("world", C.c_int32), ("tile", C.c_int32),
                ("samples_per_pass", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("closest_rays", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("boxes_closest", C.c_uint64), ("tris_closest", C.c_uint64),
                ("boxes_shadow", C.c_uint64), ("tris_shadow", C.c_uint64), ("path_iters", C.c_uint64),
                ("ms_total", C.c_double), ("ms_extend", C.c_double), ("ms_shade", C.c_double),
                ("ms_connect", C.c_double), ("ms_other", C.c_double),
                ("n_extend", C.c_uint32), ("n_shade", C.c_uint32), ("n_connect", C.c_uint32), ("n_other", C.c_uint32),
                ("bvh_nodes", C.c_uint32), ("bvh_depth", C.c_uint32), ("n_tris", C.c_uint32), ("n_materials", C.c_uint32),
                ("ms_bvh_build", C.c_double), ("ms_upload", C.c_double),
                ("lane_steps_closest", C.c_uint64), ("wave_steps_closest", C.c_uint64),
                ("lane_steps_shadow", C.c_uint64), ("wave_steps_shadow", C.c_uint64),
                ("leaf_lane_closest", C.c_uint64), ("leaf_wave_closest", C.c_uint64),
                ("leaf_lane_shadow", C.c_uint64), ("leaf_wave_shadow", C.c_uint64),
                ("ms_resume", C.c_double), ("n_resume", C.c_uint32), ("split_budget", C.c_uint32),
                ("traced_rays_last_pass", C.c_uint64), ("long_rays_last_pass", C.c_uint64),
                ("bd_pairs", C.c_uint64), ("bd_survivors", C.c_uint64), ("bd_shadow_rays", C.c_uint64), ("bd_unoccluded", C.c_uint64),
                ("bd_nodes", C.c_uint64), ("bd_tris", C.c_uint64), ("bd_spheres", C.c_uint64), ("bd_group_boxes", C.c_uint64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class PpmStats(C.Structure):
    """hpt_ppm_stats (include/hpt.h): counts and phase times of the last photon-mapping render."""
    _fields_ = [(n, C.c_uint64) for n in ("photons", "photon_rays", "deposits", "hit_points", "direct_pixels", "candidates", "accepted",
                                          "cand_median", "cand_max", "acc_median", "acc_max", "grid_buckets")] + \
               [(n, C.c_double) for n in ("ms_eye", "ms_photon", "ms_grid", "ms_gather", "ms_total")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class DenoiseParams(C.Structure):
    """hpt_denoise_params (include/hpt.h): zeros select the defaults (5 levels, sigmas 1.0 / 0.5 / 0.05); a negative
    sigma switches its term off."""
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_position", C.c_float), ("flags", C.c_int32)]


class GuidedParams(C.Structure):
    """hpt_guided_params (include/hpt.h): zeros select the defaults (5 levels, sigmas 2.0 / 0.5 / 0.05); sigma_color is in
    standard deviations of the pixel's own noise and is not halved per level; a negative sigma switches its term off."""
    _fields_ = [("iterations", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_position", C.c_float), ("flags", C.c_int32)]


class HistoryParams(C.Structure):
    """hpt_history_params (include/hpt.h): zeros select the defaults (max_history 256, plane_tolerance 0.01, normal_min
    0.9); a negative tolerance or a normal_min below -1 switches its test off."""
    _fields_ = [("max_history", C.c_float), ("plane_tolerance", C.c_float), ("normal_min", C.c_float), ("flags", C.c_int32)]


def make_history_params(max_history=0.0, plane_tolerance=0.0, normal_min=0.0) -> HistoryParams:
    return HistoryParams(float(max_history), float(plane_tolerance), float(normal_min), 0)


def make_denoise_params(iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0, demodulate=True, time=False) -> DenoiseParams:
    return DenoiseParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_position),
                         (DENOISE_DEMODULATE if demodulate else 0) | (DENOISE_TIME if time else 0))


def make_guided_params(iterations=0, sigma_color=0.0, sigma_normal=0.0, sigma_position=0.0, demodulate=True, time=False) -> GuidedParams:
    return GuidedParams(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_position),
                        (DENOISE_DEMODULATE if demodulate else 0) | (DENOISE_TIME if time else 0))


class BvhInfo(C.Structure):
    _fields_ = [("num_nodes", C.c_int32), ("num_tris", C.c_int32), ("bvh_depth", C.c_int32), ("num_rounds", C.c_int32),
                ("qorigin", C.c_float * 3), ("qscale", C.c_float * 3)]


class UpdateInfo(C.Structure):
    _fields_ = [("updates", C.c_uint64), ("live_tris", C.c_uint64), ("dead_tris", C.c_uint64),
                ("ms_pack", C.c_double), ("ms_upload", C.c_double), ("ms_refit", C.c_double)]


class TreeCost(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("inner_children", "leaf_children", "empty_children", "leaf_slots", "inner_xy", "inner_yz",
                                          "inner_zx", "leaf_xy", "leaf_yz", "leaf_zx")] + \
               [("root_extent", C.c_uint32 * 3), ("num_nodes", C.c_uint32),
                ("box_visits", C.c_double), ("tri_tests", C.c_double), ("sah", C.c_double)]


class RebuildInfo(C.Structure):
    _fields_ = [("rebuilds", C.c_uint64), ("nodes_before", C.c_uint32), ("nodes_after", C.c_uint32),
                ("depth_before", C.c_uint32), ("depth_after", C.c_uint32),
                ("ms_download", C.c_double), ("ms_build", C.c_double), ("ms_upload", C.c_double)]


class DeviceBuildInfo(C.Structure):
    _fields_ = [("builds", C.c_uint64), ("fell_back", C.c_uint32), ("nodes_before", C.c_uint32), ("nodes_after", C.c_uint32),
                ("depth_before", C.c_uint32), ("depth_after", C.c_uint32), ("wide_depth", C.c_uint32),
                ("ms_sort", C.c_double), ("ms_topology", C.c_double), ("ms_refit", C.c_double), ("ms_collapse", C.c_double)]


class BoundedBuildInfo(C.Structure):
    _fields_ = [("max_depth", C.c_uint32), ("forced_nodes", C.c_uint32), ("first_forced_level", C.c_uint32), ("reserved", C.c_uint32)]


def _tree_cost_dict(c: TreeCost) -> dict:
    """The fields of hpt_tree_cost (root_extent as a tuple) and, under "bytes", the struct's 120 bytes."""
    d = {n: getattr(c, n) for n, _ in c._fields_ if n != "root_extent"}
    d["root_extent"] = tuple(c.root_extent)
    d["bytes"] = bytes(c)
    return d


# exported tree (include/hpt.h, hpt_bvh_info): 32-B quantised nodes as 8 uint32 words, 48-B triangles as 12 words
QNODE_WORDS = 8
TRI_WORDS = 12

_lib = None


def _share_the_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch's ROCm wheels bundle their own libamdhip64.so (soname libamdhip64.so.7) and
    ask for it by the unversioned name, so if libhpt.so is loaded first it brings in /opt/rocm's copy, `import torch`
    then loads a second one, and whichever initialises second finds no device ("No HIP GPUs are available" / "no
    ROCm-capable device is detected").  When torch is installed but not imported yet, its copy is loaded here first;
    libhpt.so's NEEDED libamdhip64.so.7 then resolves to it by soname, and a later `import torch` reuses it."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.origin:
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load_library() -> C.CDLL:
    """Loads csrc/libhpt.so; raises HptError if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        _share_the_hip_runtime_with_torch()
        path = os.environ.get("HPT_LIBRARY") or LIB_PATH        # HPT_LIBRARY: another build of libhpt.so (development A/B runs)
        if not os.path.exists(path):
            raise HptError("%s not built: run `make -C path_tracing_amd/csrc` "
                           "(or __graft_entry__.build()); there is no CPU fallback" % path)
        lib = C.CDLL(path)
        lib.hpt_last_error.restype = C.c_char_p
        lib.hpt_local_pixels.restype = C.c_int64
        lib.hpt_local_pixels.argtypes = [C.c_int, C.c_int, C.POINTER(Params)]
        for name in ("hpt_scene_create", "hpt_render_pt", "hpt_render_pt_device", "hpt_untile", "hpt_scene_set_groups",
                     "hpt_render_bdpt", "hpt_render_bdpt_device", "hpt_bdpt_render_wrapper",
                     "hpt_pt_render_wrapper", "hpt_get_stats", "hpt_trace_closest", "hpt_trace_visibility",
                     "hpt_device_count", "hpt_multi_create", "hpt_multi_num_devices", "hpt_multi_set_groups",
                     "hpt_multi_render_pt", "hpt_multi_render_bdpt", "hpt_multi_get_timing", "hpt_wrapper_set_devices",
                     "hpt_probe_functions", "hpt_tonemap", "hpt_tonemap_host", "hpt_bvh_export_host", "hpt_scene_export_bvh",
                     "hpt_render_ppm", "hpt_ppm_get_stats", "hpt_ppm_render_wrapper",
                     "hpt_sppm_create", "hpt_sppm_render", "hpt_sppm_reset", "hpt_sppm_read_state",
                     "hpt_render_guides", "hpt_denoiser_create", "hpt_denoiser_set_guides", "hpt_denoiser_run",
                     "hpt_denoiser_last_ms", "hpt_denoiser_level_ms", "hpt_denoise_host",
                     "hpt_accum_create", "hpt_accum_add", "hpt_accum_mean", "hpt_accum_variance", "hpt_accum_reset", "hpt_accum_read",
                     "hpt_display_create", "hpt_display_present", "hpt_display_metrics", "hpt_display_reset",
                     "hpt_render_guides_device", "hpt_history_create", "hpt_history_advance", "hpt_history_metrics",
                     "hpt_history_read", "hpt_history_reset", "hpt_history_check",
                     "hpt_denoiser_run_guided", "hpt_denoiser_estimate_variance", "hpt_history_length", "hpt_guided_check",
                     "hpt_history_create_flags", "hpt_history_variance", "hpt_history_read_moments", "hpt_history_variance_check",
                     "hpt_scene_update_triangles", "hpt_scene_update_rounds", "hpt_scene_update_check", "hpt_scene_get_update_info",
                     "hpt_bvh_refit_host", "hpt_scene_keep_previous", "hpt_scene_has_motion", "hpt_render_guides_motion",
                     "hpt_render_guides_motion_device", "hpt_history_advance_motion", "hpt_history_motion_check",
                     "hpt_scene_update_vertices_device", "hpt_scene_set_parts", "hpt_scene_pose", "hpt_scene_read_triangles",
                     "hpt_pose_host", "hpt_scene_set_skin", "hpt_scene_skin", "hpt_skin_host", "hpt_scene_set_morphs", "hpt_scene_morph",
                     "hpt_morph_host",
                     "hpt_scene_tree_cost", "hpt_bvh_cost_host", "hpt_scene_rebuild", "hpt_scene_get_rebuild_info",
                     "hpt_scene_rebuild_device", "hpt_scene_get_device_build_info", "hpt_bvh_device_build_host",
                     "hpt_scene_rebuild_device_bounded", "hpt_scene_get_bounded_build_info", "hpt_bvh_device_build_bounded_host"):
            if hasattr(lib, name):          # (an older build loaded through HPT_LIBRARY for an A/B run lacks the newest entry points)
                getattr(lib, name).restype = C.c_int
        if hasattr(lib, "hpt_sppm_destroy"):
            lib.hpt_sppm_destroy.restype = None
            lib.hpt_sppm_destroy.argtypes = [C.c_void_p]
        if hasattr(lib, "hpt_denoiser_destroy"):
            lib.hpt_denoiser_destroy.restype = None
            lib.hpt_denoiser_destroy.argtypes = [C.c_void_p]
        for name in ("hpt_accum_destroy", "hpt_display_destroy", "hpt_history_destroy"):
            if hasattr(lib, name):
                getattr(lib, name).restype = None
                getattr(lib, name).argtypes = [C.c_void_p]
        if hasattr(lib, "hpt_accum_count"):
            lib.hpt_accum_count.restype = C.c_int64
            lib.hpt_accum_count.argtypes = [C.c_void_p]
        lib.hpt_scene_destroy.restype = None
        lib.hpt_wrapper_cache_clear.restype = None
        lib.hpt_wrapper_cache_clear.argtypes = []
        lib.hpt_scene_destroy.argtypes = [C.c_void_p]
        lib.hpt_multi_destroy.restype = None
        lib.hpt_multi_destroy.argtypes = [C.c_void_p]
        _lib = lib
    return _lib


def _check(rc: int):
    if rc != 0:
        raise HptError("hpt error %d: %s" % (rc, load_library().hpt_last_error().decode("utf-8", "replace")))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None


def device_count() -> int:
    return int(load_library().hpt_device_count())


def make_params(seed=1, sample_offset=0, max_delta=0, rank=0, world=1, tile=0, samples_per_pass=0, flags=0) -> Params:
    p = Params()
    p.seed, p.sample_offset, p.max_delta = int(seed), int(sample_offset), int(max_delta)
    p.rank, p.world, p.tile, p.samples_per_pass, p.flags, p.reserved = rank, world, tile, samples_per_pass, flags, 0
    return p


def local_pixels(W: int, H: int, params: Params) -> int:
    n = int(load_library().hpt_local_pixels(W, H, C.byref(params)))
    if n < 0:
        _check(1)
    return n


class Scene:
    """Device-resident scene + BVH (the upload half of the reference's helper API:
    move_data_to_cuda_pt, src/pt_cu_helper.cpp:12-64).  Inputs are arrays of the reference's
    records (layouts.LIGHT / SPHERE / TRIANGLE), e.g. from scene_io.flatten_for_pt."""

    def __init__(self, lights, spheres, triangles):
        self._lib = load_library()
        self._h = C.c_void_p()
        lights = np.ascontiguousarray(lights, LIGHT)
        spheres = np.ascontiguousarray(spheres, SPHERE)
        triangles = np.ascontiguousarray(triangles, TRIANGLE)
        _check(self._lib.hpt_scene_create(_vp(lights), len(lights), _vp(spheres), len(spheres),
                                          _vp(triangles), len(triangles), C.byref(self._h)))
        self.num_lights, self.num_spheres, self.num_triangles = len(lights), len(spheres), len(triangles)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.hpt_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- rendering ----------------------------------------------------------------------
    def render_pt(self, camera, W, H, eye_depth=4, spp=8, params: Params | None = None) -> np.ndarray:
        """Blocking whole-image render (run_cuda_pt, src/pt_cu_helper.cpp:66-77).
        Returns float32 [H, W, 3], row 0 = top, linear mean radiance."""
        params = params or make_params()
        cam = np.ascontiguousarray(camera, CAMERA)
        img = np.empty((H, W, 3), np.float32)
        _check(self._lib.hpt_render_pt(self._h, _vp(cam.reshape(1)), W, H, eye_depth, spp, C.byref(params), _vp(img)))
        return img

    def render_pt_device(self, camera, W, H, eye_depth, spp, params: Params, d_local_ptr: int, stream: int = 0):
        """Asynchronous render of this rank's tiles into device memory (packed local order)."""
        cam = np.ascontiguousarray(camera, CAMERA)
        _check(self._lib.hpt_render_pt_device(self._h, _vp(cam.reshape(1)), W, H, eye_depth, spp, C.byref(params),
                                              C.c_void_p(d_local_ptr), C.c_void_p(stream)))

    # -- bidirectional estimator (run_cuda_bdpt, reference include/bdpt_cu_helper.h:6; semantics of run_cpu_bdpt) ---
    def set_groups(self, kind, index, group):
        """Scene-file grouping of the objects (kind 0 sphere / 1 triangle, index, group id; insertion order)."""
        k = np.ascontiguousarray(kind, np.int32); i = np.ascontiguousarray(index, np.int32); g = np.ascontiguousarray(group, np.int32)
        _check(self._lib.hpt_scene_set_groups(self._h, _vp(k), _vp(i), _vp(g), len(k)))

    def render_bdpt(self, camera, W, H, eye_depth=4, light_depth=4, spp=8, spl=8, params: Params | None = None) -> np.ndarray:
        params = params or make_params()
        cam = np.ascontiguousarray(camera, CAMERA)
        img = np.empty((H, W, 3), np.float32)
        _check(self._lib.hpt_render_bdpt(self._h, _vp(cam.reshape(1)), W, H, eye_depth, light_depth, spp, spl, C.byref(params), _vp(img)))
        return img

    def render_bdpt_device(self, camera, W, H, eye_depth, light_depth, spp, spl, params: Params, d_local_ptr: int, stream: int = 0):
        cam = np.ascontiguousarray(camera, CAMERA)
        _check(self._lib.hpt_render_bdpt_device(self._h, _vp(cam.reshape(1)), W, H, eye_depth, light_depth, spp, spl, C.byref(params),
                                                C.c_void_p(d_local_ptr), C.c_void_p(stream)))

    # -- photon mapping (run_cuda_ppm / ppm_render_wrapper, reference src/ppm_cu.cu) ----------------------------------
    def render_ppm(self, camera, W, H, eye_depth=4, light_depth=4, spp=1, spl=8, radius=0.05, params: Params | None = None,
                   scene_min=None, scene_max=None) -> np.ndarray:
        """spp independent passes of the reference's photon-mapping estimator, averaged (FLAG_OUTPUT_SUM: summed);
        nl * spl photons per pass.  scene_min / scene_max None: the scene's own bounds.  float32 [H, W, 3]."""
        params = params or make_params()
        cam = np.ascontiguousarray(camera, CAMERA)
        img = np.empty((H, W, 3), np.float32)
        mn = (C.c_float * 3)(*scene_min) if scene_min is not None else None
        mx = (C.c_float * 3)(*scene_max) if scene_max is not None else None
        _check(self._lib.hpt_render_ppm(self._h, _vp(cam.reshape(1)), W, H, eye_depth, light_depth, spp, spl, C.c_float(radius),
                                        mn, mx, C.byref(params), _vp(img)))
        return img

    def ppm_stats(self) -> dict:
        st = PpmStats()
        _check(self._lib.hpt_ppm_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def sppm(self, camera, W, H, eye_depth=4, light_depth=4, spl=8, radius=0.05, alpha=0.7, params: Params | None = None,
             scene_min=None, scene_max=None) -> "Sppm":
        """A progressive photon-mapping state on this scene (include/hpt.h, hpt_sppm_*): per-pixel radius, photon
        count and flux that last across passes and calls.  params: seed, sample_offset, max_delta, tile (flags 0).
        The scene must stay open while the state lives."""
        return Sppm(self, camera, W, H, eye_depth, light_depth, spl, radius, alpha, params, scene_min, scene_max)

    def render_guides(self, camera, W, H, spp=4, params: Params | None = None, prev_position=False) -> dict:
        """First-hit guide images for the denoiser (include/hpt.h, hpt_render_guides): the means over spp eye-pass samples
        of base colour, ray-facing normal and position of the first non-delta surface, and the number of samples that
        found one.  dict(albedo, normal, position: float32 [H, W, 3]; coverage: float32 [H, W]); with prev_position=True
        also prev_position [H, W, 3], where each pixel's point was in the scene's previous geometry
        (hpt_render_guides_motion)."""
        params = params or make_params()
        cam = np.ascontiguousarray(camera, CAMERA)
        g = dict(albedo=np.empty((H, W, 3), np.float32), normal=np.empty((H, W, 3), np.float32),
                 position=np.empty((H, W, 3), np.float32), coverage=np.empty((H, W), np.float32))
        if prev_position:
            g["prev_position"] = np.empty((H, W, 3), np.float32)
            _check(self._lib.hpt_render_guides_motion(self._h, _vp(cam.reshape(1)), W, H, int(spp), C.byref(params), _vp(g["albedo"]),
                                                      _vp(g["normal"]), _vp(g["position"]), _vp(g["coverage"]), _vp(g["prev_position"])))
            return g
        _check(self._lib.hpt_render_guides(self._h, _vp(cam.reshape(1)), W, H, int(spp), C.byref(params), _vp(g["albedo"]),
                                           _vp(g["normal"]), _vp(g["position"]), _vp(g["coverage"])))
        return g

    def render_guides_device(self, camera, W, H, spp=4, params: Params | None = None, albedo=None, normal=None, position=None,
                             coverage=None, prev_position=None):
        """render_guides into DEVICE images (ints or torch tensors, float32, [H, W, 3]; coverage [H, W]; None = not
        wanted, at least one is): the same bytes, complete when the call returns.  prev_position: the motion guide
        (hpt_render_guides_motion_device)."""
        params = params or make_params()
        cam = np.ascontiguousarray(camera, CAMERA)
        ptr = [_dptr(x) if x is not None else None for x in (albedo, normal, position, coverage)]
        if prev_position is not None:
            _check(self._lib.hpt_render_guides_motion_device(self._h, _vp(cam.reshape(1)), W, H, int(spp), C.byref(params), *ptr,
                                                             _dptr(prev_position)))
            return
        _check(self._lib.hpt_render_guides_device(self._h, _vp(cam.reshape(1)), W, H, int(spp), C.byref(params), *ptr))

    def stats(self) -> dict:
        st = Stats()
        _check(self._lib.hpt_get_stats(self._h, C.byref(st)))
        return st.as_dict()

    def export_bvh(self) -> dict:
        """The tree this scene's device holds (include/hpt.h, hpt_scene_export_bvh): dict(info, qnodes [n, 8] uint32,
        tris [m, 12] uint32 words of the 48-B leaf-order records)."""
        return _export_bvh(lambda info, qn, qcap, tr, tcap: self._lib.hpt_scene_export_bvh(self._h, info, qn, qcap, tr, tcap))

    # -- scene updates (include/hpt.h) -----------------------------------------------------
    def update_triangles(self, triangles):
        """Moves the scene's triangles in place: the same number of records, only their vertices changed.  The tree is
        refitted on the device; every integrator renders the new scene afterwards.  Blocking."""
        tr = np.ascontiguousarray(triangles, TRIANGLE)
        _check(self._lib.hpt_scene_update_triangles(self._h, _vp(tr), len(tr)))

    def update_rounds(self, lights, spheres):
        """Replaces the lights and the spheres (same counts; sphere materials unchanged, any light field may change)."""
        L = np.ascontiguousarray(lights, LIGHT)
        sp = np.ascontiguousarray(spheres, SPHERE)
        _check(self._lib.hpt_scene_update_rounds(self._h, _vp(L), len(L), _vp(sp), len(sp)))

    def update_check(self, triangles):
        """Raises HptError where update_triangles would refuse these records; no device work."""
        update_check(self, triangles)

    # -- poses (include/hpt.h) ---------------------------------------------------------------
    def update_vertices_device(self, v, num_triangles=None):
        """update_triangles from vertices that are on the device already: a contiguous float32 CUDA torch.Tensor of shape
        [nt, 3, 3] or [nt * 9] on the scene's device (a tensor does not say which stream produced it: the device is
        waited for here), or an integer device pointer with num_triangles given (the caller has waited).  Blocking."""
        if isinstance(v, int):
            if num_triangles is None:
                raise HptError("hpt error 1: update_vertices_device: a device pointer needs num_triangles")
            ptr, nt = v, int(num_triangles)
        else:
            import torch
            if not isinstance(v, torch.Tensor) or not v.is_cuda or v.dtype != torch.float32 or not v.is_contiguous():
                raise HptError("hpt error 1: update_vertices_device takes a contiguous float32 CUDA tensor or a device pointer")
            if not ((v.dim() == 3 and tuple(v.shape[1:]) == (3, 3)) or (v.dim() == 1 and v.numel() % 9 == 0)):
                raise HptError("hpt error 1: update_vertices_device: the tensor's shape must be [nt, 3, 3] or [nt * 9], not %s" % (tuple(v.shape),))
            nt = v.numel() // 9
            if num_triangles is not None and int(num_triangles) != nt:
                raise HptError("hpt error 1: update_vertices_device: the tensor holds %d triangles, num_triangles says %d" % (nt, int(num_triangles)))
            torch.cuda.synchronize(v.device)
            ptr = v.data_ptr() if nt else 0
        _check(self._lib.hpt_scene_update_vertices_device(self._h, C.c_void_p(ptr) if ptr else None, nt))

    def set_parts(self, tri_part, num_parts):
        """Gives every triangle a part (int32 per triangle, or None with num_parts == 1) and captures the rest pose: the
        vertices as the scene holds them now."""
        tp = np.ascontiguousarray(tri_part, np.int32) if tri_part is not None else None
        n = len(tp) if tp is not None else self.num_triangles
        _check(self._lib.hpt_scene_set_parts(self._h, _vp(tp) if tp is not None else None, n, int(num_parts)))

    def pose(self, xforms):
        """One absolute pose: [num_parts, 3, 4] (or [num_parts, 12]) float32, rows (a, b, c, t), applied to the rest pose on
        the device; the tree is refitted.  Blocking."""
        x = np.ascontiguousarray(xforms, np.float32)
        if x.size % 12:
            raise HptError("hpt error 1: pose: twelve floats per part")
        _check(self._lib.hpt_scene_pose(self._h, _vp(x), x.size // 12))

    # -- skinning (include/hpt.h) ------------------------------------------------------------
    def set_skin(self, corner_bone, corner_weight, num_bones):
        """Gives every corner four (bone, weight) influences -- int32 and float32 of shape [nt, 3, 4] (or flat) -- and
        captures the rest pose; the scene's parts, if it had any, are dropped."""
        b, w = _skin_arrays("set_skin", corner_bone, corner_weight)
        _check(self._lib.hpt_scene_set_skin(self._h, _vp(b), _vp(w), b.size // 12, int(num_bones)))

    def skin(self, xforms):
        """One absolute skin: [num_bones, 3, 4] (or [num_bones, 12]) float32, rows (a, b, c, t), blended over the rest pose
        on the device; the tree is refitted.  Blocking."""
        x = np.ascontiguousarray(xforms, np.float32)
        if x.size % 12:
            raise HptError("hpt error 1: skin: twelve floats per bone")
        _check(self._lib.hpt_scene_skin(self._h, _vp(x), x.size // 12))

    # -- morph targets (include/hpt.h) --------------------------------------------------------
    def set_morphs(self, target_begin, entry_corner, entry_delta):
        """Gives the scene sparse morph targets -- target t owns entries target_begin[t] .. target_begin[t + 1] - 1, entry e
        moves corner entry_corner[e] by entry_delta[e] ([num_entries, 3] float32 or flat) -- and captures the rest pose; parts
        or a skin, if the scene has them, stay."""
        tb, ec, ed = _morph_arrays("set_morphs", target_begin, entry_corner, entry_delta)
        _check(self._lib.hpt_scene_set_morphs(self._h, _vp(tb), _vp(ec), _vp(ed), ec.size, self.num_triangles, tb.size - 1))

    def morph(self, weights):
        """One absolute morph: one float32 weight per target, summed over the rest pose on the device; the scene's deformer,
        if it has one, is then applied with its last table, and the tree is refitted.  Blocking."""
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        _check(self._lib.hpt_scene_morph(self._h, _vp(w), w.size))

    def read_triangles(self) -> np.ndarray:
        """The records the handle holds now (layouts.TRIANGLE): the scene's non-vertex bytes with the current vertices."""
        out = np.zeros(self.num_triangles, TRIANGLE)
        _check(self._lib.hpt_scene_read_triangles(self._h, _vp(out), len(out)))
        return out

    def keep_previous(self):
        """The current geometry becomes the previous one (include/hpt.h, "motion"): once per frame, after the frame's
        guides and before the next frame's updates.  Blocking."""
        _check(self._lib.hpt_scene_keep_previous(self._h))

    def has_motion(self) -> bool:
        """True when an update succeeded since the scene was created or keep_previous() was last called."""
        rc = int(self._lib.hpt_scene_has_motion(self._h))
        if rc < 0:
            _check(1)
        return rc == 1

    def update_info(self) -> dict:
        """The last triangle update of any kind (update_triangles, update_vertices_device, pose, skin, morph): dict(updates, live_tris, dead_tris, ms_pack, ms_upload, ms_refit)."""
        info = UpdateInfo()
        _check(self._lib.hpt_scene_get_update_info(self._h, C.byref(info)))
        return {n: getattr(info, n) for n, _ in info._fields_}

    # -- tree cost and rebuild (include/hpt.h) ------------------------------------------------
    def tree_cost(self) -> dict:
        """The cost of the tree the device holds, reduced on the device (include/hpt.h, "tree cost"): the fields of
        hpt_tree_cost and the struct's bytes, which equal tree_cost_host(export_bvh())'s.  Blocking."""
        c = TreeCost()
        _check(self._lib.hpt_scene_tree_cost(self._h, C.byref(c)))
        return _tree_cost_dict(c)

    def rebuild(self):
        """A new tree in place, built by the host builder from the records the handle holds now (include/hpt.h, "rebuild"):
        afterwards export_bvh() equals export_bvh_host(lights, spheres, read_triangles()).  Everything else the handle
        keeps stays.  Blocking."""
        _check(self._lib.hpt_scene_rebuild(self._h))

    def rebuild_info(self) -> dict:
        """The last rebuild: dict(rebuilds, nodes_before, nodes_after, depth_before, depth_after, ms_download, ms_build, ms_upload)."""
        info = RebuildInfo()
        _check(self._lib.hpt_scene_get_rebuild_info(self._h, C.byref(info)))
        return {n: getattr(info, n) for n, _ in info._fields_}

    def rebuild_device(self):
        """A new tree in place, built on the device from the vertices the device holds (include/hpt.h, "device builds"):
        afterwards export_bvh() equals device_build_bvh_host(lights, spheres, read_triangles()).  A tree too deep for the
        traversal falls back to rebuild() (device_build_info()["fell_back"]).  Everything else the handle keeps stays.  Blocking."""
        _check(self._lib.hpt_scene_rebuild_device(self._h))

    def device_build_info(self) -> dict:
        """The last rebuild_device: dict(builds, fell_back, nodes_before, nodes_after, depth_before, depth_after, wide_depth,
        ms_sort, ms_topology, ms_refit, ms_collapse)."""
        info = DeviceBuildInfo()
        _check(self._lib.hpt_scene_get_device_build_info(self._h, C.byref(info)))
        return {n: getattr(info, n) for n, _ in info._fields_}

    def rebuild_device_bounded(self, max_depth=0):
        """rebuild_device with a tree of at most max_depth levels (include/hpt.h, "bounded device builds"; 0: the traversal's
        30): afterwards export_bvh() equals device_build_bounded_bvh_host(lights, spheres, read_triangles(), None, max_depth).
        The depth of the data's radix tree no longer sends the call to rebuild(); a max_depth of 19 or less never falls back.
        Fills device_build_info() and bounded_build_info().  Blocking."""
        _check(self._lib.hpt_scene_rebuild_device_bounded(self._h, C.c_int(int(max_depth))))

    def bounded_build_info(self) -> dict:
        """The last rebuild_device_bounded: dict(max_depth, forced_nodes, first_forced_level); zeros before the first."""
        info = BoundedBuildInfo()
        _check(self._lib.hpt_scene_get_bounded_build_info(self._h, C.byref(info)))
        return {n: getattr(info, n) for n, _ in info._fields_ if n != "reserved"}

    # -- ray probes (tests) ---------------------------------------------------------------
    def trace_closest(self, origins, dirs, brute_force=False):
        o = np.ascontiguousarray(origins, np.float32)
        d = np.ascontiguousarray(dirs, np.float32)
        n = len(o)
        t = np.empty(n, np.float32)
        prim = np.empty(n, np.int32)
        _check(self._lib.hpt_trace_closest(self._h, _vp(o), _vp(d), n, FLAG_BRUTE_FORCE if brute_force else 0, _vp(t), _vp(prim)))
        return t, prim

    def trace_visibility(self, p1, p2, brute_force=False):
        a = np.ascontiguousarray(p1, np.float32)
        b = np.ascontiguousarray(p2, np.float32)
        n = len(a)
        vis = np.empty(n, np.int32)
        _check(self._lib.hpt_trace_visibility(self._h, _vp(a), _vp(b), n, FLAG_BRUTE_FORCE if brute_force else 0, _vp(vis)))
        return vis


class Sppm:
    """Progressive photon-mapping state (Scene.sppm).  render(passes) advances it and returns the estimate."""

    def __init__(self, scene, camera, W, H, eye_depth, light_depth, spl, radius, alpha, params, scene_min, scene_max):
        self._lib = scene._lib
        self._scene = scene                 # the scene must outlive the state
        self._h = C.c_void_p()
        self.W, self.H = W, H
        params = params or make_params()
        cam = np.ascontiguousarray(camera, CAMERA)
        mn = (C.c_float * 3)(*scene_min) if scene_min is not None else None
        mx = (C.c_float * 3)(*scene_max) if scene_max is not None else None
        _check(self._lib.hpt_sppm_create(scene._h, _vp(cam.reshape(1)), W, H, eye_depth, light_depth, spl, C.c_float(radius),
                                         C.c_float(alpha), mn, mx, C.byref(params), C.byref(self._h)))

    def render(self, passes=1, flags=0) -> np.ndarray:
        """`passes` more passes; the estimate after them, float32 [H, W, 3] (flags: FLAG_TIME_KERNELS | FLAG_COUNT_WORK,
        reported through Scene.ppm_stats)."""
        img = np.empty((self.H, self.W, 3), np.float32)
        _check(self._lib.hpt_sppm_render(self._h, int(passes), int(flags), _vp(img)))
        return img

    def reset(self):
        """Back to K = 0; bounds left to the scene at creation (scene_min / scene_max None) are taken from it again."""
        _check(self._lib.hpt_sppm_reset(self._h))

    def state(self) -> dict:
        """dict(radius2 [H, W] f32, photons [H, W] f32, passes int)."""
        r2 = np.empty((self.H, self.W), np.float32)
        n = np.empty((self.H, self.W), np.float32)
        k = C.c_int64()
        _check(self._lib.hpt_sppm_read_state(self._h, _vp(r2), _vp(n), C.byref(k)))
        return dict(radius2=r2, photons=n, passes=int(k.value))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.hpt_sppm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _dptr(x) -> C.c_void_p:
    """A device pointer: an int, or anything with data_ptr() (a torch tensor on the device)."""
    return C.c_void_p(int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x))


class Denoiser:
    """Edge-avoiding a-trous filter on the device (include/hpt.h, hpt_denoiser_*) for W x H images.  Guides and images
    are DEVICE buffers (ints or torch tensors, float32, the layouts of Scene.render_guides); set_guides once per camera
    position, run once per frame.  Both only enqueue on `stream`.  Host arrays: denoise()."""

    def __init__(self, W, H):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.W, self.H = W, H
        _check(self._lib.hpt_denoiser_create(int(W), int(H), C.byref(self._h)))

    def set_guides(self, albedo, normal, position, coverage, stream: int = 0):
        _check(self._lib.hpt_denoiser_set_guides(self._h, _dptr(albedo), _dptr(normal), _dptr(position), _dptr(coverage), C.c_void_p(stream)))

    def run(self, linear_rgb, out, params: DenoiseParams | None = None, stream: int = 0):
        params = params or make_denoise_params()
        _check(self._lib.hpt_denoiser_run(self._h, _dptr(linear_rgb), _dptr(out), C.byref(params), C.c_void_p(stream)))

    def run_guided(self, linear_rgb, variance, out, variance_out=None, params: GuidedParams | None = None, stream: int = 0):
        """The variance-guided filter: `variance` is W*H*3 (Accumulator.variance or estimate_variance); variance_out, when
        given, receives the filtered scalar variance (W*H, in the filter's working space)."""
        params = params or make_guided_params()
        _check(self._lib.hpt_denoiser_run_guided(self._h, _dptr(linear_rgb), _dptr(variance), _dptr(out),
                                                 _dptr(variance_out) if variance_out is not None else None, C.byref(params), C.c_void_p(stream)))

    def estimate_variance(self, frame, variance_out, length=None, params: GuidedParams | None = None, stream: int = 0):
        """Spatial per-channel variance (W*H*3) of ONE new frame over 7 x 7 windows steered by the guides; with `length`
        (W*H, History.length) divided by it: the variance of the mean."""
        params = params or make_guided_params()
        _check(self._lib.hpt_denoiser_estimate_variance(self._h, _dptr(frame), _dptr(length) if length is not None else None,
                                                        _dptr(variance_out), C.byref(params), C.c_void_p(stream)))

    def last_ms(self) -> dict:
        """Times of the last run with DENOISE_TIME (waits for it): dict(pack, filter, levels [8])."""
        a, b = C.c_double(), C.c_double()
        lv = (C.c_double * 8)()
        _check(self._lib.hpt_denoiser_last_ms(self._h, C.byref(a), C.byref(b)))
        _check(self._lib.hpt_denoiser_level_ms(self._h, lv, 8))
        return dict(pack=a.value, filter=b.value, levels=list(lv))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.hpt_denoiser_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def denoise(image, guides, iterations=0, sigma_color=0, sigma_normal=0, sigma_position=0, demodulate=True) -> np.ndarray:
    """Filters a host image [H, W, 3] with host guides (the dict of Scene.render_guides) through hpt_denoise_host:
    upload, set_guides, run, download.  Zeros select the defaults; a negative sigma switches its term off."""
    img = np.ascontiguousarray(image, np.float32)
    H, W = img.shape[:2]
    g = [np.ascontiguousarray(guides[k], np.float32) for k in ("albedo", "normal", "position", "coverage")]
    if img.shape != (H, W, 3) or any(a.shape != (H, W, 3) for a in g[:3]) or g[3].shape != (H, W):
        raise ValueError("denoise: image and guides must be [H, W, 3] (coverage [H, W]) of one size")
    out = np.empty((H, W, 3), np.float32)
    p = make_denoise_params(iterations, sigma_color, sigma_normal, sigma_position, demodulate)
    _check(load_library().hpt_denoise_host(_vp(img), _vp(g[0]), _vp(g[1]), _vp(g[2]), _vp(g[3]), _vp(out), W, H, C.byref(p)))
    return out


def guided_check(W, H, linear_rgb, variance, out, variance_out=None, params: GuidedParams | None = None) -> None:
    """Every argument check of Denoiser.run_guided on a W x H image, without a denoiser or a device (hpt_guided_check);
    raises HptError as the run would."""
    opt = lambda x: _dptr(x) if x is not None else None
    _check(load_library().hpt_guided_check(int(W), int(H), opt(linear_rgb), opt(variance), opt(out), opt(variance_out),
                                           C.byref(params) if params is not None else None))


def history_motion_check(W, H, camera, frame, normal=None, position=None, coverage=None, prev_position=None,
                         params: HistoryParams | None = None, mean_out=None) -> None:
    """Every argument check of History.advance with the motion guide on a W x H history, without a history or a device
    (hpt_history_motion_check); raises HptError as the advance would.  Images are device pointers (ints) or tensors."""
    opt = lambda x: _dptr(x) if x is not None else None
    cam = np.ascontiguousarray(camera, CAMERA).reshape(1) if camera is not None else None
    _check(load_library().hpt_history_motion_check(int(W), int(H), _vp(cam) if cam is not None else None, opt(frame), opt(normal),
                                                   opt(position), opt(coverage), opt(prev_position),
                                                   C.byref(params) if params is not None else None, opt(mean_out)))


def history_variance_check(W, H, out, fallback=None, min_length=0.0, moments=True) -> None:
    """Every argument check of History.variance on a W x H history, without a history or a device
    (hpt_history_variance_check); raises HptError as the call would."""
    opt = lambda x: _dptr(x) if x is not None else None
    _check(load_library().hpt_history_variance_check(int(W), int(H), C.c_int32(HISTORY_MOMENTS if moments else 0), opt(fallback),
                                                     C.c_float(min_length), opt(out)))


class Accumulator:
    """Running sum over frames on the device (include/hpt.h, hpt_accum_*) for W x H images: float32 adds in frame order,
    with moments=True also the sum of squares.  Frames and outputs are DEVICE buffers (ints or torch tensors, float32,
    W*H*3, row 0 = top); every call only enqueues on `stream`, except read()."""

    def __init__(self, W, H, moments=False):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.W, self.H, self.moments = int(W), int(H), bool(moments)
        _check(self._lib.hpt_accum_create(int(W), int(H), C.c_int32(ACCUM_MOMENTS if moments else 0), C.byref(self._h)))

    def add(self, frame, mean_out=None, stream: int = 0):
        """sum += frame; mean_out (may be `frame` itself) receives sum / count."""
        _check(self._lib.hpt_accum_add(self._h, _dptr(frame), _dptr(mean_out) if mean_out is not None else None, C.c_void_p(stream)))

    def mean(self, out, stream: int = 0):
        _check(self._lib.hpt_accum_mean(self._h, _dptr(out), C.c_void_p(stream)))

    def variance(self, out, stream: int = 0):
        """The variance of the mean (moments=True); all zeros below two frames."""
        _check(self._lib.hpt_accum_variance(self._h, _dptr(out), C.c_void_p(stream)))

    def reset(self, stream: int = 0):
        _check(self._lib.hpt_accum_reset(self._h, C.c_void_p(stream)))

    @property
    def count(self) -> int:
        return int(self._lib.hpt_accum_count(self._h))

    def read(self) -> dict:
        """Waits for the device: dict(sum [H, W, 3] f32, sumsq (the same, or None without moments), count int)."""
        s = np.empty((self.H, self.W, 3), np.float32)
        q = np.empty((self.H, self.W, 3), np.float32) if self.moments else None
        k = C.c_int64()
        _check(self._lib.hpt_accum_read(self._h, _vp(s), _vp(q), C.byref(k)))
        return dict(sum=s, sumsq=q, count=int(k.value))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.hpt_accum_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Display:
    """The bytes on screen and how much they moved (include/hpt.h, hpt_display_*): present() tone-maps a DEVICE image
    (int or torch tensor, float32, W*H*3) into a panel of a uint8 framebuffer and sums the squared byte differences
    against the previous present and against `other`, another Display; metrics() waits for the last present."""

    def __init__(self, W, H):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.W, self.H = int(W), int(H)
        _check(self._lib.hpt_display_create(int(W), int(H), C.byref(self._h)))

    def present(self, linear, out=None, other=None, pitch=0, x_offset=0, bgr=False, flip_y=False, stream: int = 0):
        flags = (DISPLAY_BGR if bgr else 0) | (DISPLAY_FLIP_Y if flip_y else 0)
        _check(self._lib.hpt_display_present(self._h, _dptr(linear), other._h if other is not None else None,
                                             _dptr(out) if out is not None else None, C.c_int64(pitch), C.c_int64(x_offset),
                                             C.c_int32(flags), C.c_void_p(stream)))

    def metrics(self) -> dict:
        """dict(rms_prev, rms_other: float; ssd_prev, ssd_other, presented: int) of the last present."""
        rp, ro = C.c_double(), C.c_double()
        sp, so = C.c_uint64(), C.c_uint64()
        n = C.c_int64()
        _check(self._lib.hpt_display_metrics(self._h, C.byref(rp), C.byref(ro), C.byref(sp), C.byref(so), C.byref(n)))
        return dict(rms_prev=rp.value, rms_other=ro.value, ssd_prev=int(sp.value), ssd_other=int(so.value), presented=int(n.value))

    def reset(self, stream: int = 0):
        _check(self._lib.hpt_display_reset(self._h, C.c_void_p(stream)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.hpt_display_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class History:
    """Per-pixel running mean that survives camera moves (include/hpt.h, hpt_history_*) for W x H images.  advance() takes
    the frame's camera record, its DEVICE colour image and the three DEVICE guide images of Scene.render_guides_device
    (all three or none), reprojects the previous state where the geometry agrees and writes the new mean; metrics()
    waits for the last advance.  Every other call only enqueues on `stream`, except read().  With moments=True the history
    also carries the running mean of the squared frame values, and variance() gives the temporal variance of the mean."""

    def __init__(self, W, H, moments=False):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.W, self.H, self.moments = int(W), int(H), bool(moments)
        if moments:
            _check(self._lib.hpt_history_create_flags(int(W), int(H), C.c_int32(HISTORY_MOMENTS), C.byref(self._h)))
        else:
            _check(self._lib.hpt_history_create(int(W), int(H), C.byref(self._h)))

    def advance(self, camera, frame, normal=None, position=None, coverage=None, params: HistoryParams | None = None, mean_out=None,
                stream: int = 0, prev_position=None):
        """mean_out (may be `frame` itself) receives the new mean; params None = the defaults.  prev_position (DEVICE,
        W*H*3, of Scene.render_guides_device) makes the advance follow moving geometry (hpt_history_advance_motion)."""
        cam = np.ascontiguousarray(camera, CAMERA)
        opt = [_dptr(x) if x is not None else None for x in (normal, position, coverage)]
        if prev_position is not None:
            _check(self._lib.hpt_history_advance_motion(self._h, _vp(cam.reshape(1)), _dptr(frame), opt[0], opt[1], opt[2],
                                                        _dptr(prev_position), C.byref(params) if params is not None else None,
                                                        _dptr(mean_out) if mean_out is not None else None, C.c_void_p(stream)))
            return
        _check(self._lib.hpt_history_advance(self._h, _vp(cam.reshape(1)), _dptr(frame), opt[0], opt[1], opt[2],
                                             C.byref(params) if params is not None else None,
                                             _dptr(mean_out) if mean_out is not None else None, C.c_void_p(stream)))

    def metrics(self) -> dict:
        """dict(kept, restarted, frames: int) of the last advance."""
        k, r = C.c_uint64(), C.c_uint64()
        n = C.c_int64()
        _check(self._lib.hpt_history_metrics(self._h, C.byref(k), C.byref(r), C.byref(n)))
        return dict(kept=int(k.value), restarted=int(r.value), frames=int(n.value))

    def read(self) -> dict:
        """Waits for the device: dict(mean [H, W, 3] f32, length [H, W] f32, frames int), and q [H, W, 3] f32 on a moments
        history."""
        m = np.empty((self.H, self.W, 3), np.float32)
        n = np.empty((self.H, self.W), np.float32)
        k = C.c_int64()
        _check(self._lib.hpt_history_read(self._h, _vp(m), _vp(n), C.byref(k)))
        out = dict(mean=m, length=n, frames=int(k.value))
        if self.moments:
            q = np.empty((self.H, self.W, 3), np.float32)
            _check(self._lib.hpt_history_read_moments(self._h, _vp(q)))
            out["q"] = q
        return out

    def variance(self, out, fallback=None, min_length=0.0, stream: int = 0):
        """The temporal variance of the mean into the DEVICE image `out` (W*H*3 float32) where a pixel's history length is
        at least min_length (0 -> 4), `fallback` (W*H*3, may be `out` itself; None -> 0) elsewhere; enqueues only."""
        _check(self._lib.hpt_history_variance(self._h, _dptr(fallback) if fallback is not None else None, C.c_float(min_length),
                                              _dptr(out) if out is not None else None, C.c_void_p(stream)))

    def length(self, out, stream: int = 0):
        """The current history length n of every pixel into the DEVICE image `out` (W*H float32); enqueues only."""
        _check(self._lib.hpt_history_length(self._h, _dptr(out), C.c_void_p(stream)))

    def reset(self, stream: int = 0):
        _check(self._lib.hpt_history_reset(self._h, C.c_void_p(stream)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.hpt_history_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class MultiScene:
    """The blocking render call fanned out over the devices of one node inside ONE process (include/hpt.h,
    hpt_multi_*): scene and BVH built once and uploaded to every device, image tiles per device, RCCL gather
    on the first device (exchange=0) or peer copies (exchange=1; the only mode that accepts several ranks on
    one device).  Same results as Scene.render_pt / render_bdpt, bit for bit."""

    def __init__(self, lights, spheres, triangles, device_ids=None, num_devices=0, exchange=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        lights = np.ascontiguousarray(lights, LIGHT)
        spheres = np.ascontiguousarray(spheres, SPHERE)
        triangles = np.ascontiguousarray(triangles, TRIANGLE)
        ids = None
        if device_ids is not None:
            ids = np.ascontiguousarray(device_ids, np.int32)
            num_devices = len(ids)
        _check(self._lib.hpt_multi_create(_vp(lights), len(lights), _vp(spheres), len(spheres), _vp(triangles), len(triangles),
                                          _vp(ids), int(num_devices), int(exchange), C.byref(self._h)))
        self.num_devices = int(self._lib.hpt_multi_num_devices(self._h))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.hpt_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_groups(self, kind, index, group):
        k = np.ascontiguousarray(kind, np.int32); i = np.ascontiguousarray(index, np.int32); g = np.ascontiguousarray(group, np.int32)
        _check(self._lib.hpt_multi_set_groups(self._h, _vp(k), _vp(i), _vp(g), len(k)))

    def render_pt(self, camera, W, H, eye_depth=4, spp=8, params: Params | None = None) -> np.ndarray:
        params = params or make_params()
        cam = np.ascontiguousarray(camera, CAMERA)
        img = np.empty((H, W, 3), np.float32)
        _check(self._lib.hpt_multi_render_pt(self._h, _vp(cam.reshape(1)), W, H, eye_depth, spp, C.byref(params), _vp(img)))
        return img

    def render_bdpt(self, camera, W, H, eye_depth=4, light_depth=4, spp=8, spl=8, params: Params | None = None) -> np.ndarray:
        params = params or make_params()
        cam = np.ascontiguousarray(camera, CAMERA)
        img = np.empty((H, W, 3), np.float32)
        _check(self._lib.hpt_multi_render_bdpt(self._h, _vp(cam.reshape(1)), W, H, eye_depth, light_depth, spp, spl, C.byref(params), _vp(img)))
        return img

    def timing(self) -> dict:
        per = (C.c_double * self.num_devices)()
        g = C.c_double(); t = C.c_double()
        _check(self._lib.hpt_multi_get_timing(self._h, per, C.byref(g), C.byref(t)))
        return {"render_ms_per_device": list(per), "gather_ms": g.value, "total_ms": t.value}


def _export_bvh(call) -> dict:
    info = BvhInfo()
    _check(call(C.byref(info), None, C.c_size_t(0), None, C.c_size_t(0)))
    qn = np.zeros((max(info.num_nodes, 1), QNODE_WORDS), np.uint32)
    tr = np.zeros((max(info.num_tris, 1), TRI_WORDS), np.uint32)
    _check(call(C.byref(info), _vp(qn), C.c_size_t(qn.nbytes), _vp(tr), C.c_size_t(tr.nbytes)))
    return {"num_nodes": info.num_nodes, "num_tris": info.num_tris, "bvh_depth": info.bvh_depth, "num_rounds": info.num_rounds,
            "qorigin": np.array(info.qorigin, np.float32), "qscale": np.array(info.qscale, np.float32),
            "qnodes": qn[:info.num_nodes], "tris": tr[:info.num_tris]}


def export_bvh_host(lights, spheres, triangles) -> dict:
    """The tree hpt_scene_create would build and upload for these records, built on the host (no device needed)."""
    lib = load_library()
    lights = np.ascontiguousarray(lights, LIGHT)
    spheres = np.ascontiguousarray(spheres, SPHERE)
    triangles = np.ascontiguousarray(triangles, TRIANGLE)
    return _export_bvh(lambda info, qn, qcap, tr, tcap: lib.hpt_bvh_export_host(
        _vp(lights), len(lights), _vp(spheres), len(spheres), _vp(triangles), len(triangles), info, qn, qcap, tr, tcap))


def tree_cost_host(bvh) -> dict:
    """hpt_bvh_cost_host, the definition of Scene.tree_cost on the host (no device needed), over a tree as export_bvh_host,
    refit_bvh_host or Scene.export_bvh return it."""
    info = BvhInfo(int(bvh["num_nodes"]), int(bvh["num_tris"]), int(bvh["bvh_depth"]), int(bvh["num_rounds"]))
    for a in range(3):
        info.qorigin[a] = bvh["qorigin"][a]
        info.qscale[a] = bvh["qscale"][a]
    qn = np.ascontiguousarray(bvh["qnodes"], np.uint32)
    c = TreeCost()
    _check(load_library().hpt_bvh_cost_host(C.byref(info), _vp(qn), C.c_size_t(qn.nbytes), C.byref(c)))
    return _tree_cost_dict(c)


def refit_bvh_host(lights, spheres, triangles, new_triangles) -> dict:
    """The tree a scene created from `triangles` holds after update_triangles(new_triangles), computed on the host (no
    device needed): the definition the device's refit is held to.  The keys of export_bvh_host."""
    lib = load_library()
    lights = np.ascontiguousarray(lights, LIGHT)
    spheres = np.ascontiguousarray(spheres, SPHERE)
    triangles = np.ascontiguousarray(triangles, TRIANGLE)
    new_triangles = np.ascontiguousarray(new_triangles, TRIANGLE)
    if len(new_triangles) != len(triangles):
        raise HptError("hpt error 1: an update keeps the triangle count: %d triangles, %d were handed over" % (len(triangles), len(new_triangles)))
    return _export_bvh(lambda info, qn, qcap, tr, tcap: lib.hpt_bvh_refit_host(
        _vp(lights), len(lights), _vp(spheres), len(spheres), _vp(triangles), _vp(new_triangles), len(triangles), info, qn, qcap, tr, tcap))


def device_build_bvh_host(lights, spheres, triangles, new_triangles=None) -> dict:
    """hpt_bvh_device_build_host, the definition of Scene.rebuild_device on the host (no device needed): the Morton-order
    linear BVH over `triangles`, refitted to new_triangles when they are given.  The keys of export_bvh_host and, under
    "build", the fields of hpt_device_build_info that describe the tree (bvh_depth may exceed 30: the device falls back then)."""
    lib = load_library()
    lights = np.ascontiguousarray(lights, LIGHT)
    spheres = np.ascontiguousarray(spheres, SPHERE)
    triangles = np.ascontiguousarray(triangles, TRIANGLE)
    if new_triangles is not None:
        new_triangles = np.ascontiguousarray(new_triangles, TRIANGLE)
        if len(new_triangles) != len(triangles):
            raise HptError("hpt error 1: an update keeps the triangle count: %d triangles, %d were handed over" % (len(triangles), len(new_triangles)))
    binfo = DeviceBuildInfo()
    out = _export_bvh(lambda info, qn, qcap, tr, tcap: lib.hpt_bvh_device_build_host(
        _vp(lights), len(lights), _vp(spheres), len(spheres), _vp(triangles), _vp(new_triangles) if new_triangles is not None else None,
        len(triangles), info, C.byref(binfo), qn, qcap, tr, tcap))
    out["build"] = {n: getattr(binfo, n) for n, _ in binfo._fields_}
    return out


def device_build_bounded_bvh_host(lights, spheres, triangles, new_triangles=None, max_depth=0) -> dict:
    """hpt_bvh_device_build_bounded_host, the definition of Scene.rebuild_device_bounded on the host (no device needed).
    The keys of device_build_bvh_host and, under "bounded", dict(max_depth, forced_nodes, first_forced_level)."""
    lib = load_library()
    lights = np.ascontiguousarray(lights, LIGHT)
    spheres = np.ascontiguousarray(spheres, SPHERE)
    triangles = np.ascontiguousarray(triangles, TRIANGLE)
    if new_triangles is not None:
        new_triangles = np.ascontiguousarray(new_triangles, TRIANGLE)
        if len(new_triangles) != len(triangles):
            raise HptError("hpt error 1: an update keeps the triangle count: %d triangles, %d were handed over" % (len(triangles), len(new_triangles)))
    binfo = DeviceBuildInfo(); bb = BoundedBuildInfo()
    out = _export_bvh(lambda info, qn, qcap, tr, tcap: lib.hpt_bvh_device_build_bounded_host(
        _vp(lights), len(lights), _vp(spheres), len(spheres), _vp(triangles), _vp(new_triangles) if new_triangles is not None else None,
        len(triangles), info, C.byref(binfo), qn, qcap, tr, tcap, C.c_int(int(max_depth)), C.byref(bb)))
    out["build"] = {n: getattr(binfo, n) for n, _ in binfo._fields_}
    out["bounded"] = {n: getattr(bb, n) for n, _ in bb._fields_ if n != "reserved"}
    return out


def pose_host(triangles, tri_part, xforms) -> np.ndarray:
    """hpt_pose_host, the definition of Scene.pose on the host (no device needed): the records with every vertex posed by
    its part's record of xforms ([num_parts, 3, 4] float32).  tri_part None: one part."""
    tr = np.ascontiguousarray(triangles, TRIANGLE)
    tp = np.ascontiguousarray(tri_part, np.int32) if tri_part is not None else None
    x = np.ascontiguousarray(xforms, np.float32)
    if x.size % 12:
        raise HptError("hpt error 1: pose_host: twelve floats per part")
    if tp is not None and len(tp) != len(tr):
        raise HptError("hpt error 1: pose_host: one part index per triangle (%d triangles, %d indices)" % (len(tr), len(tp)))
    out = np.zeros(len(tr), TRIANGLE)
    _check(load_library().hpt_pose_host(_vp(tr), len(tr), _vp(tp) if tp is not None else None, _vp(x), x.size // 12, _vp(out)))
    return out


def _skin_arrays(what, corner_bone, corner_weight):
    b = np.ascontiguousarray(corner_bone, np.int32)
    w = np.ascontiguousarray(corner_weight, np.float32)
    if b.size % 12 or w.size != b.size:
        raise HptError("hpt error 1: %s: four bones and four weights per corner, three corners per triangle (%d bones, %d weights)"
                       % (what, b.size, w.size))
    return b, w


def skin_host(triangles, corner_bone, corner_weight, xforms) -> np.ndarray:
    """hpt_skin_host, the definition of Scene.skin on the host (no device needed): the records with every corner skinned
    by its four influences over xforms ([num_bones, 3, 4] float32)."""
    tr = np.ascontiguousarray(triangles, TRIANGLE)
    b, w = _skin_arrays("skin_host", corner_bone, corner_weight)
    x = np.ascontiguousarray(xforms, np.float32)
    if x.size % 12:
        raise HptError("hpt error 1: skin_host: twelve floats per bone")
    if b.size != len(tr) * 12:
        raise HptError("hpt error 1: skin_host: twelve influences per triangle (%d triangles, %d influences)" % (len(tr), b.size))
    out = np.zeros(len(tr), TRIANGLE)
    _check(load_library().hpt_skin_host(_vp(tr), len(tr), _vp(b), _vp(w), _vp(x), x.size // 12, _vp(out)))
    return out


def _morph_arrays(what, target_begin, entry_corner, entry_delta):
    tb = np.ascontiguousarray(target_begin, np.int32).reshape(-1)
    ec = np.ascontiguousarray(entry_corner, np.int32).reshape(-1)
    ed = np.ascontiguousarray(entry_delta, np.float32).reshape(-1)
    if tb.size < 1 or ed.size != ec.size * 3:
        raise HptError("hpt error 1: %s: num_targets + 1 values of target_begin and three floats per entry (%d values, %d corners, %d floats)"
                       % (what, tb.size, ec.size, ed.size))
    return tb, ec, ed


def morph_host(triangles, target_begin, entry_corner, entry_delta, weights) -> np.ndarray:
    """hpt_morph_host, the definition of Scene.morph on the host (no device needed): the records with every corner moved by
    the weighted deltas of the active targets that name it.  The morph stage only: compose with pose_host or skin_host."""
    tr = np.ascontiguousarray(triangles, TRIANGLE)
    tb, ec, ed = _morph_arrays("morph_host", target_begin, entry_corner, entry_delta)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    if w.size != tb.size - 1:
        raise HptError("hpt error 1: morph_host: one weight per target (%d targets, %d weights)" % (tb.size - 1, w.size))
    out = np.zeros(len(tr), TRIANGLE)
    _check(load_library().hpt_morph_host(_vp(tr), len(tr), _vp(tb), _vp(ec), _vp(ed), ec.size, tb.size - 1, _vp(w), _vp(out)))
    return out


def update_check(scene, triangles, num_triangles=None) -> None:
    """hpt_scene_update_check: raises HptError for what Scene.update_triangles would refuse (scene may be None,
    triangles may be None with a count given); touches no device."""
    tr = np.ascontiguousarray(triangles, TRIANGLE) if triangles is not None else None
    n = len(tr) if num_triangles is None else int(num_triangles)
    _check(load_library().hpt_scene_update_check(scene._h if scene is not None else None, _vp(tr) if tr is not None else None, n))


def probe_functions(records) -> np.ndarray:
    """Device BSDF / Fresnel / GGX functions on [n, 24] float32 records -> [n, 40] results (tests; include/hpt.h)."""
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, 24)
    out = np.zeros((len(rec), 40), np.float32)
    _check(load_library().hpt_probe_functions(_vp(rec), len(rec), _vp(out)))
    return out


def tonemap(image) -> np.ndarray:
    """8-bit output stage on the device (reference src/main_cli.cpp:225-242): [H, W, 3] float32 -> uint8 RGB."""
    img = np.ascontiguousarray(image, np.float32)
    out = np.zeros(img.shape, np.uint8)
    _check(load_library().hpt_tonemap_host(_vp(img), _vp(out), C.c_int64(img.size // 3), 0))
    return out


def tonemap_device(d_linear_rgb, d_rgb8, num_pixels: int, bgr: bool = False, stream: int = 0):
    """hpt_tonemap on device buffers (ints or torch tensors), enqueued on `stream`: the step after Denoiser.run."""
    _check(load_library().hpt_tonemap(_dptr(d_linear_rgb), _dptr(d_rgb8), C.c_int64(num_pixels), 1 if bgr else 0, C.c_void_p(stream)))


def wrapper_set_devices(n: int) -> None:
    """Number of devices the one-shot wrappers (pt_render_wrapper / bdpt_render_wrapper) fan out over."""
    _check(load_library().hpt_wrapper_set_devices(int(n)))


def untile(d_gathered_ptr: int, d_image_ptr: int, W: int, H: int, params: Params, stream: int = 0):
    """[rank][local slot] packed framebuffers -> row-major W*H image (device pointers)."""
    _check(load_library().hpt_untile(C.c_void_p(d_gathered_ptr), C.c_void_p(d_image_ptr), W, H, C.byref(params), C.c_void_p(stream)))


def wrapper_cache_clear() -> None:
    """Releases the scene the one-shot wrappers keep between calls (include/hpt.h)."""
    load_library().hpt_wrapper_cache_clear()


def pt_render_wrapper(lights, spheres, triangles, camera, W, H, eye_depth, spp, seed=-1,
                      scene_min=(0, 0, 0), scene_max=(0, 0, 0), light_depth=4, light_sample=8) -> np.ndarray:
    """One-shot render with the reference's pt_render_wrapper argument list
    (reference include/pt_cu.cuh:6-13)."""
    lib = load_library()
    lights = np.ascontiguousarray(lights, LIGHT)
    spheres = np.ascontiguousarray(spheres, SPHERE)
    triangles = np.ascontiguousarray(triangles, TRIANGLE)
    cam = np.ascontiguousarray(camera, CAMERA).reshape(1)
    img = np.empty((H, W, 3), np.float32)
    mn = (C.c_float * 3)(*scene_min)
    mx = (C.c_float * 3)(*scene_max)
    _check(lib.hpt_pt_render_wrapper(_vp(lights), len(lights), _vp(spheres), len(spheres), _vp(triangles), len(triangles),
                                     mn, mx, _vp(cam), _vp(img), W, H, light_depth, light_sample, eye_depth, spp,
                                     C.c_int64(seed)))
    return img


def ppm_render_wrapper(lights, spheres, triangles, camera, W, H, scene_min, scene_max, light_depth=4, light_sample=8,
                       eye_depth=4, spp=1, seed=-1) -> np.ndarray:
    """One-shot photon-mapping pass with the reference's ppm_render_wrapper argument list (include/ppm_cu.cuh:8-15):
    one pass whatever spp is, the bounds as given, lights as given."""
    lib = load_library()
    lights = np.ascontiguousarray(lights, LIGHT)
    spheres = np.ascontiguousarray(spheres, SPHERE)
    triangles = np.ascontiguousarray(triangles, TRIANGLE)
    cam = np.ascontiguousarray(camera, CAMERA).reshape(1)
    img = np.empty((H, W, 3), np.float32)
    mn = (C.c_float * 3)(*scene_min)
    mx = (C.c_float * 3)(*scene_max)
    _check(lib.hpt_ppm_render_wrapper(_vp(lights), len(lights), _vp(spheres), len(spheres), _vp(triangles), len(triangles),
                                      mn, mx, _vp(cam), _vp(img), W, H, light_depth, light_sample, eye_depth, spp, C.c_int64(seed)))
    return img
