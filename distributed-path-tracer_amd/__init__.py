"""distributed-path-tracer_amd — MI355X-native ray-intersection + Monte-Carlo shading integrator.

Thin ctypes binding of the C ABI in include/ptx.h (libptx_hip.so, built from csrc/ by
`__graft_entry__.build()` / `make -C distributed-path-tracer_amd/csrc`) plus a host-side mirror of the
reference's renderer interface (core::renderer, path_tracer_lib/path_tracer/core/renderer.hpp:15-36):
same field names, same defaults, `load_gltf(path)` and `render() -> PNG bytes`.

There is no CPU implementation in this package: every compute entry point goes to the HIP library
and raises PtxError when the library or a GPU is missing.

The directory name contains '-', so import it with importlib:
    ptx = importlib.import_module("distributed-path-tracer_amd")
"""
import atexit
import ctypes as C
import os
import re
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PTX_LIB") or os.path.join(_HERE, "libptx_hip.so")  # PTX_LIB: experiment builds only
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ptx.h")

OK, ERR_INVALID, ERR_IO, ERR_PARSE, ERR_NO_CAMERA, ERR_NO_DEVICE, ERR_HIP, ERR_UNSUPPORTED = range(8)
NO_SUN_LIGHT = 0xFFFFFFFF  # core::renderer::no_sun_light, renderer.hpp:19

(ARR_MODEL_XFORM, ARR_MODEL_AABB, ARR_MODEL_SURF, ARR_SURF_RANGE, ARR_MESH_AABB, ARR_VERTICES, ARR_TRIANGLES,
 ARR_MATERIALS, ARR_KD_NODES, ARR_KD_REFS, ARR_CAMERA, ARR_SUN, ARR_MODEL_NAMES, ARR_TEXTURES, ARR_TEXELS, ARR_SURF_TEX, ARR_TEXELS_F32,
 ARR_LIGHT_TRIS, ARR_LIGHT_CDF, ARR_LIGHT_GEOM, ARR_TRI_ISECT, ARR_RES_NODES, ARR_RES_REFS, ARR_RES_TRIS, ARR_LDS_ROOT,
 ARR_RES_PLAN, ARR_ENV_ROW_CDF, ARR_ENV_CELL_CDF, ARR_PUNCTUAL, ARR_PUNCTUAL_CDF, ARR_LENS, ARR_LDS_SHAPE, ARR_SURF_AUX,
 ARR_MOTION_XFORM, ARR_MOTION_MOVED, ARR_MOTION_CAMERA, ARR_PUNCTUAL_TREE, ARR_LIGHT_TREE, ARR_LIGHT_PATH) = range(39)
LIGHT_PICK_CDF, LIGHT_PICK_TREE = 0, 1   # ptx_light_pick: how a light sample picks its emissive triangle (Scene.set_light_pick)
_LIGHT_PICK_NAMES = {"cdf": LIGHT_PICK_CDF, "tree": LIGHT_PICK_TREE}
PUNCTUAL_PICK_CDF, PUNCTUAL_PICK_TREE = 0, 1   # ptx_punctual_pick: how a punctual sample picks its light (Scene.set_punctual_pick)
LDS_LEAF_ORDER_BIT = 0x80000000  # ARR_LDS_ROOT: the surface's resident records are leaf-ordered (flat_scene.hpp)
LDS_LEAF_ONLY_BIT = 0x40000000   # ARR_LDS_SHAPE: the surface's resident tree is a single leaf
LDS_COMPLETE_BIT = 0x20000000    # ARR_LDS_SHAPE: ... is complete (no missing child) with at most KD_SHAPE_MAX_BRANCH_LEVELS branch levels
LDS_ROOT_MASK = 0x1FFFFFFF
KD_SHAPE_MAX_BRANCH_LEVELS = 3   # kShapeMaxBranchLevels = kRegStack
AUX_CHAIN_BIT = 1    # ARR_SURF_AUX, word 0: the surface's resident, leaf-ordered tree is a chain: every branch has exactly one child (none with PTX_KD_SHAPES=0)


class PtxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"ptx error {code}: {msg}")
        self.code = code


class WorkItem(C.Structure):
    _fields_ = [("mesh_name", C.c_char_p), ("primitives", C.POINTER(C.c_int32)), ("n_primitives", C.c_uint32)]


class LoadOpts(C.Structure):
    _fields_ = [("camera_index", C.c_uint32), ("sun_light_index", C.c_uint32), ("filter_primitives", C.c_uint32),
                ("n_work", C.c_uint32), ("work", C.POINTER(WorkItem))]


class WorkerEvent(C.Structure):
    _fields_ = [("num_workers", C.c_int32), ("n_work_meshes", C.c_uint32), ("worker_id", C.c_char * 64),
                ("scene_root", C.c_char * 256), ("scene_bucket", C.c_char * 128)]


class SceneDesc(C.Structure):
    _fields_ = [("n_models", C.c_uint32), ("model_xform", C.c_void_p), ("model_surf", C.c_void_p),
                ("n_surfaces", C.c_uint32), ("surf_range", C.c_void_p), ("vertices", C.c_void_p),
                ("triangles", C.c_void_p), ("materials", C.c_void_p), ("camera", C.c_void_p), ("sun", C.c_void_p)]


class Camera(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("basis", C.c_float * 9), ("yfov", C.c_float), ("lens_radius", C.c_float),
                ("focus_distance", C.c_float), ("blades", C.c_uint32), ("blade_rotation", C.c_float)]


class MotionPrev(C.Structure):
    _fields_ = [("camera", C.POINTER(Camera)), ("model_xform", C.c_void_p), ("n_models", C.c_uint32)]


class Motion(C.Structure):
    _fields_ = [("begin_camera", C.POINTER(Camera)), ("begin_model_xform", C.c_void_p), ("n_models", C.c_uint32),
                ("shutter_open", C.c_float), ("shutter_close", C.c_float)]


class SceneInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_models", "n_surfaces", "n_vertices", "n_triangles", "n_kd_nodes", "n_kd_refs",
                                          "kd_max_depth", "has_sun", "geometry_bytes", "lds_resident", "n_textures")]


class RenderCfg(C.Structure):
    _fields_ = [("W", C.c_uint32), ("H", C.c_uint32), ("spp", C.c_uint32), ("bounces", C.c_uint32),
                ("env", C.c_float * 3), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32),
                ("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("sample0", C.c_uint32), ("spp_per_pass", C.c_uint32), ("integrator", C.c_uint32),
                ("shard_index", C.c_uint32), ("shard_count", C.c_uint32), ("shard_tile", C.c_uint32)]


INTEGRATOR_LIB, INTEGRATOR_WORKER = 0, 1   # ptx_integrator


class RenderStats(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("samples", C.c_uint64), ("passes", C.c_uint64), ("kernel_ms", C.c_double)]


class AovBuffers(C.Structure):
    _fields_ = [("albedo_cov", C.c_void_p), ("normal_depth", C.c_void_p)]


class DenoiseCfg(C.Structure):
    _fields_ = [("W", C.c_uint32), ("H", C.c_uint32), ("spp_a", C.c_uint32), ("spp_b", C.c_uint32), ("iterations", C.c_uint32),
                ("sigma_l", C.c_float), ("sigma_n", C.c_float), ("sigma_z", C.c_float)]


class DenoiseStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("iterations", C.c_uint32), ("workspace_bytes", C.c_uint64)]


class DenoiseCountsCfg(C.Structure):
    _fields_ = [("W", C.c_uint32), ("H", C.c_uint32), ("guide_spp", C.c_uint32), ("iterations", C.c_uint32),
                ("sigma_l", C.c_float), ("sigma_n", C.c_float), ("sigma_z", C.c_float)]


class TemporalHistory(C.Structure):
    _fields_ = [("color", C.c_void_p), ("moments", C.c_void_p), ("geometry", C.c_void_p)]


class TemporalCfg(C.Structure):
    _fields_ = [("W", C.c_uint32), ("H", C.c_uint32), ("spp_a", C.c_uint32), ("spp_b", C.c_uint32), ("iterations", C.c_uint32),
                ("sigma_l", C.c_float), ("sigma_n", C.c_float), ("sigma_z", C.c_float), ("max_history", C.c_uint32),
                ("tau_z", C.c_float), ("tau_n", C.c_float)]


TEMPORAL_SEARCH_3X3, TEMPORAL_UNIT_NORMALS = 1, 2   # ptx_temporal_counts_cfg.flags


class TemporalCountsCfg(C.Structure):
    _fields_ = [("W", C.c_uint32), ("H", C.c_uint32), ("guide_spp", C.c_uint32), ("iterations", C.c_uint32),
                ("sigma_l", C.c_float), ("sigma_n", C.c_float), ("sigma_z", C.c_float), ("max_history", C.c_uint32),
                ("tau_z", C.c_float), ("tau_n", C.c_float), ("flags", C.c_uint32)]


class TemporalStats(C.Structure):
    _fields_ = [("filter", DenoiseStats), ("accumulate_ms", C.c_double), ("reprojected", C.c_uint64), ("reset", C.c_uint64)]


class AdaptiveCfg(C.Structure):
    _fields_ = [("min_spp", C.c_uint32), ("step_spp", C.c_uint32), ("threshold", C.c_float)]


class AdaptiveStats(C.Structure):
    _fields_ = [("render", RenderStats), ("rounds", C.c_uint32), ("active_last", C.c_uint32), ("select_ms", C.c_double)]


class NeeCfg(C.Structure):
    _fields_ = [("flags", C.c_uint32)]


class NeeStats(C.Structure):
    _fields_ = [("render", RenderStats), ("n_lights", C.c_uint32), ("light_area", C.c_float), ("light_samples", C.c_uint64),
                ("light_visible", C.c_uint64)]


class AdaptiveNeeStats(C.Structure):
    _fields_ = [("nee", NeeStats), ("rounds", C.c_uint32), ("active_last", C.c_uint32), ("select_ms", C.c_double)]


NEE_NO_LIGHT_SAMPLES = 1   # ptx_nee_cfg.flags
NEE_FUSED = 4              # one kernel launch per pass where render() runs the fused kernel; ignored on the queue route
NEE_ENV_SAMPLES = 16       # the light sample may go towards the environment map; ignored without a map or with a black one
NEE_SAMPLER_PDF = 64       # MIS weights on the density of LIB's BSDF sampler instead of LIB's pdf value: the frame's expectation is LIB's
NEE_FUSED_MOTION = 8192    # beside NEE_FUSED: the fused kernel with a time per lane under active motion (set_motion); alone, or without active motion: nothing


def NEE_CANDIDATES(m):
    """PTX_NEE_CANDIDATES(m): bits 8..11 of ptx_nee_cfg.flags. The light sample of a vertex is picked among m = 1 .. 16 candidates in
    proportion to their unshadowed contributions, one shadow ray for the pick; m = 1 is 0, the call without the bits."""
    if not 1 <= int(m) <= 16:
        raise ValueError(f"NEE_CANDIDATES: m = {m} is outside 1 .. 16")
    return (int(m) - 1) << 8


class KernelTiming(C.Structure):
    _fields_ = [("pipeline", C.c_uint32), ("steps", C.c_uint32), ("classify_ms", C.c_double), ("traverse_ms", C.c_double), ("shade_ms", C.c_double),
                ("fused_ms", C.c_double), ("fused_launches", C.c_uint32), ("pool_overflows", C.c_uint32), ("pool_pairs", C.c_uint64),
                ("peak_pairs", C.c_uint64), ("slab_paths", C.c_uint64), ("workspace_bytes", C.c_uint64), ("traverse_drain_frac", C.c_double)]


class Rays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ox", "oy", "oz", "dx", "dy", "dz")]


class Hits(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("distance", "surface", "triangle", "b0", "b1", "b2", "px", "py", "pz",
                                          "nx", "ny", "nz", "u", "v")]


MASK_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t)   # ptx_mask_exchange_fn(user, mask, n_bytes) -> status


_lib = None
_live = weakref.WeakSet()   # scenes and contexts still open; closed before interpreter teardown (atexit)
                            # so that no HIP call is made after the HIP runtime's own static destructors ran


@atexit.register
def _close_all():
    for o in sorted(list(_live), key=lambda x: isinstance(x, Context)):   # scenes first, then contexts
        try:
            o.close()
        except Exception:
            pass


def declared_symbols():
    """Entry points declared in include/ptx.h."""
    with open(HEADER_PATH) as fh:
        txt = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ptx_[a-z_0-9]+)\s*\(", txt)))


def _preload_hip_runtime():
    """One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 (+ HSA runtime) and a second
    copy from /opt/rocm in the same process leaves whichever initialises second without a GPU. When torch is
    installed, load ITS runtime first so that libptx_hip.so's DT_NEEDED libamdhip64.so.7 binds to the same one,
    whatever the import order. (torch itself is not imported here.)"""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            try:
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def lib():
    """Load libptx_hip.so. Raises (never falls back) when it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PtxError(ERR_NO_DEVICE, f"{LIB_PATH} is not built; run __graft_entry__.build() — there is no fallback path")
        _preload_hip_runtime()
        L = C.CDLL(LIB_PATH)
        L.ptx_last_error.restype = C.c_char_p
        L.ptx_version.restype = C.c_char_p
        L.ptx_ctx_stream.restype = C.c_void_p
        L.ptx_ctx_stream.argtypes = [C.c_void_p]
        L.ptx_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        L.ptx_ctx_destroy.argtypes = [C.c_void_p]
        L.ptx_ctx_synchronize.argtypes = [C.c_void_p]
        L.ptx_ctx_set_timing.argtypes = [C.c_void_p, C.c_int]
        L.ptx_ctx_get_timing.argtypes = [C.c_void_p, C.POINTER(KernelTiming)]
        L.ptx_scene_load_gltf.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(LoadOpts), C.POINTER(C.c_void_p)]
        L.ptx_worker_event_load.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(RenderCfg), C.POINTER(WorkerEvent)]
        L.ptx_scene_from_arrays.argtypes = [C.c_void_p, C.POINTER(SceneDesc), C.POINTER(C.c_void_p)]
        L.ptx_scene_destroy.argtypes = [C.c_void_p]
        L.ptx_scene_set_environment.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
        L.ptx_scene_set_punctual_lights.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ptx_scene_set_punctual_pick.argtypes = [C.c_void_p, C.c_uint32]
        L.ptx_scene_get_punctual_pick.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.ptx_punctual_pick_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.ptx_scene_set_light_pick.argtypes = [C.c_void_p, C.c_uint32]
        L.ptx_scene_get_light_pick.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.ptx_light_pick_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.ptx_light_pmf_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.ptx_scene_set_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
        L.ptx_scene_get_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
        L.ptx_scene_set_model_xforms.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        L.ptx_scene_set_motion.argtypes = [C.c_void_p, C.POINTER(Motion)]
        L.ptx_scene_motion_state.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
        L.ptx_intersect_batch_motion.argtypes = [C.c_void_p, C.POINTER(Rays), C.c_void_p, C.c_size_t, C.POINTER(Hits)]
        L.ptx_camera_lens_rays_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.ptx_gltf_read_punctual_lights.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t]
        L.ptx_gltf_read_punctual_lights.restype = C.c_int64
        L.ptx_scene_get_info.argtypes = [C.c_void_p, C.POINTER(SceneInfo)]
        L.ptx_scene_get_array.restype = C.c_int64
        L.ptx_scene_get_array.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.ptx_render.argtypes = [C.c_void_p, C.POINTER(RenderCfg), C.c_void_p, C.POINTER(RenderStats)]
        L.ptx_render_transparent.argtypes = [C.c_void_p, C.POINTER(RenderCfg), C.c_void_p, C.c_void_p, C.POINTER(RenderStats)]
        L.ptx_render_aov.argtypes = [C.c_void_p, C.POINTER(RenderCfg), C.POINTER(AovBuffers), C.POINTER(RenderStats)]
        L.ptx_render_motion.argtypes = [C.c_void_p, C.POINTER(RenderCfg), C.POINTER(MotionPrev), C.c_void_p, C.POINTER(RenderStats)]
        L.ptx_render_emission.argtypes = [C.c_void_p, C.POINTER(RenderCfg), C.c_void_p, C.POINTER(RenderStats)]
        L.ptx_emission_split.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p]
        L.ptx_emission_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t, C.c_void_p]
        L.ptx_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseCfg), C.c_void_p, C.c_void_p, C.POINTER(AovBuffers), C.c_void_p, C.POINTER(DenoiseStats)]
        L.ptx_render_adaptive.argtypes = [C.c_void_p, C.POINTER(RenderCfg), C.POINTER(AdaptiveCfg), C.c_void_p, C.c_void_p, C.POINTER(AdaptiveStats)]
        L.ptx_render_nee.argtypes = [C.c_void_p, C.POINTER(RenderCfg), C.POINTER(NeeCfg), C.c_void_p, C.POINTER(NeeStats)]
        L.ptx_render_adaptive_nee.argtypes = [C.c_void_p, C.POINTER(RenderCfg), C.POINTER(AdaptiveCfg), C.POINTER(NeeCfg), C.c_void_p, C.c_void_p, C.POINTER(AdaptiveNeeStats)]
        L.ptx_denoise_counts.argtypes = [C.c_void_p, C.POINTER(DenoiseCountsCfg), C.c_void_p, C.c_void_p, C.POINTER(AovBuffers), C.c_void_p, C.POINTER(DenoiseStats)]
        L.ptx_denoise_temporal.argtypes = [C.c_void_p, C.POINTER(TemporalCfg), C.c_void_p, C.c_void_p, C.POINTER(AovBuffers), C.c_void_p,
                                           C.POINTER(TemporalHistory), C.POINTER(TemporalHistory), C.c_void_p, C.POINTER(TemporalStats)]
        L.ptx_denoise_temporal_counts.argtypes = [C.c_void_p, C.POINTER(TemporalCountsCfg), C.c_void_p, C.c_void_p, C.POINTER(AovBuffers), C.c_void_p,
                                                  C.POINTER(TemporalHistory), C.POINTER(TemporalHistory), C.c_void_p, C.POINTER(TemporalStats)]
        L.ptx_adaptive_select.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        L.ptx_accum_mean.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.ptx_ctx_set_mask_exchange.argtypes = [C.c_void_p, MASK_EXCHANGE_FN, C.c_void_p, C.c_void_p, C.c_size_t]
        L.ptx_ctx_get_mask_exchange_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
        L.ptx_intersect_batch.argtypes = [C.c_void_p, C.POINTER(Rays), C.c_size_t, C.POINTER(Hits)]
        L.ptx_tonemap_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        L.ptx_pbr_eval_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.ptx_exact_math_check.argtypes = [C.c_void_p, C.c_void_p]
        L.ptx_shade_consts_check.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.ptx_leaf_intersect_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.ptx_camera_rays_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.ptx_material_eval_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.ptx_reduce_framebuffer.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.ptx_encode_png.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.ptx_free.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _check(rc):
    if rc != OK:
        raise PtxError(rc, lib().ptx_last_error().decode(errors="replace"))


def _torch():
    import torch
    return torch


def _ptr(x):
    """Device pointer of a torch tensor, host pointer of a numpy array, or a raw int."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    if isinstance(x, np.ndarray):
        assert x.flags["C_CONTIGUOUS"]
        return x.ctypes.data
    return x.data_ptr()  # torch.Tensor


class Context:
    """One per GPU (ptx_ctx): HIP device, stream and workspace."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib().ptx_ctx_create(device, C.byref(h)))
        self.h = h
        self.device = device
        _live.add(self)

    @property
    def stream(self):
        return lib().ptx_ctx_stream(self.h)

    def synchronize(self):
        _check(lib().ptx_ctx_synchronize(self.h))

    def set_timing(self, on=True):
        """ptx_ctx_set_timing: collect per-kernel HIP-event times of the queue-based pipeline in renders that ask for stats."""
        _check(lib().ptx_ctx_set_timing(self.h, int(bool(on))))

    def timing(self):
        """ptx_ctx_get_timing: where the time of the last render with stats went, and the workspace it used."""
        t = KernelTiming()
        _check(lib().ptx_ctx_get_timing(self.h, C.byref(t)))
        return {n: getattr(t, n) for n, _ in KernelTiming._fields_}

    def reduce_framebuffer(self, nccl_comm, accum, root=0):
        """ptx_reduce_framebuffer: in-place RCCL sum-reduce of a device-resident accumulation buffer onto `root`, on this
        context's stream. `nccl_comm`: the raw ncclComm_t (an int / ctypes pointer) of a communicator the caller created."""
        n = int(accum.numel()) if hasattr(accum, "numel") else int(accum.size)
        comm = nccl_comm if isinstance(nccl_comm, C.c_void_p) else C.c_void_p(int(nccl_comm))
        _check(lib().ptx_reduce_framebuffer(self.h, comm, _ptr(accum), n, root))

    def pbr_eval(self, records):
        """ptx_pbr_eval_batch: records [n,14] float32 (normal, outcoming, incoming, u1, u2, roughness, cos_theta, ior) ->
        [n,15] float32 (rand_cone_vec, importance_diffuse, importance_specular, pdf_diffuse, pdf_specular, fresnel, reflect)."""
        a = np.ascontiguousarray(records, np.float32).reshape(-1, 14)
        out = np.zeros((len(a), 15), np.float32)
        _check(lib().ptx_pbr_eval_batch(self.h, a.ctypes.data, len(a), out.ctypes.data))
        return out

    EXACT_MATH_FORMS = ("rcp", "sqrt", "rsqrt")

    def exact_math_check(self):
        """ptx_exact_math_check: the kernels' short reciprocal / square-root forms against the IEEE expressions over every float
        pattern. Returns {form: number of results whose bits differ (NaN equals NaN)}."""
        out = np.zeros(len(self.EXACT_MATH_FORMS), np.uint64)
        _check(lib().ptx_exact_math_check(self.h, out.ctypes.data))
        return {n: int(v) for n, v in zip(self.EXACT_MATH_FORMS, out)}

    def shade_consts_check(self, materials):
        """ptx_shade_consts_check: materials [n,9] float32 (roughness, metallic, ior, albedo rgb, emissive rgb). The per-material constants
        the scene builder puts into a shade record for each row against the path vertex's own expressions evaluated on the device.
        Returns the number of words whose bits differ (NaN equals NaN)."""
        a = np.ascontiguousarray(materials, np.float32).reshape(-1, 9)
        out = np.zeros(1, np.uint64)
        _check(lib().ptx_shade_consts_check(self.h, a.ctypes.data, len(a), out.ctypes.data))
        return int(out[0])

    def leaf_intersect(self, corners, rays, refs=None, leaf_ordered=False):
        """ptx_leaf_intersect_batch: the fused kernels' leaf loop on one leaf holding the triangles corners [n_tri,9] (a, b, c), tested in
        the order of refs (a permutation, None = identity), in the per-triangle layout behind refs (leaf_ordered 0 / False), the
        leaf-ordered one in global memory (1 / True) or the leaf-ordered one staged into LDS (2); rays [n,7]
        float32 (origin, unit direction, max_dist). -> {"t", "beta", "gamma": float32 [n], "triangle": int32 [n], -1 = miss}."""
        c = np.ascontiguousarray(corners, np.float32).reshape(-1, 9)
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 7)
        p = None if refs is None else np.ascontiguousarray(refs, np.uint32)
        if p is not None and p.shape != (len(c),):
            raise ValueError("refs must hold one reference per triangle")
        out = np.zeros((len(r), 3), np.float32)
        tri = np.full(len(r), -1, np.int32)
        _check(lib().ptx_leaf_intersect_batch(self.h, c.ctypes.data, len(c), None if p is None else p.ctypes.data, int(leaf_ordered),
                                              r.ctypes.data, len(r), out.ctypes.data, tri.ctypes.data))
        return {"t": out[:, 0].copy(), "beta": out[:, 1].copy(), "gamma": out[:, 2].copy(), "triangle": tri}

    def tonemap_encode(self, accum, W, H, spp, out=None):
        """accum: [H,W,4] float32 sums (numpy or torch-on-GPU). Returns/filles RGBA8 [H,W,4]."""
        ret = out if out is not None else np.zeros((H, W, 4), np.uint8)
        _check(lib().ptx_tonemap_encode(self.h, _ptr(accum), W, H, spp, _ptr(ret)))
        return ret

    def denoise(self, a, b, albedo_cov, normal_depth, spp_a, spp_b, iterations=0, sigma_l=0, sigma_n=0, sigma_z=0, out=None, want_stats=True):
        """ptx_denoise: variance-guided a-trous filter. a, b: [H,W,4] float32 radiance SUMS of two disjoint sample ranges of one frame
        (Scene.render of spp_a and spp_b samples); albedo_cov, normal_depth: the Scene.render_aov SUMS over all spp_a + spp_b samples;
        all numpy or all torch-on-GPU. iterations 0 = 5 (at most 8), sigmas 0 = the defaults 4, 0.5, 0.1. out: [H,W,4] buffer of the same
        kind for the filtered MEANS (may be a or b itself; None = a new one). Returns (out, stats dict or None)."""
        bufs = [a, b, albedo_cov, normal_depth] + ([out] if out is not None else [])
        shape = tuple(a.shape)
        if len(shape) != 3 or shape[2] != 4 or any(tuple(x.shape) != shape for x in bufs):
            raise ValueError(f"denoise: every buffer must be [H, W, 4] of one size, got {[tuple(x.shape) for x in bufs]}")
        if out is None:
            out = np.empty(shape, np.float32) if isinstance(a, np.ndarray) else a.new_empty(shape)   # no fill kernel on another stream
        cfg = DenoiseCfg(shape[1], shape[0], spp_a, spp_b, iterations, sigma_l, sigma_n, sigma_z)
        guides = AovBuffers(_ptr(albedo_cov), _ptr(normal_depth))
        st = DenoiseStats()
        _check(lib().ptx_denoise(self.h, C.byref(cfg), _ptr(a), _ptr(b), C.byref(guides), _ptr(out), C.byref(st) if want_stats else None))
        return out, (dict(kernel_ms=st.kernel_ms, iterations=st.iterations, workspace_bytes=st.workspace_bytes) if want_stats else None)

    def denoise_counts(self, a, b, albedo_cov, normal_depth, guide_spp, iterations=0, sigma_l=0, sigma_n=0, sigma_z=0, out=None, want_stats=True):
        """ptx_denoise_counts: denoise() for half-buffers whose alpha channel is the per-pixel sample count (Scene.render_adaptive,
        Scene.render_adaptive_nee). albedo_cov, normal_depth: the Scene.render_aov SUMS over guide_spp samples of every pixel — for an adaptive
        frame the first min_spp samples. Everything else as in denoise(). Returns (out, stats dict or None)."""
        bufs = [a, b, albedo_cov, normal_depth] + ([out] if out is not None else [])
        shape = tuple(a.shape)
        if len(shape) != 3 or shape[2] != 4 or any(tuple(x.shape) != shape for x in bufs):
            raise ValueError(f"denoise_counts: every buffer must be [H, W, 4] of one size, got {[tuple(x.shape) for x in bufs]}")
        if out is None:
            out = np.empty(shape, np.float32) if isinstance(a, np.ndarray) else a.new_empty(shape)   # no fill kernel on another stream
        cfg = DenoiseCountsCfg(shape[1], shape[0], guide_spp, iterations, sigma_l, sigma_n, sigma_z)
        guides = AovBuffers(_ptr(albedo_cov), _ptr(normal_depth))
        st = DenoiseStats()
        _check(lib().ptx_denoise_counts(self.h, C.byref(cfg), _ptr(a), _ptr(b), C.byref(guides), _ptr(out), C.byref(st) if want_stats else None))
        return out, (dict(kernel_ms=st.kernel_ms, iterations=st.iterations, workspace_bytes=st.workspace_bytes) if want_stats else None)

    def denoise_temporal(self, a, b, albedo_cov, normal_depth, motion, spp_a, spp_b, prev=None, next=None, iterations=0, sigma_l=0, sigma_n=0,
                         sigma_z=0, max_history=0, tau_z=0, tau_n=0, out=None, want_out=True, want_stats=True):
        """ptx_denoise_temporal: denoise() with last frame's history reprojected through `motion` and blended in before the filter.
        a, b, albedo_cov, normal_depth as in denoise(); motion: [H,W,4] per-pixel sums of (previous minus current screen position, distance
        from the previous camera, 1). prev: the (color [H,W,4], moments [H,W,2], geometry [H,W,4]) a previous call returned, None for the
        first frame; next: three buffers to receive this frame's history (None = new ones), none of them one of prev's. All numpy or all
        torch-on-GPU. max_history 0 = 32, tau_z and tau_n 0 = 0.1 and 0.9. want_out = False: advance the history only.
        Returns (out or None, next, stats dict or None)."""
        return self._temporal(lib().ptx_denoise_temporal, "denoise_temporal", a, b, albedo_cov, normal_depth, motion, prev, next, out, want_out, want_stats,
                              lambda W, H: TemporalCfg(W, H, spp_a, spp_b, iterations, sigma_l, sigma_n, sigma_z, max_history, tau_z, tau_n))

    def denoise_temporal_counts(self, a, b, albedo_cov, normal_depth, motion, guide_spp, prev=None, next=None, iterations=0, sigma_l=0, sigma_n=0,
                                sigma_z=0, max_history=0, tau_z=0, tau_n=0, flags=0, out=None, want_out=True, want_stats=True):
        """ptx_denoise_temporal_counts: denoise_temporal() for half-buffers whose alpha channel is the per-pixel sample count
        (Scene.render_adaptive, Scene.render_adaptive_nee), with a history counted in samples. albedo_cov, normal_depth, motion: the
        Scene.render_aov and Scene.render_motion SUMS over guide_spp samples of every pixel, for an adaptive frame its first min_spp samples.
        max_history is in samples (0 = min(32 * guide_spp, 1048576)); flags: TEMPORAL_SEARCH_3X3 | TEMPORAL_UNIT_NORMALS. prev is a history this
        call returned, not denoise_temporal's. Everything else, and what is returned, as in denoise_temporal()."""
        return self._temporal(lib().ptx_denoise_temporal_counts, "denoise_temporal_counts", a, b, albedo_cov, normal_depth, motion, prev, next, out, want_out,
                              want_stats, lambda W, H: TemporalCountsCfg(W, H, guide_spp, iterations, sigma_l, sigma_n, sigma_z, max_history, tau_z, tau_n, flags))

    def _temporal(self, fn, who, a, b, albedo_cov, normal_depth, motion, prev, next, out, want_out, want_stats, make_cfg):
        """What denoise_temporal and denoise_temporal_counts share: the shape checks, the buffers they make, the call and the stats."""
        bufs = [a, b, albedo_cov, normal_depth, motion] + ([out] if out is not None else [])
        shape = tuple(a.shape)
        if len(shape) != 3 or shape[2] != 4 or any(tuple(x.shape) != shape for x in bufs):
            raise ValueError(f"{who}: every buffer must be [H, W, 4] of one size, got {[tuple(x.shape) for x in bufs]}")
        hist_shapes = (shape, shape[:2] + (2,), shape)
        for name, h in (("prev", prev), ("next", next)):
            if h is not None and (len(h) != 3 or any(tuple(x.shape) != s for x, s in zip(h, hist_shapes))):
                raise ValueError(f"{who}: {name} must be (color [H,W,4], moments [H,W,2], geometry [H,W,4]) of the frame's size")
        new = (lambda s: np.empty(s, np.float32)) if isinstance(a, np.ndarray) else a.new_empty   # no fill kernel on another stream
        if next is None:
            next = tuple(new(s) for s in hist_shapes)
        if out is None and want_out:
            out = new(shape)
        cfg = make_cfg(shape[1], shape[0])
        guides = AovBuffers(_ptr(albedo_cov), _ptr(normal_depth))
        h_prev = None if prev is None else C.byref(TemporalHistory(*(_ptr(x) for x in prev)))
        h_next = TemporalHistory(*(_ptr(x) for x in next))
        st = TemporalStats()
        _check(fn(self.h, C.byref(cfg), _ptr(a), _ptr(b), C.byref(guides), _ptr(motion), h_prev, C.byref(h_next), _ptr(out) if want_out else None,
                  C.byref(st) if want_stats else None))
        stats = None
        if want_stats:
            stats = dict(kernel_ms=st.filter.kernel_ms, iterations=st.filter.iterations, workspace_bytes=st.filter.workspace_bytes,
                         accumulate_ms=st.accumulate_ms, reprojected=st.reprojected, reset=st.reset)
        return (out if want_out else None), tuple(next), stats

    def adaptive_select(self, a, b, threshold, done=None, want_list=True):
        """ptx_adaptive_select: one decision of ptx_render_adaptive's loop (include/ptx.h has the rule). a, b: [h,w,4] float32 radiance SUMS of
        the two halves; done: [h,w] uint8, read and updated in place (None = zeros); all numpy or all torch-on-GPU. Returns (done, the active
        list — tile-local indices ly * w + lx in the specified order, uint32 numpy or int32 torch; None without want_list —, its length)."""
        shape = tuple(a.shape)
        if len(shape) != 3 or shape[2] != 4 or tuple(b.shape) != shape or (done is not None and tuple(done.shape) != shape[:2]):
            raise ValueError("adaptive_select: a and b must be [h, w, 4] of one size and done [h, w]")
        host = isinstance(a, np.ndarray)
        if done is None:
            done = np.zeros(shape[:2], np.uint8) if host else a.new_zeros(shape[:2], dtype=_torch().uint8)
        pixels = None
        if want_list:
            pixels = np.empty(shape[0] * shape[1], np.uint32) if host else a.new_empty(shape[0] * shape[1], dtype=_torch().int32)
        n = C.c_uint32()
        _check(lib().ptx_adaptive_select(self.h, shape[1], shape[0], _ptr(a), _ptr(b), threshold, _ptr(done), _ptr(pixels), C.byref(n)))
        return done, (pixels[:n.value] if want_list else None), n.value

    def accum_mean(self, a, b=None, out=None):
        """ptx_accum_mean: the MEANS (a + b) / (a.w + b.w) of radiance sums with per-pixel sample counts ([..., 4] float32), or a / a.w
        without b; all numpy or all torch-on-GPU; out may be a or b (None = a new buffer). Write them with tonemap_encode(..., spp=1)."""
        if out is None:
            out = np.empty(a.shape, np.float32) if isinstance(a, np.ndarray) else a.new_empty(tuple(a.shape))
        n = int(np.prod(tuple(a.shape)[:-1]))
        _check(lib().ptx_accum_mean(self.h, _ptr(a), _ptr(b), n, _ptr(out)))
        return out

    def emission_split(self, emission, guide_spp, a, b=None):
        """ptx_emission_split: takes the first-hit emission out of radiance sums before a filter call, in place. emission: [..., 4] float32
        Scene.render_emission SUMS over guide_spp samples of every pixel; a, b: radiance SUMS of the same shape whose alpha channel is the
        per-pixel sample count (b may be None); all numpy or all torch-on-GPU. Per channel with e = emission / guide_spp > 0:
        a -= a.w * e. Returns (a, b)."""
        self._emission_shapes("emission_split", emission, a, *([b] if b is not None else []))
        _check(lib().ptx_emission_split(self.h, _ptr(emission), guide_spp, int(np.prod(tuple(a.shape)[:-1])), _ptr(a), _ptr(b)))
        return a, b

    def emission_merge(self, emission, guide_spp, out):
        """ptx_emission_merge: adds the first-hit emission MEAN (emission / guide_spp, where > 0) to the MEANS a filter call returned for
        halves that went through emission_split, in place. Buffers as in emission_split(). Returns out."""
        self._emission_shapes("emission_merge", emission, out)
        _check(lib().ptx_emission_merge(self.h, _ptr(emission), guide_spp, int(np.prod(tuple(out.shape)[:-1])), _ptr(out)))
        return out

    @staticmethod
    def _emission_shapes(who, *bufs):
        shape = tuple(bufs[0].shape)
        if len(shape) < 1 or shape[-1] != 4 or any(tuple(x.shape) != shape for x in bufs):
            raise ValueError(f"{who}: every buffer must be [..., 4] of one size, got {[tuple(x.shape) for x in bufs]}")

    def set_mask_exchange(self, exchange, mask=None):
        """ptx_ctx_set_mask_exchange: the merge of the noisy bytes over the ranks that Scene.render_adaptive / render_adaptive_nee with
        shard=(index, count > 1, ...) need (include/ptx.h has the sharded loop). exchange(mask, n_bytes) is called once per round after the
        library wrote this rank's bytes into `mask` (a uint8 numpy array or torch-on-GPU tensor of at least w * h elements, kept alive here)
        and synchronised its stream; it returns when `mask` holds the element-wise MAX over the ranks, and returns None / 0 for success or a
        non-zero int. An exception inside it counts as a failure (status -1; it is kept in `mask_exchange_error`). It must not call this
        context. None clears the registration."""
        if exchange is None:
            _check(lib().ptx_ctx_set_mask_exchange(self.h, MASK_EXCHANGE_FN(), None, None, 0))
            self._mask_exchange = None
            return
        if mask is None:
            raise PtxError(ERR_INVALID, "set_mask_exchange: a callback needs a mask buffer")
        self.mask_exchange_error = None

        def thunk(_user, _mask, n_bytes):
            try:
                return int(exchange(mask, n_bytes) or 0)
            except BaseException as e:   # ctypes would swallow it: the render call fails instead
                self.mask_exchange_error = e
                return -1

        fn = MASK_EXCHANGE_FN(thunk)
        n = int(mask.numel()) if hasattr(mask, "numel") else int(mask.size)
        _check(lib().ptx_ctx_set_mask_exchange(self.h, fn, None, _ptr(mask), n))
        self._mask_exchange = (fn, mask)   # the CFUNCTYPE object and the buffer live as long as the registration

    def mask_exchange_stats(self):
        """ptx_ctx_get_mask_exchange_stats: {"calls", "wall_ms"} of the exchange in this context's last adaptive call."""
        calls, ms = C.c_uint64(), C.c_double()
        _check(lib().ptx_ctx_get_mask_exchange_stats(self.h, C.byref(calls), C.byref(ms)))
        return {"calls": calls.value, "wall_ms": ms.value}

    def close(self):
        if getattr(self, "h", None):
            lib().ptx_ctx_destroy(self.h)
            self.h = None
            self._mask_exchange = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_ARR_DTYPE = {ARR_MODEL_XFORM: (np.float32, 12), ARR_MODEL_AABB: (np.float32, 6), ARR_MODEL_SURF: (np.int32, 2),
              ARR_SURF_RANGE: (np.int32, 8), ARR_MESH_AABB: (np.float32, 6), ARR_VERTICES: (np.float32, 11),
              ARR_TRIANGLES: (np.uint32, 3), ARR_MATERIALS: (np.float32, 11), ARR_KD_NODES: (np.uint32, 2),
              ARR_KD_REFS: (np.uint32, 1), ARR_CAMERA: (np.float32, 1), ARR_SUN: (np.float32, 1),
              ARR_TEXTURES: (np.uint32, 4), ARR_TEXELS: (np.uint8, 1), ARR_SURF_TEX: (np.int32, 7), ARR_TEXELS_F32: (np.float32, 1),
              ARR_LIGHT_TRIS: (np.uint32, 2), ARR_LIGHT_CDF: (np.float32, 1), ARR_LIGHT_GEOM: (np.float32, 4),
              ARR_TRI_ISECT: (np.uint32, 12), ARR_RES_NODES: (np.uint32, 2), ARR_RES_REFS: (np.uint32, 1), ARR_RES_TRIS: (np.uint32, 12),
              ARR_LDS_ROOT: (np.uint32, 1), ARR_RES_PLAN: (np.uint32, 1), ARR_ENV_ROW_CDF: (np.float32, 1), ARR_ENV_CELL_CDF: (np.float32, 1),
              ARR_PUNCTUAL: (np.float32, 16), ARR_PUNCTUAL_CDF: (np.float32, 1), ARR_LENS: (np.float32, 2),
              ARR_LDS_SHAPE: (np.uint32, 1), ARR_SURF_AUX: (np.uint32, 4),
              ARR_MOTION_XFORM: (np.float32, 12), ARR_MOTION_MOVED: (np.uint32, 1), ARR_MOTION_CAMERA: (np.float32, 1),
              ARR_PUNCTUAL_TREE: (np.uint32, 8), ARR_LIGHT_TREE: (np.uint32, 8), ARR_LIGHT_PATH: (np.uint32, 1)}


class Scene:
    """Flattened immutable scene (ptx_scene). ctx=None gives a host-only scene (inspection, no GPU work)."""

    def __init__(self, handle, ctx):
        self.h = handle
        self.ctx = ctx
        _live.add(self)

    @classmethod
    def load_gltf(cls, ctx, path, camera_index=0, sun_light_index=0, work=None):
        """work: None = every primitive (core::renderer::load_gltf); a dict {mesh name: [primitive indices]} = the host's
        per-worker filter (models::work_info::work)."""
        h = C.c_void_p()
        opts = LoadOpts(camera_index, sun_light_index, 0, 0, None)
        keep = []
        if work is not None:
            items = (WorkItem * max(len(work), 1))()
            for k, (name, prims) in enumerate(work.items()):
                arr = (C.c_int32 * max(len(prims), 1))(*prims)
                keep.append(arr)
                items[k] = WorkItem(name.encode(), arr, len(prims))
            opts = LoadOpts(camera_index, sun_light_index, 1, len(work), items)
        _check(lib().ptx_scene_load_gltf(ctx.h if ctx else None, os.fsencode(path), C.byref(opts), C.byref(h)))
        return cls(h, ctx)

    @classmethod
    def load_event(cls, ctx, event_json, local_scene_root):
        """The reference worker's Lambda event (events/event.json shape) -> (scene, RenderCfg, event info dict)."""
        h, cfg, ev = C.c_void_p(), RenderCfg(), WorkerEvent()
        _check(lib().ptx_worker_event_load(ctx.h if ctx else None, os.fsencode(event_json), os.fsencode(local_scene_root),
                                           C.byref(h), C.byref(cfg), C.byref(ev)))
        info = dict(num_workers=ev.num_workers, n_work_meshes=ev.n_work_meshes, worker_id=ev.worker_id.decode(),
                    scene_root=ev.scene_root.decode(), scene_bucket=ev.scene_bucket.decode())
        return cls(h, ctx), cfg, info

    def render_cfg(self, cfg, accum=None, want_stats=True):
        """ptx_render with a ready RenderCfg (e.g. from load_event)."""
        W, H = cfg.W, cfg.H
        w, h = (cfg.w, cfg.h) if cfg.w and cfg.h else (W, H)
        if accum is None:
            accum = np.zeros((h, w, 4), np.float32)
        st = RenderStats()
        _check(lib().ptx_render(self.h, C.byref(cfg), _ptr(accum), C.byref(st) if want_stats else None))
        return accum, (dict(rays=st.rays, samples=st.samples, passes=st.passes, kernel_ms=st.kernel_ms) if want_stats else None)

    @classmethod
    def from_arrays(cls, ctx, model_xform, model_surf, surf_range, vertices, triangles, materials, camera, sun=None):
        keep = [np.ascontiguousarray(model_xform, np.float32), np.ascontiguousarray(model_surf, np.int32),
                np.ascontiguousarray(np.asarray(surf_range)[:, :4], np.int32), np.ascontiguousarray(vertices, np.float32),
                np.ascontiguousarray(triangles, np.uint32), np.ascontiguousarray(materials, np.float32),
                np.ascontiguousarray(np.asarray(camera)[:13], np.float32)]
        sun_a = np.ascontiguousarray(sun, np.float32) if sun is not None and len(sun) else None
        d = SceneDesc(len(keep[0]), keep[0].ctypes.data, keep[1].ctypes.data, len(keep[2]), keep[2].ctypes.data,
                      keep[3].ctypes.data, keep[4].ctypes.data, keep[5].ctypes.data, keep[6].ctypes.data,
                      sun_a.ctypes.data if sun_a is not None else None)
        h = C.c_void_p()
        _check(lib().ptx_scene_from_arrays(ctx.h if ctx else None, C.byref(d), C.byref(h)))
        return cls(h, ctx)

    def info(self):
        i = SceneInfo()
        _check(lib().ptx_scene_get_info(self.h, C.byref(i)))
        return {n: getattr(i, n) for n, _ in SceneInfo._fields_}

    def array(self, which):
        n = lib().ptx_scene_get_array(self.h, which, None, 0)
        if n < 0:
            _check(ERR_INVALID)
        if which == ARR_MODEL_NAMES:
            buf = C.create_string_buffer(int(n) + 1)
            lib().ptx_scene_get_array(self.h, which, buf, n)
            return buf.raw[:n].decode().split("\n")[:-1]
        dt, cols = _ARR_DTYPE[which]
        out = np.zeros(int(n), dt)
        if n:
            got = lib().ptx_scene_get_array(self.h, which, out.ctypes.data, out.nbytes)
            assert got == n
        return out.reshape(-1, cols) if cols > 1 else out

    def render(self, W, H, spp, bounces, accum=None, env=(1.0, 1.0, 1.0), seed=0x5EED, tile=None, sample0=0,
               spp_per_pass=0, want_stats=True, integrator=INTEGRATOR_LIB, shard=None):
        """Adds radiance SUMS of samples [sample0, sample0+spp) into accum ([h,w,4] float32; numpy or torch-on-GPU).
        integrator: INTEGRATOR_LIB = core::renderer::trace, INTEGRATOR_WORKER = the HOST worker's stage pipeline.
        shard: None, or (index, count[, tile size = 64]): only the pixels in image tiles t with t % count == index are rendered.
        Returns (accum, stats dict or None)."""
        x0, y0, w, h = tile if tile else (0, 0, W, H)
        if accum is None:
            accum = np.zeros((h, w, 4), np.float32)
        cfg = RenderCfg(W, H, spp, bounces, (C.c_float * 3)(*env), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                        x0, y0, w, h, sample0, spp_per_pass, integrator, *((tuple(shard) + (0,))[:3] if shard else (0, 0, 0)))
        st = RenderStats()
        _check(lib().ptx_render(self.h, C.byref(cfg), _ptr(accum), C.byref(st) if want_stats else None))
        stats = dict(rays=st.rays, samples=st.samples, passes=st.passes, kernel_ms=st.kernel_ms) if want_stats else None
        return accum, stats

    def render_transparent(self, W, H, spp, bounces, pixels=None, claimed=None, env=(1.0, 1.0, 1.0), seed=0x5EED, tile=None, sample0=0,
                           spp_per_pass=0, want_stats=True, integrator=INTEGRATOR_LIB, shard=None):
        """ptx_render_transparent: core::renderer::render() with transparent_background set. Advances the reference's per-pixel blend
        state — pixels [h,w,4] float32 (running colour and alpha: MEANS, not sums) and claimed [h,w] uint8, numpy or torch-on-GPU, both
        of one kind — through samples [sample0, sample0+spp) in sample order. A frame starts from zeroed buffers at sample0 = 0 (the
        default when none are given); later calls must continue with ascending, adjacent sample ranges on the same buffers. Tiles and
        shards work as in render(); sample ranges rendered into separate buffers cannot be merged. INTEGRATOR_WORKER is refused.
        Returns (pixels, claimed, stats dict or None)."""
        x0, y0, w, h = tile if tile else (0, 0, W, H)
        if (pixels is None) != (claimed is None):
            raise PtxError(ERR_INVALID, "render_transparent: pass both pixels and claimed, or neither")
        if pixels is None:
            pixels, claimed = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.uint8)
        cfg = RenderCfg(W, H, spp, bounces, (C.c_float * 3)(*env), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                        x0, y0, w, h, sample0, spp_per_pass, integrator, *((tuple(shard) + (0,))[:3] if shard else (0, 0, 0)))
        st = RenderStats()
        _check(lib().ptx_render_transparent(self.h, C.byref(cfg), _ptr(pixels), _ptr(claimed), C.byref(st) if want_stats else None))
        stats = dict(rays=st.rays, samples=st.samples, passes=st.passes, kernel_ms=st.kernel_ms) if want_stats else None
        return pixels, claimed, stats

    def render_aov(self, W, H, spp, albedo=None, normal_depth=None, seed=0x5EED, tile=None, sample0=0, spp_per_pass=0, want_stats=True,
                   shard=None):
        """ptx_render_aov: first-hit guide buffers of the camera samples [sample0, sample0+spp) that render() traces. ADDS into
        albedo [h,w,4] float32 (albedo rgb SUMS over the samples that end on a surface, w = how many did) and normal_depth [h,w,4]
        (world shading normal SUMS, w = depth sum); numpy or torch-on-GPU, both of one kind. With neither given both are produced from
        zeros; with one given only that one is produced (the other is returned as None). Tiles, sample ranges and shards compose as
        in render(). Returns (albedo, normal_depth, stats dict or None)."""
        x0, y0, w, h = tile if tile else (0, 0, W, H)
        if albedo is None and normal_depth is None:
            albedo, normal_depth = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        cfg = RenderCfg(W, H, spp, 0, (C.c_float * 3)(1.0, 1.0, 1.0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                        x0, y0, w, h, sample0, spp_per_pass, INTEGRATOR_LIB, *((tuple(shard) + (0,))[:3] if shard else (0, 0, 0)))
        bufs = AovBuffers(_ptr(albedo), _ptr(normal_depth))
        st = RenderStats()
        _check(lib().ptx_render_aov(self.h, C.byref(cfg), C.byref(bufs), C.byref(st) if want_stats else None))
        stats = dict(rays=st.rays, samples=st.samples, passes=st.passes, kernel_ms=st.kernel_ms) if want_stats else None
        return albedo, normal_depth, stats

    def render_motion(self, W, H, spp, prev_camera=None, prev_model_xform=None, motion=None, seed=0x5EED, tile=None, sample0=0, spp_per_pass=0,
                      want_stats=True, shard=None):
        """ptx_render_motion: per-pixel SUMS, over the camera samples [sample0, sample0+spp) that render() and render_aov() trace, of
        (previous minus current screen position in pixels, distance from the previous camera, 1), ADDED into motion [h,w,4] float32 (numpy or
        torch-on-GPU; None = zeros). prev_camera: what camera() returned one frame earlier (a dict with origin [3], basis [9], yfov; its lens
        fields are ignored), None = the camera did not move. prev_model_xform: [n_models,12] float32 as array(ARR_MODEL_XFORM) held one frame
        earlier, None = no model moved. Tiles, sample ranges and shards compose as in render_aov(). Returns (motion, stats dict or None)."""
        x0, y0, w, h = tile if tile else (0, 0, W, H)
        if motion is None:
            motion = np.zeros((h, w, 4), np.float32)
        cfg = RenderCfg(W, H, spp, 0, (C.c_float * 3)(1.0, 1.0, 1.0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                        x0, y0, w, h, sample0, spp_per_pass, INTEGRATOR_LIB, *((tuple(shard) + (0,))[:3] if shard else (0, 0, 0)))
        cam = xf = None
        if prev_camera is not None:
            o, b = np.asarray(prev_camera["origin"], np.float32).reshape(-1), np.asarray(prev_camera["basis"], np.float32).reshape(-1)
            if len(o) != 3 or len(b) != 9:
                raise PtxError(ERR_INVALID, "render_motion: the previous camera's origin is [3], its basis [9]")
            cam = Camera((C.c_float * 3)(*o), (C.c_float * 9)(*b), prev_camera["yfov"], 0.0, 0.0, 0, 0.0)
        if prev_model_xform is not None:
            xf = np.ascontiguousarray(prev_model_xform, np.float32)
            if xf.size % 12:
                raise PtxError(ERR_INVALID, "render_motion: the previous transforms are not [n, 12]")
        prev = None
        if cam is not None or xf is not None:
            prev = C.byref(MotionPrev(C.pointer(cam) if cam is not None else None, xf.ctypes.data if xf is not None else None,
                                      xf.size // 12 if xf is not None else 0))
        st = RenderStats()
        _check(lib().ptx_render_motion(self.h, C.byref(cfg), prev, _ptr(motion), C.byref(st) if want_stats else None))
        stats = dict(rays=st.rays, samples=st.samples, passes=st.passes, kernel_ms=st.kernel_ms) if want_stats else None
        return motion, stats

    def render_emission(self, W, H, spp, emission=None, seed=0x5EED, tile=None, sample0=0, spp_per_pass=0, want_stats=True, shard=None):
        """ptx_render_emission: per-pixel SUMS, over the camera samples [sample0, sample0+spp) that render() and render_aov() trace, of what
        each sample's surface emits towards the camera (emissive * 10, 1), ADDED into emission [h,w,4] float32 (numpy or torch-on-GPU;
        None = zeros); a back-facing surface and a miss add nothing. On a scene without a sun the rgb is bitwise render(bounces=1,
        env=(0, 0, 0)). Tiles, sample ranges and shards compose as in render_aov(). Returns (emission, stats dict or None)."""
        x0, y0, w, h = tile if tile else (0, 0, W, H)
        if emission is None:
            emission = np.zeros((h, w, 4), np.float32)
        cfg = RenderCfg(W, H, spp, 0, (C.c_float * 3)(1.0, 1.0, 1.0), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                        x0, y0, w, h, sample0, spp_per_pass, INTEGRATOR_LIB, *((tuple(shard) + (0,))[:3] if shard else (0, 0, 0)))
        st = RenderStats()
        _check(lib().ptx_render_emission(self.h, C.byref(cfg), _ptr(emission), C.byref(st) if want_stats else None))
        stats = dict(rays=st.rays, samples=st.samples, passes=st.passes, kernel_ms=st.kernel_ms) if want_stats else None
        return emission, stats

    def render_adaptive(self, W, H, spp, bounces, min_spp=8, step_spp=0, threshold=0.1, a=None, b=None, env=(1.0, 1.0, 1.0), seed=0x5EED, tile=None,
                        sample0=0, spp_per_pass=0, want_stats=True, integrator=INTEGRATOR_LIB, shard=None):
        """ptx_render_adaptive: noise-driven per-pixel sample counts. `spp` is the cap; every pixel gets min_spp samples, then rounds of
        step_spp (0 = min_spp) go to the pixels whose two halves still disagree by more than `threshold` (include/ptx.h has the rule).
        ADDS radiance SUMS into the half-buffers a and b ([h,w,4] float32, numpy or torch-on-GPU, both of one kind; None = zeros): a
        pixel's count is a[..., 3] + b[..., 3]. The frame: Context.accum_mean(a, b), then tonemap_encode(..., spp=1). Always synchronises.
        shard=(index, count > 1[, tile]) needs Context.set_mask_exchange: the ranks' zeroed buffers then sum to the unsharded frame, bit for bit.
        Returns (a, b, stats dict or None)."""
        x0, y0, w, h = tile if tile else (0, 0, W, H)
        if a is None and b is None:
            a, b = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        cfg = RenderCfg(W, H, spp, bounces, (C.c_float * 3)(*env), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                        x0, y0, w, h, sample0, spp_per_pass, integrator, *((tuple(shard) + (0,))[:3] if shard else (0, 0, 0)))
        acfg = AdaptiveCfg(min_spp, step_spp, threshold)
        st = AdaptiveStats()
        _check(lib().ptx_render_adaptive(self.h, C.byref(cfg), C.byref(acfg), _ptr(a), _ptr(b), C.byref(st) if want_stats else None))
        stats = dict(rays=st.render.rays, samples=st.render.samples, passes=st.render.passes, kernel_ms=st.render.kernel_ms, rounds=st.rounds,
                     active_last=st.active_last, select_ms=st.select_ms) if want_stats else None
        return a, b, stats

    def render_nee(self, W, H, spp, bounces, accum=None, env=(1.0, 1.0, 1.0), seed=0x5EED, tile=None, sample0=0, spp_per_pass=0,
                   want_stats=True, integrator=INTEGRATOR_LIB, shard=None, flags=0, candidates=1):
        """ptx_render_nee: render()'s samples with the LIB estimator plus one light sample towards the listed emissive triangles per
        continuing vertex, MIS-weighted (include/ptx.h has the estimator). ADDS radiance SUMS into accum as render() does; tiles, sample
        ranges and shards compose the same way. flags: NEE_NO_LIGHT_SAMPLES runs with an empty list (bitwise render()'s frame);
        NEE_FUSED renders each pass with one kernel launch where render() runs its fused kernel (bitwise the unflagged frame; ignored on
        scenes of the queue route); NEE_ENV_SAMPLES lets the light sample go towards the environment map (set_environment), importance-
        sampled by luminance and MIS-weighted against the map's radiance on a miss (ignored without a map or with a black one);
        NEE_SAMPLER_PDF builds the MIS weights on the density of LIB's BSDF sampler instead of LIB's pdf value, which removes the shift of
        the expectation at glossy vertices that see a light (bitwise the unflagged frame when no light sample is possible).
        NEE_FUSED | NEE_FUSED_MOTION keeps the one launch per pass under active motion (set_motion), where NEE_FUSED alone is ignored:
        bitwise the unflagged frame under the same motion.
        candidates = m ors NEE_CANDIDATES(m) into flags: the light sample picked among m candidates, still one shadow ray per vertex.
        Returns (accum, stats dict or None)."""
        x0, y0, w, h = tile if tile else (0, 0, W, H)
        if accum is None:
            accum = np.zeros((h, w, 4), np.float32)
        cfg = RenderCfg(W, H, spp, bounces, (C.c_float * 3)(*env), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                        x0, y0, w, h, sample0, spp_per_pass, integrator, *((tuple(shard) + (0,))[:3] if shard else (0, 0, 0)))
        ncfg = NeeCfg(flags | NEE_CANDIDATES(candidates))
        st = NeeStats()
        _check(lib().ptx_render_nee(self.h, C.byref(cfg), C.byref(ncfg), _ptr(accum), C.byref(st) if want_stats else None))
        stats = dict(rays=st.render.rays, samples=st.render.samples, passes=st.render.passes, kernel_ms=st.render.kernel_ms, n_lights=st.n_lights,
                     light_area=st.light_area, light_samples=st.light_samples, light_visible=st.light_visible) if want_stats else None
        return accum, stats

    def render_adaptive_nee(self, W, H, spp, bounces, min_spp=8, step_spp=0, threshold=0.1, a=None, b=None, env=(1.0, 1.0, 1.0), seed=0x5EED, tile=None,
                            sample0=0, spp_per_pass=0, want_stats=True, integrator=INTEGRATOR_LIB, shard=None, flags=0, candidates=1):
        """ptx_render_adaptive_nee: render_adaptive()'s loop on render_nee()'s estimator with `flags` (and `candidates`, as there), one sequence of passes per round resolved
        into both halves. A pixel with n samples holds, bit for bit, what render_nee() calls of the same half ranges leave in a and b. Filter
        the result with Context.denoise_counts. Returns (a, b, stats dict or None)."""
        x0, y0, w, h = tile if tile else (0, 0, W, H)
        if a is None and b is None:
            a, b = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        cfg = RenderCfg(W, H, spp, bounces, (C.c_float * 3)(*env), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF,
                        x0, y0, w, h, sample0, spp_per_pass, integrator, *((tuple(shard) + (0,))[:3] if shard else (0, 0, 0)))
        acfg, ncfg = AdaptiveCfg(min_spp, step_spp, threshold), NeeCfg(flags | NEE_CANDIDATES(candidates))
        st = AdaptiveNeeStats()
        _check(lib().ptx_render_adaptive_nee(self.h, C.byref(cfg), C.byref(acfg), C.byref(ncfg), _ptr(a), _ptr(b), C.byref(st) if want_stats else None))
        r = st.nee.render
        stats = dict(rays=r.rays, samples=r.samples, passes=r.passes, kernel_ms=r.kernel_ms, n_lights=st.nee.n_lights, light_area=st.nee.light_area,
                     light_samples=st.nee.light_samples, light_visible=st.nee.light_visible, rounds=st.rounds, active_last=st.active_last,
                     select_ms=st.select_ms) if want_stats else None
        return a, b, stats

    def set_environment(self, png_path, srgb=True):
        """renderer::environment = image_texture::load(png_path, srgb): the miss colour becomes map(direction) * environment_factor.
        None removes the map."""
        _check(lib().ptx_scene_set_environment(self.h, os.fsencode(png_path) if png_path is not None else None, int(bool(srgb))))

    def set_punctual_lights(self, lights):
        """ptx_scene_set_punctual_lights: [n, 16] float32 records (position, range, direction, kind 0 point / 1 spot, intensity rgb, cos_inner,
        cos_outer, three zeros), e.g. read_punctual_lights(path)'s. render_nee and render_adaptive_nee then sample them as a third strategy;
        every other render ignores them. None or an empty array removes them."""
        a = np.zeros((0, 16), np.float32) if lights is None else np.ascontiguousarray(lights, np.float32)
        if a.size % 16:
            raise PtxError(ERR_INVALID, "set_punctual_lights: the array is not [n, 16]")
        a = a.reshape(-1, 16)
        _check(lib().ptx_scene_set_punctual_lights(self.h, a.ctypes.data if len(a) else None, len(a)))

    def set_punctual_pick(self, pick):
        """ptx_scene_set_punctual_pick: PUNCTUAL_PICK_CDF (the default: by lum(intensity) alone) or PUNCTUAL_PICK_TREE (a light tree descended
        from the shading point with importance power / distance^2). The mode survives set_punctual_lights; array(ARR_PUNCTUAL_TREE) is the tree."""
        _check(lib().ptx_scene_set_punctual_pick(self.h, int(pick)))

    @property
    def punctual_pick(self):
        """ptx_scene_get_punctual_pick"""
        v = C.c_uint32()
        _check(lib().ptx_scene_get_punctual_pick(self.h, C.byref(v)))
        return v.value

    def punctual_pick_batch(self, pos_u):
        """ptx_punctual_pick_batch: [n,4] float32 (position, u) -> (light [n] int32, pmf [n] float32): the light a punctual candidate at the
        position with draw u samples and its probability, by the device function the integrators inline, in the scene's mode."""
        a = np.ascontiguousarray(pos_u, np.float32).reshape(-1, 4)
        light, pmf = np.zeros(len(a), np.int32), np.zeros(len(a), np.float32)
        _check(lib().ptx_punctual_pick_batch(self.h, a.ctypes.data, len(a), light.ctypes.data, pmf.ctypes.data))
        return light, pmf

    def set_light_pick(self, pick):
        """ptx_scene_set_light_pick: "cdf" / LIGHT_PICK_CDF (the default: by area alone) or "tree" / LIGHT_PICK_TREE (a light tree over the
        light list descended from the shading point with importance power / distance^2). The mode outlives the list;
        array(ARR_LIGHT_TREE) and array(ARR_LIGHT_PATH) are the tree and the path words."""
        if isinstance(pick, str):
            if pick not in _LIGHT_PICK_NAMES:
                raise PtxError(ERR_INVALID, f"set_light_pick: unknown mode {pick!r}")
            pick = _LIGHT_PICK_NAMES[pick]
        _check(lib().ptx_scene_set_light_pick(self.h, int(pick)))

    def get_light_pick(self):
        """ptx_scene_get_light_pick -> "cdf" or "tree"""
        v = C.c_uint32()
        _check(lib().ptx_scene_get_light_pick(self.h, C.byref(v)))
        return "tree" if v.value == LIGHT_PICK_TREE else "cdf"

    def light_pick_batch(self, pos_u):
        """ptx_light_pick_batch: [n,4] float32 (position, u) -> (light [n] int32, pmf [n] float32): the entry of the light list a triangle
        sample at the position with draw u picks and its probability, by the device function the integrator inlines, in the scene's mode."""
        a = np.ascontiguousarray(pos_u, np.float32).reshape(-1, 4)
        light, pmf = np.zeros(len(a), np.int32), np.zeros(len(a), np.float32)
        _check(lib().ptx_light_pick_batch(self.h, a.ctypes.data, len(a), light.ctypes.data, pmf.ctypes.data))
        return light, pmf

    def light_pmf_batch(self, pos, light):
        """ptx_light_pmf_batch: positions [n,3] float32 and list entries [n] int32 -> pmf [n] float32: the probability with which the pick
        returns the entry from the position, by the device function the emission weight inlines."""
        a = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        k = np.ascontiguousarray(light, np.int32).reshape(-1)
        if len(k) != len(a):
            raise PtxError(ERR_INVALID, "light_pmf_batch: one entry per position")
        pmf = np.zeros(len(a), np.float32)
        _check(lib().ptx_light_pmf_batch(self.h, a.ctypes.data, k.ctypes.data, len(a), pmf.ctypes.data))
        return pmf

    def set_camera(self, origin, basis, yfov, lens_radius=0.0, focus_distance=0.0, blades=0, blade_rotation=0.0):
        """ptx_scene_set_camera: origin [3], basis [9] (columns x, y, z) and yfov as from_arrays' camera [13]; lens_radius > 0 gives a thin
        lens with a polygonal aperture of `blades` corners (0 = 16) focused at focus_distance. No tree is built and nothing is re-uploaded."""
        o, b = np.asarray(origin, np.float32).reshape(-1), np.asarray(basis, np.float32).reshape(-1)
        if len(o) != 3 or len(b) != 9:
            raise PtxError(ERR_INVALID, "set_camera: origin is [3], basis is [9]")
        cam = Camera((C.c_float * 3)(*o), (C.c_float * 9)(*b), yfov, lens_radius, focus_distance, blades, blade_rotation)
        _check(lib().ptx_scene_set_camera(self.h, C.byref(cam)))

    def camera(self):
        """ptx_scene_get_camera -> dict(origin [3], basis [9], yfov, lens_radius, focus_distance, blades, blade_rotation), as stored."""
        cam = Camera()
        _check(lib().ptx_scene_get_camera(self.h, C.byref(cam)))
        return dict(origin=np.array(cam.origin, np.float32), basis=np.array(cam.basis, np.float32), yfov=np.float32(cam.yfov),
                    lens_radius=np.float32(cam.lens_radius), focus_distance=np.float32(cam.focus_distance), blades=int(cam.blades),
                    blade_rotation=np.float32(cam.blade_rotation))

    def set_model_xforms(self, model_xform):
        """ptx_scene_set_model_xforms: [n_models, 12] float32 in ARR_MODEL_XFORM's layout. The scene then equals one created from the same
        arrays with these transforms; no KD tree is built."""
        a = np.ascontiguousarray(model_xform, np.float32)
        if a.size % 12:
            raise PtxError(ERR_INVALID, "set_model_xforms: the array is not [n, 12]")
        _check(lib().ptx_scene_set_model_xforms(self.h, a.ctypes.data, a.size // 12))

    def set_motion(self, begin_model_xform=None, begin_camera=None, shutter=(0.0, 1.0)):
        """ptx_scene_set_motion: the scene as it stands is the state at u = 1; begin_model_xform ([n_models, 12] float32, ARR_MODEL_XFORM's
        layout) and begin_camera (a dict as camera() returns, or (origin [3], basis [9], yfov)) give the state at u = 0. None: that part does
        not move. shutter = (open, close) within [0, 1]. set_model_xforms and set_camera clear the motion: call them first, this last."""
        m = Motion()
        keep = []
        if begin_model_xform is not None:
            a = np.ascontiguousarray(begin_model_xform, np.float32)
            if a.size % 12:
                raise PtxError(ERR_INVALID, "set_motion: begin_model_xform is not [n, 12]")
            keep.append(a)
            m.begin_model_xform, m.n_models = a.ctypes.data, a.size // 12
        if begin_camera is not None:
            if isinstance(begin_camera, dict):
                o, b, yfov = begin_camera["origin"], begin_camera["basis"], begin_camera["yfov"]
            else:
                o, b, yfov = begin_camera
            o, b = np.asarray(o, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
            if len(o) != 3 or len(b) != 9:
                raise PtxError(ERR_INVALID, "set_motion: the begin camera's origin is [3], its basis is [9]")
            cam = Camera((C.c_float * 3)(*o), (C.c_float * 9)(*b), float(yfov), 0.0, 0.0, 0, 0.0)
            keep.append(cam)
            m.begin_camera = C.pointer(cam)
        m.shutter_open, m.shutter_close = float(shutter[0]), float(shutter[1])
        _check(lib().ptx_scene_set_motion(self.h, C.byref(m)))

    def clear_motion(self):
        """ptx_scene_set_motion(scene, NULL): the scene renders as one never given motion."""
        _check(lib().ptx_scene_set_motion(self.h, None))

    def motion_state(self, u):
        """ptx_scene_motion_state -> (model_xform [n_models, 12], camera [12]: origin, basis) at time u, by the function the kernels use.
        Static models and a static camera come back as they are stored."""
        n = self.info()["n_models"]
        x, cam = np.zeros((n, 12), np.float32), np.zeros(12, np.float32)
        _check(lib().ptx_scene_motion_state(self.h, float(u), x.ctypes.data, cam.ctypes.data))
        return x, cam

    def intersect_motion(self, origins, dirs, time, attributes=True):
        """ptx_intersect_batch_motion: intersect() with a time per ray ([n] float32). origins/dirs [n,3] and time are numpy arrays, or torch
        tensors on the scene's GPU (then the outputs are torch tensors there). Without a moving model `time` is ignored."""
        if isinstance(origins, np.ndarray) or not hasattr(origins, "data_ptr"):
            o = np.ascontiguousarray(np.asarray(origins, np.float32).T)
            d = np.ascontiguousarray(np.asarray(dirs, np.float32).T)
            t = np.ascontiguousarray(np.asarray(time, np.float32).reshape(-1))
            n = o.shape[1]
            new = lambda dt: np.zeros(n, dt)
            f32, i32 = np.float32, np.int32
        else:
            torch = _torch()
            o, d = origins.float().t().contiguous(), dirs.float().t().contiguous()
            t = time.float().reshape(-1).contiguous()
            n = o.shape[1]
            new = lambda dt: torch.zeros(n, dtype=dt, device=o.device)
            f32, i32 = torch.float32, torch.int32
        if len(t) != n:
            raise PtxError(ERR_INVALID, "intersect_motion: time is not [n]")
        out = {k: new(f32) for k in ("distance", "b0", "b1", "b2")}
        out["surface"], out["triangle"] = new(i32), new(i32)
        if attributes:
            out.update({k: new(f32) for k in ("px", "py", "pz", "nx", "ny", "nz", "u", "v")})
        r = Rays(*[_ptr(o[k]) for k in range(3)], *[_ptr(d[k]) for k in range(3)])
        hh = Hits(*[_ptr(out[k]) if k in out else None for k, _ in Hits._fields_])
        _check(lib().ptx_intersect_batch_motion(self.h, C.byref(r), _ptr(t), n, C.byref(hh)))
        if not isinstance(o, np.ndarray):
            self.ctx.synchronize()   # device buffers: the call returns with the work queued on the context's stream
        return out

    def lens_rays(self, in5):
        """ptx_camera_lens_rays_batch: [n,5] float32 (ndc.x, ndc.y, aspect ratio, u, v) -> [n,6] float32 (origin, direction): the lens ray the
        integrators compute from the lens draws (u, v); the pinhole ray on a scene without a lens."""
        a = np.ascontiguousarray(in5, np.float32).reshape(-1, 5)
        out = np.zeros((len(a), 6), np.float32)
        _check(lib().ptx_camera_lens_rays_batch(self.h, a.ctypes.data, len(a), out.ctypes.data))
        return out

    def camera_rays(self, ndc_ratio):
        """ptx_camera_rays_batch: [n,3] float32 (ndc.x, ndc.y, aspect ratio) -> [n,6] float32 (origin, direction) = scene::camera::get_ray."""
        a = np.ascontiguousarray(ndc_ratio, np.float32).reshape(-1, 3)
        out = np.zeros((len(a), 6), np.float32)
        _check(lib().ptx_camera_rays_batch(self.h, a.ctypes.data, len(a), out.ctypes.data))
        return out

    def material_eval(self, surface, uv):
        """ptx_material_eval_batch: surface index (scalar or [n] int) and [n,2] float32 uvs -> [n,12] float32 normal_ts(3), albedo(3),
        opacity, roughness, metallic, emissive(3) * 10 = core::material::get_* as the shading kernels evaluate them."""
        a = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(surface, np.int32), (len(a),)))
        out = np.zeros((len(a), 12), np.float32)
        _check(lib().ptx_material_eval_batch(self.h, s.ctypes.data, a.ctypes.data, len(a), out.ctypes.data))
        return out

    def intersect(self, origins, dirs, attributes=True):
        """Batch closest-hit. origins/dirs: [n,3] float32 numpy. Returns dict of numpy arrays."""
        o = np.ascontiguousarray(np.asarray(origins, np.float32).T)
        d = np.ascontiguousarray(np.asarray(dirs, np.float32).T)
        n = o.shape[1]
        out = {k: np.zeros(n, np.float32) for k in ("distance", "b0", "b1", "b2")}
        out["surface"] = np.zeros(n, np.int32)
        out["triangle"] = np.zeros(n, np.int32)
        if attributes:
            out.update({k: np.zeros(n, np.float32) for k in ("px", "py", "pz", "nx", "ny", "nz", "u", "v")})
        r = Rays(*[o[k].ctypes.data for k in range(3)], *[d[k].ctypes.data for k in range(3)])
        hh = Hits(*[out[k].ctypes.data if k in out else None for k, _ in Hits._fields_])
        _check(lib().ptx_intersect_batch(self.h, C.byref(r), n, C.byref(hh)))
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().ptx_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_punctual_lights(path):
    """ptx_gltf_read_punctual_lights: the `point` and `spot` lights of a glTF file (KHR_lights_punctual), one [16] float32 record per node that
    references one, in the loader's pre-order and placed by the loader's node transforms -> [n, 16] float32 for Scene.set_punctual_lights.
    Host only. `directional` lights are skipped."""
    n = lib().ptx_gltf_read_punctual_lights(os.fsencode(path), None, 0)
    if n < 0:
        _check(int(-n))
    out = np.zeros((n, 16), np.float32)
    if n:
        got = lib().ptx_gltf_read_punctual_lights(os.fsencode(path), out.ctypes.data, out.size)
        if got < 0:
            _check(int(-got))
    return out


def encode_png(rgba8):
    """image::image::save_to_memory_png — RGBA8 [H,W,4] numpy -> PNG bytes."""
    a = np.ascontiguousarray(rgba8, np.uint8)
    H, W = a.shape[:2]
    p, n = C.c_void_p(), C.c_size_t()
    _check(lib().ptx_encode_png(a.ctypes.data, W, H, C.byref(p), C.byref(n)))
    try:
        return C.string_at(p, n.value)
    finally:
        lib().ptx_free(p)


class Renderer:
    """Host-side mirror of core::renderer (renderer.hpp:15-36): same public fields and defaults,
    load_gltf(path), render() -> PNG bytes (RGBA8, tonemapped, sRGB). Work happens on the GPU."""

    no_sun_light = NO_SUN_LIGHT

    def __init__(self, device=0):
        self.resolution = (1920, 1080)
        self.thread_count = 0            # kept for interface parity; the GPU grid replaces the thread pool
        self.sample_count = 10000
        self.bounce_count = 4
        self.environment = None          # path of a PNG environment map (the reference holds a loaded image::texture), sRGB-decoded
        self.environment_factor = (1.0, 1.0, 1.0)
        self.transparent_background = False
        self.camera_index = 0
        self.sun_light_index = 0
        self.visualize_kd_tree_depth = 0
        self.seed = 0x5EED
        # thin lens of the loaded camera (Scene.set_camera), applied before a render; lens_radius 0 = the pinhole
        self.lens_radius = 0.0
        self.focus_distance = 0.0
        self.blades = 0
        self.blade_rotation = 0.0
        self._lens_set = (0.0, 0.0, 0, 0.0)
        self._ctx = Context(device)
        self._scene = None
        self.last_stats = None
        self.last_claimed = None
        self.last_denoise_stats = None
        self.last_adaptive_stats = None

    def load_gltf(self, path):
        self._scene = Scene.load_gltf(self._ctx, path, self.camera_index, self.sun_light_index)
        self._lens_set = (0.0, 0.0, 0, 0.0)

    def _apply_lens(self):
        """the lens fields onto the loaded camera, when they changed since the last render"""
        lens = (self.lens_radius, self.focus_distance, self.blades, self.blade_rotation)
        if lens != self._lens_set:
            cam = self._scene.camera()
            self._scene.set_camera(cam["origin"], cam["basis"], cam["yfov"], *lens)
            self._lens_set = lens

    def set_punctual_lights(self, lights):
        """Scene.set_punctual_lights on the loaded scene: render_nee() and render_adaptive_nee() sample these point and spot lights; render()
        and the other calls ignore them. read_punctual_lights(path) reads a glTF file's. None removes them."""
        if self._scene is None:
            raise PtxError(ERR_INVALID, "set_punctual_lights() before load_gltf()")
        self._scene.set_punctual_lights(lights)

    def set_punctual_pick(self, pick):
        """Scene.set_punctual_pick on the loaded scene: PUNCTUAL_PICK_CDF or PUNCTUAL_PICK_TREE; the mode survives set_punctual_lights."""
        if self._scene is None:
            raise PtxError(ERR_INVALID, "set_punctual_pick() before load_gltf()")
        self._scene.set_punctual_pick(pick)

    def set_light_pick(self, pick):
        """Scene.set_light_pick on the loaded scene: "cdf" or "tree"; the mode outlives the light list."""
        if self._scene is None:
            raise PtxError(ERR_INVALID, "set_light_pick() before load_gltf()")
        self._scene.set_light_pick(pick)

    def render_accum(self):
        """Radiance SUMS [H,W,4] of the frame; with transparent_background set, the reference's blended MEANS (colour, alpha) instead
        (Scene.render_transparent) — `last_claimed` then holds the per-pixel claimed flags."""
        if self._scene is None:
            raise PtxError(ERR_INVALID, "render() before load_gltf()")
        if self.visualize_kd_tree_depth:
            # mesh.cpp:316-318 seeds each node's colour from the node's heap address: no two runs of the reference agree, so there is
            # nothing reproducible to be faithful to
            raise PtxError(ERR_UNSUPPORTED, "visualize_kd_tree_depth is not built: the reference colours KD nodes by their heap addresses (mesh.cpp:316-318)")
        W, H = self.resolution
        self._apply_lens()
        if self.environment != getattr(self, "_env_set", None):
            self._scene.set_environment(self.environment)
            self._env_set = self.environment
        if self.transparent_background:
            pixels, self.last_claimed, self.last_stats = self._scene.render_transparent(W, H, self.sample_count, self.bounce_count,
                                                                                        env=self.environment_factor, seed=self.seed)
            return pixels
        accum, self.last_stats = self._scene.render(W, H, self.sample_count, self.bounce_count,
                                                    env=self.environment_factor, seed=self.seed)
        return accum

    def render_aov(self):
        """Guide buffers of the frame's camera samples for a denoiser (Scene.render_aov), as MEANS: (albedo [H,W,3] and normal [H,W,3]
        over the samples that end on a surface, depth [H,W] over the same samples, coverage [H,W] = their share of sample_count).
        Pixels no sample covers are zero."""
        if self._scene is None:
            raise PtxError(ERR_INVALID, "render_aov() before load_gltf()")
        W, H = self.resolution
        self._apply_lens()
        alb, nd, self.last_stats = self._scene.render_aov(W, H, self.sample_count, seed=self.seed)
        cov = alb[..., 3]
        inv = np.where(cov > 0, 1.0 / np.maximum(cov, 1.0), 0.0).astype(np.float32)
        return alb[..., :3] * inv[..., None], nd[..., :3] * inv[..., None], nd[..., 3] * inv, cov / np.float32(self.sample_count)

    def render_denoised(self, iterations=0, sigma_l=0, sigma_n=0, sigma_z=0, split_emission=False):
        """The frame through the variance-guided a-trous filter (Context.denoise): renders samples [0, n/2) and [n/2, n) of
        sample_count = n into two buffers, the guide buffers of all n, and returns the filtered MEANS [H,W,4] (write them with
        tonemap_encode(..., spp=1)). `last_denoise_stats` holds the filter's stats. split_emission: the first-hit emission of the same n
        samples (Scene.render_emission) is taken out of the halves before the filter and added to its output (Context.emission_split,
        emission_merge)."""
        if self._scene is None:
            raise PtxError(ERR_INVALID, "render_denoised() before load_gltf()")
        if self.transparent_background:
            raise PtxError(ERR_UNSUPPORTED, "render_denoised: the filter takes radiance sums, which transparent_background does not produce")
        n = self.sample_count
        if n < 2:
            raise PtxError(ERR_INVALID, "render_denoised: sample_count must be at least 2 (the noise estimate needs two half-frames)")
        W, H = self.resolution
        self._apply_lens()
        if self.environment != getattr(self, "_env_set", None):
            self._scene.set_environment(self.environment)
            self._env_set = self.environment
        a, _ = self._scene.render(W, H, n // 2, self.bounce_count, env=self.environment_factor, seed=self.seed, want_stats=False)
        b, _ = self._scene.render(W, H, n - n // 2, self.bounce_count, env=self.environment_factor, seed=self.seed, sample0=n // 2, want_stats=False)
        alb, nd, _ = self._scene.render_aov(W, H, n, seed=self.seed, want_stats=False)
        em = None
        if split_emission:
            em, _ = self._scene.render_emission(W, H, n, seed=self.seed, want_stats=False)
            self._ctx.emission_split(em, n, a, b)
        out, self.last_denoise_stats = self._ctx.denoise(a, b, alb, nd, n // 2, n - n // 2, iterations, sigma_l, sigma_n, sigma_z, out=a)
        return self._ctx.emission_merge(em, n, out) if split_emission else out

    def _denoise_counts(self, a, b, min_spp, split_emission=False):
        """The adaptive halves through Context.denoise_counts, with the guides of the first min_spp samples (every pixel has them).
        split_emission: the first-hit emission of the same min_spp samples goes round the filter."""
        W, H = self.resolution
        alb, nd, _ = self._scene.render_aov(W, H, min_spp, seed=self.seed, want_stats=False)
        em = None
        if split_emission:
            em, _ = self._scene.render_emission(W, H, min_spp, seed=self.seed, want_stats=False)
            self._ctx.emission_split(em, min_spp, a, b)
        out, self.last_denoise_stats = self._ctx.denoise_counts(a, b, alb, nd, min_spp, out=a)
        return self._ctx.emission_merge(em, min_spp, out) if split_emission else out

    def render_adaptive(self, threshold=0.1, min_spp=8, step_spp=0, denoise=False, split_emission=False):
        """The frame with noise-driven per-pixel sample counts (Scene.render_adaptive, sample_count = the cap), as MEANS [H,W,4] (write them
        with tonemap_encode(..., spp=1)); the alpha channel is 1. `last_adaptive_stats` holds the stats; samples / (W * H) is the mean count.
        denoise: the frame through the filter (Context.denoise_counts, guides of the first min_spp samples); `last_denoise_stats` holds its stats.
        split_emission (with denoise): as in render_denoised(), over the first min_spp samples."""
        if self._scene is None:
            raise PtxError(ERR_INVALID, "render_adaptive() before load_gltf()")
        if self.transparent_background:
            raise PtxError(ERR_UNSUPPORTED, "render_adaptive: the decision takes radiance sums, which transparent_background does not produce")
        W, H = self.resolution
        self._apply_lens()
        if self.environment != getattr(self, "_env_set", None):
            self._scene.set_environment(self.environment)
            self._env_set = self.environment
        a, b, self.last_adaptive_stats = self._scene.render_adaptive(W, H, self.sample_count, self.bounce_count, min_spp, step_spp, threshold,
                                                                     env=self.environment_factor, seed=self.seed)
        return self._denoise_counts(a, b, min_spp, split_emission) if denoise else self._ctx.accum_mean(a, b, out=a)

    def render_adaptive_nee(self, flags=0, threshold=0.1, min_spp=8, step_spp=0, denoise=False, candidates=1, split_emission=False):
        """render_adaptive() on render_nee()'s estimator (Scene.render_adaptive_nee; flags: ptx_nee_cfg.flags, candidates: NEE_CANDIDATES): the MEANS [H,W,4], through the
        filter with denoise, and with split_emission as in render_adaptive(). `last_adaptive_stats` holds the stats, the light-sampling ones included."""
        if self._scene is None:
            raise PtxError(ERR_INVALID, "render_adaptive_nee() before load_gltf()")
        if self.transparent_background:
            raise PtxError(ERR_UNSUPPORTED, "render_adaptive_nee: the decision takes radiance sums, which transparent_background does not produce")
        W, H = self.resolution
        self._apply_lens()
        if self.environment != getattr(self, "_env_set", None):
            self._scene.set_environment(self.environment)
            self._env_set = self.environment
        a, b, self.last_adaptive_stats = self._scene.render_adaptive_nee(W, H, self.sample_count, self.bounce_count, min_spp, step_spp, threshold,
                                                                         env=self.environment_factor, seed=self.seed, flags=flags, candidates=candidates)
        return self._denoise_counts(a, b, min_spp, split_emission) if denoise else self._ctx.accum_mean(a, b, out=a)

    def render_nee(self, flags=0, candidates=1):
        """Radiance SUMS [H,W,4] of the frame with next-event estimation towards the scene's emissive triangles (Scene.render_nee):
        render_accum()'s samples plus one MIS-weighted light sample per continuing vertex. flags: ptx_nee_cfg.flags (NEE_FUSED: the same
        frame from one kernel launch per pass; NEE_ENV_SAMPLES: light samples towards `environment` too); candidates: the light sample picked among that many (NEE_CANDIDATES).
        `last_nee_stats` holds the stats."""
        if self._scene is None:
            raise PtxError(ERR_INVALID, "render_nee() before load_gltf()")
        if self.transparent_background:
            raise PtxError(ERR_UNSUPPORTED, "render_nee: transparent_background's blend is not built on this estimator")
        W, H = self.resolution
        self._apply_lens()
        if self.environment != getattr(self, "_env_set", None):
            self._scene.set_environment(self.environment)
            self._env_set = self.environment
        accum, self.last_nee_stats = self._scene.render_nee(W, H, self.sample_count, self.bounce_count, env=self.environment_factor, seed=self.seed,
                                                                    flags=flags, candidates=candidates)
        return accum

    def render(self):
        W, H = self.resolution
        accum = self.render_accum()
        # the blended means of the transparent mode are written as they are: spp = 1 (x / 1.0f is exact)
        return encode_png(self._ctx.tonemap_encode(accum, W, H, 1 if self.transparent_background else self.sample_count))
