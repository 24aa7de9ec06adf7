"""ctypes mirror of include/apd_hip.h and a thin Python driver for libapd_hip.so.

This is plumbing for tests and bench.py: the product is the C-ABI library itself. The structures
below are byte-for-byte the C ones; `ProblemArrays` keeps the numpy buffers alive while a call is in
flight. Loading fails loudly (ApdError) when the HIP library is missing: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIB_PATH = os.environ.get("APD_LIB") or os.path.join(HERE, "lib", "libapd_hip.so")  # APD_LIB: A/B tooling

MAX_IMAGES = 32
ANCHOR_NUM = 9
FIRST_INIT, REFINE_INIT, REFINE_ITER = 0, 1, 2
WEAK, STRONG, UNKNOWN = 0, 1, 2

# apd_profile_kernel kinds and apd_profile_counters slots (include/apd_hip.h)
PROF_STRONG_SWEEP, PROF_RANSAC_FIT, PROF_WEAK_CAND, PROF_WEAK_SWEEP = 0, 1, 2, 3
PROF_DEPTH_TO_WEAK, PROF_GP_COST, PROF_WEAK_CAND_G, PROF_WEAK_CAND_COMB, PROF_WEAK_PATH = 4, 5, 6, 7, 8
# apd_hip.h's counters: [0] NCC-Old (Strong sweep), [1] NCC-New (Weak sweep, algorithmic), [2] geometric
# terms (Weak sweep), [3] NCC-Old (DepthToWeak), [4] geometric terms (DepthToWeak), [5] pair windows
# (k_gp_cost), [6] centre windows (k_weak_cand_g), [7] centre / [8] anchor windows (k_sweep_weak_vm)
PROF_COUNTERS = 9

STATUS = {0: "APD_OK", -1: "APD_EINVAL", -2: "APD_ENOMEM", -3: "APD_EDEVICE", -4: "APD_ETOOMANYVIEWS",
          -5: "APD_ESTATE"}


class ApdError(RuntimeError):
    pass


class ApdCamera(C.Structure):
    _fields_ = [("K", C.c_float * 9), ("R", C.c_float * 9), ("t", C.c_float * 3), ("c", C.c_float * 3),
                ("height", C.c_int32), ("width", C.c_int32), ("depth_min", C.c_float), ("depth_max", C.c_float),
                ("interval", C.c_float), ("depth_num", C.c_float)]


assert C.sizeof(ApdCamera) == 120


class ApdParams(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("num_images", C.c_int32), ("top_k", C.c_int32),
                ("depth_min", C.c_float), ("depth_max", C.c_float), ("geom_consistency", C.c_int32),
                ("use_impetus", C.c_int32), ("strong_radius", C.c_int32), ("strong_increment", C.c_int32),
                ("weak_radius", C.c_int32), ("weak_increment", C.c_int32), ("use_APD", C.c_int32),
                ("use_sa", C.c_int32), ("weak_peak_radius", C.c_int32), ("rotate_time", C.c_int32),
                ("ransac_threshold", C.c_float), ("geom_factor", C.c_float), ("state", C.c_int32)]


class ApdProblem(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("num_images", C.c_int32),
                ("images", C.POINTER(C.POINTER(C.c_float))), ("cameras", C.POINTER(ApdCamera)),
                ("params", ApdParams), ("depths", C.POINTER(C.POINTER(C.c_float))),
                ("init_planes", C.POINTER(C.c_float)), ("weak_info", C.POINTER(C.c_uint8)),
                ("confidence", C.POINTER(C.c_uint8)), ("sa_mask", C.POINTER(C.c_uint8)), ("seed", C.c_uint64),
                ("export_reliable_curve", C.c_int32)]


class ApdOutputs(C.Structure):
    _fields_ = [("planes", C.POINTER(C.c_float)), ("weak_info", C.POINTER(C.c_uint8)),
                ("confidence", C.POINTER(C.c_uint8)), ("costs", C.POINTER(C.c_float)),
                ("selected_views", C.POINTER(C.c_uint32)), ("view_weights", C.POINTER(C.c_uint8)),
                ("anchors", C.POINTER(C.c_int16)), ("weak_count", C.POINTER(C.c_int32)),
                ("reliable_curve", C.POINTER(C.c_float))]


class ApdTiming(C.Structure):
    _fields_ = [("total_ms", C.c_float), ("init_ms", C.c_float), ("anchors_ms", C.c_float),
                ("sweep_ms", C.c_float), ("post_ms", C.c_float), ("iter_ms", C.c_float * 8),
                ("iterations", C.c_int32), ("lists_ms", C.c_float), ("pairs_ms", C.c_float),
                ("join_ms", C.c_float), ("prepare_ms", C.c_float)]


def default_params(num_images: int, depth_min: float, depth_max: float, **kw) -> ApdParams:
    """PatchMatchParams defaults (main.h:80-100) with the scaled depth range (APD.cpp:554-555)."""
    p = ApdParams(max_iterations=3, num_images=num_images, top_k=4, depth_min=depth_min, depth_max=depth_max,
                  geom_consistency=0, use_impetus=1, strong_radius=5, strong_increment=2, weak_radius=5,
                  weak_increment=5, use_APD=0, use_sa=1, weak_peak_radius=6, rotate_time=4,
                  ransac_threshold=0.005, geom_factor=0.2, state=FIRST_INIT)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ptr(a, ctype):
    """ctypes pointer to a numpy array's or a torch tensor's data (host or device memory: the C ABI
    accepts device pointers for the problem arrays and the outputs)."""
    if a is None:
        return C.POINTER(ctype)()
    if hasattr(a, "data_ptr"):
        return C.cast(C.c_void_p(a.data_ptr()), C.POINTER(ctype))
    return a.ctypes.data_as(C.POINTER(ctype))


_TORCH_DTYPES = {np.dtype(np.float32): "float32", np.dtype(np.uint8): "uint8", np.dtype(np.int32): "int32"}


def _torch_device_sync(*objs):
    """Wait for torch's current stream on the device of every CUDA tensor in `objs` (lists/tuples
    are searched one level deep). The library works on its own non-blocking HIP stream, which does
    not wait for torch's stream or for RCCL's: a tensor torch (an index_select, a .to(), a cat, an
    all_gather) has just produced may still be in flight when the library reads it, and a fresh
    torch.empty may reuse memory a pending torch kernel still touches."""
    seen = set()
    for o in objs:
        for t in (o if isinstance(o, (list, tuple)) else (o,)):
            if t is None or not hasattr(t, "is_cuda") or not t.is_cuda:
                continue
            if t.device.index in seen:
                continue
            seen.add(t.device.index)
            import torch
            torch.cuda.current_stream(t.device).synchronize()


def _keep(a, dtype):
    """A contiguous buffer of `dtype` holding `a` (numpy array or torch tensor, kept as a tensor)."""
    if a is None:
        return None
    if hasattr(a, "data_ptr"):
        import torch
        t = a.contiguous()
        want = getattr(torch, _TORCH_DTYPES[np.dtype(dtype)])
        return t if t.dtype == want else t.to(want)
    return np.ascontiguousarray(a, dtype)


@dataclass
class ProblemArrays:
    """Owns every numpy buffer an ApdProblem points into."""
    width: int
    height: int
    images: Sequence[np.ndarray]
    cameras: Sequence[dict]
    params: ApdParams
    depths: Optional[Sequence[np.ndarray]] = None
    init_planes: Optional[np.ndarray] = None  # HxWx4 {world normal, depth}
    weak_info: Optional[np.ndarray] = None
    confidence: Optional[np.ndarray] = None
    sa_mask: Optional[np.ndarray] = None
    seed: int = 0x5EED
    export_reliable_curve: bool = False

    def build(self) -> ApdProblem:
        n = len(self.images)
        self._imgs = [_keep(i, np.float32) for i in self.images]
        self._img_ptrs = (C.POINTER(C.c_float) * n)(*[_ptr(i, C.c_float) for i in self._imgs])
        self._cams = (ApdCamera * n)()
        for i, cv in enumerate(self.cameras):
            cam = self._cams[i]
            for k, v in cv.items():
                if isinstance(v, np.ndarray):
                    getattr(cam, k)[:] = [float(x) for x in v]
                else:
                    setattr(cam, k, v)
        if self.depths is not None:
            self._deps = [_keep(d, np.float32) for d in self.depths]
            dptrs = (C.POINTER(C.c_float) * n)(*[_ptr(d, C.c_float) for d in self._deps])
            self._dep_ptrs = dptrs
        else:
            self._dep_ptrs = None
        self._planes = _keep(self.init_planes, np.float32)
        self._weak = _keep(self.weak_info, np.uint8)
        self._conf = _keep(self.confidence, np.uint8)
        self._sa = _keep(self.sa_mask, np.uint8)
        pb = ApdProblem()
        pb.width, pb.height, pb.num_images = self.width, self.height, n
        pb.images = C.cast(self._img_ptrs, C.POINTER(C.POINTER(C.c_float)))
        pb.cameras = C.cast(self._cams, C.POINTER(ApdCamera))
        pb.params = self.params
        pb.params.num_images = n
        pb.depths = C.cast(self._dep_ptrs, C.POINTER(C.POINTER(C.c_float))) if self._dep_ptrs is not None \
            else C.POINTER(C.POINTER(C.c_float))()
        pb.init_planes = _ptr(self._planes, C.c_float)
        pb.weak_info = _ptr(self._weak, C.c_uint8)
        pb.confidence = _ptr(self._conf, C.c_uint8)
        pb.sa_mask = _ptr(self._sa, C.c_uint8)
        pb.seed = self.seed
        pb.export_reliable_curve = int(self.export_reliable_curve)
        self._pb = pb
        return pb


class Outputs:
    """Host buffers for apd_outputs, allocated for one problem size."""

    def __init__(self, width: int, height: int, num_src: int, want_curve: bool = False, max_weak: int = 0):
        hw = width * height
        self.planes = np.zeros((height, width, 4), np.float32)
        self.weak_info = np.zeros((height, width), np.uint8)
        self.confidence = np.zeros((height, width), np.uint8)
        self.costs = np.zeros((height, width), np.float32)
        self.selected_views = np.zeros((height, width), np.uint32)
        self.view_weights = np.zeros((num_src, height, width), np.uint8)
        # anchors are only requested when the caller sizes them (weak_count <= max_weak): the library
        # writes weak_count * 9 entries, so an undersized buffer must never be handed over
        self.anchors = np.zeros((max_weak, ANCHOR_NUM, 2), np.int16) if max_weak > 0 else None
        self.weak_count = np.zeros(1, np.int32)
        self.reliable_curve = np.zeros((hw, 61), np.float32) if want_curve else None

    def struct(self) -> ApdOutputs:
        o = ApdOutputs()
        o.planes = _ptr(self.planes, C.c_float)
        o.weak_info = _ptr(self.weak_info, C.c_uint8)
        o.confidence = _ptr(self.confidence, C.c_uint8)
        o.costs = _ptr(self.costs, C.c_float)
        o.selected_views = _ptr(self.selected_views, C.c_uint32)
        o.view_weights = _ptr(self.view_weights, C.c_uint8)
        o.anchors = _ptr(self.anchors, C.c_int16)  # NULL when not sized
        o.weak_count = _ptr(self.weak_count, C.c_int32)
        o.reliable_curve = _ptr(self.reliable_curve, C.c_float)
        return o


EXPORTS = ["apd_abi_version", "apd_device_count", "apd_create", "apd_destroy", "apd_last_error",
           "apd_set_problem", "apd_run_patchmatch", "apd_stage_prepare", "apd_stage_iteration",
           "apd_stage_finish", "apd_synchronize", "apd_get_results", "apd_get_timing", "apd_get_prepare_timing", "apd_profile_reset",
           "apd_profile_query", "apd_profile_kernel", "apd_profile_counters", "apd_profile_evaluations", "apd_epilogue", "apd_device_alloc", "apd_device_free",
           "apd_device_copy", "apd_device_copy_peer", "apd_device_bytes", "apd_device_mem_info", "apd_device_resize_nearest", "apd_result_device", "apd_fusion_create", "apd_fusion_destroy",
           "apd_fusion_last_error", "apd_fusion_set_views", "apd_fusion_weak_filter", "apd_fusion_consistency",
           "apd_fusion_tat_levels"]

# include/apd_eval.h: its own list (EXPORTS is the apd_hip.h + apd_fusion.h set apd_abi_version() covers)
EVAL_EXPORTS = ["apd_eval_create", "apd_eval_destroy", "apd_eval_last_error", "apd_eval_set_target",
                "apd_eval_distances", "apd_eval_voxel_downsample", "apd_eval_get_timing",
                "apd_eval_render_depth", "apd_eval_visibility", "apd_eval_get_render_timing",
                "apd_eval_cube_cameras", "apd_eval_free_gap", "apd_eval_voxel_scores",
                "apd_eval_get_protocol_timing",
                "apd_eval_crop_volume", "apd_eval_crop_volume_host", "apd_eval_nearest", "apd_eval_nearest_host",
                "apd_eval_transform", "apd_eval_transform_host", "apd_eval_register", "apd_eval_register_host",
                "apd_eval_register_sums", "apd_eval_register_sums_host", "apd_eval_get_register_timing",
                "apd_eval_radius_thin", "apd_eval_radius_thin_host", "apd_eval_get_thin_timing", "apd_eval_dtu_ranks",
                "apd_eval_obs_mask", "apd_eval_obs_mask_host", "apd_eval_half_space", "apd_eval_half_space_host",
                "apd_eval_masked_stats", "apd_eval_masked_stats_host", "apd_eval_get_dtu_timing"]
REG_BLOCK = 1024  # APD_EVAL_REG_BLOCK
REG_SUMS = 19


class ApdEvalRegInfo(C.Structure):  # include/apd_eval.h
    _fields_ = [("iterations", C.c_int32), ("reserved", C.c_int32), ("n_corr", C.c_int64), ("n_finite", C.c_int64),
                ("fitness", C.c_double), ("rmse", C.c_double)]

    def as_dict(self) -> dict:
        return {"iterations": self.iterations, "n_corr": self.n_corr, "n_finite": self.n_finite,
                "fitness": self.fitness, "rmse": self.rmse}

# include/apd_prep.h
PREP_EXPORTS = ["apd_prep_create", "apd_prep_destroy", "apd_prep_last_error", "apd_prep_set_model",
                "apd_prep_pair_counts", "apd_prep_depth_ranks", "apd_prep_get_timing", "apd_prep_cos_gate"]
# include/apd_prep.h, the undistortion entries: a list of their own, because PREP_EXPORTS is pinned at
# the eight entries of scan preparation proper (tests/test_prep_host.py)
PREP_UNDISTORT_EXPORTS = ["apd_prep_undistort_bgr8", "apd_prep_get_undistort_timing", "apd_prep_undistort_bgr8_host",
                          "apd_prep_atan_c", "apd_prep_undistort_xy"]
# COLMAP's camera model ids and parameter counts (FOV, 7, is not supported)
PREP_CAMERA_MODELS = {"SIMPLE_PINHOLE": (0, 3), "PINHOLE": (1, 4), "SIMPLE_RADIAL": (2, 4), "RADIAL": (3, 5),
                      "OPENCV": (4, 8), "OPENCV_FISHEYE": (5, 8), "FULL_OPENCV": (6, 12),
                      "SIMPLE_RADIAL_FISHEYE": (8, 4), "RADIAL_FISHEYE": (9, 5), "THIN_PRISM_FISHEYE": (10, 12)}
PREP_MAX_IMAGES = 16384
# include/apd_seg.h: flat-zone sa_masks. A list of its own; EXPORTS, EVAL_EXPORTS and PREP_EXPORTS stay as they are
SEG_EXPORTS = ["apd_seg_create", "apd_seg_destroy", "apd_seg_last_error", "apd_seg_flat_zones_bgr8",
               "apd_seg_label_mask", "apd_seg_get_stage", "apd_seg_get_timing", "apd_seg_flat_zones_bgr8_host",
               "apd_seg_label_mask_host", "apd_seg_working_size", "apd_seg_label_colour"]
SEG_STAGES = {"work": 0, "smooth": 1, "flat": 2, "roots": 3, "areas": 4}
SEG_TIMES = ["upload_ms", "downscale_ms", "smooth_flat_ms", "ccl_tile_ms", "ccl_merge_ms", "flatten_area_ms",
             "rank_ms", "relabel_ms", "download_ms"]
SEG_MAX_LABELS = 255
PREP_ATOMICS_DEFAULT, PREP_ATOMICS_GLOBAL, PREP_ATOMICS_LDS = 0, 1, 2


def camera_from_values(v) -> ApdCamera:
    """ApdCamera from a dict of its field values (synth.camera_struct_values)."""
    cam = ApdCamera()
    for name in ("K", "R", "t", "c"):
        if name in v:
            a = np.asarray(v[name], np.float32).ravel()
            setattr(cam, name, (C.c_float * len(a))(*[float(x) for x in a]))
    for name in ("height", "width"):
        setattr(cam, name, int(v[name]))
    for name in ("depth_min", "depth_max", "interval", "depth_num"):
        if name in v:
            setattr(cam, name, float(v[name]))
    return cam


class ApdFusionView(C.Structure):  # include/apd_fusion.h
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("camera", ApdCamera),
                ("depth", C.c_void_p), ("normal", C.c_void_p), ("weak", C.c_void_p), ("confidence", C.c_void_p)]


def torch_runtime_first():
    """One HIP runtime per process. torch ships its own libamdhip64 (soname libamdhip64.so.7) and its
    libraries load it by the file name libamdhip64.so: loaded after ours (/opt/rocm's, the same
    soname) it would be a second runtime, which finds no GPU. Loaded first, it satisfies our
    dependency too, so torch tensors and this library share one runtime (device pointers pass
    through the C ABI). Call before loading anything that links libapd_hip.so; without torch the
    library uses /opt/rocm's runtime."""
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def load_library(path: str = LIB_PATH) -> C.CDLL:
    if not os.path.exists(path):
        raise ApdError(f"libapd_hip.so not built at {path}: run `python -c 'import __graft_entry__ as g; g.build()'`")
    torch_runtime_first()
    lib = C.CDLL(path)
    lib.apd_abi_version.restype = C.c_int32
    lib.apd_device_count.restype = C.c_int32
    lib.apd_create.restype = C.c_void_p
    lib.apd_create.argtypes = [C.c_int32]
    lib.apd_destroy.argtypes = [C.c_void_p]
    lib.apd_last_error.restype = C.c_char_p
    lib.apd_last_error.argtypes = [C.c_void_p]
    for name in ["apd_run_patchmatch", "apd_stage_prepare", "apd_stage_finish", "apd_synchronize"]:
        getattr(lib, name).restype = C.c_int32
        getattr(lib, name).argtypes = [C.c_void_p]
    lib.apd_set_problem.restype = C.c_int32
    lib.apd_set_problem.argtypes = [C.c_void_p, C.POINTER(ApdProblem)]
    lib.apd_stage_iteration.restype = C.c_int32
    lib.apd_stage_iteration.argtypes = [C.c_void_p, C.c_int32]
    lib.apd_get_results.restype = C.c_int32
    lib.apd_get_results.argtypes = [C.c_void_p, C.POINTER(ApdOutputs)]
    lib.apd_get_timing.restype = C.c_int32
    lib.apd_get_timing.argtypes = [C.c_void_p, C.POINTER(ApdTiming)]
    lib.apd_get_prepare_timing.restype = C.c_int32
    lib.apd_get_prepare_timing.argtypes = [C.c_void_p, C.POINTER(ApdTiming)]
    lib.apd_profile_reset.restype = C.c_int32
    lib.apd_profile_reset.argtypes = [C.c_void_p, C.c_int32]
    lib.apd_profile_evaluations.restype = C.c_int32
    lib.apd_profile_evaluations.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.apd_profile_query.restype = C.c_int32
    lib.apd_profile_query.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int64)]
    lib.apd_profile_kernel.restype = C.c_int32
    lib.apd_profile_kernel.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                       C.POINTER(C.c_int64)]
    lib.apd_profile_counters.restype = C.c_int32
    lib.apd_profile_counters.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int32]
    lib.apd_device_alloc.restype = C.c_int32
    lib.apd_device_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
    lib.apd_device_free.restype = C.c_int32
    lib.apd_device_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.apd_device_copy.restype = C.c_int32
    lib.apd_device_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.apd_device_bytes.restype = C.c_int32
    lib.apd_device_bytes.argtypes = [C.c_void_p, C.POINTER(C.c_size_t)]
    lib.apd_device_mem_info.restype = C.c_int32
    lib.apd_device_mem_info.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    lib.apd_device_resize_nearest.restype = C.c_int32
    lib.apd_device_resize_nearest.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                              C.c_int32, C.c_int32]
    lib.apd_result_device.restype = C.c_int32
    lib.apd_result_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.apd_fusion_create.restype = C.c_void_p
    lib.apd_fusion_create.argtypes = [C.c_int32]
    lib.apd_fusion_destroy.argtypes = [C.c_void_p]
    lib.apd_fusion_last_error.restype = C.c_char_p
    lib.apd_fusion_last_error.argtypes = [C.c_void_p]
    lib.apd_fusion_set_views.restype = C.c_int32
    lib.apd_fusion_set_views.argtypes = [C.c_void_p, C.c_int32, C.POINTER(ApdFusionView)]
    lib.apd_fusion_weak_filter.restype = C.c_int32
    lib.apd_fusion_weak_filter.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_void_p]
    lib.apd_fusion_consistency.restype = C.c_int32
    lib.apd_fusion_consistency.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
    lib.apd_fusion_tat_levels.restype = C.c_int32
    lib.apd_fusion_tat_levels.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_float, C.c_float,
                                          C.c_void_p, C.c_void_p, C.c_void_p]
    lib.apd_epilogue.restype = C.c_int32
    lib.apd_epilogue.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_float), C.c_float, C.c_float,
                                 C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_uint8)]
    # include/apd_eval.h
    lib.apd_eval_create.restype = C.c_void_p
    lib.apd_eval_create.argtypes = [C.c_int32]
    lib.apd_eval_destroy.argtypes = [C.c_void_p]
    lib.apd_eval_last_error.restype = C.c_char_p
    lib.apd_eval_last_error.argtypes = [C.c_void_p]
    lib.apd_eval_set_target.restype = C.c_int32
    lib.apd_eval_set_target.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    lib.apd_eval_distances.restype = C.c_int32
    lib.apd_eval_distances.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_void_p]
    lib.apd_eval_voxel_downsample.restype = C.c_int32
    lib.apd_eval_voxel_downsample.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    lib.apd_eval_get_timing.restype = C.c_int32
    lib.apd_eval_get_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double)]
    lib.apd_eval_render_depth.restype = C.c_int32
    lib.apd_eval_render_depth.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(ApdCamera),
                                          C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    lib.apd_eval_visibility.restype = C.c_int32
    lib.apd_eval_visibility.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(ApdCamera),
                                        C.POINTER(C.c_void_p), C.c_float, C.c_void_p, C.c_void_p]
    lib.apd_eval_get_render_timing.restype = C.c_int32
    lib.apd_eval_get_render_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.apd_eval_cube_cameras.restype = C.c_int32
    lib.apd_eval_cube_cameras.argtypes = [C.c_void_p, C.c_int32, C.POINTER(ApdCamera)]
    lib.apd_eval_free_gap.restype = C.c_int32
    lib.apd_eval_free_gap.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(ApdCamera),
                                      C.POINTER(C.c_void_p), C.c_void_p]
    lib.apd_eval_voxel_scores.restype = C.c_int32
    lib.apd_eval_voxel_scores.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p,
                                          C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.apd_eval_get_protocol_timing.restype = C.c_int32
    lib.apd_eval_get_protocol_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    crop_tail = [C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_void_p,
                 C.c_void_p, C.c_void_p]
    lib.apd_eval_crop_volume.restype = C.c_int32
    lib.apd_eval_crop_volume.argtypes = [C.c_void_p] + crop_tail
    lib.apd_eval_crop_volume_host.restype = C.c_int32
    lib.apd_eval_crop_volume_host.argtypes = crop_tail
    lib.apd_eval_nearest.restype = C.c_int32
    lib.apd_eval_nearest.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p]
    lib.apd_eval_nearest_host.restype = C.c_int32
    lib.apd_eval_nearest_host.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_float, C.c_void_p,
                                          C.c_void_p]
    lib.apd_eval_transform.restype = C.c_int32
    lib.apd_eval_transform.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.apd_eval_transform_host.restype = C.c_int32
    lib.apd_eval_transform_host.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    reg_tail = [C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.c_double, C.c_double,
                C.c_void_p, C.POINTER(ApdEvalRegInfo)]
    lib.apd_eval_register.restype = C.c_int32
    lib.apd_eval_register.argtypes = [C.c_void_p] + reg_tail
    lib.apd_eval_register_host.restype = C.c_int32
    lib.apd_eval_register_host.argtypes = [C.c_int64, C.c_void_p] + reg_tail
    lib.apd_eval_register_sums.restype = C.c_int32
    lib.apd_eval_register_sums.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    lib.apd_eval_register_sums_host.restype = C.c_int32
    lib.apd_eval_register_sums_host.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_float,
                                                C.c_void_p]
    lib.apd_eval_get_register_timing.restype = C.c_int32
    lib.apd_eval_get_register_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                 C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                                 C.POINTER(C.c_double)]
    thin_tail = [C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.apd_eval_radius_thin.restype = C.c_int32
    lib.apd_eval_radius_thin.argtypes = [C.c_void_p] + thin_tail
    lib.apd_eval_radius_thin_host.restype = C.c_int32
    lib.apd_eval_radius_thin_host.argtypes = thin_tail
    lib.apd_eval_get_thin_timing.restype = C.c_int32
    lib.apd_eval_get_thin_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                             C.POINTER(C.c_int32)]
    lib.apd_eval_dtu_ranks.restype = C.c_int32
    lib.apd_eval_dtu_ranks.argtypes = [C.c_int64, C.c_uint32, C.c_void_p]
    mask_tail = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    lib.apd_eval_obs_mask.restype = C.c_int32
    lib.apd_eval_obs_mask.argtypes = [C.c_void_p] + mask_tail
    lib.apd_eval_obs_mask_host.restype = C.c_int32
    lib.apd_eval_obs_mask_host.argtypes = mask_tail
    lib.apd_eval_half_space.restype = C.c_int32
    lib.apd_eval_half_space.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.apd_eval_half_space_host.restype = C.c_int32
    lib.apd_eval_half_space_host.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    stats_tail = [C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.POINTER(C.c_int64), C.POINTER(C.c_double),
                  C.POINTER(C.c_double)]
    lib.apd_eval_masked_stats.restype = C.c_int32
    lib.apd_eval_masked_stats.argtypes = [C.c_void_p] + stats_tail
    lib.apd_eval_masked_stats_host.restype = C.c_int32
    lib.apd_eval_masked_stats_host.argtypes = stats_tail
    lib.apd_eval_get_dtu_timing.restype = C.c_int32
    lib.apd_eval_get_dtu_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                            C.POINTER(C.c_double)]
    # include/apd_prep.h
    lib.apd_prep_create.restype = C.c_void_p
    lib.apd_prep_create.argtypes = [C.c_int32]
    lib.apd_prep_destroy.argtypes = [C.c_void_p]
    lib.apd_prep_last_error.restype = C.c_char_p
    lib.apd_prep_last_error.argtypes = [C.c_void_p]
    lib.apd_prep_set_model.restype = C.c_int32
    lib.apd_prep_set_model.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.apd_prep_pair_counts.restype = C.c_int32
    lib.apd_prep_pair_counts.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_uint64)]
    lib.apd_prep_depth_ranks.restype = C.c_int32
    lib.apd_prep_depth_ranks.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.apd_prep_get_timing.restype = C.c_int32
    lib.apd_prep_get_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.apd_prep_cos_gate.restype = C.c_double
    lib.apd_prep_cos_gate.argtypes = [C.c_double]
    lib.apd_prep_undistort_bgr8.restype = C.c_int32
    lib.apd_prep_undistort_bgr8.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.apd_prep_get_undistort_timing.restype = C.c_int32
    lib.apd_prep_get_undistort_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                  C.POINTER(C.c_double)]
    lib.apd_prep_undistort_bgr8_host.restype = C.c_int32
    lib.apd_prep_undistort_bgr8_host.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                                 C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.apd_prep_atan_c.restype = C.c_double
    lib.apd_prep_atan_c.argtypes = [C.c_double]
    lib.apd_prep_undistort_xy.restype = C.c_int32
    lib.apd_prep_undistort_xy.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.POINTER(C.c_int64)]
    # include/apd_seg.h
    lib.apd_seg_create.restype = C.c_void_p
    lib.apd_seg_create.argtypes = [C.c_int32]
    lib.apd_seg_destroy.argtypes = [C.c_void_p]
    lib.apd_seg_last_error.restype = C.c_char_p
    lib.apd_seg_last_error.argtypes = [C.c_void_p]
    i32p = C.POINTER(C.c_int32)
    lib.apd_seg_flat_zones_bgr8.restype = C.c_int32
    lib.apd_seg_flat_zones_bgr8.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_void_p, i32p, i32p, i32p, i32p]
    lib.apd_seg_label_mask.restype = C.c_int32
    lib.apd_seg_label_mask.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.apd_seg_get_stage.restype = C.c_int32
    lib.apd_seg_get_stage.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.apd_seg_get_timing.restype = C.c_int32
    lib.apd_seg_get_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    lib.apd_seg_flat_zones_bgr8_host.restype = C.c_int32
    lib.apd_seg_flat_zones_bgr8_host.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                 C.c_void_p, i32p, i32p, i32p, i32p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
    lib.apd_seg_label_mask_host.restype = C.c_int32
    lib.apd_seg_label_mask_host.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.apd_seg_working_size.restype = C.c_int32
    lib.apd_seg_working_size.argtypes = [C.c_int32, C.c_int32, C.c_int32, i32p, i32p, i32p]
    lib.apd_seg_label_colour.restype = None
    lib.apd_seg_label_colour.argtypes = [C.c_int32, C.c_void_p]
    return lib


class _Context:
    """What the five engine classes share: one device context of the library, made by
    <PREFIX>_create, asked by <PREFIX>_last_error and given back by <PREFIX>_destroy."""

    PREFIX = ""

    def __init__(self, device: int = 0, lib: Optional[C.CDLL] = None):
        self.lib = lib or load_library()
        self.device = device
        self._last_error = getattr(self.lib, self.PREFIX + "_last_error")
        self.ctx = getattr(self.lib, self.PREFIX + "_create")(device)
        if not self.ctx:
            raise ApdError(f"{self.PREFIX}_create failed: " + (self._last_error(None) or b"?").decode())

    def _check(self, st: int, what: str):
        if st != 0:
            msg = (self._last_error(self.ctx) or b"").decode()
            raise ApdError(f"{what} -> {STATUS.get(st, st)}: {msg}")

    def close(self):
        if self.ctx:
            getattr(self.lib, self.PREFIX + "_destroy")(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FusionEngine(_Context):
    """One apd_fusion_ctx (include/apd_fusion.h) with its views resident on the device."""

    PREFIX = "apd_fusion"

    def set_views(self, views):
        """views: dicts with depth (H,W) f32, normal (H,W,3) f32, weak/conf (H,W) u8, cam ApdCamera."""
        self._views = views
        arr = (ApdFusionView * len(views))()
        for i, v in enumerate(views):
            arr[i] = ApdFusionView(v["depth"].shape[1], v["depth"].shape[0], v["cam"], v["depth"].ctypes.data,
                                   v["normal"].ctypes.data, v["weak"].ctypes.data, v["conf"].ctypes.data)
        self._check(self.lib.apd_fusion_set_views(self.ctx, len(views), arr), "apd_fusion_set_views")

    def weak_filter(self, ref: int, q_view: float) -> np.ndarray:
        out = np.zeros(self._views[ref]["depth"].shape, np.uint8)
        self._check(self.lib.apd_fusion_weak_filter(self.ctx, ref, q_view, out.ctypes.data), "apd_fusion_weak_filter")
        return out

    def consistency(self, ref: int, src: Sequence[int], q_angle: float):
        H, W = self._views[ref]["depth"].shape
        s = np.asarray(src, np.int32)
        pix = np.zeros((H, W, len(s)), np.int32)
        er = np.zeros((H, W, len(s)), np.float32)
        q = np.zeros((H, W, len(s)), np.float32)
        self._check(self.lib.apd_fusion_consistency(self.ctx, ref, len(s), s.ctypes.data, q_angle, pix.ctypes.data,
                                                    er.ctypes.data, q.ctypes.data), "apd_fusion_consistency")
        return pix, er, q

    def tat_levels(self, ref: int, src: Sequence[int], dist_base: float, depth_base: float, q_k=None):
        H, W = self._views[ref]["depth"].shape
        s = np.asarray(src, np.int32)
        pix = np.zeros((H, W, len(s)), np.int32)
        lv = np.zeros((H, W, len(s)), np.uint8)
        qk = None if q_k is None else np.asarray(q_k, np.float32)
        self._check(self.lib.apd_fusion_tat_levels(self.ctx, ref, len(s), s.ctypes.data, dist_base, depth_base,
                                                   None if qk is None else qk.ctypes.data, pix.ctypes.data,
                                                   lv.ctypes.data), "apd_fusion_tat_levels")
        return pix, lv

ETH3D_TOLERANCES = (0.01, 0.02, 0.05, 0.1, 0.2, 0.5)  # the ones tools/eval_eth_train.py passes


def cube_cameras(origin, size: int, lib: Optional[C.CDLL] = None):
    """The six ApdCamera faces (+X, -X, +Y, -Y, +Z, -Z) of a cube map of size x size pixels centred at
    origin (apd_eval_cube_cameras). Host only: needs no GPU."""
    lib = lib or load_library()
    o = np.ascontiguousarray(origin, np.float32).reshape(-1)
    if len(o) != 3:
        raise ValueError("origin is three floats")
    arr = (ApdCamera * 6)()
    st = lib.apd_eval_cube_cameras(o.ctypes.data, int(size), arr)
    if st != 0:
        raise ApdError(f"apd_eval_cube_cameras -> {STATUS.get(st, st)}: size outside 2..16384 or a non-finite origin")
    return [arr[i] for i in range(6)]


def _mat4(T):
    """None, or a contiguous float64 array of 16 (row-major 4x4)."""
    if T is None:
        return None
    m = np.ascontiguousarray(T, np.float64).reshape(-1)
    if m.size != 16:
        raise ValueError("a transform is 4x4")
    return m


def _polygon(polygon):
    poly = np.ascontiguousarray(polygon, np.float64)
    if poly.ndim != 2 or poly.shape[1] != 2:
        raise ValueError("a polygon is (m, 2) float64")
    return poly, int(poly.shape[0])


def _host_cloud(xyz):
    a = np.ascontiguousarray(xyz, np.float32)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"a cloud is (n, 3) float32, got shape {a.shape}")
    return a, int(a.shape[0]), (a.ctypes.data if a.shape[0] else None)


def _host_status(st: int, what: str, allow_state: bool = False):
    if st != 0 and not (allow_state and STATUS.get(st) == "APD_ESTATE"):
        raise ApdError(f"{what} -> {STATUS.get(st, st)}")


def crop_volume_host(xyz, axis: int, axis_min: float, axis_max: float, polygon, T=None,
                     lib: Optional[C.CDLL] = None) -> np.ndarray:
    """apd_eval_crop_volume_host: the crop rule on one host thread. Needs no GPU."""
    lib = lib or load_library()
    a, n, addr = _host_cloud(xyz)
    poly, m = _polygon(polygon)
    Tm = _mat4(T)
    keep = np.empty(max(n, 1), np.int32)
    n_keep = C.c_int64(0)
    _host_status(lib.apd_eval_crop_volume_host(n, addr, None if Tm is None else Tm.ctypes.data, int(axis),
                                               float(axis_min), float(axis_max), m, poly.ctypes.data, keep.ctypes.data,
                                               C.addressof(n_keep)), "apd_eval_crop_volume_host")
    return keep[:n_keep.value].copy()


def nearest_host(target, xyz, max_dist: float, lib: Optional[C.CDLL] = None):
    """apd_eval_nearest_host: (dist, idx) of xyz against target. Needs no GPU."""
    lib = lib or load_library()
    t, nt, taddr = _host_cloud(target)
    a, n, addr = _host_cloud(xyz)
    dist, idx = np.empty(n, np.float32), np.empty(n, np.int32)
    _host_status(lib.apd_eval_nearest_host(nt, taddr, n, addr, max_dist, dist.ctypes.data if n else None,
                                           idx.ctypes.data if n else None), "apd_eval_nearest_host")
    return dist, idx


def transform_host(xyz, T=None, lib: Optional[C.CDLL] = None) -> np.ndarray:
    lib = lib or load_library()
    a, n, addr = _host_cloud(xyz)
    Tm = _mat4(T)
    out = np.empty((n, 3), np.float32)
    _host_status(lib.apd_eval_transform_host(n, addr, None if Tm is None else Tm.ctypes.data,
                                             out.ctypes.data if n else None), "apd_eval_transform_host")
    return out


def register_sums_host(target, xyz, max_corr: float, T=None, lib: Optional[C.CDLL] = None) -> np.ndarray:
    lib = lib or load_library()
    t, nt, taddr = _host_cloud(target)
    a, n, addr = _host_cloud(xyz)
    Tm = _mat4(T)
    out = np.zeros(REG_SUMS, np.float64)
    _host_status(lib.apd_eval_register_sums_host(nt, taddr, n, addr, None if Tm is None else Tm.ctypes.data, max_corr,
                                                 out.ctypes.data), "apd_eval_register_sums_host")
    return out


def register_host(target, xyz, max_corr: float, T0=None, with_scale: bool = True, max_iter: int = 30,
                  eps_fitness: float = 1e-6, eps_rmse: float = 1e-6, lib: Optional[C.CDLL] = None):
    """apd_eval_register_host: (T float64[4, 4], info dict, status); APD_ESTATE is returned, not raised."""
    lib = lib or load_library()
    t, nt, taddr = _host_cloud(target)
    a, n, addr = _host_cloud(xyz)
    T0m = _mat4(T0)
    T = np.zeros(16, np.float64)
    info = ApdEvalRegInfo()
    st = lib.apd_eval_register_host(nt, taddr, n, addr, None if T0m is None else T0m.ctypes.data, max_corr,
                                    int(bool(with_scale)), int(max_iter), float(eps_fitness), float(eps_rmse),
                                    T.ctypes.data, C.byref(info))
    _host_status(st, "apd_eval_register_host", allow_state=True)
    return T.reshape(4, 4), info.as_dict(), st


def dtu_ranks(n: int, seed: int = 0, lib: Optional[C.CDLL] = None) -> np.ndarray:
    """rank[i] = word 0 of Philox4x32-10 with counter (i, 0, 0, 0) and key (seed, 0): the order in which
    `apd_eval --dtu_gt` thins a cloud (apd_eval_dtu_ranks). Needs no GPU."""
    lib = lib or load_library()
    rank = np.empty(int(n), np.uint32)
    _host_status(lib.apd_eval_dtu_ranks(int(n), int(seed) & 0xFFFFFFFF, rank.ctypes.data if n else None),
                 "apd_eval_dtu_ranks")
    return rank


def _host_rank(rank, n: int):
    if rank is None:
        return None
    r = np.ascontiguousarray(rank, np.uint32).reshape(-1)
    if len(r) != n:
        raise ValueError("rank holds one uint32 per point")
    return r


def _mask_geometry(mask, origin):
    m = np.asarray(mask)
    if m.ndim != 3:
        raise ValueError("a mask is a 3-D array")
    # bytes in MATLAB's column-major order: the first index runs fastest
    flat = np.ascontiguousarray((m != 0).astype(np.uint8).ravel(order="F"))
    dims = np.ascontiguousarray(m.shape, np.int32)
    org = np.ascontiguousarray(origin, np.float64).reshape(-1)
    if org.size != 3:
        raise ValueError("origin is three doubles")
    return flat, dims, org


def radius_thin_host(xyz, radius: float, rank=None, lib: Optional[C.CDLL] = None) -> np.ndarray:
    """apd_eval_radius_thin_host: the ascending indices of the greedy radius thinning. Needs no GPU."""
    lib = lib or load_library()
    a, n, addr = _host_cloud(xyz)
    r = _host_rank(rank, n)
    keep = np.empty(max(n, 1), np.int32)
    n_keep = C.c_int64(0)
    _host_status(lib.apd_eval_radius_thin_host(n, addr, radius, None if r is None or n == 0 else r.ctypes.data,
                                               keep.ctypes.data, C.addressof(n_keep)), "apd_eval_radius_thin_host")
    return keep[:n_keep.value].copy()


def obs_mask_host(xyz, mask, origin, res: float, lib: Optional[C.CDLL] = None) -> np.ndarray:
    """apd_eval_obs_mask_host: uint8[n], 1 where the point lies in a set cell of the 3-D mask."""
    lib = lib or load_library()
    a, n, addr = _host_cloud(xyz)
    flat, dims, org = _mask_geometry(mask, origin)
    inside = np.zeros(n, np.uint8)
    _host_status(lib.apd_eval_obs_mask_host(n, addr, dims.ctypes.data, org.ctypes.data, float(res), flat.ctypes.data,
                                            inside.ctypes.data if n else None), "apd_eval_obs_mask_host")
    return inside


def half_space_host(xyz, plane, lib: Optional[C.CDLL] = None) -> np.ndarray:
    """apd_eval_half_space_host: uint8[n], 1 where P0 x + P1 y + P2 z + P3 > 0."""
    lib = lib or load_library()
    a, n, addr = _host_cloud(xyz)
    P = np.ascontiguousarray(plane, np.float64).reshape(-1)
    if P.size != 4:
        raise ValueError("a plane is four doubles")
    above = np.zeros(n, np.uint8)
    _host_status(lib.apd_eval_half_space_host(n, addr, P.ctypes.data, above.ctypes.data if n else None),
                 "apd_eval_half_space_host")
    return above


def masked_stats_host(dist, flag, limit: float, lib: Optional[C.CDLL] = None) -> dict:
    """apd_eval_masked_stats_host: {"count", "sum", "median"} of the distances with flag set (None: all)
    that are <= limit."""
    lib = lib or load_library()
    d = np.ascontiguousarray(dist, np.float32).reshape(-1)
    f = None if flag is None else np.ascontiguousarray(flag, np.uint8).reshape(-1)
    if f is not None and len(f) != len(d):
        raise ValueError("flag holds one byte per distance")
    n = len(d)
    c, s, m = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
    _host_status(lib.apd_eval_masked_stats_host(n, d.ctypes.data if n else None,
                                                None if f is None or n == 0 else f.ctypes.data, limit, C.byref(c),
                                                C.byref(s), C.byref(m)), "apd_eval_masked_stats_host")
    return {"count": c.value, "sum": s.value, "median": m.value}


class EvalEngine(_Context):
    """One apd_eval_ctx (include/apd_eval.h): truncated nearest-neighbour distances to a target cloud,
    voxel down-sampling, z-buffer rendering and visibility, free gaps and voxel scores, crop volume,
    nearest neighbour with index, transform and ICP registration, radius thinning, observability mask,
    half-space and masked statistics. Clouds are (n, 3) float32: numpy arrays (results come back as numpy) or
    torch tensors on the context's device (results come back as tensors there; torch's current
    stream is waited for first, as for every device input of this library)."""

    PREFIX = "apd_eval"

    @staticmethod
    def _cloud(xyz):
        """(buffer kept alive, n, address or None, is_device)"""
        a = _keep(xyz, np.float32)
        if tuple(a.shape[1:]) != (3,) or len(a.shape) != 2:
            raise ValueError(f"a cloud is (n, 3) float32, got shape {tuple(a.shape)}")
        dev = hasattr(a, "data_ptr")
        n = int(a.shape[0])
        addr = (a.data_ptr() if dev else a.ctypes.data) if n else None
        return a, n, addr, dev

    def set_target_ptr(self, n: int, xyz_ptr):
        self._check(self.lib.apd_eval_set_target(self.ctx, n, xyz_ptr), "apd_eval_set_target")

    def set_target(self, xyz):
        a, n, addr, _ = self._cloud(xyz)
        _torch_device_sync(a)
        self.set_target_ptr(n, addr)

    def distances_ptr(self, n: int, xyz_ptr, max_dist: float, dist_ptr, num_tol: int = 0, tol_ptr=None,
                      within_ptr=None):
        self._check(self.lib.apd_eval_distances(self.ctx, n, xyz_ptr, max_dist, dist_ptr, num_tol, tol_ptr,
                                                within_ptr), "apd_eval_distances")

    def distances(self, xyz, max_dist: float, tolerances=None, want_dist: bool = True):
        """(dist float32[n] or None, within int64[k] or None)"""
        a, n, addr, dev = self._cloud(xyz)
        tol = None if tolerances is None else np.ascontiguousarray(tolerances, np.float32).reshape(-1)
        k = 0 if tol is None else len(tol)
        if dev:
            import torch
            dist = torch.empty(n, dtype=torch.float32, device=a.device) if want_dist else None
            within = torch.zeros(k, dtype=torch.int64, device=a.device) if tol is not None else None
            _torch_device_sync(a, dist, within)
            dptr = dist.data_ptr() if (dist is not None and n) else None
            wptr = within.data_ptr() if (within is not None and k) else None
        else:
            dist = np.empty(n, np.float32) if want_dist else None
            within = np.zeros(k, np.int64) if tol is not None else None
            dptr = dist.ctypes.data if (dist is not None and n) else None
            wptr = within.ctypes.data if (within is not None and k) else None
        self.distances_ptr(n, addr, max_dist, dptr, k, tol.ctypes.data if k else None, wptr)
        return dist, within

    def voxel_downsample_ptr(self, n: int, xyz_ptr, voxel: float, keep_ptr) -> int:
        n_keep = C.c_int64(0)
        self._check(self.lib.apd_eval_voxel_downsample(self.ctx, n, xyz_ptr, voxel, keep_ptr,
                                                       C.addressof(n_keep)), "apd_eval_voxel_downsample")
        return n_keep.value

    def voxel_downsample(self, xyz, voxel: float):
        """Ascending int32 indices of the lowest-index point of every occupied voxel."""
        a, n, addr, dev = self._cloud(xyz)
        if dev:
            import torch
            keep = torch.empty(max(n, 1), dtype=torch.int32, device=a.device)
            _torch_device_sync(a, keep)
            kptr = keep.data_ptr()
        else:
            keep = np.empty(max(n, 1), np.int32)
            kptr = keep.ctypes.data
        return keep[:self.voxel_downsample_ptr(n, addr, voxel, kptr)]

    def timing(self) -> dict:
        b, q, v = C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.apd_eval_get_timing(self.ctx, C.byref(b), C.byref(q), C.byref(v)), "apd_eval_get_timing")
        return {"build_ms": b.value, "query_ms": q.value, "voxel_ms": v.value}

    @staticmethod
    def _cams(cams):
        """ApdCamera array from ApdCamera structures or dicts of their field values
        (synth.camera_struct_values)."""
        arr = (ApdCamera * max(len(cams), 1))()
        for i, c in enumerate(cams):
            if isinstance(c, ApdCamera):
                arr[i] = c
            else:
                arr[i] = camera_from_values(c)
        return arr

    def render_depth_ptr(self, n: int, xyz_ptr, cams, splat: int, depth_ptrs, index_ptrs=None):
        """depth_ptrs / index_ptrs: one address (or None) per view; index_ptrs itself may be None."""
        arr = cams if isinstance(cams, C.Array) else self._cams(cams)
        nv = len(depth_ptrs)
        dp = (C.c_void_p * max(nv, 1))(*depth_ptrs)
        ip = None if index_ptrs is None else (C.c_void_p * max(nv, 1))(*index_ptrs)
        self._check(self.lib.apd_eval_render_depth(self.ctx, n, xyz_ptr, nv, arr, splat, dp, ip),
                    "apd_eval_render_depth")

    def render_depth(self, xyz, cams, splat: int = 0, want_index: bool = False):
        """z-buffer of the cloud in every camera: a list of (H, W) float32 depth maps (0 = nothing
        projects), or with want_index a list of (depth, index) pairs, index int32 with -1 there."""
        a, n, addr, dev = self._cloud(xyz)
        arr = self._cams(cams)
        shapes = [(int(arr[i].height), int(arr[i].width)) for i in range(len(cams))]
        if dev:
            import torch
            depth = [torch.empty(s, dtype=torch.float32, device=a.device) for s in shapes]
            index = [torch.empty(s, dtype=torch.int32, device=a.device) for s in shapes] if want_index else None
            _torch_device_sync(a, depth, index)
            addr_of = lambda t: t.data_ptr()
        else:
            depth = [np.empty(s, np.float32) for s in shapes]
            index = [np.empty(s, np.int32) for s in shapes] if want_index else None
            addr_of = lambda t: t.ctypes.data
        self.render_depth_ptr(n, addr, arr, splat, [addr_of(d) for d in depth],
                              None if index is None else [addr_of(i) for i in index])
        return list(zip(depth, index)) if want_index else depth

    def visibility_ptr(self, n: int, xyz_ptr, cams, depth_ptrs, rel_tol: float, seen_ptr) -> int:
        arr = cams if isinstance(cams, C.Array) else self._cams(cams)
        nv = len(depth_ptrs)
        dp = (C.c_void_p * max(nv, 1))(*depth_ptrs)
        n_any = C.c_int64(0)
        self._check(self.lib.apd_eval_visibility(self.ctx, n, xyz_ptr, nv, arr, dp, rel_tol, seen_ptr,
                                                 C.addressof(n_any)), "apd_eval_visibility")
        return n_any.value

    def visibility(self, xyz, cams, depths, rel_tol: float, want_any: bool = False):
        """seen int32[n]: in how many of the views point i passes the z-buffer test against depths[v]
        (an (H, W) float32 map per camera, numpy or torch). With want_any: (seen, #{seen > 0})."""
        a, n, addr, dev = self._cloud(xyz)
        arr = self._cams(cams)
        if len(depths) != len(cams):
            raise ValueError("one depth map per camera")
        maps = [_keep(d, np.float32) for d in depths]
        for i, m in enumerate(maps):
            if tuple(m.shape) != (int(arr[i].height), int(arr[i].width)):
                raise ValueError(f"depth map {i} has shape {tuple(m.shape)}, its camera {arr[i].height}x{arr[i].width}")
        if dev:
            import torch
            seen = torch.empty(n, dtype=torch.int32, device=a.device)
            sptr = seen.data_ptr() if n else None
        else:
            seen = np.empty(n, np.int32)
            sptr = seen.ctypes.data if n else None
        _torch_device_sync(a, seen, maps)
        ptrs = [m.data_ptr() if hasattr(m, "data_ptr") else m.ctypes.data for m in maps]
        n_any = self.visibility_ptr(n, addr, arr, ptrs, rel_tol, sptr)
        return (seen, n_any) if want_any else seen

    def render_timing(self) -> dict:
        r, v = C.c_double(), C.c_double()
        self._check(self.lib.apd_eval_get_render_timing(self.ctx, C.byref(r), C.byref(v)),
                    "apd_eval_get_render_timing")
        return {"render_ms": r.value, "visibility_ms": v.value}

    def free_gap_ptr(self, n: int, xyz_ptr, cams, depth_ptrs, gap_ptr):
        arr = cams if isinstance(cams, C.Array) else self._cams(cams)
        nv = len(depth_ptrs)
        dp = (C.c_void_p * max(nv, 1))(*depth_ptrs)
        self._check(self.lib.apd_eval_free_gap(self.ctx, n, xyz_ptr, nv, arr, dp, gap_ptr), "apd_eval_free_gap")

    def free_gap(self, xyz, cams, depths):
        """gap float32[n]: the largest `depth at the point's pixel - depth of the point` over the views
        whose map covers the point's centre pixel (-inf without one): how far in front of the
        surfaces of depths[v] (an (H, W) float32 map per camera, numpy or torch) the point lies."""
        a, n, addr, dev = self._cloud(xyz)
        arr = self._cams(cams)
        if len(depths) != len(cams):
            raise ValueError("one depth map per camera")
        maps = [_keep(d, np.float32) for d in depths]
        for i, m in enumerate(maps):
            if tuple(m.shape) != (int(arr[i].height), int(arr[i].width)):
                raise ValueError(f"depth map {i} has shape {tuple(m.shape)}, its camera {arr[i].height}x{arr[i].width}")
        if dev:
            import torch
            gap = torch.empty(n, dtype=torch.float32, device=a.device)
            gptr = gap.data_ptr() if n else None
        else:
            gap = np.empty(n, np.float32)
            gptr = gap.ctypes.data if n else None
        _torch_device_sync(a, gap, maps)
        ptrs = [m.data_ptr() if hasattr(m, "data_ptr") else m.ctypes.data for m in maps]
        self.free_gap_ptr(n, addr, arr, ptrs, gptr)
        return gap

    def voxel_scores_ptr(self, n: int, xyz_ptr, voxel: float, dist_ptr, gap_ptr, num_tol: int, tol_ptr, good_ptr,
                         bad_ptr, ratio_sum_ptr, voxels_ptr):
        self._check(self.lib.apd_eval_voxel_scores(self.ctx, n, xyz_ptr, voxel, dist_ptr, gap_ptr, num_tol, tol_ptr,
                                                   good_ptr, bad_ptr, ratio_sum_ptr, voxels_ptr),
                    "apd_eval_voxel_scores")

    def voxel_scores(self, xyz, voxel: float, dist, gap=None, tolerances=ETH3D_TOLERANCES) -> dict:
        """Per tolerance: good / bad point totals, the integer sum of the per-voxel fixed-point
        ratios (a << 32) // (a + b) and the number of voxels with a + b > 0 (include/apd_eval.h),
        as int64 arrays under "good", "bad", "ratio_sum", "voxels" (numpy, or tensors on the cloud's
        device), plus "score": ratio_sum / (voxels * 2^32) as a list of floats, 0 without voxels."""
        a, n, addr, dev = self._cloud(xyz)
        d = _keep(dist, np.float32)
        g = _keep(gap, np.float32)
        for name, v in (("dist", d), ("gap", g)):
            if v is not None and tuple(v.shape) != (n,):
                raise ValueError(f"{name} has shape {tuple(v.shape)}, the cloud {n} points")
        tol = np.ascontiguousarray(tolerances, np.float32).reshape(-1)
        k = len(tol)
        if dev:
            import torch
            outs = [torch.zeros(k, dtype=torch.int64, device=a.device) for _ in range(4)]
        else:
            outs = [np.zeros(k, np.int64) for _ in range(4)]
        _torch_device_sync(a, d, g, outs)
        ptr = lambda t: None if t is None or not len(t) else (t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data)
        self.voxel_scores_ptr(n, addr, voxel, ptr(d), ptr(g), k, ptr(tol), *[ptr(o) for o in outs])
        res = dict(zip(("good", "bad", "ratio_sum", "voxels"), outs))
        res["score"] = [float(int(r)) / (float(int(v)) * 4294967296.0) if int(v) else 0.0
                        for r, v in zip(res["ratio_sum"].tolist(), res["voxels"].tolist())]
        return res

    def protocol_timing(self) -> dict:
        f, s = C.c_double(), C.c_double()
        self._check(self.lib.apd_eval_get_protocol_timing(self.ctx, C.byref(f), C.byref(s)),
                    "apd_eval_get_protocol_timing")
        return {"free_gap_ms": f.value, "scores_ms": s.value}

    # ---- crop volume, nearest neighbour with index, transform, registration ----

    def crop_volume(self, xyz, axis: int, axis_min: float, axis_max: float, polygon, T=None):
        """Ascending int32 indices of the points inside the crop volume (apd_eval_crop_volume)."""
        a, n, addr, dev = self._cloud(xyz)
        poly, m = _polygon(polygon)
        Tm = _mat4(T)
        if dev:
            import torch
            keep = torch.empty(max(n, 1), dtype=torch.int32, device=a.device)
            _torch_device_sync(a, keep)
            kptr = keep.data_ptr()
        else:
            keep = np.empty(max(n, 1), np.int32)
            kptr = keep.ctypes.data
        n_keep = C.c_int64(0)
        self._check(self.lib.apd_eval_crop_volume(self.ctx, n, addr, None if Tm is None else Tm.ctypes.data, int(axis),
                                                  float(axis_min), float(axis_max), m, poly.ctypes.data, kptr,
                                                  C.addressof(n_keep)), "apd_eval_crop_volume")
        return keep[:n_keep.value]

    def nearest(self, xyz, max_dist: float):
        """(dist float32[n], idx int32[n]): apd_eval_distances' values plus the lowest target index that
        attains each, -1 where the distance is +inf."""
        a, n, addr, dev = self._cloud(xyz)
        if dev:
            import torch
            dist = torch.empty(n, dtype=torch.float32, device=a.device)
            idx = torch.empty(n, dtype=torch.int32, device=a.device)
            _torch_device_sync(a, dist, idx)
            dptr, iptr = (dist.data_ptr(), idx.data_ptr()) if n else (None, None)
        else:
            dist, idx = np.empty(n, np.float32), np.empty(n, np.int32)
            dptr, iptr = (dist.ctypes.data, idx.ctypes.data) if n else (None, None)
        self._check(self.lib.apd_eval_nearest(self.ctx, n, addr, max_dist, dptr, iptr), "apd_eval_nearest")
        return dist, idx

    def transform(self, xyz, T=None):
        """The cloud under the 4x4 double transform T, rounded to float32 (apd_eval_transform)."""
        a, n, addr, dev = self._cloud(xyz)
        Tm = _mat4(T)
        if dev:
            import torch
            out = torch.empty((n, 3), dtype=torch.float32, device=a.device)
            _torch_device_sync(a, out)
            optr = out.data_ptr() if n else None
        else:
            out = np.empty((n, 3), np.float32)
            optr = out.ctypes.data if n else None
        self._check(self.lib.apd_eval_transform(self.ctx, n, addr, None if Tm is None else Tm.ctypes.data, optr),
                    "apd_eval_transform")
        return out

    def register(self, xyz, max_corr: float, T0=None, with_scale: bool = True, max_iter: int = 30,
                 eps_fitness: float = 1e-6, eps_rmse: float = 1e-6, raise_on_state: bool = True):
        """Point-to-point ICP of xyz against the current target: (T float64[4, 4], info dict, status).
        With raise_on_state False an APD_ESTATE outcome (fewer than 3 correspondences) is returned
        instead of raised."""
        a, n, addr, _ = self._cloud(xyz)
        _torch_device_sync(a)
        T0m = _mat4(T0)
        T = np.zeros(16, np.float64)
        info = ApdEvalRegInfo()
        st = self.lib.apd_eval_register(self.ctx, n, addr, None if T0m is None else T0m.ctypes.data, max_corr,
                                        int(bool(with_scale)), int(max_iter), float(eps_fitness), float(eps_rmse),
                                        T.ctypes.data, C.byref(info))
        if st != 0 and (raise_on_state or STATUS.get(st) != "APD_ESTATE"):
            self._check(st, "apd_eval_register")
        return T.reshape(4, 4), info.as_dict(), st

    def register_sums(self, xyz, max_corr: float, T=None) -> np.ndarray:
        """The 19 sums of one evaluation of T (include/apd_eval.h)."""
        a, n, addr, _ = self._cloud(xyz)
        _torch_device_sync(a)
        Tm = _mat4(T)
        out = np.zeros(REG_SUMS, np.float64)
        self._check(self.lib.apd_eval_register_sums(self.ctx, n, addr, None if Tm is None else Tm.ctypes.data, max_corr,
                                                    out.ctypes.data), "apd_eval_register_sums")
        return out

    def register_timing(self) -> dict:
        e, f, s, c, t = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_double()
        k = C.c_int32()
        self._check(self.lib.apd_eval_get_register_timing(self.ctx, C.byref(e), C.byref(f), C.byref(s), C.byref(k),
                                                          C.byref(c), C.byref(t)), "apd_eval_get_register_timing")
        return {"eval_ms": e.value, "fold_ms": f.value, "solve_ms": s.value, "evaluations": k.value,
                "crop_ms": c.value, "transform_ms": t.value}

    # ---- radius thinning, observability mask, half-space, masked statistics ----

    def radius_thin(self, xyz, radius: float, rank=None):
        """Ascending int32 indices of the greedy radius thinning (apd_eval_radius_thin): visiting the
        points in ascending (rank, index), a point is kept iff no point kept before it lies within
        radius. rank: uint32 per point (a torch tensor: int32 holding the same bits), None = all equal."""
        a, n, addr, dev = self._cloud(xyz)
        if rank is not None and hasattr(rank, "data_ptr"):
            r = rank.contiguous().reshape(-1)
            if r.element_size() != 4 or r.numel() != n:
                raise ValueError("rank holds one 32-bit word per point")
            _torch_device_sync(r)
            rptr = r.data_ptr() if n else None
        else:
            r = _host_rank(rank, n)
            rptr = r.ctypes.data if (r is not None and n) else None
        if dev:
            import torch
            keep = torch.empty(max(n, 1), dtype=torch.int32, device=a.device)
            _torch_device_sync(a, keep)
            kptr = keep.data_ptr()
        else:
            keep = np.empty(max(n, 1), np.int32)
            kptr = keep.ctypes.data
        n_keep = C.c_int64(0)
        self._check(self.lib.apd_eval_radius_thin(self.ctx, n, addr, radius, rptr, kptr, C.addressof(n_keep)),
                    "apd_eval_radius_thin")
        return keep[:n_keep.value]

    def thin_timing(self) -> dict:
        s, r, k = C.c_double(), C.c_double(), C.c_int32()
        self._check(self.lib.apd_eval_get_thin_timing(self.ctx, C.byref(s), C.byref(r), C.byref(k)),
                    "apd_eval_get_thin_timing")
        return {"sort_ms": s.value, "rounds_ms": r.value, "rounds": k.value}

    def _flags_out(self, a, n: int, dev: bool):
        if dev:
            import torch
            out = torch.zeros(n, dtype=torch.uint8, device=a.device)
            _torch_device_sync(a, out)
            return out, (out.data_ptr() if n else None)
        out = np.zeros(n, np.uint8)
        return out, (out.ctypes.data if n else None)

    def obs_mask(self, xyz, mask, origin, res: float):
        """uint8[n]: 1 where round((x - origin) / res + 1) indexes a set cell of the 3-D array `mask`
        (apd_eval_obs_mask). The flattened mask is kept, here and on the device, while the same array
        object is given."""
        a, n, addr, dev = self._cloud(xyz)
        if getattr(self, "_mask_obj", None) is not mask:
            # the new bytes are made while the old ones are still alive, so they get another address
            # and the library, which knows a mask by its address and dims, uploads them
            flat, dims, _ = _mask_geometry(mask, origin)
            self._mask_obj, self._mask_flat, self._mask_dims = mask, flat, dims
        org = np.ascontiguousarray(origin, np.float64).reshape(-1)
        if org.size != 3:
            raise ValueError("origin is three doubles")
        inside, iptr = self._flags_out(a, n, dev)
        self._check(self.lib.apd_eval_obs_mask(self.ctx, n, addr, self._mask_dims.ctypes.data, org.ctypes.data,
                                               float(res), self._mask_flat.ctypes.data, iptr), "apd_eval_obs_mask")
        return inside

    def half_space(self, xyz, plane):
        """uint8[n]: 1 where P0 x + P1 y + P2 z + P3 > 0 in double (apd_eval_half_space)."""
        a, n, addr, dev = self._cloud(xyz)
        P = np.ascontiguousarray(plane, np.float64).reshape(-1)
        if P.size != 4:
            raise ValueError("a plane is four doubles")
        above, aptr = self._flags_out(a, n, dev)
        self._check(self.lib.apd_eval_half_space(self.ctx, n, addr, P.ctypes.data, aptr), "apd_eval_half_space")
        return above

    def masked_stats(self, dist, flag, limit: float) -> dict:
        """{"count", "sum", "median"} of the distances with flag set (None: all) that are <= limit
        (apd_eval_masked_stats); dist float32[n] and flag uint8[n] as numpy arrays or device tensors."""
        d = _keep(dist, np.float32).reshape(-1)
        f = None if flag is None else _keep(flag, np.uint8).reshape(-1)
        n = int(d.shape[0])
        if f is not None and int(f.shape[0]) != n:
            raise ValueError("flag holds one byte per distance")
        _torch_device_sync(d, f)

        def addr(t):
            if t is None or n == 0:
                return None
            return t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data
        c, s, m = C.c_int64(0), C.c_double(0.0), C.c_double(0.0)
        self._check(self.lib.apd_eval_masked_stats(self.ctx, n, addr(d), addr(f), limit, C.byref(c), C.byref(s),
                                                   C.byref(m)), "apd_eval_masked_stats")
        return {"count": c.value, "sum": s.value, "median": m.value}

    def dtu_timing(self) -> dict:
        m, h, s = C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.apd_eval_get_dtu_timing(self.ctx, C.byref(m), C.byref(h), C.byref(s)),
                    "apd_eval_get_dtu_timing")
        return {"mask_ms": m.value, "half_space_ms": h.value, "stats_ms": s.value}

def prep_cos_gate(degrees: float = 1.0, lib: Optional[C.CDLL] = None) -> float:
    """apd_prep_cos_gate: the smallest double q with (180/pi)*acos(q) < degrees. Host only."""
    return float((lib or load_library()).apd_prep_cos_gate(float(degrees)))


def prep_model_id(model) -> int:
    """COLMAP's id of a camera model given by name or id."""
    return PREP_CAMERA_MODELS[model][0] if isinstance(model, str) else int(model)


def prep_pinhole_K(model, params):
    """[fx, fy, cx, cy] of a camera's parameters (fx = fy = f for the f cx cy models)."""
    p = [float(v) for v in params]
    return [p[0], p[0], p[1], p[2]] if prep_model_id(model) in (0, 2, 3, 8, 9) else p[:4]


def _undistort_args(bgr, model, params, out_K, out_size):
    src = np.ascontiguousarray(bgr, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("bgr is (h, w, 3) uint8")
    p = np.ascontiguousarray(params, np.float64).reshape(-1)
    K = np.ascontiguousarray(prep_pinhole_K(model, p) if out_K is None else out_K, np.float64).reshape(-1)
    if len(K) != 4:
        raise ValueError("out_K is fx, fy, cx, cy")
    ow, oh = (src.shape[1], src.shape[0]) if out_size is None else (int(out_size[0]), int(out_size[1]))
    return src, p, K, ow, oh


def prep_undistort_host(bgr, model, params, out_K=None, out_size=None, lib: Optional[C.CDLL] = None) -> np.ndarray:
    """apd_prep_undistort_bgr8_host: the warp of include/apd_prep.h on the CPU. bgr (h, w, 3) uint8;
    out_K [fx, fy, cx, cy] (default: the source camera's); out_size (w, h) (default: the source's)."""
    src, p, K, ow, oh = _undistort_args(bgr, model, params, out_K, out_size)
    dst = np.empty((max(oh, 0), max(ow, 0), 3), np.uint8)
    st = (lib or load_library()).apd_prep_undistort_bgr8_host(prep_model_id(model), p.ctypes.data, len(p), src.shape[1],
                                                              src.shape[0], src.ctypes.data, K.ctypes.data, ow, oh,
                                                              dst.ctypes.data)
    if st != 0:
        raise ApdError(f"apd_prep_undistort_bgr8_host -> {STATUS.get(st, st)}")
    return dst


def prep_undistort_xy(xy, model, params, lib: Optional[C.CDLL] = None):
    """apd_prep_undistort_xy: (n, 2) distorted pixel coordinates -> ((n, 2) pinhole pixel coordinates with
    (-1, -1) where Newton's method did not converge, the number of those)."""
    pts = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    p = np.ascontiguousarray(params, np.float64).reshape(-1)
    out = np.empty_like(pts)
    bad = C.c_int64(0)
    st = (lib or load_library()).apd_prep_undistort_xy(prep_model_id(model), p.ctypes.data, len(p), len(pts),
                                                       pts.ctypes.data if len(pts) else None,
                                                       out.ctypes.data if len(pts) else None, C.byref(bad))
    if st != 0:
        raise ApdError(f"apd_prep_undistort_xy -> {STATUS.get(st, st)}")
    return out, int(bad.value)


class PrepEngine(_Context):
    """One apd_prep_ctx (include/apd_prep.h): pair counts by tracks and per-image depth order
    statistics of a sparse model. All arrays are numpy, in the layout of apd_prep_set_model."""

    PREFIX = "apd_prep"
    n_images = 0

    def set_model(self, rot, trans, centres, xyz, obs_offset, obs_point):
        r = np.ascontiguousarray(rot, np.float64).reshape(-1)
        t = np.ascontiguousarray(trans, np.float64).reshape(-1)
        c = np.ascontiguousarray(centres, np.float64).reshape(-1)
        x = np.ascontiguousarray(xyz, np.float64).reshape(-1)
        off = np.ascontiguousarray(obs_offset, np.int64).reshape(-1)
        pt = np.ascontiguousarray(obs_point, np.int32).reshape(-1)
        n = len(off) - 1
        if len(r) != 9 * n or len(t) != 3 * n or len(c) != 3 * n or len(x) % 3:
            raise ValueError("rot is (n, 3, 3), trans and centres (n, 3), xyz (m, 3), obs_offset n + 1 entries")
        self._check(self.lib.apd_prep_set_model(self.ctx, n, r.ctypes.data, t.ctypes.data, c.ctypes.data, len(x) // 3,
                                                x.ctypes.data if len(x) else None, len(pt), off.ctypes.data,
                                                pt.ctypes.data if len(pt) else None), "apd_prep_set_model")
        self.n_images = n

    def pair_counts(self, q_gate: float, atomics: int = PREP_ATOMICS_DEFAULT):
        """(shared, narrow) uint32 (n, n); self.n_records = the number of pair records."""
        n = self.n_images
        shared = np.empty((max(n, 1), max(n, 1)), np.uint32)
        narrow = np.empty_like(shared)
        rec = C.c_uint64(0)
        self._check(self.lib.apd_prep_pair_counts(self.ctx, q_gate, atomics, shared.ctypes.data, narrow.ctypes.data,
                                                  C.byref(rec)), "apd_prep_pair_counts")
        self.n_records = rec.value
        return shared, narrow

    def depth_ranks(self, fractions):
        """(z_at float64 (n, k), n_obs int64 (n,))"""
        f = np.ascontiguousarray(fractions, np.float64).reshape(-1)
        n = self.n_images
        z = np.zeros((max(n, 1), max(len(f), 1)), np.float64)
        cnt = np.zeros(max(n, 1), np.int64)
        self._check(self.lib.apd_prep_depth_ranks(self.ctx, len(f), f.ctypes.data if len(f) else None, z.ctypes.data,
                                                  cnt.ctypes.data), "apd_prep_depth_ranks")
        return z, cnt

    def timing(self) -> dict:
        a, b, r, c = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.apd_prep_get_timing(self.ctx, C.byref(a), C.byref(b), C.byref(r), C.byref(c)),
                    "apd_prep_get_timing")
        return {"tracks_ms": a.value, "pairs_ms": b.value, "records_ms": r.value, "ranks_ms": c.value}

    def undistort(self, bgr, model, params, out_K=None, out_size=None) -> np.ndarray:
        """apd_prep_undistort_bgr8: bgr (h, w, 3) uint8 taken with camera `model` (name or COLMAP id) and
        `params` -> the (out_h, out_w, 3) image of the pinhole camera out_K = [fx, fy, cx, cy] (default: the
        source camera's) of out_size = (w, h) (default: the source's). Needs no model."""
        src, p, K, ow, oh = _undistort_args(bgr, model, params, out_K, out_size)
        dst = np.empty((max(oh, 0), max(ow, 0), 3), np.uint8)
        self._check(self.lib.apd_prep_undistort_bgr8(self.ctx, prep_model_id(model), p.ctypes.data, len(p), src.shape[1],
                                                     src.shape[0], src.ctypes.data, K.ctypes.data, ow, oh,
                                                     dst.ctypes.data), "apd_prep_undistort_bgr8")
        return dst

    def undistort_timing(self) -> dict:
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._check(self.lib.apd_prep_get_undistort_timing(self.ctx, C.byref(a), C.byref(b), C.byref(c)),
                    "apd_prep_get_undistort_timing")
        return {"upload_ms": a.value, "kernel_ms": b.value, "download_ms": c.value}

def seg_threshold_q8(threshold: float) -> int:
    """A threshold in grey levels -> include/apd_seg.h's units of 1/256 level."""
    return int(round(256 * threshold))


def seg_working_size(w: int, h: int, max_size: int = 2560, lib: Optional[C.CDLL] = None):
    """apd_seg_working_size: (s, W, H) of the contract's stage 1."""
    s, W, H = C.c_int32(), C.c_int32(), C.c_int32()
    st = (lib or load_library()).apd_seg_working_size(w, h, max_size, C.byref(s), C.byref(W), C.byref(H))
    if st != 0:
        raise ApdError(f"apd_seg_working_size -> {STATUS.get(st, st)}")
    return s.value, W.value, H.value


def seg_label_colour(k: int, lib: Optional[C.CDLL] = None):
    """apd_seg_label_colour: (B, G, R) of label k in apd_segment's picture."""
    bgr = (C.c_uint8 * 3)()
    (lib or load_library()).apd_seg_label_colour(k, bgr)
    return tuple(bgr)


def _seg_image(bgr):
    """(h, w, 3) uint8, numpy or torch (kept where it is), contiguous"""
    src = _keep(bgr, np.uint8)
    if src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("bgr is (h, w, 3) uint8")
    return src


def seg_flat_zones_host(bgr, max_size: int = 2560, threshold: float = 1.0, min_area: int = 256, stages: bool = False,
                        lib: Optional[C.CDLL] = None):
    """apd_seg_flat_zones_bgr8_host: the five stages of include/apd_seg.h on the CPU. bgr (h, w, 3) uint8 ->
    (labels (H, W) uint8, n_survivors, n_labels); with stages=True a fourth entry, the dict of work (H, W, 3)
    uint8, smooth (3, H, W) uint16, flat (H, W) uint8, roots and areas (H, W) int32."""
    lib = lib or load_library()
    src = np.ascontiguousarray(_seg_image(bgr))
    h, w = src.shape[:2]
    _, W, H = seg_working_size(w, h, max_size, lib)
    labels = np.empty((H, W), np.uint8)
    st_arrays = {"work": np.empty((H, W, 3), np.uint8), "smooth": np.empty((3, H, W), np.uint16),
                 "flat": np.empty((H, W), np.uint8), "roots": np.empty((H, W), np.int32),
                 "areas": np.empty((H, W), np.int32)} if stages else {}
    ow, oh, ns, nl = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    st = lib.apd_seg_flat_zones_bgr8_host(w, h, src.ctypes.data, max_size, seg_threshold_q8(threshold), min_area,
                                          labels.ctypes.data, C.byref(ow), C.byref(oh), C.byref(ns), C.byref(nl),
                                          *[st_arrays[k].ctypes.data if stages else None for k in SEG_STAGES])
    if st != 0:
        raise ApdError(f"apd_seg_flat_zones_bgr8_host -> {STATUS.get(st, st)}")
    assert (ow.value, oh.value) == (W, H)
    return (labels, ns.value, nl.value, st_arrays) if stages else (labels, ns.value, nl.value)


def seg_label_mask_host(mask, lib: Optional[C.CDLL] = None) -> np.ndarray:
    """apd_seg_label_mask_host: (H, W) mask, non-zero = set -> (H, W) int32 roots (the smallest linear index
    of the pixel's 4-connected component), -1 where the mask is 0."""
    m = np.ascontiguousarray(mask, np.uint8)
    if m.ndim != 2:
        raise ValueError("mask is (H, W)")
    roots = np.empty(m.shape, np.int32)
    st = (lib or load_library()).apd_seg_label_mask_host(m.shape[1], m.shape[0], m.ctypes.data, roots.ctypes.data)
    if st != 0:
        raise ApdError(f"apd_seg_label_mask_host -> {STATUS.get(st, st)}")
    return roots


class SegEngine(_Context):
    """One apd_seg_ctx (include/apd_seg.h): flat-zone sa_masks on the device. Images and masks are numpy
    arrays or torch tensors; a CUDA tensor is read in place and answered with CUDA tensors."""

    PREFIX = "apd_seg"
    shape = None  # (H, W) of the last call

    @staticmethod
    def _empty(like, shape, dtype):
        if hasattr(like, "is_cuda") and like.is_cuda:
            import torch
            return torch.empty(shape, dtype=getattr(torch, _TORCH_DTYPES[np.dtype(dtype)]), device=like.device)
        return np.empty(shape, dtype)

    def flat_zones(self, bgr, max_size: int = 2560, threshold: float = 1.0, min_area: int = 256):
        """apd_seg_flat_zones_bgr8: bgr (h, w, 3) uint8 -> (labels (H, W) uint8, n_survivors, n_labels)."""
        src = _seg_image(bgr)
        h, w = int(src.shape[0]), int(src.shape[1])
        _, W, H = seg_working_size(w, h, max_size, self.lib)
        labels = self._empty(src, (H, W), np.uint8)
        _torch_device_sync(src, labels)
        ow, oh, ns, nl = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.apd_seg_flat_zones_bgr8(self.ctx, w, h, _ptr(src, C.c_uint8), max_size,
                                                     seg_threshold_q8(threshold), min_area, _ptr(labels, C.c_uint8),
                                                     C.byref(ow), C.byref(oh), C.byref(ns), C.byref(nl)),
                    "apd_seg_flat_zones_bgr8")
        self.shape = (oh.value, ow.value)
        return labels, ns.value, nl.value

    def label_mask(self, mask):
        """apd_seg_label_mask: (H, W) mask, non-zero = set -> (H, W) int32 roots, -1 where the mask is 0."""
        m = _keep(mask, np.uint8)
        if m.ndim != 2:
            raise ValueError("mask is (H, W)")
        H, W = int(m.shape[0]), int(m.shape[1])
        roots = self._empty(m, (H, W), np.int32)
        _torch_device_sync(m, roots)
        self._check(self.lib.apd_seg_label_mask(self.ctx, W, H, _ptr(m, C.c_uint8), _ptr(roots, C.c_int32)),
                    "apd_seg_label_mask")
        self.shape = (H, W)
        return roots

    def stage(self, name: str) -> np.ndarray:
        """apd_seg_get_stage of the last call: "work", "smooth", "flat", "roots" or "areas" as numpy."""
        if name not in SEG_STAGES:
            raise ValueError(f"stage is one of {list(SEG_STAGES)}")
        H, W = self.shape or (1, 1)
        shape, dtype = {"work": ((H, W, 3), np.uint8), "smooth": ((3, H, W), np.uint16), "flat": ((H, W), np.uint8),
                        "roots": ((H, W), np.int32), "areas": ((H, W), np.int32)}[name]
        out = np.empty(shape, dtype)
        self._check(self.lib.apd_seg_get_stage(self.ctx, SEG_STAGES[name], out.ctypes.data), "apd_seg_get_stage")
        return out

    def timing(self) -> dict:
        ms = (C.c_double * len(SEG_TIMES))()
        self._check(self.lib.apd_seg_get_timing(self.ctx, ms), "apd_seg_get_timing")
        return dict(zip(SEG_TIMES, [float(v) for v in ms]))

def prep_rotation(qvec) -> np.ndarray:
    """(n, 4) quaternions (w, x, y, z), not normalised -> (n, 3, 3) R by include/apd_prep.h's formula."""
    q = np.asarray(qvec, np.float64).reshape(-1, 4)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3), np.float64)
    R[:, 0, 0] = (1 - 2 * (y * y)) - 2 * (z * z)
    R[:, 0, 1] = (2 * x) * y - (2 * w) * z
    R[:, 0, 2] = (2 * z) * x + (2 * w) * y
    R[:, 1, 0] = (2 * x) * y + (2 * w) * z
    R[:, 1, 1] = (1 - 2 * (x * x)) - 2 * (z * z)
    R[:, 1, 2] = (2 * y) * z - (2 * w) * x
    R[:, 2, 0] = (2 * z) * x - (2 * w) * y
    R[:, 2, 1] = (2 * y) * z + (2 * w) * x
    R[:, 2, 2] = (1 - 2 * (x * x)) - 2 * (y * y)
    return R


def prep_model_arrays(images, point_ids, xyz) -> dict:
    """COLMAP-style model -> the arrays of apd_prep_set_model. images: dicts with id, qvec (w, x, y, z),
    tvec and point_ids (the 2D points' int64 point ids, -1 = none), in any order; point_ids / xyz: the
    3D points' ids and (m, 3) positions. Images are renumbered in ascending id. A point id an image
    names that is not among point_ids is an error."""
    order = sorted(range(len(images)), key=lambda i: int(images[i]["id"]))
    if len({int(im["id"]) for im in images}) != len(images):
        raise ValueError("duplicate image id")
    pid = np.asarray(point_ids, np.int64).reshape(-1)
    srt = np.argsort(pid, kind="stable")
    spid = pid[srt]
    if len(spid) > 1 and np.any(spid[1:] == spid[:-1]):
        raise ValueError("duplicate point id")
    q = np.array([images[i]["qvec"] for i in order], np.float64).reshape(-1, 4)
    t = np.array([images[i]["tvec"] for i in order], np.float64).reshape(-1, 3)
    R = prep_rotation(q)
    c = np.stack([-((R[:, 0, k] * t[:, 0] + R[:, 1, k] * t[:, 1]) + R[:, 2, k] * t[:, 2]) for k in range(3)], 1)
    off = [0]
    obs = []
    for i in order:
        ids = np.asarray(images[i]["point_ids"], np.int64).reshape(-1)
        ids = ids[ids != -1]
        pos = np.searchsorted(spid, ids)
        bad = (pos >= len(spid)) | (spid[np.minimum(pos, max(len(spid) - 1, 0))] != ids) if len(spid) else ids == ids
        if np.any(bad):
            raise ValueError(f"image {int(images[i]['id'])} names point {int(ids[bad][0])}, which points3D lacks")
        obs.append(srt[pos].astype(np.int32))
        off.append(off[-1] + len(ids))
    return {"ids": [int(images[i]["id"]) for i in order], "rot": R, "trans": t, "centres": c,
            "xyz": np.asarray(xyz, np.float64).reshape(-1, 3), "obs_offset": np.asarray(off, np.int64),
            "obs_point": np.concatenate(obs) if obs else np.zeros(0, np.int32)}


def prep_score(shared, narrow) -> np.ndarray:
    """score = shared, 0 where narrow >= floor(3*shared/4) + 1 (include/apd_prep.h)."""
    s = np.asarray(shared, np.int64)
    return np.where(np.asarray(narrow, np.int64) >= (3 * s) // 4 + 1, 0, s)


def prep_select(score, max_views: int = 20):
    """Per view i the first min(max_views, n-1) of j != i by (score descending, j ascending): lists of (j, score)."""
    n = len(score)
    out = []
    for i in range(n):
        cand = sorted((j for j in range(n) if j != i), key=lambda j: (-int(score[i][j]), j))
        out.append([(j, int(score[i][j])) for j in cand[:min(max_views, n - 1)]])
    return out


def prep_select_sequential(n: int, k: int = 5):
    """The reference's sequential window (tools/colmap2mvsnet.py:453-468)."""
    out = []
    lim = min(n - 1, 2 * k)
    for i in range(n):
        nb = []
        for offset in range(1, k + 1):
            for direction in (-1, 1):
                j = i + direction * offset
                if 0 <= j < n:
                    nb.append((j, k + 1 - offset))
        nb.sort(key=lambda it: (-it[1], abs(it[0] - i)))
        out.append(nb[:lim])
    return out


def prepare_views(images, point_ids, xyz, max_views: int = 20, sequential: bool = False, sequential_k: int = 5,
                  device: int = 0, engine: Optional[PrepEngine] = None) -> dict:
    """The sequence of host/prepare_main.cpp: model arrays, depth ranks (0.01, 0.99) -> depth_min /
    depth_max, and the view selection (pair counts -> score -> selection, or the sequential window)."""
    m = prep_model_arrays(images, point_ids, xyz)
    eng = engine or PrepEngine(device)
    try:
        eng.set_model(m["rot"], m["trans"], m["centres"], m["xyz"], m["obs_offset"], m["obs_point"])
        z, cnt = eng.depth_ranks([0.01, 0.99])
        has = cnt > 0
        out = {"model": m, "n_obs": cnt, "depth_min": np.where(has, z[:, 0] * 0.75, 0.0),
               "depth_max": np.where(has, z[:, 1] * 1.25, 0.0)}
        if sequential:
            out["selection"] = prep_select_sequential(len(m["ids"]), sequential_k)
        else:
            shared, narrow = eng.pair_counts(prep_cos_gate(1.0, eng.lib))
            out.update(shared=shared, narrow=narrow, score=prep_score(shared, narrow))
            out["selection"] = prep_select(out["score"], max_views)
        out["timing"] = eng.timing()
    finally:
        if engine is None:
            eng.close()
    return out


def cloud_metrics(rec_xyz, gt_xyz, tolerances=ETH3D_TOLERANCES, max_dist=None, voxel: float = 0.0,
                  engine: Optional[EvalEngine] = None, gt_cams=None, min_views: int = 1, splat: int = 0,
                  occlusion_tol: float = 0.01) -> dict:
    """Accuracy / completeness / F1 of a reconstructed cloud against a ground-truth cloud (numpy
    (n, 3) float32), the definitions the `apd_eval` command line shares: R and G are the clouds after
    dropping non-finite points and, for voxel > 0, down-sampling each on its own; accuracy =
    #{dist(R_i, G) <= t} / |R|, completeness = #{dist(G_j, R) <= t} / |G|, F1 = 2ac / (a + c), each
    ratio 0 when its denominator is 0. Plain nearest-neighbour distances truncated at max_dist
    (default: the largest tolerance); no free-space or visibility modelling.

    With gt_cams (ApdCamera structures or dicts of their values) completeness is measured over G',
    the points of G that pass a z-buffer test in at least min_views of those cameras: G itself is
    rendered into every camera (footprint `splat`), and a point is seen in a view when it projects
    into the image no deeper than (1 + occlusion_tol) times the rendered depth there. Accuracy is
    still measured against all of G: a reconstructed point near an unseen part of the scan is not an
    error. gt["points_visible"] = |G'|. A z-buffer test, not the ETH3D tool's free-space model."""
    if gt_cams is not None and min_views < 1:
        raise ValueError("min_views must be at least 1")
    tol = np.ascontiguousarray(tolerances, np.float32).reshape(-1)
    md = float(tol.max()) if max_dist is None else float(np.float32(max_dist))
    eng = engine or EvalEngine()
    out = {"tolerances": [float(t) for t in tol], "max_dist": md, "voxel": float(np.float32(voxel)), "timing_ms": {}}
    try:
        clouds = {}
        for name, xyz in (("rec", rec_xyz), ("gt", gt_xyz)):
            a = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
            info = {"points_in": int(len(a))}
            a = a[np.isfinite(a).all(axis=1)]
            info["points_finite"] = int(len(a))
            if voxel > 0:
                a = np.ascontiguousarray(a[eng.voxel_downsample(a, voxel)])
            info["points"] = int(len(a))
            clouds[name] = a
            out[name] = info
        if gt_cams is not None:
            g = clouds["gt"]
            seen = eng.visibility(g, gt_cams, eng.render_depth(g, gt_cams, splat), occlusion_tol)
            tr = eng.render_timing()
            clouds["gt_visible"] = np.ascontiguousarray(g[seen >= min_views])
            out["gt"]["points_visible"] = int(len(clouds["gt_visible"]))
            out["visibility"] = {"views": len(gt_cams), "min_views": int(min_views), "splat": int(splat),
                                 "occlusion_tol": float(np.float32(occlusion_tol))}
            out["timing_ms"]["visibility"] = tr
        else:
            clouds["gt_visible"] = clouds["gt"]
        ratios = {}
        for name, q, t in (("accuracy", "rec", "gt"), ("completeness", "gt_visible", "rec")):
            eng.set_target(clouds[t])
            dist, within = eng.distances(clouds[q], md, tol)
            tm = eng.timing()
            fin = np.isfinite(dist)
            nfin = int(fin.sum())
            n = len(dist)
            mean = float(np.cumsum(dist[fin].astype(np.float64))[-1] / nfin) if nfin else 0.0  # index order
            ratios[name] = [int(w) / n if n else 0.0 for w in within]
            out[name] = {"within": [int(w) for w in within], "inf": n - nfin, "mean": mean, "ratio": ratios[name]}
            out["timing_ms"][name] = {"build_ms": tm["build_ms"], "query_ms": tm["query_ms"]}
        out["f1"] = [2 * a * c / (a + c) if a + c > 0 else 0.0
                     for a, c in zip(ratios["accuracy"], ratios["completeness"])]
    finally:
        if engine is None:
            eng.close()
    return out


def cloud_metrics_scanners(rec_xyz, scans, tolerances=ETH3D_TOLERANCES, voxel: float = 0.01, cube_size: int = 2048,
                           splat: int = 1, max_dist=None, engine: Optional[EvalEngine] = None) -> dict:
    """Accuracy / completeness / F1 of a reconstructed cloud against laser scans with a scanner
    free-space model and voxel-averaged scores, the `apd_eval --gt_mlp` mode's sequence of calls.
    scans: a list of (points (n, 3) float32 in world coordinates, origin (3,)) per scanner position.

    R = the finite points of rec_xyz, G = the finite points of all scans in order. No cloud is
    down-sampled; `voxel` is the scoring voxel. Per tolerance t:
      accuracy: a point of R is good iff dist(R_i, G) <= t; bad iff it is not good and lies more
        than t in front of the surface some scanner saw along its ray (free_gap > t, the gap taken
        against the cube-map z-buffers of every scanner, each rendered from that scanner's own
        points with footprint `splat`); otherwise it is unobserved (behind the scanned surface, or
        where no beam went) and does not count.
      completeness: a point of G is good iff dist(G_j, R) <= t, else bad.
      Each score is the mean over the voxels with a counted point of good / (good + bad), as the
      fixed-point integers of include/apd_eval.h; F1 = 2ac / (a + c), 0 when a + c = 0.
    Distances are truncated at max_dist (default: the largest tolerance).

    Modelled on the ETH3D evaluation protocol but not the ETH3D tool: a z-buffer per cube-map pixel
    instead of per-beam cones, a free-space margin equal to the tolerance, integer-rounded voxel
    ratios. Parity with that tool is not pinned; the numbers are not for published tables."""
    tol = np.ascontiguousarray(tolerances, np.float32).reshape(-1)
    md = float(tol.max()) if max_dist is None else float(np.float32(max_dist))
    eng = engine or EvalEngine()

    def finite(x):
        a = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
        return np.ascontiguousarray(a[np.isfinite(a).all(axis=1)])

    out = {"tolerances": [float(t) for t in tol], "max_dist": md, "voxel": float(np.float32(voxel)),
           "cube_size": int(cube_size), "splat": int(splat), "timing_ms": {}}
    try:
        R = finite(rec_xyz)
        parts = [finite(p) for p, _ in scans]
        origins = [np.ascontiguousarray(o, np.float32).reshape(3) for _, o in scans]
        G = np.ascontiguousarray(np.concatenate(parts + [np.zeros((0, 3), np.float32)]))
        out["rec"] = {"points": int(len(R))}
        out["gt"] = {"points": int(len(G))}
        out["scanners"] = [{"points": int(len(p)), "origin": [float(v) for v in o]} for p, o in zip(parts, origins)]

        def side(name, q, t, gap):
            eng.set_target(t)
            dist, _ = eng.distances(q, md)
            tm = eng.timing()
            sc = eng.voxel_scores(q, voxel, dist, gap, tol)
            good = [int(v) for v in sc["good"]]
            bad = [int(v) for v in sc["bad"]]
            out[name] = {"points": int(len(q)), "good": good, "bad": bad,
                         "unobserved": [len(q) - g - b for g, b in zip(good, bad)],
                         "ratio_sum": [int(v) for v in sc["ratio_sum"]], "voxels": [int(v) for v in sc["voxels"]],
                         "score": sc["score"], "plain_of_all": [g / len(q) if len(q) else 0.0 for g in good],
                         "plain": [g / (g + b) if g + b else 0.0 for g, b in zip(good, bad)]}
            out["timing_ms"][name] = {"build_ms": tm["build_ms"], "query_ms": tm["query_ms"],
                                      "scores_ms": eng.protocol_timing()["scores_ms"]}
            return dist

        gap = np.full(len(R), -np.inf, np.float32)
        render_ms = gap_ms = 0.0
        for p, o in zip(parts, origins):  # one scanner's six maps at a time
            cams = cube_cameras(o, cube_size, eng.lib)
            maps = eng.render_depth(p, cams, splat)
            render_ms += eng.render_timing()["render_ms"]
            gap = np.maximum(gap, eng.free_gap(R, cams, maps))
            gap_ms += eng.protocol_timing()["free_gap_ms"]
        out["timing_ms"]["free_space"] = {"render_ms": render_ms, "free_gap_ms": gap_ms}
        out["accuracy_dist"] = side("accuracy", R, G, gap)
        out["accuracy_gap"] = gap
        out["completeness_dist"] = side("completeness", G, R, None)
        out["f1"] = [2 * a * c / (a + c) if a + c > 0 else 0.0
                     for a, c in zip(out["accuracy"]["score"], out["completeness"]["score"])]
    finally:
        if engine is None:
            eng.close()
    return out


def cloud_metrics_dtu(rec_xyz, gt_xyz, mask, bb, res: float, plane, density: float = 0.2, max_dist: float = 20.0,
                      seed: int = 0, thin: bool = True, engine: Optional[EvalEngine] = None) -> dict:
    """Accuracy and completeness of a reconstructed cloud under the DTU protocol, the `apd_eval --dtu_gt`
    mode's sequence of calls. mask: the 3-D observability volume (ObsMask), bb: its bounding box (2, 3)
    with the minimum in row 0 (BB), res: its cell size (Res), plane: the table plane (P, 4 values).

    1. Unless thin is False the reconstruction is thinned to a minimum spacing of `density`: in ascending
       (Philox rank drawn from `seed`, index) a point is kept iff no point kept before it lies within
       `density` (EvalEngine.radius_thin; exact, the order is the only random element).
    2. Distances thinned reconstruction -> ground truth and back, truncated at max_dist.
    3. Accuracy: the thinned points whose cell round((p - bb[0]) / res + 1) lies in the mask and is set;
       completeness: the ground-truth points with [p 1] . plane > 0. Both take the distances
       <= nextafter(max_dist, 0) (MATLAB's strict <) and give their mean and median.

    Modelled on the DTU MATLAB evaluation, not that code: a seeded order instead of randperm (reproducible,
    but not MATLAB's numbers for any seed), doubles for the mask index, no chunks. Parity is not pinned."""
    eng = engine or EvalEngine()
    out = {"density": float(np.float32(density)), "max_dist": float(np.float32(max_dist)), "seed": int(seed),
           "thinned": bool(thin), "timing_ms": {}}
    try:
        rec = np.ascontiguousarray(rec_xyz, np.float32).reshape(-1, 3)
        gt = np.ascontiguousarray(gt_xyz, np.float32).reshape(-1, 3)
        box = np.ascontiguousarray(bb, np.float64).reshape(2, 3)
        if thin:
            keep = eng.radius_thin(rec, density, dtu_ranks(len(rec), seed, eng.lib))
            out["timing_ms"]["thin"] = eng.thin_timing()
            data = np.ascontiguousarray(rec[keep])
        else:
            keep, data = np.arange(len(rec), dtype=np.int32), rec
        limit = float(np.nextafter(np.float32(max_dist), np.float32(0)))
        eng.set_target(gt)
        d_acc, _ = eng.distances(data, max_dist)
        eng.set_target(data)
        d_comp, _ = eng.distances(gt, max_dist)
        inside = eng.obs_mask(data, mask, box[0], res)
        above = eng.half_space(gt, plane)
        sa, sc = eng.masked_stats(d_acc, inside, limit), eng.masked_stats(d_comp, above, limit)
        out["timing_ms"]["dtu"] = eng.dtu_timing()
        out.update({"input_points": int(len(rec)), "thinned_points": int(len(data)),
                    "in_mask_points": int(inside.sum()), "gt_points": int(len(gt)),
                    "gt_above_plane_points": int(above.sum()), "accuracy_selected": sa["count"],
                    "completeness_selected": sc["count"],
                    "accuracy_mean": sa["sum"] / sa["count"] if sa["count"] else 0.0, "accuracy_median": sa["median"],
                    "completeness_mean": sc["sum"] / sc["count"] if sc["count"] else 0.0,
                    "completeness_median": sc["median"], "keep_idx": keep, "accuracy_dist": d_acc,
                    "completeness_dist": d_comp, "inside": inside, "above": above})
        out["overall"] = (out["accuracy_mean"] + out["completeness_mean"]) / 2.0
    finally:
        if engine is None:
            eng.close()
    return out


class Engine(_Context):
    """One apd_ctx on one HIP device."""

    PREFIX = "apd"

    def set_problem(self, arrays: ProblemArrays):
        pb = arrays.build()
        self._arrays = arrays
        # device-resident inputs (scan_runner.py) may be fresh outputs of torch / RCCL kernels
        _torch_device_sync(arrays._imgs, getattr(arrays, "_deps", None), arrays._planes, arrays._weak,
                           arrays._conf, arrays._sa)
        self._check(self.lib.apd_set_problem(self.ctx, C.byref(pb)), "apd_set_problem")

    def run(self):
        self._check(self.lib.apd_run_patchmatch(self.ctx), "apd_run_patchmatch")

    def prepare(self):
        self._check(self.lib.apd_stage_prepare(self.ctx), "apd_stage_prepare")

    def iteration(self, i: int):
        self._check(self.lib.apd_stage_iteration(self.ctx, i), "apd_stage_iteration")

    def finish(self):
        self._check(self.lib.apd_stage_finish(self.ctx), "apd_stage_finish")

    def synchronize(self):
        self._check(self.lib.apd_synchronize(self.ctx), "apd_synchronize")

    def results(self, out: Outputs):
        s = out.struct()
        self._check(self.lib.apd_get_results(self.ctx, C.byref(s)), "apd_get_results")
        return out

    def results_device(self, width: int, height: int, device: str):
        """planes / weak_info / confidence as torch tensors on `device` (the ctx's device), copied
        device to device by apd_get_results."""
        import torch
        from types import SimpleNamespace
        o = SimpleNamespace(planes=torch.empty((height, width, 4), dtype=torch.float32, device=device),
                            weak_info=torch.empty((height, width), dtype=torch.uint8, device=device),
                            confidence=torch.empty((height, width), dtype=torch.uint8, device=device))
        s = ApdOutputs()
        s.planes = _ptr(o.planes, C.c_float)
        s.weak_info = _ptr(o.weak_info, C.c_uint8)
        s.confidence = _ptr(o.confidence, C.c_uint8)
        _torch_device_sync(o.planes)
        self._check(self.lib.apd_get_results(self.ctx, C.byref(s)), "apd_get_results")
        return o

    def resize_nearest_device(self, src, dw: int, dh: int):
        """apd_device_resize_nearest of a contiguous (H, W[, C]) torch tensor on the ctx's device."""
        import torch
        src = src.contiguous()
        sh, sw = src.shape[:2]
        dst = torch.empty((dh, dw) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
        elem = src.element_size() * (src[0, 0].numel() if src.dim() > 2 else 1)
        _torch_device_sync(src, dst)
        self._check(self.lib.apd_device_resize_nearest(self.ctx, src.data_ptr(), sw, sh, dst.data_ptr(), dw, dh, elem),
                    "apd_device_resize_nearest")
        return dst

    def result_device(self, width: int, height: int, device: str):
        """apd_result_device: (depth (H, W), planes (H, W, 4)) of the last run, epilogue applied, on `device`."""
        import torch
        depth = torch.empty((height, width), dtype=torch.float32, device=device)
        planes = torch.empty((height, width, 4), dtype=torch.float32, device=device)
        _torch_device_sync(depth, planes)
        self._check(self.lib.apd_result_device(self.ctx, depth.data_ptr(), planes.data_ptr()), "apd_result_device")
        return depth, planes

    def timing(self) -> ApdTiming:
        t = ApdTiming()
        self._check(self.lib.apd_get_timing(self.ctx, C.byref(t)), "apd_get_timing")
        return t

    def prepare_timing(self) -> ApdTiming:
        """The prepare-phase fields of the last apd_stage_prepare (waits for the ctx stream)."""
        t = ApdTiming()
        self._check(self.lib.apd_get_prepare_timing(self.ctx, C.byref(t)), "apd_get_prepare_timing")
        return t

    def profile_reset(self, enable: bool = True):
        self._check(self.lib.apd_profile_reset(self.ctx, int(enable)), "apd_profile_reset")

    def profile_query(self):
        ms, n, px = C.c_double(), C.c_int64(), C.c_int64()
        self._check(self.lib.apd_profile_query(self.ctx, C.byref(ms), C.byref(n), C.byref(px)), "apd_profile_query")
        return ms.value, n.value, px.value

    def profile_kernel(self, kind: int):
        """(total ms, launches, pixels) of the profiled launches of one APD_PROF_* kind."""
        ms, n, px = C.c_double(), C.c_int64(), C.c_int64()
        self._check(self.lib.apd_profile_kernel(self.ctx, kind, C.byref(ms), C.byref(n), C.byref(px)),
                    "apd_profile_kernel")
        return ms.value, n.value, px.value

    def profile_counters(self):
        c = (C.c_int64 * PROF_COUNTERS)()
        self._check(self.lib.apd_profile_counters(self.ctx, c, PROF_COUNTERS), "apd_profile_counters")
        return list(c)

    def profile_evaluations(self) -> int:
        n = C.c_int64()
        self._check(self.lib.apd_profile_evaluations(self.ctx, C.byref(n)), "apd_profile_evaluations")
        return n.value

    def device_bytes(self) -> int:
        """Bytes of device memory the context's buffers hold."""
        n = C.c_size_t()
        self._check(self.lib.apd_device_bytes(self.ctx, C.byref(n)), "apd_device_bytes")
        return n.value


def scene_problem(scene, ref: int = 0, srcs: Optional[Sequence[int]] = None, params: Optional[ApdParams] = None,
                  seed: int = 0x5EED, **kw) -> ProblemArrays:
    """ProblemArrays for one reference view of a synth.Scene (full resolution, FIRST_INIT defaults)."""
    from importlib import import_module
    synth = import_module("synth")
    if srcs is None:
        srcs = [j for j, _ in scene.pairs[ref]]
    ids = [ref] + list(srcs)
    cams = [synth.camera_struct_values(scene.cameras[i], scene.width, scene.height) for i in ids]
    c0 = scene.cameras[ref]
    if params is None:
        params = default_params(len(ids), float(np.float32(c0.depth_min) * np.float32(0.6)),
                                float(np.float32(c0.depth_max) * np.float32(1.2)))
    return ProblemArrays(scene.width, scene.height, [scene.images[i] for i in ids], cams, params, seed=seed, **kw)
