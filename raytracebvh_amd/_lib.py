"""ctypes binding of librtbvh.so (the C ABI in include/rtbvh.h).

The product path is the HIP library; there is no CPU fallback.  If the shared
library has not been built this module raises at import time.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# RTBVH_LIB: an A/B build of the same library (raytracebvh_amd/csrc/Makefile OUT=...)
LIB_PATH = os.environ.get("RTBVH_LIB") or os.path.join(HERE, "librtbvh.so")

OK, ERR_INVALID_ARG, ERR_HIP, ERR_OOM, ERR_NOT_READY, ERR_STACK_OVERFLOW, ERR_IO, ERR_NO_DEVICE = range(8)
MORTON_CPUTESTS, MORTON_HLSL = 0, 1
DELTA_CLZ64, DELTA_CPUTESTS = 0, 1
FLAG_TIMING, FLAG_COUNT_VISITS, FLAG_REFRACT_RECORDS, FLAG_SORT_BOUNCE, FLAG_NEAREST_FIRST = 1, 2, 4, 8, 16
FLAG_PACKET_PRIMARY = 1 << 5
FLAG_REFILL_BOUNCE = 1 << 6
FLAG_WIDE_BVH = 1 << 7
FLAG_BINNED_PRIMARY = 1 << 9   # primary rays by screen-tile bins of the leaves (include/rtbvh.h)
FLAG_CERTIFIED = 1 << 10   # the certified fast walks whatever the size (include/rtbvh.h)
FLAG_MULTI_KERNEL_BUILD = 1 << 16
FLAG_AUTO_WALK = 1 << 8   # walks chosen by scene size (include/rtbvh.h)
FLAG_SPLIT_SHIFT = 17   # trace chains: (n << FLAG_SPLIT_SHIFT), 0 = automatic
FLAG_GRAPH = 1 << 20    # compute_bvh replays a captured hipGraph of the frame

# every symbol include/rtbvh.h declares (tests check the library exports them all)
EXPORTS = [
    "rtbvh_config_default", "rtbvh_create", "rtbvh_destroy", "rtbvh_last_error", "rtbvh_abi_version", "rtbvh_stats_size",
    "rtbvh_set_scene", "rtbvh_set_camera", "rtbvh_build", "rtbvh_build_async", "rtbvh_trace",
    "rtbvh_trace_async", "rtbvh_compute_bvh", "rtbvh_trace_band_async", "rtbvh_band_rows", "rtbvh_verify_walk",
    "rtbvh_deal_bands", "rtbvh_deal_rows", "rtbvh_set_band_deal",
    "rtbvh_synchronize", "rtbvh_read_framebuffer", "rtbvh_read_intensity", "rtbvh_framebuffer_device",
    "rtbvh_read_bvh", "rtbvh_read_wide", "rtbvh_read_qnodes", "rtbvh_read_walk_qnodes", "rtbvh_read_morton", "rtbvh_read_sorted", "rtbvh_read_rays", "rtbvh_get_stats",
    "rtbvh_reset_stats", "rtbvh_set_flags", "rtbvh_bin_builds", "rtbvh_bin_sets",
    "rtbvh_sort_pairs_async", "rtbvh_sort_pairs_host", "rtbvh_build_from_codes", "rtbvh_scene_load_obj",
    "rtbvh_scene_synthetic", "rtbvh_scene_free", "rtbvh_scene_num_vertices", "rtbvh_scene_num_indices",
    "rtbvh_scene_num_materials", "rtbvh_scene_num_textures", "rtbvh_scene_vertices", "rtbvh_scene_indices",
    "rtbvh_scene_mat_indices", "rtbvh_scene_materials", "rtbvh_scene_texture_path", "rtbvh_set_scene_obj",
    "rtbvh_camera_reference", "rtbvh_camera_look", "rtbvh_camera_orbit", "rtbvh_texture_load_bmp", "rtbvh_texture_load_jpeg", "rtbvh_texture_decode_jpeg",
    "rtbvh_texture_load", "rtbvh_texture_free", "rtbvh_srgb_table",
    "rtbvh_present", "rtbvh_save_bmp", "rtbvh_assemble_bands", "rtbvh_comm_unique_id", "rtbvh_comm_init",
    "rtbvh_comm_destroy", "rtbvh_trace_tiles",
    "rtbvh_query_async", "rtbvh_query_host", "rtbvh_query_counts", "rtbvh_query_walk_counts",
    "rtbvh_nearest_async", "rtbvh_nearest_host", "rtbvh_nearest_counts",
    "rtbvh_within_async", "rtbvh_within_host", "rtbvh_within_counts",
    "rtbvh_knn_async", "rtbvh_knn_host", "rtbvh_knn_counts",
    "rtbvh_allhits_async", "rtbvh_allhits_host", "rtbvh_allhits_counts",
    "rtbvh_overlap_async", "rtbvh_overlap_host", "rtbvh_overlap_counts",
    "rtbvh_signed_async", "rtbvh_signed_host", "rtbvh_signed_counts",
    "rtbvh_khits_async", "rtbvh_khits_host", "rtbvh_khits_counts",
    "rtbvh_collide_async", "rtbvh_collide_host", "rtbvh_collide_counts",
    "rtbvh_cross_async", "rtbvh_cross_host", "rtbvh_cross_first_async", "rtbvh_cross_first_host", "rtbvh_cross_counts",
    "rtbvh_clearance_async", "rtbvh_clearance_host", "rtbvh_clearance_counts",
    "rtbvh_region_async", "rtbvh_region_host", "rtbvh_region_counts", "rtbvh_region_split_counts",
    "rtbvh_sweep_async", "rtbvh_sweep_host", "rtbvh_sweep_counts",
    "rtbvh_update_vertices_async", "rtbvh_update_vertices_host", "rtbvh_refit_async", "rtbvh_refit",
]
COMM_ID_BYTES = 128

NODE_DTYPE = np.dtype([("parent", "<u4"), ("child_l", "<u4"), ("child_r", "<u4"), ("code", "<u4"),
                       ("bb_min", "<f4", (3,)), ("bb_max", "<f4", (3,)), ("index", "<u4")])
MATERIAL_DTYPE = np.dtype([("ambient", "<f4", (4,)), ("diffuse", "<f4", (4,)), ("specular", "<f4", (4,)),
                           ("shininess", "<f4"), ("optical_density", "<f4"), ("alpha", "<f4"),
                           ("specularb", "<u4"), ("tex_num", "<i4")])
assert NODE_DTYPE.itemsize == 44 and MATERIAL_DTYPE.itemsize == 68
# rtbvh_ray (32 B) and rtbvh_hit (16 B), include/rtbvh.h; a miss: t = -1, u = v = 0, tri = 0xFFFFFFFF
RAY_DTYPE = np.dtype([("origin", "<f4", (3,)), ("t_max", "<f4"), ("direction", "<f4", (3,)), ("reserved", "<u4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<u4")])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 16
QUERY_CLOSEST, QUERY_ANY, QUERY_SORT, QUERY_COUNT = 0, 1, 2, 4   # RTBVH_QUERY_*
QUERY_CERTIFIED = 1 << 8
# rtbvh_point (16 B) and rtbvh_nearest (32 B), include/rtbvh.h; no result: dist2 = -1, point = u = v = 0,
# tri = 0xFFFFFFFF
POINT_DTYPE = np.dtype([("point", "<f4", (3,)), ("max_dist2", "<f4")])
NEAREST_DTYPE = np.dtype([("point", "<f4", (3,)), ("dist2", "<f4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<u4"),
                          ("reserved", "<u4")])
assert POINT_DTYPE.itemsize == 16 and NEAREST_DTYPE.itemsize == 32
NEAREST_SORT, NEAREST_COUNT = 2, 4   # RTBVH_NEAREST_*
# rtbvh_pair (8 B): one entry of a radius query's lists
PAIR_DTYPE = np.dtype([("tri", "<u4"), ("dist2", "<f4")])
assert PAIR_DTYPE.itemsize == 8
WITHIN_SORT, WITHIN_COUNT, WITHIN_SIZES, WITHIN_FILL = 2, 4, 16, 32   # RTBVH_WITHIN_*
KNN_SORT, KNN_COUNT = 2, 4   # RTBVH_KNN_*; its lists are PAIR_DTYPE, a slot past the number found {0xFFFFFFFF, -1}
KNN_MAX_K = 32               # RTBVH_KNN_MAX_K
ALLHITS_SORT, ALLHITS_COUNT, ALLHITS_BY_T, ALLHITS_SIZES, ALLHITS_FILL = 2, 4, 8, 16, 32   # RTBVH_ALLHITS_*
# rtbvh_box (32 B): a box query's axis-aligned box; its lists hold triangle ids (uint32)
BOX_DTYPE = np.dtype([("lo", "<f4", (3,)), ("reserved0", "<u4"), ("hi", "<f4", (3,)), ("reserved1", "<u4")])
assert BOX_DTYPE.itemsize == 32
OVERLAP_SORT, OVERLAP_COUNT, OVERLAP_TRIANGLE, OVERLAP_SIZES, OVERLAP_FILL = 2, 4, 8, 16, 32   # RTBVH_OVERLAP_*
# rtbvh_signed (32 B): NEAREST_DTYPE's fields and the crossing counts (include/rtbvh.h: inside, parities, bytes)
SIGNED_DTYPE = np.dtype([("point", "<f4", (3,)), ("dist2", "<f4"), ("u", "<f4"), ("v", "<f4"), ("tri", "<u4"),
                         ("flags", "<u4")])
assert SIGNED_DTYPE.itemsize == 32
SIGNED_SORT, SIGNED_COUNT, SIGNED_VOTE3, SIGNED_INSIDE_ONLY = 2, 4, 8, 16   # RTBVH_SIGNED_*
KHITS_SORT, KHITS_COUNT = 2, 4   # RTBVH_KHITS_*; its lists are HIT_DTYPE, a slot past the number found a miss
KHITS_MAX_K = 16                 # RTBVH_KHITS_MAX_K
# RTBVH_COLLIDE_*; its lists hold triangle ids (uint32), indexed by triangle
COLLIDE_COUNT, COLLIDE_TRIANGLE, COLLIDE_SIZES, COLLIDE_FILL, COLLIDE_SYMMETRIC = 4, 8, 16, 32, 64
# rtbvh_tri: a query triangle of the triangle queries, three 16-byte words
TRI_DTYPE = np.dtype([("v0", "<f4", (3,)), ("reserved0", "<u4"), ("v1", "<f4", (3,)), ("reserved1", "<u4"),
                      ("v2", "<f4", (3,)), ("reserved2", "<u4")])
assert TRI_DTYPE.itemsize == 48
CROSS_SORT, CROSS_COUNT, CROSS_SIZES, CROSS_FILL = 2, 4, 16, 32   # RTBVH_CROSS_*; its lists hold triangle ids (uint32)
# rtbvh_clearance: the nearest scene triangle to a query triangle and the two witness points
CLEARANCE_DTYPE = np.dtype([("point_q", "<f4", (3,)), ("dist2", "<f4"), ("point_x", "<f4", (3,)), ("tri", "<u4")])
assert CLEARANCE_DTYPE.itemsize == 32
CLEARANCE_SORT, CLEARANCE_COUNT = 2, 4   # RTBVH_CLEARANCE_*
# rtbvh_region (96 B): a region query's up to six planes {nx, ny, nz, d}, inner side n.x + d <= 0, an unused plane
# all zeros; its lists hold triangle ids (uint32)
REGION_DTYPE = np.dtype([("plane", "<f4", (6, 4))])
assert REGION_DTYPE.itemsize == 96
REGION_COUNT, REGION_TRIANGLE, REGION_SIZES, REGION_FILL, REGION_NO_ACCEPT = 4, 8, 16, 32, 64   # RTBVH_REGION_*
# the split field of a region mode (bits 16..19: at most 2^v pieces a region, 15 automatic) and the bound on n * K
REGION_SPLIT_SHIFT, REGION_SPLIT_AUTO, REGION_SPLIT_MAX_PIECES = 16, 15 << 16, 1 << 20
# rtbvh_sweep (32 B: RAY_DTYPE with the radius in the reserved word) and rtbvh_sweep_hit (32 B), include/rtbvh.h; a
# miss: t = -1, point = 0, tri = 0xFFFFFFFF, feature = 0
SWEEP_DTYPE = np.dtype([("origin", "<f4", (3,)), ("t_max", "<f4"), ("direction", "<f4", (3,)), ("radius", "<f4")])
SWEEP_HIT_DTYPE = np.dtype([("t", "<f4"), ("point", "<f4", (3,)), ("tri", "<u4"), ("feature", "<u4"),
                            ("reserved", "<u4", (2,))])
assert SWEEP_DTYPE.itemsize == 32 and SWEEP_HIT_DTYPE.itemsize == 32
SWEEP_ANY, SWEEP_SORT, SWEEP_COUNT = 1, 2, 4   # RTBVH_SWEEP_*


class Config(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("morton_mode", ctypes.c_uint32), ("delta_mode", ctypes.c_uint32),
                ("flags", ctypes.c_uint32), ("scene_bb_min", ctypes.c_float * 3),
                ("scene_bb_max", ctypes.c_float * 3), ("stream", ctypes.c_void_p),
                ("stack_limit", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class Ray(ctypes.Structure):
    """rtbvh_ray (include/rtbvh.h)."""
    _fields_ = [("origin", ctypes.c_float * 3), ("t_max", ctypes.c_float), ("direction", ctypes.c_float * 3),
                ("reserved", ctypes.c_uint32)]


class Hit(ctypes.Structure):
    """rtbvh_hit (include/rtbvh.h)."""
    _fields_ = [("t", ctypes.c_float), ("u", ctypes.c_float), ("v", ctypes.c_float), ("tri", ctypes.c_uint32)]


class Point(ctypes.Structure):
    """rtbvh_point (include/rtbvh.h)."""
    _fields_ = [("point", ctypes.c_float * 3), ("max_dist2", ctypes.c_float)]


class Nearest(ctypes.Structure):
    """rtbvh_nearest (include/rtbvh.h)."""
    _fields_ = [("point", ctypes.c_float * 3), ("dist2", ctypes.c_float), ("u", ctypes.c_float), ("v", ctypes.c_float),
                ("tri", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class Texture(ctypes.Structure):
    """rtbvh_texture: RGBA8 texels, row 0 = texture row v = 0 (include/rtbvh.h)."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("rgba8", ctypes.c_void_p)]


class Stats(ctypes.Structure):
    _fields_ = [("num_tris", ctypes.c_uint32), ("num_nodes", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("primary_rays", ctypes.c_uint64), ("bounce_rays", ctypes.c_uint64),
                ("internal_visits", ctypes.c_uint64 * 2), ("leaf_visits", ctypes.c_uint64 * 2),
                ("hits", ctypes.c_uint64 * 2), ("textured_hits", ctypes.c_uint64),
                ("stack_overflows", ctypes.c_uint64), ("timed_builds", ctypes.c_uint32),
                ("timed_traces", ctypes.c_uint32), ("ms_build", ctypes.c_float), ("ms_trace", ctypes.c_float),
                ("ms_stage", ctypes.c_float * 8), ("trav_wave_steps", ctypes.c_uint64),
                ("trav_mixed_steps", ctypes.c_uint64), ("trav_active_lanes", ctypes.c_uint64),
                ("trav_max_steps", ctypes.c_uint64), ("trav_steps_log2", ctypes.c_uint64 * 32),
                ("graph_captures", ctypes.c_uint64), ("walk_flags", ctypes.c_uint32),
                ("walk_state", ctypes.c_uint32), ("packet_steps", ctypes.c_uint64 * 2),
                ("cert_traces", ctypes.c_uint64), ("redo_total", ctypes.c_uint64),
                ("bin_entries", ctypes.c_uint64 * 2), ("redo_rays", ctypes.c_uint64 * 2),
                ("trav_longest", ctypes.c_uint64), ("redo_deferred", ctypes.c_uint64),
                ("walk_tree_builds", ctypes.c_uint64), ("walk_tree_used", ctypes.c_uint32),
                ("reserved_walk_tree", ctypes.c_uint32)]

    def as_dict(self) -> dict:
        d = {}
        for k, _ in self._fields_:
            v = getattr(self, k)
            d[k] = list(v) if hasattr(v, "__len__") else v
        return d


class RtbvhError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"rtbvh status {status}: {msg}")
        self.status = status


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback for the HIP path)")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (SONAME
    # libamdhip64.so.7, NEEDED by torch as "libamdhip64.so").  Loading torch first
    # makes librtbvh.so's NEEDED libamdhip64.so.7 bind to that same runtime; the
    # other order maps two runtimes and torch then sees no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, u32, u64, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    sig = {
        "rtbvh_config_default": (None, [ctypes.POINTER(Config)]),
        "rtbvh_create": (i32, [ctypes.POINTER(Config), ctypes.POINTER(vp)]),
        "rtbvh_destroy": (None, [vp]),
        "rtbvh_last_error": (ctypes.c_char_p, [vp]),
        "rtbvh_abi_version": (i32, []),
        "rtbvh_stats_size": (ctypes.c_uint32, []),
        "rtbvh_set_scene": (i32, [vp, vp, u32, vp, u32, vp, vp, u32, vp, u32]),
        "rtbvh_set_camera": (i32, [vp, vp, vp]),
        "rtbvh_build": (i32, [vp]),
        "rtbvh_build_async": (i32, [vp]),
        "rtbvh_trace": (i32, [vp, u32, u32, u32]),
        "rtbvh_trace_async": (i32, [vp, u32, u32, u32]),
        "rtbvh_compute_bvh": (i32, [vp, u32, u32, u32]),
        "rtbvh_trace_band_async": (i32, [vp, u32, u32, u32, u32, u32, vp, vp]),
        "rtbvh_band_rows": (u32, [u32, u32, u32]),
        "rtbvh_deal_bands": (u32, [u32, u32, u32, u32, vp, u32]),
        "rtbvh_deal_rows": (u32, [u32, u32, u32, u32]),
        "rtbvh_set_band_deal": (i32, [vp, u32]),
        "rtbvh_verify_walk": (i32, [vp, u32, u32, u32, ctypes.POINTER(u64)]),
        "rtbvh_assemble_bands": (i32, [vp, u32, u32, u32, vp, u32, vp, vp]),
        "rtbvh_comm_unique_id": (i32, [vp]),
        "rtbvh_comm_init": (i32, [vp, u32, u32, vp, ctypes.POINTER(vp)]),
        "rtbvh_comm_destroy": (i32, [vp]),
        "rtbvh_trace_tiles": (i32, [vp, u32, u32, u32, u32, u32, vp]),
        "rtbvh_synchronize": (i32, [vp]),
        "rtbvh_read_framebuffer": (i32, [vp, vp]),
        "rtbvh_read_intensity": (i32, [vp, vp]),
        "rtbvh_framebuffer_device": (vp, [vp]),
        "rtbvh_read_bvh": (i32, [vp, vp, u32]),
        "rtbvh_read_morton": (i32, [vp, vp]),
        "rtbvh_read_wide": (i32, [vp, vp, ctypes.c_uint64]),
        "rtbvh_read_qnodes": (i32, [vp, vp, ctypes.c_uint64]),
        "rtbvh_read_walk_qnodes": (i32, [vp, vp, ctypes.c_uint64]),
        "rtbvh_read_sorted": (i32, [vp, vp, vp]),
        "rtbvh_read_rays": (i32, [vp, vp, vp]),
        "rtbvh_get_stats": (i32, [vp, ctypes.POINTER(Stats)]),
        "rtbvh_reset_stats": (i32, [vp]),
        "rtbvh_set_flags": (i32, [vp, u32]),
        "rtbvh_bin_builds": (u64, [vp]),
        "rtbvh_bin_sets": (u32, [vp]),
        "rtbvh_sort_pairs_async": (i32, [vp, vp, vp, vp, vp, u32, u32]),
        "rtbvh_sort_pairs_host": (i32, [vp, vp, vp, vp, vp, u32, u32]),
        "rtbvh_build_from_codes": (i32, [vp, vp, vp, u32, vp]),
        "rtbvh_scene_load_obj": (i32, [ctypes.c_char_p, ctypes.POINTER(vp)]),
        "rtbvh_scene_synthetic": (i32, [u64, u32, vp, ctypes.POINTER(vp)]),
        "rtbvh_scene_free": (None, [vp]),
        "rtbvh_scene_num_vertices": (u32, [vp]),
        "rtbvh_scene_num_indices": (u32, [vp]),
        "rtbvh_scene_num_materials": (u32, [vp]),
        "rtbvh_scene_num_textures": (u32, [vp]),
        "rtbvh_scene_vertices": (vp, [vp]),
        "rtbvh_scene_indices": (vp, [vp]),
        "rtbvh_scene_mat_indices": (vp, [vp]),
        "rtbvh_scene_materials": (vp, [vp]),
        "rtbvh_scene_texture_path": (ctypes.c_char_p, [vp, u32]),
        "rtbvh_set_scene_obj": (i32, [vp, vp, vp, u32]),
        "rtbvh_camera_reference": (None, [u32, u32, vp, vp]),
        "rtbvh_camera_look": (None, [vp, u32, u32, vp, vp]),
        "rtbvh_camera_orbit": (None, [vp, u32]),
        "rtbvh_texture_load_bmp": (i32, [ctypes.c_char_p, vp]),
        "rtbvh_texture_load_jpeg": (i32, [ctypes.c_char_p, vp]),
        "rtbvh_texture_decode_jpeg": (i32, [vp, ctypes.c_size_t, vp]),
        "rtbvh_texture_load": (i32, [ctypes.c_char_p, vp]),
        "rtbvh_texture_free": (None, [vp]),
        "rtbvh_srgb_table": (None, [vp]),
        "rtbvh_present": (i32, [vp, vp]),
        "rtbvh_save_bmp": (i32, [ctypes.c_char_p, vp, u32, u32]),
        "rtbvh_query_async": (i32, [vp, vp, u64, vp, u32, vp]),
        "rtbvh_query_host": (i32, [vp, vp, u64, vp, u32]),
        "rtbvh_query_counts": (i32, [vp, vp]),
        "rtbvh_query_walk_counts": (i32, [vp, vp]),
        "rtbvh_nearest_async": (i32, [vp, vp, u64, vp, u32, vp]),
        "rtbvh_nearest_host": (i32, [vp, vp, u64, vp, u32]),
        "rtbvh_nearest_counts": (i32, [vp, vp]),
        "rtbvh_within_async": (i32, [vp, vp, u64, vp, vp, u64, u32, vp]),
        "rtbvh_within_host": (i32, [vp, vp, u64, vp, vp, u64, u32]),
        "rtbvh_within_counts": (i32, [vp, vp]),
        "rtbvh_knn_async": (i32, [vp, vp, u64, u32, vp, u32, vp]),
        "rtbvh_knn_host": (i32, [vp, vp, u64, u32, vp, u32]),
        "rtbvh_knn_counts": (i32, [vp, vp]),
        "rtbvh_signed_async": (i32, [vp, vp, u64, vp, u32, vp]),
        "rtbvh_signed_host": (i32, [vp, vp, u64, vp, u32]),
        "rtbvh_signed_counts": (i32, [vp, vp]),
        "rtbvh_khits_async": (i32, [vp, vp, u64, u32, vp, u32, vp]),
        "rtbvh_khits_host": (i32, [vp, vp, u64, u32, vp, u32]),
        "rtbvh_khits_counts": (i32, [vp, vp]),
        "rtbvh_sweep_async": (i32, [vp, vp, u64, vp, u32, vp]),
        "rtbvh_sweep_host": (i32, [vp, vp, u64, vp, u32]),
        "rtbvh_sweep_counts": (i32, [vp, vp]),
        "rtbvh_allhits_async": (i32, [vp, vp, u64, vp, vp, u64, u32, vp]),
        "rtbvh_allhits_host": (i32, [vp, vp, u64, vp, vp, u64, u32]),
        "rtbvh_allhits_counts": (i32, [vp, vp]),
        "rtbvh_overlap_async": (i32, [vp, vp, u64, vp, vp, u64, u32, vp]),
        "rtbvh_overlap_host": (i32, [vp, vp, u64, vp, vp, u64, u32]),
        "rtbvh_overlap_counts": (i32, [vp, vp]),
        "rtbvh_collide_async": (i32, [vp, vp, vp, u64, u32, vp]),
        "rtbvh_collide_host": (i32, [vp, vp, vp, u64, u32]),
        "rtbvh_collide_counts": (i32, [vp, vp]),
        "rtbvh_cross_async": (i32, [vp, vp, u64, vp, vp, u64, u32, vp]),
        "rtbvh_cross_host": (i32, [vp, vp, u64, vp, vp, u64, u32]),
        "rtbvh_cross_first_async": (i32, [vp, vp, u64, vp, u32, vp]),
        "rtbvh_cross_first_host": (i32, [vp, vp, u64, vp, u32]),
        "rtbvh_cross_counts": (i32, [vp, vp]),
        "rtbvh_clearance_async": (i32, [vp, vp, u64, ctypes.c_float, vp, u32, vp]),
        "rtbvh_clearance_host": (i32, [vp, vp, u64, ctypes.c_float, vp, u32]),
        "rtbvh_clearance_counts": (i32, [vp, vp]),
        "rtbvh_region_async": (i32, [vp, vp, u64, vp, vp, u64, u32, vp]),
        "rtbvh_region_host": (i32, [vp, vp, u64, vp, vp, u64, u32]),
        "rtbvh_region_counts": (i32, [vp, vp]),
        "rtbvh_region_split_counts": (i32, [vp, vp]),
        "rtbvh_update_vertices_async": (i32, [vp, vp, u32, vp, u32, u32, u32, vp]),
        "rtbvh_update_vertices_host": (i32, [vp, vp, u32, vp, u32, u32, u32]),
        "rtbvh_refit_async": (i32, [vp]),
        "rtbvh_refit": (i32, [vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def ptr(a: np.ndarray):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"], "arrays passed to librtbvh must be C-contiguous"
    return ctypes.c_void_p(a.ctypes.data)


def check(status: int, ctx=None) -> None:
    if status != OK:
        msg = lib().rtbvh_last_error(ctx)
        raise RtbvhError(status, msg.decode() if msg else "")
