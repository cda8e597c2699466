"""raytracebvh_amd -- MI355X-native LBVH build + ray traversal (the hot path of
Fierykev/RayTraceBVH) as hand-written HIP kernels for gfx950 behind a C ABI
(include/rtbvh.h, librtbvh.so).  This package is the thin host-side mirror of the
reference's Manager/Graphics + ObjLoader surface; all compute is in the HIP library.
"""
from ._lib import (ALLHITS_BY_T, ALLHITS_COUNT, ALLHITS_FILL, ALLHITS_SIZES, ALLHITS_SORT, BOX_DTYPE,
                   DELTA_CLZ64, DELTA_CPUTESTS, FLAG_COUNT_VISITS, FLAG_NEAREST_FIRST, FLAG_REFRACT_RECORDS,
                   FLAG_SORT_BOUNCE, FLAG_TIMING, FLAG_AUTO_WALK, FLAG_PACKET_PRIMARY,
                   FLAG_REFILL_BOUNCE, FLAG_WIDE_BVH, FLAG_BINNED_PRIMARY, FLAG_CERTIFIED, FLAG_MULTI_KERNEL_BUILD, FLAG_SPLIT_SHIFT,
                   FLAG_GRAPH, HIT_DTYPE, KNN_COUNT, KNN_MAX_K, KNN_SORT, MATERIAL_DTYPE, MORTON_CPUTESTS, MORTON_HLSL, NEAREST_COUNT, NEAREST_DTYPE,
                   NEAREST_SORT, NODE_DTYPE, PAIR_DTYPE, POINT_DTYPE, QUERY_ANY,
                   OVERLAP_COUNT, OVERLAP_FILL, OVERLAP_SIZES, OVERLAP_SORT, OVERLAP_TRIANGLE,
                   SIGNED_COUNT, SIGNED_DTYPE, SIGNED_INSIDE_ONLY, SIGNED_SORT, SIGNED_VOTE3,
                   KHITS_COUNT, KHITS_MAX_K, KHITS_SORT,
                   COLLIDE_COUNT, COLLIDE_FILL, COLLIDE_SIZES, COLLIDE_SYMMETRIC, COLLIDE_TRIANGLE,
                   CROSS_COUNT, CROSS_FILL, CROSS_SIZES, CROSS_SORT, TRI_DTYPE,
                   CLEARANCE_COUNT, CLEARANCE_DTYPE, CLEARANCE_SORT,
                   REGION_COUNT, REGION_DTYPE, REGION_FILL, REGION_NO_ACCEPT, REGION_SIZES, REGION_TRIANGLE,
                   REGION_SPLIT_AUTO, REGION_SPLIT_MAX_PIECES, REGION_SPLIT_SHIFT,
                   SWEEP_ANY, SWEEP_COUNT, SWEEP_DTYPE, SWEEP_HIT_DTYPE, SWEEP_SORT,
                   QUERY_CERTIFIED, QUERY_CLOSEST, QUERY_COUNT, QUERY_SORT, RAY_DTYPE, WITHIN_COUNT, WITHIN_FILL, WITHIN_SIZES,
                   WITHIN_SORT, RtbvhError, lib)
from .graphics import (Context, Graphics, box_region, check_cross_tris, check_nearest_points, check_overlap_boxes,
                       check_query_rays, check_region_planes, check_sweeps, check_vertex_array, comm_destroy,
                       comm_unique_id, frustum_planes, make_boxes, make_points, make_rays, make_regions, make_sweeps,
                       make_tris, region_split, save_bmp, slab_region)
from .scene import (EYE_REFERENCE, KEY_DOWN, KEY_LEFT, KEY_RIGHT, KEY_UP, Scene, camera_look, camera_orbit,
                    camera_reference, load_npz, load_obj, synthetic)

__all__ = ["Context", "Graphics", "Scene", "load_obj", "load_npz", "synthetic", "camera_reference", "camera_look",
           "camera_orbit", "EYE_REFERENCE", "KEY_LEFT", "KEY_RIGHT", "KEY_UP", "KEY_DOWN", "lib",
           "RtbvhError", "NODE_DTYPE", "MATERIAL_DTYPE", "MORTON_CPUTESTS", "MORTON_HLSL", "DELTA_CLZ64",
           "DELTA_CPUTESTS", "FLAG_TIMING", "FLAG_COUNT_VISITS", "FLAG_REFRACT_RECORDS", "FLAG_SORT_BOUNCE",
           "FLAG_NEAREST_FIRST", "FLAG_AUTO_WALK", "FLAG_PACKET_PRIMARY", "FLAG_REFILL_BOUNCE", "FLAG_WIDE_BVH", "FLAG_BINNED_PRIMARY", "FLAG_CERTIFIED",
           "FLAG_MULTI_KERNEL_BUILD", "FLAG_SPLIT_SHIFT", "FLAG_GRAPH",
           "save_bmp", "comm_unique_id", "comm_destroy",
           "RAY_DTYPE", "HIT_DTYPE", "QUERY_CLOSEST", "QUERY_ANY", "QUERY_SORT", "QUERY_COUNT", "QUERY_CERTIFIED",
           "make_rays",
           "POINT_DTYPE", "NEAREST_DTYPE", "NEAREST_SORT", "NEAREST_COUNT", "make_points", "check_nearest_points",
           "PAIR_DTYPE", "WITHIN_SORT", "WITHIN_COUNT", "WITHIN_SIZES", "WITHIN_FILL",
           "KNN_SORT", "KNN_COUNT", "KNN_MAX_K",
           "ALLHITS_SORT", "ALLHITS_COUNT", "ALLHITS_BY_T", "ALLHITS_SIZES", "ALLHITS_FILL",
           "BOX_DTYPE", "OVERLAP_SORT", "OVERLAP_COUNT", "OVERLAP_TRIANGLE", "OVERLAP_SIZES", "OVERLAP_FILL",
           "make_boxes", "check_overlap_boxes",
           "SIGNED_DTYPE", "SIGNED_SORT", "SIGNED_COUNT", "SIGNED_VOTE3", "SIGNED_INSIDE_ONLY",
           "KHITS_SORT", "KHITS_COUNT", "KHITS_MAX_K",
           "COLLIDE_COUNT", "COLLIDE_TRIANGLE", "COLLIDE_SIZES", "COLLIDE_FILL", "COLLIDE_SYMMETRIC",
           "TRI_DTYPE", "CROSS_SORT", "CROSS_COUNT", "CROSS_SIZES", "CROSS_FILL", "make_tris", "check_cross_tris",
           "CLEARANCE_DTYPE", "CLEARANCE_SORT", "CLEARANCE_COUNT",
           "REGION_DTYPE", "REGION_COUNT", "REGION_TRIANGLE", "REGION_SIZES", "REGION_FILL", "REGION_NO_ACCEPT",
           "REGION_SPLIT_SHIFT", "REGION_SPLIT_AUTO", "REGION_SPLIT_MAX_PIECES", "region_split",
           "make_regions", "box_region", "slab_region", "frustum_planes", "check_region_planes",
           "SWEEP_DTYPE", "SWEEP_HIT_DTYPE", "SWEEP_ANY", "SWEEP_SORT", "SWEEP_COUNT", "make_sweeps", "check_sweeps",
           "check_query_rays", "check_vertex_array"]
