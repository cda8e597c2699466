"""Host-side mirror of the reference's Manager/Graphics dispatch surface.

The reference drives the path from `class Graphics : public Manager`
(Graphics.h:16-27): onInit -> loadAssets uploads the ObjLoader arrays
(Graphics.cpp:237-665), onUpdate writes the camera cbuffer and calls the private
computeBVH() (Graphics.cpp:40-61, 667-831).  `Graphics` below keeps those names
and meanings over librtbvh.so; `Context` is the thin 1:1 wrapper of the C ABI.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _lib as _L
from .scene import EYE_REFERENCE, Scene, camera_look, camera_orbit, camera_reference


def _is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def make_rays(origins, directions, t_max=float("inf")):
    """Packs (N, 3) origins and directions (and one t_max, or N of them) as query rays: torch tensors give an
    (N, 8) float32 tensor on their device, anything else a RAY_DTYPE array (include/rtbvh.h rtbvh_ray).  The
    rays live in the space the BVH was built in; directions need not be unit."""
    if _is_tensor(origins) or _is_tensor(directions):
        import torch
        dev = origins.device if _is_tensor(origins) else directions.device
        o = torch.as_tensor(origins, dtype=torch.float32, device=dev).reshape(-1, 3)
        d = torch.as_tensor(directions, dtype=torch.float32, device=dev).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError(f"make_rays: {tuple(o.shape)} origins and {tuple(d.shape)} directions")
        rays = torch.zeros((o.shape[0], 8), dtype=torch.float32, device=dev)
        rays[:, 0:3] = o
        rays[:, 3] = torch.as_tensor(t_max, dtype=torch.float32, device=dev)
        rays[:, 4:7] = d
        return rays
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError(f"make_rays: {o.shape} origins and {d.shape} directions")
    rays = np.zeros(len(o), _L.RAY_DTYPE)
    rays["origin"] = o
    rays["t_max"] = np.asarray(t_max, np.float32)
    rays["direction"] = d
    return rays


def check_query_rays(rays, device=None):
    """Context.query's input check: ("torch", rays) for an (N, 8) float32 contiguous CUDA tensor (on `device`
    when given), ("numpy", RAY_DTYPE view) for a C-contiguous RAY_DTYPE array or (N, 8) float32 array;
    ValueError for anything else.  Calls nothing in the library."""
    if _is_tensor(rays):
        import torch
        if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8:
            raise ValueError(f"query: rays must be an (N, 8) float32 tensor, got {tuple(rays.shape)} {rays.dtype}")
        if not rays.is_cuda:
            raise ValueError("query: a torch tensor of rays must be on the context's GPU (numpy arrays take the host path)")
        if device is not None and rays.device.index != device:
            raise ValueError(f"query: rays on {rays.device}, the context on device {device}")
        if not rays.is_contiguous():
            raise ValueError("query: rays must be contiguous")
        return "torch", rays
    if not isinstance(rays, np.ndarray):
        raise ValueError("query: rays must be a torch CUDA tensor or a numpy array")
    if rays.dtype == _L.RAY_DTYPE:
        if rays.ndim != 1:
            raise ValueError(f"query: a RAY_DTYPE array must be one-dimensional, got shape {rays.shape}")
    elif rays.dtype != np.float32 or rays.ndim != 2 or rays.shape[1] != 8:
        raise ValueError(f"query: rays must be RAY_DTYPE or (N, 8) float32, got {rays.shape} {rays.dtype}")
    if not rays.flags["C_CONTIGUOUS"]:
        raise ValueError("query: rays must be C-contiguous")
    return "numpy", rays.view(_L.RAY_DTYPE).reshape(-1)


def make_sweeps(origins, directions, radius, t_max=float("inf")):
    """Packs (N, 3) origins and directions, a radius and a t_max (each one value, or N of them) as sphere sweeps:
    torch tensors give an (N, 8) float32 tensor on their device, anything else a SWEEP_DTYPE array (include/rtbvh.h
    rtbvh_sweep).  The sweeps live in the space the BVH was built in, the radius too; directions need not be unit."""
    if _is_tensor(origins) or _is_tensor(directions):
        import torch
        dev = origins.device if _is_tensor(origins) else directions.device
        o = torch.as_tensor(origins, dtype=torch.float32, device=dev).reshape(-1, 3)
        d = torch.as_tensor(directions, dtype=torch.float32, device=dev).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError(f"make_sweeps: {tuple(o.shape)} origins and {tuple(d.shape)} directions")
        sweeps = torch.empty((o.shape[0], 8), dtype=torch.float32, device=dev)
        sweeps[:, 0:3] = o
        sweeps[:, 3] = torch.as_tensor(t_max, dtype=torch.float32, device=dev)
        sweeps[:, 4:7] = d
        sweeps[:, 7] = torch.as_tensor(radius, dtype=torch.float32, device=dev)
        return sweeps
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError(f"make_sweeps: {o.shape} origins and {d.shape} directions")
    sweeps = np.zeros(len(o), _L.SWEEP_DTYPE)
    sweeps["origin"] = o
    sweeps["t_max"] = np.asarray(t_max, np.float32)
    sweeps["direction"] = d
    sweeps["radius"] = np.asarray(radius, np.float32)
    return sweeps


def check_sweeps(sweeps, device=None):
    """Context.sweep's input check: ("torch", sweeps) for an (N, 8) float32 contiguous CUDA tensor (on `device` when
    given), ("numpy", SWEEP_DTYPE view) for a C-contiguous SWEEP_DTYPE array or (N, 8) float32 array; ValueError for
    anything else.  Calls nothing in the library."""
    if _is_tensor(sweeps):
        import torch
        if sweeps.dtype != torch.float32 or sweeps.dim() != 2 or sweeps.shape[1] != 8:
            raise ValueError(f"sweep: sweeps must be an (N, 8) float32 tensor (make_sweeps), got "
                             f"{tuple(sweeps.shape)} {sweeps.dtype}")
        if not sweeps.is_cuda:
            raise ValueError("sweep: a torch tensor of sweeps must be on the context's GPU (numpy arrays take the "
                             "host path)")
        if device is not None and sweeps.device.index != device:
            raise ValueError(f"sweep: sweeps on {sweeps.device}, the context on device {device}")
        if not sweeps.is_contiguous():
            raise ValueError("sweep: sweeps must be contiguous")
        return "torch", sweeps
    if not isinstance(sweeps, np.ndarray):
        raise ValueError("sweep: sweeps must be a torch CUDA tensor or a numpy array")
    if sweeps.dtype == _L.SWEEP_DTYPE:
        if sweeps.ndim != 1:
            raise ValueError(f"sweep: a SWEEP_DTYPE array must be one-dimensional, got shape {sweeps.shape}")
    elif sweeps.dtype != np.float32 or sweeps.ndim != 2 or sweeps.shape[1] != 8:
        raise ValueError(f"sweep: sweeps must be SWEEP_DTYPE or (N, 8) float32, got {sweeps.shape} {sweeps.dtype}")
    if not sweeps.flags["C_CONTIGUOUS"]:
        raise ValueError("sweep: sweeps must be C-contiguous")
    return "numpy", sweeps.view(_L.SWEEP_DTYPE).reshape(-1)


def make_points(points, max_dist2=float("inf")):
    """Packs (N, 3) points (and one max_dist2, or N of them) as closest-point queries: a torch tensor gives an
    (N, 4) float32 tensor on its device, anything else a POINT_DTYPE array (include/rtbvh.h rtbvh_point).  The
    points live in the space the BVH was built in."""
    if _is_tensor(points):
        import torch
        p = points.to(torch.float32).reshape(-1, 3)
        out = torch.empty((p.shape[0], 4), dtype=torch.float32, device=p.device)
        out[:, 0:3] = p
        out[:, 3] = torch.as_tensor(max_dist2, dtype=torch.float32, device=p.device)
        return out
    p = np.asarray(points, np.float32).reshape(-1, 3)
    out = np.zeros(len(p), _L.POINT_DTYPE)
    out["point"] = p
    out["max_dist2"] = np.asarray(max_dist2, np.float32)
    return out


def check_nearest_points(points, max_dist2=float("inf"), device=None):
    """Context.nearest's input check: ("torch", points) for an (N, 4) float32 contiguous CUDA tensor (on `device`
    when given), ("numpy", POINT_DTYPE array) for a C-contiguous POINT_DTYPE array, (N, 4) float32 array or
    (N, 3) float32 array (packed with max_dist2: one value or N of them); ValueError for anything else, and for
    a max_dist2 given beside points that carry their own.  Calls nothing in the library."""
    own_bound = np.ndim(max_dist2) == 0 and float(max_dist2) == float("inf")   # (the default: nothing asked for)
    if _is_tensor(points):
        import torch
        if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 4:
            raise ValueError(f"nearest: points must be an (N, 4) float32 tensor (make_points), got "
                             f"{tuple(points.shape)} {points.dtype}")
        if not points.is_cuda:
            raise ValueError("nearest: a torch tensor of points must be on the context's GPU (numpy arrays take the "
                             "host path)")
        if device is not None and points.device.index != device:
            raise ValueError(f"nearest: points on {points.device}, the context on device {device}")
        if not points.is_contiguous():
            raise ValueError("nearest: points must be contiguous")
        if not own_bound:
            raise ValueError("nearest: an (N, 4) tensor carries max_dist2 in its fourth column")
        return "torch", points
    if not isinstance(points, np.ndarray):
        raise ValueError("nearest: points must be a torch CUDA tensor or a numpy array")
    if points.dtype == _L.POINT_DTYPE:
        if points.ndim != 1:
            raise ValueError(f"nearest: a POINT_DTYPE array must be one-dimensional, got shape {points.shape}")
    elif points.dtype != np.float32 or points.ndim != 2 or points.shape[1] not in (3, 4):
        raise ValueError(f"nearest: points must be POINT_DTYPE, (N, 3) or (N, 4) float32, got {points.shape} "
                         f"{points.dtype}")
    if not points.flags["C_CONTIGUOUS"]:
        raise ValueError("nearest: points must be C-contiguous")
    if points.dtype != _L.POINT_DTYPE and points.shape[1] == 3:
        bound = np.asarray(max_dist2, np.float32)
        if bound.ndim > 1 or (bound.ndim == 1 and len(bound) != len(points)):
            raise ValueError(f"nearest: max_dist2 must be one value or {len(points)} of them, got shape {bound.shape}")
        return "numpy", make_points(points, bound)
    if not own_bound:
        raise ValueError("nearest: POINT_DTYPE and (N, 4) points carry max_dist2 themselves")
    return "numpy", points.view(_L.POINT_DTYPE).reshape(-1)


def make_boxes(lo, hi):
    """Packs (N, 3) lower and upper corners as box queries: torch tensors give an (N, 8) float32 tensor on their
    device, anything else a BOX_DTYPE array (include/rtbvh.h rtbvh_box).  The boxes live in the space the BVH was
    built in."""
    if _is_tensor(lo) or _is_tensor(hi):
        import torch
        dev = lo.device if _is_tensor(lo) else hi.device
        a = torch.as_tensor(lo, dtype=torch.float32, device=dev).reshape(-1, 3)
        b = torch.as_tensor(hi, dtype=torch.float32, device=dev).reshape(-1, 3)
        if a.shape != b.shape:
            raise ValueError(f"make_boxes: {tuple(a.shape)} lower and {tuple(b.shape)} upper corners")
        out = torch.zeros((a.shape[0], 8), dtype=torch.float32, device=dev)
        out[:, 0:3] = a
        out[:, 4:7] = b
        return out
    a = np.asarray(lo, np.float32).reshape(-1, 3)
    b = np.asarray(hi, np.float32).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError(f"make_boxes: {a.shape} lower and {b.shape} upper corners")
    out = np.zeros(len(a), _L.BOX_DTYPE)
    out["lo"] = a
    out["hi"] = b
    return out


def check_overlap_boxes(boxes, hi=None, device=None):
    """Context.overlap's input check: ("torch", boxes) for an (N, 8) float32 contiguous CUDA tensor (on `device`
    when given), ("numpy", BOX_DTYPE array) for a C-contiguous BOX_DTYPE array or (N, 8) float32 array, or for
    (N, 3) float32 lower corners with `hi` their (N, 3) float32 upper corners (packed with make_boxes); ValueError
    for anything else, and for a `hi` given beside boxes that carry their own.  Calls nothing in the library."""
    if _is_tensor(boxes):
        import torch
        if hi is not None:
            raise ValueError("overlap: an (N, 8) tensor carries its upper corners (make_boxes)")
        if boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] != 8:
            raise ValueError(f"overlap: boxes must be an (N, 8) float32 tensor (make_boxes), got "
                             f"{tuple(boxes.shape)} {boxes.dtype}")
        if not boxes.is_cuda:
            raise ValueError("overlap: a torch tensor of boxes must be on the context's GPU (numpy arrays take the "
                             "host path)")
        if device is not None and boxes.device.index != device:
            raise ValueError(f"overlap: boxes on {boxes.device}, the context on device {device}")
        if not boxes.is_contiguous():
            raise ValueError("overlap: boxes must be contiguous")
        return "torch", boxes
    if not isinstance(boxes, np.ndarray):
        raise ValueError("overlap: boxes must be a torch CUDA tensor or a numpy array")
    if hi is not None:
        if not isinstance(hi, np.ndarray) or boxes.dtype != np.float32 or hi.dtype != np.float32 or boxes.ndim != 2 or \
                boxes.shape[1] != 3 or hi.shape != boxes.shape:
            raise ValueError("overlap: lower and upper corners must be (N, 3) float32 arrays of one shape")
        return "numpy", make_boxes(boxes, hi)
    if boxes.dtype == _L.BOX_DTYPE:
        if boxes.ndim != 1:
            raise ValueError(f"overlap: a BOX_DTYPE array must be one-dimensional, got shape {boxes.shape}")
    elif boxes.dtype != np.float32 or boxes.ndim != 2 or boxes.shape[1] != 8:
        raise ValueError(f"overlap: boxes must be BOX_DTYPE or (N, 8) float32, got {boxes.shape} {boxes.dtype}")
    if not boxes.flags["C_CONTIGUOUS"]:
        raise ValueError("overlap: boxes must be C-contiguous")
    return "numpy", boxes.view(_L.BOX_DTYPE).reshape(-1)


def make_regions(planes):
    """Packs (N, P, 4) planes {nx, ny, nz, d}, P <= 6 (one region: (P, 4)), as region queries, the planes past P
    all zero (they hold everywhere): a torch tensor gives an (N, 24) float32 tensor on its device, anything else a
    REGION_DTYPE array (include/rtbvh.h rtbvh_region).  A point x is inside a plane when n.x + d <= 0; the planes
    live in the space the BVH was built in."""
    if _is_tensor(planes):
        import torch
        p = planes.to(torch.float32)
        if p.dim() == 2:
            p = p.reshape(1, *p.shape)
        if p.dim() != 3 or p.shape[1] > 6 or p.shape[2] != 4:
            raise ValueError(f"make_regions: planes must be (N, P <= 6, 4), got {tuple(planes.shape)}")
        out = torch.zeros((p.shape[0], 6, 4), dtype=torch.float32, device=p.device)
        out[:, :p.shape[1]] = p
        return out.reshape(-1, 24)
    p = np.asarray(planes, np.float32)
    if p.ndim == 2:
        p = p.reshape(1, *p.shape)
    if p.ndim != 3 or p.shape[1] > 6 or p.shape[2] != 4:
        raise ValueError(f"make_regions: planes must be (N, P <= 6, 4), got {np.shape(planes)}")
    out = np.zeros(len(p), _L.REGION_DTYPE)
    out["plane"][:, :p.shape[1]] = p
    return out


def box_region(lo, hi):
    """The axis-aligned boxes [lo, hi] ((N, 3) each, or one) as regions of six axis planes {-1, 0, 0, lo_x},
    {1, 0, 0, -hi_x}, ...: a plane {+-1, 0, 0, -+q} evaluates x <= q and q <= x exactly, so these regions list what
    Context.overlap lists for the boxes.  Numpy in, a REGION_DTYPE array out."""
    a = np.asarray(lo, np.float32).reshape(-1, 3)
    b = np.asarray(hi, np.float32).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError(f"box_region: {a.shape} lower and {b.shape} upper corners")
    planes = np.zeros((len(a), 6, 4), np.float32)
    for k in range(3):
        planes[:, 2 * k, k] = -1.0      # lo_k - x_k <= 0
        planes[:, 2 * k, 3] = a[:, k]
        planes[:, 2 * k + 1, k] = 1.0   # x_k - hi_k <= 0
        planes[:, 2 * k + 1, 3] = -b[:, k]
    return make_regions(planes)


def slab_region(normal, d_lo, d_hi):
    """The slabs d_lo <= n.x <= d_hi ((N, 3) normals or one, scalars or N bounds) as regions of the two planes
    {-n, d_lo}, {n, -d_hi}; d_lo == d_hi is the plane n.x = d itself, whose REGION_TRIANGLE list holds the triangles
    it cuts.  Numpy in, a REGION_DTYPE array out."""
    n = np.asarray(normal, np.float32).reshape(-1, 3)
    lo = np.broadcast_to(np.asarray(d_lo, np.float32), (len(n),))
    hi = np.broadcast_to(np.asarray(d_hi, np.float32), (len(n),))
    planes = np.zeros((len(n), 2, 4), np.float32)
    planes[:, 0, :3] = -n
    planes[:, 0, 3] = lo
    planes[:, 1, :3] = n
    planes[:, 1, 3] = -hi
    return make_regions(planes)


def frustum_planes(wvp):
    """The six planes (6, 4) float32 -- left, right, bottom, top, near, far -- of the view volume of a row-vector
    WVP ([x y z 1] . WVP = clip) with D3D depth: -w <= x <= w, -w <= y <= w, 0 <= z <= w, each as {n, d} with the
    inside n.p + d <= 0.  They are planes of the WVP's input space, so they fit a context whose BVH was built with
    an identity camera.  Computed in float64 from the matrix, rounded once."""
    m = np.asarray(wvp, np.float64).reshape(4, 4)
    cx, cy, cz, cw = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    return np.stack([-(cw + cx), -(cw - cx), -(cw + cy), -(cw - cy), -cz, -(cw - cz)]).astype(np.float32)


def region_split(k: int) -> int:
    """The mode bits that cut each region of Context.region into at most k pieces along the tree (the header's split
    field): k a power of two from 2 to 4096.  REGION_SPLIT_AUTO lets the library choose.  ValueError otherwise."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 2 or k > 4096 or k & (k - 1):
        raise ValueError(f"region_split: k must be a power of two from 2 to 4096, got {k!r}")
    return (int(k).bit_length() - 1) << _L.REGION_SPLIT_SHIFT


def check_region_planes(regions, device=None):
    """Context.region's input check: ("torch", regions) for an (N, 24) float32 contiguous CUDA tensor (on `device`
    when given), ("numpy", REGION_DTYPE array) for a C-contiguous REGION_DTYPE array, (N, 24) float32 array or
    (N, P <= 6, 4) float32 array (packed with make_regions); ValueError for anything else.  Calls nothing in the
    library."""
    if _is_tensor(regions):
        import torch
        if regions.dtype != torch.float32 or regions.dim() != 2 or regions.shape[1] != 24:
            raise ValueError(f"region: regions must be an (N, 24) float32 tensor (make_regions), got "
                             f"{tuple(regions.shape)} {regions.dtype}")
        if not regions.is_cuda:
            raise ValueError("region: a torch tensor of regions must be on the context's GPU (numpy arrays take the "
                             "host path)")
        if device is not None and regions.device.index != device:
            raise ValueError(f"region: regions on {regions.device}, the context on device {device}")
        if not regions.is_contiguous():
            raise ValueError("region: regions must be contiguous")
        return "torch", regions
    if not isinstance(regions, np.ndarray):
        raise ValueError("region: regions must be a torch CUDA tensor or a numpy array")
    if regions.dtype == _L.REGION_DTYPE:
        if regions.ndim != 1:
            raise ValueError(f"region: a REGION_DTYPE array must be one-dimensional, got shape {regions.shape}")
    elif regions.dtype == np.float32 and regions.ndim == 3 and regions.shape[1] <= 6 and regions.shape[2] == 4:
        return "numpy", make_regions(regions)
    elif regions.dtype != np.float32 or regions.ndim != 2 or regions.shape[1] != 24:
        raise ValueError(f"region: regions must be REGION_DTYPE, (N, 24) or (N, P <= 6, 4) float32, got "
                         f"{regions.shape} {regions.dtype}")
    if not regions.flags["C_CONTIGUOUS"]:
        raise ValueError("region: regions must be C-contiguous")
    return "numpy", regions.view(_L.REGION_DTYPE).reshape(-1)


def make_tris(vertices):
    """Packs (N, 3, 3) or (N, 9) triangle vertices {v0, v1, v2} as triangle queries: a torch tensor gives an (N, 12)
    float32 tensor on its device, anything else a TRI_DTYPE array (include/rtbvh.h rtbvh_tri).  The triangles live
    in the space the BVH was built in."""
    if _is_tensor(vertices):
        import torch
        v = vertices.to(torch.float32)
        if not ((v.dim() == 3 and tuple(v.shape[1:]) == (3, 3)) or (v.dim() == 2 and v.shape[1] == 9)):
            raise ValueError(f"make_tris: vertices must be (N, 3, 3) or (N, 9), got {tuple(v.shape)}")
        out = torch.zeros((v.shape[0], 3, 4), dtype=torch.float32, device=v.device)
        out[:, :, 0:3] = v.reshape(-1, 3, 3)
        return out.reshape(-1, 12)
    v = np.asarray(vertices, np.float32)
    if not ((v.ndim == 3 and v.shape[1:] == (3, 3)) or (v.ndim == 2 and v.shape[1] == 9)):
        raise ValueError(f"make_tris: vertices must be (N, 3, 3) or (N, 9), got {v.shape}")
    v = v.reshape(-1, 3, 3)
    out = np.zeros(len(v), _L.TRI_DTYPE)
    out["v0"], out["v1"], out["v2"] = v[:, 0], v[:, 1], v[:, 2]
    return out


def check_cross_tris(tris, device=None):
    """Context.cross's input check: ("torch", tris) for an (N, 12) float32 contiguous CUDA tensor (on `device` when
    given), ("numpy", TRI_DTYPE array) for a C-contiguous TRI_DTYPE array or (N, 12) float32 array (make_tris packs
    either from vertices); ValueError for anything else.  Calls nothing in the library."""
    if _is_tensor(tris):
        import torch
        if tris.dtype != torch.float32 or tris.dim() != 2 or tris.shape[1] != 12:
            raise ValueError(f"cross: tris must be an (N, 12) float32 tensor (make_tris), got "
                             f"{tuple(tris.shape)} {tris.dtype}")
        if not tris.is_cuda:
            raise ValueError("cross: a torch tensor of triangles must be on the context's GPU (numpy arrays take the "
                             "host path)")
        if device is not None and tris.device.index != device:
            raise ValueError(f"cross: tris on {tris.device}, the context on device {device}")
        if not tris.is_contiguous():
            raise ValueError("cross: tris must be contiguous")
        return "torch", tris
    if not isinstance(tris, np.ndarray):
        raise ValueError("cross: tris must be a torch CUDA tensor or a numpy array")
    if tris.dtype == _L.TRI_DTYPE:
        if tris.ndim != 1:
            raise ValueError(f"cross: a TRI_DTYPE array must be one-dimensional, got shape {tris.shape}")
    elif tris.dtype != np.float32 or tris.ndim != 2 or tris.shape[1] != 12:
        raise ValueError(f"cross: tris must be TRI_DTYPE or (N, 12) float32 (make_tris), got {tris.shape} {tris.dtype}")
    if not tris.flags["C_CONTIGUOUS"]:
        raise ValueError("cross: tris must be C-contiguous")
    return "numpy", tris.view(_L.TRI_DTYPE).reshape(-1)


def check_vertex_array(a, what="positions", device=None):
    """Context.update_vertices' input check: (kind, array, stride in floats) for an (n, 3) float32 torch CUDA
    tensor ("torch"; on `device` when given) or numpy array ("numpy") whose last dimension is contiguous and
    whose rows are at least 3 floats apart -- a packed (V, 3) array (stride 3), the [:, :3] view of a float4
    array (4) or of an rtbvh_vertex array (8); ValueError for anything else.  Calls nothing in the library."""
    name = "update_vertices: " + what
    if _is_tensor(a):
        import torch
        if a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 3:
            raise ValueError(f"{name} must be an (n, 3) float32 tensor, got {tuple(a.shape)} {a.dtype}")
        if not a.is_cuda:
            raise ValueError(f"{name}: a torch tensor must be on the context's GPU (numpy arrays take the host path)")
        if device is not None and a.device.index != device:
            raise ValueError(f"{name} on {a.device}, the context on device {device}")
        if a.shape[0] <= 1:
            return "torch", a.contiguous(), 3
        if a.stride(1) != 1 or a.stride(0) < 3:
            raise ValueError(f"{name}: the last dimension must be contiguous and the rows at least 3 floats apart, "
                             f"got strides {tuple(a.stride())}")
        return "torch", a, a.stride(0)
    if not isinstance(a, np.ndarray):
        raise ValueError(f"{name} must be a torch CUDA tensor or a numpy array")
    if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{name} must be an (n, 3) float32 array, got {a.shape} {a.dtype}")
    if a.shape[0] <= 1:
        return "numpy", np.ascontiguousarray(a), 3
    if a.strides[1] != 4 or a.strides[0] % 4 or a.strides[0] < 12:
        raise ValueError(f"{name}: the last dimension must be contiguous and the rows at least 3 floats apart, "
                         f"got byte strides {a.strides}")
    return "numpy", a, a.strides[0] // 4


class Context:
    """One rtbvh_ctx: one HIP device, one stream, the scene/BVH/frame buffers."""

    def __init__(self, device: int = 0, morton_mode: int = _L.MORTON_CPUTESTS, delta_mode: int = _L.DELTA_CLZ64,
                 flags: int = 0, scene_bb_min=(-700.0,) * 3, scene_bb_max=(700.0,) * 3, stream: int | None = None,
                 stack_limit: int = 0):
        L = _L.lib()
        cfg = _L.Config()
        L.rtbvh_config_default(ctypes.byref(cfg))
        cfg.device = device
        cfg.morton_mode = morton_mode
        cfg.delta_mode = delta_mode
        cfg.flags = flags
        cfg.scene_bb_min[:] = list(scene_bb_min)
        cfg.scene_bb_max[:] = list(scene_bb_max)
        cfg.stream = stream
        cfg.stack_limit = stack_limit
        h = ctypes.c_void_p()
        _L.check(L.rtbvh_create(ctypes.byref(cfg), ctypes.byref(h)), None)
        self._h = h
        self.device = device
        self.num_tris = 0
        self.width = self.height = 0

    # -- lifecycle --
    def close(self):
        if getattr(self, "_h", None):
            _L.lib().rtbvh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, st):
        _L.check(st, self._h)

    # -- inputs --
    def set_scene(self, scene: Scene):
        self._scene = scene   # keep arrays alive for the duration of the call (copied by the library)
        tex = (_L.Texture * max(len(scene.textures), 1))()
        for k, t in enumerate(scene.textures):
            tex[k] = _L.Texture(t.shape[1], t.shape[0], t.ctypes.data)
        self._check(_L.lib().rtbvh_set_scene(self._h, _L.ptr(scene.vertices), len(scene.vertices),
                                             _L.ptr(scene.indices), len(scene.indices), _L.ptr(scene.mat_indices),
                                             _L.ptr(scene.materials), len(scene.materials),
                                             ctypes.byref(tex) if scene.textures else None, len(scene.textures)))
        self.num_tris = scene.num_tris

    def set_camera(self, wvp, wv):
        wvp = np.ascontiguousarray(wvp, dtype=np.float32).reshape(16)
        wv = np.ascontiguousarray(wv, dtype=np.float32).reshape(16)
        self._check(_L.lib().rtbvh_set_camera(self._h, _L.ptr(wvp), _L.ptr(wv)))

    # -- hot path --
    def build(self, sync: bool = True):
        L = _L.lib()
        self._check(L.rtbvh_build(self._h) if sync else L.rtbvh_build_async(self._h))

    def trace(self, width: int, height: int, bounces: int = 1, sync: bool = True):
        L = _L.lib()
        f = L.rtbvh_trace if sync else L.rtbvh_trace_async
        self._check(f(self._h, width, height, bounces))
        self.width, self.height = width, height

    def compute_bvh(self, width: int, height: int, bounces: int = 1):
        self._check(_L.lib().rtbvh_compute_bvh(self._h, width, height, bounces))
        self.width, self.height = width, height

    def verify_walk(self, width: int, height: int, bounces: int = 1) -> int:
        """rtbvh_verify_walk: pixels whose bits differ between the reference-order frame and
        the frame of this context's walks (0: identical); leaves the latter in the framebuffer."""
        n = ctypes.c_uint64()
        self._check(_L.lib().rtbvh_verify_walk(self._h, width, height, bounces, ctypes.byref(n)))
        self.width, self.height = width, height
        return n.value

    def trace_band_async(self, width: int, height: int, bounces: int, rank: int, nranks: int, dev_out_ptr: int,
                         stream_ptr: int | None = None):
        self._check(_L.lib().rtbvh_trace_band_async(self._h, width, height, bounces, rank, nranks,
                                                    ctypes.c_void_p(dev_out_ptr),
                                                    ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def set_band_deal(self, root_share: int):
        """rtbvh_set_band_deal: rank 0's share of the bands in 1/16 of another rank's (16 = b % nranks)."""
        self._check(_L.lib().rtbvh_set_band_deal(self._h, root_share))

    def assemble_bands(self, width: int, height: int, nranks: int, dev_bands_ptr: int, stride_rows: int,
                       dev_frame_ptr: int, stream_ptr: int | None = None):
        """rtbvh_assemble_bands: the frame from the ranks' compact band buffers (one device)."""
        self._check(_L.lib().rtbvh_assemble_bands(self._h, width, height, nranks, ctypes.c_void_p(dev_bands_ptr),
                                                  stride_rows, ctypes.c_void_p(dev_frame_ptr),
                                                  ctypes.c_void_p(stream_ptr) if stream_ptr else None))

    def comm_init(self, nranks: int, rank: int, unique_id: bytes) -> int:
        """rtbvh_comm_init: an RCCL communicator (ncclComm_t) for this context's device."""
        assert len(unique_id) == _L.COMM_ID_BYTES
        comm = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * _L.COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._check(_L.lib().rtbvh_comm_init(self._h, nranks, rank, buf, ctypes.byref(comm)))
        return comm.value

    def trace_tiles(self, width: int, height: int, bounces: int, rank: int, nranks: int, comm: int):
        """rtbvh_trace_tiles: this rank's bands + the RCCL gather; rank 0 then holds the frame."""
        self._check(_L.lib().rtbvh_trace_tiles(self._h, width, height, bounces, rank, nranks, ctypes.c_void_p(comm)))
        self.width, self.height = width, height

    def synchronize(self):
        self._check(_L.lib().rtbvh_synchronize(self._h))

    # -- animated geometry --
    def update_vertices(self, positions, normals=None, first: int = 0, stream=None):
        """rtbvh_update_vertices_async / rtbvh_update_vertices_host: new positions (and, when given, normals) for
        the vertices [first, first + n) of the scene; indices, materials and texcoords stay (include/rtbvh.h).

        (n, 3) float32 torch CUDA tensors on the context's device go to the device entry with no host copy,
        enqueued on `stream` (a torch stream or a hipStream_t handle; default: the current torch stream; torch's
        legacy default stream, which the library cannot name, is synchronised and the update runs on the context
        stream); numpy arrays go through the synchronous host entry.  The row stride is taken from the array
        (check_vertex_array).  Until the next build(), refit() or compute_bvh(), trace() and query() raise
        ERR_NOT_READY.  ValueError for a wrong dtype, device, shape or layout."""
        kind, pos, ps = check_vertex_array(positions, "positions", getattr(self, "device", None))
        nrm, ns = None, 0
        if normals is not None:
            nkind, nrm, ns = check_vertex_array(normals, "normals", getattr(self, "device", None))
            if nkind != kind or nrm.shape[0] != pos.shape[0]:
                raise ValueError("update_vertices: normals must be of the positions' kind and length")
        n = int(pos.shape[0])
        if first < 0 or n < 0 or first + n > 0xFFFFFFFF:
            raise ValueError("update_vertices: first + n out of range")
        L = _L.lib()
        if kind == "numpy":
            self._check(L.rtbvh_update_vertices_host(self._h, ctypes.c_void_p(pos.ctypes.data), ps,
                                                     ctypes.c_void_p(nrm.ctypes.data) if nrm is not None else None,
                                                     ns, first, n))
            return
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(pos.device)
        handle = int(getattr(stream, "cuda_stream", stream) or 0)
        if handle == 0:
            torch.cuda.default_stream(pos.device).synchronize()
        self._check(L.rtbvh_update_vertices_async(self._h, ctypes.c_void_p(pos.data_ptr()), ps,
                                                  ctypes.c_void_p(nrm.data_ptr()) if nrm is not None else None,
                                                  ns, first, n, ctypes.c_void_p(handle) if handle else None))
        if handle == 0:
            self.synchronize()

    def refit(self, sync: bool = True):
        """rtbvh_refit / rtbvh_refit_async: new boxes over the last build's sort order and topology, for the
        current positions and camera."""
        L = _L.lib()
        self._check(L.rtbvh_refit(self._h) if sync else L.rtbvh_refit_async(self._h))

    # -- what the query methods share --
    def _stream(self, stream, device):
        """(stream, handle) of a query's `stream`: a torch stream or a hipStream_t handle; None: the current torch
        stream on `device`.  Torch's legacy default stream (handle 0), which the library cannot name, is
        synchronised here: the call then runs on the context stream (_enqueue)."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(device)
        handle = int(getattr(stream, "cuda_stream", stream) or 0)
        if handle == 0:
            torch.cuda.default_stream(device).synchronize()
        return stream, handle

    def _enqueue(self, handle, entry, *args):
        """One device entry, entry(ctx, *args, stream), on _stream's handle; the context stream (handle 0) is
        synchronised behind it."""
        self._check(entry(self._h, *args, ctypes.c_void_p(handle) if handle else None))
        if handle == 0:
            self.synchronize()

    def _async(self, entry, stream, device, *args):
        self._enqueue(self._stream(stream, device)[1], entry, *args)

    def _lists(self, host, dev, inp, n, item, shape, tdtype, sizes, fill, mode, sizes_mode, capacity, sizes_only,
               stream, on_device=None):
        """A query that answers (offsets, items) in CSR form through its `host` or `dev` entry.  `inp`: the checked
        queries, a numpy array (the host entry) or a CUDA tensor (the device entry), or None for the entries that
        take none (then on_device says which); `n`: how many lists.  The items: numpy dtype `item` on the host, a
        (capacity,) + `shape` tensor of torch dtype `tdtype` on the device.  With `capacity` one call in `mode`;
        without, a call with the kind's `sizes` bit (in `sizes_mode`), one read of the total -- on the device path
        one .item(), the only synchronisation -- and a call with its `fill` bit; sizes_only: the offsets alone."""
        if on_device is None:
            on_device = _is_tensor(inp)
        if not on_device:
            offsets = np.zeros(n + 1, np.uint64)
            head = (self._h,) if inp is None else (self._h, ctypes.c_void_p(inp.ctypes.data), n)
            head += (ctypes.c_void_p(offsets.ctypes.data),)
            if capacity is not None:
                items = np.zeros(int(capacity), item)
                self._check(host(*head, ctypes.c_void_p(items.ctypes.data), len(items), mode))
                return offsets, items[:min(int(offsets[n]), len(items))]
            self._check(host(*head, None, 0, sizes_mode | sizes))
            if sizes_only:
                return offsets
            items = np.zeros(int(offsets[n]), item)
            self._check(host(*head, ctypes.c_void_p(items.ctypes.data), len(items), mode | fill))
            return offsets, items
        import torch
        device = torch.device("cuda", self.device) if inp is None else inp.device
        tdtype = getattr(torch, tdtype)
        offsets = torch.empty(n + 1, dtype=torch.int64, device=device)
        stream, handle = self._stream(stream, device)
        head = () if inp is None else (ctypes.c_void_p(inp.data_ptr()), n)
        head += (ctypes.c_void_p(offsets.data_ptr()),)

        def call(items, m):
            self._enqueue(handle, dev, *head, ctypes.c_void_p(items.data_ptr()) if items is not None and items.numel()
                          else None, 0 if items is None else items.shape[0], m)

        if capacity is not None:
            items = torch.empty((int(capacity),) + shape, dtype=tdtype, device=device)
            call(items, mode)
            return offsets, items
        call(None, sizes_mode | sizes)
        if sizes_only:
            return offsets
        if handle:   # (.item() copies on the current stream: make that the one the sizes ran on)
            ts = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(handle, device=device)
            with torch.cuda.stream(ts):
                total = int(offsets[n].item())
        else:
            total = int(offsets[n].item())
        items = torch.empty((total,) + shape, dtype=tdtype, device=device)
        call(items, mode | fill)
        return offsets, items

    def _counts(self, name, fields):
        """rtbvh_<name>_counts as a dict of `fields`."""
        out = np.zeros(len(fields), np.uint64)
        self._check(getattr(_L.lib(), f"rtbvh_{name}_counts")(self._h, _L.ptr(out)))
        return dict(zip(fields, (int(v) for v in out)))

    # -- ray queries --
    def query(self, rays, mode: int = 0, out=None, stream=None):
        """rtbvh_query_async / rtbvh_query_host: the closest hit (or with QUERY_ANY any hit) of each ray, in the
        space the BVH was built in (include/rtbvh.h).  QUERY_CERTIFIED: the same hits through the certified 4-wide walk.

        An (N, 8) float32 contiguous CUDA tensor on the context's device (make_rays) goes to the device entry with
        no host copy, enqueued on `stream` (a torch stream or a hipStream_t handle; default: the current torch
        stream), and returns an (N, 4) float32 device tensor {t, u, v, tri}: read the triangle ids with
        hits[:, 3].view(torch.int32) (a miss: t = -1, tri = -1).  On torch's legacy default stream (handle 0,
        which the library cannot name) the query runs on the context stream between two synchronisations.
        A RAY_DTYPE or (N, 8) float32 numpy array goes through the synchronous host entry and returns a HIT_DTYPE
        array.  `out` receives the hits when given.  ValueError for a wrong shape, dtype, device or layout."""
        kind, rays = check_query_rays(rays, getattr(self, "device", None))
        n = len(rays)
        L = _L.lib()
        if kind == "numpy":
            if out is None:
                out = np.zeros(n, _L.HIT_DTYPE)
            elif not (isinstance(out, np.ndarray) and out.dtype == _L.HIT_DTYPE and out.shape == (n,) and
                      out.flags["C_CONTIGUOUS"]):
                raise ValueError(f"query: out must be a contiguous HIT_DTYPE array of {n} hits")
            self._check(L.rtbvh_query_host(self._h, ctypes.c_void_p(rays.ctypes.data), n,
                                           ctypes.c_void_p(out.ctypes.data), mode))
            return out
        import torch
        if out is None:
            out = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
        elif not (_is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (n, 4) and
                  out.device == rays.device and out.is_contiguous()):
            raise ValueError(f"query: out must be a contiguous ({n}, 4) float32 tensor on {rays.device}")
        self._async(_L.lib().rtbvh_query_async, stream, rays.device, ctypes.c_void_p(rays.data_ptr()), n,
                    ctypes.c_void_p(out.data_ptr()), mode)
        return out

    def query_counts(self) -> dict:
        """rtbvh_query_counts: rays, hits, internal and leaf visits of the last QUERY_COUNT query."""
        return self._counts("query", ("rays", "hits", "internal_visits", "leaf_visits"))

    def query_walk_counts(self) -> dict:
        """rtbvh_query_walk_counts: how the rays of the last QUERY_COUNT query were answered -- certified by the
        4-wide walk (QUERY_CERTIFIED), redone or uncovered (re-traced in the reference order), or fallback (a query
        that took the plain kernel for every ray).  The four sum to the query's rays."""
        return self._counts("query_walk", ("certified", "redone", "uncovered", "fallback"))

    # -- closest-point queries --
    def nearest(self, points, max_dist2=float("inf"), mode: int = 0, out=None, stream=None):
        """rtbvh_nearest_async / rtbvh_nearest_host: for each point the nearest triangle within max_dist2, the
        closest point on it, its squared distance and barycentrics, in the space the BVH was built in
        (include/rtbvh.h: distances are object-space distances only under an identity WVP).

        An (N, 4) float32 contiguous CUDA tensor {x, y, z, max_dist2} on the context's device (make_points) goes to
        the device entry with no host copy and no synchronisation, enqueued on `stream` (a torch stream or a
        hipStream_t handle; default: the current torch stream; torch's legacy default stream as in query), and
        returns an (N, 8) float32 device tensor {point, dist2, u, v, tri, 0}: read the triangle ids with
        out[:, 6].view(torch.int32) (no result: dist2 = -1, tri = -1).  A POINT_DTYPE, (N, 4) or (N, 3) float32
        numpy array -- the last packed with `max_dist2`, one value or N -- goes through the synchronous host entry
        and returns a NEAREST_DTYPE array.  `out` receives the results when given.  mode: NEAREST_SORT,
        NEAREST_COUNT.  ValueError for a wrong shape, dtype, device or layout."""
        kind, pts = check_nearest_points(points, max_dist2, getattr(self, "device", None))
        n = len(pts)
        if kind == "numpy":
            if out is None:
                out = np.zeros(n, _L.NEAREST_DTYPE)
            elif not (isinstance(out, np.ndarray) and out.dtype == _L.NEAREST_DTYPE and out.shape == (n,) and
                      out.flags["C_CONTIGUOUS"]):
                raise ValueError(f"nearest: out must be a contiguous NEAREST_DTYPE array of {n} results")
            self._check(_L.lib().rtbvh_nearest_host(self._h, ctypes.c_void_p(pts.ctypes.data), n,
                                                    ctypes.c_void_p(out.ctypes.data), mode))
            return out
        import torch
        if out is None:
            out = torch.empty((n, 8), dtype=torch.float32, device=pts.device)
        elif not (_is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (n, 8) and
                  out.device == pts.device and out.is_contiguous()):
            raise ValueError(f"nearest: out must be a contiguous ({n}, 8) float32 tensor on {pts.device}")
        self._async(_L.lib().rtbvh_nearest_async, stream, pts.device, ctypes.c_void_p(pts.data_ptr()), n,
                    ctypes.c_void_p(out.data_ptr()), mode)
        return out

    def nearest_counts(self) -> dict:
        """rtbvh_nearest_counts: points, results found, internal-node and leaf steps of the last NEAREST_COUNT
        query (the ray queries' counts are kept apart)."""
        return self._counts("nearest", ("points", "found", "internal_steps", "leaf_steps"))

    # -- radius queries --
    def within(self, points, max_dist2=float("inf"), mode: int = 0, capacity=None, stream=None):
        """rtbvh_within_async / rtbvh_within_host: for each point every triangle whose dist2 (Context.nearest's) is
        <= max_dist2, as (offsets, pairs) in CSR form: point k's (triangle id, dist2) pairs are
        pairs[offsets[k]:offsets[k + 1]], in the last build's sort order (read_sorted), and offsets[n] is the total.

        `points` as Context.nearest takes them.  A numpy input goes through the synchronous host entry and returns a
        uint64 (n + 1,) array and a PAIR_DTYPE array of offsets[n] pairs (of min(offsets[n], capacity) when
        `capacity` is given).  A torch CUDA (N, 4) tensor goes to the device entry, enqueued on `stream` as nearest's,
        and returns an int64 (n + 1,) device tensor and a (capacity, 2) float32 device tensor {tri, dist2} whose rows
        [0, min(total, capacity)) are written: read the ids with pairs[:, 0].view(torch.int32).  With `capacity`
        given that is one call, with no host copy and no synchronisation -- compare offsets[-1] with it afterwards;
        with capacity=None a WITHIN_SIZES call, one .item() read of the total (the only synchronisation) and a
        WITHIN_FILL call.  mode: WITHIN_SORT, WITHIN_COUNT (WITHIN_SIZES and WITHIN_FILL are this method's to set).
        ValueError for a wrong shape, dtype, device or layout."""
        kind, pts = check_nearest_points(points, max_dist2, getattr(self, "device", None))
        if mode & (_L.WITHIN_SIZES | _L.WITHIN_FILL):
            raise ValueError("within: WITHIN_SIZES and WITHIN_FILL are set by within itself")
        if capacity is not None and (int(capacity) != capacity or capacity < 0):
            raise ValueError(f"within: capacity must be a non-negative integer, got {capacity!r}")
        L = _L.lib()
        return self._lists(L.rtbvh_within_host, L.rtbvh_within_async, pts, len(pts), _L.PAIR_DTYPE, (2,), "float32",
                           _L.WITHIN_SIZES, _L.WITHIN_FILL, mode, mode, capacity, False, stream)

    def within_counts(self) -> dict:
        """rtbvh_within_counts: points, pairs (the total), internal-node and leaf steps (summed over the passes) of
        the last WITHIN_COUNT query (the ray and closest-point counts are kept apart)."""
        return self._counts("within", ("points", "pairs", "internal_steps", "leaf_steps"))

    # -- k-nearest queries --
    def knn(self, points, k, max_dist2=float("inf"), mode: int = 0, out=None, stream=None):
        """rtbvh_knn_async / rtbvh_knn_host: for each point the k triangles with the smallest (dist2, triangle id)
        among those whose dist2 (Context.nearest's) is <= max_dist2, ascending; a slot past the number found holds
        tri = 0xFFFFFFFF, dist2 = -1.  k: 1 .. KNN_MAX_K.

        `points` as Context.nearest takes them.  A numpy input goes through the synchronous host entry and returns
        an (n, k) PAIR_DTYPE array.  A torch CUDA (N, 4) tensor goes to the device entry with no host copy and no
        synchronisation, enqueued on `stream` as nearest's, and returns an (n, k, 2) float32 device tensor
        {tri, dist2}, as Context.within's pairs: read the ids with out[..., 0].view(torch.int32) (none: -1).  `out`
        receives the lists when given.  mode: KNN_SORT, KNN_COUNT.  ValueError for a bad k and for a wrong shape,
        dtype, device or layout."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= _L.KNN_MAX_K:
            raise ValueError(f"knn: k must be an integer from 1 to {_L.KNN_MAX_K}, got {k!r}")
        k = int(k)
        kind, pts = check_nearest_points(points, max_dist2, getattr(self, "device", None))
        n = len(pts)
        if kind == "numpy":
            if out is None:
                out = np.zeros((n, k), _L.PAIR_DTYPE)
            elif not (isinstance(out, np.ndarray) and out.dtype == _L.PAIR_DTYPE and out.shape == (n, k) and
                      out.flags["C_CONTIGUOUS"]):
                raise ValueError(f"knn: out must be a contiguous ({n}, {k}) PAIR_DTYPE array")
            self._check(_L.lib().rtbvh_knn_host(self._h, ctypes.c_void_p(pts.ctypes.data), n, k,
                                                ctypes.c_void_p(out.ctypes.data), mode))
            return out
        import torch
        if out is None:
            out = torch.empty((n, k, 2), dtype=torch.float32, device=pts.device)
        elif not (_is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (n, k, 2) and
                  out.device == pts.device and out.is_contiguous()):
            raise ValueError(f"knn: out must be a contiguous ({n}, {k}, 2) float32 tensor on {pts.device}")
        self._async(_L.lib().rtbvh_knn_async, stream, pts.device, ctypes.c_void_p(pts.data_ptr()), n, k,
                    ctypes.c_void_p(out.data_ptr()), mode)
        return out

    def knn_counts(self) -> dict:
        """rtbvh_knn_counts: points, pairs found, internal-node and leaf steps of the last KNN_COUNT query (the other
        queries' counts are kept apart)."""
        return self._counts("knn", ("points", "found", "internal_steps", "leaf_steps"))

    # -- all-hits ray queries --
    def allhits(self, rays, mode: int = 0, capacity=None, stream=None, sizes_only: bool = False):
        """rtbvh_allhits_async / rtbvh_allhits_host: for each ray every triangle it crosses at t <= t_max, as
        (offsets, hits) in CSR form: ray k's hits {t, u, v, tri} are hits[offsets[k]:offsets[k + 1]], in the last
        build's sort order (read_sorted) or, with ALLHITS_BY_T, ascending by (t, tri); offsets[n] is the total.

        `rays` as Context.query takes them.  A numpy input goes through the synchronous host entry and returns a
        uint64 (n + 1,) array and a HIT_DTYPE array of offsets[n] hits (of min(offsets[n], capacity) when `capacity`
        is given).  A torch CUDA (N, 8) tensor goes to the device entry, enqueued on `stream` as query's, and returns
        an int64 (n + 1,) device tensor and a (capacity, 4) float32 device tensor whose rows [0, min(total, capacity))
        are written: read the ids with hits[:, 3].view(torch.int32).  With `capacity` given that is one call, with no
        host copy and no synchronisation -- compare offsets[-1] with it afterwards; with capacity=None an
        ALLHITS_SIZES call, one .item() read of the total (the only synchronisation) and an ALLHITS_FILL call.
        sizes_only=True returns the offsets alone (crossing parity needs no hits).  mode: ALLHITS_SORT,
        ALLHITS_COUNT, ALLHITS_BY_T (ALLHITS_SIZES and ALLHITS_FILL are this method's to set).  ValueError for a
        wrong shape, dtype, device or layout."""
        kind, rays = check_query_rays(rays, getattr(self, "device", None))
        if mode & (_L.ALLHITS_SIZES | _L.ALLHITS_FILL):
            raise ValueError("allhits: ALLHITS_SIZES and ALLHITS_FILL are set by allhits itself")
        if mode & ~(_L.ALLHITS_SORT | _L.ALLHITS_COUNT | _L.ALLHITS_BY_T):
            raise ValueError(f"allhits: unknown mode bits {mode:#x}")
        if capacity is not None and (int(capacity) != capacity or capacity < 0):
            raise ValueError(f"allhits: capacity must be a non-negative integer, got {capacity!r}")
        if sizes_only and (capacity is not None or mode & _L.ALLHITS_BY_T):
            raise ValueError("allhits: sizes_only takes no capacity and no ALLHITS_BY_T")
        L = _L.lib()
        return self._lists(L.rtbvh_allhits_host, L.rtbvh_allhits_async, rays, len(rays), _L.HIT_DTYPE, (4,), "float32",
                           _L.ALLHITS_SIZES, _L.ALLHITS_FILL, mode, mode & ~_L.ALLHITS_BY_T, capacity, sizes_only,
                           stream)

    def allhits_counts(self) -> dict:
        """rtbvh_allhits_counts: rays, hits (the total), internal-node and leaf steps (summed over the passes) of
        the last ALLHITS_COUNT query (the other queries' counts are kept apart)."""
        return self._counts("allhits", ("rays", "hits", "internal_steps", "leaf_steps"))

    # -- first-k ray queries --
    def khits(self, rays, k, mode: int = 0, out=None, stream=None):
        """rtbvh_khits_async / rtbvh_khits_host: for each ray its k nearest crossings -- of the members
        Context.allhits lists, the k with the smallest (max(t, the leaf box's slab entry), triangle id), ascending,
        each as the genuine {t, u, v, tri}; a slot past the number found holds the miss t = -1, tri = 0xFFFFFFFF.
        k: 1 .. KHITS_MAX_K.

        `rays` as Context.query takes them.  A numpy input goes through the synchronous host entry and returns an
        (n, k) HIT_DTYPE array.  A torch CUDA (N, 8) tensor goes to the device entry with no host copy and no
        synchronisation, enqueued on `stream` as query's, and returns an (n, k, 4) float32 device tensor
        {t, u, v, tri}: read the ids with out[..., 3].view(torch.int32) (a miss: -1).  `out` receives the lists when
        given.  mode: KHITS_SORT, KHITS_COUNT.  ValueError for a bad k and for a wrong shape, dtype, device or
        layout."""
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= _L.KHITS_MAX_K:
            raise ValueError(f"khits: k must be an integer from 1 to {_L.KHITS_MAX_K}, got {k!r}")
        k = int(k)
        kind, rays = check_query_rays(rays, getattr(self, "device", None))
        n = len(rays)
        if kind == "numpy":
            if out is None:
                out = np.zeros((n, k), _L.HIT_DTYPE)
            elif not (isinstance(out, np.ndarray) and out.dtype == _L.HIT_DTYPE and out.shape == (n, k) and
                      out.flags["C_CONTIGUOUS"]):
                raise ValueError(f"khits: out must be a contiguous ({n}, {k}) HIT_DTYPE array")
            self._check(_L.lib().rtbvh_khits_host(self._h, ctypes.c_void_p(rays.ctypes.data), n, k,
                                                  ctypes.c_void_p(out.ctypes.data), mode))
            return out
        import torch
        if out is None:
            out = torch.empty((n, k, 4), dtype=torch.float32, device=rays.device)
        elif not (_is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (n, k, 4) and
                  out.device == rays.device and out.is_contiguous()):
            raise ValueError(f"khits: out must be a contiguous ({n}, {k}, 4) float32 tensor on {rays.device}")
        self._async(_L.lib().rtbvh_khits_async, stream, rays.device, ctypes.c_void_p(rays.data_ptr()), n, k,
                    ctypes.c_void_p(out.data_ptr()), mode)
        return out

    def khits_counts(self) -> dict:
        """rtbvh_khits_counts: rays, hits found, internal-node and leaf steps of the last KHITS_COUNT query (the other
        queries' counts are kept apart)."""
        return self._counts("khits", ("rays", "found", "internal_steps", "leaf_steps"))

    # -- box-overlap queries --
    def overlap(self, boxes, hi=None, mode: int = 0, capacity=None, sizes_only: bool = False, stream=None):
        """rtbvh_overlap_async / rtbvh_overlap_host: for each axis-aligned box every triangle whose leaf box meets it
        (closed intervals) and, with OVERLAP_TRIANGLE, that also passes the header's triangle-box test, as
        (offsets, ids) in CSR form: box k's triangle ids are ids[offsets[k]:offsets[k + 1]], in the last build's sort
        order (read_sorted), and offsets[n] is the total.

        `boxes`: make_boxes' output, or (N, 3) float32 lower corners with `hi` the upper ones (numpy).  A numpy input
        goes through the synchronous host entry and returns a uint64 (n + 1,) array and a uint32 array of offsets[n]
        ids (of min(offsets[n], capacity) when `capacity` is given).  A torch CUDA (N, 8) tensor goes to the device
        entry, enqueued on `stream` as nearest's, and returns an int64 (n + 1,) device tensor and an int32
        (capacity,) device tensor whose entries [0, min(total, capacity)) are written.  With `capacity` given that
        is one call, with no host copy and no synchronisation -- compare offsets[-1] with it afterwards; with
        capacity=None an OVERLAP_SIZES call, one .item() read of the total (the only synchronisation) and an
        OVERLAP_FILL call.  sizes_only=True returns the offsets alone.  mode: OVERLAP_SORT, OVERLAP_COUNT,
        OVERLAP_TRIANGLE (OVERLAP_SIZES and OVERLAP_FILL are this method's to set).  ValueError for a wrong shape,
        dtype, device or layout."""
        kind, bx = check_overlap_boxes(boxes, hi, getattr(self, "device", None))
        if mode & (_L.OVERLAP_SIZES | _L.OVERLAP_FILL):
            raise ValueError("overlap: OVERLAP_SIZES and OVERLAP_FILL are set by overlap itself")
        if mode & ~(_L.OVERLAP_SORT | _L.OVERLAP_COUNT | _L.OVERLAP_TRIANGLE):
            raise ValueError(f"overlap: unknown mode bits {mode:#x}")
        if capacity is not None and (int(capacity) != capacity or capacity < 0):
            raise ValueError(f"overlap: capacity must be a non-negative integer, got {capacity!r}")
        if sizes_only and capacity is not None:
            raise ValueError("overlap: sizes_only takes no capacity")
        L = _L.lib()
        return self._lists(L.rtbvh_overlap_host, L.rtbvh_overlap_async, bx, len(bx), np.uint32, (), "int32",
                           _L.OVERLAP_SIZES, _L.OVERLAP_FILL, mode, mode, capacity, sizes_only, stream)

    def overlap_counts(self) -> dict:
        """rtbvh_overlap_counts: boxes, ids (the total), internal-node and leaf steps (summed over the passes) of
        the last OVERLAP_COUNT query (the other queries' counts are kept apart)."""
        return self._counts("overlap", ("boxes", "ids", "internal_steps", "leaf_steps"))

    # -- region queries --
    def region(self, regions, mode: int = 0, capacity=None, sizes_only: bool = False, stream=None):
        """rtbvh_region_async / rtbvh_region_host: for each region of up to six planes every triangle whose leaf box
        reaches the inner side of every plane and, with REGION_TRIANGLE, that has on every plane a vertex on the
        inner side (the header's conservative vertex test; exact for a slab), as (offsets, ids) in CSR form: region
        k's triangle ids are ids[offsets[k]:offsets[k + 1]], in the last build's sort order (read_sorted), and
        offsets[n] is the total.

        `regions`: make_regions' / box_region's / slab_region's output, or (N, P <= 6, 4) float32 planes (numpy).
        Inputs, outputs, `capacity`, `sizes_only` and `stream` are Context.overlap's: numpy goes through the
        synchronous host entry, a torch CUDA (N, 24) tensor to the device entry.  mode: REGION_COUNT,
        REGION_TRIANGLE, REGION_NO_ACCEPT, and region_split(k) or REGION_SPLIT_AUTO: the same lists with each region
        cut into pieces along the tree and walked by many lanes -- for few, large regions (REGION_SIZES and
        REGION_FILL are this method's to set).  ValueError for a wrong shape, dtype, device or layout."""
        kind, rg = check_region_planes(regions, getattr(self, "device", None))
        if mode & (_L.REGION_SIZES | _L.REGION_FILL):
            raise ValueError("region: REGION_SIZES and REGION_FILL are set by region itself")
        if mode & ~(_L.REGION_COUNT | _L.REGION_TRIANGLE | _L.REGION_NO_ACCEPT | _L.REGION_SPLIT_AUTO):
            raise ValueError(f"region: unknown mode bits {mode:#x}")
        if (mode >> _L.REGION_SPLIT_SHIFT) & 15 in (13, 14):
            raise ValueError(f"region: split field {(mode >> _L.REGION_SPLIT_SHIFT) & 15} (region_split, REGION_SPLIT_AUTO)")
        if capacity is not None and (int(capacity) != capacity or capacity < 0):
            raise ValueError(f"region: capacity must be a non-negative integer, got {capacity!r}")
        if sizes_only and capacity is not None:
            raise ValueError("region: sizes_only takes no capacity")
        L = _L.lib()
        return self._lists(L.rtbvh_region_host, L.rtbvh_region_async, rg, len(rg), np.uint32, (), "int32",
                           _L.REGION_SIZES, _L.REGION_FILL, mode, mode, capacity, sizes_only, stream)

    def region_counts(self) -> dict:
        """rtbvh_region_counts: regions, ids (the total), internal-node steps, leaf steps and subtrees taken whole
        (summed over the passes) and the ids that came from those subtrees, of the last REGION_COUNT query (the
        other queries' counts are kept apart)."""
        return self._counts("region",
                            ("regions", "ids", "internal_steps", "leaf_steps", "accepted_subtrees", "accepted_ids"))

    def region_split_counts(self) -> dict:
        """rtbvh_region_split_counts: of the last REGION_COUNT query with a split field, the K used (1: the plain
        path ran), the non-empty pieces, the node tests of the expansion and the longest single piece walk in
        steps."""
        return self._counts("region_split", ("k", "pieces", "expansion_tests", "longest_piece_steps"))

    # -- self-collision queries --
    def collide(self, mode: int = 0, capacity=None, sizes_only: bool = False, stream=None, device: bool = False):
        """rtbvh_collide_async / rtbvh_collide_host: the pairs of the built mesh's own triangles whose leaf boxes meet
        and that share no vertex index and, with COLLIDE_TRIANGLE, that cross each other (the header's six
        segment-triangle tests), as (offsets, ids) in CSR form over the T triangles: triangle i's partners are
        ids[offsets[i]:offsets[i + 1]], in the last build's sort order (read_sorted), and offsets[T] is the total.  A
        pair is listed once, by the triangle that comes earlier in that order; with COLLIDE_SYMMETRIC by both.

        device=False goes through the synchronous host entry and returns a uint64 (T + 1,) array and a uint32 array
        of offsets[T] ids (of min(offsets[T], capacity) when `capacity` is given).  device=True goes to the device
        entry, enqueued on `stream` as overlap's, and returns an int64 (T + 1,) device tensor and an int32
        (capacity,) device tensor whose entries [0, min(total, capacity)) are written.  With `capacity` given that
        is one call, with no host copy and no synchronisation -- compare offsets[-1] with it afterwards; with
        capacity=None a COLLIDE_SIZES call, one .item() read of the total (the only synchronisation) and a
        COLLIDE_FILL call.  sizes_only=True returns the offsets alone.  mode: COLLIDE_COUNT, COLLIDE_TRIANGLE,
        COLLIDE_SYMMETRIC (COLLIDE_SIZES and COLLIDE_FILL are this method's to set)."""
        if mode & (_L.COLLIDE_SIZES | _L.COLLIDE_FILL):
            raise ValueError("collide: COLLIDE_SIZES and COLLIDE_FILL are set by collide itself")
        if mode & ~(_L.COLLIDE_COUNT | _L.COLLIDE_TRIANGLE | _L.COLLIDE_SYMMETRIC):
            raise ValueError(f"collide: unknown mode bits {mode:#x}")
        if capacity is not None and (int(capacity) != capacity or capacity < 0):
            raise ValueError(f"collide: capacity must be a non-negative integer, got {capacity!r}")
        if sizes_only and capacity is not None:
            raise ValueError("collide: sizes_only takes no capacity")
        if not device and stream is not None:
            raise ValueError("collide: a stream goes with device=True")
        L = _L.lib()
        return self._lists(L.rtbvh_collide_host, L.rtbvh_collide_async, None, self.num_tris, np.uint32, (), "int32",
                           _L.COLLIDE_SIZES, _L.COLLIDE_FILL, mode, mode, capacity, sizes_only, stream,
                           on_device=device)

    def collide_pairs(self, triangle: bool = True) -> np.ndarray:
        """The member pairs as a (P, 2) uint32 array of triangle ids (i, j), expanded from collide()'s default CSR
        form: row by row the owner i (the earlier triangle in the build's sort order) and one of its partners j."""
        offsets, ids = self.collide(_L.COLLIDE_TRIANGLE if triangle else 0)
        owner = np.repeat(np.arange(len(offsets) - 1, dtype=np.uint32), np.diff(offsets).astype(np.int64))
        return np.stack([owner, ids], 1)

    def collide_counts(self) -> dict:
        """rtbvh_collide_counts: triangles, entries (the total), internal-node and leaf steps (summed over the
        passes) of the last COLLIDE_COUNT query (the other queries' counts are kept apart)."""
        return self._counts("collide", ("triangles", "entries", "internal_steps", "leaf_steps"))

    # -- triangle queries --
    def cross(self, tris, mode: int = 0, capacity=None, sizes_only: bool = False, stream=None):
        """rtbvh_cross_async / rtbvh_cross_host: for each query triangle every scene triangle whose leaf box meets the
        query's box (closed intervals) and that crosses it (the header's six segment-triangle tests), as
        (offsets, ids) in CSR form: query k's triangle ids are ids[offsets[k]:offsets[k + 1]], in the last build's sort
        order (read_sorted), and offsets[n] is the total.

        `tris`: make_tris' output.  A numpy input goes through the synchronous host entry and returns a uint64
        (n + 1,) array and a uint32 array of offsets[n] ids (of min(offsets[n], capacity) when `capacity` is given).
        A torch CUDA (N, 12) tensor goes to the device entry, enqueued on `stream` as nearest's, and returns an int64
        (n + 1,) device tensor and an int32 (capacity,) device tensor whose entries [0, min(total, capacity)) are
        written.  With `capacity` given that is one call, with no host copy and no synchronisation -- compare
        offsets[-1] with it afterwards; with capacity=None a CROSS_SIZES call, one .item() read of the total (the
        only synchronisation) and a CROSS_FILL call.  sizes_only=True returns the offsets alone.  mode: CROSS_SORT,
        CROSS_COUNT (CROSS_SIZES and CROSS_FILL are this method's to set).  ValueError for a wrong shape, dtype,
        device or layout."""
        kind, tr = check_cross_tris(tris, getattr(self, "device", None))
        if mode & (_L.CROSS_SIZES | _L.CROSS_FILL):
            raise ValueError("cross: CROSS_SIZES and CROSS_FILL are set by cross itself")
        if mode & ~(_L.CROSS_SORT | _L.CROSS_COUNT):
            raise ValueError(f"cross: unknown mode bits {mode:#x}")
        if capacity is not None and (int(capacity) != capacity or capacity < 0):
            raise ValueError(f"cross: capacity must be a non-negative integer, got {capacity!r}")
        if sizes_only and capacity is not None:
            raise ValueError("cross: sizes_only takes no capacity")
        if kind == "numpy" and stream is not None:
            raise ValueError("cross: a stream goes with a torch tensor of triangles")
        L = _L.lib()
        return self._lists(L.rtbvh_cross_host, L.rtbvh_cross_async, tr, len(tr), np.uint32, (), "int32",
                           _L.CROSS_SIZES, _L.CROSS_FILL, mode, mode, capacity, sizes_only, stream)

    def cross_first(self, tris, mode: int = 0, out=None, stream=None):
        """rtbvh_cross_first_async / rtbvh_cross_first_host: for each query triangle the first id of its cross() list
        -- the member at the lowest position of the build's sort order -- or 0xFFFFFFFF (-1 in a tensor) when it
        crosses nothing; one pass whose walks end at their first member.  `tris` as cross takes them: a numpy input
        returns a uint32 (N,) array through the synchronous host entry, a torch CUDA tensor an int32 (N,) device
        tensor, enqueued on `stream` as nearest's with no synchronisation.  `out` receives the results when given.
        mode: CROSS_SORT, CROSS_COUNT."""
        kind, tr = check_cross_tris(tris, getattr(self, "device", None))
        if mode & ~(_L.CROSS_SORT | _L.CROSS_COUNT):
            raise ValueError(f"cross_first: mode takes CROSS_SORT and CROSS_COUNT only, got {mode:#x}")
        n = len(tr)
        if kind == "numpy":
            if stream is not None:
                raise ValueError("cross_first: a stream goes with a torch tensor of triangles")
            if out is None:
                out = np.zeros(n, np.uint32)
            elif not (isinstance(out, np.ndarray) and out.dtype == np.uint32 and out.shape == (n,) and
                      out.flags["C_CONTIGUOUS"]):
                raise ValueError(f"cross_first: out must be a contiguous uint32 array of {n} ids")
            self._check(_L.lib().rtbvh_cross_first_host(self._h, ctypes.c_void_p(tr.ctypes.data), n,
                                                        ctypes.c_void_p(out.ctypes.data), mode))
            return out
        import torch
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=tr.device)
        elif not (_is_tensor(out) and out.dtype == torch.int32 and tuple(out.shape) == (n,) and
                  out.device == tr.device and out.is_contiguous()):
            raise ValueError(f"cross_first: out must be a contiguous ({n},) int32 tensor on {tr.device}")
        self._async(_L.lib().rtbvh_cross_first_async, stream, tr.device, ctypes.c_void_p(tr.data_ptr()), n,
                    ctypes.c_void_p(out.data_ptr()), mode)
        return out

    def cross_pairs(self, tris) -> np.ndarray:
        """The members as a (P, 2) uint32 array of rows (query, triangle id), expanded from cross()'s CSR form: query
        by query, each list in the build's sort order (a CUDA tensor of triangles is read back)."""
        offsets, ids = self.cross(tris)
        if _is_tensor(offsets):
            offsets, ids = offsets.cpu().numpy().astype(np.uint64), ids.cpu().numpy().view(np.uint32)
        owner = np.repeat(np.arange(len(offsets) - 1, dtype=np.uint32), np.diff(offsets).astype(np.int64))
        return np.stack([owner, ids], 1)

    def cross_counts(self) -> dict:
        """rtbvh_cross_counts: queries, ids (the total; for cross_first the queries with a member), internal-node and
        leaf steps (summed over the passes) of the last CROSS_COUNT query (the other queries' counts are kept
        apart)."""
        return self._counts("cross", ("queries", "ids", "internal_steps", "leaf_steps"))

    # -- clearance queries --
    def clearance(self, tris, max_dist2=float("inf"), mode: int = 0, stream=None):
        """rtbvh_clearance_async / rtbvh_clearance_host: for each query triangle the nearest scene triangle within
        max_dist2 (one bound for the call), the squared distance -- 0 where the two cross, as cross() decides it --
        and the two witness points, in the space the BVH was built in.

        A numpy input -- (N, 3, 3) or (N, 9) vertices, packed by make_tris, or what cross() takes -- goes through the
        synchronous host entry and returns a CLEARANCE_DTYPE array (no result: dist2 = -1, tri = 0xFFFFFFFF).  A
        torch CUDA (N, 12) tensor (make_tris) goes to the device entry, enqueued on `stream` as nearest's with no host
        copy and no synchronisation, and returns an (N, 8) float32 device tensor {point_q, dist2, point_x, tri}: read
        the triangle ids with out[:, 7].view(torch.int32) (no result: -1).  mode: CLEARANCE_SORT, CLEARANCE_COUNT.
        ValueError for a wrong shape, dtype, device or layout."""
        if isinstance(tris, np.ndarray) and tris.dtype != _L.TRI_DTYPE and (
                (tris.ndim == 3 and tris.shape[1:] == (3, 3)) or (tris.ndim == 2 and tris.shape[1] == 9)):
            tris = make_tris(tris)
        kind, tr = check_cross_tris(tris, getattr(self, "device", None))
        if mode & ~(_L.CLEARANCE_SORT | _L.CLEARANCE_COUNT):
            raise ValueError(f"clearance: mode takes CLEARANCE_SORT and CLEARANCE_COUNT only, got {mode:#x}")
        try:
            bound = ctypes.c_float(max_dist2)
        except TypeError:
            raise ValueError(f"clearance: max_dist2 must be one number, got {max_dist2!r}") from None
        n = len(tr)
        if kind == "numpy":
            if stream is not None:
                raise ValueError("clearance: a stream goes with a torch tensor of triangles")
            out = np.zeros(n, _L.CLEARANCE_DTYPE)
            self._check(_L.lib().rtbvh_clearance_host(self._h, ctypes.c_void_p(tr.ctypes.data), n, bound,
                                                      ctypes.c_void_p(out.ctypes.data), mode))
            return out
        import torch
        out = torch.empty((n, 8), dtype=torch.float32, device=tr.device)
        self._async(_L.lib().rtbvh_clearance_async, stream, tr.device, ctypes.c_void_p(tr.data_ptr()), n, bound,
                    ctypes.c_void_p(out.data_ptr()), mode)
        return out

    def clearance_counts(self) -> dict:
        """rtbvh_clearance_counts: queries, results found, internal-node and leaf steps of the last CLEARANCE_COUNT
        query (the other queries' counts are kept apart)."""
        return self._counts("clearance", ("queries", "found", "internal_steps", "leaf_steps"))

    # -- sphere-sweep queries --
    def sweep(self, sweeps, mode: int = 0, stream=None):
        """rtbvh_sweep_async / rtbvh_sweep_host: for each sphere sweep (make_sweeps: a sphere of a radius moving from
        an origin along a direction, up to t_max) its first contact with the mesh -- t, the contact point on the
        triangle, the triangle and the feature touched (1 overlapping at the start, 2 the face, 3..5 an edge, 6..8 a
        vertex) -- in the space the BVH was built in (include/rtbvh.h).

        An (N, 8) float32 contiguous CUDA tensor on the context's device goes to the device entry with no host copy
        and no synchronisation, enqueued on `stream` (a torch stream or a hipStream_t handle; default: the current
        torch stream; torch's legacy default stream as in query), and returns an (N, 8) float32 device tensor
        {t, point, tri, feature, 0, 0}: read the ids with out[:, 4].view(torch.int32) (a miss: t = -1, tri = -1,
        feature = 0).  A SWEEP_DTYPE or (N, 8) float32 numpy array goes through the synchronous host entry and
        returns a SWEEP_HIT_DTYPE array.  mode: SWEEP_ANY, SWEEP_SORT, SWEEP_COUNT.  ValueError for a wrong shape,
        dtype, device or layout."""
        kind, sw = check_sweeps(sweeps, getattr(self, "device", None))
        n = len(sw)
        if kind == "numpy":
            out = np.zeros(n, _L.SWEEP_HIT_DTYPE)
            self._check(_L.lib().rtbvh_sweep_host(self._h, ctypes.c_void_p(sw.ctypes.data), n,
                                                  ctypes.c_void_p(out.ctypes.data), mode))
            return out
        import torch
        out = torch.empty((n, 8), dtype=torch.float32, device=sw.device)
        self._async(_L.lib().rtbvh_sweep_async, stream, sw.device, ctypes.c_void_p(sw.data_ptr()), n,
                    ctypes.c_void_p(out.data_ptr()), mode)
        return out

    def sweep_counts(self) -> dict:
        """rtbvh_sweep_counts: sweeps, hits, internal-node and leaf steps of the last SWEEP_COUNT query (the other
        queries' counts are kept apart)."""
        return self._counts("sweep", ("sweeps", "hits", "internal_steps", "leaf_steps"))

    # -- signed-distance queries --
    def signed(self, points, max_dist2=None, mode: int = 0, out=None, stream=None):
        """rtbvh_signed_async / rtbvh_signed_host: for each point Context.nearest's fields and `flags`, the crossing
        counts of one ray from the point (three with SIGNED_VOTE3) along fixed directions: bit 0 inside (an odd
        count; with VOTE3 two of three), bits 1..3 each ray's parity, bytes 1..3 each ray's count saturated at 255
        (include/rtbvh.h).  The rays are cast whatever the bound: max_dist2 limits the nearest fields only, and
        SIGNED_INSIDE_ONLY skips the closest-point walk (the nearest fields are then "no result").

        `points` as Context.nearest takes them (max_dist2 None: no limit).  A numpy input goes through the
        synchronous host entry and returns a SIGNED_DTYPE array.  A torch CUDA (N, 4) tensor goes to the device
        entry with no host copy and no synchronisation, enqueued on `stream` as nearest's, and returns an (N, 8)
        float32 device tensor {point, dist2, u, v, tri, flags}: read the flags with out[:, 7].view(torch.int32).
        `out` receives the records when given.  mode: SIGNED_SORT, SIGNED_COUNT, SIGNED_VOTE3, SIGNED_INSIDE_ONLY.
        ValueError for a wrong shape, dtype, device or layout."""
        kind, pts = check_nearest_points(points, float("inf") if max_dist2 is None else max_dist2,
                                         getattr(self, "device", None))
        n = len(pts)
        if kind == "numpy":
            if out is None:
                out = np.zeros(n, _L.SIGNED_DTYPE)
            elif not (isinstance(out, np.ndarray) and out.dtype == _L.SIGNED_DTYPE and out.shape == (n,) and
                      out.flags["C_CONTIGUOUS"]):
                raise ValueError(f"signed: out must be a contiguous SIGNED_DTYPE array of {n} records")
            self._check(_L.lib().rtbvh_signed_host(self._h, ctypes.c_void_p(pts.ctypes.data), n,
                                                   ctypes.c_void_p(out.ctypes.data), mode))
            return out
        import torch
        if out is None:
            out = torch.empty((n, 8), dtype=torch.float32, device=pts.device)
        elif not (_is_tensor(out) and out.dtype == torch.float32 and tuple(out.shape) == (n, 8) and
                  out.device == pts.device and out.is_contiguous()):
            raise ValueError(f"signed: out must be a contiguous ({n}, 8) float32 tensor on {pts.device}")
        self._async(_L.lib().rtbvh_signed_async, stream, pts.device, ctypes.c_void_p(pts.data_ptr()), n,
                    ctypes.c_void_p(out.data_ptr()), mode)
        return out

    @staticmethod
    def _torch_stream(stream, device):
        """`stream` as a torch stream: itself, a raw handle wrapped, or (None) the current stream."""
        import torch
        if stream is None:
            return torch.cuda.current_stream(device)
        if hasattr(stream, "cuda_stream"):
            return stream
        return torch.cuda.ExternalStream(int(stream), device=device) if int(stream) else torch.cuda.default_stream(device)

    def _signed_on_stream(self, pts, mode, stream, read):
        """signed() of checked device points into a record tensor that lives on `stream`, and read(record) there.
        The temporary is allocated under the stream it is used on, so torch's allocator hands its block to nothing
        that could run before the work enqueued here is done."""
        import torch
        ts = self._torch_stream(stream, pts.device)
        with torch.cuda.stream(ts):
            rec = torch.empty((len(pts), 8), dtype=torch.float32, device=pts.device)
            self.signed(pts, None, mode, out=rec, stream=ts)
            return read(rec)

    def signed_distance(self, points, max_dist2=None, mode: int = 0, stream=None):
        """The signed distance of each point, float32: sqrt(dist2) of Context.signed's record, negative where its
        `inside` bit is set, NaN where there is no nearest result.  A numpy array for numpy points; for a CUDA
        tensor an (N,) device tensor computed on `stream`, with no synchronisation.  Distances are object-space
        distances under an identity WVP only (Context.nearest)."""
        mode = mode & ~_L.SIGNED_INSIDE_ONLY
        if _is_tensor(points):
            import torch
            _, pts = check_nearest_points(points, float("inf") if max_dist2 is None else max_dist2,
                                          getattr(self, "device", None))

            def read(rec):
                d2 = rec[:, 3]
                d = torch.where(d2 < 0, torch.full_like(d2, float("nan")), torch.sqrt(d2.clamp(min=0)))
                inside = (rec[:, 7].contiguous().view(torch.int32) & 1) != 0
                return torch.where(inside, -d, d)
            return self._signed_on_stream(pts, mode, stream, read)
        rec = self.signed(points, max_dist2, mode)
        with np.errstate(invalid="ignore"):
            d = np.where(rec["tri"] == 0xFFFFFFFF, np.float32(np.nan), np.sqrt(rec["dist2"]))
        return np.where(rec["flags"] & 1, -d, d).astype(np.float32)

    def inside(self, points, vote3: bool = False, mode: int = 0, stream=None):
        """Whether each point is inside the (closed) surface: the `inside` bit of a SIGNED_INSIDE_ONLY query, one
        ray, or the majority of three with vote3.  A bool array for numpy points, a bool device tensor for a CUDA
        tensor (on `stream`, no synchronisation)."""
        mode = mode | _L.SIGNED_INSIDE_ONLY | (_L.SIGNED_VOTE3 if vote3 else 0)
        if _is_tensor(points):
            import torch
            _, pts = check_nearest_points(points, float("inf"), getattr(self, "device", None))
            return self._signed_on_stream(pts, mode, stream,
                                          lambda rec: (rec[:, 7].contiguous().view(torch.int32) & 1) != 0)
        return (self.signed(points, None, mode)["flags"] & 1).astype(bool)

    def signed_counts(self) -> dict:
        """rtbvh_signed_counts: points, points inside, internal-node and leaf steps (summed over all the walks) of
        the last SIGNED_COUNT query (the other queries' counts are kept apart)."""
        return self._counts("signed", ("points", "inside", "internal_steps", "leaf_steps"))

    # -- outputs --
    def read_framebuffer(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._check(_L.lib().rtbvh_read_framebuffer(self._h, _L.ptr(out)))
        return out

    def read_rays(self):
        """(reflectRay, refractRay) RayPresent records of the last full-frame trace made with
        FLAG_REFRACT_RECORDS, each (H, W, 14) float32: intensity, origin, direction,
        invDirection, color (RayTraceGlobal.hlsl:30-35)."""
        refl = np.zeros((self.height, self.width, 14), np.float32)
        refr = np.zeros((self.height, self.width, 14), np.float32)
        self._check(_L.lib().rtbvh_read_rays(self._h, _L.ptr(refl), _L.ptr(refr)))
        return refl, refr

    def present(self) -> np.ndarray:
        """The image the pixel shader shows (RayTraceBVHPS.hlsl:13-16): (H, W, 4) uint8, top row first."""
        out = np.zeros((self.height, self.width, 4), np.uint8)
        self._check(_L.lib().rtbvh_present(self._h, _L.ptr(out)))
        return out

    def read_intensity(self) -> np.ndarray:
        out = np.zeros((self.height, self.width), np.float32)
        self._check(_L.lib().rtbvh_read_intensity(self._h, _L.ptr(out)))
        return out

    def framebuffer_device_ptr(self) -> int:
        return _L.lib().rtbvh_framebuffer_device(self._h) or 0

    def read_bvh(self) -> np.ndarray:
        out = np.zeros(2 * self.num_tris - 1, dtype=_L.NODE_DTYPE)
        self._check(_L.lib().rtbvh_read_bvh(self._h, ctypes.c_void_p(out.ctypes.data), len(out)))
        return out

    def read_wide(self) -> np.ndarray:
        """Node records in slots (both walks' layout): (2(n-1), 16) uint32 records, see rtbvh_read_wide."""
        out = np.zeros((max(2 * (self.num_tris - 1), 0), 16), np.uint32)
        self._check(_L.lib().rtbvh_read_wide(self._h, _L.ptr(out), len(out)))
        return out

    def read_qnodes(self) -> np.ndarray:
        """Quantized 4-wide nodes of the bounce walk in slots: (2n-1, 16) uint32, see rtbvh_read_qnodes."""
        out = np.zeros((max(2 * self.num_tris - 1, 0) if self.num_tris > 1 else 0, 16), np.uint32)
        self._check(_L.lib().rtbvh_read_qnodes(self._h, _L.ptr(out), len(out)))
        return out

    def read_walk_qnodes(self) -> np.ndarray:
        """The walk-only tree's quantized nodes, in read_qnodes' format: (2n-1, 16) uint32, see
        rtbvh_read_walk_qnodes (RtbvhError NOT_READY when the context holds none for the current build)."""
        out = np.zeros((max(2 * self.num_tris - 1, 0), 16), np.uint32)
        self._check(_L.lib().rtbvh_read_walk_qnodes(self._h, _L.ptr(out), len(out)))
        return out

    def read_morton(self) -> np.ndarray:
        out = np.zeros(self.num_tris, np.uint32)
        self._check(_L.lib().rtbvh_read_morton(self._h, _L.ptr(out)))
        return out

    def read_sorted(self):
        keys = np.zeros(self.num_tris, np.uint32)
        ids = np.zeros(self.num_tris, np.uint32)
        self._check(_L.lib().rtbvh_read_sorted(self._h, _L.ptr(keys), _L.ptr(ids)))
        return keys, ids

    def stats(self) -> dict:
        """rtbvh_get_stats: counts of the last trace; hipEvent averages since reset_stats()."""
        s = _L.Stats()
        self._check(_L.lib().rtbvh_get_stats(self._h, ctypes.byref(s)))
        return s.as_dict()

    def reset_stats(self):
        self._check(_L.lib().rtbvh_reset_stats(self._h))

    def set_flags(self, flags: int):
        self._check(_L.lib().rtbvh_set_flags(self._h, flags))

    def bin_builds(self) -> int:
        """rtbvh_bin_builds: fills of a bin set (the binned primary pass's count pass) enqueued since create."""
        return int(_L.lib().rtbvh_bin_builds(self._h))

    def bin_sets(self) -> int:
        """rtbvh_bin_sets: the bin sets the context holds in device memory."""
        return int(_L.lib().rtbvh_bin_sets(self._h))

    # -- primitives --
    def sort_pairs(self, keys: np.ndarray, vals: np.ndarray, key_bits: int = 32):
        keys = np.ascontiguousarray(keys, np.uint32)
        vals = np.ascontiguousarray(vals, np.uint32)
        ko = np.zeros_like(keys)
        vo = np.zeros_like(vals)
        self._check(_L.lib().rtbvh_sort_pairs_host(self._h, _L.ptr(keys), _L.ptr(vals), _L.ptr(ko), _L.ptr(vo),
                                                   len(keys), key_bits))
        return ko, vo

    def sort_pairs_device(self, keys_ptr: int, vals_ptr: int, keys_out_ptr: int, vals_out_ptr: int, n: int,
                          key_bits: int = 32):
        self._check(_L.lib().rtbvh_sort_pairs_async(self._h, ctypes.c_void_p(keys_ptr), ctypes.c_void_p(vals_ptr),
                                                    ctypes.c_void_p(keys_out_ptr), ctypes.c_void_p(vals_out_ptr),
                                                    n, key_bits))

    def build_from_codes(self, sorted_codes: np.ndarray, leaf_boxes: np.ndarray) -> np.ndarray:
        codes = np.ascontiguousarray(sorted_codes, np.uint32)
        boxes = np.ascontiguousarray(leaf_boxes, np.float32).reshape(-1, 6)
        out = np.zeros(2 * len(codes) - 1, dtype=_L.NODE_DTYPE)
        self._check(_L.lib().rtbvh_build_from_codes(self._h, _L.ptr(codes), _L.ptr(boxes), len(codes),
                                                    ctypes.c_void_p(out.ctypes.data)))
        return out


class Graphics:
    """Graphics : Manager (Graphics.h:16-27) over librtbvh.so.

    onInit(scene)  ~ Graphics::onInit -> loadAssets (Graphics.cpp:34-38, 237-665)
    onUpdate()     ~ Graphics::onUpdate: camera + computeBVH (Graphics.cpp:40-61)
    computeBVH()   ~ Graphics::computeBVH (Graphics.cpp:667-831)
    """

    def __init__(self, width: int = 800, height: int = 800, bounces: int = 3, **ctx_kwargs):
        # main.cpp:7 opens an 800x800 window; Graphics.cpp:795 runs 3 reflection passes
        self.width, self.height, self.bounces = width, height, bounces
        self.eye = np.array(EYE_REFERENCE, np.float32)   # Graphics.h:200-205
        self.ctx = Context(**ctx_kwargs)

    def onInit(self, scene: Scene):  # noqa: N802
        self.ctx.set_scene(scene)

    def onUpdate(self):  # noqa: N802
        wvp, wv = camera_look(self.eye, self.width, self.height)
        self.ctx.set_camera(wvp, wv)
        self.computeBVH()

    def onKeyDown(self, key: int):  # noqa: N802
        """Graphics::onKeyDown (Graphics.cpp:937-960): KEY_LEFT/RIGHT/UP/DOWN orbit the eye about the origin."""
        self.eye = camera_orbit(self.eye, key)

    def computeBVH(self):  # noqa: N802
        self.ctx.compute_bvh(self.width, self.height, self.bounces)

    def framebuffer(self) -> np.ndarray:
        """reflectRay[].color as (H, W, 4) f32 (the framebuffer of record, RayTraceBVHPS.hlsl:13-16)."""
        return self.ctx.read_framebuffer()

    def onRender(self) -> np.ndarray:  # noqa: N802
        """Graphics::onRender's frame (the presentation pass) as RGBA8."""
        return self.ctx.present()

    def save_bmp(self, path: str):
        """SaveBMP (SaveBMP.cpp:3-62) of the presented frame."""
        save_bmp(path, self.onRender())

    def onDestroy(self):  # noqa: N802
        self.ctx.close()


def comm_unique_id() -> bytes:
    """rtbvh_comm_unique_id: the 128-B RCCL id rank 0 creates and shares with every rank."""
    buf = (ctypes.c_uint8 * _L.COMM_ID_BYTES)()
    _L.check(_L.lib().rtbvh_comm_unique_id(buf))
    return bytes(buf)


def comm_destroy(comm: int):
    """rtbvh_comm_destroy."""
    _L.check(_L.lib().rtbvh_comm_destroy(ctypes.c_void_p(comm)))


def save_bmp(path: str, rgba8: np.ndarray):
    """rtbvh_save_bmp: 24-bit BMP of an (H, W, 4) uint8 image, top row first."""
    img = np.ascontiguousarray(rgba8, dtype=np.uint8)
    _L.check(_L.lib().rtbvh_save_bmp(os.fsencode(path), _L.ptr(img), img.shape[1], img.shape[0]))
