"""Level-set crossings of the density field of K neighbour Gaussians along rays -- the stage of the Frosting pipeline
between a trained coarse model and its shell.

``level_points_along_normals`` replaces ``compute_level_points_along_normals`` (frosting_scene/frosting_model.py:2016-2208,
called at :313 and :346: the inner and outer thickness of the shell at every vertex) and ``level_surface_points_from_rays``
replaces ``compute_level_surface_points_and_range_from_camera`` from ``all_world_points`` onward (:1870-2011, called once per
training camera by frosting_extractors/coarse_shell.py:325; ``SuGaR.compute_level_surface_points_from_camera_fast``,
sugar_model.py:1885, is the same without the inner point).  Both walk n samples of a line through the density of K
neighbour Gaussians and search it for a level; the reference gathers a [samples, K, 3, 3] tensor per pass of 2 000 000
samples for that.  Here one native call (csrc/levelset.hip, ``ray_level_crossings``) loads every neighbour record once per
ray, keeps the n densities in registers and does the search and the interpolation in the same lane.

Forward only (the reference runs under ``torch.no_grad()``), float32, GPU only, K <= 32, 2 <= n <= 32, at most 8 levels.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .knn import knn_points

MAX_K = 32              # FRG_KNN_MAX_K
MAX_SAMPLES = 32        # FRG_LEVELSET_MAX_SAMPLES
MAX_LEVELS = 8          # FRG_LEVELSET_MAX_LEVELS
INNER_MODES = {"last": 0, "second_crossing": 1}     # FRG_LEVELSET_INNER_*


def quaternion_invert(q):
    """pytorch3d.transforms.quaternion_invert: the conjugate (real part first)."""
    return q * q.new_tensor([1, -1, -1, -1])


def _quaternion_raw_multiply(a, b):
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    ow = aw * bw - ax * bx - ay * by - az * bz
    ox = aw * bx + ax * bw + ay * bz - az * by
    oy = aw * by - ax * bz + ay * bw + az * bx
    oz = aw * bz + ax * by - ay * bx + az * bw
    return torch.stack((ow, ox, oy, oz), -1)


def quaternion_apply(q, v):
    """pytorch3d.transforms.quaternion_apply: q (0, v) q*, the quaternion as given (no normalisation)."""
    vq = torch.cat((v.new_zeros(v.shape[:-1] + (1,)), v), -1)
    return _quaternion_raw_multiply(_quaternion_raw_multiply(q, vq), quaternion_invert(q))[..., 1:]


def _f32(t):
    return t.detach().contiguous().float()


def ray_level_crossings(origins, directions, t_scale, t_offset, lin, idx, points, scaling, quaternions, strengths, levels,
                        density_factor=1.0, inner_mode="last", return_normals=False, return_densities=False, validate_idx=True):
    """Densities of the K Gaussians ``idx [R,K]`` names at the n samples ``origins + (lin[j] * t_scale + t_offset) *
    directions`` of every ray, and per level the reference's crossing search (include/frosting_rasterizer.h,
    frg_levelset).  Returns a dict: ``t_outer``, ``t_inner`` [L,R] float32, ``first_above``, ``last_above`` [L,R] int32,
    ``under_first`` [L,R] bool, and as requested ``normals`` [L,R,3] (zeros where ``first_above == 0``) and ``densities``
    [R,n].  Inputs that require a gradient are accepted; nothing returned carries one.  ``validate_idx`` reads one flag
    back from the device and raises IndexError for an index outside [0, P); such an index is never dereferenced either
    way and its pair contributes nothing."""
    tensors = (origins, directions, t_scale, t_offset, lin, idx, points, scaling, quaternions, strengths)
    if any(t.device.type != "cuda" for t in tensors):
        raise RuntimeError("frosting_amd ray_level_crossings runs on the GPU only (no CPU path)")
    if any(t.device != origins.device for t in tensors):
        raise RuntimeError("all tensors of ray_level_crossings must be on the same GPU")
    if inner_mode not in INNER_MODES:
        raise ValueError("inner_mode is 'last' or 'second_crossing'")
    R, P = int(origins.shape[0]), int(points.shape[0])
    if origins.dim() != 2 or origins.shape[1] != 3 or tuple(directions.shape) != (R, 3) or t_scale.numel() != R or t_offset.numel() != R:
        raise ValueError("origins (R, 3), directions (R, 3), t_scale (R,) and t_offset (R,) are expected")
    if points.dim() != 2 or points.shape[1] != 3 or tuple(scaling.shape) != (P, 3) or tuple(quaternions.shape) != (P, 4) or \
            strengths.numel() != P:
        raise ValueError("points (P, 3), scaling (P, 3), quaternions (P, 4) and strengths (P, 1) are expected")
    if idx.dim() != 2 or idx.shape[0] != R or idx.dtype not in (torch.int64, torch.int32):
        raise ValueError("idx must be an int64 or int32 tensor of dimensions (R, K)")
    K, n = int(idx.shape[1]), int(lin.numel())
    levels = [float(v) for v in levels]
    if K < 1 or K > MAX_K:
        raise ValueError(f"frosting_amd ray_level_crossings: K = {K} is outside 1 ... {MAX_K}")
    if n < 2 or n > MAX_SAMPLES:
        raise ValueError(f"frosting_amd ray_level_crossings: n = {n} samples is outside 2 ... {MAX_SAMPLES}")
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError(f"frosting_amd ray_level_crossings: {len(levels)} levels; 1 ... {MAX_LEVELS} are expected")
    if R > 0 and P == 0:
        raise ValueError("rays without Gaussians")
    L = len(levels)
    dev = origins.device
    ins = dict(origins=_f32(origins), directions=_f32(directions), t_scale=_f32(t_scale).reshape(R), t_offset=_f32(t_offset).reshape(R),
               lin=_f32(lin).reshape(n), idx=idx.contiguous(), points=_f32(points), scaling=_f32(scaling), quaternions=_f32(quaternions),
               strengths=_f32(strengths).reshape(P))
    new = lambda dtype, *shape: torch.empty(shape, dtype=dtype, device=dev)
    outs = dict(t_outer=new(torch.float32, L, R), t_inner=new(torch.float32, L, R), first_above=new(torch.int32, L, R),
                last_above=new(torch.int32, L, R), under_first=new(torch.uint8, L, R),
                normals=new(torch.float32, L, R, 3) if return_normals else None,
                densities=new(torch.float32, R, n) if return_densities else None)
    if R > 0:
        lib = _lib.lib()
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            ws = torch.empty(int(lib.frg_levelset_workspace_bytes(P, R, K, 0)) + 256, dtype=torch.uint8, device=dev)
            base = (ws.data_ptr() + 255) // 256 * 256
            a = _lib.LevelsetArgs(struct_size=C.sizeof(_lib.LevelsetArgs), P=P, R=R, K=K, n=n, L=L,
                                  idx_is_int64=int(idx.dtype == torch.int64), inner_mode=INNER_MODES[inner_mode],
                                  levels=(C.c_double * 8)(*levels), density_factor=float(density_factor),
                                  bad_index=bad.data_ptr(), workspace=base, workspace_bytes=ws.numel() - (base - ws.data_ptr()),
                                  hip_stream=stream.cuda_stream,
                                  **{k: v.data_ptr() for k, v in ins.items()},
                                  **{k: (v.data_ptr() if v is not None else None) for k, v in outs.items()})
            rc = lib.frg_levelset(C.byref(a))
            ws.record_stream(stream)
        _lib.check(rc, "frg_levelset")
        if validate_idx and int(bad.item()):
            raise IndexError(f"frosting_amd ray_level_crossings: idx holds an entry outside 0 ... {P - 1}")
    outs["under_first"] = outs["under_first"].bool()
    return {k: v for k, v in outs.items() if v is not None}


def level_points_along_normals(points, scaling, quaternions, strengths, mesh_verts, mesh_verts_normals, inner_range, outer_range,
                               n_samples_per_vertex=21, n_closest_gaussians_to_use=16, level=0.1, smooth_points=True,
                               n_neighbors_for_smoothing=4, use_last_intersection_as_inner_level_point=True,
                               min_clamping_inner_dist=None, max_clamping_outer_dist=None, min_layer_size=0.0, spatial_extent=None):
    """``compute_level_points_along_normals`` (frosting_model.py:2071-2208) on the model's tensors -- ``points``,
    ``scaling``, ``quaternions``, ``strengths`` of a SuGaR model, or ``get_xyz``, ``get_scaling``, ``get_rotation``,
    ``get_opacity`` of a vanilla 3DGS model.  In the reference's order: the neighbour table (this package's ``knn_points``),
    the densities and the level search (one native call), the "range is empty" midpoint rule, the minimal layer size
    (``spatial_extent`` is ``training_cameras.get_spatial_extent()``, needed when ``min_layer_size > 0``), the two clamps and
    the smoothing over each vertex's nearest vertices.  Returns ``outer_verts``, ``inner_verts``, ``outer_dist``,
    ``inner_dist``."""
    n = int(n_samples_per_vertex)
    with torch.no_grad():
        idx = knn_points(mesh_verts[None].float(), points[None].float(), K=n_closest_gaussians_to_use).idx[0]
        lin = torch.linspace(0., 1., n).to(mesh_verts.device)
        res = ray_level_crossings(mesh_verts, mesh_verts_normals, inner_range - outer_range, outer_range, lin, idx, points, scaling,
                                  quaternions, strengths, [level], density_factor=1.0,
                                  inner_mode="last" if use_last_intersection_as_inner_level_point else "second_crossing")
        outer_dist, inner_dist = res["t_outer"][0], res["t_inner"][0]
        # all densities under the level: the middle of the range
        empty = (res["first_above"][0] == 0) & (res["last_above"][0] == n - 1) & res["under_first"][0]
        middle = (inner_range + outer_range) / 2
        outer_dist = torch.where(empty, middle, outer_dist)
        inner_dist = torch.where(empty, middle, inner_dist)
        if min_layer_size > 0:
            if spatial_extent is None:
                raise ValueError("min_layer_size > 0 needs spatial_extent (training_cameras.get_spatial_extent())")
            flat = (inner_dist - outer_dist).abs() < min_layer_size * spatial_extent
            outer_dist = torch.where(flat, middle - 0.5 * min_layer_size * spatial_extent, outer_dist)
            inner_dist = torch.where(flat, middle + 0.5 * min_layer_size * spatial_extent, inner_dist)
        if min_clamping_inner_dist is not None:
            inner_dist = inner_dist.clamp_min(min_clamping_inner_dist)
        if max_clamping_outer_dist is not None:
            outer_dist = outer_dist.clamp_max(max_clamping_outer_dist)
        if smooth_points:
            near = knn_points(mesh_verts[None].float(), mesh_verts[None].float(), K=n_neighbors_for_smoothing).idx[0]
            outer_dist = outer_dist[near].mean(dim=1)
            inner_dist = inner_dist[near].mean(dim=1)
        return {"outer_verts": mesh_verts + outer_dist[:, None] * mesh_verts_normals,
                "inner_verts": mesh_verts + inner_dist[:, None] * mesh_verts_normals,
                "outer_dist": outer_dist, "inner_dist": inner_dist}


def level_surface_points_from_rays(world_points, camera_center, closest_gaussians_idx, points, scaling, quaternions, strengths,
                                   surface_levels, n_points_in_range=21, range_size=3.0, density_factor=1.0, return_normals=True,
                                   use_last_intersection_as_inner_level_point=False):
    """``compute_level_surface_points_and_range_from_camera`` from ``all_world_points`` onward (frosting_model.py:1870-2011):
    ``world_points [R,3]`` are the back-projected depth points of one camera, ``camera_center [3]`` or ``[1,3]`` its centre,
    ``closest_gaussians_idx [R,K]`` the rows ``knn_idx[gaussian_idx]`` of the model's neighbour table (column 0 is the pixel's
    own Gaussian, whose standard deviation along the view direction sets the range).  Returns ``{level: {
    'intersection_points', 'inner_intersection_points', 'normals' (when asked), 'valid'}}``: ``valid [R]`` is the reference's
    ``~empty_pixels`` and the other three are compacted by it, as the reference's outputs are; index ``pixel_idx`` /
    ``gaussian_idx`` with ``valid`` to get the reference's.

    Limits: what lies upstream of ``all_world_points`` -- the depth render, the back-projection and the sub-sampling of
    pixels, which are pytorch3d camera calls -- stays with the caller; ``compute_intersection_for_flat_gaussian``,
    ``compute_flat_normals`` and ``just_use_depth_as_level`` are not offered (coarse_shell.py leaves the first and last off).
    """
    with torch.no_grad():
        centre = camera_center.reshape(1, 3)
        gaussian_to_camera = torch.nn.functional.normalize(centre - points, dim=-1)
        stds = (scaling * quaternion_apply(quaternion_invert(quaternions), gaussian_to_camera)).norm(dim=-1)
        points_stds = stds[closest_gaussians_idx[..., 0].long()]
        lin = torch.linspace(-range_size, range_size, n_points_in_range).to(world_points.device)
        camera_to_samples = torch.nn.functional.normalize(world_points - centre, dim=-1)
        res = ray_level_crossings(world_points, camera_to_samples, points_stds, torch.zeros_like(points_stds), lin,
                                  closest_gaussians_idx, points, scaling, quaternions, strengths, surface_levels,
                                  density_factor=density_factor, return_normals=return_normals,
                                  inner_mode="last" if use_last_intersection_as_inner_level_point else "second_crossing")
        all_outputs = {}
        for l, level in enumerate(surface_levels):
            valid = res["under_first"][l] & (res["first_above"][l] > 0)
            base, rays = world_points[valid], camera_to_samples[valid]
            out = {"intersection_points": base + res["t_outer"][l][valid][:, None] * rays,
                   "inner_intersection_points": base + res["t_inner"][l][valid][:, None] * rays,
                   "valid": valid}
            if return_normals:
                out["normals"] = res["normals"][l][valid]
            all_outputs[level] = out
        return all_outputs
