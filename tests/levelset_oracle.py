"""Level crossings of the density of K neighbour Gaussians along rays, restated in torch ops of any dtype (float64: the
yardstick of the GPU tests; float32 on the CPU: the error a float32 evaluation of these formulas has).
tests/test_levelset_cpu.py pins this restatement to the arrays the reference's own functions produced
(tests/golden/levelset_*.npz, tools/make_golden_levelset.py)."""
import collections

import numpy as np
import torch

import knn_points_oracle as KO
from field_oracle import EPS32, inv_scaled_rotation, judge, rotation  # noqa: F401

FLOATS = ("origins", "directions", "t_scale", "t_offset", "lin", "points", "scaling", "quaternions", "strengths")


# ---- the three pytorch3d.transforms helpers the reference's functions read ----
quaternion_to_matrix = rotation


def quaternion_invert(q):
    return q * q.new_tensor([1, -1, -1, -1])


def quaternion_raw_multiply(a, b):
    aw, ax, ay, az = torch.unbind(a, -1)
    bw, bx, by, bz = torch.unbind(b, -1)
    ow = aw * bw - ax * bx - ay * by - az * bz
    ox = aw * bx + ax * bw + ay * bz - az * by
    oy = aw * by - ax * bz + ay * bw + az * bx
    oz = aw * bz + ax * by - ay * bx + az * bw
    return torch.stack((ow, ox, oy, oz), -1)


def quaternion_apply(q, point):
    real = point.new_zeros(point.shape[:-1] + (1,))
    out = quaternion_raw_multiply(quaternion_raw_multiply(q, torch.cat((real, point), -1)), quaternion_invert(q))
    return out[..., 1:]


_KNN = collections.namedtuple("KNN", "dists idx knn")


def knn_points(p1, p2, K=1, **_):
    """pytorch3d.ops.knn_points' signature over one batch: exact brute force, ties to the smaller index (the rule of
    frosting_amd.knn.knn_points)."""
    d, i = KO.knn_points(p1[0].detach().float().numpy(), p2[0].detach().float().numpy(), K)
    return _KNN(torch.from_numpy(d)[None], torch.from_numpy(i)[None], None)


# ---- the kernel's three parts ----
def sample_t(lin, t_scale, t_offset):
    return lin[None, :] * t_scale[:, None] + t_offset[:, None]                  # [R,n]


def _opacities(x, idx, points, scaling, quaternions, strengths, density_factor):
    """x [M,3], idx [M,K] -> (o [M,K], A [M,K,3,3], w [M,K,3])"""
    idx = idx.long()
    A = inv_scaled_rotation(scaling, quaternions)[idx]
    w = A.transpose(-1, -2) @ (x[:, None] - points[idx])[..., None]
    m = (w[..., 0] * w[..., 0]).sum(dim=-1).clamp(min=0., max=1e8)
    return density_factor * strengths.reshape(-1)[idx] * torch.exp(-1. / 2 * m), A, w


def densities(origins, directions, t_scale, t_offset, lin, idx, points, scaling, quaternions, strengths, density_factor=1.0):
    """-> (dens [R,n], t [R,n])"""
    t = sample_t(lin, t_scale, t_offset)
    R, n = t.shape
    x = (origins[:, None, :] + t[..., None] * directions[:, None, :]).view(-1, 3)
    o, _, _ = _opacities(x, idx[:, None, :].expand(-1, n, -1).reshape(R * n, -1), points, scaling, quaternions, strengths, density_factor)
    d = o.sum(dim=-1)
    big = d >= 1.
    d = torch.where(big, d / (d + 1e-12), d)
    return d.reshape(R, n), t


def search(dens, t, level, inner_mode="last"):
    """The reference's search and interpolation on given densities [R,n] and sample parameters [R,n]."""
    n = dens.shape[1]
    under, above = dens - level < 0, dens - level > 0
    first = above.max(dim=-1, keepdim=True)[1]
    if inner_mode == "last":
        last = (n - 1) - above.flip(dims=(-1,)).max(dim=-1, keepdim=True)[1]
    else:
        last = (under[..., 1:] * above[..., :-1]).max(dim=-1, keepdim=True)[1]
        last[last == 0] = n - 1
    bound_o = first[:, 0] > 0
    v1, v0 = dens.gather(1, first)[:, 0], dens.gather(1, (first - 1).clamp(min=0))[:, 0]
    t1, t0 = t.gather(1, first)[:, 0], t.gather(1, (first - 1).clamp(min=0))[:, 0]
    t_outer = torch.where(bound_o, (level - v0) / (v1 - v0) * (t1 - t0) + t0, t[:, 0])
    bound_i = last[:, 0] < n - 1
    after = (last + 1).clamp(max=n - 1)
    va, vb = dens.gather(1, last)[:, 0], dens.gather(1, after)[:, 0]
    ta, tb = t.gather(1, last)[:, 0], t.gather(1, after)[:, 0]
    t_inner = torch.where(bound_i, (level - va) / (vb - va) * (tb - ta) + ta, t[:, -1])
    return {"first_above": first[:, 0], "last_above": last[:, 0], "under_first": under[:, 0], "t_outer": t_outer, "t_inner": t_inner}


def normals(origins, directions, t_outer, first_above, idx, points, scaling, quaternions, strengths, density_factor=1.0):
    """-normalize(density gradient) at o + t_outer d; zeros where first_above == 0 (the kernel's convention)."""
    x = origins + t_outer[:, None] * directions
    o, A, w = _opacities(x, idx, points, scaling, quaternions, strengths, density_factor)
    grad = (o[..., None] * (A @ w)[..., 0]).sum(dim=-2)
    nrm = -torch.nn.functional.normalize(grad, dim=-1)
    return torch.where((first_above > 0)[:, None], nrm, torch.zeros_like(nrm))


def crossings(t, levels, inner_mode="last", density_factor=1.0, with_normals=True):
    """t: {name: tensor} of FLOATS and 'idx' -> what frosting_amd.levelset.ray_level_crossings returns, stacked over levels."""
    args = [t[k] for k in ("idx", "points", "scaling", "quaternions", "strengths")]
    dens, ts = densities(t["origins"], t["directions"], t["t_scale"], t["t_offset"], t["lin"], *args, density_factor)
    per = [search(dens, ts, lv, inner_mode) for lv in levels]
    out = {k: torch.stack([p[k] for p in per]) for k in per[0]}
    out["densities"], out["t"] = dens, ts
    if with_normals:
        out["normals"] = torch.stack([normals(t["origins"], t["directions"], p["t_outer"], p["first_above"], *args, density_factor) for p in per])
    return out


def tensors(arrays, dtype):
    return {k: (torch.from_numpy(np.asarray(v)).to(dtype) if k in FLOATS else torch.from_numpy(np.asarray(v))) for k, v in arrays.items()}


# ---- the two Python-level functions ----
def level_points_along_normals(points, scaling, quaternions, strengths, mesh_verts, mesh_verts_normals, inner_range, outer_range,
                               n_samples_per_vertex=21, n_closest_gaussians_to_use=16, level=0.1, smooth_points=True,
                               n_neighbors_for_smoothing=4, use_last_intersection_as_inner_level_point=True,
                               min_clamping_inner_dist=None, max_clamping_outer_dist=None, min_layer_size=0.0, spatial_extent=None,
                               idx=None):
    n = n_samples_per_vertex
    if idx is None:
        idx = knn_points(mesh_verts[None], points[None], K=n_closest_gaussians_to_use).idx[0]
    lin = torch.linspace(0., 1., n).to(mesh_verts.dtype)
    dens, t = densities(mesh_verts, mesh_verts_normals, inner_range - outer_range, outer_range, lin, idx, points, scaling, quaternions, strengths)
    s = search(dens, t, level, "last" if use_last_intersection_as_inner_level_point else "second_crossing")
    outer_dist, inner_dist = s["t_outer"], s["t_inner"]
    empty = (s["first_above"] == 0) & (s["last_above"] == n - 1) & s["under_first"]
    middle = (inner_range + outer_range) / 2
    outer_dist, inner_dist = torch.where(empty, middle, outer_dist), torch.where(empty, middle, inner_dist)
    if min_layer_size > 0:
        flat = (inner_dist - outer_dist).abs() < min_layer_size * spatial_extent
        outer_dist = torch.where(flat, middle - 0.5 * min_layer_size * spatial_extent, outer_dist)
        inner_dist = torch.where(flat, middle + 0.5 * min_layer_size * spatial_extent, inner_dist)
    if min_clamping_inner_dist is not None:
        inner_dist = inner_dist.clamp_min(min_clamping_inner_dist)
    if max_clamping_outer_dist is not None:
        outer_dist = outer_dist.clamp_max(max_clamping_outer_dist)
    if smooth_points:
        near = knn_points(mesh_verts[None], mesh_verts[None], K=n_neighbors_for_smoothing).idx[0]
        outer_dist, inner_dist = outer_dist[near].mean(dim=1), inner_dist[near].mean(dim=1)
    return {"outer_verts": mesh_verts + outer_dist[:, None] * mesh_verts_normals,
            "inner_verts": mesh_verts + inner_dist[:, None] * mesh_verts_normals,
            "outer_dist": outer_dist, "inner_dist": inner_dist,
            "first_above": s["first_above"], "last_above": s["last_above"], "under_first": s["under_first"], "empty": empty,
            "densities": dens}


def level_surface_points_from_rays(world_points, camera_center, closest_gaussians_idx, points, scaling, quaternions, strengths,
                                   surface_levels, n_points_in_range=21, range_size=3.0, density_factor=1.0, return_normals=True,
                                   use_last_intersection_as_inner_level_point=False):
    idx = closest_gaussians_idx
    centre = camera_center.reshape(1, 3)
    gaussian_to_camera = torch.nn.functional.normalize(centre - points, dim=-1)
    stds = (scaling * quaternion_apply(quaternion_invert(quaternions), gaussian_to_camera)).norm(dim=-1)
    points_stds = stds[idx[..., 0]]
    lin = torch.linspace(-range_size, range_size, n_points_in_range).to(world_points.dtype)
    rays = torch.nn.functional.normalize(world_points - centre, dim=-1)
    dens, t = densities(world_points, rays, points_stds, torch.zeros_like(points_stds), lin, idx, points, scaling, quaternions, strengths, density_factor)
    out = {}
    for level in surface_levels:
        s = search(dens, t, level, "last" if use_last_intersection_as_inner_level_point else "second_crossing")
        valid = s["under_first"] & (s["first_above"] > 0)
        o = {"intersection_points": (world_points + s["t_outer"][:, None] * rays)[valid],
             "inner_intersection_points": (world_points + s["t_inner"][:, None] * rays)[valid], "valid": valid,
             "first_above": s["first_above"], "last_above": s["last_above"], "under_first": s["under_first"], "densities": dens}
        if return_normals:
            o["normals"] = normals(world_points, rays, s["t_outer"], s["first_above"], idx, points, scaling, quaternions, strengths,
                                   density_factor)[valid]
        out[level] = o
    return out
