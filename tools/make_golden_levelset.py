"""Fixtures for the level-set crossings, produced by the reference's OWN compute_level_points_along_normals and
compute_level_surface_points_and_range_from_camera run on the CPU.

frosting_scene/frosting_model.py is imported where this tool runs, with the modules this platform lacks stubbed in
sys.modules.  The module globals the two functions read are then set: knn_points becomes an exact brute-force stand-in with
this project's tie rule, the three quaternion helpers become the restatements of tests/levelset_oracle.py, SuGaR becomes a
plain stand-in class carrying points, scaling, quaternions, strengths, device.  The camera function runs on a stand-in self,
stand-in cameras (recorded unproject_points and get_camera_center) and a rasterizer callable that returns a recorded zbuf
and pix_to_face, with splat_mesh=False and n_surface_points=-1: all_world_points is an input of the fixture.

Both functions keep their densities in a `dtype=torch.float` buffer whatever the inputs are; for the float64 run the
module's `torch` global is a proxy whose `float` is float64, so the float64 run is float64 throughout.  The functions return
positions only; their discrete results (first / last point above the level, under_level[..., 0], the empty mask) and the
densities are read from the functions' own local variables when they return (sys.setprofile).  Nothing of the reference's
text is written anywhere -- only the arrays that go in and come out, and the sha256 of the file that produced them.

Asserted for every case: the float32 and float64 runs agree on the discrete results of at least 99 % of the rays, every
file stays under 1 MiB; and over all cases every branch (outer crossing found / not, inner found / not, empty) has at
least 5 rays somewhere, and one case holds densities that reach 1.

    python tools/make_golden_levelset.py          # needs the reference (FROSTING_REFERENCE, default /root/reference)
"""
import hashlib
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("FROSTING_REFERENCE", "/root/reference")

import levelset_oracle as LO  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DISCRETE = ("first_above", "last_above", "under_first", "empty")


class _Stub(types.ModuleType):
    """A module any name can be imported from."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


class _Torch64:
    """torch, except that `float` is float64."""
    float = torch.float64

    def __getattr__(self, name):
        return getattr(torch, name)


class SuGaRStandIn:
    pass


def load_reference():
    for name in ("open3d", "pytorch3d", "pytorch3d.renderer", "pytorch3d.structures", "pytorch3d.transforms", "pytorch3d.ops",
                 "pytorch3d.utils", "pytorch3d.io", "pytorch3d.loss", "simple_knn", "simple_knn._C", "diff_gaussian_rasterization",
                 "frosting_scene.gs_model", "frosting_scene.cameras", "nvdiffrast", "nvdiffrast.torch",
                 "frosting_utils.mesh_rasterization", "frosting_utils.nvdiffrast"):
        sys.modules[name] = _Stub(name)
    sys.path.insert(0, REF)
    import frosting_scene.frosting_model as fm
    import frosting_scene.sugar_model as sm
    for mod in (fm, sm):
        mod.quaternion_to_matrix, mod.quaternion_apply, mod.quaternion_invert = LO.quaternion_to_matrix, LO.quaternion_apply, LO.quaternion_invert
        mod.knn_points = LO.knn_points
    real_sugar = sm.SuGaR
    SuGaRStandIn.get_covariance = lambda self, **kw: real_sugar.get_covariance(self, **kw)
    fm.SuGaR = SuGaRStandIn
    path = os.path.join(REF, "frosting_scene", "frosting_model.py")
    return fm, hashlib.sha256(open(path, "rb").read()).hexdigest()


def call_capturing_locals(fm, dtype, fn, *args, **kw):
    """fn(*args, **kw) -> (its result, its local variables at return).  In the float64 run the module's `torch` is the proxy."""
    box = {}

    def prof(frame, event, arg):
        if event == "return" and frame.f_code is fn.__code__:
            box.update(frame.f_locals)

    plain = fm.torch
    fm.torch = _Torch64() if dtype == torch.float64 else plain
    sys.setprofile(prof)
    try:
        out = fn(*args, **kw)
    finally:
        sys.setprofile(None)
        fm.torch = plain
    return out, box


def model_for(arrays, dtype, extent=None):
    m = SuGaRStandIn()
    for k in ("points", "scaling", "quaternions", "strengths"):
        setattr(m, k, torch.from_numpy(arrays[k]).to(dtype))
    m.device = torch.device("cpu")
    m.nerfmodel = SimpleNamespace(training_cameras=SimpleNamespace(get_spatial_extent=lambda: extent))
    return m


def scene(seed, P, R, scale_log=-2.3, strength_shift=1.5, normalise_q=False):
    """The recipe: P Gaussians on a noisy unit sphere, R rays from points near it along their own radial direction."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    ru = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    xyz = rn(P, 3)
    xyz = xyz / xyz.norm(dim=-1, keepdim=True) * (1 + 0.03 * rn(P, 1))
    q = rn(P, 4)
    if normalise_q:
        q = q / q.norm(dim=-1, keepdim=True)
    a = dict(points=xyz, scaling=torch.exp(scale_log + 0.5 * rn(P, 3)), quaternions=q, strengths=torch.sigmoid(strength_shift + rn(P, 1)))
    v = rn(R, 3)
    v = v / v.norm(dim=-1, keepdim=True)
    a["normals"] = v.clone()
    a["verts"] = v * (1 + 0.02 * rn(R, 1))
    a["inner_range"] = 0.35 + 0.3 * ru(R)
    a["outer_range"] = -a["inner_range"] * (0.6 + 0.8 * ru(R))
    a["u"] = ru(R)
    return {k: t.float().numpy() for k, t in a.items()}                      # rounded to float32 once


def discrete_of(loc, n, camera):
    first, last = loc["first_point_above_level"][..., 0], loc["last_point_above_level"][..., 0]
    under = loc["under_level"][..., 0]
    empty = loc["empty_pixels"] if camera else loc["empty_mask"]
    return {"first_above": first.numpy().astype(np.int32), "last_above": last.numpy().astype(np.int32),
            "under_first": under.numpy(), "empty": empty.numpy()}


def finish(name, fx, runs, n, coverage):
    """runs: {(tag, 'f64' | 'f32'): (float outputs, discrete results, densities)} -> the file, after the assertions."""
    tau = 0.0
    for tag in sorted({t for t, _ in runs}):
        (o64, d64, dens64), (o32, d32, dens32) = runs[(tag, "f64")], runs[(tag, "f32")]
        agree = np.ones(len(d64["first_above"]), bool)
        for k in DISCRETE:
            agree &= d64[k] == d32[k]
        assert agree.mean() >= 0.99, (name, tag, agree.mean())
        tau = max(tau, float(np.abs(dens32.astype(np.float64) - dens64).max()))
        for prec, (o, d, dens) in (("f64", runs[(tag, "f64")]), ("f32", runs[(tag, "f32")])):
            keep = (lambda v: v.astype(np.float32)) if prec == "f32" else (lambda v: v)
            fx.update({f"{tag}_{prec}_{k}": keep(v) for k, v in o.items()})
            fx.update({f"{tag}_{prec}_{k}": v for k, v in d.items()})
            fx[f"{tag}_{prec}_densities"] = keep(dens)
        f, l, e = d64["first_above"], d64["last_above"], d64["empty"]
        for key, mask in (("outer_found", f > 0), ("outer_unbound", f == 0), ("inner_found", l < n - 1), ("inner_unbound", l == n - 1), ("empty", e)):
            coverage[key] = max(coverage.get(key, 0), int(mask.sum()))
        coverage["dens_is_1"] = max(coverage.get("dens_is_1", 0), int((dens32 == 1).sum()))
        print(f"{name} {tag}: agree {agree.mean():.4f}  outer found {int((f > 0).sum())}  inner found {int((l < n - 1).sum())}  "
              f"empty {int(e.sum())}  dens == 1 (f32) {int((dens32 == 1).sum())}")
    fx["tau"] = np.float64(4.0 * tau)                        # 4 x the largest |f32 - f64| density difference of the reference
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **fx)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    print(f"{name}: tau {fx['tau']:.3e}  {os.path.getsize(path)} bytes")


def normals_case(fm, sha, name, coverage, seed, P, R, K, n, level, last, smooth, min_layer_size=0.0, clamps=False, **scene_kw):
    a = scene(seed, P, R, **scene_kw)
    extent = 2.5
    kw = dict(n_samples_per_vertex=n, n_closest_gaussians_to_use=K, level=level, smooth_points=smooth, n_neighbors_for_smoothing=4,
              use_last_intersection_as_inner_level_point=last, min_layer_size=min_layer_size)
    fx = {k: a[k] for k in ("points", "scaling", "quaternions", "strengths", "verts", "normals", "inner_range", "outer_range")}
    if clamps:
        fx["min_clamping_inner_dist"] = (0.25 * a["inner_range"] * a["u"]).astype(np.float32)
        fx["max_clamping_outer_dist"] = (0.25 * a["outer_range"] * (1 - a["u"])).astype(np.float32)
    runs = {}
    for prec, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        t = {k: torch.from_numpy(v).to(dtype) for k, v in fx.items()}
        extra = {k: t[k] for k in ("min_clamping_inner_dist", "max_clamping_outer_dist") if k in t}
        out, loc = call_capturing_locals(fm, dtype, fm.compute_level_points_along_normals, model_for(fx, dtype, extent), t["verts"],
                                         t["normals"], t["inner_range"], t["outer_range"], **kw, **extra)
        assert loc["densities"].dtype == dtype
        runs[("run", prec)] = ({k: v.double().numpy() for k, v in out.items()}, discrete_of(loc, n, False),
                               loc["densities"].double().numpy())
        idx = loc["closest_gaussians_idx"].numpy().astype(np.int64)
    fx.update(kind=np.array("normals"), idx=idx, K=np.int64(K), n=np.int64(n), levels=np.array([level]), last=np.bool_(last),
              smooth=np.bool_(smooth), min_layer_size=np.float64(min_layer_size), spatial_extent=np.float64(extent),
              frosting_model_sha256=np.array(sha))
    finish(name, fx, runs, n, coverage)


def camera_case(fm, sha, name, coverage, seed, P, H, W, K, n, levels, last, density_factor=1.0, **scene_kw):
    R = H * W
    a = scene(seed, P, R, normalise_q=True, **scene_kw)
    centre = np.array([[0.3, -0.2, 3.5]], np.float32)
    world = a["verts"].copy()
    world[:, 2] = np.abs(world[:, 2])                        # the hemisphere that faces the camera
    pix_gaussian = LO.KO.knn_points(world, a["points"], 1)[1][:, 0]
    knn_idx = LO.KO.knn_points(a["points"], a["points"], K)[1]
    depth = np.linalg.norm(world - centre, axis=-1).astype(np.float32)
    fx = {k: a[k] for k in ("points", "scaling", "quaternions", "strengths")}
    fx.update(world_points=world, camera_center=centre, idx=knn_idx[pix_gaussian].astype(np.int64))
    runs = {}
    for prec, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        for level in levels:
            me = model_for(fx, dtype)
            me.image_height, me.image_width, me.sh_levels, me.n_triangles_per_gaussian, me.knn_to_track = H, W, 1, 1, K
            me.knn_idx = torch.from_numpy(knn_idx)
            me.get_texture_img = lambda **kw: torch.zeros(1, 1, 3)
            me.mesh = SimpleNamespace(textures=SimpleNamespace(_maps_padded=None))
            cam = SimpleNamespace(unproject_points=lambda pts, scaled_depth_input=False: torch.from_numpy(world).to(dtype)[None],
                                  get_camera_center=lambda: torch.from_numpy(centre).to(dtype))
            raster = lambda mesh, cameras=None: SimpleNamespace(zbuf=torch.from_numpy(depth).to(dtype).view(1, H, W, 1),
                                                                pix_to_face=torch.from_numpy(pix_gaussian).view(1, H, W, 1))
            out, loc = call_capturing_locals(fm, dtype, fm.compute_level_surface_points_and_range_from_camera, me,
                                             nerf_cameras=SimpleNamespace(p3d_cameras=[cam]), cam_idx=0, rasterizer=raster,
                                             surface_levels=[level], n_surface_points=-1, splat_mesh=False, n_points_in_range=n,
                                             range_size=3., density_factor=density_factor, return_normals=True,
                                             use_last_intersection_as_inner_level_point=last)
            assert loc["densities"].dtype == dtype and torch.equal(loc["closest_gaussians_idx"], torch.from_numpy(fx["idx"]))
            d = discrete_of(loc, n, True)
            d["valid"] = ~d["empty"]
            runs[(f"level{level}", prec)] = ({k: v.double().numpy() for k, v in out[level].items()}, d, loc["densities"].double().numpy())
    fx.update(kind=np.array("camera"), K=np.int64(K), n=np.int64(n), levels=np.array(levels), last=np.bool_(last),
              density_factor=np.float64(density_factor), range_size=np.float64(3.0), frosting_model_sha256=np.array(sha))
    finish(name, fx, runs, n, coverage)


if __name__ == "__main__":
    fm, sha = load_reference()
    cov = {}
    normals_case(fm, sha, "levelset_normals_last", cov, seed=1, P=600, R=1000, K=16, n=21, level=0.1, last=True, smooth=True)
    normals_case(fm, sha, "levelset_normals_second", cov, seed=2, P=600, R=1000, K=16, n=21, level=0.1, last=False, smooth=False)
    normals_case(fm, sha, "levelset_normals_minlayer", cov, seed=3, P=600, R=1000, K=16, n=21, level=0.1, last=True, smooth=True,
                 min_layer_size=0.1, clamps=True)
    camera_case(fm, sha, "levelset_camera", cov, seed=4, P=600, H=25, W=40, K=16, n=21, levels=[0.1, 0.3, 0.5], last=False)
    normals_case(fm, sha, "levelset_small", cov, seed=5, P=150, R=257, K=5, n=7, level=0.3, last=True, smooth=False)
    camera_case(fm, sha, "levelset_dense", cov, seed=6, P=600, H=20, W=25, K=16, n=21, levels=[0.5], last=True, scale_log=-1.7,
                strength_shift=4.0)
    print(cov)
    assert all(cov.get(k, 0) >= 5 for k in ("outer_found", "outer_unbound", "inner_found", "inner_unbound", "empty")), cov
    assert cov["dens_is_1"] >= 5, cov
