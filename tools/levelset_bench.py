"""The level-crossing kernel and the two functions above it beside the eager torch formulation, on the GPU, at the two
workloads' own shapes.

  levelset_bench.py [--form camera|normals|both] [--p 3000000] [--width 1600 --height 1056] [--verts 1000000] [--reps 5]

camera:  one ray per pixel of a 1600 x 1056 frame, K = 16, n = 21, three levels, normals on, over 3 000 000 Gaussians
         (compute_level_surface_points_and_range_from_camera, once per training camera).
normals: 1 000 000 vertices, K = 16, n = 21, one level (compute_level_points_along_normals, twice per model).
The Gaussians are a unit-variance cloud with scales near the neighbour spacing; the neighbour table is our knn_points'.
Timed per form: the native call alone (ray_level_crossings on prepared inputs), the Python-level function (for normals it
includes both knn_points calls), and the eager chain written here from the formulas, in passes of 2 000 000 samples as the
reference runs it ([samples, K, 3, 3] gathers, the batched product, exp, sum, then the max / gather / boolean-index
search).  Every variant is warmed up, then timed over `reps` calls ending in a device synchronise, the variants alternating,
three rounds; the median round is reported.  Prints one JSON line per form.

Traffic model of the native call (bytes the algorithm needs): per ray 32 B of ray inputs, K indices of 8 B, K records of
64 B, the outputs; the normal walk reads the K records again per level on rays with a crossing.  exp model: R n K for the
densities plus K per level and crossing for the normals.  Peaks used for the two lower bounds: 8.0 TB/s HBM (spec) and
256 CUs x 16 transcendental lanes x 2.4 GHz = 9.8e12 exp/s.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from frosting_amd import levelset as LS  # noqa: E402
from frosting_amd.knn import knn_points  # noqa: E402

PASS = 2_000_000
HBM_PEAK, EXP_PEAK = 8.0e12, 256 * 16 * 2.4e9


def rotation(q):
    r, i, j, k = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    rows = (1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
            two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
            two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j))
    return torch.stack(rows, -1).reshape(q.shape[:-1] + (3, 3))


def eager_densities(samples, sample_idx, points, A, strengths, factor):
    dens = torch.zeros(len(samples), dtype=torch.float, device=samples.device)
    for i in range(0, len(samples), PASS):
        idx = sample_idx[i:i + PASS]
        w = A[idx].transpose(-1, -2) @ (samples[i:i + PASS, None] - points[idx])[..., None]
        o = factor * strengths[idx][..., 0] * torch.exp(-1. / 2 * (w[..., 0] * w[..., 0]).sum(dim=-1).clamp(min=0., max=1e8))
        d = o.sum(dim=-1)
        m = d >= 1.
        d[m] = d[m] / (d[m] + 1e-12)
        dens[i:i + PASS] = d
    return dens


def eager_search(dens, t, level, last_mode):
    n = dens.shape[1]
    under, above = dens - level < 0, dens - level > 0
    first = above.max(dim=-1, keepdim=True)[1]
    if last_mode:
        last = (n - 1) - above.flip(dims=(-1,)).max(dim=-1, keepdim=True)[1]
    else:
        last = (under[..., 1:] * above[..., :-1]).max(dim=-1, keepdim=True)[1]
        last[last == 0] = n - 1
    return under, first, last


def eager_cross(dens, t, level, a, b):
    va, vb, ta, tb = dens.gather(1, a).view(-1), dens.gather(1, b).view(-1), t.gather(1, a).view(-1), t.gather(1, b).view(-1)
    return (level - va) / (vb - va) * (tb - ta) + ta


def eager_normals_form(verts, normals, inner, outer, idx, points, scaling, quaternions, strengths, n, level, K):
    idx = knn_points(verts[None], points[None], K=K).idx[0]                 # the native search: the reference's is pytorch3d's CUDA one
    t = (torch.linspace(0., 1., n, device=verts.device).view(1, -1, 1) * (inner - outer)[..., None, None] + outer[..., None, None])
    samples = (verts[:, None, :] + t * normals[:, None, :]).view(-1, 3)
    sidx = idx[:, None, :].expand(-1, n, -1).reshape(-1, K)
    A = rotation(quaternions) * (1. / scaling.clamp(min=1e-8))[:, None]
    dens = eager_densities(samples, sidx, points, A, strengths, 1.0).reshape(-1, n)
    t = t[..., 0]
    under, first, last = eager_search(dens, t, level, True)
    ob, ib = first[..., 0] > 0, last[..., 0] < n - 1
    outer_dist, inner_dist = 0. + t[..., 0], 0. + t[..., -1]
    outer_dist[ob] = eager_cross(dens[ob], t[ob], level, first[ob] - 1, first[ob])
    inner_dist[ib] = eager_cross(dens[ib], t[ib], level, last[ib], last[ib] + 1)
    empty = (~ob) * (~ib) * under[..., 0]
    outer_dist[empty] = (inner + outer)[empty] / 2
    inner_dist[empty] = (inner + outer)[empty] / 2
    near = knn_points(verts[None], verts[None], K=4).idx[0]
    outer_dist, inner_dist = outer_dist[near].mean(dim=1), inner_dist[near].mean(dim=1)
    return verts + outer_dist[:, None] * normals, verts + inner_dist[:, None] * normals


def eager_camera_form(world, centre, idx, points, scaling, quaternions, strengths, levels, n, factor, K):
    g2c = torch.nn.functional.normalize(centre - points, dim=-1)
    stds = (scaling * LS.quaternion_apply(LS.quaternion_invert(quaternions), g2c)).norm(dim=-1)[idx[..., 0]]
    t = torch.linspace(-3., 3., n, device=world.device).view(1, -1, 1) * stds[..., None, None].expand(-1, n, 1)
    rays = torch.nn.functional.normalize(world - centre, dim=-1)
    samples = (world[:, None, :] + t * rays[:, None, :]).view(-1, 3)
    sidx = idx[:, None, :].expand(-1, n, -1).reshape(-1, K)
    A = rotation(quaternions) * (1. / scaling.clamp(min=1e-8))[:, None]
    dens = eager_densities(samples, sidx, points, A, strengths, factor).reshape(-1, n)
    t = t[..., 0]
    out = {}
    for level in levels:
        under, first, last = eager_search(dens, t, level, False)
        valid = under[..., 0] & (first[..., 0] > 0)
        ti = eager_cross(dens[valid], t[valid], level, first[valid] - 1, first[valid])
        pts = world[valid] + ti[:, None] * rays[valid]
        ib = valid & (last[..., 0] < n - 1)
        tin = 0. + t[valid][..., -1]
        tin[(last[..., 0] < n - 1)[valid]] = eager_cross(dens[ib], t[ib], level, last[ib], last[ib] + 1)
        inner_pts = world[valid] + tin[:, None] * rays[valid]
        vi = idx[valid]
        w = A[vi].transpose(-1, -2) @ (pts[:, None] - points[vi])[..., None]
        o = factor * strengths[vi][..., 0] * torch.exp(-1. / 2 * (w[..., 0] * w[..., 0]).sum(dim=-1).clamp(min=0., max=1e8))
        grad = (o[..., None] * (A[vi] @ w)[..., 0]).sum(dim=-2)
        out[level] = (pts, inner_pts, -torch.nn.functional.normalize(grad, dim=-1), valid)
    return out


def timed(variants, reps):
    for fn in variants.values():
        fn(); fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(3):
        for name, fn in variants.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(reps[name]):
                fn()
            torch.cuda.synchronize()
            rounds[name].append((time.perf_counter() - t0) / reps[name] * 1e3)
    return {k: sorted(v)[1] for k, v in rounds.items()}, rounds


def model(P, K, dev, g):
    points = torch.randn(P, 3, generator=g).to(dev)
    spacing = (1.0 / P) ** (1.0 / 3.0)
    scaling = (spacing * torch.exp(0.3 * torch.randn(P, 3, generator=g))).to(dev)
    quaternions = torch.nn.functional.normalize(torch.randn(P, 4, generator=g)).to(dev)
    strengths = torch.sigmoid(torch.randn(P, 1, generator=g)).to(dev)
    return points, scaling, quaternions, strengths, spacing


def report(form, R, P, K, n, L, ms, rounds, crossings, extra):
    kernel_s = ms["native_call"] * 1e-3
    bytes_needed = R * (32 + K * (8 + 64) + n * 0 + L * (4 + 4 + 4 + 4 + 1)) + crossings * (K * 64 + 12) + P * (44 + 64)
    exps = R * n * K + crossings * K
    out = {"tool": "levelset_bench", "form": form, "device": torch.cuda.get_device_name(0), "R": R, "P": P, "K": K, "n": n, "levels": L,
           "ms_median_of_3_rounds": {k: round(v, 3) for k, v in ms.items()}, "ms_rounds": {k: [round(x, 3) for x in v] for k, v in rounds.items()},
           "eager_over_function": round(ms["eager"] / ms["function"], 2),
           "native_call_includes": "the record pack pre-pass (P x 44 B read, 64 B written), the output allocations",
           "bytes_needed": bytes_needed, "achieved_TBps": round(bytes_needed / kernel_s / 1e12, 3),
           "exp_needed": exps, "achieved_Texp_per_s": round(exps / kernel_s / 1e12, 3),
           "floor_ms_bytes_at_8TBps": round(bytes_needed / HBM_PEAK * 1e3, 3), "floor_ms_exp_at_9.8T": round(exps / EXP_PEAK * 1e3, 3),
           "peak_memory_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    out["bound_by"] = "exp" if out["floor_ms_exp_at_9.8T"] > out["floor_ms_bytes_at_8TBps"] else "bytes"
    out.update(extra)
    print(json.dumps(out), flush=True)


def camera(a, dev):
    g = torch.Generator(device="cpu").manual_seed(20261018)
    P, K, n, levels = a.p, 16, 21, [0.1, 0.3, 0.5]
    R = a.width * a.height
    points, scaling, quaternions, strengths, spacing = model(P, K, dev, g)
    knn_idx = knn_points(points[None], points[None], K=K).idx[0]
    gidx = torch.randint(0, P, (R,), generator=g).to(dev)
    idx = knn_idx[gidx].contiguous()
    world = points[gidx] + 0.3 * spacing * torch.randn(R, 3, generator=g).to(dev)
    centre = torch.tensor([[0.0, 0.0, 8.0]], device=dev)
    factor = 1.0
    rays = torch.nn.functional.normalize(world - centre, dim=-1)
    stds = scaling[gidx].mean(-1)
    lin = torch.linspace(-3., 3., n, device=dev)
    zeros = torch.zeros_like(stds)
    native = lambda: LS.ray_level_crossings(world, rays, stds, zeros, lin, idx, points, scaling, quaternions, strengths, levels,
                                            density_factor=factor, inner_mode="second_crossing", return_normals=True, validate_idx=False)
    function = lambda: LS.level_surface_points_from_rays(world, centre, idx, points, scaling, quaternions, strengths, levels, density_factor=factor)
    eager = lambda: eager_camera_form(world, centre, idx, points, scaling, quaternions, strengths, levels, n, factor, K)
    ms, rounds = timed({"native_call": native, "function": function, "eager": eager}, {"native_call": a.reps, "function": a.reps, "eager": 1})
    f, e = function(), eager()
    agree = {}
    for lv in levels:
        same = f[lv]["valid"] == e[lv][3]
        both = f[lv]["valid"] & e[lv][3]
        mine = torch.zeros(R, 3, device=dev); mine[f[lv]["valid"]] = f[lv]["intersection_points"]
        theirs = torch.zeros(R, 3, device=dev); theirs[e[lv][3]] = e[lv][0]
        agree[str(lv)] = {"valid_equal_fraction": float(same.float().mean()), "valid_fraction": float(both.float().mean()),
                          "max_abs_point_difference_over_spacing": float((mine - theirs)[both].abs().max() / spacing) if both.any() else None}
    crossings = int(sum((native()["first_above"][l] > 0).sum() for l in range(len(levels))))
    report("camera", R, P, K, n, len(levels), ms, rounds, crossings, {"function_vs_eager": agree})


def normals(a, dev):
    g = torch.Generator(device="cpu").manual_seed(20261019)
    P, K, n, level, V = a.p_normals, 16, 21, 0.1, a.verts
    points, scaling, quaternions, strengths, spacing = model(P, K, dev, g)
    vi = torch.randint(0, P, (V,), generator=g).to(dev)
    verts = points[vi] + 0.3 * spacing * torch.randn(V, 3, generator=g).to(dev)
    nrm = torch.nn.functional.normalize(torch.randn(V, 3, generator=g)).to(dev)
    inner = (spacing * (1.5 + torch.rand(V, generator=g))).to(dev)
    outer = -inner * (0.6 + 0.8 * torch.rand(V, generator=g).to(dev))
    idx = knn_points(verts[None], points[None], K=K).idx[0]
    lin = torch.linspace(0., 1., n, device=dev)
    native = lambda: LS.ray_level_crossings(verts, nrm, inner - outer, outer, lin, idx, points, scaling, quaternions, strengths, [level],
                                            validate_idx=False)
    function = lambda: LS.level_points_along_normals(points, scaling, quaternions, strengths, verts, nrm, inner, outer, level=level)
    eager = lambda: eager_normals_form(verts, nrm, inner, outer, idx, points, scaling, quaternions, strengths, n, level, K)
    ms, rounds = timed({"native_call": native, "function": function, "eager": eager}, {"native_call": a.reps, "function": a.reps, "eager": 1})
    f, e = function(), eager()
    agree = {"outer_verts_max_abs_difference_over_spacing": float((f["outer_verts"] - e[0]).abs().max() / spacing),
             "inner_verts_max_abs_difference_over_spacing": float((f["inner_verts"] - e[1]).abs().max() / spacing),
             "outer_verts_median_abs_difference_over_spacing": float((f["outer_verts"] - e[0]).abs().median() / spacing)}
    report("normals", V, P, K, n, 1, ms, rounds, 0, {"function_vs_eager": agree, "function_includes": "both knn_points calls (native in both columns)"})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", default="both", choices=["camera", "normals", "both"])
    ap.add_argument("--p", type=int, default=3_000_000)
    ap.add_argument("--p-normals", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1056)
    ap.add_argument("--verts", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("levelset_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    if a.form in ("camera", "both"):
        camera(a, dev)
        torch.cuda.empty_cache()
    if a.form in ("normals", "both"):
        normals(a, dev)


if __name__ == "__main__":
    main()
