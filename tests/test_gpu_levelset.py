"""Level crossings along rays on the GPU (frosting_amd.levelset, csrc/levelset.hip).

Floats are judged by the project's rule (levelset_oracle.judge = field_oracle.judge): the L2 distance of ours to a float64
evaluation is at most twice the distance of a float32 CPU evaluation of the same function to it, plus float32 epsilon times
the tensor's norm.  For the fixtures both evaluations are the reference's own (tests/golden/levelset_*.npz); elsewhere they
are tests/levelset_oracle.py's, which test_levelset_cpu.py pins to those fixtures.  Discrete results (first / last sample
above the level, under_first, valid, empty) must be EQUAL on every ray that is not set aside; a ray is set aside only if
the yardstick's own two precisions disagree on it or one of its float64 densities lies within tau of a level, tau = 4 x the
largest |f32 - f64| density difference of the yardstick, and at most 1 % of the rays may be.  The search itself is also
checked free of rounding: against the oracle's search applied to the densities the kernel returned."""
import ctypes as C
import glob
import itertools
import os

import numpy as np
import pytest
import torch

import levelset_oracle as LO
from frosting_amd import _lib
from frosting_amd import levelset as LS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "levelset_*.npz")))
MODEL = ("points", "scaling", "quaternions", "strengths")
ORDER = ("origins", "directions", "t_scale", "t_offset", "lin", "idx") + MODEL
DISCRETE = ("first_above", "last_above", "under_first")


def run_kernel(arrays, levels, mode, dev, density_factor=1.0, **kw):
    t = LO.tensors(arrays, torch.float32)
    out = LS.ray_level_crossings(*[t[k].to(dev) for k in ORDER], levels, density_factor=density_factor, inner_mode=mode,
                                 return_normals=True, return_densities=True, **kw)
    return {k: v.cpu() for k, v in out.items()}


def make_inputs(P, R, K, n, seed):
    """Gaussians of scale ~0.15 in a unit box, rays through it whose ranges straddle a few of them."""
    g = np.random.default_rng(seed)
    a = dict(points=g.uniform(-1, 1, (P, 3)), scaling=np.exp(-1.9 + 0.4 * g.standard_normal((P, 3))),
             quaternions=g.standard_normal((P, 4)), strengths=1 / (1 + np.exp(-1 - g.standard_normal((P, 1)))))
    centre = g.integers(0, P, R)
    d = g.standard_normal((R, 3))
    a["directions"] = d / np.linalg.norm(d, axis=-1, keepdims=True) * g.uniform(0.8, 1.2, (R, 1))      # used as given
    a["origins"] = a["points"][centre] + 0.05 * g.standard_normal((R, 3))
    a["t_scale"], a["t_offset"] = g.uniform(0.6, 1.2, R), -g.uniform(0.3, 0.6, R)
    a["lin"] = np.linspace(0, 1, n)
    a = {k: v.astype(np.float32) for k, v in a.items()}
    if P >= K:
        a["idx"] = LO.KO.knn_points(a["origins"], a["points"], K)[1]
    else:
        a["idx"] = g.integers(0, P, (R, K))
    return a


def near_level(dens64, levels, tau):
    """[L,R]: a float64 density of the ray lies within tau of the level"""
    return np.stack([(np.abs(dens64 - lv) <= tau).any(-1) for lv in levels])


def check_search(got, arrays, levels, mode, label):
    """The search and the interpolation against the oracle's, applied in float32 to the densities the kernel returned:
    indices and flags equal on every ray, t within 4 eps32 max(|t0|, |t1|) of the bracket's samples (one fused rounding of
    `* (t1 - t0) + t0` is at most one ulp of a product bounded by 2 max(|t0|, |t1|); doubled)."""
    t32 = LO.tensors(arrays, torch.float32)
    ts = LO.sample_t(t32["lin"], t32["t_scale"], t32["t_offset"])
    n = ts.shape[1]
    for l, lv in enumerate(levels):
        want = LO.search(got["densities"], ts, lv, mode)
        for k in DISCRETE:
            assert torch.equal(got[k][l].to(want[k].dtype), want[k]), (label, lv, k)
        f, la = want["first_above"], want["last_above"]
        at = lambda i: ts.gather(1, i.clamp(0, n - 1)[:, None])[:, 0].abs()
        for k, bound in (("t_outer", torch.maximum(at(f - 1), at(f))), ("t_inner", torch.maximum(at(la), at(la + 1)))):
            err = (got[k][l] - want[k]).abs()
            assert torch.isfinite(got[k][l]).all() and bool((err <= 4 * LO.EPS32 * bound).all()), (label, lv, k, float(err.max()))
        exact = (f == 0)
        assert torch.equal(got["t_outer"][l][exact], ts[:, 0][exact]) and torch.equal(got["t_inner"][l][la == n - 1], ts[:, -1][la == n - 1])
        assert not got["normals"][l][exact].any()


def check_against_oracle(arrays, levels, mode, dev, label, density_factor=1.0, **kw):
    got = run_kernel(arrays, levels, mode, dev, density_factor, **kw)
    o64 = LO.crossings(LO.tensors(arrays, torch.float64), levels, mode, density_factor)
    o32 = LO.crossings(LO.tensors(arrays, torch.float32), levels, mode, density_factor)
    LO.judge(f"{label} densities", got["densities"], o64["densities"], o32["densities"])
    check_search(got, arrays, levels, mode, label)
    tau = 4 * float((o32["densities"].double() - o64["densities"]).abs().max())
    aside = torch.from_numpy(near_level(o64["densities"].numpy(), levels, tau))
    for k in DISCRETE:
        aside |= o64[k] != o32[k]
    assert aside.float().mean() <= 0.01, (label, float(aside.float().mean()))
    keep = ~aside
    for k in DISCRETE:
        assert torch.equal(got[k].to(o64[k].dtype)[keep], o64[k][keep]), (label, k)
    if keep.any():
        for k in ("t_outer", "t_inner", "normals"):
            LO.judge(f"{label} {k}", got[k][keep], o64[k][keep], o32[k][keep])
    return got


# ---- 1. + 2. the reference's own arrays ----
@pytest.fixture
def spy(monkeypatch):
    """Records the arguments and the result of the native call the Python-level functions make (densities switched on)."""
    calls = []
    inner = LS.ray_level_crossings

    def recording(*a, **kw):
        kw["return_densities"] = True
        out = inner(*a, **kw)
        calls.append((a, out))
        return out
    monkeypatch.setattr(LS, "ray_level_crossings", recording)
    return calls


def _judge_rows(label, ours, ours_mask, fx, tag, key, keep):
    """A compacted output against the fixture's two arrays, on the kept rays: scattered back to one row per ray first."""
    R = len(keep)
    full = lambda rows, mask: _scatter(rows, mask, R)
    m64, m32 = ~fx[f"{tag}_f64_empty"], ~fx[f"{tag}_f32_empty"]
    a, b, c = full(ours, ours_mask), full(fx[f"{tag}_f64_{key}"], m64), full(fx[f"{tag}_f32_{key}"], m32)
    rows = keep & m64
    LO.judge(label, a[rows], b[rows], c[rows])


def _scatter(rows, mask, R):
    out = np.zeros((R,) + rows.shape[1:], np.float64)
    out[mask] = rows
    return out


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
def test_fixtures(gpu_device, spy, path):
    fx = np.load(path)
    dev = gpu_device
    g = lambda k: torch.from_numpy(fx[k]).to(dev)
    model = [g(k) for k in MODEL]
    n, levels, tau = int(fx["n"]), [float(v) for v in fx["levels"]], float(fx["tau"])
    camera = str(fx["kind"]) == "camera"
    if camera:
        out = LS.level_surface_points_from_rays(g("world_points"), g("camera_center"), g("idx"), *model, levels, n_points_in_range=n,
                                                range_size=float(fx["range_size"]), density_factor=float(fx["density_factor"]),
                                                return_normals=True, use_last_intersection_as_inner_level_point=bool(fx["last"]))
        tags = [f"level{lv}" for lv in levels]
    else:
        extra = {k: g(k) for k in ("min_clamping_inner_dist", "max_clamping_outer_dist") if k in fx}
        out = LS.level_points_along_normals(*model, g("verts"), g("normals"), g("inner_range"), g("outer_range"), n_samples_per_vertex=n,
                                            n_closest_gaussians_to_use=int(fx["K"]), level=levels[0], smooth_points=bool(fx["smooth"]),
                                            use_last_intersection_as_inner_level_point=bool(fx["last"]),
                                            min_layer_size=float(fx["min_layer_size"]), spatial_extent=float(fx["spatial_extent"]), **extra)
        tags = ["run"]
    (args, raw), = spy
    assert torch.equal(args[5].cpu(), torch.from_numpy(fx["idx"]))          # the neighbour table (ours, along normals)
    raw = {k: v.cpu().numpy() for k, v in raw.items()}
    for l, tag in enumerate(tags):
        d64, d32 = fx[f"{tag}_f64_densities"], fx[f"{tag}_f32_densities"]
        LO.judge(f"{tag} densities", raw["densities"], d64, d32)
        aside = (np.abs(d64 - levels[l]) <= tau).any(-1)
        for k in ("first_above", "last_above", "under_first", "empty"):
            aside |= fx[f"{tag}_f64_{k}"] != fx[f"{tag}_f32_{k}"]
        print(f"{tag}: {int(aside.sum())} of {len(aside)} rays set aside")
        assert aside.mean() <= 0.01
        keep = ~aside
        for k in DISCRETE:
            assert np.array_equal(raw[k][l][keep], fx[f"{tag}_f64_{k}"][keep]), (tag, k)
        if camera:
            o = out[levels[l]]
            valid = o["valid"].cpu().numpy()
            assert np.array_equal(valid[keep], ~fx[f"{tag}_f64_empty"][keep])
            for k in ("intersection_points", "inner_intersection_points", "normals"):
                _judge_rows(f"{tag} {k}", o[k].cpu().numpy(), valid, fx, tag, k, keep)
        else:
            empty = (raw["first_above"][l] == 0) & (raw["last_above"][l] == n - 1) & raw["under_first"][l]
            assert np.array_equal(empty[keep], fx[f"{tag}_f64_empty"][keep])
            if bool(fx["smooth"]):                              # a smoothed vertex mixes its four nearest: all of them kept
                keep = keep[LO.KO.knn_points(fx["verts"], fx["verts"], 4)[1]].all(1)
            for k in ("outer_dist", "inner_dist", "outer_verts", "inner_verts"):
                LO.judge(f"{tag} {k}", out[k].cpu().numpy()[keep], fx[f"{tag}_f64_{k}"][keep], fx[f"{tag}_f32_{k}"][keep])


# ---- 3. the search, free of rounding: planted densities ----
@pytest.mark.parametrize("mode", ["last", "second_crossing"])
def test_search_on_planted_densities(gpu_device, mode):
    """Ray r runs along z from (10 r, 0, 0) with t_j = lin[j]; Gaussian (r, j) sits exactly on sample j with scale 0.002 (the
    next sample is 25 scales away: exp(-312) is 0 in float32) and strength v[r][j]: dens[r][j] is v[r][j] to the bit."""
    n, level = 21, 0.1
    lv = np.float32(level)
    g = np.random.default_rng(3)
    planted = np.full((9, n), 0.05, np.float32)
    planted[1] = 0.2                                   # all above
    planted[2, 0] = 0.2                                # above only at 0
    planted[3, n - 1] = 0.2                            # above only at n - 1
    planted[4, 7] = 0.3                                # one spike
    planted[5, 4:7] = 0.3; planted[5, 12:15] = 0.25    # two bumps
    planted[6, 5:9] = 0.3; planted[6, 9] = lv          # equal to the level behind a bump: neither under nor above
    planted[7, 6] = lv; planted[7, 7:10] = 0.2         # equal to the level in front of a bump
    planted[8, 3:6] = 1.5; planted[8, 10] = 1.0        # >= 1
    v = np.concatenate([planted, g.uniform(0.0, 0.25, (200, n)).astype(np.float32)])
    R = len(v)
    lin = np.linspace(0, 1, n).astype(np.float32)
    mu = np.zeros((R, n, 3), np.float32)
    mu[..., 0] = 10.0 * np.arange(R)[:, None]
    mu[..., 2] = lin[None]
    arrays = dict(origins=mu[:, 0].copy(), directions=np.tile(np.float32([0, 0, 1]), (R, 1)), t_scale=np.ones(R, np.float32),
                  t_offset=np.zeros(R, np.float32), lin=lin, idx=np.arange(R * n).reshape(R, n),
                  points=mu.reshape(-1, 3), scaling=np.full((R * n, 3), 0.002, np.float32),
                  quaternions=np.tile(np.float32([1, 0, 0, 0]), (R * n, 1)), strengths=v.reshape(-1, 1))
    arrays["origins"][:, 2] = 0
    levels = [level, 0.2]
    got = run_kernel(arrays, levels, mode, gpu_device)
    want = np.where(v >= 1, np.float32(1), v)
    assert np.array_equal(got["densities"].numpy(), want)
    check_search(got, arrays, levels, mode, mode)
    f, la, u = (got[k][0].numpy()[:9] for k in DISCRETE)
    second = mode == "second_crossing"
    assert f.tolist() == [0, 0, 0, n - 1, 7, 4, 5, 7, 3]
    assert la.tolist() == ([n - 1, n - 1, n - 1, n - 1, 7, 6, n - 1, 9, 5] if second else [n - 1, n - 1, 0, n - 1, 7, 14, 8, 9, 10])
    assert u.tolist() == [True, False, False, True, True, True, True, True, True]


# ---- 4. shapes that break kernels ----
_N, _L = (2, 7, 21, 32), (1, 3, 8)


@pytest.mark.parametrize("K", [1, 3, 16, 32])
@pytest.mark.parametrize("R", [1, 63, 65, 1000, 4097])
def test_shapes(gpu_device, K, R):
    case = [1, 63, 65, 1000, 4097].index(R) * 4 + [1, 3, 16, 32].index(K)
    n, nl = _N[case % 4 if case < 16 else (case + 1) % 4], _L[case % 3]
    mode = "second_crossing" if case % 2 else "last"
    levels = list(np.linspace(0.05, 0.6, nl))
    check_against_oracle(make_inputs(300, R, K, n, seed=1000 * K + R), levels, mode, gpu_device, f"K{K} R{R} n{n} L{nl} {mode}",
                         density_factor=0.5 if case % 3 == 0 else 1.0)


@pytest.mark.parametrize("mode", ["last", "second_crossing"])
def test_single_gaussian_duplicates_and_int32_idx(gpu_device, mode):
    check_against_oracle(make_inputs(1, 300, 8, 21, seed=5), [0.1, 0.4], mode, gpu_device, "P1")
    a = make_inputs(100, 500, 16, 21, seed=11)
    a["idx"][:, 8:] = a["idx"][:, :8]
    check_against_oracle(a, [0.1, 0.3, 0.5], mode, gpu_device, "dup")
    a = make_inputs(200, 257, 5, 7, seed=8)
    x = run_kernel(a, [0.1, 0.3], mode, gpu_device)
    y = run_kernel(dict(a, idx=a["idx"].astype(np.int32)), [0.1, 0.3], mode, gpu_device)
    z = run_kernel(a, [0.1, 0.3], mode, gpu_device)
    for k in x:
        assert torch.equal(x[k], y[k]) and torch.equal(x[k], z[k]), k          # same bits: int32 idx, and a second run


# ---- 5. output handling ----
OUTPUTS = (("densities", torch.float32), ("t_outer", torch.float32), ("t_inner", torch.float32), ("first_above", torch.int32),
           ("last_above", torch.int32), ("under_first", torch.uint8), ("normals", torch.float32))


def _raw_call(t, levels, wanted, dev, K, n):
    """frg_levelset through ctypes with only `wanted` outputs given -> {name: tensor}; the others are NULL."""
    lib = _lib.lib()
    R, P, L = t["origins"].shape[0], t["points"].shape[0], len(levels)
    shapes = dict(densities=(R, n), t_outer=(L, R), t_inner=(L, R), first_above=(L, R), last_above=(L, R), under_first=(L, R), normals=(L, R, 3))
    outs = {k: torch.full(shapes[k], 77, dtype=dt, device=dev) for k, dt in OUTPUTS if k in wanted}
    ws = torch.empty(int(lib.frg_levelset_workspace_bytes(P, R, K, 0)) + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    a = _lib.LevelsetArgs(struct_size=C.sizeof(_lib.LevelsetArgs), P=P, R=R, K=K, n=n, L=L, idx_is_int64=1, inner_mode=1,
                          levels=(C.c_double * 8)(*levels), density_factor=1.0, bad_index=bad.data_ptr(), workspace=base,
                          workspace_bytes=ws.numel() - (base - ws.data_ptr()), hip_stream=torch.cuda.current_stream(dev).cuda_stream,
                          **{k: t[k].data_ptr() for k in ORDER}, **{k: v.data_ptr() for k, v in outs.items()})
    assert lib.frg_levelset(C.byref(a)) == 0, _lib.last_error()
    torch.cuda.synchronize(dev)
    assert int(bad.item()) == 0
    return outs


def test_every_subset_of_outputs(gpu_device):
    arrays = make_inputs(120, 130, 6, 9, seed=21)
    t = {k: v.to(gpu_device).contiguous() for k, v in LO.tensors(arrays, torch.float32).items()}
    t["strengths"] = t["strengths"].reshape(-1)
    names = [k for k, _ in OUTPUTS]
    levels = [0.1, 0.3]
    with torch.cuda.device(gpu_device):
        full = _raw_call(t, levels, names, gpu_device, 6, 9)
        assert full["first_above"].max() > 0 and (full["normals"] != 77).all()
        for r in range(len(names)):
            for wanted in itertools.combinations(names, r):
                got = _raw_call(t, levels, wanted, gpu_device, 6, 9)
                for k in wanted:
                    assert torch.equal(got[k], full[k]), (wanted, k)


def test_bad_index(gpu_device):
    arrays = make_inputs(50, 200, 4, 21, seed=31)
    P = 50
    arrays["idx"][3, 1], arrays["idx"][150, 0] = P, -1
    with pytest.raises(IndexError):
        run_kernel(arrays, [0.1], "last", gpu_device)
    got = run_kernel(arrays, [0.1], "last", gpu_device, validate_idx=False)
    # the same call with those pairs pointing at a Gaussian of strength 0
    clean = {k: v.copy() for k, v in arrays.items()}
    clean["points"] = np.concatenate([arrays["points"], np.zeros((1, 3), np.float32)])
    clean["scaling"] = np.concatenate([arrays["scaling"], np.ones((1, 3), np.float32)])
    clean["quaternions"] = np.concatenate([arrays["quaternions"], np.float32([[1, 0, 0, 0]])])
    clean["strengths"] = np.concatenate([arrays["strengths"], np.zeros((1, 1), np.float32)])
    clean["idx"][3, 1] = clean["idx"][150, 0] = P
    want = run_kernel(clean, [0.1], "last", gpu_device)
    for k in got:
        assert torch.equal(got[k], want[k]), k
    t = {k: v.to(gpu_device) for k, v in LO.tensors(arrays, torch.float32).items()}
    t.update({k: t[k][:0] for k in ("origins", "directions", "t_scale", "t_offset", "idx")})          # no rays: nothing launched
    empty = LS.ray_level_crossings(*[t[k] for k in ORDER], [0.1])
    assert empty["t_outer"].shape == (1, 0)


# ---- 6. end to end ----
def test_along_normals_end_to_end(gpu_device):
    """2 000 vertices over 5 000 Gaussians: our knn_points' table inside level_points_along_normals against the oracle fed a
    brute-force table.  Vertices whose K-th and (K+1)-th neighbour distances tie (either table) are set aside."""
    V, P, K, n, level = 2000, 5000, 16, 21, 0.1
    g = np.random.default_rng(77)
    pts = g.standard_normal((P, 3))
    pts = (pts / np.linalg.norm(pts, axis=-1, keepdims=True) * (1 + 0.01 * g.standard_normal((P, 1)))).astype(np.float32)
    nrm = g.standard_normal((V, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=-1, keepdims=True)).astype(np.float32)
    a = dict(points=pts, scaling=np.exp(-3.3 + 0.4 * g.standard_normal((P, 3))).astype(np.float32),
             quaternions=g.standard_normal((P, 4)).astype(np.float32), strengths=(1 / (1 + np.exp(-1 - g.standard_normal((P, 1))))).astype(np.float32))
    verts = (nrm * (1 + 0.005 * g.standard_normal((V, 1)))).astype(np.float32)
    inner = g.uniform(0.08, 0.15, V).astype(np.float32)
    outer = (-inner * g.uniform(0.6, 1.4, V)).astype(np.float32)
    d, idx = LO.KO.knn_points(verts, pts, K + 1)
    ds, near = LO.KO.knn_points(verts, verts, 5)
    ties = (d[:, K - 1] == d[:, K]) | (ds[:, 3] == ds[:, 4])
    dev = gpu_device
    to = lambda v: torch.from_numpy(v).to(dev)
    out = LS.level_points_along_normals(*[to(a[k]) for k in MODEL], to(verts), to(nrm), to(inner), to(outer), n_samples_per_vertex=n,
                                        n_closest_gaussians_to_use=K, level=level)
    ref = {}
    for dt in (torch.float64, torch.float32):
        c = lambda v: torch.from_numpy(v).to(dt)
        ref[dt] = LO.level_points_along_normals(*[c(a[k]) for k in MODEL], c(verts), c(nrm), c(inner), c(outer), n_samples_per_vertex=n,
                                                n_closest_gaussians_to_use=K, level=level, idx=torch.from_numpy(idx[:, :K]))
    r64, r32 = ref[torch.float64], ref[torch.float32]
    tau = 4 * float((r32["densities"].double() - r64["densities"]).abs().max())
    aside = ties | near_level(r64["densities"].numpy(), [level], tau)[0]
    for k in DISCRETE + ("empty",):
        aside |= (r64[k] != r32[k]).numpy()
    print(f"{int(ties.sum())} ties, {int(aside.sum())} of {V} vertices set aside")
    assert aside.mean() <= 0.01
    keep = ~aside[near[:, :4]].any(1)                        # a smoothed vertex mixes its four nearest
    assert keep.mean() > 0.9
    for k in ("outer_dist", "inner_dist", "outer_verts", "inner_verts"):
        LO.judge(k, out[k].cpu().numpy()[keep], r64[k].numpy()[keep], r32[k].numpy()[keep])
