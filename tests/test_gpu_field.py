"""field_values / compute_density on the GPU, judged by one rule: per tensor, the L2 distance of ours to a float64
evaluation is at most twice the distance of a float32 CPU evaluation of the same function to it, plus float32 epsilon times
the tensor's norm (field_oracle.judge).  For the fixtures both evaluations are the reference's own (tests/golden/field_*.npz);
at other shapes they are tests/field_oracle.py's, which test_field_cpu.py pins to those fixtures."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import field_oracle as FO
from frosting_amd import _lib
from frosting_amd.field import compute_density, field_values
from frosting_amd.knn import knn_points

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "field_*.npz")))


def ours(inputs, idx, upstream, dev, **kw):
    """field_values on the device for the outputs that have an upstream gradient -> (outputs, gradients) as numpy arrays."""
    t = {k: torch.from_numpy(np.asarray(inputs[k], np.float32)).to(dev).requires_grad_(True) for k in FO.INPUTS}
    out = field_values(t["x"], torch.from_numpy(np.asarray(idx)).to(dev), t["points"], t["scaling"], t["quaternions"], t["strengths"],
                       return_sdf="sdf" in upstream, return_beta="beta" in upstream,
                       return_closest_gaussian_opacities="closest_gaussian_opacities" in upstream, **kw)
    assert set(out) == set(upstream) | {"density"}
    loss = sum((out[k] * torch.from_numpy(np.asarray(upstream[k], np.float32)).to(dev)).sum() for k in upstream)
    loss.backward()
    return {k: v.detach().cpu().numpy() for k, v in out.items()}, {k: t[k].grad.cpu().numpy() for k in FO.INPUTS}


def make_inputs(P, N, K, seed, flat=0.5, spread=0.5):
    """Unit-scale Gaussians, samples around some of them, the K nearest (or K random, when P < K) as neighbours."""
    g = np.random.default_rng(seed)
    points = g.standard_normal((P, 3))
    scaling = np.exp(-1.0 + flat * g.standard_normal((P, 3)))
    centre = g.integers(0, P, N)
    x = points[centre] + spread * scaling[centre].mean(-1, keepdims=True) * g.standard_normal((N, 3))
    if P >= K:
        d = ((x[:, None] - points[None]) ** 2).sum(-1)
        idx = np.argsort(d, axis=1, kind="stable")[:, :K]
    else:
        idx = g.integers(0, P, (N, K))
    inputs = dict(x=x, points=points, scaling=scaling, quaternions=g.standard_normal((P, 4)),
                  strengths=1.0 / (1.0 + np.exp(-g.standard_normal((P, 1)))))
    return {k: v.astype(np.float32).astype(np.float64) for k, v in inputs.items()}, idx.astype(np.int64)


def upstream_for(N, K, seed, keys=FO.UPSTREAM):
    g = np.random.default_rng(seed)
    shapes = {"density": (N,), "closest_gaussian_opacities": (N, K), "beta": (N,), "sdf": (N,)}
    return {k: g.standard_normal(shapes[k]).astype(np.float32).astype(np.float64) for k in keys}


def check_against_oracle(inputs, idx, upstream, dev, label, **kw):
    got_out, got_grad = ours(inputs, idx, upstream, dev, **kw)
    o64, g64 = FO.run(inputs, idx, upstream, torch.float64, **kw)
    o32, g32 = FO.run(inputs, idx, upstream, torch.float32, **kw)
    for k in o64:
        FO.judge(f"{label} {k}", got_out[k], o64[k], o32[k])
    for k in g64:
        FO.judge(f"{label} dL/d{k}", got_grad[k], g64[k], g32[k])
    return got_out, got_grad


# ---- 1. the reference's own arrays ----
@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
@pytest.mark.parametrize("mode", ["average", "weighted_average"])
@pytest.mark.parametrize("tag", ["sdf", "nosdf"])
def test_fixtures(gpu_device, path, mode, tag):
    fx = np.load(path)
    ups = {k: fx["upstream_" + k] for k in FO.UPSTREAM if not (tag == "nosdf" and k == "sdf")}
    got_out, got_grad = ours({k: fx[k] for k in FO.INPUTS}, fx["idx"], ups, gpu_device, beta_mode=mode,
                             density_factor=float(fx["density_factor"]))
    for k, v in got_out.items():
        FO.judge(f"{mode} {tag} {k}", v, fx[f"{mode}_f64_out_{k}"], fx[f"{mode}_f32_out_{k}"])
    for k, v in got_grad.items():
        FO.judge(f"{mode} {tag} dL/d{k}", v, fx[f"{mode}_{tag}_f64_grad_{k}"], fx[f"{mode}_{tag}_f32_grad_{k}"])


# ---- 2. shapes that break kernels ----
@pytest.mark.parametrize("K", [1, 3, 16, 32])
@pytest.mark.parametrize("N", [1, 63, 65, 1000, 4097])
def test_shapes(gpu_device, K, N):
    mode = "weighted_average" if (K + N) % 2 else "average"
    inputs, idx = make_inputs(300, N, K, seed=1000 * K + N)
    check_against_oracle(inputs, idx, upstream_for(N, K, 7 + N), gpu_device, f"K{K} N{N}", beta_mode=mode, density_factor=1.0 / 32)


@pytest.mark.parametrize("mode", ["average", "weighted_average"])
def test_single_gaussian_and_int32_idx(gpu_device, mode):
    # P = 1: every pair names Gaussian 0 -- duplicates inside every row and one list of N * K pairs (the hub kernel)
    inputs, idx = make_inputs(1, 300, 8, seed=5)
    check_against_oracle(inputs, idx, upstream_for(300, 8, 6), gpu_device, "P1", beta_mode=mode, density_factor=1.0 / 16)
    inputs, idx = make_inputs(200, 257, 5, seed=8)
    a = ours(inputs, idx, upstream_for(257, 5, 9), gpu_device, beta_mode=mode, density_factor=1.0 / 16)
    b = ours(inputs, idx.astype(np.int32), upstream_for(257, 5, 9), gpu_device, beta_mode=mode, density_factor=1.0 / 16)
    for x, y in zip(a, b):
        assert all(np.array_equal(x[k], y[k]) for k in x)


def test_duplicates_inside_a_row(gpu_device):
    inputs, idx = make_inputs(100, 500, 16, seed=11)
    idx[:, 8:] = idx[:, :8]
    check_against_oracle(inputs, idx, upstream_for(500, 16, 12), gpu_device, "dup", beta_mode="weighted_average", density_factor=1.0 / 16)


def _backward_raw(inputs, idx, upstream, dev, mode_code, fill=None, density_factor=1.0 / 16):
    """frg_field_backward through ctypes with the outputs (and optionally the workspace) pre-filled -> the five gradient
    tensors on the device."""
    L = _lib.lib()
    t = {k: torch.from_numpy(np.asarray(inputs[k], np.float32)).to(dev) for k in FO.INPUTS}
    up = {k: torch.from_numpy(np.asarray(v, np.float32)).to(dev) for k, v in upstream.items()}
    idx_t = torch.from_numpy(idx).to(dev)
    N, K = idx.shape
    P = t["points"].shape[0]
    outs = {k: torch.full(shape, float("nan"), device=dev) for k, shape in
            dict(dL_dx=(N, 3), dL_dpoints=(P, 3), dL_dscaling=(P, 3), dL_dquaternions=(P, 4), dL_dstrengths=(P,)).items()}
    need = int(L.frg_field_workspace_bytes(P, N, K, 1))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=dev)
    if fill is not None:
        ws.copy_(torch.from_numpy(np.random.default_rng(fill).integers(0, 256, ws.numel(), dtype=np.uint8)).to(dev))
    base = (ws.data_ptr() + 255) // 256 * 256
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    fallback = t["scaling"].min(-1)[0].max().reshape(1)
    ptr = lambda v: v.data_ptr()
    a = _lib.FieldArgs(struct_size=C.sizeof(_lib.FieldArgs), P=P, N=N, K=K, idx_is_int64=1, idx=ptr(idx_t), x=ptr(t["x"]),
                       points=ptr(t["points"]), scaling=ptr(t["scaling"]), quaternions=ptr(t["quaternions"]), strengths=ptr(t["strengths"]),
                       beta_mode=mode_code, density_threshold=1.0, density_factor=density_factor, opacity_min_clamp=1e-16,
                       beta_fallback=ptr(fallback), dL_ddensity=ptr(up["density"]), dL_dopacities=ptr(up["closest_gaussian_opacities"]),
                       dL_dbeta=ptr(up["beta"]), dL_dsdf=ptr(up["sdf"]), bad_index=ptr(bad), workspace=base,
                       workspace_bytes=need, hip_stream=torch.cuda.current_stream(dev).cuda_stream,
                       **{k: ptr(v) for k, v in outs.items()})
    _lib.check(L.frg_field_backward(C.byref(a)), "frg_field_backward")
    torch.cuda.synchronize(dev)
    assert int(bad.item()) == 0
    return outs


def test_unnamed_gaussians_get_exact_zeros_over_nan(gpu_device):
    inputs, idx = make_inputs(600, 300, 4, seed=21)
    named = np.zeros(600, bool)
    named[idx.ravel()] = True
    assert (~named).sum() > 20
    outs = _backward_raw(inputs, idx, upstream_for(300, 4, 22), gpu_device, 2)
    for k in ("dL_dpoints", "dL_dscaling", "dL_dquaternions", "dL_dstrengths"):
        v = outs[k].cpu().numpy().reshape(600, -1)
        assert np.isfinite(v).all(), k
        assert (v[~named] == 0.0).all() and not np.signbit(v[~named]).any(), k
        assert np.count_nonzero(np.abs(v[named]).sum(-1)) > named.sum() // 2, k
    assert np.isfinite(outs["dL_dx"].cpu().numpy()).all()


def test_hub_gaussian(gpu_device):
    # Gaussian 0 is named by 5000 pairs (column 0 of every row), every other Gaussian of the table once
    N, K, P = 5000, 2, 5001
    inputs, _ = make_inputs(P, 1, 1, seed=31)
    idx = np.stack([np.zeros(N, np.int64), np.arange(1, N + 1, dtype=np.int64)], axis=1)
    g = np.random.default_rng(32)
    inputs["x"] = (inputs["points"][idx[:, 1]] * 0.5 + 0.5 * inputs["points"][0] +
                   0.3 * g.standard_normal((N, 3))).astype(np.float32).astype(np.float64)
    for mode in ("average", "weighted_average"):
        check_against_oracle(inputs, idx, upstream_for(N, K, 33), gpu_device, f"hub {mode}", beta_mode=mode, density_factor=0.25)


def test_scale_below_the_clamp(gpu_device):
    inputs, idx = make_inputs(200, 400, 8, seed=41)
    inputs["scaling"][::7, 1] = np.float64(np.float32(3e-9))
    _, grads = check_against_oracle(inputs, idx, upstream_for(400, 8, 42, keys=("density", "closest_gaussian_opacities")), gpu_device,
                                    "clamp", beta_mode="average", density_factor=1.0 / 16)
    assert (grads["scaling"][::7, 1] == 0.0).all()
    # with a beta the tiny component is the minimum: it receives beta's gradient and nothing else
    _, grads = check_against_oracle(inputs, idx, upstream_for(400, 8, 42), gpu_device, "clamp+beta", beta_mode="average", density_factor=1.0 / 16)


@pytest.mark.parametrize("mode", ["average", "weighted_average"])
def test_far_samples_underflow(gpu_device, mode):
    inputs, idx = make_inputs(200, 300, 8, seed=51)
    inputs["x"][::2] += 500.0                                    # every opacity of these rows underflows to 0
    out, _ = check_against_oracle(inputs, idx, upstream_for(300, 8, 52), gpu_device, f"far {mode}", beta_mode=mode, density_factor=1.0 / 16)
    assert (out["density"][::2] == 0.0).all()
    want_sdf = out["beta"][::2] * np.float32(np.sqrt(-2.0 * np.log(1e-16)))
    np.testing.assert_allclose(out["sdf"][::2], want_sdf, rtol=1e-6)
    if mode == "weighted_average":                                # the fallback: the largest min-scale among the named Gaussians
        assert (out["beta"][::2] == np.float32(inputs["scaling"].min(-1)[np.unique(idx)].max())).all()


# ---- 3. densities >= 1 ----
def _dense_case():
    """Two clusters 10 apart: 200 samples ON centres of strong, wide Gaussians (densities >= 1 at density_factor 1) and 400
    samples among weak ones (16 x 0.05 < 1); the K nearest Gaussians of a sample lie in its own cluster."""
    inputs, _ = make_inputs(300, 1, 1, seed=61)
    g = np.random.default_rng(64)
    inputs["points"][150:, 0] += 10.0
    inputs["strengths"][:150], inputs["strengths"][150:] = np.float32(0.9), np.float32(0.05)
    inputs["scaling"][:150] = np.maximum(inputs["scaling"][:150], np.float64(np.float32(0.4)))
    big = np.arange(600) % 3 == 0
    centre = np.where(big, g.integers(0, 150, 600), g.integers(150, 300, 600))
    x = inputs["points"][centre] + np.where(big, 0.0, 0.3)[:, None] * g.standard_normal((600, 3))
    inputs["x"] = x.astype(np.float32).astype(np.float64)
    d = ((inputs["x"][:, None] - inputs["points"][None]) ** 2).sum(-1)
    idx = np.argsort(d, axis=1, kind="stable")[:, :16].astype(np.int64)
    assert (idx[big] < 150).all() and (idx[~big] >= 150).all()
    return inputs, idx, big


@pytest.mark.parametrize("mode", ["average", "weighted_average"])
def test_dense_rows_forward(gpu_device, mode):
    inputs, idx, big = _dense_case()
    t = {k: torch.from_numpy(v.astype(np.float32)).to(gpu_device) for k, v in inputs.items()}
    out = field_values(t["x"], torch.from_numpy(idx).to(gpu_device), t["points"], t["scaling"], t["quaternions"], t["strengths"],
                       beta_mode=mode, return_beta=True, density_factor=1.0)
    ups = upstream_for(600, 16, 62, keys=("density", "beta", "sdf"))
    o64, _ = FO.run(inputs, idx, ups, torch.float64, beta_mode=mode)
    o32, _ = FO.run(inputs, idx, ups, torch.float32, beta_mode=mode)          # (its gradients are not finite: not looked at)
    assert (o64["density"][big] >= 1.0).sum() > 50 and (o64["density"] < 1.0).sum() > 50
    for k in ("density", "beta", "sdf"):
        FO.judge(f"dense {mode} {k}", out[k].cpu().numpy(), o64[k], o32[k])


def test_dense_rows_do_not_disturb_the_others(gpu_device):
    inputs, idx, _ = _dense_case()
    ups = upstream_for(600, 16, 63)
    o64, _ = FO.run(inputs, idx, {"density": ups["density"]}, torch.float64)
    big = o64["density"] >= 0.999                                 # with a margin: the GPU's float32 sum decides for itself
    assert big.sum() > 50 and (~big).sum() > 50
    _, mixed = ours(inputs, idx, ups, gpu_device, beta_mode="weighted_average")
    assert all(np.isfinite(v).all() for v in mixed.values())      # finite everywhere, the dense rows included
    sub = dict(inputs, x=inputs["x"][~big])
    _, alone = ours(sub, idx[~big], {k: v[~big] for k, v in ups.items()}, gpu_device, beta_mode="weighted_average")
    touched = np.zeros(300, bool)
    touched[idx[big].ravel()] = True
    only_small = ~touched
    only_small[np.setdiff1d(np.arange(300), np.unique(idx[~big]))] = False
    assert only_small.sum() > 10
    for k in ("points", "scaling", "quaternions", "strengths"):
        assert np.array_equal(mixed[k][only_small].view(np.uint32), alone[k][only_small].view(np.uint32)), k
    assert np.array_equal(mixed["x"][~big].view(np.uint32), alone["x"].view(np.uint32))


# ---- 4. reproducibility ----
def test_backward_is_bit_reproducible(gpu_device):
    inputs, idx = make_inputs(500, 4097, 16, seed=71)
    idx[:2000, 0] = 3                                             # a list long enough for the hub kernel beside short ones
    ups = upstream_for(4097, 16, 72)
    runs = [_backward_raw(inputs, idx, ups, gpu_device, 2, fill=f) for f in (None, None, 1234)]
    for k in runs[0]:
        a = runs[0][k].cpu().numpy().view(np.uint32)
        assert np.isfinite(runs[0][k].cpu().numpy()).all()
        assert np.array_equal(a, runs[1][k].cpu().numpy().view(np.uint32)), k
        assert np.array_equal(a, runs[2][k].cpu().numpy().view(np.uint32)), f"{k}: depends on the workspace's contents"


# ---- 5. autograd ----
def test_autograd_surface(gpu_device):
    inputs, idx = make_inputs(300, 1000, 16, seed=81)
    t = {k: torch.from_numpy(v.astype(np.float32)).to(gpu_device).requires_grad_(True) for k, v in inputs.items()}
    idx_t = torch.from_numpy(idx).to(gpu_device)
    args = (t["x"], idx_t, t["points"], t["scaling"], t["quaternions"], t["strengths"])
    field_values(*args, density_factor=1.0 / 16)["sdf"].sum().backward()
    for k, v in t.items():
        assert v.grad is not None and v.grad.shape == v.shape and torch.isfinite(v.grad).all() and v.grad.abs().sum() > 0, k
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu_device)
    before = torch.cuda.memory_allocated(gpu_device)
    only = field_values(*args, return_sdf=False, density_factor=1.0 / 16)
    assert set(only) == {"density"}
    P, N, K = 300, 1000, 16
    ws = int(_lib.lib().frg_field_workspace_bytes(P, N, K, 0))
    # the density, the contiguous float copies autograd saves (none: the inputs are float32 and contiguous), the flag, the workspace
    assert torch.cuda.max_memory_allocated(gpu_device) - before <= N * 4 + ws + 256 + 4096
    fn = only["density"].grad_fn
    assert fn is not None
    d = compute_density(*args, density_factor=1.0 / 16)
    assert torch.equal(d, only["density"])
    d2, o2 = compute_density(*args, density_factor=1.0 / 16, return_closest_gaussian_opacities=True)
    assert torch.equal(d2, d) and o2.shape == (N, K)
    with pytest.raises(IndexError):
        bad = idx_t.clone()
        bad[17, 3] = 300
        field_values(t["x"], bad, *args[2:])
    with pytest.raises(NotImplementedError, match="learnable"):
        field_values(*args, beta_mode="learnable")
    assert set(field_values(*args, beta_mode="learnable", return_sdf=False)) == {"density"}


# ---- 6. with the real consumer ----
def test_with_knn_points(gpu_device):
    inputs, _ = make_inputs(3000, 1, 1, seed=91)
    pts = torch.from_numpy(inputs["points"].astype(np.float32)).to(gpu_device)
    knn_idx = knn_points(pts[None], pts[None], K=16).idx[0]
    g = np.random.default_rng(92)
    gaussian_idx = torch.from_numpy(g.integers(0, 3000, 2000)).to(gpu_device)
    idx = knn_idx[gaussian_idx]
    centre = gaussian_idx.cpu().numpy()
    x = inputs["points"][centre] + 0.5 * inputs["scaling"][centre].mean(-1, keepdims=True) * g.standard_normal((2000, 3))
    inputs["x"] = x.astype(np.float32).astype(np.float64)
    for mode in ("average", "weighted_average"):
        check_against_oracle(inputs, idx.cpu().numpy(), upstream_for(2000, 16, 93), gpu_device, f"knn {mode}", beta_mode=mode,
                             density_factor=1.0 / 16)
