"""Fixtures for the density / SDF field, produced by the reference's OWN SuGaR.get_field_values run on the CPU.

frosting_scene/sugar_model.py is imported where this tool runs, with the modules this platform lacks stubbed in
sys.modules (open3d, pytorch3d.*, simple_knn._C, diff_gaussian_rasterization, frosting_scene.gs_model,
frosting_scene.cameras: none of them is reached by the calls made here).  Its functions run unbound on a stand-in object
that carries beta_mode, scaling, strengths and points; the inverse scaled rotation is passed in, built here as
A = R(q) diag(1 / max(s, 1e-8)) with tests/field_oracle.py's restatement of quaternion_to_matrix.  Nothing of the
reference's text is written anywhere -- only the arrays that go in and come out (tests/golden/field_*.npz): per beta mode
the float64 outputs and autograd gradients for fixed upstream gradients, with and without the sdf, the same function's
float32 CPU results, and the sha256 of the file that produced them.

    python tools/make_golden_field.py          # needs the reference (FROSTING_REFERENCE, default /root/reference)
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

import field_oracle as FO  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
MODES = ("average", "weighted_average")


class _Stub(types.ModuleType):
    """A module any name can be imported from."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


def load_reference():
    for name in ("open3d", "pytorch3d", "pytorch3d.renderer", "pytorch3d.structures", "pytorch3d.transforms", "pytorch3d.ops",
                 "simple_knn", "simple_knn._C", "diff_gaussian_rasterization", "frosting_scene.gs_model", "frosting_scene.cameras"):
        sys.modules[name] = _Stub(name)
    sys.path.insert(0, REF)
    from frosting_scene.sugar_model import SuGaR
    path = os.path.join(REF, "frosting_scene", "sugar_model.py")
    return SuGaR, hashlib.sha256(open(path, "rb").read()).hexdigest()


def reference_run(SuGaR, inputs, idx, upstream, beta_mode, dtype, density_factor):
    """-> (outputs, gradients) of the reference's function in `dtype`, as float64 arrays."""
    t = {k: torch.from_numpy(inputs[k]).to(dtype).requires_grad_(True) for k in FO.INPUTS}
    fake = SimpleNamespace(beta_mode=beta_mode, scaling=t["scaling"], strengths=t["strengths"], points=t["points"])
    fake.get_beta = lambda *a, **k: SuGaR.get_beta(fake, *a, **k)
    inv = FO.inv_scaled_rotation(t["scaling"], t["quaternions"])
    fields = SuGaR.get_field_values(fake, t["x"], closest_gaussians_idx=torch.from_numpy(idx), gaussian_inv_scaled_rotation=inv,
                                    return_sdf="sdf" in upstream, density_factor=density_factor,
                                    return_closest_gaussian_opacities=True, return_beta=True)
    loss = sum((fields[k] * torch.from_numpy(upstream[k]).to(dtype)).sum() for k in upstream)
    loss.backward()
    return ({k: v.detach().double().numpy() for k, v in fields.items()}, {k: t[k].grad.double().numpy() for k in FO.INPUTS})


def make_case(SuGaR, sha, name, P, N, K, seed, density_factor, scale_spread):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    points = rn(P, 3)
    scaling = torch.exp(-1.0 + scale_spread * rn(P, 3))
    quaternions = rn(P, 4)                                           # not normalised: two_s carries the norm
    strengths = torch.sigmoid(rn(P, 1))
    centre = torch.randint(0, P, (N,), generator=g)
    x = points[centre] + 0.5 * scaling[centre].mean(-1, keepdim=True) * rn(N, 3)
    idx = torch.cdist(x, points).topk(K, dim=1, largest=False).indices
    # round to float32 once: both precisions and the GPU see the same numbers
    inputs = {k: v.float().double().numpy() for k, v in dict(x=x, points=points, scaling=scaling, quaternions=quaternions, strengths=strengths).items()}
    idx = idx.numpy().astype(np.int64)
    upstream = {"density": rn(N), "closest_gaussian_opacities": rn(N, K), "beta": rn(N), "sdf": rn(N)}
    upstream = {k: v.float().double().numpy() for k, v in upstream.items()}
    fx = dict(inputs)
    fx.update({"idx": idx, "density_factor": np.float64(density_factor), "sugar_model_sha256": np.array(sha)})
    fx.update({f"upstream_{k}": v for k, v in upstream.items()})
    for mode in MODES:
        for tag, ups in (("sdf", upstream), ("nosdf", {k: v for k, v in upstream.items() if k != "sdf"})):
            for prec, dtype in (("f64", torch.float64), ("f32", torch.float32)):
                out, grads = reference_run(SuGaR, inputs, idx, ups, mode, dtype, density_factor)
                assert (out["density"] < 1.0).all(), "a density >= 1: the reference's sdf gradient is not finite there"
                assert all(np.isfinite(v).all() for v in list(out.values()) + list(grads.values()))
                keep = (lambda v: v.astype(np.float32)) if prec == "f32" else (lambda v: v)      # exact: they are float32 values
                if tag == "sdf":                           # the outputs do not depend on which of them get a gradient
                    fx.update({f"{mode}_{prec}_out_{k}": keep(v) for k, v in out.items()})
                fx.update({f"{mode}_{tag}_{prec}_grad_{k}": keep(v) for k, v in grads.items()})
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **fx)
    assert os.path.getsize(path) < (1 << 20), (path, os.path.getsize(path))
    print(f"{name}: P {P} N {N} K {K}  density in [{out['density'].min():.3e}, {out['density'].max():.3e}]  {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    S, sha = load_reference()
    make_case(S, sha, "field_k16", P=400, N=300, K=16, seed=20261018, density_factor=1.0 / 16, scale_spread=0.3)
    make_case(S, sha, "field_k5_flat", P=150, N=257, K=5, seed=20261019, density_factor=1.0 / 16, scale_spread=0.9)
