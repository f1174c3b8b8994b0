"""The density / SDF field over K neighbour Gaussians, restated in torch ops of any dtype (float64: the yardstick of the
GPU tests; float32 on the CPU: the error a float32 evaluation of these formulas has).  tests/test_field_cpu.py pins this
restatement to the arrays the reference's own function produced (tests/golden/field_*.npz)."""
import math

import numpy as np
import torch

UPSTREAM = ("density", "closest_gaussian_opacities", "beta", "sdf")
INPUTS = ("x", "points", "scaling", "quaternions", "strengths")
EPS32 = float(np.finfo(np.float32).eps)


def rotation(q):
    """pytorch3d.transforms.quaternion_to_matrix: real part first, two_s = 2 / sum(q * q), the quaternion as given."""
    r, i, j, k = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    rows = (1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
            two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
            two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j))
    return torch.stack(rows, -1).reshape(q.shape[:-1] + (3, 3))


def inv_scaled_rotation(scaling, quaternions):
    """A_j = R(q_j) diag(1 / max(s_j, 1e-8))"""
    return rotation(quaternions) * (1.0 / scaling.clamp(min=1e-8))[:, None]


def field(x, idx, points, scaling, quaternions, strengths, beta_mode="average", return_sdf=True, density_threshold=1.,
          density_factor=1., opacity_min_clamp=1e-16, return_closest_gaussian_opacities=False, return_beta=False):
    """The `fields` dictionary, differentiable w.r.t. the five float inputs."""
    idx = idx.long()
    A = inv_scaled_rotation(scaling, quaternions)[idx]                          # [N,K,3,3]
    d = x[:, None] - points[idx]                                                # [N,K,3]
    w = (A.transpose(-1, -2) @ d[..., None])[..., 0]
    o = density_factor * strengths[idx][..., 0] * torch.exp(-0.5 * (w * w).sum(-1).clamp(min=0., max=1e8))
    density = o.sum(-1)
    out = {"density": density.clone()}
    if return_closest_gaussian_opacities:
        out["closest_gaussian_opacities"] = o
    if not (return_sdf or return_beta):
        return out
    big = density >= 1.
    normalised = torch.where(big, density / (density.detach() + 1e-12), density)
    smin = scaling.min(dim=-1)[0][idx]                                          # [N,K]
    if beta_mode == "average":
        beta = smin.mean(dim=1)
    elif beta_mode == "weighted_average":
        total = o.sum(-1, keepdim=True)
        beta = (smin * (o / total.clamp(min=opacity_min_clamp))).sum(-1)
        # a constant where every opacity of the row is 0; the VALUE only -- the gradient is that of the sum above
        beta = beta + torch.where(total[:, 0] == 0., smin.max().detach() - beta.detach(), torch.zeros_like(beta.detach()))
    else:
        raise ValueError("Unknown beta_mode.")
    if return_beta:
        out["beta"] = beta
    if return_sdf:
        offset = math.sqrt(-2. * math.log(min(density_threshold, 1.)))
        out["sdf"] = beta * (torch.sqrt(-2. * torch.log(normalised.clamp(min=opacity_min_clamp))) - offset)
    return out


def run(inputs, idx, upstream, dtype, **kw):
    """inputs: {name: array} of INPUTS; upstream: {output name: array} -- the outputs asked for are those with an upstream
    gradient ('density' always).  -> ({output: float64 array}, {input: float64 array of dL/dinput}), evaluated in `dtype`."""
    t = {k: torch.from_numpy(np.asarray(inputs[k])).to(dtype).requires_grad_(True) for k in INPUTS}
    out = field(t["x"], torch.from_numpy(np.asarray(idx)), t["points"], t["scaling"], t["quaternions"], t["strengths"],
                return_sdf="sdf" in upstream, return_beta="beta" in upstream,
                return_closest_gaussian_opacities="closest_gaussian_opacities" in upstream, **kw)
    loss = sum((out[k] * torch.from_numpy(np.asarray(upstream[k])).to(dtype)).sum() for k in upstream)
    loss.backward()
    return ({k: v.detach().double().numpy() for k, v in out.items()},
            {k: t[k].grad.double().numpy() for k in INPUTS})


def l2_distance(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b))


def judge(name, ours, f64, f32):
    """The rule of the GPU tests: |ours - f64| <= 2 |f32 - f64| + eps32 |f64| (L2 norms over the tensor), f32 being a float32
    CPU evaluation of the same function.  Returns the three figures for the message."""
    ours, f64, f32 = (np.asarray(v, np.float64) for v in (ours, f64, f32))
    assert ours.shape == f64.shape, (name, ours.shape, f64.shape)
    assert np.isfinite(ours).all(), f"{name}: not finite"
    mine, theirs, floor = l2_distance(ours, f64), l2_distance(f32, f64), EPS32 * float(np.linalg.norm(f64.ravel()))
    print(f"{name}: |ours - f64| {mine:.3e}  |f32 - f64| {theirs:.3e}  eps |f64| {floor:.3e}")
    assert mine <= 2.0 * theirs + floor, f"{name}: |ours - f64| = {mine:.3e} > 2 * {theirs:.3e} + {floor:.3e}"
    return mine, theirs, floor
