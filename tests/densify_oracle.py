"""Torch restatement of vanilla 3DGS densification, written from its description (not from the reference's text):
classification, output order, the split children, the opacity reset, and the float64 yardsticks of the GPU tests.
It runs on any device, so the GPU tier can check sizes for which no fixture can be committed; the CPU tier checks that it
reproduces every fixture the reference itself produced (tools/make_golden_densify.py).

Rows of the result: [surviving originals | clones | first children of the split rows | second children], each in
source order, each minus its pruned rows."""
from __future__ import annotations

import numpy as np
import torch

NAMES = ("means3D", "scales", "rotations", "opacities", "shs")
BAND_ULPS = 8


def thresholds32(max_grad, min_opacity, extent, percent_dense):
    """The four thresholds as the float32 values a float32 tensor is compared with (products formed in double first)."""
    f = lambda x: float(np.float32(x))
    return dict(max_grad=f(max_grad), min_opacity=f(min_opacity), dense=f(percent_dense * extent), world=f(0.1 * extent))


def classify(raw_scales, raw_opacities, accum, denom, max_grad, min_opacity, extent, percent_dense, max_screen_size):
    """Boolean masks over the source rows: 'kept' (survives as itself), 'cloned' (has a surviving clone), 'split' (has two
    surviving children), plus the intermediate predicates."""
    grad = accum.reshape(-1) / denom.reshape(-1)
    grad = torch.where(torch.isnan(grad), torch.zeros_like(grad), grad)
    s = torch.exp(raw_scales)
    smax = s.max(dim=1).values
    selected = grad >= max_grad
    big = smax > percent_dense * extent
    clone, split = selected & ~big, selected & big
    faint = torch.sigmoid(raw_opacities).reshape(-1) < min_opacity
    prune_self, prune_child = faint, faint
    if max_screen_size:
        # the screen-size term reads statistics that were zeroed a moment before: false on every row.  What is left is the
        # world-size term on the row's NEW scale (a child's: the parent's / 1.6, through log and exp)
        prune_self = faint | (smax > 0.1 * extent)
        child_max = torch.exp(torch.log(s / (0.8 * 2))).max(dim=1).values
        prune_child = faint | (child_max > 0.1 * extent)
    return dict(kept=~split & ~prune_self, cloned=clone & ~prune_self, split=split & ~prune_child,
                selected=selected, big=big, faint=faint)


def rotation_matrices(q):
    n = torch.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
    q = q / n[:, None]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.zeros((q.shape[0], 3, 3), dtype=q.dtype, device=q.device)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def children(means3D, raw_scales, rotations, z):
    """(xyz', raw_scale') of one child per row; z [n,3] standard-normal samples.  dtype follows the inputs (float32: the
    reference's evaluation; float64 inputs: the yardstick)."""
    s = torch.exp(raw_scales)
    samples = torch.zeros_like(s) + s * z
    xyz = torch.bmm(rotation_matrices(rotations), samples.unsqueeze(-1)).squeeze(-1) + means3D
    return xyz, torch.log(s / (0.8 * 2))


def densify(params, m, v, accum, denom, max_grad, min_opacity, extent, percent_dense, max_screen_size, noise):
    """-> (params', m', v', sizes, masks).  params / m / v: {name: [P, ...]}; noise [P,2,3] indexed by source row, child."""
    k = classify(params["scales"], params["opacities"], accum, denom, max_grad, min_opacity, extent, percent_dense, max_screen_size)
    A, B, C = k["kept"], k["cloned"], k["split"]
    c_xyz, c_scale = [], None
    for child in (0, 1):
        xyz, c_scale = children(params["means3D"][C], params["scales"][C], params["rotations"][C], noise[C][:, child])
        c_xyz.append(xyz)
    out_p, out_m, out_v = {}, {}, {}
    for name in params:
        p = params[name]
        first = c_xyz[0] if name == "means3D" else c_scale if name == "scales" else p[C]
        second = c_xyz[1] if name == "means3D" else c_scale if name == "scales" else p[C]
        out_p[name] = torch.cat((p[A], p[B], first, second), dim=0)
        fresh = torch.zeros((int(B.sum()) + 2 * int(C.sum()),) + tuple(p.shape[1:]), dtype=p.dtype, device=p.device)
        out_m[name] = torch.cat((m[name][A], fresh), dim=0)
        out_v[name] = torch.cat((v[name][A], fresh), dim=0)
    sizes = [int(A.sum()), int(B.sum()), int(C.sum()), int(C.sum())]
    return out_p, out_m, out_v, sizes + [sum(sizes)], k


def reset_opacity(raw_opacities):
    x = torch.minimum(torch.sigmoid(raw_opacities), torch.ones_like(raw_opacities) * 0.01)
    return torch.log(x / (1 - x))


# ---- float64 rules ---------------------------------------------------------------------------------------------------------
def band_rows(raw_scales, raw_opacities, accum, denom, max_grad, min_opacity, extent, percent_dense, ulps=BAND_ULPS):
    """Rows on which a decision may hinge on the last places of exp / sigmoid / the division: evaluated in float64 on the
    float32 inputs, a quantity within `ulps` float32 ulps of a threshold it is compared with.  max(exp(scale)) against
    percent_dense * extent, 0.1 * extent and 1.6 x either; sigmoid(opacity) against min_opacity; grad against max_grad."""
    t = thresholds32(max_grad, min_opacity, extent, percent_dense)
    near = lambda x, thr: (x - thr).abs() <= ulps * float(np.spacing(np.float32(thr)))
    smax = torch.exp(raw_scales.double()).max(dim=1).values
    grad = accum.reshape(-1).double() / denom.reshape(-1).double()
    grad = torch.where(torch.isnan(grad), torch.zeros_like(grad), grad)
    band = near(grad, t["max_grad"]) | near(torch.sigmoid(raw_opacities.double()).reshape(-1), t["min_opacity"])
    for thr in (t["dense"], t["world"], 1.6 * t["dense"], 1.6 * t["world"]):
        band |= near(smax, thr)
    return band


def children_error(xyz32, scale32, means3D, raw_scales, rotations, z):
    """Distance of a float32 evaluation of the children from the float64 one on the same float32 inputs:
    (max over rows and coordinates of |xyz - xyz64| / (|xyz64| + ||s * z||_1),  max of |raw_scale - raw_scale64|)."""
    d = lambda t: t.double()
    xyz64, scale64 = children(d(means3D), d(raw_scales), d(rotations), d(z))
    if xyz64.numel() == 0:
        return 0.0, 0.0
    size = xyz64.abs() + (torch.exp(d(raw_scales)) * d(z)).abs().sum(dim=1, keepdim=True)
    return float(((d(xyz32) - xyz64).abs() / size).max()), float((d(scale32) - scale64).abs().max())


def reset_opacity_error(raw32, raw_in):
    """max |raw32 - float64 logit(min(sigmoid(raw_in), float32(0.01)))|"""
    x = torch.minimum(torch.sigmoid(raw_in.double()), torch.full_like(raw_in, 0.01).double())
    return float((raw32.double() - torch.log(x / (1 - x))).abs().max())


# ---- fixtures --------------------------------------------------------------------------------------------------------------
def fixture_tensors(fx, device="cpu"):
    """(params, m, v) dicts of a fixture's inputs and of its outputs, as torch tensors."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    names = [n for n in NAMES if f"in_{n}" in fx]
    ins = tuple({n: t(fx[f"in{tag}_{n}"]) for n in names} for tag in ("", "_m", "_v"))
    outs = tuple({n: t(fx[f"out{tag}_{n}"]) for n in names} for tag in ("", "_m", "_v"))
    return ins, outs


def fixture_thresholds(fx):
    mss = float(fx["max_screen_size"])
    return dict(max_grad=float(fx["max_grad"]), min_opacity=float(fx["min_opacity"]), extent=float(fx["extent"]),
                percent_dense=float(fx["percent_dense"]), max_screen_size=mss if mss > 0 else None)
