"""``field_values`` / ``compute_density`` -- SuGaR's density and SDF field over the K neighbour Gaussians of every sample.

Replaces ``SuGaR.get_field_values`` (frosting_scene/sugar_model.py:1278-1347, with ``get_beta`` :1203-1276) and
``SuGaR.compute_density`` (:1376-1399), the consumer of the neighbour table ``knn_points`` fills (:1059), which the
coarse trainers call on up to 1 000 000 samples x 16 neighbours every regularised iteration
(frosting_trainers/coarse_density_and_dn_consistency.py:737-752, coarse_density.py:634-642, coarse_sdf.py).  One native
forward and one native backward (csrc/field.hip) instead of the eager gathers, the batched 3x3 products and autograd's
``index_put`` scatters; the backward uses no float atomics and returns the same bits on every run.

Limits: ``return_sdf_grad`` is not offered (no trainer passes it), ``beta_mode='learnable'`` is a scalar expand that stays
in torch (ask for the density here and form the sdf from it), K <= 32, GPU only.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

MAX_K = 32          # FRG_KNN_MAX_K
BETA_MODES = {None: 0, "average": 1, "weighted_average": 2}     # FRG_FIELD_BETA_*
_BACKWARD, _RECOMPUTE = 1, 2                                     # FRG_FIELD_BACKWARD, FRG_FIELD_RECOMPUTE


def _workspace(L, P, N, K, flags, dev):
    ws = torch.empty(int(L.frg_field_workspace_bytes(P, N, K, flags)) + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    return ws, base, ws.numel() - (base - ws.data_ptr())


def _call(fn_name, dev, cfg, tensors, ws_flags):
    """One native call: cfg = (P, N, K, beta code, flags, density_threshold, density_factor, opacity_min_clamp), tensors =
    the pointer fields by name (None = NULL).  Returns the [1] int32 flag an index outside [0, P) raises."""
    L = _lib.lib()
    P, N, K, beta_code, flags, threshold, factor, clamp = cfg
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        ws, base, nbytes = _workspace(L, P, N, K, ws_flags, dev)
        a = _lib.FieldArgs(struct_size=C.sizeof(_lib.FieldArgs), P=P, N=N, K=K,
                           idx_is_int64=int(tensors["idx"].dtype == torch.int64), beta_mode=beta_code, flags=flags,
                           density_threshold=threshold, density_factor=factor, opacity_min_clamp=clamp,
                           bad_index=bad.data_ptr(), workspace=base, workspace_bytes=nbytes, hip_stream=stream.cuda_stream,
                           **{k: (v.data_ptr() if v is not None and v.numel() else None) for k, v in tensors.items()})
        rc = getattr(L, fn_name)(C.byref(a))
        ws.record_stream(stream)
    _lib.check(rc, fn_name)
    return bad


class _Field(torch.autograd.Function):
    """(density, opacities | None, beta | None, sdf | None) of the native forward; the native backward."""

    @staticmethod
    def forward(ctx, x, idx, points, scaling, quaternions, strengths, cfg, want, fallback, validate):
        ins = [t.detach().contiguous().float() for t in (x, points, scaling, quaternions, strengths)]
        xs, pts, sc, qs, st = ins
        N, K = idx.shape
        dev = xs.device
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        want_opac, want_beta, want_sdf = want
        out = {"density": new(N), "opacities": new(N, K) if want_opac else None, "beta": new(N) if want_beta else None,
               "sdf": new(N) if want_sdf else None}
        if N > 0:
            bad = _call("frg_field_forward", dev, cfg,
                        dict(idx=idx, x=xs, points=pts, scaling=sc, quaternions=qs, strengths=st, beta_fallback=fallback, **out), 0)
            if validate and int(bad.item()):
                raise IndexError(f"frosting_amd field_values: closest_gaussians_idx holds an entry outside 0 ... {cfg[0] - 1}")
        ctx.save_for_backward(idx, xs, pts, sc, qs, st, fallback if fallback is not None else xs.new_empty(0))
        ctx.cfg, ctx.dtypes = cfg, [t.dtype for t in (x, points, scaling, quaternions, strengths)]
        ctx.shapes = [t.shape for t in (x, points, scaling, quaternions, strengths)]
        ctx.mark_non_differentiable(idx)
        return out["density"], out["opacities"], out["beta"], out["sdf"]

    @staticmethod
    def backward(ctx, g_density, g_opac, g_beta, g_sdf):
        idx, xs, pts, sc, qs, st, fallback = ctx.saved_tensors
        P, N = ctx.cfg[0], ctx.cfg[1]
        dev = xs.device
        up = [None if g is None else g.contiguous().float() for g in (g_density, g_opac, g_beta, g_sdf)]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)      # every row is stored by the native call
        grads = dict(dL_dx=new(N, 3), dL_dpoints=new(P, 3), dL_dscaling=new(P, 3), dL_dquaternions=new(P, 4), dL_dstrengths=new(P))
        _call("frg_field_backward", dev, ctx.cfg,
              dict(idx=idx, x=xs, points=pts, scaling=sc, quaternions=qs, strengths=st,
                   beta_fallback=fallback if fallback.numel() else None,
                   dL_ddensity=up[0], dL_dopacities=up[1], dL_dbeta=up[2], dL_dsdf=up[3], **grads), _BACKWARD)
        outs = [g.reshape(shape).to(dt) if need else None
                for g, shape, dt, need in zip(grads.values(), ctx.shapes, ctx.dtypes,
                                              (ctx.needs_input_grad[0],) + tuple(ctx.needs_input_grad[2:6]))]
        return outs[0], None, outs[1], outs[2], outs[3], outs[4], None, None, None, None


def _check_inputs(x, idx, points, scaling, quaternions, strengths):
    tensors = (x, idx, points, scaling, quaternions, strengths)
    if any(t.device.type != "cuda" for t in tensors):
        raise RuntimeError("frosting_amd field_values runs on the GPU only (no CPU path)")
    if any(t.device != x.device for t in tensors):
        raise RuntimeError("all tensors of field_values must be on the same GPU")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("x must have dimensions (n_samples, 3)")
    P = int(points.shape[0])
    if points.dim() != 2 or points.shape[1] != 3 or tuple(scaling.shape) != (P, 3) or tuple(quaternions.shape) != (P, 4) or \
            strengths.numel() != P or strengths.shape[0] != P:
        raise ValueError("points (P, 3), scaling (P, 3), quaternions (P, 4) and strengths (P, 1) are expected")
    if idx.dim() != 2 or idx.shape[0] != x.shape[0] or idx.dtype not in (torch.int64, torch.int32):
        raise ValueError("closest_gaussians_idx must be an int64 or int32 tensor of dimensions (n_samples, K)")
    K = int(idx.shape[1])
    if K < 1 or K > MAX_K:
        raise ValueError(f"frosting_amd field_values: K = {K} is outside 1 ... {MAX_K} (the limit of the native kernels)")
    if x.shape[0] > 0 and P == 0:
        raise ValueError("samples without Gaussians")


def field_values(x, closest_gaussians_idx, points, scaling, quaternions, strengths, *, beta_mode="average", return_sdf=True,
                 density_threshold=1., density_factor=1., return_sdf_grad=False, opacity_min_clamp=1e-16,
                 return_closest_gaussian_opacities=False, return_beta=False, validate_idx=True, _recompute=False):
    """``SuGaR.get_field_values(x, closest_gaussians_idx=...)`` on the model's tensors: ``x [N,3]``,
    ``closest_gaussians_idx [N,K]`` (int64 as ``knn_points`` returns it, or int32), ``points [P,3]``, ``scaling [P,3]``,
    ``quaternions [P,4]`` (real part first, used as given), ``strengths [P,1]``.  Returns the reference's dictionary:
    ``density [N]`` (the plain sum, before the normalisation the sdf applies) and, as requested,
    ``closest_gaussian_opacities [N,K]``, ``beta [N]``, ``sdf [N]``; what is not requested is neither allocated nor
    written.  Gradients go to ``x``, ``points``, ``scaling``, ``quaternions`` and ``strengths``.

    On rows whose density is >= 1 the reference's own sdf gradient is not finite (sqrt at exactly 0); here the sdf's
    density term carries no gradient on those rows.  ``validate_idx`` reads one flag back from the device after the
    forward and raises IndexError for an entry outside [0, P) (never dereferenced either way: such a pair contributes
    nothing).  ``beta_mode='learnable'`` and ``return_sdf_grad`` are not offered; K <= 32; GPU only.
    """
    if return_sdf_grad:
        raise NotImplementedError("frosting_amd field_values does not offer return_sdf_grad (no trainer of the reference asks for it)")
    idx = closest_gaussians_idx
    _check_inputs(x, idx, points, scaling, quaternions, strengths)
    need_beta = bool(return_sdf or return_beta)
    if need_beta and beta_mode == "learnable":
        raise NotImplementedError("beta_mode='learnable' is exp(log_beta).expand(n): it stays in torch -- take the density "
                                  "from field_values(..., return_sdf=False) and form the sdf from it")
    if need_beta and beta_mode not in ("average", "weighted_average"):
        raise ValueError("Unknown beta_mode.")
    code = BETA_MODES[beta_mode] if need_beta else 0
    fallback = None
    if code == 2:
        # get_beta's constant where every opacity of a row is 0 (:1271): the largest min-scale among the Gaussians idx names
        # (for a neighbour table over the whole model, the scene's)
        fallback = scaling.detach().float().min(dim=-1)[0][idx.long().clamp(0, max(int(points.shape[0]) - 1, 0))].max().reshape(1) \
            if idx.numel() else scaling.new_zeros(1, dtype=torch.float32)
    cfg = (int(points.shape[0]), int(x.shape[0]), int(idx.shape[1]), code, _RECOMPUTE if _recompute else 0,
           float(density_threshold), float(density_factor), float(opacity_min_clamp))
    want = (bool(return_closest_gaussian_opacities), bool(return_beta), bool(return_sdf))
    density, opac, beta, sdf = _Field.apply(x, idx.contiguous(), points, scaling, quaternions, strengths, cfg, want, fallback,
                                            bool(validate_idx))
    fields = {"density": density}
    if return_closest_gaussian_opacities:
        fields["closest_gaussian_opacities"] = opac
    if return_beta:
        fields["beta"] = beta
    if return_sdf:
        fields["sdf"] = sdf
    return fields


def compute_density(x, closest_gaussians_idx, points, scaling, quaternions, strengths, *, density_factor=1.,
                    return_closest_gaussian_opacities=False):
    """``SuGaR.compute_density`` (:1376-1399): the densities ``[N]``, or ``(densities, neighbour opacities [N,K])``."""
    f = field_values(x, closest_gaussians_idx, points, scaling, quaternions, strengths, beta_mode=None, return_sdf=False,
                     density_factor=density_factor, return_closest_gaussian_opacities=return_closest_gaussian_opacities)
    if return_closest_gaussian_opacities:
        return f["density"], f["closest_gaussian_opacities"]
    return f["density"]
