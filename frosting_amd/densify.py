"""Adaptive density control of vanilla 3DGS on the device (csrc/densify.hip).

The three calls a vanilla trainer makes between the backward and the optimizer
(gaussian_splatting/train.py:114-124; gaussian_splatting/scene/gaussian_model.py:210-213, 273-407):

    gaussians.add_densification_stats(viewspace_point_tensor, visibility_filter)   ->  DensityControl.add_stats
    gaussians.densify_and_prune(max_grad, min_opacity, extent, size_threshold)     ->  DensityControl.densify_and_prune
    gaussians.reset_opacity()                                                      ->  DensityControl.reset_opacity

on the flat parameter layout of ``FlatAdam`` with RAW scales (log) and RAW opacities (logit) -- the parameterisation
``fused.rasterize_raw`` renders and the reference's ``GaussianModel`` densifies.  One launch forms the statistics; a
densification is a classify-and-scan pass over 20 bytes per Gaussian, ONE host synchronisation (the new row count) and
one launch that writes parameters and both Adam moments of the new model -- where ``FlatAdam.append`` / ``prune`` rebuild
all three buffers four times.  The resulting rows are the reference's, in its order
``[surviving originals | clones | first children of the split rows | second children]``.  GPU only: there is no CPU path.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .optim import FlatAdam, ShardedFlatAdam
from .parallel import PARAM_ORDER, flat_layout

SECTIONS = ("kept", "cloned", "split_first", "split_second")


class _CtypesOps:
    """The five device operations over ctypes; diff_gaussian_rasterization._C exports the same five with the same
    arguments (csrc/torch_ext/torch_binding.cpp)."""

    @staticmethod
    def densify_accumulate(radii, dL_dmean2D, row_live, xyz_gradient_accum, denom, max_radii2D):
        dev = radii.device
        with torch.cuda.device(dev):
            rc = _lib.lib().frg_densify_accumulate(radii.numel(), _lib.ptr(radii), _lib.ptr(dL_dmean2D), _lib.ptr(row_live),
                                                   _lib.ptr(xyz_gradient_accum), _lib.ptr(denom), _lib.ptr(max_radii2D),
                                                   _lib.stream_ptr(dev))
        _lib.check(rc, "frg_densify_accumulate")

    @staticmethod
    def densify_accumulate_views(packets, first, count, capacity_rows, means3D, scales, rotations, opacities, raw_params,
                                 xyz_gradient_accum, denom, max_radii2D, status, status_seq):
        """frg_densify_accumulate_views: packets [n_views, words] int32 as gathered (with visibility sections), Gaussians
        [first, first + count); scales / rotations / opacities in their raw forms when raw_params; status: one int64 word
        (pinned host or device memory) or an empty tensor."""
        dev = packets.device
        v = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()
        raw = bool(raw_params)
        a = _lib.DensifyViewsArgs(struct_size=C.sizeof(_lib.DensifyViewsArgs), P=max_radii2D.numel(), first=int(first), count=int(count),
                                  n_views=packets.shape[0], packets=v(packets), packet_stride_bytes=packets.shape[1] * 4,
                                  capacity_rows=int(capacity_rows), means3D=v(means3D), scales=None if raw else v(scales),
                                  rotations=None if raw else v(rotations), opacities=None if raw else v(opacities),
                                  raw_opacities=v(opacities) if raw else None, raw_scales=v(scales) if raw else None,
                                  raw_rotations=v(rotations) if raw else None, xyz_gradient_accum=v(xyz_gradient_accum), denom=v(denom),
                                  max_radii2D=v(max_radii2D), status=v(status), status_seq=int(status_seq),
                                  hip_stream=torch.cuda.current_stream(dev).cuda_stream)
        with torch.cuda.device(dev):
            rc = _lib.lib().frg_densify_accumulate_views(C.byref(a))
        _lib.check(rc, "frg_densify_accumulate_views")

    @staticmethod
    def densify_plan(raw_scales, raw_opacities, xyz_gradient_accum, denom, max_grad, min_opacity, extent, percent_dense,
                     prune_big_points):
        L = _lib.lib()
        dev, P = raw_scales.device, raw_opacities.numel()
        with torch.cuda.device(dev):
            plan = torch.empty((4, P), dtype=torch.int32, device=dev)
            record = torch.empty(8, dtype=torch.int32, device=dev)
            ws = int(L.frg_densify_workspace_bytes(P))
            work = torch.empty(max(ws, 1), dtype=torch.uint8, device=dev)
            prm = _lib.DensifyParams(struct_size=C.sizeof(_lib.DensifyParams), max_grad=float(max_grad), min_opacity=float(min_opacity),
                                     extent=float(extent), percent_dense=float(percent_dense), prune_big_points=int(bool(prune_big_points)))
            rc = L.frg_densify_plan(P, _lib.ptr(raw_scales), _lib.ptr(raw_opacities), _lib.ptr(xyz_gradient_accum), _lib.ptr(denom),
                                    C.byref(prm), _lib.ptr(plan), _lib.ptr(record), _lib.ptr(work), ws, _lib.stream_ptr(dev))
        _lib.check(rc, "frg_densify_plan")
        return plan, record

    @staticmethod
    def densify_apply(plan, P_out, group_width, src_offsets, dst_offsets, out_numel, noise, params, exp_avg, exp_avg_sq):
        dev, n = params.device, len(group_width)
        with torch.cuda.device(dev):
            out = torch.empty(out_numel, dtype=torch.float32, device=dev)
            out_m, out_v = torch.empty_like(out), torch.empty_like(out)
            rc = _lib.lib().frg_densify_apply(plan.shape[1], int(P_out), _lib.ptr(plan), n, (C.c_int * n)(*group_width),
                                              (C.c_longlong * n)(*src_offsets), (C.c_longlong * n)(*dst_offsets), int(out_numel),
                                              _lib.ptr(noise), _lib.ptr(params), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq),
                                              _lib.ptr(out), _lib.ptr(out_m), _lib.ptr(out_v), _lib.stream_ptr(dev))
        _lib.check(rc, "frg_densify_apply")
        return out, out_m, out_v

    @staticmethod
    def reset_opacity(raw_opacities, exp_avg, exp_avg_sq):
        dev = raw_opacities.device
        with torch.cuda.device(dev):
            rc = _lib.lib().frg_reset_opacity(raw_opacities.numel(), _lib.ptr(raw_opacities), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq),
                                              _lib.stream_ptr(dev))
        _lib.check(rc, "frg_reset_opacity")


def native_ops(binding: str = "ctypes"):
    """'ctypes': the C ABI through ctypes; 'ext': the compiled torch extension diff_gaussian_rasterization._C."""
    if binding == "ext":
        import diff_gaussian_rasterization
        return diff_gaussian_rasterization._C
    if binding != "ctypes":
        raise ValueError(f"unknown binding '{binding}'")
    return _CtypesOps


class DensityControl:
    """``DensityControl(optimizer, percent_dense=0.01)`` keeps the densification statistics of the model that `optimizer`
    (a ``FlatAdam`` whose groups begin with means3D [P,3], scales [P,3] (log), rotations [P,4], opacities [P] or [P,1]
    (logit)) holds: ``xyz_gradient_accum`` [P,1], ``denom`` [P,1], ``max_radii2D`` [P], float32 as the reference keeps them.

    ``ShardedFlatAdam`` is refused: its moments exist per shard only, and moving rows re-shards them -- not implemented.
    Statistics over a view-parallel batch: hand this object to ``ViewParallelRasterizer(..., slotsum=True, densify=control)``
    -- the slot-sum exchange then adds every view of a step from the gathered packets (``frg_densify_accumulate_views``: what
    ``add_stats`` adds view by view, bit for bit, identical on every rank, no further collective); after
    ``densify_and_prune`` call ``ViewParallelRasterizer.adopt_scene`` with the resized model."""

    def __init__(self, optimizer: FlatAdam, percent_dense: float = 0.01, binding: str = "ctypes"):
        if isinstance(optimizer, ShardedFlatAdam):
            raise TypeError("DensityControl: ShardedFlatAdam keeps the moments of its own shard only; densification under a "
                            "sharded optimizer is not implemented -- use FlatAdam")
        if not isinstance(optimizer, FlatAdam):
            raise TypeError("DensityControl needs a FlatAdam")
        if tuple(optimizer.names[:4]) != PARAM_ORDER[:4]:
            raise ValueError(f"the optimizer's groups must begin with {PARAM_ORDER[:4]}, got {tuple(optimizer.names)}")
        if optimizer.flat.device.type != "cuda":
            raise RuntimeError("DensityControl runs on the GPU only (no CPU path)")
        self.optimizer = optimizer
        self.percent_dense = float(percent_dense)
        self.ops = native_ops(binding)
        self._zero_stats(self._rows())

    def _rows(self) -> int:
        opt = self.optimizer
        P = opt._per_gaussian()
        widths = [int(torch.Size(opt.shapes[k][1:]).numel()) for k in opt.names]
        if widths[:4] != [3, 3, 4, 1]:
            raise ValueError(f"means3D [P,3], scales [P,3], rotations [P,4], opacities [P] expected, got {opt.shapes}")
        return P

    def _zero_stats(self, P: int):
        dev = self.optimizer.flat.device
        self.xyz_gradient_accum = torch.zeros((P, 1), dtype=torch.float32, device=dev)
        self.denom = torch.zeros((P, 1), dtype=torch.float32, device=dev)
        self.max_radii2D = torch.zeros(P, dtype=torch.float32, device=dev)

    def add_stats(self, radii: torch.Tensor, viewspace_grad: torch.Tensor, row_live: torch.Tensor = None):
        """train.py:116-117 in one launch.  radii [P] int32 of the view just rendered, viewspace_grad [P,3] its dL_dmeans2D.
        row_live (uint8 [P], as a live_rows backward leaves it): the gradient rows of unmarked Gaussians were never written;
        they count as zero and are not read."""
        P = self.max_radii2D.numel()
        dev = self.max_radii2D.device
        if radii.dtype != torch.int32 or radii.numel() != P or radii.device != dev or not radii.is_contiguous():
            raise RuntimeError(f"radii: expected a contiguous int32 tensor of {P} entries on {dev}")
        g = viewspace_grad
        if g.dtype != torch.float32 or tuple(g.shape) != (P, 3) or g.device != dev or not g.is_contiguous():
            raise RuntimeError(f"viewspace_grad: expected a contiguous float32 [{P}, 3] tensor on {dev}")
        if row_live is not None and (row_live.dtype != torch.uint8 or row_live.numel() != P or row_live.device != dev
                                     or not row_live.is_contiguous()):
            raise RuntimeError(f"row_live: expected a contiguous uint8 tensor of {P} entries on {dev}")
        self.ops.densify_accumulate(radii, g.detach(), row_live if row_live is not None else torch.empty(0, dtype=torch.uint8, device=dev),
                                    self.xyz_gradient_accum, self.denom, self.max_radii2D)

    def densify_and_prune(self, max_grad: float, min_opacity: float, extent: float, max_screen_size, generator=None,
                          noise: torch.Tensor = None):
        """gaussian_model.py:389-403 on the optimizer's buffers.  max_screen_size: None / 0 (train.py:120 before the first
        opacity reset) or a radius; as in the reference it only switches the world-size prune (0.1 * extent) on -- the
        screen-size test itself reads statistics that the reference has just zeroed and never fires.
        noise [P,2,3]: the standard-normal samples of the split children, indexed by SOURCE row and child (recorded samples
        in tests); drawn with torch.randn(generator=generator) when absent.
        The optimizer's buffers, layout and views are replaced (its `steps` and learning rates kept), the statistics are
        zeros of the new length.  Returns (params, sizes): the new params dict and {'kept', 'cloned', 'split_first',
        'split_second', 'total'}.  One host synchronisation.  `last_plan` keeps the plan ([4,P] int32: per source row its
        destination row in each section, or -1) until the next call."""
        opt = self.optimizer
        P = self._rows()
        if P != self.max_radii2D.numel():
            raise RuntimeError(f"the optimizer holds {P} Gaussians, the statistics {self.max_radii2D.numel()}: the model was "
                               "resized behind DensityControl's back")
        dev = opt.flat.device
        if noise is None:
            noise = torch.randn((P, 2, 3), dtype=torch.float32, device=dev, generator=generator)
        if noise.dtype != torch.float32 or tuple(noise.shape) != (P, 2, 3) or noise.device != dev or not noise.is_contiguous():
            raise RuntimeError(f"noise: expected a contiguous float32 [{P}, 2, 3] tensor on {dev}")
        plan, record = self.ops.densify_plan(opt.params["scales"], opt.params["opacities"], self.xyz_gradient_accum, self.denom,
                                             float(max_grad), float(min_opacity), float(extent), self.percent_dense,
                                             bool(max_screen_size))
        sizes = [int(x) for x in record.cpu()]          # the one synchronisation: the new buffers are sized by it
        P_out = sizes[4]
        assert sizes[5] == P and sum(sizes[:4]) == P_out, sizes
        shapes = {k: (P_out,) + tuple(opt.shapes[k][1:]) for k in opt.names}
        _, layout, numel = flat_layout(shapes, opt.names)
        widths = [int(torch.Size(opt.shapes[k][1:]).numel()) for k in opt.names]
        out, out_m, out_v = self.ops.densify_apply(plan, P_out, widths, [opt.layout[k][0] for k in opt.names],
                                                   [layout[k][0] for k in opt.names], numel, noise, opt.flat, opt.exp_avg,
                                                   opt.exp_avg_sq)
        params = opt.adopt(P_out, out, out_m, out_v)
        self._zero_stats(P_out)
        self.last_plan = plan
        return params, dict(zip(SECTIONS + ("total",), sizes[:5]))

    def reset_opacity(self):
        """gaussian_model.py:210-213: raw opacity <- logit(min(sigmoid(raw), 0.01)), both moments of the group zeroed."""
        opt = self.optimizer
        self.ops.reset_opacity(opt.params["opacities"], opt.m["opacities"], opt.v["opacities"])
        return opt.params
