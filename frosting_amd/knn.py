"""``distCUDA2`` -- mean squared distance to the three nearest neighbours.

Drop-in for ``from simple_knn._C import distCUDA2`` (gaussian_splatting/scene/gaussian_model.py:20,134;
frosting_scene/frosting_model.py:9,530; frosting_scene/sugar_model.py:9): ``distCUDA2(points [P,3] float32
cuda) -> [P] float32``.  ``install_as_simple_knn()`` registers a module of that name so the reference's
import line works unchanged.  GPU only.

``knn_points`` / ``knn_gather`` -- pytorch3d.ops' K nearest neighbours between two point sets, which the reference
calls from frosting_scene/frosting_model.py:300,520,1231,1270,1729,2072,2192, frosting_scene/sugar_model.py:49,249,
1059,1074,1373 and frosting_extractors/coarse_shell.py:40,532.  ``install_as_pytorch3d_ops()`` makes
``from pytorch3d.ops import knn_points`` resolve to it.  GPU only.
"""
from __future__ import annotations

import collections
import ctypes as C
import importlib
import sys
import types

import torch

from . import _lib


def distCUDA2(points: torch.Tensor) -> torch.Tensor:
    if points.device.type != "cuda":
        raise RuntimeError("frosting_amd distCUDA2 runs on the GPU only (no CPU path)")
    if points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("points must have dimensions (num_points, 3)")
    pts = points.contiguous().float()
    P = int(pts.shape[0])
    dev = pts.device
    out = torch.full((P,), 0.0, dtype=torch.float32, device=dev)       # spatial.cu:22
    if P == 0:
        return out
    L = _lib.lib()
    with torch.cuda.device(dev):
        ws = torch.empty(int(L.frg_knn_workspace_bytes(P)) + 256, dtype=torch.uint8, device=dev)
        base = (ws.data_ptr() + 255) // 256 * 256
        stream = torch.cuda.current_stream(dev)
        rc = L.frg_knn_mean_dist2(P, C.c_void_p(pts.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(base),
                                  ws.numel() - (base - ws.data_ptr()), C.c_void_p(stream.cuda_stream))
        ws.record_stream(stream)
    _lib.check(rc, "frg_knn_mean_dist2")
    return out


def install_as_simple_knn():
    """Make ``from simple_knn._C import distCUDA2`` resolve to this implementation."""
    pkg, sub = types.ModuleType("simple_knn"), types.ModuleType("simple_knn._C")
    sub.distCUDA2 = distCUDA2
    pkg._C = sub
    sys.modules["simple_knn"], sys.modules["simple_knn._C"] = pkg, sub
    return sub


MAX_K = 32          # FRG_KNN_MAX_K: the K-best lists live in registers

_KNN = collections.namedtuple("KNN", "dists idx knn")


def _as_lengths(lengths, N, P, name):
    if lengths is None:
        return [P] * N
    if tuple(lengths.shape) != (N,):
        raise ValueError(f"{name} must have shape (N,) = ({N},)")
    out = [int(v) for v in lengths.tolist()]
    if any(v < 0 or v > P for v in out):
        raise ValueError(f"{name} must lie in 0 ... {P}")
    return out


def _knn_native(p1, p2, l1, l2, K):
    """p1 [N,P1,3], p2 [N,P2,3] contiguous float32 on one GPU -> dists [N,P1,K] float32, idx [N,P1,K] int64:
    one native call per batch element on its first l1[n] / l2[n] rows, everything else padding (0, 0)."""
    N, P1 = int(p1.shape[0]), int(p1.shape[1])
    dev = p1.device
    dists = torch.zeros((N, P1, K), dtype=torch.float32, device=dev)
    idx = torch.zeros((N, P1, K), dtype=torch.int64, device=dev)
    if P1 == 0:
        return dists, idx
    L = _lib.lib()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev)
        for n in range(N):
            n1, n2 = l1[n], l2[n]
            if n1 == 0 or n2 == 0:
                continue
            a, b = p1[n], p2[n]                                   # the first n1 / n2 rows of a contiguous [P,3] block
            self_query = a.data_ptr() == b.data_ptr() and n1 == n2
            ws = torch.empty(int(L.frg_knn_points_workspace_bytes(0 if self_query else n1, n2, K)) + 256,
                             dtype=torch.uint8, device=dev)
            base = (ws.data_ptr() + 255) // 256 * 256
            # rows of one batch element are K apart, so its first n1 rows are one contiguous [n1,K] block
            rc = L.frg_knn_points(n1, C.c_void_p(a.data_ptr()), n2, C.c_void_p(b.data_ptr()), K,
                                  C.c_void_p(dists[n].data_ptr()), C.c_void_p(idx[n].data_ptr()), C.c_void_p(base),
                                  ws.numel() - (base - ws.data_ptr()), C.c_void_p(stream.cuda_stream))
            ws.record_stream(stream)
            _lib.check(rc, "frg_knn_points")
    return dists, idx


def _valid_slots(l1, l2, P1, K, dev):
    """[N,P1,K] bool: the slots that hold a neighbour (row below lengths1, slot below min(K, lengths2))."""
    rows = torch.arange(P1, device=dev)[None, :, None] < torch.tensor(l1, device=dev)[:, None, None]
    slots = torch.arange(K, device=dev)[None, None, :] < torch.tensor(l2, device=dev)[:, None, None]
    return rows & slots


class _KnnPoints(torch.autograd.Function):
    """dists and idx of the native search; the backward of dists, 2 (p1 - p2[idx]) g, in torch ops."""

    @staticmethod
    def forward(ctx, p1, p2, l1, l2, K, same):
        a = p1.detach().contiguous().float()
        b = a if same else p2.detach().contiguous().float()
        dists, idx = _knn_native(a, b, l1, l2, K)
        ctx.save_for_backward(a, b, idx)
        ctx.l1, ctx.l2, ctx.dtypes = l1, l2, (p1.dtype, p2.dtype)
        ctx.mark_non_differentiable(idx)
        return dists, idx

    @staticmethod
    def backward(ctx, g_dists, _g_idx):
        a, b, idx = ctx.saved_tensors
        N, P1, K = idx.shape
        P2 = int(b.shape[1])
        g1, g2 = torch.zeros_like(a), torch.zeros_like(b)
        if P1 > 0 and P2 > 0:
            valid = _valid_slots(ctx.l1, ctx.l2, P1, K, a.device)
            g = torch.where(valid, g_dists.float(), torch.zeros((), device=a.device))
            w = 2.0 * (a[:, :, None, :] - knn_gather(b, idx)) * g[..., None]          # [N,P1,K,3]
            g1 = w.sum(dim=2)
            flat = (idx + torch.arange(N, device=a.device)[:, None, None] * P2).reshape(-1)
            g2.view(N * P2, 3).index_add_(0, flat, -w.reshape(-1, 3))               # padded slots add 0 to row 0
        return g1.to(ctx.dtypes[0]), g2.to(ctx.dtypes[1]), None, None, None, None


def knn_points(p1, p2, lengths1=None, lengths2=None, norm: int = 2, K: int = 1, version: int = -1,
               return_nn: bool = False, return_sorted: bool = True):
    """pytorch3d.ops.knn_points: for every point of ``p1 [N,P1,3]`` the ``K`` nearest points of ``p2 [N,P2,3]``.

    Returns the namedtuple ``(dists [N,P1,K] float32, idx [N,P1,K] int64, knn [N,P1,K,3] or None)``.

    Parity unpinned, value fully specified (pytorch3d is absent on this platform and leaves ties open):
    ``dists`` is the squared distance ``(dx*dx + dy*dy) + dz*dz`` with ``d = p1 - p2`` in float32 without
    contraction, and the K neighbours are ordered ascending by (distance, index in p2), so equal distances
    resolve to the smaller index.  Nothing is excluded: a self-query (``p1 is p2``) finds every point itself at
    distance 0 first.  Where ``K > lengths2[n]`` the trailing slots hold ``dists = 0, idx = 0``; rows at or
    beyond ``lengths1[n]`` are all padding.  ``dists`` carries a gradient to ``p1`` and ``p2``, ``idx`` none.
    ``norm`` must be 2, ``version`` is ignored, ``return_sorted=False`` returns the sorted result too, and K is
    limited to 1 ... 32.  One native call per batch element; GPU only.
    """
    if norm != 2:
        raise ValueError("frosting_amd knn_points supports norm=2 only")
    if not isinstance(K, int) or K < 1 or K > MAX_K:
        raise ValueError(f"frosting_amd knn_points: K = {K} is outside 1 ... {MAX_K} (the limit of the native search)")
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[2] != 3 or p2.shape[2] != 3:
        raise ValueError("p1 and p2 must have dimensions (N, P1, 3) and (N, P2, 3)")
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("p1 and p2 must have the same batch dimension")
    if p1.device.type != "cuda" or p2.device.type != "cuda":
        raise RuntimeError("frosting_amd knn_points runs on the GPU only (no CPU path)")
    if p1.device != p2.device:
        raise RuntimeError("p1 and p2 must be on the same GPU")
    N = int(p1.shape[0])
    l1 = _as_lengths(lengths1, N, int(p1.shape[1]), "lengths1")
    l2 = _as_lengths(lengths2, N, int(p2.shape[1]), "lengths2")
    dists, idx = _KnnPoints.apply(p1, p2, l1, l2, K, p1 is p2)
    nn = knn_gather(p2, idx, lengths2) if return_nn else None
    return _KNN(dists=dists, idx=idx, knn=nn)


def knn_gather(x, idx, lengths=None):
    """pytorch3d.ops.knn_gather: ``x [N,P2,C]``, ``idx [N,P1,K]`` -> ``[N,P1,K,C]`` with ``out[n,i,k] =
    x[n, idx[n,i,k]]``; with ``lengths [N]`` the slots ``k >= lengths[n]`` (knn_points' padding) give zeros."""
    if x.dim() != 3 or idx.dim() != 3 or x.shape[0] != idx.shape[0]:
        raise ValueError("x must be (N, P2, C) and idx (N, P1, K) with the same N")
    N, P2, Cc = x.shape
    _, P1, K = idx.shape
    if P2 == 0:
        return x.new_zeros((N, P1, K, Cc))
    out = x[:, :, None, :].expand(N, P2, K, Cc).gather(1, idx[..., None].expand(N, P1, K, Cc))
    if lengths is not None:
        if tuple(lengths.shape) != (N,):
            raise ValueError(f"lengths must have shape (N,) = ({N},)")
        pad = torch.arange(K, device=x.device)[None, :] >= lengths.to(x.device)[:, None]          # [N,K]
        out = out.masked_fill(pad[:, None, :, None], 0.0)
    return out


def install_as_pytorch3d_ops():
    """Make ``from pytorch3d.ops import knn_points, knn_gather`` resolve to this implementation.

    Where a real ``pytorch3d.ops`` imports, only these two names are set on it.  Otherwise minimal ``pytorch3d``
    and ``pytorch3d.ops`` modules carrying nothing but these two names are registered: NOTHING else of pytorch3d
    (transforms, structures, ico_sphere, the mesh losses, ...) is provided here.
    """
    try:
        ops = importlib.import_module("pytorch3d.ops")
    except ImportError:
        pkg = sys.modules.get("pytorch3d") or types.ModuleType("pytorch3d")
        ops = types.ModuleType("pytorch3d.ops")
        pkg.ops = ops
        sys.modules["pytorch3d"], sys.modules["pytorch3d.ops"] = pkg, ops
    ops.knn_points, ops.knn_gather = knn_points, knn_gather
    return ops
