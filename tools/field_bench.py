"""Forward + backward of field_values beside the eager torch chain, on the GPU, at the size the dn_consistency trainer uses.

  field_bench.py [--n 1000000] [--p 1000000] [--k 16] [--mode average|weighted_average] [--reps 10]

The neighbour table comes from our knn_points (a self-query of the Gaussians, K = 16), the samples are drawn around
randomly chosen Gaussians and take those Gaussians' rows of the table, as SuGaR does.  Timed: the fused op with the packed
records, the fused op rebuilding A per pair (FRG_FIELD_RECOMPUTE), the forward alone of both, and the eager chain written
here from the formulas (three gathers, the batched 3x3 product, exp, sums, log, sqrt; autograd's replay).  Every variant is
warmed up, then timed over `reps` calls ending in a device synchronise, the variants alternating, three rounds; the line
reports the median round of each.  Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from frosting_amd.field import field_values  # noqa: E402
from frosting_amd.knn import knn_points  # noqa: E402


def rotation(q):
    r, i, j, k = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    rows = (1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
            two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
            two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j))
    return torch.stack(rows, -1).reshape(q.shape[:-1] + (3, 3))


def eager(x, idx, points, scaling, quaternions, strengths, beta_mode, density_factor, clamp=1e-16):
    A = (rotation(quaternions) * (1.0 / scaling.clamp(min=1e-8))[:, None])[idx]
    w = (A.transpose(-1, -2) @ (x[:, None] - points[idx])[..., None])[..., 0]
    o = density_factor * strengths[idx][..., 0] * torch.exp(-0.5 * (w * w).sum(-1).clamp(min=0., max=1e8))
    density = o.sum(-1)
    dn = torch.where(density >= 1., density / (density.detach() + 1e-12), density)
    smin = scaling.min(dim=-1)[0][idx]
    if beta_mode == "average":
        beta = smin.mean(dim=1)
    else:
        total = o.sum(-1, keepdim=True)
        beta = (smin * (o / total.clamp(min=clamp))).sum(-1)
        beta = beta + torch.where(total[:, 0] == 0., smin.max().detach() - beta.detach(), torch.zeros_like(beta.detach()))
    return {"density": density, "sdf": beta * torch.sqrt(-2. * torch.log(dn.clamp(min=clamp)))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--p", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--mode", default="average")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("field_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(20261018)
    P, N, K = a.p, a.n, a.k
    points = torch.randn(P, 3, generator=g).to(dev)
    spacing = (1.0 / P) ** (1.0 / 3.0)                             # unit-variance cloud: neighbours about this far apart
    scaling = (spacing * torch.exp(0.3 * torch.randn(P, 3, generator=g))).to(dev)
    quaternions = torch.randn(P, 4, generator=g).to(dev)
    strengths = torch.sigmoid(torch.randn(P, 1, generator=g)).to(dev)
    knn_idx = knn_points(points[None], points[None], K=K).idx[0]
    gaussian_idx = torch.randint(0, P, (N,), generator=g).to(dev)
    idx = knn_idx[gaussian_idx].contiguous()
    x = points[gaussian_idx] + scaling[gaussian_idx].mean(-1, keepdim=True) * torch.randn(N, 3, generator=g).to(dev)
    params = [t.requires_grad_(True) for t in (x, points, scaling, quaternions, strengths)]
    factor = 1.0 / K

    def zero():
        for t in params:
            t.grad = None

    def fused(recompute, backward=True):
        def run():
            f = field_values(params[0], idx, *params[1:], beta_mode=a.mode, density_factor=factor, validate_idx=False, _recompute=recompute)
            if backward:
                zero()
                (f["sdf"].sum() + f["density"].sum()).backward()
            return f
        return run

    def chain(backward=True):
        def run():
            f = eager(params[0], idx, *params[1:], a.mode, factor)
            if backward:
                zero()
                (f["sdf"].sum() + f["density"].sum()).backward()
            return f
        return run

    variants = {"fused_packed": fused(False), "fused_recompute": fused(True), "eager": chain(),
                "fused_packed_fwd": fused(False, False), "fused_recompute_fwd": fused(True, False), "eager_fwd": chain(False)}
    for fn in variants.values():                                   # warm-up: code objects, the allocator's blocks, rocPRIM's choices
        fn(); fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(3):
        for name, fn in variants.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            torch.cuda.synchronize()
            rounds[name].append((time.perf_counter() - t0) / a.reps * 1e3)
    ms = {k: sorted(v)[1] for k, v in rounds.items()}

    # agreement at the timed size: the fused op against the eager chain (both float32)
    zero(); f = variants["fused_packed"](); mine = [t.grad.clone() for t in params]
    zero(); e = variants["eager"](); theirs = [t.grad.clone() for t in params]
    rel = lambda u, v: float((u - v).norm() / v.norm().clamp(min=1e-30))
    agree = {"sdf": rel(f["sdf"].detach(), e["sdf"].detach()), "density": rel(f["density"].detach(), e["density"].detach())}
    agree.update({f"grad_{n}": rel(u, v) for n, u, v in zip(("x", "points", "scaling", "quaternions", "strengths"), mine, theirs)})

    # what the forward's gather has to move: an index and a 64-byte record per pair (packed), or the 44 bytes of the four arrays
    pairs = N * K
    gather_bytes = pairs * (8 + 64) + N * 12
    out = {"tool": "field_bench", "device": torch.cuda.get_device_name(0), "N": N, "P": P, "K": K, "beta_mode": a.mode, "reps": a.reps,
           "ms_median_of_3_rounds": {k: round(v, 3) for k, v in ms.items()}, "ms_rounds": {k: [round(x, 3) for x in v] for k, v in rounds.items()},
           "eager_over_fused_fwd_bwd": round(ms["eager"] / ms["fused_packed"], 2),
           "forward_gather_bytes_packed": gather_bytes,
           "forward_gather_GBps_packed": round(gather_bytes / (ms["fused_packed_fwd"] * 1e-3) / 1e9, 1),
           "forward_includes": "the record pack pre-pass (P x 44 B read, 64 B written) and the allocator",
           "density_ge_1_rows": int((f["density"] >= 1).sum()), "relative_l2_fused_vs_eager": {k: float(f"{v:.3e}") for k, v in agree.items()},
           "peak_memory_GB": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2)}
    assert all(math.isfinite(v) for v in agree.values()), agree
    print(json.dumps(out))


if __name__ == "__main__":
    main()
