"""Times adaptive density control at the C3 shape (3 M Gaussians, SH degree 3) against the eager routes it replaces, in
one process on one GPU: hipEvents around every timed region, warm-up first, medians over repeats.

    python tools/time_densify.py [P]

  add_stats          DensityControl.add_stats (one launch) | parallel.DensificationStats.update without a process group
  densify_and_prune  frg_densify_plan + the size read-back + frg_densify_apply | the same result through torch masks and
                     FlatAdam.append, append, prune, prune (four rebuilds of the three flat buffers)
  apply              frg_densify_apply alone, as a fraction of 8 TB/s over 3 * 236 B * (P + P') algorithmic bytes
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import densify_oracle as O
from frosting_amd import scenes
from frosting_amd.densify import DensityControl
from frosting_amd.optim import FlatAdam
from frosting_amd.parallel import PARAM_ORDER, DensificationStats, ViewParallelRasterizer

dev = torch.device("cuda:0")
P = int(sys.argv[1]) if len(sys.argv) > 1 else None
scene, cam, bg = scenes.config_scene("c3", 0, P=P)
P, PD = scene.P, 0.01
shapes = {k: tuple(getattr(scene, k).shape) for k in PARAM_ORDER}
lrs = dict(means3D=1.6e-5, scales=5e-3, rotations=1e-3, opacities=5e-2, shs=2.5e-3)


def timed(fn, warmup, reps, setup=None):
    ms = []
    for i in range(warmup + reps):
        state = setup() if setup else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn(state) if setup else fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def new_optimizer():
    opt = FlatAdam(shapes, lrs, dev)
    s = scene.to(dev)
    opt.params["means3D"].copy_(s.means3D); opt.params["shs"].copy_(s.shs)
    opt.params["scales"].copy_(torch.log(s.scales)); opt.params["rotations"].copy_(s.rotations * 1.7)
    opt.params["opacities"].copy_(torch.log(s.opacities / (1 - s.opacities)))
    g = torch.Generator(device=dev).manual_seed(1)
    opt.exp_avg.copy_(torch.randn(opt.numel, device=dev, generator=g)); opt.exp_avg_sq.copy_(torch.rand(opt.numel, device=dev, generator=g))
    opt.steps = 100
    return opt


opt = new_optimizer()
dc = DensityControl(opt, percent_dense=PD)
live = scenes.Scene(opt.params["means3D"], opt.params["scales"], opt.params["rotations"], opt.params["opacities"], opt.params["shs"], scene.sh_degree)
vpr = ViewParallelRasterizer(live, dev, raw_params=True)
views = []
for view in (0, 2, 5):
    c = scenes.config_scene("c3", view, P=8)[1].to(dev)
    img, radii = vpr.forward(c, bg.to(dev))
    vpr.backward(scenes.l1_target_grad(img, view)[0])
    dc.add_stats(radii, vpr.dL_dmeans2D)
    views.append((radii.clone(), vpr.dL_dmeans2D.clone()))
del vpr

# ---- add_stats ----
radii, grad = views[0]
eager = DensificationStats(P, dev)
scratch = DensityControl(new_optimizer(), percent_dense=PD)
t_dev = timed(lambda: scratch.add_stats(radii, grad), 5, 30)
t_eager = timed(lambda: eager.update(radii, grad), 5, 30)
print(f"add_stats          P {P}: device {t_dev[0]:.4f} ms [{t_dev[1]:.4f}, {t_dev[2]:.4f}] | DensificationStats.update {t_eager[0]:.4f} ms "
      f"[{t_eager[1]:.4f}, {t_eager[2]:.4f}] | x{t_eager[0] / t_dev[0]:.1f}")
del scratch, eager

# ---- thresholds: about a fifth of the rows selected, half of them large ----
g = (dc.xyz_gradient_accum / dc.denom).reshape(-1)
g[g.isnan()] = 0.0
seen = float((g > 0).double().mean())
frac = min(0.2, 0.9 * seen)
max_grad = float(torch.sort(g).values[int((1 - frac) * P)])
smax = torch.exp(opt.params["scales"]).max(dim=1).values
extent = float(smax[g >= max_grad].double().median()) / PD
min_opacity = float(torch.sort(torch.sigmoid(opt.params["opacities"]).reshape(-1)).values[int(0.03 * P)])
noise = torch.randn((P, 2, 3), device=dev)
accum, denom = dc.xyz_gradient_accum, dc.denom
names = list(PARAM_ORDER)
widths = [int(torch.Size(shapes[k][1:]).numel()) for k in names]
src_off = [opt.layout[k][0] for k in names]
ops = dc.ops
last = {}


def device_route():
    plan, record = ops.densify_plan(opt.params["scales"], opt.params["opacities"], accum, denom, max_grad, min_opacity, extent, PD, True)
    sizes = [int(x) for x in record.cpu()]
    from frosting_amd.parallel import flat_layout
    _, layout, numel = flat_layout({k: (sizes[4],) + shapes[k][1:] for k in names}, names)
    out = ops.densify_apply(plan, sizes[4], widths, src_off, [layout[k][0] for k in names], numel, noise, opt.flat, opt.exp_avg, opt.exp_avg_sq)
    last.update(plan=plan, sizes=sizes, layout=layout, numel=numel, out=out)


t_route = timed(device_route, 2, 7)
sizes = last["sizes"]
t_plan = timed(lambda: ops.densify_plan(opt.params["scales"], opt.params["opacities"], accum, denom, max_grad, min_opacity, extent, PD, True), 3, 15)
t_apply = timed(lambda: ops.densify_apply(last["plan"], sizes[4], widths, src_off, [last["layout"][k][0] for k in names], last["numel"], noise,
                                          opt.flat, opt.exp_avg, opt.exp_avg_sq), 3, 15)
bytes_apply = 3 * 236 * (P + sizes[4])
print(f"densify_and_prune  P {P} -> {sizes[4]} (kept {sizes[0]}, cloned {sizes[1]}, split {sizes[2]} x 2; seen {seen:.3f}): device route "
      f"{t_route[0]:.3f} ms [{t_route[1]:.3f}, {t_route[2]:.3f}] = plan {t_plan[0]:.3f} ms + read-back + allocation + apply {t_apply[0]:.3f} ms")
print(f"apply              {bytes_apply / 1e9:.3f} GB algorithmic in {t_apply[0]:.3f} ms [{t_apply[1]:.3f}, {t_apply[2]:.3f}] = "
      f"{bytes_apply / t_apply[0] / 1e9:.2f} TB/s = {bytes_apply / t_apply[0] / 1e9 / 8.0:.3f} of 8 TB/s")
last.clear()


def torch_route(o):
    p = o.params
    gr = (accum / denom).reshape(-1)
    gr[gr.isnan()] = 0.0
    s = torch.exp(p["scales"])
    big = s.max(dim=1).values > PD * extent
    sel = gr >= max_grad
    clone, split = sel & ~big, sel & big
    new = {k: p[k][clone] for k in names}
    src = {k: p[k][split] for k in names}
    o.append(new)
    kids = {k: src[k].repeat(2, *([1] * (src[k].dim() - 1))) for k in names}
    z = torch.cat((noise[split][:, 0], noise[split][:, 1]))
    kids["means3D"] = torch.bmm(O.rotation_matrices(src["rotations"]).repeat(2, 1, 1), (s[split].repeat(2, 1) * z).unsqueeze(-1)).squeeze(-1) + kids["means3D"]
    kids["scales"] = torch.log(s[split].repeat(2, 1) / 1.6)
    o.append(kids)
    n_new = int(clone.sum()) + 2 * int(split.sum())
    o.prune(torch.cat((~split, torch.ones(n_new, dtype=torch.bool, device=dev))))
    p = o.params
    prune = (torch.sigmoid(p["opacities"]).reshape(-1) < min_opacity) | (torch.exp(p["scales"]).max(dim=1).values > 0.1 * extent)
    o.prune(~prune)
    last["rows"] = o.params["means3D"].shape[0]


del opt, dc
t_torch = timed(torch_route, 1, 3, setup=new_optimizer)
print(f"                   torch route (masks, append, append, prune, prune) -> {last['rows']} rows: {t_torch[0]:.3f} ms [{t_torch[1]:.3f}, {t_torch[2]:.3f}] "
      f"| x{t_torch[0] / t_route[0]:.1f} of the device route")
