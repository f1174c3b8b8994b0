"""GPU tier of adaptive density control (frosting_amd/densify.py, csrc/densify.hip) against the fixtures the reference
produced (tools/make_golden_densify.py), against float64 evaluations of its formulas, and -- at sizes no fixture can
have -- against the torch restatement tests/densify_oracle.py, which the CPU tier ties to the same fixtures.

Measured on an MI355X (distance from the float64 evaluation; the yardstick is the reference's own float32 distance, ours may
sit at up to twice it).  With exp and log correctly rounded in the kernel ours lands on the reference's figure:
    children's xyz        ours 9.99e-08  reference 9.99e-08 (deg3_screen);  ours 1.37e-07  reference 1.37e-07 (deg1_noscreen)
    children's raw scale  ours 2.63e-07  reference 2.63e-07 (deg3_screen);  ours 4.52e-07  reference 4.52e-07 (deg1_noscreen)
    reset opacity         ours 8.04e-08  reference 8.04e-08
(with the device library's one-ulp expf / logf the raw scale of deg1_noscreen read 9.29e-07: 2.05 x the yardstick.)
add_stats at C2, three views: 1.10, 1.65, 1.80 ulps from the float64 sum (bound 4 per call).  C3: 2 of 3 M rows inside
the 8-ulp bands (cap 30).
"""
import os

import numpy as np
import pytest
import torch

import densify_oracle as O
from frosting_amd import scenes
from frosting_amd.optim import FlatAdam
from frosting_amd.parallel import PARAM_ORDER, ViewParallelRasterizer

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LRS = dict(means3D=1.6e-4, scales=5e-3, rotations=1e-3, opacities=5e-2, shs=2.5e-3)
YARDSTICK_FACTOR = 2.0


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        return dict(f)


def control_from(params, m, v, dev, binding="ctypes", steps=1, percent_dense=0.01):
    from frosting_amd.densify import DensityControl
    shapes = {k: tuple(params[k].shape) for k in PARAM_ORDER}
    opt = FlatAdam(shapes, LRS, dev)
    for k in PARAM_ORDER:
        opt.params[k].copy_(params[k]); opt.m[k].copy_(m[k]); opt.v[k].copy_(v[k])
    opt.steps = steps
    return opt, DensityControl(opt, percent_dense=percent_dense, binding=binding)


def control_from_fixture(fx, dev, binding="ctypes"):
    (p, m, v), outs = O.fixture_tensors(fx)
    opt, dc = control_from(p, m, v, dev, binding, steps=int(fx["adam_steps"]), percent_dense=float(fx["percent_dense"]))
    dc.xyz_gradient_accum.copy_(torch.from_numpy(fx["accum"])); dc.denom.copy_(torch.from_numpy(fx["denom"]))
    dc.max_radii2D.copy_(torch.from_numpy(fx["max_radii2D"]))
    return opt, dc, (p, m, v), outs


def same_bytes(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 1. / 6. against the fixtures, through both bindings ---------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("binding", ["ctypes", "ext"])
@pytest.mark.parametrize("name", ["densify_deg3_screen", "densify_deg1_noscreen", "densify_identity"])
def test_densify_and_prune_against_reference_fixture(gpu_device, name, binding):
    fx = load(name)
    opt, dc, (p, m, v), (rp, rm, rv) = control_from_fixture(fx, gpu_device, binding)
    th = O.fixture_thresholds(fx)
    old_flat = opt.flat
    params, sizes = dc.densify_and_prune(th["max_grad"], th["min_opacity"], th["extent"], th["max_screen_size"],
                                         noise=torch.from_numpy(fx["noise"]).to(gpu_device))
    want = [int(x) for x in fx["sizes"]]
    assert [sizes[k] for k in ("kept", "cloned", "split_first", "split_second", "total")] == want
    nA, nB, nC = want[:3]
    assert params is opt.params and opt.flat is not old_flat and opt.steps == int(fx["adam_steps"])
    for k in PARAM_ORDER:
        assert tuple(params[k].shape) == tuple(rp[k].shape), k
        # moments: survivors carry theirs, new rows start at zero -- every byte
        assert same_bytes(opt.m[k], rm[k]) and same_bytes(opt.v[k], rv[k]), k
    for k in ("rotations", "opacities", "shs"):
        assert same_bytes(params[k], rp[k]), k                      # whole tensors: the order is the reference's
    for k in ("means3D", "scales"):
        assert same_bytes(params[k][: nA + nB], rp[k][: nA + nB]), k
    # the alignment pads of the new layout are zero, in all three buffers
    for k, (o, n) in opt.layout.items():
        end = min([o2 for (o2, _) in opt.layout.values() if o2 > o] + [opt.numel])
        for buf in (opt.flat, opt.exp_avg, opt.exp_avg_sq):
            assert not bool(buf[o + n:end].any()), k
    # statistics of the new model: zeros of its length
    assert tuple(dc.xyz_gradient_accum.shape) == (want[4], 1) and tuple(dc.denom.shape) == (want[4], 1) and tuple(dc.max_radii2D.shape) == (want[4],)
    for t in (dc.xyz_gradient_accum, dc.denom, dc.max_radii2D):
        assert same_bytes(t, torch.zeros(t.shape))
    if nC == 0:
        return
    # children's xyz and raw scale against a float64 evaluation of the reference's formulas; yardstick: the fixture's own distance
    split = O.classify(p["scales"], p["opacities"], torch.from_numpy(fx["accum"]), torch.from_numpy(fx["denom"]), **th)["split"]
    assert int(split.sum()) == nC
    src = (p["means3D"][split], p["scales"][split], p["rotations"][split])
    noise = torch.from_numpy(fx["noise"])[split]
    worst = {"ours": [0.0, 0.0], "reference": [0.0, 0.0]}
    for child in (0, 1):
        rows = slice(nA + nB + child * nC, nA + nB + (child + 1) * nC)
        for who, out in (("ours", {k: params[k].cpu() for k in ("means3D", "scales")}), ("reference", rp)):
            e = O.children_error(out["means3D"][rows], out["scales"][rows], *src, noise[:, child])
            worst[who] = [max(a, b) for a, b in zip(worst[who], e)]
    print(f"\n[{name}, {binding}] children vs float64: xyz ours {worst['ours'][0]:.2e} reference {worst['reference'][0]:.2e} | "
          f"raw scale ours {worst['ours'][1]:.2e} reference {worst['reference'][1]:.2e}")
    assert worst["reference"][0] > 0 and worst["reference"][1] > 0
    assert worst["ours"][0] <= YARDSTICK_FACTOR * worst["reference"][0], worst
    assert worst["ours"][1] <= YARDSTICK_FACTOR * worst["reference"][1], worst


# ---- 2. the opacity reset ---------------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("binding", ["ctypes", "ext"])
def test_reset_opacity_against_reference_fixture(gpu_device, binding):
    fx = load("densify_reset_opacity")
    P = fx["in_opacities"].shape[0]
    g = torch.Generator().manual_seed(5)
    p = dict(means3D=torch.randn(P, 3, generator=g), scales=torch.randn(P, 3, generator=g), rotations=torch.randn(P, 4, generator=g),
             opacities=torch.from_numpy(fx["in_opacities"]), shs=torch.randn(P, 1, 3, generator=g))
    m = {k: torch.randn(p[k].shape, generator=g) for k in p}
    v = {k: torch.rand(p[k].shape, generator=g) for k in p}
    m["opacities"], v["opacities"] = torch.from_numpy(fx["in_m_opacities"]), torch.from_numpy(fx["in_v_opacities"])
    opt, dc = control_from(p, m, v, gpu_device, binding)
    before = opt.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone()
    dc.reset_opacity()
    assert same_bytes(opt.m["opacities"], torch.from_numpy(fx["out_m_opacities"])) and same_bytes(opt.v["opacities"], torch.from_numpy(fx["out_v_opacities"]))
    assert not bool(opt.m["opacities"].any()) and not bool(opt.v["opacities"].any())
    # nothing outside the opacity segment moved
    o, n = opt.layout["opacities"]
    for now, was in zip((opt.flat, opt.exp_avg, opt.exp_avg_sq), before):
        assert torch.equal(now[:o], was[:o]) and torch.equal(now[o + n:], was[o + n:])
    raw_in = torch.from_numpy(fx["in_opacities"])
    ours = O.reset_opacity_error(opt.params["opacities"].cpu(), raw_in)
    ref = O.reset_opacity_error(torch.from_numpy(fx["out_opacities"]), raw_in)
    print(f"\n[reset_opacity, {binding}] raw opacity vs float64: ours {ours:.2e} reference {ref:.2e}")
    assert ref > 0 and ours <= YARDSTICK_FACTOR * ref, (ours, ref)


# ---- 3. statistics on a real backward -----------------------------------------------------------------------------------------
def raw_scene_of(scene, dev):
    s = scene.to(dev)
    return scenes.Scene(s.means3D, torch.log(s.scales), s.rotations * 1.7, torch.log(s.opacities / (1 - s.opacities)), s.shs, s.sh_degree)


def render_and_backward(vpr, cam, bg, dev, seed):
    img, radii = vpr.forward(cam.to(dev), bg.to(dev))
    gpix, _ = scenes.l1_target_grad(img, seed)
    vpr.backward(gpix)
    return radii, vpr.dL_dmeans2D


@pytest.mark.timeout(300)
def test_add_stats_on_a_real_backward(gpu_device):
    from frosting_amd.densify import DensityControl
    dev = gpu_device
    scene, _, bg = scenes.config_scene("c2", 0)
    raw = raw_scene_of(scene, dev)
    P = scene.P
    shapes = {k: tuple(getattr(scene, k).shape) for k in PARAM_ORDER}
    dense_dc = DensityControl(FlatAdam(shapes, LRS, dev))
    live_dc = DensityControl(FlatAdam(shapes, LRS, dev), binding="ext")
    vpr = ViewParallelRasterizer(raw, dev, raw_params=True)
    vpr_live = ViewParallelRasterizer(raw, dev, raw_params=True, live_rows=True)
    acc64 = torch.zeros(P, dtype=torch.float64, device=dev)
    den64 = torch.zeros(P, dtype=torch.float64, device=dev)
    rad64 = torch.zeros(P, dtype=torch.float64, device=dev)
    for n, view in enumerate((0, 1, 2), start=1):
        cam = scenes.config_scene("c2", view, P=8)[1]
        radii, grad = render_and_backward(vpr, cam, bg, dev, seed=view)
        dense_dc.add_stats(radii, grad)
        vis = radii > 0
        assert 0 < int(vis.sum()) < P
        g = grad.double()
        acc64 += torch.where(vis, torch.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]), torch.zeros_like(acc64))
        den64 += vis.double()
        rad64 = torch.where(vis, torch.maximum(rad64, radii.double()), rad64)
        assert torch.equal(dense_dc.denom.reshape(-1).double(), den64)
        assert torch.equal(dense_dc.max_radii2D.double(), rad64)
        # two products, one sum, one root, a running add: 4 float32 ulps per call
        ulp = torch.from_numpy(np.spacing(acc64.float().cpu().numpy())).to(dev).double()
        err = ((dense_dc.xyz_gradient_accum.reshape(-1).double() - acc64).abs() / ulp).max()
        print(f"\n[add_stats, view {view}] accum vs float64: {float(err):.2f} ulps, {int(vis.sum())} visible rows")
        assert float(err) <= 4.0 * n
        # the same view through a live_rows backward: unmarked rows are not read and count as zero -- the same bytes
        radii_l, grad_l = render_and_backward(vpr_live, cam, bg, dev, seed=view)
        assert 0 < int(vpr_live.row_live.sum()) < P
        grad_l[vpr_live.row_live == 0] = float("nan")          # whatever an unwritten row holds must not matter
        live_dc.add_stats(radii_l, grad_l, row_live=vpr_live.row_live)
        for a, b in ((dense_dc.xyz_gradient_accum, live_dc.xyz_gradient_accum), (dense_dc.denom, live_dc.denom), (dense_dc.max_radii2D, live_dc.max_radii2D)):
            assert same_bytes(a, b)
    assert float(dense_dc.denom.max()) >= 2.0


# ---- 4. scale: 3 M Gaussians against the restatement on the same GPU ---------------------------------------------------------
@pytest.mark.timeout(900)
def test_densify_at_scale_against_the_restatement(gpu_device):
    from frosting_amd.densify import DensityControl
    dev = gpu_device
    scene, _, bg = scenes.config_scene("c3", 0)
    P, pd = scene.P, 0.01
    raw = raw_scene_of(scene, dev)
    shapes = {k: tuple(getattr(scene, k).shape) for k in PARAM_ORDER}
    opt = FlatAdam(shapes, LRS, dev)
    for k in PARAM_ORDER:
        opt.params[k].copy_(getattr(raw, k).reshape(shapes[k]))
    g = torch.Generator(device=dev).manual_seed(11)
    opt.exp_avg.copy_(torch.randn(opt.numel, device=dev, generator=g)); opt.exp_avg_sq.copy_(torch.rand(opt.numel, device=dev, generator=g))
    opt.steps = 7
    dc = DensityControl(opt, percent_dense=pd)
    live = scenes.Scene(opt.params["means3D"], opt.params["scales"], opt.params["rotations"], opt.params["opacities"], opt.params["shs"], scene.sh_degree)
    vpr = ViewParallelRasterizer(live, dev, raw_params=True)
    for view in (0, 2, 5):
        cam = scenes.config_scene("c3", view, P=8)[1]
        radii, grad = render_and_backward(vpr, cam, bg, dev, seed=view)
        dc.add_stats(radii, grad)
    del vpr
    # thresholds from the statistics: about a fifth of the rows selected (fewer if fewer were seen), half of them large
    grad = (dc.xyz_gradient_accum / dc.denom).reshape(-1)
    grad[grad.isnan()] = 0.0
    seen = float((grad > 0).double().mean())
    frac = min(0.2, 0.9 * seen)
    order = torch.sort(grad).values
    max_grad = float(0.5 * (order[int((1 - frac) * P)].double() + order[int((1 - frac) * P) - 1].double()))
    smax = torch.exp(opt.params["scales"]).max(dim=1).values
    extent = float(smax[grad >= max_grad].double().median()) / pd * 1.0000123
    min_opacity = float(torch.sort(torch.sigmoid(opt.params["opacities"]).reshape(-1)).values[int(0.03 * P)].double()) * 1.0000123
    accum, denom = dc.xyz_gradient_accum.clone(), dc.denom.clone()
    noise = torch.randn((P, 2, 3), device=dev, generator=g)
    old = dict(flat=opt.flat, m=opt.exp_avg, v=opt.exp_avg_sq, layout=dict(opt.layout))
    src = {k: opt.params[k] for k in PARAM_ORDER}
    src_m, src_v = dict(opt.m), dict(opt.v)
    args = (max_grad, min_opacity, extent, 20)

    band = O.band_rows(src["scales"], src["opacities"], accum, denom, max_grad, min_opacity, extent, pd)
    n_band = int(band.sum())
    want = O.classify(src["scales"], src["opacities"], accum, denom, max_grad, min_opacity, extent, pd, 20)

    params, sizes = dc.densify_and_prune(*args, noise=noise)
    plan = dc.last_plan
    ours = dict(kept=plan[0] >= 0, cloned=plan[1] >= 0, split=plan[2] >= 0)
    print(f"\n[scale] P {P} -> {sizes}; seen {seen:.3f}; rows inside the 8-ulp bands {n_band}; max_grad {max_grad:.3e} extent {extent:.3f} min_opacity {min_opacity:.3e}")
    assert n_band <= 1e-5 * P
    assert sizes["cloned"] > 0.03 * P and sizes["split_first"] > 0.03 * P and sizes["kept"] < P - sizes["split_first"]
    differ = torch.zeros(P, dtype=torch.bool, device=dev)
    for k in ours:
        differ |= ours[k] != want[k]
    assert not bool((differ & ~band).any()), f"{int((differ & ~band).sum())} decisions differ outside the bands"
    assert bool(((plan[3] >= 0) == ours["split"]).all())
    # the order: every section ascending in the source index, sections back to back
    nA, nB, nC = sizes["kept"], sizes["cloned"], sizes["split_first"]
    for row, (mask, base) in enumerate(((ours["kept"], 0), (ours["cloned"], nA), (ours["split"], nA + nB), (ours["split"], nA + nB + nC))):
        rank = torch.cumsum(mask.int(), 0, dtype=torch.int32) - 1 + base
        assert torch.equal(plan[row][mask], rank[mask]) and int(mask.sum()) == (nA, nB, nC, nC)[row]
    assert sizes["total"] == nA + nB + 2 * nC and tuple(params["shs"].shape) == (sizes["total"],) + shapes["shs"][1:]
    # copied bytes: survivors with their moments, new rows with zero moments; children copy everything but xyz and scale
    A, B, C = (torch.nonzero(ours[k]).reshape(-1) for k in ("kept", "cloned", "split"))
    for k in PARAM_ORDER:
        assert torch.equal(params[k][:nA], src[k][A]) and torch.equal(opt.m[k][:nA], src_m[k][A]) and torch.equal(opt.v[k][:nA], src_v[k][A]), k
        assert torch.equal(params[k][nA:nA + nB], src[k][B]), k
        assert not bool(opt.m[k][nA:].any()) and not bool(opt.v[k][nA:].any()), k
        if k not in ("means3D", "scales"):
            assert torch.equal(params[k][nA + nB:nA + nB + nC], src[k][C]) and torch.equal(params[k][nA + nB + nC:], src[k][C]), k
    # the children against the restatement's float32 evaluation on the same GPU (a different exp / log: a loose sanity bound)
    for child in (0, 1):
        xyz, sc = O.children(src["means3D"][C], src["scales"][C], src["rotations"][C], noise[C][:, child])
        rows = slice(nA + nB + child * nC, nA + nB + (child + 1) * nC)
        torch.testing.assert_close(params["means3D"][rows], xyz, rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(params["scales"][rows], sc, rtol=1e-5, atol=1e-5)
    # run to run: the same inputs give the same bytes
    names = list(PARAM_ORDER)
    widths = [int(torch.Size(shapes[k][1:]).numel()) for k in names]
    plan2, record2 = dc.ops.densify_plan(src["scales"], src["opacities"], accum, denom, max_grad, min_opacity, extent, pd, True)
    out2 = dc.ops.densify_apply(plan2, sizes["total"], widths, [old["layout"][k][0] for k in names], [opt.layout[k][0] for k in names],
                                opt.numel, noise, old["flat"], old["m"], old["v"])
    assert torch.equal(plan2, plan) and [int(x) for x in record2.cpu()][:5] == [nA, nB, nC, nC, sizes["total"]]
    for a, b in zip(out2, (opt.flat, opt.exp_avg, opt.exp_avg_sq)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 5. it trains ---------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(180)
def test_optimizer_steps_after_a_densification(gpu_device):
    from frosting_amd import fused
    from helpers import settings_for
    dev = gpu_device
    fx = load("densify_deg3_screen")
    th = O.fixture_thresholds(fx)
    opt, dc, (p, m, v), _ = control_from_fixture(fx, dev)
    twin, _ = control_from(p, m, v, dev, steps=int(fx["adam_steps"]))            # the same model, never densified
    params, sizes = dc.densify_and_prune(th["max_grad"], th["min_opacity"], th["extent"], th["max_screen_size"],
                                         noise=torch.from_numpy(fx["noise"]).to(dev))
    assert opt.steps == twin.steps == int(fx["adam_steps"])
    kept = torch.nonzero(dc.last_plan[0] >= 0).reshape(-1)
    nA, nB = sizes["kept"], sizes["cloned"]
    fresh = FlatAdam({k: tuple(params[k].shape) for k in PARAM_ORDER}, LRS, dev)     # the new model with zero moments everywhere
    fresh.flat.copy_(opt.flat)
    fresh.steps = opt.steps
    g = torch.Generator().manual_seed(3)
    grads = {k: 1e-2 * torch.randn(tuple(twin.params[k].shape), generator=g).to(dev) for k in PARAM_ORDER}
    new_grads = {k: 1e-2 * torch.randn(tuple(params[k].shape), generator=g).to(dev) for k in PARAM_ORDER}
    flat_old = torch.zeros(twin.numel, device=dev)
    flat_new = torch.zeros(opt.numel, device=dev)
    for k in PARAM_ORDER:
        new_grads[k][:nA] = grads[k][kept]                                           # a survivor sees the gradient its source sees
        o, n = twin.layout[k]; flat_old[o:o + n] = grads[k].reshape(-1)
        o, n = opt.layout[k]; flat_new[o:o + n] = new_grads[k].reshape(-1)
    opt.step(flat_new); twin.step(flat_old); fresh.step(flat_new)
    assert opt.steps == twin.steps == int(fx["adam_steps"]) + 1
    for k in PARAM_ORDER:
        # a survivor's update is the one it would have had without the densification
        assert torch.equal(opt.params[k][:nA], twin.params[k][kept]) and torch.equal(opt.m[k][:nA], twin.m[k][kept]) and torch.equal(opt.v[k][:nA], twin.v[k][kept]), k
        # a new row's first update: Adam from zero moments under the kept step count
        assert torch.equal(opt.params[k][nA:], fresh.params[k][nA:]) and torch.equal(opt.m[k][nA:], fresh.m[k][nA:]), k
    assert nB > 0
    # forward + backward through the raw-parameter rasterizer on the new model
    _, cam, bg = scenes.config_scene("mini", 0, P=8)
    leaves = {k: opt.params[k].detach().clone().requires_grad_(True) for k in PARAM_ORDER}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    img, radii = fused.rasterize_raw(settings_for(cam, bg, 3, dev), leaves["shs"], leaves["opacities"], leaves["scales"], leaves["rotations"],
                                     means3D=leaves["means3D"], means2D=means2D)
    (img - 0.5).abs().mean().backward()
    assert int((radii > 0).sum()) > 0
    for k in PARAM_ORDER:
        assert leaves[k].grad.shape == leaves[k].shape and bool(torch.isfinite(leaves[k].grad).all()), k
    assert means2D.grad.shape == (sizes["total"], 3) and bool(torch.isfinite(means2D.grad).all())
    dc.add_stats(radii, means2D.grad)
    assert float(dc.denom.sum()) == float((radii > 0).sum())
