"""CPU tier of adaptive density control: the fixtures the reference produced (tools/make_golden_densify.py) are
self-consistent and satisfy the condition that makes them independent of the last place of exp / sigmoid, and the torch
restatement the GPU tier uses at sizes no fixture can have (tests/densify_oracle.py) reproduces every one of them."""
import os

import numpy as np
import pytest
import torch

import densify_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["densify_deg3_screen", "densify_deg1_noscreen", "densify_identity"]


def load(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
        return dict(f)


def test_fixture_set():
    """SH degree 3 with a screen size, SH degree 1 without, a case that changes nothing, rows with denom = 0; no file larger
    than the largest raster fixture."""
    a, b, c = (load(n) for n in CASES)
    assert a["in_shs"].shape[1] == 16 and a["max_screen_size"] == 20
    assert b["in_shs"].shape[1] == 4 and b["max_screen_size"] == 0
    assert list(c["sizes"]) == [c["in_means3D"].shape[0], 0, 0, 0, c["in_means3D"].shape[0]]
    for fx in (a, b):
        assert (fx["denom"] == 0).any() and min(fx["sizes"][:3]) > 0
        assert fx["sizes"][4] < fx["in_means3D"].shape[0] + fx["sizes"][1] + 2 * fx["sizes"][2]      # something was pruned
    largest = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.endswith(".npz") and not f.startswith("densify_"))
    for f in os.listdir(GOLDEN):
        if f.startswith("densify_"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) <= largest, f


@pytest.mark.parametrize("name", CASES)
def test_fixture_condition_and_consistency(name):
    fx = load(name)
    t = torch.from_numpy
    th = O.fixture_thresholds(fx)
    band = O.band_rows(t(fx["in_scales"]), t(fx["in_opacities"]), t(fx["accum"]), t(fx["denom"]), th["max_grad"], th["min_opacity"],
                       th["extent"], th["percent_dense"])
    assert int(band.sum()) == 0, "a fixture row sits within 8 ulps of a threshold"
    sizes = [int(x) for x in fx["sizes"]]
    assert sum(sizes[:4]) == sizes[4] and sizes[2] == sizes[3]
    P = fx["in_means3D"].shape[0]
    assert fx["noise"].shape == (P, 2, 3)
    for n in O.NAMES:
        for tag in ("", "_m", "_v"):
            assert fx[f"out{tag}_{n}"].shape[0] == sizes[4]
            assert fx[f"out{tag}_{n}"].shape[1:] == fx[f"in{tag}_{n}"].shape[1:]
        # new rows start with zero moments
        assert not fx[f"out_m_{n}"][sizes[0]:].any() and not fx[f"out_v_{n}"][sizes[0]:].any()
    # the statistics of the new model are zeros of its length (the quirk: max_radii2D is zero BEFORE the prune read it)
    assert fx["out_accum"].shape == (sizes[4], 1) and fx["out_denom"].shape == (sizes[4], 1) and fx["out_max_radii2D"].shape == (sizes[4],)
    assert not fx["out_accum"].any() and not fx["out_denom"].any() and not fx["out_max_radii2D"].any()


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference(name):
    """Row order and every copied row bit for bit; the two computed quantities (children's xyz and raw scale) too: the same
    torch ops on the same CPU."""
    fx = load(name)
    (p, m, v), (rp, rm, rv) = O.fixture_tensors(fx)
    th = O.fixture_thresholds(fx)
    t = torch.from_numpy
    op, om, ov, sizes, masks = O.densify(p, m, v, t(fx["accum"]), t(fx["denom"]), noise=t(fx["noise"]), **th)
    assert sizes == [int(x) for x in fx["sizes"]]
    for n in O.NAMES:
        assert torch.equal(op[n], rp[n]), n
        assert torch.equal(om[n], rm[n]) and torch.equal(ov[n], rv[n]), n
    if th["max_screen_size"]:
        # the screen-size quirk: survivors include rows whose max_radii2D exceeds the screen size
        assert bool((t(fx["max_radii2D"])[masks["kept"]] > th["max_screen_size"]).any())


def test_restatement_reset_opacity():
    fx = load("densify_reset_opacity")
    out = O.reset_opacity(torch.from_numpy(fx["in_opacities"]))
    assert torch.equal(out, torch.from_numpy(fx["out_opacities"]))
    assert not fx["out_m_opacities"].any() and not fx["out_v_opacities"].any()
    assert fx["in_m_opacities"].any() and fx["in_v_opacities"].any()
    # the reference's float32 evaluation against the float64 one: the yardstick the GPU tier uses
    assert O.reset_opacity_error(torch.from_numpy(fx["out_opacities"]), torch.from_numpy(fx["in_opacities"])) < 1e-5


def test_noise_convention():
    """noise[i, c] is child c of SOURCE row i: permuting the samples of rows that do not split changes nothing."""
    fx = load("densify_deg1_noscreen")
    (p, m, v), _ = O.fixture_tensors(fx)
    th = O.fixture_thresholds(fx)
    t = torch.from_numpy
    a = O.densify(p, m, v, t(fx["accum"]), t(fx["denom"]), noise=t(fx["noise"]), **th)
    noise = t(fx["noise"]).clone()
    noise[~a[4]["split"]] = 0.0
    b = O.densify(p, m, v, t(fx["accum"]), t(fx["denom"]), noise=noise, **th)
    assert torch.equal(a[0]["means3D"], b[0]["means3D"])


def test_density_control_refuses_what_it_cannot_do():
    """No CPU path, and no ShardedFlatAdam (its moments exist per shard only)."""
    from frosting_amd.densify import DensityControl
    from frosting_amd.optim import FlatAdam, ShardedFlatAdam
    shapes = dict(means3D=(4, 3), scales=(4, 3), rotations=(4, 4), opacities=(4, 1), shs=(4, 1, 3))
    with pytest.raises(RuntimeError, match="GPU only"):
        DensityControl(FlatAdam(shapes, {k: 1e-3 for k in shapes}, "cpu"))
    with pytest.raises(TypeError, match="ShardedFlatAdam"):
        DensityControl(object.__new__(ShardedFlatAdam))
    with pytest.raises(ValueError, match="begin with"):
        DensityControl(FlatAdam(dict(means3D=(4, 3), opacities=(4, 1)), dict(means3D=1e-3, opacities=1e-3), "cpu"))


def test_flat_adam_adopt_on_cpu_buffers():
    """The swap itself needs no GPU: layout, views and segment ends follow the new row count; steps and rates stay."""
    from frosting_amd.optim import FlatAdam
    from frosting_amd.parallel import flat_layout
    shapes = dict(means3D=(5, 3), scales=(5, 3), rotations=(5, 4), opacities=(5, 1), shs=(5, 4, 3))
    opt = FlatAdam(shapes, {k: 1e-3 for k in shapes}, "cpu")
    opt.steps = 9
    new_shapes = {k: (7,) + v[1:] for k, v in shapes.items()}
    _, layout, numel = flat_layout(new_shapes, opt.names)
    bufs = [torch.arange(numel, dtype=torch.float32) + i for i in range(3)]
    params = opt.adopt(7, *bufs)
    assert opt.steps == 9 and opt.numel == numel and opt.layout == layout and params is opt.params
    assert opt.flat is bufs[0] and opt.exp_avg is bufs[1] and opt.exp_avg_sq is bufs[2]
    assert tuple(params["shs"].shape) == (7, 4, 3) and params["shs"].data_ptr() == bufs[0][layout["shs"][0]:].data_ptr()
    assert list(opt._ends) == [layout[k][0] for k in opt.names[1:]] + [numel]
    with pytest.raises(RuntimeError, match="adopt"):
        opt.adopt(8, *bufs)
