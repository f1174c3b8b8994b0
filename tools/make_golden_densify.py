"""Fixtures for adaptive density control, produced by the reference's OWN GaussianModel run on the CPU.

The reference's files are read as text where this tool runs, their literal "cuda" device strings replaced by "cpu" in
memory, and executed; nothing of their text is written anywhere -- only the tensors that go in and come out travel
(tests/golden/densify_*.npz).  plyfile and simple_knn are stubbed (neither is used by the calls made here), the
optimizer is a real torch.optim.Adam(eps=1e-15) with one stepped group per tensor, as training_setup makes it.

The split children's samples are recorded: for the duration of the call torch.normal draws z = randn_like(std), keeps z and
returns mean + std * z; z is then scattered into the [P,2,3] form indexed by source row and child that
frg_densify_apply takes.

    python tools/make_golden_densify.py          # needs the reference (FROSTING_REFERENCE, default /root/reference)
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.join(os.environ.get("FROSTING_REFERENCE", "/root/reference"), "gaussian_splatting")

import densify_oracle as O  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZE_LIMIT = max(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN)
                 if f.endswith(".npz") and not f.startswith("densify_"))


def load_reference():
    """-> the reference's GaussianModel class, every tensor it makes on the CPU."""
    def run(path, name):
        text = open(os.path.join(REF, path)).read().replace('"cuda"', '"cpu"').replace("'cuda'", "'cpu'")
        mod = types.ModuleType(name)
        exec(compile(text, path, "exec"), mod.__dict__)
        return mod

    def stub(name, **attrs):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        return mod

    stub("plyfile", PlyData=None, PlyElement=None)
    stub("simple_knn")
    stub("simple_knn._C", distCUDA2=None)
    utils = stub("utils")
    utils.__path__ = []
    sys.modules["utils.general_utils"] = run("utils/general_utils.py", "utils.general_utils")
    stub("utils.system_utils", mkdir_p=None)
    stub("utils.sh_utils", RGB2SH=None)
    stub("utils.graphics_utils", BasicPointCloud=None)
    torch.cuda.empty_cache = lambda: None
    return run("scene/gaussian_model.py", "ref_gaussian_model").GaussianModel


def make_model(GaussianModel, P, degree, seed, opacity_mean, opacity_std, scale_std, percent_dense=0.01, extent=3.0):
    g = torch.Generator().manual_seed(seed)
    K = (degree + 1) ** 2
    rn = lambda *shape: torch.randn(*shape, generator=g)
    model = GaussianModel(degree)
    model.percent_dense = percent_dense
    P_ = torch.nn.Parameter
    model._xyz = P_(rn(P, 3))
    model._features_dc = P_(0.5 * rn(P, 1, 3))
    model._features_rest = P_(0.1 * rn(P, K - 1, 3))
    model._scaling = P_(float(np.log(percent_dense * extent)) - 0.9 + scale_std * rn(P, 3))
    model._rotation = P_(rn(P, 4))
    model._opacity = P_(opacity_mean + opacity_std * rn(P, 1))
    groups = [("xyz", model._xyz), ("f_dc", model._features_dc), ("f_rest", model._features_rest), ("opacity", model._opacity),
              ("scaling", model._scaling), ("rotation", model._rotation)]
    model.optimizer = torch.optim.Adam([{"params": [t], "lr": 1e-3, "name": n} for n, t in groups], lr=0.0, eps=1e-15)
    for _, t in groups:
        t.grad = 1e-2 * torch.randn(t.shape, generator=g)
    model.optimizer.step()                      # every group's state exists and is not trivial
    model.optimizer.zero_grad(set_to_none=True)
    return model, g


def snapshot(model, tag):
    st = lambda t, key: model.optimizer.state[t][key].detach().clone()
    out = {}
    shs = lambda a, b: torch.cat((a, b), dim=1)
    for suffix, get in (("", lambda t: t.detach().clone()), ("_m", lambda t: st(t, "exp_avg")), ("_v", lambda t: st(t, "exp_avg_sq"))):
        out[f"{tag}{suffix}_means3D"] = get(model._xyz)
        out[f"{tag}{suffix}_scales"] = get(model._scaling)
        out[f"{tag}{suffix}_rotations"] = get(model._rotation)
        out[f"{tag}{suffix}_opacities"] = get(model._opacity)
        out[f"{tag}{suffix}_shs"] = shs(get(model._features_dc), get(model._features_rest))
    return {k: v.numpy() for k, v in out.items()}


def check_bands(fx):
    """The condition on a fixture's inputs: no decision hinges on the last places of exp / sigmoid / a division."""
    t = torch.from_numpy
    th = O.fixture_thresholds(fx)
    band = O.band_rows(t(fx["in_scales"]), t(fx["in_opacities"]), t(fx["accum"]), t(fx["denom"]), th["max_grad"], th["min_opacity"],
                       th["extent"], th["percent_dense"])
    assert int(band.sum()) == 0, f"{int(band.sum())} rows within {O.BAND_ULPS} ulps of a threshold: pick another seed"


def densify_case(GaussianModel, name, P, degree, seed, max_grad, min_opacity, extent, max_screen_size, opacity=(-2.0, 3.0),
                 scale_std=1.2, grad_scale=4e-4):
    model, g = make_model(GaussianModel, P, degree, seed, opacity[0], opacity[1], scale_std, extent=extent)
    denom = torch.randint(0, 6, (P, 1), generator=g).float()                      # rows with denom = 0: the NaN branch
    accum = torch.rand(P, 1, generator=g) * denom * grad_scale
    model.xyz_gradient_accum, model.denom = accum.clone(), denom.clone()
    model.max_radii2D = torch.randint(0, 60, (P,), generator=g).float()
    fx = snapshot(model, "in")
    fx.update(accum=accum.numpy(), denom=denom.numpy(), max_radii2D=model.max_radii2D.numpy(),
              max_grad=np.float64(max_grad), min_opacity=np.float64(min_opacity), extent=np.float64(extent),
              percent_dense=np.float64(model.percent_dense), max_screen_size=np.float64(max_screen_size or 0.0),
              adam_steps=np.int64(1))
    check_bands(fx)

    drawn, prunes = [], []
    normal, prune_points = torch.normal, model.prune_points

    def recording_normal(mean, std):
        z = torch.randn(std.shape, generator=g)
        drawn.append((std.clone(), z))
        return mean + std * z

    def recording_prune(mask):
        prunes.append(mask.clone())
        return prune_points(mask)

    torch.normal, model.prune_points = recording_normal, recording_prune
    try:
        model.densify_and_prune(max_grad, min_opacity, extent, max_screen_size)
    finally:
        torch.normal = normal
        del model.prune_points
    fx.update(snapshot(model, "out"))
    fx.update(out_accum=model.xyz_gradient_accum.numpy(), out_denom=model.denom.numpy(), out_max_radii2D=model.max_radii2D.numpy())

    # the split rows (the first prune drops exactly them) and the section sizes, from the reference's own masks
    (std, z), = drawn
    split_filter, final = prunes
    split = split_filter[:P]
    n_split = int(split.sum())
    n_clone = split_filter.numel() - P - 2 * n_split
    assert z.shape[0] == 2 * n_split
    assert torch.equal(std, torch.exp(torch.from_numpy(fx["in_scales"]))[split].repeat(2, 1))
    noise = torch.randn(P, 2, 3, generator=g)                # rows that do not split carry samples nobody may read
    noise[split, 0], noise[split, 1] = z[:n_split], z[n_split:]
    bounds = np.cumsum([0, P - n_split, n_clone, n_split, n_split])
    keep = ~final
    sizes = [int(keep[bounds[i]:bounds[i + 1]].sum()) for i in range(4)]
    assert sizes[2] == sizes[3] and sum(sizes) == fx["out_means3D"].shape[0]
    fx.update(noise=noise.numpy(), sizes=np.asarray(sizes + [sum(sizes)], dtype=np.int64))
    assert not fx["out_max_radii2D"].any() and not fx["out_accum"].any() and not fx["out_denom"].any()
    save(name, fx)
    print(f"{name}: P {P} -> {sum(sizes)}  sections {sizes}  (selected to clone {n_clone}, to split {n_split})")


def reset_case(GaussianModel, name, P, seed):
    model, _ = make_model(GaussianModel, P, 0, seed, -3.0, 3.0, 1.0)
    fx = {"in_opacities": model._opacity.detach().clone().numpy(),
          "in_m_opacities": model.optimizer.state[model._opacity]["exp_avg"].clone().numpy(),
          "in_v_opacities": model.optimizer.state[model._opacity]["exp_avg_sq"].clone().numpy()}
    model.reset_opacity()
    fx.update(out_opacities=model._opacity.detach().numpy(), out_m_opacities=model.optimizer.state[model._opacity]["exp_avg"].numpy(),
              out_v_opacities=model.optimizer.state[model._opacity]["exp_avg_sq"].numpy())
    assert (torch.sigmoid(torch.from_numpy(fx["in_opacities"])) < 0.01).any() and (torch.sigmoid(torch.from_numpy(fx["in_opacities"])) > 0.01).any()
    save(name, fx)
    print(f"{name}: P {P}")


def save(name, fx):
    path = os.path.join(GOLDEN, name + ".npz")
    np.savez_compressed(path, **fx)
    assert os.path.getsize(path) <= SIZE_LIMIT, (path, os.path.getsize(path), SIZE_LIMIT)


if __name__ == "__main__":
    GM = load_reference()
    densify_case(GM, "densify_deg3_screen", P=300, degree=3, seed=20261016, max_grad=0.0002, min_opacity=0.005, extent=3.0, max_screen_size=20)
    densify_case(GM, "densify_deg1_noscreen", P=700, degree=1, seed=20261017, max_grad=0.0002, min_opacity=0.005, extent=3.0, max_screen_size=None)
    densify_case(GM, "densify_identity", P=150, degree=2, seed=20261018, max_grad=0.0002, min_opacity=0.005, extent=3.0, max_screen_size=None,
                 opacity=(3.0, 0.5), grad_scale=3e-5)
    reset_case(GM, "densify_reset_opacity", P=1000, seed=20261019)
