"""Per-Gaussian rotated SH view directions (sh_rotations), CPU tier: the host restatement sh.points_rgb against the
reference's own colours (tests/golden/sh_rotations.npz, tools/make_golden_sh_rotations.py), the new generations of the
argument structs and the argument rules of every layer -- all before any HIP call."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from frosting_amd import _lib, fused, sh
from frosting_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, _C

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLD, "sh_rotations.npz"))


def test_fixture_is_what_the_tool_promises(fx):
    R = fx["sh_rotations"].astype(np.float64)
    assert fx["positions"].shape == (512, 3) and fx["shs"].shape == (512, 16, 3) and R.shape == (512, 3, 3)
    assert len(str(fx["reference_sha256"])) == 64 and int(fx["seed"]) > 0
    ortho = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2))
    assert (ortho[:448] < 1e-6).all() and (ortho[448:] > 1e-3).all()      # 448 rotations, 64 general matrices
    for deg in range(4):
        clamped = (fx[f"rgb_deg{deg}"] == 0).mean()
        assert 0.05 <= clamped <= 0.95


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_points_rgb_with_rotations_matches_the_reference(fx, deg):
    """float64 restatement against the reference's float32 colours: the same clamp pattern, values within float32
    rounding (colours are O(1): 1e-6 absolute)."""
    t = {k: torch.from_numpy(fx[k]).double() for k in ("positions", "campos", "shs", "sh_rotations")}
    k = (deg + 1) ** 2
    col = sh.points_rgb(t["positions"], t["shs"][:, :k], t["campos"], deg, sh_rotations=t["sh_rotations"]).numpy()
    ref = fx[f"rgb_deg{deg}"]
    assert np.array_equal(col == 0, ref == 0)
    assert np.abs(col - ref).max() <= 1e-6
    if deg > 0:      # (the fixture can tell: without the matrices the colours are others)
        plain = sh.points_rgb(t["positions"], t["shs"][:, :k], t["campos"], deg).numpy()
        assert np.abs(plain - ref).max() > 1e-2


def test_points_rgb_without_rotations_is_unchanged(fx):
    t = {k: torch.from_numpy(fx[k]).double() for k in ("positions", "campos", "shs")}
    d = t["positions"] - t["campos"].reshape(1, 3)
    d = d / d.norm(dim=-1, keepdim=True)
    want = (sh.eval_sh(3, t["shs"].transpose(-1, -2), d) + 0.5).clamp_min(0.0)
    assert torch.equal(sh.points_rgb(t["positions"], t["shs"], t["campos"], 3), want)
    assert torch.equal(sh.points_rgb(t["positions"], t["shs"], t["campos"], 3, sh_rotations=None), want)
    eye = torch.eye(3, dtype=torch.float64).repeat(512, 1, 1)
    assert torch.equal(sh.points_rgb(t["positions"], t["shs"], t["campos"], 3, sh_rotations=eye), want)


def test_struct_generations():
    """frg_forward_args has five generations, frg_backward_args six; each earlier size is still accepted, the newest ends
    with sh_rotations."""
    L = _lib.lib()
    assert _lib.ForwardArgs._fields_[-1][0] == "sh_rotations" and _lib.BackwardArgs._fields_[-1][0] == "sh_rotations"
    assert C.sizeof(_lib.ForwardArgs) == _lib.ForwardArgs.sh_rotations.offset + 8
    assert C.sizeof(_lib.BackwardArgs) == _lib.BackwardArgs.sh_rotations.offset + 8
    assert L.frg_version() == 2
    for field in ("raw_opacities", "exact_blend", "forward_only", "sh_rotations"):
        a = _lib.ForwardArgs()
        a.struct_size = getattr(_lib.ForwardArgs, field).offset
        assert L.frg_forward_ex(C.byref(a)) < 0 and "struct_size" not in _lib.last_error(), field
    a = _lib.ForwardArgs()
    a.struct_size = C.sizeof(_lib.ForwardArgs)
    assert L.frg_forward_ex(C.byref(a)) < 0 and "struct_size" not in _lib.last_error()
    a.struct_size = C.sizeof(_lib.ForwardArgs) + 8
    assert L.frg_forward_ex(C.byref(a)) == -1 and "struct_size" in _lib.last_error()
    b = _lib.BackwardArgs(P=0, width=8, height=8)
    for size in (C.sizeof(_lib.BackwardArgs), _lib.BackwardArgs.sh_rotations.offset, _lib.BackwardArgs.range_first.offset,
                 _lib.BackwardArgs.row_live.offset, _lib.BackwardArgs.phase.offset, _lib.BackwardArgs.exact_blend.offset):
        b.struct_size = size
        assert L.frg_backward_ex(C.byref(b)) == 0, (size, _lib.last_error())
    b.struct_size = C.sizeof(_lib.BackwardArgs) + 8
    assert L.frg_backward_ex(C.byref(b)) == -1 and "struct_size" in _lib.last_error()


# a pointer that is never followed: every call below is refused by the argument checks, which look at NULL-ness only
FAKE = 4096


def _forward_fields():
    cb = _lib.ALLOC_FN(lambda user, nbytes: 0)
    return dict(geometry_alloc=cb, binning_alloc=cb, image_alloc=cb, P=8, D=3, M=16, background=FAKE, width=16, height=16,
                means3D=FAKE, opacities=FAKE, scales=FAKE, rotations=FAKE, scale_modifier=1.0, viewmatrix=FAKE, projmatrix=FAKE,
                cam_pos=FAKE, tan_fovx=0.5, tan_fovy=0.5, out_color=FAKE, radii=FAKE)


def test_forward_refuses_rotations_without_shs_before_any_hip_call():
    L = _lib.lib()
    a = _lib.ForwardArgs(struct_size=C.sizeof(_lib.ForwardArgs), colors_precomp=FAKE, sh_rotations=FAKE, **_forward_fields())
    assert L.frg_forward_ex(C.byref(a)) == -1 and "sh_rotations" in _lib.last_error()
    a = _lib.ForwardArgs(struct_size=C.sizeof(_lib.ForwardArgs), shs=FAKE, colors_precomp=FAKE, sh_rotations=FAKE, **_forward_fields())
    assert L.frg_forward_ex(C.byref(a)) == -1 and "sh_rotations" in _lib.last_error()
    a = _lib.ForwardArgs(struct_size=C.sizeof(_lib.ForwardArgs), sh_rotations=FAKE, **_forward_fields())      # neither colour input
    assert L.frg_forward_ex(C.byref(a)) == -1 and "sh_rotations" in _lib.last_error()
    # a caller of the fourth generation cannot state the field: its bytes are not read
    a = _lib.ForwardArgs(struct_size=_lib.ForwardArgs.sh_rotations.offset, colors_precomp=FAKE, shs=FAKE, sh_rotations=FAKE, **_forward_fields())
    assert L.frg_forward_ex(C.byref(a)) == -1 and "exactly one of shs / colors_precomp" in _lib.last_error()


def test_backward_refuses_rotations_without_shs_before_any_hip_call():
    L = _lib.lib()
    base = dict(P=8, D=3, M=16, R=10, background=FAKE, width=16, height=16, means3D=FAKE, scales=FAKE, rotations=FAKE,
                scale_modifier=1.0, viewmatrix=FAKE, projmatrix=FAKE, campos=FAKE, tan_fovx=0.5, tan_fovy=0.5, radii=FAKE,
                geom_buffer=FAKE, binning_buffer=FAKE, image_buffer=FAKE, dL_dpix=FAKE, dL_dmean2D=FAKE, dL_dopacity=FAKE,
                dL_dcolor=FAKE, dL_dmean3D=FAKE, dL_dcov3D=FAKE, dL_dscale=FAKE, dL_drot=FAKE)
    b = _lib.BackwardArgs(struct_size=C.sizeof(_lib.BackwardArgs), colors_precomp=FAKE, sh_rotations=FAKE, **base)
    assert L.frg_backward_ex(C.byref(b)) == -1 and "sh_rotations" in _lib.last_error()
    # the factor form of the SH gradient (dL_dsh == NULL) belongs to the view-parallel exchange, which does not carry rotations
    b = _lib.BackwardArgs(struct_size=C.sizeof(_lib.BackwardArgs), shs=FAKE, sh_rotations=FAKE, **base)
    assert L.frg_backward_ex(C.byref(b)) == -1 and "sh_rotations" in _lib.last_error() and "single-view" in _lib.last_error()


def _settings():
    return GaussianRasterizationSettings(image_height=8, image_width=8, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3),
                                         scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=3,
                                         campos=torch.zeros(3), prefiltered=False, debug=False)


def test_python_api_argument_rules():
    import inspect

    import diff_gaussian_rasterization as d
    m = torch.zeros(4, 3)
    common = dict(means3D=m, means2D=m, opacities=torch.ones(4, 1), scales=torch.ones(4, 3), rotations=torch.ones(4, 4))
    for cls in (GaussianRasterizer, d.GaussianRasterizer):
        assert "sh_rotations" in inspect.signature(cls.forward).parameters
        r = cls(raster_settings=_settings())
        with pytest.raises(Exception, match="sh_rotations only together with SHs"):
            r(colors_precomp=torch.zeros(4, 3), sh_rotations=torch.eye(3).repeat(4, 1, 1), **common)
        with pytest.raises(Exception, match="SHs or precomputed colors"):
            r(sh_rotations=torch.eye(3).repeat(4, 1, 1), **common)
        # shape, dtype and device are checked by the Python layer before the native call (no GPU here: the tensors are on the CPU,
        # like means3D, so the shape rule is the one that speaks)
        with pytest.raises(RuntimeError, match=r"sh_rotations must be a float32 tensor of shape \(num_points, 3, 3\)"):
            r(shs=torch.zeros(4, 16, 3), sh_rotations=torch.eye(3).repeat(5, 1, 1), **common)
        with pytest.raises(RuntimeError, match=r"sh_rotations must be a float32 tensor of shape \(num_points, 3, 3\)"):
            r(shs=torch.zeros(4, 16, 3), sh_rotations=torch.eye(3, dtype=torch.float64).repeat(4, 1, 1), **common)
    for mod in (_C, d._C):
        assert hasattr(mod, "rasterize_gaussians_rot") and hasattr(mod, "rasterize_gaussians_backward_rot")
    for fn in (d.rasterize_gaussians, fused.rasterize_raw, sh.points_rgb):
        assert "sh_rotations" in inspect.signature(fn).parameters
    # the compiled export checks the tensor itself as well
    e = torch.Tensor([])
    with pytest.raises(RuntimeError, match="no CPU path"):
        d._C.rasterize_gaussians_rot(e, torch.zeros(4, 3), e, e, e, e, 1.0, e, e, e, 1.0, 1.0, 8, 8, e, 0, e, False, False, e, -1, False, e)
