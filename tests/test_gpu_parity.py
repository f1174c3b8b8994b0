"""GPU parity tests (pytest -m gpu): the HIP path, called through the C ABI, against
  * the committed golden fixtures produced by the reference itself,
  * the C oracle on the same seeded inputs,
  * the reference's own rasterizer (oracle/_ref) when its .so travelled with the snapshot,
and size-independent properties at BASELINE.json's full sizes.

Bars: integer / index artefacts (radii, tile counts, sort keys, point list, ranges)
bit-exact; images <= 1e-4 mean per-pixel L1 (north_star) -- in EXACT blend mode they
are in fact bit-identical to the reference built with the same contraction mode;
gradients within the reference's own atomic-order noise.
"""
import glob
import os

import numpy as np
import pytest
import torch

from frosting_amd import _lib, scenes
from frosting_amd.introspect import State
from frosting_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, _C
from oracle import gs_oracle as G
from oracle import ref_rasterizer as REF

import helpers as Hh

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RASTER_FIXTURES = sorted(glob.glob(os.path.join(GOLD, "g_*.npz")))
L1_BAR = 1e-4  # north_star: per-pixel L1 vs the reference rasterizer


def _bwd_args(args, out, gpix):
    R, color, radii, geom, binning, img = out
    return (args[0], args[1], radii, args[2], args[4], args[5], args[6], args[7], args[8], args[9], args[10], args[11],
            gpix, args[14], args[15], args[16], geom, R, binning, img, False)


GRAD_NAMES = Hh.GRAD_NAMES


@pytest.fixture(autouse=True)
def _reset_options():
    yield
    _lib.set_option("bwd_waves", 0)
    _lib.set_option("bwd_seg_log", 0)
    _lib.set_option("fwd_order", 1)
    _lib.set_option("fwd_unroll8", 1)
    _lib.set_option("fused_small", 1)
    _lib.set_option("counter_mailbox", 1)
    _lib.set_option("sparse_sh", 1)
    _lib.set_option("sh_dir_in_backward", 0)
    _lib.set_option("async_sh", 0)
    _lib.set_option("exact_blend", 0)
    _lib.set_option("profile", 0)
    _lib.set_option("tight_binning", 0)
    _lib.set_option("global_bins", 0)


@pytest.fixture(params=["ctypes", "ext"])
def ops(request):
    """Both host bindings of the C ABI: ctypes (frosting_amd.rasterizer._C) and the compiled torch
    extension (diff_gaussian_rasterization._C)."""
    return Hh.native_ops(request.param)


def test_native_library_is_loaded(gpu_device):
    L = _lib.lib()
    assert L.frg_version() == 2
    with open("/proc/self/maps") as f:
        assert "libfrosting_rasterizer.so" in f.read()


@pytest.mark.parametrize("exact", [1, 0])
@pytest.mark.parametrize("path", RASTER_FIXTURES, ids=[os.path.basename(p) for p in RASTER_FIXTURES])
def test_against_reference_golden_fixture(gpu_device, path, exact, ops):
    fx = Hh.load_fixture(path)
    scene, cam, bg = scenes.config_scene(str(fx["cfg"]), int(fx["view"]), P=int(fx["P"]))
    _lib.set_option("exact_blend", exact)
    out, args = Hh.run_ours_native(scene, cam, bg, gpu_device, str(fx["mode"]), str(fx["cov"]), ops=ops)
    R, color, radii, geom, binning, img = out
    st = State(scene.P, cam.image_width, cam.image_height, R, geom, binning, img)
    vis = fx["radii"] > 0
    assert R == int(fx["num_rendered"])
    np.testing.assert_array_equal(radii.cpu().numpy(), fx["radii"])
    np.testing.assert_array_equal(st.tiles_touched.cpu().numpy(), fx["tiles_touched"])
    np.testing.assert_array_equal(st.ranges.cpu().numpy(), fx["ranges"])
    np.testing.assert_array_equal(st.point_list.cpu().numpy(), fx["point_list"])
    np.testing.assert_array_equal(st.sort_keys().cpu().numpy(), fx["keys"])
    np.testing.assert_array_equal(st.depths.cpu().numpy()[vis], fx["depths"][vis])
    np.testing.assert_array_equal(st.means2D.cpu().numpy()[vis], fx["means2D"][vis])
    np.testing.assert_array_equal(st.conic_opacity.cpu().numpy()[vis], fx["conic_opacity"][vis])
    image = color.cpu().numpy()
    if exact:
        np.testing.assert_array_equal(image, fx["image"])                       # bit-identical
        np.testing.assert_array_equal(st.n_contrib.cpu().numpy(), fx["n_contrib"].astype(np.int32))
    else:
        assert np.abs(image - fx["image"]).mean() <= L1_BAR
    gpix, _ = scenes.l1_target_grad(torch.from_numpy(fx["image"]), int(fx["loss_seed"]))
    grads = ops.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(gpu_device)))
    # ONE stored run of the reference's backward (its atomic-order noise is frozen into the fixture), judged like a live
    # one: both against the float64 gradient of the same forward state (the C oracle's, whose per-Gaussian stage is
    # bit-identical to the reference's)
    o = G.forward(**Hh.oracle_kwargs(scene, cam, bg, str(fx["mode"]), str(fx["cov"])))
    truth = Hh.truth_from_oracle_state(o, gpix.numpy())
    stored = {name: fx["grad_" + name] for name in GRAD_NAMES if fx["grad_" + name].size}
    Hh.judge_gradients(grads, [stored], truth, fast=not exact, label=os.path.basename(path), names=list(stored))


@pytest.mark.parametrize("mode,cov", [("sh", "sr"), ("colors", "sr"), ("sh", "cov"), ("colors", "cov")])
def test_against_c_oracle_all_input_modes(gpu_device, mode, cov):
    scene, cam, bg = scenes.config_scene("mini", 6, P=2500)
    _lib.set_option("exact_blend", 1)
    out, args = Hh.run_ours_native(scene, cam, bg, gpu_device, mode, cov)
    R, color, radii, geom, binning, img = out
    st = State(scene.P, cam.image_width, cam.image_height, R, geom, binning, img)
    o = G.forward(**Hh.oracle_kwargs(scene, cam, bg, mode, cov))
    assert R == o["num_rendered"]
    np.testing.assert_array_equal(radii.cpu().numpy(), o["radii"])
    np.testing.assert_array_equal(st.point_list.cpu().numpy().astype(np.uint32), o["point_list"])
    np.testing.assert_array_equal(st.sort_keys().cpu().numpy().astype(np.uint64), o["keys"])
    np.testing.assert_array_equal(st.ranges.cpu().numpy().astype(np.uint32), o["ranges"])
    assert np.abs(color.cpu().numpy() - o["out_color"]).mean() <= 1e-6
    gpix, _ = scenes.l1_target_grad(color.cpu(), 3)
    grads = _C.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(gpu_device)))
    og = G.backward(o, gpix.numpy())
    for name, g in zip(GRAD_NAMES, grads):
        if og[name].size == 0 or not np.any(og[name]):
            assert not g.cpu().numpy().any() or og[name].size == 0
    Hh.judge_gradients(grads, [og], Hh.truth_from_oracle_state(o, gpix.numpy()), fast=False, label=f"C oracle {mode}/{cov}")


@pytest.mark.parametrize("deg", [0, 1, 2])
def test_lower_sh_degrees(gpu_device, deg):
    scene, cam, bg = scenes.config_scene("mini", 2, P=1200)
    scene.sh_degree = deg
    _lib.set_option("exact_blend", 1)
    out, args = Hh.run_ours_native(scene, cam, bg, gpu_device)
    o = G.forward(**Hh.oracle_kwargs(scene, cam, bg))
    assert np.abs(out[1].cpu().numpy() - o["out_color"]).mean() <= 1e-6
    gpix, _ = scenes.l1_target_grad(out[1].cpu(), 4)
    grads = _C.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(gpu_device)))
    og = G.backward(o, gpix.numpy())
    dsh = grads[5].cpu().numpy()
    Hh.judge_gradients(grads, [og], Hh.truth_from_oracle_state(o, gpix.numpy()), fast=False, label=f"SH degree {deg}", names=["dL_dsh"])
    assert not dsh[:, (deg + 1) ** 2:, :].any()  # coefficients above the active degree get zero gradient


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_sh_colour_kernel_on_the_side_stream_changes_nothing(gpu_device, mode):
    """Option async_sh: the SH colours (and d colour / d direction for the backward) come from sh_color_kernel on a side
    stream instead of the preprocess.  Same arithmetic, same order: every output and gradient bit-identical."""
    scene, cam, bg = scenes.config_scene("c2", 3, P=60_000)
    out_a, args = Hh.run_ours_native(scene, cam, bg, gpu_device)
    gpix, _ = scenes.l1_target_grad(out_a[1].cpu(), 8)
    g_a = _C.rasterize_gaussians_backward(*_bwd_args(args, out_a, gpix.to(gpu_device)))
    _lib.set_option("async_sh", mode)
    try:
        out_b, args_b = Hh.run_ours_native(scene, cam, bg, gpu_device)
        g_b = _C.rasterize_gaussians_backward(*_bwd_args(args_b, out_b, gpix.to(gpu_device)))
    finally:
        _lib.set_option("async_sh", 0)
    assert out_a[0] == out_b[0] and torch.equal(out_a[1], out_b[1]) and torch.equal(out_a[2], out_b[2])
    assert all(torch.equal(a, b) for a, b in zip(g_a, g_b))


@pytest.mark.parametrize("deg", [0, 1, 2])
def test_truncated_sh_storage(gpu_device, deg):
    """A model that stores only (deg + 1)^2 coefficients per channel (M != 16): the per-coefficient SH path of the
    forward, which also leaves d colour / d direction for the backward, against the C oracle -- image, dL_dsh and the
    view-direction term inside dL_dmeans3D."""
    scene, cam, bg = scenes.config_scene("mini", 1, P=1500)
    M = (deg + 1) ** 2
    scene = scenes.Scene(scene.means3D, scene.scales, scene.rotations, scene.opacities, scene.shs[:, :M, :].contiguous(), deg)
    _lib.set_option("exact_blend", 1)
    try:
        out, args = Hh.run_ours_native(scene, cam, bg, gpu_device)
        o = G.forward(**Hh.oracle_kwargs(scene, cam, bg))
        assert out[0] == o["num_rendered"]
        assert np.abs(out[1].cpu().numpy() - o["out_color"]).mean() <= 1e-6
        gpix, _ = scenes.l1_target_grad(out[1].cpu(), 6)
        grads = _C.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(gpu_device)))
        og = G.backward(o, gpix.numpy())
        Hh.judge_gradients(grads, [og], Hh.truth_from_oracle_state(o, gpix.numpy()), fast=False, label=f"M = {M}",
                           names=["dL_dsh", "dL_dmeans3D", "dL_dopacity", "dL_dscales"])
    finally:
        _lib.set_option("exact_blend", 0)


_TRUTH_CACHE = {}


def _check_against_reference_rasterizer(gpu_device, scene, cam, bg, ops, label, scale_modifier=1.0, colors=None, campos_2d=False):
    """Ours beside the reference's own code (oracle/_ref, hipcc -ffp-contract=off) on the same tensors: every forward
    artefact bit-identical in EXACT mode; the eight gradients, in EXACT and in the default arithmetic, judged beside four
    runs of the reference's backward against the float64 gradient of that forward state (helpers.judge_gradients: the
    1e-4 gate, no per-scene factors).  Returns (tile list lengths, slots per 64-Gaussian wave).
    scale_modifier / colors (a [P,3] feature tensor as colors_precomp) / campos_2d ([1,3] camera centre): the call-site
    variations of helpers.run_ours_native."""
    P = scene.P
    ours_kw = dict(ops=ops, scale_modifier=scale_modifier, colors=colors, campos_2d=campos_2d)
    _lib.set_option("exact_blend", 1)
    out, args = Hh.run_ours_native(scene, cam, bg, gpu_device, **ours_kw)
    R, color, radii, geom, binning, img = out
    st = State(P, cam.image_width, cam.image_height, R, geom, binning, img)
    Rr, rcolor, rradii, rst = REF.forward(**Hh.oracle_kwargs(scene, cam, bg, as_numpy=False, device=gpu_device,
                                                             scale_modifier=scale_modifier, colors=colors))
    assert R == Rr
    assert torch.equal(radii, rradii)
    assert torch.equal(st.tiles_touched, rst.tiles_touched)
    assert torch.equal(st.point_offsets, rst.point_offsets)
    assert torch.equal(st.ranges, rst.ranges)
    assert torch.equal(st.point_list, rst.point_list)
    assert torch.equal(st.sort_keys(), rst.point_list_keys)
    vis = radii > 0
    assert torch.equal(st.depths[vis], rst.depths[vis]) and torch.equal(st.means2D[vis], rst.means2D[vis])
    assert torch.equal(st.conic_opacity[vis], rst.conic_opacity[vis])
    assert torch.equal(st.n_contrib, rst.n_contrib)
    assert torch.equal(st.final_T, rst.final_T)
    assert torch.equal(color, rcolor)
    list_len = (st.ranges[:, 1] - st.ranges[:, 0]).cpu()
    slots_per_wave = st.tiles_touched[: (P // 64) * 64].view(-1, 64).sum(1).cpu()
    del st
    gpix, _ = scenes.l1_target_grad(color.cpu(), 9)
    gpix = gpix.to(gpu_device)
    runs = Hh.reference_runs(lambda: REF.backward(rst, gpix))
    # (the float64 pass over a 3 M-Gaussian frame takes most of a minute of host time: one per scene, whatever the binding)
    key = (label, P, R, cam.image_width, cam.image_height, float(scale_modifier))
    if key not in _TRUTH_CACHE:
        _TRUTH_CACHE.clear()
        _TRUTH_CACHE[key] = Hh.truth_from_ref_state(rst, gpix)
    truth = _TRUTH_CACHE[key]

    def check(grads, fast, mode):
        Hh.judge_gradients(grads, runs, truth, fast, label)

    # EXACT arithmetic (the reference's operation order): backward on the bit-identical forward state
    check(ops.rasterize_gaussians_backward(*_bwd_args(args, out, gpix)), False, "exact")
    _lib.set_option("exact_blend", 0)  # default product arithmetic: tolerance bars
    out2, _ = Hh.run_ours_native(scene, cam, bg, gpu_device, **ours_kw)
    assert float((out2[1] - rcolor).abs().mean()) <= L1_BAR
    assert torch.equal(out2[2], rradii)
    check(ops.rasterize_gaussians_backward(*_bwd_args(args, out2, gpix)), True, "fast")
    return list_len, slots_per_wave


@pytest.mark.skipif(not REF.available("exact"), reason="oracle/_ref not built")
@pytest.mark.parametrize("case", ["scale_modifier=0.5", "scale_modifier=2.0", "principal=+0.1,-0.1", "principal=-0.1,+0.07",
                                  "depth_features_bg=-1", "campos=[1,3]"])
def test_call_site_variations_vs_reference_rasterizer(gpu_device, case):
    """What the reference's call sites vary and the uniform-scene tests above do not (missing 2), each at
    150 000 Gaussians on 800x800 against the reference's own code -- every forward artefact bit-identical in EXACT mode,
    gradients within the usual bars in both arithmetics:
      * scale_modifier != 1 (gaussian_renderer/__init__.py:18,42,63 -> computeCov3D's `mod`, forward.cu:118-128, and
        its backward, backward.cu:289-291);
      * the off-centre principal point Frosting patches into the projection (frosting_model.py:1440-1442);
      * a non-colour feature as colors_precomp: view depth (values ~1 - 8) composited over bg = -1, forward + backward
        (frosting_model.py:1800-1811, sugar_model.py:2364-2375);
      * campos as the [1,3] tensor p3d_camera.get_camera_center() returns (frosting_model.py:1447,1462)."""
    P = 150_000
    scene, cam, bg = scenes.config_scene("c2", 5, P=P)
    kw = {}
    if case.startswith("scale_modifier"):
        kw["scale_modifier"] = float(case.split("=")[1])
    elif case.startswith("principal"):
        cx, cy = (float(v) for v in case.split("=")[1].split(","))
        cfg = scenes.CONFIGS["c2"]
        cam = scenes.ring_camera(5, cfg["width"], cfg["height"], cfg["fx"], cfg["fy"], principal=(cx, cy))
    elif case.startswith("depth_features"):
        ph = torch.cat([scene.means3D, torch.ones(P, 1)], 1) @ cam.viewmatrix        # view-space z, as point_depth is
        kw["colors"] = ph[:, 2:3].expand(-1, 3).contiguous()
        assert float(kw["colors"].min()) > 0.9 and float(kw["colors"].max()) < 8.0
        bg = torch.tensor([-1.0, -1.0, -1.0])
    else:
        kw["campos_2d"] = True
    ops = Hh.native_ops("ext" if case[0] in "sd" else "ctypes")
    _check_against_reference_rasterizer(gpu_device, scene, cam, bg, ops, case, **kw)


@pytest.mark.skipif(not REF.available("exact"), reason="oracle/_ref not built")
@pytest.mark.parametrize("cfg,P,view,binding", [("c2", 100_000, 0, "ext"), ("c3", 400_000, 2, "ctypes"),
                                                ("c3", 3_000_000, 0, "ext")])
def test_bit_exact_vs_reference_rasterizer(gpu_device, cfg, P, view, binding):
    """The reference's own code (hipcc, -ffp-contract=off) run beside ours on the same tensors, at the FULL
    sizes of BASELINE.json's configs[1] (C2) and configs[2] (C3: 3 M Gaussians, 1600x1056, 16.4 M instances)."""
    scene, cam, bg = scenes.config_scene(cfg, view, P=P)
    _check_against_reference_rasterizer(gpu_device, scene, cam, bg, Hh.native_ops(binding), f"{cfg} P={P}")


@pytest.mark.skipif(not REF.available("exact"), reason="oracle/_ref not built")
@pytest.mark.parametrize("frame", ["c3:50000", "c3:150000", "c3:400000", "c2-scene-on-the-c3-image:100000"])
def test_sparse_frames_default_modes_vs_reference(gpu_device, frame):
    """Sparse frames on the large image: 50 k - 400 k Gaussians on 1600x1056 light every one of the
    6600 tiles with short lists -- the state of a scene early in training (3DGS starts from ~1e5 SfM points) -- and get
    the tile-per-wave backward in the default arithmetic.  Default options (fast arithmetic, automatic form), through
    the compiled extension, beside the reference's own code: forward artefacts bit-identical in EXACT mode; all eight
    gradients at the 1e-4 gate, no per-scene factor (helpers.judge_gradients).  What round 3's kernel did here -- pixel
    moments about the tile centre, shifted per instance -- is gone: the moments are the reference's, about the Gaussian
    (blend_impl.h); measured on these frames in profiles/r04_sparse_grad_check.log."""
    name, P = frame.split(":")
    if name == "c3":
        scene, cam, bg = scenes.config_scene("c3", 2, P=int(P))
    else:
        scene, _, bg = scenes.config_scene("c2", 0, P=int(P))
        _, cam, _ = scenes.config_scene("c3", 1, P=8)
    assert _lib.get_option("bwd_waves") == 0 and _lib.get_option("tight_binning") == 0      # default options
    list_len, _ = _check_against_reference_rasterizer(gpu_device, scene, cam, bg, Hh.native_ops("ext"), frame)
    assert int((list_len > 0).sum()) > 2560


@pytest.mark.skipif(not REF.available("exact"), reason="oracle/_ref not built")
def test_skewed_scene_vs_reference_rasterizer(gpu_device):
    """The clustered scene bench.py reports as `skew_scene`, at full size (3 M Gaussians, 17.6 M instances; tile lists
    up to 293 000 entries, 139 of them beyond the LDS capacity of the tile sort; near-camera Gaussians of hundreds of
    tiles) against the reference's own code: the stable global sort of rasterizer_impl.cu:303-308 at any list length,
    backward.cu:399-557 on lists of 10^5 entries."""
    cfg = scenes.CONFIGS["c3"]
    scene = scenes.make_skew_scene(cfg["P"], cfg["seed"] + 77)
    _, cam, bg = scenes.config_scene("c3", 0, P=1000)
    list_len, _ = _check_against_reference_rasterizer(gpu_device, scene, cam, bg, Hh.native_ops("ext"), "skew 3M")
    assert int(list_len.max()) > 250_000 and int((list_len > 8192).sum()) >= 100


@pytest.mark.skipif(not REF.available("exact"), reason="oracle/_ref not built")
@pytest.mark.parametrize("binding", ["ctypes", "ext"])
def test_long_lists_and_giant_gaussians_vs_reference_rasterizer(gpu_device, binding):
    """Small image, everything that only clustered scenes reach at once: four tile lists of more than 250 000
    entries and over a hundred beyond 8192 (sorted chunks + splitters instead of the LDS sort), Gaussians covering the
    whole image (their waves' slot runs are handed to the 16-wave form of the per-Gaussian backward) -- every
    sort key, the image and all eight gradients against the reference's own code."""
    scene, cam, bg = scenes.long_list_scene()
    list_len, slots = _check_against_reference_rasterizer(gpu_device, scene, cam, bg, Hh.native_ops(binding), "long lists")
    assert int((list_len > 250_000).sum()) >= 1 and int((list_len > 8192).sum()) >= 100
    assert int((slots > 4 * 896).sum()) >= 1       # BWD_HEAVY_WINDOWS x BWD_WIN (preprocess_bwd.hip)


def test_backward_is_bit_reproducible(gpu_device):
    scene, cam, bg = scenes.config_scene("c2", 1, P=50_000)
    out, args = Hh.run_ours_native(scene, cam, bg, gpu_device)
    gpix, _ = scenes.l1_target_grad(out[1].cpu(), 5)
    b = _bwd_args(args, out, gpix.to(gpu_device))
    g1 = _C.rasterize_gaussians_backward(*b)
    g2 = _C.rasterize_gaussians_backward(*b)
    assert all(torch.equal(a, c) for a, c in zip(g1, g2))


def test_forward_is_bit_reproducible_whatever_the_scatter_order(gpu_device):
    """The cell-ordered scatter reserves one run per (workgroup share, tile) with an atomic on the tile's fill
    cursor: the order of the (depth, index) pairs inside a tile segment differs from run to run.  The sort's order is
    total, so every output must not: tile lists, image, per-pixel bookkeeping and gradients of two independent runs
    are identical bit for bit (and, in the comparisons with the reference above, identical to the reference's)."""
    scene, cam, bg = scenes.config_scene("c3", 0, P=500_000)
    runs = []
    for _ in range(3):
        out, args = Hh.run_ours_native(scene, cam, bg, gpu_device)
        st = State(scene.P, cam.image_width, cam.image_height, out[0], out[3], out[4], out[5])
        gpix, _ = scenes.l1_target_grad(out[1].cpu(), 11)
        grads = _C.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(gpu_device)))
        runs.append((out[0], out[1].clone(), out[2].clone(), st.point_list.clone(), st.ranges.clone(), st.n_contrib.clone(),
                     st.final_T.clone(), [g.clone() for g in grads]))
        del st
    for r in runs[1:]:
        assert r[0] == runs[0][0]
        assert all(torch.equal(a, b) for a, b in zip(r[1:7], runs[0][1:7]))
        assert all(torch.equal(a, b) for a, b in zip(r[7], runs[0][7]))


def test_ragged_image_and_edge_sizes(gpu_device):
    scene, _, bg = scenes.config_scene("mini", 0, P=700)
    _lib.set_option("exact_blend", 1)
    for (w, h) in [(150, 101), (17, 33), (16, 16), (1, 1)]:
        cam = scenes.ring_camera(3, w, h, 120.0, 120.0)
        out, _ = Hh.run_ours_native(scene, cam, bg, gpu_device)
        o = G.forward(**Hh.oracle_kwargs(scene, cam, bg))
        assert out[0] == o["num_rendered"]
        assert tuple(out[1].shape) == (3, h, w)
        assert np.abs(out[1].cpu().numpy() - o["out_color"]).mean() <= 1e-6
    # P == 0: zero image, background not applied (rasterize_points.cu:68,81)
    empty = scenes.Scene(*(t[:0] for t in (scene.means3D, scene.scales, scene.rotations, scene.opacities, scene.shs)), 3)
    cam = scenes.ring_camera(0, 64, 48, 60.0, 60.0)
    out, args = Hh.run_ours_native(empty, cam, torch.ones(3), gpu_device)
    assert out[0] == 0 and not out[1].any() and out[2].numel() == 0
    # P == 1 and an all-culled scene
    one = scenes.Scene(*(t[:1] for t in (scene.means3D, scene.scales, scene.rotations, scene.opacities, scene.shs)), 3)
    out, _ = Hh.run_ours_native(one, cam, bg, gpu_device)
    o = G.forward(**Hh.oracle_kwargs(one, cam, bg))
    assert out[0] == o["num_rendered"] and np.abs(out[1].cpu().numpy() - o["out_color"]).mean() <= 1e-6
    behind = scenes.Scene(scene.means3D * 0 + cam.campos - 0.0, scene.scales, scene.rotations, scene.opacities, scene.shs, 3)
    out, args = Hh.run_ours_native(behind, cam, bg, gpu_device)
    assert out[0] == 0 and not out[2].any()
    np.testing.assert_allclose(out[1].cpu().numpy(), np.broadcast_to(bg.numpy()[:, None, None], (3, 48, 64)))
    gpix = torch.ones(3, 48, 64, device=gpu_device)
    grads = _C.rasterize_gaussians_backward(*_bwd_args(args, out, gpix))
    assert all(not g.any() for g in grads)


def test_depth_ties_and_oversized_tiles(gpu_device):
    """Coplanar Gaussians (equal depth keys -> index tie-break) piled onto one tile so
    that its list exceeds the 8192-entry LDS capacity (global ping-pong sort path)."""
    P = 12_000
    g = torch.Generator().manual_seed(1)
    cam = scenes.ring_camera(0, 64, 64, 80.0, 80.0)
    means = torch.zeros(P, 3)
    means[:, :2] = 0.02 * torch.randn(P, 2, generator=g)
    means[: P // 2, 2] = 0.5        # two exact depth planes => massive ties
    means[P // 2:, 2] = 0.25
    scene = scenes.Scene(means, torch.full((P, 3), 0.01), torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1),
                         torch.full((P, 1), 0.02), 0.1 * torch.randn(P, 16, 3, generator=g), 3)
    bg = torch.zeros(3)
    _lib.set_option("exact_blend", 1)
    out, _ = Hh.run_ours_native(scene, cam, bg, gpu_device)
    R, color, radii, geom, binning, img = out
    st = State(P, 64, 64, R, geom, binning, img)
    assert int(st.tile_count.max()) > 8192
    o = G.forward(**Hh.oracle_kwargs(scene, cam, bg))
    assert R == o["num_rendered"]
    np.testing.assert_array_equal(st.point_list.cpu().numpy().astype(np.uint32), o["point_list"])
    assert np.abs(color.cpu().numpy() - o["out_color"]).mean() <= 1e-6


def test_autograd_module_api_matches_call_sites(gpu_device):
    """The call pattern of gaussian_renderer/__init__.py:36-93 and frosting_model.py:1452-1467,1649-1657."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings as S2, GaussianRasterizer as R2
    scene, cam, bg = scenes.config_scene("mini", 1, P=1500)
    sc = scene.to(gpu_device)
    means3D = sc.means3D.clone().requires_grad_(True)
    shs = sc.shs.clone().requires_grad_(True)
    opac = sc.opacities.clone().requires_grad_(True)
    scales = sc.scales.clone().requires_grad_(True)
    rots = sc.rotations.clone().requires_grad_(True)
    screenspace_points = torch.zeros_like(means3D, requires_grad=True) + 0
    screenspace_points.retain_grad()
    settings = S2(image_height=int(cam.image_height), image_width=int(cam.image_width), tanfovx=cam.tanfovx,
                  tanfovy=cam.tanfovy, bg=bg.to(gpu_device), scale_modifier=1.0, viewmatrix=cam.viewmatrix.to(gpu_device),
                  projmatrix=cam.projmatrix.to(gpu_device), sh_degree=3, campos=cam.campos.to(gpu_device),
                  prefiltered=False, debug=False)
    rasterizer = R2(raster_settings=settings)
    rendered_image, radii = rasterizer(means3D=means3D, means2D=screenspace_points, shs=shs, colors_precomp=None,
                                       opacities=opac, scales=scales, rotations=rots, cov3D_precomp=None)
    assert rendered_image.shape == (3, cam.image_height, cam.image_width) and radii.dtype == torch.int32
    target = torch.rand_like(rendered_image)
    (rendered_image - target).abs().mean().backward()
    o = G.forward(**Hh.oracle_kwargs(scene, cam, bg))
    og = G.backward(o, (torch.sign(rendered_image.detach() - target) / target.numel()).cpu().numpy())
    gpix_np = (torch.sign(rendered_image.detach() - target) / target.numel()).cpu().numpy()
    mine = {"dL_dmeans3D": means3D.grad, "dL_dsh": shs.grad, "dL_dmeans2D": screenspace_points.grad,   # (means2D: the densification statistic)
            "dL_dopacity": opac.grad, "dL_dscales": scales.grad, "dL_drotations": rots.grad}
    Hh.judge_gradients(mine, [og], Hh.truth_from_oracle_state(o, gpix_np), fast=True, label="autograd module", names=list(mine))
    assert not screenspace_points.grad[:, 2].any()
    vis = rasterizer.markVisible(sc.means3D)
    np.testing.assert_array_equal(vis.cpu().numpy(), G.mark_visible(scene.means3D.numpy(), cam.viewmatrix.numpy(),
                                                                    cam.projmatrix.numpy()))
    with torch.no_grad():  # inference call (metrics.py:332-342)
        img2, _ = rasterizer(means3D=sc.means3D, means2D=screenspace_points, shs=sc.shs, opacities=sc.opacities,
                             scales=sc.scales, rotations=sc.rotations)
    assert torch.equal(img2, rendered_image.detach())


def test_prefiltered_assertion_and_debug_mode(gpu_device):
    scene, cam, bg = scenes.config_scene("mini", 0, P=300)
    sc = scene.to(gpu_device)
    kw = dict(image_height=cam.image_height, image_width=cam.image_width, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
              bg=bg.to(gpu_device), scale_modifier=1.0, viewmatrix=cam.viewmatrix.to(gpu_device),
              projmatrix=cam.projmatrix.to(gpu_device), sh_degree=3, campos=cam.campos.to(gpu_device))
    means = sc.means3D.clone()
    means[0] = cam.campos.to(gpu_device)  # behind the near plane
    r = GaussianRasterizer(GaussianRasterizationSettings(prefiltered=True, debug=False, **kw))
    with pytest.raises(RuntimeError, match="filtered although prefiltered"):
        r(means3D=means, means2D=means, shs=sc.shs, opacities=sc.opacities, scales=sc.scales, rotations=sc.rotations)
    r = GaussianRasterizer(GaussianRasterizationSettings(prefiltered=False, debug=True, **kw))
    img, _ = r(means3D=means, means2D=means, shs=sc.shs, opacities=sc.opacities, scales=sc.scales, rotations=sc.rotations)
    assert torch.isfinite(img).all()


def test_full_size_properties_c3(gpu_device):
    """BASELINE configs[2] at full size (3M Gaussians, 1600x1056): properties that need no oracle."""
    scene, cam, bg = scenes.config_scene("c3", 0)
    out, args = Hh.run_ours_native(scene, cam, bg, gpu_device)
    R, color, radii, geom, binning, img = out
    st = State(scene.P, cam.image_width, cam.image_height, R, geom, binning, img)
    assert R == int(st.tiles_touched.to(torch.int64).sum()) == int(st.point_offsets[-1])
    counts = (st.ranges[:, 1] - st.ranges[:, 0]).to(torch.int64)
    assert int(counts.sum()) == R and torch.equal(counts, st.tile_count.to(torch.int64))
    keys = st.sort_keys()
    assert bool((keys[1:] >= keys[:-1]).all())                       # sortedness of (tile, depth)
    same = keys[1:] == keys[:-1]
    pl = st.point_list.to(torch.int64)
    assert bool((pl[1:][same] > pl[:-1][same]).all())                # ties in ascending index order
    assert int(torch.bincount(pl, minlength=scene.P).sum()) == R
    assert torch.equal(torch.bincount(pl, minlength=scene.P), st.tiles_touched.to(torch.int64))  # multiset of instances
    assert torch.isfinite(color).all() and float(color.min()) >= 0.0
    T = st.final_T
    assert float(T.min()) >= 1e-4 * 0.99 and float(T.max()) <= 1.0
    assert int((st.n_contrib.to(torch.int64).view(-1) > counts.max()).sum()) == 0
    # linearity of backward in dL/dimage (fixed forward state)
    gpix, _ = scenes.l1_target_grad(color.cpu(), 1)
    gpix = gpix.to(gpu_device)
    g1 = _C.rasterize_gaussians_backward(*_bwd_args(args, out, gpix))
    g2 = _C.rasterize_gaussians_backward(*_bwd_args(args, out, 2.0 * gpix))
    for a, b in zip(g1, g2):
        assert torch.equal(2.0 * a, b)                               # exact: scaling by 2 commutes with rounding
    assert all(torch.isfinite(g).all() for g in g1)
    assert not g1[3][radii == 0].any() and not g1[5][radii == 0].any()  # culled Gaussians get zero rows


def test_full_size_c2_forward_vs_oracle(gpu_device):
    """BASELINE configs[1] (100k Gaussians, 800x800 forward) against the C oracle."""
    scene, cam, bg = scenes.config_scene("c2", 0)
    _lib.set_option("exact_blend", 0)
    out, _ = Hh.run_ours_native(scene, cam, bg, gpu_device)
    o = G.forward(**Hh.oracle_kwargs(scene, cam, bg))
    assert out[0] == o["num_rendered"]
    np.testing.assert_array_equal(out[2].cpu().numpy(), o["radii"])
    assert np.abs(out[1].cpu().numpy() - o["out_color"]).mean() <= L1_BAR


def test_large_image_binning_path(gpu_device):
    """Images with more tiles than fit the LDS histograms use global-atomic binning;
    force that path on a small image and require identical artefacts."""
    scene, cam, bg = scenes.config_scene("mini", 2, P=2500)
    _lib.set_option("exact_blend", 1)
    out_a, _ = Hh.run_ours_native(scene, cam, bg, gpu_device)
    st_a = State(scene.P, cam.image_width, cam.image_height, out_a[0], out_a[3], out_a[4], out_a[5])
    keys_a, pl_a, img_a = st_a.sort_keys().clone(), st_a.point_list.clone(), out_a[1].clone()
    _lib.set_option("global_bins", 1)
    try:
        out_b, _ = Hh.run_ours_native(scene, cam, bg, gpu_device)
        st_b = State(scene.P, cam.image_width, cam.image_height, out_b[0], out_b[3], out_b[4], out_b[5])
        assert out_a[0] == out_b[0]
        assert torch.equal(keys_a, st_b.sort_keys()) and torch.equal(pl_a, st_b.point_list)
        assert torch.equal(img_a, out_b[1])
    finally:
        _lib.set_option("global_bins", 0)


@pytest.mark.parametrize("cfg,P,exact,global_bins", [("mini", 3000, 1, 0), ("mini", 3000, 0, 0), ("c2", 60000, 0, 0),
                                                      ("mini", 2500, 0, 1)])
def test_tight_binning_is_invisible_in_every_output(gpu_device, cfg, P, exact, global_bins):
    """Option "tight_binning": (Gaussian, tile) instances that provably cannot reach alpha >= 1/255
    anywhere in the tile are dropped when the lists are built instead of when they are walked.
    num_rendered, radii and the image stay bit-identical; the tile lists become order-preserving sub-lists of the
    reference's.  Gradients: bit-identical while no tile's walk crosses a segment boundary of the backward blend (a
    boundary is a LIST POSITION, and the sub-lists put it at another Gaussian: the state restarted from there is another
    rounding of the same value) -- so with segments of 1024 entries on these frames; with the segments the forward
    chooses by itself (256 entries) the two gradients agree to float32 rounding."""
    scene, cam, bg = scenes.config_scene(cfg, 3, P=P)
    for seg_log in (10, 0):
        _lib.set_option("bwd_seg_log", seg_log)
        _lib.set_option("exact_blend", exact)
        _lib.set_option("global_bins", global_bins)          # also the large-image (global-atomic) binning path
        out_a, args = Hh.run_ours_native(scene, cam, bg, gpu_device)
        st_a = State(scene.P, cam.image_width, cam.image_height, out_a[0], out_a[3], out_a[4], out_a[5])
        ranges_a, pl_a = st_a.ranges.cpu().numpy().copy(), st_a.point_list.cpu().numpy().copy()
        longest = int((ranges_a[:, 1] - ranges_a[:, 0]).max())
        gpix, _ = scenes.l1_target_grad(out_a[1].cpu(), 17)
        gpix = gpix.to(gpu_device)
        g_a = [t.clone() for t in _C.rasterize_gaussians_backward(*_bwd_args(args, out_a, gpix))]
        img_a, radii_a = out_a[1].clone(), out_a[2].clone()
        _lib.set_option("tight_binning", 1)
        try:
            out_b, args_b = Hh.run_ours_native(scene, cam, bg, gpu_device)
            assert out_b[0] == out_a[0]                                  # num_rendered stays the reference's count
            assert torch.equal(out_b[1], img_a) and torch.equal(out_b[2], radii_a)
            st_b = State(scene.P, cam.image_width, cam.image_height, out_b[0], out_b[3], out_b[4], out_b[5])
            ranges_b, pl_b = st_b.ranges.cpu().numpy(), st_b.point_list.cpu().numpy()
            kept = int((ranges_b[:, 1] - ranges_b[:, 0]).sum())
            assert 0 < kept < out_a[0]
            for t in np.random.default_rng(0).choice(len(ranges_a), size=min(200, len(ranges_a)), replace=False):
                a = pl_a[ranges_a[t, 0]:ranges_a[t, 1]]
                b = pl_b[ranges_b[t, 0]:ranges_b[t, 1]]
                # b is a sub-list of a in the same order
                pos = {int(v): i for i, v in enumerate(a)}
                idx = [pos[int(v)] for v in b]
                assert idx == sorted(idx) and len(set(idx)) == len(idx)
            g_b = _C.rasterize_gaussians_backward(*_bwd_args(args_b, out_b, gpix))
            if longest <= (1 << (seg_log or 8)):            # no walk crosses a boundary: the same additions in the same order
                for ga, gb in zip(g_a, g_b):
                    assert torch.equal(ga, gb)
            else:
                assert seg_log == 0, (longest, "the frames of this test are meant to fit one 1024-entry segment")
                # (two roundings of the same value: 1e-6 on the well-conditioned tensors; the covariance chain amplifies them on
                # edge-on needles as it does the reference's own run-to-run noise, helpers.py)
                for name, ga, gb in zip(GRAD_NAMES, g_a, g_b):
                    bar = 1e-3 if name in ("dL_dcov3D", "dL_dscales", "dL_drotations") else 1e-5
                    assert Hh.rel_l2(gb, ga) <= bar, (name, Hh.rel_l2(gb, ga))
        finally:
            _lib.set_option("tight_binning", 0)
            _lib.set_option("exact_blend", 0)
            _lib.set_option("global_bins", 0)
            _lib.set_option("bwd_seg_log", 0)


@pytest.mark.parametrize("P,spread,planes", [(500, 0.5, 0), (3000, 0.3, 0), (9000, 0.15, 0), (30000, 0.08, 0),
                                             (40000, 0.05, 3), (150_000, 0.05, 0), (150_000, 0.05, 3), (400_000, 0.02, 2),
                                             (600_000, 0.004, 0), (600_000, 0.004, 2)])
def test_tile_sort_every_size_class(gpu_device, P, spread, planes):
    """Tile lists around every size class of the sort -- LDS (1 / 4 / 8 waves), sorted chunks + splitters
    (8193 .. 524 288 entries), global LSD passes (beyond; the 600 000 Gaussians of the last two cases sit on one
    tile corner) -- with and without massive depth ties: the output must be ordered by (tile, depth bits, index)."""
    g = torch.Generator().manual_seed(P)
    cam = scenes.ring_camera(0, 128, 96, 100.0, 100.0)
    means = torch.zeros(P, 3)
    means[:, :2] = spread * torch.randn(P, 2, generator=g)
    means[:, 2] = 0.5 * torch.rand(P, generator=g)
    if planes:
        means[:, 2] = torch.randint(0, planes, (P,), generator=g).float() * 0.1
    scene = scenes.Scene(means, torch.full((P, 3), 0.01), torch.tensor([[1.0, 0, 0, 0]]).repeat(P, 1),
                         torch.full((P, 1), 0.02), 0.1 * torch.randn(P, 16, 3, generator=g), 3)
    out, _ = Hh.run_ours_native(scene, cam, torch.zeros(3), gpu_device)
    R, color, radii, geom, binning, img = out
    st = State(P, 128, 96, R, geom, binning, img)
    keys = st.sort_keys().cpu().numpy()
    pl = st.point_list.cpu().numpy().astype(np.int64)
    longest = int((st.ranges[:, 1] - st.ranges[:, 0]).max())
    assert (longest > 8192) == (P >= 30000) and (longest > 524288) == (P >= 600_000), longest
    assert np.array_equal(np.lexsort((pl, keys)), np.arange(R))
    assert np.array_equal(np.bincount(pl, minlength=P), st.tiles_touched.cpu().numpy())


def test_backward_follows_the_forwards_modes_not_the_process_options(gpu_device):
    """The backward takes the binning mode from what the forward stamped into its image chunk: flipping
    tight_binning / global_bins / between a forward and its backward (two rasterizers in one process, a
    bench pass in another mode) must not change a single gradient bit."""
    scene, cam, bg = scenes.config_scene("c2", 4, P=40_000)
    want = {}
    for tight in (0, 1):
        _lib.set_option("tight_binning", tight)
        out, args = Hh.run_ours_native(scene, cam, bg, gpu_device)
        gpix, _ = scenes.l1_target_grad(out[1].cpu(), 23)
        b = _bwd_args(args, out, gpix.to(gpu_device))
        want[tight] = [g.clone() for g in _C.rasterize_gaussians_backward(*b)]
        for t2, gb in ((1 - tight, 0), (1 - tight, 1), (tight, 1)):
            _lib.set_option("tight_binning", t2)            # options changed AFTER the forward
            _lib.set_option("global_bins", gb)
            got = _C.rasterize_gaussians_backward(*b)
            assert all(torch.equal(a, c) for a, c in zip(want[tight], got)), (tight, t2, gb)
        _lib.set_option("global_bins", 0)
    for a, c in zip(want[0], want[1]):                       # and the two modes agree with each other
        assert torch.equal(a, c)


@pytest.mark.skipif(not REF.available("exact"), reason="oracle/_ref not built")
@pytest.mark.parametrize("exact", [1, 0])
def test_backward_blend_work_items_whatever_the_grid(gpu_device, exact):
    """The backward blend's work items (tile, segment) -- listed by the forward blend as its tiles finish, in whatever order
    that happens -- are dealt to the backward's waves statically (blend_impl.h, BwdShares):
    whatever the number of waves (option bwd_waves: fewer than items -> the waves stride, more -> most find nothing), every
    slot is written once with the same value -- gradients identical bit for bit -- on a sparse 60 k-Gaussian frame and on a
    frame that covers one corner of the image (all its items belong to the tiles of one or two XCD bands: most waves take
    theirs from the pool that evens the XCDs' shares).  Both frames against the reference's own code."""
    scene, cam, bg = scenes.config_scene("c2", 3, P=60_000)
    small = scenes.Scene(scene.means3D * 0.12 + torch.tensor([0.9, 0.6, 0.0]), scene.scales, scene.rotations, scene.opacities,
                         scene.shs, scene.sh_degree)
    for label, sc in (("60 k frame", scene), ("corner frame", small)):
        _lib.set_option("exact_blend", exact)
        out, args = Hh.run_ours_native(sc, cam, bg, gpu_device)
        if sc is small:
            st = State(small.P, cam.image_width, cam.image_height, out[0], out[3], out[4], out[5])
            assert 0 < int((st.tile_count > 0).sum()) < 1000
        gpix, _ = scenes.l1_target_grad(out[1].cpu(), 29)
        b = _bwd_args(args, out, gpix.to(gpu_device))
        want = [g.clone() for g in _C.rasterize_gaussians_backward(*b)]
        for waves in (8, 64, 1000, 4096, 30_000):
            _lib.set_option("bwd_waves", waves)
            got = _C.rasterize_gaussians_backward(*b)
            assert all(torch.equal(x, y) for x, y in zip(want, got)), (label, waves)
        _lib.set_option("bwd_waves", 0)
        _check_against_reference_rasterizer(gpu_device, sc, cam, bg, _C, label)


@pytest.mark.skipif(not REF.available("exact"), reason="oracle/_ref not built")
@pytest.mark.parametrize("binding,seg_log", [("ext", 0), ("ext", 9), ("ctypes", 10)])
def test_deep_walks_cross_many_segments_of_the_backward_blend(gpu_device, binding, seg_log):
    """The backward blend walks a tile's processed prefix in segments of 256 / 512 entries (by frame), each an independent
    work item that starts from the state the FORWARD left at the segment's end (transmittance and accumulated colour per
    pixel: BinningState::ckpt, ImageState::final_C).  A translucent scene on a small image -- opacities 0.004 ... 0.03, so
    no pixel saturates and every tile walks its whole list of several thousand entries: 8 - 16 segments per tile, every
    pixel continuing behind every boundary -- against the reference's own code: forward artefacts bit-identical, all
    eight gradients judged as everywhere; and bit-reproducible from run to run (the items are pulled by whichever wave
    is free: the order of the work must not reach the sums).  seg_log: the segment length the forward chooses by itself
    (0: 256 entries on a frame of this size) and the two longer ones, pinned -- 6 - 28 segments per tile."""
    _lib.set_option("bwd_seg_log", seg_log)
    scene, _, bg = scenes.config_scene("c2", 0, P=600_000)
    scene = scenes.Scene(scene.means3D, scene.scales * 3.0, scene.rotations, (0.004 + 0.026 * scene.opacities).contiguous(), scene.shs, 3)
    cam = scenes.ring_camera(1, 160, 128, 222.0, 222.0)
    list_len, _ = _check_against_reference_rasterizer(gpu_device, scene, cam, bg, Hh.native_ops(binding), "deep walks")
    out, args = Hh.run_ours_native(scene, cam, bg, gpu_device)
    st = State(scene.P, cam.image_width, cam.image_height, out[0], out[3], out[4], out[5])
    walked = st.n_contrib.view(8, 16, 10, 16).amax(dim=(1, 3)).flatten()          # per tile: the last contributor of its last pixel
    assert int((walked > 4 * 1024).sum()) >= 20 and int(walked.max()) > 6 * 1024, (int(walked.max()), int((walked > 4096).sum()))
    gpix, _ = scenes.l1_target_grad(out[1].cpu(), 77)
    b = _bwd_args(args, out, gpix.to(gpu_device))
    g1 = [g.clone() for g in _C.rasterize_gaussians_backward(*b)]
    for _ in range(3):
        assert all(torch.equal(x, y) for x, y in zip(g1, _C.rasterize_gaussians_backward(*b)))
    # a backward follows the segment length its FORWARD stamped, whatever the option says by then
    _lib.set_option("bwd_seg_log", 9 if seg_log != 9 else 8)
    assert all(torch.equal(x, y) for x, y in zip(g1, _C.rasterize_gaussians_backward(*b)))


def test_backward_finds_the_forwards_checkpoints_whatever_r_it_is_called_with(gpu_device):
    """the forward blend's checkpoints sit behind point_list and pairs of the binning chunk, at an
    offset that depends on the instance count the chunk was CARVED for -- the capacity of a deferred-counters forward,
    not the frame's instance count.  The backward takes that offset (and the segment length) from what the forward
    stamped into the image chunk's counters: called with the capacity or with the true count, a deep-walk frame (every
    tile crosses 6+ segment boundaries) gives the gradients of the plain forward, bit for bit; called with FEWER
    instances than a blocking forward rendered, it is refused."""
    from frosting_amd.parallel import ViewParallelRasterizer
    dev = gpu_device
    scene, _, bg = scenes.config_scene("c2", 0, P=300_000)
    scene = scenes.Scene(scene.means3D, scene.scales * 3.0, scene.rotations, (0.004 + 0.026 * scene.opacities).contiguous(), scene.shs, 3)
    cam = scenes.ring_camera(1, 160, 128, 222.0, 222.0).to(dev)
    ref = ViewParallelRasterizer(scene.to(dev), dev)
    img, _ = ref.forward(cam, bg.to(dev))
    gpix, _ = scenes.l1_target_grad(img.cpu(), 5)
    gpix = gpix.to(dev)
    ref.backward(gpix)
    want = ref.exchange.flat.clone()
    assert float(want.abs().max()) > 0
    true_R = ref.num_rendered
    vpr = ViewParallelRasterizer(scene.to(dev), dev, deferred_counters=True, capacity_slack=1.37)
    vpr.forward(cam, bg.to(dev))                    # synchronous first view: sizes the arenas, sets the capacity
    vpr.forward(cam, bg.to(dev))                    # deferred: carved for the capacity
    assert vpr.num_rendered == vpr.capacity > true_R
    vpr.backward(gpix)                              # R = the capacity (what the deferred forward returned)
    assert vpr.finish() is True and vpr.true_num_rendered == true_R
    assert torch.equal(vpr.exchange.flat, want)
    vpr.exchange.flat.zero_()
    vpr.num_rendered = true_R                       # R = the frame's instance count: another carve, the same checkpoints
    vpr.backward(gpix)
    torch.cuda.synchronize(dev)
    assert torch.equal(vpr.exchange.flat, want)
    ref.num_rendered = true_R - 1                   # fewer than the forward rendered: slots and item lists would overrun
    with pytest.raises(RuntimeError, match="rendered"):
        ref.backward(gpix)


def test_per_call_modes_of_two_rasterizers_on_two_threads(gpu_device):
    """frg_forward_args carries exact_blend / tight_binning / async_sh per call: two rasterizers with different modes,
    interleaved from two host threads (each on its own stream), produce what the same modes give when set process-wide
    and run alone -- whatever frg_set_option says meanwhile."""
    import threading
    scene, cam, bg = scenes.config_scene("c2", 5, P=30_000)
    sc = scene.to(gpu_device)
    e = torch.Tensor([])
    args = (bg.to(gpu_device), sc.means3D, e, sc.opacities, sc.scales, sc.rotations, 1.0, e, cam.viewmatrix.to(gpu_device),
            cam.projmatrix.to(gpu_device), cam.tanfovx, cam.tanfovy, cam.image_height, cam.image_width, sc.shs, sc.sh_degree,
            cam.campos.to(gpu_device), False, False)
    configs = [dict(exact_blend=1, tight_binning=0, async_sh=0), dict(exact_blend=0, tight_binning=1, async_sh=2)]
    want = []
    for md in configs:                       # process-wide, alone
        for k, v in md.items():
            _lib.set_option(k, v)
        out = _C.rasterize_gaussians(*args)
        st = State(scene.P, cam.image_width, cam.image_height, out[0], out[3], out[4], out[5])
        # (tight lists are shorter than num_rendered: only point_list[: end of the last range] is written)
        want.append((out[1].clone(), out[2].clone(), st.point_list[: int(st.ranges.max())].clone(), st.ranges.clone()))
        for k in md:
            _lib.set_option(k, 0)
    _lib.set_option("exact_blend", 0); _lib.set_option("tight_binning", 0); _lib.set_option("async_sh", 0)
    assert not torch.equal(want[0][0], want[1][0]) and want[0][2].numel() != want[1][2].numel()   # the modes do differ
    errors = []

    def worker(which):
        try:
            with torch.cuda.stream(torch.cuda.Stream(gpu_device)):
                for it in range(12):
                    out = _C.rasterize_gaussians(*args, modes=configs[which])
                    st = State(scene.P, cam.image_width, cam.image_height, out[0], out[3], out[4], out[5])
                    torch.cuda.current_stream().synchronize()
                    if not (torch.equal(out[1], want[which][0]) and torch.equal(out[2], want[which][1]) and
                            torch.equal(st.ranges, want[which][3]) and
                            torch.equal(st.point_list[: want[which][2].numel()], want[which][2])):
                        errors.append((which, it))
        except Exception as ex:      # noqa: BLE001
            errors.append((which, repr(ex)))
    threads = [threading.Thread(target=worker, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for it in range(20):                     # the process-wide options flip meanwhile
        _lib.set_option("exact_blend", it & 1)
        _lib.set_option("tight_binning", (it >> 1) & 1)
    for t in threads:
        t.join()
    assert not errors, errors


def test_counter_mailbox_and_copy_read_back_agree(gpu_device, ops):
    """The blocking forward learns num_rendered and the sort's class sizes from a pinned mailbox the scan workgroups
    post to (the scatter is enqueued while the scan stage still runs; api.hip forward_blocking) -- option counter_mailbox = 0 restores
    the copy + stream synchronisation.  Same counters, so the same everything: views with short lists, with lists
    beyond the LDS sort (the plan kernel's fork moves), an empty view and the prefiltered assertion."""
    dev = gpu_device
    cases = []
    scene, cam, bg = scenes.config_scene("c2", 1, P=60_000)
    cases.append((scene, cam, bg))
    scene, cam, bg = scenes.long_list_scene(P=300_000)
    cases += [(scene, cam, bg), (scene, cam, bg)]                      # twice: the second forward knows about the long lists
    scene, cam, bg = scenes.config_scene("c2", 0, P=5_000)
    away = scenes.Scene(scene.means3D + torch.tensor([0.0, 0.0, -50.0]), scene.scales, scene.rotations, scene.opacities, scene.shs,
                        scene.sh_degree)                               # everything behind the camera: R = 0
    cases.append((away, cam, bg))
    results = {}
    for mailbox in (1, 0):
        _lib.set_option("counter_mailbox", mailbox)
        for i, (sc, cm, b) in enumerate(cases):
            out, args = Hh.run_ours_native(sc, cm, b, dev, ops=ops)
            st = State(sc.P, cm.image_width, cm.image_height, out[0], out[3], out[4], out[5])
            gpix, _ = scenes.l1_target_grad(out[1].cpu(), 9)
            grads = ops.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(dev)))
            results[(mailbox, i)] = (out[0], out[1].clone(), out[2].clone(), st.ranges.clone(), st.point_list[:out[0]].clone(),
                                     st.n_contrib.clone(), [g.clone() for g in grads])
            del st
    for i in range(len(cases)):
        a, b = results[(1, i)], results[(0, i)]
        assert a[0] == b[0], i
        assert all(torch.equal(x, y) for x, y in zip(a[1:6], b[1:6])), i
        assert all(torch.equal(x, y) for x, y in zip(a[6], b[6])), i
    assert results[(1, 3)][0] == 0 and results[(1, 1)][0] > 300_000
    assert int((results[(1, 1)][3][:, 1] - results[(1, 1)][3][:, 0]).max()) > 8192
    # The scatter also posts how many 64-Gaussian waves need the 16-wave per-Gaussian backward; a backward that reads 0
    # skips that launch.  A post must never outlive its forward: the same buffers (the caching allocator hands the freed
    # blocks out again) filled by a forward WITHOUT mailbox, with giant Gaussians where the previous view had none.
    big, cam_b, bg_b = scenes.long_list_scene(P=300_000)
    tame = scenes.Scene(big.means3D, big.scales.clamp(max=0.02), big.rotations, big.opacities, big.shs, big.sh_degree)
    def grads_of(sc, mailbox):
        _lib.set_option("counter_mailbox", mailbox)
        out, args = Hh.run_ours_native(sc, cam_b, bg_b, dev, ops=ops)
        gpix, _ = scenes.l1_target_grad(out[1].cpu(), 9)
        return [g.clone() for g in ops.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(dev)))]
    want = grads_of(big, 0)
    for _ in range(3):
        grads_of(tame, 1)                      # posts "no heavy waves" for its buffers, then frees them
        got = grads_of(big, 0)                 # no post of its own
        assert all(torch.equal(x, y) for x, y in zip(want, got))
    assert all(torch.equal(x, y) for x, y in zip(want, grads_of(big, 1)))
    # the prefiltered assertion (auxiliary.h:154-162) is raised from the posted counters as well
    scene, cam, bg = scenes.config_scene("c2", 0, P=5_000)
    _lib.set_option("counter_mailbox", 1)
    sc = scene.to(dev)
    e = torch.Tensor([])
    with pytest.raises(RuntimeError, match="filtered"):
        ops.rasterize_gaussians(bg.to(dev), sc.means3D - torch.tensor([0.0, 0.0, 50.0], device=dev), e, sc.opacities, sc.scales, sc.rotations,
                                1.0, e, cam.viewmatrix.to(dev), cam.projmatrix.to(dev), cam.tanfovx, cam.tanfovy, cam.image_height,
                                cam.image_width, sc.shs, sc.sh_degree, cam.campos.to(dev), True, False)


def test_sh_pass_over_the_visible_gaussians_only(gpu_device, ops):
    """A view that sees a part of the model (here: half of it outside the image; with an occlusion mask:
    test_gpu_mesh.py) runs the SH pass over the visible Gaussians of every wave only, their derivative rows stored by
    rank -- chosen from what the previous forward of the thread saw, so the first forward of such a view takes the
    plain pass and the second the sparse one: image, radii and every gradient of the two are identical bit for bit,
    and identical to option sparse_sh = 0."""
    dev = gpu_device
    scene, cam, bg = scenes.config_scene("c3", 0, P=300_000)
    # the ball moved sideways by the half-width of the view at its distance: about half of it leaves the image
    moved = scenes.Scene(scene.means3D + torch.tensor([2.4, 0.0, 0.0]), scene.scales, scene.rotations, scene.opacities, scene.shs,
                         scene.sh_degree)
    def run(sc):
        out, args = Hh.run_ours_native(sc, cam, bg, dev, ops=ops)
        gpix, _ = scenes.l1_target_grad(out[1].cpu(), 13)
        grads = ops.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(dev)))
        return out[0], out[1].clone(), out[2].clone(), [g.clone() for g in grads]
    _lib.set_option("sparse_sh", 0)
    want = run(moved)
    vis = float((want[2] > 0).float().mean())
    assert 0.1 < vis < 0.7, vis
    _lib.set_option("sparse_sh", 1)
    run(scene)                       # a view that sees (nearly) everything: the next one starts with the plain pass
    for i in range(3):               # first: plain pass; then the pass over the visible ones
        got = run(moved)
        assert got[0] == want[0] and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), i
        assert all(torch.equal(a, b) for a, b in zip(got[3], want[3])), i
    # and back: a fully visible view after sparse ones
    full_want = None
    for i in range(2):
        got = run(scene)
        full_want = full_want or got
        assert all(torch.equal(a, b) for a, b in zip(got[3], full_want[3]))


@pytest.mark.parametrize("frame", ["c3:300000:3", "c3-half-outside:300000:3", "c2:60000:2", "c2:60000:3:async_sh=2"])
def test_sh_direction_derivative_formed_by_the_backward_gives_the_same_bits(gpu_device, ops, frame):
    """VERDICT r04 item 6.  Option sh_dir_in_backward = 1: the forward's SH pass neither sums nor stores d(colour)/d(direction)
    (36 bytes per VISIBLE Gaussian); the per-Gaussian backward forms it from the 192-byte SH rows of the Gaussians that HAVE a
    gradient, coefficient after coefficient in the forward's order -- image, radii and every gradient bit as with the rows
    stored, on the plain pass, on the pass over the visible Gaussians of a half-visible model (rows by rank), at a lower
    active degree and with the colours on the side stream.  The backward follows what ITS forward stamped (GeomState::
    sh_layout), not the option at the time it runs."""
    dev = gpu_device
    parts = frame.split(":")
    name, P, deg = parts[0], int(parts[1]), int(parts[2])
    scene, cam, bg = scenes.config_scene(name.split("-")[0], 0, P=P)
    means = scene.means3D + (torch.tensor([2.4, 0.0, 0.0]) if "half-outside" in name else 0.0)
    scene = scenes.Scene(means.contiguous(), scene.scales, scene.rotations, scene.opacities, scene.shs, deg)
    for extra in parts[3:]:
        k, v = extra.split("=")
        _lib.set_option(k, int(v))

    def run(flip_to=None):
        out, args = Hh.run_ours_native(scene, cam, bg, dev, ops=ops)
        gpix, _ = scenes.l1_target_grad(out[1].cpu(), 13)
        if flip_to is not None:
            _lib.set_option("sh_dir_in_backward", flip_to)          # AFTER the forward
        grads = ops.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(dev)))
        return out[0], out[1].clone(), out[2].clone(), [g.clone() for g in grads]
    _lib.set_option("sh_dir_in_backward", 0)
    run()                                    # (a half-visible model: the second forward takes the pass over the visible ones)
    want = run()
    assert float(want[3][GRAD_NAMES.index("dL_dmeans3D")].abs().max()) > 0
    _lib.set_option("sh_dir_in_backward", 1)
    for flip in (None, 0):
        got = run(flip)
        _lib.set_option("sh_dir_in_backward", 1)
        assert got[0] == want[0] and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
        for n, a, b in zip(GRAD_NAMES, got[3], want[3]):
            assert torch.equal(a, b), (n, flip)
    _lib.set_option("sh_dir_in_backward", 0)
    got = run(1)                             # rows stored by the forward, option flipped before the backward
    assert all(torch.equal(a, b) for a, b in zip(got[3], want[3]))


def test_sh_direction_derivative_in_the_backward_with_raw_parameters_and_a_shell(gpu_device):
    """The same through the view-parallel rasterizer on RAW parameters (activations inside the per-Gaussian kernels) and on
    the C4 shell scene under its occlusion mask (sparsely visible waves): the flat gradient buffer bit for bit."""
    from frosting_amd.parallel import ViewParallelRasterizer
    dev = gpu_device
    scene, cam, bg = scenes.config_scene("c3", 1, P=200_000)
    raw = scenes.Scene(scene.means3D, torch.log(scene.scales), scene.rotations * 1.3, torch.log(scene.opacities / (1 - scene.opacities)),
                       scene.shs, scene.sh_degree)
    flats = {}
    for mode in (0, 1):
        _lib.set_option("sh_dir_in_backward", mode)
        vpr = ViewParallelRasterizer(raw.to(dev), dev, raw_params=True)
        for _ in range(2):
            img, _ = vpr.forward(cam.to(dev), bg.to(dev))
            gpix, _ = scenes.l1_target_grad(img.cpu(), 7)
            vpr.exchange.flat.zero_()
            vpr.backward(gpix.to(dev), 0)
        flats[mode] = vpr.exchange.flat.clone()
    assert float(flats[0].abs().max()) > 0 and torch.equal(flats[0], flats[1])


def test_radii_may_be_null_like_the_reference(gpu_device):
    """rasterizer.h:54 / rasterizer_impl.cu:228-231,375-377: radii == nullptr -> the op keeps them in its own
    geometry state, forward and backward."""
    import ctypes as C
    from frosting_amd.parallel import _Arena, _p
    scene, cam, bg = scenes.config_scene("mini", 5, P=2000)
    sc, cd, bgd = scene.to(gpu_device), cam.to(gpu_device), bg.to(gpu_device)
    L = _lib.lib()
    out, args = Hh.run_ours_native(scene, cam, bg, gpu_device)
    gpix, _ = scenes.l1_target_grad(out[1].cpu(), 31)
    gpix = gpix.to(gpu_device)
    want = _C.rasterize_gaussians_backward(*_bwd_args(args, out, gpix))
    geom, binning, img, work = (_Arena(gpu_device) for _ in range(4))
    color = torch.empty_like(out[1])
    stream = C.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    P = scene.P
    R = L.frg_forward(geom.cb, binning.cb, img.cb, None, P, 3, 16, _p(bgd), cam.image_width, cam.image_height,
                      _p(sc.means3D), _p(sc.shs), None, _p(sc.opacities), _p(sc.scales), 1.0, _p(sc.rotations), None,
                      _p(cd.viewmatrix), _p(cd.projmatrix), _p(cd.campos), float(cam.tanfovx), float(cam.tanfovy), 0,
                      _p(color), None, 0, stream)
    assert R == out[0] and torch.equal(color, out[1])
    ws = int(L.frg_backward_workspace_bytes(P, R))
    w = work.ensure(ws)
    f = lambda *s: torch.empty(s, device=gpu_device)
    g = dict(m2=f(P, 3), op=f(P, 1), col=f(P, 3), m3=f(P, 3), cov=f(P, 6), sh=f(P, 16, 3), sc=f(P, 3), rot=f(P, 4))
    rc = L.frg_backward(P, 3, 16, R, _p(bgd), cam.image_width, cam.image_height, _p(sc.means3D), _p(sc.shs), None,
                        _p(sc.scales), 1.0, _p(sc.rotations), None, _p(cd.viewmatrix), _p(cd.projmatrix), _p(cd.campos),
                        float(cam.tanfovx), float(cam.tanfovy), None, _p(geom.buf), _p(binning.buf), _p(img.buf), _p(gpix),
                        _p(g["m2"]), None, _p(g["op"]), _p(g["col"]), _p(g["m3"]), _p(g["cov"]), _p(g["sh"]), _p(g["sc"]),
                        _p(g["rot"]), _p(w), w.numel(), 0, stream)
    assert rc == 0, _lib.last_error()
    for a, c in zip(want, (g["m2"], g["col"], g["op"], g["m3"], g["cov"], g["sh"], g["sc"], g["rot"])):
        assert torch.equal(a, c)


def test_deferred_forward_overflow_then_backward_before_finish(gpu_device):
    """Capacity exceeded on a DIFFERENT view than the one rendered before, and the backward issued before
    finish() has reported it (the documented order of a pipelined step): nothing may be read out of range,
    the frame is the background, every gradient is zero, and the repeated view is exact."""
    from frosting_amd.parallel import ViewParallelRasterizer
    scene, cam_a, bg = scenes.config_scene("c2", 0, P=60_000)
    cam_b = scenes.ring_camera(3, cam_a.image_width, cam_a.image_height, 1111.0, 1111.0)
    dev = gpu_device
    ref = ViewParallelRasterizer(scene.to(dev), dev)
    img_b, _ = ref.forward(cam_b.to(dev), bg.to(dev))
    img_b = img_b.clone()
    gpix, _ = scenes.l1_target_grad(img_b.cpu(), 77)
    gpix = gpix.to(dev)
    ref.backward(gpix)
    flat_b = ref.exchange.flat.clone()
    vpr = ViewParallelRasterizer(scene.to(dev), dev, deferred_counters=True)
    vpr.forward(cam_a.to(dev), bg.to(dev))          # synchronous first view: sizes the arenas
    vpr.backward(gpix)
    vpr.capacity = 1000                              # far below view B's instance count
    img, radii = vpr.forward(cam_b.to(dev), bg.to(dev))
    vpr.backward(gpix)                               # before finish(): must be harmless
    torch.cuda.synchronize(dev)
    assert float(vpr.exchange.flat.abs().max()) == 0.0 and bool(torch.isfinite(vpr.exchange.flat).all())
    assert torch.equal(img, bg.to(dev)[:, None, None].expand_as(img))
    assert vpr.finish() is False and vpr.capacity > 1000
    img2, _ = vpr.forward(cam_b.to(dev), bg.to(dev))
    vpr.backward(gpix)
    assert vpr.finish() is True
    assert torch.equal(img2, img_b) and torch.equal(vpr.exchange.flat, flat_b)


@pytest.mark.parametrize("tight", [0, 1])
def test_full_size_image_every_binning_mode_fits_the_lds(gpu_device, tight):
    """The LDS budget of the binning kernels depends on the number of tiles (FRG_BIN_MAX_LDS_TILES = 10112 bins): run
    the full 1600x1056 grid (6600 tiles), the largest grid of 1536 columns whose tile bins AND record cells fit the LDS
    (1536x1520: 9120 tiles + 950 cells = 10070, cell-ordered scatter), one with both just beyond (1536^2: 9216 + 960 =
    10176: scatter in the caller's order), the largest whose tile bins alone fit (1616x1600: 101 x 100 = 10100 tiles) and
    one beyond the LDS (1664^2: 10816 tiles, global-atomic binning), in both binning modes, against the C oracle."""
    scene, _, bg = scenes.config_scene("c2", 0, P=20_000)
    _lib.set_option("tight_binning", tight)
    for (w, h) in [(1600, 1056), (1536, 1520), (1536, 1536), (1616, 1600), (1664, 1664)]:
        cam = scenes.ring_camera(2, w, h, 1334.0, 1334.0)
        out, _ = Hh.run_ours_native(scene, cam, bg, gpu_device)
        o = G.forward(**Hh.oracle_kwargs(scene, cam, bg))
        assert out[0] == o["num_rendered"]
        np.testing.assert_array_equal(out[2].cpu().numpy(), o["radii"])
        assert np.abs(out[1].cpu().numpy() - o["out_color"]).mean() <= L1_BAR


def test_backward_uses_the_blend_arithmetic_of_its_forward(gpu_device):
    """A forward with a per-call mode (frg_forward_args::exact_blend) followed by the reference-shaped backward call,
    which has no mode argument: the blend pass of that backward recomputes ITS forward's alpha / T / contributor tests,
    so it takes that forward's arithmetic (remembered by the library per geometry buffer), not the process-wide option
    at the time of the call.  Both directions, bit for bit."""
    scene, cam, bg = scenes.config_scene("c2", 2, P=40_000)
    want = {}
    for exact in (0, 1):
        _lib.set_option("exact_blend", exact)
        out, args = Hh.run_ours_native(scene, cam, bg, gpu_device)
        gpix, _ = scenes.l1_target_grad(out[1].cpu(), 41)
        gpix = gpix.to(gpu_device)
        want[exact] = (out[1].clone(), [g.clone() for g in _C.rasterize_gaussians_backward(*_bwd_args(args, out, gpix))])
    assert not torch.equal(want[0][1][0], want[1][1][0])          # (the two arithmetics do differ in the last bits)
    for exact in (0, 1):
        _lib.set_option("exact_blend", 1 - exact)                 # the process says the opposite, before and after
        out, args = Hh.run_ours_native(scene, cam, bg, gpu_device)  # ... a forward of the other mode on other buffers
        out_m = _C.rasterize_gaussians(*args, modes={"exact_blend": exact})
        assert torch.equal(out_m[1], want[exact][0])
        gpix, _ = scenes.l1_target_grad(want[exact][0].cpu(), 41)
        got = _C.rasterize_gaussians_backward(*_bwd_args(args, out_m, gpix.to(gpu_device)))
        assert all(torch.equal(a, b) for a, b in zip(want[exact][1], got)), exact
        # and the backward of the process-default forward made in between still follows ITS forward
        gpix, _ = scenes.l1_target_grad(want[1 - exact][0].cpu(), 41)
        got2 = _C.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(gpu_device)))
        assert all(torch.equal(a, b) for a, b in zip(want[1 - exact][1], got2)), exact


def test_reached_marks_prune_work_not_results(gpu_device):
    """The backward blend marks the Gaussians it staged with a non-empty quadrant mask (byte 1 of the record's flag word)
    and the per-Gaussian backward reduces the slots of the marked ones only.  The marks are a function of the forward
    state alone, set by every backward itself: a repeated backward, or one that starts from cleared marks, gives the same
    bits.  With EVERY Gaussian marked (the reduction before round 4's pruning) the same slots are added, grouped differently
    into the scan's batches of 64: the same gradients to float32 rounding.  The next forward on the buffers clears the marks."""
    from frosting_amd.introspect import State
    scene, cam, bg = scenes.config_scene("c3", 1, P=1_000_000)     # (a third of the visible Gaussians stay unreached: tools/reached_fraction.py)
    out, args = Hh.run_ours_native(scene, cam, bg, gpu_device)
    W, H = cam.image_width, cam.image_height
    st = State(scene.P, W, H, out[0], out[3], out[4], out[5])
    assert int(((st.flag_words >> 8) & 0xFF).ne(0).sum()) == 0                  # a forward leaves no mark
    gpix, _ = scenes.l1_target_grad(out[1].cpu(), 13)
    b = _bwd_args(args, out, gpix.to(gpu_device))
    want = [g.clone() for g in _C.rasterize_gaussians_backward(*b)]
    marked = ((st.flag_words >> 8) & 0xFF).ne(0)
    visible = out[2] > 0
    n_marked, n_visible = int(marked.sum()), int(visible.sum())
    assert 0.3 * n_visible < n_marked < 0.8 * n_visible, (n_marked, n_visible)   # the marks do prune (and only visible ones carry them)
    assert not bool((marked & ~visible).any())
    with_grad = torch.zeros(scene.P, dtype=torch.bool, device=gpu_device)
    for g in want:
        with_grad |= g.reshape(scene.P, -1).ne(0).any(1)
    assert not bool((with_grad & ~marked).any())                                 # every Gaussian with a gradient was marked
    again = _C.rasterize_gaussians_backward(*b)                                 # the marks of the first backward are still there
    assert all(torch.equal(x, y) for x, y in zip(want, again))
    st.flag_words.bitwise_or_(0x100)                                             # every Gaussian marked: nothing pruned
    # the nine sums per Gaussian agree to rounding; the chain behind them (covariance, scales, quaternions) amplifies that
    # on the few ill-conditioned Gaussians every scene has (section 3 of DESIGN.md), so those tensors are compared on all
    # rows but the ceil(1e-4 P) farthest -- the same rule the gradient bars use
    drop = -(-scene.P // 10_000)
    report = []
    for i, (x, y) in enumerate(zip(want, _C.rasterize_gaussians_backward(*b))):
        d2 = (x.double() - y.double()).reshape(scene.P, -1).pow(2).sum(1)
        kept = d2.sum() - torch.topk(d2, drop).values.sum()
        report.append((i, float(d2.sum().sqrt() / x.double().norm()), float(kept.clamp_min(0).sqrt() / x.double().norm())))
    assert all(r[2] <= 2e-6 for r in report), report
    assert all(r[1] <= 2e-6 for r in report[:3]), report                         # dL_dmeans2D, dL_dcolors, dL_dopacity: no amplification
    st.flag_words.bitwise_and_(0xFF)                                             # none marked: this backward marks its own
    assert all(torch.equal(x, y) for x, y in zip(want, _C.rasterize_gaussians_backward(*b)))
    assert torch.equal(((st.flag_words >> 8) & 0xFF).ne(0), marked)
    # a rasterizer that keeps its buffers: the next forward clears the marks of the last backward
    from frosting_amd.parallel import ViewParallelRasterizer
    vpr = ViewParallelRasterizer(scene.to(gpu_device), gpu_device)
    cam_d, bg_d = cam.to(gpu_device), bg.to(gpu_device)
    img, _ = vpr.forward(cam_d, bg_d)
    assert torch.equal(img, out[1])
    vpr.backward(gpix.to(gpu_device), 0)
    stv = lambda: State(scene.P, W, H, vpr.true_num_rendered, vpr.geom.buf, vpr.binning.buf, vpr.img.buf)
    assert torch.equal(((stv().flag_words >> 8) & 0xFF).ne(0), marked)
    vpr.forward(cam_d, bg_d)
    assert int(((stv().flag_words >> 8) & 0xFF).ne(0).sum()) == 0


def test_two_backwards_of_one_forward_on_two_streams(gpu_device):
    """frg_backward WRITES one byte of the geometry buffer per reached Gaussian (the marks; the reference's callers never
    had to know).  Two backwards of the SAME forward state -- what retain_graph + a second .backward() does -- issued from
    two host threads on two streams at once, the marks starting cleared: both store the same byte values into words the
    other one is reading with 16-byte loads, and a load sees the mark or does not -- which only decides whether the byte is
    stored again.  Every backward sets all of its marks in its own blend pass, before its own per-Gaussian pass reads them
    (stream order), and its slots live in its own workspace: each call reproduces the lone backward bit for bit."""
    import threading
    from frosting_amd.introspect import State
    dev = gpu_device
    scene, cam, bg = scenes.config_scene("c3", 1, P=1_000_000)
    out, args = Hh.run_ours_native(scene, cam, bg, dev)
    st = State(scene.P, cam.image_width, cam.image_height, out[0], out[3], out[4], out[5])
    grads = [scenes.l1_target_grad(out[1].cpu(), 60 + k)[0].to(dev) for k in range(2)]
    lone = [[g.clone() for g in _C.rasterize_gaussians_backward(*_bwd_args(args, out, gp))] for gp in grads]
    torch.cuda.synchronize(dev)
    for trial in range(3):
        st.flag_words.bitwise_and_(0xFF)                    # marks cleared: both backwards set them while the other reads
        torch.cuda.synchronize(dev)
        streams = [torch.cuda.Stream(dev) for _ in range(2)]
        got, errs = [None, None], []
        go = threading.Barrier(2)

        def run(k):
            try:
                with torch.cuda.stream(streams[k]):
                    go.wait()
                    got[k] = [g.clone() for g in _C.rasterize_gaussians_backward(*_bwd_args(args, out, grads[k]))]
                streams[k].synchronize()
            except Exception as ex:       # noqa: BLE001
                errs.append(ex)

        th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for k in range(2):
            assert all(torch.equal(x, y) for x, y in zip(lone[k], got[k])), (trial, k)


_HEAVY_SCRIPT = r"""
import sys, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from frosting_amd import _lib, scenes
from frosting_amd.rasterizer import _C
import helpers as Hh
from test_gpu_parity import _bwd_args
dev = torch.device("cuda:0")
scene = scenes.make_skew_scene(20_000, 99, centres=[[0.0, 0.0, 0.0]], cluster_sigma=0.05, cluster_frac=0.2, n_big=120, big_scale=0.3)
cam, bg = scenes.ring_camera(0, 320, 240, 267.0, 267.0), torch.zeros(3)
out, args = Hh.run_ours_native(scene, cam, bg, dev)
gpix, _ = scenes.l1_target_grad(out[1].cpu(), 3)
b = _bwd_args(args, out, gpix.to(dev))
from frosting_amd.introspect import State
st = State(scene.P, 320, 240, out[0], out[3], out[4], out[5])
slots = st.tiles_touched[: (scene.P // 64) * 64].view(-1, 64).sum(1)
assert int((slots > 4 * 896).sum()) >= 1, "the scene has no heavy wave"
want = [g.clone() for g in _C.rasterize_gaussians_backward(*b)]            # 16-wave launch + plain kernel
assert _lib.set_option("assume_no_heavy", 1) >= 0, _lib.last_error()
got = _C.rasterize_gaussians_backward(*b)                                    # plain kernel alone
_lib.set_option("assume_no_heavy", 0)
assert all(torch.isfinite(g).all() for g in got)
assert all(torch.equal(a, c) for a, c in zip(want, got)), "gradients differ when the 16-wave launch is skipped"
# more forwards than the library remembers (64): the first one's backward still gives the same bits
small = scenes.make_scene(500, 5)
keep = [Hh.run_ours_native(small, cam, bg, dev)[0] for _ in range(70)]
again = _C.rasterize_gaussians_backward(*b)
assert all(torch.equal(a, c) for a, c in zip(want, again)), "gradients differ once the forward's note was evicted"
print("HEAVY-OK", int((slots > 4 * 896).sum()))
"""


def test_heavy_waves_are_reduced_whatever_the_host_believes(gpu_device):
    """The backward skips the 16-wave launch of the per-Gaussian backward when its forward posted "no wave owns more than
    3584 slots".  Should that belief ever be wrong, the plain kernel reduces such waves itself (FRG_PBW_NO_HEAVY_LAUNCH):
    forced here with the test hook "assume_no_heavy" (own process: the hook only exists under FROSTING_EXPERIMENTS=1) on
    a scene WITH heavy waves -- gradients identical bit for bit -- and with more outstanding forwards (70) than the
    library's 64 notes (ADVICE r03 / VERDICT r03 weak 11)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FROSTING_EXPERIMENTS="1")
    r = subprocess.run([sys.executable, "-c", _HEAVY_SCRIPT.format(root=root, tests=os.path.join(root, "tests"))],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "HEAVY-OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_forward_tile_order_changes_nothing(gpu_device):
    """Option fwd_order: the forward blend's workgroups take the tiles longest list first (default; the size-class lists of
    the scan, the empty tiles last) or band by band in tile order (rounds 1-3).  Scheduling only: image, per-pixel
    bookkeeping, checkpoints-driven backward -- every bit the same, on a full frame, on a frame with most tiles empty, on a
    ragged image and on an image without any instance."""
    scene, cam, bg = scenes.config_scene("c2", 6, P=70_000)
    corner = scenes.Scene(scene.means3D * 0.1 + torch.tensor([0.8, -0.7, 0.0]), scene.scales, scene.rotations, scene.opacities,
                          scene.shs, scene.sh_degree)
    nothing = scenes.Scene(scene.means3D * 0.0 + cam.campos, scene.scales, scene.rotations, scene.opacities, scene.shs, scene.sh_degree)
    ragged = scenes.ring_camera(2, 333, 201, 300.0, 300.0)
    for label, sc, cm in (("full", scene, cam), ("corner", corner, cam), ("ragged", scene, ragged), ("empty", nothing, cam)):
        res = {}
        for order in (1, 0):
            _lib.set_option("fwd_order", order)
            out, args = Hh.run_ours_native(sc, cm, bg, gpu_device)
            st = State(sc.P, cm.image_width, cm.image_height, out[0], out[3], out[4], out[5])
            gpix, _ = scenes.l1_target_grad(out[1].cpu(), 17)
            grads = _C.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(gpu_device)))
            res[order] = (out[0], out[1].clone(), out[2].clone(), st.final_T.clone(), st.n_contrib.clone(), [g.clone() for g in grads])
            del st
        _lib.set_option("fwd_order", 1)
        a, b = res[1], res[0]
        assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:5], b[1:5])), label
        assert all(torch.equal(x, y) for x, y in zip(a[5], b[5])), label
        if label == "empty":
            assert a[0] == 0 and torch.equal(a[1], bg.to(gpu_device)[:, None, None].expand_as(a[1]))
        if label == "corner":
            assert int((res[1][4] > 0).sum()) > 0



@pytest.mark.parametrize("exact", [0, 1])
def test_forward_blend_entries_per_trip_change_nothing(gpu_device, exact):
    """Option fwd_unroll8 (0 never | 1 the host's rule: frames whose longest list is 3.5 x their mean list | 2 always): the
    forward blend computes the falloff of four or of eight list entries side by side before the sequential part of the
    pixels' chains -- the same operations on the same values in the same order: image, per-pixel bookkeeping and the gradients
    of the backward that starts from its checkpoints are the same bits, in both arithmetics, on a full frame, a frame with most
    tiles empty (long lists in a corner: the rule's case) and a ragged image."""
    scene, cam, bg = scenes.config_scene("c2", 6, P=70_000)
    corner = scenes.Scene(scene.means3D * 0.1 + torch.tensor([0.8, -0.7, 0.0]), scene.scales, scene.rotations, scene.opacities,
                          scene.shs, scene.sh_degree)
    ragged = scenes.ring_camera(2, 333, 201, 300.0, 300.0)
    _lib.set_option("exact_blend", exact)
    _lib.set_option("fused_small", 0)                  # (the small-frame form walks four entries per trip)
    for label, sc, cm in (("full", scene, cam), ("corner", corner, cam), ("ragged", scene, ragged)):
        res = {}
        for mode in (0, 2, 1):
            _lib.set_option("fwd_unroll8", mode)
            out, args = Hh.run_ours_native(sc, cm, bg, gpu_device)
            st = State(sc.P, cm.image_width, cm.image_height, out[0], out[3], out[4], out[5])
            gpix, _ = scenes.l1_target_grad(out[1].cpu(), 23)
            grads = _C.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(gpu_device)))
            res[mode] = (out[0], out[1].clone(), out[2].clone(), st.final_T.clone(), st.n_contrib.clone(), [g.clone() for g in grads])
            del st
        for other in (2, 1):
            a, b = res[0], res[other]
            assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:5], b[1:5])), (label, other)
            assert all(torch.equal(x, y) for x, y in zip(a[5], b[5])), (label, other)
    _lib.set_option("fwd_unroll8", 1)
    _lib.set_option("fused_small", 1)
    _lib.set_option("exact_blend", 0)


def test_a_backward_finds_its_forwards_modes_in_the_buffers_and_in_the_ctx(gpu_device, ops):
    """What a backward must know about its forward beyond the three buffers -- the blend arithmetic, and whether anything was
    kept at all -- travels WITH them: stamped by the forward's blend kernel into the image chunk
    (Counters::fwd_flags) and carried by the autograd ctx of the Python layer.  So
      * the first of 1100 forwards still gets its own arithmetic in its backward (the library's notes hold 1024), with the
        process option flipped meanwhile;
      * buffers CLONED to other addresses (offloaded and restored, copied by a checkpointing wrapper) give the same bits;
      * the clone of a forward_only forward's buffers is refused like the original;
      * the module's backward follows the mode its ctx carried, whatever the option says by then."""
    dev = gpu_device
    scene, cam, bg = scenes.config_scene("c2", 1, P=30_000)
    tiny, tcam, tbg = scenes.config_scene("mini", 0, P=300)
    _lib.set_option("exact_blend", 1)
    out, args = Hh.run_ours_native(scene, cam, bg, dev, ops=ops)
    gpix, _ = scenes.l1_target_grad(out[1].cpu(), 5)
    gpix = gpix.to(dev)
    want = [g.clone() for g in ops.rasterize_gaussians_backward(*_bwd_args(args, out, gpix))]
    _lib.set_option("exact_blend", 0)
    fast_out, _ = Hh.run_ours_native(scene, cam, bg, dev, ops=ops)
    fast = [g.clone() for g in ops.rasterize_gaussians_backward(*_bwd_args(args, fast_out, gpix))]
    assert not all(torch.equal(a, b) for a, b in zip(want, fast))          # the two arithmetics do differ on this frame
    keep_alive = [Hh.run_ours_native(tiny, tcam, tbg, dev, ops=ops)[0] for _ in range(1100)]   # 1100 other geometry buffers, all alive
    assert len({o[3].data_ptr() for o in keep_alive}) == 1100
    got = ops.rasterize_gaussians_backward(*_bwd_args(args, out, gpix))        # process option: fast; the forward was exact
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    del keep_alive
    for src, ref in ((out, want), (fast_out, fast)):
        clone = (src[0], src[1], src[2], src[3].clone(), src[4].clone(), src[5].clone())
        for opt in (0, 1):
            _lib.set_option("exact_blend", opt)
            got = ops.rasterize_gaussians_backward(*_bwd_args(args, clone, gpix))
            assert all(torch.equal(a, b) for a, b in zip(ref, got)), opt
    fo = ops.rasterize_gaussians_forward_only(*args, torch.empty(0))
    fo_clone = (fo[0], fo[1], fo[2], fo[3].clone(), fo[4].clone(), fo[5].clone())
    with pytest.raises(RuntimeError, match="forward_only"):
        ops.rasterize_gaussians_backward(*_bwd_args(args, fo_clone, gpix))
    with pytest.raises(RuntimeError, match="stamp"):                            # buffers no forward ever filled
        ops.rasterize_gaussians_backward(*_bwd_args(args, (out[0], out[1], out[2], torch.zeros_like(out[3]), torch.zeros_like(out[4]),
                                                                 torch.zeros_like(out[5])), gpix))
    # the module: the ctx carries the forward's arithmetic
    from frosting_amd.rasterizer import make_rasterizer_class
    Rast, _ = make_rasterizer_class(ops)
    sc = scene.to(dev)
    kw = dict(means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, shs=sc.shs, scales=sc.scales, rotations=sc.rotations)
    for fwd_opt, ref in ((1, want), (0, fast)):
        _lib.set_option("exact_blend", fwd_opt)
        leaf = sc.means3D.clone().requires_grad_(True)
        img, _ = Rast(Hh.settings_for(cam, bg, 3, dev))(means3D=leaf, **kw)
        _lib.set_option("exact_blend", 1 - fwd_opt)
        img.backward(gpix)
        assert torch.equal(leaf.grad, ref[GRAD_NAMES.index("dL_dmeans3D")]), fwd_opt


@pytest.mark.parametrize("exact", [1, 0])
def test_forward_only_keeps_nothing_for_a_backward_and_changes_no_output_bit(gpu_device, ops, exact):
    """frg_forward_args::forward_only (every forward paid for the backward's checkpoints): the image, radii and
    instance count of a forward told that no backward follows are those of the plain forward, bit for bit -- on a frame
    whose tiles cross segment boundaries (checkpoints would be written), through both bindings, under an occlusion mask;
    a backward on its buffers is refused; the autograd function takes the form by itself when no input needs a gradient
    (torch.no_grad(), detached parameters) and the plain one as soon as one does."""
    dev = gpu_device
    _lib.set_option("exact_blend", exact)
    base, _, bg = scenes.config_scene("c2", 0, P=200_000)
    scene = scenes.Scene(base.means3D, base.scales * 2.5, base.rotations, (0.01 + 0.05 * base.opacities).contiguous(), base.shs, 3)
    cam = scenes.ring_camera(1, 320, 240, 444.0, 444.0)
    out, args = Hh.run_ours_native(scene, cam, bg, dev, ops=ops)
    st = State(scene.P, cam.image_width, cam.image_height, out[0], out[3], out[4], out[5])
    assert int((st.ranges[:, 1] - st.ranges[:, 0]).max()) > 1100        # lists longer than two segments of 512
    want = (out[0], out[1].clone(), out[2].clone(), st.final_T.clone(), st.n_contrib.clone())
    del st
    keep = (torch.arange(scene.P, device=dev) % 3 != 0)
    for mask in (torch.empty(0), keep):
        fo = ops.rasterize_gaussians_forward_only(*args, mask.to(dev) if mask.numel() else mask)
        if mask.numel() == 0:
            st = State(scene.P, cam.image_width, cam.image_height, fo[0], fo[3], fo[4], fo[5])
            assert fo[0] == want[0] and torch.equal(fo[1], want[1]) and torch.equal(fo[2], want[2])
            assert torch.equal(st.final_T, want[3]) and torch.equal(st.n_contrib, want[4])
            del st
        else:
            plain = ops.rasterize_gaussians_masked(*args, keep)
            assert fo[0] == plain[0] and torch.equal(fo[1], plain[1]) and torch.equal(fo[2], plain[2])
        gpix, _ = scenes.l1_target_grad(fo[1].cpu(), 3)
        with pytest.raises(RuntimeError, match="forward_only"):
            ops.rasterize_gaussians_backward(*_bwd_args(args, fo, gpix.to(dev)))
    # the buffers of a plain forward still serve their backward afterwards (the note belongs to the buffer, not the thread)
    gpix, _ = scenes.l1_target_grad(out[1].cpu(), 3)
    grads = ops.rasterize_gaussians_backward(*_bwd_args(args, out, gpix.to(dev)))
    assert float(grads[GRAD_NAMES.index("dL_dmeans3D")].abs().max()) > 0
    # the module: no_grad / no leaf -> forward-only by itself, same image; with a leaf the gradients are the plain ones
    from frosting_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    sc = scene.to(dev)
    settings = GaussianRasterizationSettings(cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy, bg.to(dev), 1.0,
                                             cam.viewmatrix.to(dev), cam.projmatrix.to(dev), 3, cam.campos.to(dev), False, False)
    kw = dict(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), opacities=sc.opacities, shs=sc.shs, scales=sc.scales,
              rotations=sc.rotations)
    r = GaussianRasterizer(settings)
    with torch.no_grad():
        img0, radii0 = r(**kw)
    assert torch.equal(img0, want[1]) and torch.equal(radii0, want[2]) and not img0.requires_grad
    img1, _ = r(**kw)                                     # no leaf requires a gradient
    assert torch.equal(img1, want[1]) and not img1.requires_grad
    leaf = sc.means3D.clone().requires_grad_(True)
    img2, _ = r(**dict(kw, means3D=leaf))
    assert torch.equal(img2, want[1])
    (img2 * gpix.to(dev)).sum().backward()
    assert torch.equal(leaf.grad, grads[GRAD_NAMES.index("dL_dmeans3D")])
