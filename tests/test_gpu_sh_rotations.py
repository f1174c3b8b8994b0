"""Per-Gaussian rotated SH view directions (sh_rotations) on the device: frg_forward_args / frg_backward_args::sh_rotations
through both bindings, against the reference's colours (tests/golden/sh_rotations.npz) and float64 autograd of
sh.points_rgb.  Scene: 4133 Gaussians (the last wave is partial) on a 128 x 96 image, one ring camera."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from frosting_amd import _lib, fused, introspect, scenes, sh

import helpers as Hh

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
P, W, H = 4133, 128, 96
E = torch.Tensor([])


def _random_rotations(n, seed):
    """rotation matrices from random unit quaternions, formed in float64 and rounded once"""
    g = torch.Generator().manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(n, 4, generator=g, dtype=torch.float64), dim=-1)
    r, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(n, 3, 3).float().contiguous()


class Case:
    """The scene on the device, the native arguments of a call and what the tests share of it."""

    def __init__(self, dev):
        self.dev = dev
        self.scene = scenes.make_scene(P, scenes.SEED_BASE + 77, log_scale=math.log(0.04))
        self.cam = scenes.ring_camera(1, W, H, 110.0, 110.0)
        self.bg = torch.tensor([0.1, 0.2, 0.3])
        self.sc = self.scene.to(dev)
        self.rot = _random_rotations(P, 5).to(dev)
        self.keep = (torch.arange(P, device=dev) % 3 == 0)

    def args(self, deg=3, shs=None, colors=None):
        sc, cam, dev = self.sc, self.cam, self.dev
        sh_in = E if colors is not None else (sc.shs if shs is None else shs)
        return (self.bg.to(dev), sc.means3D, E if colors is None else colors, sc.opacities, sc.scales, sc.rotations, 1.0, E,
                cam.viewmatrix.to(dev), cam.projmatrix.to(dev), cam.tanfovx, cam.tanfovy, H, W, sh_in, deg, cam.campos.to(dev),
                False, False)


@pytest.fixture(scope="module")
def case(gpu_device):
    return Case(gpu_device)


def forward(ops, a, rot=None, exact=0, keep=None, forward_only=False):
    """-> (R, image, radii, geom, binning, img) through the binding's sh_rotations export"""
    return ops.rasterize_gaussians_rot(*a, E if keep is None else keep, exact, forward_only, E if rot is None else rot)


def backward(ops, a, out, gpix, rot=None, exact=0):
    """-> the reference's eight gradients (means2D, colors, opacity, means3D, cov3D, sh, scales, rotations)"""
    R, _, radii, geom, binning, img = out
    return ops.rasterize_gaussians_backward_rot(a[0], a[1], radii, a[2], a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], gpix, a[14],
                                                a[15], a[16], geom, R, binning, img, False, exact, E if rot is None else rot)


def state(out, n=P):
    R, _, _, geom, binning, img = out
    return introspect.State(n, W, H, R, geom, binning, img)


def colours(out, n=P):
    """(rgb [n,3], clamp bits [n]) of the visible Gaussians, zeros elsewhere"""
    st = state(out, n)
    vis = (out[2] > 0)
    return torch.where(vis[:, None], st.rgb, torch.zeros_like(st.rgb)).clone(), torch.where(vis, st.clamp_bits, torch.zeros_like(st.clamp_bits))


def same_forward(a, b):
    ca, cb = colours(a), colours(b)
    return torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(ca[0], cb[0]) and torch.equal(ca[1], cb[1])


def gpix_for(out, seed=3):
    g, _ = scenes.l1_target_grad(out[1].detach().cpu(), seed)
    return g.to(out[1].device)


# ---- 1. identity is a no-op --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ["ctypes", "ext"])
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_identity_rotations_change_no_bit(case, binding, exact, deg):
    ops = Hh.native_ops(binding)
    a = case.args(deg)
    eye = torch.eye(3, device=case.dev).repeat(P, 1, 1)
    plain, turned = forward(ops, a, None, exact), forward(ops, a, eye, exact)
    assert plain[0] == turned[0] and same_forward(plain, turned)
    assert int((plain[2] > 0).sum()) > P // 2
    gpix = gpix_for(plain)
    for name, g0, g1 in zip(Hh.GRAD_NAMES, backward(ops, a, plain, gpix, None, exact), backward(ops, a, turned, gpix, eye, exact)):
        assert torch.equal(g0, g1), name
    assert float(g1.abs().sum()) > 0


# ---- 2. colours against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("binding", ["ctypes", "ext"])
def test_colours_against_the_reference(gpu_device, binding):
    """The per-Gaussian colours and clamp bits of a fused forward on the fixture's 512 Gaussians: the clamp bits are the
    reference's, the values no farther from the float64 colours than 2 x the larger of (the reference's own float32
    colours, the kernel's colours WITHOUT rotations against unrotated float64 -- the arithmetic this kernel had before).
"""
    dev, ops = gpu_device, Hh.native_ops(binding)
    fx = np.load(os.path.join(GOLD, "sh_rotations.npz"))
    n = fx["positions"].shape[0]
    t = {k: torch.from_numpy(fx[k]) for k in ("positions", "campos", "shs", "sh_rotations")}
    cam = scenes.look_at_camera(t["campos"].double().tolist(), W, H, 110.0, 110.0)
    assert torch.equal(cam.campos, t["campos"])
    quats = torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(n, 1)
    for deg in range(4):
        a = (torch.zeros(3, device=dev), t["positions"].to(dev), E, torch.full((n, 1), 0.5, device=dev), torch.full((n, 3), 0.02, device=dev),
             quats.to(dev), 1.0, E, cam.viewmatrix.to(dev), cam.projmatrix.to(dev), cam.tanfovx, cam.tanfovy, H, W, t["shs"].to(dev), deg,
             cam.campos.to(dev), False, False)
        turned, plain = forward(ops, a, t["sh_rotations"].to(dev)), forward(ops, a, None)
        assert bool((turned[2] > 0).all()), "every Gaussian of the fixture is in front of its camera"
        rgb, bits = (x.cpu() for x in colours(turned, n))
        ref = torch.from_numpy(fx[f"rgb_deg{deg}"])
        k = (deg + 1) ** 2
        f64 = {k_: v.double() for k_, v in t.items()}
        want = sh.points_rgb(f64["positions"], f64["shs"][:, :k], f64["campos"], deg, f64["sh_rotations"])
        want_plain = sh.points_rgb(f64["positions"], f64["shs"][:, :k], f64["campos"], deg)
        ref_bits = ((ref == 0).int() * torch.tensor([1, 2, 4], dtype=torch.int32)).sum(-1)
        d_ours = float((rgb.double() - want).abs().max())
        d_ref = float((ref.double() - want).abs().max())
        d_plain = float((colours(plain, n)[0].cpu().double() - want_plain).abs().max())
        print(f"\n[{binding}] degree {deg}: d_ours {d_ours:.3e}  d_ref {d_ref:.3e}  d_plain {d_plain:.3e}")
        assert torch.equal(bits.int(), ref_bits.int()), deg
        assert d_ours <= 2.0 * max(d_ref, d_plain), (deg, d_ours, d_ref, d_plain)


# ---- 3. every SH form computes the same thing ---------------------------------------------------------------------------
class _Option:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = _lib.set_option(self.name, self.value)

    def __exit__(self, *exc):
        _lib.set_option(self.name, self.old)


def test_every_sh_form_gives_the_same_colours(case):
    from frosting_amd.rasterizer import _C
    a, rot = case.args(3), case.rot
    base = forward(_C, a, rot)
    assert not same_forward(base, forward(_C, a, None)), "the rotations must matter on this scene"
    assert same_forward(base, forward(Hh.native_ops("ext"), a, rot))
    for mode in range(4):      # frg_forward_args::async_sh 1 .. 4
        assert same_forward(base, _C.rasterize_gaussians(*a, modes={"async_sh": mode}, sh_rotations=rot)), mode
    for no_dir in (0, 1):
        with _Option("sh_dir_in_backward", no_dir):
            assert same_forward(base, forward(_C, a, rot)), no_dir
            assert same_forward(base, _C.rasterize_gaussians(*a, modes={"async_sh": 2}, sh_rotations=rot)), no_dir
    assert same_forward(base, forward(_C, a, rot, forward_only=True))
    # a keep mask of every third Gaussian: the waves fall below three quarters visible and take the rank layout
    masked = {}
    for sparse in (1, 0):
        with _Option("sparse_sh", sparse):
            masked[sparse] = forward(_C, a, rot, keep=case.keep)
            for mode in (0, 1):
                assert same_forward(masked[sparse], _C.rasterize_gaussians(*a, keep_mask=case.keep, modes={"async_sh": mode}, sh_rotations=rot))
            with _Option("sh_dir_in_backward", 1):
                assert same_forward(masked[sparse], forward(_C, a, rot, keep=case.keep))
    assert same_forward(masked[0], masked[1])
    vis = masked[1][2] > 0
    assert bool((masked[1][2][~case.keep] == 0).all()) and int(vis.sum()) > P // 8
    assert torch.equal(colours(masked[1])[0][vis], colours(base)[0][vis]) and torch.equal(colours(masked[1])[1][vis], colours(base)[1][vis])


def test_deferred_forward_and_truncated_storage(case):
    from frosting_amd.rasterizer import _C
    dev, a, rot = case.dev, case.args(3), case.rot
    base = forward(_C, a, rot)
    # the deferred forward (instance_capacity > 0)
    L = _lib.lib()
    geom, binning, img = (_lib.Scratch(dev) for _ in range(3))
    color = torch.empty((3, H, W), device=dev)
    radii = torch.empty((P,), dtype=torch.int32, device=dev)
    cap = 2 * base[0]
    fa = _lib.forward_args(geometry_alloc=geom.cb, binning_alloc=binning.cb, image_alloc=img.cb, P=P, D=3, M=16, background=a[0], width=W,
                           height=H, means3D=a[1], shs=a[14], opacities=a[3], scales=a[4], scale_modifier=1.0, rotations=a[5],
                           viewmatrix=a[8], projmatrix=a[9], cam_pos=a[16], tan_fovx=a[10], tan_fovy=a[11], prefiltered=0, out_color=color,
                           radii=radii, hip_stream=torch.cuda.current_stream(dev).cuda_stream, instance_capacity=cap, sh_rotations=rot)
    assert _lib.check(L.frg_forward_ex(C.byref(fa)), "frg_forward_ex") == cap
    n = C.c_int(0)
    _lib.check(L.frg_forward_finish(C.c_void_p(img.buf.data_ptr()), 0, C.byref(n)), "frg_forward_finish")
    assert n.value == base[0]
    assert same_forward(base, (cap, color, radii, geom.buf, binning.buf, img.buf))
    # truncated storage (D = 1, M = 4: the strided SH path) against M = 16 with zero padding
    short = case.sc.shs[:, :4].contiguous()
    padded = torch.cat([short, torch.zeros(P, 12, 3, device=dev)], dim=1).contiguous()
    for exact in (0, 1):
        o4, o16 = forward(_C, case.args(1, shs=short), rot, exact), forward(_C, case.args(1, shs=padded), rot, exact)
        assert same_forward(o4, o16)
        gpix = gpix_for(o4)
        g4, g16 = backward(_C, case.args(1, shs=short), o4, gpix, rot, exact), backward(_C, case.args(1, shs=padded), o16, gpix, rot, exact)
        for name, x, y in zip(Hh.GRAD_NAMES, g4, g16):
            assert torch.equal(x, y[:, :4] if name == "dL_dsh" else y), name
        assert not g16[5][:, 4:].any()


def test_raw_parameter_mode(case):
    """fused.rasterize_raw with sh_rotations: the SH pass sees the same centres and coefficients as the activated-tensor call,
    so the per-Gaussian colours and clamp bits are the same bits (the blend sees activations that differ by an ulp)."""
    from frosting_amd.rasterizer import _C
    dev, sc = case.dev, case.sc
    o = sc.opacities.double().clamp(1e-4, 1 - 1e-4)
    raw = [torch.log(o / (1 - o)).float().reshape(-1), torch.log(sc.scales.double()).float(), sc.rotations.clone()]
    leaves = [t.clone().requires_grad_(True) for t in [sc.shs] + raw + [sc.means3D]]
    rot = case.rot.clone().requires_grad_(True)
    img, radii = fused.rasterize_raw(Hh.settings_for(case.cam, case.bg, 3, dev), *leaves[:4], means3D=leaves[4], sh_rotations=rot)
    ctx = img.grad_fn
    geom, binning, im = ctx.bufs
    mine = (ctx.R, img.detach(), radii, geom.buf, binning.buf, im.buf)
    base = forward(_C, case.args(3), case.rot)
    both = (radii > 0) & (base[2] > 0)
    assert float((radii != base[2]).float().mean()) < 1e-3 and int(both.sum()) > P // 2
    assert torch.equal(colours(mine)[0][both], colours(base)[0][both]) and torch.equal(colours(mine)[1][both], colours(base)[1][both])
    assert float((img.detach() - base[1]).abs().mean()) < 2e-7
    img.backward(gpix_for(base))
    assert rot.grad is None and all(bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().sum()) > 0 for t in leaves)


# ---- 4. + 5. blend plumbing and gradients -----------------------------------------------------------------------------
def _expected_chain(case, deg, rot, g_c, g_means_geom):
    """dL/dc chained through float64 autograd of sh.points_rgb (whose clamp_min supplies the clamp mask) -> (dL_dsh, dL_dmeans3D)"""
    means = case.scene.means3D.double().requires_grad_(True)
    k = (deg + 1) ** 2
    shs = case.scene.shs[:, :k].double().requires_grad_(True)
    col = sh.points_rgb(means, shs, case.cam.campos.double(), deg, None if rot is None else rot.cpu().double())
    (col * g_c.cpu().double()).sum().backward()
    want_sh = torch.zeros(P, 16, 3, dtype=torch.float64)
    want_sh[:, :k] = shs.grad
    return want_sh, g_means_geom.cpu().double() + means.grad


def _chain_distances(case, ops, deg, exact, rot):
    """(fused forward + backward, the distances of its dL_dsh / dL_dmeans3D to the float64 chain, the colors_precomp call's gradients)"""
    a = case.args(deg)
    fwd = forward(ops, a, rot, exact)
    c = colours(fwd)[0].contiguous()
    ac = case.args(deg, colors=c)
    pre = forward(ops, ac, None, exact)
    assert torch.equal(pre[1], fwd[1]) and torch.equal(pre[2], fwd[2]), "the fused image is the colors_precomp image of the read-back colours"
    gpix = gpix_for(fwd)
    g, gp = backward(ops, a, fwd, gpix, rot, exact), backward(ops, ac, pre, gpix, None, exact)
    want_sh, want_means = _expected_chain(case, deg, rot, gp[1], gp[3])
    return fwd, g, gp, Hh.rel_l2(g[5].cpu(), want_sh), Hh.rel_l2(g[3].cpu(), want_means), gpix


@pytest.mark.parametrize("binding", ["ctypes", "ext"])
@pytest.mark.parametrize("exact", [0, 1])
def test_gradients_against_the_float64_chain(case, binding, exact):
    """dL_dsh and dL_dmeans3D of the fused backward against dL/dc (from a colors_precomp call on a bit-identical blend)
    chained through float64 autograd of points_rgb; the bar is 2 x the same construction's distance WITHOUT rotations (the
    SH backward as it was).  The other six gradient tensors are the colors_precomp call's, bit for bit."""
    ops = Hh.native_ops(binding)
    for deg in (3, 1):
        _, g, gp, d_sh, d_means, _ = _chain_distances(case, ops, deg, exact, case.rot)
        _, _, _, p_sh, p_means, _ = _chain_distances(case, ops, deg, exact, None)
        print(f"\n[{binding}, exact {exact}, degree {deg}] rel. L2 to the float64 chain: dL_dsh {d_sh:.3e} (unrotated {p_sh:.3e}), "
              f"dL_dmeans3D {d_means:.3e} (unrotated {p_means:.3e})")
        for i in (0, 1, 2, 4, 6, 7):
            assert torch.equal(g[i], gp[i]), Hh.GRAD_NAMES[i]
        assert float(g[5].abs().sum()) > 0
        assert d_sh <= 2.0 * p_sh, (deg, d_sh, p_sh)
        assert d_means <= 2.0 * p_means, (deg, d_means, p_means)


def _backward_ctypes(case, a, out, gpix, rot, exact, phase=0, row_live=None, work=None, outs=None):
    """frg_backward_ex with the fields the bindings do not pass (phase, row_live); outputs pre-zeroed -> (rc, outputs, workspace)"""
    L, dev = _lib.lib(), case.dev
    R, _, radii, geom, binning, img = out
    z = lambda *s: torch.zeros(s, device=dev)
    outs = outs or dict(dL_dmean2D=z(P, 3), dL_dopacity=z(P, 1), dL_dcolor=z(P, 3), dL_dmean3D=z(P, 3), dL_dcov3D=z(P, 6),
                        dL_dsh=z(P, 16, 3), dL_dscale=z(P, 3), dL_drot=z(P, 4))
    ws = int(L.frg_backward_workspace_bytes(P, R))
    work = work if work is not None else torch.empty(ws, dtype=torch.uint8, device=dev)
    b = _lib.backward_args(P=P, D=a[15], M=16, R=R, background=a[0], width=W, height=H, means3D=a[1], shs=a[14], scales=a[4], scale_modifier=1.0,
                           rotations=a[5], viewmatrix=a[8], projmatrix=a[9], campos=a[16], tan_fovx=a[10], tan_fovy=a[11], radii=radii,
                           geom_buffer=geom, binning_buffer=binning, image_buffer=img, dL_dpix=gpix, workspace=work, workspace_bytes=ws,
                           hip_stream=torch.cuda.current_stream(dev).cuda_stream, exact_blend=exact + 1, phase=phase, row_live=row_live,
                           sh_rotations=rot, **outs)
    rc = L.frg_backward_ex(C.byref(b))
    torch.cuda.synchronize(dev)
    return rc, outs, work


ORDER = ["dL_dmean2D", "dL_dcolor", "dL_dopacity", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot"]


def test_backward_forms_agree_bit_for_bit(case):
    """sh_dir_in_backward = 1, row_live and the two-call backward (phase 1 + 2) against the one-call fused backward"""
    from frosting_amd.rasterizer import _C
    a, rot = case.args(3), case.rot
    fwd = forward(_C, a, rot)
    gpix = gpix_for(fwd)
    one = backward(_C, a, fwd, gpix, rot)
    rc, outs, _ = _backward_ctypes(case, a, fwd, gpix, rot, 0)
    assert rc == 0, _lib.last_error()
    for k, g in zip(ORDER, one):
        assert torch.equal(outs[k], g), k
    with _Option("sh_dir_in_backward", 1):
        f2 = forward(_C, a, rot)
        assert same_forward(fwd, f2)
        for name, x, y in zip(Hh.GRAD_NAMES, one, backward(_C, a, f2, gpix, rot)):
            assert torch.equal(x, y), name
        rc, o_live, _ = _backward_ctypes(case, a, f2, gpix, rot, 0, row_live=torch.zeros(P, dtype=torch.uint8, device=case.dev))
        assert rc == 0, _lib.last_error()
    live = torch.zeros(P, dtype=torch.uint8, device=case.dev)
    rc, o_live2, _ = _backward_ctypes(case, a, fwd, gpix, rot, 0, row_live=live)
    assert rc == 0 and 0 < int(live.sum()) < P
    for k, g in zip(ORDER, one):
        assert torch.equal(o_live[k], g) and torch.equal(o_live2[k], g), k       # (the rows left unwritten are the zero rows)
    rc, o2, work = _backward_ctypes(case, a, fwd, gpix, rot, 0, phase=1)
    assert rc == 0, _lib.last_error()
    rc, o2, _ = _backward_ctypes(case, a, fwd, gpix, rot, 0, phase=2, work=work, outs=o2)
    assert rc == 0, _lib.last_error()
    for k, g in zip(ORDER, one):
        assert torch.equal(o2[k], g), k


# ---- 6. the stamp -------------------------------------------------------------------------------------------------------
def test_backward_needs_the_forwards_rotations(case):
    """A backward without sh_rotations on a rotated forward is refused, and the reverse: on the remembered buffers (the
    host's note) and on clones of them at another address (the stamp in the image chunk).  Refusals only: no kernel runs."""
    from frosting_amd.rasterizer import _C
    L, a, rot = _lib.lib(), case.args(3), case.rot
    turned, plain = forward(_C, a, rot), forward(_C, a, None)
    gpix = gpix_for(plain)

    arenas = []

    def clone(out):
        # copies at addresses no forward of this process has used -- inside a fresh 64 MiB block of its own, far from the block's
        # start -- so that the host has no note of them, not even a stale one: the stamp in the image chunk decides
        copies = []
        for t in out[3:]:
            arena = torch.empty(64 << 20, dtype=torch.uint8, device=case.dev)
            arenas.append(arena)
            off = 256 * 12347 - arena.data_ptr() % 256
            copies.append(arena[off:off + t.numel()].copy_(t))
        return out[:3] + tuple(copies)

    for out in (turned, clone(turned)):
        rc, _, _ = _backward_ctypes(case, a, out, gpix, None, 0)
        assert rc == -1 and "sh_rotations" in _lib.last_error() and "NULL" in _lib.last_error()
        for ops in (_C, Hh.native_ops("ext")):
            with pytest.raises(RuntimeError, match="sh_rotations"):
                backward(ops, a, out, gpix, None)
    for out in (plain, clone(plain)):
        rc, _, _ = _backward_ctypes(case, a, out, gpix, rot, 0)
        assert rc == -1 and "sh_rotations given" in _lib.last_error()
    # a note that disagrees with the buffers (the rotated forward's note, its buffers overwritten with the plain forward's) does
    # not refuse on its own: the stamp is read, and the stamp says "not rotated"
    stale = forward(_C, a, rot)
    for dst, src in zip(stale[3:], plain[3:]):
        assert dst.numel() >= src.numel()
        dst[:src.numel()].copy_(src)
    rc, o_stale, _ = _backward_ctypes(case, a, (plain[0], plain[1], plain[2]) + stale[3:], gpix, None, 0)
    assert rc == 0, _lib.last_error()
    for k, g in zip(ORDER, backward(_C, a, plain, gpix, None)):
        assert torch.equal(o_stale[k], g), k
    # ... and a stale note that AGREES with a wrong call lets it through the host; the per-Gaussian backward then finds the stamp
    # against its instantiation and writes zero rows, not gradients of the wrong directions
    rc, o_guard, _ = _backward_ctypes(case, a, (plain[0], plain[1], plain[2]) + stale[3:], gpix, rot, 0)
    assert rc == 0, _lib.last_error()
    assert not any(bool(o_guard[k].any()) for k in ORDER if k != "dL_dcolor")
    # and the matching calls go through, on the clones as well
    want = backward(_C, a, turned, gpix, rot)
    got = backward(_C, a, clone(turned), gpix, rot)
    assert all(torch.equal(x, y) for x, y in zip(want, got))
    # the view-parallel exchanges run the per-Gaussian chain without the matrices: they refuse a rotated forward's buffers
    drgb = torch.zeros(P, 3, device=case.dev)
    masked = torch.empty_like(drgb)
    rc = L.frg_sh_color_grad(P, _lib.ptr(turned[3]), _lib.ptr(turned[2]), _lib.ptr(drgb), _lib.ptr(masked), _lib.stream_ptr(case.dev))
    assert rc == -1 and "single-view" in _lib.last_error()
    rc = L.frg_sh_color_grad(P, _lib.ptr(plain[3]), _lib.ptr(plain[2]), _lib.ptr(drgb), _lib.ptr(masked), _lib.stream_ptr(case.dev))
    assert rc == 0, _lib.last_error()
    rc, _, work = _backward_ctypes(case, a, turned, gpix, rot, 0, phase=1)
    assert rc == 0, _lib.last_error()
    rc = L.frg_pack_sum_rows(P, turned[0], 0, P, _lib.ptr(work), work.numel(), None, None, None, None, 0.5, 0.5, W, H, 1.0, 3, None, 0, 0, None)
    assert rc == -1 and "single-view" in _lib.last_error()
    # the factor form of the SH gradient (dL_dsh == NULL) is the exchange's payload: refused with rotations
    outs = dict(dL_dmean2D=drgb.clone(), dL_dopacity=torch.zeros(P, 1, device=case.dev), dL_dcolor=drgb.clone(), dL_dmean3D=drgb.clone(),
                dL_dcov3D=torch.zeros(P, 6, device=case.dev), dL_dsh=None, dL_dscale=drgb.clone(), dL_drot=torch.zeros(P, 4, device=case.dev))
    rc, _, _ = _backward_ctypes(case, a, turned, gpix, rot, 0, outs=outs)
    assert rc == -1 and "single-view" in _lib.last_error()


def test_python_layer_carries_the_rotations(case):
    """GaussianRasterizer(..., sh_rotations=) of both packages: the autograd ctx hands the matrices to the backward."""
    import diff_gaussian_rasterization as d
    from frosting_amd.rasterizer import GaussianRasterizer, _C
    dev, sc = case.dev, case.sc
    settings = Hh.settings_for(case.cam, case.bg, 3, dev)
    base = forward(_C, case.args(3), case.rot)
    gpix = gpix_for(base)
    want = backward(_C, case.args(3), base, gpix, case.rot)
    for cls in (GaussianRasterizer, d.GaussianRasterizer):
        leaves = [t.clone().requires_grad_(True) for t in (sc.means3D, sc.shs, sc.opacities, sc.scales, sc.rotations)]
        rot = case.rot.transpose(1, 2).contiguous().transpose(1, 2).requires_grad_(True)      # not contiguous: the binding makes it so
        img, radii = cls(settings)(means3D=leaves[0], means2D=torch.zeros_like(leaves[0]), shs=leaves[1], opacities=leaves[2],
                                   scales=leaves[3], rotations=leaves[4], sh_rotations=rot)
        assert torch.equal(img.detach(), base[1]) and torch.equal(radii, base[2])
        img.backward(gpix)
        assert rot.grad is None
        assert torch.equal(leaves[0].grad, want[3]) and torch.equal(leaves[1].grad, want[5]) and torch.equal(leaves[4].grad, want[7])
        with torch.no_grad():
            img2, _ = cls(settings)(means3D=sc.means3D, means2D=torch.zeros_like(sc.means3D), shs=sc.shs, opacities=sc.opacities,
                                    scales=sc.scales, rotations=sc.rotations, sh_rotations=case.rot, keep_mask=case.keep)
        assert torch.equal(img2, forward(_C, case.args(3), case.rot, keep=case.keep)[1])
