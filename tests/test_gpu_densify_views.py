"""Densification statistics of every view of a view-parallel step from the slot-sum packets (frg_pack_sum_rows_ex's
visibility section + frg_densify_accumulate_views; SlotSumExchange / ViewParallelRasterizer with densify=).

One process plays every rank, as tests/test_gpu_parallel.py does for the combine pass.  The yardstick is the one-view launch
that exists since adaptive density control: after each view's ONE-CALL backward, frg_densify_accumulate on that view's own
radii and dL_dmeans2D, on zero-initialised tensors, in view order.  The statistics the packets give must be the same bits.
"""
import functools
import os
import socket
import types

import pytest
import torch

from frosting_amd import _lib, scenes
from frosting_amd.densify import DensityControl, native_ops
from frosting_amd.optim import FlatAdam
from frosting_amd.parallel import PARAM_ORDER, SlotSumExchange, ViewParallelRasterizer, sum_packet_words

pytestmark = pytest.mark.gpu

STATS = ("xyz_gradient_accum", "denom", "max_radii2D")
LRS = dict(means3D=1.6e-4, scales=5e-3, rotations=1e-3, opacities=5e-2, shs=2.5e-3)

#        name    P        views                 chunks degree raw    always cull
CASES = {"mini": ("mini", 4807, [0, 3, 5, 6], 3, 1, False, False),      # the last partial block of 64, a chunk boundary inside it
         "c2": ("c2", 50_000, [0, 1, 2, 4], 2, 3, True, False),
         "c3": ("c3", 150_000, list(range(8)), 2, 3, False, False),
         "single": ("mini", 5000, [2], 1, 3, False, True)}


def _holder(P, dev, fill=0.0, binding=None):
    """Any object with the three statistic tensors (what SlotSumExchange(densify=...) takes)."""
    h = types.SimpleNamespace(xyz_gradient_accum=torch.full((P, 1), fill, dtype=torch.float32, device=dev),
                              denom=torch.full((P, 1), fill, dtype=torch.float32, device=dev),
                              max_radii2D=torch.full((P,), fill, dtype=torch.float32, device=dev))
    if binding:
        h.ops = native_ops(binding)
    return h


def _same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in STATS)


def _scene(name, P, degree=3, raw=False):
    scene, _, _ = scenes.config_scene(name, 0, P=P)
    scene.sh_degree = degree
    if raw:
        scene = scenes.Scene(scene.means3D, torch.log(scene.scales), scene.rotations * 1.7, torch.log(scene.opacities / (1 - scene.opacities)),
                             scene.shs, degree)
    return scene


def _camera(name, view):
    cfg = scenes.CONFIGS[name]
    return scenes.ring_camera(view, cfg["width"], cfg["height"], cfg["fx"], cfg["fy"]), torch.tensor(cfg["bg"], dtype=torch.float32)


def _slot_sum_views(vpr, name, views, dev, yard, cull=None, world=None, seed0=555):
    """tests/test_gpu_parallel.py's helper of the same name -- per view the one-call backward (the reference gradient of that
    view) and, from the same forward, phase 1 + the view's packets where an all-gather would have put them -- plus the
    yardstick: frg_densify_accumulate on the view's own radii and viewspace gradient, into `yard`.
    cull: keep_mask of every forward (None: decided by the first view -- every seventh Gaussian is dropped if it saw them all).
    -> (accumulated gradients, per view (visible, radii > 0 as bool))"""
    ex = vpr.exchange
    world = world or len(views)
    acc = {n: torch.zeros_like(ex.views[n]) for n in PARAM_ORDER}
    seen = []
    accumulate = native_ops("ctypes").densify_accumulate
    for slot_v, k in enumerate(views):
        cam, bg = _camera(name, k)
        cam, bg = cam.to(dev), bg.to(dev)
        img, radii = vpr.forward(cam, bg, keep_mask=cull)
        if cull is None and slot_v == 0 and bool((radii > 0).all()):
            cull = (torch.arange(vpr.P, device=dev) % 7 != 0).to(torch.uint8)
            img, radii = vpr.forward(cam, bg, keep_mask=cull)
        gpix, _ = scenes.l1_target_grad(img.cpu(), seed0 + k)
        gpix = gpix.to(dev)
        g = vpr.backward(gpix, 0)                               # every gradient of this view, one call
        for n in PARAM_ORDER:
            acc[n] += g[n]
        accumulate(vpr.radii, vpr.dL_dmeans2D, torch.empty(0, dtype=torch.uint8, device=dev), yard.xyz_gradient_accum, yard.denom,
                   yard.max_radii2D)
        seen.append(vpr.radii > 0)
        vpr.backward(gpix, 0, slot_sums=True)                   # phase 1 only: the nine sums + their bit mask in the workspace
        ex.pack_local_view(slot_v, world)
    return acc, seen, cull


@functools.lru_cache(maxsize=None)
def _run(case, steps=1, binding=None):
    """One case through the packets (`steps` steps in a row into the same statistics) and through the yardstick; everything the
    tests look at, computed once."""
    name, P, views, chunks, degree, raw, always_cull = CASES[case]
    dev = torch.device("cuda:0")
    got, yard = _holder(P, dev, binding=binding), _holder(P, dev)
    vpr = ViewParallelRasterizer(_scene(name, P, degree, raw).to(dev), dev, slotsum=True, chunks=chunks, raw_params=raw, densify=got)
    ex = vpr.exchange
    assert isinstance(ex, SlotSumExchange) and len(ex.chunks) == chunks and ex.densify is got
    cull = (torch.arange(P, device=dev) % 7 != 0).to(torch.uint8) if always_cull else None
    out = None
    for step in range(steps):
        acc, seen, cull = _slot_sum_views(vpr, name, views, dev, yard, cull=cull, seed0=555 + 100 * step)
        for t in ex.views.values():
            t.fill_(float("nan"))
        verdicts = ex.combine_local(len(views))
        torch.cuda.synchronize(dev)
        assert not any(over for over, _ in verdicts)
        rows = [sum(counts[v] for _, counts in verdicts) for v in range(len(views))]
        # the mask words of every view, unpacked: which Gaussians have a row
        live = []
        for v in range(len(views)):
            bits = []
            for c, (first, n) in enumerate(ex.chunks):
                nblk = (n + 63) // 64
                words = ex.packets_all[c][v, 64:64 + 2 * nblk].contiguous().view(torch.int64)
                b = (words[:, None] >> torch.arange(64, device=dev)[None, :]) & 1
                bits.append(b.reshape(-1)[:n].bool())
            live.append(torch.cat(bits))
        out = dict(got=got, yard=yard, rows=rows, seen=seen, live=live, grads={n: ex.views[n].clone() for n in PARAM_ORDER}, acc=acc,
                   culled=cull is not None, status=[int(s[0]) for s in ex.stats_status], seqs=list(ex.stats_seq), P=P, views=views)
    return out


# ---- 1. bit equality ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_statistics_from_the_packets_equal_the_per_view_launches_bit_for_bit(gpu_device, case):
    r = _run(case)
    P = r["P"]
    # the inputs hold all three kinds of Gaussian in every view: with a row, visible without one, not visible
    for v in range(len(r["views"])):
        visible = int(r["seen"][v].sum())
        assert 0 < r["rows"][v] < visible < P, (v, r["rows"][v], visible)
        assert int(r["live"][v].sum()) == r["rows"][v] and bool((r["live"][v] <= r["seen"][v]).all())
    if case == "single":
        assert r["culled"] and not bool(r["seen"][0][::7].any())            # the wire carried the culling
    got, yard = r["got"], r["yard"]
    for k in STATS:
        assert float(getattr(yard, k).abs().max()) > 0
        assert torch.equal(getattr(got, k), getattr(yard, k)), k
    rows_somewhere = torch.stack(r["live"]).sum(0).to(torch.float32)
    assert bool((got.denom[:, 0] > rows_somewhere).any())                    # denom counts the visible, not the rows
    no_row = ~torch.stack(r["live"]).any(0)
    assert bool((got.max_radii2D[no_row] > 0).any())                         # a radius where no view has a row
    assert bool((got.denom[:, 0] == 0).any()) or len(r["views"]) > 1         # (single view: some Gaussian is seen by none)
    # the pass posted its word: accumulated, not refused
    assert all((w >> 32) == s and (w & 0xffffffff) == 0 for w, s in zip(r["status"], r["seqs"]))


# ---- 2. repeated steps -------------------------------------------------------------------------------------------------------
def test_two_steps_in_a_row_equal_two_rounds_of_the_per_view_launches(gpu_device):
    r = _run("mini", steps=2)
    assert _same(r["got"], r["yard"])
    one = _run("mini")
    assert bool((r["got"].denom == 2 * one["got"].denom).all()) and not torch.equal(r["got"].xyz_gradient_accum, one["got"].xyz_gradient_accum)


# ---- 3. default packets unchanged --------------------------------------------------------------------------------------------
def test_packets_without_densify_are_the_parents_byte_for_byte(gpu_device):
    """frg_pack_sum_rows_ex with radii = NULL writes what frg_pack_sum_rows writes; header word 6 is 0 there and the section's
    offset with radii; the rows, masks and bases in front of the section are the same bytes either way; sizes as the formulas say."""
    import ctypes as C
    dev = gpu_device
    L = _lib.lib()
    P = 4807
    for n, cap in ((1, 0), (64, 64), (65, 7), (4807, 1000), (1_500_000, 204_800)):
        nblk = (n + 63) // 64
        assert 4 * sum_packet_words(n, cap) == L.frg_sum_packet_bytes(n, cap) == L.frg_sum_packet_bytes_ex(n, cap, 0)
        assert 4 * sum_packet_words(n, cap, True) == L.frg_sum_packet_bytes_ex(n, cap, 1)
        assert 0 <= L.frg_sum_packet_bytes_ex(n, cap, 1) - L.frg_sum_packet_bytes(n, cap) - 8 * nblk < 16
    vpr = ViewParallelRasterizer(_scene("mini", P).to(dev), dev, slotsum=True, chunks=1)
    ex = vpr.exchange
    assert ex.densify is None and ex.wire_floats_per_rank == sum_packet_words(P, P)
    cam, bg = _camera("mini", 3)
    img, _ = vpr.forward(cam.to(dev), bg.to(dev))
    gpix, _ = scenes.l1_target_grad(img.cpu(), 9)
    vpr.backward(gpix.to(dev), 0, slot_sums=True)
    ex.pack_local_view(0, 1)                                                     # the parent's call: frg_pack_sum_rows
    torch.cuda.synchronize(dev)
    parent = ex.packets_all[0][0].clone()
    assert parent.numel() == sum_packet_words(P, P) and int(parent[6]) == 0 and int(parent[0]) > 0
    c, camd = ex.view_ctx, cam.to(dev)

    def pack_ex(radii, words, fill):
        dest = torch.full((words,), fill, dtype=torch.int32, device=dev)
        a = _lib.PackSumArgs(struct_size=C.sizeof(_lib.PackSumArgs), P=P, R=int(c["R"]), first=0, count=P, workspace=c["work"].data_ptr(),
                             workspace_bytes=c["work"].numel(), drgb_masked=ex.own_drgb.data_ptr(), viewmatrix=camd.viewmatrix.data_ptr(),
                             projmatrix=camd.projmatrix.data_ptr(), campos=camd.campos.data_ptr(), tan_fovx=float(cam.tanfovx),
                             tan_fovy=float(cam.tanfovy), width=int(cam.image_width), height=int(cam.image_height), scale_modifier=1.0,
                             D=3, packet=dest.data_ptr(), packet_bytes=4 * words, capacity_rows=P,
                             radii=None if radii is None else radii.data_ptr(), hip_stream=torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(L.frg_pack_sum_rows_ex(C.byref(a)), "frg_pack_sum_rows_ex")
        torch.cuda.synchronize(dev)
        return dest

    # (the rows beyond the packed ones are not written by either call: both start from the same fill)
    base = torch.zeros_like(parent)
    ex.packer(ex, 0, base)
    plain = pack_ex(None, parent.numel(), 0)
    assert torch.equal(plain, base) and torch.equal(plain, parent)
    words = sum_packet_words(P, P, True)
    with_vis = pack_ex(vpr.radii, words, 0)
    at = int(with_vis[6])
    assert at == parent.numel() and at % 4 == 0 and words - at >= 2 * ((P + 63) // 64)
    assert torch.equal(with_vis[:6], parent[:6]) and torch.equal(with_vis[7:at], parent[7:])
    vis = with_vis[at:at + 2 * ((P + 63) // 64)].contiguous().view(torch.int64)
    bits = ((vis[:, None] >> torch.arange(64, device=dev)[None, :]) & 1).reshape(-1)
    assert torch.equal(bits[:P].bool(), vpr.radii > 0) and not bool(bits[P:].any())
    # a packet too small for the section is refused by the host
    a_small = torch.zeros(parent.numel(), dtype=torch.int32, device=dev)
    ex.densify = _holder(P, dev)
    with pytest.raises(RuntimeError, match="packet: need"):
        ex.packer(ex, 0, a_small)


# ---- 4. gradients unchanged --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["c2", "mini"])
def test_combine_pass_gradients_are_unchanged_by_the_visibility_section(gpu_device, case):
    r = _run(case)
    for n in PARAM_ORDER:
        assert float(r["acc"][n].abs().max()) > 0
        assert torch.equal(r["grads"][n], r["acc"][n]), n


# ---- 5. overflow -------------------------------------------------------------------------------------------------------------
def test_overflowed_packets_leave_the_statistics_untouched_and_count_once_after_the_repack(gpu_device):
    """The scenario of test_slot_sum_packets_report_an_overflow_and_fit_after_it: chunk 0's packets too small for their fullest
    view.  combine_local accumulates the clean chunk only; the statistics pass itself, run on the overflowed packets, writes
    nothing and says so in its status word; after the repack the chunk is counted once."""
    dev = gpu_device
    P, views = 20_000, [0, 1, 2]
    got, yard = _holder(P, dev), _holder(P, dev)
    vpr = ViewParallelRasterizer(_scene("mini", P).to(dev), dev, slotsum=True, chunks=2, densify=got)
    ex = vpr.exchange
    _, _, cull = _slot_sum_views(vpr, "mini", views, dev, yard)
    (o0, c0), (o1, c1) = ex.combine_local(len(views))
    torch.cuda.synchronize(dev)
    assert not o0 and not o1 and _same(got, yard)
    SENTINEL = -7.5
    for k in STATS:
        getattr(got, k).fill_(SENTINEL)
    ex.capacity = [max(c0) - 5, max(c1) + 3]                     # chunk 0: too small for its fullest view; chunk 1: just enough
    ex.packets_all = [None, None]
    scratch = _holder(P, dev)
    _slot_sum_views(vpr, "mini", views, dev, scratch, cull=cull)
    (o0, _), (o1, _) = ex.combine_local(len(views))
    assert o0 and not o1
    # the pass itself on the overflowed chunk: refused, nothing written
    seq = 4242
    ex.accumulator(ex, 0, ex.packets_all[0], len(views), seq)
    torch.cuda.synchronize(dev)
    assert int(ex.stats_status[0][0]) == (seq << 32 | 1)
    first1 = ex.chunks[1][0]
    for k in STATS:
        t = getattr(got, k).reshape(-1)
        assert bool((t[:first1] == SENTINEL).all()), k           # chunk 0: untouched
        assert bool((t[first1:] != SENTINEL).any()), k           # chunk 1: accumulated by combine_local
    # a packet whose header names no visibility section (word 6 = 0, what frg_pack_sum_rows writes): the device refuses the launch
    marked = {k: getattr(got, k).clone() for k in STATS}
    keep = ex.packets_all[1].clone()
    ex.packets_all[1][1, 6] = 0
    ex.accumulator(ex, 1, ex.packets_all[1], len(views), seq + 1)
    torch.cuda.synchronize(dev)
    assert int(ex.stats_status[1][0]) == ((seq + 1) << 32 | 1) and all(torch.equal(getattr(got, k), marked[k]) for k in STATS)
    ex.packets_all[1].copy_(keep)
    # ... and the host refuses packets too short to hold one
    n1 = ex.chunks[1][1]
    with pytest.raises(RuntimeError, match="visibility section"):
        ex.accumulator(ex, 1, torch.zeros((len(views), sum_packet_words(n1, ex.capacity[1])), dtype=torch.int32, device=dev), len(views), seq + 2)
    # repack chunk 0 with room, from zeroed statistics: the yardstick, every chunk counted once
    for k in STATS:
        getattr(got, k).zero_()
    ex.capacity[0] = max(c0)
    ex.packets_all[0] = None
    ex.stats_seq = [0, 0]                                        # (the refusals above were asked for by this test)
    _slot_sum_views(vpr, "mini", views, dev, scratch, cull=cull)
    (o0, _), (o1, _) = ex.combine_local(len(views))
    torch.cuda.synchronize(dev)
    assert not o0 and not o1 and _same(got, yard)
    # more than 16 views: refused by the host
    with pytest.raises(RuntimeError, match="1..16 views"):
        ex.accumulator(ex, 1, ex.packets_all[1][:1].expand(17, -1).contiguous(), 17, seq + 3)


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_train_densify_adopt_and_train_on_a_single_rank_rccl_group(gpu_device):
    """render, backward, exchange (statistics included), twice; densify_and_prune with recorded noise; adopt_scene; one more
    step: its gradients are those of a freshly constructed ViewParallelRasterizer on the resized model, bit for bit."""
    import torch.distributed as dist
    dev = gpu_device
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        P = 6000
        raw = _scene("mini", P, 3, raw=True).to(dev)
        shapes = dict(means3D=(P, 3), scales=(P, 3), rotations=(P, 4), opacities=(P, 1), shs=(P, 16, 3))
        opt = FlatAdam(shapes, LRS, dev)
        for k in PARAM_ORDER:
            opt.params[k].copy_(getattr(raw, k).reshape(shapes[k]))
        dc = DensityControl(opt)
        as_scene = lambda p: scenes.Scene(p["means3D"], p["scales"], p["rotations"], p["opacities"], p["shs"], 3)
        vpr = ViewParallelRasterizer(as_scene(opt.params), dev, process_group=dist.group.WORLD, slotsum=True, raw_params=True, densify=dc)
        yard = _holder(P, dev)
        accumulate = native_ops("ctypes").densify_accumulate
        one_view = ViewParallelRasterizer(as_scene(opt.params), dev, raw_params=True)

        def step(v, view, seed):
            cam, bg = _camera("mini", view)
            cam, bg = cam.to(dev), bg.to(dev)
            img, _ = v.forward(cam, bg)
            gpix, _ = scenes.l1_target_grad(img.cpu(), seed)
            v.backward(gpix.to(dev), 0)
            if v is one_view:
                return None
            return v.exchange_in_step(0)

        for it, view in enumerate((2, 5)):
            step(vpr, view, 77 + it)
            step(one_view, view, 77 + it)
            accumulate(one_view.radii, one_view.dL_dmeans2D, torch.empty(0, dtype=torch.uint8, device=dev), yard.xyz_gradient_accum,
                       yard.denom, yard.max_radii2D)
        torch.cuda.synchronize(dev)
        assert _same(dc, yard) and float(dc.denom.max()) == 2.0 and float(dc.xyz_gradient_accum.max()) > 0
        assert not bool(vpr.dL_dmeans2D.any())                   # never written on this plan: zeros, not uninitialised memory
        # densify: a threshold that selects some rows; recorded noise
        grads = (dc.xyz_gradient_accum / dc.denom).nan_to_num(0.0)
        max_grad = float(grads[grads > 0].median())
        noise = torch.randn((P, 2, 3), generator=torch.Generator().manual_seed(3)).to(dev)
        params, sizes = dc.densify_and_prune(max_grad, 0.005, 4.0, None, noise=noise)
        P2 = sizes["total"]
        assert P2 != P and sizes["cloned"] + sizes["split_first"] > 0
        with pytest.raises(RuntimeError, match="adopt_scene"):   # the exchange still has the old size
            step(vpr, 3, 99)
        vpr.exchanges[0]._works = []
        vpr.adopt_scene(as_scene(params))
        assert vpr.P == P2 and vpr.radii.numel() == P2 and tuple(vpr.dL_dmeans2D.shape) == (P2, 3)
        assert [ex.P for ex in vpr.exchanges] == [P2, P2] and vpr.exchanges[0].capacity == [n for _, n in vpr.exchanges[0].chunks]
        flat = step(vpr, 3, 99).clone()
        fresh = ViewParallelRasterizer(as_scene(params), dev, process_group=dist.group.WORLD, slotsum=True, raw_params=True)
        want = step(fresh, 3, 99).clone()
        torch.cuda.synchronize(dev)
        assert float(want.abs().max()) > 0 and torch.equal(flat, want)
        assert tuple(dc.denom.shape) == (P2, 1) and tuple(dc.max_radii2D.shape) == (P2,) and float(dc.denom.max()) == 1.0
        assert int((dc.denom > 0).sum()) == int((vpr.radii > 0).sum())
    finally:
        dist.destroy_process_group()


# ---- 7. both bindings --------------------------------------------------------------------------------------------------------
def test_the_extension_binding_gives_the_same_bits_as_ctypes(gpu_device):
    a, b = _run("mini"), _run("mini", binding="ext")
    assert b["got"].ops is native_ops("ext") and _same(a["got"], b["got"]) and _same(b["got"], b["yard"])
