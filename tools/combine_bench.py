"""The local terms of the slot-sum exchange on ONE GPU: eight views of the C3 scene are rendered one
after the other, phase 1 of each backward leaves its sums, the views' packets are packed where an all-gather would put them,
and the combine pass (frg_backward_combine) runs over all of them -- timed with HIP events:

    one-call backward | phase 1 alone | pack (scan + rows) | combine of N views | the rows each view wanted

and the combined gradient is checked against the accumulation of the eight one-call gradients (bit for bit).
--densify: the packets carry their visibility sections and the statistics pass (frg_densify_accumulate_views) is timed over all
chunks, beside what one GPU needs for the same result without it -- one frg_densify_accumulate launch per view on that view's
dense radii and dL_dmeans2D (kept from the one-call backwards) -- and checked against it (bit for bit).
`python tools/combine_bench.py [--config c3] [--views 8] [--chunks 2] [--points N] [--densify]`; prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from frosting_amd import scenes                                          # noqa: E402
from frosting_amd.parallel import PARAM_ORDER, ViewParallelRasterizer    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--points", type=int, default=0)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--chunks", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-check", action="store_true")
    ap.add_argument("--densify", action="store_true", help="packets with visibility sections; time the statistics pass")
    ap.add_argument("--option", action="append", default=[], help="name=value for frg_set_option")
    ap.add_argument("--side-copy", type=int, default=0,
                    help="workgroups of a copy kernel (tools/micro/side_copy.hip) that streams 7 packets' worth of bytes on a side stream "
                         "WHILE the combine pass runs: a stand-in for incoming all-gather traffic -- reports the pass's time beside it")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    from frosting_amd import _lib
    for kv in a.option:
        k, v = kv.split("=")
        _lib.set_option(k, int(v))
    cfg = scenes.CONFIGS[a.config]
    P = a.points or cfg["P"]
    scene, _, bg = scenes.config_scene(a.config, 0, P=P)
    import types
    stats = lambda: types.SimpleNamespace(xyz_gradient_accum=torch.zeros((P, 1), device=dev), denom=torch.zeros((P, 1), device=dev),
                                          max_radii2D=torch.zeros(P, device=dev))
    holder = stats() if a.densify else None
    vpr = ViewParallelRasterizer(scene.to(dev), dev, slotsum=True, chunks=a.chunks, densify=holder)
    ex = vpr.exchange
    per_view = []                      # --densify: every view's radii and viewspace gradient, as the one-call backward leaves them
    bg_d = bg.to(dev)
    cams = [scenes.ring_camera(v, cfg["width"], cfg["height"], cfg["fx"], cfg["fy"]).to(dev) for v in range(a.views)]
    ev = lambda: torch.cuda.Event(enable_timing=True)
    acc = {n: torch.zeros_like(ex.views[n]) for n in PARAM_ORDER}
    t_one, t_p1, t_pack, gpixs = [], [], [], []
    for rep in range(2):               # the second round is the one that counts (arenas sized, packets at the capacity the first asked for)
        if rep == 1:
            verdicts = ex.combine_local(a.views)
            counts = [sum(c[v] for _, c in verdicts) for v in range(a.views)]
            ex.capacity = [min(n, (int(max(c) * 1.25) // 256 + 1) * 256) for (_, n), (_, c) in zip(ex.chunks, verdicts)]
            ex.packets_all = [None] * len(ex.chunks)
            for n in PARAM_ORDER:
                acc[n].zero_()
            t_one, t_p1, t_pack = [], [], []
        for v, cam in enumerate(cams):
            img, _ = vpr.forward(cam, bg_d)
            if rep == 0:
                g, _ = scenes.l1_target_grad(img.cpu(), 20241022 + v)
                gpixs.append(g.to(dev))
            e = [ev() for _ in range(6)]
            e[0].record(); grads = vpr.backward(gpixs[v], 0); e[1].record()
            for n in PARAM_ORDER:
                acc[n] += grads[n]
            if a.densify and rep == 1:
                per_view.append((vpr.radii.clone(), vpr.dL_dmeans2D.clone()))
            e[2].record(); vpr.backward(gpixs[v], 0, slot_sums=True); e[3].record()
            e[4].record(); ex.pack_local_view(v, a.views); e[5].record()
            torch.cuda.synchronize(dev)
            t_one.append(e[0].elapsed_time(e[1])); t_p1.append(e[2].elapsed_time(e[3])); t_pack.append(e[4].elapsed_time(e[5]))
    for t in ex.views.values():
        t.fill_(float("nan"))
    if a.densify:                      # (the first round's packets were accumulated too: the check below is about this round's)
        for t in vars(holder).values():
            t.zero_()
    verdicts = ex.combine_local(a.views)
    torch.cuda.synchronize(dev)
    ok = None
    if not a.no_check:
        ok = all(torch.equal(ex.views[n], acc[n]) for n in PARAM_ORDER) and not any(o for o, _ in verdicts)
    dens = None
    if a.densify:
        from frosting_amd.densify import native_ops
        one_view = native_ops("ctypes").densify_accumulate
        none = torch.empty(0, dtype=torch.uint8, device=dev)
        want = stats()
        for radii, g2d in per_view:
            one_view(radii, g2d, none, want.xyz_gradient_accum, want.denom, want.max_radii2D)
        torch.cuda.synchronize(dev)
        same = all(torch.equal(getattr(holder, k), getattr(want, k)) for k in ("xyz_gradient_accum", "denom", "max_radii2D"))
        t_views, t_each = [], []
        for _ in range(a.iters):
            e0, e1, e2 = ev(), ev(), ev()
            e0.record()
            for c in range(len(ex.chunks)):
                ex.accumulator(ex, c, ex.packets_all[c], a.views, 1)
            e1.record()
            for radii, g2d in per_view:
                one_view(radii, g2d, none, want.xyz_gradient_accum, want.denom, want.max_radii2D)
            e2.record()
            torch.cuda.synchronize(dev)
            t_views.append(e0.elapsed_time(e1)); t_each.append(e1.elapsed_time(e2))
        plain = 4 * ex.wire_floats_per_rank
        ex.densify = None              # (the combine pass alone below; the packets keep their sections: it ignores them)
        dens = {"statistics_from_packets_ms": statistics.median(t_views), "one_launch_per_view_on_dense_tensors_ms": statistics.median(t_each),
                "equal_bit_for_bit": same, "visible_per_view": [int((r > 0).sum()) for r, _ in per_view],
                "visibility_bytes_per_view": sum(((n + 63) // 64) * 8 for _, n in ex.chunks), "packet_bytes_per_view_with_sections": plain}
    t_cmb = []
    for _ in range(a.iters):
        e0, e1 = ev(), ev()
        e0.record(); ex.combine_local(a.views); e1.record()
        torch.cuda.synchronize(dev)
        t_cmb.append(e0.elapsed_time(e1))
    med = statistics.median
    side = None
    if a.side_copy > 0:
        import ctypes as C
        lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "micro", "libside_copy.so"))
        lib.side_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        nbytes = 7 * 4 * ex.wire_floats_per_rank // 16 * 16
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        s2 = torch.cuda.Stream(dev)
        t_alone, t_cmb2, t_copy = [], [], []
        for rep in range(a.iters):                     # the copy alone (its rate), then the combine pass beside it
            c0, c1 = ev(), ev()
            torch.cuda.synchronize(dev)
            with torch.cuda.stream(s2):
                c0.record(s2); lib.side_copy(src.data_ptr(), dst.data_ptr(), nbytes, a.side_copy, 1, s2.cuda_stream); c1.record(s2)
            torch.cuda.synchronize(dev)
            t_alone.append(c0.elapsed_time(c1))
            e0, e1, c0, c1 = ev(), ev(), ev(), ev()
            with torch.cuda.stream(s2):
                c0.record(s2); lib.side_copy(src.data_ptr(), dst.data_ptr(), nbytes, a.side_copy, 2, s2.cuda_stream); c1.record(s2)
            e0.record(); ex.combine_local(a.views); e1.record()
            torch.cuda.synchronize(dev)
            t_cmb2.append(e0.elapsed_time(e1)); t_copy.append(c0.elapsed_time(c1))
        side = {"workgroups": a.side_copy, "bytes": nbytes, "copy_alone_ms": med(t_alone), "copy_alone_GBps": nbytes / med(t_alone) / 1e6,
                "combine_beside_copy_ms": med(t_cmb2), "copy_of_twice_the_bytes_beside_combine_ms": med(t_copy),
                "combine_slowdown": med(t_cmb2) / med(t_cmb)}
    live = int(((acc["opacities"] != 0).reshape(P, -1).any(1) | (acc["means3D"] != 0).any(1)).sum())
    print(json.dumps({"config": a.config, "P": P, "views": a.views, "chunks": a.chunks, "rows_wanted_per_view": counts,
                      "rows_fraction": max(counts) / P, "gaussians_with_a_row_in_some_view": live, "capacity_rows": sum(ex.capacity),
                      "packet_bytes_per_view": 4 * ex.wire_floats_per_rank, "backward_one_call_ms": med(t_one), "backward_phase1_ms": med(t_p1),
                      "pack_ms": med(t_pack), "combine_ms": med(t_cmb), "combine_ms_all": [round(x, 4) for x in t_cmb],
                      "combine_equals_accumulation_bit_for_bit": ok, "side_copy": side, "densify": dens}))


if __name__ == "__main__":
    main()
