"""CPU tier of the densification statistics on the slot-sum plan (frosting_amd.parallel.SlotSumExchange(densify=...),
ViewParallelRasterizer.adopt_scene): two gloo ranks, torch stand-ins for the three HIP hooks (packer, combiner, accumulator)
that write and read the product's packet layout, visibility section included.  What is checked here is the Python layer: the
packets are sized with the section, note_view's radii reach the packer, the accumulator hook runs exactly once per chunk and
step -- also in a step whose packets overflow and are packed again --, every rank ends with the same statistics, equal to the
per-view formula evaluated in one process, and adopt_scene refuses ranks that disagree about the model's size.
"""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from frosting_amd.parallel import PARAM_ORDER, SUM_HDR_WORDS, SUM_ROW_FLOATS, sum_packet_words

MAGIC = 0x46534d36


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _params(P, K):
    g = torch.Generator().manual_seed(11)
    shapes = dict(means3D=(P, 3), scales=(P, 3), rotations=(P, 4), opacities=(P, 1), shs=(P, K, 3))
    return shapes, {k: torch.randn(shapes[k], generator=g) for k in PARAM_ORDER}


def _view(params, view, it, P):
    """Phase 1 of view `view` in step `it`: twelve sums per Gaussian (zero rows where no pixel reached: one Gaussian in four in
    the first two steps, three in four in the third -- the packets sized from the earlier steps then overflow) and the view's
    radii: positive on the Gaussians with sums and on some more, zero elsewhere."""
    base = torch.cat([params["means3D"], params["scales"], params["rotations"][:, :3], params["shs"][:, 1, :]], 1)     # [P, 12]
    S = base * (0.25 + 0.125 * view) + 0.0625 * (1 + it)
    i = torch.arange(P)
    reached = (i * 7 + 3 * view) % 4 == 0 if it < 2 else (i * 7 + 3 * view) % 4 != 0
    S[~reached] = 0.0
    visible = reached | ((i * 5 + view) % 3 != 0)
    radii = torch.where(visible, _radius(params, view), torch.zeros(P)).to(torch.int32)
    return S, radii


def _radius(params, view):
    """The stand-in for the radius every rank recomputes from the replicated parameters and the view's camera."""
    return torch.ceil(params["scales"].abs().sum(1) * (2 + view)) + 1.0


def _layout(n, cap):
    nblk = (n + 63) // 64
    b_at = SUM_HDR_WORDS + 2 * nblk
    r_at = (b_at + nblk + 3) // 4 * 4
    v_at = (r_at + SUM_ROW_FLOATS * cap + 3) // 4 * 4
    return nblk, b_at, r_at, v_at


def _bits_to_words(bits, nblk):
    padded = np.zeros(nblk * 64, dtype=bool)
    padded[:bits.size] = bits
    return np.packbits(padded.reshape(nblk, 64), axis=1, bitorder="little").view(np.uint64).reshape(nblk), padded


def _words_to_bits(words, n):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(-1, 8), axis=1, bitorder="little").reshape(-1)[:n].astype(bool)


def torch_packer(ex, c, dest):
    first, n = ex.chunks[c]
    cap = ex.capacity[c]
    nblk, b_at, r_at, v_at = _layout(n, cap)
    S = ex.view_ctx["sums"][first:first + n]
    live = (S != 0).any(1).numpy()
    masks, padded = _bits_to_words(live, nblk)
    seen, _ = _bits_to_words((ex.view_ctx["radii"][first:first + n] > 0).numpy(), nblk)
    words = np.zeros(sum_packet_words(n, cap, True), dtype=np.int32)
    assert words.size == dest.numel() and words.size >= v_at + 2 * nblk
    want = int(live.sum())
    words[0:7] = [min(want, cap), want, n, cap, first, MAGIC, v_at]
    words[45] = ex.view_ctx["view"]                                     # (the stand-in's whole camera: which view this is)
    words[SUM_HDR_WORDS:b_at] = masks.view(np.int32)
    words[b_at:b_at + nblk] = np.concatenate([[0], np.cumsum(padded.reshape(nblk, 64).sum(1))[:-1]]).astype(np.int32)
    rows = S.numpy()[live][:cap]
    words[r_at:r_at + SUM_ROW_FLOATS * rows.shape[0]] = rows.reshape(-1).view(np.int32)
    words[v_at:v_at + 2 * nblk] = seen.view(np.int32)
    dest.copy_(torch.from_numpy(words))


def _rows_of(w, n, cap):
    """(indices of the Gaussians with a row that fits, their rows [k, 12]) of one packet."""
    nblk, b_at, r_at, _ = _layout(n, cap)
    bits = _words_to_bits(w[SUM_HDR_WORDS:b_at], n)
    idx = np.nonzero(bits)[0]
    before = np.concatenate([[0], np.cumsum(bits)])[:-1]               # exclusive prefix over the packet
    block_start = before[np.minimum(idx // 64 * 64, n - 1)] if idx.size else before[:0]
    row = w[b_at:b_at + nblk][idx // 64] + (before[idx] - block_start)
    ok = row < cap
    table = w[r_at:r_at + SUM_ROW_FLOATS * cap].view(np.float32).reshape(cap, SUM_ROW_FLOATS)
    return idx[ok], torch.from_numpy(table[row[ok]].copy())


def torch_combiner(ex, c, packets, n_views, seq):
    first, n = ex.chunks[c]
    acc = torch.zeros(n, 3)
    over, wants = False, []
    for v in range(n_views):
        w = packets[v].numpy()
        assert int(w[2]) == n and int(w[4]) == first and int(w[5]) == MAGIC
        wants.append(int(w[1]))
        over |= int(w[1]) > int(w[3])
        idx, S = _rows_of(w, n, int(w[3]))
        acc[torch.from_numpy(idx).long()] += S[:, 0:3] * ex.params["opacities"][first + torch.from_numpy(idx).long()]
    ex.views["means3D"][first:first + n] = acc
    st = ex.status[c]
    st[0] = (seq << 32) | int(over)
    st[1:1 + n_views] = torch.tensor([(seq << 32) | x for x in wants], dtype=torch.int64)


def torch_accumulator(ex, c, packets, n_views, seq):
    """The statistics pass's contract in torch: nothing is written unless EVERY packet is clean; then, in view order, denom += 1
    and the radius joins the maximum where the view's bit is set, and the norm of the two moments is added where there is a row."""
    first, n = ex.chunks[c]
    cap = ex.capacity[c]
    ex.acc_calls.append((ex.step_no, c))
    _, _, _, v_at = _layout(n, cap)
    ws = [packets[v].numpy() for v in range(n_views)]
    bad = any(int(w[1]) > int(w[3]) or int(w[5]) != MAGIC or int(w[2]) != n or int(w[4]) != first or int(w[3]) != cap or int(w[6]) != v_at
              for w in ws)
    ex.stats_status[c][0] = (seq << 32) | int(bad)
    if bad:
        return
    d = ex.densify
    rows = slice(first, first + n)
    for w in ws:
        view = int(w[45])
        seen = torch.from_numpy(_words_to_bits(w[v_at:v_at + 2 * ((n + 63) // 64)], n))
        idx, S = _rows_of(w, n, cap)
        norm = torch.zeros(n)
        norm[torch.from_numpy(idx).long()] = torch.sqrt(S[:, 3] * S[:, 3] + S[:, 4] * S[:, 4])
        d.xyz_gradient_accum[rows, 0] += torch.where(seen, norm, torch.zeros(n))
        d.denom[rows, 0] += seen.to(torch.float32)
        r = _radius({k: t[rows] for k, t in ex.params.items()}, view)
        d.max_radii2D[rows] = torch.where(seen, torch.maximum(d.max_radii2D[rows], r), d.max_radii2D[rows])


def _stats(P):
    return types.SimpleNamespace(xyz_gradient_accum=torch.zeros(P, 1), denom=torch.zeros(P, 1), max_radii2D=torch.zeros(P))


def _worker(rank, world, port, P, K, steps, chunks, q):
    import torch.distributed as dist
    from frosting_amd import scenes
    from frosting_amd.parallel import SlotSumExchange, ViewParallelRasterizer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        shapes, params = _params(P, K)
        stats = _stats(P)
        ex = SlotSumExchange(shapes, "cpu", dist.group.WORLD, chunks=chunks, packer=torch_packer, combiner=torch_combiner,
                             densify=stats, accumulator=torch_accumulator)
        ex.set_params(params)
        ex.acc_calls = []
        sized = ex.wire_floats_per_rank == sum(sum_packet_words(n, n, True) for _, n in ex.chunks)
        repacks = []
        for it in range(steps):
            S, radii = _view(params, rank, it, P)
            ex.step_no = it
            ex.note_view(sums=S, radii=radii, view=rank)
            ex.start()
            ex.finish_in_step()
            repacks.append(ex.stats["repacks"])
        # a plan without densify keeps the parent's packets
        plain = SlotSumExchange(shapes, "cpu", dist.group.WORLD, chunks=chunks, packer=torch_packer, combiner=torch_combiner)
        unchanged = plain.densify is None and plain.wire_floats_per_rank == sum(sum_packet_words(n, n) for _, n in plain.chunks)
        # adopt_scene: ranks that disagree about the new size are refused, on every rank; agreeing ranks carry on
        scene = lambda n: scenes.Scene(torch.zeros(n, 3), torch.ones(n, 3), torch.zeros(n, 4), torch.ones(n, 1), torch.zeros(n, K, 3), 3)
        vpr = ViewParallelRasterizer(scene(P), "cpu", process_group=dist.group.WORLD, slotsum=True, chunks=chunks, densify=stats)
        try:
            vpr.adopt_scene(scene(P + 64 + rank))
            refused = ""
        except RuntimeError as e:
            refused = str(e)
        vpr.exchanges[1]._works = ["pending"]
        try:
            vpr.adopt_scene(scene(P + 100))
            pending = ""
        except RuntimeError as e:
            pending = str(e)
        vpr.exchanges[1]._works = []
        old = vpr.geom
        vpr.adopt_scene(scene(P + 100))
        ex2 = vpr.exchanges[0]
        adopted = (vpr.P, ex2.P, vpr.radii.numel(), tuple(vpr.dL_dmeans2D.shape), ex2.capacity == [n for _, n in ex2.chunks],
                   ex2.densify is stats, vpr.geom is old, bool((vpr.dL_dmeans2D == 0).all()), tuple(ex2.views["shs"].shape))
        q.put((rank, {k: getattr(stats, k).numpy().copy() for k in ("xyz_gradient_accum", "denom", "max_radii2D")}, list(ex.acc_calls),
               repacks, sized, unchanged, refused, pending, adopted))
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_view_statistics_on_two_gloo_ranks_and_adopt_scene():
    world, P, K, steps, chunks = 2, 2500, 16, 3, 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, P, K, steps, chunks, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=200) for _ in range(world)]
    for p in procs:
        p.join(timeout=30)
        assert p.exitcode == 0
    # the per-view formula, in one process, in view order
    _, params = _params(P, K)
    want = _stats(P)
    rowless = True
    for it in range(steps):
        for v in range(world):
            S, radii = _view(params, v, it, P)
            seen = radii > 0
            rowless &= bool((seen & ~(S != 0).any(1)).any()) and bool((~seen).any())      # every view: visible without a row, and not visible
            want.xyz_gradient_accum[:, 0] += torch.where(seen, torch.sqrt(S[:, 3] * S[:, 3] + S[:, 4] * S[:, 4]), torch.zeros(P))
            want.denom[:, 0] += seen.to(torch.float32)
            want.max_radii2D = torch.where(seen, torch.maximum(want.max_radii2D, radii.to(torch.float32)), want.max_radii2D)
    assert float(want.denom.max()) == steps * world and float(want.denom.min()) < steps * world
    assert rowless
    for rank, stats, calls, repacks, sized, unchanged, refused, pending, adopted in got:
        for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
            assert np.array_equal(stats[k], getattr(want, k).numpy()), (rank, k)            # every rank, bit for bit
        # once per chunk and step -- the third step overflowed both chunks' packets and packed them again
        assert sorted(calls) == [(it, c) for it in range(steps) for c in range(chunks)], calls
        assert repacks == [0, 0, chunks], repacks
        assert sized and unchanged
        assert "every rank must seed" in refused and f"{P + 64} .. {P + 65}" in refused
        assert "pending" in pending
        assert adopted == (P + 100, P + 100, P + 100, (P + 100, 3), True, True, True, True, (P + 100, K, 3)), adopted


def test_new_argument_records_have_the_headers_layout(tmp_path):
    """frg_pack_sum_args / frg_densify_views_args as frosting_amd/_lib.py restates them: every field at the offset the C compiler
    gives it in include/frosting_rasterizer.h, and the sizes agree; the library exports the three new entry points."""
    import ctypes as C
    import subprocess
    from frosting_amd import _lib
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    structs = (("frg_pack_sum_args", _lib.PackSumArgs), ("frg_densify_views_args", _lib.DensifyViewsArgs))
    lines = []
    for cname, ct in structs:
        lines.append(f'printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for fname, _ in ct._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "frosting_rasterizer.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", inc, str(src), "-o", str(exe)])
    want = {}
    for ln in subprocess.check_output([str(exe)], text=True).split("\n"):
        if ln.strip():
            cname, fname, val = ln.split()
            want[(cname, fname)] = int(val)
    for cname, ct in structs:
        assert C.sizeof(ct) == want[(cname, "sizeof")], cname
        for fname, _ in ct._fields_:
            assert getattr(ct, fname).offset == want[(cname, fname)], (cname, fname)
    L = _lib.lib()
    assert all(hasattr(L, s) for s in ("frg_sum_packet_bytes_ex", "frg_pack_sum_rows_ex", "frg_densify_accumulate_views"))
    for n, cap in ((1, 0), (65, 7), (4807, 1000), (3_000_000, 3_000_000)):
        assert 4 * sum_packet_words(n, cap) == L.frg_sum_packet_bytes(n, cap) == L.frg_sum_packet_bytes_ex(n, cap, 0)
        assert 4 * sum_packet_words(n, cap, True) == L.frg_sum_packet_bytes_ex(n, cap, 1)
    # the host refuses what the launch must not see: more than 16 views, a stride without room for the sections
    a = _lib.DensifyViewsArgs(struct_size=C.sizeof(_lib.DensifyViewsArgs), P=128, first=0, count=128, n_views=17)
    assert L.frg_densify_accumulate_views(C.byref(a)) == -1 and b"1..16 views" in L.frg_last_error()
    a.n_views, a.packets, a.packet_stride_bytes, a.capacity_rows = 2, 16, L.frg_sum_packet_bytes(128, 128), 128
    assert L.frg_densify_accumulate_views(C.byref(a)) == -1 and b"visibility section" in L.frg_last_error()
