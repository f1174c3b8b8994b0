"""Timings of the nearest-neighbour searches on the GPU.

  knn_bench.py [P]                         distCUDA2 at the C3 point count (3M points of the benchmark scene)
  knn_bench.py points [--chunks N]         knn_points at the three shapes the reference calls it with, each beside the
                                           only alternative on this platform: chunked torch.cdist(...)**2 + topk with
                                           the distance block kept under 2 GB.  The brute force is linear in the
                                           queries, so it is timed on N chunks (default 8, 0 = all of them) after one
                                           warm-up chunk and scaled to the whole query set; the line says so.
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from frosting_amd import _lib, scenes
from frosting_amd.knn import distCUDA2, knn_points

dev = torch.device("cuda:0")


def timed(fn, warmup=2, reps=5):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, out


def bench_dist(P):
    scene, _, _ = scenes.config_scene("c3", 0, P=P)
    pts = scene.means3D.to(dev)
    t, d = timed(lambda: distCUDA2(pts))
    print(f"distCUDA2 on {P} points: {1e3*t:.2f} ms per call; mean 3-NN squared distance {float(d.mean()):.3e}")


def brute_force(p1, p2, K, chunks):
    """Seconds for all of p1, the chunks timed, the chunks in all, and the last chunk's (dists, idx)."""
    rows = max(1, min(p1.shape[0], (2 << 30) // (4 * p2.shape[0])))
    total = (p1.shape[0] + rows - 1) // rows
    n = total if chunks <= 0 else min(chunks, total)

    def one(c):
        d = torch.cdist(p1[c * rows:(c + 1) * rows], p2) ** 2
        return torch.topk(d, min(K, p2.shape[0]), dim=1, largest=False)
    one(0)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for c in range(n):
        out = one(c)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * total / n, n, total, rows, out


def bench_points(chunks):
    c3 = scenes.config_scene("c3", 0)[0].means3D.to(dev)
    seed = scenes.CONFIGS["c4"]["seed"]
    c4 = scenes.make_shell_scene(2_000_000, seed).scene.means3D.to(dev)
    verts = scenes.sphere_mesh(316, 632)[0].to(dev)                 # 200 344 vertices of a finer shell mesh
    samples = scenes.make_shell_scene(1_000_000, seed + 7).scene.means3D.to(dev)
    L = _lib.lib()
    cases = [("a: self-query of the C3 points (sugar_model.py:1059)", c3, c3, 16),
             ("b: shell-mesh vertices -> C4 shell points (frosting_model.py:300)", verts, c4, 16),
             ("c: shell samples -> C4 shell points (frosting_model.py:520)", samples, c4, 1)]
    for name, p1, p2, K in cases:
        P1, P2 = p1.shape[0], p2.shape[0]
        ws = int(L.frg_knn_points_workspace_bytes(0 if p1 is p2 else P1, P2, K))
        t, out = timed(lambda: knn_points(p1[None], p2[None], K=K))
        tb, n, total, rows, last = brute_force(p1, p2, K, chunks)
        # the two agree on the rows of the last brute-force chunk up to cdist's rounding (it expands the square)
        lo = (n - 1) * rows
        got = out.dists[0, lo:lo + last.values.shape[0]]
        dev_max = float((got - last.values).abs().max())
        print(f"{name}: P1 {P1}, P2 {P2}, K {K}: knn_points {1e3*t:.2f} ms per call, workspace {ws} bytes; "
              f"cdist**2 + topk {1e3*tb:.1f} ms ({n} of {total} chunks of {rows} rows timed, scaled to all); "
              f"ratio {tb/t:.1f}; max |dists - brute force| on the last timed chunk {dev_max:.2e}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "points":
        chunks = int(sys.argv[sys.argv.index("--chunks") + 1]) if "--chunks" in sys.argv else 8
        bench_points(chunks)
    else:
        bench_dist(int(sys.argv[1]) if len(sys.argv) > 1 else 3_000_000)
