"""knn_points on the GPU: bit for bit (distances AND indices) against the brute-force restatement
tests/knn_points_oracle.py, the slab boundary of the leaf sweep, the cross-check with the pinned distCUDA2,
batches / lengths, the gradient, streams and the device guard."""
import numpy as np
import pytest
import torch

import knn_points_oracle as KO
from frosting_amd.knn import distCUDA2, knn_gather, knn_points

pytestmark = pytest.mark.gpu


def _run(p1, p2, K, dev, self_query=False):
    b = torch.from_numpy(p2).to(dev)[None]
    a = b if self_query else torch.from_numpy(p1).to(dev)[None]
    out = knn_points(a, b, K=K)
    assert out.knn is None and out.dists.dtype == torch.float32 and out.idx.dtype == torch.int64
    assert out.dists.shape == (1, a.shape[1], K) and out.idx.shape == (1, a.shape[1], K)
    return out.dists[0].cpu().numpy(), out.idx[0].cpu().numpy()


_WANT = {}


def _want(p1, p2, K):
    """The restatement at K = 32, computed once per pair of sets; a smaller K is its first K columns."""
    key = (p1.tobytes(), p2.tobytes())
    if key not in _WANT:
        _WANT.clear()                                              # consecutive cases share sets; keep one
        _WANT[key] = KO.knn_points(p1, p2, 32)
    d, i = _WANT[key]
    return d[:, :K], i[:, :K]


def _check(p1, p2, K, dev, self_query=False):
    got_d, got_i = _run(p1, p2, K, dev, self_query)
    want_d, want_i = _want(p2 if self_query else p1, p2, K)
    assert np.array_equal(got_i, want_i), f"{int((got_i != want_i).any(axis=1).sum())} rows differ in idx"
    assert np.array_equal(got_d, want_d), f"{int((got_d != want_d).any(axis=1).sum())} rows differ in dists"


def _queries(n, seed):
    """Queries around p2's clouds: the normal part, wider, and every third one inside the far clump at 5."""
    q = KO.cloud(n, seed) * 1.5
    q[::3] = q[::3] * 0.01 + 5.0
    return q


# (P1, P2, K): every capacity instantiation (1, 4, 8, 16, 32) with K at and below it, padding (K > P2), leaf sizes
TWO_SET = [(1, 1, 1), (63, 2, 1), (64, 2, 3), (65, 5, 8), (257, 5, 32), (1, 255, 2), (64, 256, 4), (257, 257, 16),
           (3000, 255, 32), (257, 5000, 2), (65, 5000, 4), (63, 257, 32), (3000, 5000, 1), (3000, 5000, 3),
           (3000, 5000, 8), (3000, 5000, 16), (3000, 5000, 32)]
SELF = [(1, 1), (1, 4), (2, 2), (5, 8), (255, 3), (256, 16), (257, 32), (5000, 1), (5000, 4), (5000, 8), (5000, 16),
        (5000, 32)]


@pytest.mark.parametrize("P1,P2,K", TWO_SET)
def test_two_sets_bit_for_bit(gpu_device, P1, P2, K):
    _check(_queries(P1, 100 + P1), KO.cloud(P2, P2, clustered=P2 >= 257), K, gpu_device)


@pytest.mark.parametrize("P2,K", SELF)
def test_self_query_bit_for_bit(gpu_device, P2, K):
    p2 = KO.cloud(P2, P2, clustered=P2 >= 257)
    _check(None, p2, K, gpu_device, self_query=True)
    got_d, got_i = _run(None, p2, K, gpu_device, self_query=True)
    assert (got_d[:, 0] == 0).all()                                # every point finds itself (or an earlier duplicate)
    if P2 == 5000:
        assert (got_i[:, 0] != np.arange(P2)).sum() == 5           # the five duplicates of point 0 resolve to index 0


@pytest.mark.parametrize("K", [1, 4, 16, 32])
def test_queries_far_outside_the_bounding_box(gpu_device, K):
    p2 = KO.cloud(5000, 7, clustered=True)
    q = KO.cloud(257, 8)
    q[:100] = q[:100] * 50.0 + np.float32(1000.0)                  # far beyond one corner
    q[100:200] = q[100:200] * 50.0 - np.float32(700.0)             # and beyond the opposite one
    q[200:230, 0] += np.float32(300.0)                             # outside along one axis only
    _check(q, p2, K, gpu_device)


@pytest.mark.parametrize("P2,K", [(5, 4), (300, 8), (300, 32)])
def test_all_points_identical(gpu_device, P2, K):
    p2 = np.tile(np.array([[0.25, -1.5, 3.0]], np.float32), (P2, 1))
    _check(_queries(65, 3), p2, K, gpu_device)                     # every distance ties: indices 0 ... K-1
    _check(None, p2, K, gpu_device, self_query=True)


@pytest.mark.parametrize("axis,K", [(0, 4), (1, 16), (2, 32)])
def test_coplanar_points(gpu_device, axis, K):
    p2 = KO.cloud(1000, 11)
    p2[:, axis] = np.float32(0.5)                                  # zero extent on one axis
    p2 = np.round(p2 * 8) / np.float32(8)                          # a lattice: many exact ties and duplicates
    _check(_queries(257, 12), p2, K, gpu_device)
    _check(None, p2, K, gpu_device, self_query=True)


def test_empty_sets(gpu_device):
    p = torch.from_numpy(KO.cloud(10, 1)).to(gpu_device)[None]
    out = knn_points(p[:, :0], p, K=3, return_nn=True)
    assert out.dists.shape == (1, 0, 3) and out.idx.shape == (1, 0, 3) and out.knn.shape == (1, 0, 3, 3)
    out = knn_points(p, p[:, :0], K=3, return_nn=True)
    assert out.dists.shape == (1, 10, 3) and not out.dists.any() and not out.idx.any() and not out.knn.any()


@pytest.fixture(scope="module")
def big_cloud():
    """300 000 points: more than KNN_SLAB x KNN_LEAF = 262 144, so the leaf table takes two slabs."""
    return KO.cloud(300_000, 300_000, clustered=True)


def _rows_bit_for_bit(got_d, got_i, q, p2, K, rows):
    for r in rows:
        d = KO.dist2_rows(q[r:r + 1], p2)[0]
        order = np.argsort(d, kind="stable")[:K]
        assert np.array_equal(got_i[r], order), r
        assert np.array_equal(got_d[r], d[order]), r


def test_slab_boundary_two_sets(gpu_device, big_cloud):
    q = _queries(4096, 42)
    got_d, got_i = _run(q, big_cloud, 16, gpu_device)
    rows = np.random.default_rng(0).choice(4096, 64, replace=False)
    _rows_bit_for_bit(got_d, got_i, q, big_cloud, 16, rows)


def test_slab_boundary_self_query(gpu_device, big_cloud):
    got_d, got_i = _run(None, big_cloud, 16, gpu_device, self_query=True)
    rows = np.random.default_rng(1).choice(300_000, 64, replace=False)
    rows[:6] = [0, 149_999, 150_000, 150_004, 262_143, 299_999]    # duplicates, the clump's end, the slab's and the last leaf
    _rows_bit_for_bit(got_d, got_i, big_cloud, big_cloud, 16, rows)


@pytest.mark.parametrize("n,clustered", [(20000, False), (5000, True)])
def test_cross_check_with_distCUDA2(gpu_device, n, clustered):
    """distCUDA2 is pinned to the reference's own binary: its value is the mean of neighbours 1 ... 3 of a K = 4 self-query."""
    p = torch.from_numpy(KO.cloud(n, n, clustered)).to(gpu_device)
    d = knn_points(p[None], p[None], K=4).dists[0].cpu().numpy()
    # the mean in numpy: IEEE float32 division, as distCUDA2 divides (torch divides by a scalar with a reciprocal multiply)
    want = ((d[:, 1] + d[:, 2]) + d[:, 3]) / np.float32(3.0)
    got = distCUDA2(p).cpu().numpy()
    assert want.dtype == np.float32 and np.array_equal(want, got), f"{int((want != got).sum())} of {n} differ"


def test_batch_and_lengths(gpu_device):
    K = 8
    p1 = torch.from_numpy(np.stack([_queries(300, 1), _queries(300, 2)])).to(gpu_device)
    p2 = torch.from_numpy(np.stack([KO.cloud(600, 3, True), KO.cloud(600, 4, True)])).to(gpu_device)
    l1 = torch.tensor([300, 65], device=gpu_device)
    l2 = torch.tensor([5, 600], device=gpu_device)
    out = knn_points(p1, p2, lengths1=l1, lengths2=l2, K=K, return_nn=True)
    for n, (n1, n2) in enumerate([(300, 5), (65, 600)]):
        single = knn_points(p1[n:n + 1, :n1], p2[n:n + 1, :n2], K=K)
        assert torch.equal(out.dists[n, :n1], single.dists[0]) and torch.equal(out.idx[n, :n1], single.idx[0])
        want_d, want_i = KO.knn_points(p1[n, :n1].cpu().numpy(), p2[n, :n2].cpu().numpy(), K)
        assert np.array_equal(single.dists[0].cpu().numpy(), want_d) and np.array_equal(single.idx[0].cpu().numpy(), want_i)
        assert not out.dists[n, n1:].any() and not out.idx[n, n1:].any()        # rows beyond lengths1: padding
    assert not out.dists[0, :, 5:].any() and not out.idx[0, :, 5:].any()          # slots beyond lengths2: padding
    assert torch.equal(out.knn, knn_gather(p2, out.idx, l2))
    assert not out.knn[0, :, 5:].any()
    full = knn_points(p1, p2, K=K, return_nn=True)
    assert torch.equal(full.knn, knn_gather(p2, full.idx))
    assert torch.equal(full.knn[1, 7, 2], p2[1, full.idx[1, 7, 2]])


@pytest.mark.parametrize("weighted", [False, True])
def test_gradient(gpu_device, weighted):
    """dists' gradient to p1 and p2 against the float64 CPU autograd of ((p1[:,None] - p2[idx])**2).sum(-1) with the
    same idx.  Bound per element: (n + 3) * 2^-24 * sum|terms|, n = the number of terms the element sums, both taken
    from the float64 computation -- float32 rounding of the difference, the product with the weight and a sum of n
    terms in any order; derived, not measured."""
    K = 8
    a = torch.from_numpy(_queries(257, 5)).to(gpu_device).requires_grad_(True)
    b = torch.from_numpy(KO.cloud(300, 6, True)).to(gpu_device).requires_grad_(True)
    out = knn_points(a[None], b[None], K=K)
    assert out.dists.requires_grad and not out.idx.requires_grad
    g = torch.Generator().manual_seed(9)
    w = (torch.randn(257, K, generator=g) if weighted else torch.ones(257, K)).float()
    (out.dists[0] * w.to(gpu_device)).sum().backward()

    idx = out.idx[0].cpu()
    a64 = a.detach().cpu().double().requires_grad_(True)
    b64 = b.detach().cpu().double().requires_grad_(True)
    d64 = ((a64[:, None, :] - b64[idx]) ** 2).sum(-1)
    np.testing.assert_allclose(out.dists[0].detach().cpu().numpy(), d64.detach().numpy(), rtol=1e-6, atol=1e-12)
    (d64 * w.double()).sum().backward()
    terms = (2.0 * (a64.detach()[:, None, :] - b64.detach()[idx]) * w.double()[..., None]).abs()     # [P1,K,3]
    abs1, n1 = terms.sum(1), torch.full((257, 3), float(K), dtype=torch.float64)
    abs2 = torch.zeros(300, 3, dtype=torch.float64).index_add_(0, idx.reshape(-1), terms.reshape(-1, 3))
    n2 = torch.zeros(300, dtype=torch.float64).index_add_(0, idx.reshape(-1), torch.ones(257 * K, dtype=torch.float64))
    for name, got, want, n, s in (("p1", a.grad, a64.grad, n1, abs1), ("p2", b.grad, b64.grad, n2[:, None], abs2)):
        err = (got.cpu().double() - want).abs()
        bound = (n + 3.0) * 2.0 ** -24 * s
        worst = float((err - bound).max())
        print(f"{name}: max |err| {float(err.max()):.3e}, max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert worst <= 0.0, f"{name}: an element exceeds its bound by {worst:.3e}"
    assert float(n2.sum()) == 257 * K and bool((b.grad[n2 == 0] == 0).all())


def test_side_stream_and_device_guard(gpu_device):
    p1 = torch.from_numpy(_queries(3000, 21)).to(gpu_device)[None]
    p2 = torch.from_numpy(KO.cloud(5000, 22, True)).to(gpu_device)[None]
    want = knn_points(p1, p2, K=16)
    want_self = knn_points(p2, p2, K=4)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        got = knn_points(p1, p2, K=16)
        got_self = knn_points(p2, p2, K=4)
    side.synchronize()
    assert torch.equal(got.dists, want.dists) and torch.equal(got.idx, want.idx)
    assert torch.equal(got_self.dists, want_self.dists) and torch.equal(got_self.idx, want_self.idx)
    with torch.cuda.device(torch.cuda.device_count() - 1):         # another current device where there is one
        got = knn_points(p1, p2, K=16)
    torch.cuda.synchronize()
    assert got.dists.device == p1.device and torch.equal(got.dists, want.dists) and torch.equal(got.idx, want.idx)
