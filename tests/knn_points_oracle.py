"""TEST INFRASTRUCTURE.  Brute-force restatement of frosting_amd.knn.knn_points for one batch element: the float32
distance matrix (dx*dx + dy*dy) + dz*dz with d = p1 - p2, a stable argsort of every row -- which IS the order
ascending by (distance, index in p2) -- the first K columns, zero padding where K > P2.  numpy does not contract,
so these are the bits any exact search must give."""
import numpy as np


def cloud(n, seed, clustered=False):
    """The generator of tests/test_knn.py: a normal cloud, optionally with a dense clump far from the rest and
    exact duplicates."""
    g = np.random.default_rng(seed)
    p = g.standard_normal((n, 3)).astype(np.float32)
    if clustered:
        p[: n // 2] = p[: n // 2] * 0.01 + 5.0                   # a dense clump far from the rest
        p[n // 2: n // 2 + 5] = p[0]                             # exact duplicates (distance 0)
    return p


def dist2_rows(p1, p2):
    """[P1,P2] float32 squared distances, evaluated as the kernels evaluate them."""
    p1, p2 = np.asarray(p1, np.float32), np.asarray(p2, np.float32)
    d = p1[:, None, :] - p2[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn_points(p1, p2, K, chunk=512):
    """p1 [P1,3], p2 [P2,3] -> dists [P1,K] float32, idx [P1,K] int64."""
    P1, P2 = len(p1), len(p2)
    dists, idx = np.zeros((P1, K), np.float32), np.zeros((P1, K), np.int64)
    k = min(K, P2)
    if k == 0:
        return dists, idx
    for a in range(0, P1, chunk):
        d = dist2_rows(p1[a:a + chunk], p2)
        order = np.argsort(d, axis=1, kind="stable")[:, :k]
        idx[a:a + chunk, :k] = order
        dists[a:a + chunk, :k] = np.take_along_axis(d, order, axis=1)
    return dists, idx
