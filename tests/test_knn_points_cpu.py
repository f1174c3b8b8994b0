"""knn_points without a GPU: the brute-force restatement against scipy's k-d tree, argument validation, knn_gather,
the pytorch3d.ops shim and the C ABI's symbol lists."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import knn_points_oracle as KO
from frosting_amd import _lib
from frosting_amd.knn import install_as_pytorch3d_ops, knn_gather, knn_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K", [1, 4, 16])
def test_restatement_against_kdtree(K):
    from scipy.spatial import cKDTree
    p = KO.cloud(3000, 1, clustered=True)
    q = KO.cloud(700, 2) * 2.0
    for p1 in (p, q):                                             # a self-query and a two-set query
        d, i = cKDTree(p.astype(np.float64)).query(p1.astype(np.float64), k=K + 1)
        got_d, got_i = KO.knn_points(p1, p, K)
        np.testing.assert_allclose(got_d, d[:, :K] ** 2, rtol=2e-5, atol=1e-10)
        # the neighbour SETS, where the K+1 smallest float32 distances of the row are distinct (no tie to resolve)
        full = np.sort(KO.dist2_rows(p1, p), axis=1)[:, :K + 1]
        distinct = (np.diff(full, axis=1) > 0).all(axis=1)
        assert distinct.sum() > len(p1) // 2
        assert np.array_equal(np.sort(got_i[distinct], axis=1), np.sort(i[distinct, :K], axis=1))


def test_restatement_ties_and_padding():
    p2 = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 0]], np.float32)
    p1 = np.zeros((1, 3), np.float32)
    d, i = KO.knn_points(p1, p2, 6)
    assert i.tolist() == [[3, 0, 1, 2, 0, 0]] and d.tolist() == [[0, 1, 1, 1, 0, 0]]
    d, i = KO.knn_points(p1, p2[:0], 2)
    assert i.tolist() == [[0, 0]] and d.tolist() == [[0, 0]]
    assert KO.knn_points(p1[:0], p2, 2)[0].shape == (0, 2)


def test_argument_validation():
    p = torch.zeros(1, 5, 3)
    with pytest.raises(ValueError, match="norm"):
        knn_points(p, p, norm=1)
    for K in (0, 33, -1):
        with pytest.raises(ValueError, match="32"):
            knn_points(p, p, K=K)
    with pytest.raises(ValueError, match="dimensions"):
        knn_points(p[0], p[0])
    with pytest.raises(ValueError, match="dimensions"):
        knn_points(torch.zeros(1, 5, 2), p)
    with pytest.raises(ValueError, match="batch"):
        knn_points(torch.zeros(2, 5, 3), p)
    with pytest.raises(RuntimeError, match="GPU only"):
        knn_points(p, p, K=2, version=3, return_sorted=False)


def test_knn_gather_against_explicit_indexing():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 7, 5, generator=g)
    idx = torch.randint(0, 7, (2, 4, 3), generator=g)
    got = knn_gather(x, idx)
    assert got.shape == (2, 4, 3, 5)
    for n in range(2):
        for i in range(4):
            for k in range(3):
                assert torch.equal(got[n, i, k], x[n, idx[n, i, k]])
    lengths = torch.tensor([2, 7])
    got = knn_gather(x, idx, lengths)
    want = torch.stack([x[n][idx[n]] for n in range(2)])
    want[0, :, 2:] = 0.0
    assert torch.equal(got, want)
    assert knn_gather(x[:, :0], idx).abs().sum() == 0


def test_shim_registers_pytorch3d_ops_when_absent():
    before = {k: sys.modules.get(k) for k in ("pytorch3d", "pytorch3d.ops")}
    try:
        import pytorch3d.ops  # noqa: F401
        pytest.skip("a real pytorch3d is installed")              # (absent on this platform: SURVEY Appendix B)
    except ImportError:
        pass
    try:
        ops = install_as_pytorch3d_ops()
        from pytorch3d.ops import knn_gather as g, knn_points as f
        assert f is knn_points and g is knn_gather and sys.modules["pytorch3d.ops"] is ops
        assert sorted(n for n in vars(ops) if not n.startswith("__")) == ["knn_gather", "knn_points"]
    finally:
        for k, v in before.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_header_and_symbol_list_carry_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "frosting_rasterizer.h")).read()
    declared = set(re.findall(r"\b(frg_[a-z_0-9]+)\s*\(", hdr))
    for name in ("frg_knn_points_workspace_bytes", "frg_knn_points"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().frg_version() == 2
    assert _lib.lib().frg_knn_points(1, None, 1, None, 33, None, None, None, 0, None) != 0
    assert b"32" in _lib.lib().frg_last_error()
