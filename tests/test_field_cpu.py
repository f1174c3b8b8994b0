"""The density / SDF field without a GPU: the C ABI's names and refusals, the workspace size, the Python layer's refusals,
and tests/field_oracle.py against the arrays the reference's own get_field_values produced (tests/golden/field_*.npz;
tools/make_golden_field.py).  The float64 arrays are reproduced to 1e-12; a fixture's float32 arrays are the reference's own
float32 evaluation -- the error yardstick of the GPU tests, not something a restatement reproduces bit for bit."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest
import torch

import field_oracle as FO
from frosting_amd import _lib
from frosting_amd.field import compute_density, field_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "field_*.npz")))
NAMES = ("frg_field_workspace_bytes", "frg_field_forward", "frg_field_backward")


def test_header_and_symbol_list_carry_the_names():
    hdr = open(os.path.join(ROOT, "include", "frosting_rasterizer.h")).read()
    declared = set(re.findall(r"\b(frg_[a-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)


def _args(**over):
    """A record whose every pointer is a non-null dummy: the refusals tested here come before anything is dereferenced."""
    a = _lib.FieldArgs(struct_size=C.sizeof(_lib.FieldArgs), P=10, N=20, K=16, idx_is_int64=1, beta_mode=1)
    dummy = 256 * 4096
    for name, kind in _lib.FieldArgs._fields_:
        if kind is C.c_void_p and name != "hip_stream":
            setattr(a, name, dummy)
    a.density_threshold, a.density_factor, a.opacity_min_clamp = 1.0, 1.0, 1e-16
    a.workspace_bytes = 1 << 40
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("fn", ["frg_field_forward", "frg_field_backward"])
def test_entry_points_refuse_bad_arguments(fn):
    L = _lib.lib()
    call = getattr(L, fn)
    backward = fn.endswith("backward")
    einval = -1
    assert call(None) == einval
    assert call(C.byref(_args(struct_size=8))) == einval
    for K in (0, 33, -1):
        assert call(C.byref(_args(K=K))) == einval
        assert b"32" in L.frg_last_error()
    for mode in (-1, 3):
        assert call(C.byref(_args(beta_mode=mode))) == einval
        assert b"beta_mode" in L.frg_last_error()
    required = ["idx", "x", "points", "scaling", "quaternions", "strengths", "bad_index"]
    if backward:
        required += ["dL_dx", "dL_dpoints", "dL_dscaling", "dL_dquaternions", "dL_dstrengths"]
    for name in required:
        assert call(C.byref(_args(**{name: None}))) == einval, name
        assert b"null" in L.frg_last_error(), name
    assert call(C.byref(_args(beta_mode=2, beta_fallback=None))) == einval
    assert call(C.byref(_args(beta_mode=0))) == einval                      # beta / sdf pointers without a beta mode
    need = L.frg_field_workspace_bytes(10, 20, 16, 1 if backward else 0)
    assert need > 0
    assert call(C.byref(_args(workspace_bytes=need - 1))) == einval
    assert b"workspace" in L.frg_last_error()
    assert call(C.byref(_args(workspace=None))) == einval
    assert call(C.byref(_args(workspace=256 * 4096 + 16))) == einval        # not 256-byte aligned
    assert call(C.byref(_args(N=1 << 27))) == einval


def test_workspace_bytes_monotone_and_refusing():
    L = _lib.lib()
    for flags in (0, 1):
        sizes_n = [L.frg_field_workspace_bytes(1000, n, 16, flags) for n in (1, 63, 1000, 4097, 100000, 1000000)]
        sizes_p = [L.frg_field_workspace_bytes(p, 1000, 16, flags) for p in (1, 63, 1000, 4097, 100000, 1000000)]
        assert sizes_n == sorted(sizes_n) and sizes_p == sorted(sizes_p) and sizes_n[0] > 0
        assert all(s % 256 == 0 for s in sizes_n + sizes_p)
    assert L.frg_field_workspace_bytes(1000, 1000, 16, 1) > L.frg_field_workspace_bytes(1000, 1000, 16, 0)
    assert L.frg_field_workspace_bytes(1000, 1000, 33, 0) == 0 and L.frg_field_workspace_bytes(1000, 1000, 0, 0) == 0


def test_python_layer_refusals():
    x, idx = torch.zeros(4, 3), torch.zeros(4, 2, dtype=torch.int64)
    pts, sc, q, st = torch.zeros(5, 3), torch.ones(5, 3), torch.ones(5, 4), torch.ones(5, 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        field_values(x, idx, pts, sc, q, st)
    with pytest.raises(RuntimeError, match="GPU only"):
        compute_density(x, idx, pts, sc, q, st)
    with pytest.raises(NotImplementedError, match="return_sdf_grad"):
        field_values(x, idx, pts, sc, q, st, return_sdf_grad=True)


def test_fixtures_exist_and_name_their_source():
    assert len(FIXTURES) >= 2
    for path in FIXTURES:
        fx = np.load(path)
        assert re.fullmatch(r"[0-9a-f]{64}", str(fx["sugar_model_sha256"]))
        assert fx["idx"].dtype == np.int64 and fx["idx"].max() < fx["points"].shape[0]
        for mode in ("average", "weighted_average"):
            assert (fx[f"{mode}_f64_out_density"] < 1.0).all()                # the reference's own gradients are finite


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
@pytest.mark.parametrize("mode", ["average", "weighted_average"])
@pytest.mark.parametrize("tag", ["sdf", "nosdf"])
def test_restatement_reproduces_the_reference(path, mode, tag):
    fx = np.load(path)
    ups = {k: fx["upstream_" + k] for k in FO.UPSTREAM if not (tag == "nosdf" and k == "sdf")}
    out, grads = FO.run({k: fx[k] for k in FO.INPUTS}, fx["idx"], ups, torch.float64, beta_mode=mode,
                        density_factor=float(fx["density_factor"]))
    for k, v in out.items():
        want = fx[f"{mode}_f64_out_{k}"]
        assert np.linalg.norm(v - want) <= 1e-12 * np.linalg.norm(want), k
    for k, v in grads.items():
        want = fx[f"{mode}_{tag}_f64_grad_{k}"]
        assert np.linalg.norm(v - want) <= 1e-12 * np.linalg.norm(want), k
        # and the float32 arrays are what they claim: a float32 evaluation, close to the float64 one but not equal to it
        f32 = fx[f"{mode}_{tag}_f32_grad_{k}"]
        assert f32.dtype == np.float32 and 0 < np.linalg.norm(f32 - want) <= 1e-3 * np.linalg.norm(want), k
