"""The level-set crossings without a GPU: tests/levelset_oracle.py against the arrays the reference's own functions produced
(tests/golden/levelset_*.npz; tools/make_golden_levelset.py) -- every discrete result equal on every ray, the floats to
1e-12 -- and the C ABI's names, refusals, workspace size and record layout."""
import ctypes as C
import glob
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import levelset_oracle as LO
from frosting_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "levelset_*.npz")))
IDS = [os.path.basename(p)[:-4] for p in FIXTURES]
NAMES = ("frg_levelset_workspace_bytes", "frg_levelset")
MODEL = ("points", "scaling", "quaternions", "strengths")


def oracle_run(fx, dtype):
    """The oracle's Python-level function on a fixture's inputs -> {tag: outputs}, tags as the fixture names them."""
    t = lambda k: torch.from_numpy(fx[k]).to(dtype)
    model = [t(k) for k in MODEL]
    if str(fx["kind"]) == "normals":
        extra = {k: t(k) for k in ("min_clamping_inner_dist", "max_clamping_outer_dist") if k in fx}
        out = LO.level_points_along_normals(*model, t("verts"), t("normals"), t("inner_range"), t("outer_range"),
                                            n_samples_per_vertex=int(fx["n"]), n_closest_gaussians_to_use=int(fx["K"]),
                                            level=float(fx["levels"][0]), smooth_points=bool(fx["smooth"]),
                                            use_last_intersection_as_inner_level_point=bool(fx["last"]),
                                            min_layer_size=float(fx["min_layer_size"]), spatial_extent=float(fx["spatial_extent"]), **extra)
        return {"run": out}
    levels = [float(v) for v in fx["levels"]]
    out = LO.level_surface_points_from_rays(t("world_points"), t("camera_center"), torch.from_numpy(fx["idx"]), *model, levels,
                                            n_points_in_range=int(fx["n"]), range_size=float(fx["range_size"]),
                                            density_factor=float(fx["density_factor"]), return_normals=True,
                                            use_last_intersection_as_inner_level_point=bool(fx["last"]))
    for o in out.values():
        o["empty"] = ~o["valid"]
    return {f"level{lv}": out[lv] for lv in levels}


def test_header_and_symbol_list_carry_the_names():
    hdr = open(os.path.join(ROOT, "include", "frosting_rasterizer.h")).read()
    declared = set(re.findall(r"\b(frg_[a-z_0-9]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    from frosting_amd.levelset import level_points_along_normals, level_surface_points_from_rays, ray_level_crossings  # noqa: F401


def _args(**over):
    """A record whose every pointer is a non-null dummy: the refusals tested here come before anything is dereferenced."""
    a = _lib.LevelsetArgs(struct_size=C.sizeof(_lib.LevelsetArgs), P=10, R=20, K=16, n=21, L=1, idx_is_int64=1, inner_mode=0)
    for name, kind in _lib.LevelsetArgs._fields_:
        if kind is C.c_void_p and name != "hip_stream":
            setattr(a, name, 256 * 4096)
    a.levels[0], a.density_factor, a.workspace_bytes = 0.1, 1.0, 1 << 40
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_entry_point_refuses_bad_arguments():
    L = _lib.lib()
    call, einval = L.frg_levelset, -1
    assert call(None) == einval
    assert call(C.byref(_args(struct_size=8))) == einval and b"struct_size" in L.frg_last_error()
    for K in (0, 33, -1):
        assert call(C.byref(_args(K=K))) == einval and b"K =" in L.frg_last_error()
    for n in (1, 33, -1):
        assert call(C.byref(_args(n=n))) == einval and b"samples" in L.frg_last_error()
    for nl in (0, 9):
        assert call(C.byref(_args(L=nl))) == einval and b"levels" in L.frg_last_error()
    assert call(C.byref(_args(inner_mode=2))) == einval and b"inner_mode" in L.frg_last_error()
    for name in ("idx", "origins", "directions", "t_scale", "t_offset", "lin", "points", "scaling", "quaternions", "strengths", "bad_index"):
        assert call(C.byref(_args(**{name: None}))) == einval, name
        assert b"null" in L.frg_last_error(), name
    need = L.frg_levelset_workspace_bytes(10, 20, 16, 0)
    assert need > 0
    assert call(C.byref(_args(workspace_bytes=need - 1))) == einval and b"workspace" in L.frg_last_error()
    assert call(C.byref(_args(workspace=None))) == einval
    assert call(C.byref(_args(workspace=256 * 4096 + 16))) == einval and b"aligned" in L.frg_last_error()
    assert call(C.byref(_args(R=(1 << 31) // 21 + 1))) == einval and b"2^31" in L.frg_last_error()
    assert call(C.byref(_args(R=1 << 26, n=2, K=32))) == einval and b"2^31" in L.frg_last_error()
    # no rays: nothing to launch, whatever the pointers are
    assert call(C.byref(_args(R=0, idx=None, origins=None, workspace=None))) == 0


def test_workspace_bytes_monotone_and_refusing():
    L = _lib.lib()
    sizes_r = [L.frg_levelset_workspace_bytes(1000, r, 16, 0) for r in (1, 63, 1000, 4097, 100000, 1000000)]
    sizes_p = [L.frg_levelset_workspace_bytes(p, 1000, 16, 0) for p in (1, 63, 1000, 4097, 100000, 1000000)]
    assert sizes_r == sorted(sizes_r) and sizes_p == sorted(sizes_p) and sizes_r[0] > 0 and sizes_p[-1] > sizes_p[0]
    assert all(s % 256 == 0 for s in sizes_r + sizes_p)
    assert L.frg_levelset_workspace_bytes(1000, 1000, 33, 0) == 0 and L.frg_levelset_workspace_bytes(1000, 1000, 0, 0) == 0


def test_argument_record_has_the_headers_layout(tmp_path):
    lines = ['printf("sizeof %zu\\n", sizeof(frg_levelset_args));']
    for fname, _ in _lib.LevelsetArgs._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof(frg_levelset_args, {fname}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "frosting_rasterizer.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    want = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).split("\n") if ln.strip())
    assert C.sizeof(_lib.LevelsetArgs) == int(want["sizeof"])
    for fname, _ in _lib.LevelsetArgs._fields_:
        assert getattr(_lib.LevelsetArgs, fname).offset == int(want[fname]), fname


def test_python_layer_refusals():
    from frosting_amd.levelset import ray_level_crossings
    o, d, ts = torch.zeros(4, 3), torch.ones(4, 3), torch.ones(4)
    pts, sc, q, st = torch.zeros(5, 3), torch.ones(5, 3), torch.ones(5, 4), torch.ones(5, 1)
    with pytest.raises(RuntimeError, match="GPU only"):
        ray_level_crossings(o, d, ts, ts, torch.linspace(0, 1, 21), torch.zeros(4, 2, dtype=torch.int64), pts, sc, q, st, [0.1])


def test_fixtures_cover_the_cases_and_name_their_source():
    assert len(FIXTURES) >= 6
    kinds, covered = set(), {}
    for path in FIXTURES:
        fx = np.load(path)
        assert os.path.getsize(path) < (1 << 20)
        assert re.fullmatch(r"[0-9a-f]{64}", str(fx["frosting_model_sha256"]))
        assert fx["idx"].dtype == np.int64 and 0 <= fx["idx"].min() and fx["idx"].max() < fx["points"].shape[0]
        assert 0 < float(fx["tau"]) < 1e-4
        kinds.add((str(fx["kind"]), int(fx["K"]), int(fx["n"]), bool(fx["last"])))
        n = int(fx["n"])
        for key in fx.files:
            if key.endswith("_f64_first_above"):
                tag = key[:-len("_f64_first_above")]
                f, l, e = fx[key], fx[f"{tag}_f64_last_above"], fx[f"{tag}_f64_empty"]
                for name, m in (("outer_found", f > 0), ("outer_unbound", f == 0), ("inner_found", l < n - 1),
                                ("inner_unbound", l == n - 1), ("empty", e), ("one", fx[f"{tag}_f32_densities"] == 1)):
                    covered[name] = max(covered.get(name, 0), int(m.sum()))
    assert {("normals", 16, 21, True), ("normals", 16, 21, False), ("camera", 16, 21, False), ("normals", 5, 7, True)} <= kinds
    assert all(v >= 5 for v in covered.values()) and len(covered) == 6, covered


def test_fixtures_come_from_the_reference_file():
    path = os.path.join(os.environ.get("FROSTING_REFERENCE", "/root/reference"), "frosting_scene", "frosting_model.py")
    if not os.path.exists(path):
        pytest.skip("the reference tree is not on this machine")
    sha = hashlib.sha256(open(path, "rb").read()).hexdigest()
    for p in FIXTURES:
        assert str(np.load(p)["frosting_model_sha256"]) == sha, p


@pytest.mark.parametrize("path", FIXTURES, ids=IDS)
def test_restatement_reproduces_the_reference(path):
    fx = np.load(path)
    if str(fx["kind"]) == "normals":          # the neighbour table the reference's knn_points call produced
        d, i = LO.KO.knn_points(fx["verts"], fx["points"], int(fx["K"]))
        assert np.array_equal(i, fx["idx"])
    for tag, out in oracle_run(fx, torch.float64).items():
        for k in ("first_above", "last_above", "under_first", "empty", "valid"):
            if f"{tag}_f64_{k}" in fx:
                assert np.array_equal(out[k].numpy(), fx[f"{tag}_f64_{k}"]), (tag, k)
        checked = 0
        for k in ("densities", "outer_dist", "inner_dist", "outer_verts", "inner_verts", "intersection_points",
                  "inner_intersection_points", "normals"):
            if f"{tag}_f64_{k}" in fx:
                want, got = fx[f"{tag}_f64_{k}"], out[k].numpy()
                assert got.shape == want.shape and np.linalg.norm(got - want) <= 1e-12 * np.linalg.norm(want), (tag, k)
                f32 = fx[f"{tag}_f32_{k}"]
                assert f32.dtype == np.float32 and f32.shape == want.shape
                assert 0 < np.linalg.norm(f32 - want) <= 1e-3 * np.linalg.norm(want), (tag, k)
                checked += 1
        assert checked >= 4
