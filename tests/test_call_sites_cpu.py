"""Mechanical "callers unchanged" check (CPU tier): the reference's own call sites of the rasterizer, parsed with `ast`
(tools/make_golden_call_sites.py, recorded in tests/golden/call_sites.json) -- every import, keyword and positional
parameter they use must be accepted by the drop-in package.

Sites: gaussian_splatting/gaussian_renderer/__init__.py:14,85-93,
frosting_scene/frosting_model.py:29,1452-1467,1649-1657 (and its other render paths),
frosting_scene/sugar_model.py:10,2213-2228,2317-2325, and the alternative backend that proves the interface's shape,
gsplat_wrapper/rasterization.py:18-114.
"""
import ast
import inspect
import json
import os

import pytest

CALLERS = ["gaussian_splatting/gaussian_renderer/__init__.py", "frosting_scene/frosting_model.py",
           "frosting_scene/sugar_model.py"]
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_sites.json")) as _f:
    SITES = json.load(_f)


def _api():
    from frosting_amd import rasterizer as R
    return R.GaussianRasterizationSettings, R.GaussianRasterizer


@pytest.mark.parametrize("rel", CALLERS)
def test_imports_of_the_call_sites_resolve(rel):
    """`from diff_gaussian_rasterization import A, B`: every imported name exists in the drop-in package (its
    __init__ is read as source -- importing it needs the built extension, which the GPU tier covers)."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "diff_gaussian_rasterization", "__init__.py")) as f:
        pkg = ast.parse(f.read())
    exported = set()
    for n in ast.walk(pkg):
        if isinstance(n, ast.ImportFrom):
            exported |= {a.asname or a.name for a in n.names}
        elif isinstance(n, ast.Assign):
            for t in n.targets:
                exported |= {e.id for e in ast.walk(t) if isinstance(e, ast.Name)}
        elif isinstance(n, ast.FunctionDef):
            exported.add(n.name)
    wanted = set(SITES["callers"][rel]["imports"])
    assert wanted, f"{rel} no longer imports diff_gaussian_rasterization"
    assert wanted <= exported, wanted - exported


@pytest.mark.parametrize("rel", CALLERS)
def test_settings_keywords_of_the_call_sites(rel):
    Settings, _ = _api()
    calls = SITES["callers"][rel]["settings_calls"]
    assert calls, f"{rel}: no GaussianRasterizationSettings(...) call found"
    for c in calls:
        assert not c["positional"], f"{rel}:{c['line']}: positional settings arguments"
        kws = c["keywords"]
        assert None not in kws, f"{rel}:{c['line']}: **kwargs"
        assert set(kws) <= set(Settings._fields), (rel, c["line"], set(kws) - set(Settings._fields))
        # a NamedTuple without defaults: every field must be given, as the reference's is
        assert set(kws) == set(Settings._fields), (rel, c["line"], set(Settings._fields) - set(kws))


@pytest.mark.parametrize("rel", CALLERS)
def test_rasterizer_call_keywords_of_the_call_sites(rel):
    _, Rasterizer = _api()
    sig = inspect.signature(Rasterizer.forward)
    params = [p for p in sig.parameters.values() if p.name != "self"]
    accepted = {p.name for p in params}
    required = {p.name for p in params if p.default is inspect.Parameter.empty}
    ctor = SITES["callers"][rel]["rasterizer_ctor_calls"]
    assert ctor
    for c in ctor:
        assert c["keywords"] == ["raster_settings"] and not c["positional"], (rel, c["line"])
    assert "raster_settings" in inspect.signature(Rasterizer.__init__).parameters
    calls = SITES["callers"][rel]["rasterizer_calls"]
    assert calls, f"{rel}: no call of a GaussianRasterizer instance found"
    for c in calls:
        assert not c["positional"], f"{rel}:{c['line']}: positional call"
        kws = set(c["keywords"])
        assert kws <= accepted, (rel, c["line"], kws - accepted)
        assert required <= kws, (rel, c["line"], required - kws)


def test_interface_shape_of_the_alternative_backend():
    """gsplat_wrapper/rasterization.py re-implements the same two classes over gsplat: its settings fields and its
    forward parameter list (positional order included) are the interface every caller relies on."""
    Settings, Rasterizer = _api()
    alt = SITES["alternative_backend"]
    assert alt["file"] == "gsplat_wrapper/rasterization.py"
    fields = alt["settings_init_fields"]
    assert fields == list(Settings._fields)
    theirs = alt["forward_params"]
    ours = [p for p in inspect.signature(Rasterizer.forward).parameters if p != "self"]
    assert set(theirs) <= set(ours)
    # the two leading positional parameters agree (means3D, means2D); the rest are passed by keyword everywhere
    assert ours[:2] == theirs[:2] == ["means3D", "means2D"]


def test_native_module_exports_named_by_the_reference():
    """DGR/ext.cpp:15-18 exports three functions; the autograd wiring above them calls them by these names
    (DGR/diff_gaussian_rasterization/__init__.py:82,130,183)."""
    import re
    names = set(SITES["native_exports"]["names"])
    assert names == {"rasterize_gaussians", "rasterize_gaussians_backward", "mark_visible"}
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    binding = open(os.path.join(here, "frosting_amd", "csrc", "torch_ext", "torch_binding.cpp")).read()
    assert names <= set(re.findall(r'm\.def\("(\w+)"', binding))
    from frosting_amd.rasterizer import _C
    assert all(hasattr(_C, n) for n in names)
