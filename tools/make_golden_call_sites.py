"""Fixture of the reference's call sites of the rasterizer (tests/test_call_sites_cpu.py): its callers are parsed with
`ast` and what the test checks is recorded as names and line numbers in tests/golden/call_sites.json --
  * per caller: the names it imports from diff_gaussian_rasterization, and for every GaussianRasterizationSettings(...)
    call, GaussianRasterizer(...) call and call of a GaussianRasterizer instance its line, the number of positional
    arguments and its keywords (null for a **kwargs),
  * the alternative backend (gsplat_wrapper/rasterization.py): its settings fields and its forward parameter list,
  * the native module's exports (DGR/ext.cpp).
Run where the reference tree is present: `python tools/make_golden_call_sites.py [REFERENCE_ROOT]`
(default: $FROSTING_REFERENCE)."""
import ast
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLERS = ["gaussian_splatting/gaussian_renderer/__init__.py", "frosting_scene/frosting_model.py",
           "frosting_scene/sugar_model.py"]
BACKEND = "gsplat_wrapper/rasterization.py"
EXT = "gaussian_splatting/submodules/diff-gaussian-rasterization/ext.cpp"


def _calls(tree, name):
    """ast.Call nodes whose callee is the bare name `name`"""
    return [n for n in ast.walk(tree) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id == name]


def _rasterizer_calls(tree):
    """calls of a variable that the SAME function bound to `GaussianRasterizer(...)` (other functions of these files
    reuse the name `rasterizer` for a mesh rasterizer)"""
    out = []
    for fn in ast.walk(tree):
        if not isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
            continue
        names = set()
        for n in ast.walk(fn):
            if isinstance(n, ast.Assign) and isinstance(n.value, ast.Call) and isinstance(n.value.func, ast.Name) \
                    and n.value.func.id == "GaussianRasterizer":
                names |= {t.id for t in n.targets if isinstance(t, ast.Name)}
        out += [n for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in names]
    return out


def _site(c):
    return {"line": c.lineno, "positional": len(c.args), "keywords": [k.arg for k in c.keywords]}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ["FROSTING_REFERENCE"]
    parse = lambda rel: ast.parse(open(os.path.join(ref, rel)).read(), filename=rel)
    out = {"callers": {}}
    for rel in CALLERS:
        tree = parse(rel)
        imports = set()
        for n in ast.walk(tree):
            if isinstance(n, ast.ImportFrom) and n.module == "diff_gaussian_rasterization":
                imports |= {a.name for a in n.names}
        out["callers"][rel] = {
            "imports": sorted(imports),
            "settings_calls": [_site(c) for c in _calls(tree, "GaussianRasterizationSettings")],
            "rasterizer_ctor_calls": [_site(c) for c in _calls(tree, "GaussianRasterizer")],
            "rasterizer_calls": [_site(c) for c in _rasterizer_calls(tree)]}
    tree = parse(BACKEND)
    classes = {n.name: n for n in ast.walk(tree) if isinstance(n, ast.ClassDef)}
    init = next(f for f in classes["GaussianRasterizationSettings"].body if isinstance(f, ast.FunctionDef) and f.name == "__init__")
    fwd = next(f for f in classes["GaussianRasterizer"].body if isinstance(f, ast.FunctionDef) and f.name == "forward")
    out["alternative_backend"] = {"file": BACKEND, "settings_init_fields": [a.arg for a in init.args.args if a.arg != "self"],
                                  "forward_params": [a.arg for a in fwd.args.args if a.arg != "self"]}
    out["native_exports"] = {"file": EXT, "names": sorted(set(re.findall(r'm\.def\("(\w+)"', open(os.path.join(ref, EXT)).read())))}
    path = os.path.join(ROOT, "tests", "golden", "call_sites.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, {rel: {k: len(v) for k, v in d.items()} for rel, d in out["callers"].items()})


if __name__ == "__main__":
    main()
