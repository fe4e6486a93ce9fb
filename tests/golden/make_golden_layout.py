#!/usr/bin/env python3
"""Module inventory of the reference tree for tests/test_dropin_packages.py: which modules its packages hold (fusions, layers, lib,
models, utils; top level of each) and the public names each one defines at module level (functions, classes, assigned names).
Names only -- no source: the test builds a stand-in tree from it, so that the drop-in packages are checked against the
reference's layout without the reference itself.

    python tests/golden/make_golden_layout.py <reference checkout>      (or IMMTSF_REFERENCE=<checkout>)

Writes tests/golden/reference_layout.json.
"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PACKAGES = ("fusions", "layers", "lib", "models", "utils")


def public_names(path):
    tree = ast.parse(open(path, encoding="utf-8").read(), filename=path)
    names = []
    for node in tree.body:
        if isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
            names.append(node.name)
        elif isinstance(node, ast.Assign):
            names.extend(t.id for t in node.targets if isinstance(t, ast.Name))
        elif isinstance(node, ast.AnnAssign) and isinstance(node.target, ast.Name):
            names.append(node.target.id)
    return sorted({n for n in names if not n.startswith("_")})


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("IMMTSF_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit(__doc__)
    layout = {}
    for pkg in PACKAGES:
        d = os.path.join(ref, pkg)
        if not os.path.isdir(d):
            continue
        layout[pkg] = {f[:-3]: public_names(os.path.join(d, f)) for f in sorted(os.listdir(d))
                       if f.endswith(".py") and os.path.isfile(os.path.join(d, f))}
    with open(os.path.join(HERE, "reference_layout.json"), "w") as fh:
        json.dump(layout, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
