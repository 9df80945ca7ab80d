#!/usr/bin/env python
"""g28_main_3dident.json: what the reference's 3DIdent driver says about its own command line and latent-space set-up, recorded by
READING main_3dident.py with `ast` (the module cannot be imported: it parses sys.argv and needs faiss / torchvision) -- nothing of its
text is kept here or in the fixture.

Run only in the build container (the reference never travels to the GPU box):
    python tests/golden/gen_goldens_3dident_driver.py

  cli      every parser.add_argument call: flag, default, type name, choices, action, required (ast.literal_eval of its arguments)
  latent   the reference's own setup_latent_space -- its function node compiled and run against the reference's `spaces` /
           `latent_spaces` -- over 40 flag combinations (at most one of the four *-only flags, times the three boolean flags):
           (dim, n_non_angular, n_angular, class name) and the factor spaces (kind, dimension), or the exception's class name;
           and, per combination, what the module-level column selection (`latent_dimensions_to_use = None` and the `if` behind it)
           leaves in `latent_dimensions_to_use`, or the class of what it raises
"""
import argparse
import ast
import itertools
import json
import os
import sys

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ONLY = [None, "position_only", "rotation_and_color_only", "rotation_only", "color_only"]
BOOLS = ["non_periodic_rotation_and_color", "no_spotlight_position", "no_spotlight_color"]


def cli_table(tree):
    rows = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument":
            kw = {k.arg: k.value for k in node.keywords}
            row = dict(flag=ast.literal_eval(node.args[0]), default=None, type=None, choices=None, action=None, required=False)
            for key in ("default", "choices", "action", "required"):
                if key in kw:
                    v = ast.literal_eval(kw[key])
                    row[key] = list(v) if isinstance(v, tuple) else v
            if "type" in kw:
                row["type"] = kw["type"].id
            rows.append(row)
    rows.sort(key=lambda r: r["flag"])
    return rows


def factor_spaces(ls):
    factors = ls.spaces if hasattr(ls, "spaces") else [ls]
    return [[type(f.space).__name__, int(f.space.dim)] for f in factors]


def latent_table(tree):
    sys.path.insert(0, REF)
    import latent_spaces
    import spaces
    (fn,) = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "setup_latent_space"]
    scope = dict(spaces=spaces, latent_spaces=latent_spaces)
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "<setup_latent_space>", "exec"), scope)
    (k,) = [i for i, n in enumerate(tree.body) if isinstance(n, ast.Assign) and len(n.targets) == 1
            and getattr(n.targets[0], "id", None) == "latent_dimensions_to_use" and isinstance(n.value, ast.Constant)]
    assert isinstance(tree.body[k + 1], ast.If)
    select = compile(ast.Module(body=tree.body[k:k + 2], type_ignores=[]), "<latent_dimensions_to_use>", "exec")
    rows = []
    for only, bools in itertools.product(ONLY, itertools.product([False, True], repeat=len(BOOLS))):
        flags = {k: False for k in ONLY[1:]}
        if only:
            flags[only] = True
        flags.update(dict(zip(BOOLS, bools)))
        args = argparse.Namespace(sigma=0.1, non_periodical_conditional="l2", **flags)
        row = dict(flags={k: v for k, v in flags.items() if v})
        try:
            ls, n_non_angular, n_angular = scope["setup_latent_space"](args)
            row.update(dim=int(ls.dim), n_non_angular=int(n_non_angular), n_angular=int(n_angular), cls=type(ls).__name__,
                       factors=factor_spaces(ls))
        except Exception as e:      # noqa: BLE001  (the class of whatever the reference raises is the record)
            row.update(error=type(e).__name__)
        try:
            sel = dict(args=args)
            exec(select, sel)
            row.update(columns=sel["latent_dimensions_to_use"])
        except Exception as e:      # noqa: BLE001
            row.update(columns_error=type(e).__name__)
        rows.append(row)
    return rows


def main():
    tree = ast.parse(open(os.path.join(REF, "main_3dident.py")).read())
    out = dict(cli=cli_table(tree), latent=latent_table(tree))
    assert len(out["cli"]) == 33 and len(out["latent"]) == 40, (len(out["cli"]), len(out["latent"]))
    path = os.path.join(HERE, "g28_main_3dident.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
