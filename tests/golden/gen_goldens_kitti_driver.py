#!/usr/bin/env python
"""g29_main_kitti.json: what the reference's KITTI-masks driver says about its own command line, recorded by READING main_kitti.py
with `ast` (the module is never imported or executed: it runs `pip install` at import) -- nothing of its text is kept here or in the
fixture, which holds names and literals only.

Run only in the build container (the reference never travels to the GPU box):
    python tests/golden/gen_goldens_kitti_driver.py

  cli      every parser.add_argument call: flag, default, type name, choices, action (ast.literal_eval of its arguments)
"""
import ast
import json
import os

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def cli_table(tree):
    rows = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == "add_argument":
            kw = {k.arg: k.value for k in node.keywords}
            row = dict(flag=ast.literal_eval(node.args[0]), default=None, type=None, choices=None, action=None)
            for key in ("default", "choices", "action"):
                if key in kw:
                    v = ast.literal_eval(kw[key])
                    row[key] = list(v) if isinstance(v, tuple) else v
            if "type" in kw:
                row["type"] = kw["type"].id
            rows.append(row)
    rows.sort(key=lambda r: r["flag"])
    return rows


def main():
    tree = ast.parse(open(os.path.join(REF, "main_kitti.py")).read())
    out = dict(cli=cli_table(tree))
    assert len(out["cli"]) == 37, len(out["cli"])
    path = os.path.join(HERE, "g29_main_kitti.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
