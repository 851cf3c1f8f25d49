"""Record tests/golden/guider_surface.json from the reference's own VRGDGLTXSigmaAdvancedGuider class (names and settings only).

    python tools/make_golden_guider.py            # needs the reference checkout (VRGDG_REFERENCE_ROOT); no GPU

The node class is taken from the reference's CustomLTXNodes.py by its AST and executed as it stands (it needs nothing of ComfyUI until a
guider is built).  Recorded: INPUT_TYPES, RETURN_TYPES, RETURN_NAMES, FUNCTION, CATEGORY, DESCRIPTION, the mapping key and display name.
"""
import ast
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("VRGDG_REFERENCE_ROOT", "/root/reference")
FILENAME = "CustomLTXNodes.py"
CLASS = "VRGDGLTXSigmaAdvancedGuider"


def main():
    path = os.path.join(REFERENCE_ROOT, FILENAME)
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == CLASS]
    ns = {"torch": torch, "math": math}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    cls = ns[CLASS]
    mappings = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and ast.unparse(node.targets[0]) in ("NODE_CLASS_MAPPINGS", "NODE_DISPLAY_NAME_MAPPINGS"):
            mappings[ast.unparse(node.targets[0])] = {ast.literal_eval(k): ast.unparse(v) for k, v in zip(node.value.keys, node.value.values)}
    key = next(k for k, v in mappings["NODE_CLASS_MAPPINGS"].items() if v == CLASS)
    out = {"key": key, "class": CLASS, "display_name": ast.literal_eval(mappings["NODE_DISPLAY_NAME_MAPPINGS"][key]),
           "INPUT_TYPES": cls.INPUT_TYPES(), "RETURN_TYPES": list(cls.RETURN_TYPES), "RETURN_NAMES": list(cls.RETURN_NAMES),
           "FUNCTION": cls.FUNCTION, "CATEGORY": cls.CATEGORY, "DESCRIPTION": cls.DESCRIPTION}
    target = os.path.join(ROOT, "tests", "golden", "guider_surface.json")
    with open(target, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(target, os.path.getsize(target), "bytes")


if __name__ == "__main__":
    sys.exit(main())
