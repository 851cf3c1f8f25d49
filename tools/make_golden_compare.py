"""Record tests/golden/compare_paths.json from the reference's own VRGDG_VideoCompareNode.py (inputs, folder listings, results and names
only).

    python tools/make_golden_compare.py           # needs the reference checkout (VRGDG_REFERENCE_ROOT); no GPU

`_video_path_candidates`, `_resolve_video_path`, their suffix set and the node class are taken from the reference's file by its AST and
executed as they stand over temporary folders, with a stand-in for ComfyUI's folder_paths.  Recorded per case: the value (a tuple as
{"tuple": [...]}), the files that exist, the candidates and the resolved path or the error; every path under the temporary root is
written as {tmp}/..., and the run's working folder is {tmp}/cwd.  Also recorded: the node's surface (INPUT_TYPES and friends, the
mapping key and the display name).
"""
import ast
import json
import os
import sys
import tempfile
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.reference_loader import REFERENCE_ROOT  # noqa: E402

FILENAME = "VRGDG_VideoCompareNode.py"
CLASS = "VRGDG_VideoCompareSlider"
FOLDERS = ("output", "temp", "input", "cwd")

VHS = ["{tmp}/output/clip_00001.png", "{tmp}/output/clip_00001.mp4", "{tmp}/output/clip_00001-audio.mp4"]
#: (name, value, files that exist)
CASES = [
    ("metadata png, silent and -audio mp4", {"tuple": [True, VHS]}, ["output/clip_00001.png", "output/clip_00001.mp4", "output/clip_00001-audio.mp4"]),
    ("the -audio mp4 was not written", {"tuple": [True, VHS]}, ["output/clip_00001.png", "output/clip_00001.mp4"]),
    ("bare absolute string", "{tmp}/input/a.mov", ["input/a.mov"]),
    ("bare relative string, found under temp", "b.webm", ["temp/b.webm"]),
    ("bare relative string, output before temp and input", "c.mkv", ["input/c.mkv", "temp/c.mkv", "output/c.mkv"]),
    ("bare relative string, the working folder first", "d.avi", ["cwd/d.avi", "output/d.avi"]),
    ("relative string with a folder", "sub/e.m4v", ["output/sub/e.m4v"]),
    ("quoted string with blanks around it", "  \"{tmp}/output/f.mp4\" ", ["output/f.mp4"]),
    ("upper-case suffix", "G.MP4", ["input/G.MP4"]),
    ("list of strings: the last that exists", ["h1.mp4", "h2.mp4", "h3.mp4"], ["output/h1.mp4", "output/h2.mp4"]),
    ("dictionary: name keys, then list keys", {"filename": "i1.mp4", "fullpath": "{tmp}/output/i2.mp4", "files": ["i3.mp4"], "gifs": ["i4.gif"],
                                              "other": "i5.mp4"}, ["output/i1.mp4", "output/i2.mp4", "output/i3.mp4", "output/i4.gif", "output/i5.mp4"]),
    ("dictionary inside a tuple", {"tuple": [True, [{"path": "j.mp4"}]]}, ["temp/j.mp4"]),
    ("missing file", {"tuple": [True, ["{tmp}/output/k.mp4"]]}, []),
    ("wrong extension only", {"tuple": [True, ["{tmp}/output/l.png", "{tmp}/output/l.gif"]]}, ["output/l.png", "output/l.gif"]),
    ("wrong extension last, a video before it", ["m.mp4", "m.png"], ["output/m.mp4", "output/m.png"]),
    ("a folder with a video suffix is no file", "n.mp4", ["output/n.mp4/"]),
    ("nothing connected", None, []),
    ("empty string", "", []),
    ("a number", 7, []),
]


def decoded(value, tmp):
    """the recorded value as the node receives it"""
    if isinstance(value, str):
        return value.replace("{tmp}", tmp)
    if isinstance(value, dict) and set(value) == {"tuple"}:
        return tuple(decoded(v, tmp) for v in value["tuple"])
    if isinstance(value, dict):
        return {k: decoded(v, tmp) for k, v in value.items()}
    if isinstance(value, list):
        return [decoded(v, tmp) for v in value]
    return value


def lay_out(tmp, files):
    for folder in FOLDERS:
        os.makedirs(os.path.join(tmp, folder), exist_ok=True)
    for name in files:
        path = os.path.join(tmp, name)
        if name.endswith("/"):
            os.makedirs(path, exist_ok=True)
            continue
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as fh:
            fh.write(b"video")


def folder_paths_stub(tmp):
    stub = types.ModuleType("folder_paths")
    stub.get_output_directory = lambda: os.path.join(tmp, "output")
    stub.get_temp_directory = lambda: os.path.join(tmp, "temp")
    stub.get_input_directory = lambda: os.path.join(tmp, "input")
    return stub


def main():
    path = os.path.join(REFERENCE_ROOT, FILENAME)
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    wanted = {"_video_path_candidates", "_resolve_video_path", CLASS}
    body = [n for n in tree.body if (isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in wanted)
            or (isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "_VIDEO_EXTENSIONS")]
    ns = {"os": os}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    cases = []
    here = os.getcwd()
    for name, value, files in CASES:
        with tempfile.TemporaryDirectory() as tmp:
            tmp = os.path.realpath(tmp)
            lay_out(tmp, files)
            ns["folder_paths"] = folder_paths_stub(tmp)
            os.chdir(os.path.join(tmp, "cwd"))
            try:
                given = decoded(value, tmp)
                rec = {"name": name, "value": value, "files": files,
                       "candidates": [c.replace(tmp, "{tmp}") for c in ns["_video_path_candidates"](given)]}
                try:
                    rec["path"] = ns["_resolve_video_path"](given, "Before").replace(tmp, "{tmp}")
                except ValueError as exc:
                    rec["error"], rec["text"] = type(exc).__name__, str(exc)
            finally:
                os.chdir(here)
            cases.append(rec)
    cls = ns[CLASS]
    mappings = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and ast.unparse(node.targets[0]) in ("NODE_CLASS_MAPPINGS", "NODE_DISPLAY_NAME_MAPPINGS"):
            mappings[ast.unparse(node.targets[0])] = {ast.literal_eval(k): ast.unparse(v) for k, v in zip(node.value.keys, node.value.values)}
    key = next(k for k, v in mappings["NODE_CLASS_MAPPINGS"].items() if v == CLASS)
    surface = {"key": key, "class": CLASS, "display_name": ast.literal_eval(mappings["NODE_DISPLAY_NAME_MAPPINGS"][key]),
               "INPUT_TYPES": cls.INPUT_TYPES(), "RETURN_TYPES": list(cls.RETURN_TYPES), "RETURN_NAMES": list(cls.RETURN_NAMES),
               "FUNCTION": cls.FUNCTION, "OUTPUT_NODE": bool(cls.OUTPUT_NODE), "CATEGORY": cls.CATEGORY}
    out = {"source": FILENAME, "label": "Before", "folders": list(FOLDERS), "suffixes": sorted(ns["_VIDEO_EXTENSIONS"]), "cases": cases,
           "surface": surface}
    target = os.path.join(ROOT, "tests", "golden", "compare_paths.json")
    with open(target, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(target, os.path.getsize(target), "bytes;", sum("path" in c for c in cases), "resolved,", sum("error" in c for c in cases), "refused")


if __name__ == "__main__":
    sys.exit(main())
