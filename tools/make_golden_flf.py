"""Record tests/golden/flf_guide.json from the reference's own VRGDG_LTXFirstLastGuide class (numbers, names and settings only).

    python tools/make_golden_flf.py            # needs the reference checkout (VRGDG_REFERENCE_ROOT); no GPU

The class is taken from the reference's source by its AST and executed as it stands, with two stand-ins for what ComfyUI brings:
``LTXVAddGuide.encode`` records the guide batch it is handed and returns a latent of the asked shape, and ``comfy.utils.common_upscale``
records the view it narrows -- by the published function's centre-crop rule, written out here (comfy is not installed; see DESIGN.md
section 4) -- and resamples it with F.interpolate.  Recorded:
  surface   INPUT_TYPES, RETURN_TYPES, RETURN_NAMES, FUNCTION, CATEGORY, the display name
  curves    _curve at a few points, by name
  weights   (1.0 - amount, amount) per frame as fp32, read off a guide batch of 1 x 1 pictures (1, 0, .) and (0, 1, .)
  rects     the narrowed view per (old size, new size), among them pairs whose half surplus lands on .5
  node      what the node hands the encoder and returns: frame count, sizes, noise_mask, latent keys, both error texts
"""
import ast
import json
import os
import sys
import types

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_ROOT = os.environ.get("VRGDG_REFERENCE_ROOT", "/root/reference")
FILENAME = "VRGDG_LTXFirstLastGuide.py"
CLASS = "VRGDG_LTXFirstLastGuide"

WEIGHT_CASES = [(1, 0.05, 0.90, "smoothstep"), (2, 0.05, 0.90, "smoothstep"), (9, 0.05, 0.90, "smoothstep"), (9, 0.05, 0.90, "linear"),
                (9, 0.05, 0.90, "ease_in"), (9, 0.05, 0.90, "ease_out"), (9, 0.5, 0.90, "linear"), (9, 0.5, 0.52, "smoothstep"),
                (33, 0.0, 1.0, "ease_out"), (33, 0.95, 0.05, "ease_in"), (97, 0.05, 0.90, "smoothstep"), (121, 0.2, 0.7, "linear"),
                (257, 0.05, 0.90, "smoothstep"), (9, 2.0, -1.0, "no such curve")]
# (old_w, old_h, new_w, new_h)
RECT_CASES = [(29, 33, 37, 20), (13, 5, 5, 7), (48, 64, 12, 16), (2, 3, 40, 24), (4000, 3000, 1280, 736), (4000, 3000, 1920, 1080),
              (3000, 4000, 736, 1280), (1920, 1080, 1280, 736), (1024, 1024, 1280, 736), (7, 7, 7, 7), (10, 10, 8, 8), (640, 480, 480, 640)]


class Recorder:
    def __init__(self):
        self.rects, self.encoded, self.latent_shape = [], [], None

    def common_upscale(self, samples, width, height, upscale_method, crop):
        assert upscale_method == "bilinear" and crop == "center"
        old_width, old_height = samples.shape[-1], samples.shape[-2]
        old_aspect, new_aspect = old_width / old_height, width / height
        x = y = 0
        if old_aspect > new_aspect:
            x = round((old_width - old_width * (new_aspect / old_aspect)) / 2)
        elif old_aspect < new_aspect:
            y = round((old_height - old_height * (old_aspect / new_aspect)) / 2)
        self.rects.append([x, y, old_width - x * 2, old_height - y * 2])
        view = samples.narrow(-2, y, old_height - y * 2).narrow(-1, x, old_width - x * 2)
        return F.interpolate(view, size=(height, width), mode=upscale_method)

    def encode(self, vae, width, height, guide_video, formula):
        self.encoded.append({"width": width, "height": height, "frames": guide_video})
        return guide_video, torch.zeros(self.latent_shape, dtype=torch.float16)


def load_class(recorder):
    path = os.path.join(REFERENCE_ROOT, FILENAME)
    with open(path, "r", encoding="utf-8") as fh:
        tree = ast.parse(fh.read(), filename=path)
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == CLASS]
    display = next(ast.literal_eval(n.value) for n in tree.body
                   if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "NODE_DISPLAY_NAME_MAPPINGS")[CLASS]
    comfy = types.SimpleNamespace(utils=types.SimpleNamespace(common_upscale=recorder.common_upscale))
    ns = {"torch": torch, "comfy": comfy, "LTXVAddGuide": types.SimpleNamespace(encode=recorder.encode)}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return ns[CLASS], display


def run(cls, rec, first, last, latent_shape, encoded_shape, time_scale=8, **kw):
    rec.latent_shape = encoded_shape
    vae = types.SimpleNamespace(downscale_index_formula=(time_scale, 32, 32))
    latent = {"samples": torch.zeros(latent_shape), "batch_index": [0]}
    return cls().add_first_last_guide("P", "N", vae, latent, first, last, **kw)


def half_pairs():
    """pairs whose half surplus is k + 0.5: Python's round (half to even) and round-half-up part ways where k is even"""
    found = []
    for old_w, old_h, new_w, new_h in ((5, 4, 2, 2), (4, 5, 2, 2), (9, 4, 3, 3), (13, 8, 4, 4), (8, 13, 4, 4), (7, 6, 3, 3)):
        old_aspect, new_aspect = old_w / old_h, new_w / new_h
        half = ((old_w - old_w * (new_aspect / old_aspect)) if old_aspect > new_aspect else (old_h - old_h * (old_aspect / new_aspect))) / 2
        if half % 1 == 0.5:
            found.append((old_w, old_h, new_w, new_h))
    return found


def main():
    rec = Recorder()
    cls, display = load_class(rec)
    out = {"surface": {"INPUT_TYPES": cls.INPUT_TYPES(), "RETURN_TYPES": list(cls.RETURN_TYPES), "RETURN_NAMES": list(cls.RETURN_NAMES),
                       "FUNCTION": cls.FUNCTION, "CATEGORY": cls.CATEGORY, "display_name": display}}
    points = [0.0, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.9, 1.0]
    out["curves"] = {"points": points, "values": {name: [cls._curve(p, name) for p in points]
                                                  for name in ("smoothstep", "linear", "ease_in", "ease_out", "no such curve")}}
    first, last = torch.tensor([1.0, 0.0, 0.5]).reshape(1, 1, 1, 3), torch.tensor([0.0, 1.0, 0.5]).reshape(1, 1, 1, 3)
    out["weights"] = []
    for frames, start, end, curve in WEIGHT_CASES:
        del rec.encoded[:]
        length = (frames - 1) // 8 + 1
        assert (length - 1) * 8 + 1 == frames or frames == 2
        if frames == 2:
            run(cls, rec, first, last, (1, 4, 2, 1, 1), (1, 4, 2, 1, 1), time_scale=1, transition_start=start, transition_end=end, curve=curve)
        else:
            run(cls, rec, first, last, (1, 4, length, 1, 1), (1, 4, length, 1, 1), transition_start=start, transition_end=end, curve=curve)
        video = rec.encoded[0]["frames"]
        assert tuple(video.shape) == (frames, 1, 1, 3) and video.dtype == torch.float32
        out["weights"].append({"frame_count": frames, "transition_start": start, "transition_end": end, "curve": curve,
                               "weights": [[float(a), float(b)] for a, b, _ in video.reshape(frames, 3).tolist()]})
    out["rects"] = []
    halves = half_pairs()
    for old_w, old_h, new_w, new_h in RECT_CASES + halves:
        del rec.rects[:]
        run(cls, rec, torch.zeros(1, new_h, new_w, 3), torch.zeros(1, old_h, old_w, 3), (1, 4, 1, 1, 1), (1, 4, 1, 1, 1))
        assert len(rec.rects) == (0 if (old_w, old_h) == (new_w, new_h) else 1)
        out["rects"].append({"old": [old_w, old_h], "new": [new_w, new_h], "half": (old_w, old_h, new_w, new_h) in halves,
                             "rect": rec.rects[0] if rec.rects else None})
    # the node: a [2, 128, 5, 4, 6] latent, time scale 8 -> 33 frames; batch of 3 first images, 2 last images
    del rec.encoded[:]
    pos, neg, result = run(cls, rec, torch.rand(3, 4, 6, 3), torch.rand(2, 4, 6, 3), (2, 128, 5, 4, 6), (1, 128, 5, 2, 3), guide_strength=0.35)
    enc = rec.encoded[0]
    node = {"latent_shape": [2, 128, 5, 4, 6], "encoded_shape": [1, 128, 5, 2, 3], "time_scale": 8, "guide_strength": 0.35,
            "encoder": {"width": enc["width"], "height": enc["height"], "frames_shape": list(enc["frames"].shape)},
            "returns": [pos, neg], "keys": sorted(result), "samples_shape": list(result["samples"].shape),
            "noise_mask": {"shape": list(result["noise_mask"].shape), "dtype": str(result["noise_mask"].dtype),
                           "value": float(result["noise_mask"].flatten()[0])}, "errors": {}}
    for name, shape in (("latent_frames", (1, 128, 4, 2, 3)), ("channels", (1, 64, 5, 2, 3))):
        try:
            run(cls, rec, torch.rand(1, 4, 6, 3), torch.rand(1, 4, 6, 3), (2, 128, 5, 4, 6), shape)
            raise AssertionError("no error")
        except ValueError as exc:
            node["errors"][name] = {"encoded_shape": list(shape), "message": str(exc)}
    strengths = []
    for s in (-1.0, 0.0, 0.35, 1.0, 7.0):
        _, _, r = run(cls, rec, torch.rand(1, 4, 6, 3), torch.rand(1, 4, 6, 3), (1, 128, 1, 4, 6), (1, 128, 1, 2, 3), guide_strength=s)
        strengths.append([s, float(r["noise_mask"].flatten()[0])])
    node["strengths"] = strengths
    out["node"] = node
    path = os.path.join(ROOT, "tests", "golden", "flf_guide.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(path, os.path.getsize(path), "bytes;", len(halves), "half pairs")


if __name__ == "__main__":
    sys.exit(main())
