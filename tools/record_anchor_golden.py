"""Regenerate tests/golden/anchor_roundtrip.json and tests/golden/anchor_roundtrip.npz from the reference's five anchor nodes.

    python tools/record_anchor_golden.py

Needs the reference checkout (oracle.reference_loader.REFERENCE_ROOT) and no GPU; the tests read the fixtures only and never import this
file.  VRGDG_VideoEnhanceNodes.py and VRGDG_StandaloneFaceFixNodes.py of the reference are loaded as they stand and their classes
VRGDGVideoEnhanceLoadAnchorsMetaBatch, VRGDGVideoEnhanceStoreAnchors, VRGDGVideoEnhanceCollectLTXInputs, VRGDGFaceFixLoadAnchorsMetaBatch
and VRGDGFaceFixStoreAnchors run on the CPU over a temporary folder, with a stand-in `meta_batch` (the four attributes the nodes touch),
a stub `folder_paths` and a stub `cv2` whose imwrite records what it is handed.  Written down: the small input pictures, what every
call returns, the meta-batch state after every call, the stored bytes, the folders' listings and the context dictionaries -- data only.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# file name -> (width, height): sorted by path they come as a_10.bmp, a_9.PNG, b_2.png, c_0.png, d_1.png; the other two are no images
PICTURES = (("a_10.bmp", (40, 24)), ("a_9.PNG", (97, 61)), ("b_2.png", (17, 9)), ("c_0.png", (40, 24)), ("d_1.png", (41, 24)))
IGNORED = ("notes.txt", "e_5.gif")
# (frames_per_batch, total_frames before the first call, calls made)
SCHEDULES = ((1, 100, 6), (3, 100, 3), (5, 3, 2), (7, 100, 2))
STORE_SHAPE = (3, 5, 13, 4)
SAFE_CASES = (([0, 8, 16, 24, 32], 33), ([1, 9, 17], 40), ([0, 1, 2], 3), ([9, 9, 9, 10], 12), ([1, 1, 1], 2), ([5], 0), ([], 10))


class MetaBatch:
    """what the nodes touch of VideoHelperSuite's batch manager"""

    def __init__(self, frames_per_batch, total_frames):
        self.inputs, self.frames_per_batch, self.total_frames, self.has_closed_inputs = {}, frames_per_batch, total_frames, False

    def state(self):
        return {"inputs": sorted(self.inputs), "sizes": {k: [v[1], v[2]] for k, v in self.inputs.items()}, "total_frames": self.total_frames,
                "has_closed_inputs": self.has_closed_inputs}


def picture(index, size):
    """the bytes of input picture `index`: a smooth ramp plus seeded noise.  tests/anchor_support.py reads them from the fixture."""
    w, h = size
    rng = np.random.default_rng(700 + index)
    ramp = (np.arange(h)[:, None, None] * 5 + np.arange(w)[None, :, None] * 3 + np.arange(3)[None, None, :] * 60) % 256
    return ((ramp + rng.integers(0, 96, (h, w, 3))) % 256).astype(np.uint8)


def store_input():
    """the fp32 batch the store nodes get: values outside [0, 1] on both sides, ties of the rounding, -0.0, a subnormal, the infinities, NaN"""
    import torch
    x = torch.rand(STORE_SHAPE, generator=torch.Generator().manual_seed(811)) * 1.2 - 0.1
    flat = x.reshape(-1)
    special = [0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255, -0.0, 1e-40, float("inf"), float("-inf"), float("nan"), 1.0, 0.0, 127.5 / 255]
    flat[7:7 + len(special)] = torch.tensor(special, dtype=torch.float32)
    return x.contiguous()


def run_schedule(node, context, schedule, unique_id, frames):
    fpb, total, calls = schedule
    mb = MetaBatch(fpb, total)
    record, at = {"frames_per_batch": fpb, "total_frames": total, "unique_id": unique_id, "calls": []}, 0
    for _ in range(calls):
        if str(unique_id) not in mb.inputs:
            at = 0
        try:
            images, masks, count, ctx = node.load(context, mb, unique_id)
        except FileNotFoundError as exc:
            record["calls"].append({"error": type(exc).__name__, "text": str(exc), "state": mb.state()})
            continue
        got = images.numpy()
        assert ctx is context and got.dtype == np.float32 and np.array_equal(got.view(np.uint32), frames[at:at + count].view(np.uint32))
        assert not masks.any()
        record["calls"].append({"first": at, "count": int(count), "shape": list(images.shape), "dtype": str(images.dtype),
                                "mask_shape": list(masks.shape), "mask_dtype": str(masks.dtype), "state": mb.state()})
        at += count
    return record


def main():
    import torch
    from PIL import Image
    sys.path.insert(0, ROOT)
    from oracle import reference_loader as RL
    from tools.make_golden_resize import _write_npz

    ve = RL._load_file("_vrgdg_reference_video_enhance_anchors", "VRGDG_VideoEnhanceNodes.py")
    ff = RL._load_file("_vrgdg_reference_face_fix_anchors", "VRGDG_StandaloneFaceFixNodes.py")
    ve._log = ff._log = lambda message: None
    flat, meta = {}, {"pictures": [{"name": n, "size": list(s)} for n, s in PICTURES], "ignored": list(IGNORED)}
    classes = {"VRGDGVideoEnhanceLoadAnchorsMetaBatch": ve, "VRGDGVideoEnhanceStoreAnchors": ve, "VRGDGVideoEnhanceCollectLTXInputs": ve,
               "VRGDGFaceFixLoadAnchorsMetaBatch": ff, "VRGDGFaceFixStoreAnchors": ff}
    meta["surface"] = {name: {"INPUT_TYPES": getattr(mod, name).INPUT_TYPES(), "RETURN_TYPES": list(getattr(mod, name).RETURN_TYPES),
                              "RETURN_NAMES": list(getattr(mod, name).RETURN_NAMES), "FUNCTION": getattr(mod, name).FUNCTION,
                              "CATEGORY": getattr(mod, name).CATEGORY, "OUTPUT_NODE": bool(getattr(getattr(mod, name), "OUTPUT_NODE", False)),
                              "display_name": mod.NODE_DISPLAY_NAME_MAPPINGS[name]} for name, mod in classes.items()}

    with tempfile.TemporaryDirectory() as tmp:
        sources = os.path.join(tmp, "anchor_sources")
        os.makedirs(sources)
        for i, (name, size) in enumerate(PICTURES):
            flat[f"picture.{i}"] = picture(i, size)
            Image.fromarray(flat[f"picture.{i}"], "RGB").save(os.path.join(sources, name), format="BMP" if name.endswith(".bmp") else "PNG")
        for name in IGNORED:
            with open(os.path.join(sources, name), "wb") as fh:
                fh.write(b"not an image")
        order = sorted(range(len(PICTURES)), key=lambda i: os.path.join(sources, PICTURES[i][0]))
        meta["order"] = order
        w, h = PICTURES[order[0]][1]
        frames = np.stack([np.asarray(Image.fromarray(flat[f"picture.{i}"]).resize((w, h), Image.Resampling.LANCZOS), dtype=np.float32) / 255.0
                           for i in order])
        flat["frames"] = frames
        empty = os.path.join(tmp, "empty")
        os.makedirs(empty)

        # ---- load ----
        meta["load"] = {}
        for key, node, ctx_key in (("video_enhance", ve.VRGDGVideoEnhanceLoadAnchorsMetaBatch(), "video_enhance"),
                                   ("face_fix", ff.VRGDGFaceFixLoadAnchorsMetaBatch(), "face_fix")):
            context = {"anchor_sources_folder": sources, "job_id": "job_a"}
            entry = {"schedules": [run_schedule(node, context, s, 17 + i, frames) for i, s in enumerate(SCHEDULES)], "errors": []}
            for what, bad in (("missing folder", {"anchor_sources_folder": os.path.join(tmp, "nowhere")}), ("no folder", {}),
                              ("empty folder", {"anchor_sources_folder": empty})):
                mb = MetaBatch(2, 9)
                try:
                    node.load(bad, mb, 3)
                    raise SystemExit("the reference loaded from " + what)
                except FileNotFoundError as exc:
                    entry["errors"].append({"what": what, "type": type(exc).__name__, "text": str(exc).replace(tmp, "{tmp}"), "state": mb.state()})
            meta["load"][key] = entry

        # ---- store ----
        x = store_input()
        flat["store.input"] = x.numpy().copy()
        stub_fp = types.ModuleType("folder_paths")
        stub_fp.get_output_directory = lambda: os.path.join(tmp, "output")
        written = []
        stub_cv = types.ModuleType("cv2")
        stub_cv.COLOR_RGB2BGR = 4
        stub_cv.cvtColor = lambda image, code: np.ascontiguousarray(image[..., ::-1])

        def imwrite(path, image):
            written.append((path, np.array(image)))
            Image.fromarray(np.ascontiguousarray(image[..., ::-1]), "RGB").save(path)
            return True

        stub_cv.imwrite = imwrite
        saved = {k: sys.modules.get(k) for k in ("folder_paths", "cv2")}
        sys.modules["folder_paths"], sys.modules["cv2"] = stub_fp, stub_cv
        try:
            job = os.path.join(tmp, "jobs", "job_a")
            stale = {"enhanced_anchors": ("anchor_000009.png", "old.JPG", "keep.txt")}
            os.makedirs(os.path.join(job, "enhanced_anchors"))
            for name in stale["enhanced_anchors"]:
                open(os.path.join(job, "enhanced_anchors", name), "wb").close()
            ctx_in = {"job_id": "job_a", "job_folder": job, "anchor_indices": [0, 8, 15], "fps": 24.0}
            folder, joined, count, ctx = ve.VRGDGVideoEnhanceStoreAnchors().store(x, ctx_in)
            names = sorted(os.listdir(folder))
            flat["store.video_enhance.png"] = np.stack([np.asarray(Image.open(os.path.join(folder, n)).convert("RGB")) for n in names if n.endswith(".png")])
            record = {"stale": list(stale["enhanced_anchors"]), "files_after": names, "folder": os.path.relpath(folder, job), "indices": joined,
                      "count": count, "context_in": {k: v for k, v in ctx_in.items() if k != "job_folder"},
                      "context_keys": list(ctx), "context_folder_is_folder": ctx["enhanced_anchor_folder"] == folder,
                      "context_untouched": ctx_in == {"job_id": "job_a", "job_folder": job, "anchor_indices": [0, 8, 15], "fps": 24.0}}
            try:
                ve.VRGDGVideoEnhanceStoreAnchors().store(x[:2], ctx_in)
                raise SystemExit("the reference stored a wrong count")
            except ValueError as exc:
                record["count_error"] = {"given": 2, "type": type(exc).__name__, "text": str(exc)}
            meta["store"] = {"video_enhance": record}

            out_dir = os.path.join(tmp, "output", "face_fix_standalone", "job_f", "enhanced_anchors_512")
            os.makedirs(out_dir)
            stale_ff = ("anchor_0007.png", "other.PNG", "old.jpg")
            for name in stale_ff:
                open(os.path.join(out_dir, name), "wb").close()
            ctx_in = {"job_id": "job_f", "anchor_indices": [0, 8, 15]}
            folder, joined, count, ctx = ff.VRGDGFaceFixStoreAnchors().store(x, ctx_in)
            flat["store.face_fix.bgr"] = np.stack([image for _, image in written])
            record = {"stale": list(stale_ff), "files_after": sorted(os.listdir(folder)), "written": [os.path.basename(p) for p, _ in written],
                      "folder": os.path.relpath(folder, os.path.join(tmp, "output")), "indices": joined, "count": count, "context_in": ctx_in,
                      "context_keys": list(ctx), "context_folder_is_folder": ctx["enhanced_anchor_folder"] == folder}
            try:
                ff.VRGDGFaceFixStoreAnchors().store(x[:1], ctx_in)
                raise SystemExit("the reference stored a wrong count")
            except ValueError as exc:
                record["count_error"] = {"given": 1, "type": type(exc).__name__, "text": str(exc)}
            meta["store"]["face_fix"] = record
        finally:
            for k, v in saved.items():
                if v is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = v

        # ---- collect ----
        collect = ve.VRGDGVideoEnhanceCollectLTXInputs
        meta["safe_indices"] = []
        for indices, frame_count in SAFE_CASES:
            try:
                meta["safe_indices"].append({"indices": indices, "frame_count": frame_count, "result": collect._safe_indices(indices, frame_count)})
            except ValueError as exc:
                meta["safe_indices"].append({"indices": indices, "frame_count": frame_count, "error": type(exc).__name__, "text": str(exc)})
        video = os.path.join(tmp, "ltx_working_video.mp4")
        open(video, "wb").close()
        anchors = os.path.join(tmp, "collected")
        os.makedirs(anchors)
        for name in ("anchor_000000.png", "anchor_000001.PNG", "anchor_000002.png", "ignored.jpg"):
            open(os.path.join(anchors, name), "wb").close()
        prepared = {"job_id": "job_a", "ltx_video_path": video, "frame_count": 40, "ltx_width": 960, "ltx_height": "544", "anchor_indices": [0, 16, 39],
                    "fps": 24.0}
        enhanced = {"job_id": "job_a", "enhanced_anchor_folder": anchors, "anchor_indices": [0, 17, 39]}
        out = collect().collect(prepared, enhanced)
        runs = [{"what": "ok", "returns": [out[0] == video, out[1] == anchors, out[2], out[3], out[4], out[5]],
                 "context": {k: v for k, v in out[6].items() if k not in ("ltx_video_path", "enhanced_anchor_folder")},
                 "context_keys": list(out[6]), "context_folder_is_folder": out[6]["enhanced_anchor_folder"] == anchors}]
        for what, p, e in (("other job", prepared, dict(enhanced, job_id="job_b")), ("no job", dict(prepared, job_id=""), dict(enhanced, job_id="")),
                           ("no video", dict(prepared, ltx_video_path=os.path.join(tmp, "none.mp4")), enhanced),
                           ("no folder", prepared, dict(enhanced, enhanced_anchor_folder=os.path.join(tmp, "none"))),
                           ("count", prepared, dict(enhanced, anchor_indices=[0, 17])),
                           ("unsafe", dict(prepared, frame_count=2), dict(enhanced, anchor_indices=[1, 1, 1]))):
            try:
                collect().collect(p, e)
                raise SystemExit("the reference collected: " + what)
            except (ValueError, FileNotFoundError) as exc:
                runs.append({"what": what, "error": type(exc).__name__, "text": str(exc).replace(tmp, "{tmp}")})
        meta["collect"] = {"prepared": {k: v for k, v in prepared.items() if k != "ltx_video_path"},
                           "enhanced": {k: v for k, v in enhanced.items() if k != "enhanced_anchor_folder"},
                           "files": sorted(os.listdir(anchors)), "runs": runs}

    import PIL
    meta["provenance"] = {"torch": torch.__version__, "numpy": np.__version__, "pillow": PIL.__version__,
                          "source": "the five anchor node classes of the reference's VRGDG_VideoEnhanceNodes.py and "
                                    "VRGDG_StandaloneFaceFixNodes.py, run unmodified on the CPU; meta_batch, folder_paths and cv2 are stand-ins",
                          "recorder": "tools/record_anchor_golden.py", "covers": ["anchor_roundtrip.json", "anchor_roundtrip.npz"]}
    _write_npz(os.path.join(GOLDEN, "anchor_roundtrip.npz"), flat)
    with open(os.path.join(GOLDEN, "anchor_roundtrip.json"), "w") as fh:
        json.dump(meta, fh, indent=1)
    print(f"anchor_roundtrip.npz: {len(flat)} arrays, {os.path.getsize(os.path.join(GOLDEN, 'anchor_roundtrip.npz'))} bytes")


if __name__ == "__main__":
    main()
