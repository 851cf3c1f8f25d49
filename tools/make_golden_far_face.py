"""Make tests/golden/far_face.{json,npz}: what the reference's OWN far-face backend (scripts/far_face_repair_backend.py, loaded unmodified
with an empty stand-in for cv2, which `composite` never touches) and the installed Pillow / numpy give for the seeded inputs of
tests/far_face_support.py.

    python tools/make_golden_far_face.py /path/to/reference

`soft_face_mask` and `color_match_repaired` are the reference's functions; `composite()` runs end to end through a temporary folder of PNGs
and a manifest.  Small cases store full bytes, large ones the fp32 means as bit patterns, the count, the shift and a SHA-256.  The
restatement of tests/far_face_support.py is checked against every recorded value on the way (a mismatch stops the run), the 560 x 560
random box is recorded as sequential != exact, and the steered case -- a box whose exact-mean shift and numpy-mean shift truncate
differently -- is searched for; the run fails if none is found.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import far_face_support as S  # noqa: E402


def load_reference(root):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("far_face_repair_backend", os.path.join(root, "scripts", "far_face_repair_backend.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_composite(ref, originals, repaired, masks, boxes, feather, color_match):
    """the reference's composite() through files -> the composited frames (a frame without an entry stays as it was)"""
    from PIL import Image
    with tempfile.TemporaryDirectory() as tmp:
        entries, k = [], 0
        os.makedirs(os.path.join(tmp, "crops"))
        for f, box in enumerate(boxes):
            path = os.path.join(tmp, f"original_{f:06d}.png")
            Image.fromarray(originals[f], "RGB").save(path)
            if box is None:
                continue
            name = f"frame_{f:06d}_face_00.png"
            Image.fromarray(repaired[k], "RGB").save(os.path.join(tmp, "crops", name))
            mask_path = os.path.join(tmp, "mask_" + name)
            Image.fromarray(masks[k], "L").save(mask_path)
            k += 1
            entries.append({"frame": f, "original_frame": path, "mask": mask_path, "crop_box": list(box), "repaired_name": name})
        manifest = os.path.join(tmp, "manifest.json")
        with open(manifest, "w") as fh:
            json.dump({"entries": entries}, fh)
        ref.composite(argparse.Namespace(manifest=manifest, repaired_dir="", out="", feather=feather, color_match=color_match))
        out = originals.copy()
        for e in entries:
            out[e["frame"]] = np.asarray(Image.open(os.path.join(tmp, "composited_frames", f"frame_{e['frame']:06d}.png")).convert("RGB"))
        return out


def numpy_means(x, mask):
    """the reference's own lines (:215-222)"""
    v = np.asarray(x).astype(np.float32)
    alpha = np.asarray(mask).astype(np.float32) / 255.0
    selected = alpha > 0.25
    return int(selected.sum()), v[selected].mean(axis=0)


def means_record(ref, key, o, r, m):
    from PIL import Image
    count, om = numpy_means(o, m)
    _, rm = numpy_means(r, m)
    adjusted = np.asarray(ref.color_match_repaired(Image.fromarray(o, "RGB"), Image.fromarray(r, "RGB"), Image.fromarray(m, "L")))
    shift = ((om - rm) * 0.65).astype(np.float32)
    got, c2, om2, rm2, shift2 = S.color_match(o, r, m)
    assert c2 == count and S.bits(om2) == S.bits(om) and S.bits(rm2) == S.bits(rm) and S.bits(shift2) == S.bits(shift), key
    assert np.array_equal(got, adjusted), key
    _, eom = S.exact_means(o, m)
    return {"key": key, "count": count, "original_mean_bits": S.bits(om), "repaired_mean_bits": S.bits(rm), "shift_bits": S.bits(shift),
            "exact_original_mean_bits": S.bits(eom), "sequential_differs_from_exact": S.bits(eom) != S.bits(om), "sha256": sha(adjusted)}


def steer(ref):
    n = 400 * 400
    k = 0
    for _ in range(16):
        frames, rep, masks = S.steered_inputs(k)
        left, top, right, bottom = S.STEERED_BOX
        o = frames[0, top:bottom, left:right]
        (_, om), (_, rm) = S.sequential_means(o, masks[0]), S.sequential_means(rep[0], masks[0])
        (_, eo), (_, er) = S.exact_means(o, masks[0]), S.exact_means(rep[0], masks[0])
        s_seq = float(((om - rm) * np.float32(0.65))[0])
        s_ex = float(((eo - er) * np.float32(0.65))[0])
        if s_seq != s_ex and np.floor(s_seq) != np.floor(s_ex):
            want = run_composite(ref, frames, rep, masks, [S.STEERED_BOX], -1, True)
            other = S.composite(frames, rep, [S.STEERED_BOX], -1, True, masks, means=S.exact_means)
            mine = S.composite(frames, rep, [S.STEERED_BOX], -1, True, masks)
            assert np.array_equal(mine, want), "the restatement misses the reference on the steered case"
            differing = int((other != want).sum())
            assert differing > 0, "the steered case does not tell the two routes apart"
            return {"k": int(k), "shift_sequential": s_seq, "shift_exact": s_ex, "differing_bytes": differing, "sha256": sha(want),
                    "exact_route_sha256": sha(other)}
        if s_seq == s_ex:
            raise SystemExit("steered case: the two routes give the same shift")
        mid = (s_seq + s_ex) / 2.0
        k += int(round((round(mid) - mid) / 0.65 * n))
    raise SystemExit("steered case: no input found whose exact-mean shift and numpy-mean shift truncate differently")


def main():
    import PIL
    from PIL import Image
    ap = argparse.ArgumentParser()
    ap.add_argument("reference")
    args = ap.parse_args()
    ref = load_reference(args.reference)
    arrays = {}
    meta = {"made_by": "tools/make_golden_far_face.py", "pillow": PIL.__version__, "numpy": np.__version__,
            "source": "scripts/far_face_repair_backend.py: soft_face_mask, color_match_repaired, composite"}

    meta["resize"] = []
    for i, ((iw, ih), (ow, oh)) in enumerate(S.RESIZE_CASES):
        for c in (3, 0):
            img = S.random_image(3000 + i, ih, iw, c)
            want = np.asarray(Image.fromarray(img).resize((ow, oh), Image.Resampling.LANCZOS))
            assert np.array_equal(S.resize(img, (ow, oh)), want), (iw, ih, ow, oh, c)
            key = f"resize.{iw}x{ih}.{ow}x{oh}.{'RGB' if c else 'L'}"
            arrays[key] = want
            meta["resize"].append({"key": key, "in": [iw, ih], "out": [ow, oh], "channels": c, "seed": 3000 + i, "sha256": sha(want)})

    meta["masks"] = []
    for size in S.MASK_SIZES:
        for feather in S.FEATHERS:
            want = np.asarray(ref.soft_face_mask(size, feather))
            assert np.array_equal(S.soft_face_mask(size, feather), want), (size, feather)
            key = f"mask.{size[0]}x{size[1]}.{feather}"
            arrays[key] = want
            meta["masks"].append({"key": key, "size": list(size), "feather": feather, "sha256": sha(want)})

    meta["means"] = [means_record(ref, key, *S.means_inputs(key)) for key in S.MEANS_CASES]
    assert {m["key"]: m["sequential_differs_from_exact"] for m in meta["means"]}["560_random"], "560 x 560 random: sequential == exact"

    originals, repaired, masks = S.composite_inputs()
    meta["composites"] = []
    for i, (feather, cm) in enumerate(S.COMPOSITE_VARIANTS):
        want = run_composite(ref, originals, repaired, masks, S.COMPOSITE_BOXES, feather, cm)
        assert np.array_equal(S.composite(originals, repaired, S.COMPOSITE_BOXES, feather, cm, masks), want), (feather, cm)
        assert np.array_equal(want[4], originals[4])
        stored = []
        for f, box in enumerate(S.COMPOSITE_BOXES):
            full = box is not None and (box[2] - box[0]) * (box[3] - box[1]) > 4000
            if box is not None and (not full or (feather, cm) in ((18, True), (-1, True))):
                arrays[f"composite.{i}.{f}"] = want[f, box[1]:box[3], box[0]:box[2]]
                stored.append(f)
        meta["composites"].append({"feather": feather, "color_match": cm, "frame_sha256": [sha(want[f]) for f in range(len(want))],
                                   "stored_boxes": stored})

    frames, rep = S.large_inputs()
    want = run_composite(ref, frames, rep, [np.zeros((4, 4), np.uint8)], [S.LARGE_BOX], 18, True)
    assert np.array_equal(S.composite(frames, rep, [S.LARGE_BOX], 18, True), want)
    left, top, right, bottom = S.LARGE_BOX
    resized = np.asarray(Image.fromarray(rep[0]).resize((right - left, bottom - top), Image.Resampling.LANCZOS))
    mask = np.asarray(ref.soft_face_mask((right - left, bottom - top), 18))
    rec = means_record(ref, "large", frames[0, top:bottom, left:right], resized, mask)
    rec["sha256"] = sha(want)
    meta["large"] = rec

    meta["steered"] = steer(ref)

    np.savez_compressed(S.FIXTURE_NPZ, **arrays)
    with open(S.FIXTURE_JSON, "w") as fh:
        json.dump(meta, fh, indent=1)
        fh.write("\n")
    print(os.path.getsize(S.FIXTURE_NPZ), os.path.getsize(S.FIXTURE_JSON))
    print(json.dumps(meta["steered"]))


if __name__ == "__main__":
    main()
