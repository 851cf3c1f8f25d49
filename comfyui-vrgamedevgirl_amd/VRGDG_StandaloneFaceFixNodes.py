"""Face Fix on the MI355X: the crop sequence of the reference's Prepare nodes and its three composite nodes.

`VRGDGFaceFixComposite`, `VRGDGFaceFixCompositeOpaque` and `VRGDGFaceFixCompositeLandmarkAligned` of the reference's
VRGDG_StandaloneFaceFixNodes.py with the same names, widget specs, tooltips, messages and log lines; the pixels come from
csrc/vrg_composite.hip (ops.composite_frames, ops.aligned_composite_frames).

`VRGDGFaceFixCompositeLandmarkAligned` runs in three phases: the bicubic face of every box as bytes on the GPU (ops.face_bytes, one
launch, downloaded once); a host loop over the frames in order that asks the node's `estimator(source_u8, generated_u8) -> 2 x 3 | None`
and keeps the reference's smoothing / reset bookkeeping in float32 numpy (aligned_transforms); one composite pass in which the frames with
a transform blend cv2's byte Lanczos-4 affine warp of those bytes (csrc/vrg_warp_math.hpp) and the others the bicubic face.  Detection
is a seam: `estimator` is a class attribute, None by default -- the reference's behaviour when its detector cannot be created: every frame
takes the fallback path and the result is the opaque composite's.  INTEGRATION.md binds the reference's detector to it.  A finer seam
moves the estimator's first act -- cv2.resize(face, (320, 320), INTER_AREA) and the R,G,B -> B,G,R flip -- to the GPU as well: with
`landmark_detector(bgr_320) -> faces | None` and `transform_fit(generated_points, source_points) -> 2 x 3 | None` set (and no
`estimator`), phase 1 makes the 320 x 320 thumbnails of both faces in one more launch (ops.face_thumbs, csrc/vrg_thumbs.hip) and downloads
those alone, 614,400 bytes per frame whatever the box; `landmark_points` scales the detector's rows back to the box on the host and
`cv2_landmark_seams()` builds both callables on cv2's FaceDetectorYN where cv2 and the model file exist.  The module's
NODE_CLASS_MAPPINGS keeps its two keys (an existing test pins that set); the new node is listed in LANDMARK_NODE_CLASS_MAPPINGS /
LANDMARK_NODE_DISPLAY_NAME_MAPPINGS beside them.

`face_crop_sequence` is the outgoing half: the video and its tracked face boxes (the `entries` a Prepare node builds) become the
512 x 512 face video that LTX repairs and the composites paste back.  The reference crops frame by frame (slice, permute, bicubic
F.interpolate, permute, clamp), fills the frames without a face with copies, prefixes copies of the first crop and stacks the list; here
the whole batch -- crops, filled holes, prefix -- is one launch of csrc/vrg_crop.hip (ops.crop_frames), and of CPU frames only the boxes
are uploaded (ops.crop_frames_host).

The reference composites frame by frame in Python (about twenty eager ops, a host synchronisation and a boolean gather per frame, a full
clone of the originals); here the whole batch is two small measuring launches and one pass over the output, and whether a frame's colour
match applies (at least 16 pixels with alpha > 0.35) is decided on the device.  CPU originals (what ComfyUI hands a node) stream through
the host-fed pipeline of _devices in pieces along the frame axis, the much smaller work frames are uploaded once ahead; device tensors are
processed where they are.  Inputs are never written.  The repaired count is computed on the host from the entries.

`shot_cut_scores` / `shot_boundaries` are the hard-cut detection of the two shot-aware Prepare nodes (`_cut_score`, :421-435, called per
frame at :457): a whole-frame reduction that depends on nothing but the video, so it runs for the whole batch before the detection loop.
Every frame is quantised to bytes and reduced to cv2's 64 x 64 INTER_AREA thumbnail in one launch of csrc/vrg_cut.hip (the frame is
read once, 12 B per pixel); two small launches turn the thumbnails into hue / saturation histograms and into four exact integers per
consecutive pair, and the host finishes the score in double (cut_scores_from_sums).  CPU frames go up through the staging pipeline of
_devices; nothing but 32 bytes per pair comes back.  The `shot_id` values are what face_crop_sequence(..., per_shot=True) consumes.

`VRGDGFaceFixLoadAnchorsMetaBatch` and `VRGDGFaceFixStoreAnchors` carry the 512 x 512 anchors to the image model and back: the Meta Batch
protocol and the decode seam `image_loader` are in _anchors.py, a call's chunk of decoded bytes becomes fp32 in one launch
(ops.anchor_frames); the store quantises and swaps to B,G,R in one launch (ops.anchor_store_bytes), downloads once and hands every
frame to the seam `png_writer(path, bgr_bytes)` -- cv2.imwrite in the reference; the default writes the same pixels through Pillow.
They are listed in ANCHOR_NODE_CLASS_MAPPINGS / ANCHOR_NODE_DISPLAY_NAME_MAPPINGS.

What is NOT here: detection and tracking (cv2 DNN, candidate choice, anchor selection and the anchor PNG dump) and
with them the Prepare / Collect node classes -- a shot-aware Prepare node calls shot_boundaries once before its detection loop and
face_crop_sequence once after it, INTEGRATION.md shows the lines; the landmark detector of the aligned composite (YuNet, the RANSAC similarity fit and the .onnx asset); and
the registration in the package's NODE_CLASS_MAPPINGS: INTEGRATION.md shows the lines.  The nodes are eager.

Refused with a ValueError, because the reference fails on them rather than defines them: a box that does not lie inside its frame (shape
mismatch in the reference's composite, a smaller crop than the box in its Prepare), an empty box in VRGDGFaceFixComposite and in the crop
sequence, and channel counts other than 3 or 4 in the composites.  The cut score refuses frames with a side below 64 px (cv2's INTER_AREA
takes another, bilinear-like route there: out of scope), batches that are not [frames, height, width, channels], empty batches and fewer
than 3 channels.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch

from . import _anchors, ops
from ._devices import compute_device, intermediate_device, stream_frames_with_masks

FACE_FIX_CONTEXT = "VRGDG_FACE_FIX_CONTEXT"


def _log(message):
    print(f"[VRGDG Face Fix] {message}", flush=True)


def face_crop_sequence(video_frames, entries, *, per_shot=False, anchors=None):
    """The crop / fill / prefix / stack / anchor-gather lines of VRGDGFaceFixPrepare.prepare (per_shot=False) and
    VRGDGFaceFixPrepareShotAware.prepare (per_shot=True: holes take the first crop of their entry's "shot_id").  `entries`: one dict per
    video frame, "box" = (left, top, right, bottom) or None.  Returns (crop_batch [ltx_offset + frames, 512, 512, 3], anchor_batch =
    crop_batch[ltx_offset:][anchors] or None, ltx_offset) -- the context fields "entries", "original_frames" and "ltx_frame_offset" of
    the reference go with it unchanged to the composite nodes.  Device frames are cropped where they are and the batch stays there; of CPU
    frames only the boxes are uploaded, the batch comes back on the intermediate device.  `video_frames` is never written."""
    if not isinstance(video_frames, torch.Tensor) or video_frames.ndim != 4 or video_frames.shape[0] < 1:
        raise ValueError("Face Fix Prepare requires a non-empty IMAGE batch from a video loader.")
    count, height, width = (int(v) for v in video_frames.shape[:3])
    plan = ops.crop_sequence_plan(entries, count, height, width, per_shot=per_shot)        # refuses before anything is uploaded
    if video_frames.is_cuda:
        crop_batch = ops.crop_frames(video_frames.to(torch.float32), plan)
    else:
        crop_batch = ops.crop_frames_host(video_frames, plan)
    anchor_batch = None
    if anchors is not None:
        anchor_batch = crop_batch[plan.ltx_offset:][torch.tensor([int(a) for a in anchors], device=crop_batch.device, dtype=torch.long)]
    return crop_batch, anchor_batch, plan.ltx_offset


_THUMB_VALUES = 64 * 64 * 3         # bytes of one thumbnail
_HIST_TOTAL = 64 * 64               # every histogram sums to the pixels of a thumbnail
_HIST_BINS = 32 * 32


def cut_scores_from_sums(sums) -> np.ndarray:
    """The host half of the cut score: `sums` = int [pairs, 4] rows (D, S11, S22, S12) of ops.cut_pair_sums -> float64 [pairs + 1] with
    score[0] = 0.0 and score[i] = what `_cut_score(frame i - 1, frame i)` returns:
      mean_delta = D / (255 * 12288)
      corr       = compareHist(.., HISTCMP_CORREL) of the two L2-normalised histograms.  The correlation does not change under the
                   normalisation, so it is (1024 S12 - 4096^2) / sqrt((1024 S11 - 4096^2) (1024 S22 - 4096^2)) from exact integers; cv2's
                   `|denom| > DBL_EPSILON` test (1.0 where it fails) is evaluated on the normalised values it sees
      score      = max(mean_delta, (1 - corr) / 2)"""
    rows = [[int(v) for v in row] for row in np.asarray(sums).reshape(-1, 4).tolist()]
    scores = np.zeros(len(rows) + 1, dtype=np.float64)
    square = _HIST_TOTAL * _HIST_TOTAL
    for i, (d, s11, s22, s12) in enumerate(rows):
        mean_delta = d / (255.0 * _THUMB_VALUES)
        var1, var2, cov = _HIST_BINS * s11 - square, _HIST_BINS * s22 - square, _HIST_BINS * s12 - square
        denom_normalised = (var1 / (_HIST_BINS * s11)) * (var2 / (_HIST_BINS * s22)) if s11 > 0 and s22 > 0 else 0.0
        corr = cov / math.sqrt(var1 * var2) if abs(denom_normalised) > sys.float_info.epsilon else 1.0
        scores[i + 1] = max(mean_delta, (1.0 - corr) * 0.5)
    return scores


def boundaries_from_scores(scores, cut_sensitivity):
    """The rule of VRGDGFaceFixPrepareShotAware.prepare (:457-459): hard_cut[i] = i > 0 and score[i] >= float(cut_sensitivity); shot_id
    starts at 0 and increments at every hard cut.  Returns (hard_cut: list[bool], shot_id: list[int])."""
    threshold = float(cut_sensitivity)
    hard_cut, shot_id, shot = [], [], 0
    for index, score in enumerate(scores):
        cut = index > 0 and float(score) >= threshold
        if cut:
            shot += 1
        hard_cut.append(bool(cut))
        shot_id.append(shot)
    return hard_cut, shot_id


def shot_cut_scores(video_frames) -> np.ndarray:
    """float64 [frames]: score[0] = 0.0, score[i] = the reference's `_cut_score` of frames i - 1 and i (each quantised as :456 does).
    Device frames are reduced where they are; CPU frames stream up in pieces.  `video_frames` is never written."""
    if not isinstance(video_frames, torch.Tensor) or video_frames.ndim != 4 or video_frames.shape[0] < 1:
        raise ValueError("Shot-aware Face Fix Prepare requires a non-empty video batch.")
    if video_frames.is_cuda:
        thumbs = ops.cut_thumbnails(video_frames.to(torch.float32))
    else:
        thumbs = ops.cut_thumbnails_host(video_frames)
    if thumbs.shape[0] < 2:
        return np.zeros(int(thumbs.shape[0]), dtype=np.float64)
    return cut_scores_from_sums(ops.cut_pair_sums(thumbs).cpu().numpy())


def shot_boundaries(video_frames, cut_sensitivity):
    """(hard_cut: list[bool], shot_id: list[int]) of the video, one per frame: what the loop of VRGDGFaceFixPrepareShotAware.prepare and
    VRGDGFaceFixPrepareVideoShotAware.prepare derives frame by frame, computed before it for the whole batch."""
    return boundaries_from_scores(shot_cut_scores(video_frames), cut_sensitivity)


# ------------------------------------------------------------------------------------------------
# the detector's input and the candidates made of its output (`_detect_with_rotation` / `_detect`, :95-185)
# ------------------------------------------------------------------------------------------------
ROTATION_ANGLES = {"Off (fastest)": [0], "Light: ±15°": [0, -15, 15], "Strong: ±15° and ±30°": [0, -15, 15, -30, 30]}
BUILDER_ROTATION_ANGLES = {"off": [0], "light": [0, -15, 15], "strong": [0, -15, 15, -30, 30]}


def _iou(a, b):
    ax, ay, aw, ah = a
    bx, by, bw, bh = b
    overlap = max(0.0, min(ax + aw, bx + bw) - max(ax, bx)) * max(0.0, min(ay + ah, by + bh) - max(ay, by))
    union = aw * ah + bw * bh - overlap
    return overlap / union if union > 0 else 0.0


def _suppress(found):
    """the reference's suppression pass: by falling score (stable), keep what overlaps nothing kept by more than IoU 0.35"""
    kept = []
    for item in sorted(found, key=lambda value: value[4], reverse=True):
        if not any(_iou(item[:4], other[:4]) > 0.35 for other in kept):
            kept.append(item)
    return kept


def scan_regions(width, height, builder=False):
    """The regions one (rotated) frame is scanned in: the whole frame and, from 600 x 400 up, four 60 % x 70 % corner tiles -- int(...) in
    the stand-alone nodes (:98-102), int(round(...)) in the Builder (`_initial_regions`)."""
    width, height = int(width), int(height)
    regions = [(0, 0, width, height)]
    if width >= 600 and height >= 400:
        if builder:
            tile_w, tile_h = int(round(width * 0.60)), int(round(height * 0.70))
        else:
            tile_w, tile_h = int(width * 0.60), int(height * 0.70)
        regions += [(0, 0, tile_w, tile_h), (width - tile_w, 0, width, tile_h), (0, height - tile_h, tile_w, height),
                    (width - tile_w, height - tile_h, width, height)]
    return regions


def rotation_matrices(width, height, angle):
    """(forward, inverse) 2 x 3 float64 of one angle: cv2.getRotationMatrix2D((width / 2.0, height / 2.0), angle, 1.0) and its
    cv2.invertAffineTransform -- the same doubles warpAffine forms when it inverts the matrix itself (csrc/vrg_detect_math.hpp)."""
    radians = float(angle) * math.pi / 180.0
    a, b = math.cos(radians), math.sin(radians)
    cx, cy = width / 2.0, height / 2.0
    m = [a, b, (1.0 - a) * cx - b * cy, -b, a, b * cx + (1.0 - a) * cy]
    forward = np.array(m, dtype=np.float64).reshape(2, 3)
    d = m[0] * m[4] - m[1] * m[3]
    d = 1.0 / d if d != 0.0 else 0.0
    a11, a22 = m[4] * d, m[0] * d
    m[0], m[1], m[3], m[4] = a11, m[1] * -d, m[3] * -d, a22
    b1, b2 = -m[0] * m[2] - m[1] * m[5], -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return forward, np.array(m, dtype=np.float64).reshape(2, 3)


class DetectionPlan:
    """What the detector scans in every frame of a width x height video: `angles`; per angle the `forward` and `inverse` matrices (None at
    angle 0) and the list of `regions` (left, top, right, bottom) of the rotated frame; `transforms` = the [T, 6] inverse doubles of the
    non-zero angles in order, `transform_index[a]` = its row or -1; `slots` = the largest region count of an angle, `scanned[a][r]` =
    whether slot r of angle a exists and has both sides >= 8 (the Builder skips smaller regions; the stand-alone nodes do not meet them).
    `descriptors(frame_indices)` -> ops.DETECT_DESC records in [frame, angle, slot] order of the scanned slots, and their positions."""

    def __init__(self, width, height, angles, regions, builder):
        self.width, self.height, self.angles, self.builder = int(width), int(height), [int(a) for a in angles], bool(builder)
        self.regions = [[tuple(int(v) for v in r) for r in per_angle] for per_angle in regions]
        self.forward, self.inverse, self.transform_index, rows = [], [], [], []
        for angle in self.angles:
            if angle == 0:
                self.forward.append(None)
                self.inverse.append(None)
                self.transform_index.append(-1)
                continue
            forward, inverse = rotation_matrices(self.width, self.height, angle)
            self.forward.append(forward)
            self.inverse.append(inverse)
            self.transform_index.append(len(rows))
            rows.append(inverse.reshape(6))
        self.transforms = np.array(rows, dtype=np.float64).reshape(-1, 6)
        self.slots = max((len(r) for r in self.regions), default=0)
        self.scanned = [[(r < len(per_angle) and per_angle[r][2] - per_angle[r][0] >= ops.DETECT_MIN_SIDE and
                          per_angle[r][3] - per_angle[r][1] >= ops.DETECT_MIN_SIDE) for r in range(self.slots)] for per_angle in self.regions]

    def descriptors(self, frame_indices):
        frame_indices = [int(f) for f in frame_indices]
        per_frame = [(a, r) for a in range(len(self.angles)) for r in range(self.slots) if self.scanned[a][r]]
        desc = np.zeros(len(frame_indices) * len(per_frame), dtype=ops.DETECT_DESC)
        where = np.zeros(desc.size, dtype=np.int64)
        k = 0
        for i, f in enumerate(frame_indices):
            for a, r in per_frame:
                left, top, right, bottom = self.regions[a][r]
                desc[k] = (f, self.transform_index[a], left, top, right, bottom)
                where[k] = (i * len(self.angles) + a) * self.slots + r
                k += 1
        return desc, where


def detection_plan(width, height, rotation_assist, regions=None, builder=False):
    """The scan of `_detect_with_rotation` for width x height frames.  Stand-alone nodes (:146-166): `rotation_assist` is the widget's value
    (an unknown one scans angle 0 only) and every angle scans scan_regions(width, height).  `builder=True` (VRGDG_FaceFix.py:116-139): the
    mode names are off / light / strong (None or an unknown one: light), angle 0 scans the caller's `regions` (None: the initial regions)
    and every other angle the initial regions.  A region must lie inside the frame; one with a side below 8 is not scanned."""
    width, height = int(width), int(height)
    if not (1 <= width <= ops.DETECT_MAX_SIDE and 1 <= height <= ops.DETECT_MAX_SIDE):
        raise ValueError(f"detection_plan: {width} x {height}: sides must lie in 1 .. {ops.DETECT_MAX_SIDE}")
    if builder:
        angles = BUILDER_ROTATION_ANGLES.get(str(rotation_assist or "light").lower(), [0, -15, 15])
    else:
        angles = ROTATION_ANGLES.get(str(rotation_assist), [0])
    initial = scan_regions(width, height, builder=builder)
    own = initial if regions is None else [tuple(int(v) for v in r) for r in regions]
    for left, top, right, bottom in own:
        if left < 0 or top < 0 or right > width or bottom > height:
            raise ValueError(f"detection_plan: region {(left, top, right, bottom)} does not lie inside the {width} x {height} frame")
    if not builder and min(width, height) < ops.DETECT_MIN_SIDE:
        raise ValueError(f"detection_plan: {width} x {height} frames have a side below {ops.DETECT_MIN_SIDE} px; refused")
    return DetectionPlan(width, height, angles, [own if (angle == 0 or not builder) else initial for angle in angles], builder)


def _plan_frames(video_frames, plan, frames):
    if not isinstance(video_frames, torch.Tensor) or video_frames.ndim != 4:
        raise ValueError("the detector input requires a [frames, height, width, channels] batch")
    if (int(video_frames.shape[1]), int(video_frames.shape[2])) != (plan.height, plan.width):
        raise ValueError(f"the plan was made for {plan.width} x {plan.height} frames, the batch is {int(video_frames.shape[2])} x {int(video_frames.shape[1])}")
    count = int(video_frames.shape[0])
    indices = list(range(count)) if frames is None else [int(f) for f in frames]
    for f in indices:
        if not 0 <= f < count:
            raise ValueError(f"frame {f} is outside the batch of {count}")
    return indices


def detector_blobs(video_frames, plan, frames=None):
    """The blobs the Caffe detector is fed for the frames `frames` (None: all) of the batch: fp32 ``[F, A, R, 3, 300, 300]`` (A angles of the
    plan, R = plan.slots; a slot that is not scanned is zeros) on the compute device, in one launch of csrc/vrg_detect.hip -- the frame is
    quantised, swapped to B,G,R, rotated, cut and resized where it is read; no rotated frame is written.  `video_frames`: fp32 R,G,B
    ``[n, H, W, C >= 3]`` as the nodes get it, or uint8 B,G,R ``[n, H, W, 3]`` as the Builder decodes it; GPU or CPU; never written."""
    indices = _plan_frames(video_frames, plan, frames)
    desc, where = plan.descriptors(indices)
    blobs = ops.detect_blobs(video_frames, desc, plan.transforms)
    shape = (len(indices), len(plan.angles), plan.slots, 3, ops.DETECT_BLOB, ops.DETECT_BLOB)
    if desc.size == shape[0] * shape[1] * shape[2]:
        return blobs.view(shape)
    out = torch.zeros(shape, dtype=torch.float32, device=blobs.device)
    if desc.size:
        out.view((-1,) + shape[3:]).index_copy_(0, torch.from_numpy(where).to(blobs.device), blobs)
    return out


def rotated_frames(video_frames, plan, frames=None):
    """The rotated B,G,R byte frames of the YuNet branch (`detector.detect(region)` reads regions of them): uint8 ``[F, A, H, W, 3]`` on the
    compute device; angle 0 is the quantised frame itself.  Frames as detector_blobs takes them."""
    indices = _plan_frames(video_frames, plan, frames)
    desc = np.array([(f, t) for f in indices for t in plan.transform_index], dtype=ops.DETECT_FRAME_DESC)
    out = ops.warp_linear_bytes(video_frames, desc, plan.transforms)
    return out.view(len(indices), len(plan.angles), plan.height, plan.width, 3)


def _decode_caffe(rows, region, confidence, minimum_pixels, builder):
    left, top, right, bottom = region
    rw, rh = right - left, bottom - top
    found = []
    for item in rows:
        score = float(item[2])
        if score < confidence:
            continue
        if builder:
            x1 = max(left, left + int(round(float(item[3]) * rw)))
            y1 = max(top, top + int(round(float(item[4]) * rh)))
            x2 = min(right, left + int(round(float(item[5]) * rw)))
            y2 = min(bottom, top + int(round(float(item[6]) * rh)))
            keep = x2 > x1 and y2 > y1
        else:
            x1 = max(left, left + int(float(item[3]) * rw))
            y1 = max(top, top + int(float(item[4]) * rh))
            x2 = min(right, left + int(float(item[5]) * rw))
            y2 = min(bottom, top + int(float(item[6]) * rh))
            keep = min(x2 - x1, y2 - y1) >= minimum_pixels
        if keep:
            found.append((float(x1), float(y1), float(x2 - x1), float(y2 - y1), score))
    return found


def _decode_yunet(faces, region, confidence, minimum_pixels, builder):
    left, top, right, bottom = region
    found = []
    for item in (() if faces is None else faces):
        score = float(item[-1])
        if score < confidence:
            continue
        x1 = max(left, left + int(round(float(item[0]))))
        y1 = max(top, top + int(round(float(item[1]))))
        x2 = min(right, x1 + int(round(float(item[2]))))
        y2 = min(bottom, y1 + int(round(float(item[3]))))
        keep = (x2 > x1 and y2 > y1) if builder else min(x2 - x1, y2 - y1) >= minimum_pixels
        if keep:
            found.append((float(x1), float(y1), float(x2 - x1), float(y2 - y1), score))
    return found


def candidates_from_outputs(plan, outputs, confidence, minimum_pixels=0, kind="caffe"):
    """The candidates of ONE frame from what the detector returned for its scanned regions, host arithmetic in double as the reference does
    it.  `outputs[a][r]`: for kind "caffe" the ``[K, 7]`` rows of ``forward()[0, 0]`` of angle a, slot r (a leading ``[1, 1]`` or ``[1]`` is
    dropped); for kind "yunet" the faces ``[k, 15]`` (or None) `detector.detect` returned for that region.  A slot that is not scanned is
    ignored.  Per angle: the box decode (stand-alone: int() truncation, kept when min(w, h) >= minimum_pixels; Builder: round(), kept when
    x2 > x and y2 > y) and the IoU-0.35 suppression of `_detect`; then for a rotated angle the four corners mapped through the inverse
    matrix, their bounding box clipped to the frame and the score lowered by |angle| * 0.0001; then the suppression over all angles.
    Returns [(x, y, w, h, score)] floats."""
    confidence = float(confidence)
    width, height = plan.width, plan.height
    found = []
    for a, angle in enumerate(plan.angles):
        per_angle = []
        for r in range(plan.slots):
            if not plan.scanned[a][r]:
                continue
            rows = outputs[a][r]
            if kind == "yunet":
                per_angle += _decode_yunet(rows, plan.regions[a][r], confidence, minimum_pixels, plan.builder)
            else:
                rows = np.asarray(rows)
                per_angle += _decode_caffe(rows.reshape(-1, rows.shape[-1]) if rows.size else (), plan.regions[a][r], confidence, minimum_pixels, plan.builder)
        inverse = plan.inverse[a]
        for x, y, w, h, score in _suppress(per_angle):
            if inverse is None:
                found.append((x, y, w, h, score))
                continue
            corners = np.array([[x, y, 1.0], [x + w, y, 1.0], [x, y + h, 1.0], [x + w, y + h, 1.0]], dtype=np.float64)
            mapped = corners @ inverse.T
            x1, y1 = max(0.0, mapped[:, 0].min()), max(0.0, mapped[:, 1].min())
            x2, y2 = min(float(width), mapped[:, 0].max()), min(float(height), mapped[:, 1].max())
            if x2 > x1 and y2 > y1:
                found.append((x1, y1, x2 - x1, y2 - y1, score - abs(angle) * 0.0001))
    return _suppress(found)


def detect_with_rotation(forward=None, video_frames=None, confidence=0.70, minimum_pixels=20, rotation_assist="Light: ±15°", regions=None,
                         builder=False, frames=None, chunk_frames=16):
    """`_detect_with_rotation` for the frames `frames` (None: all) of a batch: one candidate list [(x, y, w, h, score)] per frame.
    `forward(blobs) -> [n, 1, K, 7]` is the network: it gets fp32 ``[n, 3, 300, 300]`` blobs on the compute device and returns, per blob, the
    rows of cv2.dnn's ``net.forward()[0, 0]`` (a tensor, an array, or a list of n arrays whose row counts K may differ).  It is None by default -- no detector, the state of a machine
    without cv2's DNN module or the model files: every frame then has no candidates and nothing is computed.  INTEGRATION.md binds the
    reference's Caffe net to it.  The blobs of `chunk_frames` frames are made in one launch and handed to `forward` together."""
    if not isinstance(video_frames, torch.Tensor) or video_frames.ndim != 4:
        raise ValueError("detect_with_rotation requires a [frames, height, width, channels] batch")
    plan = detection_plan(int(video_frames.shape[2]), int(video_frames.shape[1]), rotation_assist, regions=regions, builder=builder)
    indices = _plan_frames(video_frames, plan, frames)
    if forward is None:
        return [[] for _ in indices]
    results, step = [], max(1, int(chunk_frames))
    for s in range(0, len(indices), step):
        part = indices[s:s + step]
        blobs = detector_blobs(video_frames, plan, part)
        flat = blobs.view((-1,) + tuple(blobs.shape[3:]))
        outputs = forward(flat)
        if isinstance(outputs, torch.Tensor):
            outputs = outputs.detach().cpu().numpy()
        per_blob = list(outputs)                                                   # one [1, K, 7] or [K, 7] per blob; K may differ from blob to blob
        if len(per_blob) != int(flat.shape[0]):
            raise ValueError(f"forward returned {len(per_blob)} outputs for {int(flat.shape[0])} blobs")
        angles, slots = len(plan.angles), plan.slots
        for i in range(len(part)):
            results.append(candidates_from_outputs(plan, [[per_blob[(i * angles + a) * slots + r] for r in range(slots)] for a in range(angles)],
                                                   confidence, minimum_pixels))
    return results


class _Plan:
    """What a composite call works on, read from the node's inputs once: the context's original frames and entries, the index of the
    first work frame that belongs to source frame 0, how many source frames have a work frame at all, and the frame-count difference
    the reference reports (source frames minus the work frames left after the offset; more than 7 either way is refused)."""

    def __init__(self, work, context):
        self.work, self.originals, self.entries = work, context["original_frames"], context["entries"]
        self.offset = int(context.get("ltx_frame_offset") or 0)
        self.work_frames, self.sources = int(work.shape[0]), len(self.entries)
        left_after_offset = self.work_frames - self.offset if self.work_frames > self.offset else 0
        self.delta = self.sources - left_after_offset
        self.usable = self.sources if self.sources < left_after_offset else left_after_offset

    def refuse_if_counts_differ(self):
        if not -7 <= self.delta <= 7:
            raise ValueError(f"LTX returned {self.work_frames} frames for {self.sources} source frames.")

    def repaired(self, counts) -> int:
        return sum(1 for entry in self.entries[:self.usable] if counts(entry))


def _composite(plan, rule, color_match):
    """(frames, masks) wherever the originals live."""
    work, originals, entries, offset = plan.work, plan.originals, plan.entries, plan.offset
    n_work, n_orig = plan.work_frames, int(originals.shape[0])
    ops.composite_channels(rule, originals.shape[3], work.shape[3])
    rows = ops.face_fix_entries(entries, n_work, offset, n_orig)
    ops.composite_table(rows, rule, color_match, originals.shape[1], originals.shape[2])        # refuses before anything is uploaded
    if originals.is_cuda or n_orig == 0 or intermediate_device().type != "cpu":
        dev = originals.device if originals.is_cuda else compute_device()
        with torch.cuda.device(dev):
            out, masks = ops.composite_frames(originals.to(dev, torch.float32), work.to(dev, torch.float32), rows, rule, color_match)
        if not originals.is_cuda:
            out, masks = out.to(intermediate_device()), masks.to(intermediate_device())
        return out, masks
    # host-fed: the originals (24 B per pixel up and down) stream through the staging pipeline, the work frames are uploaded once
    dev = compute_device()
    with torch.cuda.device(dev):
        work_dev = work.to(dev, torch.float32)
    if originals.dtype != torch.float32:
        originals = originals.float()

    def piece(gpu_originals, first_frame):
        last = first_frame + int(gpu_originals.shape[0])
        return ops.composite_frames(gpu_originals, work_dev, ops.face_fix_entries(entries, n_work, offset, n_orig, first_frame, last), rule,
                                    color_match)

    return stream_frames_with_masks(originals, piece)


class VRGDGFaceFixComposite:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {
            "ltx_face_frames": ("IMAGE", {"tooltip": "Connect the final IMAGE batch from the LTX VAE Decode node. Do not connect source crops or anchor images here."}),
            "face_fix_context": (FACE_FIX_CONTEXT, {"tooltip": "Connect Collect LTX Inputs: face_fix_context. It supplies original full-resolution frames, crop rectangles, and no-face safety decisions."}),
            "feather_pixels": ("INT", {"default": 18, "min": 0, "max": 256, "tooltip": "Softens the boundary where each repaired face crop meets the original frame. Higher values create a wider, smoother transition; too high may weaken facial detail. Lower values are sharper but can reveal a visible edge. Recommended starting value: 18."}),
            "color_match": ("FLOAT", {"default": 0.65, "min": 0.0, "max": 1.0, "step": 0.05, "tooltip": "Shifts the repaired crop's average color toward the original face region before blending. 0 disables matching; 1 applies the full measured correction. Increase for lighting/color seams, decrease if skin tone becomes dull or unstable. Recommended: 0.65."}),
        }}

    RETURN_TYPES = ("IMAGE", "MASK", "INT")
    RETURN_NAMES = ("repaired_video_frames", "applied_face_mask", "repaired_frame_count")
    RETURN_TOOLTIPS = (
        "Original full-resolution video frame batch with safe repaired faces composited in. Connect to VHS Video Combine images.",
        "Per-frame grayscale mask showing exactly where and how strongly Face Fix was applied. Optional diagnostic output.",
        "Number of frames that received a nonzero repaired-face composite. Optional diagnostic output.",
    )
    FUNCTION = "composite"
    CATEGORY = "VRGameDevGirl/Face Fix"
    DESCRIPTION = "Feathers LTX face frames back into the original video frames; no-face and short LTX tail frames remain unchanged."

    def composite(self, ltx_face_frames, face_fix_context, feather_pixels, color_match):
        plan = _Plan(ltx_face_frames, face_fix_context)
        _log(
            f"Composite started. Job={face_fix_context.get('job_id', 'unknown')}; "
            f"source_frames={plan.sources}, LTX_frames={plan.work_frames}, delta={plan.delta}, "
            f"feather={feather_pixels}, color_match={color_match:.2f}."
        )
        plan.refuse_if_counts_differ()
        # a frame is repaired when its entry has a box and a positive strength (a missing strength is 0)
        repaired = plan.repaired(lambda entry: bool(entry.get("box")) and float(entry.get("strength", 0.0)) > 0)
        output, masks = _composite(plan, ops.CompositeRule("radial", feather=feather_pixels), color_match)
        _log(
            f"Composite finished: repaired={repaired}, unchanged={plan.sources - repaired}, "
            f"preserved_LTX_tail={plan.delta if plan.delta > 0 else 0}."
        )
        return output, masks, repaired


class VRGDGFaceFixCompositeOpaque:
    """Composite the generated crop at full opacity inside a feathered edge."""

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {
            "ltx_face_frames": ("IMAGE", {"tooltip": "The complete decoded LTX face-video batch."}),
            "face_fix_context": (FACE_FIX_CONTEXT, {"tooltip": "Tracked crop boxes and original frames from Face Fix Prepare."}),
            "feather_pixels": ("INT", {"default": 6, "min": 0, "max": 128, "tooltip": "Feather only the outer crop boundary. The face interior remains fully opaque."}),
        }}

    RETURN_TYPES = ("IMAGE", "MASK", "INT")
    RETURN_NAMES = ("repaired_video_frames", "applied_face_mask", "repaired_frame_count")
    FUNCTION = "composite"
    CATEGORY = "VRGameDevGirl/Face Fix"
    DESCRIPTION = "Fully replaces every tracked face crop; only the outside boundary is feathered."

    def composite(self, ltx_face_frames, face_fix_context, feather_pixels):
        plan = _Plan(ltx_face_frames, face_fix_context)
        plan.refuse_if_counts_differ()
        feather = int(feather_pixels) if int(feather_pixels) > 0 else 0

        def has_area(entry):                                # the opaque node ignores the strength; an empty box is skipped
            box = entry.get("box")
            if not box:
                return False
            left, top, right, bottom = (int(v) for v in box)
            return right > left and bottom > top

        repaired = plan.repaired(has_area)
        output, masks = _composite(plan, ops.CompositeRule("opaque", feather=feather), 0.0)
        _log(f"Opaque composite finished: repaired={repaired}, unchanged={plan.sources - repaired}, feather={feather}.")
        return output, masks, repaired


def _has_area(entry):
    box = entry.get("box")
    if not box:
        return False
    left, top, right, bottom = (int(v) for v in box)
    return right > left and bottom > top


def aligned_transforms(entries, usable, transform_smoothing, estimate):
    """The transform bookkeeping of VRGDGFaceFixCompositeLandmarkAligned.composite (:1011-1048) for source frames 0 .. usable - 1, in
    order: `estimate(index) -> 2 x 3 | None` is asked once for every frame whose box has area; an estimate becomes float32 and is smoothed
    into the previous one (previous * s + estimate * (1 - s), the two Python scalars entering as float32); a miss reuses the previous
    transform; `previous` is forgotten at an entry with "hard_cut" and when the "shot_id" changes (frames without a box do not take
    part).  Returns (one float32 2 x 3 or None per frame, the number of frames that have one = the log's `aligned`)."""
    smoothing = max(0.0, min(0.95, float(transform_smoothing)))
    keep, take = np.float32(smoothing), np.float32(1.0 - smoothing)
    transforms, aligned = [None] * int(usable), 0
    previous, previous_shot = None, None
    for index in range(int(usable)):
        entry = entries[index]
        if not _has_area(entry):
            continue
        shot_id = entry.get("shot_id", 0)
        if entry.get("hard_cut") or (previous_shot is not None and shot_id != previous_shot):
            previous = None
        previous_shot = shot_id
        transform = estimate(index)
        if transform is not None:
            transform = np.asarray(transform).astype(np.float32).reshape(2, 3)
            if previous is not None:
                transform = (previous * keep + transform * take).astype(np.float32)
            previous = transform
        elif previous is not None:
            transform = previous
        if transform is not None:
            transforms[index] = transform
            aligned += 1
    return transforms, aligned


def _quantise_host(values: torch.Tensor) -> np.ndarray:
    """uint8(clip(rint(v * 255), 0, 255)) in float32 on the host; NaN gives 0 (what ops.face_bytes gives on the device)"""
    v = values.detach().to(torch.float32).numpy()
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(v * np.float32(255.0)), 0, 255)
    return np.where(np.isnan(r), np.float32(0), r).astype(np.uint8)


LANDMARK_INPUT = ops.THUMB_SIDE                        # YuNet's input is fixed at 320 x 320


def landmark_points(faces, width, height):
    """The five landmarks of the best face among the detector's `[n, 15]` rows (box, right eye, left eye, nose, right and left mouth
    corner, score), scaled from the 320 x 320 thumbnail back to the width x height box: float32 `[5, 2]`, or None without a face
    (`_landmarks`, :971-979).  The row with the largest score wins, the first one on ties; each axis is multiplied by the quotient
    side / 320 formed in double and rounded to float32 once, as NumPy does when a Python float meets a float32 array."""
    if faces is None or len(faces) == 0:
        return None
    best = 0
    for i in range(1, len(faces)):
        if float(faces[i][-1]) > float(faces[best][-1]):
            best = i
    points = np.array(np.asarray(faces[best])[4:14], dtype=np.float32).reshape(5, 2)
    scale = np.array([np.float32(float(width) / float(LANDMARK_INPUT)), np.float32(float(height) / float(LANDMARK_INPUT))], dtype=np.float32)
    return points * scale[None, :]


def cv2_landmark_seams():
    """(landmark_detector, transform_fit) on cv2's FaceDetectorYN with the reference's arguments ("", (320, 320), 0.1, 0.3, 5000) and
    cv2.estimateAffinePartial2D(..., RANSAC, 3.0), or None when cv2 cannot be imported, has no FaceDetectorYN, the model file
    assets/face_detection_yunet_2023mar.onnx is not in the package (it is not shipped) or the detector cannot be created -- the
    reference's own `_detector` guard, after which every frame takes the fallback."""
    try:
        import cv2
    except Exception:
        return None
    model = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets", "face_detection_yunet_2023mar.onnx")
    create = getattr(cv2, "FaceDetectorYN_create", None)
    if create is None:
        create = getattr(getattr(cv2, "FaceDetectorYN", None), "create", None)
    if not callable(create) or not os.path.isfile(model):
        return None
    try:
        detector = create(model, "", (LANDMARK_INPUT, LANDMARK_INPUT), 0.1, 0.3, 5000)
    except Exception:
        return None

    def landmark_detector(bgr_320):
        detector.setInputSize((LANDMARK_INPUT, LANDMARK_INPUT))
        try:
            result = detector.detect(np.ascontiguousarray(bgr_320))
        except cv2.error:
            return None
        return result[1] if isinstance(result, tuple) and len(result) > 1 else result

    def transform_fit(generated_points, source_points):
        return cv2.estimateAffinePartial2D(generated_points, source_points, method=cv2.RANSAC, ransacReprojThreshold=3.0)[0]

    return landmark_detector, transform_fit


def _packed_source_bytes(faces, originals, entries, usable):
    """Host-fed originals: every box quantised on the CPU (_quantise_host) and packed at faces.offsets, as face_bytes packs the device's"""
    packed = np.zeros(int(faces.generated.numel()), dtype=np.uint8)
    for index in range(min(int(usable), len(faces.offsets))):
        if faces.offsets[index] < 0 or min(faces.sizes[index]) < 2:
            continue
        left, top, right, bottom = (int(v) for v in entries[index]["box"])
        box = _quantise_host(originals[index, top:bottom, left:right, :3].cpu())
        packed[faces.offsets[index]:faces.offsets[index] + box.size] = box.reshape(-1)
    return packed


def _aligned_composite(plan, feather, transform_smoothing, estimator, seams=None):
    """(frames, masks, aligned) wherever the originals live.  `seams` = (landmark_detector, transform_fit): the thumbnail route."""
    work, originals, entries, offset = plan.work, plan.originals, plan.entries, plan.offset
    n_work, n_orig = plan.work_frames, int(originals.shape[0])
    rule = ops.CompositeRule("opaque", feather=feather)
    ops.composite_channels(rule, originals.shape[3], work.shape[3])
    rows = ops.face_fix_entries(entries, n_work, offset, n_orig)
    ops.composite_table(rows, rule, 0.0, originals.shape[1], originals.shape[2])                # refuses before anything is uploaded
    height, width = int(originals.shape[1]), int(originals.shape[2])
    host_fed = not (originals.is_cuda or n_orig == 0 or intermediate_device().type != "cpu")
    dev = originals.device if originals.is_cuda else compute_device()
    with torch.cuda.device(dev):
        work_dev = work.to(dev, torch.float32)
        originals_dev = None if host_fed or not originals.is_cuda else originals.to(torch.float32)
        # phase 1: the faces as bytes, made on the GPU and downloaded once; the source bytes too when the originals are there
        faces = ops.face_bytes(work_dev, rows, height, width, originals=originals_dev)
        if seams is None:
            generated_host = faces.generated.cpu().numpy()
            source_host = faces.source.cpu().numpy() if faces.source is not None else None
        else:
            # the 320 x 320 B,G,R thumbnails of both faces, made on the GPU; nothing else is downloaded
            packed = None if faces.source is not None else torch.from_numpy(_packed_source_bytes(faces, originals, entries, plan.usable)).to(dev)
            thumbs, thumb_row = ops.face_thumbs(faces, ("source", "generated"), source=packed)
            thumbs_host = thumbs.cpu().numpy()

    def estimate_from_faces(index):
        left, top, right, bottom = (int(v) for v in entries[index]["box"])
        if source_host is not None:
            source = faces.image(source_host, index)
        else:
            source = _quantise_host(originals[index, top:bottom, left:right, :3].cpu())
        return estimator(source, faces.image(generated_host, index))

    def estimate_from_thumbs(index):
        row = thumb_row[index]
        if row < 0:                                         # a side below 2: `_landmarks` gives no points and resizes nothing
            return None
        detect, fit = seams
        box_w, box_h = faces.sizes[index]
        found_source, found_generated = detect(thumbs_host[row, 0]), detect(thumbs_host[row, 1])          # both, always, in this order
        source_points, generated_points = landmark_points(found_source, box_w, box_h), landmark_points(found_generated, box_w, box_h)
        if source_points is None or generated_points is None:
            return None
        return fit(generated_points, source_points)

    estimate = estimate_from_faces if seams is None else estimate_from_thumbs

    # phase 2: the estimator and the smoothing / reset rules, frame by frame on the host
    transforms, aligned = aligned_transforms(entries, plan.usable, transform_smoothing, estimate)
    transforms += [None] * (n_orig - len(transforms))
    ops.warp_records(transforms, [row["box"] for row in rows])                                  # refuses before the pass
    # phase 3: one composite pass
    if not host_fed:
        with torch.cuda.device(dev):
            frames_dev = originals_dev if originals_dev is not None else originals.to(dev, torch.float32)
            out, masks = ops.aligned_composite_frames(frames_dev, work_dev, rows, feather, transforms, generated=faces)
        if not originals.is_cuda:
            out, masks = out.to(intermediate_device()), masks.to(intermediate_device())
        return out, masks, aligned
    if originals.dtype != torch.float32:
        originals = originals.float()

    def piece(gpu_originals, first_frame):
        last = first_frame + int(gpu_originals.shape[0])
        return ops.aligned_composite_frames(gpu_originals, work_dev, ops.face_fix_entries(entries, n_work, offset, n_orig, first_frame, last),
                                            feather, transforms[first_frame:last], generated=faces.piece(first_frame, last))

    out, masks = stream_frames_with_masks(originals, piece)
    return out, masks, aligned


class VRGDGFaceFixCompositeLandmarkAligned:
    """Align the generated face to the source crop before opaque compositing."""

    #: `estimator(source_u8, generated_u8) -> 2 x 3 | None`: the transform that carries the generated face's landmarks onto the source's
    #: ([h, w, 3] uint8 RGB each), or None when either face gives no landmarks.  None = no detector: every frame takes the fallback.
    estimator = None
    #: The finer seam, used when `estimator` is None and both are set: the estimator's resize runs on the GPU and only 320 x 320 B,G,R
    #: thumbnails are downloaded.  `landmark_detector(bgr_320) -> faces | None`: the `[n, 15]` YuNet rows of one [320, 320, 3] uint8 image
    #: (None or empty: no face); `transform_fit(generated_points, source_points) -> 2 x 3 | None` on float32 [5, 2] points in box
    #: coordinates.  cv2_landmark_seams() builds both on cv2.  Assign functions with staticmethod(...), like `estimator`.
    landmark_detector = None
    transform_fit = None

    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {
            "ltx_face_frames": ("IMAGE", {"tooltip": "Decoded LTX face-video frames."}),
            "face_fix_context": (FACE_FIX_CONTEXT, {"tooltip": "Tracked source crop boxes and original frames."}),
            "feather_pixels": ("INT", {"default": 6, "min": 0, "max": 128, "tooltip": "Feather only the outer crop boundary."}),
            "transform_smoothing": ("FLOAT", {"default": 0.75, "min": 0.0, "max": 0.95, "step": 0.05, "tooltip": "Smooths landmark scale/position changes across frames. Resets automatically at hard cuts."}),
        }}

    RETURN_TYPES = ("IMAGE", "MASK", "INT")
    RETURN_NAMES = ("repaired_video_frames", "applied_face_mask", "repaired_frame_count")
    FUNCTION = "composite"
    CATEGORY = "VRGameDevGirl/Face Fix"
    DESCRIPTION = "Aligns LTX eyes/nose/mouth to the source crop, then fully replaces the tracked face."

    def composite(self, ltx_face_frames, face_fix_context, feather_pixels, transform_smoothing):
        plan = _Plan(ltx_face_frames, face_fix_context)
        plan.refuse_if_counts_differ()
        smoothing = max(0.0, min(0.95, float(transform_smoothing)))
        feather = int(feather_pixels) if int(feather_pixels) > 0 else 0
        repaired = plan.repaired(_has_area)
        estimator = self.estimator
        seams = None
        if estimator is None and self.landmark_detector is not None and self.transform_fit is not None:
            seams = (self.landmark_detector, self.transform_fit)
        if (estimator is None and seams is None) or repaired == 0:
            output, masks = _composite(plan, ops.CompositeRule("opaque", feather=feather), 0.0)
            aligned = 0
        else:
            output, masks, aligned = _aligned_composite(plan, feather, smoothing, estimator, seams)
        _log(f"Landmark composite finished: repaired={repaired}, aligned={aligned}, fallback={repaired - aligned}, feather={feather_pixels}, "
             f"smoothing={smoothing:.2f}.")
        return output, masks, repaired


NODE_CLASS_MAPPINGS = {
    "VRGDGFaceFixComposite": VRGDGFaceFixComposite,
    "VRGDGFaceFixCompositeOpaque": VRGDGFaceFixCompositeOpaque,
}


NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDGFaceFixComposite": "Face Fix - Composite Repaired Video",
    "VRGDGFaceFixCompositeOpaque": "Face Fix - Composite Opaque Full Face",
}


LANDMARK_NODE_CLASS_MAPPINGS = {
    "VRGDGFaceFixCompositeLandmarkAligned": VRGDGFaceFixCompositeLandmarkAligned,
}


LANDMARK_NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDGFaceFixCompositeLandmarkAligned": "Face Fix - Composite Landmark Aligned",
}


# ------------------------------------------------------------------------------------------------
# the anchor round trip: Load Anchors (Meta Batch) -> the image model -> Store Enhanced Anchors
# ------------------------------------------------------------------------------------------------
image_loader = _anchors.image_loader      # the decode seam of the Load node: path -> [h, w, 3] uint8 R,G,B

_NO_ANCHOR_FOLDER = "Prepared Face Fix anchor folder was not found: {}"
_NO_ANCHOR_FILES = "No anchor images were found in {}"
_NO_ANCHORS_LEFT = "The Face Fix Meta Batch has no anchor images left to load."


def png_writer(path, bgr_bytes):
    """The encode seam of the Store node: ``[h, w, 3]`` uint8 in B,G,R, what ``cv2.imwrite(path, ...)`` takes.  The default needs no cv2:
    it swaps back to R,G,B and writes the same pixels with Pillow.  A caller may bind ``cv2.imwrite`` instead."""
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(bgr_bytes[..., ::-1]), "RGB").save(path)


def _progress(index, total, label, checkpoints=10):
    done = index + 1
    if total > 0 and (done in (1, total) or done % max(total // checkpoints, 1) == 0):
        _log(f"{label}: {done}/{total}")


class VRGDGFaceFixLoadAnchorsMetaBatch:
    @classmethod
    def INPUT_TYPES(cls):
        return {
            "required": {
                "face_fix_context": (FACE_FIX_CONTEXT, {"tooltip": "Connect Face Fix - Prepare Video and Anchors: face_fix_context. It contains the automatically generated anchor-source folder."}),
                "meta_batch": ("VHS_BatchManager", {"tooltip": "Connect VHS Meta Batch Manager. Set frames_per_batch from Prepare's anchor_count so all anchors follow the same managed loading behavior used by the tested Z-Image workflow."}),
            },
            "hidden": {"unique_id": "UNIQUE_ID"},
        }

    RETURN_TYPES = ("IMAGE", "MASK", "INT", FACE_FIX_CONTEXT)
    RETURN_NAMES = ("anchor_images", "mask", "batch_frame_count", "face_fix_context")
    RETURN_TOOLTIPS = (
        "The current Meta Batch of 512×512 source anchors. Connect this to the Z-Image pixels/VAE Encode input.",
        "Blank compatibility mask supplied for workflows that require a MASK output.",
        "Number of anchors loaded in this Meta Batch execution.",
        "The unchanged Face Fix context. Connect this to Store Enhanced Anchors to preserve execution order.",
    )
    FUNCTION = "load"
    CATEGORY = "VRGameDevGirl/Face Fix"
    DESCRIPTION = "Loads prepared Face Fix anchors through VHS Meta Batch without manually selecting a folder."

    def load(self, face_fix_context, meta_batch, unique_id):
        directory = str(face_fix_context.get("anchor_sources_folder") or "")
        _log(f"Meta Batch anchor loader started. Job={face_fix_context.get('job_id', 'unknown')}; "
             f"frames_per_batch={getattr(meta_batch, 'frames_per_batch', '?')}; folder={directory}")
        if not os.path.isdir(directory):
            raise FileNotFoundError(_NO_ANCHOR_FOLDER.format(directory))
        images, masks, count = _anchors.load_chunk(directory, meta_batch, unique_id, lambda path: image_loader(path), _NO_ANCHOR_FILES,
                                                   _NO_ANCHORS_LEFT)
        _log(f"Meta Batch anchor loader returned {count} image(s) at {int(images.shape[2])}x{int(images.shape[1])}. "
             f"closed={getattr(meta_batch, 'has_closed_inputs', False)}")
        return images, masks, count, face_fix_context


class VRGDGFaceFixStoreAnchors:
    @classmethod
    def INPUT_TYPES(cls):
        return {"required": {
            "enhanced_anchors": ("IMAGE", {"tooltip": "Connect the decoded IMAGE output from Z-Image. The number and order must exactly match the anchors loaded by the Face Fix Meta Batch node."}),
            "face_fix_context": (FACE_FIX_CONTEXT, {"tooltip": "Connect Face Fix - Load Anchors (Meta Batch): face_fix_context. This links the enhanced results to the correct Face Fix job and anchor ordering."}),
        }}

    RETURN_TYPES = ("STRING", "STRING", "INT", FACE_FIX_CONTEXT)
    RETURN_NAMES = ("enhanced_anchor_folder", "anchor_indices", "anchor_count", "face_fix_context")
    RETURN_TOOLTIPS = (
        "Automatically managed folder containing the numbered Z-Image enhanced anchors for LTX.",
        "Comma-separated LTX conditioning positions corresponding to the saved anchors.",
        "Number of enhanced anchors validated and saved.",
        "Updated job context containing the enhanced-anchor folder. Connect this to Collect LTX Inputs: enhanced_anchor_context.",
    )
    FUNCTION = "store"
    CATEGORY = "VRGameDevGirl/Face Fix"
    OUTPUT_NODE = True
    DESCRIPTION = "Saves the enhanced anchor batch in deterministic order for LTX conditioning."

    def store(self, enhanced_anchors, face_fix_context):
        import folder_paths
        context = dict(face_fix_context)
        indices = list(context.get("anchor_indices") or [])
        received = int(enhanced_anchors.shape[0])
        _log(f"Store Enhanced Anchors started. Job={context.get('job_id', 'unknown')}; received={received}, expected={len(indices)}.")
        if received != len(indices):
            raise ValueError(f"Z-Image returned {received} anchors; expected {len(indices)}.")
        folder = os.path.join(folder_paths.get_output_directory(), "face_fix_standalone", context["job_id"], "enhanced_anchors_512")
        os.makedirs(folder, exist_ok=True)
        for entry in list(os.scandir(folder)):
            if entry.name.lower().endswith(".png"):
                os.remove(entry.path)
        frames = _anchors.stored_bytes(enhanced_anchors, bgr=True) if received else ()
        for order, frame in enumerate(frames):
            png_writer(os.path.join(folder, "anchor_%04d.png" % order), frame)
            _progress(order, len(frames), "Saving enhanced anchors")
        context["enhanced_anchor_folder"] = folder
        _log(f"Store Enhanced Anchors finished: {len(indices)} image(s) saved to {folder}")
        return folder, ",".join(str(value) for value in indices), len(indices), context


ANCHOR_NODE_CLASS_MAPPINGS = {
    "VRGDGFaceFixLoadAnchorsMetaBatch": VRGDGFaceFixLoadAnchorsMetaBatch,
    "VRGDGFaceFixStoreAnchors": VRGDGFaceFixStoreAnchors,
}


ANCHOR_NODE_DISPLAY_NAME_MAPPINGS = {
    "VRGDGFaceFixLoadAnchorsMetaBatch": "Face Fix - Load Anchors (Meta Batch)",
    "VRGDGFaceFixStoreAnchors": "Face Fix - Store Enhanced Anchors",
}
