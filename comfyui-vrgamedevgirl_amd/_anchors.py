"""What the Load Anchors (Meta Batch) and Store Enhanced Anchors nodes of the Video Enhance and Face Fix pipelines share: the VHS Meta Batch
protocol over a folder of anchor files, the decode seam, and the download of the file bytes.

Meta Batch protocol (VideoHelperSuite's batch manager, as the reference's nodes use it).  The first call of a node creates a generator over the
folder's image files in sorted order and stores ``(generator, width, height)`` in ``meta_batch.inputs[str(unique_id)]``; ``width, height``
is the size of the first file and ``meta_batch.total_frames`` becomes ``min(total_frames, file_count)``.  Every call takes the next
``meta_batch.frames_per_batch`` files.  When the generator ends -- the call after the last file, or a close from outside -- the entry is
popped and ``meta_batch.has_closed_inputs`` is set; a call that gets no file raises FileNotFoundError.

Here the generator yields DECODED BYTES, ``[h, w, 3]`` uint8 R,G,B of any size: one call's chunk goes to the GPU as bytes (3 B/px) and
through ``ops.anchor_frames`` in one launch, which stretches every picture to ``(width, height)`` as ``Image.resize(.., LANCZOS)`` does and
yields ``byte / 255`` in fp32.  The result stays on the compute device.
"""
from __future__ import annotations

import itertools
import os

import numpy as np
import torch

from . import ops
from ._devices import resident

IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".webp", ".bmp")


def image_loader(path) -> np.ndarray:
    """The host decode of one anchor file: ``[h, w, 3]`` uint8 R,G,B after the EXIF orientation.  A seam: the node modules look it up as
    their own ``image_loader`` attribute, which a caller may replace."""
    from PIL import Image, ImageOps
    with Image.open(path) as image:
        return np.array(ImageOps.exif_transpose(image).convert("RGB"))


def anchor_files(directory) -> list:
    """the image files of ``directory``, sorted by path"""
    return sorted(os.path.join(directory, name) for name in os.listdir(directory) if os.path.splitext(name)[1].lower() in IMAGE_SUFFIXES)


def _decoded(files, loader, meta_batch, key):
    try:
        for path in files:
            yield loader(path)
    finally:
        if meta_batch is not None and key in meta_batch.inputs:
            meta_batch.inputs.pop(key, None)
            meta_batch.has_closed_inputs = True


def load_chunk(directory, meta_batch, unique_id, loader, no_files, none_left):
    """One call of a Load Anchors node: ``(images, masks, count)``.  ``no_files`` (formatted with the folder) and ``none_left`` are the
    node's FileNotFoundError texts."""
    key = str(unique_id)
    if key not in meta_batch.inputs:
        files = anchor_files(directory)
        if not files:
            raise FileNotFoundError(no_files.format(directory))
        height, width = (int(v) for v in loader(files[0]).shape[:2])
        generator = _decoded(files, loader, meta_batch, key)
        meta_batch.inputs[key] = (generator, width, height)
        meta_batch.total_frames = min(meta_batch.total_frames, len(files))
    else:
        generator, width, height = meta_batch.inputs[key]
    chunk = list(itertools.islice(generator, int(meta_batch.frames_per_batch)))
    if not chunk:
        raise FileNotFoundError(none_left)
    images = ops.anchor_frames(chunk, size=(width, height))
    masks = torch.zeros((len(chunk), 64, 64), dtype=torch.float32)
    return images, masks, len(chunk)


def stored_bytes(images, bgr=False) -> np.ndarray:
    """``[N, H, W, 3]`` uint8 on the host, what the PNG files hold: ``ops.anchor_store_bytes`` where the batch lives (a CPU batch goes to
    the compute device first), then ONE download into page-locked memory (pageable where the host refuses to lock that much)."""
    if not isinstance(images, torch.Tensor) or images.ndim != 4:
        raise ValueError("enhanced anchors must be a [count, height, width, channels] IMAGE tensor")
    x = images.detach()
    if x.dtype != torch.float32:
        x = x.float()
    x = resident(x)
    with torch.cuda.device(x.device):
        data = ops.anchor_store_bytes(x, bgr=bgr)
        try:
            host = torch.empty(data.shape, dtype=torch.uint8, pin_memory=True)
        except RuntimeError:
            host = torch.empty(data.shape, dtype=torch.uint8)
        host.copy_(data, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    return host.numpy()
