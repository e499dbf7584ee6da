"""Ragged image batches: decoded images of different sizes through the input step on the GPU.

The reference hands each PIL image to CLIPProcessor one by one (dataset.py:152-164).  Here a batch of
uint8 [H, W, 3] images of any sizes is packed into one buffer (``ImageBatch``), optionally with a crop
box and a flip bit per image, and ``preprocess`` turns it into uint8 [B, S, S, 3] in three launches
(include/clipmi.h clipmi_resize_crop_u8), which the vision tower's fused im2col takes as it takes a
uniform uint8 batch.  Semantics: crop, then PIL ``Image.resize(BICUBIC)`` of the crop (bit-exact), then

  * ``mode="processor"``: short edge -> S, long edge -> int(S * long / short), centre S x S window
    (CLIPImageProcessor's resize + center_crop);
  * ``mode="square"``: the crop straight to S x S (what a random-resized-crop does);

then the flip, applied to the output's columns.  Downscales above 32x per axis are rejected.

Augmentation (no reference counterpart: the reference trains without any): ``random_resized_crop_boxes``
is the published RandomResizedCrop.get_params algorithm, ``TrainAugment`` draws boxes and flips from
its own seeded generator, ``CLIPAdapterTrainer(augment=...)`` applies it in ``train_step`` only."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import kernels as K

MODES = {"processor": 0, "square": 1}


class ImageItem(ctypes.Structure):
    """include/clipmi.h clipmi_image_item."""
    _fields_ = [("offset", ctypes.c_int64), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("x0", ctypes.c_int32),
                ("y0", ctypes.c_int32), ("cw", ctypes.c_int32), ("ch", ctypes.c_int32), ("flip", ctypes.c_int32)]


_lib.declare("clipmi_resize_crop_u8_ws", [ctypes.POINTER(ImageItem), ctypes.c_int, ctypes.c_int, ctypes.c_int],
             ctypes.c_int64)
_lib.declare("clipmi_resize_crop_u8", [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ImageItem),
                                       ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_int64])


class ImageBatch:
    """B channels-last RGB uint8 images of different sizes in one flat buffer.

    ``data``: uint8 [sum h*w*3] (host, pinned when CUDA is available, or device after ``.to``);
    ``sizes``: [(h, w)]; ``offsets``: byte offset of each image; ``boxes``: [(x0, y0, cw, ch)] (default:
    the whole image); ``flips``: [0 | 1] (default 0); ``mode``: "processor" | "square"."""

    def __init__(self, data, sizes, offsets, boxes=None, flips=None, mode="processor"):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
        self.data = data
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        self.offsets = [int(o) for o in offsets]
        n = len(self.sizes)
        self.boxes = [(0, 0, w, h) for h, w in self.sizes] if boxes is None else [tuple(int(v) for v in b) for b in boxes]
        self.flips = [0] * n if flips is None else [int(f) for f in flips]
        self.mode = mode
        if not (len(self.offsets) == len(self.boxes) == len(self.flips) == n):
            raise ValueError("ImageBatch: sizes, offsets, boxes and flips must have one entry per image")
        if any(len(b) != 4 for b in self.boxes):
            raise ValueError("ImageBatch: a box is (x0, y0, cw, ch)")

    @classmethod
    def pack(cls, images):
        """images: a list of uint8 [H, W, 3] tensors or ndarrays (H, W >= 1)."""
        ts = []
        for i, im in enumerate(images):
            t = torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
                raise ValueError(f"ImageBatch.pack: image {i} is not uint8")
            if t.dim() != 3 or t.shape[2] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
                raise ValueError(f"ImageBatch.pack: image {i} must be [H, W, 3], got {tuple(t.shape)}")
            ts.append(t)
        sizes = [(t.shape[0], t.shape[1]) for t in ts]
        offsets, total = [], 0
        for h, w in sizes:
            offsets.append(total)
            total += h * w * 3
        data = torch.empty(total, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        for t, o, (h, w) in zip(ts, offsets, sizes):
            data[o:o + h * w * 3].copy_(t.reshape(-1))
        return cls(data, sizes, offsets)

    def _like(self, **kw):
        a = dict(data=self.data, sizes=self.sizes, offsets=self.offsets, boxes=self.boxes, flips=self.flips,
                 mode=self.mode)
        a.update(kw)
        return ImageBatch(**a)

    def __len__(self):
        return len(self.sizes)

    @property
    def device(self):
        return self.data.device

    def to(self, device, non_blocking=False):
        return self._like(data=self.data.to(device, non_blocking=non_blocking))

    def with_boxes(self, boxes):
        return self._like(boxes=boxes)

    def with_flips(self, flips):
        return self._like(flips=flips)

    def with_mode(self, mode):
        return self._like(mode=mode)

    def items(self):
        """The clipmi_image_item table (host)."""
        arr = (ImageItem * max(len(self), 1))()
        for i, ((h, w), o, (x0, y0, cw, ch), f) in enumerate(zip(self.sizes, self.offsets, self.boxes, self.flips)):
            arr[i] = ImageItem(o, h, w, x0, y0, cw, ch, f)
        return arr


def preprocess(batch, image_size, mode=None, out=None):
    """ImageBatch (on the GPU) -> uint8 [B, S, S, 3] on its device, through clipmi_resize_crop_u8.  mode: the
    batch's own when None.  out: a contiguous uint8 view of B*S*S*3 elements to write into."""
    mode = batch.mode if mode is None else mode
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    if not batch.data.is_cuda:
        raise ValueError("preprocess needs the batch on the GPU (batch.to(device)); there is no CPU fallback")
    B, S = len(batch), int(image_size)
    items = batch.items()
    L = _lib.lib()
    nb = int(L.clipmi_resize_crop_u8_ws(items, B, S, MODES[mode]))
    if nb < 0:
        _lib.check(nb, "clipmi_resize_crop_u8_ws")
    with torch.cuda.device(batch.data.device):
        if out is None:
            out = torch.empty(B, S, S, 3, dtype=torch.uint8, device=batch.data.device)
        elif out.dtype != torch.uint8 or out.numel() != B * S * S * 3 or not out.is_contiguous():
            raise ValueError("preprocess: out must be a contiguous uint8 view of B*S*S*3 elements")
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=batch.data.device)
        _lib.check(L.clipmi_resize_crop_u8(K.stream(), K.ptr(batch.data), batch.data.numel(), items, B, K.ptr(out), S,
                                           MODES[mode], K.ptr(ws), nb), "clipmi_resize_crop_u8")
    return out.view(B, S, S, 3)


def _uniform(generator, lo, hi):
    return lo + (hi - lo) * float(torch.rand((), generator=generator))


def fallback_box(h, w, ratio=(3 / 4, 4 / 3)):
    """RandomResizedCrop's fallback: the centre crop with the aspect ratio clamped to the bounds."""
    in_ratio = w / h
    if in_ratio < min(ratio):
        cw, ch = w, min(h, int(round(w / min(ratio))))
    elif in_ratio > max(ratio):
        cw, ch = min(w, int(round(h * max(ratio)))), h
    else:
        cw, ch = w, h
    return ((w - cw) // 2, (h - ch) // 2, cw, ch)


def random_resized_crop_boxes(sizes, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), generator=None):
    """One box (x0, y0, cw, ch) per (h, w) in sizes by the published RandomResizedCrop.get_params algorithm: up
    to ten tries of area * U(scale) with a log-uniform aspect ratio, the first with cw <= w and ch <= h placed
    uniformly; else ``fallback_box``.  Host-side, from a CPU torch.Generator: a seed fixes the boxes."""
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
    boxes = []
    for h, w in sizes:
        box = None
        for _ in range(10):
            target = h * w * _uniform(generator, scale[0], scale[1])
            ar = math.exp(_uniform(generator, log_ratio[0], log_ratio[1]))
            cw, ch = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
            if 0 < cw <= w and 0 < ch <= h:
                y0 = int(torch.randint(0, h - ch + 1, (), generator=generator))
                x0 = int(torch.randint(0, w - cw + 1, (), generator=generator))
                box = (x0, y0, cw, ch)
                break
        boxes.append(box if box is not None else fallback_box(h, w, ratio))
    return boxes


def random_flips(B, p=0.5, generator=None):
    """B flip bits, each 1 with probability p."""
    return [int(v) for v in (torch.rand(B, generator=generator) < p)]


class TrainAugment:
    """ImageBatch -> ImageBatch with a random-resized-crop box and a flip bit per image, ``mode="square"``.
    Its own generator (``seed``) makes a run reproducible."""

    def __init__(self, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5, seed=0):
        self.scale, self.ratio, self.flip_p = tuple(scale), tuple(ratio), float(flip_p)
        self.generator = torch.Generator(device="cpu").manual_seed(int(seed))

    def __call__(self, batch):
        boxes = random_resized_crop_boxes(batch.sizes, self.scale, self.ratio, self.generator)
        flips = random_flips(len(batch), self.flip_p, self.generator)
        return batch.with_boxes(boxes).with_flips(flips).with_mode("square")


def collate(samples):
    """DataLoader collate_fn for dict samples: every sample's ``"image"`` (uint8 [H, W, 3], any size) packed into
    an ImageBatch under ``"pixel_values"``; the other tensor fields stacked, anything else listed."""
    out = {"pixel_values": ImageBatch.pack([s["image"] for s in samples])}
    for k in samples[0]:
        if k == "image":
            continue
        vals = [s[k] for s in samples]
        out[k] = torch.stack(vals) if isinstance(vals[0], torch.Tensor) else vals
    return out
