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
its own seeded generator, ``CLIPAdapterTrainer(augment=...)`` applies it in ``train_step`` only.

Colour: ``color_jitter_u8`` runs torchvision's ColorJitter / RandomGrayscale as they act on PIL images
(ImageEnhance.Brightness / Contrast / Color, the 8-bit HSV hue shift, convert("L")) bit for bit on uint8
[B, H, W, 3] in place, each image with its own factors and op order (include/clipmi.h clipmi_color_u8: two
launches whatever B is).  ``ColorJitter`` samples the per-image records as ColorJitter.get_params does;
an ``ImageBatch`` that carries records (``with_color``) gets them applied by ``preprocess`` after the
resize, the window and the flip.

Geometry: ``affine_u8`` is PIL's ``Image.transform(size, AFFINE, m, NEAREST | BILINEAR, fillcolor=...)`` bit for
bit on uint8 [B, H, W, 3], each image with its own matrix, filter and fill (include/clipmi.h clipmi_affine_u8: one
launch whatever B is), which is what torchvision's RandomAffine / RandomRotation do to a PIL image.
``rotation_matrix`` is Image.rotate's matrix, ``affine_matrix`` torchvision's published inverse affine matrix;
``RandomAffine`` / ``RandomRotation`` sample per-image ``AffineItem`` records as their ``get_params`` do.  An
``ImageBatch`` that carries them (``with_affine``) gets them applied by ``preprocess`` after the resize, the window
and the flip and in front of the colour records: Compose([RandomResizedCrop, RandomHorizontalFlip, RandomAffine,
ColorJitter]).

Policies: ``enhance_u8`` is PIL's ImageOps.posterize / solarize / autocontrast / equalize and ImageEnhance.Sharpness
bit for bit, each image with its own op (include/clipmi.h clipmi_enhance_u8: at most three launches whatever B is).
``apply_policy_u8`` runs a per-image sequence of torchvision's fourteen policy ops over the three kernel families,
stage by stage, so its launches are bounded per stage and not per image; ``RandAugment`` and ``TrivialAugmentWide``
sample such sequences as the published torchvision classes do.  An ``ImageBatch`` that carries them (``with_policy``)
gets them applied by ``preprocess`` after the resize, the window and the flip and in front of the affine and the
colour records."""
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


class ColorItem(ctypes.Structure):
    """include/clipmi.h clipmi_color_item.  ``ColorItem.of`` builds one from an op list."""
    _fields_ = [("brightness", ctypes.c_float), ("contrast", ctypes.c_float), ("saturation", ctypes.c_float),
                ("hue_shift", ctypes.c_int32), ("order", ctypes.c_int32), ("gray", ctypes.c_int32)]

    @classmethod
    def of(cls, ops=(), gray=0):
        """ops: [(name, value)] in the order they run, name in COLOR_OPS, each at most once; value a blend factor
        (brightness, contrast, saturation: 1 leaves the image as it is) or the hue shift 0..255 added to PIL's H."""
        it = cls(1.0, 1.0, 1.0, 0, 0, int(gray))
        if len(ops) > 4:
            raise ValueError("ColorItem.of: at most four ops")
        for k, (name, value) in enumerate(ops):
            if name not in COLOR_OPS:
                raise ValueError(f"ColorItem.of: op must be one of {sorted(COLOR_OPS)}, got {name!r}")
            setattr(it, "hue_shift" if name == "hue" else name, int(value) if name == "hue" else float(value))
            it.order |= COLOR_OPS[name] << (4 * k)
        return it

    def ops(self):
        """[(name, value)] in the order they run."""
        names = {v: k for k, v in COLOR_OPS.items()}
        out, order = [], self.order
        while order & 15:
            name = names[order & 15]
            out.append((name, self.hue_shift if name == "hue" else getattr(self, name)))
            order >>= 4
        return out


COLOR_OPS = {"brightness": 1, "contrast": 2, "saturation": 3, "hue": 4}
AFFINE_FILTERS = {"nearest": 0, "bilinear": 1}


def _fill_code(who, fill):
    """A fill colour, an int (gray) or an (r, g, b) triple of bytes, as 0xRRGGBB."""
    if isinstance(fill, (tuple, list)):
        rgb = tuple(fill)
    elif isinstance(fill, (int, float)):
        rgb = (fill,) * 3
    else:
        rgb = ()
    if len(rgb) != 3 or not all(isinstance(v, (int, float)) and v == int(v) and 0 <= v <= 255 for v in rgb):
        raise ValueError(f"{who}: fill must be an int in 0..255 or an (r, g, b) triple of them, got {fill!r}")
    r, g, b = (int(v) for v in rgb)
    return r << 16 | g << 8 | b


def _filter_code(who, interpolation):
    if interpolation not in AFFINE_FILTERS:
        raise ValueError(f"{who}: interpolation must be one of {sorted(AFFINE_FILTERS)}, got {interpolation!r}")
    return AFFINE_FILTERS[interpolation]


class AffineItem(ctypes.Structure):
    """include/clipmi.h clipmi_affine_item.  ``AffineItem.of`` builds one from a matrix."""
    _fields_ = [("m", ctypes.c_double * 6), ("filter", ctypes.c_int32), ("fill", ctypes.c_int32)]

    @classmethod
    def of(cls, matrix, interpolation="nearest", fill=0):
        """matrix: (a0..a5), output pixel -> source coordinate, PIL's AFFINE data; interpolation: "nearest" |
        "bilinear"; fill: the colour where no source pixel is hit, an int (gray) or an (r, g, b) triple."""
        m = [float(v) for v in matrix]
        if len(m) != 6:
            raise ValueError(f"AffineItem.of: the matrix has six coefficients, got {len(m)}")
        return cls((ctypes.c_double * 6)(*m), _filter_code("AffineItem.of", interpolation), _fill_code("AffineItem.of", fill))

    @property
    def matrix(self):
        return list(self.m)

    @property
    def interpolation(self):
        return {v: k for k, v in AFFINE_FILTERS.items()}[self.filter]

    def is_identity(self):
        return self.matrix == AFFINE_IDENTITY


AFFINE_IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
ENHANCE_OPS = {"none": 0, "posterize": 1, "solarize": 2, "autocontrast": 3, "equalize": 4, "sharpness": 5}


class EnhanceItem(ctypes.Structure):
    """include/clipmi.h clipmi_enhance_item.  ``EnhanceItem.of`` builds one from an op name."""
    _fields_ = [("op", ctypes.c_int32), ("value", ctypes.c_float)]

    @classmethod
    def of(cls, name, value=0):
        """name in ENHANCE_OPS; value: posterize's bits (an integer in 1..8), solarize's threshold, sharpness's
        factor (1 leaves the image as it is); "none", "autocontrast" and "equalize" take none."""
        if name not in ENHANCE_OPS:
            raise ValueError(f"EnhanceItem.of: op must be one of {sorted(ENHANCE_OPS)}, got {name!r}")
        return cls(ENHANCE_OPS[name], float(value))

    @property
    def name(self):
        return {v: k for k, v in ENHANCE_OPS.items()}[self.op]


_lib.declare("clipmi_resize_crop_u8_ws", [ctypes.POINTER(ImageItem), ctypes.c_int, ctypes.c_int, ctypes.c_int],
             ctypes.c_int64)
_lib.declare("clipmi_resize_crop_u8", [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ImageItem),
                                       ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_int64])
_lib.declare("clipmi_color_u8_ws", [ctypes.POINTER(ColorItem), ctypes.c_int, ctypes.c_int, ctypes.c_int],
             ctypes.c_int64)
_lib.declare("clipmi_color_u8", [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ColorItem), ctypes.c_int,
                                 ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64])
_lib.declare("clipmi_affine_u8_ws", [ctypes.POINTER(AffineItem), ctypes.c_int, ctypes.c_int, ctypes.c_int],
             ctypes.c_int64)
_lib.declare("clipmi_affine_u8", [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(AffineItem),
                                  ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64])
_lib.declare("clipmi_enhance_u8_ws", [ctypes.POINTER(EnhanceItem), ctypes.c_int, ctypes.c_int, ctypes.c_int],
             ctypes.c_int64)
_lib.declare("clipmi_enhance_u8", [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(EnhanceItem),
                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64])


class ImageBatch:
    """B channels-last RGB uint8 images of different sizes in one flat buffer.

    ``data``: uint8 [sum h*w*3] (host, pinned when CUDA is available, or device after ``.to``);
    ``sizes``: [(h, w)]; ``offsets``: byte offset of each image; ``boxes``: [(x0, y0, cw, ch)] (default:
    the whole image); ``flips``: [0 | 1] (default 0); ``mode``: "processor" | "square"; ``color``: one ColorItem
    per image, applied to ``preprocess``'s output (default None: no colour pass); ``affine``: one AffineItem per
    image, applied after the resize, the window and the flip and in front of ``color`` (default None: no such pass);
    ``policy``: (programs, interpolation, fill) as ``with_policy`` stores them, one policy program per image, run
    through ``apply_policy_u8`` after the resize, the window and the flip and in front of ``affine`` and ``color``
    (default None: no such pass)."""

    def __init__(self, data, sizes, offsets, boxes=None, flips=None, mode="processor", color=None, affine=None,
                 policy=None):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
        self.data = data
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        self.offsets = [int(o) for o in offsets]
        n = len(self.sizes)
        self.boxes = [(0, 0, w, h) for h, w in self.sizes] if boxes is None else [tuple(int(v) for v in b) for b in boxes]
        self.flips = [0] * n if flips is None else [int(f) for f in flips]
        self.mode = mode
        self.color = None if color is None else list(color)
        if self.color is not None and len(self.color) != n:
            raise ValueError("ImageBatch: color must have one ColorItem per image")
        self.affine = None if affine is None else list(affine)
        if self.affine is not None and (len(self.affine) != n or
                                        not all(isinstance(it, AffineItem) for it in self.affine)):
            raise ValueError("ImageBatch: affine must have one AffineItem per image")
        self.policy = None
        if policy is not None:
            programs, interpolation, fill = policy
            _filter_code("ImageBatch", interpolation)
            _fill_code("ImageBatch", 0 if fill is None else fill)
            self.policy = (_check_programs("ImageBatch", programs, n), interpolation, fill)
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
                 mode=self.mode, color=self.color, affine=self.affine, policy=self.policy)
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

    def with_color(self, items):
        return self._like(color=items)

    def with_affine(self, items):
        return self._like(affine=items)

    def with_policy(self, programs, interpolation="nearest", fill=0):
        """programs[b]: image b's [(op name, magnitude)] (``apply_policy_u8``; RandAugment / TrivialAugmentWide
        ``sample``); None removes them."""
        return self._like(policy=None if programs is None else (programs, interpolation, fill))

    def items(self):
        """The clipmi_image_item table (host)."""
        arr = (ImageItem * max(len(self), 1))()
        for i, ((h, w), o, (x0, y0, cw, ch), f) in enumerate(zip(self.sizes, self.offsets, self.boxes, self.flips)):
            arr[i] = ImageItem(o, h, w, x0, y0, cw, ch, f)
        return arr


def preprocess(batch, image_size, mode=None, out=None):
    """ImageBatch (on the GPU) -> uint8 [B, S, S, 3] on its device, through clipmi_resize_crop_u8.  mode: the
    batch's own when None.  out: a contiguous uint8 view of B*S*S*3 elements to write into.  A batch with affine
    records (``with_affine``) has the resize write a scratch [B, S, S, 3] and clipmi_affine_u8 write the output (one
    more launch); a batch with colour records (``with_color``) then gets them applied to the output in place
    (clipmi_color_u8, two more launches).  A batch with policy programs (``with_policy``) has them run by
    ``apply_policy_u8`` on the resize's output, in front of the affine and the colour records: where
    Compose([RandomResizedCrop, RandomHorizontalFlip, RandAugment, ...]) puts them."""
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
        out = out.view(B, S, S, 3)
        # every out-of-place pass reads a scratch tensor; the last one writes the output
        passes = (batch.policy is not None) + (batch.affine is not None)
        resized = out if passes == 0 else torch.empty_like(out)
        _lib.check(L.clipmi_resize_crop_u8(K.stream(), K.ptr(batch.data), batch.data.numel(), items, B, K.ptr(resized),
                                           S, MODES[mode], K.ptr(ws), nb), "clipmi_resize_crop_u8")
    if batch.policy is not None:
        programs, interpolation, fill = batch.policy
        resized = apply_policy_u8(resized, programs, interpolation, fill, out=out if passes == 1 else None)
    if batch.affine is not None:
        affine_u8(resized, batch.affine, out=out)
    if batch.color is not None:
        color_jitter_u8(out, batch.color)
    return out


def _color_table(items):
    """A ColorItem sequence as the ctypes array the library takes."""
    n = len(items)
    if not all(isinstance(it, ColorItem) for it in items):
        raise ValueError("colour records must be ColorItem (ColorItem.of, ColorJitter.sample)")
    return (ColorItem * max(n, 1))(*items), n


def color_jitter_u8(images, items):
    """uint8 [B, H, W, 3] on the GPU through clipmi_color_u8, in place: image b through items[b]'s ops in their
    order, then its grayscale.  Returns ``images``."""
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError("color_jitter_u8: images must be uint8 [B, H, W, 3]")
    if not images.is_cuda:
        raise ValueError("color_jitter_u8 needs the images on the GPU; there is no CPU fallback")
    if not images.is_contiguous():
        raise ValueError("color_jitter_u8 works in place: images must be contiguous")
    B, H, W = (int(v) for v in images.shape[:3])
    table, n = _color_table(items)
    if n != B:
        raise ValueError(f"color_jitter_u8: {n} records for {B} images")
    L = _lib.lib()
    nb = int(L.clipmi_color_u8_ws(table, B, max(H, 1) if B == 0 else H, max(W, 1) if B == 0 else W))
    if nb < 0:
        _lib.check(nb, "clipmi_color_u8_ws")
    if B == 0:
        return images
    with torch.cuda.device(images.device):
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=images.device)
        _lib.check(L.clipmi_color_u8(K.stream(), K.ptr(images), table, B, H, W, K.ptr(ws), nb), "clipmi_color_u8")
    return images


def _affine_table(items):
    """An AffineItem sequence as the ctypes array the library takes."""
    n = len(items)
    if not all(isinstance(it, AffineItem) for it in items):
        raise ValueError("affine records must be AffineItem (AffineItem.of, RandomAffine.sample)")
    return (AffineItem * max(n, 1))(*items), n


def affine_u8(images, items, out=None):
    """uint8 [B, H, W, 3] on the GPU through clipmi_affine_u8: image b through items[b]'s matrix, filter and fill.
    Returns a new tensor, or ``out`` (uint8 [B, H, W, 3], contiguous, on the same device, no byte shared with
    ``images``).  ``images`` is left as it is."""
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError("affine_u8: images must be uint8 [B, H, W, 3]")
    if not images.is_cuda:
        raise ValueError("affine_u8 needs the images on the GPU; there is no CPU fallback")
    if not images.is_contiguous():
        raise ValueError("affine_u8: images must be contiguous")
    B, H, W = (int(v) for v in images.shape[:3])
    table, n = _affine_table(items)
    if n != B:
        raise ValueError(f"affine_u8: {n} records for {B} images")
    if out is not None:
        _check_out("affine_u8", images, out, "every output pixel gathers from the source image")
    L = _lib.lib()
    nb = int(L.clipmi_affine_u8_ws(table, B, max(H, 1) if B == 0 else H, max(W, 1) if B == 0 else W))
    if nb < 0:
        _lib.check(nb, "clipmi_affine_u8_ws")
    with torch.cuda.device(images.device):
        if out is None:
            out = torch.empty_like(images)
        if B == 0:
            return out
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=images.device)
        _lib.check(L.clipmi_affine_u8(K.stream(), K.ptr(images), K.ptr(out), table, B, H, W, K.ptr(ws), nb),
                   "clipmi_affine_u8")
    return out


def _check_out(who, images, out, why):
    """``out`` as an out-of-place call takes it: images' shape, dtype and device, contiguous, no byte shared."""
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or tuple(out.shape) != tuple(images.shape)
            or not out.is_contiguous() or out.device != images.device):
        raise ValueError(f"{who}: out must be a contiguous uint8 tensor of images' shape on images' device")
    lo, hi, nbytes = images.data_ptr(), out.data_ptr(), images.numel()
    if nbytes and lo < hi + nbytes and hi < lo + nbytes:
        raise ValueError(f"{who}: out must not alias images ({why})")


def enhance_u8(images, items, out=None):
    """uint8 [B, H, W, 3] on the GPU through clipmi_enhance_u8: image b through items[b]'s op (EnhanceItem.of:
    posterize, solarize, autocontrast, equalize, sharpness as PIL's ImageOps / ImageEnhance do them, or none).
    Returns a new tensor, or ``out`` (uint8 [B, H, W, 3], contiguous, on the same device, no byte shared with
    ``images``).  ``images`` is left as it is."""
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError("enhance_u8: images must be uint8 [B, H, W, 3]")
    if not images.is_cuda:
        raise ValueError("enhance_u8 needs the images on the GPU; there is no CPU fallback")
    if not images.is_contiguous():
        raise ValueError("enhance_u8: images must be contiguous")
    B, H, W = (int(v) for v in images.shape[:3])
    n = len(items)
    if not all(isinstance(it, EnhanceItem) for it in items):
        raise ValueError("enhance records must be EnhanceItem (EnhanceItem.of)")
    if n != B:
        raise ValueError(f"enhance_u8: {n} records for {B} images")
    table = (EnhanceItem * max(n, 1))(*items)
    if out is not None:
        _check_out("enhance_u8", images, out, "sharpness reads every pixel's neighbours")
    L = _lib.lib()
    nb = int(L.clipmi_enhance_u8_ws(table, B, max(H, 1) if B == 0 else H, max(W, 1) if B == 0 else W))
    if nb < 0:
        _lib.check(nb, "clipmi_enhance_u8_ws")
    with torch.cuda.device(images.device):
        if out is None:
            out = torch.empty_like(images)
        if B == 0:
            return out
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=images.device)
        _lib.check(L.clipmi_enhance_u8(K.stream(), K.ptr(images), K.ptr(out), table, B, H, W, K.ptr(ws), nb),
                   "clipmi_enhance_u8")
    return out


# torchvision's policy ops (autoaugment._apply_op), in the order of RandAugment's and TrivialAugmentWide's op table
POLICY_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
              "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
_POLICY_AFFINE = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
_POLICY_COLOR = {"Brightness": "brightness", "Color": "saturation", "Contrast": "contrast"}
_POLICY_ENHANCE = {"Sharpness": "sharpness", "Posterize": "posterize", "Solarize": "solarize",
                   "AutoContrast": "autocontrast", "Equalize": "equalize"}


def _check_programs(who, programs, n):
    """programs as [[(op name, float magnitude)]], one list per image."""
    programs = [list(p) for p in programs]
    if len(programs) != n:
        raise ValueError(f"{who}: {len(programs)} programs for {n} images")
    out = []
    for b, prog in enumerate(programs):
        ops = []
        for op in prog:
            if not isinstance(op, (tuple, list)) or len(op) != 2 or op[0] not in POLICY_OPS:
                raise ValueError(f"{who}: program {b}: an op is (name, magnitude) with name in {list(POLICY_OPS)}, "
                                 f"got {op!r}")
            ops.append((op[0], float(op[1])))
        out.append(ops)
    return out


def policy_matrix(name, m, w, h):
    """The matrix autoaugment._apply_op hands to PIL for a geometric op of magnitude m on a w x h image."""
    if name == "ShearX":
        return affine_matrix(0.0, (0, 0), 1.0, (math.degrees(math.atan(m)), 0.0), w, h, center=(0, 0))
    if name == "ShearY":
        return affine_matrix(0.0, (0, 0), 1.0, (0.0, math.degrees(math.atan(m))), w, h, center=(0, 0))
    if name == "TranslateX":
        return affine_matrix(0.0, (int(m), 0), 1.0, (0.0, 0.0), w, h)
    if name == "TranslateY":
        return affine_matrix(0.0, (0, int(m)), 1.0, (0.0, 0.0), w, h)
    if name == "Rotate":
        return rotation_matrix(m, w, h)
    raise ValueError(f"policy_matrix: {name!r} is not one of {list(_POLICY_AFFINE)}")


def policy_calls(programs, w, h, interpolation="nearest", fill=0):
    """The calls ``apply_policy_u8`` makes for these programs on w x h images: [(kind, items)] with kind in
    "affine" | "enhance" | "color" and one record per image.  Stage k holds every image's k-th op (the identity for
    a shorter program); a stage is at most one call of each kind, in that order, and a kind no image of the stage
    uses is left out."""
    return _policy_calls(_check_programs("apply_policy_u8", programs, len(programs)), w, h, interpolation, fill)


def _policy_calls(programs, w, h, interpolation, fill):
    """policy_calls on checked programs.  The records of the images a call leaves alone are one shared instance per
    kind: a call copies its records into a table."""
    filt, fc = _filter_code("apply_policy_u8", interpolation), _fill_code("apply_policy_u8", 0 if fill is None else fill)
    same = {"affine": AffineItem.of(AFFINE_IDENTITY), "enhance": EnhanceItem.of("none"), "color": ColorItem.of([])}

    def record(kind, name, m):
        if kind == "affine":
            return AffineItem((ctypes.c_double * 6)(*policy_matrix(name, m, w, h)), filt, fc)
        if kind == "color":
            return ColorItem.of([(_POLICY_COLOR[name], 1.0 + m)])
        return EnhanceItem.of(_POLICY_ENHANCE[name], {"Sharpness": 1.0 + m, "Posterize": int(m), "Solarize": m}.get(name, 0))

    kind_of = dict([(n, "affine") for n in _POLICY_AFFINE] + [(n, "enhance") for n in _POLICY_ENHANCE] +
                   [(n, "color") for n in _POLICY_COLOR])
    calls = []
    for k in range(max((len(p) for p in programs), default=0)):
        ops = [p[k] if k < len(p) else ("Identity", 0.0) for p in programs]
        kinds = [kind_of.get(name) for name, _ in ops]
        for kind in ("affine", "enhance", "color"):
            if kind in kinds:
                calls.append((kind, [record(kind, name, m) if kd == kind else same[kind]
                                     for kd, (name, m) in zip(kinds, ops)]))
    return calls


def apply_policy_u8(images, programs, interpolation="nearest", fill=0, out=None):
    """uint8 [B, H, W, 3] on the GPU through per-image sequences of torchvision's policy ops, bit for bit what
    autoaugment._apply_op does to PIL images.  programs[b]: [(op name, magnitude)] for image b in the order the ops
    run, names in POLICY_OPS, the magnitude carrying its sign: ShearX / ShearY shear by atan(m) about the corner (0, 0),
    TranslateX / TranslateY shift by int(m) pixels, Rotate turns by m degrees; Brightness / Color / Contrast / Sharpness
    take the factor 1 + m; Posterize keeps int(m) bits; Solarize inverts bytes at or above m (compared as float32);
    Identity, AutoContrast and Equalize take none.  The geometric ops use ``interpolation`` ("nearest" | "bilinear")
    and ``fill`` (None: black).

    Execution is by stage (``policy_calls``): per stage at most one affine_u8, one enhance_u8 and one color_jitter_u8
    call over the whole batch, so the launches are bounded per stage, not per image: at most 2 + 3 + 2.  The
    out-of-place calls go back and forth between two scratch tensors and the last write lands in the result.
    Returns a new tensor, or ``out`` (no byte shared with ``images``); ``images`` is left as it is."""
    if not isinstance(images, torch.Tensor) or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise ValueError("apply_policy_u8: images must be uint8 [B, H, W, 3]")
    if not images.is_cuda:
        raise ValueError("apply_policy_u8 needs the images on the GPU; there is no CPU fallback")
    if not images.is_contiguous():
        raise ValueError("apply_policy_u8: images must be contiguous")
    B, H, W = (int(v) for v in images.shape[:3])
    calls = _policy_calls(_check_programs("apply_policy_u8", programs, B), W, H, interpolation, fill)
    if out is not None:
        _check_out("apply_policy_u8", images, out, "the first op reads the source while the result is written")
    with torch.cuda.device(images.device):
        if out is None:
            out = torch.empty_like(images)
        moves = sum(kind != "color" for kind, _ in calls)  # out-of-place calls still to come
        scratch = []
        cur = images

        def target():
            """Where the next write goes: ``out`` when no out-of-place call follows, else a scratch tensor that is
            not the one being read."""
            if moves == 0:
                return out
            for t in scratch:
                if t is not cur:
                    return t
            scratch.append(torch.empty_like(images))
            return scratch[-1]

        for kind, items in calls:
            if kind == "color":
                if cur is images:  # the in-place call must not touch the source
                    cur = target().copy_(images)
                color_jitter_u8(cur, items)
            else:
                moves -= 1
                cur = (affine_u8 if kind == "affine" else enhance_u8)(cur, items, out=target())
        if cur is not out:  # nothing ran
            out.copy_(images)
    return out


def rotation_matrix(angle, w, h, center=None):
    """PIL Image.rotate's matrix for a w x h image (PIL/Image.py): counter-clockwise by ``angle`` degrees about
    ``center`` (default (w / 2, h / 2)), as output pixel -> source coordinate."""
    angle = angle % 360.0
    cx, cy = (w / 2.0, h / 2.0) if center is None else (float(center[0]), float(center[1]))
    t = -math.radians(angle)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return m


def affine_matrix(angle=0.0, translate=(0, 0), scale=1.0, shear=(0.0, 0.0), w=1, h=1, center=None):
    """torchvision's published _get_inverse_affine_matrix as F.affine calls it for a w x h PIL image: the inverse of
    T * C * R(angle) * Shear(shear) * Scale(scale) * C^-1 with C the translation to ``center`` (default (w * 0.5,
    h * 0.5)); angle and shear (x, y) in degrees, translate (tx, ty) in pixels."""
    cx, cy = (w * 0.5, h * 0.5) if center is None else (float(center[0]), float(center[1]))
    tx, ty = translate
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [v / scale for v in (d, -b, 0.0, -c, a, 0.0)]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


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


def _jitter_range(name, value, center, bound=None):
    """torchvision's ColorJitter._check_input: a number v is [max(0, center - v), center + v] (hue: [-v, v]), a pair
    is (lo, hi); None when the op is disabled (None, 0, or a range that is the centre alone)."""
    if value is None:
        return None
    if isinstance(value, (int, float)):
        if not math.isfinite(value) or value < 0:
            raise ValueError(f"ColorJitter: {name} must be a finite number >= 0, got {value}")
        lo, hi = center - float(value), center + float(value)
        if bound is None:
            lo = max(lo, 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        lo, hi = float(value[0]), float(value[1])
    else:
        raise ValueError(f"ColorJitter: {name} must be a number or a (lo, hi) pair, got {value!r}")
    lim = (0.0, math.inf) if bound is None else bound
    if not (math.isfinite(lo) and math.isfinite(hi) and lim[0] <= lo <= hi <= lim[1]):
        raise ValueError(f"ColorJitter: {name} range ({lo}, {hi}) must be ordered and inside "
                         f"[{lim[0]}, {lim[1]}]")
    return None if lo == hi == center else (lo, hi)


def hue_shift_of(factor):
    """A hue factor in [-0.5, 0.5] as the byte torchvision's PIL path adds to H: int(f * 255), truncated toward
    zero, wrapped to 0..255."""
    return int(factor * 255) % 256


class ColorJitter:
    """torchvision's ColorJitter (+ RandomGrayscale with probability ``grayscale_p``) as a sampler of per-image
    ColorItem records.  ``brightness`` / ``contrast`` / ``saturation``: v for factors in [max(0, 1 - v), 1 + v], or
    (lo, hi) with 0 <= lo <= hi; ``hue``: h for [-h, h] with 0 <= h <= 0.5, or a pair inside [-0.5, 0.5]; 0 / None
    disables an op.  ``sample(B, generator)`` follows ColorJitter.get_params per image: a random permutation of the
    ops, then a uniform factor for each enabled one (disabled ones are left out of the list), then the grayscale
    coin when ``grayscale_p`` > 0; all from the CPU generator given, so a seed fixes the records."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, grayscale_p=0):
        self.ranges = {"brightness": _jitter_range("brightness", brightness, 1.0),
                       "contrast": _jitter_range("contrast", contrast, 1.0),
                       "saturation": _jitter_range("saturation", saturation, 1.0),
                       "hue": _jitter_range("hue", hue, 0.0, (-0.5, 0.5))}
        self.grayscale_p = float(grayscale_p)
        if not 0.0 <= self.grayscale_p <= 1.0:
            raise ValueError(f"ColorJitter: grayscale_p must be in [0, 1], got {grayscale_p}")

    def sample(self, B, generator=None):
        names = list(COLOR_OPS)  # get_params' fn_idx numbering: brightness, contrast, saturation, hue
        items = []
        for _ in range(int(B)):
            perm = torch.randperm(4, generator=generator).tolist()
            vals = {}
            for name in names:
                r = self.ranges[name]
                if r is not None:
                    f = _uniform(generator, r[0], r[1])
                    vals[name] = hue_shift_of(f) if name == "hue" else f
            gray = int(float(torch.rand((), generator=generator)) < self.grayscale_p) if self.grayscale_p > 0 else 0
            items.append(ColorItem.of([(names[i], vals[names[i]]) for i in perm if names[i] in vals], gray))
        return items


def _number_range(who, name, value, n=(2,)):
    """torchvision's _setup_angle: a number d is (-d, d) with d >= 0; else a sequence of one of the lengths n."""
    if isinstance(value, (int, float)) and not isinstance(value, bool):
        if not math.isfinite(value) or value < 0:
            raise ValueError(f"{who}: a single {name} must be a finite number >= 0, got {value}")
        return (-float(value), float(value))
    if not isinstance(value, (tuple, list)) or len(value) not in n or \
            not all(isinstance(v, (int, float)) and math.isfinite(v) for v in value):
        raise ValueError(f"{who}: {name} must be a number or a sequence of {' or '.join(map(str, n))} numbers, got {value!r}")
    return tuple(float(v) for v in value)


def _check_p(who, p):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{who}: p must be in [0, 1], got {p}")
    return p


def _check_center(who, center):
    if center is None:
        return None
    if not isinstance(center, (tuple, list)) or len(center) != 2:
        raise ValueError(f"{who}: center must be an (x, y) pair, got {center!r}")
    return (float(center[0]), float(center[1]))


class RandomAffine:
    """torchvision's RandomAffine on PIL images as a sampler of per-image AffineItem records.  ``degrees``: d for
    angles in (-d, d), or (lo, hi); ``translate``: (fx, fy) fractions in [0, 1] of the width and the height;
    ``scale``: a positive (lo, hi); ``shear``: s for an x shear in (-s, s), (lo, hi), or (xlo, xhi, ylo, yhi), in
    degrees; ``interpolation``: "nearest" | "bilinear"; ``fill``: an int or an (r, g, b) triple; ``center``: the
    image centre when None; ``p``: the probability that an image is transformed at all (RandomApply).
    ``sample(B, size, generator)`` with size = (w, h), or a number for a square, follows RandomAffine.get_params per
    image: the angle, then tx and ty (int(round(U(-max_d, max_d))), max_dx = translate[0] * w), then the scale, then
    shear_x and, for a 4-tuple, shear_y.  With p < 1 one uniform is drawn first and an image that is skipped gets the
    identity item and no further draws; with p == 1 no coin is drawn.  expand is not offered."""

    def __init__(self, degrees, translate=None, scale=None, shear=None, interpolation="nearest", fill=0, center=None,
                 p=1.0):
        who = type(self).__name__
        self.degrees = _number_range(who, "degrees", degrees)
        if translate is not None:
            if not isinstance(translate, (tuple, list)) or len(translate) != 2 or \
                    not all(isinstance(t, (int, float)) and 0.0 <= t <= 1.0 for t in translate):
                raise ValueError(f"{who}: translate must be a pair of fractions in [0, 1], got {translate!r}")
            translate = (float(translate[0]), float(translate[1]))
        self.translate = translate
        if scale is not None:
            if not isinstance(scale, (tuple, list)) or len(scale) != 2 or \
                    not all(isinstance(v, (int, float)) and math.isfinite(v) and v > 0 for v in scale):
                raise ValueError(f"{who}: scale must be a pair of positive numbers, got {scale!r}")
            scale = (float(scale[0]), float(scale[1]))
        self.scale = scale
        self.shear = None if shear is None else _number_range(who, "shear", shear, (2, 4))
        self.filter = _filter_code(who, interpolation)
        self.interpolation = interpolation
        self.fill = _fill_code(who, fill)
        self.center = _check_center(who, center)
        self.p = _check_p(who, p)

    def params(self, w, h, generator=None):
        """One get_params draw: (angle, (tx, ty), scale, (shear_x, shear_y))."""
        angle = _uniform(generator, self.degrees[0], self.degrees[1])
        tx = ty = 0
        if self.translate is not None:
            max_dx, max_dy = float(self.translate[0] * w), float(self.translate[1] * h)
            tx = int(round(_uniform(generator, -max_dx, max_dx)))
            ty = int(round(_uniform(generator, -max_dy, max_dy)))
        scale = 1.0 if self.scale is None else _uniform(generator, self.scale[0], self.scale[1])
        shear_x = shear_y = 0.0
        if self.shear is not None:
            shear_x = _uniform(generator, self.shear[0], self.shear[1])
            if len(self.shear) == 4:
                shear_y = _uniform(generator, self.shear[2], self.shear[3])
        return angle, (tx, ty), scale, (shear_x, shear_y)

    def matrix(self, w, h, generator=None):
        angle, translate, scale, shear = self.params(w, h, generator)
        return affine_matrix(angle, translate, scale, shear, w, h, self.center)

    def sample(self, B, size, generator=None):
        w, h = (size, size) if isinstance(size, (int, float)) else size
        w, h = int(w), int(h)
        items = []
        for _ in range(int(B)):
            if self.p < 1.0 and not float(torch.rand((), generator=generator)) < self.p:
                m = AFFINE_IDENTITY
            else:
                m = self.matrix(w, h, generator)
            it = AffineItem.of(m, self.interpolation)
            it.fill = self.fill
            items.append(it)
        return items


class RandomRotation(RandomAffine):
    """torchvision's RandomRotation on PIL images (Image.rotate without expand) as a sampler of per-image AffineItem
    records: one uniform angle per image from ``degrees`` (d for (-d, d), or (lo, hi)), counter-clockwise, through
    ``rotation_matrix``.  ``p`` as in RandomAffine."""

    def __init__(self, degrees, interpolation="nearest", fill=0, center=None, p=1.0):
        super().__init__(degrees, interpolation=interpolation, fill=fill, center=center, p=p)

    def matrix(self, w, h, generator=None):
        return rotation_matrix(_uniform(generator, self.degrees[0], self.degrees[1]), w, h, self.center)


class _PolicySampler:
    """What RandAugment and TrivialAugmentWide share: the op table of the published torchvision classes (POLICY_OPS in
    its order; per op a float32 ``torch.linspace`` / ``arange`` table of magnitudes, or none, and whether the sign is
    drawn) and the draws, all from the CPU generator given: per op ``randint(14)`` for the op; for TrivialAugmentWide
    only, and only for an op with a table, ``randint(bins)`` for the magnitude; only for a signed op ``randint(2)``,
    where 1 negates.  A magnitude is ``float(table[idx])``.  torchvision itself is not a dependency and was not at
    hand when this was written: the samplers are pinned to the published definition through hand-derived values
    (tests/test_cpu_enhance.py), not to torchvision's own draws."""

    def __init__(self, num_magnitude_bins, interpolation, fill):
        who = type(self).__name__
        self.num_magnitude_bins = int(num_magnitude_bins)
        if self.num_magnitude_bins < 2:
            raise ValueError(f"{who}: num_magnitude_bins must be >= 2, got {num_magnitude_bins}")
        _filter_code(who, interpolation)
        _fill_code(who, 0 if fill is None else fill)
        self.interpolation, self.fill = interpolation, fill

    def space(self, w, h):
        """{op name: (table or None, signed)} for a w x h image, in POLICY_OPS' order."""
        raise NotImplementedError

    def _space(self, w, h, shear, translate_x, translate_y, rotate, enhance, posterize_steps):
        bins = self.num_magnitude_bins
        lin = lambda hi: torch.linspace(0.0, hi, bins)  # noqa: E731
        posterize = 8 - (torch.arange(bins) / ((bins - 1) / posterize_steps)).round().int()
        return {"Identity": (None, False), "ShearX": (lin(shear), True), "ShearY": (lin(shear), True),
                "TranslateX": (lin(translate_x), True), "TranslateY": (lin(translate_y), True),
                "Rotate": (lin(rotate), True), "Brightness": (lin(enhance), True), "Color": (lin(enhance), True),
                "Contrast": (lin(enhance), True), "Sharpness": (lin(enhance), True), "Posterize": (posterize, False),
                "Solarize": (torch.linspace(255.0, 0.0, bins), False), "AutoContrast": (None, False),
                "Equalize": (None, False)}

    def _index(self, table, generator):
        raise NotImplementedError

    def _draw(self, space, generator):
        name = POLICY_OPS[int(torch.randint(len(POLICY_OPS), (1,), generator=generator))]
        table, signed = space[name]
        magnitude = 0.0 if table is None else float(table[self._index(table, generator)])
        if signed and int(torch.randint(2, (1,), generator=generator)):
            magnitude *= -1.0
        return name, magnitude

    def sample(self, B, size, generator=None):
        """B programs ([(op name, magnitude)]) for images of ``size`` = (w, h), or a number for a square."""
        w, h = (size, size) if isinstance(size, (int, float)) else size
        space = self.space(int(w), int(h))
        assert tuple(space) == POLICY_OPS
        return [[self._draw(space, generator) for _ in range(self.num_ops)] for _ in range(int(B))]


class RandAugment(_PolicySampler):
    """torchvision's RandAugment on PIL images as a sampler of per-image policy programs for ``apply_policy_u8`` /
    ``ImageBatch.with_policy``: ``num_ops`` ops per image, each uniform over the fourteen POLICY_OPS, every magnitude
    the table entry at ``magnitude`` (of ``num_magnitude_bins``): shears to 0.3, translations to 150 / 331 of the
    width or height, rotations to 30 degrees, enhancement factors 1 +- up to 0.9, posterize 8 down to 4 bits,
    solarize thresholds 255 down to 0.  Draw order and tables: see _PolicySampler."""

    def __init__(self, num_ops=2, magnitude=9, num_magnitude_bins=31, interpolation="nearest", fill=0):
        super().__init__(num_magnitude_bins, interpolation, fill)
        self.num_ops, self.magnitude = int(num_ops), int(magnitude)
        if self.num_ops < 0 or not 0 <= self.magnitude < self.num_magnitude_bins:
            raise ValueError(f"RandAugment: num_ops must be >= 0 and magnitude in 0..{self.num_magnitude_bins - 1}, "
                             f"got {num_ops}, {magnitude}")

    def space(self, w, h):
        return self._space(w, h, 0.3, 150.0 / 331.0 * w, 150.0 / 331.0 * h, 30.0, 0.9, 4)

    def _index(self, table, generator):
        return self.magnitude


class TrivialAugmentWide(_PolicySampler):
    """torchvision's TrivialAugmentWide on PIL images as a sampler of per-image policy programs: one op per image,
    uniform over the fourteen POLICY_OPS, its magnitude a uniformly drawn table entry: shears to 0.99, translations
    to 32 pixels, rotations to 135 degrees, enhancement factors 1 +- up to 0.99, posterize 8 down to 2 bits, solarize
    thresholds 255 down to 0.  Draw order and tables: see _PolicySampler."""
    num_ops = 1

    def __init__(self, num_magnitude_bins=31, interpolation="nearest", fill=0):
        super().__init__(num_magnitude_bins, interpolation, fill)

    def space(self, w, h):
        return self._space(w, h, 0.99, 32.0, 32.0, 135.0, 0.99, 6)

    def _index(self, table, generator):
        return int(torch.randint(len(table), (1,), dtype=torch.long, generator=generator))


class TrainAugment:
    """ImageBatch -> ImageBatch with a random-resized-crop box and a flip bit per image, ``mode="square"``, and,
    with ``color`` (a ColorJitter), a colour record per image, and, with ``affine`` (a RandomAffine or a
    RandomRotation) and the output size ``image_size``, an affine record per image, and, with ``policy`` (a
    RandAugment or a TrivialAugmentWide) and ``image_size``, a policy program per image.  Its own generator
    (``seed``) makes a run reproducible; the colour records are drawn after the boxes and the flips, the affine
    records after them and the policy programs last, so a seed gives the same boxes, flips, colour and affine records
    with or without them."""

    def __init__(self, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_p=0.5, seed=0, color=None, affine=None,
                 image_size=None, policy=None):
        self.scale, self.ratio, self.flip_p = tuple(scale), tuple(ratio), float(flip_p)
        self.generator = torch.Generator(device="cpu").manual_seed(int(seed))
        if color is not None and not isinstance(color, ColorJitter):
            raise ValueError("TrainAugment: color must be a ColorJitter or None")
        self.color = color
        if affine is not None and not isinstance(affine, RandomAffine):
            raise ValueError("TrainAugment: affine must be a RandomAffine, a RandomRotation or None")
        self.affine = affine
        if policy is not None and not isinstance(policy, _PolicySampler):
            raise ValueError("TrainAugment: policy must be a RandAugment, a TrivialAugmentWide or None")
        self.policy = policy
        self.image_size = None if image_size is None else int(image_size)

    def __call__(self, batch, image_size=None):
        boxes = random_resized_crop_boxes(batch.sizes, self.scale, self.ratio, self.generator)
        flips = random_flips(len(batch), self.flip_p, self.generator)
        out = batch.with_boxes(boxes).with_flips(flips).with_mode("square")
        if self.color is not None:
            out = out.with_color(self.color.sample(len(batch), self.generator))
        if self.affine is not None:
            size = self.image_size if image_size is None else int(image_size)
            if size is None:
                raise ValueError("TrainAugment: affine records need the output size (image_size here or in the call): "
                                 "the matrices turn about the output's centre and translate by fractions of it")
            out = out.with_affine(self.affine.sample(len(batch), size, self.generator))
        if self.policy is not None:
            size = self.image_size if image_size is None else int(image_size)
            if size is None:
                raise ValueError("TrainAugment: policy programs need the output size (image_size here or in the call): "
                                 "the translations are fractions of it and the rotations turn about its centre")
            out = out.with_policy(self.policy.sample(len(batch), size, self.generator), self.policy.interpolation,
                                  self.policy.fill)
        return out


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
