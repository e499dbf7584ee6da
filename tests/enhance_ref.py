"""The arithmetic csrc/enhance.hip is held to, restated in numpy: PIL's ImageOps.posterize / solarize / autocontrast /
equalize and ImageEnhance.Sharpness on uint8 [H, W, 3] arrays, and ``apply_program``, which runs one image through a
list of torchvision policy ops (autoaugment._apply_op on PIL images) by composing this file with tests/affine_ref.py
and tests/color_ref.py.  tests/test_cpu_enhance.py pins this file to PIL itself; tests/test_gpu_enhance.py holds the
kernels and clipmi.images.apply_policy_u8 to it bit for bit.

Widths: the autocontrast LUT is formed in double (Python floats), the product and the sum rounded separately and the
result truncated; equalize is all integers; ImageFilter.SMOOTH accumulates float32 products of float32 quotients
from 0.5, one row after the other; the sharpness blend is color_ref.blend."""
import math

import numpy as np

import affine_ref as A
import color_ref as C

F32 = np.float32
NONE, POSTERIZE, SOLARIZE, AUTOCONTRAST, EQUALIZE, SHARPNESS = 0, 1, 2, 3, 4, 5
OPS = {"none": NONE, "posterize": POSTERIZE, "solarize": SOLARIZE, "autocontrast": AUTOCONTRAST, "equalize": EQUALIZE,
       "sharpness": SHARPNESS}
POLICY_OPS = ["Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
              "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize"]


def posterize(img, bits):
    bits = int(bits)
    assert 1 <= bits <= 8
    return img & np.uint8(~(2 ** (8 - bits) - 1) & 255)


def solarize(img, threshold):
    """i if i < threshold else 255 - i; the compare on the float."""
    keep = img.astype(np.float64) < float(threshold)
    return np.where(keep, img, 255 - img).astype(np.uint8)


def histogram(ch):
    return np.bincount(ch.reshape(-1), minlength=256).astype(np.int64)


def autocontrast_lut(h):
    """ImageOps.autocontrast(cutoff=0) on one channel's histogram -> uint8 [256]."""
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(max(int(i * scale + offset), 0), 255) for i in range(256)], np.uint8)


def equalize_lut(h):
    """ImageOps.equalize on one channel's histogram -> uint8 [256].  An entry above 255 is stored as 255: Image.point
    clips a list LUT's entries to a byte."""
    nz = [int(v) for v in h if v]
    if len(nz) <= 1:
        return np.arange(256, dtype=np.uint8)
    step = (sum(nz) - nz[-1]) // 255
    if not step:
        return np.arange(256, dtype=np.uint8)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(n // step, 255))
        n += int(h[i])
    return np.array(lut, np.uint8)


def _per_channel(img, lut_of):
    out = np.empty_like(img)
    for c in range(3):
        out[..., c] = lut_of(histogram(img[..., c]))[img[..., c]]
    return out


def autocontrast(img):
    return _per_channel(img, autocontrast_lut)


def equalize(img):
    return _per_channel(img, equalize_lut)


SMOOTH_KERNEL = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], F32) / F32(13)).astype(F32)


def smooth(img):
    """ImageFilter.SMOOTH: the one-pixel frame is copied; inside, a float32 accumulator from 0.5 takes the three rows
    one after the other, each as k0 * left + k1 * mid + k2 * right."""
    H, W, _ = img.shape
    out = img.copy()
    if H < 3 or W < 3:
        return out
    k = SMOOTH_KERNEL
    p = img.astype(F32)
    ss = np.full((H - 2, W - 2, 3), 0.5, F32)
    for j, dy in enumerate((1, 0, -1)):
        rows = p[1 + dy:H - 1 + dy]
        left, mid, right = rows[:, 0:W - 2], rows[:, 1:W - 1], rows[:, 2:W]
        row = ((k[3 * j] * left).astype(F32) + (k[3 * j + 1] * mid).astype(F32)).astype(F32)
        row = (row + (k[3 * j + 2] * right).astype(F32)).astype(F32)
        ss = (ss + row).astype(F32)
    out[1:H - 1, 1:W - 1] = np.where(ss <= 0, 0, np.where(ss >= 255, 255, np.trunc(ss))).astype(np.uint8)
    return out


def sharpness(img, factor):
    return C.blend(smooth(img), img, factor)


def apply_enhance(img, item):
    """One image through (op name or code, value), or anything with .op and .value (clipmi.images.EnhanceItem)."""
    op, value = (item.op, item.value) if hasattr(item, "op") else item
    op = OPS.get(op, op)
    img = np.ascontiguousarray(img)
    if op == NONE:
        return img.copy()
    if op == POSTERIZE:
        return posterize(img, value)
    if op == SOLARIZE:
        return solarize(img, value)
    if op == AUTOCONTRAST:
        return autocontrast(img)
    if op == EQUALIZE:
        return equalize(img)
    assert op == SHARPNESS, op
    return sharpness(img, value)


def fill_code(fill):
    """None | int | (r, g, b) -> 0xRRGGBB."""
    if fill is None:
        return 0
    r, g, b = (fill,) * 3 if isinstance(fill, (int, float)) else fill
    return int(r) << 16 | int(g) << 8 | int(b)


def apply_op(img, name, m, interpolation="nearest", fill=0):
    """torchvision.transforms.autoaugment._apply_op on a PIL image, on uint8 [H, W, 3]."""
    h, w, _ = img.shape
    filt, fc = A.FILTERS[interpolation], fill_code(fill)
    if name == "Identity":
        return img.copy()
    if name == "ShearX":
        return A.transform(img, A.affine_matrix(0.0, (0, 0), 1.0, (math.degrees(math.atan(m)), 0.0), w, h, (0, 0)), filt, fc)
    if name == "ShearY":
        return A.transform(img, A.affine_matrix(0.0, (0, 0), 1.0, (0.0, math.degrees(math.atan(m))), w, h, (0, 0)), filt, fc)
    if name == "TranslateX":
        return A.transform(img, A.affine_matrix(0.0, (int(m), 0), 1.0, (0.0, 0.0), w, h), filt, fc)
    if name == "TranslateY":
        return A.transform(img, A.affine_matrix(0.0, (0, int(m)), 1.0, (0.0, 0.0), w, h), filt, fc)
    if name == "Rotate":
        return A.transform(img, A.rotation_matrix(m, w, h), filt, fc)
    if name == "Brightness":
        return C.brightness(img, 1.0 + m)
    if name == "Color":
        return C.saturation(img, 1.0 + m)
    if name == "Contrast":
        return C.contrast(img, 1.0 + m)
    if name == "Sharpness":
        return sharpness(img, 1.0 + m)
    if name == "Posterize":
        return posterize(img, int(m))
    if name == "Solarize":
        return solarize(img, m)
    if name == "AutoContrast":
        return autocontrast(img)
    assert name == "Equalize", name
    return equalize(img)


def apply_program(img, program, interpolation="nearest", fill=0):
    """One image through [(op name, magnitude)] in order."""
    out = np.ascontiguousarray(img).copy()
    for name, m in program:
        out = apply_op(out, name, m, interpolation, fill)
    return out
