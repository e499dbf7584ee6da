"""The colour augmentations of csrc/color.hip restated in numpy: PIL's ImageEnhance.Brightness / Contrast / Color,
the 8-bit HSV hue shift of torchvision's PIL path and convert("L"), on uint8 [H, W, 3] arrays.  Every float
operation is one IEEE operation in the named width (numpy never fuses a multiply and an add), so this file is the
arithmetic the kernels are held to bit for bit; tests/test_cpu_color.py pins it to PIL itself."""
import numpy as np

F32, F64 = np.float32, np.float64
BRIGHTNESS, CONTRAST, SATURATION, HUE = 1, 2, 3, 4
OPS = {"brightness": BRIGHTNESS, "contrast": CONTRAST, "saturation": SATURATION, "hue": HUE}


def luma(img):
    """convert("L") of uint8 [..., 3] -> uint8 [...]."""
    c = img.astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 32768) >> 16).astype(np.uint8)


def blend(d, x, a):
    """Image.blend(degenerate d, image x, factor a) per byte: two float32 roundings, truncation, and a clip only
    when a is outside [0, 1] (inside it the value cannot leave [0, 255])."""
    a = F32(a)
    diff = (np.asarray(x, np.int32) - np.asarray(d, np.int32)).astype(F32)
    t = np.asarray(d, np.int32).astype(F32) + (a * diff).astype(F32)
    t = t.astype(F32)
    if F32(0) <= a <= F32(1):
        return t.astype(np.int32).astype(np.uint8)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.int32)
    return out.astype(np.uint8)


def contrast_mean(img):
    """int(mean(L) + 0.5) as integers: floor((2 sum + n) / (2 n))."""
    L = luma(img)
    n = L.size
    return int((2 * int(L.sum(dtype=np.int64)) + n) // (2 * n))


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast(img, f):
    return blend(np.full_like(img, contrast_mean(img)), img, f)


def saturation(img, f):
    return blend(luma(img)[..., None], img, f)


def gray(img):
    return np.repeat(luma(img)[..., None], 3, axis=-1)


def rgb_to_hsv(img):
    """convert("HSV") of uint8 [..., 3]."""
    c = img.astype(np.int32)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    mx, mn = c.max(-1), c.min(-1)
    flat = mx == mn
    cr = np.where(flat, 1, mx - mn).astype(F32)
    mxf = np.where(flat, 1, mx).astype(F32)
    s = cr / mxf
    rc = (mx - r).astype(F32) / cr
    gc = (mx - g).astype(F32) / cr
    bc = (mx - b).astype(F32) / cr
    h_r = bc - gc
    h_g = ((F64(2.0) + rc.astype(F64)) - bc.astype(F64)).astype(F32)
    h_b = ((F64(4.0) + gc.astype(F64)) - rc.astype(F64)).astype(F32)
    h = np.where(r == mx, h_r, np.where(g == mx, h_g, h_b)).astype(F32)
    h = np.fmod(h.astype(F64) / F64(6.0) + F64(1.0), F64(1.0)).astype(F32)
    H = np.clip((h.astype(F64) * F64(255.0)).astype(np.int32), 0, 255)
    S = np.clip((s.astype(F64) * F64(255.0)).astype(np.int32), 0, 255)
    H, S = np.where(flat, 0, H), np.where(flat, 0, S)
    return np.stack([H, S, mx], -1).astype(np.uint8)


def _round_clip(v):
    """C round() (half away from zero) of a non-negative double, clipped to a byte."""
    fl = np.floor(v)
    return np.clip(np.where(v - fl >= 0.5, fl + 1.0, fl), 0, 255).astype(np.int32)


def hsv_to_rgb(hsv):
    """HSV -> convert("RGB") of uint8 [..., 3]."""
    c = hsv.astype(np.int32)
    H, S, V = c[..., 0], c[..., 1], c[..., 2]
    x = H.astype(F32).astype(F64) * F64(6.0) / F64(255.0)
    fi = np.floor(x)
    f = (x - fi).astype(F32).astype(F64)
    fs = (S.astype(F64) / F64(255.0)).astype(F32).astype(F64)
    v = V.astype(F64)
    p = _round_clip(v * (F64(1.0) - fs))
    q = _round_clip(v * (F64(1.0) - fs * f))
    t = _round_clip(v * (F64(1.0) - fs * (F64(1.0) - f)))
    i = fi.astype(np.int32) % 6
    R = np.choose(i, [V, q, p, p, t, V])
    G = np.choose(i, [t, V, V, q, p, p])
    B = np.choose(i, [p, p, t, V, V, q])
    out = np.stack([R, G, B], -1)
    out = np.where((S == 0)[..., None], V[..., None], out)
    return out.astype(np.uint8)


def hue(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + int(shift)) % 256).astype(np.uint8)
    return hsv_to_rgb(hsv)


_FN = {BRIGHTNESS: brightness, CONTRAST: contrast, SATURATION: saturation, HUE: hue}


def apply(img, ops, to_gray=False):
    """One image uint8 [H, W, 3] through `ops`, a list of (name or code, value) in order, then the grayscale."""
    out = np.ascontiguousarray(img)
    for op, val in ops:
        out = _FN[OPS.get(op, op)](out, val)
    return gray(out) if to_gray else out.copy()


def apply_item(img, item):
    """The same from a clipmi.images.ColorItem (or anything with its fields)."""
    vals = {BRIGHTNESS: item.brightness, CONTRAST: item.contrast, SATURATION: item.saturation, HUE: item.hue_shift}
    ops, order = [], int(item.order)
    while order & 15:
        ops.append((order & 15, vals[order & 15]))
        order >>= 4
    return apply(img, ops, bool(item.gray))
