"""The arithmetic csrc/affine.hip is held to, restated in numpy: PIL's Image.transform(size, AFFINE, m, NEAREST |
BILINEAR, fillcolor=...) on RGB images, and the two matrix builders of clipmi/images.py.  Every double operation is
one numpy operation (numpy never fuses a multiply with an add), in PIL's order.  tests/test_cpu_affine.py pins this
file to PIL itself; tests/test_gpu_affine.py holds the kernel to it bit for bit.

The three sampling paths (PIL Geometry.c):
  bilinear          ImagingGenericTransform + affine_transform + bilinear_filter32RGB: doubles per pixel
  nearest, general  affine_fixed: 16.16 fixed point, 32-bit integers
  nearest, aligned  ImagingScaleAffine (a1 == 0 and a3 == 0): a column and a row table from running double sums"""
import math

import numpy as np

NEAREST, BILINEAR = 0, 1
FILTERS = {"nearest": NEAREST, "bilinear": BILINEAR}


def fill_rgb(fill):
    """0xRRGGBB -> uint8 [3]."""
    return np.array([(fill >> 16) & 255, (fill >> 8) & 255, fill & 255], np.uint8)


def fix(v):
    """PIL's FIX: floor(v * 65536.0 + 0.5) as an integer."""
    return int(math.floor(np.float64(v) * np.float64(65536.0) + np.float64(0.5)))


def bilinear(img, m):
    """-> (uint8 [H, W, 3], inside [H, W])."""
    H, W, _ = img.shape
    a = [np.float64(v) for v in m]
    xin = np.arange(W, dtype=np.float64)[None, :] + 0.5
    yin = np.arange(H, dtype=np.float64)[:, None] + 0.5
    xo = (a[0] * xin + a[1] * yin) + a[2]
    yo = (a[3] * xin + a[4] * yin) + a[5]
    inside = ~((xo < 0) | (xo >= W) | (yo < 0) | (yo >= H))
    xo = np.where(inside, xo, 0.5) - 0.5
    yo = np.where(inside, yo, 0.5) - 0.5
    xf, yf = np.floor(xo), np.floor(yo)
    dx, dy = (xo - xf)[..., None], (yo - yf)[..., None]
    xi, yi = xf.astype(np.int64), yf.astype(np.int64)
    x0, x1 = np.clip(xi, 0, W - 1), np.clip(xi + 1, 0, W - 1)
    row = np.clip(yi, 0, H - 1)
    p = img.astype(np.int64)
    v1 = p[row, x0].astype(np.float64) + (p[row, x1] - p[row, x0]).astype(np.float64) * dx
    has2 = ((yi + 1 >= 0) & (yi + 1 < H))[..., None]
    row2 = np.clip(yi + 1, 0, H - 1)
    v2 = p[row2, x0].astype(np.float64) + (p[row2, x1] - p[row2, x0]).astype(np.float64) * dx
    v2 = np.where(has2, v2, v1)
    v = v1 + (v2 - v1) * dy
    return np.trunc(v).astype(np.uint8), inside


def nearest_fixed(img, m):
    H, W, _ = img.shape
    a = [np.float64(v) for v in m]
    A0, A1, A3, A4 = fix(a[0]), fix(a[1]), fix(a[3]), fix(a[4])
    A2 = fix((a[2] + a[0] * 0.5) + a[1] * 0.5)
    A5 = fix((a[5] + a[3] * 0.5) + a[4] * 0.5)
    x = np.arange(W, dtype=np.int64)[None, :]
    y = np.arange(H, dtype=np.int64)[:, None]
    sx = (A2 + A0 * x + A1 * y) >> 16
    sy = (A5 + A3 * x + A4 * y) >> 16
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    return img[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], inside


def scale_table(c, a, n):
    """ImagingScaleAffine's table: o = c + a * 0.5; n times: entry = -1 if o < 0 else int(o); o += a."""
    c, a = np.float64(c), np.float64(a)
    o = c + a * 0.5
    tab = np.empty(n, np.int64)
    for i in range(n):
        tab[i] = -1 if o < 0 else int(o)
        o = o + a
    return tab


def nearest_scale(img, m):
    H, W, _ = img.shape
    xt, yt = scale_table(m[2], m[0], W), scale_table(m[5], m[4], H)
    sx, sy = np.broadcast_to(xt[None, :], (H, W)), np.broadcast_to(yt[:, None], (H, W))
    inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    return img[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)], inside


def path_of(m, filt):
    if filt == BILINEAR:
        return "bilinear"
    return "scale" if m[1] == 0 and m[3] == 0 else "fixed"


def transform(img, m, filt=NEAREST, fill=0):
    """uint8 [H, W, 3] through Image.transform(size, AFFINE, m, filt, fillcolor=fill)."""
    img = np.asarray(img)
    out, inside = {"bilinear": bilinear, "scale": nearest_scale, "fixed": nearest_fixed}[path_of(m, filt)](img, m)
    return np.where(inside[..., None], out, fill_rgb(fill)[None, None, :]).astype(np.uint8)


def apply_item(img, item):
    """One clipmi.images.AffineItem on one image."""
    return transform(img, list(item.m), item.filter, item.fill)


# ------------------------------------------------------------------------------------------------ matrix builders
def rotation_matrix(angle, w, h, center=None):
    """PIL Image.rotate's matrix (PIL/Image.py), without its transpose shortcuts."""
    angle = angle % 360.0
    cx, cy = (w / 2.0, h / 2.0) if center is None else center
    t = -math.radians(angle)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]

    def tr(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]

    m[2], m[5] = tr(-cx, -cy)
    m[2] += cx
    m[5] += cy
    return m


def affine_matrix(angle=0.0, translate=(0, 0), scale=1.0, shear=(0.0, 0.0), w=1, h=1, center=None):
    """torchvision's _get_inverse_affine_matrix as F.affine calls it for PIL images."""
    cx, cy = (w * 0.5, h * 0.5) if center is None else center
    tx, ty = translate
    rot, sx, sy = math.radians(angle), math.radians(shear[0]), math.radians(shear[1])
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [v / scale for v in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m
