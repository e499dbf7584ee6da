"""Colour augmentation without a GPU: tests/color_ref.py (the arithmetic csrc/color.hip is held to, bit for bit, in
tests/test_gpu_color.py) pinned to PIL itself, exhaustively for the blend and both HSV transforms; the ColorJitter
sampler; TrainAugment's draw order; clipmi_color_u8's host-side validation through the C ABI (it rejects before any
launch: pointers are never dereferenced); the struct layout."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import color_ref as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXED_FACTORS = [0, 0.1, 1 / 3, 0.9, 1, 1.0000001, 3]


def pil():
    Image = pytest.importorskip("PIL.Image")
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    return Image, ImageEnhance


def random_image(h=37, w=53, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def all_colours():
    """Every 24-bit triple once, as a 4096 x 4096 x 3 image (read-only; tests/test_gpu_color.py shares it)."""
    a = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([a >> 16, (a >> 8) & 255, a & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    img.setflags(write=False)
    return img


# ------------------------------------------------------------------------------------------------ restatement vs PIL
def test_blend_matches_pil_on_every_byte_pair():
    Image, _ = pil()
    d, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    pd, px = Image.fromarray(d), Image.fromarray(x)
    factors = FIXED_FACTORS + np.random.default_rng(0).uniform(0, 3, 40).tolist()
    for f in factors:
        ref = np.asarray(Image.blend(pd, px, f))
        got = C.blend(d, x, f)
        assert np.array_equal(got, ref), (f, np.argwhere(got != ref)[:4].tolist())


def test_blend_in_double_would_differ():
    """The tests discriminate: forming the blend in double (or with one rounding) changes bytes."""
    d, x = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for f in (0.1, 0.9, 1 / 3):
        wide = np.trunc(d + float(np.float32(f)) * (x - d)).astype(np.uint8)
        assert int((wide != C.blend(d, x, f)).sum()) > 100


def test_enhancers_and_luma_match_pil():
    Image, ImageEnhance = pil()
    img = random_image()
    p = Image.fromarray(img)
    assert np.array_equal(C.luma(img), np.asarray(p.convert("L")))
    assert np.array_equal(C.gray(img), np.asarray(p.convert("L").convert("RGB")))
    for f in FIXED_FACTORS + [0.3, 1.7]:
        assert np.array_equal(C.brightness(img, f), np.asarray(ImageEnhance.Brightness(p).enhance(f))), f
        assert np.array_equal(C.contrast(img, f), np.asarray(ImageEnhance.Contrast(p).enhance(f))), f
        assert np.array_equal(C.saturation(img, f), np.asarray(ImageEnhance.Color(p).enhance(f))), f


def test_rgb_to_hsv_matches_pil_on_all_colours():
    Image, _ = pil()
    rgb = all_colours()
    ref = np.asarray(Image.fromarray(rgb).convert("HSV"))
    bad = (C.rgb_to_hsv(rgb) != ref).any(-1)
    assert not bad.any(), (int(bad.sum()), rgb[bad][:4].tolist())


def test_hsv_to_rgb_matches_pil_on_all_colours():
    Image, _ = pil()
    hsv = all_colours()
    planes = [Image.fromarray(np.ascontiguousarray(hsv[..., k])) for k in range(3)]
    ref = np.asarray(Image.merge("HSV", planes).convert("RGB"))
    bad = (C.hsv_to_rgb(hsv) != ref).any(-1)
    assert not bad.any(), (int(bad.sum()), hsv[bad][:4].tolist())


def pil_hue(Image, p, shift):
    """torchvision's adjust_hue on a PIL image, with the byte already formed."""
    h, s, v = p.convert("HSV").split()
    nh = np.array(h, dtype=np.uint8)
    nh = (nh.astype(np.int32) + shift).astype(np.uint8)  # wraps, as the uint8 addition does
    return Image.merge("HSV", (Image.fromarray(nh), s, v)).convert("RGB")


@pytest.mark.parametrize("order", [("brightness", "contrast", "saturation", "hue"),
                                   ("hue", "saturation", "contrast", "brightness")])
def test_chain_matches_pil_chain(order):
    Image, ImageEnhance = pil()
    img = random_image(seed=4)
    vals = {"brightness": 1.3, "contrast": 0.6, "saturation": 1.8, "hue": 200}
    p = Image.fromarray(img)
    for name in order:
        if name == "hue":
            p = pil_hue(Image, p, vals[name])
        else:
            cls = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast,
                   "saturation": ImageEnhance.Color}[name]
            p = cls(p).enhance(vals[name])
    got = C.apply(img, [(n, vals[n]) for n in order])
    assert np.array_equal(got, np.asarray(p))
    assert np.array_equal(C.apply(img, [(n, vals[n]) for n in order], True), np.asarray(p.convert("L").convert("RGB")))
    assert np.array_equal(C.hue(img, 0), np.asarray(pil_hue(Image, Image.fromarray(img), 0)))
    assert not np.array_equal(C.hue(img, 0), img)  # PIL's HSV round trip is not the identity


def test_contrast_mean_rounds_half_up_like_pil():
    """Images whose luma mean is exactly x.5: half the pixels at gray level x, half at x + 1."""
    Image, _ = pil()
    ImageStat = pytest.importorskip("PIL.ImageStat")
    for x in (0, 1, 100, 127, 254):
        img = np.full((4, 6, 3), x, np.uint8)
        img[:2] = x + 1
        mean = ImageStat.Stat(Image.fromarray(img).convert("L")).mean[0]
        assert mean == x + 0.5
        assert C.contrast_mean(img) == int(mean + 0.5) == x + 1


# ------------------------------------------------------------------------------------------------ sampler
def test_sampler_ranges_orders_and_seed():
    from clipmi.images import ColorJitter
    cj = ColorJitter(brightness=0.4, contrast=(0.5, 1.5), saturation=2.0, hue=0.1, grayscale_p=0.3)
    items = cj.sample(300, torch.Generator().manual_seed(0))
    assert len(items) == 300
    orders, grays = set(), 0
    for it in items:
        ops = dict(it.ops())
        assert sorted(ops) == ["brightness", "contrast", "hue", "saturation"]
        assert np.float32(0.6) <= it.brightness <= np.float32(1.4)
        assert 0.5 <= it.contrast <= 1.5 and 0.0 <= it.saturation <= 3.0
        assert it.hue_shift <= 25 or it.hue_shift >= 256 - 25
        assert it.gray in (0, 1)
        orders.add(tuple(n for n, _ in it.ops()))
        grays += it.gray
    assert len(orders) == 24 and 50 < grays < 130
    assert any(it.hue_shift > 128 for it in items) and any(0 < it.hue_shift < 128 for it in items)
    again = cj.sample(300, torch.Generator().manual_seed(0))
    other = cj.sample(300, torch.Generator().manual_seed(1))
    key = lambda its: [(i.brightness, i.contrast, i.saturation, i.hue_shift, i.order, i.gray) for i in its]  # noqa: E731
    assert key(items) == key(again) and key(items) != key(other)
    # factors are float32: what the kernel multiplies by is what the record says
    assert all(it.brightness == float(np.float32(it.brightness)) for it in items)


def test_sampler_leaves_disabled_ops_out():
    from clipmi.images import ColorJitter
    g = torch.Generator().manual_seed(2)
    for it in ColorJitter(contrast=0.5, hue=(-0.5, 0.5)).sample(50, g):
        assert sorted(n for n, _ in it.ops()) == ["contrast", "hue"] and it.gray == 0
    for it in ColorJitter(brightness=None, saturation=(1, 1), hue=0).sample(5, g):
        assert it.ops() == [] and it.order == 0 and it.gray == 0
    assert all(it.gray == 1 and it.order == 0 for it in ColorJitter(grayscale_p=1.0).sample(5, g))
    assert ColorJitter(brightness=0.2).sample(0, g) == []


def test_hue_factor_to_shift():
    from clipmi.images import hue_shift_of
    # int(f * 255) truncates toward zero, then wraps into a byte
    assert [hue_shift_of(f) for f in (0.0, 0.5, -0.5, 0.1, -0.1, -0.001, 0.0039, 0.004, -0.004)] == \
        [0, 127, 129, 25, 231, 0, 0, 1, 255]


@pytest.mark.parametrize("bad", [dict(brightness=-0.1), dict(contrast=(1.5, 0.5)), dict(saturation=(-0.1, 1)),
                                 dict(hue=0.6), dict(hue=(-0.6, 0.1)), dict(hue=-0.1), dict(brightness="x"),
                                 dict(contrast=(1, 2, 3)), dict(brightness=float("nan")), dict(grayscale_p=1.5)])
def test_sampler_rejects_bad_arguments(bad):
    from clipmi.images import ColorJitter
    with pytest.raises(ValueError):
        ColorJitter(**bad)


def test_train_augment_colour_keeps_boxes_and_flips():
    from clipmi.images import ColorJitter, ImageBatch, TrainAugment
    rng = np.random.default_rng(1)
    batch = ImageBatch.pack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(40, 50), (33, 21), (64, 64)]])
    plain, col = TrainAugment(seed=5), TrainAugment(seed=5, color=ColorJitter(0.4, 0.4, 0.4, 0.1, 0.2))
    a, b = plain(batch), col(batch)
    assert a.boxes == b.boxes and a.flips == b.flips and a.mode == b.mode == "square"
    assert a.color is None and len(b.color) == 3 and batch.color is None
    assert b.to("cpu").color is b.color or len(b.to("cpu").color) == 3  # _like carries the records
    # with color=None the generator is where it was before: the next draw equals a fresh TrainAugment's second one
    ref = TrainAugment(seed=5)
    ref(batch)
    assert plain(batch).boxes == ref(batch).boxes
    with pytest.raises(ValueError):
        TrainAugment(color="jitter")
    with pytest.raises(ValueError):
        batch.with_color(b.color[:2])


# ------------------------------------------------------------------------------------------------ C ABI validation
FIELDS = ("brightness", "contrast", "saturation", "hue_shift", "order", "gray")
GOOD = dict(brightness=1.2, contrast=0.8, saturation=1.1, hue_shift=7, order=0x4321, gray=0)


def _table(items):
    from clipmi.images import ColorItem
    return (ColorItem * max(len(items), 1))(*[ColorItem(*[dict(GOOD, **it)[k] for k in FIELDS]) for it in items])


def _call(items, H=8, W=8, ws_bytes=1 << 40, B=None):
    """clipmi_color_u8 with fake device pointers (validation rejects before any launch) -> (status, message)."""
    from clipmi import _lib
    L = _lib.lib()
    st = L.clipmi_color_u8(None, 4096, _table(items), len(items) if B is None else B, H, W, 8192, ws_bytes)
    return st, L.clipmi_last_error().decode()


def _ws(items, H=8, W=8):
    from clipmi import _lib
    L = _lib.lib()
    return int(L.clipmi_color_u8_ws(_table(items), len(items), H, W)), L.clipmi_last_error().decode()


def test_version():
    from clipmi import _lib
    assert _lib.lib().clipmi_version() >= 9  # 8: before clipmi_color_u8


@pytest.mark.parametrize("bad", [dict(brightness=float("nan")), dict(contrast=float("inf")), dict(saturation=-0.5),
                                 dict(brightness=-1e-30), dict(hue_shift=256), dict(hue_shift=-1),
                                 dict(order=0x5), dict(order=0x11), dict(order=0x2132), dict(order=0x0201),
                                 dict(order=0x1000), dict(order=0x14321), dict(order=-1), dict(gray=2),
                                 dict(gray=-1)])
def test_bad_item_is_rejected_with_its_index(bad):
    from clipmi import _lib
    st, msg = _call([{}, {}, bad])
    assert st == -1 and "item 2" in msg and "clipmi_color_u8" in msg, msg
    with pytest.raises(ValueError):
        _lib.check(st, "clipmi_color_u8")
    nb, msg = _ws([{}, bad])
    assert nb == -1 and "item 1" in msg, msg


def test_good_items_pass_validation_and_fail_on_the_workspace():
    for it in ({}, dict(order=0), dict(order=0x2), dict(order=0x34, gray=1), dict(brightness=0.0, hue_shift=255)):
        nb, _ = _ws([it, it])
        assert nb >= 2 * 24
        st, msg = _call([it, it], ws_bytes=nb - 1)
        assert st == -1 and "workspace" in msg, msg


def test_sizes_and_empty_batch():
    assert _ws([{}], 4096, 4096)[0] > 0
    nb, msg = _ws([{}], 4096, 4097)
    assert nb == -1 and "2^24" in msg
    st, msg = _call([{}], 4097, 4096)
    assert st == -1 and "2^24" in msg
    assert _call([{}], 0, 8)[0] == -1 and _call([{}], 8, -1)[0] == -1
    assert _call([{}], B=-1)[0] == -1
    assert _call([], B=0)[0] == 0 and _ws([])[0] == 0


def test_item_struct_matches_the_header():
    from clipmi.images import COLOR_OPS, ColorItem
    assert ctypes.sizeof(ColorItem) == 24
    with open(os.path.join(REPO, "include", "clipmi.h")) as f:
        body = re.search(r"typedef struct clipmi_color_item \{(.*?)\} clipmi_color_item;", f.read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"float": ctypes.c_float, "int32_t": ctypes.c_int32}
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            t, names = decl.split(None, 1)
            fields += [(n.strip(), ctype[t]) for n in names.split(",")]
    assert fields == list(ColorItem._fields_)
    assert [getattr(ColorItem, n).offset for n, _ in fields] == [0, 4, 8, 12, 16, 20]
    assert COLOR_OPS == {"brightness": 1, "contrast": 2, "saturation": 3, "hue": 4} == C.OPS
    it = ColorItem.of([("hue", 9), ("brightness", 0.5)], gray=1)
    assert (it.order, it.hue_shift, it.brightness, it.contrast, it.gray) == (0x14, 9, 0.5, 1.0, 1)
    assert it.ops() == [("hue", 9), ("brightness", 0.5)]
