"""Ragged image batches without a GPU: the semantics the kernels are held to (crop, then PIL bicubic), the
random-resized-crop sampler, ImageBatch.pack, and clipmi_resize_crop_u8's host-side validation through the C ABI
(it rejects before any launch: pointers are never dereferenced)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import resize_ref as RR

# (h, w, box (x0, y0, cw, ch) or None): one batch, in this order (tests/test_gpu_ragged_input.py runs it on the GPU)
SHAPES = [(1, 1, None), (1, 7, None), (7, 1, None), (5, 3, None), (100, 100, None), (37, 91, None),
          (91, 37, (3, 5, 30, 80)), (300, 451, None), (451, 300, (10, 20, 280, 400)), (64, 64, (63, 63, 1, 1)),
          (33, 47, (0, 0, 47, 33)), (640, 48, None), (48, 640, (100, 0, 500, 48)), (2300, 31, None)]


def images(seed=7):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w, _ in SHAPES]


def boxes():
    return [b if b is not None else (0, 0, w, h) for h, w, b in SHAPES]


def accepted(S, mode):
    """Indices of the list's items the library takes.  All of them, except that squaring the 2300 x 31 image to
    S = 32 is a 72x downscale, above the 32x cap: the library must reject that item (asserted below and on the
    GPU), so the S = 32 square batch is the list without it."""
    return [i for i, ((h, w, _), (x0, y0, cw, ch)) in enumerate(zip(SHAPES, boxes()))
            if mode == "processor" or max(cw, ch) <= 32 * S]


def out_size(ch, cw, S, mode):
    return RR.shortest_edge_size(ch, cw, S) if mode == "processor" else (S, S)


@pytest.mark.parametrize("S", [32, 224])
def test_crop_then_resize_oracle_matches_pil(S):
    """The reference semantics: resize_bicubic on the array slice == PIL's resize of the cropped image, for every
    shape of the list in both modes (the window and the flip are plain indexing after it)."""
    Image = pytest.importorskip("PIL.Image")
    for img, (x0, y0, cw, ch) in zip(images(), boxes()):
        crop = np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw])
        for mode in ("processor", "square"):
            oh, ow = out_size(ch, cw, S, mode)
            ref = np.asarray(Image.fromarray(crop).resize((ow, oh), Image.BICUBIC))
            assert np.array_equal(RR.resize_bicubic(crop, oh, ow), ref), (img.shape, mode)


# ---------------------------------------------------------------------------------------------- sampler
def test_sampler_boxes_inside_and_in_range():
    from clipmi.images import fallback_box, random_resized_crop_boxes
    g = torch.Generator().manual_seed(0)
    sizes = [(int(h), int(w)) for h, w in torch.randint(20, 600, (200, 2), generator=g).tolist()]
    scale, ratio = (0.08, 1.0), (3 / 4, 4 / 3)
    bx = random_resized_crop_boxes(sizes, scale, ratio, torch.Generator().manual_seed(1))
    assert len(bx) == len(sizes)
    sampled = 0
    for (h, w), (x0, y0, cw, ch) in zip(sizes, bx):
        assert cw >= 1 and ch >= 1 and 0 <= x0 <= w - cw and 0 <= y0 <= h - ch
        if (x0, y0, cw, ch) == fallback_box(h, w, ratio):
            continue
        sampled += 1
        # cw = round(sqrt(A r)), ch = round(sqrt(A / r)) with A in scale * h * w, r in ratio: each side is within
        # 0.5 of its real value
        lo_a, hi_a = (cw - 0.5) * (ch - 0.5), (cw + 0.5) * (ch + 0.5)
        assert hi_a >= scale[0] * h * w and lo_a <= scale[1] * h * w
        assert (cw + 0.5) / (ch - 0.5) >= ratio[0] and (cw - 0.5) / (ch + 0.5) <= ratio[1]
    assert sampled > 150


def test_sampler_fallback_seed_and_identity():
    from clipmi.images import random_resized_crop_boxes
    # 10 wide, 1000 tall: every try is wider than the image; the centre crop at the nearest allowed ratio (3/4)
    assert random_resized_crop_boxes([(1000, 10)], generator=torch.Generator().manual_seed(5)) == [(0, 493, 10, 13)]
    assert random_resized_crop_boxes([(10, 1000)], generator=torch.Generator().manual_seed(5)) == [(493, 0, 13, 10)]
    sizes = [(200, 300)] * 8
    a = random_resized_crop_boxes(sizes, generator=torch.Generator().manual_seed(3))
    b = random_resized_crop_boxes(sizes, generator=torch.Generator().manual_seed(3))
    c = random_resized_crop_boxes(sizes, generator=torch.Generator().manual_seed(4))
    assert a == b and a != c
    whole = random_resized_crop_boxes([(64, 64), (7, 7)], (1, 1), (1, 1), torch.Generator().manual_seed(0))
    assert whole == [(0, 0, 64, 64), (0, 0, 7, 7)]


def test_flips_and_train_augment_reproducible():
    from clipmi.images import ImageBatch, TrainAugment, random_flips
    assert random_flips(5, 0.0, torch.Generator().manual_seed(0)) == [0] * 5
    assert random_flips(5, 1.0, torch.Generator().manual_seed(0)) == [1] * 5
    batch = ImageBatch.pack(images()[3:7])
    a, b = TrainAugment(seed=3), TrainAugment(seed=3)
    for _ in range(2):
        x, y = a(batch), b(batch)
        assert x.boxes == y.boxes and x.flips == y.flips and x.mode == "square"
    assert batch.mode == "processor" and batch.flips == [0] * 4  # the input batch is left as it was


# ---------------------------------------------------------------------------------------------- ImageBatch
def test_pack_offsets_and_rejections():
    from clipmi.images import ImageBatch, collate
    imgs = images()
    batch = ImageBatch.pack([imgs[0], torch.from_numpy(imgs[1])] + imgs[2:])
    assert len(batch) == len(SHAPES) and batch.sizes == [(h, w) for h, w, _ in SHAPES]
    assert batch.offsets == [int(v) for v in np.cumsum([0] + [h * w * 3 for h, w, _ in SHAPES])[:-1]]
    assert batch.data.numel() == sum(h * w * 3 for h, w, _ in SHAPES)
    for im, o in zip(imgs, batch.offsets):
        assert np.array_equal(batch.data[o:o + im.size].numpy().reshape(im.shape), im)
    assert batch.boxes == [(0, 0, w, h) for h, w, _ in SHAPES] and batch.flips == [0] * len(SHAPES)
    moved = batch.with_boxes(boxes()).with_flips([1] * len(SHAPES))
    assert moved.boxes == boxes() and batch.boxes != moved.boxes and moved.data is batch.data
    with pytest.raises(ValueError, match="uint8"):
        ImageBatch.pack([imgs[0].astype(np.float32)])
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((3, 4, 4), np.uint8)):
        with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
            ImageBatch.pack([bad])
    out = collate([{"image": imgs[3], "input_ids": torch.arange(4)}, {"image": imgs[5], "input_ids": torch.arange(4)}])
    assert isinstance(out["pixel_values"], ImageBatch) and len(out["pixel_values"]) == 2
    assert out["input_ids"].shape == (2, 4)
    from torch.utils.data import DataLoader
    data = [{"image": im, "label": torch.tensor(i)} for i, im in enumerate(imgs[:5])]
    got = list(DataLoader(data, batch_size=2, collate_fn=collate))
    assert [len(b["pixel_values"]) for b in got] == [2, 2, 1] and got[1]["label"].tolist() == [2, 3]
    assert got[1]["pixel_values"].sizes == [(7, 1), (5, 3)]


# ---------------------------------------------------------------------------------------------- C ABI validation
def _call(items, S=224, mode=0, packed_bytes=None, ws_bytes=1 << 40, B=None):
    """clipmi_resize_crop_u8 with fake device pointers (validation rejects before any launch) -> (status, message)."""
    from clipmi import _lib
    from clipmi.images import ImageItem
    L = _lib.lib()
    arr = (ImageItem * max(len(items), 1))(*[ImageItem(*it) for it in items])
    if packed_bytes is None:
        packed_bytes = max([it[0] + it[1] * it[2] * 3 for it in items], default=0)
    st = L.clipmi_resize_crop_u8(None, 4096, packed_bytes, arr, len(items) if B is None else B, 8192, S, mode, 12288,
                                 ws_bytes)
    return st, L.clipmi_last_error().decode()


def _ws(items, S=224, mode=0):
    from clipmi import _lib
    from clipmi.images import ImageItem
    arr = (ImageItem * max(len(items), 1))(*[ImageItem(*it) for it in items])
    return int(_lib.lib().clipmi_resize_crop_u8_ws(arr, len(items), S, mode))


GOOD = (0, 100, 120, 0, 0, 120, 100, 0)  # offset, h, w, x0, y0, cw, ch, flip


def _item(**kw):
    d = dict(zip(("offset", "h", "w", "x0", "y0", "cw", "ch", "flip"), GOOD))
    d.update(kw)
    return tuple(d[k] for k in ("offset", "h", "w", "x0", "y0", "cw", "ch", "flip"))


@pytest.mark.parametrize("bad", [dict(x0=1), dict(y0=50, ch=51), dict(cw=0), dict(ch=0), dict(x0=-1, cw=10),
                                 dict(flip=2), dict(flip=-1), dict(h=0, ch=0), dict(offset=-3)])
def test_bad_item_is_rejected_with_its_index(bad):
    from clipmi import _lib
    second = (100 * 120 * 3,) + _item(**bad)[1:] if "offset" not in bad else _item(**bad)
    st, msg = _call([GOOD, second], packed_bytes=1 << 30)
    assert st == -1 and "item 1" in msg, msg
    with pytest.raises(ValueError):
        _lib.check(st, "clipmi_resize_crop_u8")
    if "offset" not in bad:  # the same table with the good item alone passes validation and fails on the workspace
        st, msg = _call([GOOD], ws_bytes=0)
        assert st == -1 and "workspace" in msg


def test_image_past_the_packed_buffer_is_rejected():
    st, msg = _call([GOOD, (36000, 100, 120, 0, 0, 120, 100, 0)], packed_bytes=72000 - 1)
    assert st == -1 and "item 1" in msg and "packed" in msg
    st, msg = _call([GOOD, (36000, 100, 120, 0, 0, 120, 100, 0)], packed_bytes=72000, ws_bytes=0)
    assert st == -1 and "workspace" in msg  # the buffer's exact size passes the items


def test_mode_size_and_workspace():
    assert _call([GOOD], mode=2)[0] == -1 and "mode" in _call([GOOD], mode=2)[1]
    assert _call([GOOD], mode=-1)[0] == -1
    assert _call([GOOD], S=0)[0] == -1
    assert _ws([GOOD], mode=3) == -1 and _ws([GOOD], S=0) == -1
    for mode in (0, 1):
        need = _ws([GOOD], mode=mode)
        assert need > 0
        st, msg = _call([GOOD], mode=mode, ws_bytes=need - 1)
        assert st == -1 and "workspace" in msg
    assert _call([], B=0)[0] == 0 and _ws([]) == 0


@pytest.mark.parametrize("mode", [0, 1])
def test_downscale_cap(mode):
    """32x per axis (129 taps) is accepted by the workspace query, 33x on either axis is not."""
    S = 8
    ok = (0, 32 * S, 32 * S, 0, 0, 32 * S, 32 * S, 0)
    assert _ws([ok], S, mode) > 0
    wide = (0, 32 * S, 33 * S, 0, 0, 33 * S, 32 * S, 0)
    tall = (0, 33 * S, 32 * S, 0, 0, 32 * S, 33 * S, 0)
    both = (0, 33 * S, 33 * S, 0, 0, 33 * S, 33 * S, 0)
    from clipmi import _lib
    # mode 0: the 32x short edge gives the long edge int(S * 33 / 32) = S output pixels for 33 S input ones
    for it in (wide, tall, both):
        assert _ws([ok, it], S, mode) == -1
        msg = _lib.lib().clipmi_last_error().decode()
        assert "item 1" in msg and "32x" in msg, msg
    # a 33x image with a 32x crop box is fine: the cap is on the crop
    assert _ws([(0, 33 * S, 33 * S, 3, 5, 32 * S, 32 * S, 1)], S, mode) > 0


@pytest.mark.parametrize("mode", ["processor", "square"])
@pytest.mark.parametrize("S", [32, 224])
def test_workspace_is_the_plan_of_the_oracles_tap_ranges(S, mode):
    """clipmi_resize_crop_u8_ws = 64-byte records + two coefficient tables at the batch's largest tap counts + an
    intermediate that holds, per image, only the crop rows the S output rows' vertical taps reach (each part padded
    to 256 bytes, each image's rows to 16): the host's row ranges are the oracle's."""
    def al(x, a=256):
        return (x + a - 1) // a * a
    keep = accepted(S, mode)
    assert keep == list(range(len(SHAPES))) or (S, mode, keep) == (32, "square", list(range(len(SHAPES) - 1)))
    B = len(keep)
    kw = kh = 1
    tmp = 0
    rows_2300 = None
    for (h, w, _), (x0, y0, cw, ch) in [(SHAPES[i], boxes()[i]) for i in keep]:
        oh, ow = out_size(ch, cw, S, mode)
        top = (oh - S) // 2
        if cw != ow:
            kw = max(kw, RR.coeffs(cw, ow)[2].shape[1])
        if ch != oh:
            lo, cnt, k = RR.coeffs(ch, oh)
            kh = max(kh, k.shape[1])
            nr = int(lo[top + S - 1] + cnt[top + S - 1] - lo[top])
        else:
            nr = S
        if h == 2300:
            rows_2300 = nr
        tmp += al(nr * S * 3, 16)
    items = [(o, h, w) + b + (0,) for o, (h, w, _), b in zip(np.cumsum([0] + [h * w * 3 for h, w, _ in SHAPES]).tolist(),
                                                              SHAPES, boxes())]
    if len(keep) < len(SHAPES):  # the 72x item is refused by name
        from clipmi import _lib
        assert _ws(items, S, MODES[mode]) == -1
        assert "item 13" in _lib.lib().clipmi_last_error().decode()
    assert _ws([items[i] for i in keep], S, MODES[mode]) == al(B * 64) + al(B * S * (2 + kw) * 4) + al(B * S * (2 + kh) * 4) + al(tmp)
    if mode == "processor":
        assert rows_2300 < 2300 // 8  # the centre window of a 2300 x 31 image needs a fraction of its rows


MODES = {"processor": 0, "square": 1}


def test_item_struct_matches_the_header():
    from clipmi.images import ImageItem
    assert ctypes.sizeof(ImageItem) == 40 and ImageItem.h.offset == 8 and ImageItem.flip.offset == 32
