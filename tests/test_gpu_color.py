"""Colour augmentation on the GPU (csrc/color.hip clipmi_color_u8, clipmi/images.py): every comparison is bit for bit
against tests/color_ref.py, which tests/test_cpu_color.py pins to PIL.  The images sit in a guard-banded buffer at a
1-byte offset, so image bases take every alignment and a store outside the batch is caught."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import color_ref as C  # noqa: E402
import test_cpu_color as cpu_cases  # noqa: E402
from kernel_checks import GUARD_PATTERN, guarded1d  # noqa: E402

from clipmi import CLIPAdapterTrainer, CLIPWithAdapters, _lib, synth  # noqa: E402
from clipmi import kernels as K  # noqa: E402
from clipmi.images import (MODES, ColorItem, ColorJitter, ImageBatch, TrainAugment, color_jitter_u8,  # noqa: E402
                           preprocess)

OPS = ("brightness", "contrast", "saturation", "hue")
IDENTITY = ColorItem.of([])


def run(imgs, items):
    """uint8 [B, H, W, 3] (numpy) through color_jitter_u8 inside guard bands at a 1-byte offset -> numpy."""
    B, H, W, _ = imgs.shape
    buf, chk = guarded1d(imgs.size, torch.uint8, offset_elems=1)
    buf.copy_(torch.from_numpy(np.ascontiguousarray(imgs)).reshape(-1))
    out = color_jitter_u8(buf.view(B, H, W, 3), items)
    torch.cuda.synchronize()
    chk()
    return out.cpu().numpy()


def expect(imgs, items):
    return np.stack([C.apply_item(im, it) for im, it in zip(imgs, items)])


def assert_same(got, ref, items):
    for b in range(len(ref)):
        assert np.array_equal(got[b], ref[b]), (b, items[b].ops(), items[b].gray, np.argwhere(got[b] != ref[b])[:4].tolist(),
                                                got[b][got[b] != ref[b]][:4].tolist(), ref[b][got[b] != ref[b]][:4].tolist())


def random_batch(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (31, 33), (32, 32)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("op", OPS + ("gray",))
def test_each_op_alone(op, hw):
    """Four values of one op and an identity item (in the middle, so both its neighbours store next to it) whose
    bytes must stay as they were.  The odd sizes put image bases at every alignment: head and tail pixels."""
    H, W = hw
    imgs = random_batch(5, H, W, seed=H * 100 + W)
    values = (0, 1, 128, 255) if op == "hue" else (0, 0.3, 1, 1.7)
    items = [ColorItem.of([], gray=1) if op == "gray" else ColorItem.of([(op, v)]) for v in values]
    items.insert(2, IDENTITY)
    got = run(imgs, items)
    assert np.array_equal(got[2], imgs[2]), "the identity item's image changed"
    assert_same(got, expect(imgs, items), items)


def test_all_24_orders():
    """Every order of the four ops, one image each: the contrast in every position, so pass 1 replays zero to three
    ops in front of it; every image with its own factors."""
    orders = list(itertools.permutations(OPS))
    imgs = random_batch(24, 31, 33, seed=24)
    rng = np.random.default_rng(1)
    items = []
    for order in orders:
        vals = {"brightness": rng.uniform(0.5, 1.6), "contrast": rng.uniform(0.4, 1.8), "saturation": rng.uniform(0, 2.2),
                "hue": int(rng.integers(0, 256))}
        items.append(ColorItem.of([(n, vals[n]) for n in order], gray=len(items) % 5 == 4))
    assert_same(run(imgs, items), expect(imgs, items), items)


def test_mixed_batch_and_constant_images():
    """Images with and without a contrast side by side (pass 1 skips the latter), partial lists, and constant images:
    a luma mean exactly at x.5 (half the pixels at gray x, half at x + 1; int(mean + 0.5) rounds up) and mx == mn
    through the hue op (H = S = 0)."""
    H, W = 6, 7
    imgs = random_batch(10, H, W, seed=5)
    half = np.full((H, W, 3), 100, np.uint8)
    half[:3] = 101
    imgs[1] = half
    imgs[4] = 255 - half
    imgs[6] = 77
    imgs[7] = 0
    imgs[8] = 255
    assert C.contrast_mean(imgs[1]) == 101 and int(C.luma(imgs[1]).sum()) * 2 == 201 * H * W
    items = [ColorItem.of([("brightness", 1.2)]),
             ColorItem.of([("contrast", 1.5)]),
             ColorItem.of([("hue", 40), ("saturation", 0.5)]),
             ColorItem.of([("saturation", 1.9), ("contrast", 0.25)], gray=1),
             ColorItem.of([("contrast", 3.0), ("hue", 0)]),
             IDENTITY,
             ColorItem.of([("hue", 99), ("contrast", 0.5)]),
             ColorItem.of([("contrast", 2.0), ("brightness", 3.0)]),
             ColorItem.of([("brightness", 0.999), ("contrast", 1.001), ("hue", 255)]),
             ColorItem.of([], gray=1)]
    got = run(imgs, items)
    assert np.array_equal(got[5], imgs[5])
    assert_same(got, expect(imgs, items), items)


@functools.lru_cache(maxsize=None)
def all_colours_hue_85():
    ref = C.hue(cpu_cases.all_colours(), 85)
    ref.setflags(write=False)
    return ref


def test_hue_on_all_colours():
    """Every 24-bit colour through RGB -> HSV -> +85 -> RGB in one 4096 x 4096 image (H * W = 2^24, the largest the
    call takes): the float / double mix can only go wrong at particular colours."""
    rgb = cpu_cases.all_colours()
    x = torch.from_numpy(rgb.copy())[None].cuda()
    color_jitter_u8(x, [ColorItem.of([("hue", 85)])])
    got = x[0].cpu().numpy()
    ref = all_colours_hue_85()
    bad = (got != ref).any(-1)
    assert not bad.any(), (int(bad.sum()), rgb[bad][:4].tolist(), got[bad][:4].tolist(), ref[bad][:4].tolist())


def test_full_size_sum_range_stride_and_reproducible():
    """S = 224, B = 3: threads stride over more than one group, a near-white image drives the luma sum to 1.2e7
    (24 bits), and the call twice from the same input gives the same bytes."""
    imgs = random_batch(3, 224, 224, seed=224)
    imgs[1] = 255 - imgs[1] // 16
    items = [ColorItem.of([("brightness", 1.1), ("contrast", 1.4), ("saturation", 0.7), ("hue", 13)]),
             ColorItem.of([("contrast", 0.6), ("hue", 200)]),
             ColorItem.of([("saturation", 1.5), ("hue", 128), ("contrast", 1.9)], gray=1)]
    assert int(C.luma(imgs[1]).sum()) > 1 << 23
    got = run(imgs, items)
    assert_same(got, expect(imgs, items), items)
    assert np.array_equal(run(imgs, items), got)


def test_invalid_items_raise_before_launch():
    x = torch.zeros(2, 4, 4, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="item 1"):
        color_jitter_u8(x, [IDENTITY, ColorItem(1.0, float("nan"), 1.0, 0, 2, 0)])
    with pytest.raises(ValueError, match="records"):
        color_jitter_u8(x, [IDENTITY])
    with pytest.raises(ValueError, match="GPU"):
        color_jitter_u8(x.cpu(), [IDENTITY, IDENTITY])
    with pytest.raises(ValueError, match="uint8"):
        color_jitter_u8(x.float(), [IDENTITY, IDENTITY])
    assert color_jitter_u8(x[:0], []).shape == (0, 4, 4, 3)
    assert int(x.sum()) == 0


# ------------------------------------------------------------------------------------------------ preprocess
def ragged_images(seed=9):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(70, 64), (65, 200), (130, 90), (64, 64), (33, 47)]]


def parent_preprocess(batch, S, mode):
    """clipmi_resize_crop_u8 called as preprocess called it before it knew of colour."""
    L = _lib.lib()
    items = batch.items()
    B = len(batch)
    nb = int(L.clipmi_resize_crop_u8_ws(items, B, S, MODES[mode]))
    out = torch.full((B, S, S, 3), GUARD_PATTERN, dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    _lib.check(L.clipmi_resize_crop_u8(K.stream(), K.ptr(batch.data), batch.data.numel(), items, B, K.ptr(out), S,
                                       MODES[mode], K.ptr(ws), nb), "clipmi_resize_crop_u8")
    return out


@pytest.mark.parametrize("mode", ["processor", "square"])
def test_preprocess_with_and_without_colour(mode):
    S = 48
    batch = ImageBatch.pack(ragged_images()).with_flips([0, 1, 0, 1, 1]).with_mode(mode).to("cuda")
    plain = preprocess(batch, S)
    assert torch.equal(plain, parent_preprocess(batch, S, mode)), "color=None no longer gives the parent's bytes"
    items = ColorJitter(0.4, 0.4, 0.4, 0.1, 0.3).sample(len(batch), torch.Generator().manual_seed(3))
    assert any(dict(it.ops()).get("contrast") is not None for it in items)
    fused = preprocess(batch.with_color(items), S)
    assert not torch.equal(fused, plain)
    assert torch.equal(fused, color_jitter_u8(plain.clone(), items))
    assert np.array_equal(fused.cpu().numpy(), expect(plain.cpu().numpy(), items))
    into = torch.empty(len(batch) * S * S * 3, dtype=torch.uint8, device="cuda")
    assert torch.equal(preprocess(batch.with_color(items), S, out=into), fused)


# ------------------------------------------------------------------------------------------------ trainer
def train_losses(augment, tmp, steps=2):
    torch.manual_seed(0)
    m = CLIPWithAdapters("tiny", use_text_adapter=True, use_vision_adapter=True, use_shared_adapters=False,
                         freeze_clip=True, device="cuda", precision="bf16")
    images = ragged_images()[:4]
    b = synth.synthetic_batch(m.config, len(images), seed=21)
    batch = {k: torch.from_numpy(b[k]) for k in ("input_ids", "attention_mask")}
    batch["pixel_values"] = ImageBatch.pack(images)
    tr = CLIPAdapterTrainer(m, [batch], learning_rate=1e-3, output_dir=str(tmp), augment=augment)
    return [tr.train_step(batch, i, steps) for i in range(steps)]


def test_trainer_colour_augment_reproducible(tmp_path):
    jitter = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, grayscale_p=0.2)
    a = train_losses(TrainAugment(seed=3, color=ColorJitter(**jitter)), tmp_path)
    b = train_losses(TrainAugment(seed=3, color=ColorJitter(**jitter)), tmp_path)
    plain = train_losses(TrainAugment(seed=3), tmp_path)
    assert all(bool(torch.isfinite(x)) for x in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), (a, b)
    assert not torch.equal(a[0], plain[0]), "the colour records did not reach the images"
