"""Affine / rotation augmentation on the GPU (csrc/affine.hip clipmi_affine_u8, clipmi/images.py): every comparison is
bit for bit against tests/affine_ref.py, which tests/test_cpu_affine.py pins to PIL.  The output sits in a
guard-banded buffer at a 1-byte offset, so image bases take every alignment and a store outside the batch is caught."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import affine_ref as A  # noqa: E402
import color_ref as C  # noqa: E402
from kernel_checks import GUARD_PATTERN, guarded1d  # noqa: E402

from clipmi import CLIPAdapterTrainer, CLIPWithAdapters, _lib, synth  # noqa: E402
from clipmi import kernels as K  # noqa: E402
from clipmi.images import (MODES, AffineItem, ColorJitter, ImageBatch, RandomAffine, RandomRotation,  # noqa: E402
                           TrainAugment, affine_matrix, affine_u8, color_jitter_u8, preprocess, rotation_matrix)

IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
OUTSIDE = [1.0, 0.0, 5000.0, 0.0, 1.0, 0.0]


def run(imgs, items):
    """uint8 [B, H, W, 3] (numpy) through affine_u8 into guard bands at a 1-byte offset -> numpy; src must come
    back unchanged."""
    B, H, W, _ = imgs.shape
    src = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    buf, chk = guarded1d(imgs.size, torch.uint8, offset_elems=1)
    out = affine_u8(src, items, out=buf.view(B, H, W, 3))
    torch.cuda.synchronize()
    chk()
    assert out.data_ptr() == buf.data_ptr()
    assert np.array_equal(src.cpu().numpy(), imgs), "affine_u8 wrote to its source"
    return out.cpu().numpy()


def expect(imgs, items):
    return np.stack([A.apply_item(im, it) for im, it in zip(imgs, items)])


def assert_same(got, ref, items):
    for b in range(len(ref)):
        bad = got[b] != ref[b]
        assert not bad.any(), (b, items[b].matrix, items[b].filter, hex(items[b].fill), np.argwhere(bad)[:4].tolist(),
                               got[b][bad][:4].tolist(), ref[b][bad][:4].tolist())


def random_batch(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def path_matrices(path, H, W):
    """Four matrices that take one sampling path on an H x W image."""
    if path == "scale":
        return [[1, 0, 1, 0, 1, -1], [0.7, 0, 0.3, 0, 1.3, -0.2], [-1, 0, W, 0, 1, 0], [0.1, 0, -0.05, 0, 0.9, -0.45]]
    return [affine_matrix(20.0, (1, 0), 1.1, (5.0, 0.0), W, H), rotation_matrix(90, W, H),
            affine_matrix(-140.0, (0, 1), 0.8, (0.0, -8.0), W, H), rotation_matrix(1e-7, W, H)]


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 7), (31, 33), (32, 32)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("path", ["bilinear", "fixed", "scale"])
def test_each_path_alone(path, hw):
    """Four matrices of one path and an identity item (in the middle, so both its neighbours store next to it) whose
    image must come out equal to the source; neighbours differ in fill, and, around the identity, in filter.  The
    odd sizes put image bases at every alignment: head and tail pixels."""
    H, W = hw
    imgs = random_batch(5, H, W, seed=H * 100 + W)
    filt = "bilinear" if path == "bilinear" else "nearest"
    fills = [0, (255, 0, 7), 0x55, (1, 2, 3)]
    items = [AffineItem.of(m, filt, f) for m, f in zip(path_matrices(path, H, W), fills)]
    assert all(A.path_of(it.matrix, it.filter) == path for it in items)
    items.insert(2, AffineItem.of(IDENTITY, "nearest" if path == "bilinear" else "bilinear", 0xAB))
    got = run(imgs, items)
    assert np.array_equal(got[2], imgs[2]), "the identity item's image changed"
    assert_same(got, expect(imgs, items), items)


def test_mixed_batch():
    """All three paths side by side on a non-square image, identities under both filters, and items that map every
    pixel outside: their images are all fill."""
    H, W = 19, 42
    imgs = random_batch(9, H, W, seed=11)
    items = [AffineItem.of(affine_matrix(12.0, (3, -2), 0.9, (4.0, 2.0), W, H), "bilinear", (10, 20, 30)),
             AffineItem.of([0.8, 0, 2.5, 0, 1.2, -1.5], "nearest", 77),
             AffineItem.of(affine_matrix(-33.0, (-4, 1), 1.2, (0.0, 9.0), W, H), "nearest", (200, 100, 0)),
             AffineItem.of(OUTSIDE, "bilinear", (9, 8, 7)),
             AffineItem.of(IDENTITY, "bilinear"),
             AffineItem.of(OUTSIDE, "nearest", (1, 255, 2)),
             AffineItem.of([0.5, 0.1, 0, 0.1, 0.5, -3000], "nearest", (3, 4, 5)),
             AffineItem.of(IDENTITY, "nearest"),
             AffineItem.of(rotation_matrix(270, W, H), "bilinear", 255)]
    assert {A.path_of(it.matrix, it.filter) for it in items} == {"bilinear", "fixed", "scale"}
    got = run(imgs, items)
    for b, rgb in ((3, (9, 8, 7)), (5, (1, 255, 2)), (6, (3, 4, 5))):
        assert (got[b] == np.array(rgb, np.uint8)).all(), b
    assert np.array_equal(got[4], imgs[4]) and np.array_equal(got[7], imgs[7])
    assert_same(got, expect(imgs, items), items)


def test_bilinear_boundaries():
    """dx, dy in {0, 0.5} (integer and half-pixel shifts in every direction), a source exactly on xo == W and on
    yo == H (outside: >=), rows with yi + 1 == H (v2 = v1) and with yi == -1 (the row clamps to 0, v2 from row 0)."""
    H, W = 6, 9
    ms = [[1, 0, sx, 0, 1, sy] for sx in (0, 0.5, -0.5, 1, -1) for sy in (0, 0.5, -0.5, 1, -1)]
    ms += [[1, 0, W - 0.5, 0, 1, 0],    # x = 0: xo = 0.5 + W - 0.5 == W exactly
           [1, 0, 0, 0, 1, H - 0.5],    # y = 0: yo == H exactly
           [1, 0, 0, 0, 1, H - 1.0],    # y = 0: yo = H - 0.5, yi = H - 1, dy = 0, yi + 1 == H
           [1, 0, 0, 0, 1, H - 0.75],   # y = 0: yi = H - 1, dy = 0.25, yi + 1 == H
           [1, 0, 0, 0, 1, -0.25],      # y = 0: yo = 0.25, yi = -1, dy = 0.75
           [1, 0, -0.25, 0, 1, -0.25]]  # xi = -1 too
    imgs = random_batch(len(ms), H, W, seed=6)
    items = [AffineItem.of(m, "bilinear", (k * 7) % 256) for k, m in enumerate(ms)]
    got = run(imgs, items)
    k = 25
    assert (got[k][:, 0] == items[k].fill & 255).all() and (got[k + 1][0] == items[k + 1].fill & 255).all()
    assert np.array_equal(got[k + 2][0], imgs[k + 2][H - 1]) and np.array_equal(got[k + 3][0], imgs[k + 3][H - 1])
    assert np.array_equal(got[k + 4][0], imgs[k + 4][0])
    assert_same(got, expect(imgs, items), items)


def test_full_size_stride_repeatable_and_source_unchanged():
    """S = 224, B = 3, one image per path: threads stride over more than one group; the call twice gives the same
    bytes and leaves src as it was (checked inside run)."""
    imgs = random_batch(3, 224, 224, seed=224)
    items = [AffineItem.of(affine_matrix(15.0, (22, -22), 1.1, (10.0, 0.0), 224, 224), "bilinear", (128, 0, 255)),
             AffineItem.of(affine_matrix(-15.0, (-9, 4), 0.9, (-10.0, 5.0), 224, 224), "nearest", 3),
             AffineItem.of([0.9, 0, -0.45, 0, 1.1, -0.55], "nearest", (0, 255, 0))]
    assert [A.path_of(it.matrix, it.filter) for it in items] == ["bilinear", "fixed", "scale"]
    got = run(imgs, items)
    assert_same(got, expect(imgs, items), items)
    assert np.array_equal(run(imgs, items), got)
    plain = affine_u8(torch.from_numpy(imgs).cuda(), items)  # out=None: a new tensor with the same bytes
    assert np.array_equal(plain.cpu().numpy(), got)


def test_invalid_input_raises_before_launch():
    x = torch.arange(2 * 4 * 4 * 3, dtype=torch.uint8, device="cuda").view(2, 4, 4, 3)
    dst = torch.full_like(x, GUARD_PATTERN)
    ident = AffineItem.of(IDENTITY)
    with pytest.raises(ValueError, match="item 1"):
        affine_u8(x, [ident, AffineItem.of([1, 0, float("nan"), 0, 1, 0])], out=dst)
    with pytest.raises(ValueError, match="item 1.*16384"):
        affine_u8(x, [ident, AffineItem.of([1, 0, 16384, 0, 1, 0])], out=dst)
    with pytest.raises(ValueError, match="item 0.*16384"):
        affine_u8(x, [AffineItem.of([1, 0, 0, 4000, 100, 0], "bilinear"), ident], out=dst)
    with pytest.raises(ValueError, match="records"):
        affine_u8(x, [ident], out=dst)
    with pytest.raises(ValueError, match="GPU"):
        affine_u8(x.cpu(), [ident, ident])
    with pytest.raises(ValueError, match="uint8"):
        affine_u8(x.float(), [ident, ident], out=dst)
    with pytest.raises(ValueError, match="AffineItem"):
        affine_u8(x, [IDENTITY, IDENTITY], out=dst)
    with pytest.raises(ValueError, match="out"):
        affine_u8(x, [ident, ident], out=dst[:1])
    torch.cuda.synchronize()
    assert bool((dst == GUARD_PATTERN).all()), "a rejected call wrote to dst"
    # aliasing: the same tensor, and a view that shares some of its bytes
    before = x.clone()
    with pytest.raises(ValueError, match="alias"):
        affine_u8(x, [ident, ident], out=x)
    flat = torch.zeros(3 * 4 * 4 * 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="alias"):
        affine_u8(flat[:96].view(2, 4, 4, 3), [ident, ident], out=flat[48:144].view(2, 4, 4, 3))
    L = _lib.lib()  # and the library itself refuses overlapping pointers
    table = (AffineItem * 2)(ident, ident)
    st = L.clipmi_affine_u8(K.stream(), x.data_ptr(), x.data_ptr() + 1, table, 2, 4, 4, K.ptr(flat), flat.numel())
    assert st == -1 and "overlap" in L.clipmi_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(x, before) and int(flat.sum()) == 0
    # B = 0 is a no-op
    assert affine_u8(x[:0], []).shape == (0, 4, 4, 3)
    assert affine_u8(x[:0], [], out=dst[:0]).shape == (0, 4, 4, 3)
    assert bool((dst == GUARD_PATTERN).all())


# ------------------------------------------------------------------------------------------------ preprocess
def ragged_images(seed=9):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(70, 64), (65, 200), (130, 90), (64, 64), (33, 47)]]


def parent_preprocess(batch, S, mode):
    """clipmi_resize_crop_u8 called as preprocess called it before it knew of affine records."""
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
@pytest.mark.parametrize("interpolation", ["nearest", "bilinear"])
def test_preprocess_with_and_without_affine(mode, interpolation):
    S = 48
    batch = ImageBatch.pack(ragged_images()).with_flips([0, 1, 0, 1, 1]).with_mode(mode).to("cuda")
    B = len(batch)
    plain = preprocess(batch, S)
    assert torch.equal(plain, parent_preprocess(batch, S, mode)), "affine=None no longer gives the parent's bytes"
    g = torch.Generator().manual_seed(3)
    items = RandomAffine(15, (0.1, 0.1), (0.9, 1.1), 10, interpolation=interpolation, fill=(5, 6, 7), p=0.8).sample(B, S, g)
    assert any(it.is_identity() for it in items) and not all(it.is_identity() for it in items)
    fused = preprocess(batch.with_affine(items), S)
    assert not torch.equal(fused, plain)
    assert torch.equal(fused, affine_u8(plain, items))
    assert np.array_equal(fused.cpu().numpy(), expect(plain.cpu().numpy(), items))
    into = torch.empty(B * S * S * 3, dtype=torch.uint8, device="cuda")
    assert torch.equal(preprocess(batch.with_affine(items), S, out=into), fused)
    assert torch.equal(preprocess(batch, S, out=into), plain)
    # with colour records too: the affine pass first, as Compose([..., RandomAffine, ColorJitter]) runs them
    colour = ColorJitter(0.4, 0.4, 0.4, 0.1, 0.3).sample(B, g)
    both = preprocess(batch.with_affine(items).with_color(colour), S)
    assert torch.equal(both, color_jitter_u8(affine_u8(plain, items), colour))
    ref = np.stack([C.apply_item(im, it) for im, it in zip(expect(plain.cpu().numpy(), items), colour)])
    assert np.array_equal(both.cpu().numpy(), ref)
    assert torch.equal(preprocess(batch.with_color(colour).with_affine(items), S, out=into), both)
    assert torch.equal(preprocess(batch.with_color(colour), S), color_jitter_u8(plain.clone(), colour))


def test_random_rotation_through_preprocess():
    S = 32
    batch = ImageBatch.pack(ragged_images()).with_mode("square").to("cuda")
    items = RandomRotation(30, interpolation="bilinear", fill=9).sample(len(batch), S, torch.Generator().manual_seed(1))
    plain = preprocess(batch, S)
    assert np.array_equal(preprocess(batch.with_affine(items), S).cpu().numpy(), expect(plain.cpu().numpy(), items))


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


def test_trainer_affine_augment_reproducible(tmp_path):
    affine = dict(degrees=15, translate=(0.1, 0.1), scale=(0.9, 1.1), shear=10, interpolation="bilinear")
    a = train_losses(TrainAugment(seed=3, affine=RandomAffine(**affine)), tmp_path)
    b = train_losses(TrainAugment(seed=3, affine=RandomAffine(**affine)), tmp_path)
    plain = train_losses(TrainAugment(seed=3), tmp_path)
    assert all(bool(torch.isfinite(x)) for x in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), (a, b)
    assert not torch.equal(a[0], plain[0]), "the affine records did not reach the images"
