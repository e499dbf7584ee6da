"""Ragged image batches on the GPU (csrc/images.hip clipmi_resize_crop_u8, clipmi/images.py): bit-exact against the
PIL restatement on the cropped array, against the uniform path's bytes, through the model and through the trainer.
The shape list, its images and boxes are tests/test_cpu_ragged_input.py's (which pins the oracle to PIL on them)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_cpu_ragged_input as cases  # noqa: E402
from kernel_checks import guarded1d, untouched  # noqa: E402
from oracle import resize_ref as RR  # noqa: E402

from clipmi import CLIPAdapterTrainer, CLIPWithAdapters, synth  # noqa: E402
from clipmi import towers as T  # noqa: E402
from clipmi.images import ImageBatch, TrainAugment, preprocess  # noqa: E402

FLIPS = [i % 2 for i in range(len(cases.SHAPES))]


@functools.lru_cache(maxsize=None)
def reference(S, mode):
    """[B, S, S, 3]: the oracle on each image's slice, the centre window in processor mode, flipped items mirrored."""
    out = []
    keep = cases.accepted(S, mode)
    for img, (x0, y0, cw, ch), f in [(cases.images()[i], cases.boxes()[i], FLIPS[i]) for i in keep]:
        oh, ow = cases.out_size(ch, cw, S, mode)
        r = RR.resize_bicubic(np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw]), oh, ow)
        top, left = (oh - S) // 2, (ow - S) // 2
        r = r[top:top + S, left:left + S]
        out.append(r[:, ::-1] if f else r)
    ref = np.stack(out)
    ref.setflags(write=False)
    return ref


def packed_with_tail(batch, fill):
    """The batch on the GPU with its packed bytes followed by 4 KiB of `fill` that belong to no image."""
    n = batch.data.numel()
    big = torch.full((n + 4096,), fill, dtype=torch.uint8, device="cuda")
    big[:n].copy_(batch.data)
    return ImageBatch(big[:n], batch.sizes, batch.offsets, batch.boxes, batch.flips, batch.mode)


@pytest.mark.parametrize("mode", ["processor", "square"])
@pytest.mark.parametrize("S", [32, 224])
def test_bit_exact_against_oracle(S, mode):
    """The whole list in one call, flips alternating, in both modes at both sizes.  Squaring 2300 x 31 to S = 32 is a
    72x downscale: above the 32x cap, so there the whole list is refused naming that item and the batch is the list
    without it (cases.accepted)."""
    keep = cases.accepted(S, mode)
    whole = ImageBatch.pack(cases.images()).with_boxes(cases.boxes()).with_flips(FLIPS)
    if len(keep) < len(whole):
        with pytest.raises(ValueError, match="item 13.*32x"):
            preprocess(whole.to("cuda"), S, mode)
    batch = ImageBatch.pack([cases.images()[i] for i in keep]).with_boxes([cases.boxes()[i] for i in keep])
    batch = batch.with_flips([FLIPS[i] for i in keep])
    B = len(batch)
    out, chk = guarded1d(B * S * S * 3, torch.uint8, offset_elems=1)  # byte-aligned, not 16-B-aligned
    preprocess(ImageBatch(torch.empty(0, dtype=torch.uint8, device="cuda"), [], []), S, mode, out=out[:0])
    torch.cuda.synchronize()
    assert untouched(out), "an empty batch stored to the output"
    got = preprocess(packed_with_tail(batch, 255), S, mode, out=out)
    torch.cuda.synchronize()
    chk()
    ref = reference(S, mode)
    got = got.cpu().numpy()
    for b in range(B):
        assert np.array_equal(got[b], ref[b]), (b, cases.SHAPES[keep[b]], np.argwhere(got[b] != ref[b])[:4].tolist())
    again = preprocess(packed_with_tail(batch, 0), S, mode)
    assert np.array_equal(again.cpu().numpy(), ref), "bytes after the packed images changed the result"


def existing_path(img, S):
    """The uniform path on one size: resize_uint8 to the shortest-edge size, then clipmi_im2col_u8's centre window."""
    x = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    x = x[None] if x.dim() == 3 else x
    oh, ow = T.shortest_edge_size(x.shape[1], x.shape[2], S)
    r = T.resize_uint8(x, oh, ow) if (oh, ow) != tuple(x.shape[1:3]) else x
    y0, x0 = (oh - S) // 2, (ow - S) // 2
    return r[:, y0:y0 + S, x0:x0 + S]


def test_uniform_batch_same_bytes_as_existing_path():
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 256, (3, 300, 451, 3), dtype=np.uint8)
    got = preprocess(ImageBatch.pack(list(imgs)).to("cuda"), 224, "processor")
    assert torch.equal(got, existing_path(imgs, 224))


@pytest.mark.parametrize("S", [32, 224])
def test_ragged_equals_one_by_one(S):
    batch = ImageBatch.pack(cases.images()).with_boxes(cases.boxes())
    got = preprocess(batch.to("cuda"), S, "processor")
    for b, (img, (x0, y0, cw, ch)) in enumerate(zip(cases.images(), cases.boxes())):
        one = existing_path(img[y0:y0 + ch, x0:x0 + cw], S)[0]
        assert torch.equal(got[b], one), (b, cases.SHAPES[b])


def test_invalid_batch_raises_before_launch():
    batch = ImageBatch.pack(cases.images()[3:6]).to("cuda")
    with pytest.raises(ValueError, match="item 1"):
        preprocess(batch.with_boxes([(0, 0, 3, 5), (0, 0, 101, 100), (0, 0, 91, 37)]), 32)
    with pytest.raises(ValueError, match="GPU"):
        preprocess(ImageBatch.pack(cases.images()[3:6]), 32)


# ------------------------------------------------------------------------------------------------ model
def tiny(precision, adapters=True, freeze=True):
    torch.manual_seed(0)
    return CLIPWithAdapters("tiny", use_text_adapter=adapters, use_vision_adapter=adapters, use_shared_adapters=False,
                            freeze_clip=freeze, device="cuda", precision=precision)


def captions(cfg, B):
    b = synth.synthetic_batch(cfg, B, seed=21)
    return {k: torch.from_numpy(b[k]) for k in ("input_ids", "attention_mask")}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_model_takes_image_batch(precision):
    m = tiny(precision, freeze=False)
    S = m.config.vision_config.image_size
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (3, 72, 80, 3), dtype=np.uint8)
    with torch.no_grad():
        a = m.get_image_features(torch.from_numpy(imgs).cuda())
        u = m.get_image_features(ImageBatch.pack(list(imgs)))  # still on the host: the model moves it
    assert torch.equal(a, u)
    ragged = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(70, 64), (65, 200), (130, 90), (64, 64)]]
    batch = ImageBatch.pack(ragged)
    with torch.no_grad():
        f = m.get_image_features(batch)
    assert f.shape == (4, m.config.projection_dim) and bool(torch.isfinite(f).all())
    out = m(pixel_values=batch, return_loss=True, **{k: v.cuda() for k, v in captions(m.config, 4).items()})
    out["loss"].backward()
    g = m.clip.vision_model.encoder.layers[0].mlp.fc1.weight.grad
    assert bool(torch.isfinite(out["loss"])) and g is not None and bool(torch.isfinite(g).all()) and float(g.abs().sum()) > 0


# ------------------------------------------------------------------------------------------------ trainer
def train_losses(augment, images, tmp, mode="processor", steps=2):
    m = tiny("bf16")
    batch = dict(captions(m.config, len(images)), pixel_values=ImageBatch.pack(images).with_mode(mode))
    tr = CLIPAdapterTrainer(m, [batch], learning_rate=1e-3, output_dir=str(tmp), augment=augment)
    return [tr.train_step(batch, i, steps) for i in range(steps)]


def test_trainer_augment_reproducible(tmp_path):
    rng = np.random.default_rng(9)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(70, 64), (65, 200), (130, 90), (64, 64)]]
    a = train_losses(TrainAugment(seed=3), images, tmp_path)
    b = train_losses(TrainAugment(seed=3), images, tmp_path)
    assert all(bool(torch.isfinite(x)) for x in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), (a, b)


def test_trainer_identity_augment_equals_square_mode(tmp_path):
    rng = np.random.default_rng(10)
    images = [rng.integers(0, 256, (n, n, 3), dtype=np.uint8) for n in (64, 90, 150, 33)]
    a = train_losses(TrainAugment(scale=(1, 1), ratio=(1, 1), flip_p=0, seed=3), images, tmp_path)
    b = train_losses(None, images, tmp_path, mode="square")
    assert all(torch.equal(x, y) for x, y in zip(a, b)), (a, b)


def test_dataloader_of_ragged_images_trains(tmp_path):
    """A DataLoader whose samples hold images of different sizes, through collate, the augmentation and train()."""
    from torch.utils.data import DataLoader
    from clipmi.images import collate
    m = tiny("bf16")
    rng = np.random.default_rng(12)
    cap = captions(m.config, 6)
    data = [{"image": torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)),
             "input_ids": cap["input_ids"][i], "attention_mask": cap["attention_mask"][i]}
            for i, (h, w) in enumerate([(70, 64), (65, 200), (130, 90), (64, 64), (33, 47), (300, 100)])]
    loader = DataLoader(data, batch_size=3, collate_fn=collate)
    tr = CLIPAdapterTrainer(m, loader, loader, learning_rate=1e-3, output_dir=str(tmp_path),
                            augment=TrainAugment(seed=1))
    before = [p.detach().clone() for p in tr.trainable_params]
    tr.train(num_epochs=1)
    assert any(not torch.equal(a, b) for a, b in zip(before, tr.trainable_params))
    assert np.isfinite(tr.evaluate())
