"""The policy augmentations on the GPU (csrc/enhance.hip clipmi_enhance_u8; clipmi/images.py enhance_u8,
apply_policy_u8, preprocess, TrainAugment): every comparison is bit for bit against tests/enhance_ref.py, which
tests/test_cpu_enhance.py pins to PIL.  The source and the output each sit in a guard-banded buffer at a 1-byte offset,
so image bases take every alignment and a store outside the batch is caught; the source is checked unchanged."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import affine_ref as A  # noqa: E402
import color_ref as C  # noqa: E402
import enhance_ref as E  # noqa: E402
from kernel_checks import GUARD_PATTERN, guarded1d  # noqa: E402
from oracle import resize_ref as RR  # noqa: E402
from test_cpu_enhance import MAGNITUDES, SIGNED, histogram_images  # noqa: E402

from clipmi import CLIPAdapterTrainer, CLIPWithAdapters, _lib, synth  # noqa: E402
from clipmi import kernels as K  # noqa: E402
from clipmi.images import (ColorJitter, EnhanceItem, ImageBatch, RandomAffine, TrainAugment,  # noqa: E402
                           TrivialAugmentWide, apply_policy_u8, enhance_u8, policy_calls, preprocess)

SIZES = [(1, 1), (2, 5), (3, 3), (5, 7), (31, 33), (16, 16)]
VALUES = {"posterize": [1, 4, 7, 8], "solarize": [0.5, 128, 178.5, 256], "sharpness": [0, 0.55, 1, 1.9],
          "autocontrast": [0, 0, 0, 0], "equalize": [0, 0, 0, 0]}


def guarded_pair(imgs):
    """(src view holding imgs, its guard check, dst view, its guard check), both at a 1-byte offset."""
    src, src_chk = guarded1d(imgs.size, torch.uint8, offset_elems=1)
    src.copy_(torch.from_numpy(np.ascontiguousarray(imgs)).reshape(-1))
    dst, dst_chk = guarded1d(imgs.size, torch.uint8, offset_elems=1)
    return src.view(imgs.shape), src_chk, dst.view(imgs.shape), dst_chk


def run(imgs, fn):
    """uint8 [B, H, W, 3] (numpy) through fn(src, out=dst) between guard bands -> numpy; src must come back unchanged."""
    src, src_chk, dst, dst_chk = guarded_pair(imgs)
    out = fn(src, out=dst)
    torch.cuda.synchronize()
    dst_chk()
    src_chk()
    assert out.data_ptr() == dst.data_ptr()
    assert np.array_equal(src.cpu().numpy(), imgs), "the call wrote to its source"
    return out.cpu().numpy()


def run_enhance(imgs, items):
    return run(imgs, lambda src, out: enhance_u8(src, items, out=out))


def expect(imgs, items):
    return np.stack([E.apply_enhance(im, it) for im, it in zip(imgs, items)])


def assert_same(got, ref, what):
    for b in range(len(ref)):
        bad = got[b] != ref[b]
        assert not bad.any(), (b, what[b], np.argwhere(bad)[:4].tolist(), got[b][bad][:4].tolist(), ref[b][bad][:4].tolist())


def describe(items):
    return [(it.name, it.value) for it in items]


def random_batch(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("op", list(VALUES))
def test_each_op_alone(op, hw):
    """Four items of one op and an identity item in the middle (both its neighbours store next to it) whose bytes
    must arrive unchanged.  The odd sizes put image bases at every alignment: head and tail pixels."""
    H, W = hw
    imgs = random_batch(5, H, W, seed=H * 100 + W)
    items = [EnhanceItem.of(op, v) for v in VALUES[op]]
    items.insert(2, EnhanceItem.of("none"))
    got = run_enhance(imgs, items)
    assert np.array_equal(got[2], imgs[2]), "the identity item's image changed"
    assert_same(got, expect(imgs, items), describe(items))
    if op == "equalize" and hw == (16, 16):
        assert (got[0] != imgs[0]).any(), "256 pixels: step == 1, equalize must act"


def test_histogram_edge_cases_in_one_mixed_batch():
    """The constant, {0, 200}, {100, 101}, 17x15 (equalize's step == 0), 16x16 and 1x300 images through autocontrast
    and equalize, posterize and identity items between them: the histogram rows of neighbouring images.  The images
    differ in size, so each size is one call over all its images under both ops."""
    by_size = {}
    for name, img in histogram_images().items():
        by_size.setdefault(img.shape, []).append((name, img))
    seen = set()
    for shape, named in by_size.items():
        imgs, items, names = [], [], []
        for name, img in named:
            for op, between in (("autocontrast", EnhanceItem.of("posterize", 3)), ("equalize", EnhanceItem.of("none"))):
                imgs += [img, img]
                items += [EnhanceItem.of(op), between]
                names += [(name, op), (name, between.name)]
        imgs = np.stack(imgs)
        got = run_enhance(imgs, items)
        assert_same(got, expect(imgs, items), names)
        for b, (name, op) in enumerate(names):
            seen.add(name)
            if name == "only_0_and_200" and op == "autocontrast":
                assert set(np.unique(got[b])) == {0, 254}
            if name in ("constant", "random_17x15") and op == "equalize":
                assert np.array_equal(got[b], imgs[b]), name
            if name == "random_16x16" and op == "equalize":
                assert (got[b] != imgs[b]).any()
    assert seen == set(histogram_images())


def test_equalize_lut_entry_above_255():
    img = np.zeros((1, 400, 3), np.uint8)
    img[0, :, :] = (np.arange(400) % 256)[:, None]
    img[0, 300:, :] = 254
    imgs = np.stack([img, img[:, ::-1].copy()])
    items = [EnhanceItem.of("equalize")] * 2
    got = run_enhance(imgs, items)
    assert got.max() == 255
    assert_same(got, expect(imgs, items), describe(items))


def test_full_size_stride_and_repeatable():
    """S = 224: 50,176 pixels, so threads take more than one group; one image each of equalize, autocontrast and
    sharpness (the autocontrast image spans 16..235, so its LUT is no identity); the call twice gives the same bytes."""
    imgs = random_batch(3, 224, 224, seed=224)
    imgs[1] = (16 + imgs[1].astype(np.int32) * 219 // 255).astype(np.uint8)
    items = [EnhanceItem.of("equalize"), EnhanceItem.of("autocontrast"), EnhanceItem.of("sharpness", 1.9)]
    got = run_enhance(imgs, items)
    assert all((got[b] != imgs[b]).any() for b in range(3))
    assert_same(got, expect(imgs, items), describe(items))
    assert np.array_equal(run_enhance(imgs, items), got)
    plain = enhance_u8(torch.from_numpy(imgs).cuda(), items)  # out=None: a new tensor, source and output aligned alike
    assert np.array_equal(plain.cpu().numpy(), got)


def test_no_histogram_op_single_image_and_unlike_alignment():
    """A batch without an autocontrast or an equalize (the one-launch path), B = 1 under every op, and a source and
    an output that sit differently modulo 4 (the source is then read byte by byte)."""
    imgs = random_batch(6, 9, 13, seed=5)
    items = [EnhanceItem.of("posterize", 2), EnhanceItem.of("solarize", 100.5), EnhanceItem.of("none"),
             EnhanceItem.of("sharpness", 0.3), EnhanceItem.of("sharpness", 3), EnhanceItem.of("posterize", 8)]
    L = _lib.lib()
    table = (EnhanceItem * 6)(*items)
    assert 0 < L.clipmi_enhance_u8_ws(table, 6, 9, 13) < 768, "a histogram table was asked for"
    ref = expect(imgs, items)
    assert_same(run_enhance(imgs, items), ref, describe(items))
    for op, v in (("none", 0), ("posterize", 5), ("solarize", 60), ("autocontrast", 0), ("equalize", 0), ("sharpness", 1.5)):
        one = [EnhanceItem.of(op, v)]
        assert_same(run_enhance(imgs[:1], one), expect(imgs[:1], one), describe(one))
    all_ops = [EnhanceItem.of(op, v) for op, v in (("equalize", 0), ("posterize", 3), ("solarize", 99), ("autocontrast", 0),
                                                   ("sharpness", 0.5), ("none", 0))]
    for shift in (0, 2, 3):  # dst at 1 (mod 4); src at 1 + shift
        src, src_chk = guarded1d(imgs.size + shift, torch.uint8, offset_elems=1)
        src[shift:].copy_(torch.from_numpy(imgs).reshape(-1))
        dst, dst_chk = guarded1d(imgs.size, torch.uint8, offset_elems=1)
        out = enhance_u8(src[shift:].view(imgs.shape), all_ops, out=dst.view(imgs.shape))
        torch.cuda.synchronize()
        dst_chk(), src_chk()
        assert_same(out.cpu().numpy(), expect(imgs, all_ops), describe(all_ops))


def test_invalid_input_raises_before_launch():
    x = torch.arange(2 * 4 * 4 * 3, dtype=torch.uint8, device="cuda").view(2, 4, 4, 3)
    dst = torch.full_like(x, GUARD_PATTERN)
    none = EnhanceItem.of("none")
    for bad, match in ((EnhanceItem.of("posterize", 0), "item 1.*bits"), (EnhanceItem.of("posterize", 2.5), "item 1.*bits"),
                       (EnhanceItem.of("solarize", float("nan")), "item 1.*finite"),
                       (EnhanceItem.of("sharpness", -1), "item 1.*sharpness"), (EnhanceItem(9, 0.0), "item 1.*op")):
        with pytest.raises(ValueError, match=match):
            enhance_u8(x, [none, bad], out=dst)
    with pytest.raises(ValueError, match="records"):
        enhance_u8(x, [none], out=dst)
    with pytest.raises(ValueError, match="GPU"):
        enhance_u8(x.cpu(), [none, none])
    with pytest.raises(ValueError, match="uint8"):
        enhance_u8(x.float(), [none, none], out=dst)
    with pytest.raises(ValueError, match="EnhanceItem"):
        enhance_u8(x, [("none", 0), ("none", 0)], out=dst)
    with pytest.raises(ValueError, match="out"):
        enhance_u8(x, [none, none], out=dst[:1])
    with pytest.raises(ValueError, match="Invert"):
        apply_policy_u8(x, [[("Invert", 0.0)], []], out=dst)
    with pytest.raises(ValueError, match="programs"):
        apply_policy_u8(x, [[]], out=dst)
    with pytest.raises(ValueError, match="bits"):
        apply_policy_u8(x, [[("Posterize", 0.0)], []], out=dst)
    torch.cuda.synchronize()
    assert bool((dst == GUARD_PATTERN).all()), "a rejected call wrote to dst"
    before = x.clone()
    with pytest.raises(ValueError, match="alias"):
        enhance_u8(x, [none, none], out=x)
    with pytest.raises(ValueError, match="alias"):
        apply_policy_u8(x, [[], []], out=x)
    flat = torch.zeros(3 * 4 * 4 * 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="alias"):
        enhance_u8(flat[:96].view(2, 4, 4, 3), [none, none], out=flat[48:144].view(2, 4, 4, 3))
    L = _lib.lib()  # and the library itself refuses overlapping pointers
    table = (EnhanceItem * 2)(none, none)
    st = L.clipmi_enhance_u8(K.stream(), x.data_ptr(), x.data_ptr() + 1, table, 2, 4, 4, K.ptr(flat), flat.numel())
    assert st == -1 and "overlap" in L.clipmi_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(x, before) and int(flat.sum()) == 0
    assert enhance_u8(x[:0], []).shape == (0, 4, 4, 3)
    assert enhance_u8(x[:0], [], out=dst[:0]).shape == (0, 4, 4, 3)
    assert apply_policy_u8(x[:0], []).shape == (0, 4, 4, 3)
    assert bool((dst == GUARD_PATTERN).all())


# ------------------------------------------------------------------------------------------------ the executor
def run_policy(imgs, programs, interpolation, fill):
    return run(imgs, lambda src, out: apply_policy_u8(src, programs, interpolation, fill, out=out))


def expect_policy(imgs, programs, interpolation, fill):
    return np.stack([E.apply_program(im, p, interpolation, fill) for im, p in zip(imgs, programs)])


def signed(name, k):
    return MAGNITUDES[name] * (-1 if name in SIGNED and k % 2 else 1)


def one_op_programs():
    return [[(name, signed(name, k))] for k, name in enumerate(E.POLICY_OPS)]


def two_op_programs():
    """Twelve programs that mix the three kinds in both orders."""
    pairs = [("Rotate", "Equalize"), ("Equalize", "Rotate"), ("ShearX", "Contrast"), ("Contrast", "ShearX"),
             ("Sharpness", "Brightness"), ("Brightness", "Sharpness"), ("TranslateY", "AutoContrast"),
             ("AutoContrast", "TranslateY"), ("Color", "Posterize"), ("Solarize", "Color"), ("ShearY", "TranslateX"),
             ("Posterize", "Sharpness")]
    return [[(a, signed(a, k)), (b, signed(b, k + 1))] for k, (a, b) in enumerate(pairs)]


@pytest.mark.parametrize("interpolation,fill", [("nearest", (9, 200, 77)), ("bilinear", 128)])
@pytest.mark.parametrize("programs", [one_op_programs, two_op_programs], ids=["one_op", "two_ops"])
def test_apply_policy_matches_apply_program(programs, interpolation, fill):
    programs = programs()
    imgs = random_batch(len(programs), 31, 33, seed=len(programs))
    got = run_policy(imgs, programs, interpolation, fill)
    assert_same(got, expect_policy(imgs, programs, interpolation, fill), programs)


def test_apply_policy_ragged_programs_and_identities():
    """Programs of length 0, 1 and 2 in one batch (shorter ones get the identity); identity programs leave the bytes
    as they were; a colour op first (the in-place call must not touch the source); fill None is black; out=None."""
    imgs = random_batch(6, 31, 33, seed=6)
    programs = [[], [("Identity", 0.0)], [("Brightness", 0.5), ("Rotate", -30.0)], [("Equalize", 0.0)],
                [("Identity", 0.0), ("Solarize", 178.5)], [("Contrast", -0.7)]]
    assert [k for k, _ in policy_calls(programs, 33, 31)] == ["enhance", "color", "affine", "enhance"]
    got = run_policy(imgs, programs, "bilinear", None)
    assert np.array_equal(got[0], imgs[0]) and np.array_equal(got[1], imgs[1])
    assert_same(got, expect_policy(imgs, programs, "bilinear", None), programs)
    colour_only = [[("Color", 0.9)], [], [("Brightness", -0.5), ("Contrast", 0.7)], [], [], [("Identity", 0.0)]]
    assert_same(run_policy(imgs, colour_only, "nearest", 0), expect_policy(imgs, colour_only, "nearest", 0), colour_only)
    nothing = [[]] * 6
    assert np.array_equal(run_policy(imgs, nothing, "nearest", 0), imgs)
    src = torch.from_numpy(imgs).cuda()
    assert np.array_equal(apply_policy_u8(src, programs, "bilinear", None).cpu().numpy(), got)
    assert np.array_equal(src.cpu().numpy(), imgs)


# ------------------------------------------------------------------------------------------------ preprocess
def ragged_images(seed=9):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(70, 64), (65, 200), (130, 90), (64, 64), (33, 47)]]


def test_preprocess_end_to_end():
    """A ragged batch with boxes, flips, a policy, affine records and colour records against the oracle's resize, then
    apply_program, affine_ref and color_ref; without a policy the bytes are those of an empty policy."""
    S = 32
    images = ragged_images()
    boxes = [(3, 5, 50, 60), (10, 0, 120, 65), (0, 20, 90, 100), (0, 0, 64, 64), (7, 3, 30, 28)]
    flips = [0, 1, 0, 1, 1]
    batch = ImageBatch.pack(images).with_boxes(boxes).with_flips(flips).with_mode("square").to("cuda")
    B = len(batch)
    resized = []
    for img, (x0, y0, cw, ch), f in zip(images, boxes, flips):
        r = RR.resize_bicubic(np.ascontiguousarray(img[y0:y0 + ch, x0:x0 + cw]), S, S)
        resized.append(np.ascontiguousarray(r[:, ::-1] if f else r))
    plain = preprocess(batch, S)
    assert np.array_equal(plain.cpu().numpy(), np.stack(resized))
    assert torch.equal(preprocess(batch.with_policy([[]] * B), S), plain)
    g = torch.Generator().manual_seed(3)
    programs = [[("Rotate", 30.0), ("Equalize", 0.0)], [("Sharpness", 0.9)], [], [("Posterize", 4.0), ("Color", -0.9)],
                [("AutoContrast", 0.0), ("TranslateX", -7.9)]]
    affine = RandomAffine(15, (0.1, 0.1), (0.9, 1.1), 10, interpolation="bilinear", fill=(5, 6, 7)).sample(B, S, g)
    colour = ColorJitter(0.4, 0.4, 0.4, 0.1, 0.3).sample(B, g)
    after_policy = [E.apply_program(r, p, "bilinear", (1, 2, 3)) for r, p in zip(resized, programs)]
    with_policy = batch.with_policy(programs, "bilinear", (1, 2, 3))
    assert np.array_equal(preprocess(with_policy, S).cpu().numpy(), np.stack(after_policy))
    after_affine = [A.apply_item(im, it) for im, it in zip(after_policy, affine)]
    assert np.array_equal(preprocess(with_policy.with_affine(affine), S).cpu().numpy(), np.stack(after_affine))
    ref = np.stack([C.apply_item(im, it) for im, it in zip(after_affine, colour)])
    into, chk = guarded1d(B * S * S * 3, torch.uint8, offset_elems=1)
    got = preprocess(with_policy.with_affine(affine).with_color(colour), S, out=into)
    torch.cuda.synchronize()
    chk()
    assert np.array_equal(got.cpu().numpy(), ref)
    ref = np.stack([C.apply_item(im, it) for im, it in zip(after_policy, colour)])
    assert np.array_equal(preprocess(with_policy.with_color(colour), S).cpu().numpy(), ref)
    assert torch.equal(preprocess(batch, S), plain)


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


def test_trainer_policy_augment_reproducible(tmp_path):
    a = train_losses(TrainAugment(seed=3, policy=TrivialAugmentWide(interpolation="bilinear")), tmp_path)
    b = train_losses(TrainAugment(seed=3, policy=TrivialAugmentWide(interpolation="bilinear")), tmp_path)
    plain = train_losses(TrainAugment(seed=3), tmp_path)
    assert all(bool(torch.isfinite(x)) for x in a)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), (a, b)
    assert not all(torch.equal(x, y) for x, y in zip(a, plain)), "the policy programs did not reach the images"
