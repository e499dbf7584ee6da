"""The policy augmentations without a GPU: tests/enhance_ref.py (the arithmetic csrc/enhance.hip and
clipmi.images.apply_policy_u8 are held to, bit for bit, in tests/test_gpu_enhance.py) pinned to PIL's ImageOps,
ImageEnhance, ImageFilter, Image.transform and Image.rotate; the RandAugment / TrivialAugmentWide samplers against
hand-derived values of the published torchvision definition; ImageBatch and TrainAugment carrying the programs;
clipmi_enhance_u8's host-side validation through the C ABI (it rejects before any launch: pointers are never
dereferenced); the struct layout."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import enhance_ref as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARP_SIZES = [(1, 1), (2, 5), (3, 3), (13, 9), (37, 53)]
SHARP_FACTORS = [0, 0.1, 0.55, 1, 1.9, 1.99, 3]
SIGNED = ["ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness"]
TABLED = SIGNED + ["Posterize", "Solarize"]


def pil():
    pytest.importorskip("PIL.Image")
    import PIL.Image
    import PIL.ImageEnhance
    import PIL.ImageFilter
    import PIL.ImageOps
    return PIL


def random_image(h, w, seed=None):
    return np.random.default_rng(h * 1000 + w if seed is None else seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def histogram_images():
    """{name: image}: the histogram edge cases of autocontrast and equalize."""
    two = np.zeros((6, 7, 3), np.uint8)
    two[::2, 1::2] = 200
    near = random_image(9, 11, seed=3)
    near[..., 1] = 100 + (random_image(9, 11, seed=4)[..., 0] & 1)
    return {"random_37x53": random_image(37, 53), "random_5x7": random_image(5, 7),
            "constant": np.full((4, 5, 3), 77, np.uint8), "only_0_and_200": two, "channel_100_101": near,
            "random_17x15": random_image(17, 15), "random_16x16": random_image(16, 16),
            "row_1x300": random_image(1, 300)}


# ------------------------------------------------------------------------------------------------ restatement vs PIL
def test_posterize_and_solarize_match_pil():
    P = pil()
    ramp = np.arange(256, dtype=np.uint8).repeat(3).reshape(16, 16, 3)
    img = random_image(13, 9)
    for x in (ramp, img):
        p = P.Image.fromarray(x)
        for bits in range(1, 9):
            assert np.array_equal(E.posterize(x, bits), np.asarray(P.ImageOps.posterize(p, bits))), bits
        for t in (0, 0.5, 127.5, 128, 178.5, 255, 256):
            assert np.array_equal(E.solarize(x, t), np.asarray(P.ImageOps.solarize(p, t))), t
    assert np.array_equal(E.posterize(ramp, 8), ramp) and np.array_equal(E.solarize(ramp, 256), ramp)
    assert np.array_equal(E.solarize(ramp, 0), 255 - ramp)


@pytest.mark.parametrize("hw", SHARP_SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_sharpness_matches_pil(hw):
    P = pil()
    img = random_image(*hw)
    p = P.Image.fromarray(img)
    assert np.array_equal(E.smooth(img), np.asarray(p.filter(P.ImageFilter.SMOOTH)))
    for f in SHARP_FACTORS:
        got, ref = E.sharpness(img, f), np.asarray(P.ImageEnhance.Sharpness(p).enhance(f))
        assert np.array_equal(got, ref), (f, np.argwhere(got != ref)[:4].tolist())
    if min(hw) < 3:
        assert np.array_equal(E.sharpness(img, 1.9), img)
    assert np.array_equal(E.sharpness(img, 1), img)


def test_autocontrast_and_equalize_match_pil():
    P = pil()
    out = {}
    for name, img in histogram_images().items():
        p = P.Image.fromarray(img)
        ac, eq = E.autocontrast(img), E.equalize(img)
        assert np.array_equal(ac, np.asarray(P.ImageOps.autocontrast(p))), name
        assert np.array_equal(eq, np.asarray(P.ImageOps.equalize(p))), name
        out[name] = (img, ac, eq)
    img, ac, eq = out["constant"]
    assert np.array_equal(ac, img) and np.array_equal(eq, img)
    img, ac, eq = out["only_0_and_200"]
    assert set(np.unique(ac)) == {0, 254}, "the truncated double product: 200 * (255 / 200) is just below 255"
    img, ac, eq = out["channel_100_101"]
    assert set(np.unique(ac[..., 1])) == {0, 255}
    img, ac, eq = out["random_17x15"]
    assert np.array_equal(eq, img), "255 pixels: step == 0, the identity"
    img, ac, eq = out["random_16x16"]
    assert int((eq != img).sum()) > 0, "256 pixels: step == 1, equalize must act"


def test_equalize_lut_entry_above_255_is_stored_as_255():
    """The last non-empty bin is 255 and the bins below it hold more than 255 steps: n // step passes 255, and
    Image.point stores the entry clipped to a byte."""
    P = pil()
    img = np.zeros((1, 400, 3), np.uint8)
    img[0, :, :] = (np.arange(400) % 256)[:, None]
    img[0, 300:, :] = 254
    h = E.histogram(img[..., 0])
    assert h[255] == 1 and (int(h.sum()) - 1) // 255 == 1 and int(h[:255].sum()) > 255
    got = E.equalize(img)
    assert got.max() == 255 and np.array_equal(got, np.asarray(P.ImageOps.equalize(P.Image.fromarray(img))))


def test_float32_lut_and_double_smooth_would_differ():
    """The tests discriminate: the autocontrast LUT formed in float32 instead of double changes bytes, and so does
    SMOOTH without its rounding offset."""
    h = np.zeros(256, np.int64)
    h[[0, 200]] = 1
    narrow = np.float32(255.0) / np.float32(200)
    assert E.autocontrast_lut(h)[200] == 254 and int(np.float32(200) * narrow + np.float32(-0.0) * narrow) == 255
    diff = 0
    for lo in range(0, 255, 7):
        for hi in range(lo + 1, 256, 5):
            h = np.zeros(256, np.int64)
            h[[lo, hi]] = 1
            s = np.float32(255.0) / np.float32(hi - lo)
            o = np.float32(-lo) * s
            f32 = np.clip((np.arange(256, dtype=np.float32) * s + o).astype(np.int64), 0, 255)
            diff += int((f32 != E.autocontrast_lut(h)).sum())
    assert diff > 0
    # SMOOTH: the exact sum is 0.5 + s / 13 with s an integer, never closer than 1 / 26 to an integer, and the float32
    # error stays below 1e-4: the width of the sum cannot show (asserted, so that nobody looks for it), the 0.5 does
    img = random_image(37, 53)
    p = img.astype(np.float64)
    k = E.SMOOTH_KERNEL.astype(np.float64)
    ss = np.zeros((35, 51, 3))
    for j, dy in enumerate((1, 0, -1)):
        rows = p[1 + dy:36 + dy]
        ss = ss + (k[3 * j] * rows[:, 0:51] + k[3 * j + 1] * rows[:, 1:52] + k[3 * j + 2] * rows[:, 2:53])
    inner = E.smooth(img)[1:-1, 1:-1]
    assert np.array_equal(np.trunc(ss + 0.5).astype(np.uint8), inner)
    assert int((np.trunc(ss).astype(np.uint8) != inner).sum()) > 1000


# ------------------------------------------------------------------------------------------------ programs vs PIL
def pil_op(P, p, name, m, interpolation, fill):
    """autoaugment._apply_op on a PIL image, spelled out with PIL calls and clipmi.images' matrices."""
    from clipmi.images import policy_matrix
    w, h = p.size
    resample = P.Image.BILINEAR if interpolation == "bilinear" else P.Image.NEAREST
    fc = tuple(int(v) for v in ((fill,) * 3 if isinstance(fill, int) else (0, 0, 0) if fill is None else fill))
    if name == "Identity":
        return p
    if name in ("ShearX", "ShearY", "TranslateX", "TranslateY"):
        return p.transform((w, h), P.Image.AFFINE, policy_matrix(name, m, w, h), resample, fillcolor=fc)
    if name == "Rotate":
        return p.rotate(m, resample, fillcolor=fc)
    if name == "Brightness":
        return P.ImageEnhance.Brightness(p).enhance(1.0 + m)
    if name == "Color":
        return P.ImageEnhance.Color(p).enhance(1.0 + m)
    if name == "Contrast":
        return P.ImageEnhance.Contrast(p).enhance(1.0 + m)
    if name == "Sharpness":
        return P.ImageEnhance.Sharpness(p).enhance(1.0 + m)
    if name == "Posterize":
        return P.ImageOps.posterize(p, int(m))
    if name == "Solarize":
        return P.ImageOps.solarize(p, m)
    if name == "AutoContrast":
        return P.ImageOps.autocontrast(p)
    assert name == "Equalize"
    return P.ImageOps.equalize(p)


def pil_program(P, img, program, interpolation, fill):
    p = P.Image.fromarray(img)
    for name, m in program:
        p = pil_op(P, p, name, m, interpolation, fill)
    return np.asarray(p)


MAGNITUDES = {"Identity": 0.0, "ShearX": 0.3, "ShearY": 0.2, "TranslateX": 7.9, "TranslateY": 4.0, "Rotate": 30.0,
              "Brightness": 0.5, "Color": 0.9, "Contrast": 0.7, "Sharpness": 0.9, "Posterize": 4.0, "Solarize": 178.5,
              "AutoContrast": 0.0, "Equalize": 0.0}


@pytest.mark.parametrize("interpolation", ["nearest", "bilinear"])
def test_each_op_alone_matches_pil(interpolation):
    P = pil()
    assert list(MAGNITUDES) == E.POLICY_OPS
    img = random_image(31, 33)
    for name, m in MAGNITUDES.items():
        for sign in ((1, -1) if name in SIGNED else (1,)):
            for fill in (0, (9, 200, 77), None):
                prog = [(name, sign * m)]
                got, ref = E.apply_program(img, prog, interpolation, fill), pil_program(P, img, prog, interpolation, fill)
                assert np.array_equal(got, ref), (name, sign, fill, np.argwhere(got != ref)[:4].tolist())
                if name != "AutoContrast":  # the identity on an image whose channels span 0..255
                    assert (name == "Identity") == np.array_equal(got, img), name


def test_two_op_programs_match_pil():
    """Five random pairs, and a geometric op with Equalize in both orders: the fill pixels enter the histogram, so the
    order shows."""
    P = pil()
    rng = np.random.default_rng(5)
    img = random_image(31, 33, seed=8)
    progs = []
    for _ in range(5):
        a, b = (E.POLICY_OPS[i] for i in rng.integers(1, 14, 2))
        progs.append([(a, MAGNITUDES[a] * (-1 if a in SIGNED and rng.integers(2) else 1)),
                      (b, MAGNITUDES[b] * (-1 if b in SIGNED and rng.integers(2) else 1))])
    progs += [[("Rotate", 30.0), ("Equalize", 0.0)], [("Equalize", 0.0), ("Rotate", 30.0)],
              [("ShearX", -0.3), ("Equalize", 0.0)], [("Equalize", 0.0), ("ShearX", -0.3)]]
    outs = []
    for prog in progs:
        for interpolation, fill in (("nearest", 128), ("bilinear", (1, 2, 3))):
            got = E.apply_program(img, prog, interpolation, fill)
            ref = pil_program(P, img, prog, interpolation, fill)
            assert np.array_equal(got, ref), (prog, interpolation, np.argwhere(got != ref)[:4].tolist())
            outs.append(got)
    assert not np.array_equal(outs[10], outs[12]) and not np.array_equal(outs[14], outs[16]), "the order must matter"


# ------------------------------------------------------------------------------------------------ samplers
def test_randaugment_hand_derived_magnitudes():
    from clipmi.images import POLICY_OPS, RandAugment
    assert list(POLICY_OPS) == E.POLICY_OPS
    progs = RandAugment().sample(400, 224, torch.Generator().manual_seed(0))
    assert len(progs) == 400 and all(len(p) == 2 for p in progs)
    seen = {}
    for name, m in (op for p in progs for op in p):
        seen.setdefault(name, set()).add(m)
    assert set(seen) == set(POLICY_OPS)
    want = {"ShearX": float(torch.linspace(0, 0.3, 31)[9]), "ShearY": float(torch.linspace(0, 0.3, 31)[9]),
            "TranslateX": float(torch.linspace(0, 150 / 331 * 224, 31)[9]),
            "TranslateY": float(torch.linspace(0, 150 / 331 * 224, 31)[9]), "Rotate": 9.0,
            "Brightness": float(torch.linspace(0, 0.9, 31)[9]), "Color": float(torch.linspace(0, 0.9, 31)[9]),
            "Contrast": float(torch.linspace(0, 0.9, 31)[9]), "Sharpness": float(torch.linspace(0, 0.9, 31)[9])}
    for name, v in want.items():
        assert seen[name] == {v, -v}, name  # both signs are drawn
    assert seen["Posterize"] == {7.0} and seen["Solarize"] == {178.5}
    assert seen["Identity"] == seen["AutoContrast"] == seen["Equalize"] == {0.0}
    assert abs(want["ShearX"] - 0.09) < 1e-7 and abs(want["TranslateX"] - 9 / 30 * 150 / 331 * 224) < 1e-4
    # a non-square size: the width scales TranslateX, the height TranslateY
    space = RandAugment().space(100, 50)
    assert float(space["TranslateX"][0][30]) == float(torch.linspace(0, 150 / 331 * 100, 31)[30])
    assert float(space["TranslateY"][0][30]) == float(torch.linspace(0, 150 / 331 * 50, 31)[30])


def test_trivialaugmentwide_tables():
    from clipmi.images import TrivialAugmentWide
    space = TrivialAugmentWide().space(224, 224)
    assert list(space) == E.POLICY_OPS
    post = space["Posterize"][0].tolist()
    assert post[0] == 8 and min(post) == post[-1] == 2 and sorted(post, reverse=True) == post
    assert float(space["ShearX"][0][-1]) == float(np.float32(0.99)) and float(space["TranslateY"][0][-1]) == 32.0
    assert float(space["Rotate"][0][-1]) == 135.0 and float(space["Sharpness"][0][-1]) == float(np.float32(0.99))
    assert space["Solarize"][0].tolist()[::30] == [255.0, 0.0]
    assert [name for name, (t, s) in space.items() if s] == SIGNED
    assert [name for name, (t, s) in space.items() if t is not None] == TABLED
    progs = TrivialAugmentWide().sample(600, 224, torch.Generator().manual_seed(1))
    assert all(len(p) == 1 for p in progs)
    bits = {m for (name, m), in progs if name == "Posterize"}
    assert bits <= {2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0} and len(bits) > 3
    assert len({m for (name, m), in progs if name == "Rotate"}) > 10, "the magnitude is drawn, not fixed"


@pytest.mark.parametrize("which", ["RandAugment", "TrivialAugmentWide"])
def test_samplers_reproducible_unsigned_and_draw_order(which):
    import clipmi.images as I
    sampler = getattr(I, which)()
    a = sampler.sample(64, (48, 32), torch.Generator().manual_seed(7))
    b = sampler.sample(64, (48, 32), torch.Generator().manual_seed(7))
    c = sampler.sample(64, (48, 32), torch.Generator().manual_seed(8))
    assert a == b != c
    for name, m in (op for p in a for op in p):
        if name not in SIGNED:
            assert m >= 0 and not math.copysign(1, m) < 0, (name, m)
    # the draws, replayed: randint(14) for the op; TrivialAugmentWide only, for an op with a table, randint(bins) for
    # the magnitude; for a signed op randint(2), where 1 negates
    g = torch.Generator().manual_seed(7)
    space = sampler.space(48, 32)
    for prog in a:
        for name, m in prog:
            assert name == I.POLICY_OPS[int(torch.randint(14, (1,), generator=g))]
            table = space[name][0]
            idx = 9
            if which == "TrivialAugmentWide" and name in TABLED:
                idx = int(torch.randint(31, (1,), dtype=torch.long, generator=g))
            want = float(table[idx]) if name in TABLED else 0.0
            if name in SIGNED and int(torch.randint(2, (1,), generator=g)):
                want = -want
            assert m == want, (name, m, want)
    used = torch.Generator().manual_seed(7)
    sampler.sample(64, (48, 32), used)
    assert torch.equal(used.get_state(), g.get_state()), "sample drew more or fewer numbers than the algorithm states"


def test_samplers_reject_bad_arguments():
    from clipmi.images import RandAugment, TrivialAugmentWide
    for bad in (dict(interpolation="bicubic"), dict(fill=256), dict(fill=(1, 2)), dict(num_magnitude_bins=1)):
        with pytest.raises(ValueError):
            RandAugment(**bad)
        with pytest.raises(ValueError):
            TrivialAugmentWide(**bad)
    for bad in (dict(magnitude=31), dict(magnitude=-1), dict(num_ops=-1)):
        with pytest.raises(ValueError):
            RandAugment(**bad)
    assert RandAugment(fill=None).fill is None and RandAugment(num_ops=0).sample(2, 8) == [[], []]


# ------------------------------------------------------------------------------------------------ batch and augment
def small_batch():
    from clipmi.images import ImageBatch
    rng = np.random.default_rng(1)
    return ImageBatch.pack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(40, 50), (33, 21), (64, 64)]])


def test_image_batch_carries_and_validates_policy():
    from clipmi.images import AffineItem, ColorItem
    batch = small_batch()
    progs = [[("Rotate", 9.0), ("Equalize", 0.0)], [], [("Posterize", 7)]]
    assert batch.policy is None
    b = batch.with_policy(progs, "bilinear", (1, 2, 3))
    assert b.policy == ([[("Rotate", 9.0), ("Equalize", 0.0)], [], [("Posterize", 7.0)]], "bilinear", (1, 2, 3))
    assert batch.policy is None and batch.with_policy(progs).policy[1:] == ("nearest", 0)
    for moved in (b.to("cpu"), b.with_flips([1, 0, 1]), b.with_mode("square"), b.with_color([ColorItem.of([])] * 3),
                  b.with_affine([AffineItem.of([1, 0, 0, 0, 1, 0])] * 3), b.with_boxes(b.boxes)):
        assert moved.policy == b.policy  # _like carries the programs
    assert b.with_policy(None).policy is None
    for bad in (progs[:2], [[("Invert", 0.0)], [], []], [[("Rotate",)], [], []], [["Rotate"], [], []]):
        with pytest.raises(ValueError):
            batch.with_policy(bad)
    with pytest.raises(ValueError):
        batch.with_policy(progs, "bicubic")
    with pytest.raises(ValueError):
        batch.with_policy(progs, fill=300)


def test_train_augment_policy_keeps_boxes_flips_colour_and_affine():
    from clipmi.images import ColorJitter, RandAugment, RandomAffine, TrainAugment, TrivialAugmentWide
    batch = small_batch()
    jitter = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, grayscale_p=0.2)
    kw = dict(seed=5, color=ColorJitter(**jitter), affine=RandomAffine(15, (0.1, 0.1), (0.9, 1.1), 10), image_size=48)
    a = TrainAugment(**kw)(batch)
    b = TrainAugment(policy=RandAugment(interpolation="bilinear", fill=(4, 5, 6)), **kw)(batch)
    assert a.boxes == b.boxes and a.flips == b.flips and a.mode == b.mode == "square"
    assert [bytes(x) for x in a.color] == [bytes(x) for x in b.color]
    assert [bytes(x) for x in a.affine] == [bytes(x) for x in b.affine]
    assert a.policy is None and len(b.policy[0]) == 3 and all(len(p) == 2 for p in b.policy[0])
    assert b.policy[1:] == ("bilinear", (4, 5, 6))
    # the programs are drawn last, from the same generator
    ref = TrainAugment(**kw)
    ref(batch)
    assert b.policy[0] == RandAugment().sample(3, 48, ref.generator)
    # the size may come with the call (the trainer passes the model's)
    taw = TrainAugment(seed=5, policy=TrivialAugmentWide())
    assert len(taw(batch, image_size=32).policy[0]) == 3
    with pytest.raises(ValueError, match="image_size"):
        taw(batch)
    with pytest.raises(ValueError):
        TrainAugment(policy="randaugment")


def test_policy_calls_are_bounded_per_stage():
    from clipmi.images import AffineItem, ColorItem, EnhanceItem, policy_calls
    progs = [[("Rotate", 9.0), ("Equalize", 0.0)], [], [("Posterize", 7.0)], [("Brightness", -0.3), ("ShearX", 0.1)],
             [("Identity", 0.0), ("Identity", 0.0), ("Color", 0.2)]]
    calls = policy_calls(progs, 32, 32, "bilinear", (1, 2, 3))
    assert [k for k, _ in calls] == ["affine", "enhance", "color", "affine", "enhance", "color"]
    assert all(len(items) == 5 for _, items in calls)
    aff, enh, col = (items for _, items in calls[:3])
    assert all(isinstance(x, AffineItem) for x in aff) and [x.is_identity() for x in aff] == [False, True, True, True, True]
    assert aff[0].filter == 1 and aff[0].fill == 0x010203
    assert all(isinstance(x, EnhanceItem) for x in enh) and [x.name for x in enh] == ["none", "none", "posterize", "none", "none"]
    assert enh[2].value == 7.0
    assert all(isinstance(x, ColorItem) for x in col) and [x.ops() for x in col][3] == [("brightness", float(np.float32(0.7)))]
    assert [x.ops() for x in col][:3] == [[], [], []]
    assert policy_calls([[], []], 8, 8) == [] and policy_calls([[("Identity", 0.0)]], 8, 8) == []


# ------------------------------------------------------------------------------------------------ C ABI validation
def _table(items):
    from clipmi.images import EnhanceItem
    return (EnhanceItem * max(len(items), 1))(*[EnhanceItem(op, v) for op, v in items])


def _call(items, H=8, W=8, ws_bytes=1 << 40, B=None, src=4096, dst=1 << 30, ws=8192, table=True):
    """clipmi_enhance_u8 with fake device pointers (validation rejects before any launch) -> (status, message)."""
    from clipmi import _lib
    L = _lib.lib()
    st = L.clipmi_enhance_u8(None, src, dst, _table(items) if table else None, len(items) if B is None else B, H, W,
                             ws, ws_bytes)
    return st, L.clipmi_last_error().decode()


def _ws(items, H=8, W=8, B=None):
    from clipmi import _lib
    L = _lib.lib()
    nb = int(L.clipmi_enhance_u8_ws(_table(items), len(items) if B is None else B, H, W))
    return nb, L.clipmi_last_error().decode()


GOOD = [(0, 0.0), (1, 4.0), (2, 178.5), (3, 0.0), (4, 0.0), (5, 1.9)]


def test_version_and_struct_layout():
    from clipmi import _lib
    from clipmi.images import ENHANCE_OPS, EnhanceItem
    assert _lib.lib().clipmi_version() >= 13  # 12: before clipmi_enhance_u8
    assert ctypes.sizeof(EnhanceItem) == 8
    with open(os.path.join(REPO, "include", "clipmi.h")) as f:
        body = re.search(r"typedef struct clipmi_enhance_item \{(.*?)\} clipmi_enhance_item;", f.read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [d.split() for d in body.split(";") if d.strip()] == [["int32_t", "op"], ["float", "value"]]
    assert [(n, getattr(EnhanceItem, n).offset) for n, _ in EnhanceItem._fields_] == [("op", 0), ("value", 4)]
    assert ENHANCE_OPS == E.OPS
    it = EnhanceItem.of("solarize", 178.5)
    assert (it.op, it.value, it.name) == (2, 178.5, "solarize") and EnhanceItem.of("equalize").value == 0.0
    with pytest.raises(ValueError):
        EnhanceItem.of("invert")


@pytest.mark.parametrize("bad", [(6, 0.0), (-1, 0.0), (1, 0.0), (1, 9.0), (1, 4.5), (1, -1.0), (1, float("nan")),
                                 (2, float("inf")), (0, float("nan")), (3, float("-inf")), (5, -0.5),
                                 (5, float("nan"))], ids=str)
def test_bad_item_is_rejected_with_its_index(bad):
    from clipmi import _lib
    st, msg = _call(GOOD + [bad])
    assert st == -1 and "item 6" in msg and "clipmi_enhance_u8" in msg, msg
    with pytest.raises(ValueError):
        _lib.check(st, "clipmi_enhance_u8")
    nb, msg = _ws(GOOD + [bad])
    assert nb == -1 and "item 6" in msg and "clipmi_enhance_u8_ws" in msg, msg


def test_good_items_pass_validation_and_fail_on_the_workspace():
    nb, msg = _ws(GOOD)
    assert nb >= 6 * 8 + 6 * 768 * 4, msg        # the records and the histogram table
    no_hist = [it for it in GOOD if it[0] not in (3, 4)]
    assert 0 < _ws(no_hist)[0] < 768             # no table without an autocontrast or an equalize
    for items in (GOOD, no_hist, [(1, 1.0)], [(1, 8.0)], [(2, -5.0)], [(5, 0.0)]):
        nb = _ws(items)[0]
        assert nb > 0
        st, msg = _call(items, ws_bytes=nb - 1)
        assert st == -1 and "workspace" in msg and "clipmi_enhance_u8" in msg, msg
        st, msg = _call(items, ws=8200)          # 8-byte aligned only
        assert st == -1 and "aligned" in msg, msg


def test_geometry_pointers_overlap_and_empty_batch():
    for H, W in ((0, 8), (8, 0), (8, -1), (4097, 4096), (1, (1 << 24) + 1)):
        st, msg = _call(GOOD, H, W)
        assert st == -1 and "clipmi_enhance_u8" in msg, (H, W, msg)
        nb, msg = _ws(GOOD, H, W)
        assert nb == -1 and "clipmi_enhance_u8_ws" in msg, (H, W, msg)
    assert _ws(GOOD, 4096, 4096)[0] > 0 and _ws(GOOD, 1, 1 << 24)[0] > 0
    for B in (-1, 65536):
        items = [(0, 0.0)] * max(B, 1)
        st, msg = _call(items, 1, 1, B=B)
        assert st == -1 and "clipmi_enhance_u8" in msg and "B" in msg, msg
        assert _ws(items, 1, 1, B=B)[0] == -1
    assert _ws([(0, 0.0)] * 65535, 1, 1)[0] > 0
    for kw in (dict(src=0), dict(dst=0), dict(ws=0), dict(table=False)):
        st, msg = _call(GOOD, **kw)
        assert st == -1 and "clipmi_enhance_u8" in msg, (kw, msg)
    n = 6 * 8 * 8 * 3
    for src, dst in ((4096, 4096), (4096, 4096 + n - 1), (4096 + n - 1, 4096), (4096, 4097)):
        st, msg = _call(GOOD, src=src, dst=dst)
        assert st == -1 and "overlap" in msg and "clipmi_enhance_u8" in msg, (src, dst, msg)
    for src, dst in ((4096, 4096 + n), (4096 + n, 4096)):  # adjacent: validation passes, the workspace check stops it
        st, msg = _call(GOOD, src=src, dst=dst, ws_bytes=0)
        assert st == -1 and "workspace" in msg, msg
    assert _call([], B=0)[0] == 0 and _ws([])[0] == 0
    assert _call([], B=0, src=0, dst=0, ws=0, ws_bytes=0)[0] == 0
