"""Affine / rotation augmentation without a GPU: tests/affine_ref.py (the arithmetic csrc/affine.hip is held to, bit
for bit, in tests/test_gpu_affine.py) pinned to PIL's Image.transform and Image.rotate; the two matrix builders; the
RandomAffine / RandomRotation samplers; ImageBatch and TrainAugment carrying the records; clipmi_affine_u8's host-side
validation through the C ABI (it rejects before any launch: pointers are never dereferenced); the struct layout."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import affine_ref as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (2, 3), (5, 7), (31, 33), (48, 48), (224, 224)]
ANGLES = [0, 90, 180, 270, -90, 45, 30.5, 359.9, 1e-7]
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


def pil():
    return pytest.importorskip("PIL.Image")


def random_image(h, w, seed=None):
    return np.random.default_rng(h * 1000 + w if seed is None else seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def matrix_families(h, w, seed=0):
    """{family: [matrix]} for an h x w image; every sampling path is taken (asserted by the caller)."""
    rng = np.random.default_rng(seed + 31 * h + w)
    fam = {
        "identity": [IDENTITY],
        "integer_shift": [[1, 0, 2, 0, 1, 0], [1, 0, -1, 0, 1, 3], [1, 0, 0, 0, 1, -2], [1, 0, w - 1, 0, 1, h - 1]],
        "half_pixel_shift": [[1, 0, 0.5, 0, 1, 0], [1, 0, 0, 0, 1, 0.5], [1, 0, -0.5, 0, 1, 1.5], [1, 0, 0.5, 0, 1, -0.5]],
        "axis_scale": [[0.7, 0, 0.3, 0, 1.3, -0.2], [1.1, 0, -0.6, 0, 0.9, 0.4], [-1, 0, w, 0, 1, 0], [1, 0, 0, 0, -1, h],
                       [-0.8, 0, 0.9 * w, 0, 1.25, -0.1 * h], [1 / 3, 0, 0.1, 0, 3.0, -h], [0, 0, 0.5, 0, 0, 0.5],
                       [0.1, 0, -0.05, 0, 0.3, -0.15], [0.9, 0, -0.45, 0, 1.1, -0.55]],  # running sums that pass integers
        "rotate_scale_shear": [A.affine_matrix(rng.uniform(-180, 180), (rng.uniform(-0.2, 0.2) * w, rng.uniform(-0.2, 0.2) * h),
                                               rng.uniform(0.6, 1.6), (rng.uniform(-25, 25), rng.uniform(-25, 25)), w, h)
                               for _ in range(6)] + [A.rotation_matrix(a, w, h) for a in (90, 45, 1e-7)],
        "all_outside": [[1, 0, 5000, 0, 1, 0], [0.5, 0.1, 0, 0.1, 0.5, -3000], [1, 0, 0, 0, 1, 4096 + h]],
    }
    return {k: [[float(v) for v in m] for m in ms] for k, ms in fam.items()}


def pil_transform(Image, img, m, filt, fill):
    h, w, _ = img.shape
    resample = Image.BILINEAR if filt == A.BILINEAR else Image.NEAREST
    return np.asarray(Image.fromarray(img).transform((w, h), Image.AFFINE, m, resample, fillcolor=tuple(A.fill_rgb(fill))))


# ------------------------------------------------------------------------------------------------ restatement vs PIL
@pytest.mark.parametrize("hw", SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_restatement_matches_pil_transform(hw):
    Image = pil()
    h, w = hw
    img = random_image(h, w)
    fams = matrix_families(h, w)
    if h == 224:  # one large size: one matrix per family
        fams = {k: ms[-1:] for k, ms in fams.items()}
    paths = set()
    for name, ms in fams.items():
        for k, m in enumerate(ms):
            for filt in (A.NEAREST, A.BILINEAR):
                fill = (0x0, 0x7F30C8, 0xFFFFFF)[(k + filt) % 3]
                ref, got = pil_transform(Image, img, m, filt, fill), A.transform(img, m, filt, fill)
                paths.add(A.path_of(m, filt))
                assert np.array_equal(got, ref), (name, m, filt, np.argwhere(got != ref)[:4].tolist())
                if name == "identity":
                    assert np.array_equal(got, img)
                if name == "all_outside":
                    assert (got == A.fill_rgb(fill)).all()
    assert paths == {"bilinear", "fixed", "scale"}


def test_closed_form_table_and_fused_coefficients_would_differ():
    """The tests discriminate: the column table from a2 + a0 (x + 0.5) instead of the running sum, and a bilinear
    source coordinate with one rounding less, both change bytes somewhere in a modest search."""
    diff_tab = 0
    for k in range(1, 31):  # steps of k / 10 from 0: the sums pass integers, where the accumulated rounding shows
        a = k / 10
        c = -(a * 0.5)
        closed = np.array([-1 if c + a * (x + 0.5) < 0 else int(c + a * (x + 0.5)) for x in range(224)])
        diff_tab += int((closed != A.scale_table(c, a, 224)).sum())
    assert diff_tab > 0
    x = np.arange(224, dtype=np.float64) + 0.5
    m = A.affine_matrix(30.0, (3, -2), 1.0, (0.0, 0.0), 224, 224)
    diff = 0
    for y in range(224):  # exact (long double) then rounded once vs rounded per operation
        two = (np.float64(m[0]) * x + np.float64(m[1]) * (y + 0.5)) + np.float64(m[2])
        one = (np.longdouble(m[0]) * x + np.longdouble(m[1]) * (y + 0.5) + np.longdouble(m[2])).astype(np.float64)
        diff += int((two != one).sum())
    assert diff > 0


@pytest.mark.parametrize("hw", [(31, 31), (48, 48), (31, 33), (40, 24)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_rotation_matrix_matches_pil_rotate(hw):
    """Image.rotate takes transpose shortcuts at 0 / 180 and, for squares, 90 / 270: the matrix path gives the same
    bytes."""
    from clipmi.images import rotation_matrix
    Image = pil()
    h, w = hw
    img = random_image(h, w)
    for angle in ANGLES:
        m = rotation_matrix(angle, w, h)
        assert m == A.rotation_matrix(angle, w, h)
        for filt, resample in ((A.NEAREST, Image.NEAREST), (A.BILINEAR, Image.BILINEAR)):
            ref = np.asarray(Image.fromarray(img).rotate(angle, resample, fillcolor=(9, 200, 77)))
            got = A.transform(img, m, filt, 0x09C84D)
            assert np.array_equal(got, ref), (angle, filt, np.argwhere(got != ref)[:4].tolist())
    m = rotation_matrix(33.0, w, h, center=(3.5, 7.25))
    ref = np.asarray(Image.fromarray(img).rotate(33.0, Image.BILINEAR, center=(3.5, 7.25), fillcolor=(1, 2, 3)))
    assert np.array_equal(A.transform(img, m, A.BILINEAR, 0x010203), ref)


# ------------------------------------------------------------------------------------------------ matrix builders
def test_affine_matrix_identity_and_rotation():
    from clipmi.images import affine_matrix, rotation_matrix
    for w, h in [(1, 1), (7, 5), (224, 224), (33, 31)]:
        assert affine_matrix(0.0, (0, 0), 1.0, (0.0, 0.0), w, h) == IDENTITY
        assert affine_matrix(w=w, h=h) == IDENTITY
        for a in (0, 15, -15, 90, 123.4, -179, 1e-7):
            got, ref = affine_matrix(angle=a, w=w, h=h), rotation_matrix(-a, w, h)
            assert np.abs(np.array(got) - np.array(ref)).max() <= 1e-12, (w, h, a, got, ref)
    args = (12.5, (3, -2), 1.1, (5.0, -7.0), 48, 32)
    assert affine_matrix(*args) == A.affine_matrix(*args)
    assert affine_matrix(*args, center=(10, 11)) == A.affine_matrix(*args, center=(10, 11))


def test_affine_matrix_inverts_the_forward_matrix():
    from clipmi.images import affine_matrix
    rng = np.random.default_rng(2)

    def T(tx, ty):
        return np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float64)

    for _ in range(50):
        w, h = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        angle, scale = rng.uniform(-180, 180), rng.uniform(0.5, 2.0)
        tx, ty = rng.uniform(-30, 30), rng.uniform(-30, 30)
        shx, shy = rng.uniform(-40, 40), rng.uniform(-40, 40)
        rot, sx, sy = math.radians(angle), math.radians(shx), math.radians(shy)
        R = np.array([[math.cos(rot), -math.sin(rot), 0], [math.sin(rot), math.cos(rot), 0], [0, 0, 1]])
        shear_y = np.array([[1, 0, 0], [-math.tan(sy), 1, 0], [0, 0, 1]])
        shear_x = np.array([[1, -math.tan(sx), 0], [0, 1, 0], [0, 0, 1]])
        S = np.diag([scale, scale, 1.0])
        cx, cy = w * 0.5, h * 0.5
        forward = T(tx, ty) @ T(cx, cy) @ R @ shear_y @ shear_x @ S @ T(-cx, -cy)
        inv = np.array(affine_matrix(angle, (tx, ty), scale, (shx, shy), w, h) + [0, 0, 1]).reshape(3, 3)
        assert np.abs(inv @ forward - np.eye(3)).max() <= 1e-9


# ------------------------------------------------------------------------------------------------ samplers
def _draws(sampler, B, size, seed=0):
    """The number of uniforms ``sample`` consumed: the position of the generator afterwards, found by matching the
    next value against a fresh stream."""
    g = torch.Generator().manual_seed(seed)
    items = sampler.sample(B, size, g)
    nxt = float(torch.rand((), generator=g))
    ref = torch.Generator().manual_seed(seed)
    for n in range(64 * max(B, 1) + 1):
        if float(torch.rand((), generator=ref)) == nxt:
            return items, n
    raise AssertionError("the generator's position was not found")


def test_samplers_are_reproducible_and_in_range():
    from clipmi.images import AffineItem, RandomAffine, RandomRotation, affine_matrix, rotation_matrix
    ra = RandomAffine(15, (0.1, 0.2), (0.9, 1.1), (-10, 10, 0, 5), interpolation="bilinear", fill=(1, 2, 3))
    a = ra.sample(16, (48, 32), torch.Generator().manual_seed(7))
    b = ra.sample(16, (48, 32), torch.Generator().manual_seed(7))
    c = ra.sample(16, (48, 32), torch.Generator().manual_seed(8))
    assert [it.matrix for it in a] == [it.matrix for it in b] != [it.matrix for it in c]
    assert all(isinstance(it, AffineItem) and it.filter == 1 and it.fill == 0x010203 for it in a)
    g = torch.Generator().manual_seed(7)
    for it in a:  # the records are get_params' draws through affine_matrix, in get_params' order
        angle, (tx, ty), scale, (shx, shy) = ra.params(48, 32, g)
        assert -15 <= angle <= 15 and abs(tx) <= 5 and abs(ty) <= 6 and tx == int(tx) and ty == int(ty)
        assert 0.9 <= scale <= 1.1 and -10 <= shx <= 10 and 0 <= shy <= 5
        assert it.matrix == affine_matrix(angle, (tx, ty), scale, (shx, shy), 48, 32)
    g = torch.Generator().manual_seed(7)  # the draw order, spelled out
    u = [float(torch.rand((), generator=g)) for _ in range(6)]
    first = affine_matrix(-15 + 30 * u[0], (int(round(-4.8 + 9.6 * u[1])), int(round(-6.4 + 12.8 * u[2]))),
                          0.9 + (1.1 - 0.9) * u[3], (-10 + 20 * u[4], 0 + 5 * u[5]), 48, 32)
    assert a[0].matrix == first
    rr = RandomRotation((10, 20), fill=7)
    r = rr.sample(8, 31, torch.Generator().manual_seed(1))
    g = torch.Generator().manual_seed(1)
    for it in r:
        angle = 10 + 10 * float(torch.rand((), generator=g))
        assert it.matrix == rotation_matrix(angle, 31, 31) and it.filter == 0 and it.fill == 0x070707
    assert RandomAffine(0).sample(3, 9)[0].is_identity()


def test_sampler_draw_counts():
    from clipmi.images import RandomAffine, RandomRotation
    assert _draws(RandomAffine(10), 5, 32)[1] == 5                                     # the angle alone
    assert _draws(RandomAffine(10, (0.1, 0.1)), 5, 32)[1] == 15                        # + tx, ty
    assert _draws(RandomAffine(10, (0.1, 0.1), (0.9, 1.1)), 5, 32)[1] == 20            # + scale
    assert _draws(RandomAffine(10, (0.1, 0.1), (0.9, 1.1), 10), 5, 32)[1] == 25        # + shear_x
    assert _draws(RandomAffine(10, None, None, (0, 1, 2, 3)), 5, 32)[1] == 15          # angle, shear_x, shear_y
    assert _draws(RandomRotation(10), 5, 32)[1] == 5
    assert _draws(RandomRotation(10, p=1.0), 5, 32)[1] == 5                            # p == 1: no coin
    items, n = _draws(RandomRotation(10, p=0.0), 5, 32)
    assert n == 5 and all(it.is_identity() for it in items)                            # the coin alone
    items, n = _draws(RandomAffine(10, (0.1, 0.1), (0.9, 1.1), 10, p=0.5), 40, 32, seed=3)
    skipped = sum(it.is_identity() for it in items)
    assert 0 < skipped < 40 and n == 40 + 5 * (40 - skipped)                           # a skipped image draws nothing more
    g = torch.Generator().manual_seed(3)
    assert items[0].is_identity() == (not float(torch.rand((), generator=g)) < 0.5)     # the coin comes first


@pytest.mark.parametrize("bad", [dict(degrees=-1), dict(degrees=(1, 2, 3)), dict(degrees="x"), dict(degrees=float("nan")),
                                 dict(translate=(0.1,)), dict(translate=(0.1, 1.5)), dict(translate=(-0.1, 0.1)),
                                 dict(translate=0.1), dict(scale=(0, 1)), dict(scale=(-1, 1)), dict(scale=1.0),
                                 dict(scale=(1, 2, 3)), dict(shear=-5), dict(shear=(1, 2, 3)), dict(shear="x"),
                                 dict(interpolation="bicubic"), dict(fill=256), dict(fill=(1, 2)), dict(fill=-1),
                                 dict(fill=1.5), dict(center=(1,)), dict(p=1.5), dict(p=-0.1)])
def test_samplers_reject_bad_arguments(bad):
    from clipmi.images import RandomAffine, RandomRotation
    with pytest.raises(ValueError):
        RandomAffine(**dict(dict(degrees=10), **bad))
    if set(bad) <= {"degrees", "interpolation", "fill", "center", "p"}:
        with pytest.raises(ValueError):
            RandomRotation(**dict(dict(degrees=10), **bad))


def test_random_rotation_has_no_expand():
    from clipmi.images import RandomRotation
    with pytest.raises(TypeError):
        RandomRotation(10, expand=True)


def test_affine_item_of():
    from clipmi.images import AffineItem
    it = AffineItem.of([1, 2, 3, 4, 5, 6], "bilinear", (1, 2, 255))
    assert (it.matrix, it.filter, it.fill, it.interpolation) == ([1.0, 2.0, 3.0, 4.0, 5.0, 6.0], 1, 0x0102FF, "bilinear")
    assert AffineItem.of(IDENTITY).is_identity() and AffineItem.of(IDENTITY, fill=128).fill == 0x808080
    for bad in (dict(matrix=[1, 0, 0]), dict(interpolation="cubic"), dict(fill=(1, 2, 300)), dict(fill="red")):
        with pytest.raises(ValueError):
            AffineItem.of(**dict(dict(matrix=IDENTITY), **bad))


# ------------------------------------------------------------------------------------------------ batch and augment
def small_batch():
    from clipmi.images import ImageBatch
    rng = np.random.default_rng(1)
    return ImageBatch.pack([rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(40, 50), (33, 21), (64, 64)]])


def test_image_batch_carries_and_validates_affine():
    from clipmi.images import AffineItem, ColorItem
    batch = small_batch()
    items = [AffineItem.of(IDENTITY), AffineItem.of([1, 0, 2, 0, 1, 0], "bilinear"), AffineItem.of(IDENTITY, fill=3)]
    assert batch.affine is None
    b = batch.with_affine(items)
    assert b.affine == items and batch.affine is None
    for moved in (b.to("cpu"), b.with_flips([1, 0, 1]), b.with_mode("square"), b.with_color([ColorItem.of([])] * 3),
                  b.with_boxes(b.boxes)):
        assert moved.affine == items  # _like carries the records
    assert b.with_affine(None).affine is None
    with pytest.raises(ValueError):
        batch.with_affine(items[:2])
    with pytest.raises(ValueError):
        batch.with_affine([IDENTITY] * 3)


def test_train_augment_affine_keeps_boxes_flips_and_colour():
    from clipmi.images import ColorJitter, RandomAffine, RandomRotation, TrainAugment
    batch = small_batch()
    jitter = dict(brightness=0.4, contrast=0.4, saturation=0.4, hue=0.1, grayscale_p=0.2)
    plain = TrainAugment(seed=5, color=ColorJitter(**jitter))
    aff = TrainAugment(seed=5, color=ColorJitter(**jitter), affine=RandomAffine(15, (0.1, 0.1), (0.9, 1.1), 10),
                       image_size=48)
    a, b = plain(batch), aff(batch)
    assert a.boxes == b.boxes and a.flips == b.flips and a.mode == b.mode == "square"
    assert [bytes(x) for x in a.color] == [bytes(x) for x in b.color]
    assert a.affine is None and len(b.affine) == 3 and not any(it.is_identity() for it in b.affine)
    # the records are drawn last, from the same generator: a fresh sampler on a generator advanced alike gives them
    ref = TrainAugment(seed=5, color=ColorJitter(**jitter))
    ref(batch)
    want = RandomAffine(15, (0.1, 0.1), (0.9, 1.1), 10).sample(3, 48, ref.generator)
    assert [it.matrix for it in b.affine] == [it.matrix for it in want]
    # the size may come with the call (the trainer passes the model's); without one there is nothing to turn about
    rot = TrainAugment(seed=5, affine=RandomRotation(20, interpolation="bilinear"))
    assert len(rot(batch, image_size=32).affine) == 3
    with pytest.raises(ValueError, match="image_size"):
        rot(batch)
    # with affine=None the generator is where it was before
    p2, r2 = TrainAugment(seed=9), TrainAugment(seed=9)
    p2(batch), r2(batch)
    assert p2(batch).boxes == r2(batch).boxes
    with pytest.raises(ValueError):
        TrainAugment(affine="rotate")


# ------------------------------------------------------------------------------------------------ C ABI validation
def _table(ms, filters=None, fills=None):
    from clipmi.images import AffineItem
    items = []
    for k, m in enumerate(ms):
        items.append(AffineItem((ctypes.c_double * 6)(*m), 0 if filters is None else filters[k], 0 if fills is None else fills[k]))
    return (AffineItem * max(len(items), 1))(*items)


def _call(ms, H=8, W=8, ws_bytes=1 << 40, B=None, src=4096, dst=1 << 30, **kw):
    """clipmi_affine_u8 with fake device pointers (validation rejects before any launch) -> (status, message)."""
    from clipmi import _lib
    L = _lib.lib()
    st = L.clipmi_affine_u8(None, src, dst, _table(ms, **kw), len(ms) if B is None else B, H, W, 8192, ws_bytes)
    return st, L.clipmi_last_error().decode()


def _ws(ms, H=8, W=8, **kw):
    from clipmi import _lib
    L = _lib.lib()
    return int(L.clipmi_affine_u8_ws(_table(ms, **kw), len(ms), H, W)), L.clipmi_last_error().decode()


def test_version():
    from clipmi import _lib
    assert _lib.lib().clipmi_version() >= 12  # 11: before clipmi_affine_u8


ROT = [0.8, 0.6, 1.0, -0.6, 0.8, 2.0]


@pytest.mark.parametrize("bad", [dict(m=[float("nan"), 0, 0, 0, 1, 0]), dict(m=[1, 0, 0, 0, 1, float("inf")]),
                                 dict(m=[1, 0, 0, float("-inf"), 1, 0]), dict(filter=2), dict(filter=-1),
                                 dict(fill=0x1000000), dict(fill=-1),
                                 dict(m=[1, 0, 16384 - 8, 0, 1, 0]), dict(m=[1, 0, 0, 0, 1, -(16384 - 8)]),
                                 dict(m=[2048, 0, 0, 0, 1, 0]), dict(m=[1, 0, 0, 1024, 1024.5, 0])])
def test_bad_item_is_rejected_with_its_index(bad):
    from clipmi import _lib
    m = bad.get("m", ROT)
    kw = dict(filters=[0, 1, bad.get("filter", 1)], fills=[0, 0xFFFFFF, bad.get("fill", 5)])
    st, msg = _call([IDENTITY, ROT, m], **kw)
    assert st == -1 and "item 2" in msg and "clipmi_affine_u8" in msg, msg
    with pytest.raises(ValueError):
        _lib.check(st, "clipmi_affine_u8")
    nb, msg = _ws([IDENTITY, ROT, m], **kw)
    assert nb == -1 and "item 2" in msg, msg


def test_bound_is_per_row_and_scales_with_the_size():
    just_inside = [1, 0, 16384 - 8.001, 0, 1, 0]
    assert _ws([just_inside])[0] > 0 and _ws([just_inside], W=9)[0] == -1
    assert _ws([[1, 1, 0, 0, 1, 0]], 4096, 4096)[0] > 0 and _ws([[2, 2, 0, 0, 1, 0]], 4096, 4096)[0] == -1


def test_good_items_pass_validation_and_fail_on_the_workspace():
    for ms, filters in (([IDENTITY, ROT], [0, 0]), ([IDENTITY, ROT], [1, 1]), ([ROT, ROT], [0, 1])):
        nb, msg = _ws(ms, filters=filters)
        assert nb >= 2 * 64, msg
        st, msg = _call(ms, filters=filters, ws_bytes=nb - 1)
        assert st == -1 and "workspace" in msg, msg
    # the axis-aligned nearest items carry their tables: W + H entries each
    assert _ws([IDENTITY] * 3, 100, 200)[0] >= _ws([ROT] * 3, 100, 200)[0] + 3 * 300 * 4 - 256


def test_overlap_sizes_and_empty_batch():
    n = 2 * 8 * 8 * 3
    for src, dst in ((4096, 4096), (4096, 4096 + n - 1), (4096 + n - 1, 4096), (4096, 4097)):
        st, msg = _call([IDENTITY, ROT], src=src, dst=dst)
        assert st == -1 and "overlap" in msg, (src, dst, msg)
    for src, dst in ((4096, 4096 + n), (4096 + n, 4096)):  # adjacent: validation passes, the workspace check stops it
        st, msg = _call([IDENTITY, ROT], src=src, dst=dst, ws_bytes=0)
        assert st == -1 and "workspace" in msg, msg
    assert _ws([IDENTITY], 4096, 4096)[0] > 0
    for H, W in ((4097, 8), (8, 4097), (0, 8), (8, -1)):
        nb, msg = _ws([IDENTITY], H, W)
        assert nb == -1 and "4096" in msg
        assert _call([IDENTITY], H, W)[0] == -1
    assert _call([IDENTITY], B=-1)[0] == -1
    assert _call([], B=0)[0] == 0 and _ws([])[0] == 0


def test_item_struct_matches_the_header():
    from clipmi.images import AFFINE_FILTERS, AffineItem
    assert ctypes.sizeof(AffineItem) == 56
    with open(os.path.join(REPO, "include", "clipmi.h")) as f:
        body = re.search(r"typedef struct clipmi_affine_item \{(.*?)\} clipmi_affine_item;", f.read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.split() for d in body.split(";") if d.strip()]
    assert decls == [["double", "m[6]"], ["int32_t", "filter"], ["int32_t", "fill"]]
    assert [n for n, _ in AffineItem._fields_] == ["m", "filter", "fill"]
    assert [getattr(AffineItem, n).offset for n, _ in AffineItem._fields_] == [0, 48, 52]
    assert AFFINE_FILTERS == A.FILTERS == {"nearest": 0, "bilinear": 1}
