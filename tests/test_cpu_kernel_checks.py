"""The structured kernel tests' helpers and preconditions, checked without a GPU: the guard bands catch a write
one element outside a view, every one-hot attention case the GPU file parametrises has an fp64 softmax leak below
2^-40, and every integer GEMM case stays exact in fp32."""
import pytest
import torch

import kernel_checks as kc


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("rows,cols,ld,off", [(5, 7, None, 0), (5, 7, 9, 0), (3, 130, 133, 1), (1, 64, None, 3)])
def test_guarded_detects_out_of_bounds_writes(dtype, rows, cols, ld, off):
    view, check = kc.guarded(rows, cols, dtype, ld, off, device="cpu")
    assert view.shape == (rows, cols) and view.stride() == (ld or cols, 1)
    es = view.element_size()
    assert view.data_ptr() % 16 == (off * es) % 16
    check()
    view.copy_(torch.arange(rows * cols).reshape(rows, cols).to(dtype))  # in-bounds writes: silent
    view[rows - 1, cols - 1] = 1.0
    view[0, 0] = float("nan")
    check()
    L = ld or cols
    flat = torch.as_strided(view, (rows * L + 2,), (1,), view.storage_offset() - 1)  # from one element before
    elems = [-1, (rows - 1) * L + cols]  # one element before the view, one after it
    if L > cols:
        elems += [cols, (rows - 1) * L - 1]  # the first pad column of row 0, the last one before the last row
    for elem in elems:
        row, col = divmod(elem, L)
        bits = flat[elem + 1:elem + 2].view(torch.uint8).clone()
        flat[elem + 1] = 0.0
        with pytest.raises(AssertionError, match=rf"\(row, column\) = \({row}, {col}\)"):
            check()
        flat[elem + 1:elem + 2].view(torch.uint8).copy_(bits)  # the guard's bits back: silent again
        check()


def test_guarded_1d_and_nan_pattern():
    v, check = kc.guarded1d(33, torch.float32, device="cpu")
    assert v.shape == (33,) and torch.isnan(v).all()  # the fill is a NaN: an element nobody stores fails its compare
    v.zero_()
    check()
    torch.as_strided(v, (1,), (1,), v.storage_offset() + 33).fill_(float("nan"))  # a NaN, but not the guard's bits
    with pytest.raises(AssertionError, match=r"byte 132 .*\(1, 0\)"):  # element 33 of a row of 33
        check()


def test_integer_tensor_is_exact_and_seeded():
    a = kc.integer_tensor((50, 40), -4, 4, torch.bfloat16, 3)
    assert a.dtype == torch.bfloat16 and a.min() == -4 and a.max() == 4
    assert torch.equal(a.float(), a.float().round())
    assert torch.equal(a, kc.integer_tensor((50, 40), -4, 4, torch.bfloat16, 3))
    assert not torch.equal(a, kc.integer_tensor((50, 40), -4, 4, torch.bfloat16, 4))


def test_gemm_cases_stay_exact_in_fp32():
    cases = kc.gemm_cases()
    assert 150 <= len(cases) <= 300, len(cases)
    for c in cases:
        assert 16 * c.K < 2 ** 24 and c.bound() < 2 ** 24, c.id()
    # every epilogue meets every alignment class, every layout x variant a ragged shape
    for (flags, bias, alpha) in kc.EXACT_EPILOGUES:
        seen = {c.cls for c in cases if (c.flags, c.bias, c.alpha) == (flags, bias, alpha) and c.split == 1}
        assert {"vec8", "vec", "scalar"} <= seen, (flags, bias, alpha, seen)
    ragged = {(c.akm, c.bkm, c.small) for c in cases if c.ab == "bf16" and (c.M % 128 or c.N % 128)}
    for (akm, bkm) in kc.LAYOUTS:
        want = [0, 1, 4, 11] + ([9, 28, 32] if akm else []) + ([28] if not akm and not bkm else [])
        for v in want:
            assert (akm, bkm, v) in ragged, (akm, bkm, v)


@pytest.mark.parametrize("N,mask", kc.attn_cases())
def test_onehot_leak_below_2_pow_minus_40(N, mask):
    """A precondition on the inputs, not a tolerance: with it the softmax of every query is its selected key to
    fp32 precision, whatever the order of summation."""
    for family in kc.attn_families(N, mask):
        case = kc.attn_onehot_case(N, mask, family)
        assert case["leak"] < kc.LEAK_MAX, (family, case["leak"])
        B, H, pi = case["B"], case["H"], case["pi"]
        cnt = kc.attn_allowed_count(B, N, case["lens"], case["causal"])
        assert (pi >= 0).all() and (pi < cnt).all(), family  # the selected key is allowed for every query
        q, k, v = case["qkv"].view(B, N, 3, H, 64).unbind(2)
        for t in (q, k, v):  # exact in bf16
            assert torch.equal(t.bfloat16().float(), t)
        if case["decoy"] is None:
            assert torch.equal(case["sel"], torch.full_like(case["sel"], 8.0 * case["c"]))
        else:  # the decoy key scores exactly what the selected key scores: leaking it halves the weight
            d = case["decoy"]
            assert (d < 0).logical_or(d >= cnt).all(), family  # masked for its query
            kk = k.permute(0, 2, 1, 3)  # [B, H, N, 64]
            kd = torch.gather(kk, 2, d.clamp_min(0)[:, None, :, None].expand(B, H, N, 64))
            sd = (q.permute(0, 2, 1, 3) * kd).sum(-1).double() / 8.0
            has = (d >= 0)[:, None, :].expand(B, H, N)
            assert torch.equal(sd[has], case["sel"][has]) and has.any()


def test_onehot_known_leaks():
    """The construction at the sizes it was designed at: c = 16 keeps the leak of a random map many orders below
    2^-40 at N = 4096 and N = 577, c = 32 with a same-strength decoy at key i + 1 under the causal mask at N = 577."""
    assert kc.attn_onehot_case(4096, "none", "random")["leak"] < 1e-15
    assert kc.attn_onehot_case(577, "none", "random")["leak"] < 1e-20
    assert kc.attn_onehot_case(577, "causal", "ident+decoy_next")["leak"] < 1e-15


def test_ln_leading_dims_differ():
    for D in kc.LN_WIDTHS:
        for strided in (("vec", "odd") if kc.ln_fast_width(D) else ("odd",)):
            lds = kc.ln_leading_dims(D, strided)
            assert len(set(lds)) == 5 and min(lds) > D
            assert all(ld % 4 == 0 for ld in lds) if strided == "vec" else any(ld % 2 for ld in lds)
        assert kc.ln_leading_dims(D, False) == [D] * 5
