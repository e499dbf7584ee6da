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


# ------------------------------------------------------------------------------------------------ exact sums
# Preconditions of tests/test_gpu_reductions.py: every int64 reference stays below 2^24 in magnitude (worst case
# over the value range, not only the drawn values, so every partial sum does too), and each case reaches the loop
# regime it is named for -- restated from the host arithmetic, so an edited case list cannot silently lose a branch.
DTYPES = [torch.float32, torch.bfloat16]


def test_colsum_cases_exact_and_reach_their_regimes():
    cases = kc.colsum_cases()
    seen = set()
    for c in cases:
        plan = kc.colsum_plan(c.R, c.N, c.N + c.ld_pad, c.x_off)
        assert c.R * max(abs(kc.COLSUM_LO), kc.COLSUM_HI) + kc.BETA_MAX < kc.EXACT, c.id()
        assert plan["chunks"] == min(max(-(-c.R // 256), 1), 512) and plan["chunks"] * plan["rows_per"] >= c.R
        assert plan["vec"] == c.regime.startswith("vec"), c.id()
        if c.regime.endswith("unrolled"):  # both loops of the reducer run, uncapped
            assert plan["unrolled"] and plan["remainder"] and plan["rows_per"] == 256 and plan["chunks"] < 512, c.id()
        if c.regime.endswith("capped"):
            assert plan["chunks"] == 512 and plan["rows_per"] > 256 and plan["unrolled"], c.id()
        if c.R <= 257:
            assert plan["chunks"] == (1 if c.R <= 256 else 2) and not plan["unrolled"], c.id()
        seen.add((c.regime, c.beta, c.ld_pad > 0))
        seen.add(("blocks", plan["vec"], plan["col_blocks"]))
    for regime in ("vec", "vec-unrolled", "vec-capped", "scalar"):
        for beta in (0, 1):
            assert any((regime, beta, pad) in seen for pad in (False, True)), (regime, beta)
        assert (regime, 0, True) in seen or (regime, 1, True) in seen, regime  # ldx > N
    assert ("blocks", True, 2) in seen and ("blocks", False, 2) in seen  # a second column block, either kernel
    assert {c.R for c in cases} >= {1, 255, 257, 114944, 131073}
    assert {c.N for c in cases} >= {1, 4, 5, 8, 257, 1028}
    assert any(c.x_off % 4 and c.N % 4 == 0 and c.ld_pad % 4 == 0 for c in cases)  # only the pointer is off
    # the drawn inputs: equal integers in both dtypes, the reference inside the bound
    for c in (cases[0], cases[-1]):
        x32, out0, ref = kc.colsum_inputs(c, torch.float32)
        x16, _, ref16 = kc.colsum_inputs(c, torch.bfloat16)
        assert torch.equal(x32, x16.float()) and torch.equal(ref, ref16) and ref.abs().max() < kc.EXACT


def test_period_sum_cases_exact_and_reach_their_regimes():
    cases = kc.period_cases()
    for c in cases:
        assert c.nb * kc.PERIOD_MAX + kc.BETA_MAX < kc.EXACT and c.D % 4 == 0 and 1 <= c.nt <= c.period, c.id()
        plan = kc.period_plan(c.nb)
        assert sum(8 * p + t for p, t in plan) == c.nb  # every row once
        assert any(p for p, _ in plan) == (c.nb >= 29), c.id()  # the unrolled loop: b + 28 < nb for b = 0
    assert kc.period_plan(28) == [(0, 7)] * 4 and kc.period_plan(29)[0] == (1, 0)
    assert kc.period_plan(33)[0] == (1, 1) and kc.period_plan(61) == [(2, 0)] + [(1, 7)] * 3
    for nb in kc.PERIOD_NB:  # every nb with (50, 7) at D = 260, both leading dimensions and both betas
        got = {(c.ld_pad, c.beta) for c in cases if (c.nb, c.period, c.nt, c.D) == (nb, 50, 7, 260)}
        assert {p for p, _ in got} == {0, 4} and {b for _, b in got} == {0, 1}, nb
    assert {(c.period, c.nt) for c in cases} == set(kc.PERIOD_PT)
    assert {c.D for c in cases} == set(kc.PERIOD_D)
    for pt in kc.PERIOD_PT:  # each (period, nt) inside and outside the unrolled loop
        assert {c.nb >= 29 for c in cases if (c.period, c.nt) == pt} == {False, True}, pt
    assert any(c.D > 256 for c in cases)  # a second column block (64 lanes x 4 columns)
    x, out0, ref = kc.period_inputs(cases[-1], torch.bfloat16)
    assert torch.equal(x.float(), x.float().round()) and ref.abs().max() < kc.EXACT


def test_embed_bwd_cases_exact_and_reach_their_regimes():
    cases = kc.embed_bwd_cases()
    for c in cases:
        assert 2 * c.R * kc.EMBED_MAX + kc.BETA_MAX < kc.EXACT and c.D % 4 == 0, c.id()  # two calls accumulate
        if c.V == 49408:
            assert c.D == 4, c.id()
        ids = kc.embed_ids(c.V, c.R, c.pattern, 41 + c.V + c.R)
        assert ids.dtype == torch.int64 and ids.shape == (c.R,)
        valid = (ids >= 0) & (ids < c.V)
        if c.pattern == "oov":
            for bad in kc.EMBED_OOV:
                assert c.R < 3 or (ids == (c.V if bad is None else bad)).any(), c.id()
        else:
            assert valid.all(), c.id()
        if c.pattern == "equal":
            assert (ids == ids[0]).all()
        if c.pattern == "distinct":
            assert ids.unique().numel() == c.R
        if c.pattern == "ascending":
            assert (ids[1:] >= ids[:-1]).all()
        if c.pattern == "alternate":
            assert ids.unique().numel() == min(2, c.R) and (c.R < 2 or ids[0] != ids[1])
        if c.pattern == "eos_tail":
            assert (ids[-(2 * c.R) // 5:] == c.V - 1).all()
    assert {c.V for c in cases} == set(kc.EMBED_V) and {c.R for c in cases} == set(kc.EMBED_R)
    assert {c.D for c in cases} == set(kc.EMBED_D) and {c.pattern for c in cases} == set(kc.EMBED_PATTERNS)
    assert {(c.pattern, c.beta) for c in cases} == {(p, b) for p in kc.EMBED_PATTERNS for b in (0, 1)}
    # id_scan_kernel's per: one entry per thread up to V = 1024, the multi-element branch above (49 at the real V)
    assert [kc.scan_per(V) for V in kc.EMBED_V] == [1, 1, 1, 2, 49]
    for V in (1025, 49408):  # ids at and past entry 1024 occur, so a scan that stops there shows
        assert any(c.V == V and (kc.embed_ids(V, c.R, c.pattern, 41 + V + c.R) % 2 ** 40 >= 1024).any() for c in cases)
    # one id owning every 64-row chunk of several, at beta 0 and 1
    assert {c.beta for c in cases if c.pattern == "equal" and c.R == 5000} == {0, 1}
    c = next(c for c in cases if c.pattern == "oov" and c.R == 5000)
    ids, dx0, g0, ref1, ref2 = kc.embed_bwd_inputs(c, torch.bfloat16)
    assert max(ref1.abs().max(), ref2.abs().max()) < kc.EXACT and torch.equal(dx0.float(), dx0.float().round())
    for B, S, D, V in kc.EMBED_FWD_CASES:
        ids = kc.embed_fwd_ids(B, S, V, 1)
        assert (B * S) % 4 and S in (1, 77) and D % 4 == 0 and (ids == 0).any() and (ids == V - 1).any()
    assert {D for _, _, D, _ in kc.EMBED_FWD_CASES} == set(kc.EMBED_D)


def test_pool_and_rows_cases():
    for kind in kc.POOL_KINDS:
        for B in kc.ROWS_B:
            for S in kc.ROWS_S:
                ids, mode, want = kc.pool_inputs(kind, B, S, B + S)
                assert ids.shape == (B, S) and want.dtype == torch.int32 and (0 <= want).all() and (want < S).all()
                if kind == "no_eos":
                    assert mode == 1 and not (ids == kc.POOL_EOS).any() and (want == 0).all()
                if kind == "several_eos":
                    hits = ids == kc.POOL_EOS
                    assert mode == 1 and hits.any(1).all() and (S == 1 or hits.sum(1).max() > 1)
                    for b in range(B):
                        assert hits[b, want[b]] and not hits[b, :want[b]].any()
                if kind == "tied_max":
                    top = ids == ids.max(1, keepdim=True).values
                    assert mode == 2 and (S == 1 or top.sum(1).max() > 1)
                    for b in range(B):
                        assert top[b, want[b]] and not top[b, :want[b]].any()
                if S > 1 and kind in ("several_eos", "tied_max"):
                    assert (want > 0).any()  # the answer is not always token 0
    cases = kc.rows_cases()
    assert {B for B, _, _ in cases} >= set(kc.ROWS_B) and {S for _, S, _ in cases} == set(kc.ROWS_S)
    for S in kc.ROWS_S:
        assert {D for _, s, D in cases if s == S} == set(kc.ROWS_D)
    assert max(B * S * D for B, S, D in cases) * 4 <= 4 << 20
    idx = kc.rows_idx(257, 77, 3)
    assert idx.dtype == torch.int32 and idx.min() == 0 and idx.max() == 76


def test_grad_norm_cases_exact_and_reach_their_regimes():
    for n in kc.GRAD_NS + kc.GRAD_MULTI_NS:
        assert kc.GRAD_MAX ** 2 * n < kc.EXACT, n
    assert kc.GRAD_MAX ** 2 * sum(kc.GRAD_MULTI_NS) < kc.EXACT
    big = max(kc.GRAD_NS)
    assert big > 1024 * 256 * 4 and kc.grad_plan(big) == (1, 1, 3)  # a full pass, a second-pass vector, a scalar tail
    assert [kc.grad_plan(n) for n in (1, 3, 4, 5, 1023)] == [(0, 0, 1), (0, 0, 3), (0, 1, 0), (0, 1, 1), (0, 255, 3)]
    assert len(kc.GRAD_MULTI_NS) == 3 and 0 in kc.GRAD_MULTI_NS and big in kc.GRAD_MULTI_NS
    g = kc.grad_tensor(1023, 5)
    assert g.abs().max() == 3 and g[0] != 0 and g[-1] != 0 and torch.equal(g, g.round())
    # the clip coefficient's contract
    assert kc.clip_expect(0, 1.0) == (0.0, 1.0) and kc.clip_expect(9, 4.0)[1] == 1.0
    assert kc.clip_expect(9, 0.0)[1] == 1.0 and kc.clip_expect(9, -1.0)[1] == 1.0
    norm, coef = kc.clip_expect(9, 1.0)
    assert norm == 3.0 and abs(coef - 1 / 3.000001) < 1e-7
    for n in kc.SUM2_NS:  # a and b in [-4, 4], scale a power of two, out0 in [-4, 4]
        assert 2 * 4 * n + kc.BETA_MAX < kc.EXACT
    assert {n > 1024 for n in kc.SUM2_NS} == {False, True}  # one pass of the 1024 threads, and a second


def test_l2norm_rows_are_exact():
    for E in kc.L2_ES:
        for entries in (1, 4):
            if E < entries:
                continue
            x, y, nrm = kc.l2norm_rows(5, E, entries, E)
            assert ((x != 0).sum(1) == entries).all()
            assert torch.equal(x.double().pow(2).sum(1).sqrt(), nrm.double())  # exact powers of two
            assert torch.equal((x.double() / nrm.double()[:, None]).float(), y)
            assert set(y.abs().unique().tolist()) <= {0.0, 1.0 if entries == 1 else 0.5}
    assert {1, 63, 64, 65} <= set(kc.L2_ES) and {1, 63, 64, 65} <= set(kc.SM_NS)  # around one wave's 64 lanes
    assert {1, 4, 5} <= set(kc.L2_BS) and {1, 4, 5} <= set(kc.SM_RS)             # around one block's 4 rows
