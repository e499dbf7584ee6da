"""Structured-input and guard-band tests of the GEMM, attention and LayerNorm kernels (helpers and case lists:
tests/kernel_checks.py; their preconditions: tests/test_cpu_kernel_checks.py).

Inputs are built so that the expected result is exact or nearly so -- integer GEMM operands, one-hot and uniform
attention -- and every output lives inside a guard band, checked bitwise after the kernel has finished."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_checks as kc  # noqa: E402
from kernel_checks import guarded, guarded1d, integer_tensor  # noqa: E402

from clipmi import kernels as kern  # noqa: E402
from clipmi import towers as T  # noqa: E402
from clipmi._lib import BF16, F32  # noqa: E402

DT = {torch.bfloat16: BF16, torch.float32: F32}
TD = {"bf16": torch.bfloat16, "f32": torch.float32, "x3": torch.float32}
TOL = {torch.bfloat16: 3e-2, torch.float32: 2e-5}  # the max/max bounds of tests/test_gpu_kernels.py


def _filled(rows, cols, dtype, values, ld=None, off=0):
    """values in a guarded [rows, cols] view: an input whose pad columns read as NaN, or an output to add onto."""
    view, check = guarded(rows, cols, dtype, ld, off)
    view.copy_(values)
    return view, check


# =============================================================================================== A. GEMM
GEMM_CASES = kc.gemm_cases()


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c.id() for c in GEMM_CASES])
def test_gemm_integer_operands_exact(case):
    """Operands, bias, residual, old C and the aux factor are integers in [-4, 4], so every value up to the output
    rounding is exact in fp32 (kernel_checks.GemmCase.bound < 2^24): fp32 C must equal the fp64 result bit for bit
    and bf16 C the result rounded to nearest even.  Only quick_gelu is inexact: there aux (the pre-activation) is
    compared exactly and C with the 3e-2 bound of test_gemm_epilogues.  The id's suffix names the epilogue's
    alignment class (vec8: 16-byte bf16 rows; vec: 4-column vectors, epilogue256 on the 256-tile kernels;
    vec+ragged: vectors but for a last group of nv < 4 columns; scalar: odd leading dimensions or a C one element
    off a 16-byte boundary)."""
    c = case
    M, N, K = c.M, c.N, c.K
    abt, ct = TD[c.ab], TD[c.c]
    checks = []
    A, _ = _filled(*((M, K) if c.akm else (K, M)), abt, integer_tensor((M, K) if c.akm else (K, M), -4, 4, abt, 1, "cuda"),
                   (K if c.akm else M) + c.pad_ab)
    B, _ = _filled(*((N, K) if c.bkm else (K, N)), abt, integer_tensor((N, K) if c.bkm else (K, N), -4, 4, abt, 2, "cuda"),
                   (K if c.bkm else N) + c.pad_ab)
    acc = (A if c.akm else A.t()).double() @ (B if c.bkm else B.t()).double().t()
    assert acc.abs().max().item() < 2 ** 24
    ref = acc * c.alpha
    bias = res = aux = pre = None
    if c.flags & kc.EPI_BIAS:
        bias = integer_tensor((N,), -4, 4, TD[c.bias], 3, "cuda")
        ref = ref + bias.double()
    if c.flags & kc.EPI_STORE_PRE:
        pre = ref.clone()
        aux, chk = guarded(M, N, ct, N + c.ldaux)
        checks.append(chk)
    if c.flags & kc.EPI_QGELU:
        ref = ref * torch.sigmoid(1.702 * ref)
    if c.flags & kc.EPI_MUL_AUX:
        aux, chk = _filled(M, N, ct, integer_tensor((M, N), -4, 4, ct, 4, "cuda"), N + c.ldaux)
        checks.append(chk)
        ref = ref * aux.double()
    if c.flags & kc.EPI_RESID:
        res, chk = _filled(M, N, ct, integer_tensor((M, N), -4, 4, ct, 5, "cuda"), N + c.ldr)
        checks.append(chk)
        ref = ref + res.double()
    C, chk = guarded(M, N, ct, N + c.ldc, c.c_off)
    checks.append(chk)
    if c.flags & kc.EPI_BETA:
        C.copy_(integer_tensor((M, N), -4, 4, ct, 6, "cuda"))
        ref = ref + C.double()
    ws = db = dbref = None
    if c.split > 1 or c.bias_grad:
        ws = torch.empty(max(1, c.split) * M * (N + 1), device="cuda", dtype=torch.float32)
    if c.bias_grad:
        db, chk = guarded1d(M, torch.float32)
        checks.append(chk)
        db.copy_(integer_tensor((M,), -4, 4, torch.float32, 7, "cuda"))
        dbref = db.double() + (A if c.akm else A.t()).double().sum(1)
    kern.gemm(M, N, K, A, A.stride(0), c.akm, B, B.stride(0), c.bkm, C, C.stride(0), bias=bias, residual=res,
              ldr=res.stride(0) if res is not None else 0, aux=aux, ldaux=aux.stride(0) if aux is not None else 0,
              alpha=c.alpha, flags=c.flags, split_k=c.split, workspace=None if c.ab == "x3" else ws, bias_grad=db,
              small_tile=c.small, split3=c.ab == "x3")
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    if c.flags & kc.EPI_QGELU:
        assert torch.equal(aux, pre.float().to(ct)), "pre-activation"
        err = (C.double() - ref).abs().max().item() / max(1.0, ref.abs().max().item())
        assert err < 3e-2, err
    else:
        want = ref.float().to(ct)
        bad = C != want  # an element nobody stored is still the guard's NaN and counts
        assert not bool(bad.any()), (int(bad.sum()), (C.double() - want.double()).abs().nan_to_num(1e30).max().item(),
                                      torch.nonzero(bad)[0].tolist())
    if db is not None:
        assert torch.equal(db.double(), dbref), "bias gradient"


# =============================================================================================== B. attention
def _attn_dtype(entry):
    return torch.float32 if entry in ("f32", "x3") else torch.bfloat16


# every entry point takes every N in [1, 4096]; kernel_checks.attn_entries leaves out those that only repeat another
ATTN_CASES = [(N, m, e) for (N, m) in kc.attn_cases() for e in kc.attn_entries(N)]


@functools.lru_cache(maxsize=8)
def _onehot(N, mask, family):
    return kc.attn_onehot_case(N, mask, family, device="cuda")


def _attn_fwd(entry, monkeypatch, qkv, kmask, causal, B, H, N):
    """Forward of an entry point into guarded outputs; returns (o or None, lse, checks)."""
    D = H * 64
    dtype = _attn_dtype(entry)
    s = kern.stream()
    mp = kmask.data_ptr() if kmask is not None else None
    lse, c_lse = guarded1d(B * H * N, torch.float32)
    monkeypatch.setenv("CLIPMI_ATTN_FA", "1" if entry == "bf16_fa" else "0")
    if entry == "mxfp8":
        o8, c1 = guarded(B * N, D, torch.uint8)
        s8, c2 = guarded(B * N, D // 32, torch.uint8)
        T.call("clipmi_attention_fwd_mxfp8", s, qkv.data_ptr(), o8.data_ptr(), s8.data_ptr(), lse.data_ptr(), mp,
               int(causal), B, H, N, D)
        return None, lse, [c_lse, c1, c2]
    o, c_o = guarded(B * N, D, dtype)
    if entry == "x3":
        T.call("clipmi_attention_fwd_x3", s, qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), mp, int(causal), B, H, N, D)
    else:
        T.call("clipmi_attention_fwd", s, DT[dtype], qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), mp, int(causal),
               B, H, N, D)
    return o, lse, [c_lse, c_o]


def _attn_bwd(entry, qkv, o, lse, do, kmask, causal, B, H, N):
    D = H * 64
    dtype = _attn_dtype(entry)
    mp = kmask.data_ptr() if kmask is not None else None
    dqkv, chk = guarded(B * N, 3 * D, dtype)
    if entry == "x3":
        T.call("clipmi_attention_bwd_x3", kern.stream(), qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), do.data_ptr(),
               dqkv.data_ptr(), mp, int(causal), B, H, N, D)
    else:
        T.call("clipmi_attention_bwd", kern.stream(), DT[dtype], qkv.data_ptr(), o.data_ptr(), lse.data_ptr(),
               do.data_ptr(), dqkv.data_ptr(), mp, int(causal), B, H, N, D)
    return dqkv, chk


def _heads(t, B, N, H):
    """[B*N, H*64] -> [B, H, N, 64]"""
    return t.view(B, N, H, 64).permute(0, 2, 1, 3)


def _onehot_run(N, mask, entry, family, monkeypatch, backward):
    """One family of a one-hot case through an entry point: (case, outputs and references), guards checked."""
    case = _onehot(N, mask, family)
    assert case["leak"] < kc.LEAK_MAX, (family, case["leak"])  # the precondition, before anything is launched
    B, H, causal = case["B"], case["H"], case["causal"]
    D, dtype = H * 64, _attn_dtype(entry)
    qkv = case["qkv"].to("cuda", dtype)
    assert torch.equal(qkv.float().cpu(), case["qkv"])  # exact in the entry point's dtype
    kmask = case["kmask"].cuda() if case["kmask"] is not None else None
    o, lse, checks = _attn_fwd(entry, monkeypatch, qkv, kmask, causal, B, H, N)
    do = dqkv = None
    if backward:
        do = integer_tensor((B * N, D), -4, 4, dtype, N + 5, "cuda")
        dqkv, chk = _attn_bwd(entry, qkv, o, lse, do, kmask, causal, B, H, N)
        checks.append(chk)
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    idx = case["pi"].cuda()[:, None, :, None].expand(B, H, N, 64)
    return case, qkv, idx, o, lse, do, dqkv


def _int_ulp(ref, dtype):
    """One ulp of dtype at an integer-valued reference.  At 0 -- where a spacing is not defined -- the spacing at 1,
    the smallest magnitude a non-zero integer reference has."""
    return kc.ulp(ref.abs().clamp_min(1.0), dtype)


@pytest.mark.parametrize("N,mask,entry", ATTN_CASES)
def test_attention_onehot_forward(N, mask, entry, monkeypatch):
    """Each query's softmax is one key (kernel_checks.onehot_attention_inputs; fp64 leak < 2^-40, re-asserted here):
    O is that key's row of V within one ulp of the output dtype (plus 8 leak + 2^-40, what the other keys may add;
    exactly 0 where V is 0) and lse
    the selected score, 8 c, within 1e-3.  A wrong row, or a decoy key -- as strong as the selected one, one
    position past the causal or padding boundary -- leaking through the mask, is an O(1) error: it halves the
    selected weight and moves lse by log 2."""
    for family in kc.attn_families(N, mask):
        case, qkv, idx, o, lse, _, _ = _onehot_run(N, mask, entry, family, monkeypatch, False)
        B, H, D, dtype = case["B"], case["H"], case["H"] * 64, _attn_dtype(entry)
        e_l = (lse.double().view(B, H, N) - case["sel"].cuda()).abs().nan_to_num(1e30).max().item()
        assert e_l <= 1e-3, (family, "lse", e_l)
        if o is None:  # the MXFP8 forward: lse only
            continue
        oref = torch.gather(_heads(qkv[:, 2 * D:].double(), B, N, H), 2, idx)
        e_o = (_heads(o.double(), B, N, H) - oref).abs().nan_to_num(1e30) - (kc.ulp(oref, dtype) + 8 * case["leak"] + 2.0 ** -40)
        assert e_o.max().item() <= 0, (family, "O", e_o.max().item())


@pytest.mark.parametrize("N,mask,entry", [c for c in ATTN_CASES if c[2] != "mxfp8"])
def test_attention_onehot_backward(N, mask, entry, monkeypatch):
    """The backward of the one-hot cases with integer dO in [-4, 4]: dV[j] is the sum of dO[i] over the queries
    selecting j, an exact integer, within one ulp of the output dtype (plus 4 N leak), and |dQ|, |dK| <= 1e-6 c,
    since dS vanishes on the selected key and the rest is below the leak.  (At a reference of 0, where a spacing is
    not defined, the spacing at 1 counts: the smallest magnitude of a non-zero integer.)

    Measured on MI355X, maxima over all cases: bf16 kernels dV 0.5 ulp (the rounding of sums above 256) and
    |dQ|, |dK| 6.3e-15 c; exact-f32 and bf16x3 kernels dV 0 ulp and 6.3e-15 c.  The bf16x3 kernels meet this only
    because they keep weightless keys out of their products (attention_x3.hip p_flush)."""
    for family in kc.attn_families(N, mask):
        case, qkv, idx, o, lse, do, dqkv = _onehot_run(N, mask, entry, family, monkeypatch, True)
        B, H, D, dtype = case["B"], case["H"], case["H"] * 64, _attn_dtype(entry)
        dvref = torch.zeros(B, H, N, 64, dtype=torch.float64, device="cuda")
        dvref.scatter_add_(2, idx, _heads(do.double(), B, N, H))
        err = (_heads(dqkv[:, 2 * D:].double(), B, N, H) - dvref).abs().nan_to_num(1e30)
        e_v = (err / (_int_ulp(dvref, dtype) + 4 * N * case["leak"])).max().item()
        e_qk = dqkv[:, :2 * D].double().abs().nan_to_num(1e30).max().item() / case["c"]
        assert e_v <= 1.0, (family, "dV", e_v)
        assert e_qk <= 1e-6, (family, "dQ/dK", e_qk)


def _uniform_inputs(B, H, N, seed):
    """q = 0, k and v standard normal rounded to bf16 (exact in every entry point's dtype); fp32 [B*N, 3*H*64]."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * N, 3 * H * 64, generator=g).bfloat16().float()
    qkv[:, :H * 64] = 0
    return qkv


# (rtol, atol) of |O - ref| <= rtol |ref| + atol.  bf16: the designed 2^-8, 2^-20 hold (measured max of
# err / (|ref| + atol / rtol): 3.89e-3 = 0.996 * 2^-8, both bf16 forwards).  fp32 and x3: the designed rtol 2^-21
# holds, the designed atol 2^-30 does not -- the fp32 accumulation of up to 4096 values of size ~1 leaves an absolute
# error on means that nearly cancel.  Measured max of err - 2^-21 |ref|: 9.05e-9 (fp32 and x3 alike), so atol is
# 2.8e-8, within 4 x that; measured max of err / |ref| over |ref| > 2^-6: 5.9e-7.  At the longest row the bound is
# 10^3 times below half of what one leaked key moves O (asserted per row in the test).
UNIFORM_O = {torch.bfloat16: (2.0 ** -8, 2.0 ** -20), torch.float32: (2.0 ** -21, 2.8e-8)}
UNIFORM_LSE = 1e-5  # measured max: 1.07e-6 bf16 / bf16 flash / mxfp8, 1.22e-6 fp32, 9.5e-7 x3


@pytest.mark.parametrize("N,mask,entry", ATTN_CASES)
def test_attention_uniform(N, mask, entry, monkeypatch):
    """q = 0: P is uniform over the allowed keys, so O is the mean of V over them (fp64 reference; |O - ref| <=
    2^-8 |ref| + 2^-20 in bf16, 2^-21 |ref| + 2.8e-8 in fp32 and x3: UNIFORM_O above, with the measured
    deviations that set it) and lse = log(count) within 1e-5.  Both bounds stay below half the effect of one leaked key at every row -- 1 / (2 count) on lse, max|V| / (2 count) on O --
    which is asserted before anything is launched.  dV against the fp64 reference with the 2 x TOL bound of
    test_attention."""
    B, H = kc.attn_dims(N, mask)
    lens, causal = kc.attn_lens(N, mask), "causal" in mask
    D, dtype = H * 64, _attn_dtype(entry)
    qkv = _uniform_inputs(B, H, N, 3 * N + 1).to("cuda", dtype)
    kmask = None if lens is None else (torch.arange(N)[None] < torch.tensor(lens)[:, None]).to(torch.int64).cuda()
    cnt = kc.attn_allowed_count(B, N, lens, causal).cuda()  # [B, N]
    v = _heads(qkv[:, 2 * D:].double(), B, N, H)
    cidx = (cnt - 1)[:, None, :, None].expand(B, H, N, 64)
    oref = torch.gather(v.cumsum(2), 2, cidx) / cnt[:, None, :, None]
    lref = torch.log(cnt.double())[:, None, :].expand(B, H, N)
    rtol, atol = UNIFORM_O[dtype]
    bound = rtol * oref.abs() + atol
    # the condition the bounds may never give up: half of what one more key would change
    vmax = v.abs().max().item()
    assert bool((bound < vmax / (2.0 * cnt[:, None, :, None])).all())
    assert UNIFORM_LSE < 1.0 / (2.0 * cnt.max().item())
    o, lse, checks = _attn_fwd(entry, monkeypatch, qkv, kmask, causal, B, H, N)
    if o is not None:
        do = torch.randn(B * N, D, generator=torch.Generator().manual_seed(N + 9)).to("cuda", dtype)
        dqkv, chk = _attn_bwd(entry, qkv, o, lse, do, kmask, causal, B, H, N)
        checks.append(chk)
    torch.cuda.synchronize()
    for chk in checks:
        chk()
    e_l = (lse.double().view(B, H, N) - lref).abs().max().item()
    if o is None:
        assert e_l <= UNIFORM_LSE, e_l
        return
    err = (_heads(o.double(), B, N, H) - oref).abs()
    m_rel = (err / (oref.abs() + atol / rtol)).max().item()  # in units of the bound's rtol
    assert e_l <= UNIFORM_LSE, e_l
    assert bool((err <= bound).all()), m_rel
    # dV[j] = sum over the queries i that see key j of dO[i] / count[i]
    w = _heads(do.double(), B, N, H) / cnt[:, None, :, None]
    if causal:
        dvref = w.flip(2).cumsum(2).flip(2)
    else:
        dvref = w.sum(2, keepdim=True).expand(B, H, N, 64).clone()
    if lens is not None:
        dvref = dvref * (torch.arange(N, device="cuda")[None, :] < torch.tensor(lens, device="cuda")[:, None])[:, None, :, None]
    dv = _heads(dqkv[:, 2 * D:].double(), B, N, H)
    e_v = (dv - dvref).abs().nan_to_num(1e30).max().item() / dvref.abs().max().clamp_min(1e-6).item()
    assert e_v < 2 * TOL[dtype], e_v


@pytest.mark.parametrize("N", [0, 4097])
def test_attention_rejects_n_outside_1_4096(N):
    B, H, D = 1, 1, 64
    buf = [torch.zeros(4096, device="cuda") for _ in range(7)]
    qkv, o, lse, do, dqkv, img, cs = [b.data_ptr() for b in buf]
    s = kern.stream()
    tail = (None, 0, B, H, N, D)
    calls = [("clipmi_attention_fwd", (s, BF16, qkv, o, lse) + tail),
             ("clipmi_attention_fwd", (s, F32, qkv, o, lse) + tail),
             ("clipmi_attention_bwd", (s, BF16, qkv, o, lse, do, dqkv) + tail),
             ("clipmi_attention_bwd", (s, F32, qkv, o, lse, do, dqkv) + tail),
             ("clipmi_attention_fwd_mxfp8", (s, qkv, o, img, lse) + tail),
             ("clipmi_attention_fwd_x3", (s, qkv, o, lse) + tail),
             ("clipmi_attention_bwd_x3", (s, qkv, o, lse, do, dqkv) + tail),
             ("clipmi_attention_fwd_x3img", (s, qkv, o, img, lse) + tail),
             ("clipmi_attention_bwd_x3img", (s, qkv, o, lse, do, img, cs, 1, dqkv, 4096 * 4) + tail)]
    for name, args in calls:
        with pytest.raises(ValueError):
            T.call(name, *args)
    torch.cuda.synchronize()


# =============================================================================================== C. LayerNorm
# Per-element bound |err| <= t (1 + |ref|) against the fp64 reference on the storage-rounded inputs: LN_T_OUT for y
# and dx by their dtype, LN_T_STAT for mean, rstd, dw and db (fp32 in every mode).  At most 4 x the maxima measured
# over all cases of test_layernorm_strided on MI355X and never above the 2e-5 / 3e-2 of test_layernorm_fwd_bwd:
#   y / dx   fp32 3.66e-7;  bf16 3.11e-3 (bf16 x), 3.12e-3 (fp32 x, with bf16 or fp32 gamma)
#   stats    4.53e-6 (f32), 5.16e-6 (bf16), 5.44e-6 (fp32 x with bf16 gradients): dw at R = 333, fp32 sums over rows;
#            4 x that is 2.2e-5, so the existing 2e-5 holds instead
LN_T_OUT = {torch.float32: 1.4e-6, torch.bfloat16: 1.2e-2}
LN_T_STAT = 2e-5
# leading dimensions: all D; all different, in odd steps (a fast width then runs the one-wave-per-row kernel); and, at
# the fast widths, all different multiples of 4 (the register-resident kernels)
LN_CASES = [(m, D, R, s) for m in kc.LN_MODES for D in kc.LN_WIDTHS for R in kc.LN_ROWS
            for s in ((False, "vec", "odd") if kc.ln_fast_width(D) else (False, "odd"))]


def _ln_err(got, ref):
    return ((got.double() - ref).abs() / (1 + ref.abs())).nan_to_num(1e30).max().item()


@pytest.mark.parametrize("mode,D,R,strided", LN_CASES)
def test_layernorm_strided(mode, D, R, strided):
    """clipmi_layernorm_fwd / _bwd (f32, bf16), _fwd2 / _bwd2 (fp32 x into bf16 y and gradients) and _bwd3 (the same
    with fp32 gamma) at every width class and leading dimensions that all differ, against fp64 on the
    storage-rounded inputs, per element: |err| <= t (1 + |ref|).  y, mean, rstd, dx, dw, db are guarded; the strided
    cases accumulate dw / db (beta_wb) onto integers."""
    xt = torch.bfloat16 if mode == "bf16" else torch.float32
    gt = torch.float32 if mode == "f32" else torch.bfloat16  # y, dy, dx, dres and the forward's w / b
    wt = torch.float32 if mode == "x32_bf16_w32" else gt     # the backward's w
    ldx, ldy, lddy, lddx, ldres = kc.ln_leading_dims(D, strided)
    g = torch.Generator().manual_seed(D + R)
    r = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    x, _ = _filled(R, D, xt, (r(R, D) * 1.5 + 0.3).cuda(), ldx)
    w = (1 + 0.2 * r(D)).to("cuda", gt)
    b = (0.2 * r(D)).to("cuda", gt)
    dy, _ = _filled(R, D, gt, r(R, D).cuda(), lddy)
    dres, _ = _filled(R, D, gt, r(R, D).cuda(), ldres)
    y, c_y = guarded(R, D, gt, ldy)
    mean, c_m = guarded1d(R, torch.float32)
    rstd, c_r = guarded1d(R, torch.float32)
    dx, c_dx = guarded(R, D, gt, lddx)
    dw, c_dw = guarded1d(D, torch.float32)
    db, c_db = guarded1d(D, torch.float32)
    beta = int(bool(strided))
    dw0 = integer_tensor((D,), -4, 4, torch.float32, 1, "cuda") if beta else torch.zeros(D, device="cuda")
    db0 = integer_tensor((D,), -4, 4, torch.float32, 2, "cuda") if beta else torch.zeros(D, device="cuda")
    if beta:
        dw.copy_(dw0)
        db.copy_(db0)
    s = kern.stream()
    eps = 1e-5
    if mode in ("f32", "bf16"):
        T.call("clipmi_layernorm_fwd", s, DT[gt], x.data_ptr(), ldx, y.data_ptr(), ldy, w.data_ptr(), b.data_ptr(),
               mean.data_ptr(), rstd.data_ptr(), R, D, eps, None, None, 0)
    else:
        T.call("clipmi_layernorm_fwd2", s, F32, BF16, x.data_ptr(), ldx, y.data_ptr(), ldy, w.data_ptr(), b.data_ptr(),
               mean.data_ptr(), rstd.data_ptr(), R, D, eps, None, None, 0)
    wb = w.to(wt)  # the same values (bf16 -> fp32 is exact)
    ws = T._ws(T._lib.lib().clipmi_layernorm_bwd_ws(R, D), "cuda")
    common = (dy.data_ptr(), lddy, x.data_ptr(), ldx, mean.data_ptr(), rstd.data_ptr(), wb.data_ptr(), dx.data_ptr(),
              lddx, dres.data_ptr(), ldres, dw.data_ptr(), db.data_ptr(), beta, ws.data_ptr(), ws.numel(), R, D)
    if mode in ("f32", "bf16"):
        T.call("clipmi_layernorm_bwd", s, DT[gt], *common)
    elif mode == "x32_bf16":
        T.call("clipmi_layernorm_bwd2", s, F32, BF16, *common)
    else:
        T.call("clipmi_layernorm_bwd3", s, F32, BF16, F32, *common)
    torch.cuda.synchronize()
    for chk in (c_y, c_m, c_r, c_dx, c_dw, c_db):
        chk()
    xd, wd, bd, dyd = x.double(), w.double(), b.double(), dy.double()
    mu = xd.mean(1, keepdim=True)
    rs = (xd.var(1, unbiased=False, keepdim=True) + eps).rsqrt()
    xh = (xd - mu) * rs
    gd = dyd * wd
    dxr = rs * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True)) + dres.double()
    e_out = max(_ln_err(y, xh * wd + bd), _ln_err(dx, dxr))
    e_stat = max(_ln_err(mean, mu[:, 0]), _ln_err(rstd, rs[:, 0]), _ln_err(dw, dw0.double() + (dyd * xh).sum(0)),
                 _ln_err(db, db0.double() + dyd.sum(0)))
    assert e_out <= LN_T_OUT[gt], e_out
    assert e_stat <= LN_T_STAT, e_stat


@pytest.mark.parametrize("D", kc.LN_WIDTHS)
def test_layernorm_fp32_constant_and_offset_rows(D):
    """Two rows that pin the two-pass variance (csrc/norm.hip computes it from the centred values): a constant row
    has variance exactly 0, so y equals b bit for bit and rstd is eps^-0.5 within 1e-6 relative; a row of
    1000 + N(0, 1) -- where E[x^2] - E[x]^2 would lose every digit in fp32 -- stays within 1e-3 absolute of fp64."""
    g = torch.Generator().manual_seed(D)
    xs = torch.stack([torch.full((D,), 1.5), 1000 + torch.randn(D, generator=g)])
    x, _ = _filled(2, D, torch.float32, xs.cuda(), D + 4)
    w = (1 + 0.2 * torch.randn(D, generator=g)).cuda()
    b = (0.2 * torch.randn(D, generator=g)).cuda()
    y, c_y = guarded(2, D, torch.float32, D + 8)
    mean, c_m = guarded1d(2, torch.float32)
    rstd, c_r = guarded1d(2, torch.float32)
    eps = 1e-5
    T.call("clipmi_layernorm_fwd", kern.stream(), F32, x.data_ptr(), D + 4, y.data_ptr(), D + 8, w.data_ptr(),
           b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), 2, D, eps, None, None, 0)
    torch.cuda.synchronize()
    for chk in (c_y, c_m, c_r):
        chk()
    assert torch.equal(y[0], b)
    assert mean[0].item() == 1.5
    assert abs(rstd[0].item() * math.sqrt(eps) - 1) <= 1e-6
    xd = x[1].double()
    ref = (xd - xd.mean()) * (xd.var(unbiased=False) + eps).rsqrt() * w.double() + b.double()
    assert (y[1].double() - ref).abs().max().item() <= 1e-3
