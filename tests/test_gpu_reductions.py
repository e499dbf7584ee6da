"""Exact-sum tests of the kernels that turn activation gradients into parameter gradients, and of the row gather /
scatter and the small fp32 reductions around them (case lists and input builders: tests/kernel_checks.py; their
preconditions -- the 2^24 bound and the loop regime every case is named for: tests/test_cpu_kernel_checks.py).

Every summed operand is an integer tensor whose partial and total sums stay below 2^24, so the fp32 result is exact
whatever the order of summation: outputs are compared with torch.equal against an int64 sum from the CPU.  Every
output lives inside a guard band, and workspaces are prefilled with bytes no kernel may rely on.  The only
tolerances are the clip coefficient's 2 ulp and the 2e-5 of the two backwards that have no exact form."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_checks as kc  # noqa: E402
from kernel_checks import guarded, guarded1d, integer_tensor, untouched  # noqa: E402

from clipmi import kernels as kern  # noqa: E402
from clipmi import shared_adapter  # noqa: E402,F401  (declares clipmi_softmax_rows / _bwd)
from clipmi import towers as T  # noqa: E402
from clipmi._lib import BF16, F32  # noqa: E402

DT = {torch.bfloat16: BF16, torch.float32: F32}
DTYPES = [torch.bfloat16, torch.float32]
TOL32 = 2e-5  # the fp32 bound of tests/test_gpu_kernels.py (max-abs error over max-abs reference)
NAN_BYTE, STALE_BYTE = 0xFF, 0xA5


def _filled(rows, cols, dtype, values, ld=None, off=0):
    """values (CPU or GPU) in a guarded [rows, cols] view: an input whose pad columns read as NaN, or an output to
    add onto."""
    view, check = guarded(rows, cols, dtype, ld, off)
    view.copy_(values)
    return view, check


def _bytes(n, fill):
    return torch.full((max(int(n), 16),), fill, dtype=torch.uint8, device="cuda")


def _same(got, want):
    """Bitwise-equal values; an element nobody stored is still the guard's NaN and fails."""
    assert got.shape == want.shape and got.dtype == want.dtype
    if not torch.equal(got, want):
        bad = got != want
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} elements differ, first at "
                             f"{torch.nonzero(bad)[0].tolist()}: got {got[bad][0].item()}, want {want[bad][0].item()}")


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().nan_to_num(1e30).max() / b.abs().max().clamp_min(1e-6)).item()


# =============================================================================================== colsum
COLSUM_CASES = kc.colsum_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("case", COLSUM_CASES, ids=[c.id() for c in COLSUM_CASES])
def test_colsum_exact(case, dtype):
    """clipmi_colsum against the int64 column sums: the vector and the one-column partial kernels, reduce_partials4
    with and without its unrolled loop, reduce_partials, the chunk count capped at 512 (rows_per = 257), ldx > N,
    x off its vector boundary, beta 0 and 1; the workspace holds NaN bytes before the call."""
    c = case
    xv, out0, ref = kc.colsum_inputs(c, dtype)
    assert ref.abs().max().item() < kc.EXACT
    x, _ = _filled(c.R, c.N, dtype, xv, c.N + c.ld_pad, c.x_off)
    out, chk = guarded1d(c.N, torch.float32)
    if c.beta:
        out.copy_(out0)
    ws = _bytes(T._lib.lib().clipmi_colsum_ws(c.R, c.N), NAN_BYTE)
    assert ws.data_ptr() % 16 == 0
    T.call("clipmi_colsum", kern.stream(), DT[dtype], x.data_ptr(), x.stride(0), c.R, c.N, out.data_ptr(), c.beta,
           ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    chk()
    _same(out.cpu(), ref.float())


# =============================================================================================== period_sum
PERIOD_CASES = kc.period_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("case", PERIOD_CASES, ids=[c.id() for c in PERIOD_CASES])
def test_period_sum_exact(case, dtype):
    """clipmi_period_sum against the int64 sums over the batch: nb on both sides of the 8-deep unrolled loop's
    threshold (29) and of a second pass (61), nt = period, nt < period (rows t >= nt of the guarded [period, D]
    block keep the guard pattern) and period = 1, one and several column blocks, ldx > D, beta 0 and 1."""
    c = case
    xv, out0, ref = kc.period_inputs(c, dtype)
    assert ref.abs().max().item() < kc.EXACT
    x, _ = _filled(c.nb * c.period, c.D, dtype, xv, c.D + c.ld_pad)
    out, chk = guarded(c.period, c.D, torch.float32)
    if c.beta:
        out[:c.nt].copy_(out0)
    T.call("clipmi_period_sum", kern.stream(), DT[dtype], x.data_ptr(), x.stride(0), c.nb, c.period, c.nt, c.D,
           out.data_ptr(), c.beta)
    torch.cuda.synchronize()
    chk()
    _same(out[:c.nt].cpu(), ref.float())
    if c.nt < c.period:
        assert untouched(out[c.nt:]), "rows t >= nt were stored to"


def test_period_sum_and_text_embed_reject_misaligned_vectors():
    """The 4-element vector accesses of both entry points are a documented precondition: a leading dimension or a
    pointer that does not fit them is CLIPMI_ERR_INVALID (ValueError), nothing is launched."""
    D, nb = 8, 3
    s = kern.stream()
    for dtype in DTYPES:
        x = torch.zeros(nb * (D + 4) + 8, dtype=dtype, device="cuda")
        out, chk = guarded(1, D, torch.float32)
        out1, chk1 = guarded(1, D, torch.float32, None, 1)
        es = x.element_size()
        for xp, ldx, op in ((x.data_ptr(), D + 1, out.data_ptr()), (x.data_ptr(), D + 2, out.data_ptr()),
                            (x.data_ptr() + es, D, out.data_ptr()), (x.data_ptr(), D, out1.data_ptr())):
            with pytest.raises(ValueError):
                T.call("clipmi_period_sum", s, DT[dtype], xp, ldx, nb, 1, 1, D, op, 0)
        with pytest.raises(ValueError):
            T.call("clipmi_period_sum", s, DT[dtype], x.data_ptr(), D + 2, nb, 1, 1, D + 2, out.data_ptr(), 0)  # D % 4
        ids = torch.zeros(2, dtype=torch.int64, device="cuda")
        tok = torch.zeros(4 * D + 8, dtype=dtype, device="cuda")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        x0, chk0 = guarded(2, D, dtype)
        x1, chk2 = guarded(2, D, dtype, None, 1)
        t, o = tok.data_ptr(), x0.data_ptr()
        for tp, pp, op in ((t + es, t, o), (t, t + es, o), (t, t, x1.data_ptr())):
            with pytest.raises(ValueError):
                T.call("clipmi_text_embed", s, DT[dtype], ids.data_ptr(), tp, pp, op, 2, 1, D, 2, bad.data_ptr())
        torch.cuda.synchronize()
        for c in (chk, chk1, chk0, chk2):
            c()
        assert untouched(out) and untouched(out1) and untouched(x0) and untouched(x1) and bad.item() == 0


# =============================================================================================== text embedding
EMBED_BWD_CASES = kc.embed_bwd_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("case", EMBED_BWD_CASES, ids=[c.id() for c in EMBED_BWD_CASES])
def test_text_embed_bwd_exact(case, dtype):
    """clipmi_text_embed_bwd against index_add_ in int64 (integer dx0: the order of the kernel's atomics does not
    matter): vocabularies on both sides of id_scan_kernel's one-entry-per-thread limit (V = 1024 / 1025) and the
    real one (49408), row counts around the 64-row chunk, one id owning every chunk, every row its own id, ids
    outside the vocabulary (-1, V, 2^40: no contribution), beta 0 and 1.  The workspace starts as 0xA5 bytes and is
    used for a second call as the first one left it."""
    c = case
    ids, dxv, g0, ref1, ref2 = kc.embed_bwd_inputs(c, dtype)
    assert max(ref1.abs().max().item(), ref2.abs().max().item()) < kc.EXACT
    dx0, _ = _filled(c.R, c.D, dtype, dxv)
    gtok, chk = guarded(c.V, c.D, torch.float32)
    if c.beta:
        gtok.copy_(g0)
    idd = ids.cuda()
    ws = _bytes(T._lib.lib().clipmi_text_embed_bwd_ws(c.R, c.V), STALE_BYTE)
    for ref in (ref1, ref2):
        T.call("clipmi_text_embed_bwd", kern.stream(), DT[dtype], idd.data_ptr(), dx0.data_ptr(), c.R, c.D, c.V,
               gtok.data_ptr(), c.beta, ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        chk()
        _same(gtok.cpu(), ref.float())


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("B,S,D,V", kc.EMBED_FWD_CASES)
def test_text_embed_fwd_exact(B, S, D, V, dtype):
    """x0[r] = tok[ids[r]] + pos[r % S]: one fp32 add rounded once to the output dtype, so bitwise equal to torch's;
    R = B S no multiple of the 4 rows of a block, ids 0 and V - 1 present.  *bad_flag stays 0 on valid ids and
    becomes 1 for a negative id and for an id >= V (such a row reads tok[0])."""
    R = B * S
    g = torch.Generator().manual_seed(R + D)
    tok = torch.randn(V, D, generator=g).to(dtype)
    pos = torch.randn(S, D, generator=g).to(dtype)
    ids = kc.embed_fwd_ids(B, S, V, R + V)
    tokd, posd = tok.cuda(), pos.cuda()
    for bad_id in (None, -1, V, 2 ** 40):
        cur = ids.clone()
        if bad_id is not None:
            cur[R // 2] = bad_id
        idd = cur.cuda()
        x0, chk = guarded(R, D, dtype)
        flag, chk_f = guarded1d(1, torch.int32)
        flag.zero_()
        T.call("clipmi_text_embed", kern.stream(), DT[dtype], idd.data_ptr(), tokd.data_ptr(), posd.data_ptr(),
               x0.data_ptr(), R, S, D, V, flag.data_ptr())
        torch.cuda.synchronize()
        chk()
        chk_f()
        safe = torch.where((cur >= 0) & (cur < V), cur, torch.zeros_like(cur))
        want = (tok.float()[safe] + pos.float()[torch.arange(R) % S]).to(dtype)
        _same(x0.cpu(), want)
        assert flag.item() == (0 if bad_id is None else 1), bad_id


# =============================================================================================== pool / gather / scatter
@pytest.mark.parametrize("kind", kc.POOL_KINDS)
@pytest.mark.parametrize("B", kc.ROWS_B)
@pytest.mark.parametrize("S", kc.ROWS_S)
def test_pool_index(kind, B, S):
    """mode 0 gives token 0; mode 1 the first EOS of several, 0 when the row has none; mode 2 the first of tied
    maxima; B around the 256 rows of a block."""
    ids, mode, want = kc.pool_inputs(kind, B, S, B + S)
    idd = ids.cuda()
    idx, chk = guarded1d(B, torch.int32)
    T.call("clipmi_pool_index", kern.stream(), idd.data_ptr(), B, S, kc.POOL_EOS, mode, idx.data_ptr())
    torch.cuda.synchronize()
    chk()
    _same(idx.cpu(), want)


ROWS_CASES = kc.rows_cases()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("B,S,D", ROWS_CASES)
def test_gather_rows_bitwise(B, S, D, dtype):
    """out[b] = src[b S + idx[b]] (idx NULL: token 0), a copy: bitwise, D around the 256 lanes of a block."""
    src = torch.randn(B * S, D, generator=torch.Generator().manual_seed(B + D)).to(dtype)
    srcd = src.cuda()
    for idx in (None, kc.rows_idx(B, S, B + S + D)):
        out, chk = guarded(B, D, dtype)
        idd = idx.cuda() if idx is not None else None
        T.call("clipmi_gather_rows", kern.stream(), DT[dtype], srcd.data_ptr(), T.P_(idd), B, S, D, out.data_ptr())
        torch.cuda.synchronize()
        chk()
        rows = torch.arange(B) * S + (idx.long() if idx is not None else 0)
        _same(out.cpu(), src[rows])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("B,S,D", ROWS_CASES)
def test_scatter_rows_bitwise(B, S, D, dtype):
    """dst[b S + idx[b]] (+)= src[b] with integer operands (the fp32 add and its rounding to dst's dtype are exact);
    dst is a guarded [B S, D] block whose unselected rows must stay guard bytes."""
    src = integer_tensor((B, D), -4, 4, dtype, B + D)
    old = integer_tensor((B, D), -4, 4, dtype, B + D + 1)
    srcd = src.cuda()
    for idx in (None, kc.rows_idx(B, S, B + S + D)):
        rows = torch.arange(B) * S + (idx.long() if idx is not None else 0)
        idd = idx.cuda() if idx is not None else None
        for beta in (0, 1):
            dst, chk = guarded(B * S, D, dtype)
            if beta:
                dst[rows.cuda()] = old.cuda()
            T.call("clipmi_scatter_rows", kern.stream(), DT[dtype], srcd.data_ptr(), T.P_(idd), B, S, D,
                   dst.data_ptr(), beta)
            torch.cuda.synchronize()
            chk()
            want = (src.float() + old.float()).to(dtype) if beta else src
            _same(dst.cpu()[rows], want)
            rest = torch.ones(B * S, dtype=torch.bool)
            rest[rows] = False
            if bool(rest.any()):
                assert untouched(dst[rest.cuda()]), "an unselected row was stored to"


# =============================================================================================== gradient norm
def _coef_ok(got, norm, want, max_norm):
    """The clip coefficient: exactly 1 where the contract says so (kernel_checks.clip_expect returns 1.0 there and
    a quotient below 1 everywhere else), else within 2 fp32 ulp of the fp64 value."""
    if want == 1.0:
        assert got == 1.0, (got, float(norm), max_norm)
        return
    assert float(norm) >= max_norm > 0
    w = torch.tensor(want, dtype=torch.float64)
    assert abs(got - want) <= 2 * kc.ulp(w, torch.float32).item(), (got, want)


@functools.lru_cache(maxsize=None)
def _grad(n):
    g = kc.grad_tensor(n, 50 + n % 1000)
    return g, int((g.long() ** 2).sum())


@pytest.mark.parametrize("n", kc.GRAD_NS)
def test_grad_norm_and_scale_exact(n):
    """clipmi_grad_norm on integers in [-3, 3]: the partial sums are exact and the finish kernel adds them in
    double, so norm_out[0] == float32(sqrt(float64(sum))) bitwise; n = 1,048,583 is one full grid-stride pass, one
    vector of a second pass and a scalar tail.  norm_out[1] is exactly 1 for max_norm <= 0, a zero gradient or a
    norm below max_norm, else within 2 ulp of max_norm / (norm + 1e-6); clipmi_grad_scale multiplies by the stored
    coefficient: bitwise the fp32 product.  Workspace prefilled with NaN bytes."""
    gv, sumsq = _grad(n)
    assert sumsq < kc.EXACT
    s = kern.stream()
    for max_norm in (1.0, 0.37, 1e6, 0.0, -1.0):
        g, chk_g = guarded1d(n, torch.float32)
        g.copy_(gv)
        assert g.data_ptr() % 16 == 0
        out, chk_o = guarded1d(2, torch.float32)
        ws = _bytes(T._lib.lib().clipmi_grad_norm_ws(), NAN_BYTE)
        T.call("clipmi_grad_norm", s, g.data_ptr(), n, max_norm, out.data_ptr(), ws.data_ptr(), ws.numel())
        T.call("clipmi_grad_scale", s, g.data_ptr(), n, out.data_ptr())
        torch.cuda.synchronize()
        chk_g()
        chk_o()
        norm, coef = kc.clip_expect(sumsq, max_norm)
        o = out.cpu()
        _same(o[0], norm)
        _coef_ok(o[1].item(), norm, coef, max_norm)
        _same(g.cpu(), gv * o[1])
    # a zero gradient: norm 0, coefficient exactly 1
    g = torch.zeros(n, device="cuda")
    out, chk_o = guarded1d(2, torch.float32)
    ws = _bytes(T._lib.lib().clipmi_grad_norm_ws(), NAN_BYTE)
    T.call("clipmi_grad_norm", s, g.data_ptr(), n, 1.0, out.data_ptr(), ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    chk_o()
    assert out.cpu().tolist() == [0.0, 1.0]


def test_grad_norm_multi_exact():
    """count = 3 segments of 5, 1,048,583 and 0 elements, each 16-byte aligned: the norm over all of them, bitwise;
    a segment 4 bytes off raises ValueError."""
    s = kern.stream()
    segs, sumsq = [], 0
    for n in kc.GRAD_MULTI_NS:
        if n:
            gv, ss = _grad(n)
            g, _ = guarded1d(n, torch.float32)
            g.copy_(gv)
            sumsq += ss
        else:
            g = torch.full((4,), float("nan"), device="cuda")  # never read
        assert g.data_ptr() % 16 == 0
        segs.append(g)
    assert sumsq < kc.EXACT
    count = len(segs)
    gp = (T.c_vp * count)(*[g.data_ptr() for g in segs])
    gn = (T.c_i64 * count)(*kc.GRAD_MULTI_NS)
    for max_norm in (1.0, 1e6):
        out, chk = guarded1d(2, torch.float32)
        ws = _bytes(T._lib.lib().clipmi_grad_norm_multi_ws(count), NAN_BYTE)
        T.call("clipmi_grad_norm_multi", s, gp, gn, count, max_norm, out.data_ptr(), ws.data_ptr(), ws.numel())
        torch.cuda.synchronize()
        chk()
        norm, coef = kc.clip_expect(sumsq, max_norm)
        o = out.cpu()
        _same(o[0], norm)
        _coef_ok(o[1].item(), norm, coef, max_norm)
    out, chk = guarded1d(2, torch.float32)
    ws = _bytes(T._lib.lib().clipmi_grad_norm_multi_ws(count), NAN_BYTE)
    gp_bad = (T.c_vp * count)(segs[0].data_ptr(), segs[1].data_ptr() + 4, segs[2].data_ptr())
    with pytest.raises(ValueError):
        T.call("clipmi_grad_norm_multi", s, gp_bad, gn, count, 1.0, out.data_ptr(), ws.data_ptr(), ws.numel())
    with pytest.raises(ValueError):
        T.call("clipmi_grad_norm", s, segs[1].data_ptr() + 4, 8, 1.0, out.data_ptr(), ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    chk()


@pytest.mark.parametrize("n", kc.SUM2_NS)
def test_sum2_exact(n):
    """out (+)= scale (sum a + sum b) with integers in [-4, 4] and scale = 0.25: exact; b NULL and given, beta 0, 1."""
    a = integer_tensor((n,), -4, 4, torch.float32, n)
    b = integer_tensor((n,), -4, 4, torch.float32, n + 1)
    ad, bd = a.cuda(), b.cuda()
    for bb in (None, b):
        for beta in (0, 1):
            out, chk = guarded1d(1, torch.float32)
            if beta:
                out.fill_(-3.0)
            T.call("clipmi_sum2", kern.stream(), ad.data_ptr(), bd.data_ptr() if bb is not None else None, n, 0.25,
                   out.data_ptr(), beta)
            torch.cuda.synchronize()
            chk()
            total = int(a.long().sum()) + (int(b.long().sum()) if bb is not None else 0)
            assert out.item() == 0.25 * total + (-3.0 if beta else 0.0)


# =============================================================================================== l2norm / softmax
@pytest.mark.parametrize("B", kc.L2_BS)
@pytest.mark.parametrize("E", kc.L2_ES)
def test_l2norm_fwd_structured(B, E):
    """Rows with four entries +-2^k (|x| = 2^(k+1), y = +-0.5) and rows with one (y = +-1): the sum of squares, its
    root and the product with the reciprocal are all exact, so y and nrm are bitwise."""
    for entries in (1, 4):
        if E < entries:
            continue
        xv, yv, nv = kc.l2norm_rows(B, E, entries, B + E)
        x = xv.cuda()
        y, c_y = guarded(B, E, torch.float32)
        nrm, c_n = guarded1d(B, torch.float32)
        T.call("clipmi_l2norm_fwd", kern.stream(), x.data_ptr(), y.data_ptr(), nrm.data_ptr(), B, E)
        torch.cuda.synchronize()
        c_y()
        c_n()
        _same(nrm.cpu(), nv)
        _same(y.cpu(), yv)


@pytest.mark.parametrize("B", kc.L2_BS)
@pytest.mark.parametrize("E", kc.L2_ES)
def test_l2norm_bwd_matches_fp64(B, E):
    """dx = (dy - y (y . dy)) / |x| against fp64 on the same fp32 inputs: max-abs error over max-abs reference
    below 2e-5 (no exact form)."""
    g = torch.Generator().manual_seed(7 * B + E)
    x = torch.randn(B, E, generator=g, dtype=torch.float64)
    n64 = x.norm(dim=1)
    yv, nv, dyv = (x / n64[:, None]).float(), n64.float(), torch.randn(B, E, generator=g)
    ref = (dyv.double() - yv.double() * (yv.double() * dyv.double()).sum(1, keepdim=True)) / nv.double()[:, None]
    y, dy, nrm = yv.cuda(), dyv.cuda(), nv.cuda()
    dx, chk = guarded(B, E, torch.float32)
    T.call("clipmi_l2norm_bwd", kern.stream(), dy.data_ptr(), y.data_ptr(), nrm.data_ptr(), dx.data_ptr(), B, E)
    torch.cuda.synchronize()
    chk()
    err = rel(dx.cpu(), ref)
    assert err < TOL32, err


@pytest.mark.parametrize("R", kc.SM_RS)
@pytest.mark.parametrize("N", kc.SM_NS)
def test_softmax_rows_structured(R, N):
    """Constant rows (integers, scale 0.5): every exponential is exp(0) = 1, the sum is N, so y == float32(1) /
    float32(N) bitwise.  One-hot rows (one 0, the rest -200, scale 1): the other exponentials underflow to exactly
    0, so y is the one-hot row itself.  Out of place and in place (y aliasing x)."""
    const = (torch.arange(R, dtype=torch.float32)[:, None] - 2).expand(R, N).contiguous()
    want_c = (torch.ones(R, N) / torch.tensor(float(N))).float()
    hot = torch.full((R, N), -200.0)
    cols = (torch.arange(R) * 37 + N - 1) % N  # row 0: the last column
    hot[torch.arange(R), cols] = 0.0
    want_h = (hot == 0).float()
    for xv, scale, want in ((const, 0.5, want_c), (hot, 1.0, want_h)):
        x = xv.cuda()
        y, chk = guarded(R, N, torch.float32)
        T.call("clipmi_softmax_rows", kern.stream(), x.data_ptr(), y.data_ptr(), R, N, scale)
        torch.cuda.synchronize()
        chk()
        _same(y.cpu(), want)
        assert torch.equal(x.cpu(), xv)  # the input of an out-of-place call is left alone
        z, chk = _filled(R, N, torch.float32, xv)
        T.call("clipmi_softmax_rows", kern.stream(), z.data_ptr(), z.data_ptr(), R, N, scale)
        torch.cuda.synchronize()
        chk()
        _same(z.cpu(), want)


@pytest.mark.parametrize("R", kc.SM_RS)
@pytest.mark.parametrize("N", kc.SM_NS)
def test_softmax_rows_bwd_matches_fp64(R, N):
    """dx = scale y (dy - <dy, y>) against fp64 on the same fp32 inputs, below 2e-5; out of place and with dx
    aliasing dy, as the adapters call it."""
    g = torch.Generator().manual_seed(11 * R + N)
    scale = 0.125
    yv = torch.softmax(scale * 8 * torch.randn(R, N, generator=g, dtype=torch.float64), 1).float()
    dyv = torch.randn(R, N, generator=g)
    ref = scale * yv.double() * (dyv.double() - (dyv.double() * yv.double()).sum(1, keepdim=True))
    y, dy = yv.cuda(), dyv.cuda()
    dx, chk = guarded(R, N, torch.float32)
    T.call("clipmi_softmax_rows_bwd", kern.stream(), y.data_ptr(), dy.data_ptr(), dx.data_ptr(), R, N, scale)
    z, chk_z = _filled(R, N, torch.float32, dyv)
    T.call("clipmi_softmax_rows_bwd", kern.stream(), y.data_ptr(), z.data_ptr(), z.data_ptr(), R, N, scale)
    torch.cuda.synchronize()
    chk()
    chk_z()
    err = max(rel(dx.cpu(), ref), rel(z.cpu(), ref))
    assert err < TOL32, err


# =============================================================================================== zero rows
def test_zero_row_calls_are_no_ops():
    """Every entry point whose grid is its row count returns CLIPMI_OK at zero rows without a launch (T.call raises
    on any other status) and leaves its guarded outputs untouched."""
    s = kern.stream()
    D, S, V, Bg = 8, 3, 5, 4
    f = torch.zeros(64, device="cuda")
    i64 = torch.zeros(8, dtype=torch.int64, device="cuda")
    i32 = torch.zeros(8, dtype=torch.int32, device="cuda")
    outs = [guarded(2, D, torch.float32) for _ in range(2)] + [guarded(2, D, torch.bfloat16)]
    (o1, _), (o2, _), (ob, _) = outs
    p1, p2, fp = o1.data_ptr(), o2.data_ptr(), f.data_ptr()
    oi, chk_i = guarded1d(4, torch.int32)
    outs.append((oi, chk_i))
    T.call("clipmi_pool_index", s, i64.data_ptr(), 0, S, 2, 1, oi.data_ptr())
    for dt, o in ((F32, o1), (BF16, ob)):
        T.call("clipmi_gather_rows", s, dt, fp, i32.data_ptr(), 0, S, D, o.data_ptr())
        T.call("clipmi_gather_rows", s, dt, fp, None, 0, S, D, o.data_ptr())
        T.call("clipmi_scatter_rows", s, dt, fp, i32.data_ptr(), 0, S, D, o.data_ptr(), 0)
        T.call("clipmi_scatter_rows", s, dt, fp, None, 0, S, D, o.data_ptr(), 1)
        T.call("clipmi_text_embed", s, dt, i64.data_ptr(), fp, fp, o.data_ptr(), 0, S, D, V, oi.data_ptr())
    T.call("clipmi_l2norm_fwd", s, fp, p1, p2, 0, D)
    T.call("clipmi_l2norm_bwd", s, fp, fp, fp, p1, 0, D)
    T.call("clipmi_contrastive_ce_fwd", s, fp, p1, fp, 0, Bg, 0, p2, p2)
    T.call("clipmi_contrastive_ce_bwd", s, fp, fp, fp, None, 0, Bg, 0, 1.0, p1, p2)
    T.call("clipmi_contrastive_ce_fwd_chunk", s, fp, fp, 0, Bg, 0, Bg, 0, p1, p2)
    T.call("clipmi_contrastive_ce_finish", s, fp, fp, 0, p1, p2)
    T.call("clipmi_contrastive_ce_bwd_chunk", s, fp, fp, fp, None, 0, Bg, 0, Bg, 0, 1.0, p1, p2, 0)
    # the token-embedding backward with no row: beta = 1 leaves gtok alone, beta = 0 zeroes it
    ws = _bytes(T._lib.lib().clipmi_text_embed_bwd_ws(0, V), STALE_BYTE)
    T.call("clipmi_text_embed_bwd", s, F32, i64.data_ptr(), fp, 0, D, V, p1, 1, ws.data_ptr(), ws.numel())
    gz, chk_z = guarded(V, D, torch.float32)
    T.call("clipmi_text_embed_bwd", s, BF16, i64.data_ptr(), fp, 0, D, V, gz.data_ptr(), 0, ws.data_ptr(), ws.numel())
    torch.cuda.synchronize()
    for o, chk in outs:
        chk()
        assert untouched(o)
    chk_z()
    assert torch.equal(gz, torch.zeros_like(gz))
