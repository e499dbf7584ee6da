"""The vision tower's cls_last mode on the GPU: the engine's mode (clipmi_encoder_desc.cls_last: the last layer's
out-projection and MLP on the CLS rows) against the full engine, the model's CLS-pooled path (towers.VisionClsFn)
against the full tower, and the single-query attention entry points (csrc/attention_cls.hip, exported for hosts that
pool one row; the engine keeps the MFMA attention kernels) against fp64 torch.

Kernel bounds are the existing attention tests' for the same dtype (tests/test_gpu_structured.py: TOL, UNIFORM_O,
UNIFORM_LSE and the one-hot tests' one-ulp / 1e-6 bounds; tests/test_gpu_kernels.py test_attention's lse bound), and
every output lives in a guard band (kernel_checks.guarded).

Engine and model bound: the cls_last error is <= 2 x the full path's error in the same case, both measured against
the same reference (the layers in fp64 torch; the committed goldens) with the metric of
tests/test_gpu_first_token.py.  Measured figures (MI355X) are recorded in DESIGN.md: the mode keeps the full mode's
activation bits, so the errors are the full engine's."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import kernel_checks as kc  # noqa: E402
from engine_harness import D, EPS, H, MODES, errors, inputs, make_weights  # noqa: E402
from engine_harness import run_engine as run  # noqa: E402
import test_gpu_structured as sg  # noqa: E402  (the bounds of the structured attention tests)
from kernel_checks import guarded, guarded1d, integer_tensor  # noqa: E402

from clipmi import CLIPWithAdapters, _lib, synth  # noqa: E402
from clipmi import kernels as K  # noqa: E402
from clipmi import towers as T  # noqa: E402
from clipmi._lib import BF16, F32  # noqa: E402

c_vp, c_i64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
_lib.declare("clipmi_attention_cls_fwd", [c_vp, c_int, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_int, c_int, c_int, c_int])
_lib.declare("clipmi_attention_cls_bwd", [c_vp, c_int, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp,
                                          c_i64, c_vp, c_i64, c_int, c_int, c_int, c_int])

DT = {torch.bfloat16: BF16, torch.float32: F32}
LSE_TOL = {torch.bfloat16: 2e-2, torch.float32: 1e-4}  # test_gpu_kernels.test_attention

# ================================================================================================ A. kernels
KERNEL_CASES = [(N, H, B) for N in (1, 2, 63, 64, 65, 197, 257, 577, 4096) for H in (1, 2, 12)
                for B in ((1,) if N == 4096 else (3, 130))]


def run_cls(dtype, q, kv, do, B, H, N):
    """Forward and backward through the entry points.  q is read with a leading dimension of D + 16 and the backward
    writes dq | dK_0 | dV_0 as one [B][3D] operand (as the engine lays it out); every output is guarded."""
    D = H * 64
    s = K.stream()
    qs, _ = guarded(B, D, dtype, D + 16)
    qs.copy_(q)
    o, c1 = guarded(B, D, dtype)
    lse, c2 = guarded1d(B * H, torch.float32)
    T.call("clipmi_attention_cls_fwd", s, DT[dtype], qs.data_ptr(), D + 16, kv.data_ptr(), o.data_ptr(), D,
           lse.data_ptr(), B, H, N, D)
    dkv, c3 = guarded(B * N, 2 * D, dtype)
    dcls, c4 = guarded(B, 3 * D, dtype)
    T.call("clipmi_attention_cls_bwd", s, DT[dtype], qs.data_ptr(), D + 16, kv.data_ptr(), o.data_ptr(), D,
           lse.data_ptr(), do.data_ptr(), D, dkv.data_ptr(), dcls.data_ptr(), 3 * D,
           dcls.data_ptr() + D * dcls.element_size(), 3 * D, B, H, N, D)
    torch.cuda.synchronize()
    for c in (c1, c2, c3, c4):
        c()
    return o, lse.view(B, H), dkv, dcls


def cls_ref(q, kv, do, B, H, N):
    """fp64: (o [B, D], lse [B, H], dkv [B*N, 2D], dq [B, D]) from the values the kernels read."""
    D = H * 64
    qh = q.double().view(B, H, 64)
    k = kv[:, :D].double().view(B, N, H, 64)
    v = kv[:, D:].double().view(B, N, H, 64)
    s = torch.einsum("bhd,bnhd->bhn", qh, k) / 8
    lse = torch.logsumexp(s, -1)
    p = torch.exp(s - lse[..., None])
    o = torch.einsum("bhn,bnhd->bhd", p, v)
    dO = do.double().view(B, H, 64)
    ds = p * (torch.einsum("bhd,bnhd->bhn", dO, v) - (dO * o).sum(-1, keepdim=True))
    dq = torch.einsum("bhn,bnhd->bhd", ds, k) / 8
    dk = torch.einsum("bhn,bhd->bnhd", ds, qh) / 8
    dv = torch.einsum("bhn,bhd->bnhd", p, dO)
    return o.reshape(B, D), lse, torch.cat([dk.reshape(B * N, D), dv.reshape(B * N, D)], 1), dq.reshape(B, D)


def rel(got, ref):
    return float((got.double() - ref).abs().nan_to_num(1e30).max()) / max(float(ref.abs().max()), 1e-30)


def rnd(shape, seed, dtype):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("N,H,B", KERNEL_CASES)
def test_cls_attention_random(N, H, B, dtype):
    D = H * 64
    q, kv, do = rnd((B, D), 21, dtype), rnd((B * N, 2 * D), 22, dtype), rnd((B, D), 23, dtype)
    o, lse, dkv, dcls = run_cls(dtype, q, kv, do, B, H, N)
    oref, lref, dkvref, dqref = cls_ref(q, kv, do, B, H, N)
    tol = sg.TOL[dtype]
    fig = {"O": rel(o, oref), "lse": float((lse.double() - lref).abs().max()), "dK": rel(dkv[:, :D], dkvref[:, :D]),
           "dV": rel(dkv[:, D:], dkvref[:, D:]), "dq": rel(dcls[:, :D], dqref)}
    print(f"\n[N={N} H={H} B={B} {dtype}] " + " ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    assert fig["O"] < tol and fig["lse"] < LSE_TOL[dtype], fig
    if N > 1:  # N = 1: p = 1, so dS, dK and dq are exactly zero in the reference
        assert fig["dK"] < 2 * tol and fig["dq"] < 2 * tol, fig
    else:
        assert float(dkv[:, :D].abs().max()) <= 2 * tol * float(do.abs().max() * q.abs().max()), fig
        assert float(dcls[:, :D].abs().max()) <= 2 * tol * float(do.abs().max() * kv.abs().max()), fig
    assert fig["dV"] < 2 * tol, fig
    # the second copy of row 0's dK | dV is the same bits
    first = dkv.view(B, N, 2 * D)[:, 0]
    assert torch.equal(dcls[:, D:].contiguous().view(torch.uint8), first.contiguous().view(torch.uint8))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("N,H,B", KERNEL_CASES)
def test_cls_attention_uniform(N, H, B, dtype):
    """q = 0: p = 1/N, lse = ln N, o = the column mean of V (UNIFORM_O / UNIFORM_LSE of test_attention_uniform),
    dV_j = dO / N (2 x TOL), dK = 0 exactly and dq = scale sum_j dS_j k_j with dS_j = (dO.v_j - dO.o) / N."""
    D = H * 64
    kv = torch.randn(B * N, 2 * D, generator=torch.Generator().manual_seed(3 * N + 1)).bfloat16().to(dtype).cuda()
    q = torch.zeros(B, D, dtype=dtype, device="cuda")
    do = rnd((B, D), N + 9, dtype)
    o, lse, dkv, dcls = run_cls(dtype, q, kv, do, B, H, N)
    oref, lref, dkvref, dqref = cls_ref(q, kv, do, B, H, N)
    rtol, atol = sg.UNIFORM_O[dtype]
    e_l = float((lse.double() - math.log(N)).abs().max())
    err = (o.double() - oref).abs().nan_to_num(1e30)
    m_rel = float((err / (oref.abs() + atol / rtol)).max())
    e_v = rel(dkv[:, D:], dkvref[:, D:])
    print(f"\n[N={N} H={H} B={B} {dtype}] lse {e_l:.3e} O (units of rtol) {m_rel:.3e} dV {e_v:.3e}")
    assert e_l <= sg.UNIFORM_LSE, e_l
    assert bool((err <= rtol * oref.abs() + atol).all()), m_rel
    assert e_v < 2 * sg.TOL[dtype], e_v
    assert not bool(dkv[:, :D].any())  # dK_j = scale dS_j q with q = 0
    if N > 1:
        assert rel(dcls[:, :D], dqref) < 2 * sg.TOL[dtype]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("N,H,B", KERNEL_CASES)
def test_cls_attention_one_dominating_key(N, H, B, dtype):
    """q = +-2 per element and k_j = 2 q at one key j per (b, h), every other k = 0: s_j = 64 against 0 elsewhere, so
    the other keys carry (N - 1) e^-64 < 2^-40 of the weight.  o = v_j and dV_j = dO within one ulp of the output
    dtype (integer v, dO), every other dV, dq and dK within 1e-6 c (c = 2, the key's scale): the bounds of
    test_attention_onehot_*.  Key j is the last key for (b, h) = (0, 0) and walks the sequence for the others."""
    D = H * 64
    g = torch.Generator().manual_seed(N + 31)
    q = (torch.randint(0, 2, (B, H, 64), generator=g) * 4 - 2).double()
    j = (torch.arange(B)[:, None] * 7 + torch.arange(H)[None, :] * 3 + N - 1) % N  # [B, H]
    k = torch.zeros(B, N, H, 64, dtype=torch.float64)
    k.scatter_(1, j[:, None, :, None].expand(B, 1, H, 64), (2 * q)[:, None])
    v = integer_tensor((B, N, H, 64), -4, 4, torch.float64, N + 32)
    do = integer_tensor((B, D), -4, 4, dtype, N + 33, "cuda")
    kv = torch.cat([k.reshape(B * N, D), v.reshape(B * N, D)], 1).to(dtype).cuda()
    leak = (N - 1) * math.exp(-64.0)
    assert leak < kc.LEAK_MAX
    o, lse, dkv, dcls = run_cls(dtype, q.reshape(B, D).to(dtype).cuda(), kv, do, B, H, N)
    jj = j.cuda()[:, None, :, None].expand(B, 1, H, 64)
    vsel = torch.gather(v.cuda(), 1, jj).reshape(B, D)
    e_o = (o.double() - vsel).abs().nan_to_num(1e30) - (kc.ulp(vsel, dtype) + 8 * leak + 2.0 ** -40)
    assert float(e_o.max()) <= 0, ("O", float(e_o.max()))
    assert float((lse.double() - 64.0).abs().max()) <= 1e-3
    dvref = torch.zeros(B, N, H, 64, dtype=torch.float64, device="cuda")
    dvref.scatter_(1, jj, do.double().view(B, 1, H, 64))
    err = (dkv[:, D:].double().view(B, N, H, 64) - dvref).abs().nan_to_num(1e30)
    e_v = float((err / (sg._int_ulp(dvref, dtype) + 4 * N * leak)).max())
    e_qk = max(float(dkv[:, :D].double().abs().nan_to_num(1e30).max()),
               float(dcls[:, :D].double().abs().nan_to_num(1e30).max())) / 2.0
    assert e_v <= 1.0, ("dV", e_v)
    assert e_qk <= 1e-6, ("dq/dK", e_qk)


# ================================================================================================ B. engine
def run_engine(cls, dtype, r32, B, N, L, weights, x0, dy0, grad_fill=None, chunks=None):
    """The non-causal engine, full or in its cls_last mode: (output at the CLS row, dx [B, N, D], gradients)."""
    return run("cls_last" if cls else "full", dtype, r32, B, N, L, weights, x0, dy0, grad_fill=grad_fill,
               chunks=chunks)


def reference(weights, x0, dy0, xdt, dtype, B, N):
    """The same layers in fp64 torch on every row, the loss reading the CLS row of the last layer's output; from the
    values the engines read (weights, input and upstream gradient rounded to their dtypes)."""
    x = x0.to(xdt).double().requires_grad_(True)
    ws = [{n: t.double().requires_grad_(True) for n, t in w.items()} for w in weights]
    ln = torch.nn.functional.layer_norm
    h = x
    for w in ws:
        a = ln(h, (D,), w["ln1_w"], w["ln1_b"], EPS)
        qkv = (a @ w["qkv_w"].t() + w["qkv_b"]).view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)  # [3, B, H, N, 64]
        p = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) / 8, -1)
        o = (p @ qkv[2]).permute(0, 2, 1, 3).reshape(B, N, D)
        h = h + o @ w["out_w"].t() + w["out_b"]
        a = ln(h, (D,), w["ln2_w"], w["ln2_b"], EPS)
        pre = a @ w["fc1_w"].t() + w["fc1_b"]
        h = h + (pre * torch.sigmoid(1.702 * pre)) @ w["fc2_w"].t() + w["fc2_b"]
    out = h[:, 0]
    out.backward(dy0.to(dtype).double())
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
    return out.detach(), x.grad, {f"{l}.{n}": zero(t) for l, w in enumerate(ws) for n, t in w.items()}


@pytest.mark.parametrize("B", [1, 3, 33, 300])
@pytest.mark.parametrize("N", [1, 2, 50, 197])
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("mode", list(MODES))
def test_engine_cls_last_matches_full_engine(mode, L, N, B):
    dtype, r32 = MODES[mode]
    xdt = torch.float32 if r32 else dtype
    weights = make_weights(7, dtype, L)
    x0, dy0 = inputs(B, N)
    ref = reference(weights, x0, dy0, xdt, dtype, B, N)
    e_full = errors(run_engine(False, dtype, r32, B, N, L, weights, x0, dy0), ref)
    e_cls = errors(run_engine(True, dtype, r32, B, N, L, weights, x0, dy0), ref)
    print(f"\n[{mode} L={L} N={N} B={B}] out/dx/grad err: cls_last {e_cls[0]:.3e} {e_cls[1]:.3e} {e_cls[2][0]:.3e} "
          f"({e_cls[2][1]}); full {e_full[0]:.3e} {e_full[1]:.3e} {e_full[2][0]:.3e} ({e_full[2][1]})")
    assert e_cls[0] <= 2 * e_full[0], ("output", e_cls[0], e_full[0])
    assert e_cls[1] <= 2 * e_full[1], ("dx", e_cls[1], e_full[1])
    assert e_cls[2][0] <= 2 * e_full[2][0], ("gradients", e_cls[2], e_full[2])


@pytest.mark.parametrize("mode", list(MODES))
def test_cls_last_backward_accumulates(mode):
    """Gradients accumulate: from a filled start every slot moves by what a zero-filled start gives.
    after = fl(s + g), so (after - s) - g is within fp32 rounding of the sum: 2^-22 (|s| + |g|)."""
    dtype, r32 = MODES[mode]
    B, N, L = 33, 50, 2
    weights = make_weights(11, dtype, L)
    x0, dy0 = inputs(B, N, seed=5)
    _, dx0, g0 = run_engine(True, dtype, r32, B, N, L, weights, x0, dy0)
    gen = torch.Generator().manual_seed(3)
    fill = {n: (0.5 + torch.rand(g.shape, generator=gen)).cuda() for n, g in g0.items()}
    _, dx1, g1 = run_engine(True, dtype, r32, B, N, L, weights, x0, dy0, grad_fill=fill)
    assert torch.equal(dx0, dx1)
    for n, g in g1.items():
        s, z = fill[n], g0[n]
        assert z.abs().max() > 0, n
        assert bool((((g - s) - z).abs() <= 2.0 ** -22 * (s.abs() + z.abs())).all()), n


@pytest.mark.parametrize("mode", list(MODES))
def test_cls_last_chunked_backward_is_bitwise(mode):
    """clipmi_encoder_bwd_layers in two calls (only the first sees the compact dx) gives the single call's bits."""
    dtype, r32 = MODES[mode]
    B, N, L = 33, 50, 2
    weights = make_weights(13, dtype, L)
    x0, dy0 = inputs(B, N, seed=9)
    out0, dx0, g0 = run_engine(True, dtype, r32, B, N, L, weights, x0, dy0)
    out1, dx1, g1 = run_engine(True, dtype, r32, B, N, L, weights, x0, dy0, chunks=[(2, 1), (1, 0)])
    assert torch.equal(out0, out1) and torch.equal(dx0, dx1)
    assert not [n for n in g0 if not torch.equal(g0[n], g1[n])]


@pytest.mark.parametrize("B,N", [(33, 50), (1100, 2)])  # both have >= 1024 tokens: the weight gradients may split
@pytest.mark.parametrize("mode", ["bf16", "bf16_resid32"])
def test_cls_last_deferred_reductions_bitwise(mode, B, N, monkeypatch):
    """CLIPMI_DEFER=0 (every split-K / LayerNorm affine-gradient reduction launched on its own) gives the bits of
    the default (deferred into the next persistent GEMM), and a replay gives the same bits again."""
    dtype, r32 = MODES[mode]
    weights = make_weights(17, dtype, 2)
    x0, dy0 = inputs(B, N, seed=2)
    monkeypatch.delenv("CLIPMI_DEFER", raising=False)
    runs = [run_engine(True, dtype, r32, B, N, 2, weights, x0, dy0) for _ in range(2)]
    monkeypatch.setenv("CLIPMI_DEFER", "0")
    runs.append(run_engine(True, dtype, r32, B, N, 2, weights, x0, dy0))
    for out, dx, g in runs[1:]:
        assert torch.equal(runs[0][0], out) and torch.equal(runs[0][1], dx)
        assert not [n for n in g if not torch.equal(runs[0][2][n], g[n])]


# ================================================================================================ C. model
def model_run(golden, monkeypatch, preset, tag, B, precision, adapters, freeze, cls):
    """Logit / image-feature errors against the golden, and the worst gradient error where it has gradients."""
    if cls:
        monkeypatch.delenv("CLIPMI_VISION_CLS_LAST", raising=False)
    else:
        monkeypatch.setenv("CLIPMI_VISION_CLS_LAST", "0")
    g = golden(f"forward_{tag}.npz")
    m = CLIPWithAdapters(preset, use_text_adapter=adapters, use_vision_adapter=adapters, use_shared_adapters=False,
                         freeze_clip=freeze, device="cuda", precision=precision)
    b = {k: torch.from_numpy(v).cuda() for k, v in synth.synthetic_batch(m.config, B, seed=1234).items()}
    out = m(**b)
    out["loss"].backward()
    torch.cuda.synchronize()
    lerr = float(np.abs(out["logits_per_text"].detach().cpu().numpy() - g["logits_per_text"]).max())
    ferr = float(np.abs(out["image_features"].detach().cpu().numpy() - g["image_features"]).max())
    params = dict(m.named_parameters())
    names = [k[5:] for k in g.files if k.startswith("grad/")]
    worst = (0.0, "")
    if names:
        gmax = max(float(np.abs(g["grad/" + n]).max()) for n in names)
        for n in names:
            assert params[n].grad is not None, n
            ref = g["grad/" + n]
            scale = max(float(np.abs(ref).max()), 0.05 * gmax, 1e-6)
            worst = max(worst, (float(np.abs(params[n].grad.cpu().numpy() - ref).max()) / scale, n))
    grads = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    with torch.no_grad():
        hs = m.vision_hidden_states(b["pixel_values"])
        feats = m.get_image_features(b["pixel_values"])
    return lerr, ferr, worst, grads, hs, feats


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("preset,tag,B,adapters,freeze", [("tiny", "tiny_full_grads", 4, False, False),
                                                          ("tiny", "tiny_adapter_grads", 4, True, True),
                                                          ("B/32", "b32", 8, True, True)])
def test_model_cls_last_matches_reference(golden, monkeypatch, preset, tag, B, precision, adapters, freeze):
    """One training step (forward, loss, backward) with the switch off and on against the committed goldens (the
    tiny goldens hold B = 4, the B/32 one B = 8 without gradients): logits, image features and the worst gradient
    within 2 x the full path's error; vision_hidden_states is not touched by the switch (bitwise)."""
    full = model_run(golden, monkeypatch, preset, tag, B, precision, adapters, freeze, cls=False)
    cl = model_run(golden, monkeypatch, preset, tag, B, precision, adapters, freeze, cls=True)
    print(f"\n[{tag} {precision}] logit / image-feature / worst-grad err: cls_last {cl[0]:.3e} {cl[1]:.3e} "
          f"{cl[2][0]:.3e} ({cl[2][1]}); full {full[0]:.3e} {full[1]:.3e} {full[2][0]:.3e} ({full[2][1]})")
    assert cl[0] <= 2 * full[0], ("logits", cl[0], full[0])
    assert cl[1] <= 2 * full[1], ("image features", cl[1], full[1])
    assert cl[2][0] <= 2 * full[2][0], ("gradients", cl[2], full[2])
    assert cl[3].keys() == full[3].keys() and len(cl[3]) > 0
    assert tuple(cl[4].shape) == tuple(full[4].shape) and cl[4].dim() == 3 and cl[4].shape[1] > 1
    assert torch.equal(cl[4], full[4])  # vision_hidden_states keeps the full tower
    assert tuple(cl[5].shape) == tuple(full[5].shape)  # inference takes the pooled form too
