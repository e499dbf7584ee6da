"""The text tower's first-token mode (clipmi_encoder_desc.first_token, towers.TextFirstTokenFn) on the GPU.

The tower is causal, so token 0 attends only to itself; under first-token pooling (model_m.py:102) the other rows
never reach the features or a gradient.  The engine's first-token mode runs token 0's row alone: these tests hold
it to the full engine on the same weights, both measured against the same layers evaluated in fp64 torch.

Bounds.  The first-token error must be <= 2 x the full engine's error, measured in the same test with the metric
of test_gradients_match_reference (max error over max(|ref| of the tensor, 5 % of the group's largest)): both
engines sum the same K products per output, the first-token one in a different tile order.  Three figures are
compared, as that test forms them: the output at row 0, dx at row 0 (each its own group) and the worst gradient
tensor of the gradient group.  Measured figures (MI355X) are recorded in DESIGN.md."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from engine_harness import D, EPS, MODES, errors, inputs, make_mask, make_weights  # noqa: E402
from engine_harness import run_engine as run  # noqa: E402

from clipmi import CLIPWithAdapters, synth  # noqa: E402

L = 2


def run_engine(first, dtype, r32, B, N, weights, mask, x0, dy0, grad_fill=None):
    """The causal engine, full or in its first_token mode: (output at row 0, dx at row 0, gradients)."""
    return run("first_token" if first else "full", dtype, r32, B, N, L, weights, x0, dy0, causal=True, mask=mask,
               grad_fill=grad_fill, row0=True)


def reference(weights, mask, x0, dy0, xdt, dtype):
    """Token 0 through the same layers in fp64 torch (the attention output zeroed where key 0 is masked, as the
    kernels do), from the values the engines read: weights, input and upstream gradient rounded to their dtypes."""
    x = x0[:, 0].to(xdt).double().requires_grad_(True)
    keep = None if mask is None else (mask[:, 0] != 0).double()[:, None]
    ws = [{n: t.double().requires_grad_(True) for n, t in w.items()} for w in weights]
    ln = torch.nn.functional.layer_norm
    h = x
    for w in ws:
        a = ln(h, (D,), w["ln1_w"], w["ln1_b"], EPS)
        v = a @ w["qkv_w"][2 * D:].t() + w["qkv_b"][2 * D:]  # softmax over token 0's one key is 1: O = V
        o = v if keep is None else v * keep
        h = h + o @ w["out_w"].t() + w["out_b"]
        a = ln(h, (D,), w["ln2_w"], w["ln2_b"], EPS)
        p = a @ w["fc1_w"].t() + w["fc1_b"]
        h = h + (p * torch.sigmoid(1.702 * p)) @ w["fc2_w"].t() + w["fc2_b"]
    h.backward(dy0.to(dtype).double())
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
    return h.detach(), x.grad, {f"{l}.{n}": zero(t) for l, w in enumerate(ws) for n, t in w.items()}


@pytest.mark.parametrize("mask_kind", ["null", "ones", "key0"])
@pytest.mark.parametrize("B", [1, 3, 33, 300])
@pytest.mark.parametrize("N", [1, 7, 77])
@pytest.mark.parametrize("mode", list(MODES))
def test_engine_first_token_matches_full_engine(mode, N, B, mask_kind):
    dtype, r32 = MODES[mode]
    xdt = torch.float32 if r32 else dtype
    weights = make_weights(7, dtype, L)
    mask = make_mask(mask_kind, B, N)
    x0, dy0 = inputs(B, N)
    ref = reference(weights, mask, x0, dy0, xdt, dtype)
    e_full = errors(run_engine(False, dtype, r32, B, N, weights, mask, x0, dy0), ref)
    e_ft = errors(run_engine(True, dtype, r32, B, N, weights, mask, x0, dy0), ref)
    print(f"\n[{mode} N={N} B={B} mask={mask_kind}] out/dx/grad err: first-token {e_ft[0]:.3e} {e_ft[1]:.3e} "
          f"{e_ft[2][0]:.3e} ({e_ft[2][1]}); full {e_full[0]:.3e} {e_full[1]:.3e} {e_full[2][0]:.3e} ({e_full[2][1]})")
    assert e_ft[0] <= 2 * e_full[0], ("output", e_ft[0], e_full[0])
    assert e_ft[1] <= 2 * e_full[1], ("dx", e_ft[1], e_full[1])
    assert e_ft[2][0] <= 2 * e_full[2][0], ("gradients", e_ft[2], e_full[2])


@pytest.mark.parametrize("mask_kind", ["null", "key0"])
@pytest.mark.parametrize("B", [3, 300])
@pytest.mark.parametrize("mode", list(MODES))
def test_first_token_backward_leaves_qk_slots_and_accumulates(mode, B, mask_kind):
    """Gradients accumulate: from a sentinel-filled start the q / k slots of qkv_w / qkv_b stay bit-identical (their
    gradient is exactly zero and the engine does not touch them) and every other slot moves by what a zero-filled
    start gives.  after = fl(s + g), so (after - s) - g is within fp32 rounding of the sum: 2^-22 (|s| + |g|)."""
    dtype, r32 = MODES[mode]
    N = 7
    weights = make_weights(11, dtype, L)
    mask = make_mask(mask_kind, B, N)
    x0, dy0 = inputs(B, N, seed=5)
    _, _, g0 = run_engine(True, dtype, r32, B, N, weights, mask, x0, dy0)
    gen = torch.Generator().manual_seed(3)
    fill = {n: (0.5 + torch.rand(g.shape, generator=gen)).cuda() for n, g in g0.items()}
    _, _, g1 = run_engine(True, dtype, r32, B, N, weights, mask, x0, dy0, grad_fill=fill)
    for n, g in g1.items():
        s, z = fill[n], g0[n]
        if n.endswith("qkv_w") or n.endswith("qkv_b"):
            assert torch.equal(g[:2 * D].view(torch.int32), s[:2 * D].view(torch.int32)), n
            assert not z[:2 * D].any(), n
            g, s, z = g[2 * D:], s[2 * D:], z[2 * D:]
        assert z.abs().max() > 0, n
        bound = 2.0 ** -22 * (s.abs() + z.abs())
        assert bool((((g - s) - z).abs() <= bound).all()), n


@pytest.mark.parametrize("B", [33, 300, 1100])  # 1100: >= 1024 tokens, where the weight gradients may split over K
@pytest.mark.parametrize("mode", ["bf16", "bf16_resid32"])
def test_first_token_deferred_reductions_bitwise(mode, B, monkeypatch):
    """CLIPMI_DEFER=0 (every split-K / LayerNorm affine-gradient reduction launched on its own) gives the bits of
    the default (deferred into the next persistent GEMM) in the first-token mode too."""
    dtype, r32 = MODES[mode]
    N = 7
    weights = make_weights(13, dtype, L)
    mask = make_mask("key0", B, N)
    x0, dy0 = inputs(B, N, seed=9)
    monkeypatch.delenv("CLIPMI_DEFER", raising=False)
    out0, dx0, g0 = run_engine(True, dtype, r32, B, N, weights, mask, x0, dy0)
    monkeypatch.setenv("CLIPMI_DEFER", "0")
    out1, dx1, g1 = run_engine(True, dtype, r32, B, N, weights, mask, x0, dy0)
    assert torch.equal(out0, out1) and torch.equal(dx0, dx1)
    assert not [n for n in g0 if not torch.equal(g0[n], g1[n])]


# ---- model ----------------------------------------------------------------------------------------------------
LOGIT_TOL = {"fp32": 1e-3, "bf16x3": 1e-3, "bf16": 0.25}  # test_gpu_model: LOGIT_TOL, BF16_TINY_LOGIT_TOL (tiny preset)


def model_run(golden, monkeypatch, precision, tag, adapters, freeze, first):
    """test_forward_matches_reference / test_gradients_match_reference on the tiny preset: their errors."""
    if first:
        monkeypatch.delenv("CLIPMI_TEXT_FIRST_TOKEN", raising=False)
    else:
        monkeypatch.setenv("CLIPMI_TEXT_FIRST_TOKEN", "0")
    g = golden(f"forward_{tag}.npz")
    m = CLIPWithAdapters("tiny", use_text_adapter=adapters, use_vision_adapter=adapters, use_shared_adapters=False,
                         freeze_clip=freeze, device="cuda", precision=precision, pooling="first")
    b = {k: torch.from_numpy(v).cuda() for k, v in synth.synthetic_batch(m.config, 4, seed=1234).items()}
    out = m(**b)
    out["loss"].backward()
    torch.cuda.synchronize()
    lerr = float(np.abs(out["logits_per_text"].detach().cpu().numpy() - g["logits_per_text"]).max())
    ferr = float(np.abs(out["text_features"].detach().cpu().numpy() - g["text_features"]).max())
    loss_err = abs(out["loss"].item() - float(g["loss"]))
    params = dict(m.named_parameters())
    names = [k[5:] for k in g.files if k.startswith("grad/")]
    assert names
    gmax = max(float(np.abs(g["grad/" + n]).max()) for n in names)
    worst = (0.0, "")
    for n in names:
        assert params[n].grad is not None, n
        ref = g["grad/" + n]
        scale = max(float(np.abs(ref).max()), 0.05 * gmax, 1e-6)
        worst = max(worst, (float(np.abs(params[n].grad.cpu().numpy() - ref).max()) / scale, n))
    with torch.no_grad():
        hs = m.text_hidden_states(b["input_ids"], b["attention_mask"])
    assert tuple(hs.shape) == (4, b["input_ids"].shape[1], m.config.text_config.hidden_size)
    return lerr, ferr, loss_err, worst


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
@pytest.mark.parametrize("tag,adapters,freeze", [("tiny_full_grads", False, False), ("tiny_adapter_grads", True, True)])
def test_model_first_token_matches_reference(golden, monkeypatch, precision, tag, adapters, freeze):
    full = model_run(golden, monkeypatch, precision, tag, adapters, freeze, first=False)
    ft = model_run(golden, monkeypatch, precision, tag, adapters, freeze, first=True)
    print(f"\n[{tag} {precision}] logit / text-feature / loss / worst-grad err: first-token {ft[0]:.3e} {ft[1]:.3e} "
          f"{ft[2]:.3e} {ft[3][0]:.3e} ({ft[3][1]}); full {full[0]:.3e} {full[1]:.3e} {full[2]:.3e} {full[3][0]:.3e} "
          f"({full[3][1]})")
    # the existing tolerances of test_forward_matches_reference and test_gradients_match_reference
    assert ft[0] < LOGIT_TOL[precision]
    assert ft[1] < (1e-4 if precision != "bf16" else 3e-2)
    assert ft[2] < {"fp32": 1e-5, "bf16x3": 3e-5}.get(precision, 2e-2)
    assert ft[3][0] < (2e-4 if precision != "bf16" else 0.2), ft[3]
    # and no worse than twice the full path
    assert ft[0] <= 2 * full[0], ("logits", ft[0], full[0])
    assert ft[3][0] <= 2 * full[3][0], ("gradients", ft[3], full[3])


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_first_token_replay_is_bitwise(precision, monkeypatch):
    """test_deterministic_replay's convention on the first-token path: the same step twice from the same state,
    logits, loss and every gradient bitwise equal but the token embedding's (fp32 atomics: within rounding)."""
    monkeypatch.delenv("CLIPMI_TEXT_FIRST_TOKEN", raising=False)
    runs = []
    for _ in range(2):
        m = CLIPWithAdapters("tiny", freeze_clip=False, use_shared_adapters=False, device="cuda", precision=precision,
                             init_seed=3)
        b = {k: torch.from_numpy(v).cuda() for k, v in synth.synthetic_batch(m.config, 33, seed=7).items()}
        out = m(**b, return_loss=True)
        out["loss"].backward()
        torch.cuda.synchronize()
        runs.append((out["logits_per_image"].detach().clone(), out["loss"].detach().clone(),
                     {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}))
        del m, out
    (l0, s0, g0), (l1, s1, g1) = runs
    assert torch.equal(l0, l1) and torch.equal(s0, s1)
    assert g0.keys() == g1.keys() and len(g0) > 0
    racy = []
    for n in g0:
        if torch.equal(g0[n], g1[n]):
            continue
        d = (g0[n] - g1[n]).abs().max().item() / max(g0[n].abs().max().item(), 1e-30)
        if "token_embedding.weight" in n and d < 1e-5:
            continue
        racy.append((n, d))
    assert not racy, racy
