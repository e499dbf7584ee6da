"""Multi-positive contrastive loss on the GPU (csrc/contrastive_keys.hip, towers.KeyedContrastiveFn, the model's
pair_keys and the trainer's positives switch).

The oracle is the definition restated in fp64 torch (tests/test_cpu_multipositive.py: masks from key equality,
logsumexp minus the mask-weighted mean, autograd for the gradients).  Tolerances are those of
test_contrastive_fn_matches_torch / test_contrastive_streamed_matches_materialised: |loss - ref| < 1e-5 max(1, |ref|),
rel < 1e-4 on the feature gradients (max-abs difference over max-abs of the reference), 1e-4 max(1, |ref|) on the
logit_scale gradient.  With all keys distinct the keyed path must be the unkeyed one bit for bit."""
import math
import os

import numpy as np
import pytest
import torch

from kernel_checks import guarded, guarded1d
from test_cpu_multipositive import oracle_loss, oracle_rows

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN100 = math.log(100.0)


def rnd(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float32).cuda()


def rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


class _A:  # minimal arena stand-in for the logit_scale gradient
    def __init__(self):
        self.grad = torch.zeros(64, device="cuda")

    def prepare_grads(self):
        pass

    def ptr(self, name, buf):
        return buf.data_ptr()


def run_fn(t0, i0, keys, chunk, monkeypatch, feature_term=True, ls0=LN100):
    """ContrastiveFn (keys None) or KeyedContrastiveFn forward + backward; chunk None: materialised.
    Returns (loss, dt, di, dls) as device tensors."""
    from clipmi import towers as T
    if chunk is None:
        monkeypatch.delenv("CLIPMI_CE_CHUNK", raising=False)
    else:
        monkeypatch.setenv("CLIPMI_CE_CHUNK", str(chunk))
    t = t0.clone().requires_grad_(True)
    i = i0.clone().requires_grad_(True)
    ls = torch.tensor(ls0, device="cuda", requires_grad=True)
    ar = _A()
    if keys is None:
        loss, th, ih, lt, li = T.ContrastiveFn.apply(t, i, ls, None, True, ar)
    else:
        loss, th, ih, lt, li = T.KeyedContrastiveFn.apply(t, i, ls, keys, None, True, ar)
    streamed = chunk is not None and t0.shape[0] > chunk
    assert (lt is None) == streamed
    total = loss + (th * th.detach()).sum() * 1e-3 if feature_term else loss  # a feature-output gradient too
    total.backward()
    return loss.detach(), t.grad, i.grad, ar.grad[0].clone()


def run_oracle(t0, i0, keys, feature_term=True, ls0=LN100):
    t = t0.double().cpu().requires_grad_(True)
    i = i0.double().cpu().requires_grad_(True)
    ls = torch.tensor(ls0, dtype=torch.float64, requires_grad=True)
    loss, tn, inn = oracle_loss(t, i, ls, keys.cpu())
    total = loss + (tn * tn.detach()).sum() * 1e-3 if feature_term else loss
    total.backward()
    return loss.detach(), t.grad, i.grad, ls.grad


def assert_close(got, ref):
    (l1, t1, i1, s1), (l0, t0, i0, s0) = got, ref
    l1, s1, l0, s0 = l1.item(), s1.item(), l0.item(), s0.item()
    print(f"loss {l1:.7f} ref {l0:.7f} diff {abs(l1 - l0):.2e}; rel dt {rel(t1.cpu(), t0):.2e} di "
          f"{rel(i1.cpu(), i0):.2e}; dls {s1:.6e} ref {s0:.6e}")
    assert abs(l1 - l0) < 1e-5 * max(1.0, abs(l0))
    assert rel(t1.cpu(), t0) < 1e-4
    assert rel(i1.cpu(), i0) < 1e-4
    assert abs(s1 - s0) < 1e-4 * max(1.0, abs(s0))


def distinct_keys(B, kind):
    if kind == "arange":
        return torch.arange(B, dtype=torch.int64, device="cuda")
    g = torch.Generator().manual_seed(B)
    # up to 1.7e17 in magnitude, both signs, low and high words both in use
    k = (torch.randperm(B, generator=g) - B // 2) * 0x9E3779B97F4A + torch.randperm(B, generator=g) * (1 << 33) + 17
    assert len(set(k.tolist())) == B
    return k.cuda()


# ---- 1. reduction to the existing loss, bit for bit ------------------------------------------------
_UNKEYED = {}


@pytest.mark.parametrize("kind", ["arange", "large"])
@pytest.mark.parametrize("chunk", [None, 1, 33, 333])
@pytest.mark.parametrize("B,E", [(7, 64), (130, 64), (1000, 512)])
def test_distinct_keys_reduce_to_unkeyed_loss_bitwise(B, E, chunk, kind, monkeypatch):
    t, i = rnd((B, E), 40 + B), rnd((B, E), 41 + B)
    if (B, chunk) not in _UNKEYED:
        _UNKEYED[(B, chunk)] = run_fn(t, i, None, chunk, monkeypatch)
    ref = _UNKEYED[(B, chunk)]
    got = run_fn(t, i, distinct_keys(B, kind), chunk, monkeypatch)
    for name, a, b in zip(("loss", "t.grad", "i.grad", "logit_scale.grad"), got, ref):
        assert torch.equal(a, b), (name, (a - b).abs().max().item())


# ---- 2. against the fp64 oracle -------------------------------------------------------------------
CASES = [(7, 64, 3), (130, 64, 7), (130, 64, 1), (257, 128, 7), (1000, 512, 35)]


def case_inputs(B, E, nk):
    g = torch.Generator().manual_seed(100 * B + nk)
    keys = torch.randint(0, nk, (B,), generator=g)
    return rnd((B, E), 50 + B), rnd((B, E), 51 + B), keys.cuda()


@pytest.mark.parametrize("B,E,nk", CASES)
def test_keyed_loss_matches_fp64_oracle(B, E, nk, monkeypatch):
    t, i, keys = case_inputs(B, E, nk)
    assert_close(run_fn(t, i, keys, None, monkeypatch), run_oracle(t, i, keys))


def test_int32_keys_through_the_model_path_match_int64(monkeypatch):
    """as_pair_keys widens int32 keys; the loss is that of the same int64 keys."""
    from clipmi.losses import as_pair_keys
    t, i, keys = case_inputs(7, 64, 3)
    k32 = as_pair_keys(keys.to(torch.int32), 7, "cuda")
    a, b = run_fn(t, i, k32, None, monkeypatch), run_fn(t, i, keys, None, monkeypatch)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- 3. key width and sign ------------------------------------------------------------------------
def abi_fwd(S, ls, keys_all, label0):
    """clipmi_contrastive_keyed_fwd on cosines S [B, Bg]; outputs inside guard bands.  Returns L, lse, ce, winv."""
    from clipmi import kernels as kern
    from clipmi import towers as T
    B, Bg = S.shape
    L, ckL = guarded(B, Bg, torch.float32)
    lse, ck1 = guarded1d(B, torch.float32)
    ce, ck2 = guarded1d(B, torch.float32)
    winv, ck3 = guarded1d(B, torch.float32)
    T.call("clipmi_contrastive_keyed_fwd", kern.stream(), S.data_ptr(), L.data_ptr(), ls.data_ptr(),
           keys_all.data_ptr(), B, Bg, label0, lse.data_ptr(), ce.data_ptr(), winv.data_ptr())
    torch.cuda.synchronize()
    for ck in (ckL, ck1, ck2, ck3):
        ck()
    return L, lse, ce, winv


def test_keys_compare_all_64_bits_and_the_sign(monkeypatch):
    """Keys that differ only above bit 32 or only in sign are different keys; equal negative keys are one group."""
    hi = 1 << 32
    keys = torch.tensor([5, 5 + hi, 5, -5, -5, 5 + 2 * hi, -5 - hi], dtype=torch.int64)
    counts = torch.tensor([2, 1, 2, 2, 2, 1, 1], dtype=torch.float64)
    t, i = rnd((7, 64), 60), rnd((7, 64), 61)
    tn = (t / t.norm(dim=-1, keepdim=True)).contiguous()
    inn = (i / i.norm(dim=-1, keepdim=True)).contiguous()
    S = (tn @ inn.t()).contiguous()
    ls = torch.tensor([LN100], device="cuda")
    L, lse, ce, winv = abi_fwd(S, ls, keys.cuda(), 0)
    lse0, ce0, winv0 = oracle_rows(S.double().cpu() * ls.double().cpu().exp(), keys, 0)
    assert torch.equal(winv0, 1.0 / counts)
    assert torch.equal(winv.cpu(), (1.0 / counts).float())
    assert (ce.cpu().double() - ce0).abs().max().item() < 1e-5 * max(1.0, ce0.abs().max().item())
    assert_close(run_fn(t, i, keys.cuda(), None, monkeypatch), run_oracle(t, i, keys))


# ---- 4. streamed equals materialised ---------------------------------------------------------------
@pytest.mark.parametrize("B,E,nk,chunk", [(130, 64, 7, 1), (130, 64, 7, 33), (1000, 512, 35, 333)])
def test_keyed_streamed_matches_materialised(B, E, nk, chunk, monkeypatch):
    """Groups span chunk borders and some chunks hold no positive of a row (chunk 1: most of them).  Also against
    the oracle, at the oracle's tolerances."""
    t, i, keys = case_inputs(B, E, nk)
    (l0, t0, i0, s0) = run_fn(t, i, keys, None, monkeypatch)
    got = run_fn(t, i, keys, chunk, monkeypatch)
    (l1, t1, i1, s1) = got
    l0, l1, s0, s1 = l0.item(), l1.item(), s0.item(), s1.item()
    print(f"loss diff {abs(l1 - l0):.2e} rel dt {rel(t1, t0):.2e} di {rel(i1, i0):.2e} dls diff {abs(s1 - s0):.2e}")
    assert abs(l1 - l0) < 1e-5 * max(1.0, abs(l0))
    assert rel(t1, t0) < 1e-5
    assert rel(i1, i0) < 1e-5
    assert abs(s1 - s0) < 1e-5 * max(1.0, abs(s0))
    assert_close(got, run_oracle(t, i, keys))


@pytest.mark.parametrize("chunk", [130, 131, 8192])
def test_keyed_one_chunk_over_the_batch_is_the_materialised_path_bitwise(chunk, monkeypatch):
    t, i, keys = case_inputs(130, 64, 7)
    a, b = run_fn(t, i, keys, None, monkeypatch), run_fn(t, i, keys, chunk, monkeypatch)
    for name, x, y in zip(("loss", "t.grad", "i.grad", "logit_scale.grad"), a, b):
        assert torch.equal(x, y), name


# ---- 5. label offset, through the C ABI ------------------------------------------------------------
def offset_case():
    """B = 5 rows at label0 = 9 of Bg = 20; key 3 sits on columns 2, 10, 12, 19 and key 8 on 7, 8, 9, 13, 14: both
    groups have members before, inside and after the local block [9, 14); the other local row (11) is alone."""
    B, Bg, lab0 = 5, 20, 9
    keys = torch.arange(100, 100 + Bg, dtype=torch.int64)
    keys[[2, 10, 12, 19]] = 3
    keys[[7, 8, 9, 13, 14]] = 8
    g = torch.Generator().manual_seed(77)
    S = (torch.rand(B, Bg, generator=g) * 2 - 1).float()
    ls = torch.tensor([LN100], dtype=torch.float32)
    gout = torch.tensor([0.75], dtype=torch.float32)
    norm = 1.0 / (2 * Bg)
    Ld = (S.double() * ls.double().exp()).requires_grad_(True)
    lse, ce, winv = oracle_rows(Ld, keys, lab0)
    (ce.sum() * gout.double() * norm).backward()
    dL = Ld.grad
    dS = dL * ls.double().exp()
    dls = (dL * (Ld.detach() - lse.detach()[:, None])).sum(1)
    assert winv.tolist() == [1 / 5, 1 / 4, 1.0, 1 / 4, 1 / 5]
    return B, Bg, lab0, keys, S, ls, gout, norm, lse.detach(), ce.detach(), winv, dS, dls


def check_rows(lse, ce, winv, dS, dls, ref):
    lse0, ce0, winv0, dS0, dls0 = ref
    assert torch.equal(winv.cpu(), winv0.float())
    assert (lse.cpu().double() - lse0).abs().max().item() < 1e-5 * max(1.0, lse0.abs().max().item())
    assert (ce.cpu().double() - ce0).abs().max().item() < 1e-5 * max(1.0, ce0.abs().max().item())
    assert rel(dS.cpu(), dS0) < 1e-4
    assert (dls.cpu().double() - dls0).abs().max().item() < 1e-4 * max(1.0, dls0.abs().max().item())


def test_label_offset_materialised_kernels_in_guard_bands():
    from clipmi import kernels as kern
    from clipmi import towers as T
    B, Bg, lab0, keys, S, ls, gout, norm, *ref = offset_case()
    Sd, lsd, gd, kd = S.cuda(), ls.cuda(), gout.cuda(), keys.cuda()
    L, lse, ce, winv = abi_fwd(Sd, lsd, kd, lab0)
    dS, ck1 = guarded(B, Bg, torch.float32)
    dls, ck2 = guarded1d(B, torch.float32)
    T.call("clipmi_contrastive_keyed_bwd", kern.stream(), L.data_ptr(), lse.data_ptr(), winv.data_ptr(), lsd.data_ptr(),
           gd.data_ptr(), kd.data_ptr(), B, Bg, lab0, norm, dS.data_ptr(), dls.data_ptr())
    torch.cuda.synchronize()
    ck1()
    ck2()
    check_rows(lse, ce, winv, dS, dls, ref)


def test_label_offset_chunk_kernels_in_guard_bands():
    """C = 6: chunks of 6, 6, 6, 2 columns; the local block [9, 14) spans two of them."""
    from clipmi import kernels as kern
    from clipmi import towers as T
    B, Bg, lab0, keys, S, ls, gout, norm, *ref = offset_case()
    lsd, gd, kd = ls.cuda(), gout.cuda(), keys.cuda()
    s = kern.stream()
    C = 6
    run, ckr = guarded(B, 4, torch.float32)
    lse, ck1 = guarded1d(B, torch.float32)
    ce, ck2 = guarded1d(B, torch.float32)
    winv, ck3 = guarded1d(B, torch.float32)
    dls, ck4 = guarded1d(B, torch.float32)
    chunks = [(c0, S[:, c0:c0 + C].contiguous().cuda()) for c0 in range(0, Bg, C)]
    for c0, Sc in chunks:
        T.call("clipmi_contrastive_keyed_fwd_chunk", s, Sc.data_ptr(), lsd.data_ptr(), kd.data_ptr(), B, Sc.shape[1],
               c0, Bg, lab0, run.data_ptr())
    T.call("clipmi_contrastive_keyed_finish", s, run.data_ptr(), B, lse.data_ptr(), ce.data_ptr(), winv.data_ptr())
    dS = torch.empty(B, Bg)
    checks = [ckr, ck1, ck2, ck3, ck4]
    for n, (c0, Sc) in enumerate(chunks):
        d, ck = guarded(B, Sc.shape[1], torch.float32)
        T.call("clipmi_contrastive_keyed_bwd_chunk", s, Sc.data_ptr(), lse.data_ptr(), winv.data_ptr(), lsd.data_ptr(),
               gd.data_ptr(), kd.data_ptr(), B, Sc.shape[1], c0, Bg, lab0, norm, d.data_ptr(), dls.data_ptr(),
               1 if n else 0)
        torch.cuda.synchronize()
        checks.append(ck)
        dS[:, c0:c0 + Sc.shape[1]] = d.cpu()
    for ck in checks:
        ck()
    check_rows(lse, ce, winv, dS, dls, ref)


# ---- 6. closed form -------------------------------------------------------------------------------
def test_all_equal_keys_and_features_give_ln_bg(monkeypatch):
    """Every pair one group and every feature row the same unit vector: all logits are equal, so lse = l + ln Bg,
    the positive mean is l, the loss is ln Bg and softmax = 1 / Bg = 1 / |P| everywhere: no gradient.
    logit_scale = 0 (logits of exactly 1): the bound 1e-6 ln Bg = 4.9e-6 is then ten fp32 spacings of lse
    (4.8e-7 at 5.9), where at ln 100 it would be below one spacing of lse (7.6e-6 at 105) and test the number
    format instead of the kernel."""
    Bg, E = 130, 64
    x = torch.zeros(Bg, E, device="cuda")
    x[:, 3] = 1.0
    keys = torch.full((Bg,), -7, dtype=torch.int64, device="cuda")
    loss, dt, di, dls = run_fn(x, x, keys, None, monkeypatch, feature_term=False, ls0=0.0)
    print(f"loss {loss.item():.8f} ln Bg {math.log(Bg):.8f}; max |dt| {dt.abs().max().item():.2e} "
          f"|di| {di.abs().max().item():.2e}")
    assert abs(loss.item() - math.log(Bg)) < 1e-6 * math.log(Bg)
    assert dt.abs().max().item() <= 1e-6 and di.abs().max().item() <= 1e-6


# ---- 7. hash --------------------------------------------------------------------------------------
def test_row_hash64_matches_python_fnv1a():
    from clipmi.losses import caption_keys, fnv1a64
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, 49408, (9, 77), generator=g)
    ids[0, :5] = torch.tensor([0, 49407, 1 << 31, (1 << 31) + 12345, (1 << 62) + 3])
    ids[1, 76] = 49407
    ids[2] = ids[1]                      # two equal rows
    ids[3] = ids[1]
    ids[3, 76] = 49406                   # differs in the last token only
    ids[4, 10] = -1                      # all 64 bits set
    got = caption_keys(ids.cuda()).cpu()
    assert got.dtype == torch.int64
    assert got.tolist() == [fnv1a64(row) for row in ids.tolist()]
    assert got[1] == got[2] and got[1] != got[3]
    assert len(set(got.tolist())) == 8
    assert torch.equal(caption_keys(ids.to(torch.int32)[5:].cuda()).cpu(), got[5:])  # narrower ids, same keys


# ---- 8. model and trainer -------------------------------------------------------------------------
KEYS8 = [0, 0, 1, 1, 2, 2, 3, 3]
EMO8 = ["fear", "fear", "anger", "anger", "neutral", "neutral", "disgust", "disgust"]


def tiny_model():
    """pooling="eos": under the reference's first-token pooling (quirk Q1) every text row is the same vector, and then
    the keyed and the diagonal loss have the same value (sum_i c_i = sum_i mean_{P_i} c_j over whole groups; only
    the gradients differ), so a test that the keys reach the loss could not tell them apart."""
    from clipmi import CLIPWithAdapters
    return CLIPWithAdapters("tiny", use_shared_adapters=False, device="cuda:0", precision="fp32", pooling="eos")


def tiny_batch(m, B=8):
    from clipmi import synth
    return {k: torch.from_numpy(v).cuda() for k, v in synth.synthetic_batch(m.config, B, seed=21).items()}


def test_model_pair_keys_loss_matches_oracle_on_its_features():
    m = tiny_model()
    b = tiny_batch(m)
    plain = m(**b)
    for keys in (KEYS8, torch.tensor(KEYS8), torch.tensor(KEYS8, dtype=torch.int32).cuda()):
        out = m(**b, pair_keys=keys)
        ref = oracle_loss(out["text_features"].detach().double().cpu(), out["image_features"].detach().double().cpu(),
                          m.clip.logit_scale.detach().double().cpu(), torch.tensor(KEYS8))[0].item()
        assert abs(out["loss"].item() - ref) < 1e-5 * max(1.0, abs(ref))
        for k in ("logits_per_text", "logits_per_image", "text_features", "image_features"):
            assert torch.equal(out[k], plain[k])  # the logits outputs do not depend on the keys
    assert abs(plain["loss"].item() - ref) > 1e-3  # and the keyed loss is another loss
    assert torch.equal(m(**b, pair_keys=None)["loss"], plain["loss"])


def _step(positives, batch, tmp_path, pair_keys=None):
    """One optimizer step of a fresh tiny trainer; returns (loss, parameters after the step)."""
    from clipmi import CLIPAdapterTrainer
    m = tiny_model()
    kw = {} if positives == "absent" else {"positives": positives}
    tr = CLIPAdapterTrainer(m, [batch], learning_rate=1e-3, output_dir=str(tmp_path), **kw)
    if pair_keys is not None:  # the keys by hand: the trainer's step with the model's own keyword
        fwd = m.forward
        m.forward = lambda **a: fwd(**a, pair_keys=pair_keys)
    loss = tr.train_step(batch, 0, 4)
    torch.cuda.synchronize()
    return loss.detach().clone(), {n: p.detach().clone() for n, p in m.named_parameters()}, tr


def test_trainer_positives_switch(tmp_path):
    from clipmi.losses import keys_from_strings
    m0 = tiny_model()
    tensors = tiny_batch(m0)
    batch = dict(tensors, emotion=list(EMO8))
    l_emo, p_emo, tr = _step("emotion", batch, tmp_path)
    l_hand, p_hand, _ = _step(None, tensors, tmp_path, pair_keys=keys_from_strings(EMO8))
    assert torch.equal(l_emo, l_hand)
    assert all(torch.equal(p_emo[n], p_hand[n]) for n in p_emo)
    l_fn, p_fn, _ = _step(lambda b: KEYS8, batch, tmp_path)  # a callable; the same groups under other key values
    assert torch.equal(l_fn, l_emo) and all(torch.equal(p_fn[n], p_emo[n]) for n in p_emo)
    # positives=None: the step of a trainer that was never told about positives, bit for bit
    l_none, p_none, _ = _step(None, batch, tmp_path)
    l_abs, p_abs, _ = _step("absent", tensors, tmp_path)
    assert torch.equal(l_none, l_abs) and all(torch.equal(p_none[n], p_abs[n]) for n in p_abs)
    assert not torch.equal(l_none, l_emo)
    assert any(not torch.equal(p_none[n], p_emo[n]) for n in p_emo)
    # evaluate() passes the keys too: the validation loss of the keyed model is the keyed loss
    tr.val_dataloader = [batch]
    with torch.no_grad():
        ref = tr.model(**tensors, pair_keys=keys_from_strings(EMO8))["loss"].item()
    assert tr.evaluate() == ref


def test_trainer_positives_caption_hashes_input_ids(tmp_path):
    """positives="caption": rows 0 / 1 and 2 / 3 carry the same caption; the step is that of those keys by hand."""
    m0 = tiny_model()
    batch = tiny_batch(m0, 4)
    for k in ("input_ids", "attention_mask"):
        batch[k][1] = batch[k][0]
        batch[k][3] = batch[k][2]
    l_cap, p_cap, _ = _step("caption", batch, tmp_path)
    l_hand, p_hand, _ = _step(None, batch, tmp_path, pair_keys=[4, 4, 9, 9])
    assert torch.equal(l_cap, l_hand) and all(torch.equal(p_cap[n], p_hand[n]) for n in p_cap)


# ---- 9. data-parallel -----------------------------------------------------------------------------
DP_KEYS = [0, 1, 0, 2, 1, 0, 3, 2]  # ranks [0, 1, 0, 2 | 1, 0, 3, 2]: positives cross the ranks


def _dp_worker(rank, world, port, q, chunk, backend):
    try:
        _dp_worker_body(rank, world, port, q, chunk, backend)
    except BaseException:  # report instead of leaving the parent waiting on the queue
        import traceback
        q.put((rank, None, traceback.format_exc()))
        raise


def _dp_worker_body(rank, world, port, q, chunk, backend):
    import sys
    if chunk is not None:
        os.environ["CLIPMI_CE_CHUNK"] = str(chunk)
    if world == 1:  # one-rank group: take the collective branches anyway (each is the identity)
        os.environ["CLIPMI_DP_FORCE_COLLECTIVES"] = "1"
    sys.path.insert(0, os.path.join(REPO, "vlm-clip_amd"))
    import torch.distributed as dist
    from clipmi import CLIPWithAdapters, synth
    from clipmi.trainer import FusedAdamW
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    group = dist.group.WORLD
    if backend == "clipmi":  # the exchanges, the key gather among them, as libclipmi's RCCL calls
        from clipmi.comm import Communicator
        group = Communicator.from_process_group(dist.group.WORLD)
    m = CLIPWithAdapters("tiny", use_shared_adapters=False, freeze_clip=False, device="cuda:0", precision="fp32",
                         pooling="eos", process_group=group)
    B = 4
    b = {k: torch.from_numpy(v).cuda() for k, v in synth.synthetic_batch(m.config, B, seed=5, start=rank * B).items()}
    opt = FusedAdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3, arenas=m.arenas())
    opt.zero_grad()
    out = m(**b, pair_keys=DP_KEYS[rank * B:(rank + 1) * B])
    opt.armed_backward(out["loss"])
    opt.grads_all_reduce(group)
    torch.cuda.synchronize()
    g = {n: p.grad.detach().cpu().numpy().copy() for n, p in m.named_parameters() if p.grad is not None}
    q.put((rank, out["loss"].item(), g))
    dist.barrier()
    dist.destroy_process_group()


def _single_device(n):
    from clipmi import CLIPWithAdapters, synth
    m = CLIPWithAdapters("tiny", use_shared_adapters=False, freeze_clip=False, device="cuda:0", precision="fp32",
                         pooling="eos")
    b = {k: torch.from_numpy(v).cuda() for k, v in synth.synthetic_batch(m.config, n, seed=5).items()}
    out = m(**b, pair_keys=DP_KEYS[:n])
    out["loss"].backward()
    torch.cuda.synchronize()
    plain = m(**b)["loss"].item()
    assert abs(plain - out["loss"].item()) > 1e-3  # the keys matter at this batch
    return out["loss"].item(), {n_: p.grad.detach().cpu().numpy() for n_, p in m.named_parameters() if p.grad is not None}


def _run_ranks(world, chunk, backend, port):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q, chunk, backend)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    for _ in procs:
        r = q.get(timeout=200)
        if r[1] is None:  # a rank failed: its partner may be stuck in a collective
            for p in procs:
                p.kill()
            raise AssertionError(f"rank {r[0]} failed:\n{r[2]}")
        res.append(r)
    for p in procs:
        p.join(120)
    return sorted(res, key=lambda x: x[0])


@pytest.mark.parametrize("chunk", [None, 3])
def test_two_rank_keyed_loss_matches_single_device(chunk):
    """Two ranks over gloo on one device, B = 4 each; chunk 3: Bg = 8 streamed in chunks of 3, 3, 2.  The
    tolerances are those of tests/test_gpu_dp.py."""
    res = _run_ranks(2, chunk, "gloo", 31100 + os.getpid() % 500 + 71 * int(chunk is not None))
    loss0, ref = _single_device(8)
    gmax = max(float(np.abs(r).max()) for r in ref.values())
    for rank, loss, g in res:
        assert abs(loss - loss0) < 1e-5, (rank, loss, loss0)
        worst = (0.0, "")
        for n, r in ref.items():
            # floor at 1 % of the largest gradient: some true gradients are ~0 (k biases)
            scale = max(float(np.abs(r).max()), 1e-2 * gmax)
            worst = max(worst, (float(np.abs(g[n] - r).max()) / scale, n))
        assert worst[0] < 1e-4, worst


def test_one_rank_communicator_key_gather_is_bitwise_single_device():
    """A one-rank clipmi.comm.Communicator with CLIPMI_DP_FORCE_COLLECTIVES=1: the keys go through libclipmi's
    all-gather as a bit-reinterpreted fp32 [B, 2] view, every collective is the identity, and the loss and the
    gradients are bitwise those of the group-free keyed run.  One gradient is left out of the bitwise comparison:
    the token embedding's (clipmi_text_embed_bwd) is not reproducible from run to run on one device with no group
    and no keys either -- three group-free runs of this model and batch differed in it by 9.5e-7 on 12 (one fp32
    spacing), all other 89 gradients were bitwise equal -- so it is held to 1e-4 of its scale, tests/test_gpu_dp.py's
    bound."""
    (_, loss, g), = _run_ranks(1, None, "clipmi", 31900 + os.getpid() % 500)
    loss0, ref = _single_device(4)
    assert loss == loss0
    assert set(g) == set(ref)
    loose = "clip.text_model.embeddings.token_embedding.weight"
    differ = [(n, float(np.abs(g[n] - r).max())) for n, r in ref.items() if n != loose and not np.array_equal(g[n], r)]
    assert not differ, differ
    assert float(np.abs(g[loose] - ref[loose]).max()) < 1e-4 * float(np.abs(ref[loose]).max())
