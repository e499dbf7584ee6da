"""Pairwise sigmoid contrastive loss, the parts that need no GPU: the fp64 oracle the GPU tests compare against
(tests/test_gpu_sigmoid.py imports it from here), the two entry points' argument guards, the model's loss= switch
and the checkpoint key rules."""
import math

import pytest
import torch
import torch.nn.functional as F

LN100 = math.log(100.0)


def pair_signs(keys_all, label0, B):
    """z [B, Bg]: +1 where the column's key equals the row's (row i is global index label0 + i), else -1."""
    return (keys_all[label0:label0 + B, None] == keys_all[None, :]).to(torch.float64) * 2 - 1


def oracle_sigmoid_loss(t, i, ls, b, keys):
    """The definition in the dtype of its inputs (fp64 in the tests): normalise, l = exp(ls) t^ i^T + b, z from key
    equality (keys None: the diagonal), loss = sum softplus(-z l) / B.  softplus(-x) is taken as -logsigmoid(x),
    which torch evaluates as max(-x, 0) + log1p(exp(-|x|)) with no threshold.  Returns (loss, t^, i^)."""
    B = t.shape[0]
    tn = t / t.norm(dim=-1, keepdim=True)
    inn = i / i.norm(dim=-1, keepdim=True)
    L = tn @ inn.t() * ls.exp() + b
    z = pair_signs(torch.arange(B) if keys is None else keys, 0, B).to(L.dtype)
    return -F.logsigmoid(z * L).sum() / B, tn, inn


def oracle_sigmoid_block(S, ls, b, keys_all, label0, norm):
    """One rank's [B, Bg] block from its cosines S (fp64): (rows [B, 3], logits, dS) as clipmi_sigmoid_pairs defines
    them: rows = (sum_j softplus(-z l), sum_j u sc s, sum_j u) with u = -z sigmoid(-z l) norm, dS = u sc."""
    B = S.shape[0]
    sc = ls.exp()
    L = S * sc + b
    z = pair_signs(keys_all, label0, B)
    u = -z * torch.sigmoid(-z * L) * norm
    rows = torch.stack([-F.logsigmoid(z * L).sum(1), (u * sc * S).sum(1), u.sum(1)], dim=1)
    return rows, L, u * sc


def test_oracle_single_pair_is_softplus_of_the_negated_logit():
    """Bg = 1: the one pair is a positive, loss = softplus(-(sc cos + b))."""
    g = torch.Generator().manual_seed(1)
    for ls, b in ((LN100, -10.0), (0.0, 0.0), (math.log(10.0), 3.0)):
        t = torch.randn(1, 16, generator=g, dtype=torch.float64)
        i = torch.randn(1, 16, generator=g, dtype=torch.float64)
        cos = F.cosine_similarity(t, i).item()
        loss = oracle_sigmoid_loss(t, i, torch.tensor(ls, dtype=torch.float64), torch.tensor(b, dtype=torch.float64),
                                   None)[0].item()
        x = -(math.exp(ls) * cos + b)
        ref = max(x, 0.0) + math.log1p(math.exp(-abs(x)))
        assert abs(loss - ref) < 1e-12 * max(1.0, abs(ref))


def test_oracle_keys_none_is_distinct_keys_and_autograd_matches_the_block_formulas():
    g = torch.Generator().manual_seed(2)
    B, E = 9, 16
    t = torch.randn(B, E, generator=g, dtype=torch.float64)
    i = torch.randn(B, E, generator=g, dtype=torch.float64)
    ls = torch.tensor(math.log(10.0), dtype=torch.float64, requires_grad=True)
    b = torch.tensor(-2.0, dtype=torch.float64, requires_grad=True)
    a = oracle_sigmoid_loss(t, i, ls, b, None)[0]
    d = oracle_sigmoid_loss(t, i, ls, b, torch.randperm(B, generator=g) * 7919 - 11)[0]
    assert a.item() == d.item()
    keys = torch.tensor([0, 1, 0, 2, 1, 0, 3, 2, 2])
    loss, tn, inn = oracle_sigmoid_loss(t, i, ls, b, keys)
    assert abs(loss.item() - a.item()) > 1e-3
    loss.backward()
    rows, L, dS = oracle_sigmoid_block((tn @ inn.t()).detach(), ls.detach(), b.detach(), keys, 0, 1.0 / B)
    assert abs(rows[:, 0].sum().item() / B - loss.item()) < 1e-12
    assert abs(rows[:, 1].sum().item() - ls.grad.item()) < 1e-12
    assert abs(rows[:, 2].sum().item() - b.grad.item()) < 1e-12


def test_sigmoid_entry_points_reject_bad_arguments_without_gpu():
    """The guards run on the host before any launch and name the operand (pointers are never dereferenced)."""
    from clipmi import _lib
    from clipmi import towers  # noqa: F401  (declares the prototypes)
    L = _lib.lib()
    assert L.clipmi_version() >= 11  # 10: before clipmi_sigmoid_pairs / clipmi_sigmoid_reduce
    S, K, O = 4096, 8192, 12288

    def err(st):
        assert st == -1
        with pytest.raises(ValueError):
            _lib.check(st, "sigmoid")
        return L.clipmi_last_error()

    # stream, S, logit_scale, logit_bias, keys_all, B, C, col0, Bg, label0, norm, logits, dS, rows
    assert b"logit_bias" in err(L.clipmi_sigmoid_pairs(None, S, S, None, K, 4, 8, 0, 8, 0, 0.125, O, O, O))
    assert b"rows" in err(L.clipmi_sigmoid_pairs(None, S, S, S, K, 4, 8, 0, 8, 0, 0.125, O, O, None))
    for lab0 in (5, -1):  # label0 + B > Bg, negative label0; with and without keys
        for keys in (K, None):
            assert b"label offset" in err(L.clipmi_sigmoid_pairs(None, S, S, S, keys, 4, 8, 0, 8, lab0, 0.125, O, O, O))
    for C, col0 in ((4, 5), (4, -1), (0, 0), (9, 0)):  # past Bg, negative start, empty, wider than Bg
        assert b"chunk" in err(L.clipmi_sigmoid_pairs(None, S, S, S, K, 4, C, col0, 8, 0, 0.125, None, O, O))
    # B == 0 returns before any launch, whatever the pointers
    assert L.clipmi_sigmoid_pairs(None, S, S, S, K, 0, 8, 0, 8, 0, 0.125, O, O, O) == 0
    assert L.clipmi_sigmoid_pairs(None, None, None, S, None, 0, 4, 4, 8, 8, 0.125, None, None, O) == 0
    # stream, rows, n, norm, gscale, loss, dls, db, beta
    assert b"rows" in err(L.clipmi_sigmoid_reduce(None, None, 4, 0.125, None, O, O, O, 0))
    assert b"negative" in err(L.clipmi_sigmoid_reduce(None, S, -1, 0.125, None, O, O, O, 0))
    assert b"all null" in err(L.clipmi_sigmoid_reduce(None, S, 4, 0.125, None, None, None, None, 1))
    assert L.clipmi_sigmoid_reduce(None, S, 0, 0.125, None, O, O, O, 0) == 0


def test_model_loss_switch_parameters_and_arenas():
    from clipmi import CLIPWithAdapters
    with pytest.raises(ValueError, match="loss"):
        CLIPWithAdapters("tiny", use_shared_adapters=False, device="cpu", loss="bogus")
    plain = CLIPWithAdapters("tiny", use_shared_adapters=False, device="cpu")
    soft = CLIPWithAdapters("tiny", use_shared_adapters=False, device="cpu", loss="softmax")
    sig = CLIPWithAdapters("tiny", use_shared_adapters=False, device="cpu", loss="sigmoid")
    names = [n for n, _ in plain.named_parameters()]
    assert not any("logit_bias" in n for n in names)
    assert [n for n, _ in soft.named_parameters()] == names and list(soft.state_dict()) == list(plain.state_dict())
    assert len(soft.arenas()) == len(plain.arenas()) == 3
    # the sigmoid model: the same parameters under the same names, plus the one bias in an arena of its own
    assert [n for n, _ in sig.named_parameters()] == names + ["sigmoid_head.logit_bias"]
    assert sig.clip.arena.offsets == plain.clip.arena.offsets and list(sig.clip.state_dict()) == list(plain.clip.state_dict())
    assert len(sig.arenas()) == 4 and sig.arenas()[-1] is sig.sigmoid_head.arena
    assert sig.sigmoid_head.logit_bias.shape == () and sig.sigmoid_head.logit_bias.item() == -10.0
    assert sig.sigmoid_head.logit_bias.requires_grad
    assert not sig.clip.logit_scale.requires_grad  # frozen with freeze_clip=True, as under the softmax loss
    assert CLIPWithAdapters("tiny", use_shared_adapters=False, device="cpu", loss="sigmoid",
                            logit_bias_init=-3.5).sigmoid_head.logit_bias.item() == -3.5
    full = CLIPWithAdapters("tiny", use_shared_adapters=False, device="cpu", loss="sigmoid", freeze_clip=False)
    assert full.clip.logit_scale.requires_grad


def test_trainer_adapter_mode_selects_the_bias_under_the_sigmoid_loss_only(tmp_path):
    from clipmi import CLIPAdapterTrainer, CLIPWithAdapters
    for loss, want in (("softmax", False), ("sigmoid", True)):
        m = CLIPWithAdapters("tiny", use_shared_adapters=False, device="cpu", loss=loss)
        tr = CLIPAdapterTrainer(m, [], output_dir=str(tmp_path))
        picked = {id(p) for p in tr.trainable_params}
        names = {n for n, p in m.named_parameters() if id(p) in picked}
        assert ("sigmoid_head.logit_bias" in names) == want
        assert all("adapter" in n for n in names - {"sigmoid_head.logit_bias"})
        assert "clip.logit_scale" not in names


def test_checkpoint_carries_the_sigmoid_head_when_and_only_when_the_loss_is_sigmoid(tmp_path):
    from clipmi import CLIPWithAdapters
    soft = CLIPWithAdapters("tiny", use_shared_adapters=False, device="cpu")
    sig = CLIPWithAdapters("tiny", use_shared_adapters=False, device="cpu", loss="sigmoid", logit_bias_init=-7.25)
    p_soft, p_sig = str(tmp_path / "soft.pt"), str(tmp_path / "sig.pt")
    soft.save_adapter_weights(p_soft)
    sig.save_adapter_weights(p_sig)
    assert set(torch.load(p_soft, weights_only=True)) == {"text_adapter", "vision_adapter"}
    sd = torch.load(p_sig, weights_only=True)
    assert set(sd) == {"text_adapter", "vision_adapter", "sigmoid_head"}
    assert set(sd["sigmoid_head"]) == {"logit_bias"} and sd["sigmoid_head"]["logit_bias"].item() == -7.25
    sig2 = CLIPWithAdapters("tiny", use_shared_adapters=False, device="cpu", loss="sigmoid", init_seed=5)
    assert sig2.sigmoid_head.logit_bias.item() == -10.0
    sig2.load_adapter_weights(p_sig)
    assert sig2.sigmoid_head.logit_bias.item() == -7.25
    assert torch.equal(sig2.text_adapter.down_project.weight, sig.text_adapter.down_project.weight)
    with pytest.raises(ValueError, match="Sigmoid head weights found"):
        soft.load_adapter_weights(p_sig)
    with pytest.raises(ValueError, match="no sigmoid head weights found"):
        sig2.load_adapter_weights(p_soft)
    # a model without adapters saves nothing, as before: the head alone is no adapter checkpoint
    bare = CLIPWithAdapters("tiny", use_text_adapter=False, use_vision_adapter=False, use_shared_adapters=False,
                            device="cpu", loss="sigmoid")
    with pytest.raises(ValueError, match="No adapters enabled"):
        bare.save_adapter_weights(p_sig)
