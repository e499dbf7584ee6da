"""Multi-positive contrastive loss, the parts that need no GPU: the keyed entry points' argument guards, the
string keys, the model's pair_keys validation, and the fp64 oracle the GPU tests compare against
(tests/test_gpu_multipositive.py imports it from here)."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "vlm-clip_amd")

EMOTIONS = ["surprise", "fear", "disgust", "happiness", "sadness", "anger", "neutral"]
TEMPLATES = ["a photo of a face showing {}", "a person expressing {}", "a facial expression of {}",
             "someone who feels {}", "a close-up portrait with a look of {}"]


def oracle_rows(L, keys_all, label0):
    """The definition on one [B, Bg] block of fp64 logits: ce_i = lse_i - mean_{j in P_i} L_ij with
    P_i = { j : key[j] == key[label0 + i] }.  Returns (lse, ce, winv)."""
    B = L.shape[0]
    mask = (keys_all[label0:label0 + B, None] == keys_all[None, :]).to(L.dtype)
    cnt = mask.sum(1)
    lse = torch.logsumexp(L, dim=1)
    return lse, lse - (L * mask).sum(1) / cnt, 1.0 / cnt


def oracle_loss(t, i, ls, keys):
    """The whole loss in the dtype of its inputs (fp64 in the tests): normalise, L = exp(ls) t^ i^T, both
    directions, / (2 Bg).  Returns (loss, t^, i^)."""
    tn = t / t.norm(dim=-1, keepdim=True)
    inn = i / i.norm(dim=-1, keepdim=True)
    L = tn @ inn.t() * ls.exp()
    ce_t = oracle_rows(L, keys, 0)[1]
    ce_i = oracle_rows(L.t(), keys, 0)[1]
    return (ce_t.sum() + ce_i.sum()) / (2 * t.shape[0]), tn, inn


@pytest.mark.parametrize("B,E", [(7, 64), (130, 64)])
def test_oracle_with_distinct_keys_is_the_reference_loss(B, E):
    """All keys distinct: the oracle is model_m.py:159-163, CE on arange targets in both directions."""
    g = torch.Generator().manual_seed(3)
    t = torch.randn(B, E, generator=g, dtype=torch.float64)
    i = torch.randn(B, E, generator=g, dtype=torch.float64)
    ls = torch.tensor(math.log(100.0), dtype=torch.float64)
    keys = torch.randperm(B, generator=g) * 7919 - 11
    loss, tn, inn = oracle_loss(t, i, ls, keys)
    L = tn @ inn.t() * ls.exp()
    lab = torch.arange(B)
    ref = (F.cross_entropy(L, lab) + F.cross_entropy(L.t(), lab)) / 2
    assert abs(loss.item() - ref.item()) < 1e-12 * max(1.0, abs(ref.item()))


def test_keyed_entry_points_reject_bad_arguments_without_gpu():
    """The guards run on the host before any launch and name the operand (pointers are never dereferenced)."""
    from clipmi import _lib
    from clipmi import towers  # noqa: F401  (declares the prototypes)
    L = _lib.lib()
    assert L.clipmi_version() >= 7  # 6: before clipmi_contrastive_keyed_* / clipmi_row_hash64
    S, K, O = 4096, 8192, 12288

    def err(st):
        assert st == -1
        with pytest.raises(ValueError):
            _lib.check(st, "keyed")
        return L.clipmi_last_error()

    # null keys
    assert b"keys_all" in err(L.clipmi_contrastive_keyed_fwd(None, S, S, S, None, 4, 8, 0, O, O, O))
    assert b"keys_all" in err(L.clipmi_contrastive_keyed_bwd(None, S, S, S, S, None, None, 4, 8, 0, 0.5, O, O))
    assert b"keys_all" in err(L.clipmi_contrastive_keyed_fwd_chunk(None, S, S, None, 4, 4, 0, 8, 0, O))
    assert b"keys_all" in err(L.clipmi_contrastive_keyed_bwd_chunk(None, S, S, S, S, None, None, 4, 4, 0, 8, 0, 0.5,
                                                                   O, O, 0))
    # label0 + B > Bg, negative label0
    for lab0 in (5, -1):
        assert b"label offset" in err(L.clipmi_contrastive_keyed_fwd(None, S, S, S, K, 4, 8, lab0, O, O, O))
        assert b"label offset" in err(L.clipmi_contrastive_keyed_bwd(None, S, S, S, S, None, K, 4, 8, lab0, 0.5, O, O))
        assert b"label offset" in err(L.clipmi_contrastive_keyed_fwd_chunk(None, S, S, K, 4, 4, 0, 8, lab0, O))
        assert b"label offset" in err(L.clipmi_contrastive_keyed_bwd_chunk(None, S, S, S, S, None, K, 4, 4, 0, 8, lab0,
                                                                           0.5, O, O, 0))
    # chunk out of range: past Bg, negative start, empty
    for C, col0 in ((4, 5), (4, -1), (0, 0), (9, 0)):
        assert b"chunk" in err(L.clipmi_contrastive_keyed_fwd_chunk(None, S, S, K, 4, C, col0, 8, 0, O))
        assert b"chunk" in err(L.clipmi_contrastive_keyed_bwd_chunk(None, S, S, S, S, None, K, 4, C, col0, 8, 0, 0.5,
                                                                    O, O, 0))
    # B == 0 returns before any launch, whatever the pointers
    assert L.clipmi_contrastive_keyed_fwd(None, S, S, S, K, 0, 8, 0, O, O, O) == 0
    assert L.clipmi_contrastive_keyed_bwd(None, S, S, S, S, None, K, 0, 8, 0, 0.5, O, O) == 0
    assert L.clipmi_contrastive_keyed_fwd_chunk(None, S, S, K, 0, 4, 0, 8, 0, O) == 0
    assert L.clipmi_contrastive_keyed_finish(None, S, 0, O, O, O) == 0
    assert L.clipmi_contrastive_keyed_bwd_chunk(None, S, S, S, S, None, K, 0, 4, 0, 8, 0, 0.5, O, O, 0) == 0
    assert L.clipmi_row_hash64(None, S, 0, 77, O) == 0
    assert b"null" in err(L.clipmi_row_hash64(None, None, 3, 77, O))


def _captions():
    return [t.format(e) for e in EMOTIONS for t in TEMPLATES]


def test_keys_from_strings_equal_and_distinct():
    from clipmi.losses import keys_from_strings
    caps = _captions()
    k = keys_from_strings(caps + caps[:3])
    assert k.dtype == torch.int64 and k.shape == (38,)
    assert torch.equal(k[35:], k[:3])                 # equal strings, equal keys
    assert len(set(k[:35].tolist())) == 35            # the 35 RAF-DB-style captions stay apart
    assert len(set(keys_from_strings(EMOTIONS).tolist())) == 7
    with pytest.raises(ValueError):
        keys_from_strings(["happiness", 3])


def test_keys_from_strings_stable_across_processes():
    """Two fresh interpreters with different hash salts give the same keys (Python's hash() would not)."""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); from clipmi.losses import keys_from_strings; "
            "print(keys_from_strings(['happiness', 'a photo of a face showing fear', '']).tolist())")
    outs = []
    for salt in ("1", "2"):
        env = dict(os.environ, PYTHONHASHSEED=salt)
        r = subprocess.run([sys.executable, "-c", code, PKG], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.strip())
    assert outs[0] == outs[1]
    from clipmi.losses import keys_from_strings
    assert outs[0] == str(keys_from_strings(["happiness", "a photo of a face showing fear", ""]).tolist())


def test_fnv1a64_reference_values():
    """The Python restatement of clipmi_row_hash64: the empty row is the offset basis; one token 0x61 taken as a
    whole uint64 is the published FNV-1a of the byte 'a' (xor with a value below 256 touches the low byte only)."""
    from clipmi.losses import fnv1a64
    assert fnv1a64([]) == 0xcbf29ce484222325 - (1 << 64)
    assert fnv1a64([0x61]) & 0xFFFFFFFFFFFFFFFF == 0xaf63dc4c8601ec8c
    assert fnv1a64([1, 2]) != fnv1a64([2, 1])
    assert fnv1a64([-1]) == fnv1a64([0xFFFFFFFFFFFFFFFF])


def test_bad_pair_keys_raise_before_any_kernel():
    """Wrong length, float dtype, non-integers: ValueError from forward() itself -- on a CPU model, where any
    kernel call would fail differently."""
    from clipmi import CLIPWithAdapters, synth
    from clipmi.losses import as_pair_keys
    m = CLIPWithAdapters("tiny", use_shared_adapters=False, device="cpu")
    b = {k: torch.from_numpy(v) for k, v in synth.synthetic_batch(m.config, 4, seed=1).items()}
    for bad in (torch.arange(5), torch.arange(3), torch.zeros(4), torch.zeros(4, dtype=torch.float64),
                torch.zeros(4, 1, dtype=torch.int64), [0, 1, 2], [0.0, 1.0, 2.0, 3.0], ["a", "b", "c", "d"],
                torch.zeros(4, dtype=torch.bool)):
        with pytest.raises(ValueError, match="pair_keys"):
            m(**b, pair_keys=bad)
    k = as_pair_keys([3, -1, 2 ** 40, 3], 4, "cpu")
    assert k.dtype == torch.int64 and k.tolist() == [3, -1, 2 ** 40, 3]
    assert as_pair_keys(torch.tensor([1, 2], dtype=torch.int32), 2, "cpu").dtype == torch.int64


def test_batch_keys_switch():
    from clipmi.losses import batch_keys, keys_from_strings
    batch = {"input_ids": torch.zeros(3, 5, dtype=torch.int64), "emotion": ["fear", "anger", "fear"],
             "label": torch.tensor([4, 1, 4])}
    assert batch_keys(batch, None) is None
    assert torch.equal(batch_keys(batch, "emotion"), keys_from_strings(["fear", "anger", "fear"]))
    assert batch_keys(batch, "label") is batch["label"]
    assert batch_keys(batch, lambda b: [7, 8, 7]) == [7, 8, 7]
    with pytest.raises(KeyError, match="caption_text"):
        batch_keys(batch, "caption_text")
