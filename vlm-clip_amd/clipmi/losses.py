"""Pair keys of the multi-positive contrastive loss (towers.KeyedContrastiveFn, csrc/contrastive_keys.hip).

Pairs of the global batch that carry the same 64-bit key are each other's positives:
``model(..., pair_keys=keys)``, ``CLIPAdapterTrainer(..., positives=...)``.  The keys are plain int64; what they
are made from is the caller's choice:

  caption_keys(input_ids)   "same caption": a 64-bit FNV-1a hash of each row of token ids, on the device
                            (clipmi_row_hash64), no host round trip and no strings
  keys_from_strings(seq)    a list of class names or captions -> int64, the first 8 bytes of blake2b; the same in
                            every process (Python's hash() is salted per process and would disagree across ranks)
  as_pair_keys(x, B, dev)   what the model accepts as pair_keys, validated and moved to the device without a sync
"""
from __future__ import annotations

import hashlib

import torch

from . import kernels as K
from . import towers as T

FNV_OFFSET, FNV_PRIME = 0xcbf29ce484222325, 0x100000001b3


def caption_keys(input_ids: torch.Tensor) -> torch.Tensor:
    """int64 [B] keys of the token rows [B, N] (any integer dtype, on the GPU): h = (h ^ token) * FNV_PRIME mod 2^64
    over the row from FNV_OFFSET, each token taken as one uint64; equal rows give equal keys."""
    if input_ids.dim() != 2 or input_ids.dtype.is_floating_point or input_ids.dtype == torch.bool:
        raise ValueError("input_ids must be an integer tensor [B, N]")
    ids = input_ids.to(torch.int64).contiguous()
    B, N = ids.shape
    out = torch.empty(B, dtype=torch.int64, device=ids.device)
    T.call("clipmi_row_hash64", K.stream(), T.P_(ids), B, N, T.P_(out))
    return out


def fnv1a64(tokens) -> int:
    """The hash of caption_keys for one row, in Python integers (as a signed 64-bit value)."""
    h = FNV_OFFSET
    for v in tokens:
        h = ((h ^ (int(v) & 0xFFFFFFFFFFFFFFFF)) * FNV_PRIME) & 0xFFFFFFFFFFFFFFFF
    return h - (1 << 64) if h >= 1 << 63 else h


def keys_from_strings(seq) -> torch.Tensor:
    """int64 [len(seq)] (CPU) keys of strings: the first 8 bytes of blake2b(utf-8), little-endian, signed."""
    out = []
    for x in seq:
        if not isinstance(x, str):
            raise ValueError(f"keys_from_strings takes strings, got {type(x).__name__}")
        out.append(int.from_bytes(hashlib.blake2b(x.encode("utf-8")).digest()[:8], "little", signed=True))
    return torch.tensor(out, dtype=torch.int64)


def as_pair_keys(keys, B: int, device) -> torch.Tensor:
    """pair_keys as the model takes them -- an int32 / int64 tensor or a sequence of ints, of length B -- as a
    contiguous int64 tensor on the device.  Anything else is a ValueError, raised before any kernel runs."""
    if isinstance(keys, torch.Tensor):
        if keys.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"pair_keys must be an int32 or int64 tensor, got {keys.dtype}")
        k = keys
    else:
        vals = list(keys)
        if not all(isinstance(v, int) and not isinstance(v, bool) for v in vals):
            raise ValueError("pair_keys must be an int32 / int64 tensor or a sequence of ints")
        k = torch.tensor(vals, dtype=torch.int64)
    if k.dim() != 1 or k.shape[0] != B:
        raise ValueError(f"pair_keys must have length {B} (one key per pair), got shape {tuple(k.shape)}")
    return k.to(device=device, dtype=torch.int64, non_blocking=True).contiguous()


def batch_keys(batch, positives, device=None):
    """The trainer's ``positives`` switch applied to one batch: None -> None (the diagonal loss); "caption" -> keys
    of batch["input_ids"] hashed on the device; another string names a batch field holding an int tensor or a list
    of strings (e.g. "emotion", as the default collate delivers it); a callable is called with the batch."""
    if positives is None:
        return None
    if callable(positives):
        return positives(batch)
    if positives == "caption":
        ids = batch["input_ids"]
        if device is not None and ids.device != torch.device(device):
            ids = ids.to(device, non_blocking=True)
        return caption_keys(ids)
    if positives not in batch:
        raise KeyError(f"positives={positives!r}: the batch has no such field (fields: {sorted(batch)})")
    v = batch[positives]
    if isinstance(v, torch.Tensor):
        return v
    v = list(v)
    if v and all(isinstance(x, str) for x in v):
        return keys_from_strings(v)
    return v
