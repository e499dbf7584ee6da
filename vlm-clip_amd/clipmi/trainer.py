"""Drop-in ``CLIPAdapterTrainer`` (trainer.py:11-167) with a fused, arena-wide optimizer.

The step is the reference's: zero_grad -> loss.backward -> clip_grad_norm_(max_grad_norm)
-> AdamW.step -> linear warmup/decay scheduler step (trainer.py:91-99,
[HF] optimization.py:101-129).  Here the clip and the AdamW update are two libclipmi
launches over the flat fp32 arenas (no per-parameter Python loop, no host sync), and in
data-parallel runs the gradient arenas are all-reduced (RCCL) once per arena.
"""
from __future__ import annotations

import ctypes
import os

import torch
import torch.distributed as dist

from . import _lib
from . import comm as CM
from . import kernels as K
from . import towers as T
from .images import ImageBatch, TrainAugment
from .losses import batch_keys


def linear_schedule_with_warmup(step, warmup, total):
    """lr multiplier of get_linear_schedule_with_warmup ([HF] optimization.py:101-104)."""
    if step < warmup:
        return float(step) / float(max(1, warmup))
    return max(0.0, float(total - step) / float(max(1, total - warmup)))


class GradBucketReducer:
    """Data-parallel gradient sum, bucketed and overlapped with backward.

    The towers report each finished chunk of encoder layers (a contiguous slice of the clip
    arena's gradient) through ``ready``; its all-reduce is issued at once on a communication
    stream that waits only for that slice's kernels, so it runs under the lower layers'
    backward.  ``finish`` all-reduces whatever was not reported (projections, logit_scale,
    final LNs, adapters) and makes the caller's stream wait for every bucket.  Each element is
    reduced exactly once per step.  Collectives are issued from the autograd thread in node
    order, which is the same on every rank.

    ``group``: a torch.distributed group or a clipmi.comm.Communicator (the all-reduce then runs as
    clipmi_allreduce on the communication stream).  ``bucket_dtype=torch.bfloat16``: each bucket is
    reduced as bf16 (cast on the communication stream, summed, cast back into the fp32 arena): half the
    bytes per ring (ViT-B/16 full fine-tune: 299 MB instead of 598 MB per step) at ~2^-9 relative rounding
    of every rank's contribution."""

    def __init__(self, arenas, group=None, bucket_dtype=torch.float32):
        if bucket_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("bucket_dtype: torch.float32 or torch.bfloat16")
        self.arenas = list(arenas)
        self.group = group
        self.bucket_dtype = bucket_dtype
        self._ids = {id(a) for a in self.arenas}
        self._done = {id(a): [] for a in self.arenas}
        self._works = []
        self._comm = None

    def _comm_stream(self, dev):
        if self._comm is None or self._comm.device != dev:
            self._comm = torch.cuda.Stream(device=dev)
        return self._comm

    def _issue(self, t):
        lib = CM.is_lib(self.group)
        half = self.bucket_dtype == torch.bfloat16
        if t.is_cuda:
            comm = self._comm_stream(t.device)
            comm.wait_stream(torch.cuda.current_stream(t.device))
            with torch.cuda.stream(comm):
                b = t.to(torch.bfloat16) if half else t
                if lib:  # enqueued on the comm stream itself: ordered before the cast back and finish()'s wait
                    self.group.all_reduce_(b, stream=comm)
                    w = None
                else:
                    w = dist.all_reduce(b, group=self.group, async_op=True)
                if half:
                    if w is not None:
                        w.wait()  # the comm stream waits for the collective before the cast back
                        w = None
                    t.copy_(b)
                self._works.append(w if w is not None else _StreamDone(comm))
        else:
            if lib:
                raise ValueError("a clipmi Communicator reduces device tensors")
            b = t.to(torch.bfloat16) if half else t
            w = dist.all_reduce(b, group=self.group, async_op=not half)
            if half:
                t.copy_(b)
            else:
                self._works.append(w)

    def ready(self, arena, off, n):
        if id(arena) not in self._ids or n <= 0:
            return
        self._done[id(arena)].append((off, off + n))
        self._issue(arena.grad[off:off + n])

    def reset(self):
        """Drop this step's bucket bookkeeping (a backward outside train_step, or gradient
        accumulation, must not leave reported slices behind for the next finish())."""
        for w in self._works:
            w.wait()
        self._works = []
        for a in self.arenas:
            self._done[id(a)] = []

    def finish(self):
        for a in self.arenas:
            pos = 0
            for lo, hi in sorted(self._done[id(a)]):
                if lo < pos:
                    raise RuntimeError("GradBucketReducer: overlapping gradient buckets")
                if lo > pos:
                    self._issue(a.grad[pos:lo])
                pos = hi
            if pos < a.numel:
                self._issue(a.grad[pos:a.numel])
            self._done[id(a)] = []
        for w in self._works:
            w.wait()  # the caller's stream waits for the bucket's collective
        self._works = []


class _StreamDone:
    """A bucket enqueued on the communication stream: waiting means the caller's stream waits for that stream."""

    def __init__(self, stream):
        self.dev = stream.device
        self.ev = torch.cuda.Event()
        self.ev.record(stream)

    def wait(self):
        torch.cuda.current_stream(self.dev).wait_event(self.ev)


class FusedAdamW:
    """torch.optim.AdamW semantics (decoupled weight decay, bias-corrected) over arenas.

    An arena whose parameters are all trainable is updated by ONE launch; otherwise each
    trainable parameter's slice gets its own launch of the same kernel."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, arenas=(),
                 process_group=None, grad_bucket_dtype=torch.float32):
        params = list(params)
        if not params:
            raise ValueError("optimizer got an empty parameter list")
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.step_count = 0
        ids = {id(p) for p in params}
        self.segments = []  # (arena, offset, numel)
        covered = set()
        for a in arenas:
            mine = [(n, p) for n, p in a.params.items() if id(p) in ids]
            if not mine:
                continue
            if len(mine) == len(a.params):
                self.segments.append((a, 0, a.numel))
            else:
                for n, p in mine:
                    off, _, numel = a.offsets[n]
                    self.segments.append((a, off, numel))
            covered |= {id(p) for _, p in mine}
        if covered != ids:
            raise ValueError("FusedAdamW: every parameter must belong to a clipmi arena")
        dev = self.segments[0][0].device
        self.state = [(torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.float32, device=dev))
                      for _, _, n in self.segments]
        self.arenas = list({id(a): a for a, _, _ in self.segments}.values())
        self.norm = torch.zeros(2, dtype=torch.float32, device=dev)
        n = len(self.segments)
        self._gp = (ctypes.c_void_p * n)()
        self._gn = (ctypes.c_int64 * n)()
        self._norm_ws = torch.empty(int(_lib.lib().clipmi_grad_norm_multi_ws(n)), dtype=torch.uint8, device=dev)
        self.reducer = None
        if process_group is not None and (CM.world_rank(process_group)[0] > 1 or T.force_collectives()):
            self.reducer = GradBucketReducer(self.arenas, process_group, grad_bucket_dtype)

    def overlap_with(self, model):
        """Let ``armed_backward`` report the model's gradient buckets to this optimizer's reducer."""
        self._model = model
        return self

    def armed_backward(self, loss):
        """loss.backward() with the gradient-ready hook armed for this one backward only: buckets
        are all-reduced while the lower layers' backward runs, and a backward outside the trainer
        step (or a second, accumulating one) never issues collectives of its own."""
        model = getattr(self, "_model", None)
        if self.reducer is None or model is None:
            loss.backward()
            return
        model.set_grad_hook(self.reducer.ready)
        try:
            loss.backward()
        finally:
            model.set_grad_hook(None)

    def zero_grad(self, set_to_none=False):
        if self.reducer is not None:
            self.reducer.reset()
        for a in self.arenas:
            a.zero_grad()

    def grads_all_reduce(self, group=None):
        """Data-parallel gradient sum: the overlapped buckets (GradBucketReducer) when this
        optimizer was built with a process group, else one RCCL all-reduce per arena."""
        if self.reducer is not None and (group is None or group is self.reducer.group):
            self.reducer.finish()
            return
        for a in self.arenas:
            CM.all_reduce_(a.grad, group)

    def clip_grad_norm(self, max_norm):
        """norm over all trainable gradients -> self.norm = [total_norm, clip_coef] on device."""
        for i, (a, off, n) in enumerate(self.segments):
            self._gp[i] = a.grad.data_ptr() + off * 4
            self._gn[i] = n
        T.call("clipmi_grad_norm_multi", K.stream(), self._gp, self._gn, len(self.segments), float(max_norm),
               T.P_(self.norm), T.P_(self._norm_ws), self._norm_ws.numel())
        return self.norm[0]

    def step(self, lr=None, clip=True):
        self.step_count += 1
        lr = self.lr if lr is None else lr
        b1, b2 = self.betas
        s = K.stream()
        for (a, off, n), (m, v) in zip(self.segments, self.state):
            shadow = a.shadow.data_ptr() + off * 2 if a.shadow is not None else None
            T.call("clipmi_adamw", s, a.data.data_ptr() + off * 4, a.grad.data_ptr() + off * 4, T.P_(m), T.P_(v),
                   shadow, n, lr, b1, b2, self.eps, self.weight_decay, self.step_count,
                   T.P_(self.norm) if clip else None)
        for a in self.arenas:
            a.data._version  # noqa: B018 (our kernel wrote master + shadow together)
            a.mark_shadow_fresh()


def _to_device(batch, device, non_blocking):
    """The batch's tensors and ImageBatch on the device; other values as they are."""
    return {k: v.to(device, non_blocking=non_blocking) if isinstance(v, (torch.Tensor, ImageBatch)) else v
            for k, v in batch.items()}


class CLIPAdapterTrainer:
    """trainer.py:11-167.  ``trainable="adapter"`` selects parameters whose name contains
    "adapter" exactly like trainer.py:40-43; ``trainable="requires_grad"`` takes every
    parameter with requires_grad (full fine-tune).  Under the model's loss="sigmoid" the adapter
    mode also takes sigmoid_head.logit_bias, the loss's own parameter (it exists under that loss only).

    ``positives`` (no reference counterpart) chooses the positives of the contrastive loss in train_step and
    evaluate(): None, the reference's diagonal loss; "caption", pairs whose token rows are equal (hashed on the
    device); any other string, a batch field holding an int tensor or a list of strings, e.g. "emotion" as the
    default collate delivers RAFDBDataset's; or a callable batch -> keys (clipmi.losses.batch_keys).  Pairs of the
    global batch with equal keys are each other's positives (towers.KeyedContrastiveFn)."""

    def __init__(self, model, train_dataloader, val_dataloader=None, learning_rate=5e-5, weight_decay=0.01,
                 warmup_steps=0, max_grad_norm=1.0, output_dir="./clip_adapter_checkpoints", *,
                 trainable="adapter", process_group=None, augment=None, positives=None):
        self.model = model
        if positives is not None and not (isinstance(positives, str) or callable(positives)):
            raise ValueError("positives: None, 'caption', a batch field name or a callable batch -> keys")
        self.positives = positives
        # ImageBatch -> ImageBatch (clipmi.images.TrainAugment), applied by train_step only; no reference counterpart
        self.augment = augment
        self.train_dataloader = train_dataloader
        self.val_dataloader = val_dataloader
        self.learning_rate = learning_rate
        self.weight_decay = weight_decay
        self.warmup_steps = warmup_steps
        self.max_grad_norm = max_grad_norm
        self.output_dir = output_dir
        self.process_group = process_group
        os.makedirs(output_dir, exist_ok=True)
        self.trainable_params = []
        for name, param in model.named_parameters():
            if trainable == "adapter":
                if "adapter" in name or "shared_adapters" in name or name == "sigmoid_head.logit_bias":
                    self.trainable_params.append(param)
            elif param.requires_grad:
                self.trainable_params.append(param)
        pg = process_group
        if pg is None and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            pg = dist.group.WORLD
        self.optimizer = FusedAdamW(self.trainable_params, lr=learning_rate, weight_decay=weight_decay,
                                    arenas=model.arenas(), process_group=pg)
        self.optimizer.overlap_with(model)
        self.total_steps = None

    def _world(self):
        if self.process_group is None and not (dist.is_available() and dist.is_initialized()):
            return 1
        if self.process_group is None:
            return dist.get_world_size()
        return CM.world_rank(self.process_group)[0]

    def _loss_kwargs(self, batch, device):
        """pair_keys of the batch under the positives switch; nothing at all for the diagonal loss."""
        keys = batch_keys(batch, self.positives, device)
        return {} if keys is None else {"pair_keys": keys}

    def train_step(self, batch, step, total_steps):
        """One reference step (trainer.py:81-99); returns the loss tensor (no host sync)."""
        device = self.model.clip.arena.device
        batch = _to_device(batch, device, True)
        if self.augment is not None and isinstance(batch.get("pixel_values"), ImageBatch):
            if isinstance(self.augment, TrainAugment):  # its affine records turn about the model's input centre
                batch["pixel_values"] = self.augment(batch["pixel_values"],
                                                     image_size=self.model.config.vision_config.image_size)
            else:
                batch["pixel_values"] = self.augment(batch["pixel_values"])
        outputs = self.model(input_ids=batch.get("input_ids"), attention_mask=batch.get("attention_mask"),
                             pixel_values=batch.get("pixel_values"), return_loss=True,
                             **self._loss_kwargs(batch, device))
        loss = outputs["loss"]
        self.optimizer.zero_grad()
        self.optimizer.armed_backward(loss)
        if self._world() > 1:
            self.optimizer.grads_all_reduce(self.process_group)
        self.optimizer.clip_grad_norm(self.max_grad_norm)
        lr = self.learning_rate * linear_schedule_with_warmup(step, self.warmup_steps, total_steps)
        self.optimizer.step(lr=lr)
        return loss

    def train(self, num_epochs, save_every=1, eval_every=1):
        total_steps = len(self.train_dataloader) * num_epochs
        self.total_steps = total_steps
        best_val_loss = float("inf")
        step = 0
        for epoch in range(num_epochs):
            self.model.train()
            epoch_loss = 0.0
            for batch in self.train_dataloader:
                loss = self.train_step(batch, step, total_steps)
                step += 1
                epoch_loss += loss.item()
            avg_train_loss = epoch_loss / len(self.train_dataloader)
            print(f"Epoch {epoch + 1} - Average training loss: {avg_train_loss:.4f}")
            if self.val_dataloader is not None and (epoch + 1) % eval_every == 0:
                val_loss = self.evaluate()
                print(f"Epoch {epoch + 1} - Validation loss: {val_loss:.4f}")
                if val_loss < best_val_loss:
                    best_val_loss = val_loss
                    self.save_model(os.path.join(self.output_dir, "best_adapter"))
            if (epoch + 1) % save_every == 0:
                self.save_model(os.path.join(self.output_dir, f"adapter_epoch_{epoch + 1}"))
        self.save_model(os.path.join(self.output_dir, "final_adapter"))

    def evaluate(self):
        assert self.val_dataloader is not None, "val_dataloader must not be None to run eval"
        self.model.eval()
        device = self.model.clip.arena.device
        val_loss = 0.0
        with torch.no_grad():
            for batch in self.val_dataloader:
                batch = _to_device(batch, device, False)
                outputs = self.model(input_ids=batch.get("input_ids"), attention_mask=batch.get("attention_mask"),
                                     pixel_values=batch.get("pixel_values"), return_loss=True,
                                     **self._loss_kwargs(batch, device))
                val_loss += outputs["loss"].item()
        return val_loss / len(self.val_dataloader)

    def evaluate_retrieval(self, ks=(1, 5, 10), topk=0, keys=None):
        """Recall@K and median / mean rank (image->text and text->image) over the whole validation set, on the
        device (clipmi.evaluation.evaluate_retrieval); unlike evaluate()'s mean batch loss it does not depend
        on the batch size.  topk > 0 adds the top-k retrieved lists (``i2t_topk`` / ``t2i_topk``).  keys adds
        the group-aware metrics (``_gR@k``, ``_g_median_rank``, ``_P@k``, ``_mAP@k``), in which every pair that
        shares a pair's key is a correct retrieval: a model trained with ``positives=...`` is usually scored with
        ``keys=trainer.positives``.  The default scores the diagonal alone.  No reference counterpart."""
        assert self.val_dataloader is not None, "val_dataloader must not be None to run eval"
        from .evaluation import evaluate_retrieval
        return evaluate_retrieval(self.model, self.val_dataloader, ks=ks, topk=topk, keys=keys)

    def save_model(self, path):
        self.model.save_adapter_weights(f"{path}.pt")

    def load_model(self, path):
        self.model.load_adapter_weights(f"{path}.pt")
