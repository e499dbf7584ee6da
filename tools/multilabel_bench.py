"""Time the multi-label path: clipmi.evaluation.average_precision and one MultiLabelCLIPAdapter.train_step against
the same work composed from torch ops on the GPU, and the AP against the host path.

  python tools/multilabel_bench.py [--reps 10] [--rounds 5] [--out profiles/multilabel_bench.log]

average_precision at (N, C) = (8192, 26) and (32768, 26), scores with ties (a grid of 4096 values), about two
positives per row: (a) the library (clipmi_ap_count + the host sum, transfer included); (b) torch on the GPU: a
stable sort per class, cumulative sums, one threshold per distinct score, result left on the device; (c) the host
path: transfer, then sklearn's average_precision_score per class where sklearn is installed, else the same sort
route in numpy.  train_step at B = 1024, E = 512, C = 26, five descriptions per class, over a feature-table
backbone: the library's head against torch autograd + torch.optim.Adam of the same model.

Device events around each call (the host path: a host clock around transfer + compute, which ends synchronised);
every variant warmed up, then the variants alternate inside every round; per round the median of --reps, then
median / min / max over the rounds.  Launches per call are counted with torch.profiler in a run of their own.
Records, does not gate: the log is where the measured values live."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vlm-clip_amd"))
from clipmi import evaluation as EV  # noqa: E402
from clipmi import heads as HD  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(variants, reps, rounds, warm=2):
    """{name: [per-round median ms]}; variants = {name: (fn, timer, reps or None)}, alternating inside every round."""
    for _ in range(warm):
        for fn, _, _ in variants.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fn, timer, r) in variants.items():
            out[k].append(statistics.median(timer(fn) for _ in range(r or reps)))
    return out


def launches(fn):
    """GPU kernels and memsets one call enqueues (torch.profiler, after a warm-up); None if the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception as e:  # the count is a side note: never lose the timings to it
        print(f"launch count unavailable: {type(e).__name__}: {e}", file=sys.stderr)
        return None


def torch_ap(s, t):
    """AP per class on the device, sklearn's definition: stable sort, cumulative sums, distinct thresholds."""
    N, C = s.shape
    order = torch.argsort(s, dim=0, descending=True, stable=True)
    ss, tt = torch.gather(s, 0, order), torch.gather(t, 0, order).double()
    tp = tt.cumsum(0)
    last = torch.cat([ss[1:] != ss[:-1], torch.ones(1, C, dtype=torch.bool, device=s.device)], 0)
    ends = torch.where(last, tp, torch.zeros_like(tp))  # tp at the end of each run of equal scores
    prev = torch.cat([torch.zeros(1, C, dtype=tp.dtype, device=s.device), torch.cummax(ends, 0).values[:-1]], 0)
    rank = torch.arange(1, N + 1, device=s.device, dtype=torch.float64)[:, None]
    total = tp[-1]
    ap = torch.where(last, (tp - prev) * tp / rank, torch.zeros_like(tp)).sum(0) / total
    return torch.where(total > 0, ap, torch.full_like(ap, float("nan")))


def numpy_ap(s, t):
    N, C = s.shape
    ap = np.full(C, np.nan)
    for c in range(C):
        total = t[:, c].sum()
        if total:
            order = np.argsort(-s[:, c], kind="stable")
            ss, tt = s[order, c], t[order, c].astype(np.float64)
            last = np.r_[np.flatnonzero(ss[1:] != ss[:-1]), N - 1]
            tp = np.cumsum(tt)[last]
            ap[c] = float(np.sum(np.diff(np.r_[0.0, tp / total]) * tp / (last + 1.0)))
    return ap


class TableBackbone:
    """A frozen backbone that serves feature tables (the towers are not what this times)."""

    def __init__(self, n_desc, n_img, dim, g):
        self.projection_dim = dim
        self.desc = torch.randn(n_desc, dim, device="cuda", generator=g)
        self.img = torch.randn(n_img, dim, device="cuda", generator=g)
        self.logit_scale = torch.tensor(math.log(100.0), device="cuda")

    def get_text_features(self, input_ids, attention_mask=None):
        return self.desc[input_ids[:, 0]]

    def get_image_features(self, pixel_values):
        return self.img[pixel_values]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multilabel_bench needs a GPU")
    try:
        from sklearn.metrics import average_precision_score
        host_name = "host: transfer + sklearn average_precision_score per class"
    except ImportError:
        average_precision_score = None
        host_name = "host: transfer + numpy sort route per class (no sklearn here)"
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = [f"multilabel_bench: {torch.cuda.get_device_name(0)}; per-round median of {args.reps} repetitions (host "
             f"path: 3), then median / min / max over {args.rounds} alternating rounds (ms)", ""]
    head = f"{'median':>10s} {'min':>10s} {'max':>10s}  launches"

    def report(title, variants, counts):
        r = alternate(variants, args.reps, args.rounds)
        lines.append(f"{title:<72s}" + head)
        for k, v in r.items():
            n = counts.get(k)
            lines.append(f"  {k:<70s}{statistics.median(v):10.4f} {min(v):10.4f} {max(v):10.4f}  "
                         f"{n if n is not None else '-'}")
        lines.append("")

    C = 26
    for N in (8192, 32768):
        s = (torch.randint(0, 4096, (N, C), device="cuda", generator=g).float() / 4096.0)
        t = (torch.rand(N, C, device="cuda", generator=g) < 2.0 / C).to(torch.uint8)

        def lib():
            return EV.average_precision(s, t)[0]

        def composed():
            return torch_ap(s, t)

        def host():
            sh, th = s.cpu().numpy(), t.cpu().numpy()
            if average_precision_score is None:
                return numpy_ap(sh, th)
            return np.array([average_precision_score(th[:, c], sh[:, c]) for c in range(C)])

        a, b, c = lib(), composed().cpu().numpy(), host()
        lines.append(f"average_precision N = {N}, C = {C}: max |library - torch| = {np.nanmax(np.abs(a - b)):.2e}, "
                     f"max |library - host| = {np.nanmax(np.abs(a - c)):.2e}, mAP = {np.nanmean(a):.6f}")
        report(f"average_precision ({N}, {C})",
               {"clipmi average_precision (counts on the device, sum on the host)": (lib, event_ms, None),
                "torch on the GPU (sort, cumsum, distinct thresholds; stays on device)": (composed, event_ms, None),
                host_name: (host, host_ms, 3)},
               {"clipmi average_precision (counts on the device, sum on the host)": launches(lib),
                "torch on the GPU (sort, cumsum, distinct thresholds; stays on device)": launches(composed)})

    # ---- one training step of the head
    B, E, nd = 1024, 512, 5
    bb = TableBackbone(C * nd, B, E, g)
    descs = {f"c{i}": (torch.arange(i * nd, (i + 1) * nd, device="cuda").view(nd, 1), None) for i in range(C)}
    y = (torch.rand(B, C, device="cuda", generator=g) < 2.0 / C).float()
    pw = HD.pos_weight_from_counts(y.sum(0).cpu(), B).cuda()
    m = HD.MultiLabelCLIPAdapter(bb, descriptions=descs, pos_weight=pw, class_bias=True, seed=1)
    idx = torch.arange(B, device="cuda")
    y_host = y.cpu()  # the reference's loader yields CPU tensors; the head checks them on the host

    def sd(ad):
        return [v.cuda().requires_grad_(True) for v in ad.state_dict_().values()]

    wv, wt = sd(m.visual_adapter), sd(m.text_adapter)
    bias = m.class_bias.detach().clone().requires_grad_(True)
    opt = torch.optim.Adam(wv + wt + [bias], lr=3e-4)
    crit = torch.nn.BCEWithLogitsLoss(pos_weight=pw)
    protos = m.emotion_embedding_tensor
    F = torch.nn.functional

    def blend(x, w, alpha, norm_in):
        if norm_in:
            x = x / x.norm(dim=-1, keepdim=True)
        z = alpha * F.linear(torch.relu(F.linear(x, w[0], w[1])), w[2], w[3]) + (1 - alpha) * x
        return z / z.norm(dim=-1, keepdim=True)

    def lib_step():
        return m.train_step(idx, y_host, 3e-4, 100.0)[0]

    def torch_step():
        loss = crit(100.0 * blend(bb.get_image_features(idx), wv, 0.2, True) @ blend(protos, wt, 0.2, False).T + bias,
                    y_host.cuda())
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    l0, l1 = lib_step().item(), torch_step().item()
    lines.append(f"train_step B = {B}, E = {E}, C = {C}: first-step loss library {l0:.6f}, torch {l1:.6f}")
    report(f"MultiLabelCLIPAdapter.train_step ({B}, {E}, {C})",
           {"clipmi train_step (class_bce, class_ce_bwd, adapters, Adam)": (lib_step, event_ms, None),
            "torch on the GPU (autograd + torch.optim.Adam)": (torch_step, event_ms, None)},
           {"clipmi train_step (class_bce, class_ce_bwd, adapters, Adam)": launches(lib_step),
            "torch on the GPU (autograd + torch.optim.Adam)": launches(torch_step)})
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
