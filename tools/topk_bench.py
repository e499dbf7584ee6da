"""Time clipmi_topk_merge against the kernels around it, and clipmi.evaluation.topk end to end.

  python tools/topk_bench.py [--n 32768] [--e 512] [--block B] [--ks 1,10,100,256] [--reps 20] [--runs 5] [--out FILE]

Paired unit-norm features, N = M, as tools/eval_bench.py draws them.  Per score block (block x block, default the
library's 8192), device-event time of one launch, median and min over --reps:
  * the block's exact-f32 GEMM;
  * clipmi_rank_count on the block (reads the same bytes once);
  * clipmi_topk_merge on the row range's first block (first = 1) and on a later block (first = 0; the lists of the
    first block are restored before every repetition, outside the timed span);
  * clipmi_topk_merge on an all-ascending block, where every element passes the threshold (k = 10 and 256).
End to end (median of --runs): evaluation.topk per k, evaluation.target_ranks (two GEMM walks), and per-block
torch.topk + cat + torch.topk in Python.  Prints a table and one JSON line, and writes both to --out."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vlm-clip_amd"))
from clipmi import evaluation as EV  # noqa: E402
from clipmi import towers as T  # noqa: E402

P_, call = T.P_, T.call


def timed(fn, reps, before=None):
    """(median, min) ms of fn() over reps, each between two events; before() runs untimed ahead of each."""
    times = []
    for n in range(reps + 2):
        if before:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if n >= 2:  # two warm-ups
            times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def torch_topk(q, c, k, blk):
    """The ad-hoc form: per-block torch.topk, merged by cat + topk (torch.matmul scores)."""
    N, M = q.shape[0], c.shape[0]
    scores = torch.empty(N, k, device=q.device)
    indices = torch.empty(N, k, dtype=torch.int64, device=q.device)
    for r0 in range(0, N, blk):
        best_s = best_i = None
        for c0 in range(0, M, blk):
            s, i = torch.topk(q[r0:r0 + blk] @ c[c0:c0 + blk].T, min(k, M - c0), dim=1)
            i = i + c0
            if best_s is not None:
                s, i = torch.cat([best_s, s], 1), torch.cat([best_i, i], 1)
                s, pick = torch.topk(s, min(k, s.shape[1]), dim=1)
                i = torch.gather(i, 1, pick)
            best_s, best_i = s, i
        scores[r0:r0 + blk, :best_s.shape[1]] = best_s
        indices[r0:r0 + blk, :best_i.shape[1]] = best_i
    return scores, indices


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--e", type=int, default=512)
    ap.add_argument("--block", type=int, default=None)
    ap.add_argument("--ks", default="1,10,100,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench needs a GPU")
    ks = [int(x) for x in args.ks.split(",")]
    N, E = args.n, args.e
    blk = min(args.block or EV.eval_block(), N)
    if N < 2 * blk:
        raise SystemExit("topk_bench needs at least two column blocks (n >= 2 * block)")
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.nn.functional.normalize(torch.randn(N, E, device="cuda", generator=g), dim=1)
    c = torch.nn.functional.normalize(q + 0.3 * torch.randn(N, E, device="cuda", generator=g), dim=1)
    s = T.K.stream()
    res = {"n": N, "e": E, "block": blk, "reps": args.reps, "runs": args.runs,
           "device": torch.cuda.get_device_name(0), "block_bytes": blk * blk * 4}
    lines = [f"topk_bench: N = M = {N}, E = {E}, block {blk} x {blk} ({blk * blk * 4 / 2**20:.0f} MiB of fp32), "
             f"{res['device']}", f"per launch: median / min ms over {args.reps} repetitions; GB/s = block bytes / median", ""]

    def rate(ms):
        return blk * blk * 4 / (ms * 1e-3) / 1e9

    def row(name, med, lo, note=""):
        lines.append(f"{name:<44s} {med:9.4f} {lo:9.4f} {rate(med):9.0f}  {note}")

    lines.append(f"{'per block':<44s} {'median':>9s} {'min':>9s} {'GB/s':>9s}")
    S0 = torch.empty(blk * blk, dtype=torch.float32, device="cuda")
    S1 = torch.empty(blk * blk, dtype=torch.float32, device="cuda")

    def gemm(buf, c0):
        T._gemm_f32(blk, blk, E, q, E, True, c[c0:], E, True, buf, blk)

    gemm(S0, 0)
    med, lo = timed(lambda: gemm(S1, blk), args.reps)
    res["gemm_ms"] = [med, lo]
    row("gemm_f32 (exact fp32)", med, lo, f"{2 * blk * blk * E / (med * 1e-3) / 1e12:.1f} TFLOP/s")

    # rank_count on the later block (paired targets: none of rows [0, blk) lies in columns [blk, 2 blk))
    ts = torch.empty(N, dtype=torch.float32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    gt, eq, t1 = (torch.empty(N, dtype=torch.int32, device="cuda") for _ in range(3))
    t1s = torch.empty(N, dtype=torch.float32, device="cuda")
    call("clipmi_rank_pick", s, P_(S0), blk, N, N, 0, blk, 0, blk, None, P_(ts), P_(bad))
    med, lo = timed(lambda: call("clipmi_rank_count", s, P_(S1), blk, N, N, 0, blk, blk, blk, None, P_(ts), 1, P_(gt),
                                 P_(eq), P_(t1), P_(t1s)), args.reps)
    res["rank_count_ms"] = [med, lo]
    rank_ms = med
    row("rank_count", med, lo)

    res["merge"] = {}
    for k in ks:
        sc = torch.empty(N, k, dtype=torch.float32, device="cuda")
        ix = torch.empty(N, k, dtype=torch.int32, device="cuda")

        def merge(buf, c0, first):
            call("clipmi_topk_merge", s, P_(buf), blk, N, N, 0, blk, c0, blk, k, first, None, P_(sc), P_(ix))

        m0 = timed(lambda: merge(S0, 0, 1), args.reps)
        merge(S0, 0, 1)
        keep_s, keep_i = sc[:blk].clone(), ix[:blk].clone()

        def restore():
            sc[:blk].copy_(keep_s)
            ix[:blk].copy_(keep_i)

        m1 = timed(lambda: merge(S1, blk, 0), args.reps, before=restore)
        res["merge"][k] = {"first_ms": list(m0), "later_ms": list(m1), "later_over_rank_count": m1[0] / rank_ms}
        row(f"topk_merge k={k:<3d} first block", *m0)
        row(f"topk_merge k={k:<3d} later block", *m1, f"{m1[0] / rank_ms:.2f} x rank_count")

    # adversarial: every row ascending, so every element passes the threshold it meets
    S0.view(blk, blk).copy_(torch.arange(blk, device="cuda", dtype=torch.float32).expand(blk, blk))
    res["ascending"] = {}
    for k in (10, 256):
        sc = torch.empty(N, k, dtype=torch.float32, device="cuda")
        ix = torch.empty(N, k, dtype=torch.int32, device="cuda")
        m = timed(lambda: call("clipmi_topk_merge", s, P_(S0), blk, N, N, 0, blk, 0, blk, k, 1, None, P_(sc), P_(ix)),
                  max(3, args.reps // 4))
        assert ix[0].tolist() == list(range(blk - 1, blk - 1 - k, -1))
        res["ascending"][k] = list(m)
        row(f"topk_merge k={k:<3d} all-ascending block", *m, f"{m[0] / rank_ms:.1f} x rank_count")
    del S0, S1

    lines += ["", f"{'end to end, N x M = ' + str(N) + ' x ' + str(N):<44s} {'median':>9s} {'min':>9s}"]

    def e2e(name, fn):
        ts_ = []
        out = None
        for n in range(args.runs + 1):
            out = None
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            if n:
                ts_.append(a.elapsed_time(b))
        med, lo = statistics.median(ts_), min(ts_)
        lines.append(f"{name:<44s} {med:9.2f} {lo:9.2f}")
        return out, [med, lo]

    _, res["target_ranks_ms"] = e2e("target_ranks (two GEMM walks)", lambda: EV.target_ranks(q, c, None, block=blk))
    res["topk_ms"], res["torch_topk_ms"], res["same_lists"] = {}, {}, {}
    for k in ks:
        got, res["topk_ms"][k] = e2e(f"evaluation.topk k={k}", lambda: EV.topk(q, c, k, block=blk))
        want, res["torch_topk_ms"][k] = e2e(f"torch.topk per block + merge k={k}", lambda: torch_topk(q, c, k, blk))
        same = float((got.indices.long() == want[1]).all(1).float().mean().item())
        res["same_lists"][k] = same  # torch's GEMM sums in another order: near-ties may swap
        lines.append(f"{'  rows with identical lists':<44s} {100 * same:8.2f} %")
    text = "\n".join(lines) + "\n\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
