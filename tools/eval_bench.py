"""Time and peak memory of clipmi.evaluation.target_ranks against the materialised form.

  python tools/eval_bench.py [--n 32768] [--e 512] [--block B] [--runs 7] [--out FILE.json] [--skip-baseline]

Paired unit-norm features, N = M.  Baseline: S = q @ c.T with torch (the [N, N] fp32 matrix), target scores
from its diagonal, greater = (S > ts).sum(1).  New path: target_ranks at the given block (default: the
library's).  Event timing after a warm-up, median of --runs; peak memory = the rise of
torch.cuda.max_memory_allocated over the call.  Prints one JSON line (and writes it to --out).  The two
`greater` vectors are compared: torch's GEMM sums in another order than the exact-f32 kernel, so rows whose
target is within rounding of another score may differ by a few places; the fraction of equal rows and the
largest difference are reported, not asserted."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vlm-clip_amd"))
from clipmi import evaluation as EV  # noqa: E402


def measure(fn, runs):
    fn()  # warm-up: library load, allocator pools
    torch.cuda.synchronize()
    times, out = [], None
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    for _ in range(runs):
        out = None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    peak = torch.cuda.max_memory_allocated() - before
    return out, statistics.median(times), min(times), max(times), peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--e", type=int, default=512)
    ap.add_argument("--block", type=int, default=None)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-baseline", action="store_true")
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.nn.functional.normalize(torch.randn(args.n, args.e, device="cuda", generator=g), dim=1)
    # candidates correlated with their query, as trained features are (at E = 512: cosine ~0.15 to the pair against
    # ~0.044 rms to the rest, so the ranks spread over tens of places instead of all being 1)
    c = torch.nn.functional.normalize(q + 0.3 * torch.randn(args.n, args.e, device="cuda", generator=g), dim=1)
    res = {"n": args.n, "e": args.e, "block": args.block or EV.eval_block(), "runs": args.runs,
           "device": torch.cuda.get_device_name(0)}

    def new():
        return EV.target_ranks(q, c, None, block=args.block).greater

    got, med, lo, hi, peak = measure(new, args.runs)
    res["target_ranks"] = {"ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                           "peak_bytes": int(peak)}
    if not args.skip_baseline:
        def base():
            S = q @ c.T
            return (S > S.diagonal().unsqueeze(1)).sum(1, dtype=torch.int32)

        want, med, lo, hi, peak = measure(base, args.runs)
        res["materialised"] = {"ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                               "peak_bytes": int(peak)}
        d = (got.long() - want.long()).abs()
        res["greater_equal_rows"] = float((d == 0).float().mean().item())
        res["greater_max_diff"] = int(d.max().item())
        res["recall_at_1_new_vs_materialised"] = [float((got == 0).float().mean().item()),
                                                  float((want == 0).float().mean().item())]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
