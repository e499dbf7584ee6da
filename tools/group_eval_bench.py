"""Time clipmi_group_count / clipmi_group_pick against clipmi_rank_count, and the shared block walk end to end.

  python tools/group_eval_bench.py [--n 32768] [--e 512] [--block B] [--groups 7,35] [--reps 20] [--runs 3] [--out FILE]

Paired unit-norm features, N = M, as tools/topk_bench.py draws them; pair i carries key i mod G (G = 7: the emotion
classes, G = 35: the captions of RAF-DB).  Per score block (block x block, default the library's 8192), device-event
time of one launch on a later block of the row range (first = 0), median and min over --reps: the block's exact-f32
GEMM, clipmi_rank_count, clipmi_group_pick and clipmi_group_count per G.  The goal is group_count <= 1.5 x
rank_count in this run.  End to end (median of --runs): the keyed evaluation of one direction -- diagonal ranks,
keyed ranks and the top-10 lists -- through the shared walk (two GEMM walks) against target_ranks + group_ranks +
topk called one after the other (five walks).  Prints a table and one JSON line, and writes both to --out."""
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


def timed(fn, reps):
    """(median, min) ms of fn() over reps, each between two events, after two warm-ups."""
    times = []
    for n in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if n >= 2:
            times.append(a.elapsed_time(b))
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--e", type=int, default=512)
    ap.add_argument("--block", type=int, default=None)
    ap.add_argument("--groups", default="7,35")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("group_eval_bench needs a GPU")
    groups = [int(x) for x in args.groups.split(",")]
    N, E = args.n, args.e
    blk = min(args.block or EV.eval_block(), N)
    if N < 2 * blk:
        raise SystemExit("group_eval_bench needs at least two column blocks (n >= 2 * block)")
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.nn.functional.normalize(torch.randn(N, E, device="cuda", generator=g), dim=1)
    c = torch.nn.functional.normalize(q + 0.3 * torch.randn(N, E, device="cuda", generator=g), dim=1)
    s = T.K.stream()
    res = {"n": N, "e": E, "block": blk, "reps": args.reps, "runs": args.runs,
           "device": torch.cuda.get_device_name(0), "block_bytes": blk * blk * 4}
    lines = [f"group_eval_bench: N = M = {N}, E = {E}, block {blk} x {blk} ({blk * blk * 4 / 2**20:.0f} MiB of fp32), "
             f"{res['device']}", f"per launch: median / min ms over {args.reps} repetitions; GB/s = block bytes / median",
             "", f"{'per block (a later block, first = 0)':<44s} {'median':>9s} {'min':>9s} {'GB/s':>9s}"]

    def row(name, med, lo, note=""):
        lines.append(f"{name:<44s} {med:9.4f} {lo:9.4f} {blk * blk * 4 / (med * 1e-3) / 1e9:9.0f}  {note}")

    S0 = torch.empty(blk * blk, dtype=torch.float32, device="cuda")
    S1 = torch.empty(blk * blk, dtype=torch.float32, device="cuda")
    T._gemm_f32(blk, blk, E, q, E, True, c, E, True, S0, blk)
    med, lo = timed(lambda: T._gemm_f32(blk, blk, E, q, E, True, c[blk:], E, True, S1, blk), args.reps)
    res["gemm_ms"] = [med, lo]
    row("gemm_f32 (exact fp32)", med, lo, f"{2 * blk * blk * E / (med * 1e-3) / 1e12:.1f} TFLOP/s")

    i32 = dict(dtype=torch.int32, device="cuda")
    f32 = dict(dtype=torch.float32, device="cuda")
    ts, bad = torch.empty(N, **f32), torch.zeros(1, **i32)
    gt, eq, t1, t1s = torch.empty(N, **i32), torch.empty(N, **i32), torch.empty(N, **i32), torch.empty(N, **f32)
    call("clipmi_rank_pick", s, P_(S0), blk, N, N, 0, blk, 0, blk, None, P_(ts), P_(bad))
    call("clipmi_rank_count", s, P_(S0), blk, N, N, 0, blk, 0, blk, None, P_(ts), 1, P_(gt), P_(eq), P_(t1), P_(t1s))
    med, lo = timed(lambda: call("clipmi_rank_count", s, P_(S1), blk, N, N, 0, blk, blk, blk, None, P_(ts), 0, P_(gt),
                                 P_(eq), P_(t1), P_(t1s)), args.reps)
    res["rank_count_ms"] = [med, lo]
    rank_ms = med
    row("rank_count", med, lo)

    res["group"] = {}
    ps, pi, npos = torch.empty(N, **f32), torch.empty(N, **i32), torch.empty(N, **i32)
    for G in groups:
        keys = (torch.arange(N, device="cuda") % G).to(torch.int64) * 2 ** 33 - 5
        call("clipmi_group_pick", s, P_(S0), blk, N, N, 0, blk, 0, blk, P_(keys), P_(keys), None, 1, P_(ps), P_(pi),
             P_(npos))
        pick = timed(lambda: call("clipmi_group_pick", s, P_(S1), blk, N, N, 0, blk, blk, blk, P_(keys), P_(keys), None,
                                  0, P_(ps), P_(pi), P_(npos)), args.reps)
        call("clipmi_group_count", s, P_(S0), blk, N, N, 0, blk, 0, blk, P_(keys), P_(keys), None, P_(ps), P_(npos), 1,
             P_(gt), P_(eq), P_(t1), P_(t1s))
        count = timed(lambda: call("clipmi_group_count", s, P_(S1), blk, N, N, 0, blk, blk, blk, P_(keys), P_(keys),
                                   None, P_(ps), P_(npos), 0, P_(gt), P_(eq), P_(t1), P_(t1s)), args.reps)
        res["group"][G] = {"pick_ms": list(pick), "count_ms": list(count), "pick_over_rank_count": pick[0] / rank_ms,
                           "count_over_rank_count": count[0] / rank_ms}
        row(f"group_pick  G={G}", *pick, f"{pick[0] / rank_ms:.2f} x rank_count")
        row(f"group_count G={G}", *count, f"{count[0] / rank_ms:.2f} x rank_count (goal <= 1.5)")
    del S0, S1

    lines += ["", f"{'end to end, one direction, N x M = ' + str(N) + ' x ' + str(N):<44s} {'median':>9s} {'min':>9s}"]

    def e2e(name, fn):
        ts_ = []
        for n in range(args.runs + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn()
            b.record()
            torch.cuda.synchronize()
            del out
            if n:
                ts_.append(a.elapsed_time(b))
        med, lo = statistics.median(ts_), min(ts_)
        lines.append(f"{name:<44s} {med:9.2f} {lo:9.2f}")
        return [med, lo]

    G = groups[-1]
    keys = (torch.arange(N, device="cuda") % G).to(torch.int64)
    res["target_ranks_ms"] = e2e("target_ranks (two walks)", lambda: EV.target_ranks(q, c, None, block=blk))
    res["group_ranks_ms"] = e2e(f"group_ranks G={G} (two walks)", lambda: EV.group_ranks(q, c, keys, keys, block=blk))
    res["topk_ms"] = e2e("topk k=10 (one walk)", lambda: EV.topk(q, c, 10, block=blk))
    res["separate_ms"] = e2e("the three calls, one after the other",
                             lambda: (EV.target_ranks(q, c, None, block=blk),
                                      EV.group_ranks(q, c, keys, keys, block=blk), EV.topk(q, c, 10, block=blk)))
    res["shared_ms"] = e2e("the shared walk (two walks)", lambda: EV._keyed_walk(q, c, keys, 10, blk))
    res["shared_over_separate"] = res["shared_ms"][0] / res["separate_ms"][0]
    lines.append(f"{'  shared / separate':<44s} {res['shared_over_separate']:9.2f}")
    text = "\n".join(lines) + "\n\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
