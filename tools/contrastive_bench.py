"""Time the contrastive head, diagonal (ContrastiveFn) against multi-positive (KeyedContrastiveFn).

  python tools/contrastive_bench.py [--reps 20] [--rounds 5] [--groups 35] [--out FILE]

Two shapes, forward plus backward, device events around each repetition:
  * materialised: ContrastiveFn / KeyedContrastiveFn.apply + backward at (B, E) = (1024, 512) on one device;
  * streamed: one rank's share of BASELINE config 5, B = 4096 local rows against Bg = 32768 gathered columns at
    E = 768 in 8192-column chunks -- both directions of towers._ce_streamed_fwd and _ce_streamed_bwd (ContrastiveFn's
    body between the all-gather and the reduce-scatter; rank 3 of 8, label offset 12288), so the four GEMMs per chunk
    are inside the time.
And the row kernels alone on one block of each shape ([1024, 1024] materialised, a [4096, 8192] chunk), with the
bytes each moves: the keyed kernels read 8 more bytes per logit (the column key).

The two variants alternate inside every round (unkeyed reps, keyed reps, ...), after warm-up of both; a round's figure
is the median of its repetitions, and the table gives the median, min and max over the rounds: the spread between
rounds of the same code is what a difference between the variants has to exceed.  Keys: --groups values drawn
uniformly (35: RAF-DB's caption count).  Prints a table and one JSON line, and writes both to --out."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vlm-clip_amd"))
from clipmi import towers as T  # noqa: E402

P_, call = T.P_, T.call


class _Arena:  # the logit_scale gradient's destination
    def __init__(self):
        self.grad = torch.zeros(64, device="cuda")

    def prepare_grads(self):
        pass

    def ptr(self, name, buf):
        return buf.data_ptr()


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternate(variants, reps, rounds, warm=3):
    """{name: [per-round median ms]} with the variants alternating inside every round."""
    for _ in range(warm):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            out[k].append(statistics.median(event_ms(fn) for _ in range(reps)))
    return out


def summary(rounds_ms):
    return {"median": statistics.median(rounds_ms), "min": min(rounds_ms), "max": max(rounds_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--groups", type=int, default=35)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contrastive_bench needs a GPU")
    os.environ.pop("CLIPMI_CE_CHUNK", None)
    g = torch.Generator(device="cuda").manual_seed(0)
    s = T.K.stream()
    ls = torch.tensor(math.log(100.0), device="cuda", requires_grad=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "groups": args.groups}
    lines = [f"contrastive_bench: {res['device']}; per-round median of {args.reps} repetitions, then median / min / max "
             f"over {args.rounds} alternating rounds (ms); keys: {args.groups} groups", ""]
    head = f"{'':<58s} {'median':>9s} {'min':>9s} {'max':>9s}"

    def report(title, variants, reps, note=None):
        r = {k: summary(v) for k, v in alternate(variants, reps, args.rounds).items()}
        lines.append(f"{title:<58s}" + head[58:])
        for k, v in r.items():
            extra = f"  {note[k]}" if note else ""
            lines.append(f"  {k:<56s} {v['median']:9.4f} {v['min']:9.4f} {v['max']:9.4f}{extra}")
        u, kd = r["unkeyed"], r["keyed"]
        spread = max(u["max"] - u["min"], kd["max"] - kd["min"])
        r["keyed_over_unkeyed"] = kd["median"] / u["median"]
        r["spread_ms"] = spread
        lines.append(f"  keyed / unkeyed {r['keyed_over_unkeyed']:.3f}; difference {kd['median'] - u['median']:+.4f} ms; "
                     f"run-to-run spread {spread:.4f} ms")
        lines.append("")
        return r

    # ---- materialised, through the autograd Functions
    B, E = 1024, 512
    t = torch.randn(B, E, device="cuda", generator=g).requires_grad_(True)
    i = torch.randn(B, E, device="cuda", generator=g).requires_grad_(True)
    keys = torch.randint(0, args.groups, (B,), device="cuda", generator=g)
    ar = _Arena()

    def fn_unkeyed():
        T.ContrastiveFn.apply(t, i, ls, None, True, ar)[0].backward()

    def fn_keyed():
        T.KeyedContrastiveFn.apply(t, i, ls, keys, None, True, ar)[0].backward()

    res["materialised_1024x512"] = report(f"ContrastiveFn forward + backward, (B, E) = ({B}, {E})",
                                          {"unkeyed": fn_unkeyed, "keyed": fn_keyed}, args.reps)

    # ---- the row kernels alone on a [1024, 1024] block
    S = torch.rand(B, B, device="cuda", generator=g) * 2 - 1
    L, dS = torch.empty_like(S), torch.empty_like(S)
    lse, ce, winv, dls = (torch.empty(B, device="cuda") for _ in range(4))
    lsd = ls.detach().reshape(1)
    norm = 1.0 / (2 * B)
    call("clipmi_contrastive_keyed_fwd", s, P_(S), P_(L), P_(lsd), P_(keys), B, B, 0, P_(lse), P_(ce), P_(winv))

    def gbs(nbytes):
        return lambda ms: f"{nbytes / (ms * 1e-3) / 1e9:7.0f} GB/s"

    n = B * B
    for title, un, kd, nb in (
            ("ce_fwd kernels, [1024, 1024] block",
             lambda: call("clipmi_contrastive_ce_fwd", s, P_(S), P_(L), P_(lsd), B, B, 0, P_(lse), P_(ce)),
             lambda: call("clipmi_contrastive_keyed_fwd", s, P_(S), P_(L), P_(lsd), P_(keys), B, B, 0, P_(lse), P_(ce),
                          P_(winv)), (12 * n, 20 * n)),  # read S, write L, read L (+ read keys)
            ("ce_bwd kernels, [1024, 1024] block",
             lambda: call("clipmi_contrastive_ce_bwd", s, P_(L), P_(lse), P_(lsd), None, B, B, 0, norm, P_(dS), P_(dls)),
             lambda: call("clipmi_contrastive_keyed_bwd", s, P_(L), P_(lse), P_(winv), P_(lsd), None, P_(keys), B, B, 0,
                          norm, P_(dS), P_(dls)), (8 * n, 16 * n))):
        r = report(title, {"unkeyed": un, "keyed": kd}, args.reps * 5)
        r["bytes"] = {"unkeyed": nb[0], "keyed": nb[1]}
        r["gbs"] = {k: nb[j] / (r[k]["median"] * 1e-3) / 1e9 for j, k in enumerate(("unkeyed", "keyed"))}
        lines[-1:-1] = [f"  bytes per launch (kernel-level, keys counted per logit): unkeyed {nb[0] / 2**20:.0f} MiB "
                        f"({r['gbs']['unkeyed']:.0f} GB/s), keyed {nb[1] / 2**20:.0f} MiB ({r['gbs']['keyed']:.0f} GB/s)"]
        res[title.split(",")[0].replace(" ", "_") + "_1024"] = r
    del S, L, dS

    # ---- streamed: B = 4096 rows of rank 3 against Bg = 32768 columns, 8192-column chunks
    B, Bg, E, C, lab0 = 4096, 32768, 768, 8192, 3 * 4096
    xg = torch.nn.functional.normalize(torch.randn(Bg, E, device="cuda", generator=g), dim=1)
    yg = torch.nn.functional.normalize(torch.randn(Bg, E, device="cuda", generator=g), dim=1)
    xl, yl = xg[lab0:lab0 + B].contiguous(), yg[lab0:lab0 + B].contiguous()
    kg = torch.randint(0, args.groups, (Bg,), device="cuda", generator=g)
    lse2, ce2, winv2, dls2 = (torch.empty(2, B, device="cuda") for _ in range(4))
    dXg, dYg = torch.empty(Bg, E, device="cuda"), torch.empty(Bg, E, device="cuda")
    dxl, dyl = torch.empty(B, E, device="cuda"), torch.empty(B, E, device="cuda")
    norm = 1.0 / (2 * Bg)

    def streamed(k, w):
        w0, w1 = (w[0], w[1]) if w is not None else (None, None)
        T._ce_streamed_fwd(s, xl, yg, lsd, lab0, C, lse2[0], ce2[0], k, w0)
        T._ce_streamed_fwd(s, yl, xg, lsd, lab0, C, lse2[1], ce2[1], k, w1)
        T._ce_streamed_bwd(s, xl, yg, lsd, None, lse2[0], lab0, norm, C, dls2[0], dYg, dxl, k, w0)
        T._ce_streamed_bwd(s, yl, xg, lsd, None, lse2[1], lab0, norm, C, dls2[1], dXg, dyl, k, w1)

    res["streamed_4096x32768x768"] = report(
        f"streamed forward + backward, {B} x {Bg}, E = {E}, chunks of {C}",
        {"unkeyed": lambda: streamed(None, None), "keyed": lambda: streamed(kg, winv2)}, max(3, args.reps // 4))

    # ---- the chunk kernels alone on one [4096, 8192] chunk
    Sc = torch.rand(B, C, device="cuda", generator=g) * 2 - 1
    dSc = torch.empty_like(Sc)
    run2, run4, lab = torch.empty(B, 2, device="cuda"), torch.empty(B, 4, device="cuda"), torch.empty(B, device="cuda")
    n = B * C
    for title, un, kd, nb in (
            ("ce_fwd_chunk kernels, [4096, 8192] chunk",
             lambda: call("clipmi_contrastive_ce_fwd_chunk", s, P_(Sc), P_(lsd), B, C, C, Bg, lab0, P_(run2), P_(lab)),
             lambda: call("clipmi_contrastive_keyed_fwd_chunk", s, P_(Sc), P_(lsd), P_(kg), B, C, C, Bg, lab0, P_(run4)),
             (8 * n, 16 * n)),  # S read twice (+ keys)
            ("ce_bwd_chunk kernels, [4096, 8192] chunk",
             lambda: call("clipmi_contrastive_ce_bwd_chunk", s, P_(Sc), P_(lse2[0]), P_(lsd), None, B, C, C, Bg, lab0, norm,
                          P_(dSc), P_(dls2[0]), 0),
             lambda: call("clipmi_contrastive_keyed_bwd_chunk", s, P_(Sc), P_(lse2[0]), P_(winv2[0]), P_(lsd), None,
                          P_(kg), B, C, C, Bg, lab0, norm, P_(dSc), P_(dls2[0]), 0), (8 * n, 16 * n))):
        run2.fill_(1.0)
        run4.fill_(1.0)
        r = report(title, {"unkeyed": un, "keyed": kd}, args.reps * 2)
        r["bytes"] = {"unkeyed": nb[0], "keyed": nb[1]}
        r["gbs"] = {k: nb[j] / (r[k]["median"] * 1e-3) / 1e9 for j, k in enumerate(("unkeyed", "keyed"))}
        lines[-1:-1] = [f"  bytes per launch (kernel-level, keys counted per logit): unkeyed {nb[0] / 2**20:.0f} MiB "
                        f"({r['gbs']['unkeyed']:.0f} GB/s), keyed {nb[1] / 2**20:.0f} MiB ({r['gbs']['keyed']:.0f} GB/s)"]
        res[title.split(",")[0].replace(" ", "_") + "_4096x8192"] = r

    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
