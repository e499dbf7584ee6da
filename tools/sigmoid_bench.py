"""Time the pairwise sigmoid contrastive head (SigmoidContrastiveFn) against the softmax one, unkeyed (ContrastiveFn)
and keyed (KeyedContrastiveFn).

  python tools/sigmoid_bench.py [--reps 20] [--rounds 5] [--groups 35] [--out FILE]

Built on tools/contrastive_bench.py: the same two shapes, forward plus backward, device events around each repetition,
  * materialised: the autograd Functions + backward at (B, E) = (1024, 512) on one device;
  * streamed: one rank's share of BASELINE config 5, B = 4096 local rows (rank 3 of 8, label offset 12288) against
    Bg = 32768 gathered columns at E = 768 in 8192-column chunks.  Softmax: both directions of
    towers._ce_streamed_fwd and _ce_streamed_bwd, 4 GEMMs per chunk and direction, 32 in all.  Sigmoid:
    towers._sigmoid_chunks over the one block, 3 GEMMs per chunk, 12 in all, plus clipmi_sigmoid_reduce;
the same alternation (every variant inside every round, after warm-up of all) and the same statistics: a round's
figure is the median of its repetitions, the table gives the median, min and max over the rounds, and the spread
between rounds of the same code is what a difference between variants has to exceed.

And, to split the streamed time, the parts alone: the three GEMMs of one [4096, 8192] chunk, and the row kernels on
one block of each shape with the bytes they move (softmax: the forward and the backward kernel of one block, back to
back; sigmoid: its one kernel, with the gradient half and without).  Keys: --groups values drawn uniformly (35:
RAF-DB's caption count).  Prints a table and one JSON line, and writes both to --out."""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from contrastive_bench import T, _Arena, alternate, summary  # noqa: E402

P_, call = T.P_, T.call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--groups", type=int, default=35)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sigmoid_bench needs a GPU")
    os.environ.pop("CLIPMI_CE_CHUNK", None)
    g = torch.Generator(device="cuda").manual_seed(0)
    s = T.K.stream()
    ls = torch.tensor(math.log(100.0), device="cuda", requires_grad=True)
    lb = torch.tensor(-10.0, device="cuda", requires_grad=True)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "groups": args.groups}
    lines = [f"sigmoid_bench: {res['device']}; per-round median of {args.reps} repetitions, then median / min / max "
             f"over {args.rounds} alternating rounds (ms); keys: {args.groups} groups", ""]
    head = f"{'':<64s} {'median':>9s} {'min':>9s} {'max':>9s}"

    def report(title, variants, reps, base=None, nbytes=None):
        """base: the variant every other one is set against (ratio, difference, the larger spread of the two)."""
        r = {k: summary(v) for k, v in alternate(variants, reps, args.rounds).items()}
        lines.append(f"{title:<64s}" + head[64:])
        for k, v in r.items():
            extra = ""
            if nbytes:
                extra = f"  {nbytes[k] / 2**20:5.0f} MiB {nbytes[k] / (v['median'] * 1e-3) / 1e9:6.0f} GB/s"
            lines.append(f"  {k:<62s} {v['median']:9.4f} {v['min']:9.4f} {v['max']:9.4f}{extra}")
        if base:
            b = r[base]
            for k in variants:
                if k == base:
                    continue
                spread = max(b["max"] - b["min"], r[k]["max"] - r[k]["min"])
                r[f"{k}_over_{base}"] = r[k]["median"] / b["median"]
                lines.append(f"  {k} / {base} {r[k]['median'] / b['median']:.3f}; difference "
                             f"{r[k]['median'] - b['median']:+.4f} ms; run-to-run spread {spread:.4f} ms")
        if nbytes:
            r["bytes"] = dict(nbytes)
        lines.append("")
        return r

    # ---- materialised, through the autograd Functions
    B, E = 1024, 512
    t = torch.randn(B, E, device="cuda", generator=g).requires_grad_(True)
    i = torch.randn(B, E, device="cuda", generator=g).requires_grad_(True)
    keys = torch.randint(0, args.groups, (B,), device="cuda", generator=g)
    ar, br = _Arena(), _Arena()
    res["materialised_1024x512"] = report(
        f"forward + backward through the Functions, (B, E) = ({B}, {E})",
        {"softmax": lambda: T.ContrastiveFn.apply(t, i, ls, None, True, ar)[0].backward(),
         "softmax_keyed": lambda: T.KeyedContrastiveFn.apply(t, i, ls, keys, None, True, ar)[0].backward(),
         "sigmoid": lambda: T.sigmoid_contrastive(t, i, ls, lb, None, None, True, ar, br)[0].backward(),
         "sigmoid_keyed": lambda: T.sigmoid_contrastive(t, i, ls, lb, keys, None, True, ar, br)[0].backward()},
        args.reps, base="softmax")

    lsd, lbd = ls.detach().reshape(1), lb.detach().reshape(1)

    def row_kernels(title, B, C, col0, Bg, lab0, kall, softmax, softmax_keyed, reps, nb_softmax):
        """The row kernels of one [B, C] block.  Bytes at kernel level, the 8-byte column key counted per logit."""
        S = torch.rand(B, C, device="cuda", generator=g) * 2 - 1
        dS = torch.empty_like(S)
        rows = torch.zeros(B, 3, device="cuda")  # a later chunk (col0 > 0) adds to them
        norm = 1.0 / Bg
        n = B * C

        def pairs(k, d):
            return lambda: call("clipmi_sigmoid_pairs", s, P_(S), P_(lsd), P_(lbd), P_(k), B, C, col0, Bg, lab0, norm,
                                None, P_(d), P_(rows))

        return report(title, {"softmax fwd + bwd kernels": softmax(S, dS),
                              "softmax_keyed fwd + bwd kernels": softmax_keyed(S, dS),
                              "sigmoid_pairs": pairs(None, dS), "sigmoid_pairs keyed": pairs(kall, dS),
                              "sigmoid_pairs keyed, loss half only": pairs(kall, None)}, reps,
                      base="softmax fwd + bwd kernels",
                      nbytes={"softmax fwd + bwd kernels": nb_softmax * n, "softmax_keyed fwd + bwd kernels":
                              (nb_softmax + 16) * n, "sigmoid_pairs": 8 * n, "sigmoid_pairs keyed": 16 * n,
                              "sigmoid_pairs keyed, loss half only": 12 * n})

    # ---- the row kernels alone on a [1024, 1024] block
    lse, ce, winv, dls = (torch.empty(B, device="cuda") for _ in range(4))
    L = torch.empty(B, B, device="cuda")
    nrm2 = 1.0 / (2 * B)

    def soft_mat(S, dS):  # read S, write L, read L; read L, write dS
        def run():
            call("clipmi_contrastive_ce_fwd", s, P_(S), P_(L), P_(lsd), B, B, 0, P_(lse), P_(ce))
            call("clipmi_contrastive_ce_bwd", s, P_(L), P_(lse), P_(lsd), None, B, B, 0, nrm2, P_(dS), P_(dls))
        return run

    def soft_mat_keyed(S, dS):
        def run():
            call("clipmi_contrastive_keyed_fwd", s, P_(S), P_(L), P_(lsd), P_(keys), B, B, 0, P_(lse), P_(ce), P_(winv))
            call("clipmi_contrastive_keyed_bwd", s, P_(L), P_(lse), P_(winv), P_(lsd), None, P_(keys), B, B, 0, nrm2,
                 P_(dS), P_(dls))
        return run

    res["row_kernels_1024"] = row_kernels("row kernels of one [1024, 1024] block", B, B, 0, B, 0, keys, soft_mat,
                                          soft_mat_keyed, args.reps * 5, 20)
    del L

    # ---- streamed: B = 4096 rows of rank 3 against Bg = 32768 columns, 8192-column chunks
    B, Bg, E, C, lab0 = 4096, 32768, 768, 8192, 3 * 4096
    xg = torch.nn.functional.normalize(torch.randn(Bg, E, device="cuda", generator=g), dim=1)
    yg = torch.nn.functional.normalize(torch.randn(Bg, E, device="cuda", generator=g), dim=1)
    xl, yl = xg[lab0:lab0 + B].contiguous(), yg[lab0:lab0 + B].contiguous()
    kg = torch.randint(0, args.groups, (Bg,), device="cuda", generator=g)
    lse2, ce2, winv2, dls2 = (torch.empty(2, B, device="cuda") for _ in range(4))
    dXg, dYg = torch.empty(Bg, E, device="cuda"), torch.empty(Bg, E, device="cuda")
    dxl, dyl = torch.empty(B, E, device="cuda"), torch.empty(B, E, device="cuda")
    rows = torch.empty(B, 3, device="cuda")
    out3 = torch.empty(3, device="cuda")
    nrm2 = 1.0 / (2 * Bg)

    def softmax_streamed(k, w):
        w0, w1 = (w[0], w[1]) if w is not None else (None, None)
        T._ce_streamed_fwd(s, xl, yg, lsd, lab0, C, lse2[0], ce2[0], k, w0)
        T._ce_streamed_fwd(s, yl, xg, lsd, lab0, C, lse2[1], ce2[1], k, w1)
        T._ce_streamed_bwd(s, xl, yg, lsd, None, lse2[0], lab0, nrm2, C, dls2[0], dYg, dxl, k, w0)
        T._ce_streamed_bwd(s, yl, xg, lsd, None, lse2[1], lab0, nrm2, C, dls2[1], dXg, dyl, k, w1)

    def sigmoid_streamed(k):
        T._sigmoid_chunks(s, xl, yg, lsd, lbd, k, lab0, 1.0 / Bg, C, rows, None, dxl, dYg)
        call("clipmi_sigmoid_reduce", s, P_(rows), B, 1.0 / Bg, None, P_(out3), P_(out3[1:]), P_(out3[2:]), 0)

    res["streamed_4096x32768x768"] = report(
        f"streamed forward + backward, {B} x {Bg}, E = {E}, chunks of {C}",
        {"softmax": lambda: softmax_streamed(None, None), "softmax_keyed": lambda: softmax_streamed(kg, winv2),
         "sigmoid": lambda: sigmoid_streamed(None), "sigmoid_keyed": lambda: sigmoid_streamed(kg)},
        max(3, args.reps // 4), base="softmax")
    res["streamed_4096x32768x768"]["gemms"] = {"softmax": 32, "sigmoid": 12}
    lines[-1:-1] = ["  GEMMs per step: softmax 32 (4 per chunk and direction), sigmoid 12 (3 per chunk): 12 / 32 = 0.375"]

    # ---- the parts of one [4096, 8192] chunk alone: its three GEMMs, then its row kernels
    Sc = torch.rand(B, C, device="cuda", generator=g) * 2 - 1
    res["chunk_gemms_4096x8192x768"] = report(
        f"the GEMMs of one [{B}, {C}] chunk, E = {E} (exact f32)",
        {"scores = x_local y_all[c0:]^T": lambda: T._gemm_f32(B, C, E, xl, E, True, yg, E, True, Sc, C),
         "dy_all[c0:] = dS^T x_local": lambda: T._gemm_f32(C, E, B, Sc, C, False, xl, E, False, dYg, E),
         "dx_local += dS y_all[c0:]": lambda: T._gemm_f32(B, E, C, Sc, C, True, yg, E, False, dxl, E,
                                                           flags=T._lib.EPI_BETA)}, max(3, args.reps // 2))
    del Sc
    run2, run4, lab = torch.ones(B, 2, device="cuda"), torch.ones(B, 4, device="cuda"), torch.empty(B, device="cuda")

    def soft_chunk(S, dS):  # S read twice; S read, dS written
        def run():
            call("clipmi_contrastive_ce_fwd_chunk", s, P_(S), P_(lsd), B, C, C, Bg, lab0, P_(run2), P_(lab))
            call("clipmi_contrastive_ce_bwd_chunk", s, P_(S), P_(lse2[0]), P_(lsd), None, B, C, C, Bg, lab0, nrm2,
                 P_(dS), P_(dls2[0]), 0)
        return run

    def soft_chunk_keyed(S, dS):
        def run():
            call("clipmi_contrastive_keyed_fwd_chunk", s, P_(S), P_(lsd), P_(kg), B, C, C, Bg, lab0, P_(run4))
            call("clipmi_contrastive_keyed_bwd_chunk", s, P_(S), P_(lse2[0]), P_(winv2[0]), P_(lsd), None, P_(kg), B, C,
                 C, Bg, lab0, nrm2, P_(dS), P_(dls2[0]), 0)
        return run

    lse2.fill_(5.0)
    winv2.fill_(1.0)
    res["row_kernels_4096x8192"] = row_kernels("row kernels of one [4096, 8192] chunk", B, C, C, Bg, lab0, kg,
                                               soft_chunk, soft_chunk_keyed, args.reps * 2, 16)

    text = "\n".join(lines) + "\n" + json.dumps(res) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
