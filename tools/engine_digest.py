"""sha256 of everything the encoder engine returns (out, dx, every gradient) over a fixed set of cases: two builds
that print the same lines compute the same bits.  Runs on the GPU, every case in one process:

    python tools/engine_digest.py > digest.txt

Uses tests/engine_harness.py alone, so the same two files run in a checkout of an earlier commit.  Cases (D = 128,
H = 2, F = 512, L = 2, each in fp32 / bf16 / bf16 with the fp32 residual stream): the full engine non-causal and
causal with a mask, the first_token mode with and without a mask below and above the split-K threshold, the
cls_last mode likewise, its chunked backward, and its bf16 cases with CLIPMI_DEFER=0."""
import hashlib
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tests"), os.path.join(REPO, "vlm-clip_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

import engine_harness as E  # noqa: E402

L = 2
# (label, mode, B, N, causal, mask kind, chunks, CLIPMI_DEFER, bf16 modes only)
CASES = [("full", "full", 33, 50, False, "null", None, None, False),
         ("full_causal_key0", "full", 33, 7, True, "key0", None, None, False)]
CASES += [(f"first_token_{m}", "first_token", B, 7, True, m, None, None, False)
          for B in (33, 1100) for m in ("null", "key0")]
CASES += [("cls_last", "cls_last", B, N, False, "null", None, None, False) for B, N in ((33, 50), (1100, 2))]
CASES += [("cls_last_chunked", "cls_last", 33, 50, False, "null", [(2, 1), (1, 0)], None, False)]
CASES += [("cls_last_defer0", "cls_last", B, N, False, "null", None, "0", True) for B, N in ((33, 50), (1100, 2))]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def main():
    for label, mode, B, N, causal, mkind, chunks, defer, bf16_only in CASES:
        for prec, (dtype, r32) in E.MODES.items():
            if bf16_only and dtype != torch.bfloat16:
                continue
            os.environ.pop("CLIPMI_DEFER", None)
            if defer is not None:
                os.environ["CLIPMI_DEFER"] = defer
            weights = E.make_weights(7, dtype, L)
            x0, dy0 = E.inputs(B, N)
            out, dx, grads = E.run_engine(mode, dtype, r32, B, N, L, weights, x0, dy0, causal=causal,
                                          mask=E.make_mask(mkind, B, N), chunks=chunks)
            tag = f"{label} B={B} N={N} {prec}"
            print(f"{tag} out {sha(out)}")
            print(f"{tag} dx {sha(dx)}")
            for n in sorted(grads):
                print(f"{tag} grad/{n} {sha(grads[n])}")
    os.environ.pop("CLIPMI_DEFER", None)


if __name__ == "__main__":
    main()
