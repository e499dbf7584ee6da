"""Golden vectors for clipmi.evaluation's classification path (evaluation.py:17-68 of the reference).

Runs the REFERENCE's own ``evaluation.evaluate_model`` (sklearn's accuracy_score / confusion_matrix /
classification_report underneath) on a fake model whose ``predict`` replays fixed probabilities, over a
three-batch loader with a ragged last batch, and records what it computed:

  tests/golden/evaluation.npz          probs [37, 7], labels, preds, confidences, conf_matrix, accuracy
  tests/golden/evaluation_report.txt   the class_report string

Class 1 ("disgust") never occurs as a label but is predicted (the zero-support row), and class 2 ("fear") is a
label but never predicted (the zero_division branch of the precision), while every class still occurs among the
labels or the predictions, so sklearn's matrix covers all 7 classes.

The reference's evaluation.py imports seaborn (plots only), which this image lacks: an empty stand-in module goes
into sys.modules before the import, and matplotlib runs on the Agg backend.  Only the reference's results are
written, none of its source.

  python tools/gen_eval_golden.py --reference DIR   (CPU; needs torch, sklearn, matplotlib, tqdm, PIL)
"""
import argparse
import os
import sys
import types

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
N, C, BATCH = 37, 7, 16
NEVER_LABEL, NEVER_PRED = 1, 2


def fixture():
    """(probs [N, C] float32 softmax rows, labels [N] int64)."""
    rng = np.random.default_rng(2024)
    labels = rng.choice([c for c in range(C) if c != NEVER_LABEL], size=N).astype(np.int64)
    labels[:C - 1] = [c for c in range(C) if c != NEVER_LABEL]  # every other class is a label at least once
    logits = rng.standard_normal((N, C)) * 1.5
    hit = rng.random(N) < 0.6
    logits[hit, labels[hit]] += 3.0  # ~60 % correct
    logits[::9, NEVER_LABEL] += 6.0  # the label-less class is predicted a few times
    logits[:, NEVER_PRED] -= 8.0     # and one labelled class is never predicted
    e = np.exp(logits - logits.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32), labels


class _Eval:
    def eval(self):
        return self


class ReplayModel:
    """What evaluate_model touches: .model.eval() and predict(pixel_values); the pixel_values are row indices."""

    def __init__(self, probs):
        import torch
        self.model = _Eval()
        self.probs = torch.from_numpy(probs)

    def predict(self, pixel_values):
        return self.probs.to(pixel_values.device)[pixel_values.long()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CLIPMI_REFERENCE"),
                    help="checkout of the reference project (or CLIPMI_REFERENCE)")
    args = ap.parse_args()
    if not args.reference or not os.path.isfile(os.path.join(args.reference, "evaluation.py")):
        sys.exit("gen_eval_golden: --reference DIR must hold the reference's evaluation.py")
    import matplotlib
    matplotlib.use("Agg")
    sys.modules.setdefault("seaborn", types.ModuleType("seaborn"))
    sys.path.insert(0, args.reference)
    import torch
    import evaluation as ref_eval
    from constants import EMOTIONS

    probs, labels = fixture()
    idx, lab = torch.arange(N), torch.from_numpy(labels)
    loader = [(idx[i:i + BATCH], lab[i:i + BATCH], [f"img_{j:03d}.jpg" for j in range(i, min(i + BATCH, N))])
              for i in range(0, N, BATCH)]
    assert [len(b[0]) for b in loader] == [16, 16, 5]
    acc, cm, report, preds, labs, paths, confs, sims = ref_eval.evaluate_model(ReplayModel(probs), loader)
    assert cm.shape == (C, C) and len(EMOTIONS) == C and len(paths) == N
    assert cm[NEVER_LABEL].sum() == 0 and cm[:, NEVER_LABEL].sum() > 0 and cm[:, NEVER_PRED].sum() == 0
    assert np.array_equal(np.asarray(labs), labels) and np.array_equal(sims, probs)
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "evaluation.npz"), probs=probs, labels=labels,
                        preds=np.asarray(preds, dtype=np.int64), confidences=np.asarray(confs, dtype=np.float32),
                        conf_matrix=np.asarray(cm, dtype=np.int64), accuracy=np.float64(acc))
    with open(os.path.join(OUT, "evaluation_report.txt"), "w", encoding="utf-8") as f:
        f.write(report)
    print(report)
    print(f"accuracy {acc:.6f}; {N} rows, {C} classes -> {OUT}")


if __name__ == "__main__":
    main()
