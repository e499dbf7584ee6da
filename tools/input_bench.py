#!/usr/bin/env python3
"""Times the ragged input step (clipmi.images.preprocess -> clipmi_resize_crop_u8) against what the library
offered before it.

  ragged batch   B images with sides drawn from 100..600 by a fixed seed: the ragged call in both modes, and the
                 only alternative there was: a per-image loop of resize_uint8 + the centre slice copied into the
                 batch tensor
  uniform batch  B x (300 x 451): the ragged call against resize_uint8 on the whole tensor (whose centre crop is
                 free: clipmi_im2col_u8 does it)

Device events around `inner` back-to-back calls, after a warm-up; the median, minimum and maximum of `repeats`
such samples, per call.  Needs a GPU.  Output: one line per measurement, then a JSON line.

  python tools/input_bench.py [--batch 256] [--size 224] [--repeats 15] [--inner 100]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "vlm-clip_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from clipmi import towers as T  # noqa: E402
from clipmi.images import ImageBatch, preprocess  # noqa: E402


def timed(fn, repeats, inner, warmup=3):
    """ms per call: (median, min, max) over `repeats` samples of `inner` calls each."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b) / inner)
    return statistics.median(samples), min(samples), max(samples)


def loop_of_resizes(images, S, out):
    """The per-image path: one resize_uint8 per image (up to four launches), its centre window into the batch."""
    for b, im in enumerate(images):
        h, w = im.shape[0], im.shape[1]
        oh, ow = T.shortest_edge_size(h, w, S)
        r = T.resize_uint8(im[None], oh, ow) if (oh, ow) != (h, w) else im[None]
        y0, x0 = (oh - S) // 2, (ow - S) // 2
        out[b].copy_(r[0, y0:y0 + S, x0:x0 + S])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("input_bench needs a GPU")
    B, S = args.batch, args.size
    rng = np.random.default_rng(args.seed)
    sides = rng.integers(100, 601, (B, 2))
    host = [torch.from_numpy(rng.integers(0, 256, (int(h), int(w), 3), dtype=np.uint8)) for h, w in sides]
    dev = [im.cuda() for im in host]
    ragged = ImageBatch.pack(host).to("cuda")
    out = torch.empty(B, S, S, 3, dtype=torch.uint8, device="cuda")
    res = {"batch": B, "size": S, "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "inner": args.inner, "ragged_megapixels": float(sides.prod(1).sum()) / 1e6}

    # results first: the timed paths agree
    ref = loop_of_resizes(dev, S, torch.empty_like(out))
    assert torch.equal(preprocess(ragged, S, "processor"), ref), "ragged call differs from the per-image loop"

    def report(name, t):
        res[name] = {"median_ms": t[0], "min_ms": t[1], "max_ms": t[2]}
        print(f"{name:34s} median {t[0]:9.3f} ms   min {t[1]:9.3f}   max {t[2]:9.3f}   "
              f"({B / t[0] * 1e3:10.0f} images/s)", flush=True)

    report("ragged/call_processor", timed(lambda: preprocess(ragged, S, "processor", out=out), args.repeats, args.inner))
    report("ragged/call_square", timed(lambda: preprocess(ragged, S, "square", out=out), args.repeats, args.inner))
    report("ragged/per_image_loop", timed(lambda: loop_of_resizes(dev, S, out), args.repeats, max(1, args.inner // 20), warmup=1))

    uni = torch.from_numpy(rng.integers(0, 256, (B, 300, 451, 3), dtype=np.uint8)).cuda()
    ubatch = ImageBatch.pack(list(uni.cpu())).to("cuda")
    oh, ow = T.shortest_edge_size(300, 451, S)
    y0, x0 = (oh - S) // 2, (ow - S) // 2
    assert torch.equal(preprocess(ubatch, S, "processor"), T.resize_uint8(uni, oh, ow)[:, y0:y0 + S, x0:x0 + S])
    report("uniform/call_processor", timed(lambda: preprocess(ubatch, S, "processor", out=out), args.repeats, args.inner))
    report("uniform/resize_uint8", timed(lambda: T.resize_uint8(uni, oh, ow), args.repeats, args.inner))
    res["ragged_call_vs_loop"] = res["ragged/per_image_loop"]["median_ms"] / res["ragged/call_processor"]["median_ms"]
    res["uniform_call_vs_resize_uint8"] = (res["uniform/resize_uint8"]["median_ms"]
                                           / res["uniform/call_processor"]["median_ms"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
