#!/usr/bin/env python3
"""Times the affine augmentation (clipmi.images.affine_u8 -> clipmi_affine_u8) against the only alternative there is:
the host loop of PIL calls that torchvision's RandomAffine makes on PIL images, producing the same bytes.

  cases   RandomAffine(15, (0.1, 0.1), (0.9, 1.1), 10).sample under "nearest" (PIL's 16.16 fixed-point path) and
          under "bilinear"; RandomAffine(0, (0.1, 0.1), (0.9, 1.1)) under "nearest" (the axis-aligned path: tables
          built on the host and uploaded with the records)
  GPU     src -> dst, so calls repeat on the same buffers: device events around `inner` back-to-back calls, after a
          warm-up of `warmup` calls; the median, minimum and maximum of `repeats` such samples, per call.  Effective
          bytes: one read and one write of the batch (the gather re-reads from L2, which is not counted), against
          the 8 TB/s HBM peak; profiles/color_jitter_bench.log has the colour pass's figure on the same terms.
  PIL     Image.transform(size, AFFINE, m, resample, fillcolor=...) image by image on one core; the bytes are
          compared with the GPU's before anything is timed.  Reported per core and scaled to the 16 CPUs a job
          gets.  --pil-only times this side alone (no GPU needed; the bytes are then compared with
          tests/affine_ref.py on the first images).

Output: one line per measurement, then a JSON line.

  python tools/affine_bench.py [--batch 256] [--size 224] [--repeats 15] [--inner 200] [--warmup 20] [--pil-only]
"""
import argparse
import json
import os
import platform
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "vlm-clip_amd"), os.path.join(REPO, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from clipmi.images import RandomAffine, affine_u8  # noqa: E402

HBM_PEAK = 8e12  # bytes / s
JOB_CPUS = 16


def pil_affine(Image, img, item):
    """One uint8 [H, W, 3] array through item as torchvision's PIL path applies it."""
    h, w, _ = img.shape
    fill = (item.fill >> 16 & 255, item.fill >> 8 & 255, item.fill & 255)
    resample = Image.BILINEAR if item.filter == 1 else Image.NEAREST
    return np.asarray(Image.fromarray(img).transform((w, h), Image.AFFINE, item.matrix, resample, fillcolor=fill))


def gpu_timed(src, dst, items, repeats, inner, warmup):
    """ms per call: (median, min, max) over `repeats` samples of `inner` calls."""
    for _ in range(warmup):
        affine_u8(src, items, out=dst)
    torch.cuda.synchronize()
    samples = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            affine_u8(src, items, out=dst)
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b) / inner)
    return statistics.median(samples), min(samples), max(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pil-only", action="store_true")
    args = ap.parse_args()
    B, S = args.batch, args.size
    gpu = not args.pil_only
    if gpu and not torch.cuda.is_available():
        sys.exit("affine_bench needs a GPU (or --pil-only)")
    try:
        from PIL import Image
    except ImportError:
        Image = None
        if not gpu:
            sys.exit("--pil-only needs PIL")
    rng = np.random.default_rng(args.seed)
    host = rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    g = torch.Generator().manual_seed(args.seed)
    recipe = (15, (0.1, 0.1), (0.9, 1.1), 10)
    cases = {"nearest_fixed_point": RandomAffine(*recipe, interpolation="nearest", fill=(124, 116, 104)).sample(B, S, g),
             "bilinear": RandomAffine(*recipe, interpolation="bilinear", fill=(124, 116, 104)).sample(B, S, g),
             "nearest_axis_aligned": RandomAffine(0, (0.1, 0.1), (0.9, 1.1), fill=(124, 116, 104)).sample(B, S, g)}
    res = {"batch": B, "size": S, "repeats": args.repeats, "inner": args.inner, "warmup": args.warmup,
           "host": platform.processor() or platform.machine(), "device": torch.cuda.get_device_name(0) if gpu else None,
           "pil": None if Image is None else Image.__version__}
    print(f"B = {B}, S = {S}; GPU: {res['device']}; host CPU for the PIL loop: {res['host']} "
          f"({'this machine' if gpu else 'no GPU on this machine'}); PIL {res['pil']}", flush=True)
    src = torch.from_numpy(host).cuda() if gpu else None
    dst = torch.empty_like(src) if gpu else None
    for name, items in cases.items():
        r = res[name] = {}
        got = affine_u8(src, items, out=dst).cpu().numpy() if gpu else None
        if Image is not None:
            t0 = time.perf_counter()
            ref = np.stack([pil_affine(Image, host[b], items[b]) for b in range(B)])
            per_image = (time.perf_counter() - t0) / B * 1e3
            if gpu:  # results first: the timed paths agree
                assert np.array_equal(got, ref), f"{name}: the GPU call and the PIL loop differ"
            else:
                import affine_ref
                n = min(B, 8)
                assert np.array_equal(np.stack([affine_ref.apply_item(host[b], items[b]) for b in range(n)]), ref[:n])
            r["pil_ms_per_image_one_core"] = per_image
            r["pil_images_per_s_one_core"] = 1e3 / per_image
            r["pil_images_per_s_16_cores_scaled"] = JOB_CPUS * 1e3 / per_image
            print(f"{name:22s} PIL loop  {per_image:8.3f} ms/image on one core = {1e3 / per_image:8.0f} images/s; "
                  f"x{JOB_CPUS} cores (scaled, not measured) {JOB_CPUS * 1e3 / per_image:8.0f} images/s"
                  f"{'; same bytes as the GPU call' if gpu else '; same bytes as tests/affine_ref.py'}", flush=True)
        if gpu:
            t = gpu_timed(src, dst, items, args.repeats, args.inner, args.warmup)
            moved = 2 * B * S * S * 3
            r.update(median_ms=t[0], min_ms=t[1], max_ms=t[2], bytes_moved=moved,
                     effective_gb_per_s=moved / (t[0] * 1e-3) / 1e9,
                     fraction_of_hbm_peak=moved / (t[0] * 1e-3) / HBM_PEAK, images_per_s=B / t[0] * 1e3)
            print(f"{name:22s} GPU call  median {t[0]:8.4f} ms   min {t[1]:8.4f}   max {t[2]:8.4f}   "
                  f"({B / t[0] * 1e3:10.0f} images/s; {moved / 1e6:.1f} MB moved = {r['effective_gb_per_s']:.1f} GB/s "
                  f"effective, {100 * r['fraction_of_hbm_peak']:.1f}% of the 8 TB/s peak)", flush=True)
            if Image is not None:
                r["gpu_vs_pil_16_cores_scaled"] = r["images_per_s"] / r["pil_images_per_s_16_cores_scaled"]
                r["gpu_vs_pil_one_core"] = r["images_per_s"] / r["pil_images_per_s_one_core"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
