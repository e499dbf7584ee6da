#!/usr/bin/env python3
"""Times the colour augmentation (clipmi.images.color_jitter_u8 -> clipmi_color_u8) against the only alternative
there is: the host loop of PIL calls that torchvision's ColorJitter makes on PIL images, producing the same bytes.

  cases   all four ops in random orders (ColorJitter(0.4, 0.4, 0.4, 0.1).sample); contrast only; hue only
  GPU     the call works in place, so every timed call gets a fresh copy of the batch (`inner` copies made outside
          the timed region): device events around `inner` back-to-back calls, after a warm-up; the median, minimum
          and maximum of `repeats` such samples, per call.  Bytes moved: one read and one write of the batch, plus
          one more read for images with a contrast (pass 1), against the 8 TB/s HBM peak.
  PIL     the same records applied image by image on one core (ImageEnhance.Brightness / Contrast / Color, the HSV
          hue shift); the bytes are compared with the GPU's before anything is timed.  Reported per core and scaled
          to the 16 CPUs a job gets.  --pil-only times this side alone (no GPU needed; the bytes are then compared
          with tests/color_ref.py on the first images).

Output: one line per measurement, then a JSON line.

  python tools/color_bench.py [--batch 256] [--size 224] [--repeats 15] [--inner 20] [--pil-only]
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

from clipmi.images import ColorJitter, color_jitter_u8  # noqa: E402

HBM_PEAK = 8e12  # bytes / s
JOB_CPUS = 16


def pil_chain(Image, ImageEnhance, img, item):
    """One uint8 [H, W, 3] array through item's ops as torchvision's PIL path applies them."""
    p = Image.fromarray(img)
    enh = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast, "saturation": ImageEnhance.Color}
    for name, value in item.ops():
        if name == "hue":
            h, s, v = p.convert("HSV").split()
            nh = (np.array(h, dtype=np.uint8).astype(np.int32) + value).astype(np.uint8)
            p = Image.merge("HSV", (Image.fromarray(nh), s, v)).convert("RGB")
        else:
            p = enh[name](p).enhance(value)
    if item.gray:
        p = p.convert("L").convert("RGB")
    return np.asarray(p)


def gpu_timed(src, items, repeats, inner, warmup=3):
    """ms per call: (median, min, max) over `repeats` samples of `inner` calls, each on its own copy of src."""
    copies = [src.clone() for _ in range(inner)]
    for c in copies[:warmup]:
        color_jitter_u8(c, items)
    samples = []
    for _ in range(repeats):
        for c in copies:
            c.copy_(src)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for c in copies:
            color_jitter_u8(c, items)
        b.record()
        b.synchronize()
        samples.append(a.elapsed_time(b) / inner)
    return statistics.median(samples), min(samples), max(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pil-only", action="store_true")
    args = ap.parse_args()
    B, S = args.batch, args.size
    gpu = not args.pil_only
    if gpu and not torch.cuda.is_available():
        sys.exit("color_bench needs a GPU (or --pil-only)")
    try:
        from PIL import Image, ImageEnhance
    except ImportError:
        Image = ImageEnhance = None
        if not gpu:
            sys.exit("--pil-only needs PIL")
    rng = np.random.default_rng(args.seed)
    host = rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    g = torch.Generator().manual_seed(args.seed)
    cases = {"all_four_random_orders": ColorJitter(0.4, 0.4, 0.4, 0.1).sample(B, g),
             "contrast_only": ColorJitter(contrast=0.4).sample(B, g),
             "hue_only": ColorJitter(hue=0.1).sample(B, g)}
    res = {"batch": B, "size": S, "repeats": args.repeats, "inner": args.inner, "host": platform.processor() or
           platform.machine(), "device": torch.cuda.get_device_name(0) if gpu else None,
           "pil": None if Image is None else Image.__version__}
    print(f"B = {B}, S = {S}; GPU: {res['device']}; host CPU for the PIL loop: {res['host']} "
          f"({'this machine' if gpu else 'no GPU on this machine'}); PIL {res['pil']}", flush=True)
    src = torch.from_numpy(host).cuda() if gpu else None
    for name, items in cases.items():
        r = res[name] = {}
        got = color_jitter_u8(src.clone(), items).cpu().numpy() if gpu else None
        if Image is not None:
            t0 = time.perf_counter()
            ref = np.stack([pil_chain(Image, ImageEnhance, host[b], items[b]) for b in range(B)])
            per_image = (time.perf_counter() - t0) / B * 1e3
            if gpu:  # results first: the timed paths agree
                assert np.array_equal(got, ref), f"{name}: the GPU call and the PIL loop differ"
            else:
                import color_ref
                n = min(B, 8)
                assert np.array_equal(np.stack([color_ref.apply_item(host[b], items[b]) for b in range(n)]), ref[:n])
            r["pil_ms_per_image_one_core"] = per_image
            r["pil_images_per_s_one_core"] = 1e3 / per_image
            r["pil_images_per_s_16_cores_scaled"] = JOB_CPUS * 1e3 / per_image
            print(f"{name:26s} PIL loop  {per_image:8.3f} ms/image on one core = {1e3 / per_image:8.0f} images/s; "
                  f"x{JOB_CPUS} cores (scaled, not measured) {JOB_CPUS * 1e3 / per_image:8.0f} images/s"
                  f"{'; same bytes as the GPU call' if gpu else '; same bytes as tests/color_ref.py'}", flush=True)
        if gpu:
            t = gpu_timed(src, items, args.repeats, args.inner)
            with_contrast = sum(1 for it in items if "contrast" in dict(it.ops()))
            moved = (2 * B + with_contrast) * S * S * 3
            r.update(median_ms=t[0], min_ms=t[1], max_ms=t[2], bytes_moved=moved,
                     fraction_of_hbm_peak=moved / (t[0] * 1e-3) / HBM_PEAK, images_per_s=B / t[0] * 1e3)
            print(f"{name:26s} GPU call  median {t[0]:8.4f} ms   min {t[1]:8.4f}   max {t[2]:8.4f}   "
                  f"({B / t[0] * 1e3:10.0f} images/s; {moved / 1e6:.1f} MB moved = {moved / (t[0] * 1e-3) / 1e12:.3f} TB/s, "
                  f"{100 * r['fraction_of_hbm_peak']:.1f}% of the 8 TB/s peak)", flush=True)
            if Image is not None:
                r["gpu_vs_pil_16_cores_scaled"] = r["images_per_s"] / r["pil_images_per_s_16_cores_scaled"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
