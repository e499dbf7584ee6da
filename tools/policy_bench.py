#!/usr/bin/env python3
"""Times the policy augmentations (clipmi.images.apply_policy_u8 over clipmi_affine_u8, clipmi_enhance_u8 and
clipmi_color_u8) against the only alternative there is: the host loop of PIL calls that torchvision's RandAugment and
TrivialAugmentWide make on PIL images, producing the same bytes.

  cases   RandAugment().sample and TrivialAugmentWide().sample (two ops and one op per image, "nearest", fill 0), and,
          for the kernel alone, enhance_u8 with every image an equalize and with the five ops in turn
  GPU     src -> dst, so calls repeat on the same buffers: device events around `inner` back-to-back calls, after a
          warm-up of `warmup` calls; the median, minimum and maximum of `repeats` such samples, per call.  The launch
          count of a call is counted from its plan (policy_calls): an affine call is one launch and a pre-pass when
          some item is axis-aligned under "nearest", an enhance call one launch, or three when some item needs a
          histogram, a colour call two.
  PIL     ImageOps / ImageEnhance / Image.transform / Image.rotate image by image on one core; the bytes are compared
          with the GPU's before anything is timed.  Reported per core and scaled to the 16 CPUs a job gets.
          --pil-only times this side alone (no GPU needed; the bytes are then compared with tests/enhance_ref.py on
          the first images).

Output: one line per measurement, then a JSON line.

  python tools/policy_bench.py [--batch 256] [--size 224] [--repeats 15] [--inner 50] [--warmup 10] [--pil-only]
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

from clipmi.images import (EnhanceItem, RandAugment, TrivialAugmentWide, apply_policy_u8, enhance_u8,  # noqa: E402
                           policy_calls, policy_matrix)

JOB_CPUS = 16


def pil_op(P, p, name, m):
    """autoaugment._apply_op on a PIL image ("nearest", fill 0)."""
    w, h = p.size
    if name == "Identity":
        return p
    if name in ("ShearX", "ShearY", "TranslateX", "TranslateY"):
        return p.transform((w, h), P.Image.AFFINE, policy_matrix(name, m, w, h), P.Image.NEAREST, fillcolor=(0, 0, 0))
    if name == "Rotate":
        return p.rotate(m, P.Image.NEAREST, fillcolor=(0, 0, 0))
    if name in ("Brightness", "Color", "Contrast", "Sharpness"):
        return getattr(P.ImageEnhance, name)(p).enhance(1.0 + m)
    if name == "Posterize":
        return P.ImageOps.posterize(p, int(m))
    if name == "Solarize":
        return P.ImageOps.solarize(p, m)
    return P.ImageOps.autocontrast(p) if name == "AutoContrast" else P.ImageOps.equalize(p)


def pil_program(P, img, program):
    p = P.Image.fromarray(img)
    for name, m in program:
        p = pil_op(P, p, name, m)
    return np.asarray(p)


def launches(calls):
    """Kernel launches of a plan, by kind."""
    n = {"affine": 0, "enhance": 0, "color": 0}
    for kind, items in calls:
        if kind == "affine":
            n[kind] += 1 + any(it.filter == 0 and it.m[1] == 0.0 and it.m[3] == 0.0 for it in items)
        elif kind == "enhance":
            n[kind] += 3 if any(it.op in (3, 4) for it in items) else 1
        else:
            n[kind] += 2
    return n


def gpu_timed(fn, repeats, inner, warmup):
    """ms per call: (median, min, max) over `repeats` samples of `inner` calls."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pil-only", action="store_true")
    args = ap.parse_args()
    B, S = args.batch, args.size
    gpu = not args.pil_only
    if gpu and not torch.cuda.is_available():
        sys.exit("policy_bench needs a GPU (or --pil-only)")
    try:
        import PIL.Image
        import PIL.ImageEnhance
        import PIL.ImageOps
        P = PIL
    except ImportError:
        P = None
        if not gpu:
            sys.exit("--pil-only needs PIL")
    rng = np.random.default_rng(args.seed)
    host = rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    g = torch.Generator().manual_seed(args.seed)
    cases = {"RandAugment": RandAugment().sample(B, S, g), "TrivialAugmentWide": TrivialAugmentWide().sample(B, S, g)}
    res = {"batch": B, "size": S, "repeats": args.repeats, "inner": args.inner, "warmup": args.warmup,
           "host": platform.processor() or platform.machine(), "device": torch.cuda.get_device_name(0) if gpu else None,
           "pil": None if P is None else P.__version__, "library": os.environ.get("CLIPMI_LIB", "libclipmi.so")}
    print(f"B = {B}, S = {S}; GPU: {res['device']}; host CPU for the PIL loop: {res['host']} "
          f"({'this machine' if gpu else 'no GPU on this machine'}); PIL {res['pil']}; library {res['library']}", flush=True)
    src = torch.from_numpy(host).cuda() if gpu else None
    dst = torch.empty_like(src) if gpu else None
    for name, programs in cases.items():
        r = res[name] = {}
        calls = policy_calls(programs, S, S)
        r["calls"] = [kind for kind, _ in calls]
        r["launches"] = launches(calls)
        r["launches_total"] = sum(r["launches"].values())
        print(f"{name:22s} plan      {len(calls)} calls ({' '.join(r['calls'])}), {r['launches_total']} launches per call "
              f"for {B} images ({r['launches']})", flush=True)
        got = apply_policy_u8(src, programs, out=dst).cpu().numpy() if gpu else None
        if P is not None:
            t0 = time.perf_counter()
            ref = np.stack([pil_program(P, host[b], programs[b]) for b in range(B)])
            per_image = (time.perf_counter() - t0) / B * 1e3
            if gpu:  # results first: the timed paths agree
                assert np.array_equal(got, ref), f"{name}: the GPU call and the PIL loop differ"
            else:
                import enhance_ref
                n = min(B, 8)
                assert np.array_equal(np.stack([enhance_ref.apply_program(host[b], programs[b]) for b in range(n)]), ref[:n])
            r["pil_ms_per_image_one_core"] = per_image
            r["pil_images_per_s_one_core"] = 1e3 / per_image
            r["pil_images_per_s_16_cores_scaled"] = JOB_CPUS * 1e3 / per_image
            print(f"{name:22s} PIL loop  {per_image:8.3f} ms/image on one core = {1e3 / per_image:8.0f} images/s; "
                  f"x{JOB_CPUS} cores (scaled, not measured) {JOB_CPUS * 1e3 / per_image:8.0f} images/s"
                  f"{'; same bytes as the GPU call' if gpu else '; same bytes as tests/enhance_ref.py'}", flush=True)
        if gpu:
            t = gpu_timed(lambda: apply_policy_u8(src, programs, out=dst), args.repeats, args.inner, args.warmup)
            r.update(median_ms=t[0], min_ms=t[1], max_ms=t[2], images_per_s=B / t[0] * 1e3)
            print(f"{name:22s} GPU call  median {t[0]:8.4f} ms   min {t[1]:8.4f}   max {t[2]:8.4f}   "
                  f"({B / t[0] * 1e3:10.0f} images/s)", flush=True)
            if P is not None:
                r["gpu_vs_pil_16_cores_scaled"] = r["images_per_s"] / r["pil_images_per_s_16_cores_scaled"]
                r["gpu_vs_pil_one_core"] = r["images_per_s"] / r["pil_images_per_s_one_core"]
                print(f"{name:22s} ratio     {r['gpu_vs_pil_one_core']:8.1f}x one core, "
                      f"{r['gpu_vs_pil_16_cores_scaled']:8.1f}x 16 cores (scaled)", flush=True)
    if gpu:  # the kernel alone
        ops = [("equalize", 0), ("autocontrast", 0), ("sharpness", 1.5), ("posterize", 4), ("solarize", 128)]
        kernel_cases = {"enhance_all_equalize": [EnhanceItem.of("equalize")] * B,
                        "enhance_five_ops": [EnhanceItem.of(*ops[b % 5]) for b in range(B)],
                        "enhance_no_histogram": [EnhanceItem.of(*ops[2 + b % 3]) for b in range(B)]}
        for name, items in kernel_cases.items():
            t = gpu_timed(lambda: enhance_u8(src, items, out=dst), args.repeats, args.inner, args.warmup)
            moved = 2 * B * S * S * 3
            res[name] = dict(median_ms=t[0], min_ms=t[1], max_ms=t[2], bytes_moved=moved,
                             effective_gb_per_s=moved / (t[0] * 1e-3) / 1e9)
            print(f"{name:22s} GPU call  median {t[0]:8.4f} ms   min {t[1]:8.4f}   max {t[2]:8.4f}   "
                  f"({moved / 1e6:.1f} MB written and read once = {res[name]['effective_gb_per_s']:.1f} GB/s effective)",
                  flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
