"""GEMM kernel selection without a GPU: clipmi_gemm_plan() reports what clipmi_gemm / clipmi_gemm_x3out would launch
(csrc/gemm_plan.cpp; the launch calls the same gemm_plan()).  Operand pointers are fabricated integers of a chosen
alignment, never dereferenced.  The expected kernels were read off a rocprofv3 kernel trace of the library before
selection became a plan (profiles/gemm_plan_kernel_trace.log), not off the plan code."""
import ast
import ctypes
import os
import subprocess
import sys

import pytest

from clipmi import _lib
from clipmi._lib import BF16, F32, FP8, GemmDesc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E = _lib
B_, Q, G, R_, DQ, DG, BETA, P, DA, MA = (E.EPI_BIAS, E.EPI_QGELU, E.EPI_GELU, E.EPI_RESID, E.EPI_DQGELU, E.EPI_DGELU,
                                         E.EPI_BETA, E.EPI_STORE_PRE, E.EPI_STORE_DACT, E.EPI_MUL_AUX)
PTR = 1 << 20  # 16-byte (and 256-byte) aligned


def desc(M, N, K, akm=True, bkm=True, flags=0, c=BF16, ab=BF16, split=1, bias_grad=False, force=0, **over):
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.A, d.B, d.C = PTR, 2 * PTR, 3 * PTR
    d.a_kmajor, d.b_kmajor = int(akm), int(bkm)
    d.lda = K if akm else M
    d.ldb = K if bkm else N
    d.ldc = d.ldr = d.ldaux = N
    d.bias, d.residual, d.aux = 4 * PTR, 5 * PTR, 6 * PTR
    d.alpha, d.flags = 1.0, flags
    d.ab_dtype, d.c_dtype, d.bias_dtype = ab, c, F32
    d.split_k = split
    if split > 1:
        d.workspace, d.workspace_bytes = 8 * PTR, split * M * (N + 1) * 4
    if bias_grad:
        d.bias_grad = 7 * PTR
    if ab == FP8:
        d.a_scale, d.b_scale = 9 * PTR, 10 * PTR
        if c == FP8:
            d.c_scale = 11 * PTR
    d.force_small_tile = force
    for k, v in over.items():
        setattr(d, k, v)
    return d


def plan(*a, x3out=False, **kw):
    return _lib.gemm_plan(desc(*a, **kw), x3out)


def kernel(*a, **kw):
    return plan(*a, **kw)["kernel"]


def wgrad(M, N, K, **kw):
    kw.setdefault("flags", BETA)
    return desc(M, N, K, akm=False, bkm=False, c=F32, **kw)


def error_of(d, x3out=False):
    info = _lib.GemmPlanInfo()
    st = _lib.lib().clipmi_gemm_plan(ctypes.byref(d), int(x3out), ctypes.byref(info))
    return st, _lib.lib().clipmi_last_error().decode()


def test_version_and_names():
    import kernel_checks as KC
    assert _lib.lib().clipmi_version() >= 10  # 9: before clipmi_gemm_plan
    for n in ("FORCE_RULE", "FORCE_128", "FORCE_ASM8", "FORCE_PP8", "FORCE_W4P", "FORCE_W4P_PF"):
        assert getattr(KC, n) == getattr(_lib, n)
    assert (_lib.FORCE_RULE, _lib.FORCE_128, _lib.FORCE_ASM8, _lib.FORCE_PP8, _lib.FORCE_W4P, _lib.FORCE_W4P_PF,
            _lib.FORCE_FP8_8W, _lib.FORCE_FP8_RULE, _lib.FORCE_PP8_STAGGER) == (0, 1, 4, 9, 28, 32, 40, 41, 100)


# ---- the production rule, k-major A, bf16, M = 512
@pytest.mark.parametrize("K,N,akm_bkm,flags,c,want", [
    (512, 1536, (1, 1), B_, BF16, "pp8"), (768, 2304, (1, 1), B_, BF16, "pp8"),
    (768, 768, (1, 1), B_ | R_, BF16, "pp8"), (768, 3072, (1, 1), B_ | Q | DA, BF16, "pp8"),
    (1536, 768, (1, 1), B_, BF16, "w4p"), (3072, 768, (1, 1), B_ | R_, BF16, "w4p"),
    (1024, 1024, (1, 1), B_, BF16, "pp8"), (1024, 4096, (1, 1), B_ | Q | P, BF16, "pp8"),
    (768, 3072, (1, 0), MA, BF16, "w4p_pf"),   # fc2's input gradient, stored-derivative product
    (768, 768, (1, 0), 0, BF16, "w4p_pf"),     # out-proj's input gradient
    (512, 512, (1, 0), 0, BF16, "w4p_pf"),
    (1024, 1024, (1, 0), 0, BF16, "pp8"),
    (3072, 768, (1, 0), 0, BF16, "w4p"), (2304, 768, (1, 0), 0, BF16, "w4p"),
    (768, 3072, (1, 0), DQ, BF16, "pp8"),
    # fp32-output instances: K = 3072 -> 4-wave, K = 768 -> ping-pong
    (3072, 768, (1, 1), B_, F32, "w4p"), (3072, 768, (1, 1), B_ | R_, F32, "w4p"), (3072, 768, (1, 1), 0, F32, "w4p"),
    (768, 768, (1, 1), B_, F32, "pp8"), (768, 768, (1, 1), B_ | R_, F32, "pp8"), (768, 768, (1, 1), 0, F32, "pp8"),
    (3072, 768, (1, 0), 0, F32, "w4p"), (768, 768, (1, 0), 0, F32, "pp8"), (768, 3072, (1, 0), MA, F32, "pp8"),
])
def test_production_rule(K, N, akm_bkm, flags, c, want):
    p = plan(512, N, K, akm=akm_bkm[0], bkm=akm_bkm[1], flags=flags, c=c)
    assert p["kernel"] == want
    assert p["tile"] == 256 and p["specialised"] == 1 and p["label"].startswith("gemm256_")


@pytest.mark.parametrize("split,bias", [(1, False), (1, True), (2, False), (4, True)])
@pytest.mark.parametrize("M,N", [(768, 3072), (3072, 768), (768, 768), (2304, 768)])
def test_every_wgrad_is_persistent_4wave(M, N, split, bias):
    p = _lib.gemm_plan(wgrad(M, N, 512, split=split, bias_grad=bias))
    assert p["kernel"] == "w4p" and p["bias_grad"] == int(bias)
    assert p["label"] == ("gemm256_wgrad_splitk" if split > 1 else "gemm256_wgrad")
    assert p["splits"] == split and p["reduce"] == (1 if split > 1 else 0)


def test_x3out_products(monkeypatch):
    fc1 = dict(flags=B_ | Q | DA, c=F32, ldc=3 * 3072, x3out=True)
    fc2d = dict(akm=True, bkm=False, flags=MA, c=F32, ldc=3 * 3072, x3out=True)
    assert plan(512, 3072, 2304, **fc1) == dict(plan(512, 3072, 2304, **fc1), kernel="w4p",
                                                 label="gemm256_fwd_bias_qgelu_dact_f32")
    assert plan(512, 3072, 2304, **dict(fc1, flags=B_ | Q))["label"] == "gemm256_fwd_bias_qgelu_f32"
    assert plan(512, 3072, 2304, **fc2d)["kernel"] == "w4p"
    assert plan(512, 3072, 2304, **fc2d)["label"] == "gemm256_dgrad_mulaux_f32"
    monkeypatch.setenv("CLIPMI_GEMM_X3_W4", "0")  # read per call
    assert plan(512, 3072, 2304, **fc1)["kernel"] == "pp8"
    assert plan(512, 3072, 2304, **fc2d)["kernel"] == "pp8"
    # the same flags without the image output have no 4-wave instance
    assert kernel(512, 3072, 2304, flags=B_ | Q | DA, c=F32) == "pp8"


# ---- fallbacks
def test_fallbacks_to_the_128_kernel():
    for p in (plan(255, 768, 768, flags=B_), plan(512, 120, 768, flags=B_), plan(512, 768, 96, flags=B_),
              plan(512, 127, 768, flags=B_)):
        assert (p["kernel"], p["tile"], p["label"], p["specialised"]) == ("bf16_128", 128, "gemm_fwd_bias", 1)
    assert kernel(256, 128, 64, flags=B_) == "pp8"
    # an unspecialised flag set on a 256-eligible shape: the 128 kernel (it has the gelu instances) ...
    p = plan(512, 768, 768, flags=B_ | G)
    assert (p["kernel"], p["label"], p["specialised"]) == ("bf16_128", "gemm_fwd_bias_gelu", 1)
    # ... and its runtime-flag instance for what no list has
    for kw in (dict(flags=Q), dict(flags=B_ | Q | R_), dict(akm=True, bkm=False, flags=B_), dict(flags=B_ | G, c=F32),
               dict(akm=False, bkm=True, c=F32), dict(split=2, c=F32)):
        p = plan(512, 768, 768, **kw)
        assert (p["kernel"], p["label"], p["specialised"], p["tile"]) == ("bf16_128", "gemm_generic", 0, 128), kw
    assert plan(248, 120, 512, akm=False, bkm=False, c=F32, flags=BETA)["label"] == "gemm_wgrad"
    assert plan(248, 120, 512, akm=False, bkm=False, c=F32, flags=BETA, split=2)["label"] == "gemm_wgrad_splitk"
    assert plan(128, 64, 64, ab=F32, c=F32)["kernel"] == "f32"
    assert plan(128, 64, 64, ab=F32, c=F32)["label"] == "gemm_f32"
    assert plan(0, 64, 64)["kernel"] == "none"


def test_bias_grad_needs_the_wgrad_layout():
    st, msg = error_of(desc(512, 768, 768, akm=True, bkm=False, c=F32, bias_grad=True))
    assert st == -1 and msg == "gemm_impl: bias_grad needs the wgrad layout (both operands row-major in k)"
    st, msg = error_of(wgrad(512, 768, 768, bias_grad=True, force=_lib.FORCE_128))
    assert st == -1 and msg == "gemm_impl: bias_grad fusion needs the 256 kernel (bf16, wgrad layout)"
    assert _lib.gemm_plan(wgrad(64, 64, 512, bias_grad=True))["kernel"] == "w4p"  # bias_grad alone selects the 256 tile


# ---- MXFP8
def test_fp8_selection():
    f = dict(ab=FP8, flags=B_)
    assert plan(512, 1024, 1024, **f) == dict(plan(512, 1024, 1024, **f), kernel="fp8_w4p", label="gemm_fp8_fwd_bias",
                                              tile=256, raster=8)
    assert kernel(256, 256, 256, **f) == "fp8_w4p"
    assert kernel(512, 1024, 128, **f) == "fp8_8w"      # K % 256 != 0
    assert kernel(512, 1024, 384, **f) == "fp8_8w"
    assert kernel(128, 1024, 1024, **f) == "fp8_8w"     # less than a full tile
    assert kernel(512, 128, 1024, **f) == "fp8_8w"
    assert kernel(512, 1024, 1024, bias=4 * PTR + 2, **f) == "fp8_8w"  # bf16 rows the 16-byte stores cannot take
    assert kernel(512, 1024, 1024, ab=FP8, flags=B_, c=F32, bias=4 * PTR + 2) == "fp8_w4p"
    assert plan(512, 1024, 1024, ab=FP8, flags=B_ | Q, c=FP8)["label"] == "gemm_fp8_fwd_bias_qgelu_q8"
    assert plan(512, 1024, 1024, ab=FP8, flags=B_ | G)["label"] == "gemm_fp8_generic"
    assert plan(512, 1024, 1024, ab=FP8, flags=B_ | G)["kernel"] == "fp8_8w"
    assert plan(512, 1024, 1024, ab=FP8, flags=B_ | G, c=F32) == dict(plan(512, 1024, 1024, ab=FP8, flags=B_ | G, c=F32),
                                                                     kernel="fp8_w4p", label="gemm_fp8", specialised=0)
    for flags in (B_, B_ | G, 0):
        st, msg = error_of(desc(512, 1024, 1024, ab=FP8, c=FP8, flags=flags))
        assert st == -1 and msg == "fp8 output: supported epilogue flags are bias + quick_gelu"


# ---- the force codes
def test_force_decode():
    fwd = dict(flags=B_)
    assert kernel(512, 768, 3072, force=_lib.FORCE_128, **fwd) == "bf16_128"
    assert kernel(512, 768, 3072, force=_lib.FORCE_ASM8, **fwd) == "asm8"
    assert kernel(512, 768, 3072, force=_lib.FORCE_PP8, **fwd) == "pp8"
    assert kernel(512, 768, 768, force=_lib.FORCE_W4P, **fwd) == "w4p"
    assert kernel(512, 768, 768, force=_lib.FORCE_W4P_PF, **fwd) == "w4p_pf"
    p = plan(512, 768, 3072, force=_lib.FORCE_PP8_STAGGER + 7, **fwd)
    assert (p["kernel"], p["stagger"]) == ("pp8", 7)
    assert plan(512, 768, 3072, **fwd)["stagger"] == 0
    # the MXFP8 codes mean nothing to bf16 operands (the ping-pong kernel, as any unnamed code), and the other way
    assert kernel(512, 768, 3072, force=_lib.FORCE_FP8_8W, **fwd) == "pp8"
    assert kernel(512, 768, 3072, force=_lib.FORCE_FP8_RULE, **fwd) == "pp8"
    assert kernel(512, 1024, 1024, ab=FP8, force=_lib.FORCE_FP8_8W, **fwd) == "fp8_8w"
    assert kernel(512, 1024, 1024, ab=FP8, force=_lib.FORCE_FP8_RULE, **fwd) == "fp8_w4p"
    assert kernel(512, 1024, 1024, ab=FP8, force=_lib.FORCE_W4P, **fwd) == "fp8_w4p"
    # weight gradients: 4 is the 8-wave baseline of the bitwise tests; 32 has no prefetch form there
    assert _lib.gemm_plan(wgrad(768, 768, 512, force=_lib.FORCE_ASM8))["kernel"] == "asm8"
    assert _lib.gemm_plan(wgrad(768, 768, 512, force=_lib.FORCE_PP8, split=2))["kernel"] == "pp8"
    assert _lib.gemm_plan(wgrad(768, 768, 512, force=_lib.FORCE_W4P_PF))["kernel"] == "w4p"
    # a forced 4-wave kernel where it has no instance leaves the product to the ping-pong kernel
    assert kernel(512, 768, 768, force=_lib.FORCE_W4P_PF, c=F32, **fwd) == "pp8"
    assert kernel(512, 768, 768, force=_lib.FORCE_W4P, c=F32, **fwd) == "w4p"
    assert kernel(512, 768, 768, force=_lib.FORCE_W4P, c=F32, flags=B_ | Q) == "pp8"
    # experiment-only codes in the product build: the ping-pong kernel, as before
    if kernel(512, 768, 768, force=10, **fwd) != "experiment":
        for code in (2, 3, 5, 8, 10, 11, 12, 16, 20, 22, 25):
            assert kernel(512, 768, 768, force=code, **fwd) == "pp8", code
            assert kernel(512, 768, 3072, force=code, **fwd) == "pp8", code
    # 1 is "small tile" for every layout; a negative code is the rule
    assert plan(512, 768, 768, force=-1, **fwd) == plan(512, 768, 768, **fwd)


# ---- environment
def test_raster_env(monkeypatch):
    monkeypatch.delenv("CLIPMI_RASTER", raising=False)
    assert plan(1024, 1024, 768, flags=B_)["raster"] == 0
    assert plan(1024, 1024, 1024, ab=FP8, flags=B_)["raster"] == 8
    # tall weight gradients walk column-major: fc2's M = 768, N = 3072 -> raster == tiles_m
    p = _lib.gemm_plan(wgrad(768, 3072, 512))
    assert (p["tiles_n"], p["ntiles"], p["raster"]) == (12, 36, 3)
    assert _lib.gemm_plan(wgrad(3072, 768, 512))["raster"] == 0
    assert _lib.gemm_plan(wgrad(768, 768, 512))["raster"] == 0
    monkeypatch.setenv("CLIPMI_RASTER", "4")  # read per call
    assert plan(1024, 1024, 768, flags=B_)["raster"] == 4
    assert plan(1024, 1024, 1024, ab=FP8, flags=B_)["raster"] == 4
    assert _lib.gemm_plan(wgrad(768, 3072, 512))["raster"] == 4
    monkeypatch.setenv("CLIPMI_RASTER", "0")
    assert _lib.gemm_plan(wgrad(768, 3072, 512))["raster"] == 0
    assert plan(1024, 1024, 1024, ab=FP8, flags=B_)["raster"] == 0


_CHILD = """
import sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {repo!r})
import test_cpu_gemm_plan as T
from clipmi import _lib
print(T.kernel(512, 768, 3072, flags=1), T.kernel(512, 768, 768, flags=1),
      _lib.gemm_plan(T.wgrad(768, 768, 512))["kernel"], T.kernel(512, 1024, 1024, ab=2, flags=1),
      T.kernel(512, 768, 3072, flags=1, force=_lib.FORCE_W4P))
"""


@pytest.mark.parametrize("env,want", [
    ({}, "w4p pp8 w4p fp8_w4p w4p"),
    ({"CLIPMI_GEMM_VAR": "9"}, "pp8 pp8 w4p fp8_w4p w4p"),      # forward / dgrad layouts only; a force code wins
    ({"CLIPMI_GEMM_VAR": "28"}, "w4p w4p w4p fp8_w4p w4p"),
    ({"CLIPMI_GEMM_WVAR": "4"}, "w4p pp8 asm8 fp8_w4p w4p"),    # the wgrad layout only
    ({"CLIPMI_GEMM_WVAR": "0"}, "w4p pp8 pp8 fp8_w4p w4p"),
    ({"CLIPMI_FP8_VAR": "40"}, "w4p pp8 w4p fp8_8w w4p"),
    ({"CLIPMI_FP8_VAR": "7"}, "w4p pp8 w4p fp8_w4p w4p"),       # only 40 / 41 are accepted
])
def test_cached_env_overrides(env, want):
    """CLIPMI_GEMM_VAR / _WVAR / CLIPMI_FP8_VAR are read once per process: one child process each."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("CLIPMI_GEMM_") and k != "CLIPMI_FP8_VAR"}
    e.update(env)
    e["PYTHONPATH"] = os.pathsep.join([os.path.join(REPO, "vlm-clip_amd"), e.get("PYTHONPATH", "")])
    code = _CHILD.format(tests=os.path.join(REPO, "tests"), repo=REPO)
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == want.split()


# ---- geometry
def test_split_k_rounding_and_tiles():
    # K = 1000, split 3, k-step 32: per = ceil(1000 / 3) = 334 -> 352 (11 steps), splits = ceil(1000 / 352) = 3.
    # The bf16 kernels step 64: 334 -> 384, ceil(1000 / 384) = 3; the fp32 SIMT kernel steps 16: 334 -> 336, 3.
    def per_splits(K, split, step):
        per = -(-K // split)
        per = -(-per // step) * step
        return per, -(-K // per)
    assert per_splits(1000, 3, 32) == (352, 3)
    p = _lib.gemm_plan(wgrad(768, 768, 1000, split=3))
    assert (p["k_per_split"], p["splits"]) == per_splits(1000, 3, 64) == (384, 3)
    p = _lib.gemm_plan(desc(768, 768, 1000, ab=F32, c=F32, flags=BETA, split=3))
    assert (p["k_per_split"], p["splits"]) == per_splits(1000, 3, 16) == (336, 3)
    p = _lib.gemm_plan(wgrad(768, 768, 1000, split=7))   # 143 -> 192: six splits cover K
    assert (p["k_per_split"], p["splits"]) == per_splits(1000, 7, 64) == (192, 6)
    p = _lib.gemm_plan(wgrad(768, 768, 64, split=2))     # one k-step: a single slab, still reduced
    assert (p["k_per_split"], p["splits"], p["reduce"], p["label"]) == (64, 1, 1, "gemm256_wgrad_splitk")
    assert plan(512, 768, 768, flags=B_)["k_per_split"] == 768
    # the scalar reduce when C cannot take 16-byte stores
    assert _lib.gemm_plan(wgrad(768, 768, 512, split=2, ldc=769))["reduce"] == 2
    # tile counts: 256-tile and 128-tile plans, ragged edges
    p = plan(1000, 776, 768, flags=B_)
    assert (p["tile"], p["tiles_n"], p["ntiles"]) == (256, 4, 16)
    p = plan(200, 136, 72, flags=B_)
    assert (p["tile"], p["tiles_n"], p["ntiles"]) == (128, 2, 4)
    p = plan(200, 136, 72, ab=F32, c=F32)
    assert (p["tile"], p["tiles_n"], p["ntiles"]) == (64, 3, 12)
    p = plan(300, 520, 256, ab=FP8, flags=B_)
    assert (p["tile"], p["tiles_n"], p["ntiles"]) == (256, 3, 6)


# ---- labels
def _bench_families():
    tree = ast.parse(open(os.path.join(REPO, "bench.py")).read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", "") in ("FAMILIES", "FAMILIES_FP32"):
            out.update(ast.literal_eval(node.value))
    return out


def _label_descriptors():
    ds = []
    for c in (BF16, F32):
        for flags in (B_, B_ | R_, B_ | Q | P, B_ | Q | DA, B_ | Q, 0, B_ | G, B_ | G | P, Q):
            for (M, N, K) in ((512, 768, 768), (512, 768, 3072), (200, 136, 72)):
                ds.append((desc(M, N, K, flags=flags, c=c), False))
        for flags in (0, DQ, MA, DG, R_):
            for (M, N, K) in ((512, 768, 768), (512, 768, 3072), (200, 136, 72)):
                ds.append((desc(M, N, K, bkm=False, flags=flags, c=c), False))
        ds.append((desc(512, 768, 768, akm=False, bkm=True, c=c), False))
    for (M, N) in ((768, 768), (128, 120)):
        for split in (1, 3):
            ds.append((wgrad(M, N, 512, split=split), False))
            ds.append((wgrad(M, N, 512, split=split, flags=0), False))
    ds.append((desc(512, 768, 768, ab=F32, c=F32), False))
    ds.append((desc(512, 3072, 2304, flags=B_ | Q | DA, c=F32, ldc=9216), True))
    ds.append((desc(512, 3072, 2304, flags=B_ | Q, c=F32, ldc=9216), True))
    ds.append((desc(512, 3072, 2304, bkm=False, flags=MA, c=F32, ldc=9216), True))
    for K in (1024, 128):
        for c in (BF16, F32):
            for flags in (B_, B_ | R_, B_ | Q, 0, B_ | G):
                ds.append((desc(512, 1024, K, ab=FP8, flags=flags, c=c), False))
        ds.append((desc(512, 1024, K, ab=FP8, flags=B_ | Q, c=FP8), False))
    return ds


def test_labels_are_the_benchmarks_families():
    fam = _bench_families()
    gemm_labels = {l for f, ls in fam.items() if f.startswith("gemm") for l in ls}
    assert len(gemm_labels) >= 25
    seen = {_lib.gemm_plan(d, x3)["label"] for d, x3 in _label_descriptors()}
    assert gemm_labels <= seen, sorted(gemm_labels - seen)
    for l in seen - gemm_labels:
        assert l in ("gemm_generic", "gemm_f32", "gemm_wgrad", "gemm_wgrad_splitk") or \
            l.startswith(("gemm_fwd", "gemm_dgrad")), l


# ---- validation: the messages of tests/test_cpu_host.py, from the launch and from the query
def _host_desc(flags, **ptrs):
    d = desc(256, 256, 64, flags=flags, aux=16384, residual=20480, bias=24576, ldc=256, ldr=256, ldaux=256)
    for k, v in ptrs.items():
        setattr(d, k, v)
    return d


@pytest.mark.parametrize("make,msg", [
    (lambda: desc(16, 12, 64, akm=False, bkm=False, bias=None, aux=None, residual=None),
     "gemm_impl: row-major B needs N % 8 == 0"),
    (lambda: _host_desc(DQ, aux=None), "gemm_impl: epilogue flags need aux (ldaux >= N)"),
    (lambda: _host_desc(DG, aux=None), "gemm_impl: epilogue flags need aux (ldaux >= N)"),
    (lambda: _host_desc(MA, aux=None), "gemm_impl: epilogue flags need aux (ldaux >= N)"),
    (lambda: _host_desc(P, aux=None), "gemm_impl: epilogue flags need aux (ldaux >= N)"),
    (lambda: _host_desc(DA | Q, aux=None), "gemm_impl: epilogue flags need aux (ldaux >= N)"),
    (lambda: _host_desc(R_, residual=None), "gemm_impl: residual flag needs residual (ldr >= N)"),
    (lambda: _host_desc(B_, bias=None), "gemm_impl: bias flag needs bias"),
    (lambda: _host_desc(DA), "gemm_impl: store_dact needs an activation flag"),
    (lambda: _host_desc(Q | P | DA), "gemm_impl: store_pre and store_dact both write aux"),
    (lambda: _host_desc(Q | MA | R_), "gemm_impl: mul_aux cannot be combined with residual / beta"),
    (lambda: _host_desc(Q | MA | BETA), "gemm_impl: mul_aux cannot be combined with residual / beta"),
    (lambda: _host_desc(Q | DQ | P), "gemm_impl: aux cannot be both read and written"),
    (lambda: _host_desc(Q | MA | DQ), "gemm_impl: at most one aux-reading flag"),
    (lambda: _host_desc(2048), "gemm_impl: unknown epilogue flag"),
    (lambda: desc(-1, 8, 8), "gemm_impl: bad shape"),
    (lambda: desc(256, 256, 64, split=2), "gemm_impl: split_k needs fp32 C"),
    (lambda: desc(256, 256, 64, A=PTR + 8), "gemm_impl: A/B must be 16-byte aligned"),
    (lambda: desc(256, 256, 64, ab=FP8, akm=False), "gemm_impl: fp8: both operands k-major"),
    (lambda: desc(512, 3072, 2304, c=F32, flags=B_ | Q, force=_lib.FORCE_128),
     "gemm_impl: x3out: needs the 256-tile kernels (M >= 256, N >= 128, K % 64 == 0)"),
])
def test_validation_messages_unchanged(make, msg):
    d = make()
    x3 = "x3out" in msg
    st, got = error_of(d, x3out=x3)
    assert st == -1 and got == msg
    if not x3:
        assert _lib.lib().clipmi_gemm(None, ctypes.byref(d)) == -1
        assert _lib.lib().clipmi_last_error().decode() == msg
