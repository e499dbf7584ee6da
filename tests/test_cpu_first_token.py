"""Host-side checks of the encoder's first-token mode (no GPU): descriptor validation, the ABI version and
clipmi_encoder_act_bytes against the sizes Encoder.alloc computed itself before the engine exported them."""
import ctypes

import pytest

from clipmi import _lib
from clipmi import towers as T

B, N, D, F, H, L = 5, 77, 128, 512, 2, 2


def desc(dtype=_lib.F32, causal=1, first_token=1, gemm_x3=0, resid_f32=0):
    d = T.EncoderDesc()
    d.dtype, d.B, d.N, d.D, d.F, d.H, d.L, d.eps, d.causal = dtype, B, N, D, F, H, L, 1e-5, causal
    d.first_token, d.gemm_x3, d.resid_f32 = first_token, gemm_x3, resid_f32
    d.keep = ((T.LayerW * L)(), (T.LayerAct * L)())  # validate() wants the tables; nothing is launched
    d.layers, d.act = d.keep
    return d


@pytest.mark.parametrize("kw,word", [({"causal": 0}, "causal"), ({"dtype": _lib.FP8}, "fp8"),
                                     ({"gemm_x3": 1}, "gemm_x3")])
def test_validate_rejects_first_token_combinations(kw, word):
    lib = _lib.lib()
    d = desc(**kw)
    for status in (lib.clipmi_encoder_fwd(None, ctypes.byref(d)), lib.clipmi_encoder_bwd(None, ctypes.byref(d), None)):
        assert status == -1  # CLIPMI_ERR_INVALID
        msg = lib.clipmi_last_error().decode()
        assert "first_token" in msg and word in msg, msg
    with pytest.raises(ValueError):
        _lib.check(lib.clipmi_encoder_fwd(None, ctypes.byref(d)), "clipmi_encoder_fwd")


def test_version_moved():
    assert _lib.lib().clipmi_version() >= 2  # 1: before clipmi_encoder_desc.first_token / clipmi_encoder_act_bytes


def act_bytes(d):
    out = (ctypes.c_int64 * len(T.A_FIELDS))()
    _lib.check(_lib.lib().clipmi_encoder_act_bytes(ctypes.byref(d), out), "clipmi_encoder_act_bytes")
    return dict(zip(T.A_FIELDS, (int(v) for v in out)))


@pytest.mark.parametrize("dtype,resid32,x3", [(_lib.F32, 0, 0), (_lib.BF16, 0, 0), (_lib.BF16, 1, 0), (_lib.F32, 0, 1),
                                              (_lib.FP8, 0, 0)])
def test_act_bytes_equals_allocs_former_arithmetic(dtype, resid32, x3):
    R = B * N
    es = 4 if dtype == _lib.F32 else 2  # the fp8 encoder's activations are bf16
    xs = 4 if resid32 else es
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    ln_b = R * 3 * D * 2 if x3 else R * D * es
    want = {"x_in": R * D * xs, "ln1": ln_b, "qkv": R * 3 * D * es,
            "o": al(R * D * 4) + R * 3 * D * 2 if x3 else R * D * es, "h": R * D * xs, "ln2": ln_b,
            "act": R * 3 * F * 2 if x3 else R * F * es, "mean1": R * 4, "rstd1": R * 4, "lse": B * H * N * 4,
            "mean2": R * 4, "rstd2": R * 4, "pre": R * F * es}
    assert act_bytes(desc(dtype=dtype, first_token=0, gemm_x3=x3, resid_f32=resid32)) == want


@pytest.mark.parametrize("dtype,resid32", [(_lib.F32, 0), (_lib.BF16, 0), (_lib.BF16, 1)])
def test_act_bytes_first_token(dtype, resid32):
    es = 4 if dtype == _lib.F32 else 2
    xs = 4 if resid32 else es
    want = {"x_in": B * D * xs, "ln1": B * D * es, "qkv": B * D * es, "o": 0, "h": B * D * xs, "ln2": B * D * es,
            "act": B * F * es, "mean1": B * 4, "rstd1": B * 4, "lse": 0, "mean2": B * 4, "rstd2": B * 4,
            "pre": B * F * es}
    assert act_bytes(desc(dtype=dtype, first_token=1, resid_f32=resid32)) == want
