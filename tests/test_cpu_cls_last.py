"""Host-side checks of the encoder's cls_last mode and the single-query attention entry points (no GPU):
descriptor validation, the ABI version, clipmi_encoder_act_bytes (unchanged by the mode) and argument checks that
must fail before any HIP call."""
import ctypes

import pytest

from clipmi import _lib
from clipmi import towers as T

B, N, D, F, H, L = 5, 50, 128, 512, 2, 2
c_vp, c_i64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int

_lib.declare("clipmi_attention_cls_fwd", [c_vp, c_int, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_int, c_int, c_int, c_int])
_lib.declare("clipmi_attention_cls_bwd", [c_vp, c_int, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp,
                                          c_i64, c_vp, c_i64, c_int, c_int, c_int, c_int])


def desc(dtype=_lib.F32, causal=0, first_token=0, gemm_x3=0, mask=None, cls_last=1, n=N):
    d = T.EncoderDesc()
    d.dtype, d.B, d.N, d.D, d.F, d.H, d.L, d.eps, d.causal = dtype, B, n, D, F, H, L, 1e-5, causal
    d.first_token, d.gemm_x3, d.cls_last = first_token, gemm_x3, cls_last
    d.attention_mask = mask
    d.keep = ((T.LayerW * L)(), (T.LayerAct * L)())  # validate() wants the tables; nothing is launched
    d.layers, d.act = d.keep
    return d


def test_version_moved():
    assert _lib.lib().clipmi_version() >= 5  # 4: before clipmi_encoder_desc.cls_last / clipmi_attention_cls_*


@pytest.mark.parametrize("kw,word", [({"causal": 1}, "causal"), ({"causal": 1, "first_token": 1}, "first_token"),
                                     ({"dtype": _lib.FP8}, "CLIPMI_FP8"), ({"gemm_x3": 1}, "gemm_x3"),
                                     ({"mask": 4096}, "attention_mask")])
def test_validate_rejects_cls_last_combinations(kw, word):
    lib = _lib.lib()
    d = desc(**kw)
    for status in (lib.clipmi_encoder_fwd(None, ctypes.byref(d)), lib.clipmi_encoder_bwd(None, ctypes.byref(d), None)):
        assert status == -1  # CLIPMI_ERR_INVALID
        msg = lib.clipmi_last_error().decode()
        assert "cls_last" in msg and word in msg, msg
    with pytest.raises(ValueError):
        _lib.check(lib.clipmi_encoder_fwd(None, ctypes.byref(d)), "clipmi_encoder_fwd")


def test_validate_rejects_long_sequences():
    d = desc(n=4097)
    assert _lib.lib().clipmi_encoder_fwd(None, ctypes.byref(d)) == -1
    assert "cls_last" in _lib.lib().clipmi_last_error().decode()


def act_bytes(d):
    out = (ctypes.c_int64 * len(T.A_FIELDS))()
    _lib.check(_lib.lib().clipmi_encoder_act_bytes(ctypes.byref(d), out), "clipmi_encoder_act_bytes")
    return [int(v) for v in out]


@pytest.mark.parametrize("dtype,resid32", [(_lib.F32, 0), (_lib.BF16, 0), (_lib.BF16, 1)])
def test_act_bytes_unchanged_by_cls_last(dtype, resid32):
    a, b = desc(dtype=dtype, cls_last=0), desc(dtype=dtype, cls_last=1)
    a.resid_f32 = b.resid_f32 = resid32
    assert act_bytes(a) == act_bytes(b)


def test_bwd_ws_is_at_least_the_full_modes():
    lib = _lib.lib()
    for dtype in (_lib.F32, _lib.BF16):
        full = int(lib.clipmi_encoder_bwd_ws(ctypes.byref(desc(dtype=dtype, cls_last=0))))
        cls = int(lib.clipmi_encoder_bwd_ws(ctypes.byref(desc(dtype=dtype, cls_last=1))))
        assert cls >= full


# clipmi_encoder_bwd_ws per (dtype, mode, B, N), recorded from the commit before the engine's layer bodies and plan()'s
# weight-gradient shape tables were merged, on a machine without a GPU.  The bf16 split choice reads the device's CU
# count, which falls back to 256 without a device: an MI355X's own count, so the table holds on both.
# D, F, H = 128, 512, 2; 768, 3072, 12 at (1024, 197).
BWD_WS = {
    ("F32", "full", 5, 50): 866816,
    ("F32", "full", 33, 50): 6510080,
    ("F32", "full", 1100, 2): 8678400,
    ("F32", "full", 1024, 197): 3750515712,
    ("F32", "first_token", 5, 50): 20480,
    ("F32", "first_token", 33, 50): 117248,
    ("F32", "first_token", 1100, 2): 4340224,
    ("F32", "first_token", 1024, 197): 35457024,
    ("F32", "cls_last", 5, 50): 866816,
    ("F32", "cls_last", 33, 50): 6510080,
    ("F32", "cls_last", 1100, 2): 8678400,
    ("F32", "cls_last", 1024, 197): 3750515712,
    ("BF16", "full", 5, 50): 482816,
    ("BF16", "full", 33, 50): 3183104,
    ("BF16", "full", 1100, 2): 4242432,
    ("BF16", "full", 1024, 197): 2007146496,
    ("BF16", "first_token", 5, 50): 12800,
    ("BF16", "first_token", 33, 50): 66560,
    ("BF16", "first_token", 1100, 2): 2122240,
    ("BF16", "first_token", 1024, 197): 11845632,
    ("BF16", "cls_last", 5, 50): 482816,
    ("BF16", "cls_last", 33, 50): 3183104,
    ("BF16", "cls_last", 1100, 2): 4242432,
    ("BF16", "cls_last", 1024, 197): 2007146496,
}


@pytest.mark.parametrize("key", list(BWD_WS), ids=lambda k: "-".join(map(str, k)))
def test_bwd_ws_matches_recorded_table(key):
    dt, mode, b, n = key
    d = T.EncoderDesc()
    d.dtype, d.B, d.N, d.L, d.eps = getattr(_lib, dt), b, n, L, 1e-5
    d.D, d.F, d.H = (768, 3072, 12) if (b, n) == (1024, 197) else (D, F, H)
    d.causal = d.first_token = int(mode == "first_token")
    d.cls_last = int(mode == "cls_last")
    assert int(_lib.lib().clipmi_encoder_bwd_ws(ctypes.byref(d))) == BWD_WS[key]


P = 4096  # a non-null, 16-byte aligned address; no call below may reach the device


def fwd(dtype=_lib.BF16, q=P, ldq=D, kv=P, o=P, ldo=D, lse=P, b=B, h=H, n=N, d=D):
    return _lib.lib().clipmi_attention_cls_fwd(None, dtype, q, ldq, kv, o, ldo, lse, b, h, n, d)


def bwd(dtype=_lib.BF16, q=P, kv=P, o=P, lse=P, dout=P, dkv=P, dq=P, dkv0=None, ld0=0, b=B, h=H, n=N, d=D, ld=D):
    return _lib.lib().clipmi_attention_cls_bwd(None, dtype, q, ld, kv, o, ld, lse, dout, ld, dkv, dq, ld, dkv0, ld0, b,
                                               h, n, d)


@pytest.mark.parametrize("kw", [{"q": None}, {"kv": None}, {"o": None}, {"lse": None}, {"d": D + 64}, {"d": D - 8},
                                {"n": 0}, {"n": 4097}, {"dtype": _lib.FP8}, {"b": -1}, {"ldq": D - 8}, {"ldq": D + 4},
                                {"q": P + 8}, {"o": P + 2}])
def test_cls_fwd_rejects_bad_arguments(kw):
    assert fwd(**kw) == -1, kw
    assert "attention_cls_fwd" in _lib.lib().clipmi_last_error().decode()


@pytest.mark.parametrize("kw", [{"q": None}, {"kv": None}, {"o": None}, {"lse": None}, {"dout": None}, {"dkv": None},
                                {"dq": None}, {"d": D + 64}, {"n": 0}, {"n": 4097}, {"dtype": _lib.FP8}, {"b": -1},
                                {"ld": D - 8}, {"dkv": P + 8}, {"dkv0": P, "ld0": D}, {"dkv0": P + 4, "ld0": 2 * D}])
def test_cls_bwd_rejects_bad_arguments(kw):
    assert bwd(**kw) == -1, kw
    assert "attention_cls_bwd" in _lib.lib().clipmi_last_error().decode()


def test_cls_empty_batch_is_a_no_op():
    assert fwd(b=0) == 0
    assert bwd(b=0) == 0
