"""One harness for the GPU tests of the encoder engine's modes (tests/test_gpu_first_token.py,
tests/test_gpu_cls_last.py) and for tools/engine_digest.py: seeded weights and inputs at D = 128, H = 2, F = 512,
one forward + backward of the native engine in the mode asked for, and the error metric the tests share (max error
over max(|ref| of the tensor, 5 % of the group's largest); a NaN counts as 1e30)."""
import ctypes
import types

import torch

from clipmi import _lib
from clipmi import kernels as K
from clipmi import towers as T

D, H, F = 128, 2, 512
EPS = 1e-5
SHAPES = {"ln1_w": (D,), "ln1_b": (D,), "qkv_w": (3 * D, D), "qkv_b": (3 * D,), "out_w": (D, D), "out_b": (D,),
          "ln2_w": (D,), "ln2_b": (D,), "fc1_w": (F, D), "fc1_b": (F,), "fc2_w": (D, F), "fc2_b": (D,)}
MODES = {"fp32": (torch.float32, False), "bf16": (torch.bfloat16, False), "bf16_resid32": (torch.bfloat16, True)}


def make_weights(seed, dtype, L):
    """[L] dicts of weights in the engine's dtype (the engines and the fp64 references read these values)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(L):
        w = {}
        for n, shp in SHAPES.items():
            t = torch.randn(shp, generator=g)
            if n in ("ln1_w", "ln2_w"):
                t = 1.0 + 0.1 * t
            elif n.endswith("_w"):
                t = t / shp[1] ** 0.5
            else:
                t = 0.1 * t
            w[n] = t.to(dtype).cuda().contiguous()
        out.append(w)
    return out


def make_mask(kind, B, N):
    if kind == "null":
        return None
    m = torch.ones(B, N, dtype=torch.int64)
    if kind == "key0":  # token 0's own key padded for every third caption (B = 1: for the only one)
        m[::3, 0] = 0
    return m.cuda()


def inputs(B, N, seed=0):
    g = torch.Generator().manual_seed(1000 * B + N + seed)
    return torch.randn(B, N, D, generator=g).cuda(), torch.randn(B, D, generator=g).cuda()


def run_engine(mode, dtype, r32, B, N, L, weights, x0, dy0, causal=False, mask=None, grad_fill=None, chunks=None,
               row0=False):
    """One forward + backward of the native engine; mode: "full", "first_token" (B compact rows, token 0 alone) or
    "cls_last" (the last layer's out-projection and MLP on the B CLS rows, x_out compact).  x0 [B, N, D] fp32,
    dy0 [B, D]: the upstream gradient at row 0 of every sequence (zero elsewhere).  grad_fill: the gradient slots'
    initial content (default zeros); chunks: the backward as clipmi_encoder_bwd_layers calls over these (hi, lo)
    ranges instead of one call.  Returns (output at row 0, dx, {layer.name: gradient}), fp32 on the device; dx is
    [B, N, D] ([B, D] in the first_token mode, which has no other row), or its row 0 with row0."""
    first, cls = mode == "first_token", mode == "cls_last"
    assert first or cls or mode == "full", mode
    dev = x0.device
    xdt = torch.float32 if r32 else dtype
    R = B if first else B * N
    tcfg = types.SimpleNamespace(hidden_size=D, intermediate_size=F, num_attention_heads=H, num_hidden_layers=L,
                                 layer_norm_eps=EPS)
    enc = T.Encoder(None, "encoder", tcfg, causal=causal)
    buf, acts = enc.alloc(B, N, dtype, dev, True, resid32=r32, first_token=first)
    x_in = (x0[:, 0] if first else x0.reshape(R, D)).to(xdt).contiguous()
    acts[0].x_in = x_in.data_ptr()
    wt, gt = (T.LayerW * L)(), (T.LayerG * L)()
    grads = []
    for l in range(L):
        gl = {}
        for n, shp in SHAPES.items():
            setattr(wt[l], n, weights[l][n].data_ptr())
            gl[n] = (torch.zeros(shp, dtype=torch.float32, device=dev) if grad_fill is None
                     else grad_fill[f"{l}.{n}"].clone())
            setattr(gt[l], n, gl[n].data_ptr())
        grads.append(gl)
    x_out = torch.empty(B if cls else R, D, dtype=xdt, device=dev)
    d = T.EncoderDesc()
    d.dtype, d.B, d.N, d.D, d.F, d.H, d.L, d.eps, d.causal = T.dcode(dtype), B, N, D, F, H, L, EPS, int(causal)
    d.attention_mask = T.P_(mask)
    d.layers, d.grads, d.act, d.x_out = wt, gt, acts, x_out.data_ptr()
    d.resid_f32, d.first_token, d.cls_last = int(r32), int(first), int(cls)
    s = K.stream()
    lib = _lib.lib()
    _lib.check(lib.clipmi_encoder_fwd(s, ctypes.byref(d)), "clipmi_encoder_fwd")
    ws = torch.empty(max(int(lib.clipmi_encoder_bwd_ws(ctypes.byref(d))), 16), dtype=torch.uint8, device=dev)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if first:
        dx = dy0.to(dtype).clone()  # the backward overwrites dx in place
    elif cls:  # dL/dx_out in the head of the [R, D] buffer; the rest is overwritten (NaN until then)
        dx = torch.full((R, D), float("nan"), dtype=dtype, device=dev)
        dx[:B] = dy0.to(dtype)
    else:
        dx = torch.zeros(B, N, D, dtype=dtype, device=dev)
        dx[:, 0] = dy0.to(dtype)
        dx = dx.reshape(R, D)
    if chunks is None:
        _lib.check(lib.clipmi_encoder_bwd(s, ctypes.byref(d), dx.data_ptr()), "clipmi_encoder_bwd")
    else:
        for hi, lo in chunks:
            _lib.check(lib.clipmi_encoder_bwd_layers(s, ctypes.byref(d), dx.data_ptr(), hi, lo),
                       "clipmi_encoder_bwd_layers")
    torch.cuda.synchronize()
    out = x_out.float() if first or cls else x_out.view(B, N, D)[:, 0].float()
    dx = dx.float() if first else dx.view(B, N, D)[:, 0].float() if row0 else dx.view(B, N, D).float()
    return out, dx, {f"{l}.{n}": g for l in range(L) for n, g in grads[l].items()}


def rel_err(got, ref, group_max):
    scale = max(float(ref.abs().max()), 0.05 * group_max, 1e-6)
    return float((got.double() - ref).abs().nan_to_num(1e30).max()) / scale


def errors(res, ref):
    out, dx, grads = res
    rout, rdx, rgrads = ref
    gmax = max(float(g.abs().max()) for g in rgrads.values())
    worst = max((rel_err(grads[n], rgrads[n], gmax), n) for n in rgrads)
    return rel_err(out, rout, float(rout.abs().max())), rel_err(dx, rdx, float(rdx.abs().max())), worst
