"""Helpers and case lists of the structured-input kernel tests (tests/test_gpu_structured.py on the GPU,
tests/test_cpu_kernel_checks.py for their preconditions on the CPU).

"Structured" inputs make the expected result exact or nearly so, so the comparison needs no tolerance wide enough
to hide a defect: integer GEMM operands (every product and sum exact in fp32), one-hot attention (each query's
softmax is a single key, so O is a row of V and a one-key mask leak is an O(1) error) and uniform attention
(q = 0: lse = log(count)).  Every output is allocated inside a guard band (guarded) that a stray store corrupts.

Nothing here imports the library: the case lists are plain data, so the CPU file can check every case's
precondition (the fp64 softmax leak, the exactness bound) without a GPU."""
import torch

# epilogue flags of include/clipmi.h (plain numbers: this module does not load the library)
EPI_BIAS, EPI_QGELU, EPI_RESID, EPI_BETA, EPI_STORE_PRE, EPI_MUL_AUX = 1, 2, 8, 64, 128, 512
# kernel overrides (clipmi/_lib.py FORCE_*; 11 is an experiments-build schedule, the ping-pong kernel otherwise)
FORCE_RULE, FORCE_128, FORCE_ASM8, FORCE_PP8, FORCE_W4P, FORCE_W4P_PF = 0, 1, 4, 9, 28, 32

GUARD_BYTES = 4096
GUARD_PATTERN = 0xFF  # 0xFFFF / 0xFFFFFFFF are NaNs in bf16 / fp32: an output element nobody stored fails its compare


# ------------------------------------------------------------------------------------------------ guard bands
def guarded(rows, cols, dtype, ld=None, offset_elems=0, device="cuda"):
    """A [rows, cols] view with row stride ld >= cols inside a flat byte buffer filled with GUARD_PATTERN: at least
    4 KiB before and after it, the ld - cols pad columns of every row and the offset_elems shift from the 4 KiB
    boundary are guard bytes.  Returns (view, check); check() compares every guard byte bitwise (uint8) and raises
    AssertionError naming the first corrupted element as (row, column) relative to the view."""
    ld = cols if ld is None else int(ld)
    assert ld >= cols and rows >= 1 and cols >= 1 and offset_elems >= 0
    es = torch.empty(0, dtype=dtype).element_size()
    start = GUARD_BYTES + offset_elems * es
    span = ((rows - 1) * ld + cols) * es
    total = (start + span + GUARD_BYTES + 15) // 16 * 16 + 16
    buf = torch.full((total,), GUARD_PATTERN, dtype=torch.uint8, device=device)
    view = torch.as_strided(buf.view(dtype), (rows, cols), (ld, 1), start // es)
    guard = torch.ones(total, dtype=torch.bool, device=device)
    torch.as_strided(guard, (rows, cols * es), (ld * es, 1), start).fill_(False)

    def check():
        bad = (buf != GUARD_PATTERN) & guard
        if bool(bad.any()):
            first = int(torch.nonzero(bad)[0, 0])
            elem = (first - start) // es  # floor: elements before the view get negative rows
            raise AssertionError(f"guard band corrupted: byte {first - start} relative to the view, "
                                 f"(row, column) = ({elem // ld}, {elem % ld}) of a [{rows}, {cols}] view with ld {ld}")

    return view, check


def guarded1d(n, dtype, offset_elems=0, device="cuda"):
    """The 1-D form (lse, mean / rstd, dw / db, bias gradients): an [n] view and its check."""
    view, check = guarded(1, n, dtype, None, offset_elems, device)
    return view[0], check


def integer_tensor(shape, lo, hi, dtype, seed, device="cpu"):
    """Uniform integers in [lo, hi] (exact in bf16 for |x| <= 256) as dtype; the values depend on the seed alone."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).to(dtype).to(device)


def ulp(ref, dtype):
    """The spacing of dtype's values at |ref| (fp64 tensor), at least the spacing at the smallest normal."""
    bits = {torch.bfloat16: 7, torch.float32: 23}[dtype]
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - bits)


# ------------------------------------------------------------------------------------------------ GEMM cases
class GemmCase:
    """One integer-operand GEMM: ab in {"bf16", "f32", "x3"} (x3: fp32 operands with split3=True), c the output
    dtype, small the forced kernel variant, ldc / ldr / ldaux the pads added to N, pad_ab to lda / ldb, c_off the
    shift of C (elements) from a 16-byte boundary, bias in {None, "bf16", "f32"}; cls names the epilogue's
    alignment class the case lands in (csrc/gemm.hip: vec8 / vec / scalar)."""

    def __init__(self, M, N, K, akm, bkm, ab="bf16", c="f32", small=0, flags=0, bias=None, alpha=1.0, ldc=0, ldr=0,
                 ldaux=0, pad_ab=0, c_off=0, split=1, bias_grad=False):
        self.M, self.N, self.K, self.akm, self.bkm = M, N, K, akm, bkm
        self.ab, self.c, self.small, self.flags, self.bias, self.alpha = ab, c, small, flags, bias, alpha
        self.ldc, self.ldr, self.ldaux, self.pad_ab, self.c_off = ldc, ldr, ldaux, pad_ab, c_off
        self.split, self.bias_grad = split, bias_grad

    @property
    def cls(self):
        N = self.N
        lds = [N + self.ldc]
        if self.flags & EPI_RESID:
            lds.append(N + self.ldr)
        if self.flags & (EPI_MUL_AUX | EPI_STORE_PRE):
            lds.append(N + self.ldaux)
        if self.c_off % (4 if self.c == "f32" else 8):
            return "scalar"
        if self.c == "bf16" and N % 8 == 0 and all(x % 8 == 0 for x in lds):
            return "vec8"
        if all(x % 4 == 0 for x in lds):
            return "vec" if N % 4 == 0 else "vec+ragged"
        return "scalar"

    def valid(self):
        """The layout rules of test_gemm_layouts (bf16 operands, and the split images of x3)."""
        if self.ab == "f32":
            return True
        if not self.akm and (self.M % 8 or self.M < 8):
            return False
        if (self.akm or self.bkm) and self.K % 8:
            return False
        if not self.bkm and self.N % 8:
            return False
        return True

    def bound(self):
        """max |value| the epilogue can hold in fp32: operands in [-4, 4], so |acc| <= 16 K; then alpha, the
        integer bias / residual / old C in [-4, 4] and the aux factor in [-4, 4]."""
        v = 16.0 * self.K * abs(self.alpha)
        if self.flags & EPI_BIAS:
            v += 4
        if self.flags & EPI_MUL_AUX:
            v *= 4
        if self.flags & EPI_RESID:
            v += 4
        if self.flags & EPI_BETA:
            v += 4
        return v

    def id(self):
        lay = ("k" if self.akm else "m") + ("k" if self.bkm else "n")
        s = f"{self.M}x{self.N}x{self.K}-{lay}-{self.ab}-c{self.c}-v{self.small}-f{self.flags}"
        if self.bias:
            s += f"-b{self.bias}"
        if self.alpha != 1.0:
            s += f"-a{self.alpha}"
        if self.ldc or self.ldr or self.ldaux:
            s += f"-ld{self.ldc}.{self.ldr}.{self.ldaux}"
        if self.pad_ab:
            s += f"-ab{self.pad_ab}"
        if self.c_off:
            s += f"-off{self.c_off}"
        if self.split != 1 or self.bias_grad:
            s += f"-s{self.split}" + ("-bg" if self.bias_grad else "")
        return s + "-" + self.cls


GEMM_SHAPES = [(256, 256, 128), (200, 136, 72), (77, 63, 768), (264, 130, 64), (520, 388, 192), (300, 1, 64),
               (1, 64, 64), (768, 256, 4160)]
LAYOUTS = [(True, True), (True, False), (False, True), (False, False)]
# the epilogues whose result stays exact: (flags, bias dtype, alpha)
EXACT_EPILOGUES = [(EPI_BIAS, "bf16", 1.0), (EPI_BIAS, "f32", 1.0), (EPI_BIAS | EPI_RESID, "f32", 1.0),
                   (EPI_BETA, None, 1.0), (EPI_MUL_AUX, None, 1.0), (0, None, 0.5),
                   (EPI_BIAS | EPI_QGELU | EPI_STORE_PRE, "f32", 1.0)]


def _takes_256(M, N, K):
    return M >= 256 and N >= 128 and K % 64 == 0


def gemm_cases():
    cases = []
    # 1. Every shape x layout x variant, contiguous.  Classes: fp32 C with N % 4 == 0 is "vec" (epilogue256 on the
    #    256-tile kernels: 256x256x128, 520x388x192, 768x256x4160), bf16 C with N % 8 == 0 is "vec8", N = 63 / 1 are
    #    "scalar" (odd ldc) and N = 130 is "scalar" too (ldc % 4 == 2).  0 production, 1 the 128 tile, 4 single-group
    #    256, 11 half-tile pipeline; 9 / 28 / 32 (8-wave ping-pong, persistent 4-wave) with a k-major A where the
    #    256-tile kernels take the shape; 28 on the weight-gradient layout.  The output dtype alternates.
    i = 0
    for (M, N, K) in GEMM_SHAPES + [(264, 136, 192)]:  # the last: ragged, every layout, the 256-tile kernels
        for (akm, bkm) in LAYOUTS:
            variants = [FORCE_RULE, FORCE_128, FORCE_ASM8, 11]
            if akm and _takes_256(M, N, K):
                variants += [FORCE_PP8, FORCE_W4P, FORCE_W4P_PF]
            if not akm and not bkm:
                variants += [FORCE_W4P]
            for v in variants:
                cases.append(GemmCase(M, N, K, akm, bkm, c=("f32", "bf16")[i % 2], small=v))
                i += 1
    # 2. fp32 operands on gemm_f32_kernel (any shape, two layouts per shape) and the split-operand product, whose
    #    lo images of integers are zero.  fp32 C: "vec" where N % 4 == 0, else "scalar".
    for j, (M, N, K) in enumerate(GEMM_SHAPES):
        for (akm, bkm) in (LAYOUTS[j % 2], LAYOUTS[3 - j % 2]):
            cases.append(GemmCase(M, N, K, akm, bkm, ab="f32"))
        for (akm, bkm) in (LAYOUTS[0], LAYOUTS[1 + j % 3]):
            cases.append(GemmCase(M, N, K, akm, bkm, ab="x3"))
    # 3. Every exact epilogue in every alignment class; ldc, ldr and ldaux all differ.
    v256 = [FORCE_RULE, FORCE_PP8, FORCE_W4P, FORCE_W4P_PF, 11, FORCE_ASM8, FORCE_RULE]
    for e, (flags, bias, alpha) in enumerate(EXACT_EPILOGUES):
        kw = dict(flags=flags, bias=bias, alpha=alpha)
        # vec8: bf16 C, N % 8 == 0, pads of 8 / 16 / 24 -- the 128-tile kernel and a 256-tile variant
        cases.append(GemmCase(200, 136, 72, True, True, c="bf16", small=e % 2, ldc=8, ldr=16, ldaux=24, **kw))
        cases.append(GemmCase(256, 256, 128, True, e % 2 == 0, c="bf16", small=v256[e], ldc=8, ldr=16, ldaux=24, **kw))
        # vec (not vec8): N % 4 == 0, N % 8 != 0, pads of 4 / 8 / 16 -- epilogue256 on the 256-tile kernel
        cases.append(GemmCase(520, 388, 192, True, True, c="bf16", small=v256[e], ldc=4, ldr=8, ldaux=16, **kw))
        cases.append(GemmCase(520, 388, 192, True, True, c="f32", small=v256[(e + 3) % 7], ldc=4, ldr=8, ldaux=16, **kw))
        # vec+ragged: N % 4 == 2 with aligned leading dimensions -- epilogue4, vector stores but for the last nv = 2
        cases.append(GemmCase(264, 130, 64, True, True, c=("bf16", "f32")[e % 2], small=v256[e], ldc=2, ldr=6,
                              ldaux=10, **kw))
        # scalar: odd leading dimensions (N + 1, N + 3, N + 5) on the 256-tile and the 128-tile kernels, odd N
        cases.append(GemmCase(520, 388, 192, True, True, c="bf16", small=v256[e], ldc=1, ldr=3, ldaux=5, **kw))
        cases.append(GemmCase(77, 63, 768, True, True, c=("f32", "bf16")[e % 2], small=e % 2, ldc=1, ldr=3, ldaux=5,
                              **kw))
        # scalar: C one element off a 16-byte boundary, every leading dimension a multiple of 8
        cases.append(GemmCase(264, 136, 64, True, True, c=("bf16", "f32")[e % 2], small=v256[e], ldc=8, ldr=16,
                              ldaux=24, c_off=1, **kw))
    for (flags, bias, alpha) in EXACT_EPILOGUES[:4]:  # N = 1: one ragged column per row
        cases.append(GemmCase(300, 1, 64, True, True, c="bf16", flags=flags, bias=bias, alpha=alpha, ldc=1, ldr=3,
                              ldaux=5))
    # 4. lda / ldb = the row length + 8, every layout (contiguous C: "vec8" / "vec")
    for j, (akm, bkm) in enumerate(LAYOUTS):
        for (M, N, K) in ((256, 256, 128), (200, 136, 72)):
            cases.append(GemmCase(M, N, K, akm, bkm, c=("bf16", "f32")[j % 2], small=(FORCE_RULE, 11, FORCE_ASM8, FORCE_W4P)[j], pad_ab=8))
            cases.append(GemmCase(M, N, K, akm, bkm, ab="f32", pad_ab=8))
    # 5. split-K on the weight-gradient layout with beta (fp32 C): splits 1 / 3 / 8, the 8-wave (4) and persistent
    #    4-wave (28) kernels, a ragged 264x136 output; "vec" (deferred vector reduce) and "scalar" (ldc = N + 1: the
    #    scalar reduce kernel); the fused bias gradient where the 256-tile kernel takes it
    for (M, N, K) in ((256, 256, 128), (264, 136, 200), (768, 256, 4160)):
        for split in (1, 3, 8):
            for v in (FORCE_ASM8, FORCE_W4P):
                cases.append(GemmCase(M, N, K, False, False, small=v, flags=EPI_BETA, split=split,
                                      ldc=(0, 1, 4)[(split + v) % 3]))
            cases.append(GemmCase(M, N, K, False, False, small=(FORCE_ASM8, FORCE_W4P, FORCE_RULE)[split % 3], flags=EPI_BETA, split=split,
                                  bias_grad=True))
        cases.append(GemmCase(M, N, K, False, False, ab="f32", flags=EPI_BETA, split=3))
        cases.append(GemmCase(M, N, K, False, False, ab="x3", flags=EPI_BETA, split=3))
    cases = [c for c in cases if c.valid()]
    ids = [c.id() for c in cases]
    assert len(set(ids)) == len(ids), "duplicate GEMM case"
    return cases


# ------------------------------------------------------------------------------------------------ attention
ATTN_NS = [1, 16, 17, 33, 64, 65, 77, 128, 129, 197, 224, 225, 256, 257, 288, 289, 320, 512, 576, 577, 1024, 4096]
ATTN_MASKS = ["none", "causal", "pad", "causal+pad"]
ATTN_ENTRIES = ["bf16", "bf16_fa", "f32", "x3", "mxfp8"]
ATTN_C, ATTN_C_DECOY = 16, 32
LEAK_MAX = 2.0 ** -40


def attn_entries(N):
    """The entry points run at N.  Above N = 288 the bf16 forward is the flash kernel whatever CLIPMI_ATTN_FA says,
    and the bf16x3 entry points hand over to the exact-f32 kernels: "bf16_fa" and "x3" would repeat "bf16" and
    "f32" there, so they stop at 288 -- but for "x3" at 289, the hand-over itself."""
    if N <= 288:
        return list(ATTN_ENTRIES)
    return ["bf16", "f32", "mxfp8"] + (["x3"] if N == 289 else [])


def attn_dims(N, mask):
    """(B, H): 6 (batch, head) items up to N = 577 and one above; a padded mask takes five batch items, one per
    length of attn_lens."""
    H = 2 if N <= 577 else 1
    if "pad" in mask:
        return 5, H
    return (3, 2) if N <= 577 else (1, 1)


def attn_lens(N, mask):
    """Key-padding lengths {1, N - 1, N, a multiple of 16, that multiple + 1} (clipped into [1, N]), or None."""
    if "pad" not in mask:
        return None
    m16 = 16 * max(1, (N // 2) // 16)
    return [min(max(1, x), N) for x in (1, N - 1, N, m16, m16 + 1)]


def attn_families(N, mask):
    """The pi families of a (N, mask): the four maps, and the decoys of a causal or padded mask."""
    fam = ["ident", "const0", "last", "random"]
    if "causal" in mask and N >= 2:
        fam.append("ident+decoy_next")
    if "pad" in mask and N >= 2:
        fam.append("last+decoy_len")
    return fam


def attn_allowed_count(B, N, lens, causal):
    """[B, N] int64: the number of keys query i of batch item b may attend."""
    cnt = torch.full((B, N), N, dtype=torch.int64)
    if causal:
        cnt = torch.arange(1, N + 1).expand(B, N).clone()
    if lens is not None:
        cnt = torch.minimum(cnt, torch.tensor(lens)[:, None])
    return cnt


def attn_pi(family, B, N, lens, causal, seed):
    """(pi, decoy, c): int64 [B, N] maps (decoy -1: none) of a family; every pi(i) is allowed under the mask."""
    cnt = attn_allowed_count(B, N, lens, causal)  # allowed keys of query i: [0, cnt)
    i = torch.arange(N).expand(B, N)
    decoy = None
    base = family.split("+")[0]
    if base == "ident":
        pi = torch.minimum(i, cnt - 1)
    elif base == "const0":
        pi = torch.zeros(B, N, dtype=torch.int64)
    elif base == "last":
        pi = cnt - 1
    else:
        g = torch.Generator().manual_seed(seed)
        pi = (torch.rand(B, N, generator=g, dtype=torch.float64) * cnt).long().clamp_max(N - 1)
        pi = torch.minimum(pi, cnt - 1)
    if family.endswith("decoy_next"):  # the first key the causal mask hides
        decoy = torch.where(i + 1 < N, i + 1, torch.full_like(i, -1))
    elif family.endswith("decoy_len"):  # the first pad key
        L = torch.tensor(lens)[:, None].expand(B, N)
        decoy = torch.where(L < N, L, torch.full_like(L, -1))
    if decoy is not None:
        # only next to the selected key: consecutive codes are orthogonal (onehot_attention_inputs), which keeps
        # the selected score at 8 c exactly and the leak small; elsewhere the row has no decoy
        decoy = torch.where(decoy == pi + 1, decoy, torch.full_like(decoy, -1))
    return pi.contiguous(), decoy, (ATTN_C if decoy is None else ATTN_C_DECOY)


def onehot_attention_inputs(B, H, N, pi, c, seed, decoy=None, lens=None, causal=False, device="cpu"):
    """qkv [B*N, 3*H*64] (fp32 holding values exact in bf16) whose softmax selects one key per query, with
    independent data per (b, h): k_j = code_j, a random +-1 vector of 64; q_i = c * code_pi(i) (+ c * code_decoy(i));
    v small integers in [-4, 4].  pi / decoy: int64 [B, N] (decoy -1: none).  Returns (qkv, pi, leak, sel_score):
    leak is the fp64 maximum over queries of the softmax weight outside the selected key under the mask (lens,
    causal), sel_score [B, H, N] the exact score q_i . k_pi(i) / 8 every lse must equal.  The data are drawn on the
    CPU from the seed; device only says where the leak is evaluated."""
    g = torch.Generator().manual_seed(seed)
    # code_0 uniform, code_{j+1} = code_j with a random half of its 64 signs flipped: every code is uniform on its
    # own, consecutive codes are exactly orthogonal, codes further apart correlate like independent ones
    step = (torch.rand(B, H, N, 64, generator=g).argsort(-1).argsort(-1) < 32).float() * 2 - 1
    step[:, :, 0] = (torch.randint(0, 2, (B, H, 64), generator=g) * 2 - 1).float()
    code = torch.cumprod(step, 2)
    v = torch.randint(-4, 5, (B, H, N, 64), generator=g).float()
    idx = pi[:, None, :, None].expand(B, H, N, 64)
    q = c * torch.gather(code, 2, idx)
    if decoy is not None:
        has = (decoy >= 0)[:, None, :, None]
        didx = decoy.clamp_min(0)[:, None, :, None].expand(B, H, N, 64)
        q = q + c * torch.gather(code, 2, didx) * has
    qkv = torch.stack([q, code, v], 2)  # [B, H, 3, N, 64]
    qkv = qkv.permute(0, 3, 2, 1, 4).reshape(B * N, 3 * H * 64).contiguous()
    cnt = attn_allowed_count(B, N, lens, causal).to(device)
    qd, kd, pid = q.to(device), code.to(device), pi.to(device)
    leak = 0.0
    sel = torch.empty(B, H, N, dtype=torch.float64)
    for b in range(B):
        kmax = int(cnt[b].max())
        # integer scores: exact in fp32 (|q . k| <= 64 * 4 c), so the fast fp32 product is the exact one
        s = (qd[b] @ kd[b, :, :kmax].transpose(-1, -2)).double() / 8.0  # [H, N, kmax]
        ok = torch.arange(kmax, device=device)[None, :] < cnt[b][:, None]  # [N, kmax]
        ssel = torch.gather(s, 2, pid[b][None, :, None].expand(H, N, 1))
        sel[b] = ssel[..., 0].cpu()
        w = torch.exp(s - ssel) * ok[None]
        w.scatter_(2, pid[b][None, :, None].expand(H, N, 1), 0.0)
        rest = w.sum(-1)
        leak = max(leak, float((rest / (1.0 + rest)).max()))
    return qkv, pi, leak, sel


def attn_cases():
    """(N, mask) over the full grid; the entry points and pi families multiply it in the test files."""
    return [(N, m) for N in ATTN_NS for m in ATTN_MASKS]


def attn_seed(N, mask, family):
    return 1000 * ATTN_MASKS.index(mask) + 7 * N + 13 * len(family)


def attn_onehot_case(N, mask, family, device="cpu"):
    """Everything a one-hot case needs: dict with qkv (fp32 CPU), pi, leak, sel_score, lens, B, H, c, mask [B, N]."""
    B, H = attn_dims(N, mask)
    lens, causal = attn_lens(N, mask), "causal" in mask
    seed = attn_seed(N, mask, family)
    pi, decoy, c = attn_pi(family, B, N, lens, causal, seed)
    for attempt in range(4):
        # among ~10^8 (query, key) pairs over all cases a few random codes nearly coincide with a query: such a
        # draw is replaced by the next seed (deterministic; the CPU file asserts the leak of what is returned)
        qkv, pi, leak, sel = onehot_attention_inputs(B, H, N, pi, c, seed + 1 + 100003 * attempt, decoy, lens, causal,
                                                       device)
        if leak < LEAK_MAX:
            break
    kmask = None if lens is None else (torch.arange(N)[None] < torch.tensor(lens)[:, None]).to(torch.int64)
    return dict(B=B, H=H, N=N, causal=causal, lens=lens, kmask=kmask, qkv=qkv, pi=pi, leak=leak, sel=sel, c=c,
                decoy=decoy)


# ------------------------------------------------------------------------------------------------ LayerNorm
LN_WIDTHS = [64, 96, 768, 1000, 2050, 4096]
LN_ROWS = [1, 5, 333]
LN_MODES = ["f32", "bf16", "x32_bf16", "x32_bf16_w32"]  # fwd / bwd, fwd / bwd, fwd2 / bwd2, fwd2 (bf16 w) / bwd3


def ln_fast_width(D):
    return D % 64 == 0 and D // 64 in (1, 2, 3, 4, 6, 8, 12, 16)


def ln_leading_dims(D, strided):
    """ldx, ldy, lddy, lddx, ldres: all D ("eq"), or five different values above D -- multiples of 4 ("vec": the
    register-resident kernels of the fast widths keep their vector accesses) or odd steps ("odd": at a fast width
    the call falls to the one-wave-per-row kernel; include/clipmi.h promises no alignment rule)."""
    if not strided:
        return [D] * 5
    if strided == "vec":
        return [D + 4 * k for k in (1, 2, 3, 4, 5)]
    return [D + k for k in (1, 3, 5, 7, 9)]


# ------------------------------------------------------------------------------------------------ exact sums
# The gradient reductions and the row gather / scatter (tests/test_gpu_reductions.py): every summed operand is an
# integer tensor whose partial and total sums stay below 2^24, so the fp32 result is exact in any order and the
# reference is an int64 sum.  The functions below restate the host arithmetic of the entry points (csrc/norm.hip,
# csrc/optim.hip), so that tests/test_cpu_kernel_checks.py can assert the loop regime every case is named for.
EXACT = 2 ** 24


def untouched(view):
    """True where no byte of a guarded view has been stored to (it still holds the guard pattern)."""
    return bool((view.contiguous().view(torch.uint8) == GUARD_PATTERN).all())


# ---- clipmi_colsum
COLSUM_LO, COLSUM_HI, BETA_MAX = -3, 8, 4  # x in [-3, 8] (sums grow with R), the accumulated-onto out in [-4, 4]


class ColsumCase:
    """out[N] (+)= column sums of x [R, N] with row stride N + ld_pad, x shifted x_off elements off a 16-byte
    boundary.  regime: what the case is there for (asserted from colsum_plan on the CPU)."""

    def __init__(self, R, N, ld_pad=0, x_off=0, beta=0, regime="vec"):
        self.R, self.N, self.ld_pad, self.x_off, self.beta, self.regime = R, N, ld_pad, x_off, beta, regime

    def id(self):
        return f"R{self.R}-N{self.N}-ld{self.ld_pad}-off{self.x_off}-b{self.beta}-{self.regime}"


def colsum_plan(R, N, ldx, x_off):
    """clipmi_colsum's host arithmetic and the loops of its second stage: chunks = clamp(ceil(R / 256), 1, 512),
    rows_per = ceil(R / chunks); the vector kernels when N, ldx and x's offset are multiples of 4 elements (8 bytes
    bf16, 16 bytes fp32; the workspace of the tests is 16-byte aligned), else one column per thread.  unrolled /
    remainder: whether some partial group of the reducer runs its unrolled loop / the loop after it
    (reduce_partials4_kernel: 64 groups, 8 partial rows 64 apart per unrolled pass; reduce_partials_kernel: 16
    groups, 2 rows 16 apart per pass, then at most one more)."""
    chunks = min(max((R + 255) // 256, 1), 512)
    rows_per = (R + chunks - 1) // chunks
    vec = N % 4 == 0 and ldx % 4 == 0 and x_off % 4 == 0
    groups, depth, step = (64, 8, 64) if vec else (16, 2, 16)
    unrolled = remainder = False
    for ty in range(groups):
        p = ty
        while p + (depth - 1) * step < chunks:
            unrolled = True
            p += depth * step
        remainder |= p < chunks
    return dict(chunks=chunks, rows_per=rows_per, vec=vec, unrolled=unrolled, remainder=remainder,
                col_blocks=((N // 4 if vec else N) + 255) // 256)


def colsum_cases():
    cases = []
    # the vector kernels at every small R x N x ldx x beta; N = 1028: a second column block with one live thread
    for R in (1, 255, 257):
        for N in (4, 8, 1028):
            for ld_pad in (0, 4):
                for beta in (0, 1):
                    cases.append(ColsumCase(R, N, ld_pad, 0, beta, "vec"))
    # 449 chunks: partial group 0 of reduce_partials4 runs its unrolled loop, the others the remainder loop;
    # 131,073 rows: the chunk count capped at 512, so rows_per = 257
    for R, regime in ((114944, "vec-unrolled"), (131073, "vec-capped")):
        cases.append(ColsumCase(R, 8, 0, 0, 1, regime))
        cases.append(ColsumCase(R, 8, 4, 0, 0, regime))
    # one column per thread: N % 4 != 0, ldx % 4 != 0 or x off its vector boundary
    for R in (1, 255, 257):
        for i, N in enumerate((1, 5, 257)):
            cases.append(ColsumCase(R, N, 0, 0, (R + i) % 2, "scalar"))
            cases.append(ColsumCase(R, N, 1, 0, (R + i + 1) % 2, "scalar"))
        cases.append(ColsumCase(R, 8, 1, 0, R % 2, "scalar"))       # N % 4 == 0, ldx = N + 1
        cases.append(ColsumCase(R, 8, 4, 1, (R + 1) % 2, "scalar"))  # N, ldx % 4 == 0, x one element off
    cases.append(ColsumCase(114944, 5, 1, 0, 1, "scalar-unrolled"))
    cases.append(ColsumCase(131073, 1, 0, 0, 0, "scalar-capped"))
    cases.append(ColsumCase(131073, 8, 4, 1, 1, "scalar-capped"))
    ids = [c.id() for c in cases]
    assert len(set(ids)) == len(ids), "duplicate colsum case"
    return cases


def colsum_inputs(case, dtype):
    """(x [R, N] of dtype on the CPU, out0 [N] fp32, ref [N] int64): the same integers for both dtypes."""
    x = integer_tensor((case.R, case.N), COLSUM_LO, COLSUM_HI, dtype, 17 + case.R + case.N)
    out0 = integer_tensor((case.N,), -BETA_MAX, BETA_MAX, torch.float32, 18 + case.N)
    ref = x.long().sum(0) + (out0.long() if case.beta else 0)
    return x, out0, ref


# ---- clipmi_period_sum
PERIOD_NB = [1, 4, 5, 28, 29, 32, 33, 61]
PERIOD_PT = [(1, 1), (50, 50), (50, 1), (50, 7)]
PERIOD_D = [4, 252, 256, 260, 768]
PERIOD_MAX = 8  # x in [-8, 8]


class PeriodCase:
    """out[t][:] (+)= sum over b < nb of x[b * period + t][:] for t < nt; x [nb * period, D], row stride D + ld_pad."""

    def __init__(self, nb, period, nt, D, ld_pad, beta):
        self.nb, self.period, self.nt, self.D, self.ld_pad, self.beta = nb, period, nt, D, ld_pad, beta

    def id(self):
        return f"nb{self.nb}-p{self.period}-nt{self.nt}-D{self.D}-ld{self.ld_pad}-b{self.beta}"


def period_plan(nb):
    """period_sum_kernel's loops: wave w of 4 takes rows b = w, w + 4, ...; the 8-deep unrolled loop runs while
    b + 28 < nb (b += 32), the tail loop takes what is left.  Returns per wave (unrolled passes, tail rows)."""
    plan = []
    for w in range(4):
        b, passes, tail = w, 0, 0
        while b + 28 < nb:
            passes += 1
            b += 32
        while b < nb:
            tail += 1
            b += 4
        plan.append((passes, tail))
    return plan


def period_cases():
    cases = []
    for i, nb in enumerate(PERIOD_NB):  # every nb with (50, 7) and D = 260, ldx and beta alternating
        cases.append(PeriodCase(nb, 50, 7, 260, 4 * (i % 2), (i // 2) % 2))
        cases.append(PeriodCase(nb, 50, 7, 260, 4 * ((i + 1) % 2), (i // 2 + 1) % 2))
    # the other (period, nt) and widths, in and out of the unrolled loop
    cases += [PeriodCase(61, 1, 1, 4, 0, 0), PeriodCase(5, 1, 1, 768, 4, 1), PeriodCase(33, 50, 50, 252, 4, 1),
              PeriodCase(4, 50, 50, 256, 0, 0), PeriodCase(29, 50, 1, 768, 0, 1), PeriodCase(28, 50, 1, 4, 4, 0),
              PeriodCase(32, 50, 7, 256, 4, 0), PeriodCase(61, 50, 7, 252, 0, 1), PeriodCase(1, 50, 50, 768, 4, 0)]
    ids = [c.id() for c in cases]
    assert len(set(ids)) == len(ids), "duplicate period_sum case"
    return cases


def period_inputs(case, dtype):
    """(x [nb * period, D] on the CPU, out0 [nt, D] fp32, ref [nt, D] int64)."""
    c = case
    x = integer_tensor((c.nb * c.period, c.D), -PERIOD_MAX, PERIOD_MAX, dtype, 31 + c.nb + c.D + c.period)
    out0 = integer_tensor((c.nt, c.D), -BETA_MAX, BETA_MAX, torch.float32, 32 + c.D)
    ref = x.long().view(c.nb, c.period, c.D)[:, :c.nt].sum(0) + (out0.long() if c.beta else 0)
    return x, out0, ref


# ---- clipmi_text_embed_bwd / clipmi_text_embed
EMBED_PATTERNS = ["equal", "distinct", "ascending", "alternate", "eos_tail", "oov"]
EMBED_V = [1, 1000, 1024, 1025, 49408]
EMBED_R = [1, 63, 64, 65, 257, 5000]
EMBED_D = [4, 260, 512]
EMBED_MAX = 3       # dx0 in [-3, 3]
EMBED_OOV = [-1, None, 2 ** 40]  # None: V itself


class EmbedBwdCase:
    def __init__(self, V, R, D, pattern, beta):
        self.V, self.R, self.D, self.pattern, self.beta = V, R, D, pattern, beta

    def id(self):
        return f"V{self.V}-R{self.R}-D{self.D}-{self.pattern}-b{self.beta}"


def embed_bwd_cases():
    rows = [(1, 1, 4, "equal", 0), (1, 5000, 260, "equal", 1), (1, 64, 512, "oov", 0),
            (1000, 63, 512, "distinct", 0), (1000, 64, 260, "alternate", 1), (1000, 65, 4, "ascending", 0),
            (1000, 5000, 260, "eos_tail", 1), (1000, 257, 512, "oov", 0), (1000, 5000, 4, "equal", 0),
            (1024, 257, 260, "distinct", 1), (1024, 5000, 4, "oov", 1), (1024, 64, 512, "ascending", 1),
            (1025, 65, 260, "distinct", 0), (1025, 5000, 260, "eos_tail", 0), (1025, 257, 512, "alternate", 0),
            (1025, 1, 4, "equal", 1),
            (49408, 5000, 4, "eos_tail", 1), (49408, 5000, 4, "oov", 0), (49408, 5000, 4, "distinct", 0),
            (49408, 64, 4, "ascending", 1), (49408, 1, 4, "equal", 0), (49408, 5000, 4, "equal", 1),
            (49408, 63, 4, "alternate", 0), (49408, 257, 4, "ascending", 0)]
    return [EmbedBwdCase(*r) for r in rows]


def scan_per(V):
    """id_scan_kernel: the vocabulary entries each of its 1024 threads scans."""
    return (V + 1023) // 1024


def embed_ids(V, R, pattern, seed):
    """int64 [R] ids of a pattern; the last id of the vocabulary is used wherever a pattern names one id."""
    g = torch.Generator().manual_seed(seed)
    rand = torch.randint(0, V, (R,), generator=g)
    if pattern == "equal":        # one id owns every 64-row chunk
        return torch.full((R,), V - 1, dtype=torch.int64)
    if pattern == "distinct":     # R <= V: every chunk flushes at every row
        assert R <= V
        return torch.randperm(V, generator=g)[:R].contiguous()
    if pattern == "ascending":
        return rand.sort().values
    if pattern == "alternate":
        return torch.where(torch.arange(R) % 2 == 0, V - 1, V // 2).to(torch.int64)
    if pattern == "eos_tail":     # the last 40 % of the rows hold the last id, like EOS padding
        rand[R - (2 * R) // 5:] = V - 1
        return rand
    assert pattern == "oov"       # about a third of the rows: -1, V and 2^40 in turn
    bad = torch.rand(R, generator=g) < 0.34
    if R >= 3:
        bad[:3] = True
    oov = torch.tensor([V if v is None else v for v in EMBED_OOV], dtype=torch.int64)
    return torch.where(bad, oov[torch.arange(R) % 3], rand)


def embed_bwd_inputs(case, dtype):
    """(ids [R] int64, dx0 [R, D] of dtype, g0 [V, D] fp32, ref1, ref2 [V, D] int64): ref1 after one call, ref2
    after a second one on the same buffers (beta: g0 + 2 sums; else the sum again)."""
    c = case
    ids = embed_ids(c.V, c.R, c.pattern, 41 + c.V + c.R)
    dx0 = integer_tensor((c.R, c.D), -EMBED_MAX, EMBED_MAX, dtype, 42 + c.R + c.D)
    g0 = integer_tensor((c.V, c.D), -BETA_MAX, BETA_MAX, torch.float32, 43 + c.V)
    ok = (ids >= 0) & (ids < c.V)
    s = torch.zeros(c.V, c.D, dtype=torch.int64).index_add_(0, ids[ok], dx0.long()[ok])
    if c.beta:
        return ids, dx0, g0, g0.long() + s, g0.long() + 2 * s
    return ids, dx0, g0, s, s


# (B, S, D, V): R = B * S is no multiple of 4; S in {1, 77}; every D
EMBED_FWD_CASES = [(3, 77, 260, 1000), (5, 1, 4, 2), (1, 77, 512, 1025), (7, 1, 512, 1000), (3, 77, 4, 49408),
                   (9, 1, 260, 1)]


def embed_fwd_ids(B, S, V, seed):
    """Random valid ids [B * S] with 0 and V - 1 present."""
    ids = torch.randint(0, V, (B * S,), generator=torch.Generator().manual_seed(seed))
    ids[0], ids[-1] = V - 1, 0
    if B * S > 2:
        ids[1] = 0
    return ids


# ---- clipmi_pool_index / clipmi_gather_rows / clipmi_scatter_rows
ROWS_B = [1, 255, 256, 257]
ROWS_S = [1, 77]
ROWS_D = [1, 255, 256, 257, 768]
POOL_KINDS = ["first_token", "no_eos", "several_eos", "tied_max"]
POOL_EOS = 49407


def pool_inputs(kind, B, S, seed):
    """(ids [B, S] int64, mode, expected [B] int32)."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 1000, (B, S), generator=g)
    pos = torch.arange(S).expand(B, S)
    if kind == "first_token":
        ids[:, S // 2] = POOL_EOS
        return ids, 0, torch.zeros(B, dtype=torch.int32)
    if kind == "no_eos":
        return ids, 1, torch.zeros(B, dtype=torch.int32)
    hit = torch.rand(B, S, generator=g) < 0.2  # several positions per row; at least the row's own, (b + S // 2) mod S
    hit[torch.arange(B), (torch.arange(B) + S // 2) % S] = True
    if kind == "several_eos":
        ids[hit] = POOL_EOS
        mode = 1
    else:  # the maximum at several positions, below it everywhere else
        ids[hit] = 1000 + (torch.arange(B)[:, None].expand(B, S))[hit]
        mode = 2
    first = torch.where(hit, pos, torch.full_like(pos, S)).min(1).values
    return ids, mode, first.to(torch.int32)


def rows_cases():
    """(B, S, D): every B with every D at S = 1; every D at S = 77 with one row; every B at S = 77 with D = 1."""
    cases = [(B, 1, D) for B in ROWS_B for D in ROWS_D]
    cases += [(1, 77, D) for D in ROWS_D if (1, 77, D) not in cases]
    cases += [(B, 77, 1) for B in ROWS_B if (B, 77, 1) not in cases]
    cases.append((5, 77, 257))
    return cases


def rows_idx(B, S, seed):
    """int32 [B] token positions with 0 and S - 1 present."""
    idx = torch.randint(0, S, (B,), generator=torch.Generator().manual_seed(seed)).to(torch.int32)
    idx[0] = S - 1
    idx[-1] = 0 if B > 1 else S - 1
    return idx


# ---- clipmi_grad_norm / _multi / clipmi_grad_scale / clipmi_sum2
NORM_PASS = 1024 * 256 * 4  # elements of one grid-stride pass of sumsq_partial_kernel: 1024 blocks x 256 lanes x 4
GRAD_NS = [1, 3, 4, 5, 1023, NORM_PASS + 7]
GRAD_MULTI_NS = [5, NORM_PASS + 7, 0]
GRAD_MAX = 3
SUM2_NS = [1, 1023, 1025, 5000]


def grad_plan(n):
    """sumsq_partial_kernel over n elements: (full grid-stride passes of the vector loop, vectors of a further
    partial pass, scalar tail elements)."""
    n4 = n // 4
    return n4 // (NORM_PASS // 4), n4 % (NORM_PASS // 4), n - 4 * n4


def grad_tensor(n, seed):
    """Integers in [-3, 3], fp32 [n], first and last element non-zero."""
    g = integer_tensor((n,), -GRAD_MAX, GRAD_MAX, torch.float32, seed)
    g[0], g[-1] = -3.0, 3.0
    return g


def clip_expect(sumsq, max_norm):
    """(norm as fp32, the clip coefficient: exactly 1.0 where the contract says so, else the fp64 value of
    max_norm / (norm + 1e-6) on the fp32 norm, fp32 constant and fp32 max_norm)."""
    norm = torch.tensor(float(sumsq), dtype=torch.float64).sqrt().float()
    mn = float(torch.tensor(max_norm, dtype=torch.float32))
    if mn <= 0 or float(norm) == 0.0 or float(norm) < mn:
        return norm, 1.0
    eps = float(torch.tensor(1e-6, dtype=torch.float32))
    return norm, min(1.0, mn / (float(norm) + eps))


# ---- clipmi_l2norm_* / clipmi_softmax_rows*
L2_ES = [1, 4, 63, 64, 65, 512, 1000]
L2_BS = [1, 4, 5]
SM_NS = [1, 63, 64, 65, 200]
SM_RS = [1, 4, 5]


def l2norm_rows(B, E, entries, seed):
    """x [B, E] fp32 with `entries` (1 or 4) non-zero elements +-2^k per row, k in [-3, 3] by row: |x| = 2^k or
    2^(k+1), so y = +-1 or +-0.5 exactly.  Returns (x, y, nrm)."""
    assert entries in (1, 4) and E >= entries
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(B, E)
    y = torch.zeros(B, E)
    nrm = torch.zeros(B)
    for r in range(B):
        k = r % 7 - 3
        cols = torch.randperm(E, generator=g)[:entries]
        if r == 0 and E - 1 not in cols.tolist():
            cols[0] = E - 1  # row 0: the row's last element is live
        sign = (torch.randint(0, 2, (entries,), generator=g) * 2 - 1).float()
        x[r, cols] = sign * 2.0 ** k
        y[r, cols] = sign * (1.0 if entries == 1 else 0.5)
        nrm[r] = 2.0 ** (k if entries == 1 else k + 1)
    return x, y, nrm
