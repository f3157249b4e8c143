"""The tiled GEMM (csrc/gemm_mfma.hip, gemm_epilogue.h, gemm_w4.h), the generic kernel (gemm_generic.hip)
and the stream-K engine (gemm_sk.hip), value for value, on every dispatch path and epilogue form.

Method. The bf16 operands hold integers in [-4, 4] and K <= 4096: every partial sum is an integer
below 2^16, so every fp32 accumulation order (MFMA, split-K tree, stream-K fold, VALU) gives the same
exact z. alpha is a power of two, bias entries are multiples of 1/8 and dropout runs at p = 0.5
(scale 2, scale^2 4, 1/scale 0.5, threshold 32768), so for act in {none, ReLU} the whole epilogue is
exact in whatever order it multiplies: the output must EQUAL bf16_rne(fp32(ref)) (ref in fp64), and
the fp32 colsum the exact column sums. p = 0.5 only looks at the top bit of a draw, so every dropout
form also runs at p = 0.3 (threshold 19661, scale not representable): there the zero pattern is
exact and kept values stay within 2^-8 |ref| (one bf16 rounding at 2^-9, at most three fp32
roundings of the scale product). Equality is by value: -0 == +0.

Sigmoid / tanh: |y - ref| <= 2^-8 |ref| + 1e-5 forward (fp32 outputs: 1e-5 |ref| + 1e-5), the stage
tests' 1e-5 |ref| + 4 2^-24 |g| scales + 2^-8 |ref| backward, colsum M 2^-24 sum|ref| + the sum of
the per-element fp32 bounds.

Every launch passes engine = 1 (PZ_GEMM_SK cannot move it) or 2, and asserts PF.gemm_last_kernel().

Dispatch cells reached (kFill = 240):
  mfma/var6/128x128/ek0/split1      S128 (200, 136, 96): every form, ragged both ways; Ssplit with no_split
  mfma/var30/256x128/ek4|5|6/split1 S256x128 (2560, 3072, 64): the w128_fixed kinds
  mfma/var30/256x128/ek0/split1     S256x128: every other form and layout
  mfma/var30/256x256/ek0|2|4|5|6    S256 (4096, 3840, 64) forward; ragged N (4096, 3832, 64): the !full_tile store loop
  mfma/var30/256x256/ek0|3          S256 dX at K = 64; ek0 also the colsum / aux forms at K = 128
  w4/var40/256x256/ek1|3            S256 dX at K = 128, plain and bitmask backward
  mfma/var30/256x256/ek1 and ek0    dW bf16 and fp32; ek0 the (A M-contiguous, B K-contiguous) layout
  mfma/var6/256x256/ek0/split1      ragged M (4088, 3840, 64) and K % 64 != 0 (4096, 3840, 96)
  mfma/var30/256x256/ek*/split8     Ssplit (1536, 1280, 4096): forward, dX, dW (fp32 accumulate: the last
                                    arriver's read-modify-write)
  mfma/var6/256x256/ek0/split8      Ssplit with ragged M (1528, 1280, 4096)
  generic/var0/64x64/ek0/split1     (67, 45, 23) forced, bf16 and fp32 operands; bf16 out + accumulate at S128;
                                    fp64 operands with fp64 C, bias, aux and column sums there and at (9, 9, 9)
                                    (fp64 bounds: run_case; the fp32 / fp64 matrix-core kernel runs through
                                    run_case from test_gemm_wide_exact_gpu.py)
  sk/var0/256x256/ek1|3|4|5|6|100    (1536, 1280, 512) on 37 CUs (30 data-parallel tiles) and 200 (two K halves);
                                    every schedule shape of the engine (two-tile regions, data-parallel rounds,
                                    uneven cuts, pairs) and every epilogue it has, ek0 and ek2 among them:
                                    test_gemm_sk_exact_gpu.py
Not reached on purpose: the !buffer_addressable fallbacks (VAR 0; need a 4 GiB operand), fp32 outputs of the
stream-K engine outside the dW layout (it has none). fp8 operands run through this file's run_case
from test_gemm_fp8_exact_gpu.py (its ``fmts`` / ``layout`` / ``q8`` arguments); gemm_pair and
gemm_update (EPI_OPT) are in test_gemm_pair_update_gpu.py.

Measured on MI355X (the file takes about 17 s): every kernel name above as predicted from
gemm_choose, every none / ReLU form at p = 0.5 and 1.0 exact. Worst err / bound: p = 0.3 kept values
0.987 (the bound has no slack: a bf16 rounding alone reaches 2^-8 |ref| just above a power of two,
its unit roundoff is 2^-8, not 2^-9), their colsum 0.013; sigmoid / tanh forward 0.994 (the same bf16
rounding), backward 0.993 with colsum 0.005.
Kinds that store -0 for a dropped negative value (they multiply by 0.f; the ReLU bitmask and the
fp8 copy read it as zero): the tiled kernels' generic epilogue ek0 (dropout_row) in the forward
no-activation and sigmoid / tanh dropout forms and in every backward-from-aux form, and the VALU
kernel's backward-from-aux forms. ek2-6 and the bitmask backward ek3 (tiled, w4, stream-K) select
+0; so do the VALU kernel's forward forms and every ReLU forward form (max(x, 0) = +0 first).
"""
import functools
import math
from dataclasses import dataclass
from types import SimpleNamespace

import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.helpers import (assert_gemm_exact, exact_operands, exact_operands_fp8, fp8_encode_reference,
                           gemm_epilogue_reference, keep2d_cached)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2
SEED = (0x1234ABCD, 0x00C0FFEE)
LID_PRE, LID_POST = 3, 4
U32 = 2.0 ** -24
NONE, RELU, SIGM, TANH = PF.ACT_NONE, PF.ACT_RELU, PF.ACT_SIGMOID, PF.ACT_TANH
LAYOUTS = {"fwd": (True, False), "dx": (True, True), "dw": (False, False), "tn": (False, True)}

SHAPES = {
    "S128": (200, 136, 96),
    "S256x128": (2560, 3072, 64),
    "S256": (4096, 3840, 64),
    "S256k128": (4096, 3840, 128),
    "S256rN": (4096, 3832, 64),
    "S256rM": (4088, 3840, 64),
    "S256k96": (4096, 3840, 96),
    "Ssplit": (1536, 1280, 4096),
    "SsplitrM": (1528, 1280, 4096),
}


@dataclass(frozen=True)
class Form:
    layout: str
    mode: int = PF.EPI_STORE
    act: int = NONE
    pre: bool = False
    post: bool = False
    bias: bool = False
    out: torch.dtype = BF16
    mask: bool = False        # EPI_FWD: write the ReLU bitmask; EPI_BWD: read it instead of aux
    aux: bool = False
    colsum: bool = False
    out8: bool = False
    accumulate: bool = False
    alpha: float | None = None
    p: tuple = (0.5,)

    @property
    def drop(self):
        return self.pre or self.post


P2 = (0.5, 0.3)
FWD = dict(layout="fwd", mode=PF.EPI_FWD, bias=True)
BWD = dict(layout="dx", mode=PF.EPI_BWD, colsum=True)
FORMS = {
    # forward (A K-contiguous, B N-contiguous), bf16 out
    "plain": Form("fwd"),
    "store_bias": Form("fwd", bias=True),
    "none_nodrop": Form(**FWD),
    "none_pre": Form(**FWD, pre=True, mask=True, p=P2),                      # EK_F_PRE (+ the bitmask of y > 0)
    "none_post": Form(**FWD, post=True, p=P2),
    "none_prepost": Form(**FWD, pre=True, post=True, p=P2),
    "relu_nodrop": Form(**FWD, act=RELU, mask=True),
    "relu_pre": Form(**FWD, act=RELU, pre=True, mask=True, p=P2),
    "relu_post": Form(**FWD, act=RELU, post=True, mask=True, p=P2),          # EK_F_RELU_POST
    "relu_prepost": Form(**FWD, act=RELU, pre=True, post=True, mask=True, p=P2),  # EK_F_RELU_PREPOST
    "relu_dropall": Form(**FWD, act=RELU, pre=True, post=True, mask=True, p=(1.0,)),
    "sigmoid_nodrop": Form(**FWD, act=SIGM),
    "sigmoid_prepost": Form(**FWD, act=SIGM, pre=True, post=True, p=P2),
    "tanh_nodrop": Form(**FWD, act=TANH),
    "tanh_prepost": Form(**FWD, act=TANH, pre=True, post=True, p=P2),
    "relu_prepost_out8": Form(**FWD, act=RELU, pre=True, post=True, mask=True, out8=True),
    "relu_nodrop_out8": Form(**FWD, act=RELU, mask=True, out8=True),
    # dX (both K-contiguous), bf16 out
    "dx_plain": Form("dx"),
    "dx_store_colsum": Form("dx", colsum=True),
    "dx_relu_mask": Form(**BWD, act=RELU, pre=True, post=True, mask=True, p=P2),
    "dx_relu_aux": Form(**BWD, act=RELU, pre=True, post=True, aux=True, p=P2),
    "dx_sigmoid_aux": Form(**BWD, act=SIGM, pre=True, post=True, aux=True, p=P2),
    "dx_tanh_aux": Form(**BWD, act=TANH, pre=True, post=True, aux=True, p=P2),
    "dx_relu_mask_out8": Form(**BWD, act=RELU, pre=True, post=True, mask=True, out8=True),
    # dW (both M/N-contiguous)
    "dw_bf16": Form("dw"),
    "dw_f32": Form("dw", out=F32),
    "dw_f32_acc": Form("dw", out=F32, alpha=0.25, accumulate=True, bias=True),
    # (A M-contiguous, B K-contiguous)
    "tn_bf16": Form("tn"),
    "tn_f32": Form("tn", out=F32),
    # generic-kernel extras: any output type accumulates, fp32 outputs take the stage epilogues
    "fwd_acc": Form("fwd", alpha=0.25, accumulate=True, bias=True),
}
FWD_FORMS = [n for n, f in FORMS.items() if f.layout == "fwd" and not f.accumulate]
DX_FORMS = [n for n, f in FORMS.items() if f.layout == "dx"]
DW_FORMS = [n for n, f in FORMS.items() if f.layout == "dw"]


def epi_kind(f: Form) -> int:
    """The epilogue kind the tiled kernels specialise on (gemm_last_kernel's ``ek`` where the tile
    config has that kind): 1 plain store, 2 ReLU stage, 3 bitmask backward, 4-6 fixed stages, 0 any."""
    if f.out != BF16 or f.accumulate:
        return 0
    if f.mode == PF.EPI_STORE:
        return 1 if not (f.bias or f.colsum) else 0
    if f.mode == PF.EPI_BWD:
        return 3 if f.mask else 0
    if f.act not in (NONE, RELU):
        return 0
    if 1.0 not in f.p:
        if f.act == RELU and f.post:
            return 5 if f.pre else 4
        if f.act == NONE and f.pre and not f.post:
            return 6
    return 2


def expected_kernel(cls: str, form: str, no_split: bool = False) -> str:
    """gemm_last_kernel() of shape class ``cls`` x form, read off gemm_choose (csrc/gemm_dispatch.h: choose_bf16) / gemm_split."""
    f, ek = FORMS[form], epi_kind(FORMS[form])
    if cls == "S128" or no_split:
        return "mfma/var6/128x128/ek0/split1"
    if cls in ("S256rM", "S256k96"):
        return "mfma/var6/256x256/ek0/split1"
    if cls == "SsplitrM":
        return "mfma/var6/256x256/ek0/split8"
    if cls == "S256x128":
        return f"mfma/var30/256x128/ek{ek if ek >= 4 else 0}/split1"
    split = 8 if cls == "Ssplit" else 1
    if cls == "S256k128" and ek in (1, 3):
        return f"w4/var40/256x256/ek{ek}/split1"
    # 256x256 on the 64-deep ring: the forward has the ReLU and fixed kinds, dX the bitmask
    # backward, dW the plain store; everything else runs the generic epilogue
    has = {"fwd": (2, 4, 5, 6), "dx": (3,), "dw": (1,), "tn": ()}[f.layout]
    return f"mfma/var30/256x256/ek{ek if ek in has else 0}/split{split}"


# ------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def operands(M, N, K, a_kc, b_kc, fmts=None, dtype=BF16, hi=4):
    """Integer operands in [-hi, hi] on the device: ``dtype``, or (``fmts`` = the two fp8 formats) fp8."""
    seed = M + 3 * N + 7 * K + 2 * a_kc + b_kc
    a, b, z = (exact_operands(M, N, K, a_kc, b_kc, seed, dtype, hi) if fmts is None
               else exact_operands_fp8(M, N, K, a_kc, b_kc, *fmts, seed))
    return a.to(DEV), b.to(DEV), z.to(DEV)


def keep(M, N, idx_ld, lid, p):
    """Device keep mask of an [M, N] output (element index m * idx_ld + n); rows are generated up
    to the next multiple of 256 so that the ragged-M classes share their whole-tile class's mask."""
    if p >= 1.0:
        return torch.zeros(M, N, dtype=torch.bool, device=DEV)
    return _keep_dev(-(-M // 256) * 256, N, idx_ld, lid, p)[:M]


@functools.lru_cache(maxsize=None)
def _keep_dev(rows, N, idx_ld, lid, p):
    return keep2d_cached(rows, N, idx_ld, SEED, lid, p).to(DEV)


@functools.lru_cache(maxsize=None)
def bias_vec(N):
    g = torch.Generator(device="cpu").manual_seed(N)
    return (torch.randint(-32, 33, (N,), generator=g).float() / 8).to(DEV)  # multiples of 1/8 in [-4, 4]


@functools.lru_cache(maxsize=None)
def stage_source(M, N, act, y_scale, dtype=BF16):
    """What a backward epilogue reads of the stage it differentiates: ReLU -> random bits (y > 0) and
    an integer-valued y with that sign pattern; sigmoid / tanh -> a stored y = act(u) * y_scale,
    rounded once to ``dtype``."""
    g = torch.Generator(device="cpu").manual_seed(M * 31 + N + act)
    if act == RELU:
        y = torch.randint(-3, 4, (M, N), generator=g).to(DEV, dtype)
        return y, y > 0
    u = torch.randn(M, N, generator=g, dtype=F64)
    return ((torch.sigmoid(u) if act == SIGM else torch.tanh(u)) * y_scale).to(DEV, dtype), None


@functools.lru_cache(maxsize=None)
def old_c(M, N):
    g = torch.Generator(device="cpu").manual_seed(M + N)
    return torch.randint(-64, 65, (M, N), generator=g).to(DEV, F32)


def framed(rows, cols, dtype, strided, fill=7.0, src=None, pad=8, odd=0):
    """A [rows, cols] tensor: contiguous, or (``strided``) the column slice [:, pad : pad + cols] of a
    tensor 2 pad + odd columns wider and 8 rows taller. Returns (view, base); everything is ``fill``
    (then ``src``). pad = 1 with an odd width puts an fp32 / fp64 view's first element 4 / 8 bytes
    past a 16-byte boundary and its rows a stride apart that is no multiple of 16 bytes."""
    if not strided:
        base = torch.full((rows, cols), fill, device=DEV, dtype=F32).to(dtype)
        view = base
    else:
        base = torch.full((rows + 8, cols + 2 * pad + odd), fill, device=DEV, dtype=F32).to(dtype)
        view = base[:rows, pad:pad + cols]
    if src is not None:
        view.copy_(src)
    return view, base


def frame_untouched(view, base, fill=7.0):
    """Every element of ``base`` outside ``view`` still holds ``fill``."""
    if view is base:
        return True
    pad = view.storage_offset() - base.storage_offset()
    # (always a copy: .float() of an fp32 base is the base itself, and would be overwritten below)
    probe = base.clone() if base.dtype == F64 else base.float().double()
    probe[:view.shape[0], pad:pad + view.shape[1]] = fill
    return bool((probe == fill).all())


def alpha_of(f: Form, K: int) -> float:
    if f.alpha is not None:
        return f.alpha
    if f.act in (SIGM, TANH) and f.mode == PF.EPI_FWD:
        # h ~ N(0, 1): var(a b) = (60 / 9)^2 for integers uniform in [-4, 4], so std(z) = 6.67 sqrt(K)
        return 2.0 ** -round(0.5 * math.log2(44.4 * K))
    if f.out8 and f.mode == PF.EPI_FWD:
        return 16.0 if K <= 192 else 2.0   # |y| 2^-3 passes 448 on some elements: the e4m3 clamp runs
    return 0.5


def within(got, ref, bound, what):
    got = got.double()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: max err {err.max().item():.3e}, worst err/bound {worst:.3f}")
    assert (err <= bound).all(), (what, err.max().item(), worst)


def fp8_codes_equal(got, y, qs, fmt):
    """``got`` (fp8 tensor) holds the nearest-even saturating codes of y * qs, up to the sign of zero."""
    g = got.contiguous().view(torch.uint8).cpu()
    want = fp8_encode_reference(y.double().cpu() * qs, fmt)
    same = (g == want) | (((g | want) & 0x7F) == 0)
    assert same.all(), (int((~same).sum()), g[~same][:4].tolist(), want[~same][:4].tolist())


# fp8 operands: the dequantisation scales (device scalars; powers of two). OUT8_Q: the out8 factors
# "sat" (some outputs pass the format's largest value) and "sub" (some land on subnormal codes: the
# smallest is 2^-9 / 2^-16, the smallest normal value 2^-6 / 2^-14)
F8_SCALES = (0.25, 2.0 ** -6)
OUT8_Q = {E4M3: dict(std=2.0 ** -3, sat=2.0 ** -3, sub=2.0 ** -8, tiny=2.0 ** -9, normal=2.0 ** -6, top=448.0),
          E5M2: dict(std=2.0 ** -3, sat=2.0 ** 8, sub=2.0 ** -16, tiny=2.0 ** -16, normal=2.0 ** -14, top=57344.0)}


@functools.lru_cache(maxsize=None)
def dev_scalar(v):
    return torch.tensor([v], device=DEV)


U64 = 2.0 ** -53
# fp64 operands, sigmoid / tanh forward: bound on |y - ref| in units of 2^-53 |ref|, ref = torch's fp64
# CPU result on the same (exact) h. The device exp / tanh are the only steps whose error is not derived:
# 4 x the worst measured on MI355X, 8.001 (tanh; sigmoid 3.567), wide and generic kernel alike. A
# figure above 16 would be a finding, not a reason to widen this.
F64_FWD_ACT_ULPS = 32.0
# fp64 operands, sigmoid / tanh backward from an fp64 aux, in units of 2^-53 |g| scale_pre scale_post
# (run_case's docstring derives it)
F64_BWD_ACT_ULPS = 16.0


def run_case(shape, form, p=0.5, *, engine=1, cus=0, force_generic=False, no_split=False, strided=False,
             idx_ld=0, in_dtype=BF16, out_dtype=None, store_c=True, layout=None, fmts=None, q8="std",
             bias_dtype=F32, colsum_dtype=F32, aux_dtype=None, hi=4, pad=None, odd=0, alpha=None):
    """One GEMM launch of ``form`` checked against the fp64 reference. Returns what it produced.
    ``fmts`` = (format of A, format of B): fp8 operands in layout ``layout`` (default: the form's),
    dequantised by F8_SCALES (folded into the reference's alpha; the kernel's alpha is raised by as
    much, so that every form sees the values the bf16 run sees). ``q8``: which OUT8_Q factor the
    fp8 copy takes ("std": 2^-3, at which e4m3 saturates too). ``alpha``: a power of two instead of
    alpha_of's (whose e4m3 saturation is sized for K <= 192 and K = 4096).

    ``in_dtype`` fp32 / fp64 (gemm_wide.hip, gemm_generic.hip): ``hi`` = the operands' integer range
    (they are generated in ``in_dtype``), ``bias_dtype`` / ``colsum_dtype`` fp32 or fp64,
    ``aux_dtype`` = the stored stage output's type (given: y is rounded once to it, not to bf16 first),
    ``pad`` / ``odd`` = the frame of the strided views of A, B, C and aux (see framed); these
    operands never take the bf16 kernels' ReLU bitmask.

    fp64 operands run the epilogue in fp64 (u = 2^-53), so the exact forms must equal the reference
    in an fp64 C, and the others get fp64 bounds (+ one rounding of an fp32 / bf16 C):
      * p = 0.3, none / ReLU: exact zero pattern, kept values within 4 u |ref|: at most two
        multiplications by the double 1/(1-p) in the kernel (epi_scale<double>) and in the reference.
        The same reference with that scale rounded to fp32 must break the bound somewhere (asserted:
        otherwise the test could not tell which scale the kernel took).
      * sigmoid / tanh forward: F64_FWD_ACT_ULPS u |ref| against torch's fp64 CPU activations.
      * sigmoid / tanh backward from an fp64 aux y: F64_BWD_ACT_ULPS u |g| scale_pre scale_post.
        Let s = fl(1 / (1 - p)), i = fl(1 - p) (the spec's two doubles), a* = y i, d* = act'(a*) and
        T = g s d* s in real arithmetic; |a*| <= 1 (asserted), so a*^2 <= 1 and d* <= 1. epi_bwd:
        a = fl(y i) = a* (1 + e); tanh d = fl(1 - fl(a a)) is within (2 + 1) u a*^2 + u d* <= 4 u of
        d*, sigmoid d = fl(a fl(1 - a)) within 3 u d* + u a*^2 <= 1.75 u; then g1 = fl(g s),
        g2 = fl(g1 d), g3 = fl(g2 s) add 3 u d: |out - T| <= 7 u |g| s^2. The reference
        (stage_bwd_reference, on the CPU) divides: a' = fl(y / s) with s = (1 / i)(1 + e1) is within
        2 u of a*, so d' is within (4 + 1) u + u = 6 u of d*, and its three multiplications add
        3 u: |ref - T| <= 9 u |g| s^2. Together 16 u |g| s^2, with one dropout or none less.
      * column sums: M u_cs sum|ref| + the sum of the per-element bounds, u_cs = 2^-53 for an fp64
        colsum; on the exact forms they equal the reference's (every partial sum is exact)."""
    M, N, K = shape
    f = FORMS[form]
    a_kc, b_kc = LAYOUTS[layout or f.layout]
    a0, b0, z = operands(M, N, K, a_kc, b_kc, fmts, in_dtype if fmts is None else BF16, hi)
    out_dtype = out_dtype or f.out
    f64 = in_dtype == F64
    what = f"{form} {shape} p={p}"
    if in_dtype != BF16:
        what += f" {str(in_dtype)[6:]}->{str(out_dtype)[6:]}" + (" generic" if force_generic else "")
    alpha = alpha_of(f, K) if alpha is None else alpha
    k_alpha, scales = alpha, {}
    if fmts is not None:
        k_alpha = alpha / (F8_SCALES[0] * F8_SCALES[1])
        scales = dict(scale_a=dev_scalar(F8_SCALES[0]), scale_b=dev_scalar(F8_SCALES[1]))
    scale = 0.0 if p >= 1.0 else 1.0 / (1.0 - p)
    ld = idx_ld or N
    kp = keep(M, N, ld, LID_PRE, p) if f.pre else None
    kq = keep(M, N, ld, LID_POST, p) if f.post else None
    epi = PF.NO_EPI if f.mode == PF.EPI_STORE else PF.epi_spec(f.act, LID_PRE if f.pre else -1,
                                                                LID_POST if f.post else -1, p, SEED)
    bias = bias_vec(N).to(bias_dtype) if f.bias else None
    # (fp8 operands: 16-byte aligned slices of rows that are a multiple of 16 bytes apart)
    opad, cpad = pad or (8 if fmts is None else 16), pad or 8
    a, _ = framed(*a0.shape, in_dtype if fmts is None else fmts[0], strided, src=a0, pad=opad, odd=odd)
    b, _ = framed(*b0.shape, in_dtype if fmts is None else fmts[1], strided, src=b0, pad=opad, odd=odd)
    aux = bits = mask = aux_v = aux_base = None
    if f.mode == PF.EPI_BWD:
        y_src, bits = stage_source(M, N, f.act, scale if f.post else 1.0, aux_dtype or BF16)
        if f.mask:
            mask = PF.relu_mask_pack(bits)
        else:
            aux, bits = y_src.to(aux_dtype or out_dtype), None
            aux_v, aux_base = framed(M, N, aux.dtype, strided, src=aux, pad=cpad, odd=odd)
    elif f.mask and not force_generic and in_dtype == BF16:
        mask = torch.full(PF.relu_mask_shape(M, N), 0xAB, device=DEV, dtype=torch.uint8)
    c_old = old_c(M, N) if f.accumulate else None
    # fp64 sigmoid / tanh stages: the reference runs on the CPU (the device's own exp, tanh and
    # division are what is under test)
    host = f64 and f.act in (SIGM, TANH) and f.mode != PF.EPI_STORE

    def reference(sc):
        on = (lambda t: None if t is None else t.cpu()) if host else (lambda t: t)
        r, cs = gemm_epilogue_reference(on(z), alpha=alpha, bias=on(bias), mode=f.mode, act=f.act, keep_pre=on(kp),
                                        keep_post=on(kq), scale=sc, aux=on(aux), bits=on(bits), c_old=on(c_old))
        return r.to(DEV), cs.to(DEV)

    ref, cs_ref = reference(scale)
    c, c_base = framed(M, N, out_dtype, strided, fill=7.0 if (strided or not store_c) else float("nan"), src=c_old,
                       pad=cpad, odd=odd)
    if strided and pad == 1:  # off the 16-byte vector path: base and row stride
        for t in (a, b, c) + (() if aux_v is None else (aux_v,)):
            assert t.data_ptr() % 16 != 0 and (t.stride(0) * t.element_size()) % 16 != 0, what
    colsum = torch.zeros(N, device=DEV, dtype=colsum_dtype) if f.colsum else None
    fmt = E5M2 if f.mode == PF.EPI_BWD else E4M3
    o8 = o8_base = qs = amax = None
    rule8, q8 = OUT8_Q[fmt], OUT8_Q[fmt][q8]
    if f.out8:
        o8, o8_base = framed(M, N, fmt, strided)
        qs, amax = torch.tensor([q8], device=DEV), torch.zeros(1, device=DEV)

    PF.gemm(a, a_kc, b, b_kc, c, bias=bias, aux=aux_v, colsum=colsum, mode=f.mode, epi=epi, alpha=k_alpha,
            accumulate=f.accumulate, idx_ld=idx_ld, force_generic=force_generic, mask=mask if not force_generic else None,
            out8=o8, out8_qscale=qs, amax=amax, no_split=no_split, store_c=store_c, engine=engine, cus=cus, **scales)
    name = PF.gemm_last_kernel()
    torch.cuda.synchronize()

    exact = f.act in (NONE, RELU) and (not f.drop or p in (0.5, 1.0))
    total = (scale if f.pre else 1.0) * (scale if f.post else 1.0)
    g_abs = (z * alpha).abs()
    # fp64 math: the per-element bound of each non-exact group, and one rounding of x to the output
    # type on top, |fl(x) - ref| <= |x - ref| + u_out |x|
    u_out = {BF16: 2.0 ** -8, F32: U32, F64: 0.0}[out_dtype] * (1 + 2.0 ** -40)
    elem64 = None
    if f64 and not exact:
        if f.act in (NONE, RELU):
            elem64 = 4 * U64 * ref.abs()
            if out_dtype == F64:
                assert ((reference(torch.tensor(scale, dtype=F32).item())[0] - ref).abs() > elem64).any(), what
        elif f.mode == PF.EPI_FWD:
            elem64 = F64_FWD_ACT_ULPS * U64 * ref.abs()
        else:
            assert aux.dtype == F64 and (aux.abs() * (1.0 - p if f.post else 1.0) <= 1).all(), what
            elem64 = F64_BWD_ACT_ULPS * U64 * g_abs * total
    if not store_c:
        assert (c_base.float() == 7.0).all(), what
        y = ref.float().to(out_dtype)  # (store_c = False runs at p = 0.5 only: the stored value is known)
        assert exact
    else:
        y = c
        if exact:
            assert_gemm_exact(c, ref)
        elif f.act in (NONE, RELU):  # p = 0.3: the zero pattern is exact, kept values carry the scale's rounding
            assert torch.isfinite(c).all(), what
            assert torch.equal(c == 0, ref == 0), what
            if f64:
                within(c, ref, elem64 + u_out * ref.abs(), "scaled64 " + what)
            else:
                within(c, ref, 2.0 ** -8 * ref.abs() if out_dtype == BF16 else 4 * U32 * ref.abs(), "scaled " + what)
        elif f.mode == PF.EPI_FWD:
            if f64:
                if out_dtype == F64:
                    ulps = ((c - ref).abs() / (U64 * ref.abs().clamp_min(1e-300))).max().item()
                    print(f"fwd_act64 {what}: worst |err| / (2^-53 max(|ref|, tiny)) = {ulps:.3f}")
                within(c, ref, elem64 + u_out * ref.abs(), "fwd_act64 " + what)
            else:
                within(c, ref, (2.0 ** -8 if out_dtype == BF16 else 1e-5) * ref.abs() + 1e-5, "fwd_act " + what)
            if kq is not None:
                assert (c[~kq] == 0).all(), what
        else:
            if f64:
                bound = elem64 + u_out * ref.abs()
            else:
                bound = 1e-5 * ref.abs() + 4 * U32 * g_abs * total + (2.0 ** -8 * ref.abs() if out_dtype == BF16 else 0.0)
            within(c, ref, bound, ("bwd_act64 " if f64 else "bwd_act ") + what)
            assert (c[~(kp & kq)] == 0).all(), what
        assert frame_untouched(c, c_base), what
    if aux_v is not None:
        assert frame_untouched(aux_v, aux_base) and torch.equal(aux_v, aux), what
    if colsum is not None:
        abs_sum = ref.abs().sum(0)
        u_cs = U64 if colsum_dtype == F64 else U32
        if exact:
            # every partial sum is exact in the colsum's type (and in the fp64 kernels' fp64 partial sums)
            assert abs_sum.max().item() / min(alpha, 1.0) < (2 ** 53 if colsum_dtype == F64 else 2 ** 24)
            assert torch.equal(colsum.double(), cs_ref), (what, (colsum.double() - cs_ref).abs().max().item())
        elif f64:
            within(colsum, cs_ref, M * u_cs * abs_sum + elem64.sum(0), "colsum64 " + what)
        elif f.act in (NONE, RELU):
            within(colsum, cs_ref, (M + 3) * U32 * abs_sum, "colsum_scaled " + what)
        else:
            elem = 1e-5 * ref.abs() + 4 * U32 * g_abs * total
            within(colsum, cs_ref, M * U32 * abs_sum + elem.sum(0), "colsum_act " + what)
    if mask is not None and f.mode == PF.EPI_FWD:
        assert torch.equal(PF.relu_mask_bits(mask, M, N), y.float() > 0), what
        if M % 256:  # rows >= M of the last 256-row block are not the kernel's to write
            rows, mld = mask.shape
            assert (mask.reshape(rows // 256, mld // 32, 256, 32)[-1, :, M % 256:, :] == 0xAB).all(), what
    if o8 is not None:
        v8 = y.double().abs() * q8
        if q8 == rule8["sub"]:
            assert ((v8 >= rule8["tiny"]) & (v8 < rule8["normal"])).any(), what
        if q8 == rule8["sat"]:
            assert (v8 > rule8["top"]).any(), what
        if store_c:  # (store_c = False: the caller compares the codes with the storing run's)
            fp8_codes_equal(o8, y, q8, fmt)
        assert amax.item() == y.float().abs().max().item(), what
        assert frame_untouched(o8, o8_base), what
    neg0 = int(((c == 0) & torch.signbit(c)).sum()) if store_c else 0
    return SimpleNamespace(name=name, c=c, mask=mask, out8=o8, amax=amax, colsum=colsum, neg0=neg0)


def run_form(cls, form, **kw):
    """Every dropout probability of ``form`` at shape class ``cls``; returns the p = 0.5 (first) result."""
    first = None
    for p in FORMS[form].p:
        r = run_case(SHAPES[cls], form, p, **kw)
        print(f"{cls} {form} p={p}: {r.name}, -0 stored: {r.neg0}")
        first = first or r
    return first


# ------------------------------------------------------------------------------------ the tiled path
FWD_CLASSES = ["S128", "S256x128", "S256", "Ssplit"]
TABLE = ([(c, f) for c in FWD_CLASSES for f in FWD_FORMS] +
         [("S256rN", f) for f in ("none_pre", "relu_post", "relu_prepost", "relu_pre", "store_bias", "relu_prepost_out8")] +
         [(c, f) for c in ("S256rM", "S256k96", "SsplitrM") for f in ("plain", "relu_prepost", "tanh_prepost", "dx_relu_mask")] +
         [(c, f) for c in ("S128", "S256x128", "S256", "S256k128", "Ssplit") for f in DX_FORMS] +
         [(c, f) for c in ("S128", "S256x128", "S256", "Ssplit") for f in DW_FORMS] +
         [(c, f) for c in ("S128", "S256") for f in ("tn_bf16", "tn_f32")])


@pytest.mark.parametrize("cls,form", TABLE, ids=[f"{c}-{f}" for c, f in TABLE])
def test_tiled_gemm_is_exact(native_lib, cls, form):
    r = run_form(cls, form)
    assert r.name == expected_kernel(cls, form)


@pytest.mark.parametrize("cls,form", [(c, f) for c in ("S128", "S256", "Ssplit")
                                      for f in ("relu_prepost_out8", "relu_nodrop_out8", "dx_relu_mask_out8")])
def test_store_c_false_writes_only_the_side_outputs(native_lib, cls, form):
    """store_c = False: C untouched, the fp8 copy, amax, bitmask and column sums identical."""
    full = run_case(SHAPES[cls], form)
    side = run_case(SHAPES[cls], form, store_c=False)
    assert side.name == full.name == expected_kernel(cls, form)
    assert torch.equal(side.out8.view(torch.uint8), full.out8.view(torch.uint8)) and torch.equal(side.amax, full.amax)
    if FORMS[form].mode == PF.EPI_FWD:
        assert torch.equal(side.mask, full.mask)
    else:
        assert torch.equal(side.colsum, full.colsum)


@pytest.mark.parametrize("form", ["plain", "relu_prepost", "relu_pre", "dx_relu_mask", "dw_f32_acc"])
def test_no_split_runs_the_skinny_shape_as_128_tiles(native_lib, form):
    r = run_form("Ssplit", form, no_split=True)
    assert r.name == expected_kernel("Ssplit", form, no_split=True)


@pytest.mark.parametrize("cls", ["S128", "S256"])
@pytest.mark.parametrize("form", ["relu_prepost_out8", "dx_relu_mask_out8", "dx_relu_aux"])
def test_strided_views_write_nothing_outside_the_slice(native_lib, cls, form):
    """A, B, C, aux and out8 as column slices [rows, 8 : 8 + width] of wider tensors filled with 7
    (C and out8 with 8 more rows below): the contiguous call's results, and every element outside
    the slices still 7 (run_case checks the frames)."""
    flat = run_case(SHAPES[cls], form)
    view = run_case(SHAPES[cls], form, strided=True)
    assert view.name == flat.name == expected_kernel(cls, form)
    assert view.c.stride(0) == SHAPES[cls][1] + 16 and torch.equal(view.c, flat.c)
    if view.out8 is not None:
        assert torch.equal(view.out8.contiguous().view(torch.uint8), flat.out8.view(torch.uint8))
        assert torch.equal(view.amax, flat.amax)
    if view.colsum is not None:
        assert torch.equal(view.colsum, flat.colsum)
    if view.mask is not None:
        assert torch.equal(view.mask, flat.mask)


@pytest.mark.parametrize("cls", ["S128", "S256"])
@pytest.mark.parametrize("form", ["relu_prepost", "dx_relu_aux"])
def test_idx_ld_strides_the_dropout_element_index(native_lib, cls, form):
    N = SHAPES[cls][1]
    r = run_case(SHAPES[cls], form, idx_ld=N + 64)
    assert r.name == expected_kernel(cls, form)
    assert not torch.equal(r.c, run_case(SHAPES[cls], form).c)


# ------------------------------------------------------------------------------------ generic kernel
GENERIC = (67, 45, 23)
GENERIC_FORMS = ([f for f in FWD_FORMS if not FORMS[f].out8] + ["fwd_acc", "dx_plain", "dx_store_colsum", "dx_relu_aux",
                 "dx_sigmoid_aux", "dx_tanh_aux", "dw_f32", "dw_f32_acc", "tn_f32"])


GENERIC_TTT = (9, 9, 9)   # the reference project's own tic-tac-toe layers


@pytest.mark.parametrize("in_dtype", [BF16, F32, F64], ids=["bf16", "f32", "f64"])
@pytest.mark.parametrize("form", GENERIC_FORMS)
def test_generic_kernel_is_exact(native_lib, form, in_dtype):
    """gemm_generic.hip at a shape with no aligned dimension: bf16 operands with the form's output
    type, fp32 operands with fp32 outputs (aux in the output type); fp64 operands (the <double, double>
    instantiation, also at the 9-wide shape) with fp64 outputs, bias, aux and column sums."""
    kw = dict(out_dtype=F32) if in_dtype == F32 else {}
    if in_dtype == F64:
        kw = dict(out_dtype=F64, bias_dtype=F64, aux_dtype=F64, colsum_dtype=F64)
    for shape in (GENERIC, GENERIC_TTT) if in_dtype == F64 else (GENERIC,):
        for p in FORMS[form].p:
            r = run_case(shape, form, p, force_generic=True, in_dtype=in_dtype, **kw)
            print(f"generic {shape} {form} p={p}: -0 stored: {r.neg0}")
            assert r.name == "generic/var0/64x64/ek0/split1"


def test_bf16_accumulate_takes_the_generic_kernel(native_lib):
    """bf16 out + accumulate is not MFMA-eligible (mfma_eligible: accumulate needs an fp32 C): the
    VALU kernel runs it, exactly."""
    r = run_case(SHAPES["S128"], "fwd_acc")
    assert r.name == "generic/var0/64x64/ek0/split1"


# ------------------------------------------------------------------------------------ stream-K engine
SK = (1536, 1280, 512)
SK_KIND = {"plain": 1, "dx_plain": 1, "dw_bf16": 1, "dw_f32": 100, "relu_post": 4, "relu_prepost": 5, "none_pre": 6,
           "dx_relu_mask": 3}


@pytest.mark.parametrize("cus", [37, 200])
@pytest.mark.parametrize("form", list(SK_KIND))
def test_stream_k_engine_is_exact(native_lib, form, cus):
    """30 tiles: one workgroup each on a 37-CU budget, two K halves each (the stream-K fold) on 200.
    The fold adds exact integers: it cannot round."""
    for p in FORMS[form].p:
        r = run_case(SK, form, p, engine=2, cus=cus)
        assert r.name == f"sk/var0/256x256/ek{SK_KIND[form]}/split1"

