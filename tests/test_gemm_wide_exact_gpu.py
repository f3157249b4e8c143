"""The fp32 / fp64 matrix-core GEMM (csrc/gemm_wide.hip: v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64,
128 x 128 tile, 32-deep K tiles, 4-deep MFMA k-steps) and the generic kernel's <double, double>
instantiation, value for value, with fp64 epilogues.

Method: test_gemm_exact_gpu's, through its run_case. Small integers are exact in fp32 and fp64, so
every accumulation order gives the same z; alpha is a power of two, bias entries are multiples of
1/8, and at p = 0.5 (and 1.0) the whole none / ReLU epilogue is exact: an fp64 C must EQUAL the fp64
reference, an fp32 / bf16 C the reference rounded once, and the column sums the exact sums (fp64
and fp32). The forms that cannot be exact take the bounds run_case's docstring derives: fp32
operands the project's fp32 bounds; fp64 operands 4 u |ref| at p = 0.3 (u = 2^-53; the reference
with an fp32-rounded scale is asserted to break that bound, so the test pins epi_scale<double>),
16 u |g| scale_pre scale_post for sigmoid / tanh backward from an fp64 aux, a measured bound for
sigmoid / tanh forward (the device exp / tanh against torch's fp64 CPU result on the same exact h),
and M u sum|ref| + the per-element bounds for their column sums. Every launch passes engine = 1 and
asserts PF.gemm_last_kernel().

Shape classes (the smallest that reach each branch):
  W_full (384, 640, 64)  15 whole tiles: the XCD remap with q = 1, remainder 7; vector loads; two K tiles
  W_rag  (200, 136, 96)  ragged M and N: the interior tile on vector loads, the edge tiles on element loads
  W_k    (130, 67, 20)   K < 32 and K % 4 != 0 (zero-filled k-steps), one ragged tile column
  W_min  (64, 64, 16)    the smallest eligible problem: a quarter of one tile
  W_row  (1, 4096, 16)   eligible by M N alone: 32 tiles with one live row

Cells reached (kernel x shape class x form group), fp32 and fp64 operands alike:
  wide/var0/128x128/ek0/split1    all five classes x the four layouts, plain store in the operand type
                                  W_rag, W_k x fwd, dw with full-width integers (|a| <= 2^20 fp64, 256 fp32:
                                  K hi^2 = 96 * 2^16 < 2^24)
                                  W_rag, W_full x every form without bitmask / fp8 copy, p in (0.5, 0.3, 1.0),
                                  bias / aux / colsum in the operand type: store + bias, the dropout forms with
                                  no activation, ReLU, sigmoid, tanh, backward from aux, EPI_STORE + colsum,
                                  accumulate with alpha = 1/4 and bias
                                  W_rag x the same forms with: fp64 operands + fp32 bias and colsum; fp32
                                  operands + bf16 aux; fp32 -> bf16 C; fp64 -> fp32 C; fp32 -> fp64 C
                                  W_rag, W_full x plain / relu_prepost / dx_tanh_aux on views whose base and
                                  row stride are no multiple of 16 bytes (element loads on interior tiles)
                                  W_rag x relu_prepost / dx_relu_aux with idx_ld = N + 64
                                  W_rag, W_k x the four layouts with random normal operands (summation bound)
  generic/var0/64x64/ek0/split1   W_rag x every form above, forced, compared with the wide kernel's C and
                                  colsum; (67, 45, 23) and (9, 9, 9) with fp64 operands are
                                  test_gemm_exact_gpu.py::test_generic_kernel_is_exact[*-f64]
  no launch                       gemm_path at the boundary M N >= 64^2 and K >= 16, and force_generic

Full-width integers cannot tell xf32 from fp32 at |a| <= 256 (10 explicit bits hold them); the random
normal run can, and the fp64 run at 2^20 fails under any fp32 or narrower step.

Documented, not a bug: GemmArgs.alpha is a float; every alpha here is a power of two.

Measured on MI355X (368 cases; the file takes about 2.3 s, the slowest case 0.5 s, the first launch):
every kernel name as predicted; every none / ReLU form at p = 0.5 and 1.0 exact in C and in both
column-sum types, in every output type; the wide and the generic kernel equal on them; full-width
integers exact; unaligned views bit for bit with untouched frames. Worst err / bound of the others:
  fp64 operands -> fp64 C   p = 0.3 kept values 0.000 (the kernel's two multiplications round as the
                            reference's do; the fp32-scale reference breaks the bound on every case),
                            sigmoid / tanh backward 0.245 (tanh; sigmoid 0.074), column sums 0.023
  fp64 sigmoid / tanh fwd   worst |err| / (2^-53 |ref|) = 8.001 for tanh, 3.567 for sigmoid, on both
                            kernels: the bound is 4 x 8.001 = 32 (F64_FWD_ACT_ULPS); err / bound 0.25
  fp64 operands -> fp32 C   0.998: the one fp32 rounding of C is the whole bound
  fp32 operands             p = 0.3 kept values 0.966, their column sums 0.005; sigmoid / tanh forward
                            0.965, backward 0.988 with column sums 0.005
  random normal operands    0.069 (fp64) and 0.071 (fp32) of 2 (K + 4) u (|a| @ |b|)
Mutation check (not committed): with epi_scale<double> returning the fp32 scale e.scale, every fp64
case with a dropout at p = 0.3 fails, test_every_epilogue_form[none_pre-W_rag-f64] first at
err / bound 5.4e7.
"""
import functools

import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.helpers import bit_equal
from tests.test_gemm_exact_gpu import F32, F64, BF16, FORMS, LAYOUTS, NONE, RELU, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDE, GENERIC = "wide/var0/128x128/ek0/split1", "generic/var0/64x64/ek0/split1"
W = {"W_full": (384, 640, 64), "W_rag": (200, 136, 96), "W_k": (130, 67, 20), "W_min": (64, 64, 16), "W_row": (1, 4096, 16)}
DTYPES = {"f32": F32, "f64": F64}
FULL_HI = {"f32": 256, "f64": 2 ** 20}
# every form the wide kernel can run: no ReLU bitmask to read, no fp8 copy (the forward forms that
# write a bitmask on the bf16 path run here without one)
WIDE_FORMS = [n for n, f in FORMS.items() if not f.out8 and not (f.mode == PF.EPI_BWD and f.mask)]
# how a run's side tensors are typed: everything in the operand type, and the mixed runs of W_rag
SAME = {"f32": dict(in_dtype=F32, out_dtype=F32, bias_dtype=F32, aux_dtype=F32, colsum_dtype=F32),
        "f64": dict(in_dtype=F64, out_dtype=F64, bias_dtype=F64, aux_dtype=F64, colsum_dtype=F64)}
MIXED = {"f64_bias32_colsum32": dict(SAME["f64"], bias_dtype=F32, colsum_dtype=F32),
         "f32_aux_bf16": dict(SAME["f32"], aux_dtype=BF16),
         "f32_to_bf16": dict(SAME["f32"], out_dtype=BF16),
         "f64_to_f32": dict(SAME["f64"], out_dtype=F32),
         "f32_to_f64": dict(SAME["f32"], out_dtype=F64)}


def is_exact(form, p):
    f = FORMS[form]
    return f.act in (NONE, RELU) and (not f.drop or p in (0.5, 1.0))


def run_all_p(shape, form, kernel=WIDE, **kw):
    """Every dropout probability of ``form``; returns the results by p."""
    out = {}
    for p in FORMS[form].p:
        out[p] = r = run_case(shape, form, p, engine=1, **kw)
        print(f"{shape} {form} p={p}: {r.name}, -0 stored: {r.neg0}")
        assert r.name == kernel, r.name
    return out


# ------------------------------------------------------------------------------------ 1, 2: plain stores
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("cls", list(W))
def test_plain_store_is_exact(native_lib, cls, layout, dt):
    r = run_case(W[cls], "plain", engine=1, layout=layout, in_dtype=DTYPES[dt], out_dtype=DTYPES[dt])
    assert r.name == WIDE


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("layout", ["fwd", "dw"])
@pytest.mark.parametrize("cls", ["W_rag", "W_k"])
def test_full_width_integers_are_exact(native_lib, cls, layout, dt):
    """Operands in [-2^20, 2^20] (fp64: products of 41 bits, sums below 2^47) and [-256, 256] (fp32:
    sums below 96 * 2^16 < 2^24): a bf16 operand path, or an fp32 accumulator under fp64, cannot
    give these values."""
    hi, K = FULL_HI[dt], W[cls][2]
    assert K * hi * hi < (2 ** 53 if dt == "f64" else 2 ** 24)
    r = run_case(W[cls], "plain", engine=1, layout=layout, in_dtype=DTYPES[dt], out_dtype=DTYPES[dt], hi=hi)
    assert r.name == WIDE
    # the inputs do produce wide results: integers of more than fp32's 24 (fp64 run) / bf16's 8 (fp32 run)
    # significand bits. This line pins no precision by itself; the equality above does for bf16 and for
    # fp32 under fp64, and the random normal test below for the fp32 significand (xf32)
    assert r.c.abs().max().item() > (2.0 ** 32 if dt == "f64" else 2.0 ** 16)


# ------------------------------------------------------------------------------------ 3: epilogue forms
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("cls", ["W_rag", "W_full"])
@pytest.mark.parametrize("form", WIDE_FORMS)
def test_every_epilogue_form(native_lib, form, cls, dt):
    run_all_p(W[cls], form, **SAME[dt])


@pytest.mark.parametrize("mix", list(MIXED))
@pytest.mark.parametrize("form", WIDE_FORMS)
def test_every_epilogue_form_with_mixed_types(native_lib, form, mix):
    run_all_p(W["W_rag"], form, **MIXED[mix])


# ------------------------------------------------------------------------------------ 4, 5: views, idx_ld
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("cls", ["W_rag", "W_full"])
@pytest.mark.parametrize("form", ["relu_prepost", "dx_tanh_aux", "plain"])
def test_unaligned_views_take_the_element_loads(native_lib, form, cls, dt):
    """A, B, C and aux as the column slice [rows, 1 : 1 + width] of tensors width + 3 wide (C and aux
    8 rows taller): base 4 / 8 bytes past a 16-byte boundary, row stride no multiple of 16 bytes
    (run_case asserts both), so Stage::load takes its element path on interior tiles too. The
    contiguous call's values bit for bit, every element outside C and aux still the fill."""
    flat = run_case(W[cls], form, engine=1, **SAME[dt])
    view = run_case(W[cls], form, engine=1, strided=True, pad=1, odd=1, **SAME[dt])
    assert view.name == flat.name == WIDE
    assert view.c.stride(0) == W[cls][1] + 3 and bit_equal(view.c.contiguous(), flat.c)
    if view.colsum is not None and is_exact(form, 0.5):
        assert torch.equal(view.colsum, flat.colsum)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("form", ["relu_prepost", "dx_relu_aux"])
def test_idx_ld_strides_the_dropout_element_index(native_lib, form, dt):
    N = W["W_rag"][1]
    r = run_case(W["W_rag"], form, engine=1, idx_ld=N + 64, **SAME[dt])   # (the reference's masks use that stride)
    assert r.name == WIDE
    assert not torch.equal(r.c, run_case(W["W_rag"], form, engine=1, **SAME[dt]).c)


# ------------------------------------------------------------------------------------ 6: dispatch
@pytest.mark.parametrize("dt", list(DTYPES))
def test_dispatch_boundary(native_lib, dt):
    """wide_eligible: M N >= 64 * 64 and K >= 16, unless force_generic. Nothing is launched."""
    def path(M, N, K, **kw):
        a, b = torch.empty(M, K, device=DEV, dtype=DTYPES[dt]), torch.empty(K, N, device=DEV, dtype=DTYPES[dt])
        return PF.gemm_path(a, True, b, False, torch.empty(M, N, device=DEV, dtype=DTYPES[dt]), **kw)

    assert path(64, 64, 16) == "mfma_wide" and path(1, 4096, 16) == "mfma_wide"
    assert path(64, 64, 15) == "generic" and path(63, 65, 16) == "generic"
    assert path(64, 64, 16, force_generic=True) == "generic" and path(384, 640, 64, force_generic=True) == "generic"


# ------------------------------------------------------------------------------------ 7: wide vs generic
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("form", WIDE_FORMS)
def test_wide_and_generic_kernels_agree(native_lib, form, dt):
    """Both kernels against the reference at W_rag; on the exact forms that makes their C and their
    column sums equal, which is asserted too."""
    wide = run_all_p(W["W_rag"], form, **SAME[dt])
    generic = run_all_p(W["W_rag"], form, kernel=GENERIC, force_generic=True, **SAME[dt])
    for p in FORMS[form].p:
        if is_exact(form, p):
            assert torch.equal(wide[p].c, generic[p].c), (form, p)
            if wide[p].colsum is not None:
                assert torch.equal(wide[p].colsum, generic[p].colsum), (form, p)


# ------------------------------------------------------------------------------------ 9: full mantissas
@functools.lru_cache(maxsize=None)
def normal_operands(M, N, K, a_kc, b_kc):
    g = torch.Generator(device="cpu").manual_seed(M + 3 * N + 7 * K + 2 * a_kc + b_kc)
    a = torch.randn((M, K) if a_kc else (K, M), generator=g, dtype=F64)
    b = torch.randn((N, K) if b_kc else (K, N), generator=g, dtype=F64)
    return a, b


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("cls", ["W_rag", "W_k"])
def test_random_normal_operands_within_the_summation_bound(native_lib, cls, layout, dt):
    """Full-mantissa operands: a sum of K products in ANY order is off by at most K u sum|a_k b_k|
    (tests/test_skinny_gpu.py's derivation; the fp64 host reference has the same bound), with a
    margin of 2: |err| <= 2 (K + 4) u (|a| @ |b|)[m, n], u = 2^-24 / 2^-53."""
    (M, N, K), (a_kc, b_kc), dtype = W[cls], LAYOUTS[layout], DTYPES[dt]
    a64, b64 = normal_operands(M, N, K, a_kc, b_kc)
    a, b = a64.to(dtype), b64.to(dtype)               # the values the kernel multiplies
    A = a.double() if a_kc else a.double().t()
    B = b.double().t() if b_kc else b.double()
    ref, mag = A @ B, A.abs() @ B.abs()
    c = torch.full((M, N), float("nan"), device=DEV, dtype=dtype)
    PF.gemm(a.to(DEV), a_kc, b.to(DEV), b_kc, c, engine=1)
    assert PF.gemm_last_kernel() == WIDE
    got = c.cpu().double()
    assert torch.isfinite(got).all()
    u = 2.0 ** -24 if dtype == F32 else 2.0 ** -53
    err, bound = (got - ref).abs(), 2 * (K + 4) * u * mag
    print(f"normal {cls} {layout} {dt}: worst err/bound {(err / bound).max().item():.4f}")
    assert (err <= bound).all(), (err / bound).max().item()
