"""The fp8 GEMMs (choose_fp8 in csrc/gemm_dispatch.h; csrc/gemm_mfma.hip: VAR 8, 9, 14, 15, 16, 17; VAR 43 in csrc/gemm_w4.h),
value for value, on every dispatch cell and epilogue form.

Method: test_gemm_exact_gpu's, through its run_case. The operands hold integers in [-4, 4] (exact in
e4m3 and in e5m2), the dequantisation scales are 2^-2 and 2^-6, and the kernel's alpha is raised by
2^8 so that every form sees the values of the bf16 run: bias in multiples of 1/8, dropout at p = 0.5
exact and at p = 0.3 with an exact zero pattern and kept values within 2^-8 |ref|, sigmoid / tanh
within that file's bounds. Every launch asserts PF.gemm_last_kernel().

The probe (test_f8f6f4_mfma_sums_small_integers_exactly, first in the file) settles what nobody had
measured: v_mfma_scale_f32_32x32x64_f8f6f4 sums such products exactly. Measured on MI355X: VAR 14 and
VAR 8 on one 256 x 256 output at K = 64 and K = 4096 (and VAR 15, and K = 8192) store bf16_rne(z 2^-8)
in every element. So every none / ReLU form below asserts equality (assert_gemm_exact), exact fp32
column sums, exact mask bits, the out8 bytes of fp8_encode_reference and amax = max |bf16 y| (the
epilogue takes it from the stored bf16 values, as the bf16 kernels do).

The fp8 copy runs at three factors: 2^-3 (the bf16 test's; e4m3 saturates there), "sat" (e5m2: 2^8,
some |y| q pass 57344) and "sub" (2^-8 / 2^-16: some outputs land on subnormal codes).

Dispatch cells, as gemm_last_kernel() named them on MI355X (all as read from gemm_choose (choose_fp8), fp8_eligible,
f8_two_wg, gemm_split and w4_shape_ok; no shape of the plan had to change):
  mfma/var8/128x128/ek0|2/split1    e4m3 x e4m3, both K-contiguous, (200, 136, 192): every forward form
  mfma/var8/256x256/ek0|2/split1    (4096, 3840, 64) and ragged (4088, 3832, 64); the fixed kinds run as ek2
  mfma/var9/128x128|256x256/ek0|3   e5m2 x e4m3 dX at the same shapes: bitmask and aux backward
  mfma/var17/256x128/ek0|3/split1   the same at 480 tiles, (5120, 6144, 64) and ragged M (5112, ...)
  mfma/var15/256x256/ek0|2|4|5|6    e4m3 x e4m3 [in, out], (512, 256, 320) and (4096, 3840, 64)
  mfma/var15/256x256/ek0|5/split4   (1536, 2560, 4096) and ragged M (1528, ...); no_split: split1
  mfma/var16/256x128/ek2|4|5|6      (5120, 6144, 64)
  w4/var43/256x256/ek1/split1       (4096, 3840, 2048) plain; K = 1920 stays on mfma/var15/256x256/ek0
  mfma/var14/256x256/ek1/split1|4|8 e4m3^T x e5m2 dW: (256, 256, 64), (512, 768, 320), (1536, 2560, 4096)
                                    split 4, (1536, 1280, 8192) split 8; no_split: split1
Not reached: an fp8 GEMM with a K-contiguous B never splits (gemm_split returns 1 for it), so VAR 8 / 9
have no split-K cell; test_kernels_gpu.py::test_gemm_fp8_split_k runs mfma/var8/128x128/ek2/split1.

Measured on MI355X (the file takes about 15 s; the slowest case, v9 at (5120, 6144, 64) with its four
keep masks, 2 s): the probe exact, every kernel name above as predicted, every none / ReLU form at
p = 0.5 and 1.0 exact with exact column sums, mask bits, out8 bytes and amax. Worst err / bound of the
bounded forms: p = 0.3 kept values 0.981 (one bf16 rounding reaches the bound, as in the bf16 test),
their column sums 0.005; sigmoid / tanh forward 0.991, backward 0.993 with column sums 0.002.
"""
import functools

import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.helpers import assert_gemm_exact, exact_operands_fp8, fp8_all_codes, gemm_split_plan
from tests.test_gemm_exact_gpu import DX_FORMS, FORMS, FWD_FORMS, epi_kind, run_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2

# cell -> (operand layout of test_gemm_exact_gpu.LAYOUTS, (format of A, format of B))
CELLS = {"v8": ("dx", (E4M3, E4M3)), "v9": ("dx", (E5M2, E4M3)), "v15": ("fwd", (E4M3, E4M3)),
         "v14": ("dw", (E4M3, E5M2))}
S128 = (200, 136, 192)
S256, S256R = (4096, 3840, 64), (4088, 3832, 64)
S2WG, S2WGR = (5120, 6144, 64), (5112, 6144, 64)
S15, S15SPLIT, S15SPLITR = (512, 256, 320), (1536, 2560, 4096), (1528, 2560, 4096)
SW4, SW4SHORT = (4096, 3840, 2048), (4096, 3840, 1920)
BWD_FORMS = [f for f in DX_FORMS if FORMS[f].mode == PF.EPI_BWD]   # e5m2 operands take backward stages only


def expected_kernel(cell, shape, form, no_split=False):
    """gemm_last_kernel() of an fp8 launch, read off gemm_choose (csrc/gemm_dispatch.h: choose_fp8)."""
    M, N, K = shape
    ek = epi_kind(FORMS[form])
    t256 = -(-M // 256) * -(-N // 256)
    split = 1 if no_split else gemm_split_plan(M, N, K, fp8=True, b_kc=cell in ("v8", "v9"))
    if cell == "v14":
        return f"mfma/var14/256x256/ek1/split{split}"
    two_wg = split == 1 and t256 >= 480 and N % 128 == 0
    if cell == "v15":
        if ek == 1 and K >= 2048 and K % 128 == 0 and M % 256 == 0 and t256 >= 240 and split == 1:
            return "w4/var43/256x256/ek1/split1"
        kind = ek if ek in (2, 4, 5, 6) else 0
        return f"mfma/var16/256x128/ek{kind}/split1" if two_wg else f"mfma/var15/256x256/ek{kind}/split{split}"
    if cell == "v9":
        kind = 3 if ek == 3 else 0
        if two_wg:
            return f"mfma/var17/256x128/ek{kind}/split1"
    else:
        kind = 2 if ek in (2, 4, 5, 6) else 0   # the fixed kinds run the ReLU-stage kind here
    return f"mfma/var{cell[1:]}/{'256x256' if t256 >= 240 else '128x128'}/ek{kind}/split1"


def run_cell(cell, shape, form, **kw):
    """Every dropout probability of ``form``; returns the p = 0.5 (first) result."""
    layout, fmts = CELLS[cell]
    first = None
    for p in FORMS[form].p:
        r = run_case(shape, form, p, layout=layout, fmts=fmts, **kw)
        print(f"{cell} {shape} {form} p={p}: {r.name}, -0 stored: {r.neg0}")
        assert r.name == expected_kernel(cell, shape, form, kw.get("no_split", False)), r.name
        first = first or r
    return first


# ------------------------------------------------------------------------------------ the probe
@pytest.mark.parametrize("K", [64, 4096])
@pytest.mark.parametrize("cell,name", [("v14", "mfma/var14/256x256/ek1/split1"), ("v8", "mfma/var8/128x128/ek0/split1")])
def test_f8f6f4_mfma_sums_small_integers_exactly(native_lib, cell, name, K):
    """One 256 x 256 output, plain store, scales 2^-2 and 2^-6: every element is bf16_rne(z 2^-8)."""
    layout, fmts = CELLS[cell]
    a_kc = b_kc = layout == "dx"
    a, b, z = exact_operands_fp8(256, 256, K, a_kc, b_kc, *fmts, seed=K)
    c = torch.full((256, 256), float("nan"), device=DEV, dtype=BF16)
    PF.gemm(a.to(DEV), a_kc, b.to(DEV), b_kc, c, scale_a=torch.tensor([0.25], device=DEV),
            scale_b=torch.tensor([2.0 ** -6], device=DEV), engine=1)
    assert PF.gemm_last_kernel() == name
    assert z.abs().max() > 128   # more than a bf16 significand: the rounding is part of what is compared
    assert_gemm_exact(c.cpu(), z * 2.0 ** -8)


# ------------------------------------------------------------------------------------ the cells
SOME_FWD = ["plain", "relu_nodrop", "relu_prepost", "none_pre", "tanh_prepost", "relu_prepost_out8"]
KINDS_15 = ["plain", "store_bias", "none_nodrop", "relu_nodrop", "relu_post", "relu_prepost", "none_pre"]
TABLE = ([("v8", S128, f) for f in FWD_FORMS] +
         [("v8", s, f) for s in (S256, S256R) for f in SOME_FWD] +
         [("v9", s, f) for s in (S128, S256) for f in BWD_FORMS] +
         [("v9", s, f) for s in (S2WG, S2WGR) for f in ("dx_relu_mask", "dx_relu_aux")] +
         [("v15", s, f) for s in (S15, S256) for f in KINDS_15 + ["relu_prepost_out8", "sigmoid_prepost"]] +
         [("v15", s, f) for s in (S15SPLIT, S15SPLITR) for f in ("plain", "relu_prepost")] +
         [("v15", S2WG, f) for f in ("relu_nodrop", "relu_post", "relu_prepost", "none_pre")] +
         [("v15", SW4, "plain"), ("v15", SW4SHORT, "plain")] +
         [("v14", s, "dw_bf16") for s in ((256, 256, 64), (512, 768, 320), S15SPLIT, (1536, 1280, 8192))])


def case_id(cell, shape, form):
    return f"{cell}-{'x'.join(map(str, shape))}-{form}"


@pytest.mark.parametrize("cell,shape,form", TABLE, ids=[case_id(*t) for t in TABLE])
def test_fp8_gemm_is_exact(native_lib, cell, shape, form):
    run_cell(cell, shape, form)


def test_table_reaches_every_cell():
    """The kernel names the table expects (each launch asserts its own) cover the dispatch of gemm_choose for fp8 operands (choose_fp8)."""
    names = {expected_kernel(*t) for t in TABLE}
    want = {f"mfma/var8/{t}/ek{k}/split1" for t in ("128x128", "256x256") for k in (0, 2)}
    want |= {f"mfma/var9/{t}/ek{k}/split1" for t in ("128x128", "256x256") for k in (0, 3)}
    want |= {f"mfma/var17/256x128/ek{k}/split1" for k in (0, 3)}
    want |= {f"mfma/var15/256x256/ek{k}/split1" for k in (0, 2, 4, 5, 6)}
    want |= {"mfma/var15/256x256/ek0/split4", "mfma/var15/256x256/ek5/split4", "w4/var43/256x256/ek1/split1"}
    want |= {f"mfma/var16/256x128/ek{k}/split1" for k in (2, 4, 5, 6)}
    want |= {f"mfma/var14/256x256/ek1/split{s}" for s in (1, 4, 8)}
    assert want <= names, want - names
    assert expected_kernel("v15", SW4SHORT, "plain") == "mfma/var15/256x256/ek0/split1"


@pytest.mark.parametrize("cell,shape,form,q8", [
    ("v8", S128, "relu_prepost_out8", "sub"), ("v8", S256R, "relu_prepost_out8", "sub"),
    ("v15", S15, "relu_prepost_out8", "sub"),      # (e4m3 saturates at the table's factor 2^-3 already)
    ("v9", S128, "dx_relu_mask_out8", "sub"), ("v9", S128, "dx_relu_mask_out8", "sat"),
    ("v9", S256, "dx_relu_mask_out8", "sub"), ("v9", S256, "dx_relu_mask_out8", "sat")])
def test_fp8_copy_saturates_and_reaches_subnormal_codes(native_lib, cell, shape, form, q8):
    run_cell(cell, shape, form, q8=q8)


@pytest.mark.parametrize("cell,shape,form", [("v8", S128, "relu_prepost_out8"), ("v8", S256, "relu_nodrop_out8"),
                                             ("v15", S15, "relu_prepost_out8"), ("v9", S128, "dx_relu_mask_out8"),
                                             ("v9", S256, "dx_relu_mask_out8")])
def test_fp8_store_c_false_writes_only_the_side_outputs(native_lib, cell, shape, form):
    """store_c = False: C untouched, the fp8 copy, amax, bitmask and column sums identical."""
    full = run_cell(cell, shape, form)
    side = run_cell(cell, shape, form, store_c=False)
    assert torch.equal(side.out8.view(torch.uint8), full.out8.view(torch.uint8)) and torch.equal(side.amax, full.amax)
    if FORMS[form].mode == PF.EPI_FWD:
        assert torch.equal(side.mask, full.mask)
    else:
        assert torch.equal(side.colsum, full.colsum)


@pytest.mark.parametrize("cell,shape,form", [("v15", S15SPLIT, "plain"), ("v15", S15SPLIT, "relu_prepost"),
                                             ("v14", S15SPLIT, "dw_bf16"), ("v14", (1536, 1280, 8192), "dw_bf16")])
def test_fp8_no_split_runs_one_pass(native_lib, cell, shape, form):
    assert run_cell(cell, shape, form, no_split=True).name.endswith("/split1")


@pytest.mark.parametrize("cell,shape,form", [("v8", S128, "relu_prepost_out8"), ("v9", S128, "dx_relu_mask_out8"),
                                             ("v9", S128, "dx_relu_aux"), ("v9", S256, "dx_relu_mask_out8"),
                                             ("v15", S15, "relu_prepost_out8"), ("v14", (512, 768, 320), "dw_bf16")])
def test_fp8_strided_views_write_nothing_outside_the_slice(native_lib, cell, shape, form):
    """A and B as 16-byte aligned column slices [rows, 16 : 16 + width] of tensors 32 bytes wider, C,
    aux and out8 as slices [rows, 8 : 8 + N] of tensors 16 columns wider and 8 rows taller, all filled
    with 7: the contiguous call's results, every element outside the slices still 7 (run_case checks
    the frames), and the bitmask rows past M still the 0xAB they were filled with."""
    flat = run_cell(cell, shape, form)
    view = run_cell(cell, shape, form, strided=True)
    assert view.c.stride(0) == shape[1] + 16 and torch.equal(view.c, flat.c)
    if view.out8 is not None:
        assert torch.equal(view.out8.contiguous().view(torch.uint8), flat.out8.view(torch.uint8))
        assert torch.equal(view.amax, flat.amax)
    if view.colsum is not None:
        assert torch.equal(view.colsum, flat.colsum)
    if view.mask is not None:
        assert torch.equal(view.mask, flat.mask)


# ------------------------------------------------------------------------------------ every code
@functools.lru_cache(maxsize=None)
def code_matrix(fmt):
    """[256, 256] of ``fmt`` cycling through every finite code, and its fp64 values."""
    codes, values = fp8_all_codes(fmt)
    idx = torch.arange(256 * 256) % len(codes)
    return codes[idx].reshape(256, 256).view(fmt).to(DEV), values[idx].reshape(256, 256).to(DEV)


@pytest.mark.parametrize("codes_in", ["b", "a"])
@pytest.mark.parametrize("cell,name", [("v8", "mfma/var8/128x128/ek0/split1"), ("v9", "mfma/var9/128x128/ek3/split1"),
                                       ("v15", "mfma/var15/256x256/ek0/split1"), ("v14", "mfma/var14/256x256/ek1/split1")])
def test_every_finite_code_passes_through_the_mfma(native_lib, cell, name, codes_in):
    """M = N = K = 256. One operand is the identity (a single 1.0 per row, at distinct k), the other
    cycles through all finite codes of its format (both signs, zeros, subnormals, the maximum; no
    NaN): with unit scales the bf16 output holds the selected code values themselves (both formats
    fit bf16), each element of the code matrix exactly once."""
    layout, (fmt_a, fmt_b) = CELLS[cell]
    a_kc, b_kc = {"dx": (True, True), "fwd": (True, False), "dw": (False, False)}[layout]
    fmt = fmt_b if codes_in == "b" else fmt_a
    mat, val = code_matrix(fmt)                      # logical [row, k] of the operand that holds the codes
    eye = torch.eye(256, device=DEV).to(fmt_a if codes_in == "b" else fmt_b)
    if codes_in == "b":                              # C[m, n] = B[n, m]
        a, b, ref = eye, (mat if b_kc else mat.t().contiguous()), val.t()
    else:                                            # C[m, n] = A[m, n]
        a, b, ref = (mat if a_kc else mat.t().contiguous()), eye, val
    c = torch.full((256, 256), float("nan"), device=DEV, dtype=BF16)
    one = torch.ones(1, device=DEV)
    if cell == "v9":   # e5m2 gradients run backward stages only: a ReLU bitmask of ones, no dropout
        mask = PF.relu_mask_pack(torch.ones(256, 256, dtype=torch.bool, device=DEV))
        PF.gemm(a, a_kc, b, b_kc, c, mode=PF.EPI_BWD, epi=PF.epi_spec(PF.ACT_RELU), mask=mask, scale_a=one, scale_b=one,
                engine=1)
    else:
        PF.gemm(a, a_kc, b, b_kc, c, scale_a=one, scale_b=one, engine=1)
    assert PF.gemm_last_kernel() == name
    assert len(torch.unique(ref)) == len(fp8_all_codes(fmt)[0]) - 1   # every value; +0 and -0 are one
    assert_gemm_exact(c, ref)
