"""``PF.quantize_cols`` and ``PF.gemm_skinny_w8`` — the column quantiser (csrc/quant_cols.hip) and the
weight-streaming e4m3 GEMM (csrc/gemm_skinny_w8.hip) of weight-only quantised inference:
``out[M,N] = act(scale[n] * (x[M,K] @ W8[K,N]) + bias[n])``, ``1 <= M <= 16``.

The quantiser is checked for EQUALITY against the pure-torch ``PF.quantize_cols_reference``.

The GEMM is checked against fp64 torch on the SAME dequantised weight values with the bound of
``test_skinny_gpu.py``, unchanged. It carries over because a bf16 x e4m3 product has at most 12
significant bits (exact in fp32) and the column scale is a power of two (its multiply is exact): with
``u = 2^-24`` an fp32 sum of K terms in any order is off by at most ``K * u * sum|x_k w_k|``, the
bias is one more term, and with a margin of 2

    |err| <= 2 * (K + 4) * u * ((|x| @ |w_deq|)[m, n] + |bias[n]|)

The activations are 1-Lipschitz; sigmoid / tanh add 1e-5 absolute (the fast exponential), a bf16
output adds ``2^-8 * |ref|`` (one bf16 rounding, with margin 2).
"""
import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACTS = {PF.ACT_NONE: lambda t: t, PF.ACT_RELU: torch.relu, PF.ACT_SIGMOID: torch.sigmoid, PF.ACT_TANH: torch.tanh}

# (M, K, N)
SHAPES = [
    (1, 1, 16),
    (1, 64, 16),
    (3, 77, 80),
    (16, 1000, 272),       # three strips, the last one partial
    (5, 4096, 1024),       # K split across workgroups
    (16, 8192, 64),        # deep K, half a strip
]
VARIANTS = [(False, PF.ACT_NONE), (True, PF.ACT_NONE), (True, PF.ACT_RELU), (True, PF.ACT_SIGMOID),
            (False, PF.ACT_TANH), (True, PF.ACT_TANH)]


def _column_binades(n):
    """A different power of two per column, 2^-6 .. 2^5: a mis-indexed scale cannot hide."""
    return torch.ldexp(torch.ones(n), torch.arange(n, dtype=torch.int32) % 12 - 6)


def _operands(m, k, n, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * m + 7 * k + n)
    x = torch.randn(m, k, generator=g).to(torch.bfloat16).to(DEV)
    w = (0.5 * torch.randn(k, n, generator=g) * _column_binades(n)).to(DEV)
    b = (0.5 * torch.randn(n, generator=g)).to(DEV)
    w8, scale = PF.quantize_cols(w)
    return x, w8, scale, b


def _bound(x, w_deq, b, ref, act, out_dtype):
    k = x.shape[1]
    mag = x.double().abs() @ w_deq.double().abs()
    if b is not None:
        mag = mag + b.double().abs()
    bound = 2.0 * (k + 4) * 2.0 ** -24 * mag
    if act in (PF.ACT_SIGMOID, PF.ACT_TANH):
        bound = bound + 1e-5
    if out_dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * ref.abs()
    return bound


def _special_matrix():
    """[40, 24]: random columns on different binades; an all-zero column (18); amax exactly at (19)
    and one ulp above (20) a scale's limit 448 * 2^-3; amax 1.0 (21); 1.0 mixed with values down to
    2^-12 and a tiny negative (22)."""
    g = torch.Generator().manual_seed(21)
    w = 0.5 * torch.randn(40, 24, generator=g) * _column_binades(24)
    w[:, 18] = 0.0
    limit = torch.tensor(448.0 * 2.0 ** -3)
    for col, top in ((19, limit), (20, torch.nextafter(limit, torch.tensor(1e9)))):
        w[:, col] = 40.0 * torch.rand(40, generator=g) - 20.0
        w[7, col] = -top
    w[:, 21] = torch.rand(40, generator=g) - 0.5
    w[39, 21] = 1.0
    w[:, 22] = torch.ldexp(torch.ones(40), -(torch.arange(40, dtype=torch.int32) % 13))
    w[5, 22] = -1e-30
    w[6, 22] = -(2.0 ** -12)
    return w


def _assert_quantised_as_reference(w_gpu, w_cpu):
    w8, scale = PF.quantize_cols(w_gpu)
    ref8, ref_scale = PF.quantize_cols_reference(w_cpu)
    assert w8.dtype == torch.float8_e4m3fn and w8.shape == w_cpu.shape and w8.is_contiguous()
    assert torch.equal(scale.cpu(), ref_scale)
    got, want = w8.cpu().float() * scale.cpu(), ref8.float() * ref_scale
    assert torch.isfinite(got).all()
    assert (got == want).all(), (got != want).nonzero()[:5]     # as floats: -0 == 0
    return scale


@pytest.mark.parametrize("k,n", [(1, 16), (77, 72), (300, 40), (1000, 272), (33, 7)],
                         ids=lambda v: str(v))
def test_quantiser_equals_the_reference(native_lib, k, n):
    g = torch.Generator().manual_seed(100 * k + n)
    w = 0.5 * torch.randn(k, n, generator=g) * _column_binades(n)
    _assert_quantised_as_reference(w.to(DEV), w)


def test_quantiser_equals_the_reference_on_the_special_columns(native_lib):
    w = _special_matrix()
    scale = _assert_quantised_as_reference(w.to(DEV), w).cpu()
    assert scale[18] == 1.0 and scale[19] == 2.0 ** -3 and scale[20] == 2.0 ** -2 and scale[21] == 2.0 ** -8


def test_quantiser_reads_strided_views_and_refuses_non_finite_weights(native_lib):
    wide = torch.randn(50, 100, generator=torch.Generator().manual_seed(5))
    wide_gpu = wide.to(DEV)
    for c0 in (8, 3):  # a 16-B aligned column slice (8 columns per lane) and a misaligned one (element-wise)
        _assert_quantised_as_reference(wide_gpu[:, c0:c0 + 40], wide[:, c0:c0 + 40].contiguous())
    bad = torch.ones(4, 16, device=DEV)
    bad[2, 3] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        PF.quantize_cols(bad)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["out_f32", "out_bf16"])
@pytest.mark.parametrize("m,k,n", SHAPES, ids=[f"{m}x{k}x{n}" for m, k, n in SHAPES])
def test_matches_fp64_within_the_summation_bound(native_lib, m, k, n, out_dtype):
    x, w8, scale, b = _operands(m, k, n)
    w_deq = w8.float() * scale
    assert len(torch.unique(scale)) > 1 or n == 1
    pre = x.double() @ w_deq.double()
    for has_bias, act in VARIANTS:
        bias = b if has_bias else None
        ref = ACTS[act](pre + b.double() if has_bias else pre)
        out = torch.full((m, n), float("nan"), device=DEV, dtype=out_dtype)
        assert PF.gemm_skinny_w8_eligible(x, w8, scale, out)
        PF.gemm_skinny_w8(x, w8, scale, out, bias=bias, act=act)
        err = (out.double() - ref).abs()
        bound = _bound(x, w_deq, bias, ref, act, out_dtype)
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"({m},{k},{n}) -> {out_dtype} bias={has_bias} act={act}: max err {err.max().item():.3e}, "
              f"max err/bound {worst:.3f}")
        assert torch.isfinite(out).all()
        assert (err <= bound).all(), (has_bias, act, err.max().item(), worst)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_identity_rows_select_rows_of_the_dequantised_matrix_exactly(native_lib, out_dtype):
    """A transposed or mis-strided read, or a scale taken from the wrong column, cannot hide: x picks
    single rows of W and every column has its own scale."""
    k, n = 300, 48
    g = torch.Generator().manual_seed(9)
    w8, scale = PF.quantize_cols((0.5 * torch.randn(k, n, generator=g) * _column_binades(n)).to(DEV))
    w_deq = w8.float() * scale
    rows = torch.tensor([0, 299, 17, 256, 31])
    x = torch.zeros(len(rows), k)
    x[torch.arange(len(rows)), rows] = 1.0
    x = x.to(torch.bfloat16).to(DEV)
    out = torch.empty(len(rows), n, device=DEV, dtype=out_dtype)
    PF.gemm_skinny_w8(x, w8, scale, out)
    assert torch.equal(out.float(), w_deq[rows.to(DEV)])


def test_strided_views_are_read_and_written_in_place(native_lib):
    """Eligible views: x with a leading dimension beyond K, W8 a 16-B aligned column slice, out a
    column slice; the bytes around out stay untouched."""
    m, k, n = 7, 200, 48
    g = torch.Generator().manual_seed(13)
    xf = torch.randn(m, k + 24, generator=g).to(torch.bfloat16).to(DEV)
    w8f, scalef = PF.quantize_cols((0.5 * torch.randn(k, n + 32, generator=g) * _column_binades(n + 32)).to(DEV))
    x, w8, scale = xf[:, 8:8 + k], w8f[:, 16:16 + n], scalef[16:16 + n].contiguous()
    of = torch.full((m, n + 5), -7.0, device=DEV)
    out = of[:, 2:2 + n]
    assert PF.gemm_skinny_w8_eligible(x, w8, scale, out)
    PF.gemm_skinny_w8(x, w8, scale, out)
    w_deq = w8.float() * scale
    ref = x.double() @ w_deq.double()
    assert ((out.double() - ref).abs() <= _bound(x, w_deq, None, ref, PF.ACT_NONE, torch.float32)).all()
    assert (of[:, :2] == -7.0).all() and (of[:, 2 + n:] == -7.0).all()


# (16, 4096, 8192): 512-row slices, so a lane of the narrow buckets sums two batches and one of the
# 16-row bucket sixteen, two turns of its ring; random operands, so the summation order shows
@pytest.mark.parametrize("m,k,n", [(16, 4096, 1024), (16, 77, 80), (16, 4096, 8192)])
def test_same_call_twice_is_bit_identical_and_rows_do_not_depend_on_the_batch(native_lib, m, k, n):
    assert PF.gemm_skinny_w8_plan(k, n)[2] == (512 if n == 8192 else 256)
    x, w8, scale, b = _operands(m, k, n, seed=3)
    out = torch.empty(m, n, device=DEV)
    again = torch.empty(m, n, device=DEV)
    PF.gemm_skinny_w8(x, w8, scale, out, bias=b, act=PF.ACT_TANH)
    PF.gemm_skinny_w8(x, w8, scale, again, bias=b, act=PF.ACT_TANH)
    assert torch.equal(out, again)
    for r in range(m):  # every row alone (M = 1 bucket) against its row of the 16-row call
        one = torch.empty(1, n, device=DEV)
        PF.gemm_skinny_w8(x[r:r + 1], w8, scale, one, bias=b, act=PF.ACT_TANH)
        assert torch.equal(one[0], out[r]), r
    for rows in (2, 3, 8):  # the other buckets too
        part = torch.empty(rows, n, device=DEV)
        PF.gemm_skinny_w8(x[:rows], w8, scale, part, bias=b, act=PF.ACT_TANH)
        assert torch.equal(part, out[:rows]), rows


def test_ineligible_operands_are_refused_and_nothing_is_launched(native_lib):
    def refused(x, w8, scale, out):
        before = out.clone()
        assert not PF.gemm_skinny_w8_eligible(x, w8, scale, out)
        with pytest.raises(RuntimeError, match="not eligible"):
            PF.gemm_skinny_w8(x, w8, scale, out)
        torch.cuda.synchronize()
        assert torch.equal(out, before)

    def e4m3(k, n):
        return torch.ones(k, n, device=DEV).to(torch.float8_e4m3fn)

    bf = dict(device=DEV, dtype=torch.bfloat16)
    ones = lambda n: torch.ones(n, device=DEV)  # noqa: E731
    refused(torch.ones(17, 64, **bf), e4m3(64, 16), ones(16), torch.zeros(17, 16, device=DEV))          # M = 17
    refused(torch.ones(2, 64, **bf), e4m3(64, 48)[:, 8:24], ones(16), torch.zeros(2, 16, device=DEV))   # W8 base + 8 B
    refused(torch.ones(2, 64, **bf), e4m3(64, 24), ones(24), torch.zeros(2, 24, device=DEV))            # N = 24: 24-B rows
    refused(torch.ones(2, 64, **bf), e4m3(64, 24)[:, :16], ones(16), torch.zeros(2, 16, device=DEV))    # W8 rows 24 B apart
    refused(torch.ones(2, 64, device=DEV), e4m3(64, 16), ones(16), torch.zeros(2, 16, device=DEV))      # fp32 x
    ok = (torch.ones(2, 64, **bf), e4m3(64, 16), ones(16), torch.zeros(2, 16, device=DEV))
    assert PF.gemm_skinny_w8_eligible(*ok)
    assert not PF.gemm_skinny_w8_eligible(*(t.cpu() for t in ok))
    before = ok[3].clone()
    for bad_scale in (ones(15), ones(17)):  # a wrong-length scale: a structural error
        assert not PF.gemm_skinny_w8_eligible(ok[0], ok[1], bad_scale, ok[3])
        with pytest.raises(RuntimeError, match="scale"):
            PF.gemm_skinny_w8(ok[0], ok[1], bad_scale, ok[3])
    with pytest.raises(RuntimeError, match="bias"):  # and a wrong-length bias
        PF.gemm_skinny_w8(*ok, bias=ones(8))
    with pytest.raises(RuntimeError, match="float8_e4m3fn"):  # W8 of another dtype
        PF.gemm_skinny_w8(ok[0], torch.ones(64, 16, **bf), ok[2], ok[3])
    torch.cuda.synchronize()
    assert torch.equal(ok[3], before)
