"""``PF.gemm_skinny`` — the forward-only weight-streaming GEMM of the inference path
(csrc/gemm_skinny.hip): ``out[M,N] = act(x[M,K] @ W[K,N] + bias)``, ``1 <= M <= 16``.

Numerics are checked against fp64 torch on the SAME bf16 / fp32 operand values. Bound per element,
with ``u = 2^-24`` for bf16 operands (their products are exact in fp32) and ``2^-23`` for fp32
operands (each product rounds once more): an fp32 sum of K terms in ANY order is off by at most
``K * u * sum|x_k w_k|``; the bias is one more term of that sum (its fp32 add rounds once), so its
magnitude joins the sum's. With a margin of 2:

    |err| <= 2 * (K + 4) * u * ((|x| @ |w|)[m, n] + |bias[n]|)

The activations are 1-Lipschitz, so the bound carries through them; sigmoid / tanh add 1e-5
absolute (the fast exponential), a bf16 output adds ``2^-8 * |ref|`` (one bf16 rounding, with
margin 2).
"""
import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ACTS = {PF.ACT_NONE: lambda t: t, PF.ACT_RELU: torch.relu, PF.ACT_SIGMOID: torch.sigmoid, PF.ACT_TANH: torch.tanh}

# (M, K, N, operand dtype)
SHAPES = [
    (1, 1, 8, torch.bfloat16),
    (1, 64, 8, torch.bfloat16),
    (3, 77, 72, torch.bfloat16),
    (16, 1000, 264, torch.bfloat16),
    (5, 4096, 1024, torch.bfloat16),     # K split across workgroups
    (16, 8192, 64, torch.bfloat16),      # deep K, few columns
    (2, 130, 4, torch.float32),
    (9, 600, 36, torch.float32),         # fp32 with K split across workgroups, two strips
]
# (bias, act): bias present and absent, each activation
VARIANTS = [(False, PF.ACT_NONE), (True, PF.ACT_NONE), (True, PF.ACT_RELU), (True, PF.ACT_SIGMOID),
            (False, PF.ACT_TANH), (True, PF.ACT_TANH)]


def _operands(m, k, n, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + 1000 * m + 7 * k + n)
    x = torch.randn(m, k, generator=g).to(dtype).to(DEV)
    w = (0.5 * torch.randn(k, n, generator=g)).to(dtype).to(DEV)
    b = (0.5 * torch.randn(n, generator=g)).to(DEV)
    return x, w, b


def _bound(x, w, b, ref, act, out_dtype):
    k = x.shape[1]
    u = 2.0 ** -24 if x.dtype == torch.bfloat16 else 2.0 ** -23
    mag = x.double().abs() @ w.double().abs()
    if b is not None:
        mag = mag + b.double().abs()
    bound = 2.0 * (k + 4) * u * mag
    if act in (PF.ACT_SIGMOID, PF.ACT_TANH):
        bound = bound + 1e-5
    if out_dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * ref.abs()
    return bound


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["out_f32", "out_bf16"])
@pytest.mark.parametrize("m,k,n,dtype", SHAPES, ids=[f"{m}x{k}x{n}_{str(d)[6:]}" for m, k, n, d in SHAPES])
def test_matches_fp64_within_the_summation_bound(native_lib, m, k, n, dtype, out_dtype):
    x, w, b = _operands(m, k, n, dtype)
    pre = x.double() @ w.double()
    for has_bias, act in VARIANTS:
        bias = b if has_bias else None
        ref = ACTS[act](pre + b.double() if has_bias else pre)
        out = torch.full((m, n), float("nan"), device=DEV, dtype=out_dtype)
        assert PF.gemm_skinny_eligible(x, w, out)
        PF.gemm_skinny(x, w, out, bias=bias, act=act)
        err = (out.double() - ref).abs()
        bound = _bound(x, w, bias, ref, act, out_dtype)
        worst = (err / bound).max().item()
        print(f"({m},{k},{n}) {dtype} -> {out_dtype} bias={has_bias} act={act}: max err {err.max().item():.3e}, "
              f"max err/bound {worst:.3f}")
        assert torch.isfinite(out).all()
        assert (err <= bound).all(), (has_bias, act, err.max().item(), worst)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16])
def test_identity_rows_select_rows_of_w_exactly(native_lib, out_dtype):
    """A transposed or mis-strided write cannot hide: W is asymmetric, integer valued below 256
    (exact in bf16), and x picks single rows of it."""
    k, n = 300, 40
    kk, nn = torch.meshgrid(torch.arange(k), torch.arange(n), indexing="ij")
    w = ((kk * 7 + nn * 3) % 251).to(torch.bfloat16).to(DEV)
    rows = torch.tensor([0, 299, 17, 256, 31])
    x = torch.zeros(len(rows), k)
    x[torch.arange(len(rows)), rows] = 1.0
    x = x.to(torch.bfloat16).to(DEV)
    out = torch.empty(len(rows), n, device=DEV, dtype=out_dtype)
    PF.gemm_skinny(x, w, out)
    assert torch.equal(out.float(), w[rows.to(DEV)].float())


def test_strided_views_are_read_and_written_in_place(native_lib):
    """Eligible views: x with a leading dimension beyond K, W a 16-B aligned column slice, out a
    column slice; the bytes around out stay untouched."""
    m, k, n = 7, 200, 48
    xf = torch.randn(m, k + 24).to(torch.bfloat16).to(DEV)
    wf = (0.5 * torch.randn(k, n + 16)).to(torch.bfloat16).to(DEV)
    x, w = xf[:, 8:8 + k], wf[:, 8:8 + n]
    of = torch.full((m, n + 5), -7.0, device=DEV)
    out = of[:, 2:2 + n]
    assert PF.gemm_skinny_eligible(x, w, out)
    PF.gemm_skinny(x, w, out)
    ref = x.double() @ w.double()
    assert ((out.double() - ref).abs() <= _bound(x, w, None, ref, PF.ACT_NONE, torch.float32)).all()
    assert (of[:, :2] == -7.0).all() and (of[:, 2 + n:] == -7.0).all()


def _rows_do_not_depend_on_the_batch(m, k, n, dtype):
    x, w, b = _operands(m, k, n, dtype, seed=3)
    out = torch.empty(m, n, device=DEV)
    again = torch.empty(m, n, device=DEV)
    PF.gemm_skinny(x, w, out, bias=b, act=PF.ACT_TANH)
    PF.gemm_skinny(x, w, again, bias=b, act=PF.ACT_TANH)
    assert torch.equal(out, again)
    for r in range(m):  # every row alone (M = 1 bucket) against its row of the 16-row call
        one = torch.empty(1, n, device=DEV)
        PF.gemm_skinny(x[r:r + 1], w, one, bias=b, act=PF.ACT_TANH)
        assert torch.equal(one[0], out[r]), r
    for rows in (2, 3, 8):  # the other buckets too
        part = torch.empty(rows, n, device=DEV)
        PF.gemm_skinny(x[:rows], w, part, bias=b, act=PF.ACT_TANH)
        assert torch.equal(part, out[:rows]), rows


# (16, 4096, 4096): 512-row slices, so a lane of the narrow buckets sums two batches and one of the
# 16-row bucket eight; random operands, so the summation order shows
@pytest.mark.parametrize("m,k,n", [(16, 4096, 1024), (16, 77, 72), (16, 4096, 4096)])
def test_same_call_twice_is_bit_identical_and_rows_do_not_depend_on_the_batch(native_lib, m, k, n):
    assert PF.gemm_skinny_plan(k, n, torch.bfloat16)[2] == (512 if n == 4096 else 256)
    _rows_do_not_depend_on_the_batch(m, k, n, torch.bfloat16)


def test_fp32_rows_do_not_depend_on_the_batch_with_512_row_slices(native_lib):
    m, k, n = 16, 4096, 2048
    assert PF.gemm_skinny_plan(k, n, torch.float32) == (64, 8, 512)
    _rows_do_not_depend_on_the_batch(m, k, n, torch.float32)


def test_ineligible_operands_are_refused_and_nothing_is_launched(native_lib):
    def refused(x, w, out):
        before = out.clone()
        assert not PF.gemm_skinny_eligible(x, w, out)
        with pytest.raises(RuntimeError, match="not eligible"):
            PF.gemm_skinny(x, w, out)
        torch.cuda.synchronize()
        assert torch.equal(out, before)

    bf = dict(device=DEV, dtype=torch.bfloat16)
    refused(torch.ones(2, 64, **bf), torch.ones(64, 12, **bf), torch.zeros(2, 12, device=DEV))        # N * 2 B = 24 B
    refused(torch.ones(17, 64, **bf), torch.ones(64, 16, **bf), torch.zeros(17, 16, device=DEV))      # M = 17
    refused(torch.ones(2, 64, **bf), torch.ones(64, 24, **bf)[:, 4:20], torch.zeros(2, 16, device=DEV))  # W base + 8 B
    refused(torch.ones(2, 64, **bf), torch.ones(64, 20, **bf)[:, :16], torch.zeros(2, 16, device=DEV))  # W rows 40 B apart
    refused(torch.ones(2, 64, device=DEV, dtype=torch.float64), torch.ones(64, 16, device=DEV, dtype=torch.float64),
            torch.zeros(2, 16, device=DEV))                                                           # fp64 operands
    ok = (torch.ones(2, 64, **bf), torch.ones(64, 16, **bf), torch.zeros(2, 16, device=DEV))
    assert PF.gemm_skinny_eligible(*ok)
    assert not PF.gemm_skinny_eligible(ok[0].cpu(), ok[1].cpu(), ok[2].cpu())
    with pytest.raises(RuntimeError):  # x and W of different dtypes: a structural error
        PF.gemm_skinny(ok[0].float(), ok[1], ok[2])
