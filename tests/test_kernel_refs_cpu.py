"""The host references the GPU kernel tests lean on, against plain Python-int arithmetic."""
import numpy as np
import pytest

import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.helpers import (ACT_FWD, FP8_SPLIT_CASES, PAIR_SPLIT_CASES, SGD_EXACT, UPDATE_SPLIT_CASES, assert_gemm_exact,
                           exact_operands, exact_operands_fp8, fp8_all_codes, fp8_code_values, fp8_encode_reference,
                           fp8_tie_points, gather_picks, gather_seed, gemm_epilogue_reference, gemm_pair_split_plan,
                           gemm_split_plan, histogram_reference, keep2d, keep2d_cached, keep_mask, opt_update_reference,
                           stage_bwd_reference, stage_fwd_reference)

M32 = 0xFFFFFFFF


def picks_by_hand(rows_valid, n_data, lo, hi, epoch):
    if epoch is not None:
        lo = (lo + epoch * 0x632BE5AB) % 2 ** 32
        hi = (hi ^ epoch) % 2 ** 32
    return [(PF.mix32(PF.mix32(row ^ lo) ^ hi) * n_data) >> 32 for row in range(rows_valid)]


@pytest.mark.parametrize("seed,n_data,epoch", [
    ((11, 22), 1000, None),
    ((0xDEADBEEF, 0x0BADF00D), 1000, 5),
    ((0xFFFFFFFF, 0xFFFFFFFF), 3, 7),            # lo + epoch * c wraps
    ((0, 0), 1, 0),
    ((0x2468ACE0, 0x13579BDF), 2 ** 31 + 12345, 123456),
    ((5, 9), 60000, 2 ** 31 - 1),
])
def test_gather_picks_matches_python_ints(seed, n_data, epoch):
    got = gather_picks(257, n_data, seed[0], seed[1], epoch)
    assert got.dtype == np.int64 and got.shape == (257,)
    assert got.tolist() == picks_by_hand(257, n_data, seed[0], seed[1], epoch)
    assert (got >= 0).all() and (got < n_data).all()
    if n_data == 1:
        assert (got == 0).all()


def test_gather_picks_spread_and_epoch_zero():
    a = gather_picks(1000, 1000, 1, 2)
    assert len(set(a.tolist())) > 500  # sampling with replacement: about 632 distinct of 1000
    assert not np.array_equal(a, gather_picks(1000, 1000, 1, 2, epoch=1))
    assert np.array_equal(a, gather_picks(1000, 1000, 1, 2, epoch=0))  # epoch 0 changes neither seed
    assert gather_seed(1, 2, None) == (1, 2) and gather_seed(M32, 6, 3) == ((M32 + 3 * 0x632BE5AB) & M32, 5)
    assert gather_picks(0, 10, 1, 2).shape == (0,)


def test_keep2d_is_the_flat_mask_at_row_stride():
    flat = keep_mask(5 * 16, 3, 4, 2, 0.25, epoch=3).reshape(5, 16)
    assert np.array_equal(keep2d(5, 10, 16, (3, 4), 2, 0.25, epoch=3).numpy(), flat[:, :10])
    assert np.array_equal(keep2d(5, 16, 0, (3, 4), 2, 0.25, epoch=3).numpy(), flat)


FP8 = {"e4m3": (torch.float8_e4m3fn, 448.0, 1020), "e5m2": (torch.float8_e5m2, 57344.0, 996)}


@pytest.mark.parametrize("name", list(FP8))
def test_fp8_code_table_is_the_formats(name):
    fmt, top, _ = FP8[name]
    table = fp8_code_values(fmt)
    by_view = torch.arange(len(table), dtype=torch.uint8).view(fmt).double().numpy()
    assert np.array_equal(table, by_view) and table[-1] == top and (np.diff(table) > 0).all()
    assert not torch.isfinite(torch.tensor([len(table)], dtype=torch.uint8).view(fmt).float()).any()


@pytest.mark.parametrize("name", list(FP8))
def test_fp8_encode_reference_matches_torch_cpu_cast(name):
    """The table-built encoder against torch's CPU cast of the clamped value on every code, every
    midpoint (the ties), their fp32 neighbours, subnormal and out-of-range points, both signs."""
    fmt, top, count = FP8[name]
    pts = fp8_tie_points(fmt)
    assert pts.dtype == torch.float32 and pts.numel() == count and not torch.isnan(pts).any()
    assert torch.equal(pts[:count // 2], -pts[count // 2:])
    got = fp8_encode_reference(pts.double(), fmt)
    ref = pts.clamp(-top, top).to(fmt).view(torch.uint8)
    assert got.dtype == torch.uint8 and torch.equal(got, ref)
    # spot checks by hand: ties to even, the sign of zero, saturation
    table = fp8_code_values(fmt)
    hand = torch.tensor([0.0, -0.0, (table[1] + table[2]) / 2, (table[2] + table[3]) / 2, table[1] / 2, 1e30, -1e30],
                        dtype=torch.float64)
    last = len(table) - 1
    assert fp8_encode_reference(hand, fmt).tolist() == [0, 0x80, 2, 2, 0, last, 0x80 | last]
    # the same points through an exact scale pair, as the codebook GPU test feeds them
    assert torch.equal((pts * 8) * 0.125, pts)


@pytest.mark.parametrize("lo,hi,bins", [(0.0, 8.0, 1), (0.0, 8.0, 8), (0.0, 8.0, 64), (-4.0, 4.0, 8),
                                        (-4.0, 4.0, 64), (0.0, 100.0, 100)])
def test_histogram_reference_matches_torch_histogram(lo, hi, bins):
    v = torch.arange(int(lo * 8) - 16, int(hi * 8) + 17, dtype=torch.float64) / 8  # every edge, hi, outside
    v = torch.cat([v, v[::3], torch.tensor([hi, hi, lo])])
    ref = torch.histogram(v, bins=bins, range=(lo, hi)).hist
    got = histogram_reference(torch.cat([v, torch.tensor([float("nan")])]), lo, hi, bins)
    assert got.dtype == np.int64 and got.tolist() == ref.tolist()
    assert got.sum() == ((v >= lo) & (v <= hi)).sum().item()


@pytest.mark.parametrize("bins", [1, 7, 8, 100])
def test_degenerate_histogram_bin(bins):
    """torch.histogram widens an all-equal range to [c - 0.5, c + 0.5]: everything lands in bin bins // 2
    (what the GPU test of the lo == hi range expects)."""
    h = torch.histogram(torch.full((10,), 3.0, dtype=torch.float64), bins=bins).hist
    want = [0] * bins
    want[bins // 2] = 10
    assert h.tolist() == want


# ------------------------------------------------------------------------------------ exact GEMM
@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, True), (False, False)])
def test_exact_operands_match_python_int_dot_products(a_kc, b_kc):
    M, N, K = 37, 29, 96
    a, b, z = exact_operands(M, N, K, a_kc, b_kc, seed=5)
    assert a.dtype == b.dtype == torch.bfloat16 and z.dtype == torch.float64 and z.shape == (M, N)
    assert a.shape == ((M, K) if a_kc else (K, M)) and b.shape == ((N, K) if b_kc else (K, N))
    for t in (a, b):
        assert torch.equal(t.double(), t.double().round()) and t.min() == -4 and t.max() == 4
    al, bl = a.int().tolist(), b.int().tolist()
    for m, n in [(0, 0), (M - 1, N - 1), (3, 17), (36, 0), (11, 28)]:
        dot = sum((al[m][k] if a_kc else al[k][m]) * (bl[n][k] if b_kc else bl[k][n]) for k in range(K))
        assert z[m, n].item() == dot
    a2, _, z2 = exact_operands(M, N, K, a_kc, b_kc, seed=5)
    assert torch.equal(a, a2) and torch.equal(z, z2)
    assert not torch.equal(a, exact_operands(M, N, K, a_kc, b_kc, seed=6)[0])
    with pytest.raises(AssertionError):
        exact_operands(8, 8, 2 ** 20, a_kc, b_kc, seed=1)


def test_assert_gemm_exact_demands_an_fp32_exact_reference_and_equal_values():
    _, _, z = exact_operands(16, 24, 64, True, False, seed=2)
    eighths = torch.arange(-12, 12, dtype=torch.float64) / 8
    ref, _ = gemm_epilogue_reference(z, alpha=0.5, bias=eighths, mode=0, act=0, keep_pre=None, keep_post=None, scale=1.0)
    assert_gemm_exact(ref.to(torch.bfloat16), ref)
    assert_gemm_exact(ref.float(), ref)
    relu = ref.clamp_min(0.0)
    assert (relu == 0).any()
    assert_gemm_exact(torch.where(relu == 0, torch.tensor(-0.0), relu.float()), relu)  # -0 equals the reference's +0
    third, _ = gemm_epilogue_reference(z, alpha=0.5, bias=torch.full((24,), 1 / 3, dtype=torch.float64), mode=0, act=0,
                                       keep_pre=None, keep_post=None, scale=1.0)
    with pytest.raises(AssertionError, match="not exact in fp32"):
        assert_gemm_exact(third.float(), third)
    off = ref.float().clone()
    off[3, 5] = torch.nextafter(off[3, 5], torch.tensor(float("inf")))
    with pytest.raises(AssertionError, match="1 of 384 elements differ"):
        assert_gemm_exact(off, ref)
    nan = ref.float().clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        assert_gemm_exact(nan, ref)


@pytest.mark.parametrize("dtype,hi", [(torch.float32, 256), (torch.float64, 2 ** 20), (torch.float64, 4), (torch.bfloat16, 256)])
@pytest.mark.parametrize("a_kc,b_kc", [(True, False), (False, True)])
def test_widened_exact_operands_match_python_int_dot_products(dtype, hi, a_kc, b_kc):
    M, N, K = 19, 23, 96
    a, b, z = exact_operands(M, N, K, a_kc, b_kc, seed=7, dtype=dtype, hi=hi)
    assert a.dtype == b.dtype == dtype and z.dtype == torch.float64 and z.shape == (M, N)
    al, bl = a.double().tolist(), b.double().tolist()
    assert all(float(v).is_integer() and abs(v) <= hi for row in al + bl for v in row)
    assert max(abs(v) for row in al for v in row) > hi * 0.9      # the range is used
    for m, n in [(0, 0), (M - 1, N - 1), (3, 17), (18, 0), (11, 22)]:
        dot = sum(int(al[m][k] if a_kc else al[k][m]) * int(bl[n][k] if b_kc else bl[k][n]) for k in range(K))
        assert z[m, n].item() == dot and int(z[m, n].item()) == dot
    if hi == 4:  # the default range draws the same integers in every dtype
        assert torch.equal(a, exact_operands(M, N, K, a_kc, b_kc, seed=7)[0].to(dtype))
    # the limits: K hi^2 below 2^24 (bf16, fp32) or 2^53 (fp64); bf16 holds integers up to 256
    exact_operands(4, 4, 255, a_kc, b_kc, seed=1, dtype=torch.float32, hi=256)
    with pytest.raises(AssertionError):
        exact_operands(4, 4, 256, a_kc, b_kc, seed=1, dtype=torch.float32, hi=256)
    exact_operands(4, 4, 2 ** 12, a_kc, b_kc, seed=1, dtype=torch.float64, hi=2 ** 20)
    with pytest.raises(AssertionError):
        exact_operands(4, 4, 2 ** 13, a_kc, b_kc, seed=1, dtype=torch.float64, hi=2 ** 20)
    with pytest.raises(AssertionError):
        exact_operands(4, 4, 16, a_kc, b_kc, seed=1, dtype=torch.bfloat16, hi=257)


def test_assert_gemm_exact_fp64_outputs_equal_the_reference_itself():
    _, _, z = exact_operands(16, 24, 64, True, False, seed=2, dtype=torch.float64, hi=2 ** 20)
    third = torch.full((24,), 1 / 3, dtype=torch.float64)
    ref, _ = gemm_epilogue_reference(z, alpha=0.5, bias=third, mode=0, act=0, keep_pre=None, keep_post=None, scale=1.0)
    assert not torch.equal(ref.float().double(), ref)     # not fp32-representable: fine for an fp64 output
    assert_gemm_exact(ref.clone(), ref)
    zero = ref.clone()
    zero[2, 2] = 0.0
    neg = zero.clone()
    neg[2, 2] = -0.0
    assert_gemm_exact(neg, zero)                          # by value: -0 equals +0
    for direction in (float("inf"), -float("inf")):       # one ulp either way is rejected
        off = ref.clone()
        off[3, 5] = torch.nextafter(off[3, 5], torch.tensor(direction, dtype=torch.float64))
        assert off[3, 5] != ref[3, 5] and abs(off[3, 5] - ref[3, 5]) <= 2.0 ** -52 * abs(ref[3, 5])
        with pytest.raises(AssertionError, match="1 of 384 elements differ"):
            assert_gemm_exact(off, ref)
    with pytest.raises(AssertionError, match="of 384 elements differ"):
        assert_gemm_exact(ref.float().double(), ref)      # an fp32 round trip of the values is not equal
    nan = ref.clone()
    nan[0, 0] = float("nan")
    with pytest.raises(AssertionError):
        assert_gemm_exact(nan, ref)


@pytest.mark.parametrize("act", [0, 1])
def test_fp64_epilogue_reference_is_exact_at_half_dropout_and_tells_the_scales_apart_at_p03(act):
    """p = 0.5: every step of the reference is exact in fp64 (checked against Python fractions).
    p = 0.3: the reference with the scale rounded to fp32 leaves the 4 * 2^-53 |ref| band the fp64
    GPU tests allow, on the shapes they use: those tests can tell which scale a kernel took."""
    from fractions import Fraction
    M, N, K = 9, 9, 9
    _, _, z = exact_operands(M, N, K, True, False, seed=M + 3 * N + 7 * K + 2, dtype=torch.float64, hi=2 ** 20)
    bias = (torch.arange(N, dtype=torch.float64) - 4) / 8
    kp, kq = keep2d(M, N, N, (1, 2), 3, 0.5), keep2d(M, N, N, (1, 2), 4, 0.5)
    ref, cs = gemm_epilogue_reference(z, alpha=0.5, bias=bias, mode=1, act=act, keep_pre=kp, keep_post=kq, scale=2.0)
    for m in range(M):
        for n in range(N):
            h = Fraction(int(z[m, n].item())) / 2 + Fraction(int(bias[n].item() * 8), 8)
            v = h * 2 if kp[m, n] else Fraction(0)
            v = max(v, Fraction(0)) if act == 1 else v
            v = v * 2 if kq[m, n] else Fraction(0)
            assert Fraction(ref[m, n].item()) == v
    assert all(Fraction(cs[n].item()) == sum(Fraction(ref[m, n].item()) for m in range(M)) for n in range(N))
    p = 0.3
    s64 = 1.0 / (1.0 - p)
    s32 = torch.tensor(s64, dtype=torch.float32).item()
    assert s32 != s64
    for shape in [(200, 136, 96), (384, 640, 64), (67, 45, 23), (9, 9, 9)]:
        M, N, K = shape
        _, _, z = exact_operands(M, N, K, True, False, seed=M + 3 * N + 7 * K + 2)
        kp, kq = keep2d(M, N, N, (1, 2), 3, p), keep2d(M, N, N, (1, 2), 4, p)
        args = dict(alpha=0.5, bias=None, mode=1, act=act, keep_pre=kp, keep_post=kq)
        ref, _ = gemm_epilogue_reference(z, scale=s64, **args)
        ref32, _ = gemm_epilogue_reference(z, scale=s32, **args)
        kept = ref != 0
        assert kept.any() and ((ref32 - ref).abs() > 4 * 2.0 ** -53 * ref.abs())[kept].all()


@pytest.mark.parametrize("act", [0, 1, 2, 3])
@pytest.mark.parametrize("pre,post", [(False, False), (True, False), (False, True), (True, True)])
def test_gemm_epilogue_reference_forward_is_the_stage_reference(act, pre, post):
    M, N, p = 24, 40, 0.5
    _, _, z = exact_operands(M, N, 64, True, False, seed=3)
    bias = torch.arange(N, dtype=torch.float64) / 8 - 2
    kp = keep2d(M, N, N + 8, (1, 2), 3, p) if pre else None
    kq = keep2d(M, N, N + 8, (1, 2), 4, p) if post else None
    got, cs = gemm_epilogue_reference(z, alpha=0.25, bias=bias, mode=1, act=act, keep_pre=kp, keep_post=kq, scale=2.0)
    h = z * 0.25 + bias
    want = stage_fwd_reference(h, act, kp, kq, torch.tensor(2.0, dtype=torch.float64))
    assert got.dtype == torch.float64 and torch.equal(got, want) and torch.equal(cs, want.sum(0))
    # by hand, element by element
    m1 = kp.double() * 2 if pre else 1.0
    m2 = kq.double() * 2 if post else 1.0
    assert torch.equal(got, ACT_FWD[act](h * m1) * m2)
    store, _ = gemm_epilogue_reference(z, alpha=0.25, bias=bias, mode=0, act=act, keep_pre=kp, keep_post=kq, scale=2.0)
    assert torch.equal(store, h)
    acc, _ = gemm_epilogue_reference(z, alpha=0.25, bias=None, mode=0, act=0, keep_pre=None, keep_post=None, scale=1.0,
                                     c_old=torch.ones(M, N))
    assert torch.equal(acc, z * 0.25 + 1)


@pytest.mark.parametrize("pre,post", [(False, False), (True, False), (False, True), (True, True)])
def test_gemm_epilogue_reference_bitmask_backward_is_the_stage_backward(pre, post):
    """A ReLU stage's stored y is positive exactly where z > 0 and both dropouts kept: the bitmask
    form (bits = y > 0, no keep masks consulted) equals the derivative chain from y."""
    M, N, p, scale = 24, 40, 0.5, 2.0
    _, _, g = exact_operands(M, N, 64, True, True, seed=4)
    _, _, h = exact_operands(M, N, 32, True, False, seed=5)
    kp = keep2d(M, N, N, (1, 2), 3, p) if pre else None
    kq = keep2d(M, N, N, (1, 2), 4, p) if post else None
    y = stage_fwd_reference(h, 1, kp, kq, torch.tensor(scale, dtype=torch.float64))
    bits = y > 0
    assert 0.05 < bits.double().mean() < 0.6
    got, cs = gemm_epilogue_reference(g, alpha=0.5, bias=None, mode=2, act=1, keep_pre=kp, keep_post=kq, scale=scale,
                                      bits=bits)
    want = stage_bwd_reference(g * 0.5, y, 1, kp, kq, scale)
    assert torch.equal(got, want) and torch.equal(cs, want.sum(0))
    from_aux, _ = gemm_epilogue_reference(g, alpha=0.5, bias=None, mode=2, act=1, keep_pre=kp, keep_post=kq, scale=scale,
                                          aux=y)
    assert torch.equal(from_aux, want)
    assert torch.equal(got, g * 0.5 * bits * (2.0 if pre else 1.0) * (2.0 if post else 1.0))


def test_keep2d_cached_is_keep2d():
    a = keep2d_cached(5, 10, 16, (3, 4), 2, 0.25)
    assert torch.equal(a, keep2d(5, 10, 16, (3, 4), 2, 0.25)) and keep2d_cached(5, 10, 16, (3, 4), 2, 0.25) is a


def test_half_dropout_is_exact_in_the_kernels_arithmetic():
    """p = 0.5: the scale, its square and its inverse are powers of two, the threshold is the top bit."""
    ei, ef = PF.epi_spec(PF.ACT_RELU, 3, 4, 0.5, (1, 2))
    assert ei[5] == 32768 and ei[6] == 0 and ef == [2.0, 0.5]
    ei, ef = PF.epi_spec(PF.ACT_RELU, 3, 4, 0.3, (1, 2))
    assert ei[5] == 19661
    ei, ef = PF.epi_spec(PF.ACT_RELU, 3, 4, 1.0, (1, 2))
    assert ei[5] == 65536 and ei[6] == 1 and ef[0] == 0.0
    assert not keep_mask(64, 1, 2, 3, 1.0).any()


E4M3, E5M2 = torch.float8_e4m3fn, torch.float8_e5m2


@pytest.mark.parametrize("fmt_a,fmt_b", [(E4M3, E4M3), (E5M2, E4M3), (E4M3, E5M2)])
@pytest.mark.parametrize("a_kc,b_kc", [(True, True), (True, False), (False, False)])
def test_exact_operands_fp8_round_trips_and_z_is_the_integer_product(fmt_a, fmt_b, a_kc, b_kc):
    M, N, K = 24, 40, 64
    a8, b8, z = exact_operands_fp8(M, N, K, a_kc, b_kc, fmt_a, fmt_b, seed=9)
    a, b, z16 = exact_operands(M, N, K, a_kc, b_kc, seed=9)
    assert a8.dtype == fmt_a and b8.dtype == fmt_b and a8.shape == a.shape and b8.shape == b.shape
    # the cast changed nothing, and a second trip through the fp8 type changes nothing either
    assert torch.equal(a8.double(), a.double()) and torch.equal(b8.double(), b.double())
    assert torch.equal(a8.float().to(fmt_a).view(torch.uint8), a8.view(torch.uint8))
    assert torch.equal(b8.float().to(fmt_b).view(torch.uint8), b8.view(torch.uint8))
    ai, bi = a8.double().long(), b8.double().long()
    assert ai.abs().max() == 4 and bi.abs().max() == 4
    want = (ai if a_kc else ai.t()) @ (bi.t() if b_kc else bi)
    assert z.dtype == torch.float64 and torch.equal(z, want.double()) and torch.equal(z, z16)


@pytest.mark.parametrize("fmt", [E4M3, E5M2])
def test_fp8_all_codes_is_the_code_table_and_fits_bf16(fmt):
    codes, values = fp8_all_codes(fmt)
    table = fp8_code_values(fmt)
    n = len(table)
    assert codes.dtype == torch.uint8 and len(codes) == 2 * n == len(set(codes.tolist()))
    assert np.array_equal(values[:n].numpy(), table) and np.array_equal(values[n:].numpy(), -table)
    assert torch.equal(codes[:n].long(), torch.arange(n)) and torch.equal(codes[n:].long(), torch.arange(n) + 128)
    as_fp8 = codes.view(fmt)
    assert torch.isfinite(as_fp8.float()).all() and torch.equal(as_fp8.double(), values)   # torch reads the codes alike
    assert torch.equal(values.to(torch.bfloat16).double(), values)                          # both formats fit bf16
    assert table[1] > 0 and (fmt != E4M3 or table[-1] == 448) and (fmt != E5M2 or table[-1] == 57344)


def test_sgd_exact_hyper_parameters_keep_the_update_fp32_representable():
    """Largest K of the gemm_update tests (4096), the largest |z| integer operands in [-4, 4] can
    give (16 K) and every p0 in multiples of 1/8 within [-4, 4]: each intermediate of the SGD formula
    is a multiple of 2^-12 below 2^12, so fp32 (and any FMA contraction of it) computes it exactly."""
    K = 4096
    g = torch.tensor([-16.0 * K, -16.0 * K + 1, -1.0, 0.0, 1.0, 777.0, 16.0 * K - 1, 16.0 * K], dtype=torch.float64)
    p0 = torch.arange(-32, 33, dtype=torch.float64) / 8
    gg, pp = torch.meshgrid(g, p0, indexing="ij")
    w = torch.ones_like(gg, dtype=torch.bool)
    hp = dict(adam=False, b1=0.0, b2=0.0, eps=0.0, bc1=1.0, bc2s=1.0, **SGD_EXACT)
    r64, _, _ = opt_update_reference(pp, gg, None, None, w, torch.float64, **hp)
    r32, _, _ = opt_update_reference(pp, gg, None, None, w, torch.float32, **hp)
    assert torch.equal(r64, pp - SGD_EXACT["lr"] * (gg * SGD_EXACT["grad_scale"] + 2 * SGD_EXACT["l2"] * pp))
    assert torch.equal(r64.float().double(), r64) and torch.equal(r32.double(), r64)
    for part in (gg * SGD_EXACT["grad_scale"], 2 * SGD_EXACT["l2"] * pp, gg * SGD_EXACT["grad_scale"] + 2 * SGD_EXACT["l2"] * pp,
                 SGD_EXACT["lr"] * (gg * SGD_EXACT["grad_scale"] + 2 * SGD_EXACT["l2"] * pp)):
        assert torch.equal(part.float().double(), part)
    assert torch.equal(r64 * 4096, (r64 * 4096).round()) and r64.abs().max() < 2 ** 12


def test_claimed_split_factors_follow_the_restated_rules():
    for (M, N, K), b_kc, split in FP8_SPLIT_CASES:
        assert gemm_split_plan(M, N, K, fp8=True, b_kc=b_kc) == split, (M, N, K, b_kc)
    for (M, N, K), split in UPDATE_SPLIT_CASES:
        assert gemm_split_plan(M, N, K) == split, (M, N, K)
    for s0, s1, K, split in PAIR_SPLIT_CASES:
        assert gemm_pair_split_plan(s0, s1, K) == gemm_pair_split_plan(s1, s0, K) == split, (s0, s1, K)
    assert {c[-1] for c in PAIR_SPLIT_CASES} == {1, 2, 4, 8}
    # by hand: 60 tiles x 4 slices = 240 workgroups of 64 / 4 = 16 fp8 K steps; bf16 K steps are 32 deep
    assert gemm_split_plan(1536, 2560, 4096, fp8=True) == 4 and gemm_split_plan(1536, 2560, 4096) == 4
    assert gemm_split_plan(1536, 2560, 2048, fp8=True) == 1 and gemm_split_plan(4096, 3840, 8192) == 1
    assert gemm_pair_split_plan((256, 512), (512, 256), 8192) == 8 and gemm_pair_split_plan((256, 512), (512, 256), 4096) == 1
