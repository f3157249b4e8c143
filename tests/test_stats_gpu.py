"""pz::tensor_moments and pz::histogram (csrc/stats.hip), raw ops, and PF.tensor_summary on top of them.

Bounds. min / max: bit-equal to torch's on the fp64 image of the data. sum and sum of squares: fp64
accumulation in any order, |error| <= n 2^-53 x the fp64 sum of |v| (of v^2). Saturation counts and
histogram counts: exact integers. Thresholds are what the binding makes of them, float(thr): 0.97f, 3, 5, 0;
the data hold each of them, its fp32 neighbours on both sides and the negatives, so `>` against `>=`
(and `<=` against `<`) changes a count. Histogram cases are dyadic (ranges, edges and data multiples of 1/8):
every operation of the bin rule is exact and `histogram_reference` (integer arithmetic, compared with
torch.histogram on the CPU in test_kernel_refs_cpu.py) is unambiguous. Outputs carry sentinels past
what the op owns.

Kernels reached:
  init_moments_kernel, decode_moments_kernel   every tensor_moments call (alone: test_moments_of_nothing)
  moments_kernel<double|float|uint16_t>        test_moments[f64|f32|bf16-*]: rules 0, 1 (SAT_ABS_GT), 2 (SAT_LE); n = 1, 63
                                               (less than a block), 257, 70000, 2048 * 256 + 777 (second sweep)
  row_rule_kernel<double|float|uint16_t>       test_row_rules[*]: rules 3 (SAT_ROW_NORM_GT) and 4 (SAT_ROW_MAX_GT), rows 1, 5,
                                               37 (not a multiple of the 4 waves), row_len 3, 64, 200
  histogram_kernel<double|float|uint16_t>      test_histogram[*], test_histogram_degenerate_range; <float> second sweep:
                                               test_histogram_second_sweep
"""
import math

import numpy as np
import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests.helpers import bit_equal, histogram_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
DTYPES = pytest.mark.parametrize("dtype", [F64, F32, BF16], ids=["f64", "f32", "bf16"])
U = 2.0 ** -53
INF = float("inf")
BIG = 2048 * 256 + 777  # one element past the widest grid's first sweep, and then some


def thr_f(thr):
    return float(np.float32(thr))


def specials(dtype):
    """Each threshold as the kernel sees it, its fp32 neighbours on both sides (for bf16 data also its
    bf16 neighbours) and the negatives of all of them, rounded to `dtype`."""
    t = torch.tensor([0.97, 3.0, 5.0, 0.0], dtype=F32)
    inf = torch.tensor(INF)
    pts = [t, torch.nextafter(t, inf), torch.nextafter(t, -inf)]
    if dtype == BF16:
        pts += [t * (1 + 2.0 ** -7), t * (1 - 2.0 ** -8), torch.tensor([2.0 ** -133, 0.96875, 0.97265625])]
    pts = torch.cat(pts)
    return torch.cat([pts, -pts]).to(dtype)


def make_data(n, dtype, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(n, generator=g, dtype=F64) * 2).to(dtype)
    sp = specials(dtype)
    k = min(n, sp.numel())
    x[:k] = sp[torch.randperm(sp.numel(), generator=g)][:k]
    if n >= 2 * sp.numel():
        x[-sp.numel():] = sp  # the last sweep sees them too
    return x


def run_moments(x_dev, row_len, rule, thr):
    out = torch.full((11,), -3.0, dtype=F64, device=DEV)
    torch.ops.pz.tensor_moments(x_dev, row_len, rule, thr, out[:8])
    out = out.cpu()
    assert out[5:8].tolist() == [0.0] * 3 and out[8:].tolist() == [-3.0] * 3
    return out


def check_min_max(out, x64):
    want = torch.stack([x64.min(), x64.max()])
    assert bit_equal(out[:2], want), (out[:2].tolist(), want.tolist())


@pytest.mark.parametrize("n", [1, 63, 257, 70000, BIG])
@DTYPES
def test_moments(native_lib, dtype, n):
    x = make_data(n, dtype, n)
    x64 = x.double()
    xd = x.to(DEV)
    s_ref, ss_ref = math.fsum(x64.tolist()), math.fsum((x64 * x64).tolist())
    s_abs = math.fsum(x64.abs().tolist())
    for rule, thr in [(0, 0.0), (0, 3.0), (1, 0.97), (1, 3.0), (1, 5.0), (2, 0.0), (2, 3.0)]:
        out = run_moments(xd, 1, rule, thr)
        check_min_max(out, x64)
        es, ess = abs(out[2].item() - s_ref), abs(out[3].item() - ss_ref)
        assert es <= n * U * s_abs and ess <= n * U * ss_ref, (rule, thr, es, n * U * s_abs, ess, n * U * ss_ref)
        want = {0: 0, 1: (x64.abs() > thr_f(thr)).sum().item(), 2: (x64 <= thr_f(thr)).sum().item()}[rule]
        assert out[4].item() == want, (rule, thr, out[4].item(), want)
    # infinities and the largest finite values: min / max stay exact, the counts too
    if n >= 2:
        top = torch.finfo(dtype).max
        for lo, hi in [(-INF, top), (-top, INF), (-INF, INF), (-top, top)]:
            y = x.clone()
            y[n // 3], y[n - 1] = lo, hi
            y64 = y.double()
            out = run_moments(y.to(DEV), 1, 1, 3.0)
            check_min_max(out, y64)
            assert out[4].item() == (y64.abs() > 3.0).sum().item()


def test_moments_of_nothing(native_lib):
    """n == 0: no error; min and max decode the untouched keys, which are NaNs, the rest is zero."""
    for dtype in (F64, F32, BF16):
        out = run_moments(torch.empty(0, dtype=dtype, device=DEV), 0, 1, 3.0)
        assert math.isnan(out[0].item()) and math.isnan(out[1].item()) and out[2:8].tolist() == [0.0] * 6


@pytest.mark.parametrize("row_len", [3, 64, 200])
@pytest.mark.parametrize("rows", [1, 5, 37])
@DTYPES
def test_row_rules(native_lib, dtype, rows, row_len):
    """One wave per row. Planted: a row of norm exactly 5, (3, 4, 0, ...), which `> 5` does not count; the
    same row with 2^-10 added, which it does; rows whose maximum is the threshold itself and its
    neighbour above. The other rows straddle the thresholds at random."""
    g = torch.Generator(device="cpu").manual_seed(100 * rows + row_len)
    x = (torch.randn(rows, row_len, generator=g, dtype=F64) * (5.0 / math.sqrt(row_len))).to(dtype)
    x[0] = 0
    x[0, 0], x[0, row_len - 1] = 3.0, 4.0
    if rows > 1:
        x[1] = x[0]
        x[1, 1] = 2.0 ** -10
    x64 = x.double()
    xd = x.to(DEV)
    norm = (x64 * x64).sum(1).sqrt()
    assert norm[0].item() == 5.0 and (rows == 1 or norm[1].item() > 5.0)
    assert ((norm[2:] - 5.0).abs() > 1e-9).all()  # no other row within rounding of the threshold
    out = run_moments(xd, row_len, 3, 5.0)
    check_min_max(out, x64)
    assert out[4].item() == (norm > 5.0).sum().item(), (out[4].item(), norm.tolist())
    assert abs(out[3].item() - (x64 * x64).sum().item()) <= x.numel() * U * (x64 * x64).sum().item()
    for thr in (0.97, 3.0):
        t = thr_f(thr)
        y = x.clone()
        if rows > 2:  # rows whose maximum is the threshold (as the dtype holds it) and the next value up
            at = torch.tensor(t, dtype=F32).to(dtype)
            up = at.float() * (1 + 2.0 ** -7) if dtype == BF16 else torch.nextafter(at.float(), torch.tensor(INF))
            up = up.to(dtype)
            y[2:4] = y[2:4].clamp(max=0.5)
            y[2, row_len // 2] = at
            y[3 % rows, row_len - 1] = up
        y64 = y.double()
        out = run_moments(y.to(DEV), row_len, 4, thr)
        want = (y64.max(1).values > t).sum().item()
        assert out[4].item() == want, (thr, out[4].item(), want)
        if rows > 2 and dtype != BF16:
            assert y64[2].max().item() == t and y64[3].max().item() > t


# ------------------------------------------------------------------------------------- histogram
def run_histogram(x_dev, lo, hi, bins, pad=3):
    rng = torch.tensor([lo, hi, -9.0], dtype=F64, device=DEV)
    pre = torch.arange(bins + pad, dtype=torch.int64) * 3 + 5
    counts = pre.clone().to(DEV)
    torch.ops.pz.histogram(x_dev, rng[:2], bins, counts)
    counts = counts.cpu()
    assert torch.equal(counts[bins:], pre[bins:]) and rng.tolist() == [lo, hi, -9.0]
    return (counts - pre)[:bins]  # what the call added to the preloaded counts


def dyadic_data(lo, hi, dtype, seed):
    """Every multiple of 1/8 from lo - 2 to hi + 2 (all edges, hi itself, values outside), hi and lo
    again, NaNs, and a random refill; what `dtype` cannot hold exactly is left out."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    k = torch.arange(int(lo * 8) - 16, int(hi * 8) + 17, dtype=F64)
    k = torch.cat([k, k[torch.randint(0, k.numel(), (3000,), generator=g)]])
    v = torch.cat([k / 8, torch.tensor([hi, hi, hi, lo, lo, float("nan"), float("nan")], dtype=F64)])
    v = v[(v.to(dtype).double() == v) | v.isnan()]
    edges = torch.arange(int(lo), int(hi) + 1, dtype=F64)
    assert torch.isin(edges, v).all()
    return v.to(dtype)


@pytest.mark.parametrize("lo,hi,bins", [(0.0, 8.0, 1), (0.0, 8.0, 8), (0.0, 8.0, 64), (-4.0, 4.0, 1), (-4.0, 4.0, 8),
                                        (-4.0, 4.0, 64), (0.0, 100.0, 100)])
@DTYPES
def test_histogram(native_lib, dtype, lo, hi, bins):
    x = dyadic_data(lo, hi, dtype, bins)
    ref = histogram_reference(x, lo, hi, bins)
    assert ref.sum() < x.numel() - 2 and ref[-1] >= 3  # some values lie outside; hi is in the last bin
    got = run_histogram(x.to(DEV), lo, hi, bins)
    assert got.tolist() == ref.tolist()
    assert run_histogram(torch.empty(0, dtype=dtype, device=DEV), lo, hi, bins).tolist() == [0] * bins  # n == 0


def test_histogram_second_sweep(native_lib):
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randint(-48, 49, (BIG,), generator=g).float() / 8
    x[-1], x[-2], x[0] = 4.0, -4.0, 4.125
    got = run_histogram(x.to(DEV), -4.0, 4.0, 64)
    assert got.tolist() == histogram_reference(x, -4.0, 4.0, 64).tolist()


@pytest.mark.parametrize("bins", [1, 7, 8, 100])
@DTYPES
def test_histogram_degenerate_range(native_lib, dtype, bins):
    """lo == hi (all values equal): the range widens to [c - 0.5, c + 0.5] and everything lands in bin
    bins // 2, torch.histogram's choice (test_kernel_refs_cpu.py::test_degenerate_histogram_bin)."""
    x = torch.full((300,), 3.0, dtype=dtype, device=DEV)
    want = [0] * bins
    want[bins // 2] = 300
    assert run_histogram(x, 3.0, 3.0, bins).tolist() == want


# -------------------------------------------------------------------------------------- refusals
def refused(call, *untouched):
    before = [t.clone() for t in untouched]
    with pytest.raises(RuntimeError):
        call()
    torch.cuda.synchronize()
    for t, b in zip(untouched, before):
        assert bit_equal(t, b)


@pytest.mark.parametrize("case", ["bins=0", "bins<0", "bins>counts", "bins>lds", "range-short", "range-cpu", "range-f32",
                                  "counts-cpu", "counts-i32"])
def test_histogram_refusals(native_lib, case):
    x = torch.ones(100, device=DEV)
    rng = torch.tensor([0.0, 2.0], dtype=F64, device=DEV)
    counts = torch.full((8,), 7, dtype=torch.int64, device=DEV)
    bins = {"bins=0": 0, "bins<0": -1, "bins>counts": 9, "bins>lds": 8193}.get(case, 8)
    if case == "bins>lds":
        counts = torch.full((8193,), 7, dtype=torch.int64, device=DEV)
    rng = {"range-short": rng[:1], "range-cpu": rng.cpu(), "range-f32": rng.float()}.get(case, rng)
    counts = {"counts-cpu": counts.cpu(), "counts-i32": counts.int()}.get(case, counts)
    refused(lambda: torch.ops.pz.histogram(x, rng, bins, counts), counts, rng)


@pytest.mark.parametrize("case", ["out-cpu", "out-short", "out-f32", "rule=5", "rule<0"])
def test_tensor_moments_refusals(native_lib, case):
    x = torch.ones(100, device=DEV)
    out = torch.full((8,), -3.0, dtype=F64, device=DEV)
    out = {"out-cpu": out.cpu(), "out-short": out[:7], "out-f32": out.float()}.get(case, out)
    rule = {"rule=5": 5, "rule<0": -1}.get(case, 1)
    refused(lambda: torch.ops.pz.tensor_moments(x, 1, rule, 3.0, out), out)


# -------------------------------------------------------------------------------- tensor_summary
def std_bound(x64, std_ref):
    """tensor_summary forms var = (ss - s s / n) / (n - 1) from the kernel's fp64 sums s and ss.
    With u = 2^-53, A = sum v^2 and S = sum |v|: ss carries at most (n + 1) u A (one rounding per square,
    n - 1 additions), s at most (n - 1) u S, so s s / n is off by at most 2 (n - 1) u S^2 / n plus 2 u S^2 / n
    for its own two roundings, and S^2 / n <= A (Cauchy-Schwarz); the subtraction and the division add
    2 u of a result that is itself <= A. To first order in u the numerator is off by at most
    (3 n + 4) u A, the variance by E = (3 n + 4) u A / (n - 1). Since |sqrt(a) - sqrt(b)| <= sqrt|a - b|
    and also <= |a - b| / sqrt(b), the std is within min(sqrt(E), E / std) of the true one (plus 4 u std
    for the square root and the reference's own rounding)."""
    n = x64.numel()
    e = (3 * n + 4) * U * math.fsum((x64 * x64).tolist()) / (n - 1)
    return min(math.sqrt(e), e / std_ref if std_ref > 0 else INF) + 4 * U * std_ref


@pytest.mark.parametrize("case", ["constant-f32", "mean1000-f64", "mean1000-f32"])
def test_tensor_summary_cancellation(native_lib, case):
    n = 4096
    if case == "constant-f32":
        x = torch.full((n,), 0.1, dtype=F32)
    else:
        g = torch.Generator(device="cpu").manual_seed(9)
        x = (1000.0 + 1e-3 * torch.randn(n, generator=g, dtype=F64)).to(F64 if case.endswith("f64") else F32)
    x64 = x.double()
    mean_ref = math.fsum(x64.tolist()) / n
    std_ref = math.sqrt(math.fsum(((x64 - mean_ref) ** 2).tolist()) / (n - 1))  # two passes: no cancellation
    got = PF.tensor_summary(x.to(DEV), None, 0)
    bound = std_bound(x64, std_ref)
    print(f"{case}: mean rel err {abs(got['mean'] - mean_ref) / abs(mean_ref):.3e}, std {got['std']:.6e} "
          f"(two-pass {std_ref:.6e}), |err| {abs(got['std'] - std_ref):.3e}, bound {bound:.3e}")
    assert abs(got["mean"] - mean_ref) <= 1e-12 * abs(mean_ref)
    assert abs(got["std"] - std_ref) <= bound
