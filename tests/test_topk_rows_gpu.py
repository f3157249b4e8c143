"""``pz::topk_rows`` (csrc/topk_rows.hip) against ``PF.topk_rows_reference`` on the inputs of
``tests/score_cases.py``: every kind of logits at widths on both sides of the thresholds between the kernel's
forms (16 lanes per row to 64 columns, a wave to 1024, a workgroup of 256 threads to 8192, of 1024 beyond),
columns exactly, log-probabilities within that file's bound for this summation order and bit-equal to
``pz::token_logprob``'s; ties at the k-th place in every form; bit reproducibility and row independence;
strided arguments; the binding's refusals."""
import math

import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests import score_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GROUPS = [(kind, cols, [(rows, seed) for _, k, rows, c, seed in C.cases() if (k, c) == (kind, cols)])
          for kind, cols in sorted({(k, c) for _, k, _, c, _ in C.cases()})]
FORMS = (27, 257, 4097, 8193)  # one width per form of the kernel


def _ks(cols):
    return sorted({1, min(cols, 5), min(cols, 64)})


def _bits(t):
    return t.view(torch.int32)


def _check(name, lg, k, idx, logprob):
    """idx exactly, logprob within the bound (equal infinities count as equal); the worst error / bound."""
    cols = lg.shape[1]
    ref_idx, ref_lp = PF.topk_rows_reference(lg, k)
    assert idx.dtype == torch.int32 and logprob.dtype == torch.float32 and idx.shape == logprob.shape == (lg.shape[0], k), name
    assert torch.equal(idx.cpu().long(), ref_idx), name
    got = logprob.cpu().double()
    inf = torch.isinf(ref_lp)
    assert torch.equal(got[inf], ref_lp[inf]), name
    err = (got[~inf] - ref_lp[~inf]).abs()
    tol = C.tolerance(cols, ref_lp[~inf])
    assert bool((err <= tol).all()), (name, float(err.max()), float((err / tol).max()))
    return float((err / tol).max()) if err.numel() else 0.0


@pytest.mark.parametrize("kind,cols,runs", GROUPS, ids=[f"{k}-{c}" for k, c, _ in GROUPS])
def test_against_the_reference(native_lib, kind, cols, runs):
    # the group's row counts in one launch per k: a row's result does not depend on its neighbours (tested below)
    lg = torch.cat([C.make_logits(kind, rows, cols, seed) for rows, seed in runs])
    dev = lg.to(DEV)
    worst = 0.0
    for k in _ks(cols):
        idx, logprob = PF.topk_rows(dev, k)
        worst = max(worst, _check(f"{kind}-{lg.shape[0]}x{cols}-k{k}", lg, k, idx, logprob))
        if kind == "flat":
            assert torch.equal(idx.cpu().long(), torch.arange(k).repeat(lg.shape[0], 1))
    print(f"{kind} V={cols}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("cols", FORMS)
def test_logprob_has_the_bits_of_token_logprob(native_lib, cols):
    for kind in ("normal", "ties", "neginf"):
        lg = C.make_logits(kind, 9, cols, 29).to(DEV)
        lg[0, 1], lg[0, 2] = -0.0, 0.0
        k = min(cols, 64)
        idx, logprob = PF.topk_rows(lg, k)
        for j in range(k):
            want = PF.token_logprob(lg, idx[:, j].long())[0]
            assert torch.equal(_bits(logprob[:, j].contiguous()), _bits(want)), (kind, cols, j)
    one = torch.tensor([[-0.0]], device=DEV)  # a lone -0: +0 from both
    assert _bits(PF.topk_rows(one, 1)[1]).item() == _bits(PF.token_logprob(one, torch.zeros(1, dtype=torch.int64, device=DEV))[0]).item()


# k = 64, or V where that is smaller. At V = 27 = k a row cannot hold k - 3 distinct values and V / 2 ties, so
# the tie there has exactly its three columns, and k = 13 (10 values, 14 ties) is run besides.
TIE_CASES = [(27, 27), (27, 13)] + [(cols, 64) for cols in FORMS[1:] + (C.HUGE,)]


@pytest.mark.parametrize("cols,k", TIE_CASES, ids=[f"{c}-k{k}" for c, k in TIE_CASES])
def test_ties_at_the_kth_place_go_to_the_lowest_columns(native_lib, cols, k):
    rows = 3
    flat = torch.full((rows, cols), C.FLAT_VALUE)
    # k - 3 distinct large values; every other column from the end (half the columns, where they fit) ties at
    # the k-th place: the three lowest of them are wanted, in order
    tied = torch.arange(cols - 1, -1, -2)[:cols - (k - 3)]
    scattered = torch.full((rows, cols), -3.0)
    scattered[:, tied] = 2.5
    is_tied = torch.zeros(cols, dtype=torch.bool)
    is_tied[tied] = True
    rest = torch.nonzero(~is_tied).reshape(-1)
    g = torch.Generator().manual_seed(cols)
    big = torch.stack([rest[torch.randperm(rest.numel(), generator=g)[:k - 3]] for _ in range(rows)])
    scattered[torch.arange(rows).unsqueeze(1), big] = 10.0 + torch.arange(k - 3, dtype=torch.float32).flip(0)
    lowest = tied.flip(0)[:3]
    assert tied.numel() >= 3 and (k == cols or tied.numel() == (cols + 1) // 2)
    # fewer than k finite columns: the -inf ones follow in column order
    few = torch.full((rows, cols), -math.inf)
    finite = torch.randperm(cols, generator=g)[:k // 2]
    few[:, finite] = torch.randn(rows, finite.numel(), generator=g)
    is_finite = torch.zeros(cols, dtype=torch.bool)
    is_finite[finite] = True
    for name, lg in (("flat", flat), ("scattered", scattered), ("few", few)):
        idx, logprob = PF.topk_rows(lg.to(DEV), k)
        _check(f"{name}-{cols}", lg, k, idx, logprob)
        got = idx.cpu().long()
        if name == "flat":
            assert torch.equal(got, torch.arange(k).repeat(rows, 1))
        elif name == "scattered":
            assert torch.equal(got[:, :k - 3], big) and torch.equal(got[:, k - 3:], lowest.repeat(rows, 1))
        else:
            n = finite.numel()
            rest_inf = torch.nonzero(~is_finite).reshape(-1)[:k - n]
            assert torch.equal(got[:, n:], rest_inf.repeat(rows, 1))
            assert bool((logprob[:, n:] == -math.inf).all()) and bool(torch.isfinite(logprob[:, :n]).all())


@pytest.mark.parametrize("cols", FORMS)
def test_bit_reproducible_and_rows_independent(native_lib, cols):
    lg = C.make_logits("ties", 257, cols, 3).to(DEV)
    k = 7
    idx1, lp1 = PF.topk_rows(lg, k)
    idx2, lp2 = PF.topk_rows(lg, k)
    assert torch.equal(idx1, idx2) and torch.equal(_bits(lp1), _bits(lp2))
    for i in (0, 1, 2, 3, 4, 130, 255, 256):
        idx, lp = PF.topk_rows(lg[i:i + 1], k)
        assert torch.equal(idx, idx1[i:i + 1]) and torch.equal(_bits(lp), _bits(lp1[i:i + 1])), i
    idx, lp = PF.topk_rows(lg[5:70], k)  # the same rows at other places of their workgroups
    assert torch.equal(idx, idx1[5:70]) and torch.equal(_bits(lp), _bits(lp1[5:70]))
    # a smaller k is a prefix of a larger one
    idx, lp = PF.topk_rows(lg, 3)
    assert torch.equal(idx, idx1[:, :3]) and torch.equal(_bits(lp), _bits(lp1[:, :3].contiguous()))


@pytest.mark.parametrize("cols", FORMS)
def test_strided_arguments(native_lib, cols):
    rows, k = 9, 6
    lg = C.make_logits("ties", rows, cols, 11).to(DEV)
    want_idx, want_lp = PF.topk_rows(lg, k)
    wide = torch.full((rows, cols + 3), 1e9, device=DEV)  # (a stray read of the margin would be the maximum)
    wide[:, 1:1 + cols] = lg
    view = wide[:, 1:1 + cols]
    assert not view.is_contiguous() and view.stride(0) == cols + 3
    out_i = torch.full((rows, k + 4), -9, device=DEV, dtype=torch.int32)
    out_l = torch.full((rows, k + 2), -5.0, device=DEV)
    idx, lp = PF.topk_rows(view, k, out_i[:, 3:3 + k], out_l[:, 1:1 + k])
    assert idx.data_ptr() == out_i[:, 3:].data_ptr() and lp.data_ptr() == out_l[:, 1:].data_ptr()
    assert torch.equal(out_i[:, 3:3 + k], want_idx) and torch.equal(_bits(out_l[:, 1:1 + k].contiguous()), _bits(want_lp))
    assert bool((out_i[:, :3] == -9).all()) and bool((out_i[:, 3 + k:] == -9).all())
    assert bool((out_l[:, :1] == -5.0).all()) and bool((out_l[:, 1 + k:] == -5.0).all())


def test_binding_refusals(native_lib):
    lg = torch.zeros(4, 8, device=DEV)
    idx = torch.zeros(4, 3, device=DEV, dtype=torch.int32)
    lp = torch.zeros(4, 3, device=DEV)
    op = native_lib.topk_rows
    op(lg, 3, idx, lp)
    wide = torch.zeros(4, 100, device=DEV)
    bad = [
        (lg.double(), 3, idx, lp), (lg.bfloat16(), 3, idx, lp), (lg.cpu(), 3, idx, lp),        # logits: dtype, device
        (lg, 3, idx.long(), lp), (lg, 3, idx, lp.double()), (lg, 3, idx.cpu(), lp), (lg, 3, idx, lp.cpu()),  # outputs
        (lg, 3, idx[:3], lp), (lg, 3, idx, lp[:3]), (lg[:3], 3, idx, lp),                         # rows
        (lg, 3, idx[:, :2], lp), (lg, 3, idx, lp[:, :2]), (lg, 2, idx, lp),                       # short / long outputs
        (lg[:, ::2], 3, idx, lp), (lg.t(), 3, idx.new_zeros(8, 3), lp.new_zeros(8, 3)),           # logits column stride
        (lg, 3, idx.new_zeros(4, 6)[:, ::2], lp), (lg, 3, idx, lp.new_zeros(4, 6)[:, ::2]),       # output column stride
        (lg, 3, idx.new_zeros(3, 4).t(), lp),                                                     # overlapping output rows
        (lg, 0, idx[:, :0], lp[:, :0]), (lg, -1, idx, lp),                                        # k < 1
        (lg, 9, idx.new_zeros(4, 9), lp.new_zeros(4, 9)),                                         # k > V
        (wide, 65, idx.new_zeros(4, 65), lp.new_zeros(4, 65)),                                    # k > 64
        (lg[:, :0], 1, idx[:, :1], lp[:, :1]),                                                    # no columns
        (lg[0], 3, idx[0], lp[0]), (lg, 3, idx.view(-1), lp.view(-1)),                            # dimensions
    ]
    if torch.cuda.device_count() > 1:
        bad.append((lg, 3, idx.to("cuda:1"), lp))
    for args in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            op(*args)
    op(wide, 64, idx.new_zeros(4, 64), lp.new_zeros(4, 64))
    torch.cuda.synchronize()
    before = (idx.clone(), lp.clone())
    op(lg[:0], 3, idx[:0], lp[:0])  # no rows: no launch
    assert torch.equal(idx, before[0]) and torch.equal(lp, before[1])
    with pytest.raises(RuntimeError):
        PF.topk_rows(lg, 9)  # the wrapper allocates [rows, k]; the binding refuses k > V
