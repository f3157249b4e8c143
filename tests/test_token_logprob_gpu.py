"""``pz::token_logprob`` (csrc/token_logprob.hip) against ``PF.token_logprob_reference`` on the inputs of
``tests/score_cases.py``: every kind of logits at widths on both sides of the thresholds between the kernel's
forms (16 lanes per row to 64 columns, a wave to 1024, a workgroup of 256 threads to 8192, of 1024 beyond),
ranks exactly, log-probabilities within that file's bound; bit reproducibility and row independence in every
form; strided arguments; targets outside the vocabulary; the binding's refusals."""
import math

import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests import score_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

GROUPS = [(kind, cols, [(rows, seed) for _, k, rows, c, seed in C.cases() if (k, c) == (kind, cols)])
          for kind, cols in sorted({(k, c) for _, k, _, c, _ in C.cases()})]


def _run(logits, targets, want_rank=True):
    rank = torch.full((logits.shape[0],), -7, device=DEV, dtype=torch.int32) if want_rank else None
    logprob, rank = PF.token_logprob(logits, targets, None, rank)
    return logprob, rank


def _check(name, lg, t, logprob, rank):
    cols = lg.shape[1]
    ref_lp, ref_rank = PF.token_logprob_reference(lg, t)
    assert torch.equal(rank.cpu().long(), ref_rank), name
    got = logprob.cpu().double()
    inf = torch.isinf(ref_lp)
    assert torch.equal(got[inf], ref_lp[inf]), name  # a -inf target scores -inf exactly
    err = (got[~inf] - ref_lp[~inf]).abs()
    tol = C.tolerance(cols, ref_lp[~inf])
    assert bool((err <= tol).all()), (name, float(err.max()), float((err / tol).max()))
    return float((err / tol).max()) if err.numel() else 0.0


@pytest.mark.parametrize("kind,cols,runs", GROUPS, ids=[f"{k}-{c}" for k, c, _ in GROUPS])
def test_against_the_reference(native_lib, kind, cols, runs):
    worst = 0.0
    for rows, seed in runs:
        lg, t = C.make_logits(kind, rows, cols, seed), C.make_targets(kind, rows, cols, seed)
        logprob, rank = _run(lg.to(DEV), t.to(DEV))
        assert logprob.dtype == torch.float32 and rank.dtype == torch.int32 and logprob.shape == rank.shape == (rows,)
        worst = max(worst, _check(f"{kind}-{rows}x{cols}", lg, t, logprob, rank))
        if kind == "flat":  # -log V within the bound, and the rank is the target's index
            assert torch.equal(rank.cpu().long(), t)
            assert abs(float(logprob[0]) + math.log(cols)) <= float(C.tolerance(cols, torch.tensor(math.log(cols))))
        if kind == "neginf" and cols >= 2 and rows >= 2:
            assert float(logprob[-1]) == -math.inf and bool(torch.isfinite(logprob[:-1]).all())
    print(f"{kind} V={cols}: worst error / bound = {worst:.3f}")


def test_a_target_far_below_the_maximum_keeps_its_digits(native_lib):
    for cols in (27, 257, 4097, 8193):
        lg = torch.zeros(2, cols)
        lg[0, 5], lg[0, 7] = 100.0, -60.0   # 160 below the maximum: exp(-160) underflows, the difference does not
        lg[1, 3] = -math.inf
        t = torch.tensor([7, 3])
        logprob, rank = _run(lg.to(DEV), t.to(DEV))
        _check(f"far-{cols}", lg, t, logprob, rank)
        assert -160.001 < float(logprob[0]) < -159.999 and float(logprob[1]) == -math.inf
        assert rank.tolist() == [cols - 1, cols - 1]


@pytest.mark.parametrize("cols", [27, 257, 4097, 8193])  # every form of the kernel
def test_bit_reproducible_and_rows_independent(native_lib, cols):
    lg = C.make_logits("normal", 257, cols, 3).to(DEV)
    t = C.make_targets("normal", 257, cols, 3).to(DEV)
    lp1, rk1 = _run(lg, t)
    lp2, rk2 = _run(lg, t)
    assert torch.equal(lp1.view(torch.int32), lp2.view(torch.int32)) and torch.equal(rk1, rk2)
    for i in (0, 1, 2, 3, 4, 130, 255, 256):
        lp, rk = _run(lg[i:i + 1], t[i:i + 1])
        assert torch.equal(lp.view(torch.int32), lp1[i:i + 1].view(torch.int32)) and torch.equal(rk, rk1[i:i + 1]), i
    lp, rk = _run(lg[5:70], t[5:70])  # the same rows at other places of their workgroups
    assert torch.equal(lp.view(torch.int32), lp1[5:70].view(torch.int32)) and torch.equal(rk, rk1[5:70])


@pytest.mark.parametrize("cols", [27, 257, 4097, 8193])
def test_strided_arguments(native_lib, cols):
    rows = 9
    lg = C.make_logits("ties", rows, cols, 11).to(DEV)
    t = C.make_targets("ties", rows, cols, 11).to(DEV)
    want_lp, want_rk = _run(lg, t)
    wide = torch.full((rows, cols + 5), 1e9, device=DEV)  # (a stray read of the margin would ruin the maximum)
    wide[:, 3:3 + cols] = lg
    seq = torch.full((rows, 5), 10 ** 12, device=DEV, dtype=torch.int64)
    seq[:, 2] = t
    out = torch.full((rows, 3), -5.0, device=DEV)
    ranks = torch.full((rows, 2), -9, device=DEV, dtype=torch.int32)
    view = wide[:, 3:3 + cols]
    assert not view.is_contiguous() and view.data_ptr() % 16 != 0
    lp, rk = PF.token_logprob(view, seq[:, 2], out[:, 1], ranks[:, 0])
    assert lp.data_ptr() == out[:, 1].data_ptr() and rk.data_ptr() == ranks.data_ptr()
    assert torch.equal(out[:, 1].view(torch.int32), want_lp.view(torch.int32)) and torch.equal(ranks[:, 0], want_rk)
    assert bool((out[:, 0] == -5.0).all()) and bool((out[:, 2] == -5.0).all()) and bool((ranks[:, 1] == -9).all())
    out2 = torch.full((rows, 3), -5.0, device=DEV)
    lp, rk = PF.token_logprob(view, seq[:, 2], out2[:, 1], None)  # no rank asked for
    assert rk is None and torch.equal(out2, out)


@pytest.mark.parametrize("cols", [27, 257, 4097, 8193])
def test_targets_outside_the_vocabulary(native_lib, cols):
    rows = 6
    big = C.make_logits("normal", rows + 2, cols, 13).to(DEV)
    lg = big[1:-1]  # even a wrong read of row -1 or row `rows` would stay inside the tensor's storage
    t = C.make_targets("normal", rows, cols, 13)
    t[1], t[4] = cols, -1
    logprob, rank = _run(lg, t.to(DEV))
    ref_lp, ref_rank = PF.token_logprob_reference(lg.cpu(), t)
    assert bool(torch.isnan(logprob[[1, 4]]).all()) and rank[[1, 4]].tolist() == [-1, -1]
    assert bool(torch.isnan(ref_lp[[1, 4]]).all()) and ref_rank[[1, 4]].tolist() == [-1, -1]
    keep = [0, 2, 3, 5]
    assert torch.equal(rank.cpu().long()[keep], ref_rank[keep])
    err = (logprob.cpu().double()[keep] - ref_lp[keep]).abs()
    assert bool((err <= C.tolerance(cols, ref_lp[keep])).all())


def test_binding_refusals(native_lib):
    lg = torch.zeros(4, 8, device=DEV)
    t = torch.zeros(4, device=DEV, dtype=torch.int64)
    lp = torch.zeros(4, device=DEV)
    rk = torch.zeros(4, device=DEV, dtype=torch.int32)
    op = native_lib.token_logprob
    op(lg, t, lp, rk)
    op(lg, t, lp, None)
    bad = [
        (lg.double(), t, lp, rk), (lg.bfloat16(), t, lp, rk), (lg.cpu(), t, lp, rk),     # logits: dtype, device
        (lg, t.int(), lp, rk), (lg, t.cpu(), lp, rk),                                   # targets: dtype, device
        (lg, t, lp.double(), rk), (lg, t, lp, rk.long()), (lg, t, lp.cpu(), rk), (lg, t, lp, rk.cpu()),  # outputs
        (lg, t[:3], lp, rk), (lg, t, lp[:3], rk), (lg, t, lp, rk[:3]), (lg[:3], t, lp, rk),   # lengths
        (lg.t(), t.new_zeros(8), lp.new_zeros(8), rk.new_zeros(8)),                     # column stride 4
        (lg[:, ::2], t, lp, rk),                                                        # column stride 2
        (lg[:, :0], t, lp, rk),                                                         # no columns
        (lg[0], t[:1], lp[:1], rk[:1]), (lg, t.view(2, 2), lp, rk),                     # dimensions
    ]
    if torch.cuda.device_count() > 1:
        bad.append((lg, t.to("cuda:1"), lp, rk))
        bad.append((lg, t, lp.to("cuda:1"), rk))
    for args in bad:
        with pytest.raises((RuntimeError, NotImplementedError)):
            op(*args)
    torch.cuda.synchronize()
    before = lp.clone()
    op(lg[:0], t[:0], lp[:0], rk[:0])  # no rows: no launch
    op(lg[:0], t[:0], lp[:0], None)
    assert torch.equal(lp, before)
