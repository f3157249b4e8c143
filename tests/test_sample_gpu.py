"""``pz::sample_rows`` (csrc/sample.hip) against ``PF.sample_rows_reference``, the same rule in fp64
with the same uniforms.

Tolerance of the inverse-CDF cases. The kernel sums fp32 weights in a fixed order whose longest
chain of dependent rounding additions is at most ``V / 64 + 16 <= 80`` for the shapes of the issue
(19 at V = 4099, 49 at V = 65536; the order is written out in sample.hip), so its normalised
prefix sums are within ``80 * 2^-24 = 4.8e-6`` of the exact ones; a few ulps of ``exp`` add about
``5e-7``. Rounded up: ``EPS = 1e-5``. A token passes if it is the fp64 reference's token, or if
``u`` lies within EPS of the fp64 CDF boundary between the two and the token is the reference
token's kept neighbour on the other side of it. At most 5 % of a case's draws may pass by the second
clause (the reference alone puts at most 2 % of these draws that close to a boundary), and every
token must be a kept column, with no tolerance."""
import math

import pytest
import torch

from penr_oz_neural_network_torch_amd.ops import functional as PF

pytestmark = pytest.mark.gpu

SEED = (11, 22)
EPS = 1e-5
DEV = "cuda:0"


def _logits(rows, cols, seed=0):
    return 2.0 * torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed))


def _draw(logits_dev, steps, temperature=1.0, top_k=None, stop_token=None, row0=0, done=None, first_step=0):
    """``steps`` kernel draws from the same logits: tokens [rows, steps] and the done flags (CPU)."""
    rows = logits_dev.shape[0]
    seq = torch.full((rows, steps), -7, device=DEV, dtype=torch.int64)
    done = torch.zeros(rows, device=DEV, dtype=torch.int32) if done is None else done.to(DEV)
    for s in range(steps):
        PF.sample_rows(logits_dev, seq, done, s, seed=SEED, step=first_step + s, temperature=temperature, top_k=top_k,
                       stop_token=stop_token, row0=row0)
    return seq.cpu(), done.cpu()


def _check_against_reference(lg, got, temperature, top_k):
    """Every draw of ``got [rows, steps]`` by the rule of the module docstring; returns the number that
    passed by the boundary clause."""
    rows, v = lg.shape
    l64 = lg.double()
    kept = torch.ones_like(l64, dtype=torch.bool)
    if top_k and top_k < v:
        kept = l64 >= torch.topk(l64, top_k, dim=-1).values[:, -1:]
    t32 = float(torch.tensor(temperature, dtype=torch.float32))
    w = torch.where(kept, torch.exp((l64 - l64.max(-1, keepdim=True).values) / t32), torch.zeros_like(l64))
    cdf = w.cumsum(-1) / w.sum(-1, keepdim=True)
    near = 0
    for s in range(got.shape[1]):
        ref = PF.sample_rows_reference(lg, SEED, s, temperature=temperature, top_k=top_k)
        assert bool(kept[torch.arange(rows), got[:, s]].all()), f"step {s}: a token outside the kept set"
        for r in (got[:, s] != ref).nonzero().flatten().tolist():
            t, want = int(got[r, s]), int(ref[r])
            lo, hi = min(t, want), max(t, want)
            assert not bool(kept[r, lo + 1:hi].any()), (s, r, t, want, "not the kept neighbour")
            u = PF.sample_uniform(SEED, r, s)
            assert abs(float(cdf[r, lo]) - u) <= EPS, (s, r, t, want, float(cdf[r, lo]), u)
            near += 1
    return near


@pytest.mark.parametrize("rows,cols,temperature,top_k", [
    (64, 27, 1.0, None), (64, 1000, 1.0, None), (64, 1000, 0.7, None), (64, 4099, 0.8, 50), (17, 1000, 1.0, 40),
    (8, 65536, 1.0, None), (8, 65536 + 77, 0.9, 100),  # 16 and 17 chunks per segment
    (4, 8192, 1.0, 7), (4, 8193, 1.0, 7),               # the last width on 4 waves, the first on 16
    (3, 1, 1.0, None), (3, 65, 1.3, 64),
])
def test_inverse_cdf_agrees_with_the_fp64_reference(native_lib, rows, cols, temperature, top_k):
    lg = _logits(rows, cols)
    got, _ = _draw(lg.to(DEV), 8, temperature=temperature, top_k=top_k)
    near = _check_against_reference(lg, got, temperature, top_k)
    print(f"V={cols} T={temperature} top_k={top_k}: {near} of {rows * 8} draws passed by the boundary clause")
    assert near <= 0.05 * rows * 8


@pytest.mark.parametrize("cols,tie", [(4099, (70, 4000)), (65536, (40000, 65000))])
def test_greedy_is_argmax_and_the_lowest_index_wins_a_tie(native_lib, cols, tie):
    lg = _logits(9, cols, seed=1)
    lg[4, tie[0]] = lg[4, tie[1]] = lg[4].max() + 1.0
    lg[5, 0] = lg[5, cols - 1] = lg[5].max() + 1.0
    got, _ = _draw(lg.to(DEV), 2, temperature=0.0)
    assert got[:, 0].tolist() == got[:, 1].tolist()  # no random number is involved
    assert torch.equal(lg.gather(1, got[:, :1])[:, 0], lg.max(-1).values)
    assert got[4, 0] == tie[0] and got[5, 0] == 0
    assert all(int(got[r, 0]) == int(lg[r].argmax()) for r in (0, 1, 2, 3, 6, 7, 8))
    assert got[:, 0].tolist() == PF.sample_rows_reference(lg, SEED, 0, temperature=0.0).tolist()
    # top_k does not change a greedy draw
    assert _draw(lg.to(DEV), 1, temperature=0.0, top_k=3)[0][:, 0].tolist() == got[:, 0].tolist()


def test_top_k_keeps_ties_at_the_threshold_and_nothing_below(native_lib):
    row = _logits(1, 1000, seed=2)[0].clamp(max=4.0)
    for c, val in [(3, 10.0), (999, 9.0), (64, 8.0), (500, 7.0), (130, 6.0), (770, 6.0), (20, 5.5)]:
        row[c] = val  # k = 5: the 5th and the 6th largest are both 6.0
    lg = row.repeat(4096, 1).to(DEV)
    got, _ = _draw(lg, 1, temperature=50.0, top_k=5)
    assert set(got[:, 0].tolist()) == {3, 999, 64, 500, 130, 770}
    got, _ = _draw(lg, 1, temperature=50.0, top_k=6)
    assert set(got[:, 0].tolist()) == {3, 999, 64, 500, 130, 770}
    got, _ = _draw(lg, 1, temperature=50.0, top_k=7)
    assert set(got[:, 0].tolist()) == {3, 999, 64, 500, 130, 770, 20}
    got, _ = _draw(lg, 1, temperature=50.0, top_k=1)
    assert set(got[:, 0].tolist()) == {3}
    # negative logits and signed zeros order like floats (-0 == +0 is a tie)
    neg = torch.full((1, 70), -5.0)
    neg[0, 7], neg[0, 66], neg[0, 30] = 0.0, -0.0, -1.0
    got, _ = _draw(neg.repeat(512, 1).to(DEV), 1, temperature=50.0, top_k=1)
    assert set(got[:, 0].tolist()) == {7, 66}


def test_draws_follow_the_distribution(native_lib):
    n = 16384
    one = _logits(1, 27, seed=3)
    p = one[0].double().softmax(0)
    got, _ = _draw(one.repeat(n, 1).to(DEV), 1)
    counts = torch.bincount(got[:, 0], minlength=27).double()
    assert counts.sum() == n
    for c in range(27):
        if p[c] >= 1e-3:
            assert abs(counts[c] - n * p[c]) <= 5.0 * math.sqrt(n * p[c] * (1 - p[c])), (c, counts[c], n * p[c])


def test_reproducible_and_independent_of_the_other_rows(native_lib):
    lg = _logits(64, 1000, seed=4)
    dev = lg.to(DEV)
    a, _ = _draw(dev, 4, temperature=0.9, top_k=300)
    b, _ = _draw(dev, 4, temperature=0.9, top_k=300)
    assert torch.equal(a, b)
    for r in range(64):  # the same logits sent alone, as row r of the request
        alone, _ = _draw(dev[r:r + 1].contiguous(), 4, temperature=0.9, top_k=300, row0=r)
        assert alone[0].tolist() == a[r].tolist(), r
    assert any(a[:, 0].tolist() != a[:, s].tolist() for s in range(1, 4))  # another step: other draws
    shifted, _ = _draw(dev, 1, temperature=0.9, top_k=300, first_step=1)
    assert shifted[:, 0].tolist() == a[:, 1].tolist()  # the step names the draw, not the column written


def test_stop_token_sets_done_and_done_rows_repeat_it(native_lib):
    lg = _logits(64, 27, seed=5)
    dev = lg.to(DEV)
    free, _ = _draw(dev, 2)
    stop = int(free[0, 0])
    got, done = _draw(dev, 2, stop_token=stop)
    assert got[:, 0].tolist() == free[:, 0].tolist()
    hit = free[:, 0] == stop
    assert hit.any() and not hit.all()
    assert torch.equal(got[hit, 1], torch.full_like(got[hit, 1], stop))      # done rows write the stop token
    assert torch.equal(got[~hit, 1], free[~hit, 1])                           # the others are untouched by them
    assert done.bool().tolist() == (hit | (free[:, 1] == stop)).tolist()      # set on the step that draws it
    preset = torch.zeros(64, dtype=torch.int32)
    preset[9] = 1
    got, done = _draw(dev, 1, stop_token=stop, done=preset)
    assert got[9, 0] == stop and done[9] == 1
    assert [t for r, t in enumerate(got[:, 0].tolist()) if r != 9] == [t for r, t in enumerate(free[:, 0].tolist()) if r != 9]
    _, done = _draw(dev, 2)  # no stop token: nothing is ever done
    assert not done.any()


def test_the_op_refuses_what_it_cannot_take(native_lib):
    lg = _logits(4, 27).to(DEV)
    seq = torch.zeros(4, 6, device=DEV, dtype=torch.int64)
    done = torch.zeros(4, device=DEV, dtype=torch.int32)
    ok = dict(seed=SEED, step=0)
    PF.sample_rows(lg, seq, done, 5, **ok)
    with pytest.raises(RuntimeError):
        PF.sample_rows(lg.bfloat16(), seq, done, 0, **ok)
    with pytest.raises(RuntimeError):
        PF.sample_rows(lg.t().contiguous().t(), seq, done, 0, **ok)
    with pytest.raises(RuntimeError):
        PF.sample_rows(lg, torch.zeros(4, 12, device=DEV, dtype=torch.int64)[:, ::2], done, 0, **ok)
    with pytest.raises(RuntimeError):
        PF.sample_rows(lg, seq.int(), done, 0, **ok)
    for pos in (6, -1):
        with pytest.raises(RuntimeError):
            PF.sample_rows(lg, seq, done, pos, **ok)
    with pytest.raises(RuntimeError):
        PF.sample_rows(lg, seq, done, 0, temperature=-0.1, **ok)
    with pytest.raises(RuntimeError):
        PF.sample_rows(lg, seq, done, 0, temperature=float("nan"), **ok)
    torch.cuda.synchronize()
    assert seq[:, :5].abs().sum() == 0  # the refused calls wrote nothing
