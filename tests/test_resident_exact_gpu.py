"""``pz::generate_resident`` (csrc/generate_resident.hip) at the op level, exactly: ``PF.generate_resident``
on hand-written plans and hand-made tensors (tests/resident_cases.py), no model. With integer-valued
parameters every fp32 partial sum of the kernel is exact in any order, so each step's logits must
equal, value for value, an fp64 forward with one rounding to the compute dtype per hidden stage
(``C.reference_logits``, which asserts the conditions that make this so). Teacher-forced: each step's
window is rebuilt from ``seq`` itself, the context and then the kernel's own tokens.

Which case reaches what (``C.regimes``; tests/test_resident_exact_cpu.py asserts the union):

    one        K = 1 < S = 4: ranges [0,1) and three empty groups; V = 1; vocab = 1
    ragged     O = 64 exactly (opad = 64, S = 4); K = 5: [0,2) [2,4) [4,5) [5,5); V = 9 under vocab = 11
    tinyK      K = 1 under S = 4; K = 33 in ranges of 9, 9, 9, 6; O = 70: opad = 128, S = 2, kc = 1; tied maxima
    k3         K = 3 and K = 7 under S = 4 (ranges of 1 / of 2, 2, 2, 1); a ring of 3; tied maxima
    s2         opad = 128, S = 2 at O = 65 and O = 128; odd K = 65 as [0,33) [33,65); O = 130: opad = 192, S = 1;
               a stage without bias; bf16 rounds hidden values
    edges      O = 192 (opad 192, S = 1), 255 (opad 256, S = 1), 256 (strided loop, no tail), 257 (loop, tail
               of 1); seven linear stages: the ping-pong buffers in both parities; bf16 rounds hidden values
    positions  split stages over P = 8 (S = 4) and P = 4 (opad = 192, S = 1): bias[n], not bias[o]; batchnorm
               with relu over 4 positions (i % N); a ring of 8; the embedding feeds a linear stage directly
    wide_p     the strided loop over P = 6, O = 300 (tail of 44, o / N crossing positions); batchnorm over 6
               positions; S = 2 with P = 2; bf16 rounds hidden values
    vmax       V = 8192 = kSampleNarrowCols in the strided loop; every row's maximum is tied; in fp32 the
               planner itself leaves the table in global memory (one placement only)

Tokens. With ``temperature = 0`` each token is the lowest index among the maxima of the *reference*
logits, which by induction fixes the whole sequence from the reference alone. With ``top_k = 1`` at
``T = 1`` the same holds wherever the maximum is unique; where it is tied the sampler's documented
rule keeps every tied column (``PF.sample_rows_reference``; tests/test_sample_gpu.py draws {7, 66} from
such a row) and draws among them, so there the token must be one of the maxima and equal what
``PF.sample_rows`` draws from the reference logits with the same key. The sampling modes are checked as
tests/test_generate_resident_gpu.py does, against ``PF.sample_rows`` on ``logits_out``.

The one real-valued stage (``test_one_real_valued_stage_stays_inside_the_fma_bound``): K = 16 fused
multiply-adds, the fold of the partial sums and one bias add in fp32 are bounded by
``(K + 2) 2^-24 (|x| |w| + |bias|)``; products of bf16 or fp32 operands inside an fma add no rounding.
The bound is derived, not measured. Largest observed |got - ref| / bound on an MI355X: 0.0757 in bf16
(largest error 1.222e-06), 0.0833 in fp32 (largest error 1.487e-06).

On an MI355X every comparison of this module held exactly as first written: the tests found no
fault in the kernel. What a slip in its indexing would do to these numbers is shown without a GPU by
``C.emulate_logits`` and its mutants (tests/test_resident_exact_cpu.py).
"""
import functools

import pytest
import torch

from penr_oz_neural_network_torch_amd.engine.resident import resident_plan
from penr_oz_neural_network_torch_amd.ops import functional as PF
from tests import resident_cases as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEY = (11, 22)
SENTINEL = -7
NAMES = list(C.CASES)
DTYPE_NAMES = list(C.DTYPES)


def _first_placement(name, dtype):
    return "lean" if (name, dtype) in C.TABLE_GLOBAL else "lds"


def _run(case, values, plan, dtype, ctx, steps, done=None, **kw):
    """One launch: ``(seq [rows, L + steps], done [rows], logits [rows, steps, V])`` on the host. The token
    columns of ``seq`` and all of ``logits_out`` start as SENTINEL."""
    rows = ctx.shape[0]
    seq = torch.full((rows, case.L + steps), SENTINEL, dtype=torch.int64)
    seq[:, :case.L] = ctx
    seq = seq.to(DEV)
    flags = torch.zeros(rows, dtype=torch.int32) if done is None else torch.tensor(done, dtype=torch.int32)
    flags = flags.to(DEV)
    logits = torch.full((rows, steps, case.V), float(SENTINEL), device=DEV, dtype=torch.float32)
    kw.setdefault("seed", KEY)
    PF.generate_resident(seq, flags, C.param_tensors(values, plan, dtype, DEV), plan.ints, steps, logits_out=logits, **kw)
    return seq.cpu(), flags.cpu(), logits.cpu()


def _launch(name, dtype, placement, ctx=None, steps=None, **kw):
    case = C.CASES[name]
    ctx = C.contexts(case) if ctx is None else ctx
    return _run(case, C.make_params(name), C.plans(case, dtype)[placement], dtype, ctx, steps or case.steps, **kw)


@functools.lru_cache(maxsize=None)
def _standard(name, dtype, placement):
    """The launch most tests share: 4 rows of ``C.contexts``, ``case.steps`` steps, T = 0.8. Not to be modified."""
    return _launch(name, dtype, placement, temperature=0.8)


def _reference_of_seq(case, values, dtype, seq, steps):
    """fp64 reference logits [rows, steps, V] of the windows of ``seq``: step s reads ``seq[:, s:s + L]``."""
    rows = seq.shape[0]
    windows = seq.unfold(1, case.L, 1)[:, :steps].reshape(rows * steps, case.L)
    return C.reference_logits(case, values, C.wrap_ids(windows, case.vocab), dtype).reshape(rows, steps, case.V)


def _assert_exact(got, ref64, what=""):
    """By value (-0 equals +0), against a reference that fp32 holds."""
    assert torch.isfinite(got).all()
    assert torch.equal(ref64.float().double(), ref64), "the reference is not exact in fp32"
    want = ref64.float()
    if not torch.equal(got, want):
        bad = got != want
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} logits differ; first at {i}: {got[i].item()} != {want[i].item()}")


def _assert_tokens_in_range(case, seq):
    tokens = seq[:, case.L:]
    assert int(tokens.min()) >= 0 and int(tokens.max()) < case.V


def _bits(t):
    return t.view(torch.int32)


# ---------------------------------------------------------------------------------------------
# a. the logits are exact, teacher-forced
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dtype,placement", C.placements())
def test_logits_are_exactly_the_reference_teacher_forced(native_lib, name, dtype, placement):
    case = C.CASES[name]
    seq, done, logits = _standard(name, dtype, placement)
    assert torch.equal(seq[:, :case.L], C.contexts(case)) and not done.any()
    _assert_tokens_in_range(case, seq)
    _assert_exact(logits, _reference_of_seq(case, C.make_params(name), dtype, seq, case.steps), f"{name} {dtype} {placement}")


@pytest.mark.parametrize("name,dtype", [(n, d) for n in NAMES for d in DTYPE_NAMES if (n, d) not in C.TABLE_GLOBAL])
def test_the_two_table_placements_agree_bit_for_bit(native_lib, name, dtype):
    lds, lean = _standard(name, dtype, "lds"), _standard(name, dtype, "lean")
    assert torch.equal(lds[0], lean[0]) and torch.equal(_bits(lds[2]), _bits(lean[2]))


# ---------------------------------------------------------------------------------------------
# b. the tokens
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
@pytest.mark.parametrize("name", NAMES)
def test_greedy_tokens_follow_from_the_reference_alone(native_lib, name, dtype):
    case = C.CASES[name]
    want, want_logits = C.greedy_tokens(case, dtype, C.contexts(case), case.steps)
    for placement in C.plans(case, dtype):
        seq, _, logits = _launch(name, dtype, placement, temperature=0.0)
        assert torch.equal(seq[:, case.L:], want), (name, dtype, placement)
        _assert_exact(logits, want_logits, f"{name} {dtype} {placement}")


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
@pytest.mark.parametrize("name", NAMES)
def test_top_1_tokens_follow_from_the_reference_alone(native_lib, name, dtype):
    """``top_k = 1`` at T = 1: the lowest index among the maxima of the reference logits where the maximum is
    unique; among tied maxima (all kept, by the sampler's rule) what ``PF.sample_rows`` draws from the
    reference logits. Either way the sequence is fixed before the kernel under test runs."""
    case, values = C.CASES[name], C.make_params(name)
    ctx, steps = C.contexts(case), case.steps
    want = torch.cat([ctx, torch.zeros(4, steps, dtype=torch.int64)], dim=1)
    drawn = torch.full((4, steps), SENTINEL, device=DEV, dtype=torch.int64)
    flags = torch.zeros(4, device=DEV, dtype=torch.int32)
    unique_steps = tied_steps = 0
    for s in range(steps):
        ref = C.reference_logits(case, values, C.wrap_ids(want[:, s:s + case.L], case.vocab), dtype)
        assert torch.equal(ref.float().double(), ref)
        PF.sample_rows(ref.float().to(DEV), drawn, flags, s, seed=KEY, step=s, temperature=1.0, top_k=1)
        token = drawn[:, s].cpu()
        is_max = ref == ref.max(-1, keepdim=True).values
        assert bool(is_max.gather(1, token.unsqueeze(1)).all()), f"step {s}: a token that is no maximum"
        unique = is_max.sum(-1) == 1
        assert torch.equal(token[unique], C.lowest_argmax(ref)[unique])
        unique_steps, tied_steps = unique_steps + int(unique.sum()), tied_steps + int((~unique).sum())
        want[:, case.L + s] = token
    print(f"\n[resident top-1] {name} {dtype}: {unique_steps} draws at a unique maximum, {tied_steps} among tied maxima")
    seq, _, _ = _launch(name, dtype, _first_placement(name, dtype), temperature=1.0, top_k=1)
    assert torch.equal(seq, want)


MODES = {"t0.8": dict(temperature=0.8), "top7": dict(temperature=1.0, top_k=7), "top_p": dict(temperature=1.0, top_p=0.8),
         "all": dict(temperature=1.0, top_p=0.8, top_k=5, min_p=0.05)}


@pytest.mark.parametrize("dtype", DTYPE_NAMES)
@pytest.mark.parametrize("name", NAMES)
def test_sampled_tokens_are_what_sample_rows_draws_from_logits_out(native_lib, name, dtype):
    case = C.CASES[name]
    for mode, kw in MODES.items():
        if mode == "t0.8":
            seq, _, logits = _standard(name, dtype, _first_placement(name, dtype))
        else:
            seq, _, logits = _launch(name, dtype, _first_placement(name, dtype), **kw)
        _assert_tokens_in_range(case, seq)
        buf = logits.to(DEV)
        drawn = torch.full((4, case.steps), SENTINEL, device=DEV, dtype=torch.int64)
        flags = torch.zeros(4, device=DEV, dtype=torch.int32)
        for s in range(case.steps):
            PF.sample_rows(buf[:, s].contiguous(), drawn, flags, s, seed=KEY, step=s, **kw)
        assert torch.equal(seq[:, case.L:], drawn.cpu()), (name, dtype, mode)
        # (and these logits are the reference's too, whatever the mode)
        _assert_exact(logits, _reference_of_seq(case, C.make_params(name), dtype, seq, case.steps), f"{name} {dtype} {mode}")


# ---------------------------------------------------------------------------------------------
# c. ids
# ---------------------------------------------------------------------------------------------
ID_CASES = [(n, d, p) for n, d, p in C.placements() if n in ("ragged", "k3", "s2", "positions")]


@pytest.mark.parametrize("name,dtype,placement", ID_CASES)
def test_negative_ids_count_from_the_end(native_lib, name, dtype, placement):
    case = C.CASES[name]
    ctx = C.contexts(case)
    negative = ctx.clone()
    negative.view(-1)[::2] -= case.vocab  # every other id in its negative form, -vocab (id 0) included
    assert int(negative.min()) >= -case.vocab and bool((negative < 0).any())
    want_seq, _, want_logits = _standard(name, dtype, placement)
    seq, _, logits = _launch(name, dtype, placement, ctx=negative, temperature=0.8)
    assert torch.equal(seq[:, :case.L], negative)  # (the context stays as given)
    assert torch.equal(seq[:, case.L:], want_seq[:, case.L:]) and torch.equal(_bits(logits), _bits(want_logits))


@pytest.mark.parametrize("name,dtype,placement", ID_CASES)
def test_an_id_outside_the_table_reads_as_a_row_of_zeros(native_lib, name, dtype, placement):
    """The binding does not look at ids and the kernel guards the read: ``vocab`` and ``-vocab - 1``, the
    nearest ids outside, give exactly the reference with a zero embedding row, for as long as they stay in the
    window."""
    case = C.CASES[name]
    ctx = C.contexts(case, seed=1)
    ctx[0, 0] = case.vocab
    ctx[1, -1] = -case.vocab - 1
    ctx[2, :] = case.vocab
    ctx[2, ::2] = -case.vocab - 1
    seq, done, logits = _launch(name, dtype, placement, ctx=ctx, temperature=0.8)
    assert torch.equal(seq[:, :case.L], ctx) and not done.any()
    _assert_tokens_in_range(case, seq)
    _assert_exact(logits, _reference_of_seq(case, C.make_params(name), dtype, seq, case.steps), f"{name} {dtype} {placement}")


# ---------------------------------------------------------------------------------------------
# d. stop and done over more than 256 steps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_stop_and_done_fill_600_steps_and_leave_unrun_logits_untouched(native_lib, dtype):
    steps = 600
    case = C.CASES["k3"]
    ctx, stop, free, free_logits = C.stop_scenario(dtype, steps)
    seq, done, logits = _launch("k3", dtype, "lds", ctx=ctx, steps=steps, done=[0, 1, 0, 0], temperature=0.0, stop_token=stop)
    tokens = seq[:, case.L:]
    assert torch.equal(seq[:, :case.L], ctx)
    assert not bool((tokens == SENTINEL).any())
    # row 1 arrived done
    assert tokens[1].tolist() == [stop] * steps and bool((logits[1] == SENTINEL).all()) and int(done[1]) == 1
    # row 0 draws the stop token at step 2
    assert tokens[0].tolist() == free[0, :3].tolist() + [stop] * (steps - 3) and int(done[0]) == 1
    _assert_exact(logits[0, :3], free_logits[0, :3], "row 0")
    assert bool((logits[0, 3:] == SENTINEL).all())
    # row 2 never draws it
    assert torch.equal(tokens[2], free[2]) and int(done[2]) == 0 and stop not in tokens[2].tolist()
    _assert_exact(logits[2], free_logits[2], "row 2")
    # row 3 draws it later, past step 2
    at = free[3].tolist().index(stop)
    assert tokens[3].tolist() == free[3, :at + 1].tolist() + [stop] * (steps - 1 - at) and int(done[3]) == 1
    _assert_exact(logits[3, :at + 1], free_logits[3, :at + 1], "row 3")
    assert bool((logits[3, at + 1:] == SENTINEL).all())
    # without a stop token nothing is cut, and the flags of rows that are not done stay
    seq, done, logits = _launch("k3", dtype, "lds", ctx=ctx, steps=steps, temperature=0.0)
    assert torch.equal(seq[:, case.L:], free) and not done.any()
    _assert_exact(logits, free_logits, "free run")


# ---------------------------------------------------------------------------------------------
# e. rows and row0
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
@pytest.mark.parametrize("name", NAMES)
def test_row0_shifts_the_rows_and_two_launches_are_bit_identical(native_lib, name, dtype):
    case, placement = C.CASES[name], _first_placement(name, dtype)
    seq4, _, logits4 = _standard(name, dtype, placement)
    seq2, _, logits2 = _launch(name, dtype, placement, ctx=C.contexts(case)[2:], temperature=0.8, row0=2)
    assert torch.equal(seq2, seq4[2:]) and torch.equal(_bits(logits2), _bits(logits4[2:]))
    again, _, logits_again = _launch(name, dtype, placement, temperature=0.8)
    assert torch.equal(again, seq4) and torch.equal(_bits(logits_again), _bits(logits4))


# ---------------------------------------------------------------------------------------------
# f. one real-valued stage
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPE_NAMES)
def test_one_real_valued_stage_stays_inside_the_fma_bound(native_lib, dtype):
    case, values = C.REAL_CASE, C.real_params(dtype)
    plan = resident_plan(case.stages, dtype, case.L)
    assert not isinstance(plan, str), plan
    ctx = C.contexts(case, rows=4)
    seq, _, logits = _run(case, values, plan, dtype, ctx, case.steps, temperature=0.8)
    _assert_tokens_in_range(case, seq)
    windows = seq.unfold(1, case.L, 1)[:, :case.steps].reshape(-1, case.L)
    ref, magnitude = C.real_reference(values, windows, dtype)
    err = (logits.double().reshape(-1, case.V) - ref).abs()
    bound = (C.REAL_K + 2) * 2.0 ** -24 * magnitude
    ratio = float((err / bound).max())
    print(f"\n[resident real stage] {dtype}: largest |got - ref| / bound = {ratio:.4f} (largest error {float(err.max()):.3e})")
    assert bool((err <= bound).all())
