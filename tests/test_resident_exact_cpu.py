"""The inputs of tests/test_resident_exact_gpu.py checked without a GPU (tests/resident_cases.py): every
case plans, the cases reach every way ``pz::generate_resident`` spreads a linear stage over its threads
(conditions on the inputs: they fail here when an edit of the case list loses one), the exactness
conditions of the reference hold, and the reference is a plain forward."""
import pytest
import torch

from penr_oz_neural_network_torch_amd.engine.resident import RESIDENT_LDS_BYTES, RESIDENT_MAX_VOCAB
from tests import resident_cases as C

NAMES = list(C.CASES)
WINDOWS = 64


def _windows(case, seed=5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = torch.randint(0, case.vocab, (WINDOWS, case.L), generator=g)
    w[:4, 0] = -1  # (a row of zeros is an input like any other)
    return w


# ---------------------------------------------------------------------------------------------
# planning
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(C.DTYPES))
@pytest.mark.parametrize("name", NAMES)
def test_every_case_plans_with_the_table_where_the_tests_expect_it(name, dtype):
    plans = C.plans(C.CASES[name], dtype)
    assert set(plans) == ({"lean"} if (name, dtype) in C.TABLE_GLOBAL else {"lds", "lean"})
    assert not plans["lean"].table_in_lds and ("lds" not in plans or plans["lds"].table_in_lds)
    assert all(p.total <= RESIDENT_LDS_BYTES for p in plans.values())
    assert sorted((n, d, p) for n, d, p in C.placements() if (n, d) == (name, dtype)) == sorted((name, dtype, p) for p in plans)


def test_the_issues_table_of_cases_is_all_there():
    want = {"one": (1, 1, 1), "ragged": (1, 11, 5), "tinyK": (1, 70, 1), "k3": (3, 13, 1), "s2": (2, 130, 7),
            "edges": (2, 257, 3), "positions": (8, 31, 3), "wide_p": (6, 40, 4), "vmax": (2, 8192, 1)}
    assert {n: (c.L, c.vocab, c.E) for n, c in C.CASES.items() if n in want} == want
    assert all(c.V <= c.vocab for c in C.CASES.values())  # (a sampled id is fed back)
    assert C.CASES["edges"].wmax == 1 and all(c.wmax == 2 for n, c in C.CASES.items() if n != "edges")


# ---------------------------------------------------------------------------------------------
# the regimes of the kernel's linear stage
# ---------------------------------------------------------------------------------------------
def test_regimes_restates_the_kernels_rule():
    assert C.regimes(1, 5, 64) == ("split", 64, 4, 2, [(0, 2), (2, 4), (4, 5), (5, 5)])
    assert C.regimes(1, 1, 1) == ("split", 64, 4, 1, [(0, 1), (1, 1), (1, 1), (1, 1)])
    assert C.regimes(1, 2, 70) == ("split", 128, 2, 1, [(0, 1), (1, 2)])
    assert C.regimes(1, 65, 128) == ("split", 128, 2, 33, [(0, 33), (33, 65)])
    assert C.regimes(1, 6, 192) == ("split", 192, 1, 6, [(0, 6)])
    assert C.regimes(1, 8, 255) == ("split", 256, 1, 8, [(0, 8)])
    assert C.regimes(1, 8, 256) == ("loop", 256, 0) and C.regimes(1, 4, 257) == ("loop", 257, 1)
    assert C.regimes(6, 4, 50) == ("loop", 300, 44) and C.regimes(8, 3, 5)[:3] == ("split", 64, 4)
    for P, K, N in [(1, 1, 1), (1, 5, 64), (3, 33, 7), (2, 65, 100), (1, 1000, 255), (5, 7, 51)]:
        _, opad, S, kc, ranges = C.regimes(P, K, N)
        assert S * opad <= 256 and opad >= P * N and len(ranges) == S  # (the partial sums fit their 256 floats)
        assert ranges[0][0] == 0 and ranges[-1][1] == K and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))


def test_the_cases_reach_every_regime():
    stages = [(name,) + r for name, c in C.CASES.items() for r in C.case_regimes(c)]
    split = [(name, p, k, n, bias, reg) for name, p, k, n, bias, reg in stages if reg[0] == "split"]
    loop = [(name, p, k, n, bias, reg) for name, p, k, n, bias, reg in stages if reg[0] == "loop"]
    assert {(reg[1], reg[2]) for *_, reg in split} >= {(64, 4), (128, 2), (192, 1), (256, 1)}
    assert any(k0 == k1 for *_, reg in split for k0, k1 in reg[4]), "no empty K group"
    assert any(reg[2] > 1 and 0 < reg[4][-1][1] - reg[4][-1][0] < reg[3] for *_, reg in split), "no ragged last group"
    assert any(k < reg[2] for _, p, k, n, _, reg in split), "no K below the number of groups"
    assert any(p > 1 for _, p, *_ in split), "no split stage over several positions"
    assert any(p > 1 and reg[2] > 1 for _, p, k, n, _, reg in split) and any(p > 1 and reg[2] == 1 for _, p, k, n, _, reg in split)
    assert any(reg[2] == 0 for *_, reg in loop) and any(reg[2] > 0 for *_, reg in loop), "loop stages: with and without a tail"
    assert any(p > 1 and n < 256 and reg[1] > 256 for _, p, k, n, _, reg in loop), "no loop stage whose o / N crosses positions"
    assert {p * n for _, p, k, n, *_ in stages} >= {64, 192, 255, 256, 257}
    assert any(not bias for *_, bias, _ in stages) and any(bias for *_, bias, _ in stages)
    # both buffer parities: a case with an even and one with an odd number of hidden linear stages
    hidden = {len(C.case_regimes(c)) - 1 for c in C.CASES.values()}
    assert any(h % 2 for h in hidden) and any(h and h % 2 == 0 for h in hidden) and max(hidden) >= 6


def test_the_cases_reach_the_other_edges():
    shapes = [s for c in C.CASES.values() for s in C.case_shapes(c)]
    assert any(kind == "bn" and p > 1 for kind, p, *_ in shapes), "no batchnorm over several positions"
    assert any(kind == "bn" and st.act == C.RELU for kind, *_, st in shapes) and any(kind == "bn" and st.act == C.NONE for kind, *_, st in shapes)
    assert any(c.V == RESIDENT_MAX_VOCAB for c in C.CASES.values()) and any(c.V == 1 for c in C.CASES.values())
    assert any(c.L > 1 and not any(s.kind == "flatten" for s in c.body[:1]) for c in C.CASES.values())
    for values in map(C.make_params, NAMES):  # every batchnorm scale occurs
        for (_, role), t in values.items():
            if role == "var":
                assert set((t + C.BN_EPS).tolist()) == {0.25, 1.0, 4.0}
            if role == "gain":
                assert set(t.abs().tolist()) == {0.5, 1.0, 2.0}


@pytest.mark.parametrize("dtype", list(C.DTYPES))
@pytest.mark.parametrize("name", ["vmax", "tinyK", "k3"])
def test_rows_with_tied_maxima_exist_where_the_token_tests_count_on_them(name, dtype):
    """On the very contexts the GPU tests generate from: at some step of the reference's greedy run a
    row's maximum sits in two columns or more, so "the lowest index wins" is put to the test."""
    case = C.CASES[name]
    _, logits = C.greedy_tokens(case, dtype, C.contexts(case), case.steps)
    tied = ((logits == logits.max(-1, keepdim=True).values).sum(-1) > 1)
    assert bool(tied.any()), "no tie"
    if name == "vmax":  # about 9 distinct values in 8192 columns
        assert bool(tied.all()) and max(len(set(r.tolist())) for r in logits.reshape(-1, case.V)[:8]) < 32


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", list(C.DTYPES))
@pytest.mark.parametrize("name", NAMES)
def test_exactness_conditions_hold_and_fp32_rounds_nothing(name, dtype):
    case, params = C.CASES[name], C.make_params(name)
    windows = _windows(case)
    ref = C.reference_logits(case, params, windows, dtype)  # (asserts its conditions)
    assert ref.shape == (WINDOWS, case.V) and torch.equal(ref.float().double(), ref) and torch.isfinite(ref).all()
    assert torch.equal(ref * 4, (ref * 4).round())
    plain = C.plain_logits(case, params, windows)
    if dtype == "float32":
        assert torch.equal(ref, plain)
    else:
        assert torch.equal(C.reference_logits(case, params, windows, dtype, rounded=False), plain)


def test_the_reference_refuses_inputs_it_cannot_be_exact_on():
    case = C.CASES["ragged"]
    windows = _windows(case)
    for key, value in [((1, "weights"), 0.125), ((0, "table"), 0.3), ((1, "weights"), 2.0 ** 22)]:
        bad = dict(C.make_params("ragged"))
        bad[key] = bad[key].clone()
        bad[key].reshape(-1)[0] = value
        with pytest.raises(AssertionError):
            C.reference_logits(case, bad, windows, "float32")


def test_bf16_rounds_hidden_values_in_some_case():
    """The one-rounding-per-hidden-stage rule is put to the test: in bf16 some cases' hidden values exceed
    8 bits, so their logits differ from the unrounded forward."""
    differs = [n for n in NAMES if not torch.equal(C.reference_logits(C.CASES[n], C.make_params(n), _windows(C.CASES[n]), "bfloat16"),
                                                   C.plain_logits(C.CASES[n], C.make_params(n), _windows(C.CASES[n])))]
    assert {"s2", "edges", "wide_p"} <= set(differs)


# which cases must expose which slip, by their shapes: drop_k / repeat_k need a stage of two K groups or more,
# bias_o and bn_channel a stage over several positions, no_round hidden values beyond bf16's 8 bits, loop_tail a
# strided loop with a tail, no_swap two hidden linear stages
EXPOSES = {
    "drop_k": {"ragged", "tinyK", "k3", "s2", "edges", "positions", "wide_p", "vmax"},
    "repeat_k": {"ragged", "tinyK", "k3", "s2", "edges", "positions", "wide_p", "vmax"},
    "bias_o": {"positions", "wide_p"},
    "bn_channel": {"positions", "wide_p"},
    "no_round": {"s2", "edges", "wide_p"},
    "loop_tail": {"edges", "wide_p"},
    "no_swap": {"tinyK", "s2", "edges", "positions", "wide_p"},
}


@pytest.mark.parametrize("dtype", list(C.DTYPES))
def test_the_kernels_indexing_restated_gives_the_reference_and_every_slip_shows(dtype):
    """``C.emulate_logits`` walks the kernel's index arithmetic (o = p N + n, the K groups, i % N, the buffer
    swaps) and equals the reference; each of its deliberate slips changes the logits of every case whose
    shapes reach it, so an exact comparison on these numbers cannot miss that slip in the kernel."""
    assert set(EXPOSES) == set(C.MUTANTS)
    shown = {m: set() for m in C.MUTANTS}
    for name in NAMES:
        case, params = C.CASES[name], C.make_params(name)
        windows = _windows(case)
        ref = C.reference_logits(case, params, windows, dtype)
        assert torch.equal(C.emulate_logits(case, params, windows, dtype), ref), name
        for m in C.MUTANTS:
            if not torch.equal(C.emulate_logits(case, params, windows, dtype, m), ref):
                shown[m].add(name)
    if dtype == "float32":  # (fp32 holds every hidden value of these cases: there is no rounding to leave out)
        assert not shown.pop("no_round")
    assert shown == {m: EXPOSES[m] for m in shown}


def test_wrap_ids():
    ids = torch.tensor([[0, 12, -1, -13, 13, -14, 99]])
    assert C.wrap_ids(ids, 13).tolist() == [[0, 12, 12, 0, -1, -1, -1]]


@pytest.mark.parametrize("dtype", list(C.DTYPES))
def test_the_stop_scenario_is_what_the_gpu_test_needs(dtype):
    ctx, stop, free, logits = C.stop_scenario(dtype)
    assert ctx.shape == (4, 3) and free.shape == (4, 600) and logits.shape == (4, 600, 13)
    assert int(free[0, 2]) == stop and stop not in free[0, :2].tolist()
    assert stop not in free[2].tolist()
    assert stop in free[3].tolist() and free[3].tolist().index(stop) > 2
